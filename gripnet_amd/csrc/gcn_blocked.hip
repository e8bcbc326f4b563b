// GCN-style layer with the neighbour features staged through LDS (column-blocked gather).
//
//   out[i, :] = act( sum_{e: dst(e)=i} norm_e (x W)[src(e), :] + b ),  norm_e = dis[src] w_e dis[dst]
//                                                                     (gripnet/layers.py:52-100)
//
// The wave-per-destination-row kernels (aggregate.cuh) ask the L2 for one neighbour row per edge and sit at the rate
// of the per-CU miss path (~64 lines in flight per CU: 0.15 random rows per clock whatever the row width).  Here the
// gathered table never leaves a CU once it is there.  For graphs whose stored weights are all 1 (GripNet passes
// edge_weight = ones or None, GripNet-pose.py:52,117-120) the coefficient factorises, norm_e = dis[src] dis[dst]:
//
//   out[i, :] = act( dis[i] * sum_{e: dst=i} T[src(e), :] + b ),      T[s, :] = dis[s] * (x W)[s, :]
//
// and an edge is a 16-bit source id, not a column index and a coefficient.  Two launches per layer:
//   k_col_transform  T = dis * (x W), exact fp32, written column-group-major: [out / CW][rows][CW], CW = 2 (or 1)
//                    columns per group, so that the slice of ALL nodes for one column group is contiguous and fits
//                    the 160 KB of LDS of one CU (19,081 genes x 8 bytes = 153 KB);
//   k_col_gather     one workgroup per (column group, range of destination rows): its slice of T goes straight into
//                    LDS (LDS-DMA, 1 KB per wave instruction), then a quad of lanes per destination row adds the
//                    CW-float entries its ids name - one ds_read_b64 per lane and edge - and writes its CW columns
//                    of the layer's slot of the concat buffer, scaled, biased, activated.  No partial sums cross
//                    workgroups: nothing to combine, nothing written but the result.
// The plan orders every row's edges so that the 32 lanes of a ds_read_b64 access group read 32 different bank pairs
// wherever the graph allows it (the order of addends is free), sorts the destination rows of a range by degree so
// that the 16 rows of a tile finish together, and deals the rows to the ranges so that every range holds the same
// number of edges.  Fixed summation order, no atomics: bitwise reproducible.
// Eight column groups x 32 ranges = 256 workgroups for 16 output columns.  Applies while one column group of all nodes
// fits the LDS: N <= ~19,900 nodes at CW = 2, ~39,800 at CW = 1; larger tables stay on the wave-per-row kernels.
// (Measured on the way, pose0-syn: source blocks of whole 16-float rows with per-block partial sums and a combine
// launch took 3.8 + 11.2 + 5.5 us per layer - the 10 MB of partial sums are flushed at one kernel boundary and read back
// behind the next - against 19.2 / 14.7 us for the wave-per-row kernels.)
#include "aggregate.cuh"
#include "dpp.cuh"
#include "layout_blocked.hpp"

#include <algorithm>
#include <numeric>
#include <vector>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#ifndef GN_COL_THREADS
#define GN_COL_THREADS 1024
#endif
constexpr int kColThreads = GN_COL_THREADS;
constexpr int kColWaves = kColThreads / 64;
static_assert(kColWaves == gn_layout::kColLayoutWaves, "the plan cuts a range's tiles into the waves of one workgroup");
constexpr size_t kColLdsBytes = 160 * 1024;
constexpr int kColSlack = gn_layout::kColLayoutSlack;            // spare iterations behind the id stream: look-ahead loads never leave it
constexpr int kWaveInts = 12;            // per wave of a range: first tile, end tile, first iteration, end iteration, the ends of its first five tiles, 3 unused

bool blocked_disabled() { return gn::fast_paths_disabled() || gn::blocked_switched_off(); }

// ---- T = dis * (x W), column-group-major ---------------------------------------------------------------------------
// A quad of lanes per row: lane j holds the features 16 p + 4 j + c of its row (one contiguous 64-byte read per quad and
// 16 features), hands them round the quad with DPP and accumulates the output columns 16 nt + 4 j + c against W rows
// read from LDS (w == null: T = dis * x, FIN == 16 NT).
struct TransArgs {
    const float* x; int64_t ld_x;
    const float* w;                      // [FIN, 16 NT] or null
    const float* dis;                    // [rows_pad], zero beyond the last node
    float* table;                        // [16 NT / CW][rows_pad][CW]
    int n, rows_pad;
};

template <int CTRL>
__device__ __forceinline__ float quad_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true));
}

template <int FIN, int NT, int CW>
__global__ __launch_bounds__(256) void k_col_transform(TransArgs a) {
    constexpr int FOUT = 16 * NT, P = FIN / 16;           // 16-byte pieces of a row per lane
    __shared__ f32x4 wl[FIN * FOUT / 4];
    const int tid = threadIdx.x, lane = tid & 63, q = lane >> 2, j = lane & 3;
    const int tiles = a.rows_pad / 16;
    int t = blockIdx.x * 4 + (tid >> 6);
    f32x4 xv[P];
    float d = 0.f;
    auto load_row = [&](int tt) {                          // requested before W is staged: one round trip, not two
        const int row = 16 * min(tt, tiles - 1) + q, rowc = min(row, a.n - 1);
        const float* __restrict__ px = a.x + (int64_t)rowc * a.ld_x + 4 * j;
#pragma unroll
        for (int p = 0; p < P; ++p) xv[p] = *reinterpret_cast<const f32x4*>(px + 16 * p);
        d = a.dis[row];
    };
    load_row(t);
    if (a.w) {
        for (int i = tid; i < FIN * FOUT / 4; i += 256) wl[i] = reinterpret_cast<const f32x4*>(a.w)[i];
        __syncthreads();
    }
    for (; t < tiles; t += gridDim.x * 4) {
        const int row = 16 * t + q;
        f32x4 acc[NT];
        if (a.w == nullptr) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = xv[nt < P ? nt : 0];
        } else {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float v = xv[p][c];
                    const float v0 = quad_bcast<0x00>(v), v1 = quad_bcast<0x55>(v), v2 = quad_bcast<0xAA>(v), v3 = quad_bcast<0xFF>(v);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {       // lane jj of the quad holds feature 16 p + 4 jj + c
                        acc[nt] += v0 * wl[(16 * p + 0 + c) * (FOUT / 4) + 4 * nt + j];
                        acc[nt] += v1 * wl[(16 * p + 4 + c) * (FOUT / 4) + 4 * nt + j];
                        acc[nt] += v2 * wl[(16 * p + 8 + c) * (FOUT / 4) + 4 * nt + j];
                        acc[nt] += v3 * wl[(16 * p + 12 + c) * (FOUT / 4) + 4 * nt + j];
                    }
                }
        }
        const float scale = d;
        const bool real = row < a.n;                        // rows beyond the last node (the zero row among them) are exact zeros
        if (t + (int)gridDim.x * 4 < tiles) load_row(t + gridDim.x * 4);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const f32x4 v = real ? acc[nt] * scale : (f32x4){0.f, 0.f, 0.f, 0.f};     // columns 16 nt + 4 j .. + 3 = groups (16 nt + 4 j) / CW ..
            if constexpr (CW == 2) {
                float* o = a.table + ((size_t)(8 * nt + 2 * j) * a.rows_pad + row) * 2;
                *reinterpret_cast<f32x2*>(o) = (f32x2){v[0], v[1]};
                *reinterpret_cast<f32x2*>(o + (size_t)a.rows_pad * 2) = (f32x2){v[2], v[3]};
            } else {
                float* o = a.table + (size_t)(16 * nt + 4 * j) * a.rows_pad + row;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[(size_t)c * a.rows_pad] = v[c];
            }
        }
    }
}

// ---- the gather ------------------------------------------------------------------------------------------------------
struct ColArgs {
    const float* table;                  // [groups][rows_pad][CW]
    const int32_t* cell;                 // [ranges][waves][kWaveInts]
    const int32_t* tile_off;             // [tiles + 3] first iteration of every tile
    const int32_t* tile_rows;            // [tiles + 4][16] destination row of every quad (-1: none)
    const float* tile_dis;               // [tiles + 4][16] dis of that row
    const u32x2* ids;                    // per iteration 64 lanes x 4 uint16 source ids (512 bytes)
    const float* dis; const float* bias;
    float* out; int64_t ld_out;
    int n, rows_pad, groups, ranges, relu;
    int per_x, group_shift;              // ranges per XCD, ceil(ranges / 8); log2(groups): groups is a power of two
    gn_side_copy side;
    float* next_table;                   // k_col_gather_next: the next layer's table, [groups][rows_pad][CW] (see col_gather)
};

#ifdef GN_STAMPS
// Diagnostic build only (make STAMPS=1): per-workgroup phase times, never part of the product library.
__device__ unsigned long long g_blk_stamps[2][512][4];
#endif

// NEXT: the workgroup that owns (column group, destination rows) also writes dis[row] * r, r = what it stores to `out`,
// into ITS cells of next_table: the table T' = dis * h of a following layer over the same graph whose transform is applied
// behind that layer's sum instead of in front of it, (A h) W = A (h W) (gn_graph_aggregate_chain_f32).  Column-local: no
// workgroup waits for another, the kernel boundary that follows hands the table over.
// STAGED: a finished tile's folded sums are parked in LDS behind the table (slot (tile - first tile of the range) * 16 +
// quad, CW floats) and the wave writes all its rows behind its loop.  Loads and stores share the in-order vmcnt: with a
// store inside the loop every wait for a later load (the ids, the next tile's row and scale) also waited for that store's
// acknowledgement from L2.  The staged loop has no vector-memory instruction but the id stream's own loads.  Plans whose
// ranges hold more tiles than fit behind the table run the direct-store loop (blocked_gather decides per launch).
// acc * d + bias with the rounding spelled out, so that the staged write-out and the direct loop cannot drift apart with the
// compiler's contraction choices: one FMA per column for two columns (what the layer has always computed there: v_pk_fma_f32),
// a product rounded on its own and a sum for one column (likewise: v_mul_f32, v_add_f32)
template <int CW, typename V>
__device__ __forceinline__ V scale_bias(V acc, float d, V bias) {
    V r;
    if constexpr (CW == 2) {
#pragma unroll
        for (int c = 0; c < CW; ++c) r[c] = __builtin_fmaf(acc[c], d, bias[c]);
    } else {
#pragma clang fp contract(off)
        const float p = acc[0] * d;
        r[0] = p + bias[0];
    }
    return r;
}

template <int CW, bool NEXT, bool STAGED>
__device__ __forceinline__ void col_gather(const ColArgs& a, int stamp_set) {
    typedef float vec_t __attribute__((ext_vector_type(CW)));
    extern __shared__ f32x4 lds4[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 2, j = lane & 3;
    // Workgroups go to the eight XCDs round-robin and every XCD has its own L2: the column groups of one range sit on
    // one XCD (its id stream is fetched into one L2), and each XCD sees every column group.
    // (per_x = ceil(ranges / 8) and log2(groups) come with the arguments: the generic division by `groups` stood, with a
    // second fetch of arguments behind it, in front of the first request.  A workgroup without a range - ranges no multiple
    // of eight - takes the same path with nothing to fill, gather or write: an early way out for it split the argument
    // loads over two blocks, and every workgroup waited for them twice.)
    const int wg = blockIdx.x;
    const int x = wg & 7, k = wg >> 3;
    const int range = x * a.per_x + (k >> a.group_shift), cg = k & (a.groups - 1);
    const bool live = range < a.ranges;
#ifdef GN_STAMPS
    const unsigned long long st0 = __builtin_amdgcn_s_memrealtime();
#endif
    // ---- this wave's tiles [c0, c1): read with scalar loads BEFORE the first vector-memory instruction (behind the
    //      DMA loads the compiler would make them vector loads, and those return in issue order: behind the table) ----
    //      (a workgroup without a range reads the record behind the last range's: no tiles, no iterations)
    const int my_range = live ? range : a.ranges;
    const int32_t* __restrict__ cell = a.cell + ((size_t)my_range * kColWaves + wave) * kWaveInts;
    const int c0 = cell[0], c1 = cell[1];
    int it = cell[2];
    const int it_last = cell[3];
    const int e0 = cell[4], e1 = cell[5], e2 = cell[6], e3 = cell[7], e4 = cell[8];   // last iteration of the wave's first five tiles
    const int range_c0 = a.cell[(size_t)my_range * kColWaves * kWaveInts];            // first tile of the range: wave 0's c0
    // (the table's address is pinned in the entry block - behind the record's loads, which an asm statement in front of them
    // would turn into vector loads: left to the compiler it was fetched from the arguments where the DMA loop starts, and the
    // wait for it there also waited for the record - a round trip to plan memory in front of the first request.  Here it
    // arrives with the other arguments, behind their one wait.)
    const float* table = a.table;
    asm volatile("" : "+s"(table));
    // ---- this column group of every node -> LDS, 1 KB per wave instruction (rows_pad * CW * 4 is a multiple of 1 KB;
    //      row n of the table is zero: padded id slots name it) ----
    {
        const int total = live ? a.rows_pad * CW / 4 : 0;                 // float4 pieces
        const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(table + (size_t)cg * a.rows_pad * CW);
        for (int i = wave * 64; i < total; i += kColThreads)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i + lane),
                                             (__attribute__((address_space(3))) void*)(lds4 + i), 16, 0, 0);
    }
    asm volatile("" ::: "memory");                                         // what follows is requested behind the DMA loads
    int tile_end = e0;
    // sixteen iterations of ids are requested before anything is consumed (a wave has ~13 on PoSE): the stream comes
    // from HBM once per range, and a loop that asks for it three iterations ahead pays that latency again and again.
    // A wave with fewer asks for its LAST iteration again instead of what lies behind it (a wave-uniform index: the loads
    // stay unconditional; the repeat is served by the L1): ids nobody reads took a fifth of the stream's share of the fill,
    // which runs at the rate the L2 feeds one compute unit.
    const u32x2* __restrict__ sp = a.ids + (size_t)it * 64 + lane;
    const int it_have = max(it_last - it, 1) - 1;                          // the last iteration the wave has (0: also for none)
    u32x2 wa[8], wb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wa[k] = sp[64 * min(k, it_have)];
#pragma unroll
    for (int k = 0; k < 8; ++k) wb[k] = sp[64 * min(8 + k, it_have)];
    sp += 1024;
    // direct stores: destination row and scale of this quad in the wave's first four tiles (more tiles: read when they
    // come up).  The staged loop needs neither: its write-out reads them for all the wave's tiles at once.
    int row = -1, row1 = -1, row2 = -1, row3 = -1;
    float d = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
    vec_t bias = (vec_t)(0.f);
    if constexpr (!STAGED) {
        const int32_t* __restrict__ trp = a.tile_rows + (size_t)c0 * 16 + q;   // the arrays end with four spare tiles
        const float* __restrict__ tdp = a.tile_dis + (size_t)c0 * 16 + q;
        row = trp[0]; row1 = trp[16]; row2 = trp[32]; row3 = trp[48];
        d = tdp[0]; d1 = tdp[16]; d2 = tdp[32]; d3 = tdp[48];
        if (a.bias) bias = *reinterpret_cast<const vec_t*>(a.bias + CW * cg);
    }
    int t = c0;
    // Everything requested so far has to be here: the LDS-DMA loads, and with them the id / row / scale loads issued
    // behind them.  (Loads return in issue order, so a count that lets exactly those later loads stay in flight would
    // release the barrier a little earlier - measured: the same total, the gather needs the first ids at once - but such
    // a count depends on how many vector loads the compiler emits for the lines above.  Zero does not.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#ifdef GN_STAMPS
    const unsigned long long st1 = __builtin_amdgcn_s_memrealtime();
#endif
    const vec_t* __restrict__ tab = reinterpret_cast<const vec_t*>(lds4);
    vec_t* stage = reinterpret_cast<vec_t*>(lds4) + a.rows_pad;          // behind the table: slot (tile - range_c0) * 16 + quad
    vec_t acc = (vec_t)(0.f);
    // (macros, not lambdas: with the closures hipcc 7.2 kept the kernel arguments and every captured local in scratch)
    // GN_COL_FLUSH: tile t is complete - fold the quad (DPP: no LDS round trip), then either park the sums (staged) or
    // scale, bias, ReLU, write (direct); step to the next tile
#define GN_COL_FLUSH()                                                                                         \
    do {                                                                                                       \
        _Pragma("unroll") for (int c = 0; c < CW; ++c)                                                         \
            acc[c] = gn::dpp_add<0x4E>(gn::dpp_add<0xB1>(acc[c]));     /* + lane ^ 1, then + lane ^ 2 */       \
        if constexpr (STAGED) {                                                                                \
            if (j == 0) stage[(t - range_c0) * 16 + q] = acc;                                                  \
        } else if (j == 0 && row >= 0) {                                                                       \
            vec_t r = scale_bias<CW>(acc, d, bias);                                                            \
            if (a.relu) {                                                                                      \
                _Pragma("unroll") for (int c = 0; c < CW; ++c) r[c] = gn::relu_keep_nan(r[c]);                        \
            }                                                                                                  \
            *reinterpret_cast<vec_t*>(a.out + (int64_t)row * a.ld_out + CW * cg) = r;                          \
            if constexpr (NEXT)                                                                                \
                *reinterpret_cast<vec_t*>(a.next_table + ((size_t)cg * a.rows_pad + row) * CW) = r * d;        \
        }                                                                                                      \
        acc = (vec_t)(0.f);                                                                                    \
        ++t;                                                                                                   \
        const int kk = t - c0;                                                                                 \
        tile_end = kk == 1 ? e1 : (kk == 2 ? e2 : (kk == 3 ? e3 : (kk == 4 ? e4 : a.tile_off[t + 1])));       \
        if constexpr (!STAGED) {                                                                               \
            if (kk < 4) {                                                                                      \
                row = kk == 1 ? row1 : (kk == 2 ? row2 : row3);                                                \
                d = kk == 1 ? d1 : (kk == 2 ? d2 : d3);                                                        \
            } else {                                                                                           \
                row = a.tile_rows[(size_t)t * 16 + q];                                                         \
                d = a.tile_dis[(size_t)t * 16 + q];                                                            \
            }                                                                                                  \
        }                                                                                                      \
    } while (0)
    // GN_COL_CONSUME: eight iterations out of registers; tile ends are wave-uniform (the inner while also passes empty tiles)
#define GN_COL_CONSUME(w)                                                                                      \
    _Pragma("unroll") for (int k = 0; k < 8; ++k) {                                                            \
        while (t < c1 && it == tile_end) GN_COL_FLUSH();                                                       \
        if (it < it_last) {                                                                                    \
            const uint32_t s0 = w[k].x & 0xffffu, s1 = w[k].x >> 16, s2 = w[k].y & 0xffffu, s3 = w[k].y >> 16; \
            acc += (tab[s0] + tab[s1]) + (tab[s2] + tab[s3]);                                                  \
            ++it;                                                                                              \
        }                                                                                                      \
    }
    // A buffer is requested again only when iterations beyond the eight the OTHER buffer holds remain: a wave of up to
    // sixteen iterations (every wave on PoSE) asks for its ids once, in the prologue.
    while (it < it_last) {
        GN_COL_CONSUME(wa)
        if (it >= it_last) break;
        if (it + 8 < it_last) {
#pragma unroll
            for (int k = 0; k < 8; ++k) wa[k] = sp[64 * k];                // the stream has slack behind its end
        }
        GN_COL_CONSUME(wb)
        if (it + 8 < it_last) {
#pragma unroll
            for (int k = 0; k < 8; ++k) wb[k] = sp[512 + 64 * k];
        }
        sp += 1024;
    }
    while (t < c1) GN_COL_FLUSH();
#undef GN_COL_CONSUME
#undef GN_COL_FLUSH
#ifdef GN_STAMPS
    const unsigned long long st2 = __builtin_amdgcn_s_memrealtime();
#endif
    if constexpr (STAGED) {
        // ---- write-out: a lane per (tile, quad) of the wave's tiles, 128 slots per trip.  The wave itself wrote the
        //      slots (LDS operations of a wave complete in order): no barrier.  Rows, scales and slots of a trip are all
        //      requested before the first store; the expressions are the direct loop's ----
        vec_t wbias = (vec_t)(0.f);
        if (a.bias) wbias = *reinterpret_cast<const vec_t*>(a.bias + CW * cg);
        const int s_end = c1 * 16;
        for (int s0 = c0 * 16 + lane; s0 < s_end; s0 += 128) {
            const bool two = s0 + 64 < s_end;
            const int s1 = two ? s0 + 64 : s0;
            int rowa = a.tile_rows[s0], rowb = a.tile_rows[s1];
            float da = a.tile_dis[s0], db = a.tile_dis[s1];
            const vec_t va = stage[s0 - range_c0 * 16], vb = stage[s1 - range_c0 * 16];
            asm volatile("" : "+v"(rowa), "+v"(rowb), "+v"(da), "+v"(db));    // one wait behind all four requests, not one per use
            vec_t ra = scale_bias<CW>(va, da, wbias), rb = scale_bias<CW>(vb, db, wbias);
            if (a.relu) {
#pragma unroll
                for (int c = 0; c < CW; ++c) { ra[c] = gn::relu_keep_nan(ra[c]); rb[c] = gn::relu_keep_nan(rb[c]); }
            }
            if (rowa >= 0) {
                *reinterpret_cast<vec_t*>(a.out + (int64_t)rowa * a.ld_out + CW * cg) = ra;
                if constexpr (NEXT) *reinterpret_cast<vec_t*>(a.next_table + ((size_t)cg * a.rows_pad + rowa) * CW) = ra * da;
            }
            if (two && rowb >= 0) {
                *reinterpret_cast<vec_t*>(a.out + (int64_t)rowb * a.ld_out + CW * cg) = rb;
                if constexpr (NEXT) *reinterpret_cast<vec_t*>(a.next_table + ((size_t)cg * a.rows_pad + rowb) * CW) = rb * db;
            }
        }
    }
#ifdef GN_STAMPS
    if (tid == 0 && blockIdx.x < 512) {
        unsigned long long* o = g_blk_stamps[stamp_set & 1][blockIdx.x];
        o[0] = st0; o[1] = st1; o[2] = __builtin_amdgcn_s_memrealtime(); o[3] = st2;
    }
#endif
    // concat slot: streamed by the whole grid, here last
    gn::side_copy_stream(a.side, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// k_col_gather / k_col_gather_next: the staged kernels; *_direct: stores from inside the loop, for plans without room for the slots
template <int CW>
__global__ __launch_bounds__(kColThreads) void k_col_gather(ColArgs a, int stamp_set) { col_gather<CW, false, true>(a, stamp_set); }
template <int CW>
__global__ __launch_bounds__(kColThreads) void k_col_gather_next(ColArgs a, int stamp_set) { col_gather<CW, true, true>(a, stamp_set); }
template <int CW>
__global__ __launch_bounds__(kColThreads) void k_col_gather_direct(ColArgs a, int stamp_set) { col_gather<CW, false, false>(a, stamp_set); }
template <int CW>
__global__ __launch_bounds__(kColThreads) void k_col_gather_next_direct(ColArgs a, int stamp_set) { col_gather<CW, true, false>(a, stamp_set); }

template <int FIN, int NT>
void launch_transform(const TransArgs& t, int cw, hipStream_t st) {
    const int grid = (int)std::min<int64_t>(gn::ceil_div(t.rows_pad / 16, 4), GN_AGG_GRID);
    if (cw == 2) k_col_transform<FIN, NT, 2><<<grid, 256, 0, st>>>(t); else k_col_transform<FIN, NT, 1><<<grid, 256, 0, st>>>(t);
}

}  // namespace

// True when gn_graph_aggregate_f32 takes the LDS-staged path for these shapes and operands: the route's own answer
// (gather_route.hpp, blocked_applicable)
static bool blocked_route(const gn_graph_plan* plan, const float* x, int64_t ld_x, int64_t fin, const float* w, int64_t fout,
                          const float* bias, const float* out, int64_t ld_out) {
    const gn::AggArgs a = gn::forward_args(plan, x, ld_x, fin, bias, 0, const_cast<float*>(out), ld_out);
    return gn::route::gather_route(gn::forward_call(plan, a, w, fout)).kernel == gn::route::Gather::blocked;
}

namespace {

// T = dis * (x W) of the plan, column-group-major (w == null: T = dis * x)
gn_status blocked_transform(const gn_graph_plan* plan, const float* x, int64_t ld_x, int64_t fin, const float* w, int64_t fout,
                            hipStream_t st) {
    TransArgs t;
    t.x = x; t.ld_x = ld_x; t.w = w; t.dis = plan->blk_dis.p; t.table = plan->blk_table.p; t.n = (int)plan->rows;
    t.rows_pad = plan->blk_rows;
    const int cw = plan->blk_cw;
    switch ((int)((w ? fin : fout) * 100 + fout)) {
        case 1616: launch_transform<16, 1>(t, cw, st); break;
        case 3216: launch_transform<32, 1>(t, cw, st); break;
        case 6416: launch_transform<64, 1>(t, cw, st); break;
        case 1632: launch_transform<16, 2>(t, cw, st); break;
        case 3232: launch_transform<32, 2>(t, cw, st); break;
        case 6432: launch_transform<64, 2>(t, cw, st); break;
        default: return gn::fail(GN_ERR_UNSUPPORTED, "no LDS-staged kernel for %lld -> %lld features", (long long)fin, (long long)fout);
    }
    GN_LAUNCH_CHECK();
    return GN_OK;
}

// The staging slots of the largest range: 16 quads x blk_cw floats per tile
size_t stage_bytes(const gn_graph_plan* plan) { return (size_t)plan->blk_range_tiles * 16 * plan->blk_cw * sizeof(float); }

// The staged kernels run when the slots fit behind the table (GN_BLOCKED_DIRECT=1, tests: never)
bool blocked_staged(const gn_graph_plan* plan) {
    const char* e = getenv("GN_BLOCKED_DIRECT");
    if (e && e[0] == '1') return false;
    return (size_t)plan->blk_rows * plan->blk_cw * sizeof(float) + stage_bytes(plan) <= kColLdsBytes;
}

// The gather from LDS over the plan's table as it stands, one workgroup per (column group, range of destination rows);
// next_table != null: the launch also fills that table of a following layer (k_col_gather_next)
gn_status blocked_gather(const gn_graph_plan* plan, int64_t fout, const float* bias, int relu, float* out, int64_t ld_out,
                         const gn_side_copy& side, float* next_table, int stamp_set, hipStream_t st) {
    const int cw = plan->blk_cw;
    GN_REQUIRE((ld_out % cw) == 0 && (reinterpret_cast<uintptr_t>(out) % (4 * cw)) == 0 &&
               (!bias || (reinterpret_cast<uintptr_t>(bias) % (4 * cw)) == 0),
               "the LDS-staged path writes %d-float column groups: out and bias must be aligned to them", cw);
    ColArgs a;
    a.table = plan->blk_table.p; a.cell = plan->blk_cell.p; a.tile_off = plan->blk_tile_off.p; a.tile_rows = plan->blk_tile_rows.p;
    a.tile_dis = plan->blk_tile_dis.p;
    a.ids = reinterpret_cast<const u32x2*>(plan->blk_ids.p); a.dis = plan->blk_dis.p; a.bias = bias;
    a.out = out; a.ld_out = ld_out; a.n = (int)plan->rows; a.rows_pad = plan->blk_rows;
    a.groups = (int)(fout / cw); a.ranges = plan->blk_cells; a.relu = relu; a.side = side; a.next_table = next_table;
    GN_REQUIRE(a.groups >= 1 && (a.groups & (a.groups - 1)) == 0, "the LDS-staged gather deals its workgroups by shifts: %d column groups are no power of two", a.groups);
    const int per_x = (a.ranges + 7) / 8;
    a.per_x = per_x;
    a.group_shift = 0;
    while ((1 << a.group_shift) < a.groups) ++a.group_shift;
    const int grid = 8 * per_x * a.groups;
    const bool staged = blocked_staged(plan);
    const size_t lds = (size_t)plan->blk_rows * cw * sizeof(float) + (staged ? stage_bytes(plan) : 0);
    auto launch = [&](auto kernel) {
        gn_status s = gn::allow_large_lds(reinterpret_cast<const void*>(kernel), (int)kColLdsBytes);
        if (s == GN_OK) kernel<<<grid, kColThreads, lds, st>>>(a, stamp_set);
        return s;
    };
    gn_status s;
    if (staged) {
        if (next_table) s = cw == 2 ? launch(k_col_gather_next<2>) : launch(k_col_gather_next<1>);
        else s = cw == 2 ? launch(k_col_gather<2>) : launch(k_col_gather<1>);
    } else {
        if (next_table) s = cw == 2 ? launch(k_col_gather_next_direct<2>) : launch(k_col_gather_next_direct<1>);
        else s = cw == 2 ? launch(k_col_gather_direct<2>) : launch(k_col_gather_direct<1>);
    }
    if (s != GN_OK) return s;
    GN_LAUNCH_CHECK();
    return GN_OK;
}

// The chained gene stack is opt-in (GN_ENABLE_CHAIN=1) until it has been measured against the four-launch stack on the GPU
bool chain_disabled() {
    const char* e = getenv("GN_ENABLE_CHAIN");
    return !(e && e[0] == '1') || blocked_disabled();
}

// `next` can take its table from a gather over `plan`: both have the LDS-staged encoding of the same unit-weight graph
bool chain_plans_match(const gn_graph_plan* plan, const gn_graph_plan* next) {
    return plan && next && plan != next && plan->blk_ok && next->blk_ok && plan->is_gcn && next->is_gcn && plan->unit_weights &&
           next->unit_weights && plan->rows == next->rows && plan->nnz == next->nnz && plan->blk_rows == next->blk_rows &&
           plan->blk_cw == next->blk_cw && plan->blk_cells == next->blk_cells && plan->blk_iters == next->blk_iters &&
           next->blk_cols >= 16;
}

}  // namespace

gn_status gn_blocked_aggregate(const gn_graph_plan* plan, const float* x, int64_t ld_x, int64_t fin, const float* w,
                               int64_t fout, const float* bias, int relu, float* out, int64_t ld_out,
                               const gn_side_copy& side, hipStream_t st) {
    // 1. the scaled table T = dis * (x W), column-group-major; 2. the gather from LDS
    const gn_status s = blocked_transform(plan, x, ld_x, fin, w, fout, st);
    return s != GN_OK ? s : blocked_gather(plan, fout, bias, relu, out, ld_out, side, nullptr, fin == 32 ? 0 : 1, st);
}

// ---- two layers over one graph, the second one's transform deferred to its reader (gripnet_hip.h) ----------------------
extern "C" int gn_graph_chain_applicable(const gn_graph_plan* plan, const gn_graph_plan* next, const float* x, int64_t ld_x,
                                         int64_t num_features, const float* weight, int64_t out_features, const float* bias,
                                         const float* out, int64_t ld_out, const float* out_next) {
    if (chain_disabled() || !chain_plans_match(plan, next) || !weight || out_features != 16) return 0;
    if (!blocked_route(plan, x, ld_x, num_features, weight, out_features, bias, out, ld_out)) return 0;
    return (reinterpret_cast<uintptr_t>(out_next) % (4 * next->blk_cw)) == 0 ? 1 : 0;
}

extern "C" gn_status gn_graph_aggregate_chain_f32(const gn_graph_plan* plan, const gn_graph_plan* next, const float* x,
                                                  int64_t ld_x, int64_t num_features, const float* weight, int64_t out_features,
                                                  const float* bias, int relu, float* out, int64_t ld_out,
                                                  const gn_side_copy* side, void* stream) {
    GN_REQUIRE(plan && next && x && weight && out, "a plan or a feature pointer is null");
    GN_REQUIRE(ld_x >= num_features && ld_out >= out_features, "leading dimension smaller than the row length");
    if (!gn_graph_chain_applicable(plan, next, x, ld_x, num_features, weight, out_features, bias, out, ld_out, nullptr))
        return gn::fail(GN_ERR_UNSUPPORTED, "the two plans do not chain (LDS-staged plans of one unit-weight graph, 16 output "
                                            "features, GN_ENABLE_CHAIN=1) or the operands keep the wave-per-row kernels");
    gn_side_copy sc;
    gn_status s = gn::check_side(side, plan->rows, &sc);
    if (s != GN_OK) return s;
    hipStream_t st = gn::as_stream(stream);
    s = blocked_transform(plan, x, ld_x, num_features, weight, out_features, st);
    return s != GN_OK ? s : blocked_gather(plan, out_features, bias, relu, out, ld_out, sc, next->blk_table.p, 0, st);
}

extern "C" gn_status gn_graph_gather_chained_f32(const gn_graph_plan* plan, float* out, int64_t ld_out, void* stream) {
    GN_REQUIRE(plan && out && ld_out >= 16, "plan or out is null, or the leading dimension smaller than 16");
    if (chain_disabled() || !plan->blk_ok || !plan->is_gcn || !plan->unit_weights || plan->blk_cols < 16)
        return gn::fail(GN_ERR_UNSUPPORTED, "the plan has no LDS-staged encoding of a unit-weight graph, or the chain is not enabled (GN_ENABLE_CHAIN=1)");
    const gn_side_copy none = {nullptr, 0, nullptr, 0, 0, 0, 0};
    // no bias, no activation: dis[i] * the sum of the table rows, i.e. A_norm h of the table's layer
    return blocked_gather(plan, 16, nullptr, 0, out, ld_out, none, nullptr, 1, gn::as_stream(stream));
}

// Adds the LDS-staged encoding to a GCN plan whose stored weights are all 1 (self loops included), for layers of up to
// `cols` output features (16 or 32).  Not an error when the graph does not qualify: the plan then keeps using the
// wave-per-row kernels (gn_graph_plan_blocked_cols returns 0).  Copies the CSR to the host and synchronises.
extern "C" int gn_graph_blocked_applicable(const gn_graph_plan* plan, const float* x, int64_t ld_x, int64_t num_features,
                                           const float* weight, int64_t out_features, const float* bias, const float* out,
                                           int64_t ld_out) {
    return plan && blocked_route(plan, x, ld_x, num_features, weight, out_features, bias, out, ld_out) ? 1 : 0;
}

extern "C" gn_status gn_graph_plan_build_blocked(gn_graph_plan* plan, int64_t cols, void* stream) {
    GN_REQUIRE(plan != nullptr, "plan is null");
    GN_REQUIRE(cols == 16 || cols == 32, "LDS-staged plans are built for layers of 16 or 32 output features, got %lld", (long long)cols);
    if (plan->blk_ok && plan->blk_cols >= cols) return GN_OK;
    if (!plan->is_gcn || !plan->unit_weights || blocked_disabled()) return GN_OK;
    const int64_t N = plan->rows, nnz = plan->nnz;
    const char* any = getenv("GN_BLOCKED_ANY");                        // tests: no size thresholds
    if (!(any && any[0] == '1') && (N < 4096 || nnz < 16 * N)) return GN_OK;    // small or very sparse graphs: the wave-per-row kernels do fine
    if (N < 1 || N >= 65535) return GN_OK;
    hipStream_t st = gn::as_stream(stream);
    // rows of the table incl. the zero row, padded so that one column group is a whole number of 1 KB DMA pieces
    int cw = 2;
    int64_t rows_pad = gn::ceil_div((N + 1) * cw * 4, 1024) * 1024 / (cw * 4);
    if (rows_pad * cw * 4 > (int64_t)kColLdsBytes) {
        cw = 1;
        rows_pad = gn::ceil_div((N + 1) * cw * 4, 1024) * 1024 / (cw * 4);
        if (rows_pad * cw * 4 > (int64_t)kColLdsBytes) return GN_OK;
    }
    const int groups = (int)(cols / cw);
    const int R = std::max(1, std::min<int>(256 / groups, (int)gn::ceil_div(N, 64)));     // ranges of destination rows

    GN_LAP(nullptr);
    gn::ArenaHold arena;                                       // (before every host array of this build: host_parallel.hpp)
    std::vector<int32_t> rp(N + 1), col(nnz);
    GN_HIP(hipMemcpyAsync(rp.data(), plan->rowptr.p, (N + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GN_HIP(hipMemcpyAsync(col.data(), plan->col.p, nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    std::vector<float> dis_host((size_t)rows_pad + 16, 0.f);
    GN_HIP(hipMemcpyAsync(dis_host.data(), plan->dis.p, N * sizeof(float), hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));

    GN_LAP("blocked: CSR to the host");
    gn_layout::BlockedLayout bl = gn_layout::build_blocked_layout(N, R, rp, col, dis_host);
    GN_LAP("blocked: host schedule");
    if (bl.failed) return gn::fail(GN_ERR_UNSUPPORTED, "internal: an edge was not scheduled");
    if (!bl.ok) return GN_OK;
    plan->blk_ok = 0;
    GN_HIP(plan->blk_dis.upload(dis_host, st));
    GN_HIP(plan->blk_tile_off.upload(bl.tile_off, st));
    GN_HIP(plan->blk_tile_rows.upload(bl.tile_rows, st));
    GN_HIP(plan->blk_tile_dis.upload(bl.tile_dis, st));
    GN_HIP(plan->blk_ids.upload(bl.ids.data(), bl.ids.size() / 2, st));           // (four 16-bit ids of a lane as two words)
    // behind the last range's record an EMPTY one (no tiles, no iterations): what the workgroups of a grid of 8 ceil(R / 8)
    // ranges beyond R walk - the gather has no separate way out for them
    bl.cell.insert(bl.cell.end(), (size_t)kColWaves * kWaveInts, 0);
    GN_HIP(plan->blk_cell.upload(bl.cell, st));
    GN_HIP(plan->blk_table.alloc((size_t)rows_pad * cols));
    // rows beyond the last node stay zero for the life of the plan (padded id slots name row N): k_col_transform writes
    // zeros there, a table filled by another plan's gather (k_col_gather_next) is written at the nodes' rows only
    GN_HIP(hipMemsetAsync(plan->blk_table.p, 0, (size_t)rows_pad * cols * sizeof(float), st));
    GN_HIP(hipStreamSynchronize(st));
    GN_LAP("blocked: upload");
    plan->blk_cols = (int)cols; plan->blk_cw = cw; plan->blk_rows = (int)rows_pad; plan->blk_cells = R;
    plan->blk_iters = bl.iters_total;
    plan->blk_range_tiles = 0;                                          // the largest range: last wave's end tile - first wave's first tile
    for (int r = 0; r < R; ++r) {
        const int32_t* c = bl.cell.data() + (size_t)r * kColWaves * kWaveInts;
        plan->blk_range_tiles = std::max<int>(plan->blk_range_tiles, c[(kColWaves - 1) * kWaveInts + 1] - c[0]);
    }
    plan->blk_ok = 1;
    return GN_OK;
}

#ifdef GN_STAMPS
extern "C" __attribute__((visibility("default"))) int gn_debug_read_blk_stamps(unsigned long long* host_out) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_blk_stamps), sizeof(unsigned long long) * 2 * 512 * 4);
}
#endif

extern "C" int gn_graph_plan_blocked_gather_kernel(const gn_graph_plan* plan) {
    if (!plan || !plan->blk_ok || blocked_disabled()) return 0;
    return blocked_staged(plan) ? 1 : 2;
}

// tests: the schedule the gather walks, [ranges][16 waves][12] (first tile, end tile, first iteration, end iteration, ...)
extern "C" int64_t gn_graph_plan_blocked_waves(const gn_graph_plan* plan, int32_t* host_out, int64_t capacity) {
    if (!plan || !plan->blk_ok) return 0;
    const int64_t count = (int64_t)plan->blk_cells * kColWaves * kWaveInts;    // (without the empty record behind the last range)
    if (host_out) {
        if (capacity < count) return -1;
        if (hipMemcpy(host_out, plan->blk_cell.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    return count;
}

extern "C" int64_t gn_graph_plan_blocked_cols(const gn_graph_plan* plan) {
    return (plan && plan->blk_ok && !blocked_disabled()) ? plan->blk_cols : 0;
}
