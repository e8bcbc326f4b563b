// Destination-major gather-reduce shared by the GCN-style layers and the general RGCN path: every kernel of the family
// and its launch function, compiled here once (aggregate.cuh: arguments and declarations; gather_route.hpp: the selection).
//
//   out[i, :] = act( (sum_{p in row i} coef[p] * T[col[p], :]) / max(1, rowdiv[i]) + addend[i, :] + bias )
//
// One 64-lane wave owns one destination row at a time.  The wave reads 64 (col, coef) pairs
// with one coalesced load each, then walks them S = 64/LPE at a time: every group of LPE
// lanes covers the feature row of one neighbour with 16-byte loads, so a wave
// keeps S independent row gathers in flight.  The S partial sums are folded with cross-lane
// shuffles, in a fixed order: results are bitwise reproducible run to run.
#include "aggregate.cuh"

#include <type_traits>

namespace gn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- what one lane reads of a table row: N features as one load, summed into float acc[N] element by element ----
struct RowScalar {                                             // 1 float: rows that are not 16-byte aligned
    static constexpr int N = 1;
    static constexpr bool kMean = true;                        // the epilogue takes rowdiv and addend
    typedef float elem;
    typedef float raw;
    static __device__ __forceinline__ const elem* table(const AggArgs& a) { return a.table; }
    static __device__ __forceinline__ raw load(const elem* p) { return *p; }
    static __device__ __forceinline__ void add(float (&acc)[N], float coef, raw r) { acc[0] += coef * r; }
};
struct RowF32 {                                                // 16 bytes = 4 floats
    static constexpr int N = 4;
    static constexpr bool kMean = true;
    typedef float elem;
    typedef f32x4 raw;
    static __device__ __forceinline__ const elem* table(const AggArgs& a) { return a.table; }
    static __device__ __forceinline__ raw load(const elem* p) { return *reinterpret_cast<const raw*>(p); }
    static __device__ __forceinline__ void add(float (&acc)[N], float coef, raw r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += coef * r[k];
    }
};
struct RowBf16 {                                               // 16 bytes = 8 bf16 (graph_bf16.hip), widened by shifts
    static constexpr int N = 8;
    static constexpr bool kMean = false;                       // gn_graph_aggregate_bf16 has neither
    typedef uint16_t elem;
    typedef u32x4 raw;
    static __device__ __forceinline__ const elem* table(const AggArgs& a) { return a.table_bf16; }
    static __device__ __forceinline__ raw load(const elem* p) { return *reinterpret_cast<const raw*>(p); }
    static __device__ __forceinline__ void add(float (&acc)[N], float coef, raw r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[2 * k] += coef * __uint_as_float(r[k] << 16);
            acc[2 * k + 1] += coef * __uint_as_float(r[k] & 0xffff0000u);
        }
    }
};

// The tail of a row's sum: the mean's divisor and the addend (MEAN: the rows that have them), the bias and the activation,
// then 16-byte stores.
template <bool MEAN, int N>
__device__ __forceinline__ void finish_row(const AggArgs& a, int row, int fcol, float (&acc)[N]) {
    const float div = MEAN && a.rowdiv ? fmaxf(a.rowdiv[row], 1.0f) : 1.0f;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        float val = MEAN && a.rowdiv ? acc[t] / div : acc[t];
        if (MEAN && a.addend) val += a.addend[(int64_t)row * a.ld_addend + fcol + t];
        if (a.bias) val += a.bias[fcol + t];
        if (a.relu) val = gn::relu_keep_nan(val);
        acc[t] = val;
    }
    float* dst = a.out + (int64_t)row * a.ld_out + fcol;
    if constexpr (N == 1) {
        dst[0] = acc[0];
    } else {
#pragma unroll
        for (int t = 0; t < N; t += 4) *reinterpret_cast<float4*>(dst + t) = make_float4(acc[t], acc[t + 1], acc[t + 2], acc[t + 3]);
    }
}

// x = hi + mid + lo exactly, every term a bf16 cut by truncation: the upper halves of the three words.
__device__ __forceinline__ void split3(float x, uint32_t (&t)[3]) {
    t[0] = __builtin_bit_cast(uint32_t, x);
    const float r = x - __builtin_bit_cast(float, t[0] & 0xffff0000u);
    t[1] = __builtin_bit_cast(uint32_t, r);
    const float s = r - __builtin_bit_cast(float, t[1] & 0xffff0000u);
    t[2] = __builtin_bit_cast(uint32_t, s);
}

// One value into the split planes of X (gn_split_planes): its three bf16 terms, cut by truncation exactly as the
// relational kernel cuts them itself (rgcn_pair.hip: split_pair), so a layer gives the same bits either way.
__device__ __forceinline__ void write_split(const gn_split_planes& sp, int64_t row, int col, float v) {
    const int cellb = 4 * ((3 * sp.nt + 1) / 2);
    const int cell = col / sp.nt, j = col - cell * sp.nt;
    unsigned short* p = reinterpret_cast<unsigned short*>(static_cast<unsigned char*>(sp.planes) + (row * 16 + cell) * cellb) + j;
    uint32_t t[3];
    split3(v, t);
    p[0] = (unsigned short)(t[0] >> 16);
    p[sp.nt] = (unsigned short)(t[1] >> 16);
    p[2 * sp.nt] = (unsigned short)(t[2] >> 16);
}

__global__ __launch_bounds__(256) void k_split_planes(const float* __restrict__ src, int64_t ld_src, int64_t rows, int cols, int col0,
                                                      gn_split_planes sp) {
    const int64_t total = rows * cols;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / cols;
        const int c = (int)(t - i * cols);
        write_split(sp, i, col0 + c, src[i * ld_src + c]);
    }
}

template <typename Row, int LPE>
__global__ __launch_bounds__(256) void k_aggregate(AggArgs a) {
    constexpr int S = kWave / LPE, N = Row::N;
    const int lane = threadIdx.x & 63;
    const int slot = lane / LPE;
    const int j = lane % LPE;
    const int wave = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
    const int n_waves = (int)(((int64_t)gridDim.x * blockDim.x) >> 6);

    side_copy_stream(a.side, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
    for (int row = wave; row < a.rows; row += n_waves) {
        const int begin = a.rowptr[row], end = a.rowptr[row + 1];
        for (int cb = 0; cb * LPE * N < a.features; ++cb) {
            const int fcol = (cb * LPE + j) * N;
            const bool active = fcol < a.features;
            float acc[N];
#pragma unroll
            for (int t = 0; t < N; ++t) acc[t] = 0.f;

            for (int base = begin; base < end; base += kWave) {
                const int mine = base + lane;
                const uint32_t c = mine < end ? a.col[mine] : 0u;
                const float v = mine < end ? (a.coef ? a.coef[mine] : 1.0f) : 0.f;
                const int cnt = min(kWave, end - base);
                // The neighbour rows of the whole batch are requested before the first one is consumed: a loop
                // that loads and adds one group of S rows per trip pays an L2 round trip per trip.
                constexpr int IT = kWave / S, U = IT < GN_AGG_U ? IT : GN_AGG_U;   // groups of S rows per batch, U in flight
                for (int it0 = 0; it0 * S < cnt; it0 += U) {
                    typename Row::raw t[U];
                    float vv[U];
#pragma unroll
                    for (int it = 0; it < U; ++it) {
                        const int idx = (it0 + it) * S + slot;
                        const uint32_t cc = (uint32_t)__shfl((int)c, idx);
                        vv[it] = __shfl(v, idx);
                        t[it] = typename Row::raw{};
                        if (idx < cnt && active) t[it] = Row::load(Row::table(a) + (int64_t)cc * a.ld_table + fcol);
                    }
#pragma unroll
                    for (int it = 0; it < U; ++it) {
                        // (the bf16 row's add() written out: through the call the same instructions are allocated 70
                        // registers for LPE 2 instead of 64, a wave per SIMD less)
                        if constexpr (std::is_same<Row, RowBf16>::value) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                acc[2 * k] += vv[it] * __uint_as_float(t[it][k] << 16);
                                acc[2 * k + 1] += vv[it] * __uint_as_float(t[it][k] & 0xffff0000u);
                            }
                        } else {
                            Row::add(acc, vv[it], t[it]);
                        }
                    }
                }
            }
#pragma unroll
            for (int off = LPE; off < kWave; off <<= 1) {
#pragma unroll
                for (int t = 0; t < N; ++t) acc[t] += __shfl_xor(acc[t], off);
            }
            if (slot == 0 && active) finish_row<Row::kMean>(a, row, fcol, acc);
        }
    }
}

// Rows of a few neighbours each (the (relation, source) rows of the relational layer's weight gradient: 6 x 10^5 rows
// of ~3 edges): a wave per row spends its time on row bookkeeping.  Here LPE lanes own a row - 64 / LPE rows per wave
// side by side, every lane sums its own four columns over the row's neighbours, two loads in flight - and nothing
// is folded across lanes.
template <int LPE>
__global__ __launch_bounds__(256) void k_aggregate_short(AggArgs a) {
    constexpr int S = kWave / LPE;
    const int lane = threadIdx.x & 63, slot = lane / LPE, j = lane % LPE;
    const int wave = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
    const int n_waves = (int)(((int64_t)gridDim.x * blockDim.x) >> 6);
    const int fcol = 4 * j;
    const bool active = fcol < a.features;
    side_copy_stream(a.side, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
    for (int row0 = wave * S; row0 < a.rows; row0 += n_waves * S) {
        const int row = row0 + slot;
        const bool live = row < a.rows && active;
        const int begin = live ? a.rowptr[row] : 0, end = live ? a.rowptr[row + 1] : 0;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = begin; __any(p < end); p += 2) {
            const bool h0 = p < end, h1 = p + 1 < end;
            const uint32_t c0 = h0 ? a.col[p] : 0u, c1 = h1 ? a.col[p + 1] : 0u;
            const float v0 = h0 ? (a.coef ? a.coef[p] : 1.0f) : 0.f, v1 = h1 ? (a.coef ? a.coef[p + 1] : 1.0f) : 0.f;
            float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
            if (h0) r0 = *reinterpret_cast<const float4*>(a.table + (int64_t)c0 * a.ld_table + fcol);
            if (h1) r1 = *reinterpret_cast<const float4*>(a.table + (int64_t)c1 * a.ld_table + fcol);
            acc.x += v0 * r0.x; acc.y += v0 * r0.y; acc.z += v0 * r0.z; acc.w += v0 * r0.w;
            acc.x += v1 * r1.x; acc.y += v1 * r1.y; acc.z += v1 * r1.z; acc.w += v1 * r1.w;
        }
        if (live) {
            float o[4] = {acc.x, acc.y, acc.z, acc.w};
            finish_row<true>(a, row, fcol, o);
        }
    }
}

// A lane group's row, summed in neighbour order: the group reads its (col, coef) pairs LPE at a time with one coalesced
// load and requests U neighbour rows before it consumes the first.  `tab` is the table at this lane's first feature;
// a lane that is not `active` (its features lie beyond the row) hands its pairs round and loads nothing.
// (AggArgs by reference, here and in finish_row: by value the lane-group kernels take up to 10 more VGPRs)
template <typename Row, int LPE, int U>
__device__ __forceinline__ void gather_group_row(const AggArgs& a, const typename Row::elem* __restrict__ tab, int begin, int end,
                                                 int j, bool active, float (&acc)[Row::N]) {
    for (int base = begin; __any(base < end); base += LPE) {
        const int mine = base + j;
        const uint32_t c = mine < end ? a.col[mine] : 0u;
        const float v = mine < end ? (a.coef ? a.coef[mine] : 1.0f) : 0.f;
        const int cnt = min(LPE, end - base);                  // of this group (<= 0 once its row is done)
        for (int t0 = 0; __any(t0 < cnt); t0 += U) {
            typename Row::raw r[U];
            float vv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t cc = (uint32_t)__shfl((int)c, t0 + u, LPE);
                vv[u] = __shfl(v, t0 + u, LPE);
                r[u] = typename Row::raw{};
                if (t0 + u < cnt && active) r[u] = Row::load(tab + (int64_t)cc * a.ld_table);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) Row::add(acc, vv[u], r[u]);
        }
    }
}

// Rows of a dozen to a few dozen neighbours (the homogeneous layers of the node-classification graphs: 5 x 10^4 rows of
// ~11 edges over a table far larger than an L2): a wave per row walks rowptr -> col -> gathered rows -> fold as four
// dependent round trips per row, six rows deep per wave.  Here LPE lanes own a row - 64 / LPE rows per wave side by
// side, one row per group and no grid-stride loop - the group reads its (col, coef) pairs LPE at a time with one
// coalesced load and requests U neighbour rows before it consumes the first: the latency chain of a row is paid once
// per wave, with 64 / LPE x U row gathers in flight.  Every lane sums its own columns in neighbour order.
// (On a bf16 table - round 6 - the wave-per-row kernel paid the row's latency chain per wave and made bf16 storage
// SLOWER than fp32: freebase-c-syn 414.7 against 381.7 us per forward.)
template <typename Row, int LPE, int U>
__global__ __launch_bounds__(256) void k_aggregate_group(AggArgs a) {
    constexpr int S = kWave / LPE, N = Row::N;
    const int lane = threadIdx.x & 63, slot = lane / LPE, j = lane % LPE;
    const int wave = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
    const int fcol = N * j;
    const bool active = fcol < a.features;
    side_copy_stream(a.side, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
    const int row = wave * S + slot;
    const bool live = row < a.rows;
    const int begin = live ? a.rowptr[row] : 0, end = live ? a.rowptr[row + 1] : 0;
    float acc[N];
#pragma unroll
    for (int t = 0; t < N; ++t) acc[t] = 0.f;
    gather_group_row<Row, LPE, U>(a, Row::table(a) + fcol, begin, end, j, active, acc);
    if (live && active) finish_row<Row::kMean>(a, row, fcol, acc);
}

// ---- aggregate, then transform: out[i, :] = act( (sum_p coef[p] * X[col[p], :]) @ W + bias ) ----------------
// A_norm (X W) = (A_norm X) W, so the dense contraction of a GCN-style layer (gripnet/layers.py:73) can run
// on the aggregated row instead of on every node beforehand: no X W launch, no [N, out] round trip through
// HBM.  The gather is bound by the number of L2 requests (one per neighbour row), not by their size, so
// gathering the wider input row costs about the same.  FIN = 4 LPE input features (one float4 per lane of
// the neighbour's group), FOUT in {16, 32}.  Epilogue: after the butterfly fold every lane holds the
// aggregated features 4j..4j+3 of its j; lane (c = lane % FOUT, kq = lane / FOUT) multiplies KPL = FIN * FOUT / 64
// of them (fetched with shuffles) by its register-resident slice W[kq*KPL .. , c] and the 64 / FOUT partial
// sums are folded with two more shuffles.
//
// TAIL (64 input features): the table's last 16 columns hold G = A_norm h of a 16 -> 16 layer whose transform was left to
// its reader (gn_graph_aggregate_tail_f32): every GATHERED row gets relu(G W2 + b2) in their place before it is multiplied
// by its coefficient - the ReLU sits between the two sums, so the product cannot move behind this one.  The four lanes
// j = 12..15 of a neighbour's group hold the 16 floats: a quad, which hands them round with DPP; lane jj of it computes
// the columns 4 jj .. 4 jj + 3 against its register-resident slice of W2 (one wave per SIMD here: registers are free).
template <int CTRL>
__device__ __forceinline__ float tail_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true));
}

// `token` as it is, in a vector register, behind sixteen gathered rows: one empty statement that reads all of them, so every
// one of their loads is issued in front of it and every use of what it returns stands behind it.
__device__ __forceinline__ int rows_landed(int token, const f32x4 (&t)[16]) {
    asm volatile("" : "+v"(token)
                 : "v"(t[0]), "v"(t[1]), "v"(t[2]), "v"(t[3]), "v"(t[4]), "v"(t[5]), "v"(t[6]), "v"(t[7]), "v"(t[8]), "v"(t[9]),
                   "v"(t[10]), "v"(t[11]), "v"(t[12]), "v"(t[13]), "v"(t[14]), "v"(t[15]));
    return token;
}
template <int N>
__device__ __forceinline__ int rows_landed(int token, const f32x4 (&)[N]) { return token; }   // (the narrow instantiations never ask)

// SPLIT (64 input features): the gathered row is kept in two tables (AggSplit) - lane j of a neighbour's group takes its 16
// bytes from the head table where 4 j < head_cols, from the tail table otherwise: the same loads, lines, sums and bits as over
// the materialised concatenation, which then has no reader.
template <int LPE, int FOUT, bool TAIL, bool SPLIT = false>
__device__ __forceinline__ void aggregate_transform(const AggArgs& a, const float* __restrict__ w, const AggTail& tail,
                                                    const AggSplit& split = AggSplit{nullptr, 0, 0}) {
    constexpr int FIN = 4 * LPE, S = kWave / LPE, G = kWave / FOUT, KPL = FIN / G;
    static_assert(KPL % 4 == 0, "K slice per lane must cover whole float4 groups");
    static_assert(!TAIL || LPE == 16, "the deferred tail transform is the last quad of a 16-lane group");
    static_assert(!SPLIT || !TAIL, "a split source has no deferred tail transform");
    static_assert(!SPLIT || LPE == 16, "a split source is 64 columns: sixteen lanes a neighbour");
    const int lane = threadIdx.x & 63;
    const int slot = lane / LPE, j = lane % LPE;
    const int c = lane % FOUT, kq = lane / FOUT;
    const int block = blockIdx.x, n_blocks = gridDim.x;
    const int wave = (int)((block * (int64_t)blockDim.x + threadIdx.x) >> 6);
    const int n_waves = (int)(((int64_t)n_blocks * blockDim.x) >> 6);
    float wreg[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) wreg[i] = w[(kq * KPL + i) * FOUT + c];
    const float bias = a.bias ? a.bias[c] : 0.f;
    f32x4 tw[TAIL ? 16 : 1], tb = (f32x4){0.f, 0.f, 0.f, 0.f};               // W2[k][4 jj .. 4 jj + 3], b2[4 jj ..]
    if constexpr (TAIL) {
#pragma unroll
        for (int k = 0; k < 16; ++k) tw[k] = *reinterpret_cast<const f32x4*>(tail.w + 16 * k + 4 * (j & 3));
        if (tail.b) tb = *reinterpret_cast<const f32x4*>(tail.b + 4 * (j & 3));
    }

    // concat slot, by the whole grid: the first element of every thread is REQUESTED here and stored behind the rows (a
    // load -> store in front of them put its round trip in front of the rows' own three), the rest (slots longer than
    // the grid) is streamed at the end
    const int64_t side_total = a.side.dst ? a.side.rows * a.side.cols : 0;
    const int64_t side_t0 = block * (int64_t)blockDim.x + threadIdx.x;
    float side_first = 0.f;
    if (side_t0 < side_total) {
        const int64_t i = side_t0 / a.side.cols, cc = side_t0 - i * a.side.cols;
        side_first = a.side.src[i * a.side.ld_src + cc];
    }
    // SPLIT: this lane's table at its first feature, and that table's row stride (both fit 32 bits: the launcher checked)
    const float* __restrict__ src = nullptr;
    uint32_t src_ld = 0;
    if constexpr (SPLIT) {
        const bool in_head = 4 * j < split.head_cols;
        src = in_head ? a.table + 4 * j : split.tail + (4 * j - split.head_cols);
        src_ld = in_head ? (uint32_t)a.ld_table : split.ld_tail;
    }
    for (int row = wave; row < a.rows; row += n_waves) {
        // padded rows: this lane's (column, coefficient) pair sits at row * 64 + lane - no row pointers in front of it
        int begin, end;
        uint32_t cl0 = 0u;
        float v0 = 0.f;
        if (a.ell_col) {
            cl0 = a.ell_col[(size_t)row * 64 + lane];
            v0 = a.ell_coef[(size_t)row * 64 + lane];
            begin = 0;
            end = __popcll(__ballot(cl0 != 0xffffffffu));
            if (lane >= end) cl0 = 0u;
        } else {
            begin = a.rowptr[row];
            end = a.rowptr[row + 1];
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int base = begin; base < end; base += kWave) {
            const int mine = base + lane;
            const uint32_t cl = a.ell_col ? cl0 : (mine < end ? a.col[mine] : 0u);
            const float v = a.ell_col ? v0 : (mine < end ? (a.coef ? a.coef[mine] : 1.0f) : 0.f);
            const int cnt = min(kWave, end - base);
            // U groups of S neighbour rows are requested before the first one is consumed (see k_aggregate); wide rows
            // (16 lanes each: the external layer, a few hundred destination rows of 14..47 edges, one wave per SIMD,
            // latency-bound) ask for all sixteen groups = 64 rows at once: a quarter of pose0-syn's rows have more than 32
            // neighbours and paid a second dependent round trip at eight groups.  Slot `slot` adds its rows in the order
            // idx = (it0 + it) * S + slot whatever U is: the bits do not depend on it.
            constexpr int IT = kWave / S, UW = LPE >= 16 ? GN_AGG_U_WIDE : GN_AGG_U, U = IT < UW ? IT : UW;
            for (int it0 = 0; it0 * S < cnt; it0 += U) {
                f32x4 t[U];
                float vv[U];
#pragma unroll
                for (int it = 0; it < U; ++it) {
                    const int idx = (it0 + it) * S + slot;
                    uint32_t cc = (uint32_t)__shfl((int)cl, idx);
                    vv[it] = __shfl(v, idx);
                    if constexpr (LPE >= 16) {
                        // Every load of the batch is issued, whatever the row's length: a slot beyond the row's end reads
                        // row 0 (a row with a neighbour has a table with a row) and what it read is dropped below.  Under
                        // `if (idx < cnt)` the compiler waits for each load inside its own branch (s_waitcnt vmcnt(0) behind
                        // every global_load of the batch): a round trip per group of four neighbours, eight in a row of 29.
                        cc &= (uint32_t)((idx - cnt) >> 31);                       // idx < cnt: all ones
                        if constexpr (SPLIT) t[it] = *reinterpret_cast<const f32x4*>(src + (uint64_t)cc * src_ld);
                        else t[it] = *reinterpret_cast<const f32x4*>(a.table + (int64_t)cc * a.ld_table + 4 * j);
                    } else {
                        t[it] = (f32x4)(0.f);
                        if (idx < cnt) t[it] = *reinterpret_cast<const f32x4*>(a.table + (int64_t)cc * a.ld_table + 4 * j);
                    }
                }
                int cnt_behind = cnt;                                              // (the row's length for what follows the loads)
                if constexpr (LPE >= 16) {
                    // A slot without a row becomes +0 through a bit mask whose operand - the row's length - comes out of
                    // rows_landed: no use of a loaded row can stand in front of the last request.  (Left to itself the
                    // compiler turned the mask back into a select, consumed the first rows in front of the last requests
                    // to save registers - one wave per SIMD has them - and made those a second and third trip.)
                    cnt_behind = rows_landed(cnt, t);
#pragma unroll
                    for (int it = 0; it < U; ++it) {
                        const uint32_t keep = (uint32_t)(((it0 + it) * S + slot - cnt_behind) >> 31);
#pragma unroll
                        for (int k = 0; k < 4; ++k) t[it][k] = __uint_as_float(__float_as_uint(t[it][k]) & keep);
                    }
                }
                if constexpr (TAIL) {
#pragma unroll
                    for (int it = 0; it < U; ++it) {
                        if ((it0 + it) * S >= cnt) continue;                       // (wave-uniform: no row in this group)
                        const float g[4] = {t[it].x, t[it].y, t[it].z, t[it].w};
                        f32x4 h = tb;
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {                           // lane jj of the quad holds G[4 jj + cc]
                            h += tail_bcast<0x00>(g[cc]) * tw[cc];
                            h += tail_bcast<0x55>(g[cc]) * tw[4 + cc];
                            h += tail_bcast<0xAA>(g[cc]) * tw[8 + cc];
                            h += tail_bcast<0xFF>(g[cc]) * tw[12 + cc];
                        }
                        if (tail.relu) {
#pragma unroll
                            for (int cc = 0; cc < 4; ++cc) h[cc] = gn::relu_keep_nan(h[cc]);
                        }
                        // (a slot beyond the row's end stays zero: relu(b2) is not)
                        if (j >= 12 && (it0 + it) * S + slot < cnt_behind) t[it] = h;
                    }
                }
#pragma unroll
                for (int it = 0; it < U; ++it) {
                    // The roundings of `acc[k] += vv * t[k]` as this loop has always been compiled, written out: features 0 and
                    // 1 of a lane fused, 2 and 3 as a rounded product and a sum (the compiler's choice with contraction left
                    // to it; it chose otherwise once the loads moved, and every output of the layer changed in its last bit).
#pragma clang fp contract(off)
                    acc[0] = __builtin_fmaf(vv[it], t[it].x, acc[0]);
                    acc[1] = __builtin_fmaf(vv[it], t[it].y, acc[1]);
                    const float pz = vv[it] * t[it].z, pw = vv[it] * t[it].w;
                    acc[2] = acc[2] + pz;
                    acc[3] = acc[3] + pw;
                }
                if constexpr (U == IT) break;                                      // (one trip, said so: it0 is the constant 0, not sixteen scalars)
            }
        }
#pragma unroll
        for (int off = LPE; off < kWave; off <<= 1) {
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] += __shfl_xor(acc[t], off);
        }
        // every lane now holds aggregated features 4j .. 4j+3; contract with W
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < KPL; ++i) part += __shfl(acc[i % 4], kq * (KPL / 4) + i / 4) * wreg[i];
#pragma unroll
        for (int off = FOUT; off < kWave; off <<= 1) part += __shfl_xor(part, off);
        if (kq == 0) {
            float val = part + bias;
            if (a.relu) val = gn::relu_keep_nan(val);
            a.out[(int64_t)row * a.ld_out + c] = val;
            if (a.split.planes) write_split(a.split, row, a.split.col_main + c, val);
        }
    }
    for (int64_t t = side_t0; t < side_total; t += (int64_t)n_blocks * blockDim.x) {
        const int64_t i = t / a.side.cols, cc = t - i * a.side.cols;
        const float v = t == side_t0 ? side_first : a.side.src[i * a.side.ld_src + cc];
        const float o = a.side.mode ? fabsf(v) : v;
        a.side.dst[i * a.side.ld_dst + cc] = o;
        if (a.split.planes) write_split(a.split, i, a.split.col_side + (int)cc, o);
    }
}

template <int LPE, int FOUT>
__global__ __launch_bounds__(256) void k_aggregate_transform(AggArgs a, const float* __restrict__ w) {
    aggregate_transform<LPE, FOUT, false>(a, w, AggTail{nullptr, nullptr, 0});
}
__global__ __launch_bounds__(256) void k_aggregate_transform_tail(AggArgs a, const float* __restrict__ w, AggTail tail) {
    aggregate_transform<16, 16, true>(a, w, tail);
}
template <int FOUT>
__global__ __launch_bounds__(256) void k_aggregate_transform_split(AggArgs a, const float* __restrict__ w, AggSplit split) {
    aggregate_transform<16, FOUT, false, true>(a, w, AggTail{nullptr, nullptr, 0}, split);
}


// ---- aggregate, then transform, for narrow rows (16 or 32 input features): quads instead of shuffles ----------
// Same job and same wave-per-destination-row mapping as k_aggregate_transform, but a neighbour row is gathered
// by a QUAD (lane j: features 4 j .. 4 j + 3, and 16 + 4 j .. for 32 features), so that the 64 (neighbour,
// coefficient) pairs of a batch are handed out with DPP quad broadcasts (the four pairs a quad works through sit in
// its own four lanes: no LDS-pipe shuffle per group of neighbours) and 16 neighbours are gathered per step.  All
// four steps' gathers are in flight before the first is consumed.  The 16 partial sums of the quads are folded with
// a butterfly (fixed order), after which every quad holds the aggregated row; quad q then computes output column q:
// lane (q, j) multiplies the features it holds by its slice of W and the quad folds with two DPP adds.
template <int CTRL>
__device__ __forceinline__ int agg_dpp(int x) { return __builtin_amdgcn_mov_dpp(x, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ float agg_dpp_add(float x) {
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

template <int VPL>
__global__ __launch_bounds__(256) void k_aggregate_transform_q(AggArgs a, const float* __restrict__ w) {
    constexpr int FOUT = 16;
    const int lane = threadIdx.x & 63;
    const int q = lane >> 2, j = lane & 3;
    const int wave = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
    const int n_waves = (int)(((int64_t)gridDim.x * blockDim.x) >> 6);
    f32x4 wreg[VPL];                                          // W[16 v + 4 j + c][q]
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
        for (int c = 0; c < 4; ++c) wreg[v][c] = w[(16 * v + 4 * j + c) * FOUT + q];
    const float bias = a.bias ? a.bias[q] : 0.f;

    side_copy_stream(a.side, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
    const float* __restrict__ tab = a.table + 4 * j;
    for (int row = wave; row < a.rows; row += n_waves) {
        const int begin = a.rowptr[row], end = a.rowptr[row + 1];
        f32x4 s[VPL];
#pragma unroll
        for (int v = 0; v < VPL; ++v) s[v] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int base = begin; base < end; base += kWave) {
            const int mine = base + lane;
            const int c = mine < end ? (int)a.col[mine] : 0;
            const float cf = mine < end ? (a.coef ? a.coef[mine] : 1.0f) : 0.f;
            const int left = end - base - 4 * q;                 // pairs of this quad that exist (may be <= 0)
            int cc[4], ff[4];
            cc[0] = agg_dpp<0x00>(c); cc[1] = agg_dpp<0x55>(c); cc[2] = agg_dpp<0xAA>(c); cc[3] = agg_dpp<0xFF>(c);
            const int fi = __float_as_int(cf);
            ff[0] = agg_dpp<0x00>(fi); ff[1] = agg_dpp<0x55>(fi); ff[2] = agg_dpp<0xAA>(fi); ff[3] = agg_dpp<0xFF>(fi);
            f32x4 t[4][VPL];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    t[k][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (left > k) t[k][v] = *reinterpret_cast<const f32x4*>(tab + (int64_t)cc[k] * a.ld_table + 16 * v);
                }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int v = 0; v < VPL; ++v) s[v] += __int_as_float(ff[k]) * t[k][v];
        }
        // fold the 16 quads (lanes with equal j): butterfly over lane bits 2 .. 5, every lane ends with the total
#pragma unroll
        for (int off = 4; off < kWave; off <<= 1)
#pragma unroll
            for (int v = 0; v < VPL; ++v)
#pragma unroll
                for (int c = 0; c < 4; ++c) s[v][c] += __shfl_xor(s[v][c], off);
        // output column q: this lane's slice of the contraction, then the quad
        float part = 0.f;
#pragma unroll
        for (int v = 0; v < VPL; ++v)
#pragma unroll
            for (int c = 0; c < 4; ++c) part += s[v][c] * wreg[v][c];
        part = agg_dpp_add<0xB1>(part);                          // quad_perm [1,0,3,2]
        part = agg_dpp_add<0x4E>(part);                          // quad_perm [2,3,0,1]
        if (j == 0) {
            float val = part + bias;
            if (a.relu) val = gn::relu_keep_nan(val);
            a.out[(int64_t)row * a.ld_out + q] = val;
        }
    }
}

// ---- aggregate, then transform, for wide layers: (A_norm x) W on the matrix cores ------------------------------
// The layers of the node-classification models whose output is at least as wide as their input (64 -> 64, 128 -> 128:
// the second layer of every homogeneous stack): transform-first pays a tall-skinny product (a launch, N x in read, N x out
// written: 14-19 us at 50,000 nodes) before it gathers rows of the SAME width.  Here the input rows are gathered (lane
// groups own rows as in k_aggregate_group), a block of 64 / 32 aggregated rows is staged in LDS and contracted with W on
// v_mfma_f32_16x16x32_bf16: both operands in three bf16 terms, six products, fp32 accumulators (the arithmetic of
// gn_gemm_f32's tall-skinny kernel; GN_GEMM_ARITH_FAST's two terms are not offered here).  W is split once per
// workgroup into LDS fragments; one persistent workgroup of sixteen waves per compute unit walks the row blocks; per block
// the sixteen (row tile, column tile) products are one per wave (two for 64 -> 128).
// 64 input features: W is 24 KB of fragments, so a workgroup per row block (no persistent loop, no 3.05 blocks in 4 rounds)
// with four row gathers in flight per lane measured 169.3 against 171.6 us on the aminer-syn forward (persistent, eight in
// flight; one block per workgroup with eight: 174); 128 features (96 KB of W) stay persistent
template <int LPE>
__global__ __launch_bounds__(1024) void k_aggregate_mfma(AggArgs a, const float* __restrict__ w, int fout, int row_blocks) {
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    constexpr int FIN = 4 * LPE, S = kWave / LPE, RPI = 16 * S, MT = RPI / 16, CH = FIN / 32, U = LPE == 16 ? GN_MFMA_U16 : 8;
    constexpr int STRIDE = FIN + 4;                            // floats between staged rows: 16 rows of a tile on 16 different bank quads
    extern __shared__ f32x4 lds_mfma[];
    u32x4* wsplit = reinterpret_cast<u32x4*>(lds_mfma);        // [CH][fout / 16][3][64]
    const int nt_all = fout >> 4;
    float* stage0 = reinterpret_cast<float*>(wsplit + (size_t)CH * nt_all * 3 * 64);  // [2][RPI][STRIDE]: blocks alternate, ONE barrier a block
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = lane / LPE, j = lane % LPE;

    auto split3x2 = [](float x0, float x1, uint32_t (&t)[3]) {   // the terms of two values as bf16 pairs, x0 in the low halves
        uint32_t lo[3], hi[3];
        split3(x0, lo);
        split3(x1, hi);
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = __builtin_amdgcn_perm(hi[k], lo[k], 0x07060302u);
    };

    // W as B-operand fragments: lane (n = l & 15, kg = l >> 4) of (chunk, column tile) holds k = 32 chunk + 8 kg .. + 7 of column 16 tile + n
    for (int idx = tid; idx < CH * nt_all * 64; idx += 1024) {
        const int l = idx & 63, t = (idx >> 6) % nt_all, ch = idx / (64 * nt_all);
        const int col = 16 * t + (l & 15), kb = 32 * ch + 8 * (l >> 4);
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = w[(int64_t)(kb + q) * fout + col];
        u32x4 tv[3];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            uint32_t t3[3];
            split3x2(v[2 * h], v[2 * h + 1], t3);
            tv[0][h] = t3[0]; tv[1][h] = t3[1]; tv[2][h] = t3[2];
        }
        u32x4* o = wsplit + ((size_t)(ch * nt_all + t) * 3) * 64 + l;
        o[0] = tv[0]; o[64] = tv[1]; o[128] = tv[2];
    }
    side_copy_stream(a.side, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
    __syncthreads();

    const float* __restrict__ tab = a.table + 4 * j;
    int flip = 0;
    for (int rb = blockIdx.x; rb < row_blocks; rb += gridDim.x, flip ^= 1) {
        // (two staging buffers: a wave that is done with the products of block i gathers block i + 1 at once and writes
        // the other buffer; the buffer of block i - 1 was read by every wave before it arrived at the barrier of block i)
        float* stage = stage0 + (size_t)flip * RPI * STRIDE;
        // ---- gather: this lane group's row of the block (the loop of k_aggregate_group; FIN = 4 LPE, so every lane is active) ----
        const int local = wave * S + slot, row = rb * RPI + local;
        const bool live = row < a.rows;
        const int begin = live ? a.rowptr[row] : 0, end = live ? a.rowptr[row + 1] : 0;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        gather_group_row<RowF32, LPE, U>(a, tab, begin, end, j, true, acc);
        *reinterpret_cast<float4*>(stage + (size_t)local * STRIDE + 4 * j) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        __syncthreads();
        // ---- contract the block with W: (row tile, column tile) products dealt to the waves ----
        const int m = lane & 15, kg = lane >> 4;
        for (int job = wave; job < MT * nt_all; job += 16) {
            const int mt = job % MT, nt = job / MT;
            f32x4 d = (f32x4)(0.f);
            const float* arow = stage + (size_t)(16 * mt + m) * STRIDE + 8 * kg;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(arow + 32 * ch), a1 = *reinterpret_cast<const f32x4*>(arow + 32 * ch + 4);
                u32x4 at[3];
                uint32_t t3[3];
                split3x2(a0[0], a0[1], t3); at[0][0] = t3[0]; at[1][0] = t3[1]; at[2][0] = t3[2];
                split3x2(a0[2], a0[3], t3); at[0][1] = t3[0]; at[1][1] = t3[1]; at[2][1] = t3[2];
                split3x2(a1[0], a1[1], t3); at[0][2] = t3[0]; at[1][2] = t3[1]; at[2][2] = t3[2];
                split3x2(a1[2], a1[3], t3); at[0][3] = t3[0]; at[1][3] = t3[1]; at[2][3] = t3[2];
                const bf16x8 xh = __builtin_bit_cast(bf16x8, at[0]), xm = __builtin_bit_cast(bf16x8, at[1]), xl = __builtin_bit_cast(bf16x8, at[2]);
                const u32x4* bp = wsplit + ((size_t)(ch * nt_all + nt) * 3) * 64 + lane;
                const bf16x8 bh = __builtin_bit_cast(bf16x8, bp[0]), bm = __builtin_bit_cast(bf16x8, bp[64]), bl = __builtin_bit_cast(bf16x8, bp[128]);
                d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, bh, d, 0, 0, 0);     // smallest terms first
                d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, bl, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, bm, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, bh, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, bm, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, bh, d, 0, 0, 0);
            }
            const int col = 16 * nt + m;                       // D: column = lane & 15, rows 4 (lane >> 4) + i
            const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int orow = rb * RPI + 16 * mt + 4 * kg + i;
                if (orow < a.rows) {
                    float val = d[i] + bias;
                    if (a.relu) val = gn::relu_keep_nan(val);
                    a.out[(int64_t)orow * a.ld_out + col] = val;
                }
            }
        }
    }
}

// Many short rows over a SMALL table (the (relation, source) sums of the relational layer's weight gradient: 6 x 10^5
// rows of ~3 edges gathering from the 645 x 32 gradient rows): the table goes into LDS once per workgroup, and a row's
// neighbours cost LDS reads instead of L2 round trips.  LPE lanes own a row (16 bytes of it each), 64 / LPE rows per
// wave side by side; a wave works on two batches of rows at a time and reads the row bounds of the batches after them
// while it does (the chain bounds -> ids -> table would otherwise be paid per batch).  Unit coefficients only.
template <int LPE>
__global__ __launch_bounds__(1024) void k_aggregate_lds_table(AggArgs a) {
    constexpr int S = kWave / LPE;
    extern __shared__ f32x4 tab[];
    const int tid = threadIdx.x, lane = tid & 63, slot = lane / LPE, j = lane % LPE;
    const bool col_live = 4 * j < a.features;
    const int tj = col_live ? j : 0;
    const int units = a.features / 4;                                  // float4 per table row
    const int n_tab = (int)a.table_rows * units;
    // (every workgroup reads the same table at the same time: each starts at its own offset, so that they do not all
    // queue on the same L2 channel)
    const int rot = (int)((blockIdx.x * 977u) % (unsigned)n_tab);
    for (int k = tid; k < n_tab; k += 1024) {
        int i = k + rot;
        i = i < n_tab ? i : i - n_tab;
        const int r = i / units, c = i - r * units;
        tab[i] = *reinterpret_cast<const f32x4*>(a.table + (int64_t)r * a.ld_table + 4 * c);
    }
    if (tid < units) tab[n_tab + tid] = (f32x4){0.f, 0.f, 0.f, 0.f};    // one zero row: what the slots past a row's end read
    __syncthreads();
    const int wave = (int)blockIdx.x * 16 + (tid >> 6), n_waves = (int)gridDim.x * 16;
    const int stride = n_waves * S;
    const uint32_t zero_row = (uint32_t)a.table_rows;
    int rowA = wave * S + slot, rowB = rowA + stride;
    // (every load is unconditional with a clamped index: hipcc waits for conditional loads one by one)
    const int last_row = a.rows - 1, last_id = (int)a.nnz - 1;
    int bA = a.rowptr[min(rowA, last_row)], eA = a.rowptr[min(rowA, last_row) + 1];
    int bB = a.rowptr[min(rowB, last_row)], eB = a.rowptr[min(rowB, last_row) + 1];
    if (rowA >= a.rows) eA = bA;
    if (rowB >= a.rows) eB = bB;
    // software pipeline: the bounds run two pairs of batches ahead of the sums, the first eight ids of every row one
    // pair ahead (the chain bounds -> ids -> table would otherwise be one HBM round trip after the other in every trip).
    // Every lane of a row reads the row's ids itself, eight at a time as two 16-byte loads (4-byte aligned: the plan's
    // id array has eight spare entries): handing them round with ds_bpermute cost more LDS time than the table reads.
    auto ids8 = [&](int first, u32x4& lo, u32x4& hi) {
        const uint32_t* __restrict__ p = a.col + min(first, last_id);
        __builtin_memcpy(&lo, p, 16);
        __builtin_memcpy(&hi, p + 4, 16);
    };
    int nA = rowA + 2 * stride, nB = rowB + 2 * stride;
    int nbA = a.rowptr[min(nA, last_row)], neA = a.rowptr[min(nA, last_row) + 1];
    int nbB = a.rowptr[min(nB, last_row)], neB = a.rowptr[min(nB, last_row) + 1];
    if (nA >= a.rows) neA = nbA;
    if (nB >= a.rows) neB = nbB;
    u32x4 iA0, iA1, iB0, iB1;
    ids8(bA, iA0, iA1);
    ids8(bB, iB0, iB1);
    const uint32_t piece = (uint32_t)tj;
    while (__any(rowA < a.rows)) {
        const int mA = nA + 2 * stride, mB = nB + 2 * stride;
        int mbA = a.rowptr[min(mA, last_row)], meA = a.rowptr[min(mA, last_row) + 1];
        int mbB = a.rowptr[min(mB, last_row)], meB = a.rowptr[min(mB, last_row) + 1];
        if (mA >= a.rows) meA = mbA;
        if (mB >= a.rows) meB = mbB;
        u32x4 jA0, jA1, jB0, jB1;                                      // the next pair's first ids
        ids8(nbA, jA0, jA1);
        ids8(nbB, jB0, jB1);
        f32x4 accA = (f32x4){0.f, 0.f, 0.f, 0.f}, accB = accA;
        // a slot past the row's end names the zero row, so the adds need no predicate
        for (int base = 0; __any(bA + base < eA || bB + base < eB); base += 8) {
            if (base > 0) { ids8(bA + base, iA0, iA1); ids8(bB + base, iB0, iB1); }      // (rows of more than eight edges)
            const int leftA = eA - bA - base, leftB = eB - bB - base;
            f32x4 vA[8], vB[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint32_t ia = t < 4 ? iA0[t & 3] : iA1[t & 3], ib = t < 4 ? iB0[t & 3] : iB1[t & 3];
                vA[t] = tab[(t < leftA ? ia : zero_row) * (uint32_t)units + piece];
                vB[t] = tab[(t < leftB ? ib : zero_row) * (uint32_t)units + piece];
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                accA += vA[t];
                accB += vB[t];
            }
        }
        {
        if (rowA < a.rows && col_live) *reinterpret_cast<f32x4*>(a.out + (int64_t)rowA * a.ld_out + 4 * j) = accA;
        if (rowB < a.rows && col_live) *reinterpret_cast<f32x4*>(a.out + (int64_t)rowB * a.ld_out + 4 * j) = accB;
        }
        rowA = nA; rowB = nB; bA = nbA; eA = neA; bB = nbB; eB = neB;
        nA = mA; nB = mB; nbA = mbA; neA = meA; nbB = mbB; neB = meB;
        iA0 = jA0; iA1 = jA1; iB0 = jB0; iB1 = jB1;
    }
}

// f(std::integral_constant<int, LPE>) for the power of two LPE in [MIN, MAX] that `lpe` names (MAX for anything above):
// a launcher instantiates its kernel for exactly those widths.
template <int MAX, int MIN = 1, typename F>
void dispatch_lpe(int lpe, F&& f) {
    if constexpr (MIN < MAX) {
        if (lpe > MIN) return dispatch_lpe<MAX, 2 * MIN>(lpe, f);
    }
    f(std::integral_constant<int, MIN>{});
}

// ---- one launch function per kernel: the geometry is the route's (gather_route.hpp), nothing is decided here ----
using route::Gather;
using route::GatherRoute;

template <typename Row>
void launch_wave(const AggArgs& a, const GatherRoute& r, hipStream_t st) {
    dispatch_lpe<64>(r.lpe, [&](auto l) { k_aggregate<Row, decltype(l)::value><<<r.grid, r.block, 0, st>>>(a); });
}

template <typename Row>
void launch_group(const AggArgs& a, const GatherRoute& r, hipStream_t st) {
    dispatch_lpe<32>(r.lpe, [&](auto l) { k_aggregate_group<Row, decltype(l)::value, GN_AGG_GROUP_U><<<r.grid, r.block, 0, st>>>(a); });
}

void launch_short(const AggArgs& a, const GatherRoute& r, hipStream_t st) {
    dispatch_lpe<16>(r.lpe, [&](auto l) { k_aggregate_short<decltype(l)::value><<<r.grid, r.block, 0, st>>>(a); });
}

gn_status launch_lds_table(const AggArgs& a, const GatherRoute& r, hipStream_t st) {
    gn_status ls = GN_OK;
    dispatch_lpe<16, 4>(r.lpe, [&](auto l) {
        ls = allow_large_lds(reinterpret_cast<const void*>(k_aggregate_lds_table<decltype(l)::value>), 160 * 1024);
        if (ls == GN_OK) k_aggregate_lds_table<decltype(l)::value><<<r.grid, r.block, r.lds, st>>>(a);
    });
    return ls;
}

gn_status launch_mfma(const AggArgs& a, const GatherRoute& r, const float* w, int fout, hipStream_t st) {
    gn_status ls = GN_OK;
    dispatch_lpe<32, 16>(r.lpe, [&](auto l) {
        ls = allow_large_lds(reinterpret_cast<const void*>(k_aggregate_mfma<decltype(l)::value>), 160 * 1024);
        if (ls == GN_OK) k_aggregate_mfma<decltype(l)::value><<<r.grid, r.block, r.lds, st>>>(a, w, fout, r.row_blocks);
    });
    return ls;
}

gn_status launch_transform(const AggArgs& a, const GatherRoute& r, const float* w, int fout, hipStream_t st) {
    switch (a.features * 100 + fout) {
        case 1616: k_aggregate_transform<4, 16><<<r.grid, r.block, 0, st>>>(a, w); break;
        case 3216: k_aggregate_transform<8, 16><<<r.grid, r.block, 0, st>>>(a, w); break;
        case 6416: k_aggregate_transform<16, 16><<<r.grid, r.block, 0, st>>>(a, w); break;
        case 3232: k_aggregate_transform<8, 32><<<r.grid, r.block, 0, st>>>(a, w); break;
        case 6432: k_aggregate_transform<16, 32><<<r.grid, r.block, 0, st>>>(a, w); break;
        default: return fail(GN_ERR_UNSUPPORTED, "no fused transform for %d -> %d features", a.features, fout);
    }
    return GN_OK;
}

void launch_transform_quad(const AggArgs& a, const GatherRoute& r, const float* w, hipStream_t st) {
    k_aggregate_transform_q<1><<<r.grid, r.block, 0, st>>>(a, w);
}

void launch_transform_tail(const AggArgs& a, const GatherRoute& r, const float* w, const AggTail& tail, hipStream_t st) {
    k_aggregate_transform_tail<<<r.grid, r.block, 0, st>>>(a, w, tail);
}

void launch_transform_split(const AggArgs& a, const GatherRoute& r, const float* w, const AggSplit& split, hipStream_t st) {
    k_aggregate_transform_split<16><<<r.grid, r.block, 0, st>>>(a, w, split);
}

}  // namespace

gn_status launch_split_planes(const float* src, int64_t ld_src, int64_t rows, int cols, int col0, const gn_split_planes& sp,
                              hipStream_t st) {
    k_split_planes<<<stream_grid(rows * cols, 256), 256, 0, st>>>(src, ld_src, rows, cols, col0, sp);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

gn_status launch_gather(const GatherRoute& r, const AggArgs& a, hipStream_t st, const float* w, int fout, const AggTail* tail,
                        const AggSplit* split) {
    gn_status s = GN_OK;
    switch (r.kernel) {
        case Gather::mfma: s = launch_mfma(a, r, w, fout, st); break;
        case Gather::transform: s = launch_transform(a, r, w, fout, st); break;
        case Gather::transform_quad: launch_transform_quad(a, r, w, st); break;
        case Gather::transform_tail: launch_transform_tail(a, r, w, *tail, st); break;
        case Gather::transform_split: launch_transform_split(a, r, w, *split, st); break;
        case Gather::lds_table: s = launch_lds_table(a, r, st); break;
        case Gather::short_rows: launch_short(a, r, st); break;
        case Gather::group: launch_group<RowF32>(a, r, st); break;
        case Gather::wave: launch_wave<RowF32>(a, r, st); break;
        case Gather::wave_scalar: launch_wave<RowScalar>(a, r, st); break;
        case Gather::bf16_group: launch_group<RowBf16>(a, r, st); break;
        case Gather::bf16_wave: launch_wave<RowBf16>(a, r, st); break;
        case Gather::blocked:
        case Gather::refused: return fail(GN_ERR_UNSUPPORTED, "internal: this route has no kernel in aggregate.hip");
    }
    if (s != GN_OK) return s;
    GN_LAUNCH_CHECK();
    return GN_OK;
}

}  // namespace gn
