// The KGE scorers on SHARED candidate lists ('tail-shared' / 'head-shared' of KGEModel.forward): the B positives are cut into G
// chunks of B / G consecutive positives and every chunk comes with ONE list of K candidate entities cand[g, :] that take the
// place of the tail (side 0) or of the head (side 1) of each of its positives - what large-scale KGE trainers (DGL-KE,
// PyTorch-BigGraph) do so that G * K entity rows are gathered instead of B * K.
//
//   g = b / (B / G)    tail side   out[b, k] = s(fixed[b], et[b], cand[g, k])     head side   out[b, k] = s(cand[g, k], et[b], fixed[b])
//
// Forward, k_kge_shared_forward<M, SIDE>.  A workgroup of four waves owns a tile of 64 positives of one chunk (16 query rows
// per wave, as the rank engine has them) and walks the chunk's K candidates in stages of 64 rows held in LDS: a staged
// candidate row is gathered once per workgroup and read by all of its query rows.  The query side is prepared once per
// positive into LDS as well (a list longer than one stage is cut among workgroups - blockIdx.y, each preparing the tile's query
// rows again - while the grid would otherwise stay below two workgroups per compute unit):
//   DistMult, ComplEx   the row q with  s = <q, candidate row>  (dscore of the candidate's role: h r, the complex product h r, or
//                       for the head side r t and its conjugate form), contracted with the staged rows on
//                       v_mfma_f32_16x16x4_f32 - k-ordered chains of fp32 fused multiply-adds over the entity row's columns:
//                       groups of 16 columns go to four partial sums in turn, added pairwise at the end, so a row of 128
//                       floats is four chains of 32 steps and sixteen accumulators (4 partials x 4 column tiles) are in flight;
//   TransE, RotatE      head_part(h, r) for the tail side, the relation operand and the tail for the head side; the vector ALU
//                       evaluates kge_term.cuh's tail_term / term per column, a lane owning 4 query rows x 4 candidates and
//                       adding the columns in ascending order (RotatE's cos / sin come from the [R, H] table of make_tables).
// Padding columns and rows are staged as zeros; their terms are exact zeros for all four models.  A wave's 16 x 64 sums go
// through its own LDS tile so that a lane finishes and stores four neighbouring scores of one row: 16-byte stores when K is a
// multiple of 4 and the outputs are 16-byte aligned, a float at a time otherwise.
//
// Backward, without float atomics and without a host synchronisation (gw = grad_out, times sigma(-s) where the forward
// returned the log-sigmoid, is formed once into scratch):
//   1. query side, k_kge_shared_query: a workgroup per 256 / lanes positives of one chunk (lanes: the power of two that
//      holds H, 16 .. 128), a thread per (positive, column), loops over
//      the chunk's K candidates in ascending k - one fused multiply-add per contribution - and leaves d_fixed[b, :] and
//      d_rel[b, :], one partial row per positive and role;
//   2. candidate side, k_kge_shared_cand: a workgroup per (chunk, 256 / lanes candidates), a thread per (candidate, column), loops
//      over the chunk's B / G positives in ascending b and leaves d_cand[g, k, :], one partial row per list entry;
//   3. three passes of the chunked segmented reduction (seg_reduce.cuh, RowTerm of kge_rows.cuh: the term is the partial row
//      itself, g = 1) add those rows: the G * K candidate rows keyed by cand[g, k] into d_ent, the B query rows keyed by
//      fixed[b] onto it, the B relation rows keyed by et[b] into d_rel.  A candidate that repeats in a list, in two lists, or
//      equals a positive's own entity is just another record of its row.  Rows that nothing touched get the combine's zeros.
// The per-column derivatives are dscore of kge_rows.cuh for all four models: the bilinear models' products g[b, :] C and
// g[:, k]^T Q are formed on the vector ALU in that fixed order.
#include "common.h"
#include "kge_rows.cuh"
#include "rank_engine.cuh"

namespace {

constexpr int kTileRows = kWaves * kRows;      // positives of a workgroup's tile
constexpr int kOutStride = kStage + 4;         // floats per row of a wave's score tile
constexpr int kSharedGridTarget = 512;         // workgroups the forward's grid aims at: two per compute unit of an MI355X
// The backward's partial-row kernels: a row (a positive, or a list entry) has `lanes` lanes - the smallest power of two that
// holds H, 16 .. 128, lane j taking the columns j, j + lanes, ... - and a workgroup 256 / lanes rows: at H = 32 eight rows of
// 32 lanes, every thread one column and ONE pass over the other side.
inline int bwd_lanes(int h) {
    int lanes = 16;
    while (lanes < 128 && lanes < h) lanes <<= 1;
    return lanes;
}
constexpr int kBwdIds = 256;                   // ids staged per trip of the backward loops

template <int M>
constexpr bool kBilinear = M == kDistMult || M == kComplEx;

// parts of a prepared query row: the bilinear models one row of the entity row's width; the distance models head_part's parts
// (tail side) or the relation operand's and the tail's (head side)
template <int M, int SIDE>
constexpr int kQueryParts = kBilinear<M> ? 1 : (SIDE == kTailSide ? Traits<M>::ent_parts : 2 * Traits<M>::ent_parts);

struct SharedShape {
    int hp;          // bilinear: the entity row padded to 16 floats; distance models: H padded to 4
    int qs, cs;      // floats per staged query row / candidate row (16-byte rows, banks shifted by 4)
    size_t lds;
};

SharedShape shared_shape(int model, int side, int h) {
    SharedShape s;
    const int pe = entity_parts(model);
    const bool bilinear = model == kDistMult || model == kComplEx;
    s.hp = bilinear ? (pe * h + 15) / 16 * 16 : (h + 3) / 4 * 4;
    const int qp = bilinear ? 1 : (side == kTailSide ? pe : 2 * pe);
    s.qs = qp * s.hp + 4;
    s.cs = (bilinear ? 1 : pe) * s.hp + 4;
    s.lds = ((size_t)kTileRows * s.qs + (size_t)kStage * s.cs + (size_t)kWaves * kRows * kOutStride + 5 * 64) * sizeof(float);
    return s;
}

struct SharedFwdArgs {
    Tables t;
    const int64_t* fixed; const int64_t* et; const int64_t* cand; int64_t ld_cand;
    int64_t b, k; int chunk, tiles;                // positives of a chunk; tiles of kTileRows positives per chunk
    int64_t span;                                  // candidates of a list that one workgroup walks (a multiple of kStage): blockIdx.y
    int hp, qs, cs;
    float gamma; int log_sigmoid; int vec_out;
    float* out; float* raw; int32_t* err;
};

template <int M, int SIDE>
__global__ __launch_bounds__(256) void k_kge_shared_forward(SharedFwdArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int PE = Traits<M>::ent_parts;
    constexpr int CAND_ROLE = SIDE == kTailSide ? kTail : kHead;
    float* qs = reinterpret_cast<float*>(lds_raw);                       // [kTileRows][a.qs]
    float* cs = qs + kTileRows * a.qs;                                    // [kStage][a.cs]
    float* ot = cs + kStage * a.cs;                                       // [kWaves][kRows][kOutStride]
    int* q_ok = reinterpret_cast<int*>(ot + kWaves * kRows * kOutStride); // [64] each
    int* q_fixed = q_ok + 64;
    int* q_rel = q_fixed + 64;
    int* c_ok = q_rel + 64;
    int* c_id = c_ok + 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, kq = lane >> 4;
    const int h = a.t.h, hp = a.hp, QS = a.qs, CS = a.cs;
    const int64_t g = blockIdx.x / a.tiles;
    const int r0 = (int)(blockIdx.x % a.tiles) * kTileRows;               // first positive of the tile inside its chunk
    const int64_t b0 = g * a.chunk + r0;
    const int rows = min(kTileRows, a.chunk - r0);

    if (tid < 64) {
        bool ok = false;
        int64_t qf = 0, qr = 0;
        if (tid < rows) {
            qf = a.fixed[b0 + tid]; qr = a.et[b0 + tid];
            ok = in_tables(a.t, qf, qf, qr);
        }
        q_ok[tid] = ok ? 1 : 0;
        q_fixed[tid] = ok ? (int)qf : 0;                                 // validated: the tables have fewer than 2^31 rows
        q_rel[tid] = ok ? (int)qr : 0;
    }
    __syncthreads();
    // the prepared query rows
    if constexpr (kBilinear<M>) {
        const int d = PE * h;
        for (int idx = tid; idx < kTileRows * hp; idx += 256) {
            const int row = idx / hp, f = idx - row * hp;
            float v = 0.f;
            if (f < d && q_ok[row]) {
                const int x = f < h ? f : f - h;
                float fr[1], fi[1], rr[1], ri[1];
                load_entity<M, 1>(a.t, q_fixed[row], x, fr, fi);
                load_relation<M, 1>(a.t, q_rel[row], x, rr, ri);
                const Col c = SIDE == kTailSide ? Col{fr[0], fi[0], rr[0], ri[0], 0.f, 0.f} : Col{0.f, 0.f, rr[0], ri[0], fr[0], fi[0]};
                float d0, d1;
                dscore<M, CAND_ROLE>(c, 1.0f, d0, d1);                   // ds / d(candidate row): s = <that, the candidate row>
                v = f < h ? d0 : d1;
            }
            qs[row * QS + f] = v;
        }
    } else {
        for (int idx = tid; idx < kTileRows * hp; idx += 256) {
            const int row = idx / hp, x = idx - row * hp;
            float fr[1] = {0.f}, fi[1] = {0.f}, rr[1] = {0.f}, ri[1] = {0.f};
            if (x < h && q_ok[row]) {
                load_entity<M, 1>(a.t, q_fixed[row], x, fr, fi);
                load_relation<M, 1>(a.t, q_rel[row], x, rr, ri);
            }
            float* q = qs + row * QS + x;
            if constexpr (SIDE == kTailSide) {
                float p0 = 0.f, p1 = 0.f;
                if (x < h && q_ok[row]) head_part<M>(Col{fr[0], fi[0], rr[0], ri[0], 0.f, 0.f}, p0, p1);
                q[0] = p0;
                if constexpr (PE == 2) q[hp] = p1;
            } else {
                q[0] = rr[0];
                if constexpr (PE == 2) q[hp] = ri[0];
                q[PE * hp] = fr[0];
                if constexpr (PE == 2) q[(PE + 1) * hp] = fi[0];
            }
        }
    }

    float* tile = ot + wave * (kRows * kOutStride);
    const int64_t k_begin = blockIdx.y * a.span, k_end = min(a.k, k_begin + a.span);
    for (int64_t k0 = k_begin; k0 < k_end; k0 += kStage) {
        const int cnt = (int)min((int64_t)kStage, a.k - k0);
        __syncthreads();                                                  // the previous stage is consumed (and the query rows are written)
        if (tid < 64) {
            int64_t cc = -1;
            if (tid < cnt) cc = a.cand[g * a.ld_cand + k0 + tid];
            const bool ok = (uint64_t)cc < (uint64_t)a.t.n;
            c_ok[tid] = ok ? 1 : 0;
            c_id[tid] = ok ? (int)cc : 0;
        }
        __syncthreads();
        {
            const int cw = CS - 4;                                        // staged floats of a candidate row
            for (int idx = tid; idx < kStage * cw; idx += 256) {
                const int c = idx / cw, f = idx - c * cw;
                float v = 0.f;
                if (c_ok[c]) {
                    const float* row = a.t.ent + (int64_t)c_id[c] * a.t.ld_ent;
                    if constexpr (kBilinear<M>) {
                        if (f < PE * h) v = row[f];
                    } else {
                        const int p = f / hp, x = f - p * hp;
                        if (x < h) v = row[p * h + x];
                    }
                }
                cs[c * CS + f] = v;
            }
        }
        __syncthreads();

        // this lane's sums: query rows 4 kq + j of the wave, candidates 16 t + col of the stage
        if constexpr (kBilinear<M>) {
            // MFMA step s contracts the features kq * S + s.  The steps go in groups of four (one float4 of either operand) to
            // four partial sums in turn - group i to partial i % 4 - so that a row of 128 floats is four chains of 32 fused
            // multiply-adds, not one of 128 (and sixteen accumulators are in flight); the partials are added pairwise.
            const int S = hp / 4;
            f32x4 acc[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* arow = qs + (wave * kRows + col) * QS + kq * S;
            const float* brow = cs + col * CS + kq * S;
            for (int base = 0; base < S; base += 16) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int s4 = base + 4 * u;
                    if (s4 >= S) continue;                                // workgroup-uniform
                    const float4 av = *reinterpret_cast<const float4*>(arow + s4);
                    float4 bv[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) bv[t] = *reinterpret_cast<const float4*>(brow + 16 * t * CS + s4);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[u][t] = mfma4(av.x, bv[t].x, acc[u][t]);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[u][t] = mfma4(av.y, bv[t].y, acc[u][t]);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[u][t] = mfma4(av.z, bv[t].z, acc[u][t]);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[u][t] = mfma4(av.w, bv[t].w, acc[u][t]);
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 sum = (acc[0][t] + acc[1][t]) + (acc[2][t] + acc[3][t]);
#pragma unroll
                for (int j = 0; j < 4; ++j) tile[(4 * kq + j) * kOutStride + 16 * t + col] = sum[j];
            }
        } else {
            float acc[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[j][t] = 0.f;
            const float* qrow = qs + (wave * kRows + 4 * kq) * QS;
            const float* crow = cs + col * CS;
            for (int x4 = 0; x4 < hp; x4 += 4) {
                float c0[4][4], c1[4][4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float4 v0 = *reinterpret_cast<const float4*>(crow + 16 * t * CS + x4);
                    float4 v1 = v0;
                    if constexpr (PE == 2) v1 = *reinterpret_cast<const float4*>(crow + 16 * t * CS + hp + x4);
                    c0[t][0] = v0.x; c0[t][1] = v0.y; c0[t][2] = v0.z; c0[t][3] = v0.w;
                    c1[t][0] = v1.x; c1[t][1] = v1.y; c1[t][2] = v1.z; c1[t][3] = v1.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* q = qrow + j * QS + x4;
                    float qa[4][4];                                       // the row's parts at these four columns
#pragma unroll
                    for (int p = 0; p < kQueryParts<M, SIDE>; ++p) {
                        const float4 v = *reinterpret_cast<const float4*>(q + p * hp);
                        qa[p][0] = v.x; qa[p][1] = v.y; qa[p][2] = v.z; qa[p][3] = v.w;
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (16 * t >= cnt) continue;                      // wave-uniform
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            if constexpr (SIDE == kTailSide) {
                                acc[j][t] += tail_term<M>(qa[0][v], PE == 2 ? qa[PE - 1][v] : 0.f, c0[t][v], c1[t][v]);
                            } else {
                                const Col c = {c0[t][v], c1[t][v], qa[0][v], PE == 2 ? qa[PE - 1][v] : 0.f, qa[PE][v],
                                               PE == 2 ? qa[2 * PE - 1][v] : 0.f};
                                acc[j][t] += term<M>(c);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) tile[(4 * kq + j) * kOutStride + 16 * t + col] = acc[j][t];
        }
        wave_sync();
        // the epilogue: lane (row 4 i + kq, columns 4 col .. 4 col + 3) of the wave's tile
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * i + kq, c4 = 4 * col;
            const int row = wave * kRows + r;
            if (row >= rows || c4 >= cnt) continue;
            const float4 sum = *reinterpret_cast<const float4*>(tile + r * kOutStride + c4);
            const float s[4] = {sum.x, sum.y, sum.z, sum.w};
            float res[4], fin[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const bool ok = q_ok[row] != 0 && c_ok[c4 + v] != 0;     // (columns behind cnt are never stored)
                fin[v] = ok ? finish<M>(s[v], a.gamma) : __builtin_nanf("");
                res[v] = a.log_sigmoid ? log_sigmoid(fin[v]) : fin[v];
                bad = bad || (!ok && c4 + v < cnt);
            }
            const int64_t at = (b0 + row) * a.k + k0 + c4;
            if (a.vec_out) {
                *reinterpret_cast<float4*>(a.out + at) = make_float4(res[0], res[1], res[2], res[3]);
                if (a.raw) *reinterpret_cast<float4*>(a.raw + at) = make_float4(fin[0], fin[1], fin[2], fin[3]);
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (c4 + v < cnt) {
                        a.out[at + v] = res[v];
                        if (a.raw) a.raw[at + v] = fin[v];
                    }
                }
            }
        }
        if (bad && a.err) atomicOr(a.err, 1);
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct SharedBwdCall : BwdFrame {
    int side;
    const int64_t* fixed; const int64_t* et; const int64_t* cand; int64_t ld_cand; int64_t b, k, g; int chunk;
    const float* gw;                               // [B, K]: the upstream with the log-sigmoid's factor
    float* q_ent; float* q_rel; float* c_ent;      // partial rows [B, De], [B, Dr], [G * K, De]
    int64_t de, dr;
};

__global__ void k_kge_shared_upstream(const float* __restrict__ grad_out, const float* __restrict__ raw, int64_t count,
                                      float* __restrict__ gw) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x)
        gw[e] = upstream(grad_out, raw, e);
}

struct SharedPartArgs {
    Tables t;
    const int64_t* fixed; const int64_t* et; const int64_t* cand; int64_t ld_cand; int64_t k; int chunk; int tiles; int lanes;
    const float* gw; float divisor;
    float* q_ent; float* q_rel; float* c_ent; int64_t de, dr;
};

// the column's Col of (fixed entity, relation operand, candidate) by the side
template <int SIDE>
__device__ __forceinline__ Col shared_col(float fr, float fi, float rr, float ri, float cr, float ci) {
    return SIDE == kTailSide ? Col{fr, fi, rr, ri, cr, ci} : Col{cr, ci, rr, ri, fr, fi};
}

// Query side: blockIdx = (chunk, tile of 256 / lanes positives); thread (p, j) sums, for the columns j, j + lanes, ... of positive p,
// gw[b, k] * ds / d(fixed row) and gw[b, k] * ds / d(relation row) over k = 0, 1, ... in that order.
template <int M, int SIDE>
__global__ __launch_bounds__(256) void k_kge_shared_query(SharedPartArgs a) {
    constexpr int PE = Traits<M>::ent_parts, PR = Traits<M>::rel_parts;
    constexpr int FIXED_ROLE = SIDE == kTailSide ? kHead : kTail;
    __shared__ int ids[kBwdIds];                   // the list's entries of this trip; -1: outside the table
    const int j = threadIdx.x % a.lanes, p = threadIdx.x / a.lanes;
    const int64_t g = blockIdx.x / a.tiles;
    const int r = (int)(blockIdx.x % a.tiles) * (256 / a.lanes) + p;
    const bool row = r < a.chunk;
    const int64_t b = g * a.chunk + (row ? r : 0);
    const int64_t qf = a.fixed[b], qr = a.et[b];
    const bool q_ok = row && in_tables(a.t, qf, qf, qr);
    const int fixed = q_ok ? (int)qf : 0, rel = q_ok ? (int)qr : 0;
    const int h = a.t.h;
    for (int x0 = 0; x0 < h; x0 += a.lanes) {                          // workgroup-uniform
        const int x = x0 + j;
        const bool live_col = x < h;
        const int xc = live_col ? x : 0;
        float fr[1], fi[1], rr[1], ri[1];
        load_entity<M, 1>(a.t, fixed, xc, fr, fi);
        load_relation<M, 1>(a.t, rel, xc, rr, ri);
        float acc_e[PE][1], acc_r[PR][1];
#pragma unroll
        for (int q = 0; q < PE; ++q) acc_e[q][0] = 0.f;
#pragma unroll
        for (int q = 0; q < PR; ++q) acc_r[q][0] = 0.f;
        for (int64_t k0 = 0; k0 < a.k; k0 += kBwdIds) {
            const int cnt = (int)min((int64_t)kBwdIds, a.k - k0);
            __syncthreads();                                              // the previous trip is done with `ids`
            if ((int)threadIdx.x < cnt) {
                const int64_t cc = a.cand[g * a.ld_cand + k0 + threadIdx.x];
                ids[threadIdx.x] = (uint64_t)cc < (uint64_t)a.t.n ? (int)cc : -1;
            }
            __syncthreads();
            if (!q_ok) continue;
#pragma unroll 4                                                        // four rows' loads in flight; the additions keep their order
            for (int i = 0; i < cnt; ++i) {
                const int cc = ids[i];
                const bool live = cc >= 0;
                const float gk = a.gw[b * a.k + k0 + i];
                float cr[1], ci[1];
                load_entity<M, 1>(a.t, live ? cc : 0, xc, cr, ci);
                const Col c = shared_col<SIDE>(fr[0], fi[0], rr[0], ri[0], cr[0], ci[0]);
                float de[PE][1], dr[PR][1], d0, d1;
                dscore<M, FIXED_ROLE>(c, a.divisor, d0, d1);
                de[0][0] = d0;
                if constexpr (PE == 2) de[1][0] = d1;
                dscore<M, kRelation>(c, a.divisor, d0, d1);
                dr[0][0] = d0;
                if constexpr (PR == 2) dr[1][0] = d1;
                gn::seg_add<true>(acc_e, gk, de, live);
                gn::seg_add<true>(acc_r, gk, dr, live);
            }
        }
        if (row && live_col) {
#pragma unroll
            for (int q = 0; q < PE; ++q) a.q_ent[b * a.de + (int64_t)q * h + x] = acc_e[q][0];
#pragma unroll
            for (int q = 0; q < PR; ++q) a.q_rel[b * a.dr + (int64_t)q * h + x] = acc_r[q][0];
        }
    }
}

// Candidate side: blockIdx = (chunk, tile of 256 / lanes candidates); thread (p, j) sums, for the columns j, j + lanes, ... of list
// entry (g, k), gw[b, k] * ds / d(candidate row) over the chunk's positives b in ascending order.
template <int M, int SIDE>
__global__ __launch_bounds__(256) void k_kge_shared_cand(SharedPartArgs a) {
    constexpr int PE = Traits<M>::ent_parts;
    constexpr int CAND_ROLE = SIDE == kTailSide ? kTail : kHead;
    __shared__ int fixed_ids[kBwdIds], rel_ids[kBwdIds];  // the positives of this trip; fixed -1: an id outside its table
    const int j = threadIdx.x % a.lanes, p = threadIdx.x / a.lanes;
    const int64_t g = blockIdx.x / a.tiles;
    const int64_t k = (int64_t)(blockIdx.x % a.tiles) * (256 / a.lanes) + p;
    const bool row = k < a.k;
    const int64_t cc = a.cand[g * a.ld_cand + (row ? k : 0)];
    const bool c_ok = row && (uint64_t)cc < (uint64_t)a.t.n;
    const int cand = c_ok ? (int)cc : 0;
    const int h = a.t.h;
    const int64_t b0 = g * a.chunk;
    for (int x0 = 0; x0 < h; x0 += a.lanes) {                          // workgroup-uniform
        const int x = x0 + j;
        const bool live_col = x < h;
        const int xc = live_col ? x : 0;
        float cr[1], ci[1];
        load_entity<M, 1>(a.t, cand, xc, cr, ci);
        float acc[PE][1];
#pragma unroll
        for (int q = 0; q < PE; ++q) acc[q][0] = 0.f;
        for (int i0 = 0; i0 < a.chunk; i0 += kBwdIds) {
            const int cnt = min(kBwdIds, a.chunk - i0);
            __syncthreads();                                              // the previous trip is done with the ids
            if ((int)threadIdx.x < cnt) {
                const int64_t qf = a.fixed[b0 + i0 + threadIdx.x], qr = a.et[b0 + i0 + threadIdx.x];
                const bool ok = in_tables(a.t, qf, qf, qr);
                fixed_ids[threadIdx.x] = ok ? (int)qf : -1;
                rel_ids[threadIdx.x] = ok ? (int)qr : 0;
            }
            __syncthreads();
            if (!c_ok) continue;
#pragma unroll 4                                                        // four rows' loads in flight; the additions keep their order
            for (int i = 0; i < cnt; ++i) {
                const int ff = fixed_ids[i];
                const bool live = ff >= 0;
                const float gk = a.gw[(b0 + i0 + i) * a.k + k];
                float fr[1], fi[1], rr[1], ri[1];
                load_entity<M, 1>(a.t, live ? ff : 0, xc, fr, fi);
                load_relation<M, 1>(a.t, rel_ids[i], xc, rr, ri);
                const Col c = shared_col<SIDE>(fr[0], fi[0], rr[0], ri[0], cr[0], ci[0]);
                float d[PE][1], d0, d1;
                dscore<M, CAND_ROLE>(c, a.divisor, d0, d1);
                d[0][0] = d0;
                if constexpr (PE == 2) d[1][0] = d1;
                gn::seg_add<true>(acc, gk, d, live);
            }
        }
        if (row && live_col) {
#pragma unroll
            for (int q = 0; q < PE; ++q) a.c_ent[(g * a.k + k) * a.de + (int64_t)q * h + x] = acc[q][0];
        }
    }
}

// one record per list entry for the pass that adds the candidates' partial rows: h = the entry (its partial row), t = its entity
struct ListSrc {
    const int64_t* cand; int64_t ld_cand, k;
    __device__ bool get(int64_t e, const Tables& t, Rec& rec) const {
        const int64_t cc = cand[(e / k) * ld_cand + e % k];
        if ((uint64_t)cc >= (uint64_t)t.n) return false;
        rec = {(uint32_t)e, (uint32_t)cc, 0u, 1.0f};
        return true;
    }
};

// The backward's scratch: one reduction's over max(B, G * K) records; in its tail RotatE's cos / sin tables, the partial rows
// [B, De], [B, Dr] and [G * K, De] and the upstream [B, K]; the chunk partials are sized for chunks of kRowChunkRecs records.
gn::SegLayout shared_ws_layout(int model, int64_t n, int64_t r, int64_t h, int64_t b, int64_t g, int64_t k) {
    const int64_t de = entity_parts(model) * h, dr = relation_parts(model) * h;
    const int64_t most = std::max(b, g * k), least = std::min(b, g * k);
    const size_t tail = trig_bytes(model, r, h) + rows_bytes(b, de) + rows_bytes(b, dr) + rows_bytes(g * k, de) + rows_bytes(b, k);
    return gn::seg_layout<Rec>(most, std::max(n, r), 2, tail, kRowChunkRecs, least);
}

// `count` partial rows `rows` [count, parts * h] from `src`, added per key of `role` into o
template <typename Src>
gn_status partial_row_pass(const SharedBwdCall& c, const gn::SegWs<Rec>& w, const Src& src, int role, int64_t count,
                           const int64_t* sorted_types, const gn::SegOut& o, const float* rows, int64_t ld) {
    return record_pass(c, w, src, role, count, sorted_types, o,
                       [&](const gn::SegFrame<Rec>& f, int, unsigned chunks) {
                           with_flag(o.parts == 2, [&](auto two) {
                               launch_seg_reduce<RowTerm<decltype(two)::value ? 2 : 1>, kRowChunkRecs>({rows, ld, c.t.h}, f, c.vec, c.lpe, chunks, c.st);
                           });
                       },
                       kRowChunkRecs);
}

gn_status partial_rows(const SharedBwdCall& c) {
    SharedPartArgs a = {c.t, c.fixed, c.et, c.cand, c.ld_cand, c.k, c.chunk, 0, bwd_lanes(c.t.h), c.gw, c.divisor, c.q_ent, c.q_rel, c.c_ent, c.de, c.dr};
    SharedPartArgs q = a, k = a;
    const int rows = 256 / a.lanes;
    q.tiles = (int)gn::ceil_div((int64_t)c.chunk, (int64_t)rows);
    k.tiles = (int)gn::ceil_div(c.k, (int64_t)rows);
    with_model(c.model, [&](auto m) {
        with_flag(c.side == kHeadSide, [&](auto head) {
            constexpr int SIDE = decltype(head)::value ? kHeadSide : kTailSide;
            k_kge_shared_query<decltype(m)::value, SIDE><<<(unsigned)(c.g * q.tiles), 256, 0, c.st>>>(q);
            k_kge_shared_cand<decltype(m)::value, SIDE><<<(unsigned)(c.g * k.tiles), 256, 0, c.st>>>(k);
        });
    });
    GN_LAUNCH_CHECK();
    return GN_OK;
}

gn_status check_shared(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel, int64_t r, int64_t h,
                       int64_t b, int64_t g, int64_t k, int64_t ld_cand, int side) {
    GN_REQUIRE(side == kTailSide || side == kHeadSide, "unknown side %d (0 tail, 1 head)", side);
    GN_REQUIRE(b >= 0 && g >= 0 && k >= 0, "negative size");
    GN_REQUIRE(b == 0 || (g >= 1 && g <= b && b % g == 0), "%lld candidate lists do not divide %lld positives into equal chunks",
               (long long)g, (long long)b);
    if (b >= (1ll << 31) || k >= (1ll << 31) || (double)b * (double)k >= (double)(1ll << 40))
        return gn::fail(GN_ERR_UNSUPPORTED, "the score block is beyond the 32-bit record encoding");
    GN_OK_OR_RETURN(check_shapes(model, ent, ld_ent, n, rel, ld_rel, r, h, std::max(b, g * k)));
    if (entity_parts(model) * h > kMaxFeatures)
        return gn::fail(GN_ERR_UNSUPPORTED, "the shared-list kernels take entity rows of at most %d floats (got %lld)", kMaxFeatures,
                        (long long)(entity_parts(model) * h));
    GN_REQUIRE(ld_cand >= k, "leading dimension of the candidates smaller than K");
    return GN_OK;
}

template <int M, int SIDE>
gn_status launch_forward(const SharedFwdArgs& a, const SharedShape& s, int64_t g, hipStream_t st) {
    auto kernel = &k_kge_shared_forward<M, SIDE>;
    if (s.lds > 64 * 1024) {                                  // (the opt-in is made once per kernel: for the widest row)
        const int widest = kMaxFeatures / Traits<M>::ent_parts;
        GN_OK_OR_RETURN(gn::allow_large_lds(reinterpret_cast<const void*>(kernel), (int)shared_shape(M, SIDE, widest).lds));
    }
    kernel<<<dim3((unsigned)(g * a.tiles), (unsigned)gn::ceil_div(a.k, a.span)), 256, s.lds, st>>>(a);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

}  // namespace

extern "C" size_t gn_kge_shared_forward_workspace_bytes(int model, int64_t r, int64_t h) {
    if (r < 0 || h < 0) return 0;
    return trig_bytes(model, r, h);
}

extern "C" gn_status gn_kge_shared_forward_f32(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                               int64_t r, int64_t h, const int64_t* fixed, const int64_t* et, const int64_t* cand,
                                               int64_t ld_cand, int64_t b, int64_t g, int64_t k, int side, float gamma,
                                               float phase_divisor, int log_sigmoid_out, float* out, float* raw_out, int32_t* err,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    GN_OK_OR_RETURN(check_shared(model, ent, ld_ent, n, rel, ld_rel, r, h, b, g, k, ld_cand, side));
    if (b == 0 || k == 0) return GN_OK;
    GN_REQUIRE(fixed && et && cand && out, "operand pointer is null");
    hipStream_t st = gn::as_stream(stream);
    SharedFwdArgs a;
    GN_OK_OR_RETURN(make_tables(a.t, model, ent, ld_ent, n, rel, ld_rel, r, h, phase_divisor, workspace, workspace_bytes, st));
    const SharedShape s = shared_shape(model, side, (int)h);
    a.fixed = fixed; a.et = et; a.cand = cand; a.ld_cand = ld_cand; a.b = b; a.k = k;
    a.chunk = (int)(b / g); a.tiles = (int)gn::ceil_div((int64_t)a.chunk, (int64_t)kTileRows);
    // a list is cut among workgroups (each prepares the tile's query rows again) while the grid is below two workgroups per
    // compute unit: B = 1,024 positives are 16 tiles only
    const int64_t stages = gn::ceil_div(k, (int64_t)kStage);
    a.span = kStage * std::max<int64_t>(1, std::min(stages, stages * g * a.tiles / kSharedGridTarget));
    a.hp = s.hp; a.qs = s.qs; a.cs = s.cs;
    a.gamma = gamma; a.log_sigmoid = log_sigmoid_out; a.out = out; a.raw = raw_out; a.err = err;
    a.vec_out = k % 4 == 0 && gn::aligned16(out) && (raw_out == nullptr || gn::aligned16(raw_out));
    return with_model(model, [&](auto m) {
        return with_flag(side == kHeadSide, [&](auto head) {
            return launch_forward<decltype(m)::value, decltype(head)::value ? kHeadSide : kTailSide>(a, s, g, st);
        });
    });
}

extern "C" size_t gn_kge_shared_backward_workspace_bytes(int model, int64_t n, int64_t r, int64_t h, int64_t b, int64_t g, int64_t k) {
    if (n < 0 || r < 0 || h < 0 || b <= 0 || g <= 0 || k <= 0 || b >= (1ll << 31) || k >= (1ll << 31) || g > b) return 0;
    return shared_ws_layout(model, n, r, h, b, g, k).total;
}

extern "C" gn_status gn_kge_shared_backward_f32(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                                int64_t r, int64_t h, const int64_t* fixed, const int64_t* et, const int64_t* cand,
                                                int64_t ld_cand, int64_t b, int64_t g, int64_t k, int side, float phase_divisor,
                                                const float* grad_out, const float* raw_scores, float* d_ent, int64_t ld_dent,
                                                float* d_rel, int64_t ld_drel, int flags, void* workspace, size_t workspace_bytes,
                                                void* stream) {
    GN_OK_OR_RETURN(check_shared(model, ent, ld_ent, n, rel, ld_rel, r, h, b, g, k, ld_cand, side));
    const bool empty = b == 0 || k == 0 || h == 0;          // gradients of an empty sum
    SharedBwdCall c;
    gn::SegLayout l;
    GN_OK_OR_RETURN(backward_frame(c, l, model, ent, ld_ent, n, rel, ld_rel, r, h, empty, fixed && et && cand, phase_divisor, grad_out,
                                   raw_scores, d_ent, ld_dent, d_rel, ld_drel, flags, workspace, workspace_bytes,
                                   [&] { return shared_ws_layout(model, n, r, h, b, g, k); }, gn::as_stream(stream)));
    if (empty) return GN_OK;
    c.side = side; c.fixed = fixed; c.et = et; c.cand = cand; c.ld_cand = ld_cand; c.b = b; c.k = k; c.g = g; c.chunk = (int)(b / g);
    c.de = entity_parts(model) * h; c.dr = relation_parts(model) * h;
    char* at = static_cast<char*>(workspace) + l.tail + trig_bytes(model, r, h);
    c.q_ent = reinterpret_cast<float*>(at); at += rows_bytes(b, c.de);
    c.q_rel = reinterpret_cast<float*>(at); at += rows_bytes(b, c.dr);
    c.c_ent = reinterpret_cast<float*>(at); at += rows_bytes(g * k, c.de);
    float* gw = reinterpret_cast<float*>(at);
    const gn::SegWs<Rec> w(static_cast<char*>(workspace), l);
    if (raw_scores) {
        k_kge_shared_upstream<<<gn::stream_grid(b * k, 256), 256, 0, c.st>>>(grad_out, raw_scores, b * k, gw);
        GN_LAUNCH_CHECK();
        c.gw = gw;
    } else {
        c.gw = grad_out;
    }
    GN_OK_OR_RETURN(partial_rows(c));
    const int pe = entity_parts(model), pr = relation_parts(model);
    GN_OK_OR_RETURN(partial_row_pass(c, w, ListSrc{cand, ld_cand, k}, kTail, g * k, nullptr, {d_ent, ld_dent, c.t.h, pe, 0}, c.c_ent, c.de));
    GN_OK_OR_RETURN(partial_row_pass(c, w, RowSrc{fixed, et}, kTail, b, nullptr, {d_ent, ld_dent, c.t.h, pe, 1}, c.q_ent, c.de));
    return partial_row_pass(c, w, RowSrc{fixed, et}, kRelation, b, c.types_sorted ? et : nullptr, {d_rel, ld_drel, c.t.h, pr, 0}, c.q_rel, c.dr);
}
