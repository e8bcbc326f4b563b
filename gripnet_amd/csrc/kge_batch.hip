// The KGE scorers on candidate blocks ('head-batch' / 'tail-batch' of KGEModel.forward,
// baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:127-136, :150-173): a positive (fixed[b], et[b]) comes with K
// candidate entities cand[b, :] that take the place of its tail (side 0) or of its head (side 1).
//
//   tail side   out[b, k] = s(fixed[b], et[b], cand[b, k])          head side   out[b, k] = s(cand[b, k], et[b], fixed[b])
//
// Forward.  A work item is one positive and 64 of its candidates; a wave takes one item at a time.  The wave reads the 64
// candidate ids in one coalesced load, and its lanes keep their own columns of the query side in registers for the item
// when a lane owns one unit of the row (rows of up to 64 floats on the float4 path): head_part(h, r) on the tail side, the
// relation operand and the tail's columns on the head side.  Only candidate rows are gathered.  Wider rows read the query's
// columns again per candidate (from L1).  The lane group per score, the order of the units in a lane, term / head_part /
// tail_term, the xor fold and finish are those of k_kge_forward (kge.hip): a score is bit for bit what the list kernel
// gives for that triple.  With fewer than 64 candidates the item's last lanes idle; positives are not packed into a wave.
//
// Backward, without float atomics:
//   1. candidate side: B * K records (h, t, r, g) keyed by the candidate, through seg_pass with the list kernels' KgeTerm;
//   2. query side and relation: k_kge_batch_query, a workgroup per positive, sums g[b, k] * ds / d(fixed row) and
//      g[b, k] * ds / d(relation row) over k with the query's columns in registers - a thread (slot, lane) takes
//      k = slot, slot + S, ... in that order, the S slots are folded in slot order - into one partial row per positive and role;
//   3. two seg_pass calls over B records keyed by fixed[b] and et[b] add those rows (RowTerm: the term is the partial row
//      itself, g = 1: the fused multiply-add by 1 is exact); the entity one accumulates onto the candidate pass.
#include "common.h"
#include "kge_rows.cuh"

namespace {

enum { kTailSide = GN_KGE_SIDE_TAIL, kHeadSide = GN_KGE_SIDE_HEAD };

// the VEC columns [k, k + VEC) of an entity row, real and imaginary member
template <int M, int VEC>
__device__ __forceinline__ void load_entity(const Tables& t, int row, int k, float (&re)[VEC], float (&im)[VEC]) {
    const float* p = t.ent + (int64_t)row * t.ld_ent + k;
    constexpr bool two = Traits<M>::ent_parts == 2;
    if constexpr (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        float4 ai = a;
        if constexpr (two) ai = *reinterpret_cast<const float4*>(p + t.h);
        re[0] = a.x; re[1] = a.y; re[2] = a.z; re[3] = a.w;
        im[0] = ai.x; im[1] = ai.y; im[2] = ai.z; im[3] = ai.w;
    } else {
        re[0] = p[0];
        im[0] = two ? p[t.h] : 0.f;
    }
}

// the same columns of a relation's operand (RotatE: cos, sin)
template <int M, int VEC>
__device__ __forceinline__ void load_relation(const Tables& t, int row, int k, float (&re)[VEC], float (&im)[VEC]) {
    const float* p = t.rel + (int64_t)row * t.ld_rel + k;
    const float* pi = t.rel_im + (int64_t)row * t.ld_rel + k;
    constexpr bool two = Traits<M>::ent_parts == 2;
    if constexpr (VEC == 4) {
        const float4 w = *reinterpret_cast<const float4*>(p);
        float4 wi = w;
        if constexpr (two) wi = *reinterpret_cast<const float4*>(pi);
        re[0] = w.x; re[1] = w.y; re[2] = w.z; re[3] = w.w;
        im[0] = wi.x; im[1] = wi.y; im[2] = wi.z; im[3] = wi.w;
    } else {
        re[0] = p[0];
        im[0] = two ? pi[0] : 0.f;
    }
}

// A lane's share of the query side for one unit: SIDE tail - head_part(h, r); SIDE head - the relation operand and the tail.
template <int VEC>
struct Query { float a0[VEC], a1[VEC], b0[VEC], b1[VEC]; };

template <int M, int VEC, int SIDE>
__device__ __forceinline__ void load_query(const Tables& t, int fixed, int rel, int k, Query<VEC>& q) {
    load_relation<M, VEC>(t, rel, k, q.a0, q.a1);
    load_entity<M, VEC>(t, fixed, k, q.b0, q.b1);
    if constexpr (SIDE == kTailSide) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const Col c = {q.b0[v], q.b1[v], q.a0[v], q.a1[v], 0.f, 0.f};
            head_part<M>(c, q.a0[v], q.a1[v]);
        }
    }
}

// sum over the unit's VEC columns of the candidate's terms, added to acc in column order
template <int M, int VEC, int SIDE>
__device__ __forceinline__ float add_terms(const Tables& t, const Query<VEC>& q, int cand, int k, float acc) {
    float cr[VEC], ci[VEC];
    load_entity<M, VEC>(t, cand, k, cr, ci);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        if constexpr (SIDE == kTailSide) {
            acc += tail_term<M>(q.a0[v], q.a1[v], cr[v], ci[v]);
        } else {
            const Col c = {cr[v], ci[v], q.a0[v], q.a1[v], q.b0[v], q.b1[v]};
            acc += term<M>(c);
        }
    }
    return acc;
}

struct FwdArgs {
    Tables t;
    const int64_t* fixed; const int64_t* et; const int64_t* cand; int64_t ld_cand;
    int64_t b; int64_t k; int64_t tiles;           // tiles: items of 64 candidates per positive
    float gamma; int log_sigmoid; int group;       // lanes per score: a power of two, 1..16
    float* out; float* raw; int32_t* err;
};

// HOLD: a lane owns at most one unit (units <= group) and keeps the query's share of it in registers for the item
template <int M, int VEC, int SIDE, bool HOLD>
__global__ __launch_bounds__(256) void k_kge_batch_forward(FwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int group = a.group, slots = 64 / group;
    const int slot = lane / group, j = lane % group;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int units = a.t.h / VEC;
    const int64_t items = a.b * a.tiles;

    for (int64_t item = wave; item < items; item += n_waves) {
        const int64_t b = item / a.tiles, k0 = (item % a.tiles) * 64;
        const int64_t qf = a.fixed[b], qr = a.et[b];
        const bool q_ok = (uint64_t)qf < (uint64_t)a.t.n && (uint64_t)qr < (uint64_t)a.t.r;
        const int fixed = q_ok ? (int)qf : 0, rel = q_ok ? (int)qr : 0;      // validated: the tables have fewer than 2^31 rows
        const int cnt = (int)min((int64_t)64, a.k - k0);
        int64_t mc = 0;
        bool ok = q_ok;
        if (lane < cnt) {
            mc = a.cand[b * a.ld_cand + k0 + lane];
            if ((uint64_t)mc >= (uint64_t)a.t.n) { ok = false; mc = 0; }
        }
        const int ic = (int)mc;
        Query<VEC> q;
        if constexpr (HOLD) {
            if (j < units) load_query<M, VEC, SIDE>(a.t, fixed, rel, j * VEC, q);
        }
        float result = 0.f;
        for (int it = 0; it * slots < cnt; ++it) {
            const int idx = it * slots + slot;
            const int cc = __shfl(ic, idx & 63);
            float acc = 0.f;
            if (idx < cnt) {
                if constexpr (HOLD) {
                    if (j < units) acc = add_terms<M, VEC, SIDE>(a.t, q, cc, j * VEC, acc);
                } else {
                    for (int c = j; c < units; c += group) {
                        load_query<M, VEC, SIDE>(a.t, fixed, rel, c * VEC, q);
                        acc = add_terms<M, VEC, SIDE>(a.t, q, cc, c * VEC, acc);
                    }
                }
            }
            for (int off = 1; off < group; off <<= 1) acc += __shfl_xor(acc, off);
            // lane l keeps the score of candidate k0 + l: iteration l / slots, slot l % slots
            const float got = __shfl(acc, (lane % slots) * group);
            if (lane / slots == it) result = got;
        }
        if (lane < cnt) {
            result = finish<M>(result, a.gamma);
            if (!ok) {
                result = __builtin_nanf("");
                if (a.err) atomicOr(a.err, 1);
            }
            const int64_t at = b * a.k + k0 + lane;
            if (a.raw) a.raw[at] = result;
            a.out[at] = a.log_sigmoid ? log_sigmoid(result) : result;
        }
    }
}

template <int M, int VEC, int SIDE>
void launch_forward_hold(const FwdArgs& a, bool hold, int grid, hipStream_t st) {
    if (hold) k_kge_batch_forward<M, VEC, SIDE, true><<<grid, 256, 0, st>>>(a);
    else k_kge_batch_forward<M, VEC, SIDE, false><<<grid, 256, 0, st>>>(a);
}

template <int M>
void launch_forward(const FwdArgs& a, bool vec, int side, bool hold, int grid, hipStream_t st) {
    if (vec) {
        if (side == kTailSide) launch_forward_hold<M, 4, kTailSide>(a, hold, grid, st); else launch_forward_hold<M, 4, kHeadSide>(a, hold, grid, st);
    } else {
        if (side == kTailSide) launch_forward_hold<M, 1, kTailSide>(a, hold, grid, st); else launch_forward_hold<M, 1, kHeadSide>(a, hold, grid, st);
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct BwdCall {
    int model, side; Tables t;
    const int64_t* fixed; const int64_t* et; const int64_t* cand; int64_t ld_cand; int64_t b, k;
    const float* grad_out; const float* raw; float divisor;
    float* d_ent; int64_t ld_dent; float* d_rel; int64_t ld_drel;
    float* q_ent; float* q_rel; int64_t de, dr;    // the positives' partial rows [B, De], [B, Dr]
    bool types_sorted, vec; int lpe; hipStream_t st;
};

// the candidate side's records, keyed by the candidate; grad_out and raw are [B, K] contiguous
__global__ void k_kge_batch_recs(int side, const int64_t* __restrict__ fixed, const int64_t* __restrict__ et,
                                 const int64_t* __restrict__ cand, int64_t ld_cand, const float* __restrict__ grad_out,
                                 const float* __restrict__ raw, int64_t E, int64_t K, int64_t n, int64_t R,
                                 uint32_t* __restrict__ keys, Rec* __restrict__ recs) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = e / K, k = e % K;
        const int64_t ff = fixed[b], rr = et[b], cc = cand[b * ld_cand + k];
        const bool ok = (uint64_t)ff < (uint64_t)n && (uint64_t)cc < (uint64_t)n && (uint64_t)rr < (uint64_t)R;
        Rec rec = {kSkip, 0u, 0u, 0.f};
        uint32_t key = (uint32_t)n;                      // sorted past the last row, never read
        if (ok) {
            float g = grad_out[e];
            if (raw) g = g * sigmoid_neg(raw[e]);
            rec = side == kTailSide ? Rec{(uint32_t)ff, (uint32_t)cc, (uint32_t)rr, g} : Rec{(uint32_t)cc, (uint32_t)ff, (uint32_t)rr, g};
            key = (uint32_t)cc;
        }
        keys[e] = key;
        recs[e] = rec;
    }
}

// one record per positive for the passes that add the partial rows: h = the positive (its partial row), g = 1.
// keys == null: the records stay in list order (the relation pass over a sorted et)
__global__ void k_kge_batch_row_recs(int role, const int64_t* __restrict__ fixed, const int64_t* __restrict__ et, int64_t B,
                                     int64_t n, int64_t R, uint32_t num_keys, uint32_t* __restrict__ keys, Rec* __restrict__ recs) {
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ff = fixed[b], rr = et[b];
        const bool ok = (uint64_t)ff < (uint64_t)n && (uint64_t)rr < (uint64_t)R;
        Rec rec = {kSkip, 0u, 0u, 0.f};
        uint32_t key = num_keys;
        if (ok) {
            rec = {(uint32_t)b, (uint32_t)ff, (uint32_t)rr, 1.0f};
            key = role == kRelation ? rec.r : rec.t;
        }
        if (keys) keys[b] = key;
        recs[b] = rec;
    }
}

// Records of a chunk in the passes that add the partial rows.  Most of their rows hold one record or two (a mini-batch's
// positives rarely share an entity), and a chunk's rows are taken one after the other: 32 rows per workgroup, not 2 048.
constexpr int kRowChunkRecs = 32;

// A positive's partial row as a contribution: rows [B, P * h], part p at column p * h.
template <int PARTS>
struct RowTerm {
    using Rec = ::Rec;
    static constexpr int P = PARTS;
    static constexpr bool kFused = true;
    const float* rows; int64_t ld; int h;
    static __device__ __forceinline__ bool skip(const Rec& r) { return r.h == kSkip; }
    template <int VEC>
    __device__ __forceinline__ void terms(const Rec& r, int unit, float (&d)[P][VEC]) const {
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int v = 0; v < VEC; ++v) d[p][v] = rows[(int64_t)r.h * ld + (int64_t)p * h + unit * VEC + v];
    }
};

struct QueryArgs {
    Tables t;
    const int64_t* fixed; const int64_t* et; const int64_t* cand; int64_t ld_cand; int64_t b; int64_t k;
    const float* grad_out; const float* raw; float divisor;
    float* q_ent; float* q_rel; int64_t de, dr;
};

// A workgroup per positive: S = 256 / LPE slots x LPE lanes of VEC columns.  Thread (slot, j) sums its unit's contributions
// of k = slot, slot + S, ... in that order, one fused multiply-add each (seg_add, as the record reductions add); the slots
// are folded through LDS in slot order.  Rows wider than LPE units take the column blocks one after the other.
template <int M, int VEC, int LPE, int SIDE>
__global__ __launch_bounds__(256) void k_kge_batch_query(QueryArgs a) {
    constexpr int S = 256 / LPE;
    constexpr int PE = Traits<M>::ent_parts, PR = M == kComplEx ? 2 : 1, PT = PE + PR;
    constexpr int FIXED_ROLE = SIDE == kTailSide ? kHead : kTail;
    static_assert(PT * LPE * VEC <= 256, "one fold trip");
    __shared__ float part[PT][S][LPE * VEC];
    const int j = threadIdx.x % LPE, slot = threadIdx.x / LPE;
    const int units = a.t.h / VEC;
    for (int64_t b = blockIdx.x; b < a.b; b += gridDim.x) {
        const int64_t qf = a.fixed[b], qr = a.et[b];
        const bool q_ok = (uint64_t)qf < (uint64_t)a.t.n && (uint64_t)qr < (uint64_t)a.t.r;
        const int fixed = q_ok ? (int)qf : 0, rel = q_ok ? (int)qr : 0;
        for (int u0 = 0; u0 < units; u0 += LPE) {               // workgroup-uniform
            const int unit = u0 + j;
            float acc_e[PE][VEC], acc_r[PR][VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
#pragma unroll
                for (int p = 0; p < PE; ++p) acc_e[p][v] = 0.f;
#pragma unroll
                for (int p = 0; p < PR; ++p) acc_r[p][v] = 0.f;
            }
            if (unit < units && q_ok) {
                float fr[VEC], fi[VEC], rr[VEC], ri[VEC];         // the query side: held for every k
                load_entity<M, VEC>(a.t, fixed, unit * VEC, fr, fi);
                load_relation<M, VEC>(a.t, rel, unit * VEC, rr, ri);
                for (int64_t k = slot; k < a.k; k += S) {
                    const int64_t cc = a.cand[b * a.ld_cand + k];
                    const bool live = (uint64_t)cc < (uint64_t)a.t.n;
                    float g = a.grad_out[b * a.k + k];
                    if (a.raw) g = g * sigmoid_neg(a.raw[b * a.k + k]);
                    float cr[VEC], ci[VEC];
                    load_entity<M, VEC>(a.t, live ? (int)cc : 0, unit * VEC, cr, ci);
                    float de[PE][VEC], dr[PR][VEC];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const Col c = SIDE == kTailSide ? Col{fr[v], fi[v], rr[v], ri[v], cr[v], ci[v]}
                                                        : Col{cr[v], ci[v], rr[v], ri[v], fr[v], fi[v]};
                        float d0, d1;
                        dscore<M, FIXED_ROLE>(c, a.divisor, d0, d1);
                        de[0][v] = d0;
                        if constexpr (PE == 2) de[1][v] = d1;
                        dscore<M, kRelation>(c, a.divisor, d0, d1);
                        dr[0][v] = d0;
                        if constexpr (PR == 2) dr[1][v] = d1;
                    }
                    gn::seg_add<true>(acc_e, g, de, live);
                    gn::seg_add<true>(acc_r, g, dr, live);
                }
            }
            __syncthreads();                                    // the previous fold is done with `part`
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
#pragma unroll
                for (int p = 0; p < PE; ++p) part[p][slot][j * VEC + v] = acc_e[p][v];
#pragma unroll
                for (int p = 0; p < PR; ++p) part[PE + p][slot][j * VEC + v] = acc_r[p][v];
            }
            __syncthreads();
            // thread (part, column) folds the S slots in slot order
            const int p = threadIdx.x / (LPE * VEC), c = threadIdx.x % (LPE * VEC);
            const int column = u0 * VEC + c;
            if (p < PT && column < units * VEC) {
                float s = part[p][0][c];
#pragma unroll
                for (int k = 1; k < S; ++k) s += part[p][k][c];
                if (p < PE) a.q_ent[b * a.de + (int64_t)p * a.t.h + column] = s;
                else a.q_rel[b * a.dr + (int64_t)(p - PE) * a.t.h + column] = s;
            }
        }
    }
}

template <int M, int SIDE>
void launch_query_side(const QueryArgs& a, bool vec, int lpe, int grid, hipStream_t st) {
    if (!vec) k_kge_batch_query<M, 1, 16, SIDE><<<grid, 256, 0, st>>>(a);
    else if (lpe == 8) k_kge_batch_query<M, 4, 8, SIDE><<<grid, 256, 0, st>>>(a);
    else k_kge_batch_query<M, 4, 16, SIDE><<<grid, 256, 0, st>>>(a);
}

template <int M>
void launch_query(const QueryArgs& a, int side, bool vec, int lpe, int grid, hipStream_t st) {
    if (side == kTailSide) launch_query_side<M, kTailSide>(a, vec, lpe, grid, st); else launch_query_side<M, kHeadSide>(a, vec, lpe, grid, st);
}

template <int M>
void launch_candidate_reduce(const BwdCall& c, const gn::SegFrame<Rec>& f, unsigned chunks) {
    if (c.side == kTailSide) launch_seg_reduce(KgeTerm<M, kTail>{c.t, c.divisor}, f, c.vec, c.lpe, chunks, c.st);
    else launch_seg_reduce(KgeTerm<M, kHead>{c.t, c.divisor}, f, c.vec, c.lpe, chunks, c.st);
}

int entity_parts(int model) { return (model == kComplEx || model == kRotatE) ? 2 : 1; }
int relation_parts(int model) { return model == kComplEx ? 2 : 1; }

// d_ent = the candidates' sums
gn_status candidate_pass(const BwdCall& c, const gn::SegWs<Rec>& w) {
    const int64_t e = c.b * c.k;
    k_kge_batch_recs<<<gn::stream_grid(e, 256), 256, 0, c.st>>>(c.side, c.fixed, c.et, c.cand, c.ld_cand, c.grad_out, c.raw, e, c.k,
                                                                 c.t.n, c.t.r, w.keys, w.recs);
    GN_LAUNCH_CHECK();
    const gn::SegOut o = {c.d_ent, c.ld_dent, c.t.h, entity_parts(c.model), 0};
    const int vecw = c.vec ? 4 : 1;
    return gn::seg_pass(w, e, c.t.n, nullptr, o, c.t.h / vecw, vecw, c.lpe,
                        [&](const gn::SegFrame<Rec>& f, int, unsigned chunks) {
                            switch (c.model) {
                                case kTransE: launch_candidate_reduce<kTransE>(c, f, chunks); break;
                                case kDistMult: launch_candidate_reduce<kDistMult>(c, f, chunks); break;
                                case kComplEx: launch_candidate_reduce<kComplEx>(c, f, chunks); break;
                                default: launch_candidate_reduce<kRotatE>(c, f, chunks); break;
                            }
                        },
                        c.st);
}

// the positives' partial rows
gn_status query_sums(const BwdCall& c) {
    QueryArgs a;
    a.t = c.t; a.fixed = c.fixed; a.et = c.et; a.cand = c.cand; a.ld_cand = c.ld_cand; a.b = c.b; a.k = c.k;
    a.grad_out = c.grad_out; a.raw = c.raw; a.divisor = c.divisor;
    a.q_ent = c.q_ent; a.q_rel = c.q_rel; a.de = c.de; a.dr = c.dr;
    const int grid = (int)std::min<int64_t>(c.b, 256 * 64);
    switch (c.model) {
        case kTransE: launch_query<kTransE>(a, c.side, c.vec, c.lpe, grid, c.st); break;
        case kDistMult: launch_query<kDistMult>(a, c.side, c.vec, c.lpe, grid, c.st); break;
        case kComplEx: launch_query<kComplEx>(a, c.side, c.vec, c.lpe, grid, c.st); break;
        default: launch_query<kRotatE>(a, c.side, c.vec, c.lpe, grid, c.st); break;
    }
    GN_LAUNCH_CHECK();
    return GN_OK;
}

// d_ent += the partial rows by fixed[b] (role kTail: the key is the record's t), or d_rel = the partial rows by et[b]
gn_status row_pass(int role, const BwdCall& c, const gn::SegWs<Rec>& w) {
    const bool relation = role == kRelation;
    const int64_t rows = relation ? c.t.r : c.t.n;
    const bool in_place = relation && c.types_sorted;
    k_kge_batch_row_recs<<<gn::stream_grid(c.b, 256), 256, 0, c.st>>>(role, c.fixed, c.et, c.b, c.t.n, c.t.r, (uint32_t)rows,
                                                                       in_place ? nullptr : w.keys, w.recs);
    GN_LAUNCH_CHECK();
    const int parts = relation ? relation_parts(c.model) : entity_parts(c.model);
    const gn::SegOut o = {relation ? c.d_rel : c.d_ent, relation ? c.ld_drel : c.ld_dent, c.t.h, parts, relation ? 0 : 1};
    const float* partial = relation ? c.q_rel : c.q_ent;
    const int64_t ld = relation ? c.dr : c.de;
    const int vecw = c.vec ? 4 : 1;
    return gn::seg_pass(w, c.b, rows, in_place ? c.et : nullptr, o, c.t.h / vecw, vecw, c.lpe,
                        [&](const gn::SegFrame<Rec>& f, int, unsigned chunks) {
                            if (parts == 1) launch_seg_reduce<RowTerm<1>, kRowChunkRecs>({partial, ld, c.t.h}, f, c.vec, c.lpe, chunks, c.st);
                            else launch_seg_reduce<RowTerm<2>, kRowChunkRecs>({partial, ld, c.t.h}, f, c.vec, c.lpe, chunks, c.st);
                        },
                        c.st, kRowChunkRecs);
}

size_t rows_bytes(int64_t b, int64_t d) { return gn::seg_align_up((size_t)b * d * sizeof(float)); }

// The backward's scratch: one reduction's (the B * K candidate records; the B row records reuse it afterwards); in its
// tail RotatE's cos / sin tables, then the positives' partial rows [B, De] and [B, Dr].
gn::SegLayout ws_layout(int model, int64_t n, int64_t r, int64_t h, int64_t b, int64_t k) {
    const size_t tail = trig_bytes(model, r, h) + rows_bytes(b, entity_parts(model) * h) + rows_bytes(b, relation_parts(model) * h);
    // (the partials hold a slot pair per chunk: sized for the B * K records in chunks of kSegChunkRecs and for the B
    // records in chunks of kRowChunkRecs)
    gn::SegLayout l = gn::seg_layout<Rec>(b * std::max<int64_t>(k, gn::kSegChunkRecs / kRowChunkRecs), std::max(n, r), 2, tail);
    // the sort's temporary serves the sorts of B records as well (rocPRIM picks its algorithm, and its scratch, by size)
    const size_t rows_sort = gn::seg_layout<Rec>(b, 0, 0, 0).total - gn::seg_layout<Rec>(b, 0, 0, 0).sort_tmp;
    l.total = std::max(l.total, l.sort_tmp + rows_sort);
    return l;
}

gn_status check_batch(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel, int64_t r, int64_t h,
                      int64_t b, int64_t k, int64_t ld_cand, int side) {
    GN_REQUIRE(side == kTailSide || side == kHeadSide, "unknown side %d (0 tail, 1 head)", side);
    GN_REQUIRE(b >= 0 && k >= 0, "negative size");
    if (b >= (1ll << 31) || k >= (1ll << 31))
        return gn::fail(GN_ERR_UNSUPPORTED, "the candidate block is beyond the 32-bit record encoding");
    GN_OK_OR_RETURN(check_shapes(model, ent, ld_ent, n, rel, ld_rel, r, h, b * k));
    GN_REQUIRE(ld_cand >= k, "leading dimension of the candidates smaller than K");
    return GN_OK;
}

}  // namespace

extern "C" size_t gn_kge_batch_forward_workspace_bytes(int model, int64_t r, int64_t h) {
    if (r < 0 || h < 0) return 0;
    return trig_bytes(model, r, h);
}

extern "C" gn_status gn_kge_batch_forward_f32(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                              int64_t r, int64_t h, const int64_t* fixed, const int64_t* et, const int64_t* cand,
                                              int64_t ld_cand, int64_t b, int64_t k, int side, float gamma, float phase_divisor,
                                              int log_sigmoid_out, float* out, float* raw_out, int32_t* err, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    GN_OK_OR_RETURN(check_batch(model, ent, ld_ent, n, rel, ld_rel, r, h, b, k, ld_cand, side));
    if (b == 0 || k == 0) return GN_OK;
    GN_REQUIRE(fixed && et && cand && out, "operand pointer is null");
    hipStream_t st = gn::as_stream(stream);
    FwdArgs a;
    a.t.ent = ent; a.t.ld_ent = ld_ent; a.t.n = n; a.t.r = r; a.t.h = (int)h;
    if (model == kRotatE) {
        GN_REQUIRE(phase_divisor != 0.f, "RotatE: the phase divisor is zero");
        GN_REQUIRE(workspace && workspace_bytes >= trig_bytes(model, r, h) && gn::aligned16(workspace),
                   "workspace too small: need %zu bytes (16-byte aligned)", trig_bytes(model, r, h));
    }
    GN_OK_OR_RETURN(relation_operand(model, a.t, rel, ld_rel, phase_divisor, static_cast<float*>(workspace), st));
    a.fixed = fixed; a.et = et; a.cand = cand; a.ld_cand = ld_cand; a.b = b; a.k = k; a.tiles = gn::ceil_div(k, 64);
    a.gamma = gamma; a.log_sigmoid = log_sigmoid_out; a.out = out; a.raw = raw_out; a.err = err;
    const bool vec = vector_rows(a.t);
    const int64_t units = vec ? h / 4 : h;
    a.group = forward_group(units);
    const bool hold = units <= a.group;
    const int grid = gn::stream_grid(b * a.tiles * 64, 256);
    switch (model) {
        case kTransE: launch_forward<kTransE>(a, vec, side, hold, grid, st); break;
        case kDistMult: launch_forward<kDistMult>(a, vec, side, hold, grid, st); break;
        case kComplEx: launch_forward<kComplEx>(a, vec, side, hold, grid, st); break;
        default: launch_forward<kRotatE>(a, vec, side, hold, grid, st); break;
    }
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" size_t gn_kge_batch_backward_workspace_bytes(int model, int64_t n, int64_t r, int64_t h, int64_t b, int64_t k) {
    if (n < 0 || r < 0 || h < 0 || b <= 0 || k <= 0 || b >= (1ll << 31) || k >= (1ll << 31)) return 0;
    return ws_layout(model, n, r, h, b, k).total;
}

extern "C" gn_status gn_kge_batch_backward_f32(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                               int64_t r, int64_t h, const int64_t* fixed, const int64_t* et, const int64_t* cand,
                                               int64_t ld_cand, int64_t b, int64_t k, int side, float phase_divisor,
                                               const float* grad_out, const float* raw_scores, float* d_ent, int64_t ld_dent,
                                               float* d_rel, int64_t ld_drel, int flags, void* workspace, size_t workspace_bytes,
                                               void* stream) {
    GN_OK_OR_RETURN(check_batch(model, ent, ld_ent, n, rel, ld_rel, r, h, b, k, ld_cand, side));
    const int64_t de = entity_parts(model) * h, dr = relation_parts(model) * h;
    GN_REQUIRE((n == 0 || h == 0 || d_ent) && (r == 0 || h == 0 || d_rel), "gradient pointer is null");
    GN_REQUIRE(ld_dent >= de && ld_drel >= dr, "leading dimension of a gradient smaller than the row length");
    hipStream_t st = gn::as_stream(stream);
    if (b == 0 || k == 0 || h == 0) {                       // gradients of an empty sum
        if (n > 0 && de > 0) GN_HIP(hipMemset2DAsync(d_ent, ld_dent * sizeof(float), 0, de * sizeof(float), n, st));
        if (r > 0 && dr > 0) GN_HIP(hipMemset2DAsync(d_rel, ld_drel * sizeof(float), 0, dr * sizeof(float), r, st));
        return GN_OK;
    }
    GN_REQUIRE(fixed && et && cand && grad_out, "operand pointer is null");
    const gn::SegLayout l = ws_layout(model, n, r, h, b, k);
    GN_REQUIRE(workspace && workspace_bytes >= l.total, "workspace too small: need %zu bytes", l.total);
    GN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    char* ws = static_cast<char*>(workspace);
    BwdCall c;
    c.model = model; c.side = side;
    c.t.ent = ent; c.t.ld_ent = ld_ent; c.t.n = n; c.t.r = r; c.t.h = (int)h;
    if (model == kRotatE) GN_REQUIRE(phase_divisor != 0.f, "RotatE: the phase divisor is zero");
    GN_OK_OR_RETURN(relation_operand(model, c.t, rel, ld_rel, phase_divisor, reinterpret_cast<float*>(ws + l.tail), st));
    c.fixed = fixed; c.et = et; c.cand = cand; c.ld_cand = ld_cand; c.b = b; c.k = k;
    c.grad_out = grad_out; c.raw = raw_scores;
    c.divisor = model == kRotatE ? phase_divisor : 1.0f;
    c.d_ent = d_ent; c.ld_dent = ld_dent; c.d_rel = d_rel; c.ld_drel = ld_drel;
    c.de = de; c.dr = dr;
    c.q_ent = reinterpret_cast<float*>(ws + l.tail + trig_bytes(model, r, h));
    c.q_rel = reinterpret_cast<float*>(ws + l.tail + trig_bytes(model, r, h) + rows_bytes(b, de));
    c.types_sorted = (flags & GN_DM_TYPES_SORTED) != 0;
    c.vec = vector_rows(c.t);                              // (the gradients are stored a float at a time: any ld)
    c.lpe = reduce_lanes(c.vec, (int)(c.vec ? h / 4 : h));
    c.st = st;
    const gn::SegWs<Rec> w(ws, l);
    GN_OK_OR_RETURN(candidate_pass(c, w));
    GN_OK_OR_RETURN(query_sums(c));
    GN_OK_OR_RETURN(row_pass(kTail, c, w));
    return row_pass(kRelation, c, w);
}
