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
// columns again per candidate (from L1).  The wave loop and the epilogue are wave_scores and store_score of kge_rows.cuh,
// which k_kge_forward (kge.hip) runs as well, around the same term / head_part / tail_term in the same unit order: a score
// is bit for bit what the list kernel gives for that triple.  With fewer than 64 candidates the item's last lanes idle;
// positives are not packed into a wave.
//
// Backward, without float atomics:
//   1. candidate side: B * K records (h, t, r, g) keyed by the candidate, through seg_pass with the list kernels' KgeTerm;
//   2. query side and relation: k_kge_batch_query, a workgroup per positive, sums g[b, k] * ds / d(fixed row) and
//      g[b, k] * ds / d(relation row) over k with the query's columns in registers - a thread (slot, lane) takes
//      k = slot, slot + S, ... in that order, the S slots are folded in slot order - into one partial row per positive and role;
//   3. two seg_pass calls over B records keyed by fixed[b] and et[b] add those rows (RowTerm: the term is the partial row
//      itself, g = 1: the fused multiply-add by 1 is exact); the entity one accumulates onto the candidate pass.
// The records of 1 and 3 come from the one builder of kge_rows.cuh (BlockSrc here, RowSrc there); RowSrc, RowTerm and the
// chunk size of the row passes are in kge_rows.cuh, shared with kge_shared.hip; the checks both backward entry points make,
// and what their passes hold, are backward_frame / BwdFrame there.
#include "common.h"
#include "kge_rows.cuh"

namespace {

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
    const int group = a.group, j = lane % group;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int units = a.t.h / VEC;
    const int64_t items = a.b * a.tiles;

    for (int64_t item = wave; item < items; item += n_waves) {
        const int64_t b = item / a.tiles, k0 = (item % a.tiles) * 64;
        const int64_t qf = a.fixed[b], qr = a.et[b];
        const bool q_ok = in_tables(a.t, qf, qf, qr);
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
        const float sum = wave_scores(lane, group, cnt, [&](int idx) {
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
            return acc;
        });
        if (lane < cnt) store_score<M>(sum, ok, b * a.k + k0 + lane, a.gamma, a.log_sigmoid, a.out, a.raw, a.err);
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct BwdCall : BwdFrame {
    int side;
    const int64_t* fixed; const int64_t* et; const int64_t* cand; int64_t ld_cand; int64_t b, k;
    float* q_ent; float* q_rel; int64_t de, dr;    // the positives' partial rows [B, De], [B, Dr]
};

// the record of candidate e = b * K + k, its h and t by the side; grad_out and raw are [B, K] contiguous
struct BlockSrc {
    int side; const int64_t* fixed; const int64_t* et; const int64_t* cand; int64_t ld_cand, k;
    const float* grad_out; const float* raw;
    __device__ bool get(int64_t e, const Tables& t, Rec& rec) const {
        const int64_t b = e / k;
        const int64_t ff = fixed[b], rr = et[b], cc = cand[b * ld_cand + e % k];
        if (!in_tables(t, ff, cc, rr)) return false;
        const float g = upstream(grad_out, raw, e);
        rec = side == kTailSide ? Rec{(uint32_t)ff, (uint32_t)cc, (uint32_t)rr, g} : Rec{(uint32_t)cc, (uint32_t)ff, (uint32_t)rr, g};
        return true;
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
    constexpr int PE = Traits<M>::ent_parts, PR = Traits<M>::rel_parts, PT = PE + PR;
    constexpr int FIXED_ROLE = SIDE == kTailSide ? kHead : kTail;
    static_assert(PT * LPE * VEC <= 256, "one fold trip");
    __shared__ float part[PT][S][LPE * VEC];
    const int j = threadIdx.x % LPE, slot = threadIdx.x / LPE;
    const int units = a.t.h / VEC;
    for (int64_t b = blockIdx.x; b < a.b; b += gridDim.x) {
        const int64_t qf = a.fixed[b], qr = a.et[b];
        const bool q_ok = in_tables(a.t, qf, qf, qr);
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
                    const float g = upstream(a.grad_out, a.raw, b * a.k + k);
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

// d_ent = the candidates' sums: the candidate is the record's tail (tail side) or head
gn_status candidate_pass(const BwdCall& c, const gn::SegWs<Rec>& w) {
    const gn::SegOut o = {c.d_ent, c.ld_dent, c.t.h, entity_parts(c.model), 0};
    const BlockSrc src = {c.side, c.fixed, c.et, c.cand, c.ld_cand, c.k, c.grad_out, c.raw};
    return record_pass(c, w, src, c.side == kTailSide ? kTail : kHead, c.b * c.k, nullptr, o,
                       [&](const gn::SegFrame<Rec>& f, int, unsigned chunks) {
                           with_model(c.model, [&](auto m) {
                               with_flag(c.side == kTailSide, [&](auto tail) {
                                   constexpr int ROLE = decltype(tail)::value ? kTail : kHead;
                                   launch_seg_reduce(KgeTerm<decltype(m)::value, ROLE>{c.t, c.divisor}, f, c.vec, c.lpe, chunks, c.st);
                               });
                           });
                       });
}

// the positives' partial rows
gn_status query_sums(const BwdCall& c) {
    const QueryArgs a = {c.t, c.fixed, c.et, c.cand, c.ld_cand, c.b, c.k, c.grad_out, c.raw, c.divisor, c.q_ent, c.q_rel, c.de, c.dr};
    const int grid = (int)std::min<int64_t>(c.b, 256 * 64);
    // (VEC, LPE) by the reductions' column-block rule: (1, 16), (4, 8) or (4, 16) - 8 lanes are float4 rows' only
    with_model(c.model, [&](auto m) {
        with_flag(c.side == kHeadSide, [&](auto head) {
            with_flag(c.vec, [&](auto vec) {
                with_flag(c.lpe == 8, [&](auto eight) {
                    constexpr int VEC = decltype(vec)::value ? 4 : 1, LPE = VEC == 4 && decltype(eight)::value ? 8 : 16;
                    k_kge_batch_query<decltype(m)::value, VEC, LPE, decltype(head)::value ? kHeadSide : kTailSide><<<grid, 256, 0, c.st>>>(a);
                });
            });
        });
    });
    GN_LAUNCH_CHECK();
    return GN_OK;
}

// d_ent += the partial rows by fixed[b] (ROLE kTail: the key is the record's t), or d_rel = the partial rows by et[b]
template <int ROLE>
gn_status row_pass(const BwdCall& c, const gn::SegWs<Rec>& w) {
    constexpr bool relation = ROLE == kRelation;
    const int parts = relation ? relation_parts(c.model) : entity_parts(c.model);
    const gn::SegOut o = {relation ? c.d_rel : c.d_ent, relation ? c.ld_drel : c.ld_dent, c.t.h, parts, relation ? 0 : 1};
    const float* partial = relation ? c.q_rel : c.q_ent;
    const int64_t ld = relation ? c.dr : c.de;
    return record_pass(c, w, RowSrc{c.fixed, c.et}, ROLE, c.b, relation && c.types_sorted ? c.et : nullptr, o,
                       [&](const gn::SegFrame<Rec>& f, int, unsigned chunks) {
                           with_flag(parts == 2, [&](auto two) {
                               launch_seg_reduce<RowTerm<decltype(two)::value ? 2 : 1>, kRowChunkRecs>({partial, ld, c.t.h}, f, c.vec, c.lpe, chunks, c.st);
                           });
                       },
                       kRowChunkRecs);
}

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
    GN_OK_OR_RETURN(make_tables(a.t, model, ent, ld_ent, n, rel, ld_rel, r, h, phase_divisor, workspace, workspace_bytes, st));
    a.fixed = fixed; a.et = et; a.cand = cand; a.ld_cand = ld_cand; a.b = b; a.k = k; a.tiles = gn::ceil_div(k, 64);
    a.gamma = gamma; a.log_sigmoid = log_sigmoid_out; a.out = out; a.raw = raw_out; a.err = err;
    const bool vec = vector_rows(a.t);
    const int64_t units = vec ? h / 4 : h;
    a.group = forward_group(units);
    const int grid = gn::stream_grid(b * a.tiles * 64, 256);
    with_model(model, [&](auto m) {
        with_flag(vec, [&](auto v) {
            with_flag(side == kHeadSide, [&](auto head) {
                with_flag(units <= a.group, [&](auto hold) {
                    k_kge_batch_forward<decltype(m)::value, decltype(v)::value ? 4 : 1, decltype(head)::value ? kHeadSide : kTailSide,
                                        decltype(hold)::value><<<grid, 256, 0, st>>>(a);
                });
            });
        });
    });
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
    const bool empty = b == 0 || k == 0 || h == 0;          // gradients of an empty sum
    BwdCall c;
    gn::SegLayout l;
    GN_OK_OR_RETURN(backward_frame(c, l, model, ent, ld_ent, n, rel, ld_rel, r, h, empty, fixed && et && cand, phase_divisor, grad_out,
                                   raw_scores, d_ent, ld_dent, d_rel, ld_drel, flags, workspace, workspace_bytes,
                                   [&] { return ws_layout(model, n, r, h, b, k); }, gn::as_stream(stream)));
    if (empty) return GN_OK;
    c.side = side; c.fixed = fixed; c.et = et; c.cand = cand; c.ld_cand = ld_cand; c.b = b; c.k = k;
    c.de = entity_parts(model) * h; c.dr = relation_parts(model) * h;
    char* rows = static_cast<char*>(workspace) + l.tail + trig_bytes(model, r, h);
    c.q_ent = reinterpret_cast<float*>(rows);
    c.q_rel = reinterpret_cast<float*>(rows + rows_bytes(b, c.de));
    const gn::SegWs<Rec> w(static_cast<char*>(workspace), l);
    GN_OK_OR_RETURN(candidate_pass(c, w));
    GN_OK_OR_RETURN(query_sums(c));
    GN_OK_OR_RETURN(row_pass<kTail>(c, w));
    return row_pass<kRelation>(c, w);
}
