// Knowledge-graph-embedding scorers of the link-prediction baselines (KGEModel.forward,
// baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:127-235) and their gradients:
//
//   h = Ent[head_e]   t = Ent[tail_e]   r = Rel[type_e]           out[e] = logsigmoid?( s_e )
//   TransE    s = gamma - sum_k |h_k + r_k - t_k|
//   DistMult  s = sum_k h_k r_k t_k
//   ComplEx   s = sum_k (hr rr - hi ri) tr + (hr ri + hi rr) ti        (real part: columns [0, H), imaginary: [H, 2H))
//   RotatE    s = gamma - sum_k sqrt(a_k^2 + b_k^2),  a = hr cos - hi sin - tr,  b = hr sin + hi cos - ti,  theta = r / divisor
//
// Forward: the kernel shape of k_distmult (distmult.hip) - a lane per triple streams the ids, a lane group per triple
// reads 16-byte pieces of the three rows, folds in a fixed order, and the scores leave in one coalesced store per wave.  A
// lane owns a real piece and the matching imaginary piece.  The tables (19.7 k x 64 floats in the driver: 5 MB) stay in L2 /
// Infinity Cache; nothing is planned, the negatives change every step.  RotatE's cos / sin are evaluated once per call for
// the [R, H] relation table (k_kge_trig), not once per triple and column.
//
// Backward: no float atomics.  Per pass (key = head, key = tail, key = relation) 16-byte records (head, tail, relation, g)
// go through the chunked segmented reduction of seg_reduce.cuh, which the DistMult decoder's general backward shares: sorted
// by key, cut into chunks, summed per row in a fixed order.  g = grad_out * sigma(-s) when the forward returned the
// log-sigmoid.  The contribution of a record is g * ds/d(row), a function of the three rows per model and role (KgeTerm).
// This file holds what is the triple list's own: the id loading and inner sum of the forward kernel, the record source and the
// three passes.  The tables, the row loaders, the wave loop and epilogue, dscore, KgeTerm, the record builder and the
// backward's frame are in kge_rows.cuh, shared with kge_batch.hip.
#include "common.h"
#include "kge_rows.cuh"

namespace {

struct FwdArgs {
    Tables t;
    const int64_t* head; const int64_t* tail; const int64_t* et;
    int64_t e; float gamma; int log_sigmoid; int group;     // lanes per triple: a power of two, 1..16
    float* out; float* raw; int32_t* err;
};

template <int M, int VEC>
__global__ __launch_bounds__(256) void k_kge_forward(FwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int group = a.group, j = lane % group;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int units = a.t.h / VEC;

    for (int64_t e0 = wave * 64; e0 < a.e; e0 += n_waves * 64) {
        const int64_t mine = e0 + lane;
        int64_t mh = 0, mt = 0, mr = 0;
        bool ok = true;
        if (mine < a.e) {
            mh = a.head[mine]; mt = a.tail[mine]; mr = a.et[mine];
            ok = in_tables(a.t, mh, mt, mr);
            if (!ok) { mh = mt = mr = 0; }
        }
        const int ih = (int)mh, it_ = (int)mt, ir = (int)mr;       // validated: the tables have fewer than 2^31 rows
        const int cnt = (int)min((int64_t)64, a.e - e0);
        const float sum = wave_scores(lane, group, cnt, [&](int idx) {
            const int hh = __shfl(ih, idx & 63), tt = __shfl(it_, idx & 63), rr = __shfl(ir, idx & 63);
            float acc = 0.f;
            if (idx < cnt) {
                for (int c = j; c < units; c += group) {
                    Col col[VEC];
                    load_cols<M, VEC>(a.t, hh, tt, rr, c * VEC, col);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc += term<M>(col[v]);
                }
            }
            return acc;
        });
        if (mine < a.e) store_score<M>(sum, ok, mine, a.gamma, a.log_sigmoid, a.out, a.raw, a.err);
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct BwdCall : BwdFrame {
    const int64_t* head; const int64_t* tail; const int64_t* et; int64_t e;
};

// the record of triple e
struct ListSrc {
    const int64_t* head; const int64_t* tail; const int64_t* et; const float* grad_out; const float* raw;
    __device__ bool get(int64_t e, const Tables& t, Rec& rec) const {
        const int64_t hh = head[e], tt = tail[e], rr = et[e];
        if (!in_tables(t, hh, tt, rr)) return false;
        rec = {(uint32_t)hh, (uint32_t)tt, (uint32_t)rr, upstream(grad_out, raw, e)};
        return true;
    }
};

// the backward's scratch: the reduction's (up to two output parts), RotatE's cos / sin tables in its tail
gn::SegLayout ws_layout(int model, int64_t n, int64_t r, int64_t h, int64_t e) {
    return gn::seg_layout<Rec>(e, std::max(n, r), 2, trig_bytes(model, r, h));
}

// one pass: the row of `role` receives (d_ent = head pass, then + tail pass)
template <int ROLE>
gn_status pass(const BwdCall& c, const gn::SegWs<Rec>& w) {
    constexpr bool relation = ROLE == kRelation;
    const gn::SegOut o = {relation ? c.d_rel : c.d_ent, relation ? c.ld_drel : c.ld_dent, c.t.h,
                          relation ? relation_parts(c.model) : entity_parts(c.model), ROLE == kTail};
    return record_pass(c, w, ListSrc{c.head, c.tail, c.et, c.grad_out, c.raw}, ROLE, c.e, relation && c.types_sorted ? c.et : nullptr, o,
                       [&](const gn::SegFrame<Rec>& f, int, unsigned chunks) {
                           with_model(c.model, [&](auto m) {
                               launch_seg_reduce(KgeTerm<decltype(m)::value, ROLE>{c.t, c.divisor}, f, c.vec, c.lpe, chunks, c.st);
                           });
                       });
}

}  // namespace

extern "C" size_t gn_kge_forward_workspace_bytes(int model, int64_t r, int64_t h) {
    if (r < 0 || h < 0) return 0;
    return trig_bytes(model, r, h);
}

extern "C" gn_status gn_kge_forward_f32(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                        int64_t r, int64_t h, const int64_t* head, const int64_t* tail, const int64_t* et,
                                        int64_t e, float gamma, float phase_divisor, int log_sigmoid_out, float* out, float* raw_out,
                                        int32_t* err, void* workspace, size_t workspace_bytes, void* stream) {
    GN_OK_OR_RETURN(check_shapes(model, ent, ld_ent, n, rel, ld_rel, r, h, e));
    if (e == 0) return GN_OK;
    GN_REQUIRE(head && tail && et && out, "operand pointer is null");
    hipStream_t st = gn::as_stream(stream);
    FwdArgs a;
    GN_OK_OR_RETURN(make_tables(a.t, model, ent, ld_ent, n, rel, ld_rel, r, h, phase_divisor, workspace, workspace_bytes, st));
    a.head = head; a.tail = tail; a.et = et; a.e = e; a.gamma = gamma; a.log_sigmoid = log_sigmoid_out;
    a.out = out; a.raw = raw_out; a.err = err;
    const bool vec = vector_rows(a.t);
    a.group = forward_group(vec ? h / 4 : h);
    const int grid = gn::stream_grid(gn::ceil_div(e, 64) * 64, 256);
    with_model(model, [&](auto m) {
        with_flag(vec, [&](auto v) { k_kge_forward<decltype(m)::value, decltype(v)::value ? 4 : 1><<<grid, 256, 0, st>>>(a); });
    });
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" size_t gn_kge_backward_workspace_bytes(int model, int64_t n, int64_t r, int64_t h, int64_t e) {
    if (n < 0 || r < 0 || h < 0 || e <= 0) return 0;
    return ws_layout(model, n, r, h, e).total;
}

extern "C" gn_status gn_kge_backward_f32(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                         int64_t r, int64_t h, const int64_t* head, const int64_t* tail, const int64_t* et,
                                         int64_t e, float phase_divisor, const float* grad_out, const float* raw_scores,
                                         float* d_ent, int64_t ld_dent, float* d_rel, int64_t ld_drel, int flags,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    GN_OK_OR_RETURN(check_shapes(model, ent, ld_ent, n, rel, ld_rel, r, h, e));
    const bool empty = e == 0 || h == 0;                    // gradients of an empty sum
    BwdCall c;
    gn::SegLayout l;
    GN_OK_OR_RETURN(backward_frame(c, l, model, ent, ld_ent, n, rel, ld_rel, r, h, empty, head && tail && et, phase_divisor, grad_out,
                                   raw_scores, d_ent, ld_dent, d_rel, ld_drel, flags, workspace, workspace_bytes,
                                   [&] { return ws_layout(model, n, r, h, e); }, gn::as_stream(stream)));
    if (empty) return GN_OK;
    c.head = head; c.tail = tail; c.et = et; c.e = e;
    const gn::SegWs<Rec> w(static_cast<char*>(workspace), l);
    GN_OK_OR_RETURN(pass<kHead>(c, w));
    GN_OK_OR_RETURN(pass<kTail>(c, w));
    return pass<kRelation>(c, w);
}
