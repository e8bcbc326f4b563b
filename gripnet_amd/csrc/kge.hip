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
// The tables, a triple's columns, dscore, the record and KgeTerm are in kge_rows.cuh, shared with kge_batch.hip.
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
    const int group = a.group, slots = 64 / group;
    const int slot = lane / group, j = lane % group;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int units = a.t.h / VEC;

    for (int64_t e0 = wave * 64; e0 < a.e; e0 += n_waves * 64) {
        const int64_t mine = e0 + lane;
        int64_t mh = 0, mt = 0, mr = 0;
        bool ok = true;
        if (mine < a.e) {
            mh = a.head[mine]; mt = a.tail[mine]; mr = a.et[mine];
            ok = (uint64_t)mh < (uint64_t)a.t.n && (uint64_t)mt < (uint64_t)a.t.n && (uint64_t)mr < (uint64_t)a.t.r;
            if (!ok) { mh = mt = mr = 0; }
        }
        const int ih = (int)mh, it_ = (int)mt, ir = (int)mr;       // validated: the tables have fewer than 2^31 rows
        const int cnt = (int)min((int64_t)64, a.e - e0);
        float result = 0.f;
        for (int it = 0; it * slots < cnt; ++it) {
            const int idx = it * slots + slot;
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
            for (int off = 1; off < group; off <<= 1) acc += __shfl_xor(acc, off);
            // lane l keeps the score of triple e0 + l: iteration l / slots, slot l % slots
            const float got = __shfl(acc, (lane % slots) * group);
            if (lane / slots == it) result = got;
        }
        if (mine < a.e) {
            result = finish<M>(result, a.gamma);
            if (!ok) {
                result = __builtin_nanf("");
                if (a.err) atomicOr(a.err, 1);
            }
            if (a.raw) a.raw[mine] = result;
            a.out[mine] = a.log_sigmoid ? log_sigmoid(result) : result;
        }
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// keys == null: the records stay in list order (a relation pass over a sorted edge_type)
__global__ void k_kge_recs(int role, const int64_t* __restrict__ head, const int64_t* __restrict__ tail,
                           const int64_t* __restrict__ et, const float* __restrict__ grad_out,
                           const float* __restrict__ raw, int64_t E, int64_t n, int64_t R, uint32_t num_keys,
                           uint32_t* __restrict__ keys, Rec* __restrict__ recs) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t hh = head[e], tt = tail[e], rr = et[e];
        const bool ok = (uint64_t)hh < (uint64_t)n && (uint64_t)tt < (uint64_t)n && (uint64_t)rr < (uint64_t)R;
        Rec rec = {kSkip, 0u, 0u, 0.f};
        uint32_t key = num_keys;                         // sorted past the last row, never read
        if (ok) {
            float g = grad_out[e];
            if (raw) {                                       // d logsigmoid(s) / d s = sigma(-s), without an overflow of exp
                const float s = raw[e], ex = expf(-fabsf(s));
                g = g * (s > 0.f ? ex / (1.0f + ex) : 1.0f / (1.0f + ex));
            }
            rec = {(uint32_t)hh, (uint32_t)tt, (uint32_t)rr, g};
            key = role == kHead ? rec.h : (role == kTail ? rec.t : rec.r);
        }
        if (keys) keys[e] = key;
        recs[e] = rec;
    }
}

// the backward's scratch: the reduction's (up to two output parts), RotatE's cos / sin tables in its tail
gn::SegLayout ws_layout(int model, int64_t n, int64_t r, int64_t h, int64_t e) {
    return gn::seg_layout<Rec>(e, std::max(n, r), 2, trig_bytes(model, r, h));
}

template <int M>
void launch_forward(const FwdArgs& a, bool vec, int grid, hipStream_t st) {
    if (vec) k_kge_forward<M, 4><<<grid, 256, 0, st>>>(a); else k_kge_forward<M, 1><<<grid, 256, 0, st>>>(a);
}

struct BwdCall {
    int model; Tables t;
    const int64_t* head; const int64_t* tail; const int64_t* et; int64_t e;
    const float* grad_out; const float* raw; float divisor;
    float* d_ent; int64_t ld_dent; float* d_rel; int64_t ld_drel;
    bool types_sorted, vec; hipStream_t st;
};

template <int M, int ROLE>
void launch_reduce(const BwdCall& c, const gn::SegFrame<Rec>& f, int lpe, unsigned chunks) {
    launch_seg_reduce(KgeTerm<M, ROLE>{c.t, c.divisor}, f, c.vec, lpe, chunks, c.st);
}

template <int M>
void launch_reduce_role(int role, const BwdCall& c, const gn::SegFrame<Rec>& f, int lpe, unsigned chunks) {
    if (role == kHead) launch_reduce<M, kHead>(c, f, lpe, chunks);
    else if (role == kTail) launch_reduce<M, kTail>(c, f, lpe, chunks);
    else launch_reduce<M, kRelation>(c, f, lpe, chunks);
}

// one pass: records keyed by `role`, sorted (or left in list order: a relation pass over a sorted edge_type), reduced per row
gn_status pass(int role, const BwdCall& c, const gn::SegWs<Rec>& w) {
    const int64_t rows = role == kRelation ? c.t.r : c.t.n;
    const bool in_place = role == kRelation && c.types_sorted;
    k_kge_recs<<<gn::stream_grid(c.e, 256), 256, 0, c.st>>>(role, c.head, c.tail, c.et, c.grad_out, c.raw, c.e, c.t.n, c.t.r, (uint32_t)rows,
                                                             in_place ? nullptr : w.keys, w.recs);
    GN_LAUNCH_CHECK();
    gn::SegOut o;
    o.out = role == kRelation ? c.d_rel : c.d_ent;
    o.ld_out = role == kRelation ? c.ld_drel : c.ld_dent;
    o.out_h = c.t.h;
    o.parts = role == kRelation ? (c.model == kComplEx ? 2 : 1) : ((c.model == kComplEx || c.model == kRotatE) ? 2 : 1);
    o.accumulate = role == kTail;                           // d_ent = head pass, then + tail pass
    const int vecw = c.vec ? 4 : 1;
    const int units = c.t.h / vecw;
    const int lpe = reduce_lanes(c.vec, units);
    return gn::seg_pass(w, c.e, rows, in_place ? c.et : nullptr, o, units, vecw, lpe,
                        [&](const gn::SegFrame<Rec>& f, int, unsigned chunks) {
                            switch (c.model) {
                                case kTransE: launch_reduce_role<kTransE>(role, c, f, lpe, chunks); break;
                                case kDistMult: launch_reduce_role<kDistMult>(role, c, f, lpe, chunks); break;
                                case kComplEx: launch_reduce_role<kComplEx>(role, c, f, lpe, chunks); break;
                                default: launch_reduce_role<kRotatE>(role, c, f, lpe, chunks); break;
                            }
                        },
                        c.st);
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
    a.t.ent = ent; a.t.ld_ent = ld_ent; a.t.n = n; a.t.r = r; a.t.h = (int)h;
    if (model == kRotatE) {
        GN_REQUIRE(phase_divisor != 0.f, "RotatE: the phase divisor is zero");
        GN_REQUIRE(workspace && workspace_bytes >= trig_bytes(model, r, h) && gn::aligned16(workspace),
                   "workspace too small: need %zu bytes (16-byte aligned)", trig_bytes(model, r, h));
    }
    GN_OK_OR_RETURN(relation_operand(model, a.t, rel, ld_rel, phase_divisor, static_cast<float*>(workspace), st));
    a.head = head; a.tail = tail; a.et = et; a.e = e; a.gamma = gamma; a.log_sigmoid = log_sigmoid_out;
    a.out = out; a.raw = raw_out; a.err = err;
    const bool vec = vector_rows(a.t);
    a.group = forward_group(vec ? h / 4 : h);
    const int grid = gn::stream_grid(gn::ceil_div(e, 64) * 64, 256);
    switch (model) {
        case kTransE: launch_forward<kTransE>(a, vec, grid, st); break;
        case kDistMult: launch_forward<kDistMult>(a, vec, grid, st); break;
        case kComplEx: launch_forward<kComplEx>(a, vec, grid, st); break;
        default: launch_forward<kRotatE>(a, vec, grid, st); break;
    }
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
    const int64_t de = (model == kComplEx || model == kRotatE) ? 2 * h : h, dr = model == kComplEx ? 2 * h : h;
    GN_REQUIRE((n == 0 || h == 0 || d_ent) && (r == 0 || h == 0 || d_rel), "gradient pointer is null");
    GN_REQUIRE(ld_dent >= de && ld_drel >= dr, "leading dimension of a gradient smaller than the row length");
    hipStream_t st = gn::as_stream(stream);
    if (e == 0 || h == 0) {                                 // gradients of an empty sum
        if (n > 0 && de > 0) GN_HIP(hipMemset2DAsync(d_ent, ld_dent * sizeof(float), 0, de * sizeof(float), n, st));
        if (r > 0 && dr > 0) GN_HIP(hipMemset2DAsync(d_rel, ld_drel * sizeof(float), 0, dr * sizeof(float), r, st));
        return GN_OK;
    }
    GN_REQUIRE(head && tail && et && grad_out, "operand pointer is null");
    const gn::SegLayout l = ws_layout(model, n, r, h, e);
    GN_REQUIRE(workspace && workspace_bytes >= l.total, "workspace too small: need %zu bytes", l.total);
    GN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    char* ws = static_cast<char*>(workspace);
    BwdCall c;
    c.model = model;
    c.t.ent = ent; c.t.ld_ent = ld_ent; c.t.n = n; c.t.r = r; c.t.h = (int)h;
    if (model == kRotatE) GN_REQUIRE(phase_divisor != 0.f, "RotatE: the phase divisor is zero");
    GN_OK_OR_RETURN(relation_operand(model, c.t, rel, ld_rel, phase_divisor, reinterpret_cast<float*>(ws + l.tail), st));
    c.head = head; c.tail = tail; c.et = et; c.e = e; c.grad_out = grad_out; c.raw = raw_scores;
    c.divisor = model == kRotatE ? phase_divisor : 1.0f;
    c.d_ent = d_ent; c.ld_dent = ld_dent; c.d_rel = d_rel; c.ld_drel = ld_drel;
    c.types_sorted = (flags & GN_DM_TYPES_SORTED) != 0;
    c.vec = vector_rows(c.t);                              // (the gradients are stored a float at a time: any ld)
    c.st = st;
    const gn::SegWs<Rec> w(ws, l);
    GN_OK_OR_RETURN(pass(kHead, c, w));
    GN_OK_OR_RETURN(pass(kTail, c, w));
    return pass(kRelation, c, w);
}
