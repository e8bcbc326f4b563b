// What the KGE entry points (kge.hip: triple lists, kge_batch.hip: candidate blocks, kge_rank.hip: ranking) share beyond the
// column arithmetic of kge_term.cuh, one definition each, so that a score or a gradient of one triple is the same bits
// whichever entry point it came through:
//   * Tables and make_tables: the operands as the kernels read them, with the refusals of a RotatE call;
//   * load_entity / load_relation / load_cols: the float4-or-scalar row loaders;
//   * wave_scores and store_score: the forward kernels' wave loop (lane groups, xor fold, transposition) and epilogue;
//   * dscore, Rec, KgeTerm: the derivative of a column's term per role, the backward's record and its contribution to
//     seg_reduce.cuh; k_kge_recs: the one record builder, over a source per entry point;
//   * BwdFrame and backward_frame: what both backward entry points check and hold; launch_seg_reduce: the column-block rule;
//   * RowSrc, RowTerm, kRowChunkRecs: the passes that add partial rows (one per positive, or per shared candidate).
#pragma once

#include "common.h"
#include "kge_term.cuh"
#include "plan_device.cuh"
#include "seg_reduce.cuh"

namespace {

enum { kHead = 0, kTail = 1, kRelation = 2 };

// ds / d(row of ROLE) for one column: (d0, d1) = derivative with respect to the real and the imaginary member (d1 unused
// by the real models).  RotatE's relation derivative is with respect to the phase's source r = theta * divisor: d0 only.
// torch's conventions: sign(0) = 0 (TransE), a zero-length (a, b) contributes nothing (RotatE).
template <int M, int ROLE>
__device__ __forceinline__ void dscore(const Col& c, float divisor, float& d0, float& d1) {
#pragma clang fp contract(off)
    d0 = 0.f; d1 = 0.f;
    if constexpr (M == kTransE) {
        const float d = (c.hr + c.rr) - c.tr;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        d0 = ROLE == kTail ? sg : -sg;
    } else if constexpr (M == kDistMult) {
        d0 = ROLE == kHead ? c.rr * c.tr : (ROLE == kTail ? c.hr * c.rr : c.hr * c.tr);
    } else if constexpr (M == kComplEx) {
        if constexpr (ROLE == kHead) {
            d0 = c.rr * c.tr + c.ri * c.ti;
            d1 = c.rr * c.ti - c.ri * c.tr;
        } else if constexpr (ROLE == kTail) {
            d0 = c.hr * c.rr - c.hi * c.ri;
            d1 = c.hr * c.ri + c.hi * c.rr;
        } else {
            d0 = c.hr * c.tr + c.hi * c.ti;
            d1 = c.hr * c.ti - c.hi * c.tr;
        }
    } else {
        const float a = (c.hr * c.rr - c.hi * c.ri) - c.tr;
        const float b = (c.hr * c.ri + c.hi * c.rr) - c.ti;
        const float m = sqrtf(a * a + b * b);
        if (m > 0.f) {
            const float ua = a / m, ub = b / m;
            if constexpr (ROLE == kHead) {
                d0 = -(ua * c.rr + ub * c.ri);
                d1 = ua * c.ri - ub * c.rr;
            } else if constexpr (ROLE == kTail) {
                d0 = ua;
                d1 = ub;
            } else {
                // d a / d theta = -hr sin - hi cos,  d b / d theta = hr cos - hi sin
                const float dth = ua * (c.hr * c.ri + c.hi * c.rr) - ub * (c.hr * c.rr - c.hi * c.ri);
                d0 = dth / divisor;                          // the backward of `relation / divisor`
            }
        }
    }
}

struct Tables {
    const float* ent; int64_t ld_ent; int64_t n;
    const float* rel; int64_t ld_rel;              // RotatE: the cos table
    const float* rel_im; int64_t r;                // ComplEx: rel + H; RotatE: the sin table
    int h;
};

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

// The same columns of a triple's three rows.  Not two load_entity calls and a load_relation call: that form issues the
// loads row by row, this one the three real pieces before the three imaginary ones, and the record reductions, which at a
// record or two per row wait for exactly these loads, measured 0.4 - 0.8 % slower with it (profiles/r23_kge_once.md).
template <int M, int VEC>
__device__ __forceinline__ void load_cols(const Tables& t, int hh, int tt, int rr, int k, Col (&c)[VEC]) {
    const float* ph = t.ent + (int64_t)hh * t.ld_ent + k;
    const float* pt = t.ent + (int64_t)tt * t.ld_ent + k;
    const float* pr = t.rel + (int64_t)rr * t.ld_rel + k;
    const float* pri = t.rel_im + (int64_t)rr * t.ld_rel + k;
    constexpr bool two = Traits<M>::ent_parts == 2;
    if constexpr (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(ph);
        const float4 b = *reinterpret_cast<const float4*>(pt);
        const float4 w = *reinterpret_cast<const float4*>(pr);
        float4 ai = a, bi = b, wi = w;
        if constexpr (two) {
            ai = *reinterpret_cast<const float4*>(ph + t.h);
            bi = *reinterpret_cast<const float4*>(pt + t.h);
            wi = *reinterpret_cast<const float4*>(pri);
        }
        c[0] = {a.x, ai.x, w.x, wi.x, b.x, bi.x};
        c[1] = {a.y, ai.y, w.y, wi.y, b.y, bi.y};
        c[2] = {a.z, ai.z, w.z, wi.z, b.z, bi.z};
        c[3] = {a.w, ai.w, w.w, wi.w, b.w, bi.w};
    } else {
        c[0] = {ph[0], two ? ph[t.h] : 0.f, pr[0], two ? pri[0] : 0.f, pt[0], two ? pt[t.h] : 0.f};
    }
}

// every id inside its table (a query, which has one entity, passes it twice)
__device__ __forceinline__ bool in_tables(const Tables& t, int64_t head, int64_t tail, int64_t rel) {
    return (uint64_t)head < (uint64_t)t.n && (uint64_t)tail < (uint64_t)t.n && (uint64_t)rel < (uint64_t)t.r;
}

__device__ __forceinline__ float log_sigmoid(float s) { return fminf(s, 0.f) - log1pf(expf(-fabsf(s))); }

// d logsigmoid(s) / d s = sigma(-s), without an overflow of exp
__device__ __forceinline__ float sigmoid_neg(float s) {
    const float ex = expf(-fabsf(s));
    return s > 0.f ? ex / (1.0f + ex) : 1.0f / (1.0f + ex);
}

// ds of score `at`'s upstream: grad_out, times sigma(-s) when the forward returned the log-sigmoid (raw holds s then)
__device__ __forceinline__ float upstream(const float* __restrict__ grad_out, const float* __restrict__ raw, int64_t at) {
    const float g = grad_out[at];
    return raw ? g * sigmoid_neg(raw[at]) : g;
}

// ---- forward: the wave loop ----------------------------------------------------------------------------------------------
// A wave scores cnt <= 64 triples, `group` lanes (a power of two, 1..16) per score, 64 / group scores per trip.  partial(idx)
// is lane j's share of score idx's column sum, j = lane % group: every lane calls it in every trip (it may shuffle the ids a
// lane read) and a slot past cnt returns 0.  The group's shares are folded by xor in a fixed order and lane l keeps the sum
// of score l (trip l / slots, slot l % slots), so the scores leave in one coalesced store.  The list kernel and the block
// kernel run THIS loop: a triple's score is the same bits from either.
template <typename Partial>
__device__ __forceinline__ float wave_scores(int lane, int group, int cnt, Partial&& partial) {
    const int slots = 64 / group, slot = lane / group;
    float result = 0.f;
    for (int it = 0; it * slots < cnt; ++it) {
        float acc = partial(it * slots + slot);
        for (int off = 1; off < group; off <<= 1) acc += __shfl_xor(acc, off);
        const float got = __shfl(acc, (lane % slots) * group);
        if (lane / slots == it) result = got;
    }
    return result;
}

// The epilogue of score `at`: the model's finish; NaN and bit 0 of the error word for an id outside its table; the raw score
// for the backward; the log-sigmoid or the score itself.
template <int M>
__device__ __forceinline__ void store_score(float sum, bool ok, int64_t at, float gamma, int log_sigmoid_out, float* out,
                                            float* raw, int32_t* err) {
    float result = finish<M>(sum, gamma);
    if (!ok) {
        result = __builtin_nanf("");
        if (err) atomicOr(err, 1);
    }
    if (raw) raw[at] = result;
    out[at] = log_sigmoid_out ? log_sigmoid(result) : result;
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct Rec { uint32_t h, t, r; float g; };      // 16 bytes; h = kSkip: a triple with an id outside its table
constexpr uint32_t kSkip = 0xffffffffu;

// What a record contributes to the row of ROLE: ds / d(row), per part and column (seg_reduce.cuh accumulates g times it with
// one fused multiply-add per element, as the backward always has).
template <int M, int ROLE>
struct KgeTerm {
    using Rec = ::Rec;
    static constexpr int P = ROLE == kRelation ? Traits<M>::rel_parts : Traits<M>::ent_parts;
    static constexpr bool kFused = true;
    Tables t; float divisor;
    static __device__ __forceinline__ bool skip(const Rec& r) { return r.h == kSkip; }
    template <int VEC>
    __device__ __forceinline__ void terms(const Rec& r, int unit, float (&d)[P][VEC]) const {
        Col col[VEC];
        load_cols<M, VEC>(t, (int)r.h, (int)r.t, (int)r.r, unit * VEC, col);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float d0, d1;
            dscore<M, ROLE>(col[v], divisor, d0, d1);
            d[0][v] = d0;
            if constexpr (P == 2) d[1][v] = d1;
        }
    }
};

// The records of a pass.  A source yields element e's record - src.get(e, t, rec): false for an id outside its table - and
// the record is keyed by its member for `role`; an invalid element becomes a skip record whose key sorts past the last
// row and is never read.  keys == null: the records stay in list order (a relation pass over sorted relation ids).
template <typename Src>
__global__ void k_kge_recs(Src src, int role, int64_t count, Tables t, uint32_t num_keys, uint32_t* __restrict__ keys,
                           Rec* __restrict__ recs) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        Rec rec;
        uint32_t key = num_keys;
        if (src.get(e, t, rec)) key = role == kHead ? rec.h : (role == kTail ? rec.t : rec.r);
        else rec = {kSkip, 0u, 0u, 0.f};
        if (keys) keys[e] = key;
        recs[e] = rec;
    }
}

size_t trig_bytes(int model, int64_t r, int64_t h) { return model == kRotatE ? gn::seg_align_up((size_t)2 * r * h * sizeof(float)) : 0; }

// The relation operand as the kernels read it: the table itself, or (RotatE) cos / sin of its phases in `trig`.
gn_status relation_operand(int model, Tables& t, const float* rel, int64_t ld_rel, float divisor, float* trig, hipStream_t st) {
    t.rel = rel; t.ld_rel = ld_rel; t.rel_im = rel + t.h;
    if (model != kRotatE) return GN_OK;
    float* cos_t = trig;
    float* sin_t = trig + t.r * t.h;
    k_kge_trig<<<gn::stream_grid(t.r * t.h, 256), 256, 0, st>>>(rel, ld_rel, t.r, t.h, divisor, cos_t, sin_t);
    GN_LAUNCH_CHECK();
    t.rel = cos_t; t.rel_im = sin_t; t.ld_rel = t.h;
    return GN_OK;
}

// The ready tables of a call with work to do, for every entry point: RotatE needs a divisor and trig_bytes of 16-byte aligned
// scratch for its cos / sin tables.
gn_status make_tables(Tables& t, int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel, int64_t r,
                      int64_t h, float divisor, void* trig, size_t trig_size, hipStream_t st) {
    t.ent = ent; t.ld_ent = ld_ent; t.n = n; t.r = r; t.h = (int)h;
    if (model == kRotatE) {
        GN_REQUIRE(divisor != 0.f, "RotatE: the phase divisor is zero");
        GN_REQUIRE(trig && trig_size >= trig_bytes(model, r, h) && gn::aligned16(trig),
                   "workspace too small: need %zu bytes (16-byte aligned)", trig_bytes(model, r, h));
    }
    return relation_operand(model, t, rel, ld_rel, divisor, static_cast<float*>(trig), st);
}

bool vector_rows(const Tables& t) {
    return t.h % 4 == 0 && t.ld_ent % 4 == 0 && t.ld_rel % 4 == 0 && gn::aligned16(t.ent) && gn::aligned16(t.rel) &&
           gn::aligned16(t.rel_im);
}

// lanes per score of the forward kernels: H / 4 lanes on float4 rows, 8 at the driver's H = 32, never more than 16
int forward_group(int64_t units) {
    int group = 1;
    while (group < 16 && group < units) group <<= 1;
    return group;
}

gn_status check_shapes(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel, int64_t r,
                       int64_t h, int64_t e) {
    GN_REQUIRE(model >= kTransE && model <= kRotatE, "unknown model %d (0 TransE, 1 DistMult, 2 ComplEx, 3 RotatE)", model);
    GN_REQUIRE(n >= 0 && r >= 0 && h >= 0 && e >= 0, "negative size");
    if (n >= (1ll << 31) - 512 || r >= (1ll << 31) - 512 || h >= (1ll << 29) || e >= (1ll << 31) - gn::kSegChunkRecs)   // (grids of 256 threads over rows + 1)
        return gn::fail(GN_ERR_UNSUPPORTED, "a table or the triple list is beyond the 32-bit record encoding");
    if (e == 0) return GN_OK;
    GN_REQUIRE(n > 0 && r > 0, "triples given but the entity or relation table is empty");
    GN_REQUIRE(ent && rel, "operand pointer is null");
    GN_REQUIRE(ld_ent >= entity_parts(model) * h && ld_rel >= relation_parts(model) * h, "leading dimension smaller than the row length");
    return GN_OK;
}

// The column-block rule of the record reductions (the bits depend on it): float4 rows take blocks of 8 units on 8 lanes when
// a row has no more than 8 units, of 16 on 16 lanes otherwise; rows that are not float4 rows take 16 lanes of one column.
inline int reduce_lanes(bool vec, int units) { return (vec && units <= 8) ? 8 : 16; }

template <typename C, int CHUNK = gn::kSegChunkRecs>
void launch_seg_reduce(const C& c, const gn::SegFrame<Rec>& f, bool vec, int lpe, unsigned chunks, hipStream_t st) {
    const gn::SegArgs<C> a = {c, f};
    if (!vec) gn::k_seg_reduce<C, 1, 16, CHUNK><<<chunks, 256, 0, st>>>(a);
    else if (lpe == 8) gn::k_seg_reduce<C, 4, 8, CHUNK><<<chunks, 256, 0, st>>>(a);
    else gn::k_seg_reduce<C, 4, 16, CHUNK><<<chunks, 256, 0, st>>>(a);
}

// What a backward entry point holds for its passes, whatever its ids are; an entry point derives from it and adds those.
struct BwdFrame {
    int model; Tables t;
    const float* grad_out; const float* raw; float divisor;     // upstream; the forward's raw scores or null; 1 unless RotatE
    float* d_ent; int64_t ld_dent; float* d_rel; int64_t ld_drel;
    bool types_sorted, vec; int lpe; hipStream_t st;              // vec, lpe: the column-block rule, decided here once
};

// The backward entry points' common part, after check_shapes: the gradients' checks; with `empty` (no score or no column)
// the gradients of an empty sum, and nothing else; otherwise the pointer and workspace checks (layout() is the entry
// point's SegLayout, RotatE's tables at its tail) and the frame.  ids: the entry point's id pointers are all there.
template <typename Layout>
gn_status backward_frame(BwdFrame& c, gn::SegLayout& l, int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel,
                         int64_t ld_rel, int64_t r, int64_t h, bool empty, bool ids, float divisor, const float* grad_out,
                         const float* raw, float* d_ent, int64_t ld_dent, float* d_rel, int64_t ld_drel, int flags, void* workspace,
                         size_t workspace_bytes, Layout&& layout, hipStream_t st) {
    const int64_t de = entity_parts(model) * h, dr = relation_parts(model) * h;
    GN_REQUIRE((n == 0 || h == 0 || d_ent) && (r == 0 || h == 0 || d_rel), "gradient pointer is null");
    GN_REQUIRE(ld_dent >= de && ld_drel >= dr, "leading dimension of a gradient smaller than the row length");
    if (empty) {
        if (n > 0 && de > 0) GN_HIP(hipMemset2DAsync(d_ent, ld_dent * sizeof(float), 0, de * sizeof(float), n, st));
        if (r > 0 && dr > 0) GN_HIP(hipMemset2DAsync(d_rel, ld_drel * sizeof(float), 0, dr * sizeof(float), r, st));
        return GN_OK;
    }
    GN_REQUIRE(ids && grad_out, "operand pointer is null");
    l = layout();
    GN_REQUIRE(workspace && workspace_bytes >= l.total, "workspace too small: need %zu bytes", l.total);
    GN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    c.model = model;
    GN_OK_OR_RETURN(make_tables(c.t, model, ent, ld_ent, n, rel, ld_rel, r, h, divisor, static_cast<char*>(workspace) + l.tail,
                                trig_bytes(model, r, h), st));
    c.grad_out = grad_out; c.raw = raw;
    c.divisor = model == kRotatE ? divisor : 1.0f;
    c.d_ent = d_ent; c.ld_dent = ld_dent; c.d_rel = d_rel; c.ld_drel = ld_drel;
    c.types_sorted = (flags & GN_DM_TYPES_SORTED) != 0;
    c.vec = vector_rows(c.t);                                     // (the gradients are stored a float at a time: any ld)
    c.lpe = reduce_lanes(c.vec, c.t.h / (c.vec ? 4 : 1));
    c.st = st;
    return GN_OK;
}

// One pass of a backward: `count` records from `src` keyed by `role` - sorted, or left in list order when `sorted_types` are
// the relation pass's own sorted ids - and reduced per row into `o` by the contribution that `launch` starts.
template <typename Src, typename Launch>
gn_status record_pass(const BwdFrame& c, const gn::SegWs<Rec>& w, const Src& src, int role, int64_t count,
                      const int64_t* sorted_types, const gn::SegOut& o, Launch&& launch, int chunk = gn::kSegChunkRecs) {
    const int64_t rows = role == kRelation ? c.t.r : c.t.n;
    k_kge_recs<<<gn::stream_grid(count, 256), 256, 0, c.st>>>(src, role, count, c.t, (uint32_t)rows, sorted_types ? nullptr : w.keys, w.recs);
    GN_LAUNCH_CHECK();
    const int vecw = c.vec ? 4 : 1;
    return gn::seg_pass(w, count, rows, sorted_types, o, c.t.h / vecw, vecw, c.lpe, launch, c.st, chunk);
}

// ---- partial rows: the passes that add one row per record (kge_batch.hip: a positive's row; kge_shared.hip: also a shared
// candidate's) ------------------------------------------------------------------------------------------------------------
// one record per positive for the passes that add the partial rows: h = the positive (its partial row), t = its entity, g = 1
struct RowSrc {
    const int64_t* fixed; const int64_t* et;
    __device__ bool get(int64_t b, const Tables& t, Rec& rec) const {
        const int64_t ff = fixed[b], rr = et[b];
        if (!in_tables(t, ff, ff, rr)) return false;
        rec = {(uint32_t)b, (uint32_t)ff, (uint32_t)rr, 1.0f};
        return true;
    }
};

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

inline size_t rows_bytes(int64_t b, int64_t d) { return gn::seg_align_up((size_t)b * d * sizeof(float)); }

}  // namespace
