// What the KGE scorers' triple-list kernels (kge.hip) and candidate-block kernels (kge_batch.hip) share beyond the column
// arithmetic of kge_term.cuh: the tables as the kernels read them, a triple's columns, the derivative of a column's term per
// role, the backward's record and its contribution to seg_reduce.cuh, the reduce launch rule and the operand checks.  One
// definition each, so that a score or a gradient of one triple is the same bits whichever entry point it came through.
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

// the VEC columns [k, k + VEC) of a triple's three rows
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

__device__ __forceinline__ float log_sigmoid(float s) { return fminf(s, 0.f) - log1pf(expf(-fabsf(s))); }

// d logsigmoid(s) / d s = sigma(-s), without an overflow of exp
__device__ __forceinline__ float sigmoid_neg(float s) {
    const float ex = expf(-fabsf(s));
    return s > 0.f ? ex / (1.0f + ex) : 1.0f / (1.0f + ex);
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct Rec { uint32_t h, t, r; float g; };      // 16 bytes; h = kSkip: a triple with an id outside its table
constexpr uint32_t kSkip = 0xffffffffu;

// What a record contributes to the row of ROLE: ds / d(row), per part and column (seg_reduce.cuh accumulates g times it with
// one fused multiply-add per element, as the backward always has).
template <int M, int ROLE>
struct KgeTerm {
    using Rec = ::Rec;
    static constexpr int P = ROLE == kRelation ? (M == kComplEx ? 2 : 1) : Traits<M>::ent_parts;
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
    const int64_t de = (model == kComplEx || model == kRotatE) ? 2 * h : h, dr = model == kComplEx ? 2 * h : h;
    GN_REQUIRE(ld_ent >= de && ld_rel >= dr, "leading dimension smaller than the row length");
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

}  // namespace
