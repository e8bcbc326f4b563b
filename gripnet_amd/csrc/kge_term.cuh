// What every knowledge-graph-embedding kernel (kge.hip, kge_batch.hip, kge_rank.hip) starts from: the model and side ids, how
// many parts a row has, the one place where a run-time model id or flag becomes a template argument, and the per-column
// arithmetic - one definition of what a column contributes, so that every kernel rounds a term alike.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

enum { kTransE = GN_KGE_TRANSE, kDistMult = GN_KGE_DISTMULT, kComplEx = GN_KGE_COMPLEX, kRotatE = GN_KGE_ROTATE };
enum { kTailSide = GN_KGE_SIDE_TAIL, kHeadSide = GN_KGE_SIDE_HEAD };      // which end of the triple the candidates fill

// parts (real, imaginary) of an entity row and of a row of the relation table (RotatE's table holds phases: one part; the
// operand the kernels read has two, cos and sin)
template <int M> struct Traits;
template <> struct Traits<kTransE>   { static constexpr int ent_parts = 1, rel_parts = 1; };
template <> struct Traits<kDistMult> { static constexpr int ent_parts = 1, rel_parts = 1; };
template <> struct Traits<kComplEx>  { static constexpr int ent_parts = 2, rel_parts = 2; };
template <> struct Traits<kRotatE>   { static constexpr int ent_parts = 2, rel_parts = 1; };

// The dispatch: f(std::integral_constant<int, model>{}) for a validated model id, f(std::true_type / std::false_type{}) for a
// flag.  A launch site is these two around a generic lambda that names its kernel once.
template <typename F>
auto with_model(int model, F&& f) {
    switch (model) {
        case kTransE: return f(std::integral_constant<int, kTransE>{});
        case kDistMult: return f(std::integral_constant<int, kDistMult>{});
        case kComplEx: return f(std::integral_constant<int, kComplEx>{});
        default: return f(std::integral_constant<int, kRotatE>{});
    }
}

template <typename F>
auto with_flag(bool flag, F&& f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}

int entity_parts(int model) { return with_model(model, [](auto m) { return Traits<decltype(m)::value>::ent_parts; }); }
int relation_parts(int model) { return with_model(model, [](auto m) { return Traits<decltype(m)::value>::rel_parts; }); }

// One column of a triple: (hr, hi), (rr, ri), (tr, ti); the imaginary members are unused by the real models.  For RotatE
// (rr, ri) = (cos theta, sin theta).
struct Col { float hr, hi, rr, ri, tr, ti; };

// The column's term in two steps.  head_part: what the tail does not enter (TransE h + r, DistMult h r, ComplEx and RotatE
// the complex product of h and the relation operand); tail_term: the term from that and the tail's column.  A scan over
// tails evaluates head_part once per query and column and tail_term per candidate: the operations and their order are
// those of term<M>, so the bits are.  No contraction into fused multiply-adds here or in dscore: every product is rounded
// as the reference's element-wise kernels round it, so a term that cancels inside (ComplEx's four products, a short
// (a, b) of RotatE) carries the reference's own error, not another one.
template <int M>
__device__ __forceinline__ void head_part(const Col& c, float& p0, float& p1) {
#pragma clang fp contract(off)
    p1 = 0.f;
    if constexpr (M == kTransE) {
        p0 = c.hr + c.rr;
    } else if constexpr (M == kDistMult) {
        p0 = c.hr * c.rr;
    } else {
        p0 = c.hr * c.rr - c.hi * c.ri;
        p1 = c.hr * c.ri + c.hi * c.rr;
    }
}

template <int M>
__device__ __forceinline__ float tail_term(float p0, float p1, float tr, float ti) {
#pragma clang fp contract(off)
    if constexpr (M == kTransE) {
        return fabsf(p0 - tr);
    } else if constexpr (M == kDistMult) {
        return p0 * tr;
    } else if constexpr (M == kComplEx) {
        return p0 * tr + p1 * ti;
    } else {
        const float a = p0 - tr;
        const float b = p1 - ti;
        return sqrtf(a * a + b * b);
    }
}

// the column's term of the sum (TransE and RotatE: of the distance that gamma is reduced by)
template <int M>
__device__ __forceinline__ float term(const Col& c) {
    float p0, p1;
    head_part<M>(c, p0, p1);
    return tail_term<M>(p0, p1, c.tr, c.ti);
}

template <int M>
__device__ __forceinline__ float finish(float sum, float gamma) {
    return (M == kTransE || M == kRotatE) ? gamma - sum : sum;
}

// cos / sin of the relation table's phases, once per call: [R, H] each, rows H apart
__global__ void k_kge_trig(const float* __restrict__ rel, int64_t ld_rel, int64_t r, int h, float divisor,
                           float* __restrict__ cos_out, float* __restrict__ sin_out) {
    const int64_t total = r * h;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float theta = rel[(i / h) * ld_rel + (i % h)] / divisor;
        cos_out[i] = cosf(theta);
        sin_out[i] = sinf(theta);
    }
}

}  // namespace
