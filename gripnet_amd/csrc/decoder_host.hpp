// Host pieces the decoder's forward files (distmult.hip, distmult_fast.hip, distmult_plan.hip) share: what the raw and the
// packed entry point require of a call, the route's DecoderCall of an entry point's arguments, and the one launch function
// that another file calls.
#pragma once

#include "distmult_quad.cuh"

namespace gn_dm {

// The checks of gn_distmult_forward_f32 and gn_distmult_packed_forward_f32, in their order.  *empty: no edges - nothing to
// launch, and nothing further is asked of the call.  ids_31_bits: the raw kernels narrow validated ids and f to int.
inline gn_status require_edge_call(int64_t n, int64_t f, int64_t r, int64_t e, int64_t ld_z, int64_t ld_d, bool ids_31_bits,
                                   bool operands, bool* empty) {
    *empty = e == 0;
    GN_REQUIRE(n >= 0 && f >= 0 && r >= 0 && e >= 0, "negative size");
    GN_REQUIRE(!ids_31_bits || (f < (1ll << 31) && n < (1ll << 31) && r < (1ll << 31)), "table too large");
    if (e == 0) return GN_OK;
    GN_REQUIRE(n > 0 && r > 0, "edges given but the node or relation table is empty");
    GN_REQUIRE(operands, "operand pointer is null");
    GN_REQUIRE(ld_z >= f && ld_d >= f, "leading dimension smaller than the row length");
    return GN_OK;
}

// A call over all f columns (the planned entry narrows them and adds its plan's facts).  GN_DISABLE_FAST is read here, once.
inline gn::route::DecoderCall decoder_call(gn::route::DecoderKind kind, int64_t n, int64_t f, int64_t r, int64_t e, const float* z,
                                           int64_t ld_z, const float* d, int64_t ld_d) {
    gn::route::DecoderCall c{};
    c.kind = kind; c.n = n; c.f = f; c.r = r; c.e = e; c.ld_z = ld_z; c.ld_d = ld_d;
    c.z_at = (unsigned)(reinterpret_cast<uintptr_t>(z) & 15); c.d_at = (unsigned)(reinterpret_cast<uintptr_t>(d) & 15);
    c.col_lo = 0; c.col_hi = f; c.num_features = f;
    c.fast_disabled = gn::fast_paths_disabled();
    c.threads = kThreads;
    return c;
}

// distmult_fast.hip: k_distmult_lds<false> as the route lays it out
gn_status launch_lds_raw(const gn::route::DecoderRoute& rt, const float* z, int64_t ld_z, int64_t n, int64_t f, const int64_t* u,
                         const int64_t* v, const int64_t* et, const float* d, int64_t ld_d, int64_t r, int64_t e, int sigmoid,
                         float* out, int32_t* err, hipStream_t st);

}  // namespace gn_dm
