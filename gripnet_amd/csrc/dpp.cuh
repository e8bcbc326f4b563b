// DPP helpers shared by the quad-per-row kernels (distmult_quad.cuh, gcn_blocked.hip): a lane reads a neighbour's register
// inside the VALU, no LDS round trip.
#pragma once

namespace gn {

// quad_perm controls write every lane, so no "old" value has to be set up in front of the DPP move
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) { return __builtin_amdgcn_mov_dpp(x, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
    return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}

}  // namespace gn
