// Lane layout and folds of the graph-attention kernels (gat.hip).
//
// A row of H heads x C channels is held by "units" of four consecutive channels of one head: a head takes LH units (the
// power of two >= ceil(C / 4), so its partial sums fold with DPP inside an aligned lane run), a row H * LH of them.  A wave
// works on ONE node and deals that node's edges to G = 64 / (H * LH) lane groups, one row per group in flight; rows of more
// than 64 units (C = 1 with more than 64 heads) give every lane two units.  Every fold below has a fixed order, and every
// lane of a head (of a row position) ends with the same bits.
#pragma once

#include "common.h"
#include "dpp.cuh"

namespace gn {

constexpr int kGatMaxRow = GN_GAT_MAX_ROW;   // floats of a row the kernels take

struct GatLay {
    int H, C, LH, units, Lr, G, pow2;   // Lr: lanes of a row (min(units, 64)); pow2: Lr is a power of two (G * Lr == 64 then)
};

inline GatLay gat_layout(int H, int C) {
    GatLay l;
    l.H = H; l.C = C;
    int lh = 1;
    while (lh * 4 < C) lh <<= 1;
    l.LH = lh;
    l.units = H * lh;
    l.Lr = l.units < kWave ? l.units : kWave;
    l.G = kWave / l.Lr;
    l.pow2 = (l.Lr & (l.Lr - 1)) == 0;
    return l;
}

// A lane's place: its group, and per unit the head, the first channel and how many of the four exist
template <int UN>
struct GatLane {
    int g, r;            // lane group (edges are dealt to groups g < G), position in the row
    bool active;         // g < G
    int hh[UN], c0[UN], nc[UN];
};

template <int UN>
__device__ __forceinline__ GatLane<UN> gat_lane(const GatLay& l, int lane) {
    GatLane<UN> p;
    p.g = lane / l.Lr;
    p.r = lane - p.g * l.Lr;
    p.active = p.g < l.G;
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        const int q = p.r + u * kWave;
        const bool valid = q < l.units;
        p.hh[u] = valid ? q / l.LH : 0;
        p.c0[u] = 4 * (q % l.LH);
        const int left = l.C - p.c0[u];
        p.nc[u] = !valid || left <= 0 ? 0 : (left < 4 ? left : 4);
    }
    return p;
}

// the up to four floats of a unit; a unit's missing channels read as zero
template <bool VEC>
__device__ __forceinline__ void gat_load(const float* __restrict__ at, int nc, float v[4]) {
    if constexpr (VEC) {
        const float4 t = nc ? *reinterpret_cast<const float4*>(at) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < nc ? at[k] : 0.0f;
    }
}
template <bool VEC>
__device__ __forceinline__ void gat_store(float* __restrict__ at, int nc, const float v[4]) {
    if constexpr (VEC) {
        if (nc) *reinterpret_cast<float4*>(at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nc) at[k] = v[k];
    }
}

// sum over the LH lanes of a head (an aligned run): every lane of the run gets the same bits.  Called by all 64 lanes.
__device__ __forceinline__ float gat_head_sum(float v, int LH) {
    if (LH >= 2) v = dpp_add<0xB1>(v);     // quad_perm [1,0,3,2]
    if (LH >= 4) v = dpp_add<0x4E>(v);     // quad_perm [2,3,0,1]
    if (LH >= 8) v = dpp_add<0x141>(v);    // row_half_mirror
    if (LH >= 16) v = dpp_add<0x140>(v);   // row_mirror
    if (LH >= 32) v += __shfl_xor(v, 16);
    return v;
}

// sum / maximum over the lane groups of a wave, per row position: a tree over lane ^ Lr, lane ^ 2 Lr, ... where Lr is a power
// of two, else the groups in order 0 .. G - 1
__device__ __forceinline__ float gat_group_sum(float v, const GatLay& l, int r) {
    if (l.G == 1) return v;
    if (l.pow2) {
        for (int off = l.Lr; off < kWave; off <<= 1) v += __shfl_xor(v, off);
        return v;
    }
    float t = 0.0f;
    for (int g = 0; g < l.G; ++g) t += __shfl(v, g * l.Lr + r);
    return t;
}
__device__ __forceinline__ float gat_group_max(float v, const GatLay& l, int r) {
    if (l.G == 1) return v;
    if (l.pow2) {
        for (int off = l.Lr; off < kWave; off <<= 1) v = fmaxf(v, __shfl_xor(v, off));
        return v;
    }
    float t = __shfl(v, r);
    for (int g = 1; g < l.G; ++g) t = fmaxf(t, __shfl(v, g * l.Lr + r));
    return t;
}

__device__ __forceinline__ float gat_leaky(float z, float slope) { return z > 0.0f ? z : slope * z; }
// exp(d) for d <= 0 as 2^(d log2 e): relative error |d| u + the instruction's, in a term of weight e^d
__device__ __forceinline__ float gat_exp(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896340736f); }

}  // namespace gn
