// Graph attention (GATConv of PyG 1.4 / 1.5, baselines/NC_baselines/GAT.py of the reference): a softmax over the in-edges of
// every node, one per head, and its gradient.  Four passes over the working list of a GCN-style plan (input loops dropped, one
// loop per node, duplicates kept):
//   k_gat_logits    a_dst, a_src of every node and head from h = x W
//   k_gat_forward   destination-major: max of the leaky logits, sum of exp(l - m) * h[src], one division; bias, head mean, ReLU
//   k_gat_bwd_dst   destination-major: D = g . o, the logit gradients of a node's in-edges summed into da_dst
//   k_gat_bwd_src   source-major: dh = sum alpha g[dst], da_src, and the logits' share of dh
//   k_gat_att_*     d att as a column reduction over the nodes in three fixed-order stages
// alpha is recomputed from (a_dst, a_src, m, 1 / denominator) wherever it is needed: nothing of size [E', H] is kept.  No float
// atomics: every sum has a fixed order (gat_lanes.cuh), two calls on the same inputs give the same bits.
#include "gat_lanes.cuh"

namespace gn {
namespace {

constexpr int kGatWaves = 4;    // waves (nodes) per workgroup
constexpr int kGatU = 4;        // edges a lane group has in flight
constexpr int kAttRows = 32;    // nodes per workgroup of the d att reduction's first stage
constexpr int kAttFold = 64;    // first-stage sums per workgroup of its second stage

// one thread per (node, head): the two dot products of a head's C channels with the halves of att[head]
__global__ __launch_bounds__(256) void k_gat_logits(const float* __restrict__ h, int64_t ld_h, int64_t n, int H, int C,
                                                    const float* __restrict__ att, float* __restrict__ a_dst,
                                                    float* __restrict__ a_src) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= n * H) return;
    const int64_t i = t / H;
    const int hh = (int)(t - i * H);
    const float* row = h + i * ld_h + (int64_t)hh * C;
    const float* a = att + (int64_t)hh * 2 * C;
    float d = 0.0f, s = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float v = row[c];
        d = fmaf(v, a[c], d);
        s = fmaf(v, a[C + c], s);
    }
    a_dst[t] = d;
    a_src[t] = s;
}

struct GatFwd {
    const int32_t* rowptr; const int32_t* col;
    const float* h; int64_t ld_h;
    const float* a_dst; const float* a_src;
    float slope;
    const float* bias;
    int concat, relu;
    float* out; int64_t ld_out;
    float* o_save;      // [n, H * C] or null
    float* m; float* rinv;
    int n;
    GatLay lay;
};

template <bool VEC, int UN>
__global__ __launch_bounds__(kGatWaves* kWave) void k_gat_forward(const GatFwd a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int i = blockIdx.x * kGatWaves + (threadIdx.x >> 6);
    if (i >= a.n) return;                                        // (a whole wave leaves: the folds below see all 64 lanes)
    const GatLay l = a.lay;
    const GatLane<UN> p = gat_lane<UN>(l, lane);
    const int H = l.H, C = l.C, F = H * C;
    const int start = a.rowptr[i], end = a.rowptr[i + 1];
    const int step = l.G * kGatU;
    float ad[UN], m[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) { ad[u] = a.a_dst[(int64_t)i * H + p.hh[u]]; m[u] = -INFINITY; }
    // pass 1: the maximum of the leaky logits over the in-edges (the loop is wave-uniform, a lane's own edge may be none)
    for (int base = start; base < end; base += step) {
        int j[kGatU];
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            const int q = base + p.g + e * l.G;
            j[e] = (p.active && q < end) ? a.col[q] : -1;
        }
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            if (j[e] < 0) continue;
#pragma unroll
            for (int u = 0; u < UN; ++u)
                m[u] = fmaxf(m[u], gat_leaky(ad[u] + a.a_src[(int64_t)j[e] * H + p.hh[u]], a.slope));
        }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) m[u] = gat_group_max(m[u], l, p.r);
    // pass 2: sum of exp(l - m) and of exp(l - m) * h[src]
    float acc[UN][4], s[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) { s[u] = 0.0f; acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0f; }
    for (int base = start; base < end; base += step) {
        int j[kGatU];
        float as[kGatU][UN], row[kGatU][UN][4];
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            const int q = base + p.g + e * l.G;
            j[e] = (p.active && q < end) ? a.col[q] : -1;
        }
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            const int64_t jj = j[e] < 0 ? i : j[e];              // (a slot without an edge reads the node's own row and drops it)
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                as[e][u] = a.a_src[jj * H + p.hh[u]];
                gat_load<VEC>(a.h + jj * a.ld_h + (int64_t)p.hh[u] * C + p.c0[u], p.nc[u], row[e][u]);
            }
        }
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            if (j[e] < 0) continue;
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const float w = gat_exp(gat_leaky(ad[u] + as[e][u], a.slope) - m[u]);
                s[u] += w;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[u][k] = fmaf(w, row[e][u][k], acc[u][k]);
            }
        }
    }
    float o[UN][4];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        s[u] = gat_group_sum(s[u], l, p.r);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[u][k] = gat_group_sum(acc[u][k], l, p.r) / s[u];
    }
    const bool writer = p.g == 0;
    if (writer) {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            if (p.nc[u] == 0) continue;
            if (p.c0[u] == 0) {
                a.m[(int64_t)i * H + p.hh[u]] = m[u];
                a.rinv[(int64_t)i * H + p.hh[u]] = 1.0f / s[u];
            }
            if (a.o_save) gat_store<VEC>(a.o_save + (int64_t)i * F + (int64_t)p.hh[u] * C + p.c0[u], p.nc[u], o[u]);
        }
    }
    if (a.concat) {
        if (writer) {
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                if (p.nc[u] == 0) continue;
                const int c = p.hh[u] * C + p.c0[u];
                float v[4], b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (a.bias) gat_load<VEC>(a.bias + c, p.nc[u], b);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = o[u][k] + b[k];
                    if (a.relu) v[k] = v[k] < 0.0f ? 0.0f : v[k];
                }
                gat_store<VEC>(a.out + (int64_t)i * a.ld_out + c, p.nc[u], v);
            }
        }
    } else {
        // the mean over the heads, head 0 first: the lanes of head 0 collect their channels of every head
        const int lh = p.r % l.LH;
        float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int hh = 0; hh < H; ++hh) {
            const int q = hh * l.LH + lh;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float mine = o[0][k];
                if constexpr (UN == 2) mine = q >= kWave ? o[1][k] : o[0][k];
                tot[k] += __shfl(mine, q & (kWave - 1));
            }
        }
        if (writer && p.r < l.LH && p.nc[0]) {
            float v[4], b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (a.bias) gat_load<VEC>(a.bias + p.c0[0], p.nc[0], b);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = tot[k] / (float)H + b[k];
                if (a.relu) v[k] = v[k] < 0.0f ? 0.0f : v[k];
            }
            gat_store<VEC>(a.out + (int64_t)i * a.ld_out + p.c0[0], p.nc[0], v);
        }
    }
}

struct GatBwd {
    const int32_t* rowptr; const int32_t* col;   // the CSR of the pass: destination-major, or its transpose
    const float* h; int64_t ld_h;
    const float* a_dst; const float* a_src; const float* m; const float* rinv;
    float slope;
    const float* g; int64_t ld_g;                // gradient of the output before bias and ReLU: [n, H * C], or [n, C] (head mean)
    int concat;
    const float* o;                              // [n, H * C] what the forward left (k_gat_bwd_dst)
    float4* pack;                                // [n, H] (a_dst, m, 1 / denominator, D) for the source-major pass
    float* da_dst; float* da_src;                // [n, H]
    const float* att;                            // [H, 2 C]
    float* dh; int64_t ld_dh;
    int n;
    GatLay lay;
};

// the gradient that reaches o[i, head, c0 .. c0 + 3]: the row's own columns, or the head mean's share
template <bool VEC>
__device__ __forceinline__ void gat_load_g(const GatBwd& a, int64_t i, int hh, int c0, int nc, float v[4]) {
    if (a.concat) {
        gat_load<VEC>(a.g + i * a.ld_g + (int64_t)hh * a.lay.C + c0, nc, v);
    } else {
        gat_load<VEC>(a.g + i * a.ld_g + c0, nc, v);
        const float heads = (float)a.lay.H;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] / heads;
    }
}

template <bool VEC, int UN>
__global__ __launch_bounds__(kGatWaves* kWave) void k_gat_bwd_dst(const GatBwd a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int i = blockIdx.x * kGatWaves + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const GatLay l = a.lay;
    const GatLane<UN> p = gat_lane<UN>(l, lane);
    const int H = l.H, C = l.C, F = H * C;
    const int start = a.rowptr[i], end = a.rowptr[i + 1];
    const int step = l.G * kGatU;
    float g[UN][4], ad[UN], m[UN], ri[UN], D[UN], sum[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        float o[4];
        gat_load_g<VEC>(a, i, p.hh[u], p.c0[u], p.nc[u], g[u]);
        gat_load<VEC>(a.o + (int64_t)i * F + (int64_t)p.hh[u] * C + p.c0[u], p.nc[u], o);
        D[u] = gat_head_sum(fmaf(g[u][3], o[3], fmaf(g[u][2], o[2], fmaf(g[u][1], o[1], g[u][0] * o[0]))), l.LH);
        const int64_t at = (int64_t)i * H + p.hh[u];
        ad[u] = a.a_dst[at]; m[u] = a.m[at]; ri[u] = a.rinv[at];
        sum[u] = 0.0f;
    }
    for (int base = start; base < end; base += step) {
        int j[kGatU];
        float as[kGatU][UN], row[kGatU][UN][4];
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            const int q = base + p.g + e * l.G;
            j[e] = (p.active && q < end) ? a.col[q] : -1;
        }
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            const int64_t jj = j[e] < 0 ? i : j[e];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                as[e][u] = a.a_src[jj * H + p.hh[u]];
                gat_load<VEC>(a.h + jj * a.ld_h + (int64_t)p.hh[u] * C + p.c0[u], p.nc[u], row[e][u]);
            }
        }
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const float* r = row[e][u];
                const float dot = gat_head_sum(fmaf(g[u][3], r[3], fmaf(g[u][2], r[2], fmaf(g[u][1], r[1], g[u][0] * r[0]))), l.LH);
                const float z = ad[u] + as[e][u];
                const float alpha = gat_exp(gat_leaky(z, a.slope) - m[u]) * ri[u];
                const float dz = alpha * (dot - D[u]) * (z > 0.0f ? 1.0f : a.slope);
                if (j[e] >= 0) sum[u] += dz;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        sum[u] = gat_group_sum(sum[u], l, p.r);
        if (p.g == 0 && p.nc[u] && p.c0[u] == 0) {
            const int64_t at = (int64_t)i * H + p.hh[u];
            a.da_dst[at] = sum[u];
            a.pack[at] = make_float4(ad[u], m[u], ri[u], D[u]);
        }
    }
}

// wave = source node j; `rowptr` / `col` are the transposed CSR: col holds the destination of every edge that leaves j
template <bool VEC, int UN>
__global__ __launch_bounds__(kGatWaves* kWave) void k_gat_bwd_src(const GatBwd a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int jn = blockIdx.x * kGatWaves + (threadIdx.x >> 6);
    if (jn >= a.n) return;
    const GatLay l = a.lay;
    const GatLane<UN> p = gat_lane<UN>(l, lane);
    const int H = l.H, C = l.C;
    const int start = a.rowptr[jn], end = a.rowptr[jn + 1];
    const int step = l.G * kGatU;
    float hj[UN][4], as[UN], acc[UN][4], sum[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        gat_load<VEC>(a.h + (int64_t)jn * a.ld_h + (int64_t)p.hh[u] * C + p.c0[u], p.nc[u], hj[u]);
        as[u] = a.a_src[(int64_t)jn * H + p.hh[u]];
        sum[u] = 0.0f;
        acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0f;
    }
    for (int base = start; base < end; base += step) {
        int d[kGatU];
        float4 pk[kGatU][UN];
        float g[kGatU][UN][4];
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            const int q = base + p.g + e * l.G;
            d[e] = (p.active && q < end) ? a.col[q] : -1;
        }
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
            const int64_t ii = d[e] < 0 ? jn : d[e];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                pk[e][u] = a.pack[ii * H + p.hh[u]];
                gat_load_g<VEC>(a, ii, p.hh[u], p.c0[u], p.nc[u], g[e][u]);
            }
        }
#pragma unroll
        for (int e = 0; e < kGatU; ++e) {
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const float* gi = g[e][u];
                const float dot = gat_head_sum(fmaf(gi[3], hj[u][3], fmaf(gi[2], hj[u][2], fmaf(gi[1], hj[u][1], gi[0] * hj[u][0]))), l.LH);
                const float z = pk[e][u].x + as[u];
                const float alpha = gat_exp(gat_leaky(z, a.slope) - pk[e][u].y) * pk[e][u].z;
                const float dz = alpha * (dot - pk[e][u].w) * (z > 0.0f ? 1.0f : a.slope);
                if (d[e] >= 0) {
                    sum[u] += dz;
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[u][k] = fmaf(alpha, gi[k], acc[u][k]);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        sum[u] = gat_group_sum(sum[u], l, p.r);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = gat_group_sum(acc[u][k], l, p.r);
        if (p.g != 0 || p.nc[u] == 0) continue;
        const int64_t at = (int64_t)jn * H + p.hh[u];
        if (p.c0[u] == 0) a.da_src[at] = sum[u];
        // the logits' share: a_dst[j] and a_src[j] are dot products of h[j] with the two halves of att
        const float dd = a.da_dst[at];
        const float* ad = a.att + (int64_t)p.hh[u] * 2 * C + p.c0[u];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < p.nc[u]) v[k] = fmaf(sum[u], ad[C + k], fmaf(dd, ad[k], v[k]));
        gat_store<VEC>(a.dh + (int64_t)jn * a.ld_dh + (int64_t)p.hh[u] * C + p.c0[u], p.nc[u], v);
    }
}

// d att, stage 1: thread t < 2 F owns a column of [d att_dst | d att_src] and sums its block's kAttRows nodes in order (the
// row count is a constant and the loop unrolled: eight rows' loads are in flight, the additions keep their order)
__global__ __launch_bounds__(256) void k_gat_att_partial(const float* __restrict__ h, int64_t ld_h, int64_t n, int H, int C,
                                                         const float* __restrict__ da_dst, const float* __restrict__ da_src,
                                                         float* __restrict__ partial) {
    const int F = H * C, t = threadIdx.x;
    if (t >= 2 * F) return;
    const int side = t / F, c = t - side * F, hh = c / C;
    const float* da = side ? da_src : da_dst;
    const int64_t lo = (int64_t)blockIdx.x * kAttRows;
    float s = 0.0f;
#pragma unroll 8
    for (int k = 0; k < kAttRows; ++k) {
        const int64_t i = lo + k < n ? lo + k : n - 1;            // (a row past the end reads the last one and adds nothing)
        const float v = da[i * H + hh] * h[i * ld_h + c];
        s += lo + k < n ? v : 0.0f;
    }
    partial[(int64_t)blockIdx.x * 2 * F + t] = s;
}

// stage 2: the sums of kAttFold consecutive rows of in[rows, width], in row order: out[ceil(rows / kAttFold), width]
__global__ __launch_bounds__(256) void k_gat_att_fold(const float* __restrict__ in, int rows, int width, float* __restrict__ out) {
    const int t = threadIdx.x;
    if (t >= width) return;
    const int lo = blockIdx.x * kAttFold;
    float s = 0.0f;
#pragma unroll 8
    for (int k = 0; k < kAttFold; ++k) {
        const int r = lo + k < rows ? lo + k : rows - 1;
        const float v = in[(int64_t)r * width + t];
        s += lo + k < rows ? v : 0.0f;
    }
    out[(int64_t)blockIdx.x * width + t] = s;
}

// stage 3: what is left, in order, written as att is laid out ([H, 2 C]: a head's target half, then its source half)
__global__ __launch_bounds__(256) void k_gat_att_final(const float* __restrict__ partial, int blocks, int H, int C,
                                                       float* __restrict__ d_att) {
    const int F = H * C, t = threadIdx.x;
    if (t >= 2 * F) return;
    float s = 0.0f;
    for (int b = 0; b < blocks; ++b) s += partial[(int64_t)b * 2 * F + t];
    const int side = t / F, c = t - side * F, hh = c / C;
    d_att[(int64_t)hh * 2 * C + side * C + (c - hh * C)] = s;
}

gn_status check_shape(const gn_graph_plan* plan, int64_t H, int64_t C) {
    GN_REQUIRE(plan != nullptr, "plan is null");
    GN_REQUIRE(plan->is_gcn, "graph attention needs a plan of gn_gcn_plan_create (one loop per node)");
    GN_REQUIRE(H >= 1 && C >= 1, "heads and channels must be positive (H=%lld, C=%lld)", (long long)H, (long long)C);
    GN_REQUIRE(H * C <= kGatMaxRow, "rows of %lld floats: the graph-attention kernels take at most %d", (long long)(H * C), kGatMaxRow);
    return GN_OK;
}

inline bool vec_ok(int64_t C, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
    if (C % 4) return false;
    for (const void* q : ptrs)
        if (q && !aligned16(q)) return false;
    for (int64_t d : lds)
        if (d % 4) return false;
    return true;
}

template <typename A, typename KV, typename KS, typename KS2>
gn_status launch_rows(const A& a, bool vec, KV kv, KS ks, KS2 ks2, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div((int64_t)a.n, kGatWaves)), block(kGatWaves * kWave);
    if (a.lay.units > kWave) hipLaunchKernelGGL(ks2, grid, block, 0, st, a);
    else if (vec) hipLaunchKernelGGL(kv, grid, block, 0, st, a);
    else hipLaunchKernelGGL(ks, grid, block, 0, st, a);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

}  // namespace
}  // namespace gn

extern "C" {

gn_status gn_gat_logits_f32(const float* h, int64_t ld_h, int64_t num_nodes, int64_t heads, int64_t channels, const float* att,
                            float* a_dst, float* a_src, void* stream) {
    GN_REQUIRE(num_nodes >= 0 && heads >= 1 && channels >= 1, "negative or empty size");
    GN_REQUIRE(heads * channels <= gn::kGatMaxRow, "rows of %lld floats: the graph-attention kernels take at most %d",
               (long long)(heads * channels), gn::kGatMaxRow);
    GN_REQUIRE(num_nodes < ((int64_t)1 << 31), "more than 2^31 nodes");
    if (num_nodes == 0) return GN_OK;
    GN_REQUIRE(h && att && a_dst && a_src, "null pointer");
    GN_REQUIRE(ld_h >= heads * channels, "leading dimension smaller than a row");
    gn::k_gat_logits<<<(unsigned)gn::ceil_div(num_nodes * heads, 256), 256, 0, gn::as_stream(stream)>>>(
        h, ld_h, num_nodes, (int)heads, (int)channels, att, a_dst, a_src);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

gn_status gn_gat_forward_f32(const gn_graph_plan* plan, const float* h, int64_t ld_h, int64_t heads, int64_t channels,
                             const float* a_dst, const float* a_src, float negative_slope, const float* bias, int concat,
                             int relu, float* out, int64_t ld_out, float* o_save, float* m, float* rinv, void* stream) {
    GN_OK_OR_RETURN(gn::check_shape(plan, heads, channels));
    if (plan->rows == 0) return GN_OK;
    GN_REQUIRE(h && a_dst && a_src && out && m && rinv, "null pointer");
    const int64_t F = heads * channels;
    GN_REQUIRE(ld_h >= F && ld_out >= (concat ? F : channels), "leading dimension smaller than a row");
    gn::GatFwd a{plan->rowptr.p, plan->col.p, h, ld_h, a_dst, a_src, negative_slope, bias, concat, relu, out, ld_out, o_save,
                 m, rinv, (int)plan->rows, gn::gat_layout((int)heads, (int)channels)};
    const bool vec = gn::vec_ok(channels, {h, bias, out, o_save}, {ld_h, ld_out});
    return gn::launch_rows(a, vec, gn::k_gat_forward<true, 1>, gn::k_gat_forward<false, 1>, gn::k_gat_forward<false, 2>,
                           gn::as_stream(stream));
}

gn_status gn_gat_backward_dst_f32(const gn_graph_plan* plan, const float* h, int64_t ld_h, int64_t heads, int64_t channels,
                                  const float* a_dst, const float* a_src, const float* m, const float* rinv, float negative_slope,
                                  const float* g, int64_t ld_g, int concat, const float* o, float* pack, float* da_dst,
                                  void* stream) {
    GN_OK_OR_RETURN(gn::check_shape(plan, heads, channels));
    if (plan->rows == 0) return GN_OK;
    GN_REQUIRE(h && a_dst && a_src && m && rinv && g && o && pack && da_dst, "null pointer");
    GN_REQUIRE(gn::aligned16(pack), "pack must be 16-byte aligned");
    const int64_t F = heads * channels;
    GN_REQUIRE(ld_h >= F && ld_g >= (concat ? F : channels), "leading dimension smaller than a row");
    gn::GatBwd a{plan->rowptr.p, plan->col.p, h, ld_h, a_dst, a_src, m, rinv, negative_slope, g, ld_g, concat, o,
                 reinterpret_cast<float4*>(pack), da_dst, nullptr, nullptr, nullptr, 0, (int)plan->rows,
                 gn::gat_layout((int)heads, (int)channels)};
    const bool vec = gn::vec_ok(channels, {h, g, o}, {ld_h, ld_g});
    return gn::launch_rows(a, vec, gn::k_gat_bwd_dst<true, 1>, gn::k_gat_bwd_dst<false, 1>, gn::k_gat_bwd_dst<false, 2>,
                           gn::as_stream(stream));
}

gn_status gn_gat_backward_src_f32(const gn_graph_plan* plan, const float* h, int64_t ld_h, int64_t heads, int64_t channels,
                                  const float* a_src, const float* pack, float negative_slope, const float* g, int64_t ld_g,
                                  int concat, const float* da_dst, const float* att, float* dh, int64_t ld_dh, float* da_src,
                                  void* stream) {
    GN_OK_OR_RETURN(gn::check_shape(plan, heads, channels));
    GN_REQUIRE(plan->has_transpose, "the plan has no source-major CSR: call gn_graph_plan_build_transpose first");
    if (plan->rows == 0) return GN_OK;
    GN_REQUIRE(h && a_src && pack && g && da_dst && att && dh && da_src, "null pointer");
    GN_REQUIRE(gn::aligned16(pack), "pack must be 16-byte aligned");
    const int64_t F = heads * channels;
    GN_REQUIRE(ld_h >= F && ld_dh >= F && ld_g >= (concat ? F : channels), "leading dimension smaller than a row");
    gn::GatBwd a{plan->t_rowptr.p, plan->t_col.p, h, ld_h, nullptr, a_src, nullptr, nullptr, negative_slope, g, ld_g, concat,
                 nullptr, reinterpret_cast<float4*>(const_cast<float*>(pack)), const_cast<float*>(da_dst), da_src, att, dh, ld_dh,
                 (int)plan->rows, gn::gat_layout((int)heads, (int)channels)};
    const bool vec = gn::vec_ok(channels, {h, g, dh}, {ld_h, ld_g, ld_dh});
    return gn::launch_rows(a, vec, gn::k_gat_bwd_src<true, 1>, gn::k_gat_bwd_src<false, 1>, gn::k_gat_bwd_src<false, 2>,
                           gn::as_stream(stream));
}

size_t gn_gat_att_grad_workspace_bytes(int64_t num_nodes, int64_t heads, int64_t channels) {
    if (num_nodes <= 0 || heads <= 0 || channels <= 0) return 0;
    const size_t blocks = (size_t)gn::ceil_div(num_nodes, gn::kAttRows);
    return (blocks + (size_t)gn::ceil_div((int64_t)blocks, gn::kAttFold)) * 2 * (size_t)(heads * channels) * sizeof(float);
}

gn_status gn_gat_att_grad_f32(const float* h, int64_t ld_h, int64_t num_nodes, int64_t heads, int64_t channels,
                              const float* da_dst, const float* da_src, float* d_att, void* workspace, size_t workspace_bytes,
                              void* stream) {
    GN_REQUIRE(num_nodes >= 0 && heads >= 1 && channels >= 1, "negative or empty size");
    GN_REQUIRE(heads * channels <= gn::kGatMaxRow, "rows of %lld floats: the graph-attention kernels take at most %d",
               (long long)(heads * channels), gn::kGatMaxRow);
    GN_REQUIRE(d_att != nullptr, "null pointer");
    hipStream_t st = gn::as_stream(stream);
    GN_REQUIRE(num_nodes < ((int64_t)1 << 31), "more than 2^31 nodes");
    const int blocks = (int)gn::ceil_div(num_nodes, gn::kAttRows), folded = (int)gn::ceil_div((int64_t)blocks, gn::kAttFold);
    float* first = static_cast<float*>(workspace);
    float* second = first + (size_t)blocks * 2 * (size_t)(heads * channels);
    if (blocks > 0) {
        GN_REQUIRE(h && da_dst && da_src && workspace, "null pointer");
        GN_REQUIRE(ld_h >= heads * channels, "leading dimension smaller than a row");
        GN_REQUIRE(workspace_bytes >= gn_gat_att_grad_workspace_bytes(num_nodes, heads, channels), "workspace too small");
        gn::k_gat_att_partial<<<blocks, 256, 0, st>>>(h, ld_h, num_nodes, (int)heads, (int)channels, da_dst, da_src, first);
        GN_LAUNCH_CHECK();
        gn::k_gat_att_fold<<<folded, 256, 0, st>>>(first, blocks, (int)(2 * heads * channels), second);
        GN_LAUNCH_CHECK();
    }
    gn::k_gat_att_final<<<1, 256, 0, st>>>(second, folded, (int)heads, (int)channels, d_att);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

}  // extern "C"
