// The negative-sampling loss of the KGE baselines' mini-batches (baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:
// 266-286 with the subsampling weights of the code base that KGEModel comes from) on RAW scores pos [B] and neg [B, K]:
//
//   ls(x) = min(x, 0) - log1p(exp(-|x|))
//   P_b = ls(pos_b)
//   N_b = (1 / K) sum_k ls(-s_bk)                                           (plain)
//   N_b = sum_k p_bk ls(-s_bk),   p_b = softmax_k(T s_bk), a constant       (self-adversarial, temperature T)
//   W = sum_b w_b,   loss = -(sum_b w_b P_b) / (2 W) - (sum_b w_b N_b) / (2 W)
//
// as ONE launch forward and ONE launch backward; written with torch ops (kge.self_adversarial_loss) it is about twenty
// element-wise / reduction launches over the [B, K] block.  Deterministic the way k_link_loss is (loss.hip): a wave's rows
// are fixed by the grid, a row's sum is a fixed tree over its lanes, a workgroup's partial sums are added in workgroup order
// by the last workgroup to arrive, in double, handed over without fences.
//
// Rows.  K <= 32: a row is a group of L lanes, L the power of two >= K, 64 / L rows per wave and turn (K = 8: eight rows per
// wave, no lane idles), one 4-byte load per lane, a wave's loads contiguous.  K > 32: a wave per row; lane l of turn j holds
// the four scores (j * 64 + l) * 4 .. + 3, loaded as one 16-byte word where base and leading dimension allow (template VEC),
// as four 4-byte words otherwise - the same registers, the same sums, the same bits.  A row is kept in registers up to
// kNsPart = 1,024 scores (kNsTurns = 4 turns): every score is read once.  A longer row goes part by part with a running
// maximum, the sums of the parts rescaled by exp(m_part - m) in double (one rescale per 1,024 scores).
//
// The exponent.  p_bk = exp(T s_bk - m_b) / Z_b with m_b = max_k fl(T s_bk).  A negative far below its row's maximum keeps a
// weight down to an argument of -87; the hardware's exp2 on x * log2(e) loses |x| units there.  The argument is ONE rounding,
// fmaf(T, s, -m), and the exponential is the library's expf (1 unit); the backward recomputes both from the saved m_b: the
// same bits as the forward's.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNsGroups = 512, kNsThreads = 256, kNsWaves = kNsThreads / 64;
constexpr int kNsTurns = 4, kNsPart = kNsTurns * 256;          // a row part in registers: 4 x 64 lanes x 4 scores
constexpr int kNsSmallK = 32;                                   // rows of up to 32 scores share a wave

__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }   // a NaN stays

// ls(-s) = min(-s, 0) - log1p(exp(-|s|)), the subtraction in double (the caller sums in double)
__device__ __forceinline__ double log_sigmoid_neg(float s) {
    return (double)fminf(-s, 0.f) - (double)log1pf(expf(-fabsf(s)));
}

// sigma(s) without overflow: 1 / (1 + t) or t / (1 + t), t = exp(-|s|)
__device__ __forceinline__ float sigmoid(float s) {
    const float t = expf(-fabsf(s));
    return (s >= 0.f ? 1.0f : t) / (1.0f + t);
}

// the scores (j * 64 + lane) * 4 .. + 3 of a row part of `len` scores; `first`: index of the lane's first score
template <bool VEC>
__device__ __forceinline__ f32x4 load_quad(const float* __restrict__ part, int first, int len) {
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if (first + 3 < len) {
        if constexpr (VEC) return *reinterpret_cast<const f32x4*>(part + first);
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = part[first + c];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (first + c < len) q[c] = part[first + c];
    }
    return q;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

struct NsArgs {
    const float* pos;
    const float* neg;
    int64_t ld_neg, B;
    int K;
    const float* weight;        // nullable: 1
    int adversarial;
    float temperature;
};

// What every forward kernel ends with: the wave's three sums -> the workgroup's -> the grid's, by the last arriver.
// (acc: sum w P, sum w N, sum w; each lane's own rows, in the order the grid gave them)
__device__ __forceinline__ void ns_finish(double accP, double accN, double accW, double* __restrict__ partial,
                                          unsigned int* __restrict__ counter, float* __restrict__ loss, float* __restrict__ scale) {
    __shared__ double red[3][kNsWaves];
    __shared__ bool last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    accP = wave_sum(accP); accN = wave_sum(accN); accW = wave_sum(accW);
    if (lane == 0) { red[0][wave] = accP; red[1][wave] = accN; red[2][wave] = accW; }
    __syncthreads();
    if (tid == 0) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int w = 0; w < kNsWaves; ++w) { s[0] += red[0][w]; s[1] += red[1][w]; s[2] += red[2][w]; }
        // the hand-over of k_link_loss (loss.hip): write-through stores of the partial sums, drained, then the ticket; the
        // last arriver reads them with agent-scope loads.  No fence: a release would write back the XCD's L2 per workgroup.
        unsigned long long* out = reinterpret_cast<unsigned long long*>(partial) + 3 * blockIdx.x;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            __hip_atomic_store(out + i, (unsigned long long)__double_as_longlong(s[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int arrived = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = arrived == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    // thread t takes the workgroups t, t + 256, ... in that order, then a fixed tree over the threads
    double s[3] = {0.0, 0.0, 0.0};
    const unsigned long long* __restrict__ ps = reinterpret_cast<const unsigned long long*>(partial);
    for (unsigned g = tid; g < gridDim.x; g += kNsThreads) {
        unsigned long long v[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = __hip_atomic_load(ps + 3 * g + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] += __longlong_as_double((long long)v[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) s[i] = wave_sum(s[i]);
    __syncthreads();                                               // (red was read above by thread 0 only, before the barrier)
    if (lane == 0) { red[0][wave] = s[0]; red[1][wave] = s[1]; red[2][wave] = s[2]; }
    __syncthreads();
    if (tid == 0) {
        double p = 0.0, n = 0.0, w = 0.0;
        for (int i = 0; i < kNsWaves; ++i) { p += red[0][i]; n += red[1][i]; w += red[2][i]; }
        const double half = 1.0 / (2.0 * w);
        *loss = (float)(-(p * half) - n * half);
        *scale = (float)half;
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch (stream-ordered)
    }
}

// ---- forward --------------------------------------------------------------------------------------------------------------
// K <= 32: `shift` = log2 of the lane group L; row = (wave's turn) * (64 / L) + lane / L, score = lane % L.
__global__ __launch_bounds__(kNsThreads) void k_ns_loss_small(NsArgs a, int shift, float* __restrict__ row_stats, double* __restrict__ partial,
                                                              unsigned int* __restrict__ counter, float* __restrict__ loss,
                                                              float* __restrict__ scale) {
    const int lane = threadIdx.x & 63, L = 1 << shift, col = lane & (L - 1), rows = 64 >> shift;
    const int64_t waves = (int64_t)gridDim.x * kNsWaves, turns = (a.B + rows - 1) / rows;
    double accP = 0.0, accN = 0.0, accW = 0.0;
    for (int64_t turn = (int64_t)blockIdx.x * kNsWaves + (threadIdx.x >> 6); turn < turns; turn += waves) {
        const int64_t b = turn * rows + (lane >> shift);
        const bool row = b < a.B, own = row && col < a.K;
        const float s = own ? a.neg[b * a.ld_neg + col] : 0.f;
        float m = 0.f, e = 1.0f;
        if (a.adversarial) {
            m = own ? a.temperature * s : -INFINITY;
            for (int off = L >> 1; off > 0; off >>= 1) m = max_nan(m, __shfl_xor(m, off));
            e = own ? expf(fmaf(a.temperature, s, -m)) : 0.f;
        }
        double z = own ? (double)e : 0.0, num = own ? (double)e * log_sigmoid_neg(s) : 0.0;
        for (int off = L >> 1; off > 0; off >>= 1) { z += __shfl_xor(z, off); num += __shfl_xor(num, off); }
        if (row && col == 0) {
            const double w = a.weight ? (double)a.weight[b] : 1.0;
            const double nb = num / z;                          // (plain: z = K)
            if (row_stats) {                                    // (plain: a NaN score marks its row for the backward)
                row_stats[2 * b] = a.adversarial ? m : (float)nb * 0.f;
                row_stats[2 * b + 1] = (float)(1.0 / z) + (float)nb * 0.f;
            }
            accP += w * log_sigmoid_neg(-a.pos[b]);
            accN += w * nb;
            accW += w;
        }
    }
    ns_finish(accP, accN, accW, partial, counter, loss, scale);
}

// K > 32: a wave per row.
template <bool VEC>
__global__ __launch_bounds__(kNsThreads) void k_ns_loss_rows(NsArgs a, float* __restrict__ row_stats, double* __restrict__ partial,
                                                             unsigned int* __restrict__ counter, float* __restrict__ loss,
                                                             float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * kNsWaves;
    double accP = 0.0, accN = 0.0, accW = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * kNsWaves + (threadIdx.x >> 6); b < a.B; b += waves) {
        const float* __restrict__ row = a.neg + b * a.ld_neg;
        float m = -INFINITY;                                    // the running maximum of T s
        double z = 0.0, num = 0.0;                              // sum e, sum e ls(-s) relative to m (plain: K so far, sum ls(-s))
        for (int p0 = 0; p0 < a.K; p0 += kNsPart) {
            const int len = min(a.K - p0, kNsPart);
            f32x4 q[kNsTurns];
#pragma unroll
            for (int j = 0; j < kNsTurns; ++j) q[j] = load_quad<VEC>(row + p0, (j * 64 + lane) * 4, len);
            float mp = -INFINITY;
            if (a.adversarial) {
#pragma unroll
                for (int j = 0; j < kNsTurns; ++j)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if ((j * 64 + lane) * 4 + c < len) mp = max_nan(mp, a.temperature * q[j][c]);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) mp = max_nan(mp, __shfl_xor(mp, off));
            }
            double zp = 0.0, np = 0.0;
#pragma unroll
            for (int j = 0; j < kNsTurns; ++j) {
                if (j * 256 >= len) break;                      // (uniform)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if ((j * 64 + lane) * 4 + c >= len) continue;
                    const float s = q[j][c];
                    const double e = a.adversarial ? (double)expf(fmaf(a.temperature, s, -mp)) : 1.0;
                    zp += e;
                    np += e * log_sigmoid_neg(s);
                }
            }
            zp = wave_sum(zp);
            np = wave_sum(np);
            if (a.K <= kNsPart || !a.adversarial) {             // (one part, or nothing to rescale)
                m = mp; z += zp; num += np;
            } else {
                const float mn = max_nan(m, mp);
                const double keep = exp((double)m - (double)mn), add = exp((double)mp - (double)mn);
                z = z * keep + zp * add;
                num = num * keep + np * add;
                m = mn;
            }
        }
        if (lane == 0) {
            const double w = a.weight ? (double)a.weight[b] : 1.0;
            const double nb = num / z;
            if (row_stats) {
                row_stats[2 * b] = a.adversarial ? m : (float)nb * 0.f;
                row_stats[2 * b + 1] = (float)(1.0 / z) + (float)nb * 0.f;
            }
            accP += w * log_sigmoid_neg(-a.pos[b]);
            accN += w * nb;
            accW += w;
        }
    }
    ns_finish(accP, accN, accW, partial, counter, loss, scale);
}

// ---- backward -------------------------------------------------------------------------------------------------------------
// d_pos[b] = -g w_b sigma(-pos_b) / (2 W),  d_neg[b, k] = g w_b p_bk sigma(s_bk) / (2 W).  Per row one constant
// c_b = w_b / (2 W Z_b) (plain: w_b / (2 W K)) taken in double and rounded once; an element is g * (c_b * (e * sigma)): the
// upstream gradient multiplies last, so that g = 1 changes no bit and any g costs one rounding.
struct NsGradArgs {
    const float* row_stats;     // nullable unless adversarial
    const float* scale;         // 1 / (2 W)
    const float* upstream;      // nullable: 1
    float* d_pos;
    float* d_neg;
    int64_t ld_dneg;
};

__device__ __forceinline__ float row_constant(const NsArgs& a, const NsGradArgs& g, int64_t b, double half_w, float& m) {
    m = 0.f;
    if (a.adversarial) {
        m = g.row_stats[2 * b];
        return (float)(half_w * (double)g.row_stats[2 * b + 1]);
    }
    const float mark = g.row_stats ? g.row_stats[2 * b + 1] * 0.f : 0.f;   // NaN: the row held a NaN score
    return (float)(half_w / (double)a.K) + mark;
}

__device__ __forceinline__ float pos_gradient(float pos, double half_w) {
    const double t = (double)expf(-fabsf(pos));                 // sigma(-pos) = t / (1 + t) or 1 / (1 + t)
    return -(float)(half_w * ((pos >= 0.f ? t : (pos < 0.f ? 1.0 : (double)pos)) / (1.0 + t)));
}

__global__ __launch_bounds__(kNsThreads) void k_ns_grad_small(NsArgs a, int shift, NsGradArgs g) {
    const int lane = threadIdx.x & 63, L = 1 << shift, col = lane & (L - 1), rows = 64 >> shift;
    const int64_t waves = (int64_t)gridDim.x * kNsWaves, turns = (a.B + rows - 1) / rows;
    const float up = g.upstream ? *g.upstream : 1.0f;
    const double half = (double)*g.scale;
    for (int64_t turn = (int64_t)blockIdx.x * kNsWaves + (threadIdx.x >> 6); turn < turns; turn += waves) {
        const int64_t b = turn * rows + (lane >> shift);
        if (b >= a.B || col >= a.K) continue;
        const double half_w = a.weight ? half * (double)a.weight[b] : half;
        float m;
        const float c = row_constant(a, g, b, half_w, m);
        const float s = a.neg[b * a.ld_neg + col];
        const float e = a.adversarial ? expf(fmaf(a.temperature, s, -m)) : 1.0f;
        g.d_neg[b * g.ld_dneg + col] = up * (c * (e * sigmoid(s)));
        if (col == 0) g.d_pos[b] = up * pos_gradient(a.pos[b], half_w);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kNsThreads) void k_ns_grad_rows(NsArgs a, NsGradArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * kNsWaves;
    const float up = g.upstream ? *g.upstream : 1.0f;
    const double half = (double)*g.scale;
    for (int64_t b = (int64_t)blockIdx.x * kNsWaves + (threadIdx.x >> 6); b < a.B; b += waves) {
        const double half_w = a.weight ? half * (double)a.weight[b] : half;
        float m;
        const float c = row_constant(a, g, b, half_w, m);
        const float* __restrict__ row = a.neg + b * a.ld_neg;
        float* __restrict__ out = g.d_neg + b * g.ld_dneg;
        for (int first = lane * 4; first < a.K; first += 256) {
            const f32x4 q = load_quad<VEC>(row, first, a.K);
            f32x4 d;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const float s = q[c4];
                const float e = a.adversarial ? expf(fmaf(a.temperature, s, -m)) : 1.0f;
                d[c4] = up * (c * (e * sigmoid(s)));
            }
            if (VEC && first + 3 < a.K) {
                *reinterpret_cast<f32x4*>(out + first) = d;
            } else {
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4)
                    if (first + c4 < a.K) out[first + c4] = d[c4];
            }
        }
        if (lane == 0) g.d_pos[b] = up * pos_gradient(a.pos[b], half_w);
    }
}

int lane_group_shift(int64_t K) {                              // log2 of the power of two >= K (K <= 32)
    int shift = 0;
    while ((1 << shift) < K) ++shift;
    return shift;
}

int ns_grid(int64_t B, int64_t K) {                            // a wave per turn of rows, capped: the kernels stride
    const int64_t rows = K <= kNsSmallK ? (64 >> lane_group_shift(K)) : 1;
    const int64_t turns = (B + rows - 1) / rows;
    return (int)std::min<int64_t>((turns + kNsWaves - 1) / kNsWaves, kNsGroups);
}

gn_status check_block(const float* pos, const float* neg, int64_t ld_neg, int64_t B, int64_t K) {
    GN_REQUIRE(B >= 1 && K >= 1 && K < (1ll << 31), "the loss needs at least one positive and one negative each (B=%lld, K=%lld)",
               (long long)B, (long long)K);
    GN_REQUIRE(ld_neg >= K, "leading dimension %lld below K = %lld", (long long)ld_neg, (long long)K);
    GN_REQUIRE(pos && neg, "score pointer is null");
    return GN_OK;
}

}  // namespace

extern "C" {

size_t gn_kge_ns_loss_workspace_bytes(int64_t /*num_positives*/) { return (size_t)kNsGroups * 3 * sizeof(double) + 64; }

gn_status gn_kge_ns_loss_forward_f32(const float* pos, const float* neg, int64_t ld_neg, int64_t B, int64_t K, const float* weight,
                                     int adversarial, float temperature, float* loss, float* row_stats, float* scale, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    GN_OK_OR_RETURN(check_block(pos, neg, ld_neg, B, K));
    GN_REQUIRE(loss && scale && (row_stats || !adversarial), "loss / scale / row_stats pointer is null");
    GN_REQUIRE(workspace && workspace_bytes >= gn_kge_ns_loss_workspace_bytes(B) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               "workspace too small or unaligned: need %zu bytes, 8-byte aligned, zero-initialised once", gn_kge_ns_loss_workspace_bytes(B));
    double* partial = static_cast<double*>(workspace);
    unsigned int* counter = reinterpret_cast<unsigned int*>(partial + 3 * kNsGroups);
    const NsArgs a{pos, neg, ld_neg, B, (int)K, weight, adversarial != 0, temperature};
    const int grid = ns_grid(B, K);
    hipStream_t st = gn::as_stream(stream);
    if (K <= kNsSmallK)
        k_ns_loss_small<<<grid, kNsThreads, 0, st>>>(a, lane_group_shift(K), row_stats, partial, counter, loss, scale);
    else if (gn::aligned16(neg) && ld_neg % 4 == 0)
        k_ns_loss_rows<true><<<grid, kNsThreads, 0, st>>>(a, row_stats, partial, counter, loss, scale);
    else
        k_ns_loss_rows<false><<<grid, kNsThreads, 0, st>>>(a, row_stats, partial, counter, loss, scale);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

gn_status gn_kge_ns_loss_backward_f32(const float* pos, const float* neg, int64_t ld_neg, int64_t B, int64_t K, const float* weight,
                                      int adversarial, float temperature, const float* row_stats, const float* scale,
                                      const float* upstream, float* d_pos, float* d_neg, int64_t ld_dneg, void* stream) {
    GN_OK_OR_RETURN(check_block(pos, neg, ld_neg, B, K));
    GN_REQUIRE(ld_dneg >= K, "leading dimension %lld below K = %lld", (long long)ld_dneg, (long long)K);
    GN_REQUIRE(scale && d_pos && d_neg && (row_stats || !adversarial), "scale / gradient / row_stats pointer is null");
    const NsArgs a{pos, neg, ld_neg, B, (int)K, weight, adversarial != 0, temperature};
    const NsGradArgs g{row_stats, scale, upstream, d_pos, d_neg, ld_dneg};
    const int grid = ns_grid(B, K);
    hipStream_t st = gn::as_stream(stream);
    if (K <= kNsSmallK)
        k_ns_grad_small<<<grid, kNsThreads, 0, st>>>(a, lane_group_shift(K), g);
    else if (gn::aligned16(neg) && ld_neg % 4 == 0 && gn::aligned16(d_neg) && ld_dneg % 4 == 0)
        k_ns_grad_rows<true><<<grid, kNsThreads, 0, st>>>(a, g);
    else
        k_ns_grad_rows<false><<<grid, kNsThreads, 0, st>>>(a, g);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

}  // extern "C"
