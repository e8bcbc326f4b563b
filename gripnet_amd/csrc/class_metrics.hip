// Node-classification metrics on the device: argmax, per-class counts, precision / recall / F1, micro / macro F1, accuracy.
//
// Every epoch of the node-classification drivers computes `pred = torch.argmax(score, dim=1)` and then
// `micro_macro(classes, pred)`, once in train() and once in test() (GripNet-aminer.py:130-137,153-156;
// GripNet-freebase-c.py:165-172,188-191): two device -> host copies and two scikit-learn f1_score calls each time
// (gripnet/utils.py:38-52).  Here it is two launches:
//   1. k_class_count: a grid-stride pass over the rows.  A row is a lane (C <= 8) or a group of 8 / 64 lanes that reduces
//      (value, index) pairs over shuffles with torch.argmax's order; the row's (true, predicted) ids are counted per
//      workgroup in LDS: a wave takes the distinct classes of its rows one at a time (ballot + popcount per class, one LDS
//      integer add per class and wave).  Each workgroup writes its counts as one int32 partial row to the workspace.
//   2. k_class_finalize: one workgroup adds the partials (integers: the sum does not depend on the order), then writes the
//      counts, the per-class ratios (one float64 division of exact integers each) and the summary.  The macro mean adds the
//      F1 of the classes present in the labels or the predictions in numpy's pairwise order, so it has scikit-learn's bits.
// No float atomics, no host synchronisation, no allocation: the call is graph-capturable.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kCountThreads = 256;
constexpr int kMaxGroups = 512;               // workgroups of the counting pass (partials the finalize adds)
constexpr int kMaxClasses = 1024;
constexpr int kFinThreads = 1024;             // one thread per class in the finalize
constexpr int kErrClassId = 8;                // bit of *error_flag: a class id outside [0, C)

// Partial row of a workgroup: [0, C) support, [C, 2C) predicted, [2C, 3C) correct, 3C all correct rows, 3C + 1 rows with
// an id out of range; padded to a multiple of 4 ints.
inline int partial_stride(int C) { return (3 * C + 2 + 3) & ~3; }
constexpr int kMaxStride = (3 * kMaxClasses + 2 + 3) & ~3;

inline int lanes_per_row(int C) { return C <= 8 ? 1 : (C <= 128 ? 8 : 64); }

// workgroups of the counting pass at W lanes per row (the workspace is sized for the score mode's W: the prediction mode,
// a lane per row, never needs more)
inline int count_groups(int64_t n, int W) {
    const int64_t rows_per_group = kCountThreads / W;
    return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGroups, (n + rows_per_group - 1) / rows_per_group));
}

// torch.argmax's order (CPU and GPU alike): NaN above every number, the first NaN wins; otherwise the larger value, and of
// equal values (+0.0 and -0.0 among them) the lower index.  A total order on (value, index): the reduction may pair in any order.
__device__ __forceinline__ bool beats(float v, int i, float bv, int bi) {
    const bool vn = __builtin_isnan(v), bn = __builtin_isnan(bv);
    if (vn) return !bn || i < bi;
    if (bn) return false;
    return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ void take(float v, int i, float& bv, int& bi) {
    if (beats(v, i, bv, bi)) { bv = v; bi = i; }
}

struct CountArgs {
    const float* score; int64_t ld;
    const int64_t* pred_in;
    const int64_t* classes;
    int64_t n;
    int C, S;
    int64_t* pred_out;
    int32_t* err;
    int32_t* part;                // [gridDim.x][S]
};

// W lanes per row (1, 8, 64); PRED: the predictions are given; VEC: the score rows start 16-byte aligned (float4 loads).
template <int W, bool PRED, bool VEC>
__global__ __launch_bounds__(kCountThreads) void k_class_count(CountArgs a) {
    __shared__ int cnt[kMaxStride];
    const int tid = threadIdx.x, lane = tid & 63, g = tid % W;
    const int C = a.C;
    for (int j = tid; j < a.S; j += kCountThreads) cnt[j] = 0;
    __syncthreads();
    constexpr int kRows = kCountThreads / W;                  // rows of a workgroup per iteration
    int bad_rows = 0;
    for (int64_t base = (int64_t)blockIdx.x * kRows; base < a.n; base += (int64_t)gridDim.x * kRows) {   // uniform
        const int64_t i = base + tid / W;
        const bool has = i < a.n;
        int64_t p = -1;
        if constexpr (PRED) {
            if (has) p = a.pred_in[i];
        } else {
            float bv = -__builtin_inff();                     // (-inf, INT_MAX) loses to every element of the row
            int bi = 0x7fffffff;
            if (has) {
                const float* __restrict__ row = a.score + i * a.ld;
                int j0 = 0;
                if constexpr (VEC) {
                    const int nq = C >> 2;
                    for (int q = g; q < nq; q += W) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
                        take(v[0], 4 * q, bv, bi); take(v[1], 4 * q + 1, bv, bi);
                        take(v[2], 4 * q + 2, bv, bi); take(v[3], 4 * q + 3, bv, bi);
                    }
                    j0 = 4 * nq;
                }
                for (int j = j0 + g; j < C; j += W) take(row[j], j, bv, bi);
            }
#pragma unroll
            for (int off = W / 2; off > 0; off >>= 1) {
                const float ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                take(ov, oi, bv, bi);
            }
            p = bi;
        }
        const bool leader = has && g == 0;
        int64_t y = -1;
        if (leader) y = a.classes[i];
        const bool ok = leader && (uint64_t)y < (uint64_t)C && (uint64_t)p < (uint64_t)C;
        if (leader && !ok) ++bad_rows;
        if (!PRED && leader && a.pred_out) a.pred_out[i] = p;
        const int yi = ok ? (int)y : -1, pi = ok ? (int)p : -1;
        const unsigned long long okm = __ballot(ok);
        const unsigned long long hit = __ballot(ok && yi == pi);
        if (lane == 0 && hit) atomicAdd(&cnt[3 * C], __popcll(hit));
        // the distinct true classes of the wave's rows, one at a time: support and correct
        for (unsigned long long rest = okm; rest;) {
            const int c = __shfl(yi, __ffsll((long long)rest) - 1);
            const unsigned long long m = __ballot(ok && yi == c);
            rest &= ~m;
            if (lane == 0) {
                atomicAdd(&cnt[c], __popcll(m));
                if (m & hit) atomicAdd(&cnt[2 * C + c], __popcll(m & hit));
            }
        }
        // the distinct predicted classes: predicted
        for (unsigned long long rest = okm; rest;) {
            const int c = __shfl(pi, __ffsll((long long)rest) - 1);
            const unsigned long long m = __ballot(ok && pi == c);
            rest &= ~m;
            if (lane == 0) atomicAdd(&cnt[C + c], __popcll(m));
        }
    }
    if (bad_rows) {
        atomicAdd(&cnt[3 * C + 1], bad_rows);
        if (a.err) atomicOr(a.err, kErrClassId);
    }
    __syncthreads();
    int32_t* __restrict__ part = a.part + (size_t)blockIdx.x * a.S;
    for (int j = tid; j < a.S; j += kCountThreads) part[j] = cnt[j];
}

// numpy's pairwise summation of a float64 vector (what np.mean adds with): blocks of at most 128 in eight interleaved sums,
// longer ranges cut in two at a multiple of 8.  D levels of cuts reach every n <= 1024 (four are needed).
__device__ __forceinline__ double pairwise_leaf(const double* a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

template <int D>
__device__ __forceinline__ double pairwise_sum(const double* a, int n) {
    if constexpr (D == 0) {
        return pairwise_leaf(a, n);
    } else {
        if (n <= 128) return pairwise_leaf(a, n);
        const int n2 = (n / 2) - (n / 2) % 8;
        return pairwise_sum<D - 1>(a, n2) + pairwise_sum<D - 1>(a + n2, n - n2);
    }
}

// One workgroup: the partials' sums, then counts [3][C] (int64), per_class [3][C] and summary [3] (float64).
// P = slices the workgroups' partials are split into when a partial row is short (P S <= 1024 threads add in parallel).
__global__ __launch_bounds__(kFinThreads) void k_class_finalize(const int32_t* __restrict__ part, int G, int C, int S, int P, int64_t n,
                                                                int64_t* __restrict__ counts, double* __restrict__ per_class,
                                                                double* __restrict__ summary) {
    __shared__ long long red[kFinThreads];
    __shared__ long long tot[kMaxStride];
    __shared__ double f1c[kMaxClasses];
    __shared__ int wcnt[kFinThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (P > 1) {
        if (t < P * S) {
            const int s = t / S, j = t - s * S;
            long long acc = 0;
            for (int b = s; b < G; b += P) acc += part[(size_t)b * S + j];
            red[t] = acc;
        }
        __syncthreads();
        if (t < S) {
            long long acc = 0;
            for (int s = 0; s < P; ++s) acc += red[s * S + t];
            tot[t] = acc;
        }
    } else {
        for (int j = t; j < S; j += kFinThreads) {
            long long acc = 0;
            for (int b = 0; b < G; ++b) acc += part[(size_t)b * S + j];
            tot[j] = acc;
        }
    }
    __syncthreads();
    const bool bad = tot[3 * C + 1] != 0;
    const double nan = __builtin_nan("");
    double f1 = 0.0;
    bool present = false;
    if (t < C) {
        const long long sup = tot[t], prd = tot[C + t], tp = tot[2 * C + t];
        counts[t] = sup;
        counts[C + t] = prd;
        counts[2 * C + t] = tp;
        // scikit-learn's divisions (precision_recall_fscore_support, beta = 1, zero_division = 0): exact integers, one rounding
        const double prec = prd ? (double)tp / (double)prd : 0.0;
        const double rec = sup ? (double)tp / (double)sup : 0.0;
        f1 = (sup + prd) ? (2.0 * (double)tp) / (double)(sup + prd) : 0.0;
        present = sup + prd > 0;
        per_class[t] = bad ? nan : prec;
        per_class[C + t] = bad ? nan : rec;
        per_class[2 * C + t] = bad ? nan : f1;
    }
    // the F1 of the present classes, compacted in class order (unique_labels of the labels and the predictions)
    const unsigned long long m = __ballot(present);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, L = 0;
    for (int w = 0; w < kFinThreads / 64; ++w) {
        before += w < wave ? wcnt[w] : 0;
        L += wcnt[w];
    }
    if (present) f1c[before + __popcll(m & ((1ull << lane) - 1))] = f1;
    __syncthreads();
    if (t == 0) {
        const double T = (double)tot[3 * C];
        const double macro = L ? pairwise_sum<4>(f1c, L) / (double)L : nan;
        summary[0] = bad ? nan : (n ? T / (double)n : 0.0);      // micro-F1 = 2T / 2n: the same quotient as T / n
        summary[1] = bad ? nan : macro;
        summary[2] = bad ? nan : (n ? T / (double)n : nan);      // accuracy
    }
}

template <int W>
void launch_count(bool pred, bool vec, int grid, const CountArgs& a, hipStream_t st) {
    if (pred) k_class_count<1, true, false><<<grid, kCountThreads, 0, st>>>(a);
    else if (vec) k_class_count<W, false, true><<<grid, kCountThreads, 0, st>>>(a);
    else k_class_count<W, false, false><<<grid, kCountThreads, 0, st>>>(a);
}

}  // namespace

extern "C" {

size_t gn_class_metrics_workspace_bytes(int64_t n, int64_t num_class) {
    if (n < 0 || num_class < 1 || num_class > kMaxClasses) return 0;
    const int C = (int)num_class;
    return (size_t)count_groups(n, lanes_per_row(C)) * partial_stride(C) * sizeof(int32_t);
}

gn_status gn_class_metrics_f32(const float* score, int64_t ld_score, const int64_t* pred_in, const int64_t* classes, int64_t n,
                               int64_t num_class, int64_t* pred_out, int64_t* counts, double* per_class, double* summary,
                               int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream) {
    if (num_class < 1 || num_class > kMaxClasses)
        return gn::fail(GN_ERR_UNSUPPORTED, "class metrics: num_class %lld outside [1, %d]", (long long)num_class, kMaxClasses);
    if (n > 0x7fffffffll) return gn::fail(GN_ERR_UNSUPPORTED, "class metrics: %lld rows exceed 2^31 - 1", (long long)n);
    GN_REQUIRE(n >= 0, "class metrics: negative row count %lld", (long long)n);
    GN_REQUIRE(!(score && pred_in) && (score || pred_in || n == 0), "class metrics: give exactly one of score and pred_in");
    GN_REQUIRE(score == nullptr || ld_score >= num_class || n <= 1, "class metrics: ld_score %lld < num_class %lld",
               (long long)ld_score, (long long)num_class);
    GN_REQUIRE(n == 0 || classes != nullptr, "class metrics: classes is null");
    GN_REQUIRE(counts && per_class && summary, "class metrics: null output pointer");
    const int C = (int)num_class;
    const size_t need = gn_class_metrics_workspace_bytes(n, num_class);
    GN_REQUIRE(workspace != nullptr && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
               "class metrics: workspace too small or not 4-byte aligned: need %zu bytes", need);
    hipStream_t st = gn::as_stream(stream);
    const bool pred = pred_in != nullptr;
    const int W = pred ? 1 : lanes_per_row(C), G = count_groups(n, W), S = partial_stride(C);
    CountArgs a{score, ld_score, pred_in, classes, n, C, S, pred_in ? nullptr : pred_out, error_flag,
                static_cast<int32_t*>(workspace)};
    const bool vec = !pred && (reinterpret_cast<uintptr_t>(score) & 15) == 0 && (n <= 1 || ld_score % 4 == 0);
    if (W == 1) launch_count<1>(pred, vec, G, a, st);
    else if (W == 8) launch_count<8>(pred, vec, G, a, st);
    else launch_count<64>(pred, vec, G, a, st);
    GN_LAUNCH_CHECK();
    int P = 1;
    while (P < 16 && 2 * P * S <= kFinThreads) P *= 2;
    k_class_finalize<<<1, kFinThreads, 0, st>>>(static_cast<const int32_t*>(workspace), G, C, S, P, n, counts, per_class, summary);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

}  // extern "C"
