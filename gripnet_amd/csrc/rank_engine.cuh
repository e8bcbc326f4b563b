// The score engine of filtered ranking and top-k retrieval: queries against every row of a table on the fp32 matrix cores,
// with the known-pair filter and the deterministic top-k lists.  Described at the head of distmult_rank.hip, which runs it
// with the A operand z[u] * D[r] formed on load; kge_rank.hip runs it with prepared query rows (DistMult, ComplEx) and
// shares the filter bitmap and the list merge with its distance engine (TransE, RotatE).
#pragma once
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;                   // waves per workgroup
constexpr int kRows = 16;                   // query rows per wave
constexpr int kStage = 64;                  // columns of z staged per step: four MFMA column tiles
constexpr int kChunk = 2048;                // columns per known-pair bitmap window
constexpr int kChunkWords = kChunk / 32;
constexpr int kCap = 32;                    // top-k: candidate buffer per row
constexpr int kMaxK = 64;
constexpr int kMaxFeatures = 128;

struct RankArgs {
    const float* z; int64_t ld_z; int n; int f;
    const float* d; int64_t ld_d; int R;
    const float* q; int64_t ld_q;                        // PREPARED: the A rows [Q, f] as they stand (d unused)
    const int64_t* u; const int64_t* v; const int64_t* et; int64_t Q;
    const int32_t* rowptr; const int32_t* partners;      // null: no filter
    const int64_t* cand_range;                            // [R][2] candidate range (lo, hi) per relation; null: (0, n)
    int32_t* greater; int32_t* ties;                      // rank
    float* scores; int64_t* ids; int k;                   // top-k
    int32_t* err;
};

__device__ __forceinline__ bool better(float s, int v, float ts, int tv) { return s > ts || (s == ts && v < tv); }

// LDS written by one lane read by another lane of the SAME wave (the top-k lists): keep the compiler from moving LDS
// accesses across this point and wait for the wave's outstanding ones
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// The known-pair bitmap of one query row over the window of kChunk columns that starts at c0: kChunkWords words.  The
// partners [lo, hi) of the row that fall into the window are set by the lanes that share the row (every `step`-th from
// `first`) with LDS integer OR: the same bits whatever the order.
__device__ __forceinline__ void bitmap_clear(uint32_t* bits, int words, int lane) {
    for (int w = lane; w < words; w += 64) bits[w] = 0u;
}

__device__ __forceinline__ void bitmap_set(uint32_t* row_bits, const int32_t* __restrict__ partners, int lo, int hi, int c0,
                                           int first, int step) {
    for (int p = lo + first; p < hi; p += step) {
        const int w = partners[p] - c0;
        if (w >= 0 && w < kChunk) atomicOr(&row_bits[w >> 5], 1u << (w & 31));
    }
}

__device__ __forceinline__ uint32_t bitmap_test(const uint32_t* row_bits, int w) { return (row_bits[w >> 5] >> (w & 31)) & 1u; }

// The candidate range of a query of relation r: cand_range's row (lo, hi), or (0, n) without a table.  False for a row
// that is no sub-range of [0, n] (the caller treats the query as one with an id out of range); then lo = hi = 0.
__device__ __forceinline__ bool query_range(const int64_t* __restrict__ cand_range, int r, int n, int& lo, int& hi) {
    lo = 0; hi = n;
    if (cand_range == nullptr) return true;
    const int64_t l = cand_range[2 * (int64_t)r], h = cand_range[2 * (int64_t)r + 1];
    const bool good = l >= 0 && l <= h && h <= (int64_t)n;
    lo = good ? (int)l : 0;
    hi = good ? (int)h : 0;
    return good;
}

// The union [wlo, whi) of the candidate ranges of a workgroup's valid queries (a lane without one passes lo = INT_MAX,
// hi = 0), agreed on by its four waves through `slots` (LDS, 2 kWaves ints) behind one barrier: every wave runs the same
// number of stages, the scan loop holds __syncthreads.  `slots` may be reused once another barrier has passed.  Without a
// valid query wlo > whi: no stage runs.
__device__ __forceinline__ void workgroup_range(int* slots, int wave, int lane, int lo, int hi, int& wlo, int& whi) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { lo = min(lo, __shfl_xor(lo, off)); hi = max(hi, __shfl_xor(hi, off)); }
    if (lane == 0) { slots[2 * wave] = lo; slots[2 * wave + 1] = hi; }
    __syncthreads();
    wlo = slots[0]; whi = slots[1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { wlo = min(wlo, slots[2 * w]); whi = max(whi, slots[2 * w + 1]); }
}

// Top-k: merge row q's list (cs/ci[0, len)) and buffer ([k, k + cnt)) into the list, run by the row's 16 lanes (lanes
// 16 kq + c16).  Every candidate's rank is the number of candidates better than it (ranks are unique: the order is total),
// ranks < k are kept.  The candidates stay in registers (lane c16 holds c16, c16 + 16, ...) and travel by shuffles inside
// the group; the trip count is the wave's longest merge, so every shuffle runs with the whole wave.
template <int CAP = kCap>
__device__ __forceinline__ void merge_row(float* cs, int* ci, int k, int kq, int c16, int& len, int& cnt, float& ts, int& tv) {
    const int m = len + cnt;
    int mw = max(m, __shfl_xor(m, 16));
    mw = max(mw, __shfl_xor(mw, 32));
    constexpr int kMine = (kMaxK + CAP + 15) / 16;
    float ms[kMine];
    int mi[kMine], mr[kMine];
#pragma unroll
    for (int j = 0; j < kMine; ++j) {
        const int c = c16 + 16 * j;
        const int p = c < len ? c : k + (c - len);
        const bool have = c < m;
        ms[j] = have ? cs[p] : -__builtin_inff();        // (a missing candidate is better than none)
        mi[j] = have ? ci[p] : 0x7fffffff;
        mr[j] = have ? 0 : k;                             // (never written)
    }
#pragma unroll
    for (int j2 = 0; j2 < kMine; ++j2) {
        if (16 * j2 >= mw) {                                // (no candidates from here on; hipcc unrolls the loop with the
            if constexpr (CAP == kCap) break; else continue;  //  early exit at kMine = 6 only, without it at kMine = 12 only)
        }
#pragma unroll
        for (int l2 = 0; l2 < 16; ++l2) {
            const float s = __shfl(ms[j2], 16 * kq + l2);
            const int v = __shfl(mi[j2], 16 * kq + l2);
#pragma unroll
            for (int j = 0; j < kMine; ++j)
                if (16 * j < mw) mr[j] += better(s, v, ms[j], mi[j]) ? 1 : 0;
        }
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < kMine; ++j)
        if (mr[j] < k) { cs[mr[j]] = ms[j]; ci[mr[j]] = mi[j]; }
    wave_sync();
    len = min(k, m);
    cnt = 0;
    if (len == k) { ts = cs[k - 1]; tv = ci[k - 1]; }
}

// The scan of one workgroup.  PREPARED: the A rows are read from a.q as they stand (k_query_rank); otherwise they are
// z[u] * D[r], formed on load (k_dm_rank: the decoder).  RANGED: a.cand_range gives every query a candidate range (the
// _ranged kernels); without it the range test is the parent `v < n` and the scan runs over [0, n) - a template parameter
// because the per-row test and the two range registers per row cost the unranged call 2 - 7 %, measured.
template <int S, bool TOPK, bool PREPARED, bool RANGED>
__device__ __forceinline__ void rank_scan(const RankArgs& a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int KP = 4 * S;                               // padded features
    constexpr int STRIDE = KP + 4;                          // floats per staged column (16-byte rows, banks shifted)
    float* zs = reinterpret_cast<float*>(lds_raw);          // [kStage][STRIDE]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 15, kq = lane >> 4;
    uint32_t* bits = reinterpret_cast<uint32_t*>(zs + kStage * STRIDE) + wave * (kRows * kChunkWords);
    const int KC = a.k + kCap;                              // top-k: list + buffer slots per row
    float* cs = reinterpret_cast<float*>(zs + kStage * STRIDE + kWaves * kRows * kChunkWords) + wave * (2 * kRows * KC);
    int* ci = reinterpret_cast<int*>(cs + kRows * KC);
    const int64_t qb = ((int64_t)blockIdx.x * kWaves + wave) * kRows;
    const int n = a.n;

    // this lane's A row: query qb + col
    const int64_t qa = qb + col;
    int ua = 0, ra = 0, va = 0, loa = 0, hia = 0;             // (loa, hia): the query's candidate range
    bool oka = false;
    if (qa < a.Q) {
        const int64_t uu = a.u[qa], rr = a.et[qa];
        const int64_t vv = TOPK ? 0 : a.v[qa];
        oka = (uint64_t)uu < (uint64_t)n && (uint64_t)rr < (uint64_t)a.R && (uint64_t)vv < (uint64_t)n;
        if constexpr (RANGED) oka = oka && query_range(a.cand_range, (int)rr, n, loa, hia);
        if (oka) { ua = (int)uu; ra = (int)rr; va = (int)vv; }
        else if (kq == 0 && a.err) atomicOr(a.err, 1);
    }
    int wlo = 0, whi = n;                                    // the columns this workgroup scans
    if constexpr (RANGED) workgroup_range(reinterpret_cast<int*>(zs), wave, lane, oka ? loa : 0x7fffffff, oka ? hia : 0, wlo, whi);
    float av[S];
    {
        const float* zu = PREPARED ? a.q + qa * a.ld_q : a.z + (int64_t)ua * a.ld_z;
        const float* dr = a.d + (int64_t)ra * a.ld_d;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int fi = kq * S + s;
            if constexpr (PREPARED) av[s] = (oka && fi < a.f) ? zu[fi] : 0.f;
            else av[s] = (oka && fi < a.f) ? zu[fi] * dr[fi] : 0.f;
        }
    }
    // the output rows of this lane: 4 kq + j
    bool okr[4];
    int vt[4], lor[4] = {0, 0, 0, 0};
    uint32_t wr[4] = {0u, 0u, 0u, 0u};                       // RANGED: candidate v of row j iff (uint32_t)(v - lor[j]) < wr[j]; none for a bad query
    const int wa = oka ? hia - loa : 0;                      // (every shuffle with the whole wave: none inside a condition)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        okr[j] = __shfl((int)oka, 4 * kq + j) != 0;
        vt[j] = __shfl(va, 4 * kq + j);
        if constexpr (RANGED) {
            lor[j] = __shfl(loa, 4 * kq + j);
            wr[j] = (uint32_t)__shfl(wa, 4 * kq + j);
        }
    }
    auto admitted = [&](int v, int j) {
        if constexpr (RANGED) return (uint32_t)(v - lor[j]) < wr[j];
        else return v < n;
    };

    float st[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!TOPK) {
        // prologue tile: B column j = z[v_true of row j]; element (row q, column q) is the scan's value at v_true
        const float* zv = a.z + (int64_t)va * a.ld_z;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int fi = kq * S + s;
            acc = mfma4(av[s], (oka && fi < a.f) ? zv[fi] : 0.f, acc);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) st[j] = __shfl(acc[j], 20 * kq + j);     // lane 16 kq + (4 kq + j), register j
    }

    int gt[4] = {0, 0, 0, 0}, tie[4] = {0, 0, 0, 0};
    int len[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
    float ts[4];
    int tv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { ts[j] = -__builtin_inff(); tv[j] = -1; }

    const bool filter = a.rowptr != nullptr;
    // the stages that hold a column of [wlo, whi); RANGED: the first may lie inside a bitmap window, which is built from its start
    int window = RANGED ? -kChunk : 0;
    for (int c0 = RANGED ? wlo & ~(kStage - 1) : 0; c0 < whi; c0 += kStage) {
        if (filter && (RANGED ? c0 - window >= kChunk : c0 % kChunk == 0)) {
            // this wave's bitmap of columns [window, window + kChunk): the known partners of its 16 rows
            window = c0 - c0 % kChunk;
            __syncthreads();                                 // (the previous window is no longer read)
            bitmap_clear(bits, kRows * kChunkWords, lane);
            __syncthreads();
            if (oka) {
                const int64_t row = (int64_t)ra * n + ua;
                const int lo = a.rowptr[row], hi = a.rowptr[row + 1];
                bitmap_set(bits + col * kChunkWords, a.partners, lo, hi, window, kq, 4);
            }
        }
        __syncthreads();                                     // the previous stage is consumed (and the bitmap is complete)
        for (int idx = threadIdx.x; idx < kStage * KP; idx += 256) {
            const int c = idx / KP, fi = idx - c * KP;
            zs[c * STRIDE + fi] = ((!RANGED || c0 + c >= wlo) && c0 + c < whi && fi < a.f) ? a.z[(int64_t)(c0 + c) * a.ld_z + fi] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kStage / 16; t += 2) {
            if (c0 + 16 * t >= whi) break;
            if (RANGED && c0 + 16 * (t + 2) <= wlo) continue; // (both tiles in front of every range)
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            const float* b0 = zs + (16 * t + col) * STRIDE + kq * S;
            const float* b1 = b0 + 16 * STRIDE;
#pragma unroll
            for (int s4 = 0; s4 < S / 4; ++s4) {
                const float4 p = *reinterpret_cast<const float4*>(b0 + 4 * s4);
                const float4 q = *reinterpret_cast<const float4*>(b1 + 4 * s4);
                acc[0] = mfma4(av[4 * s4 + 0], p.x, acc[0]);
                acc[1] = mfma4(av[4 * s4 + 0], q.x, acc[1]);
                acc[0] = mfma4(av[4 * s4 + 1], p.y, acc[0]);
                acc[1] = mfma4(av[4 * s4 + 1], q.y, acc[1]);
                acc[0] = mfma4(av[4 * s4 + 2], p.z, acc[0]);
                acc[1] = mfma4(av[4 * s4 + 2], q.z, acc[1]);
                acc[0] = mfma4(av[4 * s4 + 3], p.w, acc[0]);
                acc[1] = mfma4(av[4 * s4 + 3], q.w, acc[1]);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int v = c0 + 16 * (t + h) + col;        // this lane's candidate column
                uint32_t known[4] = {0u, 0u, 0u, 0u};
                if (filter) {
                    const int w = v - window;                 // (v < window + kChunk: windows are multiples of the stage)
#pragma unroll
                    for (int j = 0; j < 4; ++j) known[j] = bitmap_test(bits + (4 * kq + j) * kChunkWords, w);
                }
                if constexpr (!TOPK) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool cand = admitted(v, j) && v != vt[j] && !known[j];
                        gt[j] += (cand && !(acc[h][j] <= st[j])) ? 1 : 0;   // (NaN on either side counts: never flatters)
                        tie[j] += (cand && acc[h][j] == st[j]) ? 1 : 0;
                    }
                } else {
                    const int K = a.k;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float s = acc[h][j];
                        const bool pass = admitted(v, j) && !known[j] && better(s, v, ts[j], tv[j]);
                        const uint64_t m = __ballot(pass);
                        const uint32_t g = (uint32_t)(m >> (16 * kq)) & 0xFFFFu;
                        if (pass) {
                            const int slot = (4 * kq + j) * KC + K + cnt[j] + __popc(g & ((1u << col) - 1u));
                            cs[slot] = s;
                            ci[slot] = v;
                        }
                        cnt[j] += __popc(g);
                    }
                    // a buffer that could overflow on the next tile: merge every row of the wave
                    const bool full = cnt[0] > kCap - 16 || cnt[1] > kCap - 16 || cnt[2] > kCap - 16 || cnt[3] > kCap - 16;
                    if (__ballot(full) != 0) {
                        wave_sync();
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            merge_row(cs + (4 * kq + j) * KC, ci + (4 * kq + j) * KC, K, kq, col, len[j], cnt[j], ts[j], tv[j]);
                    }
                }
            }
        }
    }

    if constexpr (!TOPK) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
#pragma unroll
            for (int j = 0; j < 4; ++j) { gt[j] += __shfl_xor(gt[j], off); tie[j] += __shfl_xor(tie[j], off); }
        if (col < 4) {                                        // lane 16 kq + j writes row 4 kq + j
            int g = gt[0], e = tie[0];
#pragma unroll
            for (int j = 1; j < 4; ++j) if (col == j) { g = gt[j]; e = tie[j]; }
            const int64_t q = qb + 4 * kq + col;
            bool ok = okr[0];
#pragma unroll
            for (int j = 1; j < 4; ++j) if (col == j) ok = okr[j];
            if (q < a.Q) {
                a.greater[q] = ok ? g : -1;
                a.ties[q] = ok ? e : -1;
            }
        }
    } else {
        const int K = a.k;
        const bool left = cnt[0] > 0 || cnt[1] > 0 || cnt[2] > 0 || cnt[3] > 0;
        if (__ballot(left) != 0) {
            wave_sync();
#pragma unroll
            for (int j = 0; j < 4; ++j)
                merge_row(cs + (4 * kq + j) * KC, ci + (4 * kq + j) * KC, K, kq, col, len[j], cnt[j], ts[j], tv[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t q = qb + 4 * kq + j;
            if (q >= a.Q) continue;
            const float* rs = cs + (4 * kq + j) * KC;
            const int* ri = ci + (4 * kq + j) * KC;
            for (int e = col; e < K; e += 16) {
                const bool have = okr[j] && e < len[j];
                a.scores[q * K + e] = have ? rs[e] : (okr[j] ? -__builtin_inff() : __builtin_nanf(""));
                a.ids[q * K + e] = have ? (int64_t)ri[e] : -1;
            }
        }
    }
}

template <int S, bool TOPK>
__global__ __launch_bounds__(256) void k_dm_rank(RankArgs a) { rank_scan<S, TOPK, false, false>(a); }

template <int S, bool TOPK>
__global__ __launch_bounds__(256) void k_query_rank(RankArgs a) { rank_scan<S, TOPK, true, false>(a); }

template <int S, bool TOPK>
__global__ __launch_bounds__(256) void k_dm_rank_ranged(RankArgs a) { rank_scan<S, TOPK, false, true>(a); }

template <int S, bool TOPK>
__global__ __launch_bounds__(256) void k_query_rank_ranged(RankArgs a) { rank_scan<S, TOPK, true, true>(a); }

template <int S, bool TOPK, bool PREPARED>
gn_status launch_s(const RankArgs& a, size_t lds, size_t lds_max, hipStream_t st) {
    auto plain = [] { if constexpr (PREPARED) return &k_query_rank<S, TOPK>; else return &k_dm_rank<S, TOPK>; }();
    auto ranged = [] { if constexpr (PREPARED) return &k_query_rank_ranged<S, TOPK>; else return &k_dm_rank_ranged<S, TOPK>; }();
    auto kernel = a.cand_range ? ranged : plain;
    if (lds > 64 * 1024) {                                   // (the opt-in is made once per kernel: for the largest k)
        const gn_status ls = gn::allow_large_lds(reinterpret_cast<const void*>(kernel), (int)lds_max);
        if (ls != GN_OK) return ls;
    }
    const unsigned grid = (unsigned)gn::ceil_div(a.Q, (int64_t)kWaves * kRows);
    kernel<<<grid, 256, lds, st>>>(a);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

template <bool TOPK, bool PREPARED = false>
gn_status launch(const RankArgs& a, int S, hipStream_t st) {
    if (S < 4 || S > 32 || S % 4 != 0) return gn::fail(GN_ERR_UNSUPPORTED, "ranking kernels take at most %d features", kMaxFeatures);
    auto lds_of = [&](int k) {
        return (size_t)kStage * (4 * S + 4) * 4 + (size_t)kWaves * kRows * kChunkWords * 4 + (TOPK ? (size_t)kWaves * kRows * (k + kCap) * 8 : 0);
    };
    switch (S) {
#define GN_RANK_CASE(s) case s: return launch_s<s, TOPK, PREPARED>(a, lds_of(a.k), lds_of(kMaxK), st);
        GN_RANK_CASE(4) GN_RANK_CASE(8) GN_RANK_CASE(12) GN_RANK_CASE(16) GN_RANK_CASE(20) GN_RANK_CASE(24) GN_RANK_CASE(28) GN_RANK_CASE(32)
#undef GN_RANK_CASE
    }
    return GN_OK;
}

gn_status fill_args(RankArgs& a, const float* z, int64_t ld_z, int64_t n, int64_t f, const float* d, int64_t ld_d, int64_t R,
                    const int64_t* u, const int64_t* et, int64_t Q, const gn_known_pairs* known, const int64_t* cand_range,
                    int32_t* err, int& S) {
    GN_REQUIRE(n >= 0 && f >= 1 && R >= 0 && Q >= 0, "bad size (n=%lld, features=%lld, R=%lld, queries=%lld)",
               (long long)n, (long long)f, (long long)R, (long long)Q);
    GN_REQUIRE(n < (1ll << 31) && R < (1ll << 31) && Q < (1ll << 40), "table too large");
    if (f > kMaxFeatures) return gn::fail(GN_ERR_UNSUPPORTED, "ranking kernels take at most %d features (got %lld)", kMaxFeatures, (long long)f);
    GN_REQUIRE(ld_z >= f && ld_d >= f, "leading dimension smaller than the row length");
    if (known) GN_REQUIRE(known->num_nodes == n && known->num_relations == R,
                          "known pairs were built for %lld nodes and %lld relations, the call has %lld and %lld",
                          (long long)known->num_nodes, (long long)known->num_relations, (long long)n, (long long)R);
    a = RankArgs{};
    a.z = z; a.ld_z = ld_z; a.n = (int)n; a.f = (int)f; a.d = d; a.ld_d = ld_d; a.R = (int)R;
    a.u = u; a.et = et; a.Q = Q; a.err = err; a.cand_range = cand_range;
    if (known) { a.rowptr = known->rowptr.p; a.partners = known->partners.p; }
    S = (int)((f + 15) / 16) * 4;
    return GN_OK;
}

}  // namespace

