// Filtered ranking and top-k partner retrieval for the DistMult decoder (link-prediction evaluation).
//
// A query is a row (u, r); its candidate scores are the logits s(v) = sum_k z[u,k] D[r,k] z[v,k] for every v in [0, n):
// one row of the skinny product (z[u] * D[r]) @ z^T, K = num_features.  One score engine, two epilogues:
//   rank  (gn_distmult_rank_f32): per query (u, r, v_true) the counts of the non-known candidates v != v_true with
//         s(v) > s(v_true) and s(v) == s(v_true);
//   top-k (gn_distmult_topk_f32): per query (u, r) the k <= 64 best non-known candidates, score descending then id ascending.
// Nothing of the [Q, n] score matrix reaches memory.
//
// Engine.  A workgroup is four waves; a wave owns 16 query rows (the M of v_mfma_f32_16x16x4_f32, an exact fp32 FMA chain
// on gfx950).  Its A operand, z[u] * D[r] per row (rows of different relations share a tile), is formed on load and kept in
// registers for the whole scan: lane l holds features kq * S + s (kq = l >> 4, s < S) of row l & 15, the features padded
// with zeros to 4 S (a multiple of 16).  z streams through LDS as B, 64 columns (four 16-column MFMA tiles) per stage,
// shared by the four waves; every wave runs two tiles' chains interleaved.  Output element (row 4 (l >> 4) + j, column
// l & 15) sits in register j of lane l.
//
// The true score.  An MFMA output element depends only on its A row, its B column and the order of the K steps, so the
// rank kernel computes s(v_true) in a prologue tile whose B column j is z[v_true] of the wave's query j (the same floats
// the stage holds for that column), through the same chain: the diagonal of that tile is bit-identical to what the scan
// computes at column v_true.  A pair recomputed in another order could count itself as a near-tie or a "greater".
//
// Filter.  gn_known_pairs (negsample.hip) keeps one sorted partner row per (r, u).  Per window of 2,048 columns every wave
// sets the bits of its 16 rows' partners in a [16][64]-word LDS bitmap (LDS integer OR: the same bits whatever the order);
// the epilogue tests one bit per output element.
//
// Top-k.  Per row the wave keeps a list of up to k entries (sorted) and a buffer of kCap candidates in LDS, and in
// registers the list's last entry as a threshold.  An element that beats the threshold is appended (slot from a ballot
// prefix: no atomics, the same slots every run); before a buffer can overflow, list and buffer are merged by rank counting
// (the order is total: ids are unique), which is deterministic as well.
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
    const int64_t* u; const int64_t* v; const int64_t* et; int64_t Q;
    const int32_t* rowptr; const int32_t* partners;      // null: no filter
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

// Top-k: merge row q's list (cs/ci[0, len)) and buffer ([k, k + cnt)) into the list, run by the row's 16 lanes (lanes
// 16 kq + c16).  Every candidate's rank is the number of candidates better than it (ranks are unique: the order is total),
// ranks < k are kept.  The candidates stay in registers (lane c16 holds c16, c16 + 16, ...) and travel by shuffles inside
// the group; the trip count is the wave's longest merge, so every shuffle runs with the whole wave.
__device__ __forceinline__ void merge_row(float* cs, int* ci, int k, int kq, int c16, int& len, int& cnt, float& ts, int& tv) {
    const int m = len + cnt;
    int mw = max(m, __shfl_xor(m, 16));
    mw = max(mw, __shfl_xor(mw, 32));
    constexpr int kMine = (kMaxK + kCap + 15) / 16;
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
        if (16 * j2 >= mw) break;
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

template <int S, bool TOPK>
__global__ __launch_bounds__(256) void k_dm_rank(RankArgs a) {
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
    int ua = 0, ra = 0, va = 0;
    bool oka = false;
    if (qa < a.Q) {
        const int64_t uu = a.u[qa], rr = a.et[qa];
        const int64_t vv = TOPK ? 0 : a.v[qa];
        oka = (uint64_t)uu < (uint64_t)n && (uint64_t)rr < (uint64_t)a.R && (uint64_t)vv < (uint64_t)n;
        if (oka) { ua = (int)uu; ra = (int)rr; va = (int)vv; }
        else if (kq == 0 && a.err) atomicOr(a.err, 1);
    }
    float av[S];
    {
        const float* zu = a.z + (int64_t)ua * a.ld_z;
        const float* dr = a.d + (int64_t)ra * a.ld_d;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int fi = kq * S + s;
            av[s] = (oka && fi < a.f) ? zu[fi] * dr[fi] : 0.f;
        }
    }
    // the output rows of this lane: 4 kq + j
    bool okr[4];
    int vt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        okr[j] = __shfl((int)oka, 4 * kq + j) != 0;
        vt[j] = __shfl(va, 4 * kq + j);
    }

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
    int window = 0;
    for (int c0 = 0; c0 < n; c0 += kStage) {
        if (filter && c0 % kChunk == 0) {
            // this wave's bitmap of columns [c0, c0 + kChunk): the known partners of its 16 rows
            window = c0;
            __syncthreads();                                 // (the previous window is no longer read)
            for (int w = lane; w < kRows * kChunkWords; w += 64) bits[w] = 0u;
            __syncthreads();
            if (oka) {
                const int64_t row = (int64_t)ra * n + ua;
                const int lo = a.rowptr[row], hi = a.rowptr[row + 1];
                for (int p = lo + kq; p < hi; p += 4) {
                    const int w = a.partners[p] - c0;
                    if (w >= 0 && w < kChunk) atomicOr(&bits[col * kChunkWords + (w >> 5)], 1u << (w & 31));
                }
            }
        }
        __syncthreads();                                     // the previous stage is consumed (and the bitmap is complete)
        for (int idx = threadIdx.x; idx < kStage * KP; idx += 256) {
            const int c = idx / KP, fi = idx - c * KP;
            zs[c * STRIDE + fi] = (c0 + c < n && fi < a.f) ? a.z[(int64_t)(c0 + c) * a.ld_z + fi] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kStage / 16; t += 2) {
            if (c0 + 16 * t >= n) break;
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
                    for (int j = 0; j < 4; ++j) known[j] = (bits[(4 * kq + j) * kChunkWords + (w >> 5)] >> (w & 31)) & 1u;
                }
                if constexpr (!TOPK) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool cand = v < n && v != vt[j] && !known[j];
                        gt[j] += (cand && acc[h][j] > st[j]) ? 1 : 0;
                        tie[j] += (cand && acc[h][j] == st[j]) ? 1 : 0;
                    }
                } else {
                    const int K = a.k;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float s = acc[h][j];
                        const bool pass = v < n && !known[j] && better(s, v, ts[j], tv[j]);
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

template <bool TOPK>
gn_status launch(const RankArgs& a, int S, hipStream_t st) {
    const void* fn = nullptr;
    switch (S) {
#define GN_RANK_CASE(s) case s: fn = reinterpret_cast<const void*>(k_dm_rank<s, TOPK>); break;
        GN_RANK_CASE(4) GN_RANK_CASE(8) GN_RANK_CASE(12) GN_RANK_CASE(16) GN_RANK_CASE(20) GN_RANK_CASE(24) GN_RANK_CASE(28) GN_RANK_CASE(32)
#undef GN_RANK_CASE
        default: return gn::fail(GN_ERR_UNSUPPORTED, "ranking kernels take at most %d features", kMaxFeatures);
    }
    auto lds_of = [&](int k) {
        return (size_t)kStage * (4 * S + 4) * 4 + (size_t)kWaves * kRows * kChunkWords * 4 + (TOPK ? (size_t)kWaves * kRows * (k + kCap) * 8 : 0);
    };
    const size_t lds = lds_of(a.k);
    if (lds > 64 * 1024) {                                   // (the opt-in is made once per kernel: for the largest k)
        const gn_status ls = gn::allow_large_lds(fn, (int)lds_of(kMaxK));
        if (ls != GN_OK) return ls;
    }
    const unsigned grid = (unsigned)gn::ceil_div(a.Q, (int64_t)kWaves * kRows);
    switch (S) {
#define GN_RANK_CASE(s) case s: k_dm_rank<s, TOPK><<<grid, 256, lds, st>>>(a); break;
        GN_RANK_CASE(4) GN_RANK_CASE(8) GN_RANK_CASE(12) GN_RANK_CASE(16) GN_RANK_CASE(20) GN_RANK_CASE(24) GN_RANK_CASE(28) GN_RANK_CASE(32)
#undef GN_RANK_CASE
    }
    GN_LAUNCH_CHECK();
    return GN_OK;
}

gn_status fill_args(RankArgs& a, const float* z, int64_t ld_z, int64_t n, int64_t f, const float* d, int64_t ld_d, int64_t R,
                    const int64_t* u, const int64_t* et, int64_t Q, const gn_known_pairs* known, int32_t* err, int& S) {
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
    a.u = u; a.et = et; a.Q = Q; a.err = err;
    if (known) { a.rowptr = known->rowptr.p; a.partners = known->partners.p; }
    S = (int)((f + 15) / 16) * 4;
    return GN_OK;
}

}  // namespace

extern "C" {

gn_status gn_distmult_rank_f32(const float* z, int64_t ld_z, int64_t n, int64_t f, const float* d, int64_t ld_d, int64_t R,
                               const int64_t* u, const int64_t* v, const int64_t* et, int64_t Q, const gn_known_pairs* known,
                               int32_t* greater, int32_t* ties, int32_t* err, void* stream) {
    RankArgs a;
    int S = 0;
    const gn_status s = fill_args(a, z, ld_z, n, f, d, ld_d, R, u, et, Q, known, err, S);
    if (s != GN_OK) return s;
    if (Q == 0) return GN_OK;
    GN_REQUIRE(z && d && u && v && et && greater && ties, "operand pointer is null");
    GN_REQUIRE(n > 0 && R > 0, "queries given but the node or relation table is empty");
    a.v = v; a.greater = greater; a.ties = ties;
    return launch<false>(a, S, gn::as_stream(stream));
}

gn_status gn_distmult_topk_f32(const float* z, int64_t ld_z, int64_t n, int64_t f, const float* d, int64_t ld_d, int64_t R,
                               const int64_t* u, const int64_t* et, int64_t Q, int64_t k, const gn_known_pairs* known,
                               float* scores, int64_t* ids, int32_t* err, void* stream) {
    GN_REQUIRE(k >= 1 && k <= kMaxK, "k must be in [1, %d], got %lld", kMaxK, (long long)k);
    RankArgs a;
    int S = 0;
    const gn_status s = fill_args(a, z, ld_z, n, f, d, ld_d, R, u, et, Q, known, err, S);
    if (s != GN_OK) return s;
    if (Q == 0) return GN_OK;
    GN_REQUIRE(z && d && u && et && scores && ids, "operand pointer is null");
    GN_REQUIRE(n > 0 && R > 0, "queries given but the node or relation table is empty");
    a.scores = scores; a.ids = ids; a.k = (int)k;
    return launch<true>(a, S, gn::as_stream(stream));
}

}  // extern "C"
