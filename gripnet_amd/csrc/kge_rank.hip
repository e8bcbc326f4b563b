// Filtered ranking and top-k retrieval for the knowledge-graph-embedding baselines (KGEModel.rank / .top_k).
//
// A query is (fixed entity, relation) and a side: on the tail side the fixed entity is the head and every entity is a
// candidate tail, on the head side the fixed entity is the tail and every entity is a candidate head.  Per query the
// raw score of kge.hip against each of the n candidates; rank counts the non-known candidates NOT below-or-equal and equal
// to the true partner's score (a NaN on either side counts as greater: a non-finite score never flatters the model), top-k
// keeps the k <= 64 best (score descending, id ascending; NaN and -inf never enter).  Nothing of a [Q, n] score matrix or a
// [Q, n, D] difference block reaches memory.  The known-pair rows are keyed (relation, fixed entity): for the head side the
// caller builds the gn_known_pairs from the flipped lists.
//
// Inner-product engine (DistMult, ComplEx).  The score is a dot product of a prepared query row with the candidate's row:
//   DistMult, either side   q = fixed * r
//   ComplEx, tail side      q = (hr rr - hi ri, hr ri + hi rr)   against (tr, ti)
//   ComplEx, head side      q = (rr tr + ri ti, rr ti - ri tr)   against (hr, hi)
// k_kge_query writes the rows [Q, De] to scratch (every product rounded by itself), and the engine of rank_engine.cuh -
// fp32 MFMA 16x16x4 with the entity table streamed through LDS - takes them as its A operand.  Entity rows of at most 128
// floats: H <= 128 (DistMult), H <= 64 (ComplEx).
//
// Distance engine (TransE, RotatE): k_kge_dist.  An L1 norm and a sum of complex moduli have no matrix-instruction form;
// this runs on the vector ALU, candidate-stationary:
//   * a workgroup is four waves, a wave owns kDistQueries = 8 queries for the whole scan;
//   * the entity table streams through LDS in stages of 64 rows ([64][EW + 1] floats, EW the padded row: the odd stride
//     puts the 32 lanes of a ds_read_b32 half on 32 banks), staged once per workgroup and read by its four waves;
//   * a lane copies ONE candidate's row from the stage into registers (EW <= 128 VGPRs) and keeps it while the wave's
//     eight queries pass by; a query's operands lie in LDS as planes of W columns and are read as wave-uniform
//     ds_read_b128 broadcasts: tail side the head_part of kge_term.cuh, prepared once per query (TransE h + r: one subtract
//     and one |.|-add per candidate and column; RotatE the rotated head), head side the relation operand and the tail
//     (TransE r, t; RotatE cos, sin, tr, ti) - the arithmetic is term<M> with the operands in the model's own roles;
//   * the column sum is ONE serial chain over the columns 0 .. W - 1 (padding columns add an exact +0), so a score is a
//     function of the query's bits, the candidate row's bits and nothing else: equal rows tie, in any stage or window;
//   * rank: the true partner's score comes from a prologue in which lane j holds the row of query j's true partner and
//     runs the same scan code; the comparison is a ballot and a population count, the counters live in lane j;
//   * top-k: one list per query in LDS ([k] sorted + a buffer of kDistCap = 128), its length, fill and threshold in lane j;
//     a candidate that beats the threshold takes a slot from the ballot's prefix count; a buffer that the next stage could
//     overflow (> 64 entries) is merged by merge_row's rank counting - no float atomics, the same bits in every run;
//   * filter: per window of 2,048 columns a [8][64]-word bitmap per wave (bitmap_set of rank_engine.cuh);
//   * candidate ranges (RANGED; the _ranged entry points): lane j keeps the range (lo, hi) of query j's relation next to
//     its filter row, the workgroup scans the stages that hold a candidate of the union of its queries' ranges and a
//     candidate is admitted per query iff lo <= v < hi; a score does not depend on where the scan starts, so the result is
//     the full scan's restricted to the range, bit for bit.
// Budget at the widest row (EW = 128, head side): registers 128 (row) + ~40; LDS 33 KB stage + 32 KB queries
// (4 waves x 8 x 256 floats) + 8 KB bitmaps + (top-k) 4 x 8 x (k + 128) x 8 B <= 48 KB: 121 KB of the CU's 160, one
// workgroup per CU, one wave per SIMD.  At the driver's H = 32 (RotatE: EW = 64): 16.6 + 16 + 8 + 35 KB.
// The operands are the Tables of kge_rows.cuh, made ready by its make_tables as for every KGE entry point (DistArgs takes
// their members over at the scan loops' widths: embedding the struct cost two of k_kge_dist's lines 1 - 3 %, measured).
#include "kge_rows.cuh"
#include "rank_engine.cuh"

namespace {

constexpr int kDistQueries = 8;              // queries per wave
constexpr int kDistCap = 128;                // top-k: candidate buffer per query (a stage appends up to 64)
constexpr int kDistStage = 64;               // candidates per stage: one per lane

struct DistArgs {
    const float* ent; int64_t ld_ent; int n; int h;                 // Tables' members at the widths the scan loops use
    const float* rel; const float* rel_im; int64_t ld_rel; int R;   // TransE: the table; RotatE: cos and sin of its phases
    const int64_t* fixed; const int64_t* truth; const int64_t* et; int64_t Q;
    const int32_t* rowptr; const int32_t* partners;                 // null: no filter
    const int64_t* cand_range;                                       // [R][2] candidate range per relation; null: (0, n)
    float gamma;
    int32_t* greater; int32_t* ties;                                // rank
    float* scores; int64_t* ids; int k;                             // top-k
    int32_t* err;
};

template <int M, int SIDE, int W> struct DistShape {
    static constexpr int P = Traits<M>::ent_parts;
    static constexpr int EW = P * W;                                 // a candidate's padded row
    static constexpr int QF = SIDE == kTailSide ? P * W : 2 * P * W; // a query's operand planes
    static constexpr int STRIDE = EW + 1;
};

// The score of the candidate row `row` (registers: real columns [0, W), imaginary [W, 2 W)) for the query whose planes
// start at `q` (LDS, wave-uniform).  One chain over the columns in order; rank's prologue and both scans run THIS code.
template <int M, int SIDE, int W>
__device__ __forceinline__ float scan_score(const float* q, const float (&row)[DistShape<M, SIDE, W>::EW], float gamma) {
#pragma clang fp contract(off)
    constexpr int P = DistShape<M, SIDE, W>::P;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < W; c += 4) {
        float x[4][4];                                               // [plane][column]
#pragma unroll
        for (int p = 0; p < DistShape<M, SIDE, W>::QF / W; ++p) {
            const float4 t = *reinterpret_cast<const float4*>(q + p * W + c);
            x[p][0] = t.x; x[p][1] = t.y; x[p][2] = t.z; x[p][3] = t.w;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float er = row[c + v], ei = P == 2 ? row[(P - 1) * W + c + v] : 0.f;
            if constexpr (SIDE == kTailSide) {
                acc += tail_term<M>(x[0][v], P == 2 ? x[P - 1][v] : 0.f, er, ei);
            } else if constexpr (M == kTransE) {
                acc += term<M>(Col{er, 0.f, x[0][v], 0.f, x[1][v], 0.f});
            } else {
                acc += term<M>(Col{er, ei, x[0][v], x[1][v], x[2][v], x[3][v]});
            }
        }
    }
    return finish<M>(acc, gamma);
}

// RANGED: a.cand_range gives every query a candidate range; without it the range test is `v < n` and the scan runs over
// [0, n), the kernel as it was before the ranges (a template parameter for the reason given at rank_engine.cuh's rank_scan).
template <int M, int SIDE, bool TOPK, int W, bool RANGED>
__global__ __launch_bounds__(256) void k_kge_dist(DistArgs a) {
    using Sh = DistShape<M, SIDE, W>;
    constexpr int P = Sh::P, EW = Sh::EW, QF = Sh::QF, STRIDE = Sh::STRIDE, QW = kDistQueries;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* zs = reinterpret_cast<float*>(lds_raw);                              // [kDistStage][STRIDE]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kq = lane >> 4, c16 = lane & 15;
    float* qs = zs + kDistStage * STRIDE + wave * (QW * QF);                    // [QW][QF]   (16-byte rows: STRIDE is odd, 64 * 4 * odd)
    uint32_t* bits = reinterpret_cast<uint32_t*>(zs + kDistStage * STRIDE + kWaves * QW * QF) + wave * (QW * kChunkWords);
    const int KC = a.k + kDistCap;
    float* cs = reinterpret_cast<float*>(zs + kDistStage * STRIDE + kWaves * QW * QF + kWaves * QW * kChunkWords) + wave * (2 * QW * KC);
    int* ci = reinterpret_cast<int*>(cs + QW * KC);
    const int64_t qb = ((int64_t)blockIdx.x * kWaves + wave) * QW;
    const int n = a.n, h = a.h;
    const bool filter = a.rowptr != nullptr;

    // lane j < QW keeps query qb + j: its ids, its filter row, its candidate range, its counters or its list's state
    int fx = 0, rl = 0, tr = 0, f_lo = 0, f_hi = 0, c_lo = 0, c_hi = 0;
    bool ok = false;
    if (lane < QW && qb + lane < a.Q) {
        const int64_t ff = a.fixed[qb + lane], rr = a.et[qb + lane];
        const int64_t tt = TOPK ? 0 : a.truth[qb + lane];
        ok = (uint64_t)ff < (uint64_t)n && (uint64_t)rr < (uint64_t)a.R && (uint64_t)tt < (uint64_t)n;
        if constexpr (RANGED) ok = ok && query_range(a.cand_range, (int)rr, n, c_lo, c_hi);
        if (ok) {
            fx = (int)ff; rl = (int)rr; tr = (int)tt;
            if (filter) {
                const int64_t row = (int64_t)rl * n + fx;
                f_lo = a.rowptr[row]; f_hi = a.rowptr[row + 1];
            }
        } else if (a.err) {
            atomicOr(a.err, 1);
        }
    }
    const uint32_t c_w = ok ? (uint32_t)(c_hi - c_lo) : 0u;  // RANGED: candidate v of query j iff (uint32_t)(v - c_lo) < c_w; none for a bad query
    int wlo = 0, whi = n;                                    // the candidates this workgroup scans (the stage is not written before the loop's first barrier)
    if constexpr (RANGED) workgroup_range(reinterpret_cast<int*>(zs), wave, lane, ok ? c_lo : 0x7fffffff, ok ? c_hi : 0, wlo, whi);

    // the queries' operand planes
    for (int j = 0; j < QW; ++j) {
        const bool okj = __shfl((int)ok, j) != 0;
        const float* pe = a.ent + (int64_t)__shfl(fx, j) * a.ld_ent;
        const float* pr = a.rel + (int64_t)__shfl(rl, j) * a.ld_rel;
        const float* pi = a.rel_im + (int64_t)__shfl(rl, j) * a.ld_rel;
        for (int c = lane; c < W; c += 64) {
            const bool in = okj && c < h;
            Col col = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (in) {
                col.rr = pr[c];
                if constexpr (P == 2) col.ri = pi[c];
                if constexpr (SIDE == kTailSide) { col.hr = pe[c]; if constexpr (P == 2) col.hi = pe[h + c]; }
                else { col.tr = pe[c]; if constexpr (P == 2) col.ti = pe[h + c]; }
            }
            float* q = qs + j * QF + c;
            if constexpr (SIDE == kTailSide) {
                float p0, p1;
                head_part<M>(col, p0, p1);
                q[0] = p0;
                if constexpr (P == 2) q[W] = p1;
            } else if constexpr (M == kTransE) {
                q[0] = col.rr; q[W] = col.tr;
            } else {
                q[0] = col.rr; q[W] = col.ri; q[2 * W] = col.tr; q[3 * W] = col.ti;
            }
        }
    }
    __syncthreads();

    float row[EW];
    float st = 0.f;                                         // rank: lane j keeps s(true partner) of query j
    if constexpr (!TOPK) {
        // prologue: lane j's candidate is the true partner of query j, scored by the scan's own code
        const float* pt = a.ent + (int64_t)tr * a.ld_ent;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int c = 0; c < W; ++c) row[p * W + c] = (ok && c < h) ? pt[p * h + c] : 0.f;
        for (int j = 0; j < QW; ++j) {
            const float s = scan_score<M, SIDE, W>(qs + j * QF, row, a.gamma);
            if (lane == j) st = s;
        }
    }

    int gt = 0, tie = 0;                                    // rank
    int len = 0, cnt = 0, tv = -1;                          // top-k: list length, buffer fill, the threshold (ts, tv)
    float ts = -__builtin_inff();
    const int K = a.k;

    // top-k: merge the lists of all QW queries; group kq of 16 lanes merges query 4 i + kq in round i
    auto merge_all = [&]() {
        wave_sync();
#pragma unroll
        for (int i = 0; i < QW / 4; ++i) {
            const int r = 4 * i + kq;
            int rlen = __shfl(len, r), rcnt = __shfl(cnt, r), rtv = __shfl(tv, r);
            float rts = __shfl(ts, r);
            merge_row<kDistCap>(cs + r * KC, ci + r * KC, K, kq, c16, rlen, rcnt, rts, rtv);
            const int src = 16 * (lane & 3);                // lane 4 i + g takes group g's results
            const int nlen = __shfl(rlen, src), ncnt = __shfl(rcnt, src), ntv = __shfl(rtv, src);
            const float nts = __shfl(rts, src);
            if ((lane >> 2) == i) { len = nlen; cnt = ncnt; ts = nts; tv = ntv; }
        }
    };

    // the stages that hold a candidate of [wlo, whi); RANGED: the first may lie inside a bitmap window, which is built from its start
    int window = 0;
    const int c_first = RANGED ? wlo & ~(kDistStage - 1) : 0;
    for (int c0 = c_first; c0 < (RANGED ? whi : n); c0 += kDistStage) {
        if (filter && (c0 % kChunk == 0 || (RANGED && c0 == c_first))) {
            window = RANGED ? c0 - c0 % kChunk : c0;
            __syncthreads();                                 // (the previous window is no longer read)
            bitmap_clear(bits, QW * kChunkWords, lane);
            __syncthreads();
            for (int j = 0; j < QW; ++j)
                bitmap_set(bits + j * kChunkWords, a.partners, __shfl(f_lo, j), __shfl(f_hi, j), window, lane, 64);
        }
        __syncthreads();                                     // the previous stage is consumed (and the bitmap is complete)
        for (int idx = threadIdx.x; idx < kDistStage * EW; idx += 256) {
            const int c = idx / EW, fi = idx - c * EW;
            const int p = fi / W, k = fi - p * W;
            zs[c * STRIDE + fi] = ((!RANGED || c0 + c >= wlo) && c0 + c < (RANGED ? whi : n) && k < h) ? a.ent[(int64_t)(c0 + c) * a.ld_ent + p * h + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int fi = 0; fi < EW; ++fi) row[fi] = zs[lane * STRIDE + fi];
        const int v = c0 + lane;                             // this lane's candidate
        const bool inr = RANGED || v < n;
        for (int j = 0; j < QW; ++j) {
            const float s = scan_score<M, SIDE, W>(qs + j * QF, row, a.gamma);
            const bool known = filter && bitmap_test(bits + j * kChunkWords, v - window) != 0u;
            bool okj;                                         // (every shuffle with the whole wave: none inside a condition)
            if constexpr (RANGED) {                           // a valid query that admits v
                const int lo_j = __shfl(c_lo, j);
                const uint32_t w_j = __shfl(c_w, j);
                okj = (uint32_t)(v - lo_j) < w_j;
            } else {
                okj = __shfl((int)ok, j) != 0;
            }
            if constexpr (!TOPK) {
                const float sj = __shfl(st, j);
                const int vj = __shfl(tr, j);
                const bool cand = inr && okj && !known && v != vj;
                const int g = __popcll(__ballot(cand && !(s <= sj))), e = __popcll(__ballot(cand && s == sj));   // (NaN on either side counts)
                if (lane == j) { gt += g; tie += e; }
            } else {
                const float tsj = __shfl(ts, j);
                const int tvj = __shfl(tv, j), cntj = __shfl(cnt, j);
                const bool pass = inr && okj && !known && better(s, v, tsj, tvj);
                const uint64_t m = __ballot(pass);
                if (m != 0) {
                    if (pass) {
                        const int slot = j * KC + K + cntj + __popcll(m & ((1ull << lane) - 1ull));
                        cs[slot] = s;
                        ci[slot] = v;
                    }
                    if (lane == j) cnt += __popcll(m);
                }
            }
        }
        if constexpr (TOPK) {
            if (__ballot(cnt > kDistCap - kDistStage) != 0) merge_all();      // the next stage could overflow a buffer
        }
    }

    if constexpr (!TOPK) {
        if (lane < QW && qb + lane < a.Q) {
            a.greater[qb + lane] = ok ? gt : -1;
            a.ties[qb + lane] = ok ? tie : -1;
        }
    } else {
        if (__ballot(cnt > 0) != 0) merge_all();
        wave_sync();
        for (int j = 0; j < QW; ++j) {
            const int64_t q = qb + j;
            if (q >= a.Q) break;
            const bool okj = __shfl((int)ok, j) != 0;
            const int lj = __shfl(len, j);
            for (int e = lane; e < K; e += 64) {
                const bool have = okj && e < lj;
                a.scores[q * K + e] = have ? cs[j * KC + e] : (okj ? -__builtin_inff() : __builtin_nanf(""));
                a.ids[q * K + e] = have ? (int64_t)ci[j * KC + e] : -1;
            }
        }
    }
}

template <int M, int SIDE, bool TOPK, int W>
gn_status launch_dist_w(const DistArgs& a, hipStream_t st) {
    using Sh = DistShape<M, SIDE, W>;
    auto lds_of = [](int k) {
        return (size_t)kDistStage * Sh::STRIDE * 4 + (size_t)kWaves * kDistQueries * Sh::QF * 4 +
               (size_t)kWaves * kDistQueries * kChunkWords * 4 + (TOPK ? (size_t)kWaves * kDistQueries * (k + kDistCap) * 8 : 0);
    };
    const size_t lds = lds_of(a.k);
    auto kernel = a.cand_range ? &k_kge_dist<M, SIDE, TOPK, W, true> : &k_kge_dist<M, SIDE, TOPK, W, false>;
    if (lds > 64 * 1024)                                      // (the opt-in is made once per kernel: for the largest k)
        GN_OK_OR_RETURN(gn::allow_large_lds(reinterpret_cast<const void*>(kernel), (int)lds_of(kMaxK)));
    const unsigned grid = (unsigned)gn::ceil_div(a.Q, (int64_t)kWaves * kDistQueries);
    kernel<<<grid, 256, lds, st>>>(a);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

template <int M, int SIDE, bool TOPK>
gn_status launch_dist(const DistArgs& a, hipStream_t st) {
    if (a.h <= 8) return launch_dist_w<M, SIDE, TOPK, 8>(a, st);
    if (a.h <= 16) return launch_dist_w<M, SIDE, TOPK, 16>(a, st);
    if (a.h <= 32) return launch_dist_w<M, SIDE, TOPK, 32>(a, st);
    if (a.h <= 64) return launch_dist_w<M, SIDE, TOPK, 64>(a, st);
    if constexpr (M == kTransE) return launch_dist_w<M, SIDE, TOPK, 128>(a, st);
    return gn::fail(GN_ERR_UNSUPPORTED, "the ranking kernels take entity rows of at most %d floats", kMaxFeatures);
}

template <bool TOPK>
gn_status launch_dist_model(int model, int side, const DistArgs& a, hipStream_t st) {
    if (model == kTransE)
        return side == kTailSide ? launch_dist<kTransE, kTailSide, TOPK>(a, st) : launch_dist<kTransE, kHeadSide, TOPK>(a, st);
    return side == kTailSide ? launch_dist<kRotatE, kTailSide, TOPK>(a, st) : launch_dist<kRotatE, kHeadSide, TOPK>(a, st);
}

// ---- the inner-product models' query rows ------------------------------------------------------------------------------
struct QueryArgs {
    Tables t;
    const int64_t* fixed; const int64_t* et; int64_t Q;
    float* q;                                                        // [Q, De]
};

// q[query] per the table at the head of the file; a query with an id outside its table gets zeros (the engine flags it)
template <int M, int SIDE>
__global__ void k_kge_query(QueryArgs a) {
#pragma clang fp contract(off)
    constexpr int P = Traits<M>::ent_parts;
    const int h = a.t.h;
    const int64_t total = a.Q * h;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t query = i / h;
        const int c = (int)(i - query * h);
        const int64_t ff = a.fixed[query], rr = a.et[query];
        float q0 = 0.f, q1 = 0.f;
        if (in_tables(a.t, ff, ff, rr)) {
            const float* pe = a.t.ent + ff * a.t.ld_ent;
            const float* pr = a.t.rel + rr * a.t.ld_rel;
            if constexpr (SIDE == kTailSide || M == kDistMult) {
                const Col col = {pe[c], P == 2 ? pe[h + c] : 0.f, pr[c], P == 2 ? pr[h + c] : 0.f, 0.f, 0.f};
                head_part<M>(col, q0, q1);
            } else {
                const float tr = pe[c], ti = pe[h + c], wr = pr[c], wi = pr[h + c];
                q0 = wr * tr + wi * ti;
                q1 = wr * ti - wi * tr;
            }
        }
        float* out = a.q + query * (int64_t)(P * h);
        out[c] = q0;
        if constexpr (P == 2) out[h + c] = q1;
    }
}

// the [Q, De] query rows of the inner-product models (the distance models have the trig tables there instead)
size_t query_bytes(int model, int64_t h, int64_t q) {
    return model == kDistMult || model == kComplEx ? gn::seg_align_up((size_t)entity_parts(model) * q * h * sizeof(float)) : 0;
}

struct Call {
    int model, side;
    const float* ent; int64_t ld_ent, n; const float* rel; int64_t ld_rel, R, h;
    const int64_t* fixed; const int64_t* truth; const int64_t* et; int64_t Q;
    float gamma, divisor; const gn_known_pairs* known; const int64_t* cand_range;
    int32_t* greater; int32_t* ties; float* scores; int64_t* ids; int k;
    int32_t* err; void* ws; size_t ws_bytes; hipStream_t st;
};

template <bool TOPK>
gn_status run(const Call& c) {
    GN_REQUIRE(c.model >= kTransE && c.model <= kRotatE, "unknown model %d (0 TransE, 1 DistMult, 2 ComplEx, 3 RotatE)", c.model);
    GN_REQUIRE(c.side == kTailSide || c.side == kHeadSide, "unknown side %d (0 tail, 1 head)", c.side);
    GN_REQUIRE(c.n >= 0 && c.R >= 0 && c.h >= 1 && c.Q >= 0, "bad size (n=%lld, R=%lld, hidden=%lld, queries=%lld)",
               (long long)c.n, (long long)c.R, (long long)c.h, (long long)c.Q);
    GN_REQUIRE(c.n < (1ll << 31) && c.R < (1ll << 31) && c.Q < (1ll << 40), "table too large");
    const int64_t de = entity_parts(c.model) * c.h, dr = relation_parts(c.model) * c.h;
    if (de > kMaxFeatures)
        return gn::fail(GN_ERR_UNSUPPORTED, "the ranking kernels take entity rows of at most %d floats (got %lld)", kMaxFeatures, (long long)de);
    GN_REQUIRE(c.ld_ent >= de && c.ld_rel >= dr, "leading dimension smaller than the row length");
    if (c.known) GN_REQUIRE(c.known->num_nodes == c.n && c.known->num_relations == c.R,
                            "known pairs were built for %lld entities and %lld relations, the call has %lld and %lld",
                            (long long)c.known->num_nodes, (long long)c.known->num_relations, (long long)c.n, (long long)c.R);
    if (c.Q == 0) return GN_OK;
    GN_REQUIRE(c.ent && c.rel && c.fixed && c.et, "operand pointer is null");
    GN_REQUIRE(c.n > 0 && c.R > 0, "queries given but the entity or relation table is empty");
    const size_t need = trig_bytes(c.model, c.R, c.h) + query_bytes(c.model, c.h, c.Q);
    GN_REQUIRE(need == 0 || (c.ws && c.ws_bytes >= need && gn::aligned16(c.ws)), "workspace too small: need %zu bytes (16-byte aligned)", need);
    Tables t;
    GN_OK_OR_RETURN(make_tables(t, c.model, c.ent, c.ld_ent, c.n, c.rel, c.ld_rel, c.R, c.h, c.divisor, c.ws, c.ws_bytes, c.st));

    if (c.model == kDistMult || c.model == kComplEx) {
        QueryArgs qa = {t, c.fixed, c.et, c.Q, static_cast<float*>(c.ws)};
        const int grid = gn::stream_grid(c.Q * c.h, 256);
        if (c.model == kDistMult) k_kge_query<kDistMult, kTailSide><<<grid, 256, 0, c.st>>>(qa);
        else if (c.side == kTailSide) k_kge_query<kComplEx, kTailSide><<<grid, 256, 0, c.st>>>(qa);
        else k_kge_query<kComplEx, kHeadSide><<<grid, 256, 0, c.st>>>(qa);
        GN_LAUNCH_CHECK();
        RankArgs a;
        int S = 0;
        GN_OK_OR_RETURN(fill_args(a, c.ent, c.ld_ent, c.n, de, nullptr, de, c.R, c.fixed, c.et, c.Q, c.known, c.cand_range, c.err, S));
        a.q = qa.q; a.ld_q = de;
        a.v = c.truth; a.greater = c.greater; a.ties = c.ties; a.scores = c.scores; a.ids = c.ids; a.k = c.k;
        return launch<TOPK, true>(a, S, c.st);
    }

    DistArgs a = {};
    a.ent = t.ent; a.ld_ent = t.ld_ent; a.n = (int)t.n; a.h = t.h;
    a.rel = t.rel; a.rel_im = t.rel_im; a.ld_rel = t.ld_rel; a.R = (int)t.r;
    a.fixed = c.fixed; a.truth = c.truth; a.et = c.et; a.Q = c.Q;
    if (c.known) { a.rowptr = c.known->rowptr.p; a.partners = c.known->partners.p; }
    a.cand_range = c.cand_range;
    a.gamma = c.gamma; a.greater = c.greater; a.ties = c.ties; a.scores = c.scores; a.ids = c.ids; a.k = c.k; a.err = c.err;
    return launch_dist_model<TOPK>(c.model, c.side, a, c.st);
}

}  // namespace

extern "C" {

size_t gn_kge_rank_workspace_bytes(int model, int64_t r, int64_t h, int64_t q) {
    if (r < 0 || h < 0 || q < 0) return 0;
    return trig_bytes(model, r, h) + query_bytes(model, h, q);
}

gn_status gn_kge_rank_ranged_f32(int model, int side, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                 int64_t r, int64_t h, const int64_t* fixed, const int64_t* truth, const int64_t* et, int64_t q,
                                 float gamma, float phase_divisor, const gn_known_pairs* known, int32_t* greater, int32_t* ties,
                                 int32_t* err, void* workspace, size_t workspace_bytes, void* stream, const int64_t* cand_range) {
    GN_REQUIRE(q <= 0 || (truth && greater && ties), "operand pointer is null");
    const Call c = {model, side, ent, ld_ent, n, rel, ld_rel, r, h, fixed, truth, et, q, gamma, phase_divisor, known, cand_range,
                    greater, ties, nullptr, nullptr, 0, err, workspace, workspace_bytes, gn::as_stream(stream)};
    return run<false>(c);
}

gn_status gn_kge_rank_f32(int model, int side, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                          int64_t r, int64_t h, const int64_t* fixed, const int64_t* truth, const int64_t* et, int64_t q,
                          float gamma, float phase_divisor, const gn_known_pairs* known, int32_t* greater, int32_t* ties,
                          int32_t* err, void* workspace, size_t workspace_bytes, void* stream) {
    return gn_kge_rank_ranged_f32(model, side, ent, ld_ent, n, rel, ld_rel, r, h, fixed, truth, et, q, gamma, phase_divisor, known,
                                  greater, ties, err, workspace, workspace_bytes, stream, nullptr);
}

gn_status gn_kge_topk_ranged_f32(int model, int side, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                 int64_t r, int64_t h, const int64_t* fixed, const int64_t* et, int64_t q, int64_t k, float gamma,
                                 float phase_divisor, const gn_known_pairs* known, float* scores, int64_t* ids, int32_t* err,
                                 void* workspace, size_t workspace_bytes, void* stream, const int64_t* cand_range) {
    GN_REQUIRE(k >= 1 && k <= kMaxK, "k must be in [1, %d], got %lld", kMaxK, (long long)k);
    GN_REQUIRE(q <= 0 || (scores && ids), "operand pointer is null");
    const Call c = {model, side, ent, ld_ent, n, rel, ld_rel, r, h, fixed, nullptr, et, q, gamma, phase_divisor, known, cand_range,
                    nullptr, nullptr, scores, ids, (int)k, err, workspace, workspace_bytes, gn::as_stream(stream)};
    return run<true>(c);
}

gn_status gn_kge_topk_f32(int model, int side, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                          int64_t r, int64_t h, const int64_t* fixed, const int64_t* et, int64_t q, int64_t k, float gamma,
                          float phase_divisor, const gn_known_pairs* known, float* scores, int64_t* ids, int32_t* err,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return gn_kge_topk_ranged_f32(model, side, ent, ld_ent, n, rel, ld_rel, r, h, fixed, et, q, k, gamma, phase_divisor, known,
                                  scores, ids, err, workspace, workspace_bytes, stream, nullptr);
}

}  // extern "C"
