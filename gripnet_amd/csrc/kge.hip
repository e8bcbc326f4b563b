// Knowledge-graph-embedding scorers of the link-prediction baselines (KGEModel.forward,
// baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:127-235) and their gradients:
//
//   h = Ent[head_e]   t = Ent[tail_e]   r = Rel[type_e]           out[e] = logsigmoid?( s_e )
//   TransE    s = gamma - sum_k |h_k + r_k - t_k|
//   DistMult  s = sum_k h_k r_k t_k
//   ComplEx   s = sum_k (hr rr - hi ri) tr + (hr ri + hi rr) ti        (real part: columns [0, H), imaginary: [H, 2H))
//   RotatE    s = gamma - sum_k sqrt(a_k^2 + b_k^2),  a = hr cos - hi sin - tr,  b = hr sin + hi cos - ti,  theta = r / divisor
//
// Forward: the kernel shape of k_distmult (distmult.hip) - a lane per triple streams the ids, a lane group per triple
// reads 16-byte pieces of the three rows, folds in a fixed order, and the scores leave in one coalesced store per wave.  A
// lane owns a real piece and the matching imaginary piece.  The tables (19.7 k x 64 floats in the driver: 5 MB) stay in L2 /
// Infinity Cache; nothing is planned, the negatives change every step.  RotatE's cos / sin are evaluated once per call for
// the [R, H] relation table (k_kge_trig), not once per triple and column.
//
// Backward: the rule of distmult_bwd.hip - no float atomics.  Per pass (key = head, key = tail, key = relation) 16-byte
// records (head, tail, relation, g) are sorted by key (rocPRIM radix sort, stable); the sorted array is cut into chunks of
// kChunkRecs records, one workgroup each; a row that lies inside a chunk is final, a row that continues in a neighbour chunk
// leaves a partial that k_kge_combine adds in chunk order.  g = grad_out * sigma(-s) when the forward returned the
// log-sigmoid.  The contribution of a record is g * ds/d(row), a function of the three rows per model and role.
#include "common.h"
#include "kge_term.cuh"
#include "plan_device.cuh"
#include "seg_sort.cuh"

namespace {

enum { kHead = 0, kTail = 1, kRelation = 2 };

// ds / d(row of ROLE) for one column: (d0, d1) = derivative with respect to the real and the imaginary member (d1 unused
// by the real models).  RotatE's relation derivative is with respect to the phase's source r = theta * divisor: d0 only.
// torch's conventions: sign(0) = 0 (TransE), a zero-length (a, b) contributes nothing (RotatE).
template <int M, int ROLE>
__device__ __forceinline__ void dscore(const Col& c, float divisor, float& d0, float& d1) {
#pragma clang fp contract(off)
    d0 = 0.f; d1 = 0.f;
    if constexpr (M == kTransE) {
        const float d = (c.hr + c.rr) - c.tr;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        d0 = ROLE == kTail ? sg : -sg;
    } else if constexpr (M == kDistMult) {
        d0 = ROLE == kHead ? c.rr * c.tr : (ROLE == kTail ? c.hr * c.rr : c.hr * c.tr);
    } else if constexpr (M == kComplEx) {
        if constexpr (ROLE == kHead) {
            d0 = c.rr * c.tr + c.ri * c.ti;
            d1 = c.rr * c.ti - c.ri * c.tr;
        } else if constexpr (ROLE == kTail) {
            d0 = c.hr * c.rr - c.hi * c.ri;
            d1 = c.hr * c.ri + c.hi * c.rr;
        } else {
            d0 = c.hr * c.tr + c.hi * c.ti;
            d1 = c.hr * c.ti - c.hi * c.tr;
        }
    } else {
        const float a = (c.hr * c.rr - c.hi * c.ri) - c.tr;
        const float b = (c.hr * c.ri + c.hi * c.rr) - c.ti;
        const float m = sqrtf(a * a + b * b);
        if (m > 0.f) {
            const float ua = a / m, ub = b / m;
            if constexpr (ROLE == kHead) {
                d0 = -(ua * c.rr + ub * c.ri);
                d1 = ua * c.ri - ub * c.rr;
            } else if constexpr (ROLE == kTail) {
                d0 = ua;
                d1 = ub;
            } else {
                // d a / d theta = -hr sin - hi cos,  d b / d theta = hr cos - hi sin
                const float dth = ua * (c.hr * c.ri + c.hi * c.rr) - ub * (c.hr * c.rr - c.hi * c.ri);
                d0 = dth / divisor;                          // the backward of `relation / divisor`
            }
        }
    }
}

struct Tables {
    const float* ent; int64_t ld_ent; int64_t n;
    const float* rel; int64_t ld_rel;              // RotatE: the cos table
    const float* rel_im; int64_t r;                // ComplEx: rel + H; RotatE: the sin table
    int h;
};

// the VEC columns [k, k + VEC) of a triple's three rows
template <int M, int VEC>
__device__ __forceinline__ void load_cols(const Tables& t, int hh, int tt, int rr, int k, Col (&c)[VEC]) {
    const float* ph = t.ent + (int64_t)hh * t.ld_ent + k;
    const float* pt = t.ent + (int64_t)tt * t.ld_ent + k;
    const float* pr = t.rel + (int64_t)rr * t.ld_rel + k;
    const float* pri = t.rel_im + (int64_t)rr * t.ld_rel + k;
    constexpr bool two = Traits<M>::ent_parts == 2;
    if constexpr (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(ph);
        const float4 b = *reinterpret_cast<const float4*>(pt);
        const float4 w = *reinterpret_cast<const float4*>(pr);
        float4 ai = a, bi = b, wi = w;
        if constexpr (two) {
            ai = *reinterpret_cast<const float4*>(ph + t.h);
            bi = *reinterpret_cast<const float4*>(pt + t.h);
            wi = *reinterpret_cast<const float4*>(pri);
        }
        c[0] = {a.x, ai.x, w.x, wi.x, b.x, bi.x};
        c[1] = {a.y, ai.y, w.y, wi.y, b.y, bi.y};
        c[2] = {a.z, ai.z, w.z, wi.z, b.z, bi.z};
        c[3] = {a.w, ai.w, w.w, wi.w, b.w, bi.w};
    } else {
        c[0] = {ph[0], two ? ph[t.h] : 0.f, pr[0], two ? pri[0] : 0.f, pt[0], two ? pt[t.h] : 0.f};
    }
}

struct FwdArgs {
    Tables t;
    const int64_t* head; const int64_t* tail; const int64_t* et;
    int64_t e; float gamma; int log_sigmoid; int group;     // lanes per triple: a power of two, 1..16
    float* out; float* raw; int32_t* err;
};

__device__ __forceinline__ float log_sigmoid(float s) { return fminf(s, 0.f) - log1pf(expf(-fabsf(s))); }

template <int M, int VEC>
__global__ __launch_bounds__(256) void k_kge_forward(FwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int group = a.group, slots = 64 / group;
    const int slot = lane / group, j = lane % group;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int units = a.t.h / VEC;

    for (int64_t e0 = wave * 64; e0 < a.e; e0 += n_waves * 64) {
        const int64_t mine = e0 + lane;
        int64_t mh = 0, mt = 0, mr = 0;
        bool ok = true;
        if (mine < a.e) {
            mh = a.head[mine]; mt = a.tail[mine]; mr = a.et[mine];
            ok = (uint64_t)mh < (uint64_t)a.t.n && (uint64_t)mt < (uint64_t)a.t.n && (uint64_t)mr < (uint64_t)a.t.r;
            if (!ok) { mh = mt = mr = 0; }
        }
        const int ih = (int)mh, it_ = (int)mt, ir = (int)mr;       // validated: the tables have fewer than 2^31 rows
        const int cnt = (int)min((int64_t)64, a.e - e0);
        float result = 0.f;
        for (int it = 0; it * slots < cnt; ++it) {
            const int idx = it * slots + slot;
            const int hh = __shfl(ih, idx & 63), tt = __shfl(it_, idx & 63), rr = __shfl(ir, idx & 63);
            float acc = 0.f;
            if (idx < cnt) {
                for (int c = j; c < units; c += group) {
                    Col col[VEC];
                    load_cols<M, VEC>(a.t, hh, tt, rr, c * VEC, col);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc += term<M>(col[v]);
                }
            }
            for (int off = 1; off < group; off <<= 1) acc += __shfl_xor(acc, off);
            // lane l keeps the score of triple e0 + l: iteration l / slots, slot l % slots
            const float got = __shfl(acc, (lane % slots) * group);
            if (lane / slots == it) result = got;
        }
        if (mine < a.e) {
            result = finish<M>(result, a.gamma);
            if (!ok) {
                result = __builtin_nanf("");
                if (a.err) atomicOr(a.err, 1);
            }
            if (a.raw) a.raw[mine] = result;
            a.out[mine] = a.log_sigmoid ? log_sigmoid(result) : result;
        }
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct Rec { uint32_t h, t, r; float g; };      // 16 bytes; h = kSkip: a triple with an id outside its table
constexpr uint32_t kSkip = 0xffffffffu;
constexpr int kChunkRecs = gn::kSegChunkRecs;
constexpr int kPartialPerChunk = 2 * 2 * 64;    // floats: [first / last row of the chunk][part][64 columns]

size_t align_up(size_t v) { return gn::seg_align_up(v); }

// keys == null: the records stay in list order (a relation pass over a sorted edge_type)
__global__ void k_kge_recs(int role, const int64_t* __restrict__ head, const int64_t* __restrict__ tail,
                           const int64_t* __restrict__ et, const float* __restrict__ grad_out,
                           const float* __restrict__ raw, int64_t E, int64_t n, int64_t R, uint32_t num_keys,
                           uint32_t* __restrict__ keys, Rec* __restrict__ recs) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t hh = head[e], tt = tail[e], rr = et[e];
        const bool ok = (uint64_t)hh < (uint64_t)n && (uint64_t)tt < (uint64_t)n && (uint64_t)rr < (uint64_t)R;
        Rec rec = {kSkip, 0u, 0u, 0.f};
        uint32_t key = num_keys;                         // sorted past the last row, never read
        if (ok) {
            float g = grad_out[e];
            if (raw) {                                       // d logsigmoid(s) / d s = sigma(-s), without an overflow of exp
                const float s = raw[e], ex = expf(-fabsf(s));
                g = g * (s > 0.f ? ex / (1.0f + ex) : 1.0f / (1.0f + ex));
            }
            rec = {(uint32_t)hh, (uint32_t)tt, (uint32_t)rr, g};
            key = role == kHead ? rec.h : (role == kTail ? rec.t : rec.r);
        }
        if (keys) keys[e] = key;
        recs[e] = rec;
    }
}

struct BwdArgs {
    Tables t;
    const int32_t* rowptr; const Rec* recs; int64_t n_recs; int rows;
    float* out; int64_t ld_out; int out_h;          // part p of the output row starts at column p * out_h
    float* partial; int u0;                         // first unit (of VEC columns) of this launch's column block
    float divisor; int accumulate;
};

// Chunked segmented reduction (the scheme of k_seg_reduce, distmult_bwd.hip).  256 threads = (256 / LPE) records in flight
// x LPE lanes of VEC columns; per row of the chunk the lanes' sums are folded through LDS in a fixed order.
template <int M, int ROLE, int VEC, int LPE>
__global__ __launch_bounds__(256) void k_kge_reduce(BwdArgs a) {
    constexpr int S = 256 / LPE;
    constexpr int P = ROLE == kRelation ? (M == kComplEx ? 2 : 1) : Traits<M>::ent_parts;
    __shared__ float part[P][S][LPE * VEC];
    const int j = threadIdx.x % LPE, slot = threadIdx.x / LPE;
    const int lo = blockIdx.x * kChunkRecs;
    const int hi = (int)min((int64_t)lo + kChunkRecs, a.n_recs);
    const int unit = a.u0 + j;
    const bool col_ok = unit * VEC < a.t.h;                 // (h is a multiple of VEC)
    // the first row with a record at or behind `lo`: the last row that begins at or before it
    int r_first = 0;
    {
        int l = 0, h = a.rows;                              // largest row in [0, rows) with rowptr[row] <= lo, 0 if none
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (a.rowptr[mid] <= lo) l = mid + 1; else h = mid;
        }
        r_first = max(l - 1, 0);
    }
    for (int row = r_first; row < a.rows; ++row) {
        const int rb = a.rowptr[row], re = a.rowptr[row + 1];
        if (rb >= hi) break;                                // workgroup-uniform
        const int begin = max(lo, rb), end = min(hi, re);
        if (begin >= end) continue;
        float acc[P][VEC];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[p][v] = 0.f;
        if (col_ok) {
            for (int i = begin + slot; i < end; i += S) {
                const Rec rec = a.recs[i];
                if (rec.h == kSkip) continue;
                Col col[VEC];
                load_cols<M, VEC>(a.t, (int)rec.h, (int)rec.t, (int)rec.r, unit * VEC, col);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    float d0, d1;
                    dscore<M, ROLE>(col[v], a.divisor, d0, d1);
                    acc[0][v] += rec.g * d0;
                    if constexpr (P == 2) acc[1][v] += rec.g * d1;
                }
            }
        }
        __syncthreads();                                    // the previous row's fold is done with `part`
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int v = 0; v < VEC; ++v) part[p][slot][j * VEC + v] = acc[p][v];
        __syncthreads();
        // thread (p, column) folds the S slots in slot order
        for (int idx = threadIdx.x; idx < P * LPE * VEC; idx += 256) {
            const int p = idx / (LPE * VEC), c = idx % (LPE * VEC);
            const int column = a.u0 * VEC + c;
            if (column >= a.t.h) continue;
            float s = part[p][0][c];
            for (int k = 1; k < S; ++k) s += part[p][k][c];
            if (rb >= lo && re <= hi) {                     // the whole row is here: final
                float* o = a.out + (int64_t)row * a.ld_out + (int64_t)p * a.out_h + column;
                *o = a.accumulate ? *o + s : s;
            } else {                                        // shared with a neighbour chunk
                const int which = rb <= lo ? 0 : 1;
                a.partial[(size_t)blockIdx.x * kPartialPerChunk + (which * 2 + p) * 64 + c] = s;
            }
        }
    }
}

// Rows that straddle chunks: out[row, block] (+)= the chunks' partials in chunk order; rows without a record: zeros.
__global__ void k_kge_combine(const int32_t* __restrict__ rowptr, const float* __restrict__ partial, float* __restrict__ out,
                              int64_t ld_out, int out_h, int parts, int c0, int width, int accumulate) {
    const int row = blockIdx.x, c = threadIdx.x % 64, p = threadIdx.x / 64;
    if (c >= width || p >= parts) return;
    const int rb = rowptr[row], re = rowptr[row + 1];
    float* o = out + (int64_t)row * ld_out + (int64_t)p * out_h + c0 + c;
    if (rb >= re) {
        if (!accumulate) *o = 0.f;
        return;
    }
    const int cb = rb / kChunkRecs, ce = (re - 1) / kChunkRecs;
    if (cb == ce) return;                                   // inside one chunk: k_kge_reduce wrote the final value
    float s = 0.f;
    for (int b = cb; b <= ce; ++b) {
        const int which = rb <= b * kChunkRecs ? 0 : 1;
        s += partial[(size_t)b * kPartialPerChunk + (which * 2 + p) * 64 + c];
    }
    *o = accumulate ? *o + s : s;
}

struct WsLayout { size_t keys, keys_sorted, recs, recs_sorted, rowptr, partial, trig, sort_tmp, total; };

WsLayout ws_layout(int model, int64_t n, int64_t r, int64_t h, int64_t e) {
    WsLayout l;
    size_t sort_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const Rec*)nullptr,
                                    (Rec*)nullptr, (size_t)e, 0, 32, (hipStream_t)0);
    l.keys = 0;
    l.keys_sorted = l.keys + align_up(e * sizeof(uint32_t));
    l.recs = l.keys_sorted + align_up(e * sizeof(uint32_t));
    l.recs_sorted = l.recs + align_up(e * sizeof(Rec));
    l.rowptr = l.recs_sorted + align_up(e * sizeof(Rec));
    l.partial = l.rowptr + align_up((std::max(n, r) + 2) * sizeof(int32_t));
    l.trig = l.partial + align_up((size_t)gn::ceil_div(e, kChunkRecs) * kPartialPerChunk * sizeof(float));
    l.sort_tmp = l.trig + align_up(model == kRotatE ? (size_t)2 * r * h * sizeof(float) : 0);
    l.total = l.sort_tmp + align_up(sort_bytes);
    return l;
}

size_t trig_bytes(int model, int64_t r, int64_t h) { return model == kRotatE ? align_up((size_t)2 * r * h * sizeof(float)) : 0; }

// The relation operand as the kernels read it: the table itself, or (RotatE) cos / sin of its phases in `trig`.
gn_status relation_operand(int model, Tables& t, const float* rel, int64_t ld_rel, float divisor, float* trig, hipStream_t st) {
    t.rel = rel; t.ld_rel = ld_rel; t.rel_im = rel + t.h;
    if (model != kRotatE) return GN_OK;
    float* cos_t = trig;
    float* sin_t = trig + t.r * t.h;
    k_kge_trig<<<gn::stream_grid(t.r * t.h, 256), 256, 0, st>>>(rel, ld_rel, t.r, t.h, divisor, cos_t, sin_t);
    GN_LAUNCH_CHECK();
    t.rel = cos_t; t.rel_im = sin_t; t.ld_rel = t.h;
    return GN_OK;
}

bool vector_rows(const Tables& t) {
    return t.h % 4 == 0 && t.ld_ent % 4 == 0 && t.ld_rel % 4 == 0 && gn::aligned16(t.ent) && gn::aligned16(t.rel) &&
           gn::aligned16(t.rel_im);
}

gn_status check_shapes(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel, int64_t r,
                       int64_t h, int64_t e) {
    GN_REQUIRE(model >= kTransE && model <= kRotatE, "unknown model %d (0 TransE, 1 DistMult, 2 ComplEx, 3 RotatE)", model);
    GN_REQUIRE(n >= 0 && r >= 0 && h >= 0 && e >= 0, "negative size");
    if (n >= (1ll << 31) - 512 || r >= (1ll << 31) - 512 || h >= (1ll << 29) || e >= (1ll << 31) - kChunkRecs)   // (grids of 256 threads over rows + 1)
        return gn::fail(GN_ERR_UNSUPPORTED, "a table or the triple list is beyond the 32-bit record encoding");
    if (e == 0) return GN_OK;
    GN_REQUIRE(n > 0 && r > 0, "triples given but the entity or relation table is empty");
    GN_REQUIRE(ent && rel, "operand pointer is null");
    const int64_t de = (model == kComplEx || model == kRotatE) ? 2 * h : h, dr = model == kComplEx ? 2 * h : h;
    GN_REQUIRE(ld_ent >= de && ld_rel >= dr, "leading dimension smaller than the row length");
    return GN_OK;
}

template <int M>
void launch_forward(const FwdArgs& a, bool vec, int grid, hipStream_t st) {
    if (vec) k_kge_forward<M, 4><<<grid, 256, 0, st>>>(a); else k_kge_forward<M, 1><<<grid, 256, 0, st>>>(a);
}

template <int M, int ROLE>
void launch_reduce(const BwdArgs& a, bool vec, int lpe, unsigned chunks, hipStream_t st) {
    if (!vec) k_kge_reduce<M, ROLE, 1, 16><<<chunks, 256, 0, st>>>(a);
    else if (lpe == 8) k_kge_reduce<M, ROLE, 4, 8><<<chunks, 256, 0, st>>>(a);
    else k_kge_reduce<M, ROLE, 4, 16><<<chunks, 256, 0, st>>>(a);
}

template <int M>
void launch_reduce_role(int role, const BwdArgs& a, bool vec, int lpe, unsigned chunks, hipStream_t st) {
    if (role == kHead) launch_reduce<M, kHead>(a, vec, lpe, chunks, st);
    else if (role == kTail) launch_reduce<M, kTail>(a, vec, lpe, chunks, st);
    else launch_reduce<M, kRelation>(a, vec, lpe, chunks, st);
}

struct BwdCall {
    int model; Tables t;
    const int64_t* head; const int64_t* tail; const int64_t* et; int64_t e;
    const float* grad_out; const float* raw; float divisor;
    float* d_ent; int64_t ld_dent; float* d_rel; int64_t ld_drel;
    bool types_sorted, vec; hipStream_t st;
};

// one pass: records keyed by `role`, sorted (or left in list order), reduced per row
gn_status pass(int role, const BwdCall& c, char* ws, const WsLayout& l) {
    uint32_t* keys = reinterpret_cast<uint32_t*>(ws + l.keys);
    uint32_t* keys_sorted = reinterpret_cast<uint32_t*>(ws + l.keys_sorted);
    Rec* recs = reinterpret_cast<Rec*>(ws + l.recs);
    Rec* recs_sorted = reinterpret_cast<Rec*>(ws + l.recs_sorted);
    int32_t* rowptr = reinterpret_cast<int32_t*>(ws + l.rowptr);
    float* partial = reinterpret_cast<float*>(ws + l.partial);
    size_t sort_bytes = l.total - l.sort_tmp;
    hipStream_t st = c.st;
    const int64_t e = c.e;
    const int64_t rows = role == kRelation ? c.t.r : c.t.n;
    const bool in_place = role == kRelation && c.types_sorted;
    k_kge_recs<<<gn::stream_grid(e, 256), 256, 0, st>>>(role, c.head, c.tail, c.et, c.grad_out, c.raw, e, c.t.n, c.t.r, (uint32_t)rows,
                                                         in_place ? nullptr : keys, recs);
    GN_LAUNCH_CHECK();
    const int off_grid = (int)gn::ceil_div(rows + 1, 256);
    if (in_place) {
        gn::k_key_offsets<int64_t><<<off_grid, 256, 0, st>>>(c.et, e, (int)rows, rowptr);
        GN_LAUNCH_CHECK();
    } else {
        GN_HIP(rocprim::radix_sort_pairs(ws + l.sort_tmp, sort_bytes, keys, keys_sorted, recs, recs_sorted, (size_t)e, 0,
                                         gn::bits_for(rows + 1), st));
        gn::k_key_offsets<uint32_t><<<off_grid, 256, 0, st>>>(keys_sorted, e, (int)rows, rowptr);
        GN_LAUNCH_CHECK();
    }
    BwdArgs a;
    a.t = c.t; a.rowptr = rowptr; a.recs = in_place ? recs : recs_sorted; a.n_recs = e; a.rows = (int)rows;
    a.out = role == kRelation ? c.d_rel : c.d_ent;
    a.ld_out = role == kRelation ? c.ld_drel : c.ld_dent;
    a.out_h = c.t.h; a.partial = partial; a.divisor = c.divisor;
    a.accumulate = role == kTail;                           // d_ent = head pass, then + tail pass
    const int parts = role == kRelation ? (c.model == kComplEx ? 2 : 1) : ((c.model == kComplEx || c.model == kRotatE) ? 2 : 1);
    const int vecw = c.vec ? 4 : 1;
    const int units = c.t.h / vecw;
    const int lpe = (c.vec && units <= 8) ? 8 : 16;
    const unsigned chunks = (unsigned)gn::ceil_div(e, kChunkRecs);
    for (int u0 = 0; u0 < units; u0 += lpe) {
        a.u0 = u0;
        switch (c.model) {
            case kTransE: launch_reduce_role<kTransE>(role, a, c.vec, lpe, chunks, st); break;
            case kDistMult: launch_reduce_role<kDistMult>(role, a, c.vec, lpe, chunks, st); break;
            case kComplEx: launch_reduce_role<kComplEx>(role, a, c.vec, lpe, chunks, st); break;
            default: launch_reduce_role<kRotatE>(role, a, c.vec, lpe, chunks, st); break;
        }
        GN_LAUNCH_CHECK();
        const int width = std::min(lpe * vecw, c.t.h - u0 * vecw);
        k_kge_combine<<<(unsigned)rows, 64 * parts, 0, st>>>(rowptr, partial, a.out, a.ld_out, a.out_h, parts, u0 * vecw, width, a.accumulate);
        GN_LAUNCH_CHECK();
    }
    return GN_OK;
}

}  // namespace

extern "C" size_t gn_kge_forward_workspace_bytes(int model, int64_t r, int64_t h) {
    if (r < 0 || h < 0) return 0;
    return trig_bytes(model, r, h);
}

extern "C" gn_status gn_kge_forward_f32(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                        int64_t r, int64_t h, const int64_t* head, const int64_t* tail, const int64_t* et,
                                        int64_t e, float gamma, float phase_divisor, int log_sigmoid_out, float* out, float* raw_out,
                                        int32_t* err, void* workspace, size_t workspace_bytes, void* stream) {
    GN_OK_OR_RETURN(check_shapes(model, ent, ld_ent, n, rel, ld_rel, r, h, e));
    if (e == 0) return GN_OK;
    GN_REQUIRE(head && tail && et && out, "operand pointer is null");
    hipStream_t st = gn::as_stream(stream);
    FwdArgs a;
    a.t.ent = ent; a.t.ld_ent = ld_ent; a.t.n = n; a.t.r = r; a.t.h = (int)h;
    if (model == kRotatE) {
        GN_REQUIRE(phase_divisor != 0.f, "RotatE: the phase divisor is zero");
        GN_REQUIRE(workspace && workspace_bytes >= trig_bytes(model, r, h) && gn::aligned16(workspace),
                   "workspace too small: need %zu bytes (16-byte aligned)", trig_bytes(model, r, h));
    }
    GN_OK_OR_RETURN(relation_operand(model, a.t, rel, ld_rel, phase_divisor, static_cast<float*>(workspace), st));
    a.head = head; a.tail = tail; a.et = et; a.e = e; a.gamma = gamma; a.log_sigmoid = log_sigmoid_out;
    a.out = out; a.raw = raw_out; a.err = err;
    const bool vec = vector_rows(a.t);
    const int64_t units = vec ? h / 4 : h;
    int group = 1;
    while (group < 16 && group < units) group <<= 1;       // H / 4 lanes per triple: 8 at the driver's H = 32
    a.group = group;
    const int grid = gn::stream_grid(gn::ceil_div(e, 64) * 64, 256);
    switch (model) {
        case kTransE: launch_forward<kTransE>(a, vec, grid, st); break;
        case kDistMult: launch_forward<kDistMult>(a, vec, grid, st); break;
        case kComplEx: launch_forward<kComplEx>(a, vec, grid, st); break;
        default: launch_forward<kRotatE>(a, vec, grid, st); break;
    }
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" size_t gn_kge_backward_workspace_bytes(int model, int64_t n, int64_t r, int64_t h, int64_t e) {
    if (n < 0 || r < 0 || h < 0 || e <= 0) return 0;
    return ws_layout(model, n, r, h, e).total;
}

extern "C" gn_status gn_kge_backward_f32(int model, const float* ent, int64_t ld_ent, int64_t n, const float* rel, int64_t ld_rel,
                                         int64_t r, int64_t h, const int64_t* head, const int64_t* tail, const int64_t* et,
                                         int64_t e, float phase_divisor, const float* grad_out, const float* raw_scores,
                                         float* d_ent, int64_t ld_dent, float* d_rel, int64_t ld_drel, int flags,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    GN_OK_OR_RETURN(check_shapes(model, ent, ld_ent, n, rel, ld_rel, r, h, e));
    const int64_t de = (model == kComplEx || model == kRotatE) ? 2 * h : h, dr = model == kComplEx ? 2 * h : h;
    GN_REQUIRE((n == 0 || h == 0 || d_ent) && (r == 0 || h == 0 || d_rel), "gradient pointer is null");
    GN_REQUIRE(ld_dent >= de && ld_drel >= dr, "leading dimension of a gradient smaller than the row length");
    hipStream_t st = gn::as_stream(stream);
    if (e == 0 || h == 0) {                                 // gradients of an empty sum
        if (n > 0 && de > 0) GN_HIP(hipMemset2DAsync(d_ent, ld_dent * sizeof(float), 0, de * sizeof(float), n, st));
        if (r > 0 && dr > 0) GN_HIP(hipMemset2DAsync(d_rel, ld_drel * sizeof(float), 0, dr * sizeof(float), r, st));
        return GN_OK;
    }
    GN_REQUIRE(head && tail && et && grad_out, "operand pointer is null");
    const WsLayout l = ws_layout(model, n, r, h, e);
    GN_REQUIRE(workspace && workspace_bytes >= l.total, "workspace too small: need %zu bytes", l.total);
    GN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    char* ws = static_cast<char*>(workspace);
    BwdCall c;
    c.model = model;
    c.t.ent = ent; c.t.ld_ent = ld_ent; c.t.n = n; c.t.r = r; c.t.h = (int)h;
    if (model == kRotatE) GN_REQUIRE(phase_divisor != 0.f, "RotatE: the phase divisor is zero");
    GN_OK_OR_RETURN(relation_operand(model, c.t, rel, ld_rel, phase_divisor, reinterpret_cast<float*>(ws + l.trig), st));
    c.head = head; c.tail = tail; c.et = et; c.e = e; c.grad_out = grad_out; c.raw = raw_scores;
    c.divisor = model == kRotatE ? phase_divisor : 1.0f;
    c.d_ent = d_ent; c.ld_dent = ld_dent; c.d_rel = d_rel; c.ld_drel = ld_drel;
    c.types_sorted = (flags & GN_DM_TYPES_SORTED) != 0;
    c.vec = vector_rows(c.t);                              // (the gradients are stored a float at a time: any ld)
    c.st = st;
    GN_OK_OR_RETURN(pass(kHead, c, ws, l));
    GN_OK_OR_RETURN(pass(kTail, c, ws, l));
    return pass(kRelation, c, ws, l);
}
