// Layouts of the DistMult decoder on a static list (distmult_plan.hip): pairing of mirrored triples, the row-class
// encoding and the column-phase batches.  No HIP.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#endif

#include "host_parallel.hpp"
#include "layout_util.hpp"

namespace gn_layout {

constexpr uint32_t kNoMirror = 0xffffffffu;
constexpr int kClsDCache = 64;        // relation rows of D a workgroup of k_distmult_class keeps in LDS
constexpr int kClsSlack = 64;         // readable batches behind the last one (the kernel's prefetches run ahead unclamped)
constexpr int kClsMaxWalks = 8;       // position sub-ranges an XCD's workgroups walk one after the other (k_distmult_class)
constexpr int64_t kClsWindowBytes = 1 << 20;   // scores of one sub-range: what an XCD's 4 MB L2 holds half-written next to the streams

// ---- DistMult decoder on a static list (distmult_plan.hip) -------------------------------------------------------------
// Triples with the same unordered node pair and relation have the same score (the reference's positive list holds every
// edge in both directions, utils.py:132-138): they are paired up, the first of a pair is scored and writes both positions.
// mirror_of[e] = the later copy that takes e's score (-1: none); covered[e] = e is such a later copy.
// (the serial form: any order of relations)
template <typename V>
inline void pair_mirrors_serial(const V& hu, const V& hv, const V& hr, int node_bits,
                                gn::RawVec<int64_t>& mirror_of, gn::RawVec<char>& covered) {
    const int64_t E = (int64_t)hu.size();
    mirror_of.assign((size_t)E, -1);
    covered.assign((size_t)E, 0);
    PairingTable table;
    table.open((size_t)E);
    for (int64_t e = 0; e < E; ++e) {
        const uint64_t lo = (uint64_t)std::min(hu[e], hv[e]), hi = (uint64_t)std::max(hu[e], hv[e]);
        const int64_t first = table.pair_up(((uint64_t)hr[e] << (2 * node_bits)) | (lo << node_bits) | hi, e);
        if (first >= 0) { mirror_of[first] = e; covered[e] = 1; }
    }
}

// Round 6: a type-sorted list (the reference's layout, utils.py:168-198) pairs up inside every relation on its own - the
// relations are dealt to the builder threads in contiguous runs of about equal edge counts, each thread with one small
// open-addressing table that it wipes by the slots it touched.  Same pairs as the serial pass (within a relation the
// edges are visited in list order).  2 M edges: 92 -> 14 ms on eight threads.
// (V: a vector of int64_t - the reference's index type - or of a narrower unsigned type the caller narrowed the validated ids to on the device)
template <typename V>
inline void pair_mirrors(const V& hu, const V& hv, const V& hr, int node_bits,
                         gn::RawVec<int64_t>& mirror_of, gn::RawVec<char>& covered) {
    const int64_t E = (int64_t)hu.size();
    GN_LAP(nullptr);
    // sorted by relation?  and the first edge of every run of equal relation ids: 64 slices of the list on the builder threads
    constexpr int kSlices = 64;
    std::vector<std::vector<int64_t>> slice_starts(kSlices);
    std::vector<char> slice_unsorted(kSlices, 0);
    gn::parallel_for(kSlices, 1, [&](int64_t s0, int64_t s1) {
        for (int64_t sl = s0; sl < s1; ++sl)
            for (int64_t e = E * sl / kSlices; e < E * (sl + 1) / kSlices; ++e)
                if (e == 0 || hr[e] != hr[e - 1]) {
                    slice_starts[(size_t)sl].push_back(e);
                    if (e > 0 && hr[e - 1] > hr[e]) slice_unsorted[(size_t)sl] = 1;
                }
    });
    bool sorted = true;
    for (char c : slice_unsorted) sorted = sorted && !c;
    if (!sorted || E < (1 << 16)) { pair_mirrors_serial(hu, hv, hr, node_bits, mirror_of, covered); return; }
    mirror_of.resize((size_t)E);                                 // (every task below wipes its own range first)
    covered.resize((size_t)E);
    std::vector<int64_t> rel_start;                              // first edge of every run of equal relation ids, then E
    for (const auto& v : slice_starts) rel_start.insert(rel_start.end(), v.begin(), v.end());
    rel_start.push_back(E);
    const int64_t runs = (int64_t)rel_start.size() - 1;
    // tasks: contiguous runs of relations of ~E / 64 edges each (a relation is never cut)
    const std::vector<int64_t> task_first =
        equal_weight_tasks(runs, [&](int64_t r) { return rel_start[r + 1] - rel_start[r]; }, std::max<int64_t>(1, E / 64));
    GN_LAP("mirrors: runs + tasks");
    gn::parallel_for((int64_t)task_first.size() - 1, 1, [&](int64_t t0, int64_t t1) {
        PairingTable table;
        for (int64_t t = t0; t < t1; ++t) {
            std::fill(mirror_of.begin() + rel_start[task_first[t]], mirror_of.begin() + rel_start[task_first[t + 1]], (int64_t)-1);
            std::fill(covered.begin() + rel_start[task_first[t]], covered.begin() + rel_start[task_first[t + 1]], (char)0);
            for (int64_t r = task_first[t]; r < task_first[t + 1]; ++r) {
                const int64_t lo_e = rel_start[r], hi_e = rel_start[r + 1];
                table.open((size_t)(hi_e - lo_e));
                for (int64_t e = lo_e; e < hi_e; ++e) {
                    const uint64_t lo = (uint64_t)std::min(hu[e], hv[e]), hi = (uint64_t)std::max(hu[e], hv[e]);
                    const int64_t first = table.pair_up((lo << node_bits) | hi, e);
                    if (first >= 0) { mirror_of[first] = e; covered[e] = 1; }
                }
                table.wipe();
            }
        }
    });
    GN_LAP("mirrors: tables (parallel)");
}

// The edges the decoder scores (the others are written as their pair's mirror), in list order.
inline gn::RawVec<int64_t> scored_edges(const gn::RawVec<char>& covered) {
    constexpr int kSlices = 64;
    const int64_t E = (int64_t)covered.size();
    std::vector<int64_t> first(kSlices + 1, 0);
    gn::parallel_for(kSlices, 1, [&](int64_t s0, int64_t s1) {
        for (int64_t sl = s0; sl < s1; ++sl) {
            int64_t c = 0;
            for (int64_t e = E * sl / kSlices; e < E * (sl + 1) / kSlices; ++e) c += !covered[(size_t)e];
            first[(size_t)sl + 1] = c;
        }
    });
    for (int sl = 0; sl < kSlices; ++sl) first[(size_t)sl + 1] += first[(size_t)sl];
    gn::RawVec<int64_t> scored((size_t)first[kSlices]);
    gn::parallel_for(kSlices, 1, [&](int64_t s0, int64_t s1) {
        for (int64_t sl = s0; sl < s1; ++sl) {
            int64_t at = first[(size_t)sl];
            for (int64_t e = E * sl / kSlices; e < E * (sl + 1) / kSlices; ++e)
                if (!covered[(size_t)e]) scored[(size_t)at++] = e;
        }
    });
    return scored;
}

// Deals the (up to) 64 edges of a batch to its slots.  Lane l of the wave holds slot l; wave step S works on the
// slots 4 q + S of the 16 quads q, and ds_read_b128 serves the quads in four access groups.  A cell = (step,
// access group) = four slots that hit the LDS together: its edges should have four different u % 4 and four
// different v % 4 (the bank slot of a row is (row * odd stride) % 4).
inline void deal_batch(const int64_t* u, const int64_t* v, int count, int* slot_of_edge) {
    static const int kPerms[24][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {0, 3, 2, 1},
                                      {1, 0, 2, 3}, {1, 0, 3, 2}, {1, 2, 0, 3}, {1, 2, 3, 0}, {1, 3, 0, 2}, {1, 3, 2, 0},
                                      {2, 0, 1, 3}, {2, 0, 3, 1}, {2, 1, 0, 3}, {2, 1, 3, 0}, {2, 3, 0, 1}, {2, 3, 1, 0},
                                      {3, 0, 1, 2}, {3, 0, 2, 1}, {3, 1, 0, 2}, {3, 1, 2, 0}, {3, 2, 0, 1}, {3, 2, 1, 0}};
    SmallStack bucket[4][4];                         // edges by (u % 4, v % 4)
    for (int e = 0; e < count; ++e) bucket[u[e] & 3][v[e] & 3].push_back(e);
    int left = count;
    for (int cell = 0; cell < 16; ++cell) {
        const int S = cell & 3, g = cell >> 2;
        int chosen[4] = {-1, -1, -1, -1};
        if (left > 0) {
            // a full cell: one edge from each (c, sigma(c)) for the permutation whose scarcest bucket is fullest
            int best = -1, best_min = 0;
            for (int p = 0; p < 24; ++p) {
                int mn = 1 << 30;
                for (int c = 0; c < 4; ++c) mn = std::min(mn, (int)bucket[c][kPerms[p][c]].size());
                if (mn > best_min) { best_min = mn; best = p; }
            }
            if (best >= 0) {
                for (int c = 0; c < 4; ++c) { auto& bk = bucket[c][kPerms[best][c]]; chosen[c] = bk.back(); bk.pop_back(); }
            } else {
                // no conflict-free quadruple left: take edges one by one, preferring unused u and v classes
                unsigned used_u = 0, used_v = 0;
                for (int k = 0; k < 4; ++k) {
                    int bc = -1, bd = -1, bscore = -1;
                    for (int c = 0; c < 4; ++c)
                        for (int dd = 0; dd < 4; ++dd) {
                            if (bucket[c][dd].empty()) continue;
                            const int score = 2 * (!((used_u >> c) & 1) + !((used_v >> dd) & 1)) * 64 + (int)bucket[c][dd].size();
                            if (score > bscore) { bscore = score; bc = c; bd = dd; }
                        }
                    if (bc < 0) break;
                    chosen[k] = bucket[bc][bd].back();
                    bucket[bc][bd].pop_back();
                    used_u |= 1u << bc; used_v |= 1u << bd;
                }
            }
        }
        for (int k = 0; k < 4; ++k)
            if (chosen[k] >= 0) { slot_of_edge[chosen[k]] = 4 * kGroupQuads[g][k] + S; --left; }
    }
}

// Cells of four pairs for one run of pairs that share class and relation: the four pairs of a cell are read by one
// 16-lane access group of ds_read_b128, so they should have four different (local row of u) % 4 and four different
// (local row of v) % 4 - the 64-byte bank slot of a row is (row * odd stride) % 4.  Cells fill whole steps first
// (step = cell / 4): a run is padded to a multiple of 16 pairs, not 64.  order[cell * 4 + k] = pair of the run, or -1.
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define GN_DEAL_SSSE3 1
// The permutation search of deal_run in six byte shuffles: sz = the sixteen stack sizes (bytes, index 4 c + d); returns the first
// of the 24 permutations (kPerms order) whose scarcest bucket is fullest, -1 when every permutation has an empty bucket.
__attribute__((target("ssse3"))) inline int best_permutation_ssse3(const uint8_t* sz, const uint8_t (*idx)[16]) {
    const __m128i s = _mm_loadu_si128(reinterpret_cast<const __m128i*>(sz));   // (sz: sixteen bytes the caller keeps 16-byte stores to)
    const __m128i lo = _mm_min_epu8(_mm_min_epu8(_mm_shuffle_epi8(s, _mm_loadu_si128(reinterpret_cast<const __m128i*>(idx[0]))),
                                                 _mm_shuffle_epi8(s, _mm_loadu_si128(reinterpret_cast<const __m128i*>(idx[1])))),
                                    _mm_min_epu8(_mm_shuffle_epi8(s, _mm_loadu_si128(reinterpret_cast<const __m128i*>(idx[2]))),
                                                 _mm_shuffle_epi8(s, _mm_loadu_si128(reinterpret_cast<const __m128i*>(idx[3])))));
    const __m128i hi = _mm_min_epu8(_mm_min_epu8(_mm_shuffle_epi8(s, _mm_loadu_si128(reinterpret_cast<const __m128i*>(idx[4]))),
                                                 _mm_shuffle_epi8(s, _mm_loadu_si128(reinterpret_cast<const __m128i*>(idx[5])))),
                                    _mm_min_epu8(_mm_shuffle_epi8(s, _mm_loadu_si128(reinterpret_cast<const __m128i*>(idx[6]))),
                                                 _mm_shuffle_epi8(s, _mm_loadu_si128(reinterpret_cast<const __m128i*>(idx[7])))));
    __m128i m = _mm_max_epu8(lo, hi);
    m = _mm_max_epu8(m, _mm_srli_si128(m, 8));
    m = _mm_max_epu8(m, _mm_srli_si128(m, 4));
    m = _mm_max_epu8(m, _mm_srli_si128(m, 2));
    m = _mm_max_epu8(m, _mm_srli_si128(m, 1));
    const int best_min = _mm_cvtsi128_si32(m) & 0xff;
    if (best_min == 0) return -1;
    const __m128i all = _mm_set1_epi8((char)best_min);
    const int first_lo = _mm_movemask_epi8(_mm_cmpeq_epi8(lo, all));
    if (first_lo) return __builtin_ctz((unsigned)first_lo);
    return 16 + __builtin_ctz((unsigned)_mm_movemask_epi8(_mm_cmpeq_epi8(hi, all)));
}
__attribute__((target("ssse3"))) inline void take_permutation_ssse3(uint8_t* szv, const uint8_t* take) {
    _mm_store_si128(reinterpret_cast<__m128i*>(szv), _mm_sub_epi8(_mm_load_si128(reinterpret_cast<const __m128i*>(szv)),
                                                                 _mm_load_si128(reinterpret_cast<const __m128i*>(take))));
}
#endif

inline void deal_run(const int* lu, const int* lv, int count, std::vector<int>& order) {
    static const int kPerms[24][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {0, 3, 2, 1},
                                      {1, 0, 2, 3}, {1, 0, 3, 2}, {1, 2, 0, 3}, {1, 2, 3, 0}, {1, 3, 0, 2}, {1, 3, 2, 0},
                                      {2, 0, 1, 3}, {2, 0, 3, 1}, {2, 1, 0, 3}, {2, 1, 3, 0}, {2, 3, 0, 1}, {2, 3, 1, 0},
                                      {3, 0, 1, 2}, {3, 0, 2, 1}, {3, 1, 0, 2}, {3, 1, 2, 0}, {3, 2, 0, 1}, {3, 2, 1, 0}};
#ifdef GN_DEAL_SSSE3
    // shuffle controls: idx[c] = the bucket 4 c + sigma_p(c) of permutations p = 0..15, idx[4 + c] of p = 16..23 (then 0x80: a zero)
    struct ShuffleTable {
        uint8_t idx[8][16];
        alignas(16) uint8_t take[24][16];             // 1 at the four buckets of a permutation
        ShuffleTable() {
            for (int c = 0; c < 4; ++c)
                for (int p = 0; p < 32; ++p) idx[(p >> 4) * 4 + c][p & 15] = p < 24 ? (uint8_t)(4 * c + kPerms[p][c]) : (uint8_t)0x80;
            for (int p = 0; p < 24; ++p) {
                for (int b = 0; b < 16; ++b) take[p][b] = 0;
                for (int c = 0; c < 4; ++c) take[p][4 * c + kPerms[p][c]] = 1;
            }
        }
    };
    static const ShuffleTable table;
    static const bool use_ssse3 = __builtin_cpu_supports("ssse3");
#endif
    const int steps = (count + 15) / 16;
    order.assign((size_t)steps * 16, -1);
    // sixteen stacks by (lu % 4, lv % 4), their sizes side by side in sixteen bytes: the search below reads nothing else
    int stack[16][64];
    uint8_t sz[16] = {0};
    for (int e = count - 1; e >= 0; --e) { const int b = (lu[e] & 3) * 4 + (lv[e] & 3); stack[b][sz[b]++] = e; }   // (popped from the back: list order)
#ifdef GN_DEAL_SSSE3
    alignas(16) uint8_t szv[16];                      // the sizes again, only ever stored whole (a vector load behind byte stores stalls)
    std::memcpy(szv, sz, 16);
#endif
    int left = count;
    for (int cell = 0; cell < steps * 4 && left > 0; ++cell) {
        int chosen[4] = {-1, -1, -1, -1};
        // a full cell: one pair from each (c, sigma(c)) for the permutation whose scarcest bucket is fullest (the first of equals)
        int best = -1;
#ifdef GN_DEAL_SSSE3
        if (use_ssse3) {
            best = best_permutation_ssse3(szv, table.idx);
        } else
#endif
        {
            int best_min = 0;
            for (int p = 0; p < 24; ++p) {
                const int mn = std::min(std::min((int)sz[kPerms[p][0]], (int)sz[4 + kPerms[p][1]]), std::min((int)sz[8 + kPerms[p][2]], (int)sz[12 + kPerms[p][3]]));
                if (mn > best_min) { best_min = mn; best = p; }
            }
        }
        if (best >= 0) {
            for (int c = 0; c < 4; ++c) { const int b = c * 4 + kPerms[best][c]; chosen[c] = stack[b][--sz[b]]; }
#ifdef GN_DEAL_SSSE3
            if (use_ssse3) take_permutation_ssse3(szv, table.take[best]);
#endif
        } else {
            // no conflict-free quadruple left: pairs one by one, preferring unused u and v classes
            unsigned used_u = 0, used_v = 0;
            for (int k = 0; k < 4; ++k) {
                int bb = -1, bscore = -1;
                for (int b = 0; b < 16; ++b) {
                    if (sz[b] == 0) continue;
                    const int score = 2 * (!((used_u >> (b >> 2)) & 1) + !((used_v >> (b & 3)) & 1)) * 64 + (int)sz[b];
                    if (score > bscore) { bscore = score; bb = b; }
                }
                if (bb < 0) break;
                chosen[k] = stack[bb][--sz[bb]];
                used_u |= 1u << (bb >> 2); used_v |= 1u << (bb & 3);
            }
#ifdef GN_DEAL_SSSE3
            std::memcpy(szv, sz, 16);
#endif
        }
        for (int k = 0; k < 4; ++k)
            if (chosen[k] >= 0) { order[(size_t)cell * 4 + k] = chosen[k]; --left; }
    }
}

// The row-class encoding of the scored pairs (see k_distmult_class in distmult_plan.hip).  ok = false when a class's
// rows do not fit the LDS with `features` columns, or a workgroup's batches name more relations than its D cache holds.
struct ClassLayout {
    bool ok = false;
    int groups = 0;
    int walks = 1;                      // batch ranges per workgroup (descriptor: 4 + 4 walks ints)
    int64_t batches = 0;
    gn::RawVec<uint32_t> packed, own, mirror;
    std::vector<uint32_t> rel32;
    std::vector<int32_t> wg;
    // The same rows once per CLASS (a plan has one or three), and every workgroup's class: what a launch of up to 256
    // workgroups hands over with the kernel arguments, so that the kernel requests its rows without waiting for wg[]
    int32_t cls_rows[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    std::vector<uint8_t> wg_cls;        // [groups]
};

// How build_class_layout cuts the node table and the list.  The table: one block, or three of which a class holds two (its
// own and the next).  The list: `parts` position ranges (one per XCD) of `walks` sub-ranges each; a GROUP = (part, class).
// The passes over the pairs run on the builder threads in FIXED chunks (2^15 pairs, or a 64th of the list) - what a chunk
// computes does not depend on the thread count - or one position part per task.
struct ClassShape {
    int64_t n = 0, blk = 0;
    int nblocks = 1, nclasses = 1;
    int parts = 1, walks = 1, nparts = 1, ngroups = 1;           // part p = XCD (p / walks), walk (p % walks)
    int64_t chunk_pairs = 0, nchunks = 0;                        // (at most 64 chunks: their histograms stay small)
    int64_t bstart(int b) const { return std::min<int64_t>(n, (int64_t)b * blk); }
    int64_t bsize(int b) const { return bstart(b + 1) - bstart(b); }
    // local row of `node` (of block b) in class k's table
    int local_row(int64_t node, int b, int k) const { return (int)(b == k ? node - bstart(k) : bsize(k) + node - bstart((k + 1) % 3)); }
    int group_of(int x, int walk, int c) const { return (x * walks + walk) * nclasses + c; }
};

// Position parts.  A 64-byte line of the score vector holds sixteen consecutive edges of one relation - pairs of all
// three classes - so three workgroups write it, a third each.  The list is cut into eight position ranges, one per
// XCD (workgroup b runs on XCD b % 8), and inside a range each class gets its share of that XCD's compute units: the
// three writers of a line share an L2, which holds the range's whole share of the scores.
// When an XCD's share of the score vector exceeds what its L2 keeps half-written (pose2-syn: 4.2 MB of 33.5: 97 MB were
// written for them, the lines leaving L2 a third at a time), the XCD's range is cut into `walks` sub-ranges that its
// workgroups walk one after the other: the live window is one sub-range.
// false: the row-class kernel does not take a list of this shape.
inline bool class_shape(int64_t n, int64_t features, int64_t S, int64_t E, int cus, int64_t window_bytes, ClassShape& sh) {
    if (features < 16 || features % 16 != 0 || features > 128 || S < 1 || n < 1) return false;
    const int J = (int)(features / 16), str4 = (J & 1) ? 4 * J : 4 * J + 4;
    const int64_t rows_fit = ((int64_t)160 * 1024 - (int64_t)kClsDCache * 4 * J * 16) / ((int64_t)str4 * 16);
    sh.n = n; sh.blk = n;
    if (n > rows_fit) {
        sh.blk = gn::ceil_div(n, 3);
        if (2 * sh.blk > rows_fit) return false;
        sh.nblocks = 3;
    }
    if (n > 65535) return false;
    sh.nclasses = sh.nblocks == 1 ? 1 : 3;
    sh.parts = (cus % 8 == 0 && cus >= 24 && S >= (int64_t)64 * 4 * cus) ? 8 : 1;
    const int64_t list_bytes = E * 4;
    sh.walks = sh.parts == 8 ? (int)std::max<int64_t>(1, std::min<int64_t>(kClsMaxWalks, gn::ceil_div(list_bytes / 8, window_bytes))) : 1;
    sh.nparts = sh.parts * sh.walks;
    sh.ngroups = sh.nparts * sh.nclasses;
    sh.chunk_pairs = std::max<int64_t>(1 << 15, gn::ceil_div(S, 64));
    sh.nchunks = gn::ceil_div(S, sh.chunk_pairs);
    return true;
}

// The scored pairs' endpoints, relation and block ids as compact arrays in list order (round 6): every pass below walks
// THESE (8 bytes per pair) instead of chasing scored[] into four int64 arrays of the whole list (64 MB at pose0-syn: the
// builder was bound by cache misses, 120 ms on eight threads).
struct ScoredPairs {
    gn::RawVec<uint16_t> su, sv, sr;
    gn::RawVec<uint8_t> sbu, sbv;
    gn::RawVec<uint32_t> sm;                                     // the pair's mirror position (kNoMirror: none)
    int64_t n_rel = 0;                                           // relations: the largest id + 1
    int64_t size() const { return (int64_t)su.size(); }
};

template <typename V>
inline ScoredPairs compact_scored_pairs(const V& hu, const V& hv, const V& hr, const gn::RawVec<int64_t>& scored,
                                        const gn::RawVec<int64_t>& mirror_of, const ClassShape& sh) {
    const int64_t S = (int64_t)scored.size();
    ScoredPairs P;
    P.su.resize((size_t)S); P.sv.resize((size_t)S); P.sr.resize((size_t)S);
    P.sbu.resize((size_t)S); P.sbv.resize((size_t)S);
    P.sm.resize((size_t)S);
    std::vector<int64_t> chunk_max_rel((size_t)sh.nchunks, 0);
    gn::parallel_for(sh.nchunks, 1, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
            int64_t mx = 0;
            for (int64_t i = c * sh.chunk_pairs; i < std::min(S, (c + 1) * sh.chunk_pairs); ++i) {
                const int64_t e = scored[(size_t)i];
                P.sm[(size_t)i] = mirror_of[(size_t)e] >= 0 ? (uint32_t)mirror_of[(size_t)e] : kNoMirror;
                P.su[(size_t)i] = (uint16_t)hu[(size_t)e]; P.sv[(size_t)i] = (uint16_t)hv[(size_t)e]; P.sr[(size_t)i] = (uint16_t)hr[(size_t)e];
                P.sbu[(size_t)i] = (uint8_t)(hu[(size_t)e] / sh.blk); P.sbv[(size_t)i] = (uint8_t)(hv[(size_t)e] / sh.blk);
                mx = std::max<int64_t>(mx, (int64_t)P.sr[(size_t)i] + 1);
            }
            chunk_max_rel[(size_t)c] = mx;
        }
    });
    for (int64_t c = 0; c < sh.nchunks; ++c) P.n_rel = std::max(P.n_rel, chunk_max_rel[(size_t)c]);
    return P;
}

// The position parts are cut by BATCHES, not by pairs: a relation's pairs of a (part, class) are a run padded to
// steps of sixteen slots - about eight slots per run and class - so a range of many small relations (the tail of the
// type-sorted list) has more batches per pair than the head's few large ones (pose0-syn: 2,083 against 1,954 with
// equal pair counts, 65 batches per workgroup against 61).  Every pair weighs 1 + 24 / (its relation's pairs).
// (Walks of equal weight: cutting them in whole wave trips - 17 trips of sixteen batches per workgroup at pose2-syn instead
// of 5 x 4 - changed nothing, 47.4 us either way: the loop follows a compute unit's batches, not its waves' trips.)
// Returns part_first: part p = pairs [part_first[p], part_first[p + 1]) (list order: monotone).
inline std::vector<int64_t> position_parts(const ScoredPairs& P, const ClassShape& sh) {
    const int64_t S = P.size(), n_rel = P.n_rel, nchunks = sh.nchunks, kChunkPairs = sh.chunk_pairs;
    const int nparts = sh.nparts;
    const gn::RawVec<uint16_t>& sr = P.sr;
    gn::RawVec<int32_t> part_of((size_t)S);
    std::vector<int64_t> part_first((size_t)nparts + 1, S);
    // a relation's pair count: per-chunk histograms, added up
    std::vector<int32_t> hist((size_t)nchunks * (size_t)n_rel, 0);
    gn::parallel_for(nchunks, 1, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
            int32_t* h = hist.data() + (size_t)c * (size_t)n_rel;
            for (int64_t i = c * kChunkPairs; i < std::min(S, (c + 1) * kChunkPairs); ++i) h[sr[(size_t)i]]++;
        }
    });
    std::vector<int64_t> rel_cnt((size_t)n_rel, 0);
    for (int64_t c = 0; c < nchunks; ++c)
        for (int64_t r = 0; r < n_rel; ++r) rel_cnt[(size_t)r] += hist[(size_t)c * (size_t)n_rel + (size_t)r];
    double total_w = 0.0;
    std::vector<double> rel_w((size_t)n_rel, 0.0);
    for (int64_t r = 0; r < n_rel; ++r) {
        total_w += rel_cnt[(size_t)r] > 0 ? (double)rel_cnt[(size_t)r] + 24.0 : 0.0;
        rel_w[(size_t)r] = rel_cnt[(size_t)r] > 0 ? 1.0 + 24.0 / (double)rel_cnt[(size_t)r] : 0.0;
    }
    // the weight before every chunk (from its histogram), then the chunks on their own
    std::vector<double> chunk_cum((size_t)nchunks + 1, 0.0);
    for (int64_t c = 0; c < nchunks; ++c) {
        double w = 0.0;
        for (int64_t r = 0; r < n_rel; ++r) w += (double)hist[(size_t)c * (size_t)n_rel + (size_t)r] * rel_w[(size_t)r];
        chunk_cum[(size_t)c + 1] = chunk_cum[(size_t)c] + w;
    }
    std::vector<int32_t> chunk_last((size_t)nchunks, 0);
    gn::parallel_for(nchunks, 1, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
            double cum = chunk_cum[(size_t)c];
            int32_t run_max = 0;
            for (int64_t i = c * kChunkPairs; i < std::min(S, (c + 1) * kChunkPairs); ++i) {
                const double w = rel_w[sr[(size_t)i]];
                run_max = std::max(run_max, (int32_t)std::min<int64_t>(nparts - 1, (int64_t)((cum + 0.5 * w) * nparts / total_w)));
                part_of[(size_t)i] = run_max;
                cum += w;
            }
            chunk_last[(size_t)c] = run_max;
        }
    });
    // monotone over the chunks' borders too: a chunk starts no lower than the one before it ended
    for (int64_t c = 1; c < nchunks; ++c) {
        const int32_t carry = chunk_last[(size_t)c - 1];
        chunk_last[(size_t)c] = std::max(chunk_last[(size_t)c], carry);
        for (int64_t i = c * kChunkPairs; i < std::min(S, (c + 1) * kChunkPairs) && part_of[(size_t)i] < carry; ++i) part_of[(size_t)i] = carry;
    }
    for (int p = 0; p <= nparts; ++p)
        part_first[(size_t)p] = p == nparts ? S : std::lower_bound(part_of.begin(), part_of.end(), (int32_t)p) - part_of.begin();
    return part_first;
}

// The class of a pair INSIDE one block is free between the two classes that hold the block.  With eight position ranges an
// XCD's 32 compute units go to the three classes as 11 + 11 + 10, and a class that gets ten for a third of the batches
// has 65 per workgroup where the others have 59 (pose0-syn: 59-70 over the 256 workgroups, and the launch ends with the
// fullest - `tools/dm_stamps.py`: last waves done 11.9-16.0 us; evened out, 61-63 and 12.8-15.2 us, the step 1.2 us
// shorter on the same box).  So the free pairs are dealt per (part, relation, block) - a relation's pairs of a block stay
// one run - to whichever of the two classes is further below its share of the part: class loads in the ratio of the units
// they will get.  (What counts is a compute unit's batches, not its waves' trips: see the walks above.)
// (A group of a few hundred pairs or more - the head of the list is one or two relations - is CUT between its two classes
// where that evens them out: the first free_cut pairs of the group, in list order, go to the block's own class.)
// Returns free_cut[part][relation][block]: pairs of the group that go to class `block`; empty without three blocks on eight ranges.
inline std::vector<int32_t> free_cuts(const ScoredPairs& P, const ClassShape& sh, const std::vector<int64_t>& part_first, int cus) {
    std::vector<int32_t> free_cut;
    if (sh.nblocks != 3 || sh.parts != 8) return free_cut;
    const int64_t n_rel = P.n_rel;
    const int nparts = sh.nparts, walks = sh.walks;
    free_cut.assign((size_t)nparts * n_rel * 3, 0);
    const int W = cus / 8;
    std::vector<int64_t> fixed((size_t)nparts * 3, 0), flex((size_t)nparts * n_rel * 3, 0);
    gn::parallel_for(nparts, 1, [&](int64_t p0, int64_t p1) {
        for (int64_t part = p0; part < p1; ++part)
            for (int64_t i = part_first[(size_t)part]; i < part_first[(size_t)part + 1]; ++i) {
                const int bu = P.sbu[(size_t)i], bv = P.sbv[(size_t)i];
                if (bu != bv) fixed[(size_t)part * 3 + ((bu + 1) % 3 == bv ? bu : bv)]++;
                else flex[((size_t)part * n_rel + P.sr[(size_t)i]) * 3 + bu]++;
            }
    });
    gn::parallel_for(nparts, 1, [&](int64_t p0, int64_t p1) {
        for (int part = (int)p0; part < (int)p1; ++part) {
            // the units of the classes: as even as W allows, the smaller shares to the classes with the least fixed load - of the
            // whole RANGE (its workgroups keep their class through all its walks)
            const int x0 = part / walks * walks;
            int64_t fixed_x[3] = {0, 0, 0};
            for (int wk = 0; wk < walks; ++wk)
                for (int c = 0; c < 3; ++c) fixed_x[c] += fixed[(size_t)(x0 + wk) * 3 + c];
            int order3[3] = {0, 1, 2};
            std::sort(order3, order3 + 3, [&](int a, int b) { return fixed_x[a] != fixed_x[b] ? fixed_x[a] > fixed_x[b] : a < b; });
            double share[3];
            for (int k = 0; k < 3; ++k) share[order3[k]] = (double)(W / 3 + (k < W % 3 ? 1 : 0));
            double load[3] = {(double)fixed[(size_t)part * 3], (double)fixed[(size_t)part * 3 + 1], (double)fixed[(size_t)part * 3 + 2]};
            // largest groups first (ties in (relation, block) order)
            std::vector<std::pair<int64_t, int32_t>> groups;
            for (int64_t r = 0; r < n_rel; ++r)
                for (int b = 0; b < 3; ++b)
                    if (flex[((size_t)part * n_rel + r) * 3 + b] > 0) groups.push_back({-flex[((size_t)part * n_rel + r) * 3 + b], (int32_t)(r * 3 + b)});
            std::sort(groups.begin(), groups.end());
            for (const auto& gq : groups) {
                const int b = gq.second % 3, c0 = b, c1 = (b + 2) % 3;            // the two classes that hold block b
                const double m = (double)-gq.first;
                // x pairs to c0 so that both end at the same load per unit: (load0 + x) / share0 = (load1 + m - x) / share1
                double x = (share[c0] * (load[c1] + m) - share[c1] * load[c0]) / (share[c0] + share[c1]);
                x = std::min(m, std::max(0.0, x));
                if (m < 512.0) x = x >= 0.5 * m ? m : 0.0;                       // a small group stays one run
                else x = std::min(m, std::floor(x / 64.0 + 0.5) * 64.0);
                load[c0] += x; load[c1] += m - x;
                free_cut[(size_t)part * n_rel * 3 + gq.second] = (int32_t)x;
            }
        }
    });
    return free_cut;
}

// The scored pairs by (part, class, relation), list order inside: a stable counting sort, one position part per task (the
// buckets of a part are its own; round 6: std::stable_sort with a comparator over 10^6 indices was the builder's longest
// serial stretch, then the serial counting sort was).  A RUN = a non-empty bucket, padded to steps of 16 slots; a group's
// steps are padded to batches of four.
struct ClassRun { int64_t lo, hi; int grp, rel; int64_t step0; };
struct ClassRuns {
    gn::RawVec<uint32_t> key, idx;                               // (part, class) << 16 | relation of every pair; pair of every sorted position
    std::vector<ClassRun> runs;                                  // [lo, hi) of idx, (part, class), relation, first step inside the group
    std::vector<int64_t> grp_steps, grp_batch0;                  // steps of every group; first batch of every group, then the batch count
};

inline ClassRuns sort_into_runs(const ScoredPairs& P, const ClassShape& sh, const std::vector<int64_t>& part_first,
                                const std::vector<int32_t>& free_cut) {
    const int64_t S = P.size(), n_rel = P.n_rel;
    const int nparts = sh.nparts, nclasses = sh.nclasses, nblocks = sh.nblocks, ngroups = sh.ngroups;
    ClassRuns R;
    R.key.resize((size_t)S); R.idx.resize((size_t)S);
    const gn::RawVec<uint32_t>& key = R.key;
    std::vector<int32_t> free_seen(free_cut.size(), 0);
    const size_t nbuckets = (size_t)ngroups * (size_t)n_rel;
    std::vector<int64_t> first(nbuckets + 1, 0);
    auto bucket = [&](int64_t i) { return (size_t)(key[(size_t)i] >> 16) * (size_t)n_rel + (size_t)(key[(size_t)i] & 0xffffu); };
    gn::parallel_for(nparts, 1, [&](int64_t p0, int64_t p1) {
        for (int64_t part = p0; part < p1; ++part)
            for (int64_t i = part_first[(size_t)part]; i < part_first[(size_t)part + 1]; ++i) {
                const int bu = P.sbu[(size_t)i], bv = P.sbv[(size_t)i], rel = P.sr[(size_t)i];
                int c = 0;                                       // (cls_of, on the compact arrays)
                if (nblocks != 1) c = bu != bv ? ((bu + 1) % 3 == bv ? bu : bv) : ((rel & 1) ? (bu + 2) % 3 : bu);
                if (!free_cut.empty() && bu == bv) {
                    const size_t cell = ((size_t)part * n_rel + rel) * 3 + (size_t)bu;
                    c = free_seen[cell]++ < free_cut[cell] ? bu : (bu + 2) % 3;
                }
                R.key[(size_t)i] = (uint32_t)(part * nclasses + c) << 16 | (uint32_t)rel;
                first[bucket(i) + 1]++;
            }
    });
    GN_LAP("class: keys");
    for (size_t b = 1; b < first.size(); ++b) first[b] += first[b - 1];
    gn::parallel_for(nparts, 1, [&](int64_t p0, int64_t p1) {
        for (int64_t part = p0; part < p1; ++part)
            for (int64_t i = part_first[(size_t)part]; i < part_first[(size_t)part + 1]; ++i) R.idx[(size_t)first[bucket(i)]++] = (uint32_t)i;
    });
    GN_LAP("class: counting sort");
    // runs (the non-empty buckets: first[b] is now bucket b's end) -> steps of 16 slots
    R.grp_steps.assign((size_t)ngroups, 0);
    for (size_t b = 0; b < nbuckets; ++b) {
        const int64_t lo = b ? first[b - 1] : 0, hi = first[b];
        if (hi <= lo) continue;
        const int g = (int)(b / (size_t)n_rel);
        R.runs.push_back({lo, hi, g, (int)(b % (size_t)n_rel), R.grp_steps[g]});
        R.grp_steps[g] += gn::ceil_div(hi - lo, 16);
    }
    R.grp_batch0.assign((size_t)ngroups + 1, 0);
    for (int g = 0; g < ngroups; ++g) R.grp_batch0[g + 1] = R.grp_batch0[g] + gn::ceil_div(R.grp_steps[g], 4);
    return R;
}

// The runs' pairs in their slots: `batches` batches of 64 and kClsSlack readable ones behind them; rel16 = the relation of every step.
struct ClassSlots {
    int64_t batches = 0;
    gn::RawVec<uint32_t> packed, own, mirror;
    std::vector<uint16_t> rel16;
};

inline ClassSlots deal_runs_to_slots(const ScoredPairs& P, const ClassShape& sh, const ClassRuns& R, const gn::RawVec<int64_t>& scored) {
    const int64_t S = P.size();
    const int ngroups = sh.ngroups, nclasses = sh.nclasses;
    const std::vector<ClassRun>& runs = R.runs;
    const std::vector<int64_t>& grp_batch0 = R.grp_batch0;
    ClassSlots out;
    const int64_t NB = grp_batch0[ngroups], NBA = NB + kClsSlack;
    out.batches = NB;
    gn::RawVec<uint32_t>& packed = out.packed; gn::RawVec<uint32_t>& own = out.own; gn::RawVec<uint32_t>& mirror = out.mirror;
    std::vector<uint16_t>& rel16 = out.rel16;
    gn::parallel_assign(packed, (size_t)NBA * 64, 0u);
    gn::parallel_assign(own, (size_t)NBA * 64, kNoMirror);
    gn::parallel_assign(mirror, (size_t)NBA * 64, kNoMirror);
    rel16.assign((size_t)NBA * 4, 0);
    GN_LAP("class: output arrays");
    // tasks of about equal PAIR counts (contiguous runs): the runs of the list's head are two orders of magnitude longer than
    // those of its tail, and equal numbers of runs per builder thread left one thread with most of the pairs
    const std::vector<int64_t> task_first =
        equal_weight_tasks((int64_t)runs.size(), [&](int64_t ri) { return runs[(size_t)ri].hi - runs[(size_t)ri].lo; }, std::max<int64_t>(1, S / 256));
    GN_LAP("class: tasks");
    gn::parallel_for((int64_t)task_first.size() - 1, 1, [&](int64_t t0, int64_t t1) {
        std::vector<int> lu, lv, order;
        for (int64_t ri = task_first[(size_t)t0]; ri < task_first[(size_t)t1]; ++ri) {
            const ClassRun& run = runs[ri];
            const int count = (int)(run.hi - run.lo), cls = run.grp % nclasses;
            lu.resize(count); lv.resize(count);
            for (int k = 0; k < count; ++k) {
                const size_t i = (size_t)R.idx[run.lo + k];
                lu[k] = sh.local_row(P.su[i], P.sbu[i], cls); lv[k] = sh.local_row(P.sv[i], P.sbv[i], cls);
            }
            // dealt 64 consecutive pairs (one batch, one store instruction per lane) at a time: the 64 scores of a batch then
            // land inside a window of ~200 list positions.  Dealt over the whole run - more freedom for conflict-free
            // LDS cells - a batch's scores were spread over the relation's whole block and every lane's store became its own
            // 32-byte memory write: 202 MB written for the 33.5 MB of scores of pose2-syn (WRITE_SIZE), 71 us instead of 51
            order.clear();
            {
                std::vector<int> part;
                for (int c0 = 0; c0 < count; c0 += 64) {
                    const int cn = std::min(64, count - c0);
                    deal_run(lu.data() + c0, lv.data() + c0, cn, part);
                    for (int v : part) order.push_back(v >= 0 ? v + c0 : -1);
                }
            }
            const int steps = (int)(order.size() / 16);
            for (int t = 0; t < steps; ++t) {
                const int64_t gstep = grp_batch0[run.grp] * 4 + run.step0 + t;
                const int64_t bat = gstep >> 2;
                const int s_in = (int)(gstep & 3);
                rel16[(size_t)gstep] = (uint16_t)run.rel;
                for (int gq = 0; gq < 4; ++gq)
                    for (int k = 0; k < 4; ++k) {
                        const int pr = order[(size_t)t * 16 + gq * 4 + k];
                        const size_t slot = (size_t)bat * 64 + 4 * kGroupQuads[gq][k] + s_in;
                        const int src = pr >= 0 ? pr : 0;                       // padding repeats the run's first pair, writes nothing
                        packed[slot] = (uint32_t)lu[src] | (uint32_t)lv[src] << 16;
                        if (pr >= 0) {
                            const size_t i = (size_t)R.idx[run.lo + pr];
                            own[slot] = (uint32_t)scored[i];
                            mirror[slot] = P.sm[i];
                        }
                    }
            }
        }
    });
    GN_LAP("class: deal (parallel)");
    // steps that pad a group to whole batches: the relation of the step before them (no reload), pair (0, 0), no positions
    for (int g = 0; g < ngroups; ++g)
        for (int64_t gstep = grp_batch0[g] * 4 + R.grp_steps[g]; gstep < grp_batch0[g + 1] * 4; ++gstep)
            rel16[(size_t)gstep] = gstep > 0 ? rel16[(size_t)gstep - 1] : 0;
    for (int64_t gstep = NB * 4; gstep < NBA * 4; ++gstep) rel16[(size_t)gstep] = NB > 0 ? rel16[(size_t)NB * 4 - 1] : 0;
    return out;
}

// Workgroups: inside an XCD's range, a share of its compute units per class in proportion to the class's batches (over
// all the range's walks); a workgroup takes the same slice of its class's batches in every walk, contiguous batch
// ranges; with eight ranges workgroup 8 l + x is the l-th of range x.  Writes L.wg and L.groups; false when a range has
// fewer units than classes with work, or a workgroup's batches name more relations than its D cache holds.
inline bool describe_workgroups(const ClassShape& sh, const std::vector<int64_t>& grp_batch0, const std::vector<uint16_t>& rel16,
                                int cus, ClassLayout& L) {
    const int parts = sh.parts, walks = sh.walks, nclasses = sh.nclasses;
    const int64_t NB = grp_batch0[sh.ngroups];
    const int per_part = parts == 8 ? cus / 8 : (int)std::min<int64_t>(cus, std::max<int64_t>(NB, 1));
    struct Wg { int cls; int share, k; };
    std::vector<std::vector<Wg>> part_wgs(parts);
    for (int x = 0; x < parts; ++x) {
        int64_t nb_part = 0;
        int live = 0;
        std::vector<int64_t> nb_cls(nclasses, 0);
        for (int c = 0; c < nclasses; ++c) {
            for (int wk = 0; wk < walks; ++wk) { const int g = sh.group_of(x, wk, c); nb_cls[c] += grp_batch0[g + 1] - grp_batch0[g]; }
            nb_part += nb_cls[c];
            live += nb_cls[c] > 0;
        }
        const int W = parts == 8 ? per_part : std::max(std::min<int>(per_part, (int)std::max<int64_t>(nb_part, 1)), live);
        if (W < live) return false;
        std::vector<double> want(nclasses, 0.0);
        for (int c = 0; c < nclasses; ++c)
            if (nb_cls[c] > 0) want[c] = (double)W * nb_cls[c] / std::max<int64_t>(nb_part, 1);
        const std::vector<int> share = largest_remainder_shares(want.data(), nclasses, W, 1);
        for (int c = 0; c < nclasses; ++c)
            for (int k = 0; k < share[c]; ++k) part_wgs[x].push_back({c, share[c], k});
        while (parts == 8 && (int)part_wgs[x].size() < W) part_wgs[x].push_back({0, 0, 0});      // (a range without work for all its units)
    }
    int G = 0;
    for (int x = 0; x < parts; ++x) G += (int)part_wgs[x].size();
    if (G < 1) return false;
    const int dstride = 4 + 4 * walks;
    L.wg.assign((size_t)G * dstride, 0);
    L.wg_cls.assign((size_t)G, 0);
    for (int x = 0; x < parts; ++x)
        for (size_t l = 0; l < part_wgs[x].size(); ++l) {
            const Wg& w = part_wgs[x][l];
            const int c = w.cls;
            const size_t at = parts == 8 ? (size_t)(8 * l + x) : l;
            int32_t* d = L.wg.data() + at * dstride;
            if (sh.nblocks == 1) { d[0] = 0; d[1] = (int32_t)sh.n; d[2] = 0; d[3] = 0; }
            else { d[0] = (int32_t)sh.bstart(c); d[1] = (int32_t)sh.bsize(c); d[2] = (int32_t)sh.bstart((c + 1) % 3); d[3] = (int32_t)sh.bsize((c + 1) % 3); }
            L.wg_cls[at] = (uint8_t)c;
            for (int k = 0; k < 4; ++k) L.cls_rows[c][k] = d[k];
            for (int wk = 0; wk < walks; ++wk) {
                const int g = sh.group_of(x, wk, c);
                const int64_t nb = grp_batch0[g + 1] - grp_batch0[g];
                const int64_t lo = w.share ? grp_batch0[g] + nb * w.k / w.share : 0, hi = w.share ? grp_batch0[g] + nb * (w.k + 1) / w.share : 0;
                int rlo = 1 << 30, rhi = -1;
                for (int64_t gstep = lo * 4; gstep < hi * 4; ++gstep) { rlo = std::min<int>(rlo, rel16[(size_t)gstep]); rhi = std::max<int>(rhi, rel16[(size_t)gstep]); }
                if (hi <= lo) { rlo = 0; rhi = 0; }
                if (rhi - rlo + 1 > kClsDCache) return false;                     // (the column-phase kernel serves such a list)
                d[4 + 4 * wk] = (int32_t)lo; d[5 + 4 * wk] = (int32_t)hi; d[6 + 4 * wk] = rlo; d[7 + 4 * wk] = rhi - rlo + 1;
            }
        }
    L.groups = G;
    return true;
}

template <typename V>
inline ClassLayout build_class_layout(const V& hu, const V& hv, const V& hr,
                                      const gn::RawVec<int64_t>& scored, const gn::RawVec<int64_t>& mirror_of, int64_t n,
                                      int64_t features, int cus, int64_t window_bytes = kClsWindowBytes) {
#ifdef GN_LAYOUT_TIMES
    struct ExitLap { ~ExitLap() { GN_LAP("class: locals freed"); } } exit_lap;
#endif
    ClassLayout L;
    ClassShape sh;
    if (!class_shape(n, features, (int64_t)scored.size(), (int64_t)hu.size(), cus, window_bytes, sh)) return L;
    GN_LAP(nullptr);
    const ScoredPairs P = compact_scored_pairs(hu, hv, hr, scored, mirror_of, sh);
    GN_LAP("class: compact arrays (parallel)");
    const std::vector<int64_t> part_first = position_parts(P, sh);
    GN_LAP("class: position parts");
    const std::vector<int32_t> free_cut = free_cuts(P, sh, part_first, cus);
    GN_LAP("class: free cuts");
    const ClassRuns R = sort_into_runs(P, sh, part_first, free_cut);     // (laps "class: keys" and "class: counting sort" inside)
    GN_LAP("class: runs");
    ClassSlots slots = deal_runs_to_slots(P, sh, R, scored);             // ("class: output arrays", "class: tasks", "class: deal (parallel)")
    if (!describe_workgroups(sh, R.grp_batch0, slots.rel16, cus, L)) { L.wg.clear(); return L; }
    L.rel32.resize(slots.rel16.size() / 2);
    for (size_t i = 0; i < L.rel32.size(); ++i) L.rel32[i] = (uint32_t)slots.rel16[2 * i] | (uint32_t)slots.rel16[2 * i + 1] << 16;
    GN_LAP("class: workgroups + rel32");
    L.packed.swap(slots.packed); L.own.swap(slots.own); L.mirror.swap(slots.mirror);
    L.batches = slots.batches; L.walks = sh.walks;
    L.ok = true;
    return L;
}

// The column-phase encoding (k_distmult_plan in distmult_plan.hip).  Batches: 64 consecutive scored edges each, in list
// order; a batch's slots are dealt independently of the others.  packed = u | v << node_bits; batch_rel = the batch's
// relation when all its edges share one, else -1 (the kernel then reads rel16 per slot).
struct PhaseLayout {
    std::vector<uint32_t> packed, own, mirror;    // [batches][64]
    std::vector<int32_t> batch_rel;               // [batches]
    std::vector<uint16_t> rel16;                  // [batches][64]
};

template <typename V>
inline PhaseLayout build_phase_layout(const V& hu, const V& hv, const V& hr, const gn::RawVec<int64_t>& scored,
                                      const gn::RawVec<int64_t>& mirror_of, int node_bits) {
    PhaseLayout L;
    const int64_t NBs = gn::ceil_div((int64_t)scored.size(), 64);
    L.packed.resize((size_t)NBs * 64); L.own.resize((size_t)NBs * 64); L.mirror.resize((size_t)NBs * 64);
    L.batch_rel.resize((size_t)NBs);
    L.rel16.resize((size_t)NBs * 64);
    gn::parallel_for(NBs, 64, [&](int64_t b0, int64_t b1) {
        int slot_of_edge[64];
        int64_t cu[64], cv[64], ce[64];
        for (int64_t bi = b0; bi < b1; ++bi) {
            const int count = (int)std::min<int64_t>(64, (int64_t)scored.size() - bi * 64);
            for (int k = 0; k < count; ++k) { ce[k] = scored[bi * 64 + k]; cu[k] = hu[ce[k]]; cv[k] = hv[ce[k]]; }
            deal_batch(cu, cv, count, slot_of_edge);
            bool uniform = true;
            for (int k = 1; k < count; ++k) uniform = uniform && hr[ce[k]] == hr[ce[0]];
            const size_t s0 = (size_t)bi * 64;
            L.batch_rel[bi] = uniform ? (int32_t)hr[ce[0]] : -1;
            bool taken[64] = {false};
            auto fill = [&](int s, int k) {
                const int64_t e = ce[k];
                L.packed[s0 + s] = (uint32_t)hu[e] | ((uint32_t)hv[e] << node_bits);
                L.own[s0 + s] = (uint32_t)e;
                L.rel16[s0 + s] = (uint16_t)hr[e];
                L.mirror[s0 + s] = mirror_of[e] >= 0 ? (uint32_t)mirror_of[e] : kNoMirror;
            };
            for (int k = 0; k < count; ++k) { taken[slot_of_edge[k]] = true; fill(slot_of_edge[k], k); }
            // a slot without an edge repeats the batch's first one: the same score into the same positions
            for (int s = 0; s < 64; ++s)
                if (!taken[s]) fill(s, 0);
        }
    });
    return L;
}

}  // namespace gn_layout
