// Layout of the relational layer's destination-major kernel (rgcn_pair.hip).  No HIP.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_parallel.hpp"
#include "layout_util.hpp"

namespace gn_layout {

// ---- relational layer, destination-major kernel (rgcn_pair.hip) -----------------------------------------------------------
constexpr int kPairWaves = 16;             // waves of a workgroup: four per SIMD, 128 registers each, one destination row per wave
constexpr int kPairThreads = kPairWaves * 64;
constexpr int kPairLdsBytes = 160 * 1024;  // the workgroup's LDS: the compute unit's
constexpr int kPairRowBytes = 128;         // LDS stride of an att row (32 bases; fewer: zero padded)
// what the kernel is instantiated for (rgcn_route.hpp holds the rule)
constexpr int kPairMaxFin = 64, kPairMaxFout = 64, kPairMaxBases = kPairRowBytes / 4;
constexpr int kPairMaxTiles = 6;           // (fin / 16) * ceil(bases / 16): accumulator tiles of a lane
constexpr int kPairRegRows = 16, kPairRegRowsWide = 12;   // rows of basis a thread holds in registers in the epilogue; at fin 48 and 64
constexpr int kPairMaxD = 3;               // destination rows per workgroup
constexpr int kPairSectionCap = 64;        // blocks of a section inside one unit
constexpr int kPairSlackBlocks = 192;      // readable blocks behind the last wave's stream (the window reads ahead)

// The blocks of one section: four lists of relation ids (one per lane group), `nb` blocks of four positions each.
// Lane groups 0/1 and 2/3 share the 32 lanes of one LDS access: rows of equal parity sit in the same banks, so the
// lists of a group pair are laid out even rows first / odd rows last against odd rows first / even rows last, and a
// padded position names the zero row of the parity its partner does not use.
inline void lay_out_section(const uint32_t* const (&list)[4], const int (&len)[4], int nb, uint32_t R, std::vector<uint32_t>& out) {
    const int P = 4 * nb;
    const uint32_t none = 0xffffffffu;
    // (on the stack, and without data-dependent branches: a plan lays out 10^5 sections of a dozen rows each, and the parity
    // of a relation id is a coin flip - with a branch per row the mispredictions were most of the layout's time)
    uint32_t pos[4][4 * kPairSectionCap], lead[4 * kPairSectionCap + 1], trail[4 * kPairSectionCap + 1];
    for (int k = 0; k < 4; ++k) {
        const uint32_t lead_parity = (k & 1) ? 1u : 0u;
        // first the rows of the leading parity, left aligned, in list order; then the others, right aligned, in list order
        int nl = 0, nt = 0;
        for (int i = 0; i < len[k]; ++i) {
            const uint32_t v = list[k][i];
            const int is_lead = (v & 1u) == lead_parity;
            lead[nl] = v; trail[nt] = v;
            nl += is_lead; nt += 1 - is_lead;
        }
        uint32_t* pk = pos[k];
        for (int i = 0; i < nl; ++i) pk[i] = lead[i];
        for (int i = nl; i < P - nt; ++i) pk[i] = none;
        for (int i = 0; i < nt; ++i) pk[P - nt + i] = trail[i];
    }
    const uint32_t zero_even = (R & 1u) ? R + 1 : R, zero_odd = (R & 1u) ? R : R + 1;
    const size_t base = out.size();
    out.resize(base + (size_t)nb * 16);
    uint32_t* o = out.data() + base;
    for (int k = 0; k < 4; ++k) {
        const uint32_t* mine = pos[k];
        const uint32_t* theirs = pos[k ^ 1];
        const uint32_t both_padded = (k & 1) ? zero_odd : zero_even;             // two padded partners: one of each
        for (int i = 0; i < P; ++i) {
            const uint32_t row = mine[i], other = theirs[i];
            uint32_t pad = (other & 1u) == 0u ? zero_odd : zero_even;             // the zero row of the parity the partner does not use
            pad = other == none ? both_padded : pad;
            o[(size_t)(i >> 2) * 16 + k * 4 + (i & 3)] = (row == none ? pad : row) * (uint32_t)kPairRowBytes;
        }
    }
}

// Units, per-wave streams and descriptors of the destination-major plan.  rp: [N * kpad + 1] first edge of every
// (destination, K position) cell of the edge list sorted by that key; rels: the relation of every sorted edge; perm: the
// source node at every K position (N: none).  G workgroups, up to D rows each.
struct PairLayout {
    bool ok = false;
    int64_t blocks = 0;
    gn::RawVec<uint32_t> stream;
    std::vector<uint32_t> wave_first, desc, wave_units, wave_desc;
    std::vector<int32_t> wg_dst;
};

// A unit = (destination, chunk, slice j of <= kPairSectionCap blocks per section).  Blocks of a section = the longest of
// its four pairs, in fours, at least one; a (destination, chunk) without any edge is no unit at all.
// K order PER DESTINATION: its (destination, source) pairs by edge count, longest first, four consecutive ones to the
// four lane groups of a section - lock-step partners then have (nearly) equal runs and what is left of the padding is
// the rounding to blocks of four (pose0-syn: 1.83 -> 1.32 x the edges, tools/pair_sim.py).  kord[i][pos] = the global
// K position (cell of `rp`) that sits at operand position pos = 32 chunk + 8 group + t of destination i; the sources
// of a (destination, chunk) are a row of `perm2` (the kernel reads its x rows through it).  cost[i] = the row's blocks.
struct PairOrder {
    const std::vector<int32_t>& rp;
    int chunks, kpad;
    std::vector<int32_t> kord, perm2;
    std::vector<int64_t> cost;
    size_t cell(int64_t i, int pos) const { return (size_t)i * kpad + kord[(size_t)i * kpad + pos]; }
    int pair_len(int64_t i, int pos) const { const size_t c = cell(i, pos); return rp[c + 1] - rp[c]; }
    bool chunk_empty(int64_t i, int ch) const { return pair_len(i, 32 * ch) == 0; }   // (position 32 ch holds the chunk's longest pair)
    int section_blocks(int64_t i, int ch, int t) const {
        int longest = 0;
        for (int k = 0; k < 4; ++k) longest = std::max(longest, pair_len(i, 32 * ch + 8 * k + t));
        return std::max(1, (longest + 3) / 4);
    }
};

inline PairOrder pair_k_order(int64_t N, int chunks, int kpad, const std::vector<int32_t>& rp, const std::vector<int32_t>& perm) {
    PairOrder O{rp, chunks, kpad, std::vector<int32_t>((size_t)N * kpad), std::vector<int32_t>((size_t)N * kpad), std::vector<int64_t>(N, 0)};
    gn::parallel_for(N, 8, [&](int64_t b, int64_t e) {
        std::vector<int32_t> idx(kpad);
        std::vector<uint64_t> keyed(kpad);
        for (int64_t i = b; i < e; ++i) {
            const int32_t* r = rp.data() + (size_t)i * kpad;
            // longest first, equal lengths in K order: a counting sort when the lengths are small (they are: a few edges per
            // (destination, source) pair), else one sort of (complement of the length, position) words
            int longest = 0;
            for (int q = 0; q < kpad; ++q) longest = std::max(longest, r[q + 1] - r[q]);
            if (longest < 1024) {
                int32_t start[1025];
                std::fill(start, start + longest + 2, 0);
                for (int q = 0; q < kpad; ++q) start[longest - (r[q + 1] - r[q]) + 1]++;
                for (int l = 0; l <= longest; ++l) start[l + 1] += start[l];
                for (int q = 0; q < kpad; ++q) idx[start[longest - (r[q + 1] - r[q])]++] = q;
            } else {
                for (int q = 0; q < kpad; ++q) keyed[q] = (uint64_t)(0x7fffffff - (r[q + 1] - r[q])) << 32 | (uint32_t)q;
                std::sort(keyed.begin(), keyed.end());
                for (int q = 0; q < kpad; ++q) idx[q] = (int32_t)(uint32_t)keyed[q];
            }
            for (int q = 0; q < kpad; ++q) {
                const int ch = q >> 5, t = (q & 31) >> 2, k = q & 3;
                const size_t pos = (size_t)i * kpad + 32 * ch + 8 * k + t;
                O.kord[pos] = idx[q];
                // a pair without edges names no source: its x row is not read and counts as zero, so a non-finite x[s]
                // reaches only the destinations s has an edge to (0 . inf would be NaN), as in the reference's edge sum
                O.perm2[pos] = r[idx[q] + 1] > r[idx[q]] ? perm[idx[q]] : (int32_t)N;
            }
            // the row's cost (its K order is known now): blocks of all its sections, + a unit's split and matrix products
            int64_t blocks = 0;
            for (int ch = 0; ch < chunks; ++ch) {
                if (O.chunk_empty(i, ch)) continue;
                int deepest = 1;
                for (int t = 0; t < 8; ++t) {
                    const int nb = O.section_blocks(i, ch, t);
                    deepest = std::max(deepest, nb);
                    blocks += nb;
                }
                blocks += 12 * gn::ceil_div(deepest, kPairSectionCap);             // in block times
            }
            O.cost[i] = blocks;
        }
    });
    return O;
}

// Destinations to workgroups: longest first, each to the least loaded workgroup that still has room.
inline std::vector<std::vector<int32_t>> pair_rows_to_workgroups(int64_t N, int G, int D, const std::vector<int64_t>& cost) {
    std::vector<std::vector<int32_t>> wg_rows(G);
    std::vector<int64_t> load(G, 0);
    for (int32_t i : descending_order<int32_t>(N, [&](int32_t x) { return cost[x]; })) {
        int best = -1;
        for (int gg = 0; gg < G; ++gg)
            if ((int)wg_rows[gg].size() < D && (best < 0 || load[gg] < load[best])) best = gg;
        wg_rows[best].push_back(i);
        load[best] += cost[i];
    }
    return wg_rows;
}

// Per workgroup: every destination row gets a share of the sixteen waves in proportion to its cost (at least one), a
// wave a contiguous run of its row's units (chunk order) of equal cost; per wave the descriptors (eight dwords a unit,
// pages of eight units) and the stream.
struct PairWaves {
    std::vector<std::vector<uint32_t>> stream, desc;             // [G * kPairWaves] of every wave
    std::vector<uint32_t> wave_units;
    std::vector<int32_t> wg_dst;
};

inline PairWaves pair_wave_streams(const PairOrder& O, int64_t R, int G, const std::vector<std::vector<int32_t>>& wg_rows,
                                   const std::vector<uint32_t>& rels) {
    const std::vector<int32_t>& rp = O.rp;
    const int chunks = O.chunks;
    PairWaves W;
    W.stream.resize((size_t)G * kPairWaves); W.desc.resize((size_t)G * kPairWaves);
    W.wave_units.assign((size_t)G * kPairWaves, 0u);
    W.wg_dst.assign((size_t)G * 4, -1);
    gn::parallel_for(G, 1, [&](int64_t b, int64_t e) {
        struct Unit { int32_t ch, slice; int64_t cost; };
        std::vector<Unit> units;
        for (int64_t gg = b; gg < e; ++gg) {
            const std::vector<int32_t>& rows = wg_rows[gg];
            const int nd = (int)rows.size();
            for (int d = 0; d < nd; ++d) W.wg_dst[gg * 4 + d] = rows[d];
            // waves per row: largest remainders of the proportional share
            int64_t cost_total = 0;
            for (int d = 0; d < nd; ++d) cost_total += std::max<int64_t>(O.cost[rows[d]], 1);
            double want[kPairMaxD] = {0, 0, 0};
            for (int d = 0; d < nd; ++d) want[d] = (double)kPairWaves * std::max<int64_t>(O.cost[rows[d]], 1) / cost_total;
            const std::vector<int> share = largest_remainder_shares(want, nd, kPairWaves, 1);
            int wave0 = 0;
            uint32_t starts = 0;
            for (int d = 0; d < nd; ++d) {
                if (d == 1) starts |= (uint32_t)wave0;
                if (d == 2) starts |= (uint32_t)wave0 << 8;
                const int64_t i = rows[d];
                units.clear();
                int64_t total = 0;
                for (int ch = 0; ch < chunks; ++ch) {
                    if (O.chunk_empty(i, ch)) continue;
                    int nb[8], deepest = 1;
                    for (int t = 0; t < 8; ++t) { nb[t] = O.section_blocks(i, ch, t); deepest = std::max(deepest, nb[t]); }
                    for (int j = 0; j * kPairSectionCap < deepest; ++j) {
                        int64_t c = 16;                                        // x chunk, split, matrix products: in block times
                        for (int t = 0; t < 8; ++t) c += std::max(1, std::min(kPairSectionCap, nb[t] - j * kPairSectionCap));
                        units.push_back({ch, j, c});
                        total += c;
                    }
                }
                int64_t seen = 0;
                for (const Unit& un : units) {
                    // the wave of this row whose share of the cost line holds this unit's midpoint
                    const int wv = wave0 + (total > 0 ? (int)std::min<int64_t>(share[d] - 1, (2 * seen + un.cost) * share[d] / (2 * total)) : 0);
                    seen += un.cost;
                    std::vector<uint32_t>& out = W.stream[gg * kPairWaves + wv];
                    std::vector<uint32_t>& dv = W.desc[gg * kPairWaves + wv];
                    const size_t at = dv.size();
                    dv.resize(at + 32, 0u);
                    for (int q = 0; q < 16; ++q) {                             // the chunk's sources, 16 bits each (N: none)
                        const int32_t* ids = O.perm2.data() + ((size_t)i * chunks + un.ch) * 32 + 2 * q;
                        dv[at + 8 + q] = (uint32_t)ids[0] | (uint32_t)ids[1] << 16;
                    }
                    for (int t = 0; t < 8; ++t) {
                        const uint32_t* list[4];
                        int len[4], longest = 0;
                        for (int k = 0; k < 4; ++k) {
                            const size_t key_id = O.cell(i, 32 * un.ch + 8 * k + t);
                            const int full = rp[key_id + 1] - rp[key_id];
                            const int from = std::min(full, un.slice * kPairSectionCap * 4);
                            list[k] = rels.data() + rp[key_id] + from;
                            len[k] = std::min(full - from, kPairSectionCap * 4);
                            longest = std::max(longest, len[k]);
                        }
                        const int nb = std::max(1, (longest + 3) / 4);
                        dv[at + (t >> 2)] |= (uint32_t)nb << (8 * (t & 3));
                        lay_out_section(list, len, nb, (uint32_t)R, out);
                    }
                    W.wave_units[gg * kPairWaves + wv] += 1;
                }
                wave0 += share[d];
            }
            if (nd < 2) starts |= (uint32_t)kPairWaves;
            if (nd < 3) starts |= (uint32_t)kPairWaves << 8;
            W.wg_dst[gg * 4 + 3] = (int32_t)starts;
            for (int wv = 0; wv < kPairWaves; ++wv) {                              // whole pages
                std::vector<uint32_t>& dv = W.desc[gg * kPairWaves + wv];
                dv.resize((dv.size() + 63) / 64 * 64, 0u);
            }
        }
    });
    return W;
}

// The waves' descriptors and streams one after the other, the slack behind them.  false: more blocks than a 31-bit index holds.
inline bool pair_concatenate(PairWaves& W, int64_t R, PairLayout& L) {
    L.wave_desc.resize(W.desc.size());
    for (size_t i = 0; i < W.desc.size(); ++i) {
        L.wave_desc[i] = (uint32_t)(L.desc.size() / 32);
        L.desc.insert(L.desc.end(), W.desc[i].begin(), W.desc[i].end());
    }
    L.desc.resize(L.desc.size() + 128, 0u);                                     // a wave without units still reads a page (and the one after)
    L.wave_first.resize(W.stream.size());
    size_t total = 0;
    for (size_t i = 0; i < W.stream.size(); ++i) { L.wave_first[i] = (uint32_t)(total / 16); total += W.stream[i].size(); }
    if (total / 16 + kPairSlackBlocks >= ((size_t)1 << 31)) return false;
    L.stream.resize(total + (size_t)kPairSlackBlocks * 16);                     // (the waves' streams tile [0, total): only the slack is filled)
    std::fill(L.stream.begin() + (std::ptrdiff_t)total, L.stream.end(), (uint32_t)R * kPairRowBytes);
    gn::parallel_for((int64_t)W.stream.size(), 64, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i)
            if (!W.stream[i].empty()) memcpy(L.stream.data() + (size_t)L.wave_first[i] * 16, W.stream[i].data(), W.stream[i].size() * sizeof(uint32_t));
    });
    L.blocks = (int64_t)(total / 16);
    L.wave_units.swap(W.wave_units);
    L.wg_dst.swap(W.wg_dst);
    return true;
}

inline PairLayout build_pair_layout(int64_t N, int64_t R, int chunks, int kpad, int G, int D, const std::vector<int32_t>& rp,
                                    const std::vector<uint32_t>& rels, const std::vector<int32_t>& perm) {
    GN_LAP(nullptr);
    const PairOrder O = pair_k_order(N, chunks, kpad, rp, perm);
    GN_LAP("pair: K order + costs (parallel)");
    const std::vector<std::vector<int32_t>> wg_rows = pair_rows_to_workgroups(N, G, D, O.cost);
    GN_LAP("pair: rows to workgroups");
    PairWaves W = pair_wave_streams(O, R, G, wg_rows, rels);
    GN_LAP("pair: streams (parallel)");
    PairLayout L;
    if (!pair_concatenate(W, R, L)) return PairLayout();
    GN_LAP("pair: concatenate");
    L.ok = true;
    return L;
}

}  // namespace gn_layout
