// Host schedule of the LDS-accumulator relational kernel (rgcn_fast.hip): work items out of the (relation, source tile)
// segments, their pieces dealt to the persistent workgroups, and the descriptors every workgroup walks.  No HIP.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "layout_util.hpp"

namespace gn_layout {

constexpr int kFastFout = 32;                            // out_features of the layer this kernel is built for,
constexpr int kFastMaxFin = 64;                          // in_features: 16, 32, 48 or 64 (the finalisation alone: any up to 64)
constexpr int kFastGroups = 256;                         // persistent workgroups = CUs of an MI355X
constexpr int kFastChunk = 4096;                         // packed words per work item = LDS edge buffer (16 KB)
constexpr int kFastItemEdges = kFastChunk - 3 * 128;     // edges per work item: every one of the 128 slot lists is padded to 4 words
constexpr int kFastItemOverhead = 2048;                  // H-tile cost in edge equivalents (LPT balancing)

// One work item as the kernel reads it (32 bytes, wave-uniform scalar load).
struct alignas(32) FastWorkDesc {
    int32_t rel, tile, start, count, item, pad0, pad1, pad2;
};
constexpr int kFastDescWords = (int)(sizeof(FastWorkDesc) / sizeof(int32_t));
static_assert(kFastDescWords == 8, "the kernel loads a descriptor as eight words");

// Work items: every non-empty (relation, tile) segment of the key-sorted edges, cut into chunks of <= kFastItemEdges edges.
// Balancing unit = piece: up to `piece_chunks` consecutive items of one segment - a workgroup that runs them back to back
// builds the segment's H tile once.  Pieces go to the workgroups by longest processing time first.
struct FastItems {
    std::vector<int32_t> item_rel, item_tile;   // [n_items]
    std::vector<int32_t> item_begin;            // [n_items + 1] first edge of every item, then E
    std::vector<int32_t> piece_first;           // [n_pieces + 1] first item of every piece, then n_items
    std::vector<int32_t> piece_group;           // [n_pieces] the workgroup that runs the piece
    int groups = 0;                             // 0: more than `max_items` items (nothing behind item_begin is built)
    int n_items() const { return (int)item_rel.size(); }
    int n_pieces() const { return (int)piece_group.size(); }
    int64_t piece_cost(int pc) const { return (int64_t)kFastItemOverhead + (item_begin[piece_first[pc + 1]] - item_begin[piece_first[pc]]); }
};

// `seg`: [R * tiles + 1] offsets of the segments (relation-major) into the E sorted edges.
inline FastItems build_fast_items(const std::vector<int32_t>& seg, int tiles, int64_t E, int64_t max_items = INT32_MAX) {
    FastItems L;
    const int n_seg = (int)seg.size() - 1;
    int64_t total_cost = 0;
    for (int sg = 0; sg < n_seg; ++sg) {
        for (int32_t b = seg[sg]; b < seg[sg + 1]; b += kFastItemEdges) {
            L.item_rel.push_back(sg / tiles);
            L.item_tile.push_back(sg % tiles);
            L.item_begin.push_back(b);
        }
        if (seg[sg + 1] > seg[sg]) total_cost += kFastItemOverhead + (seg[sg + 1] - seg[sg]);
    }
    const int n_items = L.n_items();
    L.item_begin.push_back((int32_t)E);
    if (n_items > max_items) return L;
    const int groups0 = std::min(kFastGroups, std::max(n_items, 1));
    const int64_t piece_cap = std::max<int64_t>(kFastItemOverhead + kFastItemEdges, total_cost / groups0 / 4);
    const int piece_chunks = (int)std::max<int64_t>(1, (piece_cap - kFastItemOverhead) / kFastItemEdges);
    for (int i = 0; i < n_items;) {
        int jn = i + 1;
        while (jn < n_items && jn - i < piece_chunks && L.item_rel[jn] == L.item_rel[i] && L.item_tile[jn] == L.item_tile[i]) ++jn;
        L.piece_first.push_back(i);
        i = jn;
    }
    const int n_pieces = (int)L.piece_first.size();
    L.piece_first.push_back(n_items);
    L.piece_group.assign((size_t)n_pieces, 0);
    L.groups = std::min(groups0, std::max(n_pieces, 1));
    // longest-processing-time assignment of pieces to the persistent workgroups
    const std::vector<int> order = descending_order<int>(n_pieces, [&](int x) { return L.piece_cost(x); });
    std::vector<std::pair<int64_t, int>> heap;   // min-heap over (load, group)
    for (int g = 0; g < L.groups; ++g) heap.emplace_back(0, g);
    auto cmp = [](const std::pair<int64_t, int>& x, const std::pair<int64_t, int>& y) { return x > y; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (int pc : order) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        auto& top = heap.back();
        L.piece_group[pc] = top.second;
        top.first += L.piece_cost(pc);
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
    return L;
}

// Per workgroup: all items of one source tile together (the X fragments stay in registers), relation order inside a tile
// (W_r reuse in L2) - its items sorted by (tile, item).  `item_pad`: [n_items + 1] offsets of the items' padded edge words.
struct FastWork {
    std::vector<int32_t> wg_begin;   // [groups + 1] ranges into the descriptors
    std::vector<int32_t> desc;       // [n_items][kFastDescWords]: FastWorkDesc
};

inline FastWork build_fast_work(const FastItems& L, const std::vector<int32_t>& item_pad) {
    FastWork W;
    const int n_items = L.n_items();
    std::vector<std::vector<int32_t>> bins((size_t)L.groups);
    for (int pc = 0; pc < L.n_pieces(); ++pc)
        for (int32_t it = L.piece_first[pc]; it < L.piece_first[pc + 1]; ++it) bins[L.piece_group[pc]].push_back(it);
    W.wg_begin.assign((size_t)L.groups + 1, 0);
    W.desc.reserve((size_t)n_items * kFastDescWords);
    for (int g = 0; g < L.groups; ++g) {
        std::sort(bins[g].begin(), bins[g].end(), [&](int32_t x, int32_t y) {
            return L.item_tile[x] != L.item_tile[y] ? L.item_tile[x] < L.item_tile[y] : x < y;
        });
        for (int32_t it : bins[g]) {
            const FastWorkDesc w = {L.item_rel[it], L.item_tile[it], item_pad[it], item_pad[it + 1] - item_pad[it], it, 0, 0, 0};
            int32_t words[kFastDescWords];
            std::memcpy(words, &w, sizeof w);
            W.desc.insert(W.desc.end(), words, words + kFastDescWords);
        }
        W.wg_begin[g + 1] = (int32_t)(W.desc.size() / kFastDescWords);
    }
    return W;
}

}  // namespace gn_layout
