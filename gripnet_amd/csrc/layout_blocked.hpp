// Layout of the gene layers' LDS-staged gather (gcn_blocked.hip).  No HIP.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_parallel.hpp"
#include "layout_util.hpp"

namespace gn_layout {

// ---- gene layers, LDS-staged gather (gcn_blocked.hip) -----------------------------------------------------------------------
constexpr int kColLayoutWaves = 16;        // waves of a k_col_gather workgroup
constexpr int kColLayoutSlack = 32;        // spare iterations behind the id stream

// Destination rows -> ranges -> 16-row tiles -> (iteration, slot) of every edge, chosen for conflict-free LDS reads.
// rp / col: the destination-major CSR; dis: deg^-1/2 per node (zero padded).  R ranges of destination rows.
struct BlockedLayout {
    bool ok = false, failed = false;
    int64_t iters_total = 0;
    std::vector<int32_t> tile_off, tile_rows, cell;
    std::vector<float> tile_dis;
    gn::RawVec<uint16_t> ids;
};

// Destination rows by degree (descending, stable), dealt to the ranges in a snake: every range gets the same number
// of edges (to within a row) and rows of every degree; inside a range the rows stay in degree order, so that the 16
// rows of a tile have similar lengths
inline std::vector<std::vector<int32_t>> blocked_range_rows(int64_t N, int R, const std::vector<int32_t>& rp) {
    const std::vector<int32_t> order = descending_order<int32_t>(N, [&](int32_t x) { return rp[x + 1] - rp[x]; });
    std::vector<std::vector<int32_t>> range_rows(R);
    for (int64_t k = 0; k < N; ++k) {
        const int64_t lap = k / R, pos = k % R;
        range_rows[(lap & 1) ? R - 1 - pos : pos].push_back(order[k]);
    }
    return range_rows;
}

// Tiles of 16 rows; a row's edges are dealt to the 4 lanes of its quad, 4 ids per lane and iteration.  Which edge
// goes into which (iteration, slot) is free (the order of a sum), so it is chosen for the LDS: ds_read_b64 (and
// b32) serves lanes 0-31 and 32-63 as two access groups, conflict-free when the ids of a group differ mod 32.
// (the ranges are scheduled independently of each other, on the plan builders' threads, and concatenated in order)
struct BlockedRange { std::vector<int32_t> tile_iters, tile_rows; std::vector<uint16_t> ids; bool failed = false; };

inline std::vector<BlockedRange> blocked_schedule_ranges(int64_t N, int R, const std::vector<std::vector<int32_t>>& range_rows,
                                                         const std::vector<int32_t>& rp, const std::vector<int32_t>& col) {
    std::vector<BlockedRange> built(R);
    const uint16_t zero_id = (uint16_t)N;
    gn::parallel_for(R, 1, [&](int64_t r0, int64_t r1) {
        // a row's ids by (id mod 32): thirty-two stacks in one flat array (filled in CSR order, popped from the back), their
        // live sizes in cnt[row][class] - the scheduler's inner loop is "the fullest class of this row that this instruction's
        // access group has not used yet", a scan of 32 counters (round 6: with a std::vector per stack the scan chased 64
        // pointers and the gene plan spent 10 ms of sixteen threads here)
        std::vector<uint16_t> flat;
        int32_t cnt[16][32], first[16][32];
        for (int64_t r = r0; r < r1; ++r) {
            const std::vector<int32_t>& rows = range_rows[r];
            BlockedRange& o = built[r];
            const int tiles_r = (int)gn::ceil_div((int64_t)rows.size(), 16);
            o.tile_rows.reserve((size_t)tiles_r * 16);
            o.tile_iters.reserve((size_t)tiles_r);
            for (int tl = 0; tl < tiles_r; ++tl) {
                int32_t trow[16], rem[16];
                int iters = 0;
                size_t total = 0;
                for (int qi = 0; qi < 16; ++qi) {
                    const size_t k = (size_t)tl * 16 + qi;
                    trow[qi] = k < rows.size() ? rows[k] : -1;
                    rem[qi] = trow[qi] < 0 ? 0 : rp[trow[qi] + 1] - rp[trow[qi]];
                    total += (size_t)rem[qi];
                    iters = std::max(iters, (rem[qi] + 15) / 16);
                }
                if (flat.size() < total) flat.resize(total);
                size_t at = 0;
                for (int qi = 0; qi < 16; ++qi) {
                    for (int c = 0; c < 32; ++c) cnt[qi][c] = 0;
                    if (trow[qi] < 0) { for (int c = 0; c < 32; ++c) first[qi][c] = 0; continue; }
                    const int32_t p0 = rp[trow[qi]], p1 = rp[trow[qi] + 1];
                    for (int32_t p = p0; p < p1; ++p) cnt[qi][col[p] & 31]++;
                    for (int c = 0; c < 32; ++c) { first[qi][c] = (int32_t)at; at += (size_t)cnt[qi][c]; cnt[qi][c] = 0; }
                    for (int32_t p = p0; p < p1; ++p) { const int c = col[p] & 31; flat[(size_t)first[qi][c] + cnt[qi][c]++] = (uint16_t)col[p]; }
                }
                for (int qi = 0; qi < 16; ++qi) o.tile_rows.push_back(trow[qi]);
                const size_t base = o.ids.size();
                o.ids.resize(base + (size_t)iters * 256, zero_id);
                uint16_t* out_ids = o.ids.data() + base;
                for (int itn = 0; itn < iters; ++itn)
                    for (int s = 0; s < 4; ++s)                               // one LDS instruction: slot s of every lane
                        for (int half = 0; half < 2; ++half) {                // its two access groups: rows 0-7, rows 8-15
                            int32_t open_mask[32];                            // -1: class not used by this access group yet
                            for (int c = 0; c < 32; ++c) open_mask[c] = -1;
                            int rows_by_need[8];
                            for (int k = 0; k < 8; ++k) rows_by_need[k] = half * 8 + k;
                            std::sort(rows_by_need, rows_by_need + 8, [&](int x, int y) { return rem[x] > rem[y]; });
                            const int left = (iters - itn) * 4 - s;           // instructions left, this one included
                            for (int k = 0; k < 8; ++k) {
                                const int qi = rows_by_need[k];
                                int32_t* cq = cnt[qi];
                                for (int jl = 0; jl < 4; ++jl) {
                                    if (rem[qi] == 0) break;
                                    // must this lane take an edge now?  (4 lanes x (left - 1) instructions remain after this one)
                                    const bool must = rem[qi] > (left - 1) * 4 + (3 - jl);
                                    // the fullest open class, the lowest of equals: the largest of (count << 5 | 31 - class)
                                    int32_t bestkey = 0;
                                    for (int c = 0; c < 32; ++c) bestkey = std::max(bestkey, ((cq[c] << 5) | (31 - c)) & open_mask[c]);
                                    int best = bestkey >> 5 ? 31 - (bestkey & 31) : -1;
                                    if (best < 0) {
                                        if (!must) continue;                  // sits this slot out: the zero row
                                        bestkey = 0;
                                        for (int c = 0; c < 32; ++c) bestkey = std::max(bestkey, (cq[c] << 5) | (31 - c));
                                        best = 31 - (bestkey & 31);
                                    }
                                    out_ids[((size_t)itn * 64 + qi * 4 + jl) * 4 + s] = flat[(size_t)first[qi][best] + --cq[best]];
                                    open_mask[best] = 0;
                                    --rem[qi];
                                }
                            }
                        }
                for (int qi = 0; qi < 16; ++qi)
                    if (rem[qi] != 0) o.failed = true;
                o.tile_iters.push_back(iters);
            }
        }
    });
    return built;
}

// The ranges one after the other, every range's tiles cut into the contiguous ranges of its workgroup's waves.  Leaves
// L.failed set when an edge was not scheduled, L.ok unset when the id stream outgrows its 31-bit index.
inline void blocked_concatenate(std::vector<BlockedRange>& built, int64_t N, int R, const std::vector<float>& dis_host, BlockedLayout& L) {
    const uint16_t zero_id = (uint16_t)N;
    std::vector<int32_t> tile_off(1, 0), tile_rows, cell;
    // the ranges' id streams one after the other: sized once, copied on the builder threads (6 MB at pose0-syn; appended
    // range by range on one thread this was a third of the schedule's time)
    std::vector<size_t> ids_first((size_t)R + 1, 0);
    for (int r = 0; r < R; ++r) {
        if (built[r].failed) { L.failed = true; return; }
        ids_first[(size_t)r + 1] = ids_first[(size_t)r] + built[r].ids.size();
    }
    gn::RawVec<uint16_t> ids(ids_first[(size_t)R] + (size_t)kColLayoutSlack * 256);
    std::fill(ids.begin() + (std::ptrdiff_t)ids_first[(size_t)R], ids.end(), zero_id);
    gn::parallel_for(R, 1, [&](int64_t r0, int64_t r1) {
        for (int64_t r = r0; r < r1; ++r)
            if (!built[r].ids.empty()) memcpy(ids.data() + ids_first[(size_t)r], built[r].ids.data(), built[r].ids.size() * sizeof(uint16_t));
    });
    for (int r = 0; r < R; ++r) {
        BlockedRange& o = built[r];
        const int tiles_r = (int)o.tile_iters.size();
        const int first_tile = (int)tile_off.size() - 1;
        for (int tl = 0; tl < tiles_r; ++tl) tile_off.push_back(tile_off.back() + o.tile_iters[tl]);
        tile_rows.insert(tile_rows.end(), o.tile_rows.begin(), o.tile_rows.end());
        // the range's tiles, cut into the contiguous ranges of the workgroup's waves by iterations (+ a cost per tile)
        auto cost_upto = [&](int tl) { return (int64_t)(tile_off[first_tile + tl] - tile_off[first_tile]) + 2 * (int64_t)tl; };
        int wt = 0;
        for (int wv = 0; wv < kColLayoutWaves; ++wv) {
            int wt1 = tiles_r;
            if (wv < kColLayoutWaves - 1) {
                const int64_t goal = cost_upto(tiles_r) * (wv + 1) / kColLayoutWaves;
                wt1 = wt;
                while (wt1 < tiles_r && cost_upto(wt1 + 1) <= goal) ++wt1;
            }
            cell.push_back(first_tile + wt); cell.push_back(first_tile + wt1);
            cell.push_back(tile_off[first_tile + wt]); cell.push_back(tile_off[first_tile + wt1]);
            for (int k = 1; k <= 5; ++k) cell.push_back(tile_off[std::min(first_tile + wt + k, first_tile + tiles_r)]);
            cell.push_back(0); cell.push_back(0); cell.push_back(0);
            wt = wt1;
        }
        o = BlockedRange();
    }
    const int64_t iters_total = tile_off.back();
    for (int k = 0; k < 6; ++k) tile_off.push_back((int32_t)iters_total);
    for (int k = 0; k < 64; ++k) tile_rows.push_back(-1);
    std::vector<float> tile_dis(tile_rows.size(), 0.f);
    for (size_t k = 0; k < tile_rows.size(); ++k)
        if (tile_rows[k] >= 0) tile_dis[k] = dis_host[tile_rows[k]];
    if (ids.size() / 2 >= ((size_t)1 << 31)) return;
    L.iters_total = iters_total;
    L.tile_off.swap(tile_off); L.tile_rows.swap(tile_rows); L.cell.swap(cell); L.tile_dis.swap(tile_dis); L.ids.swap(ids);
    L.ok = true;
}

inline BlockedLayout build_blocked_layout(int64_t N, int R, const std::vector<int32_t>& rp, const std::vector<int32_t>& col,
                                          const std::vector<float>& dis_host) {
    BlockedLayout L;
    GN_LAP(nullptr);
    const std::vector<std::vector<int32_t>> range_rows = blocked_range_rows(N, R, rp);
    GN_LAP("blocked: rows by degree, ranges");
    std::vector<BlockedRange> built = blocked_schedule_ranges(N, R, range_rows, rp, col);
    GN_LAP("blocked: tiles (parallel)");
    blocked_concatenate(built, N, R, dis_host, L);
    GN_LAP("blocked: concatenate");
    return L;
}

}  // namespace gn_layout
