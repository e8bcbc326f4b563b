// Small algorithms that more than one plan layout uses, each written once.  No HIP.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "host_parallel.hpp"

namespace gn_layout {

// The quads of a wave that one ds_read_b128 serves together: four access groups of sixteen lanes (MI355X_MICROARCH.md, LDS).
constexpr int kGroupQuads[4][4] = {{0, 3, 5, 6}, {1, 2, 4, 7}, {8, 11, 13, 14}, {9, 10, 12, 15}};

// A bucket of the dealers: at most 64 entries, no allocation (with std::vector buckets a deal of 64 pairs cost ~50 us -
// sixteen vectors grown by push_back - and the decoder plan of pose0-syn spent 100 ms of eight threads in them).
struct SmallStack {
    int v[64];
    int n = 0;
    void push_back(int x) { v[n++] = x; }
    int back() const { return v[n - 1]; }
    void pop_back() { --n; }
    size_t size() const { return (size_t)n; }
    bool empty() const { return n == 0; }
};

// Whole shares of `total` in proportion to want[0..n) (want[i] = the real-valued share of entry i; an entry that wants
// nothing is not live and gets nothing): every live entry starts at max(min_share, floor(want)), then the largest
// remainders take one more - or the smallest give one back, never below min_share - until the shares add up to `total`
// (the first of equals).  When even min_share for every live entry exceeds `total` the shares stay above it.
inline std::vector<int> largest_remainder_shares(const double* want, int n, int total, int min_share) {
    std::vector<int> share((size_t)n, 0);
    std::vector<double> frac((size_t)n, 0.0);
    int given = 0;
    for (int i = 0; i < n; ++i) {
        if (!(want[i] > 0.0)) continue;
        share[i] = std::max(min_share, (int)want[i]);
        frac[i] = want[i] - share[i];
        given += share[i];
    }
    while (given < total) {
        int best = -1;
        for (int i = 0; i < n; ++i)
            if (want[i] > 0.0 && (best < 0 || frac[i] > frac[best])) best = i;
        if (best < 0) break;
        share[best]++; frac[best] -= 1.0; ++given;
    }
    while (given > total) {
        int best = -1;
        for (int i = 0; i < n; ++i)
            if (share[i] > min_share && (best < 0 || frac[i] < frac[best])) best = i;
        if (best < 0) break;
        share[best]--; frac[best] += 1.0; --given;
    }
    return share;
}

// Contiguous tasks of about equal weight over the items [0, n): a task ends with the item that brings it to `want` (an
// item is never cut).  Returns the first item of every task, then n.
template <typename W>
inline std::vector<int64_t> equal_weight_tasks(int64_t n, W weight_of, int64_t want) {
    std::vector<int64_t> task_first(1, 0);
    int64_t acc = 0;
    for (int64_t i = 0; i < n; ++i) {
        acc += weight_of(i);
        if (acc >= want && i + 1 < n) { task_first.push_back(i + 1); acc = 0; }
    }
    task_first.push_back(n);
    return task_first;
}

// The items [0, n) by cost, largest first, equal costs in index order.
template <typename I, typename C>
inline std::vector<I> descending_order(int64_t n, C cost_of) {
    std::vector<I> order((size_t)n);
    std::iota(order.begin(), order.end(), (I)0);
    std::stable_sort(order.begin(), order.end(), [&](I x, I y) { return cost_of(x) > cost_of(y); });
    return order;
}

// The table the decoder's pairing passes keep their open triples in: open addressing on a power-of-two table (keys are
// unique per open triple; a closed slot keeps its key with value -1 so that probe chains stay intact).  A pass that
// reuses the table wipes it by the slots it touched.
struct PairingTable {
    static constexpr uint64_t kEmpty = ~(uint64_t)0;
    std::vector<uint64_t> keys;
    std::vector<int64_t> vals;
    std::vector<uint32_t> touched;
    size_t mask = 0;
    // a clean table for up to `count` entries (at most half full)
    void open(size_t count) {
        size_t cap = 16;
        while (cap < count * 2 + 16) cap <<= 1;
        if (keys.size() < cap) { keys.assign(cap, kEmpty); vals.assign(cap, -1); }
        mask = cap - 1;
        touched.clear();
    }
    // the open entry of `key` (which is closed by this), or -1: `e` is the first (or third, fifth, ...) copy and stays open
    int64_t pair_up(uint64_t key, int64_t e) {
        size_t h = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & mask;
        while (keys[h] != kEmpty && keys[h] != key) h = (h + 1) & mask;
        if (keys[h] == key && vals[h] >= 0) {
            const int64_t first = vals[h];
            vals[h] = -1;
            return first;
        }
        if (keys[h] != key) touched.push_back((uint32_t)h);
        keys[h] = key;
        vals[h] = e;
        return -1;
    }
    void wipe() {
        for (uint32_t h : touched) { keys[h] = kEmpty; vals[h] = -1; }
        touched.clear();
    }
};

}  // namespace gn_layout
