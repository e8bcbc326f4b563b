// Runs the pure host-side layout code of the plan builders (gripnet_amd/csrc/host_layout.hpp, the umbrella over
// host_parallel.hpp, layout_util.hpp and one layout_*.hpp per plan) on random inputs, once on one
// builder thread and once on sixteen, under the sanitizer this file was compiled with (make -C gripnet_amd/csrc SAN=asan
// or SAN=tsan; tests/test_host_layout.py builds and runs both).  Checks that every edge lands in exactly one slot and that
// a plan does not depend on the thread count.  No HIP, no GPU.
// `digest` as the first argument prints an FNV-1a hash of every output array of every case instead, on 1 and on 16 threads:
// two trees lay out the same plans when the program, built against each tree's host_layout.hpp, prints the same lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <initializer_list>
#include <random>
#include <thread>
#include <utility>

#include <sys/wait.h>
#include <unistd.h>

#include "host_layout.hpp"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); std::exit(1); } \
    } while (0)

namespace {

void set_threads(int n) {
    char buf[16];
    std::snprintf(buf, sizeof buf, "%d", n);
    setenv("GN_PLAN_THREADS", buf, 1);
}

// ---- digest mode -----------------------------------------------------------------------------------------------------
bool g_digest = false;

template <typename V>
uint64_t fnv(const V& v) {
    uint64_t h = 1469598103934665603ull;
    for (const auto& x : v) h = (h ^ (uint64_t)x) * 1099511628211ull;
    return h;
}

void emit(const char* name, std::initializer_list<uint64_t> hashes) {
    if (!g_digest) return;
    std::printf("%s", name);
    for (uint64_t h : hashes) std::printf(" %016llx", (unsigned long long)h);
    std::printf("\n");
}

// ---- decoder: pairing + row classes ------------------------------------------------------------------------------------
// a bidirectional list of R relations, relation r with e_dir / (r + 1) random pairs
void decoder_list(int64_t n, int R, int64_t e_dir, unsigned seed, std::vector<int64_t>& hu, std::vector<int64_t>& hv, std::vector<int64_t>& hr) {
    std::mt19937_64 rng(seed);
    for (int r = 0; r < R; ++r) {
        const int64_t cnt = std::max<int64_t>(1, e_dir / (r + 1));
        std::vector<int64_t> u(cnt), v(cnt);
        for (int64_t k = 0; k < cnt; ++k) { u[k] = (int64_t)(rng() % (uint64_t)n); v[k] = (int64_t)(rng() % (uint64_t)n); }
        for (int64_t k = 0; k < cnt; ++k) { hu.push_back(u[k]); hv.push_back(v[k]); hr.push_back(r); }
        for (int64_t k = 0; k < cnt; ++k) { hu.push_back(v[k]); hv.push_back(u[k]); hr.push_back(r); }   // to_bidirection
    }
}

gn_layout::ClassLayout decoder_case(int64_t n, int R, int64_t e_dir, int64_t features, unsigned seed, bool check,
                                   int64_t window_bytes = gn_layout::kClsWindowBytes, bool expect_ok = true) {
    std::vector<int64_t> hu, hv, hr;
    decoder_list(n, R, e_dir, seed, hu, hv, hr);
    const int64_t E = (int64_t)hu.size();
    gn::RawVec<int64_t> mirror_of;
    gn::RawVec<char> covered;
    gn_layout::pair_mirrors(hu, hv, hr, 13, mirror_of, covered);
    const gn::RawVec<int64_t> scored = gn_layout::scored_edges(covered);
    gn_layout::ClassLayout L = gn_layout::build_class_layout(hu, hv, hr, scored, mirror_of, n, features, 256, window_bytes);
    if (!check) return L;
    if (!expect_ok) { CHECK(!L.ok); return L; }             // (a list the row-class kernel does not take: the column-phase kernel serves it)
    CHECK(L.ok);
    // every edge position is written exactly once: as a scored pair's own position or as its mirror
    std::vector<int> seen((size_t)E, 0);
    for (size_t s = 0; s < (size_t)L.batches * 64; ++s) {
        if (L.own[s] != gn_layout::kNoMirror) { CHECK(L.own[s] < (uint32_t)E); seen[L.own[s]]++; }
        else CHECK(L.mirror[s] == gn_layout::kNoMirror);
        if (L.mirror[s] != gn_layout::kNoMirror) { CHECK(L.mirror[s] < (uint32_t)E); seen[L.mirror[s]]++; }
    }
    for (int64_t e = 0; e < E; ++e) CHECK(seen[e] == 1);
    // workgroups: contiguous batch ranges that together tile [0, batches) (with eight position parts workgroup 8 l + x is
    // the l-th of part x, so they are not in index order); local rows inside the class's rows; relations inside the D cache
    std::vector<std::pair<int64_t, int64_t>> ranges;
    CHECK(L.walks >= 1 && L.walks <= gn_layout::kClsMaxWalks);
    for (int g = 0; g < L.groups; ++g) {
        const int32_t* h = L.wg.data() + (size_t)g * (4 + 4 * L.walks);
        const int rows = h[1] + h[3];
        for (int wk = 0; wk < L.walks; ++wk) {                  // a workgroup's batch range of every walk of its position range
            const int32_t* d = h + 4 * wk;
            CHECK(d[5] >= d[4] && d[4] >= 0 && d[5] <= L.batches);
            if (d[5] > d[4]) ranges.push_back({d[4], d[5]});
            CHECK(d[7] >= 1 && d[7] <= gn_layout::kClsDCache);
            for (int64_t b = d[4]; b < d[5]; ++b) {
                for (int s = 0; s < 64; ++s) {
                    const uint32_t w = L.packed[(size_t)b * 64 + s];
                    CHECK((int)(w & 0xffffu) < rows && (int)(w >> 16) < rows);
                }
                for (int k = 0; k < 4; ++k) {
                    const uint32_t word = L.rel32[(size_t)b * 2 + (k >> 1)];
                    const int rel = (int)((k & 1) ? word >> 16 : word & 0xffffu);
                    CHECK(rel >= d[6] && rel < d[6] + d[7]);
                }
            }
        }
    }
    std::sort(ranges.begin(), ranges.end());
    int64_t at = 0;
    for (auto& r : ranges) { CHECK(r.first == at); at = r.second; }
    CHECK(at == L.batches);
    // eight position ranges, three classes: the parts are cut by batches and the free pairs dealt so that no workgroup is far
    // above the mean (a wave takes whole batches: one batch too many in a workgroup is one more trip for the whole launch)
    if (L.groups == 256 && n > 512 && L.batches >= 256 * 32) {
        int64_t most = 0;
        for (int g = 0; g < L.groups; ++g) {
            const int32_t* h = L.wg.data() + (size_t)g * (4 + 4 * L.walks);
            int64_t nb = 0;
            for (int wk = 0; wk < L.walks; ++wk) nb += h[5 + 4 * wk] - h[4 + 4 * wk];
            most = std::max(most, nb);
        }
        CHECK(most * L.groups <= L.batches + 3 * L.groups + L.batches / 50);
    }
    return L;
}

// ---- decoder: column-phase batches ------------------------------------------------------------------------------------------
#if __has_include("layout_decoder.hpp")
using gn_layout::PhaseLayout;
using gn_layout::build_phase_layout;
#else
// (a tree from before build_phase_layout: the same loop as it stood in build_distmult_plan, for the digest comparison)
struct PhaseLayout {
    std::vector<uint32_t> packed, own, mirror;
    std::vector<int32_t> batch_rel;
    std::vector<uint16_t> rel16;
};
template <typename V>
PhaseLayout build_phase_layout(const V& hu, const V& hv, const V& hr, const gn::RawVec<int64_t>& scored,
                               const gn::RawVec<int64_t>& mirror_of, int node_bits) {
    const int kNodeBits = node_bits;
    const uint32_t kNoMirror = gn_layout::kNoMirror;
    const int64_t NBs = gn::ceil_div((int64_t)scored.size(), 64);
    std::vector<uint32_t> packed((size_t)NBs * 64), own((size_t)NBs * 64), mirror((size_t)NBs * 64);
    std::vector<int32_t> batch_rel((size_t)NBs);
    std::vector<uint16_t> rel16((size_t)NBs * 64);
    gn::parallel_for(NBs, 64, [&](int64_t b0, int64_t b1) {
        int slot_of_edge[64];
        int64_t cu[64], cv[64], ce[64];
        for (int64_t bi = b0; bi < b1; ++bi) {
            const int count = (int)std::min<int64_t>(64, (int64_t)scored.size() - bi * 64);
            for (int k = 0; k < count; ++k) { ce[k] = scored[bi * 64 + k]; cu[k] = hu[ce[k]]; cv[k] = hv[ce[k]]; }
            gn_layout::deal_batch(cu, cv, count, slot_of_edge);
            bool uniform = true;
            for (int k = 1; k < count; ++k) uniform = uniform && hr[ce[k]] == hr[ce[0]];
            const size_t s0 = (size_t)bi * 64;
            batch_rel[bi] = uniform ? (int32_t)hr[ce[0]] : -1;
            bool taken[64] = {false};
            auto fill = [&](int s, int k) {
                const int64_t e = ce[k];
                packed[s0 + s] = (uint32_t)hu[e] | ((uint32_t)hv[e] << kNodeBits);
                own[s0 + s] = (uint32_t)e;
                rel16[s0 + s] = (uint16_t)hr[e];
                mirror[s0 + s] = mirror_of[e] >= 0 ? (uint32_t)mirror_of[e] : kNoMirror;
            };
            for (int k = 0; k < count; ++k) { taken[slot_of_edge[k]] = true; fill(slot_of_edge[k], k); }
            for (int s = 0; s < 64; ++s)
                if (!taken[s]) fill(s, 0);
        }
    });
    PhaseLayout L;
    L.packed.swap(packed); L.own.swap(own); L.mirror.swap(mirror); L.batch_rel.swap(batch_rel); L.rel16.swap(rel16);
    return L;
}
#endif

// Every position of the list is written exactly once, as a scored edge's own position or as its mirror (the empty slots of
// a ragged last batch repeat the batch's first edge: the same score into the same positions); a batch's relation is -1 or
// that of all its slots.  `slots`: deal_batch over the same batches, on its own.
PhaseLayout phase_case(int64_t n, int R, int64_t e_dir, unsigned seed, std::vector<int>& slots) {
    std::vector<int64_t> hu, hv, hr;
    decoder_list(n, R, e_dir, seed, hu, hv, hr);
    const int64_t E = (int64_t)hu.size();
    gn::RawVec<int64_t> mirror_of;
    gn::RawVec<char> covered;
    gn_layout::pair_mirrors(hu, hv, hr, 13, mirror_of, covered);
    const gn::RawVec<int64_t> scored = gn_layout::scored_edges(covered);
    const int64_t S = (int64_t)scored.size(), NB = gn::ceil_div(S, 64);
    slots.assign((size_t)NB * 64, -1);
    for (int64_t b = 0; b < NB; ++b) {
        int64_t cu[64], cv[64];
        const int count = (int)std::min<int64_t>(64, S - b * 64);
        for (int k = 0; k < count; ++k) { cu[k] = hu[scored[b * 64 + k]]; cv[k] = hv[scored[b * 64 + k]]; }
        gn_layout::deal_batch(cu, cv, count, slots.data() + b * 64);
        bool used[64] = {false};
        for (int k = 0; k < count; ++k) { CHECK(slots[b * 64 + k] >= 0 && slots[b * 64 + k] < 64 && !used[slots[b * 64 + k]]); used[slots[b * 64 + k]] = true; }
    }
    const PhaseLayout L = build_phase_layout(hu, hv, hr, scored, mirror_of, 13);
    CHECK((int64_t)L.batch_rel.size() == NB && L.packed.size() == (size_t)NB * 64 && L.own.size() == (size_t)NB * 64 &&
          L.mirror.size() == (size_t)NB * 64 && L.rel16.size() == (size_t)NB * 64);
    std::vector<int> written((size_t)E, 0), slots_of((size_t)E, 0);
    for (int64_t b = 0; b < NB; ++b)
        for (int s = 0; s < 64; ++s) {
            const size_t at = (size_t)b * 64 + s;
            const uint32_t e = L.own[at];
            CHECK(e < (uint32_t)E && !covered[e]);
            CHECK(L.packed[at] == ((uint32_t)hu[e] | (uint32_t)hv[e] << 13) && L.rel16[at] == (uint16_t)hr[e]);
            CHECK(L.mirror[at] == (mirror_of[e] >= 0 ? (uint32_t)mirror_of[e] : gn_layout::kNoMirror));
            CHECK(L.batch_rel[b] == -1 || L.batch_rel[b] == (int32_t)L.rel16[at]);
            if (slots_of[e]++ > 0) { CHECK(b == NB - 1 && (int64_t)e == scored[(size_t)b * 64]); continue; }   // (an empty slot of the ragged batch)
            written[e]++;
            if (L.mirror[at] != gn_layout::kNoMirror) { CHECK(L.mirror[at] < (uint32_t)E); written[L.mirror[at]]++; }
        }
    for (int64_t e = 0; e < E; ++e) CHECK(written[e] == 1);
    int64_t repeats = 0;
    for (int64_t e = 0; e < E; ++e) repeats += std::max(0, slots_of[e] - 1);
    CHECK(repeats == NB * 64 - S);
    return L;
}

#if __has_include("layout_util.hpp")
// largest_remainder_shares: the shares add up to the total, every live entry has its minimum, and an input whose minimum
// shares already exceed the total ends (nobody can give one back) with the minimum for everybody.
void shares_case() {
    const double want[4] = {5.3, 0.0, 2.9, 7.8};
    const std::vector<int> a = gn_layout::largest_remainder_shares(want, 4, 16, 1);
    CHECK(a.size() == 4 && a[0] + a[1] + a[2] + a[3] == 16 && a[1] == 0 && a[0] >= 5 && a[2] >= 2 && a[3] >= 7);
    const double skew[3] = {15.9, 0.05, 0.05};                    // the minimum of the small ones comes out of the large one
    const std::vector<int> b = gn_layout::largest_remainder_shares(skew, 3, 16, 1);
    CHECK(b[0] + b[1] + b[2] == 16 && b[1] >= 1 && b[2] >= 1);
    const double tight[3] = {0.7, 0.7, 0.6};                     // three live entries, two to give: 1 + 1 + 1 > 2 and every share is 1
    const std::vector<int> c = gn_layout::largest_remainder_shares(tight, 3, 2, 1);
    CHECK(c[0] == 1 && c[1] == 1 && c[2] == 1);
    const std::vector<int> none = gn_layout::largest_remainder_shares(want, 0, 16, 1);
    CHECK(none.empty());
    const double dead[2] = {0.0, 0.0};                           // nobody to give to
    const std::vector<int> d = gn_layout::largest_remainder_shares(dead, 2, 4, 1);
    CHECK(d[0] == 0 && d[1] == 0);
}
#else
void shares_case() {}
#endif

// ---- relational layer: destination-major streams --------------------------------------------------------------------------
gn_layout::PairLayout pair_case(int64_t N, int64_t R, int64_t E, unsigned seed, bool check) {
    std::mt19937_64 rng(seed);
    const int cus = 256;
    const int chunks = (int)gn::ceil_div(N, 32), kpad = chunks * 32;
    const int D = (int)gn::ceil_div(N, cus), G = (int)std::min<int64_t>(N, cus);
    std::vector<int64_t> src((size_t)E), dst((size_t)E);
    std::vector<uint32_t> rel((size_t)E);
    std::vector<int32_t> outdeg((size_t)N, 0);
    for (int64_t e = 0; e < E; ++e) {
        src[e] = (int64_t)(rng() % (uint64_t)N);
        dst[e] = (int64_t)((rng() % (uint64_t)N) * (rng() % 3 ? 1 : 0));   // a third of the edges into node 0: a hub, runs longer than one unit
        rel[e] = (uint32_t)(rng() % (uint64_t)R);
        outdeg[src[e]]++;
    }
    std::vector<int32_t> order((size_t)N), perm((size_t)kpad, (int32_t)N), kpos((size_t)N);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return outdeg[x] > outdeg[y]; });
    for (int64_t k = 0; k < N; ++k) { perm[k] = order[k]; kpos[order[k]] = (int32_t)k; }
    std::vector<int64_t> idx((size_t)E);
    std::iota(idx.begin(), idx.end(), 0);
    auto key = [&](int64_t e) { return dst[e] * kpad + kpos[src[e]]; };
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return key(x) < key(y); });
    std::vector<int32_t> rp((size_t)N * kpad + 1, 0);
    std::vector<uint32_t> rels((size_t)E);
    for (int64_t i = 0; i < E; ++i) { rels[i] = rel[idx[i]]; rp[key(idx[i]) + 1]++; }
    for (size_t i = 1; i < rp.size(); ++i) rp[i] += rp[i - 1];
    gn_layout::PairLayout L = gn_layout::build_pair_layout(N, R, chunks, kpad, G, D, rp, rels, perm);
    if (!check) return L;
    CHECK(L.ok);
    // every edge is one stream word that names a real att row; everything else names one of the two zero rows
    int64_t real = 0;
    std::vector<int64_t> per_rel((size_t)R, 0), want((size_t)R, 0);
    for (size_t i = 0; i < (size_t)L.blocks * 16; ++i) {
        const uint32_t row = L.stream[i] / gn_layout::kPairRowBytes;
        CHECK(L.stream[i] % gn_layout::kPairRowBytes == 0 && row <= (uint32_t)R + 1);
        if (row < (uint32_t)R) { ++real; per_rel[row]++; }
    }
    for (int64_t e = 0; e < E; ++e) want[rel[e]]++;
    CHECK(real == E);
    for (int64_t r = 0; r < R; ++r) CHECK(per_rel[r] == want[r]);
    // every destination row belongs to exactly one workgroup
    std::vector<int> owner((size_t)N, 0);
    for (int g = 0; g < G; ++g)
        for (int d = 0; d < 3; ++d)
            if (L.wg_dst[(size_t)g * 4 + d] >= 0) owner[L.wg_dst[(size_t)g * 4 + d]]++;
    for (int64_t i = 0; i < N; ++i) CHECK(owner[i] == 1);
    return L;
}

// ---- relational layer: LDS-accumulator work items ----------------------------------------------------------------------------
#if __has_include("layout_rgcn_fast.hpp")
using gn_layout::FastItems;
using gn_layout::FastWork;
using gn_layout::build_fast_items;
using gn_layout::build_fast_work;
using gn_layout::kFastItemEdges;
using gn_layout::kFastItemOverhead;
#else
// (a tree from before layout_rgcn_fast.hpp: the same loops as they stood in gn_rgcn_build_fast_segments, for the digest comparison)
constexpr int kFastItemEdges = 4096 - 3 * 128, kFastItemOverhead = 2048;
struct FastItems {
    std::vector<int32_t> item_rel, item_tile, item_begin, piece_first, piece_group;
    int groups = 0;
    int n_items() const { return (int)item_rel.size(); }
    int n_pieces() const { return (int)piece_group.size(); }
    int64_t piece_cost(int pc) const { return (int64_t)kFastItemOverhead + (item_begin[piece_first[pc + 1]] - item_begin[piece_first[pc]]); }
};
struct FastWork { std::vector<int32_t> wg_begin, desc; };
FastItems build_fast_items(const std::vector<int32_t>& seg, int tiles, int64_t E) {
    const int kGroups = 256, kItemEdges = kFastItemEdges, kItemOverhead = kFastItemOverhead;
    const int n_seg = (int)seg.size() - 1;
    FastItems L;
    std::vector<int32_t>&item_rel = L.item_rel, &item_tile = L.item_tile, &item_begin = L.item_begin;
    for (int sg = 0; sg < n_seg; ++sg) {
        for (int32_t b = seg[sg]; b < seg[sg + 1]; b += kItemEdges) {
            item_rel.push_back(sg / tiles);
            item_tile.push_back(sg % tiles);
            item_begin.push_back(b);
        }
    }
    const int n_items = (int)item_rel.size();
    item_begin.push_back((int32_t)E);
    int64_t total_cost = 0;
    for (int sg = 0; sg < n_seg; ++sg)
        if (seg[sg + 1] > seg[sg]) total_cost += kItemOverhead + (seg[sg + 1] - seg[sg]);
    const int groups0 = std::min(kGroups, std::max(n_items, 1));
    const int64_t piece_cap = std::max<int64_t>(kItemOverhead + kItemEdges, total_cost / groups0 / 4);
    const int piece_chunks = (int)std::max<int64_t>(1, (piece_cap - kItemOverhead) / kItemEdges);
    std::vector<int32_t> piece_first, piece_count;
    std::vector<int64_t> piece_cost;
    for (int i = 0; i < n_items;) {
        int jn = i + 1;
        while (jn < n_items && jn - i < piece_chunks && item_rel[jn] == item_rel[i] && item_tile[jn] == item_tile[i]) ++jn;
        piece_first.push_back(i);
        piece_count.push_back(jn - i);
        piece_cost.push_back((int64_t)kItemOverhead + (item_begin[jn] - item_begin[i]));
        i = jn;
    }
    const int n_pieces = (int)piece_first.size();
    const int groups = std::min(groups0, std::max(n_pieces, 1));
    const std::vector<int> order = gn_layout::descending_order<int>(n_pieces, [&](int x) { return piece_cost[x]; });
    L.piece_group.assign((size_t)n_pieces, 0);
    {
        std::vector<std::pair<int64_t, int>> heap;   // min-heap over (load, group)
        for (int gidx = 0; gidx < groups; ++gidx) heap.emplace_back(0, gidx);
        auto cmp = [](const std::pair<int64_t, int>& x, const std::pair<int64_t, int>& y) { return x > y; };
        std::make_heap(heap.begin(), heap.end(), cmp);
        for (int pc : order) {
            std::pop_heap(heap.begin(), heap.end(), cmp);
            auto& top = heap.back();
            L.piece_group[pc] = top.second;
            top.first += piece_cost[pc];
            std::push_heap(heap.begin(), heap.end(), cmp);
        }
    }
    L.piece_first = piece_first;
    L.piece_first.push_back(n_items);
    L.groups = groups;
    return L;
}
FastWork build_fast_work(const FastItems& L, const std::vector<int32_t>& item_pad) {
    const int groups = L.groups;
    std::vector<std::vector<int32_t>> bins(groups);
    for (int pc = 0; pc < L.n_pieces(); ++pc)
        for (int32_t it = L.piece_first[pc]; it < L.piece_first[pc + 1]; ++it) bins[L.piece_group[pc]].push_back(it);
    FastWork W;
    W.wg_begin.assign((size_t)groups + 1, 0);
    for (int gidx = 0; gidx < groups; ++gidx) {
        std::sort(bins[gidx].begin(), bins[gidx].end(), [&](int32_t x, int32_t y) {
            return L.item_tile[x] != L.item_tile[y] ? L.item_tile[x] < L.item_tile[y] : x < y;
        });
        for (int32_t it : bins[gidx]) {
            const int32_t w[8] = {L.item_rel[it], L.item_tile[it], item_pad[it], item_pad[it + 1] - item_pad[it], it, 0, 0, 0};
            W.desc.insert(W.desc.end(), w, w + 8);
        }
        W.wg_begin[gidx + 1] = (int32_t)(W.desc.size() / 8);
    }
    return W;
}
#endif

// R x tiles segments over E sorted edges (a hub relation, empty segments), the items' padded offsets as the device scan would
// give them.  Every item sits in exactly one workgroup; the workgroups' loads differ by at most the largest piece (each piece
// went to the least loaded one); a workgroup's descriptors are sorted by tile, then item, and name their item's words.
std::pair<FastItems, FastWork> fast_case(int64_t R, int tiles, int64_t E, unsigned seed) {
    std::mt19937_64 rng(seed);
    const int n_seg = (int)(R * tiles);
    std::vector<int32_t> seg((size_t)n_seg + 1, 0);
    for (int64_t e = 0; e < E; ++e) {
        const int64_t sg = e < E / 3 ? (int64_t)(rng() % (uint64_t)tiles) : (int64_t)(rng() % (uint64_t)n_seg);   // relation 0 is a hub
        if (sg % 7 != 3 || n_seg < 8) seg[(size_t)sg + 1]++; else seg[1]++;                                     // (empty segments)
    }
    for (int sg = 0; sg < n_seg; ++sg) seg[(size_t)sg + 1] += seg[(size_t)sg];
    CHECK(seg[(size_t)n_seg] == E);
    const FastItems L = build_fast_items(seg, tiles, E);
    const int n_items = L.n_items(), n_pieces = L.n_pieces();
    CHECK((int)L.item_begin.size() == n_items + 1 && L.item_begin[(size_t)n_items] == E && (int)L.piece_first.size() == n_pieces + 1);
    CHECK(L.groups >= 1 && L.groups <= 256 && L.groups <= std::max(n_pieces, 1));
    for (int i = 0; i < n_items; ++i) {
        const int sg = L.item_rel[i] * tiles + L.item_tile[i];
        const int32_t len = L.item_begin[(size_t)i + 1] - L.item_begin[i];
        CHECK(L.item_tile[i] >= 0 && L.item_tile[i] < tiles && L.item_rel[i] >= 0 && L.item_rel[i] < R);
        CHECK(len >= 1 && len <= kFastItemEdges && L.item_begin[i] >= seg[sg] && L.item_begin[(size_t)i + 1] <= seg[(size_t)sg + 1]);
    }
    // pieces: consecutive items of one segment; loads: the least loaded workgroup took every piece in turn
    std::vector<int64_t> load((size_t)L.groups, 0);
    int64_t largest = 0;
    CHECK(L.piece_first[0] == 0 && L.piece_first[(size_t)n_pieces] == n_items);
    for (int pc = 0; pc < n_pieces; ++pc) {
        CHECK(L.piece_first[(size_t)pc + 1] > L.piece_first[pc] && L.piece_group[pc] >= 0 && L.piece_group[pc] < L.groups);
        for (int32_t it = L.piece_first[pc]; it < L.piece_first[(size_t)pc + 1]; ++it)
            CHECK(L.item_rel[it] == L.item_rel[L.piece_first[pc]] && L.item_tile[it] == L.item_tile[L.piece_first[pc]]);
        load[(size_t)L.piece_group[pc]] += L.piece_cost(pc);
        largest = std::max(largest, L.piece_cost(pc));
    }
    if (n_pieces > 0) CHECK(*std::max_element(load.begin(), load.end()) - *std::min_element(load.begin(), load.end()) <= largest);
    std::vector<int32_t> item_pad((size_t)n_items + 1, 0);
    for (int i = 0; i < n_items; ++i)
        item_pad[(size_t)i + 1] = item_pad[i] + ((L.item_begin[(size_t)i + 1] - L.item_begin[i] + 3 * (int32_t)(rng() % 128) + 3) & ~3);
    const FastWork W = build_fast_work(L, item_pad);
    CHECK((int)W.wg_begin.size() == L.groups + 1 && W.wg_begin[0] == 0 && W.wg_begin[(size_t)L.groups] == n_items && W.desc.size() == (size_t)n_items * 8);
    std::vector<int> seen((size_t)n_items, 0);
    for (int g = 0; g < L.groups; ++g)
        for (int32_t k = W.wg_begin[g]; k < W.wg_begin[(size_t)g + 1]; ++k) {
            const int32_t* d = W.desc.data() + (size_t)k * 8;
            const int32_t it = d[4];
            CHECK(it >= 0 && it < n_items);
            seen[it]++;
            CHECK(d[0] == L.item_rel[it] && d[1] == L.item_tile[it] && d[2] == item_pad[it] && d[3] == item_pad[(size_t)it + 1] - item_pad[it]);
            CHECK(d[5] == 0 && d[6] == 0 && d[7] == 0);
            if (k > W.wg_begin[g]) CHECK(d[-7] < d[1] || (d[-7] == d[1] && d[-4] < d[4]));      // by tile, then item
        }
    for (int i = 0; i < n_items; ++i) CHECK(seen[i] == 1);
    return {L, W};
}

// ---- gene layers: LDS-staged gather ----------------------------------------------------------------------------------------
gn_layout::BlockedLayout blocked_case(int64_t N, int deg, int R, unsigned seed, bool check) {
    std::mt19937_64 rng(seed);
    std::vector<int32_t> rp((size_t)N + 1, 0), col;
    for (int64_t i = 0; i < N; ++i) {
        const int d = 1 + (int)(rng() % (uint64_t)(2 * deg));
        for (int k = 0; k < d; ++k) col.push_back((int32_t)(rng() % (uint64_t)N));
        rp[i + 1] = (int32_t)col.size();
    }
    std::vector<float> dis((size_t)N + 64, 0.f);
    for (int64_t i = 0; i < N; ++i) dis[i] = 1.0f / std::sqrt((float)(rp[i + 1] - rp[i]));
    gn_layout::BlockedLayout L = gn_layout::build_blocked_layout(N, R, rp, col, dis);
    if (!check) return L;
    CHECK(L.ok && !L.failed);
    int64_t real = 0;
    for (uint16_t id : L.ids) real += id != (uint16_t)N;
    CHECK(real == (int64_t)col.size());
    std::vector<int> seen((size_t)N, 0);
    for (int32_t r : L.tile_rows)
        if (r >= 0) seen[r]++;
    for (int64_t i = 0; i < N; ++i) CHECK(seen[i] == 1);
    return L;
}

// ---- relational weight gradient: units of four chunks of (relation, source) rows -----------------------------------------
gn_layout::RelGradLayout rel_grad_case(int64_t n, int64_t R, int64_t E, int groups, unsigned seed, bool check) {
    std::mt19937_64 rng(seed);
    // (relation, source)-major CSR with a hub relation (a quarter of the edges), empty relations and empty rows
    std::vector<std::vector<int32_t>> rows((size_t)(R * n));
    for (int64_t e = 0; e < E; ++e) {
        int64_t r = (e % 4 == 0) ? 0 : (int64_t)(rng() % (uint64_t)R);
        if (R > 3 && r == 2) r = 3;                                       // relation 2 stays empty
        rows[(size_t)(r * n + (int64_t)(rng() % (uint64_t)n))].push_back((int32_t)(rng() % (uint64_t)n));
    }
    std::vector<int32_t> rp((size_t)(R * n) + 1, 0), col;
    for (size_t k = 0; k < rows.size(); ++k) { col.insert(col.end(), rows[k].begin(), rows[k].end()); rp[k + 1] = (int32_t)col.size(); }
    gn_layout::RelGradLayout L = gn_layout::build_rel_grad_layout(rp.data(), col.data(), n, R, groups);
    if (!check) return L;
    CHECK(L.ok && L.groups == groups);
    const size_t entries = L.entry.size() / 4;
    CHECK(L.wg_off.size() == (size_t)groups + 1 && (size_t)L.wg_off.back() == entries && L.wave_cnt.size() == entries * gn_layout::kRelWaves);
    // every wave's units are one contiguous run, in workgroup / wave / entry order, a multiple of the ring depth per entry
    int64_t u = 0;
    std::vector<int64_t> got((size_t)(R * n), 0);                         // edges found per (relation, source) row
    std::vector<int> parts_seen((size_t)R, 0);
    for (int g = 0; g < groups; ++g)
        for (int w = 0; w < gn_layout::kRelWaves; ++w) {
            CHECK(L.wave_u0[(size_t)g * gn_layout::kRelWaves + w] == u);
            for (int e = L.wg_off[g]; e < L.wg_off[g + 1]; ++e) {
                const int rel = L.entry[4 * (size_t)e], cnt = L.wave_cnt[(size_t)e * gn_layout::kRelWaves + w];
                CHECK(rel >= 0 && rel < R && cnt % gn_layout::kRelRing == 0);
                if (w == 0) parts_seen[(size_t)rel]++;
                for (int k = 0; k < cnt; ++k, ++u)
                    for (int lg = 0; lg < 4; ++lg) {
                        const uint16_t s = L.src[(size_t)u * 4 + lg];
                        for (int t = 0; t < gn_layout::kRelChunk; ++t) {
                            const uint16_t d = L.ids[((size_t)u * 4 + lg) * gn_layout::kRelChunk + t];
                            if (s == gn_layout::kRelNoSource) { CHECK(d == (uint16_t)n); continue; }
                            CHECK(s < n && d <= n);
                            if (d < n) got[(size_t)(rel * n + s)]++;
                        }
                    }
            }
        }
    CHECK(u == L.units && L.src.size() == (size_t)(u + gn_layout::kRelSlackUnits) * 4);
    for (size_t k = 0; k < got.size(); ++k) CHECK(got[k] == rp[k + 1] - rp[k]);
    // every relation is listed, all its parts exactly once, and the parts' scratch slots do not overlap
    int slots = 0;
    for (int64_t r = 0; r < R; ++r) CHECK(parts_seen[(size_t)r] >= 1);
    for (size_t e = 0; e < entries; ++e) {
        const int rel = L.entry[4 * e], parts = L.entry[4 * e + 1], index = L.entry[4 * e + 2], slot0 = L.entry[4 * e + 3];
        CHECK(parts == parts_seen[(size_t)rel] && index >= 0 && index < parts);
        if (parts > 1) { CHECK(slot0 >= 0 && slot0 + parts <= L.scratch_slots); if (index == 0) slots += parts; }
    }
    CHECK(slots == L.scratch_slots);
    return L;
}

template <typename V>
bool same(const V& a, const V& b) { return a == b; }

}  // namespace

// balance_batch64: a permutation of the batch, never more access cycles than the input order, close to the 32 of a perfect split
void balance_case(unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<int> all_orders;
    for (int round = 0; round < 200; ++round) {
        uint8_t cls[64];
        const int skew = round % 5;                      // 0: uniform classes; else: one class rare / absent
        for (int i = 0; i < 64; ++i) {
            int c = (int)(rng() % 16);
            if (skew == 1 && (c & 3) == 3) c &= 12;
            if (skew == 2) c &= 5;
            if (skew == 3) c = 6;
            cls[i] = (uint8_t)c;
        }
        int order[64], ident[64];
        for (int i = 0; i < 64; ++i) { order[i] = -1; ident[i] = i; }
        gn_layout::balance_batch64(cls, order);
        all_orders.insert(all_orders.end(), order, order + 64);
        bool seen[64] = {false};
        for (int i = 0; i < 64; ++i) {
            if (order[i] < 0 || order[i] >= 64 || seen[order[i]]) { std::fprintf(stderr, "balance_batch64: not a permutation\n"); std::exit(1); }
            seen[order[i]] = true;
        }
        const int before = gn_layout::batch64_access_cycles(cls, ident), after = gn_layout::batch64_access_cycles(cls, order);
        if (round < 5 && seed == 5 && !g_digest) std::printf("balance_batch64 (class mix %d): %d -> %d LDS cycles per batch (32 = no conflict)\n", skew, before, after);
        if (after > before || (skew == 0 && after > 56)) {
            std::fprintf(stderr, "balance_batch64: %d -> %d cycles (round %d)\n", before, after, round);
            std::exit(1);
        }
    }
    emit("balance_batch64", {fnv(all_orders)});
}

// ---- relational layer of any size: degree order, weight-gradient items ----------------------------------------------------------
void general_case(int64_t N, int64_t R, int64_t E, unsigned seed) {
    std::mt19937_64 rng(seed);
    std::vector<int32_t> rp((size_t)N + 1, 0);
    for (int64_t e = 0; e < E; ++e) rp[(size_t)(1 + (e < E / 3 ? e % std::max<int64_t>(1, N / 50) : (int64_t)(rng() % (uint64_t)N)))]++;   // a few hub rows
    for (int64_t i = 0; i < N; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
    std::vector<int32_t> order;
    int64_t heavy = -1;
    gn_layout::degree_order(rp, order, heavy);
    CHECK((int64_t)order.size() == N);
    std::vector<char> seen((size_t)N, 0);
    int64_t heavy_ref = 0;
    for (int64_t i = 0; i < N; ++i) {
        CHECK(order[(size_t)i] >= 0 && order[(size_t)i] < N && !seen[(size_t)order[(size_t)i]]);
        seen[(size_t)order[(size_t)i]] = 1;
        const int64_t d = rp[(size_t)order[(size_t)i] + 1] - rp[(size_t)order[(size_t)i]];
        if (i > 0) {
            const int64_t dp = rp[(size_t)order[(size_t)i - 1] + 1] - rp[(size_t)order[(size_t)i - 1]];
            CHECK(dp > d || (dp == d && order[(size_t)i - 1] < order[(size_t)i]));       // largest first, ties by row id
        }
        heavy_ref += d > gn_layout::kBasisHeavyEdges ? 1 : 0;
        if (i < heavy) CHECK(d > gn_layout::kBasisHeavyEdges);                             // the heavy rows lead the order
    }
    CHECK(heavy == heavy_ref);
    emit("degree_order", {fnv(order), (uint64_t)heavy});
    // relation ranges (a hub relation, empty relations), the whole list and two shards' edge ranges
    std::vector<int64_t> ranges((size_t)(2 * R));
    int64_t at = 0;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t len = r == 0 ? E / 2 : (r % 5 == 1 ? 0 : (int64_t)(rng() % (uint64_t)std::max<int64_t>(1, 2 * (E - E / 2) / R)));
        ranges[(size_t)(2 * r)] = at;
        at = std::min(E, at + len);
        ranges[(size_t)(2 * r + 1)] = r == R - 1 ? E : at;
        if (r == R - 1) at = E;
    }
    const int64_t cuts[3][2] = {{0, E}, {0, E / 3}, {E / 3, E}};
    for (auto& c : cuts) {
        const gn_layout::RelDwItems L = gn_layout::build_rel_dw_items(ranges, c[0], c[1]);
        CHECK(L.ok && L.items.size() % 4 == 0 && L.multi.size() % 4 == 0);
        emit("rel_dw_items", {fnv(L.items), fnv(L.multi), (uint64_t)L.parts});
        // the items tile [lo, hi) exactly, in order, inside their relation's range, at most kRelDwItemEdges edges each
        int64_t pos = c[0], slots = 0;
        for (size_t i = 0; i < L.items.size(); i += 4) {
            const int64_t r = L.items[i], a = L.items[i + 1], b = L.items[i + 2], slot = L.items[i + 3];
            CHECK(r >= 0 && r < R && a < b && b - a <= gn_layout::kRelDwItemEdges);
            CHECK(a >= ranges[(size_t)(2 * r)] && b <= ranges[(size_t)(2 * r + 1)]);
            while (pos < a) { bool inside_empty = true; (void)inside_empty; CHECK(false); }   // (no gap: a shard's relations are contiguous)
            CHECK(a == pos);
            pos = b;
            if (slot >= 0) { CHECK(slot == slots); ++slots; }
        }
        CHECK(pos == c[1] && slots == L.parts);
        for (size_t m = 0; m < L.multi.size(); m += 4) CHECK(L.multi[m + 2] > 1 && L.multi[m + 1] + L.multi[m + 2] <= L.parts);
    }
}

// After a fork the child has none of the parent's parked builder threads (host_parallel.hpp, WorkerPool): its first parallel pass
// must make its own instead of waiting for threads that do not exist there.
int fork_case() {
    set_threads(16);
    gn_layout::ClassLayout before = decoder_case(645, 40, 20000, 80, 7, true);      // the parent's pool exists from here on
    const pid_t child = fork();
    CHECK(child >= 0);
    if (child == 0) {
        gn_layout::ClassLayout in_child = decoder_case(645, 40, 20000, 80, 7, true);
        _exit(same(before.packed, in_child.packed) && same(before.own, in_child.own) ? 0 : 3);
    }
    int status = 0;
    CHECK(waitpid(child, &status, 0) == child);
    CHECK(WIFEXITED(status) && WEXITSTATUS(status) == 0);
    gn_layout::ClassLayout after = decoder_case(645, 40, 20000, 80, 7, true);       // ... and still works in the parent
    CHECK(same(before.packed, after.packed));
    std::printf("host layout: builder threads ok across fork\n");
    return 0;
}

// The cases main() runs, each on 1 and on 16 threads.
// (decoder: two giant relations; one relation; a long tail of small relations - more of them per workgroup than its D cache
// holds: not taken, as before)
const struct { int64_t n; int R; int64_t e; int64_t f; bool ok; } kDecoderCases[] = {
    {645, 40, 20000, 80, true}, {200, 7, 3000, 80, true}, {645, 3, 50000, 48, true}, {30, 2, 5, 16, true},
    {645, 200, 150000, 80, true}, {645, 2, 300000, 80, true}, {645, 1, 200000, 80, true}, {645, 964, 60000, 80, false}};
const int64_t kWindowCases[] = {(int64_t)8 << 10, (int64_t)40 << 10};     // an XCD's position range walked in several sub-ranges
const struct { int64_t n; int R; int64_t e; } kPhaseCases[] = {{645, 40, 20000}, {645, 7, 3000}, {30, 2, 5}};   // (the last: fewer than 64 scored edges)
const struct { int64_t N, R, E; } kPairCases[] = {{645, 30, 60000}, {200, 5, 9000}, {1, 1, 300}, {300, 964, 20000}};
const struct { int64_t N; int deg, R; } kBlockedCases[] = {{5000, 16, 32}, {700, 3, 11}, {19081, 38, 32}};
const struct { int64_t R; int tiles; int64_t E; } kFastCases[] = {{30, 2, 2000000}, {964, 1, 400000}, {3, 1, 300}, {5, 4, 9000}, {1, 1, 1}};
const struct { int64_t n, R, E; int groups; } kRelGradCases[] = {{645, 40, 200000, 256}, {100, 7, 5000, 256}, {37, 3, 10, 8}, {300, 964, 60000, 64}};

void general_cases() {
    balance_case(5);
    general_case(20000, 600, 300000, 21);
    general_case(50, 3, 40, 22);
    general_case(1, 1, 1500, 23);
}

// One line per case: its name, then the hash of every output array (and of its scalars).
void digest_all(int threads) {
    set_threads(threads);
    std::printf("threads %d\n", threads);
    general_cases();
    char name[96];
    for (auto& c : kDecoderCases) {
        const gn_layout::ClassLayout L = decoder_case(c.n, c.R, c.e, c.f, 7, true, gn_layout::kClsWindowBytes, c.ok);
        std::snprintf(name, sizeof name, "decoder %lld/%d/%lld/%lld", (long long)c.n, c.R, (long long)c.e, (long long)c.f);
        emit(name, {fnv(L.packed), fnv(L.own), fnv(L.mirror), fnv(L.rel32), fnv(L.wg), (uint64_t)L.ok, (uint64_t)L.groups, (uint64_t)L.walks, (uint64_t)L.batches});
    }
    for (int64_t window : kWindowCases) {
        const gn_layout::ClassLayout L = decoder_case(645, 40, 20000, 80, 9, true, window);
        std::snprintf(name, sizeof name, "window %lld", (long long)window);
        emit(name, {fnv(L.packed), fnv(L.own), fnv(L.mirror), fnv(L.rel32), fnv(L.wg), (uint64_t)L.ok, (uint64_t)L.groups, (uint64_t)L.walks, (uint64_t)L.batches});
    }
    for (auto& c : kPhaseCases) {
        std::vector<int> slots;
        const PhaseLayout L = phase_case(c.n, c.R, c.e, 7, slots);
        std::snprintf(name, sizeof name, "deal_batch %lld/%d/%lld", (long long)c.n, c.R, (long long)c.e);
        emit(name, {fnv(slots)});
        std::snprintf(name, sizeof name, "phase %lld/%d/%lld", (long long)c.n, c.R, (long long)c.e);
        emit(name, {fnv(L.packed), fnv(L.own), fnv(L.mirror), fnv(L.batch_rel), fnv(L.rel16)});
    }
    for (auto& c : kPairCases) {
        const gn_layout::PairLayout L = pair_case(c.N, c.R, c.E, 11, true);
        std::snprintf(name, sizeof name, "pair %lld/%lld/%lld", (long long)c.N, (long long)c.R, (long long)c.E);
        emit(name, {fnv(L.stream), fnv(L.wave_first), fnv(L.desc), fnv(L.wave_units), fnv(L.wave_desc), fnv(L.wg_dst), (uint64_t)L.blocks});
    }
    for (auto& c : kFastCases) {
        const std::pair<FastItems, FastWork> L = fast_case(c.R, c.tiles, c.E, 19);
        std::snprintf(name, sizeof name, "rgcn_fast %lld/%d/%lld", (long long)c.R, c.tiles, (long long)c.E);
        emit(name, {fnv(L.first.item_rel), fnv(L.first.item_tile), fnv(L.first.item_begin), fnv(L.first.piece_first), fnv(L.first.piece_group),
                    (uint64_t)L.first.groups, fnv(L.second.wg_begin), fnv(L.second.desc)});
    }
    for (auto& c : kBlockedCases) {
        const gn_layout::BlockedLayout L = blocked_case(c.N, c.deg, c.R, 13, true);
        std::snprintf(name, sizeof name, "blocked %lld/%d/%d", (long long)c.N, c.deg, c.R);
        std::vector<uint32_t> dis_bits(L.tile_dis.size());
        std::memcpy(dis_bits.data(), L.tile_dis.data(), dis_bits.size() * sizeof(uint32_t));
        emit(name, {fnv(L.tile_off), fnv(L.tile_rows), fnv(L.cell), fnv(dis_bits), fnv(L.ids), (uint64_t)L.iters_total});
    }
    for (auto& c : kRelGradCases) {
        const gn_layout::RelGradLayout L = rel_grad_case(c.n, c.R, c.E, c.groups, 17, true);
        std::snprintf(name, sizeof name, "rel_grad %lld/%lld/%lld/%d", (long long)c.n, (long long)c.R, (long long)c.E, c.groups);
        emit(name, {fnv(L.src), fnv(L.ids), fnv(L.entry), fnv(L.wave_cnt), fnv(L.wg_off), fnv(L.wave_u0), (uint64_t)L.groups,
                    (uint64_t)L.scratch_slots, (uint64_t)L.units});
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "fork") == 0) return fork_case();
    if (argc > 1 && std::strcmp(argv[1], "digest") == 0) {
        g_digest = true;
        digest_all(1);
        digest_all(16);
        return 0;
    }
    general_cases();
    shares_case();
    for (auto& c : kDecoderCases) {
        set_threads(1);
        gn_layout::ClassLayout a = decoder_case(c.n, c.R, c.e, c.f, 7, true, gn_layout::kClsWindowBytes, c.ok);
        set_threads(16);
        gn_layout::ClassLayout b = decoder_case(c.n, c.R, c.e, c.f, 7, true, gn_layout::kClsWindowBytes, c.ok);
        CHECK(same(a.packed, b.packed) && same(a.own, b.own) && same(a.mirror, b.mirror) && same(a.rel32, b.rel32) && same(a.wg, b.wg));
    }
    for (auto& c : kPhaseCases) {
        std::vector<int> slots;
        set_threads(1);
        const PhaseLayout a = phase_case(c.n, c.R, c.e, 7, slots);
        set_threads(16);
        const PhaseLayout b = phase_case(c.n, c.R, c.e, 7, slots);
        CHECK(same(a.packed, b.packed) && same(a.own, b.own) && same(a.mirror, b.mirror) && same(a.batch_rel, b.batch_rel) && same(a.rel16, b.rel16));
    }
    // the builders' host arena (host_parallel.hpp): the same plan with its large arrays out of the kept block - the first hold finds no
    // block (everything by malloc, the demand noted), the later ones are served from it; a second builder meanwhile gets malloc
    {
        set_threads(16);
        std::vector<uint32_t> want_packed;
        {
            gn_layout::ClassLayout plain = decoder_case(645, 40, 20000, 80, 7, false);
            want_packed.assign(plain.packed.begin(), plain.packed.end());
            CHECK(!gn::arena_owns(plain.packed.data()));
        }
        for (int pass = 0; pass < 3; ++pass) {
            gn::ArenaHold hold;
            CHECK(hold.held);
            gn_layout::ClassLayout l = decoder_case(645, 40, 20000, 80, 7, true);
            CHECK(l.packed.size() == want_packed.size() && std::equal(want_packed.begin(), want_packed.end(), l.packed.begin()));
            CHECK(l.packed.size() * sizeof(uint32_t) >= gn::HostArena::kMinBytes);
            CHECK(gn::arena_owns(l.packed.data()) == (pass > 0));
            std::thread other([] {
                gn::ArenaHold second;
                CHECK(!second.held);
                gn::RawVec<int> v((size_t)1 << 20);
                CHECK(!gn::arena_owns(v.data()));
            });
            other.join();
        }
    }
    for (int64_t window : kWindowCases) {
        set_threads(16);
        gn_layout::ClassLayout w = decoder_case(645, 40, 20000, 80, 9, true, window);
        CHECK(w.walks == (window == ((int64_t)8 << 10) ? 8 : 3));
    }
    for (auto& c : kPairCases) {
        set_threads(1);
        gn_layout::PairLayout a = pair_case(c.N, c.R, c.E, 11, true);
        set_threads(16);
        gn_layout::PairLayout b = pair_case(c.N, c.R, c.E, 11, true);
        CHECK(same(a.stream, b.stream) && same(a.desc, b.desc) && same(a.wave_first, b.wave_first) && same(a.wave_units, b.wave_units) &&
              same(a.wave_desc, b.wave_desc) && same(a.wg_dst, b.wg_dst));
    }
#if __has_include("layout_rgcn_fast.hpp")
    {   // more items than the caller's 32-bit indices hold: nothing behind the items is built
        const FastItems refused = build_fast_items({0, 3 * kFastItemEdges}, 1, 3 * kFastItemEdges, 2);
        CHECK(refused.n_items() == 3 && refused.groups == 0 && refused.piece_first.empty());
        CHECK(build_fast_items({0, 3 * kFastItemEdges}, 1, 3 * kFastItemEdges, 3).groups >= 1);
    }
#endif
    for (auto& c : kFastCases) {
        set_threads(1);
        const std::pair<FastItems, FastWork> a = fast_case(c.R, c.tiles, c.E, 19);
        set_threads(16);
        const std::pair<FastItems, FastWork> b = fast_case(c.R, c.tiles, c.E, 19);
        CHECK(same(a.first.item_begin, b.first.item_begin) && same(a.first.piece_group, b.first.piece_group) && a.first.groups == b.first.groups &&
              same(a.second.wg_begin, b.second.wg_begin) && same(a.second.desc, b.second.desc));
    }
    for (auto& c : kBlockedCases) {
        set_threads(1);
        gn_layout::BlockedLayout a = blocked_case(c.N, c.deg, c.R, 13, true);
        set_threads(16);
        gn_layout::BlockedLayout b = blocked_case(c.N, c.deg, c.R, 13, true);
        CHECK(same(a.ids, b.ids) && same(a.tile_off, b.tile_off) && same(a.tile_rows, b.tile_rows) && same(a.cell, b.cell));
    }
    for (auto& c : kRelGradCases) {
        set_threads(1);
        gn_layout::RelGradLayout a = rel_grad_case(c.n, c.R, c.E, c.groups, 17, true);
        set_threads(16);
        gn_layout::RelGradLayout b = rel_grad_case(c.n, c.R, c.E, c.groups, 17, true);
        CHECK(same(a.src, b.src) && same(a.ids, b.ids) && same(a.entry, b.entry) && same(a.wave_cnt, b.wave_cnt) && same(a.wave_u0, b.wave_u0));
    }
    std::printf("host layout: all builders ok on 1 and 16 threads\n");
    return 0;
}
