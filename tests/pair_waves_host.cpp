// How the destination-major relational plan deals a workgroup's sixteen waves to its rows (gripnet_amd/csrc/layout_rgcn_pair.hpp:
// build_pair_layout), as a stand-alone host program: reads "N R E G" and E lines "src dst relation" (relations ascending, as a range
// list gives them) from standard input, lays the plan out as gn_rgcn_build_pair_plan does for G workgroups, and prints one line per
// workgroup: the number of waves of each of its rows.  tests/test_gpu_rel_epilogue.py builds it with g++ and asserts that its
// graphs put a row on one wave and a row on all sixteen.  No HIP, no GPU.
#include <cstdio>
#include <numeric>

#include "host_layout.hpp"

int main() {
    long long N, R, E, G;
    if (scanf("%lld %lld %lld %lld", &N, &R, &E, &G) != 4) return 2;
    std::vector<int64_t> src((size_t)E), dst((size_t)E);
    std::vector<uint32_t> rel((size_t)E);
    std::vector<int32_t> outdeg((size_t)N, 0);
    for (long long e = 0; e < E; ++e) {
        long long s, d, r;
        if (scanf("%lld %lld %lld", &s, &d, &r) != 3) return 2;
        src[e] = s; dst[e] = d; rel[e] = (uint32_t)r;
        outdeg[s]++;
    }
    const int chunks = (int)((N + 31) / 32), kpad = chunks * 32, D = (int)((N + G - 1) / G);
    std::vector<int32_t> order((size_t)N), perm((size_t)kpad, (int32_t)N), kpos((size_t)N);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return outdeg[x] > outdeg[y]; });
    for (long long k = 0; k < N; ++k) { perm[k] = order[k]; kpos[order[k]] = (int32_t)k; }
    std::vector<int64_t> idx((size_t)E);
    std::iota(idx.begin(), idx.end(), 0);
    auto key = [&](int64_t e) { return dst[e] * kpad + kpos[src[e]]; };
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return key(x) < key(y); });
    std::vector<int32_t> rp((size_t)N * kpad + 1, 0);
    std::vector<uint32_t> rels((size_t)E);
    for (long long i = 0; i < E; ++i) { rels[i] = rel[idx[i]]; rp[key(idx[i]) + 1]++; }
    for (size_t i = 1; i < rp.size(); ++i) rp[i] += rp[i - 1];
    const gn_layout::PairLayout L = gn_layout::build_pair_layout(N, R, chunks, kpad, (int)G, D, rp, rels, perm);
    if (!L.ok) return 3;
    for (long long g = 0; g < G; ++g) {
        const int32_t* w = L.wg_dst.data() + g * 4;
        const int nd = (w[0] >= 0) + (w[1] >= 0) + (w[2] >= 0);
        // the first wave of rows 1 and 2, eight bits each (16 where the workgroup has no such row): what the kernel reads
        const int b1 = w[3] & 0xff, b2 = (w[3] >> 8) & 0xff;
        if (nd == 1) printf("%d\n", 16);
        else if (nd == 2) printf("%d %d\n", b1, 16 - b1);
        else if (nd == 3) printf("%d %d %d\n", b1, b2 - b1, 16 - b2);
        else printf("\n");
    }
    return 0;
}
