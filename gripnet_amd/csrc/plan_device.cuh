// Device stages that several plan builders share: the rocprim size-query / scratch / run triples, the two binary searches and
// the row-pointer kernel.  Plan construction, and the row offsets of the sort-based backwards (seg_reduce.cuh); the other
// step-path kernels keep their own searches.
#pragma once

#include "common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace gn {

// bits of a radix sort over keys in [0, n)
inline int bits_for(int64_t n) {
    int b = 1;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}

// Stable radix sorts over the low `bits` bits; the workspace comes out of `tmp`.  Nothing for n == 0.  (The inputs are plain
// pointers like the outputs: rocprim instantiates its passes per iterator type, and a `const K*` input would add a second set
// of them - a third of a megabyte of code per file that sorts.)
template <typename K, typename V>
gn_status sort_pairs(Scratch& tmp, K* kin, K* kout, V* vin, V* vout, size_t n, int bits, hipStream_t st) {
    if (n == 0) return GN_OK;
    size_t bytes = 0;
    GN_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0, bits, st));
    char* work = nullptr;
    GN_HIP(tmp.get(&work, bytes));
    GN_HIP(rocprim::radix_sort_pairs(work, bytes, kin, kout, vin, vout, n, 0, bits, st));
    return GN_OK;
}

template <typename K>
gn_status sort_keys(Scratch& tmp, K* kin, K* kout, size_t n, int bits, hipStream_t st) {
    if (n == 0) return GN_OK;
    size_t bytes = 0;
    GN_HIP(rocprim::radix_sort_keys(nullptr, bytes, kin, kout, n, 0, bits, st));
    char* work = nullptr;
    GN_HIP(tmp.get(&work, bytes));
    GN_HIP(rocprim::radix_sort_keys(work, bytes, kin, kout, n, 0, bits, st));
    return GN_OK;
}

// out[i] = in[0] + ... + in[i - 1]  (a template like the sorts, so that only a file that scans carries rocprim's scan kernels)
template <typename In>
gn_status exclusive_scan_i32(Scratch& tmp, In in, int32_t* out, size_t n, hipStream_t st) {
    size_t bytes = 0;
    GN_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, n, rocprim::plus<int32_t>(), st));
    char* work = nullptr;
    GN_HIP(tmp.get(&work, bytes));
    GN_HIP(rocprim::exclusive_scan(work, bytes, in, out, 0, n, rocprim::plus<int32_t>(), st));
    return GN_OK;
}

// Last i in [0, n) with starts[i] <= e (0 when there is none): the relation of edge e from the range starts of a type-sorted
// list, the work item of a position from the items' first positions.
template <typename T, typename E>
__device__ __forceinline__ int last_start_le(const T* __restrict__ starts, int n, E e) {
    int a = 0, b = n;
    while (b - a > 1) {
        const int mid = a + ((b - a) >> 1);
        if (starts[mid] <= e) a = mid; else b = mid;
    }
    return a;
}

// First position in the sorted keys[0, n) whose key is >= v (n when there is none).  n up to 2^31 - 1: lo + hi may not be formed.
template <typename T>
__device__ __forceinline__ int lower_bound(const T* __restrict__ keys, int n, T v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// out[i] = first position whose key is >= i, for i in [0, count]: the row pointers of a sorted key list - a plan's, or a
// step's (seg_reduce.cuh).  The compare is signed and 64 bits wide: the ids below 0 of a sorted int64 edge_type sit in
// front of row 0 (ids >= count behind the last row), and a uint32 sort key compares as itself.
template <typename T>
__global__ void k_first_at_least(const T* __restrict__ sorted, int64_t n, int64_t count, int32_t* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i > count) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)sorted[mid] < i) lo = mid + 1; else hi = mid;
    }
    out[i] = (int32_t)lo;
}

template <typename T>
gn_status first_at_least(const T* sorted, int64_t n, int64_t count, int32_t* out, hipStream_t st) {
    k_first_at_least<T><<<(int)ceil_div(count + 1, 256), 256, 0, st>>>(sorted, n, count, out);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

}  // namespace gn
