// What the two sort-based segmented reductions (distmult_bwd.hip: the DistMult decoder's gradients; kge.hip: the KGE
// scorers') share: the chunk length their sorted record arrays are cut into, the alignment of their workspace arrays, and
// the row offsets of a sorted key array.  The records themselves differ (12 bytes: two factor rows and g; 16 bytes: head,
// tail, relation and g) and so do the reductions' contributions (a product of two rows; a functor of three).
#pragma once

#include "common.h"

namespace gn {

constexpr int kSegChunkRecs = 2048;            // records of a chunk: one workgroup each

inline size_t seg_align_up(size_t v) { return (v + 255) & ~size_t(255); }

// rowptr[i] = first position whose (sorted) key is >= i, for i in [0, rows]: uint32 sort keys, or an int64 edge_type that the
// caller promises to be non-decreasing (ids below 0 then sit in front of row 0, ids >= rows behind the last row)
template <typename K>
__global__ void k_key_offsets(const K* __restrict__ sorted, int64_t n, int rows, int32_t* __restrict__ rowptr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > rows) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)sorted[mid] < (int64_t)i) lo = mid + 1; else hi = mid;
    }
    rowptr[i] = (int32_t)lo;
}

}  // namespace gn
