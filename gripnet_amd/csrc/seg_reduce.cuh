// The chunked segmented reduction behind the sort-based backwards (distmult_bwd.hip: the DistMult decoder's general path;
// kge.hip: the KGE scorers):  out[key_e, :] (+)= sum over the records e of a key of  g_e * d(record e, :)  without float
// atomics, bitwise reproducible.
//
//   1. the caller builds one record per list entry (ids and g) and a key;
//   2. the records are radix-sorted by key (rocPRIM, stable) - or left alone when the list is already in key order - and the
//      row offsets come from a binary search (gn::first_at_least, plan_device.cuh);
//   3. the sorted array is cut into chunks of kSegChunkRecs records, one workgroup each (a hub row of 10^5 records and rows
//      of a few records cost the same per record); a caller whose rows hold a record or two asks for smaller chunks (CHUNK);
//   4. per row of a chunk the workgroup sums the row's records inside the chunk: 256 threads = S = 256 / LPE records in
//      flight x LPE lanes of VEC columns each; a thread visits begin + slot, + S, + 2 S, ... in that order, two records per
//      trip where the registers allow it;
//   5. the S slots are folded through LDS in slot order;
//   6. a row that lies wholly inside the chunk is final and goes to `out`;
//   7. a row that continues in a neighbour chunk goes to one of the chunk's two partial slots: slot 0 when the row began at
//      or before the chunk's first record, slot 1 otherwise.  A chunk has at most one row of either kind, every chunk that
//      a straddling row touches holds a record of it, and `rowptr` alone tells which slot: nothing is zeroed beforehand;
//   8. k_seg_combine adds the partials of a straddling row in chunk order and zeroes the rows that have no record.
//
// What a record contributes is the caller's: a Contribution type C with
//   C::Rec                       the record, with a member `float g`; Rec{} (all zero) must name rows that exist
//   C::P                         output parts (1 or 2): part p of a row starts at column p * out_h
//   C::kFused                    acc = fma(g, d, acc) when true, acc + g * d rounded twice when false
//   C::skip(rec)                 a record that contributes nothing (an id outside its table)
//   c.terms<VEC>(rec, unit, d)   d[p][v] for the columns [unit * VEC, unit * VEC + VEC)
// A slot behind the row's end reads the row's first record again, a skipped record is replaced by Rec{} - its gathers read
// row 0 - and the term of either is dropped: no read outside a table.
#pragma once

#include "common.h"
#include "plan_device.cuh"

namespace gn {

constexpr int kSegChunkRecs = 2048;            // records of a chunk: one workgroup each
constexpr int kSegBlockCols = 64;              // columns of a partial slot: the widest column block of a launch

inline size_t seg_align_up(size_t v) { return (v + 255) & ~size_t(255); }

// everything of a launch but the contribution
template <typename Rec>
struct SegFrame {
    const int32_t* rowptr; const Rec* recs; int64_t n_recs; int rows;
    float* out; int64_t ld_out; int out_h;         // part p of the output row starts at column p * out_h
    float* partial;                                // [chunk][slot 0 / 1][part][kSegBlockCols]
    int u0, units;                                 // first unit (of VEC columns) of this launch's column block; units of a row
    int accumulate;
};

template <typename C>
struct SegArgs { C c; SegFrame<typename C::Rec> f; };

template <bool FUSED, int P, int VEC>
__device__ __forceinline__ void seg_add(float (&acc)[P][VEC], float g, const float (&d)[P][VEC], bool live) {
#pragma clang fp contract(off)
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float next = FUSED ? __builtin_fmaf(g, d[p][v], acc[p][v]) : acc[p][v] + g * d[p][v];
            acc[p][v] = live ? next : acc[p][v];
        }
}

// CHUNK: records of a chunk.  kSegChunkRecs wherever rows are long; a pass over few records with short rows (a record or
// two per row: the rows of a chunk are taken one after the other, two barriers each) cuts smaller chunks for more workgroups.
template <typename C, int VEC, int LPE, int CHUNK = kSegChunkRecs>
__global__ __launch_bounds__(256) void k_seg_reduce(SegArgs<C> a) {
    using Rec = typename C::Rec;
    constexpr int S = 256 / LPE, P = C::P;         // S: records per step
    // Records a thread has in flight: two where a record's terms are four floats or fewer - four or more gathers in flight;
    // one where they are eight (two parts of float4 columns): a second record's rows would take those kernels past 64
    // registers, an occupancy step, or into scratch.  The order of the additions does not depend on it.
    constexpr int T = P * VEC > 4 ? 1 : 2;
    static_assert(LPE * VEC <= kSegBlockCols && P * LPE * VEC <= 256, "a column block fits a partial slot and one fold trip");
    __shared__ float part[P][S][LPE * VEC];
    const SegFrame<Rec>& f = a.f;
    const int j = threadIdx.x % LPE, slot = threadIdx.x / LPE;
    const int lo = blockIdx.x * CHUNK;
    const int hi = (int)min((int64_t)lo + CHUNK, f.n_recs);
    const int unit = f.u0 + j;
    const bool col_ok = unit < f.units;
    // the first row with a record at or behind `lo`: the last row that begins at or before it
    for (int row = last_start_le(f.rowptr, f.rows, lo); row < f.rows; ++row) {
        const int rb = f.rowptr[row], re = f.rowptr[row + 1];
        if (rb >= hi) break;                                // workgroup-uniform
        const int begin = max(lo, rb), end = min(hi, re);
        if (begin >= end) {
            // No record here.  The record at rb, if there is one, belongs to the last row that starts at rb: go there in
            // one search instead of one dependent load per empty row (1 024 records keyed into 19 726 rows walked most
            // of them, 4 ms of a pass).  The rows visited, and their order, stay the same.
            const int next = last_start_le(f.rowptr, f.rows, rb);
            if (next > row) row = next - 1;
            continue;
        }
        float acc[P][VEC];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[p][v] = 0.f;
        if (col_ok) {
            for (int base = begin; base < end; base += T * S) {     // T records per thread and trip, added in position order
                Rec r[T];
                bool live[T];
                float d[T][P][VEC];
                // (unconditional loads at a clamped index: behind a conditional load hipcc waits before it issues the next one)
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const int i = base + t * S + slot;
                    live[t] = i < end;
                    r[t] = f.recs[live[t] ? i : begin];
                }
                __builtin_amdgcn_sched_barrier(0);          // every record is requested before the first one is waited for
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    if (C::skip(r[t])) { live[t] = false; r[t] = Rec{}; }
                }
#pragma unroll
                for (int t = 0; t < T; ++t) a.c.template terms<VEC>(r[t], unit, d[t]);
#pragma unroll
                for (int t = 0; t < T; ++t) seg_add<C::kFused>(acc, r[t].g, d[t], live[t]);
            }
        }
        __syncthreads();                                    // the previous row's fold is done with `part`
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int v = 0; v < VEC; ++v) part[p][slot][j * VEC + v] = acc[p][v];
        __syncthreads();
        // thread (p, column) folds the S slots in slot order
        const int p = threadIdx.x / (LPE * VEC), c = threadIdx.x % (LPE * VEC);
        const int column = f.u0 * VEC + c;
        if (p < P && column < f.units * VEC) {
            float s = part[p][0][c];
#pragma unroll
            for (int k = 1; k < S; ++k) s += part[p][k][c];
            if (rb >= lo && re <= hi) {                     // the whole row is here: final
                float* o = f.out + (int64_t)row * f.ld_out + (int64_t)p * f.out_h + column;
                *o = f.accumulate ? *o + s : s;
            } else {                                        // shared with a neighbour chunk
                const int which = rb <= lo ? 0 : 1;
                f.partial[(((size_t)blockIdx.x * 2 + which) * P + p) * kSegBlockCols + c] = s;
            }
        }
    }
}

// Rows that straddle chunks: out[row, block] (+)= the chunks' partials in chunk order; rows without a record: zeros.
// A workgroup per row, 64 threads per part.  (static: a plain kernel in a header that two files include)
static __global__ void k_seg_combine(const int32_t* __restrict__ rowptr, const float* __restrict__ partial, float* __restrict__ out,
                              int64_t ld_out, int out_h, int parts, int c0, int width, int accumulate, int chunk_recs) {
    const int row = blockIdx.x, c = threadIdx.x % kSegBlockCols, p = threadIdx.x / kSegBlockCols;
    if (c >= width || p >= parts) return;
    const int rb = rowptr[row], re = rowptr[row + 1];
    float* o = out + (int64_t)row * ld_out + (int64_t)p * out_h + c0 + c;
    if (rb >= re) {
        if (!accumulate) *o = 0.f;
        return;
    }
    const int cb = rb / chunk_recs, ce = (re - 1) / chunk_recs;
    if (cb == ce) return;                                   // inside one chunk: k_seg_reduce wrote the final value
    float s = 0.f;
    for (int b = cb; b <= ce; ++b) {
        const int which = rb <= b * chunk_recs ? 0 : 1;
        s += partial[(((size_t)b * 2 + which) * parts + p) * kSegBlockCols + c];
    }
    *o = accumulate ? *o + s : s;
}

// ---- host side ----------------------------------------------------------------------------------------------------
// A pass's scratch: keys and records before and behind the sort, the row offsets of up to max_rows rows, the chunks'
// partials for up to `parts` output parts, a tail that is the caller's (the KGE scorers keep RotatE's cos / sin tables
// there), rocPRIM's temporary.  chunk_recs: the smallest chunk any pass over this scratch cuts (the partials hold a slot pair
// per chunk).  also_sorts: a smaller record count that a later pass sorts in the same scratch (rocPRIM picks its algorithm,
// and its temporary, by size: the temporary is the larger of the two).
struct SegLayout { size_t keys, keys_sorted, recs, recs_sorted, rowptr, partial, tail, sort_tmp, total; };

template <typename Rec>
SegLayout seg_layout(int64_t e, int64_t max_rows, int parts, size_t tail_bytes, int chunk_recs = kSegChunkRecs, int64_t also_sorts = 0) {
    SegLayout l;
    size_t sort_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (Rec*)nullptr, (Rec*)nullptr,
                                    (size_t)e, 0, 32, (hipStream_t)0);
    if (also_sorts > 0) {
        size_t other = 0;
        (void)rocprim::radix_sort_pairs(nullptr, other, (uint32_t*)nullptr, (uint32_t*)nullptr, (Rec*)nullptr, (Rec*)nullptr,
                                        (size_t)also_sorts, 0, 32, (hipStream_t)0);
        sort_bytes = std::max(sort_bytes, other);
    }
    l.keys = 0;
    l.keys_sorted = l.keys + seg_align_up(e * sizeof(uint32_t));
    l.recs = l.keys_sorted + seg_align_up(e * sizeof(uint32_t));
    l.recs_sorted = l.recs + seg_align_up(e * sizeof(Rec));
    l.rowptr = l.recs_sorted + seg_align_up(e * sizeof(Rec));
    l.partial = l.rowptr + seg_align_up((max_rows + 2) * sizeof(int32_t));
    l.tail = l.partial + seg_align_up((size_t)ceil_div(e, (int64_t)chunk_recs) * 2 * parts * kSegBlockCols * sizeof(float));
    l.sort_tmp = l.tail + seg_align_up(tail_bytes);
    l.total = l.sort_tmp + seg_align_up(sort_bytes);
    return l;
}

template <typename Rec>
struct SegWs {
    uint32_t *keys, *keys_sorted;
    Rec *recs, *recs_sorted;
    int32_t* rowptr;
    float* partial;
    void* sort_tmp; size_t sort_bytes;
    SegWs(char* ws, const SegLayout& l)
        : keys(reinterpret_cast<uint32_t*>(ws + l.keys)), keys_sorted(reinterpret_cast<uint32_t*>(ws + l.keys_sorted)),
          recs(reinterpret_cast<Rec*>(ws + l.recs)), recs_sorted(reinterpret_cast<Rec*>(ws + l.recs_sorted)),
          rowptr(reinterpret_cast<int32_t*>(ws + l.rowptr)), partial(reinterpret_cast<float*>(ws + l.partial)),
          sort_tmp(ws + l.sort_tmp), sort_bytes(l.total - l.sort_tmp) {}
};

// where a pass's sums go
struct SegOut { float* out; int64_t ld_out; int out_h, parts, accumulate; };

// From w.keys / w.recs to records in key order and their row offsets.  `ordered`: the int64 keys of a list that the caller
// promises to be in key order already - nothing is sorted, the records stay in w.recs (ids below 0 sit in front of row 0, ids
// >= rows behind the last row).  Returns the records to reduce.
template <typename Rec>
gn_status seg_sort(const SegWs<Rec>& w, int64_t e, int64_t rows, const int64_t* ordered, const Rec** sorted, hipStream_t st) {
    *sorted = ordered ? w.recs : w.recs_sorted;
    if (ordered) return first_at_least(ordered, e, rows, w.rowptr, st);
    size_t sort_bytes = w.sort_bytes;
    GN_HIP(rocprim::radix_sort_pairs(w.sort_tmp, sort_bytes, w.keys, w.keys_sorted, w.recs, w.recs_sorted, (size_t)e, 0, bits_for(rows + 1), st));
    return first_at_least(w.keys_sorted, e, rows, w.rowptr, st);
}

// One pass behind the caller's record kernel: sort (or not), offsets, then per column block of `block_units` units a reduce
// launch and the combine.  reduce(frame, units of the block, chunks) launches k_seg_reduce with the caller's contribution,
// VEC and the LPE of its own rule - and with CHUNK = chunk_recs where that is not kSegChunkRecs (the workspace's partials
// must then hold ceil(e / chunk_recs) chunks).
template <typename Rec, typename Reduce>
gn_status seg_pass(const SegWs<Rec>& w, int64_t e, int64_t rows, const int64_t* ordered, const SegOut& o, int units, int vec,
                   int block_units, Reduce reduce, hipStream_t st, int chunk_recs = kSegChunkRecs) {
    SegFrame<Rec> f;
    GN_OK_OR_RETURN(seg_sort(w, e, rows, ordered, &f.recs, st));
    f.rowptr = w.rowptr; f.n_recs = e; f.rows = (int)rows;
    f.out = o.out; f.ld_out = o.ld_out; f.out_h = o.out_h; f.partial = w.partial; f.units = units; f.accumulate = o.accumulate;
    const unsigned chunks = (unsigned)ceil_div(e, chunk_recs);
    for (int u0 = 0; u0 < units; u0 += block_units) {
        const int block = std::min(block_units, units - u0);
        f.u0 = u0;
        reduce(f, block, chunks);
        GN_LAUNCH_CHECK();
        k_seg_combine<<<(unsigned)rows, kSegBlockCols * o.parts, 0, st>>>(w.rowptr, w.partial, o.out, o.ld_out, o.out_h, o.parts, u0 * vec,
                                                                           block * vec, o.accumulate, chunk_recs);
        GN_LAUNCH_CHECK();
    }
    return GN_OK;
}

}  // namespace gn
