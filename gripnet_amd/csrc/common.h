// Shared host-side helpers for the gfx950 supergraph propagation library.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <type_traits>
#include <vector>

#include "gripnet_hip.h"
#include "host_parallel.hpp"

namespace gn {

constexpr int kWave = 64;  // CDNA wavefront width

// ---- per-thread error message ------------------------------------------------------------
inline char* error_buffer() {
    static thread_local char buf[512] = {0};
    return buf;
}

inline gn_status fail(gn_status code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#define GN_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t _e = (call);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return gn::fail(GN_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, \
                            __LINE__);                                                            \
    } while (0)

#define GN_REQUIRE(cond, ...)                                   \
    do {                                                        \
        if (!(cond)) return gn::fail(GN_ERR_INVALID_ARG, __VA_ARGS__); \
    } while (0)

#define GN_LAUNCH_CHECK() GN_HIP(hipGetLastError())

#define GN_OK_OR_RETURN(call)           \
    do {                                \
        const gn_status _s = (call);    \
        if (_s != GN_OK) return _s;     \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }


// The ReLU of every epilogue: NaN stays NaN (torch.relu's contract; fmaxf alone returns 0 for it, and a diverged model
// then looks finite).  Every other value, -0 and the infinities included, keeps the bits fmaxf(v, 0) gives it: v for a NaN,
// fmaxf(v, 0) otherwise is IEEE 754-2019's `maximum`, one v_maximum3_f32 on gfx950 where fmaxf was one v_max_f32 (written as
// `v != v ? v : fmaxf(v, 0.f)` it is a compare and a select more per stored element).
__device__ __forceinline__ float relu_keep_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }

// Compute units of the current device (persistent kernels launch one workgroup each); 256 if the query fails.
inline int compute_units() {
    static int cached[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
    if (cached[dev] == 0) {
        hipDeviceProp_t prop;
        cached[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    return cached[dev];
}

// GN_DISABLE_FAST=1 forces the general kernels (used by the parity tests to cover both paths).
inline bool fast_paths_disabled() {
    const char* e = getenv("GN_DISABLE_FAST");
    return e && e[0] == '1';
}

// Every device allocation of the library goes through these two, so that gn_device_blocks_live() counts exactly what the
// plans (DevBuf) and their builders (Scratch) hold.
inline std::atomic<int64_t>& device_blocks_live() {
    static std::atomic<int64_t> live{0};
    return live;
}
inline hipError_t device_malloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) device_blocks_live().fetch_add(1, std::memory_order_relaxed);
    return e;
}
inline void device_free(void* p) {
    (void)hipFree(p);
    device_blocks_live().fetch_sub(1, std::memory_order_relaxed);
}

// Device buffer owned by a plan (or by a scope): freed by its destructor, movable, not copyable.  A plan struct is destroyed
// by `delete`, a create function holds the plan in a std::unique_ptr until it hands it out - no list of buffers anywhere.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // releases what the buffer held, then allocates `count` elements (nothing when count is 0)
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) return hipSuccess;
        const hipError_t e = device_malloc(reinterpret_cast<void**>(&p), count * sizeof(T));
        if (e == hipSuccess) n = count; else p = nullptr;
        return e;
    }
    // alloc(count), then the copy of `count` elements from the host queued on `st` (none when count is 0).  Does not wait:
    // the caller synchronises the stream once, behind its last upload and before the host arrays die.
    hipError_t upload(const void* host, size_t count, hipStream_t st) {
        const hipError_t e = alloc(count);
        if (e != hipSuccess || count == 0) return e;
        return hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, st);
    }
    template <typename C>
    hipError_t upload(const C& host, hipStream_t st) {
        static_assert(sizeof(*host.data()) == sizeof(T), "element sizes differ: use the pointer form");
        return upload(host.data(), host.size(), st);
    }
    void release() {
        if (p) device_free(p);
        p = nullptr;
        n = 0;
    }
};
static_assert(!std::is_copy_constructible<DevBuf<int32_t>>::value && std::is_move_constructible<DevBuf<int32_t>>::value,
              "a DevBuf has one owner");

// Scoped device scratch of a plan builder, carved out of a few large blocks: a builder asks for ten to twenty arrays, and a
// hipMalloc / hipFree pair per array (the free waits for the device and unmaps) was a third of a relational plan's build
// time.  Every array is 256-byte aligned; a request that does not fit the current block opens a new one.
struct Scratch {
    static constexpr size_t kBlockBytes = (size_t)2 << 20;
    std::vector<void*> blocks;
    char* at = nullptr;
    size_t left = 0;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        GN_LAP(nullptr);
        for (void* b : blocks) device_free(b);
        GN_LAP("  scratch: frees");
    }
    // `reserve_bytes`: what the builder knows it will ask for in total (one block then serves all of it)
    hipError_t reserve(size_t reserve_bytes) { return reserve_bytes > left ? open(reserve_bytes) : hipSuccess; }
    template <typename T>
    hipError_t get(T** out, size_t count) {
        const size_t bytes = (((count ? count : 1) * sizeof(T)) + 255) & ~(size_t)255;
        *out = nullptr;
        if (bytes > left) {
            const hipError_t e = open(std::max(bytes, kBlockBytes << std::min<size_t>(blocks.size(), 5)));
            if (e != hipSuccess) return e;
        }
        *out = reinterpret_cast<T*>(at);
        at += bytes; left -= bytes;
        return hipSuccess;
    }
  private:
    hipError_t open(size_t bytes) {
        void* b = nullptr;
        const hipError_t e = device_malloc(&b, bytes);
        if (e != hipSuccess) return e;
        blocks.push_back(b);
        at = static_cast<char*>(b); left = bytes;
        return hipSuccess;
    }
};

// starts[R + 1] of a range_list [R][2] that must tile [0, E) in relation order (starts[R] = E).  bad_row: the first row that does
// not begin where the one before it ended or that ends before it begins, -1 when every row is in place; covered: where the rows
// in place ended - E when the list tiles [0, E).
struct RangeTiling {
    int64_t bad_row = -1, covered = 0;
};
inline RangeTiling range_starts(const int64_t* ranges, int64_t R, int64_t E, std::vector<int64_t>& starts) {
    starts.assign((size_t)R + 1, E);
    RangeTiling t;
    for (int64_t r = 0; r < R; ++r) {
        if (ranges[2 * r] != t.covered || ranges[2 * r + 1] < t.covered) { t.bad_row = r; break; }
        starts[r] = t.covered;
        t.covered = ranges[2 * r + 1];
    }
    return t;
}

// Grid size for a memory-bound grid-stride kernel: enough blocks to fill 256 CUs, capped.
inline int stream_grid(int64_t work_items, int block, int max_blocks = 256 * 8) {
    int64_t g = ceil_div(work_items, block);
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return static_cast<int>(g);
}

// Opt a kernel in to more than 64 KB of dynamic LDS, once per (kernel, device).
gn_status allow_large_lds(const void* kernel, int bytes);

// HIP events that the calling thread asked the NEXT timed kernel launch to carry (gn_time_next_launch): the launch site
// that supports it hands them to hipExtLaunchKernelGGL, which stamps the dispatch itself - no marker packets in the stream
// (an event record in front of and behind a launch costs ~4.5 us of stream time each on this stack).
struct LaunchEvents { hipEvent_t start = nullptr, stop = nullptr; };
LaunchEvents take_launch_events();          // the pending pair (or nulls), cleared

}  // namespace gn

// ---- plan layouts (shared between the builders and the kernels' launchers) --------------
struct gn_graph_plan {
    int64_t input_edges = 0;  // E the plan was built from (the reference's cache key)
    int64_t nnz = 0;          // stored coefficients (E' for GCN, E for bipartite)
    int64_t rows = 0;         // destination rows of the CSR
    int64_t table_rows = 0;   // rows of the gathered table (N for GCN, num_sources for bipartite)
    int64_t max_row_nnz = 0;
    int is_gcn = 0;
    // destination-major CSR streamed by the aggregation kernel
    gn::DevBuf<int32_t> rowptr;   // [rows + 1]
    gn::DevBuf<int32_t> col;      // [nnz]
    gn::DevBuf<float> coef;       // [nnz]
    // reference-order copies kept for myGCN.norm parity (GCN plans only)
    gn::DevBuf<int64_t> ref_edge_index;  // [2, nnz]
    gn::DevBuf<float> ref_norm;          // [nnz]
    // padded rows (bipartite plans whose longest row has at most 64 entries): lane L of the wave that owns row r reads entry
    // r * 64 + L directly - one dependent round trip less than row pointers -> columns (the external layer is three of them)
    int ell_ok = 0;
    gn::DevBuf<uint32_t> ell_col;        // [rows * 64] source row, 0xffffffff beyond the row's end
    gn::DevBuf<float> ell_coef;          // [rows * 64]
    // source-major CSR of the same coefficients (built on demand for the backward pass)
    int has_transpose = 0;
    gn::DevBuf<int32_t> t_rowptr;        // [table_rows + 1]
    gn::DevBuf<int32_t> t_col;           // [nnz] destination row of every stored coefficient
    gn::DevBuf<float> t_coef;            // [nnz]
    // LDS-staged encoding (gcn_blocked.hip; GCN plans whose stored weights are all 1, built on demand by
    // gn_graph_plan_build_blocked): destination rows in ranges x 16-row tiles, 16-bit source ids ordered for the LDS
    gn::DevBuf<float> dis;               // [rows] deg^-1/2 of every node (GCN plans)
    int unit_weights = 0;                // every stored weight (self loops included) is exactly 1
    int plain_ones = 0;                  // a plain sum without weights: every coefficient is exactly 1
    int blk_ok = 0, blk_cols = 0;        // built for layers of up to blk_cols output features
    int blk_cw = 0;                      // columns per column group (2, or 1 for larger graphs)
    int blk_rows = 0;                    // rows of one column group of the table (nodes + the zero row, padded to 1 KB pieces)
    int blk_cells = 0;                   // ranges of destination rows (workgroups per column group)
    int64_t blk_iters = 0;               // 512-byte iterations of the id stream
    int blk_range_tiles = 0;             // tiles of the largest range (the staged gather parks a range's tile sums in LDS)
    gn::DevBuf<float> blk_dis;           // [blk_rows + 16] dis, zero padded
    gn::DevBuf<int32_t> blk_tile_off;    // [tiles + 4] first iteration of every tile
    gn::DevBuf<int32_t> blk_tile_rows;   // [tiles + 4][16] destination row of every quad of a tile (-1: none)
    gn::DevBuf<float> blk_tile_dis;      // [tiles + 4][16] dis of that row
    gn::DevBuf<uint32_t> blk_ids;        // per iteration 64 lanes x 4 uint16 source ids (512 bytes)
    gn::DevBuf<int32_t> blk_cell;        // [blk_cells][waves][12] tile and iteration range of every wave of a range, the ends of its first five tiles
    gn::DevBuf<float> blk_table;         // [blk_cols / blk_cw][blk_rows][blk_cw] dis * (x W) (scratch of the plan)
};

struct gn_rgcn_plan {
    int64_t input_edges = 0;   // full E
    int64_t edge_lo = 0, edge_hi = 0;
    int64_t shard_edges = 0;
    int64_t num_nodes = 0;
    int64_t num_relations = 0;
    int64_t max_row_nnz = 0;
    gn::DevBuf<float> indeg;       // [N] in-degree over the FULL graph, as float (divisor of the mean)
    // general path: destination-major CSR over the shard, column = relation * N + src
    gn::DevBuf<int32_t> rowptr;    // [N + 1]
    gn::DevBuf<uint32_t> key;      // [shard_edges]
    gn::DevBuf<int32_t> row_order; // [N] destination rows by the shard's in-degree, largest first (rgcn_basis.hip deals rows in this order)
    int64_t heavy_rows = 0;        // rows of more than gn_layout::kBasisHeavyEdges edges (the first entries of row_order)
    gn::DevBuf<int32_t> pos;       // [shard_edges] of every key: its edge's position in the caller's own list (weighted calls only:
    int has_pos = 0;               // gn_rgcn_plan_build_positions, on first use)
    // relation-major work items of the general weight gradient (rgcn_basis.hip): (relation, first edge, end edge, part | parts << 16)
    // over the shard's edges in the caller's (type-sorted) order, <= gn_layout::kRelDwItemEdges edges each
    gn::DevBuf<int32_t> dw_items;  // [n_dw_items][4]
    int64_t n_dw_items = 0, n_dw_parts = 0;   // parts: items of relations cut into more than one (their sums meet in a workspace)
    gn::DevBuf<int32_t> dw_multi;  // [n_dw_multi][4] relations of several parts: (relation, first slot, parts, 0)
    int64_t n_dw_multi = 0;
    // LDS-resident path (rgcn_fast.hip): work items = (relation, source tile, <= chunk edges)
    gn::DevBuf<int32_t> seg_begin;  // [n_items * buckets + 1] bucket offsets into packed
    gn::DevBuf<uint32_t> packed;    // [shard_edges] (dst << 16 | src - tile base), bucket-sorted inside an item
    gn::DevBuf<int32_t> wg_begin;   // [groups + 1] ranges into wg_items
    gn::DevBuf<int32_t> wg_items;   // item ids per persistent workgroup
    int fast_groups = 0, fast_ts = 0;
    size_t fast_lds_bytes = 0;
    int fast_cols = 32;             // output columns per workgroup of the LDS-resident kernel (32, or 16 = column halves)
    int fast_ok = 0;
    // destination-major path (rgcn_pair.hip): a workgroup owns up to three destination rows outright; per wave one
    // flat stream of 64-byte blocks (4 lane groups x 4 edges, each a 32-bit LDS byte offset of a relation's att row)
    gn::DevBuf<uint32_t> pair_stream;     // blocks of 16 words
    gn::DevBuf<uint32_t> pair_wave_first; // [groups * 8] first block of every wave
    gn::DevBuf<uint32_t> pair_desc;       // 32 dwords per unit: eight 8-bit block counts, [8..23] the chunk's 32 source ids (16 bits; num_nodes: none); pages of two units per wave
    gn::DevBuf<uint32_t> pair_wave_units; // [groups * 8] units of every wave
    gn::DevBuf<uint32_t> pair_wave_desc;  // [groups * 16] first descriptor of every wave
    gn::DevBuf<int32_t> pair_wg_dst;      // [groups][4] destination rows of a workgroup (-1: none)
    int pair_groups = 0, pair_d = 0, pair_chunks = 0;
    int64_t pair_blocks = 0;
    int pair_ok = 0;
};

// Known (relation, u, v) pairs of the filtered ranking kernels (negsample.hip builds it, distmult_rank.hip reads it): the
// union of the caller's lists, sorted on the sampler's (relation << 40 | u * n + v) keys, as one row per (relation, u) of
// sorted partner ids.  Duplicates stay (the kernels set bits: set semantics).  O(E + R * n) words.
struct gn_known_pairs {
    int64_t num_edges = 0, num_nodes = 0, num_relations = 0;
    gn::DevBuf<int32_t> rowptr;     // [R * n + 1] first partner of row r * n + u
    gn::DevBuf<int32_t> partners;   // [E] v, sorted inside a row
};
