// Which kernel serves a dense product, and with which tile, grid and LDS size: the one place where gemm.hip's entry points
// (gn_gemm_addend_f32, gn_xtg_f32, gn_xtg_wide_supported) and its queue of batched products read it.  Pure host arithmetic on
// the arguments of a validated call - no HIP in here, no allocation, no formatting - so that this file also builds with plain
// g++, where tests/dense_route_host.cpp prints the route of every boundary shape (tests/test_dense_route.py holds the table).
#pragma once

#include <algorithm>
#include <cstdint>

#include "gripnet_hip.h"

namespace gn {
namespace route {

constexpr int kColTiles = 4;             // 16-column tiles per wave of k_gemm_f32 and the tall-skinny fp32 kernel
constexpr int kXtgSlices = 256;          // row slices of an x^T g at most: what gn_xtg_workspace_bytes holds
constexpr int kXtgMaxRows = 128;         // rows of a slice that k_xtg_partial holds in LDS at a time
constexpr int kXtgMfmaSlices = 32;       // slices of the one-launch x^T g that the last one to arrive adds alone
constexpr int kXtgMfmaMax = 128;         // slices of a long one (two levels)
constexpr int64_t kFragBytes = 64 * 16;  // one matrix-instruction fragment: a 16-byte word per lane
constexpr int64_t kLdsSmall = 64 * 1024; // dynamic LDS a kernel gets without the opt-in (gn::allow_large_lds)

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- c = a b --------------------------------------------------------------------------------------------------------
enum class Gemm { general, deep, lds, split, refused };
enum class Refusal { none, batch_limit, out_bf16, a_transposed_shape };

struct GemmCall {
    int64_t m, n, k, batch;   // all > 0 but k >= 0; m, n, k < 2^31
    int flags;                // GN_GEMM_*
    bool a_rows;              // A is row-gathered
    bool a_vec_ok;            // A takes 16-byte loads
    bool bf16_vec_ok;         // the bf16 form of c_vec_ok: n % 4 == 0, ldc % 4 == 0, c 8-byte aligned, bias 16-byte aligned
    bool addend;              // the call has one
    bool fast_disabled;       // GN_DISABLE_FAST=1
    bool join;                // a batch is open and the call carries GN_GEMM_JOIN_BATCH
    int compute_units;
};

struct GemmRoute {
    Gemm kernel;
    gn_status status;         // GN_OK, or the refusal's (the caller writes the message)
    Refusal why;
    bool queue;               // leaves with the open batch
    bool out_bf16;            // c is a bf16 table (split only)
    unsigned grid_x, grid_y, grid_z;   // of the kernel's own launch
    int64_t lds;              // dynamic LDS bytes.  deep: of the batched form (k_gemm_deep holds the same bytes statically)
    int mt, nt;               // deep: the tile template
    int gx, blocks;           // deep, lds: the batched form, workgroups [0, blocks) as a grid gx wide
    int row_tiles;            // lds, split
    int terms, ct, slab, ch;  // split: bf16 terms per operand, column tiles per wave, 32-deep chunks of B in LDS at a time, and
                              // the chunk count the kernel knows at compile time (0: any number)
};

inline GemmRoute gemm_refusal(gn_status status, Refusal why) {
    GemmRoute r{};
    r.kernel = Gemm::refused; r.status = status; r.why = why;
    return r;
}

inline GemmRoute gemm_route(const GemmCall& c) {
    const int64_t m = c.m, n = c.n, k = c.k;
    const bool at = (c.flags & GN_GEMM_A_TRANSPOSED) != 0, fast = (c.flags & GN_GEMM_ARITH_FAST) != 0;
    // a legal request beyond the grid's third dimension: the caller cuts it (as rgcn.hip does), not an argument error
    if (c.batch > 65535) return gemm_refusal(GN_ERR_UNSUPPORTED, Refusal::batch_limit);

    // The tall-skinny split kernel: the shape it wants (tall, or asked for by a caller whose products must not change kernel -
    // and bits - with their row count), and whether it runs.
    const bool split_shape = !at && (m >= 2048 || (c.flags & GN_GEMM_SPLIT_KERNEL)) && k >= 32 && k % 32 == 0 && c.a_vec_ok;
    const bool split = split_shape && c.batch == 1 && !c.a_rows && !c.fast_disabled;

    GemmRoute r{};
    r.status = GN_OK; r.why = Refusal::none;
    if (c.flags & GN_GEMM_OUT_BF16) {
        // only the split kernel stores a bf16 table.  (m >= 2048 even with GN_GEMM_SPLIT_KERNEL: preserves the parent's route)
        if (!split || m < 2048 || !c.bf16_vec_ok || (c.flags & GN_GEMM_ACCUMULATE) || c.addend || at)
            return gemm_refusal(GN_ERR_UNSUPPORTED, Refusal::out_bf16);
        r.out_bf16 = true;
    }
    r.row_tiles = (int)cdiv(m, 16);

    // Deep and narrow: a workgroup per output tile, K over its waves.
    //  - `at`: a product given A transposed comes here whatever k is and whatever GN_DISABLE_FAST says (preserves the parent's
    //    route: no other kernel reads a transposed A)
    //  - `!split_shape`, not `!split`: a shape of the split kernel stays off this one even where the split kernel will not run
    //    (GN_DISABLE_FAST=1, a row gather, batch > 1) and lands on k_gemm_f32 (preserves the parent's route)
    if (c.batch == 1 && !c.a_rows && (m <= 64 || n <= 32) && !split_shape && (at || (k >= 256 && !c.fast_disabled))) {
        r.kernel = Gemm::deep;
        if (m <= 64) {
            r.mt = m > 32 ? 4 : m > 16 ? 2 : 1; r.nt = 1;
            r.gx = 1; r.blocks = (int)cdiv(n, 16);
        } else {
            r.mt = 1; r.nt = n > 16 ? 2 : 1;
            r.gx = (int)cdiv(m, 16); r.blocks = r.gx;
        }
        r.grid_x = (unsigned)r.gx; r.grid_y = (unsigned)(r.blocks / r.gx); r.grid_z = 1;
        r.lds = 16 * r.mt * r.nt * kFragBytes;
        r.queue = c.join;
        return r;
    }
    if (at) return gemm_refusal(GN_ERR_INVALID_ARG, Refusal::a_transposed_shape);

    if (split) {
        // one shared B (as stored, or given transposed): the bf16 matrix instruction on split operands.  Never queued: on
        // 50,000 x 128 x 128 it takes a third of the fp32 instruction's time.
        r.kernel = Gemm::split;
        r.terms = fast ? 2 : 3;
        // a wave keeps 64 columns of a row tile, or 128 when the product is wider than 64 (A is then read once per 128)
        r.ct = n > 64 ? 8 : 4;
        // B in LDS: 2 bytes per term and element, at most 160 KB; a deeper K goes through in slabs
        const int64_t chunk_bytes = (int64_t)r.ct * r.terms * kFragBytes;
        r.slab = (int)std::min<int64_t>(k / 32, std::min<int64_t>(8, (160 * 1024) / chunk_bytes));
        r.lds = r.slab * chunk_bytes;
        const int64_t chunks = r.slab < k / 32 ? 0 : k / 32;
        r.ch = (chunks == 1 || chunks == 2 || chunks == 4 || (chunks == 8 && r.ct == 4)) ? (int)chunks : 0;
        // one persistent workgroup of sixteen waves per compute unit (and column block)
        r.grid_x = (unsigned)std::min<int64_t>(r.row_tiles, c.compute_units); r.grid_y = (unsigned)cdiv(n, 16 * r.ct); r.grid_z = 1;
        return r;
    }
    const int64_t b_bytes = cdiv(k, 16) * kColTiles * kFragBytes;   // B as fragments, per 64-column block
    if (c.batch == 1 && m >= 256 && b_bytes <= kLdsSmall && !c.fast_disabled) {
        // tall-skinny on the fp32 instruction, B in LDS: four waves per workgroup alone, sixteen in a batch
        r.kernel = Gemm::lds;
        r.lds = b_bytes;
        r.grid_x = (unsigned)std::min<int64_t>(cdiv(r.row_tiles, 4), 1024); r.grid_y = (unsigned)cdiv(n, 16 * kColTiles); r.grid_z = 1;
        r.gx = (int)std::min<int64_t>(cdiv(r.row_tiles, 16), 256); r.blocks = r.gx * (int)r.grid_y;
        r.queue = c.join && !c.a_rows;     // (joins a batch only without a row gather: preserves the parent's route)
        return r;
    }
    r.kernel = Gemm::general;
    r.grid_x = (unsigned)cdiv(m, 64); r.grid_y = (unsigned)cdiv(n, 16 * kColTiles); r.grid_z = (unsigned)c.batch;
    return r;
}

// ---- out[k1, k2] = x^T g over m rows ----------------------------------------------------------------------------------
enum class Xtg { wide, mfma, partial, unsupported };

struct XtgCall {
    int64_t m, k1, k2;        // m >= 0, k1 > 0, k2 > 0
    int flags;                // GN_XTG_*
    bool ws_aligned4;         // the workspace is 4-byte aligned
    bool fast_disabled;       // GN_DISABLE_FAST=1
    bool join;                // a batch is open and the call carries GN_XTG_JOIN_BATCH
    int compute_units;
};

struct XtgRoute {
    Xtg kernel;
    bool queue;               // may leave with the open batch (gemm.hip still asks whether a queued product owns the workspace)
    int slices;               // workgroups = row slices
    int64_t lds;              // dynamic LDS bytes
    int ti, tj, wpt;          // wide: tiles of 64 x 32 outputs, and the waves that share one
    int mt, nt;               // mfma: the tile template (16 x 16 tiles)
};

// about two chunks of sixteen rows per wave; up to 40 of them are 32 (one level), more are up to 128 (two)
inline int xtg_slices(int64_t m) {
    const int64_t want = cdiv(m, 16 * 16 * 2);
    return (int)std::max<int64_t>(1, want <= 40 ? std::min<int64_t>(kXtgMfmaSlices, want) : std::min<int64_t>(kXtgMfmaMax, want));
}

// a wide product: whole tiles of 64 x 32 outputs, 2 to 16 of them, that share a workgroup's sixteen waves evenly
inline bool xtg_wide(int64_t m, int64_t k1, int64_t k2, bool fast_disabled) {
    if (fast_disabled || m < 4096 || k1 < 64 || k2 < 32 || k1 % 64 != 0 || k2 % 32 != 0 || k1 > 256 || k2 > 128) return false;
    const int64_t tiles = (k1 / 64) * (k2 / 32);
    return tiles >= 2 && tiles <= 16 && 16 % tiles == 0;
}

inline XtgRoute xtg_route(const XtgCall& c) {
    const int64_t m = c.m, k1 = c.k1, k2 = c.k2;
    XtgRoute r{};
    if (xtg_wide(m, k1, k2, c.fast_disabled)) {
        // all tiles of a row slice in one workgroup, then the fold (two launches whatever the width; never queued)
        r.kernel = Xtg::wide;
        r.ti = (int)(k1 / 64); r.tj = (int)(k2 / 32); r.wpt = 16 / (r.ti * r.tj);
        r.slices = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kXtgSlices, c.compute_units), cdiv(m, 16) / (2 * r.wpt)));
        r.lds = r.wpt > 1 ? 16 * 8 * kFragBytes : 0;
        return r;
    }
    if (k1 * k2 > 4096) {
        r.kernel = Xtg::unsupported;
        return r;
    }
    // one launch on the matrix cores.  (It needs the caller's promise of a zeroed ticket and a workspace it can draw tickets
    // from; without either the LDS kernel runs: preserves the parent's route)
    if (m > 0 && k1 <= 64 && k2 <= 32 && (c.flags & GN_XTG_TICKET_ZEROED) && c.ws_aligned4 && !c.fast_disabled) {
        r.kernel = Xtg::mfma;
        r.mt = (int)cdiv(k1, 16); r.nt = (int)cdiv(k2, 16);
        r.slices = xtg_slices(m);
        r.lds = 16 * r.mt * r.nt * kFragBytes;
        r.queue = c.join;
        return r;
    }
    r.kernel = Xtg::partial;
    r.slices = (int)std::max<int64_t>(1, std::min<int64_t>(kXtgSlices, cdiv(m, 16)));
    r.lds = kXtgMaxRows * (k1 + 1 + k2) * (int64_t)sizeof(float);
    return r;
}

}  // namespace route
}  // namespace gn
