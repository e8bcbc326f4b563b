// Which kernel serves a gather-reduce, with which grid, block and LDS size, and whether the call is admissible at all: the one
// place where the forward entry points (graph.hip, graph_bf16.hip), the plain sums of rgcn.hip and gn_graph_aggregate_t_f32,
// the exported queries (gn_*_fusable, gn_graph_*_applicable) and aggregate.hip's launch functions read it.  Pure host
// arithmetic on the facts of a validated call - no HIP in here, no allocation, no formatting - so that this file also builds
// with plain g++, where tests/gather_route_host.cpp prints the route of every boundary shape (tests/test_gather_route.py holds
// the table).
//
//   request       ladder, first rule that holds                                    kernel (aggregate.hip unless named)
//   fp32 table    LDS-staged plan, its switch on, operands in column groups        blocked (gcn_blocked.hip: its own geometry)
//                 weight, 64|128 -> 64..128 (% 16, >= in), rows >= 4096, short rows mfma            k_aggregate_mfma<LPE>
//                 weight, 16 -> 16 (GN_DISABLE_QUAD: the next row)                 transform_quad  k_aggregate_transform_q<1>
//                 weight, {16,32,64} -> 16 or {32,64} -> 32                        transform       k_aggregate_transform<LPE, FOUT>
//                 weight, anything else                                            refused
//                 16-byte rows, lpe 4..16, rows >= 65536, < 8 a row, a bare sum over a table of <= 128 KB
//                                                                                  lds_table       k_aggregate_lds_table<LPE>
//                 16-byte rows, lpe <= 16, < GN_AGG_SHORT_MAX_DEG a row            short_rows      k_aggregate_short<LPE>
//                 16-byte rows, lpe <= 32, < GN_AGG_GROUP_MAX_DEG a row            group           k_aggregate_group<RowF32, LPE, U>
//                 16-byte rows                                                     wave            k_aggregate<RowF32, LPE>
//                 otherwise                                                        wave_scalar     k_aggregate<RowScalar, LPE>
//   bf16 table    lpe <= 32, < GN_AGG_GROUP_MAX_DEG a row, rows >= 4096            bf16_group      k_aggregate_group<RowBf16, LPE, U>
//                 otherwise                                                        bf16_wave       k_aggregate<RowBf16, LPE>
//   tail          64 -> 16 over 16-byte rows, else refused                         transform_tail  k_aggregate_transform_tail
//   split source  64 -> 16, head of 16|32|48 columns, 16-byte rows, else refused   transform_split k_aggregate_transform_split<16>
//
// GN_DISABLE_FAST=1 leaves wave, wave_scalar and bf16_wave, and refuses every call that brings a weight.
#pragma once

#include <algorithm>
#include <cstdint>

#include "gripnet_hip.h"

// Upper bound of the launch grid (blocks of four waves); rows beyond it are taken grid-stride.
#ifndef GN_AGG_GRID
#define GN_AGG_GRID (256 * 8)
#endif
// Average row length below which LPE lanes own a row (k_aggregate_short: two gathers in flight per lane; k_aggregate_group:
// GN_AGG_GROUP_U of them) instead of a wave
#ifndef GN_AGG_SHORT_MAX_DEG
#define GN_AGG_SHORT_MAX_DEG 8
#endif
#ifndef GN_AGG_GROUP_MAX_DEG
#define GN_AGG_GROUP_MAX_DEG 48
#endif

namespace gn {
namespace route {

constexpr int kGatherWave = 64;                      // lanes of a wave
constexpr int64_t kLdsTableRows = 65536;             // destination rows from which the LDS-table kernel pays,
constexpr int64_t kLdsTableMaxDeg = 8;               // the average row length below which,
constexpr int64_t kLdsTableBytes = 128 * 1024;       // and the gathered table it holds at the most (plus one zero row)
constexpr int64_t kMfmaRows = 4096;                  // destination rows from which k_aggregate_mfma pays
constexpr int64_t kBf16GroupRows = 4096;             // and from which lane groups own the rows of a bf16 table

inline int64_t gather_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// lanes a feature row of `units` 16-byte (or scalar) loads takes: the next power of two, one wave at the most
inline int lanes_per_row(int64_t units) {
    int lpe = 1;
    while (lpe < units && lpe < kGatherWave) lpe <<= 1;
    return lpe;
}

enum class Gather { blocked, mfma, transform, transform_quad, transform_tail, transform_split, lds_table, short_rows, group, wave,
                    wave_scalar, bf16_group, bf16_wave, refused };
enum class Source { f32, bf16, tail, split };
enum class GatherRefusal { none, no_fused_transform, tail_operands, split_fast_off, split_widths, split_head_cols, split_alignment,
                           split_ld_multiple, split_ld_short, split_ld_31_bits };

struct GatherCall {
    Source kind;
    // the plan
    int64_t rows, nnz, table_rows;     // nnz, table_rows: -1 where the caller does not know them
    bool blk_ok; int blk_cw, blk_cols; // its LDS-staged encoding
    // the operands: widths, leading dimensions, and each pointer's bytes past a 16-byte boundary
    int64_t features, fout;            // gathered row, written row (without a weight: the same)
    bool weight;
    int64_t ld_table, ld_out;          // (split source: ld_table is the head's, ld_head)
    unsigned table_at, out_at, bias_at, weight_at;
    bool coef, rowdiv, addend, bias, relu, side;
    bool planes;                       // split planes were offered
    int64_t head_cols, ld_tail;        // split source
    bool head, tail;                   //   both tables are there
    unsigned tail_at;
    unsigned tail_w_at, tail_b_at;     // tail transform
    // the environment, read by the caller (a switch whose rule the call cannot reach may stay false)
    bool fast_disabled, quad_disabled, lds_table_disabled, blocked_disabled;     // GN_DISABLE_FAST / _QUAD / _LDS_TABLE / _BLOCKED
    int compute_units;
};

struct GatherRoute {
    Gather kernel;
    gn_status status;                  // GN_OK, or the refusal's (the caller writes the message)
    GatherRefusal why;
    int lpe;                           // lanes per gathered row: the kernel's template argument
    unsigned grid, block;              // (blocked: gcn_blocked.hip has its own)
    int64_t lds;                       // dynamic LDS bytes
    int row_blocks;                    // mfma: blocks of 16 * (64 / lpe) rows, a kernel argument
    bool planes_by_kernel;             // the kernel writes the offered planes in its epilogue (false: the stand-alone split follows)
};

// ---- the rules, each asked by gather_route and by the exported query of the same name -------------------------------------
// The shuffle / quad epilogue's width pairs.  (16 -> 32 has no fused transform - its K slice per lane would be two floats:
// preserves the parent's route)
inline bool transform_fusable(int64_t fin, int64_t fout, bool fast_disabled) {
    if (fast_disabled) return false;
    return (fout == 16 && (fin == 16 || fin == 32 || fin == 64)) || (fout == 32 && (fin == 32 || fin == 64));
}

// The matrix-core form: rows of up to GN_AGG_GROUP_MAX_DEG neighbours on average (longer rows belong to a wave each: the
// product first, then k_aggregate).  (rows >= 4096 and fout >= fin: preserves the parent's route)
inline bool mfma_fusable(int64_t fin, int64_t fout, int64_t rows, int64_t nnz, bool fast_disabled) {
    if (fast_disabled) return false;
    if (!(fin == 64 || fin == 128) || fout % 16 != 0 || fout < fin || fout > 128) return false;
    return nnz >= 0 && nnz < GN_AGG_GROUP_MAX_DEG * rows && rows >= kMfmaRows;
}

// The LDS-staged path: the gather writes out (and reads bias) in column groups of blk_cw floats, so an output slice at an odd
// column or with an odd stride keeps the wave-per-row kernels
inline bool blocked_applicable(const GatherCall& c) {
    if (!c.blk_ok || c.fast_disabled || c.blocked_disabled) return false;
    const unsigned group = 4u * (unsigned)c.blk_cw;
    if (c.ld_out % c.blk_cw != 0 || c.out_at % group != 0 || (c.bias && c.bias_at % group != 0)) return false;
    if (!(c.fout == 16 || c.fout == 32) || c.fout > c.blk_cols) return false;
    if (c.weight) {
        if (!(c.features == 16 || c.features == 32 || c.features == 64) || c.weight_at != 0) return false;
    } else if (c.features != c.fout) {
        return false;
    }
    return c.ld_table % 4 == 0 && c.table_at == 0;
}

// Why the split-source form does not take these operands (none: it does)
inline GatherRefusal split_source_refusal(const GatherCall& c) {
    if (c.fast_disabled) return GatherRefusal::split_fast_off;
    if (c.features != 64 || c.fout != 16) return GatherRefusal::split_widths;
    if (c.head_cols != 16 && c.head_cols != 32 && c.head_cols != 48) return GatherRefusal::split_head_cols;
    if (!c.head || !c.tail || c.table_at != 0 || c.tail_at != 0) return GatherRefusal::split_alignment;
    if (c.ld_table % 4 != 0 || c.ld_tail % 4 != 0) return GatherRefusal::split_ld_multiple;
    if (c.ld_table < c.head_cols || c.ld_tail < c.features - c.head_cols) return GatherRefusal::split_ld_short;
    if (c.ld_table >= (1ll << 31) || c.ld_tail >= (1ll << 31)) return GatherRefusal::split_ld_31_bits;
    return GatherRefusal::none;
}

// ---- the route ----------------------------------------------------------------------------------------------------------
inline GatherRoute gather_refusal(GatherRefusal why) {
    GatherRoute r{};
    r.kernel = Gather::refused; r.status = GN_ERR_UNSUPPORTED; r.why = why;
    return r;
}

inline GatherRoute gather_route(const GatherCall& c) {
    const int64_t rows = c.rows;
    GatherRoute r{};
    r.status = GN_OK; r.why = GatherRefusal::none; r.block = 256;
    // a wave per destination row, four to a workgroup: the shuffle, quad, tail and split transforms and k_aggregate
    const unsigned wave_grid = (unsigned)std::min<int64_t>(gather_cdiv(rows, 4), GN_AGG_GRID);
    auto lane_group_grid = [&] { return (unsigned)gather_cdiv(rows * r.lpe, 256); };   // one row per lane group, no grid-stride loop

    if (c.kind == Source::bf16) {
        // 16 bytes = 8 bf16 features per lane.  Many short rows (the node-classification graphs): lane groups own rows.
        // (rows >= 4096, which the fp32 rule below does not ask: preserves the parent's route)
        r.lpe = lanes_per_row(c.features / 8);
        if (r.lpe <= 32 && c.nnz < GN_AGG_GROUP_MAX_DEG * rows && rows >= kBf16GroupRows && !c.fast_disabled) {
            r.kernel = Gather::bf16_group; r.grid = lane_group_grid();
        } else {
            r.kernel = Gather::bf16_wave; r.grid = wave_grid;
        }
        return r;
    }
    if (c.kind == Source::tail) {
        if (c.features != 64 || c.fout != 16 || c.fast_disabled || c.ld_table % 4 != 0 || c.table_at != 0 || c.tail_w_at != 0 ||
            c.tail_b_at != 0)
            return gather_refusal(GatherRefusal::tail_operands);
        r.kernel = Gather::transform_tail; r.lpe = 16; r.grid = wave_grid; r.planes_by_kernel = c.planes;
        return r;
    }
    if (c.kind == Source::split) {
        const GatherRefusal why = split_source_refusal(c);
        if (why != GatherRefusal::none) return gather_refusal(why);
        r.kernel = Gather::transform_split; r.lpe = 16; r.grid = wave_grid; r.planes_by_kernel = c.planes;
        return r;
    }

    if (blocked_applicable(c)) {
        r.kernel = Gather::blocked; r.grid = 0; r.block = 0;
        return r;
    }
    const bool table_vec = c.ld_table % 4 == 0 && c.table_at == 0;
    if (c.weight) {
        r.lpe = (int)(c.features / 4);
        if (mfma_fusable(c.features, c.fout, rows, c.nnz, c.fast_disabled) && table_vec) {
            // wide layers: W on the matrix cores.  A workgroup per block of rows at 64 features, persistent ones at 128 (see
            // k_aggregate_mfma); W as three bf16 terms and two row buffers in LDS
            const int rpi = 16 * (kGatherWave / r.lpe);
            r.kernel = Gather::mfma; r.block = 1024;
            r.row_blocks = (int)gather_cdiv(rows, rpi);
            r.grid = (unsigned)(r.lpe == 16 ? r.row_blocks : std::min(r.row_blocks, c.compute_units));
            r.lds = c.features * c.fout * 6 + 2 * (int64_t)rpi * (c.features + 4) * (int64_t)sizeof(float);
            return r;
        }
        // aggregate the input rows, then contract with W in the epilogue
        if (!transform_fusable(c.features, c.fout, c.fast_disabled) || !table_vec) return gather_refusal(GatherRefusal::no_fused_transform);
        // 16-wide rows: quad gathers (14.8 vs 16.4 us on the second gene layer of pose0-syn); 32-wide rows are faster with
        // one 16-byte load per lane and neighbour (k_aggregate_transform<8, 16> 19.2 us, the quad form 21.5).  The quad
        // kernel does not write split planes.
        const bool quad = c.features == 16 && c.fout == 16 && !c.quad_disabled;
        r.kernel = quad ? Gather::transform_quad : Gather::transform;
        r.grid = wave_grid; r.planes_by_kernel = c.planes && !quad;
        return r;
    }

    const bool vec = c.features % 4 == 0 && table_vec && c.ld_out % 4 == 0 && c.out_at == 0;
    r.lpe = lanes_per_row(vec ? c.features / 4 : c.features);
    const bool fast = vec && !c.fast_disabled;
    if (fast && r.lpe >= 4 && r.lpe <= 16 && c.nnz > 0 && c.nnz < kLdsTableMaxDeg * rows && rows >= kLdsTableRows && !c.coef && !c.rowdiv &&
        !c.addend && !c.bias && !c.relu && !c.side && c.table_rows > 0 &&
        c.table_rows * c.features * (int64_t)sizeof(float) <= kLdsTableBytes && !c.lds_table_disabled) {
        // many short rows over a table that fits the LDS, nothing but a plain sum: the table is gathered from there.
        // (lpe >= 4, where the short-row kernel below takes narrower rows too: preserves the parent's route)
        r.kernel = Gather::lds_table; r.block = 1024;
        r.grid = (unsigned)std::min<int64_t>(256, gather_cdiv(rows * r.lpe, 2 * 1024));
        r.lds = (c.table_rows + 1) * c.features * (int64_t)sizeof(float);
    } else if (fast && r.lpe <= 16 && c.nnz >= 0 && c.nnz < GN_AGG_SHORT_MAX_DEG * rows) {
        r.kernel = Gather::short_rows;
        r.grid = (unsigned)std::min<int64_t>(gather_cdiv(rows * r.lpe, 256), GN_AGG_GRID);
    } else if (fast && r.lpe <= 32 && c.nnz >= 0 && c.nnz < GN_AGG_GROUP_MAX_DEG * rows) {
        r.kernel = Gather::group; r.grid = lane_group_grid();
    } else {
        r.kernel = vec ? Gather::wave : Gather::wave_scalar; r.grid = wave_grid;
    }
    return r;
}

}  // namespace route
}  // namespace gn
