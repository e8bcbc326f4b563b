// Which kernel serves a call of the multi-relational layer, with which template arguments and which workspace layout, and
// whether the call is admissible at all: the one place where the forward entry points of rgcn.hip (gn_rgcn_forward_f32,
// gn_rgcn_forward_weighted_f32, gn_rgcn_finalize_f32), its exported queries (gn_rgcn_workspace_bytes, gn_rgcn_forward_path,
// gn_rgcn_forward_choice, gn_rgcn_weighted_supported, gn_rgcn_weighted_workspace_bytes) and the launch functions of
// rgcn_pair.hip, rgcn_fast.hip and rgcn_basis.hip read it.  Pure host arithmetic on the facts of a validated call - no HIP in
// here, no allocation, no getenv, no formatting - so that this file also builds with plain g++, where
// tests/rgcn_route_host.cpp prints the route of every boundary shape (tests/test_rgcn_route.py holds the table).
//
//   request    ladder, first rule that holds                                              kernel
//   forward    flag bits the entry does not define; GN_RGCN_SUM with GN_RGCN_PARTIAL       refused (GN_ERR_INVALID_ARG)
//              GN_RGCN_SUM: general covers the shapes (32 tiles), table not forced         general   k_rgcn_basis<BT, NT, false>
//              GN_RGCN_SUM otherwise                                                       table
//              pair forced, pair covers the call                                           pair      k_rgcn_pair<NT, BT, TERMS, .>
//              lds forced, lds covers the call                                             lds       k_rgcn_lds<FIN, ., .>
//              table forced                                                                table
//              general forced: general covers the shapes (16 tiles), else table            general | table
//              pair covers the call                                                        pair
//              lds covers the call                                                         lds
//              general covers the shapes (16 tiles)                                        general
//              otherwise                                                                   table     gn_gemm_f32 x 2, launch_aggregate
//              then: GN_RGCN_BASIS_TRANSPOSED on a kernel other than pair                  refused (GN_ERR_UNSUPPORTED)
//   weighted   flags other than GN_RGCN_SUM or GN_RGCN_PARTIAL alone                       refused (GN_ERR_INVALID_ARG)
//              general covers the shapes (32 tiles), else                                  general   k_rgcn_basis<BT, NT, edges > 0>
//                                                                                          refused (GN_ERR_UNSUPPORTED)
//   finalize   fast paths on, fin <= 64 -> 32, summed 16-byte aligned with ld 32           slab_finalize   k_rgcn_slab_finalize
//              otherwise                                                                   gemm_finalize   gn_gemm_f32, k_rgcn_finalize
//
//   pair covers     fast paths on, the plan has the pair schedule, fin in {16, 32, 48, 64}, 1..32 bases, fout % 4 in 4..64,
//                   (fin / 16) * ceil(bases / 16) <= 6 tiles, <= 16 rows of basis a thread (12 at fin 48), basis 16-byte aligned
//   lds covers      fast paths on, the plan has the work items, fin in {16, 32, 48, 64} -> 32, x unknown or 16-byte aligned
//                   with ld_x % 4 == 0
//   general covers  the plan has the rows' degree order, fin <= 128, bases <= 64, ceil(bases / 16) * ceil(fin / 16) tiles
//
// GN_DISABLE_FAST=1 (fast_disabled) leaves general, table and gemm_finalize.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "gripnet_hip.h"
#include "layout_rgcn_basis.hpp"
#include "layout_rgcn_fast.hpp"
#include "layout_rgcn_pair.hpp"

namespace gn {
namespace route {

enum class RelKind { forward, weighted, finalize };
enum class RelKernel { pair, lds, general, table, slab_finalize, gemm_finalize, refused };
enum class RelRefusal { none, undefined_flags, sum_with_partial, weighted_flags, basis_transposed, weighted_shapes };

struct RelCall {
    RelKind kind;
    // the plan
    int64_t num_nodes, num_relations, shard_edges;
    bool pair_ok, fast_ok;             // the destination-major schedule, the LDS kernel's work items
    int fast_groups;                   //   and its persistent workgroups
    bool row_order;                    // the rows' degree order (the general kernel deals rows in it)
    // the call: widths, flags, and each pointer's bytes past a 16-byte boundary
    int64_t fin, fout, bases;
    int flags;
    bool x_known;                      // false: a query without x answers for an aligned one
    int64_t ld_x;
    unsigned x_at, basis_at;
    int64_t ld_summed;                 // finalize
    unsigned summed_at;
    // the environment, read by the caller
    bool fast_disabled;                // GN_DISABLE_FAST
    int64_t slab_bytes;                // gn_layout::kSlabBytes, or what GN_RGCN_SLAB_MB says
};

struct RelRoute {
    RelKernel kernel;
    gn_status status;                  // GN_OK, or the refusal's (the caller writes the message)
    RelRefusal why;
    int nt, bt, terms;                 // tiles of 16 input features and of 16 bases; bf16 terms of a split operand
    bool wt;                           // general: the instantiation that reads edge factors
    size_t workspace;                  // bytes the kernel writes: what the entry point asks of the caller
    // general: [basis ; root ; 0] of kp rows | the slabs' work counters | (several slabs) heavy counts, the slabs' own orders | a slab of U
    int kp;
    int64_t slab_rows, slabs;
    size_t w_off, q_off, o_off, u_off;
    // table: W [R, fin * fout] (at w_off) | H [R, N, fout] | x root + bias [N, fout]
    size_t h_off, xr_off;
    // lds: W_r transposed, then the workgroups' slabs
    size_t lds_w_bytes;
};

inline size_t rel_align(size_t v) { return (v + 255) & ~size_t(255); }

// ---- what each kernel covers ------------------------------------------------------------------------------------------------
inline bool rel_pair_covers(const RelCall& c) {
    using namespace gn_layout;
    if (!c.pair_ok || c.fast_disabled) return false;
    if (c.fin % 16 != 0 || c.fin < 16 || c.fin > kPairMaxFin || c.bases < 1 || c.bases > kPairMaxBases || c.fout % 4 != 0 || c.fout < 4 ||
        c.fout > kPairMaxFout)
        return false;
    const int64_t nt = c.fin / 16, bt = (c.bases + 15) / 16;
    // the waves' shares of U in LDS: 16 waves x 3 rows x (16 bt x fin) floats, plus the slices' sums behind wave 0's
    const int64_t kp = (16 * bt + 4) * c.fin;                                          // (four pad floats per feature, see the kernel)
    const int64_t part = (int64_t)(kPairWaves + kPairMaxD) * kp * 4;                   // the waves' shares, the rows' sums
    const int64_t red = (int64_t)kPairThreads * kPairMaxD * 16 + (int64_t)kPairThreads * 16;   // the slices' sums (padded) reuse the shares' space
    const int64_t slices = kPairThreads / (c.fout / 4), per = (c.bases * c.fin + slices - 1) / slices;
    const int64_t need = (int64_t)kPairWaves * kp >= (int64_t)kPairThreads * kPairMaxD * 4 + kPairThreads * 4 ? std::max(part, red)
                                                                                                              : part + red;   // (narrow layers: behind the sums)
    // need <= kPairLdsBytes cannot bind inside the other clauses: six tiles bound kp by 36 * 48 = 1728 floats, so the shares
    // take at most 19 * 1728 * 4 = 131,328 bytes (more than the sums' 65,536), and below kp = 1024, where the two add up, at
    // most 77,824 + 65,536.  Nor can the 16 rows of basis a thread: below fin 48 a thread holds at most 32 * 32 / 64.  Both
    // stay: they state what the kernel's LDS map and its epilogue's registers hold.
    return need <= kPairLdsBytes && nt * bt <= kPairMaxTiles && per <= (nt <= 2 ? kPairRegRows : kPairRegRowsWide) &&   // (rows of basis a thread holds in registers)
           c.basis_at == 0;
}

inline bool rel_lds_covers(const RelCall& c) {
    using namespace gn_layout;
    if (!c.fast_ok || c.fast_disabled) return false;
    if (c.fout != kFastFout || c.fin % 16 != 0 || c.fin < 16 || c.fin > kFastMaxFin || c.bases < 1) return false;   // (bases < 1 cannot bind: a validated call has one)
    return !c.x_known || (c.ld_x % 4 == 0 && c.x_at == 0);                             // (16-byte row loads)
}

// `tiles`: kBasisTiles accumulator tiles for the mean, kBasisTilesSum for the sum and the weighted calls
inline bool rel_general_covers(const RelCall& c, int tiles) {
    if (!c.row_order || c.fin < 1 || c.fin > 128 || c.bases < 1 || c.bases > 64 || c.fout < 1) return false;   // (the lower bounds bind for the weighted queries alone: every other caller has validated them)
    return ((c.bases + 15) / 16) * ((c.fin + 15) / 16) <= tiles;
}

// ---- the workspaces ---------------------------------------------------------------------------------------------------------
inline void rel_general_layout(const RelCall& c, RelRoute& r) {
    const int64_t rows = std::max<int64_t>(c.num_nodes, 1);
    r.bt = (int)((c.bases + 15) / 16); r.nt = (int)((c.fin + 15) / 16);
    r.kp = (int)(((c.bases + 1) * c.fin + 31) / 32 * 32);
    r.slab_rows = std::min<int64_t>(rows, std::max<int64_t>(256, c.slab_bytes / ((int64_t)r.kp * 4)));
    r.slab_rows = std::max<int64_t>(r.slab_rows, (rows + 255) / 256);                  // at most 256 slabs (one work counter each)
    r.slabs = (rows + r.slab_rows - 1) / r.slab_rows;
    r.w_off = 0;
    r.q_off = rel_align((size_t)r.kp * c.fout * sizeof(float));
    r.o_off = r.q_off + rel_align((size_t)r.slabs * sizeof(unsigned int));
    r.u_off = r.o_off + (r.slabs > 1 ? rel_align(((size_t)r.slabs + (size_t)c.num_nodes) * sizeof(int32_t)) : 0);
    r.workspace = r.u_off + (size_t)r.slab_rows * r.kp * sizeof(float);
}

inline void rel_table_layout(const RelCall& c, RelRoute& r) {
    r.w_off = 0;
    r.h_off = rel_align((size_t)c.num_relations * c.fin * c.fout * sizeof(float));
    r.xr_off = r.h_off + rel_align((size_t)c.num_relations * c.num_nodes * c.fout * sizeof(float));
    r.workspace = r.xr_off + rel_align((size_t)c.num_nodes * c.fout * sizeof(float));
}

inline void rel_lds_layout(const RelCall& c, RelRoute& r) {
    r.lds_w_bytes = rel_align((size_t)c.num_relations * c.fin * c.fout * sizeof(float));
    r.workspace = r.lds_w_bytes + (size_t)c.fast_groups * c.num_nodes * c.fout * sizeof(float);
}

// ---- the route --------------------------------------------------------------------------------------------------------------
inline RelRoute rel_refusal(gn_status status, RelRefusal why) {
    RelRoute r{};
    r.kernel = RelKernel::refused; r.status = status; r.why = why;
    return r;
}

// The forward's ladder.  A forced kernel that does not cover the call is not taken.
inline RelKernel rel_forward_kernel(const RelCall& c) {
    using namespace gn_layout;
    const int forced = (c.flags >> GN_RGCN_PATH_SHIFT) & 7;
    if (c.flags & GN_RGCN_SUM)             // the sum's epilogue lives in the general kernel's slab product and in the table kernel's gather
        return (forced != GN_RGCN_PATH_TABLE && rel_general_covers(c, kBasisTilesSum)) ? RelKernel::general : RelKernel::table;
    const bool pair = rel_pair_covers(c), lds = rel_lds_covers(c), general = rel_general_covers(c, kBasisTiles);
    if (forced == GN_RGCN_PATH_PAIR && pair) return RelKernel::pair;
    if (forced == GN_RGCN_PATH_LDS && lds) return RelKernel::lds;
    if (forced == GN_RGCN_PATH_TABLE) return RelKernel::table;
    if (forced == GN_RGCN_PATH_GENERAL) return general ? RelKernel::general : RelKernel::table;
    if (pair) return RelKernel::pair;
    if (lds) return RelKernel::lds;
    return general ? RelKernel::general : RelKernel::table;
}

inline RelRoute rel_route(const RelCall& c) {
    using namespace gn_layout;
    RelRoute r{};
    r.status = GN_OK; r.why = RelRefusal::none;
    r.terms = (c.flags & GN_RGCN_ARITH_FAST) ? 2 : 3;
    if (c.kind == RelKind::finalize) {
        // the all-reduced [n, 32] sum is one "slab" of the LDS kernel's finalisation; else the root term's product, then the mean
        const bool slab = !c.fast_disabled && c.fout == kFastFout && c.fin >= 1 && c.fin <= kFastMaxFin && c.ld_summed == kFastFout &&
                          c.summed_at == 0;
        r.kernel = slab ? RelKernel::slab_finalize : RelKernel::gemm_finalize;
        return r;
    }
    if (c.kind == RelKind::weighted) {
        if (c.flags != GN_RGCN_SUM && c.flags != GN_RGCN_PARTIAL) return rel_refusal(GN_ERR_INVALID_ARG, RelRefusal::weighted_flags);
        if (!rel_general_covers(c, kBasisTilesSum)) return rel_refusal(GN_ERR_UNSUPPORTED, RelRefusal::weighted_shapes);
        r.kernel = RelKernel::general; r.wt = c.shard_edges > 0;                       // (no edges: no factor is read)
        rel_general_layout(c, r);
        return r;
    }
    if (c.flags & ~(GN_RGCN_PARTIAL | GN_RGCN_ARITH_FAST | GN_RGCN_BASIS_TRANSPOSED | GN_RGCN_SUM | (7 << GN_RGCN_PATH_SHIFT)))
        return rel_refusal(GN_ERR_INVALID_ARG, RelRefusal::undefined_flags);
    if ((c.flags & GN_RGCN_SUM) && (c.flags & GN_RGCN_PARTIAL)) return rel_refusal(GN_ERR_INVALID_ARG, RelRefusal::sum_with_partial);
    r.kernel = rel_forward_kernel(c);
    if ((c.flags & GN_RGCN_BASIS_TRANSPOSED) && r.kernel != RelKernel::pair) return rel_refusal(GN_ERR_UNSUPPORTED, RelRefusal::basis_transposed);
    switch (r.kernel) {
        case RelKernel::pair: r.nt = (int)(c.fin / 16); r.bt = (int)((c.bases + 15) / 16); break;   // (no workspace)
        case RelKernel::lds: rel_lds_layout(c, r); break;
        case RelKernel::general: rel_general_layout(c, r); break;
        default: rel_table_layout(c, r); break;
    }
    return r;
}

}  // namespace route
}  // namespace gn
