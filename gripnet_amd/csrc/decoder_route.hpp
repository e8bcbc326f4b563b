// Which kernel serves a forward call of the DistMult decoder, with which template arguments, grid, block and LDS size, with
// which column phases, workgroup split, staging and partial-sum room, and whether the call is admissible at all: the one place
// where the forward entry points of distmult.hip (gn_distmult_forward_f32), distmult_fast.hip (gn_distmult_packed_forward_f32)
// and distmult_plan.hip (gn_distmult_plan_forward_f32, gn_distmult_plan_forward_cols_f32) and their launch functions read it.
// Pure host arithmetic on the facts of a validated call - no HIP in here, no allocation, no getenv, no formatting - so that
// this file also builds with plain g++, where tests/decoder_route_host.cpp prints the route of every boundary shape
// (tests/test_decoder_route.py holds the table).
//
//   request   ladder, first rule that holds                                                 kernel
//   raw       lds covers the call                                                           lds_raw         k_distmult_lds<false>
//             vector ok                                                                     general_vec     k_distmult<4>
//             otherwise                                                                     general_scalar  k_distmult<1>
//   packed    n <= 65535, r <= 65535, lds covers the call                                   lds_packed      k_distmult_lds<true>
//             otherwise                                                                     refused (GN_ERR_UNSUPPORTED, packed_shape)
//   planned   the plan has the row-class encoding, fast paths on, 1 or 2 column parts,
//             f % 16 == 0, f <= the plan's features, (f / 16, first part / 16) among
//             (5,3) (5,4) (4,4) (3,3) (2,2) (1,1): rows with the arguments (<= 256 groups)  cls             k_distmult_class<J, J1>
//                                                  rows from the descriptors                cls_wide        k_distmult_class_wide<J, J1>
//             the plan has the row-class encoding only (no batches)                         refused (GN_ERR_UNSUPPORTED, class_only)
//             lds covers the call                                                           phase           k_distmult_plan
//             otherwise                                                                     refused (GN_ERR_UNSUPPORTED, planned_shape)
//
//   vector ok    f % 4 == 0, ld_z % 4 == 0, ld_d % 4 == 0, z and d 16-byte aligned
//   lds covers   fast paths on, vector ok, 1..4 column phases (plan_phases: n rows of 16 columns fit kLdsBudget, n <= 2400)
//
// planned: n, e and the plan's facts are the plan's, f = col_hi - col_lo, and c0[] counts from column 0 of z.
// GN_DISABLE_FAST=1 (fast_disabled) leaves general_vec and general_scalar.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "gripnet_hip.h"

namespace gn {
namespace route {

constexpr int kMaxPhases = 8;
constexpr size_t kLdsBudget = 150 * 1024;   // of 160 KB; the rest is left to the runtime
constexpr int64_t kLdsCu = 160 * 1024;      // the compute unit's LDS: what the kernels opt in to
constexpr int kLdsMaxPhases = 4;            // beyond that the general (L2-gather) kernel is the better choice
constexpr int64_t kDecoderGroups = 256;     // one workgroup per CU
constexpr int64_t kGeneralMaxBlocks = 256 * 8;   // k_distmult: blocks of four waves, edges beyond them are taken grid-stride

inline int64_t decoder_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Column phases: as few as possible; each at most 64 columns (4 lanes x 4 chunks x float4) with
// n x width x 4 B inside the LDS budget; widths are multiples of 16 columns except the last.
inline int plan_phases(int64_t n, int64_t f, int* c0, int* width) {
    if (n <= 0 || f <= 0 || f % 4 != 0) return 0;
    int64_t max_w = (int64_t)(kLdsBudget / (n * 4)) / 16 * 16;
    if (max_w > 64) max_w = 64;
    if (max_w < 16) return 0;
    const int64_t phases = decoder_cdiv(f, max_w);
    if (phases > kMaxPhases) return 0;
    int64_t c = 0;
    int k = 0;
    while (c < f) {
        const int64_t w = std::min(max_w, f - c);
        c0[k] = (int)c;
        width[k] = (int)w;
        c += w;
        ++k;
    }
    return k;
}

// LDS rows keep one stride for all phases, an odd number of 64-byte slots where there is room: a quad reads
// 64 contiguous bytes of a row, and with rows 128 bytes apart (a 32-column phase) the four quads of a
// 16-lane access group would share only two of the four 64-byte bank slots.
inline int lds_stride4(int64_t n, int max_w) {
    int stride4 = max_w / 4;
    if ((stride4 / 4) % 2 == 0 && (size_t)n * (stride4 + 4) * 16 <= kLdsBudget + 8 * 1024) stride4 += 4;
    return stride4;
}

// The raw list's triples staged in LDS behind the table (DmFastArgs): what a table fill and a pass over the list cost
constexpr double kStageFillBytesPerUs = 1.0e7;     // every workgroup reads the whole phase table again: ~3 us each at this size
constexpr double kStageStreamBytesPerUs = 5.0e6;   // the list streams at ~5 TB/s
constexpr double kStageTripleBytes = 24.0;         // (u, v, r) as int64: what a pass over the list moves per edge and phase
constexpr int64_t kStageMinTile = 1024;            // edges: a tile of a useful size

enum class DecoderKind { raw, packed, planned };
enum class DecoderKernel { general_vec, general_scalar, lds_raw, lds_packed, cls, cls_wide, phase, refused };
enum class DecoderRefusal { none, packed_shape, class_only, planned_shape };

struct DecoderCall {
    DecoderKind kind;
    int64_t n, f, r, e;                // nodes, columns of this launch, relations (planned: unread), edges
    int64_t ld_z, ld_d;
    unsigned z_at, d_at;               // each pointer's bytes past a 16-byte boundary
    int64_t col_lo, col_hi, num_features;   // planned: the launch's columns of the features (raw, packed: 0, f, f)
    // the plan's facts (planned)
    bool cls_ok;                       // it holds the row-class encoding,
    int cls_features, cls_groups;      //   built for so many features, in so many workgroups,
    bool cls_by_args;                  //   whose rows fit the kernel arguments
    int64_t batches;                   // batches of 64 scored edges of the column-phase encoding (0: the plan holds none)
    // the environment, read by the caller
    bool fast_disabled;                // GN_DISABLE_FAST
    int threads;                       // GN_DM_THREADS: threads of a workgroup of the LDS kernels
};

struct DecoderRoute {
    DecoderKernel kernel;
    gn_status status;                  // GN_OK, or the refusal's (the caller writes the message)
    DecoderRefusal why;
    unsigned grid, block;
    size_t lds_bytes;                  // dynamic LDS
    // every LDS kernel: the column phases (cls, cls_wide: the parts of the sum) and the table's row stride in float4
    int n_phases, c0[kMaxPhases], width[kMaxPhases], stride4;
    // lds_raw, lds_packed
    int64_t edges_per_wg;
    int stage_bytes; int64_t tile_edges; int stage_off;   // lds_raw: bytes of a staged triple (0: none), edges of a tile, where they start
    // cls, cls_wide
    int J, J1;                         // 16-column chunks of a row, and of the first part of the sum
    bool dma;                          // the LDS image is a byte copy of whole rows: filled by LDS-DMA
    // phase
    int64_t batches_per_wg;
    int keep_n;                        // batches per wave whose partial sums stay in LDS between the phases
    bool all_kept;                     // no wave has more batches than that
    // planned: the launch starts the sums (column 0 is its first), finishes them (its last column is the features' last)
    bool first_launch, last_launch;
};

// 16-byte loads of z and D rows: the one predicate every kernel but the scalar one stands on
inline bool decoder_vector_ok(const DecoderCall& c) {
    return c.f % 4 == 0 && c.ld_z % 4 == 0 && c.ld_d % 4 == 0 && c.z_at == 0 && c.d_at == 0;
}

inline DecoderRoute decoder_refusal(DecoderRefusal why) {
    DecoderRoute r{};
    r.kernel = DecoderKernel::refused; r.status = GN_ERR_UNSUPPORTED; r.why = why;
    return r;
}

// ---- the geometry of each kernel ---------------------------------------------------------------------------------------------
inline int decoder_max_width(const DecoderRoute& r) {
    int max_w = 0;
    for (int k = 0; k < r.n_phases; ++k) max_w = std::max(max_w, r.width[k]);
    return max_w;
}

// The staging decision of lds_raw: the triples of the raw int64 list staged in LDS behind the table (see DmFastArgs): where a
// tile of a useful size fits, and the table fills of the extra tiles (every workgroup reads the whole phase table again: ~3 us
// each at this size) cost less than the passes over the list they save (24 bytes per edge and phase at ~5 TB/s)
inline void decoder_staging(const DecoderCall& c, DecoderRoute& r) {
    const size_t table_bytes = r.lds_bytes;
    const int sb = (c.n <= 1023 && c.r <= 4096) ? 4 : 8;
    const int64_t room = kLdsCu - (int64_t)table_bytes;
    const int64_t tile = room / sb / 64 * 64;
    if (tile < kStageMinTile) return;
    const int64_t tiles = decoder_cdiv(r.edges_per_wg, tile);
    const double fill_us = (double)table_bytes * (double)r.grid / kStageFillBytesPerUs;
    const double pass_us = (double)c.e * kStageTripleBytes / kStageStreamBytesPerUs;
    if ((double)(tiles - 1) * r.n_phases * fill_us < (double)(r.n_phases - 1) * pass_us) {
        r.stage_bytes = sb;
        r.tile_edges = std::min<int64_t>(tile, r.edges_per_wg);
        r.lds_bytes += (size_t)r.tile_edges * sb;
    }
}

inline void decoder_lds_geometry(const DecoderCall& c, DecoderRoute& r) {
    r.stride4 = lds_stride4(c.n, decoder_max_width(r));
    r.lds_bytes = (size_t)c.n * r.stride4 * 16;
    // one workgroup per CU; every workgroup's range is a multiple of 64 edges
    int64_t groups = std::min<int64_t>(kDecoderGroups, decoder_cdiv(c.e, 64 * (c.threads / 64)));
    if (groups < 1) groups = 1;
    r.edges_per_wg = decoder_cdiv(decoder_cdiv(c.e, groups), 64) * 64;
    r.grid = (unsigned)decoder_cdiv(c.e, r.edges_per_wg);
    r.block = (unsigned)c.threads;
    r.stage_bytes = 0; r.tile_edges = 0; r.stage_off = (int)r.lds_bytes;
    if (r.kernel == DecoderKernel::lds_raw && r.n_phases > 1) decoder_staging(c, r);   // (packed: six bytes per edge and phase as they are)
}

// (a plan with edges and without the row-class encoding has batches: the split below divides by them)
inline void decoder_phase_geometry(const DecoderCall& c, DecoderRoute& r) {
    const int waves = c.threads / 64;
    r.stride4 = lds_stride4(c.n, decoder_max_width(r));
    const size_t table_bytes = (size_t)c.n * r.stride4 * 16;
    int64_t groups = std::min<int64_t>(kDecoderGroups, decoder_cdiv(c.batches, waves));
    if (groups < 1) groups = 1;
    r.batches_per_wg = decoder_cdiv(c.batches, groups);
    groups = decoder_cdiv(c.batches, r.batches_per_wg);
    // partial sums between phases: as many batches per wave as the LDS left over by the table holds (4 KB each per workgroup)
    const int64_t per_wave = decoder_cdiv(c.batches, groups * waves);
    const int64_t room = (kLdsCu - 1024 - (int64_t)table_bytes) / (waves * 256);
    r.keep_n = r.n_phases > 1 ? (int)std::max<int64_t>(0, std::min(per_wave, room)) : 0;
    // (a launch that takes sums from, or leaves them to, another launch needs the edge positions in those phases too)
    r.all_kept = r.n_phases > 1 && r.keep_n >= per_wave && r.first_launch && r.last_launch;
    r.grid = (unsigned)groups; r.block = (unsigned)c.threads;
    r.lds_bytes = table_bytes + (size_t)r.keep_n * waves * 256;
}

// The row-class kernel's instantiations: the sum keeps the column parts of the phase kernels (plan_phases), so the bits do not
// depend on the kernel.  (Parts are multiples of 16 columns but the last, and f % 16 == 0 here: so is every part.)
inline bool decoder_class_covers(const DecoderCall& c, const DecoderRoute& r) {
    if (!c.cls_ok || c.fast_disabled || r.n_phases < 1 || r.n_phases > 2 || c.f % 16 != 0 || c.f > c.cls_features) return false;
    const int J = (int)(c.f / 16), J1 = r.width[0] / 16;
    return (J == 5 && (J1 == 3 || J1 == 4)) || (J <= 4 && J1 == J);               // other widths: the column-phase kernel
}

// ---- the route --------------------------------------------------------------------------------------------------------------
inline DecoderRoute decoder_route(const DecoderCall& c) {
    DecoderRoute r{};
    r.status = GN_OK; r.why = DecoderRefusal::none;
    r.first_launch = c.col_lo == 0; r.last_launch = c.col_hi == c.num_features;
    const bool vec = decoder_vector_ok(c);
    r.n_phases = vec ? plan_phases(c.n, c.f, r.c0, r.width) : 0;
    for (int k = 0; k < r.n_phases; ++k) r.c0[k] += (int)c.col_lo;
    const bool lds = !c.fast_disabled && r.n_phases >= 1 && r.n_phases <= kLdsMaxPhases;
    if (c.kind == DecoderKind::planned) {
        if (decoder_class_covers(c, r)) {
            r.kernel = c.cls_by_args ? DecoderKernel::cls : DecoderKernel::cls_wide;   // (the class table of the arguments covers 256 workgroups)
            r.J = (int)(c.f / 16); r.J1 = r.width[0] / 16;
            // (odd J: no padding between the LDS rows; z and d are 16-byte aligned and ld_d a multiple of four floats here)
            r.dma = (r.J & 1) && c.ld_z == c.f && c.col_lo == 0;
            r.grid = (unsigned)c.cls_groups; r.block = (unsigned)c.threads; r.lds_bytes = (size_t)kLdsCu;
            return r;
        }
        if (c.cls_ok && c.batches == 0) return decoder_refusal(DecoderRefusal::class_only);
        if (!lds) return decoder_refusal(DecoderRefusal::planned_shape);
        r.kernel = DecoderKernel::phase;
        decoder_phase_geometry(c, r);
        return r;
    }
    // (n <= 65535 cannot bind for raw - 16 columns of n rows fit the budget up to n = 2400 - and stays: the staged triples hold
    // node ids of 16 bits)
    if (lds && c.n <= 65535 && (c.kind == DecoderKind::raw || c.r <= 65535)) {
        r.kernel = c.kind == DecoderKind::raw ? DecoderKernel::lds_raw : DecoderKernel::lds_packed;
        decoder_lds_geometry(c, r);
        return r;
    }
    if (c.kind == DecoderKind::packed) return decoder_refusal(DecoderRefusal::packed_shape);
    DecoderRoute g{};
    g.status = GN_OK; g.why = DecoderRefusal::none;
    g.kernel = vec ? DecoderKernel::general_vec : DecoderKernel::general_scalar;
    g.grid = (unsigned)std::max<int64_t>(1, std::min(decoder_cdiv(decoder_cdiv(c.e, 64) * 64, 256), kGeneralMaxBlocks));
    g.block = 256;
    return g;
}

}  // namespace route
}  // namespace gn
