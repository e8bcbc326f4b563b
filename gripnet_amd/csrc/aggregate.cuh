// Destination-major gather-reduce shared by the GCN-style layers and the general RGCN path.
//
//   out[i, :] = act( (sum_{p in row i} coef[p] * T[col[p], :]) / max(1, rowdiv[i]) + addend[i, :] + bias )
//
// The kernels and their launch functions live in aggregate.hip, compiled once; which of them serves a call is gather_route.hpp's
// to say.  This header is what their callers need: the argument block, the call's facts as the route asks them, and
// launch_gather's declaration.
#pragma once

#include "common.h"

#include "gather_route.hpp"

// Groups of S neighbour rows a wave requests before it consumes the first one.
#ifndef GN_AGG_U
#define GN_AGG_U 2
#endif
// (the 16-lanes-per-neighbour transform kernels: all sixteen groups of four, a whole padded row of 64 in one request round)
#ifndef GN_AGG_U_WIDE
#define GN_AGG_U_WIDE 16
#endif
// Row gathers in flight per lane of k_aggregate_group
#ifndef GN_AGG_GROUP_U
#define GN_AGG_GROUP_U 8
#endif
// Row gathers in flight per lane of the matrix-core kernel at 64 input features (see k_aggregate_mfma)
#ifndef GN_MFMA_U16
#define GN_MFMA_U16 4
#endif

namespace gn {

struct AggArgs {
    const int32_t* rowptr;
    const uint32_t* col;
    const float* coef;     // nullable (all ones)
    const float* table;    // the gathered table in fp32 (the bf16 kernels read table_bf16 instead)
    int64_t ld_table;
    int features;
    const float* rowdiv;   // nullable
    const float* addend;   // nullable
    int64_t ld_addend;
    const float* bias;     // nullable
    int relu;
    float* out;
    int64_t ld_out;
    int rows;
    gn_side_copy side = {nullptr, 0, nullptr, 0, 0, 0, 0};   // optional fused row copy (dst == nullptr: none)
    gn_split_planes split = {nullptr, 0, 0, 0, 0};           // optional bf16 split planes of what the launch writes
    const uint32_t* ell_col = nullptr;   // padded rows of the plan (rows of at most 64 entries), or null
    const float* ell_coef = nullptr;
    int64_t nnz = -1;      // stored coefficients, when the caller knows them (picks the short-row kernel)
    int64_t table_rows = -1;   // rows of the gathered table, when the caller knows them (picks the LDS-table kernel)
    const uint16_t* table_bf16 = nullptr;   // the gathered table in bf16 storage (ld_table counts bf16 elements)
};

// A 16 -> 16 transform left to the reader of its input (k_aggregate_transform_tail): relu(G w + b) of the last 16 columns
// of every gathered row
struct AggTail {
    const float* w;        // [16, 16] row-major, 16-byte aligned
    const float* b;        // [16], 16-byte aligned, nullable
    int relu;
};

// A gathered row kept in two tables (k_aggregate_transform_split): its first head_cols columns are row `col` of AggArgs::table
// (leading dimension ld_table), the rest row `col` of `tail` - a concat that is read where its parts lie, not built
struct AggSplit {
    const float* tail;     // [table rows, features - head_cols], 16-byte aligned
    uint32_t ld_tail;      // % 4 == 0
    int head_cols;         // 16, 32 or 48 of the 64
};

// The fused row copy of a launch (a concat slot), streamed by the whole grid; where in the kernel is the caller's choice
// (the gather family streams it before its own rows, k_col_gather behind them: nothing depends on the order).  The kernel
// hands in its global thread index and the grid's thread count: blockDim read inside a __device__ function compiles to
// the form that allows for a partial last workgroup, a kernel's own read does not.  The descriptor comes by value: through a
// reference to the kernel's argument block the compiler schedules the whole of k_col_gather differently.
__device__ __forceinline__ void side_copy_stream(gn_side_copy s, int64_t thread, int64_t n_threads) {
    if (s.dst) {
        const int64_t total = s.rows * s.cols;
        for (int64_t t = thread; t < total; t += n_threads) {
            const int64_t i = t / s.cols, c = t - i * s.cols;
            const float v = s.src[i * s.ld_src + c];
            s.dst[i * s.ld_dst + c] = s.mode ? fabsf(v) : v;
        }
    }
}

inline gn_status check_side(const gn_side_copy* side, int64_t rows, gn_side_copy* out) {
    *out = gn_side_copy{nullptr, 0, nullptr, 0, 0, 0, 0};
    if (!side || side->rows == 0 || side->cols == 0) return GN_OK;
    GN_REQUIRE(side->src && side->dst && side->rows > 0 && side->cols > 0, "side copy has a null pointer or a negative size");
    GN_REQUIRE(side->rows <= rows, "side copy has %lld rows, the launch only %lld", (long long)side->rows, (long long)rows);
    GN_REQUIRE(side->ld_src >= side->cols && side->ld_dst >= side->cols, "side copy leading dimension smaller than its row");
    GN_REQUIRE(side->mode == 0 || side->mode == 1, "unknown side copy mode %d", side->mode);
    *out = *side;
    return GN_OK;
}

// The gather's arguments of a forward call on `plan`
inline AggArgs forward_args(const gn_graph_plan* plan, const float* xw, int64_t ld_xw, int64_t num_features, const float* bias,
                            int relu, float* out, int64_t ld_out) {
    AggArgs a;
    a.rowptr = plan->rowptr.p;
    a.col = reinterpret_cast<const uint32_t*>(plan->col.p);
    a.coef = plan->plain_ones ? nullptr : plan->coef.p;       // (null = all ones)
    a.table = xw;
    a.ld_table = ld_xw;
    a.features = (int)num_features;
    a.rowdiv = nullptr;
    a.addend = nullptr;
    a.ld_addend = 0;
    a.bias = bias;
    a.relu = relu;
    a.out = out;
    a.ld_out = ld_out;
    a.rows = (int)plan->rows;
    a.nnz = plan->nnz;
    a.table_rows = plan->table_rows;
    if (plan->ell_ok) { a.ell_col = plan->ell_col.p; a.ell_coef = plan->ell_coef.p; }
    return a;
}

// ---- what gather_route.hpp is asked: the facts of a call, with the environment's switches read here ----
// A getenv or a device query costs a recorded step more than the route's arithmetic (0.3-0.4 us per gather call, measured on the
// flagship step), so a switch is read only where the call can reach the rule that asks it, and stays false elsewhere.
inline bool switched_on(const char* value) { return value && value[0] == '1'; }
inline bool blocked_switched_off() { return switched_on(getenv("GN_DISABLE_BLOCKED")); }     // (gcn_blocked.hip asks as well)

inline unsigned past16(const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15); }

// a bare gather-reduce: no plan behind it, no weight (rgcn.hip's sum, gn_graph_aggregate_t_f32, and what forward_call starts from)
inline route::GatherCall gather_call(const AggArgs& a) {
    route::GatherCall c{};
    c.kind = a.table_bf16 ? route::Source::bf16 : route::Source::f32;
    c.rows = a.rows; c.nnz = a.nnz; c.table_rows = a.table_rows;
    c.features = a.features; c.fout = a.features;
    c.ld_table = a.ld_table; c.ld_out = a.ld_out;
    c.table_at = past16(a.table_bf16 ? static_cast<const void*>(a.table_bf16) : a.table);
    c.out_at = past16(a.out); c.bias_at = past16(a.bias);
    c.coef = a.coef != nullptr; c.rowdiv = a.rowdiv != nullptr; c.addend = a.addend != nullptr; c.bias = a.bias != nullptr;
    c.relu = a.relu != 0; c.side = a.side.dst != nullptr;
    c.fast_disabled = fast_paths_disabled();
    c.lds_table_disabled = a.rows >= route::kLdsTableRows && switched_on(getenv("GN_DISABLE_LDS_TABLE"));   // (asked from there on)
    return c;
}

// a forward call on `plan` that writes rows of `width` floats (weight == null: the gathered row's own)
inline route::GatherCall forward_call(const gn_graph_plan* plan, const AggArgs& a, const float* weight, int64_t width) {
    route::GatherCall c = gather_call(a);
    c.weight = weight != nullptr; c.weight_at = past16(weight); c.fout = width;
    if (plan->blk_ok) {
        c.blk_ok = true; c.blk_cw = plan->blk_cw; c.blk_cols = plan->blk_cols;
        c.blocked_disabled = blocked_switched_off();
        if (route::blocked_applicable(c)) return c;          // (the first rule of the ladder, and it reads nothing of what follows)
    }
    if (weight) {
        // GN_DISABLE_QUAD=1: the shuffle-based kernel for 16-wide rows as well (parity tests cover both)
        c.quad_disabled = switched_on(getenv("GN_DISABLE_QUAD"));
        if (route::mfma_fusable(c.features, c.fout, c.rows, c.nnz, c.fast_disabled)) c.compute_units = compute_units();
    }
    return c;
}

// ---- launchers (aggregate.hip) ----
// The kernel `r` names over `a`: one launch function per kernel behind it.  `w` [features, fout]: the weight of the mfma and
// transform kernels; `tail` / `split`: the extra operand of transform_tail / transform_split.  (blocked is not launched from
// here: gcn_blocked.hip)
gn_status launch_gather(const route::GatherRoute& r, const AggArgs& a, hipStream_t st, const float* w = nullptr, int fout = 0,
                        const AggTail* tail = nullptr, const AggSplit* split = nullptr);
// the route of a bare gather-reduce, launched
inline gn_status launch_aggregate(const AggArgs& a, hipStream_t st) {
    if (a.rows == 0 || a.features == 0) return GN_OK;
    return launch_gather(route::gather_route(gather_call(a)), a, st);
}
// the three bf16 terms of src[rows, cols] into columns col0 .. of the planes
gn_status launch_split_planes(const float* src, int64_t ld_src, int64_t rows, int cols, int col0, const gn_split_planes& sp, hipStream_t st);

}  // namespace gn
