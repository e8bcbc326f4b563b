// Destination-major gather-reduce shared by the GCN-style layers and the general RGCN path.
//
//   out[i, :] = act( (sum_{p in row i} coef[p] * T[col[p], :]) / max(1, rowdiv[i]) + addend[i, :] + bias )
//
// The kernels and their launchers live in aggregate.hip, compiled once; this header is what their callers need: the
// argument block, the thresholds of the selection rules, the host predicates and the launchers' declarations.
#pragma once

#include "common.h"

// Groups of S neighbour rows a wave requests before it consumes the first one.
#ifndef GN_AGG_U
#define GN_AGG_U 2
#endif
#ifndef GN_AGG_U_WIDE
#define GN_AGG_U_WIDE 8
#endif
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
    const float* table;    // the gathered table in fp32 (launch_aggregate_bf16 reads table_bf16 instead)
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

// lanes a feature row of `units` 16-byte (or scalar) loads takes: the next power of two, one wave at the most
inline int lanes_per_row(int64_t units) {
    int lpe = 1;
    while (lpe < units && lpe < kWave) lpe <<= 1;
    return lpe;
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

// FIN in {16, 32, 64}, FOUT in {16, 32} with at least 4 input features per lane slice
inline bool transform_fusable(int64_t fin, int64_t fout) {
    if (fast_paths_disabled()) return false;
    // exactly the specialisations launch_aggregate_transform has (16 -> 32 has none: its K slice per lane would be two floats)
    return (fout == 16 && (fin == 16 || fin == 32 || fin == 64)) || (fout == 32 && (fin == 32 || fin == 64));
}

// in -> out widths the matrix-core form takes (gn_graph_aggregate_f32 with weight != NULL); rows of up to
// GN_AGG_GROUP_MAX_DEG neighbours on average (longer rows belong to a wave each: the product first, then k_aggregate)
inline bool mfma_fusable(int64_t fin, int64_t fout, int64_t rows, int64_t nnz) {
    if (fast_paths_disabled()) return false;
    if (!(fin == 64 || fin == 128) || fout % 16 != 0 || fout < fin || fout > 128) return false;
    return nnz >= 0 && nnz < GN_AGG_GROUP_MAX_DEG * rows && rows >= 4096;
}

// GN_DISABLE_QUAD=1: the shuffle-based kernel for 16- and 32-wide rows as well (parity tests cover both)
inline bool quad_gather_disabled() {
    const char* e = getenv("GN_DISABLE_QUAD");
    return e && e[0] == '1';
}

// (the quad kernel does not write split planes: its caller follows it with the stand-alone split)
inline bool transform_takes_quad_kernel(int64_t fin, int64_t fout) { return fin == 16 && fout == 16 && !quad_gather_disabled(); }

inline bool lds_table_disabled() {
    const char* e = getenv("GN_DISABLE_LDS_TABLE");
    return e && e[0] == '1';
}

// ---- launchers (aggregate.hip) ----
// the fp32 gather-reduce: picks the LDS-table, short-row, lane-group or wave-per-row kernel from the shapes
gn_status launch_aggregate(const AggArgs& a, hipStream_t st);
// the same over a.table_bf16 with lpe = lanes_per_row(features / 8); the caller says which of the two mappings (lane groups
// own rows, or a wave per row)
gn_status launch_aggregate_bf16(const AggArgs& a, int lpe, bool by_group, hipStream_t st);
// out = act( (A table) w + bias ): shuffle or quad epilogue (transform_fusable), or the matrix cores (mfma_fusable)
gn_status launch_aggregate_transform(const AggArgs& a, const float* w, int fout, hipStream_t st);
// the 64 -> 16 shuffle form with the deferred tail transform of the table's columns 48..63
gn_status launch_aggregate_transform_tail(const AggArgs& a, const float* w, int fout, const AggTail& tail, hipStream_t st);
// the 64 -> 16 shuffle form over a row kept in two tables; split_source_refusal: why it does not take these operands (null:
// it does), asked without launching
const char* split_source_refusal(const float* head, int64_t ld_head, int64_t head_cols, const float* tail, int64_t ld_tail,
                                 int64_t features, int64_t fout);
gn_status launch_aggregate_transform_split(const AggArgs& a, const float* w, int fout, const AggSplit& split, hipStream_t st);
gn_status launch_aggregate_mfma(const AggArgs& a, const float* w, int fout, hipStream_t st);
// the three bf16 terms of src[rows, cols] into columns col0 .. of the planes
gn_status launch_split_planes(const float* src, int64_t ld_src, int64_t rows, int cols, int col0, const gn_split_planes& sp, hipStream_t st);

}  // namespace gn
