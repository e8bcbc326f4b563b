/*
 * gripnet_hip.h - C ABI of the MI355X (gfx950) supergraph propagation engine.
 *
 * The reference (NYXFLOWER/GripNet) has no FFI layer: its hot path is Python that calls into
 * ATen / torch_geometric / torch_scatter.  This header is the boundary a maintainer binds
 * instead of those calls; every entry point names the reference lines it replaces
 * (paths relative to the reference tree).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in _host;
 *   - feature matrices are row-major fp32 with an explicit leading dimension (elements);
 *   - node / edge indices are int64, exactly as the reference's torch.long tensors;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous with respect to
 *     the host except the *_plan_create functions, which synchronise `stream` once;
 *   - outputs and scratch are caller-allocated; the library owns only what hangs off an
 *     opaque plan handle (the cached CSR / normalisation / counts of one static graph);
 *   - every function returns a gn_status; gn_last_error() gives the calling thread's message;
 *   - re-entrant and thread-safe on distinct plans; no global mutable state.
 */
#ifndef GRIPNET_HIP_H
#define GRIPNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GN_VERSION 173 /* 0.1.67 */

#if defined(GN_BUILDING)
#define GN_API __attribute__((visibility("default")))
#else
#define GN_API
#endif

typedef enum gn_status {
    GN_OK = 0,
    GN_ERR_INVALID_ARG = 1,   /* null pointer, negative size, unsupported shape          */
    GN_ERR_HIP = 2,           /* a HIP runtime call failed (message carries hipGetErrorString) */
    GN_ERR_INDEX_RANGE = 3,   /* an edge endpoint / relation id is outside its table     */
    GN_ERR_UNSUPPORTED = 4,   /* sizes beyond what the 32-bit plan encoding can hold     */
    GN_ERR_EDGE_COUNT = 5     /* plan was built for a different number of edges          */
} gn_status;

/* Optional row-wise side copy fused into an aggregation launch: the concat slots the reference fills
 * with torch.cat (gripnet/layers.py:264-266,309,376).  dst[i, 0:cols] = src[i, 0:cols] (mode 0) or
 * |src[i, 0:cols]| (mode 1) for i in [0, rows); rows must not exceed the rows of the launch. */
typedef struct gn_side_copy {
    const float* src; int64_t ld_src;
    float* dst; int64_t ld_dst;
    int64_t rows, cols;
    int mode;
} gn_side_copy;

/* Optional third output of an aggregation launch, and optional input of gn_rgcn_forward_f32: a row-major matrix
 * X [rows, 16 nt] as the three bf16 terms the relational layer's matrix products run on (x = hi + mid + lo exactly,
 * each cut by truncation).  The relational kernel otherwise splits the same 645 x 48 values again in every one of its
 * 13,500 units (gripnet/layers.py:172-186 is the product this feeds); the layer that PRODUCES x - the external layer
 * writing y, its side copy writing |target_feat| (layers.py:370,376) - can leave the terms behind for free.
 * Layout: planes[(row * 16 + cell) * cb + (term * nt + j) * 2], two bytes each: cell = column / nt, j = column % nt,
 * cb = 4 * ceil(3 nt / 2) bytes per cell, term 0 / 1 / 2 = hi / mid / lo.  The buffer holds rows + 1 rows and the
 * caller keeps row `rows` ZERO (a source that is none names it): (rows + 1) * 16 * cb bytes (gn_split_planes_bytes). */
typedef struct gn_split_planes {
    void* planes;
    int64_t rows;
    int nt;           /* columns of X / 16 */
    int col_main;     /* column of X where the launch's main output starts */
    int col_side;     /* column of X where the launch's side copy starts (ignored without one) */
} gn_split_planes;

typedef struct gn_graph_plan gn_graph_plan; /* GCN-style graphs (square or bipartite)  */
typedef struct gn_rgcn_plan gn_rgcn_plan;   /* multi-relational graph of one supervertex */

GN_API int gn_version(void);
/* Message of the last failing call made by this thread ("" if none). */
GN_API const char* gn_last_error(void);
/* Device allocations the library holds right now: the buffers of every live plan, sampler and known-pair set plus the
 * scratch blocks of a builder that is running.  Back to its earlier value once a handle is destroyed or a create fails. */
GN_API int64_t gn_device_blocks_live(void);

/* ---------------------------------------------------------------------------------------
 * GCN-style normalised graph.  Replaces myGCN.norm + its cache (gripnet/layers.py:52-69,
 * 83-90): drops existing self loops, appends one loop per node (weight = that node's last
 * listed loop weight, else 1, or 2 if `improved`), deg = sum of weights by DESTINATION,
 * norm = deg[src]^-1/2 * w * deg[dst]^-1/2 (inf -> 0).  The plan holds edge_index'
 * (non-loops in input order, then loops 0..N-1) and norm in the reference's order, plus a
 * destination-major CSR (int32 columns, fp32 coefficients) used by gn_graph_aggregate_f32.
 * w may be NULL (all ones).
 */
GN_API gn_status gn_gcn_plan_create(const int64_t* src, const int64_t* dst, const float* w, int64_t num_edges,
                             int64_t num_nodes, int improved, void* stream, gn_graph_plan** plan);

/* External (inter-supervertex) layer graph.  Replaces the index shift, zero padding and the
 * dead self loops of interGraph.forward (gripnet/layers.py:363-368) by their closed form:
 * coefficient of edge s->t is w_e * (1 + sum of weights into t)^-1/2; rows are targets. */
GN_API gn_status gn_bipartite_plan_create(const int64_t* src, const int64_t* dst, const float* w, int64_t num_edges,
                                   int64_t num_sources, int64_t num_targets, void* stream, gn_graph_plan** plan);

/* Plain (un-normalised) weighted-sum graph: out[t] = sum_{e: dst(e)=t} w_e * table[src(e)], w NULL = ones.
 * Used by the backward pass of the relational layer (rows = (relation, source) pairs, autograd of
 * gripnet/layers.py:178-189). */
GN_API gn_status gn_sum_plan_create(const int64_t* src, const int64_t* dst, const float* w, int64_t num_edges,
                             int64_t num_sources, int64_t num_targets, void* stream, gn_graph_plan** plan);

GN_API void gn_graph_plan_destroy(gn_graph_plan* plan);
/* Number of edges the plan was built from (the reference's cache key, layers.py:76-84). */
GN_API int64_t gn_graph_plan_input_edges(const gn_graph_plan* plan);
/* Number of stored coefficients: E' = non-loop edges + N for a GCN plan, E for a bipartite plan. */
GN_API int64_t gn_graph_plan_nnz(const gn_graph_plan* plan);
/* Copy edge_index' ([2, E'] int64) and norm ([E'] fp32) in the reference's order (GCN plans). */
GN_API gn_status gn_graph_plan_export(const gn_graph_plan* plan, int64_t* edge_index_out, float* norm_out, void* stream);

/* out[i, :] = act( sum_{e: dst(e)=i} coef_e * xw[src(e), :] + bias ),  i in [0, rows).
 * Replaces propagate/message/update of myGCN (gripnet/layers.py:92-100) and the ReLU that
 * always follows (layers.py:279,305,370).  xw = x @ W is computed first with gn_gemm_f32,
 * as the reference does (layers.py:73).  bias may be NULL.  `out` may be a column slice of a
 * wider matrix (ld_out), which is how the concat of layers.py:309,376 is written in place. */
GN_API gn_status gn_graph_aggregate_f32(const gn_graph_plan* plan, const float* xw, int64_t ld_xw, int64_t num_features,
                                 const float* weight /* nullable */, int64_t out_features,
                                 const float* bias, int relu, float* out, int64_t ld_out,
                                 const gn_side_copy* side /* nullable */, const gn_split_planes* planes /* nullable */,
                                 void* stream);
/* `planes`: the launch also leaves the bf16 split planes of what it writes (main output and side copy, as columns
 * col_main.. / col_side.. of X).  The wave-per-row transform kernel writes them from its epilogue; the other kernels
 * are followed by gn_split_planes_f32 launches.  The same planes from a matrix that already exists: */
GN_API size_t gn_split_planes_bytes(int64_t rows, int nt);
GN_API gn_status gn_split_planes_f32(const float* src, int64_t ld_src, int64_t rows, int64_t cols, int64_t col0,
                              const gn_split_planes* planes, void* stream);
/* With weight != NULL ([num_features, out_features], row-major, contiguous) the table is the layer INPUT x
 * and the call computes act( (A_norm x) W + bias ) = act( A_norm (x W) + bias ): the contraction of
 * layers.py:73 runs on the aggregated row, so no x W launch is needed.  Supported for (num_features,
 * out_features) in {16,32,64} x {16} and {32,64} x {32}, and for the wide layers gn_graph_transform_fusable describes
 * (GN_ERR_UNSUPPORTED otherwise: call gn_gemm_f32 first).  gn_transform_fusable / gn_graph_transform_fusable tell
 * without launching. */
GN_API int gn_transform_fusable(int64_t in_features, int64_t out_features);
/* The same question for one plan: besides the widths above, layers at least as wide as their input (64 or 128 input
 * features, out_features a multiple of 16 in [in_features, 128]) contract on the matrix cores in the same launch when
 * the plan's rows average fewer than 48 neighbours and there are at least 4,096 of them (the second layer of the
 * node-classification stacks: no x W launch, no [N, out] round trip). */
GN_API int gn_graph_transform_fusable(const gn_graph_plan* plan, int64_t in_features, int64_t out_features);

/* gn_graph_aggregate_f32 with `weight` on the wave-per-row transform kernel over a gathered row that is kept in TWO tables:
 * row `col` of the table is row `col` of `head` ([table rows, head_cols], leading dimension ld_head) followed by row `col`
 * of `tail` ([table rows, num_features - head_cols], leading dimension ld_tail) - the concat of layers.py:309 read where
 * its parts lie instead of built (the external layer of PoSE reads the gene embedding parameter itself: no copy of it
 * into a concat slot).  Per lane the same 16-byte loads, the same sums in the same order, the same contraction: the
 * bits of gn_graph_aggregate_f32 over the materialised [head | tail].  Plan, bias, relu, `side` and `planes` as there.
 * Supported: num_features 64 -> out_features 16, head_cols 16, 32 or 48, both tables 16-byte aligned with leading
 * dimensions that are multiples of 4 and below 2^31, not under GN_DISABLE_FAST; GN_ERR_UNSUPPORTED otherwise, with
 * nothing launched.  gn_graph_split_applicable tells without launching.  Nothing is kept between calls.
 * Measured on pose0-syn (round 19, profiles/r19_split_source.md): without the copy the first gene layer's gather launch
 * takes 8.7-9.0 us instead of 10.8, the external launch 7.5-7.7 us over either source (7.5 over the concat), the step
 * 1.6-2.5 us less of ~75; z and score bit for bit the parent's. */
GN_API int gn_graph_split_applicable(const gn_graph_plan* plan, const float* head, int64_t ld_head, int64_t head_cols,
                                     const float* tail, int64_t ld_tail, int64_t num_features, int64_t out_features);
GN_API gn_status gn_graph_aggregate_split_f32(const gn_graph_plan* plan, const float* head, int64_t ld_head, int64_t head_cols,
                                       const float* tail, int64_t ld_tail, int64_t num_features, const float* weight,
                                       int64_t out_features, const float* bias, int relu, float* out, int64_t ld_out,
                                       const gn_side_copy* side /* nullable */, const gn_split_planes* planes /* nullable */,
                                       void* stream);

/* Column-group encoding of a GCN plan for LDS-staged gathers (the gene supervertex of PoSE: 19,081 nodes, 1.45 M
 * stored edges; gcn_blocked.hip).  Applies to plans whose stored weights are all exactly 1, self loops included
 * (edge_weight NULL or ones and not `improved`: every GripNet caller, GripNet-pose.py:52,117-120): norm_e =
 * dis[src] dis[dst] then factorises and an edge is a 16-bit source id.  The table T = dis * (x W) is cut by COLUMNS:
 * a workgroup holds two fp32 columns (one above ~19,900 nodes, up to ~39,800) of EVERY node in 160 KB of LDS, so it
 * owns its destination rows outright - no partial sums, no combine pass.  gn_graph_aggregate_f32 takes this path (two
 * launches: the exact-fp32 transform writing T column-group-major into scratch the PLAN owns, then the gather from
 * LDS; fixed summation order) when the plan has the encoding and the shapes are covered: out_features 16 or 32 <= cols,
 * with `weight` num_features in {16,32,64}, x 16-byte aligned with ld % 4 == 0, out and bias aligned to the gather's column
 * groups (gn_graph_blocked_applicable).  Calls on one plan must be
 * stream-ordered (the scratch table).  Graphs that do not qualify (weighted, `improved`, fewer than 4,096 nodes or
 * fewer than 16 stored edges per node, too many nodes for one column in LDS) keep the wave-per-row kernels and the call
 * returns GN_OK; gn_graph_plan_blocked_cols tells (0 = not built).  Copies the CSR to the host once, schedules it there
 * and synchronises `stream`: meant for graphs that are kept (the Python layer builds it only for `cached=True`). */
GN_API gn_status gn_graph_plan_build_blocked(gn_graph_plan* plan, int64_t cols, void* stream);
GN_API int64_t gn_graph_plan_blocked_cols(const gn_graph_plan* plan);
/* Which gather kernel the LDS-staged path launches for this plan right now: 0 = the plan has no such encoding, 1 = the
 * staged kernel (a range's tile sums parked in LDS behind the table, all rows written behind the loop), 2 = the
 * direct-store kernel (no room for the slots behind the table, or GN_BLOCKED_DIRECT=1).  Same bits either way. */
GN_API int gn_graph_plan_blocked_gather_kernel(const gn_graph_plan* plan);
/* The schedule the gather walks, copied to `host_out` (null: only counted): per range and per wave of its workgroup (16)
 * twelve ints - first tile, end tile, first iteration, end iteration of the id stream, the ends of its first five tiles,
 * three unused.  Returns the number of ints, 0 without the encoding, -1 when `capacity` is too small or the copy failed.
 * Synchronises the device.  For tests and tools that must know which waves a graph produces. */
GN_API int64_t gn_graph_plan_blocked_waves(const gn_graph_plan* plan, int32_t* host_out, int64_t capacity);
/* Whether gn_graph_aggregate_f32 with these operands takes the LDS-staged path (it also needs `out`, `ld_out` and `bias`
 * aligned to the gather's column groups; other operands keep the wave-per-row kernels).  Launches nothing. */
GN_API int gn_graph_blocked_applicable(const gn_graph_plan* plan, const float* x, int64_t ld_x, int64_t num_features,
                                       const float* weight, int64_t out_features, const float* bias, const float* out,
                                       int64_t ld_out);

/* Two GCN-style layers over ONE graph followed by a reader of their rows, with the second layer's 16 -> 16 transform left
 * to that reader (the gene stack of PoSE feeding the external layer: three gene launches instead of four):
 *   h1 = act( A (x W1) + b1 ),   h2 = act( A (h1 W2) + b2 ) = act( (A h1) W2 + b2 ).
 * `plan` and `next` are the two layers' plans: both with the LDS-staged encoding of the same unit-weight graph (equal
 * rows, stored edges, table rows, column groups and schedule sizes; the caller vouches that the edge lists are the same).
 *   gn_graph_aggregate_chain_f32   layer 1 as gn_graph_aggregate_f32 computes it (same launches, same bits in `out`); the
 *                                  gather also stores dis[i] * h1[i, :] into `next`'s scratch table, each workgroup its
 *                                  own (column group, rows) cells.  out_features = 16.
 *   gn_graph_gather_chained_f32    out[i, 0:16] = dis[i] * sum of the rows of the plan's table AS IT STANDS (no transform
 *                                  launch, no bias, no activation): G = A h1 after the call above, with plan = `next`.
 *   gn_graph_aggregate_tail_f32    gn_graph_aggregate_f32 with `weight` for 64 -> 16 features on the wave-per-row kernel,
 *                                  except that columns 48..63 of every gathered row are replaced, in registers, by
 *                                  act(row[48:64] tail_w + tail_b) (tail_relu: the ReLU) BEFORE the row enters the sum.
 * GN_ERR_UNSUPPORTED where the chain cannot hold: a plan without the encoding, a weighted graph, plans that differ, other
 * widths, operands gn_graph_blocked_applicable refuses, GN_DISABLE_BLOCKED / GN_DISABLE_FAST, or without GN_ENABLE_CHAIN=1
 * (the chain is opt-in until it has been measured against the four-launch stack).  gn_graph_chain_applicable tells without launching; out_next is where gn_graph_gather_chained_f32 will write.
 * Nothing is kept between calls: weights and biases are read by the launches that use them.  The calls on the two plans
 * must be stream-ordered.  The sum of layer 2 is re-associated, (sum dis h1) W2 instead of sum dis (h1 W2): the same number
 * of fp32 operations per element, not the same bits. */
GN_API int gn_graph_chain_applicable(const gn_graph_plan* plan, const gn_graph_plan* next, const float* x, int64_t ld_x,
                                     int64_t num_features, const float* weight, int64_t out_features, const float* bias,
                                     const float* out, int64_t ld_out, const float* out_next);
GN_API gn_status gn_graph_aggregate_chain_f32(const gn_graph_plan* plan, const gn_graph_plan* next, const float* x, int64_t ld_x,
                                       int64_t num_features, const float* weight, int64_t out_features, const float* bias,
                                       int relu, float* out, int64_t ld_out, const gn_side_copy* side /* nullable */,
                                       void* stream);
GN_API gn_status gn_graph_gather_chained_f32(const gn_graph_plan* plan, float* out, int64_t ld_out, void* stream);
GN_API gn_status gn_graph_aggregate_tail_f32(const gn_graph_plan* plan, const float* x, int64_t ld_x, int64_t num_features,
                                      const float* weight, int64_t out_features, const float* bias, int relu, float* out,
                                      int64_t ld_out, const gn_side_copy* side /* nullable */,
                                      const gn_split_planes* planes /* nullable */, const float* tail_w,
                                      const float* tail_b /* nullable */, int tail_relu, void* stream);

/* bf16 STORAGE of the gathered table (the reference is fp32 throughout, this is the build's own
 * reduced-traffic variant for the node-classification suite): gn_cast_bf16 rounds x W to bf16 once,
 * gn_graph_aggregate_bf16 computes out[i,:] = act( sum_e coef_e * table[src(e),:] + bias ) from it with fp32 sums and an
 * fp32 result.  num_features % 8 == 0, 16-byte aligned rows.  Error against the fp32 layer: one bf16 rounding (2^-9
 * relative) of every gathered element; exact against the same sum over the rounded table. */
GN_API gn_status gn_cast_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst, int64_t rows, int64_t cols,
                       void* stream);
GN_API gn_status gn_graph_aggregate_bf16(const gn_graph_plan* plan, const uint16_t* table, int64_t ld_table, int64_t num_features,
                                  const float* bias, int relu, float* out, int64_t ld_out,
                                  const gn_side_copy* side /* nullable */, void* stream);

/* Backward pass of the GCN-style layers (autograd of GripNet-pose.py:140-146 through layers.py:92-100).
 * gn_graph_plan_build_transpose adds the source-major CSR of the same coefficients to a plan (once;
 * synchronises `stream`); gn_graph_aggregate_t_f32 then computes, for every source row s,
 *   gxw[s, :] = sum_{e: src(e)=s} coef_e * g[dst(e), :]        (d loss / d (x W) from d loss / d out). */
GN_API gn_status gn_graph_plan_build_transpose(gn_graph_plan* plan, void* stream);
GN_API gn_status gn_graph_aggregate_t_f32(const gn_graph_plan* plan, const float* g, int64_t ld_g, int64_t num_features,
                                   float* out, int64_t ld_out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dense fp32 contraction on the matrix cores:
 *   C[b] = act( gather_rows(A[b]) @ B[b] + bias ),  b in [0, batch).
 * Replaces torch.matmul at gripnet/layers.py:73,172-173,193,383 and decoder.py:42.
 * a_rows (int64, may be NULL) selects rows of A (z[node_list], decoder.py:42).
 * stride_* are batch strides in elements (0 = shared operand).  batch <= 65535 (more: GN_ERR_UNSUPPORTED, the caller cuts it).
 * Arithmetic (part of the contract, never read from the environment): by default fp32-faithful - the fp32 matrix
 * instruction (v_mfma_f32_16x16x4_f32, exact) or, for tall-skinny products, bf16 matrix instructions on operands split
 * into THREE bf16 terms (six products; what is dropped is below 2^-23 of a product).  GN_GEMM_ARITH_FAST keeps two terms
 * and three products (<= 2^-16 relative per product). */
#define GN_GEMM_RELU 1           /* flags of gn_gemm_f32 */
#define GN_GEMM_ARITH_FAST 2
#define GN_GEMM_B_TRANSPOSED 4  /* b is given as [n, k] row-major (leading dimension ldb >= k): c = a b^T - the dx = g W^T of the backward passes */
#define GN_GEMM_ACCUMULATE 8    /* c += a b (+ bias) instead of c = ... */
#define GN_GEMM_A_TRANSPOSED 16  /* a is given as [k, m] row-major (lda >= m): c = a^T b; m <= 64 or n <= 32 only: dbasis = att^T dW */
#define GN_GEMM_JOIN_BATCH 32   /* the product may leave with the open batch (gn_dense_batch_begin / _end, below) */
#define GN_GEMM_SPLIT_KERNEL 128 /* take the tall-skinny split kernel whatever the row count (k % 32 == 0, aligned rows): a caller that cuts one
                                 * product into slabs of rows gets the same bits for every slab size */
#define GN_GEMM_OUT_BF16 64     /* c is a bf16 table [m, n] (ldc in bf16 elements, rows 8-byte aligned, n % 4 == 0): every value is rounded to
                                 * nearest even ONCE, where the product is stored - gn_cast_bf16's rounding without its pass (the table of a
                                 * bf16-storage layer, gn_graph_aggregate_bf16).  Tall-skinny products only (m >= 2048, k % 32 == 0, no
                                 * accumulate / addend / row gather): GN_ERR_UNSUPPORTED otherwise, and the caller casts a fp32 product */
GN_API gn_status gn_gemm_f32(const float* a, int64_t lda, int64_t stride_a, const int64_t* a_rows, int64_t a_table_rows,
                      const float* b, int64_t ldb, int64_t stride_b, float* c, int64_t ldc, int64_t stride_c,
                      int64_t m, int64_t n, int64_t k, int64_t batch, const float* bias, int flags, void* stream);
/* The same product with an ADDEND: c = a b (+ bias) (+ c with GN_GEMM_ACCUMULATE) + addend, addend [m, n] with rows ld_addend
 * floats apart (may be NULL: gn_gemm_f32), batch == 1.  For the backward pass of a layer whose input also sits in a concat
 * (layers.py:280-281,307-309): dx = g W^T + (the concat's gradient columns of that input) leaves one launch instead of the
 * product and an element-wise sum.  The addend is only read; it may be a column slice of a wider matrix. */
GN_API gn_status gn_gemm_addend_f32(const float* a, int64_t lda, int64_t stride_a, const int64_t* a_rows, int64_t a_table_rows,
                      const float* b, int64_t ldb, int64_t stride_b, float* c, int64_t ldc, int64_t stride_c,
                      int64_t m, int64_t n, int64_t k, int64_t batch, const float* bias, const float* addend, int64_t ld_addend,
                      int flags, void* stream);

/* out[k1, k2] = x^T g over m rows (x [m, k1], g [m, k2]; k1 * k2 <= 4096): the weight gradients dW = x^T (A_norm^T g)
 * of the GCN-style layers and d root = x^T g of the relational one (autograd of layers.py:73,193).  Row slices are
 * reduced in a fixed order: bitwise reproducible.  Scratch is caller-provided (gn_xtg_workspace_bytes).
 * flags: GN_XTG_TICKET_ZEROED promises that the 64 bytes at offset gn_xtg_workspace_bytes(k1, k2) - 64 of the workspace
 * were zeroed once by the caller and are touched by nobody else (calls on one workspace stream-ordered): up to 64 x 32 outputs then take ONE launch on the matrix
 * cores (slices added in slice order by the last slice to arrive - beyond 32 slices, the products over tens of thousands of
 * rows, in two levels: sets of sixteen slices, then the sets) instead of a partial-sum launch and a fold. */
#define GN_XTG_TICKET_ZEROED 1
#define GN_XTG_JOIN_BATCH 2      /* the product may leave with the open batch (gn_dense_batch_begin / _end) */
GN_API size_t gn_xtg_workspace_bytes(int64_t k1, int64_t k2);
/* 1 when gn_xtg_f32 takes a product of these sizes as ONE wide product (k1 in {64, 128, 256}, k2 in {32, 64, 128}, 2-16 tiles of
 * 64 x 32, at least 4096 rows: a workgroup per row slice computes every tile, a fold launch adds the slices in slice order; x and g
 * are read once) - the weight gradients of the 128 x 64 ... 256 x 128 layers of the node-classification models.  Such a product may
 * have more than 4096 outputs; it is never queued in a dense batch. */
GN_API int gn_xtg_wide_supported(int64_t m, int64_t k1, int64_t k2);
GN_API gn_status gn_xtg_f32(const float* x, int64_t ld_x, const float* g, int64_t ld_g, int64_t m, int64_t k1, int64_t k2,
                     float* out, int64_t ld_out, void* workspace, size_t workspace_bytes, int flags, void* stream);

/* Element-wise merges of the external layer (gripnet/layers.py:375-384) and slot copies of the
 * concat outputs:  mode 0: dst = src;  1: dst = |src|;  2: dst = (dst + |src|) / 2;
 * 3: dst = (dst + relu(src)) / 2;  4: dst = (dst + src + src2) / 3 (freebase-c merge,
 * GripNet-freebase-c.py:158-162).  Backward helpers:  5: dst = src2 > 0 ? src : 0 (ReLU mask by the
 * saved output);  6: dst = src * sign(src2) (gradient of |.|);  7: dst = src / 3 (every operand's share of mode 4);
 * 8: dst = src / 2 (the first operand's share of modes 2 and 3);  9: dst = src * sign(src2) / 2 (the |.| operand of
 * mode 2);  10: dst = src2 > 0 ? src / 2 : 0 (the ReLU operand of mode 3). */
GN_API gn_status gn_merge_f32(float* dst, int64_t ld_dst, const float* src, int64_t ld_src, const float* src2,
                       int64_t ld_src2, int64_t rows, int64_t cols, int mode, void* stream);

/* Row softmax in place (decoder.py:43). */
GN_API gn_status gn_softmax_rows_f32(float* x, int64_t ld, int64_t rows, int64_t cols, void* stream);
/* Its gradient (autograd of decoder.py:43 in the training loops, GripNet-aminer.py:124-147): dx = probs * (grad - sum_c grad_c probs_c) per row. */
GN_API gn_status gn_softmax_rows_backward_f32(const float* probs, int64_t ld_probs, const float* grad, int64_t ld_grad, float* dx,
                                       int64_t ld_dx, int64_t rows, int64_t cols, void* stream);
/* out[i, :] = softmax?( z[node_list[i], :] @ W ), i in [0, m): multiClassInnerProductDecoder.forward in one launch
 * (gripnet/decoder.py:42-43: `pred = torch.matmul(z[node_list], self.weight)`, then `torch.softmax(pred, dim=1)`).
 * node_list may be NULL (rows 0..m-1); an entry outside [0, table_rows) scores a row of zeros, as gn_gemm_f32's a_rows.
 * W is [k, n] row-major.  Up to 16 classes run as one pass over the selected rows; more go through gn_gemm_f32 +
 * gn_softmax_rows_f32. */
GN_API gn_status gn_class_scores_f32(const float* z, int64_t ld_z, int64_t table_rows, const int64_t* node_list, int64_t m,
                              const float* w, int64_t ld_w, int64_t k, int64_t n, int softmax, float* out, int64_t ld_out,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * Multi-relational internal layer (myRGCN, gripnet/layers.py:165-197).
 * The plan caches what depends only on the (static) dd graph: per-destination in-degree over
 * ALL relations (the global mean of layers.py:131) and the relation-major / destination-major
 * edge encodings the kernels stream.  range_list ([R,2] int64, half-open, must tile [0,E) in
 * order as produced by utils.get_range_list) may live on the host or on the device.
 * edge_lo/edge_hi select a contiguous edge sub-range (multi-GPU sharding by relation / edge
 * range); in-degrees are always over the full [0,E) graph.
 */
GN_API gn_status gn_rgcn_plan_create(const int64_t* src, const int64_t* dst, const int64_t* range_list,
                              int range_list_on_host, int64_t num_relations, int64_t num_edges,
                              int64_t num_nodes, int64_t edge_lo, int64_t edge_hi, void* stream,
                              gn_rgcn_plan** plan);
/* flags & GN_RGCN_PLAN_LIGHT: only what the general O(E) kernel reads (the destination-major key list, sorted on the device,
 * in-degrees, the rows' degree order) - none of the host-built schedules of the LDS-resident kernels: for a caller whose edge
 * list changes from call to call (the reference's myRGCN has no set-up cost at all, layers.py:165-169), a fraction of the
 * full plan's build time; its forwards take GN_RGCN_PATH_GENERAL (or the table path beyond its shapes). */
#define GN_RGCN_PLAN_LIGHT 1
GN_API gn_status gn_rgcn_plan_create_ex(const int64_t* src, const int64_t* dst, const int64_t* range_list,
                                 int range_list_on_host, int64_t num_relations, int64_t num_edges,
                                 int64_t num_nodes, int64_t edge_lo, int64_t edge_hi, int flags, void* stream,
                                 gn_rgcn_plan** plan);
GN_API void gn_rgcn_plan_destroy(gn_rgcn_plan* plan);
GN_API int64_t gn_rgcn_plan_input_edges(const gn_rgcn_plan* plan);

/* Timing without marker packets: the NEXT kernel launched by this thread through gn_rgcn_forward_f32 (destination-major
 * kernel) or gn_distmult_plan_forward_f32 (row-class kernel) carries the two HIP events (hipEvent_t, created by the caller)
 * as the start / stop stamps of its own dispatch (hipExtLaunchKernel); hipEventElapsedTime(start, stop) is then the
 * kernel's duration on its stream.  A pair of hipEventRecord calls around a launch costs ~9 us of stream time on this
 * stack - a tenth of the PoSE forward.  gn_time_launch_pending: 1 when the events are still waiting (the call in
 * between took a kernel that does not carry them: time it with event records instead); clears them. */
GN_API gn_status gn_time_next_launch(void* start_event, void* stop_event);
GN_API int gn_time_launch_pending(void);

/* The plan builders (`*_plan_create`, gn_graph_plan_build_blocked) keep two things of the PROCESS between builds: their host
 * threads (GN_PLAN_THREADS of them, parked; a forked child starts its own at its first build) and ONE block of host memory
 * their large arrays come out of (it grows to 5/4 of what the largest build asked for, at most 1 GB; ~110 MB after the
 * decoder plan of PoSE-0, ~500 MB after that of a four times larger list).  gn_host_scratch_release gives the block back
 * to the system (unless a build is using it right now) and returns the bytes freed; the next build starts a new one. */
GN_API size_t gn_host_scratch_release(void);

/* Bytes of caller-provided scratch a gn_rgcn_forward_f32 call with these shapes and flags needs: none on the
 * destination-major kernel, W_r and the slabs of the LDS-accumulator kernel, a slab of rows (<= 256 MB) and the stacked
 * weights on the general path (independent of R and N), the [R, N, out] table on the table path.  (The forward checks the workspace against the kernel IT takes and refuses a smaller one.)
 * The answer is for an x that is 16-byte aligned with ld % 4 == 0; gn_rgcn_forward_choice answers for a given x (the
 * LDS-accumulator kernel reads aligned rows only: a column slice of a concat at an odd offset takes the general kernel). */
GN_API size_t gn_rgcn_workspace_bytes(const gn_rgcn_plan* plan, int64_t in_features, int64_t out_features,
                               int64_t num_bases, int flags);
/* The kernel (GN_RGCN_PATH_*) a gn_rgcn_forward_f32 call on this x takes (x == NULL: on an aligned one, as the two queries
 * without x answer), and (workspace_bytes, nullable) the scratch it needs; -1 for a null plan or non-positive sizes.  The
 * queries answer for a 16-byte aligned `basis` and never refuse; the rules they and the forward share, first one that holds:
 * the table at the top of gripnet_amd/csrc/rgcn_route.hpp. */
GN_API int gn_rgcn_forward_choice(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t in_features,
                                  int64_t out_features, int64_t num_bases, int flags, size_t* workspace_bytes);

#define GN_RGCN_PARTIAL 1        /* flags of gn_rgcn_forward_f32 */
#define GN_RGCN_ARITH_FAST 4     /* dense products on two-term bf16 splits (<= 2^-16 relative per product) instead of the
                                  * default fp32-faithful arithmetic (three-term splits / the fp32 matrix instruction) */
/* GN_RGCN_BASIS_TRANSPOSED: `basis` is stored [bases][fout][fin] - the layer's own parameter seen from the reversed layer of
 * its backward (dx = the same layer on the reversed graph with W_r^T, autograd.rgcn_edge_gradients): no transposed copy per
 * step.  Read by the destination-major kernel only; GN_ERR_UNSUPPORTED on the others (pass a transposed copy there). */
#define GN_RGCN_BASIS_TRANSPOSED 64
/* GN_RGCN_SUM: the sum over the in-edges instead of their mean (RGCNConv of torch_geometric 1.4 / 1.5, aggr='add'):
 *   out[i,:] = act( sum_{e: dst=i} x[src_e] W_{r(e)} + x[i] root + bias ),   root may be NULL (root_weight=False).
 * Served by the general kernel, whose slab product with [basis ; root] carries the root term, the bias and the activation
 * (the row's divisor is simply not applied), and by the table kernel beyond the general kernel's shapes. */
#define GN_RGCN_SUM 128
/* Kernel choice, for tests and measurements (0 = the library decides; a kernel that does not cover the shapes is not
 * forced): (GN_RGCN_PATH_x << GN_RGCN_PATH_SHIFT) in flags.  gn_rgcn_forward_path tells which one a call would take. */
#define GN_RGCN_PATH_SHIFT 8
#define GN_RGCN_PATH_PAIR 1      /* destination-major in basis space (rgcn_pair.hip): no W_r, no workspace, one launch */
#define GN_RGCN_PATH_LDS 3       /* LDS accumulator rows (rgcn_fast.hip) */
#define GN_RGCN_PATH_GENERAL 4   /* any size, O(E) memory: basis-space sums per destination on the fp32 matrix instruction, one dense
                                 * product per slab of rows with [basis ; root] (rgcn_basis.hip); up to 64 bases and 128 input
                                 * features, else the table path */
#define GN_RGCN_PATH_TABLE 5     /* transform-then-gather through an [R, N, out] table in HBM (rgcn.hip): any shape */
GN_API int gn_rgcn_forward_path(const gn_rgcn_plan* plan, int64_t in_features, int64_t out_features, int64_t num_bases, int flags);

/* flags & GN_RGCN_PARTIAL == 0:  out[i,:] = act( (sum_{e: dst=i} x[src_e] W_{r(e)}) / max(1, indeg_i) + x[i] root + bias )
 * flags & GN_RGCN_PARTIAL:       out[i,:] = sum_{e in [edge_lo,edge_hi): dst=i} x[src_e] W_{r(e)}   (un-normalised
 *                                shard contribution; all-reduce it, then call gn_rgcn_finalize_f32)
 * with W_r = sum_b att[r,b] basis[b]  (layers.py:172-173).  bias may be NULL. */
GN_API gn_status gn_rgcn_forward_f32(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t in_features,
                              const float* basis, const float* att, int64_t num_bases, const float* root,
                              const float* bias, int64_t out_features, int relu, int flags, float* out,
                              int64_t ld_out, const gn_side_copy* side /* nullable */,
                              const void* x_planes /* nullable: gn_split_planes.planes of x, written by its producer */,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The same layer with a per-edge factor w_e on every message (edge_norm of RGCNConv):
 *   flags & GN_RGCN_SUM:      out[i,:] = act( sum_{e: dst=i} w_e x[src_e] W_{r(e)} + x[i] root + bias )   (root may be NULL)
 *   flags & GN_RGCN_PARTIAL:  out[i,:] = sum_{e: dst=i} w_e x[src_e] W_{r(e)}
 * (one of the two; the mean has no weighted form).  General kernel only: w_e multiplies att[r(e), b] on the A operand of the
 * fp32 matrix instruction.  edge_weight [E] fp32 is read in the CALLER's edge order through the plan's position list
 * (gn_rgcn_plan_build_positions, once per plan).  Up to 64 bases and 128 input features (gn_rgcn_weighted_supported), else
 * GN_ERR_UNSUPPORTED.  No atomics on floats: the same bits every run. */
GN_API gn_status gn_rgcn_plan_build_positions(gn_rgcn_plan* plan, const int64_t* dst /* the list the plan was built from */,
                                       const int64_t* perm /* nullable: position of every listed edge in the caller's own list */,
                                       void* stream);
GN_API int gn_rgcn_weighted_supported(const gn_rgcn_plan* plan, int64_t in_features, int64_t out_features, int64_t num_bases);
GN_API size_t gn_rgcn_weighted_workspace_bytes(const gn_rgcn_plan* plan, int64_t in_features, int64_t out_features, int64_t num_bases);
GN_API gn_status gn_rgcn_forward_weighted_f32(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t in_features,
                                       const float* basis, const float* att, int64_t num_bases, const float* root,
                                       const float* bias, int64_t out_features, int relu, int flags, const float* edge_weight,
                                       float* out, int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream);

/* out[i,:] = act( summed[i,:] / max(1, indeg_i) + x[i] root + bias )  (layers.py:131,191-197). */
GN_API gn_status gn_rgcn_finalize_f32(const gn_rgcn_plan* plan, const float* summed, int64_t ld_summed, const float* x,
                               int64_t ld_x, int64_t in_features, const float* root, const float* bias,
                               int64_t out_features, int relu, float* out, int64_t ld_out,
                               const gn_side_copy* side /* nullable */, void* stream);

/* Weight gradient of the relational layer (autograd of layers.py:165-197 under the loss of GripNet-pose.py:140-146): with
 * P = sum_e x[src_e] W_{r(e)} and gm = dL/dP ([n, out_features]),
 *   dw[r] = sum_{e in r} x[src_e]^T gm[dst_e]      ([num_relations][in_features][out_features], row-major, overwritten),
 * from which dbasis = att^T dw and datt = dw basis^T (layers.py:172-173).  The plan is built from the plain-sum plan of
 * the layer's edges keyed dst -> relation * n + src (gn_sum_plan_create with num_relations * n targets over n
 * sources: one row per (relation, source), its entries the destinations) and holds what depends on the edges only.
 * One launch: the (relation, source) sums of gm never exist in memory (they were 80 MB per step on PoSE).  No float
 * atomics: the same bits every run.  GN_ERR_UNSUPPORTED (see gn_rel_weight_grad_supported) for in_features other than
 * 16 / 32 / 48 / 64, out_features other than 16 / 32, or a gm table that does not fit the LDS: sum the rows with
 * gn_graph_aggregate_f32 on the plain-sum plan and contract them with x per relation instead. */
/* The same gradient for supervertices beyond the fused kernel (any number of nodes; up to 128 input and 64 output features):
 * per relation the outer products of its edges' endpoint rows on the fp32 matrix instruction, O(E) memory - the reference's
 * own per-relation formulation (layers.py:178-186 under autograd; the all-nodes baseline rgcn_pose.py:53-106).  src / dst:
 * the rows of the caller's [2, E] int64 edge_index the plan was built from (type-sorted; a shard's plan covers its edge
 * range).  workspace: gn_rgcn_weight_grad_workspace_bytes (the parts of relations of more than 512 edges, added in part
 * order: the same bits every run). */
GN_API size_t gn_rgcn_weight_grad_workspace_bytes(const gn_rgcn_plan* plan, int64_t in_features, int64_t out_features);
GN_API int gn_rgcn_weight_grad_supported(const gn_rgcn_plan* plan, int64_t in_features, int64_t out_features);
GN_API gn_status gn_rgcn_weight_grad_f32(const gn_rgcn_plan* plan, const int64_t* src, const int64_t* dst, const float* x, int64_t ld_x,
                                  int64_t in_features, const float* gm, int64_t ld_g, int64_t out_features, float* dw, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* dw[r] = sum_{e in r} w_e x[src_e]^T gm[dst_e]: gn_rgcn_weight_grad_f32 with a per-edge factor, edge_weight [E] fp32 in the
 * order of src / dst (the type-sorted list). */
GN_API gn_status gn_rgcn_weight_grad_weighted_f32(const gn_rgcn_plan* plan, const int64_t* src, const int64_t* dst, const float* edge_weight,
                                           const float* x, int64_t ld_x, int64_t in_features, const float* gm, int64_t ld_g,
                                           int64_t out_features, float* dw, void* workspace, size_t workspace_bytes, void* stream);
typedef struct gn_rel_grad_plan gn_rel_grad_plan;
GN_API gn_status gn_rel_grad_plan_create(const gn_graph_plan* relation_source_sums, int64_t num_nodes, int64_t num_relations,
                                  void* stream, gn_rel_grad_plan** plan);
GN_API void gn_rel_grad_plan_destroy(gn_rel_grad_plan* plan);
GN_API int gn_rel_weight_grad_supported(const gn_rel_grad_plan* plan, int64_t in_features, int64_t out_features);
GN_API gn_status gn_rel_weight_grad_f32(const gn_rel_grad_plan* plan, const float* x, int64_t ld_x, int64_t in_features,
                                 const float* gm, int64_t ld_gm, int64_t out_features, float* dw, void* stream);

/* ---------------------------------------------------------------------------------------
 * DistMult decoder (multiRelaInnerProductDecoder.forward, gripnet/decoder.py:19-23):
 *   out[e] = sigma?( sum_k z[u_e,k] * z[v_e,k] * D[r_e,k] ).
 * Consumes the raw int64 edge_index rows and edge_type every call (negative samples change
 * every epoch, GripNet-pose.py:131), so nothing is cached.  An endpoint or relation outside its
 * table yields NaN for that edge and sets bit 0 of *error_flag (device int32, may be NULL). */
GN_API gn_status gn_distmult_forward_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features,
                                  const int64_t* u, const int64_t* v, const int64_t* edge_type,
                                  const float* d, int64_t ld_d, int64_t num_relations, int64_t num_edges,
                                  int apply_sigmoid, float* out, int32_t* error_flag, void* stream);

/* The same decoder (same kernel, same arithmetic, same bits) on PACKED triples: packed_uv[e] = u | v << 16 and
 * relation[e] (uint16): 6 bytes per edge and column phase instead of 24.  For edge lists that change every epoch, where
 * a plan cannot pay off: the negative samples of GripNet-pose.py:131,138, which gn_negative_sampler_sample_packed writes
 * in this form; `relation` is the static edge_type of the positives (GripNet-pose.py:138 scores the negatives with
 * train_et) narrowed once.  GN_ERR_UNSUPPORTED when ids need more than 16 bits or the node table does not fit the LDS
 * in four column phases. */
GN_API gn_status gn_distmult_packed_forward_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features,
                                         const uint32_t* packed_uv, const uint16_t* relation, const float* d, int64_t ld_d,
                                         int64_t num_relations, int64_t num_edges, int apply_sigmoid, float* out,
                                         int32_t* error_flag, void* stream);

/* The same decoder on a cached, re-encoded STATIC edge list: the positive edges, which the reference scores with the
 * same train_idx / train_et tensors every epoch (GripNet-pose.py:137,185).  The plan validates the triples once
 * (GN_ERR_INDEX_RANGE), pairs up triples with the same unordered node pair and relation (both directions of an edge,
 * utils.py:132-138: the same score bit for bit, computed once and written to both positions), packs the scored ones
 * into 32-bit words and orders them inside every 64-edge batch for conflict-free LDS gathers; scores come out in the
 * caller's edge order, bitwise equal to gn_distmult_forward_f32.
 * Plan creation copies the triples to the host and synchronises `stream`.  GN_ERR_UNSUPPORTED: more than 8192 nodes
 * or 65535 relations (create), or a node table that does not fit the LDS in four column phases (forward) - use
 * gn_distmult_forward_f32 then. */
typedef struct gn_distmult_plan gn_distmult_plan;
GN_API gn_status gn_distmult_plan_create(const int64_t* u, const int64_t* v, const int64_t* edge_type, int64_t num_edges,
                                  int64_t num_nodes, int64_t num_relations, int64_t num_features, void* stream,
                                  gn_distmult_plan** plan);
GN_API void gn_distmult_plan_destroy(gn_distmult_plan* plan);
GN_API int64_t gn_distmult_plan_edges(const gn_distmult_plan* plan);
GN_API gn_status gn_distmult_plan_forward_f32(const gn_distmult_plan* plan, const float* z, int64_t ld_z, int64_t num_features,
                                       const float* d, int64_t ld_d, int apply_sigmoid, float* out, void* stream);
/* The same scores in several launches: feature columns [col_lo, col_hi) only (col_lo a multiple of 4; z and d point at
 * column 0, ld_z >= col_hi).  The launch with col_lo = 0 starts the sums; a launch with col_hi < num_features leaves raw
 * partial sums in `out` (at the edges' own positions), the next one continues from them; the launch with
 * col_hi = num_features applies the sigmoid and fills the mirror positions.  Split at the column where the
 * single launch would change phase (48 of 80 at 645 nodes) the scores are the same bits.  For the relation-sharded
 * forward: the columns that are the relational layer's INPUT (concat slot 0 of homoGraph / interGraph, gripnet/layers.py:264-266)
 * are scored while the all-reduce of the layer's partial sums is in flight. */
GN_API gn_status gn_distmult_plan_forward_cols_f32(const gn_distmult_plan* plan, const float* z, int64_t ld_z, int64_t num_features,
                                            int64_t col_lo, int64_t col_hi, const float* d, int64_t ld_d, int apply_sigmoid,
                                            float* out, void* stream);

/* Backward of the DistMult decoder (autograd of decoder.py:19-23 under the loss of GripNet-pose.py:140-146).
 * grad_logit[e] = d loss / d s_e (the caller folds the sigmoid derivative in).  dz [n, F] and dD [R, F]
 * are overwritten:  dz[u_e] += g_e z[v_e] * D[r_e],  dz[v_e] += g_e z[u_e] * D[r_e],  dD[r_e] += g_e z[u_e] * z[v_e].
 * Edges with an id outside its table contribute nothing.  Sort-based segmented reduction: no atomics,
 * bitwise reproducible.  Scratch is caller-provided (gn_distmult_backward_workspace_bytes).
 * gn_distmult_backward_ex_f32 takes flags: GN_DM_TYPES_SORTED promises that edge_type is non-decreasing (the
 * reference's layout, utils.py:168-198), which saves the sort of the dD pass.  sigmoid_scores (the probabilities the
 * forward returned, decoder.py:23) makes grad_logit the gradient with respect to those: the factor p (1 - p) is
 * applied where the records are built.  type_offsets ([R + 1] int32 on the device, with GN_DM_TYPES_SORTED): the first
 * edge of every relation, for callers that keep it with a static edge_type instead of having it searched per call.
 * GN_DM_TYPE_TASKS: type_offsets points at a buffer that gn_distmult_type_tasks filled for this (R, E) - the offsets and,
 * behind them, the task list of the relation-major reduction, which then is not rebuilt per call (a one-workgroup launch
 * of 7 us).  Node and relation tables that fit the LDS in 16-column blocks ((n + R) * 64 B <= 150 KB) are reduced from
 * there; larger ones from L2. */
#define GN_DM_TYPES_SORTED 1
#define GN_DM_TYPE_TASKS 2
GN_API size_t gn_distmult_type_tasks_bytes(int64_t num_relations, int64_t num_edges);
/* out (16-byte aligned, gn_distmult_type_tasks_bytes bytes; may be where type_offsets already sits): type_offsets [R + 1],
 * then the task list. */
GN_API gn_status gn_distmult_type_tasks(const int32_t* type_offsets, int64_t num_relations, int64_t num_edges, void* out,
                                 size_t out_bytes, void* stream);
/* The same gradients from the triples as the negative sampler leaves them next to its int64 output
 * (gn_negative_sampler_sample_packed / _stepped): packed_uv[e] = u | v << 16 and a 16-bit relation id per position (the
 * static edge_type, narrowed once by the caller) - 6 instead of 24 bytes per edge in each pass of the counting sort.  Takes
 * the counting-sort / LDS path only: GN_DM_TYPES_SORTED with type_offsets, tables that fit the LDS, at most 4,096 nodes;
 * GN_ERR_UNSUPPORTED otherwise (call gn_distmult_backward_ex_f32 on the int64 arrays).  Same bits as the int64 call. */
GN_API gn_status gn_distmult_backward_packed_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features,
                                          const uint32_t* packed_uv, const uint16_t* rel16, const float* d, int64_t ld_d,
                                          int64_t num_relations, int64_t num_edges, const float* grad_logit, float* dz,
                                          int64_t ld_dz, float* dd, int64_t ld_dd, int flags, const float* sigmoid_scores,
                                          const int32_t* type_offsets, void* workspace, size_t workspace_bytes, void* stream);
GN_API size_t gn_distmult_backward_workspace_bytes(int64_t num_nodes, int64_t num_features, int64_t num_relations,
                                            int64_t num_edges);
GN_API gn_status gn_distmult_backward_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features,
                                   const int64_t* u, const int64_t* v, const int64_t* edge_type, const float* d,
                                   int64_t ld_d, int64_t num_relations, int64_t num_edges, const float* grad_logit,
                                   float* dz, int64_t ld_dz, float* dd, int64_t ld_dd, void* workspace,
                                   size_t workspace_bytes, void* stream);
GN_API gn_status gn_distmult_backward_ex_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features,
                                      const int64_t* u, const int64_t* v, const int64_t* edge_type, const float* d,
                                      int64_t ld_d, int64_t num_relations, int64_t num_edges, const float* grad_logit,
                                      float* dz, int64_t ld_dz, float* dd, int64_t ld_dd, int flags,
                                      const float* sigmoid_scores /* nullable */,
                                      const int32_t* type_offsets /* nullable */, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* The same gradients for a STATIC edge list (the positive edges, scored with the same tensors every epoch,
 * GripNet-pose.py:137).  What the sort and the reductions derive from the triples alone is built once: the two
 * directions of an edge (same unordered node pair and relation) are paired up - their records differ only in g, so a
 * pair is reduced as one triple with g1 + g2 -, and the scanned offsets of the counting sort and the task lists of
 * what is left are kept; a call sums the pairs' gradients, starts at the scatter pass and runs the two segment
 * reductions (6 launches instead of 12, on half the records for a bidirectional list).  Create copies the triples to
 * the host, validates them (GN_ERR_INDEX_RANGE) and synchronises `stream`; GN_ERR_UNSUPPORTED when the tables do not
 * fit the LDS path or edge_type is not sorted (create), when rows are not aligned float4 columns or the list is too
 * long for the staged scatter (backward): use gn_distmult_backward_f32 then.  Results equal the plan-less call up to
 * the rounding of g1 + g2 and are bitwise reproducible. */
typedef struct gn_distmult_bwd_plan gn_distmult_bwd_plan;
GN_API gn_status gn_distmult_bwd_plan_create(const int64_t* u, const int64_t* v, const int64_t* edge_type, int64_t num_edges,
                                      int64_t num_nodes, int64_t num_relations, void* stream, gn_distmult_bwd_plan** plan);
GN_API void gn_distmult_bwd_plan_destroy(gn_distmult_bwd_plan* plan);
GN_API size_t gn_distmult_bwd_plan_workspace_bytes(const gn_distmult_bwd_plan* plan, int64_t num_features);
GN_API gn_status gn_distmult_backward_planned_f32(const gn_distmult_bwd_plan* plan, const float* z, int64_t ld_z,
                                           int64_t num_features, const float* d, int64_t ld_d,
                                           const float* grad_logit, const float* sigmoid_scores /* nullable */,
                                           float* dz, int64_t ld_dz, float* dd, int64_t ld_dd, void* workspace,
                                           size_t workspace_bytes, void* stream);

/* The decoder's backward fed by the LINK LOSS directly (round 6): the scores of a list go into the loss of
 * GripNet-pose.py:140-142, -mean(log(p + eps)) over the positives' list or -mean(log(1 - p + eps)) over the negatives', and
 * d loss / d s_e = (-+ upstream / num_edges) / (p_e (or 1 - p_e) + eps) * p_e (1 - p_e) is a function of the edge's own probability
 * only - it is computed where the edge records are built, in the arithmetic of gn_link_loss_backward_f32 followed by the
 * sigmoid factor (the SAME bits as the two-step path), and the loss's backward launch and the [E] gradient vector's round
 * trip through memory disappear.  upstream: the loss's one upstream gradient on the device (NULL: 1).
 * dz_addend / dd_addend (packed form): the gradients of the SAME z and D from the step's other list (the positives' call): added
 * where this call stores its sums (dz = sums + dz_addend, may alias dz), so that the two lists' gradients need no adding launch;
 * GN_ERR_UNSUPPORTED where the two reductions do not share their combine launch, or where an addend's rows are not 16-byte
 * aligned with a leading dimension % 4 == 0 (call without addends and add); GN_ERR_INVALID_ARG for an addend's leading
 * dimension below num_features or addends with an empty list. */
typedef struct gn_link_loss_grad {
    const float* upstream;
    float eps;
    int negative;              /* 0: the list's scores are the loss's positives, 1: its negatives */
} gn_link_loss_grad;
GN_API gn_status gn_distmult_backward_loss_packed_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features,
                                               const uint32_t* packed_uv, const uint16_t* rel16, const float* d, int64_t ld_d,
                                               int64_t num_relations, int64_t num_edges, const gn_link_loss_grad* loss,
                                               const float* sigmoid_scores, float* dz, int64_t ld_dz, float* dd, int64_t ld_dd,
                                               int flags, const int32_t* type_offsets,
                                               const float* dz_addend /* nullable */, int64_t ld_dz_addend,
                                               const float* dd_addend /* nullable */, int64_t ld_dd_addend,
                                               void* workspace, size_t workspace_bytes, void* stream);
GN_API gn_status gn_distmult_backward_loss_planned_f32(const gn_distmult_bwd_plan* plan, const float* z, int64_t ld_z,
                                                int64_t num_features, const float* d, int64_t ld_d,
                                                const gn_link_loss_grad* loss, const float* sigmoid_scores,
                                                float* dz, int64_t ld_dz, float* dd, int64_t ld_dd, void* workspace,
                                                size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Knowledge-graph-embedding scorers of the link-prediction baselines (KGEModel.forward,
 * baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:127-235).  With h = ent[head_e], t = ent[tail_e],
 * r = rel[edge_type_e] and H = hidden_dim:
 *   GN_KGE_TRANSE    ent [n, H],  rel [R, H]    s_e = gamma - sum_k |h_k + r_k - t_k|                          (:189-193)
 *   GN_KGE_DISTMULT  ent [n, H],  rel [R, H]    s_e = sum_k h_k r_k t_k                                        (:195-199)
 *   GN_KGE_COMPLEX   ent [n, 2H], rel [R, 2H]   s_e = sum_k (hr rr - hi ri) tr + (hr ri + hi rr) ti            (:201-211)
 *   GN_KGE_ROTATE    ent [n, 2H], rel [R, H]    s_e = gamma - sum_k sqrt(a_k^2 + b_k^2),  theta = r / phase_divisor,
 *                                               a = hr cos - hi sin - tr,  b = hr sin + hi cos - ti            (:213-235)
 * (real part: columns [0, H), imaginary part: columns [H, 2H)).  phase_divisor is the fp32 value of embedding_range / pi
 * (:221): the phases are divided by it, not multiplied by a reciprocal.  out[e] = s_e, or with log_sigmoid
 * min(s, 0) - log1p(exp(-|s|)) (:187); raw_out (nullable) receives s_e as well.  cos / sin are evaluated once per call
 * for the relation table, into `workspace` (gn_kge_forward_workspace_bytes bytes, 16-byte aligned; 0 for the other
 * models).  A head, tail or relation outside its table yields NaN for that triple and sets bit 0 of *error_flag (device
 * int32, may be NULL).  GN_ERR_INVALID_ARG: an unknown model, a null operand, a leading dimension below the row length,
 * a zero phase_divisor, a workspace that is too small; GN_ERR_UNSUPPORTED: 2^31 - 512 or more rows in a table, 2^31 - 2048
 * or more triples, a hidden_dim of 2^29 or more. */
#define GN_KGE_TRANSE 0
#define GN_KGE_DISTMULT 1
#define GN_KGE_COMPLEX 2
#define GN_KGE_ROTATE 3
GN_API size_t gn_kge_forward_workspace_bytes(int model, int64_t num_relations, int64_t hidden_dim);
GN_API gn_status gn_kge_forward_f32(int model, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                             int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* head,
                             const int64_t* tail, const int64_t* edge_type, int64_t num_edges, float gamma,
                             float phase_divisor, int log_sigmoid, float* out, float* raw_out /* nullable */,
                             int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the scorers (autograd of :127-235 under the loss of :266-268).  grad_out[e] is the gradient with respect
 * to what the forward returned: with raw_scores (the s_e of raw_out) that is the log-sigmoid, and the factor sigma(-s_e)
 * is applied where the records are built; with raw_scores = NULL it is s_e itself.  d_ent [n, De] and d_rel [R, Dr] are
 * overwritten with the sums of g_e * ds_e/d(row) over the triples of every row; rows without a triple get exact zeros;
 * triples with an id outside its table contribute nothing.  torch's subgradients: sign(0) = 0 (TransE), a term with
 * a = b = 0 contributes nothing (RotatE).  Three passes (key = head, + key = tail, key = relation) of a sort-based
 * segmented reduction: no float atomics, chunk partials added in chunk order, two calls give the same bits.
 * flags: GN_DM_TYPES_SORTED promises a non-decreasing edge_type - the relation pass then skips its sort and takes the row
 * offsets by binary search.  Scratch is caller-provided: gn_kge_backward_workspace_bytes bytes, 256-byte aligned.
 * Refusals as for the forward. */
GN_API size_t gn_kge_backward_workspace_bytes(int model, int64_t num_entities, int64_t num_relations, int64_t hidden_dim,
                                       int64_t num_edges);
GN_API gn_status gn_kge_backward_f32(int model, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                              int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* head,
                              const int64_t* tail, const int64_t* edge_type, int64_t num_edges, float phase_divisor,
                              const float* grad_out, const float* raw_scores /* nullable */, float* d_ent, int64_t ld_dent,
                              float* d_rel, int64_t ld_drel, int flags, void* workspace, size_t workspace_bytes,
                              void* stream);

/* The scorers on candidate blocks: the 'head-batch' / 'tail-batch' modes of KGEModel.forward (:127-136, :150-173).  A
 * positive b is (fixed[b], edge_type[b]) with K candidate entities cand[b * ld_cand + k] (int64, ld_cand >= K) and a side
 * (GN_KGE_SIDE_TAIL 0, GN_KGE_SIDE_HEAD 1, defined with the ranking entry points below):
 *   tail side: fixed is the head,  out[b * K + k] = s(fixed[b], edge_type[b], cand[b, k])
 *   head side: fixed is the tail,  out[b * K + k] = s(cand[b, k], edge_type[b], fixed[b])
 * or its log-sigmoid; raw_out (nullable, [B, K]) receives s as well.  Tables, gamma, phase_divisor, models, hidden sizes and
 * the workspace (gn_kge_batch_forward_workspace_bytes, 16-byte aligned) are those of gn_kge_forward_f32, and every score is
 * bit for bit what gn_kge_forward_f32 gives for that triple in a list: the same lanes per score, column order, term
 * arithmetic and fold.  8 bytes of ids are read per score instead of 24, and the query's rows once per 64 candidates.
 * A fixed entity or relation outside its table makes the whole row NaN, a candidate outside makes its element NaN; either
 * sets bit 0 of *error_flag; nothing outside a table is read.  B == 0 or K == 0: nothing is written.
 * GN_ERR_UNSUPPORTED: B * K beyond the triple count gn_kge_forward_f32 takes. */
GN_API size_t gn_kge_batch_forward_workspace_bytes(int model, int64_t num_relations, int64_t hidden_dim);
GN_API gn_status gn_kge_batch_forward_f32(int model, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                                   int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* fixed,
                                   const int64_t* edge_type, const int64_t* cand, int64_t ld_cand, int64_t num_positives,
                                   int64_t num_candidates, int side, float gamma, float phase_divisor, int log_sigmoid,
                                   float* out, float* raw_out /* nullable */, int32_t* error_flag, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* Their backward.  grad_out [B, K] (contiguous) and raw_scores (nullable, [B, K]) as for gn_kge_backward_f32; d_ent and
 * d_rel are overwritten.  No float atomics, no host synchronisation, the same bits in every call:
 *   - the candidates' rows: B * K records keyed by the candidate through the list backward's segmented reduction;
 *   - the fixed entity's and the relation's rows: per positive the K contributions are summed first (a workgroup per
 *     positive, k ascending within one of its 256 / lanes slots, the slots folded in slot order) into one partial row per
 *     positive and role; two segmented reductions over B records keyed by fixed[b] and edge_type[b] then add those rows;
 *   - d_ent is the candidate pass plus the fixed-entity pass.
 * GN_DM_TYPES_SORTED in flags promises a non-decreasing edge_type [B]: the relation pass skips its sort.  Positives and
 * candidates with an id outside its table contribute nothing.  B == 0 or K == 0: zero gradients.  Scratch:
 * gn_kge_batch_backward_workspace_bytes bytes, 256-byte aligned. */
GN_API size_t gn_kge_batch_backward_workspace_bytes(int model, int64_t num_entities, int64_t num_relations, int64_t hidden_dim,
                                             int64_t num_positives, int64_t num_candidates);
GN_API gn_status gn_kge_batch_backward_f32(int model, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                                    int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* fixed,
                                    const int64_t* edge_type, const int64_t* cand, int64_t ld_cand, int64_t num_positives,
                                    int64_t num_candidates, int side, float phase_divisor, const float* grad_out,
                                    const float* raw_scores /* nullable */, float* d_ent, int64_t ld_dent, float* d_rel,
                                    int64_t ld_drel, int flags, void* workspace, size_t workspace_bytes, void* stream);

/* The scorers on SHARED candidate lists (the 'tail-shared' / 'head-shared' modes of gripnet_amd.KGEModel; no counterpart in
 * the reference: what DGL-KE and PyTorch-BigGraph do with their negatives).  The B positives (fixed[b], edge_type[b]) are cut
 * into G = num_lists chunks of B / G consecutive positives (1 <= G <= B, B % G == 0) and chunk g comes with ONE list of K
 * candidate entities cand[g * ld_cand + k] (int64, ld_cand >= K):
 *   g = b / (B / G)
 *   tail side: fixed is the head,  out[b * K + k] = s(fixed[b], edge_type[b], cand[g, k])
 *   head side: fixed is the tail,  out[b * K + k] = s(cand[g, k], edge_type[b], fixed[b])
 * or its log-sigmoid; raw_out (nullable, [B, K]) receives s as well.  G == B is gn_kge_batch_forward_f32's meaning.  Tables,
 * gamma, phase_divisor, models and the workspace (gn_kge_shared_forward_workspace_bytes, 16-byte aligned) are those of
 * gn_kge_forward_f32; entity rows of at most 128 floats (hidden_dim <= 128 for TransE and DistMult, <= 64 for ComplEx and
 * RotatE: the ranking limit), GN_ERR_UNSUPPORTED beyond.  G * K entity rows are gathered instead of B * K: a workgroup owns 64
 * positives of one chunk (16 per wave) and walks the list in stages of 64 candidate rows held in LDS, each gathered once
 * per workgroup.  The sum over the columns:
 *   DistMult, ComplEx   the query row q with s = <q, candidate row> is prepared once per positive (h r, the complex product, or
 *                       for the head side r t and its conjugate form, every product rounded as gn_kge_forward_f32 rounds it)
 *                       and contracted on v_mfma_f32_16x16x4_f32, each instruction a chain of four fp32 fused multiply-adds:
 *                       step s = 0 .. S - 1 takes the columns s, S + s, 2 S + s, 3 S + s in that order, S a quarter of the
 *                       row's length padded to a multiple of 16.  The steps go in groups of four to FOUR partial sums in turn
 *                       (group i = steps 4 i .. 4 i + 3 to partial i % 4, ascending i within a partial) and the score is
 *                       (p0 + p1) + (p2 + p3): a row of 128 floats is four chains of 32, not one of 128.  The value is NOT the bits of
 *                       gn_kge_forward_f32 for that triple (another order, products fused into the sum); it is held to the
 *                       same per-element bound;
 *   TransE, RotatE      the per-column terms of gn_kge_forward_f32 (the same operations in the same order), added in ascending
 *                       column order on the vector ALU, then gamma - sum.  TransE on tables where h + r - t and the sums are
 *                       exact gives the bits of gn_kge_batch_forward_f32.
 * A fixed entity or relation outside its table makes the whole row NaN, a candidate outside makes its column of its chunk NaN;
 * either sets bit 0 of *error_flag; nothing outside a table is read.  B == 0 or K == 0: nothing is written.  16-byte stores
 * where K % 4 == 0 and out / raw_out are 16-byte aligned.  GN_ERR_INVALID_ARG: a G that does not divide B. */
GN_API size_t gn_kge_shared_forward_workspace_bytes(int model, int64_t num_relations, int64_t hidden_dim);
GN_API gn_status gn_kge_shared_forward_f32(int model, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                                    int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* fixed,
                                    const int64_t* edge_type, const int64_t* cand, int64_t ld_cand, int64_t num_positives,
                                    int64_t num_lists, int64_t num_candidates, int side, float gamma, float phase_divisor,
                                    int log_sigmoid, float* out, float* raw_out /* nullable */, int32_t* error_flag,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* Their backward.  grad_out [B, K] (contiguous) and raw_scores (nullable, [B, K]) as for gn_kge_backward_f32; d_ent and
 * d_rel are overwritten.  No float atomics, no host synchronisation, the same bits in every call:
 *   - g[b, k] = grad_out, times sigma(-s) with raw_scores, is formed once;
 *   - query side: per positive the K contributions g[b, k] ds / d(fixed row) and g[b, k] ds / d(relation row) are summed in
 *     ascending k, one fused multiply-add each, into one partial row per positive and role (a thread per positive and
 *     column);
 *   - candidate side: per list entry (g, k) the B / G contributions g[b, k] ds / d(candidate row) of its chunk's positives
 *     are summed in ascending b into one partial row per entry (a thread per entry and column);
 *   - three segmented reductions (chunks of 32 records) add the partial rows: G * K records keyed by cand[g, k] into d_ent,
 *     B records keyed by fixed[b] onto it, B records keyed by edge_type[b] into d_rel.  A candidate that repeats in a list,
 *     in several lists or equals a positive's own entity is one more record of its row.
 * The derivatives are those of gn_kge_backward_f32, per column.  GN_DM_TYPES_SORTED in flags promises a non-decreasing
 * edge_type [B]: the relation pass skips its sort.  Positives and candidates with an id outside its table contribute nothing;
 * rows that nothing touched get exact zeros.  B == 0 or K == 0: zero gradients.  Scratch:
 * gn_kge_shared_backward_workspace_bytes bytes, 256-byte aligned. */
GN_API size_t gn_kge_shared_backward_workspace_bytes(int model, int64_t num_entities, int64_t num_relations, int64_t hidden_dim,
                                              int64_t num_positives, int64_t num_lists, int64_t num_candidates);
GN_API gn_status gn_kge_shared_backward_f32(int model, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                                     int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* fixed,
                                     const int64_t* edge_type, const int64_t* cand, int64_t ld_cand, int64_t num_positives,
                                     int64_t num_lists, int64_t num_candidates, int side, float phase_divisor,
                                     const float* grad_out, const float* raw_scores /* nullable */, float* d_ent,
                                     int64_t ld_dent, float* d_rel, int64_t ld_drel, int flags, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* The negative-sampling loss of a KGE mini-batch on RAW scores, and its gradient: pos [B] (gn_kge_forward_f32 without the
 * log-sigmoid), neg [B, K] with a leading dimension ld_neg >= K (gn_kge_batch_forward_f32 likewise), weight [B] (nullable: 1;
 * the subsampling weights of the code base KGEModel comes from, constants) and, with `adversarial` != 0, a temperature T.
 * With ls(x) = min(x, 0) - log1p(exp(-|x|)):
 *   P_b = ls(pos_b)
 *   N_b = (1 / K) sum_k ls(-s_bk)                                              (adversarial == 0; temperature is not read)
 *   N_b = sum_k p_bk ls(-s_bk),   p_b = softmax_k(T s_bk), a constant          (adversarial != 0)
 *   W   = sum_b w_b                                                            (B without weights)
 *   loss = -(sum_b w_b P_b) / (2 W) - (sum_b w_b N_b) / (2 W)
 *   d_pos[b]    = -g w_b sigma(-pos_b) / (2 W)
 *   d_neg[b, k] = +g w_b p_bk sigma(s_bk) / (2 W)                              (p_bk = 1 / K when adversarial == 0)
 * g = *upstream (a device scalar; NULL: 1).  Without weights this is the loss of TransE_DistMult_ComplEx_RotatE.py:266-286
 * on one block, (-logsigmoid(pos).mean() - neg.mean()) / 2.
 * Forward, one launch, every score read once: *loss, *scale = 1 / (2 W) and, per row, row_stats[2 b] = m_b = max_k fl(T s_bk)
 * and row_stats[2 b + 1] = 1 / Z_b, Z_b = sum_k exp(T s_bk - m_b), which the backward recomputes p_bk from: the argument is
 * the single rounding fmaf(T, s, -m_b), the exponential the library's expf (not the hardware's exp2 on x log2 e, which
 * loses |x| units at the arguments down to -87 that a weight far below its row's maximum has).  row_stats may be NULL when
 * adversarial == 0; given there, its second word carries 1 / K, or NaN for a row with a NaN score.  Rows of up to 32 scores
 * share a wave in power-of-two lane groups, a longer row is one wave's, held in registers up to 1,024 scores and taken in
 * parts of 1,024 with a running maximum beyond; 16-byte loads when neg is 16-byte aligned and ld_neg a multiple of four,
 * 4-byte loads into the same registers otherwise (the same bits).  The sums over a row and over the rows are taken in
 * double, each in a fixed order: rows are dealt to the waves by the grid, a workgroup's three partial sums are added in
 * workgroup order by the last workgroup to arrive.  No float atomics, no host synchronisation, capturable.
 * Backward, one launch: d_pos [B] and d_neg [B, K] (ld_dneg >= K) from the scores and row_stats / scale as the forward
 * left them; nothing else of size [B, K] exists.  An element is g * (c_b * (e * sigma(s))) with c_b = w_b / (2 W Z_b) taken in
 * double and rounded once: an upstream of 1 changes no bit, any other costs one rounding.
 * A NaN score makes the loss NaN and its row of d_neg NaN (without row_stats: its own element); a NaN positive makes the
 * loss and its d_pos NaN; every other gradient element keeps its bits.  A row with w_b = 0 gets exact zeros.
 * `workspace`: gn_kge_ns_loss_workspace_bytes(B) bytes, 8-byte aligned, ZEROED ONCE by the caller (the launch leaves it
 * ready for the next one); calls on one workspace must be stream-ordered.
 * GN_ERR_INVALID_ARG: B < 1 or K < 1 (K < 2^31), a leading dimension below K, a null operand, a short workspace. */
GN_API size_t gn_kge_ns_loss_workspace_bytes(int64_t num_positives);
GN_API gn_status gn_kge_ns_loss_forward_f32(const float* pos, const float* neg, int64_t ld_neg, int64_t num_positives,
                                     int64_t num_candidates, const float* weight /* nullable */, int adversarial,
                                     float temperature, float* loss /* [1] */,
                                     float* row_stats /* [B, 2]; nullable unless adversarial */, float* scale /* [1]: 1 / (2 W) */,
                                     void* workspace, size_t workspace_bytes, void* stream);
GN_API gn_status gn_kge_ns_loss_backward_f32(const float* pos, const float* neg, int64_t ld_neg, int64_t num_positives,
                                      int64_t num_candidates, const float* weight /* nullable */, int adversarial,
                                      float temperature, const float* row_stats, const float* scale,
                                      const float* upstream /* device, nullable */, float* d_pos, float* d_neg, int64_t ld_dneg,
                                      void* stream);

/* ---------------------------------------------------------------------------------------
 * Graph attention: GATConv of torch_geometric 1.4 / 1.5 as baselines/NC_baselines/GAT.py uses it (single `weight`, single
 * `att`).  The graph is a plan of gn_gcn_plan_create: it is the layer's working list already - input loops dropped, one
 * loop per node, duplicate edges kept, in-edges of a node in input order - and an id outside [0, N) is refused there as
 * for myGCN (GN_ERR_INDEX_RANGE); its coefficients are not read.  With h = x W [N, H * C] (gn_gemm_f32), att [H, 2 C]
 * (a head's target half, then its source half) and l_e = leaky_relu(a_dst[i] + a_src[j]) for an edge j -> i:
 *   gn_gat_logits_f32        a_dst[i, h] = sum_c h[i, h, c] att[h, c],  a_src[i, h] = sum_c h[i, h, c] att[h, C + c]
 *   gn_gat_forward_f32       m[i, h] = max_e l_e,  s = sum_e exp(l_e - m),  o[i, h, :] = (sum_e exp(l_e - m) h[j_e, h, :]) / s,
 *                            out = act(o as [N, H * C] + bias)  (concat)  or  act(mean_h o + bias) [N, C];  o_save (nullable,
 *                            [N, H * C] contiguous) receives o, rinv = 1 / s.  (PyG's 1e-16 in the denominator is below half
 *                            a unit of s >= 1 and is left out.)  exp is 2^(x log2 e) on the hardware instruction.
 *   gn_gat_backward_dst_f32  from g = dL/d(out before bias and act) ([N, H * C], or [N, C] for the head mean, whose 1 / H the
 *                            kernel applies): D[i, h] = g[i, h, :] . o[i, h, :],  dz_e = alpha_e (g[i, h, :] . h[j, h, :] - D)
 *                            (z_e > 0 ? 1 : slope),  da_dst[i, h] = sum_{e into i} dz_e;  pack [N, H, 4] (16-byte aligned)
 *                            receives (a_dst, m, rinv, D) for the next pass.
 *   gn_gat_backward_src_f32  over the plan's source-major CSR (gn_graph_plan_build_transpose first):  da_src[j, h] =
 *                            sum_{e out of j} dz_e,  dh[j, h, :] = sum_{e out of j} alpha_e g[i_e, h, :] + da_dst[j, h] att[h, :C]
 *                            + da_src[j, h] att[h, C:].
 *   gn_gat_att_grad_f32      d_att[h, :C] = sum_i da_dst[i, h] h[i, h, :],  d_att[h, C:] likewise with da_src: blocks of 32
 *                            nodes, 64 blocks each, then what is left in order.  Scratch: gn_gat_att_grad_workspace_bytes bytes, 4-byte aligned.
 * alpha_e is recomputed from (a_dst, a_src, m, rinv): nothing of size [E', H] is kept.  No float atomics, every sum in a
 * fixed order: two calls give the same bits.  A node of any degree is one wave's (its edges in turns of the wave's lane
 * groups).  GN_ERR_INVALID_ARG: H * C above GN_GAT_MAX_ROW, a plan of another kind, a null operand, a leading dimension
 * below the row length. */
#define GN_GAT_MAX_ROW 128
GN_API gn_status gn_gat_logits_f32(const float* h, int64_t ld_h, int64_t num_nodes, int64_t heads, int64_t channels,
                            const float* att, float* a_dst, float* a_src, void* stream);
GN_API gn_status gn_gat_forward_f32(const gn_graph_plan* plan, const float* h, int64_t ld_h, int64_t heads, int64_t channels,
                             const float* a_dst, const float* a_src, float negative_slope, const float* bias /* nullable */,
                             int concat, int relu, float* out, int64_t ld_out, float* o_save /* nullable */, float* m,
                             float* rinv, void* stream);
GN_API gn_status gn_gat_backward_dst_f32(const gn_graph_plan* plan, const float* h, int64_t ld_h, int64_t heads, int64_t channels,
                                  const float* a_dst, const float* a_src, const float* m, const float* rinv,
                                  float negative_slope, const float* g, int64_t ld_g, int concat, const float* o, float* pack,
                                  float* da_dst, void* stream);
GN_API gn_status gn_gat_backward_src_f32(const gn_graph_plan* plan, const float* h, int64_t ld_h, int64_t heads, int64_t channels,
                                  const float* a_src, const float* pack, float negative_slope, const float* g, int64_t ld_g,
                                  int concat, const float* da_dst, const float* att, float* dh, int64_t ld_dh, float* da_src,
                                  void* stream);
GN_API size_t gn_gat_att_grad_workspace_bytes(int64_t num_nodes, int64_t heads, int64_t channels);
GN_API gn_status gn_gat_att_grad_f32(const float* h, int64_t ld_h, int64_t num_nodes, int64_t heads, int64_t channels,
                              const float* da_dst, const float* da_src, float* d_att, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * Typed negative sampling on the device (replaces gripnet/utils.py:98-119 and its per-epoch host round
 * trip, GripNet-pose.py:131).  The sampler sorts the positive pairs of every relation block once
 * (range_list on the host, [R,2], must tile [0,E)); gn_negative_sampler_sample then writes, for every
 * positive edge e of block r, one pair (u, v) drawn uniformly (with replacement) from the n^2 pairs
 * that are not positives of block r.  Deterministic in `seed`.  Bit 1 of *error_flag (device int32,
 * may be NULL) is set if a block's positives leave (almost) no pair to draw. */
typedef struct gn_negative_sampler gn_negative_sampler;
GN_API gn_status gn_negative_sampler_create(const int64_t* u, const int64_t* v, const int64_t* range_list_host,
                                     int64_t num_relations, int64_t num_edges, int64_t num_nodes, void* stream,
                                     gn_negative_sampler** sampler);
GN_API void gn_negative_sampler_destroy(gn_negative_sampler* sampler);
GN_API gn_status gn_negative_sampler_sample(const gn_negative_sampler* sampler, uint64_t seed, int64_t* out_u,
                                     int64_t* out_v, int32_t* error_flag, void* stream);
/* The same draw, which also leaves every pair as one 32-bit word u | v << 16 (graphs of up to 65,535 nodes) for
 * gn_distmult_packed_forward_f32: the sampler produces the pairs, so it can hand the decoder 4 bytes per edge instead
 * of 16.  GN_ERR_UNSUPPORTED for larger graphs. */
GN_API gn_status gn_negative_sampler_sample_packed(const gn_negative_sampler* sampler, uint64_t seed, int64_t* out_u,
                                            int64_t* out_v, uint32_t* packed_uv, int32_t* error_flag, void* stream);
/* The draw of a RECORDED training loop (a hipGraph replays its launch arguments): the seed of the draw is seed + *step, with
 * `step` a 64-bit counter in device memory (8-byte aligned, set by the caller once) that a one-thread launch behind the draw
 * advances by one.  Replay k of a captured call therefore writes what gn_negative_sampler_sample(_packed) writes for
 * seed + step0 + k: new negatives every epoch (GripNet-pose.py:131) without a launch outside the graph.  packed_uv may be
 * NULL.  Stepped draws of ONE sampler must not run concurrently (they share the sampler's arrival counter): one stream, or
 * one sampler per stream. */
GN_API gn_status gn_negative_sampler_sample_stepped(const gn_negative_sampler* sampler, uint64_t seed, uint64_t* step, int64_t* out_u,
                                             int64_t* out_v, uint32_t* packed_uv, int32_t* error_flag, void* stream);

/* ---------------------------------------------------------------------------------------
 * Filtered ranking and top-k partner retrieval for the DistMult decoder (link-prediction evaluation: filtered MRR / Hits@k).
 * A query is a row (u, r); its candidate scores are the logits s(v) = sum_k z[u,k] D[r,k] z[v,k] for every v in [0, n).
 *
 * gn_known_pairs: the union of one or more (u, v, relation) lists (train + test, typically), validated and sorted once on
 * the negative sampler's (relation, u * n + v) keys: a row of sorted partners per (relation, u), O(E + R * n) words.
 * Duplicates are allowed (set semantics).  Ids outside [0, n) / [0, R): GN_ERR_INDEX_RANGE.  Synchronises `stream`.
 * Holds n < 2^20, R < 2^23, R * n < 2^31 and E < 2^31 (GN_ERR_UNSUPPORTED beyond). */
typedef struct gn_known_pairs gn_known_pairs;
GN_API gn_status gn_known_pairs_create(const int64_t* u, const int64_t* v, const int64_t* edge_type, int64_t num_edges,
                                int64_t num_nodes, int64_t num_relations, void* stream, gn_known_pairs** known);
GN_API void gn_known_pairs_destroy(gn_known_pairs* known);
/* Per query e = (u[e], v[e], edge_type[e]): greater[e] / ties[e] = the candidates v' != v[e] whose (r, u, v') is not a
 * known pair (known may be NULL: no filter) with NOT (s(v') <= s(v[e])) / s(v') == s(v[e]).  The true score is the scan's
 * own value for column v[e] (same operands, same fp32 FMA order on the matrix cores).  No [Q, n] buffer, no float atomics,
 * no host synchronisation.  A query with an id out of range gets -1 / -1 and sets bit 0 of *error_flag.  num_features
 * <= 128; `known` must have been built for the same num_nodes and num_relations.
 * NON-FINITE SCORES never flatter the model.  greater[e] counts the admitted candidates c with NOT (s(c) <= s(true)),
 * ties[e] those with s(c) == s(true): a NaN true score puts every admitted candidate into `greater` (the true pair ranks
 * last, ties = 0), and a NaN candidate counts as greater than any true score.  -inf and +inf follow ordinary comparison:
 * equal infinities tie, a -inf candidate is greater than nothing.  "Admitted" is applied before the comparison (not the
 * true partner, not a known pair, inside the relation's range, < num_nodes): a known or out-of-range candidate never counts
 * whatever its score.  Non-finite scores set NO bit of *error_flag.  (The library is built without any fast-math option;
 * the rule depends on it.) */
GN_API gn_status gn_distmult_rank_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features, const float* d,
                               int64_t ld_d, int64_t num_relations, const int64_t* u, const int64_t* v, const int64_t* edge_type,
                               int64_t num_queries, const gn_known_pairs* known /* nullable */, int32_t* greater, int32_t* ties,
                               int32_t* error_flag, void* stream);
/* Per query e = (u[e], edge_type[e]): the k (1..64) best candidates that are not known pairs, by logit descending then id
 * ascending: scores[e * k + j] (fp32 logits) and ids[e * k + j]; padded with -inf / -1 when fewer than k candidates with a
 * score above -inf remain.  A NaN or -inf score never enters; +inf enters, and equal scores (equal infinities too) order by
 * ascending id.  A query whose whole candidate row is NaN (a NaN z[u], say) gets a full row of padding -inf / -1 and sets
 * no bit of *error_flag; a query with an id out of range gets NaN / -1 and sets bit 0 of *error_flag. */
GN_API gn_status gn_distmult_topk_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features, const float* d,
                               int64_t ld_d, int64_t num_relations, const int64_t* u, const int64_t* edge_type, int64_t num_queries,
                               int64_t k, const gn_known_pairs* known /* nullable */, float* scores, int64_t* ids,
                               int32_t* error_flag, void* stream);
/* Per-relation candidate ranges (type-constrained candidates: on a homogenised heterogeneous graph a relation's partners are
 * one node type, a contiguous id range).  cand_range: int64 [num_relations, 2] in device memory, row r = (lo_r, hi_r); a
 * candidate v' of a query of relation r is admitted iff lo_r <= v' < hi_r, on top of every rule above (not the true partner,
 * not a known pair, v' < num_nodes).  The table is per side, as `known` is.  The true partner may lie outside its
 * relation's range (it is never a candidate); greater / ties then count the admitted candidates.  An empty range
 * (lo == hi) is valid: 0 / 0, or a row of -inf / -1.  A row with lo < 0, hi > num_nodes or lo > hi is read on the device
 * (no host synchronisation) and makes its relation's queries queries with an id out of range: -1 / -1 or NaN / -1 and
 * bit 0 of *error_flag.  A workgroup scans the stages that hold a column of its queries' ranges only, so queries sorted by
 * relation are scanned against their own ranges; a score does not depend on where the scan starts, so the results are
 * those of the unranged call restricted to the range, bit for bit.  cand_range == NULL: the unranged call itself (which is
 * this call with NULL). */
GN_API gn_status gn_distmult_rank_ranged_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features, const float* d,
                               int64_t ld_d, int64_t num_relations, const int64_t* u, const int64_t* v, const int64_t* edge_type,
                               int64_t num_queries, const gn_known_pairs* known /* nullable */, int32_t* greater, int32_t* ties,
                               int32_t* error_flag, void* stream,
                               const int64_t* cand_range /* nullable, device, [num_relations, 2] */);
GN_API gn_status gn_distmult_topk_ranged_f32(const float* z, int64_t ld_z, int64_t num_nodes, int64_t num_features, const float* d,
                               int64_t ld_d, int64_t num_relations, const int64_t* u, const int64_t* edge_type, int64_t num_queries,
                               int64_t k, const gn_known_pairs* known /* nullable */, float* scores, int64_t* ids,
                               int32_t* error_flag, void* stream,
                               const int64_t* cand_range /* nullable, device, [num_relations, 2] */);

/* ---------------------------------------------------------------------------------------
 * Filtered ranking and top-k retrieval for the knowledge-graph-embedding scorers (GN_KGE_*; tables, gamma and
 * phase_divisor as for gn_kge_forward_f32, scores are the raw s, not their log-sigmoid).  A query is (fixed[e],
 * edge_type[e]) and a side: GN_KGE_SIDE_TAIL - fixed is the head, the candidates are the tails t' of (fixed, r, t');
 * GN_KGE_SIDE_HEAD - fixed is the tail, the candidates are the heads h' of (h', r, fixed).  `known` (nullable) filters the
 * candidates whose (relation, fixed, candidate) is a known pair: its rows are keyed (relation, fixed entity), so for the
 * head side it is built from the FLIPPED lists (u = tail, v = head).
 *   rank:  greater[e] / ties[e] = the non-known candidates c != truth[e] with NOT (s(c) <= s(truth[e])) / s(c) == s(truth[e]);
 *   top-k: the k (1..64) best non-known candidates, score descending then id ascending: scores[e * k + j], ids[e * k + j],
 *          padded with -inf / -1.
 * NON-FINITE SCORES never flatter the model (the rules of gn_distmult_rank_f32 / gn_distmult_topk_f32).  rank: greater[e] =
 * the admitted candidates c with NOT (s(c) <= s(true)), ties[e] = those with s(c) == s(true): a NaN true score puts every
 * admitted candidate into `greater` (the true triple ranks last, ties = 0), a NaN candidate counts as greater than any true
 * score; -inf and +inf follow ordinary comparison (equal infinities tie, a -inf candidate is greater than nothing).
 * "Admitted" (not the true partner, not a known pair, inside the relation's range, < num_entities) is applied before the
 * comparison: a known or out-of-range candidate never counts whatever its score.  top-k: a NaN or -inf score never enters,
 * +inf enters, equal scores order by ascending id; a query whose whole candidate row is NaN (a NaN fixed entity, say) gets
 * a full row of padding -inf / -1, not the NaN / -1 of an id out of range.  Non-finite scores set NO bit of *error_flag.
 * (TransE and RotatE score gamma - distance: never +inf.)
 * WHICH SCORE.  s is the value the scan computes, and with non-finite rows the formulation matters.  TransE, RotatE and
 * ComplEx on the tail side evaluate the forward's expression in the forward's order, DistMult a product of three factors
 * whose kind no order changes (0 * inf and inf - inf give NaN where they do in the forward).  ComplEx on the HEAD side folds the relation and the fixed tail into the query row first:
 *   s(h') = sum_k (rr tr + ri ti)_k hr'_k + (rr ti - ri tr)_k hi'_k,
 * the forward's Re((h' r) conj t) regrouped - the same number up to rounding on finite rows, but another KIND of value on a
 * non-finite one: a candidate head with hr'_k = +inf scores +-inf by the sign of (rr tr + ri ti)_k, where the forward gives
 * NaN as soon as one of rr, ri, tr, ti is zero in that column or the two products differ in sign.  The rules above hold for
 * this s (a NaN row still scores NaN; a row with an infinite entry may rank by its infinity instead of last).
 * A candidate's score depends on the query's and the candidate row's bits and a fixed column order only (equal rows tie),
 * and the true score is the scan's own value for that candidate.  DistMult and ComplEx run on the fp32 matrix cores (the
 * engine of gn_distmult_rank_f32, fed with query rows that a small launch prepares), TransE and RotatE on the vector ALU
 * with the arithmetic of the forward's terms.  No [Q, n] or [Q, n, D] buffer, no float atomics, no host synchronisation.
 * A query with an id out of range gets -1 / -1 (rank) or NaN / -1 (top-k) and sets bit 0 of *error_flag.  Entity rows of
 * at most 128 floats: hidden_dim <= 128 (TransE, DistMult), <= 64 (ComplEx, RotatE); GN_ERR_UNSUPPORTED beyond.  Scratch:
 * gn_kge_rank_workspace_bytes bytes, 16-byte aligned (RotatE: cos / sin of the relation table; DistMult, ComplEx: the
 * query rows [Q, De]; TransE: 0).  `known` must have been built for the same num_entities and num_relations. */
#define GN_KGE_SIDE_TAIL 0
#define GN_KGE_SIDE_HEAD 1
GN_API size_t gn_kge_rank_workspace_bytes(int model, int64_t num_relations, int64_t hidden_dim, int64_t num_queries);
GN_API gn_status gn_kge_rank_f32(int model, int side, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                          int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* fixed,
                          const int64_t* truth, const int64_t* edge_type, int64_t num_queries, float gamma,
                          float phase_divisor, const gn_known_pairs* known /* nullable */, int32_t* greater, int32_t* ties,
                          int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream);
GN_API gn_status gn_kge_topk_f32(int model, int side, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                          int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* fixed,
                          const int64_t* edge_type, int64_t num_queries, int64_t k, float gamma, float phase_divisor,
                          const gn_known_pairs* known /* nullable */, float* scores, int64_t* ids, int32_t* error_flag,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The same with per-relation candidate ranges: cand_range as for gn_distmult_rank_ranged_f32 (int64 [num_relations, 2] on
 * the device, row r = (lo_r, hi_r); candidate c admitted iff lo_r <= c < hi_r on top of the rules above; the valid tails
 * for GN_KGE_SIDE_TAIL, the valid heads for GN_KGE_SIDE_HEAD; empty range: 0 / 0 or padding; invalid row: its queries get
 * -1 / -1 or NaN / -1 and bit 0; NULL: the unranged call). */
GN_API gn_status gn_kge_rank_ranged_f32(int model, int side, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                          int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* fixed,
                          const int64_t* truth, const int64_t* edge_type, int64_t num_queries, float gamma,
                          float phase_divisor, const gn_known_pairs* known /* nullable */, int32_t* greater, int32_t* ties,
                          int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream,
                          const int64_t* cand_range /* nullable, device, [num_relations, 2] */);
GN_API gn_status gn_kge_topk_ranged_f32(int model, int side, const float* ent, int64_t ld_ent, int64_t num_entities, const float* rel,
                          int64_t ld_rel, int64_t num_relations, int64_t hidden_dim, const int64_t* fixed,
                          const int64_t* edge_type, int64_t num_queries, int64_t k, float gamma, float phase_divisor,
                          const gn_known_pairs* known /* nullable */, float* scores, int64_t* ids, int32_t* error_flag,
                          void* workspace, size_t workspace_bytes, void* stream,
                          const int64_t* cand_range /* nullable, device, [num_relations, 2] */);

/* The candidate block of a KGE mini-batch: cand[b * ld_cand + k] (int64, ld_cand >= K), K entities per positive
 * (fixed[b], edge_type[b]) drawn uniformly, with replacement, from the entities that are NOT partners of the row
 * (edge_type[b], fixed[b]) of `known` (nullable: no filter) - the filtered negatives of the code base KGEModel comes from,
 * for gn_kge_batch_forward_f32.  `known` is keyed as for gn_kge_rank_f32: (relation, head) for candidate tails, built from
 * the flipped lists for candidate heads; it must have been built for num_entities and num_relations (GN_ERR_INVALID_ARG).
 * THE DRAW IS PART OF THIS INTERFACE.  With mix64 the splitmix64 finaliser
 *   mix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31
 * (64-bit wrapping arithmetic), seed' = seed + *step when `step` (a device counter, 8-byte aligned, nullable) is given,
 * n = num_entities and element (b, k):
 *   base = mix64(seed' ^ ((uint64)(b * K + k) * 0xD6E8FEB86659FD93))
 *   attempt a = 0, 1, ...:   h = mix64(base + a);   c = (low32(h) * n) >> 32
 *   cand[b, k] = the first c that is not a partner of the row   (without `known`: attempt 0)
 * Membership is a binary search in the row's sorted partners (duplicates do no harm).  After 4,096 attempts - the typed
 * sampler's cap - the last draw is written and bit 1 of *error_flag (nullable) is set: the row knows (nearly) every
 * entity.  A fixed entity or relation outside its table writes -1 into the whole row and sets bit 0; nothing outside the
 * known pairs' row table is read, and the scorers turn such a row into NaN.  `step` is read, not advanced: the caller's
 * step += 1 is an ordinary launch of its own, so a captured mini-batch draws anew at every replay.  No host
 * synchronisation.  n < 2^31.  B == 0 or K == 0: nothing is written. */
GN_API gn_status gn_kge_candidates_sample(const int64_t* fixed, const int64_t* edge_type, int64_t num_positives,
                                   int64_t num_candidates, int64_t num_entities, int64_t num_relations,
                                   const gn_known_pairs* known /* nullable */, uint64_t seed,
                                   const uint64_t* step /* nullable, device */, int64_t* cand, int64_t ld_cand,
                                   int32_t* error_flag, void* stream);
/* The same draw from per-relation candidate ranges (cand_range as for gn_kge_rank_ranged_f32: int64 [num_relations, 2] on
 * the device, the valid tails or heads of each relation; num_relations is then the table's row count, also without
 * `known`).  THE RANGED DRAW IS PART OF THIS INTERFACE.  With (lo, hi) the row of edge_type[b] and m = hi - lo, base as above:
 *   attempt a = 0, 1, ...:   h = mix64(base + a);   c = lo + ((low32(h) * m) >> 32)
 *   cand[b, k] = the first c that is not a partner of the row
 * With (0, num_entities) this is the draw above, element for element, and so is cand_range == NULL.  An empty range
 * (lo == hi) writes -1 into the whole row and sets bit 1 of *error_flag (no entity to draw); a row with lo < 0,
 * hi > num_entities or lo > hi is read on the device and treated as an id out of range: a row of -1 and bit 0. */
GN_API gn_status gn_kge_candidates_sample_ranged(const int64_t* fixed, const int64_t* edge_type, int64_t num_positives,
                                   int64_t num_candidates, int64_t num_entities, int64_t num_relations,
                                   const gn_known_pairs* known /* nullable */, uint64_t seed,
                                   const uint64_t* step /* nullable, device */, int64_t* cand, int64_t ld_cand,
                                   int32_t* error_flag, void* stream,
                                   const int64_t* cand_range /* nullable, device, [num_relations, 2] */);

/* Independent small products in ONE launch.  Between gn_dense_batch_begin() and gn_dense_batch_end(stream) (per host thread,
 * not nested) the calls that carry GN_GEMM_JOIN_BATCH / GN_XTG_JOIN_BATCH - those of gn_gemm_f32 that take the deep-and-narrow kernel (a single product with at most 64 rows or 32 columns
 * of output and A given transposed or K >= 256) or the tall-skinny fp32 kernel (a single product of >= 256 rows whose B fits 64 KB
 * of LDS, no row gather; a product of >= 2048 rows with K a multiple of 32 takes the split-bf16 kernel instead and launches at once) and of gn_xtg_f32 that take the one-launch kernel are queued instead of launched,
 * and leave together at _end as one grid (up to four per launch; a product alone in its batch launches as usual); every other
 * call inside the bracket (without the flag, of another shape, or made by the library inside another entry point) launches at once.  The caller promises that the queued products neither depend on each other nor
 * share a workspace (a second gn_xtg_f32 on a queued workspace launches at once), and that their operands stay valid until
 * _end.  The dense products of the relational layer's backward (dbasis, datt, droot, dx += g root^T: layers.py:165-197 under
 * autograd) are four ~10 us launches, or one of 13 us; a GCN layer's dx and dW (layers.py:71-100) two, or one. */
GN_API gn_status gn_dense_batch_begin(void);
GN_API gn_status gn_dense_batch_end(void* stream);

/* The element-wise glue in front of a layer's backward pass, in one launch (autograd of layers.py:71-100,165-197 with the
 * ReLU of layers.py:279,305,370):  gm = saved_out > 0 ? g : 0 (saved_out NULL: gm = g);  gd = gm / rowdiv[row] (the mean
 * of the relational layer, layers.py:191);  colsum[c] = sum over the rows of gm[:, c] (the bias gradient).  gm, gd and
 * colsum are each optional (NULL).  Deterministic (fixed row slices, added in workgroup order by the last workgroup to
 * arrive).  `workspace` (needed for colsum): gn_grad_prologue_workspace_bytes() bytes, 4-byte aligned, ZEROED ONCE by the
 * caller; calls on one workspace must be stream-ordered.  Any width (one launch per block of 256 columns). */
GN_API size_t gn_grad_prologue_workspace_bytes(void);
GN_API gn_status gn_grad_prologue_f32(const float* g, int64_t ld_g, const float* saved_out, int64_t ld_saved, const float* rowdiv,
                               int64_t rows, int64_t cols, float* gm, int64_t ld_gm, float* gd, int64_t ld_gd, float* colsum,
                               void* workspace, size_t workspace_bytes, void* stream);

/* One Adam step over all parameter tensors in one launch (torch.optim.Adam(model.parameters(), lr) + optimizer.step(),
 * GripNet-pose.py:104,146; the update of torch/optim/adam.py without amsgrad / maximize):
 *   t = *step + 1;  g += weight_decay p;  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g g;
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);   *step = t.
 * `tensors` is a HOST array (copied into the launch's arguments, so a captured launch replays with it): device pointers
 * of parameter, gradient, first and second moment, and the element count.  `step`: one float on the device, the number of
 * steps taken so far (0 before the first), advanced by the launch.  `workspace`: 4 bytes on the device, 4-byte aligned,
 * ZEROED ONCE by the caller.  Calls on one (step, workspace) must be stream-ordered.  The betas are doubles (torch's are Python
 * floats): 1 - beta and the bias corrections 1 - beta^t are taken from them without the cancellation of an fp32 beta. */
#define GN_ADAM_MAX_TENSORS 64   /* per launch; longer tables take several launches */
typedef struct gn_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} gn_adam_tensor;
GN_API gn_status gn_adam_step_f32(const gn_adam_tensor* tensors, int num_tensors, float* step, void* workspace, size_t workspace_bytes,
                           float lr, double beta1, double beta2, float eps, float weight_decay, void* stream);

/* The link-prediction loss of the training loop and its gradient (GripNet-pose.py:140-142 with EPS of gripnet/utils.py:10):
 *   loss = - mean(log(pos + eps)) - mean(log(1 - neg + eps)),
 *   dpos[i] = - g / (num_pos (pos[i] + eps)),   dneg[i] = g / (num_neg (1 - neg[i] + eps)),   g = *upstream_grad (NULL: 1).
 * One launch each (written with torch ops: ~20 element-wise and reduction launches per step).  Deterministic: fixed
 * slices summed in a fixed order, partial sums added in workgroup order by the last workgroup to arrive.  `workspace`:
 * gn_link_loss_workspace_bytes() bytes, 8-byte aligned, ZEROED ONCE by the caller (the launch leaves it ready for the
 * next one); calls on one workspace must be stream-ordered. */
GN_API size_t gn_link_loss_workspace_bytes(void);
/* The node-classification loss of the NC training loops and its gradient (GripNet-aminer.py:133 and every freebase driver):
 *   loss = - mean_i log(score[i, classes[i]] + eps),   dscore[i, c] = c == classes[i] ? - g / (n (score[i, c] + eps)) : 0.
 * One launch each (the torch expression is an advanced-indexing gather, a log, a mean and their backward kernels).
 * A class id outside [0, num_classes) sets bit 0 of *error_flag (nullable) and contributes nothing. */
GN_API gn_status gn_class_loss_forward_f32(const float* score, int64_t ld_score, const int64_t* classes, int64_t num_nodes,
                                    int64_t num_classes, float eps, float* loss, int32_t* error_flag, void* stream);
GN_API gn_status gn_class_loss_backward_f32(const float* score, int64_t ld_score, const int64_t* classes, int64_t num_nodes,
                                     int64_t num_classes, float eps, const float* upstream_grad, float* dscore, int64_t ld_dscore,
                                     void* stream);
GN_API gn_status gn_link_loss_forward_f32(const float* pos_score, int64_t num_pos, const float* neg_score, int64_t num_neg, float eps,
                                   float* loss, void* workspace, size_t workspace_bytes, void* stream);
GN_API gn_status gn_link_loss_backward_f32(const float* pos_score, int64_t num_pos, const float* neg_score, int64_t num_neg, float eps,
                                    const float* upstream_grad /* device, nullable */, float* dpos, float* dneg, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-relation evaluation metrics (replaces the R scikit-learn calls and device -> host copies per epoch
 * of GripNet-pose.py:148-160,188-199 / gripnet/utils.py:28-35).  pos_score / neg_score hold E scores
 * each, segmented by the same range_list ([R,2] on the host).  out is [3, R] float64 on the device:
 * row 0 area under the precision-recall curve (trapezoid, with the point recall 0 / precision 1),
 * row 1 ROC AUC, row 2 average precision, per relation, with scikit-learn's treatment of tied scores;
 * NaN for a relation without edges.  Scores are compared as fp32 values: -0.0 and +0.0 tie, denormals stay distinct;
 * NaN and +-inf scores are the caller's to exclude (scikit-learn raises on them). */
typedef struct gn_link_metrics_plan gn_link_metrics_plan;
/* What depends on the range list only (the (relation, class) segments of the two score vectors, their chunk and tile maps):
 * built once per list (synchronises `stream` once); a planned call is asynchronous - chunk sort in LDS, merge rounds for the
 * relations longer than 4,096 edges, the curves' terms from binary searches between a relation's two sorted classes, a fold in
 * fixed order (bitwise reproducible).  workspace: gn_link_metrics_plan_workspace_bytes. */
GN_API gn_status gn_link_metrics_plan_create(const int64_t* range_list_host, int64_t num_relations, int64_t num_edges, void* stream,
                                      gn_link_metrics_plan** plan);
GN_API void gn_link_metrics_plan_destroy(gn_link_metrics_plan* plan);
GN_API size_t gn_link_metrics_plan_workspace_bytes(const gn_link_metrics_plan* plan);
GN_API gn_status gn_link_metrics_planned_f32(const gn_link_metrics_plan* plan, const float* pos_score, const float* neg_score,
                                      double* out, void* workspace, size_t workspace_bytes, void* stream);
/* The same without a kept plan (builds one, uses it, drops it: synchronises `stream`). */
GN_API size_t gn_link_metrics_workspace_bytes(int64_t num_relations, int64_t num_edges);
GN_API gn_status gn_link_metrics_f32(const float* pos_score, const float* neg_score, const int64_t* range_list_host,
                              int64_t num_relations, int64_t num_edges, double* out, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Node-classification metrics (replaces `pred = torch.argmax(score, dim=1)` and the device -> host copies and two
 * scikit-learn f1_score calls of micro_macro, gripnet/utils.py:38-52, twice per epoch of the node-classification drivers:
 * GripNet-aminer.py:130-137,153-156, GripNet-freebase-c.py:165-172,188-191).
 * Input: EXACTLY ONE of score (fp32 [n, num_class], row stride ld_score >= num_class, unit column stride, any alignment)
 * and pred_in (int64 [n] predicted class ids); classes: int64 [n] true class ids.  Outputs (device):
 *   pred_out  int64 [n] (score mode; nullable): torch.argmax(score, 1) - NaN above every number (the first NaN wins),
 *             otherwise the larger value, equal values (+0.0 == -0.0) by the lower index; an all -inf row gives 0;
 *   counts    int64 [3][num_class]: support (true count), predicted count, correct count (tp) per class;
 *   per_class float64 [3][num_class]: precision tp / predicted, recall tp / support, F1 2 tp / (support + predicted),
 *             each one division of exact integers, 0.0 where the denominator is 0 (scikit-learn's zero_division = 0);
 *   summary   float64 [3]: micro-F1 (= accuracy = sum tp / n), macro-F1 (the mean of F1 over the classes present in the
 *             labels or the predictions, summed in numpy's pairwise order: scikit-learn's bits), accuracy; n = 0 gives
 *             0.0, NaN, NaN as scikit-learn does.
 * A class id (or pred_in id) outside [0, num_class) ORs bit 3 (value 8) into *error_flag (nullable): every float64
 * output is then NaN and counts cover the rows whose ids are both in range.  Two launches, integer counts only (the same
 * bits every run), no host synchronisation, no allocation: graph-capturable.  workspace: at least
 * gn_class_metrics_workspace_bytes(n, num_class) bytes, 4-byte aligned, no initial contents.  1 <= num_class <= 1024
 * and n < 2^31, GN_ERR_UNSUPPORTED otherwise. */
GN_API size_t gn_class_metrics_workspace_bytes(int64_t n, int64_t num_class);
GN_API gn_status gn_class_metrics_f32(const float* score, int64_t ld_score, const int64_t* pred_in, const int64_t* classes,
                                      int64_t n, int64_t num_class, int64_t* pred_out, int64_t* counts, double* per_class,
                                      double* summary, int32_t* error_flag, void* workspace, size_t workspace_bytes,
                                      void* stream);

/* ---------------------------------------------------------------------------------------
 * One-shot direct exchange: the all-reduce of the sharded relational layer's partial sums ([n_d, 32] floats,
 * 82,560 B on PoSE: latency-bound) as ONE hop over xGMI's point-to-point links instead of a ring's 2 (G - 1): every rank
 * writes its partial into its slot of every peer's buffer (peer-mapped device memory: hipIpc handles exchanged by the caller),
 * raises a flag, waits for its own G flags on the device (bounded: timeout_ms, then bit 2 of *error_flag) and adds the G
 * slots in RANK ORDER - every rank holds the same bits.  Slot buffer per rank: gn_exchange_buffer_bytes(n, world) bytes
 * ([2][world][n] floats, slots alternate by step parity); flags: [world] int32, zero before step 1; ticket: one zeroed
 * uint32; step = 1, 2, 3, ... the same on every rank.  No host synchronisation. */
GN_API size_t gn_exchange_buffer_bytes(int64_t n, int world);
GN_API gn_status gn_exchange_push_f32(const float* src, int64_t n, void* const* peer_slots /* [world] device pointers, host array */,
                               void* const* peer_flags /* [world] */, unsigned int* ticket, int world, int rank, int step, void* stream);
GN_API gn_status gn_exchange_wait_sum_f32(const void* my_slots, const void* my_flags, int64_t n, int world, int step, float* dst,
                                   int timeout_ms, int32_t* error_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRIPNET_HIP_H */
