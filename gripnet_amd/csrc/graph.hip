// GCN-style aggregation over a cached plan (square graphs with self loops, or the bipartite
// external layer).  Replaces propagate/message/update of myGCN (gripnet/layers.py:92-100).
#include "aggregate.cuh"

// gcn_blocked.hip: the LDS-staged, source-blocked path
gn_status gn_blocked_aggregate(const gn_graph_plan* plan, const float* x, int64_t ld_x, int64_t fin, const float* w,
                               int64_t fout, const float* bias, int relu, float* out, int64_t ld_out,
                               const gn_side_copy& side, hipStream_t st);

namespace {

using gn::route::Gather;
using gn::route::GatherCall;
using gn::route::GatherRefusal;
using gn::route::GatherRoute;
using gn::route::Source;

// what a forward entry point gathers: one table, or (split) a row kept in two - head_cols columns of `table`, the rest in `tail`
struct GatherSource {
    const float* table; int64_t ld_table;
    bool split; int64_t head_cols; const float* tail; int64_t ld_tail;
};

GatherCall split_call(const float* head, int64_t ld_head, int64_t head_cols, const float* tail, int64_t ld_tail,
                      int64_t num_features, int64_t out_features) {
    GatherCall c{};
    c.kind = Source::split;
    c.features = num_features; c.fout = out_features; c.weight = true;
    c.head = head != nullptr; c.tail = tail != nullptr; c.head_cols = head_cols;
    c.ld_table = ld_head; c.ld_tail = ld_tail; c.table_at = gn::past16(head); c.tail_at = gn::past16(tail);
    c.fast_disabled = gn::fast_paths_disabled();
    return c;
}

gn_status refuse(const GatherRoute& r, const GatherCall& c) {
    const long long fin = c.features, fout = c.fout, head = c.head_cols;
    const char* why = "";
    switch (r.why) {
        case GatherRefusal::none: return GN_OK;
        case GatherRefusal::no_fused_transform:
            return gn::fail(r.status, "no fused transform for %lld -> %lld features (or unaligned rows)", fin, fout);
        case GatherRefusal::tail_operands:
            return gn::fail(r.status, "the deferred tail transform exists for 64 -> 16 features over 16-byte aligned rows on the "
                                      "wave-per-row kernel, got %lld -> %lld", fin, fout);
        case GatherRefusal::split_fast_off: why = "the wave-per-row transform kernel is switched off (GN_DISABLE_FAST)"; break;
        case GatherRefusal::split_widths: why = "the split source exists for 64 -> 16 features"; break;
        case GatherRefusal::split_head_cols: why = "head_cols must be 16, 32 or 48"; break;
        case GatherRefusal::split_alignment: why = "both tables must be 16-byte aligned"; break;
        case GatherRefusal::split_ld_multiple: why = "both leading dimensions must be multiples of 4"; break;
        case GatherRefusal::split_ld_short: why = "a leading dimension is smaller than its table's row"; break;
        case GatherRefusal::split_ld_31_bits: why = "a leading dimension does not fit 31 bits"; break;
    }
    return gn::fail(r.status, "split source, %lld -> %lld features, head %lld: %s", fin, fout, head, why);
}

gn_status check_planes(const gn_split_planes* planes, const gn_graph_plan* plan, int64_t width, const gn_side_copy& side) {
    if (planes && planes->planes) {
        GN_REQUIRE(planes->nt >= 1 && planes->nt <= 4 && planes->rows >= plan->rows && planes->col_main >= 0 &&
                       planes->col_main + width <= 16 * planes->nt &&
                       (!side.dst || (planes->col_side >= 0 && planes->col_side + side.cols <= 16 * planes->nt)),
                   "split planes do not hold the launch's columns");
    }
    return GN_OK;
}

// The one body of the three forward entry points: checks, the route, the launch, and the stand-alone split of what a kernel
// that does not write the offered planes itself has written.  `tail`: the deferred 16 -> 16 transform of columns 48..63.
// The tail and split entries refuse what they do not cover before they look at an empty plan, the side copy or the planes;
// the plain entry returns from an empty call first and refuses last (preserves the parent's order, and so every status).
gn_status graph_forward(const gn_graph_plan* plan, const GatherSource& src, int64_t num_features, const float* weight,
                        int64_t out_features, const float* bias, int relu, float* out, int64_t ld_out, const gn_side_copy* side,
                        const gn_split_planes* planes, const gn::AggTail* tail, void* stream) {
    GN_REQUIRE(plan != nullptr, "plan is null");
    const bool plain = !tail && !src.split;
    if (plain) {
        GN_REQUIRE(num_features >= 0 && num_features < (1ll << 31), "bad feature count");
        if (plan->rows == 0 || num_features == 0) return GN_OK;
    }
    GN_REQUIRE(out && (src.split || src.table) && (plain || weight) && (!tail || tail->w), "a feature, weight or output pointer is null");
    const int64_t width = weight ? out_features : num_features;
    if (!src.split) GN_REQUIRE(src.ld_table >= num_features && ld_out >= width, "leading dimension smaller than the row length");

    gn::AggArgs a = gn::forward_args(plan, src.table, src.ld_table, num_features, bias, relu, out, ld_out);
    GatherCall c;
    if (src.split) {
        c = split_call(src.table, src.ld_table, src.head_cols, src.tail, src.ld_tail, num_features, out_features);
        c.rows = plan->rows;
    } else {
        c = gn::forward_call(plan, a, weight, width);
        if (tail) { c.kind = Source::tail; c.tail_w_at = gn::past16(tail->w); c.tail_b_at = gn::past16(tail->b); }
    }
    const bool offered = planes && planes->planes;
    c.planes = offered;
    const GatherRoute r = gn::route::gather_route(c);
    if (!plain) {
        if (r.kernel == Gather::refused) return refuse(r, c);
        if (src.split) GN_REQUIRE(ld_out >= width, "leading dimension smaller than the row length");
        if (plan->rows == 0) return GN_OK;
    }
    gn_status s = gn::check_side(side, plan->rows, &a.side);
    if (s != GN_OK) return s;
    s = check_planes(planes, plan, width, a.side);
    if (s != GN_OK) return s;
    if (r.kernel == Gather::refused) return refuse(r, c);

    hipStream_t st = gn::as_stream(stream);
    if (r.planes_by_kernel) a.split = *planes;
    if (r.kernel == Gather::blocked) {
        s = gn_blocked_aggregate(plan, src.table, src.ld_table, num_features, weight, width, bias, relu, out, ld_out, a.side, st);
    } else {
        const gn::AggSplit split = {src.tail, (uint32_t)src.ld_tail, (int)src.head_cols};
        s = gn::launch_gather(r, a, st, weight, (int)out_features, tail, &split);
    }
    if (s != GN_OK || !offered || r.planes_by_kernel) return s;
    s = gn_split_planes_f32(out, ld_out, plan->rows, width, planes->col_main, planes, stream);
    if (s == GN_OK && a.side.dst)
        s = gn_split_planes_f32(a.side.dst, a.side.ld_dst, a.side.rows, a.side.cols, planes->col_side, planes, stream);
    return s;
}

}  // namespace

extern "C" gn_status gn_graph_aggregate_f32(const gn_graph_plan* plan, const float* xw, int64_t ld_xw,
                                            int64_t num_features, const float* weight, int64_t out_features,
                                            const float* bias, int relu, float* out, int64_t ld_out,
                                            const gn_side_copy* side, const gn_split_planes* planes, void* stream) {
    return graph_forward(plan, GatherSource{xw, ld_xw, false, 0, nullptr, 0}, num_features, weight, out_features, bias, relu, out, ld_out,
                         side, planes, nullptr, stream);
}

// act( (A_norm x') weight + bias ), x' = x with its columns 48..63 replaced row by row by act2(x[:, 48:64] tail_w + tail_b):
// the external layer reading a gene concat whose last layer left A_norm h there and its 16 -> 16 transform to this launch
extern "C" gn_status gn_graph_aggregate_tail_f32(const gn_graph_plan* plan, const float* x, int64_t ld_x, int64_t num_features,
                                                 const float* weight, int64_t out_features, const float* bias, int relu,
                                                 float* out, int64_t ld_out, const gn_side_copy* side,
                                                 const gn_split_planes* planes, const float* tail_w, const float* tail_b,
                                                 int tail_relu, void* stream) {
    const gn::AggTail tail = {tail_w, tail_b, tail_relu};
    return graph_forward(plan, GatherSource{x, ld_x, false, 0, nullptr, 0}, num_features, weight, out_features, bias, relu, out, ld_out,
                         side, planes, &tail, stream);
}

// act( (A_norm [head | tail]) weight + bias ) without the concatenation: row `col` of the gathered table is row `col` of `head`
// (head_cols columns) followed by row `col` of `tail` - the external layer reading the gene embedding where it lies
extern "C" gn_status gn_graph_aggregate_split_f32(const gn_graph_plan* plan, const float* head, int64_t ld_head, int64_t head_cols,
                                                  const float* tail, int64_t ld_tail, int64_t num_features, const float* weight,
                                                  int64_t out_features, const float* bias, int relu, float* out, int64_t ld_out,
                                                  const gn_side_copy* side, const gn_split_planes* planes, void* stream) {
    return graph_forward(plan, GatherSource{head, ld_head, true, head_cols, tail, ld_tail}, num_features, weight, out_features, bias, relu,
                         out, ld_out, side, planes, nullptr, stream);
}

extern "C" int gn_graph_split_applicable(const gn_graph_plan* plan, const float* head, int64_t ld_head, int64_t head_cols,
                                         const float* tail, int64_t ld_tail, int64_t num_features, int64_t out_features) {
    return plan && gn::route::gather_route(split_call(head, ld_head, head_cols, tail, ld_tail, num_features, out_features)).kernel ==
                       Gather::transform_split ? 1 : 0;
}

extern "C" size_t gn_split_planes_bytes(int64_t rows, int nt) {
    if (rows < 0 || nt < 1) return 0;
    return (size_t)(rows + 1) * 64 * (size_t)((3 * nt + 1) / 2);
}

extern "C" gn_status gn_split_planes_f32(const float* src, int64_t ld_src, int64_t rows, int64_t cols, int64_t col0,
                                         const gn_split_planes* planes, void* stream) {
    GN_REQUIRE(planes && planes->planes, "planes are null");
    GN_REQUIRE(planes->nt >= 1 && planes->nt <= 4 && rows >= 0 && rows <= planes->rows && cols >= 0 && col0 >= 0 &&
                   col0 + cols <= 16 * planes->nt, "split planes do not hold these columns");
    if (rows == 0 || cols == 0) return GN_OK;
    GN_REQUIRE(src && ld_src >= cols, "source matrix is null or its leading dimension too small");
    return gn::launch_split_planes(src, ld_src, rows, (int)cols, (int)col0, *planes, gn::as_stream(stream));
}

// Backward of the aggregation with respect to its table: gxw[s, :] = sum_{e: src(e)=s} coef_e * g[dst(e), :]
// (the transpose of the normalised adjacency applied to the output gradient).
extern "C" gn_status gn_graph_aggregate_t_f32(const gn_graph_plan* plan, const float* g, int64_t ld_g,
                                              int64_t num_features, float* out, int64_t ld_out, void* stream) {
    GN_REQUIRE(plan != nullptr, "plan is null");
    GN_REQUIRE(plan->has_transpose, "call gn_graph_plan_build_transpose first");
    GN_REQUIRE(num_features >= 0 && num_features < (1ll << 31), "bad feature count");
    if (plan->table_rows == 0 || num_features == 0) return GN_OK;
    GN_REQUIRE(g && out, "feature pointers are null");
    GN_REQUIRE(ld_g >= num_features && ld_out >= num_features, "leading dimension smaller than the row length");
    gn::AggArgs a;
    a.rowptr = plan->t_rowptr.p;
    a.col = reinterpret_cast<const uint32_t*>(plan->t_col.p);
    a.coef = plan->t_coef.p;
    a.table = g;
    a.ld_table = ld_g;
    a.features = (int)num_features;
    a.rowdiv = nullptr;
    a.addend = nullptr;
    a.ld_addend = 0;
    a.bias = nullptr;
    a.relu = 0;
    a.out = out;
    a.ld_out = ld_out;
    a.rows = (int)plan->table_rows;
    a.nnz = plan->nnz;
    return gn::launch_aggregate(a, gn::as_stream(stream));
}

extern "C" int gn_transform_fusable(int64_t in_features, int64_t out_features) {
    return gn::route::transform_fusable(in_features, out_features, gn::fast_paths_disabled()) ? 1 : 0;
}

extern "C" int gn_graph_transform_fusable(const gn_graph_plan* plan, int64_t in_features, int64_t out_features) {
    if (!plan) return 0;
    const bool off = gn::fast_paths_disabled();
    return (gn::route::transform_fusable(in_features, out_features, off) ||
            gn::route::mfma_fusable(in_features, out_features, plan->rows, plan->nnz, off)) ? 1 : 0;
}
