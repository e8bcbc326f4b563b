// Multi-relational internal layer (myRGCN, gripnet/layers.py:165-197): the entry points and queries, each validate -> route
// (rgcn_route.hpp decides the kernel, its template arguments and its workspace) -> one launch function per kernel, and the
// TABLE path.
//
// Kernels: destination-major in basis space for small supervertices (rgcn_pair.hip), LDS accumulator rows
// (rgcn_fast.hip), and for everything else the O(E)-memory basis-space path of rgcn_basis.hip (GN_RGCN_PATH_GENERAL).
// The table path below (GN_RGCN_PATH_TABLE) is the transform-then-gather ordering: W_r = att[r,:] .
// basis, H_r = X W_r for every relation (two MFMA GEMMs), then one destination-major gather-reduce over the [R*N, out]
// table with the global mean, the root term and the activation in the epilogue.  It works for any shape but needs
// R * N * out floats of workspace: kept for the shapes the basis-space path does not cover (> 64 bases, > 128 input
// features) and as an independent cross-check in the tests.
#include "aggregate.cuh"
#include "rgcn_route.hpp"

using gn::route::RelCall;
using gn::route::RelKernel;
using gn::route::RelKind;
using gn::route::RelRefusal;
using gn::route::RelRoute;

// rgcn_pair.hip, rgcn_fast.hip, rgcn_basis.hip: one launch function per kernel
gn_status gn_rgcn_pair_forward(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t fin, const float* basis,
                               const float* att, int64_t bases, const float* root, const float* bias, int64_t fout,
                               int relu, int partial, float* out, int64_t ld_out, const gn_side_copy& side, const void* x_planes,
                               const RelRoute& route, int basis_transposed, hipStream_t st);
gn_status gn_rgcn_fast_forward(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t fin,
                               const float* basis, const float* att, int64_t bases, const float* root,
                               const float* bias, int64_t fout, int relu, int partial, float* out,
                               int64_t ld_out, const gn_side_copy& side, void* ws, const RelRoute& route, hipStream_t st);
gn_status gn_rgcn_fast_finalize(const gn_rgcn_plan* plan, const float* summed, const float* x, int64_t ld_x, int64_t fin,
                                const float* root, const float* bias, int relu, float* out, int64_t ld_out,
                                const gn_side_copy& side, hipStream_t st);
gn_status gn_rgcn_basis_forward(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t fin, const float* basis,
                                const float* att, int64_t bases, const float* root, const float* bias, int64_t fout, int relu,
                                int partial, int sum, const float* edge_weight, float* out, int64_t ld_out, const gn_side_copy& side,
                                void* ws, const RelRoute& route, hipStream_t st);

namespace {

unsigned past16(const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15); }

// The facts of a call, for gn::route::rel_route.  What a query does not see stays at "aligned":
//   x      gn_rgcn_workspace_bytes, gn_rgcn_forward_path and the weighted queries pass none (x_known = false);
//   basis  no query sees it (null: aligned).  A forward whose basis is not 16-byte aligned leaves the destination-major kernel
//          for the next one of the ladder, needs THAT kernel's scratch, and is refused with that size if it got less - whatever
//          the query said for an aligned basis (torch allocations are).
// A query keeps the flags that choose a kernel; which flags a forward refuses is the forward's to say.
RelCall rel_call(RelKind kind, const gn_rgcn_plan* plan, int64_t fin, int64_t fout, int64_t bases, int flags, const float* x = nullptr,
                 int64_t ld_x = 0, const void* basis = nullptr) {
    RelCall c{};
    c.kind = kind;
    c.num_nodes = plan->num_nodes; c.num_relations = plan->num_relations; c.shard_edges = plan->shard_edges;
    c.pair_ok = plan->pair_ok != 0; c.fast_ok = plan->fast_ok != 0; c.fast_groups = plan->fast_groups;
    c.row_order = plan->row_order.p != nullptr;
    c.fin = fin; c.fout = fout; c.bases = bases; c.flags = flags;
    c.x_known = x != nullptr; c.ld_x = ld_x; c.x_at = past16(x); c.basis_at = past16(basis);
    c.fast_disabled = gn::fast_paths_disabled();
    c.slab_bytes = gn_layout::kSlabBytes;
    if (const char* e = getenv("GN_RGCN_SLAB_MB")) {                       // test hook: small slabs (the same bits: a slab is a range of rows)
        const long mb = atol(e);
        if (mb >= 1 && mb <= 4096) c.slab_bytes = (int64_t)mb << 20;
    }
    return c;
}

constexpr int kQueryFlags = GN_RGCN_SUM | GN_RGCN_ARITH_FAST | (7 << GN_RGCN_PATH_SHIFT);

// The kernel's GN_RGCN_PATH_* code: what the queries answer
int path_code(RelKernel k) {
    return k == RelKernel::pair ? GN_RGCN_PATH_PAIR : k == RelKernel::lds ? GN_RGCN_PATH_LDS : k == RelKernel::general ? GN_RGCN_PATH_GENERAL : GN_RGCN_PATH_TABLE;
}

gn_status refuse(const RelRoute& route, int flags) {
    switch (route.why) {
        case RelRefusal::undefined_flags: return gn::fail(route.status, "flags 0x%x: bits this entry point does not define", flags);
        case RelRefusal::sum_with_partial: return gn::fail(route.status, "GN_RGCN_SUM and GN_RGCN_PARTIAL exclude each other");
        case RelRefusal::weighted_flags: return gn::fail(route.status, "flags 0x%x: a weighted call is GN_RGCN_SUM or GN_RGCN_PARTIAL", flags);
        case RelRefusal::basis_transposed:
            return gn::fail(route.status, "GN_RGCN_BASIS_TRANSPOSED: only the destination-major kernel reads a transposed basis (pass a transposed copy)");
        default: return gn::fail(route.status, "the weighted relational layer covers up to 64 bases and 128 input features");
    }
}

// The table kernel: W_r for every relation, H[r] = X W_r, then one gather-reduce over the [R * N, out] table
gn_status table_forward(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t fin, const float* basis, const float* att,
                        int64_t bases, const float* root, const float* bias, int64_t fout, int relu, int partial, int sum, float* out,
                        int64_t ld_out, const gn_side_copy& side, void* workspace, const RelRoute& l, hipStream_t st) {
    const int64_t N = plan->num_nodes, R = plan->num_relations;
    char* ws = static_cast<char*>(workspace);
    float* W = reinterpret_cast<float*>(ws + l.w_off);
    float* H = reinterpret_cast<float*>(ws + l.h_off);
    float* XR = reinterpret_cast<float*>(ws + l.xr_off);
    if (R > 0) {
        // K7: W[R, fin*fout] = att[R,B] @ basis[B, fin*fout]   (layers.py:172-173)
        GN_OK_OR_RETURN(gn_gemm_f32(att, bases, 0, nullptr, 0, basis, fin * fout, 0, W, fin * fout, 0, R, fin * fout, bases, 1, nullptr, 0, st));
        // H[r] = X @ W[r] for all relations; grid.z carries the relation, in slabs of 32768
        for (int64_t r0 = 0; r0 < R; r0 += 32768) {
            const int64_t nb = std::min<int64_t>(32768, R - r0);
            GN_OK_OR_RETURN(gn_gemm_f32(x, ld_x, 0, nullptr, 0, W + r0 * fin * fout, fout, fin * fout, H + r0 * N * fout, fout,
                                        N * fout, N, fout, fin, nb, nullptr, 0, st));
        }
    }
    const bool with_root = !partial && root != nullptr;
    if (with_root)   // K12: x @ root (+ bias) goes in as the addend of the gather epilogue (layers.py:193-196)
        GN_OK_OR_RETURN(gn_gemm_f32(x, ld_x, 0, nullptr, 0, root, fout, 0, XR, fout, 0, N, fout, fin, 1, bias, 0, st));
    gn::AggArgs a;
    a.rowptr = plan->rowptr.p;
    a.col = plan->key.p;
    a.coef = nullptr;
    a.table = H;
    a.ld_table = fout;
    a.features = (int)fout;
    a.rowdiv = (partial || sum) ? nullptr : plan->indeg.p;
    a.addend = with_root ? XR : nullptr;
    a.ld_addend = fout;
    a.bias = (!partial && !with_root) ? bias : nullptr;    // (the sum without a root term: the bias rides in the gather's epilogue)
    a.relu = partial ? 0 : relu;
    a.out = out;
    a.ld_out = ld_out;
    a.rows = (int)N;
    a.side = side;
    return gn::launch_aggregate(a, st);
}

__global__ void k_rgcn_finalize(const float* __restrict__ summed, int64_t ld_s, const float* __restrict__ indeg,
                                int relu, float* __restrict__ out, int64_t ld_o, int64_t rows, int cols,
                                gn_side_copy side) {
    // concat slot 0
    gn::side_copy_stream(side, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
    const int64_t total = rows * cols;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / cols;
        const int c = (int)(t - i * cols);
        float v = summed[i * ld_s + c] / fmaxf(indeg[i], 1.0f) + out[i * ld_o + c];   // out holds x.root + bias
        if (relu) v = gn::relu_keep_nan(v);
        out[i * ld_o + c] = v;
    }
}

}  // namespace

extern "C" {

// The queries answer for the kernel a forward with these flags takes on aligned operands (rel_call), and never refuse.
size_t gn_rgcn_workspace_bytes(const gn_rgcn_plan* plan, int64_t fin, int64_t fout, int64_t bases, int flags) {
    if (!plan || fin <= 0 || fout <= 0 || bases <= 0) return 0;
    return rel_route(rel_call(RelKind::forward, plan, fin, fout, bases, flags & kQueryFlags)).workspace;
}

int gn_rgcn_forward_path(const gn_rgcn_plan* plan, int64_t fin, int64_t fout, int64_t bases, int flags) {
    if (!plan || fin <= 0 || fout <= 0 || bases <= 0) return -1;
    return path_code(rel_route(rel_call(RelKind::forward, plan, fin, fout, bases, flags & kQueryFlags)).kernel);
}

int gn_rgcn_forward_choice(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t fin, int64_t fout, int64_t bases,
                           int flags, size_t* workspace_bytes) {
    if (workspace_bytes) *workspace_bytes = 0;
    if (!plan || fin <= 0 || fout <= 0 || bases <= 0) return -1;
    const RelRoute route = rel_route(rel_call(RelKind::forward, plan, fin, fout, bases, flags & kQueryFlags, x, ld_x));
    if (workspace_bytes) *workspace_bytes = route.workspace;
    return path_code(route.kernel);
}

gn_status gn_rgcn_forward_f32(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t fin,
                              const float* basis, const float* att, int64_t bases, const float* root,
                              const float* bias, int64_t fout, int relu, int flags, float* out, int64_t ld_out,
                              const gn_side_copy* side, const void* x_planes, void* workspace, size_t workspace_bytes,
                              void* stream) {
    const int partial = flags & GN_RGCN_PARTIAL, sum = (flags & GN_RGCN_SUM) ? 1 : 0;
    GN_REQUIRE(plan != nullptr, "plan is null");
    GN_REQUIRE(fin > 0 && fout > 0 && bases > 0, "feature / basis counts must be positive");
    // the kernel THIS call takes, on its own x and basis, with its own scratch (a forced general or table path, or a basis
    // pointer the destination-major kernel cannot use, needs its own whatever gn_rgcn_workspace_bytes said for the default choice)
    const RelRoute route = rel_route(rel_call(RelKind::forward, plan, fin, fout, bases, flags, x, ld_x, basis));
    if (route.status == GN_ERR_INVALID_ARG) return refuse(route, flags);       // its flags are refused before anything looks at its operands,
    GN_REQUIRE(!sum || !side || !side->dst, "GN_RGCN_SUM takes no side copy");
    const int64_t N = plan->num_nodes;
    if (N == 0) return GN_OK;
    GN_REQUIRE(x && basis && att && out && (partial || sum || root), "operand pointer is null");
    GN_REQUIRE(ld_x >= fin && ld_out >= fout, "leading dimension smaller than the row length");
    if (route.kernel == RelKernel::refused) return refuse(route, flags);       // its kernel after them
    GN_REQUIRE(route.workspace == 0 || (workspace && workspace_bytes >= route.workspace), "workspace too small: this call needs %zu bytes, got %zu",
               route.workspace, workspace_bytes);
    hipStream_t st = gn::as_stream(stream);
    gn_side_copy sc;
    gn_status ss = gn::check_side(side, N, &sc);
    if (ss != GN_OK) return ss;
    switch (route.kernel) {
        case RelKernel::pair:
            return gn_rgcn_pair_forward(plan, x, ld_x, fin, basis, att, bases, root, bias, fout, relu, partial, out, ld_out, sc, x_planes, route,
                                        flags & GN_RGCN_BASIS_TRANSPOSED, st);
        case RelKernel::lds:
            return gn_rgcn_fast_forward(plan, x, ld_x, fin, basis, att, bases, root, bias, fout, relu, partial, out, ld_out, sc, workspace, route, st);
        case RelKernel::general:
            return gn_rgcn_basis_forward(plan, x, ld_x, fin, basis, att, bases, root, bias, fout, relu, partial, sum, nullptr, out, ld_out, sc,
                                         workspace, route, st);
        default:
            return table_forward(plan, x, ld_x, fin, basis, att, bases, root, bias, fout, relu, partial, sum, out, ld_out, sc, workspace, route, st);
    }
}

int gn_rgcn_weighted_supported(const gn_rgcn_plan* plan, int64_t fin, int64_t fout, int64_t bases) {
    if (!plan) return 0;
    return rel_route(rel_call(RelKind::weighted, plan, fin, fout, bases, GN_RGCN_SUM)).kernel == RelKernel::general ? 1 : 0;
}

size_t gn_rgcn_weighted_workspace_bytes(const gn_rgcn_plan* plan, int64_t fin, int64_t fout, int64_t bases) {
    if (!plan) return 0;
    return rel_route(rel_call(RelKind::weighted, plan, fin, fout, bases, GN_RGCN_SUM)).workspace;      // (refused: 0)
}

gn_status gn_rgcn_forward_weighted_f32(const gn_rgcn_plan* plan, const float* x, int64_t ld_x, int64_t fin, const float* basis,
                                       const float* att, int64_t bases, const float* root, const float* bias, int64_t fout,
                                       int relu, int flags, const float* edge_weight, float* out, int64_t ld_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    GN_REQUIRE(plan != nullptr, "plan is null");
    GN_REQUIRE(fin > 0 && fout > 0 && bases > 0, "feature / basis counts must be positive");
    const RelRoute route = rel_route(rel_call(RelKind::weighted, plan, fin, fout, bases, flags, x, ld_x, basis));
    if (route.kernel == RelKernel::refused) return refuse(route, flags);
    if (plan->num_nodes == 0) return GN_OK;
    GN_REQUIRE(x && basis && att && out, "operand pointer is null");
    GN_REQUIRE(edge_weight || plan->shard_edges == 0, "edge_weight is null");
    GN_REQUIRE(plan->has_pos || plan->shard_edges == 0, "the plan has no position list: call gn_rgcn_plan_build_positions first");
    GN_REQUIRE(ld_x >= fin && ld_out >= fout, "leading dimension smaller than the row length");
    GN_REQUIRE(workspace && workspace_bytes >= route.workspace, "workspace too small: this call needs %zu bytes, got %zu", route.workspace,
               workspace_bytes);
    const int partial = flags & GN_RGCN_PARTIAL;
    return gn_rgcn_basis_forward(plan, x, ld_x, fin, basis, att, bases, root, bias, fout, relu, partial, partial ? 0 : 1, edge_weight, out, ld_out,
                                 gn_side_copy{nullptr, 0, nullptr, 0, 0, 0, 0}, workspace, route, gn::as_stream(stream));
}

gn_status gn_rgcn_finalize_f32(const gn_rgcn_plan* plan, const float* summed, int64_t ld_summed, const float* x,
                               int64_t ld_x, int64_t fin, const float* root, const float* bias, int64_t fout,
                               int relu, float* out, int64_t ld_out, const gn_side_copy* side, void* stream) {
    GN_REQUIRE(plan != nullptr, "plan is null");
    GN_REQUIRE(fin > 0 && fout > 0 && fout < (1ll << 31), "feature counts must be positive");
    const int64_t N = plan->num_nodes;
    if (N == 0) return GN_OK;
    GN_REQUIRE(summed && x && root && out, "operand pointer is null");
    GN_REQUIRE(summed != out, "finalize cannot run in place");
    gn_side_copy sc;
    gn_status ss = gn::check_side(side, N, &sc);
    if (ss != GN_OK) return ss;
    RelCall c = rel_call(RelKind::finalize, plan, fin, fout, 0, 0);
    c.ld_summed = ld_summed; c.summed_at = past16(summed);
    switch (rel_route(c).kernel) {
        case RelKernel::slab_finalize:
            return gn_rgcn_fast_finalize(plan, summed, x, ld_x, fin, root, bias, relu, out, ld_out, sc, gn::as_stream(stream));
        default: {
            GN_OK_OR_RETURN(gn_gemm_f32(x, ld_x, 0, nullptr, 0, root, fout, 0, out, ld_out, 0, N, fout, fin, 1, bias, 0, stream));
            k_rgcn_finalize<<<gn::stream_grid(N * fout, 256), 256, 0, gn::as_stream(stream)>>>(
                summed, ld_summed, plan->indeg.p, relu, out, ld_out, N, (int)fout, sc);
            GN_LAUNCH_CHECK();
            return GN_OK;
        }
    }
}

}  // extern "C"
