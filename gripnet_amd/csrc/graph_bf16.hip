// bf16 STORAGE of the gathered table for the GCN-style layers (BASELINE.json configs[4]).
// The reference has no reduced precision anywhere (fp32 throughout); this is the build's own definition:
// the table a layer gathers from - x W, rounded once to bf16 - is read at half the bytes, the sum over the
// neighbours, the bias and the activation stay fp32, and the layer's output is fp32 (the concat buffers, the
// decoders and every parameter are unchanged).  out = act( A_norm . bf16(xw) + b ).
#include "aggregate.cuh"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));       // round to nearest even, NaN stays NaN
}

// dst[i, c] = bf16(src[i, c]); cols % 8 == 0, 16-byte aligned rows on both sides
__global__ __launch_bounds__(256) void k_cast_bf16(const float* __restrict__ src, int64_t ld_src, uint16_t* __restrict__ dst,
                                                  int64_t ld_dst, int64_t rows, int cols8) {
    const int64_t total = rows * cols8;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / cols8;
        const int c = (int)(t - i * cols8) * 8;
        const float4 a = *reinterpret_cast<const float4*>(src + i * ld_src + c);
        const float4 b = *reinterpret_cast<const float4*>(src + i * ld_src + c + 4);
        *reinterpret_cast<u32x4*>(dst + i * ld_dst + c) =
            (u32x4){pack_bf16(a.x, a.y), pack_bf16(a.z, a.w), pack_bf16(b.x, b.y), pack_bf16(b.z, b.w)};
    }
}

}  // namespace

extern "C" {

gn_status gn_cast_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst, int64_t rows, int64_t cols, void* stream) {
    GN_REQUIRE(rows >= 0 && cols >= 0, "negative size");
    if (rows == 0 || cols == 0) return GN_OK;
    GN_REQUIRE(src && dst, "operand pointer is null");
    GN_REQUIRE(cols % 8 == 0 && ld_src % 4 == 0 && ld_dst % 8 == 0 && ld_src >= cols && ld_dst >= cols && gn::aligned16(src) &&
               gn::aligned16(dst), "gn_cast_bf16 needs cols %% 8 == 0 and 16-byte aligned rows");
    k_cast_bf16<<<gn::stream_grid(rows * (cols / 8), 256), 256, 0, gn::as_stream(stream)>>>(src, ld_src, dst, ld_dst, rows, (int)(cols / 8));
    GN_LAUNCH_CHECK();
    return GN_OK;
}

gn_status gn_graph_aggregate_bf16(const gn_graph_plan* plan, const uint16_t* table, int64_t ld_table, int64_t num_features,
                                  const float* bias, int relu, float* out, int64_t ld_out, const gn_side_copy* side, void* stream) {
    GN_REQUIRE(plan != nullptr, "plan is null");
    GN_REQUIRE(num_features >= 0 && num_features < (1ll << 31), "bad feature count");
    if (plan->rows == 0 || num_features == 0) return GN_OK;
    GN_REQUIRE(table && out, "feature pointers are null");
    GN_REQUIRE(num_features % 8 == 0 && ld_table % 8 == 0 && ld_out % 4 == 0 && ld_table >= num_features && ld_out >= num_features &&
               gn::aligned16(table) && gn::aligned16(out), "gn_graph_aggregate_bf16 needs features %% 8 == 0 and 16-byte aligned rows");
    gn::AggArgs a;
    a.rowptr = plan->rowptr.p; a.col = reinterpret_cast<const uint32_t*>(plan->col.p); a.coef = plan->coef.p;
    a.table = nullptr; a.table_bf16 = table; a.ld_table = ld_table; a.features = (int)num_features;
    a.rowdiv = nullptr; a.addend = nullptr; a.ld_addend = 0; a.bias = bias; a.relu = relu;
    a.out = out; a.ld_out = ld_out; a.rows = (int)plan->rows;
    gn_status ss = gn::check_side(side, plan->rows, &a.side);
    if (ss != GN_OK) return ss;
    // lane groups own rows or a wave per destination row (gather_route.hpp; aggregate.hip: k_aggregate_group / k_aggregate on
    // 16 bytes = 8 bf16 features per lane)
    gn::route::GatherCall c = gn::gather_call(a);
    c.nnz = plan->nnz;
    return gn::launch_gather(gn::route::gather_route(c), a, gn::as_stream(stream));
}

}  // extern "C"
