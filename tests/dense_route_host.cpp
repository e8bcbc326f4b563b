// The dense products' route (gripnet_amd/csrc/dense_route.hpp) as a stand-alone host program: reads one case per line from
// standard input and prints the route - kernel, tile, grid and LDS fields, or the refusal's status - one line per case.
// tests/test_dense_route.py builds it with g++ under AddressSanitizer + UBSan and holds the expected lines.
//
//   gemm m n k batch flags a_rows a_vec_ok c_offset addend disable_fast batch_open compute_units
//        (c_offset: bytes of c past a 16-byte boundary; the leading dimension of c is n, there is no bias)
//   xtg  m k1 k2 flags workspace_offset disable_fast batch_open compute_units
//   wide m k1 k2 disable_fast                                          (gn_xtg_wide_supported)
//
// A product that would be queued prints the fields of its entry in the batch's table, any other those of its own launch.
#include <cstdio>

#include "dense_route.hpp"

using namespace gn::route;

static void print_gemm(const GemmRoute& r) {
    switch (r.kernel) {
        case Gemm::refused: printf("refused %d\n", (int)r.status); break;
        case Gemm::general: printf("general grid=%u,%u,%u\n", r.grid_x, r.grid_y, r.grid_z); break;
        case Gemm::deep:
            if (r.queue) printf("deep queued mt=%d nt=%d gx=%d blocks=%d lds=%lld\n", r.mt, r.nt, r.gx, r.blocks, (long long)r.lds);
            else printf("deep mt=%d nt=%d grid=%u,%u\n", r.mt, r.nt, r.grid_x, r.grid_y);
            break;
        case Gemm::lds:
            if (r.queue) printf("lds queued row_tiles=%d gx=%d blocks=%d lds=%lld\n", r.row_tiles, r.gx, r.blocks, (long long)r.lds);
            else printf("lds row_tiles=%d grid=%u,%u lds=%lld\n", r.row_tiles, r.grid_x, r.grid_y, (long long)r.lds);
            break;
        case Gemm::split:
            printf("split terms=%d ct=%d slab=%d ch=%d row_tiles=%d grid=%u,%u lds=%lld bf16=%d\n", r.terms, r.ct, r.slab, r.ch, r.row_tiles,
                   r.grid_x, r.grid_y, (long long)r.lds, r.out_bf16 ? 1 : 0);
            break;
    }
}

static void print_xtg(const XtgRoute& r) {
    switch (r.kernel) {
        case Xtg::unsupported: printf("refused %d\n", (int)GN_ERR_UNSUPPORTED); break;
        case Xtg::wide: printf("wide ti=%d tj=%d wpt=%d slices=%d lds=%lld\n", r.ti, r.tj, r.wpt, r.slices, (long long)r.lds); break;
        case Xtg::mfma:
            if (r.queue) printf("mfma queued mt=%d nt=%d blocks=%d lds=%lld\n", r.mt, r.nt, r.slices, (long long)r.lds);
            else printf("mfma mt=%d nt=%d slices=%d lds=%lld\n", r.mt, r.nt, r.slices, (long long)r.lds);
            break;
        case Xtg::partial: printf("partial slices=%d lds=%lld\n", r.slices, (long long)r.lds); break;
    }
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        long long m, n, k, batch, k1, k2;
        int flags, a_rows, a_vec_ok, c_offset, addend, disabled, open, cus, ws_offset;
        if (sscanf(line, "gemm %lld %lld %lld %lld %d %d %d %d %d %d %d %d", &m, &n, &k, &batch, &flags, &a_rows, &a_vec_ok, &c_offset, &addend,
                   &disabled, &open, &cus) == 12) {
            GemmCall c;
            c.m = m; c.n = n; c.k = k; c.batch = batch; c.flags = flags;
            c.a_rows = a_rows != 0; c.a_vec_ok = a_vec_ok != 0; c.addend = addend != 0;
            c.bf16_vec_ok = n % 4 == 0 && c_offset % 8 == 0;
            c.fast_disabled = disabled != 0; c.join = open && (flags & GN_GEMM_JOIN_BATCH); c.compute_units = cus;
            print_gemm(gemm_route(c));
        } else if (sscanf(line, "xtg %lld %lld %lld %d %d %d %d %d", &m, &k1, &k2, &flags, &ws_offset, &disabled, &open, &cus) == 8) {
            XtgCall c;
            c.m = m; c.k1 = k1; c.k2 = k2; c.flags = flags; c.ws_aligned4 = ws_offset % 4 == 0;
            c.fast_disabled = disabled != 0; c.join = open && (flags & GN_XTG_JOIN_BATCH); c.compute_units = cus;
            print_xtg(xtg_route(c));
        } else if (sscanf(line, "wide %lld %lld %lld %d", &m, &k1, &k2, &disabled) == 4) {
            printf("wide_supported %d\n", xtg_wide(m, k1, k2, disabled != 0) ? 1 : 0);
        } else {
            printf("?\n");
        }
    }
    return 0;
}
