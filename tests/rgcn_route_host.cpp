// The relational forward's route (gripnet_amd/csrc/rgcn_route.hpp) as a stand-alone host program: reads one case per line from
// standard input and prints the route - kernel, template arguments, workspace bytes and layout - or the refusal's status and
// reason, one line per case.  tests/test_rgcn_route.py builds it with g++ under AddressSanitizer + UBSan and holds the
// expected lines.
//
// A case is a request kind and key=value pairs; what a line leaves out keeps its default:
//
//   forward | weighted | finalize     gn_rgcn_forward_f32, gn_rgcn_forward_weighted_f32, gn_rgcn_finalize_f32
//
//   nodes=645 rels=100 edges=10000 pair_ok=1 fast_ok=1 groups=256 row_order=1     the plan
//   fin=48 fout=32 bases=32                                                       widths
//   partial fast transposed sum = 0, force=0 (a GN_RGCN_PATH_* code), bits=0      flags: the named ones, a forced kernel, raw bits
//   x_known=1 ld_x=fin x_at=0 basis_at=0                                          x (0: a query without x), bytes past a 16-byte boundary
//   ld_summed=fout summed_at=0                                                    finalize
//   fast_off=0 slab_mb=256                                                        GN_DISABLE_FAST, GN_RGCN_SLAB_MB
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "rgcn_route.hpp"

using namespace gn::route;

struct Case {
    std::string kind;
    std::map<std::string, long long> v;
    long long get(const char* key, long long dflt) const {
        auto it = v.find(key);
        return it == v.end() ? dflt : it->second;
    }
};

static bool parse(char* line, Case& c) {
    char* tok = strtok(line, " \t\n");
    if (!tok) return false;
    c.kind = tok;
    while ((tok = strtok(nullptr, " \t\n")) != nullptr) {
        char* eq = strchr(tok, '=');
        if (!eq) return false;
        c.v[std::string(tok, eq - tok)] = atoll(eq + 1);
    }
    return true;
}

static RelCall call_of(const Case& k) {
    RelCall c{};
    c.kind = k.kind == "weighted" ? RelKind::weighted : k.kind == "finalize" ? RelKind::finalize : RelKind::forward;
    c.num_nodes = k.get("nodes", 645); c.num_relations = k.get("rels", 100); c.shard_edges = k.get("edges", 10000);
    c.pair_ok = k.get("pair_ok", 1) != 0; c.fast_ok = k.get("fast_ok", 1) != 0; c.fast_groups = (int)k.get("groups", 256);
    c.row_order = k.get("row_order", 1) != 0;
    c.fin = k.get("fin", 48); c.fout = k.get("fout", 32); c.bases = k.get("bases", 32);
    c.flags = (k.get("partial", 0) ? GN_RGCN_PARTIAL : 0) | (k.get("fast", 0) ? GN_RGCN_ARITH_FAST : 0) |
              (k.get("transposed", 0) ? GN_RGCN_BASIS_TRANSPOSED : 0) | (k.get("sum", 0) ? GN_RGCN_SUM : 0) |
              ((int)k.get("force", 0) << GN_RGCN_PATH_SHIFT) | (int)k.get("bits", 0);
    c.x_known = k.get("x_known", 1) != 0; c.ld_x = k.get("ld_x", c.fin); c.x_at = (unsigned)k.get("x_at", 0);
    c.basis_at = (unsigned)k.get("basis_at", 0);
    c.ld_summed = k.get("ld_summed", c.fout); c.summed_at = (unsigned)k.get("summed_at", 0);
    c.fast_disabled = k.get("fast_off", 0) != 0;
    c.slab_bytes = k.get("slab_mb", 256) << 20;
    return c;
}

static const char* kKernel[] = {"pair", "lds", "general", "table", "slab_finalize", "gemm_finalize", "refused"};
static const char* kWhy[] = {"none", "undefined_flags", "sum_with_partial", "weighted_flags", "basis_transposed", "weighted_shapes"};

static void print_route(const RelRoute& r) {
    const char* name = kKernel[(int)r.kernel];
    switch (r.kernel) {
        case RelKernel::refused: printf("refused %d %s\n", (int)r.status, kWhy[(int)r.why]); break;
        case RelKernel::pair: printf("pair nt=%d bt=%d terms=%d ws=%zu\n", r.nt, r.bt, r.terms, r.workspace); break;
        case RelKernel::lds: printf("lds ws=%zu wbytes=%zu\n", r.workspace, r.lds_w_bytes); break;
        case RelKernel::general:
            printf("general nt=%d bt=%d terms=%d wt=%d ws=%zu kp=%d slab_rows=%lld slabs=%lld w=%zu q=%zu o=%zu u=%zu\n", r.nt, r.bt, r.terms,
                   r.wt ? 1 : 0, r.workspace, r.kp, (long long)r.slab_rows, (long long)r.slabs, r.w_off, r.q_off, r.o_off, r.u_off);
            break;
        case RelKernel::table: printf("table ws=%zu w=%zu h=%zu xr=%zu\n", r.workspace, r.w_off, r.h_off, r.xr_off); break;
        default: printf("%s\n", name); break;
    }
}

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        Case k;
        if (!parse(line, k) || (k.kind != "forward" && k.kind != "weighted" && k.kind != "finalize")) {
            printf("?\n");
            continue;
        }
        print_route(rel_route(call_of(k)));
    }
    return 0;
}
