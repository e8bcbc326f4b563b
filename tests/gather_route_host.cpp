// The gather family's route (gripnet_amd/csrc/gather_route.hpp) as a stand-alone host program: reads one case per line from
// standard input and prints the route - kernel, lanes per row, grid, block, LDS bytes, who writes the planes - or the refusal's
// status and reason, one line per case.  tests/test_gather_route.py builds it with g++ under AddressSanitizer + UBSan and holds
// the expected lines.
//
// A case is a request kind and key=value pairs; what a line leaves out keeps its default:
//
//   f32 | bf16 | tail | split     a forward call of that kind (gn_graph_aggregate_f32, _bf16, _tail_f32, _split_f32; a bare
//                                 gather-reduce - rgcn.hip's sum, gn_graph_aggregate_t_f32 - is an f32 call without a plan's facts)
//   q_blocked                     gn_graph_blocked_applicable for the same operands
//   fusable                       gn_transform_fusable and gn_graph_transform_fusable (fin fout rows nnz fast_off)
//
//   rows=1000 nnz=-1 table_rows=-1 blk_ok=0 cw=2 blk_cols=32            the plan
//   fin=16 fout=fin w=0 ld_table=fin ld_out=fout                        widths, a weight, leading dimensions
//   table_at out_at bias_at w_at tail_at tail_w_at tail_b_at = 0        bytes of the pointer past a 16-byte boundary
//   coef rowdiv addend bias relu side planes = 0                        what the call brings
//   head_cols=16 ld_tail=fin-head_cols head=1 tail=1                    split source
//   fast_off quad_off lds_off blk_off = 0, cus=256                      GN_DISABLE_FAST / _QUAD / _LDS_TABLE / _BLOCKED, compute units
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "gather_route.hpp"

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

static GatherCall call_of(const Case& k) {
    GatherCall c{};
    c.kind = k.kind == "bf16" ? Source::bf16 : k.kind == "tail" ? Source::tail : k.kind == "split" ? Source::split : Source::f32;
    c.rows = k.get("rows", 1000); c.nnz = k.get("nnz", -1); c.table_rows = k.get("table_rows", -1);
    c.blk_ok = k.get("blk_ok", 0) != 0; c.blk_cw = (int)k.get("cw", 2); c.blk_cols = (int)k.get("blk_cols", 32);
    c.features = k.get("fin", 16); c.fout = k.get("fout", c.features); c.weight = k.get("w", 0) != 0;
    c.ld_table = k.get("ld_table", c.kind == Source::split ? k.get("head_cols", 16) : c.features); c.ld_out = k.get("ld_out", c.fout);
    c.table_at = (unsigned)k.get("table_at", 0); c.out_at = (unsigned)k.get("out_at", 0); c.bias_at = (unsigned)k.get("bias_at", 0);
    c.weight_at = (unsigned)k.get("w_at", 0);
    c.coef = k.get("coef", 0) != 0; c.rowdiv = k.get("rowdiv", 0) != 0; c.addend = k.get("addend", 0) != 0;
    c.bias = k.get("bias", 0) != 0; c.relu = k.get("relu", 0) != 0; c.side = k.get("side", 0) != 0; c.planes = k.get("planes", 0) != 0;
    c.head_cols = k.get("head_cols", 16); c.ld_tail = k.get("ld_tail", c.features - c.head_cols);
    c.head = k.get("head", 1) != 0; c.tail = k.get("tail", 1) != 0; c.tail_at = (unsigned)k.get("tail_at", 0);
    c.tail_w_at = (unsigned)k.get("tail_w_at", 0); c.tail_b_at = (unsigned)k.get("tail_b_at", 0);
    c.fast_disabled = k.get("fast_off", 0) != 0; c.quad_disabled = k.get("quad_off", 0) != 0;
    c.lds_table_disabled = k.get("lds_off", 0) != 0; c.blocked_disabled = k.get("blk_off", 0) != 0;
    c.compute_units = (int)k.get("cus", 256);
    return c;
}

static const char* kKernel[] = {"blocked", "mfma", "transform", "transform_quad", "transform_tail", "transform_split", "lds_table",
                                "short_rows", "group", "wave", "wave_scalar", "bf16_group", "bf16_wave", "refused"};
static const char* kWhy[] = {"none", "no_fused_transform", "tail_operands", "split_fast_off", "split_widths", "split_head_cols",
                             "split_alignment", "split_ld_multiple", "split_ld_short", "split_ld_31_bits"};

static void print_route(const GatherRoute& r) {
    const int by_kernel = r.planes_by_kernel ? 1 : 0;
    if (r.kernel == Gather::refused) printf("refused %d %s\n", (int)r.status, kWhy[(int)r.why]);
    else if (r.kernel == Gather::blocked) printf("blocked planes_by_kernel=%d\n", by_kernel);
    else if (r.kernel == Gather::mfma)
        printf("mfma lpe=%d grid=%u block=%u lds=%lld row_blocks=%d planes_by_kernel=%d\n", r.lpe, r.grid, r.block, (long long)r.lds,
               r.row_blocks, by_kernel);
    else
        printf("%s lpe=%d grid=%u block=%u lds=%lld planes_by_kernel=%d\n", kKernel[(int)r.kernel], r.lpe, r.grid, r.block,
               (long long)r.lds, by_kernel);
}

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        Case k;
        if (!parse(line, k)) {
            printf("?\n");
            continue;
        }
        const GatherCall c = call_of(k);
        if (k.kind == "f32" || k.kind == "bf16" || k.kind == "tail" || k.kind == "split") {
            print_route(gather_route(c));
        } else if (k.kind == "q_blocked") {
            printf("blocked_applicable %d\n", gather_route(c).kernel == Gather::blocked ? 1 : 0);
        } else if (k.kind == "fusable") {
            const bool t = transform_fusable(c.features, c.fout, c.fast_disabled);
            printf("transform_fusable %d graph_transform_fusable %d\n", t ? 1 : 0,
                   t || mfma_fusable(c.features, c.fout, c.rows, c.nnz, c.fast_disabled) ? 1 : 0);
        } else {
            printf("?\n");
        }
    }
    return 0;
}
