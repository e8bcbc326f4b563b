// The decoder forward's route (gripnet_amd/csrc/decoder_route.hpp) as a stand-alone host program: reads one case per line from
// standard input and prints the route - kernel, grid, block, LDS bytes and the fields the kernel's arguments take from it - or
// the refusal's status and reason, one line per case.  tests/test_decoder_route.py builds it with g++ under AddressSanitizer +
// UBSan and holds the expected lines.
//
// A case is a request kind and key=value pairs; what a line leaves out keeps its default:
//
//   raw | packed      gn_distmult_forward_f32, gn_distmult_packed_forward_f32:  f=80 ld_z=f ld_d=f
//   planned           gn_distmult_plan_forward_cols_f32:  nf=80 col_lo=0 col_hi=nf ld_z=nf ld_d=nf (f is col_hi - col_lo)
//                     the plan: cls_ok=0 cls_features=nf cls_groups=256 cls_by_args=(cls_groups <= 256) batches=1000
//
//   n=645 r=8 e=100000            nodes, relations, edges
//   z_at d_at = 0                 bytes of the pointer past a 16-byte boundary
//   fast_off=0 threads=1024       GN_DISABLE_FAST, GN_DM_THREADS
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "decoder_route.hpp"

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

static DecoderCall call_of(const Case& k) {
    DecoderCall c{};
    c.kind = k.kind == "planned" ? DecoderKind::planned : k.kind == "packed" ? DecoderKind::packed : DecoderKind::raw;
    c.n = k.get("n", 645); c.r = k.get("r", 8); c.e = k.get("e", 100000);
    if (c.kind == DecoderKind::planned) {
        c.num_features = k.get("nf", 80); c.col_lo = k.get("col_lo", 0); c.col_hi = k.get("col_hi", c.num_features);
        c.f = c.col_hi - c.col_lo;
    } else {
        c.f = k.get("f", 80);
        c.col_lo = 0; c.col_hi = c.f; c.num_features = c.f;
    }
    c.ld_z = k.get("ld_z", c.num_features); c.ld_d = k.get("ld_d", c.num_features);
    c.z_at = (unsigned)k.get("z_at", 0); c.d_at = (unsigned)k.get("d_at", 0);
    c.cls_ok = k.get("cls_ok", 0) != 0; c.cls_features = (int)k.get("cls_features", c.num_features);
    c.cls_groups = (int)k.get("cls_groups", 256); c.cls_by_args = k.get("cls_by_args", c.cls_groups <= 256) != 0;
    c.batches = k.get("batches", 1000);
    c.fast_disabled = k.get("fast_off", 0) != 0; c.threads = (int)k.get("threads", 1024);
    return c;
}

static const char* kKernel[] = {"general_vec", "general_scalar", "lds_raw", "lds_packed", "cls", "cls_wide", "phase", "refused"};
static const char* kWhy[] = {"none", "packed_shape", "class_only", "planned_shape"};

static void print_list(const char* name, const int* v, int k) {
    printf(" %s=", name);
    for (int i = 0; i < k; ++i) printf(i ? ",%d" : "%d", v[i]);
}

static void print_route(const DecoderRoute& r) {
    const char* name = kKernel[(int)r.kernel];
    switch (r.kernel) {
        case DecoderKernel::refused: printf("refused %d %s\n", (int)r.status, kWhy[(int)r.why]); return;
        case DecoderKernel::cls:
        case DecoderKernel::cls_wide:
            printf("%s J=%d J1=%d dma=%d grid=%u block=%u lds=%zu\n", name, r.J, r.J1, r.dma ? 1 : 0, r.grid, r.block, r.lds_bytes);
            return;
        case DecoderKernel::general_vec:
        case DecoderKernel::general_scalar: printf("%s grid=%u block=%u lds=%zu\n", name, r.grid, r.block, r.lds_bytes); return;
        default: break;
    }
    printf("%s grid=%u block=%u lds=%zu phases=%d", name, r.grid, r.block, r.lds_bytes, r.n_phases);
    print_list("c0", r.c0, r.n_phases);
    print_list("width", r.width, r.n_phases);
    if (r.kernel == DecoderKernel::phase)
        printf(" stride4=%d batches_per_wg=%lld keep_n=%d all_kept=%d\n", r.stride4, (long long)r.batches_per_wg, r.keep_n, r.all_kept ? 1 : 0);
    else
        printf(" stride4=%d edges_per_wg=%lld stage_bytes=%d tile_edges=%lld stage_off=%d\n", r.stride4, (long long)r.edges_per_wg,
               r.stage_bytes, (long long)r.tile_edges, r.stage_off);
}

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        Case k;
        if (!parse(line, k) || (k.kind != "raw" && k.kind != "packed" && k.kind != "planned")) {
            printf("?\n");
            continue;
        }
        print_route(decoder_route(call_of(k)));
    }
    return 0;
}
