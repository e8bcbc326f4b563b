"""The relational forward's route (gripnet_amd/csrc/rgcn_route.hpp): which kernel a gn_rgcn_forward_f32, gn_rgcn_forward_weighted_f32
or gn_rgcn_finalize_f32 call takes, with which template arguments, how many bytes of workspace in which layout, and what is
refused why - one case on each side of every boundary (no GPU)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The cases as tests/rgcn_route_host.cpp reads them (its header lists the keys and their defaults: a 645-node plan with both
# schedules and the degree order, 48 -> 32 on 32 bases, an aligned x and basis).
# The expected lines were printed once by the code the library held before the route was written down in one place (commit
# 983e0c9: select_path, path_workspace_bytes and general_layout of rgcn.hip with the flag and GN_RGCN_BASIS_TRANSPOSED refusals of
# gn_rgcn_forward_f32 and the flag and shape refusals of gn_rgcn_forward_weighted_f32 around them, gn_rgcn_pair_applicable,
# gn_rgcn_fast_applicable, gn_rgcn_fast_workspace_bytes, gn_rgcn_fast_finalize_applicable, gn_rgcn_basis_applicable, basis_layout
# and gn_rgcn_basis_workspace_bytes, and the nt / bt / terms / offsets lines of gn_rgcn_pair_forward, gn_rgcn_fast_forward and
# gn_rgcn_basis_forward, lifted verbatim into a scratch program with a stand-in plan struct and recorders in place of the launches),
# not by rgcn_route.hpp.
# "refused N why": gn_status N (1 GN_ERR_INVALID_ARG, 4 GN_ERR_UNSUPPORTED) and the refusal the caller words.
# Three bounds have no far side inside the clauses around them, and so no case beyond them: a thread of the destination-major
# kernel holds at most 32 * 32 / 64 = 16 rows of basis below fin 48 (17 needs fout 68: the case below fails the width clause with
# it), 17 tiles is no product of a bases count and a features count (18 stands in), and 128 features on 64 bases, the widest the
# general kernel takes, are the sum's 32 tiles.
ROUTES = [
    # pair, widths: fin 15 / 16 / 17 and 64 / 80 (16 bases: four tiles), bases 0 / 1 and 32 / 33, fout 3 / 4, 6, 64 / 68 (32 -> ., 16 bases)
    ("forward fin=15",                                                              "general nt=1 bt=2 terms=3 wt=0 ws=1386752 kp=512 slab_rows=645 slabs=1 w=0 q=65536 o=65792 u=65792"),
    ("forward fin=16",                                                              "pair nt=1 bt=2 terms=3 ws=0"),
    ("forward fin=17",                                                              "general nt=2 bt=2 terms=3 wt=0 ws=1560064 kp=576 slab_rows=645 slabs=1 w=0 q=73728 o=73984 u=73984"),
    ("forward fin=64 bases=16",                                                     "pair nt=4 bt=1 terms=3 ws=0"),
    ("forward fin=80 bases=16",                                                     "general nt=5 bt=1 terms=3 wt=0 ws=3726464 kp=1376 slab_rows=645 slabs=1 w=0 q=176128 o=176384 u=176384"),
    ("forward bases=0",                                                             "table ws=8953088 w=0 h=614400 xr=8870400"),
    ("forward bases=1",                                                             "pair nt=3 bt=1 terms=3 ws=0"),
    ("forward bases=32",                                                            "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward bases=33",                                                            "lds ws=21749760 wbytes=614400"),
    ("forward fout=3",                                                              "general nt=3 bt=2 terms=3 wt=0 ws=4147456 kp=1600 slab_rows=645 slabs=1 w=0 q=19200 o=19456 u=19456"),
    ("forward fout=4",                                                              "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward fout=6",                                                              "general nt=3 bt=2 terms=3 wt=0 ws=4166656 kp=1600 slab_rows=645 slabs=1 w=0 q=38400 o=38656 u=38656"),
    ("forward fin=32 bases=16 fout=64",                                             "pair nt=2 bt=1 terms=3 ws=0"),
    ("forward fin=32 bases=16 fout=68",                                             "general nt=2 bt=1 terms=3 wt=0 ws=1551744 kp=544 slab_rows=645 slabs=1 w=0 q=147968 o=148224 u=148224"),
    # pair, tiles: (fin / 16) * ceil(bases / 16) = 6 (48 x 32 bases) against 8 (64 x 17 bases: nine rows of basis a thread)
    ("forward fin=48 bases=32",                                                     "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward fin=64 bases=17",                                                     "lds ws=21954560 wbytes=819200"),
    # pair, rows of basis a thread: 12 / 13 at fin 48 (28 / 30 bases -> 36: 113 slices), 16 at fin 32 (32 bases -> 64: 64 slices)
    ("forward fin=48 bases=28 fout=36",                                             "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward fin=48 bases=30 fout=36",                                             "general nt=3 bt=2 terms=3 wt=0 ws=4097152 kp=1504 slab_rows=645 slabs=1 w=0 q=216576 o=216832 u=216832"),
    ("forward fin=32 bases=32 fout=64",                                             "pair nt=2 bt=2 terms=3 ws=0"),
    ("forward fin=32 bases=32 fout=68",                                             "general nt=2 bt=2 terms=3 wt=0 ws=3011968 kp=1056 slab_rows=645 slabs=1 w=0 q=287232 o=287488 u=287488"),
    # pair, the call and the plan: basis 0 / 4 bytes past alignment, no pair schedule, fast paths off
    ("forward basis_at=0",                                                          "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward basis_at=4",                                                          "lds ws=21749760 wbytes=614400"),
    ("forward basis_at=4 fast_ok=0",                                                "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward pair_ok=0",                                                           "lds ws=21749760 wbytes=614400"),
    ("forward fast_off=1",                                                          "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    # lds (a plan without the pair schedule): fout 31 / 32 / 33, fin 16 / 32 / 48 / 64 and one value between each, beyond 64
    ("forward pair_ok=0 fout=31",                                                   "general nt=3 bt=2 terms=3 wt=0 ws=4326656 kp=1600 slab_rows=645 slabs=1 w=0 q=198400 o=198656 u=198656"),
    ("forward pair_ok=0 fout=32",                                                   "lds ws=21749760 wbytes=614400"),
    ("forward pair_ok=0 fout=33",                                                   "general nt=3 bt=2 terms=3 wt=0 ws=4339456 kp=1600 slab_rows=645 slabs=1 w=0 q=211200 o=211456 u=211456"),
    ("forward pair_ok=0 fin=16",                                                    "lds ws=21340160 wbytes=204800"),
    ("forward pair_ok=0 fin=24",                                                    "general nt=2 bt=2 terms=3 wt=0 ws=2166656 kp=800 slab_rows=645 slabs=1 w=0 q=102400 o=102656 u=102656"),
    ("forward pair_ok=0 fin=32",                                                    "lds ws=21544960 wbytes=409600"),
    ("forward pair_ok=0 fin=40",                                                    "general nt=3 bt=2 terms=3 wt=0 ws=3639808 kp=1344 slab_rows=645 slabs=1 w=0 q=172032 o=172288 u=172288"),
    ("forward pair_ok=0 fin=48",                                                    "lds ws=21749760 wbytes=614400"),
    ("forward pair_ok=0 fin=56",                                                    "general nt=4 bt=2 terms=3 wt=0 ws=5026304 kp=1856 slab_rows=645 slabs=1 w=0 q=237568 o=237824 u=237824"),
    ("forward pair_ok=0 fin=64",                                                    "lds ws=21954560 wbytes=819200"),
    ("forward pair_ok=0 fin=80",                                                    "general nt=5 bt=2 terms=3 wt=0 ws=7192704 kp=2656 slab_rows=645 slabs=1 w=0 q=339968 o=340224 u=340224"),
    # lds: ld_x % 4, x 4 bytes past alignment, x unknown (a query: aligned, whatever ld_x), no work items
    ("forward pair_ok=0 ld_x=52",                                                   "lds ws=21749760 wbytes=614400"),
    ("forward pair_ok=0 ld_x=50",                                                   "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward pair_ok=0 x_at=4",                                                    "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward pair_ok=0 x_known=0",                                                 "lds ws=21749760 wbytes=614400"),
    ("forward pair_ok=0 x_known=0 ld_x=50 x_at=4",                                  "lds ws=21749760 wbytes=614400"),
    ("forward pair_ok=0 fast_ok=0",                                                 "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward pair_ok=0 groups=3 nodes=40 rels=3",                                  "lds ws=33792 wbytes=18432"),
    # general (neither schedule): fin 128 / 129, bases 64 / 65, 16 / 18 tiles for the mean (17 is no product of the two counts)
    ("forward pair_ok=0 fast_ok=0 fin=128 bases=32",                                "general nt=8 bt=2 terms=3 wt=0 ws=11438848 kp=4224 slab_rows=645 slabs=1 w=0 q=540672 o=540928 u=540928"),
    ("forward pair_ok=0 fast_ok=0 fin=129 bases=16",                                "table ws=9989888 w=0 h=1651200 xr=9907200"),
    ("forward pair_ok=0 fast_ok=0 fin=64 bases=64",                                 "general nt=4 bt=4 terms=3 wt=0 ws=11265536 kp=4160 slab_rows=645 slabs=1 w=0 q=532480 o=532736 u=532736"),
    ("forward pair_ok=0 fast_ok=0 fin=48 bases=65",                                 "table ws=8953088 w=0 h=614400 xr=8870400"),
    ("forward pair_ok=0 fast_ok=0 fin=96 bases=48",                                 "table ws=9567488 w=0 h=1228800 xr=9484800"),
    ("forward pair_ok=0 fast_ok=0 fin=1 bases=1 fout=1",                            "general nt=1 bt=1 terms=3 wt=0 ws=83072 kp=32 slab_rows=645 slabs=1 w=0 q=256 o=512 u=512"),
    # general: 32 tiles (128 features x 64 bases, the most the widths allow) for the sum and the weighted kind, not for the mean
    ("forward pair_ok=0 fast_ok=0 fin=128 bases=64",                                "table ws=9977088 w=0 h=1638400 xr=9894400"),
    ("forward pair_ok=0 fast_ok=0 fin=128 bases=64 sum=1",                          "general nt=8 bt=4 terms=3 wt=0 ws=22530816 kp=8320 slab_rows=645 slabs=1 w=0 q=1064960 o=1065216 u=1065216"),
    ("weighted fin=128 bases=64 sum=1",                                             "general nt=8 bt=4 terms=3 wt=1 ws=22530816 kp=8320 slab_rows=645 slabs=1 w=0 q=1064960 o=1065216 u=1065216"),
    ("forward pair_ok=0 fast_ok=0 fin=129 bases=64 sum=1",                          "table ws=9989888 w=0 h=1651200 xr=9907200"),
    ("forward pair_ok=0 fast_ok=0 fin=128 bases=65 sum=1",                          "table ws=9977088 w=0 h=1638400 xr=9894400"),
    # general: no degree order
    ("forward pair_ok=0 fast_ok=0 row_order=0",                                     "table ws=8953088 w=0 h=614400 xr=8870400"),
    ("forward row_order=0 sum=1",                                                   "table ws=8953088 w=0 h=614400 xr=8870400"),
    ("weighted row_order=0 sum=1",                                                  "refused 4 weighted_shapes"),
    # general, workspace (rows of 1600 floats): exactly one slab and one row more; the 256-row floor; the 256-slab cap; a 1 MB slab of
    # 128-byte rows; no nodes
    ("forward force=4 nodes=41943",                                                 "general nt=3 bt=2 terms=3 wt=0 ws=268640256 kp=1600 slab_rows=41943 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward force=4 nodes=41944",                                                 "general nt=3 bt=2 terms=3 wt=0 ws=268808192 kp=1600 slab_rows=41943 slabs=2 w=0 q=204800 o=205056 u=372992"),
    ("forward force=4 nodes=1000 slab_mb=1",                                        "general nt=3 bt=2 terms=3 wt=0 ws=1847552 kp=1600 slab_rows=256 slabs=4 w=0 q=204800 o=205056 u=209152"),
    ("forward force=4 nodes=256 slab_mb=1",                                         "general nt=3 bt=2 terms=3 wt=0 ws=1843456 kp=1600 slab_rows=256 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward force=4 nodes=257 slab_mb=1",                                         "general nt=3 bt=2 terms=3 wt=0 ws=1844736 kp=1600 slab_rows=256 slabs=2 w=0 q=204800 o=205056 u=206336"),
    ("forward force=4 nodes=100000 slab_mb=1",                                      "general nt=3 bt=2 terms=3 wt=0 ws=3109376 kp=1600 slab_rows=391 slabs=256 w=0 q=204800 o=205824 u=606976"),
    ("forward force=4 nodes=100097 slab_mb=1",                                      "general nt=3 bt=2 terms=3 wt=0 ws=3116288 kp=1600 slab_rows=392 slabs=256 w=0 q=204800 o=205824 u=607488"),
    ("forward force=4 nodes=10000 slab_mb=1 fin=16 bases=1",                        "general nt=1 bt=1 terms=3 wt=0 ws=1093120 kp=32 slab_rows=8192 slabs=2 w=0 q=4096 o=4352 u=44544"),
    ("forward force=4 nodes=8192 slab_mb=1 fin=16 bases=1",                         "general nt=1 bt=1 terms=3 wt=0 ws=1052928 kp=32 slab_rows=8192 slabs=1 w=0 q=4096 o=4352 u=4352"),
    ("forward force=4 nodes=0",                                                     "general nt=3 bt=2 terms=3 wt=0 ws=211456 kp=1600 slab_rows=1 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward force=4 nodes=1000000 fin=128 bases=32 fout=64",                      "general nt=8 bt=2 terms=3 wt=0 ws=273508608 kp=4224 slab_rows=15887 slabs=63 w=0 q=1081344 o=1081600 u=5081856"),
    # table: W, H and x root at sizes that are and are not multiples of 256 bytes (H = relations x the third); no relations; no nodes
    ("forward force=5 nodes=64 rels=1 fin=16 fout=4",                               "table ws=2304 w=0 h=256 xr=1280"),
    ("forward force=5 nodes=64 rels=1 fin=15 fout=4",                               "table ws=2304 w=0 h=256 xr=1280"),
    ("forward force=5 nodes=8 rels=2 fin=16 fout=4",                                "table ws=1024 w=0 h=512 xr=768"),
    ("forward force=5 nodes=8 rels=3 fin=16 fout=4",                                "table ws=1536 w=0 h=768 xr=1280"),
    ("forward force=5 nodes=1 rels=1 fin=1 fout=1 bases=1",                         "table ws=768 w=0 h=256 xr=512"),
    ("forward force=5 rels=0",                                                      "table ws=82688 w=0 h=0 xr=0"),
    ("forward force=5 nodes=0",                                                     "table ws=614400 w=0 h=614400 xr=614400"),
    # forced kernels on shapes all four cover, on shapes only general and table cover, on shapes only table covers; codes without a kernel
    ("forward force=0",                                                             "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward force=1",                                                             "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward force=3",                                                             "lds ws=21749760 wbytes=614400"),
    ("forward force=4",                                                             "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward force=5",                                                             "table ws=8953088 w=0 h=614400 xr=8870400"),
    ("forward force=0 fin=80 bases=16",                                             "general nt=5 bt=1 terms=3 wt=0 ws=3726464 kp=1376 slab_rows=645 slabs=1 w=0 q=176128 o=176384 u=176384"),
    ("forward force=1 fin=80 bases=16",                                             "general nt=5 bt=1 terms=3 wt=0 ws=3726464 kp=1376 slab_rows=645 slabs=1 w=0 q=176128 o=176384 u=176384"),
    ("forward force=3 fin=80 bases=16",                                             "general nt=5 bt=1 terms=3 wt=0 ws=3726464 kp=1376 slab_rows=645 slabs=1 w=0 q=176128 o=176384 u=176384"),
    ("forward force=4 fin=80 bases=16",                                             "general nt=5 bt=1 terms=3 wt=0 ws=3726464 kp=1376 slab_rows=645 slabs=1 w=0 q=176128 o=176384 u=176384"),
    ("forward force=5 fin=80 bases=16",                                             "table ws=9362688 w=0 h=1024000 xr=9280000"),
    ("forward force=0 fin=129 bases=16",                                            "table ws=9989888 w=0 h=1651200 xr=9907200"),
    ("forward force=1 fin=129 bases=16",                                            "table ws=9989888 w=0 h=1651200 xr=9907200"),
    ("forward force=3 fin=129 bases=16",                                            "table ws=9989888 w=0 h=1651200 xr=9907200"),
    ("forward force=4 fin=129 bases=16",                                            "table ws=9989888 w=0 h=1651200 xr=9907200"),
    ("forward force=5 fin=129 bases=16",                                            "table ws=9989888 w=0 h=1651200 xr=9907200"),
    ("forward force=2",                                                             "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward force=6",                                                             "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward force=7",                                                             "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward force=3 x_at=4",                                                      "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward force=1 basis_at=4",                                                  "lds ws=21749760 wbytes=614400"),
    # flags: the sum alone, with each forced kernel, with the partial sum; a transposed basis on pair and on each other kernel
    ("forward sum=1",                                                               "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward sum=1 force=1",                                                       "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward sum=1 force=3",                                                       "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward sum=1 force=4",                                                       "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward sum=1 force=5",                                                       "table ws=8953088 w=0 h=614400 xr=8870400"),
    ("forward sum=1 fin=129 bases=16",                                              "table ws=9989888 w=0 h=1651200 xr=9907200"),
    ("forward sum=1 partial=1",                                                     "refused 1 sum_with_partial"),
    ("forward partial=1",                                                           "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward transposed=1",                                                        "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward transposed=1 force=1",                                                "pair nt=3 bt=2 terms=3 ws=0"),
    ("forward transposed=1 force=3",                                                "refused 4 basis_transposed"),
    ("forward transposed=1 force=4",                                                "refused 4 basis_transposed"),
    ("forward transposed=1 force=5",                                                "refused 4 basis_transposed"),
    ("forward transposed=1 basis_at=4",                                             "refused 4 basis_transposed"),
    ("forward transposed=1 sum=1",                                                  "refused 4 basis_transposed"),
    ("forward transposed=1 fast_off=1",                                             "refused 4 basis_transposed"),
    # flags: bits the entry does not define; fast paths off; two bf16 terms against three on pair and on general
    ("forward bits=2",                                                              "refused 1 undefined_flags"),
    ("forward bits=8",                                                              "refused 1 undefined_flags"),
    ("forward bits=16",                                                             "refused 1 undefined_flags"),
    ("forward bits=32",                                                             "refused 1 undefined_flags"),
    ("forward bits=2048",                                                           "refused 1 undefined_flags"),
    ("forward bits=2 sum=1 partial=1",                                              "refused 1 undefined_flags"),
    ("forward fast_off=1 force=1",                                                  "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward fast_off=1 force=3",                                                  "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward fast=1",                                                              "pair nt=3 bt=2 terms=2 ws=0"),
    ("forward fast=1 force=4",                                                      "general nt=3 bt=2 terms=2 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("forward fast=1 force=3",                                                      "lds ws=21749760 wbytes=614400"),
    ("forward fast=1 sum=1",                                                        "general nt=3 bt=2 terms=2 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    # the weighted kind: one of the two flags alone; no edges; shapes the general kernel does not cover
    ("weighted sum=1",                                                              "general nt=3 bt=2 terms=3 wt=1 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("weighted partial=1",                                                          "general nt=3 bt=2 terms=3 wt=1 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("weighted sum=1 partial=1",                                                    "refused 1 weighted_flags"),
    ("weighted",                                                                    "refused 1 weighted_flags"),
    ("weighted sum=1 fast=1",                                                       "refused 1 weighted_flags"),
    ("weighted sum=1 force=4",                                                      "refused 1 weighted_flags"),
    ("weighted sum=1 edges=0",                                                      "general nt=3 bt=2 terms=3 wt=0 ws=4333056 kp=1600 slab_rows=645 slabs=1 w=0 q=204800 o=205056 u=205056"),
    ("weighted sum=1 fin=129 bases=16",                                             "refused 4 weighted_shapes"),
    ("weighted sum=1 fin=48 bases=65",                                              "refused 4 weighted_shapes"),
    ("weighted sum=1 pair_ok=0 fast_ok=0 fast_off=1 nodes=100000 slab_mb=1",        "general nt=3 bt=2 terms=3 wt=1 ws=3109376 kp=1600 slab_rows=391 slabs=256 w=0 q=204800 o=205824 u=606976"),
    # finalize: fout 32 / 33, fin 64 / 65, ld_summed 32 / 36, summed 4 bytes past alignment, fast paths off
    ("finalize fout=32",                                                            "slab_finalize"),
    ("finalize fout=33",                                                            "gemm_finalize"),
    ("finalize fout=31",                                                            "gemm_finalize"),
    ("finalize fin=64",                                                             "slab_finalize"),
    ("finalize fin=65",                                                             "gemm_finalize"),
    ("finalize fin=1",                                                              "slab_finalize"),
    ("finalize ld_summed=32",                                                       "slab_finalize"),
    ("finalize ld_summed=36",                                                       "gemm_finalize"),
    ("finalize summed_at=4",                                                        "gemm_finalize"),
    ("finalize fast_off=1",                                                         "gemm_finalize"),
    # the smallest plan all four kernels take (tests/test_gpu_parity.py runs these ten on the GPU): each forced kernel, on an aligned x and on
    # a view 4 bytes past alignment
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=0",           "pair nt=1 bt=1 terms=3 ws=0"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=1",           "pair nt=1 bt=1 terms=3 ws=0"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=3",           "lds ws=21504 wbytes=6144"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=4",           "general nt=1 bt=1 terms=3 wt=0 ws=18688 kp=64 slab_rows=40 slabs=1 w=0 q=8192 o=8448 u=8448"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=5",           "table ws=26624 w=0 h=6144 xr=21504"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=0 x_at=4",    "pair nt=1 bt=1 terms=3 ws=0"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=1 x_at=4",    "pair nt=1 bt=1 terms=3 ws=0"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=3 x_at=4",    "pair nt=1 bt=1 terms=3 ws=0"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=4 x_at=4",    "general nt=1 bt=1 terms=3 wt=0 ws=18688 kp=64 slab_rows=40 slabs=1 w=0 q=8192 o=8448 u=8448"),
    ("forward nodes=40 rels=3 edges=300 groups=3 fin=16 bases=2 force=5 x_at=4",    "table ws=26624 w=0 h=6144 xr=21504"),
]


def route_line(case):
    """The expected line of `case` (tests/test_gpu_parity.py holds the library's answers on the GPU to the same table)."""
    return dict(ROUTES)[case]


def test_rgcn_routes_at_every_boundary(tmp_path):
    """tests/rgcn_route_host.cpp, built with g++ under AddressSanitizer + UBSan, prints the route of every case of ROUTES:
    each line equals what the earlier choice, applicability and layout functions said for the same arguments."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    assert len(dict(ROUTES)) == len(ROUTES), "a case is listed twice"
    exe = tmp_path / "rgcn_route_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-I", os.path.join(REPO, "gripnet_amd", "csrc"), "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "rgcn_route_host.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], input="".join(case + "\n" for case, _ in ROUTES), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    got = run.stdout.splitlines()
    assert len(got) == len(ROUTES), (len(got), run.stderr[-2000:])
    wrong = [(case, want, line) for (case, want), line in zip(ROUTES, got) if line != want]
    assert not wrong, wrong
