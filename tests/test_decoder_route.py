"""The decoder forward's route (gripnet_amd/csrc/decoder_route.hpp): which kernel and instantiation, grid, block, LDS size,
column phases, workgroup split, staging and partial-sum room a gn_distmult_forward_f32, gn_distmult_packed_forward_f32 or
gn_distmult_plan_forward_cols_f32 call gets, and what is refused why - one case on each side of every boundary (no GPU)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The cases as tests/decoder_route_host.cpp reads them (its header lists the keys and their defaults: 645 nodes, 80 features,
# 8 relations, 100000 edges, a plan of 1000 batches without the row-class encoding).
# The expected lines were printed once by the dispatch code the library held before the route was written down in one place
# (commit f5a4451: the if-chains of gn_distmult_forward_f32, gn_distmult_fast_applicable, distmult_lds_launch,
# gn_distmult_packed_forward_f32 and plan_forward_cols with plan_phases and lds_stride4 of distmult_quad.cuh, lifted verbatim into
# a scratch program with recorders in place of the launches), not by decoder_route.hpp.
# "refused N why": gn_status N (4 GN_ERR_UNSUPPORTED) and the refusal the caller words.
LDS_645 = "block=1024 lds=123840 phases=2 c0=0,48 width=48,32 stride4=12"      # the packed / unstaged call at the defaults
PHASE_645 = "block=1024 lds=127936 phases=2 c0=0,48 width=48,32 stride4=12"    # the planned call at the defaults: one kept batch a wave
ROUTES = [
    # "vector ok": f % 4, ld_z % 4, ld_d % 4, z and d alignment - each failing alone, on each request kind and plan encoding
    ("raw",                                         "lds_raw grid=98 block=1024 lds=127936 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=123840"),
    ("raw f=82 ld_z=84 ld_d=84",                    "general_scalar grid=391 block=256 lds=0"),
    ("raw ld_z=82",                                 "general_scalar grid=391 block=256 lds=0"),
    ("raw ld_d=82",                                 "general_scalar grid=391 block=256 lds=0"),
    ("raw z_at=4",                                  "general_scalar grid=391 block=256 lds=0"),
    ("raw d_at=8",                                  "general_scalar grid=391 block=256 lds=0"),
    ("packed",                                      "lds_packed grid=98 " + LDS_645 + " edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed f=82 ld_z=84 ld_d=84",                 "refused 4 packed_shape"),
    ("packed ld_z=82",                              "refused 4 packed_shape"),
    ("packed ld_d=82",                              "refused 4 packed_shape"),
    ("packed z_at=4",                               "refused 4 packed_shape"),
    ("packed d_at=8",                               "refused 4 packed_shape"),
    ("planned",                                     "phase grid=63 " + PHASE_645 + " batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned col_hi=78",                           "refused 4 planned_shape"),
    ("planned ld_z=82",                             "refused 4 planned_shape"),
    ("planned ld_d=82",                             "refused 4 planned_shape"),
    ("planned z_at=4",                              "refused 4 planned_shape"),
    ("planned d_at=8",                              "refused 4 planned_shape"),
    ("planned cls_ok=1",                            "cls J=5 J1=3 dma=1 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 col_hi=78",                  "refused 4 planned_shape"),
    ("planned cls_ok=1 ld_z=82",                    "refused 4 planned_shape"),
    ("planned cls_ok=1 ld_d=82",                    "refused 4 planned_shape"),
    ("planned cls_ok=1 z_at=4",                     "refused 4 planned_shape"),
    ("planned cls_ok=1 d_at=8",                     "refused 4 planned_shape"),
    # GN_DISABLE_FAST on each request kind (a class-only plan is refused as such first)
    ("raw fast_off=1",                              "general_vec grid=391 block=256 lds=0"),
    ("raw fast_off=1 z_at=4",                       "general_scalar grid=391 block=256 lds=0"),
    ("packed fast_off=1",                           "refused 4 packed_shape"),
    ("planned fast_off=1",                          "refused 4 planned_shape"),
    ("planned cls_ok=1 fast_off=1",                 "refused 4 planned_shape"),
    ("planned cls_ok=1 batches=0 fast_off=1",       "refused 4 class_only"),
    # n = 0 (the entry points refuse it when there are edges; the ladder still answers), n at 65535 / 65536 (beyond what the
    # LDS holds either way), packed r at 65535 / 65536
    ("raw n=0",                                     "general_vec grid=391 block=256 lds=0"),
    ("packed n=0",                                  "refused 4 packed_shape"),
    ("planned n=0",                                 "refused 4 planned_shape"),
    ("raw n=65535",                                 "general_vec grid=391 block=256 lds=0"),
    ("raw n=65536",                                 "general_vec grid=391 block=256 lds=0"),
    ("packed n=65535",                              "refused 4 packed_shape"),
    ("packed n=65536",                              "refused 4 packed_shape"),
    ("packed r=65535",                              "lds_packed grid=98 " + LDS_645 + " edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed r=65536",                              "refused 4 packed_shape"),
    # kLdsBudget: the widest phase 64 / 48 columns at n = 600 / 601, 16 columns / no LDS path at n = 2400 / 2401
    ("raw n=600",                                   "lds_raw grid=98 block=1024 lds=157696 phases=2 c0=0,64 width=64,16 stride4=16 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=153600"),
    ("raw n=601",                                   "lds_raw grid=98 block=1024 lds=119488 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=115392"),
    ("raw n=2400 f=64",                             "lds_raw grid=98 block=1024 lds=161792 phases=4 c0=0,16,32,48 width=16,16,16,16 stride4=4 edges_per_wg=1024 stage_bytes=8 tile_edges=1024 stage_off=153600"),
    ("raw n=2401 f=64",                             "general_vec grid=391 block=256 lds=0"),
    ("packed n=600",                                "lds_packed grid=98 block=1024 lds=153600 phases=2 c0=0,64 width=64,16 stride4=16 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=153600"),
    ("packed n=601",                                "lds_packed grid=98 block=1024 lds=115392 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=115392"),
    ("packed n=2400 f=64",                          "lds_packed grid=98 block=1024 lds=153600 phases=4 c0=0,16,32,48 width=16,16,16,16 stride4=4 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=153600"),
    ("packed n=2401 f=64",                          "refused 4 packed_shape"),
    ("planned n=600",                               "phase grid=63 block=1024 lds=157696 phases=2 c0=0,64 width=64,16 stride4=16 batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned n=601",                               "phase grid=63 block=1024 lds=119488 phases=2 c0=0,48 width=48,32 stride4=12 batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned n=2400 nf=64",                        "phase grid=63 block=1024 lds=157696 phases=4 c0=0,16,32,48 width=16,16,16,16 stride4=4 batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned n=2401 nf=64",                        "refused 4 planned_shape"),
    # phases at 4 / 5 (n = 2400, f = 64 above / 68), f = 4, f at the kMaxPhases edge (8 phases / none: both beyond the LDS
    # kernels' four)
    ("raw n=2400 f=68",                             "general_vec grid=391 block=256 lds=0"),
    ("packed n=2400 f=68",                          "refused 4 packed_shape"),
    ("planned n=2400 nf=68",                        "refused 4 planned_shape"),
    ("raw f=4",                                     "lds_raw grid=98 block=1024 lds=51600 phases=1 c0=0 width=4 stride4=5 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=51600"),
    ("packed f=4",                                  "lds_packed grid=98 block=1024 lds=51600 phases=1 c0=0 width=4 stride4=5 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=51600"),
    ("planned nf=4",                                "phase grid=63 block=1024 lds=51600 phases=1 c0=0 width=4 stride4=5 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("raw n=2400 f=128",                            "general_vec grid=391 block=256 lds=0"),
    ("raw n=2400 f=132",                            "general_vec grid=391 block=256 lds=0"),
    ("packed n=2400 f=128",                         "refused 4 packed_shape"),
    ("planned n=2400 nf=132",                       "refused 4 planned_shape"),
    # the row stride's pad (lds_stride4): on (32 columns; 64 columns at n = 505), none to add (16, 48 columns), refused for room
    # (64 columns at n = 506, 32 columns at n = 1000)
    ("raw f=32",                                    "lds_raw grid=98 block=1024 lds=123840 phases=1 c0=0 width=32 stride4=12 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("raw f=16",                                    "lds_raw grid=98 block=1024 lds=41280 phases=1 c0=0 width=16 stride4=4 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=41280"),
    ("raw f=48",                                    "lds_raw grid=98 block=1024 lds=123840 phases=1 c0=0 width=48 stride4=12 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("raw n=505 f=64",                              "lds_raw grid=98 block=1024 lds=161600 phases=1 c0=0 width=64 stride4=20 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=161600"),
    ("raw n=506 f=64",                              "lds_raw grid=98 block=1024 lds=129536 phases=1 c0=0 width=64 stride4=16 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=129536"),
    ("raw n=1000 f=64",                             "lds_raw grid=98 block=1024 lds=132096 phases=2 c0=0,32 width=32,32 stride4=8 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=128000"),
    ("planned n=505 nf=64",                         "phase grid=63 block=1024 lds=161600 phases=1 c0=0 width=64 stride4=20 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned n=506 nf=64",                         "phase grid=63 block=1024 lds=129536 phases=1 c0=0 width=64 stride4=16 batches_per_wg=16 keep_n=0 all_kept=0"),
    # staging: 4- or 8-byte triples at n = 1023 / 1024 and r = 4096 / 4097; none for packed and for single-phase calls
    ("raw n=1023",                                  "lds_raw grid=98 block=1024 lds=135040 phases=3 c0=0,32,64 width=32,32,16 stride4=8 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=130944"),
    ("raw n=1024",                                  "lds_raw grid=98 block=1024 lds=139264 phases=3 c0=0,32,64 width=32,32,16 stride4=8 edges_per_wg=1024 stage_bytes=8 tile_edges=1024 stage_off=131072"),
    ("raw r=4096",                                  "lds_raw grid=98 block=1024 lds=127936 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=123840"),
    ("raw r=4097",                                  "lds_raw grid=98 block=1024 lds=132032 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=1024 stage_bytes=8 tile_edges=1024 stage_off=123840"),
    ("packed r=4097",                               "lds_packed grid=98 " + LDS_645 + " edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("raw n=500 f=64",                              "lds_raw grid=98 block=1024 lds=160000 phases=1 c0=0 width=64 stride4=20 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=160000"),
    # staging: room for a tile of 1024 / 960 edges beside the table (n = 499 / 500 under 80 columns: the minimum is 1024), and
    # for 512 of 8 bytes
    ("raw n=499",                                   "lds_raw grid=98 block=1024 lds=163776 phases=2 c0=0,64 width=64,16 stride4=20 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=159680"),
    ("raw n=500",                                   "lds_raw grid=98 block=1024 lds=160000 phases=2 c0=0,64 width=64,16 stride4=20 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=160000"),
    ("raw n=499 r=4097",                            "lds_raw grid=98 block=1024 lds=159680 phases=2 c0=0,64 width=64,16 stride4=20 edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=159680"),
    # staging: the last e at which a workgroup's range is one tile and the first at which it needs two - where the second
    # tile's table fills cost more than the passes over the list they save (n = 499, n = 800: not staged) and where they cost
    # less (n = 645: two tiles of 9984 edges)
    ("raw n=499 e=262144",                          "lds_raw grid=256 block=1024 lds=163776 phases=2 c0=0,64 width=64,16 stride4=20 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=159680"),
    ("raw n=499 e=262145",                          "lds_raw grid=241 block=1024 lds=159680 phases=2 c0=0,64 width=64,16 stride4=20 edges_per_wg=1088 stage_bytes=0 tile_edges=0 stage_off=159680"),
    ("raw n=800 e=655360",                          "lds_raw grid=256 block=1024 lds=163840 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=2560 stage_bytes=4 tile_edges=2560 stage_off=153600"),
    ("raw n=800 e=655361",                          "lds_raw grid=250 block=1024 lds=153600 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=2624 stage_bytes=0 tile_edges=0 stage_off=153600"),
    ("raw n=645 e=2555904",                         "lds_raw grid=256 block=1024 lds=163776 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=9984 stage_bytes=4 tile_edges=9984 stage_off=123840"),
    ("raw n=645 e=2555905",                         "lds_raw grid=255 block=1024 lds=163776 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=10048 stage_bytes=4 tile_edges=9984 stage_off=123840"),
    # workgroups: e at 1, 64, 65; 255 / 256 groups; the last e of 1024-edge ranges and the first of longer ones under the cap of
    # 256 groups; the general kernel's grid at its cap of 2048 blocks
    ("raw e=1",                                     "lds_raw grid=1 block=1024 lds=124096 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=64 stage_bytes=4 tile_edges=64 stage_off=123840"),
    ("raw e=64",                                    "lds_raw grid=1 block=1024 lds=124096 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=64 stage_bytes=4 tile_edges=64 stage_off=123840"),
    ("raw e=65",                                    "lds_raw grid=1 block=1024 lds=124352 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=128 stage_bytes=4 tile_edges=128 stage_off=123840"),
    ("packed e=1",                                  "lds_packed grid=1 " + LDS_645 + " edges_per_wg=64 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed e=64",                                 "lds_packed grid=1 " + LDS_645 + " edges_per_wg=64 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed e=65",                                 "lds_packed grid=1 " + LDS_645 + " edges_per_wg=128 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed e=261120",                             "lds_packed grid=255 " + LDS_645 + " edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed e=261121",                             "lds_packed grid=256 " + LDS_645 + " edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed e=262144",                             "lds_packed grid=256 " + LDS_645 + " edges_per_wg=1024 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed e=262145",                             "lds_packed grid=241 " + LDS_645 + " edges_per_wg=1088 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("packed e=10000000",                           "lds_packed grid=256 " + LDS_645 + " edges_per_wg=39104 stage_bytes=0 tile_edges=0 stage_off=123840"),
    ("raw e=262144",                                "lds_raw grid=256 block=1024 lds=127936 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=1024 stage_bytes=4 tile_edges=1024 stage_off=123840"),
    ("raw e=262145",                                "lds_raw grid=241 block=1024 lds=128192 phases=2 c0=0,48 width=48,32 stride4=12 edges_per_wg=1088 stage_bytes=4 tile_edges=1088 stage_off=123840"),
    ("raw fast_off=1 e=1",                          "general_vec grid=1 block=256 lds=0"),
    ("raw fast_off=1 e=523968",                     "general_vec grid=2047 block=256 lds=0"),
    ("raw fast_off=1 e=524288",                     "general_vec grid=2048 block=256 lds=0"),
    ("raw fast_off=1 e=524289",                     "general_vec grid=2048 block=256 lds=0"),
    # row-class kernel: each of the six (J, J1) instantiations
    ("planned cls_ok=1 n=645 nf=80",                "cls J=5 J1=3 dma=1 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 n=400 nf=80",                "cls J=5 J1=4 dma=1 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 n=400 nf=64",                "cls J=4 J1=4 dma=0 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 n=645 nf=48",                "cls J=3 J1=3 dma=1 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 n=645 nf=32",                "cls J=2 J1=2 dma=0 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 n=645 nf=16",                "cls J=1 J1=1 dma=1 grid=256 block=1024 lds=163840"),
    # row-class kernel: a (J, J1) with no instantiation - (6, 3), (4, 3), three parts, (6, 4), (3, 2), (2, 1) - falls to the column
    # phases, or is refused on a class-only plan
    ("planned cls_ok=1 n=1000 nf=48",               "phase grid=63 block=1024 lds=132096 phases=2 c0=0,32 width=32,16 stride4=8 batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned cls_ok=1 n=2400 nf=32",               "phase grid=63 block=1024 lds=157696 phases=2 c0=0,16 width=16,16 stride4=4 batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned cls_ok=1 nf=96",                      "phase grid=63 block=1024 lds=127936 phases=2 c0=0,48 width=48,48 stride4=12 batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned cls_ok=1 nf=96 batches=0",            "refused 4 class_only"),
    ("planned cls_ok=1 nf=64",                      "phase grid=63 block=1024 lds=127936 phases=2 c0=0,48 width=48,16 stride4=12 batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned cls_ok=1 nf=64 batches=0",            "refused 4 class_only"),
    ("planned cls_ok=1 n=1000 nf=80",               "phase grid=63 block=1024 lds=132096 phases=3 c0=0,32,64 width=32,32,16 stride4=8 batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned cls_ok=1 n=1000 nf=80 batches=0",     "refused 4 class_only"),
    ("planned cls_ok=1 n=400 nf=96",                "phase grid=63 block=1024 lds=132096 phases=2 c0=0,64 width=64,32 stride4=20 batches_per_wg=16 keep_n=1 all_kept=1"),
    # row-class kernel: 256 / 257 workgroups (rows with the arguments / from the descriptors), and 256 whose rows did not fit the
    # arguments
    ("planned cls_ok=1 cls_groups=256",             "cls J=5 J1=3 dma=1 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 cls_groups=257",             "cls_wide J=5 J1=3 dma=1 grid=257 block=1024 lds=163840"),
    ("planned cls_ok=1 cls_groups=256 cls_by_args=0", "cls_wide J=5 J1=3 dma=1 grid=256 block=1024 lds=163840"),
    # row-class kernel: LDS-DMA with J odd / even (5, 3 above / 4), ld_z == f / ld_z > f, col_lo = 0 / col_lo > 0
    ("planned cls_ok=1 nf=80 ld_z=84",              "cls J=5 J1=3 dma=0 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 nf=80 col_lo=16 col_hi=64 ld_z=48", "cls J=3 J1=3 dma=0 grid=256 block=1024 lds=163840"),
    # row-class kernel: more columns than the plan was built for / as many
    ("planned cls_ok=1 nf=80 cls_features=64",      "phase grid=63 " + PHASE_645 + " batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned cls_ok=1 nf=80 cls_features=64 batches=0", "refused 4 class_only"),
    ("planned cls_ok=1 nf=64 n=400 cls_features=64", "cls J=4 J1=4 dma=0 grid=256 block=1024 lds=163840"),
    # column ranges: (0, 48) + (48, 80) of 80; (0, 16), (16, 36), (36, 80); on both encodings
    ("planned col_hi=48",                           "phase grid=63 block=1024 lds=123840 phases=1 c0=0 width=48 stride4=12 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned col_lo=48",                           "phase grid=63 block=1024 lds=123840 phases=1 c0=48 width=32 stride4=12 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned cls_ok=1 col_hi=48",                  "cls J=3 J1=3 dma=0 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 col_lo=48",                  "cls J=2 J1=2 dma=0 grid=256 block=1024 lds=163840"),
    ("planned col_hi=16",                           "phase grid=63 block=1024 lds=41280 phases=1 c0=0 width=16 stride4=4 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned col_lo=16 col_hi=36",                 "phase grid=63 block=1024 lds=51600 phases=1 c0=16 width=20 stride4=5 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned col_lo=36",                           "phase grid=63 block=1024 lds=154800 phases=1 c0=36 width=44 stride4=15 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned cls_ok=1 col_hi=16",                  "cls J=1 J1=1 dma=0 grid=256 block=1024 lds=163840"),
    ("planned cls_ok=1 col_lo=16 col_hi=36",        "phase grid=63 block=1024 lds=51600 phases=1 c0=16 width=20 stride4=5 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned cls_ok=1 col_lo=36",                  "phase grid=63 block=1024 lds=154800 phases=1 c0=36 width=44 stride4=15 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned cls_ok=1 col_lo=16 col_hi=36 batches=0", "refused 4 class_only"),
    # col_lo = 2 and col_hi > num_features (the entry point refuses both before it asks the route; the ladder still answers)
    ("planned col_lo=2 col_hi=50",                  "phase grid=63 block=1024 lds=123840 phases=1 c0=2 width=48 stride4=12 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned col_hi=84 ld_z=84",                   "phase grid=63 block=1024 lds=127936 phases=2 c0=0,48 width=48,36 stride4=12 batches_per_wg=16 keep_n=1 all_kept=0"),
    # column-phase kernel: keep_n 0 (one phase; two phases without room beside the table at n = 499), keep_n at the room limit of
    # 9 batches a wave (all kept / one more), all_kept false only because the launch is a partial column range, batches 1 / 0,
    # 16 / 17 (one workgroup / two), 4096 / 4097 (where the cap of 256 groups begins to bind)
    ("planned nf=48",                               "phase grid=63 block=1024 lds=123840 phases=1 c0=0 width=48 stride4=12 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned n=499",                               "phase grid=63 block=1024 lds=159680 phases=2 c0=0,64 width=64,16 stride4=20 batches_per_wg=16 keep_n=0 all_kept=0"),
    ("planned batches=36864",                       "phase grid=256 block=1024 lds=160704 phases=2 c0=0,48 width=48,32 stride4=12 batches_per_wg=144 keep_n=9 all_kept=1"),
    ("planned batches=36865",                       "phase grid=255 block=1024 lds=160704 phases=2 c0=0,48 width=48,32 stride4=12 batches_per_wg=145 keep_n=9 all_kept=0"),
    ("planned batches=100000",                      "phase grid=256 block=1024 lds=160704 phases=2 c0=0,48 width=48,32 stride4=12 batches_per_wg=391 keep_n=9 all_kept=0"),
    ("planned nf=160 col_hi=80",                    "phase grid=63 " + PHASE_645 + " batches_per_wg=16 keep_n=1 all_kept=0"),
    ("planned nf=160 col_lo=80 col_hi=160",         "phase grid=63 block=1024 lds=127936 phases=2 c0=80,128 width=48,32 stride4=12 batches_per_wg=16 keep_n=1 all_kept=0"),
    ("planned batches=1",                           "phase grid=1 " + PHASE_645 + " batches_per_wg=1 keep_n=1 all_kept=1"),
    ("planned cls_ok=1 batches=0",                  "cls J=5 J1=3 dma=1 grid=256 block=1024 lds=163840"),
    ("planned batches=16",                          "phase grid=1 " + PHASE_645 + " batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned batches=17",                          "phase grid=2 " + PHASE_645 + " batches_per_wg=9 keep_n=1 all_kept=1"),
    ("planned batches=4096",                        "phase grid=256 " + PHASE_645 + " batches_per_wg=16 keep_n=1 all_kept=1"),
    ("planned batches=4097",                        "phase grid=241 block=1024 lds=132032 phases=2 c0=0,48 width=48,32 stride4=12 batches_per_wg=17 keep_n=2 all_kept=1"),
]


def test_decoder_routes_at_every_boundary(tmp_path):
    """tests/decoder_route_host.cpp, built with g++ under AddressSanitizer + UBSan, prints the route of every case of ROUTES:
    each line equals what the earlier dispatch code chose for the same arguments."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "decoder_route_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-I", os.path.join(REPO, "gripnet_amd", "csrc"), "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "decoder_route_host.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], input="".join(case + "\n" for case, _ in ROUTES), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    got = run.stdout.splitlines()
    assert len(got) == len(ROUTES), (len(got), run.stderr[-2000:])
    wrong = [(case, want, line) for (case, want), line in zip(ROUTES, got) if line != want]
    assert not wrong, wrong
