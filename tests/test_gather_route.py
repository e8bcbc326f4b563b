"""The gather family's route (gripnet_amd/csrc/gather_route.hpp): which kernel, lanes per row, grid, block and LDS size a
gn_graph_aggregate_f32 / _bf16 / _tail_f32 / _split_f32 call or a bare gather-reduce gets, who writes the offered split planes,
and what is refused why - one case on each side of every boundary (no GPU)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The cases as tests/gather_route_host.cpp reads them (its header lists the keys and their defaults).
# The expected lines were printed once by the dispatch chains the library held before the route was written down in one
# place (commit 1763e9b: the if-chains of gn_graph_aggregate_f32, its tail and split entries, gn_graph_aggregate_bf16,
# launch_aggregate, launch_aggregate_transform*, launch_aggregate_mfma, gn_blocked_applicable and split_source_refusal, lifted
# verbatim into a scratch program with recorders in place of the launches), not by gather_route.hpp.
# "refused N why": gn_status N (4 GN_ERR_UNSUPPORTED) and the refusal the caller words.
ROUTES = [
    # vector path: features % 4, ld_table % 4, ld_out % 4, table and output alignment - each failing alone
    ("f32 fin=16",                                                                 "wave lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=18",                                                                 "wave_scalar lpe=32 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 ld_table=18",                                                     "wave_scalar lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 ld_out=18",                                                       "wave_scalar lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 table_at=4",                                                      "wave_scalar lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 out_at=8",                                                        "wave_scalar lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    # lanes_per_row at 4 / 5, 16 / 17, 64 / 65 and 256 / 257 features (scalar where % 4 fails), and 5, 17, 65 16-byte units
    ("f32 fin=4",                                                                  "wave lpe=1 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=5",                                                                  "wave_scalar lpe=8 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=17",                                                                 "wave_scalar lpe=32 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=64",                                                                 "wave lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=65",                                                                 "wave_scalar lpe=64 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=256",                                                                "wave lpe=64 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=257",                                                                "wave_scalar lpe=64 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=20",                                                                 "wave lpe=8 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=68",                                                                 "wave lpe=32 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=260",                                                                "wave lpe=64 grid=250 block=256 lds=0 planes_by_kernel=0"),
    # LDS table: rows 65535 / 65536
    ("f32 fin=16 rows=65535 nnz=100000 table_rows=100",                            "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100",                            "lds_table lpe=4 grid=128 block=1024 lds=6464 planes_by_kernel=0"),
    # nnz = 8 * rows - 1 / 8 * rows, and nnz = 0 / 1
    ("f32 fin=16 rows=65536 nnz=524287 table_rows=100",                            "lds_table lpe=4 grid=128 block=1024 lds=6464 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=524288 table_rows=100",                            "group lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=0 table_rows=100",                                 "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=1 table_rows=100",                                 "lds_table lpe=4 grid=128 block=1024 lds=6464 planes_by_kernel=0"),
    # table bytes 131072 / the next size 16-byte rows reach (131136; 131076 is no multiple of 16)
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=2048",                           "lds_table lpe=4 grid=128 block=1024 lds=131136 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=2049",                           "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    # lpe 2 / 4 and 16 / 32
    ("f32 fin=8 rows=65536 nnz=100000 table_rows=100",                             "short_rows lpe=2 grid=512 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=64 rows=65536 nnz=100000 table_rows=100",                            "lds_table lpe=16 grid=256 block=1024 lds=25856 planes_by_kernel=0"),
    ("f32 fin=128 rows=65536 nnz=100000 table_rows=100",                           "group lpe=32 grid=8192 block=256 lds=0 planes_by_kernel=0"),
    # table_rows <= 0
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=0",                              "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=-1",                             "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    # each of coef, rowdiv, addend, bias, relu and the side copy present alone
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100 coef=1",                     "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100 rowdiv=1",                   "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100 addend=1",                   "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100 bias=1",                     "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100 relu=1",                     "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100 side=1",                     "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    # both switches
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100 lds_off=1",                  "short_rows lpe=4 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=65536 nnz=100000 table_rows=100 fast_off=1",                 "wave lpe=4 grid=2048 block=256 lds=0 planes_by_kernel=0"),
    # workgroups where the cap of 256 begins to bind (131072 / 131073 rows at lpe 4) and far beyond it
    ("f32 fin=16 rows=131072 nnz=200000 table_rows=100",                           "lds_table lpe=4 grid=256 block=1024 lds=6464 planes_by_kernel=0"),
    ("f32 fin=16 rows=131073 nnz=200000 table_rows=100",                           "lds_table lpe=4 grid=256 block=1024 lds=6464 planes_by_kernel=0"),
    ("f32 fin=16 rows=200000 nnz=200000 table_rows=100",                           "lds_table lpe=4 grid=256 block=1024 lds=6464 planes_by_kernel=0"),
    # short rows: nnz at GN_AGG_SHORT_MAX_DEG * rows, lpe 16 / 32, unknown nnz, nnz = 0, the grid's cap
    ("f32 fin=16 nnz=7999",                                                        "short_rows lpe=4 grid=16 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 nnz=8000",                                                        "group lpe=4 grid=16 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=64 nnz=1000",                                                        "short_rows lpe=16 grid=63 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=128 nnz=1000",                                                       "group lpe=32 grid=125 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 nnz=-1",                                                          "wave lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 nnz=0",                                                           "short_rows lpe=4 grid=16 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 nnz=1000 fast_off=1",                                             "wave lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=200000 nnz=200000",                                          "short_rows lpe=4 grid=2048 block=256 lds=0 planes_by_kernel=0"),
    # lane groups: nnz at GN_AGG_GROUP_MAX_DEG * rows, lpe 32 / 64, the grid ceil(rows * lpe / 256) without a cap
    ("f32 fin=16 nnz=47999",                                                       "group lpe=4 grid=16 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 nnz=48000",                                                       "wave lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=128 nnz=10000",                                                      "group lpe=32 grid=125 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=256 nnz=10000",                                                      "wave lpe=64 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=128 rows=1000000 nnz=10000000",                                      "group lpe=32 grid=125000 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 nnz=10000 fast_off=1",                                            "wave lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    # wave per row: the grid where GN_AGG_GRID begins to bind
    ("f32 fin=16 rows=8188",                                                       "wave lpe=4 grid=2047 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=8192",                                                       "wave lpe=4 grid=2048 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 rows=8193",                                                       "wave lpe=4 grid=2048 block=256 lds=0 planes_by_kernel=0"),
    # matrix cores: fin 64 / 128 / 32
    ("f32 w=1 fin=64 fout=64 rows=4096 nnz=100000",                                "mfma lpe=16 grid=64 block=1024 lds=59392 row_blocks=64 planes_by_kernel=0"),
    ("f32 w=1 fin=128 fout=128 rows=4096 nnz=100000",                              "mfma lpe=32 grid=128 block=1024 lds=132096 row_blocks=128 planes_by_kernel=0"),
    ("f32 w=1 fin=32 fout=64 rows=4096 nnz=100000",                                "refused 4 no_fused_transform"),
    # fout 64 / 80 / 128 / 144 (and 72), fout < fin
    ("f32 w=1 fin=64 fout=80 rows=4096 nnz=100000",                                "mfma lpe=16 grid=64 block=1024 lds=65536 row_blocks=64 planes_by_kernel=0"),
    ("f32 w=1 fin=64 fout=128 rows=4096 nnz=100000",                               "mfma lpe=16 grid=64 block=1024 lds=83968 row_blocks=64 planes_by_kernel=0"),
    ("f32 w=1 fin=64 fout=144 rows=4096 nnz=100000",                               "refused 4 no_fused_transform"),
    ("f32 w=1 fin=64 fout=72 rows=4096 nnz=100000",                                "refused 4 no_fused_transform"),
    ("f32 w=1 fin=128 fout=64 rows=4096 nnz=100000",                               "refused 4 no_fused_transform"),
    # rows 4095 / 4096, nnz at the boundary and unknown
    ("f32 w=1 fin=64 fout=64 rows=4095 nnz=100000",                                "refused 4 no_fused_transform"),
    ("f32 w=1 fin=64 fout=64 rows=4096 nnz=196607",                                "mfma lpe=16 grid=64 block=1024 lds=59392 row_blocks=64 planes_by_kernel=0"),
    ("f32 w=1 fin=64 fout=64 rows=4096 nnz=196608",                                "refused 4 no_fused_transform"),
    ("f32 w=1 fin=64 fout=64 rows=4096 nnz=-1",                                    "refused 4 no_fused_transform"),
    # an unaligned table, fast paths off, planes offered
    ("f32 w=1 fin=64 fout=64 rows=4096 nnz=100000 table_at=4",                     "refused 4 no_fused_transform"),
    ("f32 w=1 fin=64 fout=64 rows=4096 nnz=100000 ld_table=66",                    "refused 4 no_fused_transform"),
    ("f32 w=1 fin=64 fout=64 rows=4096 nnz=100000 fast_off=1",                     "refused 4 no_fused_transform"),
    ("f32 w=1 fin=64 fout=64 rows=4096 nnz=100000 planes=1",                       "mfma lpe=16 grid=64 block=1024 lds=59392 row_blocks=64 planes_by_kernel=0"),
    # the grid as row blocks at lpe 16; as min(row blocks, compute units) at lpe 32, on both sides
    ("f32 w=1 fin=64 fout=64 rows=4097 nnz=100000",                                "mfma lpe=16 grid=65 block=1024 lds=59392 row_blocks=65 planes_by_kernel=0"),
    ("f32 w=1 fin=64 fout=64 rows=100000 nnz=1000000 cus=64",                      "mfma lpe=16 grid=1563 block=1024 lds=59392 row_blocks=1563 planes_by_kernel=0"),
    ("f32 w=1 fin=128 fout=128 rows=4096 nnz=100000 cus=64",                       "mfma lpe=32 grid=64 block=1024 lds=132096 row_blocks=128 planes_by_kernel=0"),
    ("f32 w=1 fin=128 fout=128 rows=8192 nnz=100000 cus=256",                      "mfma lpe=32 grid=256 block=1024 lds=132096 row_blocks=256 planes_by_kernel=0"),
    ("f32 w=1 fin=128 fout=128 rows=8193 nnz=100000 cus=256",                      "mfma lpe=32 grid=256 block=1024 lds=132096 row_blocks=257 planes_by_kernel=0"),
    # fused transform: the five admitted width pairs, 16 -> 32 refused, 16 -> 16 without the quad kernel
    ("f32 w=1 fin=16 fout=16",                                                     "transform_quad lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=32 fout=16",                                                     "transform lpe=8 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=64 fout=16",                                                     "transform lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=32 fout=32",                                                     "transform lpe=8 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=64 fout=32",                                                     "transform lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=32",                                                     "refused 4 no_fused_transform"),
    ("f32 w=1 fin=16 fout=16 quad_off=1",                                          "transform lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=64 fout=16 rows=8193 nnz=10000",                                 "transform lpe=16 grid=2048 block=256 lds=0 planes_by_kernel=0"),
    # who writes the planes: quad, mfma (above), blocked (below) and plain do not; the shuffle, tail and split forms do
    ("f32 w=1 fin=16 fout=16 planes=1",                                            "transform_quad lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 planes=1 quad_off=1",                                 "transform lpe=4 grid=250 block=256 lds=0 planes_by_kernel=1"),
    ("f32 w=1 fin=32 fout=16 planes=1",                                            "transform lpe=8 grid=250 block=256 lds=0 planes_by_kernel=1"),
    ("f32 fin=16 planes=1",                                                        "wave lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=16 nnz=1000 planes=1",                                               "short_rows lpe=4 grid=16 block=256 lds=0 planes_by_kernel=0"),
    ("tail w=1 fin=64 fout=16 planes=1",                                           "transform_tail lpe=16 grid=250 block=256 lds=0 planes_by_kernel=1"),
    ("split w=1 fin=64 fout=16 planes=1",                                          "transform_split lpe=16 grid=250 block=256 lds=0 planes_by_kernel=1"),
    # an unaligned table, fast paths off
    ("f32 w=1 fin=32 fout=16 table_at=8",                                          "refused 4 no_fused_transform"),
    ("f32 w=1 fin=32 fout=16 ld_table=34",                                         "refused 4 no_fused_transform"),
    ("f32 w=1 fin=32 fout=16 fast_off=1",                                          "refused 4 no_fused_transform"),
    # tail: 64 -> 16 admitted; refused for 32 -> 16, 64 -> 32, fast paths off, unaligned tail_w, tail_b or table
    ("tail w=1 fin=64 fout=16",                                                    "transform_tail lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("tail w=1 fin=32 fout=16",                                                    "refused 4 tail_operands"),
    ("tail w=1 fin=64 fout=32",                                                    "refused 4 tail_operands"),
    ("tail w=1 fin=64 fout=16 fast_off=1",                                         "refused 4 tail_operands"),
    ("tail w=1 fin=64 fout=16 tail_w_at=4",                                        "refused 4 tail_operands"),
    ("tail w=1 fin=64 fout=16 tail_b_at=8",                                        "refused 4 tail_operands"),
    ("tail w=1 fin=64 fout=16 table_at=4",                                         "refused 4 tail_operands"),
    ("tail w=1 fin=64 fout=16 ld_table=66",                                        "refused 4 tail_operands"),
    ("tail w=1 fin=64 fout=16 rows=8193",                                          "transform_tail lpe=16 grid=2048 block=256 lds=0 planes_by_kernel=0"),
    # split source: head_cols 16 / 32 / 48 admitted, 0 / 8 / 64 refused
    ("split w=1 fin=64 fout=16 head_cols=16",                                      "transform_split lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("split w=1 fin=64 fout=16 head_cols=32",                                      "transform_split lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("split w=1 fin=64 fout=16 head_cols=48",                                      "transform_split lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("split w=1 fin=64 fout=16 head_cols=0",                                       "refused 4 split_head_cols"),
    ("split w=1 fin=64 fout=16 head_cols=8",                                       "refused 4 split_head_cols"),
    ("split w=1 fin=64 fout=16 head_cols=64",                                      "refused 4 split_head_cols"),
    # ld_tail 2^31 - 4 / 2^31, the same for the head, ld_head < head_cols, a short ld_tail
    ("split w=1 fin=64 fout=16 ld_tail=2147483644",                                "transform_split lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("split w=1 fin=64 fout=16 ld_tail=2147483648",                                "refused 4 split_ld_31_bits"),
    ("split w=1 fin=64 fout=16 ld_table=2147483644",                               "transform_split lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("split w=1 fin=64 fout=16 ld_table=2147483648",                               "refused 4 split_ld_31_bits"),
    ("split w=1 fin=64 fout=16 head_cols=32 ld_table=28",                          "refused 4 split_ld_short"),
    ("split w=1 fin=64 fout=16 head_cols=16 ld_tail=44",                           "refused 4 split_ld_short"),
    # each alignment, a missing table, fast paths off, other widths
    ("split w=1 fin=64 fout=16 table_at=4",                                        "refused 4 split_alignment"),
    ("split w=1 fin=64 fout=16 tail_at=4",                                         "refused 4 split_alignment"),
    ("split w=1 fin=64 fout=16 head=0",                                            "refused 4 split_alignment"),
    ("split w=1 fin=64 fout=16 tail=0",                                            "refused 4 split_alignment"),
    ("split w=1 fin=64 fout=16 ld_table=18",                                       "refused 4 split_ld_multiple"),
    ("split w=1 fin=64 fout=16 ld_tail=50",                                        "refused 4 split_ld_multiple"),
    ("split w=1 fin=64 fout=16 fast_off=1",                                        "refused 4 split_fast_off"),
    ("split w=1 fin=32 fout=16",                                                   "refused 4 split_widths"),
    ("split w=1 fin=64 fout=32",                                                   "refused 4 split_widths"),
    ("split w=1 fin=64 fout=16 rows=8193",                                         "transform_split lpe=16 grid=2048 block=256 lds=0 planes_by_kernel=0"),
    # blocked: blk_ok on / off, the switch, fast paths off
    ("f32 w=1 fin=16 fout=16 blk_ok=1 blk_cols=16",                                "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=0 blk_cols=16",                                "transform_quad lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 blk_cols=16 blk_off=1",                      "transform_quad lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 blk_cols=16 fast_off=1",                     "refused 4 no_fused_transform"),
    ("f32 fin=16 blk_ok=1 blk_cols=16 fast_off=1",                                 "wave lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 blk_cols=16 planes=1",                       "blocked planes_by_kernel=0"),
    # cw 1 and 2 against ld_out, output and bias residues
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=2 ld_out=17",                             "transform_quad lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=1 ld_out=17",                             "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=2 out_at=4",                              "transform_quad lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=1 out_at=4",                              "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=2 out_at=8",                              "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=2 bias=1 bias_at=4",                      "transform_quad lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=1 bias=1 bias_at=4",                      "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=2 bias=1 bias_at=8",                      "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 cw=2 bias=0 bias_at=4",                      "blocked planes_by_kernel=0"),
    # fout 16 / 32 / 48 against blk_cols 16 / 32
    ("f32 w=1 fin=32 fout=32 blk_ok=1 blk_cols=16",                                "transform lpe=8 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=32 fout=32 blk_ok=1 blk_cols=32",                                "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=32 fout=16 blk_ok=1 blk_cols=32",                                "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=64 fout=48 blk_ok=1 blk_cols=32",                                "refused 4 no_fused_transform"),
    ("f32 w=1 fin=16 fout=32 blk_ok=1 blk_cols=32",                                "blocked planes_by_kernel=0"),
    # fin in and out of {16, 32, 64} with a weight; an unaligned weight or table
    ("f32 w=1 fin=64 fout=16 blk_ok=1",                                            "blocked planes_by_kernel=0"),
    ("f32 w=1 fin=48 fout=16 blk_ok=1",                                            "refused 4 no_fused_transform"),
    ("f32 w=1 fin=128 fout=16 blk_ok=1",                                           "refused 4 no_fused_transform"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 w_at=4",                                     "transform_quad lpe=4 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 table_at=4",                                 "refused 4 no_fused_transform"),
    ("f32 w=1 fin=16 fout=16 blk_ok=1 ld_table=18",                                "refused 4 no_fused_transform"),
    # without a weight: fin == fout is the gathered row; fin != fout only reaches the query
    ("f32 fin=16 blk_ok=1",                                                        "blocked planes_by_kernel=0"),
    ("f32 fin=32 blk_ok=1 blk_cols=16",                                            "wave lpe=8 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("f32 fin=48 blk_ok=1",                                                        "wave lpe=16 grid=250 block=256 lds=0 planes_by_kernel=0"),
    ("q_blocked fin=16 fout=16 blk_ok=1",                                          "blocked_applicable 1"),
    ("q_blocked fin=16 fout=32 blk_ok=1",                                          "blocked_applicable 0"),
    ("q_blocked w=1 fin=16 fout=32 blk_ok=1",                                      "blocked_applicable 1"),
    ("q_blocked w=1 fin=16 fout=32 blk_ok=1 blk_off=1",                            "blocked_applicable 0"),
    ("q_blocked w=1 fin=64 fout=16 blk_ok=1 out_at=4",                             "blocked_applicable 0"),
    # bf16: rows 4095 / 4096, nnz at the boundary, features 256 / 264 (lpe 32 / 64), fast paths off
    ("bf16 fin=64 rows=4095 nnz=10000",                                            "bf16_wave lpe=8 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("bf16 fin=64 rows=4096 nnz=10000",                                            "bf16_group lpe=8 grid=128 block=256 lds=0 planes_by_kernel=0"),
    ("bf16 fin=64 rows=4096 nnz=196607",                                           "bf16_group lpe=8 grid=128 block=256 lds=0 planes_by_kernel=0"),
    ("bf16 fin=64 rows=4096 nnz=196608",                                           "bf16_wave lpe=8 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("bf16 fin=256 rows=4096 nnz=10000",                                           "bf16_group lpe=32 grid=512 block=256 lds=0 planes_by_kernel=0"),
    ("bf16 fin=264 rows=4096 nnz=10000",                                           "bf16_wave lpe=64 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("bf16 fin=64 rows=4096 nnz=10000 fast_off=1",                                 "bf16_wave lpe=8 grid=1024 block=256 lds=0 planes_by_kernel=0"),
    ("bf16 fin=64 rows=8193 nnz=1000000",                                          "bf16_wave lpe=8 grid=2048 block=256 lds=0 planes_by_kernel=0"),
    # gn_transform_fusable / gn_graph_transform_fusable
    ("fusable fin=16 fout=16",                                                     "transform_fusable 1 graph_transform_fusable 1"),
    ("fusable fin=16 fout=32",                                                     "transform_fusable 0 graph_transform_fusable 0"),
    ("fusable fin=64 fout=32",                                                     "transform_fusable 1 graph_transform_fusable 1"),
    ("fusable fin=64 fout=64 rows=4096 nnz=1000",                                  "transform_fusable 0 graph_transform_fusable 1"),
    ("fusable fin=64 fout=64 rows=4095 nnz=1000",                                  "transform_fusable 0 graph_transform_fusable 0"),
    ("fusable fin=128 fout=128 rows=4096 nnz=196608",                              "transform_fusable 0 graph_transform_fusable 0"),
    ("fusable fin=64 fout=64 rows=4096 nnz=1000 fast_off=1",                       "transform_fusable 0 graph_transform_fusable 0"),
    ("fusable fin=16 fout=16 fast_off=1",                                          "transform_fusable 0 graph_transform_fusable 0"),
]


def test_gather_routes_at_every_boundary(tmp_path):
    """tests/gather_route_host.cpp, built with g++ under AddressSanitizer + UBSan, prints the route of every case of ROUTES:
    each line equals what the earlier dispatch chains chose for the same arguments."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "gather_route_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-I", os.path.join(REPO, "gripnet_amd", "csrc"), "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "gather_route_host.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], input="".join(case + "\n" for case, _ in ROUTES), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    got = run.stdout.splitlines()
    assert len(got) == len(ROUTES), (len(got), run.stderr[-2000:])
    wrong = [(case, want, line) for (case, want), line in zip(ROUTES, got) if line != want]
    assert not wrong, wrong
