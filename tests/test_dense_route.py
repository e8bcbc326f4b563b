"""The dense products' route (gripnet_amd/csrc/dense_route.hpp): which kernel, tile, grid and LDS size a gn_gemm_f32 /
gn_xtg_f32 call gets, one case on each side of every boundary (no GPU)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The cases as tests/dense_route_host.cpp reads them:
#   gemm m n k batch flags a_rows a_vec_ok c_offset addend disable_fast batch_open compute_units
#        flags: RELU 1, ARITH_FAST 2, B_TRANSPOSED 4, ACCUMULATE 8, A_TRANSPOSED 16, JOIN_BATCH 32, OUT_BF16 64, SPLIT_KERNEL 128
#   xtg  m k1 k2 flags workspace_offset disable_fast batch_open compute_units        flags: TICKET_ZEROED 1, JOIN_BATCH 2
#   wide m k1 k2 disable_fast
# The expected lines were printed by the dispatch chain that gemm.hip held before the route was written down once (commit
# e8ac882: the if-chains of gn_gemm_addend_f32 and gn_xtg_f32, xtg_slices, gn_xtg_wide_supported, behind recorders in place
# of the launches), not by dense_route.hpp.  "refused N": gn_status N (1 GN_ERR_INVALID_ARG, 4 GN_ERR_UNSUPPORTED).
ROUTES = [
    # deep and narrow: m = 64 / 65, n = 32 / 33, k = 255 / 256
    ("gemm 64 200 300 1 0 0 1 0 0 0 0 256",                 "deep mt=4 nt=1 grid=1,13"),
    ("gemm 65 200 300 1 0 0 1 0 0 0 0 256",                 "general grid=2,4,1"),
    ("gemm 200 32 300 1 0 0 1 0 0 0 0 256",                 "deep mt=1 nt=2 grid=13,1"),
    ("gemm 200 33 300 1 0 0 1 0 0 0 0 256",                 "general grid=4,1,1"),
    ("gemm 64 200 255 1 0 0 1 0 0 0 0 256",                 "general grid=1,4,1"),
    ("gemm 64 200 256 1 0 0 1 0 0 0 0 256",                 "deep mt=4 nt=1 grid=1,13"),
    # its four tile shapes
    ("gemm 16 200 256 1 0 0 1 0 0 0 0 256",                 "deep mt=1 nt=1 grid=1,13"),
    ("gemm 17 200 256 1 0 0 1 0 0 0 0 256",                 "deep mt=2 nt=1 grid=1,13"),
    ("gemm 32 200 256 1 0 0 1 0 0 0 0 256",                 "deep mt=2 nt=1 grid=1,13"),
    ("gemm 33 200 256 1 0 0 1 0 0 0 0 256",                 "deep mt=4 nt=1 grid=1,13"),
    ("gemm 200 16 256 1 0 0 1 0 0 0 0 256",                 "deep mt=1 nt=1 grid=13,1"),
    ("gemm 200 17 256 1 0 0 1 0 0 0 0 256",                 "deep mt=1 nt=2 grid=13,1"),
    # tall-skinny fp32, B in LDS: m = 255 / 256, k = 256 / 257 (65,536 / 69,632 bytes)
    ("gemm 255 64 48 1 0 0 1 0 0 0 0 256",                  "general grid=4,1,1"),
    ("gemm 256 64 48 1 0 0 1 0 0 0 0 256",                  "lds row_tiles=16 grid=4,1 lds=12288"),
    ("gemm 300 64 256 1 0 0 1 0 0 0 0 256",                 "lds row_tiles=19 grid=5,1 lds=65536"),
    ("gemm 300 64 257 1 0 0 1 0 0 0 0 256",                 "general grid=5,1,1"),
    ("gemm 100000 200 48 1 0 0 1 0 0 0 0 256",              "lds row_tiles=6250 grid=1024,4 lds=12288"),
    # split: m = 2047 / 2048, k = 32 / 31 / 48 / 64
    ("gemm 2047 64 128 1 0 0 1 0 0 0 0 256",                "lds row_tiles=128 grid=32,1 lds=32768"),
    ("gemm 2048 64 128 1 0 0 1 0 0 0 0 256",                "split terms=3 ct=4 slab=4 ch=4 row_tiles=128 grid=128,1 lds=49152 bf16=0"),
    ("gemm 2048 64 32 1 0 0 1 0 0 0 0 256",                 "split terms=3 ct=4 slab=1 ch=1 row_tiles=128 grid=128,1 lds=12288 bf16=0"),
    ("gemm 2048 64 31 1 0 0 1 0 0 0 0 256",                 "lds row_tiles=128 grid=32,1 lds=8192"),
    ("gemm 2048 64 48 1 0 0 1 0 0 0 0 256",                 "lds row_tiles=128 grid=32,1 lds=12288"),
    ("gemm 2048 64 64 1 0 0 1 0 0 0 0 256",                 "split terms=3 ct=4 slab=2 ch=2 row_tiles=128 grid=128,1 lds=24576 bf16=0"),
    # n = 64 / 65 (ct 4 / 8), fast off and on
    ("gemm 2048 64 128 1 2 0 1 0 0 0 0 256",                "split terms=2 ct=4 slab=4 ch=4 row_tiles=128 grid=128,1 lds=32768 bf16=0"),
    ("gemm 2048 65 128 1 0 0 1 0 0 0 0 256",                "split terms=3 ct=8 slab=4 ch=4 row_tiles=128 grid=128,1 lds=98304 bf16=0"),
    ("gemm 2048 65 128 1 2 0 1 0 0 0 0 256",                "split terms=2 ct=8 slab=4 ch=4 row_tiles=128 grid=128,1 lds=65536 bf16=0"),
    # k = 256: n = 128 (slab 6 < 8 chunks: CH 0), n = 64 (slab 8: CH 8), n = 128 fast (slab 8 but ct 8: CH 0); a deeper K in slabs
    ("gemm 2048 128 256 1 0 0 1 0 0 0 0 256",               "split terms=3 ct=8 slab=6 ch=0 row_tiles=128 grid=128,1 lds=147456 bf16=0"),
    ("gemm 2048 64 256 1 0 0 1 0 0 0 0 256",                "split terms=3 ct=4 slab=8 ch=8 row_tiles=128 grid=128,1 lds=98304 bf16=0"),
    ("gemm 2048 128 256 1 2 0 1 0 0 0 0 256",               "split terms=2 ct=8 slab=8 ch=0 row_tiles=128 grid=128,1 lds=131072 bf16=0"),
    ("gemm 2048 64 512 1 0 0 1 0 0 0 0 256",                "split terms=3 ct=4 slab=8 ch=0 row_tiles=128 grid=128,1 lds=98304 bf16=0"),
    # fewer row tiles than compute units; fewer compute units
    ("gemm 2048 64 128 1 0 0 1 0 0 0 0 64",                 "split terms=3 ct=4 slab=4 ch=4 row_tiles=128 grid=64,1 lds=49152 bf16=0"),
    ("gemm 5000 64 128 1 0 0 1 0 0 0 0 256",                "split terms=3 ct=4 slab=4 ch=4 row_tiles=313 grid=256,1 lds=49152 bf16=0"),
    # GN_GEMM_SPLIT_KERNEL at m = 100
    ("gemm 100 64 64 1 128 0 1 0 0 0 0 256",                "split terms=3 ct=4 slab=2 ch=2 row_tiles=7 grid=7,1 lds=24576 bf16=0"),
    ("gemm 100 64 48 1 128 0 1 0 0 0 0 256",                "general grid=2,1,1"),
    # batch = 2, a row gather, a_vec_ok = 0
    ("gemm 5000 64 128 2 0 0 1 0 0 0 0 256",                "general grid=79,1,2"),
    ("gemm 64 200 300 2 0 0 1 0 0 0 0 256",                 "general grid=1,4,2"),
    ("gemm 5000 64 128 1 0 1 1 0 0 0 0 256",                "lds row_tiles=313 grid=79,1 lds=32768"),
    ("gemm 64 200 300 1 0 1 1 0 0 0 0 256",                 "general grid=1,4,1"),
    ("gemm 5000 64 128 1 0 0 0 0 0 0 0 256",                "lds row_tiles=313 grid=79,1 lds=32768"),
    # A transposed: (64, 200), (200, 32), (65, 33) refused; shallow k; batch 2 refused
    ("gemm 64 200 10 1 16 0 1 0 0 0 0 256",                 "deep mt=4 nt=1 grid=1,13"),
    ("gemm 200 32 10 1 16 0 1 0 0 0 0 256",                 "deep mt=1 nt=2 grid=13,1"),
    ("gemm 65 33 10 1 16 0 1 0 0 0 0 256",                  "refused 1"),
    ("gemm 64 200 10 2 16 0 1 0 0 0 0 256",                 "refused 1"),
    ("gemm 2048 32 256 1 16 0 1 0 0 0 0 256",               "deep mt=1 nt=2 grid=128,1"),
    # the same shapes under GN_DISABLE_FAST=1
    ("gemm 64 200 300 1 0 0 1 0 0 1 0 256",                 "general grid=1,4,1"),
    ("gemm 256 64 48 1 0 0 1 0 0 1 0 256",                  "general grid=4,1,1"),
    ("gemm 2048 64 128 1 0 0 1 0 0 1 0 256",                "general grid=32,1,1"),
    ("gemm 64 200 10 1 16 0 1 0 0 1 0 256",                 "deep mt=4 nt=1 grid=1,13"),
    ("gemm 200 32 10 1 16 0 1 0 0 1 0 256",                 "deep mt=1 nt=2 grid=13,1"),
    ("gemm 65 33 10 1 16 0 1 0 0 1 0 256",                  "refused 1"),
    # a shape of the split kernel stays off the deep kernel even where the split kernel does not run
    ("gemm 2048 32 256 1 0 0 1 0 0 0 0 256",                "split terms=3 ct=4 slab=8 ch=8 row_tiles=128 grid=128,1 lds=98304 bf16=0"),
    ("gemm 2048 32 256 1 0 0 1 0 0 1 0 256",                "general grid=32,1,1"),
    ("gemm 2048 32 256 1 0 1 1 0 0 0 0 256",                "lds row_tiles=128 grid=32,1 lds=65536"),
    ("gemm 2048 32 256 2 0 0 1 0 0 0 0 256",                "general grid=32,1,2"),
    ("gemm 2048 32 288 1 0 0 0 0 0 0 0 256",                "deep mt=1 nt=2 grid=128,1"),
    # GN_GEMM_OUT_BF16: accepted (16- and 8-byte aligned c), and refused for each reason
    ("gemm 2048 64 128 1 64 0 1 0 0 0 0 256",               "split terms=3 ct=4 slab=4 ch=4 row_tiles=128 grid=128,1 lds=49152 bf16=1"),
    ("gemm 2048 64 128 1 64 0 1 8 0 0 0 256",               "split terms=3 ct=4 slab=4 ch=4 row_tiles=128 grid=128,1 lds=49152 bf16=1"),
    ("gemm 2047 64 128 1 64 0 1 0 0 0 0 256",               "refused 4"),
    ("gemm 100 64 128 1 192 0 1 0 0 0 0 256",               "refused 4"),
    ("gemm 2048 64 128 1 64 1 1 0 0 0 0 256",               "refused 4"),
    ("gemm 2048 64 48 1 64 0 1 0 0 0 0 256",                "refused 4"),
    ("gemm 2048 64 128 1 64 0 0 0 0 0 0 256",               "refused 4"),
    ("gemm 2048 64 128 1 64 0 1 0 0 1 0 256",               "refused 4"),
    ("gemm 2048 66 128 1 64 0 1 0 0 0 0 256",               "refused 4"),
    ("gemm 2048 64 128 1 64 0 1 4 0 0 0 256",               "refused 4"),
    ("gemm 2048 64 128 1 72 0 1 0 0 0 0 256",               "refused 4"),
    ("gemm 2048 64 128 1 64 0 1 0 1 0 0 256",               "refused 4"),
    ("gemm 2048 64 128 1 80 0 1 0 0 0 0 256",               "refused 4"),
    ("gemm 2048 64 128 2 64 0 1 0 0 0 0 256",               "refused 4"),
    # batch = 65,535 / 65,536
    ("gemm 64 32 16 65535 0 0 1 0 0 0 0 256",               "general grid=1,1,65535"),
    ("gemm 64 32 16 65536 0 0 1 0 0 0 0 256",               "refused 4"),
    # join-batch on each route (and the flag without an open batch)
    ("gemm 64 200 300 1 32 0 1 0 0 0 1 256",                "deep queued mt=4 nt=1 gx=1 blocks=13 lds=65536"),
    ("gemm 200 32 10 1 48 0 1 0 0 0 1 256",                 "deep queued mt=1 nt=2 gx=13 blocks=13 lds=32768"),
    ("gemm 200 17 256 1 32 0 1 0 0 0 1 256",                "deep queued mt=1 nt=2 gx=13 blocks=13 lds=32768"),
    ("gemm 256 64 48 1 32 0 1 0 0 0 1 256",                 "lds queued row_tiles=16 gx=1 blocks=1 lds=12288"),
    ("gemm 100000 200 48 1 32 0 1 0 0 0 1 256",             "lds queued row_tiles=6250 gx=256 blocks=1024 lds=12288"),
    ("gemm 256 64 48 1 32 1 1 0 0 0 1 256",                 "lds row_tiles=16 grid=4,1 lds=12288"),
    ("gemm 2048 64 128 1 32 0 1 0 0 0 1 256",               "split terms=3 ct=4 slab=4 ch=4 row_tiles=128 grid=128,1 lds=49152 bf16=0"),
    ("gemm 255 64 48 1 32 0 1 0 0 0 1 256",                 "general grid=4,1,1"),
    ("gemm 64 200 300 1 32 0 1 0 0 0 0 256",                "deep mt=4 nt=1 grid=1,13"),
    ("gemm 256 64 48 1 32 0 1 0 0 0 0 256",                 "lds row_tiles=16 grid=4,1 lds=12288"),
    # gn_xtg_wide_supported
    ("wide 4095 128 32 0",                                  "wide_supported 0"),
    ("wide 4096 128 32 0",                                  "wide_supported 1"),
    ("wide 4096 64 32 0",                                   "wide_supported 0"),
    ("wide 4096 64 64 0",                                   "wide_supported 1"),
    ("wide 4096 256 128 0",                                 "wide_supported 1"),
    ("wide 4096 192 32 0",                                  "wide_supported 0"),
    ("wide 4096 100 32 0",                                  "wide_supported 0"),
    ("wide 4096 128 32 1",                                  "wide_supported 0"),
    # wide x^T g
    ("xtg 4096 128 32 1 0 0 0 256",                         "wide ti=2 tj=1 wpt=8 slices=16 lds=131072"),
    ("xtg 4096 64 64 1 0 0 0 256",                          "wide ti=1 tj=2 wpt=8 slices=16 lds=131072"),
    ("xtg 4096 256 128 1 0 0 0 256",                        "wide ti=4 tj=4 wpt=1 slices=128 lds=0"),
    ("xtg 100000 256 128 1 0 0 0 256",                      "wide ti=4 tj=4 wpt=1 slices=256 lds=0"),
    ("xtg 100000 256 128 1 0 0 0 64",                       "wide ti=4 tj=4 wpt=1 slices=64 lds=0"),
    ("xtg 100000 128 32 3 0 0 1 256",                       "wide ti=2 tj=1 wpt=8 slices=256 lds=131072"),
    # k1 * k2 = 4096 / 4097 when not wide; a wide shape with too few rows; 192 x 32
    ("xtg 100 64 64 1 0 0 0 256",                           "partial slices=7 lds=66048"),
    ("xtg 100 4097 1 1 0 0 0 256",                          "refused 4"),
    ("xtg 4095 128 32 1 0 0 0 256",                         "partial slices=256 lds=82432"),
    ("xtg 4095 128 64 1 0 0 0 256",                         "refused 4"),
    ("xtg 4096 192 32 1 0 0 0 256",                         "refused 4"),
    # one-launch x^T g at (16, 16), (64, 32), (49, 17)
    ("xtg 600 16 16 1 0 0 0 256",                           "mfma mt=1 nt=1 slices=2 lds=16384"),
    ("xtg 600 64 32 1 0 0 0 256",                           "mfma mt=4 nt=2 slices=2 lds=131072"),
    ("xtg 600 49 17 1 0 0 0 256",                           "mfma mt=4 nt=2 slices=2 lds=131072"),
    ("xtg 600 65 32 1 0 0 0 256",                           "partial slices=38 lds=50176"),
    ("xtg 600 64 33 1 0 0 0 256",                           "partial slices=38 lds=50176"),
    # xtg_slices at ceil_div(m, 512) = 1, 32, 40, 41, 128, 129
    ("xtg 1 64 32 1 0 0 0 256",                             "mfma mt=4 nt=2 slices=1 lds=131072"),
    ("xtg 16384 64 32 1 0 0 0 256",                         "mfma mt=4 nt=2 slices=32 lds=131072"),
    ("xtg 20480 64 32 1 0 0 0 256",                         "mfma mt=4 nt=2 slices=32 lds=131072"),
    ("xtg 20992 64 32 1 0 0 0 256",                         "mfma mt=4 nt=2 slices=41 lds=131072"),
    ("xtg 65536 64 32 1 0 0 0 256",                         "mfma mt=4 nt=2 slices=128 lds=131072"),
    ("xtg 66048 64 32 1 0 0 0 256",                         "mfma mt=4 nt=2 slices=128 lds=131072"),
    # no GN_XTG_TICKET_ZEROED, a misaligned workspace, GN_DISABLE_FAST=1, no rows
    ("xtg 600 64 32 0 0 0 0 256",                           "partial slices=38 lds=49664"),
    ("xtg 600 64 32 1 2 0 0 256",                           "partial slices=38 lds=49664"),
    ("xtg 600 64 32 1 0 1 0 256",                           "partial slices=38 lds=49664"),
    ("xtg 0 64 32 1 0 0 0 256",                             "partial slices=1 lds=49664"),
    ("xtg 100000 64 32 0 0 0 0 256",                        "partial slices=256 lds=49664"),
    # join-batch
    ("xtg 600 64 32 3 0 0 1 256",                           "mfma queued mt=4 nt=2 blocks=2 lds=131072"),
    ("xtg 600 64 32 3 0 0 0 256",                           "mfma mt=4 nt=2 slices=2 lds=131072"),
    ("xtg 600 64 32 2 0 0 1 256",                           "partial slices=38 lds=49664"),
]


def test_dense_routes_at_every_boundary(tmp_path):
    """tests/dense_route_host.cpp, built with g++ under AddressSanitizer + UBSan, prints the route of every case of ROUTES:
    each line equals what the earlier dispatch chain chose for the same arguments."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "dense_route_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-I", os.path.join(REPO, "gripnet_amd", "csrc"), "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "dense_route_host.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], input="".join(case + "\n" for case, _ in ROUTES), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    got = run.stdout.splitlines()
    assert len(got) == len(ROUTES), (len(got), run.stderr[-2000:])
    wrong = [(case, want, line) for (case, want), line in zip(ROUTES, got) if line != want]
    assert not wrong, wrong
