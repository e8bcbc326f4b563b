"""The staged gene gather's structural promise, read from the built library's gfx950 code object (no GPU): between the
table fill and the end of a wave's loop there is no store to memory - a finished tile's sums are parked in LDS and written
behind the loop.  Loads and stores share one in-order counter on this hardware, so a store inside the loop is waited for
by every later wait for a load (profiles/r17_loop_waits.md).

In program order every `global_store` of k_col_gather<2>, k_col_gather<1> and k_col_gather_next<2> lies behind the last
`ds_read_b64` / `ds_read_b32`: the table gather's reads and, in the write-out, the reads of the parked sums.  The
direct-store kernels (k_col_gather_direct, k_col_gather_next_direct: plans without room for the slots) are exempt."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from gripnet_amd import _hip

LLVM = "/opt/rocm/lib/llvm/bin"
STAGED = ["k_col_gather<2>", "k_col_gather<1>", "k_col_gather_next<2>"]


def disassemble(names):
    """{demangled kernel name: [instruction mnemonic, ...]} of the named kernels, from the library's gfx950 code objects"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(_hip.library_path(), copy)       # llvm-objdump writes the bundles next to its input
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], check=True, capture_output=True)
        for obj in sorted(os.listdir(tmp)):
            if "gfx950" not in obj:
                continue
            path = os.path.join(tmp, obj)
            syms = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--syms", path], check=True, capture_output=True,
                                  text=True).stdout.split()
            mangled = sorted({s for s in syms if "k_col_gather" in s and not s.endswith(".kd")})
            if not mangled:
                continue
            dem = subprocess.run(["c++filt"] + mangled, check=True, capture_output=True, text=True).stdout.split("\n")
            short = {m: d.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "") for m, d in zip(mangled, dem)}
            wanted = [m for m in mangled if short[m] in names]
            if not wanted:
                continue
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + ",".join(wanted), path],
                                  check=True, capture_output=True, text=True).stdout
            current = None
            for line in text.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    current = short.get(m.group(1))
                    if current is not None:
                        out[current] = []
                    continue
                m = re.match(r"^\s+([a-z_0-9]+)\b", line)
                if m and current is not None:
                    out[current].append(m.group(1))
    return out


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.fail("llvm-objdump of the ROCm toolchain is missing")
    return disassemble(set(STAGED + ["k_col_gather_direct<2>"]))


@pytest.mark.parametrize("name", STAGED)
def test_no_store_in_front_of_the_last_lds_read(kernels, name):
    assert name in kernels, (name, sorted(kernels))
    ins = kernels[name]
    reads = [i for i, op in enumerate(ins) if op in ("ds_read_b64", "ds_read_b32")]
    stores = [i for i, op in enumerate(ins) if op.startswith("global_store")]
    assert len(reads) >= 64, "the table gather's reads were not found: the pattern is stale"      # 16 unrolled iterations x 4 ids
    assert stores, "no store at all: the pattern is stale"
    early = [i for i in stores if i < reads[-1]]
    assert not early, "{}: {} of {} global stores lie in front of the last LDS read (instruction {} of {})".format(
        name, len(early), len(stores), reads[-1], len(ins))


def test_the_pattern_sees_the_direct_kernels_stores(kernels):
    """The same reading of the direct-store kernel finds its stores inside the loop: the check above can fail."""
    ins = kernels["k_col_gather_direct<2>"]
    reads = [i for i, op in enumerate(ins) if op in ("ds_read_b64", "ds_read_b32")]
    stores = [i for i, op in enumerate(ins) if op.startswith("global_store")]
    assert len([i for i in stores if i < reads[-1]]) >= 16
