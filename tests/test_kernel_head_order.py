"""The order of the first requests of two forward kernels, read from the built library's gfx950 code object (no GPU).

Plan memory is L2-cold at kernel start, so a scalar load from it is a long round trip, and a `s_waitcnt lgkmcnt(0)` waits
for every scalar load in flight.  What does not depend on plan data has to be requested in front of such a wait:

  * k_rgcn_pair<3, 2, 3, true> (the workload's relational kernel): the first LDS-DMA load - the att table, the bulk of the
    prologue - lies in front of the first `s_waitcnt lgkmcnt(0)` that follows a scalar load from plan memory (a scalar
    load whose base is not the kernel-argument pointer);
  * k_distmult_class<5, 3> (the workload's decoder): at most one `s_waitcnt lgkmcnt(0)` - the kernel arguments' - precedes
    the first LDS-DMA load: the class's rows come from the arguments, not from the workgroup descriptor.
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from gripnet_amd import _hip

LLVM = "/opt/rocm/lib/llvm/bin"
PAIR, CLASS = "k_rgcn_pair<3, 2, 3, true>", "k_distmult_class<5, 3>"


def disassemble(names):
    """{demangled kernel name: [(mnemonic, operands), ...]} of the named kernels, from the library's gfx950 code objects"""
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
            mangled = sorted({s for s in syms if ("k_rgcn_pair" in s or "k_distmult_class" in s) and not s.endswith(".kd")})
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
                m = re.match(r"^\s+([a-z_0-9]+)\b\s*([^/]*)", line)
                if m and current is not None:
                    out[current].append((m.group(1), m.group(2).strip()))
    return out


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.fail("llvm-objdump of the ROCm toolchain is missing")
    return disassemble({PAIR, CLASS})


def first_dma(ins):
    at = [i for i, (op, _) in enumerate(ins) if op.startswith("global_load_lds")]
    assert at, "no LDS-DMA load at all: the pattern is stale"
    return at[0]


def full_scalar_waits(ins):
    return [i for i, (op, args) in enumerate(ins) if op == "s_waitcnt" and re.search(r"lgkmcnt\(0\)", args)]


def test_pair_kernel_requests_the_att_table_in_front_of_the_plan_wait(kernels):
    assert PAIR in kernels, sorted(kernels)
    ins = kernels[PAIR]
    # the kernel-argument pointer: the base of the very first scalar load
    first = next(args for op, args in ins if op.startswith("s_load"))
    kernarg = re.search(r"s\[\d+:\d+\]", first.split(",", 1)[1]).group(0)
    plan_loads = [i for i, (op, args) in enumerate(ins)
                  if op.startswith("s_load") and re.search(r"s\[\d+:\d+\]", args.split(",", 1)[1]).group(0) != kernarg]
    assert plan_loads, "no scalar load from plan memory: the pattern is stale"
    waits = [i for i in full_scalar_waits(ins) if i > plan_loads[0]]
    assert waits, "no wait behind the plan loads: the pattern is stale"
    assert first_dma(ins) < waits[0], "the first LDS-DMA load (instruction {}) lies behind the wait for plan memory ({})".format(
        first_dma(ins), waits[0])


def test_class_kernel_requests_its_rows_behind_one_wait(kernels):
    assert CLASS in kernels, sorted(kernels)
    ins = kernels[CLASS]
    dma = first_dma(ins)
    early = [i for i in full_scalar_waits(ins) if i < dma]
    assert len(early) <= 1, "{} full scalar waits in front of the first LDS-DMA load (instruction {}): at {}".format(len(early), dma, early)
