"""The external layer's request round, read from the built library's gfx950 code object (no GPU): in the 16-lanes-per-neighbour
instantiations of aggregate_transform (aggregate.hip) the sixteen 16-byte row loads of a batch stand, in program order, in front
of the first vector-memory wait that follows the first of them.  A wait between them makes the loads behind it a second
dependent round trip of a latency-bound launch: the compiler put one behind EVERY load while each sat under its own
`if (idx < cnt)` (profiles/r26_epilogue_and_rows.md).

Only the order of loads and waits is inspected."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from gripnet_amd import _hip

LLVM = "/opt/rocm/lib/llvm/bin"
WIDE = ["k_aggregate_transform_split<16>", "k_aggregate_transform<16, 16>", "k_aggregate_transform<16, 32>", "k_aggregate_transform_tail"]
NARROW = "k_aggregate_transform<8, 16>"
BATCH = 16


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
            mangled = sorted({s for s in syms if "k_aggregate_transform" in s and not s.endswith(".kd")})
            if not mangled:
                continue
            dem = subprocess.run(["c++filt"] + mangled, check=True, capture_output=True, text=True).stdout.split("\n")
            short = {m: d.replace("(anonymous namespace)::", "").replace("gn::", "").split("(")[0].replace("void ", "")
                     for m, d in zip(mangled, dem)}
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
    return disassemble(set(WIDE + [NARROW]))


def longest_run_of_row_loads(ins):
    """The most 16-byte global loads between two vector-memory waits (the first wait behind a load ends its run), and where."""
    best, run, start, at = 0, 0, None, None
    for i, (op, args) in enumerate(ins):
        if op == "global_load_dwordx4":
            start = i if run == 0 else start
            run += 1
        elif op == "s_waitcnt" and "vmcnt" in args and run:
            if run > best:
                best, at = run, start
            run = 0
    return best, at


@pytest.mark.parametrize("name", WIDE)
def test_a_batch_of_rows_is_one_request_round(kernels, name):
    assert name in kernels, (name, sorted(kernels))
    ins = kernels[name]
    loads = [i for i, (op, _) in enumerate(ins) if op == "global_load_dwordx4"]
    assert len(loads) >= BATCH, "the row loads were not found: the pattern is stale"
    # the row loop's loads are the LAST sixteen of the kernel (the tail variant reads W2 with sixteen more, up front)
    batch = loads[-BATCH:]
    waits = [i for i, (op, args) in enumerate(ins) if op == "s_waitcnt" and "vmcnt" in args and i > batch[0]]
    assert waits, "no vector-memory wait behind the row loads: the pattern is stale"
    late = [i for i in batch if i > waits[0]]
    assert not late, "{}: {} of the {} row loads lie behind the first wait (instruction {}) that follows the first of them ({})".format(
        name, len(late), BATCH, waits[0], batch[0])


def test_the_pattern_sees_a_wait_between_loads(kernels):
    """The same reading of a narrow instantiation (two groups in flight, each load under its own condition) finds no run of
    sixteen loads in front of a wait: the check above can fail."""
    best, _ = longest_run_of_row_loads(kernels[NARROW])
    assert 1 <= best < BATCH, best
