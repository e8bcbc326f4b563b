"""The epilogue of the destination-major relational kernel (rgcn_pair.hip) on every shape of it: the waves' shares of U summed
per row (three rows are more 16-byte items than threads), U contracted with basis, the slices' sums folded per output.

Graphs of 50, 300 and 700 destinations (one, two and three rows per workgroup on a device of 256 compute units) and a few
thousand edges.  Two thirds of the destinations draw about one edge, the others the rest: a workgroup's waves are dealt in
proportion to its rows' costs, at least one each, so a light row next to heavy ones sits on one wave, and the only row of a
one-row workgroup on all sixteen.  test_wave_split_has_both_extremes holds that to the plan's own host layout
(tests/pair_waves_host.cpp), without a GPU.

Every case: per element against the float64 oracle at the bound the relational tests hold this kernel to
(rho_default <= C max(rho_exact, rho_ref32), C = 1.5, tests/test_gpu_scales.py; the exact path is the general kernel), and
twice for identical bits."""
import functools
import os
import subprocess

import pytest
import torch

import gripnet_amd
import scale_cases as sc
from gripnet_amd import _hip
from oracle import gripnet_oracle as orc

C = 1.5

# (destinations, edges, relations, fin, fout, bases, basis stored transposed, partial sums, x with its split planes)
CASES = [
    (50, 3000, 5, 48, 32, 32, False, False, True),       # one row a workgroup: all sixteen waves; the workload's instantiation
    (300, 4000, 5, 48, 32, 32, False, False, True),      # two rows
    (700, 6000, 7, 48, 32, 32, False, False, True),      # three rows: 1,296 items of the shares' sum on 1,024 threads
    (700, 6000, 7, 48, 32, 32, True, True, False),
    (645, 5000, 1000, 48, 32, 32, False, False, True),   # an att table of 1,000 relations: 126 KB of the 160 KB
    (700, 5000, 5, 48, 4, 32, False, False, False),      # 1,024 slices: two rows of basis a thread, eight passes of the fold
    (300, 4000, 5, 48, 8, 5, False, True, False),        # 5 bases: one tile of bases, the slices' sums behind the rows' sums
    (700, 5000, 5, 48, 16, 5, True, False, True),
    (300, 4000, 5, 48, 64, 5, False, False, False),      # 64 outputs: the widest the route admits (64 slices)
    (300, 4000, 5, 16, 32, 32, False, False, False),     # 16 and 32 inputs: sixteen rows of basis a thread
    (700, 5000, 5, 32, 64, 32, True, True, False),
    (700, 5000, 5, 32, 4, 5, False, False, False),
    (50, 2000, 5, 16, 8, 5, False, True, False),
    (300, 4000, 5, 64, 32, 16, False, False, False),     # 64 inputs on 16 bases: four tiles of features
    (700, 6000, 7, 64, 16, 16, True, False, False),
]


def case_id(c):
    return "n{}-R{}-{}to{}-B{}{}{}{}".format(c[0], c[2], c[3], c[4], c[5], "-t" if c[6] else "", "-partial" if c[7] else "", "-planes" if c[8] else "")


@functools.lru_cache(maxsize=None)
def operands(case):
    n, e, rel, fin, fout, bases, _, _, _ = case
    gen = torch.Generator().manual_seed(sum(case[:6]) + 7 * int(case[6]) + 11 * int(case[7]))
    light = (2 * n) // 3                                          # destinations [0, light): about one edge each
    sizes = [e // rel] * rel
    sizes[1] = 0                                                  # an empty relation
    sizes[-1] += e - sum(sizes)
    blocks = []
    for s in sizes:
        dst = torch.randint(light, n, (s,), generator=gen)
        few = torch.rand(s, generator=gen) < light / e
        dst[few] = torch.randint(0, light, (int(few.sum()),), generator=gen)
        blocks.append(torch.stack([torch.randint(0, n, (s,), generator=gen), dst]))
    rei, rl = torch.cat(blocks, dim=1), gripnet_amd.utils.get_range_list(blocks)
    std = 1 / fin ** 0.5
    ops = {"x": torch.randn(n, fin, generator=gen), "basis": torch.randn(bases, fin, fout, generator=gen) * std,
           "att": torch.randn(rel, bases, generator=gen) / bases ** 0.5, "root": torch.randn(fin, fout, generator=gen) * std,
           "bias": torch.randn(fout, generator=gen)}
    return ops, rei, rl


def oracle(case, ops, rei, rl, dtype, magnitude=False):
    """The layer (or, partial, its un-normalised edge sums) by the oracle in `dtype`; `magnitude`: on the operands' absolute values."""
    partial = case[7]
    t = {k: (v.abs() if magnitude else v).to(dtype) for k, v in ops.items()}
    if not partial:
        return orc.rgcn_forward(t["x"], rei, rl, t["basis"], t["att"], t["root"], t["bias"])
    mean = orc.rgcn_forward(t["x"], rei, rl, t["basis"], t["att"], torch.zeros_like(t["root"]), None)
    cnt = torch.bincount(rei[1], minlength=case[0]).clamp(min=1).to(dtype)
    return mean * cnt.view(-1, 1)


def run(case, ops, rei, rl, gpu, path="pair"):
    n, e, rel, fin, fout, bases, transposed, partial, planes = case
    plan = _hip.RgcnPlan(rei.to(gpu), rl, n)
    assert plan.path(fin, fout, bases, path=path) == path
    x = ops["x"].to(gpu)
    xp = _hip.SplitPlanes(n, fin // 16, gpu).fill_from(x) if planes and path == "pair" else None
    basis = ops["basis"].to(gpu)
    stored = basis.transpose(1, 2).contiguous() if transposed and path == "pair" else basis
    out = torch.full((n, fout), float("nan"), device=gpu)
    root, bias = (None, None) if partial else (ops["root"].to(gpu), ops["bias"].to(gpu))
    outs = []
    for _ in range(2 if path == "pair" else 1):
        out = torch.full((n, fout), float("nan"), device=gpu)
        plan.forward(x, stored, ops["att"].to(gpu), root, bias, False, out, partial=partial, path=path, x_planes=xp,
                     basis_transposed=transposed and path == "pair")
        outs.append(out)
    torch.cuda.synchronize()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_epilogue_against_the_oracle(gpu, monkeypatch, index):
    monkeypatch.setenv("GN_DISABLE_FAST", "0")
    case = CASES[index]
    ops, rei, rl = operands(case)
    deg = torch.bincount(rei[1], minlength=case[0])
    assert (deg == 0).any() and (deg[: 2 * case[0] // 3] <= 4).float().mean() > 0.9 and deg.max() >= 15
    outs = run(case, ops, rei, rl, gpu)
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    ref64, mag64 = oracle(case, ops, rei, rl, torch.float64), oracle(case, ops, rei, rl, torch.float64, magnitude=True)
    rho = {"default": sc.componentwise(outs[0], ref64, mag64),
           "exact-general": sc.componentwise(run(case, ops, rei, rl, gpu, "general")[0], ref64, mag64),
           "ref32": sc.componentwise(oracle(case, ops, rei, rl, torch.float32), ref64, mag64)}
    sc.check("pair epilogue " + case_id(case), rho, C)
    _hip.raise_if_index_errors(gpu)


COMPUTE_UNITS = 256                                               # the device the plan's geometry is laid out for (MI355X)


def test_wave_split_has_both_extremes(tmp_path):
    """No GPU: the plan's host layout on the graphs above.  With one row a workgroup the row has all sixteen waves; among the
    workgroups of two and three rows there is a row on a single wave; every row has a wave and every workgroup sixteen."""
    exe = tmp_path / "pair_waves_host"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-I", os.path.join(repo, "gripnet_amd", "csrc"),
                            os.path.join(repo, "tests", "pair_waves_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    seen = {}
    for case in {(c[0], c[1], c[2]): c for c in CASES}.values():
        n, e, rel = case[:3]
        _, rei, rl = operands(case)
        et = [r for r in range(rl.shape[0]) for _ in range(int(rl[r, 1] - rl[r, 0]))]
        groups = min(n, COMPUTE_UNITS)
        text = "{} {} {} {}\n".format(n, rel, e, groups) + "".join("{} {} {}\n".format(int(rei[0, i]), int(rei[1, i]), et[i]) for i in range(e))
        run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        shares = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
        assert len(shares) == groups and all(sum(s) == 16 and min(s) >= 1 for s in shares), case_id(case)
        assert sum(len(s) for s in shares) == n and max(len(s) for s in shares) == -(-n // COMPUTE_UNITS)
        seen.setdefault(n, []).extend(shares)
    assert all(s == [16] for s in seen[50])
    for n, rows in ((300, 2), (700, 3)):
        multi = [s for s in seen[n] if len(s) == rows]
        assert multi and any(min(s) == 1 for s in multi), n
    assert any(len(s) == 1 for s in seen[300])                     # 300 rows on 256 workgroups: most have one row
