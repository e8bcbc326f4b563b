"""The heads of the forward step's kernels: what they request before their first barrier and in what order.  None of it
reaches a result, so every case here is held to recorded bits.

  * relational layer on the destination-major kernel (rgcn_pair.hip): one, two and three rows per workgroup; an att table
    of no whole DMA piece, exactly one, one and a tail; the DMA and the padded fill; with and without the side copy; 32 and
    48 inputs.  Against the float64 oracle at the scale tests' tolerance, twice (same bits), and against the recording.
  * decoder (distmult_plan.hip): the plan kernel's scores are the plan-less kernel's, bit for bit - one class and three,
    the DMA and the register-staged fill, few and many relations, one walk and two, the two-launch column form, z
    rewritten between ten calls.
  * gene gather (gcn_blocked.hip) on small graphs whose waves have 0, 1, 7, 8, 9, 15, 16, 17 and 25 iterations: staged and
    direct kernels, same bits, the recorded ones, within the layer tests' tolerance of the oracle.

The recordings (tests/golden/kernel_heads_*.npy) come from the library as it was before the heads were reordered: see
tests/kernel_heads_cases.py.
"""
import os

import pytest
import torch

import kernel_heads_cases as kh
import scale_cases as sc
from gripnet_amd import _hip
from oracle import gripnet_oracle as orc
from test_gpu_decoder_fill import CALLS, make_list, plan_serves, spread

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("GN_DISABLE_FAST") == "1", reason="fast paths disabled")]

C = 1.5                                          # tests/test_gpu_scales.py: rho_default <= C max(rho_exact..., rho_ref32)


@pytest.fixture(autouse=True)
def every_fast_path_on(monkeypatch):
    for hook in ("GN_DISABLE_FAST", "GN_DISABLE_QUAD", "GN_DISABLE_BLOCKED", "GN_DISABLE_LDS_TABLE"):
        monkeypatch.setenv(hook, "0")
    monkeypatch.delenv("GN_BLOCKED_DIRECT", raising=False)
    monkeypatch.setenv("GN_BLOCKED_ANY", "1")


# ---- relational layer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(kh.PAIR_CASES)), ids=[kh.pair_id(c) for c in kh.PAIR_CASES])
def test_pair_kernel_keeps_its_bits(gpu, index):
    case = kh.PAIR_CASES[index]
    n, rel, bases, catout, fin = case
    ops, rei, rl = kh.pair_operands(case)
    run = kh.PairRunner(case, ops, rei, rl, gpu)
    y, slot = run.run("pair")
    assert run.path("pair") == "pair"
    # 1. the float64 oracle, per element, at the scale tests' tolerance for this kernel
    act = torch.relu if catout else (lambda t: t)
    ref64, mag64 = sc.rgcn_ref(ops["x"], rei, rl, ops)
    ref64 = act(ref64)
    rho = {"default": sc.componentwise(y, ref64, mag64)}
    for kernel in ("general", "lds"):
        rho["exact-" + kernel] = sc.componentwise(run.run(kernel)[0], ref64, mag64)
        assert run.path(kernel) == kernel
    rho["ref32"] = sc.componentwise(act(sc.rgcn_ref(ops["x"], rei, rl, ops, torch.float32)), ref64, mag64)
    sc.check("pair " + kh.pair_id(case), rho, C)
    if catout:
        assert torch.equal(slot, run.x), "the side copy of x"
    # 2. a second call, 3. the recording
    again, slot2 = run.run("pair")
    assert torch.equal(again, y), "two calls differ"
    if catout:
        assert torch.equal(slot2, run.x)
    kh.assert_recorded("pair", index, kh.pair_id(case), y)
    _hip.raise_if_index_errors(gpu)


# ---- decoder -----------------------------------------------------------------------------------------------------------
def many_relations(total_pairs, relations):
    """`relations` relations of a few pairs each (odd sizes, some empty)."""
    sizes = [(total_pairs // relations) + (r % 5) - 2 if r % 11 else 0 for r in range(relations)]
    sizes[-1] += total_pairs - sum(sizes)
    return sizes


def check_plan_against_plan_less(gpu, n, f, ei, et, R, seed):
    """z rewritten between ten calls per sigmoid setting; the plan kernel's scores against the plan-less kernel's."""
    ei, et = ei.to(gpu), et.to(gpu)
    gen = torch.Generator(device=gpu).manual_seed(4000 + seed)
    z = torch.zeros(n, f, device=gpu)
    w = torch.randn(R, f, generator=gen, device=gpu)
    plan = _hip.DistMultPlan(ei, et, n, R, f)
    assert plan_serves(n, f)
    E = ei.shape[1]
    for sigmoid in (True, False):
        for _ in range(CALLS):
            z.copy_(torch.randn(n, f, generator=gen, device=gpu))
            want = _hip.distmult(z, ei, et, w, sigmoid, torch.full((E,), float("nan"), device=gpu))
            got, served = _hip.distmult_forward(z, ei, et, w, sigmoid, torch.full((E,), float("nan"), device=gpu), plan)
            assert served, "the plan left the call to the plan-less kernel"
            assert torch.equal(got, want), (n, f, E, sigmoid, (got != want).sum().item())
    _hip.raise_if_index_errors(gpu)
    return plan, z, w


# 40 nodes: one block, one class, a handful of workgroups; 449 and 645: three classes.  80 features: J = 5, odd, the LDS-DMA
# fill; 64: J = 4, the register-staged fill.  7 relations of uneven sizes; 200 relations of a few pairs each (a workgroup's
# batches name many rows of D).
@pytest.mark.parametrize("relations", [7, 200])
@pytest.mark.parametrize("f", [80, 64])
@pytest.mark.parametrize("n", [40, 449, 645])
def test_plan_kernel_equals_plan_less_kernel(gpu, n, f, relations):
    if f == 64 and n == 645:
        assert not plan_serves(n, f)            # (645 nodes cut 64 columns into 48 | 16: no instantiation, not a case of this kernel)
        n = 470                                 # three classes at 64 features (449 is one block there)
    pairs = 3000 if relations == 7 else 4000
    sizes = spread(pairs, relations) if relations == 7 else many_relations(pairs, relations)
    ei, et = make_list(n, sizes, seed=n + f + relations)
    check_plan_against_plan_less(gpu, n, f, ei, et, relations, seed=n + f)


def test_plan_kernel_on_eight_position_parts(gpu):
    """Enough pairs for the eight position ranges (one per XCD) and all 256 workgroups: one walk."""
    n, R = 645, 7
    ei, et = make_list(n, spread(72000, R), seed=31)
    check_plan_against_plan_less(gpu, n, 80, ei, et, R, seed=31)


def test_plan_kernel_two_walks(gpu):
    """Just past the 1 MB score window per XCD: every workgroup walks two batch ranges and refills its rows of D between
    them (the list size is what tests/test_gpu_decoder_fill.py forces a second walk with)."""
    n, R = 449, 8
    ei, et = make_list(n, [137500] * R, seed=8)
    check_plan_against_plan_less(gpu, n, 80, ei, et, R, seed=8)


def test_plan_kernel_two_launch_column_form(gpu):
    """Columns [0, 48) and [48, 80) in two launches (the first by LDS-DMA on a 48-column table, or strided on the whole
    one; the second never a byte copy): the single launch's bits."""
    n, f, R = 645, 80, 7
    ei, et = make_list(n, spread(20000, R), seed=41)
    plan, z, w = check_plan_against_plan_less(gpu, n, f, ei, et, R, seed=41)
    E = ei.shape[1]
    gen = torch.Generator(device=gpu).manual_seed(42)
    for sigmoid in (True, False):
        for _ in range(CALLS):
            z.copy_(torch.randn(n, f, generator=gen, device=gpu))
            whole = plan.forward(z, w, sigmoid, torch.full((E,), float("nan"), device=gpu))
            for first in (z[:, :48].contiguous(), z):
                out = torch.full((E,), float("nan"), device=gpu)
                plan.forward_cols(first, f, 0, 48, w, sigmoid, out)
                plan.forward_cols(z, f, 48, 80, w, sigmoid, out)
                assert torch.equal(out, whole)


# ---- gene gather -------------------------------------------------------------------------------------------------------
GATHER_TOL = 2e-5                                # tests/test_gpu_blocked.py's, for unit-scale inputs


@pytest.mark.parametrize("index", range(len(kh.GATHER_CASES)), ids=[c[0] for c in kh.GATHER_CASES])
def test_gather_heads_keep_their_bits(gpu, monkeypatch, index):
    case = kh.GATHER_CASES[index]
    name, n, _, wanted = case
    ei, xw, bias = kh.gather_operands(case)
    ref = torch.relu(orc.gcn_forward(xw.double(), torch.eye(kh.GATHER_COLS, dtype=torch.float64), bias.double(), ei, None))
    plan, staged = kh.run_gather(case, ei, xw, bias, gpu)
    assert plan.blocked_gather_kernel == "staged"
    iters = set(plan.blocked_waves()[:, :, 1].flatten().tolist())
    assert wanted <= iters, "{}: no wave with {} iterations (the waves have {})".format(name, sorted(wanted - iters), sorted(iters))
    monkeypatch.setenv("GN_BLOCKED_DIRECT", "1")
    plan_d, direct = kh.run_gather(case, ei, xw, bias, gpu)
    assert plan_d.blocked_gather_kernel == "direct"
    monkeypatch.delenv("GN_BLOCKED_DIRECT")
    assert torch.equal(staged, direct), "staged and direct kernels differ in {} values".format((staged != direct).sum().item())
    for out in (staged, direct):
        assert torch.isfinite(out).all()
        err = (out.cpu().double() - ref).abs().max().item()
        assert err <= GATHER_TOL, "max abs err {:.3e} > {:.1e}".format(err, GATHER_TOL)
    kh.assert_recorded("gather", index, name + " staged", staged)
    kh.assert_recorded("gather", index, name + " direct", direct)
    _, again = kh.run_gather(case, ei, xw, bias, gpu)
    assert torch.equal(again, staged), "two calls differ"
    _hip.raise_if_index_errors(gpu)
