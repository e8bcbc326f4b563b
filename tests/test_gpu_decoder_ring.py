"""The row-class decoder's batch loop (k_distmult_class, distmult_plan.hip) at every number of batches a wave can have: its
prefetch ring runs three batches ahead of the arithmetic, so what matters is how many batches a wave has, up to two whole
periods of the ring and every remainder.  The contract is the existing one: the plan's scores are those of the plan-less
kernel, bit for bit.

A wave's batches: a workgroup takes a contiguous share of its class's batches per walk, its sixteen waves every sixteenth
of them.  On 256 compute units a list of S scored pairs (half the edges where every pair is listed in both directions) is
S / 64 batches on 256 workgroups once S >= 65,536, and one batch per workgroup below that.  The lists below were sized
with the host layout code (layout_decoder.hpp) on the CPU, which gave per wave and walk:

    tiny        360 scored pairs                  0 or 1 batch
    small       393,300                           1 or 2      (22-25 per workgroup)
    medium      918,000                           3 or 4      (53-58)
    distinct    1,800,000, no pair listed twice   6 or 7      (107-112; the most one walk holds: beyond 2,097,152 edges
                                                               a workgroup walks two ranges of half the size)
    two_walks   1,100,000, 2.2 M edges            1 to 3      (30-36 per walk)

which is every remainder of a period of three behind zero, one and two whole periods.
"""
import functools
import os

import pytest
import torch

from gripnet_amd import _hip
from gripnet_amd.utils import to_bidirection

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("GN_DISABLE_FAST") == "1", reason="fast paths disabled")]

CALLS = 10
N = 645


def mirrored_list(n, pairs_per_relation, relations, seed):
    """A type-sorted list: every relation's random pairs, each in both directions (the second copy takes the first's score)."""
    gen = torch.Generator().manual_seed(seed)
    eis, ets = [], []
    for r in range(relations):
        eis.append(to_bidirection(torch.randint(0, n, (2, pairs_per_relation), generator=gen)))
        ets.append(torch.full((2 * pairs_per_relation,), r, dtype=torch.int64))
    return torch.cat(eis, dim=1), torch.cat(ets)


def distinct_list(n, pairs_per_relation, relations, seed):
    """Every (unordered pair, relation) at most once: every edge is scored, none is a mirror."""
    gen = torch.Generator().manual_seed(seed)
    iu = torch.triu_indices(n, n, offset=1)
    eis, ets = [], []
    for r in range(relations):
        eis.append(iu[:, torch.randperm(iu.shape[1], generator=gen)[:pairs_per_relation]])
        ets.append(torch.full((pairs_per_relation,), r, dtype=torch.int64))
    return torch.cat(eis, dim=1), torch.cat(ets)


@functools.lru_cache(maxsize=None)
def edge_list(name):
    """(edges, types, relations), shared by the tests and never changed"""
    if name == "tiny":
        return mirrored_list(N, 40, 9, 1) + (9,)
    if name == "small":
        return mirrored_list(N, 43700, 9, 2) + (9,)
    if name == "medium":
        return mirrored_list(N, 102000, 9, 3) + (9,)
    if name == "distinct":
        return distinct_list(N, 60000, 30, 4) + (30,)
    if name == "two_walks":
        return mirrored_list(N, 137500, 8, 5) + (8,)
    raise KeyError(name)


def check(gpu, name, f, calls=CALLS):
    """`calls` calls per sigmoid setting, z rewritten in place between them: the class path against the plan-less kernel."""
    ei, et, R = edge_list(name)
    if name == "distinct":
        assert ei.shape[1] <= 2097152                       # one walk
    if name == "two_walks":
        assert ei.shape[1] > 2097152
    ei, et = ei.to(gpu), et.to(gpu)
    E = ei.shape[1]
    gen = torch.Generator(device=gpu).manual_seed(100 + f)
    z = torch.zeros(N, f, device=gpu)
    w = torch.randn(R, f, generator=gen, device=gpu)
    plan = _hip.DistMultPlan(ei, et, N, R, f)
    with pytest.raises(_hip.Unsupported):                   # the plan holds the row-class encoding, and only that
        plan.forward_cols(z, f, 0, 4, w, True, torch.empty(E, device=gpu))
    for sigmoid in (True, False):
        for _ in range(calls):
            z.copy_(torch.randn(N, f, generator=gen, device=gpu))
            want = _hip.distmult(z, ei, et, w, sigmoid, torch.full((E,), float("nan"), device=gpu))
            got = plan.forward(z, w, sigmoid, torch.full((E,), float("nan"), device=gpu))
            assert torch.equal(got, want), (name, f, E, sigmoid, (got != want).sum().item())
    _hip.raise_if_index_errors(gpu)
    return plan, z, w, gen


@pytest.mark.parametrize("name", ["tiny", "small", "medium", "distinct", "two_walks"])
def test_every_remainder_of_the_period_80_features(gpu, name):
    check(gpu, name, 80)


@pytest.mark.parametrize("name", ["tiny", "small", "medium"])
def test_every_remainder_of_the_period_48_features(gpu, name):
    check(gpu, name, 48)


@pytest.mark.parametrize("name", ["tiny", "small", "medium", "two_walks"])
def test_two_launch_column_form(gpu, name):
    """Columns [0, 48) then [48, 80): the first launch starts the sums and leaves raw partial sums in `out` (no carried sum,
    no mirror positions), the second reads them back as every batch's carried sum, one batch ahead, and finishes them.  The
    single launch's bits."""
    f = 80
    plan, z, w, gen = check(gpu, name, f, calls=1)
    E = edge_list(name)[0].shape[1]
    for sigmoid in (True, False):
        for _ in range(CALLS):
            z.copy_(torch.randn(N, f, generator=gen, device=gpu))
            whole = plan.forward(z, w, sigmoid, torch.full((E,), float("nan"), device=gpu))
            out = torch.full((E,), float("nan"), device=gpu)
            plan.forward_cols(z, f, 0, 48, w, sigmoid, out)
            plan.forward_cols(z, f, 48, 80, w, sigmoid, out)
            assert torch.equal(out, whole), (name, sigmoid, (out != whole).sum().item())
    _hip.raise_if_index_errors(gpu)
