"""The LDS-staged gene gather's two loops (csrc/gcn_blocked.hip): the staged kernel parks a finished tile's sums in LDS
behind the table and writes every row behind its loop, the direct kernel stores from inside the loop.  Same order of
addends, same expressions: the two must agree bit for bit, and both are held to the float64 oracle at the blocked-path
tests' tolerance.

Which waves a graph produces is read back from the plan (GraphPlan.blocked_waves) and asserted, not assumed: waves
without a tile, with exactly five and with more than five tiles (the tile ends beyond the fifth are loaded inside the
loop), and id streams of exactly 8, exactly 16 and 17 iterations (the prologue requests sixteen; a buffer is requested
again only when iterations beyond the other buffer remain: skipped, skipped, taken).  The sizes were chosen with the
host layout code (layout_blocked.hpp) on the CPU; GN_BLOCKED_ANY=1 lifts the plans' size thresholds."""
import functools
import os

import pytest
import torch

from gripnet_amd import _hip
from oracle import gripnet_oracle as orc

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("GN_DISABLE_FAST") == "1" or os.environ.get("GN_DISABLE_BLOCKED") == "1",
                                 reason="the source-blocked path is switched off")]

TIGHT = 2e-5            # tests/test_gpu_blocked.py
LDS_BYTES = 160 * 1024


@pytest.fixture
def any_size(monkeypatch):
    monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    monkeypatch.delenv("GN_BLOCKED_DIRECT", raising=False)


def stars(n, hubs, isolated=0):
    """A symmetric simple graph on n nodes.  Node k < len(hubs) is joined to hubs[k] of the other nodes, dealt round-robin;
    those also form a ring with their next two neighbours.  The last `isolated` nodes keep nothing but their self loop."""
    h, leaves = len(hubs), n - isolated - len(hubs)
    src, dst, at = [], [], 0
    for k, d in enumerate(hubs):
        assert d <= leaves
        src.append(torch.full((d,), k, dtype=torch.long))
        dst.append(h + (at + torch.arange(d)) % leaves)
        at += d
    ring = h + torch.arange(leaves)
    for step in (1, 2):
        src.append(ring)
        dst.append(h + (torch.arange(leaves) + step) % leaves)
    s, t = torch.cat(src), torch.cat(dst)
    return torch.stack([torch.cat([s, t]), torch.cat([t, s])])


# hubs of 4,001 / 3,001 stored edges: waves of 251 / 189 iterations with six / two tiles, five- and six-tile waves behind
# them; 271 / 251 / 121 stored edges: tiles of exactly 17 / 16 / 8 iterations that are alone in their wave
MIX_HUBS = [4000] * 4 + [3000] * 4 + [270] * 8 + [250] * 8 + [120] * 8
GRAPHS = {
    "mix": (6139, MIX_HUBS, 40),                   # two columns per group, ragged last tiles (rows -1), isolated nodes
    "one_column": (20600, MIX_HUBS, 7),            # beyond 19,9xx nodes a workgroup holds one column
    # 160 KB of LDS = the table (1 KB pieces) + 128 bytes per tile of the largest range.  At 19,839 nodes: 155 pieces +
    # 39 tiles of the 40 that fit.  One node more: 156 pieces, room for 32 tiles, still 39.  (No node count puts a plan
    # at capacity + 1: the table grows by eight tiles' worth at a time and the tile count by one per 512 nodes.)
    "fits": (19839, [300] * 40, 3),
    "too_large": (19840, [300] * 40, 3),
}


@functools.lru_cache(maxsize=None)
def case(name, f):
    """Graph, features, bias and the float64 references (bias + ReLU, no bias and no ReLU), shared and never changed."""
    n, hubs, isolated = GRAPHS[name]
    ei = stars(n, hubs, isolated)
    g = torch.Generator().manual_seed(n + f)
    xw = torch.randn(n, f, generator=g)
    bias = torch.randn(f, generator=g)
    ei2, norm = orc.gcn_norm(ei, n, None, False, torch.float64)
    plain = orc.gcn_propagate(xw.double(), ei2, norm, None)
    return n, ei, xw, bias, {(True, True): torch.relu(plain + bias.double()), (False, False): plain,
                             (True, False): plain + bias.double(), (False, True): torch.relu(plain)}


def err(a, b):
    a = a.detach().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all()
    return (a.double() - b).abs().max().item()


def plan_of(ei, n, f, gpu):
    plan = _hip.GraphPlan.gcn(ei.to(gpu), n)
    assert plan.build_blocked(f) >= f, "the plan did not get its LDS-staged encoding"
    return plan


def takes_the_staged_path(plan, x, bias, out):
    """the library's own answer for a weight-less call (the table is given): LDS-staged gather, not the wave-per-row kernels"""
    return bool(_hip.load().gn_graph_blocked_applicable(plan._h, x.data_ptr(), _hip.ld(x), x.shape[1], None, x.shape[1],
                                                        None if bias is None else bias.data_ptr(), out.data_ptr(), _hip.ld(out)))


def run_both(monkeypatch, launch):
    """launch() under the staged and under the forced direct kernel"""
    staged = launch()
    monkeypatch.setenv("GN_BLOCKED_DIRECT", "1")
    direct = launch()
    monkeypatch.delenv("GN_BLOCKED_DIRECT")
    return staged, direct


def test_the_graphs_produce_the_waves_the_tests_are_about(gpu, any_size):
    n, ei, _, _, _ = case("mix", 16)
    plan = plan_of(ei, n, 16, gpu)
    waves = plan.blocked_waves()
    assert waves.shape == (32, 16, 2)
    tiles, iters = waves[:, :, 0].flatten().tolist(), waves[:, :, 1].flatten().tolist()
    assert 0 in tiles and 5 in tiles and max(tiles) > 5
    for count in (8, 16, 17):
        assert any(t == 1 and i == count for t, i in zip(tiles, iters)), count
    assert max(iters) > 32                        # both buffers requested again, more than once
    assert plan.blocked_gather_kernel == "staged"


@pytest.mark.parametrize("name,f,relu,with_bias", [
    ("mix", 16, True, True), ("mix", 16, False, False), ("mix", 32, True, False), ("mix", 32, False, True),
    ("one_column", 16, True, True), ("one_column", 16, False, False)])
def test_staged_equals_direct_and_the_oracle(gpu, any_size, monkeypatch, name, f, relu, with_bias):
    n, ei, xw, bias, refs = case(name, f)
    plan = plan_of(ei, n, f, gpu)
    assert plan.blocked_gather_kernel == "staged"
    x, b = xw.to(gpu), bias.to(gpu) if with_bias else None

    def launch():
        out = torch.full((n, f), float("nan"), device=gpu)
        assert takes_the_staged_path(plan, x, b, out)
        return plan.aggregate(x, b, relu, out)
    staged, direct = run_both(monkeypatch, launch)
    e = err(staged, refs[(with_bias, relu)])
    print("{} f={} relu={} bias={}: max |staged - float64| = {:.3e}".format(name, f, relu, with_bias, e))
    assert torch.equal(staged, direct)
    assert e <= TIGHT


def test_strided_slot_of_a_concat_buffer_with_a_side_copy(gpu, any_size, monkeypatch):
    """The layer's slot of a wider buffer (row stride 48 + 16), slot 0 filled by the launch's side copy; nothing else is
    touched."""
    n, ei, xw, bias, refs = case("mix", 16)
    plan = plan_of(ei, n, 16, gpu)
    x, b = xw.to(gpu), bias.to(gpu)
    extra = torch.randn(n, 32, device=gpu)

    def launch():
        buf = torch.full((n, 64), float("nan"), device=gpu)
        assert takes_the_staged_path(plan, x, b, buf[:, 32:48])
        plan.aggregate(x, b, True, buf[:, 32:48], side=(extra, buf[:, :32], 0))
        return buf
    staged, direct = run_both(monkeypatch, launch)
    assert torch.equal(staged[:, :48], direct[:, :48])
    assert torch.equal(staged[:, :32], extra)
    assert torch.isnan(staged[:, 48:]).all() and torch.isnan(direct[:, 48:]).all()
    assert err(staged[:, 32:48], refs[(True, True)]) <= TIGHT


@pytest.mark.parametrize("name,kernel", [("fits", "staged"), ("too_large", "direct")])
def test_the_launch_switches_kernel_at_the_staging_capacity(gpu, any_size, monkeypatch, name, kernel):
    n, ei, xw, bias, refs = case(name, 16)
    plan = plan_of(ei, n, 16, gpu)
    tiles = int(plan.blocked_waves()[:, :, 0].sum(dim=1).max())
    table = -(-(n + 1) * 8 // 1024) * 1024
    assert tiles == 39 and (table + 128 * tiles <= LDS_BYTES) == (kernel == "staged")
    assert plan.blocked_gather_kernel == kernel
    x, b = xw.to(gpu), bias.to(gpu)
    out = plan.aggregate(x, b, True, torch.full((n, 16), float("nan"), device=gpu))
    assert err(out, refs[(True, True)]) <= TIGHT
    monkeypatch.setenv("GN_BLOCKED_DIRECT", "1")
    assert plan.blocked_gather_kernel == "direct"
    assert torch.equal(plan.aggregate(x, b, True, torch.full((n, 16), float("nan"), device=gpu)), out)


@pytest.mark.parametrize("name", ["mix", "one_column"])
def test_chained_gather_writes_out_and_the_next_table(gpu, any_size, monkeypatch, name):
    """k_col_gather_next: `out` and, read through the next layer's gather, the table dis * out it leaves for that layer."""
    monkeypatch.setenv("GN_ENABLE_CHAIN", "1")
    n, ei, _, bias, _ = case(name, 16)
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(n, 32, generator=g), torch.randn(32, 16, generator=g) / 4
    ei2, norm = orc.gcn_norm(ei, n, None, False, torch.float64)
    h = torch.relu(orc.gcn_propagate(x.double() @ w.double(), ei2, norm, bias.double()))
    h_next = orc.gcn_propagate(h, ei2, norm, None)
    first, second = plan_of(ei, n, 16, gpu), plan_of(ei, n, 16, gpu)
    xg, wg, bg = x.to(gpu), w.to(gpu), bias.to(gpu)
    assert first.chain_ok(second, xg, wg, bg, torch.empty(n, 16, device=gpu), torch.empty(n, 16, device=gpu))

    def launch():
        out = torch.full((n, 16), float("nan"), device=gpu)
        nxt = torch.full((n, 16), float("nan"), device=gpu)
        first.aggregate_chain(second, xg, wg, bg, True, out)
        second.gather_chained(nxt)
        return out, nxt
    (out_s, next_s), (out_d, next_d) = run_both(monkeypatch, launch)
    assert torch.equal(out_s, out_d) and torch.equal(next_s, next_d)
    assert err(out_s, h) <= TIGHT and err(next_s, h_next) <= TIGHT
