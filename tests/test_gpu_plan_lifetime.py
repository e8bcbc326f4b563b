"""Every handle of the library gives back exactly the device memory it took: gn_device_blocks_live() counts the library's
own device allocations (plan buffers and builders' scratch blocks), so "nothing leaked" is an equality of two counts - on a
shared card free memory says nothing.  Covered: a build, one use where the use allocates, and the destroy of every handle
type; and every create that refuses its input."""
import gc

import pytest
import torch

from gripnet_amd import _hip

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _edges(n_src, n_dst, e, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_dst, (e,), generator=g)]).to(DEV)


def _typed(n, r, e, seed):
    """A type-sorted list of e edges over n nodes: (edge_index, edge_type, range_list)."""
    g = torch.Generator().manual_seed(seed)
    et = torch.sort(torch.randint(0, r, (e,), generator=g)).values
    ends = torch.cumsum(torch.bincount(et, minlength=r), 0)
    ranges = torch.stack([ends - torch.bincount(et, minlength=r), ends], dim=1)
    return _edges(n, n, e, seed + 1), et.to(DEV), ranges


def _gcn():
    plan = _hip.GraphPlan.gcn(_edges(64, 64, 400, 1), 64)
    plan.aggregate_t(torch.ones((64, 8), device=DEV), torch.empty((64, 8), device=DEV))     # builds the transpose
    assert plan.build_blocked(16) == 16
    after_first = _hip.device_blocks_live()
    assert plan.build_blocked(32) == 32                      # re-allocates all seven blocked buffers
    assert _hip.device_blocks_live() == after_first
    return plan


def _bipartite():
    return _hip.GraphPlan.bipartite(_edges(30, 12, 100, 2), 30, 12)


def _sum_and_rel_grad():
    n, r = 40, 3
    ei, et, _ = _typed(n, r, 300, 3)
    sums = _hip.GraphPlan.plain_sum(torch.stack([ei[1], et * n + ei[0]]), n, r * n)
    return sums, _hip.RelGradPlan(sums, n, r)


def _rgcn(light=False, empty_shard=False):
    ei, _, ranges = _typed(40, 3, 300, 4)
    plan = _hip.RgcnPlan(ei, ranges, 40, 150 if empty_shard else None, 150 if empty_shard else None, light=light)
    # the full plan holds both LDS encodings and a light plan neither (a forced path the plan cannot serve falls to another
    # kernel); a shard without edges has no LDS-accumulator segments, its destination-major units are built (all empty)
    assert (plan.path(16, 32, 2, path="lds") == "lds") == (not light and not empty_shard)
    assert (plan.path(16, 32, 2, path="pair") == "pair") == (not light)
    return plan


def _distmult(features):
    ei, et, _ = _typed(20, 3, 200, 5)
    return _hip.DistMultPlan(ei, et, 20, 3, features)


def _distmult_bwd():
    ei, et, _ = _typed(20, 3, 200, 5)
    return _hip.DistMultBwdPlan(ei, et, 20, 3)


def _metrics():
    return _hip.MetricsPlan(_typed(20, 3, 50, 6)[2], DEV)


def _sampler():
    ei, _, ranges = _typed(20, 3, 200, 7)
    before = _hip.device_blocks_live()
    sampler = _hip.NegativeSampler(ei, 20, ranges)
    # the library has no query for a sampler's encodings; its buffers say it: sorted keys and block starts, then the narrow
    # keys and relation ids, the bitmap, the tasks - one device block each, the builder's scratch already gone
    assert _hip.device_blocks_live() - before == 6
    return sampler


def _known(e=200):
    ei, et, _ = _typed(20, 3, e, 8)
    return _hip.KnownPairs((ei, et), 20, 3)


BUILDERS = {
    "gcn": _gcn,
    "bipartite": _bipartite,
    "sum+rel_grad": _sum_and_rel_grad,
    "rgcn": _rgcn,
    "rgcn-light": lambda: _rgcn(light=True),
    "rgcn-empty-shard": lambda: _rgcn(empty_shard=True),
    "distmult-row-class": lambda: _distmult(16),
    "distmult-column-phase": lambda: _distmult(0),
    "distmult-bwd": _distmult_bwd,
    "link-metrics": _metrics,
    "sampler": _sampler,
    "known-pairs": _known,
    "known-pairs-empty": lambda: _known(0),
}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_build_and_destroy_leave_no_device_block(name, monkeypatch):
    monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    for _ in range(2):                                       # (twice: a leak of a first-use path is not a baseline)
        before = _hip.device_blocks_live()
        handle = BUILDERS[name]()
        torch.cuda.synchronize()
        assert _hip.device_blocks_live() > before
        del handle
        gc.collect()
        assert _hip.device_blocks_live() == before


def _bad_node(n_src, n_dst, e, seed, bad):
    ei = _edges(n_src, n_dst, e, seed)
    ei[1, e // 2] = bad
    return ei


def _bad_rgcn_ranges():
    ei, _, ranges = _typed(40, 3, 300, 4)
    ranges = ranges.clone()
    ranges[1, 0] += 1                                        # relation 1 does not begin where relation 0 ended
    return _hip.RgcnPlan(ei, ranges, 40)


def _bad_sampler_ranges():
    ei, _, ranges = _typed(20, 3, 200, 7)
    ranges = ranges.clone()
    ranges[2, 1] -= 1                                        # the rows end one edge short of E
    return _hip.NegativeSampler(ei, 20, ranges)


def _bad_distmult():
    ei, et, _ = _typed(20, 3, 200, 5)
    et = et.clone()
    et[-1] = 3
    return _hip.DistMultPlan(ei, et, 20, 3, 16)


# (a create that refuses its input, the error it raises, the correct create of the same type)
REFUSALS = {
    "gcn-node": (lambda: _hip.GraphPlan.gcn(_bad_node(64, 64, 400, 1, 64), 64), IndexError, lambda: _hip.GraphPlan.gcn(_edges(64, 64, 400, 1), 64)),
    "bipartite-node": (lambda: _hip.GraphPlan.bipartite(_bad_node(30, 12, 100, 2, 12), 30, 12), IndexError, _bipartite),
    "rgcn-node": (lambda: _hip.RgcnPlan(_bad_node(40, 40, 300, 4, 40), _typed(40, 3, 300, 4)[2], 40), IndexError, _rgcn),
    "sampler-node": (lambda: _hip.NegativeSampler(_bad_node(20, 20, 200, 7, 20), 20, _typed(20, 3, 200, 7)[2]), IndexError, _sampler),
    "known-pairs-node": (lambda: _hip.KnownPairs((_bad_node(20, 20, 200, 8, 20), _typed(20, 3, 200, 8)[1]), 20, 3), IndexError, _known),
    "distmult-relation": (_bad_distmult, IndexError, lambda: _distmult(16)),
    "rgcn-ranges": (_bad_rgcn_ranges, ValueError, _rgcn),
    "sampler-ranges": (_bad_sampler_ranges, ValueError, _sampler),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_create_leaves_no_device_block(name):
    refused, error, correct = REFUSALS[name]
    before = _hip.device_blocks_live()
    with pytest.raises(error):
        refused()
    gc.collect()
    assert _hip.device_blocks_live() == before
    handle = correct()                                       # the library still builds the same type right after
    assert _hip.device_blocks_live() > before
    del handle
    gc.collect()
    assert _hip.device_blocks_live() == before
