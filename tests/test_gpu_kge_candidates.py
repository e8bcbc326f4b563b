"""The [B, K] candidate sampler of the KGE mini-batches on the GPU (k_kge_candidates of csrc/negsample.hip,
kge.sample_candidates) against the numpy model of the documented draw (tests/kge_loss_cases.py: draw), element for element.
The model's distribution is tested where no GPU is needed (tests/test_kge_minibatch_host.py)."""
import functools

import numpy as np
import pytest
import torch

import kge_loss_cases as lc
from gripnet_amd import _hip
from gripnet_amd import kge
from gripnet_amd.decoder import KnownPairs

pytestmark = pytest.mark.gpu

SENTINEL = -77
R = 3


@functools.lru_cache(maxsize=None)
def _case(B, K, n):
    """B positives and a known list of about 2 n triples over R relations that also holds every positive (n = 2: the
    positive alone, which leaves its row one entity)."""
    gen = torch.Generator().manual_seed(100 * B + K + n)
    positive = torch.randint(0, n, (2, B), generator=gen)
    et = torch.randint(0, R, (B,), generator=gen)
    if n == 2:
        return positive, et, positive, et
    more = torch.randint(0, n, (2, 2 * n), generator=gen)
    more[0, : n // 2] = positive[0, 0]                             # a long row for the first positive's head
    more_et = torch.randint(0, R, (2 * n,), generator=gen)
    more_et[: n // 2] = et[0]
    return positive, et, torch.cat([positive, more], dim=1), torch.cat([et, more_et])


def _known(edge_index, edge_type, n, side, gpu):
    ei = edge_index if side == "tail" else edge_index.flip(0)
    return KnownPairs([(ei.contiguous().to(gpu), edge_type.to(gpu))], n, R)


def _flags(gpu):
    """The device's error word, read and cleared (the tests provoke its bits on purpose)."""
    flag = _hip.error_flag(gpu)
    bits = int(flag.item())
    flag.zero_()
    return bits


@pytest.mark.parametrize("seed", (0, 1111))
@pytest.mark.parametrize("side", ("tail", "head"))
@pytest.mark.parametrize("filtered", (False, True))
@pytest.mark.parametrize("B,K,n", ((1, 1, 2), (3, 7, 37), (5, 65, 37), (2, 257, 1000)))
def test_the_block_is_the_documented_draw(gpu, B, K, n, filtered, side, seed):
    """cand equals the model element for element; the output is a column view of a wider matrix of a sentinel, which stays
    as it was beside the view; no candidate is a known partner of its row."""
    positive, et, ei, types = _case(B, K, n)
    rows = lc.known_rows(ei, types, side) if filtered else None
    fixed = positive[0] if side == "tail" else positive[1]
    want, flags, _ = lc.draw(fixed, et, K, n, seed, rows, R)
    assert flags == 0
    big = torch.full((B, K + 3), SENTINEL, dtype=torch.int64, device=gpu)
    known = _known(ei, types, n, side, gpu) if filtered else None
    got = kge.sample_candidates(positive.to(gpu), et.to(gpu), K, n, side=side, known=known, seed=seed, out=big[:, 1:1 + K])
    assert got.data_ptr() == big[:, 1:1 + K].data_ptr()
    assert np.array_equal(got.cpu().numpy(), want)
    assert bool((big[:, 0] == SENTINEL).all()) and bool((big[:, 1 + K:] == SENTINEL).all())
    if filtered:
        for b in range(B):
            assert not set(want[b].tolist()) & rows.get((int(et[b]), int(fixed[b])), set())
    fresh = kge.sample_candidates(positive.to(gpu), et.to(gpu), K, n, side=side, known=known, seed=seed)
    assert fresh.is_contiguous() and np.array_equal(fresh.cpu().numpy(), want)
    assert _flags(gpu) == 0


def test_duplicate_known_pairs_change_nothing(gpu):
    positive, et, ei, types = _case(5, 65, 37)
    twice = _known(torch.cat([ei, ei, ei[:, :9]], dim=1), torch.cat([types, types, types[:9]]), 37, "tail", gpu)
    once = _known(ei, types, 37, "tail", gpu)
    a = kge.sample_candidates(positive.to(gpu), et.to(gpu), 65, 37, known=once, seed=4)
    b = kge.sample_candidates(positive.to(gpu), et.to(gpu), 65, 37, known=twice, seed=4)
    assert torch.equal(a, b)


def test_step_on_the_device_and_a_captured_draw(gpu):
    """step = s gives the draw of seed + s; the counter is read, not advanced; a captured draw replayed after step += 1 gives
    the next one."""
    positive, et, ei, types = _case(3, 7, 37)
    known = _known(ei, types, 37, "tail", gpu)
    rows = lc.known_rows(ei, types, "tail")
    p, t = positive.to(gpu), et.to(gpu)
    step = torch.tensor([5], dtype=torch.int64, device=gpu)
    got = kge.sample_candidates(p, t, 7, 37, known=known, seed=20, step=step)
    assert np.array_equal(got.cpu().numpy(), lc.draw(positive[0], et, 7, 37, 25, rows, R)[0])
    assert np.array_equal(got.cpu().numpy(), lc.draw(positive[0], et, 7, 37, 20, rows, R, step=5)[0])
    assert int(step) == 5
    out = torch.empty(3, 7, dtype=torch.int64, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        kge.sample_candidates(p, t, 7, 37, known=known, seed=20, step=step, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kge.sample_candidates(p, t, 7, 37, known=known, seed=20, step=step, out=out)
        step += 1
    step.fill_(5)
    for replay in range(3):
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), lc.draw(positive[0], et, 7, 37, 25 + replay, rows, R)[0])
    assert int(step) == 8 and _flags(gpu) == 0


def test_one_entity_left_and_none_left(gpu):
    """n = 8, seed 5, K = 64: a row that knows the entities 0..6 draws 7 everywhere and leaves the flag clear (the model goes
    to attempt 40 at most, far below the cap of 4,096); a row that knows all 8 keeps its last draw and sets bit 1."""
    n = 8
    heads = torch.tensor([2, 4])
    ei = torch.stack([torch.cat([heads[:1].repeat(7), heads[1:].repeat(8)]), torch.cat([torch.arange(7), torch.arange(8)])])
    types = torch.ones(15, dtype=torch.long)
    known = KnownPairs([(ei.to(gpu), types.to(gpu))], n, R)
    positive, et = torch.tensor([[2], [0]], device=gpu), torch.tensor([1], device=gpu)
    got = kge.sample_candidates(positive, et, 64, n, known=known, seed=5)
    assert bool((got == 7).all()) and _flags(gpu) == 0
    positive = torch.tensor([[2, 4], [0, 0]], device=gpu)
    et = torch.tensor([1, 1], device=gpu)
    got = kge.sample_candidates(positive, et, 2, n, known=known, seed=5)
    want, flags, _ = lc.draw([2, 4], [1, 1], 2, n, 5, lc.known_rows(ei, types, "tail"), R)
    assert flags == 2 and np.array_equal(got.cpu().numpy(), want)
    assert _flags(gpu) == 2


@pytest.mark.parametrize("filtered", (False, True))
def test_bad_ids_give_a_row_of_minus_one(gpu, filtered):
    """A fixed entity or (with a filter: the relation table's size is the filter's) a relation outside its table: -1 in the
    whole row and bit 0; the other rows equal the model.  Nothing outside the filter's row table is read."""
    positive, et, ei, types = _case(5, 65, 37)
    positive, et = positive.clone(), et.clone()
    positive[0, 1], positive[0, 3] = 37, -1
    if filtered:
        et[4] = R
    et[0] = -2
    rows = lc.known_rows(ei, types, "tail") if filtered else None
    want, flags, _ = lc.draw(positive[0], et, 65, 37, 9, rows, R if filtered else None)
    assert flags == 1 and bool((want[[0, 1, 3]] == -1).all()) and bool((want[2] >= 0).all())
    known = _known(ei, types, 37, "tail", gpu) if filtered else None
    got = kge.sample_candidates(positive.to(gpu), et.to(gpu), 65, 37, known=known, seed=9)
    assert np.array_equal(got.cpu().numpy(), want)
    assert _flags(gpu) == 1


def test_a_filter_of_another_size_is_refused(gpu):
    positive, et, ei, types = _case(3, 7, 37)
    known = _known(ei, types, 37, "tail", gpu)
    with pytest.raises(ValueError):
        kge.sample_candidates(positive.to(gpu), et.to(gpu), 7, 38, known=known)
    with pytest.raises(ValueError):                               # the C boundary's own check
        _hip._call("gn_kge_candidates_sample", positive.to(gpu).data_ptr(), et.to(gpu).data_ptr(), 3, 7, 37, R + 1, known._h, 0, None,
                   torch.empty(3, 7, dtype=torch.int64, device=gpu).data_ptr(), 7, None, _hip.stream_ptr(gpu))
