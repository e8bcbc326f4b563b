"""Per-relation candidate ranges on the GPU: the `candidates` argument of KGEModel.rank / .top_k,
multiRelaInnerProductDecoder.rank / .top_k and kge.sample_candidates (gn_*_ranged*, csrc/rank_engine.cuh, csrc/kge_rank.hip,
k_kge_candidates of csrc/negsample.hip).

  1. exact tables: rank and top-k equal the float64 reference whose mask also holds every candidate outside the range;
  2. random tables: the ranged call equals the library's own full scan whose KnownPairs additionally holds every
     out-of-range (r, fixed, v), bit for bit, with mixed workgroups (queries as they come) and homogeneous ones (sorted by
     relation: the scan really shortens);
  3. a table of full ranges equals candidates=None, bit for bit;
  4. the sampler equals the numpy model of the documented ranged draw (tests/typed_candidates_cases.py) element for element;
  5. invalid ranges are found on the device and reach only their relation's queries; bad tables raise ValueError;
  6. ranged calls are capturable.
The cases are kge_rank_cases.ranking_case at NS = (37, 645, 2113), whose relations are random (64-query workgroups hold
mixed relations), with typed_candidates_cases.ranges(n)."""
import functools

import numpy as np
import pytest
import torch

import kge_cases as kc
import kge_loss_cases as lc
import kge_rank_cases as rc
import typed_candidates_cases as tc
from gripnet_amd import _hip, kge, utils
from gripnet_amd.decoder import KnownPairs, multiRelaInnerProductDecoder
from test_gpu_kge_ranking import NS, _reference, known_of, model_of, on

pytestmark = pytest.mark.gpu

EXACT = [(m, H) for m in ("TransE", "DistMult", "ComplEx") for H in rc.EXACT_H[m]]
KS = (1, 10, 64)
SENTINEL = -77


def _flags(gpu):
    """The device's error word, read and cleared (tests 4 and 5 provoke its bits on purpose)."""
    flag = _hip.error_flag(gpu)
    bits = int(flag.item())
    flag.zero_()
    return bits


def decoder_of(c, dev):
    """The DistMult decoder with the case's relation table: z = the entity table gives the KGE DistMult scores."""
    dec = multiRelaInnerProductDecoder(c.H, c.R).to(dev)
    with torch.no_grad():
        dec.weight.copy_(c.rel)
    return dec


# ---- 1: exact against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("model,H", EXACT)
def test_rank_exact(gpu, model, H, n):
    c, m, sample, et, ref = _reference(model, n, H, True, str(gpu))
    table = tc.ranges(n).to(gpu)
    out = tc.outside(table, et, n)
    differs = 0
    for side in rc.SIDES:
        fixed, truth = rc.split(sample, side)
        for which in rc.FILTERS:
            greater, ties = m.rank(sample, et, side=side, known=known_of(c, which, side, gpu), candidates=table)
            g_ref, t_ref = rc.ref_rank(ref[side], truth, ref[side, which] | out)
            assert torch.equal(greater.long(), g_ref), (side, which)
            assert torch.equal(ties.long(), t_ref), (side, which)
            g_all, t_all = rc.ref_rank(ref[side], truth, ref[side, which])
            differs += int((g_all != g_ref).sum()) + int((t_all != t_ref).sum())
            assert not greater[et == tc.EMPTY].any() and not ties[et == tc.EMPTY].any()
    assert differs > 0                                                # the ranges change the counts
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("model,H", EXACT)
def test_top_k_exact(gpu, model, H, n, k):
    c, m, sample, et, ref = _reference(model, n, H, True, str(gpu))
    table = tc.ranges(n).to(gpu)
    out = tc.outside(table, et, n)
    for side in rc.SIDES:
        fixed, _ = rc.split(sample, side)
        for which in rc.FILTERS:
            scores, ids = m.top_k(fixed, et, k, side=side, known=known_of(c, which, side, gpu), candidates=table)
            val, idx = rc.ref_topk(ref[side], ref[side, which] | out, k)
            assert torch.equal(ids, idx), (side, which)
            assert torch.equal(scores.to(torch.float64), val), (side, which)
            assert ids[et == tc.EMPTY].eq(-1).all() and torch.isneginf(scores[et == tc.EMPTY]).all()
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("H", rc.EXACT_H["DistMult"])
def test_decoder_exact(gpu, H, n):
    """multiRelaInnerProductDecoder.rank / .top_k with z = the entity table: the DistMult case's tail side."""
    c, _, sample, et, ref = _reference("DistMult", n, H, True, str(gpu))
    dec, z = decoder_of(c, gpu), c.ent.to(gpu)
    table = tc.ranges(n).to(gpu)
    out = tc.outside(table, et, n)
    for which in rc.FILTERS:
        known = known_of(c, which, "tail", gpu)
        greater, ties = dec.rank(z, sample, et, known=known, candidates=table)
        g_ref, t_ref = rc.ref_rank(ref["tail"], sample[1], ref["tail", which] | out)
        assert torch.equal(greater.long(), g_ref) and torch.equal(ties.long(), t_ref), which
        for k in KS:
            scores, ids = dec.top_k(z, sample[0], et, k, known=known, candidates=table)
            val, idx = rc.ref_topk(ref["tail"], ref["tail", which] | out, k)
            assert torch.equal(ids, idx) and torch.equal(scores.to(torch.float64), val), (which, k)
    _hip.raise_if_index_errors(gpu)


# ---- 2: random tables, bit for bit against the library's own full scan ------------------------------------------------------
RANDOM = [(m, n, H) for m in kc.MODELS for n in (645, 2113) for H in ((8, 36, 64, 128) if m == "TransE" else (8, 36, 64))]


@pytest.mark.parametrize("side", rc.SIDES)
@pytest.mark.parametrize("model,n,H", RANDOM)
def test_ranged_equals_the_full_scan_with_the_rest_known(gpu, model, n, H, side):
    c = rc.ranking_case(model, n, H, 31 * n + H, False)
    m = model_of(c, gpu)
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    fixed, _ = rc.split(sample, side)
    table = tc.ranges(n).to(gpu)
    lists = on(gpu, rc.lists_for(c.lists, side))
    known = KnownPairs(lists, n, c.R)
    rows, cols = tc.outside(table, et, n).nonzero(as_tuple=True)
    rest = KnownPairs(lists + [(torch.stack([fixed[rows], cols]), et[rows])], n, c.R)     # rows keyed (relation, fixed entity)
    g_full, t_full = m.rank(sample, et, side=side, known=rest)
    top_full = {k: m.top_k(fixed, et, k, side=side, known=rest) for k in (10, 64)}
    order = torch.sort(et, stable=True).indices                       # homogeneous workgroups
    for perm in (torch.arange(et.numel(), device=gpu), order):
        greater, ties = m.rank(sample[:, perm].contiguous(), et[perm], side=side, known=known, candidates=table)
        assert torch.equal(greater, g_full[perm]) and torch.equal(ties, t_full[perm])
        for k, (s_full, i_full) in top_full.items():
            scores, ids = m.top_k(fixed[perm], et[perm], k, side=side, known=known, candidates=table)
            assert torch.equal(ids, i_full[perm]), k
            assert torch.equal(scores.view(torch.int32), s_full[perm].view(torch.int32)), k
    assert int(g_full.sum()) > 0
    _hip.raise_if_index_errors(gpu)


# ---- 3: full ranges are candidates=None ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", (False, True))
@pytest.mark.parametrize("model", kc.MODELS)
def test_full_ranges_equal_no_table(gpu, model, filtered):
    n, H = 2113, 36
    c = rc.ranking_case(model, n, H, 5, False)
    m = model_of(c, gpu)
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    full = utils.candidate_ranges(c.R, n, device=gpu)
    assert full.is_cuda and full.tolist() == [[0, n]] * c.R
    for side in rc.SIDES:
        known = known_of(c, "full", side, gpu) if filtered else None
        fixed, _ = rc.split(sample, side)
        a, b = m.rank(sample, et, side=side, known=known), m.rank(sample, et, side=side, known=known, candidates=full)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a, b = m.top_k(fixed, et, 10, side=side, known=known), m.top_k(fixed, et, 10, side=side, known=known, candidates=full)
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        a = kge.sample_candidates(sample, et, 33, n, side=side, known=known, seed=9)
        b = kge.sample_candidates(sample, et, 33, n, side=side, known=known, seed=9, candidates=full)
        assert torch.equal(a, b)
    if model == "DistMult":
        dec, z = decoder_of(c, gpu), c.ent.to(gpu)
        known = known_of(c, "full", "tail", gpu) if filtered else None
        a, b = dec.rank(z, sample, et, known=known), dec.rank(z, sample, et, known=known, candidates=full)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a, b = dec.top_k(z, sample[0], et, 10, known=known), dec.top_k(z, sample[0], et, 10, known=known, candidates=full)
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert _flags(gpu) == 0


# ---- 4: the sampler ---------------------------------------------------------------------------------------------------------
N37 = 37


@functools.lru_cache(maxsize=None)
def _sampler_case(B):
    """B positives over the relations 0..3 (B = 1: one per call of the test) and a known list of about 3 n triples that
    holds every positive, a long row for the first positive, and partners inside every range."""
    gen = torch.Generator().manual_seed(40 + B)
    positive = torch.randint(0, N37, (2, max(B, 4)), generator=gen)
    et = torch.arange(max(B, 4)) % 4
    more = torch.randint(0, N37, (2, 3 * N37), generator=gen)
    more_et = torch.randint(0, tc.R, (3 * N37,), generator=gen)
    for side_row in (0, 1):                                          # a long row of the first positive, for either side
        more[side_row, side_row * 20: side_row * 20 + 18] = positive[side_row, 0]
        more_et[side_row * 20: side_row * 20 + 18] = et[0]
    return positive, et, torch.cat([positive, more], dim=1), torch.cat([et, more_et])


@pytest.mark.parametrize("side", ("tail", "head"))
@pytest.mark.parametrize("filtered", (False, True))
@pytest.mark.parametrize("K", (1, 7, 64))
@pytest.mark.parametrize("B", (1, 5))
def test_the_block_is_the_documented_ranged_draw(gpu, B, K, filtered, side):
    """cand equals the model element for element (with a device step), written into a column view of a wider matrix of a
    sentinel; every element lies in its relation's range and none is a known partner of its row."""
    positive, et, ei, types = _sampler_case(B)
    table = tc.ranges(N37)
    rows = lc.known_rows(ei, types, side) if filtered else None
    known = KnownPairs([((ei if side == "tail" else ei.flip(0)).contiguous().to(gpu), types.to(gpu))], N37, tc.R) if filtered else None
    step = torch.tensor([3], dtype=torch.int64, device=gpu)
    for first in range(4 if B == 1 else 1):                          # B = 1: each of the ranges r0..r3 in turn
        p, t = positive[:, first:first + B], et[first:first + B]
        fixed = p[0] if side == "tail" else p[1]
        want, flags, _ = tc.draw(fixed, t, K, N37, 11, table, rows, step=3)
        assert flags == 0
        big = torch.full((B, K + 3), SENTINEL, dtype=torch.int64, device=gpu)
        got = kge.sample_candidates(p.to(gpu), t.to(gpu), K, N37, side=side, known=known, seed=11, step=step,
                                    out=big[:, 1:1 + K], candidates=table.to(gpu))
        assert got.data_ptr() == big[:, 1:1 + K].data_ptr()
        assert np.array_equal(got.cpu().numpy(), want)
        assert bool((big[:, 0] == SENTINEL).all()) and bool((big[:, 1 + K:] == SENTINEL).all())
        for b in range(B):
            lo, hi = table[int(t[b])].tolist()
            assert lo <= want[b].min() and want[b].max() < hi
            if filtered:
                assert not set(want[b].tolist()) & rows.get((int(t[b]), int(fixed[b])), set())
        fresh = kge.sample_candidates(p.to(gpu), t.to(gpu), K, N37, side=side, known=known, seed=14, candidates=table.to(gpu))
        assert fresh.is_contiguous() and np.array_equal(fresh.cpu().numpy(), want)      # seed 14 = seed 11 + step 3
    assert int(step) == 3 and _flags(gpu) == 0


def test_a_fully_known_range_and_an_empty_range(gpu):
    """Relation 3's range [36, 37) is one entity: a row that knows it keeps its last draw (36) and sets bit 1; relation 4's
    range is empty: a row of -1 and bit 1; the other rows equal the model."""
    table = tc.ranges(N37)
    positive = torch.tensor([[2, 4, 6], [0, 0, 0]])
    et = torch.tensor([3, 1, 3])
    ei, types = torch.tensor([[2, 2], [36, 5]]), torch.tensor([3, 3])
    known = KnownPairs([(ei.to(gpu), types.to(gpu))], N37, tc.R)
    rows = lc.known_rows(ei, types, "tail")
    want, flags, most = tc.draw(positive[0], et, 7, N37, 5, table, rows)
    assert flags == 2 and most == lc.MAX_ATTEMPTS - 1 and bool((want[[0, 2]] == 36).all())
    got = kge.sample_candidates(positive.to(gpu), et.to(gpu), 7, N37, known=known, seed=5, candidates=table.to(gpu))
    assert np.array_equal(got.cpu().numpy(), want) and _flags(gpu) == 2
    et = torch.tensor([1, tc.EMPTY, 2])
    for kn, r in ((known, rows), (None, None)):
        want, flags, _ = tc.draw(positive[0], et, 7, N37, 5, table, r)
        assert flags == 2 and bool((want[1] == -1).all()) and bool((want[[0, 2]] >= 0).all())
        got = kge.sample_candidates(positive.to(gpu), et.to(gpu), 7, N37, known=kn, seed=5, candidates=table.to(gpu))
        assert np.array_equal(got.cpu().numpy(), want) and _flags(gpu) == 2
    with pytest.raises(RuntimeError, match="no entity"):
        kge.sample_candidates(positive.to(gpu), et.to(gpu), 7, N37, seed=5, candidates=table.to(gpu))
        _hip.raise_if_index_errors(gpu)
    assert _flags(gpu) == 0


# ---- 5: errors ----------------------------------------------------------------------------------------------------------------
def _invalid_rows(n):
    return ((-1, 5), (3, n + 1), (9, 4))


@pytest.mark.parametrize("bad_relation", (0, 2))
@pytest.mark.parametrize("model", ["TransE", "ComplEx", "decoder"])
def test_invalid_ranges_reach_only_their_relation(gpu, model, bad_relation):
    """A row with lo < 0, hi > n or lo > hi is read on the device: -1 / -1 (rank), NaN / -1 (top-k) for its relation's
    queries, the bits of the valid table's call for the others, and the IndexError at the next check."""
    n = 645
    c = rc.ranking_case("DistMult" if model == "decoder" else model, n, 8, 9, True)
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    if model == "decoder":
        dec, z = decoder_of(c, gpu), c.ent.to(gpu)
        rank = lambda side, t: dec.rank(z, sample, et, candidates=t)
        top_k = lambda side, t: dec.top_k(z, sample[0], et, 10, candidates=t)
        sides = ("tail",)
    else:
        m = model_of(c, gpu)
        rank = lambda side, t: m.rank(sample, et, side=side, candidates=t)
        top_k = lambda side, t: m.top_k(rc.split(sample, side)[0], et, 10, side=side, candidates=t)
        sides = rc.SIDES
    good = tc.ranges(n).to(gpu)
    hit = et == bad_relation
    assert 0 < int(hit.sum()) < et.numel()
    _hip.raise_if_index_errors(gpu)
    for row in _invalid_rows(n):
        bad = good.clone()
        bad[bad_relation] = torch.tensor(row, device=gpu)
        for side in sides:
            g0, t0 = rank(side, good)
            g1, t1 = rank(side, bad)
            assert g1[hit].eq(-1).all() and t1[hit].eq(-1).all()
            assert torch.equal(g1[~hit], g0[~hit]) and torch.equal(t1[~hit], t0[~hit])
            with pytest.raises(IndexError):
                _hip.raise_if_index_errors(gpu)
            s0, i0 = top_k(side, good)
            s1, i1 = top_k(side, bad)
            assert i1[hit].eq(-1).all() and torch.isnan(s1[hit]).all()
            assert torch.equal(i1[~hit], i0[~hit]) and torch.equal(s1[~hit].view(torch.int32), s0[~hit].view(torch.int32))
            with pytest.raises(IndexError):
                utils.ranking_metrics(g1, t1, et, c.R)
            _hip.raise_if_index_errors(gpu)                           # the flag is cleared


@pytest.mark.parametrize("filtered", (False, True))
def test_sampler_invalid_ranges_give_rows_of_minus_one(gpu, filtered):
    positive, et, ei, types = _sampler_case(5)
    good = tc.ranges(N37)
    rows = lc.known_rows(ei, types, "tail") if filtered else None
    known = KnownPairs([(ei.to(gpu), types.to(gpu))], N37, tc.R) if filtered else None
    base = kge.sample_candidates(positive.to(gpu), et.to(gpu), 7, N37, known=known, seed=2, candidates=good.to(gpu))
    for row in _invalid_rows(N37):
        bad = good.clone()
        bad[1] = torch.tensor(row)
        want, flags, _ = tc.draw(positive[0], et, 7, N37, 2, bad, rows)
        assert flags == 1 and bool((want[et == 1] == -1).all())
        got = kge.sample_candidates(positive.to(gpu), et.to(gpu), 7, N37, known=known, seed=2, candidates=bad.to(gpu))
        assert np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(got[(et != 1).to(gpu)], base[(et != 1).to(gpu)])
        with pytest.raises(IndexError):
            _hip.raise_if_index_errors(gpu)
    if not filtered:                                                  # without `known` the table's rows are the relations
        short = good[:3].to(gpu)
        want, flags, _ = tc.draw(positive[0], et, 7, N37, 2, good[:3])
        assert flags == 1 and bool((want[et == 3] == -1).all()) and bool((want[et != 3] >= 0).all())
        got = kge.sample_candidates(positive.to(gpu), et.to(gpu), 7, N37, seed=2, candidates=short)
        assert np.array_equal(got.cpu().numpy(), want) and _flags(gpu) == 1


def test_bad_tables_raise_value_error(gpu):
    c = rc.ranking_case("TransE", 37, 8, 9, True)
    m, dec = model_of(c, gpu), decoder_of(c, gpu)
    sample, et, z = c.sample.to(gpu), c.et.to(gpu), c.ent.to(gpu)
    known = known_of(c, "full", "tail", gpu)
    good = tc.ranges(37).to(gpu)
    for bad in (good[:4], torch.zeros(c.R, 3, dtype=torch.int64, device=gpu), good.reshape(-1), good.to(torch.int32),
                good.float(), good.cpu(), good.tolist()):
        with pytest.raises(ValueError):
            m.rank(sample, et, candidates=bad)
        with pytest.raises(ValueError):
            m.top_k(sample[0], et, 3, side="head", candidates=bad)
        with pytest.raises(ValueError):
            dec.rank(z, sample, et, candidates=bad)
        with pytest.raises(ValueError):
            dec.top_k(z, sample[0], et, 3, candidates=bad)
        with pytest.raises(ValueError):
            kge.sample_candidates(sample, et, 4, 37, known=known, candidates=bad)
    wide = torch.zeros(c.R, 4, dtype=torch.int64, device=gpu)
    wide[:, ::2] = good                                               # a strided view: made contiguous
    g0, t0 = m.rank(sample, et, candidates=good)
    g1, t1 = m.rank(sample, et, candidates=wide[:, ::2])
    assert torch.equal(g0, g1) and torch.equal(t0, t1)
    _hip.raise_if_index_errors(gpu)


# ---- 6: capture -----------------------------------------------------------------------------------------------------------------
def test_ranged_rank_and_sampler_capture(gpu):
    n = 645
    c = rc.ranking_case("RotatE", n, 36, 7, False)
    m = model_of(c, gpu)
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    known = known_of(c, "full", "tail", gpu)
    table = tc.ranges(n).to(gpu)
    rows = lc.known_rows(torch.cat([ei for ei, _ in c.lists], 1), torch.cat([t for _, t in c.lists]), "tail")
    step = torch.tensor([5], dtype=torch.int64, device=gpu)
    keep = (c.et != tc.EMPTY)[:8]
    p8, t8 = c.sample[:, :8][:, keep], c.et[:8][keep]                  # the sampler's positives: none of the empty range
    out = torch.empty(p8.shape[1], 7, dtype=torch.int64, device=gpu)
    p8_dev, t8_dev = p8.to(gpu), t8.to(gpu)

    def run():
        res = m.rank(sample, et, known=known, candidates=table)
        kge.sample_candidates(p8_dev, t8_dev, 7, n, known=known, seed=20, step=step, out=out, candidates=table)
        return res

    eager = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
        step += 1
    step.fill_(5)
    for replay in range(3):
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])
        want, flags, _ = tc.draw(p8[0], t8, 7, n, 25 + replay, table.cpu(), rows)
        assert flags == 0 and np.array_equal(out.cpu().numpy(), want)
    assert int(step) == 8 and _flags(gpu) == 0
