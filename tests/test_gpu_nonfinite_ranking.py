"""Ranking and top-k under non-finite scores on the GPU (KGEModel.rank / .top_k, multiRelaInnerProductDecoder.rank / .top_k;
csrc/rank_engine.cuh, csrc/kge_rank.hip) against the float64 references of tests/nonfinite_rank_cases.py, which state the
contract of include/gripnet_hip.h: a non-finite score never flatters the model.

  rank   greater = the admitted candidates with NOT (s(c) <= s(true)), ties = those with s(c) == s(true);
  top-k  NaN and -inf never enter, +inf enters, equal scores by ascending id, padding -inf / -1;
  non-finite scores set no bit of the error word; out-of-range ids, invalid and empty ranges keep their results.

The cases are exact (tests/test_nonfinite_rank_host.py holds them to that, and to the conditions under which a pass means
something: every class of score among the true scores and the admitted candidates, poisoned candidates behind the filter and
outside the ranges, and counts that differ from the rule s(c) > s(true) the kernels had before - on those kernels
test_rank_counts and test_a_diverged_model_does_not_score_well fail).  So every comparison is torch.equal; there is no
tolerance anywhere.  Scores are compared by their bits after `+ 0.0` (the sign of a zero score is not part of the contract),
and no NaN may appear in a valid query's list.  Five instantiation families run: the decoder (z[u] * D[r] on load), prepared
query rows (DistMult, ComplEx), the vector-ALU scan (TransE, RotatE), each ranged and unranged, each for rank and top-k.

Found on the first run on an MI355X: ComplEx on the head side with +inf in one column of a candidate's row gave counts 13
below raw_score's for 84 of 300 queries (the 13 poisoned rows), at every n and H - the head-side scan scores the regrouped
form (rr tr + ri ti) hr + (rr ti - ri tr) hi, which is +-inf where Re((h r) conj t) is NaN.  No 0 * inf came out as
anything but NaN on the matrix cores or the vector ALU.  The header now documents that form and the reference of ComplEx's
head side is nonfinite_rank_cases.complex_head_score; every other family equals kge_cases.raw_score's float64 run."""
import functools

import pytest
import torch

import gripnet_amd
import kge_rank_cases as rc
import nonfinite_rank_cases as nf
import typed_candidates_cases as tc
from gripnet_amd import _hip, utils
from gripnet_amd.decoder import KnownPairs, multiRelaInnerProductDecoder
from test_gpu_kge_ranking import on
from test_gpu_typed_candidates import _flags

pytestmark = pytest.mark.gpu


class Scorer:
    """rank / top_k of a KGEModel or of the decoder on given tables, one calling convention."""

    def __init__(self, c, ent, rel, dev):
        self.c, self.ent = c, ent.to(dev)
        if c.model == "decoder":
            self.m = multiRelaInnerProductDecoder(c.H, c.R).to(dev)
            with torch.no_grad():
                self.m.weight.copy_(rel)
        else:
            self.m = gripnet_amd.KGEModel(c.model, c.n, c.R, c.H, c.gamma).to(dev)
            with torch.no_grad():
                self.m.entity_embedding.copy_(ent)
                self.m.relation_embedding.copy_(rel)

    def rank(self, sample, et, side, known=None, candidates=None):
        if self.c.model == "decoder":
            return self.m.rank(self.ent, sample, et, known=known, candidates=candidates)
        return self.m.rank(sample, et, side=side, known=known, candidates=candidates)

    def top_k(self, fixed, et, k, side, known=None, candidates=None):
        if self.c.model == "decoder":
            return self.m.top_k(self.ent, fixed, et, k, known=known, candidates=candidates)
        return self.m.top_k(fixed, et, k, side=side, known=known, candidates=candidates)


def known_pairs(c, which, side, dev):
    lists = rc.filter_lists(c, which)
    return KnownPairs(on(dev, rc.lists_for(lists, side)), c.n, c.R) if lists else None


@functools.lru_cache(maxsize=None)
def _shared(model, n, H, dev):
    """What every poison of a case shares: per side the clean float64 scores, the known masks and the KnownPairs; the
    queries, the range table and its out-of-range mask, all on the device.  Left unchanged by the tests."""
    c = nf.case(model, n, H)
    dev = torch.device(dev)
    sample, et = c.sample.to(dev), c.et.to(dev)
    per_side = {}
    for side in nf.sides(model):
        fixed, truth = rc.split(sample, side)
        clean = nf.scores(model, c.ent.to(dev), c.rel.to(dev), fixed, et, c.gamma, side)
        per_side[side] = (clean, nf.masks(c, side, dev), {w: known_pairs(c, w, side, dev) for w in rc.FILTERS})
    return c, sample, et, per_side, tc.ranges(n).to(dev), nf.outside(c, dev)


@functools.lru_cache(maxsize=None)
def _reference(model, n, H, poison, dev):
    """Per side: (float64 scores on the poisoned tables, a Scorer on them); computed once, shared by the tests."""
    c, _, _, per_side, _, _ = _shared(model, n, H, dev)
    out = {}
    for side in nf.sides(model):
        ent, rel = nf.poisoned(c, side, poison)
        out[side] = (nf.poisoned_scores(c, side, poison, per_side[side][0]), Scorer(c, ent, rel, torch.device(dev)))
    return out


def bits(x):
    return (x.float() + 0.0).view(torch.int32)


def check_rank(scorer, s64, sample, et, side, known, mask, table, out):
    """rank with and without the range table against the reference; the empty range's queries give 0 / 0."""
    _, truth = rc.split(sample, side)
    for cands in (None, table):
        greater, ties = scorer.rank(sample, et, side, known=known, candidates=cands)
        g_ref, t_ref = nf.ref_rank(s64, truth, mask if cands is None else mask | out)
        assert torch.equal(greater.long(), g_ref), (side, cands is not None, int((greater.long() != g_ref).sum()))
        assert torch.equal(ties.long(), t_ref), (side, cands is not None, int((ties.long() != t_ref).sum()))
        if cands is not None:
            assert not greater[et == tc.EMPTY].any() and not ties[et == tc.EMPTY].any()


def check_top_k(scorer, s64, sample, et, side, known, mask, table, out, ks=nf.KS):
    fixed, _ = rc.split(sample, side)
    padded = 0
    for cands in (None, table):
        full_mask = mask if cands is None else mask | out
        for k in ks:
            scores, ids = scorer.top_k(fixed, et, k, side, known=known, candidates=cands)
            val, idx = nf.ref_topk(s64, full_mask, k)
            assert not torch.isnan(scores).any(), (side, k)          # every query of the case has valid ids
            assert torch.equal(ids, idx), (side, k, cands is not None, int((ids != idx).any(1).sum()))
            assert torch.equal(bits(scores), bits(val)), (side, k, cands is not None)
            empty = (idx == -1).all(1)
            assert ids[empty].eq(-1).all() and torch.isneginf(scores[empty]).all()
            padded += int(empty.sum())
    return padded


# ---- 1, 2: every case against the float64 contract ---------------------------------------------------------------------------
@pytest.mark.parametrize("model,n,H,poison", nf.POISONED)
def test_rank_counts(gpu, model, n, H, poison):
    c, sample, et, per_side, table, out = _shared(model, n, H, str(gpu))
    ref = _reference(model, n, H, poison, str(gpu))
    assert _flags(gpu) == 0
    for side in nf.sides(model):
        s64, scorer = ref[side]
        _, masks, known = per_side[side]
        for which in rc.FILTERS:
            check_rank(scorer, s64, sample, et, side, known[which], masks[which], table, out)
    assert _flags(gpu) == 0                                           # a non-finite score is no index error


@pytest.mark.parametrize("model,n,H,poison", nf.POISONED)
def test_top_k_lists(gpu, model, n, H, poison):
    c, sample, et, per_side, table, out = _shared(model, n, H, str(gpu))
    ref = _reference(model, n, H, poison, str(gpu))
    padded = 0
    for side in nf.sides(model):
        s64, scorer = ref[side]
        _, masks, known = per_side[side]
        for which in rc.FILTERS:
            padded += check_top_k(scorer, s64, sample, et, side, known[which], masks[which], table, out)
    assert padded > 0                                                 # rows of nothing but padding were among them
    assert _flags(gpu) == 0


# ---- 3: a list full of equal +inf ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (8, 36))
@pytest.mark.parametrize("model", ("DistMult", "ComplEx", "decoder"))
def test_flood_of_equal_infinities(gpu, model, H):
    """More than 64 admitted candidates score +inf: the threshold (ts, tv) and merge_row order by id alone."""
    c, sample, et, per_side, table, out = _shared(model, nf.FLOOD_N, H, str(gpu))
    ent, rel = nf.flood(c)
    scorer = Scorer(c, ent, rel, gpu)
    for side in nf.sides(model):
        fixed, _ = rc.split(sample, side)
        s64 = nf.scores(model, ent.to(gpu), rel.to(gpu), fixed, et, c.gamma, side)
        _, masks, known = per_side[side]
        for which in ("none", "full"):
            check_top_k(scorer, s64, sample, et, side, known[which], masks[which], table, out, ks=(nf.FLOOD_K, 10))
            check_rank(scorer, s64, sample, et, side, known[which], masks[which], table, out)
        val, _ = nf.ref_topk(s64, masks["full"], nf.FLOOD_K)
        assert int(torch.isposinf(val).all(1).sum()) >= 4            # (the host test holds the case to this)
    assert _flags(gpu) == 0


# ---- 4: the poison contract carried to the scans ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", nf.MODELS)
def test_clean_queries_keep_their_bits(gpu, model):
    """Random fp32 tables (n = 645, H = 36).  A launch with the poisoned rows NaN against the same launch with those rows
    0.0, over the queries whose fixed entity and true partner are clean: the top-64 list of the NaN launch is the zeroed
    launch's with the zeroed rows' entries taken out, ids and score bits (the NaN rows never enter; what is left of the zeroed
    launch's list is a prefix of the other), and greater_nan - greater_zero equals the float64 reference's difference - for
    the queries in which no zeroed row's float64 score lies within the fp32 error band (kge_rank_cases.tolerance) of the
    true score, decided from the reference alone; at least 100 queries remain."""
    n, H, k = 645, 36, 64
    c = rc.ranking_case(nf.scorer(model), n, H, 4242, False)
    c.model = model
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    table, out = tc.ranges(n).to(gpu), tc.outside(tc.ranges(n), c.et, n).to(gpu)
    for side in nf.sides(model):
        rows = torch.tensor(nf.rows_of(c, side), device=gpu)
        fixed, truth = rc.split(sample, side)
        ent_nan, ent_zero = c.ent.clone(), c.ent.clone()
        ent_nan[rows.cpu()], ent_zero[rows.cpu()] = float("nan"), 0.0
        with_nan, with_zero = Scorer(c, ent_nan, c.rel, gpu), Scorer(c, ent_zero, c.rel, gpu)
        clean = ~torch.isin(fixed, rows) & ~torch.isin(truth, rows)
        # the float64 reference of both launches and the queries it decides
        z64, rel64 = ent_zero.to(gpu), c.rel.to(gpu)
        s_zero = nf.scores(model, z64, rel64, fixed, et, c.gamma, side)
        s_nan = s_zero.clone()
        s_nan[:, rows] = float("nan")
        tol = rc.tolerance(nf.scorer(model), H, z64, rel64, fixed, et, c.gamma, side)
        st = s_zero.gather(1, truth.unsqueeze(1))
        band = tol + tol.gather(1, truth.unsqueeze(1))
        decided = clean & ~((s_zero - st).abs() <= band)[:, rows].any(1)
        assert int(decided.sum()) >= 100, int(decided.sum())
        known = known_pairs(c, "full", side, gpu)
        mask = nf.masks(c, side, gpu)["full"]
        stood = 0
        for cands in (None, table):
            full_mask = mask if cands is None else mask | out
            g_nan, t_nan = with_nan.rank(sample, et, side, known=known, candidates=cands)
            g_zero, t_zero = with_zero.rank(sample, et, side, known=known, candidates=cands)
            want = nf.ref_rank(s_nan, truth, full_mask)[0] - nf.ref_rank(s_zero, truth, full_mask)[0]
            assert torch.equal((g_nan - g_zero).long()[decided], want[decided]), side
            counted = (~full_mask[:, rows] & (rows.unsqueeze(0) != truth.unsqueeze(1))).sum(1)
            assert int(counted[decided].sum()) > 0 and bool((want[decided] >= 0).all())     # NaN rows are among the admitted
            sp, ip = with_nan.top_k(fixed, et, k, side, known=known, candidates=cands)
            sz, iz = with_zero.top_k(fixed, et, k, side, known=known, candidates=cands)
            assert not torch.isin(ip, rows).any()
            keep = ~torch.isin(iz, rows) & (iz >= 0)                  # the zeroed launch's entries that are no zeroed row
            order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices       # kept entries first, in order
            left = keep.sum(1, keepdim=True)
            prefix = torch.arange(k, device=gpu).unsqueeze(0) < left
            same = (ip == iz.gather(1, order)) & (sp.view(torch.int32) == sz.gather(1, order).view(torch.int32))
            assert bool((same | ~prefix)[clean].all()), side
            stood += int((~keep & (iz >= 0))[clean].sum())
        assert stood > 0                                              # zeroed rows did stand in the zeroed launch's lists
    assert _flags(gpu) == 0


# ---- 5: bad ids beside non-finite scores -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ("TransE", "ComplEx", "decoder"))
def test_bad_ids_beside_non_finite_scores(gpu, model):
    """One launch holds an out-of-range id, an invalid range row and NaN scores: -1 / -1 and NaN / -1 for exactly the
    former two, the reference for the rest, bit 0 set, and cleared by the check."""
    n, H, bad_relation = 645, 8, 2
    c, sample, et, per_side, table, out = _shared(model, n, H, str(gpu))
    ref = _reference(model, n, H, "nan", str(gpu))
    bad_table = table.clone()
    bad_table[bad_relation] = torch.tensor((3, n + 1), device=gpu)
    bad_query = int(((et != bad_relation) & (et != tc.EMPTY)).nonzero()[5])      # a query of a valid, non-empty range
    hit = et == bad_relation
    hit[bad_query] = True
    _hip.raise_if_index_errors(gpu)
    for side in nf.sides(model):
        s64, scorer = ref[side]
        _, masks, known = per_side[side]
        fixed, truth = rc.split(sample, side)
        bad_sample = sample.clone()
        bad_sample[1 if side == "tail" else 0, bad_query] = n          # the true partner's id == n
        greater, ties = scorer.rank(bad_sample, et, side, known=known["full"], candidates=bad_table)
        g_ref, t_ref = nf.ref_rank(s64, truth, masks["full"] | out)
        assert greater[hit].eq(-1).all() and ties[hit].eq(-1).all()
        assert torch.equal(greater.long()[~hit], g_ref[~hit]) and torch.equal(ties.long()[~hit], t_ref[~hit])
        assert int(torch.isnan(s64.gather(1, truth.unsqueeze(1)))[~hit].sum()) >= 4      # NaN true scores among the rest
        with pytest.raises(IndexError):
            utils.ranking_metrics(greater, ties, et, c.R)
        _hip.raise_if_index_errors(gpu)                               # the check cleared the word
        bad_fixed = fixed.clone()
        bad_fixed[bad_query] = n
        scores, ids = scorer.top_k(bad_fixed, et, 10, side, known=known["full"], candidates=bad_table)
        val, idx = nf.ref_topk(s64, masks["full"] | out, 10)
        assert ids[hit].eq(-1).all() and torch.isnan(scores[hit]).all()
        assert torch.equal(ids[~hit], idx[~hit]) and torch.equal(bits(scores[~hit]), bits(val[~hit]))
        assert not torch.isnan(scores[~hit]).any()
        assert _flags(gpu) == 1                                       # bit 0, read and cleared
    assert _flags(gpu) == 0


# ---- 6: a diverged model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ("TransE", "ComplEx", "decoder"))
def test_a_diverged_model_does_not_score_well(gpu, model):
    """The whole entity table NaN (one vector-ALU model, one matrix-core model, the decoder): every admitted candidate is
    `greater`, nothing ties, MRR is mean(1 / (1 + greater)) and Hits@1 is 0 - and nothing raises."""
    n, H = 645, 36
    c, sample, et, per_side, table, out = _shared(model, n, H, str(gpu))
    scorer = Scorer(c, torch.full_like(c.ent, float("nan")), c.rel, gpu)
    cols = torch.arange(n, device=gpu).unsqueeze(0)
    for side in nf.sides(model):
        _, masks, known = per_side[side]
        fixed, truth = rc.split(sample, side)
        for which in rc.FILTERS:
            for cands in (None, table):
                admitted = (~masks[which] & (cols != truth.unsqueeze(1)) & (True if cands is None else ~out)).sum(1)
                greater, ties = scorer.rank(sample, et, side, known=known[which], candidates=cands)
                assert torch.equal(greater.long(), admitted) and not ties.any(), (side, which)
                m = utils.ranking_metrics(greater, ties, et, c.R)     # raises nothing
                assert float(m["mrr_all"]) == float((1.0 / (1.0 + greater.double())).mean())
                assert float(m["hits@1_all"]) == float((admitted == 0).double().mean())
                if cands is None:
                    assert bool((admitted > 0).all()) and float(m["hits@1_all"]) == 0.0 and float(m["mrr_all"]) < 0.01
                scores, ids = scorer.top_k(fixed, et, 10, side, known=known[which], candidates=cands)
                assert ids.eq(-1).all() and torch.isneginf(scores).all()
    _hip.raise_if_index_errors(gpu)
    assert _flags(gpu) == 0


# ---- 7: capture --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ("RotatE", "ComplEx"))
def test_capture(gpu, model):
    n, H = 645, 36
    c, sample, et, per_side, table, out = _shared(model, n, H, str(gpu))
    ref = _reference(model, n, H, "+inf@col", str(gpu))

    def run():
        res = []
        for side in rc.SIDES:
            scorer, known = ref[side][1], per_side[side][2]["full"]
            res += scorer.rank(sample, et, side, known=known, candidates=table)
            res += scorer.top_k(rc.split(sample, side)[0], et, 10, side, known=known, candidates=table)
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
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b)
    for side in rc.SIDES:                                             # and the eager bits are the reference's
        s64 = ref[side][0]
        _, truth = rc.split(sample, side)
        g_ref, t_ref = nf.ref_rank(s64, truth, per_side[side][1]["full"] | out)
        i = 0 if side == "tail" else 4
        assert torch.equal(eager[i].long(), g_ref) and torch.equal(eager[i + 1].long(), t_ref)
    assert _flags(gpu) == 0
