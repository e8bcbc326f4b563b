"""Filtered ranking and top-k of the KGE baselines (KGEModel.rank / .top_k, csrc/kge_rank.hip) on the GPU against the float64
references of tests/kge_rank_cases.py (kge_cases.raw_score over every candidate triple): exact on tables whose fp32 scores
are exact, within a per-triple bound on random fp32 tables, both sides, with and without the filter.

Bounds (tests 5 and 6).  tol(q, v) = (T + D) * kappa_s * u * scale of tests/test_gpu_kge.py's docstring, with T =
kge_cases.TERM_ROUNDINGS, D = kge_rank_cases.scan_depth (the ranking kernels' own column sum), kappa_s =
kge_cases.condition_scores and scale = kge_cases.abs_term_sum over the candidate triples, u = 2^-24.  A candidate v' counts as
undecided for query q when its float64 score lies within band(q, v') = tol(q, v') + tol(q, v_true) of the true triple's:
g_lo <= greater and greater + ties <= g_hi, as test_gpu_ranking.check_bounded does.  The undecided candidates are capped at
1 % of Q * n per case, asserted from the float64 reference before any kernel output is read.

Measured on an MI355X (the tests print every figure next to its bound; run with -s).  Undecided candidates of Q * n (cap
1 %) and the largest |score - s64| / tol over the top-10 entries (bound 1), tail side / head side:
  RotatE    n = 37     H = 8: 39 / 46 of 11,100 (0.41 %), 0.034;  H = 36: 50 / 42, 0.030;  H = 64: 56 / 49 (0.50 %), 0.026
            n = 645    H = 8: 26 / 30 of 193,500, 0.029;  H = 36: 52 / 46, 0.033;  H = 64: 82 / 83 (0.04 %), 0.034
            n = 2113   H = 8: 43 / 51 of 633,900, 0.027;  H = 36: 105 / 101, 0.039;  H = 64: 189 / 202 (0.03 %), 0.031
  ComplEx   n = 645    H = 8: 31 / 26 of 193,500, 0.021;  H = 36: 41 / 31, 0.027
  DistMult  n = 645    H = 8: 22 / 24 of 193,500, 0.299;  H = 36: 24 / 26, 0.125
  size (n = 19,726, R = 964, H = 32, 2,000 queries): RotatE 4,997 / 5,024 of 39,452,000 (0.013 %), 0.028;
            TransE 3,589 / 3,489 (0.009 %), 0.029
Every count of rank lay inside [g_lo, g_hi], and the exact cases matched the float64 counts and lists on all 33
(model, H, n) shapes.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import gripnet_amd
import kge_cases as kc
import kge_rank_cases as rc
from gripnet_amd import _hip, utils
from gripnet_amd.decoder import KnownPairs
from gripnet_amd.synth import make_rgcn_pose

pytestmark = pytest.mark.gpu

NS = (37, 645, 2113)           # less than one tile; several tiles; not a multiple of 64 and across one 2,048-column window


def model_of(c, dev):
    m = gripnet_amd.KGEModel(c.model, c.n, c.R, c.H, c.gamma).to(dev)
    with torch.no_grad():
        m.entity_embedding.copy_(c.ent)
        m.relation_embedding.copy_(c.rel)
    return m


def on(dev, lists):
    return [(ei.to(dev), et.to(dev)) for ei, et in lists]


def known_of(c, which, side, dev):
    lists = rc.filter_lists(c, which)
    return KnownPairs(on(dev, rc.lists_for(lists, side)), c.n, c.R) if lists else None


@functools.lru_cache(maxsize=None)
def _reference(model, n, H, exact, dev):
    """One case per (model, n, H) and its float64 reference, shared by the tests that use it: per side the scores [Q, n] and
    per (side, filter) the mask."""
    c = rc.ranking_case(model, n, H, 1000 + 7 * n + H, exact)
    dev = torch.device(dev)
    ent, rel, sample, et = c.ent.to(dev), c.rel.to(dev), c.sample.to(dev), c.et.to(dev)
    ref = {}
    for side in rc.SIDES:
        fixed, truth = rc.split(sample, side)
        ref[side] = rc.scores64(model, ent, rel, fixed, et, c.gamma, side)
        for which in rc.FILTERS:
            keys = rc.known_keys(rc.lists_for(rc.filter_lists(c, which), side), n)
            ref[side, which] = rc.known_mask(fixed, et, n, keys)
    return c, model_of(c, dev), sample, et, ref


EXACT = [(m, H) for m in ("TransE", "DistMult", "ComplEx") for H in rc.EXACT_H[m]]


# ---- 1, 2: exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("model,H", EXACT)
def test_rank_exact(gpu, model, H, n):
    c, m, sample, et, ref = _reference(model, n, H, True, str(gpu))
    for side in rc.SIDES:
        fixed, truth = rc.split(sample, side)
        for which in rc.FILTERS:
            greater, ties = m.rank(sample, et, side=side, known=known_of(c, which, side, gpu))
            assert greater.dtype == torch.int32 and ties.dtype == torch.int32 and greater.shape == (sample.shape[1],)
            g_ref, t_ref = rc.ref_rank(ref[side], truth, ref[side, which])
            assert torch.equal(greater.long(), g_ref), (side, which)
            assert torch.equal(ties.long(), t_ref), (side, which)
            assert int(ties.sum()) > 0                       # the engineered ties are there
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("model,H", EXACT)
def test_top_k_exact(gpu, model, H, n, k):
    c, m, sample, et, ref = _reference(model, n, H, True, str(gpu))
    for side in rc.SIDES:
        fixed, _ = rc.split(sample, side)
        scores, ids = m.top_k(fixed, et, k, side=side, known=known_of(c, "full", side, gpu))
        assert scores.shape == (fixed.numel(), k) and scores.dtype == torch.float32 and ids.dtype == torch.int64
        val, idx = rc.ref_topk(ref[side], ref[side, "full"], k)
        assert torch.equal(ids, idx), side
        assert torch.equal(scores.to(torch.float64), val), side
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("side", rc.SIDES)
@pytest.mark.parametrize("model", ["TransE", "ComplEx"])
def test_top_k_pads_when_the_filter_leaves_fewer_than_k(gpu, model, side):
    c = rc.ranking_case(model, 37, 8, 5, True)
    m = model_of(c, gpu)
    # query (entity 4, relation 0): every partner but 0, 11 and 36 is known -> 3 candidates; (9, 1): nothing known
    keep = torch.tensor([v for v in range(37) if v not in (0, 11, 36)], device=gpu)
    ki = torch.stack([torch.full_like(keep, 4), keep])              # rows keyed (relation, fixed entity) for either side
    known = KnownPairs((ki, torch.zeros_like(keep)), 37, c.R)
    fixed = torch.tensor([4, 9], device=gpu)
    r = torch.tensor([0, 1], device=gpu)
    scores, ids = m.top_k(fixed, r, 8, side=side, known=known)
    assert sorted(ids[0, :3].tolist()) == [0, 11, 36]
    assert ids[0, 3:].tolist() == [-1] * 5 and torch.isneginf(scores[0, 3:]).all()
    assert (ids[1] >= 0).all() and torch.isfinite(scores[1]).all()
    s64 = rc.scores64(model, c.ent.to(gpu), c.rel.to(gpu), fixed, r, c.gamma, side)
    val, idx = rc.ref_topk(s64, rc.known_mask(fixed, r, 37, rc.known_keys([(ki, torch.zeros_like(keep))], 37)), 8)
    assert torch.equal(ids, idx) and torch.equal(scores.to(torch.float64), val)


# ---- 3: the true score is the scan's value (rule 2) --------------------------------------------------------------------------
@pytest.mark.parametrize("n,H", [(17, 8), (50, 36), (64, 64)])
@pytest.mark.parametrize("side", rc.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_rank_agrees_with_top_k_bits(gpu, model, side, n, H):
    c = rc.ranking_case(model, n, H, n + H, False, Q=500, R=4)
    m = model_of(c, gpu)
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    fixed, truth = rc.split(sample, side)
    greater, ties = m.rank(sample, et, side=side)
    scores, ids = m.top_k(fixed, et, n, side=side)
    assert (ids >= 0).all()
    s_true = scores.gather(1, torch.argsort(ids, dim=1)).gather(1, truth.unsqueeze(1))      # score of the true candidate
    other = ids != truth.unsqueeze(1)
    assert torch.equal(greater.long(), ((scores > s_true) & other).sum(1))
    assert torch.equal(ties.long(), ((scores == s_true) & other).sum(1))


# ---- 4: equal rows tie wherever they lie (rule 1) ----------------------------------------------------------------------------
@pytest.mark.parametrize("side", rc.SIDES)
@pytest.mark.parametrize("model", ["RotatE", "ComplEx"])
def test_equal_rows_tie_across_stages_and_windows(gpu, model, side):
    n, H, R = 2113, 32, 5
    c = rc.ranking_case(model, n, H, 77, False, R=R)
    firsts = (5, 100, 700, 1000)
    for i in firsts:
        c.ent[i + 1024 + 37] = c.ent[i]                          # another stage, another lane, (for 1000) another window
    m = model_of(c, gpu)
    gen = torch.Generator().manual_seed(3)
    q = 64
    true = torch.tensor([firsts[j % 4] + (1024 + 37) * ((j // 4) % 2) for j in range(q)])
    twin = torch.where(true >= 1024 + 37, true - (1024 + 37), true + 1024 + 37)
    fixed = torch.randint(0, n, (q,), generator=gen)
    et = torch.randint(0, R, (q,), generator=gen).to(gpu)
    sample = (torch.stack([fixed, true]) if side == "tail" else torch.stack([true, fixed])).to(gpu)
    fixed, true, twin = fixed.to(gpu), true.to(gpu), twin.to(gpu)
    g0, t0 = m.rank(sample, et, side=side)
    only_twin = KnownPairs((torch.stack([fixed, twin]), et), n, R)  # rows keyed (relation, fixed entity)
    g1, t1 = m.rank(sample, et, side=side, known=only_twin)
    assert (t0 >= 1).all()
    assert torch.equal(g1, g0) and torch.equal(t1, t0 - 1)          # the twin was a tie, not a "greater"
    # top-k over ten candidates that include both twins: everything else is filtered
    keep = torch.stack([true, twin, *[(true + d) % n for d in (1, 2, 3, 50, 64, 2047, 2048, 1500)]], 1)      # [q, 10]
    drop = torch.ones(q, n, dtype=torch.bool, device=gpu).scatter_(1, keep, False)
    rows, cols = drop.nonzero(as_tuple=True)
    known = KnownPairs((torch.stack([fixed[rows], cols]), et[rows]), n, R)
    scores, ids = m.top_k(fixed, et, 16, side=side, known=known)
    left = (~drop).sum(1)
    bits = scores.view(torch.int32)
    for j in range(q):
        row = ids[j, :int(left[j])].tolist()
        assert sorted(row) == sorted(set(keep[j].tolist())) and ids[j, int(left[j]):].eq(-1).all()
        a, b = row.index(int(min(true[j], twin[j]))), row.index(int(max(true[j], twin[j])))
        assert b == a + 1                                            # equal scores: ascending ids, side by side
        assert bits[j, a] == bits[j, b]


# ---- 5: bounded ----------------------------------------------------------------------------------------------------------------
BOUNDED = [("RotatE", n, H) for n in NS for H in (8, 36, 64)] + [(mm, 645, H) for mm in ("ComplEx", "DistMult") for H in (8, 36)]


def bounded_side(c, m, sample, et, side, lists, dev, k=10):
    """The bounded checks of one side; returns (undecided candidates, largest top-k |error| / tol)."""
    fixed, truth = rc.split(sample, side)
    ent, rel = c.ent.to(dev), c.rel.to(dev)
    s64 = rc.scores64(c.model, ent, rel, fixed, et, c.gamma, side)
    tol = rc.tolerance(c.model, c.H, ent, rel, fixed, et, c.gamma, side)
    mask = rc.known_mask(fixed, et, c.n, rc.known_keys(rc.lists_for(lists, side), c.n))
    _, _, undecided = rc.rank_bounds(s64, tol, truth, mask)
    assert undecided <= 0.01 * s64.numel(), (undecided, s64.numel())     # from the reference alone, before any kernel output
    known = KnownPairs(on(dev, rc.lists_for(lists, side)), c.n, c.R) if lists else None
    greater, ties = m.rank(sample, et, side=side, known=known)
    rc.check_rank_bounded(s64, tol, truth, mask, greater, ties)
    scores, ids = m.top_k(fixed, et, k, side=side, known=known)
    return undecided, rc.check_top_k_bounded(s64, tol, mask, scores, ids)


@pytest.mark.parametrize("model,n,H", BOUNDED)
def test_bounded(gpu, model, n, H):
    c = rc.ranking_case(model, n, H, 500 + n + H, False)
    m = model_of(c, gpu)
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    for side in rc.SIDES:
        undecided, worst = bounded_side(c, m, sample, et, side, c.lists, gpu)
        print("{} n={} H={} {}: undecided {} of {} (cap 1 %), top-k |err| / tol = {:.3f} (bound 1)".format(
            model, n, H, side, undecided, sample.shape[1] * n, worst))
    _hip.raise_if_index_errors(gpu)


# ---- 6: size ---------------------------------------------------------------------------------------------------------------------
def test_size_pose0(gpu):
    data = make_rgcn_pose("pose0-syn")
    n, R, H = int(data.n_node), int(data.n_edge_type), 32
    ei, et_all = data.train_idx.to(gpu), data.train_et.to(gpu)
    e = ei.shape[1]
    pick = torch.randint(0, e, (2000,), generator=torch.Generator().manual_seed(3)).to(gpu)
    sample, et = ei[:, pick].contiguous(), et_all[pick].contiguous()
    chunk = 90                                                         # float64 [90, 19726, 64]: 0.9 GB
    for model in ("RotatE", "TransE"):
        gen = torch.Generator().manual_seed(2)
        ent, rel = rc.random_tables(model, n, R, H, gen)
        c = SimpleNamespace(model=model, n=n, R=R, H=H, gamma=rc.GAMMA, ent=ent, rel=rel)
        m = model_of(c, gpu)
        ent, rel = ent.to(gpu), rel.to(gpu)
        for side in rc.SIDES:
            lists = rc.lists_for([(ei, et_all)], side)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            free0 = torch.cuda.mem_get_info(gpu)[0]
            known = KnownPairs(lists, n, R)
            greater, ties = m.rank(sample, et, side=side, known=known)
            fixed, truth = rc.split(sample, side)
            scores, ids = m.top_k(fixed[:chunk], et[:chunk], 10, side=side, known=known)
            torch.cuda.synchronize()
            held = (greater, ties, scores, ids)
            torch.cuda.empty_cache()
            kept = free0 - torch.cuda.mem_get_info(gpu)[0]
            assert kept <= 4 * (R * n + 1) + 4 * e + (64 << 20), kept  # O(E + R n): no [Q, n] or [Q, n, D] block is held
            keys = rc.known_keys(lists, n)
            undecided = 0
            for a in range(0, sample.shape[1], chunk):
                f, t, r = fixed[a:a + chunk], truth[a:a + chunk], et[a:a + chunk]
                s64 = rc.scores64(model, ent, rel, f, r, c.gamma, side)
                tol = rc.tolerance(model, H, ent, rel, f, r, c.gamma, side)
                mask = rc.known_mask(f, r, n, keys)
                undecided += rc.rank_bounds(s64, tol, t, mask)[2]
                rc.check_rank_bounded(s64, tol, t, mask, greater[a:a + chunk], ties[a:a + chunk])
                if a == 0:
                    worst = rc.check_top_k_bounded(s64, tol, mask, scores, ids)
            print("{} {} at n={}: undecided {} of {}, top-k |err| / tol = {:.3f}".format(
                model, side, n, undecided, sample.shape[1] * n, worst))
            del known, held
    _hip.raise_if_index_errors(gpu)


# ---- 7: capture --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["RotatE", "ComplEx"])
def test_rank_and_top_k_capture(gpu, model):
    c = rc.ranking_case(model, 645, 36, 7, False)
    m = model_of(c, gpu)
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    known = {side: known_of(c, "full", side, gpu) for side in rc.SIDES}

    def run():
        out = []
        for side in rc.SIDES:
            out += m.rank(sample, et, side=side, known=known[side])
            out += m.top_k(rc.split(sample, side)[0], et, 10, side=side, known=known[side])
        return out

    eager = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)


# ---- 8: errors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["TransE", "ComplEx"])
def test_out_of_range_ids_raise_at_the_check(gpu, model):
    c = rc.ranking_case(model, 37, 8, 9, True)
    m = model_of(c, gpu)
    sample, et = c.sample.to(gpu), c.et.to(gpu)
    _hip.raise_if_index_errors(gpu)
    for side in rc.SIDES:
        bad_i, bad_t = sample.clone(), et.clone()
        bad_i[1, 3] = 37                                             # an entity id == n
        bad_t[5] = c.R                                               # a relation id == R
        greater, ties = m.rank(bad_i, bad_t, side=side)
        assert greater[3].item() == -1 and ties[3].item() == -1 and greater[5].item() == -1 and ties[5].item() == -1
        assert (greater[:3] >= 0).all()
        with pytest.raises(IndexError):
            utils.ranking_metrics(greater, ties, bad_t.clamp(max=c.R - 1), c.R)
        greater, ties = m.rank(sample, et, side=side)              # the next call is clean
        utils.ranking_metrics(greater, ties, et, c.R)
        fixed = rc.split(sample, side)[0].clone()
        fixed[2] = 37
        bad_t = et.clone()
        bad_t[4] = c.R
        scores, ids = m.top_k(fixed, bad_t, 4, side=side)
        assert (ids[2] == -1).all() and torch.isnan(scores[2]).all() and (ids[4] == -1).all() and torch.isnan(scores[4]).all()
        assert (ids[0] >= 0).all()
        with pytest.raises(IndexError):
            _hip.raise_if_index_errors(gpu)
        _hip.raise_if_index_errors(gpu)


def test_bad_side_k_filter_and_width(gpu):
    m = gripnet_amd.KGEModel("TransE", 5, 3, 8, 12.0).to(gpu)
    ei = torch.zeros(2, 4, dtype=torch.long, device=gpu)
    et = torch.zeros(4, dtype=torch.long, device=gpu)
    with pytest.raises(ValueError):
        m.rank(ei, et, side="both")
    with pytest.raises(ValueError):
        m.top_k(ei[0], et, 3, side="left")
    for k in (0, 65):
        with pytest.raises(ValueError):
            m.top_k(ei[0], et, k)
    known = KnownPairs((ei, et), 6, 3)                               # built for 6 entities
    with pytest.raises(ValueError):
        m.rank(ei, et, known=known)
    with pytest.raises(ValueError):
        m.top_k(ei[0], et, 3, known=KnownPairs((ei, et), 5, 4))      # built for 4 relations
    wide = gripnet_amd.KGEModel("ComplEx", 5, 3, 65, 12.0).to(gpu)     # entity rows of 130 floats
    with pytest.raises(ValueError, match="128"):
        wide.rank(ei, et)
    with pytest.raises(ValueError, match="128"):
        wide.top_k(ei[0], et, 3)
    gripnet_amd.KGEModel("ComplEx", 5, 3, 64, 12.0).to(gpu).rank(ei, et)   # the limit itself is served
    _hip.raise_if_index_errors(gpu)
