"""The poisoned ranking cases of tests/nonfinite_rank_cases.py held to their conditions from the float64 reference alone (no
GPU), so that a pass of tests/test_gpu_nonfinite_ranking.py means something:

  * the fp32 torch formulation of the scores equals the float64 one element for element, NaN positions included (the tables
    are exact, poison and all: the GPU comparison needs no tolerance);
  * per (model, n, H), over the poisons and sides: every non-finite class the model can produce (NaN and -inf; +inf for
    DistMult / ComplEx / the decoder only - TransE and RotatE never reach it, asserted) occurs at least FLOOR times among
    the true scores and among the admitted candidates, unranged and with typed_candidates_cases.ranges(n); at least FLOOR
    non-finite candidates are removed by the filter and at least FLOOR by the range;
  * per (model, n, H, poison, side): `greater` of the contract differs from the rule s(c) > s(true) that the kernels had
    before for at least FLOOR queries - the GPU tests fail on such kernels - and at least 100 of the 300 queries have a clean
    fixed entity and a finite true score;
  * a query with valid ids has a top-k row that is all padding; the flood case has more than 64 admitted +inf candidates;
  * the vectorised references equal a plain double loop on kge_rank_cases.tiny_case with one poisoned row per value."""
import math

import pytest
import torch

import kge_cases as kc
import kge_rank_cases as rc
import nonfinite_rank_cases as nf

FLOOR = 4


def same_with_nan(a32, b64):
    a = a32.double()
    return bool((torch.isnan(a) == torch.isnan(b64)).all()) and bool((a == b64)[~torch.isnan(b64)].all())


@pytest.mark.parametrize("model,n,H", nf.CASES)
def test_cases_meet_their_conditions(model, n, H):
    c = nf.case(model, n, H)
    out = nf.outside(c)
    cols = torch.arange(n).unsqueeze(0)
    true_count = {(cl, rg): 0 for cl in nf.classes(model) for rg in (False, True)}
    cand_count = dict(true_count)
    by_filter = by_range = padded = 0
    for side in nf.sides(model):
        fixed, truth = rc.split(c.sample, side)
        known = nf.masks(c, side)
        other = cols != truth.unsqueeze(1)
        clean64 = nf.scores(model, c.ent, c.rel, fixed, c.et, c.gamma, side)
        clean32 = nf.scores(model, c.ent, c.rel, fixed, c.et, c.gamma, side, torch.float32)
        assert torch.isfinite(clean64).all() and torch.equal(clean32.double(), clean64)
        before = (c.ent.clone(), c.rel.clone())
        for poison in nf.poisons(model):
            s64 = nf.poisoned_scores(c, side, poison, clean64)
            s32 = nf.poisoned_scores(c, side, poison, clean32, torch.float32)
            assert s32.dtype == torch.float32 and same_with_nan(s32, s64), (side, poison)
            if n == nf.NS[0]:                                         # the patched evaluation is the full one
                ent, rel = nf.poisoned(c, side, poison)
                assert same_with_nan(nf.scores(model, ent, rel, fixed, c.et, c.gamma, side), s64)
                assert same_with_nan(nf.scores(model, ent, rel, fixed, c.et, c.gamma, side, torch.float32), s64)
            if nf.scorer(model) in ("TransE", "RotatE"):
                assert not torch.isposinf(s64).any()                  # gamma - distance
            st = s64.gather(1, truth.unsqueeze(1)).squeeze(1)
            for ranged in (False, True):
                admitted = ~known["full"] & other & (~out if ranged else True)
                asked = admitted.any(1)                               # queries whose true score is compared at all
                for cl in nf.classes(model):
                    true_count[cl, ranged] += int((nf.in_class(st, cl) & asked).sum())
                    cand_count[cl, ranged] += int((nf.in_class(s64, cl) & admitted).sum())
            bad = ~torch.isfinite(s64) & other
            by_filter += int((bad & known["full"]).sum())
            by_range += int((bad & ~known["full"] & out).sum())
            # the contract against the rule before it, without filter and ranges
            none = torch.zeros_like(bad)
            g_new, t_new = nf.ref_rank(s64, truth, none)
            differs = int((g_new != nf.old_rule_greater(s64, truth, none)).sum())
            assert differs >= FLOOR, (side, poison, differs)
            if poison != "D+inf@col":                                 # (no entity row is poisoned there)
                assert int(nf.clean_queries(c, side, s64).sum()) >= 100, (side, poison)
            val, idx = nf.ref_topk(s64, none, 10)
            padded += int((idx == -1).all(1).sum())
            assert not torch.isnan(val).any() and bool(((idx >= 0) == ~torch.isneginf(val)).all())
        assert torch.equal(c.ent, before[0]) and torch.equal(c.rel, before[1])     # the case's tensors are never written
    for key, count in true_count.items():
        assert count >= FLOOR, ("true scores", key, count)
    for key, count in cand_count.items():
        assert count >= FLOOR, ("admitted candidates", key, count)
    assert by_filter >= FLOOR and by_range >= FLOOR, (by_filter, by_range)
    assert padded >= 1                                                # an all-padding row while the ids are valid


@pytest.mark.parametrize("model", ("DistMult", "ComplEx", "decoder"))
@pytest.mark.parametrize("H", (8, 36))
def test_flood_fills_a_list_with_equal_infinities(model, H):
    c = nf.case(model, nf.FLOOD_N, H)
    ent, rel = nf.flood(c)
    assert int(torch.isposinf(ent[:, nf.COLUMN]).sum()) >= 80
    stages = torch.isposinf(ent[:, nf.COLUMN]).nonzero().flatten() // 64
    assert stages.unique().numel() == -(-nf.FLOOD_N // 64)             # spread over every stage
    for side in nf.sides(model):
        fixed, truth = rc.split(c.sample, side)
        s64 = nf.scores(model, ent, rel, fixed, c.et, c.gamma, side)
        assert same_with_nan(nf.scores(model, ent, rel, fixed, c.et, c.gamma, side, torch.float32), s64)
        known = nf.masks(c, side)["full"]
        admitted = ~known & (torch.arange(c.n).unsqueeze(0) != truth.unsqueeze(1))
        assert int((torch.isposinf(s64) & admitted).sum(1).max()) > nf.FLOOD_K, side
        val, idx = nf.ref_topk(s64, known, nf.FLOOD_K)
        full = torch.isposinf(val).all(1)
        assert int(full.sum()) >= FLOOR                               # lists of nothing but +inf ...
        assert bool((idx[full][:, 1:] > idx[full][:, :-1]).all())     # ... ordered by id alone
        g, t = nf.ref_rank(s64, truth, known)
        assert int((t > nf.FLOOD_K).sum()) >= 1                       # a +inf true score ties with all of them


# ---- the vectorised references against a double loop ----------------------------------------------------------------------
def loop_reference(s, truth, mask, k):
    """greater, ties and the top-k list of every query by the contract's words, element by element."""
    out = []
    for q in range(s.shape[0]):
        st = float(s[q, truth[q]])
        greater = ties = 0
        entries = []
        for v in range(s.shape[1]):
            if mask[q, v]:
                continue
            x = float(s[q, v])
            if v != truth[q]:
                if math.isnan(x) or math.isnan(st) or x > st:
                    greater += 1
                elif x == st:
                    ties += 1
            if not math.isnan(x) and x != float("-inf"):
                entries.append((x, v))
        entries.sort(key=lambda sv: (-sv[0], sv[1]))
        entries = entries[:k] + [(float("-inf"), -1)] * (k - len(entries))
        out.append((greater, ties, entries[:k]))
    return out


@pytest.mark.parametrize("value", ("nan", "+inf", "-inf", "+inf@col"))
@pytest.mark.parametrize("side", rc.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_references_agree_with_a_double_loop(model, side, value):
    c = rc.tiny_case(model)
    ent = c.ent.clone()
    if value == "+inf@col":
        ent[2, 1] = float("inf")
    else:
        ent[2] = nf._value(value)                                     # entity 2: fixed, true and candidate in the tiny case
    fixed, truth = rc.split(c.sample, side)
    s64 = nf.scores(model, ent, c.rel, fixed, c.et, c.gamma, side)
    assert not torch.isfinite(s64).all()
    for lists in ([], c.lists):
        mask = rc.known_mask(fixed, c.et, c.n, rc.known_keys(rc.lists_for(lists, side), c.n))
        greater, ties = nf.ref_rank(s64, truth, mask)
        val, idx = nf.ref_topk(s64, mask, 5)
        want = loop_reference(s64, truth.tolist(), mask, 5)
        assert greater.tolist() == [w[0] for w in want] and ties.tolist() == [w[1] for w in want]
        assert idx.tolist() == [[v for _, v in w[2]] for w in want]
        assert val.tolist() == [[x for x, _ in w[2]] for w in want]
        # the shared references of the finite tests now state the same top-k contract
        val2, idx2 = rc.ref_topk(s64, mask, 5)
        assert torch.equal(idx2, idx) and torch.equal(val2, val)
