"""The float64 ranking references of tests/kge_rank_cases.py against a brute-force double loop over kge_cases.raw_score on a
7-entity, 2-relation case: both sides, with and without the filter, and the head-side filter convention (a filter keyed
(relation, tail) is built from the flipped lists)."""
import pytest
import torch

import kge_cases as kc
import kge_rank_cases as rc


def brute_force(c, side, known):
    """Per query: the float64 score of every candidate by one raw_score call each, the candidate set by membership in the
    python set `known` of (head, relation, tail) triples."""
    ent, rel = c.ent.double(), c.rel.double()
    out = []
    for e in range(c.sample.shape[1]):
        h, t, r = int(c.sample[0, e]), int(c.sample[1, e]), int(c.et[e])

        def triple(v):
            return (h, r, v) if side == "tail" else (v, r, t)

        def score(v):
            hh, rr, tt = triple(v)
            return float(kc.raw_score(c.model, ent, rel, torch.tensor([[hh], [tt]]), torch.tensor([rr]), c.gamma)[0])

        truth = t if side == "tail" else h
        s_true = score(truth)
        cands = [(score(v), v) for v in range(c.n) if triple(v) not in known]
        greater = sum(1 for s, v in cands if v != truth and s > s_true)
        ties = sum(1 for s, v in cands if v != truth and s == s_true)
        ordered = sorted(cands, key=lambda sv: (-sv[0], sv[1]))
        out.append((greater, ties, ordered))
    return out


def known_set(lists):
    return {(int(ei[0, i]), int(et[i]), int(ei[1, i])) for ei, et in lists for i in range(et.numel())}


@pytest.mark.parametrize("model", kc.MODELS)
@pytest.mark.parametrize("side", rc.SIDES)
@pytest.mark.parametrize("filtered", [False, True])
def test_references_agree_with_a_double_loop(model, side, filtered):
    c = rc.tiny_case(model)
    lists = c.lists if filtered else []
    fixed, truth = rc.split(c.sample, side)
    s64 = rc.scores64(model, c.ent, c.rel, fixed, c.et, c.gamma, side)
    mask = rc.known_mask(fixed, c.et, c.n, rc.known_keys(rc.lists_for(lists, side), c.n))
    greater, ties = rc.ref_rank(s64, truth, mask)
    val, idx = rc.ref_topk(s64, mask, 5)
    want = brute_force(c, side, known_set(lists))
    assert greater.tolist() == [w[0] for w in want] and ties.tolist() == [w[1] for w in want]
    for q, (_, _, ordered) in enumerate(want):
        top = ordered[:5]
        assert idx[q, :len(top)].tolist() == [v for _, v in top]
        assert val[q, :len(top)].tolist() == [s for s, _ in top]
        assert (idx[q, len(top):] == -1).all() and torch.isneginf(val[q, len(top):]).all()
    if filtered:
        assert int(mask.sum()) > 0
    assert int(ties.sum()) > 0                               # entities 2 and 6 share a row


def test_head_side_filter_is_keyed_by_relation_and_tail():
    """The known triple (h, r, t) = (4, 0, 2) removes head 4 from the candidates of (., 0, 2) - found under the key
    (r, t, h) of the flipped list - and tail 2 from those of (4, 0, .); a head-side lookup in the unflipped keys would
    ask for (r, t, h') = (0, 2, .), which holds the tails of HEAD 2 instead."""
    c = rc.tiny_case("TransE")
    fixed_t = torch.tensor([2])
    r = torch.tensor([0])
    head_mask = rc.known_mask(fixed_t, r, c.n, rc.known_keys(rc.lists_for(c.lists, "head"), c.n))
    assert head_mask[0].nonzero().flatten().tolist() == [0, 4]             # (0, 0, 2) and (4, 0, 2)
    wrong = rc.known_mask(fixed_t, r, c.n, rc.known_keys(c.lists, c.n))
    assert wrong[0].nonzero().flatten().tolist() == [0]                    # (2, 0, 0): a tail of head 2
    tail_mask = rc.known_mask(torch.tensor([4]), r, c.n, rc.known_keys(rc.lists_for(c.lists, "tail"), c.n))
    assert tail_mask[0].nonzero().flatten().tolist() == [2, 5]


@pytest.mark.parametrize("model", kc.MODELS)
def test_scan_depth_counts_the_chain(model):
    assert rc.scan_depth(model, 1) >= 1
    assert rc.scan_depth(model, 64) > rc.scan_depth(model, 8)
