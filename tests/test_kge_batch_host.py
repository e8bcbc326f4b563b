"""The candidate-block modes of KGEModel without a GPU: the expansion that defines their reference, the loss on raw scores
against its formula in float64, the refusals of the module (an unknown mode, candidates of the wrong shape), and what the
gradient cases of tests/test_gpu_kge_batch.py are built to hold (rows across the chunks of the passes over the positives)."""
import math

import pytest
import torch

import gripnet_amd
import kge_batch_cases as kb
import kge_cases as kc
from gripnet_amd.kge import self_adversarial_loss


def test_expand_by_hand():
    """B = 2 positives, K = 3 candidates each, row-major (b, k)."""
    positive = torch.tensor([[10, 11], [20, 21]])
    et = torch.tensor([5, 6])
    negatives = torch.tensor([[1, 2, 3], [4, 5, 6]])
    sample, types = kb.expand(positive, et, negatives, "tail")
    assert sample.tolist() == [[10, 10, 10, 11, 11, 11], [1, 2, 3, 4, 5, 6]]
    assert types.tolist() == [5, 5, 5, 6, 6, 6]
    sample, types = kb.expand(positive, et, negatives, "head")
    assert sample.tolist() == [[1, 2, 3, 4, 5, 6], [20, 20, 20, 21, 21, 21]]
    assert types.tolist() == [5, 5, 5, 6, 6, 6]
    assert kb.fixed_of(positive, "tail").tolist() == [10, 11] and kb.fixed_of(positive, "head").tolist() == [20, 21]


def test_case_a_holds_what_it_promises():
    c = kb.case_a("TransE", "tail")
    assert c.sample.shape == (2, 5200) and c.E == 5200
    assert int((c.sample[1] == 0).sum()) == 2049 and int((c.sample[0] == 1).sum()) == 3 * c.K
    for b, k in c.same:
        assert int(c.et[b]) == 3 and int(c.negatives[b, k]) == int(c.positive[0, b])
    assert float(c.rel[3, 2]) == 0.0
    assert bool((c.et[1:] >= c.et[:-1]).all()) and set(c.et.tolist()) == {1, 2, 3, 4, 5}
    h = kb.case_a("RotatE", "head")
    assert int((h.sample[0] == 0).sum()) == 2049 and int((h.sample[1] == 1).sum()) == 3 * h.K


def _kinds(keys, rows, chunk=kb.ROW_CHUNK):
    """Which kinds of rows the passes over the positives meet when the records are in the order of `keys`."""
    counts = torch.bincount(keys, minlength=rows).tolist()
    straddlers = kb.straddling_rows(keys, chunk)
    kinds = set()
    touched = {}
    for key, (begin, end) in straddlers.items():
        kinds.add("straddler from inside a chunk" if begin % chunk else "straddler from a cut")
        first, last = begin // chunk, (end - 1) // chunk
        if last - first >= 2:
            kinds.add("whole interior chunk")
        for c in range(first, last + 1):
            touched.setdefault(c, set()).add(key)
    if any(len(rows_of) == 2 for rows_of in touched.values()):
        kinds.add("chunk with two straddlers")
    assert all(len(rows_of) <= 2 for rows_of in touched.values())   # (a chunk has one row that came in and one that goes on)
    begin = 0
    for key, count in enumerate(counts):
        if count == chunk and begin % chunk == 0:
            kinds.add("aligned one-chunk row")
        if count == 1:
            kinds.add("one-record row")
        if count == 0:
            kinds.add("empty row")
        begin += count
    if keys.numel() % chunk:
        kinds.add("short last chunk")
    return kinds, straddlers


@pytest.mark.parametrize("side", kb.SIDES)
def test_case_d_has_rows_across_chunks_of_every_kind(side):
    """Pins what kge_batch_cases.case_d is there for, so that an edit of the builder cannot lose it: in the order of the
    relation pass and in the order of the entity pass, rows of every kind the chunked reduction tells apart.  Case A, the
    only other gradient case with more positives than a chunk, has no such row in the relation pass and at most one
    two-record row in the entity pass: the reason for case D."""
    everything = {"straddler from inside a chunk", "straddler from a cut", "whole interior chunk", "chunk with two straddlers",
                  "aligned one-chunk row", "one-record row", "empty row", "short last chunk"}
    for shuffled in (False, True):
        c = kb.case_d("TransE", side, 8, shuffled)
        assert (c.n, c.R, c.K, c.B) == (90, 12, 5, 230) and c.B == 7 * kb.ROW_CHUNK + 6
        assert torch.bincount(c.et, minlength=c.R).tolist() == [0, 31, 2, 0, 31, 32, 0, 70, 1, 0, 33, 30]
        fixed = kb.fixed_of(c.positive, side)
        kinds, straddlers = _kinds(c.et, c.R)
        assert kinds == everything
        assert straddlers == {2: (31, 33), 7: (96, 166), 10: (167, 200), 11: (200, 230)}
        assert all(int(torch.bincount(c.et, minlength=c.R)[r]) == 0 for r in c.empty_relations)
        # the entity pass: the same cuts up to position 165, then single records and entity 80 across the last cut; no
        # chunk of it holds two straddlers (the counts leave entity 20's last chunk to rows of one record)
        kinds, straddlers = _kinds(fixed, c.n)
        assert kinds == everything - {"chunk with two straddlers"}
        assert straddlers == {4: (31, 33), 20: (96, 166), 80: (200, 230)}
        # rows of d_ent that get a candidate-pass sum and a straddling row-pass sum
        assert all(bool((c.negatives == e).any()) for e in (3, 4, 9, 20, 80))
        assert not bool((c.negatives == c.unused_entity).any()) and not bool((c.positive == c.unused_entity).any())
        # a real permutation for the entity pass's sort, and (shuffled) for the relation pass's
        assert not bool((fixed[1:] >= fixed[:-1]).all())
        assert bool((c.et[1:] >= c.et[:-1]).all()) == (not shuffled)
    # the two orders are one block: the sorted one is the stable sort of the shuffled one
    s, o = kb.case_d("RotatE", side, 35, True), kb.case_d("RotatE", side, 35, False)
    order = s.et.sort(stable=True).indices
    assert int((order != torch.arange(s.B)).sum()) > s.B // 2
    assert torch.equal(s.et[order], o.et) and torch.equal(s.positive[:, order], o.positive)
    assert torch.equal(s.negatives[order], o.negatives) and torch.equal(s.up[order], o.up)
    assert s.gamma == 1.0 and kb.case_d("RotatE", side, 72, True).gamma == 12.0
    # case A: no relation's row straddles, and no entity's - but for ComplEx's draw of the fixed entities, which puts the two
    # records of entity 46 on either side of position 32: a two-chunk row from inside a chunk, the one kind case A ever has
    across = {"straddler from inside a chunk", "straddler from a cut", "whole interior chunk", "chunk with two straddlers"}
    for model in kc.MODELS:
        a = kb.case_a(model, side)
        assert a.B > kb.ROW_CHUNK and kb.straddling_rows(a.et) == {}
        kinds, straddlers = _kinds(kb.fixed_of(a.positive, side), a.n)
        assert straddlers == ({46: (31, 33)} if model == "ComplEx" else {})
        assert kinds & across <= {"straddler from inside a chunk"}


def test_case_e_is_beyond_one_grid_of_the_query_kernel():
    for side in kb.SIDES:
        c = kb.case_e("DistMult", side)
        assert c.B == 256 * 64 + 1 and c.K == 2 and c.H == 4
        busiest = int(torch.bincount(c.et).max())
        assert 1750 <= busiest <= 1950                              # about B / R = 1 820: some 58 chunks in the combine
        assert len(kb.straddling_rows(c.et)) == c.R
        # K below CHUNK / ROW_CHUNK: the chunks of the passes over the positives size the workspace's partials
        assert c.K < kc.CHUNK // kb.ROW_CHUNK and c.B > kb.ROW_CHUNK


@pytest.mark.parametrize("side", kb.SIDES)
def test_the_bounds_take_the_depth_of_the_busiest_row(side, monkeypatch):
    """The GPU tests' c_g counts the additions of the longest path: query_reduction_depth must be asked for the busiest
    relation and the busiest fixed entity of the case at hand - 70 positives in case D, about 1 820 in case E."""
    import test_gpu_kge_batch as gpu_tests                          # (its helpers run on the CPU; its tests need the GPU)
    asked = []
    depth = kb.query_reduction_depth

    def recording(K, B_per_row, lanes):
        asked.append((K, B_per_row, lanes))
        return depth(K, B_per_row, lanes)

    monkeypatch.setattr(kb, "query_reduction_depth", recording)
    for H, lanes, by_hand in ((8, 8, 1 + 32 + 1 + 32 + 3 + 1), (72, 16, 1 + 16 + 2 + 16 + 3 + 1)):
        c = kb.case_d("DistMult", side, H, True)
        del asked[:]
        gpu_tests._gradient_bounds(c, c.sample, c.et_list, c.up.reshape(-1), True)
        assert asked == [(5, 70, lanes), (5, 70, lanes)]            # (the busiest fixed entity, the busiest relation)
        assert depth(5, 70, lanes) == by_hand
    c = kb.case_e("DistMult", side)
    busiest_rel = int(torch.bincount(c.et).max())
    busiest_fixed = int(torch.bincount(kb.fixed_of(c.positive, side)).max())
    del asked[:]
    gpu_tests._gradient_bounds(c, c.sample, c.et_list, torch.linspace(-1.0, 1.0, c.E), True)
    assert asked == [(2, busiest_fixed, 8), (2, busiest_rel, 8)]
    assert depth(2, busiest_rel, 8) == 1 + 32 + 1 + 32 + -(-busiest_rel // 32) + 1


def _log_sigmoid(x):
    return -math.log1p(math.exp(-x)) if x >= 0 else x - math.log1p(math.exp(x))


def _loss_by_hand(pos, neg, temperature):
    B, K = len(neg), len(neg[0])
    p = sum(_log_sigmoid(s) for s in pos) / B
    total = 0.0
    for row in neg:
        if temperature is None:
            total += sum(_log_sigmoid(-s) for s in row) / K
        else:
            top = max(s * temperature for s in row)
            w = [math.exp(s * temperature - top) for s in row]
            total += sum(wi / sum(w) * _log_sigmoid(-s) for wi, s in zip(w, row))
    return (-p - total / B) / 2


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("temperature", [None, 0.5, 2.0])
def test_self_adversarial_loss_element_by_element(K, temperature):
    gen = torch.Generator().manual_seed(3 + K)
    pos = torch.randn(4, generator=gen, dtype=torch.float64) * 3
    neg = torch.randn(4, K, generator=gen, dtype=torch.float64) * 3
    want = _loss_by_hand(pos.tolist(), neg.tolist(), temperature)
    got = self_adversarial_loss(pos, neg, temperature)
    assert got.shape == () and abs(float(got) - want) <= 1e-13 * max(1.0, abs(want))
    # the weights are constants: the gradient with respect to the negatives is that of the weighted sum alone
    n = neg.clone().requires_grad_(True)
    self_adversarial_loss(pos, n, temperature).backward()
    w = torch.full_like(neg, 1.0 / K) if temperature is None else torch.softmax(neg * temperature, dim=1)
    assert torch.allclose(n.grad, w * torch.sigmoid(neg) / (2 * 4), rtol=1e-12, atol=0)


def test_unknown_mode_and_candidate_shape_are_refused():
    model = gripnet_amd.KGEModel("TransE", 9, 3, 4, 12.0)
    positive = torch.zeros(2, 5, dtype=torch.long)
    et = torch.zeros(5, dtype=torch.long)
    for call in (model, model.score):
        with pytest.raises(ValueError, match="mode batch not supported"):
            call(positive, et, mode="batch")
        with pytest.raises(ValueError, match="mode tail_batch not supported"):
            call((positive, torch.zeros(5, 2, dtype=torch.long)), et, mode="tail_batch")
        for mode in ("tail-batch", "head-batch"):
            for bad in (torch.zeros(4, 2, dtype=torch.long), torch.zeros(5, dtype=torch.long), torch.zeros(5, 2, 1, dtype=torch.long)):
                with pytest.raises(ValueError, match=r"negatives must have shape \[5, K\]"):
                    call((positive, bad), et, mode=mode)
    # the accepted shapes get as far as the device check: these tables are on the CPU
    with pytest.raises(RuntimeError, match="MI355X only"):
        model((positive, torch.zeros(5, 2, dtype=torch.long)), et, mode="tail-batch")
