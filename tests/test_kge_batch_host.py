"""The candidate-block modes of KGEModel without a GPU: the expansion that defines their reference, the loss on raw scores
against its formula in float64, and the refusals of the module (an unknown mode, candidates of the wrong shape)."""
import math

import pytest
import torch

import gripnet_amd
import kge_batch_cases as kb
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
