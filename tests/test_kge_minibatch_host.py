"""The KGE mini-batch path without a GPU: the numpy model of the documented candidate draw is uniform over the entities a
row does not know (tests/test_gpu_kge_candidates.py pins the kernel to this model element for element), and the three
Python entry points refuse bad shapes with ValueError before they ask for a GPU."""
import numpy as np
import pytest
import torch

import kge_loss_cases as lc
from gripnet_amd import KGEModel
from gripnet_amd import kge


def test_the_documented_draw_is_uniform_over_the_unknown_entities():
    """n = 37, B = 8, K = 4,096, seed 0; the even rows know {3, 4, 5, 17, 36}, the odd rows nothing: 16,384 draws per group.
    Pearson's chi-square against the uniform distribution stays below the 99.9 % quantile: 61.1 at 31 degrees of freedom
    (filtered), 68.0 at 36 (plain).  Measured: 39.3 and 23.5 (seeds 1 and 1111: 45.3 / 42.6 and 34.5 / 39.5).  No known
    entity is drawn, and no element goes beyond attempt a = 5."""
    n, B, K = 37, 8, 4096
    known = {3, 4, 5, 17, 36}
    fixed, et = np.arange(B), np.zeros(B, dtype=np.int64)
    rows = {(0, b): known for b in range(0, B, 2)}
    cand, flags, most = lc.draw(fixed, et, K, n, 0, rows)
    assert flags == 0 and most <= 5, (flags, most)
    filtered = np.bincount(cand[0::2].reshape(-1), minlength=n)
    plain = np.bincount(cand[1::2].reshape(-1), minlength=n)
    assert filtered.sum() == plain.sum() == 16384
    assert all(filtered[e] == 0 for e in known)
    allowed = np.array([e for e in range(n) if e not in known])
    chi_filtered, chi_plain = lc.chi_square(filtered, allowed), lc.chi_square(plain, np.arange(n))
    print("chi-square: filtered {:.1f} (< 61.1), plain {:.1f} (< 68.0), last attempt a = {}".format(chi_filtered, chi_plain, most))
    assert chi_filtered < 61.1 and chi_plain < 68.0


def test_the_model_without_a_filter_takes_attempt_zero_and_steps_with_the_seed():
    fixed, et = np.array([0, 1, 2]), np.array([0, 0, 1])
    plain, flags, most = lc.draw(fixed, et, 7, 37, 5)
    assert flags == 0 and most == 0 and plain.min() >= 0 and plain.max() < 37
    assert np.array_equal(lc.draw(fixed, et, 7, 37, 2, step=3)[0], plain)
    bad, flags, _ = lc.draw(np.array([0, 37, -1]), et, 7, 37, 5)
    assert flags == 1 and np.array_equal(bad[0], plain[0]) and bool((bad[1:] == -1).all())


def test_one_entity_left_and_none_left():
    """n = 8, seed 5, K = 64: a row that knows 0..6 draws 7 everywhere by attempt a = 40; one that knows all 8 exhausts the cap."""
    cand, flags, most = lc.draw([2], [1], 64, 8, 5, {(1, 2): set(range(7))})
    assert flags == 0 and most <= 40 and bool((cand == 7).all()), (flags, most)
    _, flags, most = lc.draw([2], [1], 2, 8, 5, {(1, 2): set(range(8))})
    assert flags == 2 and most == lc.MAX_ATTEMPTS - 1


def test_loss_value_errors_come_before_the_gpu_check():
    pos, neg = torch.zeros(3), torch.zeros(3, 4)
    for p, n, t, w in ((torch.zeros(3, 1), neg, None, None), (torch.zeros(0), torch.zeros(0, 4), None, None), (pos, torch.zeros(3), None, None),
                       (pos, torch.zeros(2, 4), None, None), (pos, torch.zeros(3, 0), None, None), (pos, neg, None, torch.zeros(4)),
                       (pos, neg, "1", None), (pos, neg, True, None)):
        with pytest.raises(ValueError):
            kge.negative_sampling_loss(p, n, t, w)
    with pytest.raises(RuntimeError, match="MI355X only"):
        kge.negative_sampling_loss(pos, neg, 1.0, torch.ones(3))


def test_model_loss_value_errors_come_before_the_gpu_check():
    model = KGEModel("TransE", 10, 3, 4, 12.0)
    positive, et, negatives = torch.zeros(2, 3, dtype=torch.long), torch.zeros(3, dtype=torch.long), torch.zeros(3, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="mode single not supported"):
        model.negative_sampling_loss(positive, et, negatives, mode="single")
    with pytest.raises(ValueError):
        model.negative_sampling_loss(positive, et, torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(ValueError):
        model.negative_sampling_loss(torch.zeros(3, 3, dtype=torch.long), et, negatives, mode="head-batch")
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.negative_sampling_loss(positive, et, negatives)


def test_sampler_value_errors_come_before_the_gpu_check():
    positive, et = torch.zeros(2, 3, dtype=torch.long), torch.zeros(3, dtype=torch.long)
    bad = (dict(side="both"), dict(positive=torch.zeros(3, 3, dtype=torch.long)), dict(et=torch.zeros(4, dtype=torch.long)),
           dict(K=0), dict(K=2.0), dict(K=True), dict(nentity=0), dict(nentity=2 ** 31), dict(step=torch.zeros(1)),
           dict(step=torch.zeros(2, dtype=torch.long)), dict(out=torch.zeros(3, 5, dtype=torch.long)),
           dict(out=torch.zeros(3, 4, dtype=torch.int32)), dict(out=torch.zeros(4, 3, dtype=torch.long).t()))
    for change in bad:
        args = dict(positive=positive, et=et, K=4, nentity=10)
        args.update(change)
        with pytest.raises(ValueError):
            kge.sample_candidates(**args)
    with pytest.raises(TypeError):
        kge.sample_candidates(positive, et, 4, 10, known=object())
    with pytest.raises(RuntimeError, match="MI355X only"):
        kge.sample_candidates(positive, et, 4, 10, step=torch.zeros(1, dtype=torch.long), out=torch.zeros(3, 4, dtype=torch.long))
