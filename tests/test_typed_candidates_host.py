"""Per-relation candidate ranges without a GPU: utils.candidate_ranges, the ValueErrors of the five Python entry points
that take `candidates` (before they ask for a GPU), and the numpy model of the documented ranged draw
(tests/typed_candidates_cases.py: draw; tests/test_gpu_typed_candidates.py pins the kernel to it element for element)."""
import numpy as np
import pytest
import torch

import kge_loss_cases as lc
import typed_candidates_cases as tc
from gripnet_amd import KGEModel, kge, multiRelaInnerProductDecoder, utils


def test_candidate_ranges_values():
    full = utils.candidate_ranges(4, 19)
    assert full.dtype == torch.int64 and full.device.type == "cpu" and full.tolist() == [[0, 19]] * 4
    t = utils.candidate_ranges(6, 100, [(0, 3, 0, 10), (3, 4, 10, 100), (2, 3, 7, 7), (5, 5, 1, 2)])
    assert t.tolist() == [[0, 10], [0, 10], [7, 7], [10, 100], [0, 100], [0, 100]]      # later spans win; an empty span of relations
    assert utils.candidate_ranges(0, 5).shape == (0, 2)
    assert utils.candidate_ranges(np.int64(2), np.int64(3), [(np.int64(0), 1, 0, 3)], device="cpu").tolist() == [[0, 3], [0, 3]]
    assert utils.candidate_ranges(2, 5, [(0, 2, 5, 5), (1, 2, 0, 0)]).tolist() == [[5, 5], [0, 0]]


@pytest.mark.parametrize("spans", ([(0, 1, 4, 3)], [(0, 1, -1, 3)], [(0, 1, 0, 11)], [(0, 4, 0, 3)], [(-1, 2, 0, 3)], [(2, 1, 0, 3)],
                                   [(0, 1, 3)], [(0, 1, 0.0, 3)], [(0, 1, 0, True)]))
def test_candidate_ranges_refuses_bad_spans(spans):
    with pytest.raises(ValueError):
        utils.candidate_ranges(3, 10, spans)


def test_candidate_ranges_refuses_bad_sizes():
    for r, n in ((-1, 5), (3, -1), (2.0, 5), (True, 5)):
        with pytest.raises(ValueError):
            utils.candidate_ranges(r, n)


def _bad_tables(R):
    good = utils.candidate_ranges(R, 10)
    return (torch.zeros(R + 1, 2, dtype=torch.int64), torch.zeros(R, 3, dtype=torch.int64), torch.zeros(2 * R, dtype=torch.int64),
            good.to(torch.int32), good.double(), good.tolist(), torch.zeros(R, 2, dtype=torch.int64, device="meta"))


def test_kge_value_errors_come_before_the_gpu_check():
    model = KGEModel("TransE", 10, 3, 4, 12.0)
    sample, et = torch.zeros(2, 3, dtype=torch.long), torch.zeros(3, dtype=torch.long)
    for bad in _bad_tables(3):
        with pytest.raises(ValueError):
            model.rank(sample, et, candidates=bad)
        with pytest.raises(ValueError):
            model.top_k(sample[0], et, 2, side="head", candidates=bad)
    good = utils.candidate_ranges(3, 10)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.rank(sample, et, candidates=good)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.top_k(sample[0], et, 2, candidates=good.t().contiguous().t())      # not contiguous: accepted


def test_decoder_value_errors_come_before_the_gpu_check():
    dec = multiRelaInnerProductDecoder(4, 3)
    z, ei, et = torch.zeros(10, 4), torch.zeros(2, 3, dtype=torch.long), torch.zeros(3, dtype=torch.long)
    for bad in _bad_tables(3):
        with pytest.raises(ValueError):
            dec.rank(z, ei, et, candidates=bad)
        with pytest.raises(ValueError):
            dec.top_k(z, ei[0], et, 2, candidates=bad)
    good = utils.candidate_ranges(3, 10)
    with pytest.raises(RuntimeError, match="MI355X only"):
        dec.rank(z, ei, et, candidates=good)
    with pytest.raises(RuntimeError, match="MI355X only"):
        dec.top_k(z, ei[0], et, 2, candidates=good)


def test_sampler_value_errors_come_before_the_gpu_check():
    positive, et = torch.zeros(2, 3, dtype=torch.long), torch.zeros(3, dtype=torch.long)
    for bad in _bad_tables(3)[1:]:                                  # without `known` the table's row count is the relation count
        with pytest.raises(ValueError):
            kge.sample_candidates(positive, et, 4, 10, candidates=bad)
    with pytest.raises(RuntimeError, match="MI355X only"):
        kge.sample_candidates(positive, et, 4, 10, candidates=utils.candidate_ranges(7, 10))


def test_the_ranged_model_with_a_full_range_is_the_documented_draw():
    """(0, n) gives kge_loss_cases.draw element for element, with and without known rows, flags and attempts included."""
    n, B, K = 37, 5, 65
    gen = np.random.default_rng(3)
    fixed, et = gen.integers(0, n, B), gen.integers(0, 3, B)
    rows = {(int(et[b]), int(fixed[b])): set(gen.integers(0, n, 12).tolist()) for b in range(B)}
    full = utils.candidate_ranges(3, n)
    for r in (None, rows):
        for seed, step in ((0, 0), (1111, 4)):
            want = lc.draw(fixed, et, K, n, seed, r, 3, step=step)
            got = tc.draw(fixed, et, K, n, seed, full, r, step=step)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    bad = tc.draw([0, 37, 2, 3], [0, 0, 3, 1], 4, n, 0, [(0, n), (5, 5), (3, 2)])
    assert bad[1] == 3 and bool((bad[0][1:] == -1).all()) and bool((bad[0][0] >= 0).all())
    assert tc.draw([1], [0], 4, n, 0, [(-1, 5)])[1] == 1 and tc.draw([1], [0], 4, n, 0, [(3, n + 1)])[1] == 1


def test_the_ranged_draw_is_uniform_over_the_admitted_entities():
    """n = 37, B = 8, K = 4,096, seed 0, range [10, 30) for relation 0; the even rows know {3, 12, 17, 29, 36} (two of them
    outside the range), the odd rows nothing: 16,384 draws per group.  Pearson's chi-square against the uniform distribution
    over the admitted entities stays below the 99.9 % quantile: 39.25 at 16 degrees of freedom (filtered: 17 entities),
    43.82 at 19 (plain: 20).  Measured: 23.1 and 15.4 (seeds 1 and 1111: 18.8 / 19.3 and 7.8 / 18.8).  No known and no
    out-of-range entity is drawn, and no element goes beyond attempt a = 6 (measured: 4)."""
    n, B, K = 37, 8, 4096
    lo, hi = 10, 30
    known = {3, 12, 17, 29, 36}
    fixed, et = np.arange(B), np.zeros(B, dtype=np.int64)
    rows = {(0, b): known for b in range(0, B, 2)}
    cand, flags, most = tc.draw(fixed, et, K, n, 0, [(lo, hi)], rows)
    assert flags == 0 and most <= 6, (flags, most)
    filtered = np.bincount(cand[0::2].reshape(-1), minlength=n)
    plain = np.bincount(cand[1::2].reshape(-1), minlength=n)
    assert filtered.sum() == plain.sum() == 16384
    inside = np.arange(lo, hi)
    assert filtered[:lo].sum() == filtered[hi:].sum() == plain[:lo].sum() == plain[hi:].sum() == 0
    assert all(filtered[e] == 0 for e in known)
    allowed = np.array([e for e in inside if e not in known])
    assert len(allowed) == 17
    chi_filtered, chi_plain = lc.chi_square(filtered, allowed), lc.chi_square(plain, inside)
    print("chi-square: filtered {:.1f} (< 39.25), plain {:.1f} (< 43.82), last attempt a = {}".format(chi_filtered, chi_plain, most))
    assert chi_filtered < 39.25 and chi_plain < 43.82
