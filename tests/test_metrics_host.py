"""What tests/test_gpu_link_metrics.py leans on, checked without a GPU: the float64 reference of tests/metric_cases.py agrees
with scikit-learn (utils.auprc_auroc_ap, called per relation the way the reference's epoch loop does) on every case, and
every case meets the condition it is built for."""
import numpy as np
import pytest
import torch

import metric_cases as mc
from gripnet_amd.utils import auprc_auroc_ap

SKLEARN_TOL = 1e-12


@pytest.mark.parametrize("name", list(mc.CASES))
def test_reference_matches_sklearn(name):
    pos, neg, sizes = mc.case(name)
    ref = mc.reference(name)
    assert ref.shape == (3, len(sizes))
    worst = 0.0
    for r, (s, e) in enumerate(mc.range_list(sizes).tolist()):
        if e == s:
            assert np.isnan(ref[:, r]).all()
            continue
        target = torch.cat([torch.ones(e - s), torch.zeros(e - s)])
        score = torch.cat([pos[s:e], neg[s:e]]).double()              # the same values: nothing in sklearn then rounds to fp32
        want = auprc_auroc_ap(target, score)
        worst = max(worst, max(abs(a - b) for a, b in zip(ref[:, r], want)))
        assert worst <= SKLEARN_TOL, "relation {} ({} edges): reference {} vs sklearn {}".format(r, e - s, ref[:, r].tolist(), want)
    print("reference-to-sklearn[{}]: {:.3g}".format(name, worst))


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_meets_its_condition(name):
    """The builder itself, not the shared copy: its assertions run here whatever ran before."""
    pos, neg, sizes = mc.CASES[name]()
    shared = mc.case(name)
    assert torch.equal(pos.view(torch.int32), shared[0].view(torch.int32)) and torch.equal(neg.view(torch.int32), shared[1].view(torch.int32))
    assert tuple(sizes) == shared[2]


def test_signed_zero_cases_are_the_listed_ones():
    assert [n for n in mc.CASES if mc.has_both_zeros(*mc.case(n)[:2])] == sorted(mc.SIGNED_ZERO_CASES, key=list(mc.CASES).index)


def test_reference_by_hand():
    """Three positives and three negatives worked out on paper, a tie between the classes included."""
    # thresholds 4, 3, 2, 1: (tp, fp) = (1, 0), (2, 1), (2, 2), (3, 3)
    auprc, auroc, ap = mc.ref_link_metrics([4.0, 3.0, 1.0], [3.0, 2.0, 1.0])
    assert ap == pytest.approx((1 / 3) * 1 + (1 / 3) * (2 / 3) + 0 + (1 / 3) * (3 / 6), abs=1e-15)
    assert auprc == pytest.approx((1 / 3) * 1 + (1 / 3) * (1 + 2 / 3) / 2 + (1 / 3) * (2 / 4 + 3 / 6) / 2, abs=1e-15)
    assert auroc == (0 + 1 * (1 + 2) + 1 * (2 + 2) + 1 * (2 + 3)) / (2 * 3 * 3)
    assert all(np.isnan(v) for v in mc.ref_link_metrics([], []))
    # the sign of a zero does not order it, a denormal does
    assert mc.ref_link_metrics(np.float32([-0.0]), np.float32([0.0]))[1] == 0.5
    assert mc.ref_link_metrics(np.float32([2.0 ** -149]), np.float32([0.0]))[1] == 1.0


def test_helpers_describe_the_geometry():
    assert mc.chunk_lengths(8193) == [4096, 4096, 1] and mc.sort_width(256) == 256 and mc.sort_width(257) == 1024
    assert mc.tile_windows(np.arange(2048.0), np.array([-1.0, 0.0, 1023.5, 1024.0, 2047.0, 3000.0])) == [2, 1]
    assert mc.tie_groups(np.array([1.0, 3.0, 3.0, 2.0, 3.0])) == [(0, 2), (3, 3), (4, 4)]
    got = np.array([[0.5, np.nan], [0.25, np.nan], [1.0, np.nan]])
    assert mc.distance(got, got) == 0.0 and mc.distance(got + 1e-3, got) == pytest.approx(1e-3)
    with pytest.raises(AssertionError, match="NaN"):
        mc.distance(np.nan_to_num(got), got)
