"""Filtered ranking without a GPU: ranking_metrics against numpy, the CPU refusal of rank / top_k, and the register budget
of the ranking kernels read from the gfx950 code objects."""
import os
import sys

import numpy as np
import pytest
import torch

from gripnet_amd import _hip, utils
from gripnet_amd.decoder import KnownPairs, multiRelaInnerProductDecoder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranking_metrics_matches_numpy():
    rng = np.random.RandomState(3)
    e, num_et = 500, 7
    greater = rng.randint(0, 30, e)
    ties = rng.randint(0, 4, e)
    et = rng.randint(0, num_et - 1, e)                      # the last relation has no queries
    got = utils.ranking_metrics(torch.from_numpy(greater).int(), torch.from_numpy(ties).int(), torch.from_numpy(et), num_et,
                                hits=(1, 3, 10))
    rank = 1.0 + greater + ties / 2.0
    for r in range(num_et):
        sel = et == r
        want_mrr = (1.0 / rank[sel]).mean() if sel.any() else np.nan
        assert got["mrr"].dtype == torch.float64
        np.testing.assert_allclose(got["mrr"][r].item(), want_mrr, rtol=1e-12, equal_nan=True)
        for k in (1, 3, 10):
            want = (rank[sel] <= k).mean() if sel.any() else np.nan
            np.testing.assert_allclose(got["hits@{}".format(k)][r].item(), want, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(got["mrr_all"].item(), (1.0 / rank).mean(), rtol=1e-12)
    for k in (1, 3, 10):
        np.testing.assert_allclose(got["hits@{}_all".format(k)].item(), (rank <= k).mean(), rtol=1e-12)


def test_ranking_metrics_realistic_rank_of_ties():
    # one query with 2 above and 2 tied: rank 1 + 2 + 1 = 4
    got = utils.ranking_metrics(torch.tensor([2], dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
                                torch.tensor([0]), 1, hits=(3, 4))
    assert got["mrr_all"].item() == 0.25
    assert got["hits@3_all"].item() == 0.0 and got["hits@4_all"].item() == 1.0


def test_rank_and_top_k_refuse_cpu_tensors():
    dec = multiRelaInnerProductDecoder(8, 3)
    z = torch.zeros(5, 8)
    ei = torch.zeros(2, 4, dtype=torch.long)
    et = torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="MI355X only"):
        dec.rank(z, ei, et)
    with pytest.raises(RuntimeError, match="MI355X only"):
        dec.top_k(z, ei[0], et, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        KnownPairs((ei, et), 5, 3)


def test_top_k_rejects_bad_k_before_touching_the_device():
    dec = multiRelaInnerProductDecoder(8, 3)
    for k in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            dec.top_k(torch.zeros(5, 8), torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long), k)


def test_ranking_kernels_register_budgets():
    """Every instantiation of the score engine (4 S features, S = 4 .. 32; rank and top-k epilogues) keeps its A operand,
    the two interleaved chains and the epilogue in registers: no scratch, no spills."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources(_hip.library_path())
    for s in range(4, 33, 4):
        for topk in ("false", "true"):
            name = "k_dm_rank<{}, {}>".format(s, topk)
            assert name in res, (name, sorted(k for k in res if "dm_rank" in k))
            r = res[name]
            assert r[".private_segment_fixed_size"] == 0, (name, r)
            assert r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (name, r)
            assert r[".vgpr_count"] + r.get(".agpr_count", 0) <= (128 if topk == "false" else 256), (name, r)
    for name in ("k_known_keys", "k_known_rows", "k_known_partners"):
        assert name in res, name
