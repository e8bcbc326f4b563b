"""Node-classification metrics without a GPU: argument checks of utils.class_metrics that come before any device work,
the CPU refusal, the workspace query, and the resources of the two kernels read from the gfx950 code objects."""
import os
import sys

import pytest
import torch

from gripnet_amd import _hip, utils

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_class_metrics_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="MI355X only"):
        utils.class_metrics(torch.zeros(6, 4), torch.zeros(6, dtype=torch.long))
    with pytest.raises(RuntimeError, match="MI355X only"):
        utils.class_metrics(torch.zeros(6, dtype=torch.long), torch.zeros(6, dtype=torch.long), 4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        _hip.class_metrics(torch.zeros(6, 4), torch.zeros(6, dtype=torch.long))


@pytest.mark.parametrize("args, error", [
    ((torch.zeros(6, dtype=torch.long), torch.zeros(6, dtype=torch.long)), ValueError),             # pred mode: num_class missing
    ((torch.zeros(6, 0), torch.zeros(6, dtype=torch.long)), ValueError),                            # C = 0 (width)
    ((torch.zeros(6, dtype=torch.long), torch.zeros(6, dtype=torch.long), 0), ValueError),         # C = 0 (given)
    ((torch.zeros(6, 1025), torch.zeros(6, dtype=torch.long)), ValueError),                         # C = 1025 (width)
    ((torch.zeros(6, dtype=torch.long), torch.zeros(6, dtype=torch.long), 1025), ValueError),      # C = 1025 (given)
    ((torch.zeros(6, 4), torch.zeros(6, dtype=torch.long), 5), ValueError),                         # num_class != width
    ((torch.zeros(6, 4), torch.zeros(6, dtype=torch.int32)), TypeError),                            # non-int64 class ids
    ((torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.long), 4), TypeError),         # non-int64 predictions
    ((torch.zeros(6, 4, dtype=torch.float64), torch.zeros(6, dtype=torch.long)), TypeError),        # non-fp32 scores
    ((torch.zeros(6, 4), torch.zeros(5, dtype=torch.long)), ValueError),                            # length mismatch
    ((torch.zeros(6, dtype=torch.long), torch.zeros(7, dtype=torch.long), 4), ValueError),         # length mismatch
    ((torch.zeros(6, 4), torch.zeros(6, 1, dtype=torch.long)), ValueError),                         # classes not 1-D
    ((torch.zeros(2, 3, 4), torch.zeros(2, dtype=torch.long)), ValueError),                         # 3-D input
    ((torch.zeros(6, dtype=torch.long), torch.zeros(6, dtype=torch.long), True), ValueError),      # bool is no class count
])
def test_class_metrics_argument_errors_come_before_the_device(args, error):
    with pytest.raises(error):
        utils.class_metrics(*args)
    with pytest.raises(error):
        _hip.class_metrics(*args)


def test_class_metrics_workspace_query():
    lib = _hip.load()
    assert lib.gn_class_metrics_workspace_bytes(10_000, 0) == 0
    assert lib.gn_class_metrics_workspace_bytes(10_000, 1025) == 0
    assert lib.gn_class_metrics_workspace_bytes(-1, 8) == 0
    for n, c in ((0, 1), (1, 8), (10_000, 8), (1_000_003, 17), (63, 1024)):
        b = lib.gn_class_metrics_workspace_bytes(n, c)
        assert b > 0 and b % 16 == 0, (n, c, b)
    # one partial row of 3 C + 2 ints (padded to 16 bytes) per workgroup of the counting pass, at most 512 of them
    assert lib.gn_class_metrics_workspace_bytes(10 ** 9, 8) == 512 * 28 * 4


def test_class_metrics_unsupported_sizes_are_refused_by_the_library():
    lib = _hip.load()
    for c in (0, 1025):
        status = lib.gn_class_metrics_f32(None, 0, None, None, 0, c, None, None, None, None, None, None, 0, None)
        assert status == _hip.GN_ERR_UNSUPPORTED, (c, status)


def test_class_metrics_kernels_have_no_scratch():
    """Both kernels, every instantiation of the counting pass (1 / 8 / 64 lanes per row, scores with and without float4
    loads, given predictions) and the finalize: no scratch, no spills."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources(_hip.library_path())
    names = ["k_class_count<{}, false, {}>".format(w, v) for w in (1, 8, 64) for v in ("false", "true")]
    names += ["k_class_count<1, true, false>", "k_class_finalize"]
    for name in names:
        assert name in res, (name, sorted(k for k in res if "k_class" in k))
        r = res[name]
        assert r[".private_segment_fixed_size"] == 0, (name, r)
        assert r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (name, r)
