"""Node-classification metrics on the device (gn_class_metrics_f32) against torch.argmax on the GPU tensor, numpy and
scikit-learn (the reference's micro_macro / acc, gripnet/utils.py:38-52): counts exactly, per-class ratios, micro-F1 and
accuracy bit for bit, macro-F1 to 1e-15 relative."""
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from gripnet_amd import _hip, utils
from gripnet_amd.decoder import multiClassInnerProductDecoder

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sk_reference(y, p, C):
    """What scikit-learn 1.7.2 says for true ids y and predicted ids p (numpy int64)."""
    from sklearn.metrics import accuracy_score, f1_score, precision_recall_fscore_support
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prec, rec, f1, _ = precision_recall_fscore_support(y, p, labels=list(range(C)), zero_division=0)
        return {"precision": prec, "recall": rec, "f1": f1, "micro_f1": f1_score(y, p, average="micro"),
                "macro_f1": f1_score(y, p, average="macro"), "accuracy": accuracy_score(y, p)}


def assert_matches_reference(got, y, p, C):
    np.testing.assert_array_equal(got["support"].cpu().numpy(), np.bincount(y, minlength=C))
    np.testing.assert_array_equal(got["predicted"].cpu().numpy(), np.bincount(p, minlength=C))
    np.testing.assert_array_equal(got["correct"].cpu().numpy(), np.bincount(y[y == p], minlength=C))
    want = sk_reference(y, p, C)
    for k in ("precision", "recall", "f1"):
        g = got[k].cpu().numpy()
        assert g.dtype == np.float64
        assert np.array_equal(g, want[k]), (k, C, len(y))                          # bit for bit
    for k in ("micro_f1", "accuracy"):
        g = got[k].item()
        assert (g == want[k]) or (math.isnan(g) and math.isnan(want[k])), (k, g, want[k])
    g, w = got["macro_f1"].item(), float(want["macro_f1"])
    if math.isnan(w):
        assert math.isnan(g)
    else:
        assert abs(g - w) <= 1e-15 * abs(w), (g, w)


def grid():
    for C in (1, 2, 3, 8, 17, 64, 65, 100, 1024):
        for n in (0, 1, 63, 64, 65, 10_000, 1_000_003):
            if n * C <= 20_000_000:
                yield C, n


@pytest.mark.parametrize("C, n", list(grid()))
def test_parity_with_sklearn_and_numpy(gpu, C, n):
    g = torch.Generator(device=gpu).manual_seed(1000 * C + n % 997)
    score = torch.randn((n, C), generator=g, device=gpu)
    # the labels use the lower half of the classes only: the upper half occurs in the predictions alone, and with few rows
    # many classes occur in neither
    y = torch.randint(0, max(1, (C + 1) // 2), (n,), generator=g, device=gpu)
    if n > 10 and C > 2:
        score[: n // 3, 0] += 3.0                              # a third of the rows predict class 0: some rows are right
    got = utils.class_metrics(score, y)
    want_pred = torch.argmax(score, 1)
    assert got["pred"].dtype == torch.int64 and torch.equal(got["pred"], want_pred)
    assert_matches_reference(got, y.cpu().numpy(), want_pred.cpu().numpy(), C)
    for k in ("micro_f1", "macro_f1", "accuracy"):
        assert got[k].dim() == 0 and got[k].dtype == torch.float64 and got[k].device == score.device


def test_empty_list_gives_sklearns_values(gpu):
    got = utils.class_metrics(torch.empty((0, 5), device=gpu), torch.empty((0,), dtype=torch.long, device=gpu))
    assert got["micro_f1"].item() == 0.0
    assert math.isnan(got["macro_f1"].item()) and math.isnan(got["accuracy"].item())
    assert got["pred"].numel() == 0 and int(got["support"].sum()) == 0
    assert not got["f1"].any()
    got = utils.class_metrics(torch.empty((0,), dtype=torch.long, device=gpu), torch.empty((0,), dtype=torch.long, device=gpu), 3)
    assert got["pred"] is None and got["micro_f1"].item() == 0.0 and math.isnan(got["accuracy"].item())


def crafted_scores(n, C, seed, dev):
    """Small integers (ties everywhere, -0.0 next to +0.0), NaN in some rows and columns, all-NaN rows, +-inf, all -inf rows."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-2, 3, (n, C), generator=g).float()
    s[torch.rand((n, C), generator=g) < 0.2] = -0.0
    r = torch.arange(n)
    nan_rows = r[(r % 7) == 1]
    s[nan_rows, torch.randint(0, C, (len(nan_rows),), generator=g)] = float("nan")
    two = r[(r % 11) == 2]
    s[two, torch.randint(0, C, (len(two),), generator=g)] = float("nan")        # rows with two NaNs (or one twice)
    s[two, (C - 1)] = float("nan")
    s[r[(r % 13) == 3]] = float("nan")                                         # all NaN
    s[r[(r % 17) == 4]] = float("-inf")                                        # all -inf
    inf_rows = r[(r % 5) == 0]
    s[inf_rows, torch.randint(0, C, (len(inf_rows),), generator=g)] = float("inf")
    s[inf_rows[::2], (C - 1) // 2] = float("inf")                              # tied +inf
    s[r[(r % 19) == 6], :] = -0.0
    s[r[(r % 19) == 6], C - 1] = 0.0                                           # +0.0 after -0.0: ties with the first column
    ninf = r[(r % 23) == 7]
    s[ninf] = float("-inf")
    s[ninf, C - 1] = float("nan")                                              # -inf everywhere but a last-column NaN
    return s.to(dev)


@pytest.mark.parametrize("C", [1, 2, 3, 5, 8, 9, 17, 64, 100, 129, 1024])
def test_pred_equals_torch_argmax_on_crafted_rows(gpu, C):
    s = crafted_scores(700, C, C, gpu)
    got, _, _, _ = _hip.class_metrics(s, torch.zeros(700, dtype=torch.long, device=gpu))
    assert torch.equal(got, torch.argmax(s, 1))
    assert torch.equal(got.cpu(), torch.argmax(s.cpu(), 1))                     # (and CPU torch agrees on these rows)


def test_pred_equals_torch_argmax_on_the_class_decoders_softmax(gpu):
    torch.manual_seed(5)
    dec = multiClassInnerProductDecoder(16, 12).to(gpu)
    with torch.no_grad():
        dec.weight[:, 5] = dec.weight[:, 2]                                    # equal logits: equal probabilities
        dec.weight[:, 9] = dec.weight[:, 2]
        dec.weight[:, 7] = dec.weight[:, 1]
        dec.weight.mul_(40.0)                                                  # saturated rows: many exact 0.0 and 1.0
    z = torch.randn(3000, 16, device=gpu)
    nodes = torch.arange(3000, device=gpu)
    with torch.no_grad():
        prob = dec(z, nodes)
    assert (prob == 1.0).any() and (prob[:, 2] == prob[:, 5]).all()
    ties = (prob == prob.max(1, keepdim=True).values).sum(1) > 1
    assert ties.sum() > 100, int(ties.sum())
    y = torch.randint(0, 12, (3000,), device=gpu)
    got = utils.class_metrics(prob, y)
    assert torch.equal(got["pred"], torch.argmax(prob, 1))
    assert_matches_reference(got, y.cpu().numpy(), torch.argmax(prob, 1).cpu().numpy(), 12)


@pytest.mark.parametrize("C", [1, 3, 8, 17, 100, 300])
def test_strided_view_equals_its_contiguous_copy(gpu, C):
    g = torch.Generator(device=gpu).manual_seed(C)
    wide = torch.randn((5000, C + 7), generator=g, device=gpu)
    wide[::3, 3] = wide[::3, 4]                                                # ties inside the view
    view = wide[:, 3:3 + C]                                                    # odd offset, ld = C + 7
    assert view.stride(0) == C + 7 and view.data_ptr() % 16 != 0
    y = torch.randint(0, C, (5000,), generator=g, device=gpu)
    a, b = utils.class_metrics(view, y), utils.class_metrics(view.contiguous(), y)
    for k in a:
        assert torch.equal(a[k], b[k]) or (a[k].is_floating_point() and torch.equal(a[k].isnan(), b[k].isnan())
                                           and torch.equal(a[k].nan_to_num(), b[k].nan_to_num())), k
    assert torch.equal(a["pred"], torch.argmax(view, 1))


@pytest.mark.parametrize("C", [1, 4, 8, 33, 1024])
def test_pred_mode_equals_score_mode(gpu, C):
    g = torch.Generator(device=gpu).manual_seed(7 + C)
    score = torch.randn((20_000, C), generator=g, device=gpu)
    y = torch.randint(0, C, (20_000,), generator=g, device=gpu)
    a = utils.class_metrics(score, y)
    b = utils.class_metrics(torch.argmax(score, 1), y, C)
    assert b["pred"] is None
    for k in a:
        if k != "pred":
            assert torch.equal(a[k], b[k]) or (torch.isnan(a[k]).all() and torch.isnan(b[k]).all()), k


@pytest.mark.parametrize("bad", [-1, "C"])
def test_out_of_range_class_ids(gpu, bad):
    C, n = 6, 1000
    g = torch.Generator(device=gpu).manual_seed(3)
    score = torch.randn((n, C), generator=g, device=gpu)
    y = torch.randint(0, C, (n,), generator=g, device=gpu)
    y[[5, 700]] = C if bad == "C" else bad
    _hip.raise_if_index_errors(gpu)
    with pytest.raises(IndexError, match="class id"):
        utils.class_metrics(score, y)
    # through the asynchronous launch: NaN outputs now, the IndexError at the next check, then a clear flag
    pred, counts, per_class, summary = _hip.class_metrics(score, y)
    assert torch.isnan(per_class).all() and torch.isnan(summary).all()
    ok = ((y >= 0) & (y < C)).cpu().numpy()
    yy, pp = y.cpu().numpy()[ok], pred.cpu().numpy()[ok]
    np.testing.assert_array_equal(counts[0].cpu().numpy(), np.bincount(yy, minlength=C))
    np.testing.assert_array_equal(counts[1].cpu().numpy(), np.bincount(pp, minlength=C))
    np.testing.assert_array_equal(counts[2].cpu().numpy(), np.bincount(yy[yy == pp], minlength=C))
    assert torch.equal(pred, torch.argmax(score, 1))
    with pytest.raises(IndexError, match="class id"):
        _hip.raise_if_index_errors(gpu)
    assert int(_hip.error_flag(gpu).item()) == 0
    y[[5, 700]] = 0
    got = utils.class_metrics(score, y)
    assert_matches_reference(got, y.cpu().numpy(), torch.argmax(score, 1).cpu().numpy(), C)


def test_out_of_range_predicted_ids(gpu):
    y = torch.zeros(300, dtype=torch.long, device=gpu)
    p = torch.zeros(300, dtype=torch.long, device=gpu)
    p[17] = 4
    with pytest.raises(IndexError, match="class id"):
        utils.class_metrics(p, y, 4)
    p[17] = 3
    assert utils.class_metrics(p, y, 4)["accuracy"].item() == 299 / 300


def test_two_calls_give_the_same_bits(gpu):
    g = torch.Generator(device=gpu).manual_seed(11)
    for C in (8, 100):
        score = torch.randn((300_001, C), generator=g, device=gpu)
        y = torch.randint(0, C, (300_001,), generator=g, device=gpu)
        a, b = _hip.class_metrics(score, y), _hip.class_metrics(score, y)
        for x, z in zip(a, b):
            assert torch.equal(x, z)


def test_graph_capture_replays_on_new_contents(gpu):
    C, n = 8, 10_000
    g = torch.Generator(device=gpu).manual_seed(21)
    score = torch.randn((n, C), generator=g, device=gpu)
    y = torch.randint(0, C, (n,), generator=g, device=gpu)
    _hip.class_metrics(score, y)                                               # error word and library loaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            outs = _hip.class_metrics(score, y)
    torch.cuda.current_stream().wait_stream(s)
    for seed in (1, 2):
        score.copy_(torch.randn((n, C), generator=g, device=gpu))
        y.copy_(torch.randint(0, C, (n,), generator=g, device=gpu))
        graph.replay()
        eager = _hip.class_metrics(score, y)
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)
        assert_matches_reference({"support": outs[1][0], "predicted": outs[1][1], "correct": outs[1][2], "precision": outs[2][0],
                                  "recall": outs[2][1], "f1": outs[2][2], "micro_f1": outs[3][0], "macro_f1": outs[3][1],
                                  "accuracy": outs[3][2]}, y.cpu().numpy(), torch.argmax(score, 1).cpu().numpy(), C)
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("which", ["aminer", "freebase-c"])
def test_full_size_models_match_micro_macro_and_acc(gpu, which):
    from gripnet_amd.pipeline import AminerModel, FreebaseCModel
    from gripnet_amd.synth import make_nc
    data = make_nc("aminer-syn").to(gpu)
    torch.manual_seed(1111)
    model = (AminerModel(data.n_p_node, data.n_a_node, data.n_a_type) if which == "aminer" else
             FreebaseCModel(data.n_p_node, data.n_q_node, data.n_a_node, data.n_a_type)).to(gpu)
    test_nodes = torch.arange(1, data.n_a_node, 2, device=gpu)
    test_class = data.a_label[test_nodes].contiguous()
    with torch.no_grad():
        _, score = model(data, test_nodes)
    got = utils.class_metrics(score, test_class)
    pred = torch.argmax(score, dim=1)
    assert torch.equal(got["pred"], pred)
    micro, macro = utils.micro_macro(test_class, pred)
    assert got["micro_f1"].item() == micro
    assert abs(got["macro_f1"].item() - macro) <= 1e-15 * abs(macro)
    assert got["accuracy"].item() == utils.acc(test_class, pred)


def test_example_runs(gpu):
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train_nc.py"), "--workload", "tiny", "--epochs", "2"],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "micro" in ln]
    assert len(lines) == 2, r.stdout
    for ln in lines:
        nums = [float(w.split(":")[1]) for w in ln.split() if w.startswith(("train_micro:", "train_macro:", "test_micro:", "test_macro:"))]
        assert len(nums) == 4 and all(math.isfinite(x) for x in nums), ln
