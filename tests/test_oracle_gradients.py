"""The oracle's differentiable form against the reference's own ``loss.backward()`` (the gradient fixtures of
tests/golden/make_golden.py --grads).  tests/test_gpu_backward.py holds the HIP gradients to torch autograd THROUGH
oracle/gripnet_oracle.py; this is what holds that to the reference: a slip in the oracle's op order, in a detached
tensor or in where EPS enters the loss shows here, without a GPU.

float64 against ``grad64``: 1e-9 of the gradient's largest entry (two float64 evaluations of one formula).  fp32 against
``grad32``: 1e-5 of it, the generator's own bound on the distance of the reference's fp32 run from float64; pose_small
stores no ``grad32`` (file size), there the oracle's fp32 run is held to ``grad64`` at the bound the generator proved for the
reference's fp32 run (``meta["fp32_distance"]`` where it is not 1e-5)."""
import pytest
import torch

import grad_cases as gc

CASES = [(name, "") for name in gc.CALLERS] + gc.LAYERS


@pytest.mark.parametrize("name,tag", CASES, ids=["-".join(filter(None, c)) for c in CASES])
def test_oracle_autograd_matches_the_reference(golden, name, tag):
    gr = golden(name + "_grad")
    prefix = tag + "." if tag else ""
    g64, g32 = gc.stored(gr, prefix, "grad64"), gc.stored(gr, prefix, "grad32")
    none_ok = gc.no_grad_keys(gr, prefix)
    loss, leaves = gc.oracle_case(golden, name, tag, torch.float64)
    want = float(gr.t(prefix + "loss64"))
    assert abs(float(loss) - want) <= 1e-9 * abs(want), (float(loss), want)
    assert set(g64) | set(none_ok) == set(leaves), (sorted(g64), sorted(leaves))
    gc.check_gradients({k: v.grad for k, v in leaves.items()}, g64, 1e-9, name + " " + tag + " float64", none_ok=none_ok)
    loss, leaves = gc.oracle_case(golden, name, tag, torch.float32)
    assert loss.dtype == torch.float32
    assert abs(float(loss) - float(gr.t(prefix + "loss32"))) <= 1e-6 * abs(want)
    got = {k: v.grad for k, v in leaves.items()}
    if g32:
        assert set(g32) == set(g64)
        scaled = {k: 1e-5 * float(g64[k].abs().max()) / max(float(g32[k].abs().max()), 1e-300) for k in g32}
        gc.check_gradients(got, g32, 1e-5, name + " " + tag + " fp32", none_ok=none_ok, bars=scaled)
    else:
        gc.check_gradients(got, g64, 1e-5, name + " " + tag + " fp32 (no grad32 stored)", none_ok=none_ok,
                           bars=gr.meta.get("fp32_distance"))


def test_oracle_on_saturated_scores(golden):
    """decoder_saturated: where fp32 and float64 part ways (fp32 sigmoid is 1.0 from 16.64 upward: such a negative costs
    -log(EPS) = 29.93 and carries no gradient) the oracle follows the reference in each precision."""
    gr = golden("decoder_saturated")
    for dtype, which, rel in ((torch.float64, "64", 1e-9), (torch.float32, "32", 1e-5)):
        loss, leaves = gc.oracle_case(golden, "decoder_saturated", "", dtype)
        want = float(gr.t("loss" + which))
        assert abs(float(loss) - want) <= (1e-9 if which == "64" else 1e-6) * abs(want)
        gc.check_gradients({k: v.grad for k, v in leaves.items()}, gc.stored(gr, "", "grad" + which), rel, "saturated " + which)
    hot = gr.meta["bands"]["hot"]
    assert float(leaves["dmt.weight"].grad[hot].abs().max()) == 0.0
    assert float(leaves["z"].grad[gr.meta["hot_only_nodes"]].abs().max()) == 0.0
    assert abs(float(gr.t("loss32")) - float(gr.t("loss64"))) > 1e-3          # the case does separate the two precisions


def test_gradient_fixtures_hold_what_the_gpu_tests_lean_on(golden):
    """The facts the GPU gradient tests lean on: every stored gradient is finite and not identically zero, the
    saturated bands are where ``meta`` says, and the small gradients that absolute bars let through are small."""
    for name, tag in CASES:
        gr = golden(name + "_grad")
        g64 = gc.stored(gr, tag + "." if tag else "", "grad64")
        assert g64, (name, tag)
        for k, v in g64.items():
            assert v.dtype == torch.float64 and torch.isfinite(v).all() and float(v.abs().max()) > 0, (name, tag, k)
    small = gc.stored(golden("pose_small_grad"), "", "grad64")
    assert float(small["gg.embedding"].abs().max()) < 1e-3 and float(small["gd.target_feat"].abs().max()) < 1e-2
    gr = golden("decoder_saturated")
    et, bands = gr.t("edge_type"), gr.meta["bands"]
    for side in ("pos", "neg"):
        lg, s = gr.t(side + "_logit64"), gr.t(side + "_score")
        sel = {b: torch.isin(et, torch.tensor(r)) for b, r in bands.items()}
        assert (lg[sel["ordinary"]].abs() <= 4).all() and (lg[sel["hot"]] >= 20).all()
        assert (lg[sel["cold"]] <= -20).all() and (lg[sel["frozen"]] <= -110).all()
        assert (s[sel["hot"]] == 1).all() and (s[sel["frozen"]] == 0).all()
    assert float(gr.t("neg_score.grad")[torch.isin(et, torch.tensor(bands["hot"]))].min()) > 1e10
