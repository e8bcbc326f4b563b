"""The cases of the gradient fixtures (tests/golden/*_grad.npz, decoder_saturated.npz; written by
``tests/golden/make_golden.py --grads`` from the reference's own ``loss.backward()``) and the comparisons the CPU and
the GPU gradient tests share.  Not a test module.

A fixture holds, per case: what the generator drew (``neg_index`` / ``labels`` / ``<tag>.proj``), ``loss32`` / ``loss64`` and
``grad32.<key>`` / ``grad64.<key>`` for every parameter (state-dict names) and for the layer's input (``x`` or ``z``); keys of a
layer fixture carry the case's tag in front (``cat.grad64.conv.weight``).  ``meta["no_grad"]`` lists what the reference
left without a gradient."""
import torch

from oracle import gripnet_oracle as orc

EPS = 1e-13                                                       # gripnet/utils.py:10

CALLERS = ["pose_tiny", "pose_small", "aminer_tiny", "freebase_a_tiny", "freebase_b_tiny", "freebase_c_tiny"]
LAYERS = [("gcn_forward", t) for t in ("wb", "nb")] \
    + [("inter_cases", t) for t in ("cat", "cat_w_norelu", "add_eq", "add_down", "noext")] \
    + [("rgcn_cases", t) for t in ("plain", "after_relu", "bias")] \
    + [("homo_cases", t) for t in ("gcn2_cat", "gcn2_nocat", "start1", "rgcn2")] \
    + [("decoder_cases", t) for t in ("dmt_sigmoid", "dmt_logits", "mcip_softmax", "mcip_logits")]
ROW_TABLES = ("embedding", "target_feat", "aa_embeddings", "x", "z")   # 2-D per-node tables: compared per row as well


def link_loss_expr(pos, neg):
    return -torch.log(pos + EPS).mean() - torch.log(1 - neg + EPS).mean()          # GripNet-pose.py:140-142


def class_loss_expr(score, labels):
    return -torch.log(score[torch.arange(labels.shape[0], device=labels.device), labels] + EPS).mean()   # GripNet-aminer.py:133


def layer_info(grad_fixture, tag):
    return next(v for v in grad_fixture.meta["cases"] if v["tag"] == tag)


def forward_variant(fixture, tag):
    return next(v for v in fixture.meta["variants"] if v["tag"] == tag)


def stored(grad_fixture, prefix, which):
    """{key: tensor} of one case's ``grad32`` / ``grad64`` entries."""
    full = prefix + which + "."
    return {k[len(full):]: torch.from_numpy(v) for k, v in grad_fixture.arrays.items() if k.startswith(full)}


def no_grad_keys(grad_fixture, prefix):
    """What the reference left without a gradient in one case (`prefix`: "" for a caller, "<tag>." for a layer)."""
    return [k[len(prefix):] for k in grad_fixture.meta.get("no_grad", []) if k.startswith(prefix)]


def is_row_table(key, grad):
    return grad.dim() == 2 and key.split(".")[-1] in ROW_TABLES


def check_gradients(got, want, rel, what, none_ok=(), row_rel=None, row_abs=None, bars=None):
    """Every gradient of `want` ({key: reference}) against `got` ({key: tensor or None}) at ``rel * max|want|`` (``bars``:
    another factor for single keys); an all-zero reference must be matched exactly; with `row_rel`, the per-node tables
    also row by row at ``row_rel * max|want[i]| + row_abs * max|want|``.  Keys in `none_ok` must be None or zero."""
    for k in none_ok:
        g = got.get(k)
        assert g is None or float(g.abs().max()) == 0.0, "{}: {} has a gradient the reference does not".format(what, k)
    assert want, what
    for k, ref in want.items():
        g = got.get(k)
        assert g is not None, "{}: no gradient for {}".format(what, k)
        g, ref = g.detach().cpu().double(), ref.double()
        assert g.shape == ref.shape, (what, k, g.shape, ref.shape)
        assert torch.isfinite(g).all(), "{}: {} is not finite".format(what, k)
        scale = float(ref.abs().max()) if ref.numel() else 0.0
        err = float((g - ref).abs().max()) if ref.numel() else 0.0
        bar = (bars or {}).get(k, rel)
        assert err <= bar * scale, "{}: {} off by {:.3e} = {:.2e} of its largest entry {:.3e} (bar {:.1e})".format(
            what, k, err, err / scale if scale else float("inf"), scale, bar)
        if row_rel is not None and is_row_table(k, ref):
            row_err = (g - ref).abs().amax(dim=1)
            allowed = row_rel * ref.abs().amax(dim=1) + row_abs * scale
            bad = (row_err > allowed).nonzero().view(-1)
            assert bad.numel() == 0, "{}: {} rows {} off by {} (allowed {})".format(
                what, k, bad[:5].tolist(), row_err[bad[:5]].tolist(), allowed[bad[:5]].tolist())


# ---- the oracle's differentiable form on a fixture's inputs ------------------------------------------------------------
def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


def oracle_case(golden, name, tag, dtype):
    """Loss and {key: leaf} of one case through oracle/gripnet_oracle.py under torch autograd in `dtype`, after
    ``backward()``: the gradients are the leaves' ``.grad``."""
    g = golden(name)
    gr = golden("decoder_saturated" if name == "decoder_saturated" else name + "_grad")

    def cast(key):
        t = g.t(key)
        return t.to(dtype) if t.is_floating_point() else t

    if name in CALLERS or name == "decoder_saturated":
        sd = {k[3:]: _leaf(g.t(k), dtype) for k in g.arrays if k.startswith("sd.")}
        leaves = dict(sd)
        if name.startswith("pose_"):
            out = orc.pose_forward(sd, g.t("gg_edge_index"), cast("edge_weight"), g.t("gd_edge_index"), g.t("train_idx"),
                                   g.t("train_et"), g.t("train_range"))
            neg = orc.distmult(out["z_dd"], gr.t("neg_index").long(), g.t("train_et"), sd["dmt.weight"])
            loss = link_loss_expr(out["score"], neg)
        elif name == "decoder_saturated":
            leaves["z"] = z = _leaf(g.t("z"), dtype)
            et = g.t("edge_type")
            loss = link_loss_expr(orc.distmult(z, g.t("pos_index"), et, sd["dmt.weight"]),
                                  orc.distmult(z, g.t("neg_index"), et, sd["dmt.weight"]))
        else:
            if name in ("aminer_tiny", "freebase_b_tiny"):
                out = orc.aminer_forward(sd, g.t("pp_edge_idx"), cast("pp_edge_weight"), g.t("pa_edge_idx"), g.t("aa_edge_idx"),
                                         cast("aa_edge_weight"), g.t("node_list"))
            elif name == "freebase_a_tiny":
                out = orc.freebase_a_forward(sd, g.t("aa_edge_idx"), cast("aa_edge_weight"), g.t("node_list"))
            else:
                leaves["aa_embeddings"] = aae = _leaf(g.t("aa_embeddings"), dtype)
                out = orc.freebase_c_forward(sd, g.t("pp_edge_idx"), cast("pp_edge_weight"), g.t("pa_edge_idx"),
                                             g.t("qq_edge_idx"), cast("qq_edge_weight"), g.t("qa_edge_idx"), aae,
                                             g.t("aa_edge_idx"), cast("aa_edge_weight"), g.t("node_list"), g.meta["n_a"])
            loss = class_loss_expr(out["score"], gr.t("labels"))
        loss.backward()
        return loss.detach(), leaves

    info = layer_info(gr, tag)
    full = "sd." + info["state"]
    own = [k for k in g.arrays if k.startswith(full)]
    if name == "gcn_forward" and tag == "wb":
        own = ["sd.weight", "sd.bias"]
    sd = {"m." + k[len(full):]: _leaf(g.t(k), dtype) for k in own}
    leaves = {k[2:]: v for k, v in sd.items()}
    if name == "gcn_forward":
        leaves["x"] = x = _leaf(g.t("x0"), dtype)
        y = orc.gcn_forward(x, sd["m.weight"], sd.get("m.bias"), g.t("edge_index"), cast("edge_weight") if info["weighted"] else None)
    elif name == "inter_cases":
        v = forward_variant(g, tag)
        leaves["x"] = x = _leaf(g.t("x"), dtype)
        y = orc.inter_forward(sd, "m.", x, g.t("edge_index"), cast("edge_weight") if v["weighted"] else None,
                              if_relu=v["if_relu"], mod=v["mod"], n_target=g.meta["n_target"])
    elif name == "rgcn_cases":
        leaves["x"] = x = _leaf(g.t("x"), dtype)
        y = orc.rgcn_forward(x, g.t("edge_index"), g.t("range_list"), sd["m.basis"], sd["m.att"], sd["m.root"], sd.get("m.bias"))
    elif name == "homo_cases":
        x = None
        if tag != "start1":
            leaves["x"] = x = _leaf(g.t("x"), dtype)
        if tag == "rgcn2":
            y = orc.homo_forward(sd, "m.", x, g.t("rel.edge_index"), range_list=g.t("rel.range_list"), if_catout=True)
        else:
            y = orc.homo_forward(sd, "m.", x, g.t("edge_index"), None if tag == "start1" else cast("edge_weight"),
                                 if_catout=info["if_catout"])
    else:
        leaves["z"] = z = _leaf(g.t("z"), dtype)
        if tag.startswith("dmt"):
            y = orc.distmult(z, g.t("edge_index"), g.t("edge_type"), sd["m.weight"], sigmoid=info["sigmoid"])
        else:
            y = orc.multiclass(z, g.t("node_list"), sd["m.weight"], softmax=info["softmax"])
    loss = (y * gr.t(tag + ".proj").to(dtype)).sum()
    loss.backward()
    return loss.detach(), leaves
