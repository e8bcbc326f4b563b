"""Gradients of the HIP path against the reference's own ``loss.backward()``: the fixtures that
``tests/golden/make_golden.py --grads`` wrote from the reference's modules in fp32 and in float64 (reads only tests/golden/).

Every gradient is held to ``grad64`` at 1e-4 of ITS OWN largest entry (the project's 1e-4 contract at the gradient's scale: the
largest entry of ``gg.embedding.grad`` on pose_small is 1.4e-4, so an absolute 1e-4 lets half of every entry go missing), the
loss at 1e-5 relative.  The generator proved the reference's fp32 run to sit at a tenth of that bar (one exception, recorded
in the fixture: ``dmt.weight`` of pose_small, 1.9e-5).  Per-node tables (``*.embedding``, ``target_feat``, ``aa_embeddings``, the
layer inputs' ``dx`` / ``dz``) are also compared row by row, ``1e-4 * max|row| + 1e-5 * max|tensor|``: a dropped, doubled or
misrouted edge moves its row by the row's own size and hides at the tensor's scale when the row is small.  Tables whose
rows are sums over very many triples (``dmt.weight``) get the tensor-scale check only.

Every case runs twice (the second call takes the plans the first one left) and under each setting of the library's
kernel-selection hooks.  The relational layers' ``kernel`` attribute is not read by the training path, so the hooks are
what selects a path there.

decoder_saturated: DistMult + link loss where fp32 and float64 part ways.  An fp32 sigmoid is exactly 1.0 from a logit of
16.64 upward; such a negative costs -log(EPS) = 29.93 and, its s (1 - s) being zero, carries no gradient.  The contract is
the reference's fp32 behaviour, so this case is held to ``loss32`` / ``grad32``."""
import pytest
import torch

import grad_cases as gc
import gripnet_amd
from gripnet_amd import _hip
from gripnet_amd.pipeline import AminerModel, FreebaseAModel, FreebaseBModel, FreebaseCModel, PoseModel
from gripnet_amd.synth import Data
from gripnet_amd.utils import class_loss, link_loss, link_prediction_loss

pytestmark = pytest.mark.gpu

LOSS_REL, GRAD_REL, ROW_REL, ROW_ABS = 1e-5, 1e-4, 1e-4, 1e-5


@pytest.fixture(params=["default", "no-quad", "general"])
def hooks(request, monkeypatch):
    """The environment hooks of tests/test_gpu_parity.py's `kernel_path`: every fast path on; the shuffle form of the
    16-wide gathers and the LDS-resident relational kernel instead of the destination-major one; every fast path off."""
    monkeypatch.setenv("GN_DISABLE_FAST", "1" if request.param == "general" else "0")
    monkeypatch.setenv("GN_DISABLE_QUAD", "0" if request.param == "default" else "1")
    return request.param


def load_into(module, state, dev):
    module.load_state_dict(state)
    return module.to(dev)


def leaf(t, dev):
    return t.to(dev).detach().clone().requires_grad_(True)


def check_case(gr, prefix, loss, grads, what, dev):
    want = float(gr.t(prefix + "loss64"))
    err = abs(float(loss) - want)
    print("{}: loss {:.8g} vs {:.8g} ({:.2e} relative)".format(what, float(loss), want, err / abs(want)))
    for k, ref in gc.stored(gr, prefix, "grad64").items():
        if grads.get(k) is not None:
            print("   {}: {:.2e} of its largest entry {:.3e}".format(
                k, float((grads[k].detach().cpu().double() - ref).abs().max()) / float(ref.abs().max()), float(ref.abs().max())))
    assert err <= LOSS_REL * abs(want), (what, float(loss), want)
    gc.check_gradients(grads, gc.stored(gr, prefix, "grad64"), GRAD_REL, what, none_ok=gc.no_grad_keys(gr, prefix),
                       row_rel=ROW_REL, row_abs=ROW_ABS)
    _hip.raise_if_index_errors(dev)


# ---- callers -----------------------------------------------------------------------------------------------------------
def pose_setup(golden, scale, dev):
    g, gr = golden("pose_" + scale), golden("pose_{}_grad".format(scale))
    model = load_into(PoseModel(g.meta["n_g"], g.meta["n_d"], g.meta["R"]), g.state("", strip=False), dev)
    data = Data(**{k: g.t(k, dev) for k in ("gg_edge_index", "edge_weight", "gd_edge_index", "train_idx", "train_et", "train_range")})
    return gr, model, data, gr.t("neg_index").long().to(dev).contiguous()


def link_loss_three_ways(way, dmt, z, pos_index, neg_index, et):
    if way == "spelled":                                                   # GripNet-pose.py:137-142
        return gc.link_loss_expr(dmt(z, pos_index, et), dmt(z, neg_index, et))
    if way == "link_loss":
        return link_loss(dmt(z, pos_index, et), dmt(z, neg_index, et))
    return link_prediction_loss(dmt, z, pos_index, neg_index, et)[0]


@pytest.mark.parametrize("way", ["spelled", "link_loss", "fused"])
@pytest.mark.parametrize("scale", ["tiny", "small"])
def test_pose_training_step_against_the_reference(gpu, golden, hooks, scale, way):
    """GripNet-pose.py:117-144 with the fixture's negative list: the loss spelled out over two decoder calls, through
    utils.link_loss, and through utils.link_prediction_loss (fused) with the list as a plain int64 tensor.  (The packed
    32-bit pairs that the fused backward reads for sampled negatives exist only behind NegativeSampler.sample's own draws:
    its public surface does not pack a given list, so that launch is not reachable with a fixed list.)"""
    gr, model, data, neg = pose_setup(golden, scale, gpu)
    for call in range(2):
        model.zero_grad()
        z = model.encode(data)
        loss = link_loss_three_ways(way, model.dmt, z, data.train_idx, neg, data.train_et)
        loss.backward()
        check_case(gr, "", loss, {k: p.grad for k, p in model.named_parameters()},
                   "pose_{} {} {} call {}".format(scale, way, hooks, call), gpu)


def nc_model(g, name):
    m = g.meta
    if name == "freebase_a_tiny":
        return FreebaseAModel(m["n_a"], m["n_class"], pp_nhids=m["pp_nhids"])
    if name == "freebase_c_tiny":
        return FreebaseCModel(m["n_p"], m["n_q"], m["n_a"], m["n_class"], pp_nhids=m["pp_nhids"], qq_nhids=m["qq_nhids"],
                              pa_out=m["pa_out"], aa_hidden=m["aa_nhids"][1:])
    cls = AminerModel if name == "aminer_tiny" else FreebaseBModel
    return cls(m["n_p"], m["n_a"], m["n_class"], pp_nhids=m["pp_nhids"], pa_out=m["pa_out"], aa_hidden=m["aa_nhids"][1:])


@pytest.mark.parametrize("way", ["spelled", "class_loss"])
@pytest.mark.parametrize("name", ["aminer_tiny", "freebase_a_tiny", "freebase_b_tiny", "freebase_c_tiny"])
def test_node_classification_step_against_the_reference(gpu, golden, hooks, name, way):
    """The drivers' ``-log(score[range(n), cls] + EPS).mean()`` (GripNet-aminer.py:133) with the fixture's labels, spelled
    out with torch indexing and through utils.class_loss."""
    g, gr = golden(name), golden(name + "_grad")
    sd = g.state("", strip=False)
    if name == "freebase_c_tiny":
        sd["aa_embeddings"] = g.t("aa_embeddings")
    model = load_into(nc_model(g, name), sd, gpu)
    keys = [k for k in ("pp_edge_idx", "pa_edge_idx", "qq_edge_idx", "qa_edge_idx", "aa_edge_idx", "pp_edge_weight",
                        "qq_edge_weight", "aa_edge_weight") if g.has(k)]
    data = Data(**{k: g.t(k, gpu) for k in keys})
    nodes, labels = g.t("node_list", gpu), gr.t("labels", gpu)
    for call in range(2):
        model.zero_grad()
        _, score = model(data, nodes)
        loss = gc.class_loss_expr(score, labels) if way == "spelled" else class_loss(score, labels)
        loss.backward()
        check_case(gr, "", loss, {k: p.grad for k, p in model.named_parameters()}, "{} {} {} call {}".format(name, way, hooks, call), gpu)


# ---- layers: loss = (y * P).sum() with the stored P ----------------------------------------------------------------------
def hip_layer(golden, name, tag, dev):
    """(module, forward(x) -> y, input leaf or None) of one layer case on the HIP kernels."""
    g, gr = golden(name), golden(name + "_grad")
    info = gc.layer_info(gr, tag)
    if name == "gcn_forward":
        state = {"weight": g.t("sd.weight"), "bias": g.t("sd.bias")} if tag == "wb" else g.state("nb.")
        m = load_into(gripnet_amd.myGCN(g.meta["fin"], info["fout"], cached=info["bias"], bias=info["bias"]), state, dev)
        ei, w = g.t("edge_index", dev), g.t("edge_weight", dev) if info["weighted"] else None
        return m, (lambda x: m(x, ei, w)), leaf(g.t("x0"), dev)
    if name == "inter_cases":
        v = gc.forward_variant(g, tag)
        m = gripnet_amd.interGraph(g.meta["source_dim"], v["target_dim"], g.meta["n_target"], target_feat_dim=v["target_feat_dim"],
                                   if_one_external=v["if_one_external"])
        m = load_into(m, g.state(tag + "."), dev)
        ei, w = g.t("edge_index", dev), g.t("edge_weight", dev) if v["weighted"] else None
        return m, (lambda x: m(x, ei, w, if_relu=v["if_relu"], mod=v["mod"])), leaf(g.t("x"), dev)
    if name == "rgcn_cases":
        v = gc.forward_variant(g, tag)
        m = load_into(gripnet_amd.myRGCN(g.meta["fin"], g.meta["fout"], g.meta["R"], g.meta["B"], v["after_relu"], bias=v["bias"]),
                      g.state(tag + "."), dev)
        ei, et, rl = g.t("edge_index", dev), g.t("edge_type", dev), g.t("range_list", dev)
        return m, (lambda x: m(x, ei, et, rl)), leaf(g.t("x"), dev)
    if name == "homo_cases":
        if tag == "start1":
            m = load_into(gripnet_amd.homoGraph([10, 16], start_graph=True, in_dim=g.meta["n"]), g.state("start1."), dev)
            ei = g.t("edge_index", dev)
            return m, (lambda x: m(None, ei, None, if_catout=True)), None
        if tag == "rgcn2":
            m = load_into(gripnet_amd.homoGraph([12, 8, 6], multi_relational=True, n_rela=3, n_base=5), g.state("rgcn2."), dev)
            ei, et, rl = g.t("rel.edge_index", dev), g.t("rel.edge_type", dev), g.t("rel.range_list", dev)
            return m, (lambda x: m(x, ei, edge_type=et, range_list=rl, if_catout=True)), leaf(g.t("x"), dev)
        m = load_into(gripnet_amd.homoGraph([12, 8, 8]), g.state("gcn2."), dev)
        ei, w = g.t("edge_index", dev), g.t("edge_weight", dev)
        return m, (lambda x: m(x, ei, w, if_catout=info["if_catout"])), leaf(g.t("x"), dev)
    if tag.startswith("dmt"):
        m = load_into(gripnet_amd.multiRelaInnerProductDecoder(g.meta["F"], g.meta["R"]), g.state("dmt."), dev)
        ei, et = g.t("edge_index", dev), g.t("edge_type", dev)
        return m, (lambda z: m(z, ei, et, sigmoid=info["sigmoid"])), leaf(g.t("z"), dev)
    m = load_into(gripnet_amd.multiClassInnerProductDecoder(g.meta["F"], g.meta["n_class"]), g.state("mcip."), dev)
    nodes = g.t("node_list", dev)
    return m, (lambda z: m(z, nodes, softmax=info["softmax"])), leaf(g.t("z"), dev)


@pytest.mark.parametrize("name,tag", gc.LAYERS, ids=["-".join(c) for c in gc.LAYERS])
def test_layer_gradients_against_the_reference(gpu, golden, hooks, name, tag):
    """Every variant the forward fixtures hold: weighted / unweighted, with and without bias and ReLU, the external layer's
    five merges (`add_down` is the only place target_feat_down gets a gradient), duplicate edges, empty relations,
    zero in-degree nodes, stacks with and without concat, a repeated triple and a u == v triple in the decoder's list."""
    gr = golden(name + "_grad")
    m, forward, x = hip_layer(golden, name, tag, gpu)
    proj = gr.t(tag + ".proj", gpu)
    for call in range(2):
        m.zero_grad()
        if x is not None:
            x.grad = None
        loss = (forward(x) * proj).sum()
        loss.backward()
        grads = {k: p.grad for k, p in m.named_parameters()}
        if x is not None:
            grads["z" if name == "decoder_cases" else "x"] = x.grad
        check_case(gr, tag + ".", loss, grads, "{} {} {} call {}".format(name, tag, hooks, call), gpu)


# ---- saturated scores ------------------------------------------------------------------------------------------------------
def test_link_loss_kernels_on_the_reference_scores(gpu, golden):
    """utils.link_loss on the reference's own fp32 scores (both sides start from the same bits): the value against the
    expression in float64 over those scores - which is the stored loss32 -, both gradients per element against the
    stored ``.grad``, the 1e13-sized entries at q == 1.0 included."""
    gr = golden("decoder_saturated")
    hot = torch.isin(gr.t("edge_type"), torch.tensor(gr.meta["bands"]["hot"]))
    assert (gr.t("neg_score")[hot] == 1).all()
    p, q = leaf(gr.t("pos_score"), gpu), leaf(gr.t("neg_score"), gpu)
    ref = float(gc.link_loss_expr(gr.t("pos_score").double(), gr.t("neg_score").double()))
    assert abs(ref - float(gr.t("loss32"))) <= 2e-6 * abs(ref), (ref, float(gr.t("loss32")))
    loss = link_loss(p, q)
    loss.backward()
    print("loss {:.8g} vs {:.8g}".format(float(loss), ref))
    assert abs(float(loss) - ref) <= 2e-6 * abs(ref), (float(loss), ref)
    for name, got, want in (("dpos", p.grad.cpu(), gr.t("pos_score.grad")), ("dneg", q.grad.cpu(), gr.t("neg_score.grad"))):
        assert torch.isfinite(got).all(), name
        rel = ((got.double() - want.double()).abs() / want.double().abs().clamp(min=1e-300))
        print("{}: worst {:.2e} relative, largest entry {:.3e}".format(name, float(rel.max()), float(want.abs().max())))
        assert ((got.double() - want.double()).abs() <= 2e-6 * want.double().abs()).all(), (name, float(rel.max()))
    assert float(q.grad[hot.to(gpu)].min()) > 1e10


def decoder_forward_paths(dm, z, ei, et, monkeypatch):
    """{path: scores}: the plan-less kernels (first sighting of the list), the planned one (from the second sighting),
    the general kernel (every fast path off) and the general kernel at an odd width (a zero column added to z and D:
    the same logits)."""
    out = {}
    with torch.no_grad():
        dm.forget_static()
        out["plan-less"] = dm(z, ei, et).clone()
        dm(z, ei, et)
        out["planned"] = dm(z, ei, et).clone()
        assert dm._find(ei, et).plan, "the third call did not take a plan"
        monkeypatch.setenv("GN_DISABLE_FAST", "1")
        dm.forget_static()
        out["general"] = dm(z, ei, et).clone()
        monkeypatch.setenv("GN_DISABLE_FAST", "0")
        odd = gripnet_amd.multiRelaInnerProductDecoder(dm.in_dim + 1, dm.num_et).to(z.device)
        odd.weight.data.zero_()
        odd.weight.data[:, :dm.in_dim] = dm.weight.data
        z_odd = torch.zeros(z.shape[0], dm.in_dim + 1, device=z.device)
        z_odd[:, :dm.in_dim] = z
        out["odd width"] = odd(z_odd, ei, et).clone()
        out["odd width, planned"] = [odd(z_odd, ei, et) for _ in range(2)][-1].clone()
    return out


def check_saturated_scores(s, logit64, what):
    """Range; exactly 1.0 from a logit of 20 upward; <= 1e-8 from -20 downward and < 1e-37 from -110 downward; within 2e-5
    of the float64 sigmoid up to |logit| = 20 (the suite's bar on a score); between -80 and -20 within 2e-5 RELATIVE
    (there the score enters log(pos + EPS) relatively).  Returns the number of decreasing steps in the logit's order."""
    s = s.detach().cpu()
    x = logit64.double()
    s64 = torch.sigmoid(x)
    assert torch.isfinite(s).all() and (s >= 0).all() and (s <= 1).all(), what
    assert (s[x >= 20] == 1).all(), (what, "not 1.0 on the hot band")
    assert (s[x <= -20] <= 1e-8).all() and (s[x <= -110] < 1e-37).all(), what
    mid = x.abs() <= 20
    err = float((s.double() - s64)[mid].abs().max())
    cold = (x <= -20) & (x > -80)
    rel = float(((s.double() - s64).abs() / s64)[cold].max()) if cold.any() else 0.0
    order = torch.argsort(x, stable=True)
    drops = int((s[order][1:] < s[order][:-1]).sum())
    print("{}: |s - s64| {:.2e} up to |logit| 20, {:.2e} relative on (-80, -20], {} decreasing steps".format(what, err, rel, drops))
    assert err <= 2e-5 and rel <= 2e-5, (what, err, rel)
    return drops


def test_decoder_forward_on_saturated_logits(gpu, golden, monkeypatch):
    gr = golden("decoder_saturated")
    dm = load_into(gripnet_amd.multiRelaInnerProductDecoder(gr.meta["F"], gr.meta["R"]), gr.state("dmt."), gpu)
    z, et = gr.t("z", gpu), gr.t("edge_type", gpu)
    for side in ("pos", "neg"):
        ei = gr.t(side + "_index", gpu)
        for path, s in decoder_forward_paths(dm, z, ei, et, monkeypatch).items():
            check_saturated_scores(s, gr.t(side + "_logit64"), "{} list, {}".format(side, path))
            assert float((s.cpu() - gr.t(side + "_score")).abs().max()) <= 2e-5, (side, path)
    _hip.raise_if_index_errors(gpu)


def test_decoder_sigmoid_sweep(gpu, monkeypatch):
    """Logits that are exact in fp32 (one non-zero feature per row: 1 * |x| * (+-1)) over [-110, 110], dense in
    [-20, 20], through every forward path.  Monotonicity in the logit is reported, not asserted: a reciprocal good to
    one ulp need not be monotone."""
    mag = torch.cat([torch.linspace(0, 20, 801), torch.linspace(20, 110, 181)[1:], torch.tensor([16.6, 16.64, 17.3, 17.33, 87.3, 88.7, 89.0, 103.9])])
    n, f = mag.numel() + 1, 16                                     # (about 1,000 nodes of 16 features: a table the planned kernel holds in LDS)
    z = torch.zeros(n, f)
    z[0, 0] = 1.0
    z[1:, 0] = mag
    ei = torch.stack([torch.zeros(2 * (n - 1), dtype=torch.int64), torch.arange(1, n).repeat(2)])
    et = torch.cat([torch.zeros(n - 1, dtype=torch.int64), torch.ones(n - 1, dtype=torch.int64)])
    dm = gripnet_amd.multiRelaInnerProductDecoder(f, 2).to(gpu)
    dm.weight.data.zero_()
    dm.weight.data[0, 0], dm.weight.data[1, 0] = 1.0, -1.0
    x = torch.cat([mag, -mag]).double()
    for path, s in decoder_forward_paths(dm, z.to(gpu), ei.to(gpu), et.to(gpu), monkeypatch).items():
        check_saturated_scores(s, x, "sweep, " + path)
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("way", ["spelled", "link_loss", "fused"])
def test_saturated_training_step_against_the_reference(gpu, golden, hooks, way):
    """Decoder + loss + backward on decoder_saturated, against the reference's fp32 run.  The hot relation contributes
    exactly nothing there (its positives and its negatives have s (1 - s) == 0 while dloss/ds is 1e13 / E), so dD of that
    relation and dz of the nodes that only hot triples touch must vanish."""
    gr = golden("decoder_saturated")
    dm = load_into(gripnet_amd.multiRelaInnerProductDecoder(gr.meta["F"], gr.meta["R"]), gr.state("dmt."), gpu)
    pos, neg, et = gr.t("pos_index", gpu), gr.t("neg_index", gpu), gr.t("edge_type", gpu)
    want = float(gr.t("loss32"))
    g32 = gc.stored(gr, "", "grad32")
    for call in range(2):
        dm.zero_grad()
        z = leaf(gr.t("z"), gpu)
        loss = link_loss_three_ways(way, dm, z, pos, neg, et)
        loss.backward()
        what = "saturated {} {} call {}".format(way, hooks, call)
        print("{}: loss {:.8g} vs {:.8g}".format(what, float(loss), want))
        for k, got in (("z", z.grad), ("dmt.weight", dm.weight.grad)):
            print("   {}: {:.2e} of its largest entry".format(k, float((got.cpu() - g32[k]).abs().max() / g32[k].abs().max())))
        assert abs(float(loss) - want) <= LOSS_REL * abs(want), (what, float(loss), want)
        gc.check_gradients({"z": z.grad, "dmt.weight": dm.weight.grad}, g32, GRAD_REL, what)
        assert float(dm.weight.grad[gr.meta["bands"]["hot"]].abs().max()) <= 1e-6 * float(g32["dmt.weight"].abs().max()), what
        assert float(z.grad[gr.meta["hot_only_nodes"]].abs().max()) <= 1e-6 * float(g32["z"].abs().max()), what
    _hip.raise_if_index_errors(gpu)
