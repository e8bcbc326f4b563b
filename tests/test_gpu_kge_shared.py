"""The KGE scorers on shared candidate lists (csrc/kge_shared.hip, KGEModel's 'tail-shared' / 'head-shared' modes) on the GPU
against float64.

The float64 reference is kge_batch_cases' on the block that the lists stand for (kge_shared_cases.expand_lists:
negatives[g].expand per chunk), which is kge_cases' formulation on the expanded triple list; nothing is computed twice.

Bounds: the rule at the head of tests/test_gpu_kge.py, |got - ref64| <= c * u * scale per element, elements of zero scale
exactly zero, with this kernel's own depths from tests/kge_shared_cases.py:
  c_s = min((T + D) * kappa_s, 4 * t_s)    D = kge_shared_cases.score_depth: H + 1 (TransE, RotatE: one serial chain and gamma),
                                           DistMult / ComplEx: the row's groups of 16 columns go to four partial chains of
                                           fused multiply-adds on the matrix cores, added pairwise: 34 at a row of 128
  c_g = min((G + R) * kappa_g + (T + D) * kappa_s * max scale_s, 4 * t_g)    R = kge_shared_cases.gradient_depths
  log-sigmoid: sigma(-s64) * c_s * u * scale + c_y * u * |y64|,  c_y = max(4, 2 t_y)
t_s, t_y, t_g are the figures of the fp32 torch formulation on the CPU on the same inputs, computed here: every case is held to
its own.  One exception: shape a, (B, G, K) = (48, 1, 1), takes the larger of its own figures and those of shape e (6 000 scores
on the same pair of tables, kge_shared_cases.family_tables).  Its 48 scores - and at H = 1 the five elements of d_rel, where
torch's figure is 0.21 - are no sample of an arithmetic's error, as the head of tests/test_gpu_kge.py says of a one-triple
prefix; with its own figure alone TransE's d_rel at H = 1 measures 1.20 against 4 t = 0.85.
TransE's tables sit on the 2^-16 grid: t_s = 0, its scores must be exact - and are compared bit for bit with 'tail-batch' /
'head-batch' on the expanded block.  DistMult and ComplEx run on the matrix cores: their bits are not those of
mode="single", and are not asked to be.

Measured on an MI355X (the tests print every figure next to its bound; run with -s), over the five shapes, every width and
both sides, every case against the bound from its own torch figure (shape a as said above) - largest figure / smallest bound c
any case was held to / worst figure-to-bound ratio of any one case:
                 TransE                 DistMult               ComplEx                 RotatE
  scores         0 / 0 (exact)          2.23 / 1.38 / 0.72     51,686 / 1.48 / 0.78    4.40 / 3.29 / 0.76
  d_ent          14.5 / 3.80 / 0.41     7.22 / 7.83 / 0.28     10,163 / 5.49 / 0.38    5,833 / 9.71 / 0.62
  d_rel          2.83 / 1.86 / 0.52     2.68 / 4.63 / 0.38     5.15 / 0.98 / 0.45      20.2 / 1.31 / 0.33
  log-sigmoid    0.44 of its bound      0.43                   0.41                    0.71
(ComplEx at H = 1 and RotatE's d_ent reach figures in the thousands where a single term or a short (a, b) cancels - kappa is
large there and torch's fp32 run rounds the same products the same way: its figure is a quarter of the bound where 4 t binds.
DistMult at H = 128 measured 3.44 against a bound of 3.36 while its row was ONE chain of 128 fused multiply-adds; the four
partial chains of csrc/kge_shared.hip brought that case to 1.22.)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import gripnet_amd
import kge_batch_cases as kb
import kge_cases as kc
import kge_shared_cases as ks
from gripnet_amd import _hip, kge

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = kc.U


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _divisor(c):
    return kc.embedding_range(c.gamma, c.H) / kc.PI


def _operands(c, dev, positive=None, et=None, lists=None, ent=None, rel=None):
    ent = c.ent.to(dev) if ent is None else ent
    rel = c.rel.to(dev) if rel is None else rel
    fixed = kb.fixed_of(c.positive if positive is None else positive, c.side).to(dev)
    et = (c.et if et is None else et).to(dev)
    lists = (c.lists if lists is None else lists).to(dev)
    return ent, rel, fixed, et, lists


def _forward(c, dev, log_sigmoid, out=None, raw=None, **ids):
    """(out, raw) of the shared-list kernel, both prefilled with a sentinel."""
    ent, rel, fixed, et, lists = _operands(c, dev, **ids)
    shape = (fixed.shape[0], lists.shape[1])
    out = torch.full(shape, 7.0, device=dev) if out is None else out
    raw = torch.full(shape, 7.0, device=dev) if raw is None else raw
    _hip.kge_shared_forward(c.model, ent, rel, fixed, et, lists, c.side, c.gamma, _divisor(c), log_sigmoid, out,
                            raw if log_sigmoid else None)
    return out, raw


def _backward(c, dev, upstream, log_sigmoid=True, types_sorted=None, **ids):
    raw = None
    if log_sigmoid:
        _, raw = _forward(c, dev, True, **ids)
    ent, rel, fixed, et, lists = _operands(c, dev, **ids)
    d_ent = torch.full(tuple(ent.shape), NAN, device=dev)
    d_rel = torch.full(tuple(rel.shape), NAN, device=dev)
    _hip.kge_shared_backward(c.model, ent, rel, fixed, et, lists, c.side, _divisor(c), upstream.to(dev), raw, d_ent, d_rel,
                             types_sorted=types_sorted)
    return d_ent, d_rel


@functools.lru_cache(maxsize=None)
def _figures(model, side, H, name):
    """What one case's bounds are made of, computed once on the CPU and left unchanged: float64 scores and gradients, the
    scales, the figures of the fp32 torch formulation, the condition numbers and the derived constants."""
    c = ks.case(model, side, H, name)
    args = (c.ent, c.rel, c.sample, c.et_list, c.gamma)
    r = {"case": c, "up": ks.upstream(c)}
    r["s64"] = kc.raw_score(model, c.ent.double(), c.rel.double(), c.sample, c.et_list, c.gamma)
    r["y64"] = F.logsigmoid(r["s64"])
    r["scale_s"] = kc.abs_term_sum(model, *args)
    r["t_s"] = kc.figure(kc.raw_score(model, *args), r["s64"], r["scale_s"])
    s32 = r["s64"].float()
    y_ref = F.logsigmoid(s32.double())
    big = y_ref.abs() >= 2.0 ** -100
    r["t_y"] = float(((F.logsigmoid(s32).double() - y_ref).abs()[big] / (U * y_ref.abs()[big])).max()) if bool(big.any()) else 0.0
    up = r["up"].reshape(-1)
    r["g64"] = kc.reference_gradients(model, *args, up, torch.float64)
    r["scale_g"] = kc.abs_contributions(model, *args, up)
    g32 = kc.reference_gradients(model, *args, up, torch.float32)
    r["t_g"] = [kc.figure(a, b, s, strict=False) for a, b, s in zip(g32, r["g64"], r["scale_g"])]
    kappa_s, kappa_g = kc.condition_scores(model, *args), kc.condition_gradients(model, *args)
    own_s = (kc.TERM_ROUNDINGS[model] + ks.score_depth(model, H)) * kappa_s
    r["derived_s"] = own_s
    r["derived_g"] = [(kc.CONTRIBUTION_ROUNDINGS[model] + depth) * kappa_g + own_s * float(r["scale_s"].max())
                      for depth in ks.gradient_depths(c)]
    return r


@functools.lru_cache(maxsize=None)
def _reference(model, side, H, name):
    """A case's figures and its bounds' constants: the torch figures are the case's own, on its own inputs.  Shape a alone -
    48 scores, and at H = 1 five elements of d_rel - also takes the figures of shape e (6 000 scores on the same tables): the
    module docstring says why."""
    r = dict(_figures(model, side, H, name))
    if name == "a":
        whole = _figures(model, side, H, "e")
        r["t_s"], r["t_y"] = max(r["t_s"], whole["t_s"]), max(r["t_y"], whole["t_y"])
        r["t_g"] = [max(a, b) for a, b in zip(r["t_g"], whole["t_g"])]
    r["c_s"] = min(r["derived_s"], 4 * r["t_s"])
    r["c_y"] = max(4.0, 2 * r["t_y"])
    r["c_g"] = [min(d, 4 * t) for d, t in zip(r["derived_g"], r["t_g"])]
    return r


def _check_scores(r, raw, y, what, keep=None):
    """Raw scores and log-sigmoid values against float64 at the case's bounds (keep: a [B, K] mask of the elements to compare)."""
    s64, y64, scale = r["s64"], r["y64"], r["scale_s"]
    raw, y = raw.cpu().double().reshape(-1), y.cpu().double().reshape(-1)
    if keep is not None:
        keep = keep.reshape(-1)
        raw, y, s64, y64, scale = raw[keep], y[keep], s64[keep], y64[keep], scale[keep]
    fig = kc.figure(raw, s64, scale)
    print("{}: scores {:.2f} (bound {:.2f}: derived {:.1f}, torch fp32 {:.2f})".format(what, fig, r["c_s"], r["derived_s"], r["t_s"]))
    assert fig <= r["c_s"], (what, fig, r["c_s"])
    bound = torch.sigmoid(-s64) * r["c_s"] * U * scale + r["c_y"] * U * y64.abs()
    tiny = y64.abs() < 2.0 ** -100
    err = (y - y64).abs()
    worst = float((err[~tiny] / bound[~tiny].clamp_min(1e-300)).max()) if bool((~tiny).any()) else 0.0
    print("{}: log-sigmoid at {:.2f} of its bound (c_y {:.2f})".format(what, worst, r["c_y"]))
    assert bool((err[~tiny] <= bound[~tiny]).all()), (what, worst)
    assert bool(((y[tiny] <= 0) & (y[tiny] >= -2.0 ** -99)).all()), what


def _check_gradients(r, got, what, g64=None, scale=None):
    g64 = r["g64"] if g64 is None else g64
    scale = r["scale_g"] if scale is None else scale
    for g, ref, sc, c_g, t_g, d, name in zip(got, g64, scale, r["c_g"], r["t_g"], r["derived_g"], ("d_ent", "d_rel")):
        assert bool(torch.isfinite(g).all()), (what, name)
        fig = kc.figure(g, ref, sc)
        print("{}: {} {:.2f} (bound {:.2f}: derived {:.1f}, torch fp32 {:.2f})".format(what, name, fig, c_g, d, t_g))
        assert fig <= c_g, (what, name, fig, c_g)


# ---- scores and gradients against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ks.SHAPES))
@pytest.mark.parametrize("side", ks.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_scores_and_gradients_against_float64(gpu, model, side, name):
    """Every shape of kge_shared_cases.SHAPES at every width of kge_shared_cases.widths: raw scores, log-sigmoid values, d_ent
    and d_rel per element; rows that nothing touched are exact zeros; TransE's scores are the block kernel's bits."""
    for H in ks.widths(model):
        r = _reference(model, side, H, name)
        c = r["case"]
        what = "{} {} H={} shape {} (B, G, K) = {}".format(model, side, H, name, ks.SHAPES[name])
        plain, _ = _forward(c, gpu, False)
        y, raw = _forward(c, gpu, True)
        assert plain.shape == (c.B, c.K) and torch.equal(raw, plain), what
        _check_scores(r, plain, y, what)
        if model == "TransE":
            ent, rel, fixed, et, _ = _operands(c, gpu)
            block = _hip.kge_batch_forward(model, ent, rel, fixed, et, c.negatives.to(gpu), side, c.gamma, _divisor(c), False,
                                           torch.full((c.B, c.K), -3.0, device=gpu))
            assert torch.equal(plain, block), what
        got = [g.cpu() for g in _backward(c, gpu, r["up"])]
        _check_gradients(r, got, what)
        assert float(got[0][c.unused_entity].abs().max()) == 0.0, what
        assert float(got[1][c.unused_relation].abs().max()) == 0.0, what
        if name == "b":                                             # the identity upstream (no log-sigmoid factor) and the sort route
            plain_up = [g.cpu() for g in _backward(c, gpu, r["up"], log_sigmoid=False, types_sorted=False)]
            g64 = kc.reference_gradients(model, c.ent, c.rel, c.sample, c.et_list, c.gamma, r["up"].reshape(-1), torch.float64, log_sigmoid=False)
            scale = kc.abs_contributions(model, c.ent, c.rel, c.sample, c.et_list, c.gamma, r["up"].reshape(-1), log_sigmoid=False)
            g32 = kc.reference_gradients(model, c.ent, c.rel, c.sample, c.et_list, c.gamma, r["up"].reshape(-1), torch.float32, log_sigmoid=False)
            own = dict(r)
            own["t_g"] = [kc.figure(a, b, s, strict=False) for a, b, s in zip(g32, g64, scale)]
            own["c_g"] = [min(d, 4 * t) for d, t in zip(r["derived_g"], own["t_g"])]
            _check_gradients(own, plain_up, what + " (raw upstream)", g64, scale)
    _hip.raise_if_index_errors(gpu)


# ---- 16-byte stores, strided tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ks.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_vector_stores_and_strided_tables(gpu, model, side):
    """K % 4 == 0 with aligned outputs takes the 16-byte stores (no shape of SHAPES does): the same bits as the float-at-a-time
    route, which outputs that start 4 bytes past an aligned address take, at K = 8 (one partial stage) and K = 68 (a stage and a
    4-column rest).  Tables as column views of wider NaN matrices (ld = D + 3): the same bits, forward and backward."""
    for K in (8, 68):
        c0 = ks.case(model, side, 36, "c")
        lists = torch.randint(0, ks.N - 1, (c0.G, K), generator=torch.Generator().manual_seed(K))
        c = kb._case(model, side, ks.N, ks.R, 36, c0.gamma, c0.ent, c0.rel, c0.positive, c0.et, ks.expand_lists(lists, c0.B), lists=lists, G=c0.G)
        s64 = kc.raw_score(model, c.ent.double(), c.rel.double(), c.sample, c.et_list, c.gamma).view(c.B, K)
        y, raw = _forward(c, gpu, True)
        assert y.data_ptr() % 16 == 0 and raw.data_ptr() % 16 == 0
        flat_y, flat_raw = torch.full((c.B * K + 1,), 7.0, device=gpu), torch.full((c.B * K + 1,), 7.0, device=gpu)
        y1, raw1 = _forward(c, gpu, True, out=flat_y[1:].view(c.B, K), raw=flat_raw[1:].view(c.B, K))
        assert y1.data_ptr() % 16 == 4
        assert torch.equal(y, y1) and torch.equal(raw, raw1), (model, side, K)
        assert float(flat_y[0]) == 7.0 and float(flat_raw[0]) == 7.0
        scale = kc.abs_term_sum(model, c.ent, c.rel, c.sample, c.et_list, c.gamma).view(c.B, K)
        derived = (kc.TERM_ROUNDINGS[model] + ks.score_depth(model, 36)) * kc.condition_scores(model, c.ent, c.rel, c.sample, c.et_list, c.gamma)
        t_s = kc.figure(kc.raw_score(model, c.ent, c.rel, c.sample, c.et_list, c.gamma).view(c.B, K), s64, scale)
        fig = kc.figure(raw, s64, scale)
        print("{} {} K={}: scores {:.2f} (bound {:.2f}: derived {:.1f}, torch fp32 {:.2f})".format(model, side, K, fig, min(derived, 4 * t_s), derived, t_s))
        assert fig <= min(derived, 4 * t_s), (model, side, K, fig)
        de, dr = kc.dims(model, 36)
        big_e = torch.full((ks.N, de + 3), NAN, device=gpu)
        big_r = torch.full((ks.R, dr + 3), NAN, device=gpu)
        big_e[:, 3:] = c.ent.to(gpu)
        big_r[:, :dr] = c.rel.to(gpu)
        y2, raw2 = _forward(c, gpu, True, ent=big_e[:, 3:], rel=big_r[:, :dr])
        assert torch.equal(y, y2) and torch.equal(raw, raw2), (model, side, K)
        up = ks.upstream(c)
        g0 = _backward(c, gpu, up)
        g1 = _backward(c, gpu, up, ent=big_e[:, 3:], rel=big_r[:, :dr])
        assert torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1]), (model, side, K)
    _hip.raise_if_index_errors(gpu)


# ---- the same bits in every call, and under capture ---------------------------------------------------------------------------
@pytest.mark.parametrize("side", ks.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_same_bits_in_every_call_and_under_capture(gpu, model, side):
    """Shape b at H = 36: two calls give the same bits for the scores and both gradients; forward plus backward captured with
    torch.cuda.graph (no host synchronisation inside: the capture would fail) and replayed once give the eager bits."""
    c = ks.case(model, side, 36, "b")
    ent, rel, fixed, et, lists = _operands(c, gpu)
    up = ks.upstream(c).to(gpu)

    def step():
        y, raw = torch.full((c.B, c.K), NAN, device=gpu), torch.full((c.B, c.K), NAN, device=gpu)
        d_ent, d_rel = torch.full_like(ent, NAN), torch.full_like(rel, NAN)
        _hip.kge_shared_forward(model, ent, rel, fixed, et, lists, side, c.gamma, _divisor(c), True, y, raw)
        _hip.kge_shared_backward(model, ent, rel, fixed, et, lists, side, _divisor(c), up, raw, d_ent, d_rel, types_sorted=False)
        return y, raw, d_ent, d_rel

    eager = [t.clone() for t in step()]
    for a, b in zip(eager, step()):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    _hip.raise_if_index_errors(gpu)


# ---- the module ------------------------------------------------------------------------------------------------------------
def _module(c, dev):
    m = gripnet_amd.KGEModel(c.model, c.n, c.R, c.H, c.gamma)
    with torch.no_grad():
        m.entity_embedding.copy_(c.ent)
        m.relation_embedding.copy_(c.rel)
    return m.to(dev)


@pytest.mark.parametrize("side", ks.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_module_modes_are_the_kernels_and_the_loss_is_its_parts(gpu, model, side):
    """KGEModel.forward / .score in the shared modes return the kernels' bits (with and without autograd), autograd returns the
    backward kernel's, and model.negative_sampling_loss(..., mode=) equals kge.negative_sampling_loss applied to the two score
    calls bit for bit - the loss and both gradients, with a temperature and subsampling weights."""
    c = ks.case(model, side, 8, "c")
    mode = ks.MODES[side]
    m = _module(c, gpu)
    positive, et, lists = c.positive.to(gpu), c.et.to(gpu), c.lists.to(gpu)
    want_y, want_raw = _forward(c, gpu, True)
    with torch.no_grad():
        assert torch.equal(m((positive, lists), et, mode=mode), want_y)
        assert torch.equal(m.score((positive, lists), et, mode=mode), want_raw)
    y = m((positive, lists), et, mode=mode)
    assert y.requires_grad and torch.equal(y.detach(), want_y)
    up = ks.upstream(c).to(gpu)
    got = torch.autograd.grad(y, (m.entity_embedding, m.relation_embedding), grad_outputs=up)
    want = _backward(c, gpu, up)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])

    weight = torch.linspace(0.5, 2.0, c.B, device=gpu)
    loss = m.negative_sampling_loss(positive, et, lists, mode=mode, adversarial_temperature=1.0, subsampling_weight=weight)
    loss.backward()
    g_fused = [m.entity_embedding.grad.clone(), m.relation_embedding.grad.clone()]
    m.zero_grad(set_to_none=True)
    parts = kge.negative_sampling_loss(m.score(positive, et), m.score((positive, lists), et, mode=mode), 1.0, weight)
    parts.backward()
    assert torch.equal(loss.detach(), parts.detach()) and bool(torch.isfinite(loss))
    assert torch.equal(g_fused[0], m.entity_embedding.grad) and torch.equal(g_fused[1], m.relation_embedding.grad)
    _hip.raise_if_index_errors(gpu)


def test_refused_width_on_the_device(gpu):
    for model in kc.MODELS:
        H = ks.first_refused_width(model)
        de, dr = kc.dims(model, H)
        ent, rel = torch.zeros(4, de, device=gpu), torch.zeros(2, dr, device=gpu)
        ids = torch.zeros(4, dtype=torch.long, device=gpu)
        with pytest.raises(ValueError, match="at most 128 floats"):
            _hip.kge_shared_forward(model, ent, rel, ids, ids, ids.view(2, 2), "tail", 12.0, 1.0, False, torch.empty(4, 2, device=gpu))
        with pytest.raises(ValueError, match="at most 128 floats"):
            _hip.kge_shared_backward(model, ent, rel, ids, ids, ids.view(2, 2), "tail", 1.0, torch.empty(4, 2, device=gpu), None,
                                     torch.empty_like(ent), torch.empty_like(rel))


# ---- ids outside the tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ks.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_bad_ids(gpu, model, side):
    """Shape b at H = 8 with a negative and a too large id among the fixed entities, the relations and the lists' entries
    (kge_shared_cases.with_bad_ids): NaN in the bad positives' rows and in the bad candidates' columns of THEIR chunk, nowhere
    else; every other score within its bounds; IndexError at _hip.raise_if_index_errors; the backward sums the good triples
    only (float64 on the list without the bad ones) and stays finite."""
    r = _reference(model, side, 8, "b")
    c = r["case"]
    positive, et, lists, rows, columns = ks.with_bad_ids(c)
    _hip.raise_if_index_errors(gpu)                                  # (nothing pending)
    plain, _ = _forward(c, gpu, False, positive=positive, et=et, lists=lists)
    y, raw = _forward(c, gpu, True, positive=positive, et=et, lists=lists)
    with pytest.raises(IndexError):
        _hip.raise_if_index_errors(gpu)
    bad = torch.zeros(c.B, c.K, dtype=torch.bool)
    bad[rows] = True
    chunk = ks.chunk_of(c.B, c.G)
    for g, k in columns:
        bad[chunk == g, k] = True
    what = "{} {} bad ids".format(model, side)
    for t in (plain, y, raw):
        assert torch.equal(torch.isnan(t.cpu()), bad), what
    _check_scores(r, plain, y, what, keep=~bad)
    up = r["up"]
    got = [g.cpu() for g in _backward(c, gpu, up, positive=positive, et=et, lists=lists)]
    with pytest.raises(IndexError):
        _hip.raise_if_index_errors(gpu)
    keep = (~bad).reshape(-1)
    sample, et_list, up_list = c.sample[:, keep], c.et_list[keep], up.reshape(-1)[keep]
    g64 = kc.reference_gradients(model, c.ent, c.rel, sample, et_list, c.gamma, up_list, torch.float64)
    scale = kc.abs_contributions(model, c.ent, c.rel, sample, et_list, c.gamma, up_list)
    _check_gradients(r, got, what, g64, scale)
