"""The KGE scorers and their gradients (csrc/kge.hip, gripnet_amd.kge.KGEModel) on the GPU against float64.

The float64 reference is tests/kge_cases.py, which tests/test_kge_host.py pins to the reference's own runs.

Bounds.  u = 2^-24.  Every bound has the form  |got - ref64| <= c * u * scale  per element, with scale taken in float64:
sum_k |term_k| of the triple (gamma counts as a term for TransE and RotatE) for a raw score, and the sum over a row's records
of |contribution| for a gradient element.  Elements of zero scale - rows without a record, the zero subgradients - must be
exactly zero.

  c_s = min( (T + D) * kappa_s , 4 * t_s )
      T: roundings per term (kge_cases.TERM_ROUNDINGS: 2 / 2 / 7 / 16 for TransE / DistMult / ComplEx / RotatE);
      D: additions on the longest path of the sum (kge_cases.fold_depth: a lane's own columns, the cross-lane fold of its
         lane group, gamma - 8 at H = 32, 7 at H = 36 on the scalar path);
      kappa_s: the case's largest ratio of operand magnitudes to |term|s (kge_cases.condition_scores) - a count of roundings
         holds against the operands' magnitude, and a term that cancels inside is smaller than its operands;
      t_s: the figure max |s32 - s64| / (u * scale) that the fp32 torch formulation reaches on the same inputs on the CPU; the
         reference's op order is torch's, and a factor of 4 covers another summation tree.  (The shape cases of one (model, H)
         are prefixes of one 257-triple list on one pair of tables; a prefix takes the larger of its own figure and the
         whole list's: one triple, or the few elements of d_rel, are no sample.)
  log-sigmoid:  |y - y64| <= sigma(-s64) * c_s * u * scale + c_y * u * |y64|,  c_y = max(4, 2 * t_y)  with t_y torch's CPU fp32
      figure of logsigmoid on the same (fp32-rounded) scores; where |y64| < 2^-100:  -2^-99 <= y <= 0.
  c_g = min( (G + R) * kappa_g + (T + D) * kappa_s * max scale_s , 4 * t_g )
      G: roundings per contribution (kge_cases.CONTRIBUTION_ROUNDINGS: 6 / 7 / 9 / 26); R: additions on the longest path of
         the segmented sum (kge_cases.reduction_depth: a thread's share of a 2048-record chunk, the fold over the threads of
         a column, the chunks in order - 100 for the 5 000-record hub at 8 lanes per record); kappa_g:
         kge_cases.condition_gradients; the second summand is the score's own error, which moves sigma(-s) and with it all
         contributions of a triple; t_g: the figure of fp32 torch autograd on the CPU on the same inputs.

The test tables sit on a grid of 2^-16 (kge_cases.tables): TransE's h + r - t and its sum are then exact in fp32, so its
scores must be exact (t_s = 0) and its sign(h + r - t) is the float64 one.

Measured on an MI355X (the tests print every figure next to its bound; run with -s):
figure of the kernels / smallest bound c it was held to (torch fp32 on the CPU reaches a quarter of c where 4 t binds)
                               TransE          DistMult        ComplEx         RotatE
gradient case   scores         0 / 0 (exact)   3.11 / 8.00     2.31 / 11.10    1.56 / 6.25
                d_ent          2.62 / 61.3     2.78 / 223      2.50 / 58.8     3.46 / 76.0
                d_rel          3.06 / 59.1     1.70 / 222      4.15 / 107      2.53 / 81.9
                log-sigmoid    0.42 of bound   0.37            0.20            0.22
saturated       scores         0 / 0           1.75 / 6.41     2.29 / 8.86     1.63 / 8.20
                d_ent          2.16 / 10.7     5.18 / 10.6     3.35 / 10.7     4.84 / 17.8
                d_rel          1.33 / 16.9     1.45 / 16.2     1.38 / 13.9     1.80 / 6.59
size            scores         0 / 0           2.06 / 10.0     2.09 / 10.3     1.62 / 7.78
(E = 300 000)   d_ent          3.48 / 13.9     3.24 / 15.1     4.53 / 16.5     233 / 931
                d_rel          1.78 / 205      0.19 / 9.94     0.21 / 11.0     0.87 / 8.35
(RotatE's d_ent at the size case: among 9.6 million (a, b) some are far shorter than their operands, and a / sqrt(a^2 + b^2)
there carries the operands' rounding at that ratio; torch's fp32 run reaches 232.7 on the same inputs.)
shape cases (prefixes of one list per (model, H), H up to 72): every figure is at most 0.65 of its bound (TransE d_rel; scores
<= 0.30, d_ent <= 0.45, log-sigmoid values <= 0.44).  ComplEx at H = 1 and RotatE's d_ent reach figures in the hundreds and
above where a single term or a short (a, b) cancels (kappa large); torch's fp32 run rounds the same products the same way.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import gripnet_amd
import grad_cases
import kge_cases as kc
from gripnet_amd import _hip

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = kc.U



# ---- helpers -----------------------------------------------------------------------------------------------------------
def _sliced(t, left, width, dev):
    """`t` as the column view big[:, left:left + cols] of a [rows, width] matrix of NaN: a leading dimension above the row
    length, and nothing beside the view may be read into a result or written."""
    rows, cols = t.shape
    assert width >= left + cols
    big = torch.full((rows, width), NAN, device=dev)
    big[:, left:left + cols] = t.to(dev)
    return big, big[:, left:left + cols]


def _beside_is_nan(big, left, cols):
    return bool(torch.isnan(big[:, :left]).all()) and bool(torch.isnan(big[:, left + cols:]).all())


def _divisor(c):
    return kc.embedding_range(c.gamma, c.H) / kc.PI


def _forward(c, dev, log_sigmoid, ent=None, rel=None, sample=None, et=None):
    ent = c.ent.to(dev) if ent is None else ent
    rel = c.rel.to(dev) if rel is None else rel
    sample = (c.sample if sample is None else sample).to(dev)
    et = (c.et if et is None else et).to(dev)
    e = sample.shape[1]
    out, raw = torch.full((e,), 7.0, device=dev), torch.full((e,), 7.0, device=dev)
    _hip.kge_forward(c.model, ent, rel, sample, et, c.gamma, _divisor(c), log_sigmoid, out, raw if log_sigmoid else None)
    return out, raw


def _backward(c, dev, upstream, log_sigmoid=True, ent=None, rel=None, sample=None, et=None, types_sorted=None, d_ent=None,
              d_rel=None):
    ent = c.ent.to(dev) if ent is None else ent
    rel = c.rel.to(dev) if rel is None else rel
    sample = (c.sample if sample is None else sample).to(dev)
    et = (c.et if et is None else et).to(dev)
    raw = None
    if log_sigmoid:
        _, raw = _forward(c, dev, True, ent, rel, sample, et)
    d_ent = torch.full(tuple(ent.shape), NAN, device=dev) if d_ent is None else d_ent
    d_rel = torch.full(tuple(rel.shape), NAN, device=dev) if d_rel is None else d_rel
    _hip.kge_backward(c.model, ent, rel, sample, et, _divisor(c), upstream.to(dev), raw, d_ent, d_rel, types_sorted=types_sorted)
    return d_ent, d_rel


def _upstream(e):
    return torch.linspace(-1.0, 1.0, e) if e > 1 else torch.ones(e)


@functools.lru_cache(maxsize=None)
def _figures(key):
    """What one case's bounds are made of, computed once on the CPU: float64 scores and gradients, the scales, the figures
    of the fp32 torch formulation and the derived constants."""
    c = _CASES[key]()
    m, args = c.model, (c.ent, c.rel, c.sample, c.et, c.gamma)
    r = {"case": c}
    r["s64"] = kc.raw_score(m, c.ent.double(), c.rel.double(), c.sample, c.et, c.gamma)
    r["y64"] = F.logsigmoid(r["s64"])
    r["scale_s"] = kc.abs_term_sum(m, *args)
    depth = max(kc.fold_depth(c.H, True), kc.fold_depth(c.H, False))
    if c.E:
        r["t_s"] = kc.figure(kc.raw_score(m, *args), r["s64"], r["scale_s"])
        kappa_s = kc.condition_scores(m, *args)
        r["derived_s"] = (kc.TERM_ROUNDINGS[m] + depth) * kappa_s
        s32 = r["s64"].float()
        y_ref = F.logsigmoid(s32.double())
        big = y_ref.abs() >= 2.0 ** -100
        r["t_y"] = float(((F.logsigmoid(s32).double() - y_ref).abs()[big] / (U * y_ref.abs()[big])).max()) if bool(big.any()) else 0.0
        r["up"] = _upstream(c.E)
        r["g64"] = kc.reference_gradients(m, *args, r["up"], torch.float64)
        r["scale_g"] = kc.abs_contributions(m, *args, r["up"])
        g32 = kc.reference_gradients(m, *args, r["up"], torch.float32)
        r["t_g"] = [kc.figure(a, b, s, strict=False) for a, b, s in zip(g32, r["g64"], r["scale_g"])]
        kappa_g = kc.condition_gradients(m, *args)
        longest = [int(max(torch.bincount(c.sample[0], minlength=1).max(), torch.bincount(c.sample[1], minlength=1).max())),
                   int(torch.bincount(c.et, minlength=1).max())]
        lanes = 8 if c.H <= 32 else 16
        r["derived_g"] = [(kc.CONTRIBUTION_ROUNDINGS[m] + kc.reduction_depth(n, lanes)) * kappa_g
                          + (kc.TERM_ROUNDINGS[m] + depth) * kappa_s * float(r["scale_s"].max()) for n in longest]
    return r


@functools.lru_cache(maxsize=None)
def _reference(key):
    """A case's figures and its bounds' constants.  Every list is held to the torch figures of its own inputs.  The lists of a
    shape family are prefixes of one 257-triple list on one pair of tables; a prefix takes the larger of its own figure and
    the whole list's: the maximum over one or a few elements is no measure of an arithmetic's error (one triple; the
    4 x Dr elements of d_rel at any E)."""
    r = dict(_figures(key))
    if not r["case"].E:
        return r
    if key[0] == "shape":
        whole = _figures(key[:3] + (kc.SHAPE_E[-1],))
        r["t_s"], r["t_y"] = max(r["t_s"], whole["t_s"]), max(r["t_y"], whole["t_y"])
        r["t_g"] = [max(a, b) for a, b in zip(r["t_g"], whole["t_g"])]
    r["c_s"] = min(r["derived_s"], 4 * r["t_s"])
    r["c_y"] = max(4.0, 2 * r["t_y"])
    r["c_g"] = [min(d, 4 * t) for d, t in zip(r["derived_g"], r["t_g"])]
    return r


def _check_scores(r, raw, y, what, keep=None):
    """raw scores and log-sigmoid values against the case's float64 reference at its bounds (keep: the positions to compare)."""
    s64, y64, scale = r["s64"], r["y64"], r["scale_s"]
    raw, y = raw.cpu().double(), y.cpu().double()
    if keep is not None:
        raw, y = raw[keep], y[keep]
    fig = kc.figure(raw, s64, scale)
    print("{}: scores {:.2f} (bound {:.2f}, torch fp32 {:.2f})".format(what, fig, r["c_s"], r["t_s"]))
    assert fig <= r["c_s"], (what, fig, r["c_s"])
    bound = torch.sigmoid(-s64) * r["c_s"] * U * scale + r["c_y"] * U * y64.abs()
    tiny = y64.abs() < 2.0 ** -100
    err = (y - y64).abs()
    worst = float((err[~tiny] / bound[~tiny].clamp_min(1e-300)).max()) if bool((~tiny).any()) else 0.0
    print("{}: log-sigmoid at {:.2f} of its bound (c_y {:.2f})".format(what, worst, r["c_y"]))
    assert bool((err[~tiny] <= bound[~tiny]).all()), (what, worst)
    assert bool(((y[tiny] <= 0) & (y[tiny] >= -2.0 ** -99)).all()), what


def _check_gradients(r, got, what):
    for g, ref, scale, c_g, t_g, name in zip(got, r["g64"], r["scale_g"], r["c_g"], r["t_g"], ("d_ent", "d_rel")):
        assert bool(torch.isfinite(g).all()), (what, name)
        fig = kc.figure(g, ref, scale)
        print("{}: {} {:.2f} (bound {:.2f}, torch fp32 {:.2f})".format(what, name, fig, c_g, t_g))
        assert fig <= c_g, (what, name, fig, c_g)


_CASES = {}
for _m in kc.MODELS:
    _CASES[("gradient", _m)] = functools.partial(kc.gradient_case, _m)
    _CASES[("saturated", _m)] = functools.partial(kc.saturated_case, _m)
    _CASES[("size", _m)] = functools.partial(kc.case, _m, 20000, 37, 32, 300000, seed=3)
    for _h in kc.SHAPE_H:
        for _e in kc.SHAPE_E:
            _CASES[("shape", _m, _h, _e)] = functools.partial(kc.shape_case, _m, _h, _e)


# ---- fixture parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [m + "." + s for m in kc.MODELS for s in ("small", "driver")])
def test_fixture_parity(gpu, golden, tag):
    """The module on the reference's own state dicts: out / out_neg, and the gradients of both tables under the reference's
    loss (:266-268) against grad64 at the decoder bar of test_gpu_backward.py (1e-4 of the gradient's largest entry)."""
    fx = golden("kge_cases")
    c = next(k for k in fx.meta["cases"] if k["tag"] == tag)
    g = lambda k: fx.t(tag + "." + k)
    model = gripnet_amd.KGEModel(c["model"], c["n"], c["R"], c["H"], c["gamma"])
    model.load_state_dict({k[len(tag) + 4:]: fx.t(k) for k in fx.arrays if k.startswith(tag + ".sd.")})
    model = model.to(gpu)
    sample, neg, et = g("sample").to(gpu), g("neg").to(gpu), g("et").to(gpu)
    neg_score = model(neg, et)
    pos_score = model(sample, et)
    loss = kc.loss_expr(pos_score, neg_score)
    loss.backward()
    _hip.raise_if_index_errors(gpu)
    ent, rel = g("sd.entity_embedding"), g("sd.relation_embedding")
    for lst, y, key in ((g("sample"), pos_score, "out"), (g("neg"), neg_score, "out_neg")):
        args = (c["model"], ent, rel, lst, g("et"), c["gamma"])
        s64, scale = kc.raw_score(c["model"], ent.double(), rel.double(), lst, g("et"), c["gamma"]), kc.abs_term_sum(*args)
        depth = max(kc.fold_depth(c["H"], True), kc.fold_depth(c["H"], False))
        c_s = (kc.TERM_ROUNDINGS[c["model"]] + depth) * kc.condition_scores(*args)
        y64 = g(key + "64")
        own = torch.sigmoid(-s64) * c_s * U * scale + 4 * U * y64.abs()
        y = y.detach().cpu().double()
        assert bool(((y - y64).abs() <= own).all()), (key, float(((y - y64).abs() / own).max()))
        # against the reference's fp32 values: this kernel's bound plus the reference's own distance from float64
        assert bool(((y - g(key).double()).abs() <= own + (g(key).double() - y64).abs()).all()), key
    assert abs(float(loss.detach()) - float(g("loss64"))) <= 1e-5 * abs(float(g("loss64")))
    got = {"entity_embedding": model.entity_embedding.grad, "relation_embedding": model.relation_embedding.grad}
    grad_cases.check_gradients(got, grad_cases.stored(fx, tag + ".", "grad64"), 1e-4, tag)
    assert model.gamma.grad is None and model.embedding_range.grad is None


# ---- scores and gradients per element ------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", kc.MODELS)
@pytest.mark.parametrize("kind", ["gradient", "saturated", "size"])
def test_scores_and_gradients_per_element(gpu, model, kind):
    """Raw scores, log-sigmoid values and one backward against float64, per element.  `gradient`: the reduction's edge cases
    (kge_cases.gradient_case); `saturated`: scores of about +-80 - finite gradients; `size`: n = 20 000, R = 37, H = 32,
    E = 300 000, the shape of test_distmult_improved_baseline_caller."""
    r = _reference((kind, model))
    c = r["case"]
    what = "{} {}".format(model, kind)
    y, raw = _forward(c, gpu, True)
    plain, _ = _forward(c, gpu, False)
    assert torch.equal(plain, raw)                              # the raw scores are the same bits in both output modes
    _check_scores(r, raw, y, what)
    got = [g.cpu() for g in _backward(c, gpu, r["up"])]
    _check_gradients(r, got, what)
    _hip.raise_if_index_errors(gpu)
    if kind == "gradient":
        assert float(got[0][c.unused_entity].abs().max()) == 0.0
        assert float(got[1][list(c.empty_relations)].abs().max()) == 0.0
        # two calls: the same bits
        again = _backward(c, gpu, r["up"])
        assert torch.equal(again[0].cpu(), got[0]) and torch.equal(again[1].cpu(), got[1])
        # the promise of a sorted edge_type kept and not given, and the same list shuffled: the same gradients to the bound
        unsorted_route = [g.cpu() for g in _backward(c, gpu, r["up"], types_sorted=False)]
        _check_gradients(r, unsorted_route, what + " (sort route)")
        assert torch.equal(unsorted_route[0], got[0])           # (the entity passes do not depend on the flag)
        perm = torch.randperm(c.E, generator=torch.Generator().manual_seed(1))
        shuffled = [g.cpu() for g in _backward(c, gpu, r["up"][perm], sample=c.sample[:, perm].contiguous(),
                                               et=c.et[perm].contiguous(), types_sorted=False)]
        _check_gradients(r, shuffled, what + " (shuffled)")
        # gradient with respect to the raw scores (KGEModel.score)
        g64 = kc.reference_gradients(model, c.ent, c.rel, c.sample, c.et, c.gamma, r["up"], torch.float64, log_sigmoid=False)
        scale = kc.abs_contributions(model, c.ent, c.rel, c.sample, c.et, c.gamma, r["up"], log_sigmoid=False)
        g32 = kc.reference_gradients(model, c.ent, c.rel, c.sample, c.et, c.gamma, r["up"], torch.float32, log_sigmoid=False)
        for g, ref, s, t32, name in zip(_backward(c, gpu, r["up"], log_sigmoid=False), g64, scale, g32, ("d_ent", "d_rel")):
            fig, t_g = kc.figure(g, ref, s), kc.figure(t32, ref, s, strict=False)
            print("{} raw: {} {:.2f} (torch fp32 {:.2f})".format(what, name, fig, t_g))
            assert fig <= 4 * t_g, (what, name, fig, t_g)


@pytest.mark.parametrize("model", ["TransE", "RotatE"])
def test_zero_subgradients(gpu, model):
    """h == t and r = 0: logsigmoid(gamma) and all-zero, finite gradients (sign(0) = 0; a = b = 0 contributes nothing)."""
    for H in (3, 4):
        c = kc.case(model, 6, 2, H, 70, seed=2)
        c.rel.zero_()
        c.sample[1] = c.sample[0]
        y, raw = _forward(c, gpu, True)
        assert torch.equal(raw.cpu(), torch.full((70,), c.gamma))
        y64 = F.logsigmoid(torch.tensor(c.gamma, dtype=torch.float64))
        assert float((y.cpu().double() - y64).abs().max()) <= 4 * U * abs(float(y64))
        d_ent, d_rel = _backward(c, gpu, torch.ones(70))
        assert float(d_ent.abs().max()) == 0.0 and float(d_rel.abs().max()) == 0.0


# ---- shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", kc.MODELS)
@pytest.mark.parametrize("H", kc.SHAPE_H)
def test_shapes(gpu, model, H):
    """H: kge_cases.shape_case (scalar path, one vector piece, the driver's size, ragged trips, and at 72 the vector path's
    second trip and second column block); E around the wave's 64 triples, prefixes of one list; the tables contiguous, as column views with ld = D + 1 (the scalar path) and ld = D + 4,
    NaN beside them: nothing beside a view may be read into a result or written."""
    for E in kc.SHAPE_E:
        r = _reference(("shape", model, H, E))
        c = r["case"]
        de, dr = kc.dims(model, H)
        for pad in (0, 1, 4):
            what = "{} H={} E={} ld=D+{}".format(model, H, E, pad)
            if pad:                                             # NaN left of the entity rows and of d_rel, right of the relation rows and of d_ent
                big_e, ent = _sliced(c.ent, pad, de + pad, gpu)
                big_r, rel = _sliced(c.rel, 0, dr + pad, gpu)
                big_de, d_ent = _sliced(torch.full((c.n, de), NAN), 0, de + pad, gpu)
                big_dr, d_rel = _sliced(torch.full((c.R, dr), NAN), pad, dr + pad, gpu)
            else:
                ent, rel, d_ent, d_rel = c.ent.to(gpu), c.rel.to(gpu), None, None
            y, raw = _forward(c, gpu, True, ent, rel)
            assert y.shape == (E,)
            if E == 0:
                d_ent, d_rel = _backward(c, gpu, torch.ones(0), ent=ent, rel=rel, d_ent=d_ent, d_rel=d_rel)
                assert float(d_ent.abs().sum()) == 0.0 and float(d_rel.abs().sum()) == 0.0
            else:
                _check_scores(r, raw, y, what)
                got = _backward(c, gpu, r["up"], ent=ent, rel=rel, d_ent=d_ent, d_rel=d_rel)
                _check_gradients(r, [g.cpu() for g in got], what)
            if pad:
                assert _beside_is_nan(big_e, pad, de) and _beside_is_nan(big_r, 0, dr), what
                assert _beside_is_nan(big_de, 0, de) and _beside_is_nan(big_dr, pad, dr), what + ": written beside the gradients"
    _hip.raise_if_index_errors(gpu)


# ---- ids ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", kc.MODELS)
@pytest.mark.parametrize("relations", [True, False])
def test_ids_outside_the_tables(gpu, model, relations):
    """A negative or too large head, tail or relation: that score is NaN, the flag is set and raise_if_index_errors raises
    IndexError; every other score and the gradients are the same bits as without the bad triples (the relation gradient of
    the in-place pass: to the bound).  `relations` False: edge_type stays sorted, so the
    relation pass keeps its records in list order and has to skip the bad ones there."""
    r = _reference(("gradient", model))
    c = r["case"]
    sample, et, good = kc.with_bad_ids(c, relations)
    _hip.raise_if_index_errors(gpu)
    clean_y, clean_raw = _forward(c, gpu, True)
    y, raw = _forward(c, gpu, True, sample=sample, et=et)
    with pytest.raises(IndexError):
        _hip.raise_if_index_errors(gpu)
    _hip.raise_if_index_errors(gpu)                             # (the flag is cleared by the check)
    assert bool(torch.isnan(y.cpu()[~good]).all()) and bool(torch.isnan(raw.cpu()[~good]).all())
    assert torch.equal(y.cpu()[good], clean_y.cpu()) and torch.equal(raw.cpu()[good], clean_raw.cpu())
    up = torch.zeros(sample.shape[1])
    up[good] = r["up"]
    up[~good] = 3.0
    got = [g.cpu() for g in _backward(c, gpu, up, sample=sample, et=et)]
    _check_gradients(r, got, "{} bad ids".format(model))
    # A pass that sorts gives the bad records the key behind the last row, and the sort is stable: the good records keep
    # their places, so the sums are the same bits.  The head and tail passes always sort; the relation pass sorts unless
    # edge_type is sorted (relations False) - there the bad records sit between the good ones and the chunks' cuts move.
    clean = [g.cpu() for g in _backward(c, gpu, r["up"], types_sorted=False)]
    assert torch.equal(got[0], clean[0])
    if relations:
        assert torch.equal(got[1], clean[1])
    with pytest.raises(IndexError):                             # (the backward's own forward saw them again)
        _hip.raise_if_index_errors(gpu)


# ---- training ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", kc.MODELS)
def test_three_adam_steps(gpu, golden, model):
    """Three torch.optim.Adam steps of the reference's loss on the fixture's driver-sized case with its fixed negatives: the
    loss after each step within 1e-5 relative of the same loop on the fp32 torch formulation (the bar of the
    reference-autograd gradient fixtures)."""
    fx = golden("kge_cases")
    tag = model + ".driver"
    c = next(k for k in fx.meta["cases"] if k["tag"] == tag)
    g = lambda k: fx.t(tag + "." + k)
    sd = {k[len(tag) + 4:]: fx.t(k) for k in fx.arrays if k.startswith(tag + ".sd.")}
    m = gripnet_amd.KGEModel(model, c["n"], c["R"], c["H"], c["gamma"])
    m.load_state_dict(sd)
    m = m.to(gpu)
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    ent = sd["entity_embedding"].clone().requires_grad_(True)
    rel = sd["relation_embedding"].clone().requires_grad_(True)
    ref_opt = torch.optim.Adam([ent, rel], lr=0.01)
    sample, neg, et = g("sample"), g("neg"), g("et")
    d_sample, d_neg, d_et = sample.to(gpu), neg.to(gpu), et.to(gpu)
    for step in range(4):
        opt.zero_grad()
        loss = kc.loss_expr(m(d_sample, d_et), m(d_neg, d_et))
        ref_opt.zero_grad()
        ref = kc.loss_expr(kc.log_sigmoid_score(model, ent, rel, sample, et, c["gamma"]),
                           kc.log_sigmoid_score(model, ent, rel, neg, et, c["gamma"]))
        assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach())), (step, float(loss.detach()), float(ref.detach()))
        if step == 3:
            break
        loss.backward()
        opt.step()
        ref.backward()
        ref_opt.step()
    _hip.raise_if_index_errors(gpu)
