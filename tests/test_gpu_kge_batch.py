"""The KGE scorers on candidate blocks (csrc/kge_batch.hip, KGEModel's 'tail-batch' / 'head-batch' modes) on the GPU.

Scores: bit for bit those of the list kernel (_hip.kge_forward) on the expansion (kge_batch_cases.expand) - no tolerance;
the list kernel itself is held to float64 by tests/test_gpu_kge.py.

Gradients: against float64 autograd on the expansion (kge_cases.reference_gradients), per element, under the rule of
tests/test_gpu_kge.py:  |got - ref64| <= c_g * u * scale,  scale = the sum over a row's records of |contribution| in float64
(kge_cases.abs_contributions on the expansion), elements of zero scale exactly zero, and

  c_g = min( (G + R') * kappa_g + (T + D) * kappa_s * max scale_s , 4 * t_g )

with G, T, D, kappa_g, kappa_s as there, t_g the figure of fp32 torch autograd on the same expansion on the CPU, and R' the
additions on the longest path as kge_batch.hip builds it:
  d_rel:  kge_batch_cases.query_reduction_depth(K, positives of the busiest relation, lanes)
  d_ent:  the candidate pass's kge_cases.reduction_depth(records of the busiest candidate, lanes), the query-side depth of
          the busiest fixed entity, and the addition of the two passes.

Case C keeps gamma = 1 (kge_batch_cases.case_c): at gamma = 12 its three-column scores reach +-150, where sigma(-s) is
1e-66 in float64 and 0 in fp32 - a gradient below fp32's range, which no count of roundings in units of u describes.

Measured on an MI355X (the tests print every figure next to its bound; run with -s): figure of the kernels / the bound c_g
it was held to; 4 t_g binds everywhere (the derived constant is 49 to 7e7).  The sort route of the relation pass gives the
same figures to the digits shown.
                          TransE          DistMult        ComplEx         RotatE
case A  tail   d_ent      3.38 / 44.4     5.38 / 35.1     4.96 / 130      4.35 / 40.4
               d_rel      1.66 / 54.1     1.18 / 38.6     1.42 / 57.2     1.10 / 26.6
        head   d_ent      3.29 / 35.0     5.38 / 36.4     5.00 / 146      4.65 / 67.9
               d_rel      1.41 / 31.3     1.16 / 38.6     2.68 / 45.1     1.07 / 15.3
case B  tail   d_ent      2.71 / 41.5     4.12 / 16.5     5.16 / 19.3     18.0 / 52.3
               d_rel      2.11 / 24.6     0.72 / 9.96     1.20 / 11.4     1.11 / 9.75
        head   d_ent      3.20 / 45.0     4.69 / 23.7     4.87 / 19.4     16.5 / 79.6
               d_rel      2.72 / 41.7     0.88 / 12.7     1.37 / 12.1     1.17 / 9.04
case C  tail   d_ent      1.07 / 8.31     1.95 / 10.6     49.2 / 197      34.3 / 137
               d_rel      0.87 / 7.66     1.17 / 4.68     1.19 / 4.15     3.46 / 17.1
        head   d_ent      1.49 / 7.80     2.69 / 8.54     3.88 / 87.4     157 / 483
               d_rel      0.91 / 6.20     0.97 / 3.29     1.64 / 6.54     4.40 / 19.4
(ComplEx and RotatE at H = 3: a term that cancels inside, or a short (a, b), carries its operands' rounding at that ratio;
torch's fp32 run reaches 49.2, 34.3 and 121 on the same inputs.)
Through the module on case A (score / forward) every figure is at most 0.21 of its bound; with bad ids (case A without
the bad entries) at most 0.17.

Cases D and E (kge_batch_cases.case_d, case_e: rows of the passes over the positives across their chunks of 32 records; more
positives than the query kernel's grid).  4 t_g binds everywhere here too (the derived constant is 46 to 8e9).  Case D's
d_rel is the same bits from the shuffled block by the sort route and from the sorted block by either route
(test_the_sort_route_sorts), d_ent of the sorted block is the same from both routes, and the module gives the figures of
the direct call; case E gives the same figures by both routes.
                                  TransE          DistMult        ComplEx         RotatE
D H=8   tail  d_ent shuffled      2.50 / 13.3     3.28 / 13.0     7.65 / 26.8     7.35 / 29.4
              d_ent sorted        2.56 / 14.8     3.29 / 17.8     5.75 / 29.9     8.24 / 29.4
              d_rel               2.09 / 17.3     3.55 / 10.5     7.34 / 26.6     2.30 / 19.0
        head  d_ent shuffled      2.84 / 13.3     2.97 / 13.7     5.13 / 22.7     8.94 / 25.6
              d_ent sorted        3.36 / 32.7     3.42 / 15.2     3.66 / 21.7     8.94 / 27.6
              d_rel               1.97 / 33.0     1.85 / 9.39     3.62 / 21.5     3.22 / 8.46
D H=36  tail  d_ent shuffled      2.58 / 15.6     2.68 / 12.7     3.52 / 14.1     15.5 / 52.2
              d_ent sorted        3.34 / 16.6     4.32 / 16.0     3.47 / 16.6     15.5 / 52.2
              d_rel               2.50 / 20.1     1.40 / 8.16     1.51 / 7.73     5.02 / 32.6
        head  d_ent shuffled      3.01 / 13.2     2.68 / 12.7     3.95 / 15.1     23.9 / 91.1
              d_ent sorted        3.23 / 13.6     4.32 / 12.7     3.26 / 15.1     24.1 / 91.3
              d_rel               1.95 / 25.3     1.40 / 9.75     1.79 / 10.2     4.18 / 21.0
D H=72  tail  d_ent shuffled      2.84 / 16.1     3.83 / 15.3     3.92 / 15.7     10.9 / 43.5
              d_ent sorted        2.63 / 19.4     3.06 / 14.2     4.01 / 14.2     10.9 / 43.5
              d_rel               2.64 / 35.2     1.32 / 9.16     2.42 / 10.8     8.71 / 24.3
        head  d_ent shuffled      3.36 / 22.3     3.83 / 16.7     4.13 / 13.0     25.2 / 112
              d_ent sorted        3.41 / 17.4     3.06 / 16.7     3.79 / 15.7     25.2 / 109
              d_rel               2.31 / 33.4     1.32 / 7.85     1.79 / 11.0     11.0 / 41.5
D H=35  tail  d_ent shuffled      2.20 / 13.9     3.56 / 14.2     3.05 / 11.5     12.4 / 152
              d_ent sorted        2.34 / 13.5     3.15 / 10.7     3.61 / 12.1     12.4 / 152
              d_rel               2.70 / 33.7     1.38 / 6.98     1.90 / 8.80     4.05 / 16.2
        head  d_ent shuffled      2.23 / 25.8     3.56 / 14.2     3.43 / 14.9     160 / 643
              d_ent sorted        2.14 / 26.8     3.15 / 10.3     5.42 / 19.6     160 / 642
              d_rel               2.38 / 18.4     1.38 / 6.98     2.08 / 9.28     14.0 / 56.7
case E  tail  d_ent               2.85 / 18.1     2.20 / 10.8     3.17 / 11.7     3.46 / 14.8
              d_rel               4.38 / 84.4     2.66 / 89.2     2.76 / 114      0.34 / 4.82
        head  d_ent               2.37 / 19.9     2.71 / 18.6     2.97 / 16.8     2.19 / 14.3
              d_rel               1.87 / 99.2     2.26 / 73.5     2.30 / 52.9     0.29 / 6.41
(RotatE at H = 35, head side: the short (a, b) of case C's note; torch's fp32 run reaches 161 on the same inputs.)
No figure of the cases D and E is above 0.39 of its bound (RotatE, case D at H = 8, head side, d_rel: 3.22 / 8.46).
"""
import functools

import pytest
import torch

import gripnet_amd
import kge_batch_cases as kb
import kge_cases as kc
from gripnet_amd import _hip

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _sliced(t, left, width, dev, fill=NAN):
    """`t` as the column view big[:, left:left + cols] of a wider matrix of `fill`."""
    rows, cols = t.shape
    assert width >= left + cols
    big = torch.full((rows, width), fill, dtype=t.dtype, device=dev)
    big[:, left:left + cols] = t.to(dev)
    return big, big[:, left:left + cols]


def _beside_is(big, left, cols, fill=NAN):
    beside = torch.cat([big[:, :left], big[:, left + cols:]], dim=1)
    return bool(torch.isnan(beside).all()) if fill != fill else bool((beside == fill).all())


def _divisor(c):
    return kc.embedding_range(c.gamma, c.H) / kc.PI


def _operands(c, dev, ent, rel, positive, et, negatives):
    ent = c.ent.to(dev) if ent is None else ent
    rel = c.rel.to(dev) if rel is None else rel
    fixed = kb.fixed_of(c.positive if positive is None else positive, c.side).to(dev)
    et = (c.et if et is None else et).to(dev)
    negatives = c.negatives.to(dev) if negatives is None else negatives
    return ent, rel, fixed, et, negatives


def _forward(c, dev, log_sigmoid, ent=None, rel=None, positive=None, et=None, negatives=None):
    """(out, raw) of the batch kernel, both prefilled with a sentinel."""
    ent, rel, fixed, et, negatives = _operands(c, dev, ent, rel, positive, et, negatives)
    shape = tuple(negatives.shape)
    out, raw = torch.full(shape, 7.0, device=dev), torch.full(shape, 7.0, device=dev)
    _hip.kge_batch_forward(c.model, ent, rel, fixed, et, negatives, c.side, c.gamma, _divisor(c), log_sigmoid, out,
                           raw if log_sigmoid else None)
    return out, raw


def _list_forward(c, dev, log_sigmoid):
    """The same scores from the list kernel on the expansion, prefilled with another sentinel, as [B, K]."""
    out, raw = torch.full((c.E,), -3.0, device=dev), torch.full((c.E,), -3.0, device=dev)
    _hip.kge_forward(c.model, c.ent.to(dev), c.rel.to(dev), c.sample.to(dev), c.et_list.to(dev), c.gamma, _divisor(c), log_sigmoid,
                     out, raw if log_sigmoid else None)
    return out.view(c.B, c.K), raw.view(c.B, c.K)


def _backward(c, dev, upstream, log_sigmoid=True, ent=None, rel=None, positive=None, et=None, negatives=None, types_sorted=None,
              d_ent=None, d_rel=None):
    raw = None
    if log_sigmoid:
        _, raw = _forward(c, dev, True, ent, rel, positive, et, negatives)
    ent, rel, fixed, et, negatives = _operands(c, dev, ent, rel, positive, et, negatives)
    d_ent = torch.full(tuple(ent.shape), NAN, device=dev) if d_ent is None else d_ent
    d_rel = torch.full(tuple(rel.shape), NAN, device=dev) if d_rel is None else d_rel
    _hip.kge_batch_backward(c.model, ent, rel, fixed, et, negatives, c.side, _divisor(c), upstream.to(dev), raw, d_ent, d_rel,
                            types_sorted=types_sorted)
    return d_ent, d_rel


def _upstream(c):
    return torch.linspace(-1.0, 1.0, c.B * c.K).view(c.B, c.K)


_CASES = {"A": kb.case_a, "B": kb.case_b, "C": kb.case_c}


def _busiest(ids):
    return int(torch.bincount(ids, minlength=1).max())


def _gradient_bounds(c, sample, et_list, up_list, log_sigmoid):
    """float64 gradients of the list (sample, et_list) under the upstream `up_list`, their scales, torch's fp32 figures and
    the constants c_g (d_ent, d_rel).  The depths are those of the case's own block (its busiest rows)."""
    m = c.model
    args = (c.ent, c.rel, sample, et_list, c.gamma)
    g64 = kc.reference_gradients(m, *args, up_list, torch.float64, log_sigmoid=log_sigmoid)
    scale = kc.abs_contributions(m, *args, up_list, log_sigmoid=log_sigmoid)
    g32 = kc.reference_gradients(m, *args, up_list, torch.float32, log_sigmoid=log_sigmoid)
    t_g = [kc.figure(a, b, s, strict=False) for a, b, s in zip(g32, g64, scale)]
    kappa_g, kappa_s = kc.condition_gradients(m, *args), kc.condition_scores(m, *args)
    scale_s = float(kc.abs_term_sum(m, *args).max())
    depth = max(kc.fold_depth(c.H, True), kc.fold_depth(c.H, False))
    lanes = kb.reduce_lanes(c.H)
    fixed = kb.fixed_of(c.positive, c.side)
    r_ent = kc.reduction_depth(_busiest(c.negatives.reshape(-1)), lanes) + kb.query_reduction_depth(c.K, _busiest(fixed), lanes) + 1
    r_rel = kb.query_reduction_depth(c.K, _busiest(c.et), lanes)
    derived = [(kc.CONTRIBUTION_ROUNDINGS[m] + r) * kappa_g + (kc.TERM_ROUNDINGS[m] + depth) * kappa_s * scale_s for r in (r_ent, r_rel)]
    return {"g64": g64, "scale": scale, "t_g": t_g, "derived": derived, "c_g": [min(d, 4 * t) for d, t in zip(derived, t_g)]}


@functools.lru_cache(maxsize=None)
def _reference(name, model, side, log_sigmoid=True):
    """A case and what its gradients are held to, computed once on the CPU and left unchanged."""
    c = _CASES[name](model, side)
    r = _gradient_bounds(c, c.sample, c.et_list, _upstream(c).reshape(-1), log_sigmoid)
    r["case"], r["up"] = c, _upstream(c)
    return r


def _check_gradients(r, got, what):
    for g, ref, scale, c_g, t_g, d, name in zip(got, r["g64"], r["scale"], r["c_g"], r["t_g"], r["derived"], ("d_ent", "d_rel")):
        assert bool(torch.isfinite(g).all()), (what, name)
        fig = kc.figure(g, ref, scale)
        print("{}: {} {:.2f} (bound {:.2f}: derived {:.1f}, torch fp32 {:.2f})".format(what, name, fig, c_g, d, t_g))
        assert fig <= c_g, (what, name, fig, c_g)


# ---- forward: the list kernel's bits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("H", kc.SHAPE_H)
@pytest.mark.parametrize("model", kc.MODELS)
def test_forward_bits_of_the_list_kernel(gpu, model, H, side):
    """Raw scores and log-sigmoid values equal _hip.kge_forward on the expansion bit for bit, at every (B, K) of
    kge_batch_cases.SHAPE_BK; the outputs are prefilled with different sentinels, so an element that equals the list's
    was written."""
    for B, K in kb.SHAPE_BK:
        c = kb.shape_case(model, H, B, K, side)
        what = "{} {} H={} B={} K={}".format(model, side, H, B, K)
        plain, _ = _forward(c, gpu, False)
        y, raw = _forward(c, gpu, True)
        want_plain, _ = _list_forward(c, gpu, False)
        want_y, want_raw = _list_forward(c, gpu, True)
        assert plain.shape == (B, K) and y.shape == (B, K)
        assert torch.equal(plain, want_plain), what
        assert torch.equal(raw, want_raw) and torch.equal(raw, plain), what
        assert torch.equal(y, want_y), what
        assert not bool(torch.isnan(plain).any()), what
    _hip.raise_if_index_errors(gpu)


# ---- strided operands --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_strided_operands(gpu, model, side):
    """Tables and gradients as column views of wider NaN matrices (ld = D + 4 on the vector path at H = 32, D + 1 on the
    scalar path at H = 3), the candidates as a column slice of a wider int64 matrix of ids outside the table: the same bits
    as from contiguous operands, nothing beside the views read into a result or written.  And D + 4 at H = 72 on the
    shuffled case D (kge_batch_cases.case_d): two column blocks, rows that go through the chunk partials and the combine,
    which writes d_rel and adds onto d_ent at the views' leading dimensions."""
    for H, pad in ((32, 4), (3, 1), (72, 4)):
        c = kb.case_d(model, side, H, True) if H == 72 else kb.random_case(model, side, 60, 7, H, 5, 70, seed=20 + H)
        de, dr = kc.dims(model, H)
        up = c.up if H == 72 else _upstream(c)
        y0, raw0 = _forward(c, gpu, True)
        g0 = _backward(c, gpu, up)
        big_e, ent = _sliced(c.ent, pad, de + pad, gpu)
        big_r, rel = _sliced(c.rel, 0, dr + pad, gpu)
        big_n, negatives = _sliced(c.negatives, 2, c.K + 5, gpu, fill=-7)
        big_de, d_ent = _sliced(torch.full((c.n, de), NAN), 0, de + pad, gpu)
        big_dr, d_rel = _sliced(torch.full((c.R, dr), NAN), pad, dr + pad, gpu)
        assert not negatives.is_contiguous()
        y, raw = _forward(c, gpu, True, ent=ent, rel=rel, negatives=negatives)
        got = _backward(c, gpu, up, ent=ent, rel=rel, negatives=negatives, d_ent=d_ent, d_rel=d_rel)
        what = "{} {} H={}".format(model, side, H)
        assert torch.equal(y, y0) and torch.equal(raw, raw0), what
        assert torch.equal(got[0], g0[0]) and torch.equal(got[1], g0[1]), what
        assert _beside_is(big_e, pad, de) and _beside_is(big_r, 0, dr) and _beside_is(big_n, 2, c.K, fill=-7), what
        assert _beside_is(big_de, 0, de) and _beside_is(big_dr, pad, dr), what + ": written beside the gradients"
        assert torch.equal(negatives.cpu(), c.negatives), what
    _hip.raise_if_index_errors(gpu)


# ---- gradients against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("model", kc.MODELS)
def test_gradients_against_float64(gpu, model, name, side):
    """A: the reduction's edge cases (kge_batch_cases.case_a); B: the vector path, several items per positive; C: the scalar
    path.  The upstream is linspace(-1, 1, B * K); the forward returned the log-sigmoid."""
    r = _reference(name, model, side)
    c = r["case"]
    what = "{} {} case {}".format(model, side, name)
    got = [g.cpu() for g in _backward(c, gpu, r["up"])]
    _check_gradients(r, got, what)
    unsorted_route = [g.cpu() for g in _backward(c, gpu, r["up"], types_sorted=False)]
    _check_gradients(r, unsorted_route, what + " (sort route)")
    assert torch.equal(unsorted_route[0], got[0])               # (the entity passes do not depend on the flag)
    if name == "A":
        assert float(got[0][c.unused_entity].abs().max()) == 0.0
        assert float(got[1][list(c.empty_relations)].abs().max()) == 0.0
    _hip.raise_if_index_errors(gpu)


# ---- rows across the chunks of the passes over the positives ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_d(model, side, H, shuffled):
    """Case D in one of its two orders and what its gradients are held to (the upstream is the case's own)."""
    c = kb.case_d(model, side, H, shuffled)
    r = _gradient_bounds(c, c.sample, c.et_list, c.up.reshape(-1), True)
    r["case"], r["up"] = c, c.up
    return r


@functools.lru_cache(maxsize=None)
def _reference_e(model, side):
    c = kb.case_e(model, side)
    r = _gradient_bounds(c, c.sample, c.et_list, _upstream(c).reshape(-1), True)
    r["case"], r["up"] = c, _upstream(c)
    return r


def _check_exact_zeros(c, got, what):
    assert float(got[0][c.unused_entity].abs().max()) == 0.0, what
    assert float(got[1][list(c.empty_relations)].abs().max()) == 0.0, what


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("H", kb.D_HIDDEN)
@pytest.mark.parametrize("model", kc.MODELS)
def test_rows_across_chunks_against_float64(gpu, model, H, side):
    """kge_batch_cases.case_d: rows of the relation pass and of the accumulating entity pass that lie in two, three and
    parts of two chunks of 32 records, at every column-block shape (kge_batch_cases.D_HIDDEN).  The shuffled block goes
    through the sort route (what training runs), the stably sorted one through the ordered and through the sort route.
    d_ent and d_rel are prefilled with NaN; the rows of the empty relations and of the unused entity are exact zeros."""
    what = "{} {} case D H={}".format(model, side, H)
    r = _reference_d(model, side, H, True)
    got = [g.cpu() for g in _backward(r["case"], gpu, r["up"], types_sorted=False)]
    _check_gradients(r, got, what + " shuffled (sort route)")
    _check_exact_zeros(r["case"], got, what)
    r = _reference_d(model, side, H, False)
    for types_sorted in (True, False):
        got = [g.cpu() for g in _backward(r["case"], gpu, r["up"], types_sorted=types_sorted)]
        _check_gradients(r, got, what + " sorted ({} route)".format("ordered" if types_sorted else "sort"))
        _check_exact_zeros(r["case"], got, what)
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_the_sort_route_sorts(gpu, model, side):
    """d_rel of the shuffled case D by the sort route is, bit for bit, d_rel of the stably sorted block by the ordered route:
    a positive's partial row does not depend on its place in the batch, a stable sort keeps the batch order inside a
    relation, and the chunks are cut by sorted position - so both add the same rows in the same order.  No reference and
    no tolerance.  (d_ent is not compared: the candidate pass orders a candidate's records by batch position, which the
    shuffle changes; test_rows_across_chunks_against_float64 holds it to its bound.)"""
    for H in kb.D_HIDDEN:
        s, o = kb.case_d(model, side, H, True), kb.case_d(model, side, H, False)
        assert not bool((s.et[1:] >= s.et[:-1]).all()) and bool((o.et[1:] >= o.et[:-1]).all())
        _, shuffled = _backward(s, gpu, s.up, types_sorted=False)
        _, ordered = _backward(o, gpu, o.up, types_sorted=True)
        assert bool(torch.isfinite(ordered).all()) and float(ordered.abs().max()) > 0.0
        assert torch.equal(shuffled, ordered), "{} {} H={}".format(model, side, H)
        looked_up = _backward(s, gpu, s.up)[1]                    # (the route the module takes: the order is looked up)
        assert torch.equal(looked_up, ordered)
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_forward_bits_on_the_gradient_blocks(gpu, model, side):
    """The scores of case D (H = 72: rows wider than a lane group holds; H = 35: the scalar path), shuffled and sorted, and of
    case E (16 385 positives of two candidates) are the list kernel's on the expansion, bit for bit."""
    cases = [kb.case_d(model, side, H, shuffled) for H in (72, 35) for shuffled in (True, False)] + [kb.case_e(model, side)]
    for c in cases:
        what = "{} {} H={} B={}".format(model, side, c.H, c.B)
        plain, _ = _forward(c, gpu, False)
        y, raw = _forward(c, gpu, True)
        want_plain, _ = _list_forward(c, gpu, False)
        want_y, want_raw = _list_forward(c, gpu, True)
        assert torch.equal(plain, want_plain), what
        assert torch.equal(raw, want_raw) and torch.equal(raw, plain), what
        assert torch.equal(y, want_y), what
        assert not bool(torch.isnan(plain).any()), what
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_more_positives_than_one_grid_against_float64(gpu, model, side):
    """kge_batch_cases.case_e: the query kernel's workgroups take a second positive (B = 16 385 over a grid of 16 384), every
    relation's row is the combine's sum over some 58 chunks, and with K = 2 the chunks of the passes over the positives size
    the workspace's partials."""
    r = _reference_e(model, side)
    c = r["case"]
    what = "{} {} case E".format(model, side)
    got = [g.cpu() for g in _backward(c, gpu, r["up"])]
    _check_gradients(r, got, what)
    unsorted_route = [g.cpu() for g in _backward(c, gpu, r["up"], types_sorted=False)]
    _check_gradients(r, unsorted_route, what + " (sort route)")
    assert torch.equal(unsorted_route[0], got[0]) and torch.equal(unsorted_route[1], got[1])
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_empty_blocks_give_zero_gradients(gpu, model, side):
    for B, K in ((0, 5), (3, 0)):
        c = kb.shape_case(model, 4, B, K, side)
        d_ent, d_rel = _backward(c, gpu, torch.ones(B, K))
        assert float(d_ent.abs().sum()) == 0.0 and float(d_rel.abs().sum()) == 0.0


# ---- through the module --------------------------------------------------------------------------------------------------
def _module(c, dev):
    model = gripnet_amd.KGEModel(c.model, c.n, c.R, c.H, c.gamma)
    with torch.no_grad():
        model.entity_embedding.copy_(c.ent)
        model.relation_embedding.copy_(c.rel)
    return model.to(dev)


def _grads(model):
    got = model.entity_embedding.grad.clone(), model.relation_embedding.grad.clone()
    model.zero_grad(set_to_none=True)
    return got


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_through_the_module(gpu, model, side):
    """KGEModel.score and KGEModel.forward in the batch modes on case A: values are the kernel's, gradients are held to the
    float64 reference at the same bounds; a loss of a `single` positive score and a batch negative score of the same tables
    gets the sum of the two separate gradients bit for bit."""
    mode = kb.MODES[side]
    for log_sigmoid in (False, True):
        r = _reference("A", model, side) if log_sigmoid else _reference("A", model, side, False)
        c = r["case"]
        m = _module(c, gpu)
        positive, negatives, et, up = c.positive.to(gpu), c.negatives.to(gpu), c.et.to(gpu), r["up"].to(gpu)
        out = (m if log_sigmoid else m.score)((positive, negatives), et, mode=mode)
        assert out.shape == (c.B, c.K) and out.requires_grad
        assert torch.equal(out.detach(), _forward(c, gpu, log_sigmoid)[0])
        with torch.no_grad():
            assert torch.equal((m if log_sigmoid else m.score)((positive, negatives), et, mode=mode), out.detach())
        (out * up).sum().backward()
        batch = _grads(m)
        _check_gradients(r, [g.cpu() for g in batch], "{} {} module {}".format(model, side, "forward" if log_sigmoid else "score"))
    # `single` and batch scores in one loss
    up_pos = torch.linspace(0.5, 1.5, c.B, device=gpu)
    (m.score(positive, et) * up_pos).sum().backward()
    single = _grads(m)
    ((m.score(positive, et) * up_pos).sum() + (m((positive, negatives), et, mode=mode) * up).sum()).backward()
    both = _grads(m)
    assert torch.equal(both[0], single[0] + batch[0]) and torch.equal(both[1], single[1] + batch[1])
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_a_shuffled_batch_through_the_module(gpu, model, side):
    """KGEModel.forward on the shuffled case D at H = 72 and .backward(): the route of a training step - the relation pass
    sorts - through autograd, held to the float64 reference at the bounds of the direct call."""
    r = _reference_d(model, side, 72, True)
    c = r["case"]
    m = _module(c, gpu)
    out = m((c.positive.to(gpu), c.negatives.to(gpu)), c.et.to(gpu), mode=kb.MODES[side])
    assert out.shape == (c.B, c.K) and torch.equal(out.detach(), _forward(c, gpu, True)[0])
    (out * r["up"].to(gpu)).sum().backward()
    got = [g.cpu() for g in _grads(m)]
    _check_gradients(r, got, "{} {} case D H=72 shuffled, module".format(model, side))
    _check_exact_zeros(c, got, "module")
    _hip.raise_if_index_errors(gpu)


# ---- ids ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_ids_outside_the_tables(gpu, model, side):
    """A negative and a too large id in `fixed`, in `et` and in `negatives` (kge_batch_cases.with_bad_ids): a bad fixed entity
    or relation makes its whole row NaN, a bad candidate its element; every other score keeps its bits; the flag is set and
    raise_if_index_errors raises IndexError; the gradients are finite and those of the expansion without the bad entries,
    at the case's bounds."""
    r = _reference("A", model, side)
    c = r["case"]
    positive, et, negatives, bad_rows, bad_elements = kb.with_bad_ids(c)
    bad = torch.zeros(c.B, c.K, dtype=torch.bool)
    bad[bad_rows] = True
    for b, k in bad_elements:
        bad[b, k] = True
    _hip.raise_if_index_errors(gpu)
    clean_y, clean_raw = _forward(c, gpu, True)
    y, raw = _forward(c, gpu, True, positive=positive, et=et, negatives=negatives.to(gpu))
    with pytest.raises(IndexError):
        _hip.raise_if_index_errors(gpu)
    _hip.raise_if_index_errors(gpu)                             # (the flag is cleared by the check)
    y, raw = y.cpu(), raw.cpu()
    assert bool(torch.isnan(y[bad]).all()) and bool(torch.isnan(raw[bad]).all())
    assert torch.equal(y[~bad], clean_y.cpu()[~bad]) and torch.equal(raw[~bad], clean_raw.cpu()[~bad])
    up = r["up"].clone()
    up[bad] = 3.0
    got = [g.cpu() for g in _backward(c, gpu, up, positive=positive, et=et, negatives=negatives.to(gpu))]
    with pytest.raises(IndexError):                             # (the backward's own forward saw them again)
        _hip.raise_if_index_errors(gpu)
    good = ~bad.reshape(-1)
    kept = _gradient_bounds(c, c.sample[:, good], c.et_list[good], r["up"].reshape(-1)[good], True)
    _check_gradients(kept, got, "{} {} bad ids".format(model, side))
    assert float(got[0][c.unused_entity].abs().max()) == 0.0


# ---- repeatability and capture -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_same_bits_in_every_call_and_under_capture(gpu, model, side):
    """Two calls of forward and backward give identical bits; one forward + backward captured with torch.cuda.graph and
    replayed gives the eager bits (no host synchronisation inside: the capture would fail)."""
    c = kb.case_b(model, side)
    ent, rel, fixed, et, negatives = _operands(c, gpu, None, None, None, None, None)
    up = _upstream(c).to(gpu)

    def step():
        y, raw = torch.empty(c.B, c.K, device=gpu), torch.empty(c.B, c.K, device=gpu)
        d_ent, d_rel = torch.empty_like(ent), torch.empty_like(rel)
        _hip.kge_batch_forward(c.model, ent, rel, fixed, et, negatives, side, c.gamma, _divisor(c), True, y, raw)
        _hip.kge_batch_backward(c.model, ent, rel, fixed, et, negatives, side, _divisor(c), up, raw, d_ent, d_rel, types_sorted=True)
        return y, raw, d_ent, d_rel

    eager = [t.clone() for t in step()]
    again = step()
    for a, b in zip(eager, again):
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
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_a_shuffled_batch_under_capture(gpu, model, side):
    """The same on the shuffled case D at H = 72, where the relation pass sorts (rocPRIM inside the capture), rows go through
    the chunk partials and every pass takes a second column block: a replay that kept a partial of the previous launch, or
    ran a column block ahead of its combine, would not give the eager bits.  The outputs are refilled with NaN between the
    replays."""
    c = kb.case_d(model, side, 72, True)
    ent, rel, fixed, et, negatives = _operands(c, gpu, None, None, None, None, None)
    up = c.up.to(gpu)
    y, raw = torch.empty(c.B, c.K, device=gpu), torch.empty(c.B, c.K, device=gpu)
    d_ent, d_rel = torch.empty_like(ent), torch.empty_like(rel)
    outputs = (y, raw, d_ent, d_rel)

    def step():
        _hip.kge_batch_forward(c.model, ent, rel, fixed, et, negatives, side, c.gamma, _divisor(c), True, y, raw)
        _hip.kge_batch_backward(c.model, ent, rel, fixed, et, negatives, side, _divisor(c), up, raw, d_ent, d_rel, types_sorted=False)

    step()
    eager = [t.clone() for t in outputs]
    assert all(bool(torch.isfinite(t).all()) for t in eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        for t in outputs:
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outputs):
            assert torch.equal(a, b)
    _hip.raise_if_index_errors(gpu)
