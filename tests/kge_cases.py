"""The KGE baselines (KGEModel, baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:127-235) as a torch formulation
that runs in float64 and in fp32, the cases of tests/test_kge_host.py and tests/test_gpu_kge.py, and their error
measures.  Not a test module.

The formulation is written from the models' definitions; it gathers the three rows, evaluates the terms and applies
logsigmoid in the order the reference does, so in float64 it is what the reference class gives after ``.double()`` (tests/test_kge_host.py holds it to
tests/golden/kge_cases.npz), so the GPU tests' float64 reference is pinned to the reference itself."""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

MODELS = ("TransE", "DistMult", "ComplEx", "RotatE")
EPS = 1e-13                                                       # gripnet/utils.py:10
PI = 3.14159265358979323846                                       # :214
U = 2.0 ** -24                                                    # unit roundoff of fp32
CHUNK = 2048                                                      # records per workgroup of the backward's reduction (csrc/seg_reduce.cuh: kSegChunkRecs)


def dims(model, H):
    """(entity row length, relation row length)."""
    return (2 * H if model in ("ComplEx", "RotatE") else H), (2 * H if model == "ComplEx" else H)


def embedding_range(gamma, H):
    """The fp32 value the reference keeps in its `embedding_range` parameter (:78-81), as a host float."""
    return float(np.float32((float(np.float32(gamma)) + 2.0) / H))


def rows(ent, rel, sample, et):
    return ent.index_select(0, sample[0]), rel.index_select(0, et), ent.index_select(0, sample[1])


def _halves(x):
    """(real part, imaginary part) of rows that hold them side by side."""
    H = x.shape[-1] // 2
    return x[..., :H], x[..., H:]


def _complex_product(xr, xi, yr, yi):
    return xr * yr - xi * yi, xr * yi + xi * yr


def column_terms(model, head, relation, tail, gamma, H):
    """The terms over the last dimension whose sum (DistMult, ComplEx) or whose sum taken from gamma (TransE, RotatE) is
    the score, written from the models' definitions:
      TransE |h + r - t|;  DistMult h r t;  ComplEx Re((h r) conj(t));  RotatE |h e^(i theta) - t|, theta = r / (range / pi)."""
    if model == "TransE":
        return torch.abs(head + relation - tail)
    if model == "DistMult":
        return head * relation * tail
    (hr, hi), (tr, ti) = _halves(head), _halves(tail)
    if model == "ComplEx":
        pr, pi = _complex_product(hr, hi, *_halves(relation))
        return pr * tr + pi * ti
    theta = relation / (embedding_range(gamma, H) / PI)
    pr, pi = _complex_product(hr, hi, torch.cos(theta), torch.sin(theta))
    return torch.linalg.vector_norm(torch.stack((pr - tr, pi - ti)), dim=0)


def raw_score(model, ent, rel, sample, et, gamma):
    """The scores [E].  The gathered rows are kept as [E, 1, D] and reduced over the last dimension, the shapes the
    reference computes on: torch's CPU reductions pick their summation tree by shape, and with these the fp32 run gives the
    reference's bits (tests/test_kge_host.py)."""
    H = rel.shape[1] // 2 if model == "ComplEx" else rel.shape[1]
    head, relation, tail = [x.unsqueeze(1) for x in rows(ent, rel, sample, et)]
    if model == "TransE":                                     # the 1-norm kernel: another summation tree than abs().sum() in fp32
        total = torch.linalg.vector_norm(head + relation - tail, ord=1, dim=-1).squeeze(1)
    else:
        total = column_terms(model, head, relation, tail, gamma, H).sum(dim=-1).squeeze(1)
    return float(np.float32(gamma)) - total if model in ("TransE", "RotatE") else total


def log_sigmoid_score(model, ent, rel, sample, et, gamma):
    return F.logsigmoid(raw_score(model, ent, rel, sample, et, gamma))


def loss_expr(pos, neg):
    return -(pos + EPS).mean() + -(1 - neg + EPS).mean()          # :266-268


def abs_term_sum(model, ent, rel, sample, et, gamma):
    """sum_k |term_k| in float64 (gamma counts as a term for TransE and RotatE): the scale of a score's rounding error."""
    H = rel.shape[1] // 2 if model == "ComplEx" else rel.shape[1]
    s = column_terms(model, *rows(ent.double(), rel.double(), sample, et), gamma, H).abs().sum(dim=1)
    return s + abs(float(gamma)) if model in ("TransE", "RotatE") else s


def reference_gradients(model, ent, rel, sample, et, gamma, upstream, dtype, log_sigmoid=True):
    """(d ent, d rel) of ``sum(upstream * f(scores))`` through torch autograd in `dtype` (f: logsigmoid or identity)."""
    e = ent.to(dtype).clone().requires_grad_(True)
    r = rel.to(dtype).clone().requires_grad_(True)
    y = (log_sigmoid_score if log_sigmoid else raw_score)(model, e, r, sample, et, gamma)
    (y * upstream.to(dtype)).sum().backward()
    return e.grad, r.grad


def abs_contributions(model, ent, rel, sample, et, gamma, upstream, log_sigmoid=True):
    """Per output element of (d ent, d rel): the sum over the row's records of |contribution|, in float64 - the scale of a
    gradient element's rounding error.  A record's contribution to a row is g_e * ds_e / d row; autograd on the GATHERED
    rows (a leaf per triple and role) gives them one by one, and their absolute values are scattered to the rows."""
    ent64, rel64 = ent.double(), rel.double()
    H = rel.shape[1] // 2 if model == "ComplEx" else rel.shape[1]
    h, r, t = [x.clone().requires_grad_(True) for x in rows(ent64, rel64, sample, et)]
    total = column_terms(model, h, r, t, gamma, H).sum(dim=1)
    s = float(np.float32(gamma)) - total if model in ("TransE", "RotatE") else total
    y = F.logsigmoid(s) if log_sigmoid else s
    (y * upstream.double()).sum().backward()
    a_ent = torch.zeros_like(ent64).index_add_(0, sample[0], h.grad.abs()).index_add_(0, sample[1], t.grad.abs())
    a_rel = torch.zeros_like(rel64).index_add_(0, et, r.grad.abs())
    return a_ent, a_rel


def figure(got, ref64, scale64, strict=True):
    """max |got - ref| / (u * scale) over the elements with a non-zero scale; with `strict`, elements of zero scale must
    match exactly.  (Not strict: for torch's own fp32 run, which leaves a residue where a derivative cancels to an exact
    zero in float64 - ComplEx's d s / d ri = hr ti - hi tr at head == tail; the kernels are held to the zero.)"""
    got, ref64 = got.detach().cpu().double(), ref64.detach().cpu().double()
    err = (got - ref64).abs()
    zero = scale64 == 0
    assert not strict or bool((err[zero] == 0).all()), "an element without any contribution is not exactly its reference"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (U * scale64[~zero])).max())


# ---- cases -------------------------------------------------------------------------------------------------------------
GRID = 2.0 ** -16


def tables(model, n, R, H, gamma, gen):
    """Uniform in +-embedding_range like the reference's initialisation, on a grid of 2^-16: h + r - t is then exact in
    fp32 and in float64, so TransE's sign(h + r - t) - a gradient of +-g - is the same in both (a rounding that moves a
    difference across zero is a whole contribution, not a rounding error; products and the other models round as ever)."""
    de, dr = dims(model, H)
    rho = embedding_range(gamma, H)
    ent = torch.round((torch.rand(n, de, generator=gen) * 2 - 1) * rho / GRID) * GRID
    rel = torch.round((torch.rand(R, dr, generator=gen) * 2 - 1) * rho / GRID) * GRID
    return ent, rel


def case(model, n, R, H, E, gamma=12.0, seed=0, sort=True):
    """Random tables in +-embedding_range and E random triples with a sorted edge_type."""
    gen = torch.Generator().manual_seed(seed)
    ent, rel = tables(model, n, R, H, gamma, gen)
    sample = torch.randint(0, n, (2, E), generator=gen)
    et = torch.randint(0, R, (E,), generator=gen)
    if sort:
        et = et.sort().values
    return SimpleNamespace(model=model, n=n, R=R, H=H, E=E, gamma=gamma, ent=ent, rel=rel, sample=sample, et=et)


SHAPE_H = (1, 3, 4, 32, 36, 72)
SHAPE_E = (0, 1, 63, 64, 65, 257)


def shape_case(model, H, E):
    """The first E triples of ONE list of 257 on one pair of tables per (model, H) (n = 50, R = 4).  H: the scalar path (1, 3),
    one vector piece (4), the driver's size (32), more units than a lane group's first trip covers evenly (36: 9 units on 16
    lanes; 36 columns on the scalar path: three trips), and a second trip and a second column block of the vector path (72:
    18 units).  gamma = 1: the tables' range (gamma + 2) / H stays small at H = 1 and with it |s| - at gamma = 12 a DistMult
    score of H = 1 reaches 14^3, where sigma(-s) is below fp32's range and nothing is left to compare."""
    c = case(model, 50, 4, H, SHAPE_E[-1], gamma=1.0, seed=100 + 7 * H)
    c.sample, c.et, c.E = c.sample[:, :E].contiguous(), c.et[:E].contiguous(), E
    return c


def gradient_case(model, seed=5):
    """The reduction's edge cases in one list (n = 60, R = 7, H = 8, E = 13 000):
      * entities 0, 1, 2 with CHUNK - 1, CHUNK, CHUNK + 1 records, entity 3 a hub of 5 000 (more than two chunks) - each of
        them so often as head AND so often as tail (the tails are the heads rotated);
      * entity 59 in no triple, relations 0 and 6 without triples: exact zeros;
      * head == tail triples (the hub's rotation overlaps itself; entity 4 under relation 3);
      * column 2 of relation 3 is zero: with head == tail that is TransE's h + r - t = 0 and RotatE's a = b = 0."""
    gen = torch.Generator().manual_seed(seed)
    n, R, H, gamma = 60, 7, 8, 12.0
    ent, rel = tables(model, n, R, H, gamma, gen)
    rel[3, 2] = 0.0
    counts = [CHUNK - 1, CHUNK, CHUNK + 1, 5000]
    heads = torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in enumerate(counts)])
    tails = torch.roll(heads, 3000)
    extra = 13000 - heads.numel() - 40
    xh = torch.randint(4, n - 1, (extra,), generator=gen)
    xt = torch.randint(4, n - 1, (extra,), generator=gen)
    same = torch.full((40,), 4, dtype=torch.long)
    sample = torch.stack([torch.cat([heads, xh, same]), torch.cat([tails, xt, same])])
    et = torch.cat([torch.randint(1, R - 1, (heads.numel() + extra,), generator=gen), torch.full((40,), 3, dtype=torch.long)])
    order = torch.randperm(sample.shape[1], generator=gen)
    sample, et = sample[:, order], et[order]
    order = et.sort(stable=True).indices
    sample, et = sample[:, order].contiguous(), et[order].contiguous()
    return SimpleNamespace(model=model, n=n, R=R, H=H, E=sample.shape[1], gamma=gamma, ent=ent, rel=rel, sample=sample, et=et,
                           counts=counts, unused_entity=n - 1, empty_relations=(0, R - 1), zero_relation=3, zero_column=2,
                           same_entity=4)


def saturated_case(model, seed=9):
    """Scores of about +-80: relation 1's rows scaled (TransE: a distance of ~90; DistMult, ComplEx: products of both signs);
    RotatE's relation is a phase only, so there the rows of entities 0..4 are scaled instead.  TransE and RotatE cannot
    exceed gamma: they saturate on the negative side only."""
    c = case(model, 30, 3, 8, 600, seed=seed)
    rho = embedding_range(c.gamma, c.H)
    if model == "TransE":
        c.rel[1] = torch.where(c.rel[1] >= 0, 1.0, -1.0) * (92.0 / c.H)
    elif model == "RotatE":
        c.ent[:5] *= 92.0 / (c.H * rho * 0.77)                    # (0.77 A: the mean modulus of a complex number uniform in +-A)
    else:
        s64 = raw_score(model, c.ent.double(), c.rel.double(), c.sample, c.et, c.gamma)
        peak = float(s64[c.et == 1].abs().max())
        c.rel[1] *= 80.0 / peak
    return c


def with_bad_ids(c, relations=True):
    """A copy of the case's list with bad triples inserted (a negative and a too large head, tail and - with `relations` -
    relation), and the positions of the good ones.  Without bad relations a sorted edge_type stays sorted."""
    bad = [(-1, 0, None), (c.n, 1, None), (0, -3, None), (1, c.n + 5, None)] + ([(2, 3, -1), (3, 2, c.R)] if relations else [])
    E = c.E + len(bad)
    at = torch.linspace(0, E - 1, len(bad)).long()
    good = torch.ones(E, dtype=torch.bool)
    good[at] = False
    sample = torch.zeros(2, E, dtype=torch.long)
    et = torch.zeros(E, dtype=torch.long)
    sample[:, good], et[good] = c.sample, c.et
    for p, (h, t, r) in zip(at.tolist(), bad):
        near = c.et[min(int(good[:p].sum()), c.E - 1)]             # the relation of the good triple behind it
        sample[0, p], sample[1, p], et[p] = h, t, (near if r is None else r)
    return sample, et, good


# ---- bounds ------------------------------------------------------------------------------------------------------------
# An fp32 evaluation's error is a number of roundings times u times the magnitude of the OPERANDS that were rounded; the tests
# state their bounds against sum |term| (scores) and sum |contribution| (gradients), which are smaller where a term or a
# derivative cancels inside (ComplEx's four products, TransE's h + r - t, RotatE's a / sqrt(a^2 + b^2) at a short (a, b)).
# `condition_*` is the largest ratio of the two scales over a case's elements: a count of roundings times it is a valid
# constant against the smaller scale.
def _parts(model, ent, rel, sample, et, gamma):
    H = rel.shape[1] // 2 if model == "ComplEx" else rel.shape[1]
    h, r, t = rows(ent.double(), rel.double(), sample, et)
    if model in ("TransE", "DistMult"):
        return H, h, None, r, None, t, None
    hr, hi = torch.chunk(h, 2, dim=1)
    tr, ti = torch.chunk(t, 2, dim=1)
    if model == "ComplEx":
        rr, ri = torch.chunk(r, 2, dim=1)
    else:
        phase = r / (embedding_range(gamma, H) / PI)
        rr, ri = torch.cos(phase), torch.sin(phase)
    return H, hr, hi, rr, ri, tr, ti


def condition_scores(model, ent, rel, sample, et, gamma):
    """max over the triples of (sum_k operand magnitude of term k) / (sum_k |term_k|), gamma on both sides where it counts."""
    H, hr, hi, rr, ri, tr, ti = _parts(model, ent, rel, sample, et, gamma)
    extra = abs(float(gamma)) if model in ("TransE", "RotatE") else 0.0
    if model == "TransE":
        mag = hr.abs() + rr.abs() + tr.abs()
    elif model == "DistMult":
        return 1.0
    elif model == "ComplEx":
        mag = ((hr * rr).abs() + (hi * ri).abs()) * tr.abs() + ((hr * ri).abs() + (hi * rr).abs()) * ti.abs()
    else:
        a = (hr * rr).abs() + (hi * ri).abs() + tr.abs()
        b = (hr * ri).abs() + (hi * rr).abs() + ti.abs()
        mag = (a * a + b * b).sqrt()
    scale = abs_term_sum(model, ent, rel, sample, et, gamma)
    ok = scale > 0
    return float(((mag.sum(dim=1) + extra)[ok] / scale[ok]).max()) if bool(ok.any()) else 1.0


def condition_gradients(model, ent, rel, sample, et, gamma):
    """max over the records, roles and columns of (operand magnitude of ds / d row) / |ds / d row| (where that is not zero)."""
    if model in ("TransE", "DistMult"):
        return 1.0                                             # a sign; a single product
    H, hr, hi, rr, ri, tr, ti = _parts(model, ent, rel, sample, et, gamma)
    if model == "ComplEx":
        pairs = [(rr * tr, ri * ti), (rr * ti, ri * tr), (hr * rr, hi * ri), (hr * ri, hi * rr), (hr * tr, hi * ti), (hr * ti, hi * tr)]
        signs = [1, -1, -1, 1, 1, -1]
        worst = 1.0
        for (x, y), sg in zip(pairs, signs):
            d, mag = (x + sg * y).abs(), x.abs() + y.abs()
            ok = d > 0
            if bool(ok.any()):
                worst = max(worst, float((mag[ok] / d[ok]).max()))
        return worst
    a = (hr * rr - hi * ri) - tr
    b = (hr * ri + hi * rr) - ti
    m = (a * a + b * b).sqrt()
    mag = ((hr * rr).abs() + (hi * ri).abs() + tr.abs() + (hr * ri).abs() + (hi * rr).abs() + ti.abs())
    ok = m > 0
    amp = mag[ok] / m[ok]                                      # the unit vector (a, b) / m moves by (operands / m) roundings
    ua, ub = (a[ok] / m[ok]).abs(), (b[ok] / m[ok]).abs()
    c, s = rr[ok].abs(), ri[ok].abs()
    worst = 1.0
    for d, w in ((ua, amp), (ub, amp), ((a[ok] / m[ok] * rr[ok] + b[ok] / m[ok] * ri[ok]).abs(), amp * (c + s)),
                 ((a[ok] / m[ok] * ri[ok] - b[ok] / m[ok] * rr[ok]).abs(), amp * (c + s)),
                 ((a[ok] / m[ok] * (hr * ri + hi * rr)[ok] - b[ok] / m[ok] * (hr * rr - hi * ri)[ok]).abs(),
                  amp * (hr.abs() + hi.abs())[ok] * (c + s))):
        nz = d > 0
        if bool(nz.any()):
            worst = max(worst, float((w[nz] / d[nz]).max()))
    return worst


def fold_depth(H, vec):
    """Additions on the longest path of the forward's sum: a lane's serial sum over its columns, the cross-lane fold, and
    gamma (csrc/kge.hip: a lane group of min(16, 2^ceil(log2 units)) lanes, units = H / 4 on the vector path, H on the scalar)."""
    w = 4 if vec else 1
    units = max(H // w, 1)
    group = 1
    while group < 16 and group < units:
        group <<= 1
    return -(-units // group) * w + int(math.log2(group)) + 1


TERM_ROUNDINGS = {"TransE": 2, "DistMult": 2, "ComplEx": 7, "RotatE": 16}
"""Roundings per term.  TransE: h + r, - t.  DistMult: two products.  ComplEx: four products and two sums for (re, im), two
products and a sum with the tail.  RotatE: theta = r / divisor with the divisor itself rounded to fp32 (2, and each moves
cos and sin by up to |theta| <= pi roundings' worth: 2 pi), cosf and sinf (2 ulp each), (re, im) and the two differences
(8), two squares, their sum and the root (4): 16 rounded up."""

CONTRIBUTION_ROUNDINGS = {"TransE": 6, "DistMult": 7, "ComplEx": 9, "RotatE": 26}
"""Roundings per contribution g * ds/d row.  g = grad * 1 / (1 + exp(s)): the score's own error enters through exp (counted
by the caller through the score bound: it scales ALL of a triple's contributions alike), exp, the sum, the quotient and the
product: 5; the product with the derivative: 1; the derivative: 0 (a sign), 1 (a product), 3 (two products and a sum), and
for RotatE the term's 16 for (a, b), the norm, two quotients and the products with cos / sin / h and the divisor: 20."""


def reduction_depth(records, lanes_per_record):
    """Additions on the longest path of the backward's segmented sum for a row of `records` records: a thread's serial sum
    over its share of a chunk, the fold over the 256 / lanes_per_record threads of a column, the chunks in order."""
    slots = 256 // lanes_per_record
    inside = min(records, CHUNK)
    return -(-inside // slots) + slots + -(-records // CHUNK) + 1
