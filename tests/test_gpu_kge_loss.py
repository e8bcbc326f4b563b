"""The negative-sampling loss of the KGE mini-batches on the GPU (csrc/kge_loss.hip, kge.negative_sampling_loss): values and
gradients per element against the float64 torch formulation of tests/kge_loss_cases.py on the same fp32 scores.

Bounds.  u = 2^-24.  The rule of tests/test_gpu_kge.py: a figure of the kernel is at most FOUR TIMES the figure t that the
fp32 torch formulation reaches on the same inputs on the CPU, t floored at 1 unit.
  d_pos, d_neg:  max |got - ref| / (u |ref|) over the elements with |ref| >= 2^-126; an element whose float64 reference lies
                 below 2^-126 must satisfy |got| <= 2^-126;
  loss:          |got - ref| / (u S), S the float64 sum of the terms' absolute values over 2 W.
The dominant error of a self-adversarial weight is the ONE rounding of its exponent's argument T s - m, |T s - m| units at
worst, which the kernel (fmaf) and torch (an exact product by these temperatures, a rounded difference) share; what the kernel
adds is the library's expf and log1pf (1 unit each), the quotient of sigma, two products, and the rounding of 1 / Z_b and
1 / (2 W) to fp32.

Figures on an MI355X next to torch's on the CPU stand in the docstrings of the tests; the kernel's worst figure over all of
them is half its bound.
"""
import functools

import pytest
import torch

import gripnet_amd
import kge_batch_cases as kb
import kge_cases as kc
import kge_loss_cases as lc
from gripnet_amd import _hip
from gripnet_amd import kge

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _through_autograd(gpu, pos, neg, weight, T, factor=None):
    """(loss, d_pos, d_neg) of kge.negative_sampling_loss under loss.backward() (or (factor * loss).backward())."""
    p, n = pos.to(gpu).requires_grad_(True), neg.to(gpu).requires_grad_(True)
    loss = kge.negative_sampling_loss(p, n, T, None if weight is None else weight.to(gpu))
    (loss if factor is None else factor * loss).backward()
    return loss.detach(), p.grad, n.grad


def _kernels(gpu, pos, neg, weight, T, up=None, d_neg=None):
    """The same from the two launches themselves; pos / neg / weight on the device already."""
    loss, stats, scale = _hip.kge_ns_loss_forward(pos, neg, weight, T)
    d_pos, d_neg = _hip.kge_ns_loss_backward(pos, neg, weight, T, stats, scale, up, d_neg=d_neg)
    return loss, d_pos, d_neg, stats


def _hold(r, got, what, worst):
    """The three figures of one case against its bounds; `worst` collects (figure, torch's) per quantity."""
    loss, d_pos, d_neg = got
    figs = (abs(float(loss) - r["loss"]) / (lc.U * r["S"]), lc.figure(d_pos, r["d_pos"]), lc.figure(d_neg, r["d_neg"]))
    for name, fig, t in zip(("loss", "d_pos", "d_neg"), figs, r["t"]):
        print("{} {}: {:.2f} (torch fp32 {:.2f}, bound {:.2f})".format(what, name, fig, t, 4 * max(t, 1.0)))
        if fig / max(t, 1.0) > worst.get(name, (0.0, 0.0, 0.0))[0]:
            worst[name] = (fig / max(t, 1.0), fig, t)
    for name, fig, t in zip(("loss", "d_pos", "d_neg"), figs, r["t"]):
        assert fig <= 4 * max(t, 1.0), (what, name, fig, t)


@pytest.mark.parametrize("amplitude", lc.AMPLITUDES)
@pytest.mark.parametrize("K", lc.KS)
def test_values_and_gradients_per_element(gpu, K, amplitude):
    """K in {1, 2, 7, 8} (lane groups of 1, 2, 8, 8), {33, 64, 65, 257} (a wave per row: one turn, a second one, a scalar
    tail), 1,024 and 1,025 (the last row held in registers; the first one taken in two parts with a running maximum) x B in
    {1, 3, 5} x T in {none, 0.5, 1, 4} x weights absent and rand + 0.5, scores uniform in +-4 and +-200 (where a fifth to
    a third of the d_neg references underflow fp32: the clause on |got| <= 2^-126 is exercised on those).

    Figures on an MI355X, the largest of the 240 cases per amplitude, kernel (range of torch's fp32 figures):
      +-4:    loss 0.90 (0.01 - 3.22)   d_pos 1.47 (0.12 - 3.10)   d_neg 5.05 (0.14 - 7.13)     worst figure / bound 0.47
      +-200:  loss 0.85 (0.00 - 2.79)   d_pos 1.13 (0.00 - 2.57)   d_neg 66.51 (0.00 - 68.18)   worst figure / bound 0.50
    (the 63 - 68 units of d_neg at +-200 are the rounding of the argument T s - m at K >= 1,024 and at T = 0.5: torch's too)"""
    worst = {}
    for B in lc.BS:
        for T in lc.TEMPERATURES:
            for weighted in (False, True):
                r = lc.reference("random", B, K, amplitude, weighted, T)
                got = _through_autograd(gpu, r["pos"], r["neg"], r["weight"], T)
                _hold(r, got, "K={} +-{} B={} T={} w={}".format(K, amplitude, B, T, weighted), worst)
    print("worst of K={} +-{}: {}".format(K, amplitude, {k: "{:.2f} ({:.2f})".format(v[1], v[2]) for k, v in worst.items()}))


def test_one_row_more_than_a_pass_of_the_grid(gpu):
    """K = 2 and B = 65,537: one row more than the forward's 2,048 waves take in one pass (32 rows of two lanes per wave), so
    one wave strides on.  T = 1, weighted, +-4.

    Figures on an MI355X, kernel (torch fp32): loss 0.12 (0.12), d_pos 2.09 (3.74), d_neg 4.95 (5.75)."""
    r = lc.reference("random", lc.ONE_PASS_ROWS_K2 + 1, 2, 4.0, True, 1.0)
    _hold(r, _through_autograd(gpu, r["pos"], r["neg"], r["weight"], 1.0), "grid", {})


@pytest.mark.parametrize("T", lc.TEMPERATURES)
@pytest.mark.parametrize("K", (8, 65))
def test_hand_built_rows(gpu, K, T):
    """Rows built by hand (kge_loss_cases.hand_built): all scores equal; one score more than 104 / T above the rest, so that
    every other weight underflows; pos = +-200; a zero score; a row of weight 0, which gets exact zeros.

    Figures on an MI355X, the largest of the eight cases, kernel (range of torch's): loss 0.65 (0.07 - 1.36), d_pos 1.09
    (0.91 - 1.09), d_neg 3.33 (1.88 - 4.58); worst figure / bound 0.44."""
    r = lc.reference("hand", 5, K, 0.0, True, T)
    loss, d_pos, d_neg = _through_autograd(gpu, r["pos"], r["neg"], r["weight"], T)
    _hold(r, (loss, d_pos, d_neg), "hand K={} T={}".format(K, T), {})
    assert float(d_pos[3].abs()) == 0.0 and float(d_neg[3].abs().max()) == 0.0
    if T is not None:                                         # the weights below the row's largest underflow to zero
        others = torch.arange(K) != K // 2
        assert float(d_neg[1].cpu()[others].abs().max()) == 0.0


def _wide(t, ld, left, gpu):
    """`t` as the column view big[:, left:left + K] of a NaN matrix with rows of `ld` floats."""
    big = torch.full((t.shape[0], ld), NAN, device=gpu)
    big[:, left:left + t.shape[1]] = t.to(gpu)
    return big, big[:, left:left + t.shape[1]]


@pytest.mark.parametrize("T", (None, 1.0))
@pytest.mark.parametrize("K", (8, 64, 260))
def test_column_views_give_the_bits_of_contiguous_operands(gpu, K, T):
    """neg and d_neg as column views of wider NaN matrices: ld = K + 4 from an aligned base (the vector path at K = 64 and
    260), ld = K + 3, and ld = K + 4 from a base one float further (the scalar path).  Loss, row figures and gradients
    have the bits of the contiguous run, and the NaN beside the views is neither read into a result nor overwritten."""
    r = lc.reference("random", 5, K, 4.0, True, T)
    pos, weight = r["pos"].to(gpu), r["weight"].to(gpu)
    want = _kernels(gpu, pos, r["neg"].to(gpu), weight, T)
    for ld, left in ((K + 4, 0), (K + 3, 0), (K + 4, 1)):
        big, neg = _wide(r["neg"], ld, left, gpu)
        out_big = torch.full((5, ld), NAN, device=gpu)
        got = _kernels(gpu, pos, neg, weight, T, d_neg=out_big[:, left:left + K])
        for a, b in zip(want, got):
            assert torch.equal(a, b), (ld, left)
        beside = torch.cat([out_big[:, :left], out_big[:, left + K:]], dim=1)
        assert bool(torch.isnan(beside).all())
        assert torch.equal(big[:, left:left + K].cpu(), r["neg"])


@pytest.mark.parametrize("T", (None, 1.0))
@pytest.mark.parametrize("K", (8, 65, lc.REGISTER_K + 1))
def test_a_nan_score_reaches_the_loss_and_its_own_row(gpu, K, T):
    """One NaN negative: the loss is NaN and that row of d_neg is NaN; every other row of d_neg and all of d_pos keep the
    bits of the clean run.  One NaN positive: the loss and its own d_pos."""
    r = lc.reference("random", 5, K, 4.0, True, T)
    clean = _through_autograd(gpu, r["pos"], r["neg"], r["weight"], T)
    neg = r["neg"].clone()
    neg[1, K // 3] = NAN
    loss, d_pos, d_neg = _through_autograd(gpu, r["pos"], neg, r["weight"], T)
    keep = [0, 2, 3, 4]
    assert bool(torch.isnan(loss)) and bool(torch.isnan(d_neg[1]).all())
    assert torch.equal(d_neg[keep], clean[2][keep]) and torch.equal(d_pos, clean[1])
    pos = r["pos"].clone()
    pos[2] = NAN
    loss, d_pos, d_neg = _through_autograd(gpu, pos, r["neg"], r["weight"], T)
    assert bool(torch.isnan(loss)) and bool(torch.isnan(d_pos[2]))
    keep = [0, 1, 3, 4]
    assert torch.equal(d_pos[keep], clean[1][keep]) and torch.equal(d_neg, clean[2])


@pytest.mark.parametrize("K", (8, 257))
def test_upstream_gradient(gpu, K):
    """(3 * loss).backward() gives three times the gradients of loss.backward() within one rounding per element (the
    upstream multiplies last: half a unit, or half a subnormal step); a null upstream is the upstream 1.0 bit for bit."""
    r = lc.reference("random", 5, K, 200.0, True, 0.5)
    _, d_pos, d_neg = _through_autograd(gpu, r["pos"], r["neg"], r["weight"], 0.5)
    _, d_pos3, d_neg3 = _through_autograd(gpu, r["pos"], r["neg"], r["weight"], 0.5, factor=3.0)
    for one, three in ((d_pos, d_pos3), (d_neg, d_neg3)):
        exact = 3.0 * one.double()
        assert bool(((three.double() - exact).abs() <= torch.clamp(lc.U * exact.abs(), min=2.0 ** -150)).all())
    pos, neg, weight = r["pos"].to(gpu), r["neg"].to(gpu), r["weight"].to(gpu)
    null = _kernels(gpu, pos, neg, weight, 0.5, up=None)
    unit = _kernels(gpu, pos, neg, weight, 0.5, up=torch.ones((), device=gpu))
    assert torch.equal(null[1], unit[1]) and torch.equal(null[2], unit[2])
    assert torch.equal(null[1], d_pos) and torch.equal(null[2], d_neg)


def test_inputs_that_are_not_fp32_rows_are_made_so(gpu):
    """A float64 block and a transposed one go through a contiguous fp32 copy: the gradients come back in the inputs' own
    dtype and layout, with the fp32 run's values."""
    r = lc.reference("random", 5, 33, 4.0, False, 1.0)
    want = _through_autograd(gpu, r["pos"], r["neg"], None, 1.0)
    got = _through_autograd(gpu, r["pos"].double(), r["neg"].double(), None, 1.0)
    assert got[1].dtype == torch.float64 and torch.equal(got[0], want[0]) and torch.equal(got[2].float(), want[2])
    n = r["neg"].t().contiguous().to(gpu).t().requires_grad_(True)
    loss = kge.negative_sampling_loss(r["pos"].to(gpu), n, 1.0)
    loss.backward()
    assert torch.equal(loss.detach(), want[0]) and torch.equal(n.grad, want[2])


# ---- through the module -------------------------------------------------------------------------------------------------
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


@functools.lru_cache(maxsize=None)
def _module_reference(model, side, T):
    """Case A, its subsampling weights, and the float64 gradients of the whole chain (scores and loss) with their scales."""
    c = kb.case_a(model, side)
    weight = torch.rand(c.B, generator=torch.Generator().manual_seed(3)) + 0.5
    ent = c.ent.double().requires_grad_(True)
    rel = c.rel.double().requires_grad_(True)
    pos = kc.raw_score(model, ent, rel, c.positive, c.et, c.gamma)
    neg = kc.raw_score(model, ent, rel, c.sample, c.et_list, c.gamma).view(c.B, c.K)
    pos.retain_grad()
    neg.retain_grad()
    loss = lc.loss_terms(pos, neg, T, weight)[0]
    loss.backward()
    both = torch.cat([c.positive, c.sample], dim=1)
    types = torch.cat([c.et, c.et_list])
    up = torch.cat([pos.grad, neg.grad.reshape(-1)])
    scale = kc.abs_contributions(model, c.ent, c.rel, both, types, c.gamma, up, log_sigmoid=False)
    return dict(case=c, weight=weight, loss=float(loss), g64=(ent.grad, rel.grad), scale=scale)


@pytest.mark.parametrize("side", kb.SIDES)
@pytest.mark.parametrize("model", kc.MODELS)
def test_through_the_module(gpu, model, side):
    """model.negative_sampling_loss on case A of kge_batch_cases (B = 40, K = 130, T = 1): the embeddings' gradients are bit
    for bit those of _hip.kge_backward and _hip.kge_batch_backward fed with the loss kernel's d_pos / d_neg, added; against
    the float64 chain they are held to four times the figure of the kge.self_adversarial_loss path on the same scorers
    (without weights: that path has none).

    Figures on an MI355X, d_ent / d_rel in units of u * (sum of |contributions|), new loss (torch-op loss), tail then head:
      TransE 4.96 (7.06) / 1.52 (1.52), 8.38 (6.97) / 1.33 (1.27);    DistMult 8.92 (9.06) / 2.02 (2.02), 9.39 (9.39) / 2.84 (2.84);
      ComplEx 13.62 (13.21) / 3.29 (2.25), 22.12 (22.28) / 3.60 (3.60);   RotatE 66.02 (66.02) / 2.87 (2.67), 24.66 (24.66) / 3.10 (3.36)
    - the scorers' own fp32 error, which both paths share."""
    T = 1.0
    r = _module_reference(model, side, T)
    c = r["case"]
    m = _module(c, gpu)
    positive, et, negatives, weight = c.positive.to(gpu), c.et.to(gpu), c.negatives.to(gpu), r["weight"].to(gpu)
    loss = m.negative_sampling_loss(positive, et, negatives, kb.MODES[side], T, weight)
    loss.backward()
    got = _grads(m)
    # the same from the entry points, one by one
    ent, rel = m.entity_embedding.detach(), m.relation_embedding.detach()
    gamma, divisor = m._constants()
    fixed = kb.fixed_of(positive, side)
    pos = _hip.kge_forward(model, ent, rel, positive, et, gamma, divisor, False, torch.empty(c.B, device=gpu))
    neg = _hip.kge_batch_forward(model, ent, rel, fixed, et, negatives, side, gamma, divisor, False, torch.empty(c.B, c.K, device=gpu))
    by_hand, d_pos, d_neg, _ = _kernels(gpu, pos, neg, weight, T)
    one = _hip.kge_backward(model, ent, rel, positive, et, divisor, d_pos, None, torch.empty_like(ent), torch.empty_like(rel))
    two = _hip.kge_batch_backward(model, ent, rel, fixed, et, negatives, side, divisor, d_neg, None, torch.empty_like(ent),
                                  torch.empty_like(rel))
    assert torch.equal(loss.detach(), by_hand)
    assert torch.equal(got[0], one[0] + two[0]) and torch.equal(got[1], one[1] + two[1])
    assert abs(float(loss) - r["loss"]) <= 1e-5 * abs(r["loss"])
    for g, ref, scale, name in zip(got, r["g64"], r["scale"], ("d_ent", "d_rel")):
        print("{} {} weighted {}: {:.2f}".format(model, side, name, kc.figure(g, ref, scale)))
    # against the torch-op loss on the same scorers, without weights
    r0 =_unweighted_reference(model, side, T)
    m.negative_sampling_loss(positive, et, negatives, kb.MODES[side], T).backward()
    ours = _grads(m)
    kge.self_adversarial_loss(m.score(positive, et), m.score((positive, negatives), et, kb.MODES[side]), T).backward()
    theirs = _grads(m)
    for g, other, ref, scale, name in zip(ours, theirs, r0["g64"], r0["scale"], ("d_ent", "d_rel")):
        fig, t = kc.figure(g, ref, scale), kc.figure(other, ref, scale, strict=False)
        print("{} {} {}: {:.2f} (torch-op loss {:.2f})".format(model, side, name, fig, t))
        assert fig <= 4 * max(t, 1.0), (name, fig, t)
    _hip.raise_if_index_errors(gpu)


@functools.lru_cache(maxsize=None)
def _unweighted_reference(model, side, T):
    c = kb.case_a(model, side)
    ent = c.ent.double().requires_grad_(True)
    rel = c.rel.double().requires_grad_(True)
    pos = kc.raw_score(model, ent, rel, c.positive, c.et, c.gamma)
    neg = kc.raw_score(model, ent, rel, c.sample, c.et_list, c.gamma).view(c.B, c.K)
    pos.retain_grad()
    neg.retain_grad()
    lc.loss_terms(pos, neg, T, None)[0].backward()
    up = torch.cat([pos.grad, neg.grad.reshape(-1)])
    scale = kc.abs_contributions(model, c.ent, c.rel, torch.cat([c.positive, c.sample], dim=1), torch.cat([c.et, c.et_list]), c.gamma,
                                 up, log_sigmoid=False)
    return dict(g64=(ent.grad, rel.grad), scale=scale)


@pytest.mark.parametrize("B,K", ((40, 8), (5, 257), (3, lc.REGISTER_K + 1)))
def test_same_bits_in_every_call_and_under_capture(gpu, B, K):
    """Two calls give identical bits; forward + backward captured with torch.cuda.graph and replayed give the eager bits
    (no host synchronisation inside: the capture would fail), the outputs refilled with NaN between the replays (the
    forward's arrival counter is left ready by every launch, replays included)."""
    pos, neg, weight = (t.to(gpu) for t in lc.block(B, K, 4.0, True, seed=3))

    def step():
        loss, d_pos, d_neg, stats = _kernels(gpu, pos, neg, weight, 1.0)
        return loss, d_pos, d_neg, stats

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
    for _ in range(2):
        for t in captured:
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)


def test_refusals(gpu):
    """B == 0 or K == 0 is GN_ERR_INVALID_ARG at the C boundary (the binding's ValueError), as are a short leading dimension and missing row figures."""
    pos, neg = torch.zeros(3, device=gpu), torch.zeros(3, 4, device=gpu)
    out = [torch.empty((), device=gpu), torch.empty(3, 2, device=gpu), torch.empty(1, device=gpu)]
    ws = torch.zeros(int(_hip.load().gn_kge_ns_loss_workspace_bytes(3)), dtype=torch.uint8, device=gpu)

    def forward(b, k, ld, stats=out[1], adversarial=1):
        _hip._call("gn_kge_ns_loss_forward_f32", pos.data_ptr(), neg.data_ptr(), ld, b, k, None, adversarial, 1.0, out[0].data_ptr(),
                   None if stats is None else stats.data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel(), _hip.stream_ptr(gpu))

    for args in ((0, 4, 4), (3, 0, 4), (3, 4, 3)):
        with pytest.raises(ValueError):
            forward(*args)
    with pytest.raises(ValueError):
        forward(3, 4, 4, stats=None)
    forward(3, 4, 4, stats=None, adversarial=0)
    torch.cuda.synchronize()
    assert abs(float(out[0]) - 0.6931472) < 1e-6
