"""The inputs, bounds and measures of tests/test_gpu_head.py, checked without a GPU.

* `head_cases.exact_logits` is exact for every (k, n, s) in use: fp32 and float64 products give the same bits.
* torch's own fp32 softmax, link loss and class loss stay inside the bounds the kernels are held to, on the very inputs the
  GPU module uses: the bounds are fp32's, not a kernel's.
* At most 5 % of a softmax case's elements lie below 2^-100 (where only a range is checked).
* The measures see what they are for: a softmax without max subtraction is non-finite, a link loss with one spike dropped
  or counted twice leaves its bound, and so does a class loss that reads the column beside the label.

Measured (largest figure over the cases, in multiples of u = 2^-24): torch's fp32 softmax 5.33 of 12 + cols / 64, the softmax
gradient's fp32 expression 4.99 of 10 + cols / 64, link loss 2.67 of 16, its single logarithm 1.0 of 4, class loss 1.41 of 8."""
import pytest
import torch

import head_cases as hc


def _kns():
    kns = {(k, n) for k, n in hc.FUSED_KN + hc.GEMM_KN}
    kns |= {(hc.ROWS_K, c) for _, c in hc.ROWS_SHAPES}
    kns |= {(hc.backward_depth(c), c) for _, c in hc.BACKWARD_SHAPES}
    return sorted(kns)


@pytest.mark.parametrize("k,n", _kns())
def test_exact_logits_are_exact(k, n):
    z, w = hc.exact_logits(65, k, n, seed=k * 1009 + n)
    s = hc.scale_of(k)
    assert torch.equal((z @ w).double(), z.double() @ w.double())
    assert torch.equal(z, z.round()) and torch.equal(w * s, (w * s).round())
    assert (z[:, 0] == 64).all() and (w[0] == 32).all()
    assert float((z @ w).min()) > 1024                              # the common offset is there: exp(logit) overflows


def test_the_scale_of_the_deepest_case_is_needed():
    """With s = 16 the k = 2560 case loses far more than 5 % of its elements below 2^-100."""
    z, w = hc.exact_logits(65, 2560, 16, seed=1, s=16)
    ref = torch.softmax(z.double() @ w.double(), dim=1)
    assert float((ref < hc.LIVE).double().mean()) > 0.25


@pytest.mark.parametrize("k,n,m", hc.FUSED_CASES + hc.GEMM_CASES, ids=lambda v: str(v))
def test_torch_softmax_on_the_head_cases(k, n, m):
    case = hc.head_case(k, n, m)
    assert torch.equal(case.logits32.double(), case.logits64)
    rel, dead = hc.softmax_measure(torch.softmax(case.logits32, dim=1), case.ref64)
    hc.show("host softmax " + repr(case), rel=rel, bound=hc.softmax_bound(n))
    assert rel <= hc.softmax_bound(n)
    assert dead <= hc.DEAD_SHARE, dead
    if m >= 4:
        assert int((~case.inside).sum()) == 2 and bool((case.nodes < 0).any()) and bool((case.nodes == case.table_rows).any())
    if m >= 5:
        assert case.nodes[case.inside].unique().numel() < int(case.inside.sum())      # repeats
    # without max subtraction every row is non-finite, and the measure refuses it
    naive = torch.exp(case.logits32[case.inside]) / torch.exp(case.logits32[case.inside]).sum(dim=1, keepdim=True)
    if naive.numel():
        assert not torch.isfinite(naive).any()
        with pytest.raises(AssertionError):
            hc.softmax_measure(naive, case.ref64[case.inside])


@pytest.mark.parametrize("rows,cols", hc.ROWS_SHAPES)
def test_torch_softmax_on_the_in_place_cases(rows, cols):
    x, ref = hc.rows_logits(rows, cols)
    rel, dead = hc.softmax_measure(torch.softmax(x, dim=1), ref)
    hc.show("host softmax rows {}x{}".format(rows, cols), rel=rel, bound=hc.softmax_bound(cols))
    assert rel <= hc.softmax_bound(cols) and dead <= hc.DEAD_SHARE


def test_softmax_measure_sees_a_wrong_small_probability():
    """A probability of 1e-30 that is 1 % off passes any max-norm check and fails this one; below 2^-100 only the range
    counts."""
    ref = torch.tensor([[1.0 - 1e-30, 1e-30, 2.0 ** -120]], dtype=torch.float64)
    good = ref.clone()
    good[0, 2] = 2.0 ** -99
    assert hc.softmax_measure(good, ref)[0] == 0
    bad = ref.clone()
    bad[0, 1] *= 1.01
    assert hc.softmax_measure(bad, ref)[0] > 1e5 * hc.U
    for v in (-1e-40, 2.0 ** -98):
        worse = ref.clone()
        worse[0, 2] = v
        with pytest.raises(AssertionError):
            hc.softmax_measure(worse, ref)


@pytest.mark.parametrize("rows,cols", hc.BACKWARD_SHAPES)
def test_softmax_backward_cases_stay_normal(rows, cols):
    """No magnitude of a backward case is so small that a gradient could underflow (a denormal's rounding error is
    absolute: 2^-150 would count against the bound), and the fp32 expression itself is inside the bound."""
    p, g, ref, mag = hc.softmax_backward_case(rows, cols)
    assert float(mag.min()) >= 2.0 ** -116                          # 2^-150 is then 2^-10 u of any magnitude
    assert float(p.sum(dim=1).sub(1).abs().max()) < 1e-5
    assert cols == 1 or (float(p.max(dim=1).values.mean()) > 0.5 and float(p[p > 0].min()) < 1e-9)    # saturated rows
    dx = p * (g - (p * g).sum(dim=1, keepdim=True))
    rho = hc.sc.componentwise(dx, ref, mag)
    hc.show("host softmax backward {}x{}".format(rows, cols), rho=rho, bound=hc.backward_bound(cols))
    assert rho <= hc.backward_bound(cols)
    # the measure sees a dot product that dropped its largest term
    terms = p * g
    terms[torch.arange(rows), terms.abs().argmax(dim=1)] = 0
    if cols > 1:
        assert hc.sc.componentwise(p * (g - terms.sum(dim=1, keepdim=True)), ref, mag) > 1000 * hc.backward_bound(cols)


@pytest.mark.parametrize("n_pos,n_neg", hc.LINK_SIZES)
def test_torch_link_loss_and_one_spike_more_or_less(n_pos, n_neg):
    pos, neg, ref = hc.link_case(n_pos, n_neg)
    assert ref > 0
    rel = abs(hc.link_torch32(pos, neg) - ref) / ref
    hc.show("host link loss {}+{}".format(n_pos, n_neg), rel=rel, bound=hc.LINK_BOUND)
    assert rel <= hc.LINK_BOUND
    # every element off the spikes contributes exactly 0 in fp32
    eps = torch.tensor(hc.EPS, dtype=torch.float32)
    assert float(torch.log(torch.ones(1) + eps)) == 0 and float(torch.log(1.0 - torch.zeros(1) + eps)) == 0
    # the weakest spike of either list, dropped or counted twice
    for n, negative in ((n_pos, False), (n_neg, True)):
        if n == 0:
            continue
        _, idx, terms = hc.link_indicator(n, negative)
        assert idx.numel() >= min(n, 11) and (terms < 0).all()
        weakest = float(terms.abs().min()) / n
        for wrong in (ref - weakest, ref + weakest):
            assert abs(wrong - ref) > 100 * hc.LINK_BOUND * ref       # (measured: 680 bounds at 2.2 M scores, more below)


def test_link_spikes_reach_every_unroll_slot():
    """At 2.2 M scores a spike sits on both sides of every multiple of 524288 float (the first element of slot k of the
    four-deep unroll is vector 131072 k) and of the second trip, in the scalar tail and at the very end."""
    n = 2228227
    idx = set(hc.spike_indices(n).tolist())
    for a in (0, 4, 524288, 1048576, 1572864, 2097152, 4 * (n // 4), n):
        assert {j for j in range(a - 5, a + 6) if 0 <= j < n} <= idx
    assert max(idx) == n - 1 and len(idx) < 100
    assert hc.alignments_of(524293, 174764)[-1] == "adjacent" and "adjacent" not in hc.alignments_of(2097159, 699053)
    assert "adjacent" in hc.alignments_of(699053, 2097159)


def test_log_points_and_their_reference():
    for negative in (False, True):
        x = hc.log_points(negative)
        ref = hc.log_ref(x, negative)
        assert x.numel() == 164 and torch.isfinite(ref).all() and (ref >= 0).all()
        got = -torch.log((1.0 - x if negative else x) + torch.tensor(hc.EPS, dtype=torch.float32))
        rel = hc.relative(got, ref)
        hc.show("host log, " + ("neg" if negative else "pos"), rel=rel, bound=hc.LOG_BOUND)
        assert rel <= hc.LOG_BOUND
        # an absolute error of 2^-24 (a logarithm that is only accurate in absolute terms) fails near 1
        near = (ref > 0) & (ref < 1e-3)
        assert int(near.sum()) >= 10 and hc.relative((got + 2.0 ** -24)[near], ref[near]) > 100 * hc.LOG_BOUND


@pytest.mark.parametrize("n_pos,n_neg", [sz for sz in hc.LINK_SIZES if max(sz) < 10 or max(sz) == 524293])
def test_link_gradient_reference(n_pos, n_neg):
    pos, neg = hc.link_grad_case(n_pos, n_neg)
    eps = torch.tensor(hc.EPS, dtype=torch.float32)
    refs = hc.link_grad_ref(pos, neg, 3.0)
    for x, n, ref, vals in ((pos, n_pos, refs[0], 3), (neg, n_neg, refs[1], 4)):
        if n == 0:
            continue
        assert float(x.min()) >= 0 and float(x.max()) <= 1
        if n >= 4 * vals:
            for v in (0.0, hc.DENORMAL, 1.0) + ((1.0 - 2.0 ** -24,) if vals == 4 else ()):
                hits = (x == v).nonzero().view(-1)
                assert hits.numel() == 3 and hits[0] < vals and hits[-1] >= n - vals, (v, hits)
        got = (torch.tensor(-3.0) / n) / (x + eps) if x is pos else (torch.tensor(3.0) / n) / (1.0 - x + eps)
        assert torch.isfinite(ref).all()
        assert hc.relative(got, ref) <= hc.LINK_GRAD_BOUND


@pytest.mark.parametrize("classes", hc.CLASS_C)
@pytest.mark.parametrize("n", hc.CLASS_N)
def test_torch_class_loss_and_the_column_beside_the_label(n, classes):
    score, labels = hc.class_indicator(n, classes)
    ref = hc.class_ref(score, labels)
    assert ref > 0
    rel = abs(hc.class_torch32(score, labels) - ref) / ref
    hc.show("host class loss n={} classes={}".format(n, classes), rel=rel, bound=hc.CLASS_BOUND)
    assert rel <= hc.CLASS_BOUND
    if classes > 1:                                                  # one row that reads the next column
        for row in (0, n // 2, n - 1):
            beside = labels.clone()
            beside[row] = (beside[row] + 1) % classes
            assert abs(hc.class_ref(score, beside) - ref) > 1000 * hc.CLASS_BOUND * ref
    # one spike row dropped
    row = int(hc.class_spike_rows(n)[-1])
    dropped = ref + float(torch.log(score[row, labels[row]].double() + hc.EPS32)) / n
    assert abs(dropped - ref) > 1000 * hc.CLASS_BOUND * ref


def test_class_loss_reference_skips_labels_outside():
    score, labels = hc.class_indicator(8200, 8)
    labels = labels.clone()
    labels[10], labels[2058], labels[8199] = -1, 8, -1
    ref = hc.class_ref(score, labels)
    ok = (labels >= 0) & (labels < 8)
    assert abs(ref - hc.class_torch32(score[ok], labels[ok]) * float(ok.sum()) / 8200) <= hc.CLASS_BOUND * ref
    assert ref != hc.class_ref(*hc.class_indicator(8200, 8))        # row 8199 is a spike: leaving it out shows
    assert (hc.class_grad_ref(score, labels, 2.0)[[10, 2058, 8199]] == 0).all()


@pytest.mark.parametrize("rows,cols", hc.MERGE_SHAPES)
def test_merge_references(rows, cols):
    dst, src, src2 = hc.merge_operands(rows, cols)
    if rows * cols >= len(hc.SRC2_VALUES):
        assert {float(v) for v in src2.view(-1)} == {float(torch.tensor(v, dtype=torch.float32)) for v in hc.SRC2_VALUES}
        assert bool(((src2 == 0) & torch.signbit(src2)).any()) and bool(((src2 == 0) & ~torch.signbit(src2)).any())
        assert bool(((src2 != 0) & (src2.abs() < 2.0 ** -126)).any())
    for mode in range(11):
        ref, mag = hc.merge_ref(mode, dst, src, src2)
        assert torch.isfinite(ref).all() and ref.shape == (rows, cols) and (mag >= ref.abs() * (1 - 1e-12)).all()
        if mode in (6, 9):
            assert (ref[src2 == 0] == 0).all() and (ref[src2 != 0] != 0).all()
        if mode in (5, 10):
            assert (ref[src2 <= 0] == 0).all()
        if mode in hc.MERGE_EXACT:
            assert torch.equal(ref, ref.float().double())           # representable: the kernel can be held to the bits
