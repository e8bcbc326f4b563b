"""The classifier head and the losses per element against float64: the class decoder with its softmax (fused and GEMM +
stand-alone), the softmax's gradient, the link loss, the class loss and the element-wise merges.

The rest of the suite holds this stage to max-norm tolerances on logits of order 1.  Its values feed a logarithm, so here
every probability is held to a RELATIVE error, on logits that are exact in fp32 and offset by 2048 (a row without max
subtraction overflows), and every loss runs on inputs whose terms are exactly 0 except at spikes placed around every unroll
slot, clamped load, tail and end of the kernels' loops (tests/head_cases.py; tests/test_head_host.py checks the inputs, the
bounds on torch's own fp32 and that each measure sees the fault it is for).

Bounds, with u = 2^-24 (each test prints its figure in multiples of u):

    softmax                 rel <= (12 + cols / 64) u over the elements >= 2^-100; 0 <= y <= 2^-99 below
    softmax backward        rho <= (10 + cols / 64) u of p (|g| + sum p |g|)
    link loss               16 u relative; its gradient 4 u per element; a single term (the logarithm itself) 4 u
    class loss              8 u relative; its gradient 4 u on the label column, exactly 0 off it
    merges                  modes 0, 1, 5, 6, 8, 9, 10 exact; modes 2, 3, 4, 7 within 2 u of the operands' absolute sum

Measured on an MI355X (largest figure of a section, in multiples of u, next to its bound):

    fused class scores + softmax        3.89   of 12.2      (k = 128, n = 16; the 160 KB launch at k = 2560 runs)
    GEMM + gn_softmax_rows_f32          5.43   of 15.1      (k = 129, n = 200)
    gn_softmax_rows_f32 in place        5.33   of 14        (257 x 130)
    logits without softmax              the same bits on every case
    softmax backward                    4.23   of 11        (257 x 65)
    link loss, indicator inputs         1.24   of 16        every size, list combination and alignment; repeats the same bits
    link loss backward                  1.89   of 4
    link loss, one term                 2.66   of 4         pos and neg alike, the same figure near 1: without fast-math
                                                            __logf compiles to logf's own instruction sequence
    class loss / its gradient           1.14   of 8  /  1.61 of 4
    merges, modes 2, 3, 4, 7            0.68   of 2         the other seven modes exact, zeros and denormals included

With a library changed in seven places, each of them fails exactly its tests here and passes the rest of this module: the
stand-alone softmax's sum stopped at column 128, __expf in the fused softmax, the backward's dot product stopped at column
64, sign(0) = -1 in merge mode 6, the shorter negative list's clamped loads counted, the scalar link loss without its last
positive, and a class-loss `bad` branch that counts nothing.
"""
import pytest
import torch

import head_cases as hc
import scale_cases as sc
from gripnet_amd import _hip, utils

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(autouse=True)
def every_fast_path_on(monkeypatch):
    monkeypatch.setenv("GN_DISABLE_FAST", "0")


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


# ---- 1. softmax on exact logits -----------------------------------------------------------------------------------------
def _class_scores(case, dev, softmax):
    """gn_class_scores_f32 on a case with every operand a column slice (ld_z > k, ld_w > n, ld_out > n)."""
    _, z = _sliced(case.z, 1, case.k + 3, dev)
    _, w = _sliced(case.w, 2, case.n + 5, dev)
    big, out = _sliced(torch.full((case.m, case.n), NAN), 2, case.n + 3, dev)
    _hip.class_scores(z, w, case.nodes.to(dev), out, softmax)
    assert _beside_is_nan(big, 2, case.n), "the columns beside the output were written"
    return out.cpu()


def _check_scores(case, dev, route):
    y = _class_scores(case, dev, True)
    rel, dead = hc.softmax_measure(y, case.ref64)
    line = hc.show("{} softmax {!r}".format(route, case), rel=rel, bound=hc.softmax_bound(case.n))
    assert rel <= hc.softmax_bound(case.n), line
    assert dead <= hc.DEAD_SHARE
    outside = y[~case.inside]
    assert torch.equal(outside, torch.full_like(outside, 1.0) / case.n), "a row outside the table is not exactly 1 / n"
    logits = _class_scores(case, dev, False)
    assert torch.equal(logits, case.logits32), "exact logits did not come back bit for bit"
    return rel


@pytest.mark.parametrize("k,n,m", hc.FUSED_CASES, ids=str)
def test_fused_class_scores_per_element(gpu, k, n, m):
    """k_class_scores (at most 16 classes, W in LDS up to exactly 160 KB at k = 2560): every probability relative to float64,
    out-of-table entries exactly 1 / n, the logits themselves bit for bit."""
    _check_scores(hc.head_case(k, n, m), gpu, "fused")


@pytest.mark.parametrize("k,n,m", hc.GEMM_CASES, ids=str)
def test_gemm_route_class_scores_per_element(gpu, k, n, m):
    """The row-gather GEMM + gn_softmax_rows_f32 behind the same entry point: more than 16 classes (one, two and four trips
    of the softmax's 64-column loops) and the first depth whose W does not fit the fused kernel's LDS."""
    _check_scores(hc.head_case(k, n, m), gpu, "gemm")


@pytest.mark.parametrize("rows,cols", hc.ROWS_SHAPES)
def test_softmax_rows_in_place_per_element(gpu, rows, cols):
    x, ref = hc.rows_logits(rows, cols)
    big, view = _sliced(x, 3, cols + 6, gpu)
    _hip.softmax_rows(view)
    assert _beside_is_nan(big, 3, cols)
    rel, dead = hc.softmax_measure(view.cpu(), ref)
    line = hc.show("softmax_rows {}x{}".format(rows, cols), rel=rel, bound=hc.softmax_bound(cols))
    assert rel <= hc.softmax_bound(cols) and dead <= hc.DEAD_SHARE, line


# ---- 2. softmax backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", hc.BACKWARD_SHAPES)
def test_softmax_backward_per_element(gpu, rows, cols):
    p, g, ref, mag = hc.softmax_backward_case(rows, cols)
    _, pv = _sliced(p, 1, cols + 2, gpu)
    _, gv = _sliced(g, 2, cols + 5, gpu)
    big, dx = _sliced(torch.full((rows, cols), NAN), 3, cols + 7, gpu)
    assert len({_hip.ld(pv), _hip.ld(gv), _hip.ld(dx)}) == (3 if rows > 1 else 1)
    _hip._call("gn_softmax_rows_backward_f32", _hip.ptr(pv), pv.stride(0), _hip.ptr(gv), gv.stride(0), _hip.ptr(dx), dx.stride(0),
               rows, cols, _hip.stream_ptr(gpu))
    assert _beside_is_nan(big, 3, cols)
    rho = sc.componentwise(dx.cpu(), ref, mag)
    line = hc.show("softmax backward {}x{}".format(rows, cols), rho=rho, bound=hc.backward_bound(cols))
    assert rho <= hc.backward_bound(cols), line


# ---- 3. link loss -------------------------------------------------------------------------------------------------------
def _placed(pos, neg, how, dev):
    """The two lists on the device: each at a 16-byte line or 4 bytes behind one, or as adjacent views of one buffer."""
    def at(x, off):
        buf = torch.empty(x.numel() + off, device=dev)
        buf[off:] = x.to(dev)
        return buf[off:]
    if how == "adjacent":
        buf = torch.cat([pos, neg]).to(dev)
        p, n = buf[:pos.numel()], buf[pos.numel():]
        assert p.data_ptr() % 16 == 0 and n.data_ptr() % 16 == 4
        return p, n
    p, n = at(pos, 1 if how in ("pos+4", "both+4") else 0), at(neg, 1 if how in ("neg+4", "both+4") else 0)
    for x, shifted in ((p, how in ("pos+4", "both+4")), (n, how in ("neg+4", "both+4"))):
        if x.numel():
            assert x.data_ptr() % 16 == (4 if shifted else 0)
    return p, n


def _counter(dev):
    """The arrival counter behind the 512 pairs of partial sums of the link loss's workspace."""
    ws = _hip.zeroed_once(dev, "link loss", _hip.load().gn_link_loss_workspace_bytes)
    return int(ws[512 * 16:512 * 16 + 4].view(torch.int32).item())


@pytest.mark.parametrize("n_pos,n_neg", hc.LINK_SIZES)
def test_link_loss_every_path_and_position(gpu, n_pos, n_neg):
    """The vector kernel (every unroll slot, the clamped loads of the shorter list, the second trip, the tail) and the scalar
    kernel (either list 4 bytes off a 16-byte line) on indicator inputs: one element dropped or read twice anywhere near
    the loops' edges moves the loss by hundreds of bounds."""
    pos, neg, ref = hc.link_case(n_pos, n_neg)
    worst = 0.0
    for how in hc.alignments_of(n_pos, n_neg):
        p, n = _placed(pos, neg, how, gpu)
        first = _hip.link_loss_forward(p, n, hc.EPS)
        again = _hip.link_loss_forward(p, n, hc.EPS)
        assert _counter(gpu) == 0, "the launch did not leave its counter ready"
        assert first.item() == again.item(), "a repeated call gave other bits"
        rel = abs(first.item() - ref) / ref
        assert rel <= hc.LINK_BOUND, hc.show("link loss {}+{} {}".format(n_pos, n_neg, how), rel=rel, bound=hc.LINK_BOUND)
        worst = max(worst, rel)
    hc.show("link loss {}+{}".format(n_pos, n_neg), rel=worst, bound=hc.LINK_BOUND)


def test_link_loss_calls_share_one_workspace(gpu):
    """Calls of different sizes and alignments in a row, nothing synchronised in between, then the same round again: each
    its own value, the same bits both times, the counter back at 0."""
    sizes = ((9, 3), (524293, 174764), (0, 7), (174764, 524293), (5, 0), (524293, 0), (2, 8))
    hows = ("adjacent", "both+4", "neg+4", "aligned", "pos+4", "aligned", "both+4")
    placed = []
    for (n_pos, n_neg), how in zip(sizes, hows):
        pos, neg, ref = hc.link_case(n_pos, n_neg)
        assert how in hc.alignments_of(n_pos, n_neg)
        placed.append(_placed(pos, neg, how, gpu) + (ref,))
    rounds = [torch.stack([_hip.link_loss_forward(p, n, hc.EPS) for p, n, _ in placed]).cpu() for _ in range(2)]
    assert _counter(gpu) == 0
    assert torch.equal(rounds[0], rounds[1])
    rel = max(abs(float(y) - ref) / ref for y, (_, _, ref) in zip(rounds[0], placed))
    line = hc.show("link loss, one workspace", rel=rel, bound=hc.LINK_BOUND)
    assert rel <= hc.LINK_BOUND, line


@pytest.mark.parametrize("n_pos,n_neg", hc.LINK_SIZES)
def test_link_loss_backward_per_element(gpu, n_pos, n_neg):
    """Random scores with 0, a denormal, 1.0 (and 1 - 2^-24 in neg) at the first, middle and last indices, upstream 3."""
    pos, neg = hc.link_grad_case(n_pos, n_neg)
    refs = hc.link_grad_ref(pos, neg, 3.0)
    g = torch.tensor(3.0, device=gpu)
    worst = 0.0
    for how in hc.alignments_of(n_pos, n_neg)[::2]:                  # aligned, neg + 4, adjacent
        p, n = _placed(pos, neg, how, gpu)
        for d, ref in zip(_hip.link_loss_backward(p, n, hc.EPS, g), refs):
            worst = max(worst, hc.relative(d, ref))
    line = hc.show("link loss backward {}+{}".format(n_pos, n_neg), rel=worst, bound=hc.LINK_GRAD_BOUND)
    assert worst <= hc.LINK_GRAD_BOUND, line


def test_link_loss_backward_under_autograd(gpu):
    pos, neg = hc.link_grad_case(524293, 174764)
    refs = hc.link_grad_ref(pos, neg, 3.0)
    p, n = pos.to(gpu).requires_grad_(True), neg.to(gpu).requires_grad_(True)
    utils.link_loss(p, n).backward(torch.tensor(3.0, device=gpu))
    rel = max(hc.relative(p.grad, refs[0]), hc.relative(n.grad, refs[1]))
    line = hc.show("link loss autograd", rel=rel, bound=hc.LINK_GRAD_BOUND)
    assert rel <= hc.LINK_GRAD_BOUND, line


@pytest.mark.parametrize("negative", (False, True), ids=("pos", "neg"))
def test_link_loss_logarithm_per_term(gpu, negative):
    """Lists of one score: the loss is one logarithm.  Its argument runs up to 1 - 2^-24, where a logarithm that is accurate
    only in absolute terms loses the whole value."""
    x = hc.log_points(negative)
    ref = hc.log_ref(x, negative)
    xs, none = x.to(gpu), torch.empty(0, device=gpu)
    # (xs[i:i + 1] sits on a 16-byte line for every fourth i only: both kernels take their share of the points)
    got = torch.stack([_hip.link_loss_forward(none, xs[i:i + 1], hc.EPS) if negative else
                       _hip.link_loss_forward(xs[i:i + 1], none, hc.EPS) for i in range(x.numel())]).cpu()
    near = ref < 1e-3
    rel, rel_near = hc.relative(got, ref), hc.relative(got[near], ref[near])
    line = hc.show("link loss, one term, " + ("neg" if negative else "pos"), rel=rel, near_1=rel_near, bound=hc.LOG_BOUND)
    assert rel <= hc.LOG_BOUND, line


# ---- 4. class loss ------------------------------------------------------------------------------------------------------
def _class_loss(score, labels, dev, sliced, upstream=2.0):
    """(loss, dscore) of utils.class_loss under autograd, the score contiguous or a column slice (ld > classes)."""
    n, classes = score.shape
    s = _sliced(score, 2, classes + 3, dev)[1] if sliced else score.to(dev)
    assert (_hip.ld(s) > classes) == (sliced and n > 1)
    s = s.detach().requires_grad_(True)
    loss = utils.class_loss(s, labels.to(dev))
    loss.backward(torch.tensor(upstream, device=dev))
    return loss.item(), s.grad.cpu()


@pytest.mark.parametrize("sliced", (False, True), ids=("contiguous", "sliced"))
@pytest.mark.parametrize("classes", hc.CLASS_C)
@pytest.mark.parametrize("n", hc.CLASS_N)
def test_class_loss_every_path(gpu, n, classes, sliced):
    """The four-in-flight loop (n > 3072), its second trip (n > 7168) and the tail loop on indicator scores; the gradient
    exactly 0 off the label column."""
    score, labels = hc.class_indicator(n, classes)
    ref = hc.class_ref(score, labels)
    loss, d = _class_loss(score, labels, gpu, sliced)
    dref = hc.class_grad_ref(score, labels, 2.0)
    rel, rel_d = abs(loss - ref) / ref, hc.relative(d, dref)         # (relative: exactly 0 wherever the reference is)
    line = hc.show("class loss n={} classes={} {}".format(n, classes, "sliced" if sliced else "contiguous"),
                   rel=rel, bound=hc.CLASS_BOUND, grad=rel_d, grad_bound=hc.CLASS_GRAD_BOUND)
    assert rel <= hc.CLASS_BOUND and rel_d <= hc.CLASS_GRAD_BOUND, line


@pytest.mark.parametrize("last", (-1, 8), ids=("last=-1", "last=classes"))
def test_class_loss_labels_outside_the_table(gpu, last):
    """-1 and `classes` among one thread's four rows in flight (rows 10 and 2058: the `bad` branch) and in the tail loop
    (row 8199, a spike): the loss is the valid rows' sum over n, the error word is raised once, their gradient rows are 0.
    Rows 1034 and 3082, the valid two of that thread's four, are made spikes: the `bad` branch must still count them."""
    score, labels = hc.class_indicator(8200, 8)
    score, labels = score.clone(), labels.clone()
    score[1034, labels[1034]], score[3082, labels[3082]] = 2.0 ** -5, 2.0 ** -7
    labels[10], labels[2058], labels[8199] = -1, 8, last
    ref = hc.class_ref(score, labels)
    try:
        _hip.raise_if_index_errors(gpu)                              # (whatever an earlier test left)
    except (IndexError, RuntimeError):
        pass
    loss, d = _class_loss(score, labels, gpu, sliced=True)
    with pytest.raises(IndexError):
        _hip.raise_if_index_errors(gpu)
    _hip.raise_if_index_errors(gpu)
    rel, rel_d = abs(loss - ref) / ref, hc.relative(d, hc.class_grad_ref(score, labels, 2.0))
    line = hc.show("class loss, labels outside", rel=rel, bound=hc.CLASS_BOUND, grad=rel_d, grad_bound=hc.CLASS_GRAD_BOUND)
    assert rel <= hc.CLASS_BOUND and rel_d <= hc.CLASS_GRAD_BOUND, line
    assert (d[[10, 2058, 8199]] == 0).all()


# ---- 5. merges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(11))
@pytest.mark.parametrize("rows,cols", hc.MERGE_SHAPES)
def test_merge_modes_against_the_header(gpu, rows, cols, mode):
    """gn_merge_f32 called directly, every operand a column slice of its own leading dimension, src2 with both zeros and
    denormals of both signs: sign(+-0) = 0 in modes 6 and 9, the masks of modes 5 and 10 closed at zeros and negatives."""
    dst0, src, src2 = hc.merge_operands(rows, cols)
    ref, mag = hc.merge_ref(mode, dst0, src, src2)
    big, dst = _sliced(dst0, 1, cols + 2, gpu)
    _, s = _sliced(src, 2, cols + 5, gpu)
    _, s2 = _sliced(src2, 3, cols + 7, gpu)
    assert torch.equal(s2.cpu().view(torch.int32), src2.view(torch.int32))          # signed zeros and denormals arrived
    _hip.merge(dst, s, mode, src2=s2)
    assert _beside_is_nan(big, 1, cols)
    y = dst.cpu()
    if mode in hc.MERGE_EXACT:
        assert torch.equal(y.double(), ref), "mode {} is not exact".format(mode)
        rho = 0.0
    else:
        rho = sc.componentwise(y, ref, mag)
    line = hc.show("merge mode {} {}x{}".format(mode, rows, cols), rho=rho, bound=hc.MERGE_BOUND)
    assert rho <= hc.MERGE_BOUND, line
    zero, closed = src2 == 0, src2 <= 0
    if mode in (6, 9):
        assert (y[zero] == 0).all()
    if mode in (5, 10):
        assert (y[closed] == 0).all()
