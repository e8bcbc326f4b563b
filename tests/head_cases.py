"""Helpers of the classifier-head and loss tests (tests/test_gpu_head.py on the GPU, tests/test_head_host.py on the host): the
inputs, the case lists, the float64 references and the measures.  Not a test module.

The training step's last stage feeds a logarithm, so its tests measure RELATIVE errors per element (a probability of 1e-6
may be 100 % wrong under any max-norm tolerance) and use inputs on which everything but the arithmetic under test is exact:

* logits that are the same bits in any summation order (`exact_logits`), shifted by 2048: what is left to measure is the
  softmax's own max / exp / sum / divide, and a row without max subtraction overflows;
* loss inputs whose terms are exactly 0 except at a few "spikes" (`link_indicator`, `class_indicator`) placed where an
  unrolled loop, a clamped load or a tail can drop or double an element: one spike more or less moves the loss by far more
  than the bound, whatever the length of the list.

Every figure is printed in multiples of u = 2^-24 (`show`).  Every input is generated on the CPU from a seed of its case, so
that the host module checks the very tensors the GPU module uses."""
import functools

import torch

import scale_cases as sc

U = sc.U
EPS = 1e-13                                                        # gripnet/utils.py:10
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))              # what a kernel gets: the entry points take eps as a C float
LIVE, DEAD_MAX = 2.0 ** -100, 2.0 ** -99                           # softmax: relative error above LIVE, 0 <= y <= DEAD_MAX below
DEAD_SHARE = 0.05


def show(what, **figures):
    """One line per case: every figure in multiples of u, the bound next to what it bounds."""
    return sc.show(what, figures)


# ---- 1. softmax on exact logits -----------------------------------------------------------------------------------------
FUSED_KN = ((1, 16), (15, 3), (16, 16), (17, 1), (30, 4), (127, 15), (128, 16), (129, 2), (288, 16), (2560, 16))
FUSED_M = (1, 2, 3, 4, 5, 63, 64, 65, 257)
GEMM_KN = ((2561, 16), (64, 17), (96, 20), (33, 63), (33, 64), (33, 65), (16, 130), (129, 200))
GEMM_M = (1, 3, 65)
ROWS_SHAPES = tuple((r, c) for r in (1, 5, 257) for c in (1, 2, 63, 64, 65, 130, 200))
ROWS_K = 33                                                        # the depth behind the logits handed to the in-place softmax


def scale_of(k):
    """W's power-of-two divisor: 16, and 128 from k = 2560 on (with 16 the spread of 2560 products leaves 47 % of the
    probabilities below 2^-100)."""
    return 128 if k >= 2560 else 16


def exact_logits(rows, k, n, seed, s=None):
    """(z [rows, k], W [k, n]) in fp32 with logits that are exact in any order: z integers in [-8, 8], W integers in [-4, 4]
    over s; z[:, 0] = 64 and W[0, :] = 32 add 2048 to every logit.  Every product and partial sum is a multiple of 1 / s
    below 2^24 / s (2048 s + 32 k < 2^24 for every k in use)."""
    s = scale_of(k) if s is None else s
    assert 2048 * s + 32 * k < 2 ** 24
    gen = torch.Generator().manual_seed(seed)
    z = torch.randint(-8, 9, (rows, k), generator=gen).float()
    w = torch.randint(-4, 5, (k, n), generator=gen).float() / s
    z[:, 0] = 64.0
    w[0, :] = 32.0
    return z, w


def softmax_bound(cols):
    """(12 + cols / 64) u: x - max is exact, expf up to 2 ulp per term, cols / 64 additions per lane and 6 shuffles of
    positive terms, a correctly rounded division."""
    return (12 + cols / 64) * U


def softmax_measure(y, ref64):
    """(largest relative error over the elements with ref64 >= 2^-100, share of the elements below); below, the output
    must lie in [0, 2^-99]; a non-finite output fails."""
    y = torch.as_tensor(y).detach().cpu().double()
    assert y.shape == ref64.shape, (y.shape, ref64.shape)
    assert torch.isfinite(y).all(), "non-finite values in the softmax"
    live = ref64 >= LIVE
    assert ((y[~live] >= 0) & (y[~live] <= DEAD_MAX)).all(), "a probability below 2^-100 came out negative or above 2^-99"
    rel = float(((y - ref64).abs()[live] / ref64[live]).max()) if bool(live.any()) else 0.0
    return rel, 1.0 - float(live.double().mean())


class HeadCase:
    """One class-score case: a table z (its first column 64), W, a node list with repeats and (from four entries on) one
    negative entry and one equal to the table's row count, the float64 logits of the listed rows (zeros for the two) and
    the mask of the rows inside the table."""

    def __init__(self, k, n, m):
        self.k, self.n, self.m = k, n, m
        self.table_rows = max(2, (m + 1) // 2)                      # (fewer rows than entries: repeats from m = 5 on)
        self.z, self.w = exact_logits(self.table_rows, k, n, seed=(k * 1009 + n) * 1009 + m)
        gen = torch.Generator().manual_seed(m * 7919 + k)
        self.nodes = torch.randint(0, self.table_rows, (m,), generator=gen)
        if m >= 4:
            self.nodes[m // 2] = -1
            self.nodes[m - 1] = self.table_rows
        self.inside = (self.nodes >= 0) & (self.nodes < self.table_rows)
        rows = self.z[self.nodes.clamp(0, self.table_rows - 1)] * self.inside.float().view(-1, 1)
        self.logits32 = rows @ self.w                                # exact: tests/test_head_host.py
        self.logits64 = rows.double() @ self.w.double()
        self.ref64 = torch.softmax(self.logits64, dim=1)

    def __repr__(self):
        return "k={} n={} m={}".format(self.k, self.n, self.m)


@functools.lru_cache(maxsize=None)
def head_case(k, n, m):
    return HeadCase(k, n, m)


FUSED_CASES = tuple((k, n, m) for k, n in FUSED_KN for m in FUSED_M)
GEMM_CASES = tuple((k, n, m) for k, n in GEMM_KN for m in GEMM_M)


@functools.lru_cache(maxsize=None)
def rows_logits(rows, cols):
    """Exact fp32 logits handed to the in-place softmax directly, with their float64 softmax."""
    z, w = exact_logits(rows, ROWS_K, cols, seed=rows * 1009 + cols)
    x = z @ w
    return x, torch.softmax(x.double(), dim=1)


# ---- 2. softmax backward ------------------------------------------------------------------------------------------------
BACKWARD_SHAPES = tuple((r, c) for r in (1, 5, 257) for c in (1, 8, 63, 64, 65, 200))


def backward_bound(cols):
    """(10 + cols / 64) u of p (|g| + sum p |g|): the dot product is cols / 64 additions per lane, 6 shuffles and the
    products' roundings, then one subtraction and one product."""
    return (10 + cols / 64) * U


def backward_depth(cols):
    """The depth behind the logits of a backward case: 288 up to 8 columns; 129 beyond, where the spread of 288 products
    over more columns leaves probabilities whose gradients are denormal (an absolute rounding error of 2^-150)."""
    return 288 if cols <= 8 else 129


@functools.lru_cache(maxsize=None)
def softmax_backward_case(rows, cols):
    """(probs, grad, ref64, mag64): probs the float64 softmax of exact logits rounded to fp32 (saturated rows: the logits
    behind them span up to ~75), grad with columns in 2^[-8, 8]; ref = p (g - sum p g) in float64 of these fp32 operands."""
    k = backward_depth(cols)
    z, w = exact_logits(rows, k, cols, seed=rows * 4099 + cols)
    p = torch.softmax(z.double() @ w.double(), dim=1).float()
    gen = torch.Generator().manual_seed(rows * 31 + cols)
    g = sc.mixed_scale(torch.randn(rows, cols, generator=gen), -8, 8, dim=1, gen=gen)
    p64, g64 = p.double(), g.double()
    ref = p64 * (g64 - (p64 * g64).sum(dim=1, keepdim=True))
    mag = p64 * (g64.abs() + (p64 * g64.abs()).sum(dim=1, keepdim=True))
    return p, g, ref, mag


# ---- 3. link loss -------------------------------------------------------------------------------------------------------
LINK_N = (1, 2, 3, 4, 5, 7, 8, 9, 524293, 2097159, 2228227)
LINK_BOUND = 16 * U                                                # <= 3 u per term, an fp32 chain of <= 6 per thread, then doubles
LINK_GRAD_BOUND = 4 * U                                            # -g / n, p + eps and the quotient: one rounding each
LOG_BOUND = 4 * U


def link_sizes(n):
    """The (n_pos, n_neg) of one size: the other list a third as long (np4 >> nn4: the clamped loads of the shorter list),
    its mirror, and either list empty."""
    return ((n, n // 3), (n // 3, n), (n, 0), (0, n))


LINK_SIZES = tuple(dict.fromkeys(sz for n in LINK_N for sz in link_sizes(n)))     # (n = 1, 2: the third is empty already)
ALIGNMENTS = ("aligned", "pos+4", "neg+4", "both+4", "adjacent")


def alignments_of(n_pos, n_neg):
    """"adjacent" (pos = buf[:E], neg = buf[E:]) only where E % 4 == 1 leaves the second list 4 bytes past a 16-byte line."""
    return tuple(a for a in ALIGNMENTS if a != "adjacent" or (n_pos % 4 == 1 and n_neg > 0))


def spike_indices(n):
    """Every index within 5 of 0, 4, 524288 k (k = 1..4), 4 (n // 4) and n: the start, the first vector, each unroll slot
    of the vector kernel and the second trip of its loop, the tail and the end."""
    idx = set()
    for a in (0, 4, 524288, 2 * 524288, 3 * 524288, 4 * 524288, 4 * (n // 4), n):
        idx.update(j for j in range(a - 5, a + 6) if 0 <= j < n)
    return torch.tensor(sorted(idx), dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def link_indicator(n, negative):
    """(scores, spike indices, float64 log terms of the spikes): pos is 1.0 and neg 0.0 (a term that is exactly 0 in
    fp32) except at the spikes, 2^-(1 + j % 32) in pos and 1 - 2^-(1 + j % 23) in neg."""
    x = torch.zeros(n) if negative else torch.ones(n)
    idx = spike_indices(n)
    if negative:
        x[idx] = 1.0 - torch.ldexp(torch.ones(idx.numel()), -(1 + idx % 23))
    else:
        x[idx] = torch.ldexp(torch.ones(idx.numel()), -(1 + idx % 32))
    return x, idx, link_terms(x[idx], negative)


def link_terms(x, negative):
    """log(pos + eps) or log(1 - neg + eps) in float64 of fp32 scores."""
    x = x.double()
    return torch.log((1.0 - x if negative else x) + EPS32)


def link_ref(pos, neg):
    """-mean(log(pos + eps)) - mean(log(1 - neg + eps)) in float64 of the fp32 scores; an empty list adds nothing."""
    lp = float(link_terms(pos, False).mean()) if pos.numel() else 0.0
    ln = float(link_terms(neg, True).mean()) if neg.numel() else 0.0
    return -lp - ln


@functools.lru_cache(maxsize=None)
def link_case(n_pos, n_neg):
    """(pos, neg, ref64) of the indicator inputs."""
    pos, neg = link_indicator(n_pos, False)[0], link_indicator(n_neg, True)[0]
    return pos, neg, link_ref(pos, neg)


def link_torch32(pos, neg):
    """The reference's expression in torch fp32 (GripNet-pose.py:140-142)."""
    eps = torch.tensor(EPS, dtype=torch.float32)
    lp = torch.log(pos + eps).mean() if pos.numel() else torch.zeros(())
    ln = torch.log(1.0 - neg + eps).mean() if neg.numel() else torch.zeros(())
    return float(-lp - ln)


DENORMAL = 2.0 ** -140


@functools.lru_cache(maxsize=None)
def link_grad_case(n_pos, n_neg):
    """(pos, neg) of the backward test: random scores in [1e-6, 1 - 1e-6]; at the first, middle and last indices of each
    list 0, a denormal and 1.0, in neg also 1 - 2^-24 (as many of them as the list has room for)."""
    gen = torch.Generator().manual_seed(n_pos * 3 + n_neg)
    out = []
    for n, vals in ((n_pos, (0.0, DENORMAL, 1.0)), (n_neg, (0.0, DENORMAL, 1.0, 1.0 - 2.0 ** -24))):
        x = torch.rand(n, generator=gen).clamp(1e-6, 1 - 1e-6)
        places = []
        for a in (0, n // 2, n - len(vals)):
            places += [j for j in range(a, a + len(vals)) if 0 <= j < n and j not in places]
        for t, j in enumerate(places):
            x[j] = vals[t % len(vals)]
        out.append(x)
    return tuple(out)


def link_grad_ref(pos, neg, upstream):
    """(dpos, dneg) in float64: -g / (n_pos (pos + eps)) and g / (n_neg (1 - neg + eps))."""
    dp = -upstream / (pos.numel() * (pos.double() + EPS32)) if pos.numel() else pos.double()
    dn = upstream / (neg.numel() * ((1.0 - neg.double()) + EPS32)) if neg.numel() else neg.double()
    return dp, dn


def log_points(negative):
    """The single scores of the logarithm test: a = p + eps (or 1 - q + eps) runs over 1 - 2^-k (k = 1..24), 2^-k
    (k = 1..40, what of it fp32's 1 - q can hold) and 100 seeded values in [0.9, 1)."""
    k24, k40 = torch.arange(1, 25), torch.arange(1, 41)
    gen = torch.Generator().manual_seed(11)
    near = 0.9 + 0.1 * torch.rand(100, generator=gen, dtype=torch.float64)
    a = torch.cat([1.0 - torch.ldexp(torch.ones(24, dtype=torch.float64), -k24),
                   torch.ldexp(torch.ones(40, dtype=torch.float64), -k40), near])
    return ((1.0 - a) if negative else a).float()


def log_ref(x, negative):
    """-log(a32) in float64, a32 the fp32 value of p + eps (or of 1 - q + eps) by the same two fp32 operations."""
    eps = torch.tensor(EPS, dtype=torch.float32)
    a32 = (1.0 - x + eps) if negative else (x + eps)
    return -torch.log(a32.double())


def relative(y, ref64):
    """max |y - ref64| / |ref64|; where ref64 == 0 the value must be 0."""
    y, ref64 = torch.as_tensor(y).detach().cpu().double().reshape(-1), torch.as_tensor(ref64).double().reshape(-1)
    assert y.shape == ref64.shape, (y.shape, ref64.shape)
    assert torch.isfinite(y).all(), "non-finite values in the output"
    dead = ref64 == 0
    assert (y[dead] == 0).all(), "a value whose reference is zero is not zero"
    if bool(dead.all()):
        return 0.0
    return float(((y - ref64).abs()[~dead] / ref64.abs()[~dead]).max())


# ---- 4. class loss ------------------------------------------------------------------------------------------------------
CLASS_N = (1, 5, 1023, 1025, 3072, 3073, 4096, 4097, 8200)
CLASS_C = (1, 2, 8, 40)
CLASS_BOUND = 8 * U                                                # logf, the sum in double
CLASS_GRAD_BOUND = 4 * U
OFF_LABEL = 1e-30                                                  # reading a wrong column costs log(1e-30 + eps) = -29.9 a row


def class_spike_rows(n):
    """Every row within 3 of 0, 1024, 3072, 4096, 8192 and n: the first thread, the slots of the four-in-flight loop, its
    second trip, the tail loop and the end."""
    idx = set()
    for a in (0, 1024, 3072, 4096, 8192, n):
        idx.update(j for j in range(a - 3, a + 4) if 0 <= j < n)
    return torch.tensor(sorted(idx), dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def class_indicator(n, classes):
    """(score [n, classes], labels): score[i, label_i] = 1.0 (a term that is exactly 0), 2^-(1 + i % 32) at the spike rows;
    every other column 1e-30."""
    gen = torch.Generator().manual_seed(n * 41 + classes)
    labels = torch.randint(0, classes, (n,), generator=gen)
    score = torch.full((n, classes), OFF_LABEL)
    score[torch.arange(n), labels] = 1.0
    rows = class_spike_rows(n)
    score[rows, labels[rows]] = torch.ldexp(torch.ones(rows.numel()), -(1 + rows % 32))
    return score, labels


def class_ref(score, labels):
    """-sum over the rows with a label inside the table of log(score[i, label_i] + eps), over ALL n rows, in float64."""
    n, classes = score.shape
    ok = (labels >= 0) & (labels < classes)
    picked = score[torch.arange(n)[ok], labels[ok]].double()
    return -float(torch.log(picked + EPS32).sum()) / n


def class_torch32(score, labels):
    """The drivers' expression in torch fp32 (GripNet-aminer.py:133)."""
    eps = torch.tensor(EPS, dtype=torch.float32)
    return float(-torch.log(score[torch.arange(score.shape[0]), labels] + eps).mean())


def class_grad_ref(score, labels, upstream):
    """dscore[i, label_i] = -g / (n (score + eps)) in float64 (zero elsewhere and in rows whose label is outside)."""
    n, classes = score.shape
    ok = (labels >= 0) & (labels < classes)
    d = torch.zeros(n, classes, dtype=torch.float64)
    rows = torch.arange(n)[ok]
    d[rows, labels[ok]] = -upstream / (n * (score[rows, labels[ok]].double() + EPS32))
    return d


# ---- 5. merges ----------------------------------------------------------------------------------------------------------
MERGE_SHAPES = ((1, 1), (7, 3), (300, 130))
MERGE_EXACT = (0, 1, 5, 6, 8, 9, 10)                               # copies, signs, masks and halvings: no rounding
MERGE_BOUND = 2 * U                                                # of the operands' absolute sum: modes 2, 3, 4, 7
SRC2_VALUES = (0.0, -0.0, DENORMAL, -DENORMAL, 1.5, -0.75, 3e-5, -2e4)


@functools.lru_cache(maxsize=None)
def merge_operands(rows, cols):
    """(dst, src, src2): finite values; src2 cycles through +0, -0, a denormal of each sign and ordinary values of each
    sign, starting at another of them in every row (a 1 x 1 case takes +0)."""
    gen = torch.Generator().manual_seed(rows * 131 + cols)
    dst, src = torch.randn(rows, cols, generator=gen), torch.randn(rows, cols, generator=gen)
    v = torch.tensor(SRC2_VALUES, dtype=torch.float32)
    i, c = torch.arange(rows).view(-1, 1), torch.arange(cols).view(1, -1)
    return dst, src, v[(3 * i + c) % len(SRC2_VALUES)].clone()


def merge_ref(mode, dst, src, src2):
    """(ref64, mag64) of include/gripnet_hip.h's formulas; mag64 is the operands' absolute sum."""
    d, s, r = dst.double(), src.double(), src2.double()
    sign = torch.sign(r)                                             # (0 at both zeros)
    zero = torch.zeros_like(s)
    ref = {0: s, 1: s.abs(), 2: (d + s.abs()) / 2, 3: (d + s.clamp(min=0)) / 2, 4: (d + s + r) / 3,
           5: torch.where(r > 0, s, zero), 6: s * sign, 7: s / 3, 8: s / 2, 9: s * sign / 2,
           10: torch.where(r > 0, s / 2, zero)}[mode]
    mag = {2: d.abs() + s.abs(), 3: d.abs() + s.abs(), 4: d.abs() + s.abs() + r.abs(), 7: s.abs()}.get(mode, s.abs())
    return ref, mag
