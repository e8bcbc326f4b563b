"""Helpers of the scale tests (tests/test_gpu_scales.py on the GPU, tests/test_scales_host.py on the host): the per-element
error measure, inputs whose rows or columns differ in scale, the power-of-two factors of the homogeneity checks, the
float64 references with their magnitudes, and a torch emulation of the bf16 term splits.  Not a test module.

The measure: for y = f(operands), rho = max over elements of |y - ref64| / mag64, where mag64 is the same float64
expression on the absolute values of every operand - the bound every backward-stable evaluation of f satisfies with a
constant of a few u (u = 2^-24) times the length of its sums, whatever the scales of single rows or columns.  A max-norm
cannot see an error in a small row next to a large one; rho can."""
import torch

from oracle import gripnet_oracle as orc

U = 2.0 ** -24                                                    # fp32's unit round-off: rho is printed in multiples of it

# With unit-scale operands and weights around 0.1 nothing comes near a denormal or an overflow at these factors, in fp32 or
# in any bf16 term (the third term of a split is 2^-16 of its value: 2^-76 at the smallest factor; fp32 and bf16 share the
# exponent range, normal down to 2^-126)
pow2_scales = (2.0 ** -60, 2.0 ** -20, 2.0 ** 20, 2.0 ** 40)


def componentwise(y, ref64, mag64):
    """rho = max |y - ref64| / mag64 over EVERY element: where mag64 == 0 the output must be exactly 0 (such an element
    counts as rho = 0), a non-finite output fails."""
    y = torch.as_tensor(y).detach().cpu().double()
    ref64, mag64 = ref64.detach().cpu().double(), mag64.detach().cpu().double()
    assert y.shape == ref64.shape == mag64.shape, (y.shape, ref64.shape, mag64.shape)
    assert torch.isfinite(y).all(), "non-finite values in the output"
    assert torch.isfinite(mag64).all() and (mag64 >= 0).all(), "the magnitude itself is not finite: choose other inputs"
    dead = mag64 == 0
    assert (y[dead] == 0).all(), "an output whose every contribution is zero is not exactly zero"
    if y.numel() == 0 or bool(dead.all()):
        return 0.0
    return float(((y - ref64).abs()[~dead] / mag64[~dead]).max())


def mixed_scale(t, lo, hi, dim, gen):
    """`t` with its rows (dim = 0) or columns (dim = 1) multiplied by 2^e, e a seeded uniform integer in [lo, hi]: exact
    in fp32 while nothing leaves the normal range."""
    e = torch.randint(lo, hi + 1, (t.shape[dim],), generator=gen)
    f = torch.ldexp(torch.ones(t.shape[dim], dtype=t.dtype), e)
    return t * (f.view(-1, 1) if dim == 0 else f.view(1, -1))


def show(what, rho):
    """One line per case with every figure in multiples of u (pytest -s shows it; a failing assertion shows it too)."""
    line = "rho[{}]: ".format(what) + "  ".join("{} {:.3g} u".format(k, v / U) for k, v in rho.items())
    print(line)
    return line


def bound(rho, c):
    """c * max(rho_exact..., rho_ref32): what the default is held to and the fast mode must exceed twice over."""
    return c * max(v for k, v in rho.items() if k.startswith("exact") or k == "ref32")


def check(what, rho, c):
    """rho_default <= c max(rho_exact, rho_ref32), no absolute floor; rho_fast (where the path has such a mode) above twice
    that: the bound would catch a dropped term on this very path and shape."""
    line = show(what, rho)
    assert rho["default"] <= bound(rho, c), line
    if "fast" in rho:
        assert rho["fast"] > 2 * bound(rho, c), "the two-term mode is not told from the default here: " + line


# ---- float64 references with their magnitudes ---------------------------------------------------------------------------
def _abs64(t):
    return None if t is None else t.double().abs()


def _f64(t):
    return None if t is None else t.double()


def gemm_ref(a, b, bias=None, addend=None):
    """(ref64, mag64) of a @ b (+ bias) (+ addend); a [.., m, k], b [.., k, n]."""
    ref, mag = a.double() @ b.double(), a.double().abs() @ b.double().abs()
    for t in (bias, addend):
        if t is not None:
            ref, mag = ref + t.double(), mag + t.double().abs()
    return ref, mag


def gcn_ref(x, w, bias, ei, ew=None, dtype=torch.float64):
    """The oracle's GCN layer in `dtype`, and (float64 only) its magnitude: the normalisation coefficients of non-negative
    edge weights are non-negative themselves."""
    cast = (lambda t: None if t is None else t.to(dtype))
    ref = orc.gcn_forward(cast(x), cast(w), cast(bias), ei, cast(ew))
    if dtype != torch.float64:
        return ref
    return ref, orc.gcn_forward(_abs64(x), _abs64(w), _abs64(bias), ei, _abs64(ew))


def bipartite_ref(x, w, bias, ei, n_target, ew=None, dtype=torch.float64):
    """The external layer's conv (closed form of the oracle), before ReLU and merge."""
    cast = (lambda t: None if t is None else t.to(dtype))
    sd = {"conv.weight": cast(w)}
    if bias is not None:
        sd["conv.bias"] = cast(bias)
    ref = orc.inter_forward_closed(sd, "", cast(x), ei, n_target, cast(ew))
    if dtype != torch.float64:
        return ref
    sd = {k: v.abs() for k, v in sd.items()}
    return ref, orc.inter_forward_closed(sd, "", _abs64(x), ei, n_target, _abs64(ew))


def rgcn_ref(x, ei, rl, sd, dtype=torch.float64):
    cast = (lambda t: None if t is None else t.to(dtype))
    ref = orc.rgcn_forward(cast(x), ei, rl, cast(sd["basis"]), cast(sd["att"]), cast(sd["root"]), cast(sd.get("bias")))
    if dtype != torch.float64:
        return ref
    return ref, orc.rgcn_forward(_abs64(x), ei, rl, _abs64(sd["basis"]), _abs64(sd["att"]), _abs64(sd["root"]), _abs64(sd.get("bias")))


def distmult_ref(z, ei, et, d, dtype=torch.float64):
    ref = orc.distmult(z.to(dtype), ei, et, d.to(dtype), sigmoid=False)
    if dtype != torch.float64:
        return ref
    return ref, orc.distmult(_abs64(z), ei, et, _abs64(d), sigmoid=False)


def class_ref(z, nodes, w, dtype=torch.float64):
    ref = orc.multiclass(z.to(dtype), nodes, w.to(dtype), softmax=False)
    if dtype != torch.float64:
        return ref
    return ref, orc.multiclass(_abs64(z), nodes, _abs64(w), softmax=False)


def grads_ref(fn, leaves, upstream, dtype=torch.float64):
    """Gradients of ``(fn(*leaves) * upstream).sum()`` under torch autograd in `dtype`; in float64 also their magnitudes: the
    same sum over |leaves| with |upstream| (every partial derivative of these multilinear layers is a sum of products of
    the operands, so autograd on the absolute values adds up the absolute value of every term)."""
    def run(ls, g):
        ls = [t.to(dtype).clone().requires_grad_(True) for t in ls]
        return torch.autograd.grad(fn(*ls), ls, g.to(dtype))
    ref = run(leaves, upstream)
    if dtype != torch.float64:
        return ref
    return ref, run([t.abs() for t in leaves], upstream.abs())


# ---- the bf16 term splits, emulated (include/gripnet_hip.h, "Arithmetic") ------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def split_terms(t, terms):
    """`t` (fp32) as `terms` bf16 terms, each the nearest bf16 of what the terms before it left (gemm.hip's split_terms)."""
    out, rest = [], t.clone()
    for _ in range(terms):
        out.append(_bf16(rest))
        rest = rest - out[-1]
    return out


# the products the two arithmetic modes keep (indices of the terms of a and of b): six for three terms, three for two
PRODUCTS = {3: ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)), 2: ((0, 0), (0, 1), (1, 0))}


def split_matmul(a, b, terms):
    """a @ b on `terms`-term splits with the header's product list, summed in float64: the error left is what the dropped
    products leave, before any fp32 accumulation."""
    ta, tb = split_terms(a, terms), split_terms(b, terms)
    return sum(ta[i].double() @ tb[j].double() for i, j in PRODUCTS[terms])


def random_graph(n, degree, gen, isolated=0, symmetric=False):
    """[2, ~n * degree] edges whose sources are drawn over all nodes (with rows of mixed scale every destination then sums
    neighbours from the whole exponent range); the last `isolated` nodes get no incoming edge; `symmetric`: both directions,
    no self loops (what the LDS-staged plans are built for)."""
    e = n * degree // (2 if symmetric else 1)
    ei = torch.stack([torch.randint(0, n, (e,), generator=gen), torch.randint(0, n - isolated, (e,), generator=gen)])
    if symmetric:
        ei = ei[:, ei[0] != ei[1]]
        ei = torch.cat([ei, ei.flip(0)], dim=1)
    return ei.long()
