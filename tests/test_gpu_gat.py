"""gripnet_amd.GATConv (csrc/gat.hip) on the GPU against the float64 formulation of tests/gat_cases.py, which
tests/test_gat_host.py pins by hand.

Bounds.  u = 2^-24.  Every bound has the form  |got - ref64| <= c * u * scale  per element, scale taken in float64:
  output     sum_e alpha |h|_j (1 + 2 dz) + |bias|,  |h| = |x| |W|,  dz = the largest sum_c |h att| of the node's in-edges (a logit
             that moves by dz u moves every alpha of its softmax by at most 2 dz u of itself)       (gat_cases.output_scale)
  gradients  the sums of the absolute contributions to dx, dweight, datt, dbias                    (gat_cases.gradient_scales)
  c = 4 t,   t the figure max |fp32 - ref64| / (u scale) that the fp32 torch formulation of gat_cases.py (index_select,
             scatter_reduce(amax), index_add_) reaches on the same inputs on the CPU; the factor 4 covers another summation
             tree, as in test_gpu_kge.py.  A graph of a dozen nodes or one node is no sample: it takes the larger of its own t and
             the t of the 2,000-node random graph on the same tables.
Elements of zero scale must be exactly the reference's.  The tests print every figure next to its bound (run with -s).

Measured on an MI355X, figure of the kernels / bound c = 4 t it was held to (t is taken on the CPU of the machine that runs the
test and moves with its BLAS: the same cases gave t(dx) = 2.66 on one host and 1.16 on another):
case                                  out           dx             dweight       datt          dbias
random 4x16 Fin 256 cat               0.02 / 0.05   2.05 / 4.64    0.12 / 0.41   0.09 / 0.24   1.01 / 1.52
random 1x32 Fin 64 mean               0.02 / 0.09   1.47 / 4.61    0.18 / 0.97   0.04 / 0.14   0.28 / 1.27
random 3x5 Fin 7 cat                  0.16 / 0.70   1.79 / 6.95    0.15 / 0.97   0.06 / 0.23   0.16 / 0.60
random 3x5 Fin 7 mean no bias         0.10 / 0.35   1.91 / 9.08    0.14 / 0.76   0.04 / 0.20   -
staircase 4x16 Fin 7 cat              0.07 / 0.77   0.81 / 13.10   0.41 / 4.28   0.33 / 2.35   0.42 / 1.83
staircase 3x5 Fin 7 mean              0.12 / 0.47   0.80 / 8.66    0.21 / 1.10   0.14 / 0.99   0.27 / 0.85
staircase_t 1x32 Fin 7 cat no bias    0.02 / 0.17   0.82 / 2.31    0.19 / 0.29   0.22 / 0.28   -
staircase_t 1x1 Fin 7 cat             0.03 / 0.14   0.57 / 2.77    0.20 / 1.30   0.14 / 1.34   0.00 / 2.88
hubs 8x8 Fin 7 cat                    0.36 / 2.29   0.88 / 4.84    0.08 / 1.43   0.04 / 0.30   1.21 / 1.89
hubs 4x16 Fin 7 mean                  0.09 / 1.22   1.39 / 78.83   0.06 / 0.56   0.04 / 0.60   0.21 / 1.12
hubs 3x5 Fin 7 cat no bias            0.16 / 4.71   3.94 / 70.01   0.07 / 2.18   0.05 / 0.71   -
random 1x128 Fin 7 cat                0.08 / 0.20   0.39 / 1.24    0.03 / 0.16   0.03 / 0.11   0.64 / 2.69
random 128x1 Fin 7 mean               0.13 / 0.44   0.81 / 3.31    0.07 / 1.80   0.18 / 0.30   0.04 / 0.14
random 8x16 Fin 7 cat                 0.13 / 0.56   0.42 / 1.95    0.12 / 1.59   0.05 / 0.22   0.63 / 2.52
small 4x16 Fin 256 cat                0.00 / 0.05   0.34 / 4.64    0.66 / 5.55   0.41 / 2.87   0.63 / 5.31
small 3x5 Fin 7 mean no bias          0.03 / 0.35   0.63 / 9.08    0.94 / 3.31   0.39 / 1.56   -
small 128x1 Fin 7 mean                0.08 / 0.44   0.31 / 3.31    0.97 / 5.39   1.17 / 3.99   0.11 / 0.45
single 4x16 Fin 256 cat               0.00 / 0.05   0.10 / 4.64    0.48 / 1.92   0.00 / 0.24   0.00 / 1.52
single 3x5 Fin 7 mean no bias         0.02 / 0.35   0.25 / 9.08    0.52 / 2.07   0.00 / 0.20   -
z across +-200                        0.16 / 0.35   1.23 / 7.03    0.08 / 0.38   0.06 / 0.33   0.26 / 1.03
equal logits below -1000              0.00 / 0.00   0.40 / 3.62    0.01 / 0.06   0.01 / 0.04   0.37 / 1.02
The closest: datt of the transposed staircase at 0.79 of its bound, dbias (the column sums of gn_grad_prologue_f32 against
torch's pairwise sum) at 0.64-0.66, dweight of the transposed staircase at 0.66, datt of the 128 heads at 0.60.
"""
import functools

import pytest
import torch

import gat_cases as gc
import gripnet_amd
from gripnet_amd import GATConv, _hip
from gripnet_amd import gat as gat_module

pytestmark = pytest.mark.gpu

NAN = float("nan")
SMALL = ("small", "single")


def _module(c, dev):
    conv = GATConv(c.fin, c.channels, heads=c.heads, concat=c.concat, negative_slope=c.slope, bias=c.bias is not None)
    sd = {"weight": c.weight, "att": c.att}
    if c.bias is not None:
        sd["bias"] = c.bias
    conv.load_state_dict(sd)
    return conv.to(dev)


def _run(c, dev, relu=True, x=None):
    """(out, dx, dweight, datt, dbias) of sum(out * upstream) through the module on the GPU"""
    conv = _module(c, dev)
    x = c.x.to(dev).requires_grad_(True) if x is None else x
    out = conv(x, c.edge_index.to(dev), _relu=relu)
    (out * c.upstream.to(dev)).sum().backward()
    return out.detach(), x.grad, conv.weight.grad, conv.att.grad, None if conv.bias is None else conv.bias.grad


@functools.lru_cache(maxsize=None)
def _figures(key):
    graph, heads, channels, fin, concat, bias, att_scale = key
    c = gc.case(graph, heads, channels, fin, concat, bias, att_scale=att_scale)
    args = (c.x, c.weight, c.att, c.bias, c.edge_index, heads, concat, c.slope, True, c.upstream)
    r = {"case": c}
    r["ref"] = gc.gradients(*args, torch.float64)
    got32 = gc.gradients(*args, torch.float32)
    g = c.upstream.double() * (r["ref"][0] > 0)
    r["scale"] = (gc.output_scale(c.x, c.weight, c.att, c.bias, c.edge_index, heads, concat, c.slope),) + \
        gc.gradient_scales(c.x, c.weight, c.att, c.bias, c.edge_index, heads, concat, c.slope, g)
    r["t"] = [0.0 if a is None else gc.figure(a, b, s) for a, b, s in zip(got32, r["ref"], r["scale"])]
    return r


def _reference(key):
    r = dict(_figures(key))
    if key[0] in SMALL:
        whole = _figures(("random",) + key[1:])
        r["t"] = [max(a, b) for a, b in zip(r["t"], whole["t"])]
    r["c"] = [4 * t for t in r["t"]]
    return r


NAMES = ("out", "dx", "dweight", "datt", "dbias")


def _check(r, got, what):
    for name, g, ref, scale, c, t in zip(NAMES, got, r["ref"], r["scale"], r["c"], r["t"]):
        if ref is None:
            assert g is None
            continue
        assert bool(torch.isfinite(g).all()), (what, name)
        fig = gc.figure(g, ref, scale)
        print("{}: {} {:.2f} (bound {:.2f}, torch fp32 {:.2f})".format(what, name, fig, c, t))
        assert fig <= c, (what, name, fig, c)


#        graph          H   C   Fin  concat bias  att scale
GENERAL = [
    ("random",      4,  16, 256, True,  True,  1.0),      # the reference's first layer
    ("random",      1,  32, 64,  False, True,  1.0),      # its second
    ("random",      3,  5,  7,   True,  True,  1.0),      # 15-float rows
    ("random",      3,  5,  7,   False, False, 1.0),
    ("staircase",   4,  16, 7,   True,  True,  1.0),
    ("staircase",   3,  5,  7,   False, True,  1.0),
    ("staircase_t", 1,  32, 7,   True,  False, 1.0),
    ("staircase_t", 1,  1,  7,   True,  True,  1.0),
    ("hubs",        8,  8,  7,   True,  True,  1.0),
    ("hubs",        4,  16, 7,   False, True,  1.0),
    ("hubs",        3,  5,  7,   True,  False, 1.0),
    ("random",      1,  128, 7,  True,  True,  1.0),      # the last admitted width, one head
    ("random",      128, 1, 7,   False, True,  1.0),      # ... and as 128 heads: two units per lane
    ("random",      8,  16, 7,   True,  True,  1.0),
    ("small",       4,  16, 256, True,  True,  1.0),
    ("small",       3,  5,  7,   False, False, 1.0),
    ("small",       128, 1, 7,   False, True,  1.0),
    ("single",      4,  16, 256, True,  True,  1.0),
    ("single",      3,  5,  7,   False, False, 1.0),
]


@pytest.mark.parametrize("key", GENERAL, ids=lambda k: "{}-{}x{}-{}-{}{}".format(k[0], k[1], k[2], k[3], "cat" if k[4] else "mean", "" if k[5] else "-nobias"))
def test_general_cases(gpu, key):
    r = _reference(key)
    _check(r, _run(r["case"], gpu), str(key))


def test_single_node_is_h_plus_bias(gpu):
    c = gc.case("single", 4, 16, 256)
    conv = _module(c, gpu)
    with torch.no_grad():
        out = conv(c.x.to(gpu), c.edge_index.to(gpu))
    h = torch.empty((1, 64), device=gpu)
    _hip.gemm(c.x.to(gpu), conv.weight.detach(), h)
    assert torch.equal(out, h + conv.bias.detach())


def test_first_refused_width(gpu):
    h = torch.zeros((4, 129), device=gpu)
    plan = gat_module.gat_plan(torch.zeros((2, 1), dtype=torch.long, device=gpu), 4)
    with pytest.raises(ValueError, match="at most 128"):
        _hip.gat_forward(plan, h, torch.zeros((1, 1, 258), device=gpu), 1, 0.2, None, True, False, torch.zeros((4, 129), device=gpu))
    with pytest.raises(ValueError, match="at most 128"):
        GATConv(8, 129)


# ---- exact cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,channels,concat", [(4, 16, True), (4, 16, False), (3, 5, True), (1, 32, True)])
def test_zero_att_is_the_exact_mean(gpu, heads, channels, concat):
    """att = 0, every in-degree + 1 a power of two, x and W on a grid of 2^-3: h, the sums and the divisions are exact"""
    ei, n = gc.power_of_two_graph()
    g = torch.Generator().manual_seed(9)
    c = gc.case((ei, n), heads, channels, 7, concat, True)
    c.x, c.weight, c.bias = gc.grid((n, 7), 3, g), gc.grid((7, heads * channels), 3, g), gc.grid(c.bias.shape, 3, g)
    c.att = torch.zeros_like(c.att)
    ref = gc.forward(c.x.double(), c.weight.double(), c.att.double(), c.bias.double(), ei, heads, concat)
    assert torch.equal(ref.float().double(), ref)                              # (the reference itself is exact in fp32)
    with torch.no_grad():
        out = _module(c, gpu)(c.x.to(gpu), ei.to(gpu))
    assert torch.equal(out.cpu(), ref.float())


def test_one_hot_attention_needs_the_max_subtraction(gpu):
    """a_src = 256 * node id: the best in-edge of a node leads the rest by 256 or more, alpha is exactly one-hot, the output
    row is the winner's h - and exp(256 * id) overflows unless the maximum is subtracted first"""
    ei, n = gc.random_graph(200, 1500, seed=8)
    c = gc.case((ei, n), 1, 4, 2, True, False)
    c.x = torch.stack([torch.arange(n, dtype=torch.float32), torch.zeros(n)], dim=1)
    c.weight = torch.tensor([[1.0, 0.5, -0.25, 0.125], [0.0, 0.0, 0.0, 0.0]])
    c.att = torch.tensor([[[0.0, 0.0, 0.0, 0.0, 256.0, 0.0, 0.0, 0.0]]])
    src, dst = gc.working_list(ei, n)
    winner = torch.zeros(n, dtype=torch.long).scatter_reduce(0, dst, src, "amax", include_self=True)
    ref = gc.forward(c.x.double(), c.weight.double(), c.att.double(), None, ei, 1).float()
    assert torch.equal(ref, (c.x @ c.weight)[winner])
    with torch.no_grad():
        out = _module(c, gpu)(c.x.to(gpu), ei.to(gpu))
    assert torch.equal(out.cpu(), ref)


# ---- saturation ----------------------------------------------------------------------------------------------------------
def test_saturated_logits(gpu):
    base = gc.case("random", 4, 16, 7)
    z = gc.parts(base.x.double(), base.weight.double(), base.att.double(), base.edge_index, 4)[3]
    scale = 200.0 / float(z.abs().max())
    key = ("random", 4, 16, 7, True, True, scale)
    r = _reference(key)
    z = gc.parts(r["case"].x.double(), r["case"].weight.double(), r["case"].att.double(), base.edge_index, 4)[3]
    assert float(z.max()) > 150 and float(z.min()) < -150
    _check(r, _run(r["case"], gpu), "z across +-200")


def test_equal_and_hugely_negative_logits(gpu):
    """only the target's half of att is set, and to -300: every logit of a node is the same, far below zero"""
    c = gc.case("random", 4, 16, 7)
    c.x, c.weight = c.x.abs() + 0.5, c.weight.abs()
    c.att = torch.cat([torch.full((1, 4, 16), -300.0), torch.zeros((1, 4, 16))], dim=2)
    args = (c.x, c.weight, c.att, c.bias, c.edge_index, 4, True, c.slope, True, c.upstream)
    ref = gc.gradients(*args, torch.float64)
    z = gc.parts(c.x.double(), c.weight.double(), c.att.double(), c.edge_index, 4)[3]
    assert float(z.max()) < -1000
    got32 = gc.gradients(*args, torch.float32)
    g = c.upstream.double() * (ref[0] > 0)
    scales = (gc.output_scale(c.x, c.weight, c.att, c.bias, c.edge_index, 4, True, c.slope),) + \
        gc.gradient_scales(c.x, c.weight, c.att, c.bias, c.edge_index, 4, True, c.slope, g)
    t = [gc.figure(a, b, s) for a, b, s in zip(got32, ref, scales)]
    _check({"ref": ref, "scale": scales, "t": t, "c": [4 * v for v in t]}, _run(c, gpu), "equal logits below -1000")


# ---- views, repeatability, plans -----------------------------------------------------------------------------------------
def test_views_of_nan_matrices(gpu):
    """x, h and the output as column views of NaN-filled matrices: nothing beside a view is read or written"""
    c = gc.case("random", 3, 5, 7)
    want = _run(c, gpu)
    big = torch.full((c.n, 16), NAN, device=gpu)
    big[:, 5:12] = c.x.to(gpu)
    x = big[:, 5:12].detach().requires_grad_(True)
    got = _run(c, gpu, x=x)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    conv = _module(c, gpu)
    plan = gat_module.gat_plan(c.edge_index.to(gpu), c.n)
    hbig, obig = torch.full((c.n, 24), NAN, device=gpu), torch.full((c.n, 21), NAN, device=gpu)
    _hip.gemm(c.x.to(gpu), conv.weight.detach(), hbig[:, 3:18])
    _hip.gat_forward(plan, hbig[:, 3:18], conv.att.detach(), 3, 0.2, conv.bias.detach(), True, True, obig[:, 1:16])
    assert torch.equal(obig[:, 1:16], want[0])
    assert bool(torch.isnan(obig[:, :1]).all()) and bool(torch.isnan(obig[:, 16:]).all())
    assert bool(torch.isnan(hbig[:, :3]).all()) and bool(torch.isnan(hbig[:, 18:]).all())


@pytest.mark.parametrize("heads,channels,concat", [(4, 16, True), (3, 5, False)])
def test_two_calls_give_the_same_bits(gpu, heads, channels, concat):
    c = gc.case("hubs", heads, channels, 7, concat)
    a, b = _run(c, gpu), _run(c, gpu)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_plan_is_reused_and_rebuilt_after_an_edit(gpu):
    c = gc.case("small", 4, 16, 7)
    ei = c.edge_index.to(gpu)
    plan = gat_module.gat_plan(ei, c.n)
    assert gat_module.gat_plan(ei, c.n) is plan
    conv = _module(c, gpu)
    with torch.no_grad():
        before = conv(c.x.to(gpu), ei)
        assert gat_module.gat_plan(ei, c.n) is plan
        ei[0, 0] = 5                                                           # in place: the tensor's version moves
        after = conv(c.x.to(gpu), ei)
    assert gat_module.gat_plan(ei, c.n) is not plan
    assert not torch.equal(before, after)
    ref = gc.forward(c.x.double(), c.weight.double(), c.att.double(), c.bias.double(), ei.cpu(), 4)
    assert torch.allclose(after.cpu().double(), ref, rtol=1e-4, atol=1e-5)


def test_node_id_out_of_range_as_for_mygcn(gpu):
    ei = torch.tensor([[0, 1, 4], [1, 2, 0]], device=gpu)
    x = torch.zeros((4, 8), device=gpu)
    with pytest.raises(IndexError):
        gripnet_amd.myGCN(8, 4).to(gpu)(x, ei)
    with pytest.raises(IndexError):
        GATConv(8, 4).to(gpu)(x, ei)


def test_captured_step_replays_the_eager_bits(gpu):
    c = gc.case("random", 4, 16, 256)
    conv = _module(c, gpu)
    ei, up = c.edge_index.to(gpu), c.upstream.to(gpu)
    x = c.x.to(gpu).requires_grad_(True)

    def step():
        for p in (x, conv.weight, conv.att, conv.bias):
            p.grad = None
        out = conv(x, ei, _relu=True)
        (out * up).sum().backward()
        return out.detach(), x.grad, conv.weight.grad, conv.att.grad, conv.bias.grad

    eager = [t.clone() for t in step()]
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


def test_memory_held_is_linear_in_nodes_and_edges(gpu):
    """N = 100,000, E = 500,000, 4 x 16: what a training step allocates at its peak stays a few [N, H C] and [N, H] arrays -
    an [E', H C] buffer alone would be 154 MB"""
    n, e, f = 100_000, 500_000, 64
    g = torch.Generator().manual_seed(4)
    ei = torch.randint(0, n, (2, e), generator=g).to(gpu)
    conv = GATConv(32, 16, heads=4).to(gpu)
    x = torch.randn((n, 32), generator=g).to(gpu).requires_grad_(True)
    gat_module.gat_plan(ei, n, transpose=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = conv(x, ei, _relu=True)
    held = torch.cuda.memory_allocated() - base
    out.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    row = 4 * n * f
    print("held after the forward {:.1f} MB, peak of the step {:.1f} MB ([N, H C] is {:.1f} MB)".format(held / 2 ** 20, peak / 2 ** 20, row / 2 ** 20))
    assert held <= 4 * row                 # h, o, out and the four [N, H] arrays (x itself is the caller's)
    assert peak <= 8 * row                 # + g masked, dh, dx, pack, the logit gradients: ~6.2; one [E', H C] buffer more is 6 rows more
    assert bool(torch.isfinite(x.grad).all())
