"""The graph-attention layer written from its definition with plain torch ops (no GPU, not a test module): the float64
reference of tests/test_gat_host.py and tests/test_gpu_gat.py, the same formulation in fp32 (the "torch formulation" the
GPU bounds are taken from), the scales of the per-element bounds, and the case builders.

GATConv of torch_geometric 1.4 / 1.5 (baselines/NC_baselines/GAT.py:3,66-67): edges j -> i (row 0 the source), input loops
dropped, one loop per node added, duplicates kept; h = x W as [N, H, C]; z = h[i] . att[:, :C] + h[j] . att[:, C:];
alpha = softmax over the in-edges of i of leaky_relu(z) (1e-16 in the denominator); out = sum alpha h[j], heads
concatenated or averaged, plus bias.
"""
import math
import types

import torch
import torch.nn.functional as F

U = 2.0 ** -24
MAX_ROW = 128


def working_list(edge_index, n):
    keep = edge_index[0] != edge_index[1]
    loops = torch.arange(n, dtype=torch.long, device=edge_index.device)
    return torch.cat([edge_index[:, keep], torch.stack([loops, loops])], dim=1)


def parts(x, weight, att, edge_index, heads, slope=0.2, leaky=None, working=None):
    """(h [N, H, C], src, dst, z [E', H], alpha [E', H]) in the dtype and on the device of x.  `leaky`: another function in
    place of leaky_relu; `working`: the working list of `edge_index`, for a caller that keeps it."""
    n, f = x.shape[0], weight.shape[1]
    c = f // heads
    src, dst = working_list(edge_index, n) if working is None else working
    h = (x @ weight).view(n, heads, c)
    a_dst = (h * att[0, :, :c]).sum(-1)
    a_src = (h * att[0, :, c:]).sum(-1)
    z = a_dst.index_select(0, dst) + a_src.index_select(0, src)
    l = F.leaky_relu(z, slope) if leaky is None else leaky(z)   # derivative at 0: slope
    idx = dst[:, None].expand(-1, heads)
    m = torch.full((n, heads), -math.inf, dtype=x.dtype, device=x.device).scatter_reduce(0, idx, l.detach(), "amax", include_self=True)
    w = torch.exp(l - m.index_select(0, dst))                  # (the softmax does not depend on m: it carries no gradient)
    s = torch.zeros((n, heads), dtype=x.dtype, device=x.device).index_add_(0, dst, w)
    alpha = w / (s.index_select(0, dst) + 1e-16)
    return h, src, dst, z, alpha


def forward(x, weight, att, bias, edge_index, heads, concat=True, slope=0.2, relu=False, leaky=None, working=None):
    h, src, dst, _, alpha = parts(x, weight, att, edge_index, heads, slope, leaky, working)
    n, c = x.shape[0], h.shape[2]
    o = torch.zeros((n, heads, c), dtype=x.dtype, device=x.device).index_add_(0, dst, alpha[:, :, None] * h.index_select(0, src))
    out = o.reshape(n, heads * c) if concat else o.mean(dim=1)
    if bias is not None:
        out = out + bias
    return torch.relu(out) if relu else out


def gradients(x, weight, att, bias, edge_index, heads, concat, slope, relu, upstream, dtype):
    """(out, dx, dweight, datt, dbias) of sum(out * upstream) in `dtype` by torch autograd."""
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (x, weight, att)] + ([] if bias is None else [bias.to(dtype).clone().requires_grad_(True)])
    out = forward(leaves[0], leaves[1], leaves[2], leaves[3] if bias is not None else None, edge_index, heads, concat, slope, relu)
    g = torch.autograd.grad((out * upstream.to(dtype)).sum(), leaves)
    return (out.detach(),) + tuple(g) + ((None,) if bias is None else ())


def output_scale(x, weight, att, bias, edge_index, heads, concat=True, slope=0.2):
    """float64 scale of an output element: sum_e alpha |h|_j (1 + 2 dz) + |bias| with |h| = |x| |W| (what the product's own
    rounding is relative to) and dz the largest sum_c |h att| of the node's in-edges: a logit that moves by dz u moves every
    alpha of its softmax by at most 2 dz u of itself."""
    x, weight, att = x.double(), weight.double(), att.double()
    n, f = x.shape[0], weight.shape[1]
    c = f // heads
    _, src, dst, _, alpha = parts(x, weight, att, edge_index, heads, slope)
    habs = (x.abs() @ weight.abs()).view(n, heads, c)
    zabs = (habs * att[0, :, :c].abs()).sum(-1).index_select(0, dst) + (habs * att[0, :, c:].abs()).sum(-1).index_select(0, src)
    zmax = torch.zeros((n, heads), dtype=torch.float64).scatter_reduce(0, dst[:, None].expand(-1, heads), zabs, "amax", include_self=True)
    a = torch.zeros((n, heads, c), dtype=torch.float64).index_add_(0, dst, alpha[:, :, None] * habs.index_select(0, src))
    a = a * (1 + 2 * zmax[:, :, None])
    scale = a.reshape(n, f) if concat else a.mean(dim=1)
    return scale if bias is None else scale + bias.double().abs()


def gradient_scales(x, weight, att, bias, edge_index, heads, concat, slope, g):
    """float64 scales of (dx, dweight, datt, dbias): the sums of the absolute contributions, `g` the gradient that reaches the
    output before the bias (after the ReLU's mask)."""
    x, weight, att, g = x.double(), weight.double(), att.double(), g.double().abs()
    n, f = x.shape[0], weight.shape[1]
    c = f // heads
    h, src, dst, z, alpha = parts(x, weight, att, edge_index, heads, slope)
    h = h.abs()
    go = g.view(n, heads, c) if concat else (g / heads)[:, None, :].expand(n, heads, c)
    dot = (go.index_select(0, dst) * h.index_select(0, src)).sum(-1)
    idx = dst[:, None].expand(-1, heads)
    d = torch.zeros((n, heads), dtype=torch.float64).index_add_(0, dst, alpha * dot)
    dz = alpha * (dot + d.index_select(0, dst)) * torch.where(z > 0, 1.0, slope)
    da_dst = torch.zeros((n, heads), dtype=torch.float64).index_add_(0, dst, dz)
    da_src = torch.zeros((n, heads), dtype=torch.float64).index_add_(0, src, dz)
    dh = torch.zeros((n, heads, c), dtype=torch.float64).index_add_(0, src, alpha[:, :, None] * go.index_select(0, dst))
    dh = dh + da_dst[:, :, None] * att[0, :, :c].abs() + da_src[:, :, None] * att[0, :, c:].abs()
    datt = torch.cat([(da_dst[:, :, None] * h).sum(0), (da_src[:, :, None] * h).sum(0)], dim=1)[None]
    dh = dh.reshape(n, f)
    return dh @ weight.abs().t(), x.abs().t() @ dh, datt, (None if bias is None else g.sum(0))


def figure(got, ref, scale):
    """max |got - ref| / (u scale) over the elements of positive scale; elements of zero scale must be exactly the reference's."""
    got, ref, scale = got.double().cpu(), ref.double(), scale.double()
    zero = scale == 0
    assert bool((got[zero] == ref[zero]).all()), "an element of zero scale differs"
    if bool(zero.all()):
        return 0.0
    return float(((got - ref).abs()[~zero] / (U * scale[~zero])).max())


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def staircase(n=131):
    """node i has the i in-edges from nodes 0 .. i - 1: 8,515 edges, in-degrees across 63 / 64 / 65 and 127 / 128 / 129"""
    dst = torch.repeat_interleave(torch.arange(n), torch.arange(n))
    src = torch.cat([torch.arange(i) for i in range(n)]) if n > 1 else torch.zeros(0, dtype=torch.long)
    return torch.stack([src.long(), dst.long()]), n


def transposed(graph):
    ei, n = graph
    return torch.stack([ei[1], ei[0]]), n


def hubs(n=5100, degree=5000, seed=5):
    """node 0 has `degree` in-edges, node 1 `degree` out-edges; nodes n - 20 .. n - 1 are isolated; a few loops and duplicates"""
    g = torch.Generator().manual_seed(seed)
    others = torch.randperm(n - 22, generator=g)[:degree] + 2
    into = torch.stack([others, torch.zeros(degree, dtype=torch.long)])
    out = torch.stack([torch.ones(degree, dtype=torch.long), others])
    extra = torch.tensor([[2, 3, 3, 4, 0], [2, 4, 4, 4, 0]])            # loops at 2, 4 and 0; 3 -> 4 twice
    return torch.cat([into, out, extra], dim=1), n


def random_graph(n=2000, e=20000, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n, (2, e), generator=g), n                  # (loops and duplicates occur)


def small_graph():
    """12 nodes: loops (one node with two of them), a duplicate edge, two isolated nodes"""
    ei = torch.tensor([[0, 1, 2, 2, 3, 3, 3, 4, 5, 6, 7, 7, 8, 1, 9],
                       [1, 2, 0, 0, 3, 3, 4, 5, 5, 7, 6, 8, 9, 9, 0]])
    return ei, 12


def power_of_two_graph(n=40, seed=2):
    """every in-degree + 1 is a power of two (1, 2, 4, 8, 16 or 32 entries in the softmax)"""
    g = torch.Generator().manual_seed(seed)
    src, dst = [], []
    for i in range(n):
        k = (1 << (i % 6)) - 1
        others = torch.randperm(n - 1, generator=g)[:k]
        src.append(others + (others >= i).long())
        dst.append(torch.full((k,), i, dtype=torch.long))
    return torch.stack([torch.cat(src), torch.cat(dst)]), n


GRAPHS = {"staircase": staircase, "staircase_t": lambda: transposed(staircase()), "hubs": hubs, "random": random_graph,
          "small": small_graph, "single": lambda: (torch.zeros((2, 0), dtype=torch.long), 1)}


def case(graph, heads, channels, fin=7, concat=True, bias=True, seed=0, att_scale=1.0):
    """A layer's operands on the CPU in fp32: weight, att, bias (or None) - the same tables for every graph at one
    (heads, channels, fin, seed) - then x and an upstream gradient."""
    ei, n = GRAPHS[graph]() if isinstance(graph, str) else graph
    g = torch.Generator().manual_seed(1000 + seed)
    f = heads * channels
    c = types.SimpleNamespace(edge_index=ei, n=n, heads=heads, channels=channels, fin=fin, concat=concat, slope=0.2)
    c.weight = torch.randn((fin, f), generator=g) / math.sqrt(fin)
    c.att = torch.randn((1, heads, 2 * channels), generator=g) * att_scale
    both = torch.randn((f + channels,), generator=g)
    c.bias = (both[:f] if concat else both[f:]).clone() if bias else None
    c.x = torch.randn((n, fin), generator=g)
    c.upstream = torch.randn((n, f if concat else channels), generator=g)
    return c


def grid(shape, k, g, span=8):
    """values on a grid of 2^-k in [-span, span) 2^-k"""
    return torch.randint(-span, span, shape, generator=g).float() * 2.0 ** -k
