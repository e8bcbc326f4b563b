"""RGCNConv written from its definition with plain torch ops (no GPU, not a test module): the float64 reference of
tests/test_rgcn_conv_host.py and tests/test_gpu_rgcn_conv.py, the same formulation in fp32 (the "torch formulation" the GPU
bounds are taken from: index_select, bmm, index_add_), and the case builders.

RGCNConv of torch_geometric 1.4 / 1.5 (baselines/NC_baselines/RGCN_MLP.py:3,52-63): edges j -> i (row 0 the source) exactly as
listed, `edge_type` in any order,

    W_r    = sum_b att[r, b] basis[b]
    out[i] = sum_{e: dst_e = i} w_e x[src_e] W_{r(e)}  (+ x[i] root)  (+ bias),      w_e = edge_norm[e] or 1
"""
import functools
import math
import os
import re
import types

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def heavy_edges() -> int:
    """gn_layout::kBasisHeavyEdges, read where it is defined: destinations with more in-edges are walked by a workgroup"""
    with open(os.path.join(_ROOT, "gripnet_amd", "csrc", "layout_rgcn_basis.hpp")) as f:
        return int(re.search(r"constexpr\s+int\s+kBasisHeavyEdges\s*=\s*(\d+)\s*;", f.read()).group(1))


def forward(x, basis, att, root, bias, edge_index, edge_type, edge_norm=None, relu=False):
    """the definition in the dtype of x: every relation's table H_r = x W_r by one batched product, the edges' rows selected,
    scaled and added onto their destinations in list order"""
    B, fin, fout = basis.shape
    R, n = att.shape[0], x.shape[0]
    w = (att @ basis.reshape(B, fin * fout)).view(R, fin, fout)
    h = torch.bmm(x.unsqueeze(0).expand(R, n, fin), w).reshape(R * n, fout)
    msg = h.index_select(0, edge_type * n + edge_index[0])
    if edge_norm is not None:
        msg = msg * edge_norm.to(x.dtype)[:, None]
    out = torch.zeros((n, fout), dtype=x.dtype, device=x.device).index_add_(0, edge_index[1], msg)
    if root is not None:
        out = out + x @ root
    if bias is not None:
        out = out + bias
    return torch.relu(out) if relu else out


NAMES = ("out", "dx", "dbasis", "datt", "droot", "dbias")


def gradients(c, dtype, relu=True):
    """(out, dx, dbasis, datt, droot, dbias) of sum(out * upstream) in `dtype` by torch autograd (None for an absent parameter)"""
    leaf = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
    x, basis, att, root, bias = (leaf(t) for t in (c.x, c.basis, c.att, c.root, c.bias))
    out = forward(x, basis, att, root, bias, c.edge_index, c.edge_type, c.edge_norm, relu)
    leaves = [t for t in (x, basis, att, root, bias) if t is not None]
    g = iter(torch.autograd.grad((out * c.upstream.to(dtype)).sum(), leaves))
    return (out.detach(),) + tuple(None if t is None else next(g) for t in (x, basis, att, root, bias))


def errors(got, ref):
    """largest |got - ref| of every tensor (None for an absent one)"""
    return [None if r is None else float((g.double().cpu() - r.double()).abs().max()) for g, r in zip(got, ref)]


# ---- the graph ---------------------------------------------------------------------------------------------------------------
N, R = 300, 5
EMPTY_RELATION = 3
DEGREES = (0, 1, 3, 4, 5, 63, 64, 65, 129)           # exact in-degrees of nodes 0 .. 8; node 9: above the heavy threshold
HEAVY_NODE, HUB_SOURCE = 9, 10                       # node 10: as many OUT-edges (the heavy row of the reversed plan)


@functools.lru_cache(maxsize=None)
def graph(seed=7):
    """(edge_index [2, E], edge_type [E]) on N = 300 nodes: nodes 0 .. 8 have exactly DEGREES in-edges (four edges per matrix
    instruction, chunks of 64), node 9 kBasisHeavyEdges + 7; node 2's three in-edges hold a duplicate pair, node 3's four a
    self loop and node 9's a self loop and duplicates; node 10 sends kBasisHeavyEdges + 7 edges; 1,500 random edges among the
    nodes from 10 on (loops and duplicates occur).  Five relations, relation 3 without an edge, everything shuffled."""
    g = torch.Generator().manual_seed(seed)
    heavy = heavy_edges() + 7
    src, dst = [], []
    for node, deg in enumerate(DEGREES + (heavy,)):
        s = torch.randint(0, N, (deg,), generator=g)
        if node == 2:
            s[1] = s[0]                                                          # a duplicate edge
        if node in (3, HEAVY_NODE):
            s[0] = node                                                          # a self loop
        src.append(s)
        dst.append(torch.full((deg,), node, dtype=torch.long))
    src.append(torch.full((heavy,), HUB_SOURCE, dtype=torch.long))
    dst.append(torch.randint(HUB_SOURCE, N, (heavy,), generator=g))
    src.append(torch.randint(0, N, (1500,), generator=g))
    dst.append(torch.randint(HUB_SOURCE, N, (1500,), generator=g))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    et = torch.randint(0, R - 1, (ei.shape[1],), generator=g)
    et = et + (et >= EMPTY_RELATION).long()                                     # 0, 1, 2, 4
    order = torch.randperm(ei.shape[1], generator=g)
    return ei[:, order].contiguous(), et[order].contiguous()


def relation_mean_norm(edge_index, edge_type, n):
    """1 / c_{i,r}: the RGCN paper's normaliser, one over the number of in-edges of the destination under the edge's relation"""
    key = edge_type * n + edge_index[1]
    count = torch.zeros(int(edge_type.max()) * n + n if key.numel() else n, dtype=torch.float32).index_add_(0, key, torch.ones(key.numel()))
    return 1.0 / count.index_select(0, key)


NORMS = ("none", "random", "mean")
SHAPES = ((1, 1, 1), (16, 32, 16), (33, 7, 17), (128, 64, 64))                 # (in, out, bases)


@functools.lru_cache(maxsize=None)
def case(fin, fout, bases, norm="none", root=True, bias=True, seed=0):
    """A layer's operands on the CPU in fp32 on `graph()`: parameters (PyG's scale), x, an upstream gradient, edge_norm."""
    ei, et = graph()
    g = torch.Generator().manual_seed(2000 + seed)
    c = types.SimpleNamespace(edge_index=ei, edge_type=et, n=N, relations=R, fin=fin, fout=fout, bases=bases, norm=norm)
    bound = 1.0 / math.sqrt(bases * fin)
    uni = lambda *shape: (torch.rand(shape, generator=g) * 2 - 1) * bound
    c.basis, c.att = uni(bases, fin, fout), uni(R, bases)
    r, b = uni(fin, fout), uni(fout)
    c.root, c.bias = (r if root else None), (b if bias else None)
    c.x = torch.randn((N, fin), generator=g)
    c.upstream = torch.randn((N, fout), generator=g)
    w = torch.randn((ei.shape[1],), generator=g)
    w[::7] = 0.0                                                                # zeros among them (and about half are negative)
    c.edge_norm = {"none": None, "random": w, "mean": relation_mean_norm(ei, et, N), "ones": torch.ones(ei.shape[1])}[norm]
    return c


@functools.lru_cache(maxsize=None)
def reference(fin, fout, bases, norm="none", root=True, bias=True):
    """(case, float64 results, the fp32 torch formulation's largest errors against them) - computed once, shared, not modified"""
    c = case(fin, fout, bases, norm, root, bias)
    ref = gradients(c, torch.float64)
    return c, ref, errors(gradients(c, torch.float32), ref)


GENERAL = [(fin, fout, bases, norm, True, True) for (fin, fout, bases) in SHAPES for norm in NORMS] + [
    (16, 32, 16, "random", False, True), (16, 32, 16, "none", False, False), (33, 7, 17, "mean", True, False)]


def hand_case():
    """Five nodes, worked by hand: in = out = 1, two bases, two relations.
        x = (1, 2, 3, 4, 5);  basis = (1, 10);  att = ((1, 2), (0, 1))  =>  W_0 = 1 + 2 * 10 = 21,  W_1 = 10;  root = 100;  bias = 0.5
        edges (src -> dst, type, w):  0 -> 1 (0, 1),   2 -> 1 (1, 0.5),   1 -> 1 (0, 2) a loop,   4 -> 3 (1, 1) twice
      with edge_norm:
        out[0] = 100 + 0.5 = 100.5                                                (no in-edge: x root + bias)
        out[1] = 1 * 1 * 21 + 0.5 * 3 * 10 + 2 * 2 * 21 + 200 + 0.5 = 320.5
        out[2] = 300.5,   out[3] = 2 * (5 * 10) + 400 + 0.5 = 500.5,   out[4] = 500.5
      without:
        out[1] = 21 + 30 + 42 + 200.5 = 293.5,   the others as above
      and without root and bias, with edge_norm: (0, 120, 0, 100, 0)."""
    c = types.SimpleNamespace()
    c.x = torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0]], dtype=torch.float64)
    c.basis = torch.tensor([[[1.0]], [[10.0]]], dtype=torch.float64)
    c.att = torch.tensor([[1.0, 2.0], [0.0, 1.0]], dtype=torch.float64)
    c.root = torch.tensor([[100.0]], dtype=torch.float64)
    c.bias = torch.tensor([0.5], dtype=torch.float64)
    c.edge_index = torch.tensor([[0, 2, 1, 4, 4], [1, 1, 1, 3, 3]])
    c.edge_type = torch.tensor([0, 1, 0, 1, 1])
    c.edge_norm = torch.tensor([1.0, 0.5, 2.0, 1.0, 1.0], dtype=torch.float64)
    c.weighted = torch.tensor([[100.5], [320.5], [300.5], [500.5], [500.5]], dtype=torch.float64)
    c.plain = torch.tensor([[100.5], [293.5], [300.5], [500.5], [500.5]], dtype=torch.float64)
    c.bare = torch.tensor([[0.0], [120.0], [0.0], [100.0], [0.0]], dtype=torch.float64)
    return c
