"""gripnet_amd.RGCNConv (the weighted instantiation of csrc/rgcn_basis.hip, GN_RGCN_SUM) and gripnet_amd.GCNConv on the GPU
against the float64 formulation of tests/rgcn_conv_cases.py, which tests/test_rgcn_conv_host.py pins by hand.

Bounds.  The output and every gradient (dx, dbasis, datt, droot, dbias of sum(out * upstream) behind the fused ReLU) are held
per element:  max |got - ref64| <= 4 t,  t = max |fp32 - ref64| of the fp32 torch formulation of rgcn_conv_cases.py
(index_select, bmm, index_add_) on the same case on the CPU; the factor 4 covers another summation tree, as in
test_gpu_kge.py and test_gpu_gat.py.  test_rgcn_conv_host.py checks that no t is zero.  The tests print every figure next to
its bound (run with -s).

One graph serves the cases (rgcn_conv_cases.graph): 300 nodes, in-degrees 0, 1, 3, 4, 5, 63, 64, 65, 129 and one above
gn_layout::kBasisHeavyEdges, a source with as many out-edges (the reversed plan's heavy row), duplicates, self loops, five
relations of which one is empty, types shuffled.

edge_norm = ones against edge_norm = None: the OUTPUT is the same bits at every shape (both run the general kernel's
accumulation, att * 1.0f is att).  The gradients are not compared bit for bit: without edge_norm the backward takes the
relational layer's own routes (the reversed plan's destination-major or LDS kernel, the fused weight gradient), with it
the weighted general kernels - other summation trees; both are held to the bounds above.

Measured on an MI355X, largest |got - ref64| / the bound 4 t it was held to, in units of 1e-7 (t is taken on the CPU of the
machine that runs the test and moves with its BLAS):
case                                    out             dx              dbasis          datt            droot           dbias
1, 1, 1, none                           5.8 / 398.8     4.4 / 64.2      60.2 / 293.1    121.3 / 203.7   23.9 / 114.6    3.9 / 53.6
1, 1, 1, random                         7.2 / 25.3      4.7 / 20.2      0.8 / 302.1     32.6 / 363.4    6.7 / 141.4     18.4 / 79.0
1, 1, 1, mean                           2.1 / 7.3       2.7 / 37.1      0.4 / 36.5      30.1 / 59.6     2.1 / 46.6      6.6 / 7.2
16, 32, 16, none                        9.4 / 22.7      3.6 / 8.8       13.3 / 114.1    68.9 / 539.9    51.0 / 335.0    20.2 / 82.7
16, 32, 16, random                      3.5 / 15.6      9.2 / 10.8      14.6 / 71.8     80.1 / 333.6    45.6 / 377.0    22.9 / 91.8
16, 32, 16, mean                        0.7 / 2.9       4.2 / 6.6       6.1 / 79.9      33.8 / 226.3    60.9 / 512.7    23.2 / 133.4
33, 7, 17, none                         1.4 / 5.1       0.9 / 2.2       18.6 / 111.1    117.8 / 225.0   41.5 / 538.2    12.6 / 52.9
33, 7, 17, random                       1.5 / 4.1       0.4 / 1.7       8.0 / 68.0      71.4 / 269.9    56.5 / 404.8    9.9 / 38.8
33, 7, 17, mean                         0.8 / 3.3       0.3 / 1.2       4.2 / 65.9      26.8 / 161.4    45.3 / 658.5    11.0 / 67.0
128, 64, 64, none                       3.1 / 5.6       1.4 / 1.7       12.2 / 36.8     185.3 / 939.4   67.7 / 561.5    30.6 / 125.7
128, 64, 64, random                     3.0 / 5.0       1.0 / 1.4       5.4 / 18.8      151.4 / 851.5   79.2 / 438.4    16.3 / 147.0
128, 64, 64, mean                       1.3 / 5.6       0.8 / 1.5       3.9 / 14.5      76.6 / 499.7    67.5 / 522.6    21.8 / 159.6
16, 32, 16, random no root              3.5 / 14.9      4.7 / 11.8      15.5 / 73.0     81.8 / 454.1    -               43.0 / 133.4
16, 32, 16, none no root no bias        5.5 / 21.3      1.4 / 8.7       22.2 / 102.5    52.1 / 453.6    -               -
33, 7, 17, mean no bias                 0.8 / 3.2       0.4 / 0.9       4.5 / 34.0      26.8 / 104.9    53.0 / 492.1    -
ones 1, 1, 1                            5.8 / 398.8     4.4 / 64.2      3.0 / 293.1     31.3 / 203.7    23.9 / 114.6    3.9 / 53.6
ones 16, 32, 16                         9.4 / 22.7      8.8 / 8.8       14.8 / 114.1    71.5 / 539.9    51.0 / 335.0    20.2 / 82.7
ones 33, 7, 17                          1.4 / 5.1       0.9 / 2.2       10.0 / 111.1    84.4 / 225.0    41.5 / 538.2    12.6 / 52.9
ones 128, 64, 64                        3.1 / 5.6       1.4 / 1.7       7.5 / 36.8      167.1 / 939.4   67.7 / 561.5    30.6 / 125.7
column slice none                       1.4 / 5.1       0.9 / 2.2       18.6 / 111.1    117.8 / 225.0   41.5 / 538.2    12.6 / 52.9
column slice random                     1.5 / 4.1       0.4 / 1.7       8.0 / 68.0      71.4 / 269.9    56.5 / 404.8    9.9 / 38.8
sorted list                             3.5 / 15.6      9.2 / 10.8      14.6 / 71.8     80.1 / 333.6    45.6 / 377.0    22.9 / 91.8
The closest: dx of ones 16, 32, 16 at 0.99 of its bound; dbias of 1, 1, 1, mean at 0.91 of its bound; dx of sorted list at 0.85 of its bound; dx of 16, 32, 16, random at 0.85 of its bound.
"""
import os
import re
import subprocess
import sys

import pytest
import torch

import rgcn_conv_cases as rc
import gripnet_amd
from gripnet_amd import GCNConv, RGCNConv
from gripnet_amd import pyg_convs

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(c, dev):
    conv = RGCNConv(c.fin, c.fout, c.relations, c.bases, root_weight=c.root is not None, bias=c.bias is not None)
    sd = {"basis": c.basis, "att": c.att}
    if c.root is not None:
        sd["root"] = c.root
    if c.bias is not None:
        sd["bias"] = c.bias
    conv.load_state_dict(sd)
    return conv.to(dev)


def _operands(c, dev):
    return c.edge_index.to(dev), c.edge_type.to(dev), None if c.edge_norm is None else c.edge_norm.to(dev)


def _run(c, dev, relu=True, x=None, graph=None):
    """(out, dx, dbasis, datt, droot, dbias) of sum(out * upstream) through the module on the GPU"""
    conv = _module(c, dev)
    ei, et, w = _operands(c, dev) if graph is None else graph
    x = c.x.to(dev).requires_grad_(True) if x is None else x
    out = conv(x, ei, et, w, _relu=relu)
    (out * c.upstream.to(dev)).sum().backward()
    grad = lambda p: None if p is None else p.grad
    return out.detach(), x.grad, conv.basis.grad, conv.att.grad, grad(conv.root), grad(conv.bias)


def _check(key, got, what=None):
    c, ref, t = rc.reference(*key)
    what = str(key) if what is None else what
    for name, g, r, e in zip(rc.NAMES, got, ref, t):
        if r is None:
            assert g is None, (what, name)
            continue
        assert bool(torch.isfinite(g).all()), (what, name)
        err = float((g.double().cpu() - r).abs().max())
        print("{}: {} {:.3e} (bound {:.3e} = 4 x torch fp32 {:.3e})".format(what, name, err, 4 * e, e))
        assert err <= 4 * e, (what, name, err, 4 * e)


def _id(k):
    return "{}-{}-{}-{}{}{}".format(k[0], k[1], k[2], k[3], "" if k[4] else "-noroot", "" if k[5] else "-nobias")


@pytest.mark.parametrize("key", rc.GENERAL, ids=_id)
def test_general_cases(gpu, key):
    c = rc.case(*key)
    _check(key, _run(c, gpu))


@pytest.mark.parametrize("fin,fout,bases,why", [(129, 8, 4, "input"), (8, 129, 4, "output"), (8, 8, 65, "bases")])
def test_first_refused_size_of_the_weighted_path(gpu, fin, fout, bases, why):
    ei, et = (t.to(gpu) for t in rc.graph())
    conv = RGCNConv(fin, fout, rc.R, bases).to(gpu)
    x = torch.zeros((rc.N, fin), device=gpu)
    with pytest.raises(ValueError, match="64 bases and 128"):
        conv(x, ei, et, torch.ones(ei.shape[1], device=gpu))
    rel = pyg_convs.relational_list(ei, et, rc.N, rc.R)
    assert rel.plan.weighted_supported(128, 128, 64)
    if why != "output":                                                         # (the output width binds in the backward: dx is the layer reversed)
        assert not rel.plan.weighted_supported(fin, fout, bases)
    with torch.no_grad():                                                       # without edge_norm the size is served
        out = conv(x, ei, et)
    assert tuple(out.shape) == (rc.N, fout) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: "{}-{}-{}".format(*s))
def test_edge_norm_of_ones_gives_the_bits_of_none(gpu, shape):
    c, ones = rc.case(*shape, "none"), rc.case(*shape, "ones")
    conv = _module(c, gpu)
    ei, et, _ = _operands(c, gpu)
    with torch.no_grad():
        a = conv(c.x.to(gpu), ei, et, _relu=True)
        b = conv(c.x.to(gpu), ei, et, ones.edge_norm.to(gpu), _relu=True)
    assert torch.equal(a, b)
    _check(shape + ("none", True, True), _run(ones, gpu), "ones {}".format(shape))


def test_no_vector_of_ones_without_edge_norm(gpu):
    """edge_norm=None: the unweighted instantiation runs and the plan builds no position list (4 bytes per edge)"""
    c = rc.case(16, 32, 16, "none")
    ei, et = (t.clone() for t in _operands(c, gpu)[:2])
    _run(c, gpu, graph=(ei, et, None))
    rel = pyg_convs.relational_list(ei, et, rc.N, rc.R)
    assert not rel.plan._has_pos and not rel.plan.reversed_plan()._has_pos
    _run(c, gpu, graph=(ei, et, torch.ones(ei.shape[1], device=gpu)))
    assert pyg_convs.relational_list(ei, et, rc.N, rc.R) is rel
    assert rel.plan._has_pos and rel.plan.reversed_plan()._has_pos


@pytest.mark.parametrize("norm", ["none", "random"])
def test_x_as_a_column_slice_of_a_nan_matrix(gpu, norm):
    key = (33, 7, 17, norm, True, True)
    c = rc.case(*key)
    big = torch.full((c.n, 40), NAN, device=gpu)
    big[:, 3:36] = c.x.to(gpu)
    x = big[:, 3:36].detach().requires_grad_(True)
    assert not x.is_contiguous()
    got = _run(c, gpu, x=x)
    _check(key, got, "column slice {}".format(norm))
    assert torch.equal(got[0], _run(c, gpu)[0])
    assert bool(torch.isnan(big[:, :3]).all()) and bool(torch.isnan(big[:, 36:]).all())


def test_a_sorted_list_needs_no_permutation(gpu):
    key = (16, 32, 16, "random", True, True)
    c = rc.case(*key)
    order = torch.sort(c.edge_type, stable=True).indices
    graph = (c.edge_index[:, order].contiguous().to(gpu), c.edge_type[order].contiguous().to(gpu), c.edge_norm[order].contiguous().to(gpu))
    assert pyg_convs.relational_list(graph[0], graph[1], rc.N, rc.R).perm is None
    got = _run(c, gpu, graph=graph)
    _check(key, got, "sorted list")
    for a, b in zip(got, _run(c, gpu)):                                         # the stable sort gives this very list
        assert torch.equal(a, b)


def test_edge_type_modified_in_place_plans_again(gpu):
    key = (16, 32, 16, "random", True, True)
    c = rc.case(*key)
    ei, et, w = _operands(c, gpu)
    et = et.clone()
    conv = _module(c, gpu)
    rel = pyg_convs.relational_list(ei, et, rc.N, rc.R)
    with torch.no_grad():
        before = conv(c.x.to(gpu), ei, et, w)
        assert pyg_convs.relational_list(ei, et, rc.N, rc.R) is rel
        et[:100] = (et[:100] + 1) % 3                                           # in place: the tensor's version moves
        after = conv(c.x.to(gpu), ei, et, w)
    assert pyg_convs.relational_list(ei, et, rc.N, rc.R) is not rel
    assert not torch.equal(before, after)
    ref = rc.forward(c.x.double(), c.basis.double(), c.att.double(), c.root.double(), c.bias.double(), c.edge_index, et.cpu(), c.edge_norm.double())
    t = float((rc.forward(c.x, c.basis, c.att, c.root, c.bias, c.edge_index, et.cpu(), c.edge_norm).double() - ref).abs().max())
    assert t > 0 and float((after.double().cpu() - ref).abs().max()) <= 4 * t


def test_conv1_and_conv2_share_one_plan(gpu):
    ei, et = (t.to(gpu) for t in rc.graph())
    a, b = RGCNConv(16, 32, rc.R, rc.R).to(gpu), RGCNConv(32, 8, rc.R, rc.R).to(gpu)
    with torch.no_grad():
        h = a(torch.randn((rc.N, 16), device=gpu), ei, et, _relu=True)
        rel = pyg_convs.relational_list(ei, et, rc.N, rc.R)
        b(h, ei, et, _relu=True)
    assert pyg_convs.relational_list(ei, et, rc.N, rc.R) is rel


@pytest.mark.parametrize("key", [(16, 32, 16, "random", True, True), (128, 64, 64, "mean", True, True), (33, 7, 17, "none", True, True)], ids=_id)
def test_two_calls_give_the_same_bits(gpu, key):
    c = rc.case(*key)
    a, b = _run(c, gpu), _run(c, gpu)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_ids_out_of_range_as_for_myrgcn(gpu):
    x = torch.zeros((4, 8), device=gpu)
    conv = RGCNConv(8, 4, 2, 2).to(gpu)
    with pytest.raises(IndexError):                                              # a node id: the plan builder's refusal, as for myRGCN
        gripnet_amd.myRGCN(8, 4, 2, 2, after_relu=False).to(gpu)(x, torch.tensor([[0, 1, 4], [1, 2, 0]], device=gpu), None, torch.tensor([[0, 2], [2, 3]]))
    with pytest.raises(IndexError):
        conv(x, torch.tensor([[0, 1, 4], [1, 2, 0]], device=gpu), torch.tensor([0, 1, 0], device=gpu))
    with pytest.raises(IndexError):
        conv(x, torch.tensor([[0, 1, 3], [1, 2, -1]], device=gpu), torch.tensor([0, 1, 0], device=gpu))
    with pytest.raises(IndexError):                                              # a relation outside [0, R)
        conv(x, torch.tensor([[0, 1, 3], [1, 2, 0]], device=gpu), torch.tensor([0, 2, 0], device=gpu))
    with pytest.raises(IndexError):
        conv(x, torch.tensor([[0, 1, 3], [1, 2, 0]], device=gpu), torch.tensor([0, -1, 0], device=gpu))


@pytest.mark.parametrize("norm", ["random", "none"])
def test_captured_step_replays_the_eager_bits(gpu, norm):
    c = rc.case(16, 32, 16, norm)
    conv = _module(c, gpu)
    ei, et, w = _operands(c, gpu)
    up = c.upstream.to(gpu)
    x = c.x.to(gpu).requires_grad_(True)
    params = (x, conv.basis, conv.att, conv.root, conv.bias)

    def step():
        for p in params:
            p.grad = None
        out = conv(x, ei, et, w, _relu=True)
        (out * up).sum().backward()
        return (out.detach(),) + tuple(p.grad for p in params)

    eager = [t.clone() for t in step()]                                         # (builds every plan the step needs)
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


# ---- GCNConv ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fin,fout,improved", [(256, 64, False), (64, 32, False), (256, 64, True), (64, 32, True)])
def test_gcnconv_is_mygcn_bit_for_bit(gpu, fin, fout, improved):
    g = torch.Generator().manual_seed(21)
    n = 70
    ei = torch.randint(0, n, (2, 400), generator=g).to(gpu)                     # loops and duplicates occur
    mine, theirs = gripnet_amd.myGCN(fin, fout, improved=improved).to(gpu), GCNConv(fin, fout, improved=improved).to(gpu)
    theirs.load_state_dict(mine.state_dict())
    with torch.no_grad():
        mine.bias.copy_(torch.randn((fout,), generator=g))
        theirs.bias.copy_(mine.bias)
    x0, up = torch.randn((n, fin), generator=g).to(gpu), torch.randn((n, fout), generator=g).to(gpu)
    res = []
    for conv in (mine, theirs):
        x = x0.clone().requires_grad_(True)
        out = conv(x, ei, _relu=True)
        (out * up).sum().backward()
        with torch.no_grad():
            res.append((out.detach(), x.grad, conv.weight.grad, conv.bias.grad, conv(x0, ei)))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    a, b = mine.norm(ei, n, None, improved), GCNConv.norm(ei, n, None, improved)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_gcnconv_keeps_its_plan_and_plans_again_after_an_edit(gpu):
    g = torch.Generator().manual_seed(22)
    n = 70
    ei = torch.randint(0, n, (2, 400), generator=g).to(gpu)
    a, b = GCNConv(16, 8).to(gpu), GCNConv(8, 4).to(gpu)
    x = torch.randn((n, 16), generator=g).to(gpu)
    with torch.no_grad():
        h = a(x, ei, _relu=True)
        plan = a.cached_result
        b(h, ei)
        assert b.cached_result is plan                                          # conv1 and conv2 share one build
        assert torch.equal(a(x, ei, _relu=True), h) and a.cached_result is plan
        ei[1, :50] = (ei[1, :50] + 1) % n                                       # in place: the tensor's version moves
        after = a(x, ei, _relu=True)
        assert a.cached_result is not plan
        mine = gripnet_amd.myGCN(16, 8).to(gpu)
        mine.load_state_dict(a.state_dict())
        assert torch.equal(after, mine(x, ei, _relu=True)) and not torch.equal(after, h)
        w = torch.rand((400,), generator=g).to(gpu)
        assert torch.equal(a(x, ei, w), mine(x, ei, w))                         # an edge_weight: a plan of its own
        assert torch.equal(a(x, ei), mine(x, ei))


# ---- the example ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["rgcn", "gcn"])
def test_example_trains_with_a_falling_loss(gpu, model):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_nc_baselines.py"), "--model", model, "--workload", "tiny",
                          "--epochs", "6"], capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout + run.stderr
    first, last = (float(v) for v in re.search(r"loss ([-0-9.einfa]+) -> ([-0-9.einfa]+)", run.stdout).groups())
    print(run.stdout)
    assert first == first and last == last and abs(first) != float("inf") and last < first
