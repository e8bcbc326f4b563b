"""The graph-attention reference of tests/gat_cases.py pinned on the CPU (torch_geometric is not installed, so no fixture of
its GATConv can be made: the definition is checked by hand instead), and what gripnet_amd.GATConv does without a GPU."""
import math

import pytest
import torch

import gat_cases as gc
import gripnet_amd
from gripnet_amd import GATConv

LN2 = math.log(2.0)


def _scalar_layer(att_dst, att_src):
    """one head, one channel, h = x: the weights of a node's softmax are exp(leaky(att_dst x_i + att_src x_j))"""
    x = torch.tensor([[1.0], [2.0], [3.0]], dtype=torch.float64)
    w = torch.ones((1, 1), dtype=torch.float64)
    att = torch.tensor([[[att_dst, att_src]]], dtype=torch.float64)
    ei = torch.tensor([[0, 1], [2, 2]])
    return x, w, att, ei


def test_three_nodes_by_hand():
    # z = ln 2 * x_j > 0: node 2 weighs its in-edges from 0, 1 and itself by 2, 4, 8
    x, w, att, ei = _scalar_layer(0.0, LN2)
    _, src, dst, _, alpha = gc.parts(x, w, att, ei, 1)
    assert src.tolist() == [0, 1, 0, 1, 2] and dst.tolist() == [2, 2, 0, 1, 2]
    assert torch.allclose(alpha[:, 0], torch.tensor([2 / 14, 4 / 14, 1.0, 1.0, 8 / 14], dtype=torch.float64), rtol=1e-14)
    out = gc.forward(x, w, att, torch.tensor([0.5], dtype=torch.float64), ei, 1)
    assert torch.allclose(out[:, 0], torch.tensor([1.5, 2.5, 34 / 14 + 0.5], dtype=torch.float64), rtol=1e-14)
    # z = -5 ln 2 * x_j < 0 under slope 0.2: l = -ln 2 * x_j, weights 1/2, 1/4, 1/8
    x, w, att, ei = _scalar_layer(0.0, -5 * LN2)
    out = gc.forward(x, w, att, None, ei, 1, slope=0.2)
    assert torch.allclose(out[:, 0], torch.tensor([1.0, 2.0, 11 / 7], dtype=torch.float64), rtol=1e-14)
    # the first half of att belongs to the target: it shifts every logit of a node alike and changes nothing
    x, w, att, ei = _scalar_layer(3.0, LN2)
    assert torch.allclose(gc.forward(x, w, att, None, ei, 1)[:, 0], torch.tensor([1.0, 2.0, 34 / 14], dtype=torch.float64), rtol=1e-13)


@pytest.mark.parametrize("graph", ["small", "random"])
def test_alpha_sums_to_one_and_zero_att_is_the_mean(graph):
    c = gc.case(graph, 3, 5)
    x, w, att = c.x.double(), c.weight.double(), c.att.double()
    _, src, dst, _, alpha = gc.parts(x, w, att, c.edge_index, 3)
    total = torch.zeros((c.n, 3), dtype=torch.float64).index_add_(0, dst, alpha)
    assert torch.allclose(total, torch.ones_like(total), rtol=1e-13)
    out = gc.forward(x, w, torch.zeros_like(att), None, c.edge_index, 3)
    h = x @ w
    deg = torch.zeros(c.n, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64))
    mean = torch.zeros_like(h).index_add_(0, dst, h[src]) / deg[:, None]
    assert torch.allclose(out, mean, rtol=1e-13, atol=1e-15)


def test_input_loop_is_replaced_and_duplicate_counts_twice():
    x, w, att, _ = _scalar_layer(0.0, LN2)
    plain = gc.forward(x, w, att, None, torch.tensor([[0, 1], [2, 2]]), 1)
    looped = gc.forward(x, w, att, None, torch.tensor([[0, 2, 1, 2, 0], [2, 2, 2, 2, 0]]), 1)
    assert torch.equal(plain, looped)
    assert gc.working_list(torch.tensor([[0, 2, 1, 2, 0], [2, 2, 2, 2, 0]]), 3).shape[1] == 5
    twice = gc.forward(x, w, att, None, torch.tensor([[0, 0, 1], [2, 2, 2]]), 1)
    assert torch.allclose(twice[2, 0], torch.tensor((2 * 2 * 1 + 4 * 2 + 8 * 3) / 16, dtype=torch.float64), rtol=1e-14)


@pytest.mark.parametrize("concat", [True, False])
def test_gradcheck_of_the_reference(concat):
    c = gc.case("small", 2, 3, fin=4, concat=concat, seed=4)
    x, w, att, b = (t.double().requires_grad_(True) for t in (c.x, c.weight, c.att, c.bias))
    z = gc.parts(x, w, att, c.edge_index, 2)[3].detach()
    assert bool((z < 0).any()) and bool((z > 0).any()) and float(z.abs().min()) > 1e-3      # both branches, none at the kink
    assert torch.autograd.gradcheck(lambda *a: gc.forward(*a, c.edge_index, 2, concat), (x, w, att, b), eps=1e-6, atol=1e-7)


def test_subgradient_at_zero_is_the_negative_slope():
    # z = x_i - x_j: 0 on the loops and on 0 -> 1, -1 on 2 -> 0, never positive - the layer equals the one whose activation is
    # slope * z, and so do its gradients exactly when the derivative taken at z = 0 is the slope
    slope = 0.2
    ei = torch.tensor([[0, 2], [1, 0]])

    def run(leaky):
        x = torch.tensor([[1.0], [1.0], [2.0]], dtype=torch.float64, requires_grad=True)
        w = torch.ones((1, 1), dtype=torch.float64, requires_grad=True)
        att = torch.tensor([[[1.0, -1.0]]], dtype=torch.float64, requires_grad=True)
        z = gc.parts(x, w, att, ei, 1, slope)[3]
        assert sorted(z[:, 0].tolist()) == [-1.0, 0.0, 0.0, 0.0, 0.0]
        out = gc.forward(x, w, att, None, ei, 1, True, slope, leaky=leaky)
        return torch.autograd.grad((out * torch.tensor([[1.0], [-2.0], [3.0]], dtype=torch.float64)).sum(), (x, w, att))

    for a, b in zip(run(None), run(lambda z: slope * z)):
        assert torch.equal(a, b) and bool((a != 0).any())


def test_constructor_state_and_initialisation():
    torch.manual_seed(0)
    conv = GATConv(256, 16, heads=4)
    assert repr(conv) == "GATConv(256, 16, heads=4)"
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {"weight": (256, 64), "att": (1, 4, 32), "bias": (64,)}
    bw, ba = math.sqrt(6 / (256 + 64)), math.sqrt(6 / (4 + 32))
    assert 0.9 * bw < float(conv.weight.data.abs().max()) <= bw and 0.8 * ba < float(conv.att.data.abs().max()) <= ba
    assert bool((conv.bias == 0).all())
    mean = GATConv(64, 32, concat=False)
    assert {k: tuple(v.shape) for k, v in mean.state_dict().items()} == {"weight": (64, 32), "att": (1, 1, 64), "bias": (32,)}
    assert list(GATConv(8, 4, heads=2, bias=False).state_dict()) == ["weight", "att"]
    assert (conv.negative_slope, conv.dropout, conv.concat, mean.concat) == (0.2, 0, True, False)
    assert gripnet_amd.GATConv is GATConv


def test_refusals():
    with pytest.raises(ValueError, match="dropout"):
        GATConv(8, 4, dropout=0.6)
    GATConv(8, 32, heads=4)                                                   # the last admitted width
    GATConv(8, gc.MAX_ROW, heads=1)
    with pytest.raises(ValueError, match="at most 128"):
        GATConv(8, 43, heads=3)                                               # 129 floats
    conv = GATConv(8, 4)
    ei = torch.zeros((2, 1), dtype=torch.long)
    with pytest.raises(ValueError, match="bipartite"):
        conv((torch.zeros(3, 8), torch.zeros(2, 8)), ei)
    with pytest.raises(ValueError, match="bipartite"):
        conv(torch.zeros(3, 8), ei, size=(3, 3))


def test_cpu_tensor_raises():
    conv = GATConv(8, 4, heads=2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        conv(torch.zeros(3, 8), torch.zeros((2, 1), dtype=torch.long))


def test_homogeneous_workload():
    d = gripnet_amd.synth.make_nc_homogeneous("tiny")
    base = gripnet_amd.synth.make_nc("tiny")
    n = base.n_a_node + base.n_p_node + base.n_q_node
    assert d.num_nodes == n and d.num_classes == base.n_a_type
    ei = d.edge_index
    assert ei.dtype == torch.long and int(ei.min()) >= 0 and int(ei.max()) < n
    pairs = set(map(tuple, ei.t().tolist()))
    assert all((b, a) in pairs for a, b in pairs)                              # bidirectional
    assert ei.shape[1] == base.n_aa_edge + base.n_pp_edge + base.n_qq_edge + 2 * (base.pa_edge_idx.shape[1] + base.qa_edge_idx.shape[1])
    both = torch.cat([d.train_idx, d.test_idx])
    assert sorted(both.tolist()) == list(range(base.n_a_node)) and len(d.train_idx) > len(d.test_idx) > 0
    assert torch.equal(d.train_y, base.a_label[d.train_idx]) and torch.equal(d.test_y, base.a_label[d.test_idx])
