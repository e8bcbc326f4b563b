"""gripnet_amd.RGCNConv and gripnet_amd.GCNConv without a GPU: constructor, state dict, initialisation, refusals, and the
float64 formulation of tests/rgcn_conv_cases.py against a five-node case worked by hand.  Also: the fp32 torch formulation's
error against float64, which the GPU tests take their bounds from, is non-zero on every case (a bound of 4 x 0 would hold
nothing)."""
import math

import pytest
import torch

import rgcn_conv_cases as rc
import gripnet_amd
from gripnet_amd import GCNConv, RGCNConv


def test_constructor_state_dict_and_shapes():
    conv = RGCNConv(6, 4, 5, 3)
    sd = conv.state_dict()
    assert list(sd) == ["basis", "att", "root", "bias"]
    assert tuple(sd["basis"].shape) == (3, 6, 4) and tuple(sd["att"].shape) == (5, 3)
    assert tuple(sd["root"].shape) == (6, 4) and tuple(sd["bias"].shape) == (4,)
    assert (conv.in_channels, conv.out_channels, conv.num_relations, conv.num_bases) == (6, 4, 5, 3)
    assert repr(conv) == "RGCNConv(6, 4, num_relations=5)"
    assert gripnet_amd.RGCNConv is RGCNConv and "RGCNConv" in gripnet_amd.__all__ and "GCNConv" in gripnet_amd.__all__


def test_root_weight_and_bias_can_be_left_out():
    conv = RGCNConv(6, 4, 5, 3, root_weight=False)
    assert list(conv.state_dict()) == ["basis", "att", "bias"] and conv.root is None
    conv = RGCNConv(6, 4, 5, 3, bias=False)
    assert list(conv.state_dict()) == ["basis", "att", "root"] and conv.bias is None
    conv = RGCNConv(6, 4, 5, 3, root_weight=False, bias=False)
    assert list(conv.state_dict()) == ["basis", "att"]


@pytest.mark.parametrize("fin,bases", [(6, 3), (32, 7), (1, 1)])
def test_initialisation_is_uniform_in_one_over_sqrt_bases_times_in(fin, bases):
    torch.manual_seed(3)
    conv = RGCNConv(fin, 9, 5, bases)
    bound = 1.0 / math.sqrt(bases * fin)
    for name, p in conv.named_parameters():
        assert float(p.abs().max()) <= bound, name
        assert bool((p != 0).any()), name
    assert float(conv.basis.abs().max()) > 0.5 * bound or conv.basis.numel() < 8


def _operands():
    conv = RGCNConv(2, 3, 2, 2)
    x = torch.zeros((4, 2))
    ei = torch.tensor([[0, 1], [1, 2]])
    et = torch.tensor([1, 0])
    return conv, x, ei, et


def test_refusals():
    conv, x, ei, et = _operands()
    with pytest.raises(ValueError, match="featureless"):
        conv(None, ei, et)
    with pytest.raises(ValueError, match="bipartite"):
        conv((x, x), ei, et)
    with pytest.raises(ValueError, match="bipartite"):
        conv(x, ei, et, size=(4, 4))
    with pytest.raises(ValueError, match="unknown arguments"):
        conv(x, ei, et, flow="target_to_source")
    with pytest.raises(ValueError, match="unknown arguments"):
        RGCNConv(2, 3, 2, 2, aggr="mean")
    with pytest.raises(ValueError, match="differentiable edge_norm"):
        conv(x, ei, et, edge_norm=torch.ones(2, requires_grad=True))
    with pytest.raises(ValueError, match="positive"):
        RGCNConv(2, 3, 2, 0)


def test_a_cpu_tensor_raises_as_for_every_layer():
    conv, x, ei, et = _operands()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, ei, et)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GCNConv(2, 3)(x, ei)


def test_gcnconv_is_its_own_class_with_mygcn_state():
    conv = GCNConv(256, 64)
    assert repr(conv) == "GCNConv(256, 64)" and type(conv).__name__ == "GCNConv" and GCNConv is not gripnet_amd.myGCN
    assert list(conv.state_dict()) == ["weight", "bias"]
    assert tuple(conv.weight.shape) == (256, 64) and tuple(conv.bias.shape) == (64,)
    assert conv.cached_result is None and conv.improved is False and conv.cached is False
    assert list(GCNConv(8, 4, bias=False).state_dict()) == ["weight"]
    assert GCNConv(8, 4, improved=True, cached=True).improved is True
    assert GCNConv.norm is gripnet_amd.myGCN.norm
    mine = gripnet_amd.myGCN(8, 4)
    assert [(k, tuple(v.shape)) for k, v in GCNConv(8, 4).state_dict().items()] == [(k, tuple(v.shape)) for k, v in mine.state_dict().items()]
    with pytest.raises(ValueError, match="normalize=False"):
        GCNConv(8, 4, normalize=False)
    with pytest.raises(ValueError, match="unknown arguments"):
        GCNConv(8, 4, flow="target_to_source")


def test_float64_formulation_against_the_hand_worked_case():
    c = rc.hand_case()
    assert torch.equal(rc.forward(c.x, c.basis, c.att, c.root, c.bias, c.edge_index, c.edge_type, c.edge_norm), c.weighted)
    assert torch.equal(rc.forward(c.x, c.basis, c.att, c.root, c.bias, c.edge_index, c.edge_type), c.plain)
    assert torch.equal(rc.forward(c.x, c.basis, c.att, None, None, c.edge_index, c.edge_type, c.edge_norm), c.bare)
    # the order of the list does not matter to the definition
    flip = torch.tensor([4, 2, 0, 3, 1])
    assert torch.equal(rc.forward(c.x, c.basis, c.att, c.root, c.bias, c.edge_index[:, flip], c.edge_type[flip], c.edge_norm[flip]), c.weighted)


def test_the_graph_holds_what_the_gpu_tests_rely_on():
    ei, et = rc.graph()
    deg = torch.bincount(ei[1], minlength=rc.N)
    assert tuple(deg[:9].tolist()) == rc.DEGREES
    assert int(deg[rc.HEAVY_NODE]) > rc.heavy_edges() and int(torch.bincount(ei[0], minlength=rc.N)[rc.HUB_SOURCE]) > rc.heavy_edges()
    assert bool((ei[0] == ei[1]).any())                                         # self loops
    pairs = ei[0] * rc.N + ei[1]
    assert pairs.unique().numel() < pairs.numel()                               # duplicates
    counts = torch.bincount(et, minlength=rc.R)
    assert int(counts[rc.EMPTY_RELATION]) == 0 and bool((counts[[0, 1, 2, 4]] > 0).all())
    assert bool((et[1:] < et[:-1]).any())                                       # unsorted
    w = rc.case(16, 32, 16, "random").edge_norm
    assert bool((w == 0).any()) and bool((w < 0).any())
    m = rc.case(16, 32, 16, "mean").edge_norm
    assert float(m.max()) == 1.0 and float(m.min()) > 0


@pytest.mark.parametrize("key", rc.GENERAL, ids=lambda k: "{}-{}-{}-{}{}{}".format(k[0], k[1], k[2], k[3], "" if k[4] else "-noroot", "" if k[5] else "-nobias"))
def test_fp32_formulation_error_is_non_zero(key):
    c, ref, t = rc.reference(*key)
    for name, r, e in zip(rc.NAMES, ref, t):
        if r is None:
            assert e is None
            continue
        print("{} {}: torch fp32 max error {:.3e}".format(key, name, e))
        assert e > 0.0, (key, name)
