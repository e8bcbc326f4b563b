"""Graph-attention layer under the reference's import name: ``from torch_geometric.nn import GATConv`` of
baselines/NC_baselines/GAT.py:3,66-67 (torch_geometric 1.4 / 1.5: one ``weight``, one ``att``), computed by csrc/gat.hip.

    h = x W  viewed [N, H, C];   z_e,h = h[i,h,:] . att[0,h,:C] + h[j,h,:] . att[0,h,C:]   for an edge j -> i
    alpha = softmax over the in-edges of i of leaky_relu(z);   out[i,h,:] = sum_e alpha_e,h h[j_e,h,:]

over the edge list without its loops plus one loop per node (duplicate edges count separately); the heads are concatenated
or averaged, then the bias is added.  Attention dropout, bipartite inputs and ``size=`` are refused.
"""
from __future__ import annotations

import math

import torch
from torch.nn import Module, Parameter

from . import _hip
from ._cache import MISS, VersionedCache
from .autograd import GatConvFn

_plans = VersionedCache(4)          # (edge_index tensor, N) -> the GraphPlan of its working list


def gat_plan(edge_index: torch.Tensor, num_nodes: int, transpose: bool = False):
    """The plan of `edge_index` over `num_nodes` nodes: input loops dropped, one loop per node, duplicates kept - the list
    myGCN normalises, so an id outside [0, N) raises the same IndexError.  Kept while the same unmodified tensor keeps coming
    (a static graph is planned once, by whichever layer sees it first).  `transpose`: with the source-major CSR of the
    backward, built now (it synchronises the stream once; nothing after it does)."""
    plan = _plans.get(edge_index, int(num_nodes))
    if plan is MISS:
        plan = _plans.put(edge_index, _hip.GraphPlan.gcn(edge_index, num_nodes), int(num_nodes))
    return plan.build_transpose() if transpose else plan


class GATConv(Module):
    """``GATConv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0, bias=True)``; state-dict keys
    ``weight`` [Fin, H * C], ``att`` [1, H, 2 C] (a head's target half, then its source half) and ``bias``."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0, bias=True, **kwargs):
        super().__init__()
        if dropout != 0:
            raise ValueError("GATConv: attention dropout is not built (dropout={!r}); the reference never sets it".format(dropout))
        if kwargs:
            raise ValueError("GATConv: unknown arguments {}".format(sorted(kwargs)))
        if heads < 1 or out_channels < 1 or in_channels < 1:
            raise ValueError("GATConv: in_channels, out_channels and heads must be positive")
        if heads * out_channels > _hip.GAT_MAX_ROW:
            raise ValueError("GATConv: heads * out_channels = {} floats per row, the kernels take at most {}".format(
                heads * out_channels, _hip.GAT_MAX_ROW))
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = concat, negative_slope, dropout
        self.weight = Parameter(torch.empty(in_channels, heads * out_channels))
        self.att = Parameter(torch.empty(1, heads, 2 * out_channels))
        if bias:
            self.bias = Parameter(torch.empty(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        for p in (self.weight, self.att):                                        # glorot: +- sqrt(6 / (size(-2) + size(-1)))
            bound = math.sqrt(6.0 / (p.size(-2) + p.size(-1)))
            p.data.uniform_(-bound, bound)
        if self.bias is not None:
            self.bias.data.fill_(0)

    def forward(self, x, edge_index, size=None, *, _relu=False):
        # _relu: the ReLU that follows the layer in GAT.py:66-67, applied where the output is stored
        if size is not None or isinstance(x, (tuple, list)):
            raise ValueError("GATConv: bipartite inputs (a tuple x, size=) are not built")
        _hip.require_gpu(x, edge_index, self.weight)
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError("expected x of shape [N, {}], got {}".format(self.in_channels, tuple(x.shape)))
        need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        plan = gat_plan(edge_index, x.shape[0], transpose=need_grad)
        return GatConvFn.apply(x, self.weight, self.att, self.bias, plan, self.heads, self.concat, self.negative_slope, _relu)

    def __repr__(self):
        return "{}({}, {}, heads={})".format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)
