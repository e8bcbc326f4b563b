"""The two stock layers of the reference's remaining node-classification baselines under their import names:
``from torch_geometric.nn import GCNConv`` (baselines/NC_baselines/GCN_MLP.py:4,47-48) and ``from torch_geometric.nn import
RGCNConv`` (baselines/NC_baselines/RGCN_MLP.py:3,52-57), as torch_geometric 1.4 / 1.5 define them.

GCNConv is the layer the reference's myGCN was copied from: the same arithmetic on the same kernels, under its own name.

RGCNConv differs from myRGCN where it reaches the kernels:

    W_r    = sum_b att[r, b] basis[b]
    out[i] = sum_{e: dst_e = i} w_e x[src_e] W_{r(e)}  (+ x[i] root)  (+ bias),     w_e = edge_norm[e] or 1

a SUM over the in-edges (aggr='add'), an optional per-edge factor, `edge_type` in any order and no range list.  The edge
list is taken exactly as given: no loops added or removed, duplicates count separately.  The featureless mode (x=None),
bipartite inputs, ``size=`` and a differentiable `edge_norm` are refused.
"""
from __future__ import annotations

import math

import torch
from torch.nn import Module, Parameter

from . import _hip
from ._cache import MISS, VersionedCache
from .autograd import RgcnSumConvFn
from .layers import myGCN

RGCN_MAX_BASES, RGCN_MAX_FEATURES = 64, 128        # the general relational kernel's limits (GN_RGCN_PATH_GENERAL), both sides of the layer

_plans = VersionedCache(4)          # (edge_index, (edge_type, its version, N, R)) -> RelationalList
_gcn_plans = VersionedCache(4)      # (edge_index, (N, improved, edge_weight and its version)) -> (GraphPlan, edge_weight) of GCNConv(cached=False)


class RelationalList:
    """What one (edge_index, edge_type) pair needs before its first launch: the stable sort of the edges by type (the
    permutation, None for a list that is sorted already), the [R, 2] ranges and the plan of the sorted list.  Holds the
    caller's `edge_type` (compared with `is`, with its version) next to the cache's own watch on `edge_index`."""

    def __init__(self, edge_index, edge_type, num_nodes, num_relations):
        e = _hip.e_count(edge_index)
        if edge_type.dim() != 1 or edge_type.numel() != e:
            raise ValueError("RGCNConv: edge_type has shape {} for {} edges".format(tuple(edge_type.shape), e))
        et = _hip.i64_vec(edge_type)
        self.edge_type, self.type_version = edge_type, edge_type._version
        counts = torch.zeros(num_relations, dtype=torch.int64, device=et.device)
        if e:
            # one synchronisation per new graph: the extremes (a type outside [0, R) raises like a node id outside [0, N)),
            # whether the list is sorted already, and the relations' counts
            lo, hi, unsorted = int(et.min()), int(et.max()), bool((et[1:] < et[:-1]).any())
            if lo < 0 or hi >= num_relations:
                raise IndexError("edge_type holds a relation outside [0,{})".format(num_relations))
            counts = torch.bincount(et, minlength=num_relations)
        else:
            unsorted = False
        ends = torch.cumsum(counts, 0)
        self.range_list = torch.stack([ends - counts, ends], dim=1).cpu()
        if unsorted:
            self.perm = torch.sort(et, stable=True).indices                     # stable: inside a relation the caller's order
            sorted_index = edge_index.index_select(1, self.perm).contiguous()
        else:
            self.perm, sorted_index = None, edge_index.detach()               # (another object: a cache value does not hold its key)
        # a light plan: the sum and the weighted calls run on the general kernel (the table kernel beyond its shapes) only
        self.plan = _hip.RgcnPlan(sorted_index, self.range_list, num_nodes, light=True, perm=self.perm)

    def in_sorted_order(self, edge_norm):
        return edge_norm if self.perm is None else edge_norm.index_select(0, self.perm)


def relational_list(edge_index, edge_type, num_nodes, num_relations) -> RelationalList:
    """The RelationalList of this pair, kept while the same unmodified tensors keep coming (`conv1` and `conv2` of the
    baseline share one build; an in-place write to either tensor plans again)."""
    extra = (id(edge_type), edge_type._version, int(num_nodes), int(num_relations))
    hit = _plans.get(edge_index, *extra)
    if hit is not MISS and hit.edge_type is edge_type:
        return hit
    return _plans.put(edge_index, RelationalList(edge_index, edge_type, int(num_nodes), int(num_relations)), *extra)


class RGCNConv(Module):
    """``RGCNConv(in_channels, out_channels, num_relations, num_bases, root_weight=True, bias=True)``; state-dict keys ``basis``
    [num_bases, in, out], ``att`` [num_relations, num_bases], ``root`` [in, out] and ``bias`` [out] (the last two where
    they exist)."""

    def __init__(self, in_channels, out_channels, num_relations, num_bases, root_weight=True, bias=True, **kwargs):
        super().__init__()
        if kwargs:
            raise ValueError("RGCNConv: unknown arguments {}".format(sorted(kwargs)))
        if in_channels < 1 or out_channels < 1 or num_relations < 1 or num_bases < 1:
            raise ValueError("RGCNConv: in_channels, out_channels, num_relations and num_bases must be positive")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_relations, self.num_bases = num_relations, num_bases
        self.basis = Parameter(torch.empty(num_bases, in_channels, out_channels))
        self.att = Parameter(torch.empty(num_relations, num_bases))
        if root_weight:
            self.root = Parameter(torch.empty(in_channels, out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.num_bases * self.in_channels)               # uniform(num_bases * in_channels, .)
        for p in (self.basis, self.att, self.root, self.bias):
            if p is not None:
                p.data.uniform_(-bound, bound)

    def weighted_limits_ok(self) -> bool:
        return (self.num_bases <= RGCN_MAX_BASES and self.in_channels <= RGCN_MAX_FEATURES and
                self.out_channels <= RGCN_MAX_FEATURES)

    def forward(self, x, edge_index, edge_type, edge_norm=None, size=None, *, _relu=False, **kwargs):
        # _relu: the ReLU that follows the layer in RGCN_MLP.py:62-63, applied where the output is stored
        if kwargs:
            raise ValueError("RGCNConv: unknown arguments {}".format(sorted(kwargs)))
        if x is None:
            raise ValueError("RGCNConv: the featureless mode (x=None) is not built")
        if size is not None or isinstance(x, (tuple, list)):
            raise ValueError("RGCNConv: bipartite inputs (a tuple x, size=) are not built")
        if edge_norm is not None and edge_norm.requires_grad:
            raise ValueError("RGCNConv: a differentiable edge_norm is not built (pass edge_norm.detach())")
        _hip.require_gpu(x, edge_index, edge_type, edge_norm, self.basis)
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError("expected x of shape [N, {}], got {}".format(self.in_channels, tuple(x.shape)))
        if edge_norm is not None:
            if edge_norm.dim() != 1 or edge_norm.numel() != _hip.e_count(edge_index):
                raise ValueError("RGCNConv: edge_norm has shape {} for {} edges".format(tuple(edge_norm.shape), _hip.e_count(edge_index)))
            if not self.weighted_limits_ok():
                raise ValueError("RGCNConv: edge_norm is taken up to {} bases and {} input and output features, got {} bases, {} -> {}".format(
                    RGCN_MAX_BASES, RGCN_MAX_FEATURES, self.num_bases, self.in_channels, self.out_channels))
            edge_norm = edge_norm.detach().to(torch.float32).contiguous()
        rel = relational_list(edge_index, edge_type, x.shape[0], self.num_relations)
        w_sorted = None if edge_norm is None else rel.in_sorted_order(edge_norm)
        return RgcnSumConvFn.apply(x, self.basis, self.att, self.root, self.bias, rel.plan, edge_norm, w_sorted, _relu)

    def __repr__(self):
        return "{}({}, {}, num_relations={})".format(self.__class__.__name__, self.in_channels, self.out_channels, self.num_relations)


class GCNConv(myGCN):
    """``GCNConv(in_channels, out_channels, improved=False, cached=False, bias=True, normalize=True)`` of torch_geometric
    1.4 / 1.5: ``out = D^-1/2 (A + I) D^-1/2 (x W) + b``.  The reference's myGCN is a copy of this class (layers.py:15-105),
    so the arithmetic, the kernels, the state dict (``weight``, ``bias``), ``cached_result`` and ``norm`` are myGCN's; the
    name and the printed form are the baseline's."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, normalize=True, **kwargs):
        if kwargs:
            raise ValueError("GCNConv: unknown arguments {}".format(sorted(kwargs)))
        if not normalize:
            raise ValueError("GCNConv: normalize=False is not built; the reference never sets it")
        super().__init__(in_channels, out_channels, improved=improved, cached=cached, bias=bias)
        self.normalize = True

    def _gcn_plan(self, edge_index, n, edge_weight):
        """cached=False (the baseline's setting) recomputes the normalised list on every call in PyG; here the plan of an
        unmodified `edge_index` (and `edge_weight`) is the same plan, so it is kept while the same tensors keep coming - by
        whichever layer sees them first, as for GATConv - and an in-place write plans again.  cached=True: myGCN's protocol."""
        if self.cached:
            return super()._gcn_plan(edge_index, n, edge_weight)
        extra = (int(n), bool(self.improved), None if edge_weight is None else (id(edge_weight), edge_weight._version))
        hit = _gcn_plans.get(edge_index, *extra)
        if hit is MISS or hit[1] is not edge_weight:
            hit = _gcn_plans.put(edge_index, (_hip.GraphPlan.gcn(edge_index, n, edge_weight, self.improved), edge_weight), *extra)
        self.cached_num_edges, self.cached_result = edge_index.size(1), hit[0]
        return hit[0]

    def forward(self, x, edge_index, edge_weight=None, *, _relu=False):
        # _relu: the ReLU that follows the layer in GCN_MLP.py:53-54, applied where the output is stored
        if isinstance(x, (tuple, list)):
            raise ValueError("GCNConv: bipartite inputs (a tuple x) are not built")
        return super().forward(x, edge_index, edge_weight, _relu=_relu)

    def __repr__(self):
        return "GCNConv({}, {})".format(self.in_channels, self.out_channels)
