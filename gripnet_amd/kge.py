"""The knowledge-graph-embedding baselines of the link-prediction comparison: TransE, DistMult, ComplEx, RotatE.

Drop-in for the ``KGEModel`` that baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:58-235 defines in the driver
itself: the same constructor signature, attributes, state-dict keys, initialisation range and errors; ``forward`` scores a triple list in
one HIP launch (csrc/kge.hip) instead of three ``index_select``s of [E, D] and a dozen element-wise kernels, and its
gradients come from a sort-based segmented reduction instead of autograd's scatter-adds.
"""
import torch
from torch import nn

from . import _hip
from .autograd import KgeScoreFn

PI = 3.14159265358979323846                                    # the constant the reference divides by (:214)

# model -> (entity rows hold a real and an imaginary half, relation rows do); None: the caller's flag decides
_HALVES = {"TransE": (None, None), "DistMult": (None, None), "ComplEx": (True, True), "RotatE": (True, None)}


class KGEModel(nn.Module):
    """``KGEModel(model_name, nentity, nrelation, hidden_dim, gamma)``: entity table [nentity, De], relation table
    [nrelation, Dr] with De, Dr = hidden_dim or twice that (ComplEx: both doubled; RotatE: the entities; otherwise as the two
    flags say), both uniform in +-(gamma + 2) / hidden_dim; ``gamma`` and ``embedding_range`` are frozen one-element
    parameters, so that the state dict is the reference's."""

    def __init__(self, model_name, nentity, nrelation, hidden_dim, gamma, double_entity_embedding=False,
                 double_relation_embedding=False):
        if model_name not in _HALVES:
            raise ValueError("model %s not supported" % model_name)
        wide_entity, wide_relation = [flag if forced is None else forced for forced, flag in
                                      zip(_HALVES[model_name], (double_entity_embedding, double_relation_embedding))]
        if model_name == "RotatE" and wide_relation:               # a relation is one phase per column
            raise ValueError("RotatE should use --double_entity_embedding")
        super().__init__()
        self.model_name, self.nentity, self.nrelation, self.hidden_dim = model_name, nentity, nrelation, hidden_dim
        self.epsilon = 2.0
        self.entity_dim = (2 if wide_entity else 1) * hidden_dim
        self.relation_dim = (2 if wide_relation else 1) * hidden_dim
        margin = torch.tensor([float(gamma)])
        spread = (margin.item() + self.epsilon) / hidden_dim       # (from the fp32 margin, as the state dict holds it)
        self.gamma = nn.Parameter(margin, requires_grad=False)
        self.embedding_range = nn.Parameter(torch.tensor([spread]), requires_grad=False)
        spread = self.embedding_range.item()
        self.entity_embedding = nn.Parameter(torch.empty(nentity, self.entity_dim).uniform_(-spread, spread))
        self.relation_embedding = nn.Parameter(torch.empty(nrelation, self.relation_dim).uniform_(-spread, spread))

    def _constants(self):
        """(gamma, phase divisor) as host floats, read from the parameters once per (tensor, version): `.item()` on a device
        parameter is a synchronising copy, and the reference pays it in every forward (:192, :221)."""
        key = (self.gamma.data_ptr(), self.gamma._version, self.embedding_range.data_ptr(), self.embedding_range._version)
        cached = self.__dict__.get("_consts")
        if cached is None or cached[0] != key:
            cached = (key, (self.gamma.item(), self.embedding_range.item() / PI))
            self.__dict__["_consts"] = cached
        return cached[1]

    def _score(self, sample, et, log_sigmoid):
        ent, rel = self.entity_embedding, self.relation_embedding
        _hip.require_gpu(ent, rel, sample, et)
        gamma, divisor = self._constants()
        if torch.is_grad_enabled() and (ent.requires_grad or rel.requires_grad):
            return KgeScoreFn.apply(ent, rel, sample, et, self.model_name, gamma, divisor, log_sigmoid)
        out = torch.empty((sample.shape[1],), dtype=torch.float32, device=ent.device)
        return _hip.kge_forward(self.model_name, _hip.f32_rows(ent.detach()), _hip.f32_rows(rel.detach()), sample, et, gamma,
                                divisor, log_sigmoid, out)

    def forward(self, sample, et, mode="single"):
        """``logsigmoid(score)`` [E] of the triples (sample[0, e], et[e], sample[1, e]) (:127-187).  An id outside its table
        gives NaN for that triple and raises IndexError at the next synchronising check (``_hip.raise_if_index_errors``,
        ``utils.relation_metrics``), as the decoders do."""
        return self._score(sample, et, True)

    def score(self, sample, et):
        """The raw scores [E] (before the log-sigmoid): for metrics and tests."""
        return self._score(sample, et, False)
