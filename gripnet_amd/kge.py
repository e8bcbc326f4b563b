"""The knowledge-graph-embedding baselines of the link-prediction comparison: TransE, DistMult, ComplEx, RotatE.

Drop-in for the ``KGEModel`` that baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:58-235 defines in the driver
itself: the same constructor signature, attributes, state-dict keys, initialisation range and errors; ``forward`` scores a triple list in
one HIP launch (csrc/kge.hip) instead of three ``index_select``s of [E, D] and a dozen element-wise kernels, and its
gradients come from a sort-based segmented reduction instead of autograd's scatter-adds.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _hip
from .autograd import KgeBatchScoreFn, KgeNegativeSamplingLossFn, KgeScoreFn, KgeSharedScoreFn

PI = 3.14159265358979323846                                    # the constant the reference divides by (:214)

# model -> (entity rows hold a real and an imaginary half, relation rows do); None: the caller's flag decides
_HALVES = {"TransE": (None, None), "DistMult": (None, None), "ComplEx": (True, True), "RotatE": (True, None)}

_BATCH_SIDES = {"tail-batch": "tail", "head-batch": "head"}    # forward's batch modes -> the side the candidates stand on
_SHARED_SIDES = {"tail-shared": "tail", "head-shared": "head"}  # forward's shared-list modes -> that side


def self_adversarial_loss(positive_score, negative_score, adversarial_temperature=None):
    """The negative-sampling loss these four models are trained with where K negatives come with every positive, on RAW
    scores: positive_score [B], negative_score [B, K].  The negatives are averaged, or - with a temperature T - weighted by
    ``softmax(T * negative_score, dim=1)`` taken as a constant (self-adversarial weighting).
    ``(-logsigmoid(s_pos).mean() - neg.mean()) / 2``.  Plain torch ops: 4 bytes per score."""
    pos = F.logsigmoid(positive_score)
    neg = F.logsigmoid(-negative_score)
    if adversarial_temperature is None:
        neg = neg.mean(dim=1)
    else:
        neg = (F.softmax(negative_score * adversarial_temperature, dim=1).detach() * neg).sum(dim=1)
    return (-pos.mean() - neg.mean()) / 2


def _loss_block(positive_score, negative_score, adversarial_temperature, subsampling_weight):
    """The shape checks of ``negative_sampling_loss``; the temperature as a float or None."""
    if positive_score.dim() != 1 or positive_score.shape[0] < 1:
        raise ValueError("positive_score must have shape [B] with B >= 1, got {}".format(tuple(positive_score.shape)))
    b = positive_score.shape[0]
    if negative_score.dim() != 2 or negative_score.shape[0] != b or negative_score.shape[1] < 1:
        raise ValueError("negative_score must have shape [{}, K] with K >= 1, got {}".format(b, tuple(negative_score.shape)))
    if subsampling_weight is not None and tuple(subsampling_weight.shape) != (b,):
        raise ValueError("subsampling_weight must have shape [{}], got {}".format(b, tuple(subsampling_weight.shape)))
    if adversarial_temperature is None:
        return None
    number = (int, float, np.integer, np.floating)
    if isinstance(adversarial_temperature, bool) or not isinstance(adversarial_temperature, number):
        raise ValueError("adversarial_temperature must be a number or None, got {!r}".format(adversarial_temperature))
    return float(adversarial_temperature)


def negative_sampling_loss(positive_score, negative_score, adversarial_temperature=None, subsampling_weight=None):
    """``self_adversarial_loss`` in one HIP launch forward and one backward (csrc/kge_loss.hip), with the subsampling weights
    of the code base these models come from: on RAW scores positive_score [B] and negative_score [B, K] (what
    ``KGEModel.score`` returns; a column view of a wider matrix is read in place), with w = subsampling_weight [B]
    (constants; None: ones),

        loss = -(sum_b w_b logsigmoid(pos_b)) / (2 sum_b w_b) - (sum_b w_b N_b) / (2 sum_b w_b)

    N_b the mean over k of logsigmoid(-neg_bk) or - with a temperature T - their sum weighted by
    ``softmax(T * neg_b)`` taken as a constant.  A 0-d tensor; the gradients reach the embeddings through the score
    functions' own backward.  Deterministic, no host synchronisation, capturable.  B == 0 or K == 0: ValueError."""
    temperature = _loss_block(positive_score, negative_score, adversarial_temperature, subsampling_weight)
    _hip.require_gpu(positive_score, negative_score, subsampling_weight)
    return KgeNegativeSamplingLossFn.apply(positive_score, negative_score, subsampling_weight, temperature)


def _shared_block(positive, negatives, et):
    """The shape checks of the shared-list modes: positive [2, B], et [B], negatives [G, K] with 1 <= G <= B, B % G == 0."""
    if positive.dim() != 2 or positive.shape[0] != 2 or positive.shape[1] < 1:
        raise ValueError("positive must have shape [2, B] with B >= 1, got {}".format(tuple(positive.shape)))
    b = positive.shape[1]
    if et.dim() != 1 or et.shape[0] != b:
        raise ValueError("edge_type must have shape [{}], got {}".format(b, tuple(et.shape)))
    if negatives.dim() != 2 or not 1 <= negatives.shape[0] <= b:
        raise ValueError("negatives must have shape [G, K] with 1 <= G <= {}, got {}".format(b, tuple(negatives.shape)))
    if b % negatives.shape[0] != 0:
        raise ValueError("the {} lists of negatives {} do not divide the {} positives {} into equal chunks".format(
            negatives.shape[0], tuple(negatives.shape), b, tuple(positive.shape)))


def sample_candidates(positive, et, K, nentity, side="tail", known=None, seed=0, step=None, out=None, candidates=None):
    """int64 [B, K]: K candidate entities per positive (positive[0, b], et[b], positive[1, b]) for the batch modes of
    ``KGEModel.forward`` / ``.score``, drawn on the device (gn_kge_candidates_sample) uniformly, with replacement, from the
    entities that are not known partners.  `side` and `known` as for ``rank`` / ``top_k``: ``side="tail"`` fixes the head
    positive[0] and takes a KnownPairs keyed (r, head) - candidate tails t' with (h, r, t') known are never drawn;
    ``side="head"`` fixes the tail positive[1] and takes one built from the FLIPPED lists.  ``known=None``: no filter
    (``torch.randint``'s distribution, this sampler's stream; the relation table's size then comes from nowhere, and a
    relation id is only held to be non-negative).  The draw is a pure function of (seed, b, k, the row's
    partners), documented in include/gripnet_hip.h.  `step`: a one-element int64 tensor on the device; the draw is then that
    of ``seed + step``, read on the device and NOT advanced - ``step += 1`` after the call is an op of the caller's, so a
    captured mini-batch draws anew at every replay.  `out`: an int64 [B, K] tensor to fill (unit inner stride; a column
    view of a wider matrix is written in place).  No host synchronisation: a positive with an id outside its table gets a
    row of -1 (NaN scores) and a row that knows every entity keeps its last draw; both raise at the next synchronising check
    (``_hip.raise_if_index_errors``).  `candidates`: an int64 [R, 2] tensor on the device, row r = (lo, hi) the entities a
    positive of relation r draws from - the valid tails for ``side="tail"``, the valid heads for ``side="head"``
    (``utils.candidate_ranges``; R is `known`'s relation count, or with ``known=None`` the table's own, and a relation id
    beyond it then gets a row of -1).  The draw becomes ``lo + ((low32(h) * (hi - lo)) >> 32)``; with (0, nentity) it is
    the unranged draw element for element.  An empty range gives a row of -1 and the "no entity to draw" RuntimeError, a
    range outside [0, nentity] or with lo > hi a row of -1 and the IndexError, both at the next check."""
    if side not in _hip.KGE_SIDES:
        raise ValueError("side must be 'tail' or 'head', got {!r}".format(side))
    if positive.dim() != 2 or positive.shape[0] != 2:
        raise ValueError("positive must have shape [2, B], got {}".format(tuple(positive.shape)))
    b = positive.shape[1]
    if et.dim() != 1 or et.shape[0] != b:
        raise ValueError("edge_type has {} entries for {} positives".format(et.numel(), b))
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or int(K) < 1:
        raise ValueError("K must be a positive integer, got {!r}".format(K))
    if isinstance(nentity, bool) or not isinstance(nentity, (int, np.integer)) or not 1 <= int(nentity) < 2 ** 31:
        raise ValueError("nentity must be an integer in [1, 2^31), got {!r}".format(nentity))
    K, nentity = int(K), int(nentity)
    if known is not None:
        if not isinstance(known, _hip.KnownPairs):
            raise TypeError("`known` must be a KnownPairs, got {}".format(type(known).__name__))
        if known.num_nodes != nentity or known.device != positive.device:
            raise ValueError("KnownPairs was built for {} entities on {}; the call has {} on {}".format(
                known.num_nodes, known.device, nentity, positive.device))
    if step is not None and (step.dtype != torch.int64 or step.numel() != 1 or step.device != positive.device):
        raise ValueError("`step` must be a one-element int64 tensor on {}".format(positive.device))
    if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (b, K) or out.device != positive.device or
                            (K > 1 and out.stride(1) != 1) or (b > 1 and out.stride(0) < K)):
        raise ValueError("`out` must be an int64 [{}, {}] tensor with a unit inner stride on {}".format(b, K, positive.device))
    candidates = _hip.candidate_table(candidates, None if known is None else known.num_et, positive.device)
    _hip.require_gpu(positive, et)
    if out is None:
        out = torch.empty((b, K), dtype=torch.int64, device=positive.device)
    fixed = positive[0] if side == "tail" else positive[1]
    return _hip.kge_candidates_sample(fixed, et, K, nentity, known, seed, step, out, candidates)


def sample_shared_candidates(G, K, nentity, seed=0, step=None, out=None, candidates_range=None, device=None):
    """int64 [G, K]: one list of K candidate entities per chunk of positives for the shared-list modes of
    ``KGEModel.forward`` / ``.score`` ('tail-shared' / 'head-shared'), drawn on the device uniformly, with replacement, from
    all `nentity` entities or - with ``candidates_range=(lo, hi)`` - from the entities lo <= c < hi.  It is
    ``sample_candidates``' unfiltered draw with the chunk index g in the place of the positive b: the same kernel and the same
    documented stream (include/gripnet_hip.h, gn_kge_candidates_sample), ``base = mix64(seed ^ (g K + k) *
    0xD6E8FEB86659FD93)``, element for element what ``sample_candidates(known=None)`` gives G positives.  `seed`, `step`
    and `out` (int64 [G, K], unit inner stride) as there; `device`: where to draw when neither `out` nor `step` says
    (default: the current GPU).  A list is shared by many positives, so a per-positive `known` filter cannot apply to it:
    NO false negative is filtered or masked here (a drawn candidate may be a positive's true partner, as in the trainers
    this scheme comes from); a caller who needs filtered negatives uses ``sample_candidates`` and the block modes.  A range
    outside [0, nentity] or with lo > hi gives rows of -1 and the IndexError, an empty one rows of -1 and the "no entity to
    draw" RuntimeError, both at the next synchronising check (``_hip.raise_if_index_errors``)."""
    for name, value in (("G", G), ("K", K)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 1:
            raise ValueError("{} must be a positive integer, got {!r}".format(name, value))
    if isinstance(nentity, bool) or not isinstance(nentity, (int, np.integer)) or not 1 <= int(nentity) < 2 ** 31:
        raise ValueError("nentity must be an integer in [1, 2^31), got {!r}".format(nentity))
    G, K, nentity = int(G), int(K), int(nentity)
    if device is None:
        device = out.device if out is not None else step.device if step is not None else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if step is not None and (step.dtype != torch.int64 or step.numel() != 1 or step.device != device):
        raise ValueError("`step` must be a one-element int64 tensor on {}".format(device))
    if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (G, K) or out.device != device or
                            (K > 1 and out.stride(1) != 1) or (G > 1 and out.stride(0) < K)):
        raise ValueError("`out` must be an int64 [{}, {}] tensor with a unit inner stride on {}".format(G, K, device))
    table = None
    if candidates_range is not None:
        try:
            lo, hi = (int(v) for v in candidates_range)
        except (TypeError, ValueError):
            raise ValueError("candidates_range must be a pair (lo, hi) of integers, got {!r}".format(candidates_range)) from None
        table = torch.tensor([[lo, hi]], dtype=torch.int64, device=device)
    zeros = torch.zeros(G, dtype=torch.int64, device=device)       # every chunk "fixes" entity 0 under relation 0: never read without a filter
    _hip.require_gpu(zeros)
    if out is None:
        out = torch.empty((G, K), dtype=torch.int64, device=device)
    return _hip.kge_candidates_sample(zeros, zeros, K, nentity, None, seed, step, out, table)


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

    def _score(self, sample, et, log_sigmoid, mode="single"):
        ent, rel = self.entity_embedding, self.relation_embedding
        if mode in _SHARED_SIDES:
            return self._score_shared(sample, et, log_sigmoid, mode)
        if mode != "single":
            return self._score_batch(sample, et, log_sigmoid, mode)
        _hip.require_gpu(ent, rel, sample, et)
        gamma, divisor = self._constants()
        if torch.is_grad_enabled() and (ent.requires_grad or rel.requires_grad):
            return KgeScoreFn.apply(ent, rel, sample, et, self.model_name, gamma, divisor, log_sigmoid)
        out = torch.empty((sample.shape[1],), dtype=torch.float32, device=ent.device)
        return _hip.kge_forward(self.model_name, _hip.f32_rows(ent.detach()), _hip.f32_rows(rel.detach()), sample, et, gamma,
                                divisor, log_sigmoid, out)

    def _score_batch(self, sample, et, log_sigmoid, mode):
        """[B, K]: the candidates negatives[b, :] in the place of the positive's tail ('tail-batch') or head ('head-batch')."""
        if mode not in _BATCH_SIDES:
            raise ValueError("mode %s not supported" % mode)
        side = _BATCH_SIDES[mode]
        positive, negatives = sample
        if positive.dim() != 2 or positive.shape[0] != 2:
            raise ValueError("positive must have shape [2, B], got {}".format(tuple(positive.shape)))
        if negatives.dim() != 2 or negatives.shape[0] != positive.shape[1]:
            raise ValueError("negatives must have shape [{}, K], got {}".format(positive.shape[1], tuple(negatives.shape)))
        ent, rel = self.entity_embedding, self.relation_embedding
        _hip.require_gpu(ent, rel, positive, negatives, et)
        gamma, divisor = self._constants()
        fixed = positive[0] if side == "tail" else positive[1]     # the member the candidates do not replace
        negatives = negatives.contiguous()
        if torch.is_grad_enabled() and (ent.requires_grad or rel.requires_grad):
            return KgeBatchScoreFn.apply(ent, rel, fixed, et, negatives, side, self.model_name, gamma, divisor, log_sigmoid)
        out = torch.empty(tuple(negatives.shape), dtype=torch.float32, device=ent.device)
        return _hip.kge_batch_forward(self.model_name, _hip.f32_rows(ent.detach()), _hip.f32_rows(rel.detach()), fixed, et,
                                      negatives, side, gamma, divisor, log_sigmoid, out)

    def _score_shared(self, sample, et, log_sigmoid, mode):
        """[B, K]: the candidates negatives[b // (B // G), :] in the place of the positive's tail ('tail-shared') or head."""
        side = _SHARED_SIDES[mode]
        positive, negatives = sample
        _shared_block(positive, negatives, et)
        ent, rel = self.entity_embedding, self.relation_embedding
        if ent.shape[1] > _hip.KGE_SHARED_MAX_ROW:
            raise ValueError("{}: mode {} takes entity rows of at most {} floats (hidden_dim <= {}), got {}".format(
                self.model_name, mode, _hip.KGE_SHARED_MAX_ROW, _hip.KGE_SHARED_MAX_ROW * self.hidden_dim // ent.shape[1], ent.shape[1]))
        _hip.require_gpu(ent, rel, positive, negatives, et)
        gamma, divisor = self._constants()
        fixed = positive[0] if side == "tail" else positive[1]     # the member the candidates do not replace
        negatives = negatives.contiguous()
        if torch.is_grad_enabled() and (ent.requires_grad or rel.requires_grad):
            return KgeSharedScoreFn.apply(ent, rel, fixed, et, negatives, side, self.model_name, gamma, divisor, log_sigmoid)
        out = torch.empty((positive.shape[1], negatives.shape[1]), dtype=torch.float32, device=ent.device)
        return _hip.kge_shared_forward(self.model_name, _hip.f32_rows(ent.detach()), _hip.f32_rows(rel.detach()), fixed, et,
                                       negatives, side, gamma, divisor, log_sigmoid, out)

    def forward(self, sample, et, mode="single"):
        """``mode="single"``: ``logsigmoid(score)`` [E] of the triples (sample[0, e], et[e], sample[1, e]) (:127-187).
        ``mode="tail-batch"`` / ``"head-batch"`` (:127-136, :150-173): `sample` is a pair ``(positive, negatives)`` -
        positive [2, B], negatives int64 [B, K] (made contiguous if it is not), et [B] - and the result is
        ``logsigmoid(score)`` [B, K] of (positive[0, b], et[b], negatives[b, k]) for 'tail-batch', of (negatives[b, k], et[b],
        positive[1, b]) for 'head-batch': K corrupted tails or heads per positive in one launch, every score the same bits
        as the 'single' mode gives for that triple.
        ``mode="tail-shared"`` / ``"head-shared"``: `sample` is ``(positive, negatives)`` with positive [2, B], et [B] and
        negatives int64 [G, K], 1 <= G <= B and B % G == 0 (``sample_shared_candidates``): the positives are cut into G chunks
        of B // G consecutive ones, positive b belongs to chunk g = b // (B // G) and is scored against the ONE list
        negatives[g, :] of its chunk - ``logsigmoid(score)`` [B, K] of (positive[0, b], et[b], negatives[g, k]) for
        'tail-shared', of (negatives[g, k], et[b], positive[1, b]) for 'head-shared'; G == B is the batch modes' meaning.
        G K entity rows are gathered instead of B K (csrc/kge_shared.hip).  TransE and RotatE evaluate the 'single' mode's
        per-column terms and add them in column order; DistMult and ComplEx contract a prepared query row with the
        candidate rows on the fp32 matrix cores, so for these two bitwise equality with ``mode="single"`` is NOT given (nor
        required): every score is held to the same per-element bound against float64 (tests/test_gpu_kge_shared.py).  Entity
        rows of at most 128 floats (the ``rank`` limit), a wrong shape or a G that does not divide B: ValueError with the
        shapes.  A bad positive id gives NaN in its row, a bad candidate id NaN in its column of its chunk.
        Any other mode raises ``ValueError("mode %s not supported")``; before the batch modes existed every string was
        accepted and ignored, and no caller in the reference, the examples or the tests passes one.  An id outside its
        table gives NaN for that triple (a bad positive: its whole row) and raises IndexError at the next synchronising
        check (``_hip.raise_if_index_errors``, ``utils.relation_metrics``), as the decoders do."""
        return self._score(sample, et, True, mode)

    def score(self, sample, et, mode="single"):
        """The raw scores (before the log-sigmoid), [E] or - in the batch modes - [B, K]: differentiable; for losses on raw
        scores (``self_adversarial_loss``), metrics and tests."""
        return self._score(sample, et, False, mode)

    def negative_sampling_loss(self, positive, et, negatives, mode="tail-batch", adversarial_temperature=None,
                               subsampling_weight=None):
        """The loss of one mini-batch: ``negative_sampling_loss(self.score(positive, et), self.score((positive, negatives),
        et, mode), adversarial_temperature, subsampling_weight)`` - positive [2, B], et [B], negatives int64 [B, K]
        (``sample_candidates``) standing for the tails ('tail-batch') or the heads ('head-batch'), or - with
        ``mode="tail-shared"`` / ``"head-shared"`` - negatives int64 [G, K] (``sample_shared_candidates``), one list per
        chunk of B // G positives.  The two scorers and one launch for the loss; ``loss.backward()`` is the loss's one
        launch and the two scorers' own backward."""
        if mode in _SHARED_SIDES:
            if negatives.dim() == 2 and negatives.shape[1] < 1:
                raise ValueError("negatives must have shape [G, K] with K >= 1, got {}".format(tuple(negatives.shape)))
            _shared_block(positive, negatives, et)
            if subsampling_weight is not None and tuple(subsampling_weight.shape) != (positive.shape[1],):
                raise ValueError("subsampling_weight must have shape [{}], got {}".format(
                    positive.shape[1], tuple(subsampling_weight.shape)))
            return negative_sampling_loss(self.score(positive, et), self.score((positive, negatives), et, mode),
                                          adversarial_temperature, subsampling_weight)
        if mode not in _BATCH_SIDES:
            raise ValueError("mode %s not supported" % mode)
        if positive.dim() != 2 or positive.shape[0] != 2 or positive.shape[1] < 1:
            raise ValueError("positive must have shape [2, B] with B >= 1, got {}".format(tuple(positive.shape)))
        if negatives.dim() != 2 or negatives.shape[0] != positive.shape[1] or negatives.shape[1] < 1:
            raise ValueError("negatives must have shape [{}, K] with K >= 1, got {}".format(
                positive.shape[1], tuple(negatives.shape)))
        if subsampling_weight is not None and tuple(subsampling_weight.shape) != (positive.shape[1],):
            raise ValueError("subsampling_weight must have shape [{}], got {}".format(
                positive.shape[1], tuple(subsampling_weight.shape)))
        return negative_sampling_loss(self.score(positive, et), self.score((positive, negatives), et, mode),
                                      adversarial_temperature, subsampling_weight)

    def _eval_operands(self, *index):
        ent, rel = self.entity_embedding, self.relation_embedding
        _hip.require_gpu(ent, rel, *index)
        return _hip.f32_rows(ent.detach()), _hip.f32_rows(rel.detach())

    def rank(self, sample, et, side="tail", known=None, candidates=None):
        """Filtered ranking of the triples (h, r, t) = (sample[0], et, sample[1]) against every candidate entity:
        ``(greater, ties)``, int32 [E] each.  ``side="tail"``: the candidates t' != t whose (r, h, t') is not in `known`
        (a KnownPairs, None: no filter) with NOT (s(h, r, t') <= s(h, r, t)) and with s(h, r, t') == s(h, r, t) - a
        non-finite score never flatters the model: a NaN true score puts every admitted candidate into `greater` (the
        true triple ranks last, ties = 0), a NaN candidate counts as greater than any true score, -inf and +inf compare
        as numbers (equal infinities tie, a -inf candidate is greater than nothing), the filter is applied before the
        comparison, and non-finite scores set no bit of the error word (``ranking_metrics`` returns numbers: a table that
        went to NaN reports an MRR near 0, not 1).  ``side="head"``: the
        candidates h' != h of (., r, t), filtered by a KnownPairs whose rows are keyed (r, t) - one built from the FLIPPED
        lists, ``KnownPairs([(ei.flip(0), et), ...], nentity, nrelation)``; the filter given for the tail side does not
        serve the head side (TransE, ComplEx and RotatE are not symmetric; neither are their known pairs).  Raw scores
        (``score``), not their log-sigmoid; the true triple's score is the scan's own value for that candidate.  No
        autograd, no host synchronisation: an id out of range gives -1 / -1 and the IndexError at the next check
        (``utils.ranking_metrics`` / ``_hip.raise_if_index_errors``); ``utils.ranking_metrics`` turns the counts into MRR
        and Hits@k.  Entity rows of at most 128 floats (hidden_dim <= 128 for TransE and DistMult, <= 64 for ComplEx and
        RotatE): ValueError beyond, there is no torch fallback.  `candidates`: an int64 [nrelation, 2] tensor on the
        device, row r = (lo, hi): a query of relation r is ranked against the candidates lo <= c < hi only (on top of the
        rules above) - the valid tails for ``side="tail"``, the valid heads for ``side="head"``
        (``utils.candidate_ranges``).  The true partner may lie outside its range; an empty range gives 0 / 0; a range
        outside [0, nentity] or with lo > hi is found on the device and gives -1 / -1 and the IndexError.  The counts are
        those of the unranged call over the range, bit for bit; queries sorted by relation scan only their range.
        Wrong shape, dtype or device: ValueError."""
        candidates = _hip.candidate_table(candidates, self.relation_embedding.shape[0], self.entity_embedding.device)
        ent, rel = self._eval_operands(sample, et)
        gamma, divisor = self._constants()
        with torch.no_grad():
            return _hip.kge_rank(self.model_name, ent, rel, sample, et, gamma, divisor, side, known, candidates)

    def top_k(self, entities, et, k, side="tail", known=None, candidates=None):
        """The `k` (1..64) best partners of every query (entities[q], et[q]) that are not in `known`: the tails of
        (entities[q], r, .) for ``side="tail"``, the heads of (., r, entities[q]) for ``side="head"`` (`known` keyed as for
        ``rank``: built from the flipped lists for the head side).  ``(scores, ids)``: fp32 raw scores [Q, k] and int64
        ids [Q, k], by score descending then id ascending, padded with -inf / -1 when fewer than k candidates remain.  A
        NaN or -inf score never enters, +inf enters, equal scores order by ascending id; a query whose whole candidate
        row is NaN (a NaN fixed entity) gets a full row of padding, not the NaN / -1 of an id out of range.  ComplEx on
        the head side scores the relation and tail folded into one row first (the header says which kind of value an
        infinite entry then gives).  No
        autograd, no host synchronisation (ids out of range: NaN / -1 and the IndexError at the next check).  Width limit
        as for ``rank``.  `candidates` as for ``rank``: only the entities of the relation's range enter the list (an empty
        range: a row of padding; an invalid one: NaN / -1 and the IndexError)."""
        candidates = _hip.candidate_table(candidates, self.relation_embedding.shape[0], self.entity_embedding.device)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("k must be an integer in [1, 64], got {!r}".format(k))
        ent, rel = self._eval_operands(entities, et)
        gamma, divisor = self._constants()
        with torch.no_grad():
            return _hip.kge_topk(self.model_name, ent, rel, entities, et, int(k), gamma, divisor, side, known, candidates)
