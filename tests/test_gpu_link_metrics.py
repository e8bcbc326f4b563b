"""Per-relation AUPRC / AUROC / AP on the device (gripnet_amd/csrc/metrics.hip through utils.relation_metrics) against the
float64 definitions of tests/metric_cases.py, at 1e-9 absolute per relation and metric: scores outside (0, 1) - logits,
signed zeros, denormals, neighbours one ulp apart -, every size at which the chunk sort or the merge changes shape,
windows of the other class at and beyond what stays in LDS, tie groups that cross tiles, 1500 relations, no edges at all,
a plan used again with other scores, and what must not change the bits: the order of the scores, the plan's age.

tests/test_metrics_host.py holds the reference to scikit-learn and runs every case's own check of its condition.
Every test prints `metric-distance[...]`, the largest distance from the reference it saw (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import metric_cases as mc
from gripnet_amd import _hip
from gripnet_amd.utils import relation_metrics

pytestmark = pytest.mark.gpu


def run(pos, neg, rl):
    """[3, R] float64 numpy of relation_metrics; `pos` / `neg` as given (already on the GPU)."""
    out = relation_metrics(pos, neg, rl)
    assert all(o.dtype == torch.float64 and o.shape == (rl.shape[0],) for o in out)
    return torch.stack(out).cpu().numpy()


def run_fresh(pos, neg, rl, gpu):
    """The same through a MetricsPlan built for this call and a workspace of its own."""
    plan = _hip.MetricsPlan(rl, gpu)
    p, n = pos.to(gpu, torch.float32).contiguous(), neg.to(gpu, torch.float32).contiguous()
    out = torch.empty((3, plan.R), dtype=torch.float64, device=gpu)
    ws = plan.workspace()
    _hip._call("gn_link_metrics_planned_f32", plan._h, p.data_ptr(), n.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
               _hip.stream_ptr(gpu))
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def library(name, gpu):
    pos, neg, sizes = mc.case(name)
    out = run(pos.to(gpu), neg.to(gpu), mc.range_list(sizes))
    out.setflags(write=False)
    return out


def held(what, got, ref):
    d = mc.distance(got, ref)
    print("metric-distance[{}]: {:.3g}".format(what, d))
    assert d <= mc.TOL, "{}: {:.3g} from the reference".format(what, d)
    return d


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_against_float64_reference(gpu, name):
    got, ref = library(name, gpu), mc.reference(name)
    if name in mc.SIGNED_ZERO_CASES or name == "separated_classes":
        print("values[{}]: library {} reference {}".format(name, got[:, :2].T.tolist(), ref[:, :2].T.tolist()))
    held(name, got, ref)


def test_signed_zeros_tie(gpu):
    """[-0.0] against [+0.0] is one tie: AUROC 0.5, AP 0.5, AUPRC 0.75 - not the 0 / 0.5 / 0.25 of +0.0 ranked above -0.0."""
    got = library("hand_signed_zero", gpu)
    assert got[:, 0].tolist() == [0.75, 0.5, 0.5]


def test_separated_classes_are_exact(gpu):
    """No positive among the negatives: AUROC is 1.0, and 0.0 the other way round, to the bit."""
    got = library("separated_classes", gpu)
    print("auroc[separated_classes]: {!r} {!r}".format(float(got[1, 0]), float(got[1, 1])))
    assert got[1, 0] == 1.0 and got[1, 1] == 0.0


def test_no_edges_is_all_nan(gpu):
    got = library("no_edges", gpu)
    assert got.shape == (3, 3) and np.isnan(got).all()


def test_many_relations_empty_ones_in_place(gpu):
    sizes = np.array(mc.case("many_relations")[2])
    got = library("many_relations", gpu)
    assert np.array_equal(np.isnan(got).all(axis=0), sizes == 0) and np.array_equal(np.isnan(got).any(axis=0), sizes == 0)
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, -1]).all()


# ---- a plan used again ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(4097, 300), (8193, 300)], ids=["one-merge-round", "two-merge-rounds"])
def test_plan_reused_with_other_scores(gpu, sizes):
    """One range-list tensor, so one kept plan and one workspace: scores A, scores B, scores A again.  What an earlier call
    left in the two key buffers (an odd number of merge rounds ends in the second, an even one in the first) must not
    show: every result has the bits of a plan built for that call alone."""
    assert mc.merge_rounds(sizes) == (1 if sizes[0] == 4097 else 2)
    g, E, rl = torch.Generator().manual_seed(61 + sizes[0]), sum(sizes), mc.range_list(sizes)
    a = (torch.randn(E, generator=g) + 0.5, torch.randn(E, generator=g))
    b = (torch.round(4 * torch.randn(E, generator=g)) / 4 - 0.25, torch.round(4 * torch.randn(E, generator=g)) / 4)
    assert mc.has_both_zeros(b[1])                                    # (rounding keeps the sign of what it rounds to zero)
    kept = None
    for tag, (pos, neg) in (("a", a), ("b", b), ("a again", a)):
        got = run(pos.to(gpu), neg.to(gpu), rl)
        plan = _hip._range_plans.get(rl, gpu)
        assert plan is not _hip.MISS and (kept is None or plan is kept), "the plan of the first call serves the later ones"
        kept = plan
        assert same_bits(got, run_fresh(pos, neg, rl, gpu)), tag
        held("reuse {} {}".format(sizes, tag), got, mc.ref_relations(pos, neg, sizes))


def test_plan_cache_eviction_changes_nothing(gpu):
    """Five range lists of one E in rotation through the four kept plans: every call builds its plan anew, the bits stay."""
    g, E = torch.Generator().manual_seed(67), 700
    pos, neg = torch.round(8 * torch.randn(E, generator=g)) / 8 + 0.25, torch.round(8 * torch.randn(E, generator=g)) / 8
    splits = [(700,), (300, 400), (1, 0, 699), (257, 256, 187), (100, 100, 100, 100, 300)]
    lists = [mc.range_list(s) for s in splits]
    pg, ng = pos.to(gpu), neg.to(gpu)
    first = [run(pg, ng, rl) for rl in lists]
    assert _hip._range_plans.get(lists[0], gpu) is _hip.MISS, "a fifth list pushes the first one out"
    for _ in range(2):
        for rl, want in zip(lists, first):
            assert same_bits(run(pg, ng, rl), want)
    for s, got in zip(splits, first):
        held("rotation {}".format(s), got, mc.ref_relations(pos, neg, s))


# ---- what must not change the bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sort_sizes_random", "sort_sizes_eighths", "tie_groups_across_tiles", "relu_signed_zeros",
                                  "window_other_class_tied"])
def test_order_inside_a_relation_does_not_matter(gpu, name):
    pos, neg, sizes = mc.case(name)
    g = torch.Generator().manual_seed(71)
    p, n = pos.clone(), neg.clone()
    for s, e in mc.range_list(sizes).tolist():
        p[s:e] = pos[s:e][torch.randperm(e - s, generator=g)]
        n[s:e] = neg[s:e][torch.randperm(e - s, generator=g)]          # its own permutation: the pairing means nothing
    assert not torch.equal(p, pos) and not torch.equal(n, neg)
    assert same_bits(run(p.to(gpu), n.to(gpu), mc.range_list(sizes)), library(name, gpu))


# ---- inputs that are converted first ------------------------------------------------------------------------------------------
INPUT_SIZES = (300, 5000)


def test_strided_views(gpu):
    """Every second element of a buffer whose other elements would change every metric."""
    pos, neg, sizes = mc.case("logits")
    views = []
    for v in (pos, neg):
        buf = torch.full((2 * v.numel(),), 1e30, device=gpu)
        buf[::2] = v.to(gpu)
        views.append(buf[::2])
    assert views[0].stride() == (2,) and not views[0].is_contiguous()
    got = run(views[0], views[1], mc.range_list(sizes))
    assert same_bits(got, library("logits", gpu))
    held("stride 2", got, mc.reference("logits"))


def test_float64_scores_are_rounded_to_fp32_first(gpu):
    """Scores that differ in float64 and tie once rounded: the library compares fp32 values, so do the reference's inputs."""
    g, E = torch.Generator().manual_seed(73), sum(INPUT_SIZES)
    make = lambda shift: (torch.round(8 * torch.randn(E, generator=g)) / 8 + shift).double() * (1 + 1e-11 * torch.randn(E, generator=g).double())
    pos, neg = make(0.25), make(0.0)
    ref = mc.ref_relations(pos.float(), neg.float(), INPUT_SIZES)
    unrounded = np.stack([mc.ref_link_metrics(pos[s:e].numpy(), neg[s:e].numpy()) for s, e in mc.range_list(INPUT_SIZES).tolist()], axis=1)
    assert np.abs(unrounded - ref).min() > 1e3 * mc.TOL, "the rounding must show in every figure"
    held("float64 scores", run(pos.to(gpu), neg.to(gpu), mc.range_list(INPUT_SIZES)), ref)


def test_bf16_scores_convert_exactly(gpu):
    g, E = torch.Generator().manual_seed(79), sum(INPUT_SIZES)
    pos, neg = (3 * torch.randn(E, generator=g) + 0.5).bfloat16(), (3 * torch.randn(E, generator=g)).bfloat16()
    assert torch.equal(pos.float().bfloat16(), pos)
    held("bf16 scores", run(pos.to(gpu), neg.to(gpu), mc.range_list(INPUT_SIZES)), mc.ref_relations(pos.float(), neg.float(), INPUT_SIZES))
