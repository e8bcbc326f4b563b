"""The KGE baselines' Python layer and the float64 reference of the GPU tests, without a GPU.

`kge_cases` restates KGEModel.forward (baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:127-235) in torch; here it is
held to tests/golden/kge_cases.npz (the reference class's own runs) at 1e-6 absolute, precision by precision: in fp32
against the fp32 ``out`` / ``out_neg``, in float64 against ``out64`` / ``out_neg64``, ``loss64`` and ``grad64``.  (The float64
formulation against the fp32 ``out`` is off by up to 2.7e-6 - TransE, H = 32 - and so is the reference's own float64 run:
that distance is the rounding of the reference's fp32 sum over 32 columns, not a property of the restatement.  Measured:
fp32 against ``out`` 0 in all eight cases, float64 against ``out64`` 0, against ``grad64`` <= 1.4e-17.)"""
import pytest
import torch
import torch.nn.functional as F

import gripnet_amd
import kge_cases as kc

CASES = [m + "." + s for m in kc.MODELS for s in ("small", "driver")]


def _info(fx, tag):
    return next(c for c in fx.meta["cases"] if c["tag"] == tag)


@pytest.mark.parametrize("tag", CASES)
def test_module_matches_the_reference_layout(golden, tag):
    fx = golden("kge_cases")
    c = _info(fx, tag)
    torch.manual_seed(0)
    m = gripnet_amd.KGEModel(c["model"], c["n"], c["R"], c["H"], c["gamma"])
    want = {k[len(tag) + 4:]: tuple(v.shape) for k, v in fx.arrays.items() if k.startswith(tag + ".sd.")}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert list(want) == ["gamma", "embedding_range", "entity_embedding", "relation_embedding"]
    assert sorted(k for k, p in m.named_parameters() if not p.requires_grad) == sorted(c["frozen"]) == ["embedding_range", "gamma"]
    assert (m.model_name, m.nentity, m.nrelation, m.hidden_dim, m.epsilon) == (c["model"], c["n"], c["R"], c["H"], 2.0)
    assert (m.entity_dim, m.relation_dim) == (c["entity_dim"], c["relation_dim"]) == kc.dims(c["model"], c["H"])
    rho = c["embedding_range"]
    assert m.embedding_range.item() == rho == kc.embedding_range(c["gamma"], c["H"]) and m.gamma.item() == c["gamma"]
    for table in (m.entity_embedding.detach(), m.relation_embedding.detach()):
        assert float(table.abs().max()) <= rho and float(table.abs().max()) > 0.8 * rho        # uniform in +-range
        assert abs(float(table.mean())) < 0.2 * rho
    m.load_state_dict({k[len(tag) + 4:]: fx.t(k) for k in fx.arrays if k.startswith(tag + ".sd.")})


def test_constructor_errors():
    with pytest.raises(ValueError, match="model TransH not supported"):
        gripnet_amd.KGEModel("TransH", 5, 2, 4, 12.0)
    with pytest.raises(ValueError, match="RotatE should use --double_entity_embedding"):
        gripnet_amd.KGEModel("RotatE", 5, 2, 4, 12.0, double_relation_embedding=True)
    # (ComplEx forces both doublings, as the reference does: its check cannot fire; the condition is spelled all the same)
    m = gripnet_amd.KGEModel("ComplEx", 5, 2, 4, 12.0)
    assert (m.entity_dim, m.relation_dim) == (8, 8)
    m = gripnet_amd.KGEModel("TransE", 5, 2, 4, 12.0, double_entity_embedding=True, double_relation_embedding=True)
    assert (m.entity_dim, m.relation_dim) == (8, 8)


@pytest.mark.parametrize("model", kc.MODELS)
def test_no_cpu_fallback(model):
    m = gripnet_amd.KGEModel(model, 5, 2, 4, 12.0)
    sample, et = torch.zeros(2, 3, dtype=torch.long), torch.zeros(3, dtype=torch.long)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(sample, et)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.score(sample, et)


@pytest.mark.parametrize("tag", CASES)
def test_formulation_reproduces_the_fixture(golden, tag):
    fx = golden("kge_cases")
    c = _info(fx, tag)
    g = lambda k: fx.t(tag + "." + k)
    ent, rel, sample, neg, et = g("sd.entity_embedding"), g("sd.relation_embedding"), g("sample"), g("neg"), g("et")
    assert bool((et[1:] >= et[:-1]).all())
    for lst, key in ((sample, "out"), (neg, "out_neg")):
        y32 = kc.log_sigmoid_score(c["model"], ent, rel, lst, et, c["gamma"])
        y64 = kc.log_sigmoid_score(c["model"], ent.double(), rel.double(), lst, et, c["gamma"])
        assert float((y32 - g(key)).abs().max()) <= 1e-6
        assert float((y64 - g(key + "64")).abs().max()) <= 1e-6
    e, r = ent.double().requires_grad_(True), rel.double().requires_grad_(True)
    loss = kc.loss_expr(kc.log_sigmoid_score(c["model"], e, r, sample, et, c["gamma"]),
                        kc.log_sigmoid_score(c["model"], e, r, neg, et, c["gamma"]))
    loss.backward()
    assert abs(float(loss.detach()) - float(g("loss64"))) <= 1e-6
    assert float((e.grad - g("grad64.entity_embedding")).abs().max()) <= 1e-6
    assert float((r.grad - g("grad64.relation_embedding")).abs().max()) <= 1e-6
    # what the small case is there for
    if c["size"] == "small":
        assert c["unused_entities"] and c["empty_relations"] and bool((sample[0] == sample[1]).any())
        assert float(g("grad64.entity_embedding")[c["unused_entities"]].abs().max()) == 0.0
        assert float(g("grad64.relation_embedding")[c["empty_relations"]].abs().max()) == 0.0


def test_zero_subgradients_are_torch_s():
    """h == t and r = 0: TransE's h + r - t and RotatE's (a, b) are exactly zero in every column; both return
    logsigmoid(gamma) and all-zero gradients (sign(0) = 0; a zero-length (a, b) contributes nothing)."""
    for model in ("TransE", "RotatE"):
        c = kc.case(model, 6, 2, 4, 10, seed=2)
        c.rel.zero_()
        c.sample[1] = c.sample[0]
        y = kc.log_sigmoid_score(model, c.ent.double(), c.rel.double(), c.sample, c.et, c.gamma)
        assert torch.equal(y, F.logsigmoid(torch.full((10,), c.gamma, dtype=torch.float64)))
        for dtype in (torch.float32, torch.float64):
            ge, gr = kc.reference_gradients(model, c.ent, c.rel, c.sample, c.et, c.gamma, torch.ones(10), dtype)
            assert float(ge.abs().max()) == 0.0 and float(gr.abs().max()) == 0.0


@pytest.mark.parametrize("model", kc.MODELS)
def test_case_builders(model):
    c = kc.gradient_case(model)
    for i, want in enumerate(c.counts):
        assert int((c.sample[0] == i).sum()) == want and int((c.sample[1] == i).sum()) == want
    assert c.counts[:3] == [kc.CHUNK - 1, kc.CHUNK, kc.CHUNK + 1] and c.counts[3] > 2 * kc.CHUNK
    assert not bool((c.sample == c.unused_entity).any())
    assert all(not bool((c.et == r).any()) for r in c.empty_relations) and c.empty_relations == (0, c.R - 1)
    assert bool((c.et[1:] >= c.et[:-1]).all())
    same = c.sample[0] == c.sample[1]
    assert int(same.sum()) >= 40 and bool(((c.et == c.zero_relation) & same & (c.sample[0] == c.same_entity)).any())
    assert float(c.rel[c.zero_relation, c.zero_column]) == 0.0
    ge, gr = kc.reference_gradients(model, c.ent, c.rel, c.sample, c.et, c.gamma, torch.ones(c.E), torch.float64)
    assert float(ge[c.unused_entity].abs().max()) == 0.0 and float(gr[list(c.empty_relations)].abs().max()) == 0.0
    # the tables sit on the grid that makes h + r - t exact
    assert torch.equal(torch.round(c.ent / kc.GRID) * kc.GRID, c.ent)
    # saturation: about +-80 where the model can get there, finite float64 gradients
    s = kc.saturated_case(model)
    s64 = kc.raw_score(model, s.ent.double(), s.rel.double(), s.sample, s.et, s.gamma)
    assert float(s64.min()) <= -60.0
    if model in ("DistMult", "ComplEx"):
        assert float(s64.max()) >= 50.0 and float(s64.abs().max()) <= 81.0
    # log-sigmoid values too small to hold a relative bound: at most 1 % of every case's elements
    for k in [c, s, kc.case(model, 20000, 37, 32, 300000, seed=3)] + [kc.shape_case(model, H, E) for H in kc.SHAPE_H for E in kc.SHAPE_E if E]:
        y64 = kc.log_sigmoid_score(model, k.ent.double(), k.rel.double(), k.sample, k.et, k.gamma)
        assert float((y64.abs() < 2.0 ** -100).double().mean()) <= 0.01
    # the shape cases of one (model, H) are prefixes of one list on the same tables
    whole = kc.shape_case(model, 36, 257)
    for E in kc.SHAPE_E:
        part = kc.shape_case(model, 36, E)
        assert part.E == E and torch.equal(part.sample, whole.sample[:, :E]) and torch.equal(part.et, whole.et[:E])
        assert torch.equal(part.ent, whole.ent) and torch.equal(part.rel, whole.rel)
    # bad ids: every kind, and the list without them is the case's own
    sample, et, good = kc.with_bad_ids(c)
    assert int((~good).sum()) == 6 and torch.equal(sample[:, good], c.sample) and torch.equal(et[good], c.et)
    sample, et, good = kc.with_bad_ids(c, relations=False)
    assert int((~good).sum()) == 4 and bool((et[1:] >= et[:-1]).all()) and torch.equal(sample[:, good], c.sample)
    assert bool(((sample[:, ~good] < 0) | (sample[:, ~good] >= c.n)).any(dim=0).all())
