"""The gene stack in three launches (layers.gene_stack_to_external): the last gene layer's 16 -> 16 transform is applied by the
external layer's launch to the rows it gathers, its gather reads a table the first layer's gather wrote.

Reference: the float64 oracle of the two module calls.  GN_BLOCKED_ANY=1 lifts the size thresholds of the LDS-staged plans, so
that small gene graphs take them; GN_ENABLE_CHAIN=1 switches the chained launches on."""
import functools
import os
import sys

import pytest
import torch

from gripnet_amd import _hip
from gripnet_amd.layers import gene_stack_path, gene_stack_to_external
from gripnet_amd.pipeline import PoseModel
from gripnet_amd.synth import Data, make_pose
from gripnet_amd.utils import set_arithmetic, set_table_storage
from oracle import gripnet_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = 2e-5
gpu_test = pytest.mark.gpu
N_D = 128
HUB, EMPTY_DRUG, BUSY_DRUG = 5, 3, 7


def err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return (a - b).abs().max().item()


@pytest.fixture
def any_size(monkeypatch):
    monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    monkeypatch.setenv("GN_ENABLE_CHAIN", "1")                     # (the chained launches are opt-in)


def make_case(n_g, seed=7):
    """PoSE-shaped data on n_g genes and 128 drugs: gene HUB takes 600 edges, the last five genes keep nothing but their self
    loop, drug EMPTY_DRUG has no gene, drug BUSY_DRUG more than 64 (beyond a padded row of the external plan)."""
    data = make_pose("small", seed=seed, n_g=n_g, e_gg_dir=10 * n_g, n_d=N_D, e_gd=2000)
    g = torch.Generator().manual_seed(seed + 1)
    a = torch.randint(0, n_g - 5, (2, 10 * n_g), generator=g)
    a[1, :600] = HUB
    a = a[:, a[0] != a[1]]
    data.gg_edge_index = torch.cat([a, a.flip(0)], dim=1).long()
    data.edge_weight = torch.ones(data.gg_edge_index.shape[1])
    data.n_gg_edge = int(data.gg_edge_index.shape[1])
    gd = data.gd_edge_index.clone()
    gd[1, :100] = BUSY_DRUG
    gd[1][gd[1] == EMPTY_DRUG] = EMPTY_DRUG + 1
    data.gd_edge_index = gd
    return data


def make_model(data, seed=3, **kw):
    """Random biases everywhere; b2 moved so that about half of every column of h2 is cut by the ReLU."""
    torch.manual_seed(seed)
    model = PoseModel(data.n_g_node, data.n_d_node, data.n_dd_edge_type, **kw)
    convs = list(model.gg.conv_list)
    for c in convs + [model.gd.conv]:
        c.bias.data.normal_(std=0.3)
    sd = {k: v.double() for k, v in model.state_dict().items()}
    ei, norm = orc.gcn_norm(data.gg_edge_index, data.n_g_node, data.edge_weight.double(), False, torch.float64)
    h = sd["gg.embedding"]
    for i, c in enumerate(convs[:-1]):
        h = torch.relu(orc.gcn_propagate(h @ sd["gg.conv_list.{}.weight".format(i)], ei, norm, sd["gg.conv_list.{}.bias".format(i)]))
    pre = orc.gcn_propagate(h @ convs[-1].weight.data.double(), ei, norm, None)
    convs[-1].bias.data.copy_(-pre.median(dim=0).values.float())
    return model


def oracle(model, data):
    """(gene concat, external output, h2) of the float64 oracle."""
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    z_gg = orc.homo_forward(sd, "gg.", None, data.gg_edge_index, data.edge_weight.double(), if_catout=True)
    z_gd = orc.inter_forward(sd, "gd.", z_gg, data.gd_edge_index, None, if_relu=True, mod="cat")
    return z_gg, z_gd, z_gg[:, -model.gg.out_dim:]


@functools.lru_cache(maxsize=None)
def case(n_g):
    """One graph, one parameter set and its reference per size, shared by the tests (none of them changes it: they work on
    copies of the model)."""
    data = make_case(n_g)
    model = make_model(data)
    return data, model.state_dict(), oracle(model, data)


def on_gpu(n_g, gpu):
    data, state, ref = case(n_g)
    model = PoseModel(data.n_g_node, data.n_d_node, data.n_dd_edge_type)
    model.load_state_dict(state)
    return copy_to(data, gpu), model.to(gpu), ref


def copy_to(data, device):
    """(Data.to moves in place: the shared CPU case stays where it is)"""
    return Data(**{k: getattr(data, k) for k in data.keys()}).to(device)


def chained(model, data):
    with torch.no_grad():
        out = gene_stack_to_external(model.gg, model.gd, data.gg_edge_index, data.edge_weight, data.gd_edge_index)
    return out, gene_stack_path(model.gg)


def separate(model, data):
    z = model.gg(None, data.gg_edge_index, edge_weight=data.edge_weight, if_catout=True)
    return model.gd(z, data.gd_edge_index, mod="cat", if_relu=True)


@gpu_test
@pytest.mark.parametrize("n_g", [1037, 2000, 4099])
def test_chained_vs_oracle_at_awkward_sizes(gpu, any_size, n_g):
    data, model, (_, z_gd, _) = on_gpu(n_g, gpu)
    cpu = case(n_g)[0]
    deg = torch.bincount(cpu.gg_edge_index[1], minlength=n_g)
    assert deg[HUB] >= 500 and (deg[-5:] == 0).all()                   # a hub; genes whose only edge is the self loop
    per_drug = torch.bincount(cpu.gd_edge_index[1], minlength=N_D)
    assert per_drug[EMPTY_DRUG] == 0 and per_drug[BUSY_DRUG] > 64
    out, path = chained(model, data)
    assert path == "chained"
    e = err(out, z_gd)
    print("n_g {}: max |chained - oracle| = {:.3e}".format(n_g, e))
    assert e <= TIGHT


def test_reference_exercises_the_relu():
    """On the CPU reference: the ReLU of the deferred layer cuts between a quarter and three quarters of h2 and no column
    is all zero or all positive - a tail transform applied behind the sum, or without its ReLU, is far from such a reference."""
    for n_g in (1037, 2000, 4099):
        h2 = case(n_g)[2][2]
        zeros = (h2 == 0).double()
        assert 0.25 <= zeros.mean().item() <= 0.75, zeros.mean().item()
        col = zeros.mean(dim=0)
        assert (col > 0).all() and (col < 1).all(), col


@gpu_test
def test_wrong_order_or_no_relu_would_fail_by_far(gpu, any_size):
    """What the comparison of the first test can tell apart: the same stack with the ReLU of the last layer left out is
    orders of magnitude beyond TIGHT from the reference."""
    data, model, (z_gg, z_gd, _) = on_gpu(2000, gpu)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    ei, norm = orc.gcn_norm(data.gg_edge_index.cpu(), 2000, None, False, torch.float64)
    h1 = z_gg[:, 32:48]
    no_relu = orc.gcn_propagate(h1 @ sd["gg.conv_list.1.weight"], ei, norm, sd["gg.conv_list.1.bias"])
    wrong = orc.inter_forward(sd, "gd.", torch.cat([z_gg[:, :48], no_relu], dim=1), data.gd_edge_index.cpu(), None)
    assert err(wrong, z_gd) > 100 * TIGHT
    out, _ = chained(model, data)
    assert err(out, z_gd) <= TIGHT


@gpu_test
def test_fresh_plan_first(gpu, any_size):
    """The very first gene launches of a new model are the chained ones: no transform has ever written the second layer's
    table, whose rows beyond the last node (1,152 table rows for 1,037 genes and the zero row) must read as zeros."""
    data, model, (_, z_gd, _) = on_gpu(1037, gpu)
    assert model.gg.conv_list[1].cached_result is None
    out, path = chained(model, data)
    assert path == "chained"
    assert err(out, z_gd) <= TIGHT


@gpu_test
def test_no_stale_state_between_paths(gpu, any_size):
    data, model, _ = on_gpu(2000, gpu)
    with torch.no_grad():
        sep0 = separate(model, data).clone()
    train0 = model.encode(data).detach().clone()
    first, path = chained(model, data)
    assert path == "chained"
    first = first.clone()
    with torch.no_grad():
        assert torch.equal(separate(model, data), sep0)
    again, path = chained(model, data)
    assert path == "chained" and torch.equal(again, first)
    assert torch.equal(model.encode(data).detach(), train0)
    assert gene_stack_path(model.gg) == "separate"                   # (encode with gradients: the four-launch path)
    for _ in range(3):                                               # (the third call replays the memoised launches)
        again, path = chained(model, data)
        assert path == "chained" and torch.equal(again, first)
    with torch.no_grad():
        assert torch.equal(separate(model, data), sep0)


def _fallback_cases():
    def widths(data, gpu):
        return make_model(data, gg_nhids=[15, 17, 16]).to(gpu), data

    def weighted(data, gpu):
        g = torch.Generator().manual_seed(1)
        data.edge_weight = torch.rand(data.gg_edge_index.shape[1], generator=g) + 0.5
        return make_model(data).to(gpu), data

    def bf16(data, gpu):
        model = make_model(data).to(gpu)
        set_table_storage(model, "bf16")
        return model, data

    def fast(data, gpu):
        model = make_model(data).to(gpu)
        set_arithmetic(model, "fast")
        return model, data

    def plain(data, gpu):
        return make_model(data).to(gpu), data
    return {"widths_15_17_16": widths, "weighted_graph": weighted, "bf16_storage": bf16, "fast_arithmetic": fast,
            "blocked_disabled": plain, "grad_enabled": plain, "chain_not_enabled": plain}


@gpu_test
@pytest.mark.parametrize("name", sorted(_fallback_cases()))
def test_fallbacks_are_todays_bits(gpu, any_size, monkeypatch, name):
    data = make_case(2000)
    model, data = _fallback_cases()[name](data, gpu)
    data = data.to(gpu)
    if name == "blocked_disabled":
        monkeypatch.setenv("GN_DISABLE_BLOCKED", "1")
    if name == "chain_not_enabled":
        monkeypatch.delenv("GN_ENABLE_CHAIN")
    with torch.set_grad_enabled(name == "grad_enabled"):
        want = separate(model, data)
        got = gene_stack_to_external(model.gg, model.gd, data.gg_edge_index, data.edge_weight, data.gd_edge_index)
    assert gene_stack_path(model.gg) == "separate"
    assert torch.equal(got.detach(), want.detach())
    assert got.requires_grad == want.requires_grad


@gpu_test
@pytest.mark.parametrize("how", ["memoised", "recorded"])
def test_parameters_by_pointer_not_by_value(gpu, any_size, monkeypatch, how):
    data, model, (_, z_gd, _) = on_gpu(2000, gpu)
    replays = []
    replay = _hip.replay
    monkeypatch.setattr(_hip, "replay", lambda calls: (replays.append(len(calls)), replay(calls))[1])
    if how == "memoised":
        out = None
        for _ in range(6):                         # (the output freed before the next call: the allocator hands out its address again)
            out = None
            out, path = chained(model, data)
            assert path == "chained"
        assert replays and set(replays) == {3}     # run, recorded, then replayed: three entry points per step
    else:
        chained(model, data)
        with _hip.Recorder() as rec:
            out, path = chained(model, data)
        assert path == "chained" and len(rec.calls) == 3
    assert err(out, z_gd) <= TIGHT
    c2, cd = model.gg.conv_list[1], model.gd.conv
    versions = [p._version for p in (c2.weight, c2.bias, cd.weight)]
    g = torch.Generator().manual_seed(11)
    c2.weight.data.mul_(-0.7)                      # (in place through .data: same storage, no version bump)
    c2.bias.data.add_(0.05 * torch.randn(16, generator=g).to(gpu))
    cd.weight.data.add_(0.1 * torch.randn(64, 16, generator=g).to(gpu))
    assert versions == [p._version for p in (c2.weight, c2.bias, cd.weight)]
    if how == "memoised":
        before = len(replays)
        out = None
        out, path = chained(model, data)
        assert path == "chained" and len(replays) == before + 1        # this result came from the recording
    else:
        _hip.replay(rec.calls)
    _, new_ref, _ = oracle(model, case(2000)[0])
    assert err(new_ref, z_gd) > 100 * TIGHT        # the change is visible
    assert err(out, new_ref) <= TIGHT


def test_new_kernels_register_budgets():
    """No GPU needed: the chained gather and the tail-transform external kernel have no scratch and no spills; the gather
    stays within the 128 registers of sixteen waves per compute unit."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources(_hip.library_path())
    names = ["k_col_gather_next<2>", "k_col_gather_next<1>", "gn::k_aggregate_transform_tail"]
    for name in names:
        assert name in res, (name, sorted(k for k in res if "col_gather" in k or "aggregate_transform" in k))
        r = res[name]
        assert r[".private_segment_fixed_size"] == 0, (name, r)
        assert r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (name, r)
        if "col_gather" in name:
            assert r[".vgpr_count"] + r.get(".agpr_count", 0) <= 128, (name, r)
