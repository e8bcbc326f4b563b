"""The external layer reading the gene embedding in place (gn_graph_aggregate_split_f32, layers.gene_stack_to_external on its
separate path): a gathered row kept in two tables gives the bits of the same launch over the materialised concatenation.

Every comparison is bitwise.  GN_BLOCKED_ANY=1 lifts the size thresholds of the LDS-staged plans, so that a small gene graph
takes them; without it the gene layers of these sizes run on the wave-per-row kernels."""
import functools
import os
import sys

import pytest
import torch

from gripnet_amd import _hip
from gripnet_amd.layers import gene_stack_path, gene_stack_to_external
from gripnet_amd.pipeline import PoseModel, PoseStages
from gripnet_amd.synth import Data, make_pose
from gripnet_amd.utils import set_arithmetic, set_table_storage

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu_test = pytest.mark.gpu
SPLIT, PLAIN = "gn_graph_aggregate_split_f32", "gn_graph_aggregate_f32"
SIDE_OF = {PLAIN: 10, "gn_graph_aggregate_bf16": 8}    # where the entry points take their side copy
SIDE_ARG = 10                                         # gn_graph_aggregate_f32(plan, xw, ld, fin, w, fout, bias, relu, out, ld, side, ..)

# ---- the entry point against gn_graph_aggregate_f32 over the materialised concatenation ------------------------------
N_SRC, N_TGT = 300, 70
DEGREES = {"padded": {0: 0, 1: 1, 2: 64}, "long": {0: 0, 1: 1, 2: 64, 3: 100}}   # the other targets: 5 .. 40 neighbours


@functools.lru_cache(maxsize=None)
def bipartite_edges(kind):
    """[2, E] gene -> drug edges and weights: targets of degree 0, 1 and exactly 64 ("padded": no row beyond a padded row of
    64, the plan keeps its padded rows), and with "long" one of 100 (the plan walks row pointers)."""
    g = torch.Generator().manual_seed(11)
    src, dst = [], []
    for t in range(N_TGT):
        deg = DEGREES[kind].get(t, int(torch.randint(5, 41, (1,), generator=g)))
        src.append(torch.randperm(N_SRC, generator=g)[:deg])
        dst.append(torch.full((deg,), t, dtype=torch.long))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    perm = torch.randperm(ei.shape[1], generator=g)
    return ei[:, perm].contiguous(), torch.rand(ei.shape[1], generator=g) + 0.5


@functools.lru_cache(maxsize=None)
def operands():
    g = torch.Generator().manual_seed(12)
    return {"x": torch.randn(N_SRC, 64, generator=g), "w": torch.randn(64, 16, generator=g) * 0.3,
            "b": torch.randn(16, generator=g), "tf": torch.randn(N_TGT, 32, generator=g)}


def in_wider(t, pad):
    """`t` as a 16-byte aligned view into a buffer whose rows are `pad` floats longer."""
    if not pad:
        return t.contiguous()
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=t.device)
    view = wide[:, 4:4 + t.shape[1]]
    view.copy_(t)
    return view


def run_both(gpu, kind, head_cols, weighted=False, relu=True, bias=True, pad=0):
    ei, wgt = bipartite_edges(kind)
    plan = _hip.GraphPlan.bipartite(ei.to(gpu), N_SRC, N_TGT, wgt.to(gpu) if weighted else None)
    op = {k: v.to(gpu) for k, v in operands().items()}
    b = op["b"] if bias else None
    res = []
    for split in (False, True):
        out = torch.full((N_TGT, 48), -7.0, device=gpu)
        planes = _hip.SplitPlanes(N_TGT, 3, gpu)
        y, side = out[:, :16], (op["tf"], out[:, 16:], 1)
        if split:
            head, tail = in_wider(op["x"][:, :head_cols], pad), in_wider(op["x"][:, head_cols:], pad)
            assert plan.split_ok(head, tail, 16)
            plan.aggregate_split(head, tail, b, relu, y, op["w"], side=side, planes=(planes, 0, 16))
        else:
            plan.aggregate(op["x"], b, relu, y, side, weight=op["w"], planes=(planes, 0, 16))
        res.append((out, planes.buf))
    torch.cuda.synchronize()
    return res


def same(res):
    (out0, planes0), (out1, planes1) = res
    assert torch.isfinite(out0).all() and (out0[:, :16] != -7.0).any()
    assert torch.equal(out0[:, :16], out1[:, :16]), "out"
    assert torch.equal(out0[:, 16:], out1[:, 16:]) and torch.equal(out1[:, 16:], operands()["tf"].abs().to(out1.device)), "side slot"
    assert planes0.any() and torch.equal(planes0, planes1), "split planes"


@gpu_test
@pytest.mark.parametrize("kind", ["padded", "long"])
@pytest.mark.parametrize("head_cols", [16, 32, 48])
def test_entry_point_is_the_concat_launch(gpu, kind, head_cols):
    ei, _ = bipartite_edges(kind)
    deg = torch.bincount(ei[1], minlength=N_TGT)
    assert deg[0] == 0 and deg[1] == 1 and deg[2] == 64 and (deg.max() > 64) == (kind == "long")
    same(run_both(gpu, kind, head_cols))


@gpu_test
@pytest.mark.parametrize("kind", ["padded", "long"])
@pytest.mark.parametrize("variant", ["wider_buffers", "weighted", "no_relu", "no_bias"])
def test_entry_point_variants(gpu, kind, variant):
    kw = {"wider_buffers": dict(pad=8), "weighted": dict(weighted=True), "no_relu": dict(relu=False), "no_bias": dict(bias=False)}[variant]
    for head_cols in (16, 32, 48):
        res = run_both(gpu, kind, head_cols, **kw)
        same(res)
        if variant == "no_relu":
            assert (res[1][0][:, :16] < 0).any()


@gpu_test
@pytest.mark.parametrize("name", ["head_0", "head_64", "head_20", "misaligned_head", "ld_not_4", "32_to_16"])
def test_refusals_launch_nothing(gpu, name):
    ei, _ = bipartite_edges("long")
    plan = _hip.GraphPlan.bipartite(ei.to(gpu), N_SRC, N_TGT, None)
    x = operands()["x"].to(gpu)
    w = operands()["w"].to(gpu)
    if name.startswith("head_"):
        hc = int(name[5:])
        head, tail = x[:, :hc], x[:, hc:]
        if hc in (0, 64):                               # (an empty table still has an address and a leading dimension)
            assert (head if hc == 0 else tail).shape[1] == 0
    elif name == "misaligned_head":
        wide = torch.zeros((N_SRC, 36), device=gpu)
        head, tail = wide[:, 1:33], x[:, 32:].contiguous()
        assert head.data_ptr() % 16 == 4
    elif name == "ld_not_4":
        wide = torch.zeros((N_SRC, 34), device=gpu)
        head, tail = wide[:, :32], x[:, 32:].contiguous()
        assert head.data_ptr() % 16 == 0 and _hip.ld(head) % 4 == 2
    else:
        head, tail, w = x[:, :16].contiguous(), x[:, 16:32].contiguous(), w[:32].contiguous()
    out = torch.full((N_TGT, 16), -7.0, device=gpu)
    assert not plan.split_ok(head, tail, 16)
    with pytest.raises(_hip.Unsupported) as info:
        plan.aggregate_split(head, tail, None, True, out, w)
    assert info.value.status == _hip.GN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ---- the gene stack: the separate path without the concat's slot 0 ---------------------------------------------------
N_G, N_D = 2000, 128
HUB, EMPTY_DRUG, BUSY_DRUG = 5, 3, 7


@functools.lru_cache(maxsize=None)
def pose_case():
    """PoSE-shaped data on 2,000 genes and 128 drugs: gene HUB takes 600 edges, the last five genes keep nothing but their
    self loop, drug EMPTY_DRUG has no gene, drug BUSY_DRUG more than 64 (beyond a padded row of the external plan); and one
    parameter set with random biases.  Shared by the tests below, which work on copies."""
    data = make_pose("small", seed=7, n_g=N_G, e_gg_dir=10 * N_G, n_d=N_D, e_gd=2000)
    g = torch.Generator().manual_seed(8)
    a = torch.randint(0, N_G - 5, (2, 10 * N_G), generator=g)
    a[1, :600] = HUB
    a = a[:, a[0] != a[1]]
    data.gg_edge_index = torch.cat([a, a.flip(0)], dim=1).long()
    data.edge_weight = torch.ones(data.gg_edge_index.shape[1])
    data.n_gg_edge = int(data.gg_edge_index.shape[1])
    gd = data.gd_edge_index.clone()
    gd[1, :100] = BUSY_DRUG
    gd[1][gd[1] == EMPTY_DRUG] = EMPTY_DRUG + 1
    data.gd_edge_index = gd
    deg = torch.bincount(data.gg_edge_index[1], minlength=N_G)
    assert deg[HUB] >= 500 and (deg[-5:] == 0).all()
    per_drug = torch.bincount(gd[1], minlength=N_D)
    assert per_drug[EMPTY_DRUG] == 0 and per_drug[BUSY_DRUG] > 64
    return data, new_model(data).state_dict()


def new_model(data, seed=3, **kw):
    torch.manual_seed(seed)
    model = PoseModel(data.n_g_node, data.n_d_node, data.n_dd_edge_type, **kw)
    for c in list(model.gg.conv_list) + [model.gd.conv]:
        c.bias.data.normal_(std=0.3)
    return model


def on_gpu(gpu, state=None, **kw):
    data, shared = pose_case()
    model = new_model(data, **kw)
    if state is not None or not kw:
        model.load_state_dict({k: v.clone() for k, v in (state or shared).items()})
    return Data(**{k: getattr(data, k) for k in data.keys()}).to(gpu), model.to(gpu)


def stack(model, data):
    return gene_stack_to_external(model.gg, model.gd, data.gg_edge_index, data.edge_weight, data.gd_edge_index)


def separate(model, data):
    z = model.gg(None, data.gg_edge_index, edge_weight=data.edge_weight, if_catout=True)
    return model.gd(z, data.gd_edge_index, mod="cat", if_relu=True)


def recorded(fn):
    """(result, [(entry point, arguments)]) of fn() under a recorder (which also keeps the modules off their memos)."""
    with _hip.Recorder() as rec:
        out = fn()
    return out, [(name, args) for _, args, name, _ in rec.calls]


@pytest.fixture(params=["staged", "wave_per_row"])
def gene_kernels(request, monkeypatch):
    if request.param == "staged":
        monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    else:
        monkeypatch.delenv("GN_BLOCKED_ANY", raising=False)
    monkeypatch.delenv("GN_ENABLE_CHAIN", raising=False)
    return request.param


@gpu_test
def test_gene_stack_reads_the_embedding_in_place(gpu, gene_kernels):
    data, model = on_gpu(gpu)
    with torch.no_grad():
        want, ref_calls = recorded(lambda: separate(model, data))
        want_planes = _hip.SplitPlanes.of(want, 3).buf.clone()    # (the next launch rewrites the layer's planes)
        got, calls = recorded(lambda: stack(model, data))
    assert (model.gg.conv_list[0].cached_result.blocked_cols > 0) == (gene_kernels == "staged")
    assert gene_stack_path(model.gg) == "separate"
    assert torch.equal(got, want)
    assert [n for n, _ in ref_calls] == [PLAIN] * 3 and ref_calls[0][1][SIDE_ARG] is not None     # today: the copy rides on layer 1
    assert [n for n, _ in calls] == [PLAIN, PLAIN, SPLIT]
    assert calls[0][1][SIDE_ARG] is None and calls[1][1][SIDE_ARG] is None
    planes = _hip.SplitPlanes.of(got, 3)                      # the output is tagged with the planes the launch left
    assert planes is not None and want_planes.any() and torch.equal(planes.buf, want_planes)
    with torch.no_grad():
        for _ in range(4):                                    # (from the third call: the memoised launches)
            again = None
            again = stack(model, data)
            assert torch.equal(again, want) and gene_stack_path(model.gg) == "separate"


@gpu_test
def test_recorded_step_is_the_eager_step(gpu, gene_kernels):
    data, model = on_gpu(gpu)
    with torch.no_grad():
        x = separate(model, data)
        z0 = model.dd(x, data.train_idx, edge_type=data.train_et, range_list=data.train_range, if_catout=True)
        s0 = model.dmt(z0, data.train_idx, data.train_et)
        z0, s0 = z0.clone(), s0.clone()
        stages = PoseStages(model, data, graphs=False, recorded=True)
        names = [name for _, _, name, _ in stages._whole.calls]
        assert len(names) == 5 and names[:3] == [PLAIN, PLAIN, SPLIT], names
        for _ in range(2):
            z, s = stages.step()
            assert torch.equal(z, z0) and torch.equal(s, s0)
        z, s = model(data)
        assert torch.equal(z, z0) and torch.equal(s, s0)


@gpu_test
@pytest.mark.parametrize("how", ["memoised", "recorded"])
def test_embedding_by_pointer_not_by_value(gpu, gene_kernels, monkeypatch, how):
    data, model = on_gpu(gpu)
    replays = []
    replay = _hip.replay
    monkeypatch.setattr(_hip, "replay", lambda calls: (replays.append(len(calls)), replay(calls))[1])
    with torch.no_grad():
        if how == "memoised":
            out = None
            for _ in range(6):                     # (the output freed before the next call: the allocator hands out its address again)
                out = None
                out = stack(model, data)
            assert replays and set(replays) == {3}
        else:
            stack(model, data)
            with _hip.Recorder() as rec:
                out = stack(model, data)
            assert [name for _, _, name, _ in rec.calls] == [PLAIN, PLAIN, SPLIT]
        before = out.clone()
        emb = model.gg.embedding
        address, g = emb.data_ptr(), torch.Generator().manual_seed(21)
        emb.data.add_(0.5 * torch.randn(emb.shape, generator=g).to(gpu))          # an optimizer step: same storage, new values
        assert emb.data_ptr() == address
        if how == "memoised":
            n = len(replays)
            out = None
            out = stack(model, data)
            assert len(replays) == n + 1                                          # this result came from the recording
        else:
            _hip.replay(rec.calls)
        _, fresh = on_gpu(gpu, state={k: v.detach().cpu() for k, v in model.state_dict().items()})
        want = separate(fresh, data)
    assert not torch.equal(want, before)           # the change is visible
    assert torch.equal(out, want)


def _fallbacks():
    def grad(gpu):
        return on_gpu(gpu)

    def bf16(gpu):
        data, model = on_gpu(gpu)
        set_table_storage(model, "bf16")
        return data, model

    def fast(gpu):
        data, model = on_gpu(gpu)
        set_arithmetic(model, "fast")
        return data, model

    def strided(gpu):
        data, model = on_gpu(gpu)
        wide = torch.zeros((N_G, 40), device=gpu)
        wide[:, :32] = model.gg.embedding.data
        model.gg.embedding.data = wide[:, :32]                # rows contiguous and 16-byte aligned, 40 floats apart
        assert not model.gg.embedding.is_contiguous() and model.gg.embedding.data_ptr() % 16 == 0
        return data, model

    def widths(gpu):
        return on_gpu(gpu, gg_nhids=[32, 16, 8])
    return {"grad_enabled": grad, "bf16_storage": bf16, "fast_arithmetic": fast, "strided_embedding": strided, "widths_32_16_8": widths}


@gpu_test
@pytest.mark.parametrize("name", sorted(_fallbacks()))
def test_fallbacks_keep_todays_route_and_bits(gpu, gene_kernels, name):
    data, model = _fallbacks()[name](gpu)
    with torch.set_grad_enabled(name == "grad_enabled"):
        want, ref_calls = recorded(lambda: separate(model, data))
        got, calls = recorded(lambda: stack(model, data))
        assert gene_stack_path(model.gg) == "separate"
        assert [n for n, _ in calls] == [n for n, _ in ref_calls] and SPLIT not in [n for n, _ in calls]
        copies = [[a[SIDE_OF[n]] is not None for n, a in c if n in SIDE_OF] for c in (calls, ref_calls)]
        assert copies[0] == copies[1] and copies[0][0]         # the concat's slot 0 is still copied by the first gene layer
        assert torch.equal(got.detach(), want.detach())
        assert got.requires_grad == want.requires_grad and got.requires_grad == (name == "grad_enabled")
        for _ in range(3):                                     # and through the modules' own memos
            again = stack(model, data)
            assert torch.equal(again.detach(), want.detach()) and gene_stack_path(model.gg) == "separate"


def test_split_kernel_resources():
    """No GPU needed: the split-source instantiation has no scratch and no spills, and the kernel of the concat form is
    still there beside it."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources(_hip.library_path())
    for name in ("gn::k_aggregate_transform_split<16>", "gn::k_aggregate_transform<16, 16>", "gn::k_aggregate_transform_tail"):
        assert name in res, (name, sorted(k for k in res if "aggregate_transform" in k))
        r = res[name]
        assert r[".private_segment_fixed_size"] == 0, (name, r)
        assert r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (name, r)
