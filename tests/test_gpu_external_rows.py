"""The external layer's rows around the 32 and 64 marks of its request rounds (aggregate.hip: aggregate_transform at 16 lanes
per neighbour asks for all sixteen groups of four neighbour rows before it consumes the first; it asked for eight).

A bipartite graph of 40 targets over 300 sources, 64 source columns, 16 outputs; target degrees 0, 1, 4, 31, 32, 33, 47, 48, 63
and 64, four of each: every row fits a padded row of 64, so the plan keeps its padded (ELL) form.  A second graph holds the same
edges in the same order and one more target of degree 65: that plan has no padded rows and walks row pointers.

  * the concat entry point (gn_graph_aggregate_f32 over the 64 columns) and the split entry point (two tables) agree bit for bit;
  * both agree with the float64 closed form per element at the bound tests/test_gpu_scales.py holds the external layer to:
    rho_default <= C max(rho_exact, rho_ref32), C = 1.5;
  * the 40 common rows of the second graph are bit for bit the first graph's: a slot adds its neighbours in the order
    idx = (it0 + it) * 4 + slot whatever the number of groups in flight and whatever the form of the rows;
  * the deferred 16 -> 16 transform (k_aggregate_transform_tail, GN_ENABLE_CHAIN=1) over padded rows of up to 64 genes, against
    the float64 oracle at tests/test_gpu_gene_chain.py's tolerance (its own cases keep a drug of more than 64 genes: row pointers).
"""
import functools

import pytest
import torch

import gripnet_amd
import scale_cases as sc
import test_gpu_gene_chain as gc
from gripnet_amd import _hip

pytestmark = pytest.mark.gpu

C = 1.5                                          # tests/test_gpu_scales.py
N_SRC, FIN, FOUT = 300, 64, 16
DEGREES = [0, 1, 4, 31, 32, 33, 47, 48, 63, 64] * 4
N_TGT = len(DEGREES)
LONG = 65


@functools.lru_cache(maxsize=None)
def edges():
    """([2, E] padded-form graph, its weights, [2, E + 65] the same edges and one target of 65 behind them, its weights)"""
    g = torch.Generator().manual_seed(26)
    src, dst = [], []
    for t, deg in enumerate(DEGREES):
        src.append(torch.randperm(N_SRC, generator=g)[:deg])
        dst.append(torch.full((deg,), t, dtype=torch.long))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()
    w = torch.rand(ei.shape[1], generator=g) + 0.5
    extra = torch.stack([torch.randperm(N_SRC, generator=g)[:LONG], torch.full((LONG,), N_TGT, dtype=torch.long)])
    return ei, w, torch.cat([ei, extra], dim=1).contiguous(), torch.cat([w, torch.rand(LONG, generator=g) + 0.5])


@functools.lru_cache(maxsize=None)
def operands():
    g = torch.Generator().manual_seed(27)
    return {"x": torch.randn(N_SRC, FIN, generator=g), "w": torch.randn(FIN, FOUT, generator=g) * 0.3, "b": torch.randn(FOUT, generator=g)}


def run(gpu, ei, n_tgt, weights, split, head_cols=32):
    plan = _hip.GraphPlan.bipartite(ei.to(gpu), N_SRC, n_tgt, None if weights is None else weights.to(gpu))
    op = {k: v.to(gpu) for k, v in operands().items()}
    out = torch.full((n_tgt, FOUT), float("nan"), device=gpu)
    if split:
        head, tail = op["x"][:, :head_cols].contiguous(), op["x"][:, head_cols:].contiguous()
        assert plan.split_ok(head, tail, FOUT)
        plan.aggregate_split(head, tail, op["b"], False, out, op["w"])
    else:
        plan.aggregate(op["x"], op["b"], False, out, None, weight=op["w"])
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def reference(weighted):
    ei, w, _, _ = edges()
    op = operands()
    ew = w if weighted else None
    ref64, mag64 = sc.bipartite_ref(op["x"], op["w"], op["b"], ei, N_TGT, ew)
    return ref64, mag64, sc.bipartite_ref(op["x"], op["w"], op["b"], ei, N_TGT, ew, torch.float32)


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weighted"])
def test_rows_around_the_request_rounds(gpu, monkeypatch, weighted):
    ei, w, ei_long, w_long = edges()
    deg = torch.bincount(ei[1], minlength=N_TGT)
    assert deg.tolist() == DEGREES and int(torch.bincount(ei_long[1])[N_TGT]) == LONG
    ew, ew_long = (w, w_long) if weighted else (None, None)
    concat = run(gpu, ei, N_TGT, ew, split=False)
    assert torch.isfinite(concat).all()
    # the split entry point, every cut of the 64 columns: the concat launch's bits
    for head_cols in (16, 32, 48):
        assert torch.equal(run(gpu, ei, N_TGT, ew, split=True, head_cols=head_cols), concat), head_cols
    # the float64 closed form, per element
    ref64, mag64, ref32 = reference(weighted)
    rho = {"default": sc.componentwise(concat, ref64, mag64), "ref32": sc.componentwise(ref32, ref64, mag64)}
    with monkeypatch.context() as m:                 # (the layer on the general kernels, as tests/test_gpu_scales.py runs it)
        m.setenv("GN_DISABLE_FAST", "1")
        conv = gripnet_amd.myGCN(FIN, FOUT, cached=True).to(gpu)
        with torch.no_grad():
            conv.weight.copy_(operands()["w"].to(gpu))
            conv.bias.copy_(operands()["b"].to(gpu))
            exact = conv.forward_bipartite(operands()["x"].to(gpu), ei.to(gpu), N_TGT, None if ew is None else ew.to(gpu))
        rho["exact"] = sc.componentwise(exact, ref64, mag64)
    sc.check("external rows " + ("weighted" if weighted else "ones"), rho, C)
    # one target of 65 behind them: no padded rows, row pointers - the common rows keep their bits
    for split in (False, True):
        long = run(gpu, ei_long, N_TGT + 1, ew_long, split=split)
        assert torch.isfinite(long).all()
        same = (long[:N_TGT] == concat).all(dim=1)
        assert same.all(), "rows of degree {} differ between the padded and the row-pointer form".format(
            sorted({DEGREES[i] for i in torch.nonzero(~same).flatten().tolist()}))
    # twice: same bits
    assert torch.equal(run(gpu, ei, N_TGT, ew, split=False), concat)
    _hip.raise_if_index_errors(gpu)


def test_deferred_transform_over_padded_rows(gpu, monkeypatch):
    """The tail variant applies W2 per group of four gathered rows: drugs of 33 to 64 genes, all in padded rows."""
    monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    monkeypatch.setenv("GN_ENABLE_CHAIN", "1")
    n_g = 1037
    data = gc.make_case(n_g)
    gd = data.gd_edge_index
    # gc.make_case gives one drug more than a hundred genes: 64 of them stay there, 40 go to its neighbour, the rest are dealt round
    busy = torch.nonzero(gd[1] == gc.BUSY_DRUG).flatten()
    gd[1, busy[64:104]] = gc.BUSY_DRUG + 1
    gd[1, busy[104:]] = 20 + torch.arange(busy.numel() - 104) % 16
    data.gd_edge_index = gd
    per_drug = torch.bincount(gd[1], minlength=gc.N_D)
    assert per_drug.max() == 64 and per_drug[gc.BUSY_DRUG] == 64 and (per_drug > 32).sum() >= 2 and per_drug[gc.EMPTY_DRUG] == 0
    model = gc.make_model(data)
    _, z_gd, _ = gc.oracle(model, data)
    out, path = gc.chained(model.to(gpu), gc.copy_to(data, gpu))
    assert path == "chained"
    e = gc.err(out, z_gd)
    print("padded rows, deferred transform: max |chained - oracle| = {:.3e}".format(e))
    assert e <= gc.TIGHT
