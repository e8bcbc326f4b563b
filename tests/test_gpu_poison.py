"""A non-finite table row reaches only the outputs that read it - on the kernels (the contract, the cases and `check`:
tests/poison_cases.py; the same cases against the reference alone: tests/test_poison_host.py).

Most kernels read "a slot past the end" from a real table row - the padded (ELL) rows of the external layer ask for table row
0 and clear what arrives with a bit mask, the dense products clamp the last row of a ragged tile, the relational pair kernel
reloads 32 source cells per chunk - and then mask it, multiply it by a zero coefficient or send it to a zero row.  On finite
data a multiply by 0.0 gives the mask's numbers; on a NaN it does not.  Every launch here runs twice more than once: on a table
with one or two rows written over with NaN, +Inf or -Inf, and on the same table with those rows at 0.0 - same kernel, same
route.  The float64 reference on the poisoned input says which outputs depend on the rows (dep); the others must come out bit
for bit as from the zeroed table, dep must be exactly the non-finite set, and a NaN poison must arrive as NaN - also through
every ReLU epilogue (torch.relu keeps NaN; fmaxf(NaN, 0) is 0, which hid a diverged model behind finite activations).

What it found when it was written: the LDS-accumulator relational kernel (k_rgcn_lds) restarted a slot's run sum as
`sum * 0 + H[src]`, which handed the NaN of a finished run to the slot's next destination (cases 257-lds, 769-lds, 769-auto);
and with `fmaxf` in the ReLU epilogues every relu=True case of the gathers, the relational kernels, the dense products and
merge mode 3 fails - transform_tail_cols is there for the inner ReLU of the deferred tail transform, which the other cases
cannot see behind the row's first 48 columns.

Every test prints the route it ran and the sizes of dep and clean (pytest -s).  Where the library says which kernel ran the
test asserts it: `path` of a relational plan, `blocked_ok` / `transform_ok` / `split_ok` of a graph plan, the entry points the
binding's Recorder wrote down.  The bare gathers and the dense products have no such query: their shapes are taken from the
route tables (tests/test_gather_route.py, tests/test_dense_route.py) and `plain_gather_route` restates the ladder's rule for the
plan's own counts, so that a shape that drifts off its route is noticed here.
"""
import pytest
import torch

import gripnet_amd
import poison_cases as pc
from gripnet_amd import _hip
from gripnet_amd.gat import GATConv
from gripnet_amd.pyg_convs import RGCNConv

pytestmark = pytest.mark.gpu

SWITCHES = ("GN_DISABLE_FAST", "GN_DISABLE_QUAD", "GN_DISABLE_BLOCKED", "GN_DISABLE_LDS_TABLE", "GN_BLOCKED_ANY")


@pytest.fixture(autouse=True)
def switches_off(monkeypatch):
    for hook in SWITCHES:
        monkeypatch.setenv(hook, "0")


def served(fn):
    """(result, names of the entry points that took the calls `fn` made, in order) - tests/test_gpu_boundaries.py"""
    with _hip.Recorder() as rec:
        result = fn()
    return result, [name for _, _, name, _ in rec.calls]


def drive(dev, case, launch):
    """Every variant of `case`: `launch(tensors, **flags)` -> (out, route) on the poisoned and on the zeroed tensors, held to the
    contract against the float64 reference of the poisoned ones.  Returns the routes that ran."""
    zeroed, routes = {}, set()

    def finished(tensors, flags):
        try:
            result = launch(tensors, **flags)
            torch.cuda.synchronize()
            return result
        except RuntimeError as e:                        # a device error ends the session: nothing more is launched on that device
            if any(word in str(e) for word in ("HIP error", "hipError", "illegal memory access")):
                pytest.exit("{}: {}".format(case.name, e), returncode=3)
            raise
    for poison, flags in case.variants:
        key = tuple(sorted(flags))
        if key not in zeroed:
            zeroed[key] = finished(pc.poisoned(case, 0.0), flags)
        out_0, route_0 = zeroed[key]
        tensors = pc.poisoned(case, poison)
        out_p, route = finished(tensors, flags)
        assert route == route_0, "{}: the poisoned launch ran {} and the zeroed one {}".format(case.name, route, route_0)
        what = "{} [{}{}] route {}".format(case.name, poison, "".join(" " + k for k in flags), route)
        pc.check(out_p, out_0, case.ref(tensors, torch.float64, **flags), what, nan=poison in pc.NAN_POISONS)
        routes.add(route)
    _hip.raise_if_index_errors(dev)
    return routes


def on(dev, t, *keys):
    return [None if t.get(k) is None else t[k].to(dev) for k in keys]


# ---- GCN-style gathers -------------------------------------------------------------------------------------------------------
def plain_gather_route(plan, features, ld_ok, bf16, bias, relu, env):
    """gather_route.hpp's rule for a gather without a weight over 16-byte-aligned operands, on the plan's own counts."""
    rows, nnz = plan.n_rows, plan.nnz
    fast_off = env.get("GN_DISABLE_FAST") == "1"
    lanes = lambda units: next(p for p in (1, 2, 4, 8, 16, 32, 64) if p >= min(units, 64))
    if bf16:
        return "bf16_group" if lanes(features // 8) <= 32 and nnz < 48 * rows and rows >= 4096 and not fast_off else "bf16_wave"
    vec = features % 4 == 0 and ld_ok
    lpe = lanes(features // 4 if vec else features)
    fast = vec and not fast_off
    if (fast and 4 <= lpe <= 16 and 0 < nnz < 8 * rows and rows >= 65536 and plan.kind == "sum" and not bias and not relu and
            plan.n_table * features * 4 <= 128 * 1024 and env.get("GN_DISABLE_LDS_TABLE") != "1"):
        return "lds_table"
    if fast and lpe <= 16 and nnz < 8 * rows:
        return "short_rows"
    if fast and lpe <= 32 and nnz < 48 * rows:
        return "group"
    return "wave" if vec else "wave_scalar"


def gather_plan(dev, case, t):
    ei, ew = on(dev, t, "ei", "ew")
    if case.kind == "gcn":
        return _hip.GraphPlan.gcn(ei, case.n_src, ew)
    if case.kind == "sum":
        return _hip.GraphPlan.plain_sum(ei, case.n_src, case.n_dst)
    return _hip.GraphPlan.bipartite(ei, case.n_src, case.n_dst, ew)


@pytest.mark.parametrize("which", pc.ROW_SETS)
@pytest.mark.parametrize("route", list(pc.GATHER_SPECS))
def test_gather_keeps_a_poisoned_row_to_its_readers(gpu, monkeypatch, route, which):
    case = pc.gather_case(route, which)
    spec, entry = case.spec, case.spec.get("entry")
    env = spec.get("env", {})
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = gather_plan(gpu, case, case.tensors)
    fin, fout = spec["fin"], spec["fout"]
    if case.route == "blocked" or "GN_DISABLE_BLOCKED" in env:
        assert plan.build_blocked(fout) == (0 if "GN_DISABLE_BLOCKED" in env else fout), case.name

    def launch(t, relu=False):
        x, w, b, w2, b2 = on(gpu, t, "x", "w", "b", "w2", "b2")
        rows_out = case.n_src if entry == "t" else case.n_dst
        out = torch.full((rows_out, fout or fin), float("nan"), device=gpu)
        if entry == "t":
            plan.aggregate_t(x, out)
            return out, "transposed"
        if entry in ("bf16", "bf16_product"):
            named = plain_gather_route(plan, fout or fin, True, True, b is not None, relu, env)
            if entry == "bf16_product":
                table = torch.empty((x.shape[0], fout), dtype=torch.bfloat16, device=gpu)
                _, names = served(lambda: _hip.gemm(x, w, table, out_bf16=True))          # (Unsupported would raise: no fp32 detour here)
                assert names == ["gn_gemm_f32"], names
                plan.aggregate_bf16(table, b, relu, out)
                return out, "split + " + named
            plan.aggregate_bf16(x, b, relu, out)
            return out, named
        if entry == "tail":
            plan.aggregate(x, b, relu, out, weight=w, tail=(w2, b2))
            return out, "transform_tail"
        if entry == "split":
            head, tail = x[:, :32].contiguous(), x[:, 32:].contiguous()
            assert plan.split_ok(head, tail, fout), case.name
            plan.aggregate_split(head, tail, b, relu, out, w)
            return out, "transform_split"
        if w is None:
            plan.aggregate(x, b, relu, out)
            return out, plain_gather_route(plan, fin, True, False, b is not None, relu, env)
        blocked = plan.blocked_ok(x, w, b, out)
        assert blocked or plan.transform_ok(fin, fout, x), case.name + ": the library has no fused form for this call"
        plan.aggregate(x, b, relu, out, weight=w)
        if blocked:
            return out, "blocked"
        if fout >= 64:
            return out, "mfma"
        return out, "transform_quad" if (fin, fout) == (16, 16) and env.get("GN_DISABLE_QUAD") != "1" else "transform"
    routes = drive(gpu, case, launch)
    assert routes == {case.route}, (case.name, routes)


# ---- the relational layer ---------------------------------------------------------------------------------------------------
def relational_layer(dev, case, kernel):
    t = case.tensors
    rg = gripnet_amd.myRGCN(case.fin, case.fout, case.R, case.bases, False, bias=True).to(dev)
    with torch.no_grad():
        for name in ("basis", "att", "root", "bias"):
            getattr(rg, name).copy_(t[name].to(dev))
    rg.kernel = kernel
    return rg


RELATIONAL_RUNS = [(256, "auto"), (257, "auto"), (768, "auto"), (769, "auto"), (256, "pair"), (768, "pair"), (257, "lds"), (769, "lds"),
                   (257, "general"), (768, "general"), (256, "table"), (769, "table")]


@pytest.mark.parametrize("which", pc.ROW_SETS)
@pytest.mark.parametrize("n,kernel", RELATIONAL_RUNS)
def test_relational_layer_keeps_a_poisoned_row_to_its_readers(gpu, n, kernel, which):
    """myRGCN at 256 / 257 and 768 / 769 nodes (the destination-major kernel's last size and the next; "auto" takes it up to 768
    and the LDS-accumulator kernel from 769), every kernel also asked for by name: the plan's path query must name it."""
    case = pc.relational_case(n, which)
    rg = relational_layer(gpu, case, kernel)
    ei = case.tensors["ei"].to(gpu)
    rl = case.tensors["rl"]

    def launch(t, relu=False):
        with torch.no_grad():
            y = rg(t["x"].to(gpu), ei, None, rl, _relu=relu)
        return y, rg._plan.path(case.fin, case.fout, case.bases, rg._fast(), kernel)
    routes = drive(gpu, case, launch)
    want = ("pair" if n <= 768 else "lds") if kernel == "auto" else kernel
    assert routes == {want}, (case.name, kernel, routes)


@pytest.mark.parametrize("which", pc.ROW_SETS)
@pytest.mark.parametrize("weighted", [True, False], ids=["edge_norm", "sum"])
def test_rgcn_conv_keeps_a_poisoned_row_to_its_readers(gpu, weighted, which):
    case = pc.relational_conv_case(which, weighted)
    t = case.tensors
    conv = RGCNConv(case.fin, case.fout, case.R, case.bases).to(gpu)
    with torch.no_grad():
        for name in ("basis", "att", "root", "bias"):
            getattr(conv, name).copy_(t[name].to(gpu))
    ei, et, norm = on(gpu, t, "ei", "et", "norm")

    def launch(tt, relu=False):
        def run():
            with torch.no_grad():
                return conv(tt["x"].to(gpu), ei, et, norm, _relu=relu)
        y, names = served(run)
        return y, "+".join(names)
    routes = drive(gpu, case, launch)
    assert len(routes) == 1 and all(("weighted" in r) == weighted for r in routes), (case.name, routes)


# ---- the DistMult decoder ---------------------------------------------------------------------------------------------------
def pack_words(ei):
    """u | v << 16 of every pair as the int32 words a NegativeSampler leaves next to its draw (tests/test_gpu_boundaries.py)"""
    w = ei[0] | (ei[1] << 16)
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


DECODER_RUNS = [(shape, "planned") for shape in pc.DECODER_SHAPES] + [("lds fit", "packed"), ("lds miss", "packed"), ("lds miss", "general"),
                                                                      ("odd width", "general")]
# the entry point that must serve a run (None: the library decides; the test reports it)
DECODER_SERVED = {("lds fit", "planned"): "gn_distmult_plan_forward_f32", ("lds miss", "planned"): "gn_distmult_forward_f32",
                  ("row classes", "planned"): "gn_distmult_plan_forward_f32", ("three blocks", "planned"): "gn_distmult_plan_forward_f32",
                  ("column phases", "planned"): "gn_distmult_plan_forward_f32", ("odd width", "planned"): None,
                  ("lds fit", "packed"): "gn_distmult_packed_forward_f32", ("lds miss", "packed"): "gn_distmult_forward_f32",
                  ("lds miss", "general"): "gn_distmult_forward_f32", ("odd width", "general"): "gn_distmult_forward_f32"}


@pytest.mark.parametrize("which", pc.ROW_SETS)
@pytest.mark.parametrize("target", ["z", "d"])
@pytest.mark.parametrize("shape,form", DECODER_RUNS)
def test_decoder_keeps_a_poisoned_row_to_its_pairs(gpu, shape, form, target, which):
    """The plan-less decoder on int64 triples, on a sampler's packed words (node table in LDS up to 2400 nodes) and the planned
    kernels (LDS table, row classes in one and in three blocks, column phases), a node's row and a relation's row poisoned."""
    case = pc.decoder_case(shape, target, which)
    ei, et = on(gpu, case.tensors, "ei", "et")
    words = pack_words(case.tensors["ei"]).to(gpu)
    plan = _hip.DistMultPlan(ei, et, case.n, case.R, case.f) if form == "planned" else None

    def launch(t, sigmoid=False):
        z, d = on(gpu, t, "z", "d")
        out = torch.full((ei.shape[1],), float("nan"), device=gpu)

        def run():
            if form == "packed":
                try:
                    return _hip.distmult_packed(z, words, et, d, sigmoid, out)
                except _hip.Unsupported:
                    pass
            if form == "planned":
                return _hip.distmult_forward(z, ei, et, d, sigmoid, out, plan)[0]
            return _hip.distmult(z, ei, et, d, sigmoid, out)
        _, names = served(run)
        return out, names[-1]
    routes = drive(gpu, case, launch)
    want = DECODER_SERVED[(shape, form)]
    assert len(routes) == 1 and (want is None or routes == {want}), (case.name, form, routes)


# ---- dense products ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.gemm_cases(), ids=lambda c: c.name.replace(" ", "-"))
def test_gemm_keeps_a_poisoned_row_to_its_outputs(gpu, case):
    """_hip.gemm on every kernel of dense_route.hpp (the shape names it: tests/test_dense_route.py holds the table): a row of A
    moves its output row(s) alone, B's last column at a ragged n its output column alone."""
    m, k, n, opt, batch = case.m, case.k, case.n, case.opt, case.batch
    at, bt = opt.get("at", False), opt.get("bt", False)

    def launch(t, relu=False):
        a, b, bias, idx = on(gpu, t, "a", "b", "bias", "idx")
        a = a.transpose(-1, -2).contiguous() if at else a
        b = b.transpose(-1, -2).contiguous() if bt else b
        out = torch.full(((batch,) if batch > 1 else ()) + (m, n), float("nan"), device=gpu)
        kw = dict(bias=bias, relu=relu, a_transposed=at, b_transposed=bt, a_rows=idx)
        if batch > 1:
            _hip.gemm(a.view(-1, k), b.view(-1, n), out.view(-1, n), batch=batch, stride_a=m * k, stride_b=k * n, stride_c=m * n,
                      m=m, n=n, k=k, **kw)
        else:
            _hip.gemm(a, b, out, **kw)
        return out, case.shape
    drive(gpu, case, launch)


# ---- merges and class scores ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.rowwise_cases(), ids=lambda c: c.name.replace(" ", "-"))
def test_rowwise_kernels_keep_a_poisoned_row_to_itself(gpu, case):
    def launch(t):
        if case.family == "merge":
            dst, src, src2 = on(gpu, t, "dst", "src", "src2")
            return _hip.merge(dst.clone(), src, case.mode, src2 if case.mode == 4 else None), "gn_merge_f32 mode {}".format(case.mode)
        z, w, nodes = on(gpu, t, "z", "w", "nodes")
        out = torch.full((nodes.numel(), w.shape[1]), float("nan"), device=gpu)
        return _hip.class_scores(z, w, nodes, out, case.softmax), "gn_class_scores_f32"
    drive(gpu, case, launch)


# ---- graph attention --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.gat_cases(), ids=lambda c: c.name.replace(" ", "-"))
def test_gat_keeps_a_poisoned_row_to_its_readers(gpu, case):
    t = case.tensors
    conv = GATConv(t["x"].shape[1], case.channels, heads=case.heads, negative_slope=case.slope).to(gpu)
    with torch.no_grad():
        conv.weight.copy_(t["w"].to(gpu))
        conv.att.copy_(t["att"].to(gpu))
        conv.bias.copy_(t["b"].to(gpu))
    ei = t["ei"].to(gpu)

    def launch(tt, relu=False):
        def run():
            with torch.no_grad():
                return conv(tt["x"].to(gpu), ei, _relu=relu)
        y, names = served(run)
        return y, "+".join(names)
    routes = drive(gpu, case, launch)
    assert len(routes) == 1 and "gn_gat_forward_f32" in next(iter(routes)), routes


# ---- KGE scorers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.kge_cases(), ids=lambda c: c.name.replace(" ", "-"))
def test_kge_scorers_keep_a_poisoned_entity_to_its_scores(gpu, case):
    import kge_cases as kc
    divisor = kc.embedding_range(case.gamma, case.H) / kc.PI
    t = case.tensors
    ids = {k: t[k].to(gpu) for k in t if k not in ("ent", "rel")}

    def launch(tt):
        ent, rel = on(gpu, tt, "ent", "rel")
        if case.batch:
            out = torch.full(tuple(ids["negatives"].shape), float("nan"), device=gpu)
            _hip.kge_batch_forward(case.model, ent, rel, ids["positive"][0].contiguous(), ids["et"], ids["negatives"], "tail", case.gamma,
                                   divisor, False, out)
            return out, "gn_kge_batch_forward_f32"
        out = torch.full((ids["sample"].shape[1],), float("nan"), device=gpu)
        _hip.kge_forward(case.model, ent, rel, ids["sample"], ids["et"], case.gamma, divisor, False, out)
        return out, "gn_kge_forward_f32"
    drive(gpu, case, launch)
