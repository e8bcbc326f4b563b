"""Every default-arithmetic path at any scale: exact homogeneity under power-of-two factors, and fp32's own error per element.

The rest of the suite draws inputs at unit scale and takes max-norm errors: a default path that lost a cross term of its
bf16 split (the two-term "fast" mode stays under every such tolerance) would pass it.  Here

* every kernel that is linear in an input must return ``f(s x) == s f(x)`` BIT FOR BIT for s in scale_cases.pow2_scales
  (a power-of-two factor commutes with every IEEE rounding while nothing under- or overflows; the fp32 oracle has the
  property, tests/test_scales_host.py) - reference-free; it catches absolute thresholds, flushed remainders of a split and
  range limits of the bf16 terms;
* rho = max |y - ref64| / mag64 (scale_cases.componentwise) of the default path is held to ``C`` times the larger of the
  exact paths' (GN_DISABLE_FAST=1: the fp32 matrix instruction; for the relational layer also kernel="general" / "lds") and
  the fp32 CPU reference's, with no absolute floor, at unit scale and with rows in 2^[-30, 30] and weight columns in
  2^[-10, 10]; where a path has a two-term mode, that mode must EXCEED twice the bound - the proof that the bound would
  catch a dropped term on that path and shape.

Factors on z of the decoder act squared (s^2): single products z_u z_v d of small entries are denormal at 2^-120, in the
fp32 oracle as well (test_scales_host), so those rows run over Z_SCALES = the factors from 2^-20 up.

Measured on an MI355X (rho in multiples of u = 2^-24, smallest - largest over unit / mixed scale, weighted / unweighted and,
for the backward rows, over every returned gradient; "worst" = largest rho_default / max(rho_exact, rho_ref32) of a single
case, "fast x" = smallest rho_fast / max(rho_exact, rho_ref32)):

    path                          default     exact        ref32       fast     worst  fast x
    gemm split, 2048 x 32 x 8     1.17-1.23   2.77-3.00    2.82-2.86   87-106   0.43   30
    gemm split, K in slabs        3.89-4.66   4.46-4.56    3.74-4.13   32       1.04   7.0
    gemm split, ragged, CT = 8    3.60-3.73   4.56-4.72    4.49-6.13   56-59    0.82   9.1
    gemm split, b transposed      3.73-3.76   4.01-4.13    5.17-5.37   72-75    0.73   13
    gemm fp32 LDS / accumulate    3.16-3.53   (same bits)  3.64-4.42   -        0.97
    gemm deep / deep transposed   0.79-1.26   0.95-2.11    1.50-1.76   -        0.75
    gemm general / gather / batch 1.68-3.62   (same bits)  1.68-3.62   -        1.00
    x^T g one-launch/tiles/wide   0.25-0.58   0.28-0.51    0.51-1.34   -        0.55
    gcn wave-per-row              1.48-3.76   1.48-4.36    1.44-4.36   -        1.00
    gcn fused 32->16, 64->32      1.00-2.77   1.22-4.14    1.23-4.66   -        0.73
    gcn wide fused 64->64         1.88-3.63   1.86-6.12    1.86-6.12   -        1.01
    gcn LDS-staged 16 / 32        0.80-4.30   1.10-4.29    0.91-4.64   -        0.93
    gcn tall product + gather     1.01-3.55   1.83-4.54    1.56-4.76   45-106   0.78   18
    gcn bf16 table (own table)    4.22-6.42   -            3.95-7.65   -        1.07
    bipartite conv                0.90-1.75   1.26-3.61    1.46-3.37   -        0.61
    rgcn destination-major        1.27-1.66   2.01-5.04    1.87-3.18   18-152   0.52   5.8
    rgcn LDS accumulator          1.28-2.09   2.01-3.45    1.87-3.07   -        0.61
    rgcn general (basis space)    1.75-2.87   3.06-3.40    3.07        68-71    0.84   20
    distmult 80 (all three forms) 1.24-2.34   1.39-3.12    1.56-3.52   -        0.93
    distmult 45                   1.96-3.85   (same bits)  2.05-4.57   -        0.96
    class scores 8 / 17           0.89-4.30   2.90-4.30    2.57-3.80   -        1.00
    gcn backward (dx, dW, db)     0.09-8.94   0.10-8.23    0.11-9.10   -        1.11
    rgcn backward (5 gradients)   0.15-8.31   0.18-11.6    0.20-7.87   -        1.19
    distmult backward (dz, dD)    1.01-4.73   1.88-4.73    3.12-5.66   -        1.00

C stays at 1.5: no correct default path measured above 1.19 of its bound, and no two-term mode below 5.8 of it (the
counter-assertion asks for 2 C = 3).  Every homogeneity check held at every factor.  With the default silently switched
to two terms (every gn_gemm_f32 call and every relational layer), exactly the error tests of the split-kernel paths
fail: gemm split-*, gcn tall-product, rgcn pair-* / general-8.
"""
import contextlib

import pytest
import torch

import gripnet_amd
import scale_cases as sc
from gripnet_amd import _hip
from gripnet_amd.decoder import multiClassInnerProductDecoder, multiRelaInnerProductDecoder
from oracle import gripnet_oracle as orc

pytestmark = pytest.mark.gpu

C = 1.5                                          # one margin for the whole module (the two "as exact as fp32" tests' own)
Z_SCALES = tuple(s for s in sc.pow2_scales if s >= 2.0 ** -20)
MODES = ("unit", "mixed")
BASE_ROWS, BASE_COLS = (-12, 12), (-6, 6)        # exponents of the mixed-scale BASE input of a homogeneity check
RHO_ROWS, RHO_COLS = (-30, 30), (-10, 10)        # exponents of the mixed-scale input of an error check


@pytest.fixture(autouse=True)
def every_fast_path_on(monkeypatch):
    for hook in ("GN_DISABLE_FAST", "GN_DISABLE_QUAD", "GN_DISABLE_BLOCKED", "GN_DISABLE_LDS_TABLE"):
        monkeypatch.setenv(hook, "0")
    monkeypatch.delenv("GN_BLOCKED_ANY", raising=False)


@contextlib.contextmanager
def exact_paths(monkeypatch):
    """GN_DISABLE_FAST=1: the general kernels on the fp32 matrix instruction."""
    with monkeypatch.context() as m:
        m.setenv("GN_DISABLE_FAST", "1")
        yield


def served(fn):
    with _hip.Recorder() as rec:
        result = fn()
    return result, [name for _, _, name, _ in rec.calls]


def scale_rows(t, mode, gen, rows=RHO_ROWS):
    return t if mode == "unit" else sc.mixed_scale(t, rows[0], rows[1], 0, gen)


def scale_cols(t, mode, gen, cols=RHO_COLS):
    if mode == "unit":
        return t
    return sc.mixed_scale(t.view(1, -1), cols[0], cols[1], 1, gen).view(-1) if t.dim() == 1 else sc.mixed_scale(t, cols[0], cols[1], 1, gen)


def homogeneous(run, operands, groups, scales=sc.pow2_scales, power=1, what=""):
    """``run(**operands)`` (a tensor or a tuple of tensors) twice on the base input (same bits), then with the operands of
    every group multiplied by s: every output must be the base output times s^power, bit for bit."""
    def outputs(ops):
        out = run(**ops)
        return [t.detach().clone() for t in (out if isinstance(out, (tuple, list)) else (out,))]
    base = outputs(operands)
    for a, b in zip(base, outputs(operands)):
        assert torch.equal(a, b), "{}: not the same bits on a second run".format(what)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in base), what
    for keys in groups:
        assert all(k in operands for k in keys), keys
        for s in scales:
            scaled = {k: (v * s if k in keys and v is not None else v) for k, v in operands.items()}
            for i, (got, want) in enumerate(zip(outputs(scaled), base)):
                want = want * (s ** power)
                bad = int((got != want).sum())
                assert bad == 0, "{}: output {} with {} x {:g}: {} of {} elements differ from the scaled base".format(
                    what, i, "+".join(keys), s, bad, want.numel())


# =============================================================================================================================
# gn_gemm_f32
# =============================================================================================================================
GEMM_CASES = {
    # name:            (m,    k,   n,   options)                        the kernel the shape reaches (gemm.hip's dispatch)
    "split-threshold": (2048, 32, 8, dict(bias=True)),                  # tall-skinny split kernel at its first row count
    "split-slabs": (2048, 288, 72, dict(bias=True)),                    # ... K = 9 chunks through a 6-chunk LDS slab, CT = 8
    "split-ragged": (2049, 128, 128, dict()),                           # ... a last row tile of one row, CT = 8
    "split-b-transposed": (2048, 64, 32, dict(bt=True)),                # ... dx = g W^T of the wide layers' backward
    "lds-fp32": (300, 64, 48, dict(bias=True)),                         # B in LDS, fp32 matrix instruction
    "deep": (16, 256, 70, dict()),                                      # deep and narrow: K over the waves
    "deep-transposed": (17, 300, 21, dict(at=True, bt=True)),
    "general": (40, 5, 100, dict(bias=True)),
    "row-gather": (500, 40, 24, dict(a_rows=True)),
    "accumulate-addend": (300, 64, 48, dict(accumulate=True, addend=True, bias=True)),
    "batch-3": (40, 5, 100, dict(batch=3)),
}
SPLIT_GEMMS = {k for k in GEMM_CASES if k.startswith("split")}


def gemm_operands(name, mode, seed=0, rows=RHO_ROWS, cols=RHO_COLS):
    m, k, n, opt = GEMM_CASES[name]
    gen = torch.Generator().manual_seed(m * 7 + k * 3 + n + seed)
    batch = opt.get("batch", 1)
    table = 300 if opt.get("a_rows") else m
    lead = (batch,) if batch > 1 else ()
    ops = {"a": scale_rows(torch.randn(*lead, table, k, generator=gen).view(-1, k), mode, gen, rows).view(*lead, table, k),
           "b": torch.stack([scale_cols(torch.randn(k, n, generator=gen) * 0.1, mode, gen, cols) for _ in range(batch)]).view(*lead, k, n),
           "bias": scale_cols(torch.randn(n, generator=gen), mode, gen, cols) if opt.get("bias") else None,
           "addend": scale_cols(torch.randn(m, n, generator=gen), mode, gen, cols) if opt.get("addend") else None,
           "c0": scale_cols(torch.randn(m, n, generator=gen), mode, gen, cols) if opt.get("accumulate") else None}
    rows_idx = torch.randint(0, table, (m,), generator=gen) if opt.get("a_rows") else None
    return ops, rows_idx


def gemm_reference(name, ops, rows_idx, dtype=torch.float64):
    a = ops["a"] if rows_idx is None else ops["a"][rows_idx]
    if dtype == torch.float64:
        ref, mag = sc.gemm_ref(a, ops["b"], ops["bias"], ops["addend"])
        return (ref, mag) if ops["c0"] is None else (ref + ops["c0"].double(), mag + ops["c0"].double().abs())
    y = a @ ops["b"]
    for t in (ops["bias"], ops["addend"], ops["c0"]):
        y = y if t is None else y + t
    return y


def run_gemm(name, dev, rows_idx, fast=False, a=None, b=None, bias=None, addend=None, c0=None):
    m, k, n, opt = GEMM_CASES[name]
    batch = opt.get("batch", 1)
    at, bt = opt.get("at", False), opt.get("bt", False)
    ag = (a.transpose(-1, -2).contiguous() if at else a.contiguous()).to(dev)
    bg = (b.transpose(-1, -2).contiguous() if bt else b.contiguous()).to(dev)
    out = c0.clone().to(dev) if c0 is not None else torch.full(((batch,) if batch > 1 else ()) + (m, n), float("nan"), device=dev)
    kw = dict(bias=None if bias is None else bias.to(dev), fast=fast, a_transposed=at, b_transposed=bt, accumulate=c0 is not None,
              addend=None if addend is None else addend.to(dev), a_rows=None if rows_idx is None else rows_idx.to(dev))
    if batch > 1:
        _hip.gemm(ag.view(-1, k), bg.view(-1, n), out.view(-1, n), batch=batch, stride_a=m * k, stride_b=k * n, stride_c=m * n,
                  m=m, n=n, k=k, **kw)
        return out
    return _hip.gemm(ag, bg, out, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_is_homogeneous(gpu, name, mode):
    ops, rows_idx = gemm_operands(name, mode, rows=BASE_ROWS, cols=BASE_COLS)
    homogeneous(lambda **t: run_gemm(name, gpu, rows_idx, **t), ops,
                [("a", "bias", "addend", "c0"), ("b", "bias", "addend", "c0")], what="gemm " + name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_error_per_element(gpu, monkeypatch, name, mode):
    ops, rows_idx = gemm_operands(name, mode, seed=1)
    ref64, mag64 = gemm_reference(name, ops, rows_idx)
    default = run_gemm(name, gpu, rows_idx, **ops)
    fast = run_gemm(name, gpu, rows_idx, fast=True, **ops)
    rho = {"default": sc.componentwise(default, ref64, mag64)}
    with exact_paths(monkeypatch):
        rho["exact"] = sc.componentwise(run_gemm(name, gpu, rows_idx, **ops), ref64, mag64)
    rho["ref32"] = sc.componentwise(gemm_reference(name, ops, rows_idx, torch.float32), ref64, mag64)
    if name in SPLIT_GEMMS:
        rho["fast"] = sc.componentwise(fast, ref64, mag64)
    else:                                       # no two-term mode behind this shape: the flag changes nothing
        assert torch.equal(fast, default), name
    sc.check("gemm {} {}".format(name, mode), rho, C)


# =============================================================================================================================
# gn_xtg_f32 (weight gradients)
# =============================================================================================================================
XTG_CASES = {"one-launch": (700, 64, 32), "tiles": (700, 65, 33), "wide": (4096, 128, 64)}


def xtg_operands(name, mode, seed=0, rows=RHO_ROWS, cols=RHO_COLS):
    m, k1, k2 = XTG_CASES[name]
    gen = torch.Generator().manual_seed(m + k1 * 5 + k2 + seed)
    # x^T g: the rows of the left operand are the COLUMNS of x
    return {"x": scale_cols(torch.randn(m, k1, generator=gen), mode, gen, rows),
            "g": scale_cols(torch.randn(m, k2, generator=gen) * 0.1, mode, gen, cols)}


def check_xtg_kernel(name):
    m, k1, k2 = XTG_CASES[name]
    wide = bool(_hip.load().gn_xtg_wide_supported(m, k1, k2))
    assert wide == (name == "wide") and (k1 <= 64 and k2 <= 32) == (name == "one-launch")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(XTG_CASES))
def test_xtg_is_homogeneous(gpu, name, mode):
    check_xtg_kernel(name)
    ops = xtg_operands(name, mode, rows=BASE_ROWS, cols=BASE_COLS)
    homogeneous(lambda x, g: _hip.xtg(x.to(gpu), g.to(gpu)), ops, [("x",), ("g",)], what="xtg " + name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(XTG_CASES))
def test_xtg_error_per_element(gpu, monkeypatch, name, mode):
    check_xtg_kernel(name)
    ops = xtg_operands(name, mode, seed=1)
    x, g = ops["x"], ops["g"]
    ref64, mag64 = sc.gemm_ref(x.t(), g)
    rho = {"default": sc.componentwise(_hip.xtg(x.to(gpu), g.to(gpu)), ref64, mag64)}
    with exact_paths(monkeypatch):
        rho["exact"] = sc.componentwise(_hip.xtg(x.to(gpu), g.to(gpu)), ref64, mag64)
    rho["ref32"] = sc.componentwise(x.t() @ g, ref64, mag64)
    sc.check("xtg {} {}".format(name, mode), rho, C)


# =============================================================================================================================
# GCN-style layers
# =============================================================================================================================
GCN_CASES = {
    # name:        (n,    fin, fout, degree, options)
    "wave-per-row": (700, 24, 20, 8, dict()),
    "fused-32-16": (300, 32, 16, 8, dict(fused=True)),
    "fused-64-32": (300, 64, 32, 8, dict(fused=True)),
    "wide-fused": (4096, 64, 64, 8, dict(fused=True, wide=True)),
    "blocked-16": (4096, 32, 16, 16, dict(blocked=True)),
    "blocked-32": (4096, 64, 32, 16, dict(blocked=True)),
    "tall-product": (2048, 32, 24, 8, dict(fast=True)),            # x W on the tall-skinny split kernel: the layer's two-term mode
}
# (the LDS-staged plans are built for unit weights only)
GCN_RUNS = [(name, weighted) for name in GCN_CASES for weighted in (False, True) if not (weighted and GCN_CASES[name][4].get("blocked"))]


def gcn_operands(name, mode, weighted, seed=0, rows=RHO_ROWS, cols=RHO_COLS):
    n, fin, fout, degree, opt = GCN_CASES[name]
    gen = torch.Generator().manual_seed(n + fin * 11 + fout + seed)
    ei = sc.random_graph(n, degree, gen, isolated=0 if opt.get("blocked") else 9, symmetric=bool(opt.get("blocked")))
    ew = torch.rand(ei.shape[1], generator=gen) + 0.25 if weighted else None
    ops = {"x": scale_rows(torch.randn(n, fin, generator=gen), mode, gen, rows),
           "w": scale_cols(torch.randn(fin, fout, generator=gen) * 0.1, mode, gen, cols),
           "bias": scale_cols(torch.randn(fout, generator=gen), mode, gen, cols)}
    return ops, ei, ew


class GcnRunner:
    """One myGCN on the GPU; `__call__` loads the operands it is given and runs the inference launches."""

    def __init__(self, name, ei, ew, dev, storage="fp32", arithmetic="fp32"):
        n, fin, fout, degree, opt = GCN_CASES[name]
        self.name, self.opt, self.dev = name, opt, dev
        self.conv = gripnet_amd.myGCN(fin, fout, cached=True).to(dev)
        self.conv.table_storage, self.conv.arithmetic = storage, arithmetic
        self.ei, self.ew = ei.to(dev), None if ew is None else ew.to(dev)

    def __call__(self, x, w, bias):
        with torch.no_grad():
            self.conv.weight.copy_(w.to(self.dev))
            self.conv.bias.copy_(bias.to(self.dev))
            return self.conv(x.to(self.dev), self.ei, self.ew)

    def check_kernel(self, x, w, bias):
        """The kernel the case is named after is the one that serves it."""
        (y, names) = served(lambda: self(x, w, bias))
        plan, conv, opt = self.conv.cached_result, self.conv, self.opt
        xg = x.to(self.dev)
        blocked = plan.blocked_ok(xg, conv.weight, conv.bias, y)
        assert blocked == bool(opt.get("blocked")), (self.name, plan.blocked_cols)
        if conv.table_storage == "bf16":
            assert names == ["gn_gemm_f32", "gn_graph_aggregate_bf16"], names
        elif opt.get("blocked") or opt.get("fused"):
            assert names == ["gn_graph_aggregate_f32"], names
            if not opt.get("blocked"):
                assert plan.transform_ok(conv.in_channels, conv.out_channels, xg)
                assert _hip.transform_fusable(conv.in_channels, conv.out_channels, xg) == (not opt.get("wide"))
        else:
            assert names == ["gn_gemm_f32", "gn_graph_aggregate_f32"], names
            assert not plan.transform_ok(conv.in_channels, conv.out_channels, xg)
        return y


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,weighted", GCN_RUNS)
def test_gcn_is_homogeneous(gpu, name, mode, weighted):
    ops, ei, ew = gcn_operands(name, mode, weighted, rows=BASE_ROWS, cols=BASE_COLS)
    run = GcnRunner(name, ei, ew, gpu)
    run.check_kernel(**ops)
    homogeneous(run, ops, [("x", "bias")], what="gcn " + name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,weighted", GCN_RUNS)
def test_gcn_error_per_element(gpu, monkeypatch, name, mode, weighted):
    ops, ei, ew = gcn_operands(name, mode, weighted, seed=1)
    ref64, mag64 = sc.gcn_ref(ops["x"], ops["w"], ops["bias"], ei, ew)
    assert bool((mag64 > 0).all())
    rho = {"default": sc.componentwise(GcnRunner(name, ei, ew, gpu).check_kernel(**ops), ref64, mag64)}
    with exact_paths(monkeypatch):
        rho["exact"] = sc.componentwise(GcnRunner(name, ei, ew, gpu)(**ops), ref64, mag64)
    rho["ref32"] = sc.componentwise(sc.gcn_ref(ops["x"], ops["w"], ops["bias"], ei, ew, torch.float32), ref64, mag64)
    if GCN_CASES[name][4].get("fast"):           # the layer's dense product is tall enough for the split kernel
        rho["fast"] = sc.componentwise(GcnRunner(name, ei, ew, gpu, arithmetic="fast")(**ops), ref64, mag64)
    sc.check("gcn {} {} {}".format(name, mode, "weighted" if weighted else "unweighted"), rho, C)


BF16_CASE = "wide-fused"          # 4096 nodes, degree 8: lane groups own rows (k_aggregate_group_bf16)


@pytest.mark.parametrize("mode", MODES)
def test_gcn_bf16_table_is_homogeneous(gpu, mode):
    """A bf16 rounding is scale-free too: the layer with bf16 table storage commutes with a power-of-two factor."""
    ops, ei, ew = gcn_operands(BF16_CASE, mode, True, rows=BASE_ROWS, cols=BASE_COLS)
    run = GcnRunner(BF16_CASE, ei, ew, gpu, storage="bf16")
    run.check_kernel(**ops)
    homogeneous(run, ops, [("x", "bias")], what="gcn bf16 table")


@pytest.mark.parametrize("mode", MODES)
def test_gcn_bf16_table_is_exact_against_the_rounded_table_at_any_scale(gpu, mode):
    """bf16 storage is not held to fp32's error against the fp32 layer; it is held to it against the same sum over the
    rounded table (the table the layer's own product stores)."""
    ops, ei, ew = gcn_operands(BF16_CASE, mode, True, seed=1)
    n, fin, fout = GCN_CASES[BF16_CASE][:3]
    table = torch.empty(n, fout, dtype=torch.bfloat16, device=gpu)
    _hip.gemm(ops["x"].to(gpu), ops["w"].to(gpu), table, out_bf16=True)
    xw16 = table.float().cpu()
    ei2, norm = orc.gcn_norm(ei, n, ew)
    norm64 = orc.gcn_norm(ei, n, ew.double())[1]
    ref64 = orc.gcn_propagate(xw16.double(), ei2, norm64, ops["bias"].double())
    mag64 = orc.gcn_propagate(xw16.double().abs(), ei2, norm64, ops["bias"].double().abs())
    rho = {"default": sc.componentwise(GcnRunner(BF16_CASE, ei, ew, gpu, storage="bf16").check_kernel(**ops), ref64, mag64)}
    rho["ref32"] = sc.componentwise(orc.gcn_propagate(xw16, ei2, norm, ops["bias"]), ref64, mag64)
    # (GN_DISABLE_FAST=1 rounds the table of ANOTHER product kernel: where the two products differ in the last bit a bf16
    # rounding flips, 2^-8 of an entry - so the fp32 CPU sum over the same table is the only yardstick here)
    sc.check("gcn bf16 table " + mode, rho, C)


def test_gcn_norm_is_invariant_under_a_factor_on_every_weight(gpu):
    """norm = deg[src]^-1/2 w deg[dst]^-1/2 (gn_gcn_plan_create, exported): the same bits when every edge weight is multiplied
    by 4^k - sqrt(4^k deg) is exact.  Every node carries a self loop in the list (a node without one gets a loop of weight
    1, which no factor on the weights reaches); loops of weight 0 on nodes without another incoming edge give degree 0:
    the "inf -> 0" rule."""
    gen = torch.Generator().manual_seed(5)
    n, e, lonely = 500, 4000, 25
    ei = torch.stack([torch.randint(0, n, (e,), generator=gen), torch.randint(0, n - lonely, (e,), generator=gen)])
    ei = ei[:, ei[0] != ei[1]]
    loops = torch.arange(n).repeat(2, 1)
    w = torch.cat([torch.rand(ei.shape[1], generator=gen) + 0.1, torch.rand(n, generator=gen) + 0.1])
    w[-lonely:] = 0.0
    ei = torch.cat([ei, loops], dim=1)
    base_ei, base = gripnet_amd.myGCN.norm(ei.to(gpu), n, w.to(gpu))
    ref_ei, ref = orc.gcn_norm(ei, n, w)
    assert torch.equal(base_ei.cpu(), ref_ei) and float((base.cpu() - ref).abs().max()) <= 1e-6
    assert bool(torch.isfinite(base).all()) and int((base == 0).sum()) >= lonely and int((ref == 0).sum()) == int((base == 0).sum())
    for k in (-10, 10):
        got_ei, got = gripnet_amd.myGCN.norm(ei.to(gpu), n, (w * 4.0 ** k).to(gpu))
        assert torch.equal(got_ei, base_ei)
        assert torch.equal(got.view(torch.int32), base.view(torch.int32)), (k, int((got != base).sum()))


# ---- external layer and merges ------------------------------------------------------------------------------------------------
INTER_CASES = {
    # name:    (source_dim, target_dim, target_feat_dim, if_one_external, mod)
    "cat": (32, 16, 16, True, "cat"),
    "add-equal": (32, 16, 16, True, "add"),          # gn_merge_f32 mode 2
    "add-down": (32, 16, 24, True, "add"),           # gn_gemm_f32 + mode 3
    "conv-only": (24, 20, 0, False, "cat"),
}


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(INTER_CASES))
def test_external_layer_is_homogeneous(gpu, name, mode, weighted):
    src_dim, tgt_dim, tf_dim, one, mod = INTER_CASES[name]
    gen = torch.Generator().manual_seed(src_dim + tgt_dim * 3 + tf_dim)
    n_src, n_tgt, e = 300, 210, 2500
    ei = torch.stack([torch.randint(0, n_src, (e,), generator=gen), torch.randint(0, n_tgt - 7, (e,), generator=gen)]).to(gpu)
    ew = (torch.rand(e, generator=gen) + 0.25).to(gpu) if weighted else None
    m = gripnet_amd.interGraph(src_dim, tgt_dim, n_tgt, target_feat_dim=tf_dim, if_one_external=one).to(gpu)
    ops = {"x": scale_rows(torch.randn(n_src, src_dim, generator=gen), mode, gen, BASE_ROWS),
           "bias": torch.randn(tgt_dim, generator=gen)}
    if one:
        ops["target_feat"] = scale_rows(torch.randn(n_tgt, tf_dim, generator=gen), mode, gen, BASE_ROWS)

    def run(x, bias, target_feat=None):
        with torch.no_grad():
            m.conv.bias.copy_(bias.to(gpu))
            if target_feat is not None:
                m.target_feat.copy_(target_feat.to(gpu))
            return m(x.to(gpu), ei, ew, if_relu=True, mod=mod)

    homogeneous(run, ops, [tuple(ops)], what="interGraph " + name)


@pytest.mark.parametrize("mode", MODES)
def test_external_layer_error_per_element(gpu, monkeypatch, mode):
    """The bipartite conv of interGraph (rows are targets, closed form) before ReLU and merge."""
    gen = torch.Generator().manual_seed(77)
    n_src, n_tgt, e, fin, fout = 300, 210, 2500, 32, 16
    ei = torch.stack([torch.randint(0, n_src, (e,), generator=gen), torch.randint(0, n_tgt - 7, (e,), generator=gen)])
    ew = torch.rand(e, generator=gen) + 0.25
    x = scale_rows(torch.randn(n_src, fin, generator=gen), mode, gen)
    w = scale_cols(torch.randn(fin, fout, generator=gen) * 0.1, mode, gen)
    b = scale_cols(torch.randn(fout, generator=gen), mode, gen)
    ref64, mag64 = sc.bipartite_ref(x, w, b, ei, n_tgt, ew)

    def run():
        conv = gripnet_amd.myGCN(fin, fout, cached=True).to(gpu)
        with torch.no_grad():
            conv.weight.copy_(w.to(gpu))
            conv.bias.copy_(b.to(gpu))
            return conv.forward_bipartite(x.to(gpu), ei.to(gpu), n_tgt, ew.to(gpu))

    y, names = served(run)
    assert names == ["gn_graph_aggregate_f32"], names           # 32 -> 16: the fused transform
    rho = {"default": sc.componentwise(y, ref64, mag64)}
    with exact_paths(monkeypatch):
        rho["exact"] = sc.componentwise(run(), ref64, mag64)
    rho["ref32"] = sc.componentwise(sc.bipartite_ref(x, w, b, ei, n_tgt, ew, torch.float32), ref64, mag64)
    sc.check("bipartite conv " + mode, rho, C)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("merge_mode", [1, 2, 3, 4])
def test_merges_are_homogeneous(gpu, merge_mode, mode):
    gen = torch.Generator().manual_seed(merge_mode)
    ops = {k: scale_rows(torch.randn(333, 21, generator=gen), mode, gen, BASE_ROWS) for k in ("dst", "src", "src2")}

    def run(dst, src, src2):
        return _hip.merge(dst.clone().to(gpu), src.to(gpu), merge_mode, src2=src2.to(gpu) if merge_mode == 4 else None)

    y = run(**ops)
    d, s, s2 = (ops[k] for k in ("dst", "src", "src2"))
    want = {1: s.abs(), 2: (d + s.abs()) / 2, 3: (d + torch.relu(s)) / 2, 4: (d + s + s2) / 3}[merge_mode]
    assert torch.equal(y.cpu(), want), merge_mode                # (one rounding per operation, as torch's)
    homogeneous(run, ops, [("dst", "src", "src2")], what="merge mode {}".format(merge_mode))


# =============================================================================================================================
# relational layer
# =============================================================================================================================
RGCN_CASES = {
    # name:       (n,   fin, fout, bases, path, options)            path: what RgcnPlan.path reports for the call
    "pair-32": (645, 48, 32, 32, "pair", dict()),                   # destination-major, the library's own choice
    "pair-5": (200, 32, 32, 5, "pair", dict()),
    "lds-5": (200, 32, 32, 5, "lds", dict(kernel="lds")),           # LDS-resident accumulator, by flag
    "lds-8": (769, 48, 32, 8, "lds", dict()),                       # ... and as the library's own choice
    "general-8": (769, 48, 32, 8, "general", dict(kernel="general")),
    "pair-planes": (645, 48, 32, 32, "pair", dict(planes=True)),    # x arrives with the bf16 split planes its producer left
}
REL_SIZES = [0, 9000, 3, 0, 700, 1, 2500, 0]


def rgcn_operands(name, mode, seed=0, rows=RHO_ROWS, cols=RHO_COLS):
    n, fin, fout, bases, path, opt = RGCN_CASES[name]
    gen = torch.Generator().manual_seed(n * 7 + fin + bases + seed)
    blocks = [torch.randint(0, max(1, n - n // 7), (2, s), generator=gen) for s in REL_SIZES]   # the last nodes: no edge at all
    rei, rl = torch.cat(blocks, dim=1), gripnet_amd.utils.get_range_list(blocks)
    std = 1 / fin ** 0.5
    ops = {"x": scale_rows(torch.randn(n, fin, generator=gen), mode, gen, rows),
           "basis": scale_cols((torch.randn(bases, fin, fout, generator=gen) * std).view(-1, fout), mode, gen, cols).view(bases, fin, fout),
           "att": torch.randn(len(REL_SIZES), bases, generator=gen) / bases ** 0.5,
           "root": scale_cols(torch.randn(fin, fout, generator=gen) * std, mode, gen, cols),
           "bias": scale_cols(torch.randn(fout, generator=gen), mode, gen, cols)}
    return ops, rei, rl


class RgcnRunner:
    def __init__(self, name, rei, rl, dev, kernel=None, arithmetic="fp32"):
        n, fin, fout, bases, path, opt = RGCN_CASES[name]
        self.name, self.dev, self.opt = name, dev, opt
        self.layer = gripnet_amd.myRGCN(fin, fout, len(REL_SIZES), bases, False, bias=True).to(dev)
        self.layer.kernel, self.layer.arithmetic = kernel or opt.get("kernel", "auto"), arithmetic
        self.rei, self.rl = rei.to(dev), rl

    def __call__(self, x, basis, att, root, bias):
        m = self.layer
        with torch.no_grad():
            for p, v in ((m.basis, basis), (m.att, att), (m.root, root), (m.bias, bias)):
                p.copy_(v.to(self.dev))
            xg = x.to(self.dev)
            if self.opt.get("planes"):           # the planes a producing layer would have left with x
                _hip.SplitPlanes(xg.shape[0], m.in_channels // 16, self.dev).fill_from(xg).tag(xg)
                assert _hip.SplitPlanes.of(xg, m.in_channels // 16) is not None
            return m(xg, self.rei, None, self.rl)

    def path(self):
        m = self.layer
        return m._plan.path(m.in_channels, m.out_channels, m.num_bases, m._fast(), m.kernel)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(RGCN_CASES))
def test_rgcn_is_homogeneous(gpu, name, mode):
    """Linear in (x, bias), in (basis, root, bias) and in (att, root, bias): the root term and the bias do not pass
    through W_r = sum_b att[r, b] basis[b]."""
    ops, rei, rl = rgcn_operands(name, mode, rows=BASE_ROWS, cols=BASE_COLS)
    run = RgcnRunner(name, rei, rl, gpu)
    run(**ops)
    assert run.path() == RGCN_CASES[name][4]
    homogeneous(run, ops, [("x", "bias"), ("basis", "root", "bias"), ("att", "root", "bias")], what="rgcn " + name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(RGCN_CASES))
def test_rgcn_error_per_element(gpu, monkeypatch, name, mode):
    ops, rei, rl = rgcn_operands(name, mode, seed=1)
    ref64, mag64 = sc.rgcn_ref(ops["x"], rei, rl, ops)
    assert bool((mag64 > 0).all())
    path = RGCN_CASES[name][4]
    default = RgcnRunner(name, rei, rl, gpu)
    y = default(**ops)
    assert default.path() == path
    rho = {"default": sc.componentwise(y, ref64, mag64)}
    for kernel in ("general", "lds"):
        exact = RgcnRunner(name, rei, rl, gpu, kernel=kernel)
        rho["exact-" + kernel] = sc.componentwise(exact(**ops), ref64, mag64)
        assert exact.path() == kernel
    with exact_paths(monkeypatch):
        exact = RgcnRunner(name, rei, rl, gpu, kernel="auto")
        rho["exact-env"] = sc.componentwise(exact(**ops), ref64, mag64)
        assert exact.path() == "general"
    rho["ref32"] = sc.componentwise(sc.rgcn_ref(ops["x"], rei, rl, ops, torch.float32), ref64, mag64)
    fast = RgcnRunner(name, rei, rl, gpu, arithmetic="fast")
    yf = fast(**ops)
    assert fast.path() == path
    if path == "lds":                            # fp32 matrix instruction: no two-term mode behind this kernel
        assert torch.equal(yf, y)
    else:
        rho["fast"] = sc.componentwise(yf, ref64, mag64)
    sc.check("rgcn {} {}".format(name, mode), rho, C)


# =============================================================================================================================
# decoders
# =============================================================================================================================
DEC_SIZES = [900, 0, 1500, 40, 1100, 700, 760]          # R = 7 relations, 5000 pairs


def decoder_operands(f, mode, seed=0, rows=RHO_ROWS, cols=RHO_COLS, n=645):
    gen = torch.Generator().manual_seed(f * 13 + seed)
    ei = torch.randint(0, n, (2, sum(DEC_SIZES)), generator=gen)
    et = torch.repeat_interleave(torch.arange(len(DEC_SIZES)), torch.tensor(DEC_SIZES))
    rl = gripnet_amd.utils.get_range_list([ei[:, :s] for s in DEC_SIZES])
    ops = {"z": scale_rows(torch.randn(n, f, generator=gen), mode, gen, rows),
           "weight": scale_cols(torch.randn(len(DEC_SIZES), f, generator=gen) / f ** 0.5, mode, gen, cols)}
    return ops, ei, et, rl


class DecoderRunner:
    """One multiRelaInnerProductDecoder; `kind`: "plan-less" (a list's first sighting), "planned" (its second), "packed"
    (a NegativeSampler's list, scored from its 32-bit words)."""
    ENTRY = {"plan-less": "gn_distmult_forward_f32", "planned": "gn_distmult_plan_forward_f32",
             "packed": "gn_distmult_packed_forward_f32"}

    def __init__(self, f, kind, ei, et, rl, dev, n=645, expect_entry=True):
        self.dm = multiRelaInnerProductDecoder(f, len(DEC_SIZES)).to(dev)
        self.kind, self.dev, self.expect_entry = kind, dev, expect_entry
        self.et = et.to(dev)
        self.ei = _hip.NegativeSampler(ei.to(dev), n, rl).sample(seed=3) if kind == "packed" else ei.to(dev)
        assert (_hip.packed_pairs(self.ei) is not None) == (kind == "packed")

    def __call__(self, z, weight):
        with torch.no_grad():
            self.dm.weight.copy_(weight.to(self.dev))
            zg = z.to(self.dev)
            if self.kind != "planned":            # a first sighting, every time
                self.dm.forget_static()
            elif self.kind == "planned" and self.dm.plan_for(zg, self.ei, self.et) is None:
                self.dm(zg, self.ei, self.et, sigmoid=False)              # the first sighting
            out, names = served(lambda: self.dm(zg, self.ei, self.et, sigmoid=False))
        if self.expect_entry:
            assert names == [self.ENTRY[self.kind]], (self.kind, names)
        return out


# (a width that is no multiple of 4 has no plan and no packed form: the general kernel's scalar columns serve it)
DEC_KINDS = [(80, "plan-less"), (80, "planned"), (80, "packed"), (45, "plan-less")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f,kind", DEC_KINDS)
def test_distmult_is_homogeneous(gpu, f, kind, mode):
    ops, ei, et, rl = decoder_operands(f, mode, rows=BASE_ROWS, cols=BASE_COLS)
    run = DecoderRunner(f, kind, ei, et, rl, gpu)
    homogeneous(run, ops, [("weight",)], what="distmult {} {} in weight".format(f, kind))
    homogeneous(run, ops, [("z",)], scales=Z_SCALES, power=2, what="distmult {} {} in z".format(f, kind))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f,kind", DEC_KINDS)
def test_distmult_error_per_element(gpu, monkeypatch, f, kind, mode):
    ops, ei, et, rl = decoder_operands(f, mode, seed=1)
    run = DecoderRunner(f, kind, ei, et, rl, gpu)
    pairs = run.ei.cpu()                                                  # (the sampler's pairs, for "packed")
    ref64, mag64 = sc.distmult_ref(ops["z"], pairs, et, ops["weight"])
    rho = {"default": sc.componentwise(run(**ops), ref64, mag64)}
    with exact_paths(monkeypatch):
        exact = DecoderRunner(f, "plan-less", pairs, et, rl, gpu, expect_entry=False)
        rho["exact"] = sc.componentwise(exact(**ops), ref64, mag64)
    rho["ref32"] = sc.componentwise(sc.distmult_ref(ops["z"], pairs, et, ops["weight"], torch.float32), ref64, mag64)
    sc.check("distmult f={} {} {}".format(f, kind, mode), rho, C)
    _hip.raise_if_index_errors(gpu)


def class_operands(classes, mode, seed=0, rows=RHO_ROWS, cols=RHO_COLS):
    gen = torch.Generator().manual_seed(classes + seed)
    n, f = 645, 80
    return ({"z": scale_rows(torch.randn(n, f, generator=gen), mode, gen, rows),
             "weight": scale_cols(torch.randn(f, classes, generator=gen) * 0.1, mode, gen, cols)},
            torch.randint(0, n, (1001,), generator=gen))


def run_class_scores(dev, nodes, z, weight):
    mc = multiClassInnerProductDecoder(z.shape[1], weight.shape[1]).to(dev)
    with torch.no_grad():
        mc.weight.copy_(weight.to(dev))
        return mc(z.to(dev), nodes.to(dev), softmax=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("classes", [8, 17])              # the one-pass kernel (<= 16 classes); the row-gather GEMM behind it
def test_class_scores_are_homogeneous(gpu, classes, mode):
    ops, nodes = class_operands(classes, mode, rows=BASE_ROWS, cols=BASE_COLS)
    homogeneous(lambda **t: run_class_scores(gpu, nodes, **t), ops, [("z",), ("weight",)], what="class scores {}".format(classes))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("classes", [8, 17])
def test_class_scores_error_per_element(gpu, monkeypatch, classes, mode):
    ops, nodes = class_operands(classes, mode, seed=1)
    ref64, mag64 = sc.class_ref(ops["z"], nodes, ops["weight"])
    rho = {"default": sc.componentwise(run_class_scores(gpu, nodes, **ops), ref64, mag64)}
    with exact_paths(monkeypatch):
        rho["exact"] = sc.componentwise(run_class_scores(gpu, nodes, **ops), ref64, mag64)
    rho["ref32"] = sc.componentwise(sc.class_ref(ops["z"], nodes, ops["weight"], torch.float32), ref64, mag64)
    sc.check("class scores {} {}".format(classes, mode), rho, C)


@pytest.mark.parametrize("mode", MODES)
def test_rank_and_top_k_survive_a_factor(gpu, mode):
    """A real-valued model (randn, not the integer one of the ranking tests): a positive power-of-two factor on the relation
    weights leaves every comparison of two logits as it was - `greater` and `ties` identical; a factor on z leaves the
    partner ids identical and multiplies the logits by s^2."""
    n, f = 645, 80
    ops, ei, et, rl = decoder_operands(f, mode, rows=BASE_ROWS, cols=BASE_COLS)
    gen = torch.Generator().manual_seed(9)
    pick = torch.randperm(ei.shape[1], generator=gen)[:300]
    pairs, rel = ei[:, pick].contiguous().to(gpu), et[pick].contiguous().to(gpu)
    dm = multiRelaInnerProductDecoder(f, len(DEC_SIZES)).to(gpu)

    def rank(z, weight):
        with torch.no_grad():
            dm.weight.copy_(weight.to(gpu))
        return dm.rank(z.to(gpu), pairs, rel)

    def top_k(z, weight):
        with torch.no_grad():
            dm.weight.copy_(weight.to(gpu))
        return dm.top_k(z.to(gpu), pairs[0], rel, 10)

    greater, ties = rank(**ops)
    assert int(greater.min()) >= 0 and int(greater.max()) > 0 and int(greater.float().mean()) > 50
    for s in sc.pow2_scales:
        g2, t2 = rank(ops["z"], ops["weight"] * s)
        assert torch.equal(g2, greater) and torch.equal(t2, ties), s
    scores, ids = top_k(**ops)
    assert bool(torch.isfinite(scores).all()) and int(ids.min()) >= 0
    for s in Z_SCALES:
        s2, i2 = top_k(ops["z"] * s, ops["weight"])
        assert torch.equal(i2, ids), s
        assert torch.equal(s2, scores * (s * s)), s
    _hip.raise_if_index_errors(gpu)


# =============================================================================================================================
# backward passes: a factor on the upstream gradient
# =============================================================================================================================
def gcn_backward(name, dev, ei, ew, x, w, bias, g):
    n, fin, fout = GCN_CASES[name][:3]
    conv = gripnet_amd.myGCN(fin, fout, cached=True).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w.to(dev))
        conv.bias.copy_(bias.to(dev))
    xg = x.to(dev).requires_grad_(True)
    y = conv(xg, ei.to(dev), None if ew is None else ew.to(dev))
    return torch.autograd.grad(y, [xg, conv.weight, conv.bias], g.to(dev))


def rgcn_backward(name, dev, rei, rl, x, basis, att, root, bias, g):
    run = RgcnRunner(name, rei, rl, dev)
    m = run.layer
    with torch.no_grad():
        for p, v in ((m.basis, basis), (m.att, att), (m.root, root), (m.bias, bias)):
            p.copy_(v.to(dev))
    xg = x.to(dev).requires_grad_(True)
    y = m(xg, run.rei, None, rl)
    return torch.autograd.grad(y, [xg, m.basis, m.att, m.root, m.bias], g.to(dev))


def distmult_backward(f, kind, dev, ei, et, z, weight, g):
    dm = multiRelaInnerProductDecoder(f, len(DEC_SIZES)).to(dev)
    with torch.no_grad():
        dm.weight.copy_(weight.to(dev))
    eg, tg = ei.to(dev), et.to(dev)
    if kind == "planned":
        dm.register_static(eg, tg, num_nodes=z.shape[0])
    zg = z.to(dev).requires_grad_(True)
    y = dm(zg, eg, tg, sigmoid=False)
    return torch.autograd.grad(y, [zg, dm.weight], g.to(dev))


BWD_GCN = ["wave-per-row", "fused-64-32", "wide-fused"]


def upstream(shape, mode, gen, rows):
    g = torch.randn(*shape, generator=gen)
    return g if mode == "unit" else (sc.mixed_scale(g.view(-1, 1), rows[0], rows[1], 0, gen).view(-1) if g.dim() == 1 else
                                     sc.mixed_scale(g, rows[0], rows[1], 0, gen))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", BWD_GCN)
def test_gcn_backward_is_homogeneous_in_the_upstream_gradient(gpu, name, mode):
    ops, ei, ew = gcn_operands(name, mode, True, rows=BASE_ROWS, cols=BASE_COLS)
    ops["g"] = upstream((GCN_CASES[name][0], GCN_CASES[name][2]), mode, torch.Generator().manual_seed(1), BASE_ROWS)
    homogeneous(lambda **t: gcn_backward(name, gpu, ei, ew, **t), ops, [("g",)], what="gcn backward " + name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", BWD_GCN)
def test_gcn_backward_error_per_element(gpu, monkeypatch, name, mode):
    ops, ei, ew = gcn_operands(name, mode, True, seed=1)
    g = upstream((GCN_CASES[name][0], GCN_CASES[name][2]), mode, torch.Generator().manual_seed(2), RHO_ROWS)
    leaves = [ops["x"], ops["w"], ops["bias"]]
    fn = lambda x, w, b: orc.gcn_forward(x, w, b, ei, ew.to(x.dtype))
    ref64, mag64 = sc.grads_ref(fn, leaves, g)
    ref32 = sc.grads_ref(fn, leaves, g, torch.float32)
    got = gcn_backward(name, gpu, ei, ew, g=g, **ops)
    with exact_paths(monkeypatch):
        exact = gcn_backward(name, gpu, ei, ew, g=g, **ops)
    for i, key in enumerate(("dx", "dweight", "dbias")):
        rho = {"default": sc.componentwise(got[i], ref64[i], mag64[i]), "exact": sc.componentwise(exact[i], ref64[i], mag64[i]),
               "ref32": sc.componentwise(ref32[i], ref64[i], mag64[i])}
        sc.check("gcn backward {} {} {}".format(name, mode, key), rho, C)


BWD_RGCN = ["pair-32", "pair-5", "lds-8"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", BWD_RGCN)
def test_rgcn_backward_is_homogeneous_in_the_upstream_gradient(gpu, name, mode):
    ops, rei, rl = rgcn_operands(name, mode, rows=BASE_ROWS, cols=BASE_COLS)
    ops["g"] = upstream((RGCN_CASES[name][0], RGCN_CASES[name][2]), mode, torch.Generator().manual_seed(1), BASE_ROWS)
    homogeneous(lambda **t: rgcn_backward(name, gpu, rei, rl, **t), ops, [("g",)], what="rgcn backward " + name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", BWD_RGCN)
def test_rgcn_backward_error_per_element(gpu, monkeypatch, name, mode):
    ops, rei, rl = rgcn_operands(name, mode, seed=1)
    g = upstream((RGCN_CASES[name][0], RGCN_CASES[name][2]), mode, torch.Generator().manual_seed(2), RHO_ROWS)
    keys = ("x", "basis", "att", "root", "bias")
    leaves = [ops[k] for k in keys]
    fn = lambda x, basis, att, root, bias: orc.rgcn_forward(x, rei, rl, basis, att, root, bias)
    ref64, mag64 = sc.grads_ref(fn, leaves, g)
    ref32 = sc.grads_ref(fn, leaves, g, torch.float32)
    got = rgcn_backward(name, gpu, rei, rl, g=g, **ops)
    with exact_paths(monkeypatch):
        exact = rgcn_backward(name, gpu, rei, rl, g=g, **ops)
    for i, key in enumerate(keys):
        rho = {"default": sc.componentwise(got[i], ref64[i], mag64[i]), "exact": sc.componentwise(exact[i], ref64[i], mag64[i]),
               "ref32": sc.componentwise(ref32[i], ref64[i], mag64[i])}
        sc.check("rgcn backward {} {} d{}".format(name, mode, key), rho, C)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f,kind", [(80, "plan-less"), (80, "planned"), (45, "plan-less")])
def test_distmult_backward_is_homogeneous_in_the_upstream_gradient(gpu, f, kind, mode):
    ops, ei, et, rl = decoder_operands(f, mode, rows=BASE_ROWS, cols=BASE_COLS)
    ops["g"] = upstream((ei.shape[1],), mode, torch.Generator().manual_seed(1), BASE_ROWS)
    homogeneous(lambda **t: distmult_backward(f, kind, gpu, ei, et, **t), ops, [("g",)], what="distmult backward {} {}".format(f, kind))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f,kind", [(80, "plan-less"), (80, "planned"), (45, "plan-less")])
def test_distmult_backward_error_per_element(gpu, monkeypatch, f, kind, mode):
    ops, ei, et, rl = decoder_operands(f, mode, seed=1)
    g = upstream((ei.shape[1],), mode, torch.Generator().manual_seed(2), RHO_ROWS)
    leaves = [ops["z"], ops["weight"]]
    fn = lambda z, d: orc.distmult(z, ei, et, d, sigmoid=False)
    ref64, mag64 = sc.grads_ref(fn, leaves, g)
    ref32 = sc.grads_ref(fn, leaves, g, torch.float32)
    got = distmult_backward(f, kind, gpu, ei, et, g=g, **ops)
    with exact_paths(monkeypatch):
        exact = distmult_backward(f, "plan-less", gpu, ei, et, g=g, **ops)
    for i, key in enumerate(("dz", "dweight")):
        rho = {"default": sc.componentwise(got[i], ref64[i], mag64[i]), "exact": sc.componentwise(exact[i], ref64[i], mag64[i]),
               "ref32": sc.componentwise(ref32[i], ref64[i], mag64[i])}
        sc.check("distmult backward f={} {} {} {}".format(f, kind, mode, key), rho, C)
    _hip.raise_if_index_errors(gpu)
