"""Odd layer widths and strided inputs against the float64 oracle.  The kernels pick their path from the width and from the
row alignment of every operand (vector loads where rows are 16-byte aligned with a leading dimension % 4 == 0, scalar tails
elsewhere); the other GPU tests run almost only widths that are multiples of 4 on fresh tensors.  Here every layer runs at
widths that reach each tail ({1, 3, 5, 13, 15, 17, 31, 33, 45, 50, 63, 65, 97, 127} next to the aligned 16 / 32 / 48 / 64 /
128) on fresh tensors and on column views ``big[:, k:k + f]`` with an odd k and an odd ``big.shape[1]`` - what every layer
after the first reads inside ``homoGraph(if_catout=True)`` - forward and backward.  Every failure message names the shape
and the kernel path taken."""
import pytest
import torch

import gripnet_amd
from gripnet_amd import _hip, utils
from gripnet_amd.utils import EPS
from oracle import gripnet_oracle as orc

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 2e-5, 1e-4


def _rel_err(y, ref):
    y, ref = y.detach().cpu().double(), ref.detach().cpu().double()
    assert y.shape == ref.shape, (tuple(y.shape), tuple(ref.shape))
    if not ref.numel():
        return 0.0
    return (y - ref).abs().max().item() / max(1.0, ref.abs().max().item())


def _strided(t, k, dev):
    """`t` as the column view big[:, k:k + f] of a wider matrix whose width is odd (row stride not a multiple of 4, the
    pointer not 16-byte aligned for an odd k); the other columns hold garbage the kernels must not read into the result."""
    n, f = t.shape
    w = f + k + 2 + ((f + k + 2) % 2 == 0)
    big = torch.full((n, w), float("nan"), device=dev)
    big[:, k:k + f] = t.to(dev)
    view = big[:, k:k + f]
    assert view.stride(0) % 2 == 1 and (f <= 1 or view.stride(1) == 1)
    return view


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _typed_blocks(n, sizes, gen):
    blocks = [torch.randint(0, n, (2, s), generator=gen) for s in sizes]
    ei = torch.cat(blocks, dim=1)
    et = torch.cat([torch.full((b.shape[1],), r, dtype=torch.long) for r, b in enumerate(blocks)])
    return ei, et, utils.get_range_list(blocks)


# ---- 1. decoder ---------------------------------------------------------------------------------------------------------
DEC_WIDTHS = [1, 3, 5, 13, 15, 16, 17, 31, 32, 33, 45, 48, 50, 63, 64, 65, 97, 127, 128]


def _dec_case(n, f, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    R = 5
    sizes = [min(3 * n, 900), 0, 64, 65, 1]                              # relation 1: no edges
    ei, et, rl = _typed_blocks(n, sizes, gen)
    z = torch.randn(n, f, generator=gen)
    torch.manual_seed(seed)
    dm = gripnet_amd.multiRelaInnerProductDecoder(f, R).to(dev)
    return z, ei, et, rl, dm


def test_decoder_forward_odd_widths(gpu, monkeypatch):
    """Every entry path of the decoder at every width: the first sighting (plan-less int64), the second and third (planned),
    register_static, the sampler's packed pairs and GN_DISABLE_FAST=1; fresh and strided z; n across the LDS thresholds."""
    for case, f in enumerate(DEC_WIDTHS):
        n = (37, 645, 4100)[case % 3]
        z, ei, et, rl, dm = _dec_case(n, f, 300 + case, gpu)
        eg, tg = ei.to(gpu), et.to(gpu)
        D = dm.weight.detach().cpu().double()
        for strided in (False, True):
            zg = _strided(z, 1 + 2 * (case % 3), gpu) if strided else z.to(gpu)
            first = {}
            for sig in (True, False):
                ref = orc.distmult(z.double(), ei, et, D, sigmoid=sig)
                eg = eg.clone()                                          # a list the decoder has not seen: plan-less first
                with torch.no_grad():
                    outs = [dm(zg, eg, tg, sigmoid=sig) for _ in range(3)]
                planned = dm.plan_for(zg, eg, tg) is not None
                what = (n, f, strided, sig, "planned" if planned else "plan-less")
                assert _rel_err(outs[0], ref) <= FWD_TOL, what
                assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2]), ("planned vs plan-less bits",) + what
                first[sig] = outs[0]
            reg = gripnet_amd.multiRelaInnerProductDecoder(f, 5).to(gpu)
            with torch.no_grad():
                reg.weight.copy_(dm.weight)
            reg.register_static(eg, tg, num_nodes=n)
            with torch.no_grad():
                y = reg(zg, eg, tg)
            assert torch.equal(y, first[True]), ("register_static", n, f, strided)
            # the sampler's packed pairs (16-bit ids)
            sampler = _hip.NegativeSampler(eg, n, rl)
            neg = sampler.sample(seed=case)
            packed = _hip.packed_pairs(neg) is not None
            with torch.no_grad():
                yn = dm(zg, neg, tg)
            refn = orc.distmult(z.double(), neg.cpu(), et, D)
            assert _rel_err(yn, refn) <= FWD_TOL, ("negatives", "packed" if packed else "int64", n, f, strided)
            monkeypatch.setenv("GN_DISABLE_FAST", "1")
            with torch.no_grad():
                yd = dm(zg, eg.clone(), tg)
            monkeypatch.delenv("GN_DISABLE_FAST")
            assert _rel_err(yd, orc.distmult(z.double(), ei, et, D)) <= FWD_TOL, ("GN_DISABLE_FAST", n, f, strided)
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("f", [1, 3, 13, 45, 50, 63, 64, 127])
def test_decoder_backward_odd_widths(gpu, f):
    """DistMultFn's backward, with and without sigmoid, plan-less (first sighting) and planned (third), fresh and strided z,
    against float64 autograd through the oracle."""
    n = 645 if f % 2 else 300
    z, ei, et, rl, dm = _dec_case(n, f, 700 + f, gpu)
    gen = torch.Generator().manual_seed(f)
    wgt = torch.randn(ei.shape[1], generator=gen)
    eg, tg, wg = ei.to(gpu), et.to(gpu), wgt.to(gpu)
    for sig in (True, False):
        zr, Dr = _leaf(z.double()), _leaf(dm.weight.detach().cpu().double())
        (orc.distmult(zr, ei, et, Dr, sigmoid=sig) * wgt.double()).sum().backward()
        for strided in (False, True):
            eg = eg.clone()
            got = []
            for sighting in range(3):
                if strided:
                    big = _leaf(_strided(z, 3, gpu)._base)
                    zg = big[:, 3:3 + f]
                else:
                    zg = _leaf(z.to(gpu))
                dm.weight.grad = None
                (dm(zg, eg, tg, sigmoid=sig) * wg).sum().backward()
                gz = big.grad[:, 3:3 + f] if strided else zg.grad
                if strided:
                    rest = torch.cat([big.grad[:, :3], big.grad[:, 3 + f:]], 1)
                    assert not bool(rest.ne(0).any()), "gradient leaked into the columns next to the view"
                got.append((gz.clone(), dm.weight.grad.clone()))
            planned = dm.plan_for(zg, eg, tg) is not None
            for s, (gz, gd) in enumerate(got):
                what = (n, f, sig, strided, "sighting", s, "planned" if planned and s else "plan-less")
                assert _rel_err(gz / max(1.0, zr.grad.abs().max().item()), zr.grad / max(1.0, zr.grad.abs().max().item())) <= GRAD_TOL, ("dz",) + what
                assert _rel_err(gd / max(1.0, Dr.grad.abs().max().item()), Dr.grad / max(1.0, Dr.grad.abs().max().item())) <= GRAD_TOL, ("dD",) + what
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("f", [13, 45, 50, 64])
def test_link_prediction_loss_odd_widths(gpu, f):
    """utils.link_prediction_loss with packed and with int64 negatives at a decoder width % 4 != 0 (PoseModel(gd_out=[7, 6])
    has 45): bit for bit the three separate calls, and loss and gradients against the float64 oracle."""
    from gripnet_amd.utils import link_loss, link_prediction_loss
    n = 300
    z, ei, et, rl, dm = _dec_case(n, f, 900 + f, gpu)
    eg, tg = ei.to(gpu), et.to(gpu)
    neg_packed = _hip.NegativeSampler(eg, n, rl).sample(seed=3)
    neg_plain = neg_packed.clone()
    assert _hip.packed_pairs(neg_packed) is not None and _hip.packed_pairs(neg_plain) is None
    dm.auto_static = False
    dm.register_static(eg, tg, num_nodes=n)
    for neg in (neg_packed, neg_plain):
        kind = "packed" if neg is neg_packed else "int64"
        zr, Dr = _leaf(z.double()), _leaf(dm.weight.detach().cpu().double())
        ps, ns = orc.distmult(zr, ei, et, Dr), orc.distmult(zr, neg.cpu(), et, Dr)
        loss_ref = -torch.log(ps + EPS).mean() - torch.log(1 - ns + EPS).mean()
        (0.37 * loss_ref).backward()
        outs = []
        for fused in (False, True):
            for _ in range(2):
                zg = _leaf(z.to(gpu))
                dm.weight.grad = None
                if fused:
                    loss, pos, negs = link_prediction_loss(dm, zg, eg, neg, tg)
                else:
                    pos, negs = dm(zg, eg, tg), dm(zg, neg, tg)
                    loss = link_loss(pos, negs)
                (0.37 * loss).backward()
            outs.append((loss.detach().clone(), pos.detach().clone(), negs.detach().clone(), zg.grad.clone(), dm.weight.grad.clone()))
        for a, b, name in zip(outs[0], outs[1], ("loss", "pos", "neg", "dz", "dD")):
            assert torch.equal(a, b), (name, kind, f, float((a - b).abs().max()))
        assert abs(float(outs[1][0]) - float(loss_ref)) <= FWD_TOL * max(1.0, abs(float(loss_ref))), (kind, f)
        for g, r, name in ((outs[1][3], zr.grad, "dz"), (outs[1][4], Dr.grad, "dD")):
            s = max(1.0, r.abs().max().item())
            assert _rel_err(g / s, r / s) <= GRAD_TOL, (name, kind, f)
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("f", [1, 3, 17, 127, 128])
def test_rank_and_top_k_odd_widths(gpu, f):
    """rank / top_k on the exact integer model of test_gpu_ranking at odd widths, on a fresh and on a strided z."""
    from test_gpu_ranking import decoder_with, exact_scores, integer_case, keys_of, known_mask, ref_rank, ref_topk
    from gripnet_amd.decoder import KnownPairs
    n = 645
    z, d, lists, qi, qt = integer_case(n, f, 500 + f, gpu)
    dec = decoder_with(d, gpu)
    known = KnownPairs(lists, n, d.shape[0])
    scores = exact_scores(z, d, qi[0], qt)
    mask = known_mask(qi[0], qt, n, keys_of(lists, n))
    g_ref, t_ref = ref_rank(scores, qi[1], mask)
    val, idx = ref_topk(scores, mask, 10)
    for strided in (False, True):
        zf = _strided(z.to(torch.float32), 3, gpu) if strided else z.to(torch.float32)
        greater, ties = dec.rank(zf, qi, qt, known=known)
        assert torch.equal(greater.long(), g_ref) and torch.equal(ties.long(), t_ref), ("rank", n, f, strided)
        s, i = dec.top_k(zf, qi[0], qt, 10, known=known)
        assert torch.equal(i, idx) and torch.equal(s.to(torch.float64), val), ("top_k", n, f, strided)
    _hip.raise_if_index_errors(gpu)


# ---- 2. GCN layer -------------------------------------------------------------------------------------------------------
# (n, fin, fout, strided x, GN_BLOCKED_ANY): the LDS-staged path at fout 16 / 32, the wave-per-row kernels elsewhere, and at
# n >= 2048 with fin % 32 == 0 the tall-skinny product with its scalar store for an odd fout
GCN_CASES = [(600, 15, 16, False, True), (600, 17, 32, True, True), (600, 16, 16, True, True), (600, 64, 32, True, True),
             (300, 1, 3, False, False), (300, 3, 1, True, False), (300, 33, 17, True, False), (300, 45, 50, False, False),
             (300, 65, 13, True, False), (4100, 64, 17, False, False), (4100, 32, 45, True, False), (300, 127, 5, True, False)]


@pytest.mark.parametrize("case", range(len(GCN_CASES)))
def test_gcn_layer_odd_widths(gpu, monkeypatch, case):
    n, fin, fout, strided, blocked = GCN_CASES[case]
    if blocked:
        monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    gen = torch.Generator().manual_seed(40 + case)
    ei = torch.randint(0, n, (2, 20 * n), generator=gen)
    x = torch.randn(n, fin, generator=gen)
    wgt = torch.randn(n, fout, generator=gen)
    torch.manual_seed(case)
    conv = gripnet_amd.myGCN(fin, fout, cached=True).to(gpu)
    conv.bias.data.normal_()
    eg = ei.to(gpu)
    xg = _strided(x, 1, gpu) if strided else x.to(gpu)
    with torch.no_grad():
        y = conv(xg, eg, _relu=True)
    plan = conv.cached_result
    path = "blocked cols {}, weight-fused blocked {}".format(plan.blocked_cols, plan.blocked_ok(xg, conv.weight, conv.bias, y))
    sd = {k: _leaf(v.detach().cpu().double()) for k, v in conv.state_dict().items()}
    xr = _leaf(x.double())
    ref = torch.relu(orc.gcn_forward(xr, sd["weight"], sd["bias"], ei, None))
    what = (n, fin, fout, strided, path)
    assert _rel_err(y, ref) <= FWD_TOL, what
    (ref * wgt.double()).sum().backward()
    if strided:
        base = _leaf(xg._base)
        xl = base[:, 1:1 + fin]
    else:
        xl = _leaf(xg)
    y2 = conv(xl, eg, _relu=True)
    assert _rel_err(y2, ref) <= FWD_TOL, ("training forward",) + what
    (y2 * wgt.to(gpu)).sum().backward()
    gx = base.grad[:, 1:1 + fin] if strided else xl.grad
    for name, g, r in (("x", gx, xr.grad), ("weight", conv.weight.grad, sd["weight"].grad), ("bias", conv.bias.grad, sd["bias"].grad)):
        s = max(1.0, r.abs().max().item())
        assert _rel_err(g / s, r / s) <= GRAD_TOL, (name,) + what


@pytest.mark.parametrize("widths", [[15, 16, 16], [16, 17, 16], [17, 32, 16], [3, 5, 13]])
def test_homograph_catout_odd_widths(gpu, monkeypatch, widths):
    """homoGraph(if_catout=True) with odd earlier widths on a graph that takes the LDS-staged gathers (GN_BLOCKED_ANY=1): the
    later layers read a misaligned column slice of the concat and write into one (15 + 16 at an odd offset of a 47-wide
    buffer), at inference and under autograd."""
    monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    n = 700
    gen = torch.Generator().manual_seed(sum(widths))
    ei = torch.randint(0, n, (2, 24 * n), generator=gen)
    x = torch.randn(n, widths[0], generator=gen)
    torch.manual_seed(sum(widths))
    hg = gripnet_amd.homoGraph(widths).to(gpu)
    for c in hg.conv_list:
        c.bias.data.normal_()
    sd = {k: _leaf(v.detach().cpu().double()) for k, v in hg.state_dict().items()}
    xr = _leaf(x.double())
    ref = orc.homo_forward(sd, "", xr, ei, if_catout=True)
    eg, xg = ei.to(gpu), x.to(gpu)
    with torch.no_grad():
        y = hg(xg, eg, if_catout=True)
        y2 = hg(xg, eg, if_catout=True)
    blocked = [c.cached_result.blocked_cols for c in hg.conv_list]
    assert _rel_err(y, ref) <= FWD_TOL, (widths, "blocked cols", blocked)
    assert torch.equal(y, y2), widths
    wgt = torch.randn(ref.shape, generator=gen)
    (ref * wgt.double()).sum().backward()
    xl = _leaf(xg)
    yt = hg(xl, eg, if_catout=True)
    assert _rel_err(yt, ref) <= FWD_TOL, (widths, "training forward")
    (yt * wgt.to(gpu)).sum().backward()
    for name, p in [("x", xl)] + list(hg.named_parameters()):
        r = xr.grad if name == "x" else sd[name].grad
        s = max(1.0, r.abs().max().item())
        assert _rel_err(p.grad / s, r / s) <= GRAD_TOL, (name, widths)


# ---- 3. relational layer ------------------------------------------------------------------------------------------------
# (fin, fout, bases): fin over every tile count NT = ceil(fin / 16) = 1..8 at fin % 16 != 0 and == 0, bases over BT = 1..4
RGCN_CASES = [(5, 3, 1), (16, 32, 17), (17, 17, 33), (32, 32, 40), (33, 1, 64), (48, 32, 40), (48, 33, 16), (50, 32, 17),
              (64, 32, 64), (64, 3, 33), (65, 17, 16), (80, 32, 17), (90, 33, 1), (96, 32, 33), (97, 1, 17), (112, 32, 16),
              (112, 17, 17), (127, 32, 16), (128, 3, 1), (13, 32, 40), (32, 32, 16), (64, 32, 32)]
RGCN_PATHS = ("auto", "pair", "lds", "general", "table")


def _rgcn_graph(n, R, seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = [(0, 1, 70, 300, 2500)[(r + seed) % 5] for r in range(R)]
    blocks = [torch.randint(0, n, (2, s), generator=gen) for s in sizes]
    for b in blocks:                                           # hubs: rows with full 64-edge chunks
        b[1, :b.shape[1] // 3] = 3 + (b.shape[1] % 2)
    return torch.cat(blocks, dim=1), utils.get_range_list(blocks), gen


@pytest.mark.parametrize("case", range(len(RGCN_CASES)))
def test_relational_layer_odd_widths(gpu, case):
    """myRGCN forward on every path the plan accepts for the shape (fresh and strided x), then x and parameter gradients
    through RgcnConvFn, against the oracle."""
    fin, fout, bases = RGCN_CASES[case]
    n = 700 if fin % 16 == 0 and fin <= 64 and fout % 4 == 0 and bases <= 32 else 900     # (the destination-major kernel: <= 768 nodes)
    R = 6
    ei, rl, gen = _rgcn_graph(n, R, case)
    x = torch.randn(n, fin, generator=gen)
    wgt = torch.randn(n, fout, generator=gen)
    torch.manual_seed(case)
    rg = gripnet_amd.myRGCN(fin, fout, R, bases, False, bias=True).to(gpu)
    rg.bias.data.normal_()
    eg = ei.to(gpu)
    sd = {k: _leaf(v.detach().cpu().double()) for k, v in rg.state_dict().items()}
    xr = _leaf(x.double())
    ref = torch.relu(orc.rgcn_forward(xr, ei, rl, sd["basis"], sd["att"], sd["root"], sd["bias"]))
    ran = set()
    for strided in (False, True):
        xg = _strided(x, 3, gpu) if strided else x.to(gpu)
        for path in RGCN_PATHS:
            rg.kernel = path
            with torch.no_grad():
                y = rg(xg, eg, None, rl, _relu=True)
            took = rg._plan.path(fin, fout, bases, path=path)
            if path not in ("auto", took):
                continue                                             # a forced kernel that does not cover the shape
            ran.add(took)
            assert _rel_err(y, ref) <= FWD_TOL, (n, fin, fout, bases, strided, path, took)
    rg.kernel = "auto"
    (ref * wgt.double()).sum().backward()
    for strided in (False, True):
        rg.zero_grad()
        if strided:
            big = _leaf(_strided(x, 3, gpu)._base)
            xl = big[:, 3:3 + fin]
        else:
            xl = _leaf(x.to(gpu))
        (rg(xl, eg, None, rl, _relu=True) * wgt.to(gpu)).sum().backward()
        gx = big.grad[:, 3:3 + fin] if strided else xl.grad
        for name, g, r in (("x", gx, xr.grad), ("basis", rg.basis.grad, sd["basis"].grad), ("att", rg.att.grad, sd["att"].grad),
                           ("root", rg.root.grad, sd["root"].grad), ("bias", rg.bias.grad, sd["bias"].grad)):
            s = max(1.0, r.abs().max().item())
            assert _rel_err(g / s, r / s) <= GRAD_TOL, (name, n, fin, fout, bases, strided, sorted(ran))


def test_relational_catout_unaligned_input_on_the_lds_path(gpu):
    """homoGraph([17, 48, 32], multi_relational=True, n_base=40): the second layer (48 -> 32, 40 bases: the LDS-accumulator
    kernel, not the destination-major one) reads cat[:, 17:65] of a 97-wide buffer."""
    n, R = 900, 5
    ei, rl, gen = _rgcn_graph(n, R, 77)
    x = torch.randn(n, 17, generator=gen)
    torch.manual_seed(77)
    hg = gripnet_amd.homoGraph([17, 48, 32], multi_relational=True, n_rela=R, n_base=40).to(gpu)
    sd = {k: _leaf(v.detach().cpu().double()) for k, v in hg.state_dict().items()}
    xr = _leaf(x.double())
    ref = orc.homo_forward(sd, "", xr, ei, range_list=rl, if_catout=True)
    eg, xg = ei.to(gpu), x.to(gpu)
    et = torch.zeros(ei.shape[1], dtype=torch.long, device=gpu)
    with torch.no_grad():
        y = hg(xg, eg, edge_type=et, range_list=rl, if_catout=True)
    paths = [c._plan.path(c.in_channels, c.out_channels, c.num_bases) for c in hg.conv_list]
    assert paths[1] == "lds", paths
    assert _rel_err(y, ref) <= FWD_TOL, paths
    wgt = torch.randn(ref.shape, generator=gen)
    (ref * wgt.double()).sum().backward()
    xl = _leaf(xg)
    yt = hg(xl, eg, edge_type=et, range_list=rl, if_catout=True)
    assert _rel_err(yt, ref) <= FWD_TOL, (paths, "training forward")
    (yt * wgt.to(gpu)).sum().backward()
    for name, p in [("x", xl)] + list(hg.named_parameters()):
        r = xr.grad if name == "x" else sd[name].grad
        s = max(1.0, r.abs().max().item())
        assert _rel_err(p.grad / s, r / s) <= GRAD_TOL, (name, paths)


# ---- 4. external layer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source_dim,target_dim,target_feat_dim,mod", [(15, 7, 6, "cat"), (17, 13, 13, "add"), (33, 5, 9, "add"),
                                                                        (48, 17, 3, "cat")])
def test_inter_graph_odd_widths(gpu, source_dim, target_dim, target_feat_dim, mod):
    n_s, n_t = 700, 129
    gen = torch.Generator().manual_seed(source_dim + target_dim)
    iei = torch.stack([torch.randint(0, n_s, (3000,), generator=gen), torch.randint(0, n_t, (3000,), generator=gen)])
    x = torch.randn(n_s, source_dim, generator=gen)
    torch.manual_seed(source_dim)
    ig = gripnet_amd.interGraph(source_dim, target_dim, n_t, target_feat_dim=target_feat_dim).to(gpu)
    ig.conv.bias.data.normal_()
    sd = {k: _leaf(v.detach().cpu().double()) for k, v in ig.state_dict().items()}
    xr = _leaf(x.double())
    ref = orc.inter_forward(sd, "", xr, iei, None, if_relu=True, mod=mod)
    eg = iei.to(gpu)
    with torch.no_grad():
        y = ig(x.to(gpu), eg, mod=mod, if_relu=True)
    what = (source_dim, target_dim, target_feat_dim, mod)
    assert _rel_err(y, ref) <= FWD_TOL, what
    wgt = torch.randn(ref.shape, generator=gen)
    (ref * wgt.double()).sum().backward()
    xl = _leaf(x.to(gpu))
    (ig(xl, eg, mod=mod, if_relu=True) * wgt.to(gpu)).sum().backward()
    for name, p in [("x", xl)] + list(ig.named_parameters()):
        r = xr.grad if name == "x" else sd[name].grad
        if r is None:                                              # (target_feat_down is unused in cat mode)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, (name,) + what
            continue
        s = max(1.0, r.abs().max().item())
        assert _rel_err(p.grad / s, r / s) <= GRAD_TOL, (name,) + what


# ---- 5. whole models ----------------------------------------------------------------------------------------------------
def test_pose_model_odd_widths_training_step(gpu):
    """PoseModel(gg_nhids=[15, 17, 16], gd_out=[7, 6]) - decoder width 45 - on make_pose("small"): one training step with
    utils.link_prediction_loss on the sampler's negatives against the oracle's float64 autograd, then Adam steps."""
    from gripnet_amd.optim import Adam
    from gripnet_amd.pipeline import PoseModel
    from gripnet_amd.synth import make_pose
    data = make_pose("small")
    torch.manual_seed(59)
    model = PoseModel(data.n_g_node, data.n_d_node, data.n_dd_edge_type, gg_nhids=[15, 17, 16], gd_out=[7, 6])
    assert model.dmt.in_dim == 45
    sd = {k: _leaf(v.double()) for k, v in model.state_dict().items()}
    model = model.to(gpu)
    dg = make_pose("small").to(gpu)
    sampler = _hip.NegativeSampler(dg.train_idx, dg.n_d_node, dg.train_range)
    neg = sampler.sample(seed=1)
    assert _hip.packed_pairs(neg) is not None
    z = model.encode(dg)
    loss, _, _ = utils.link_prediction_loss(model.dmt, z, dg.train_idx, neg, dg.train_et)
    loss.backward()
    ref = orc.pose_forward(sd, data.gg_edge_index, data.edge_weight, data.gd_edge_index, data.train_idx, data.train_et,
                           data.train_range)
    neg_ref = orc.distmult(ref["z_dd"], neg.cpu(), data.train_et, sd["dmt.weight"])
    loss_ref = -torch.log(ref["score"] + EPS).mean() - torch.log(1 - neg_ref + EPS).mean()
    loss_ref.backward()
    assert abs(float(loss) - float(loss_ref)) <= FWD_TOL * max(1.0, abs(float(loss_ref)))
    paths = [c._plan.path(c.in_channels, c.out_channels, c.num_bases) for c in model.dd.conv_list]
    for k, p in model.named_parameters():
        if sd[k].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        s = max(1.0, float(sd[k].grad.abs().max()))
        assert _rel_err(p.grad / s, sd[k].grad / s) <= GRAD_TOL, (k, paths)
    opt = Adam(model.parameters(), lr=0.01)
    losses = []
    for step in range(5):
        opt.zero_grad()
        z = model.encode(dg)
        l2, _, _ = utils.link_prediction_loss(model.dmt, z, dg.train_idx, neg, dg.train_et)
        l2.backward()
        opt.step()
        losses.append(float(l2))
    assert losses[-1] < losses[0], losses


def test_aminer_model_odd_widths(gpu):
    """AminerModel with odd pp_nhids / pa_out / aa_hidden and utils.class_loss: forward and every gradient vs the oracle."""
    from gripnet_amd.pipeline import AminerModel
    from gripnet_amd.synth import make_nc
    data = make_nc("tiny", n_p=900, e_pp=9000, n_a=301, e_pa=2000, e_aa=1500)
    torch.manual_seed(83)
    model = AminerModel(data.n_p_node, data.n_a_node, data.n_a_type, pp_nhids=(15, 17, 33), pa_out=(13, 7), aa_hidden=(31, 5))
    sd = {k: _leaf(v.double()) for k, v in model.state_dict().items()}
    model = model.to(gpu)
    nodes = torch.randperm(data.n_a_node, generator=torch.Generator().manual_seed(3))[:200]
    dg = make_nc("tiny", n_p=900, e_pp=9000, n_a=301, e_pa=2000, e_aa=1500).to(gpu)
    z, score = model(dg, nodes.to(gpu))
    loss = utils.class_loss(score, dg.a_label[nodes.to(gpu)])
    loss.backward()
    ref = orc.aminer_forward(sd, data.pp_edge_idx, data.pp_edge_weight, data.pa_edge_idx, data.aa_edge_idx, data.aa_edge_weight,
                             nodes)
    assert _rel_err(z, ref["z"]) <= FWD_TOL and _rel_err(score, ref["score"]) <= FWD_TOL
    loss_ref = -torch.log(ref["score"][torch.arange(nodes.numel()), data.a_label[nodes]] + EPS).mean()
    loss_ref.backward()
    assert abs(float(loss) - float(loss_ref)) <= FWD_TOL * max(1.0, abs(float(loss_ref)))
    for k, p in model.named_parameters():
        if sd[k].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        s = max(1.0, float(sd[k].grad.abs().max()))
        assert _rel_err(p.grad / s, sd[k].grad / s) <= GRAD_TOL, k


def test_default_pose_widths_keep_their_paths(gpu):
    """The default PoseModel widths take the kernels they took before the odd-width fixes: the destination-major relational
    kernel, the LDS-staged gene layers, and the planned positives / packed negatives of the fused link loss."""
    from gripnet_amd.pipeline import PoseModel
    from gripnet_amd.synth import make_pose
    dg = make_pose("small").to(gpu)
    torch.manual_seed(5)
    model = PoseModel(dg.n_g_node, dg.n_d_node, dg.n_dd_edge_type).to(gpu)
    neg = _hip.NegativeSampler(dg.train_idx, dg.n_d_node, dg.train_range).sample(seed=2)
    for _ in range(2):
        z = model.encode(dg)
        loss, _, _ = utils.link_prediction_loss(model.dmt, z, dg.train_idx, neg, dg.train_et)
        loss.backward()
    paths = [c._plan.path(c.in_channels, c.out_channels, c.num_bases) for c in model.dd.conv_list]
    assert paths == ["pair"], paths
    assert model.dmt.plan_for(z, dg.train_idx, dg.train_et) is not None
    assert _hip.packed_pairs(neg) is not None
    assert z.shape[1] % 4 == 0 and z.stride(0) % 4 == 0
