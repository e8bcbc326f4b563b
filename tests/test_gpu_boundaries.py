"""Every packed-id and capacity guard of the library at its last admitted and its first refused size.

The kernels narrow the reference's int64 ids (16-bit node and relation ids, 13-bit ids in the decoder plan's words, "row n" as
the zero row of an LDS table) behind guards of the form "up to this many, else the next kernel down".  Each test here builds
the smallest problem that sits exactly on such a guard, and the one just behind it, with the top ids load-bearing: the edge
list holds (n-1, n-1), (0, n-1), (n-1, 0) and (n-2, n-1) in relation 0 and in relation R-1, rows n-1, n-2 and R-1 of every
table hold a pattern unlike any other row, and the upstream gradient is non-zero on them.  The result is compared with
oracle/gripnet_oracle.py in float64 (plain float64 torch where the oracle has no such function) at the suite's bars - 2e-5
forward, 1e-4 of each gradient's largest entry, per row for per-node tables, index outputs and integer models bit for bit -
and the top rows are asserted on their own.  Where the library can say which kernel ran, the test asserts it: a path query, a
plan's presence, or the entry points that served the call (`served`: the binding's Recorder writes down every entry point
that accepted; a refused one is not written down).

Guard by guard (csrc line numbers as of ABI 159; "formula": the size is found by bisecting the library's own host-side answer):

  distmult_plan.hip:522    plan words, nodes <= 8192, relations <= 65535    test_decoder_at_the_plan_word_limit[8192|8193],
                                                                            test_decoder_relation_counts[65535|65536]
                           (a plan of 2401..8192 nodes is built but none of its kernels takes it: the LDS fit below binds first)
  decoder_route.hpp:54     node table in LDS, 16 columns of n rows <= 150 KB test_decoder_at_the_lds_table_limit (arithmetic: the
                           (plan forward, plan-less fast decoder)           library exports no query; `served` checks the arithmetic)
  host_layout.hpp:583-593  class layout rows_fit / three blocks / n > 65535  test_decoder_at_the_class_layout_limits (arithmetic, as
                                                                            above: one block, three blocks, none).  n > 65535 and the
                                                                            (uint16_t) stores at :626 are unreachable: the plan refuses
                                                                            n > 8192 before the layout is built.
  decoder_route.hpp:229    n <= 65535, r <= 65535                            n: unreachable (the LDS fit above, n <= 2400, binds first);
                                                                            r: behind Python's 32767, test_decoder_relation_counts
  distmult_bwd.hip:652,1215,1233  n <= 65535 / <= 65536                      the n, r <= 65535 test of the LDS path is gone: tables_fit_lds
                                                                            (:762, n + r <= 2400) binds first, and the static_assert
                                                                            kLdsTableBudget / 64 <= 65535 (:764) says so.  r <= 65535 stays
                                                                            for the relation-major reduction alone (:857: it decides at 200
                                                                            nodes x 65536 relations, test_decoder_relation_counts[65536]);
                                                                            <= 65536 stays as the packed entry points' argument contract
  distmult_bwd.hip:243,651        kSortMaxKeys = 4096                        no run-time test left: static_assert kLdsTableBudget / 64 <=
                                                                            kSortMaxKeys (:763).  The binding limit is the formula
                                                                            n + r <= 2400 (route_of_shapes, :851): test_decoder_backward_at_the_lds_limit
                                                                            (planned, packed and loss-fed launches; bisected on plan builds)
  _hip.py:1005,1201,1224,1312  n <= 65535, relations <= 32767               test_decoder_relation_counts[32767|32768],
                                                                            test_sampler_and_decoder_at_the_16_bit_node_limit
  negsample.hip:402,484,494  N < 2^16, R < 2^16 (narrow keys, packed words)  test_sampler_and_decoder_at_the_16_bit_node_limit[65535|65536|65537],
                                                                            test_sampler_relation_counts[65535|65536]
  negsample.hip:411        bitmap, R * words * 4 <= 128 MB                   test_sampler_at_the_bitmap_limit (arithmetic from R * words * 4)
  negsample.hip:425        staged ids, relation <= 1024 positions            tests/test_gpu_callers.py::test_sampler_kernels_draw_the_same_pairs
                                                                            (1024 and 1025 positions, tasks on and off) - not repeated
  negsample.hip:370,504    N < 2^20, R < 2^23, R * N < 2^31                  left out: memory (see below)
  host_layout.hpp:1414,1436, rel_grad.hip:342  n <= 65534                    test_relational_layer_at_the_16_bit_node_limit[65534|65535|65536]
  rel_grad.hip:388         (n + 1) * out * 4 + ... <= 160 KB (formula)       test_relational_weight_gradient_at_the_lds_limit
  rel_grad.hip:399         (n + 1) * ld_x < 2^31                             left out: memory
  gcn_blocked.hip gn_graph_plan_build_blocked  N <= 65534; (N + 1) * 4 <= 160 KB (formula)
                                                                            test_gcn_gather_at_the_lds_limit (bisected; 65534 is unreachable,
                                                                            the LDS fit binds first), test_gcn_layer_at_the_16_bit_node_limit
  rgcn_fast.hip:671-673    N <= 32767, geometry(N).tiles > 0 (formula)       test_relational_layer_at_the_lds_accumulator_limit (bisected; 32767
                                                                            is unreachable, the geometry binds first); R * tiles < 2^20: left out
                                                                            (a plan of 2^20 relations: host schedules of minutes)
  rgcn_pair.hip:776-778    up to 768 nodes, a formula of the widths          test_relational_layer_at_the_destination_major_limit (bisected)
  rgcn.hip:179-181         relation slabs of 32768                           test_relational_table_path_relation_slabs[32768|32769]
  plan.hip:459             ELL rows <= 2^20                                  test_short_row_gather_at_2_to_the_20_rows
  gather_route.hpp gather_route (lds_table rule, kLdsTableRows)  LDS-table short-row gather, rows >= 65536
                                                                            test_plain_sum_at_65536_rows[65535|65536] (no query: parity only)
  dense_route.hpp:66       batch <= 65535                                    test_dense_batch_limit
  adam.hip:35,94           64 tensors per launch; alignment                  test_adam_tensor_counts_and_update
  class_metrics.hip:23     1024 classes                                      C = 1025 is refused in tests/test_class_metrics_host.py already
  metrics.hip              4096 scores per chunk                             tests/test_gpu_parity.py (4096 / 4097) already
  distmult_rank.hip        candidate columns, KnownPairs rows               test_rank_and_top_k_at_the_16_bit_node_limit[65535|65536]

Left out on purpose (tens of gigabytes): the guards that need >= 2^31 edges or rows (plan.hip:264,438,453,481,557,
host_layout.hpp:1224,1398,1512, rel_grad.hip:399), R * N >= 2^31 known-pair rows, 2^20 sampler nodes, R * tiles >= 2^20.

No test here launches past a guard: refusals are read from the library's status (Unsupported, None plans, path queries).
"""
import pytest
import torch

import grad_cases as gc
import gripnet_amd
from gripnet_amd import _hip
from gripnet_amd.decoder import KnownPairs, multiRelaInnerProductDecoder
from gripnet_amd.utils import link_prediction_loss
from oracle import gripnet_oracle as orc
from test_gpu_ranking import exact_scores, keys_of, known_mask, ref_rank, ref_topk

pytestmark = pytest.mark.gpu

FWD, GRAD_REL, ROW_REL, ROW_ABS = 2e-5, 1e-4, 1e-4, 1e-5          # the suite's bars (test_gpu_parity, test_gpu_reference_gradients)


@pytest.fixture(autouse=True)
def every_fast_path_on(monkeypatch):
    for hook in ("GN_DISABLE_FAST", "GN_DISABLE_QUAD", "GN_DISABLE_BLOCKED", "GN_DISABLE_LDS_TABLE"):
        monkeypatch.setenv(hook, "0")
    monkeypatch.delenv("GN_SAMPLER_TASKS", raising=False)


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def served(fn):
    """(result, names of the entry points that took the calls `fn` made, in order)."""
    with _hip.Recorder() as rec:
        result = fn()
    return result, [name for _, _, name, _ in rec.calls]


def last_admitted(lo, hi, admitted, sane, what):
    """The largest n in [lo, hi) the library admits, by bisection of host-side answers (`admitted(lo)` must hold, `admitted(hi)`
    must not); asserted to lie in `sane`, so that a guard that collapses is noticed."""
    assert admitted(lo), "{}: not even n = {} is admitted".format(what, lo)
    assert not admitted(hi), "{}: n = {} is still admitted".format(what, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if admitted(mid) else (lo, mid)
    print("{}: last admitted size {}".format(what, lo))
    assert sane[0] <= lo <= sane[1], "{}: the last admitted size is {}, outside {}".format(what, lo, sane)
    return lo


def close(got, ref, bar, what):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), "{}: not finite".format(what)
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert err <= bar, "{}: off by {:.3e} (bar {:.1e})".format(what, err, bar)


def top_rows_forward(got, ref, rows, what):
    """Rows `rows` of a forward output on their own (2e-5), and they carry something."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    for i in rows:
        assert float(ref[i].abs().max()) > 1e-3, "{}: reference row {} is empty - the top id is not load-bearing".format(what, i)
        err = float((got[i] - ref[i]).abs().max())
        assert err <= FWD, "{}: TOP ROW {} off by {:.3e} (bar {:.1e})".format(what, i, err, FWD)


def top_rows_gradient(got, ref, rows, what):
    """Rows `rows` of a gradient on their own, each at 1e-4 of ITS largest entry (no share of the tensor's scale)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    for i in rows:
        scale = float(ref[i].abs().max())
        assert scale > 0.0, "{}: reference gradient row {} is zero - the top id is not load-bearing".format(what, i)
        err = float((got[i] - ref[i]).abs().max())
        assert err <= GRAD_REL * scale, "{}: TOP ROW {} off by {:.3e} = {:.2e} of its largest entry".format(what, i, err, err / scale)


def pattern(f, base, slope):
    """A row unlike any drawn one: base, base + slope, ... in a period of eight columns."""
    return base + slope * (torch.arange(f) % 8).to(torch.float32)


def pack_words(ei):
    """u | v << 16 of every pair as the int32 words gn_negative_sampler_sample_packed writes next to its draw."""
    w = ei[0] | (ei[1] << 16)
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def top_pairs(n):
    return torch.tensor([[n - 1, 0, n - 1, n - 2], [n - 1, n - 1, 0, n - 1]], dtype=torch.long)


def typed_edges(n, R, extra, gen):
    """[2, E] pairs and [E] sorted relation ids: the four top pairs in relation 0 and in relation R - 1, `extra` random ones."""
    ei = torch.cat([top_pairs(n), top_pairs(n), torch.randint(0, n, (2, extra), generator=gen)], dim=1)
    et = torch.cat([torch.zeros(4, dtype=torch.long), torch.full((4,), R - 1, dtype=torch.long),
                    torch.randint(0, R, (extra,), generator=gen)])
    order = torch.sort(et, stable=True).indices
    return ei[:, order].contiguous(), et[order].contiguous()


def range_list_of(et, R):
    ids = torch.arange(R, dtype=torch.long)
    return torch.stack([torch.searchsorted(et, ids), torch.searchsorted(et, ids, right=True)], dim=1).contiguous()


# ---- the DistMult decoder ---------------------------------------------------------------------------------------------------

def decoder_tables(n, R, f, gen):
    z = 0.3 * torch.randn(n, f, generator=gen)
    d = 0.25 * torch.randn(R, f, generator=gen)
    z[n - 1], z[n - 2] = pattern(f, 1.0, 0.03), -pattern(f, 0.8, 0.02)
    d[R - 1] = pattern(f, 0.5, -0.02)
    return z, d


def decoder_with(d, dev):
    dec = multiRelaInnerProductDecoder(d.shape[1], d.shape[0]).to(dev)
    with torch.no_grad():
        dec.weight.copy_(d.to(dev))
    return dec


def decoder_reference(z, d, ei, et, proj, sigmoid):
    z64, d64 = z.double().requires_grad_(True), d.double().requires_grad_(True)
    s = orc.distmult(z64, ei, et, d64, sigmoid)
    (s * proj.double()).sum().backward()
    return s.detach(), z64.grad, d64.grad


def check_decoder(what, n, R, ei, et, score, dz, dd, ref):
    s_ref, dz_ref, dd_ref = ref
    top = ((ei[0] >= n - 2) | (ei[1] >= n - 2) | (et == R - 1)).nonzero().view(-1)
    assert top.numel() >= 8, what
    close(score.detach().cpu()[top], s_ref[top], FWD, what + " scores of the TOP ids' edges")     # (the top ids first, then everything)
    close(score, s_ref, FWD, what + " scores")
    top_rows_gradient(dz, dz_ref, [n - 1, n - 2, 0], what + " dz")
    top_rows_gradient(dd, dd_ref, [R - 1, 0], what + " dD")
    gc.check_gradients({"z": dz, "weight": dd}, {"z": dz_ref, "weight": dd_ref}, GRAD_REL, what, row_rel=ROW_REL, row_abs=ROW_ABS)


def run_decoder(dev, n, R, f, sigmoid, static, seed, extra=4000, packed_negatives=False):
    """One forward + backward of the decoder on a list with load-bearing top ids; returns what was served and the plan."""
    gen = torch.Generator().manual_seed(seed)
    ei, et = typed_edges(n, R, extra, gen)
    z, d = decoder_tables(n, R, f, gen)
    proj = 0.5 + torch.rand(ei.shape[1], generator=gen)
    dec = decoder_with(d, dev)
    ei_g, et_g = ei.to(dev), et.to(dev)
    if packed_negatives:
        # The list under test is a sampler's draw (it carries packed words) with the top pairs written over its first and last
        # four pairs (relation 0 and relation R - 1 of the sorted list): a draw alone hardly ever names node n - 1.  The write
        # moves `_version`, so the words are attached again, in the sampler's encoding (which the sampler tests hold bit for bit).
        sampler = _hip.NegativeSampler(ei_g, n, range_list_of(et, R))
        ei_g = sampler.sample(seed=seed)
        assert (_hip.packed_pairs(ei_g) is not None) == (n <= 65535)
        ei = ei_g.cpu()
        ei[:, :4], ei[:, -4:] = top_pairs(n), top_pairs(n)
        ei_g.copy_(ei)
        if n <= 65535:
            ei_g._gn_packed = (pack_words(ei).to(dev), ei_g._version)
    plan = None
    if static:
        dec.register_static(ei_g, et_g, num_nodes=n)
    zg = z.to(dev).requires_grad_(True)
    plan = dec.plan_for(zg, ei_g, et_g) if static else None

    def step():
        out = dec(zg, ei_g, et_g, sigmoid)
        (out * proj.to(dev)).sum().backward()
        return out
    out, names = served(step)
    what = "decoder n={} R={} f={} sigmoid={} static={}".format(n, R, f, sigmoid, static)
    check_decoder(what, n, R, ei, et, out, zg.grad, dec.weight.grad, decoder_reference(z, d, ei, et, proj, sigmoid))
    _hip.raise_if_index_errors(dev)
    return names, plan, (ei_g, et_g), what


LDS_NODES_16 = 150 * 1024 // (16 * 4)           # decoder_route.hpp:54: sixteen columns of n rows inside kLdsBudget = 150 KB -> 2400


@pytest.mark.parametrize("sigmoid", [True, False])
@pytest.mark.parametrize("n", [LDS_NODES_16, LDS_NODES_16 + 1])
def test_decoder_at_the_lds_table_limit(gpu, n, sigmoid):
    """The planned decoder and the plan-less packed decoder keep sixteen columns of the node table in LDS: 2400 nodes fit, 2401
    do not and the general kernel serves them (the plan exists either way)."""
    fits = n <= LDS_NODES_16
    names, plan, _, what = run_decoder(gpu, n, 8, 16, sigmoid, True, seed=n)
    assert plan is not None, what
    assert names[0] == ("gn_distmult_plan_forward_f32" if fits else "gn_distmult_forward_f32"), (what, names)
    names, _, lists, what = run_decoder(gpu, n, 8, 16, sigmoid, False, seed=n + 7, packed_negatives=True)
    assert _hip.packed_pairs(lists[0]) is not None, what
    assert names[0] == ("gn_distmult_packed_forward_f32" if fits else "gn_distmult_forward_f32"), (what, names)


def class_rows_fit(f):
    """host_layout.hpp:584-585: rows of `f` columns (+ 64 bytes where f / 16 is even) next to 64 relation rows in 160 KB."""
    j = f // 16
    str4 = 4 * j if j % 2 else 4 * j + 4
    return (160 * 1024 - 64 * 4 * j * 16) // (str4 * 16)


@pytest.mark.parametrize("which", ["one block", "three blocks", "last three blocks", "no class layout"])
def test_decoder_at_the_class_layout_limits(gpu, which):
    """The row-class encoding of the plan at 80 features: rows_fit nodes in one block, one more in three blocks, 3 * rows_fit / 2
    as the last three-block size, one more on the column-phase kernel.  The library does not say which of the plan's kernels
    ran (their scores are the same bits): the plan must serve all four, and the top ids must come out right."""
    fit = class_rows_fit(80)
    assert 256 <= fit <= 1024, fit
    n = {"one block": fit, "three blocks": fit + 1, "last three blocks": 3 * (fit // 2), "no class layout": 3 * (fit // 2) + 1}[which]
    names, plan, _, what = run_decoder(gpu, n, 12, 80, True, True, seed=n)
    assert plan is not None and names[0] == "gn_distmult_plan_forward_f32", (what, names, "rows_fit = {}".format(fit))


@pytest.mark.parametrize("n", [8192, 8193])
def test_decoder_at_the_plan_word_limit(gpu, n):
    """13-bit node ids in the plan's words: a plan is built for 8192 nodes and refused for 8193.  Neither size fits the LDS, so
    both are scored by the general kernel - the plan of 8192 nodes is built, asked once and put aside."""
    names, plan, _, what = run_decoder(gpu, n, 8, 16, True, True, seed=n)
    assert (plan is not None) == (n <= 8192), what
    assert names[0] == "gn_distmult_forward_f32" and "gn_distmult_backward_ex_f32" in names, (what, names)


@pytest.mark.parametrize("R", [32767, 32768, 65535, 65536])
def test_decoder_relation_counts(gpu, R):
    """Relation ids at the int16 rung of the binding (32767) and the uint16 rung of the library (65535), on a small node table:
    a static list (plan up to 65535 relations) and a sampler's packed negatives (packed forward up to 32767), forward,
    backward and loss-fed backward.  The packed BACKWARD is refused by the library at these counts (its tables must fit the
    LDS: nodes + relations <= 2400), so every backward here is the int64 one."""
    n, f = 200, 16
    names, plan, lists, what = run_decoder(gpu, n, R, f, True, True, seed=R, extra=3000)
    assert (plan is not None) == (R <= 65535), what
    assert names[0] == ("gn_distmult_plan_forward_f32" if R <= 65535 else "gn_distmult_forward_f32"), (what, names)
    assert plan is None or plan.backward_plan(*lists) is None, what
    assert "gn_distmult_backward_ex_f32" in names, (what, names)
    names, _, lists, what = run_decoder(gpu, n, R, f, False, False, seed=R + 1, extra=3000, packed_negatives=True)
    assert _hip.packed_pairs(lists[0]) is not None, what
    assert names[0] == ("gn_distmult_packed_forward_f32" if R <= 32767 else "gn_distmult_forward_f32"), (what, names)
    assert "gn_distmult_backward_ex_f32" in names and "gn_distmult_backward_packed_f32" not in names, (what, names)
    loss_fed_step(gpu, n, R, f, seed=R + 2, expect_planned=False, expect_packed=False)


def loss_fed_step(dev, n, R, f, seed, expect_planned, expect_packed):
    """utils.link_prediction_loss on a static positive list and a sampler's draw against the spelled-out float64 loss."""
    gen = torch.Generator().manual_seed(seed)
    ei, et = typed_edges(n, R, 3000, gen)
    z, d = decoder_tables(n, R, f, gen)
    z, d = 0.5 * z, 0.5 * d                                  # (probabilities away from 0 and 1: the loss is not EPS alone)
    dec = decoder_with(d, dev)
    ei_g, et_g = ei.to(dev), et.to(dev)
    dec.register_static(ei_g, et_g, num_nodes=n)
    sampler = _hip.NegativeSampler(ei_g, n, range_list_of(et, R))
    neg_g = sampler.sample(seed=seed)
    neg = neg_g.cpu()
    neg[:, :4], neg[:, -4:] = top_pairs(n).flip(0), top_pairs(n).flip(0)
    neg_g.copy_(neg)
    if n <= 65535:                                           # (as in run_decoder: the draw's words, with the top pairs)
        neg_g._gn_packed = (pack_words(neg).to(dev), neg_g._version)
    zg = z.to(dev).requires_grad_(True)

    def step():
        loss = link_prediction_loss(dec, zg, ei_g, neg_g, et_g)[0]
        (2.0 * loss).backward()
        return loss
    loss, names = served(step)
    what = "loss-fed decoder n={} R={} f={}".format(n, R, f)
    z64, d64 = z.double().requires_grad_(True), d.double().requires_grad_(True)
    ref = gc.link_loss_expr(orc.distmult(z64, ei, et, d64), orc.distmult(z64, neg, et, d64))
    (2.0 * ref).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach())), (what, float(loss.detach()), float(ref.detach()))
    top_rows_gradient(zg.grad, z64.grad, [n - 1, n - 2, 0], what + " dz")
    top_rows_gradient(dec.weight.grad, d64.grad, [R - 1, 0], what + " dD")
    gc.check_gradients({"z": zg.grad, "weight": dec.weight.grad}, {"z": z64.grad, "weight": d64.grad}, GRAD_REL, what,
                       row_rel=ROW_REL, row_abs=ROW_ABS)
    assert ("gn_distmult_backward_loss_planned_f32" in names) == expect_planned, (what, names)
    assert ("gn_distmult_backward_loss_packed_f32" in names) == expect_packed, (what, names)
    _hip.raise_if_index_errors(dev)


def test_decoder_backward_at_the_lds_limit(gpu):
    """The planned, the packed and the loss-fed backward keep dz and dD in LDS: nodes + relations <= 2400 (distmult_bwd.hip:650,739).
    The last admitted node count is found by bisecting backward-plan builds; it and the next one run every backward form."""
    R, f = 8, 16
    gen = torch.Generator().manual_seed(1)
    small_ei, small_et = typed_edges(64, R, 200, gen)
    small_ei, small_et = small_ei.to(gpu), small_et.to(gpu)

    def admitted(n):
        try:
            _hip.DistMultBwdPlan(small_ei, small_et, n, R)
            return True
        except _hip.Unsupported:
            return False
    last = last_admitted(64, 8193, admitted, (1024, 4096), "decoder backward plan")
    for n in (last, last + 1):
        fits = n == last
        names, plan, lists, what = run_decoder(gpu, n, R, f, True, True, seed=n)
        what += " (last admitted {})".format(last)
        assert plan is not None and (plan.backward_plan(*lists) is not None) == fits, what
        assert ("gn_distmult_backward_planned_f32" in names) == fits, (what, names)
        names, _, lists, what = run_decoder(gpu, n, R, f, True, False, seed=n + 3, packed_negatives=True)
        assert _hip.packed_pairs(lists[0]) is not None, what
        assert ("gn_distmult_backward_packed_f32" in names) == fits, (what, names, last)
        loss_fed_step(gpu, n, R, f, seed=n + 5, expect_planned=fits, expect_packed=fits)


# ---- the sampler ------------------------------------------------------------------------------------------------------------

def no_positive_drawn(pos, neg, rl, n, what):
    pos, neg = pos.cpu(), neg.cpu()
    assert int(neg.min()) >= 0 and int(neg.max()) < n, what
    pk, nk = pos[0] * n + pos[1], neg[0] * n + neg[1]
    for r, (s, e) in enumerate(rl.tolist()):
        if e > s:
            assert not torch.isin(nk[s:e], pk[s:e]).any(), "{}: relation {} drew a positive pair".format(what, r)


@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_sampler_and_decoder_at_the_16_bit_node_limit(gpu, n):
    """65535 nodes: narrow keys and packed words; from 65536 on the 64-bit sampler and no words.  Positives on pairs of node
    n - 1; draws valid, u and v both reach 0 and n - 1, the stepped draw is the draw of seed + step; and the decoder scores
    and differentiates the draw (general kernels on either side; the words are offered up to 65535 and refused by the LDS fit)."""
    gen = torch.Generator().manual_seed(n)
    sizes = [150000, 0, 50000, 4]
    blocks = [torch.randint(0, n, (2, s), generator=gen) for s in sizes]
    blocks[0][:, :4], blocks[3] = top_pairs(n), top_pairs(n)
    pos = torch.cat(blocks, dim=1)
    rl = gripnet_amd.utils.get_range_list(blocks)
    sampler = _hip.NegativeSampler(pos.to(gpu), n, rl)
    what = "sampler n={}".format(n)
    lo, hi = torch.full((2,), n, dtype=torch.long), torch.full((2,), -1, dtype=torch.long)
    for seed in range(4):
        neg = sampler.sample(seed=seed)
        words = _hip.packed_pairs(neg)
        assert (words is not None) == (n <= 65535), what
        if words is not None:
            assert torch.equal(words.long() & 0xffffffff, neg[0] | (neg[1] << 16)), what + ": packed words"
        no_positive_drawn(pos, neg, rl, n, what)
        lo, hi = torch.minimum(lo, neg.amin(dim=1).cpu()), torch.maximum(hi, neg.amax(dim=1).cpu())
    assert lo.tolist() == [0, 0] and hi.tolist() == [n - 1, n - 1], (what, lo.tolist(), hi.tolist())   # 800,000 draws: P(miss) < 1e-5
    step = torch.full((1,), 3, dtype=torch.long, device=gpu)
    stepped = sampler.sample(seed=5, step=step).clone()
    assert int(step) == 4 and torch.equal(stepped, sampler.sample(seed=8)), what + ": stepped draw"
    _hip.raise_if_index_errors(gpu)
    names, _, lists, what = run_decoder(gpu, n, 3, 16, True, False, seed=n, packed_negatives=True)
    assert (_hip.packed_pairs(lists[0]) is not None) == (n <= 65535), what
    assert names[0] == "gn_distmult_forward_f32" and "gn_distmult_backward_ex_f32" in names, (what, names)


@pytest.mark.parametrize("R", [65535, 65536])
def test_sampler_relation_counts(gpu, R, monkeypatch):
    """65535 relations: 16-bit relation ids, bitmap and task kernel; 65536: the 64-bit sampler.  Nearly every relation is empty;
    relation 0, one in the middle and relation R - 1 hold pairs, the last one nearly all 16 pairs of its four nodes."""
    n = 50
    gen = torch.Generator().manual_seed(R)
    held = {0: torch.randint(0, n, (2, 40), generator=gen), R // 2: torch.tensor([[n - 1], [n - 1]]),
            R - 1: torch.cat([torch.randint(n - 4, n, (2, 30), generator=gen), top_pairs(n)], dim=1)}
    pos = torch.cat([held[0], held[R // 2], held[R - 1]], dim=1)
    et = torch.cat([torch.full((held[r].shape[1],), r, dtype=torch.long) for r in (0, R // 2, R - 1)])
    rl = range_list_of(et, R)
    sampler = _hip.NegativeSampler(pos.to(gpu), n, rl)
    monkeypatch.setenv("GN_SAMPLER_TASKS", "0")
    plain = _hip.NegativeSampler(pos.to(gpu), n, rl)
    monkeypatch.delenv("GN_SAMPLER_TASKS")
    what = "sampler R={}".format(R)
    live = [(r, int(rl[r, 0]), int(rl[r, 1])) for r in (0, R // 2, R - 1)]
    for seed in range(3):
        neg = sampler.sample(seed=seed)
        assert torch.equal(neg, plain.sample(seed=seed)), what + ": task kernel against the bitmap kernel"
        assert _hip.packed_pairs(neg) is not None, what
        negc = neg.cpu()
        assert int(negc.min()) >= 0 and int(negc.max()) < n, what
        for r, s, e in live:
            assert not torch.isin(negc[0, s:e] * n + negc[1, s:e], pos[0, s:e] * n + pos[1, s:e]).any(), (what, r)
    _hip.raise_if_index_errors(gpu)


def test_sampler_at_the_bitmap_limit(gpu):
    """R * words * 4 <= 128 MB decides between the bitmap and the searching sampler; both draw from one stream, so the 1024
    relations of a graph exactly at the limit (1024 nodes: 128 KB of bits each) must draw what the same relations draw in the
    graph with one relation more (128 MB + 128 KB: binary search)."""
    n = 1024
    words = ((n * n + 31) // 32 + 3) & ~3
    assert 1024 * words * 4 == 128 << 20 and 1025 * words * 4 > 128 << 20
    gen = torch.Generator().manual_seed(12)
    sizes = [5] * 1024
    sizes[0], sizes[7], sizes[1023] = 3000, 1025, 1500
    blocks = [torch.randint(0, n, (2, s), generator=gen) for s in sizes]
    blocks[0][:, :4], blocks[1023][:, :4] = top_pairs(n), top_pairs(n)
    extra = torch.cat([top_pairs(n), torch.randint(0, n, (2, 60), generator=gen)], dim=1)
    e = sum(sizes)
    draws = []
    for blk in (blocks, blocks + [extra]):
        pos = torch.cat(blk, dim=1)
        rl = gripnet_amd.utils.get_range_list(blk)
        sampler = _hip.NegativeSampler(pos.to(gpu), n, rl)
        neg = [sampler.sample(seed=s) for s in (0, 9)]
        for d in neg:
            no_positive_drawn(pos, d, rl, n, "sampler at the bitmap limit, {} relations".format(len(blk)))
        draws.append(neg)
    for a, b in zip(*draws):
        assert torch.equal(a, b[:, :e]), "the bitmap sampler and the searching sampler drew different pairs"
        assert torch.equal(_hip.packed_pairs(a), _hip.packed_pairs(b)[:e])
    _hip.raise_if_index_errors(gpu)


# ---- ranking ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65535, 65536])
def test_rank_and_top_k_at_the_16_bit_node_limit(gpu, n):
    """Filtered rank and top-k on the exact integer model of test_gpu_ranking.py: rows n - 1 and n - 2 lie outside the drawn range
    (+4 and -4: node n - 1 is the strictly best partner of the all-positive probe node 9 in relation R - 1, node n - 2 its own),
    queries on (n - 1, n - 1, R - 1) and a filter that holds pairs of node n - 1 in relation R - 1."""
    R, f = 5, 8
    gen = torch.Generator().manual_seed(n)
    z = torch.randint(-3, 4, (n, f), generator=gen)
    d = torch.randint(-2, 3, (R, f), generator=gen)
    z[n - 1], z[n - 2], z[7], z[9] = 4, -4, z[3], 3
    d[R - 1] = 2
    top, flat = top_pairs(n), torch.tensor([R - 1, R - 1, 0, R - 1])
    ki = torch.cat([top, torch.tensor([[n - 1, 0], [n - 2, n - 1]]), torch.randint(0, n, (2, 3000), generator=gen)], dim=1)
    kt = torch.cat([flat, torch.tensor([R - 1, 1]), torch.randint(0, R, (3000,), generator=gen)])
    qi = torch.cat([top, torch.tensor([[9, 9], [0, n - 1]]), torch.randint(0, n, (2, 58), generator=gen)], dim=1)
    qt = torch.cat([flat, torch.tensor([R - 1, R - 1]), torch.randint(0, R, (58,), generator=gen)])
    z, d, ki, kt, qi, qt = (t.to(gpu) for t in (z, d, ki, kt, qi, qt))
    dec = decoder_with(d.float(), gpu)
    lists = [(ki, kt)]
    known = KnownPairs(lists, n, R)
    scores = exact_scores(z, d, qi[0], qt)
    what = "ranking n={}".format(n)
    for filt, kn in ((None, None), (lists, known)):
        greater, ties = dec.rank(z.float(), qi, qt, known=kn)
        mask = known_mask(qi[0], qt, n, keys_of(filt, n) if filt else torch.empty(0, dtype=torch.long, device=gpu))
        g_ref, t_ref = ref_rank(scores, qi[1], mask)
        assert torch.equal(greater.long()[:6], g_ref[:6]) and torch.equal(ties.long()[:6], t_ref[:6]), what + ": the TOP ids' queries"
        assert torch.equal(greater.long(), g_ref) and torch.equal(ties.long(), t_ref), what
    mask = known_mask(qi[0], qt, n, keys_of(lists, n))
    assert bool(mask[0, n - 1]) and bool(mask[1, n - 1]) and not bool(mask[4, n - 1]), what + ": the filter does not hold the top pairs"
    val, idx = dec.top_k(z.float(), qi[0], qt, 10, known=known)
    v_ref, i_ref = ref_topk(scores, mask, 10)
    assert torch.equal(idx[:6], i_ref[:6]) and torch.equal(val[:6].double(), v_ref[:6]), what + ": the TOP ids' queries (top-k)"
    assert torch.equal(idx, i_ref) and torch.equal(val.double(), v_ref), what
    assert i_ref[4, 0] == n - 1 and i_ref[5, 0] == n - 1 and i_ref[3, 0] == n - 2, what + ": nodes n - 1 / n - 2 are not the best partners"
    _hip.raise_if_index_errors(gpu)


# ---- GCN-style layers -------------------------------------------------------------------------------------------------------

def gcn_graph(n, e, gen):
    a = torch.randint(0, n, (2, e), generator=gen)
    a = a[:, a[0] != a[1]]
    return torch.cat([top_pairs(n), a, a.flip(0)], dim=1).contiguous()


def run_gcn_layer(dev, n, fin, fout, seed, e=120000):
    """One cached GCN layer, inference forward (with its ReLU) and training step, against the float64 oracle; returns the layer.
    The training step has no ReLU: among the million outputs of these sizes one pre-activation lies within fp32 rounding of
    zero (9.6e-8 at n = 65534), fp32 and float64 then disagree about its mask and the gradients differ by that output's whole
    term.  The masked backward is held elsewhere (test_gpu_reference_gradients.py); the ids are the subject here."""
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    ei = gcn_graph(n, e, gen)
    x = torch.randn(n, fin, generator=gen)
    x[n - 1], x[n - 2] = pattern(fin, 2.0, 0.05), -pattern(fin, 1.5, 0.04)
    proj = torch.randn(n, fout, generator=gen)
    proj[n - 1], proj[n - 2], proj[0] = 1.5, -1.25, 0.75
    conv = gripnet_amd.myGCN(fin, fout, cached=True)
    conv.bias.data.normal_()
    x64 = x.double().requires_grad_(True)
    w64, b64 = conv.weight.data.double().requires_grad_(True), conv.bias.data.double().requires_grad_(True)
    pre = orc.gcn_forward(x64, w64, b64, ei, None)
    (pre * proj.double()).sum().backward()
    pre, ref = pre.detach(), torch.relu(pre.detach())
    conv = conv.to(dev)
    what = "GCN layer n={} {}->{}".format(n, fin, fout)
    with torch.no_grad():
        y = conv(x.to(dev), ei.to(dev), None, _relu=True)
    top_rows_forward(y, ref, [n - 1, 0], what)
    close(y, ref, FWD, what)
    xg = x.to(dev).requires_grad_(True)
    yt = conv(xg, ei.to(dev), None)
    (yt * proj.to(dev)).sum().backward()
    close(yt, pre, FWD, what + " (training forward)")
    top_rows_gradient(xg.grad, x64.grad, [n - 1, n - 2, 0], what + " dx")
    gc.check_gradients({"x": xg.grad, "weight": conv.weight.grad, "bias": conv.bias.grad},
                       {"x": x64.grad, "weight": w64.grad, "bias": b64.grad}, GRAD_REL, what, row_rel=ROW_REL, row_abs=ROW_ABS)
    return conv, x.to(dev), what


def test_gcn_gather_at_the_lds_limit(gpu, monkeypatch):
    """The LDS-staged gather keeps a column group of the table, N rows and a zero row, in 160 KB: the last N that gets the
    encoding is found by bisecting plan builds (the N <= 65534 of gcn_blocked.hip, gn_graph_plan_build_blocked, lies behind it); it runs on the staged
    kernels, N + 1 on the wave-per-row ones."""
    monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    ring = torch.tensor([[0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 0]], device=gpu)
    last = last_admitted(64, 65536, lambda n: _hip.GraphPlan.gcn(ring, n).build_blocked(16) == 16, (16384, 65534),
                         "LDS-staged GCN gather")
    for n in (last, last + 1):
        conv, x, what = run_gcn_layer(gpu, n, 32, 16, seed=n)
        what += " (last admitted {})".format(last)
        plan = conv.cached_result
        out = torch.empty(n, 16, device=gpu)
        assert (plan.blocked_cols == 16) == (n == last), what
        assert plan.blocked_ok(x, conv.weight, conv.bias, out) == (n == last), what


@pytest.mark.parametrize("n", [65534, 65535, 65536])
def test_gcn_layer_at_the_16_bit_node_limit(gpu, n, monkeypatch):
    """Node counts around the 16-bit ids of the LDS-staged encoding (zero row = N): none of them gets it (the table does not
    fit), all three run on the wave-per-row kernels with one and the same answer about the fused contraction."""
    monkeypatch.setenv("GN_BLOCKED_ANY", "1")
    conv, x, what = run_gcn_layer(gpu, n, 32, 16, seed=n)
    plan = conv.cached_result
    assert plan.blocked_cols == 0 and not plan.blocked_ok(x, conv.weight, conv.bias, torch.empty(n, 16, device=gpu)), what
    assert plan.transform_ok(32, 16, x) == _hip.transform_fusable(32, 16, x), what


@pytest.mark.parametrize("rows", [65535, 65536])
def test_plain_sum_at_65536_rows(gpu, rows):
    """A plain sum over many short rows gathers a small table from LDS from 65536 rows on (gather_route.hpp, the lds_table rule of gather_route; row
    table_rows is its zero row).  The library has no query for it: both sizes are held to the float64 sums."""
    n_src, f = 2000, 16
    gen = torch.Generator().manual_seed(rows)
    ei = torch.stack([torch.randint(0, n_src, (150000,), generator=gen), torch.randint(0, rows, (150000,), generator=gen)])
    ei[:, :4] = torch.tensor([[n_src - 1, 0, n_src - 1, n_src - 2], [rows - 1, rows - 1, 0, rows - 1]])
    table = torch.randn(n_src, f, generator=gen)
    table[n_src - 1], table[n_src - 2] = pattern(f, 3.0, 0.1), -pattern(f, 2.0, 0.1)
    ref = torch.zeros(rows, f, dtype=torch.float64).index_add_(0, ei[1], table.double()[ei[0]])
    plan = _hip.GraphPlan.plain_sum(ei.to(gpu), n_src, rows)
    out = torch.full((rows, f), float("nan"), device=gpu)
    plan.aggregate(table.to(gpu), None, False, out)
    what = "plain sum over {} rows".format(rows)
    top_rows_forward(out, ref, [rows - 1, 0], what)
    close(out, ref, FWD, what)


@pytest.mark.parametrize("rows", [1 << 20, (1 << 20) + 1])
def test_short_row_gather_at_2_to_the_20_rows(gpu, rows):
    """The external layer's padded (ELL) rows are built for up to 2^20 targets (plan.hip:459); one more keeps the CSR kernels."""
    n_src, f = 300, 16
    gen = torch.Generator().manual_seed(rows & 0xffff)
    ei = torch.stack([torch.randint(0, n_src, (200000,), generator=gen), torch.randint(0, rows, (200000,), generator=gen)])
    ei[:, :4] = torch.tensor([[n_src - 1, 0, n_src - 1, n_src - 2], [rows - 1, rows - 1, 0, rows - 1]])
    x = torch.randn(n_src, f, generator=gen)
    x[n_src - 1], x[n_src - 2] = pattern(f, 3.0, 0.1), -pattern(f, 2.0, 0.1)
    bias = torch.randn(f, generator=gen)
    sd = {"p.conv.weight": torch.eye(f, dtype=torch.float64), "p.conv.bias": bias.double()}
    ref = orc.inter_forward_closed(sd, "p.", x.double(), ei, rows)
    plan = _hip.GraphPlan.bipartite(ei.to(gpu), n_src, rows)
    out = torch.full((rows, f), float("nan"), device=gpu)
    plan.aggregate(x.to(gpu), bias.to(gpu), False, out)
    what = "external layer's gather over {} targets".format(rows)
    top_rows_forward(out, ref, [rows - 1, 0], what)
    close(out, ref, FWD, what)


# ---- the relational layer ---------------------------------------------------------------------------------------------------

def relational_case(n, R, fin, fout, bases, seed, extra=6000):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    ei, et = typed_edges(n, R, extra, gen)
    rl = range_list_of(et, R)
    x = torch.randn(n, fin, generator=gen)
    x[n - 1], x[n - 2] = pattern(fin, 1.5, 0.05), -pattern(fin, 1.2, 0.04)
    rg = gripnet_amd.myRGCN(fin, fout, R, bases, False, bias=True)
    rg.bias.data.normal_()
    rg.att.data[R - 1] = pattern(bases, 0.9, 0.1)
    return rg, x, ei, rl


def relational_reference(rg, x, ei, rl, proj):
    """Output (no ReLU: see run_gcn_layer) and float64 leaves of the layer after backward of (output * proj).sum()."""
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in rg.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    ref = orc.rgcn_forward(x64, ei, rl, sd["basis"], sd["att"], sd["root"], sd["bias"])
    (ref * proj.double()).sum().backward()
    return ref.detach(), x64, sd


def run_relational_forward(dev, n, R, fin, fout, bases, seed, kernel, expect):
    """An inference forward with `kernel` asked for; `expect`: the kernel the path query must name."""
    rg, x, ei, rl = relational_case(n, R, fin, fout, bases, seed)
    sd = {k: v.detach().double() for k, v in rg.state_dict().items()}
    ref = orc.rgcn_forward(x.double(), ei, rl, sd["basis"], sd["att"], sd["root"], sd["bias"])      # (no ReLU: no top row left at zero)
    rg = rg.to(dev)
    rg.kernel = kernel
    with torch.no_grad():
        y = rg(x.to(dev), ei.to(dev), None, rl)
    what = "relational layer n={} R={} {}->{} bases={} kernel={}".format(n, R, fin, fout, bases, kernel)
    assert rg._plan.path(fin, fout, bases, rg._fast(), kernel) == expect, (what, rg._plan.path(fin, fout, bases, rg._fast(), kernel))
    top_rows_forward(y, ref, [n - 1, 0], what)
    close(y, ref, FWD, what)
    _hip.raise_if_index_errors(dev)


def relational_path_limit(dev, fin, fout, bases, R, kernel, lo, hi, sane, what):
    ring = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 0]], device=dev)
    rl = torch.tensor([[0, 8]] + [[8, 8]] * (R - 1))
    return last_admitted(lo, hi, lambda n: _hip.RgcnPlan(ring, rl, n).path(fin, fout, bases, path=kernel) == kernel, sane, what)


def test_relational_layer_at_the_destination_major_limit(gpu):
    """The destination-major kernel takes up to 768 nodes (24 chunks of 32 sources; fewer on a device with few compute units):
    the last size the path query names it for, and the next one on the LDS-accumulator kernel."""
    fin, fout, bases, R = 32, 32, 8, 6
    last = relational_path_limit(gpu, fin, fout, bases, R, "pair", 8, 4096, (256, 768), "destination-major relational kernel")
    run_relational_forward(gpu, last, R, fin, fout, bases, last, "auto", "pair")
    run_relational_forward(gpu, last + 1, R, fin, fout, bases, last + 1, "auto", "lds")


def test_relational_layer_at_the_lds_accumulator_limit(gpu):
    """The LDS-accumulator kernel keeps [N + tile, 32] floats in LDS (geometry(N).tiles > 0; N <= 32767 lies far behind that):
    the last N the forced path is taken for, and N + 1 on the general kernel."""
    fin, fout, bases, R = 16, 32, 4, 6
    last = relational_path_limit(gpu, fin, fout, bases, R, "lds", 8, 32769, (512, 32767), "LDS-accumulator relational kernel")
    run_relational_forward(gpu, last, R, fin, fout, bases, last, "lds", "lds")
    run_relational_forward(gpu, last + 1, R, fin, fout, bases, last + 1, "lds", "general")


@pytest.mark.parametrize("R", [32768, 32769])
def test_relational_table_path_relation_slabs(gpu, R):
    """The [R, N, out] table path computes H[r] = X W[r] in grid slabs of 32768 relations: one slab, and a second slab of one
    relation that holds the top pairs."""
    run_relational_forward(gpu, 6, R, 4, 4, 2, R, "table", "table")


def run_relational_step(dev, n, R, fin, fout, bases, seed):
    """A training step of the layer against float64 autograd through the oracle; returns the layer's plan."""
    rg, x, ei, rl = relational_case(n, R, fin, fout, bases, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    proj = torch.randn(n, fout, generator=gen)
    proj[n - 1], proj[n - 2], proj[0] = 1.5, -1.25, 0.75
    ref, x64, sd = relational_reference(rg, x, ei, rl, proj)
    rg = rg.to(dev)
    xg = x.to(dev).requires_grad_(True)

    def step():
        out = rg(xg, ei.to(dev), None, rl)
        (out * proj.to(dev)).sum().backward()
        return out
    y, names = served(step)
    what = "relational step n={} R={} {}->{} bases={}".format(n, R, fin, fout, bases)
    top_rows_forward(y, ref, [n - 1, 0], what)
    close(y, ref, FWD, what)
    got = {k: p.grad for k, p in rg.named_parameters()}
    got["x"] = xg.grad
    want = {k: v.grad for k, v in sd.items()}
    want["x"] = x64.grad
    top_rows_gradient(xg.grad, x64.grad, [n - 1, n - 2, 0], what + " dx")
    top_rows_gradient(rg.att.grad, sd["att"].grad, [R - 1, 0], what + " datt")
    gc.check_gradients(got, want, GRAD_REL, what, row_rel=ROW_REL, row_abs=ROW_ABS)
    _hip.raise_if_index_errors(dev)
    return rg._plan, names, what


@pytest.mark.parametrize("n", [65534, 65535, 65536])
def test_relational_layer_at_the_16_bit_node_limit(gpu, n):
    """65534 nodes: the fused weight gradient's plan exists (0xffff = "no source", id n = the zero row) but its table does not
    fit the LDS; from 65535 on there is no plan.  Every size runs the general forward and the O(E) weight gradient."""
    plan, names, what = run_relational_step(gpu, n, 5, 16, 16, 3, seed=n)
    wg = plan.weight_grad_plan()
    assert (wg is not None) == (n <= 65534), what
    assert wg is None or not wg.supported(16, 16), what
    assert plan.path(16, 16, 3) == "general", (what, plan.path(16, 16, 3))
    assert "gn_rgcn_weight_grad_f32" in names and "gn_rel_weight_grad_f32" not in names, (what, names)


def test_relational_weight_gradient_at_the_lds_limit(gpu):
    """The fused weight gradient keeps [n + 1, out] gradient rows in LDS: the last n its plan says `supported` for (bisected on
    plan builds), and the next one on the general weight gradient."""
    fin, fout, bases, R = 16, 16, 3, 5
    ring = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 0]], device=gpu)
    rl = torch.tensor([[0, 8]] + [[8, 8]] * (R - 1))

    def admitted(n):
        wg = _hip.RgcnPlan(ring, rl, n).weight_grad_plan()
        return wg is not None and wg.supported(fin, fout)
    last = last_admitted(8, 65535, admitted, (1024, 65534), "fused relational weight gradient")
    for n in (last, last + 1):
        plan, names, what = run_relational_step(gpu, n, R, fin, fout, bases, seed=n)
        wg = plan.weight_grad_plan()
        assert wg is not None and wg.supported(fin, fout) == (n == last), (what, last)
        assert ("gn_rel_weight_grad_f32" in names) == (n == last) and ("gn_rgcn_weight_grad_f32" in names) == (n != last), (what, last, names)


# ---- dense batch, Adam ------------------------------------------------------------------------------------------------------

def test_dense_batch_limit(gpu):
    """gn_gemm_f32 takes 65535 products in one call (the grid's third dimension) and refuses 65536 with Unsupported."""
    m, k, n, batch = 2, 4, 4, 65535
    gen = torch.Generator().manual_seed(4)
    a, b = torch.randn(batch + 1, m, k, generator=gen), torch.randn(batch + 1, k, n, generator=gen)
    a[batch - 1], b[batch - 1] = pattern(k, 2.0, 0.25).repeat(m, 1), pattern(n, -1.0, 0.5).repeat(k, 1)
    ag, bg = a.to(gpu), b.to(gpu)
    out = torch.full((batch + 1, m, n), float("nan"), device=gpu)

    def product(count):
        return _hip.gemm(ag.view(-1, k), bg.view(-1, n), out.view(-1, n), batch=count, stride_a=m * k, stride_b=k * n,
                         stride_c=m * n, m=m, n=n, k=k)
    product(batch)
    ref = torch.bmm(a.double(), b.double())
    close(out[:batch], ref[:batch], FWD, "65535 products")
    close(out[batch - 1], ref[batch - 1], FWD, "the LAST of 65535 products")
    assert float(ref[batch - 1].abs().max()) > 5.0 and torch.isnan(out[batch]).all()
    with pytest.raises(_hip.Unsupported):
        product(batch + 1)
    assert torch.isnan(out[batch]).all(), "a refused call wrote"


def adam_float64(params, grads_per_step, lr, b1, b2, eps):
    """torch/optim/adam.py's update in float64: per step (updates, exp_avg, exp_avg_sq) of every tensor."""
    p = [t.double().clone() for t in params]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    history = []
    for t, grads in enumerate(grads_per_step, start=1):
        upd = []
        for k, g in enumerate(grads):
            g = g.double()
            m[k] = m[k] + (g - m[k]) * (1 - b1)
            v[k] = b2 * v[k] + (1 - b2) * g * g
            step = lr / (1 - b1 ** t) * m[k] / (v[k].sqrt() / (1 - b2 ** t) ** 0.5 + eps)
            p[k] = p[k] - step
            upd.append(-step)
        history.append((upd, [t.clone() for t in m], [t.clone() for t in v]))
    return history


@pytest.mark.parametrize("count", [64, 65, 129])
def test_adam_tensor_counts_and_update(gpu, count):
    """64 tensors are one launch, 65 two and 129 three (only the last advances the step counter); one parameter is a view one
    element into its storage (the scalar path).  Held to float64 Adam on the UPDATE p_t - p_(t-1) and on both moments, not
    on the parameter (whose own rounding, 6e-8 |p|, hides a relative error of the step).

    Bar of the update: the distance of torch's fp32 torch.optim.Adam from float64 Adam on the same inputs, measured here, over
    all tensors of a magnitude class (parameters of order 1, where the parameter's rounding dominates, and of order 1e-3,
    where the step does); the HIP step may be twice as far.  Measured on an MI355X (64 tensors, steps 1 to 4, largest
    distance of a class): torch fp32 2.2e-7 .. 2.4e-7 (order 1) and 2.9e-9 .. 3.3e-9 (order 1e-3); HIP 2.2e-7 .. 2.4e-7 and
    2.7e-9 .. 3.4e-9.  Before ABI 159 (fp32 betas, bias corrections as 1 - __powf(b, t)) the HIP step of the 1e-3 class was
    3.6e-8 / 3.4e-8 / 3.0e-8 from float64 at steps 2 / 3 / 4 - twelve times torch's distance - and every second moment 1.3e-5
    off (1 - 0.999f).
    Bar of the moments: at most six fp32 roundings per step (v: beta2 and 1 - beta2 as fp32, three products, the sum; m: four),
    each <= 2^-24 of the larger of the old moment and the new term, over the steps taken:
    |m - m64| <= 6 t 2^-24 max(|m64|, |g|), the same with v and g^2."""
    lr, b1, b2, eps, steps = 0.01, 0.9, 0.999, 1e-8, 4
    gen = torch.Generator().manual_seed(count)
    shapes = [(5000, 7), (4097,), (33, 5), (1,), (3,), (640, 16)]
    sizes = [shapes[k % len(shapes)] for k in range(count)]
    small = [k % 2 == 1 for k in range(count)]                       # every other tensor of order 1e-3
    init = [torch.randn(s, generator=gen) * (1e-3 if sm else 1.0) for s, sm in zip(sizes, small)]
    grads = [[torch.randn(s, generator=gen) * (10.0 ** (t - 2)) for s in sizes] for t in range(steps)]
    store = torch.zeros(init[2].numel() + 1, device=gpu)
    ours = [torch.nn.Parameter(p.to(gpu)) for p in init]
    ours[2] = torch.nn.Parameter(store[1:].view(sizes[2]))           # storage offset of one element: 4 bytes past 16-byte alignment
    with torch.no_grad():
        ours[2].copy_(init[2].to(gpu))
    assert ours[2].data_ptr() % 16 == 4 and ours[2].is_contiguous()
    theirs = [torch.nn.Parameter(p.to(gpu)) for p in init]
    a = gripnet_amd.optim.Adam(ours, lr=lr, betas=(b1, b2), eps=eps)
    b = torch.optim.Adam(theirs, lr=lr, betas=(b1, b2), eps=eps)
    ref = adam_float64(init, grads, lr, b1, b2, eps)
    ulp = 2.0 ** -24
    for t in range(steps):
        before = [[p.detach().double().cpu() for p in group] for group in (ours, theirs)]
        for k in range(count):
            ours[k].grad, theirs[k].grad = grads[t][k].to(gpu), grads[t][k].to(gpu)
        (_, names), _ = served(a.step), b.step()
        assert names == ["gn_adam_step_f32"], names
        assert float(a.param_groups[0]["step"]) == t + 1.0, "the step counter moved {} times in step {}".format(
            float(a.param_groups[0]["step"]) - t, t + 1)
        upd64, m64, v64 = ref[t]
        for cls in (False, True):
            dist = {"hip": 0.0, "torch": 0.0}
            for k in range(count):
                if small[k] != cls:
                    continue
                for name, group, old in (("hip", ours, before[0]), ("torch", theirs, before[1])):
                    upd = group[k].detach().double().cpu() - old[k]
                    dist[name] = max(dist[name], float((upd - upd64[k]).abs().max()))
            print("Adam, {} tensors, step {}, parameters of order {}: update off float64 by {:.3e} (HIP), {:.3e} (torch fp32)".format(
                count, t + 1, "1e-3" if cls else "1", dist["hip"], dist["torch"]))
            assert dist["torch"] > 0.0
            assert dist["hip"] <= 2.0 * dist["torch"], (count, t + 1, cls, dist)
        for k in range(count):
            g = grads[t][k].double()
            for name, got, want, term in (("exp_avg", a.state[ours[k]]["exp_avg"], m64[k], g.abs()),
                                          ("exp_avg_sq", a.state[ours[k]]["exp_avg_sq"], v64[k], g * g)):
                err = (got.detach().double().cpu() - want).abs()
                bar = 6 * (t + 1) * ulp * torch.maximum(want.abs(), term)
                assert (err <= bar).all(), "{} of tensor {} at step {}: off by {:.3e} of its scale".format(
                    name, k, t + 1, float((err / torch.maximum(want.abs(), term).clamp_min(1e-300)).max()))
    _hip.raise_if_index_errors(gpu)
