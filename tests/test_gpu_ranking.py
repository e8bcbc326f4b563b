"""Filtered ranking and top-k retrieval of the DistMult decoder (gn_distmult_rank_f32 / gn_distmult_topk_f32) against torch
references: exact on integer models, within a per-query error bound on fp32 models at pose0-syn and make_rgcn_pose scale."""
import pytest
import torch

from gripnet_amd import _hip, utils
from gripnet_amd.decoder import KnownPairs, multiRelaInnerProductDecoder
from gripnet_amd.synth import add_pose_test_split, make_pose, make_rgcn_pose

pytestmark = pytest.mark.gpu


# ---- torch references ---------------------------------------------------------------------------------------------------

def known_mask(u, r, n, known_keys):
    """[Q, n] bool: (r, u, v) is a known pair; known_keys: sorted int64 (r * n + u) * n + v."""
    keys = ((r * n + u) * n).unsqueeze(1) + torch.arange(n, device=u.device).unsqueeze(0)
    if known_keys.numel() == 0:
        return torch.zeros_like(keys, dtype=torch.bool)
    pos = torch.searchsorted(known_keys, keys).clamp_(max=known_keys.numel() - 1)
    return known_keys[pos] == keys


def keys_of(lists, n):
    ks = [(et * n + ei[0]) * n + ei[1] for ei, et in lists]
    return torch.sort(torch.cat(ks)).values


def exact_scores(z, d, u, r):
    """int64 [Q, n] logits of an integer model (float64 products of small integers are exact)."""
    return ((z[u] * d[r]).double() @ z.T.double()).round().long()


def ref_rank(scores, v, mask):
    n = scores.shape[1]
    cand = ~mask & (torch.arange(n, device=scores.device).unsqueeze(0) != v.unsqueeze(1))
    st = scores.gather(1, v.unsqueeze(1))
    return ((scores > st) & cand).sum(1), ((scores == st) & cand).sum(1)


def ref_topk(scores, mask, k):
    s = scores.to(torch.float64)
    s = s.masked_fill(mask | torch.isnan(s), float("-inf"))            # a NaN score never enters (nor does -inf: padding)
    val, idx = torch.sort(s, dim=1, descending=True, stable=True)      # stable: equal scores keep ascending ids
    val, idx = val[:, :k], idx[:, :k]
    if val.shape[1] < k:
        pad = k - val.shape[1]
        val = torch.cat([val, torch.full((val.shape[0], pad), float("-inf"), dtype=val.dtype, device=val.device)], 1)
        idx = torch.cat([idx, torch.full((idx.shape[0], pad), -1, dtype=idx.dtype, device=idx.device)], 1)
    idx = torch.where(torch.isneginf(val), torch.full_like(idx, -1), idx)     # (a +inf entry keeps its id)
    return val, idx


def integer_model(n, f, R, seed, dev):
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-3, 4, (n, f), generator=g)
    d = torch.randint(-2, 3, (R, f), generator=g)
    z[7 % n] = z[3 % n]                                     # equal rows: engineered ties for every query
    z[(n - 1)] = z[5 % n]
    return z.to(dev), d.to(dev)


def decoder_with(d, dev):
    R, f = d.shape
    dec = multiRelaInnerProductDecoder(f, R).to(dev)
    with torch.no_grad():
        dec.weight.copy_(d.to(torch.float32))
    return dec


def integer_case(n, f, seed, dev):
    R = 5
    z, d = integer_model(n, f, R, seed, dev)
    g = torch.Generator().manual_seed(seed + 1)
    e_known = 6 * n
    ki = torch.randint(0, n, (2, e_known), generator=g)
    kt = torch.randint(0, R - 1, (e_known,), generator=g)          # relation R - 1 has no known pairs
    ki = torch.cat([ki, ki[:, :50]], 1)                             # duplicates
    kt = torch.cat([kt, kt[:50]])
    q = 300
    qi = torch.randint(0, n, (2, q), generator=g)
    qt = torch.randint(0, R, (q,), generator=g)
    qi[:, :40], qt[:40] = ki[:, 10:50], kt[10:50]                   # true pairs that are in the filter
    qi[1, 40:60] = 3                                                # true partner 3: partner 7 has the same row (a tie)
    lists = [(ki.to(dev), kt.to(dev)), (qi.to(dev), qt.to(dev))]
    return z, d, lists, qi.to(dev), qt.to(dev)


# ---- 1, 2: exact integer cases -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [37, 645, 1000])
@pytest.mark.parametrize("f", [8, 50, 80])
def test_rank_exact_integer_model(gpu, n, f):
    z, d, lists, qi, qt = integer_case(n, f, 100 + n + f, gpu)
    dec = decoder_with(d, gpu)
    zf = z.to(torch.float32)
    for filt in (None, lists, lists[:1]):
        known = KnownPairs(filt, n, d.shape[0]) if filt is not None else None
        greater, ties = dec.rank(zf, qi, qt, known=known)
        assert greater.dtype == torch.int32 and ties.dtype == torch.int32
        kk = keys_of(filt, n) if filt is not None else torch.empty(0, dtype=torch.long, device=gpu)
        scores = exact_scores(z, d, qi[0], qt)
        mask = known_mask(qi[0], qt, n, kk)
        g_ref, t_ref = ref_rank(scores, qi[1], mask)
        assert torch.equal(greater.long(), g_ref) and torch.equal(ties.long(), t_ref)
        assert int(ties.sum()) > 0                          # the engineered ties are there
    _hip.raise_if_index_errors(gpu)


@pytest.mark.parametrize("n", [37, 645, 1000])
@pytest.mark.parametrize("f", [8, 50, 80])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_top_k_exact_integer_model(gpu, n, f, k):
    z, d, lists, qi, qt = integer_case(n, f, 200 + n + f, gpu)
    dec = decoder_with(d, gpu)
    known = KnownPairs(lists, n, d.shape[0])
    scores, ids = dec.top_k(z.to(torch.float32), qi[0], qt, k, known=known)
    assert scores.shape == (qi.shape[1], k) and scores.dtype == torch.float32 and ids.dtype == torch.int64
    ref = exact_scores(z, d, qi[0], qt)
    mask = known_mask(qi[0], qt, n, keys_of(lists, n))
    val, idx = ref_topk(ref, mask, k)
    assert torch.equal(ids, idx)
    assert torch.equal(scores.to(torch.float64), val)
    _hip.raise_if_index_errors(gpu)


def test_top_k_pads_when_the_filter_leaves_fewer_than_k(gpu):
    n, f, R = 37, 8, 2
    z, d = integer_model(n, f, R, 5, gpu)
    dec = decoder_with(d, gpu)
    # query (u = 4, r = 0): every partner but 0, 11 and 36 is known -> 3 candidates; (u = 9, r = 1): nothing known
    keep = torch.tensor([v for v in range(n) if v not in (0, 11, 36)], device=gpu)
    ki = torch.stack([torch.full_like(keep, 4), keep])
    known = KnownPairs((ki, torch.zeros_like(keep)), n, R)
    nodes = torch.tensor([4, 9], device=gpu)
    rel = torch.tensor([0, 1], device=gpu)
    scores, ids = dec.top_k(z.to(torch.float32), nodes, rel, 8, known=known)
    assert sorted(ids[0, :3].tolist()) == [0, 11, 36]
    assert ids[0, 3:].tolist() == [-1] * 5 and torch.isneginf(scores[0, 3:]).all()
    assert (ids[1] >= 0).all() and torch.isfinite(scores[1]).all()
    ref = exact_scores(z, d, nodes, rel)
    val, idx = ref_topk(ref, known_mask(nodes, rel, n, keys_of([(ki, torch.zeros_like(keep))], n)), 8)
    assert torch.equal(ids, idx) and torch.equal(scores.to(torch.float64), val)


# ---- 3: the true score is the scan's value ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,f", [(50, 50), (64, 80), (17, 8)])
def test_rank_agrees_with_top_k_bits(gpu, n, f):
    g = torch.Generator().manual_seed(n + f)
    R = 4
    z = torch.randn(n, f, generator=g).to(gpu)
    dec = multiRelaInnerProductDecoder(f, R).to(gpu)
    q = 500
    qi = torch.randint(0, n, (2, q), generator=g).to(gpu)
    qt = torch.randint(0, R, (q,), generator=g).to(gpu)
    greater, ties = dec.rank(z, qi, qt)
    scores, ids = dec.top_k(z, qi[0], qt, n)
    assert (ids >= 0).all()
    s_true = scores.gather(1, torch.argsort(ids, dim=1)).gather(1, qi[1].unsqueeze(1))     # score of column v_true
    other = ids != qi[1].unsqueeze(1)
    assert torch.equal(greater.long(), ((scores > s_true) & other).sum(1))
    assert torch.equal(ties.long(), ((scores == s_true) & other).sum(1))


# ---- 4, 5: fp32 models at scale, bounded checks --------------------------------------------------------------------------

def check_bounded(dec, z, qi, qt, known_keys, n, greater, ties, chunk=4096, rel=4e-6):
    z64, d64 = z.double(), dec.weight.detach().double()
    for a in range(0, qi.shape[1], chunk):
        u, v, r = qi[0, a:a + chunk], qi[1, a:a + chunk], qt[a:a + chunk]
        a_rows = z64[u] * d64[r]
        s = a_rows @ z64.T
        tol = rel * (a_rows.abs() @ z64.abs().T).max(dim=1, keepdim=True).values + 1e-30
        mask = known_mask(u, r, n, known_keys) | (torch.arange(n, device=z.device).unsqueeze(0) == v.unsqueeze(1))
        st = s.gather(1, v.unsqueeze(1))
        g_lo = ((s > st + tol) & ~mask).sum(1)
        g_hi = ((s >= st - tol) & ~mask).sum(1)
        g, t = greater[a:a + chunk].long(), ties[a:a + chunk].long()
        assert (g >= 0).all() and (t >= 0).all()
        assert (g_lo <= g).all(), int((g_lo - g).max())
        assert (g + t <= g_hi).all(), int((g + t - g_hi).max())


def check_top_k_bounded(dec, z, nodes, rel_t, known_keys, n, scores, ids, rel=4e-6):
    z64, d64 = z.double(), dec.weight.detach().double()
    a_rows = z64[nodes] * d64[rel_t]
    s = a_rows @ z64.T
    tol = rel * (a_rows.abs() @ z64.abs().T).max(dim=1, keepdim=True).values + 1e-30
    mask = known_mask(nodes, rel_t, n, known_keys)
    k = ids.shape[1]
    assert (ids >= 0).all() and not mask.gather(1, ids).any()
    assert all(len(set(row)) == k for row in ids.tolist())
    assert ((s.gather(1, ids) - scores.double()).abs() <= tol).all()
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    outside = s.masked_fill(mask, float("-inf")).scatter(1, ids, float("-inf"))
    assert (outside.max(dim=1, keepdim=True).values <= scores[:, -1:].double() + 2 * tol).all()


def test_pose0_full_size(gpu):
    data = add_pose_test_split(make_pose("pose0-syn")).to(gpu)
    n, R, f = int(data.n_d_node), int(data.n_dd_edge_type), 80
    torch.manual_seed(0)
    z = torch.randn(n, f, device=gpu)
    dec = multiRelaInnerProductDecoder(f, R).to(gpu)
    lists = [(data.train_idx, data.train_et), (data.test_idx, data.test_et)]
    known = KnownPairs(lists, n, R)
    greater, ties = dec.rank(z, data.test_idx, data.test_et, known=known)
    assert greater.shape == (data.test_idx.shape[1],)
    check_bounded(dec, z, data.test_idx, data.test_et, keys_of(lists, n), n, greater, ties)
    m = utils.ranking_metrics(greater, ties, data.test_et, R)
    assert 0 < m["mrr_all"].item() <= 1
    # top-10 of a spread of (u, r) rows
    g = torch.Generator().manual_seed(1)
    nodes = torch.randint(0, n, (2000,), generator=g).to(gpu)
    rel_t = torch.randint(0, R, (2000,), generator=g).to(gpu)
    scores, ids = dec.top_k(z, nodes, rel_t, 10, known=known)
    check_top_k_bounded(dec, z, nodes, rel_t, keys_of(lists, n), n, scores, ids)


def test_large_n_rgcn_pose(gpu):
    data = make_rgcn_pose("pose0-syn")
    n, R, f = int(data.n_node), int(data.n_edge_type), 32
    ei, et = data.train_idx.to(gpu), data.train_et.to(gpu)
    e = ei.shape[1]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info(gpu)[0]
    known = KnownPairs((ei, et), n, R)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    kept = free0 - torch.cuda.mem_get_info(gpu)[0]
    assert kept <= 4 * (R * n + 1) + 4 * e + (64 << 20), kept            # O(E + R n); an R n^2 bitmap would be 47 GB
    torch.manual_seed(2)
    z = torch.randn(n, f, device=gpu)
    dec = multiRelaInnerProductDecoder(f, R).to(gpu)
    g = torch.Generator().manual_seed(3)
    pick = torch.randint(0, e, (3000,), generator=g).to(gpu)
    qi, qt = ei[:, pick], et[pick]
    greater, ties = dec.rank(z, qi, qt, known=known)
    check_bounded(dec, z, qi, qt, keys_of([(ei, et)], n), n, greater, ties, chunk=500)
    scores, ids = dec.top_k(z, qi[0, :300], qt[:300], 10, known=known)
    check_top_k_bounded(dec, z, qi[0, :300], qt[:300], keys_of([(ei, et)], n), n, scores, ids)
    _hip.raise_if_index_errors(gpu)


# ---- 6: capture ------------------------------------------------------------------------------------------------------------

def test_rank_and_top_k_capture(gpu):
    z, d, lists, qi, qt = integer_case(645, 80, 7, gpu)
    dec = decoder_with(d, gpu)
    zf = z.to(torch.float32)
    known = KnownPairs(lists, 645, d.shape[0])
    g0, t0 = dec.rank(zf, qi, qt, known=known)
    s0, i0 = dec.top_k(zf, qi[0], qt, 10, known=known)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dec.rank(zf, qi, qt, known=known)
        dec.top_k(zf, qi[0], qt, 10, known=known)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g1, t1 = dec.rank(zf, qi, qt, known=known)
        s1, i1 = dec.top_k(zf, qi[0], qt, 10, known=known)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g0, g1) and torch.equal(t0, t1)
        assert torch.equal(s0, s1) and torch.equal(i0, i1)


# ---- 7: errors -------------------------------------------------------------------------------------------------------------

def test_out_of_range_ids_raise_at_the_check(gpu):
    z, d, lists, qi, qt = integer_case(37, 8, 9, gpu)
    dec = decoder_with(d, gpu)
    zf = z.to(torch.float32)
    _hip.raise_if_index_errors(gpu)
    bad_i, bad_t = qi.clone(), qt.clone()
    bad_i[1, 3] = 37
    bad_t[5] = 5
    greater, ties = dec.rank(zf, bad_i, bad_t)
    assert greater[3].item() == -1 and ties[3].item() == -1 and greater[5].item() == -1
    assert (greater[:3] >= 0).all()
    with pytest.raises(IndexError):
        utils.ranking_metrics(greater, ties, bad_t.clamp(max=4), 5)
    greater, ties = dec.rank(zf, qi, qt)                   # the next call is clean
    utils.ranking_metrics(greater, ties, qt, 5)
    bad_n = qi[0].clone()
    bad_n[2] = -1
    scores, ids = dec.top_k(zf, bad_n, qt, 4)
    assert (ids[2] == -1).all() and torch.isnan(scores[2]).all() and (ids[0] >= 0).all()
    with pytest.raises(IndexError):
        _hip.raise_if_index_errors(gpu)
    _hip.raise_if_index_errors(gpu)
    with pytest.raises(IndexError):
        KnownPairs((qi, bad_t), 37, 5)


def test_bad_width_k_and_filter(gpu):
    dec = multiRelaInnerProductDecoder(8, 3).to(gpu)
    ei = torch.zeros(2, 4, dtype=torch.long, device=gpu)
    et = torch.zeros(4, dtype=torch.long, device=gpu)
    with pytest.raises(ValueError):
        dec.rank(torch.zeros(5, 9, device=gpu), ei, et)
    with pytest.raises(ValueError):
        dec.top_k(torch.zeros(5, 9, device=gpu), ei[0], et, 3)
    for k in (0, 65):
        with pytest.raises(ValueError):
            dec.top_k(torch.zeros(5, 8, device=gpu), ei[0], et, k)
    known = KnownPairs((ei, et), 6, 3)                      # built for 6 nodes
    with pytest.raises(ValueError):
        dec.rank(torch.zeros(5, 8, device=gpu), ei, et, known=known)
