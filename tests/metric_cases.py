"""Helpers of the link-metric tests (tests/test_gpu_link_metrics.py on the GPU, tests/test_metrics_host.py on the host): a
float64 reference of AUPRC / AUROC / AP written from the definitions, and score vectors built to reach one branch each of
gripnet_amd/csrc/metrics.hip.  Not a test module; uses no GPU.

The library has no path query for the metrics, so every builder ASSERTS the condition it is named after, in numpy on the
sorted arrays, with the kernels' geometry restated below: a case that no longer meets its condition fails instead of
passing for nothing.  `case(name)` and `reference(name)` are computed once and shared; nobody writes to what they return."""
import functools

import numpy as np
import torch

CHUNK = 4096        # keys a workgroup sorts in LDS (kChunk); a longer segment goes through merge rounds
TILE = 1024         # elements of a terms workgroup (kTile)
WINDOW = 4096       # keys of the other class a terms workgroup keeps in LDS (kWindow); a larger window is searched in global memory
SORT_WIDTHS = (256, 1024, 4096)   # the three sizes of the register sort: a chunk takes the smallest that holds it
TOL = 1e-9          # |library - reference| per metric and relation (the bar of test_relation_metrics_match_sklearn)


# ---- the reference ----------------------------------------------------------------------------------------------------
def ref_link_metrics(pos, neg):
    """(auprc, auroc, ap) of positive scores `pos` against negative scores `neg`, float64, from the definitions.

    The thresholds are the distinct values of pos U neg, compared as float64 values (-0.0 == +0.0), from the largest
    down.  At a threshold tp / fp count the positives / negatives at or above it; precision = tp / (tp + fp), recall =
    tp / P.  AP = sum (tp - tp0) / P * precision; AUPRC = the trapezoid of (recall, precision) from the start point
    (recall 0, precision 1); AUROC = the trapezoid of (fp / N, tp / P) from (0, 0).  Empty input gives NaN."""
    p = np.sort(np.asarray(pos, dtype=np.float64).ravel())
    n = np.sort(np.asarray(neg, dtype=np.float64).ravel())
    P, N = p.size, n.size
    if P == 0 or N == 0:
        return float("nan"), float("nan"), float("nan")
    thr = np.unique(np.concatenate([p, n]))[::-1]                  # np.unique compares values: one entry for both zeros
    tp = (P - np.searchsorted(p, thr, side="left")).astype(np.float64)
    fp = (N - np.searchsorted(n, thr, side="left")).astype(np.float64)
    tp0, fp0 = np.concatenate([[0.0], tp[:-1]]), np.concatenate([[0.0], fp[:-1]])
    prec = tp / (tp + fp)                                          # tp + fp >= 1: a threshold is somebody's score
    prec0 = np.concatenate([[1.0], prec[:-1]])
    ap = float(np.sum((tp - tp0) / P * prec))
    auprc = float(np.sum((tp - tp0) / P * (prec + prec0) * 0.5))
    auroc = float(np.sum((fp - fp0) * (tp + tp0))) / (2.0 * P * N)  # a sum of integers below 2^53: exact, rounded once
    return auprc, auroc, ap


def range_list(sizes):
    """[R, 2] int64 (start, end) rows of consecutive blocks of the given lengths."""
    end = np.cumsum(np.asarray(sizes, dtype=np.int64))
    return torch.from_numpy(np.stack([end - np.asarray(sizes, dtype=np.int64), end], axis=1))


def ref_relations(pos, neg, sizes):
    """[3, R] float64: `ref_link_metrics` of every block (the scores as the fp32 values the library compares)."""
    p, n = _np32(pos), _np32(neg)
    out = np.empty((3, len(sizes)), dtype=np.float64)
    for r, (s, e) in enumerate(range_list(sizes).tolist()):
        out[:, r] = ref_link_metrics(p[s:e], n[s:e])
    return out


def _np32(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float32).contiguous().numpy()


# ---- what the builders assert about their own output --------------------------------------------------------------------
def descending(x):
    return np.sort(np.asarray(x, dtype=np.float64))[::-1]


def chunk_lengths(n):
    """Lengths of the runs the chunk sort leaves of a segment of n keys."""
    return [min(CHUNK, n - o) for o in range(0, n, CHUNK)]


def sort_width(n):
    return next(w for w in SORT_WIDTHS if n <= w)


def merge_rounds(sizes):
    chunks = max([len(chunk_lengths(n)) for n in sizes] + [1])
    return int(np.ceil(np.log2(chunks)))


def tile_windows(own, oth):
    """For every tile of TILE consecutive keys of the sorted class `own`: how many scores of `oth` lie between the tile's
    first and last score, both included - the window of the other class the tile's searches run in."""
    o, a = descending(own), np.sort(np.asarray(oth, dtype=np.float64))
    out = []
    for t0 in range(0, o.size, TILE):
        first, last = o[t0], o[min(t0 + TILE, o.size) - 1]
        at_or_above_last = a.size - np.searchsorted(a, last, side="left")
        above_first = a.size - np.searchsorted(a, first, side="right")
        out.append(int(at_or_above_last - above_first))
    return out


def tie_groups(x):
    """(start, end) positions, end included, of every run of equal values in the sorted class."""
    o = descending(x)
    cut = np.flatnonzero(np.diff(o) != 0)
    starts, ends = np.concatenate([[0], cut + 1]), np.concatenate([cut, [o.size - 1]])
    return list(zip(starts.tolist(), ends.tolist()))


def has_both_zeros(*scores):
    """-0.0 and +0.0 both occur: what an order on the bit patterns ranks apart and an order on the values ties."""
    v = np.concatenate([_np32(t) for t in scores])
    return bool(((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _shuffled(values, gen):
    t = torch.as_tensor(np.ascontiguousarray(values), dtype=torch.float32)
    return t[torch.randperm(t.numel(), generator=gen)]


def _blocks(sizes):
    return [(int(s), int(e)) for s, e in range_list(sizes).tolist()]


# ---- score domain: outside (0, 1) -----------------------------------------------------------------------------------------
DOMAIN_SIZES = (300, 5000)


def logits():
    g, E = _gen(11), sum(DOMAIN_SIZES)
    pos, neg = 30.0 * torch.randn(E, generator=g) + 5.0, 30.0 * torch.randn(E, generator=g) - 5.0
    for s, e in _blocks(DOMAIN_SIZES):
        for v in (pos[s:e], neg[s:e]):
            assert v.min() < -30.0 and v.max() > 30.0, "logits on both sides of (0, 1)"
    return pos, neg, DOMAIN_SIZES


def relu_signed_zeros():
    """Positives relu(randn) against negatives -relu(randn): about half of either class is an exact zero, +0.0 among the
    positives and -0.0 among the negatives - one tied value in float64, and the only value the classes share."""
    g, E = _gen(12), sum(DOMAIN_SIZES)
    pos, neg = torch.relu(torch.randn(E, generator=g)), -torch.relu(torch.randn(E, generator=g))
    for s, e in _blocks(DOMAIN_SIZES):
        p, n = pos[s:e].numpy(), neg[s:e].numpy()
        assert ((p == 0) & ~np.signbit(p)).sum() > (e - s) // 4, "+0.0 among the positives"
        assert ((n == 0) & np.signbit(n)).sum() > (e - s) // 4, "-0.0 among the negatives"
        assert p.max() > 0 and n.min() < 0
    return pos, neg, DOMAIN_SIZES


def hand_signed_zero():
    """Positives [-0.0] against negatives [+0.0]: one tie, AUROC 0.5 (0 for an order that puts +0.0 above -0.0)."""
    pos, neg = torch.tensor([-0.0]), torch.tensor([0.0])
    assert np.signbit(pos.numpy()[0]) and not np.signbit(neg.numpy()[0]) and pos.numpy()[0] == neg.numpy()[0]
    assert ref_link_metrics(pos.numpy(), neg.numpy()) == (0.75, 0.5, 0.5)
    return pos, neg, (1,)


def zeros_of_both_signs_in_each_class():
    """-1, -0.0, +0.0 and 1 in either class: the two zeros are one group of ties inside a class as well as between them."""
    g, n = _gen(15), 300
    table = torch.tensor([-1.0, -0.0, 0.0, 1.0])
    pos, neg = table[torch.randint(0, 4, (n,), generator=g)], table[torch.randint(0, 4, (n,), generator=g)]
    for v in (pos.numpy(), neg.numpy()):
        assert ((v == 0) & np.signbit(v)).sum() > 30 and ((v == 0) & ~np.signbit(v)).sum() > 30
        assert [b - a + 1 for a, b in tie_groups(v)][1] == (v == 0).sum()
    return pos, neg, (n,)


def denormals_next_to_huge():
    """k 2^-149 for k in [-3, 3] next to +-3e38: seven values that differ, the four smallest magnitudes fp32 has.  An order
    that flushes denormals ties all seven; the builder asserts that the reference tells the two apart."""
    g, E = _gen(13), sum(DOMAIN_SIZES)

    def draw(shift):
        k = torch.randint(-3, 4, (E,), generator=g).double()
        k = torch.clamp(k + (torch.rand(E, generator=g) < 0.3).double() * shift, -3, 3)      # the classes lean apart by one step
        v = (k * 2.0 ** -149).float()
        huge = torch.rand(E, generator=g)
        v[huge < 0.05] = 3e38
        v[huge > 0.95] = -3e38
        return v

    pos, neg = draw(1.0), draw(-1.0)
    tiny = np.float32(2.0 ** -126)
    for s, e in _blocks(DOMAIN_SIZES):
        for v in (pos[s:e].numpy(), neg[s:e].numpy()):
            small = v[np.abs(v) < tiny]
            assert np.unique(small).size == 7 and np.unique(small.view(np.uint32) & np.uint32(0x7fffffff)).size == 4, "denormals k 2^-149"
            assert v.max() == np.float32(3e38) and v.min() == np.float32(-3e38)
        flush = lambda v: np.where(np.abs(v) < tiny, np.float32(0), v)
        kept = ref_link_metrics(pos[s:e].numpy(), neg[s:e].numpy())
        flushed = ref_link_metrics(flush(pos[s:e].numpy()), flush(neg[s:e].numpy()))
        assert min(abs(a - b) for a, b in zip(kept, flushed)) > 1e3 * TOL, "flushing the denormals must show in every metric"
    return pos, neg, DOMAIN_SIZES


def one_ulp_apart():
    """The seven fp32 values within three ulps of 1.0 and the seven around -1.0: neighbours differ in the last bit only."""
    g, E = _gen(14), sum(DOMAIN_SIZES)
    centres = np.array([1.0, -1.0], dtype=np.float32).view(np.int32)

    def draw(lean):
        j = torch.randint(-3, 4, (E,), generator=g) + (torch.rand(E, generator=g) < 0.3).long() * lean
        j = torch.clamp(j, -3, 3).numpy().astype(np.int32)
        side = torch.randint(0, 2, (E,), generator=g).numpy()
        j = np.where(side == 1, -j, j)              # pattern + j is a larger MAGNITUDE: negated at -1.0, so that the lean points up in value there too
        return torch.from_numpy((centres[side] + j).view(np.float32).copy())

    pos, neg = draw(1), draw(-1)
    for s, e in _blocks(DOMAIN_SIZES):
        for v in (pos[s:e].numpy(), neg[s:e].numpy()):
            bits = np.unique(v.view(np.int32))
            assert bits.size == 14 and np.all(np.diff(bits)[np.diff(bits) < 100] == 1), "14 values, neighbours one ulp apart"
            assert np.unique(v.astype(np.float64)).size == 14
    return pos, neg, DOMAIN_SIZES


# ---- sort sizes -------------------------------------------------------------------------------------------------------
SORT_SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4097, 8193, 12289)


def _assert_sort_sizes():
    runs = {n: chunk_lengths(n) for n in SORT_SIZES}
    widths = {n: sort_width(r[0]) for n, r in runs.items() if len(r) == 1}
    assert widths[256] == 256 and widths[257] == 1024 and widths[1024] == 1024 and widths[1025] == 4096 and widths[4095] == 4096
    assert runs[4097] == [4096, 1] and runs[8193] == [4096, 4096, 1] and runs[12289] == [4096] * 3 + [1]
    # 8193: round 1 merges (4096, 4096) and leaves the run of 1 alone, round 2 merges 8192 with 1;
    # 12289: round 1 leaves (8192, 4097), round 2 merges them - runs of 3 full chunks plus 1 key in the last pair
    assert merge_rounds(SORT_SIZES) == 2 and merge_rounds([4097]) == 1


def sort_sizes_random():
    _assert_sort_sizes()
    g, E = _gen(21), sum(SORT_SIZES)
    pos, neg = torch.randn(E, generator=g) + 0.5, torch.randn(E, generator=g)
    for s, e in _blocks(SORT_SIZES):
        if e - s >= 255:
            assert np.unique(pos[s:e].numpy()).size > 0.99 * (e - s), "(nearly) no ties"
    return pos, neg, SORT_SIZES


def sort_sizes_eighths():
    """The same scores rounded to 1/8: some sixty distinct values, so ties cross every chunk, run and tile boundary.
    Rounding leaves the sign: scores in (-1/16, 0) become -0.0, those in [0, 1/16) +0.0 - zeros of both signs in one group."""
    pos, neg, sizes = sort_sizes_random()
    pos, neg = torch.round(pos * 8) / 8, torch.round(neg * 8) / 8
    assert has_both_zeros(pos) and has_both_zeros(neg)
    s, e = _blocks(sizes)[-1]
    assert np.unique(np.concatenate([pos[s:e].numpy(), neg[s:e].numpy()])).size < 100
    assert max(b - a + 1 for a, b in tie_groups(pos[s:e].numpy())) > 300
    return pos, neg, sizes


# ---- windows of the other class -----------------------------------------------------------------------------------------
N_WINDOW = 5000


def window_other_class_tied():
    """Relation 0: every negative is 0.5, inside the positives' range - the positives' tile that holds 0.5 brackets all
    5000 negatives (> WINDOW: the global-memory search), the negatives' tiles bracket no positive at all.  Relation 1:
    the classes swapped, so both branches of the terms run on a global window."""
    g, n = _gen(31), N_WINDOW
    spread = lambda: (torch.randperm(2 * n, generator=g)[:n].float() + 0.25) / (2 * n)     # distinct, in (0, 1), never 0.5
    tied = torch.full((n,), 0.5)
    pos, neg = torch.cat([spread(), tied]), torch.cat([tied, spread()])
    for (s, e), (own, oth) in zip(_blocks((n, n)), ((pos, neg), (neg, pos))):
        own, oth = own[s:e].numpy(), oth[s:e].numpy()
        assert own.min() < 0.5 < own.max() and not (own == 0.5).any()
        w = tile_windows(own, oth)
        assert max(w) == n > WINDOW and sorted(w)[:-1] == [0] * (len(w) - 1), w
        assert tile_windows(oth, own) == [0] * len(w)
    return pos, neg, (n, n)


def _window_of(count):
    """Positives 5000, 4999, .. 1: their tile 1 runs from 3976 down to 2953.  `count` negatives lie in [2953, 3976], one on
    either end, the others above and below."""
    g, n = _gen(32 + count), N_WINDOW
    pos = np.arange(n, 0, -1, dtype=np.float64)
    first, last = pos[TILE], pos[2 * TILE - 1]
    inside = last + (first - last) * torch.rand(count - 2, generator=g).double().numpy()
    above = first + 0.5 + (n - first - 0.5) * torch.rand(400, generator=g).double().numpy()
    below = (last - 0.5) * torch.rand(n - count - 400, generator=g).double().numpy()
    neg = np.concatenate([inside, [first, last], above, below])
    pos, neg = _shuffled(pos, g), _shuffled(neg, g)
    w = tile_windows(pos.numpy(), neg.numpy())
    assert w[1] == count == max(w), w
    assert max(tile_windows(neg.numpy(), pos.numpy())) <= WINDOW
    return pos, neg, (n,)


def window_exactly_4096():
    pos, neg, sizes = _window_of(WINDOW)
    assert max(tile_windows(pos.numpy(), neg.numpy())) == WINDOW             # the last size that stays in LDS
    return pos, neg, sizes


def window_exactly_4097():
    pos, neg, sizes = _window_of(WINDOW + 1)
    assert max(tile_windows(pos.numpy(), neg.numpy())) == WINDOW + 1         # the first size searched in global memory
    return pos, neg, sizes


def separated_classes():
    """Relation 0: every positive above every negative; relation 1: the reverse.  Every window is empty, AUROC is 1 and 0."""
    g, n = _gen(34), N_WINDOW
    hi, lo = 1.0 + torch.rand(2 * n, generator=g), -1.0 - torch.rand(2 * n, generator=g)
    pos, neg = torch.cat([hi[:n], lo[:n]]), torch.cat([lo[n:], hi[n:]])
    for s, e in _blocks((n, n)):
        assert tile_windows(pos[s:e].numpy(), neg[s:e].numpy()) == [0] * 5 == tile_windows(neg[s:e].numpy(), pos[s:e].numpy())
    assert pos[:n].min() > neg[:n].max() and pos[n:].max() < neg[n:].min()
    ref = ref_relations(pos, neg, (n, n))
    assert ref[1, 0] == 1.0 and ref[1, 1] == 0.0
    return pos, neg, (n, n)


# ---- tie groups against tiles -------------------------------------------------------------------------------------------
N_TIES = 3000


def _with_groups(n, groups, gen):
    """n scores, distinct multiples of 1/8 except that the sorted positions a..b of every (a, b) in `groups` share one."""
    v = np.sort(torch.randperm(3 * n, generator=gen)[:n].numpy())[::-1].astype(np.float64) / 8
    for a, b in groups:
        v[a:b + 1] = v[a]
    got = [g for g in tie_groups(v) if g[1] > g[0]]
    assert got == sorted(groups), (got, groups)
    return _shuffled(v, gen)


def tie_groups_across_tiles():
    """Relation 0: a group of 1500 that starts in tile 0 and ends in tile 1 (positives) and one that starts in tile 0, covers
    tile 1 and ends in tile 2 (negatives).  Relation 1: groups whose last element is the first key of a tile.  Relation 2:
    groups that end on a tile's last key.  The first two kinds begin in front of the tile that accounts for them."""
    g, n = _gen(41), N_TIES
    plan = [([(300, 1799)], [(700, 2199)]),
            ([(2040, 2048)], [(1020, 1024), (2047, 2048)]),
            ([(1000, 1023)], [(2000, 2047), (5, 1023)])]
    pos = torch.cat([_with_groups(n, p, g) for p, _ in plan])
    neg = torch.cat([_with_groups(n, q, g) for _, q in plan])
    (s0, e0), (s1, e1), (s2, e2) = _blocks((n, n, n))
    long = [b for b in tie_groups(pos[s0:e0].numpy()) if b[1] - b[0] + 1 == 1500]
    assert long and long[0][0] // TILE == 0 and long[0][1] // TILE == 1
    assert any(a // TILE == 0 and b // TILE == 2 for a, b in tie_groups(neg[s0:e0].numpy()))
    for v in (pos[s1:e1], neg[s1:e1]):
        assert any(b > a and b % TILE == 0 for a, b in tie_groups(v.numpy())), "a group whose last element opens a tile"
    for v in (pos[s2:e2], neg[s2:e2]):
        assert any(b > a and b % TILE == TILE - 1 for a, b in tie_groups(v.numpy())), "a group that ends on a tile's last key"
    shared = np.intersect1d(pos[s0:e0].numpy(), neg[s0:e0].numpy()).size
    assert shared > 100, "ties between the classes as well"
    return pos, neg, (n, n, n)


# ---- many relations -------------------------------------------------------------------------------------------------------
MANY_R = 1500
MANY_LENGTHS = (0, 0, 1, 2, 3, 5, 64, 65, 300)
MANY_SEED = 9       # the first seed whose draw meets the conditions the builder asserts


def _many_sizes(seed):
    # 300 is drawn at 3 %, the others alike: some 40 k scores in all
    w = np.array([1.0] * 8 + [0.0]) * (0.97 / 8) + np.array([0.0] * 8 + [0.03])
    return np.random.RandomState(seed).choice(np.array(MANY_LENGTHS), size=MANY_R, p=w)


def _many_ok(sizes):
    empty = "".join("0" if s == 0 else "x" for s in sizes)
    return sizes[0] == 0 and sizes[-1] == 0 and "000" in empty and set(sizes.tolist()) == set(MANY_LENGTHS) and sizes.sum() <= 42000


def many_relations():
    sizes = _many_sizes(MANY_SEED)
    assert _many_ok(sizes), "first and last relation empty, three empty ones in a row, every length drawn"
    g, E = _gen(51), int(sizes.sum())
    pos, neg = torch.randn(E, generator=g) + 0.5, torch.randn(E, generator=g)
    pos, neg = torch.round(pos * 16) / 16, torch.round(neg * 16) / 16      # (ties, and zeros of both signs: see sort_sizes_eighths)
    assert has_both_zeros(pos) and has_both_zeros(neg)
    return pos, neg, tuple(int(s) for s in sizes)


def no_edges():
    return torch.empty(0), torch.empty(0), (0, 0, 0)


CASES = {f.__name__: f for f in (
    logits, relu_signed_zeros, hand_signed_zero, zeros_of_both_signs_in_each_class, denormals_next_to_huge, one_ulp_apart,
    sort_sizes_random, sort_sizes_eighths,
    window_other_class_tied, window_exactly_4096, window_exactly_4097, separated_classes,
    tie_groups_across_tiles, many_relations, no_edges)}
# the cases with zeros of both signs: what an order on the bit patterns gets wrong (test_metrics_host.py holds the list to the cases)
SIGNED_ZERO_CASES = ("relu_signed_zeros", "hand_signed_zero", "zeros_of_both_signs_in_each_class", "sort_sizes_eighths", "many_relations")


@functools.lru_cache(maxsize=None)
def case(name):
    """(pos, neg, sizes) of a builder, its own assertions run: fp32 CPU tensors, shared - do not write to them."""
    pos, neg, sizes = CASES[name]()
    assert pos.dtype == neg.dtype == torch.float32 and pos.shape == neg.shape == (sum(sizes),)
    assert torch.isfinite(pos).all() and torch.isfinite(neg).all()
    return pos, neg, tuple(sizes)


@functools.lru_cache(maxsize=None)
def reference(name):
    out = ref_relations(*case(name))
    out.setflags(write=False)
    return out


def distance(got, ref):
    """Largest |got - ref| over [3, R]; NaN must stand exactly where the reference has it."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN for the relations without edges, and for no other"
    live = ~np.isnan(ref)
    return float(np.abs(got - ref)[live].max()) if live.any() else 0.0
