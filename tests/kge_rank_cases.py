"""Float64 references, cases and error measures of the KGE ranking tests (KGEModel.rank / .top_k, csrc/kge_rank.hip):
tests/test_kge_ranking_host.py and tests/test_gpu_kge_ranking.py.  Not a test module.

The reference scores are kge_cases.raw_score (pinned to the reference's own runs by tests/test_kge_host.py) over the Q * n
candidate triples of a case: every candidate entity in the tail's place (side "tail") or the head's place (side "head") of
each query.  The filter is a sorted key list; for the head side it is built from the FLIPPED lists, as the KnownPairs is."""
from types import SimpleNamespace

import torch

import kge_cases as kc

SIDES = ("tail", "head")


# ---- float64 references -------------------------------------------------------------------------------------------------
def candidate_triples(fixed, et, n, side):
    """(sample [2, Q n], edge_type [Q n]): query q's candidates are the triples q n .. q n + n - 1, candidate id ascending."""
    q = fixed.numel()
    cand = torch.arange(n, device=fixed.device).repeat(q)
    fx = fixed.repeat_interleave(n)
    sample = torch.stack([fx, cand]) if side == "tail" else torch.stack([cand, fx])
    return sample, et.repeat_interleave(n)


def per_candidate(fn, model, ent, rel, fixed, et, gamma, side):
    """fn (kge_cases.raw_score, kge_cases.abs_term_sum) over the candidate triples in float64: [Q, n]."""
    n = ent.shape[0]
    sample, types = candidate_triples(fixed, et, n, side)
    return fn(model, ent.double(), rel.double(), sample, types, gamma).reshape(-1, n)


def scores64(model, ent, rel, fixed, et, gamma, side):
    return per_candidate(kc.raw_score, model, ent, rel, fixed, et, gamma, side)


def split(sample, side):
    """(fixed, truth) of a triple list for a side."""
    return (sample[0], sample[1]) if side == "tail" else (sample[1], sample[0])


def flipped(lists):
    return [(ei.flip(0), et) for ei, et in lists]


def lists_for(lists, side):
    """The lists a KnownPairs / a key list of `side` is built from."""
    return lists if side == "tail" else flipped(lists)


def known_keys(lists, n):
    """Sorted int64 keys (r * n + u) * n + v of (edge_index, edge_type) lists; empty for no lists."""
    if not lists:
        return torch.empty(0, dtype=torch.long)
    return torch.sort(torch.cat([(et * n + ei[0]) * n + ei[1] for ei, et in lists])).values


def known_mask(fixed, r, n, keys):
    """[Q, n] bool: (r, fixed, candidate) is a known pair."""
    want = ((r * n + fixed) * n).unsqueeze(1) + torch.arange(n, device=fixed.device).unsqueeze(0)
    if keys.numel() == 0:
        return torch.zeros_like(want, dtype=torch.bool)
    keys = keys.to(want.device)
    pos = torch.searchsorted(keys, want).clamp_(max=keys.numel() - 1)
    return keys[pos] == want


def ref_rank(scores, truth, mask):
    n = scores.shape[1]
    cand = ~mask & (torch.arange(n, device=scores.device).unsqueeze(0) != truth.unsqueeze(1))
    st = scores.gather(1, truth.unsqueeze(1))
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


# ---- bounds ---------------------------------------------------------------------------------------------------------------
def scan_depth(model, H):
    """Additions on the longest path of the ranking kernels' column sum (csrc/kge_rank.hip as built).  TransE, RotatE: ONE
    serial chain over the H columns and gamma - sum: H + 1 (padding columns add an exact zero).  DistMult, ComplEx: the
    matrix cores' fp32 fused-multiply-add chain over the entity row's H or 2 H columns, one rounding per step."""
    return {"TransE": H + 1, "RotatE": H + 1, "DistMult": H, "ComplEx": 2 * H}[model]


def tolerance(model, H, ent, rel, fixed, et, gamma, side):
    """[Q, n] per-triple bound (T + D) * kappa_s * u * scale of tests/test_gpu_kge.py's docstring, over the candidate triples."""
    n = ent.shape[0]
    sample, types = candidate_triples(fixed, et, n, side)
    kappa = kc.condition_scores(model, ent, rel, sample, types, gamma)
    scale = kc.abs_term_sum(model, ent, rel, sample, types, gamma).reshape(-1, n)
    return (kc.TERM_ROUNDINGS[model] + scan_depth(model, H)) * kappa * kc.U * scale


def rank_bounds(s64, tol, truth, mask):
    """(g_lo, g_hi, candidates inside their band): band(q, v') = tol(q, v') + tol(q, v_true)."""
    n = s64.shape[1]
    cand = ~mask & (torch.arange(n, device=s64.device).unsqueeze(0) != truth.unsqueeze(1))
    st = s64.gather(1, truth.unsqueeze(1))
    band = tol + tol.gather(1, truth.unsqueeze(1))
    g_lo = ((s64 > st + band) & cand).sum(1)
    g_hi = ((s64 >= st - band) & cand).sum(1)
    return g_lo, g_hi, int((g_hi - g_lo).sum())


def check_rank_bounded(s64, tol, truth, mask, greater, ties):
    g_lo, g_hi, _ = rank_bounds(s64, tol, truth, mask)
    g, t = greater.long(), ties.long()
    assert (g >= 0).all() and (t >= 0).all()
    assert (g_lo <= g).all(), int((g_lo - g).max())
    assert (g + t <= g_hi).all(), int((g + t - g_hi).max())


def check_top_k_bounded(s64, tol, mask, scores, ids):
    """The conditions of test_gpu_ranking.check_top_k_bounded with a per-candidate tolerance.  Returns the largest
    |score - s64| / tol over the list entries."""
    k = ids.shape[1]
    assert (ids >= 0).all() and not mask.gather(1, ids).any()
    assert all(len(set(row)) == k for row in ids.tolist())
    err = (s64.gather(1, ids) - scores.double()).abs()
    assert (err <= tol.gather(1, ids)).all()
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    # a candidate left outside scored at most the list's last entry in fp32, so its float64 score less its bound did too
    outside = (s64 - tol).masked_fill(mask, float("-inf")).scatter(1, ids, float("-inf"))
    assert (outside.max(dim=1, keepdim=True).values <= scores[:, -1:].double()).all()
    return float((err / tol.gather(1, ids)).max())


# ---- cases ----------------------------------------------------------------------------------------------------------------
GAMMA = 12.0
EXACT_H = {"TransE": (1, 8, 36, 128), "DistMult": (8, 36, 128), "ComplEx": (1, 8, 36, 64)}
TWINS = ((3, 7), (5, -1))                 # (entity, its copy; -1: the last entity): equal rows, so equal scores


def exact_tables(model, n, R, H, gen):
    """Tables on which fp32 scores are exact whatever the order of the sum: TransE on kge_cases' 2^-16 grid (differences,
    their sums and gamma - sum need at most 23 bits), DistMult and ComplEx small integers."""
    if model == "TransE":
        return kc.tables(model, n, R, H, GAMMA, gen)
    de, dr = kc.dims(model, H)
    return (torch.randint(-3, 4, (n, de), generator=gen).float(), torch.randint(-2, 3, (R, dr), generator=gen).float())


def random_tables(model, n, R, H, gen):
    """fp32 tables uniform in +-embedding_range, as the model initialises them."""
    de, dr = kc.dims(model, H)
    rho = kc.embedding_range(GAMMA, H)
    return (torch.rand(n, de, generator=gen) * 2 - 1) * rho, (torch.rand(R, dr, generator=gen) * 2 - 1) * rho


def ranking_case(model, n, H, seed, exact, Q=300, R=5):
    """Tables, a query list of Q triples and known lists [(random pairs with duplicates), (the queries)]: relation R - 1 has
    no pair in the first list; queries 0..39 are pairs of it; entity 3 is the true tail of queries 40..59 and the true head
    of queries 60..79, and entities 7 and n - 1 carry the rows of 3 and 5 (TWINS)."""
    gen = torch.Generator().manual_seed(seed)
    ent, rel = (exact_tables if exact else random_tables)(model, n, R, H, gen)
    for a, b in TWINS:
        ent[b % n] = ent[a % n]
    e_known = 6 * n
    ki = torch.randint(0, n, (2, e_known), generator=gen)
    kt = torch.randint(0, R - 1, (e_known,), generator=gen)
    ki = torch.cat([ki, ki[:, :50]], 1)                              # duplicates
    kt = torch.cat([kt, kt[:50]])
    qi = torch.randint(0, n, (2, Q), generator=gen)
    qt = torch.randint(0, R, (Q,), generator=gen)
    qi[:, :40], qt[:40] = ki[:, 10:50], kt[10:50]                    # true pairs that are in the filter
    qi[1, 40:60] = 3 % n
    qi[0, 60:80] = 3 % n
    return SimpleNamespace(model=model, n=n, R=R, H=H, gamma=GAMMA, ent=ent, rel=rel, sample=qi, et=qt,
                           lists=[(ki, kt), (qi, qt)])


FILTERS = ("none", "full", "partial")


def filter_lists(case, which):
    return {"none": [], "full": case.lists, "partial": case.lists[:1]}[which]


def tiny_case(model):
    """7 entities, 2 relations, H = 2: small enough for a double loop over every candidate."""
    gen = torch.Generator().manual_seed(11)
    ent, rel = exact_tables(model, 7, 2, 2, gen)
    ent[6] = ent[2]
    sample = torch.tensor([[0, 1, 2, 2, 5, 6, 3, 4], [2, 2, 0, 6, 5, 1, 3, 2]])
    et = torch.tensor([0, 1, 0, 1, 0, 1, 1, 0])
    ki = torch.tensor([[0, 0, 1, 2, 4, 4, 0], [2, 3, 2, 0, 2, 5, 3]])
    kt = torch.tensor([0, 0, 1, 0, 0, 0, 0])
    return SimpleNamespace(model=model, n=7, R=2, H=2, gamma=GAMMA, ent=ent, rel=rel, sample=sample, et=et, lists=[(ki, kt)])
