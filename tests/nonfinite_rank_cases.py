"""Ranking and top-k under non-finite scores: the float64 references of the documented contract (include/gripnet_hip.h, both
ranking sections) and the poisoned cases of tests/test_nonfinite_rank_host.py and tests/test_gpu_nonfinite_ranking.py.
Not a test module.

The contract - a non-finite score never flatters the model:
  rank   greater = the admitted candidates c with NOT (s(c) <= s(true)), ties = those with s(c) == s(true).  A NaN true
         score therefore puts every admitted candidate into `greater` (the true triple ranks last, ties = 0), a NaN
         candidate counts as greater than any true score, the infinities compare as numbers (equal infinities tie, a -inf
         candidate is greater than nothing).  The filter comes first: a known, out-of-range or true candidate never counts.
  top-k  a NaN or -inf score never enters, +inf enters, equal scores order by ascending id, padding is -inf / -1.
Non-finite scores set no bit of the error word.
The score is kge_cases.raw_score in float64 - except ComplEx on the head side, whose scan folds relation and tail into the
query row first (`complex_head_score`; the header documents it): with an infinite entry that form gives +-inf where
raw_score gives NaN, and the kernels are held to the form they document.  Found by these tests on the first GPU run.

Cases.  kge_rank_cases.ranking_case(model, n, H, seed, exact=True) at n in NS and H in widths(model): scores on these tables
are exact in fp32 in any summation order, so every comparison with the float64 reference is torch.equal.  RotatE has no exact
table of its own: `case` builds one from TransE's grid (all phases 0: cos = 1 and sin = 0 exactly; the entity rows' real half
on the grid, the imaginary half zero), on which a column's modulus is sqrt(a * a) = |a| exactly.  This checks the COMPARISON
logic of RotatE's instantiation, not its arithmetic, which test_gpu_kge_ranking.test_bounded holds.  "decoder" is the
DistMult case with z = the entity table (test_gpu_typed_candidates.decoder_of), tail side only.

Poison.  `poisoned(c, side, poison)` returns COPIES of the tables (the case's tensors are never written) with the rows of
`poison_rows(c, side)` overwritten: NaN, +inf or -inf over the whole row, or +inf in column COLUMN only.  On the integer
tables of DistMult / ComplEx / the decoder a whole-row infinity mostly yields NaN (inf * 0, inf - inf); the single column is
what produces +inf and -inf scores.  TransE and RotatE score gamma - distance and never reach +inf.  The decoder has one
more variant, "D+inf@col": +inf in column COLUMN of relation D_ROW's row of the relation table, the entity rows clean."""
import functools
from types import SimpleNamespace

import torch

import kge_cases as kc
import kge_rank_cases as rc
import typed_candidates_cases as tc

NS = (37, 645, 2113)                # one partial stage; several 64-column stages; the bitmap window boundary at 2048
MODELS = ("TransE", "DistMult", "ComplEx", "RotatE", "decoder")
POISONS = ("nan", "+inf", "-inf", "+inf@col")
COLUMN = 1                          # the single poisoned column (of the real half)
D_ROW = 1                           # "D+inf@col": the poisoned relation
KS = (1, 10, 64)
FLOOD_N, FLOOD_K, FLOOD_STEP = 645, 64, 8       # flood: every 8th row (81 rows over all 11 stages) holds +inf in COLUMN


def widths(model):
    return (8, 36, 128) if model == "TransE" else (8, 36)


def poisons(model):
    return POISONS + (("D+inf@col",) if model == "decoder" else ())


def sides(model):
    return ("tail",) if model == "decoder" else rc.SIDES


def scorer(model):
    """The scorer whose formulation (kge_cases.raw_score) gives the model's scores."""
    return "DistMult" if model == "decoder" else model


CASES = [(m, n, H) for m in MODELS for n in NS for H in widths(m)]
POISONED = [(m, n, H, p) for m, n, H in CASES for p in poisons(m)]


@functools.lru_cache(maxsize=None)
def case(model, n, H):
    """The exact case of (model, n, H); shared, never written."""
    seed = 1000 + 7 * n + H
    if model != "RotatE":
        c = rc.ranking_case(scorer(model), n, H, seed, True)
        c.model = model
        return c
    c = rc.ranking_case("TransE", n, H, seed, True)
    c.model = "RotatE"
    c.ent = torch.cat([c.ent, torch.zeros_like(c.ent)], 1)
    c.rel = torch.zeros_like(c.rel)
    return c


# ---- float64 references ------------------------------------------------------------------------------------------------
def ref_rank(scores64, truth, mask):
    """(greater, ties) of the contract; `mask` [Q, n] holds every candidate that is not admitted for another reason than
    being the true partner (known pairs, out of range)."""
    n = scores64.shape[1]
    cand = ~mask & (torch.arange(n, device=scores64.device).unsqueeze(0) != truth.unsqueeze(1))
    st = scores64.gather(1, truth.unsqueeze(1))
    return (~(scores64 <= st) & cand).sum(1), ((scores64 == st) & cand).sum(1)


def old_rule_greater(scores64, truth, mask):
    """`greater` of the rule the kernels had before (s(c) > s(true)): what the contract replaces."""
    return rc.ref_rank(scores64, truth, mask)[0]


def ref_topk(scores64, mask, k):
    """(values float64 [Q, k], ids [Q, k]): NaN and -inf never enter, stable descending sort (equal scores keep ascending
    ids), padded with -inf / -1; padding is told by isneginf, so a +inf entry keeps its id."""
    s = scores64.to(torch.float64)
    s = s.masked_fill(mask | torch.isnan(s) | torch.isneginf(s), float("-inf"))
    val, idx = torch.sort(s, dim=1, descending=True, stable=True)
    val, idx = val[:, :k], idx[:, :k]
    if val.shape[1] < k:
        pad = k - val.shape[1]
        val = torch.cat([val, torch.full((val.shape[0], pad), float("-inf"), dtype=val.dtype, device=val.device)], 1)
        idx = torch.cat([idx, torch.full((idx.shape[0], pad), -1, dtype=idx.dtype, device=idx.device)], 1)
    return val, torch.where(torch.isneginf(val), torch.full_like(idx, -1), idx)


def scores(model, ent, rel, fixed, et, gamma, side, dtype=torch.float64):
    """[Q, n] scores of every candidate by kge_cases.raw_score in `dtype` (float64: the reference; float32: the torch
    formulation the host test holds to it)."""
    return _scores(model, ent.to(dtype), rel.to(dtype), fixed, et, gamma, side, torch.arange(ent.shape[0], device=fixed.device))


def _scores(model, ent, rel, fixed, et, gamma, side, cand):
    """[Q, len(cand)]: the scores of the candidates `cand` only, in the tables' dtype."""
    m = cand.numel()
    chunk = max(1, (1 << 24) // max(1, m * ent.shape[1]))            # queries per call: blocks of at most 2^24 elements
    out = [torch.empty(0, m, dtype=ent.dtype, device=ent.device)]
    for a in range(0, fixed.numel(), chunk):
        fx, types = fixed[a:a + chunk], et[a:a + chunk]
        cnd, fx = cand.repeat(fx.numel()), fx.repeat_interleave(m)
        sample = torch.stack([fx, cnd]) if side == "tail" else torch.stack([cnd, fx])
        types = types.repeat_interleave(m)
        if model == "ComplEx" and side == "head":
            out.append(complex_head_score(ent, rel, sample, types).reshape(-1, m))
        else:
            out.append(kc.raw_score(scorer(model), ent, rel, sample, types, gamma).reshape(-1, m))
    return torch.cat(out)


def complex_head_score(ent, rel, sample, et):
    """ComplEx scored the way the head-side scan scores it (include/gripnet_hip.h, the KGE ranking section): the relation
    and the fixed tail are folded into one row first, sum_k (rr tr + ri ti)_k hr_k + (rr ti - ri tr)_k hi_k.  On finite rows
    this is kge_cases.raw_score regrouped (the same value on the exact tables); with a non-finite entry the two differ in
    kind - +inf in a candidate's hr_k gives +-inf here by the sign of (rr tr + ri ti)_k, where Re((h r) conj t) gives NaN
    as soon as one of rr, ri, tr, ti is zero there.  The contract speaks of the score the scan compares: this one."""
    head, relation, tail = kc.rows(ent, rel, sample, et)
    H = relation.shape[1] // 2
    (hr, hi), (rr, ri), (tr, ti) = [(x[:, :H], x[:, H:]) for x in (head, relation, tail)]
    return (torch.cat([rr * tr + ri * ti, rr * ti - ri * tr], 1) * torch.cat([hr, hi], 1)).sum(dim=1)


def poisoned_scores(c, side, poison, clean, dtype=torch.float64):
    """[Q, n] scores of the case on the tables of `poisoned(c, side, poison)`, from `clean` (the scores of the case's own
    tables in `dtype`, left unchanged): a score is a function of the fixed entity's row, the relation's row and the
    candidate's row, so only the queries whose fixed entity or relation is poisoned and the poisoned candidates' columns are
    evaluated again.  The host test holds this to the full evaluation."""
    ent, rel = [x.to(device=clean.device, dtype=dtype) for x in poisoned(c, side, poison)]
    fixed, _ = rc.split(c.sample.to(clean.device), side)
    et = c.et.to(clean.device)
    s = clean.clone()
    if poison == "D+inf@col":
        again = et == D_ROW
    else:
        rows = torch.tensor(poison_rows(c.model, c.n, c.H, side), device=clean.device)
        again = torch.isin(fixed, rows)
        s[:, rows] = _scores(c.model, ent, rel, fixed, et, c.gamma, side, rows)
    s[again] = scores(c.model, ent, rel, fixed[again], et[again], c.gamma, side, dtype)
    return s


def masks(c, side, device="cpu"):
    """{filter name: [Q, n] known mask} of the case's queries on `side`."""
    fixed, _ = rc.split(c.sample, side)
    out = {}
    for which in rc.FILTERS:
        keys = rc.known_keys(rc.lists_for(rc.filter_lists(c, which), side), c.n)
        out[which] = rc.known_mask(fixed, c.et, c.n, keys).to(device)
    return out


def outside(c, device="cpu"):
    """[Q, n]: candidate outside the range of the query's relation (typed_candidates_cases.ranges)."""
    return tc.outside(tc.ranges(c.n), c.et, c.n).to(device)


# ---- poison ----------------------------------------------------------------------------------------------------------------
QUERIES_FIXED = (100, 200)          # their fixed entities are poisoned
QUERY_TRUE = 150                    # its true partner is poisoned
QUERY_KNOWN = 120                   # the first query from here on with a known partner that is not its true one: poisoned


@functools.lru_cache(maxsize=None)
def poison_rows(model, n, H, side):
    """Sorted ids of the poisoned entity rows of the case on `side`:
      entity 3 - the true partner of queries 40..59 (tail) / 60..79 (head) and the fixed entity of the other twenty; its twin
        7 stays clean, so the twins stop tying;
      the fixed entities of QUERIES_FIXED and the true partner of QUERY_TRUE;
      candidate rows 0, 63, 64, n - 2, n - 1 and, past the bitmap window boundary, 2047, 2048, 2050 (those below n);
      a known partner of one query (rows 0, 63, 64 lie outside the ranges [5, 23) of relation 1 for every n)."""
    return rows_of(case(model, n, H), side)


def rows_of(c, side):
    """poison_rows for any kge_rank_cases.ranking_case."""
    n = c.n
    fixed, truth = rc.split(c.sample, side)
    rows = {3, int(truth[QUERY_TRUE]), 0, 63, 64, n - 2, n - 1, 2047, 2048, 2050}
    rows |= {int(fixed[q]) for q in QUERIES_FIXED}
    keys = rc.known_keys(rc.lists_for(c.lists, side), n)
    for q in range(QUERY_KNOWN, c.sample.shape[1]):
        known = rc.known_mask(fixed[q:q + 1], c.et[q:q + 1], n, keys)[0]
        known[truth[q]] = False
        if bool(known.any()):
            rows.add(int(known.nonzero()[0]))
            break
    return tuple(sorted(r for r in rows if 0 <= r < n))


def _value(poison):
    return {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[poison]


def poisoned(c, side, poison):
    """(ent, rel): copies of the case's tables with the poison written."""
    ent, rel = c.ent.clone(), c.rel.clone()
    if poison == "D+inf@col":
        rel[D_ROW, COLUMN] = float("inf")
        return ent, rel
    rows = torch.tensor(poison_rows(c.model, c.n, c.H, side))
    if poison == "+inf@col":
        ent[rows, COLUMN] = float("inf")
    elif poison == "zero":                                            # the poisoned rows cleared: the twin launch of the bits test
        ent[rows] = 0.0
    else:
        ent[rows] = _value(poison)
    return ent, rel


def flood(c):
    """(ent, rel) of the flood variant: +inf in COLUMN of every FLOOD_STEP-th entity row.  A query whose operand is positive
    in that column scores +inf on all of them: a top-64 list full of equal +inf, ordered by id alone."""
    ent, rel = c.ent.clone(), c.rel.clone()
    ent[::FLOOD_STEP, COLUMN] = float("inf")
    return ent, rel


def clean_queries(c, side, s64):
    """[Q] bool: the fixed entity is not poisoned and the true score is finite."""
    fixed, truth = rc.split(c.sample, side)
    rows = torch.tensor(poison_rows(c.model, c.n, c.H, side))
    st = s64.gather(1, truth.to(s64.device).unsqueeze(1)).squeeze(1)
    return ~torch.isin(fixed, rows).to(s64.device) & torch.isfinite(st)


def classes(model):
    """The non-finite classes the model's scores can take."""
    return ("nan", "-inf") + (("+inf",) if scorer(model) in ("DistMult", "ComplEx") else ())


def in_class(s, name):
    return {"nan": torch.isnan, "-inf": torch.isneginf, "+inf": torch.isposinf}[name](s)
