"""The shared-candidate-list modes of the KGE baselines ('tail-shared' / 'head-shared' of KGEModel.forward,
csrc/kge_shared.hip): the chunk rule, the expansion into the candidate block of the batch modes, the cases of
tests/test_kge_shared_host.py and tests/test_gpu_kge_shared.py, and the fold depths of the new sums.  Not a test module.

The float64 reference of the shared modes IS kge_batch_cases' (kge_cases.raw_score / reference_gradients / abs_term_sum /
abs_contributions on the expansion of the block) with every chunk's list expanded to its positives - negatives[g].expand per
chunk; there is no new arithmetic here."""
import functools

import torch

import kge_batch_cases as kb
import kge_cases as kc
import kge_rank_cases as kr

SIDES = kb.SIDES
MODES = {"tail": "tail-shared", "head": "head-shared"}

N, R = 40, 5
"""Entities and relations of every case; entity N - 1 and relation R - 1 appear nowhere: their gradient rows are exact zeros."""

SHAPES = {"a": (48, 1, 1), "b": (51, 3, 65), "c": (34, 2, 17), "d": (6, 6, 5), "e": (2000, 1, 3)}
"""(B, G, K).  a: one shared list of one candidate.  b: chunks of 17 - a partial 16-row tile of a wave, a partial 64-row tile of a
workgroup - and K one past a 64-column stage.  c: a second partial-tile shape (chunks of 17, a partial 16-column tile).  d: G == B,
the batch modes' meaning.  e: the hub - 2 000 positives in one chunk (32 workgroup tiles, the last one partial; eight trips of the
candidate side's 256-id staging), K = 3: a long fixed-order sum on the candidate side."""

MAX_ROW = 128                                                     # floats of an entity row the kernels take (_hip.KGE_SHARED_MAX_ROW)


def entity_parts(model):
    return 2 if model in ("ComplEx", "RotatE") else 1


def widths(model):
    """kge_rank_cases.EXACT_H (RotatE: ComplEx's, its entity rows are as wide), 36 and the largest admitted width."""
    base = kr.EXACT_H.get(model, kr.EXACT_H["ComplEx"])
    return tuple(sorted(set(base) | {36, MAX_ROW // entity_parts(model)}))


def first_refused_width(model):
    return MAX_ROW // entity_parts(model) + 1


def gamma_of(H):
    """12 where the tables' range (gamma + 2) / H keeps |s| moderate, 1 on the narrow rows (kge_batch_cases.case_c argues it)."""
    return 12.0 if H % 4 == 0 else 1.0


def chunk_of(B, G):
    """[B]: the chunk g = b // (B // G) of every positive."""
    assert 1 <= G <= B and B % G == 0
    return torch.arange(B) // (B // G)


def expand_lists(lists, B):
    """[B, K]: the candidate block of the batch modes that the shared lists [G, K] stand for - negatives[g].expand per chunk."""
    G, K = lists.shape
    assert 1 <= G <= B and B % G == 0
    return torch.cat([lists[g].expand(B // G, K) for g in range(G)]).contiguous()


@functools.lru_cache(maxsize=None)
def family_tables(model, H):
    """One pair of tables per (model, H) on kge_cases.tables' 2^-16 grid: the five shapes of a family share it."""
    gen = torch.Generator().manual_seed(700 + 11 * H)
    return kc.tables(model, N, R, H, gamma_of(H), gen)


def case(model, side, H, name):
    """Shape `name` of SHAPES on the family's tables: random positives (entities 0 .. N - 2, relations 0 .. R - 2, edge_type in
    batch order: not sorted) and lists, with the three patterns
      * a candidate repeated inside a list:            lists[0, K - 1] = lists[0, 0]                 (K > 1)
      * the same entity in two chunks' lists:          lists[1, 0] = lists[0, 0]                     (G > 1)
      * a candidate equal to the positive's own head AND tail:  positive[:, 0] = lists[0, 0]         (positive 0 is of chunk 0).
    The case is kge_batch_cases' (its sample / et_list: the expansion of the block expand_lists gives) plus `lists` and `G`."""
    B, G, K = SHAPES[name]
    ent, rel = family_tables(model, H)
    gen = torch.Generator().manual_seed(9000 + 13 * B + K)
    positive = torch.randint(0, N - 1, (2, B), generator=gen)
    et = torch.randint(0, R - 1, (B,), generator=gen)
    lists = torch.randint(0, N - 1, (G, K), generator=gen)
    if K > 1:
        lists[0, K - 1] = lists[0, 0]
    if G > 1:
        lists[1, 0] = lists[0, 0]
    positive[:, 0] = lists[0, 0]
    return kb._case(model, side, N, R, H, gamma_of(H), ent, rel, positive, et, expand_lists(lists, B), lists=lists, G=G, name=name,
                    unused_entity=N - 1, unused_relation=R - 1)


def upstream(c):
    return torch.linspace(-1.0, 1.0, c.B * c.K).view(c.B, c.K) if c.B * c.K > 1 else torch.ones(c.B, c.K)


def with_bad_ids(c):
    """(positive, et, lists, bad rows, bad (chunk, column) pairs): a negative and a too large id among the fixed entities, the
    relations and the lists' entries."""
    positive, et, lists = c.positive.clone(), c.et.clone(), c.lists.clone()
    row = 0 if c.side == "tail" else 1
    B, (G, K) = c.B, lists.shape
    rows = sorted({1 % B, B // 2, B - 1, (B - 2) % B})
    positive[row, rows[0]] = -1
    positive[row, rows[-1]] = c.n
    if len(rows) > 2:
        et[rows[1]] = -2
    if len(rows) > 3:
        et[rows[2]] = c.R
    columns = sorted({(0, 0), (G - 1, K - 1), (G // 2, K // 2)})
    for i, (g, k) in enumerate(columns):
        lists[g, k] = -5 if i % 2 == 0 else c.n + 3
    return positive, et, lists, rows, columns


# ---- fold depths of the new sums (csrc/kge_shared.hip as built) ------------------------------------------------------------
def score_depth(model, H):
    """D: additions on the longest path of a score's column sum.  TransE, RotatE: ONE serial chain over the H columns (padding
    columns add an exact zero) and gamma - sum: H + 1.  DistMult, ComplEx: the entity row's H or 2 H columns, padded to groups of
    16, go group by group to four partial sums in turn - each a chain of fp32 fused multiply-adds on the matrix cores, one
    rounding per step (a padding column adds an exact zero) - and the partials are added pairwise: at most 16 columns for
    each of the first partial's groups 0, 4, ..., and 2."""
    if model in ("TransE", "RotatE"):
        return H + 1
    row = entity_parts(model) * H
    return sum(min(16, row - first) for first in range(0, row, 64)) + 2


def rows_depth(records, lanes):
    """The segmented sum of `records` partial rows in chunks of kge_batch_cases.ROW_CHUNK records (kge_cases.reduction_depth at
    that chunk size): a thread's share of a chunk, the fold over the threads of a column, the chunks in order."""
    slots = 256 // lanes
    inside = min(records, kb.ROW_CHUNK)
    return -(-inside // slots) + slots + -(-records // kb.ROW_CHUNK) + 1


def _busiest(ids):
    return int(torch.bincount(ids.reshape(-1), minlength=1).max())


def gradient_depths(c):
    """(R of d_ent, R of d_rel): additions on the longest path of a gradient element.  A list entry's partial row is a serial
    chain over its chunk's B / G positives, a positive's partial rows are serial chains over the K candidates (one fused
    multiply-add per contribution); the rows of an entity - as a candidate, then as a fixed entity, one accumulating add
    between the two passes - and of a relation go through rows_depth."""
    lanes = kb.reduce_lanes(c.H)
    fixed = kb.fixed_of(c.positive, c.side)
    r_ent = c.B // c.G + rows_depth(_busiest(c.lists), lanes) + c.K + rows_depth(_busiest(fixed), lanes) + 1
    r_rel = c.K + rows_depth(_busiest(c.et), lanes)
    return r_ent, r_rel
