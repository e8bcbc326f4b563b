"""The candidate-block modes of the KGE baselines ('tail-batch' / 'head-batch' of KGEModel.forward,
baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py:127-136, :150-173): the expansion into a triple list, the cases of
tests/test_kge_batch_host.py and tests/test_gpu_kge_batch.py and the depth of the new query-side sum.  Not a test module.

The float64 reference of the batch modes IS kge_cases.raw_score / reference_gradients / abs_term_sum / abs_contributions on
the expansion, which tests/test_kge_host.py pins to the reference's own runs; there is no second formulation."""
from types import SimpleNamespace

import torch

import kge_cases as kc

SIDES = ("tail", "head")
MODES = {"tail": "tail-batch", "head": "head-batch"}


def expand(positive, et, negatives, side):
    """(sample [2, B * K], et [B * K]) in row-major (b, k) order: the candidates negatives[b, :] stand for the tail of
    positive b (`side` "tail") or for its head ("head"); the other two members are the positive's own."""
    B, K = negatives.shape
    flat = negatives.reshape(-1)
    if side == "tail":
        sample = torch.stack([positive[0].repeat_interleave(K), flat])
    else:
        sample = torch.stack([flat, positive[1].repeat_interleave(K)])
    return sample, et.repeat_interleave(K)


def fixed_of(positive, side):
    """The member of the positives that the candidates do not replace."""
    return positive[0] if side == "tail" else positive[1]


def _case(model, side, n, R, H, gamma, ent, rel, positive, et, negatives, **more):
    sample, et_list = expand(positive, et, negatives, side)
    return SimpleNamespace(model=model, side=side, n=n, R=R, H=H, gamma=gamma, ent=ent, rel=rel, positive=positive, et=et,
                           negatives=negatives, B=negatives.shape[0], K=negatives.shape[1], sample=sample, et_list=et_list,
                           E=sample.shape[1], **more)


SHAPE_BK = ((0, 5), (3, 0), (1, 1), (2, 7), (2, 8), (2, 9), (3, 65), (1, 257))
"""Around one pass of a wave (8 candidates at H = 32), one wave's item (64) and several items of one positive."""


def shape_case(model, H, B, K, side):
    """Random positives and candidates on the tables of kge_cases.shape_case's family: n = 50, R = 4, gamma = 1."""
    gen = torch.Generator().manual_seed(300 + 7 * H)
    ent, rel = kc.tables(model, 50, 4, H, 1.0, gen)
    gen = torch.Generator().manual_seed(1000 * B + K)
    positive = torch.randint(0, 50, (2, B), generator=gen)
    et = torch.randint(0, 4, (B,), generator=gen)
    negatives = torch.randint(0, 50, (B, K), generator=gen)
    return _case(model, side, 50, 4, H, 1.0, ent, rel, positive, et, negatives)


def random_case(model, side, n, R, H, B, K, seed, gamma=12.0):
    """Random tables in +-embedding_range, B random positives with a sorted edge_type, K random candidates each."""
    gen = torch.Generator().manual_seed(seed)
    ent, rel = kc.tables(model, n, R, H, gamma, gen)
    positive = torch.randint(0, n, (2, B), generator=gen)
    et = torch.randint(0, R, (B,), generator=gen).sort().values
    negatives = torch.randint(0, n, (B, K), generator=gen)
    return _case(model, side, n, R, H, gamma, ent, rel, positive, et, negatives)


def case_b(model, side):
    """The vector path with several items per positive: H = 32, B = 5, K = 257."""
    return random_case(model, side, 60, 7, 32, 5, 257, seed=11)


def case_c(model, side):
    """The scalar path: H = 3, B = 4, K = 9.  gamma = 1, as kge_cases.shape_case has it for its narrow rows: at gamma = 12
    the tables' range (gamma + 2) / H is 4.7 and a three-column score reaches +-150, where sigma(-s) is below fp32's range
    (1e-66 in float64, 0 in fp32) and an error in units of u * scale says nothing."""
    return random_case(model, side, 60, 7, 3, 4, 9, seed=12, gamma=1.0)


def case_a(model, side, seed=5):
    """The backward's edge cases in one block (n = 60, R = 7, H = 8, B = 40, K = 130: 5 200 records):
      * entity 0 is a candidate in exactly CHUNK + 1 = 2 049 records: its row of the candidate pass straddles two chunks;
      * entity 1 is the fixed entity of the positives 0, 1, 2 and a candidate of ten elements of other positives;
      * six elements have candidate == fixed entity, under relation 3, whose column 2 is zero: TransE's h + r - t = 0 and
        RotatE's a = b = 0 there - the zero subgradients;
      * entity 59 appears nowhere, the relations 0 and 6 are unused: exact zeros;
      * edge_type is sorted (eight positives of each relation 1..5)."""
    gen = torch.Generator().manual_seed(seed)
    n, R, H, gamma, B, K = 60, 7, 8, 12.0, 40, 130
    ent, rel = kc.tables(model, n, R, H, gamma, gen)
    rel[3, 2] = 0.0
    et = (torch.arange(B) % 5 + 1).sort().values                 # rows 16..23 carry relation 3
    fixed = torch.randint(2, n - 1, (B,), generator=gen)
    fixed[:3] = 1
    other = torch.randint(1, n - 1, (B,), generator=gen)           # the member that the candidates replace: never read
    positive = torch.stack([fixed, other]) if side == "tail" else torch.stack([other, fixed])
    negatives = torch.randint(2, n - 1, (B, K), generator=gen)
    same = [(16, 5), (16, 77), (17, 5), (17, 77), (18, 5), (18, 77)]
    reserved = torch.zeros(B, K, dtype=torch.bool)
    for b, k in same:
        negatives[b, k] = fixed[b]
        reserved[b, k] = True
    free = (~reserved).reshape(-1).nonzero().squeeze(1)
    free = free[torch.randperm(free.numel(), generator=gen)]
    flat = negatives.reshape(-1)                                   # (a view: the assignments land in `negatives`)
    flat[free[:kc.CHUNK + 1]] = 0
    rest = free[kc.CHUNK + 1:]
    rest = rest[rest >= 3 * K][:10]                                # elements of the positives 3 and up
    flat[rest] = 1
    c = _case(model, side, n, R, H, gamma, ent, rel, positive, et, negatives, same=same, unused_entity=n - 1,
              empty_relations=(0, R - 1), zero_relation=3, zero_column=2)
    assert int((negatives == 0).sum()) == kc.CHUNK + 1 and int((negatives == 1).sum()) == 10
    assert not bool((negatives == n - 1).any()) and not bool((positive == n - 1).any())
    return c


def with_bad_ids(c):
    """A copy of the case's block with a negative and a too large id in `fixed`, in `et` and in `negatives`:
    (positive, et, negatives, bad rows, bad elements).  (Not sorted any more: the relation pass sorts.)"""
    positive, et, negatives = c.positive.clone(), c.et.clone(), c.negatives.clone()
    row = 0 if c.side == "tail" else 1
    positive[row, 4], positive[row, 30] = -1, c.n
    et[9], et[25] = -2, c.R
    elements = [(0, 0), (7, 129), (20, 64), (39, 3)]
    for i, (b, k) in enumerate(elements):
        negatives[b, k] = -5 if i % 2 == 0 else c.n + 3
    return positive, et, negatives, [4, 30, 9, 25], elements


def query_reduction_depth(K, B_per_row, lanes):
    """Additions on the longest path of a fixed entity's or a relation's gradient element through the new query-side sum,
    as csrc/kge_batch.hip builds it: a workgroup per positive of S = 256 / lanes slots - a thread's serial sum over
    k = slot, slot + S, ... (ceil(K / S) fused multiply-adds), the fold of the S slots in slot order - and then the
    segmented sum of the row's `B_per_row` partial rows, which is kge_cases.reduction_depth with chunks of ROW_CHUNK
    records: a thread's share of a chunk, the fold over the S threads of a column, the chunks in order."""
    slots = 256 // lanes
    inside = min(B_per_row, ROW_CHUNK)
    return -(-K // slots) + slots + -(-inside // slots) + slots + -(-B_per_row // ROW_CHUNK) + 1


ROW_CHUNK = 32                                                    # records per workgroup of the passes over B records (csrc/kge_batch.hip: kRowChunkRecs)


def reduce_lanes(H, vec=None):
    """Lanes per record of the reductions and of the query-side kernel: 8 for float4 rows of up to 8 units, 16 otherwise."""
    vec = H % 4 == 0 if vec is None else vec
    return 8 if vec and H // 4 <= 8 else 16
