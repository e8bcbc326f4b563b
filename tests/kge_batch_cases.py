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


D_RELATION_COUNTS = ((1, 31), (2, 2), (4, 31), (5, 32), (7, 70), (8, 1), (10, 33), (11, 30))
D_ENTITY_COUNTS = ((3, 31), (4, 2), (5, 31), (9, 32), (20, 70)) + tuple((e, 1) for e in range(30, 64)) + ((80, 30),)
D_HIDDEN = (8, 36, 72, 35)
"""One column block on 8 lanes; 9 units on 16 lanes; 18 units - a second column block of the reductions and a second trip of
the query kernel's column loop; the scalar path with three column blocks."""


def _repeat(counts):
    return torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in counts])


def case_d(model, side, H, shuffled, seed=31):
    """Rows of the passes over the B positives (chunks of ROW_CHUNK = 32 records) that lie in more than one chunk: n = 90,
    R = 12, K = 5, B = 230 = 7 * 32 + 6, gamma as case_c argues (12 at H % 4 == 0, 1 on the scalar path).  In key order the
    relations D_RELATION_COUNTS hold the positions
      1: 0-30    2: 31-32    4: 33-63    5: 64-95    7: 96-165    8: 166    10: 167-199    11: 200-229
    so relation 2 is a two-record row across a cut (the chunk's second slot, then the next chunk's first), 4 ends on a cut, 5
    is exactly one aligned chunk (final, never a partial), 7 begins on a cut and spans three chunks with chunk 4 wholly inside
    it, chunk 5 holds the end of 7, the one-record row 8 and the start of 10, chunk 6 the end of 10 and the start of 11, the
    last chunk holds six records, and the relations 0, 3, 6 and 9 are empty.  The fixed entities D_ENTITY_COUNTS cut the
    same way up to position 165 (3, 4, 5, 9, 20), then come 34 entities of one positive each and entity 80 on 200-229; they
    are dealt to the positives in a random order, so the entity pass sorts a real permutation and adds its straddling rows
    onto the candidate pass's sums (the candidates are uniform over the entities 0..88: the rows 3, 9 and 20 of d_ent get
    both).  Entity 89 appears nowhere.
    `shuffled`: the positives (with their candidates and upstream rows) in a random order, as a training batch has them;
    otherwise THAT block reordered by et.sort(stable=True) - what a stable sort by relation makes of it.  The upstream
    `up` [B, K] belongs to the positives and moves with them."""
    n, R, K, B = 90, 12, 5, 230
    gamma = 12.0 if H % 4 == 0 else 1.0
    gen = torch.Generator().manual_seed(seed)
    ent, rel = kc.tables(model, n, R, H, gamma, gen)
    et = _repeat(D_RELATION_COUNTS)
    fixed = _repeat(D_ENTITY_COUNTS)
    assert et.numel() == B and fixed.numel() == B
    fixed = fixed[torch.randperm(B, generator=gen)]
    other = torch.randint(0, n - 1, (B,), generator=gen)           # the member that the candidates replace: never read
    negatives = torch.randint(0, n - 1, (B, K), generator=gen)
    up = torch.linspace(-1.0, 1.0, B * K).view(B, K)
    order = torch.randperm(B, generator=gen)
    if not shuffled:
        order = order[et[order].sort(stable=True).indices]
    et, fixed, other, negatives, up = et[order], fixed[order], other[order], negatives[order].contiguous(), up[order].contiguous()
    positive = torch.stack([fixed, other]) if side == "tail" else torch.stack([other, fixed])
    return _case(model, side, n, R, H, gamma, ent, rel, positive, et, negatives, up=up, unused_entity=n - 1,
                 empty_relations=(0, 3, 6, 9))


def case_e(model, side):
    """More positives than the query kernel's grid of 16 384 workgroups: B = 16 385, K = 2, H = 4, n = 500, R = 9.  A
    relation owns about 1 820 positives: the combine adds the partials of some 58 chunks of ROW_CHUNK records."""
    return random_case(model, side, 500, 9, 4, 16385, 2, seed=41)


def straddling_rows(keys, chunk=None):
    """{key: (first, last + 1)} of the rows of `keys` in key order whose records lie in more than one chunk of `chunk`
    records (ROW_CHUNK by default): the rows that leave the reduction as chunk partials and are added by the combine."""
    chunk = ROW_CHUNK if chunk is None else chunk
    counts = torch.bincount(keys)
    ends = torch.cumsum(counts, 0)
    out = {}
    for key, (count, end) in enumerate(zip(counts.tolist(), ends.tolist())):
        begin = end - count
        if count > 0 and begin // chunk != (end - 1) // chunk:
            out[key] = (begin, end)
    return out


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
