"""Per-relation candidate ranges (the `candidates` argument of rank / top_k / kge.sample_candidates): the range tables of the
tests, the out-of-range masks of the float64 references, and the numpy model of the documented RANGED candidate draw
(include/gripnet_hip.h, gn_kge_candidates_sample_ranged).  tests/test_typed_candidates_host.py and
tests/test_gpu_typed_candidates.py.  Not a test module."""
import numpy as np
import torch

import kge_loss_cases as lc

R = 5
EMPTY = 4                                                        # the relation whose range is empty


def ranges(n):
    """[R, 2] int64 per n of kge_rank_cases' NS = (37, 645, 2113):
    r0 everything; r1 [5, 23) inside one stage - it holds entity 7 and not its twin 3, so tie counts change; r2 across the
    stage boundary at 64 (n = 37: up to n, with the last entity, the twin of 5; n = 2113: from the start of a bitmap
    window); r3 the last entities (n = 2113: across the window boundary at 2048 and up to n); r4 empty."""
    r2 = {37: (30, 37), 2113: (2048, 2100)}.get(n, (50, 70))
    r3 = {37: (36, 37), 645: (600, 645), 2113: (2040, 2113)}[n]
    return torch.tensor([(0, n), (5, 23), r2, r3, (9, 9)], dtype=torch.int64)


def outside(table, et, n):
    """[Q, n] bool: candidate v is outside the range of query q's relation."""
    table = table.to(et.device)
    v = torch.arange(n, device=et.device).unsqueeze(0)
    return (v < table[et, 0].unsqueeze(1)) | (v >= table[et, 1].unsqueeze(1))


def draw(fixed, et, K, n, seed, table, rows=None, step=0):
    """(cand int64 [B, K], flag bits, the highest attempt an element went to) of the documented ranged draw:
    attempt a: c = lo + ((low32(mix64(base + a)) * (hi - lo)) >> 32) with (lo, hi) = table[et[b]] and base as in
    kge_loss_cases.draw.  A fixed entity outside [0, n), a relation outside the table, or a row that is no sub-range of
    [0, n]: a row of -1 and bit 0; an empty range: a row of -1 and bit 1.  rows: kge_loss_cases.known_rows(...) or None."""
    fixed, et = [int(v) for v in fixed], [int(v) for v in et]
    table = [(int(lo), int(hi)) for lo, hi in np.asarray(table).tolist()]
    B = len(fixed)
    cand = np.empty((B, K), dtype=np.int64)
    flags, most = 0, 0
    seed = (seed + step) & lc.M64
    for b in range(B):
        if not 0 <= fixed[b] < n or not 0 <= et[b] < len(table):
            cand[b], flags = -1, flags | 1
            continue
        lo, hi = table[et[b]]
        if lo < 0 or hi > n or lo > hi:
            cand[b], flags = -1, flags | 1
            continue
        if lo == hi:
            cand[b], flags = -1, flags | 2
            continue
        row = rows.get((et[b], fixed[b]), ()) if rows is not None else ()
        for k in range(K):
            base = lc.mix64(seed ^ (((b * K + k) * 0xD6E8FEB86659FD93) & lc.M64))
            for a in range(lc.MAX_ATTEMPTS):
                c = lo + (((lc.mix64((base + a) & lc.M64) & 0xFFFFFFFF) * (hi - lo)) >> 32)
                if c not in row:
                    break
            else:
                flags |= 2
            most = max(most, a)
            cand[b, k] = c
    return cand, flags, most
