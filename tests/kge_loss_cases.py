"""The KGE mini-batch path (csrc/kge_loss.hip, k_kge_candidates of csrc/negsample.hip): the float64 / fp32 torch formulation
of the negative-sampling loss, the error figures of tests/test_gpu_kge_loss.py, its cases, and the numpy model of the
documented candidate draw (include/gripnet_hip.h, gn_kge_candidates_sample).  Not a test module."""
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -126                                               # fp32's smallest normal

# ---- the loss kernel's shape limits (csrc/kge_loss.hip) -----------------------------------------------------------------
SMALL_K = 32                      # kNsSmallK: rows up to here share a wave in power-of-two lane groups
REGISTER_K = 1024                 # kNsPart: a row is held in registers up to here; beyond, parts with a running maximum
GRID_WAVES = 512 * 4              # kNsGroups workgroups of four waves: one pass of the forward's grid
ONE_PASS_ROWS_K2 = GRID_WAVES * 32
"""Rows of K = 2 (a lane group of 2: 32 rows per wave) that the forward takes in a single pass of its grid."""

KS = (1, 2, 7, 8, 33, 64, 65, 257, REGISTER_K, REGISTER_K + 1)
BS = (1, 3, 5)
TEMPERATURES = (None, 0.5, 1.0, 4.0)
AMPLITUDES = (4.0, 200.0)


def block(B, K, amplitude, weighted, seed=0):
    """(pos [B], neg [B, K], weight [B] or None): scores uniform in +-amplitude, weights rand + 0.5."""
    gen = torch.Generator().manual_seed(1000 * K + 10 * B + seed + (7 if amplitude > 10 else 0))
    pos = (torch.rand(B, generator=gen) * 2 - 1) * amplitude
    neg = (torch.rand(B, K, generator=gen) * 2 - 1) * amplitude
    weight = torch.rand(B, generator=gen) + 0.5 if weighted else None
    return pos, neg, weight


def hand_built(K, T):
    """Five rows: all scores equal (pos = 200); one score more than 104 / T above the rest, so that every other weight
    underflows (pos = -200); a zero score (pos = 0); a row of weight 0; an ordinary row."""
    gen = torch.Generator().manual_seed(77 + K)
    neg = (torch.rand(5, K, generator=gen) * 2 - 1) * 4
    pos = (torch.rand(5, generator=gen) * 2 - 1) * 4
    neg[0] = 1.25
    neg[1] = -3.0 + 0.5 * torch.rand(K, generator=gen)
    neg[1, K // 2] = -2.5 + 104.0 / (T or 1.0) + 5.0
    neg[2, 0] = 0.0
    pos[0], pos[1], pos[2] = 200.0, -200.0, 0.0
    weight = torch.tensor([1.0, 0.7, 1.3, 0.0, 0.9])
    return pos, neg, weight


def loss_terms(p, n, T, weight):
    """(loss, w, P, L, share) of the formulas of the header comment on tensors of one dtype; without weights the loss is
    kge.self_adversarial_loss, operation for operation."""
    P, L = F.logsigmoid(p), F.logsigmoid(-n)
    share = torch.full_like(L, 1.0 / n.shape[1]) if T is None else F.softmax(n * T, dim=1).detach()
    N = L.mean(dim=1) if T is None else (share * L).sum(dim=1)
    if weight is None:
        return (-P.mean() - N.mean()) / 2, torch.ones_like(P), P, L, share
    w = weight.to(p.dtype)
    return (-(w * P).sum() / w.sum() - (w * N).sum() / w.sum()) / 2, w, P, L, share


def formulation(pos, neg, T, weight, dtype):
    """(loss, d_pos, d_neg, S) through torch autograd in `dtype`.  S: the sum of the terms' absolute values over 2 W (the
    scale of the loss's error)."""
    p = pos.to(dtype).clone().requires_grad_(True)
    n = neg.to(dtype).clone().requires_grad_(True)
    loss, w, P, L, share = loss_terms(p, n, T, weight)
    loss.backward()
    S = ((w * P.abs()).sum() + (w[:, None] * share * L.abs()).sum()) / (2 * w.sum())
    return loss.detach(), p.grad, n.grad, float(S.detach())


def figure(got, ref, strict=True):
    """max |got - ref| / (u |ref|) over the elements with |ref| >= 2^-126; the elements whose float64 reference lies below
    must satisfy |got| <= 2^-126 (asserted when `strict`; the reference formulation itself is only measured)."""
    got, ref = got.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    big = ref.abs() >= TINY
    if strict:
        assert bool((got[~big].abs() <= TINY).all()), float(got[~big].abs().max())
    if not bool(big.any()):
        return 0.0
    return float(((got[big] - ref[big]).abs() / (U * ref[big].abs())).max())


@lru_cache(maxsize=None)
def reference(kind, B, K, amplitude, weighted, T):
    """The case's block, its float64 reference and the fp32 torch formulation's figures t = (loss, d_pos, d_neg)."""
    pos, neg, weight = hand_built(K, T) if kind == "hand" else block(B, K, amplitude, weighted)
    l64, dp64, dn64, S = formulation(pos, neg, T, weight, torch.float64)
    l32, dp32, dn32, _ = formulation(pos, neg, T, weight, torch.float32)
    t = (abs(float(l32) - float(l64)) / (U * S), figure(dp32, dp64, strict=False), figure(dn32, dn64, strict=False))
    return dict(pos=pos, neg=neg, weight=weight, loss=float(l64), d_pos=dp64, d_neg=dn64, S=S, t=t)


# ---- the candidate draw -------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
MAX_ATTEMPTS = 4096


def mix64(x):
    """The splitmix64 finaliser on Python integers."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def known_rows(edge_index, edge_type, side):
    """{(relation, fixed entity): set of partners} of a triple list, keyed as a KnownPairs for `side` is."""
    rows = {}
    fixed, other = (0, 1) if side == "tail" else (1, 0)
    for a, b, r in zip(edge_index[fixed].tolist(), edge_index[other].tolist(), edge_type.tolist()):
        rows.setdefault((r, a), set()).add(b)
    return rows


def draw(fixed, et, K, n, seed, rows=None, nrelation=None, step=0):
    """(cand int64 [B, K], flag bits, the highest attempt a that an element went to: 0 when every first draw was taken) of the
    documented draw.  rows: known_rows(...) or None."""
    fixed, et = [int(v) for v in fixed], [int(v) for v in et]
    B = len(fixed)
    cand = np.empty((B, K), dtype=np.int64)
    flags, most = 0, 0
    seed = (seed + step) & M64
    for b in range(B):
        if not 0 <= fixed[b] < n or et[b] < 0 or (nrelation is not None and et[b] >= nrelation):
            cand[b], flags = -1, flags | 1
            continue
        row = rows.get((et[b], fixed[b]), ()) if rows is not None else ()
        for k in range(K):
            base = mix64(seed ^ (((b * K + k) * 0xD6E8FEB86659FD93) & M64))
            for a in range(MAX_ATTEMPTS):
                c = ((mix64((base + a) & M64) & 0xFFFFFFFF) * n) >> 32
                if c not in row:
                    break
            else:
                flags |= 2
            most = max(most, a)
            cand[b, k] = c
    return cand, flags, most


def chi_square(counts, allowed):
    """Pearson's statistic of `counts` (per entity) against the uniform distribution over the `allowed` entities."""
    total = counts[allowed].sum()
    expected = total / len(allowed)
    return float(((counts[allowed] - expected) ** 2 / expected).sum())
