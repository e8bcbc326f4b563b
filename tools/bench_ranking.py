#!/usr/bin/env python3
"""Filtered ranking and top-k retrieval on pose0-syn (multiRelaInnerProductDecoder.rank / top_k) against the chunked torch
formulation of the same questions, timed in one process on the same inputs; prints one JSON line.

  rank   : every test pair (220,608) against all 645 candidates, train + test pairs filtered
  top_k  : the 10 best non-known partners of every (u, r) row (645 x 964)

The torch formulation: per chunk of queries, scores = (z[u] * D[r]) @ z.T, the known pairs' mask gathered from a dense
[R, n, n] bool table (built once, not timed), then compare-and-sum or masked topk.  Parity (the counts, the top-10 ids
and scores) is asserted in the run.  Times: HIP events around `--reps` calls after `--warmup` calls.

    python tools/bench_ranking.py [--reps 20] [--warmup 3] [--chunk 16384]

`--typed` measures per-relation candidate ranges instead, on the homogenised graph of the all-nodes baselines (z holds every
drug and gene: 19,726 rows of 32 features, 964 relations): the three alternating calls, the parities and the options of
`tools/bench_kge_ranking.py --typed`, for multiRelaInnerProductDecoder.rank / top_k.

    python tools/bench_ranking.py --typed [--parent-lib PATH] [--runs 3] [--reps 9] [--markdown PATH]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gripnet_amd import _hip, utils                                      # noqa: E402
from gripnet_amd.decoder import KnownPairs, multiRelaInnerProductDecoder  # noqa: E402
from gripnet_amd.synth import add_pose_test_split, make_pose             # noqa: E402

PEAK_TF = 157.3                                                          # fp32 matrix peak, MI355X


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def typed_mode(args):
    import bench_kge_ranking as kb
    from gripnet_amd.synth import make_rgcn_pose
    dev = torch.device("cuda:0")
    data = make_rgcn_pose("pose0-syn").to(dev)
    n, R, f, n_drug = int(data.n_node), int(data.n_edge_type), args.typed_dim, int(data.n_drug)
    sample, et, table = kb.typed_queries(data, args.queries, dev)
    parent = kb.ParentLibrary(args.parent_lib)
    torch.manual_seed(2024)
    z = torch.randn(n, f, device=dev)
    dec = multiRelaInnerProductDecoder(f, R).to(dev)
    lists = [(data.train_idx, data.train_et)]
    known = KnownPairs(lists, n, R)
    rest = kb.rest_known(lists, sample[0], et, n, n_drug, R)

    def in_parent(fn):
        def call():
            with parent.active():
                return fn()
        return call

    ops = {"rank": lambda **kw: dec.rank(z, sample, et, **kw), "top-10": lambda **kw: dec.top_k(z, sample[0], et, 10, **kw)}
    rows = []
    for run in range(args.runs):
        for op, fn in ops.items():
            with torch.no_grad():
                ms, got = kb.three_way({"a": in_parent(lambda: fn(known=known)), "b": lambda: fn(known=known),
                                        "c": lambda: fn(known=known, candidates=table)}, args.reps, args.warmup)
                assert kb.same_bits(got["a"], got["b"]), (op, "parent and this build differ")
                assert kb.same_bits(got["c"], fn(known=rest)), (op, "ranged and full scan differ")
            rows.append(dict(run=run + 1, model="decoder", side="tail", op=op, **ms))
    _hip.raise_if_index_errors(dev)
    out = {"workload": "pose0-syn homogenised decoder ranking, typed candidates (n {}, {} drugs, R {}, {} features, {} drug-drug "
                       "queries sorted by relation)".format(n, n_drug, R, f, sample.shape[1]),
           "a_is": "the parent commit's build, unranged" if args.parent_lib else "this build, unranged (no parent build given)",
           "results": kb.summarise(rows), "reps": args.reps, "warmup": args.warmup, "runs": args.runs,
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))
    if args.markdown:
        kb.write_typed_markdown(args.markdown, "Decoder ranking and top-10 with per-relation candidate ranges",
                                "tools/bench_ranking.py --typed --runs {} --reps {} --warmup {} --queries {}".format(
                                    args.runs, args.reps, args.warmup, args.queries), out, out["results"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--typed", action="store_true", help="per-relation candidate ranges: parent / unranged / ranged")
    ap.add_argument("--parent-lib", default=None, help="--typed: the parent commit's libgripnet_hip.so for call (a)")
    ap.add_argument("--runs", type=int, default=3, help="--typed: repetitions of the whole measurement")
    ap.add_argument("--queries", type=int, default=2000, help="--typed: drug-drug queries")
    ap.add_argument("--typed-dim", type=int, default=32, help="--typed: features of z")
    ap.add_argument("--markdown", default=None, help="--typed: also write the table here")
    ap.add_argument("--chunk", type=int, default=16384, help="queries per chunk of the torch formulation")
    ap.add_argument("--in-dim", type=int, default=80)
    args = ap.parse_args()
    if args.typed:
        return typed_mode(args)
    dev = torch.device("cuda:0")
    data = add_pose_test_split(make_pose("pose0-syn")).to(dev)
    n, R, f = int(data.n_d_node), int(data.n_dd_edge_type), args.in_dim
    torch.manual_seed(2024)
    z = torch.randn(n, f, device=dev)
    dec = multiRelaInnerProductDecoder(f, R).to(dev)
    lists = [(data.train_idx, data.train_et), (data.test_idx, data.test_et)]
    known = KnownPairs(lists, n, R)
    qi, qt = data.test_idx, data.test_et
    rows_u = torch.arange(n, device=dev).repeat(R)                      # every (u, r) row
    rows_r = torch.arange(R, device=dev).repeat_interleave(n)
    D = dec.weight.detach()

    # the torch formulation's known-pair table: dense [R, n, n] bool (401 MB at pose0-syn), not timed
    dense = torch.zeros(R * n * n, dtype=torch.bool, device=dev)
    for ei, et in lists:
        dense[(et * n + ei[0]) * n + ei[1]] = True
    dense = dense.view(R * n, n)
    cols = torch.arange(n, device=dev)

    def torch_rank():
        g_out, t_out = [], []
        for a in range(0, qi.shape[1], args.chunk):
            u, v, r = qi[0, a:a + args.chunk], qi[1, a:a + args.chunk], qt[a:a + args.chunk]
            s = (z[u] * D[r]) @ z.T
            cand = ~dense[r * n + u] & (cols.unsqueeze(0) != v.unsqueeze(1))
            st = s.gather(1, v.unsqueeze(1))
            g_out.append(((s > st) & cand).sum(1, dtype=torch.int32))
            t_out.append(((s == st) & cand).sum(1, dtype=torch.int32))
        return torch.cat(g_out), torch.cat(t_out)

    def torch_topk():
        s_out, i_out = [], []
        for a in range(0, rows_u.numel(), args.chunk):
            u, r = rows_u[a:a + args.chunk], rows_r[a:a + args.chunk]
            s = ((z[u] * D[r]) @ z.T).masked_fill_(dense[r * n + u], float("-inf"))
            val, idx = s.topk(10, dim=1)
            s_out.append(val)
            i_out.append(idx)
        return torch.cat(s_out), torch.cat(i_out)

    with torch.no_grad():
        t_rank, (greater, ties) = timed(lambda: dec.rank(z, qi, qt, known=known), args.reps, args.warmup)
        t_topk, (scores, ids) = timed(lambda: dec.top_k(z, rows_u, rows_r, 10, known=known), args.reps, args.warmup)
        t_rank_torch, (g_ref, t_ref) = timed(torch_rank, args.reps, args.warmup)
        t_topk_torch, (s_ref, i_ref) = timed(torch_topk, args.reps, args.warmup)
    _hip.raise_if_index_errors(dev)

    # parity: the two formulations round differently (fp32 FMA chains in another order), so near-ties may move a count
    m_ours = utils.ranking_metrics(greater, ties, qt, R)
    m_ref = utils.ranking_metrics(g_ref, t_ref, qt, R)
    same_counts = ((greater == g_ref) & (ties == t_ref)).double().mean().item()
    rank_diff = ((greater.double() + 0.5 * ties.double()) - (g_ref.double() + 0.5 * t_ref.double())).abs().max().item()
    assert same_counts >= 0.999 and rank_diff <= 3, (same_counts, rank_diff)
    assert abs(m_ours["mrr_all"].item() - m_ref["mrr_all"].item()) <= 1e-4 * m_ref["mrr_all"].item()
    same_rows = (ids == i_ref).all(dim=1).double().mean().item()
    assert same_rows >= 0.99, same_rows
    assert torch.allclose(scores, s_ref, rtol=1e-5, atol=1e-5)

    q_rank, q_topk = int(qi.shape[1]), int(rows_u.numel())
    fl_rank, fl_topk = 2.0 * q_rank * n * f, 2.0 * q_topk * n * f
    out = {
        "workload": "pose0-syn filtered ranking (DistMult, in_dim {})".format(f),
        "rank": {"queries": q_rank, "candidates": n, "ms": round(t_rank, 4), "torch_ms": round(t_rank_torch, 4),
                 "speedup": round(t_rank_torch / t_rank, 2), "gflop": round(fl_rank / 1e9, 2),
                 "tflops": round(fl_rank / t_rank / 1e9, 2), "share_of_fp32_matrix_peak": round(fl_rank / t_rank / 1e9 / PEAK_TF, 4),
                 "same_counts": round(same_counts, 6), "max_rank_diff": rank_diff,
                 "mrr": round(m_ours["mrr_all"].item(), 6), "hits@10": round(m_ours["hits@10_all"].item(), 6)},
        "top_k": {"queries": q_topk, "k": 10, "ms": round(t_topk, 4), "torch_ms": round(t_topk_torch, 4),
                  "speedup": round(t_topk_torch / t_topk, 2), "gflop": round(fl_topk / 1e9, 2),
                  "tflops": round(fl_topk / t_topk / 1e9, 2), "share_of_fp32_matrix_peak": round(fl_topk / t_topk / 1e9 / PEAK_TF, 4),
                  "same_rows": round(same_rows, 6)},
        "reps": args.reps, "warmup": args.warmup, "torch_chunk": args.chunk,
        "device": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
