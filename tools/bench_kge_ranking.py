#!/usr/bin/env python3
"""Filtered ranking and top-k of the KGE baselines (KGEModel.rank / top_k) at pose0-syn's homogenised size (n = 19,726
entities, R = 964 relations, H = 32) against a chunked torch formulation of the same questions, timed in one process on the
same inputs and the same GPU.  Per model (TransE, DistMult, ComplEx, RotatE) and side (tail, head):

  rank   : a fixed sample of `--queries` triples of the list against all n candidates, the list's pairs filtered
  top_k  : the 10 best non-known partners of the same sample's (fixed entity, relation) queries

The torch formulation, per chunk of queries: TransE and RotatE broadcast the [chunk, n, D] block of differences (the chunk
is sized so that the block takes `--block-mb`), take the norm and sum; DistMult and ComplEx form the query rows and multiply
with the table's transpose; the known pairs' mask comes from a searchsorted over the sorted keys (the dense [R, n, n] table
of tools/bench_ranking.py would take 375 GB here); then compare-and-sum or masked topk.  Parity of the counts and of the
top-10 ids is asserted in the run.  Times: HIP events around `--reps` calls after `--warmup` calls; `--runs` repetitions of
the whole measurement.  Prints one JSON line; `--markdown PATH` also writes the runs as a table.

    python tools/bench_kge_ranking.py [--runs 3] [--reps 5] [--warmup 2] [--queries 2000] [--markdown profiles/r18_kge_ranking.md]

`--typed` measures per-relation candidate ranges instead (the `candidates` argument): `--queries` drug-drug triples of the
list, sorted by relation, ranked and top-10'd as three calls that alternate inside one run,
  (a) the unranged call of the library given with `--parent-lib` (the parent commit's build, loaded into the same process;
      without the option: this build's unranged call a second time),
  (b) this build's unranged call,
  (c) this build's call with candidates = [0, n_drug) for the drug-drug relations.
(a) and (b) must agree bit for bit, and (c) must equal the unranged call whose KnownPairs additionally holds every
(relation, fixed entity, gene) - both asserted in the run.  Median of `--reps` alternating rounds per run.

    python tools/bench_kge_ranking.py --typed [--parent-lib PATH] [--runs 3] [--reps 9] [--markdown PATH]
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gripnet_amd import KGEModel, _hip                                   # noqa: E402
from gripnet_amd.decoder import KnownPairs                               # noqa: E402
from gripnet_amd.kge import PI                                           # noqa: E402
from gripnet_amd.synth import make_rgcn_pose                             # noqa: E402

MODELS = ("TransE", "DistMult", "ComplEx", "RotatE")
SIDES = ("tail", "head")


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


class ParentLibrary:
    """Another build of the library (the parent commit's) in this process: inside `with parent.active():` the package's
    calls of the ranged entry points go to that build's unranged ones (the table must be None)."""

    def __init__(self, path):
        self.path, self.lib, self.current = path, ctypes.CDLL(path) if path else None, _hip.load()

    def __getattr__(self, name):
        if "_ranged" not in name:
            return getattr(self.current, name)
        old = name.replace("_ranged", "")
        fn = getattr(self.lib, old)
        fn.restype, fn.argtypes = _hip.SIGNATURES[old]

        def call(*args):
            assert args[-1] is None, "the parent build takes no candidate table"
            return fn(*args[:-1])
        return call

    @contextlib.contextmanager
    def active(self):
        if self.lib is None:
            yield
            return
        _hip._lib = self
        try:
            yield
        finally:
            _hip._lib = self.current


def three_way(calls, reps, warmup):
    """Median milliseconds of each of `calls` (name -> function), timed one call at a time in alternating rounds; the last
    outputs."""
    out, times = {}, {k: [] for k in calls}
    for _ in range(warmup):
        for k, fn in calls.items():
            out[k] = fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out[k] = fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}, out


def typed_queries(data, queries, dev):
    """(sample [2, Q], et [Q]) drug-drug triples of the list sorted by relation, and the candidate table."""
    from gripnet_amd.utils import candidate_ranges
    n, R, n_drug = int(data.n_node), int(data.n_edge_type), int(data.n_drug)
    drug_edges = int(data.train_range[-2][0])
    pick = torch.randperm(drug_edges, generator=torch.Generator().manual_seed(7))[:queries].to(dev)
    pick = pick[torch.sort(data.train_et[pick], stable=True).indices]
    table = candidate_ranges(R, n, [(0, R - 2, 0, n_drug), (R - 2, R - 1, n_drug, n)], device=dev)
    return data.train_idx[:, pick].contiguous(), data.train_et[pick].contiguous(), table


def rest_known(lists, fixed, et, n, n_drug, R):
    """KnownPairs of `lists` and every (relation, fixed entity, gene) of the queries: the unranged call's filter that
    leaves the drugs."""
    genes = torch.arange(n_drug, n, device=fixed.device)
    rows = torch.stack([fixed.repeat_interleave(genes.numel()), genes.repeat(fixed.numel())])
    return KnownPairs(lists + [(rows, et.repeat_interleave(genes.numel()))], n, R)


def same_bits(x, y):
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(x, y))


def write_typed_markdown(path, title, command, out, rows):
    """rows: dicts with what / side / op and per run a_ms, b_ms, c_ms."""
    with open(path, "w") as fh:
        fh.write("# {}\n\n`{}` on {}: {}.\n".format(title, command, out["device"], out["workload"]))
        fh.write("Milliseconds per call (HIP events, median of {} alternating rounds), {} runs.  (a) {}; (b) this build, "
                 "unranged; (c) this build, candidates = the drugs.  Parity is asserted in the run: (a) == (b) bit for bit, "
                 "(c) == the unranged call whose KnownPairs also holds every gene.\n\n".format(out["reps"], out["runs"], out["a_is"]))
        fh.write("| model | side | call | (a) runs | (b) runs | (c) runs | (a) spread | (b) - (a) medians | (b) / (c) |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            fh.write("| {} | {} | {} | {} | {} | {} | {:.3f} | {:+.3f} | {:.2f} |\n".format(
                r["model"], r["side"], r["op"], " / ".join("{:.3f}".format(x) for x in r["a_ms"]),
                " / ".join("{:.3f}".format(x) for x in r["b_ms"]), " / ".join("{:.3f}".format(x) for x in r["c_ms"]),
                r["a_spread"], r["b_minus_a"], r["b_over_c"]))


def summarise(rows):
    """Per (model, side, op): the runs' figures side by side, (a)'s spread, and the two conditions."""
    merged = {}
    for r in rows:
        m = merged.setdefault((r["model"], r["side"], r["op"]), {"model": r["model"], "side": r["side"], "op": r["op"],
                                                                "a_ms": [], "b_ms": [], "c_ms": []})
        for k in ("a", "b", "c"):
            m[k + "_ms"].append(round(r[k], 4))
    for m in merged.values():
        med = {k: sorted(m[k + "_ms"])[len(m[k + "_ms"]) // 2] for k in ("a", "b", "c")}
        m["a_spread"] = round(max(m["a_ms"]) - min(m["a_ms"]), 4)
        m["b_minus_a"] = round(med["b"] - med["a"], 4)
        m["b_over_c"] = round(med["b"] / med["c"], 3)
        m["b_within_spread_of_a"] = bool(med["b"] - med["a"] <= m["a_spread"])
        m["c_not_slower_than_b"] = bool(med["c"] <= med["b"])
    return list(merged.values())


def typed_mode(args):
    dev = torch.device("cuda:0")
    data = make_rgcn_pose("pose0-syn").to(dev)
    n, R, H, n_drug = int(data.n_node), int(data.n_edge_type), args.hidden, int(data.n_drug)
    sample, et, table = typed_queries(data, args.queries, dev)
    parent = ParentLibrary(args.parent_lib)
    lists = {"tail": [(data.train_idx, data.train_et)], "head": [(data.train_idx.flip(0), data.train_et)]}
    rows = []
    for side in SIDES:
        fixed = sample[0] if side == "tail" else sample[1]
        known = KnownPairs(lists[side], n, R)
        rest = rest_known(lists[side], fixed, et, n, n_drug, R)
        for run in range(args.runs):
            for name in MODELS:
                torch.manual_seed(2024)
                model = KGEModel(name, n, R, H, 12.0).to(dev)

                def in_parent(fn):
                    def call():
                        with parent.active():
                            return fn()
                    return call

                ops = {"rank": lambda **kw: model.rank(sample, et, side=side, **kw),
                       "top-10": lambda **kw: model.top_k(fixed, et, 10, side=side, **kw)}
                for op, fn in ops.items():
                    with torch.no_grad():
                        ms, got = three_way({"a": in_parent(lambda: fn(known=known)), "b": lambda: fn(known=known),
                                             "c": lambda: fn(known=known, candidates=table)}, args.reps, args.warmup)
                        assert same_bits(got["a"], got["b"]), (name, side, op, "parent and this build differ")
                        assert same_bits(got["c"], fn(known=rest)), (name, side, op, "ranged and full scan differ")
                    rows.append(dict(run=run + 1, model=name, side=side, op=op, **ms))
        _hip.raise_if_index_errors(dev)
        del rest
    out = {"workload": "pose0-syn homogenised KGE ranking, typed candidates (n {}, {} drugs, R {}, H {}, {} drug-drug queries "
                       "sorted by relation)".format(n, n_drug, R, H, sample.shape[1]),
           "a_is": "the parent commit's build, unranged" if args.parent_lib else "this build, unranged (no parent build given)",
           "results": summarise(rows), "reps": args.reps, "warmup": args.warmup, "runs": args.runs,
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))
    if args.markdown:
        write_typed_markdown(args.markdown, "KGE ranking and top-10 with per-relation candidate ranges",
                             "tools/bench_kge_ranking.py --typed --runs {} --reps {} --warmup {} --queries {}".format(
                                 args.runs, args.reps, args.warmup, args.queries), out, out["results"])


def torch_scores(model, side, ent, rel, fixed, r, gamma, divisor):
    """[chunk, n] raw scores of every candidate, fp32, in the reference's operation order."""
    H = rel.shape[1] // 2 if model == "ComplEx" else rel.shape[1]
    f, w = ent[fixed], rel[r]
    if model == "TransE":
        diff = (f + w).unsqueeze(1) - ent.unsqueeze(0) if side == "tail" else (ent.unsqueeze(0) + w.unsqueeze(1)) - f.unsqueeze(1)
        return gamma - diff.abs().sum(-1)
    if model == "DistMult":
        return (f * w) @ ent.T
    fr, fi = f[:, :H], f[:, H:]
    if model == "ComplEx":
        wr, wi = w[:, :H], w[:, H:]
        q = (fr * wr - fi * wi, fr * wi + fi * wr) if side == "tail" else (wr * fr + wi * fi, wr * fi - wi * fr)
        return torch.cat(q, 1) @ ent.T
    theta = w / divisor
    c, s = torch.cos(theta), torch.sin(theta)
    er, ei = ent[:, :H].unsqueeze(0), ent[:, H:].unsqueeze(0)
    if side == "tail":
        a = (fr * c - fi * s).unsqueeze(1) - er
        b = (fr * s + fi * c).unsqueeze(1) - ei
    else:
        c, s = c.unsqueeze(1), s.unsqueeze(1)
        a = (er * c - ei * s) - fr.unsqueeze(1)
        b = (er * s + ei * c) - fi.unsqueeze(1)
    return gamma - torch.sqrt(a * a + b * b).sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--block-mb", type=int, default=1024, help="size of the torch formulation's [chunk, n, D] block")
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--typed", action="store_true", help="per-relation candidate ranges: parent / unranged / ranged")
    ap.add_argument("--parent-lib", default=None, help="--typed: the parent commit's libgripnet_hip.so for call (a)")
    args = ap.parse_args()
    if args.typed:
        return typed_mode(args)
    dev = torch.device("cuda:0")
    data = make_rgcn_pose("pose0-syn").to(dev)
    n, R, H = int(data.n_node), int(data.n_edge_type), args.hidden
    ei, et_all = data.train_idx, data.train_et
    pick = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(7))[:args.queries].to(dev)
    sample, et = ei[:, pick].contiguous(), et_all[pick].contiguous()
    cols = torch.arange(n, device=dev)
    known, keys = {}, {}
    for side in SIDES:
        lists = [(ei, et_all)] if side == "tail" else [(ei.flip(0), et_all)]
        known[side] = KnownPairs(lists, n, R)
        keys[side] = torch.sort((lists[0][1] * n + lists[0][0][0]) * n + lists[0][0][1]).values

    def mask_of(side, fixed, r):
        want = ((r * n + fixed) * n).unsqueeze(1) + cols.unsqueeze(0)
        k = keys[side]
        return k[torch.searchsorted(k, want).clamp_(max=k.numel() - 1)] == want

    results = []
    for run in range(args.runs):
        for name in MODELS:
            torch.manual_seed(2024)
            model = KGEModel(name, n, R, H, 12.0).to(dev)
            ent, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
            gamma, divisor = model.gamma.item(), model.embedding_range.item() / PI
            chunk = max(1, (args.block_mb << 20) // (n * ent.shape[1] * 4))
            for side in SIDES:
                fixed, truth = (sample[0], sample[1]) if side == "tail" else (sample[1], sample[0])

                def torch_rank():
                    g_out, t_out = [], []
                    for a in range(0, fixed.numel(), chunk):
                        f, v, r = fixed[a:a + chunk], truth[a:a + chunk], et[a:a + chunk]
                        s = torch_scores(name, side, ent, rel, f, r, gamma, divisor)
                        cand = ~mask_of(side, f, r) & (cols.unsqueeze(0) != v.unsqueeze(1))
                        st = s.gather(1, v.unsqueeze(1))
                        g_out.append(((s > st) & cand).sum(1, dtype=torch.int32))
                        t_out.append(((s == st) & cand).sum(1, dtype=torch.int32))
                    return torch.cat(g_out), torch.cat(t_out)

                def torch_topk():
                    s_out, i_out = [], []
                    for a in range(0, fixed.numel(), chunk):
                        f, r = fixed[a:a + chunk], et[a:a + chunk]
                        s = torch_scores(name, side, ent, rel, f, r, gamma, divisor).masked_fill_(mask_of(side, f, r), float("-inf"))
                        val, idx = s.topk(10, dim=1)
                        s_out.append(val)
                        i_out.append(idx)
                    return torch.cat(s_out), torch.cat(i_out)

                with torch.no_grad():
                    t_rank, (greater, ties) = timed(lambda: model.rank(sample, et, side=side, known=known[side]), args.reps, args.warmup)
                    t_topk, (scores, ids) = timed(lambda: model.top_k(fixed, et, 10, side=side, known=known[side]), args.reps, args.warmup)
                    t_rank_torch, (g_ref, t_ref) = timed(torch_rank, args.reps, args.warmup)
                    t_topk_torch, (s_ref, i_ref) = timed(torch_topk, args.reps, args.warmup)
                _hip.raise_if_index_errors(dev)
                # parity: the two formulations sum in another order; among 19,726 candidates a few lie within fp32's error of
                # the true score, so a count moves by a place or two in a share of the queries (the bounded tests decide those)
                same_counts = ((greater == g_ref) & (ties == t_ref)).double().mean().item()
                rank_diff = ((greater.double() + 0.5 * ties.double()) - (g_ref.double() + 0.5 * t_ref.double())).abs().max().item()
                same_rows = (ids == i_ref).all(dim=1).double().mean().item()
                assert same_counts >= 0.5 and rank_diff <= 5, (name, side, same_counts, rank_diff)
                assert same_rows >= 0.95, (name, side, same_rows)
                assert torch.allclose(scores, s_ref, rtol=1e-4, atol=1e-4), (name, side)
                results.append({"run": run + 1, "model": name, "side": side, "queries": int(fixed.numel()), "torch_chunk": chunk,
                                "rank_ms": round(t_rank, 4), "rank_torch_ms": round(t_rank_torch, 4),
                                "rank_speedup": round(t_rank_torch / t_rank, 2),
                                "topk_ms": round(t_topk, 4), "topk_torch_ms": round(t_topk_torch, 4),
                                "topk_speedup": round(t_topk_torch / t_topk, 2),
                                "same_counts": round(same_counts, 6), "max_rank_diff": rank_diff, "same_rows": round(same_rows, 6)})
    out = {"workload": "pose0-syn homogenised KGE ranking (n {}, R {}, H {})".format(n, R, H), "results": results,
           "reps": args.reps, "warmup": args.warmup, "runs": args.runs, "block_mb": args.block_mb,
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))
    if args.markdown:
        with open(args.markdown, "w") as fh:
            fh.write("# KGE filtered ranking and top-k against the chunked torch formulation\n\n")
            fh.write("`tools/bench_kge_ranking.py --runs {} --reps {} --warmup {} --queries {} --block-mb {}` on {}: {}.\n"
                     "Milliseconds per call (HIP events), {} queries against {} candidates; the torch figures are from the same "
                     "process and inputs.\n\n".format(args.runs, args.reps, args.warmup, args.queries, args.block_mb, out["device"],
                                                      out["workload"], args.queries, n))
            fh.write("| run | model | side | rank ms | torch rank ms | ratio | top-10 ms | torch top-10 ms | ratio | same counts | same top-10 rows |\n")
            fh.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in results:
                fh.write("| {run} | {model} | {side} | {rank_ms:.3f} | {rank_torch_ms:.3f} | {rank_speedup:.2f} | {topk_ms:.3f} | "
                         "{topk_torch_ms:.3f} | {topk_speedup:.2f} | {same_counts:.4f} | {same_rows:.4f} |\n".format(**r))


if __name__ == "__main__":
    main()
