#!/usr/bin/env python3
"""Shared candidate lists for the KGE baselines (KGEModel's 'tail-shared' / 'head-shared' modes) against the candidate-block
modes they replace, at pose0-syn's homogenised size (n = 19,726 entities, R = 964 relations, H = 32) with B = 1,024
positives, K in {8, 256, 1,024} candidates per list and G in {1, 8, 64} lists.  Per model (TransE, DistMult, ComplEx, RotatE)
and side (tail, head), one forward (log-sigmoid scores [B, K]) plus one backward (both tables' gradients), timed three ways in
one process on the same inputs, the same build and the same GPU:

  (a) shared  : model((positive, lists), et, mode="tail-shared" / "head-shared") with lists [G, K]
                - gn_kge_shared_forward_f32 / gn_kge_shared_backward_f32
  (b) block   : model((positive, block), et, mode="tail-batch" / "head-batch") with the same lists expanded to [B, K]
                (the expansion is made once, outside the timed window) - gn_kge_batch_forward_f32 / gn_kge_batch_backward_f32
  (c) torch   : the broadcast torch formulation ([B, 1, D] query rows against the [B, K, D] gathered block) with autograd

The three take turns inside a run (a, b, c, a, b, c, ...), so that a drift of the machine falls on all of them.  Parity is
asserted in the run: the scores of (a) agree with (b) and (c) to 1e-4, both gradients to 1e-4 of the gradient's largest entry.
Times: HIP events around `--reps` forward + backward pairs after `--warmup` pairs; `--runs` repetitions.  Prints one JSON line;
`--markdown PATH` also writes every row of every run as a table.

    python tools/bench_kge_shared.py [--runs 3] [--reps 5] [--warmup 2] [--markdown profiles/r28_kge_shared.md]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_kge_negatives import MODELS, SIDES, torch_scores              # noqa: E402
from gripnet_amd import KGEModel, _hip                                   # noqa: E402
from gripnet_amd.kge import PI, sample_shared_candidates                 # noqa: E402
from gripnet_amd.synth import make_rgcn_pose                             # noqa: E402

SHARED = {"tail": "tail-shared", "head": "head-shared"}
BLOCK = {"tail": "tail-batch", "head": "head-batch"}


def measure(name, side, n, R, H, B, G, K, data, dev, reps, warmup):
    """Milliseconds per forward + backward of the three ways, parity asserted."""
    torch.manual_seed(2024)
    model = KGEModel(name, n, R, H, 12.0).to(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    pick = torch.randperm(data.train_idx.shape[1], generator=gen, device=dev)[:B]
    positive, et = data.train_idx[:, pick].contiguous(), data.train_et[pick].contiguous()
    lists = sample_shared_candidates(G, K, n, seed=7, device=dev)
    block = lists.repeat_interleave(B // G, dim=0).contiguous()
    up = torch.linspace(-1.0, 1.0, B * K, device=dev).view(B, K)
    gamma, divisor = model.gamma.item(), model.embedding_range.item() / PI
    params = (model.entity_embedding, model.relation_embedding)
    fixed = positive[0] if side == "tail" else positive[1]

    def finish(y):
        for p in params:
            p.grad = None
        y.backward(up)
        return y.detach(), params[0].grad, params[1].grad

    def shared():
        return finish(model((positive, lists), et, mode=SHARED[side]))

    def blocked():
        return finish(model((positive, block), et, mode=BLOCK[side]))

    def broadcast():
        return finish(torch_scores(name, side, params[0], params[1], fixed, et, block, gamma, divisor))

    ways = (("shared", shared), ("block", blocked), ("torch", broadcast))
    outs = {}
    for _ in range(warmup):
        for key, fn in ways:
            outs[key] = [t.clone() for t in fn()]
    torch.cuda.synchronize()
    events = {key: [] for key, _ in ways}
    for _ in range(reps):
        for key, fn in ways:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events[key].append((a, b))
    torch.cuda.synchronize()
    _hip.raise_if_index_errors(dev)
    for other in ("block", "torch"):
        assert torch.allclose(outs["shared"][0], outs[other][0], rtol=1e-4, atol=1e-4), (name, side, G, K, other)
        for g, ref in zip(outs["shared"][1:], outs[other][1:]):
            assert float((g - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), (name, side, G, K, other)
    ms = {key: sum(a.elapsed_time(b) for a, b in pairs) / reps for key, pairs in events.items()}
    return {"model": name, "side": side, "B": B, "G": G, "K": K, "shared_ms": round(ms["shared"], 4), "block_ms": round(ms["block"], 4),
            "torch_ms": round(ms["torch"], 4), "block_over_shared": round(ms["block"] / ms["shared"], 2),
            "torch_over_shared": round(ms["torch"] / ms["shared"], 2)}


ROW = "| {run} | {model} | {side} | {B} | {G} | {K} | {shared_ms:.3f} | {block_ms:.3f} | {torch_ms:.3f} | {block_over_shared:.2f} | {torch_over_shared:.2f} |\n"
HEAD = ("| run | model | side | B | G | K | (a) shared ms | (b) block ms | (c) torch ms | (b) / (a) | (c) / (a) |\n"
        "|---|---|---|---|---|---|---|---|---|---|---|\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--negatives", type=int, nargs="*", default=[8, 256, 1024])
    ap.add_argument("--lists", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--models", nargs="*", default=list(MODELS), choices=MODELS)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    data = make_rgcn_pose("pose0-syn").to(dev)
    n, R, H = int(data.n_node), int(data.n_edge_type), args.hidden
    results = []
    for run in range(args.runs):
        for name in args.models:
            for side in SIDES:
                for K in args.negatives:
                    for G in args.lists:
                        results.append(dict(measure(name, side, n, R, H, args.batch, G, K, data, dev, args.reps, args.warmup), run=run + 1))
                        print(ROW.format(**results[-1]), end="", file=sys.stderr, flush=True)
    out = {"workload": "pose0-syn homogenised tables (n {}, R {}, H {})".format(n, R, H), "results": results,
           "reps": args.reps, "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))
    if args.markdown:
        with open(args.markdown, "w") as fh:
            fh.write("# KGE baselines: shared candidate lists against candidate blocks and torch\n\n")
            fh.write("`tools/bench_kge_shared.py --runs {} --reps {} --warmup {}` on {}: {}.  Milliseconds per forward "
                     "(log-sigmoid scores [B, K]) plus backward (both tables' gradients), HIP events, the three ways taking "
                     "turns inside a run.  (a) `tail-shared` / `head-shared` on G lists of K candidates; (b) `tail-batch` / "
                     "`head-batch` on the same lists expanded to [B, K]; (c) the broadcast torch formulation on that block.\n\n".format(
                         args.runs, args.reps, args.warmup, out["device"], out["workload"]))
            fh.write(HEAD)
            for r in results:
                fh.write(ROW.format(**r))


if __name__ == "__main__":
    main()
