#!/usr/bin/env python3
"""K negatives per positive for the KGE baselines (KGEModel's 'tail-batch' / 'head-batch' modes) at pose0-syn's homogenised
size (n = 19,726 entities, R = 964 relations, H = 32) with B = 1,024 positives and K = 256 candidates each - the batch
shapes of the code base the class comes from.  Per model (TransE, DistMult, ComplEx, RotatE) and side (tail, head), one
forward (log-sigmoid scores [B, K]) plus one backward (both tables' gradients), timed three ways in one process on the same
inputs and the same GPU:

  (a) batch   : model((positive, negatives), et, mode=...) - gn_kge_batch_forward_f32 / gn_kge_batch_backward_f32
  (b) list    : the expansion into three int64 lists of B * K entries (repeat_interleave / reshape, inside the timed
                window: a caller pays it) through model(sample, et) - gn_kge_forward_f32 / gn_kge_backward_f32
  (c) torch   : the broadcast torch formulation ([B, 1, D] query rows against [B, K, D] gathered candidates) with autograd

The three take turns inside a run (a, b, c, a, b, c, ...), so that a drift of the machine falls on all of them.  Parity is
asserted in the run: (a) equals (b) bit for bit in the scores, both gradients agree with (b) and (c) to 1e-4 of the
gradient's largest entry.  Times: HIP events around `--reps` forward + backward pairs after `--warmup` pairs; `--runs`
repetitions.  `--extra-k` adds one line per K (tail side) at the same B.  Prints one JSON line; `--markdown PATH` also
writes the tables.

    python tools/bench_kge_negatives.py [--runs 3] [--reps 10] [--warmup 3] [--markdown profiles/r22_kge_negatives.md]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gripnet_amd import KGEModel, _hip                                   # noqa: E402
from gripnet_amd.kge import PI                                           # noqa: E402
from gripnet_amd.synth import make_rgcn_pose                             # noqa: E402

MODELS = ("TransE", "DistMult", "ComplEx", "RotatE")
SIDES = ("tail", "head")
MODES = {"tail": "tail-batch", "head": "head-batch"}


def torch_scores(model, side, ent, rel, fixed, et, negatives, gamma, divisor):
    """logsigmoid of the [B, K] scores in the reference's operation order (:189-235), the candidates broadcast against the
    query rows."""
    f, w, c = ent[fixed].unsqueeze(1), rel[et].unsqueeze(1), ent[negatives]
    head, tail = (f, c) if side == "tail" else (c, f)
    H = rel.shape[1] // 2 if model == "ComplEx" else rel.shape[1]
    if model == "TransE":
        s = gamma - torch.norm(head + w - tail, p=1, dim=2)
    elif model == "DistMult":
        s = (head * w * tail).sum(dim=2)
    else:
        hr, hi, tr, ti = head[..., :H], head[..., H:], tail[..., :H], tail[..., H:]
        if model == "ComplEx":
            wr, wi = w[..., :H], w[..., H:]
            s = ((hr * wr - hi * wi) * tr + (hr * wi + hi * wr) * ti).sum(dim=2)
        else:
            theta = w / divisor
            wr, wi = torch.cos(theta), torch.sin(theta)
            a, b = (hr * wr - hi * wi) - tr, (hr * wi + hi * wr) - ti
            s = gamma - torch.stack([a, b], dim=0).norm(dim=0).sum(dim=2)
    return F.logsigmoid(s)


def measure(name, side, n, R, H, B, K, data, dev, reps, warmup):
    """Milliseconds per forward + backward of the three ways, parity asserted."""
    torch.manual_seed(2024)
    model = KGEModel(name, n, R, H, 12.0).to(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    pick = torch.randperm(data.train_idx.shape[1], generator=gen, device=dev)[:B]
    positive, et = data.train_idx[:, pick].contiguous(), data.train_et[pick].contiguous()
    negatives = torch.randint(0, n, (B, K), generator=gen, device=dev)
    up = torch.linspace(-1.0, 1.0, B * K, device=dev).view(B, K)
    gamma, divisor = model.gamma.item(), model.embedding_range.item() / PI
    params = (model.entity_embedding, model.relation_embedding)
    fixed = positive[0] if side == "tail" else positive[1]

    def finish(y):
        for p in params:
            p.grad = None
        y.backward(up)
        return y.detach(), params[0].grad, params[1].grad

    def batch():
        return finish(model((positive, negatives), et, mode=MODES[side]))

    def expanded():
        flat = negatives.reshape(-1)
        rep = fixed.repeat_interleave(K)
        sample = torch.stack([rep, flat]) if side == "tail" else torch.stack([flat, rep])
        return finish(model(sample, et.repeat_interleave(K)).view(B, K))

    def broadcast():
        return finish(torch_scores(name, side, params[0], params[1], fixed, et, negatives, gamma, divisor))

    ways = (("batch", batch), ("list", expanded), ("torch", broadcast))
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
    assert torch.equal(outs["batch"][0], outs["list"][0]), (name, side, "scores differ from the list kernel's")
    for other in ("list", "torch"):
        assert torch.allclose(outs["batch"][0], outs[other][0], rtol=1e-4, atol=1e-4), (name, side, other)
        for g, ref in zip(outs["batch"][1:], outs[other][1:]):
            assert float((g - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), (name, side, other)
    ms = {key: sum(a.elapsed_time(b) for a, b in pairs) / reps for key, pairs in events.items()}
    return {"model": name, "side": side, "B": B, "K": K, "batch_ms": round(ms["batch"], 4), "list_ms": round(ms["list"], 4),
            "torch_ms": round(ms["torch"], 4), "list_over_batch": round(ms["list"] / ms["batch"], 2),
            "torch_over_batch": round(ms["torch"] / ms["batch"], 2)}


ROW = "| {run} | {model} | {side} | {B} | {K} | {batch_ms:.3f} | {list_ms:.3f} | {torch_ms:.3f} | {list_over_batch:.2f} | {torch_over_batch:.2f} |\n"
HEAD = ("| run | model | side | B | K | (a) batch ms | (b) list ms | (c) torch ms | (b) / (a) | (c) / (a) |\n"
        "|---|---|---|---|---|---|---|---|---|---|\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--negatives", type=int, default=256)
    ap.add_argument("--extra-k", type=int, nargs="*", default=[8, 1024])
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    data = make_rgcn_pose("pose0-syn").to(dev)
    n, R, H = int(data.n_node), int(data.n_edge_type), args.hidden
    results, extra = [], []
    for run in range(args.runs):
        for name in MODELS:
            for side in SIDES:
                results.append(dict(measure(name, side, n, R, H, args.batch, args.negatives, data, dev, args.reps, args.warmup), run=run + 1))
    for k in args.extra_k:
        for name in MODELS:
            extra.append(dict(measure(name, "tail", n, R, H, args.batch, k, data, dev, args.reps, args.warmup), run=1))
    out = {"workload": "pose0-syn homogenised tables (n {}, R {}, H {})".format(n, R, H), "results": results, "extra_k": extra,
           "reps": args.reps, "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))
    if args.markdown:
        with open(args.markdown, "w") as fh:
            fh.write("# KGE baselines: K negatives per positive, three ways\n\n")
            fh.write("`tools/bench_kge_negatives.py --runs {} --reps {} --warmup {}` on {}: {}.  Milliseconds per forward "
                     "(log-sigmoid scores [B, K]) plus backward (both tables' gradients), HIP events, the three ways taking "
                     "turns inside a run.\n\n".format(args.runs, args.reps, args.warmup, out["device"], out["workload"]))
            fh.write(HEAD)
            for r in results:
                fh.write(ROW.format(**r))
            if extra:
                fh.write("\nOther K at the same B (tail side, one run):\n\n" + HEAD)
                for r in extra:
                    fh.write(ROW.format(**r))


if __name__ == "__main__":
    main()
