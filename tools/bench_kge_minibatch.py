#!/usr/bin/env python3
"""One mini-batch step of the KGE baselines - draw the candidates, score the positives and the [B, K] block, loss, backward,
Adam - at pose0-syn's homogenised tables (n = 19,726 entities, R = 964 relations, H = 32) with B = 1,024 positives, K in
{8, 256, 1,024} candidates each, temperature 1, the sides alternating from step to step (examples/train_kge.py
--negatives K --adversarial-temperature 1).  Per model, three ways in one process, each on its own copy of the model and its
own torch.optim.Adam, taking turns inside a run (a, b, c, a, b, c, ...) so that a drift of the machine falls on all of them:

  (a) torch   : torch.randint candidates + kge.self_adversarial_loss in torch ops (what --torch-loss keeps)
  (b) hip     : kge.sample_candidates without a filter + kge.negative_sampling_loss (one launch forward, one backward)
  (c) filtered: the same with the two KnownPairs of the training list (tail side keyed (r, head), head side flipped)

and the loss alone on one fixed block of raw scores, forward plus backward: torch ops against the two HIP launches.  Times:
HIP events around every step after `--warmup` steps, `--reps` steps per way, `--runs` repetitions.  Prints one JSON line;
`--markdown PATH` also writes the tables.

    python tools/bench_kge_minibatch.py [--runs 3] [--reps 20] [--warmup 5] [--markdown profiles/r23_kge_minibatch.md]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gripnet_amd import KGEModel, _hip                                   # noqa: E402
from gripnet_amd.decoder import KnownPairs                               # noqa: E402
from gripnet_amd.kge import negative_sampling_loss, sample_candidates, self_adversarial_loss   # noqa: E402
from gripnet_amd.synth import make_rgcn_pose                             # noqa: E402

MODELS = ("TransE", "DistMult", "ComplEx", "RotatE")
MODES = ("tail-batch", "head-batch")
SIDES = {"tail-batch": "tail", "head-batch": "head"}
T = 1.0


def timed(fns, reps, warmup):
    """Milliseconds per call of every function of `fns` (name -> callable(i)), the functions taking turns."""
    for i in range(warmup):
        for fn in fns.values():
            fn(i)
    torch.cuda.synchronize()
    events = {key: [] for key in fns}
    for i in range(reps):
        for key, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(warmup + i)
            b.record()
            events[key].append((a, b))
    torch.cuda.synchronize()
    return {key: sum(a.elapsed_time(b) for a, b in pairs) / reps for key, pairs in events.items()}


def measure(name, n, R, H, B, K, data, known, dev, reps, warmup):
    torch.manual_seed(2024)
    first = KGEModel(name, n, R, H, 12.0).to(dev)
    models = {"torch": first, "hip": KGEModel(name, n, R, H, 12.0).to(dev), "filtered": KGEModel(name, n, R, H, 12.0).to(dev)}
    for m in models.values():
        m.load_state_dict(first.state_dict())
    optims = {key: torch.optim.Adam(m.parameters(), lr=0.01) for key, m in models.items()}
    gen = torch.Generator(device=dev).manual_seed(7)
    batches = []
    for _ in range(4):                                                  # the positives of four steps, reused in turn
        pick = torch.randperm(data.train_idx.shape[1], generator=gen, device=dev)[:B]
        batches.append((data.train_idx[:, pick].contiguous(), data.train_et[pick].contiguous()))

    def step(key, i):
        model, mode = models[key], MODES[i % 2]
        positive, et = batches[i % len(batches)]
        optims[key].zero_grad()
        if key == "torch":
            candidates = torch.randint(0, n, (B, K), generator=gen, device=dev)
            loss = self_adversarial_loss(model.score(positive, et), model.score((positive, candidates), et, mode=mode), T)
        else:
            candidates = sample_candidates(positive, et, K, n, side=SIDES[mode], known=known[SIDES[mode]] if key == "filtered" else None,
                                           seed=i)
            loss = negative_sampling_loss(model.score(positive, et), model.score((positive, candidates), et, mode=mode), T)
        loss.backward()
        optims[key].step()

    ms = timed({key: (lambda i, key=key: step(key, i)) for key in models}, reps, warmup)
    _hip.raise_if_index_errors(dev)

    # the loss alone, on one block of raw scores
    with torch.no_grad():
        positive, et = batches[0]
        pos = first.score(positive, et)
        neg = first.score((positive, torch.randint(0, n, (B, K), generator=gen, device=dev)), et, mode="tail-batch")

    def alone(fn):
        p, q = pos.clone().requires_grad_(True), neg.clone().requires_grad_(True)
        loss = fn(p, q, T)
        loss.backward()
        return loss.detach(), p.grad, q.grad

    ours, theirs = alone(negative_sampling_loss), alone(self_adversarial_loss)
    assert abs(float(ours[0]) - float(theirs[0])) <= 1e-5 * abs(float(theirs[0])), (name, K, float(ours[0]), float(theirs[0]))
    for g, ref in zip(ours[1:], theirs[1:]):
        assert float((g - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), (name, K)
    loss_ms = timed({"torch": lambda i: alone(self_adversarial_loss), "hip": lambda i: alone(negative_sampling_loss)}, reps, warmup)
    return {"model": name, "B": B, "K": K, "torch_ms": round(ms["torch"], 4), "hip_ms": round(ms["hip"], 4),
            "filtered_ms": round(ms["filtered"], 4), "torch_over_hip": round(ms["torch"] / ms["hip"], 2),
            "filtered_over_hip": round(ms["filtered"] / ms["hip"], 2), "loss_torch_ms": round(loss_ms["torch"], 4),
            "loss_hip_ms": round(loss_ms["hip"], 4)}


ROW = ("| {run} | {model} | {B} | {K} | {torch_ms:.3f} | {hip_ms:.3f} | {filtered_ms:.3f} | {torch_over_hip:.2f} | {filtered_over_hip:.2f} | "
       "{loss_torch_ms:.3f} | {loss_hip_ms:.3f} |\n")
HEAD = ("| run | model | B | K | (a) torch step ms | (b) hip step ms | (c) filtered step ms | (a) / (b) | (c) / (b) | loss alone, torch ms | "
        "loss alone, hip ms |\n|---|---|---|---|---|---|---|---|---|---|---|\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--negatives", type=int, nargs="*", default=[8, 256, 1024])
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    data = make_rgcn_pose("pose0-syn").to(dev)
    n, R, H = int(data.n_node), int(data.n_edge_type), args.hidden
    known = {"tail": KnownPairs([(data.train_idx, data.train_et)], n, R),
             "head": KnownPairs([(data.train_idx.flip(0), data.train_et)], n, R)}
    results = []
    for run in range(args.runs):
        for k in args.negatives:
            for name in MODELS:
                results.append(dict(measure(name, n, R, H, args.batch, k, data, known, dev, args.reps, args.warmup), run=run + 1))
    out = {"workload": "pose0-syn homogenised tables (n {}, R {}, H {})".format(n, R, H), "results": results, "reps": args.reps,
           "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))
    if args.markdown:
        with open(args.markdown, "w") as fh:
            fh.write("# KGE baselines: one mini-batch step, three ways\n\n")
            fh.write("`tools/bench_kge_minibatch.py --runs {} --reps {} --warmup {}` on {}: {}.  Milliseconds per step (draw, two "
                     "scores, loss at temperature 1, backward, torch.optim.Adam; the sides alternate), HIP events, the three ways "
                     "taking turns inside a run; and of the loss alone on one block of raw scores, forward plus backward.\n\n".format(
                         args.runs, args.reps, args.warmup, out["device"], out["workload"]))
            fh.write(HEAD)
            for r in results:
                fh.write(ROW.format(**r))


if __name__ == "__main__":
    main()
