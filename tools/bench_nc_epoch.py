#!/usr/bin/env python3
"""A node-classification epoch with host metrics against the same epoch with device metrics, on make_nc("aminer-syn").

The epoch is the reference's: GripNet-aminer.py:120-179 for AminerModel, GripNet-freebase-c.py:146-191 with its loop from
:201 for FreebaseCModel - a training step (forward on the training nodes, loss, backward, Adam), the train metrics of
that step's scores, then the test scores of the returned z and their metrics.  Nodes with even ids train, odd ids test
(as tools/train_nc.py).  Two variants share the training step (utils.class_loss, one launch each way):

  (a) pred = torch.argmax(score, 1); utils.micro_macro(classes, pred)      twice per epoch (the reference's host path)
  (b) utils.class_metrics(score, classes), micro / macro read to the host   twice per epoch

Epochs alternate in blocks between (a) and (b).  Every epoch is timed on its own (wall time from its first launch to its
metrics on the host); behind it, untimed, the other variant's metrics of the same scores are computed and parity is
asserted: metrics within 1e-12, pred equal.  Also: the training step alone, the time of one class_metrics call (CUDA
events around `--calls` back-to-back asynchronous calls: bounded below by the two kernels and by the host's launch rate),
the wall time of one synchronised call as the epoch makes it, and one argmax + micro_macro.  With --rocprof the launch count of (b) is read from a
`rocprofv3 --kernel-trace --stats` run of this script's --metrics-only mode (a child process).  One JSON line.

    python tools/bench_nc_epoch.py [--models aminer,freebase-c] [--epochs 40] [--warmup 5] [--rocprof]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gripnet_amd import _hip, utils                                  # noqa: E402
from gripnet_amd.optim import Adam                                   # noqa: E402
from gripnet_amd.pipeline import AminerModel, FreebaseCModel        # noqa: E402
from gripnet_amd.synth import make_nc                               # noqa: E402


def setup(which, dev):
    data = make_nc("aminer-syn").to(dev)
    torch.manual_seed(1111)
    model = (AminerModel(data.n_p_node, data.n_a_node, data.n_a_type) if which == "aminer" else
             FreebaseCModel(data.n_p_node, data.n_q_node, data.n_a_node, data.n_a_type)).to(dev)
    opt = Adam(model.parameters(), lr=0.01)
    train_nodes = torch.arange(0, data.n_a_node, 2, device=dev)
    test_nodes = torch.arange(1, data.n_a_node, 2, device=dev)
    return data, model, opt, train_nodes, test_nodes, data.a_label[train_nodes].contiguous(), data.a_label[test_nodes].contiguous()


def host_metrics(score, classes):                                    # (a): GripNet-aminer.py:131,137 / :154-156
    pred = torch.argmax(score, dim=1)
    micro, macro = utils.micro_macro(classes, pred)
    return pred, float(micro), float(macro)


def device_metrics(score, classes):                                  # (b)
    m = utils.class_metrics(score, classes)
    return m["pred"], m["micro_f1"].item(), m["macro_f1"].item()


def run_model(which, dev, epochs, warmup, calls):
    data, model, opt, train_nodes, test_nodes, train_class, test_class = setup(which, dev)

    def step():
        model.train()
        opt.zero_grad()
        z, score = model(data, train_nodes)
        loss = utils.class_loss(score, train_class)
        loss.backward()
        opt.step()
        return z.detach(), score.detach()

    def test_scores(z):
        model.eval()
        with torch.no_grad():
            return model.mcip(z, test_nodes)

    def epoch(metrics):
        z, s_tr = step()
        tr = metrics(s_tr, train_class)
        s_te = test_scores(z)
        te = metrics(s_te, test_class)
        return (s_tr, tr), (s_te, te)

    def check(parts, other):
        for (score, got), classes in zip(parts, (train_class, test_class)):
            ref = other(score, classes)
            assert torch.equal(got[0], ref[0]), "pred differs"
            assert abs(got[1] - ref[1]) <= 1e-12 and abs(got[2] - ref[2]) <= 1e-12, (got[1:], ref[1:])

    for _ in range(warmup):
        check(epoch(host_metrics), device_metrics)
        check(epoch(device_metrics), host_metrics)
    times = {"a": [], "b": []}
    block = max(1, epochs // 8)
    done = 0
    while done < epochs:
        for name, metrics, other in (("a", host_metrics, device_metrics), ("b", device_metrics, host_metrics)):
            for _ in range(min(block, epochs - done)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                parts = epoch(metrics)                               # both variants end with the numbers on the host
                times[name].append(time.perf_counter() - t0)
                check(parts, other)
        done += block
    # the training step alone
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        step()
    torch.cuda.synchronize()
    step_ms = 1e3 * (time.perf_counter() - t0) / epochs
    # one asynchronous class_metrics call, back to back, event-timed (the test list's scores)
    z, _ = step()
    s_te = test_scores(z)
    for _ in range(10):
        _hip.class_metrics(s_te, test_class)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        _hip.class_metrics(s_te, test_class)
    e1.record()
    torch.cuda.synchronize()
    call_us = 1e3 * e0.elapsed_time(e1) / calls
    # one utils.class_metrics call as the epoch makes it (launch, error check, two numbers to the host), wall time
    t0 = time.perf_counter()
    for _ in range(calls):
        device_metrics(s_te, test_class)
    sync_call_us = 1e6 * (time.perf_counter() - t0) / calls
    t0 = time.perf_counter()
    for _ in range(max(1, calls // 10)):
        host_metrics(s_te, test_class)
    host_call_us = 1e6 * (time.perf_counter() - t0) / max(1, calls // 10)
    _hip.raise_if_index_errors(dev)

    def median(v):
        v = sorted(v)
        return v[len(v) // 2]

    return {"model": which, "n_train": int(train_nodes.numel()), "n_test": int(test_nodes.numel()), "classes": int(data.n_a_type),
            "epochs_per_variant": len(times["a"]),
            "epoch_ms_a_host_metrics": round(1e3 * sum(times["a"]) / len(times["a"]), 3),
            "epoch_ms_b_device_metrics": round(1e3 * sum(times["b"]) / len(times["b"]), 3),
            "epoch_ms_a_median": round(1e3 * median(times["a"]), 3), "epoch_ms_b_median": round(1e3 * median(times["b"]), 3),
            "train_step_ms": round(step_ms, 3), "class_metrics_event_us_per_call": round(call_us, 2),
            "class_metrics_synced_us_per_call": round(sync_call_us, 1), "argmax_micro_macro_us_per_call": round(host_call_us, 1),
            "parity": "asserted every epoch (1e-12, pred equal)"}


def metrics_only(dev, calls):
    """`calls` utils.class_metrics calls on aminer-syn-sized test scores, nothing else on the device after the setup."""
    g = torch.Generator(device=dev).manual_seed(1)
    score = torch.softmax(torch.randn((10_000, 8), generator=g, device=dev), 1)
    y = torch.randint(0, 8, (10_000,), generator=g, device=dev)
    torch.cuda.synchronize()
    for _ in range(calls):
        utils.class_metrics(score, y)
    torch.cuda.synchronize()


def launch_count(calls):
    """Kernels per utils.class_metrics call, from a rocprofv3 kernel trace of `--metrics-only` (None without rocprofv3)."""
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if prof is None:
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--metrics-only", "--calls", str(calls)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            return None, "rocprofv3 exit {}: {}".format(r.returncode, (r.stderr or r.stdout)[-300:])
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, "no kernel_stats.csv"
        per = {}                                                     # kernel -> [calls, total ns]
        for f in files:
            for row in csv.DictReader(open(f)):
                m = re.search(r"k_class_\w+(<[^>]*>)?", row["Name"])
                if m:
                    c = per.setdefault(m.group(0), [0, 0.0])
                    c[0] += int(row["Calls"])
                    c[1] += float(row["TotalDurationNs"])
    detail = {k: {"calls": c, "mean_us": round(t / max(c, 1) / 1e3, 2)} for k, (c, t) in per.items()}
    return sum(c for c, _ in per.values()) / calls, detail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="aminer,freebase-c")
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--metrics-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.metrics_only:
        metrics_only(dev, args.calls)
        return
    out = {"tool": "bench_nc_epoch", "workload": "aminer-syn", "runs": []}
    for which in args.models.split(","):
        out["runs"].append(run_model(which, dev, args.epochs, args.warmup, args.calls))
        torch.cuda.empty_cache()
    if args.rocprof:
        per_call, detail = launch_count(50)
        out["launches_per_class_metrics_call"] = per_call
        out["launch_detail"] = detail                                # kernels of `calls` calls and their mean device time
    print(json.dumps(out))


if __name__ == "__main__":
    main()
