#!/usr/bin/env python3
"""The GAT baseline (examples/train_gat.py's model: embedding [N, 256], GATConv(256, 16, heads=4), GATConv(64, 32,
concat=False), class decoder) on make_nc_homogeneous("aminer-syn") against the torch formulation of tests/gat_cases.py
(index_select, scatter_reduce(amax), index_add_; its working list built once, outside the timed window), in one process on
the same inputs and the same GPU:

  forward : the two attention layers with their ReLUs on relu(embedding), no gradients
  step    : forward, class decoder, loss, backward, Adam step (gripnet_amd.optim.Adam / torch.optim.Adam)
  layer 1 : every entry point of GATConv(256, 16, heads=4) on its own, with two byte counts: what the launch requests (int32
            CSR ids, an fp32 row per edge, the [N, H] arrays) and what it has to move at the least (every array once: the
            gathered table fits the caches); the latter over the time is priced against the HBM peak of 8 TB/s

Parity of the forward's output and of the step's loss and gradients is asserted in the run.  Times: HIP events around `--reps`
calls after `--warmup` calls; `--runs` repetitions of the whole measurement.  Prints one JSON line; `--markdown PATH` also
writes the runs as tables.

    python tools/bench_gat.py [--runs 3] [--reps 20] [--warmup 5] [--workload aminer-syn] [--markdown profiles/r20_gat.md]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gat_cases as gc                                                    # noqa: E402
from gripnet_amd import GATConv, _hip, multiClassInnerProductDecoder      # noqa: E402
from gripnet_amd.gat import gat_plan                                      # noqa: E402
from gripnet_amd.optim import Adam                                        # noqa: E402
from gripnet_amd.synth import make_nc_homogeneous                         # noqa: E402
from gripnet_amd.utils import class_loss                                  # noqa: E402

HBM_PEAK_GBS = 8000.0


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


class Net(torch.nn.Module):
    def __init__(self, n, classes):
        super().__init__()
        self.embedding = torch.nn.Parameter(torch.randn(n, 256))
        self.conv1, self.conv2 = GATConv(256, 16, heads=4), GATConv(64, 32, concat=False)
        self.mclp = multiClassInnerProductDecoder(32, classes)

    def embed(self, ei):
        return self.conv2(self.conv1(torch.relu(self.embedding), ei, _relu=True), ei, _relu=True)


class TorchNet(torch.nn.Module):
    """the same parameters under the torch formulation"""

    def __init__(self, net):
        super().__init__()
        self.embedding = torch.nn.Parameter(net.embedding.detach().clone())
        self.p1 = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in (net.conv1.weight, net.conv1.att, net.conv1.bias)])
        self.p2 = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in (net.conv2.weight, net.conv2.att, net.conv2.bias)])
        self.w = torch.nn.Parameter(net.mclp.weight.detach().clone())

    def embed(self, ei, working):
        x = gc.forward(torch.relu(self.embedding), *self.p1, ei, 4, True, 0.2, True, working=working)
        return gc.forward(x, *self.p2, ei, 1, False, 0.2, True, working=working)


def layer_entries(net, ei, n, reps, warmup):
    """[(entry point, ms, bytes requested, bytes every array once)] of layer 1 on its own"""
    dev = ei.device
    plan = gat_plan(ei, n, transpose=True)
    nnz, H, C, Fn = plan.nnz, 4, 16, 64
    w, att, b = net.conv1.weight.detach(), net.conv1.att.detach(), net.conv1.bias.detach()
    x = torch.relu(net.embedding.detach())
    h, out, o = (torch.empty((n, Fn), device=dev) for _ in range(3))
    g = torch.randn((n, Fn), device=dev)
    _hip.gemm(x, w, h)
    a_dst, a_src, m, rinv = _hip.gat_forward(plan, h, att, H, 0.2, b, True, True, out, o)
    lib, sp, p = _hip.load(), _hip.stream_ptr, _hip.ptr
    pack, da_dst, da_src = torch.empty((n, H, 4), device=dev), torch.empty((n, H), device=dev), torch.empty((n, H), device=dev)
    dh, d_att = torch.empty_like(h), torch.empty_like(att)
    need = int(lib.gn_gat_att_grad_workspace_bytes(n, H, C))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    row, nh, csr = 4 * Fn, 4 * H, 4 * nnz + 8 * n
    calls = [
        ("gn_gemm_f32 (h = x W)", lambda: _hip.gemm(x, w, h), n * (4 * 256 + row), n * (4 * 256 + row)),
        ("gn_gat_logits_f32", lambda: _hip._call("gn_gat_logits_f32", p(h), Fn, n, H, C, p(att), p(a_dst), p(a_src), sp(dev)), n * (row + 2 * nh), n * (row + 2 * nh)),
        ("gn_gat_forward_f32", lambda: _hip._call("gn_gat_forward_f32", plan._h, p(h), Fn, H, C, p(a_dst), p(a_src), 0.2, p(b), 1, 1, p(out), Fn,
                                                  p(o), p(m), p(rinv), sp(dev)), nnz * (4 + row + nh) + n * (8 + 2 * row + 3 * nh), csr + n * (3 * row + 4 * nh)),
        ("gn_gat_backward_dst_f32", lambda: _hip._call("gn_gat_backward_dst_f32", plan._h, p(h), Fn, H, C, p(a_dst), p(a_src), p(m), p(rinv), 0.2,
                                                       p(g), Fn, 1, p(o), p(pack), p(da_dst), sp(dev)), nnz * (4 + row + nh) + n * (8 + 2 * row + 8 * nh), csr + n * (3 * row + 9 * nh)),
        ("gn_gat_backward_src_f32", lambda: _hip._call("gn_gat_backward_src_f32", plan._h, p(h), Fn, H, C, p(a_src), p(pack), 0.2, p(g), Fn, 1,
                                                       p(da_dst), p(att), p(dh), Fn, p(da_src), sp(dev)), nnz * (4 + row + 4 * nh) + n * (8 + 2 * row + 3 * nh), csr + n * (3 * row + 7 * nh)),
        ("gn_gat_att_grad_f32", lambda: _hip._call("gn_gat_att_grad_f32", p(h), Fn, n, H, C, p(da_dst), p(da_src), p(d_att), p(ws), need, sp(dev)),
         n * (row + 2 * nh), n * (row + 2 * nh)),
    ]
    return [(name, timed(fn, reps, warmup)[0], int(asked), int(least)) for name, fn, asked, least in calls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="aminer-syn")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    data = make_nc_homogeneous(args.workload).to(dev)
    n, ei = int(data.num_nodes), data.edge_index
    torch.manual_seed(1111)
    net = Net(n, data.num_classes).to(dev)
    ref = TorchNet(net).to(dev)
    working = tuple(gc.working_list(ei, n))
    opt, opt_ref = Adam(net.parameters(), lr=0.01), torch.optim.Adam(ref.parameters(), lr=0.01)

    def step():
        opt.zero_grad()
        loss = class_loss(net.mclp(net.embed(ei), data.train_idx), data.train_y)
        loss.backward()
        opt.step()
        return loss.detach()

    def step_ref():
        opt_ref.zero_grad()
        z = ref.embed(ei, working)
        loss = F.nll_loss(torch.log(torch.softmax(z[data.train_idx] @ ref.w, dim=1) + 1e-13), data.train_y)
        loss.backward()
        opt_ref.step()
        return loss.detach()

    # parity before anything is trained: the forward, the loss and every gradient of one step
    with torch.no_grad():
        z, z_ref = net.embed(ei), ref.embed(ei, working)
    assert torch.allclose(z, z_ref, rtol=1e-4, atol=1e-5), float((z - z_ref).abs().max())
    loss = class_loss(net.mclp(net.embed(ei), data.train_idx), data.train_y)
    loss.backward()
    loss_ref = F.nll_loss(torch.log(torch.softmax(ref.embed(ei, working)[data.train_idx] @ ref.w, dim=1) + 1e-13), data.train_y)
    loss_ref.backward()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-5 * abs(float(loss_ref.detach())), (float(loss.detach()), float(loss_ref.detach()))
    pairs = [(net.embedding, ref.embedding), (net.mclp.weight, ref.w)] + list(zip(net.conv1.parameters(), ref.p1)) + list(zip(net.conv2.parameters(), ref.p2))
    for a, b in pairs:
        tol = 1e-3 * float(b.grad.abs().max()) + 1e-12
        assert float((a.grad - b.grad).abs().max()) <= tol, (tuple(a.shape), float((a.grad - b.grad).abs().max()), tol)
    _hip.raise_if_index_errors(dev)

    results, entries = [], []
    for run in range(args.runs):
        with torch.no_grad():
            t_fwd, _ = timed(lambda: net.embed(ei), args.reps, args.warmup)
            t_fwd_ref, _ = timed(lambda: ref.embed(ei, working), args.reps, args.warmup)
        t_step, _ = timed(step, args.reps, args.warmup)
        t_step_ref, _ = timed(step_ref, args.reps, args.warmup)
        results.append({"run": run + 1, "forward_ms": round(t_fwd, 4), "forward_torch_ms": round(t_fwd_ref, 4),
                        "forward_ratio": round(t_fwd_ref / t_fwd, 2), "step_ms": round(t_step, 4), "step_torch_ms": round(t_step_ref, 4),
                        "step_ratio": round(t_step_ref / t_step, 2)})
        for name, ms, asked, least in layer_entries(net, ei, n, args.reps, args.warmup):
            entries.append({"run": run + 1, "entry": name, "us": round(1e3 * ms, 2), "requested_mb": round(asked / 1e6, 2),
                            "least_mb": round(least / 1e6, 2), "requested_gbs": round(asked / (ms * 1e-3) / 1e9, 1),
                            "hbm_frac": round(least / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
    out = {"workload": "{} (N {}, E {}, working list {})".format(data.name, n, int(ei.shape[1]), int(working[0].numel())),
           "results": results, "layer1": entries, "reps": args.reps, "warmup": args.warmup, "runs": args.runs,
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))
    if args.markdown:
        with open(args.markdown, "w") as fh:
            fh.write("# GAT baseline against the torch formulation\n\n")
            fh.write("`tools/bench_gat.py --runs {} --reps {} --warmup {} --workload {}` on {}: {}.\nMilliseconds per call (HIP events); "
                     "the torch figures are from the same process, inputs and parameters, parity of the forward, the loss and the "
                     "gradients asserted first.  ratio = torch / this library.\n\n".format(args.runs, args.reps, args.warmup, args.workload,
                                                                                            out["device"], out["workload"]))
            fh.write("| run | forward ms | torch forward ms | ratio | step ms | torch step ms | ratio |\n|---|---|---|---|---|---|---|\n")
            for r in results:
                fh.write("| {run} | {forward_ms:.3f} | {forward_torch_ms:.3f} | {forward_ratio:.2f} | {step_ms:.3f} | {step_torch_ms:.3f} | "
                         "{step_ratio:.2f} |\n".format(**r))
            fh.write("\nLayer 1 (256 -> 4 x 16), every entry point on its own: microseconds per call; the bytes the launch requests (a "
                     "row per edge) and their rate; the bytes it has to move at the least (every array once) and their rate as a share "
                     "of the 8 TB/s HBM peak.\n\n| run | entry point | us | requested MB | requested GB/s | least MB | share of HBM peak |\n"
                     "|---|---|---|---|---|---|---|\n")
            for e in entries:
                fh.write("| {run} | {entry} | {us:.2f} | {requested_mb:.2f} | {requested_gbs:.1f} | {least_mb:.2f} | {hbm_frac:.4f} |\n".format(**e))


if __name__ == "__main__":
    main()
