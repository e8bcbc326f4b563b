#!/usr/bin/env python3
"""The GCN and RGCN node-classification baselines (examples/train_nc_baselines.py's models) on the flattened aminer-syn graph
against the torch formulation (index_select, bmm, index_add_; tests/rgcn_conv_cases.py for RGCNConv, the exported normalised
list for GCNConv), in one process on the same inputs, parameters and GPU:

  forward : the two layers with their ReLUs on relu(embedding), no gradients
  step    : forward, class decoder, loss, backward, Adam step (gripnet_amd.optim.Adam / torch.optim.Adam)

for GCN, for RGCN without edge_norm and for RGCN with edge_norm = 1 / c_{i,r} (the weighted instantiation of the general
kernel).  Parity of the forward's output and of the step's loss is asserted in the run.  Times: HIP events around `--reps`
calls after `--warmup` calls; `--runs` repetitions of the whole measurement.  Prints one JSON line; `--markdown PATH` also
writes the runs as a table.

    python tools/bench_rgcn_conv.py [--runs 3] [--reps 20] [--warmup 5] [--workload aminer-syn] [--markdown profiles/r21_rgcn_conv.md]
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
import rgcn_conv_cases as rc                                                              # noqa: E402
from gripnet_amd import GCNConv, RGCNConv, _hip, multiClassInnerProductDecoder, myGCN     # noqa: E402
from gripnet_amd.optim import Adam                                                        # noqa: E402
from gripnet_amd.synth import make_nc_relational                                          # noqa: E402
from gripnet_amd.utils import class_loss                                                  # noqa: E402


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
    def __init__(self, model, data):
        super().__init__()
        self.model = model
        if model == "gcn":                                                               # GCN_MLP.py:41-49
            self.embedding = torch.nn.Parameter(torch.randn(data.num_nodes, 256))
            self.conv1, self.conv2 = GCNConv(256, 64), GCNConv(64, 32)
        else:                                                                            # RGCN_MLP.py:46-58
            R = data.num_relations
            self.embedding = torch.nn.Parameter(torch.randn(data.num_nodes, 32))
            self.conv1, self.conv2 = RGCNConv(32, 32, R, num_bases=R), RGCNConv(32, 32, R, num_bases=R)
        self.mclp = multiClassInnerProductDecoder(32, data.num_classes)

    def embed(self, data, norm=None):
        x = torch.relu(self.embedding)
        if self.model == "gcn":
            return self.conv2(self.conv1(x, data.edge_index, _relu=True), data.edge_index, _relu=True)
        x = self.conv1(x, data.edge_index, data.edge_type, norm, _relu=True)
        return self.conv2(x, data.edge_index, data.edge_type, norm, _relu=True)


class TorchNet(torch.nn.Module):
    """the same parameters under the torch formulation"""

    def __init__(self, net, data):
        super().__init__()
        self.model = net.model
        self.embedding = torch.nn.Parameter(net.embedding.detach().clone())
        self.p1 = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in net.conv1.parameters()])
        self.p2 = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in net.conv2.parameters()])
        self.w = torch.nn.Parameter(net.mclp.weight.detach().clone())
        if self.model == "gcn":
            self.ei, self.norm = myGCN.norm(data.edge_index, data.num_nodes, None)       # the cached normalised list, built once

    def _gcn(self, x, p):
        xw = x @ p[0]
        out = torch.zeros_like(xw).index_add_(0, self.ei[1], self.norm[:, None] * xw.index_select(0, self.ei[0]))
        return torch.relu(out + p[1])

    def embed(self, data, norm=None):
        x = torch.relu(self.embedding)
        if self.model == "gcn":
            return self._gcn(self._gcn(x, self.p1), self.p2)
        x = rc.forward(x, *self.p1, data.edge_index, data.edge_type, norm, relu=True)
        return rc.forward(x, *self.p2, data.edge_index, data.edge_type, norm, relu=True)


def measure(model, data, norm, args):
    dev = data.edge_index.device
    torch.manual_seed(1111)
    net = Net(model, data).to(dev)
    ref = TorchNet(net, data).to(dev)
    opt, opt_ref = Adam(net.parameters(), lr=0.01), torch.optim.Adam(ref.parameters(), lr=0.01)

    def loss_of(z, w=None):
        if w is None:
            return class_loss(net.mclp(z, data.train_idx), data.train_y)
        return F.nll_loss(torch.log(torch.softmax(z[data.train_idx] @ w, dim=1) + 1e-13), data.train_y)

    def step():
        opt.zero_grad()
        loss = loss_of(net.embed(data, norm))
        loss.backward()
        opt.step()
        return loss.detach()

    def step_ref():
        opt_ref.zero_grad()
        loss = loss_of(ref.embed(data, norm), ref.w)
        loss.backward()
        opt_ref.step()
        return loss.detach()

    with torch.no_grad():
        z, z_ref = net.embed(data, norm), ref.embed(data, norm)
    assert torch.allclose(z, z_ref, rtol=1e-4, atol=1e-4 * float(z_ref.abs().max())), float((z - z_ref).abs().max())
    a, b = float(loss_of(net.embed(data, norm)).detach()), float(loss_of(ref.embed(data, norm), ref.w).detach())
    assert abs(a - b) <= 1e-4 * abs(b), (a, b)
    _hip.raise_if_index_errors(dev)
    rows = []
    for run in range(args.runs):
        with torch.no_grad():
            t_fwd, _ = timed(lambda: net.embed(data, norm), args.reps, args.warmup)
            t_fwd_ref, _ = timed(lambda: ref.embed(data, norm), args.reps, args.warmup)
        t_step, _ = timed(step, args.reps, args.warmup)
        t_step_ref, _ = timed(step_ref, args.reps, args.warmup)
        rows.append({"model": model + ("" if norm is None else " + edge_norm"), "run": run + 1, "forward_ms": round(t_fwd, 4),
                     "forward_torch_ms": round(t_fwd_ref, 4), "forward_ratio": round(t_fwd_ref / t_fwd, 2), "step_ms": round(t_step, 4),
                     "step_torch_ms": round(t_step_ref, 4), "step_ratio": round(t_step_ref / t_step, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="aminer-syn")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    data = make_nc_relational(args.workload)
    norm = rc.relation_mean_norm(data.edge_index, data.edge_type, int(data.num_nodes)).to(dev)
    data = data.to(dev)
    results = measure("gcn", data, None, args) + measure("rgcn", data, None, args) + measure("rgcn", data, norm, args)
    out = {"workload": "{} (N {}, E {}, R {})".format(data.name, int(data.num_nodes), int(data.edge_index.shape[1]), int(data.num_relations)),
           "results": results, "reps": args.reps, "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))
    if args.markdown:
        with open(args.markdown, "w") as fh:
            fh.write("# GCN and RGCN baselines against the torch formulation\n\n")
            fh.write("`tools/bench_rgcn_conv.py --runs {} --reps {} --warmup {} --workload {}` on {}: {}.\nMilliseconds per call (HIP events); "
                     "the torch figures (index_select, bmm, index_add_) are from the same process, inputs and parameters, parity of the "
                     "forward and the loss asserted first.  ratio = torch / this library.\n\n".format(
                         args.runs, args.reps, args.warmup, args.workload, out["device"], out["workload"]))
            fh.write("| model | run | forward ms | torch forward ms | ratio | step ms | torch step ms | ratio |\n|---|---|---|---|---|---|---|---|\n")
            for r in results:
                fh.write("| {model} | {run} | {forward_ms:.3f} | {forward_torch_ms:.3f} | {forward_ratio:.2f} | {step_ms:.3f} | {step_torch_ms:.3f} | "
                         "{step_ratio:.2f} |\n".format(**r))


if __name__ == "__main__":
    main()
