#!/usr/bin/env python3
"""Counterpart of the reference's node-classification drivers (GripNet-aminer.py, GripNet-freebase-c.py) on the MI355X path.

The reference scripts load pickled torch_geometric Data objects that are not available offline; this driver runs the same
models, loss, optimiser and epoch structure (GripNet-aminer.py:113,120-179; GripNet-freebase-c.py:146-211) on the synthetic
NC ladder of gripnet_amd.synth.  Nodes with even ids train, odd ids test:

    python examples/train_nc.py --model aminer --workload aminer-syn --epochs 20

The per-epoch train and test micro / macro F1 come from utils.class_metrics: the reference's
`pred = torch.argmax(score, dim=1)` + `micro_macro(classes, pred)` (a host copy and two scikit-learn calls each) on the GPU.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gripnet_amd.pipeline import AminerModel, FreebaseCModel
from gripnet_amd.synth import make_nc
from gripnet_amd.utils import EPS, class_metrics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("aminer", "freebase-c"), default="aminer")
    ap.add_argument("--workload", choices=("tiny", "aminer-syn"), default="aminer-syn")
    ap.add_argument("--epochs", type=int, default=20)
    args = ap.parse_args()
    torch.manual_seed(1111)                                           # GripNet-aminer.py:15
    device = torch.device("cuda")
    data = make_nc(args.workload).to(device)
    if args.model == "aminer":                                        # GripNet-aminer.py:96-108
        model = AminerModel(data.n_p_node, data.n_a_node, data.n_a_type)
    else:                                                             # GripNet-freebase-c.py:102-136
        model = FreebaseCModel(data.n_p_node, data.n_q_node, data.n_a_node, data.n_a_type)
    model = model.to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01)         # GripNet-aminer.py:100,113
    train_nodes = torch.arange(0, data.n_a_node, 2, device=device)
    test_nodes = torch.arange(1, data.n_a_node, 2, device=device)
    train_class, test_class = data.a_label[train_nodes].contiguous(), data.a_label[test_nodes].contiguous()

    def train():                                                      # GripNet-aminer.py:120-147
        model.train()
        optimizer.zero_grad()
        z, score = model(data, train_nodes)
        loss = -torch.log(score[range(score.shape[0]), train_class] + EPS).mean()
        loss.backward()
        optimizer.step()
        m = class_metrics(score.detach(), train_class)                # argmax + micro_macro, on the device
        return z.detach(), loss, m

    def test(z):                                                      # GripNet-aminer.py:150-158
        model.eval()
        with torch.no_grad():
            score = model.mcip(z, test_nodes)
        return class_metrics(score, test_class)

    for epoch in range(args.epochs):
        t0 = time.time()
        z, loss, tr = train()
        te = test(z)
        numbers = (float(loss), float(tr["micro_f1"]), float(tr["macro_f1"]), float(te["micro_f1"]), float(te["macro_f1"]))
        print("{:3d}   loss:{:0.4f}   train_micro:{:0.4f}   train_macro:{:0.4f}   test_micro:{:0.4f}   test_macro:{:0.4f}"
              "   time:{:0.2f}ms".format(epoch, *numbers, 1e3 * (time.time() - t0)))


if __name__ == "__main__":
    main()
