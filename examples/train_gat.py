#!/usr/bin/env python3
"""Counterpart of the reference's GAT node-classification baseline (baselines/NC_baselines/GAT.py) on the MI355X path.

`Net` and the loop are GAT.py:59-120 with the imports swapped: a [N, 256] embedding (GAT.py's `sparse_id` product is the
identity), `GATConv(256, 16, heads=4)`, `GATConv(64, 32, concat=False)`, a ReLU after each (fused into the layer's store), the
class decoder over the labelled nodes.  The reference's `nll_loss(log_softmax(...)[train_idx], train_y)` is the project's
`class_loss(softmax(...), train_y)` up to its EPS; the optimiser is gripnet_amd.optim.Adam (one launch), the metrics
utils.class_metrics.  The reference loads a pickled Data object that is not available offline; the graph is the synthetic NC
ladder flattened by synth.make_nc_homogeneous:

    python examples/train_gat.py --workload aminer-syn --epochs 20
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gripnet_amd import GATConv, multiClassInnerProductDecoder
from gripnet_amd.optim import Adam
from gripnet_amd.synth import make_nc_homogeneous
from gripnet_amd.utils import class_loss, class_metrics


class Net(torch.nn.Module):                                           # GAT.py:59-74
    def __init__(self, num_nodes, num_classes, heads=4, hidden_features=16, embeddings=32):
        super().__init__()
        self.embedding = torch.nn.Parameter(torch.empty(num_nodes, 256))
        self.embedding.data.normal_()
        self.conv1 = GATConv(256, hidden_features, heads=heads)
        self.conv2 = GATConv(hidden_features * heads, embeddings, concat=False)
        self.mclp = multiClassInnerProductDecoder(embeddings, num_classes)

    def embed(self, edge_index):
        x = torch.relu(self.embedding)
        x = self.conv1(x, edge_index, _relu=True)
        return self.conv2(x, edge_index, _relu=True)

    def forward(self, edge_index, nodes):
        return self.mclp(self.embed(edge_index), nodes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("tiny", "aminer-syn"), default="aminer-syn")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--lr", type=float, default=0.01)
    args = ap.parse_args()
    torch.manual_seed(1111)                                           # GAT.py:14
    device = torch.device("cuda")
    data = make_nc_homogeneous(args.workload).to(device)
    model = Net(data.num_nodes, data.num_classes).to(device)
    optimizer = Adam(model.parameters(), lr=args.lr)                  # GAT.py:78

    def train():                                                      # GAT.py:92-103
        model.train()
        optimizer.zero_grad()
        score = model(data.edge_index, data.train_idx)
        loss = class_loss(score, data.train_y)
        loss.backward()
        optimizer.step()
        return loss.detach(), class_metrics(score.detach(), data.train_y)

    def test():                                                       # GAT.py:106-113
        model.eval()
        with torch.no_grad():
            return class_metrics(model(data.edge_index, data.test_idx), data.test_y)

    first = last = None
    for epoch in range(1, args.epochs + 1):
        t0 = time.time()
        loss, tr = train()
        te = test()
        numbers = (float(loss), float(tr["micro_f1"]), float(tr["macro_f1"]), float(te["micro_f1"]), float(te["macro_f1"]))
        first, last = (numbers[0] if first is None else first), numbers[0]
        print("{:3d}   loss:{:0.4f}   train_micro:{:0.4f}   train_macro:{:0.4f}   test_micro:{:0.4f}   test_macro:{:0.4f}"
              "   time:{:0.2f}ms".format(epoch, *numbers, 1e3 * (time.time() - t0)))
    print("loss {:0.4f} -> {:0.4f}".format(first, last))


if __name__ == "__main__":
    main()
