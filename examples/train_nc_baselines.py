#!/usr/bin/env python3
"""Counterparts of the reference's GCN and RGCN node-classification baselines (baselines/NC_baselines/GCN_MLP.py and
RGCN_MLP.py) on the MI355X path.

`Net` and the loop are GCN_MLP.py:41-99 and RGCN_MLP.py:46-101 with the imports swapped: an embedding ([N, 256] for GCN, [N, 32]
for RGCN; the baselines' `sparse_id` product is the identity), `GCNConv(256, 64)`, `GCNConv(64, 32)` or
`RGCNConv(32, 32, R, num_bases=R)` twice (RGCN_MLP.py:52-57), a ReLU after each (fused into the layer's store), the class
decoder over the labelled nodes.  The reference's `nll_loss(out[train_idx], train_y)` is the project's
`class_loss(softmax(...), train_y)` up to its EPS; the optimiser is gripnet_amd.optim.Adam (one launch), the metrics
utils.class_metrics.  The reference loads pickled Data objects that are not available offline; the graph is the synthetic NC
ladder flattened by synth.make_nc_homogeneous / make_nc_relational (seven relations, `edge_type` unsorted):

    python examples/train_nc_baselines.py --model rgcn --workload aminer-syn --epochs 20
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gripnet_amd import GCNConv, RGCNConv, multiClassInnerProductDecoder
from gripnet_amd.optim import Adam
from gripnet_amd.synth import make_nc_homogeneous, make_nc_relational
from gripnet_amd.utils import class_loss, class_metrics


class GcnNet(torch.nn.Module):                                        # GCN_MLP.py:41-56
    def __init__(self, data, hidden=64, embeddings=32):
        super().__init__()
        self.embedding = torch.nn.Parameter(torch.empty(data.num_nodes, 256))
        self.embedding.data.normal_()
        self.conv1 = GCNConv(256, hidden)
        self.conv2 = GCNConv(hidden, embeddings)
        self.mclp = multiClassInnerProductDecoder(embeddings, data.num_classes)

    def forward(self, data, nodes):
        x = torch.relu(self.embedding)
        x = self.conv1(x, data.edge_index, _relu=True)
        x = self.conv2(x, data.edge_index, _relu=True)
        return self.mclp(x, nodes)


class RgcnNet(torch.nn.Module):                                       # RGCN_MLP.py:46-65
    def __init__(self, data, in_dim=32, hidden=32, embeddings=32):
        super().__init__()
        self.embedding = torch.nn.Parameter(torch.empty(data.num_nodes, in_dim))
        self.embedding.data.normal_()
        self.conv1 = RGCNConv(in_dim, hidden, data.num_relations, num_bases=data.num_relations)
        self.conv2 = RGCNConv(hidden, embeddings, data.num_relations, num_bases=data.num_relations)
        self.mclp = multiClassInnerProductDecoder(embeddings, data.num_classes)

    def forward(self, data, nodes):
        x = torch.relu(self.embedding)
        x = self.conv1(x, data.edge_index, data.edge_type, _relu=True)
        x = self.conv2(x, data.edge_index, data.edge_type, _relu=True)
        return self.mclp(x, nodes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("gcn", "rgcn"), required=True)
    ap.add_argument("--workload", choices=("tiny", "aminer-syn"), default="aminer-syn")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--lr", type=float, default=0.01)
    args = ap.parse_args()
    torch.manual_seed(1111)                                           # GCN_MLP.py:12, RGCN_MLP.py:12
    device = torch.device("cuda")
    data = (make_nc_homogeneous if args.model == "gcn" else make_nc_relational)(args.workload).to(device)
    model = (GcnNet if args.model == "gcn" else RgcnNet)(data).to(device)
    optimizer = Adam(model.parameters(), lr=args.lr)                  # GCN_MLP.py:60, RGCN_MLP.py:70

    def train():                                                      # RGCN_MLP.py:84-93
        model.train()
        optimizer.zero_grad()
        score = model(data, data.train_idx)
        loss = class_loss(score, data.train_y)
        loss.backward()
        optimizer.step()
        return loss.detach(), class_metrics(score.detach(), data.train_y)

    def test():                                                       # RGCN_MLP.py:96-101
        model.eval()
        with torch.no_grad():
            return class_metrics(model(data, data.test_idx), data.test_y)

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
