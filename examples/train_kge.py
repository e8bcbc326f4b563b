#!/usr/bin/env python3
"""Counterpart of the reference's KGE link-prediction baselines (baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py)
on the MI355X path.

The reference script executes at import and loads `datasets_baselines/pose-*-combl.pt` (:28), which is not available
offline; this driver runs the same model, loss, optimiser and epoch structure (:238-305) on the synthetic homogenised
graph of gripnet_amd.synth.make_rgcn_pose (all drug and gene nodes are entities; the gene-gene and gene-drug edges are the
last two relations):

    python examples/train_kge.py --model RotatE --workload pose0-syn --epochs 3
    python examples/train_kge.py --model RotatE --workload pose0-syn --time
    python examples/train_kge.py --model RotatE --workload pose0-syn --epochs 3 --rank
    python examples/train_kge.py --model RotatE --workload pose0-syn --epochs 3 --negatives 256 --adversarial-temperature 1.0

The reference defines KGEModel in the driver itself; here it comes from the package.  `--time` prints the milliseconds of
one training step (forward of both lists, backward, optimiser; fixed negatives) and, next to it, the same step with the
scoring done by the torch formulation of the reference (tests/kge_cases.py) on the same GPU.  `--rank` prints, after the
last epoch, filtered MRR and Hits@1/3/10 of a fixed sample of the list's triples against every entity, tail side and head
side (KGEModel.rank; the synthetic graph has no held-out split, so the triples ranked are training triples and the
filter is the training list: as given for the tail side, flipped for the head side).

`--negatives K` (and / or `--adversarial-temperature T`) trains the way these four models are trained in the code base the
class comes from: an epoch is a pass over shuffled mini-batches of `--batch` positives, every positive gets K uniform
candidate entities (gripnet_amd.kge.sample_candidates, drawn on the device) that replace its tail ('tail-batch') or its
head ('head-batch'), alternating from batch to batch, and the loss is gripnet_amd.kge.negative_sampling_loss on the raw
scores: one HIP launch forward and one backward.  `--filter-negatives` keeps the known triples of the training list out of
the candidates (two KnownPairs: keyed (relation, head) for candidate tails, built from the flipped list for candidate
heads); `--subsampling` weights every positive by 1 / sqrt(count(r, h) + count(r, t) + 4), as that code base does;
`--torch-loss` keeps the earlier formulation for comparison: torch.randint candidates and
gripnet_amd.kge.self_adversarial_loss in torch ops (no filter, no weights).  Without these flags the script does what it
always did.

    python examples/train_kge.py --model RotatE --workload pose0-syn --epochs 3 --negatives 256 --adversarial-temperature 1.0 --filter-negatives

`--shared-negatives G` (with `--negatives K`) shares one list of K candidates among a chunk of the mini-batch's positives, as
DGL-KE and PyTorch-BigGraph do: the batch is cut into G chunks, gripnet_amd.kge.sample_shared_candidates draws G lists on the
device and the scorer runs in the 'tail-shared' / 'head-shared' modes - G K entity rows are gathered instead of batch x K, and
DistMult and ComplEx score on the matrix cores.  A shared list cannot be filtered per positive, so the flag does not combine
with `--filter-negatives`, `--typed-candidates` or `--torch-loss`; a last, shorter batch takes gcd(its size, G) chunks.

    python examples/train_kge.py --model ComplEx --workload pose0-syn --epochs 3 --negatives 256 --shared-negatives 8

`--typed-candidates` restricts `--rank` and `--negatives K` to the entities that can fill the slot at all (the reference
draws its evaluation negatives from the drugs only, :277-279): a drug-drug relation's heads and tails are drugs
[0, n_drug), the gene-gene relation's are genes [n_drug, n_node), the bidirectional gene-drug relation keeps every
entity; one table serves both sides (gripnet_amd.utils.candidate_ranges, the `candidates` argument).  The triples ranked
are then sorted by relation, so that a workgroup's queries share a range and the scan is as short as the range.

    python examples/train_kge.py --model RotatE --workload pose0-syn --epochs 3 --rank --typed-candidates
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gripnet_amd import KGEModel                                      # reference: class KGEModel, :58-235
from gripnet_amd import _hip
from gripnet_amd.kge import negative_sampling_loss, sample_candidates, sample_shared_candidates, self_adversarial_loss
from gripnet_amd.synth import make_rgcn_pose
from gripnet_amd.decoder import KnownPairs
from gripnet_amd.utils import (EPS, candidate_ranges, device_negative_sampler, ranking_metrics, relation_metrics,
                               typed_negative_sampling)


class Negatives:
    """Per-relation negatives of a static positive list: drawn on the device; where the device sampler refuses the list
    (its pair keys do not hold this many entities) by the host loop of utils.typed_negative_sampling."""

    def __init__(self, pos_index, num_nodes, range_list):
        self.pos, self.n, self.ranges = pos_index, num_nodes, range_list
        try:
            self.sampler = device_negative_sampler(pos_index, num_nodes, range_list)
        except (_hip.GripNetHipError, ValueError):
            self.sampler, self.host_pos = None, pos_index.cpu()

    def sample(self, seed):
        if self.sampler is not None:
            return self.sampler.sample(seed=seed)
        return typed_negative_sampling(self.host_pos, self.n, self.ranges.cpu(), np.random.RandomState(seed)).to(self.pos.device)


class TorchKGE(torch.nn.Module):
    """The same parameters scored by the torch formulation of the reference (for --time only)."""

    def __init__(self, model):
        super().__init__()
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import kge_cases
        self.formulation = kge_cases.log_sigmoid_score
        self.name, self.gamma = model.model_name, model.gamma.item()
        self.entity_embedding = torch.nn.Parameter(model.entity_embedding.detach().clone())
        self.relation_embedding = torch.nn.Parameter(model.relation_embedding.detach().clone())

    def forward(self, sample, et):
        return self.formulation(self.name, self.entity_embedding, self.relation_embedding, sample, et, self.gamma)


def step_ms(model, optimizer, pos_index, neg_index, et, warmup=3, steps=10):
    def step():
        optimizer.zero_grad()
        neg_score = model(neg_index, et)
        pos_score = model(pos_index, et)
        loss = -(pos_score + EPS).mean() + -(1 - neg_score + EPS).mean()
        loss.backward()
        optimizer.step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="RotatE", choices=["TransE", "DistMult", "ComplEx", "RotatE"])
    ap.add_argument("--workload", default="small")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rank", action="store_true", help="filtered MRR / Hits@k of both sides after the last epoch")
    ap.add_argument("--rank-sample", type=int, default=20000, help="triples ranked by --rank")
    ap.add_argument("--negatives", type=int, default=None, help="K uniform candidates per positive: mini-batch training")
    ap.add_argument("--adversarial-temperature", type=float, default=None, help="self-adversarial weighting of the K negatives")
    ap.add_argument("--batch", type=int, default=1024, help="positives per mini-batch (with --negatives)")
    ap.add_argument("--filter-negatives", action="store_true", help="never draw a known training triple as a negative")
    ap.add_argument("--subsampling", action="store_true", help="weight a positive by 1 / sqrt(count(r, h) + count(r, t) + 4)")
    ap.add_argument("--torch-loss", action="store_true", help="torch.randint candidates and the loss in torch ops")
    ap.add_argument("--shared-negatives", type=int, default=None, metavar="G",
                    help="share one list of K candidates among each of G chunks of a mini-batch ('tail-shared' / 'head-shared')")
    ap.add_argument("--typed-candidates", action="store_true",
                    help="--rank and --negatives take a relation's candidates from the node type that can fill the slot")
    args = ap.parse_args()
    torch.manual_seed(1111)
    np.random.seed(1111)
    device = torch.device("cuda")
    data = make_rgcn_pose(args.workload).to(device)
    embed_dim, learning_rate = 32, 0.01                                # :54-55
    model = KGEModel(args.model, data.n_node, data.n_edge_type, hidden_dim=embed_dim, gamma=12).to(device)   # :238-244
    optimizer = torch.optim.Adam(model.parameters(), lr=learning_rate)                                       # :247
    negatives = Negatives(data.train_idx, data.n_node, data.train_range)
    drug_edges = int(data.train_range[-2][0])
    drug_ranges = data.train_range[:-2]
    drug_negatives = Negatives(data.train_idx[:, :drug_edges].contiguous(), data.n_drug, drug_ranges)

    if args.time:
        neg_index = negatives.sample(0)
        other = TorchKGE(model).to(device)
        other_optimizer = torch.optim.Adam(other.parameters(), lr=learning_rate)
        for run in range(3):
            ours = step_ms(model, optimizer, data.train_idx, neg_index, data.train_et)
            torch_ms = step_ms(other, other_optimizer, data.train_idx, neg_index, data.train_et)
            print("{} {} run {}: E = {}, n = {}, R = {}: HIP step {:.3f} ms, torch formulation {:.3f} ms ({:.2f}x)".format(
                args.model, data.name, run + 1, data.train_idx.shape[1], data.n_node, data.n_edge_type, ours, torch_ms,
                torch_ms / ours))
        _hip.raise_if_index_errors(device)
        return

    def train(epoch):                                                 # :254-305
        model.train()
        optimizer.zero_grad()
        pos_index = data.train_idx
        neg_index = negatives.sample(2 * epoch)
        neg_score = model(neg_index, data.train_et)
        pos_score = model(pos_index, data.train_et)
        pos_loss = -(pos_score + EPS).mean()
        neg_loss = -(1 - neg_score + EPS).mean()
        loss = pos_loss + neg_loss
        loss.backward()
        optimizer.step()
        model.eval()
        with torch.no_grad():
            neg_score = model(drug_negatives.sample(2 * epoch + 1), data.train_et[:drug_edges])
        # the reference loops over the drug relations with one scikit-learn call each (:282-293); here one pass on the GPU
        auprc, auroc, ap = relation_metrics(pos_score.detach()[:drug_edges].contiguous(), neg_score, drug_ranges)
        return float(loss.detach()), float(auprc.nanmean()), float(auroc.nanmean()), float(ap.nanmean())

    batched = args.negatives is not None or args.adversarial_temperature is not None or args.shared_negatives is not None
    n_negatives = 256 if args.negatives is None else args.negatives

    if args.torch_loss and (args.filter_negatives or args.subsampling or args.typed_candidates):
        ap.error("--torch-loss is the unfiltered, unweighted, untyped formulation")
    if args.shared_negatives is not None:
        if args.torch_loss or args.filter_negatives or args.typed_candidates:
            ap.error("--shared-negatives draws unfiltered, untyped lists and scores them on the HIP path")
        if not 1 <= args.shared_negatives <= args.batch:
            ap.error("--shared-negatives G needs 1 <= G <= --batch")
    typed = None
    if args.typed_candidates:                                         # drug-drug relations, then gene-gene, then gene-drug (both ways)
        R, n_drug, n_node = int(data.n_edge_type), int(data.n_drug), int(data.n_node)
        typed = candidate_ranges(R, n_node, [(0, R - 2, 0, n_drug), (R - 2, R - 1, n_drug, n_node)], device=device)
    sides = {"tail-batch": "tail", "head-batch": "head"}
    known = {"tail": None, "head": None}
    if batched and args.filter_negatives:
        known = {"tail": KnownPairs([(data.train_idx, data.train_et)], data.n_node, data.n_edge_type),
                 "head": KnownPairs([(data.train_idx.flip(0), data.train_et)], data.n_node, data.n_edge_type)}
    weights = None
    if batched and args.subsampling:                                  # one count per (relation, head) and (relation, tail)
        head_key, tail_key = (data.train_et * data.n_node + data.train_idx[i] for i in (0, 1))
        size = data.n_edge_type * data.n_node
        count = torch.bincount(head_key, minlength=size)[head_key] + torch.bincount(tail_key, minlength=size)[tail_key]
        weights = torch.rsqrt((count + 4).float())

    def train_batched(epoch):
        """One pass over shuffled mini-batches; the metrics are the full-list ones of `train`, after the pass."""
        model.train()
        gen = torch.Generator(device=device).manual_seed(1111 + epoch)
        e = data.train_idx.shape[1]
        order = torch.randperm(e, generator=gen, device=device)
        total = torch.zeros((), device=device)
        starts = range(0, e, args.batch)
        for i, lo in enumerate(starts):
            pick = order[lo:lo + args.batch]
            positive, et = data.train_idx[:, pick].contiguous(), data.train_et[pick].contiguous()
            mode = "tail-batch" if i % 2 == 0 else "head-batch"
            optimizer.zero_grad()
            if args.shared_negatives is not None:
                lists = math.gcd(pick.numel(), args.shared_negatives)
                mode = mode.replace("batch", "shared")
                candidates = sample_shared_candidates(lists, n_negatives, data.n_node, seed=(1111 + epoch) * len(starts) + i, device=device)
                loss = negative_sampling_loss(model.score(positive, et), model.score((positive, candidates), et, mode=mode),
                                              args.adversarial_temperature, None if weights is None else weights[pick])
            elif args.torch_loss:
                candidates = torch.randint(0, data.n_node, (pick.numel(), n_negatives), generator=gen, device=device)
                loss = self_adversarial_loss(model.score(positive, et), model.score((positive, candidates), et, mode=mode),
                                             args.adversarial_temperature)
            else:
                candidates = sample_candidates(positive, et, n_negatives, data.n_node, side=sides[mode], known=known[sides[mode]],
                                               seed=(1111 + epoch) * len(starts) + i, candidates=typed)
                loss = negative_sampling_loss(model.score(positive, et), model.score((positive, candidates), et, mode=mode),
                                              args.adversarial_temperature, None if weights is None else weights[pick])
            loss.backward()
            optimizer.step()
            total += loss.detach()
        _hip.raise_if_index_errors(device)                            # (a row that knows every entity would have kept a positive)
        model.eval()
        with torch.no_grad():
            pos_score = model(data.train_idx[:, :drug_edges].contiguous(), data.train_et[:drug_edges])
            neg_score = model(drug_negatives.sample(2 * epoch + 1), data.train_et[:drug_edges])
        auprc, auroc, ap = relation_metrics(pos_score, neg_score, drug_ranges)
        return float(total) / len(starts), float(auprc.nanmean()), float(auroc.nanmean()), float(ap.nanmean())

    for epoch in range(args.epochs):
        t0 = time.time()
        loss, auprc, auroc, ap = (train_batched if batched else train)(epoch)
        torch.cuda.synchronize()
        print("{:3d}   loss:{:0.4f}   auprc:{:0.4f}   auroc:{:0.4f}   ap@50:{:0.4f}    time:{:0.2f}s".format(
            epoch, loss, auprc, auroc, ap, time.time() - t0))

    if args.rank:
        lists = [(data.train_idx, data.train_et)]
        known = {"tail": KnownPairs(lists, data.n_node, data.n_edge_type),                      # rows keyed (relation, head)
                 "head": KnownPairs([(ei.flip(0), et) for ei, et in lists], data.n_node, data.n_edge_type)}   # (relation, tail)
        e = data.train_idx.shape[1]
        pick = torch.randperm(e, generator=torch.Generator().manual_seed(7))[:args.rank_sample].to(device)
        if typed is not None:
            pick = pick[torch.sort(data.train_et[pick], stable=True).indices]      # a workgroup's queries share a range
        sample, et = data.train_idx[:, pick].contiguous(), data.train_et[pick].contiguous()
        against = "{} entities".format(data.n_node)
        if typed is not None:
            width = (typed[:, 1] - typed[:, 0])[et]
            against = "{}..{} candidates of the relation's type, {:.0f} on average".format(
                int(width.min()), int(width.max()), width.double().mean().item())
        for side in ("tail", "head"):
            greater, ties = model.rank(sample, et, side=side, known=known[side], candidates=typed)
            m = ranking_metrics(greater, ties, et, data.n_edge_type)
            print("filtered ranking, {} side ({} triples against {}):   mrr:{:0.4f}   hits@1:{:0.4f}   hits@3:{:0.4f}   "
                  "hits@10:{:0.4f}".format(side, sample.shape[1], against, m["mrr_all"].item(), m["hits@1_all"].item(),
                                           m["hits@3_all"].item(), m["hits@10_all"].item()))


if __name__ == "__main__":
    main()
