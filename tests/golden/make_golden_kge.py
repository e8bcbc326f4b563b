#!/usr/bin/env python
"""Generate tests/golden/kge_cases.npz FROM THE REFERENCE'S OWN KGEModel.

    python tests/golden/make_golden_kge.py --reference <checkout of the reference>

Run only where the reference is checked out; never imported by a test.  The reference file
(baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py) is a script that loads a dataset and trains at import, so it
is parsed with ``ast`` and only its ``KGEModel`` class node is compiled, into a namespace that holds ``torch``, ``nn`` and
``F`` - the class as it stands, no stand-in.  The fixture is data only; no reference text is stored.

Per model two cases under ``torch.manual_seed``: the state dict, ``sample`` / ``et`` (sorted) / a fixed ``neg``, the
reference's ``out`` / ``out_neg`` in fp32 (and ``out64`` / ``out_neg64``), and ``loss32`` / ``loss64`` / ``grad32.*`` / ``grad64.*`` of both embedding tables
under the driver's loss (:266-268); the float64 run is the same class after ``.double()``."""
import argparse
import ast
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from kge_cases import EPS, MODELS, loss_expr            # noqa: E402

SOURCE = os.path.join("baselines", "LP_baselines", "TransE_DistMult_ComplEx_RotatE.py")
SIZES = [dict(tag="small", n=37, R=5, H=6, E=200, gamma=7.0), dict(tag="driver", n=120, R=12, H=32, E=1500, gamma=12.0)]


def reference_class(root):
    path = os.path.join(root, SOURCE)
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "KGEModel")
    space = {"torch": torch, "nn": nn, "F": F}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), space)
    return space["KGEModel"]


def triples(size, gen):
    n, R, E = size["n"], size["R"], size["E"]
    top = n - 2 if size["tag"] == "small" else n          # small: the last two entities are in no triple
    sample = torch.randint(0, top, (2, E), generator=gen)
    neg = torch.randint(0, top, (2, E), generator=gen)
    et = torch.randint(0, R, (E,), generator=gen)
    if size["tag"] == "small":
        et[et == 3] = 4                                    # relation 3 has no triple
        sample[1, 0] = sample[0, 0]                        # head == tail
        neg[1, 5] = neg[0, 5]
    return sample, neg, et.sort().values


def loss_of(model, sample, neg, et):
    neg_score = model(neg, et)                             # (the driver's order: negatives first)
    pos_score = model(sample, et)
    return loss_expr(pos_score, neg_score), pos_score, neg_score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "kge_cases.npz"))
    args = ap.parse_args()
    KGEModel = reference_class(args.reference)
    arrays, cases = {}, []
    for mi, name in enumerate(MODELS):
        for si, size in enumerate(SIZES):
            seed = 9000 + 10 * mi + si
            torch.manual_seed(seed)
            model = KGEModel(name, size["n"], size["R"], size["H"], size["gamma"])
            gen = torch.Generator().manual_seed(seed + 100)
            sample, neg, et = triples(size, gen)
            tag = "{}.{}.".format(name, size["tag"])
            for k, v in model.state_dict().items():
                arrays[tag + "sd." + k] = v.detach().clone().numpy()
            arrays[tag + "sample"], arrays[tag + "neg"], arrays[tag + "et"] = sample.numpy(), neg.numpy(), et.numpy()
            loss, pos, negs = loss_of(model, sample, neg, et)
            loss.backward()
            arrays[tag + "out"], arrays[tag + "out_neg"] = pos.detach().numpy(), negs.detach().numpy()
            arrays[tag + "loss32"] = loss.detach().numpy()
            grads32 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
            model64 = KGEModel(name, size["n"], size["R"], size["H"], size["gamma"])
            model64.load_state_dict(model.state_dict())
            model64 = model64.double()
            loss64, pos64, negs64 = loss_of(model64, sample, neg, et)
            loss64.backward()
            arrays[tag + "out64"], arrays[tag + "out_neg64"] = pos64.detach().numpy(), negs64.detach().numpy()
            arrays[tag + "loss64"] = loss64.detach().numpy()
            for k, p in model64.named_parameters():
                if p.grad is None:
                    continue
                arrays[tag + "grad32." + k], arrays[tag + "grad64." + k] = grads32[k].numpy(), p.grad.numpy()
                scale = float(p.grad.abs().max())
                assert float((grads32[k].double() - p.grad).abs().max()) <= 1e-5 * scale, (tag, k)
            used = torch.zeros(size["n"], dtype=torch.bool)
            used[sample.reshape(-1)] = True
            used[neg.reshape(-1)] = True
            cases.append(dict(size, tag=tag[:-1], size=size["tag"], model=name, seed=seed,
                              embedding_range=float(model.embedding_range.item()), entity_dim=model.entity_dim,
                              relation_dim=model.relation_dim, unused_entities=(~used).nonzero().view(-1).tolist(),
                              empty_relations=[r for r in range(size["R"]) if not bool((et == r).any())],
                              frozen=[k for k, p in model.named_parameters() if not p.requires_grad]))
    meta = dict(cases=cases, eps=EPS, source=SOURCE, source_lines="58-235, loss 266-268")
    np.savez_compressed(args.out, meta=np.array(json.dumps(meta)), **arrays)
    print("wrote {} ({} bytes, {} arrays)".format(args.out, os.path.getsize(args.out), len(arrays)))


if __name__ == "__main__":
    main()
