#!/usr/bin/env python3
"""Generate the golden input/output vectors under tests/golden/ FROM THE REFERENCE ITSELF.

Run only in the build container (needs /root/reference, which never travels):

    python tests/golden/make_golden.py            # the forward fixtures (re-drawn from the unseeded global RNG: they move)
    python tests/golden/make_golden.py --grads    # the gradient fixtures only: reads the forward fixtures, writes new files

The reference's hot path (gripnet/layers.py, gripnet/decoder.py) imports three third-party
symbols that are not installed here (torch_geometric.utils.add_remaining_self_loops,
torch_geometric.nn.conv.MessagePassing, torch_scatter.scatter_add).  This script registers
small stand-ins for exactly those symbols (PyG-1.x semantics), imports the
reference package unmodified, runs it on seeded inputs and stores inputs, weights and outputs
as .npz fixtures.  The fixtures are data; no reference source is stored.

The stand-ins are independently cross-checked by tests/test_oracle_golden.py through the dense
closed forms of SURVEY.md App. A (a dense normalised adjacency product etc.).
"""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"


# --------------------------------------------------------------------------------------
# stand-ins for the three missing third-party symbols
# --------------------------------------------------------------------------------------
def _scatter_add(src, index, dim=0, out=None, dim_size=None):
    assert dim == 0
    if out is None:
        n = int(index.max()) + 1 if dim_size is None else dim_size
        out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    return out.index_add_(0, index, src)


def _add_remaining_self_loops(edge_index, edge_weight=None, fill_value=1, num_nodes=None):
    n = int(edge_index.max()) + 1 if num_nodes is None else num_nodes
    row, col = edge_index
    keep = row != col
    loops = torch.arange(n, dtype=edge_index.dtype, device=edge_index.device)
    if edge_weight is not None:
        loop_w = torch.full((n,), fill_value, dtype=edge_weight.dtype, device=edge_weight.device)
        loop_w[row[~keep]] = edge_weight[~keep]
        edge_weight = torch.cat([edge_weight[keep], loop_w])
    edge_index = torch.cat([edge_index[:, keep], torch.stack([loops, loops])], dim=1)
    return edge_index, edge_weight


class _MessagePassing(torch.nn.Module):
    """PyG-1.x propagate: gather by name suffix, aggregate at edge_index[1], then update."""

    def __init__(self, aggr="add", flow="source_to_target", node_dim=0):
        super().__init__()
        assert aggr in ("add", "mean") and flow == "source_to_target" and node_dim == 0
        self.aggr = aggr
        self._msg_names = list(inspect.signature(self.message).parameters)
        self._upd_names = list(inspect.signature(self.update).parameters)[1:]

    def propagate(self, edge_index, size=None, **kw):
        n = None
        args = []
        for name in self._msg_names:
            if name.endswith("_j") or name.endswith("_i"):
                t = kw[name[:-2]]
                n = t.size(0)
                args.append(t.index_select(0, edge_index[0 if name.endswith("_j") else 1]))
            elif name == "edge_index":
                args.append(edge_index)
            else:
                args.append(kw[name])
        msg = self.message(*args)
        out = torch.zeros((n,) + tuple(msg.shape[1:]), dtype=msg.dtype).index_add_(0, edge_index[1], msg)
        if self.aggr == "mean":
            cnt = torch.zeros(n, dtype=msg.dtype).index_add_(
                0, edge_index[1], torch.ones(edge_index.shape[1], dtype=msg.dtype))
            out = out / cnt.clamp(min=1).view(-1, 1)
        return self.update(out, **{k: kw[k] for k in self._upd_names})


def _install_standins():
    sys.dont_write_bytecode = True
    tg = types.ModuleType("torch_geometric")
    tg_utils = types.ModuleType("torch_geometric.utils")
    tg_nn = types.ModuleType("torch_geometric.nn")
    tg_conv = types.ModuleType("torch_geometric.nn.conv")
    ts = types.ModuleType("torch_scatter")
    tg_utils.add_remaining_self_loops = _add_remaining_self_loops
    tg_conv.MessagePassing = _MessagePassing
    ts.scatter_add = _scatter_add
    tg.utils, tg.nn, tg_nn.conv = tg_utils, tg_nn, tg_conv
    sys.modules.update({
        "torch_geometric": tg, "torch_geometric.utils": tg_utils, "torch_geometric.nn": tg_nn,
        "torch_geometric.nn.conv": tg_conv, "torch_scatter": ts,
    })
    sys.path.insert(0, REFERENCE)


# --------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


class Case:
    def __init__(self, name, **meta):
        self.name, self.meta, self.arrays = name, meta, {}

    def put(self, key, value):
        self.arrays[key] = _np(value)

    def put_state(self, prefix, module):
        for k, v in module.state_dict().items():
            self.arrays["sd.{}{}".format(prefix, k)] = _np(v)

    def save(self):
        path = os.path.join(HERE, self.name + ".npz")
        np.savez_compressed(path, meta=np.array(json.dumps(self.meta)), **self.arrays)
        print("wrote", os.path.relpath(path, REPO), "{:.1f} KB".format(os.path.getsize(path) / 1024))


def main():
    _install_standins()
    from gripnet.layers import myGCN, myRGCN, homoGraph, interGraph  # the reference, unmodified
    from gripnet.decoder import multiRelaInnerProductDecoder, multiClassInnerProductDecoder
    from gripnet import utils as ref_utils

    sys.path.insert(0, REPO)
    from gripnet_amd.synth import make_pose, make_nc

    torch.set_grad_enabled(False)
    gen = torch.Generator().manual_seed(20261003)

    def randn(*s):
        return torch.randn(*s, generator=gen)

    def randint(hi, *s):
        return torch.randint(0, hi, s, generator=gen)

    # (0) hand-checkable known answer -------------------------------------------------
    c = Case("norm_known")
    ei = torch.tensor([[0, 1], [1, 0]])
    ei2, nrm = myGCN.norm(ei, 3, None, improved=True, dtype=torch.float32)
    c.put("edge_index", ei); c.put("out.edge_index", ei2); c.put("out.norm", nrm)
    c.meta.update(num_nodes=3, improved=True)
    c.save()

    # (1) norm edge cases ------------------------------------------------------------
    c = Case("norm_cases")
    specs = []
    n = 9
    base = randint(n, 2, 40)
    base[:, 5] = torch.tensor([3, 3]); base[:, 17] = torch.tensor([3, 3])   # two self loops at node 3
    base[:, 20] = torch.tensor([6, 6])
    base[:, 8] = base[:, 7]                                                # duplicate edge
    base[base == 8] = 2                                                    # node 8 isolated
    w = torch.rand(40, generator=gen) + 0.25
    for i, (weights, improved) in enumerate([(None, False), (w, False), (w, True), (None, True)]):
        ei2, nrm = myGCN.norm(base, n, weights, improved=improved, dtype=torch.float32)
        c.put("c{}.edge_index".format(i), base)
        if weights is not None:
            c.put("c{}.edge_weight".format(i), weights)
        c.put("c{}.out.edge_index".format(i), ei2); c.put("c{}.out.norm".format(i), nrm)
        specs.append(dict(num_nodes=n, improved=improved, weighted=weights is not None))
    # directed graph, zero-in-degree nodes only get their self loop
    d = torch.stack([randint(4, 30), randint(12, 30)])
    ei2, nrm = myGCN.norm(d, 12, None, improved=False, dtype=torch.float32)
    c.put("c4.edge_index", d); c.put("c4.out.edge_index", ei2); c.put("c4.out.norm", nrm)
    specs.append(dict(num_nodes=12, improved=False, weighted=False))
    c.meta["cases"] = specs
    c.save()

    # (2) myGCN.forward, cached re-use ------------------------------------------------
    c = Case("gcn_forward")
    n, fin, fout = 37, 24, 16
    conv = myGCN(fin, fout, cached=True)
    conv.bias.data = randn(fout) * 0.1
    ei = randint(n, 2, 300)
    w = torch.rand(300, generator=gen) + 0.5
    x0, x1 = randn(n, fin), randn(n, fin)
    c.put("edge_index", ei); c.put("edge_weight", w); c.put("x0", x0); c.put("x1", x1)
    c.put_state("", conv)
    c.put("out.y0", conv(x0, ei, w))
    c.put("out.y1", conv(x1, ei, w))          # served from the cache
    conv_nb = myGCN(fin, 20, cached=False, bias=False)
    c.put_state("nb.", conv_nb)
    c.put("out.y_nobias_unweighted", conv_nb(x0, ei))
    c.meta.update(n=n, fin=fin, fout=fout)
    c.save()

    # (3) interGraph -------------------------------------------------------------------
    c = Case("inter_cases")
    ns, nt, sd = 30, 11, 20
    x = randn(ns, sd)
    ei = torch.stack([randint(ns, 70), randint(nt - 2, 70)])   # targets nt-2, nt-1 isolated
    w = torch.rand(70, generator=gen) + 0.5
    c.put("x", x); c.put("edge_index", ei); c.put("edge_weight", w)
    variants = []

    def run_inter(tag, target_dim, tfd, if_one_external, weights, if_relu, mod):
        m = interGraph(sd, target_dim, nt, target_feat_dim=tfd, if_one_external=if_one_external)
        m.conv.bias.data = randn(target_dim) * 0.2
        before = ei.clone()
        y = m(x, ei, weights, if_relu=if_relu, mod=mod)
        assert torch.equal(before, ei)
        c.put_state(tag + ".", m)
        c.put(tag + ".out", y)
        variants.append(dict(tag=tag, target_dim=target_dim, target_feat_dim=tfd,
                             if_one_external=if_one_external, weighted=weights is not None,
                             if_relu=if_relu, mod=mod))

    run_inter("cat", 16, 32, True, None, True, "cat")
    run_inter("cat_w_norelu", 16, 32, True, w, False, "cat")
    run_inter("add_eq", 16, 16, True, None, True, "add")
    run_inter("add_down", 16, 32, True, w, True, "add")
    run_inter("noext", 16, 32, False, None, True, "add")
    c.meta.update(n_source=ns, n_target=nt, source_dim=sd, variants=variants)
    c.save()

    # (4) myRGCN -----------------------------------------------------------------------
    c = Case("rgcn_cases")
    n, fin, fout, R, B = 23, 12, 8, 6, 4
    sizes = [9, 0, 14, 5, 0, 11]          # relations 1 and 4 empty
    blocks = []
    for s in sizes:
        e = torch.stack([randint(n, s), randint(n - 3, s)])   # nodes n-3.. have zero in-degree
        if s > 2:
            e[:, 1] = e[:, 0]                                  # duplicate edge
        blocks.append(e)
    ei = torch.cat(blocks, dim=1)
    rl = ref_utils.get_range_list(blocks)
    et = torch.cat([torch.full((s,), r, dtype=torch.long) for r, s in enumerate(sizes)])
    x = randn(n, fin)
    c.put("x", x); c.put("edge_index", ei); c.put("edge_type", et); c.put("range_list", rl)
    variants = []
    for tag, after_relu, bias in [("plain", False, False), ("after_relu", True, False), ("bias", False, True)]:
        m = myRGCN(fin, fout, R, B, after_relu, bias=bias)
        if bias:
            m.bias.data = randn(fout) * 0.3
        c.put_state(tag + ".", m)
        c.put(tag + ".out", m(x, ei, et, rl))
        variants.append(dict(tag=tag, after_relu=after_relu, bias=bias))
    c.meta.update(n=n, fin=fin, fout=fout, R=R, B=B, variants=variants)
    c.save()

    # (5) homoGraph ---------------------------------------------------------------------
    c = Case("homo_cases")
    n = 31
    ei = randint(n, 2, 200)
    w = torch.rand(200, generator=gen) + 0.5
    x = randn(n, 12)
    c.put("edge_index", ei); c.put("edge_weight", w); c.put("x", x)
    variants = []
    m = homoGraph([12, 8, 8])
    c.put_state("gcn2.", m)
    c.put("gcn2.out_cat", m(x, ei, w, if_catout=True))
    m2 = homoGraph([12, 8, 8]); m2.load_state_dict(m.state_dict())
    c.put("gcn2.out_nocat", m2(x, ei, w, if_catout=False))
    variants.append(dict(tag="gcn2", nhid=[12, 8, 8], start_graph=False, multi_relational=False))
    m = homoGraph([10, 16], start_graph=True, in_dim=n)
    c.put_state("start1.", m)
    c.put("start1.out_cat", m(torch.zeros(1), ei, None, if_catout=True))   # x is ignored
    variants.append(dict(tag="start1", nhid=[10, 16], start_graph=True, multi_relational=False))
    # relational stack, two layers
    R = 3
    blocks = [torch.stack([randint(n, s), randint(n, s)]) for s in (40, 25, 60)]
    rei = torch.cat(blocks, dim=1)
    rl = ref_utils.get_range_list(blocks)
    ret = torch.cat([torch.full((b.shape[1],), r, dtype=torch.long) for r, b in enumerate(blocks)])
    c.put("rel.edge_index", rei); c.put("rel.edge_type", ret); c.put("rel.range_list", rl)
    m = homoGraph([12, 8, 6], multi_relational=True, n_rela=R, n_base=5)
    c.put_state("rgcn2.", m)
    c.put("rgcn2.out_cat", m(x, rei, edge_type=ret, range_list=rl, if_catout=True))
    variants.append(dict(tag="rgcn2", nhid=[12, 8, 6], start_graph=False, multi_relational=True, n_rela=R, n_base=5))
    c.meta.update(n=n, variants=variants)
    c.save()

    # (6) decoders ----------------------------------------------------------------------
    c = Case("decoder_cases")
    n, F, R = 19, 80, 7
    z = randn(n, F).abs()
    E = 120
    ei = randint(n, 2, E)
    ei[:, 3] = ei[:, 2]                     # repeated edge
    ei[1, 10] = ei[0, 10]                   # u == v
    et = randint(R, E)
    dm = multiRelaInnerProductDecoder(F, R)
    c.put("z", z); c.put("edge_index", ei); c.put("edge_type", et)
    c.put_state("dmt.", dm)
    c.put("dmt.out_sigmoid", dm(z, ei, et)); c.put("dmt.out_logits", dm(z, ei, et, sigmoid=False))
    mc = multiClassInnerProductDecoder(F, 5)
    nodes = randint(n, 30)
    c.put("node_list", nodes); c.put_state("mcip.", mc)
    c.put("mcip.out_softmax", mc(z, nodes)); c.put("mcip.out_logits", mc(z, nodes, softmax=False))
    c.meta.update(n=n, F=F, R=R, n_class=5)
    c.save()

    # (7) end-to-end pose pipeline (GripNet-pose.py:86-99,117-138) ----------------------
    for scale in ("tiny", "small"):
        c = Case("pose_" + scale)
        data = make_pose(scale)
        gg_nhids, gd_out = [32, 16, 16], [16, 32]
        dd_nhids = [sum(gd_out), 32]
        gg = homoGraph(gg_nhids, start_graph=True, in_dim=data.n_g_node)
        gd = interGraph(sum(gg_nhids), gd_out[0], data.n_d_node, target_feat_dim=gd_out[-1])
        dd = homoGraph(dd_nhids, multi_relational=True, n_rela=data.n_dd_edge_type)
        dmt = multiRelaInnerProductDecoder(sum(dd_nhids), data.n_dd_edge_type)
        gg.conv_list[0].bias.data = randn(16) * 0.1
        gg.conv_list[1].bias.data = randn(16) * 0.1
        gd.conv.bias.data = randn(16) * 0.1
        for k in ("gg_edge_index", "edge_weight", "gd_edge_index", "train_idx", "train_et", "train_range"):
            c.put(k, getattr(data, k))
        for tag, mod in (("gg.", gg), ("gd.", gd), ("dd.", dd), ("dmt.", dmt)):
            c.put_state(tag, mod)
        z_gg = gg(torch.zeros(1), data.gg_edge_index, edge_weight=data.edge_weight, if_catout=True)
        z_gd = gd(z_gg, data.gd_edge_index, mod="cat", if_relu=True)
        z_dd = dd(z_gd, data.train_idx, edge_type=data.train_et, range_list=data.train_range, if_catout=True)
        c.put("out.z_gg", z_gg); c.put("out.z_gd", z_gd); c.put("out.z_dd", z_dd)
        c.put("out.score", dmt(z_dd, data.train_idx, data.train_et))
        c.put("out.logits", dmt(z_dd, data.train_idx, data.train_et, sigmoid=False))
        c.meta.update(n_g=data.n_g_node, n_d=data.n_d_node, R=data.n_dd_edge_type,
                      gg_nhids=gg_nhids, gd_out=gd_out, dd_nhids=dd_nhids, synth=scale, seed=7)
        c.save()

    # (8) aminer-style and freebase-c-style pipelines, tiny ------------------------------
    data = make_nc("tiny")
    c = Case("aminer_tiny")     # GripNet-aminer.py:96-108,124-130 with smaller widths
    pp_nh, pa_out = [16, 8, 8], [8, 8]
    aa_nh = [sum(pa_out), 16, 4]
    pp = homoGraph(pp_nh, start_graph=True, in_dim=data.n_p_node)
    pa = interGraph(sum(pp_nh), pa_out[0], data.n_a_node, target_feat_dim=pa_out[-1])
    aa = homoGraph(aa_nh)
    mcip = multiClassInnerProductDecoder(sum(aa_nh), data.n_a_type)
    nodes = randint(data.n_a_node, 15)
    for k in ("pp_edge_idx", "pa_edge_idx", "aa_edge_idx", "pp_edge_weight", "aa_edge_weight"):
        c.put(k, getattr(data, k))
    c.put("node_list", nodes)
    for tag, mod in (("pp.", pp), ("pa.", pa), ("aa.", aa), ("mcip.", mcip)):
        c.put_state(tag, mod)
    z = pp(torch.zeros(1), data.pp_edge_idx, edge_weight=data.pp_edge_weight, if_catout=True)
    z = pa(z, data.pa_edge_idx, if_relu=True, mod="cat")
    z = aa(z, data.aa_edge_idx, edge_weight=data.aa_edge_weight, if_catout=True)
    c.put("out.z", z); c.put("out.score", mcip(z, nodes))
    c.meta.update(pp_nhids=pp_nh, pa_out=pa_out, aa_nhids=aa_nh, n_p=data.n_p_node, n_a=data.n_a_node,
                  n_class=data.n_a_type)
    c.save()

    c = Case("freebase_c_tiny")  # GripNet-freebase-c.py:102-136,150-165 with smaller widths
    pp_nh, qq_nh, pa_out = [16, 8, 8], [16, 8, 8], [8, 8]
    aa_nh = [pa_out[-1], 4]
    pp = homoGraph(pp_nh, start_graph=True, in_dim=data.n_p_node)
    pa = interGraph(sum(pp_nh), pa_out[0], data.n_a_node, target_feat_dim=pa_out[-1], if_one_external=False)
    qq = homoGraph(qq_nh, start_graph=True, in_dim=data.n_q_node)
    qa = interGraph(sum(qq_nh), pa_out[0], data.n_a_node, target_feat_dim=pa_out[-1], if_one_external=False)
    aae = randn(data.n_a_node, aa_nh[0])
    aa = homoGraph(aa_nh)
    mcip = multiClassInnerProductDecoder(aa_nh[-1], data.n_a_type)
    for k in ("pp_edge_idx", "pa_edge_idx", "qq_edge_idx", "qa_edge_idx", "aa_edge_idx",
              "pp_edge_weight", "qq_edge_weight", "aa_edge_weight"):
        c.put(k, getattr(data, k))
    c.put("node_list", nodes); c.put("aa_embeddings", aae)
    for tag, mod in (("pp.", pp), ("pa.", pa), ("qq.", qq), ("qa.", qa), ("aa.", aa), ("mcip.", mcip)):
        c.put_state(tag, mod)
    z = pa(pp(torch.zeros(1), data.pp_edge_idx, edge_weight=data.pp_edge_weight, if_catout=True),
           data.pa_edge_idx, mod="add", if_relu=True)
    z1 = qa(qq(torch.zeros(1), data.qq_edge_idx, edge_weight=data.qq_edge_weight, if_catout=True),
            data.qa_edge_idx, mod="add", if_relu=True)
    z = aa((z + z1 + aae) / 3, data.aa_edge_idx, edge_weight=data.aa_edge_weight)
    c.put("out.z", z); c.put("out.score", mcip(z, nodes))
    c.meta.update(pp_nhids=pp_nh, qq_nhids=qq_nh, pa_out=pa_out, aa_nhids=aa_nh, n_p=data.n_p_node,
                  n_q=data.n_q_node, n_a=data.n_a_node, n_class=data.n_a_type)
    c.save()

    # (9) layout helpers (utils.py:132-148,168-198) --------------------------------------
    c = Case("layout_helpers")
    raw = [torch.stack([randint(20, s), randint(20, s)]) for s in (6, 0, 9, 4)]
    for i, r in enumerate(raw):
        c.put("raw{}".format(i), r)
    np.random.seed(4242)
    outs = ref_utils.process_edge_multirelational(raw, p=0.7)
    for k, v in zip(("train_idx", "train_et", "train_range", "test_idx", "test_et", "test_range"), outs):
        c.put("out." + k, v)
    c.put("out.bidir", ref_utils.to_bidirection(raw[0]))
    c.meta.update(n_raw=len(raw), p=0.7, np_seed=4242)
    c.save()

    # (10) freebase-a and freebase-b pipelines, tiny (added after every earlier case: their vectors do not move) -----
    c = Case("freebase_a_tiny")  # GripNet-freebase-a.py:94,101-104,120-122 with smaller widths: one supervertex, no catout
    pp_nh = [16, 8, 8]
    pp = homoGraph(pp_nh, start_graph=True, in_dim=data.n_a_node)
    mcip = multiClassInnerProductDecoder(pp_nh[-1], data.n_a_type)
    for k in ("aa_edge_idx", "aa_edge_weight"):
        c.put(k, getattr(data, k))
    c.put("node_list", nodes)
    for tag, mod in (("pp.", pp), ("mcip.", mcip)):
        c.put_state(tag, mod)
    z = pp(torch.zeros(1), data.aa_edge_idx, edge_weight=data.aa_edge_weight)
    c.put("out.z", z); c.put("out.score", mcip(z, nodes)); c.put("out.logits", mcip(z, nodes, softmax=False))
    c.meta.update(pp_nhids=pp_nh, n_a=data.n_a_node, n_class=data.n_a_type)
    c.save()

    c = Case("freebase_b_tiny")  # GripNet-freebase-b.py:96-98,112-117,129-135 with smaller widths (pa_out of equal halves)
    pp_nh, pa_out = [16, 8, 8], [16, 16]
    aa_nh = [sum(pa_out), 16, 4]
    pp = homoGraph(pp_nh, start_graph=True, in_dim=data.n_p_node)
    pa = interGraph(sum(pp_nh), pa_out[0], data.n_a_node, target_feat_dim=pa_out[-1])
    aa = homoGraph(aa_nh)
    mcip = multiClassInnerProductDecoder(sum(aa_nh), data.n_a_type)
    for k in ("pp_edge_idx", "pa_edge_idx", "aa_edge_idx", "pp_edge_weight", "aa_edge_weight"):
        c.put(k, getattr(data, k))
    c.put("node_list", nodes)
    for tag, mod in (("pp.", pp), ("pa.", pa), ("aa.", aa), ("mcip.", mcip)):
        c.put_state(tag, mod)
    z = pp(torch.zeros(1), data.pp_edge_idx, edge_weight=data.pp_edge_weight, if_catout=True)
    z = pa(z, data.pa_edge_idx, if_relu=True, mod="cat")
    z = aa(z, data.aa_edge_idx, edge_weight=data.aa_edge_weight, if_catout=True)
    c.put("out.z", z); c.put("out.score", mcip(z, nodes))
    c.meta.update(pp_nhids=pp_nh, pa_out=pa_out, aa_nhids=aa_nh, n_p=data.n_p_node, n_a=data.n_a_node,
                  n_class=data.n_a_type)
    c.save()

    # (11) the remaining helpers the drivers import by name (utils.py:13-25,151-165,201-247); added last -----
    c = Case("utils_helpers")
    sp = ref_utils.sparse_id(7)
    c.put("sparse_id.indices", sp._indices()); c.put("sparse_id.values", sp._values())
    c.put("sparse_id.shape", np.asarray(sp.shape)); c.put("sparse_id.dense", sp.to_dense())
    xn = randn(6, 5)
    c.put("normalize.in", xn); c.put("normalize.out", ref_utils.normalize(xn))
    both = ref_utils.to_bidirection(torch.stack([randint(30, 25), randint(30, 25)]))
    c.put("process_edge.in", both)
    np.random.seed(777)
    tr, te = ref_utils.process_edge(both)
    c.put("process_edge.train", tr); c.put("process_edge.test", te)
    node_lists = [randint(100, s) for s in (11, 0, 23, 5)]
    for i, nl in enumerate(node_lists):
        c.put("nodes{}".format(i), nl)
    np.random.seed(778)
    outs = ref_utils.process_node_multilabel(node_lists)
    for k, v in zip(("train_idx", "train_class", "train_range", "test_idx", "test_class", "test_range"), outs):
        c.put("multilabel." + k, v)
    c.meta.update(n=7, seed_edge=777, seed_nodes=778, n_lists=len(node_lists),
                  sparse_layout=str(sp.layout), sparse_dtype=str(sp.dtype), sparse_device=str(sp.device))
    c.save()

    # (12) what every caller imports from the package, by name: {script: {module: [names]}} (names only, as data) -----
    import ast
    callers = ["GripNet-pose.py", "GripNet-aminer.py", "GripNet-freebase-a.py", "GripNet-freebase-b.py",
               "GripNet-freebase-c.py", "GripNet-freebase-d.py", "baselines/LP_baselines/rgcn_pose.py",
               "baselines/LP_baselines/dmt_pose.py", "baselines/LP_baselines/TransE_DistMult_ComplEx_RotatE.py"]
    names = {}
    for rel in callers:
        with open(os.path.join(REFERENCE, rel)) as f:
            tree = ast.parse(f.read())
        per = {}
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "gripnet":
                per.setdefault(node.module, []).extend(a.name for a in node.names)
        names[rel] = {m: sorted(set(v)) for m, v in sorted(per.items())}
    public = {}                                  # every top-level def / class / constant of the three library modules
    for mod in ("utils", "layers", "decoder"):
        with open(os.path.join(REFERENCE, "gripnet", mod + ".py")) as f:
            tree = ast.parse(f.read())
        found = []
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                found.append(node.name)
            elif isinstance(node, ast.Assign):
                found.extend(t.id for t in node.targets if isinstance(t, ast.Name))
        public["gripnet." + mod] = sorted(found)
    names["__library_top_level__"] = public
    path = os.path.join(HERE, "driver_imports.json")
    with open(path, "w") as f:
        json.dump(names, f, indent=1, sort_keys=True)
    print("wrote", os.path.relpath(path, REPO))


# --------------------------------------------------------------------------------------
# gradient fixtures: the reference's own loss.backward(), in fp32 and after .double()
# --------------------------------------------------------------------------------------
# The self-check holds the reference's fp32 gradients to 1e-5 of float64 at the gradient's largest entry, a tenth of the
# bar of the GPU tests.  One gradient cannot meet it: the reference adds the 8,878 triples of pose_small's largest relation
# one after the other in fp32, twice (positives 0.198, negatives -0.186 at the largest entry, 0.049 left after they cancel);
# measured 1.0e-5 ... 1.9e-5 over several negative lists and runs (the threaded sums differ from run to run).  It is held to
# 3e-5; the GPU tests' bar against float64 stays 1e-4.
FP32_DISTANCE = {("pose_small_grad", "dmt.weight"): 3e-5}
ROW_TABLES = ("embedding", "target_feat", "aa_embeddings", "x", "z")   # 2-D per-node tables: checked per row as well


def is_row_table(key, grad):
    return grad.dim() == 2 and key.split(".")[-1] in ROW_TABLES


def grads_main():
    """`--grads`: writes <name>_grad.npz next to the forward fixtures and decoder_saturated.npz, and nothing else.  The
    modules are the reference's, built fresh per precision and loaded from the stored state dicts; inputs come from the
    stored fixtures; everything drawn here (negative lists, labels, projections, the saturated case) comes from one
    seeded generator and is stored.  Every case is run in fp32 and again in float64."""
    _install_standins()
    from gripnet.layers import myGCN, myRGCN, homoGraph, interGraph  # the reference, unmodified
    from gripnet.decoder import multiRelaInnerProductDecoder, multiClassInnerProductDecoder
    from gripnet.utils import EPS

    gen = torch.Generator().manual_seed(20261016)

    def load(name):
        with np.load(os.path.join(HERE, name + ".npz")) as f:
            return {k: torch.from_numpy(f[k]) for k in f.files if k != "meta"}, json.loads(str(f["meta"]))

    def loaded(module, arrays, prefix):
        full = "sd." + prefix
        module.load_state_dict({k[len(full):]: v for k, v in arrays.items() if k.startswith(full)})
        return module

    def run_both(c, tag, build, forward, leaves=None, check=True, keep32=True):
        """build() -> {key prefix: module} (made under the current default dtype); forward(mods, leaves, cast) -> loss.
        Stores <tag>loss32/64 and <tag>grad32/64.<key>; returns the fp32 run's (loss, grads)."""
        runs = {}
        for bits, dtype in ((32, torch.float32), (64, torch.float64)):
            torch.set_default_dtype(dtype)
            try:
                mods = build()
                lv = {k: v.to(dtype).clone().requires_grad_(True) for k, v in (leaves or {}).items()}
                loss = forward(mods, lv, lambda t: t.to(dtype))
                loss.backward()
            finally:
                torch.set_default_dtype(torch.float32)
            grads = {p + k: q.grad for p, m in mods.items() for k, q in
                     ([("", m)] if isinstance(m, torch.nn.Parameter) else m.named_parameters())}
            grads.update({k: v.grad for k, v in lv.items()})
            assert loss.dtype == dtype and all(g is None or g.dtype == dtype for g in grads.values())
            runs[bits] = (loss.detach(), grads)
        (l32, g32), (l64, g64) = runs[32], runs[64]
        assert torch.isfinite(l32) and torch.isfinite(l64)
        worst = (0.0, "-")
        if check:
            assert abs(float(l32) - float(l64)) <= 1e-6 * abs(float(l64)), (c.name, tag, float(l32), float(l64))
        c.put(tag + "loss32", l32)
        c.put(tag + "loss64", l64)
        for k in g64:
            if g64[k] is None:
                assert g32[k] is None
                c.meta.setdefault("no_grad", []).append(tag + k)
                continue
            a, b = g32[k].double(), g64[k]
            assert torch.isfinite(a).all() and torch.isfinite(b).all()
            scale = float(b.abs().max())
            if check:
                err = float((a - b).abs().max())
                bar = FP32_DISTANCE.get((c.name, tag + k), 1e-5)
                assert err <= bar * scale, (c.name, tag, k, err, scale)
                if bar != 1e-5:
                    c.meta.setdefault("fp32_distance", {})[tag + k] = bar
                worst = max(worst, (err / scale if scale else 0.0, k))
                if is_row_table(k, b):
                    rows = b.abs().amax(dim=1)
                    assert ((a - b).abs().amax(dim=1) <= 1e-5 * rows + 1e-6 * scale).all(), (c.name, tag, k, "per row")
            if keep32:
                c.put(tag + "grad32." + k, g32[k])
            else:                                   # 40 of the 52 mantissa bits (2^-41 relative; the tests ask 1e-9): the zeros compress
                b = torch.from_numpy(((b.numpy().view(np.int64) + (1 << 11)) & ~np.int64((1 << 12) - 1)).view(np.float64))
            c.put(tag + "grad64." + k, b)
        print("  {}{}: loss {:.6g}, worst fp32 distance {:.2e} ({})".format(c.name, " " + tag if tag else "", float(l64), *worst))
        return runs[32]

    # ---- callers: the loss the driver spells out ------------------------------------------------------------------
    for scale in ("tiny", "small"):
        a, meta = load("pose_" + scale)
        c = Case("pose_{}_grad".format(scale), forward="pose_" + scale)
        neg = torch.randint(0, meta["n_d"], tuple(a["train_idx"].shape), generator=gen)
        c.put("neg_index", neg.to(torch.int16 if meta["n_d"] < 2 ** 15 else torch.int64))

        def build():
            dd_nhids = meta["dd_nhids"]
            return {"gg.": loaded(homoGraph(meta["gg_nhids"], start_graph=True, in_dim=meta["n_g"]), a, "gg."),
                    "gd.": loaded(interGraph(sum(meta["gg_nhids"]), meta["gd_out"][0], meta["n_d"],
                                             target_feat_dim=meta["gd_out"][-1]), a, "gd."),
                    "dd.": loaded(homoGraph(dd_nhids, multi_relational=True, n_rela=meta["R"]), a, "dd."),
                    "dmt.": loaded(multiRelaInnerProductDecoder(sum(dd_nhids), meta["R"]), a, "dmt.")}

        def forward(m, lv, cast):                                       # GripNet-pose.py:117-142
            z = m["gg."](torch.zeros(1), a["gg_edge_index"], edge_weight=cast(a["edge_weight"]), if_catout=True)
            z = m["gd."](z, a["gd_edge_index"], mod="cat", if_relu=True)
            z = m["dd."](z, a["train_idx"], edge_type=a["train_et"], range_list=a["train_range"], if_catout=True)
            pos_score = m["dmt."](z, a["train_idx"], a["train_et"])
            neg_score = m["dmt."](z, neg, a["train_et"])
            return -torch.log(pos_score + EPS).mean() - torch.log(1 - neg_score + EPS).mean()

        run_both(c, "", build, forward, keep32=scale == "tiny")       # (small: 130 k gradients; grad64 alone, see keep32)
        c.save()

    def nc_case(name, build, forward):
        a, meta = load(name)
        c = Case(name + "_grad", forward=name)
        labels = torch.randint(0, meta["n_class"], tuple(a["node_list"].shape), generator=gen)
        c.put("labels", labels)

        def loss(m, lv, cast):                                          # GripNet-aminer.py:133
            score = forward(a, m, cast)
            return -torch.log(score[range(score.shape[0]), labels] + EPS).mean()

        run_both(c, "", lambda: build(a, meta), loss)
        c.save()

    def aminer_build(a, meta):
        return {"pp.": loaded(homoGraph(meta["pp_nhids"], start_graph=True, in_dim=meta["n_p"]), a, "pp."),
                "pa.": loaded(interGraph(sum(meta["pp_nhids"]), meta["pa_out"][0], meta["n_a"],
                                         target_feat_dim=meta["pa_out"][-1]), a, "pa."),
                "aa.": loaded(homoGraph(meta["aa_nhids"]), a, "aa."),
                "mcip.": loaded(multiClassInnerProductDecoder(sum(meta["aa_nhids"]), meta["n_class"]), a, "mcip.")}

    def aminer_forward(a, m, cast):                                     # GripNet-aminer.py:124-130
        z = m["pp."](torch.zeros(1), a["pp_edge_idx"], edge_weight=cast(a["pp_edge_weight"]), if_catout=True)
        z = m["pa."](z, a["pa_edge_idx"], if_relu=True, mod="cat")
        z = m["aa."](z, a["aa_edge_idx"], edge_weight=cast(a["aa_edge_weight"]), if_catout=True)
        return m["mcip."](z, a["node_list"])

    nc_case("aminer_tiny", aminer_build, aminer_forward)
    nc_case("freebase_b_tiny", aminer_build, aminer_forward)

    def fa_build(a, meta):
        return {"pp.": loaded(homoGraph(meta["pp_nhids"], start_graph=True, in_dim=meta["n_a"]), a, "pp."),
                "mcip.": loaded(multiClassInnerProductDecoder(meta["pp_nhids"][-1], meta["n_class"]), a, "mcip.")}

    def fa_forward(a, m, cast):                                         # GripNet-freebase-a.py:120-122
        z = m["pp."](torch.zeros(1), a["aa_edge_idx"], edge_weight=cast(a["aa_edge_weight"]))
        return m["mcip."](z, a["node_list"])

    nc_case("freebase_a_tiny", fa_build, fa_forward)

    def fc_build(a, meta):
        pa_out = meta["pa_out"]
        return {"pp.": loaded(homoGraph(meta["pp_nhids"], start_graph=True, in_dim=meta["n_p"]), a, "pp."),
                "pa.": loaded(interGraph(sum(meta["pp_nhids"]), pa_out[0], meta["n_a"], target_feat_dim=pa_out[-1],
                                         if_one_external=False), a, "pa."),
                "qq.": loaded(homoGraph(meta["qq_nhids"], start_graph=True, in_dim=meta["n_q"]), a, "qq."),
                "qa.": loaded(interGraph(sum(meta["qq_nhids"]), pa_out[0], meta["n_a"], target_feat_dim=pa_out[-1],
                                         if_one_external=False), a, "qa."),
                "aa_embeddings": torch.nn.Parameter(a["aa_embeddings"].to(torch.get_default_dtype()).clone()),
                "aa.": loaded(homoGraph(meta["aa_nhids"]), a, "aa."),
                "mcip.": loaded(multiClassInnerProductDecoder(meta["aa_nhids"][-1], meta["n_class"]), a, "mcip.")}

    def fc_forward(a, m, cast):                                         # GripNet-freebase-c.py:150-165
        z = m["pa."](m["pp."](torch.zeros(1), a["pp_edge_idx"], edge_weight=cast(a["pp_edge_weight"]), if_catout=True),
                     a["pa_edge_idx"], mod="add", if_relu=True)
        z1 = m["qa."](m["qq."](torch.zeros(1), a["qq_edge_idx"], edge_weight=cast(a["qq_edge_weight"]), if_catout=True),
                      a["qa_edge_idx"], mod="add", if_relu=True)
        z = m["aa."]((z + z1 + m["aa_embeddings"]) / 3, a["aa_edge_idx"], edge_weight=cast(a["aa_edge_weight"]))
        return m["mcip."](z, a["node_list"])

    nc_case("freebase_c_tiny", fc_build, fc_forward)

    # ---- layers: loss = (y * P).sum() with a stored random P, every variant of the forward fixtures -----------------
    def layer_case(c, tag, build, call, leaves, info):
        """call(mods, leaves, cast) -> y.  The projection is drawn at y's shape on the first (fp32) run and given the signs
        of that y: every element still carries its own random weight, and the loss is a sum of non-negative terms, so
        that `loss32 == loss64` to 1e-6 relative is a statement about the layer and not about how much of a signed sum
        cancels (with free signs the sums of these ~200 ... 600 terms cancel to a tenth and miss that bar by chance)."""
        proj = {}

        def forward(m, lv, cast):
            y = call(m, lv, cast)
            if "p" not in proj:
                sign = torch.where(y.detach() < 0, -1.0, 1.0).float()
                proj["p"] = sign * (0.25 + torch.randn(tuple(y.shape), generator=gen).abs())
            return (y * cast(proj["p"])).sum()

        run_both(c, tag + ".", build, forward, leaves)
        c.put(tag + ".proj", proj["p"])
        c.meta.setdefault("cases", []).append(dict(tag=tag, **info))

    a, meta = load("gcn_forward")
    c = Case("gcn_forward_grad", forward="gcn_forward")
    def build_wb():
        m = myGCN(meta["fin"], meta["fout"], cached=True)
        m.load_state_dict({"weight": a["sd.weight"], "bias": a["sd.bias"]})
        return {"": m}

    layer_case(c, "wb", build_wb,
               lambda m, lv, cast: m[""](lv["x"], a["edge_index"], cast(a["edge_weight"])), {"x": a["x0"]},
               dict(state="", fout=meta["fout"], bias=True, weighted=True))
    nb_state = {k[len("sd.nb."):]: v for k, v in a.items() if k.startswith("sd.nb.")}

    def build_nb():
        m = myGCN(meta["fin"], 20, cached=False, bias=False)
        m.load_state_dict(nb_state)
        return {"": m}

    layer_case(c, "nb", build_nb, lambda m, lv, cast: m[""](lv["x"], a["edge_index"]), {"x": a["x0"]},
               dict(state="nb.", fout=20, bias=False, weighted=False))
    c.save()

    a, meta = load("inter_cases")
    c = Case("inter_cases_grad", forward="inter_cases")
    for v in meta["variants"]:
        def build(v=v):
            return {"": loaded(interGraph(meta["source_dim"], v["target_dim"], meta["n_target"],
                                          target_feat_dim=v["target_feat_dim"], if_one_external=v["if_one_external"]),
                               a, v["tag"] + ".")}

        def call(m, lv, cast, v=v):
            return m[""](lv["x"], a["edge_index"], cast(a["edge_weight"]) if v["weighted"] else None,
                         if_relu=v["if_relu"], mod=v["mod"])

        layer_case(c, v["tag"], build, call, {"x": a["x"]}, dict(state=v["tag"] + "."))
    assert "add_down.grad64.target_feat_down" in c.arrays               # the only place it gets a gradient
    c.save()

    a, meta = load("rgcn_cases")
    c = Case("rgcn_cases_grad", forward="rgcn_cases")
    for v in meta["variants"]:
        layer_case(c, v["tag"],
                   lambda v=v: {"": loaded(myRGCN(meta["fin"], meta["fout"], meta["R"], meta["B"], v["after_relu"],
                                                  bias=v["bias"]), a, v["tag"] + ".")},
                   lambda m, lv, cast: m[""](lv["x"], a["edge_index"], a["edge_type"], a["range_list"]),
                   {"x": a["x"]}, dict(state=v["tag"] + "."))
    c.save()

    a, meta = load("homo_cases")
    c = Case("homo_cases_grad", forward="homo_cases")
    for tag, catout in (("gcn2_cat", True), ("gcn2_nocat", False)):
        layer_case(c, tag, lambda: {"": loaded(homoGraph([12, 8, 8]), a, "gcn2.")},
                   lambda m, lv, cast, catout=catout: m[""](lv["x"], a["edge_index"], cast(a["edge_weight"]), if_catout=catout),
                   {"x": a["x"]}, dict(state="gcn2.", if_catout=catout))
    layer_case(c, "start1", lambda: {"": loaded(homoGraph([10, 16], start_graph=True, in_dim=meta["n"]), a, "start1.")},
               lambda m, lv, cast: m[""](torch.zeros(1), a["edge_index"], None, if_catout=True), {},
               dict(state="start1.", if_catout=True))
    layer_case(c, "rgcn2",
               lambda: {"": loaded(homoGraph([12, 8, 6], multi_relational=True, n_rela=3, n_base=5), a, "rgcn2.")},
               lambda m, lv, cast: m[""](lv["x"], a["rel.edge_index"], edge_type=a["rel.edge_type"],
                                         range_list=a["rel.range_list"], if_catout=True),
               {"x": a["x"]}, dict(state="rgcn2.", if_catout=True))
    c.save()

    a, meta = load("decoder_cases")
    c = Case("decoder_cases_grad", forward="decoder_cases")
    for tag, sig in (("dmt_sigmoid", True), ("dmt_logits", False)):
        layer_case(c, tag, lambda: {"": loaded(multiRelaInnerProductDecoder(meta["F"], meta["R"]), a, "dmt.")},
                   lambda m, lv, cast, sig=sig: m[""](lv["z"], a["edge_index"], a["edge_type"], sigmoid=sig),
                   {"z": a["z"]}, dict(state="dmt.", sigmoid=sig))
    for tag, soft in (("mcip_softmax", True), ("mcip_logits", False)):
        layer_case(c, tag, lambda: {"": loaded(multiClassInnerProductDecoder(meta["F"], meta["n_class"]), a, "mcip.")},
                   lambda m, lv, cast, soft=soft: m[""](lv["z"], a["node_list"], softmax=soft),
                   {"z": a["z"]}, dict(state="mcip.", softmax=soft))
    c.save()

    # ---- saturated scores: DistMult + link loss where fp32 and float64 part ways ----------------------------------
    # Every triple of a relation lies in one band of the float64 logit: z = (row scale in [0.8, 1.2)) x (entries in [0.5, 1))
    # is non-negative, so a relation whose D entries have one sign has logits of that sign, about 18 x (0.64 ... 1.44) x
    # mean |D| with F = 32.  The asserts below are what holds the bands, not this estimate.
    c = Case("decoder_saturated")
    n, F, hot_only = 40, 32, [36, 37, 38, 39]
    bands = {"ordinary": [0, 1, 2], "hot": [3], "cold": [4], "frozen": [5]}
    sizes = [50, 40, 60, 50, 50, 40]
    R = len(sizes)
    z = (0.8 + 0.4 * torch.rand(n, 1, generator=gen)) * (0.5 + 0.5 * torch.rand(n, F, generator=gen))
    D = torch.empty(R, F)
    D[:3] = torch.randn(3, F, generator=gen) * torch.tensor([[0.3], [0.6], [0.9]])
    D[3] = 1.8 + torch.rand(F, generator=gen) * 0.4                     # about 22 ... 50: fp32 is at 1.0, float64 mostly is not
    D[4] = -(1.8 + torch.rand(F, generator=gen) * 0.4)                  # about -50 ... -22: s against EPS = 1e-13 matters
    D[5] = -(14 + torch.rand(F, generator=gen))                         # below -160: exp overflows, s == 0
    et = torch.cat([torch.full((s,), r, dtype=torch.long) for r, s in enumerate(sizes)])
    lists = []
    for _ in range(2):                                                  # positives, negatives
        ei = torch.randint(0, n - len(hot_only), (2, int(et.numel())), generator=gen)
        hot = (et == 3).nonzero().view(-1)
        ei[:, hot] = torch.randint(0, n, (2, int(hot.numel())), generator=gen)
        ei[0, hot[:4]] = torch.tensor(hot_only)                         # every hot-only node is in the list
        ei[1, hot[4:8]] = torch.tensor(hot_only)
        lists.append(ei)
    pos_index, neg_index = lists
    pos_index[:, 3] = pos_index[:, 2]                                   # a repeated triple
    pos_index[1, 10] = pos_index[0, 10]                                 # u == v
    for ei in lists:
        assert not torch.isin(ei[:, et != 3], torch.tensor(hot_only)).any()
    for k, v in (("z", z), ("sd.dmt.weight", D), ("pos_index", pos_index), ("neg_index", neg_index), ("edge_type", et)):
        c.put(k, v)
    logit64 = {}
    for name, ei in (("pos", pos_index), ("neg", neg_index)):
        lg = (z.double()[ei[0]] * z.double()[ei[1]] * D.double()[et]).sum(dim=1)
        sel = lambda band: torch.isin(et, torch.tensor(bands[band]))
        assert (lg[sel("ordinary")].abs() <= 4).all(), float(lg[sel("ordinary")].abs().max())
        assert (lg[sel("hot")] >= 20).all() and (lg[sel("cold")] <= -20).all() and (lg[sel("frozen")] <= -110).all()
        assert (lg[sel("cold")] > -110).all() and (lg[sel("cold")] > -80).any()
        assert not (((lg > 4) & (lg < 20)) | ((lg < -4) & (lg > -20))).any()
        logit64[name] = lg
        c.put(name + "_logit64", lg)
    kept = {}

    def build():
        dm = multiRelaInnerProductDecoder(F, R)
        dm.weight.data.copy_(D)
        return {"dmt.": dm}

    def forward(m, lv, cast):
        pos_score = m["dmt."](lv["z"], pos_index, et)
        neg_score = m["dmt."](lv["z"], neg_index, et)
        pos_score.retain_grad()
        neg_score.retain_grad()
        kept[pos_score.dtype] = (pos_score, neg_score)
        return -torch.log(pos_score + EPS).mean() - torch.log(1 - neg_score + EPS).mean()

    l32, g32 = run_both(c, "", build, forward, {"z": z}, check=False)
    ps, ns = kept[torch.float32]
    hot = et == 3
    assert (ps[hot] == 1).all() and (ns[hot] == 1).all()
    assert (ps >= 0).all() and (ps <= 1).all() and (ns >= 0).all() and (ns <= 1).all()
    assert (g32["dmt.weight"][3] == 0).all() and (g32["z"][hot_only] == 0).all()
    assert torch.isfinite(ps.grad).all() and torch.isfinite(ns.grad).all()
    assert float(ns.grad[hot].min()) > 1e10                              # 1 / (1 - 1 + EPS) / E
    for k, v in (("pos_score", ps), ("neg_score", ns), ("pos_score.grad", ps.grad), ("neg_score.grad", ns.grad)):
        c.put(k, v)
    c.meta.update(n=n, F=F, R=R, bands=bands, hot_only_nodes=hot_only, eps=EPS,
                  loss_differs_from_float64=abs(float(l32) - float(c.arrays["loss64"])))
    c.save()

    limit = 1 << 20
    for name in sorted(os.listdir(HERE)):
        if name.endswith("_grad.npz") or name == "decoder_saturated.npz":
            assert os.path.getsize(os.path.join(HERE, name)) < limit, name


if __name__ == "__main__":
    if sys.argv[1:] == ["--grads"]:
        grads_main()
    elif sys.argv[1:]:
        sys.exit("usage: make_golden.py [--grads]")
    else:
        main()
