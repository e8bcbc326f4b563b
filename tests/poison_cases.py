"""A non-finite table row reaches only the outputs that read it: the cases of tests/test_poison_host.py and
tests/test_gpu_poison.py, their float64 references and the `check` both use.  Not a test module.

The contract.  One or two rows P of a launch's table are written over with a poison value (NaN, +Inf, -Inf; on the paths that
store bf16 also the NaN whose payload sits in the low half of the word only).  Three results are compared:

  out_p   the launch on the poisoned table
  out_0   the same launch - same kernel, same route - with the rows P set to 0.0
  ref_p   oracle/gripnet_oracle.py in float64 on the poisoned input (plain float64 torch where the oracle has no such function)

With dep = ~isfinite(ref_p) and clean = ~dep, `check` asserts
  1. torch.equal(out_p[clean], out_0[clean]): a clean element is what it is without the poison;
  2. ~isfinite(out_p) == dep, element by element;
  3. with a NaN poison every dependent element is NaN (an infinity may come out as either infinity or as NaN: the bf16 split
     of Inf is Inf - Inf, the basis-space route adds infinities of both signs);
  4. under a ReLU (or a sigmoid) only the NaN poisons are run: relu(-Inf) and sigmoid(+-Inf) are finite in the reference too.
There is no tolerance anywhere: set equality and torch.equal.

A case says which rows are poisoned and what depends on them by the graph alone (`dep_graph`: the rows with an edge from P -
plus P itself where a layer has a self loop or a root term - or the edges and scores that name P).  tests/test_poison_host.py
holds every case to its conditions from the reference alone: dep(float64) == dep_graph; at least four dependent rows (edges,
scores) except in the "nobody" variants, where no edge names the poisoned row and dep is empty or the row itself; clean at
least half of the output; and, where a case has destination rows (`lengths`), one clean row that is empty and one that is
shorter than the kernels' padding unit of four neighbours - otherwise no padded slot is read at all.

The cases are kept as small as the routes allow (the route tables of tests/test_gather_route.py, tests/test_rgcn_route.py and
tests/test_dense_route.py name the thresholds); every builder is cached, a case's tensors are never written to (`overwrite`
copies)."""
import functools
import types

import torch

import gat_cases as gcs
import kge_batch_cases as kb
import kge_cases as kc
import rgcn_conv_cases as rcc
from oracle import gripnet_oracle as orc

NAN, INF = float("nan"), float("inf")
LOW_NAN = "low-half nan"                     # bits 0x7F800001: a NaN that a truncation to bf16 would turn into +Inf
POISONS = {"nan": NAN, "+inf": INF, "-inf": -INF, "low nan": LOW_NAN}
NAN_POISONS = ("nan", "low nan")
PAD_UNIT = 4                                 # neighbours a gather asks for together at the least (a quad of lanes, a group of four rows)


# ---- the contract -----------------------------------------------------------------------------------------------------------
def overwrite(case, value):
    """The case's tensors with rows (axis 1: columns) `case.rows` of tensor `case.target` set to `value` (a float, a key of
    POISONS, or LOW_NAN).  A copy: the case's own tensors stay as they are."""
    value = POISONS.get(value, value) if isinstance(value, str) else value
    tensors = dict(case.tensors)
    t = tensors[case.target].clone()
    for r in case.rows:
        part = t[r] if case.axis == 0 else t[..., r]
        if getattr(case, "cols", None):                       # (only these columns of the row)
            part = part[case.cols[0]:case.cols[1]]
        if value == LOW_NAN:
            part.view(torch.int32).fill_(0x7F800001) if part.is_contiguous() else part.copy_(
                torch.full(part.shape, 0x7F800001, dtype=torch.int32).view(torch.float32))
        else:
            part.fill_(value)
    tensors[case.target] = t
    return tensors


def check(out_p, out_0, ref_p, what, nan=True):
    """Assertions 1 to 3 of the contract on one poisoned launch; prints the sizes of dep and clean.  Returns (dep, clean)."""
    out_p, out_0, ref_p = out_p.detach().cpu().float(), out_0.detach().cpu().float(), ref_p.detach().cpu()
    assert out_p.shape == out_0.shape == ref_p.shape, (what, out_p.shape, out_0.shape, ref_p.shape)
    dep = ~torch.isfinite(ref_p)
    clean = ~dep
    print("{}: dep {} clean {} of {} elements".format(what, int(dep.sum()), int(clean.sum()), dep.numel()))
    wrong = []
    moved = clean & ~((out_p == out_0) | (torch.isnan(out_p) & torch.isnan(out_0)))
    if not torch.equal(out_p[clean], out_0[clean]):
        at = torch.nonzero(moved | (clean & torch.isnan(out_p)))[:6].tolist()
        wrong.append("{} clean elements differ from the zeroed launch (first at {})".format(int((moved | (clean & torch.isnan(out_p))).sum()), at))
    nonfinite = ~torch.isfinite(out_p)
    if not torch.equal(nonfinite, dep):
        leaked, lost = nonfinite & clean, dep & ~nonfinite
        wrong.append("{} clean elements are not finite (first at {}), {} dependent elements are finite (first at {}: {})".format(
            int(leaked.sum()), torch.nonzero(leaked)[:6].tolist(), int(lost.sum()), torch.nonzero(lost)[:6].tolist(),
            out_p[lost][:6].tolist()))
    if nan and not bool(torch.isnan(out_p[dep]).all()):
        inf = dep & torch.isinf(out_p)
        wrong.append("{} dependent elements of a NaN poison are infinite (first at {})".format(int(inf.sum()), torch.nonzero(inf)[:6].tolist()))
    assert not wrong, "{}: {}".format(what, "; ".join(wrong))
    return dep, clean


def make_case(name, family, tensors, target, rows, ref, dep_graph, variants, axis=0, lengths=None, nobody=False, unit=None, **opts):
    """`ref(tensors, dtype, **flags)`: the reference in `dtype`; `variants`: [(poison name, flags of the launch), ...];
    `lengths`: neighbours of every destination row (None: the family has no rows of neighbours); `unit`: what the "at least
    four dependent ..." condition counts - "row" (a 2-D output of a graph layer), "edge" (a 1-D list of scores) or "element"
    (the row-local families: one poisoned row of A is one output row); `opts`: what the GPU runner needs to know."""
    unit = unit or ("edge" if dep_graph.dim() == 1 else "row")
    return types.SimpleNamespace(name=name, family=family, tensors=tensors, target=target, rows=tuple(int(r) for r in rows), axis=axis,
                                 ref=ref, dep_graph=dep_graph, variants=list(variants), lengths=lengths, nobody=nobody, unit=unit,
                                 **opts)


def cast(tensors, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in tensors.items()}


def variants_of(relu=True, bf16=False, gate="relu"):
    """The three poisons on the bare launch, the NaN poison(s) again under the ReLU (or the sigmoid)."""
    names = ["nan", "+inf", "-inf"] + (["low nan"] if bf16 else [])
    out = [(p, {}) for p in names]
    if relu:
        out += [(p, {gate: True}) for p in names if p in NAN_POISONS]
    return out


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def make_graph(n_src, lengths, named, seed, square=False, lo=0, hi=None):
    """[2, E] edges: destination t gets lengths[t] sources drawn (with repeats) from [lo, hi) without the rows `named` holds;
    row s of `named` is then written over the k-th slot of every destination in named[s] (k: its place among the keys).
    `square`: sources and destinations are one node set - no drawn edge is a loop.  The edges are shuffled."""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.as_tensor(lengths, dtype=torch.long)
    special = sorted(named)
    pool = torch.tensor([i for i in range(lo, n_src if hi is None else hi) if i not in named], dtype=torch.long)
    dst = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    at = torch.randint(0, pool.numel(), (dst.numel(),), generator=g)
    src = pool[at]
    if square:
        src = torch.where(src == dst, pool[(at + 1) % pool.numel()], src)
    first = torch.cumsum(lengths, 0) - lengths
    for k, s in enumerate(special):
        for t in named[s]:
            assert lengths[t] > k and not (square and s == t), (s, t)
            src[first[t] + k] = s
    order = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[order], dst[order]]).contiguous()


def rows_reading(ei, rows, n_dst, own=False):
    """[n_dst] bool: the destinations with an edge from one of `rows` (`own`: and the rows themselves - a self loop, a root term)."""
    hit = torch.zeros(n_dst, dtype=torch.bool)
    hit[ei[1][torch.isin(ei[0], torch.tensor(rows))]] = True
    if own:
        hit[list(rows)] = True
    return hit


def spread(pattern, n, named_rows, per_row=5):
    """For each of `named_rows` (in order) `per_row` destinations out of n, chosen so that the k-th named row only lands on
    destinations longer than k, none twice for one row, and the destinations of different rows overlap in one."""
    lengths = [pattern[i % len(pattern)] for i in range(n)]
    named, taken = {}, []
    for k, s in enumerate(sorted(named_rows)):                # (make_graph's order of the slots)
        fit =[t for t in range(n) if lengths[t] > k and t != s]
        # one short row, then every (len(fit) // per_row)-th: short and long rows, padded and unpadded ones
        step = max(1, len(fit) // per_row)
        pick = [fit[(k + i * (step + 1)) % len(fit)] for i in range(per_row)]        # (+ 1: another place in the pattern each time)
        shared = next((t for t in taken if lengths[t] > k and t != s), None)
        if shared is not None:
            pick[-1] = shared
        named[s] = sorted(set(pick))
        taken += named[s]
    return lengths, named


# ---- GCN-style gathers -------------------------------------------------------------------------------------------------------
EXT_DEGREES = [0, 1, 4, 31, 32, 33, 47, 48, 63, 64]          # tests/test_gpu_external_rows.py: around the 32 and 64 marks of the padded rows
GATHER_GRAPHS = {
    # name:   (plan,        sources, destinations, row lengths,                         sources drawn below)
    "ext":    ("bipartite", 300, 40, EXT_DEGREES, None),                               # padded (ELL) rows; 34 neighbours a row
    "ext_t":  ("bipartite", 300, 40, EXT_DEGREES, 280),                                # ... sources 280.. without an edge (transposed gather)
    "short":  ("bipartite", 300, 64, [0, 1, 2, 3, 5, 7, 9, 4], None),                  # fewer than 8 a row
    "long":   ("bipartite", 300, 24, [0, 1, 3, 64, 65, 100, 130, 129], None),          # 48 a row and more; row pointers
    "square": ("gcn", 300, 300, [0, 1, 2, 3, 5, 8, 13, 31, 33, 64], None),
    "big":    ("bipartite", 300, 4096, [0, 1, 2, 3, 4, 5, 6], None),                   # rows >= 4096: matrix cores, bf16 lane groups
    "tall":   ("bipartite", 2050, 4096, [0, 1, 2, 3, 4, 5, 6], None),                  # a table the tall-skinny product stores as bf16
    "sum":    ("sum", 300, 65536, [0, 1, 2, 3, 4], None),                              # rows >= 65536: the LDS-table gather
}


@functools.lru_cache(maxsize=None)
def gather_graph(name, which):
    """(edges [2, E], poisoned rows, lengths) of graph `name`; `which`: "row0" (row 0 named), "last+mid" (the last table row
    and a middle one named) or "nobody" (edges over [1, n) only, row 0 poisoned)."""
    kind, n_src, n_dst, pattern, hi = GATHER_GRAPHS[name]
    square = kind == "gcn"
    rows = {"row0": (0,), "last+mid": (n_src - 1, n_src // 2), "nobody": (0,)}[which]
    if which == "nobody":
        lengths, named = [pattern[i % len(pattern)] for i in range(n_dst)], {0: []}
    else:
        lengths, named = spread(pattern, n_dst, rows)
    ei = make_graph(n_src, lengths, named, seed=len(name) * 131 + len(which), square=square, hi=hi)
    return ei, rows, torch.tensor(lengths)


def gather_reference(spec):
    kind = GATHER_GRAPHS[spec["graph"]][0]
    n_dst = GATHER_GRAPHS[spec["graph"]][2]

    def ref(t, dtype, relu=False):
        t = cast(t, dtype)
        x, w, b, ew = t["x"], t.get("w"), t.get("b"), t.get("ew")
        if spec.get("entry") == "tail":                      # the gathered row's last 16 columns enter as relu(row[-16:] W2 + b2)
            x = torch.cat([x[:, :-16], torch.relu(x[:, -16:] @ t["w2"] + t["b2"])], dim=1)
        if spec.get("entry") == "bf16_product":              # (the table is x W rounded to bf16: non-finite where x W is)
            x, w = x @ w, None
        if kind == "gcn":
            y = orc.gcn_forward(x, w, b, t["ei"], ew) if w is not None else orc.gcn_propagate(x, *orc.gcn_norm(t["ei"], x.shape[0], ew, False, dtype), b)
        elif kind == "bipartite":
            sd = {"conv.weight": w if w is not None else torch.eye(x.shape[1], dtype=dtype)}
            if b is not None:
                sd["conv.bias"] = b
            y = orc.inter_forward_closed(sd, "", x, t["ei"], n_dst, ew)
        else:
            y = torch.zeros(n_dst, x.shape[1], dtype=dtype).index_add_(0, t["ei"][1], x[t["ei"][0]])
        return torch.relu(y) if relu else y
    return ref


GATHER_SPECS = {
    # route name:      graph, gathered width, output width (None: no weight), edge weights, entry point, switches
    "wave":            dict(graph="long", fin=16, fout=None, weighted=True),
    "wave_fast_off":   dict(graph="ext", fin=16, fout=None, weighted=False, env={"GN_DISABLE_FAST": "1"}, route="wave"),
    "wave_scalar":     dict(graph="ext", fin=15, fout=None, weighted=True),
    "group":           dict(graph="ext", fin=16, fout=None, weighted=False),
    "short_rows":      dict(graph="short", fin=16, fout=None, weighted=True),
    "lds_table":       dict(graph="sum", fin=16, fout=None, weighted=False, bias=False, relu=False),
    "lds_table_off":   dict(graph="sum", fin=16, fout=None, weighted=False, bias=False, relu=False, env={"GN_DISABLE_LDS_TABLE": "1"},
                            route="short_rows"),
    "transform_16_16": dict(graph="ext", fin=16, fout=16, weighted=True, env={"GN_DISABLE_QUAD": "1"}, route="transform"),
    "transform_quad":  dict(graph="ext", fin=16, fout=16, weighted=False),
    "transform_32_16": dict(graph="ext", fin=32, fout=16, weighted=False, route="transform"),
    "transform_64_16": dict(graph="ext", fin=64, fout=16, weighted=True, route="transform"),          # sixteen lanes a neighbour: the padded form
    "transform_32_32": dict(graph="ext", fin=32, fout=32, weighted=True, route="transform"),
    "transform_64_32": dict(graph="ext", fin=64, fout=32, weighted=False, route="transform"),
    "transform_long":  dict(graph="long", fin=64, fout=16, weighted=False, route="transform"),        # ... over row pointers
    "transform_tail":  dict(graph="ext", fin=64, fout=16, weighted=True, entry="tail"),
    # ... the poison in the row's last 16 columns alone: it reaches the sum through relu(row[-16:] W2 + b2) only, the inner ReLU
    "transform_tail_cols": dict(graph="ext", fin=64, fout=16, weighted=False, entry="tail", cols=(48, 64), route="transform_tail"),
    "transform_split": dict(graph="ext", fin=64, fout=16, weighted=False, entry="split"),
    "mfma":            dict(graph="big", fin=64, fout=64, weighted=True),
    "square":          dict(graph="square", fin=32, fout=16, weighted=True, route="transform"),
    "square_plain":    dict(graph="square", fin=16, fout=None, weighted=False, route="group"),
    "blocked_16":      dict(graph="square", fin=32, fout=16, weighted=False, env={"GN_BLOCKED_ANY": "1"}, route="blocked"),
    "blocked_32":      dict(graph="square", fin=64, fout=32, weighted=False, env={"GN_BLOCKED_ANY": "1"}, route="blocked"),
    "blocked_off":     dict(graph="square", fin=32, fout=16, weighted=False, env={"GN_BLOCKED_ANY": "1", "GN_DISABLE_BLOCKED": "1"},
                            route="transform"),
    "bf16_wave":       dict(graph="ext", fin=16, fout=None, weighted=True, entry="bf16"),
    "bf16_group":      dict(graph="big", fin=16, fout=None, weighted=False, entry="bf16"),
    "bf16_product":    dict(graph="tall", fin=32, fout=16, weighted=False, entry="bf16_product", route="split + bf16_group"),
    "transposed":      dict(graph="ext_t", fin=16, fout=None, weighted=True, entry="t", bias=False, relu=False),
}
ROW_SETS = ("row0", "last+mid", "nobody")


@functools.lru_cache(maxsize=None)
def gather_case(route, which):
    spec = dict(GATHER_SPECS[route])
    kind, n_src, n_dst, _, _ = GATHER_GRAPHS[spec["graph"]]
    ei, rows, lengths = gather_graph(spec["graph"], which)
    g = torch.Generator().manual_seed(1000 + len(route))
    fin, fout = spec["fin"], spec["fout"]
    t = {"ei": ei, "x": torch.randn(n_src, fin, generator=g)}
    if fout is not None:
        t["w"] = torch.randn(fin, fout, generator=g) * 0.3
    if spec.get("bias", True):
        t["b"] = torch.randn(fout or fin, generator=g)
    if spec["weighted"]:
        t["ew"] = torch.rand(ei.shape[1], generator=g) + 0.5
    if spec.get("entry") == "tail":
        t["w2"], t["b2"] = torch.randn(16, 16, generator=g) * 0.3, torch.randn(16, generator=g)
    bf16 = spec.get("entry") in ("bf16", "bf16_product")
    variants = variants_of(relu=spec.get("relu", True), bf16=bf16)
    if spec.get("entry") == "t":
        return transposed_case(route, which, spec, t, variants)
    dep_rows = rows_reading(ei, rows, n_dst, own=kind == "gcn")
    width = fout or fin
    return make_case("{} {}".format(route, which), "gather", t, "x", rows, gather_reference(spec), dep_rows[:, None].expand(n_dst, width).clone(),
                     variants, lengths=lengths, nobody=which == "nobody", spec=spec, kind=kind, n_src=n_src, n_dst=n_dst,
                     route=spec.get("route", route), cols=spec.get("cols"))


def transposed_case(route, which, spec, t, variants):
    """gn_graph_aggregate_t_f32: out[s] = sum over the edges leaving s of coef * g[dst].  The table is g [targets, f]: the rows
    poisoned are TARGETS (the empty target 0 is the one nobody reads; targets 1 and 2 have one and four sources), the output
    rows are sources - those from 280 on have no edge at all."""
    kind, n_src, n_dst, _, _ = GATHER_GRAPHS[spec["graph"]]
    ei, lengths = t["ei"], torch.bincount(t["ei"][0], minlength=n_src)
    g = torch.Generator().manual_seed(77)
    t["x"] = torch.randn(n_dst, spec["fin"], generator=g)
    rows = {"row0": (1, 2), "last+mid": (n_dst - 1, 12), "nobody": (0,)}[which]

    def ref(tt, dtype, relu=False):
        tt = cast(tt, dtype)
        deg = torch.ones(n_dst, dtype=dtype).index_add_(0, ei[1], tt["ew"])
        coef = tt["ew"] * deg.pow(-0.5)[ei[1]]
        return torch.zeros(n_src, spec["fin"], dtype=dtype).index_add_(0, ei[0], coef[:, None] * tt["x"][ei[1]])
    dep_rows = torch.zeros(n_src, dtype=torch.bool)
    dep_rows[ei[0][torch.isin(ei[1], torch.tensor(rows))]] = True
    return make_case("{} {}".format(route, which), "gather", t, "x", rows, ref, dep_rows[:, None].expand(n_src, spec["fin"]).clone(), variants,
                     lengths=lengths, nobody=which == "nobody", spec=spec, kind=kind, n_src=n_src, n_dst=n_dst, route="transposed")


def gather_cases():
    return [gather_case(route, which) for route in GATHER_SPECS for which in ROW_SETS]


# ---- the relational layer ---------------------------------------------------------------------------------------------------
REL_SHAPE = dict(fin=32, fout=32, bases=8, R=6)           # tests/test_gpu_boundaries.py: the destination-major kernel takes it up to 768 nodes
REL_NODES = (256, 257, 768, 769)                          # tests/test_gpu_fuzz.py RGCN_EDGE_CASES
REL_LENGTHS = [0, 1, 2, 3, 5, 8, 13, 31, 33, 40]
EMPTY_REL, ONE_EDGE_REL = 1, 4


@functools.lru_cache(maxsize=None)
def relational_case(n, which):
    fin, fout, bases, R = (REL_SHAPE[k] for k in ("fin", "fout", "bases", "R"))
    rows = {"row0": (0,), "last+mid": (n - 1, n // 2), "nobody": (0,)}[which]
    if which == "nobody":
        lengths, named = [REL_LENGTHS[i % len(REL_LENGTHS)] for i in range(n)], {0: []}
    else:
        lengths, named = spread(REL_LENGTHS, n, rows)
    ei = make_graph(n, lengths, named, seed=n + len(which), square=True)
    g = torch.Generator().manual_seed(n * 3 + len(which))
    live = torch.tensor([r for r in range(R) if r not in (EMPTY_REL, ONE_EDGE_REL)])
    et = live[torch.randint(0, live.numel(), (ei.shape[1],), generator=g)]
    et[ei.shape[1] // 3] = ONE_EDGE_REL                                        # relation 1 stays empty, relation 4 has one edge
    order = torch.sort(et, stable=True).indices
    ei, et = ei[:, order].contiguous(), et[order].contiguous()
    ids = torch.arange(R)
    rl = torch.stack([torch.searchsorted(et, ids), torch.searchsorted(et, ids, right=True)], dim=1).contiguous()
    assert int(rl[EMPTY_REL, 1] - rl[EMPTY_REL, 0]) == 0 and int(rl[ONE_EDGE_REL, 1] - rl[ONE_EDGE_REL, 0]) == 1
    t = {"ei": ei, "rl": rl, "x": torch.randn(n, fin, generator=g), "basis": torch.randn(bases, fin, fout, generator=g) / fin ** 0.5,
         "att": torch.randn(R, bases, generator=g) / bases ** 0.5, "root": torch.randn(fin, fout, generator=g) / fin ** 0.5,
         "bias": torch.randn(fout, generator=g)}

    def ref(tt, dtype, relu=False):
        tt = cast(tt, dtype)
        y = orc.rgcn_forward(tt["x"], tt["ei"], tt["rl"], tt["basis"], tt["att"], tt["root"], tt["bias"])
        return torch.relu(y) if relu else y
    dep = rows_reading(ei, rows, n, own=True)                                  # (own: the root term x[i] root)
    return make_case("relational n={} {}".format(n, which), "relational", t, "x", rows, ref, dep[:, None].expand(n, fout).clone(),
                     variants_of(), lengths=torch.tensor(lengths), nobody=which == "nobody", n=n, **REL_SHAPE)


@functools.lru_cache(maxsize=None)
def relational_conv_case(which, weighted):
    """RGCNConv (gripnet_amd/pyg_convs.py) on the graph of 257 nodes with its edges shuffled out of relation order: the sums
    (no mean) with an `edge_norm` factor on every message, or without one."""
    base = relational_case(257, which)
    ei, rl = base.tensors["ei"], base.tensors["rl"]
    g = torch.Generator().manual_seed(41)
    et = torch.repeat_interleave(torch.arange(rl.shape[0]), rl[:, 1] - rl[:, 0])
    order = torch.randperm(ei.shape[1], generator=g)
    t = dict(base.tensors, ei=ei[:, order].contiguous(), et=et[order].contiguous())
    del t["rl"]
    if weighted:
        t["norm"] = torch.rand(ei.shape[1], generator=g) + 0.5

    def ref(tt, dtype, relu=False):
        tt = cast(tt, dtype)
        return rcc.forward(tt["x"], tt["basis"], tt["att"], tt["root"], tt["bias"], tt["ei"], tt["et"], tt.get("norm"), relu)
    return make_case("RGCNConv {} {}".format("edge_norm" if weighted else "sum", which), "relational", t, "x", base.rows, ref, base.dep_graph,
                     variants_of(), lengths=base.lengths, nobody=base.nobody, n=257, conv=True, **REL_SHAPE)


def relational_cases():
    return ([relational_case(n, which) for n in REL_NODES for which in ROW_SETS] +
            [relational_conv_case(which, weighted) for weighted in (True, False) for which in ROW_SETS])


# ---- the DistMult decoder ---------------------------------------------------------------------------------------------------
DECODER_SHAPES = {
    # name:          (nodes, relations, features, edges)
    "lds fit":       (2400, 8, 16, 3000),            # tests/test_gpu_boundaries.py LDS_NODES_16: the node table's last size in LDS
    "lds miss":      (2401, 8, 16, 3000),
    "row classes":   (400, 12, 80, 3000),            # tests/test_gpu_boundaries.py class_rows_fit(80) = 480: one block of whole rows
    "three blocks":  (600, 12, 80, 3000),            # ... three blocks
    "column phases": (900, 12, 80, 3000),            # ... beyond 3 * 480 / 2 rows: the column-phase kernel
    "odd width":     (300, 7, 20, 1000),            # 20 features: no plan kernel's multiple of 16
}
DECODER_EMPTY_REL = 1


@functools.lru_cache(maxsize=None)
def decoder_lists(shape):
    """(pairs [2, E], sorted relation ids [E]) over nodes [1, n - 1) without n // 2; relation DECODER_EMPTY_REL holds none.
    Nodes 0, n // 2 and n - 1 are named by five pairs each, as u and as v, in the first and in the last relation too."""
    n, R, f, E = DECODER_SHAPES[shape]
    g = torch.Generator().manual_seed(n + R)
    pool = torch.tensor([i for i in range(1, n - 1) if i != n // 2])
    ei = pool[torch.randint(0, pool.numel(), (2, E), generator=g)]
    live = torch.tensor([r for r in range(R) if r != DECODER_EMPTY_REL])
    et = live[torch.randint(0, live.numel(), (E,), generator=g)]
    et[:6] = torch.tensor([0, R - 1, 0, R - 1, R // 2, R // 2])
    for k, node in enumerate((0, n // 2, n - 1)):
        for i in range(5):
            ei[i % 2, 10 * k + 2 * i + 20] = node            # (slots 20..49: alternately as u and as v)
    ei[:, 0], ei[:, 1] = torch.tensor([0, n - 1]), torch.tensor([n - 1, 0])          # both poisoned rows in one pair, first and last relation
    order = torch.sort(et, stable=True).indices
    return ei[:, order].contiguous(), et[order].contiguous()


@functools.lru_cache(maxsize=None)
def decoder_case(shape, target, which):
    """`target` "z": a node's row is poisoned, dep = the pairs that name it; "d": a relation's row, dep = its pairs.  "nobody":
    node n // 2 + 1 taken out of the list / the empty relation."""
    n, R, f, E = DECODER_SHAPES[shape]
    ei, et = decoder_lists(shape)
    g = torch.Generator().manual_seed(n * 7 + R)
    t = {"ei": ei, "et": et, "z": 0.3 * torch.randn(n, f, generator=g), "d": 0.25 * torch.randn(R, f, generator=g)}
    if target == "z":
        rows = {"row0": (0,), "last+mid": (n - 1, n // 2), "nobody": (n // 2 + 1,)}[which]
        if which == "nobody":
            moved = ei.clone()
            moved[moved == n // 2 + 1] = n // 2 + 2
            t["ei"] = ei = moved
        dep = torch.isin(ei[0], torch.tensor(rows)) | torch.isin(ei[1], torch.tensor(rows))
    else:
        rows = {"row0": (0,), "last+mid": (R - 1, R // 2), "nobody": (DECODER_EMPTY_REL,)}[which]
        dep = torch.isin(et, torch.tensor(rows))

    def ref(tt, dtype, sigmoid=False):
        tt = cast(tt, dtype)
        return orc.distmult(tt["z"], tt["ei"], tt["et"], tt["d"], sigmoid)
    return make_case("decoder {} {} {}".format(shape, target, which), "decoder", t, target, rows, ref, dep, variants_of(gate="sigmoid"),
                     nobody=which == "nobody", shape=shape, n=n, R=R, f=f, half=target == "z")


def decoder_cases():
    return [decoder_case(shape, target, which) for shape in DECODER_SHAPES for target in ("z", "d") for which in ROW_SETS]


# ---- dense products ---------------------------------------------------------------------------------------------------------
GEMM_SHAPES = {
    # name:             (m,    k,   n,  options)          the kernel the shape reaches (dense_route.hpp; tests/test_dense_route.py, tests/test_gpu_scales.py GEMM_CASES)
    "general":          (100, 40, 72, dict()),
    "general-ragged":   (40, 5, 20, dict()),
    "deep":             (40, 256, 20, dict()),
    "deep-transposed":  (17, 300, 21, dict(at=True, bt=True)),
    "lds":              (300, 64, 72, dict()),
    "split-ct4":        (2050, 64, 20, dict()),
    "split-ct8":        (2049, 128, 72, dict()),
    "split-slabs":      (2050, 288, 72, dict()),             # nine chunks of K through a six-chunk slab
    "split-b-transposed": (2050, 64, 20, dict(bt=True)),
    "row-gather":       (500, 40, 24, dict(a_rows=True)),
    "batch-3":          (40, 5, 20, dict(batch=3)),
}


@functools.lru_cache(maxsize=None)
def gemm_case(shape, which):
    """`which`: "a row0" / "a last+mid" (rows of A: only those output rows may change; the middle row sits inside a 16-row tile),
    "b column" (B's last column at a ragged n: only that output column), "nobody" (row-gather only: a table row the list does
    not name)."""
    m, k, n, opt = GEMM_SHAPES[shape]
    batch = opt.get("batch", 1)
    table = 300 if opt.get("a_rows") else m
    g = torch.Generator().manual_seed(m * 7 + k * 3 + n)
    lead = (batch,) if batch > 1 else ()
    t = {"a": torch.randn(*lead, table, k, generator=g), "b": torch.randn(*lead, k, n, generator=g) * 0.1, "bias": torch.randn(n, generator=g)}
    idx = None
    if opt.get("a_rows"):
        pool = torch.tensor([i for i in range(1, table - 1) if i not in (table // 2, 7)])
        idx = pool[torch.randint(0, pool.numel(), (m,), generator=g)]
        idx[torch.tensor([3, 100, 250, 499, 16])] = 0                       # (row 0 of the table: five times; 7: never)
        idx[torch.tensor([0, 33, 200, 498])] = table - 1
        idx[torch.tensor([5, 77, 300, 497])] = table // 2
        t["idx"] = idx
    dep = torch.zeros(*lead, m, n, dtype=torch.bool)
    if which == "b column":
        target, rows, axis = "b", (n - 1,), 1
        dep[..., n - 1] = True
    else:
        target, axis = "a", 0
        if idx is not None:
            rows = {"a row0": (0,), "a last+mid": (table - 1, table // 2), "nobody": (7,)}[which]
            dep[torch.isin(idx, torch.tensor(rows))] = True
        else:
            rows = {"a row0": (0,), "a last+mid": (m - 1, (m // 2) // 16 * 16 + 5)}[which]
            for r in rows:
                dep[..., r, :] = True
        if batch > 1:                                                        # (rows of the second product only)
            dep[0], dep[2] = False, False

    def ref(tt, dtype, relu=False):
        tt = cast(tt, dtype)
        a = tt["a"] if idx is None else tt["a"][idx]
        y = a @ tt["b"] + tt["bias"]
        return torch.relu(y) if relu else y
    case = make_case("gemm {} {}".format(shape, which), "gemm", t, target, rows, ref, dep, variants_of(), axis=axis, nobody=which == "nobody",
                     unit="element", shape=shape, m=m, k=k, n=n, opt=opt, batch=batch)
    return case


def gemm_overwrite(case, value):
    """`overwrite` for a batched A: the rows are rows of the SECOND product's A."""
    if case.batch > 1 and case.target == "a":
        inner = types.SimpleNamespace(tensors={"a": case.tensors["a"][1]}, target="a", rows=case.rows, axis=0)
        a = case.tensors["a"].clone()
        a[1] = overwrite(inner, value)["a"]
        return dict(case.tensors, a=a)
    return overwrite(case, value)


def gemm_cases():
    out = []
    for shape, (_, _, _, opt) in GEMM_SHAPES.items():
        sets = ["a row0", "a last+mid", "b column"] + (["nobody"] if opt.get("a_rows") else [])
        out += [gemm_case(shape, which) for which in sets]
    return out


# ---- merges and class scores ------------------------------------------------------------------------------------------------
def merge_reference(mode):
    def ref(t, dtype):
        t = cast(t, dtype)
        d, s = t["dst"], t["src"]
        return {1: s.abs(), 2: (d + s.abs()) / 2, 3: (d + torch.relu(s)) / 2, 4: (d + s + t["src2"]) / 3}[mode]
    return ref


@functools.lru_cache(maxsize=None)
def merge_case(mode, which):
    """gn_merge_f32 modes 1 to 4 on [37, 19]: row-local.  Mode 3 holds a ReLU: its NaN stays NaN; its -Inf is a finite half of dst
    in the reference too, so the infinities are left to the other modes."""
    rows_n, cols = 37, 19
    g = torch.Generator().manual_seed(mode)
    t = {"dst": torch.randn(rows_n, cols, generator=g), "src": torch.randn(rows_n, cols, generator=g), "src2": torch.randn(rows_n, cols, generator=g)}
    rows = {"row0": (0,), "last+mid": (rows_n - 1, rows_n // 2)}[which]
    dep = torch.zeros(rows_n, cols, dtype=torch.bool)
    dep[list(rows)] = True
    variants = [("nan", {})] if mode == 3 else [(p, {}) for p in ("nan", "+inf", "-inf")]
    return make_case("merge mode {} {}".format(mode, which), "merge", t, "src", rows, merge_reference(mode), dep, variants, unit="element", mode=mode)


@functools.lru_cache(maxsize=None)
def class_scores_case(which, softmax):
    """gn_class_scores_f32: softmax?(z[nodes] W): the rows of the node list that name a poisoned row of z.  Under the softmax a
    row with an infinity is NaN or holds a NaN (exp(inf - inf)): NaN poison only, like the other gated outputs."""
    n, f, C, m = 200, 24, 7, 150
    g = torch.Generator().manual_seed(5)
    pool = torch.tensor([i for i in range(1, n - 1) if i not in (n // 2, 9)])
    nodes = pool[torch.randint(0, pool.numel(), (m,), generator=g)]
    nodes[torch.tensor([0, 40, 41, 90, 149])] = 0
    nodes[torch.tensor([1, 50, 91, 148])] = n - 1
    nodes[torch.tensor([2, 60, 92, 147])] = n // 2
    t = {"z": torch.randn(n, f, generator=g), "w": torch.randn(f, C, generator=g) * 0.3, "nodes": nodes}
    rows = {"row0": (0,), "last+mid": (n - 1, n // 2), "nobody": (9,)}[which]
    dep = torch.isin(nodes, torch.tensor(rows))[:, None].expand(m, C).clone()

    def ref(tt, dtype):
        tt = cast(tt, dtype)
        return orc.multiclass(tt["z"], tt["nodes"], tt["w"], softmax)
    variants = [("nan", {})] if softmax else [(p, {}) for p in ("nan", "+inf", "-inf")]
    return make_case("class scores {} softmax={}".format(which, softmax), "class_scores", t, "z", rows, ref, dep, variants,
                     nobody=which == "nobody", softmax=softmax)


def rowwise_cases():
    return ([merge_case(mode, which) for mode in (1, 2, 3, 4) for which in ("row0", "last+mid")] +
            [class_scores_case(which, softmax) for which in ROW_SETS for softmax in (False, True)])


# ---- graph attention --------------------------------------------------------------------------------------------------------
GAT_ROWS = {
    # graph: row sets.  "small" (12 nodes) has no node with three distinct out-neighbours, node 0 of the staircase feeds every
    # node and node n - 1 of the transposed staircase does: the sets that leave half of the output clean are the ones below.
    "small":       {"last+mid": (11, 7), "own": (10,)},
    "staircase":   {"last+mid": (130, 100), "own": (130,)},
    "staircase_t": {"mid": (30,), "own": (0,)},
}


@functools.lru_cache(maxsize=None)
def gat_case(graph, which):
    """GATConv, 2 heads of 8 channels: dep = the rows with an in-edge from P plus P itself (its own loop), every head and column.
    "own": a row no other row reads - dep is the row itself."""
    c = gcs.case(graph, heads=2, channels=8, fin=7, seed=3)
    rows = GAT_ROWS[graph][which]
    work = gcs.working_list(c.edge_index, c.n)
    dep = rows_reading(work, rows, c.n, own=True)
    t = {"x": c.x, "w": c.weight, "att": c.att, "b": c.bias, "ei": c.edge_index}

    def ref(tt, dtype, relu=False):
        tt = cast(tt, dtype)
        return gcs.forward(tt["x"], tt["w"], tt["att"], tt["b"], tt["ei"], c.heads, True, c.slope, relu)
    lengths = torch.bincount(work[1], minlength=c.n) - 1
    return make_case("gat {} {}".format(graph, which), "gat", t, "x", rows, ref, dep[:, None].expand(c.n, 16).clone(), variants_of(),
                     lengths=lengths, nobody=which == "own", heads=c.heads, channels=c.channels, slope=c.slope)


def gat_cases():
    return [gat_case(graph, which) for graph, sets in GAT_ROWS.items() for which in sets]


# ---- KGE scorers ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kge_case(model, which, batch):
    """gn_kge_forward_f32 over 257 triples (H = 36: a second trip of the lane group) and the candidate-block
    gn_kge_batch_forward_f32 (5 x 67 candidates): the raw scores that name a poisoned entity row."""
    n, R, H, gamma = 60, 4, 36, 12.0
    g = torch.Generator().manual_seed(len(model) + 10 * batch)
    ent, rel = kc.tables(model, n, R, H, gamma, g)
    pool = torch.tensor([i for i in range(1, n - 1) if i not in (n // 2, 9)])
    rows = {"row0": (0,), "last+mid": (n - 1, n // 2), "nobody": (9,)}[which]
    if batch:
        B, K = 5, 67
        positive = pool[torch.randint(0, pool.numel(), (2, B), generator=g)]
        et = torch.randint(0, R, (B,), generator=g).sort().values
        negatives = pool[torch.randint(0, pool.numel(), (B, K), generator=g)]
        for k, node in enumerate((0, n // 2, n - 1)):
            negatives[torch.arange(5), torch.arange(5) * 13 + k] = node
        sample, et_list = kb.expand(positive, et, negatives, "tail")
        t = {"ent": ent, "rel": rel, "positive": positive, "et": et, "negatives": negatives}
        shape = (B, K)
    else:
        E = 257
        sample = pool[torch.randint(0, pool.numel(), (2, E), generator=g)]
        et_list = torch.randint(0, R, (E,), generator=g).sort().values
        for k, node in enumerate((0, n // 2, n - 1)):
            for i in range(5):
                sample[i % 2, 50 * i + k] = node
        t = {"ent": ent, "rel": rel, "sample": sample, "et": et_list}
        shape = (E,)
    dep = (torch.isin(sample[0], torch.tensor(rows)) | torch.isin(sample[1], torch.tensor(rows))).view(shape)

    def ref(tt, dtype):
        tt = cast(tt, dtype)
        return kc.raw_score(model, tt["ent"], tt["rel"], sample, et_list, gamma).view(shape)
    return make_case("kge {} {} {}".format(model, "block" if batch else "list", which), "kge", t, "ent", rows, ref, dep,
                     [(p, {}) for p in ("nan", "+inf", "-inf")], nobody=which == "nobody", unit="edge", model=model, gamma=gamma, H=H, batch=batch)


def kge_cases():
    return [kge_case(model, which, batch) for model in kc.MODELS for batch in (False, True) for which in ROW_SETS]


FAMILIES = {"gather": gather_cases, "relational": relational_cases, "decoder": decoder_cases, "gemm": gemm_cases,
            "rowwise": rowwise_cases, "gat": gat_cases, "kge": kge_cases}


def poisoned(case, value):
    return gemm_overwrite(case, value) if case.family == "gemm" else overwrite(case, value)
