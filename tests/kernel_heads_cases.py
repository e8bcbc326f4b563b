"""Cases and fixtures of tests/test_gpu_kernel_heads.py (not a test module): the relational layer on the destination-major
kernel and the gene gather on small graphs, each with outputs recorded ONCE on the GPU by the library of the commit in front
of the one that reordered the kernels' heads (requests in front of descriptor waits, clamped id prefetch).  None of those
changes may move a bit.

An output is up to 645 x 32 floats and there are 72 relational cases, so a fixture holds, per case, the SHA-256 of the
output's bytes (equal digests = equal bits) and the output's first eight rows as they are (what a mismatch report shows):

    tests/golden/kernel_heads_pair_digest.npy    [cases, 32] uint8     tests/golden/kernel_heads_pair_rows.npy    [cases, 8, 32] float32
    tests/golden/kernel_heads_gather_digest.npy  [cases, 32] uint8     tests/golden/kernel_heads_gather_rows.npy  [cases, 8, 16] float32

`python tests/kernel_heads_cases.py --record` (on a GPU, with the library to record from) rewrites them.
"""
import hashlib
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS_KEPT = 8

# ---- relational layer --------------------------------------------------------------------------------------------------
# n: 40 = fewer nodes than compute units, one row per workgroup; 300 = two rows; 645 = three (the workload's).
# relations: 5 = the att table is no whole 1 KB DMA piece (eight rows of 32 bases); 8 = exactly one; 13 = one and a tail.
# bases: 32 = rows are the LDS rows, LDS-DMA fill; 20 = the padded fill.  catout: the side copy of x into slot 0 of a concat
# buffer (and the ReLU homoGraph asks for with it).  48 inputs arrive with their bf16 split planes, as in the workload
# (k_rgcn_pair<3, 2, 3, true>); 32 inputs are split by the kernel itself.
PAIR_FOUT = 32
PAIR_CASES = [(n, rel, bases, catout, fin)
              for n in (40, 300, 645) for rel in (5, 8, 13) for bases in (32, 20) for catout in (False, True) for fin in (32, 48)]


def pair_id(case):
    return "n{}-R{}-B{}-{}-f{}".format(case[0], case[1], case[2], "cat" if case[3] else "plain", case[4])


def pair_operands(case):
    """Seeded operands on the CPU: about 20 edges per node in uneven relation blocks (an empty relation among them), the
    last seventh of the nodes without an incoming edge."""
    import gripnet_amd
    n, rel, bases, catout, fin = case
    gen = torch.Generator().manual_seed(n * 131 + rel * 17 + bases + fin + int(catout))
    total = 20 * n
    sizes = [max(0, total // rel + (7 * r if r % 2 else -5 * r)) for r in range(rel)]
    sizes[1] = 0
    sizes[-1] += total - sum(sizes)
    blocks = [torch.stack([torch.randint(0, n, (s,), generator=gen), torch.randint(0, max(1, n - n // 7), (s,), generator=gen)])
              for s in sizes]
    rei, rl = torch.cat(blocks, dim=1), gripnet_amd.utils.get_range_list(blocks)
    std = 1 / fin ** 0.5
    ops = {"x": torch.randn(n, fin, generator=gen),
           "basis": torch.randn(bases, fin, PAIR_FOUT, generator=gen) * std,
           "att": torch.randn(rel, bases, generator=gen) / bases ** 0.5,
           "root": torch.randn(fin, PAIR_FOUT, generator=gen) * std,
           "bias": torch.randn(PAIR_FOUT, generator=gen)}
    return ops, rei, rl


class PairRunner:
    """The layer of one case on the GPU; `run(kernel)` = (output, side slot or None) of a forward on that kernel."""

    def __init__(self, case, ops, rei, rl, dev):
        import gripnet_amd
        n, rel, bases, catout, fin = case
        self.case, self.dev = case, dev
        self.layer = gripnet_amd.myRGCN(fin, PAIR_FOUT, rel, bases, False, bias=True).to(dev)
        with torch.no_grad():
            for p, v in ((self.layer.basis, ops["basis"]), (self.layer.att, ops["att"]), (self.layer.root, ops["root"]),
                         (self.layer.bias, ops["bias"])):
                p.copy_(v.to(dev))
        self.x = ops["x"].to(dev)
        self.rei, self.rl = rei.to(dev), rl

    def path(self, kernel):
        m = self.layer
        return m._plan.path(m.in_channels, m.out_channels, m.num_bases, False, kernel)

    def run(self, kernel="pair"):
        from gripnet_amd import _hip
        n, rel, bases, catout, fin = self.case
        m = self.layer
        m.kernel = kernel
        x = self.x.clone()
        if fin == 48:
            _hip.SplitPlanes(n, fin // 16, self.dev).fill_from(x).tag(x)
            assert _hip.SplitPlanes.of(x, fin // 16) is not None
        with torch.no_grad():
            if catout:
                buf = torch.full((n, fin + PAIR_FOUT), float("nan"), device=self.dev)
                y = m(x, self.rei, None, self.rl, _out=buf[:, fin:], _relu=True, _side=(x, buf[:, :fin], 0))
                return y, buf[:, :fin]
            return m(x, self.rei, None, self.rl), None


# ---- gene gather -------------------------------------------------------------------------------------------------------
# A tile is 16 destination rows of similar degree and takes ceil(largest degree / 16) iterations of the id stream; a wave
# walks a contiguous run of its range's tiles.  64 nodes are one range of four tiles, dealt to four of the sixteen waves (the
# other twelve have no iteration at all); the in-degrees below put the tiles at the iteration counts named (a self loop
# comes on top: the degrees sit in the middle of their bucket of sixteen).  The prologue requests sixteen iterations in two
# buffers of eight, the loop refills a buffer only beyond that: 0, 1, 7, 8, 9, 15, 16, 17 and 25 iterations are every side
# of those edges.
def _deg(iters):
    return 16 * (iters - 1) + 8


GATHER_CASES = [
    # name,           nodes, in-degree of the rows of each tile (None: random graph), iteration counts some wave must have
    ("tiles-25-17-16-15", 64, [_deg(25), _deg(17), _deg(16), _deg(15)], {0, 15, 16, 17, 25}),
    ("tiles-9-8-7-1", 64, [_deg(9), _deg(8), _deg(7), _deg(1)], {0, 1, 7, 8, 9}),
    ("random-333", 333, None, set()),          # six ranges, ragged last tiles
    ("random-2000", 2000, None, set()),        # thirty-two ranges
]
GATHER_COLS = 16


def gather_operands(case):
    name, n, tile_deg, _ = case
    gen = torch.Generator().manual_seed(n + len(name))
    if tile_deg is None:
        e = 12 * n
        a = torch.randint(0, n, (2, e), generator=gen)
        a[1, : e // 8] = n // 3                                   # a hub row
        a = a[:, a[0] != a[1]]
        ei = torch.cat([a, a.flip(0)], dim=1)
    else:
        src, dst = [], []
        for i in range(n):
            d = tile_deg[i // 16] - (i % 16) // 3                 # a few edges fewer down the tile: same bucket
            s = torch.randint(0, n - 1, (d,), generator=gen)
            src.append(s + (s >= i).long())                       # any node but i itself
            dst.append(torch.full((d,), i, dtype=torch.int64))
        ei = torch.stack([torch.cat(src), torch.cat(dst)])
    return ei.long(), torch.randn(n, GATHER_COLS, generator=gen), torch.randn(GATHER_COLS, generator=gen)


def run_gather(case, ei, xw, bias, dev):
    """(plan, out) of act(A_norm xw + b) on the LDS-staged path as the environment has it (GN_BLOCKED_ANY=1 is the caller's)."""
    from gripnet_amd import _hip
    n = case[1]
    plan = _hip.GraphPlan.gcn(ei.to(dev), n)
    assert plan.build_blocked(GATHER_COLS) == GATHER_COLS, "the plan did not get its LDS-staged encoding"
    out = torch.full((n, GATHER_COLS), float("nan"), device=dev)
    plan.aggregate(xw.to(dev), bias.to(dev), True, out)
    return plan, out


# ---- fixtures ----------------------------------------------------------------------------------------------------------
def digest(t):
    return np.frombuffer(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).digest(), dtype=np.uint8)


def head_rows(t):
    rows = np.zeros((ROWS_KEPT, t.shape[1]), dtype=np.float32)
    k = min(ROWS_KEPT, t.shape[0])
    rows[:k] = t.detach().cpu().numpy()[:k]
    return rows


def load_golden(kind):
    return (np.load(os.path.join(GOLDEN, "kernel_heads_{}_digest.npy".format(kind))),
            np.load(os.path.join(GOLDEN, "kernel_heads_{}_rows.npy".format(kind))))


def assert_recorded(kind, index, what, t):
    """`t` is, bit for bit, what the fixture's library computed for case `index`."""
    digests, rows = load_golden(kind)
    got = head_rows(t)
    same_rows = got.view(np.uint32) == rows[index].view(np.uint32)
    assert same_rows.all(), "{}: {} of the first {} rows' values differ from the recorded ones, first at {}".format(
        what, int((~same_rows).sum()), ROWS_KEPT, tuple(np.argwhere(~same_rows)[0]))
    assert (digest(t) == digests[index]).all(), "{}: the first rows match the recording, the whole output does not".format(what)


def record(dev):
    os.environ["GN_BLOCKED_ANY"] = "1"
    os.environ.pop("GN_BLOCKED_DIRECT", None)
    d, r = [], []
    for case in PAIR_CASES:
        ops, rei, rl = pair_operands(case)
        run = PairRunner(case, ops, rei, rl, dev)
        y, _ = run.run("pair")
        assert run.path("pair") == "pair", pair_id(case)
        d.append(digest(y)); r.append(head_rows(y))
    np.save(os.path.join(GOLDEN, "kernel_heads_pair_digest.npy"), np.stack(d))
    np.save(os.path.join(GOLDEN, "kernel_heads_pair_rows.npy"), np.stack(r))
    d, r = [], []
    for case in GATHER_CASES:
        ei, xw, bias = gather_operands(case)
        plan, out = run_gather(case, ei, xw, bias, dev)
        assert plan.blocked_gather_kernel == "staged", case[0]
        d.append(digest(out)); r.append(head_rows(out))
    np.save(os.path.join(GOLDEN, "kernel_heads_gather_digest.npy"), np.stack(d))
    np.save(os.path.join(GOLDEN, "kernel_heads_gather_rows.npy"), np.stack(r))
    print("recorded {} relational and {} gather cases".format(len(PAIR_CASES), len(GATHER_CASES)))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["--record"]:
        record(torch.device("cuda:0"))
    else:
        sys.exit("usage: python tests/kernel_heads_cases.py --record")
