"""The row-class decoder kernel's table fill (k_distmult_class, distmult_plan.hip).

Where the LDS image of a class is a byte copy of rows of z (80, 48, 16 features, z contiguous, the whole column range)
the table and the relation rows of D arrive by LDS-DMA in 1 KB pieces; every other layout (64 features: padded LDS
stride; z a column slice of a wider tensor; the second launch of the two-launch column form) keeps the register-staged
fill.  Either way the scores are those of the plan-less kernel, bit for bit.

Every case is called ten times per sigmoid setting with z rewritten between the calls: a table that is read before it
has landed, or that keeps rows of the previous call, shows as a mismatch when the timing is unlucky.  (A clean run does
not prove the waits; they are placed by count - see DESIGN.md section 4.2.)
"""
import os

import pytest
import torch

from gripnet_amd import _hip
from gripnet_amd.utils import to_bidirection

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("GN_DISABLE_FAST") == "1", reason="fast paths disabled")]

CALLS = 10


def make_list(n, pairs_per_relation, seed, lo_u=None, lo_v=None):
    """A type-sorted list: every relation's random pairs, each in both directions (so mirrors exist).
    lo_u / lo_v = (lo, hi): draw that endpoint from [lo, hi) instead of [0, n)."""
    gen = torch.Generator().manual_seed(seed)
    eis, ets = [], []
    for r, s in enumerate(pairs_per_relation):
        u = torch.randint(*(lo_u or (0, n)), (s,), generator=gen)
        v = torch.randint(*(lo_v or (0, n)), (s,), generator=gen)
        eis.append(to_bidirection(torch.stack([u, v])))
        ets.append(torch.full((2 * s,), r, dtype=torch.int64))
    return torch.cat(eis, dim=1), torch.cat(ets)


def spread(total_pairs, relations):
    """`total_pairs` over `relations` uneven relation sizes (odd sizes, an empty relation, a single pair)."""
    sizes = [1, 0, 37] + [0] * (relations - 3)
    left = total_pairs - sum(sizes)
    for r in range(3, relations):
        sizes[r] = left // (relations - 3) + (r if r % 2 else -r)
    sizes[-1] += total_pairs - sum(sizes)
    return sizes


def plan_serves(n, f):
    """Whether the row-class kernel takes (n nodes, f features): the rows of one block, or of two of three, fit the LDS
    next to 64 relation rows of D (build_class_layout), and the sum's column parts (plan_phases: as many columns as fit
    150 KB with every node, 64 at the most) are one part, or two with an instantiation of the kernel."""
    j = f // 16
    stride = f if j % 2 else f + 16
    rows_fit = (160 * 1024 - 64 * f * 4) // (stride * 4)
    max_w = min(64, 150 * 1024 // (4 * n) // 16 * 16)
    if max_w < 16 or not (n <= rows_fit or 2 * -(-n // 3) <= rows_fit):
        return False
    return -(-f // max_w) <= 2 and (j, min(max_w, f) // 16) in ((5, 3), (5, 4), (4, 4), (3, 3), (2, 2), (1, 1))


def check_plan(gpu, n, f, ei, et, R, z_slice=False, seed=0):
    """Ten calls per sigmoid setting, z rewritten in place between them; the plan's scores (through the decoder's ladder,
    `_hip.distmult_forward`: a plan that refuses the shape leaves the call to the plan-less kernel) against the plan-less
    kernel's."""
    ei, et = ei.to(gpu), et.to(gpu)
    gen = torch.Generator(device=gpu).manual_seed(1000 + seed)
    if z_slice:                                                   # columns [8, 8 + f) of a wider tensor: 16-byte aligned, strided
        z = torch.zeros(n, f + 16, device=gpu)[:, 8:8 + f]
    else:
        z = torch.zeros(n, f, device=gpu)
    w = torch.randn(R, f, generator=gen, device=gpu)
    plan = _hip.DistMultPlan(ei, et, n, R, f)
    E = ei.shape[1]
    assert plan_serves(n, f) or (n, f) == (1344, 80)
    if plan_serves(n, f):                                         # the plan holds the row-class encoding (and only that)
        with pytest.raises(_hip.Unsupported):
            plan.forward_cols(z, f, 0, 4, w, True, torch.empty(E, device=gpu))
    for sigmoid in (True, False):
        for _ in range(CALLS):
            z.copy_(torch.randn(n, f, generator=gen, device=gpu))
            want = _hip.distmult(z, ei, et, w, sigmoid, torch.full((E,), float("nan"), device=gpu))
            got, served = _hip.distmult_forward(z, ei, et, w, sigmoid, torch.full((E,), float("nan"), device=gpu), plan)
            assert served or not plan_serves(n, f)
            assert torch.equal(got, want), (n, f, E, sigmoid, (got != want).sum().item())
    _hip.raise_if_index_errors(gpu)
    return plan, z, w


# 80 features: 448 = the largest single block (140 KB exactly); 449 = the smallest three-block case (150 / 150 / 149);
# 451 = blocks of 151 rows, 48,320 bytes, no multiple of a piece: a piece straddles the blocks; 645 = the workload's;
# 672 = the largest three-block case (two blocks of 224 rows are 140 KB); 1344 = three blocks of 448 rows: a class of two
# does not fit and the plan refuses the call.  ~3 k edges: one batch range; ~144 k: eight position parts.
@pytest.mark.parametrize("pairs", [1500, 72000])
@pytest.mark.parametrize("n", [448, 449, 451, 645, 672, 1344])
def test_class_boundaries_80_features(gpu, n, pairs):
    R = 9
    ei, et = make_list(n, spread(pairs, R), seed=n + pairs)
    check_plan(gpu, n, 80, ei, et, R, seed=n)


# 48 and 16 features: rows shorter than a piece (192 and 64 bytes); 64 features: padded stride, the register-staged fill.
# One block (645; 2400 = the most nodes the kernel takes at 16 features; 449) and three (795: blocks of 265 rows = 50,880
# bytes; 470; no 16-feature list has three: whatever fits the column parts fits one block)
@pytest.mark.parametrize("n,f", [(645, 48), (795, 48), (645, 16), (2400, 16), (449, 64), (470, 64)])
@pytest.mark.parametrize("pairs", [1500, 72000])
def test_other_feature_counts(gpu, n, f, pairs):
    R = 9
    ei, et = make_list(n, spread(pairs, R), seed=n + f + pairs)
    check_plan(gpu, n, f, ei, et, R, seed=f)


def test_more_than_one_walk(gpu):
    """Just past the 1 MB score window (2.2 M edges on eight position parts): the workgroups walk two batch ranges and
    refill their relation rows of D between them."""
    n, R = 449, 8
    ei, et = make_list(n, [137500] * R, seed=7)
    check_plan(gpu, n, 80, ei, et, R, seed=7)


# n = 449: blocks [0, 150), [150, 300), [300, 449)
@pytest.mark.parametrize("what", ["all_cross", "all_in_block0", "few_in_block0"])
def test_pairs_inside_and_across_blocks(gpu, what):
    n, R = 449, 5
    if what == "all_cross":                                       # no pair has both endpoints in one block
        a, ta = make_list(n, [700] * R, seed=1, lo_u=(0, 150), lo_v=(150, 300))
        b, tb = make_list(n, [700] * R, seed=2, lo_u=(150, 300), lo_v=(300, 449))
        c, tc = make_list(n, [700] * R, seed=3, lo_u=(300, 449), lo_v=(0, 150))
        ei, et = torch.cat([a, b, c], dim=1), torch.cat([ta, tb, tc])
        order = torch.sort(et, stable=True).indices
        ei, et = ei[:, order], et[order]
    elif what == "all_in_block0":
        ei, et = make_list(n, [2000] * R, seed=4, lo_u=(0, 150), lo_v=(0, 150))
    else:                                                         # a handful of pairs inside block 0 among crossing ones
        a, ta = make_list(n, [3] * R, seed=5, lo_u=(0, 150), lo_v=(0, 150))
        b, tb = make_list(n, [1500] * R, seed=6, lo_u=(0, 150), lo_v=(150, 449))
        ei, et = torch.cat([a, b], dim=1), torch.cat([ta, tb])
        order = torch.sort(et, stable=True).indices
        ei, et = ei[:, order], et[order]
    check_plan(gpu, n, 80, ei, et, R, seed=11)


@pytest.mark.parametrize("n", [449, 645])
def test_z_as_a_column_slice(gpu, n):
    """z strided (columns of a wider tensor): not a byte copy of rows, so the register-staged fill."""
    R = 9
    ei, et = make_list(n, spread(20000, R), seed=n)
    check_plan(gpu, n, 80, ei, et, R, z_slice=True, seed=n)


def test_two_launch_column_form(gpu):
    """gn_distmult_plan_forward_cols_f32 split where the single launch changes its column part (48 | 32 at 645 nodes):
    the first launch on a table of the first 48 columns only (LDS-DMA, 192-byte rows) or on the whole table (strided for
    that launch), the second launch from column 48 (never a byte copy): the single launch's bits."""
    n, f, R = 645, 80, 9
    ei, et = make_list(n, spread(20000, R), seed=21)
    plan, z, w = check_plan(gpu, n, f, ei, et, R, seed=21)
    E = ei.shape[1]
    gen = torch.Generator(device=gpu).manual_seed(22)
    for sigmoid in (True, False):
        for _ in range(CALLS):
            z.copy_(torch.randn(n, f, generator=gen, device=gpu))
            whole = plan.forward(z, w, sigmoid, torch.full((E,), float("nan"), device=gpu))
            for first in (z[:, :48].contiguous(), z):
                out = torch.full((E,), float("nan"), device=gpu)
                plan.forward_cols(first, f, 0, 48, w, sigmoid, out)
                plan.forward_cols(z, f, 48, 80, w, sigmoid, out)
                assert torch.equal(out, whole)
