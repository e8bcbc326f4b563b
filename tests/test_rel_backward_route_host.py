"""The relational layer's backward route (gripnet_amd.autograd.relational_backward_route): which of its functions computes
dx, dW_r and dbasis for a set of plain answers - one case on each side of every rule, written out as a table (no GPU, no
library).  The widths are the forward layer's: fin -> fout on `bases` bases."""
import pytest

from gripnet_amd.autograd import RelBackwardRoute, relational_backward_route

BUDGET = 6 * 300 * 16          # R * n * fout of the `dw` rows below


def route(fin=48, fout=32, bases=4, relations=6, nodes=300, q_budget=1 << 26, need_x=True, need_basis=True, need_att=True, **answers):
    return relational_backward_route(fin, fout, bases, relations=relations, nodes=nodes, q_budget=q_budget, need_x=need_x,
                                     need_basis=need_basis, need_att=need_att, **answers)


# (kernel of the reversed plan, fin, fout, the forward's basis usable in place) -> dx
DX = [
    ("pair",     48, 32, True,  "transposed"),
    ("pair",     48, 32, False, "direct"),
    ("lds",      48, 32, True,  "blocks"),
    ("lds",      48, 32, False, "blocks"),
    ("general",  48, 32, True,  "blocks"),
    ("general",  48, 32, False, "blocks"),
    ("general",  33, 32, True,  "blocks"),                     # one column past a block
    ("general",  40, 32, False, "blocks"),
    ("lds",      64, 32, True,  "direct"),                     # whole blocks: the kernel's own widths
    ("lds",      32, 32, True,  "direct"),
    ("general",  96, 32, False, "direct"),
    ("general",  16, 32, True,  "direct"),                     # narrower than a block
    ("general",  48, 16, True,  "direct"),                     # fout is not 32
    ("table",   160, 16, False, "direct"),
]


@pytest.mark.parametrize("kernel,fin,fout,in_place,want", DX)
def test_dx_route(kernel, fin, fout, in_place, want):
    assert route(fin=fin, fout=fout, rev_kernel=kernel, basis_in_place=in_place).dx == want


# (x and gm have unit column stride, the fused kernel takes the shapes, the general kernel does, R * n * fout) -> dw
DW = [
    (True,  True,  False, BUDGET,     "fused"),
    (True,  True,  True,  BUDGET,     "fused"),
    (True,  False, True,  BUDGET,     "general"),
    (False, True,  True,  BUDGET,     "dense"),                # a strided x: neither kernel, whatever they say of the widths
    (False, True,  True,  BUDGET - 1, "slabs"),
    (True,  False, False, BUDGET,     "dense"),                # R * n * fout equal to the budget
    (True,  False, False, BUDGET - 1, "slabs"),                # one float over it
]


@pytest.mark.parametrize("unit,fused,general,budget,want", DW)
def test_dw_route(unit, fused, general, budget, want):
    got = route(fin=160, fout=16, rev_kernel="table", unit_strides=unit, fused_ok=fused, general_ok=general, q_budget=budget)
    assert got.dw == want


@pytest.mark.parametrize("bases,want", [(1, "gemm"), (64, "gemm"), (65, "torch"), (80, "torch")])
def test_dbasis_route(bases, want):
    assert route(bases=bases, rev_kernel="pair").dbasis == want


# (need_x, need_basis, need_att) -> the route of the PoSE step's layer (transposed / fused / gemm) with the parts nobody needs left out
NEEDS = [
    (True,  True,  True,  ("transposed", "fused", "gemm")),
    (False, True,  True,  (None,         "fused", "gemm")),
    (True,  False, True,  ("transposed", "fused", None)),      # datt alone still needs dW
    (True,  True,  False, ("transposed", "fused", "gemm")),
    (False, False, True,  (None,         "fused", None)),
    (False, True,  False, (None,         "fused", "gemm")),
    (True,  False, False, ("transposed", None,    None)),
    (False, False, False, (None,         None,    None)),
]


@pytest.mark.parametrize("need_x,need_basis,need_att,want", NEEDS)
def test_parts_nobody_needs_have_no_route(need_x, need_basis, need_att, want):
    got = route(need_x=need_x, need_basis=need_basis, need_att=need_att, rev_kernel="pair" if need_x else None,
                basis_in_place=True, unit_strides=True, fused_ok=True)
    assert got == RelBackwardRoute(*want) and (got.dx, got.dw, got.dbasis) == want
