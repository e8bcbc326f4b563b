"""What tests/test_gpu_scales.py leans on, checked without a GPU: the fp32 oracle is homogeneous bit for bit under
power-of-two factors (so any kernel that is linear in an input must be), and the per-element measure of
tests/scale_cases.py tells a three-term split from a two-term one on a product whose rows differ in scale."""
import pytest
import torch

import scale_cases as sc
from oracle import gripnet_oracle as orc


def _graph(n, e, gen):
    return torch.randint(0, n, (2, e), generator=gen)


@pytest.mark.parametrize("s", sc.pow2_scales)
def test_fp32_oracle_is_homogeneous_bit_for_bit(s):
    gen = torch.Generator().manual_seed(7)
    n, fin, fout, R, B = 300, 24, 20, 4, 3
    x = sc.mixed_scale(torch.randn(n, fin, generator=gen), -8, 8, 0, gen)
    w, b = torch.randn(fin, fout, generator=gen) * 0.1, torch.randn(fout, generator=gen)
    ei, ew = _graph(n, 3000, gen), torch.rand(3000, generator=gen) + 0.1
    for weights in (None, ew):
        assert torch.equal(orc.gcn_forward(x * s, w, b * s, ei, weights), orc.gcn_forward(x, w, b, ei, weights) * s)

    blocks = [_graph(n, k, gen) for k in (900, 0, 40, 700)]
    rei = torch.cat(blocks, dim=1)
    rl = torch.tensor([[0, 900], [900, 900], [900, 940], [940, 1640]])
    basis, att = torch.randn(B, fin, fout, generator=gen) * 0.2, torch.randn(R, B, generator=gen) * 0.5
    root = torch.randn(fin, fout, generator=gen) * 0.2
    base = orc.rgcn_forward(x, rei, rl, basis, att, root, b)
    assert torch.equal(orc.rgcn_forward(x * s, rei, rl, basis, att, root, b * s), base * s)
    # linear in (basis, root, bias) and in (att, root, bias) jointly: the root term and the bias do not pass through W_r
    assert torch.equal(orc.rgcn_forward(x, rei, rl, basis * s, att, root * s, b * s), base * s)
    assert torch.equal(orc.rgcn_forward(x, rei, rl, basis, att * s, root * s, b * s), base * s)

    z, d = torch.randn(n, fout, generator=gen), torch.randn(R, fout, generator=gen) * 0.2
    et = torch.randint(0, R, (rei.shape[1],), generator=gen)
    logits = orc.distmult(z, rei, et, d, sigmoid=False)
    assert torch.equal(orc.distmult(z, rei, et, d * s, sigmoid=False), logits * s)
    if 2.0 ** -40 <= s <= 2.0 ** 40:     # s^2 of the outer factors leaves single products of small entries denormal
        assert torch.equal(orc.distmult(z * s, rei, et, d, sigmoid=False), logits * (s * s))


def test_componentwise_refuses_what_it_must():
    ref = torch.tensor([1.0, 0.0, 2.0], dtype=torch.float64)
    mag = torch.tensor([1.0, 0.0, 4.0], dtype=torch.float64)
    assert sc.componentwise(torch.tensor([1.0, 0.0, 3.0]), ref, mag) == 0.25
    with pytest.raises(AssertionError, match="exactly zero"):
        sc.componentwise(torch.tensor([1.0, 1e-30, 2.0]), ref, mag)
    with pytest.raises(AssertionError, match="non-finite"):
        sc.componentwise(torch.tensor([1.0, 0.0, float("inf")]), ref, mag)


def test_mixed_scale_is_exact_and_seeded():
    t = torch.randn(50, 7, generator=torch.Generator().manual_seed(1))
    a = sc.mixed_scale(t, -30, 30, 0, torch.Generator().manual_seed(2))
    b = sc.mixed_scale(t, -30, 30, 0, torch.Generator().manual_seed(2))
    assert torch.equal(a, b)
    e = torch.log2((a / t)[:, 0])
    assert torch.equal(e, e.round()) and e.min() >= -30 and e.max() <= 30 and e.unique().numel() > 20
    assert torch.equal((a / t), (a / t)[:, :1].expand(-1, 7))
    cols = sc.mixed_scale(t, -10, 10, 1, torch.Generator().manual_seed(3)) / t
    assert torch.equal(cols, cols[:1].expand(50, -1))


def test_componentwise_separates_three_terms_from_two():
    """[2048 x 128] @ [128 x 64], row exponents of A in [-30, 30], column exponents of B in [-10, 10]: the two-term split's
    error is invisible to a max-norm (1e-5 of the largest output) and far above fp32's per element; the three-term split's is
    far below."""
    gen = torch.Generator().manual_seed(3)
    a = sc.mixed_scale(torch.randn(2048, 128, generator=gen), -30, 30, 0, gen)
    b = sc.mixed_scale(torch.randn(128, 64, generator=gen) * 0.2, -10, 10, 1, gen)
    ref64, mag64 = sc.gemm_ref(a, b)
    rho = {"ref32": sc.componentwise(a @ b, ref64, mag64)}
    rho["three"] = sc.componentwise(sc.split_matmul(a, b, 3), ref64, mag64)
    rho["two"] = sc.componentwise(sc.split_matmul(a, b, 2), ref64, mag64)
    line = sc.show("emulated split, mixed 2048x128x64", rho)
    assert 0.5 * sc.U <= rho["ref32"] <= 16 * sc.U, line          # (the reference's own error is what the issue measured: a few u)
    assert rho["three"] < 2 * 1.5 * rho["ref32"] < rho["two"], line
    maxnorm = float((sc.split_matmul(a, b, 2) - ref64).abs().max() / ref64.abs().max())
    assert maxnorm < 2e-5, maxnorm                                  # what every other tolerance of the suite would have seen
