"""The shared-candidate-list modes of the KGE baselines without a GPU: the shape and mode errors of KGEModel and
kge.sample_shared_candidates, the chunk rule, and that the cases of tests/kge_shared_cases.py are what tests/test_gpu_kge_shared.py
takes them for (G == B is the block reference; the three patterns are there).  The last test rebuilds the shared sampler's draw
from the documented stream and needs the GPU."""
import numpy as np
import pytest
import torch

import gripnet_amd
import kge_batch_cases as kb
import kge_cases as kc
import kge_loss_cases as lc
import kge_shared_cases as ks
import typed_candidates_cases as tc
from gripnet_amd import _hip, kge


def _model(name="DistMult", hidden=4):
    return gripnet_amd.KGEModel(name, 10, 3, hidden, 1.0)


def _block(B=6, G=3, K=4):
    return torch.zeros(2, B, dtype=torch.long), torch.zeros(B, dtype=torch.long), torch.zeros(G, K, dtype=torch.long)


@pytest.mark.parametrize("mode", sorted(ks.MODES.values()))
def test_shape_errors_name_the_shapes(mode):
    m = _model()
    positive, et, lists = _block()
    for call in (lambda p, t, n: m((p, n), t, mode=mode), lambda p, t, n: m.score((p, n), t, mode=mode),
                 lambda p, t, n: m.negative_sampling_loss(p, t, n, mode=mode)):
        with pytest.raises(ValueError, match=r"4 lists of negatives \(4, 4\) do not divide the 6 positives \(2, 6\)"):
            call(positive, et, torch.zeros(4, 4, dtype=torch.long))
        with pytest.raises(ValueError, match=r"1 <= G <= 6, got \(7, 4\)"):
            call(positive, et, torch.zeros(7, 4, dtype=torch.long))
        with pytest.raises(ValueError, match=r"1 <= G <= 6, got \(0, 4\)"):
            call(positive, et, torch.zeros(0, 4, dtype=torch.long))
        with pytest.raises(ValueError, match=r"\[G, K\].*got \(12,\)"):
            call(positive, et, torch.zeros(12, dtype=torch.long))
        with pytest.raises(ValueError, match=r"positive must have shape \[2, B\] with B >= 1, got \(3, 6\)"):
            call(torch.zeros(3, 6, dtype=torch.long), et, lists)
        with pytest.raises(ValueError, match=r"edge_type must have shape \[6\], got \(5,\)"):
            call(positive, et[:5], lists)
    with pytest.raises(ValueError, match=r"K >= 1, got \(3, 0\)"):
        m.negative_sampling_loss(positive, et, torch.zeros(3, 0, dtype=torch.long), mode=mode)
    with pytest.raises(ValueError, match=r"subsampling_weight must have shape \[6\], got \(5,\)"):
        m.negative_sampling_loss(positive, et, lists, mode=mode, subsampling_weight=torch.ones(5))
    # well-formed: the call goes on to the device check (there is no CPU path)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m((positive, lists), et, mode=mode)


def test_other_modes_are_unchanged():
    m = _model()
    positive, et, lists = _block()
    for mode in ("shared", "tail_shared", "tail-shared ", "Tail-Shared", ""):
        with pytest.raises(ValueError, match="mode {} not supported".format(mode)):
            m((positive, lists), et, mode=mode)
        with pytest.raises(ValueError, match="mode {} not supported".format(mode)):
            m.negative_sampling_loss(positive, et, lists, mode=mode)
    with pytest.raises(ValueError, match=r"negatives must have shape \[6, K\], got \(3, 4\)"):      # the block modes' own check
        m((positive, lists), et, mode="tail-batch")


@pytest.mark.parametrize("model", kc.MODELS)
def test_first_refused_width(model):
    """Entity rows of more than 128 floats: ValueError before anything touches a device; the largest admitted width passes on
    to the device check."""
    positive, et, lists = _block()
    wide = gripnet_amd.KGEModel(model, 10, 3, ks.first_refused_width(model), 12.0)
    assert wide.entity_dim > ks.MAX_ROW == _hip.KGE_SHARED_MAX_ROW
    for mode in ks.MODES.values():
        with pytest.raises(ValueError, match="at most 128 floats"):
            wide.score((positive, lists), et, mode=mode)
    widest = gripnet_amd.KGEModel(model, 10, 3, ks.widths(model)[-1], 12.0)
    assert widest.entity_dim == ks.MAX_ROW
    with pytest.raises(RuntimeError, match="MI355X only"):
        widest.score((positive, lists), et, mode="tail-shared")


def test_chunk_assignment():
    """b // (B // G) at the first and the last positive of every chunk."""
    for B, G, _ in list(ks.SHAPES.values()) + [(12, 4, 1), (7, 7, 1), (7, 1, 1)]:
        chunk = ks.chunk_of(B, G)
        size = B // G
        for g in range(G):
            assert int(chunk[g * size]) == g and int(chunk[(g + 1) * size - 1]) == g
        assert int(chunk[0]) == 0 and int(chunk[-1]) == G - 1
        lists = torch.arange(G * 3).view(G, 3)
        block = ks.expand_lists(lists, B)
        assert block.shape == (B, 3) and torch.equal(block, lists[chunk])


@pytest.mark.parametrize("side", ks.SIDES)
def test_g_equal_b_is_the_block_reference(side):
    """Shape d (G == B): the expansion is the lists themselves, and the case's triple list is kge_batch_cases.expand of them."""
    c = ks.case("ComplEx", side, 8, "d")
    assert c.G == c.B and torch.equal(c.negatives, c.lists)
    sample, et_list = kb.expand(c.positive, c.et, c.lists, side)
    assert torch.equal(c.sample, sample) and torch.equal(c.et_list, et_list)


@pytest.mark.parametrize("name", sorted(ks.SHAPES))
def test_cases_hold_their_patterns(name):
    for side in ks.SIDES:
        c = ks.case("TransE", side, 8, name)
        B, G, K = ks.SHAPES[name]
        assert (c.B, c.G, c.K) == (B, G, K) and c.lists.shape == (G, K) and c.E == B * K
        e = int(c.lists[0, 0])
        assert int(c.positive[0, 0]) == e and int(c.positive[1, 0]) == e          # the candidate is the positive's own head and tail
        if K > 1:
            assert int(c.lists[0, K - 1]) == e
        if G > 1:
            assert int(c.lists[1, 0]) == e
        for ids, unused in ((c.positive, c.unused_entity), (c.lists, c.unused_entity), (c.et, c.unused_relation)):
            assert not bool((ids == unused).any())
        # the reference's triple (b, k) reads its chunk's list
        chunk = ks.chunk_of(B, G)
        member = 1 if side == "tail" else 0
        assert torch.equal(c.sample[member].view(B, K), c.lists[chunk])
        assert torch.equal(c.sample[1 - member].view(B, K), kb.fixed_of(c.positive, side).unsqueeze(1).expand(B, K))
    assert ks.widths("TransE") == (1, 8, 36, 128) and ks.widths("DistMult") == (8, 36, 128)
    assert ks.widths("ComplEx") == ks.widths("RotatE") == (1, 8, 36, 64)


def test_sampler_errors():
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="G must be a positive integer"):
            kge.sample_shared_candidates(bad, 4, 10, device="cpu")
        with pytest.raises(ValueError, match="K must be a positive integer"):
            kge.sample_shared_candidates(3, bad, 10, device="cpu")
    with pytest.raises(ValueError, match="nentity must be an integer"):
        kge.sample_shared_candidates(3, 4, 0, device="cpu")
    with pytest.raises(ValueError, match=r"`out` must be an int64 \[3, 4\]"):
        kge.sample_shared_candidates(3, 4, 10, out=torch.zeros(3, 5, dtype=torch.long))
    with pytest.raises(ValueError, match="candidates_range must be a pair"):
        kge.sample_shared_candidates(3, 4, 10, candidates_range=(1, 2, 3), device="cpu")
    with pytest.raises(RuntimeError, match="MI355X only"):
        kge.sample_shared_candidates(3, 4, 10, device="cpu")


@pytest.mark.gpu
def test_shared_sampler_is_the_documented_stream(gpu):
    """kge.sample_shared_candidates element for element: the numpy model of the documented draw with the chunk index in the
    place of b (kge_loss_cases.draw: base = mix64(seed ^ (g K + k) * 0xD6E8FEB86659FD93)), kge.sample_candidates(known=None)
    given G positives, the stepped seed, a preallocated `out` inside a wider matrix, and one range for every list
    (typed_candidates_cases.draw)."""
    n = 19726
    zeros = np.zeros
    for G, K, seed in ((1, 1, 0), (3, 65, 7), (64, 8, 2 ** 63 + 5)):
        got = kge.sample_shared_candidates(G, K, n, seed=seed, device=gpu)
        want, flags, most = lc.draw(zeros(G, dtype=np.int64), zeros(G, dtype=np.int64), K, n, seed)
        assert got.dtype == torch.int64 and got.shape == (G, K) and got.device.type == "cuda"
        assert flags == 0 and most == 0 and np.array_equal(got.cpu().numpy(), want)
        positive = torch.randint(0, n, (2, G), generator=torch.Generator().manual_seed(G)).to(gpu)
        block = kge.sample_candidates(positive, torch.zeros(G, dtype=torch.long, device=gpu), K, n, known=None, seed=seed)
        assert torch.equal(got, block)
    step = torch.tensor([41], dtype=torch.int64, device=gpu)
    wide = torch.full((3, 70), -9, dtype=torch.int64, device=gpu)
    out = kge.sample_shared_candidates(3, 65, n, seed=7, step=step, out=wide[:, 2:67])
    assert out.data_ptr() == wide[:, 2:67].data_ptr() and int(step) == 41
    assert np.array_equal(out.cpu().numpy(), lc.draw(zeros(3, dtype=np.int64), zeros(3, dtype=np.int64), 65, n, 7, step=41)[0])
    assert bool((wide[:, :2] == -9).all()) and bool((wide[:, 67:] == -9).all())
    lo, hi = 600, 645
    ranged = kge.sample_shared_candidates(5, 33, n, seed=3, candidates_range=(lo, hi), device=gpu)
    want = tc.draw(zeros(5, dtype=np.int64), zeros(5, dtype=np.int64), 33, n, 3, [(lo, hi)])[0]
    assert np.array_equal(ranged.cpu().numpy(), want) and int(ranged.min()) >= lo and int(ranged.max()) < hi
    full = kge.sample_shared_candidates(5, 33, n, seed=3, candidates_range=(0, n), device=gpu)
    assert torch.equal(full, kge.sample_shared_candidates(5, 33, n, seed=3, device=gpu))
    _hip.raise_if_index_errors(gpu)
