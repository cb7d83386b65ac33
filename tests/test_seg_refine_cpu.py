"""The fp64 restatement of the pixel-adaptive refinement (tests/pamr_reference.py) checked on its own, without a GPU: the
properties of the definition that the kernel tests then lean on, and that the refinement moves a displaced border back onto a
picture edge."""
import pytest
import torch

from tests import pamr_reference as pr

MEAN, STD = (122.7709383, 116.7460125, 104.09373615), (68.5005327, 66.6321579, 70.32316305)


def _random_scene(h, w, C, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 256, (h, w, 3), generator=g).to(torch.uint8)
    labels = torch.randint(0, C, (h, w), generator=g).to(torch.uint8)
    return raw, labels


def test_zero_iterations_is_the_identity():
    raw, labels = _random_scene(9, 13, 4, 1)
    labels[2, 3] = 200                                   # a byte >= C belongs to no plane and stays
    out, m = pr.refine(raw, labels, 4, MEAN, STD, (1, 2), 0)
    assert torch.equal(out, labels)
    assert torch.equal(m, pr.one_hot(labels, 4))
    assert float(m[:, 2, 3].sum()) == 0.0


@pytest.mark.parametrize("dilations,iters", [((1,), 3), ((1, 2), 5), ((8, 16), 10)])
def test_planes_sum_to_one_and_stay_in_range(dilations, iters):
    raw, labels = _random_scene(20, 27, 5, 2)
    w = pr.weights(raw, MEAN, STD, dilations)
    assert w.shape[0] == 8 * len(dilations)
    assert float((w.sum(dim=0) - 1).abs().max()) < 1e-12 and float(w.min()) >= 0.0
    m = pr.planes(raw, labels, 5, MEAN, STD, dilations, iters)
    assert float((m.sum(dim=0) - 1).abs().max()) < 1e-12
    assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0 + 1e-12


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("dilations", [(1,), (1, 2), (4, 8), (1, 2, 4)])
def test_constant_picture_has_uniform_weights(dilations, dtype):
    raw = torch.full((7, 9, 3), 131, dtype=torch.uint8)
    w = pr.weights(raw, MEAN, STD, dilations, dtype=dtype)
    assert torch.equal(w, torch.full_like(w, 1.0 / (8 * len(dilations))))


@pytest.mark.parametrize("dilations,iters", [((1, 2), 5), ((1,), 8), ((4, 8), 5)])
def test_constant_picture_is_exact_in_fp32(dilations, iters):
    """what the kernel's bit-equality cases rest on: every weight a power of two, every partial sum exact"""
    raw = torch.full((24, 40, 3), 77, dtype=torch.uint8)
    labels = torch.randint(0, 5, (24, 40), generator=torch.Generator().manual_seed(5)).to(torch.uint8)
    l64, m64 = pr.refine(raw, labels, 5, MEAN, STD, dilations, iters)
    l32, m32 = pr.refine(raw, labels, 5, MEAN, STD, dilations, iters, dtype=torch.float32)
    assert torch.equal(m32.double(), m64) and torch.equal(l32, l64)


def test_reverse_channels_matches_a_flipped_picture():
    raw, labels = _random_scene(11, 8, 3, 3)
    a = pr.planes(raw, labels, 3, MEAN, STD, (1, 2), 2, reverse_channels=True)
    b = pr.planes(raw.flip(2), labels, 3, MEAN, STD, (1, 2), 2)
    assert float((a - b).abs().max()) < 1e-12


@pytest.mark.parametrize("h,w,noise,shift,dilations", [(96, 128, 12, (5, -5), (8, 16)), (56, 80, 10, (3, -4), (1, 2, 4))])
def test_refinement_snaps_a_displaced_border(h, w, noise, shift, dilations):
    raw, labels, gt = pr.snapping_scene(h, w, noise, shift)
    before = pr.miou(labels, gt, 3)
    out, _ = pr.refine(raw, labels, 3, MEAN, STD, dilations, 10)
    after = pr.miou(out, gt, 3)
    print(f"snapping {h}x{w} {dilations}: mIoU {before:.4f} -> {after:.4f}")
    assert before < 0.95
    assert after - before > 0.05
