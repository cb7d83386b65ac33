"""CPU: the yardstick of the training front end.  tests/train_frontend_reference.py (the integer restatement the GPU tests compare
with) against Pillow's own outputs (tests/golden/train_frontend_pil.npz, and Pillow directly where it is installed), against
ATen's nearest index, and segclip_amd.transforms' host side (sampler, eval geometry, value table, label boxes) against the
restatement.  Every comparison is exact."""
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from segclip_amd.transforms import CLIP_MEAN, CLIP_STD, RawImageTransform
from tests import train_frontend_reference as R
from tests.helpers import load_golden

NEAREST_SIZES = [(640, 224), (480, 224), (224, 224), (1, 224), (2, 32), (37, 32), (53, 32), (225, 224), (223, 224), (1000, 224),
                 (333, 224), (500, 224), (375, 224), (100, 14), (7, 28)]


def test_restatement_equals_golden():
    g = load_golden("train_frontend_pil.npz")
    for name in R.GOLDEN_CASES:
        assert np.array_equal(R.case_resized(name), g[name]), name
    for name in R.GOLDEN_EVAL:
        assert np.array_equal(R.eval_bytes(name), g[name]), name


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_pillow(name):
    Image = pytest.importorskip("PIL.Image")
    _, (x0, y0, bw, bh), (RW, RH), _, _, _, _ = R.CASES[name]
    im = Image.fromarray(R.case_source(name)).crop((x0, y0, x0 + bw, y0 + bh)).resize((RW, RH), Image.BICUBIC)
    assert np.array_equal(R.case_resized(name), np.asarray(im))


def test_crop_then_resize_is_not_resize_with_box():
    """the trap: the filter clamps at the crop's edges; a restatement that filtered across them would pass no golden case"""
    Image = pytest.importorskip("PIL.Image")
    a = R.source("rand", 300, 400, 7)
    box = (30, 20, 330, 270)
    crop_resize = np.asarray(Image.fromarray(a).crop(box).resize((224, 224), Image.BICUBIC))
    resize_box = np.asarray(Image.fromarray(a).resize((224, 224), Image.BICUBIC, box=box))
    assert np.array_equal(R.resize_crop(a, box, 224, 224), crop_resize)
    assert int((crop_resize != resize_box).sum()) > 0


def test_large_downscale_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    a = R.source("rand", 600, 800, 3)
    want = np.asarray(Image.fromarray(a).resize((224, 224), Image.BICUBIC))
    assert np.array_equal(R.resize_crop(a, (0, 0, 800, 600), 224, 224), want)


@pytest.mark.parametrize("n_in,n_out", NEAREST_SIZES)
def test_nearest_index_is_atens(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
    want = F.interpolate(src, size=(1, n_out), mode="nearest").view(-1).long().numpy()
    assert np.array_equal(R.nearest_index(n_in, n_out), want)


def test_integer_nearest_index_differs():
    """d * in // out is not ATen's index: the yardstick above tells them apart.  On this size list they part at 480 -> 224
    (fp32 15 / 7 rounds down, so destination 7 k can land one below 15 k); at 640 -> 224 fp32 20 / 7 rounds up and they agree."""
    assert int((R.nearest_index(480, 224) != R.nearest_index_integer(480, 224)).sum()) >= 1
    assert sum(int((R.nearest_index(i, o) != R.nearest_index_integer(i, o)).sum()) for (i, o) in NEAREST_SIZES) >= 1


def test_patch_labels_restatement_equals_reference_expressions():
    """the restatement against the reference's own lines (interpolate on floats, np.mean, astype) without einops"""
    rng = np.random.default_rng(5)
    for (h, w), box, flags, size, patch in (((48, 64), (3, 5, 60, 40), 0, 32, 16), ((37, 53), (0, 0, 0, 0), 3, 32, 16),
                                            ((64, 48), (2, 1, 47, 63), 1, 28, 14)):
        seg = rng.integers(0, 2000, (h, w)).astype(np.int32)
        x0, y0, x1, y1 = box
        m = seg if (y1 - y0 < 2 or x1 - x0 < 2) else seg[y0:y1, x0:x1]
        if flags & 1:
            m = np.flip(m, axis=1)
        if flags & 2:
            m = np.flip(m, axis=0)
        t = torch.tensor(m.copy()).reshape(1, 1, *m.shape)
        t = F.interpolate(t.to(torch.float), size=size, mode="nearest").squeeze().to(torch.long).numpy()
        P = size // patch
        t = t.reshape(P, patch, P, patch).transpose(0, 2, 1, 3).reshape(P * P, patch * patch)
        want = np.mean(t, axis=-1).reshape(P, P).astype(np.int64)
        assert np.array_equal(R.patch_labels(seg, box, flags, size, patch), want)


def test_sampler_draw_for_draw():
    tf = RawImageTransform(is_train=True)
    a, b = random.Random(11), random.Random(11)
    sizes = random.Random(2)
    for _ in range(1000):
        h, w = sizes.randint(1, 700), sizes.randint(1, 700)
        assert tf.sample(h, w, a) == R.sample(h, w, b)
    assert a.random() == b.random()   # the same number of draws


@pytest.mark.parametrize("h,w,want", [(1000, 100, (433, 0, 133, 100)), (100, 1000, (0, 433, 100, 133))])
def test_sampler_fallback(h, w, want):
    """no crop of half the area and a ratio in [3/4, 4/3] fits: ten attempts, then the central crop"""
    tf = RawImageTransform(is_train=True)
    rng, twin = random.Random(3), random.Random(3)
    box, coord = tf.sample(h, w, rng)
    assert box == want == R.sample(h, w, random.Random(3))[0]
    for _ in range(20):   # exactly ten attempts of two draws each
        twin.random()
    assert rng.random() == twin.random()
    i, j, ch, cw = box
    assert coord == [j / (w - 1), i / (h - 1), (j + cw - 1) / (w - 1), (i + ch - 1) / (h - 1)]


def test_one_pixel_wide_coord():
    tf = RawImageTransform(is_train=True)
    for h, w in ((50, 1), (1, 50), (1, 1)):
        box, coord = tf.sample(h, w, random.Random(0))
        assert coord == [0., 0., 0., 0.] and box == R.sample(h, w, random.Random(0))[0]
    assert tf.label_box([0., 0., 0., 0.], 40, 30) == (0, 0, 0, 0, 0)   # thinner than 2: the whole map


@pytest.mark.parametrize("h,w,want", [
    (500, 375, (224, 298, 0, 37)),        # portrait: int(224 * 500 / 375) = 298
    (375, 500, (298, 224, 37, 0)),        # landscape
    (300, 300, (224, 224, 0, 0)),         # square
    (224, 301, (301, 224, 38, 0)),        # the short side is the size already: unchanged; round((301 - 224) / 2.0) = round(38.5)
    (225, 224, (224, 225, 0, 0)),         # round(0.5) = 0
])
def test_eval_geometry(h, w, want):
    assert RawImageTransform().eval_geometry(h, w) == want == R.eval_geometry(h, w, 224)


def test_value_table():
    tf = RawImageTransform()
    want = ((torch.arange(256, dtype=torch.float32) / 255).view(-1, 1) - torch.tensor(CLIP_MEAN, dtype=torch.float32)) \
        / torch.tensor(CLIP_STD, dtype=torch.float32)
    got = tf.value_table()
    assert got.dtype == torch.float32 and tuple(got.shape) == (256, 3) and torch.equal(got, want) and torch.equal(got, R.value_table())
    assert tf.value_table() is got
    # ToTensor + Normalize of an image of every byte
    img = torch.arange(256, dtype=torch.uint8).view(16, 16, 1).expand(16, 16, 3)
    t = img.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    t = (t - torch.tensor(CLIP_MEAN, dtype=torch.float32).view(3, 1, 1)) / torch.tensor(CLIP_STD, dtype=torch.float32).view(3, 1, 1)
    assert torch.equal(t, got[img[..., 0].long()].permute(2, 0, 1))


def test_label_box_rounds_the_coord_to_fp32():
    """the box from the coord as the reference holds it, a float32 tensor (rawimage_util.py:108-120)"""
    tf = RawImageTransform(is_train=True)
    rng = random.Random(9)
    for _ in range(300):
        h, w = rng.randint(2, 600), rng.randint(2, 600)
        _, coord = tf.sample(h, w, rng)
        if rng.random() < 0.3:
            coord = [coord[2], coord[1], coord[0], coord[3]]
        got = tf.label_box(coord, h, w)
        assert got == R.label_box(coord, h, w)
        t = torch.Tensor(coord)   # the reference's coord
        xu, yu, xl, yl = (float(v) for v in t)
        flip = xu > xl
        if flip:
            xu, xl = xl, xu
        assert got == (int(xu * w), int(yu * h), math.ceil(xl * w), math.ceil(yl * h), int(flip))
