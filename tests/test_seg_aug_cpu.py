"""CPU: tests/seg_aug_reference.py against a direct torch transcription of mmseg's aug_test, in fp64; TestAug.views against
hand-computed mmseg sizes and order; the flipped front-end restatement against F.interpolate of the flipped image."""
import pytest
import torch
import torch.nn.functional as F

from segclip_amd.segmentation import ImageTransform, TestAug, test_size
from tests import seg_aug_reference as sar
from tests import seg_frontend_reference as sfr


def _aug_test(view_logits, flags, oh, ow):
    """aug_test as mmseg writes it: per view resize -> softmax(dim=1) -> flip; sum / V; argmax."""
    total = None
    for lg, f in zip(view_logits, flags):
        p = F.interpolate(lg[None].double(), size=(oh, ow), mode="bilinear", align_corners=False).softmax(dim=1)
        if f & 1:
            p = p.flip(dims=(3,))
        if f & 2:
            p = p.flip(dims=(2,))
        total = p if total is None else total + p
    mean = total / len(view_logits)
    return mean[0], mean.argmax(dim=1)[0]


@pytest.mark.parametrize("flags,sizes,out", [
    ((0,), [(14, 19)], (23, 31)),
    ((0, 1), [(14, 19)] * 2, (23, 31)),
    ((0, 2), [(14, 19)] * 2, (9, 30)),
    ((0, 1, 0, 1), [(14, 19), (14, 19), (21, 28), (21, 28)], (23, 31)),
    ((0, 1, 2, 3), [(8, 8)] * 4, (5, 3)),
])
def test_mean_probs_equal_aug_test(flags, sizes, out):
    g = torch.Generator().manual_seed(len(flags) * 100 + out[0])
    logits = [torch.randn(7, H, W, generator=g, dtype=torch.float64) * 3 for (H, W) in sizes]
    mean = sar.mean_probs(logits, flags, *out)
    want, want_lab = _aug_test(logits, flags, *out)
    assert float((mean - want).abs().max()) <= 1e-12
    labels, gap = sar.labels_and_gap(mean)
    decided = gap > 1e-9
    assert bool(decided.any()) and bool((labels == want_lab)[decided].all())
    assert float((mean.sum(dim=0) - 1.0).abs().max()) <= 1e-12
    top2 = want.topk(2, dim=0).values
    assert float((gap - (top2[0] - top2[1])).abs().max()) <= 1e-12


def test_flip_back_and_spread():
    x = torch.arange(12.0).view(3, 4)
    assert torch.equal(sar.flip_back(x, 0), x)
    assert torch.equal(sar.flip_back(x, 1), x.flip(1)) and torch.equal(sar.flip_back(x, 2), x.flip(0))
    assert torch.equal(sar.flip_back(x, 3), x.flip(0, 1))
    mask = torch.zeros(4, 4, dtype=torch.bool)
    mask[0, 0] = True
    got = sar.spread_view(mask, 8, 8, 1)     # a horizontally flipped view: its left edge is the output's right edge
    assert bool(got[0, -1]) and not bool(got[0, 0]) and not bool(got[-1, -1])


def test_views_follow_mmseg():
    tf = ImageTransform()   # img_scale (2048, 224)
    # 375 x 500 at ratio 1: scale min(2048 / 500, 224 / 375) -> (224, 299); at 1.5: img_scale (3072, 336) -> (336, 448);
    # at 0.75: (1536, 168) -> (168, 224); at 1.25: (2560, 280) -> (280, 373) (500 * 280 / 375 = 373.33)
    assert TestAug().views(375, 500, tf) == [(224, 299, 0)]
    assert TestAug(flip=True).views(375, 500, tf) == [(224, 299, 0), (224, 299, 1)]
    assert TestAug(flip=True, flip_direction="vertical").views(500, 375, tf) == [(299, 224, 0), (299, 224, 2)]
    assert TestAug((1.0, 1.5), flip=True).views(375, 500, tf) == [(224, 299, 0), (224, 299, 1), (336, 448, 0), (336, 448, 1)]
    assert TestAug((0.75, 1.25)).views(375, 500, tf) == [(168, 224, 0), (280, 373, 0)]
    # mmseg: for each scale, unflipped then flipped; one direction only (a list of directions is not taken)
    assert [f for _, _, f in TestAug((1.0, 2.0), True, "vertical").views(100, 100, tf)] == [0, 2, 0, 2]
    with pytest.raises(ValueError, match="flip_direction"):
        TestAug(flip=True, flip_direction=["horizontal", "vertical"])
    # int() of the scaled img_scale, as MultiScaleFlipAug: (2048 * 1.3, 224 * 1.3) -> (2662, 291)
    assert TestAug((1.3,)).views(375, 500, tf) == [test_size(375, 500, (2662, 291)) + (0,)]
    with pytest.raises(ValueError, match="empty ratio list"):
        TestAug(img_ratios=[])
    with pytest.raises(ValueError, match="positive"):
        TestAug(img_ratios=[1.0, 0.0])
    with pytest.raises(ValueError, match="flip_direction"):
        TestAug(flip=True, flip_direction="both")


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_view_input_is_the_flipped_resize(flags):
    g = torch.Generator().manual_seed(5 + flags)
    raw = torch.randint(0, 256, (37, 53, 3), generator=g, dtype=torch.uint8)
    tf = ImageTransform()
    net = (61, 87)
    got = sar.view_input(raw, net, tf.mean, tf.inv_std, flags)
    x = raw.permute(2, 0, 1)[None].double()
    r = F.interpolate(x, size=net, mode="bilinear", align_corners=False)[0]
    want = (r - torch.tensor(tf.mean, dtype=torch.float64)[:, None, None]) * torch.tensor(tf.inv_std, dtype=torch.float64)[:, None, None]
    dims = [d for d, bit in ((2, 1), (1, 2)) if flags & bit]
    want = want.flip(dims) if dims else want
    assert float((got - want).abs().max()) <= 1e-9
    # flipping after the resize is not resizing the flipped image when the taps are not symmetric - it is here (bilinear
    # geometry is mirror-symmetric), which is why mmseg's order does not matter for the geometry, only for the byte order
    flipped_first = sfr.resize_normalise(raw.flip(dims=[d - 1 for d in dims]) if dims else raw, net, tf.mean, tf.inv_std)
    assert float((got - flipped_first).abs().max()) <= 1e-9
