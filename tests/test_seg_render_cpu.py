"""CPU: the yardsticks of tests/seg_render_reference.py against hand-computed values, and the host side of the rendering
interface (segclip_amd.segmentation: anchors_from_sums, default_group_palette, argument errors that need no device)."""
import numpy as np
import pytest
import torch

from segclip_amd import segmentation as seg
from tests import seg_render_reference as rr


def test_blend_reference_by_hand():
    img = np.array([[[10, 20, 30], [200, 100, 0]], [[255, 255, 255], [1, 2, 3]]], dtype=np.uint8)
    idx = np.array([[0, 1], [2, 5]])
    pal = np.array([[0, 0, 0], [255, 0, 10], [100, 100, 100]], dtype=np.uint8)
    got = rr.blend(img, idx, pal, 0.5)
    # 0.5 is exact: (p + c) / 2 truncated; index 5 is outside the palette and black
    want = np.array([[[5, 10, 15], [227, 50, 5]], [[177, 177, 177], [0, 1, 1]]], dtype=np.uint8)
    assert np.array_equal(got, want)
    # skip_zero leaves the pixel of index 0 alone; a BGR picture meets the palette reversed
    got = rr.blend(img, idx, pal, 0.5, skip_zero=True, reverse_channels=True)
    want[0, 0] = img[0, 0]
    want[0, 1] = [(200 + 10) // 2, 50, 255 // 2]
    assert np.array_equal(got, want)
    assert np.array_equal(rr.blend(img, idx, pal, 1.0)[0, 1], pal[1])
    # the rounding the kernel has to reproduce: two rounded fp64 products, one rounded sum, truncation; 1 - 0.8 is
    # 0.19999999999999996, so 5 * (1 - 0.8) + 0 * 0.8 truncates to 0 where the real number 1 would not
    a, b = 1 - 0.8, 0.8
    for p, c in ((5, 0), (5, 5), (10, 10), (0, 255), (255, 255), (35, 35)):
        one = rr.blend(np.full((1, 1, 3), p, np.uint8), np.zeros((1, 1), int), np.full((1, 3), c, np.uint8), 0.8)
        assert int(one[0, 0, 0]) == int(float(np.float64(p) * a + np.float64(c) * b))
    assert int(rr.blend(np.full((1, 1, 3), 5, np.uint8), np.zeros((1, 1), int), np.zeros((1, 3), np.uint8), 0.8)[0, 0, 0]) == 0


def test_blend_reference_fp32_and_fused_differ():
    """The issue's table: what an fp32 or a fused fp64 kernel would get wrong over all 256 x 256 (pixel, colour) pairs."""
    p = np.arange(256, dtype=np.float64)[:, None]
    c = np.arange(256, dtype=np.float64)[None, :]
    for opacity, n32 in ((0.8, 1201), (0.6, 208), (0.3, 1415)):
        a, b = 1 - opacity, opacity
        want = (p * a + c * b).astype(np.uint8)
        f32 = (p.astype(np.float32) * np.float32(a) + c.astype(np.float32) * np.float32(b)).astype(np.uint8)
        assert int((f32 != want).sum()) == n32


def test_seg2coord_reference_by_hand():
    m = np.array([[3, 3, 0, 0], [3, 0, 0, 0], [0, 0, 0, 7]])
    co = rr.seg2coord(m)
    assert sorted(co) == [0, 3, 7]
    assert np.allclose(co[3], [1 / 3, 1 / 3]) and np.allclose(co[7], [2, 3])
    assert rr.anchors(m) == [(0, 1, 1), (3, 0, 0), (7, 2, 3)]
    assert rr.anchors(m, P=5) == [(0, 1, 1), (3, 0, 0)]
    s = rr.sums(m, 8)
    assert s[3].tolist() == [3, 1, 1] and s[7].tolist() == [1, 2, 3] and s[0].tolist() == [8, 9, 14] and s[1].tolist() == [0, 0, 0]


def test_group_map_reference_by_hand():
    # two groups on a 1 x 2 grid, network size 1 x 4, output 1 x 8: resizing twice is linear in between and clamps outside
    soft = torch.tensor([[[1.0, 0.0]], [[0.0, 1.0]]])
    net = rr.sr.upsample(soft, 1, 4)
    assert torch.allclose(net[0, 0], torch.tensor([1.0, 0.75, 0.25, 0.0], dtype=torch.float64))
    groups, gap = rr.group_map(soft, (1, 4), (1, 8))
    assert groups.tolist() == [[0, 0, 0, 0, 1, 1, 1, 1]]
    assert gap.shape == (1, 8) and float(gap[0, 0]) == 1.0 and float(gap.min()) > 0.2
    # identity output size: the network-size groups
    g1, _ = rr.group_map(soft, (1, 4), (1, 4))
    assert g1.tolist() == [[0, 0, 1, 1]]
    # exact tie: the first maximum
    tie, gap = rr.group_map(torch.ones(3, 2, 2), (4, 4), (5, 3))
    assert int(tie.abs().sum()) == 0 and float(gap.abs().max()) == 0.0


def test_anchors_from_sums():
    rng = np.random.default_rng(3)
    maps = [rng.integers(0, 6, (17, 23)), np.full((4, 5), 2), rng.integers(3, 9, (9, 2))]
    P = 7
    sums = torch.from_numpy(np.stack([rr.sums(m, P) for m in maps]))
    got = seg.anchors_from_sums(sums)
    assert got == [rr.anchors(m, P) for m in maps]
    assert got[1] == [(2, 1, 2)]
    with pytest.raises(ValueError, match="int64"):
        seg.anchors_from_sums(sums.float())
    with pytest.raises(ValueError, match="int64"):
        seg.anchors_from_sums(sums[0])


def test_default_group_palette():
    for G in (1, 3, 8, 64, 256):
        p = seg.default_group_palette(G)
        assert tuple(p.shape) == (G, 3) and p.dtype == torch.uint8 and not p.is_cuda
        assert len({tuple(r) for r in p.tolist()}) == G, f"G={G}: colours repeat"
    assert torch.equal(seg.default_group_palette(8), seg.default_group_palette(8))
    for G in (0, 257):
        with pytest.raises(ValueError, match="256 colours"):
            seg.default_group_palette(G)


def test_host_side_argument_errors():
    raw = torch.zeros(4, 5, 3, dtype=torch.uint8)
    idx = torch.zeros(4, 5, dtype=torch.uint8)
    pal = torch.zeros(3, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.blend([raw], [idx], pal)
    for opacity in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="opacity"):
            seg.blend([raw], [idx], pal, opacity=opacity)
    with pytest.raises(ValueError, match="index maps"):
        seg.blend([raw, raw], [idx], pal)
    with pytest.raises(ValueError, match="empty image list"):
        seg.blend([], [], pal)
    with pytest.raises(ValueError, match="channel_order"):
        seg.blend([raw], [idx], pal, channel_order="rbg")
    assert "input_pred_label" in seg.VIS_MODES and len(seg.VIS_MODES) == 7
