"""Yardsticks of the rendering of segmentation results, written from the definitions (not from the reference's program text).

  blend       : the overlay of blend_result in numpy: every byte is (img * (1 - opacity) + color * opacity).astype(uint8)
                with img and color uint8 arrays and opacity a Python float, i.e. fp64: two rounded products, one rounded
                sum, truncation.  The palette is RGB; a BGR image meets it reversed.  An index outside the palette is
                black; with skip_zero the pixels of index 0 are not touched.
  seg2coord   : per index present in a map, the mean (y, x) of its pixels in fp64; anchors = its truncation to int32.
  group_map   : the soft assignment resized bilinearly (align_corners=False) to the network size, resized again to the
                output size, first maximum over the groups - in a dtype (float64 = the yardstick), with the top-two gap.
"""
import numpy as np
import torch

from tests import seg_reference as sr


def blend(img, seg, palette, opacity, skip_zero=False, reverse_channels=False):
    """img (h, w, 3) uint8, seg (h, w) integer, palette (P, 3) uint8 RGB -> (h, w, 3) uint8."""
    img, seg, palette = np.asarray(img), np.asarray(seg), np.asarray(palette)
    assert img.dtype == np.uint8 and palette.dtype == np.uint8 and 0 < opacity <= 1.0
    color = np.zeros(seg.shape + (3,), dtype=np.uint8)
    for index, rgb in enumerate(palette):
        color[seg == index, :] = rgb
    if reverse_channels:
        color = color[..., ::-1]
    out = img.copy()
    if skip_zero:
        fg = seg != 0
        out[fg] = (img[fg] * (1 - opacity) + color[fg] * opacity).astype(np.uint8)
        return out
    return (img * (1 - opacity) + color * opacity).astype(np.uint8)


def seg2coord(seg):
    """(h, w) integer map -> {index: fp64 array (mean y, mean x)} for the indices present."""
    seg = np.asarray(seg)
    ys, xs = np.meshgrid(np.arange(seg.shape[0]), np.arange(seg.shape[1]), indexing="ij")
    coords = np.stack([ys, xs], axis=-1)
    return {int(index): coords[seg == index].mean(axis=0) for index in np.unique(seg)}


def anchors(seg, P=None):
    """[(index, y, x)] as the demo places its texts: seg2coord truncated to int32; indices >= P left out."""
    return [(k, int(v.astype(np.int32)[0]), int(v.astype(np.int32)[1])) for k, v in sorted(seg2coord(seg).items())
            if P is None or k < P]


def sums(seg, P):
    """(P, 3) int64: pixel count, sum of y, sum of x per index < P."""
    seg = np.asarray(seg)
    ys, xs = np.meshgrid(np.arange(seg.shape[0]), np.arange(seg.shape[1]), indexing="ij")
    out = np.zeros((P, 3), dtype=np.int64)
    for k in range(P):
        m = seg == k
        out[k] = (int(m.sum()), int(ys[m].sum()), int(xs[m].sum()))
    return out


def group_map(soft, net, out, dtype=torch.float64):
    """soft (G, gh, gw), network size (H, W), output size (oh, ow) -> (groups (oh, ow) long, gap (oh, ow) = top value - second
    value of the twice-resized assignment; inf for G = 1)."""
    up = sr.upsample(sr.upsample(soft, net[0], net[1], dtype), out[0], out[1], dtype)
    groups = up.argmax(dim=0)
    if up.shape[0] > 1:
        top2 = up.topk(2, dim=0).values
        gap = top2[0] - top2[1]
    else:
        gap = torch.full(groups.shape, float("inf"), dtype=dtype)
    return groups, gap
