"""The boundary bands and boundary areas of include/segclip_hip.h (segclip_seg_boundary) restated in numpy: the (2d+1)^2 window
by brute force on a map padded with -1, the areas by masks.  tests/test_seg_boundary_cpu.py ties it to
scipy.ndimage.binary_erosion, tests/test_seg_boundary_gpu.py holds the kernels to it with torch.equal.  Importing this module
needs numpy only."""
import math

import numpy as np


def radius(h, w, ratio=0.02):
    """Boundary IoU's dilation in pixels: the ratio of the diagonal, Python's round, at least 1"""
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def band(m, d):
    """(h, w) uint8 map -> (h, w) uint8 band bytes: bit 0 = some pixel of the map inside the (2d+1)^2 window has another byte,
    bit 1 = the window leaves the map"""
    h, w = m.shape
    pad = np.full((h + 2 * d, w + 2 * d), -1, dtype=np.int16)
    pad[d:d + h, d:d + w] = m
    centre = m.astype(np.int16)
    differs = np.zeros((h, w), dtype=bool)
    outside = np.zeros((h, w), dtype=bool)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            v = pad[dy:dy + h, dx:dx + w]
            outside |= v < 0
            differs |= (v >= 0) & (v != centre)
    return (differs.astype(np.uint8) | (outside.astype(np.uint8) << 1)).astype(np.uint8)


def plain_areas(pred, gt, C, ignore_index=255, reduce_zero_label=False, where=None):
    """mmseg's intersect_and_union as segclip_seg_areas states it, over the pixels of `where` -> (3, C) int64"""
    q, g = pred.astype(np.int64).ravel(), gt.astype(np.int64).ravel()
    keep = g != ignore_index
    if reduce_zero_label:
        keep &= g != 0
        g = g - 1
    if where is not None:
        keep &= where.ravel()
    out = np.zeros((3, C), dtype=np.int64)
    for k in range(C):
        out[0, k] = np.sum(keep & (q == k) & (g == k))
        out[1, k] = np.sum(keep & (q == k))
        out[2, k] = np.sum(keep & (g == k))
    return out


def areas(preds, gts, radii, C, ignore_index=255, reduce_zero_label=False):
    """lists of (h_i, w_i) uint8 maps and their radii -> (2, 3, C) int64: slot 0 Boundary IoU, slot 1 trimap"""
    out = np.zeros((2, 3, C), dtype=np.int64)
    for pred, gt, d in zip(preds, gts, radii):
        bp, bg = band(pred, d), band(gt, d)
        q, g = pred.astype(np.int64), gt.astype(np.int64)
        keep = g != ignore_index
        if reduce_zero_label:
            keep &= g != 0
            g = g - 1
        for k in range(C):
            out[0, 0, k] += np.sum(keep & (q == k) & (g == k) & (bp != 0) & (bg != 0))
            out[0, 1, k] += np.sum(keep & (q == k) & (bp != 0))
            out[0, 2, k] += np.sum(keep & (g == k) & (bg != 0))
        out[1] += plain_areas(pred, gt, C, ignore_index, reduce_zero_label, where=(bg & 1) != 0)
    return out


def metrics(a):
    """(2, 3, C) areas -> (mbIoU, trimap mIoU): a class absent from both sides of a slot is left out of its mean"""
    a = a.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        b = a[0, 0] / (a[0, 1] + a[0, 2] - a[0, 0])
        t = a[1, 0] / (a[1, 1] + a[1, 2] - a[1, 0])
    return float(np.nanmean(b)), float(np.nanmean(t))


# ---------------------------------------------------------------- the maps of the tests
def _blocks(rng, h, w, cell, labels):
    """random labels in cells of cell x cell pixels"""
    gh, gw = (h + cell - 1) // cell, (w + cell - 1) // cell
    coarse = np.asarray(labels, dtype=np.uint8)[rng.integers(0, len(labels), size=(gh, gw))]
    return np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:h, :w].copy()


def odd_pixel(h, w, y, x):
    a = np.zeros((h, w), dtype=np.uint8)
    a[y, x] = 1
    return a


def stripes(h, w, d, start, vertical):
    """on 0s, a stripe of 2d pixels beginning at `start` and, one stripe of 0s of 2d + 1 later, a stripe of 2d + 1 pixels: of
    the two only the wider one has a pixel whose window sees no other byte"""
    a = np.zeros((h, w), dtype=np.uint8)
    first = slice(start, start + 2 * d)
    second = slice(start + 4 * d + 1, start + 6 * d + 2)
    if vertical:
        a[:, first], a[:, second] = 1, 2
    else:
        a[first, :], a[second, :] = 1, 2
    return a


def cases(tile_h, tile_w):
    """name -> (map, [radii]) around a strip of tile_h rows x tile_w columns (the row pass works in chunks of tile_w columns):
    features sit on the strip's and the chunk's borders"""
    rng = np.random.default_rng(20261019)
    c = {
        "1x1": (np.full((1, 1), 7, dtype=np.uint8), [1, 3]),
        "1x130": (_blocks(rng, 1, 130, 3, (0, 1)), [1, 3]),
        "130x1": (_blocks(rng, 130, 1, 3, (0, 1)), [1, 3]),
        "constant_33x130": (np.full((33, 130), 4, dtype=np.uint8), [1, 5, 16, 64]),
        # the clipped square of the odd pixel crosses the strip's lower border and the chunk's right border
        "odd_pixel": (odd_pixel(40, 150, tile_h - 2, tile_w + 1), [1, 7, 16]),
        "odd_pixel_corner": (odd_pixel(40, 150, 0, 149), [1, 7, 16]),
        "checkerboard": ((np.add.outer(np.arange(tile_h + 5), np.arange(tile_w + 7)) % 2).astype(np.uint8), [1, 2]),
        "noise_3_labels": (_blocks(rng, tile_h + 9, 2 * tile_w + 11, 1, (0, 254, 255)), [1, 2, 5]),
        "blobs": (_blocks(rng, 2 * tile_h + 13, 2 * tile_w + 27, 11, (0, 1, 254, 255)), [1, 4, 9, 20]),
        "radius_100": (_blocks(rng, 60, 260, 37, (0, 1, 2)), [100]),
        "radius_128": (_blocks(rng, 2 * tile_h + 3, 300, 50, (0, 3, 255)), [128]),
    }
    for d in (1, 2, 9):
        # the narrow stripe straddles the border of the chunk (columns) or of the strip (rows)
        c[f"stripes_vertical_d{d}"] = (stripes(tile_h + 3, tile_w + 8 * d + 8, d, tile_w - d, True), [d])
        c[f"stripes_horizontal_d{d}"] = (stripes(tile_h + 8 * d + 8, tile_w + 3, d, tile_h - d, False), [d])
    return c


def mixed_call(rng=None):
    """the maps of one call of mixed sizes -> (maps, radii)"""
    rng = rng or np.random.default_rng(7)
    sizes, radii = [(1, 1), (17, 65), (50, 200), (96, 128)], [1, 2, 9, 3]
    return [_blocks(rng, h, w, 5, (0, 1, 2, 255)) for (h, w) in sizes], radii


def area_pair(rng, h, w, labels, ignore=255):
    """a random prediction and ground truth over `labels` with an ignored region in the ground truth"""
    gt = _blocks(rng, h, w, 9, labels)
    pred = gt.copy()
    noise = _blocks(rng, h, w, 4, labels)
    swap = _blocks(rng, h, w, 6, (0, 0, 1)).astype(bool)
    pred[swap] = noise[swap]
    gt[h // 3:h // 3 + 7, w // 4:w // 4 + 20] = ignore
    return pred, gt
