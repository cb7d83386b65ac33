"""Components, merge rounds, boundary bands and boundary areas of 16-bit label maps, restated on the CPU (the definitions stand
in include/segclip_hip.h: segclip_seg_components_wide, segclip_seg_sieve_wide, segclip_seg_boundary_wide - the uint8 ones with
"byte" read as "16-bit value").  Maps are (h, w) numpy uint16 arrays; a torch.int16 map goes in as .numpy().view(np.uint16).
cc_reference.label compares Python integers and serves any width as it is; everything that cast to uint8, packed a label into 8
bits or padded with an int16 -1 is restated here.  Slow and obvious on purpose; tests/test_seg_wide_post_cpu.py ties it to
scipy.ndimage and, through an order-preserving relabelling, to the uint8 restatements; the GPU tests compare with torch.equal."""
import numpy as np

from tests import boundary_reference as bd
from tests import cc_reference as cc

RECORD = cc.RECORD
TOP = 65535    # the largest label


def u16(m):
    m = np.asarray(m)
    if m.dtype == np.int16:
        return m.view(np.uint16)
    if m.dtype != np.uint16:
        raise TypeError(f"a 16-bit label map is a uint16 (or int16) array, got {m.dtype}")
    return m


# ------------------------------------------------------------------------------------------------ components
def components(maps, connectivity=8, skip_label=None, min_area=0, fill=0):
    """maps [(h, w) uint16] -> (ids [(h, w) int32], area_px [(h, w) int32], records (n, 10) int64 in ascending (image, id) order
    with the 16-bit label in column 2, cleaned [(h, w) uint16])"""
    ids_all, area_all, rows, cleaned_all = [], [], [], []
    for img, L in enumerate(maps):
        L = u16(L)
        h, w = L.shape
        ids = cc.label(L, connectivity, skip_label)
        area = np.zeros((h, w), dtype=np.int32)
        ys, xs = np.mgrid[0:h, 0:w]
        for i in np.unique(ids[ids >= 0]).tolist():       # ascending
            m = ids == i
            n = int(m.sum())
            area[m] = n
            y, x = ys[m], xs[m]
            rows.append([img, i, int(L.reshape(-1)[i]), n, int(y.min()), int(x.min()), int(y.max()) + 1, int(x.max()) + 1,
                         int(y.sum()), int(x.sum())])
        cleaned = L.copy()
        cleaned[(ids >= 0) & (area < min_area)] = fill
        ids_all.append(ids)
        area_all.append(area)
        cleaned_all.append(cleaned)
    return ids_all, area_all, np.asarray(rows, dtype=np.int64).reshape(-1, RECORD), cleaned_all


# ------------------------------------------------------------------------------------------------ merge rounds
def merge_round(L, connectivity=8, skip_label=None, min_area=0):
    """one round on one map -> (the new map, the mask of the orphans' pixels); the winner is the maximum of
    (area << 16) | (65535 - label) over the contacts"""
    L = u16(L)
    h, w = L.shape
    ids = cc.label(L, connectivity, skip_label)
    flat_ids = ids.reshape(-1)
    area = np.bincount(flat_ids[flat_ids >= 0], minlength=h * w)      # at a component's id: its pixel count
    out, orphans = L.copy(), np.zeros((h, w), dtype=bool)
    members = {}
    for p in np.flatnonzero(flat_ids >= 0).tolist():
        i = int(flat_ids[p])
        if area[i] < min_area:
            members.setdefault(i, []).append(p)
    for i, pixels in members.items():
        best = 0
        for p in pixels:
            y, x = divmod(p, w)
            for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                if not (0 <= yy < h and 0 <= xx < w):
                    continue
                j = int(ids[yy, xx])
                if j < 0 or j == i or area[j] < min_area:
                    continue
                best = max(best, (int(area[j]) << 16) | (TOP - int(L[yy, xx])))
        for p in pixels:
            if best:
                out.reshape(-1)[p] = TOP - (best & TOP)
            else:
                orphans.reshape(-1)[p] = True
    return out, orphans


def merge(L, connectivity=8, skip_label=None, min_area=0, orphan_fill=None, rounds=1):
    """`rounds` rounds on one map -> the new map; after the last round the orphans become orphan_fill if one is given"""
    cur = u16(L)
    orphans = np.zeros(cur.shape, dtype=bool)
    for _ in range(rounds):
        cur, orphans = merge_round(cur, connectivity, skip_label, min_area)
    if orphan_fill is not None:
        cur = cur.copy()
        cur[orphans] = orphan_fill
    return cur


# ------------------------------------------------------------------------------------------------ boundary
def band(m, d):
    """(h, w) uint16 map -> (h, w) uint8 band bytes: bit 0 = some pixel of the map inside the (2d+1)^2 window has another value,
    bit 1 = the window leaves the map.  Brute force on a map padded with -1, in int64 so that no label is negative."""
    m = u16(m)
    h, w = m.shape
    pad = np.full((h + 2 * d, w + 2 * d), -1, dtype=np.int64)
    pad[d:d + h, d:d + w] = m
    centre = m.astype(np.int64)
    differs = np.zeros((h, w), dtype=bool)
    outside = np.zeros((h, w), dtype=bool)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            v = pad[dy:dy + h, dx:dx + w]
            outside |= v < 0
            differs |= (v >= 0) & (v != centre)
    return (differs.astype(np.uint8) | (outside.astype(np.uint8) << 1)).astype(np.uint8)


def present(values, C, reduce_zero_label):
    """the classes below C that a map's raw values can count for"""
    shift = 1 if reduce_zero_label else 0
    return sorted({int(v) - shift for v in values if 0 <= int(v) - shift < C})


def areas(preds, gts, radii, C, ignore_index=TOP, reduce_zero_label=False):
    """lists of (h_i, w_i) uint16 maps and their radii -> (2, 3, C) int64: slot 0 Boundary IoU, slot 1 trimap.  Only the classes
    that occur are visited (C may be 1024); the ground-truth rule is boundary_reference.plain_areas'."""
    out = np.zeros((2, 3, C), dtype=np.int64)
    for pred, gt, d in zip(preds, gts, radii):
        pred, gt = u16(pred), u16(gt)
        bp, bg = band(pred, d), band(gt, d)
        q, g = pred.astype(np.int64), gt.astype(np.int64)
        keep = g != ignore_index
        if reduce_zero_label:
            keep &= g != 0
            g = g - 1
        tri = keep & ((bg & 1) != 0)
        for k in sorted(set(present(np.unique(pred), C, False)) | set(present(np.unique(gt), C, reduce_zero_label))):
            out[0, 0, k] += np.sum(keep & (q == k) & (g == k) & (bp != 0) & (bg != 0))
            out[0, 1, k] += np.sum(keep & (q == k) & (bp != 0))
            out[0, 2, k] += np.sum(keep & (g == k) & (bg != 0))
            out[1, 0, k] += np.sum(tri & (q == k) & (g == k))
            out[1, 1, k] += np.sum(tri & (q == k))
            out[1, 2, k] += np.sum(tri & (g == k))
    return out


def plain_areas(pred, gt, C, ignore_index=TOP, reduce_zero_label=False):
    """segclip_seg_areas_wide's (3, C) of one pair of maps: boundary_reference.plain_areas works in int64 and takes any width"""
    return bd.plain_areas(u16(pred), u16(gt), C, ignore_index, reduce_zero_label)


# ------------------------------------------------------------------------------------------------ the order-preserving injection
def rank_relabel(maps):
    """maps with at most 256 distinct values between them -> (the uint8 maps whose value is the RANK of the 16-bit value among
    the distinct ones, the sorted distinct values).  values[ranked] gives the maps back.  Equality and order of labels are kept,
    so components, bands and the sieve's tie-break (smallest label) cannot tell the two apart."""
    maps = [u16(m) for m in maps]
    values = np.unique(np.concatenate([m.reshape(-1) for m in maps]))
    if len(values) > 256:
        raise ValueError(f"{len(values)} distinct values do not fit a byte")
    return [np.searchsorted(values, m).astype(np.uint8) for m in maps], values


# ------------------------------------------------------------------------------------------------ the test maps
SHARED_LOW_BYTE = (1, 257, 513)          # a byte reader merges them
TOP_BIT_AND_SENTINEL = (255, 32768, 65535)   # sign extension, and a -1 sentinel in 16 bits
SIZES = ((1, 1), (1, 200), (40, 1), (17, 65), (33, 130), (48, 80))   # the last four cross the 16 x 64 tile and the 32 x 64 strip


def blocks(rng, h, w, side, values):
    """random blocks of side x side pixels drawn from `values`, uint16"""
    small = rng.choice(np.asarray(values, dtype=np.uint16), size=((h + side - 1) // side, (w + side - 1) // side))
    return np.ascontiguousarray(np.kron(small, np.ones((side, side), dtype=np.uint16))[:h, :w])


def batch(values, seed=20261021, side=2):
    """one map of every size of SIZES over `values`"""
    rng = np.random.default_rng(seed)
    return [blocks(rng, h, w, side, values) for (h, w) in SIZES]


def speck_between(left, right, speck=7, n=6, wider_right=0):
    """4 rows x (2 n + 2 + wider_right): columns 0 .. n are `left`, the others `right`, and a 2 x 2 speck in rows 1 .. 2 sits on
    the two columns where they meet, one column of each.  The regions keep 4 (n + 1) - 2 and 4 (n + 1 + wider_right) - 2 pixels:
    with wider_right = 0 the two candidates have EQUAL areas, and the speck touches both."""
    w = 2 * n + 2 + wider_right
    a = np.empty((4, w), dtype=np.uint16)
    a[:, :n + 1], a[:, n + 1:] = left, right          # each side owns one column of the middle pair
    a[1:3, n:n + 2] = speck                           # the speck takes 2 pixels of each: the areas stay equal
    return a


def nested(outer=300, ring=513, inner=40000, h=12, w=14, cy=5, cx=6):
    """a 1-pixel speck inside a 3 x 3 ring in a region: with min_area 9 round 1 merges the ring, round 2 the inner pixel"""
    a = np.full((h, w), outer, dtype=np.uint16)
    a[cy - 1:cy + 2, cx - 1:cx + 2] = ring
    a[cy, cx] = inner
    return a


def walled_in(wall=65535, speck=700):
    """a speck surrounded by pixels of `wall`; with skip_label=wall it has no candidate: an orphan"""
    a = np.full((7, 9), 2, dtype=np.uint16)
    a[2:5, 3:6] = wall
    a[3, 4] = speck
    return a
