"""Despeckling by merging, restated on the CPU with numpy on top of cc_reference.label (the definition stands in
include/segclip_hip.h, segclip_seg_sieve).  Slow and obvious on purpose; the GPU tests compare against it with torch.equal,
tests/test_seg_merge_cpu.py ties it to a scipy.ndimage formulation.

A round, per map L with `connectivity`, `skip_label` and `min_area`:
  components and areas are those of cc_reference.label; skipped pixels belong to none, never change and are never voted for;
  a component is small when its area < min_area, otherwise kept;
  the candidates of a small component are the kept components owning a pixel 4-adjacent (inside the map) to one of its pixels -
  4-adjacent whatever the connectivity, a diagonal touch is no contact;
  the winner is the candidate with the largest area, among equal areas the smallest label: max of (area << 8) | (255 - label);
  the small component's pixels take the winner's label; without a candidate it is an orphan and keeps its label.
Rounds: round r + 1 runs on the output of round r; after the last round only, orphans become orphan_fill if one is given."""
import numpy as np

from tests import cc_reference as cc


def merge_round(L, connectivity=8, skip_label=None, min_area=0):
    """one round on one map -> (the new map, the mask of the orphans' pixels)"""
    L = np.asarray(L, dtype=np.uint8)
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
                best = max(best, (int(area[j]) << 8) | (255 - int(L[yy, xx])))
        for p in pixels:
            if best:
                out.reshape(-1)[p] = 255 - (best & 255)
            else:
                orphans.reshape(-1)[p] = True
    return out, orphans


def chain(L, connectivity, skip_label, min_area, rounds):
    """[(map, orphans) after round 1, 2, .. rounds]: what every (rounds, orphan rule) pair of one setting shares"""
    steps, cur = [], np.asarray(L, dtype=np.uint8)
    for _ in range(rounds):
        cur, orphans = merge_round(cur, connectivity, skip_label, min_area)
        steps.append((cur, orphans))
    return steps


def finish(step, orphan_fill):
    """a chain's step as the result of a call that ends there"""
    out, orphans = step
    if orphan_fill is None:
        return out
    out = out.copy()
    out[orphans] = orphan_fill
    return out


def merge(L, connectivity=8, skip_label=None, min_area=0, orphan_fill=None, rounds=1):
    """`rounds` rounds on one map -> the new map"""
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= 8:
        raise ValueError("rounds is an integer in 1 .. 8")
    return finish(chain(L, connectivity, skip_label, min_area, rounds)[-1], orphan_fill)


def small_left(L, connectivity, skip_label, min_area):
    """the number of small components of a map"""
    ids = cc.label(L, connectivity, skip_label).reshape(-1)
    counts = np.bincount(ids[ids >= 0])
    return int(((counts > 0) & (counts < min_area)).sum())


# ------------------------------------------------------------------------------------------------ the test maps
def no_background_scene():
    """(scene, speckled): 48 x 80, three regions labelled 1..3 (there is no class 0), and the same with six 2 x 2 specks of
    another of the three labels, each inside one region.  Merging with min_area 16 restores the scene; fill=0 writes 24 pixels
    of a class that the scene does not contain."""
    scene = np.empty((48, 80), dtype=np.uint8)
    scene[:, :30], scene[:, 30:], scene[28:, 20:] = 1, 2, 3
    speckled = scene.copy()
    for (y, x) in ((4, 5), (20, 12), (6, 50), (14, 70), (36, 40), (42, 66)):
        speckled[y:y + 2, x:x + 2] = scene[y, x] % 3 + 1
    return scene, speckled


def nested_specks(h=12, w=14, cy=5, cx=6):
    """a 1-pixel speck (3) inside a 3 x 3 ring (2) around (cy, cx) in a region of 1s.  With min_area 9 both are small: round 1
    merges the ring into the region and leaves the inner pixel (its only neighbours were small), round 2 merges that too."""
    a = np.ones((h, w), dtype=np.uint8)
    a[cy - 1:cy + 2, cx - 1:cx + 2] = 2
    a[cy, cx] = 3
    return a


def area_tie(n=4):
    """1 x (2 n + 1): n pixels of 5, a speck (9), n pixels of 3.  The two candidates have equal areas: the speck becomes 3."""
    return np.asarray([5] * n + [9] + [3] * n, dtype=np.uint8).reshape(1, -1)


def checkerboard(h=7, w=9):
    return (np.add.outer(np.arange(h), np.arange(w)) % 2).astype(np.uint8)


def noise(seed=20261020, h=24, w=70):
    """3-label noise; the default map, 4-connected with min_area 6, has no small component left after two rounds"""
    return np.random.default_rng(seed).integers(0, 3, size=(h, w)).astype(np.uint8)


def corner_speck(th, tw):
    """2 x 2 tiles of th x tw.  A 1-pixel speck (9) at the last pixel (th - 1, tw - 1) of the first tile: its 4-neighbours lie in
    three tiles (the most that one pixel's can) and belong to four kept components, one-pixel-wide arms of labels 1..4 and areas
    tw - 1, th - 1, 40 and th + tw that lie in the four tiles.  The largest (4) touches the speck from the tile below only and
    has most of its pixels in the fourth tile."""
    a = np.zeros((2 * th, 2 * tw), dtype=np.uint8)
    y, x = th - 1, tw - 1
    a[y, :x] = 1                            # from the left, tile (0, 0)
    a[:y, x] = 2                            # from above, tile (0, 0)
    a[y, x + 1:x + 41] = 3                  # from the right, tile (0, 1)
    a[y + 1:, x] = 4                        # from below, tile (1, 0) ...
    a[2 * th - 1, x + 1:] = 4               # ... and on along the last row of tile (1, 1)
    a[y, x] = 9
    return a


def speck_across_tiles(th, tw):
    """2 rows: a region of 1s (2 x (tw - 2)), a 2 x 4 speck (9) across the border of the first two tile columns, a region of 2s
    (2 x (tw + 8)).  The larger candidate touches the speck only in the second tile."""
    a = np.empty((2, 2 * tw + 10), dtype=np.uint8)
    a[:, :tw - 2], a[:, tw - 2:tw + 2], a[:, tw + 2:] = 1, 9, 2
    return a


def serpentine_tail(th, tw):
    """cc_reference.serpentine over more than 2 x 2 tiles, the last pixel of its path replaced by a speck (7): both kept
    components, the path and the gaps, have almost all of their pixels in other tiles than the speck's"""
    a = cc.serpentine(2 * th + 3, 2 * tw + 3)
    ys, xs = np.nonzero(a == 1)
    y = int(ys.max())
    row = xs[ys == y]
    x = int(row.min()) if a[y - 1, int(row.min())] == 0 else int(row.max())   # the free end of the last row
    a[y, x] = 7
    return a


def diagonal_only(th, tw):
    """a 1-pixel speck (9) at a tile corner whose four 4-neighbours are 1-pixel specks of four other labels and whose diagonal
    neighbours belong to the kept background: with min_area 2 it has no candidate in round 1, an orphan"""
    a = np.zeros((th + 4, tw + 4), dtype=np.uint8)
    y, x = th, tw
    a[y, x] = 9
    a[y, x - 1], a[y, x + 1], a[y - 1, x], a[y + 1, x] = 11, 12, 13, 14
    return a


def frame_and_skip():
    """20 x 70 (2 x 2 tiles of 16 x 64): specks in the corners and on the edges of the picture frame, beside a bar of the skip
    label 255, and one walled in by skipped pixels (an orphan)"""
    a = np.full((20, 70), 1, dtype=np.uint8)
    a[:, 35:] = 2
    a[0, 0], a[0, 69], a[19, 0], a[19, 69] = 5, 5, 5, 5
    a[0, 20:22], a[19, 50:52], a[8:10, 0], a[12, 69] = 6, 6, 6, 6
    a[5:9, 30] = 255
    a[6, 31], a[7, 29] = 7, 7
    a[14:17, 40:43] = 255
    a[15, 41] = 8
    return a


def key_above_bit_16():
    """272 x 272: in raster order 65536 + 100 pixels of 3, a speck (9), 5000 pixels of 2, the rest 0.  The speck touches the 3s
    (left, up) and the 2s (right, down); the 3s win by bit 16 of their area alone: the low 16 bits say 100 < 5000."""
    a = np.zeros((272, 272), dtype=np.uint8)
    flat = a.reshape(-1)
    n3, n2 = 65536 + 100, 5000
    flat[:n3], flat[n3], flat[n3 + 1:n3 + 1 + n2] = 3, 9, 2
    return a


def column(repeat=4):
    """(21 * repeat, 1): runs of 1, 2 and 3 with lengths 4 1 2 5 2 6 1; the last run of a repeat joins the next one's first"""
    one = [1, 1, 1, 1, 2, 1, 1, 3, 3, 3, 3, 3, 2, 2, 3, 3, 3, 3, 3, 3, 1]
    return np.asarray(one * repeat, dtype=np.uint8).reshape(-1, 1)


def row(repeat=4):
    return np.ascontiguousarray(column(repeat).reshape(1, -1))
