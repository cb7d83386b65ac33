"""Connected components of label maps, restated on the CPU: numpy and a plain Python union-find, nothing else (the definition
stands in include/segclip_hip.h, segclip_seg_components).  Slow and obvious on purpose; the GPU tests compare against it with
torch.equal, tests/test_seg_objects_cpu.py ties it to scipy.ndimage."""
import numpy as np

RECORD = 10    # image, id, label, area, y0, x0, y1, x1, sum of y, sum of x


def _find(parent, a):
    root = a
    while parent[root] != root:
        root = parent[root]
    while parent[a] != root:
        parent[a], a = root, parent[a]
    return root


def label(L, connectivity=8, skip_label=None):
    """L (h, w) uint8 -> ids (h, w) int32: the smallest flat index y * w + x of the pixel's component, -1 where L is skip_label"""
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8")
    L = np.asarray(L)
    h, w = L.shape
    flat = L.reshape(-1).tolist()
    parent = list(range(h * w))
    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for y in range(h):
        for x in range(w):
            p = y * w + x
            if flat[p] == skip_label:
                continue
            for dy, dx in back:
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < w and flat[yy * w + xx] == flat[p]:
                    a, b = _find(parent, p), _find(parent, yy * w + xx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)   # the root is the component's smallest index
    ids = [(-1 if flat[p] == skip_label else _find(parent, p)) for p in range(h * w)]
    return np.asarray(ids, dtype=np.int32).reshape(h, w)


def components(maps, connectivity=8, skip_label=None, min_area=0, fill=0):
    """maps [(h, w) uint8] -> (ids [(h, w) int32], area_px [(h, w) int32], records (n, 10) int64 in ascending (image, id) order,
    cleaned [(h, w) uint8])"""
    ids_all, area_all, rows, cleaned_all = [], [], [], []
    for img, L in enumerate(maps):
        L = np.asarray(L, dtype=np.uint8)
        h, w = L.shape
        ids = label(L, connectivity, skip_label)
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


# ------------------------------------------------------------------------------------------------ the test maps
def _blocks(rng, h, w, side, values):
    """random blocks of side x side pixels drawn from `values`"""
    small = rng.choice(np.asarray(values, dtype=np.uint8), size=((h + side - 1) // side, (w + side - 1) // side))
    return np.ascontiguousarray(np.kron(small, np.ones((side, side), dtype=np.uint8))[:h, :w])


def serpentine(h, w):
    """a one-pixel path of 1s winding row by row inside a frame of 0s: the path is one long chain, the gaps the second component"""
    a = np.zeros((h, w), dtype=np.uint8)
    for y in range(1, h, 2):
        a[y, 1:w - 1] = 1
        if y + 2 < h:
            a[y + 1, w - 2 if (y // 2) % 2 == 0 else 1] = 1
    return a


def spiral(h, w):
    """a one-pixel path of 1s spiralling inwards with one pixel of 0s between its turns"""
    a = np.zeros((h, w), dtype=np.uint8)
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    y = x = d = turns = 0
    a[0, 0] = 1
    while turns < 2:
        dy, dx = dirs[d]
        ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < h and 0 <= nx < w and a[ny, nx] == 0 and not (0 <= my < h and 0 <= mx < w and a[my, mx] == 1):
            y, x, turns = ny, nx, 0
            a[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return a


def u_shapes(th, tw):
    """U shapes whose arms meet only in the lower tile row (one inside a tile column, one across two) and an inverted U whose
    arms hang into the lower tile row: an arm takes the id of the arm it meets late"""
    a = np.zeros((2 * th + 2, tw + 10), dtype=np.uint8)
    a[3:th + 3, 2] = 1
    a[1:th + 3, 6] = 1
    a[th + 2, 2:7] = 1
    a[2:th + 5, tw - 3] = 2
    a[0:th + 5, tw + 4] = 2
    a[th + 4, tw - 3:tw + 5] = 2
    a[th - 4, 10:21] = 3
    a[th - 4:2 * th + 2, 10] = 3
    a[th - 4:2 * th + 2, 20] = 3
    return a


def diagonals(th, tw):
    """name -> map: two pixels of 1 on 0s, diagonally adjacent across a four-tile corner or a tile edge"""
    out = {}
    for name, pts in (("diag_corner_main", [(th - 1, tw - 1), (th, tw)]), ("diag_corner_anti", [(th - 1, tw), (th, tw - 1)]),
                      ("diag_vertical_edge", [(5, tw - 1), (6, tw)]), ("diag_vertical_edge_anti", [(6, tw - 1), (5, tw)]),
                      ("diag_horizontal_edge", [(th - 1, 5), (th, 6)]), ("diag_horizontal_edge_anti", [(th - 1, 6), (th, 5)])):
        a = np.zeros((2 * th, 2 * tw), dtype=np.uint8)
        for y, x in pts:
            a[y, x] = 1
        out[name] = [a]
    return out


def cases(th, tw):
    """name -> [maps] for a tile of th x tw pixels"""
    rng = np.random.default_rng(20261019)
    big = (2 * th + 6, 2 * tw + 26)
    c = {
        "1x1": [np.full((1, 1), 3, dtype=np.uint8)],
        "1x9": [_blocks(rng, 1, 9, 1, (0, 1))],
        "7x1": [_blocks(rng, 7, 1, 1, (0, 1))],
        "long_row": [np.full((1, 8 * tw + 3), 5, dtype=np.uint8)],
        "long_column": [np.full((8 * th + 3, 1), 2, dtype=np.uint8)],
        "whole_image": [np.full((2 * th + 1, 2 * tw + 2), 1, dtype=np.uint8)],
        "serpentine": [serpentine(2 * th + 3, 2 * tw + 3)],
        "spiral": [spiral(2 * th + 3, 2 * tw + 3)],
        "u_shapes": [u_shapes(th, tw)],
        "checkerboard": [(np.add.outer(np.arange(th + 1), np.arange(tw + 3)) % 2).astype(np.uint8)],
        "noise_3_labels": [_blocks(rng, *big, 1, (0, 1, 2))],
        "blocks_21_labels": [_blocks(rng, *big, 4, tuple(range(21)))],
        "bytes_0_7_255": [_blocks(rng, *big, 2, (0, 7, 255))],
        "mixed_batch": [_blocks(rng, h, w, 2, (0, 1, 2)) for (h, w) in [(5, 7), (9, 11), (13, 3), big]],
        # 130 tiles: more row segments than one workgroup of the count scan takes (2048)
        "tall_noise": [_blocks(rng, 129 * th + 5, 3, 1, (0, 1, 2))],
    }
    c.update(diagonals(th, tw))
    return c
