"""numpy restatement of the integer SLIC superpixels and of the majority vote, written from the definitions in
include/segclip_hip.h (segclip_seg_superpixels, segclip_seg_vote).  Everything is integer arithmetic."""
import numpy as np


def grid(h, w, S):
    return -(-h // S), -(-w // S)


def init_centres(raw, S):
    """-> (K, 5) int64 rows (y, x, r, g, b): centre k = i * gw + j at the middle of cell (i, j), clamped to the picture"""
    h, w = raw.shape[:2]
    gh, gw = grid(h, w, S)
    cen = np.zeros((gh * gw, 5), dtype=np.int64)
    for i in range(gh):
        for j in range(gw):
            y, x = min(i * S + S // 2, h - 1), min(j * S + S // 2, w - 1)
            cen[i * gw + j] = (y, x, *raw[y, x].astype(np.int64))
    return cen


def assign(raw, cen, S, m):
    """-> (h, w) int32 ids: the candidates are visited in increasing index order and replace the best only when strictly
    nearer, so equal distances go to the smallest index"""
    h, w = raw.shape[:2]
    gh, gw = grid(h, w, S)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    ci, cj = ys // S, xs // S
    col = raw.astype(np.int64)
    best = np.full((h, w), np.iinfo(np.int64).max, dtype=np.int64)
    ids = np.full((h, w), -1, dtype=np.int64)
    for di in (-1, 0, 1):          # (di, dj) in row-major order = increasing k for one pixel
        for dj in (-1, 0, 1):
            ni, nj = ci + di, cj + dj
            ok = (ni >= 0) & (ni < gh) & (nj >= 0) & (nj < gw)
            k = np.where(ok, ni * gw + nj, 0)
            c = cen[k]
            dc2 = ((col - c[..., 2:5]) ** 2).sum(-1)
            ds2 = (ys - c[..., 0]) ** 2 + (xs - c[..., 1]) ** 2
            D = S * S * dc2 + m * m * ds2
            assert int(D.max()) < 2 ** 31, "D < 2^31 under the limits"
            take = ok & (D < best)
            best = np.where(take, D, best)
            ids = np.where(take, k, ids)
    assert (ids >= 0).all()
    return ids.astype(np.int32)


def update(raw, ids, cen):
    """floor-divided means of the members; a centre without members keeps its values.  -> (new centres, member counts)"""
    K = cen.shape[0]
    h, w = raw.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    flat = ids.reshape(-1).astype(np.int64)
    n = np.bincount(flat, minlength=K).astype(np.int64)
    vals = np.concatenate([ys.reshape(-1, 1), xs.reshape(-1, 1), raw.reshape(-1, 3).astype(np.int64)], axis=1)
    out = cen.copy()
    for c in range(5):
        s = np.zeros(K, dtype=np.int64)
        np.add.at(s, flat, vals[:, c])
        out[:, c] = np.where(n > 0, s // np.maximum(n, 1), cen[:, c])
    return out, n


def slic(raw, S, m, iters, with_counts=False):
    """raw (h, w, 3) uint8 -> (ids (h, w) int32, centres (K, 5) int32[, member counts of the final assignment])"""
    raw = np.asarray(raw)
    assert raw.ndim == 3 and raw.shape[2] == 3 and raw.dtype == np.uint8
    assert 4 <= S <= 64 and 1 <= m <= 64 and 0 <= iters <= 16
    cen = init_centres(raw, S)
    for _ in range(iters):
        ids = assign(raw, cen, S, m)
        cen, _ = update(raw, ids, cen)
    ids = assign(raw, cen, S, m)
    if with_counts:
        return ids, cen.astype(np.int32), np.bincount(ids.reshape(-1), minlength=cen.shape[0])
    return ids, cen.astype(np.int32)


def vote(labels, seg, K, C, min_share=0):
    """labels (h, w) unsigned integers, seg (h, w) int32 -> the snapped map, of the labels' dtype"""
    labels, seg = np.asarray(labels), np.asarray(seg)
    lab = labels.astype(np.int64).reshape(-1)
    s = seg.astype(np.int64).reshape(-1)
    votes = (lab < C) & (s >= 0) & (s < K)
    cnt = np.zeros((K, C), dtype=np.int64)
    np.add.at(cnt, (s[votes], lab[votes]), 1)
    tot, top = cnt.sum(1), cnt.max(1)
    win = cnt.argmax(1)                      # the first (smallest) class that reaches the maximum
    snaps = (tot > 0) & (100 * top >= min_share * tot)
    out = lab.copy()
    take = votes.copy()
    take[votes] = snaps[s[votes]]
    out[take] = win[s[take]]
    return out.reshape(labels.shape).astype(labels.dtype)


def block_picture():
    """The seeded 48 x 60 picture of flat 6 x 6 blocks in three grey levels plus a little noise: at S = 7, m = 1, T = 6 some of its
    63 centres lose every pixel."""
    rng = np.random.default_rng(0)
    b = int(rng.integers(2, 7))
    base = rng.integers(0, 3, (8, 10, 1), dtype=np.uint8) * 120
    raw = np.repeat(np.repeat(base, b, axis=0), b, axis=1)
    raw = np.repeat(raw, 3, axis=2)
    return raw + rng.integers(0, 3, raw.shape, dtype=np.uint8)
