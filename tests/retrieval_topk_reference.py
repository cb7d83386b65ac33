"""The yardstick of the top-K search: numpy, fp64.  The definition is this project's (include/segclip_hip.h,
segclip_amd/retrieval.py) and is restated here.

    Q (Nq, E) queries, X (Nx, E) gallery, s[q, j] = <Q[q], X[j]>
    Row q of the result holds the first min(k, Nx) gallery indices under the total order "higher score first, equal scores:
    lower index first", and their scores.  Positions from min(k, Nx) on hold idx = -1, val = -inf.
"""
import numpy as np


def scores(Q, X):
    return np.asarray(Q, dtype=np.float64) @ np.asarray(X, dtype=np.float64).T


def topk_of_scores(s, k):
    """(Nq, Nx) scores -> (idx (Nq, k) int64, val (Nq, k) of s's dtype): a stable sort on (-score, index)."""
    Nq, Nx = s.shape
    kk = min(k, Nx)
    idx = np.full((Nq, k), -1, dtype=np.int64)
    val = np.full((Nq, k), -np.inf, dtype=s.dtype)
    order = np.argsort(-s, axis=1, kind="stable")[:, :kk]
    idx[:, :kk] = order
    val[:, :kk] = np.take_along_axis(s, order, axis=1)
    return idx, val


def topk(Q, X, k):
    return topk_of_scores(scores(Q, X), k)


def topk_by_selection(Q, X, k):
    """The second definition: per row, pick again and again the maximum with the lowest index among what is left."""
    s = scores(Q, X)
    Nq, Nx = s.shape
    idx = np.full((Nq, k), -1, dtype=np.int64)
    val = np.full((Nq, k), -np.inf)
    for q in range(Nq):
        left = np.ones(Nx, dtype=bool)
        for p in range(min(k, Nx)):
            best = np.max(s[q, left])
            j = int(np.nonzero(left & (s[q] == best))[0][0])
            idx[q, p], val[q, p], left[j] = j, best, False
    return idx, val


def _order_key(val):
    """fp32 -> the unsigned integers of the same order (the library's key): equal keys are equal bits"""
    u = np.ascontiguousarray(val, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(u >> 31, 0xFFFFFFFF - u, u | 0x80000000)


def determined(s64, k, b):
    """(Nq, min(k, Nx)) bool: the yardstick entries that lie farther than 2 b from both neighbours in their row's full fp64
    order.  A computation with an error of at most b per score must return the yardstick's index there."""
    Nq, Nx = s64.shape
    kk = min(k, Nx)
    v = -np.sort(-s64, axis=1)
    gap = v[:, :-1] - v[:, 1:]                     # gap[p]: between places p and p + 1
    wide = np.concatenate([np.ones((Nq, 1), bool), gap > 2 * b, np.ones((Nq, 1), bool)], axis=1)
    return (wide[:, :-1] & wide[:, 1:])[:, :kk]


def topk_valid(s64, idx, val, k, b):
    """What a top-k computed with an absolute error of at most b per score may return, against the fp64 scores s64 (Nq, Nx).
    -> (the list of violations, empty where the result is admissible; the share of (row, place) entries that are determined).
    Per row: the padding is -1 / -inf; the indices are distinct and in range; |val[p] - s64[q, idx[p]]| <= b; the list is
    ordered by (score descending - fp32 results: by their bits - and index ascending); every index not returned has
    s64 <= val[k - 1] + b; a determined entry holds the yardstick's index."""
    idx, val = np.asarray(idx), np.asarray(val)
    Nq, Nx = s64.shape
    kk = min(k, Nx)
    bad = []
    if idx.shape != (Nq, k) or val.shape != (Nq, k):
        return [f"shapes {idx.shape}, {val.shape} for {(Nq, k)}"], 0.0
    if kk < k and not ((idx[:, kk:] == -1).all() and np.isneginf(val[:, kk:]).all()):
        bad.append("padding: not idx = -1, val = -inf")
    det = determined(s64, k, b)
    if kk == 0:
        return bad, 1.0
    ii, vv = idx[:, :kk].astype(np.int64), val[:, :kk]
    if (ii < 0).any() or (ii >= Nx).any():
        return bad + ["an index out of range"], float(det.mean())
    srt = np.sort(ii, axis=1)
    if (srt[:, 1:] == srt[:, :-1]).any():
        bad.append(f"a duplicated index, first in row {int(np.nonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))[0][0])}")
    err = np.abs(vv.astype(np.float64) - np.take_along_axis(s64, ii, axis=1))
    if (err > b).any():
        bad.append(f"a score off by {err.max():.3e} > {b:.3e}")
    key = _order_key(vv) if vv.dtype == np.float32 else vv
    ordered = (key[:, :-1] > key[:, 1:]) | ((key[:, :-1] == key[:, 1:]) & (ii[:, :-1] < ii[:, 1:]))
    if not ordered.all():
        bad.append(f"order: row {int(np.nonzero(~ordered.all(axis=1))[0][0])} is not (score descending, index ascending)")
    rest = s64.copy()
    np.put_along_axis(rest, ii, -np.inf, axis=1)
    over = rest.max(axis=1) > vv[:, -1].astype(np.float64) + b
    if over.any():
        bad.append(f"row {int(np.nonzero(over)[0][0])}: an index not returned scores above the last one returned + b")
    want, _ = topk_of_scores(s64, k)
    wrong = det & (ii != want[:, :kk])
    if wrong.any():
        q, p = (int(x[0]) for x in np.nonzero(wrong))
        bad.append(f"row {q} place {p}: index {int(ii[q, p])}, the yardstick's {int(want[q, p])} is determined")
    return bad, float(det.mean())
