"""numpy restatement of the confusion matrix of label maps (include/segclip_hip.h, segclip_seg_confusion) and of what
SegEvaluator derives from it: the masking rule pixel by pixel, np.add.at into (C + 1, C + 1), the metric formulae in fp64.
Importing this module needs numpy only."""
import numpy as np


def confusion(pred, gt, C, ignore_index=255, reduce_zero=False):
    """pred, gt: integer arrays of one size holding the UNSIGNED values -> (C + 1, C + 1) int64, row = ground truth, column =
    prediction, index C the out-of-range bin."""
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    keep = g != ignore_index
    if reduce_zero:
        keep &= g != 0
        g = g - 1
    row, col = np.minimum(g[keep], C), np.minimum(p[keep], C)
    out = np.zeros((C + 1, C + 1), np.int64)
    np.add.at(out, (row, col), 1)
    return out


def areas_from_confusion(conf):
    """-> (3, C) int64: intersection, prediction area, label area (mmseg's intersect_and_union of the same pixels)"""
    conf = np.asarray(conf, np.int64)
    C = conf.shape[0] - 1
    return np.stack([np.diagonal(conf)[:C], conf.sum(0)[:C], conf.sum(1)[:C]])


def areas(pred, gt, C, ignore_index=255, reduce_zero=False):
    """mmseg's intersect_and_union stated on its own, not through the matrix -> (3, C) int64"""
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    keep = g != ignore_index
    if reduce_zero:
        keep &= g != 0
        g = g - 1
    p, g = p[keep], g[keep]
    out = np.zeros((3, C), np.int64)
    for c in range(C):
        out[0, c] = np.count_nonzero((p == c) & (g == c))
        out[1, c] = np.count_nonzero(p == c)
        out[2, c] = np.count_nonzero(g == c)
    return out


def metrics(conf):
    """-> dict of fp64 figures; a class absent from prediction and label is NaN and left out of the means"""
    conf = np.asarray(conf, np.int64)
    inter, pred, label = areas_from_confusion(conf).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dice = 2.0 * inter / (pred + label)
        precision, recall = inter / pred, inter / label
        fscore = 2.0 * precision * recall / (precision + recall)
        iou = inter / (pred + label - inter)
        seen = label > 0
        fw = float((label[seen] * iou[seen]).sum() / label.sum())
        m = conf.astype(np.float64)
        total = m.sum()
        po = np.trace(m) / total
        pe = float((m.sum(1) * m.sum(0)).sum() / (total * total))
        kappa = float((po - pe) / (1.0 - pe))

        def mean(v):
            return float(v[~np.isnan(v)].mean()) if (~np.isnan(v)).any() else float("nan")
    return dict(Dice=dice, Precision=precision, Recall=recall, Fscore=fscore, mDice=mean(dice), mFscore=mean(fscore), fwIoU=fw,
                kappa=kappa)


def confused_pairs(conf, k):
    """-> [(gt, pred, count, share of the gt class's pixels)], the k largest non-empty off-diagonal cells of the first C rows
    and columns, by falling count and then rising (gt, pred)"""
    conf = np.asarray(conf, np.int64)
    C = conf.shape[0] - 1
    cells = [(int(conf[g, p]), g, p) for g in range(C) for p in range(C) if g != p and conf[g, p] > 0]
    cells.sort(key=lambda t: (-t[0], t[1], t[2]))
    return [(g, p, n, n / float(conf[g].sum())) for n, g, p in cells[:k]]


def merge_classes(conf, mapping):
    """-> (M + 1, M + 1) int64, the out-of-range bins carried over as bin M"""
    conf = np.asarray(conf, np.int64)
    C = conf.shape[0] - 1
    M = max(mapping) + 1
    to = list(mapping) + [M]
    out = np.zeros((M + 1, M + 1), np.int64)
    for g in range(C + 1):
        for p in range(C + 1):
            out[to[g], to[p]] += conf[g, p]
    return out


# ---------------------------------------------------------------- the maps of the GPU tests
def blocky_pair(rng, n, C):
    """A label map of about 8 x 8 constant blocks over 0 .. C - 1 as a flat array of n pixels, and a copy shifted by one row
    and one column as the ground truth: most pixels agree, the borders do not."""
    w = 64
    h = -(-n // w) + 8
    blocks = rng.integers(0, C, size=(h // 8 + 2, w // 8 + 2))
    full = np.kron(blocks, np.ones((8, 8), np.int64))
    pred = full[:h, :w].reshape(-1)[:n]
    gt = full[1:h + 1, 1:w + 1].reshape(-1)[:n]
    return pred.copy(), gt.copy()


def random_pair(rng, n, C, top):
    """Independent uniform labels over 0 .. min(C + 2, top): out-of-range values on both sides where the dtype has them."""
    hi = min(C + 2, top) + 1
    return rng.integers(0, hi, size=n), rng.integers(0, hi, size=n)
