"""Restatement of the per-image areas of label maps (include/segclip_hip.h, segclip_seg_image_areas) and of what SegEvaluator
derives from them.  The areas are tests/confusion_reference.areas, picture by picture; the fine-grained figures, worst_images
and the bootstrap are explicit Python loops in fp64 (the bootstrap over the same torch.randint draws).  Importing this module
needs numpy and torch only."""
import math

import numpy as np
import torch

from tests import confusion_reference as cr

NAN = float("nan")


def image_areas(preds, gts, C, ignore_index=255, reduce_zero=False):
    """preds, gts: lists of integer arrays holding the UNSIGNED values -> (B, 3, C) int64"""
    return np.stack([cr.areas(p, g, C, ignore_index, reduce_zero) for p, g in zip(preds, gts)]) if len(preds) else \
        np.zeros((0, 3, C), np.int64)


def _mean(values):
    values = [v for v in values if not math.isnan(v)]
    return math.fsum(values) / len(values) if values else NAN


def _lowest_mean(values, q):
    values = sorted(v for v in values if not math.isnan(v))
    if not values:
        return NAN
    k = max(1, math.ceil(q * len(values)))
    return math.fsum(values[:k]) / k


def _iou(a):
    """(n, 3, C) integers -> iou[i][c], NaN where the union is empty"""
    a = np.asarray(a, np.int64)
    n, _, C = a.shape
    out = []
    for i in range(n):
        row = []
        for c in range(C):
            inter, pred, label = int(a[i, 0, c]), int(a[i, 1, c]), int(a[i, 2, c])
            union = pred + label - inter
            row.append(inter / union if union > 0 else NAN)
        out.append(row)
    return out


def fine_grained(a, quantiles=(0.05, 0.1)):
    a = np.asarray(a, np.int64)
    n, _, C = a.shape
    iou = _iou(a)
    image_miou = [_mean(iou[i]) for i in range(n)]
    in_class = [[iou[i][c] for i in range(n) if a[i, 2, c] > 0] for c in range(C)]
    iou_c = [_mean(v) for v in in_class]
    return dict(image_mIoU=np.array(image_miou, np.float64), mIoU_I=_mean(image_miou), IoU_C=np.array(iou_c, np.float64),
                mIoU_C=_mean(iou_c), mIoU_I_q={float(q): _lowest_mean(image_miou, q) for q in quantiles},
                mIoU_C_q={float(q): _mean([_lowest_mean(v, q) for v in in_class]) for q in quantiles})


def worst_images(a, k):
    scores = fine_grained(a, ())["image_mIoU"].tolist()
    ranked = sorted(((s, i) for i, s in enumerate(scores) if not math.isnan(s)), key=lambda t: (t[0], t[1]))
    return [(i, s) for s, i in ranked[:k]]


def miou(areas):
    """(3, C) numbers -> the data-set mIoU: the mean of I / (P + L - I) over the classes present on either side"""
    inter, pred, label = [[float(v) for v in row] for row in np.asarray(areas)]
    return _mean([i / (p + lab - i) if p + lab - i > 0 else NAN for i, p, lab in zip(inter, pred, label)])


def bootstrap(a, n_boot=1000, alpha=0.05, seed=0):
    a = np.asarray(a, np.int64)
    n = a.shape[0]
    idx = torch.randint(0, n, (n_boot, n), generator=torch.Generator().manual_seed(seed)).numpy()
    reps = []
    for r in range(n_boot):
        total = np.zeros(a.shape[1:], np.int64)
        for i in idx[r]:
            total += a[i]
        reps.append(miou(total))
    ordered = sorted(v for v in reps if not math.isnan(v))   # a replicate of all-ignored pictures has no mIoU and is left out
    m = len(ordered)
    if m == 0:
        return dict(lo=NAN, hi=NAN, std=NAN, replicates=np.array(reps, np.float64))

    def quantile(q):   # linear interpolation between the order statistics, torch.quantile's default
        pos = q * (m - 1)
        lo = int(math.floor(pos))
        hi = min(lo + 1, m - 1)
        return ordered[lo] + (ordered[hi] - ordered[lo]) * (pos - lo)

    mean = math.fsum(ordered) / m
    std = math.sqrt(math.fsum((v - mean) ** 2 for v in ordered) / (m - 1)) if m > 1 else 0.0
    return dict(lo=quantile(alpha / 2.0), hi=quantile(1.0 - alpha / 2.0), std=std, replicates=np.array(reps, np.float64))
