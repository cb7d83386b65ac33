"""Torch-CPU statement of the zero-shot segmentation evaluation, written from its description.

mmseg and mmcv are not part of the reference tree: rescaling the logits to the ground truth's size followed by the arg-max,
intersect_and_union, eval_metrics and mmcv's rescale_size are UNPINNED third-party behaviour restated here (as
tests/seg_reference.py says of the slide assembly).  The reference-pinned part, encode_decode's logits, stays pinned by
tests/golden/seg_tiny.npz.  mmseg takes a softmax between the resize and the arg-max; the arg-max of the logits is the same
except where fp32 exp rounds two different logits to one value, which is not emulated.

  rescale_labels : bilinear (align_corners=False) resize of (..., C, H, W) logits, first maximum over C, top-two gap
  areas          : per class intersection / prediction area / label area with ignore_index and reduce_zero_label
  metrics        : mIoU, aAcc, mAcc, IoU, Acc from the areas (nanmean: a class absent from both is left out)
  spread         : which output pixels have one of their (up to four) source taps in a mask

Everything takes a dtype (float64 = the yardstick).
"""
import torch

from tests import seg_reference as sr


def rescale_labels(logits, oh, ow, dtype=torch.float64):
    """logits (..., C, H, W) -> labels (..., oh, ow) long, gap (..., oh, ow) = top value - second value."""
    up = sr.upsample(logits, oh, ow, dtype)
    labels = up.argmax(dim=-3)
    if up.shape[-3] > 1:
        top2 = up.topk(2, dim=-3).values
        gap = top2.select(-3, 0) - top2.select(-3, 1)
    else:
        gap = torch.full(labels.shape, float("inf"), dtype=dtype)
    return labels, gap


def spread(mask, oh, ow):
    """mask (..., H, W) bool -> (..., oh, ow): true where one of the pixel's bilinear taps is true in mask."""
    y0, y1, _ = sr._taps(oh, mask.shape[-2], torch.float64)
    x0, x1, _ = sr._taps(ow, mask.shape[-1], torch.float64)
    rows0, rows1 = mask[..., y0, :], mask[..., y1, :]
    return rows0[..., x0] | rows0[..., x1] | rows1[..., x0] | rows1[..., x1]


def areas(pred, gt, C, ignore=255, reduce_zero=False):
    """-> (3, C) long: intersection, prediction area, label area.  The ignore value (and 0 with reduce_zero, every other
    value then counting as g - 1) contributes nothing; g >= C counts in the prediction area only (histc drops it)."""
    p, g = pred.reshape(-1).long(), gt.reshape(-1).long()
    keep = g != ignore
    if reduce_zero:
        keep &= g != 0
        g = g - 1
    p, g = p[keep], g[keep]

    def hist(v):
        return torch.bincount(v[(v >= 0) & (v < C)], minlength=C)
    return torch.stack([hist(p[p == g]), hist(p), hist(g)])


def metrics(a, dtype=torch.float64):
    a = a.to(dtype)
    inter, pred, label = a[0], a[1], a[2]
    iou, acc = inter / (pred + label - inter), inter / label
    return dict(mIoU=float(torch.nanmean(iou)), aAcc=float(inter.sum() / label.sum()), mAcc=float(torch.nanmean(acc)),
                IoU=iou, Acc=acc)
