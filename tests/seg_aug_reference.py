"""Torch-CPU statement of mmseg's aug_test for flip and multi-scale views, written from its description (mmseg is not part of
the reference tree: UNPINNED third-party behaviour restated here, as tests/seg_eval_reference.py says of the rescaling).

  every view is segmented -> its logits are resized to the output size (bilinear, align_corners=False) -> soft-max over the
  classes (subtract the maximum, exp, divide by the sum) -> flipped back -> the probabilities are summed in view order and
  divided by the view count -> first maximum.

The per-view logits come from tests/seg_reference.py (assemble), the resize from its upsample.  The flipped front end
(MultiScaleFlipAug flips AFTER the resize) is tests/seg_frontend_reference.py's resized image, mirrored.

Everything takes a dtype (float64 = the yardstick, float32 = the same operation order in fp32, for the tolerance)."""
import torch

from tests import seg_eval_reference as ser
from tests import seg_frontend_reference as sfr
from tests import seg_reference as sr

FLIP_H, FLIP_V = 1, 2


def flip_back(x, flags):
    """Mirror the last two axes (rows with FLIP_V, columns with FLIP_H)."""
    dims = [d for d, bit in ((-1, FLIP_H), (-2, FLIP_V)) if flags & bit]
    return x.flip(dims) if dims else x


def softmax(x, dim):
    e = (x - x.amax(dim=dim, keepdim=True)).exp()
    return e / e.sum(dim=dim, keepdim=True)


def mean_probs(view_logits, flags, oh, ow, dtype=torch.float64):
    """view_logits [(C, H_v, W_v)], flags [int] -> (C, oh, ow): the mean over the views, summed in view order."""
    total = None
    for lg, f in zip(view_logits, flags):
        p = flip_back(softmax(sr.upsample(lg, oh, ow, dtype), 0), f)
        total = p if total is None else total + p
    return total / torch.tensor(float(len(view_logits)), dtype=dtype)


def labels_and_gap(mean):
    """(C, oh, ow) -> first maximum (oh, ow) long, top value - second value."""
    labels = mean.argmax(dim=0)
    if mean.shape[0] > 1:
        top2 = mean.topk(2, dim=0).values
        return labels, top2[0] - top2[1]
    return labels, torch.full(labels.shape, float("inf"), dtype=mean.dtype)


def spread_view(mask, oh, ow, flags):
    """A view's source mask (H, W) -> the output pixels (oh, ow) that read one of its true pixels."""
    return flip_back(ser.spread(mask, oh, ow), flags)


def view_input(raw, net, mean, inv_std, flags, reverse_channels=False):
    """The network input of one view: the image resized to `net` and normalised, then mirrored -> (3, H, W) fp64."""
    return flip_back(sfr.resize_normalise(raw, net, mean, inv_std, reverse_channels), flags)
