"""CPU: the host side of the background-threshold sweep (segmentation.SegSweepEvaluator, check_thresholds) and the property the
sweep kernel's switch index rests on, restated with the fp32 reference of tests/seg_reference.py: over ascending thresholds a
pixel's label lies in {0, f} for one foreground label f, and the background set only grows."""
import math

import pytest
import torch

from segclip_amd import ops
from segclip_amd.segmentation import SegEvaluator, SegSweepEvaluator, check_thresholds
from tests import seg_eval_reference as ser
from tests import seg_reference as sr

THR = [0.0, 0.05, 0.2, 0.4, 0.6, 0.8, 0.95, 2.0]


# ------------------------------------------------------------------------------------------------ compute()'s reduction
def _areas(rows):
    """rows[t] = (intersection, prediction, label) per class -> (T, 3, C) long"""
    return torch.tensor(rows, dtype=torch.long)


def test_sweep_from_areas_by_hand():
    # three classes; class 2 is absent from prediction and label at every threshold: IoU 0 / 0 = NaN, left out of the mean
    areas = _areas([
        [[6, 2, 0], [10, 4, 0], [8, 6, 0]],    # IoU 6 / 12, 2 / 8  -> mIoU 0.375; aAcc 8 / 14
        [[8, 3, 0], [8, 6, 0], [8, 6, 0]],     # IoU 8 / 8, 3 / 9   -> mIoU 2 / 3
        [[4, 6, 0], [4, 10, 0], [8, 6, 0]],    # IoU 4 / 8, 6 / 10  -> mIoU 0.55
    ])
    out = SegSweepEvaluator.sweep_from_areas(areas, [0.1, 0.5, 0.9])
    assert out["thresholds"] == [0.1, 0.5, 0.9]
    assert [m["mIoU"] for m in out["metrics"]] == pytest.approx([0.375, 2.0 / 3.0, 0.55], abs=1e-15)
    assert out["metrics"][0]["aAcc"] == pytest.approx(8.0 / 14.0, abs=1e-15)
    assert out["metrics"][0]["mAcc"] == pytest.approx((6.0 / 8.0 + 2.0 / 6.0) / 2.0, abs=1e-15)
    assert all(math.isnan(float(m["IoU"][2])) for m in out["metrics"])
    assert out["best"] == (1, 0.5, pytest.approx(2.0 / 3.0, abs=1e-15))
    for t, m in enumerate(out["metrics"]):   # every slice is SegEvaluator's reduction of that slice
        one = SegEvaluator.metrics_from_areas(areas[t])
        assert m["mIoU"] == one["mIoU"] and torch.equal(m["IoU"].nan_to_num(-1.0), one["IoU"].nan_to_num(-1.0))


def test_best_takes_the_lowest_threshold_among_equal_miou():
    a = [[5, 5], [10, 10], [10, 10]]      # mIoU 1 / 3
    b = [[8, 8], [10, 10], [10, 10]]      # mIoU 2 / 3
    out = SegSweepEvaluator.sweep_from_areas(_areas([a, b, b, a]), [0.1, 0.2, 0.3, 0.4])
    assert out["best"][:2] == (1, 0.2)
    out = SegSweepEvaluator.sweep_from_areas(_areas([b, b]), [0.1, 0.2])
    assert out["best"][:2] == (0, 0.1)
    # a slice without any counted pixel has a NaN mIoU and never wins
    nan = [[0, 0], [0, 0], [0, 0]]
    out = SegSweepEvaluator.sweep_from_areas(_areas([nan, a, b]), [0.1, 0.2, 0.3])
    assert out["best"][:2] == (2, 0.3)
    out = SegSweepEvaluator.sweep_from_areas(_areas([nan, nan]), [0.1, 0.2])
    assert out["best"][:2] == (0, 0.1) and math.isnan(out["best"][2])
    with pytest.raises(ValueError, match="areas"):
        SegSweepEvaluator.sweep_from_areas(_areas([a, b]), [0.1])


# ------------------------------------------------------------------------------------------------ the threshold validation
def test_check_thresholds():
    assert check_thresholds([0.25]) == [0.25]
    assert check_thresholds((0.0, 0.5, 2)) == [0.0, 0.5, 2.0]
    got = check_thresholds([0.1, 0.8])     # the fp32 values the kernel compares
    assert got == torch.tensor([0.1, 0.8]).tolist()
    assert len(check_thresholds([i / 16 for i in range(ops.SEG_MAX_THRESHOLDS)])) == 16
    with pytest.raises(ValueError, match="thresholds.*empty"):
        check_thresholds([])
    with pytest.raises(ValueError, match="thresholds.*at most 16"):
        check_thresholds([i / 17 for i in range(17)])
    with pytest.raises(ValueError, match="thresholds.*sorted"):
        check_thresholds([0.5, 0.4])
    with pytest.raises(ValueError, match="thresholds.*duplicate"):
        check_thresholds([0.4, 0.4])
    with pytest.raises(ValueError, match="thresholds.*duplicate"):
        check_thresholds([0.4, 0.4 + 1e-12])   # one fp32 value
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="thresholds.*finite"):
            check_thresholds([0.1, bad])
    with pytest.raises(ValueError, match="thresholds"):
        check_thresholds(0.5)


class _NoBackground:
    with_bg = False


def test_evaluator_needs_the_background_class():
    with pytest.raises(ValueError, match="with_bg"):
        SegSweepEvaluator(_NoBackground(), [0.5])


# ------------------------------------------------------------------------------------------------ the switch-index property
def _small_case(mode, seed):
    """A small geometry with every kind of pixel: slide windows that overlap in x (224 x 300, stride 112: a pixel has 1, 2 or 3
    covering windows) or one whole window, rescaled by a ratio that is no integer."""
    G, N = 8, 6
    H, W = (224, 300) if mode == "slide" else (224, 224)
    wins, win = sr.window_list(1, H, W, mode, (224, 224), (112, 112))
    g = torch.Generator().manual_seed(seed)
    soft = torch.softmax(torch.randn(len(wins), G, 14, 14, generator=g) * 3.0, dim=1)
    table = torch.rand(len(wins), G, N, generator=g, dtype=torch.float64) * 0.1
    for k in range(len(wins)):
        for j in range(G):   # best scores spread over the thresholds
            table[k, j, (k * G + j) * 5 % N] = 0.02 + 0.96 * float(torch.rand((), generator=g))
    t = table.float()
    score, cls = t.max(dim=-1)
    t32 = dict(table=t, table_max=t.amax(dim=(1, 2)), best_class=cls, best_score=score)
    return dict(soft=soft, t32=t32, wins=wins, win=win, net=(H, W), out=(131, 173))


@pytest.mark.parametrize("mode,seed", [("slide", 31), ("whole", 32)])
def test_labels_switch_once_to_background(mode, seed):
    case = _small_case(mode, seed)
    (H, W), (oh, ow) = case["net"], case["out"]
    planes = []
    for thr in THR:
        ref = sr.assemble(case["soft"], case["t32"], case["wins"], (1, H, W), case["win"], True, thr, torch.float32)
        planes.append(ser.rescale_labels(ref["logits"], oh, ow, torch.float32)[0][0])
    planes = torch.stack(planes)                      # (T, oh, ow)
    fg = planes.amax(dim=0)                           # the one foreground label of a pixel, 0 where it has none
    assert bool(((planes == 0) | (planes == fg)).all()), "a pixel took two different foreground labels over the thresholds"
    bg = planes == 0
    assert bool((bg[1:] | ~bg[:-1]).all()), "a background pixel returned to the foreground at a higher threshold"
    changed = [int((planes[t] != planes[t + 1]).sum()) for t in range(len(THR) - 1)]
    assert sum(1 for c in changed if c) >= 3, f"the thresholds do not change the labels: {changed}"
    assert int(bg[0].sum()) < int(bg[-1].sum())
