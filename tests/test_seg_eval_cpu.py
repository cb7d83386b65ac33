"""CPU: the pure-Python parts of the zero-shot segmentation evaluation (segclip_amd.segmentation.test_size, the window
planner, SegEvaluator.metrics_from_areas) and the yardstick of the GPU tests (tests/seg_eval_reference.py)."""
import math

import pytest
import torch

from segclip_amd.segmentation import SegEvaluator, _plan_windows, slide_windows, test_size
from tests import seg_eval_reference as ser


@pytest.mark.parametrize("hw,expect", [((375, 500), (224, 299)), ((500, 375), (299, 224)), ((281, 500), (224, 399)),
                                       ((300, 300), (224, 224)), ((100, 3000), (68, 2048))])
def test_test_size(hw, expect):
    """mmcv's keep-ratio rule at img_scale (2048, 224); the last image is bound by the long side: 2048 / 3000."""
    assert test_size(*hw) == expect
    assert test_size(*hw, img_scale=(224, 2048)) == expect


def test_metrics_from_areas_hand_worked():
    """3 classes, class 2 absent from prediction and label.  IoU = 2/(4+3-2), 3/(4+5-3), NaN; Acc = 2/3, 3/5, NaN."""
    a = torch.tensor([[2, 3, 0], [4, 4, 0], [3, 5, 0]])
    for m in (SegEvaluator.metrics_from_areas(a), ser.metrics(a)):
        assert m["IoU"][0] == pytest.approx(0.4) and m["IoU"][1] == pytest.approx(0.5) and math.isnan(float(m["IoU"][2]))
        assert m["mIoU"] == pytest.approx(0.45)
        assert m["Acc"][0] == pytest.approx(2 / 3) and m["Acc"][1] == pytest.approx(0.6) and math.isnan(float(m["Acc"][2]))
        assert m["mAcc"] == pytest.approx((2 / 3 + 0.6) / 2)
        assert m["aAcc"] == pytest.approx(5 / 8)


def test_metrics_with_reduce_zero_label():
    """gt 0 is dropped and 1, 2, 3 count as 0, 1, 2.  Predictions 0 1 2 2 against 1 2 2 0 -> the last pixel is ignored:
    I = (1, 1, 0), P = (1, 1, 1), L = (1, 2, 0) -> IoU = 1, 1/2, 0/1."""
    pred, gt = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 2, 2, 0])
    a = ser.areas(pred, gt, 3, 255, True)
    assert a.tolist() == [[1, 1, 0], [1, 1, 1], [1, 2, 0]]
    m = SegEvaluator.metrics_from_areas(a)
    assert m["IoU"].tolist() == [1.0, 0.5, 0.0] and m["mIoU"] == pytest.approx(0.5) and m["aAcc"] == pytest.approx(2 / 3)


@pytest.mark.parametrize("reduce_zero", [False, True])
def test_reference_areas_against_a_python_loop(reduce_zero):
    C = 5
    g = torch.Generator().manual_seed(3)
    pred = torch.randint(0, C, (7, 9), generator=g)
    gt = torch.randint(0, C + 1, (7, 9), generator=g)   # C itself is a value >= C (and C - 1 after the shift)
    gt[2, 3], gt[5, 5], gt[0, 0] = 255, 255, 200
    want = [[0] * C for _ in range(3)]
    for p, t in zip(pred.reshape(-1).tolist(), gt.reshape(-1).tolist()):
        if t == 255 or (reduce_zero and t == 0):
            continue
        t = t - 1 if reduce_zero else t
        want[1][p] += 1
        if t < C:
            want[2][t] += 1
            if p == t:
                want[0][p] += 1
    assert ser.areas(pred, gt, C, 255, reduce_zero).tolist() == want
    assert sum(want[1]) == 7 * 9 - 2 - (int((gt == 0).sum()) if reduce_zero else 0)


# ------------------------------------------------------------------------------------------------ the window planner
SLIDE = dict(crop_size=(64, 64), stride=(48, 40))


def test_plan_whole_mode_batches_by_size_in_first_seen_order():
    plan = _plan_windows("whole", (224, 224), (224, 224), [(128, 128), (256, 64), (128, 128)])
    assert plan.batches == [((128, 128), [(0, 0, 0), (2, 0, 0)]), ((256, 64), [(1, 0, 0)])]
    # an entry's first window is its place in the tower order; one window each, of the entry's own size
    assert plan.entries == [(0, 1, (128, 128)), (2, 1, (256, 64)), (1, 1, (128, 128))]
    assert plan.image_windows == [1, 1, 1]


def test_plan_slide_mode_is_one_batch_of_every_entrys_grid():
    sizes = [(100, 150), (64, 64)]
    plan = _plan_windows("slide", sizes=sizes, **SLIDE)
    assert len(plan.batches) == 1 and plan.batches[0][0] == (64, 64)
    wins, first = plan.batches[0][1], 0
    for e, (H, W) in enumerate(sizes):
        grid = slide_windows(H, W, SLIDE["crop_size"], SLIDE["stride"])
        assert plan.entries[e] == (first, len(grid), (64, 64))
        assert wins[first:first + len(grid)] == [(e, y, x) for (y, x) in grid]
        first += len(grid)
    assert first == len(wins) and plan.image_windows == [8, 1]


def test_plan_sums_an_images_windows_over_its_views():
    sizes = [(100, 150), (64, 64), (64, 100)]   # image 0: two views, image 1: one
    plan = _plan_windows("slide", sizes=sizes, view_counts=[2, 1], **SLIDE)
    per = [len(slide_windows(H, W, SLIDE["crop_size"], SLIDE["stride"])) for (H, W) in sizes]
    assert [count for _, count, _ in plan.entries] == per
    assert plan.image_windows == [per[0] + per[1], per[2]] == [9, 2]
    assert _plan_windows("whole", None, None, sizes, [2, 1]).image_windows == [2, 1]


def test_plan_names_image_and_view_of_a_bad_entry():
    with pytest.raises(ValueError, match="image 1 view 1.*smaller than the crop"):
        _plan_windows("slide", sizes=[(64, 64), (64, 64), (60, 64)], view_counts=[1, 2], **SLIDE)
    with pytest.raises(ValueError, match="image 0 view 0.*smaller than the crop"):
        _plan_windows("slide", sizes=[(64, 63)], **SLIDE)
    # (64 + 8 * 8) / 8 -> a 9 x 9 grid of 81 windows for one entry
    with pytest.raises(ValueError, match="image 1 view 0.*81 windows, at most 64"):
        _plan_windows("slide", (64, 64), (8, 8), [(64, 64), (128, 128)])
    with pytest.raises(ValueError, match="image 0 view 2.*81 windows, at most 64"):
        _plan_windows("slide", (64, 64), (8, 8), [(64, 64), (64, 64), (128, 128)], [3])
    # 8 views of 9 windows: every view within the limit, the image over it
    with pytest.raises(ValueError, match="image 1: 72 windows over its 8 views, at most 64"):
        _plan_windows("slide", (64, 64), (32, 32), [(64, 64)] + [(128, 128)] * 8, [1, 8])
    with pytest.raises(ValueError, match="image 0: 17 views"):
        _plan_windows("whole", None, None, [(64, 64)] * 17, [17])
