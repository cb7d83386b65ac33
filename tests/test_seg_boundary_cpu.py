"""The restatement of the boundary bands and areas (tests/boundary_reference.py) checked on its own, without a GPU: against
scipy.ndimage.binary_erosion where it is installed, the two identities of the definition that the kernel tests then lean on,
the radius rule, the figures from a hand-made area tensor and the host-side refusals that need no device."""
import math

import numpy as np
import pytest
import torch

from segclip_amd import ops
from segclip_amd.segmentation import Boundary, SegEvaluator, boundary_areas, boundary_bands
from tests import boundary_reference as br

SH, TW = ops.SEG_BOUNDARY_TILE
CASES = br.cases(SH, TW)
ROWS = [(name, d) for name, (_, radii) in CASES.items() for d in radii]


def test_tile_and_cases():
    assert (SH, TW) == (32, 64) and ops.SEG_BOUNDARY_MAX_RADIUS == 128
    sizes = {k: m.shape for k, (m, _) in CASES.items()}
    assert sizes["1x1"] == (1, 1) and sizes["1x130"] == (1, 130) and sizes["130x1"] == (130, 1)
    assert sizes["constant_33x130"] == (33, 130) and CASES["constant_33x130"][1] == [1, 5, 16, 64]
    assert sizes["odd_pixel"] == (40, 150) and CASES["odd_pixel"][1] == [1, 7, 16]
    assert sizes["radius_100"] == (60, 260) and CASES["radius_100"][1] == [100] and CASES["radius_128"][1] == [128]
    for name in ("noise_3_labels", "blobs"):
        assert {0, 254, 255} <= set(np.unique(CASES[name][0]).tolist())
    maps, radii = br.mixed_call()
    assert [m.shape for m in maps] == [(1, 1), (17, 65), (50, 200), (96, 128)] and radii == [1, 2, 9, 3]


@pytest.mark.parametrize("name,d", ROWS)
def test_restatement_against_scipy(name, d):
    """band != 0 is, for every class at once, mask_to_boundary of Boundary IoU: the mask minus its d-fold 3 x 3 erosion with
    zeros outside the picture"""
    ndi = pytest.importorskip("scipy.ndimage")
    m = CASES[name][0]
    b = br.band(m, d)
    for k in np.unique(m).tolist():
        mask = m == k
        eroded = ndi.binary_erosion(mask, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
        assert np.array_equal(mask & ~eroded, mask & (b != 0)), (name, d, k)


def test_restatement_against_scipy_random_maps():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for _ in range(40):
        h, w, d = int(rng.integers(1, 21)), int(rng.integers(1, 31)), int(rng.integers(1, 17))
        m = br._blocks(rng, h, w, int(rng.integers(1, 5)), (0, 1, 255))
        b = br.band(m, d)
        for k in np.unique(m).tolist():
            eroded = ndi.binary_erosion(m == k, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
            assert np.array_equal((m == k) & ~eroded, (m == k) & (b != 0)), (h, w, d, k)


def test_what_the_cases_are_there_for():
    m, radii = CASES["constant_33x130"]
    for d in radii:
        b = br.band(m, d)
        assert not (b & 1).any()
        inner = np.zeros_like(b)
        inner[d:33 - d, d:130 - d] = 1 if d < 17 else 0
        assert np.array_equal(b == 0, inner.astype(bool))
    assert (br.band(m, 64) == 2).all()
    m, radii = CASES["odd_pixel"]
    (y,), (x,) = np.nonzero(m)
    for d in radii:
        square = np.zeros(m.shape, dtype=bool)
        square[max(0, y - d):y + d + 1, max(0, x - d):x + d + 1] = True
        assert np.array_equal((br.band(m, d) & 1).astype(bool), square)
    for d in (1, 2, 9):
        for name in (f"stripes_vertical_d{d}", f"stripes_horizontal_d{d}"):
            m = CASES[name][0]
            clear = (br.band(m, d) & 1) == 0
            assert not clear[m == 1].any() and clear[m == 2].any(), name
            # the narrow stripe lies across the chunk's (strip's) border
            along = m.any(axis=0) if "vertical" in name else m.any(axis=1)
            edge = TW if "vertical" in name else SH
            assert along[edge - 1] and along[edge]


def test_radius_rule():
    b = Boundary()
    assert [b.radius_of(h, w) for (h, w) in [(375, 500), (500, 500), (1024, 2048), (25, 25)]] == [12, 14, 46, 1]
    assert [br.radius(h, w) for (h, w) in [(375, 500), (500, 500), (1024, 2048), (25, 25)]] == [12, 14, 46, 1]
    assert Boundary(radius=7).radius_of(1000, 3) == 7 and Boundary(ratio=0.5, radius=128).radius_of(9, 9) == 128
    assert Boundary(ratio=0.02).radius_of(4500, 4500) == 127
    with pytest.raises(ValueError, match="image 3 of 5000x5000 has the radius 141"):
        Boundary().radius_of(5000, 5000, image=3)


@pytest.mark.parametrize("reduce_zero", [False, True])
@pytest.mark.parametrize("C", [1, 4, 256])
def test_identities(C, reduce_zero):
    rng = np.random.default_rng(C)
    pred, gt = br.area_pair(rng, 37, 70, (0, 1, 2, 3, 200))
    # a radius of at least the larger side: every window leaves the map, and slot 0 is the plain areas
    a = br.areas([pred], [gt], [70], C, 255, reduce_zero)
    assert np.array_equal(a[0], br.plain_areas(pred, gt, C, 255, reduce_zero))
    assert a[0].sum() > 0
    # a ground truth of one byte has no label change: the trimap is empty whatever the prediction
    flat = np.full_like(gt, 2)
    assert not br.areas([pred], [flat], [5], C, 255, reduce_zero)[1].any()
    # and in between the band restricts: no more than the plain areas, and something
    mid = br.areas([pred], [gt], [3], C, 255, reduce_zero)
    assert (mid <= br.plain_areas(pred, gt, C, 255, reduce_zero)[None]).all() and mid[1].sum() > 0


def test_metrics_from_a_hand_made_tensor():
    a = torch.tensor([[[6, 0, 2], [8, 0, 4], [10, 0, 2]],
                      [[3, 0, 0], [5, 0, 1], [4, 0, 0]]], dtype=torch.int64)
    m = SegEvaluator.boundary_metrics_from_areas(a)
    assert set(m) == {"bIoU", "mbIoU", "trimap_IoU", "trimap_mIoU", "trimap_aAcc"}
    assert m["bIoU"][0].item() == 6 / 12 and math.isnan(m["bIoU"][1].item()) and m["bIoU"][2].item() == 2 / 4
    assert m["mbIoU"] == (0.5 + 0.5) / 2
    assert m["trimap_IoU"][0].item() == 3 / 6 and math.isnan(m["trimap_IoU"][1].item()) and m["trimap_IoU"][2].item() == 0.0
    assert m["trimap_mIoU"] == 0.25 and m["trimap_aAcc"] == 3 / 4
    assert (m["mbIoU"], m["trimap_mIoU"]) == br.metrics(a.numpy())
    with pytest.raises(ValueError, match=r"\(2, 3, C\)"):
        SegEvaluator.boundary_metrics_from_areas(a[0])


def test_host_layer_refusals():
    for kw in (dict(ratio=0.0), dict(ratio=-1.0), dict(ratio=float("nan")), dict(ratio="a"), dict(radius=0), dict(radius=129),
               dict(radius=2.0), dict(radius=True)):
        with pytest.raises(ValueError, match="Boundary: (ratio|radius)"):
            Boundary(**kw)
    table = ops.seg_boundary_table
    t, n_blocks, side = table([(33, 130), (1, 1)], [0, 4292], [0, -1], [3, 1], "cpu")
    # 2 x 3 strips in 2 workgroups, then 1
    assert t.tolist() == [[33, 130, 0, 0, 3, 0, 0, 0], [1, 1, 4292, -1, 1, 2, 0, 0]] and (n_blocks, side) == (3, 130)
    assert table([(5, 5)], [0], None, [2], "cpu")[0][0, 3].item() == -1
    with pytest.raises(ValueError, match="sizes is empty"):
        table([], [], None, [], "cpu")
    with pytest.raises(ValueError, match="pred_offsets has 1 entries"):
        table([(5, 5), (6, 6)], [0], None, [1, 1], "cpu")
    with pytest.raises(ValueError, match="gt_offsets has 3 entries"):
        table([(5, 5), (6, 6)], [0, 28], [0, 25, 61], [1, 1], "cpu")
    with pytest.raises(ValueError, match="radii has 1 entries"):
        table([(5, 5), (6, 6)], [0, 28], None, [1], "cpu")
    with pytest.raises(ValueError, match="map 1 is 0x6"):
        table([(5, 5), (0, 6)], [0, 28], None, [1, 1], "cpu")
    with pytest.raises(ValueError, match="map 0 is 32768x1"):
        table([(32768, 1)], [0], None, [1], "cpu")
    for d in (0, 129):
        with pytest.raises(ValueError, match=rf"map 1 \(6x6\) has radius {d}"):
            table([(5, 5), (6, 6)], [0, 28], None, [1, d], "cpu")
    with pytest.raises(ValueError, match="pred_offsets are not negative"):
        table([(5, 5)], [-1], None, [1], "cpu")
    with pytest.raises(ValueError, match="gt_offsets are not negative"):
        table([(5, 5)], [0], [-2], [1], "cpu")
    with pytest.raises(ValueError, match="empty list of label maps"):
        boundary_bands([], Boundary())
    with pytest.raises(TypeError, match="boundary is a Boundary"):
        boundary_bands([torch.zeros(2, 2, dtype=torch.uint8)], 0.02)
    with pytest.raises(TypeError, match="boundary is a Boundary"):
        boundary_areas([torch.zeros(2, 2, dtype=torch.uint8)], [torch.zeros(2, 2, dtype=torch.uint8)], 2, None)
    with pytest.raises(TypeError, match="boundary is a Boundary"):
        SegEvaluator(None, boundary=0.02)
