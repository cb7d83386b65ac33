"""CPU: what the confusion matrix (csrc/segment_confusion.inc, SegEvaluator(confusion=True)) states without a device - the three
entries of the C ABI and their binding, and the static helpers of SegEvaluator on hand-made matrices against
tests/confusion_reference.py: integers exactly, fp64 figures within 1e-12 relative (the same integers go through the same
formulae; only the order of operations can differ)."""
import os

import numpy as np
import pytest
import torch

from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import SegEvaluator
from tests import confusion_reference as cr
from tests.helpers import header_declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


def test_header_declares_the_entries_and_lib_binds_them():
    narrow = header_declaration("segclip_seg_confusion")
    assert narrow == ["const uint8_t* pred", "const uint8_t* gt", "int64_t n", "int64_t C", "int ignore_index",
                      "int reduce_zero_label", "int64_t* conf", "void* stream"]
    wide = header_declaration("segclip_seg_confusion_wide")
    assert wide == ["const uint16_t* pred", "const uint16_t* gt"] + narrow[2:]
    assert narrow[:6] == header_declaration("segclip_seg_areas")[:6]
    route = header_declaration("segclip_seg_confusion_route")
    assert route == ["int64_t C", "int wide"]
    assert {"segclip_seg_confusion", "segclip_seg_confusion_wide", "segclip_seg_confusion_route"} <= set(L.SIGNATURES)   # types: test_abi.py
    assert os.path.exists(os.path.join(ROOT, "segclip_amd", "csrc", "segment_confusion.inc"))


def test_cpu_tensors_are_refused():
    lab = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_confusion(lab, lab, 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_confusion(lab.to(torch.int16), lab.to(torch.int16), 300)
    with pytest.raises(ValueError, match="uint8 or torch.int16"):
        ops.seg_confusion_route(21, torch.int32)


# ---------------------------------------------------------------- hand-made matrices
def _matrices():
    rng = np.random.default_rng(5)
    out = {}
    # three classes and the bins; class 2 is absent from both sides (row 2 and column 2 are empty)
    out["absent"] = np.array([[50, 7, 0, 2],
                              [7, 30, 0, 0],
                              [0, 0, 0, 0],
                              [4, 1, 0, 3]], np.int64)
    # class 1 is predicted but never labelled, class 2 labelled but never predicted: an undefined Fscore on one side only
    out["one_sided"] = np.array([[10, 3, 0, 0],
                                 [0, 0, 0, 0],
                                 [5, 2, 0, 1],
                                 [0, 0, 0, 0]], np.int64)
    # equal off-diagonal counts: the order of confused_pairs falls back to (gt, pred)
    out["ties"] = np.array([[9, 4, 4, 1],
                            [4, 9, 2, 0],
                            [2, 4, 9, 5],
                            [8, 8, 8, 8]], np.int64)
    out["one_class"] = np.array([[5, 2], [3, 1]], np.int64)
    out["random21"] = rng.integers(0, 1000, size=(22, 22))
    out["wide300"] = rng.integers(0, 3, size=(301, 301)) * rng.integers(0, 2 ** 33, size=(301, 301))   # counts past 32 bits
    return out


MATRICES = _matrices()


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern"
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok])), f"{what}: {got} != {want}"


@pytest.mark.parametrize("name", list(MATRICES))
def test_areas_and_metrics(name):
    m = MATRICES[name]
    conf = torch.from_numpy(m)
    areas = SegEvaluator.areas_from_confusion(conf)
    assert areas.dtype == torch.int64 and np.array_equal(areas.numpy(), cr.areas_from_confusion(m))
    assert np.array_equal(SegEvaluator.areas_from_confusion(conf.to(torch.int32) if m.max() < 2 ** 31 else conf).numpy(),
                          cr.areas_from_confusion(m))
    got, want = SegEvaluator.confusion_metrics(conf), cr.metrics(m)
    assert set(got) == set(want) | {"confusion"}
    assert got["confusion"].dtype == torch.int64 and torch.equal(got["confusion"], conf)
    for key in ("Dice", "Precision", "Recall", "Fscore"):
        assert got[key].dtype == torch.float64
        _close(got[key].numpy(), want[key], f"{name} {key}")
    for key in ("mDice", "mFscore", "fwIoU", "kappa"):
        assert isinstance(got[key], float)
        _close(got[key], want[key], f"{name} {key}")


def test_absent_class_is_nan_and_left_out_of_the_means():
    got = SegEvaluator.confusion_metrics(torch.from_numpy(MATRICES["absent"]))
    for key in ("Dice", "Precision", "Recall", "Fscore"):
        assert torch.isnan(got[key][2]) and not torch.isnan(got[key][:2]).any(), key
    # by hand: I = (50, 30), P = (61, 38), L = (59, 37)
    assert got["mDice"] == pytest.approx((100 / 120 + 60 / 75) / 2, rel=RTOL)
    assert got["mFscore"] == pytest.approx(got["mDice"], rel=1e-12)   # F1 is Dice where both are defined
    iou = np.array([50 / 70, 30 / 45])
    assert got["fwIoU"] == pytest.approx((59 * iou[0] + 37 * iou[1]) / 96, rel=RTOL)
    one = SegEvaluator.confusion_metrics(torch.from_numpy(MATRICES["one_sided"]))
    assert torch.isnan(one["Fscore"][1]) and torch.isnan(one["Fscore"][2]) and float(one["Dice"][1]) == 0.0
    assert one["mFscore"] == pytest.approx(float(one["Fscore"][0]), rel=RTOL)
    assert one["mDice"] == pytest.approx(float(one["Dice"][0]) / 3, rel=RTOL)
    # a perfect prediction: kappa 1
    assert SegEvaluator.confusion_metrics(torch.diag(torch.tensor([4, 5, 6, 0])))["kappa"] == 1.0


@pytest.mark.parametrize("name", list(MATRICES))
def test_confused_pairs(name):
    m = MATRICES[name]
    conf = torch.from_numpy(m)
    C = m.shape[0] - 1
    for k in (0, 1, 3, 10, C * C + 5):
        got, want = SegEvaluator.confused_pairs(conf, k), cr.confused_pairs(m, k)
        assert [t[:3] for t in got] == [t[:3] for t in want], (name, k)
        _close([t[3] for t in got], [t[3] for t in want], f"{name} share")
        assert len(got) <= k


def test_confused_pairs_ties_and_names():
    conf = torch.from_numpy(MATRICES["ties"])
    got = SegEvaluator.confused_pairs(conf, 5)
    # the bins (row 3, column 3) hold the largest cells and are left out; the four 4s come in (gt, pred) order
    assert [t[:3] for t in got] == [(0, 1, 4), (0, 2, 4), (1, 0, 4), (2, 1, 4), (1, 2, 2)]
    assert got[0][3] == 4 / 18 and got[3][3] == 4 / 20
    named = SegEvaluator.confused_pairs(conf, 2, names=["sofa", "chair", "table"])
    assert [t[:3] for t in named] == [("sofa", "chair", 4), ("sofa", "table", 4)]
    with pytest.raises(ValueError, match="names"):
        SegEvaluator.confused_pairs(conf, 2, names=["sofa"])
    assert SegEvaluator.confused_pairs(torch.from_numpy(MATRICES["one_class"]), 4) == []


def test_merge_classes():
    for name, m in MATRICES.items():
        C = m.shape[0] - 1
        conf = torch.from_numpy(m)
        mappings = [list(range(C)), [0] * C, [c % 2 for c in range(C)] if C > 1 else [0], [C - 1 - c for c in range(C)]]
        for mapping in mappings:
            got = SegEvaluator.merge_classes(conf, mapping)
            want = cr.merge_classes(m, mapping)
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want), (name, mapping[:4])
            assert int(got.sum()) == int(m.sum())
    m = MATRICES["ties"]
    conf = torch.from_numpy(m)
    assert torch.equal(SegEvaluator.merge_classes(conf, [0, 1, 2]), conf)
    # everything into one class: the inner block, the two borders and the corner
    one = SegEvaluator.merge_classes(conf, [0, 0, 0])
    assert one.tolist() == [[int(m[:3, :3].sum()), int(m[:3, 3].sum())], [int(m[3, :3].sum()), int(m[3, 3])]]
    # two synonyms as one class: the score after merging, without a second run
    two = SegEvaluator.merge_classes(conf, [0, 0, 1])
    assert two.tolist() == [[9 + 4 + 4 + 9, 4 + 2, 1], [2 + 4, 9, 5], [16, 8, 8]]
    merged = SegEvaluator.metrics_from_areas(SegEvaluator.areas_from_confusion(two))
    assert merged["IoU"][0] == pytest.approx(26 / (26 + 6 + 1 + 6 + 16), rel=RTOL)
    for bad in ([0, 1], [0, 2, 2], [0, -1, 1], [1, 1, 1]):
        with pytest.raises(ValueError, match="mapping"):
            SegEvaluator.merge_classes(conf, bad)


def test_helpers_refuse_what_is_no_matrix():
    for fn in (SegEvaluator.areas_from_confusion, SegEvaluator.confusion_metrics):
        with pytest.raises(ValueError, match="integer tensor"):
            fn(torch.zeros(3, 4, dtype=torch.int64))
        with pytest.raises(ValueError, match="integer tensor"):
            fn(torch.zeros(3, 3))


def test_reference_matrix_projects_onto_the_areas():
    """The reference's own identity: the areas through the matrix are intersect_and_union stated directly."""
    rng = np.random.default_rng(8)
    for C, ignore, rz in ((5, 255, False), (5, 3, True), (21, 255, True), (1, 0, False)):
        pred, gt = cr.random_pair(rng, 4000, C, 255)
        m = cr.confusion(pred, gt, C, ignore, rz)
        assert np.array_equal(cr.areas_from_confusion(m), cr.areas(pred, gt, C, ignore, rz))
        kept = np.count_nonzero((gt != ignore) & ((gt != 0) | (not rz)))
        assert int(m.sum()) == kept
