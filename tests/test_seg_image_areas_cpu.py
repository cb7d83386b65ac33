"""CPU: what the per-image areas (csrc/segment_image_areas.inc, SegEvaluator(per_image=True)) state without a device - the two
entries of the C ABI and their binding, the table builder, and the static reductions of SegEvaluator on hand-made (n, 3, C)
tensors against tests/image_areas_reference.py: fp64 figures within 1e-12 relative (sums of at most a few thousand values in
[0, 1], error <= n * 2^-53; only the order of operations can differ)."""
import math
import os
import types

import numpy as np
import pytest
import torch

from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import SegEvaluator, image_areas
from tests import image_areas_reference as ir
from tests.helpers import header_declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12
fine = SegEvaluator.fine_grained_from_image_areas


def test_header_declares_the_entries_and_lib_binds_them():
    narrow = header_declaration("segclip_seg_image_areas")
    assert narrow == ["const uint8_t* pred", "int64_t pred_elems", "const uint8_t* gt", "int64_t gt_elems", "const int64_t* images",
                      "int64_t B", "int64_t n_blocks", "int64_t C", "int ignore_index", "int reduce_zero_label", "int64_t* out",
                      "void* stream"]
    wide = header_declaration("segclip_seg_image_areas_wide")
    assert wide == ["const uint16_t* pred", narrow[1], "const uint16_t* gt"] + narrow[3:]
    assert {"segclip_seg_image_areas", "segclip_seg_image_areas_wide"} <= set(L.SIGNATURES)   # types: test_abi.py
    assert L.const("SEG_IA_COLS") == 4 == ops.SEG_IA_COLS and L.const("SEG_IA_TILE") == ops.SEG_IA_TILE >= 4096
    assert os.path.exists(os.path.join(ROOT, "segclip_amd", "csrc", "segment_image_areas.inc"))


def test_table_builder():
    T = ops.SEG_IA_TILE
    table, n_blocks = ops.seg_image_areas_table([0, 8, 4 * T], [0, 5, 5 + T], [5, T, T + 1], "cpu")
    assert table.dtype == torch.int64 and table.tolist() == [[0, 0, 5, 0], [8, 5, T, 1], [4 * T, 5 + T, T + 1, 2]] and n_blocks == 4
    with pytest.raises(ValueError, match="counts is empty"):
        ops.seg_image_areas_table([], [], [], "cpu")
    with pytest.raises(ValueError, match="gt_offs has 1 entries"):
        ops.seg_image_areas_table([0, 1], [0], [1, 1], "cpu")
    with pytest.raises(ValueError, match="picture 1 has 0"):
        ops.seg_image_areas_table([0, 1], [0, 1], [1, 0], "cpu")
    with pytest.raises(ValueError, match=r"picture 0 has 2147483648"):
        ops.seg_image_areas_table([0], [0], [1 << 31], "cpu")
    with pytest.raises(ValueError, match="not negative"):
        ops.seg_image_areas_table([0, -4], [0, 1], [1, 1], "cpu")


def test_cpu_tensors_are_refused():
    lab = torch.zeros(64, dtype=torch.uint8)
    table, n_blocks = ops.seg_image_areas_table([0], [0], [64], "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_image_areas(lab, lab, table, n_blocks, 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_image_areas(lab.to(torch.int16), lab.to(torch.int16), table, n_blocks, 300)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_areas([lab.view(8, 8)], [lab.view(8, 8)], 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_areas([lab.view(8, 8).to(torch.int16)], [lab.view(8, 8).to(torch.int16)], 300)


def test_an_evaluator_starts_without_rows():
    seg = types.SimpleNamespace(label_dtype=torch.uint8, num_classes=21, text_embedding=torch.zeros(1))
    ev = SegEvaluator(seg, per_image=True)
    assert tuple(ev.image_areas.shape) == (0, 3, 21) and ev.image_areas.dtype == torch.int64
    ev.reset()
    assert tuple(ev.image_areas.shape) == (0, 3, 21)
    assert SegEvaluator(seg).image_areas is None
    wide = types.SimpleNamespace(label_dtype=torch.int16, num_classes=848, text_embedding=torch.zeros(1))
    assert tuple(SegEvaluator(wide, ignore_index=65535, per_image=True).image_areas.shape) == (0, 3, 848)


# ---------------------------------------------------------------- hand-made areas
def _row(C, cells):
    """{class: (I, P, L)} -> (3, C)"""
    a = np.zeros((3, C), np.int64)
    for c, ipl in cells.items():
        a[:, c] = ipl
    return a


def _tensors():
    rng = np.random.default_rng(9)
    out = {}
    # picture 1 is all ignored (a row of zeros); class 2 is predicted in picture 0 but labelled nowhere; class 3 is absent
    out["ignored_and_unlabelled"] = np.stack([_row(4, {0: (40, 50, 45), 1: (10, 30, 25), 2: (0, 12, 0)}),
                                              _row(4, {}),
                                              _row(4, {0: (5, 5, 60), 1: (60, 115, 60)}),
                                              _row(4, {0: (7, 7, 7)})])
    out["one_picture"] = np.stack([_row(3, {0: (3, 4, 9), 2: (1, 8, 2)})])
    out["one_class"] = np.stack([_row(1, {0: (k, k + 2, 2 * k + 1)}) for k in range(6)])
    # equal scores: pictures 0, 2 and 3 score 0.5, picture 1 scores 0.25
    out["ties"] = np.stack([_row(2, {0: (1, 2, 1)}), _row(2, {1: (1, 4, 1)}), _row(2, {0: (2, 2, 4)}), _row(2, {1: (3, 6, 3)})])
    out["all_ignored"] = np.zeros((3, 3, 5), np.int64)
    inter = rng.integers(0, 500, size=(40, 21))
    out["random21"] = np.stack([inter, inter + rng.integers(0, 300, size=(40, 21)), inter + rng.integers(0, 300, size=(40, 21))], 1) \
        * (rng.random((40, 1, 21)) < 0.4)   # a picture holds some of the classes
    big = rng.integers(0, 2 ** 33, size=(7, 300))   # counts past 32 bits
    out["wide300"] = np.stack([big, big * 2, big + 5], 1)
    return out


TENSORS = _tensors()
QS = (0.05, 0.1, 0.26, 0.5, 1.0)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern {got} / {want}"
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok])), f"{what}: {got} != {want}"


def _check_fine(got, want, n, C, qs, what):
    assert list(got) == ["image_mIoU", "mIoU_I", "IoU_C", "mIoU_C", "mIoU_I_q", "mIoU_C_q"], what
    assert got["image_mIoU"].dtype == torch.float64 and tuple(got["image_mIoU"].shape) == (n,) and not got["image_mIoU"].is_cuda
    assert got["IoU_C"].dtype == torch.float64 and tuple(got["IoU_C"].shape) == (C,) and not got["IoU_C"].is_cuda
    _close(got["image_mIoU"].numpy(), want["image_mIoU"], f"{what} image_mIoU")
    _close(got["IoU_C"].numpy(), want["IoU_C"], f"{what} IoU_C")
    for key in ("mIoU_I", "mIoU_C"):
        assert isinstance(got[key], float)
        _close(got[key], want[key], f"{what} {key}")
    for key in ("mIoU_I_q", "mIoU_C_q"):
        assert list(got[key]) == [float(q) for q in qs], what
        for q in qs:
            _close(got[key][q], want[key][q], f"{what} {key}[{q}]")


@pytest.mark.parametrize("name", list(TENSORS))
def test_fine_grained_figures(name):
    a = TENSORS[name]
    n, _, C = a.shape
    for dtype in (torch.int64, torch.int32) if a.max() < 2 ** 31 else (torch.int64,):
        got = fine(torch.from_numpy(a).to(dtype), QS)
        _check_fine(got, ir.fine_grained(a, QS), n, C, QS, name)
    for key in ("mIoU_I", "mIoU_C"):   # q = 1 is the plain mean, bit for bit
        assert got[key + "_q"][1.0] == got[key] or (math.isnan(got[key]) and math.isnan(got[key + "_q"][1.0])), (name, key)
    default = fine(torch.from_numpy(a))
    assert list(default["mIoU_I_q"]) == [0.05, 0.1] == list(default["mIoU_C_q"])
    _close(default["mIoU_I_q"][0.1], got["mIoU_I_q"][0.1], f"{name}: the default quantiles")


def test_fine_grained_figures_written_down():
    got = fine(torch.from_numpy(TENSORS["ignored_and_unlabelled"]), (0.05, 0.5, 1.0))
    # picture 0: classes 0, 1 and the unlabelled class 2, which counts as 0; picture 1 has no score; picture 3 is perfect
    i0 = (40 / 55 + 10 / 45 + 0.0) / 3
    i2 = (5 / 60 + 60 / 115) / 2
    _close(got["image_mIoU"].numpy(), [i0, float("nan"), i2, 1.0], "image_mIoU")
    _close(got["mIoU_I"], (i0 + i2 + 1.0) / 3, "mIoU_I")
    # class 2 is labelled nowhere and class 3 is absent: NaN; class 0 over pictures 0, 2, 3, class 1 over pictures 0, 2
    c0, c1 = (40 / 55 + 5 / 60 + 1.0) / 3, (10 / 45 + 60 / 115) / 2
    _close(got["IoU_C"].numpy(), [c0, c1, float("nan"), float("nan")], "IoU_C")
    _close(got["mIoU_C"], (c0 + c1) / 2, "mIoU_C")
    # m = 3 pictures: ceil(0.05 * 3) = 1 -> the lowest; ceil(0.5 * 3) = 2 -> the two lowest
    _close(got["mIoU_I_q"][0.05], i2, "mIoU_I_q[0.05]")
    _close(got["mIoU_I_q"][0.5], (i2 + i0) / 2, "mIoU_I_q[0.5]")
    assert got["mIoU_I_q"][1.0] == got["mIoU_I"]
    # per class: class 0 has m = 3, class 1 m = 2; at q = 0.05 the lowest of each, at q = 0.5 two of class 0 and one of class 1
    _close(got["mIoU_C_q"][0.05], (5 / 60 + 10 / 45) / 2, "mIoU_C_q[0.05]")
    _close(got["mIoU_C_q"][0.5], ((5 / 60 + 40 / 55) / 2 + 10 / 45) / 2, "mIoU_C_q[0.5]")
    one = fine(torch.from_numpy(TENSORS["one_picture"]), (0.05, 1.0))
    s = (3 / 10 + 1 / 9) / 2
    _close(one["image_mIoU"].numpy(), [s], "n = 1")
    assert one["mIoU_I"] == one["mIoU_I_q"][0.05] == one["mIoU_I_q"][1.0] == one["image_mIoU"][0].item()
    _close(one["IoU_C"].numpy(), [3 / 10, float("nan"), 1 / 9], "n = 1 IoU_C")
    empty = fine(torch.zeros(0, 3, 4, dtype=torch.int64))
    assert tuple(empty["image_mIoU"].shape) == (0,) and math.isnan(empty["mIoU_I"]) and math.isnan(empty["mIoU_C_q"][0.1])
    nothing = fine(torch.from_numpy(TENSORS["all_ignored"]))
    assert bool(torch.isnan(nothing["image_mIoU"]).all()) and math.isnan(nothing["mIoU_I"]) and math.isnan(nothing["mIoU_I_q"][0.05])


def test_worst_images():
    ties = torch.from_numpy(TENSORS["ties"])
    assert SegEvaluator.worst_images(ties, 4) == [(1, 0.25), (0, 0.5), (2, 0.5), (3, 0.5)]
    assert SegEvaluator.worst_images(ties, 2) == [(1, 0.25), (0, 0.5)]
    assert SegEvaluator.worst_images(ties, 9) == SegEvaluator.worst_images(ties, 4) and SegEvaluator.worst_images(ties, 0) == []
    mixed = torch.from_numpy(TENSORS["ignored_and_unlabelled"])
    got = SegEvaluator.worst_images(mixed, 10)
    assert [i for i, _ in got] == [2, 0, 3], "the all-ignored picture has no score and is left out"
    for name, a in TENSORS.items():
        got, want = SegEvaluator.worst_images(torch.from_numpy(a), 5), ir.worst_images(a, 5)
        assert [i for i, _ in got] == [i for i, _ in want], name
        _close([s for _, s in got], [s for _, s in want], name)


@pytest.mark.parametrize("name", ["ignored_and_unlabelled", "random21", "one_picture"])
def test_bootstrap(name):
    a = TENSORS[name]
    t = torch.from_numpy(a)
    got = SegEvaluator.bootstrap_miou(t, n_boot=200, alpha=0.1, seed=3)
    assert list(got) == ["lo", "hi", "std", "replicates"]
    assert got["replicates"].dtype == torch.float64 and tuple(got["replicates"].shape) == (200,)
    assert got["lo"] <= got["hi"] and got["std"] >= 0.0
    again = SegEvaluator.bootstrap_miou(t, n_boot=200, alpha=0.1, seed=3)
    assert np.array_equal(got["replicates"].numpy(), again["replicates"].numpy(), equal_nan=True)
    assert (got["lo"], got["hi"], got["std"]) == (again["lo"], again["hi"], again["std"])
    if a.shape[0] > 1:
        other = SegEvaluator.bootstrap_miou(t, n_boot=200, alpha=0.1, seed=4)
        assert not np.array_equal(got["replicates"].numpy(), other["replicates"].numpy(), equal_nan=True), "the seed is not read"
    want = ir.bootstrap(a, n_boot=200, alpha=0.1, seed=3)
    if name == "ignored_and_unlabelled":   # some replicate drew the all-ignored picture four times: no mIoU, left out of the figures
        assert bool(torch.isnan(got["replicates"]).any()) and not math.isnan(got["lo"])
    _close(got["replicates"].numpy(), want["replicates"], name)
    _close([got["lo"], got["hi"]], [want["lo"], want["hi"]], name)
    # the deviations from the mean are differences of figures in [0, 1] that each carry a rounding of 2^-53: an absolute floor
    assert abs(got["std"] - want["std"]) <= RTOL * want["std"] + 1e-15, name


def test_bootstrap_of_identical_pictures_is_a_point():
    row = _row(5, {0: (30, 40, 50), 1: (7, 9, 8), 4: (0, 3, 0)})
    t = torch.from_numpy(np.stack([row] * 6))
    got = SegEvaluator.bootstrap_miou(t, n_boot=50)
    plain = SegEvaluator.metrics_from_areas(t.sum(0))["mIoU"]
    assert plain == pytest.approx(SegEvaluator.metrics_from_areas(torch.from_numpy(row))["mIoU"], rel=RTOL)
    # every replicate sums six copies of one row: the same three integers per class, so the same quotient bit for bit
    assert got["lo"] == got["hi"] == plain and bool((got["replicates"] == plain).all()) and got["std"] <= 1e-15
    defaults = SegEvaluator.bootstrap_miou(t[:2])
    assert tuple(defaults["replicates"].shape) == (1000,)


def test_value_errors():
    good = torch.zeros(2, 3, 4, dtype=torch.int64)
    for call in (fine, lambda a: SegEvaluator.worst_images(a, 1), SegEvaluator.bootstrap_miou):
        for bad in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(2, 2, 4, dtype=torch.int64), torch.zeros(2, 3, 4, 1, dtype=torch.int64)):
            with pytest.raises(ValueError, match=r"\(n, 3, C\) integer tensor, got torch.int64"):
                call(bad)
        for bad in (good.double(), good.float(), good.bool()):
            with pytest.raises(ValueError, match=r"\(n, 3, C\) integer tensor, got torch\.(float|bool)"):
                call(bad)
        with pytest.raises(ValueError, match=r"\(n, 3, C\) integer tensor"):
            call(good.tolist())
    for q in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match=r"q lies in \(0, 1\]"):
            fine(good, (0.05, q))
    with pytest.raises(ValueError, match="at least one picture"):
        SegEvaluator.bootstrap_miou(good[:0])
    with pytest.raises(ValueError, match="at least one picture and one replicate"):
        SegEvaluator.bootstrap_miou(good, n_boot=0)
    for alpha in (0.0, 1.0, -1.0):
        with pytest.raises(ValueError, match=r"alpha lies in \(0, 1\)"):
            SegEvaluator.bootstrap_miou(good, alpha=alpha)
