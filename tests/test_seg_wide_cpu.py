"""CPU: what the 16-bit label-map path (csrc/segment_wide.inc, SegInference(label_dtype=torch.int16)) states without a device -
the reference counts of the synthetic cases of tests/seg_wide_cases.py, the two new symbols of the C ABI and their binding,
and the argument validation of the host layer."""
import os
import types

import pytest
import torch

from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import Boundary, SegEvaluator, SegInference, SegSweepEvaluator, _Maps
from tests import seg_wide_cases as swc
from tests.helpers import HEADER, header_declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(swc.CASES))
def test_case_generators_reproduce_the_reference_counts(name):
    """Output pixels, near-ties, distinct labels, labels above 255 and the largest label of the fp64 reference alone; the fp32
    restatement of the reference gives the same labels."""
    case, want, tie = swc.reference(name)
    assert swc.counts(want, tie) == swc.NEAR_TIE_COUNTS[name]
    assert int(tie.sum()) <= swc.CAP * tie.numel()
    l32, _, _ = swc.reference_of(case, torch.float32)
    assert torch.equal(l32, want)
    mode, stride, B, net, out, N, with_bg, thr, seed, step = swc.CASES[name]
    assert tuple(want.shape) == (B, *out) and int(want.max()) <= N - 1 + int(with_bg)
    assert case["t32"]["table"].shape == (len(case["wins"]), swc.G, N)


def test_cases_cover_what_they_are_for():
    labels = {name: set(swc.reference(name)[1].unique().tolist()) for name in swc.CASES}
    assert 847 in labels["w848_slide"] and 459 in labels["w460_whole"]       # the last class of a vocabulary, 847 = 13 * 64 + 15
    assert 1023 in labels["w1024_nobg"]                                       # and of one that is a multiple of 64
    assert {255, 256, 257} & labels["w848_slide"] and {256, 257} <= labels["w460_whole"] | labels["w848_slide"]
    counts = {name: swc.sr.assemble(c["soft"], c["t32"], c["wins"], (c["B"], *c["net"]), c["win"], c["with_bg"], c["thr"])["count"]
              for name, c in ((n, swc.make_case(n)) for n in ("w460_whole", "w848_slide", "w300_down"))}
    assert int(counts["w460_whole"].max()) == 1 and int(counts["w848_slide"].max()) == 2 and int(counts["w300_down"].max()) == 4
    # tables staged in LDS (all six windows of an image within the copy of 4096 floats) and read from global memory (not one
    # window's table fits, or not the four windows that touch a tile)
    assert swc.G * swc.CASES["w21_small"][5] * 6 <= 4096 < swc.G * swc.CASES["w848_slide"][5]
    # the per-lane scan of up to 32 classes and the cooperative scan above them, both on staged tables
    assert swc.CASES["w21_small"][5] + 1 <= 32 < swc.CASES["w61_staged"][5] + 1 and swc.G * swc.CASES["w61_staged"][5] * 6 <= 4096
    assert 4096 < swc.G * swc.CASES["w1024_nobg"][5] and 4096 < 4 * swc.G * swc.CASES["w300_down"][5]
    scale = {name: (c[4][0] / c[3][0], c[4][1] / c[3][1]) for name, c in swc.CASES.items()}
    assert min(scale["w848_slide"]) > 1 and max(scale["w300_down"]) < 1 and scale["w1024_nobg"] == (1, 1)


def test_i16_round_trip():
    v = torch.tensor([0, 1, 255, 256, 1023, 32767, 32768, 42405, 65535])
    assert swc.to_i16(v).dtype == torch.int16 and torch.equal(swc.from_i16(swc.to_i16(v)), v)
    assert int(swc.to_i16(torch.tensor([65535]))) == -1


def test_header_declares_the_wide_entries_and_lib_binds_them():
    wide = header_declaration("segclip_seg_label_map_rescaled_wide")
    narrow = header_declaration("segclip_seg_label_map_rescaled")
    assert len(wide) == len(narrow) == 24
    changed = [(a, b) for a, b in zip(narrow, wide) if a != b]
    assert changed == [("uint8_t* labels", "uint16_t* labels"), ("int64_t labels_bytes", "int64_t labels_elems"),
                       ("const uint8_t* gt", "const uint16_t* gt"), ("int64_t gt_bytes", "int64_t gt_elems")]
    areas = header_declaration("segclip_seg_areas_wide")
    assert areas[:2] == ["const uint16_t* pred", "const uint16_t* gt"] and len(areas) == len(header_declaration("segclip_seg_areas")) == 8
    assert L.SIGNATURES["segclip_seg_label_map_rescaled_wide"] == L.SIGNATURES["segclip_seg_label_map_rescaled"]
    assert ops.SEG_WIDE_MAX_CLASSES == 1024
    inc = open(os.path.join(ROOT, "segclip_amd", "csrc", "segment_wide.inc")).read()
    assert "#define SEGCLIP_SEG_WIDE_MAX_CLASSES 1024 " in open(HEADER).read() and "SEG_WIDE_MAX_CLASSES SEGCLIP_SEG_WIDE_MAX_CLASSES" in inc
    assert "SEG_WIDE_LANE_SCAN_CLASSES 32" in inc   # what the cases w21_small and w61_staged are placed around


def test_seg_inference_arguments():
    emb = torch.zeros(4, 8)
    for bad in (torch.int32, torch.int64, torch.float32, "int16", None):
        with pytest.raises(ValueError, match="label_dtype"):
            SegInference(None, emb, True, label_dtype=bad)
    for ok in (torch.uint8, torch.int16):     # a valid label_dtype reaches the device check: there is no CPU path
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            SegInference(None, emb, True, label_dtype=ok)
    check = SegInference._check_classes
    check(types.SimpleNamespace(wide=True, num_classes=1024))
    check(types.SimpleNamespace(wide=False, num_classes=256))
    with pytest.raises(L.Unsupported, match="1025.*1024"):
        check(types.SimpleNamespace(wide=True, num_classes=1025))
    with pytest.raises(L.Unsupported, match="257.*256.*label_dtype=torch.int16"):
        check(types.SimpleNamespace(wide=False, num_classes=257))


def test_seg_evaluator_arguments():
    wide = types.SimpleNamespace(label_dtype=torch.int16, wide=True, with_bg=True, num_classes=848, text_embedding=torch.zeros(1))
    ev = SegEvaluator(wide, ignore_index=65535)
    assert tuple(ev.areas.shape) == (3, 848) and ev.areas.dtype == torch.int64 and ev.gt_dtype == torch.int16
    assert SegEvaluator(wide).ignore_index == 255 and SegEvaluator(wide, ignore_index=0).ignore_index == 0
    for bad in (-1, 65536, 255.0, True, None):
        with pytest.raises(ValueError, match="0 .. 65535"):
            SegEvaluator(wide, ignore_index=bad)
    with pytest.raises(ValueError, match="boundary"):
        SegEvaluator(wide, boundary=Boundary())
    with pytest.raises(ValueError, match="SegSweepEvaluator"):
        SegSweepEvaluator(wide, [0.1, 0.2])
    narrow = types.SimpleNamespace(label_dtype=torch.uint8, wide=False, with_bg=True, num_classes=21, text_embedding=torch.zeros(1))
    assert SegEvaluator(narrow, boundary=Boundary()).gt_dtype == torch.uint8
    assert len(SegSweepEvaluator(narrow, [0.1, 0.2]).thresholds) == 2


def test_ops_refuse_cpu_tensors():
    lab = torch.zeros(16, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_areas_wide(lab, lab, 300)
    t = (torch.zeros(1, 8, 300), torch.zeros(1), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_label_map_rescaled_wide(torch.zeros(128), t, torch.zeros(1, 3, dtype=torch.int32),
                                        torch.zeros(1, 16, dtype=torch.int64), 1, 1, True, 0.5, labels=lab)


def test_maps_keep_the_element_type():
    """_Maps counts elements: a list of int16 maps that are not views of one buffer is gathered into an int16 buffer at offsets
    that are multiples of 4, views of one buffer are used where they lie."""
    a, b = torch.arange(15, dtype=torch.int16).view(3, 5) + 1000, torch.arange(6, dtype=torch.int16).view(2, 3) - 7
    batch = _Maps.of([a, b])
    assert batch.flat.dtype == torch.int16 and batch.offs == [0, 16] and batch.flat.numel() == 24
    assert all(torch.equal(v, m) for v, m in zip(batch.views(), (a, b))) and int(batch.flat[15]) == 0
    assert batch.empty_like().flat.dtype == torch.int16
    again = _Maps.of(batch.views())
    assert again.flat.data_ptr() == batch.flat.data_ptr() and again.offs == [0, 16]
