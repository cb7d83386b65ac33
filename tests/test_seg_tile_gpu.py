"""GPU: the device-side row check of the three rescaled label-map entries - segclip_seg_label_map_rescaled, its 16-bit twin
and the threshold sweep (csrc/segment_tile.inc: seg_tile_load).  The host entries cannot inspect the image table, which lives
in device memory, so the kernels range-check every row and skip an image whose row is inconsistent: its label elements keep
what they held, its pixels add nothing to the areas, and the other images of the table are not disturbed.  The rows used here
are table contents the kernels are written to refuse.

Two images in one table, one 32 x 32 window each on a 2 x 2 grid, 8 groups, 5 classes + background, outputs of 20 x 27 (540
pixels: no lane straddles an image's end) and, for the equality case, 21 x 27 (567 = 4 * 141 + 3: the last lane of an image
stores three labels one by one and counts three ground-truth pixels).
"""
import functools

import pytest
import torch

from segclip_amd import _lib as L
from segclip_amd import ops
from tests import seg_wide_cases as swc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G, N, C, NET, GRID = 8, 5, 6, (32, 32), (2, 2)
THR, SWEEP_THR = 0.5, (0.3, 0.5, 0.7)
SENT = {torch.uint8: 0xA5, torch.int16: -23131}   # 0xA5A5 as int16
ENTRIES = ("rescaled", "wide", "sweep")
SI_OH, SI_LAB, SI_GT, SI_SOFT = (L.const("SI_" + c) for c in ("OH", "LAB", "GT", "SOFT"))   # columns of the image table


@functools.lru_cache(maxsize=None)
def _inputs(out):
    """Device inputs of the two images at output size `out`, made once and never written to."""
    g = torch.Generator().manual_seed(7)
    soft = torch.softmax(torch.randn(2, G, *GRID, generator=g) * 2.0, dim=1)
    t32 = swc.f32_tables(torch.rand(2, G, N, generator=g, dtype=torch.float64))
    tabs = (t32["table"].to(DEV), t32["table_max"].to(DEV), t32["best_class"].int().to(DEV), t32["best_score"].to(DEV))
    oh, ow = out
    gt = torch.randint(0, C + 1, (2, oh * ow), generator=g)   # C itself: counted in the prediction area only
    gt[:, 5:40] = -1                                          # the ignore value of either width
    rows = [dict(first=b, count=1, net=NET, out=out, win=NET, grid=GRID, soft_off=b * G * GRID[0] * GRID[1], gt_off=b * oh * ow)
            for b in range(2)]
    images, offs, n_elems, n_blocks, most = ops.seg_image_table(rows, DEV)
    dwin = torch.tensor([(0, 0, 0), (1, 0, 0)], dtype=torch.int32, device=DEV)
    return dict(soft=soft.reshape(-1).to(DEV), tabs=tabs, dwin=dwin, images=images, offs=offs, n=n_elems, n_blocks=n_blocks,
                most=most, gt=gt, total=oh * ow)


def _run(entry, inp, images):
    """One launch on a pre-filled label buffer -> (labels (T, n) as the stored elements, areas (T, 3, C)), on the CPU."""
    dtype = torch.int16 if entry == "wide" else torch.uint8
    T = len(SWEEP_THR) if entry == "sweep" else 1
    gt = (inp["gt"] & (0xFFFF if entry == "wide" else 0xFF)).reshape(-1)
    gt = (swc.to_i16(gt) if entry == "wide" else gt.to(torch.uint8)).to(DEV)
    labels = torch.full((T, inp["n"]), SENT[dtype], dtype=dtype, device=DEV)
    areas = torch.zeros(T, 3, C, dtype=torch.int64, device=DEV)
    common = (inp["soft"], inp["tabs"], inp["dwin"], images, inp["n_blocks"], inp["most"])
    if entry == "sweep":
        ops.seg_label_map_sweep(*common, SWEEP_THR, labels=labels, gt=gt, areas=areas, ignore_index=255)
    elif entry == "wide":
        ops.seg_label_map_rescaled_wide(*common, True, THR, labels=labels[0], gt=gt, areas=areas[0], ignore_index=65535)
    else:
        ops.seg_label_map_rescaled(*common, True, THR, labels=labels[0], gt=gt, areas=areas[0], ignore_index=255)
    torch.cuda.synchronize()
    return labels.cpu(), areas.cpu()


def _areas_alone(entry, inp, labels, b):
    """segclip_seg_areas / _wide of image b's stored labels against its ground truth, per plane -> (T, 3, C) on the CPU."""
    o, total = inp["offs"][b], inp["total"]
    out = []
    for plane in labels:
        pred = plane[o:o + total].to(DEV)
        if entry == "wide":
            gt = swc.to_i16(inp["gt"][b] & 0xFFFF).to(DEV)
            out.append(ops.seg_areas_wide(pred, gt, C, 65535))
        else:
            gt = (inp["gt"][b] & 0xFF).to(torch.uint8).to(DEV)
            out.append(ops.seg_areas(pred, gt, C, 255))
    return torch.stack(out).cpu()


@functools.lru_cache(maxsize=None)
def _clean(entry, out):
    """The uncorrupted call of an entry and the areas of each image's labels alone, computed once."""
    inp = _inputs(out)
    labels, areas = _run(entry, inp, inp["images"])
    return labels, areas, [_areas_alone(entry, inp, labels, b) for b in range(2)]


def _corrupt(inp, what, bad):
    images = inp["images"].clone()
    if what == "soft":      # the image's soft assignment would end one float past soft_attn
        images[bad, SI_SOFT] = inp["soft"].numel() - G * GRID[0] * GRID[1] + 1
    elif what == "oh":
        images[bad, SI_OH] = 0
    else:                   # the labels would end past the buffer; no ground truth for this image
        images[bad, SI_LAB] = inp["n"] - inp["total"] + 1
        images[bad, SI_GT] = -1
    return images


@pytest.mark.parametrize("bad", [0, 1])
@pytest.mark.parametrize("what", ["soft", "oh", "lab"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_row_is_skipped(entry, what, bad):
    out = (20, 27)
    inp = _inputs(out)
    want_labels, want_areas, alone = _clean(entry, out)
    assert torch.equal(want_areas, alone[0] + alone[1]), "the uncorrupted call's areas are not the sum of its images'"
    assert int(alone[bad][:, 1].sum()) > 0, "the image to corrupt counts nothing anyway"
    labels, areas = _run(entry, inp, _corrupt(inp, what, bad))
    good = 1 - bad
    o_bad, o_good, total = inp["offs"][bad], inp["offs"][good], inp["total"]
    sent = SENT[labels.dtype]
    assert bool((labels[:, o_bad:o_bad + total] == sent).all()), "the refused image's labels were written"
    assert bool((want_labels[:, o_bad:o_bad + total] != sent).all()), "the sentinel is a label of the uncorrupted call"
    assert torch.equal(labels[:, o_good:o_good + total], want_labels[:, o_good:o_good + total]), "the other image's labels changed"
    assert torch.equal(areas, alone[good]), "the areas are not those of the other image alone"


@pytest.mark.parametrize("entry", ENTRIES)
def test_lane_straddling_an_images_end(entry):
    """567 pixels per image: the last lane of an image owns three of them.  The fused counters equal segclip_seg_areas /
    segclip_seg_areas_wide of the entry's own labels, and the padding element between the images is not written."""
    out = (21, 27)
    inp = _inputs(out)
    assert inp["total"] % 4 == 3 and inp["offs"] == [0, inp["total"] + 1]
    labels, areas, alone = _clean(entry, out)
    sent = SENT[labels.dtype]
    assert bool((labels[:, inp["total"]] == sent).all()) and bool((labels[:, inp["n"] - 1] == sent).all())
    assert bool((labels[:, :inp["total"]] != sent).all())
    assert torch.equal(areas, alone[0] + alone[1])
    assert int(areas[:, 1].sum()) == areas.shape[0] * int((inp["gt"] >= 0).sum())
