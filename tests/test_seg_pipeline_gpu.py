"""The whole post-processing chain of SegEvaluator.update_raw / SegInference.predict_raw in one call: all 16 combinations of
aug x refine x clean x boundary, held bit for bit and integer for integer to the composition of the public stand-alone
functions (predict_raw -> refine_labels -> despeckle, ops.seg_areas, boundary_areas).  It pins which maps every stage sees
and which kernel counts the mIoU areas, whatever the code between the entry points and the kernels looks like."""
import functools
import itertools

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import ops
from segclip_amd.segmentation import (PAMR, Boundary, Despeckle, ImageTransform, SegEvaluator, SegInference, TestAug,
                                      boundary_areas, despeckle, refine_labels)
from tests import boundary_reference as br
from tests.helpers import CountedEncodeImage, load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TF = ImageTransform()
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(90, 120), (130, 101), (75, 75)]
AUG, REFINE, CLEAN, BOUNDARY = TestAug(flip=True), PAMR(iters=2, dilations=(1, 2)), Despeckle(12), Boundary(radius=2)


@functools.lru_cache(maxsize=None)
def _setup():
    """(model, seg, raws, gts): built once, read by every case."""
    model = tiny_seg_model()
    emb = torch.from_numpy(load_golden("seg_tiny.npz")["text_embedding"]).to(DEV)
    g = torch.Generator().manual_seed(11)
    raws = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in RAW_SIZES]
    gts = [torch.from_numpy(br._blocks(np.random.default_rng(11 + i), h, w, 13, tuple(range(14)))).to(DEV)
           for i, (h, w) in enumerate(RAW_SIZES)]
    for t in gts:
        t[5:9] = 255
    return model, SegInference(model, emb, True, bg_thresh=0.02, **SLIDE), raws, gts


@functools.lru_cache(maxsize=None)
def _composed(aug, refine, clean):
    """The maps of the stand-alone functions one after the other, as clones that nothing writes to again; with no stage also
    the encode_image calls of the plain update_raw."""
    model, seg, raws, gts = _setup()
    if not refine and not clean:
        with CountedEncodeImage(model) as calls:
            maps = seg.predict_raw(raws, TF, aug=AUG if aug else None)
        with CountedEncodeImage(model) as plain:
            assert SegEvaluator(seg, reduce_zero_label=True).update_raw(raws, gts, TF, aug=AUG if aug else None) is None
        assert calls == plain and len(calls) > 0
        return [m.clone() for m in maps], plain
    if clean:
        before = _composed(aug, refine, False)[0]
        maps = despeckle(before, CLEAN.min_area)
    else:
        before = _composed(aug, False, False)[0]
        maps = refine_labels(raws, before, seg.num_classes, TF, REFINE)
    assert any(not torch.equal(a, b) for a, b in zip(maps, before)), "the stage changes nothing: the case proves nothing"
    return [m.clone() for m in maps], None


@pytest.mark.parametrize("aug,refine,clean,boundary", list(itertools.product([False, True], repeat=4)))
def test_every_combination_of_stages(aug, refine, clean, boundary):
    try:
        model, seg, raws, gts = _setup()
        C = seg.num_classes
        want, _ = _composed(aug, refine, clean)
        plain_calls = _composed(aug, False, False)[1]
        kw = dict(aug=AUG if aug else None, refine=REFINE if refine else None, clean=CLEAN if clean else None)
        want_areas = ops.seg_areas(torch.cat([m.reshape(-1) for m in want]), torch.cat([g.reshape(-1) for g in gts]), C,
                                   ignore_index=255, reduce_zero_label=True)
        assert int(want_areas[0].sum()) > 0
        want_b = boundary_areas(want, gts, C, BOUNDARY, reduce_zero_label=True) if boundary else None

        with CountedEncodeImage(model) as calls:
            predicted = seg.predict_raw(raws, TF, **kw)
        assert calls == plain_calls
        assert [tuple(t.shape) for t in predicted] == RAW_SIZES
        assert all(torch.equal(a, b) for a, b in zip(predicted, want)), "predict_raw differs from the composition"

        ev = SegEvaluator(seg, reduce_zero_label=True, boundary=BOUNDARY if boundary else None)
        with CountedEncodeImage(model) as calls:
            labels = ev.update_raw(raws, gts, TF, return_labels=True, **kw)
        assert calls == plain_calls
        assert [tuple(t.shape) for t in labels] == RAW_SIZES and all(t.dtype == torch.uint8 for t in labels)
        assert all(torch.equal(a, b) for a, b in zip(labels, predicted)), "update_raw's labels differ from predict_raw's"
        assert all(torch.equal(a, b) for a, b in zip(labels, want)), "update_raw's labels differ from the composition"
        assert torch.equal(ev.areas, want_areas), "the areas are not those of the final maps, counted once"
        if boundary:
            assert torch.equal(ev.boundary_areas, want_b) and int(want_b[0, 0].sum()) > 0 and int(want_b[1, 2].sum()) > 0
        else:
            assert ev.boundary_areas is None

        with CountedEncodeImage(model) as calls:
            assert ev.update_raw(raws, gts, TF, **kw) is None
        assert calls == plain_calls
        assert torch.equal(ev.areas, 2 * want_areas), "the call without return_labels counts other areas"
        if boundary:
            assert torch.equal(ev.boundary_areas, 2 * want_b)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
