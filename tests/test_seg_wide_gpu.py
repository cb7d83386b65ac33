"""GPU: 16-bit label maps for vocabularies of up to 1024 classes - segclip_seg_label_map_rescaled_wide / segclip_seg_areas_wide
(csrc/segment_wide.inc), SegInference(label_dtype=torch.int16), SegEvaluator over it and train.eval_epoch - against the fp64
yardsticks tests/seg_reference.py and tests/seg_eval_reference.py on the cases of tests/seg_wide_cases.py.

Near-ties: the rule and the cap of tests/test_seg_eval_gpu.py (a differing pixel is accepted only where a source tap or the
rescaled top-two gap is below 1e-6; at most 0.05 % of a case's output pixels, a fixed condition).  The reference of every case
has none (seg_wide_cases.NEAR_TIE_COUNTS), so the kernel's labels must equal the fp64 labels everywhere.

The end-to-end checks compare with the fp64 rescaling of THIS build's encode_decode logits, in which the groups are already
decided: there a near-tie is a rescaled gap below the bound alone."""
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops, synth
from segclip_amd.segmentation import (PAMR, Boundary, Despeckle, ImageTransform, SegEvaluator, SegInference, SegSweepEvaluator,
                                      TestAug, build_text_embedding, preprocess)
from segclip_amd.train import eval_epoch
from tests import seg_eval_reference as ser
from tests import seg_wide_cases as swc
from tests.helpers import tiny_seg_model
from tests.seg_wide_cases import CAP, CASES, G, GRID, NEAR_TIE_COUNTS, TIE, from_i16, to_i16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT16 = 0xA5A5 - 65536   # the frame of an int16 buffer: no label reaches it


def _dev_tables(t32):
    return (t32["table"].to(DEV), t32["table_max"].to(DEV), t32["best_class"].int().to(DEV), t32["best_score"].to(DEV))


def _kernel_inputs(case, gt_offsets=None):
    images, lab_offs, n_elems, n_blocks, most = ops.seg_image_table(swc.image_rows(case, gt_offsets), DEV)
    dwin = torch.tensor(case["wins"], dtype=torch.int32, device=DEV).view(-1, 3)
    return case["soft"].reshape(-1).to(DEV), _dev_tables(case["t32"]), dwin, images, lab_offs, n_elems, n_blocks, most


def _run_wide(case, gt=None, reduce_zero=False, ignore_index=65535, pad=64):
    """The kernel through a framed int16 buffer, launched twice (labels and areas bit-equal), frame and gaps checked.
    -> labels (B, oh, ow) long on the CPU, areas (3, C) long or None."""
    B, (oh, ow) = case["B"], case["out"]
    C = case["N"] + int(case["with_bg"])
    offs = None if gt is None else [b * oh * ow for b in range(B)]
    soft, tabs, dwin, images, lab_offs, n_elems, n_blocks, most = _kernel_inputs(case, offs)
    gt_dev = None if gt is None else to_i16(gt).reshape(-1).to(DEV)
    res = []
    for _ in range(2):
        buf = torch.full((n_elems + 2 * pad,), SENT16, dtype=torch.int16, device=DEV)
        view = buf[pad:pad + n_elems]
        areas = None if gt is None else torch.zeros(3, C, dtype=torch.int64, device=DEV)
        ops.seg_label_map_rescaled_wide(soft, tabs, dwin, images, n_blocks, most, case["with_bg"], case["thr"], labels=view,
                                        gt=gt_dev, areas=areas, ignore_index=ignore_index, reduce_zero_label=reduce_zero)
        torch.cuda.synchronize()
        assert bool((buf[:pad] == SENT16).all()) and bool((buf[pad + n_elems:] == SENT16).all()), "the kernel wrote outside its output"
        for b, o in enumerate(lab_offs):   # the elements between two images are not written either
            end = lab_offs[b + 1] if b + 1 < B else n_elems
            assert bool((view[o + oh * ow:end] == SENT16).all())
        labels = from_i16(torch.stack([view[o:o + oh * ow].view(oh, ow) for o in lab_offs]).cpu())
        res.append((labels, None if areas is None else areas.cpu()))
    assert torch.equal(res[0][0], res[1][0]), "repeat launch differs"
    if gt is not None:
        assert torch.equal(res[0][1], res[1][1]), "repeat launch: areas differ"
    return res[0]


# ------------------------------------------------------------------------------------------------ a. kernel against fp64
@pytest.mark.parametrize("name", list(CASES))
def test_wide_labels_against_reference(name):
    case, want, tie = swc.reference(name)
    n_tie = int(tie.sum())
    # an odd pad: the first image's labels start on no 8-byte boundary, and the lanes fall back to 2-byte stores
    got, _ = _run_wide(case, pad=64 if CASES[name][-2] % 2 else 3)
    print(f"{name}: {tie.numel()} output pixels, {n_tie} near-ties, labels differ at {int((got != want).sum())}, "
          f"{got.unique().numel()} distinct labels, largest {int(got.max())}")
    assert swc.counts(want, tie) == NEAR_TIE_COUNTS[name], "the reference's own counts changed"
    assert n_tie <= CAP * tie.numel(), f"{name}: {n_tie} near-ties of {tie.numel()} pixels in the reference itself"
    assert bool((got == want)[~tie].all()), f"{name}: labels differ away from near-ties"


# ------------------------------------------------------------------------------------------------ b. the uint8 kernel's bits
@pytest.mark.parametrize("name, N", [("w21_small", None), ("w61_staged", None), ("w300_down", 255)])
def test_wide_equals_narrow_below_257_classes(name, N):
    case = swc.make_case(name, N)
    B, (oh, ow) = case["B"], case["out"]
    C = case["N"] + int(case["with_bg"])
    assert C <= 256
    want, _, _ = swc.reference_of(case)
    gt = swc.synthetic_gt(want, C, 78).clamp_max(255)   # what a uint8 ground truth can hold; 255 is ignored by both
    offs = [b * oh * ow for b in range(B)]
    soft, tabs, dwin, images, lab_offs, n_elems, n_blocks, most = _kernel_inputs(case, offs)
    lab8 = torch.zeros(n_elems, dtype=torch.uint8, device=DEV)
    lab16 = torch.zeros(n_elems, dtype=torch.int16, device=DEV)
    a8, a16 = (torch.zeros(3, C, dtype=torch.int64, device=DEV) for _ in range(2))
    args = (soft, tabs, dwin, images, n_blocks, most, case["with_bg"], case["thr"])
    ops.seg_label_map_rescaled(*args, labels=lab8, gt=gt.to(torch.uint8).reshape(-1).to(DEV), areas=a8, ignore_index=255)
    ops.seg_label_map_rescaled_wide(*args, labels=lab16, gt=to_i16(gt).reshape(-1).to(DEV), areas=a16, ignore_index=255)
    torch.cuda.synchronize()
    assert torch.equal(lab16, lab8.to(torch.int16)), f"{name}: the 16-bit labels differ from the uint8 kernel's"
    assert torch.equal(a16, a8), f"{name}: the areas differ from the uint8 kernel's"
    assert int(a8[0].sum()) > 0 and lab8.unique().numel() >= 10


# ------------------------------------------------------------------------------------------------ c. first maximum on exact ties
def test_first_maximum_on_exact_ties():
    """Every table row holds 0.875 at the classes 70 and 700 and 0.75 at 130 and 641: whatever the windows and taps, the classes
    70 and 700 tie exactly, and the first maximum is 70 (label 71 behind the background); lanes 6 and 60 of the scan hold them,
    lanes 2 and 1 the lower pair."""
    case = swc.make_case("w848_slide")
    case["out"] = case["net"]
    t = case["t32"]["table"].double()
    t[..., 70] = t[..., 700] = 0.875
    t[..., 130] = t[..., 641] = 0.75
    case["t32"] = swc.f32_tables(t)
    got, _ = _run_wide(case)
    B, (H, W) = case["B"], case["net"]
    C = case["N"] + 1
    dwin = torch.tensor(case["wins"], dtype=torch.int32, device=DEV).view(-1, 3)
    dfirst = torch.arange(0, len(case["wins"]) + 1, case["per"], dtype=torch.int32, device=DEV)
    soft = case["soft"].reshape(len(case["wins"]), G, -1).to(DEV)
    logits = ops.seg_logits(soft, _dev_tables(case["t32"]), dwin, dfirst, (B, H, W), case["win"], GRID, True, case["thr"])
    amax = logits.amax(dim=1, keepdim=True)
    idx = torch.arange(C, device=DEV).view(1, C, 1, 1)
    first = torch.where(logits == amax, idx, torch.full_like(idx, C)).amin(dim=1).cpu()
    assert torch.equal(got, first), "the labels are not the first maximum of segclip_seg_logits"
    assert int((got == 701).sum()) == 0 and int((got == 71).sum()) > 0
    tied = (logits[:, 71] == logits[:, 701]) & (logits[:, 71] == amax[:, 0])
    assert int(tied.sum()) == int((got == 71).sum())


# ------------------------------------------------------------------------------------------------ d. areas
@pytest.mark.parametrize("name", ["w848_slide", "w460_whole", "w300_down"])
@pytest.mark.parametrize("reduce_zero", [False, True])
@pytest.mark.parametrize("ignore_index", [65535, 255])
def test_wide_areas(name, reduce_zero, ignore_index):
    case, want, tie = swc.reference(name)
    C = case["N"] + int(case["with_bg"])
    gt = swc.synthetic_gt(want, C, 77)
    labels, areas = _run_wide(case, gt=gt, reduce_zero=reduce_zero, ignore_index=ignore_index)
    assert torch.equal(areas, ser.areas(labels, gt, C, ignore_index, reduce_zero)), "areas differ from the reference on the same labels"
    lab16, gt16 = to_i16(labels).to(DEV), to_i16(gt).to(DEV)
    alone = ops.seg_areas_wide(lab16, gt16, C, ignore_index, reduce_zero)
    assert torch.equal(areas, alone.cpu()), "the fused counters differ from segclip_seg_areas_wide on the kernel's own labels"
    twice = ops.seg_areas_wide(lab16, gt16, C, ignore_index, reduce_zero, areas=alone.clone())
    assert torch.equal(twice, 2 * alone), "a second call must double the areas it is given"
    ignored = (gt == ignore_index) | ((gt == 0) if reduce_zero else torch.zeros_like(gt, dtype=torch.bool))
    assert int(areas[1].sum()) == int((~ignored).sum())
    assert bool((areas[0] <= areas[1]).all()) and bool((areas[0] <= areas[2]).all())
    if not reduce_zero:   # with it the ground truth, the labels themselves, is shifted by one class against them
        assert int(areas[0].sum()) > 0
    if ignore_index == 255:   # the band of 65535 is then a value >= C: in the prediction area only
        assert int(areas[2].sum()) < int(areas[1].sum())


# ------------------------------------------------------------------------------------------------ e. limits and refusals
def test_kernel_limits():
    case = swc.make_case("w21_small")
    soft, tabs, dwin, images, _, n_elems, n_blocks, most = _kernel_inputs(case)
    labels = torch.zeros(n_elems, dtype=torch.int16, device=DEV)
    args = (soft, tabs, dwin, images, n_blocks, most, True, 0.5)
    big = swc.f32_tables(torch.rand(len(case["wins"]), G, 1024, dtype=torch.float64))
    with pytest.raises(L.Unsupported, match="1025"):   # 1024 classes + background
        ops.seg_label_map_rescaled_wide(soft, _dev_tables(big), dwin, images, n_blocks, most, True, 0.5, labels=labels)
    ops.seg_label_map_rescaled_wide(soft, _dev_tables(big), dwin, images, n_blocks, most, False, 0.5, labels=labels)   # 1024 fit
    with pytest.raises(L.Unsupported, match="1025"):
        ops.seg_areas_wide(labels, labels, 1025)
    with pytest.raises(L.Unsupported, match="65 windows"):
        ops.seg_label_map_rescaled_wide(soft, tabs, dwin, images, n_blocks, 65, True, 0.5, labels=labels)
    with pytest.raises(ValueError, match="int16"):
        ops.seg_label_map_rescaled_wide(*args, labels=labels.to(torch.uint8))
    with pytest.raises(ValueError, match="int16"):
        ops.seg_label_map_rescaled_wide(*args, labels=labels, gt=labels.to(torch.uint8), areas=torch.zeros(3, 21, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="areas"):
        ops.seg_label_map_rescaled_wide(*args, labels=labels, gt=labels, areas=torch.zeros(3, 20, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="int16"):
        ops.seg_areas_wide(labels.to(torch.uint8), labels, 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_areas_wide(labels.cpu(), labels.cpu(), 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_label_map_rescaled_wide(*args, labels=labels.cpu())
    # the uint8 entries keep their limit
    with pytest.raises(L.Unsupported):
        ops.seg_areas(labels.to(torch.uint8), labels.to(torch.uint8), 257)
    wide = swc.f32_tables(torch.rand(len(case["wins"]), G, 256, dtype=torch.float64))
    with pytest.raises(L.Unsupported):
        ops.seg_label_map_rescaled(soft, _dev_tables(wide), dwin, images, n_blocks, most, True, 0.5,
                                   labels=labels.to(torch.uint8))
    torch.cuda.synchronize()


SLIDE = dict(mode="slide", crop_size=(64, 64), stride=(48, 48))


def _embedding(n, seed=3, width=64):
    e = torch.randn(n, width, generator=torch.Generator().manual_seed(seed))
    return (e / e.norm(dim=-1, keepdim=True)).to(DEV)


def test_refused_stages_and_class_limits():
    try:
        model = tiny_seg_model()
        seg = SegInference(model, _embedding(300), True, bg_thresh=0.03, label_dtype=torch.int16, **SLIDE)
        tf = ImageTransform(img_scale=(256, 96))
        raw = torch.zeros(120, 150, 3, dtype=torch.uint8, device=DEV)
        img = torch.zeros(3, 96, 120, device=DEV)
        gt16 = torch.zeros(120, 150, dtype=torch.int16, device=DEV)
        ev = SegEvaluator(seg, ignore_index=65535)
        calls = []
        model.clip.encode_image = lambda *a, **k: calls.append(1)   # a refusal comes before the towers
        try:
            for stage, call in [
                    ("aug", lambda: seg.predict_raw([raw], tf, aug=TestAug(flip=True))),
                    ("refine", lambda: seg.predict_raw([raw], tf, refine=PAMR())),
                    ("clean", lambda: seg.predict_raw([raw], tf, clean=Despeckle(4))),
                    ("refine", lambda: seg.predict_list([img], refine=PAMR())),
                    ("clean", lambda: seg.predict_list([img], clean=Despeckle(4))),
                    ("predict_views", lambda: seg.predict_views([[(img, 0)]], [(120, 150)])),
                    ("render_raw", lambda: seg.render_raw([raw], tf, ["pred"], torch.zeros(4, 3, dtype=torch.uint8))),
                    ("aug", lambda: ev.update_raw([raw], [gt16], tf, aug=TestAug(flip=True))),
                    ("refine", lambda: ev.update_raw([raw], [gt16], tf, refine=PAMR())),
                    ("clean", lambda: ev.update_raw([raw], [gt16], tf, clean=Despeckle(4))),
                    ("refine", lambda: ev.update([img], [gt16], refine=PAMR())),
                    ("update_views", lambda: ev.update_views([[(img, 0)]], [gt16])),
                    ("boundary", lambda: SegEvaluator(seg, boundary=Boundary())),
                    ("SegSweepEvaluator", lambda: SegSweepEvaluator(seg, [0.1, 0.2]))]:
                with pytest.raises(ValueError, match=stage):
                    call()
            with pytest.raises(ValueError, match="int16"):   # a uint8 ground truth for a wide evaluator
                ev.update([img], [gt16.to(torch.uint8)])
            with pytest.raises(ValueError, match="uint8"):   # and an int16 one for a narrow evaluator
                SegEvaluator(SegInference(model, _embedding(20), True, **SLIDE)).update([img], [gt16])
            with pytest.raises(ValueError, match="65535"):
                SegEvaluator(seg, ignore_index=-1)
            with pytest.raises(ValueError, match="label_dtype"):
                SegInference(model, _embedding(20), True, label_dtype=torch.int32)
            with pytest.raises(L.Unsupported, match="1025.*1024"):
                SegInference(model, _embedding(1024), True, label_dtype=torch.int16, **SLIDE).predict_list([img])
            with pytest.raises(L.Unsupported, match="257"):   # the narrow path keeps its limit
                SegInference(model, _embedding(256), True, **SLIDE).predict(img[None])
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                seg.predict_list([img.cpu()])
            assert not calls and int(ev.areas.abs().sum()) == 0
        finally:
            del model.clip.encode_image
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ f. end to end
def _first_maximum(logits):
    """(C, H, W) -> (H, W) long: the lowest class among the maxima."""
    C = logits.shape[0]
    idx = torch.arange(C, device=logits.device).view(C, 1, 1)
    return torch.where(logits == logits.amax(dim=0, keepdim=True), idx, torch.full_like(idx, C)).amin(dim=0)


def test_end_to_end_300_classes():
    try:
        model = tiny_seg_model()
        emb = _embedding(300)
        seg = SegInference(model, emb, True, bg_thresh=0.0, label_dtype=torch.int16, **SLIDE)
        C = seg.num_classes
        assert C == 301
        gen = torch.Generator().manual_seed(6)
        # predict = the first maximum of this build's encode_decode, slide and whole
        batch = torch.randn(2, 3, 100, 150, generator=gen).to(DEV)
        got = seg.predict(batch)
        assert got.dtype == torch.int16 and tuple(got.shape) == (2, 100, 150)
        logits = seg.encode_decode(batch)
        assert all(torch.equal(from_i16(got[b]), _first_maximum(logits[b])) for b in range(2))
        whole = SegInference(model, emb, True, bg_thresh=0.0, label_dtype=torch.int16)
        square = torch.randn(1, 3, 128, 128, generator=gen).to(DEV)
        assert torch.equal(from_i16(whole.predict(square)[0]), _first_maximum(whole.encode_decode(square)[0]))
        print(f"predict: {from_i16(got).unique().numel()} distinct labels, largest {int(from_i16(got).max())}")
        # predict_list / predict_raw against the fp64 rescaling of those logits
        tf = ImageTransform(img_scale=(256, 96))
        raws = [torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).to(DEV) for (h, w) in [(120, 150), (133, 100), (96, 96)]]
        imgs = preprocess(raws, tf)
        outs = [tuple(r.shape[:2]) for r in raws]
        listed, from_raw = seg.predict_list(imgs, outs), seg.predict_raw(raws, tf)
        assert all(t.dtype == torch.int16 and tuple(t.shape) == o for t, o in zip(listed, outs))
        store = listed[0].untyped_storage().data_ptr()
        assert all(t.untyped_storage().data_ptr() == store for t in listed), "list calls return views of one buffer"
        assert all(torch.equal(a, b) for a, b in zip(listed, from_raw))
        n_tie, high = 0, 0
        for img, out, lab in zip(imgs, outs, listed):
            want, gap = ser.rescale_labels(seg.encode_decode(img[None])[0].cpu(), out[0], out[1])
            tie = gap < TIE
            n_tie += int(tie.sum())
            high += int((want > 255).sum())
            assert bool((from_i16(lab.cpu()) == want)[~tie].all()), "labels differ from the fp64 rescaling"
            assert int(tie.sum()) <= CAP * tie.numel()
        print(f"predict_list: {n_tie} rescaled gaps below 1e-6 in {sum(a * b for a, b in outs)} output pixels, {high} labels above 255")
        assert high > 0, "the case does not reach the high label byte"
        # SegEvaluator.update_raw + compute against the reference's areas of the returned labels
        gts = []
        for i, lab in enumerate(listed):
            gt = swc.synthetic_gt(from_i16(lab.cpu())[None], C, 60 + i)[0]
            gts.append(to_i16(gt).to(DEV))
        want_areas = sum(ser.areas(from_i16(l.cpu()), from_i16(g.cpu()), C, 65535) for l, g in zip(listed, gts))
        ev = SegEvaluator(seg, ignore_index=65535)
        labels = ev.update_raw(raws, gts, tf, return_labels=True)
        assert all(torch.equal(a, b) for a, b in zip(labels, listed))
        assert tuple(ev.areas.shape) == (3, C) and torch.equal(ev.areas.cpu(), want_areas)
        assert ev.compute()["mIoU"] == pytest.approx(ser.metrics(want_areas)["mIoU"], abs=1e-12)
        # the same call enqueues only: no host synchronisation before compute()
        ev.reset()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            assert ev.update_raw(raws, gts, tf) is None
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(ev.areas.cpu(), want_areas)
        ev2 = SegEvaluator(seg, ignore_index=65535)
        ev2.update(imgs, gts)
        assert torch.equal(ev2.areas.cpu(), want_areas)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_eval_epoch_int16():
    """eval_epoch(test_cfg={"label_dtype": torch.int16, "ignore_index": 65535}) with int16 ground truths = 100 * the reference's
    mIoU of the areas of the labels that predict_list returns for the same class prompts."""
    try:
        model = tiny_seg_model()
        spec = synth.SPECS["tiny"]
        tokens = synth.synthetic_batch(spec, 300, seed=78)["input_ids"][:, 0].view(300, 1, -1)
        cfg = dict(bg_thresh=0.0, label_dtype=torch.int16, **SLIDE)
        seg = SegInference(model, build_text_embedding(model, tokens.to(DEV)), True, **cfg)
        C = seg.num_classes
        gen = torch.Generator().manual_seed(7)
        batches, want = [], torch.zeros(3, C, dtype=torch.long)
        for k, sizes in enumerate([[(96, 120), (64, 64)], [(100, 70)]]):
            imgs = [torch.randn(3, h, w, generator=gen) for (h, w) in sizes]
            outs = [(h + 30, w + 21) for (h, w) in sizes]
            labels = [from_i16(t.cpu()) for t in seg.predict_list([t.to(DEV) for t in imgs], outs)]
            gts = [swc.synthetic_gt(lab[None], C, 50 + k)[0] for lab in labels]
            want += sum(ser.areas(lab, gt, C, 65535, True) for lab, gt in zip(labels, gts))
            batches.append((imgs, [to_i16(gt) for gt in gts]))
        model.train()   # eval_epoch switches to eval mode itself
        got = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(cfg, ignore_index=65535, reduce_zero_label=True))
        assert not model.training
        print(f"eval_epoch: {got:.6f}, reference {100 * ser.metrics(want)['mIoU']:.6f}")
        assert 0.0 < got < 100.0
        assert got == pytest.approx(100.0 * ser.metrics(want)["mIoU"], abs=1e-9)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
