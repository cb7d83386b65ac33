"""GPU: the zero-shot segmentation evaluation - segclip_seg_label_map_rescaled / segclip_seg_areas (csrc/segment_eval.inc),
SegInference.predict_list, SegEvaluator and train.eval_epoch - against tests/seg_eval_reference.py (fp64).  Rescale-then-
arg-max, intersect_and_union and eval_metrics are mmseg behaviour restated from its description (see that module).

Near-ties.  A rescaled label may legitimately differ from the fp64 yardstick where fp32 cannot resolve the decision.  A
differing pixel is accepted only as a VERIFIED near-tie: (a) one of its source taps is a near-tie by the rule of
tests/test_seg_gpu.py (group gap < 1e-6, or class gap < 1e-6 under overlapping windows), or (b) its own rescaled top-two class
gap is < 1e-6.  Near-ties may be at most 0.05 % of a case's output pixels (a fixed condition: a seed whose reference alone
exceeds it is replaced).  The cap is wider than the 0.01 % of the network-size test because one source near-tie reaches up to
about 4 * (oh / H) * (ow / W) output pixels.  NEAR_TIE_COUNTS holds the counts of the fp64 reference alone and the number of
pixels where the fp32 reference differs from it (CPU: `python -m tests.test_seg_eval_gpu`).

The end-to-end checks compare predict_list with the fp64 rescaling of THIS build's encode_decode logits, in which the groups
are already decided: there a near-tie is a rescaled gap below the bound alone.  Counted on an MI355X: see the tests.
"""
import math

import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import config, ops
from segclip_amd.segmentation import SegEvaluator, SegInference
from segclip_amd.train import eval_epoch
from tests import seg_eval_reference as ser
from tests import seg_reference as sr
from tests.helpers import load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8 = 0xA5
TIE, CAP = 1e-6, 5e-4
G, GRID, CC, LOG_SCALE = 8, (14, 14), 32, 3.0

# name: (mode, stride, B, (H, W), (oh, ow), N, with_bg, bg_thresh, seed)
CASES = {
    "voc": ("slide", 224, 2, (224, 299), (375, 500), 20, True, 0.8, 11),
    "context_tall": ("slide", 224, 1, (299, 224), (500, 375), 59, True, 0.25, 12),
    "whole": ("whole", 0, 2, (224, 224), (333, 500), 20, True, 0.65, 13),
    "downscale": ("whole", 0, 1, (224, 224), (100, 181), 5, False, 0.0, 14),
    "identity": ("whole", 0, 1, (224, 224), (224, 224), 20, True, 0.8, 15),
    "x2": ("whole", 0, 1, (224, 224), (448, 448), 20, True, 0.8, 16),
    "x1.5": ("whole", 0, 1, (224, 224), (336, 336), 20, True, 0.8, 17),
    "slide112": ("slide", 112, 1, (300, 340), (441, 500), 20, True, 0.8, 18),
    # every (window, group) has a dominant class of its own: 4 windows x 8 groups over 20 classes
    "many_classes": ("slide", 224, 2, (224, 299), (375, 500), 20, True, 0.8, 19),
}
# name: (output pixels, near-ties of the fp64 reference, pixels where the fp32 reference's label differs, distinct labels)
NEAR_TIE_COUNTS = {
    "voc": (375000, 0, 0, 5),
    "context_tall": (187500, 62, 0, 3),
    "whole": (333000, 12, 0, 3),
    "downscale": (18100, 1, 0, 4),
    "identity": (50176, 0, 0, 2),
    "x2": (200704, 0, 0, 2),
    "x1.5": (112896, 0, 0, 2),
    "slide112": (220500, 0, 0, 7),
    "many_classes": (375000, 12, 0, 16),
}


def _soft(seed, nW, G, gh, gw):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.softmax(torch.randn(nW, G, gh, gw, generator=g) * (1.0 + seed % 4), dim=1)


def _features(seed, nW, G, N, Cc):
    g = torch.Generator().manual_seed(2000 + seed)
    gt, pf = torch.randn(nW, G, Cc, generator=g), torch.randn(nW, Cc, generator=g)
    tx = torch.randn(N, Cc, generator=g)
    return gt, pf, tx / tx.norm(dim=-1, keepdim=True)


def _f32_tables(table):
    """A table rounded to fp32 and everything derived from it exactly (both sides then read the same numbers)."""
    t = table.float()
    score, cls = t.max(dim=-1)
    return dict(table=t, table_max=t.amax(dim=(1, 2)), best_class=cls, best_score=score)


def _dev_tables(t32):
    return (t32["table"].to(DEV), t32["table_max"].to(DEV), t32["best_class"].int().to(DEV), t32["best_score"].to(DEV))


def _case(name):
    """-> dict(soft, t32, wins, win, ...) of a case, all on the CPU."""
    mode, stride, B, (H, W), out, N, with_bg, thr, seed = CASES[name]
    wins, win = sr.window_list(B, H, W, mode, (224, 224), (stride, stride))
    nW = len(wins)
    soft = _soft(seed, nW, G, *GRID)
    if name == "many_classes":
        g = torch.Generator().manual_seed(2000 + seed)
        table = torch.rand(nW, G, N, generator=g, dtype=torch.float64) * 0.1
        for k in range(nW):
            for j in range(G):
                table[k, j, (k * G + j) * 7 % N] = 0.82 + 0.15 * float(torch.rand((), generator=g))
        table[:, ::4] *= 0.5      # every fourth group falls under the background threshold
    else:
        gt, pf, tx = _features(seed, nW, G, N, CC)
        table = sr.group_table(gt, pf, tx, LOG_SCALE, min(5, N))["table"]
    return dict(name=name, B=B, net=(H, W), out=out, N=N, with_bg=with_bg, thr=thr, wins=wins, win=win, soft=soft,
                t32=_f32_tables(table), per=nW // B)


def _reference(case, dtype=torch.float64):
    """fp64 labels at the output size, the near-tie mask, the network-size assembly."""
    B, (H, W), (oh, ow) = case["B"], case["net"], case["out"]
    ref = sr.assemble(case["soft"], case["t32"], case["wins"], (B, H, W), case["win"], case["with_bg"], case["thr"], dtype)
    labels, gap = ser.rescale_labels(ref["logits"], oh, ow, dtype)
    src_tie = (ref["group_gap"] < TIE) | ((ref["count"] > 1) & (ref["class_gap"] < TIE))
    return labels, ser.spread(src_tie, oh, ow) | (gap < TIE), ref


def _image_rows(case, gt_offsets=None):
    gh, gw = GRID
    return [dict(first=b * case["per"], count=case["per"], net=case["net"], out=case["out"], win=case["win"], grid=GRID,
                 soft_off=b * case["per"] * G * gh * gw, gt_off=-1 if gt_offsets is None else gt_offsets[b])
            for b in range(case["B"])]


def _run_rescaled(case, gt=None, reduce_zero=False, pad=64):
    """The kernel through a framed label buffer, launched twice (labels and areas bit-equal), frames checked.
    -> labels (B, oh, ow) long on the CPU, areas (3, C) long or None."""
    B, (oh, ow) = case["B"], case["out"]
    C = case["N"] + int(case["with_bg"])
    offs = None if gt is None else [b * oh * ow for b in range(B)]
    images, lab_offs, nbytes, n_blocks, most = ops.seg_image_table(_image_rows(case, offs), DEV)
    dwin = torch.tensor(case["wins"], dtype=torch.int32, device=DEV).view(-1, 3)
    soft, tabs = case["soft"].reshape(-1).to(DEV), _dev_tables(case["t32"])
    gt_dev = None if gt is None else gt.to(torch.uint8).reshape(-1).to(DEV)
    res = []
    for _ in range(2):
        buf = torch.full((nbytes + 2 * pad,), SENT8, dtype=torch.uint8, device=DEV)
        view = buf[pad:pad + nbytes]
        areas = None if gt is None else torch.zeros(3, C, dtype=torch.int64, device=DEV)
        ops.seg_label_map_rescaled(soft, tabs, dwin, images, n_blocks, most, case["with_bg"], case["thr"], labels=view, gt=gt_dev,
                                   areas=areas, ignore_index=255, reduce_zero_label=reduce_zero)
        torch.cuda.synchronize()
        assert bool((buf[:pad] == SENT8).all()) and bool((buf[pad + nbytes:] == SENT8).all()), "the kernel wrote outside its output"
        for b, o in enumerate(lab_offs):   # the padding between two images is not written either
            end = lab_offs[b + 1] if b + 1 < B else nbytes
            assert bool((view[o + oh * ow:end] == SENT8).all())
        labels = torch.stack([view[o:o + oh * ow].view(oh, ow) for o in lab_offs]).cpu().long()
        res.append((labels, None if areas is None else areas.cpu()))
    assert torch.equal(res[0][0], res[1][0]), "repeat launch differs"
    if gt is not None:
        assert torch.equal(res[0][1], res[1][1]), "repeat launch: areas differ"
    return res[0]


# ------------------------------------------------------------------------------------------------ 1. kernel against fp64
@pytest.mark.parametrize("name", list(CASES))
def test_rescaled_labels_against_reference(name):
    case = _case(name)
    want, tie, _ = _reference(case)
    n_tie = int(tie.sum())
    got, _ = _run_rescaled(case, pad=64 if CASES[name][-1] % 2 else 3)
    print(f"{name}: {tie.numel()} output pixels, {n_tie} near-ties, labels differ at {int((got != want).sum())}, "
          f"{got.unique().numel()} distinct labels")
    assert (tie.numel(), n_tie) == NEAR_TIE_COUNTS[name][:2], "the reference's own count changed"
    assert n_tie <= CAP * tie.numel(), f"{name}: {n_tie} near-ties of {tie.numel()} pixels in the reference itself"
    assert bool((got == want)[~tie].all()), f"{name}: labels differ away from near-ties"
    if name == "many_classes":
        assert got.unique().numel() >= 10


@pytest.mark.parametrize("name", ["identity", "voc", "slide112", "many_classes"])
def test_identity_equals_label_map(name):
    """(oh, ow) == (H, W): every lambda is 0 and the result is segclip_seg_label_map's, bit for bit (whole and slide)."""
    case = _case(name)
    case["out"] = case["net"]
    got, _ = _run_rescaled(case)
    B, (H, W) = case["B"], case["net"]
    dwin = torch.tensor(case["wins"], dtype=torch.int32, device=DEV).view(-1, 3)
    dfirst = torch.arange(0, len(case["wins"]) + 1, case["per"], dtype=torch.int32, device=DEV)
    soft = case["soft"].reshape(len(case["wins"]), G, -1).to(DEV)
    merged = ops.seg_label_map(soft, _dev_tables(case["t32"]), dwin, dfirst, (B, H, W), case["win"], GRID, case["with_bg"],
                               case["thr"])[0]
    assert torch.equal(got, merged.cpu().long())


# ------------------------------------------------------------------------------------------------ 2. areas
def _synthetic_gt(want, C, seed):
    """The reference's labels with random rectangles relabelled, a band of 255 and a few values >= C."""
    g = torch.Generator().manual_seed(seed)
    gt = want.clone()
    B, oh, ow = gt.shape
    for _ in range(12):
        b, y, x = int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, oh - 20, (1,), generator=g)), \
            int(torch.randint(0, ow - 20, (1,), generator=g))
        h, w = int(torch.randint(5, oh // 3, (1,), generator=g)), int(torch.randint(5, ow // 3, (1,), generator=g))
        gt[b, y:y + h, x:x + w] = int(torch.randint(0, C, (1,), generator=g))
    gt[:, oh // 2:oh // 2 + 9, :] = 255
    gt[:, 3:7, 5:40] = C + 3
    gt[:, -1, -5:] = C
    return gt


@pytest.mark.parametrize("name", ["voc", "context_tall", "whole", "many_classes"])
@pytest.mark.parametrize("reduce_zero", [False, True])
def test_areas(name, reduce_zero):
    case = _case(name)
    C = case["N"] + int(case["with_bg"])
    want, tie, _ = _reference(case)
    gt = _synthetic_gt(want, C, 77)
    labels, areas = _run_rescaled(case, gt=gt, reduce_zero=reduce_zero)
    lab8, gt8 = labels.to(torch.uint8).to(DEV), gt.to(torch.uint8).to(DEV)
    alone = ops.seg_areas(lab8, gt8, C, 255, reduce_zero)
    again = ops.seg_areas(lab8, gt8, C, 255, reduce_zero)
    torch.cuda.synchronize()
    assert torch.equal(alone, again)
    assert torch.equal(areas, alone.cpu()), "the fused counters differ from segclip_seg_areas on the kernel's own labels"
    assert torch.equal(areas, ser.areas(labels, gt, C, 255, reduce_zero)), "areas differ from the reference on the same labels"
    ref_areas = ser.areas(want, gt, C, 255, reduce_zero)
    n_tie = int(tie.sum())
    print(f"{name} reduce_zero={reduce_zero}: largest difference to the fp64 labels' areas {int((areas - ref_areas).abs().max())}, "
          f"{n_tie} near-ties")
    assert int((areas - ref_areas).abs().max()) <= n_tie
    ignored = (gt == 255) | ((gt == 0) if reduce_zero else torch.zeros_like(gt, dtype=torch.bool))
    assert int(areas[1].sum()) == int((~ignored).sum())
    assert int(areas[0].sum()) > 0 and bool((areas[0] <= areas[1]).all()) and bool((areas[0] <= areas[2]).all())
    # seg_areas adds to a tensor it is given
    twice = ops.seg_areas(lab8, gt8, C, 255, reduce_zero, areas=alone.clone())
    assert torch.equal(twice, 2 * alone)


def test_kernel_limits():
    case = _case("identity")
    images, _, nbytes, n_blocks, most = ops.seg_image_table(_image_rows(case), DEV)
    dwin = torch.tensor(case["wins"], dtype=torch.int32, device=DEV).view(-1, 3)
    labels = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    wide = _f32_tables(torch.rand(1, G, 256, dtype=torch.float64))
    with pytest.raises(L.Unsupported):   # 256 classes + background
        ops.seg_label_map_rescaled(case["soft"].reshape(-1).to(DEV), _dev_tables(wide), dwin, images, n_blocks, most, True, 0.5,
                                   labels=labels)
    with pytest.raises(L.Unsupported):   # 65 windows per image
        ops.seg_label_map_rescaled(case["soft"].reshape(-1).to(DEV), _dev_tables(case["t32"]), dwin, images, n_blocks, 65, True, 0.5,
                                   labels=labels)
    with pytest.raises(L.Unsupported):
        ops.seg_areas(labels, labels, 257)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_areas(labels.cpu(), labels.cpu(), 21)


# ------------------------------------------------------------------------------------------------ 3. end to end
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
# network sizes: square, tall, wide, wide (mmcv test sizes of 300 x 300, 500 x 375, 375 x 500 and 281 x 500 images)
RAGGED = [((224, 224), (300, 300)), ((299, 224), (500, 375)), ((224, 299), (375, 500)), ((224, 399), (281, 500))]


def _ragged_images(seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, H, W, generator=g).to(DEV) for (H, W), _ in RAGGED], [o for _, o in RAGGED]


def _e2e_reference(seg, img, out):
    """fp64 rescaling of this build's encode_decode logits of one image -> labels, rescaled top-two gap."""
    logits = seg.encode_decode(img[None])[0].cpu()
    return ser.rescale_labels(logits, out[0], out[1])


def test_ragged_list_end_to_end():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        imgs, outs = _ragged_images()
        seg = SegInference(model, emb, True, bg_thresh=0.03, **SLIDE)
        total = sum(len(sr.slide_windows(H, W, SLIDE["crop_size"], SLIDE["stride"])) for (H, W), _ in RAGGED)
        calls = []
        real = model.clip.encode_image

        def counted(*a, **k):
            calls.append(a[0].shape[0])
            return real(*a, **k)

        model.clip.encode_image = counted
        try:
            together = seg.predict_list(imgs, outs)
            assert len(calls) == 1 and calls[0] == total
            for mw in (1, 3, 256):
                del calls[:]
                chunked = SegInference(model, emb, True, bg_thresh=0.03, max_windows=mw, **SLIDE).predict_list(imgs, outs)
                assert len(calls) == math.ceil(total / mw), (mw, calls)
                assert all(torch.equal(a, b) for a, b in zip(chunked, together)), f"max_windows={mw} differs"
        finally:
            del model.clip.encode_image
        assert [tuple(t.shape) for t in together] == outs and all(t.dtype == torch.uint8 for t in together)
        n_tie = 0
        for i, (img, out) in enumerate(zip(imgs, outs)):
            assert torch.equal(seg.predict_list([img], [out])[0], together[i]), f"image {i} alone differs"
            want, gap = _e2e_reference(seg, img, out)
            tie = gap < TIE
            n_tie += int(tie.sum())
            assert bool((together[i].cpu().long() == want)[~tie].all()), f"image {i}: labels differ from the fp64 rescaling"
            assert int(tie.sum()) <= CAP * tie.numel()
        print(f"ragged list: {n_tie} rescaled gaps below 1e-6 in {sum(a * b for a, b in outs)} output pixels")
        # default output shapes = the images' own sizes = predict
        own = seg.predict_list(imgs[:1])[0]
        assert torch.equal(own, seg.predict(imgs[0][None])[0])
        # shuffling permutes the outputs and leaves the areas alone; one image at a time gives the same areas
        gts = [torch.randint(0, 14, o, generator=torch.Generator().manual_seed(9 + i)).to(torch.uint8).to(DEV) for i, o in enumerate(outs)]
        for t in gts:
            t[5:9] = 255
        ev = SegEvaluator(seg)
        assert ev.update(imgs, gts) is None
        perm = [2, 0, 3, 1]
        shuffled = seg.predict_list([imgs[i] for i in perm], [outs[i] for i in perm])
        assert all(torch.equal(shuffled[k], together[i]) for k, i in enumerate(perm))
        ev2 = SegEvaluator(seg)
        labels = ev2.update([imgs[i] for i in perm], [gts[i] for i in perm], return_labels=True)
        assert all(torch.equal(labels[k], together[i]) for k, i in enumerate(perm))
        ev3 = SegEvaluator(seg)
        for img, t in zip(imgs, gts):
            ev3.update([img], [t])
        assert torch.equal(ev.areas, ev2.areas) and torch.equal(ev.areas, ev3.areas)
        want = sum(ser.areas(together[i].cpu(), gts[i].cpu(), seg.num_classes) for i in range(len(imgs)))
        assert torch.equal(ev.areas.cpu(), want)
        assert ev.compute()["mIoU"] == pytest.approx(ser.metrics(want)["mIoU"], abs=1e-12)
        ev.reset()
        assert int(ev.areas.abs().sum()) == 0
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("mode", ["whole", "slide"])
def test_predict_list_equals_predict_on_a_batch(mode):
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        gen = torch.Generator().manual_seed(5)
        kw = dict(mode="slide", crop_size=(64, 64), stride=(48, 40)) if mode == "slide" else {}
        image = (torch.randn(3, 3, 100, 150, generator=gen) if mode == "slide" else torch.randn(3, 3, 128, 128, generator=gen)).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.03, **kw)
        batch = seg.predict(image)
        listed = seg.predict_list(list(image))
        assert all(torch.equal(listed[b], batch[b]) for b in range(3))
        if mode == "whole":   # two sizes in one call: one tower call per size, the outputs in the caller's order
            small = torch.randn(3, 64, 64, generator=gen).to(DEV)
            mixed = seg.predict_list([image[0], small, image[1]])
            assert torch.equal(mixed[0], batch[0]) and torch.equal(mixed[2], batch[1])
            assert torch.equal(mixed[1], seg.predict(small[None])[0])
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


# counted on the CPU from the golden alone: its source pixels with a group gap below 1e-4 (7 and 1 of 32 768) reach 51 and 9 of
# 69 200 output pixels at the sizes below; together with the rescaled gaps of the golden's logits below 1e-4: at most 90 and
# 10 of 69 200 (0.13 %, 0.014 %) over the six class-list cases
GOLDEN_OUT = [(200, 173), (346, 100)]


def test_against_reference_golden():
    """The golden images through encode_decode (the path pinned to the real reference), those logits through the fp64
    rescaling, against predict_list.  Rule of the end-to-end test of tests/test_seg_gpu.py: near-tie = a source tap whose
    winning group has a gap below 1e-4 in the golden's own soft_attn, or a rescaled gap below 1e-4; at most 0.25 % of a
    case's output pixels (one source near-tie reaches up to 4 * (oh / H) * (ow / W) output pixels: 7 of 32 768 source pixels
    stay below the cap)."""
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        for si, (H, W) in enumerate(g["sizes"].tolist()):
            image = torch.from_numpy(g[f"image_{si}"]).to(DEV)
            soft = torch.from_numpy(g[f"soft_{si}"])
            _, ggap = sr.window_groups(soft.view(soft.shape[0], -1, H // 16, W // 16), H, W)
            oh, ow = GOLDEN_OUT[si]
            for ci, (with_bg, N, thr) in enumerate(g["cases"].tolist()):
                seg = SegInference(model, emb[:int(N)], bool(with_bg), bg_thresh=thr)
                want, gap = ser.rescale_labels(seg.encode_decode(image).cpu(), oh, ow)
                tie = ser.spread(ggap < 1e-4, oh, ow) | (gap < 1e-4)
                got = torch.stack(seg.predict_list(list(image), [(oh, ow)] * image.shape[0])).cpu().long()
                print(f"golden {H}x{W} -> {oh}x{ow} case {ci}: {int(tie.sum())} near-ties of {tie.numel()}, labels differ at "
                      f"{int((got != want).sum())}")
                assert int(tie.sum()) <= 2.5e-3 * tie.numel()
                assert bool((got == want)[~tie].all())
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_update_allocates_less_than_one_fp32_plane_per_image():
    """SegEvaluator.update on one 224 x 299 -> 375 x 500 image with 21 classes: the peak beyond the towers' own (encode_image
    on the stacked windows, the stack included) stays below one fp32 plane of the output: no (C, oh, ow) tensor exists."""
    try:
        model = tiny_seg_model()
        gen = torch.Generator().manual_seed(8)
        emb = torch.randn(20, 64, generator=gen)
        emb = (emb / emb.norm(dim=-1, keepdim=True)).to(DEV)
        img = torch.randn(3, 224, 299, generator=gen).to(DEV)
        gt = torch.randint(0, 21, (375, 500), generator=gen).to(torch.uint8).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.03, **SLIDE)
        ev = SegEvaluator(seg)
        wins = sr.slide_windows(224, 299, SLIDE["crop_size"], SLIDE["stride"])

        def towers():
            with torch.no_grad(), config.scope(cross_mode="intended"):
                x = torch.stack([img[:, y:y + 128, x0:x0 + 128] for (y, x0) in wins])
                return model.clip.encode_image(x, return_hidden=True)

        def peak(fn):
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            p = torch.cuda.max_memory_allocated() - base
            del out
            return p

        p_enc, p_upd = peak(towers), peak(lambda: ev.update([img], [gt]))
        plane = 4 * 375 * 500
        print(f"towers' peak {p_enc} bytes, update peak {p_upd} bytes, one fp32 plane {plane} bytes")
        assert p_upd - p_enc < plane
        assert int(ev.areas[1].sum()) == 2 * 375 * 500
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_interface_errors():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        seg = SegInference(model, emb, True, **SLIDE)
        img = torch.zeros(3, 160, 160, device=DEV)
        gt = torch.zeros(200, 200, dtype=torch.uint8, device=DEV)
        ev = SegEvaluator(seg)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            seg.predict_list([img.cpu()])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ev.update([img], [gt.cpu()])
        with pytest.raises(ValueError, match="smaller than the crop"):
            seg.predict_list([img, torch.zeros(3, 100, 200, device=DEV)])
        with pytest.raises(ValueError, match="output shapes"):
            seg.predict_list([img, img], [(200, 200)])
        with pytest.raises(ValueError, match="ground truths"):
            ev.update([img, img], [gt])
        with pytest.raises(ValueError, match="uint8"):
            ev.update([img], [gt.float()])
        with pytest.raises(ValueError, match="uint8"):
            ev.update([img], [gt[None]])   # a ground truth whose shape is not an (oh, ow) output shape
        gen = torch.Generator().manual_seed(3)
        wide = torch.randn(256, emb.shape[1], generator=gen)
        wide = (wide / wide.norm(dim=-1, keepdim=True)).to(DEV)
        with pytest.raises(L.Unsupported):
            SegInference(model, wide, True, **SLIDE).predict_list([img])
        assert int(ev.areas.abs().sum()) == 0
        model.train()
        with pytest.raises(RuntimeError, match="model.eval"):
            seg.predict_list([img])
        model.eval()
        assert tuple(seg.predict_list([img], [(200, 200)])[0].shape) == (200, 200)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_eval_epoch():
    """eval_epoch on three synthetic batches = 100 * mIoU of the fp64 rescaling's areas.  Where rescaled gaps below 1e-6
    exist, n such pixels move a class's I, P and L by at most n each, hence its IoU = I / U by at most 2 n / (U - n)."""
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        tokens = torch.from_numpy(g["prompt_ids"])
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        cfg = dict(bg_thresh=0.03, **SLIDE)
        seg = SegInference(model, emb, True, **cfg)
        C = seg.num_classes
        batches, ref_areas, n_tie = [], torch.zeros(3, C, dtype=torch.long), 0
        for k in range(3):
            imgs, outs = _ragged_images(seed=20 + k)
            imgs, outs = imgs[:2 + k % 2], outs[:2 + k % 2]
            gts = []
            for img, out in zip(imgs, outs):
                want, gap = _e2e_reference(seg, img, out)
                n_tie += int((gap < TIE).sum())
                gt = _synthetic_gt(want[None], C, 50 + k)[0]
                ref_areas += ser.areas(want, gt, C)
                gts.append(gt.to(torch.uint8))
            batches.append(([t.cpu() for t in imgs], gts))
        ref = ser.metrics(ref_areas)
        union = ref_areas[1] + ref_areas[2] - ref_areas[0]
        present = union > 0
        per_class = torch.where(union > n_tie, 2.0 * n_tie / (union - n_tie).clamp_min(1).double(), torch.ones(C, dtype=torch.float64))
        margin = 100.0 * float(per_class[present].mean()) if n_tie else 1e-9
        model.train()   # eval_epoch switches to eval mode itself
        got = eval_epoch(None, model, DEV, 1, batches, tokens, True, cfg)
        assert not model.training
        print(f"eval_epoch: {got:.6f}, reference {100 * ref['mIoU']:.6f}, {n_tie} near-ties, margin {margin:.3e}")
        assert 0.0 < got < 100.0
        assert abs(got - 100.0 * ref["mIoU"]) <= margin
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def _reference_counts():
    """CPU: the NEAR_TIE_COUNTS table."""
    for name in CASES:
        case = _case(name)
        want, tie, _ = _reference(case)
        l32, _, _ = _reference(case, torch.float32)
        print(f'"{name}": ({tie.numel()}, {int(tie.sum())}, {int((l32 != want).sum())}, {want.unique().numel()}),', flush=True)
    g = load_golden("seg_tiny.npz")
    for si, (H, W) in enumerate(g["sizes"].tolist()):
        soft = torch.from_numpy(g[f"soft_{si}"])
        _, ggap = sr.window_groups(soft.view(soft.shape[0], -1, H // 16, W // 16), H, W)
        oh, ow = GOLDEN_OUT[si]
        src = ser.spread(ggap < 1e-4, oh, ow)
        for ci in range(len(g["cases"])):
            _, gap = ser.rescale_labels(torch.from_numpy(g[f"logits_{si}_{ci}"]), oh, ow)
            print(f"golden {H}x{W} -> {oh}x{ow} case {ci}: source near-ties reach {int(src.sum())}, with rescaled gaps below 1e-4 "
                  f"{int((src | (gap < 1e-4)).sum())} of {src.numel()}")


if __name__ == "__main__":
    _reference_counts()
