"""GPU: flip and multi-scale test-time augmentation - segclip_seg_label_map_views / segclip_seg_view_probs
(csrc/segment_aug.inc), segclip_seg_view_windows_from_u8, SegInference.predict_raw(aug=) / predict_views / predict_proba_*,
SegEvaluator.update_raw(aug=) / update_views and eval_epoch(test_cfg={"aug": ...}) - against tests/seg_aug_reference.py (fp64).

Kernel cases: synthetic soft_attn and tables as tests/test_seg_eval_gpu.py builds them (G = 8, grid 14 x 14, windows
224 x 224), every view with data of its own.

Tolerance.  PROB_DIFF_F32 is the largest absolute difference of the mean probabilities between the fp32 and the fp64
restatement of the same operation order over all cases, measured on the CPU away from source near-ties (there the two may
pick different groups, which moves a probability by up to 1): `python -m tests.test_seg_aug_gpu`.  The dense entry is held
to PROB_TOL = 4 x that figure (headroom for the device's expf), away from source near-ties.

Near-ties.  A label may differ from the fp64 yardstick only at a VERIFIED near-tie: (a) a source tap of any view is one by
the rule of tests/test_seg_eval_gpu.py (group gap < 1e-6, or class gap < 1e-6 under overlapping windows), spread to the output
and mirrored back, or (b) the pixel's fp64 top-two gap of the mean probabilities is below PROB_TOL.  At most 0.2 % of a
case's output pixels (0.05 % per view x the four views of the largest case; a fixed condition).  NEAR_TIE_COUNTS holds the
fp64 reference's own counts.
"""
import functools

import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import config, ops
from segclip_amd.segmentation import ImageTransform, SegEvaluator, SegInference, TestAug, preprocess
from segclip_amd.train import eval_epoch
from tests import seg_aug_reference as sar
from tests import seg_eval_reference as ser
from tests import seg_frontend_reference as sfr
from tests import seg_reference as sr
from tests.helpers import load_golden, tiny_seg_model
from tests.test_seg_eval_gpu import _f32_tables, _dev_tables, _features, _soft, _synthetic_gt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8 = 0xA5
TIE, CAP = 1e-6, 2e-3
G, GRID, CC, LOG_SCALE = 8, (14, 14), 32, 3.0
PROB_DIFF_F32 = 2.036e-6   # measured, see the module docstring and _reference_counts
PROB_TOL = 4 * PROB_DIFF_F32
FE_TOL = 5e-6            # tests/test_seg_frontend_gpu.py

W224, S224, S112 = ("whole", 0), ("slide", 224), ("slide", 112)
# name: (N, with_bg, bg_thresh, seed, images [((oh, ow), views [((mode, stride), (H, W), flags)])])
CASES = {
    "one_view": (20, True, 0.8, 31, [((150, 200), [(W224, (224, 224), 0)])]),
    "hflip_whole": (20, True, 0.8, 32, [((150, 200), [(W224, (224, 224), 0), (W224, (224, 224), 1)])] * 2),
    "vflip": (20, True, 0.65, 33, [((160, 150), [(W224, (224, 224), 0), (W224, (224, 224), 2)])]),
    "two_ratios": (20, True, 0.8, 34, [((150, 200), [(S224, (224, 299), 0), (S224, (224, 299), 1), (S224, (336, 448), 0),
                                                    (S224, (336, 448), 1)])]),
    "slide112": (20, True, 0.8, 35, [((147, 167), [(S112, (300, 340), 0), (S112, (300, 340), 1)])]),
    "context59": (59, True, 0.25, 36, [((150, 200), [(W224, (224, 224), 0), (W224, (224, 224), 1)])]),
    "five_no_bg": (5, False, 0.0, 37, [((100, 181), [(W224, (224, 224), 0), (W224, (224, 224), 1)])]),
    # an odd width (the mirror has no centre column pair) and an output narrower than one dword
    "odd_narrow": (20, True, 0.8, 38, [((150, 201), [(W224, (224, 224), 0), (W224, (224, 224), 1)]),
                                       ((151, 3), [(W224, (224, 224), 0), (W224, (224, 224), 3)])]),
    "v16": (20, True, 0.8, 39, [((60, 80), [(W224, (224, 224), k % 4) for k in range(16)])]),
    # more classes than one accumulator chunk holds beside the overlap lists: the (maximum, sum) of a view kept in LDS
    "chunked": (255, True, 0.25, 40, [((40, 50), [(S112, (300, 340), 0), (S112, (300, 340), 1)])]),
}
# name: (output pixels, near-ties of the fp64 reference, pixels where the fp32 restatement's label differs)
NEAR_TIE_COUNTS = {
    "one_view": (30000, 0, 0),   # fp32 - fp64 probabilities 1.042e-06
    "hflip_whole": (60000, 4, 0),   # fp32 - fp64 probabilities 7.068e-07
    "vflip": (24000, 1, 0),   # fp32 - fp64 probabilities 4.964e-07
    "two_ratios": (30000, 0, 0),   # fp32 - fp64 probabilities 4.380e-07
    "slide112": (24549, 1, 0),   # fp32 - fp64 probabilities 7.634e-07
    "context59": (30000, 0, 0),   # fp32 - fp64 probabilities 1.703e-07
    "five_no_bg": (18100, 0, 0),   # fp32 - fp64 probabilities 2.036e-06
    "odd_narrow": (30603, 0, 0),   # fp32 - fp64 probabilities 8.474e-07
    "v16": (4800, 1, 0),   # fp32 - fp64 probabilities 7.961e-08
    "chunked": (2000, 0, 0),   # fp32 - fp64 probabilities 2.856e-08
}


def _case(name):
    """-> dict of a case on the CPU: the global window list (image column = view entry), per view its soft_attn and tables."""
    N, with_bg, thr, seed, images = CASES[name]
    views, wins_all, k = [], [], 0
    for i, (out, per) in enumerate(images):
        for v, ((mode, stride), (H, W), flags) in enumerate(per):
            wins, win = sr.window_list(1, H, W, mode, (224, 224), (stride, stride))
            nW = len(wins)
            soft = _soft(seed + 7 * k, nW, G, *GRID)
            gt, pf, tx = _features(seed + 7 * k, nW, G, N, CC)
            t32 = _f32_tables(sr.group_table(gt, pf, tx, LOG_SCALE, min(5, N))["table"])
            views.append(dict(image=i, net=(H, W), flags=flags, wins=wins, win=win, soft=soft, t32=t32, first=len(wins_all), out=out))
            wins_all += [(k, y, x) for (_, y, x) in wins]
            k += 1
    return dict(name=name, N=N, with_bg=with_bg, thr=thr, views=views, wins=wins_all, outs=[o for o, _ in images],
                counts=[len(per) for _, per in images])


@functools.lru_cache(maxsize=None)
def _reference(name, dtype=torch.float64):
    """Per image: (mean probabilities (C, oh, ow), labels, near-tie mask, source near-tie mask).  Computed once per case."""
    case = _case(name)
    res, e = [], 0
    for i, V in enumerate(case["counts"]):
        oh, ow = case["outs"][i]
        logits, flags, src_tie = [], [], torch.zeros(oh, ow, dtype=torch.bool)
        for vw in case["views"][e:e + V]:
            H, W = vw["net"]
            ref = sr.assemble(vw["soft"], vw["t32"], vw["wins"], (1, H, W), vw["win"], case["with_bg"], case["thr"], dtype)
            logits.append(ref["logits"][0])
            flags.append(vw["flags"])
            tie = (ref["group_gap"][0] < TIE) | ((ref["count"][0] > 1) & (ref["class_gap"][0] < TIE))
            src_tie |= sar.spread_view(tie, oh, ow, vw["flags"])
        mean = sar.mean_probs(logits, flags, oh, ow, dtype)
        labels, gap = sar.labels_and_gap(mean)
        res.append((mean, labels, src_tie | (gap < PROB_TOL), src_tie))
        e += V
    return res


def _rows(case, images=None, gt=False):
    """The view rows of ops.seg_view_tables for all images of a case, or the listed ones."""
    gh, gw = GRID
    rows, counts, gt_off = [], [], 0
    soft_off = [0]
    for vw in case["views"]:
        soft_off.append(soft_off[-1] + vw["soft"].numel())
    for i, V in enumerate(case["counts"]):
        if images is not None and i not in images:
            continue
        for k, vw in enumerate(case["views"]):
            if vw["image"] == i:
                rows.append(dict(first=vw["first"], count=len(vw["wins"]), net=vw["net"], out=vw["out"], win=vw["win"], grid=GRID,
                                 soft_off=soft_off[k], gt_off=gt_off if gt else -1, flags=vw["flags"]))
        counts.append(V)
        gt_off += case["outs"][i][0] * case["outs"][i][1]
    return rows, counts


def _device_inputs(case):
    soft = torch.cat([vw["soft"].reshape(-1) for vw in case["views"]]).to(DEV)
    tabs = tuple(torch.cat([_dev_tables(vw["t32"])[j] for vw in case["views"]]) for j in range(4))
    dwin = torch.tensor(case["wins"], dtype=torch.int32, device=DEV).view(-1, 3)
    return soft, tabs, dwin


def _run_views(case, gts=None, reduce_zero=False, pad=64):
    """The label kernel through a framed buffer, launched twice (labels and areas bit-equal), frames checked.
    -> [labels (oh, ow) long on the CPU], areas (3, C) long or None."""
    C = case["N"] + int(case["with_bg"])
    rows, counts = _rows(case, gt=gts is not None)
    images, vtab, offs, nbytes, n_blocks, most_img, most_view, most_v = ops.seg_view_tables(rows, counts, DEV)
    soft, tabs, dwin = _device_inputs(case)
    gt_dev = None if gts is None else torch.cat([g.to(torch.uint8).reshape(-1) for g in gts]).to(DEV)
    res = []
    for _ in range(2):
        buf = torch.full((nbytes + 2 * pad,), SENT8, dtype=torch.uint8, device=DEV)
        view = buf[pad:pad + nbytes]
        areas = None if gts is None else torch.zeros(3, C, dtype=torch.int64, device=DEV)
        ops.seg_label_map_views(soft, tabs, dwin, images, vtab, n_blocks, most_img, most_view, most_v, case["with_bg"], case["thr"],
                                labels=view, gt=gt_dev, areas=areas, ignore_index=255, reduce_zero_label=reduce_zero)
        torch.cuda.synchronize()
        assert bool((buf[:pad] == SENT8).all()) and bool((buf[pad + nbytes:] == SENT8).all()), "the kernel wrote outside its output"
        for b, o in enumerate(offs):   # the padding between two images is not written either
            oh, ow = case["outs"][b]
            end = offs[b + 1] if b + 1 < len(offs) else nbytes
            assert bool((view[o + oh * ow:end] == SENT8).all())
        labels = [view[o:o + oh * ow].view(oh, ow).cpu().long() for o, (oh, ow) in zip(offs, case["outs"])]
        res.append((labels, None if areas is None else areas.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0])), "repeat launch differs"
    if gts is not None:
        assert torch.equal(res[0][1], res[1][1]), "repeat launch: areas differ"
    return res[0]


def _run_probs(case, i, pad=16):
    """The dense entry for image i through a framed buffer, launched twice -> (C, oh, ow) fp32 on the CPU."""
    C = case["N"] + int(case["with_bg"])
    oh, ow = case["outs"][i]
    rows, counts = _rows(case, images=[i])
    images, vtab, _, _, n_blocks, most_img, most_view, most_v = ops.seg_view_tables(rows, counts, DEV)
    soft, tabs, dwin = _device_inputs(case)
    res = []
    for _ in range(2):
        buf = torch.full((C * oh * ow + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
        out = buf[pad:pad + C * oh * ow]
        ops.seg_view_probs(soft, tabs, dwin, images, vtab, n_blocks, most_img, most_view, most_v, case["with_bg"], case["thr"], (oh, ow),
                           out=out)
        torch.cuda.synchronize()
        assert bool(buf[:pad].isnan().all()) and bool(buf[pad + C * oh * ow:].isnan().all()), "the kernel wrote outside its output"
        res.append(out.view(C, oh, ow).cpu())
    assert torch.equal(res[0], res[1]), "repeat launch differs"
    return res[0]


# ------------------------------------------------------------------------------------------------ 1. kernels against fp64
@pytest.mark.parametrize("name", list(CASES))
def test_views_against_reference(name):
    case = _case(name)
    ref = _reference(name)
    got, _ = _run_views(case, pad=64 if CASES[name][3] % 2 else 3)
    n_pix = sum(r[1].numel() for r in ref)
    n_tie = sum(int(r[2].sum()) for r in ref)
    worst = 0.0
    for i, (mean, want, tie, src_tie) in enumerate(ref):
        probs = _run_probs(case, i)
        assert bool(probs.isfinite().all())
        err = (probs.double() - mean).abs().amax(dim=0)
        worst = max(worst, float(err[~src_tie].max()))
        assert torch.equal(got[i], probs.argmax(dim=0)), f"{name} image {i}: the label is not the dense entry's first maximum"
        assert bool((got[i] == want)[~tie].all()), f"{name} image {i}: labels differ away from near-ties"
    print(f"{name}: {n_pix} output pixels, {n_tie} near-ties, labels differ at "
          f"{sum(int((g != r[1]).sum()) for g, r in zip(got, ref))}, largest probability error {worst:.3e} (tolerance {PROB_TOL:.3e})")
    assert (n_pix, n_tie) == NEAR_TIE_COUNTS[name][:2], "the reference's own count changed"
    assert n_tie <= CAP * n_pix, f"{name}: {n_tie} near-ties of {n_pix} pixels in the reference itself"
    assert worst <= PROB_TOL


def test_one_view_equals_rescaled_away_from_near_ties():
    """One unflipped view: the arg-max of the soft-max is the rescaled entry's arg-max of the logits."""
    case = _case("one_view")
    (_, _, tie, _), = _reference("one_view")
    got, _ = _run_views(case)
    vw = case["views"][0]
    rows = [dict(first=0, count=1, net=vw["net"], out=vw["out"], win=vw["win"], grid=GRID, soft_off=0)]
    images, offs, nbytes, n_blocks, most = ops.seg_image_table(rows, DEV)
    soft, tabs, dwin = _device_inputs(case)
    labels = ops.seg_label_map_rescaled(soft, tabs, dwin, images, n_blocks, most, case["with_bg"], case["thr"],
                                        labels=torch.empty(nbytes, dtype=torch.uint8, device=DEV))
    oh, ow = vw["out"]
    single = labels[:oh * ow].view(oh, ow).cpu().long()
    assert bool((got[0] == single)[~tie].all())


@pytest.mark.parametrize("name", ["hflip_whole", "two_ratios", "odd_narrow"])
@pytest.mark.parametrize("reduce_zero", [False, True])
def test_areas(name, reduce_zero):
    case = _case(name)
    C = case["N"] + int(case["with_bg"])
    ref = _reference(name)
    gts = [_synthetic_gt(r[1][None], C, 77 + i)[0] if r[1].shape[1] > 40 else r[1].clone() for i, r in enumerate(ref)]
    labels, areas = _run_views(case, gts=gts, reduce_zero=reduce_zero)
    own = sum(ser.areas(lab, gt, C, 255, reduce_zero) for lab, gt in zip(labels, gts))
    assert torch.equal(areas, own), "areas differ from the reference on the kernel's own labels"
    ref_areas = sum(ser.areas(r[1], gt, C, 255, reduce_zero) for r, gt in zip(ref, gts))
    n_tie = sum(int(r[2].sum()) for r in ref)
    print(f"{name} reduce_zero={reduce_zero}: largest difference to the fp64 labels' areas {int((areas - ref_areas).abs().max())}, "
          f"{n_tie} near-ties")
    assert int((areas - ref_areas).abs().max()) <= n_tie
    assert int(areas[0].sum()) > 0


def test_kernel_limits():
    case = _case("hflip_whole")
    rows, counts = _rows(case)
    images, vtab, offs, nbytes, n_blocks, most_img, most_view, most_v = ops.seg_view_tables(rows, counts, DEV)
    soft, tabs, dwin = _device_inputs(case)
    labels = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def call(tabs=tabs, most_img=most_img, most_v=most_v):
        ops.seg_label_map_views(soft, tabs, dwin, images, vtab, n_blocks, most_img, most_view, most_v, True, 0.5, labels=labels)

    wide = _dev_tables(_f32_tables(torch.rand(len(case["wins"]), G, 256, dtype=torch.float64)))
    with pytest.raises(L.Unsupported):   # 256 classes + background
        call(tabs=wide)
    with pytest.raises(L.Unsupported):   # 17 views
        call(most_v=17)
    with pytest.raises(L.Unsupported):   # 65 windows of an image
        call(most_img=65)
    with pytest.raises(ValueError, match="17 views"):
        ops.seg_view_tables([rows[0]] * 17, [17], DEV)
    with pytest.raises(ValueError, match="windows over its"):
        ops.seg_view_tables([dict(rows[0], count=33)] * 2, [2], DEV)
    with pytest.raises(ValueError, match="output size"):
        ops.seg_view_tables([rows[0], dict(rows[1], out=(10, 10))], [2], DEV)
    with pytest.raises(ValueError, match="flags"):
        ops.seg_view_tables([dict(rows[0], flags=4)], [1], DEV)
    with pytest.raises(ValueError, match="one image per call"):
        ops.seg_view_probs(soft, tabs, dwin, images, vtab, n_blocks, most_img, most_view, most_v, True, 0.5, case["outs"][0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_label_map_views(soft.cpu(), tabs, dwin, images, vtab, n_blocks, most_img, most_view, most_v, True, 0.5, labels=labels)
    # a view table that points outside the image table (5 views from row 0 and from row 2 of 4 rows): both images are skipped
    # on the device, nothing is written
    buf = torch.full((nbytes,), SENT8, dtype=torch.uint8, device=DEV)
    bad = vtab.clone()
    bad[:, 1] = 5
    ops.seg_label_map_views(soft, tabs, dwin, images, bad, n_blocks, most_img, most_view, most_v, True, 0.5, labels=buf)
    torch.cuda.synchronize()
    assert bool((buf == SENT8).all())


# ------------------------------------------------------------------------------------------------ 2. the flipped front end
RAW_SIZES = [(120, 161), (75, 100)]
TF = ImageTransform()


def _raws(seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in RAW_SIZES]


def test_view_front_end():
    raws = _raws()
    nets = [(224, 301), (224, 299)]
    rep, sizes = [raws[0]] * 4 + [raws[1]] * 4, [nets[0]] * 4 + [nets[1]] * 4
    flags = [0, 1, 2, 3] * 2
    wins = [(e, 0, x) for e in range(8) for x in (0, sizes[e][1] - 224)]
    got = ops.seg_view_windows_from_u8(rep, sizes, flags, wins, (224, 224), TF.mean, TF.inv_std)
    plain = ops.seg_windows_from_u8(rep, sizes, wins, (224, 224), TF.mean, TF.inv_std)
    zero = ops.seg_view_windows_from_u8(rep, sizes, [0] * 8, wins, (224, 224), TF.mean, TF.inv_std)
    torch.cuda.synchronize()
    assert torch.equal(zero, plain), "flags 0 differ from segclip_seg_windows_from_u8"
    worst = 0.0
    for k, (e, y, x) in enumerate(wins):
        want = sar.view_input(rep[e].cpu(), sizes[e], TF.mean, TF.inv_std, flags[e])[:, y:y + 224, x:x + 224]
        worst = max(worst, float((got[k].cpu().double() - want).abs().max()))
    print(f"flipped front end: largest error {worst:.3e}")
    assert worst <= FE_TOL
    # an odd window width takes the scalar-store path; a whole-image window of a flipped view is the flipped preprocess
    odd = ops.seg_view_windows_from_u8(rep, sizes, flags, [(1, 0, 0)], nets[0], TF.mean, TF.inv_std)
    pre = preprocess(raws[:1], TF, net_sizes=nets[:1])[0]
    assert torch.equal(odd[0], pre.flip(-1))
    with pytest.raises(ValueError, match="flag word"):
        ops.seg_view_source_table(rep, sizes, [0] * 7)
    with pytest.raises(ValueError, match="flag word"):
        ops.seg_view_source_table(rep, sizes, [4] * 8)


# ------------------------------------------------------------------------------------------------ 3. end to end
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
TF_SMALL = ImageTransform(img_scale=(1024, 128))
AUG = TestAug(img_ratios=(1.0, 1.5), flip=True)


def _pre_views(raws, tf, aug):
    """Every view pre-processed and flipped separately, as mmseg's pipeline hands them to aug_test."""
    out = []
    for raw in raws:
        per = []
        for (H, W, f) in aug.views(raw.shape[0], raw.shape[1], tf):
            per.append((sar.flip_back(preprocess([raw], tf, net_sizes=[(H, W)])[0], f).contiguous(), f))
        out.append(per)
    return out


def _e2e_reference(seg, views, out):
    """The fp64 combination of this build's own per-view encode_decode logits -> mean probabilities, labels, gap."""
    logits = [seg.encode_decode(t[None])[0].cpu() for t, _ in views]
    mean = sar.mean_probs(logits, [f for _, f in views], out[0], out[1])
    return (mean,) + sar.labels_and_gap(mean)


def test_predict_raw_aug_end_to_end():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        raws = _raws()
        outs = [(h + 3, w - 2) for (h, w) in RAW_SIZES]
        seg = SegInference(model, emb, True, bg_thresh=0.03, **SLIDE)
        views = _pre_views(raws, TF_SMALL, AUG)
        assert [len(p) for p in views] == [4, 4]
        calls, real = [], model.clip.encode_image

        def counted(*a, **k):
            calls.append(a[0].shape[0])
            return real(*a, **k)

        model.clip.encode_image = counted
        try:
            got = seg.predict_raw(raws, TF_SMALL, outs, aug=AUG)
            assert len(calls) == 1, "the windows of all views share one tower call"
            want = seg.predict_views(views, outs)
        finally:
            del model.clip.encode_image
        assert all(torch.equal(a, b) for a, b in zip(got, want)), "predict_raw(aug=) differs from predict_views"
        assert [tuple(t.shape) for t in got] == outs and all(t.dtype == torch.uint8 for t in got)
        for i in range(2):
            mean, lab, gap = _e2e_reference(seg, views[i], outs[i])
            tie = gap < PROB_TOL
            probs = seg.predict_proba_views(views[i], outs[i])
            assert torch.equal(probs, seg.predict_proba_raw(raws[i], TF_SMALL, AUG, outs[i]))
            assert torch.equal(probs.argmax(dim=0).cpu(), got[i].cpu().long())
            err = float((probs.cpu().double() - mean).abs().max())
            print(f"image {i}: largest probability error {err:.3e}, {int(tie.sum())} near-ties of {tie.numel()}")
            assert err <= PROB_TOL
            assert bool((got[i].cpu().long() == lab)[~tie].all())
            assert int(tie.sum()) <= CAP * tie.numel()
            assert torch.equal(seg.predict_raw(raws[i:i + 1], TF_SMALL, outs[i:i + 1], aug=AUG)[0], got[i]), "an image alone differs"
        # the calls without augmentation are untouched by an augmented call in between
        assert all(torch.equal(a, b) for a, b in zip(seg.predict_raw(raws, TF_SMALL, outs),
                                                      seg.predict_list(preprocess(raws, TF_SMALL), outs)))
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_update_raw_aug_and_eval_epoch():
    """Areas and mIoU against the fp64 combination of this build's per-view logits; margin rule of test_eval_epoch: n near-tie
    pixels move a class's I, P and L by at most n each, hence its IoU = I / U by at most 2 n / (U - n)."""
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        tokens = torch.from_numpy(g["prompt_ids"])
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        cfg = dict(bg_thresh=0.03, **SLIDE)
        seg = SegInference(model, emb, True, **cfg)
        C = seg.num_classes
        aug = TestAug(flip=True)
        batches, ref_areas, n_tie = [], torch.zeros(3, C, dtype=torch.long), 0
        ev = SegEvaluator(seg)
        for k in range(2):
            raws = _raws(seed=20 + k)
            outs = [tuple(t.shape[:2]) for t in raws]
            views = _pre_views(raws, TF_SMALL, aug)
            gts, labs = [], []
            for i in range(len(raws)):
                _, lab, gap = _e2e_reference(seg, views[i], outs[i])
                n_tie += int((gap < PROB_TOL).sum())
                gt = _synthetic_gt(lab[None], C, 50 + k)[0]
                ref_areas += ser.areas(lab, gt, C)
                gts.append(gt.to(torch.uint8))
            batches.append(([t.cpu() for t in raws], gts))
            before = ev.areas.clone()
            labels = ev.update_raw(raws, [t.to(DEV) for t in gts], TF_SMALL, return_labels=True, aug=aug)
            own = sum(ser.areas(lab.cpu(), gt, C) for lab, gt in zip(labels, gts))
            assert torch.equal((ev.areas - before).cpu(), own)
            ev2 = SegEvaluator(seg)
            assert ev2.update_views(views, [t.to(DEV) for t in gts]) is None
            assert torch.equal(ev2.areas, ev.areas - before)
        assert int((ev.areas.cpu() - ref_areas).abs().max()) <= n_tie
        ref = ser.metrics(ref_areas)
        union = ref_areas[1] + ref_areas[2] - ref_areas[0]
        present = union > 0
        per_class = torch.where(union > n_tie, 2.0 * n_tie / (union - n_tie).clamp_min(1).double(), torch.ones(C, dtype=torch.float64))
        margin = 100.0 * float(per_class[present].mean()) if n_tie else 1e-9
        got = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(cfg, aug=aug), transform=TF_SMALL)
        print(f"eval_epoch(aug): {got:.6f}, reference {100 * ref['mIoU']:.6f}, {n_tie} near-ties, margin {margin:.3e}")
        assert 0.0 < got < 100.0
        assert abs(got - 100.0 * ref["mIoU"]) <= margin
        assert got == pytest.approx(100.0 * ev.compute()["mIoU"], abs=1e-12)
        with pytest.raises(ValueError, match="transform"):
            eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(cfg, aug=aug))
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_update_aug_allocates_less_than_one_fp32_plane_per_image():
    """update_raw(aug=) on one image -> 375 x 500 with 21 classes and four views: the peak beyond the towers' own stays below
    one fp32 plane of the output: no (C, oh, ow) tensor and no per-view probability array exists."""
    try:
        model = tiny_seg_model()
        gen = torch.Generator().manual_seed(8)
        emb = torch.randn(20, 64, generator=gen)
        emb = (emb / emb.norm(dim=-1, keepdim=True)).to(DEV)
        raw = torch.randint(0, 256, (375, 500, 3), generator=gen, dtype=torch.uint8).to(DEV)
        gt = torch.randint(0, 21, (375, 500), generator=gen).to(torch.uint8).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.03, **SLIDE)
        ev = SegEvaluator(seg)
        src_views = AUG.views(375, 500, TF_SMALL)

        sizes, flags = [(H, W) for (H, W, _) in src_views], [f for (_, _, f) in src_views]
        wins = [(e, y, x0) for e, (H, W) in enumerate(sizes) for (y, x0) in sr.slide_windows(H, W, SLIDE["crop_size"], SLIDE["stride"])]

        def towers():   # the windows as the front end writes them (no resized image), through the towers
            with torch.no_grad(), config.scope(cross_mode="intended"):
                x = ops.seg_view_windows_from_u8([raw] * len(sizes), sizes, flags, wins, SLIDE["crop_size"], TF_SMALL.mean, TF_SMALL.inv_std)
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

        p_enc, p_upd = peak(towers), peak(lambda: ev.update_raw([raw], [gt], TF_SMALL, aug=AUG))
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
        raw = _raws()[0]
        img = torch.zeros(3, 160, 160, device=DEV)
        with pytest.raises(ValueError, match="empty ratio list"):
            TestAug(img_ratios=())
        with pytest.raises(ValueError, match="flip_direction"):
            TestAug(flip=True, flip_direction="diagonal")
        with pytest.raises(TypeError, match="TestAug"):
            seg.predict_raw([raw], TF_SMALL, aug=dict(flip=True))
        with pytest.raises(ValueError, match="image 0 view 0.*smaller than the crop"):   # ratio 0.5: 64 x 86 under a 128 crop
            seg.predict_raw([raw], TF_SMALL, aug=TestAug(img_ratios=(0.5, 1.0)))
        with pytest.raises(ValueError, match="image 1 view 1.*smaller than the crop"):
            seg.predict_views([[(img, 0)], [(img, 0), (torch.zeros(3, 100, 200, device=DEV), 1)]], [(50, 50)] * 2)
        with pytest.raises(ValueError, match="image 0: 17 views"):
            seg.predict_views([[(img, 0)] * 17], [(50, 50)])
        with pytest.raises(ValueError, match="image 0: 72 windows"):   # 8 views of 9 windows each
            seg.predict_views([[(torch.zeros(3, 320, 320, device=DEV), 0)] * 8], [(50, 50)])
        with pytest.raises(ValueError, match="image 0 view 1: flags"):
            seg.predict_views([[(img, 0), (img, 4)]], [(50, 50)])
        with pytest.raises(ValueError, match="output shapes"):
            seg.predict_views([[(img, 0)], [(img, 1)]], [(50, 50)])
        with pytest.raises(ValueError, match="one image per call"):
            seg._views_forward(segclip_amd.segmentation._SlicedImages([[(img, 0)], [(img, 0)]], augmented=True), [(50, 50)] * 2, dense=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            seg.predict_views([[(img.cpu(), 0)]], [(50, 50)])
        with pytest.raises(ValueError, match="image 0 view 1.*1x or 4x"):   # whole mode: a view the tower has no segmentation branch for
            SegInference(model, emb, True).predict_views([[(torch.zeros(3, 128, 128, device=DEV), 0),
                                                           (torch.zeros(3, 96, 96, device=DEV), 1)]], [(50, 50)])
        with pytest.raises(ValueError, match="one \\(H, W\\) per view"):
            seg.predict_raw([raw], TF_SMALL, aug=TestAug(flip=True), net_sizes=[[(128, 172)]])
        assert tuple(seg.predict_views([[(img, 0), (img, 1)]], [(50, 51)])[0].shape) == (50, 51)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def _reference_counts():
    """CPU: PROB_DIFF_F32 and the NEAR_TIE_COUNTS table."""
    worst = 0.0
    for name in CASES:
        r64, r32 = _reference(name), _reference(name, torch.float32)
        diff = max(float((a[0].double() - b[0]).abs().amax(dim=0)[~b[3]].max()) for a, b in zip(r32, r64))
        worst = max(worst, diff)
        n_pix, n_tie = sum(r[1].numel() for r in r64), sum(int(r[2].sum()) for r in r64)
        n_diff = sum(int((a[1] != b[1]).sum()) for a, b in zip(r32, r64))
        print(f'    "{name}": ({n_pix}, {n_tie}, {n_diff}),   # fp32 - fp64 probabilities {diff:.3e}', flush=True)
    print(f"PROB_DIFF_F32 = {worst:.3e}")


if __name__ == "__main__":
    _reference_counts()
