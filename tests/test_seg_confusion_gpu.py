"""GPU: the confusion matrix of label maps - segclip_seg_confusion / segclip_seg_confusion_wide (csrc/segment_confusion.inc)
through ops.seg_confusion, SegEvaluator(confusion=True) on every update path and eval_epoch(test_cfg={"confusion": True}) -
held to tests/confusion_reference.py with torch.equal: every count is an integer.  The main check beside the reference is the
identity areas_from_confusion(conf) == ops.seg_areas / seg_areas_wide on the same inputs."""
import functools

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import PAMR, Despeckle, ImageTransform, SegEvaluator, SegInference, TestAug, preprocess
from segclip_amd.train import eval_epoch
from tests import confusion_reference as cr
from tests import kernel_frames as kf
from tests.helpers import load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I16 = torch.uint8, torch.int16
SIZES = (1, 15, 17, 255, 4099, 300007)
# (ignore_index, reduce_zero_label): the dtype's usual value, a value that occurs, values outside the dtype
RULES = {U8: [(255, False), (255, True), (1, False), (1, True), (300, False), (-1, True), (0, False), (65535, True)],
         I16: [(65535, False), (65535, True), (1, False), (1, True), (70000, False), (-1, True), (255, False), (0, True)]}


def _dense_limit():
    """the largest class count of the dense route, read from the route entry (it is the same for both dtypes)"""
    lo, hi = 21, 256   # dense at 21 and sparse at 256 are asserted by test_routes
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ops.seg_confusion_route(mid, U8) == "dense":
            lo = mid
        else:
            hi = mid
    return lo


@functools.lru_cache(maxsize=None)
def class_counts(dtype):
    d = _dense_limit()
    return ((1, 2, 21, 151, 256) if dtype == U8 else (21, 257, 460, 848, 1024)) + (d, d + 1)


def _to_dev(values, dtype, offset):
    """the values in a view that starts `offset` elements after a 256-byte aligned address"""
    n = len(values)
    buf = torch.zeros(n + 64, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 256 == 0
    t = torch.from_numpy(np.asarray(values, np.int64))
    if dtype == I16:
        t = torch.where(t >= 32768, t - 65536, t)
    view = buf[offset:offset + n]
    view.copy_(t.to(dtype))
    return view


def _areas(pred, gt, C, ignore_index, reduce_zero):
    fn = ops.seg_areas if pred.dtype == U8 else ops.seg_areas_wide
    return fn(pred, gt, C, ignore_index, reduce_zero)


@functools.lru_cache(maxsize=None)
def _maps(kind, n, C, top):
    rng = np.random.default_rng(1000 * C + n % 997 + (7 if kind == "blocky" else 0))
    return cr.blocky_pair(rng, n, C) if kind == "blocky" else cr.random_pair(rng, n, C, top)


def _case_ids():
    return [(dtype, i) for dtype in (U8, I16) for i in range(7)]


@pytest.mark.parametrize("dtype,which", _case_ids(), ids=lambda v: str(v).replace("torch.", ""))
def test_kernel_against_reference(dtype, which):
    """Every n, both kinds of map and every combination of the two bases' offsets; the rule changes from case to case, so that
    every class count meets all eight.  Exact equality with the numpy reference, and the identity with seg_areas."""
    C = class_counts(dtype)[which]
    top = 255 if dtype == U8 else 65535
    rules = RULES[dtype]
    seen, step = set(), which
    for n in SIZES:
        for kind in ("blocky", "random"):
            ignore_index, reduce_zero = rules[step % len(rules)]
            step += 1
            seen.add((ignore_index, reduce_zero))
            pred, gt = _maps(kind, n, C, top)
            want = torch.from_numpy(cr.confusion(pred, gt, C, ignore_index, reduce_zero))
            want_areas = torch.from_numpy(cr.areas_from_confusion(want.numpy()))
            for po in (0, 1):
                for go in (0, 1):
                    p, g = _to_dev(pred, dtype, po), _to_dev(gt, dtype, go)
                    assert p.data_ptr() % 16 == po * p.element_size() and g.data_ptr() % 16 == go * g.element_size()
                    conf = ops.seg_confusion(p, g, C, ignore_index, reduce_zero)
                    what = f"C={C} n={n} {kind} offsets ({po}, {go}) ignore {ignore_index} reduce_zero {reduce_zero}"
                    assert conf.dtype == torch.int64 and tuple(conf.shape) == (C + 1, C + 1) and conf.is_cuda, what
                    assert torch.equal(conf.cpu(), want), what
                    areas = _areas(p, g, C, ignore_index, reduce_zero).cpu()
                    assert torch.equal(SegEvaluator.areas_from_confusion(conf.cpu()), areas), f"{what}: the identity"
                    assert torch.equal(areas, want_areas), what
    assert len(seen) == len(rules)


def test_routes():
    assert ops.seg_confusion_route(21, U8) == "dense" and ops.seg_confusion_route(21, I16) == "dense"
    assert ops.seg_confusion_route(1, U8) == "dense"
    assert ops.seg_confusion_route(256, U8) == "sparse"
    assert ops.seg_confusion_route(1024, I16) == "sparse" and ops.seg_confusion_route(460, I16) == "sparse"
    d = _dense_limit()
    print(f"dense up to {d} classes")
    assert d >= 151, "VOC, COCO and ADE20K-150 are meant to be on the dense route"
    for dtype in (U8, I16):
        assert ops.seg_confusion_route(d, dtype) == "dense" and ops.seg_confusion_route(d + 1, dtype) == "sparse"
    with pytest.raises(L.Unsupported):
        ops.seg_confusion_route(257, U8)
    with pytest.raises(L.Unsupported):
        ops.seg_confusion_route(1025, I16)
    with pytest.raises(RuntimeError):
        ops.seg_confusion_route(0, U8)
    # the wide entry at 21 classes counts what the uint8 entry counts
    for kind in ("blocky", "random"):
        pred, gt = _maps(kind, 4099, 21, 255)
        for ignore_index, reduce_zero in ((255, False), (1, True)):
            c8 = ops.seg_confusion(_to_dev(pred, U8, 1), _to_dev(gt, U8, 0), 21, ignore_index, reduce_zero)
            c16 = ops.seg_confusion(_to_dev(pred, I16, 0), _to_dev(gt, I16, 1), 21, ignore_index, reduce_zero)
            assert torch.equal(c8, c16) and int(c8.sum()) > 0


@pytest.mark.parametrize("dtype,C", [(U8, 21), (U8, 256), (I16, 151), (I16, 848)], ids=lambda v: str(v).replace("torch.", ""))
def test_accumulation(dtype, C):
    """A second call into the same matrix doubles it, two launches into fresh matrices are bit-equal, and nothing outside
    the (C + 1)^2 elements of a framed matrix is written."""
    top = 255 if dtype == U8 else 65535
    for kind in ("blocky", "random"):
        pred, gt = _maps(kind, 300007, C, top)
        p, g = _to_dev(pred, dtype, 1), _to_dev(gt, dtype, 0)
        rule = (top, True)
        frame = kf.Frame((C + 1, C + 1), torch.int64)
        frame.v.zero_()
        assert frame.v.is_contiguous()
        assert ops.seg_confusion(p, g, C, *rule, conf=frame.v).data_ptr() == frame.v.data_ptr()
        first = frame.v.clone()
        fresh = ops.seg_confusion(p, g, C, *rule)
        torch.cuda.synchronize()
        assert frame.intact(), "written outside the matrix"
        assert torch.equal(first, fresh), "two launches differ"
        assert torch.equal(first.cpu(), torch.from_numpy(cr.confusion(pred, gt, C, *rule)))
        ops.seg_confusion(p, g, C, *rule, conf=frame.v)
        assert torch.equal(frame.v, 2 * first) and frame.intact()
        assert int(first.sum()) > 0
    # n == 0 launches nothing and returns zeros
    empty = ops.seg_confusion(p[:0], g[:0], C)
    assert tuple(empty.shape) == (C + 1, C + 1) and int(empty.abs().sum()) == 0


def test_more_pixels_than_one_launch_counts():
    """2^30 + 4099 pixels: the entry splits the input at 2^30 so that no 32-bit counter of a workgroup can overflow.  Constant
    maps with marked pixels around the split and at both ends; the expected matrix is written down, not computed."""
    n, C = (1 << 30) + 4099, 5
    pred, gt = torch.zeros(n, dtype=U8, device=DEV), torch.zeros(n, dtype=U8, device=DEV)
    want = torch.zeros(C + 1, C + 1, dtype=torch.int64)
    marks = {0: (1, 2), (1 << 30) - 1: (2, 3), 1 << 30: (3, 4), (1 << 30) + 1: (4, 9), n - 1: (200, 1), 77: (1, 255)}
    for i, (p, g) in marks.items():
        pred[i], gt[i] = p, g
        if g != 255:
            want[min(g, C), min(p, C)] += 1
    want[0, 0] = n - len(marks)
    conf = ops.seg_confusion(pred, gt, C)
    assert torch.equal(conf.cpu(), want)
    assert torch.equal(SegEvaluator.areas_from_confusion(conf.cpu()), ops.seg_areas(pred, gt, C).cpu())


def test_refusals():
    lab8 = torch.zeros(64, dtype=U8, device=DEV)
    lab16 = torch.zeros(64, dtype=I16, device=DEV)
    with pytest.raises(L.Unsupported, match="at most 256"):
        ops.seg_confusion(lab8, lab8, 257)
    with pytest.raises(L.Unsupported, match="at most 1024"):
        ops.seg_confusion(lab16, lab16, 1025)
    with pytest.raises(RuntimeError):
        ops.seg_confusion(lab8, lab8, 0)
    with pytest.raises(ValueError, match="both uint8 or both int16"):
        ops.seg_confusion(lab8, lab16, 21)
    with pytest.raises(ValueError, match="both uint8 or both int16"):
        ops.seg_confusion(lab8.int(), lab8.int(), 21)
    with pytest.raises(ValueError, match="same size"):
        ops.seg_confusion(lab8, lab8[:63], 21)
    for bad in (torch.zeros(21, 21, dtype=torch.int64, device=DEV), torch.zeros(22, 22, dtype=torch.int32, device=DEV),
                torch.zeros(22, 44, dtype=torch.int64, device=DEV)[:, ::2], torch.zeros(3, 21, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match=r"\(C \+ 1, C \+ 1\) int64"):
            ops.seg_confusion(lab8, lab8, 21, conf=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_confusion(lab8.cpu(), lab8.cpu(), 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_confusion(lab8, lab8, 21, conf=torch.zeros(22, 22, dtype=torch.int64))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
TF = ImageTransform()
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(90, 120), (130, 101), (75, 75)]
OLD_KEYS = {"mIoU", "aAcc", "mAcc", "IoU", "Acc"}
NEW_KEYS = {"confusion", "Dice", "Precision", "Recall", "Fscore", "mDice", "mFscore", "fwIoU", "kappa"}


def _raws(seed, C, dtype=U8):
    """three decoded pictures and blocky ground truths over 0 .. C + 1 with a band of the dtype's ignore value"""
    g = torch.Generator().manual_seed(seed)
    raws = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=U8).to(DEV) for (h, w) in RAW_SIZES]
    gts = []
    for i, (h, w) in enumerate(RAW_SIZES):
        _, gt = cr.blocky_pair(np.random.default_rng(seed + i), h * w, C + 2)
        gt = gt.reshape(h, w)
        gt[5:9] = 255 if dtype == U8 else 65535
        gts.append(_to_dev(gt.reshape(-1), dtype, 0).view(h, w))
    return raws, gts


def _unsigned(t):
    t = t.cpu()
    return (t.long() & 0xFFFF).numpy() if t.dtype == I16 else t.numpy()


def _check_compute(out, old, conf):
    assert set(out) == OLD_KEYS | NEW_KEYS and set(old) == OLD_KEYS
    assert out["mIoU"] == old["mIoU"] and torch.equal(out["IoU"].nan_to_num(-1.0), old["IoU"].nan_to_num(-1.0))
    assert out["confusion"].dtype == torch.int64 and not out["confusion"].is_cuda and np.array_equal(out["confusion"].numpy(), conf)
    ref = cr.metrics(conf)
    for key in ("Dice", "Precision", "Recall", "Fscore"):
        got = out[key].numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref[key])), key
        ok = ~np.isnan(got)
        assert np.all(np.abs(got[ok] - ref[key][ok]) <= 1e-12 * np.abs(ref[key][ok])), key
    for key in ("mDice", "mFscore", "fwIoU", "kappa"):
        assert out[key] == pytest.approx(ref[key], rel=1e-12), key


def _run_paths(seg, paths, gts, rule, ignore_index):
    C = seg.num_classes
    for name, path in paths.items():
        ev0 = SegEvaluator(seg, **rule)
        ev = SegEvaluator(seg, confusion=True, **rule)
        assert ev0.confusion is None
        assert ev.confusion.is_cuda and ev.confusion.dtype == torch.int64 and tuple(ev.confusion.shape) == (C + 1, C + 1)
        assert path(ev0) is None
        labels = path(ev, return_labels=True)
        assert [tuple(t.shape) for t in labels] == RAW_SIZES, name
        assert torch.equal(ev.areas, ev0.areas) and int(ev.areas.sum()) > 0, name
        want = sum(ops.seg_confusion(lab.reshape(-1), gt.reshape(-1), C, **rule) for lab, gt in zip(labels, gts))
        assert torch.equal(ev.confusion, want), name
        ref = sum(cr.confusion(_unsigned(lab), _unsigned(gt), C, ignore_index, rule["reduce_zero_label"]) for lab, gt in zip(labels, gts))
        assert np.array_equal(ev.confusion.cpu().numpy(), ref), name
        assert torch.equal(SegEvaluator.areas_from_confusion(ev.confusion.cpu()), ev.areas.cpu()), name
        # inside, the labels are formed even when the caller does not want them
        assert path(ev) is None
        assert torch.equal(ev.areas, 2 * ev0.areas) and torch.equal(ev.confusion, 2 * want), name
        _check_compute(ev.compute(), ev0.compute(), 2 * ref)
        ev.reset()
        assert int(ev.areas.abs().sum()) == 0 and int(ev.confusion.abs().sum()) == 0


def test_end_to_end():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.02, **SLIDE)
        raws, gts = _raws(11, seg.num_classes)
        pre = preprocess(raws, TF)
        views = [[(t, 0), (t.flip(-1).contiguous(), ops.SEG_FLIP_H)] for t in pre]
        pamr = PAMR(iters=2, dilations=(1, 2))
        paths = {
            "update": lambda ev, **kw: ev.update(pre, gts, **kw),
            "update_raw": lambda ev, **kw: ev.update_raw(raws, gts, TF, **kw),
            "update_raw_aug": lambda ev, **kw: ev.update_raw(raws, gts, TF, aug=TestAug(flip=True), **kw),
            "update_raw_refine": lambda ev, **kw: ev.update_raw(raws, gts, TF, refine=pamr, **kw),
            "update_raw_clean": lambda ev, **kw: ev.update_raw(raws, gts, TF, clean=Despeckle(12, fill=0), **kw),
            "update_views": lambda ev, **kw: ev.update_views(views, gts, **kw),
        }
        _run_paths(seg, paths, gts, dict(reduce_zero_label=True), 255)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_end_to_end_int16():
    try:
        model = tiny_seg_model()
        e = torch.randn(300, 64, generator=torch.Generator().manual_seed(3))
        emb = (e / e.norm(dim=-1, keepdim=True)).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.0, label_dtype=I16, **SLIDE)
        assert seg.num_classes == 301 and ops.seg_confusion_route(301, I16) == "sparse"
        raws, gts = _raws(12, seg.num_classes, I16)
        pre = preprocess(raws, TF)
        paths = {
            "update": lambda ev, **kw: ev.update(pre, gts, **kw),
            "update_raw": lambda ev, **kw: ev.update_raw(raws, gts, TF, **kw),
        }
        _run_paths(seg, paths, gts, dict(ignore_index=65535, reduce_zero_label=False), 65535)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_eval_epoch():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        tokens = torch.from_numpy(g["prompt_ids"])
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.02, **SLIDE)
        batches = []
        for k in range(2):
            raws, gts = _raws(40 + k, seg.num_classes)
            batches.append(([t.cpu() for t in raws[:2 + k]], [t.cpu() for t in gts[:2 + k]]))
        cfg = dict(bg_thresh=0.02, reduce_zero_label=True, **SLIDE)
        plain = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(cfg), transform=TF)
        assert isinstance(plain, float)
        assert plain == eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(confusion=False, **cfg), transform=TF)
        got = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(confusion=True, **cfg), transform=TF)
        ev = SegEvaluator(seg, reduce_zero_label=True, confusion=True)
        for raws, gts in batches:
            ev.update_raw([t.to(DEV) for t in raws], [t.to(DEV) for t in gts], TF)
        want = ev.compute()
        assert set(got) == {"mIoU", "mDice", "mFscore", "fwIoU", "kappa", "confusion"} and got["mIoU"] == plain
        for key in ("mDice", "mFscore", "fwIoU"):
            assert got[key] == want[key] * 100.0 and 0.0 <= got[key] <= 100.0, key
        assert got["kappa"] == want["kappa"] and -1.0 <= got["kappa"] <= 1.0
        assert torch.equal(got["confusion"], want["confusion"]) and int(got["confusion"].sum()) > 0
        assert SegEvaluator.metrics_from_areas(SegEvaluator.areas_from_confusion(got["confusion"]))["mIoU"] * 100.0 == plain
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
