"""GPU: the background-threshold sweep - segclip_seg_label_map_rescaled_sweep (csrc/segment_sweep.inc), ops.seg_label_map_sweep,
SegSweepEvaluator and train.sweep_bg_thresh.

The yardstick is the single-threshold entry itself: plane t and areas slice t of a sweep must equal, bit for bit and integer
for integer, what segclip_seg_label_map_rescaled gives for bg_thresh = thresholds[t] (torch.equal; there is no tolerance).
That entry is held to the fp64 reference by tests/test_seg_eval_gpu.py; one plane per case is held to it here directly as well,
by the near-tie rule of that file (TIE = 1e-6, at most 0.05 % of the output pixels, the counts of NEAR_TIE_COUNTS).  The
geometries are the cases of that file: overlapping windows, disagreeing taps, tiles that straddle two images."""
import functools

import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import ImageTransform, SegEvaluator, SegInference, SegSweepEvaluator, TestAug
from segclip_amd.train import sweep_bg_thresh
from tests import kernel_frames as kf
from tests.helpers import CountedEncodeImage, load_golden, tiny_seg_model
from tests.test_seg_eval_gpu import (CAP, G, NEAR_TIE_COUNTS, SLIDE, TIE, _case, _dev_tables, _f32_tables, _image_rows,
                                     _reference, _synthetic_gt)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8 = 0xA5
BASE = (0.0, 0.05, 0.2, 0.4, 0.6, 0.8, 0.95, 2.0)
NAMES = ["voc", "context_tall", "whole", "identity", "x1.5", "slide112", "many_classes"]
ERR_INVALID, ERR_UNSUPPORTED = -1, -2


def _thr_list(case):
    return sorted(set(BASE) | {case["thr"]})


class _Ctx:
    """A case on the device: tables, descriptor table, a synthetic ground truth built on the single entry's own labels at the
    case's threshold, and the single-threshold results, computed once per (threshold, reduce_zero) and left unchanged."""

    def __init__(self, name, tables=None, N=None):
        case = _case(name)
        if tables is not None:
            case["t32"], case["N"] = tables, N
        self.case, self.B, (self.oh, self.ow) = case, case["B"], case["out"]
        self.C = case["N"] + 1
        offs = [b * self.oh * self.ow for b in range(self.B)]
        self.images, self.lab_offs, self.nbytes, self.n_blocks, self.most = ops.seg_image_table(_image_rows(case, offs), DEV)
        self.dwin = torch.tensor(case["wins"], dtype=torch.int32, device=DEV).view(-1, 3)
        self.soft, self.tabs = case["soft"].reshape(-1).to(DEV), _dev_tables(case["t32"])
        self._singles = {}
        base = self.planes_of(self.single(case["thr"])[0][None])[0].cpu().long()
        self.gt = _synthetic_gt(base, self.C, 77).to(torch.uint8).reshape(-1).to(DEV)

    def planes_of(self, flat):
        """(T, plane bytes) -> (T, B, oh, ow)"""
        n = self.oh * self.ow
        return torch.stack([flat[:, o:o + n].reshape(-1, self.oh, self.ow) for o in self.lab_offs], dim=1)

    def single(self, thr, reduce_zero=None):
        """segclip_seg_label_map_rescaled at one threshold -> (labels (nbytes) with zeroed padding, areas (3, C) or None)"""
        key = (float(thr), reduce_zero)
        if key not in self._singles:
            labels = torch.zeros(self.nbytes, dtype=torch.uint8, device=DEV)
            areas = None if reduce_zero is None else torch.zeros(3, self.C, dtype=torch.int64, device=DEV)
            ops.seg_label_map_rescaled(self.soft, self.tabs, self.dwin, self.images, self.n_blocks, self.most, True, thr, labels=labels,
                                       gt=None if reduce_zero is None else self.gt, areas=areas, ignore_index=255,
                                       reduce_zero_label=bool(reduce_zero))
            self._singles[key] = (labels, areas)
        return self._singles[key]

    def sweep(self, thr, reduce_zero=None, want_labels=True, extra=0, pad=64):
        """The sweep into sentinel-framed buffers, launched twice: identical bits, frames and padding untouched.
        extra: bytes between two planes (1: the odd planes start off a dword boundary and take the byte stores).
        -> (labels (T, B, oh, ow) or None, areas (T, 3, C) or None)"""
        T, plane = len(thr), self.nbytes + extra
        res = []
        for _ in range(2):
            buf = torch.full((T * plane + 2 * pad,), SENT8, dtype=torch.uint8, device=DEV)
            view = buf[pad:pad + T * plane].view(T, plane) if want_labels else None
            fa = None
            if reduce_zero is not None:
                fa = kf.Frame((T, 3, self.C), torch.int64)
                fa.v.zero_()
            ops.seg_label_map_sweep(self.soft, self.tabs, self.dwin, self.images, self.n_blocks, self.most, thr, labels=view,
                                    gt=None if fa is None else self.gt, areas=None if fa is None else fa.v, ignore_index=255,
                                    reduce_zero_label=bool(reduce_zero))
            torch.cuda.synchronize()
            assert bool((buf[:pad] == SENT8).all()) and bool((buf[pad + T * plane:] == SENT8).all()), "wrote outside the planes"
            if want_labels:
                n = self.oh * self.ow
                for b, o in enumerate(self.lab_offs):   # the padding between two images and between two planes
                    end = self.lab_offs[b + 1] if b + 1 < self.B else plane
                    assert bool((view[:, o + n:end] == SENT8).all()), "wrote into the padding"
            else:
                assert bool((buf == SENT8).all())
            if fa is not None:
                assert fa.intact(), "wrote outside the areas"
            res.append((None if view is None else self.planes_of(view), None if fa is None else fa.v.clone()))
        if want_labels:
            assert torch.equal(res[0][0], res[1][0]), "repeat launch: labels differ"
        if fa is not None:
            assert torch.equal(res[0][1], res[1][1]), "repeat launch: areas differ"
        return res[0]

    def check_equal(self, thr, reduce_zero=False, **kw):
        """Every plane and every areas slice of the sweep against the single-threshold entry."""
        labels, areas = self.sweep(thr, reduce_zero, **kw)
        for t, v in enumerate(thr):
            one_l, one_a = self.single(v, reduce_zero)
            assert torch.equal(labels[t], self.planes_of(one_l[None])[0]), f"{self.case['name']}: plane {t} (bg_thresh {v}) differs"
            assert torch.equal(areas[t], one_a), f"{self.case['name']}: areas slice {t} (bg_thresh {v}) differs"
        return labels, areas


@functools.lru_cache(maxsize=None)
def _ctx(name):
    return _Ctx(name)


# ------------------------------------------------------------------------------------------------ 1. bit-equality
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("reduce_zero", [False, True])
def test_sweep_equals_single_threshold_entry(name, reduce_zero):
    ctx = _ctx(name)
    thr = _thr_list(ctx.case)
    odd = NAMES.index(name) % 2 == 1   # every other case: planes off the dword boundary, a frame of 3 bytes
    labels, areas = ctx.check_equal(thr, reduce_zero, extra=1 if odd else 0, pad=3 if odd else 64)
    changed = [int((labels[t] != labels[t + 1]).sum()) for t in range(len(thr) - 1)]
    print(f"{name} reduce_zero={reduce_zero}: T={len(thr)}, labels changed between neighbouring thresholds: {changed}")
    assert sum(1 for c in changed if c) >= 1, "every plane is the same: the comparison shows nothing"
    assert not torch.equal(areas[0], areas[-1])
    # the label area does not depend on the threshold
    assert all(torch.equal(areas[t, 2], areas[0, 2]) for t in range(len(thr)))


# ------------------------------------------------------------------------------------------------ 2. threshold edge values
def _own_scores(ctx):
    """Three fp32 values of the case's best_score that lie below their window's table_max (where the threshold decides)."""
    score, tmax = ctx.case["t32"]["best_score"], ctx.case["t32"]["table_max"]
    vals = score[score < tmax[:, None]].unique().tolist()
    assert len(vals) >= 3
    return [vals[len(vals) // 4], vals[len(vals) // 2], vals[3 * len(vals) // 4]]


@pytest.mark.parametrize("name", ["voc", "slide112"])
def test_threshold_edge_values(name):
    ctx = _ctx(name)
    b = _own_scores(ctx)
    after = float(torch.nextafter(torch.tensor(b[1]), torch.tensor(float("inf"))))
    top = float(ctx.case["t32"]["table_max"].max())
    lists = {
        "T=1": [ctx.case["thr"]],
        "T=16": [0.03 + 0.064 * i for i in range(16)],
        "own scores": b,                                   # strict <: a group is not background at its own score
        "own score and its successor": sorted({b[0], b[1], after, b[2]}),
        "above every table_max": [0.5 * top, top, float(torch.nextafter(torch.tensor(top), torch.tensor(2.0))), 1.5],
        "zero": [0.0, 0.5],
        "negative": [-1.0, 0.0],
    }
    for what, thr in lists.items():
        thr = torch.tensor(thr).tolist()   # the fp32 values both entries see
        labels, _ = ctx.check_equal(thr, False)
        print(f"{name} {what}: background pixels per threshold {[int((labels[t] == 0).sum()) for t in range(len(thr))]}")
        if what == "zero":   # no background by threshold: only pixels whose best score is not positive
            assert int((labels[0] == 0).sum()) <= int((labels[1] == 0).sum())
        if what == "above every table_max":   # table_max clamps: the planes above it are equal
            assert torch.equal(labels[1], labels[3]) and torch.equal(labels[2], labels[3])


# ------------------------------------------------------------------------------------------------ 3. against fp64
@pytest.mark.parametrize("name", NAMES)
def test_own_threshold_plane_against_fp64(name):
    ctx = _ctx(name)
    thr = _thr_list(ctx.case)
    want, tie, _ = _reference(ctx.case)
    n_tie = int(tie.sum())
    labels, _ = ctx.sweep(thr)
    got = labels[thr.index(ctx.case["thr"])].cpu().long()
    print(f"{name}: {tie.numel()} output pixels, {n_tie} near-ties, labels differ at {int((got != want).sum())}")
    assert (tie.numel(), n_tie) == NEAR_TIE_COUNTS[name][:2], "the reference's own count changed"
    assert n_tie <= CAP * tie.numel()
    assert bool((got == want)[~tie].all()), f"{name}: labels differ away from near-ties"
    assert TIE == 1e-6 and CAP == 5e-4


# ------------------------------------------------------------------------------------------------ 4. the accumulating contract
def test_areas_accumulate_and_optional_outputs():
    ctx = _ctx("voc")
    thr = _thr_list(ctx.case)
    _, once = ctx.check_equal(thr, False)
    areas = torch.zeros(len(thr), 3, ctx.C, dtype=torch.int64, device=DEV)
    for _ in range(2):
        ops.seg_label_map_sweep(ctx.soft, ctx.tabs, ctx.dwin, ctx.images, ctx.n_blocks, ctx.most, thr, gt=ctx.gt, areas=areas)
    assert torch.equal(areas, 2 * once), "two calls on the same areas do not double them"
    # labels = NULL with areas; labels without a ground truth
    _, alone = ctx.sweep(thr, False, want_labels=False)
    assert torch.equal(alone, once)
    labels, none = ctx.sweep(thr, None)
    assert none is None
    for t, v in enumerate(thr):
        assert torch.equal(labels[t], ctx.planes_of(ctx.single(v, False)[0][None])[0])


def test_largest_lds_footprint():
    """N + 1 = 256 classes at T = 16 on the many_classes geometry: the counters take 35 KiB beside 48 KiB of tables and lists,
    past the 64 KiB a kernel gets without asking."""
    g = torch.Generator().manual_seed(91)
    nW = len(_case("many_classes")["wins"])
    table = torch.rand(nW, G, 255, generator=g, dtype=torch.float64) * 0.1
    for k in range(nW):
        for j in range(G):
            table[k, j, (k * G + j) * 37 % 255] = 0.05 + 0.9 * float(torch.rand((), generator=g))
    ctx = _Ctx("many_classes", _f32_tables(table), 255)
    thr = [0.06 * (i + 1) for i in range(16)]
    thr = torch.tensor(thr).tolist()
    labels, areas = ctx.check_equal(thr, False)
    assert labels[0].unique().numel() >= 10
    assert not torch.equal(labels[0], labels[-1])


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_return_their_code_and_write_nothing():
    ctx = _ctx("identity")
    lib = L.load()
    fl = kf.Frame((16, ctx.nbytes), torch.uint8)
    fa = kf.Frame((16, 3, ctx.C), torch.int64)
    nan, inf = float("nan"), float("inf")

    def call(thr, T=None, N=None, most=None, refused=True):
        host = (L.C.c_float * max(len(thr), 1))(*thr)
        rc = lib.segclip_seg_label_map_rescaled_sweep(
            L.ptr(ctx.soft), ctx.soft.numel(), *(L.ptr(t) for t in ctx.tabs), L.ptr(ctx.dwin), L.ptr(ctx.images), ctx.dwin.shape[0],
            ctx.B, ctx.n_blocks, ctx.most if most is None else most, G, ctx.case["N"] if N is None else N,
            L.C.cast(host, L.C.c_void_p), len(thr) if T is None else T, fl.p, ctx.nbytes, L.ptr(ctx.gt), ctx.gt.numel(), 255, 0, fa.p,
            L.stream())
        torch.cuda.synchronize()
        assert not refused or (fl.untouched() and fa.untouched()), f"a refused call wrote something: thresholds {thr}"
        return rc

    assert call([0.5], T=0) == ERR_INVALID
    assert call([0.5], T=-1) == ERR_INVALID
    assert call([0.1, nan]) == ERR_INVALID
    assert call([nan]) == ERR_INVALID
    assert call([0.1, inf]) == ERR_INVALID
    assert call([-inf, 0.1]) == ERR_INVALID
    assert call([0.4, 0.4]) == ERR_INVALID
    assert call([0.5, 0.4, 0.6]) == ERR_INVALID
    assert b"increasing" in lib.segclip_last_error_string()
    assert call([0.05 * i for i in range(17)]) == ERR_UNSUPPORTED
    assert call([0.5], N=256) == ERR_UNSUPPORTED      # 256 classes + background
    assert call([0.5], most=65) == ERR_UNSUPPORTED    # 65 windows per image
    # the wrapper turns the codes into exceptions
    with pytest.raises(L.Unsupported):
        ops.seg_label_map_sweep(ctx.soft, ctx.tabs, ctx.dwin, ctx.images, ctx.n_blocks, ctx.most, [0.05 * i for i in range(17)],
                                labels=fl.v.new_zeros(17, ctx.nbytes))
    with pytest.raises(RuntimeError, match="increasing"):
        ops.seg_label_map_sweep(ctx.soft, ctx.tabs, ctx.dwin, ctx.images, ctx.n_blocks, ctx.most, [0.5, 0.5],
                                labels=fl.v.new_zeros(2, ctx.nbytes))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_label_map_sweep(ctx.soft, ctx.tabs, ctx.dwin, ctx.images, ctx.n_blocks, ctx.most, [0.5],
                                labels=torch.zeros(1, ctx.nbytes, dtype=torch.uint8))
    # and the accepted call on the same frames writes every plane
    assert call([0.2, 0.8], refused=False) == 0
    assert not fl.untouched() and fl.intact()


# ------------------------------------------------------------------------------------------------ 6. end to end
E2E_THR = [0.0, 0.01, 0.02, 0.03, 0.05, 0.1, 0.5, 2.0]
RAW_SIZES = [(300, 300), (500, 375), (375, 500), (281, 500)]
TF = ImageTransform()


def _raws(seed):
    g = torch.Generator().manual_seed(seed)
    raws = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in RAW_SIZES]
    gts = [torch.randint(0, 14, (h, w), generator=g).to(torch.uint8).to(DEV) for (h, w) in RAW_SIZES]
    for t in gts:
        t[5:9] = 255
    return raws, gts


def _peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del out
    return p


@pytest.mark.parametrize("mode", ["slide", "whole"])
def test_evaluator_end_to_end(mode):
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        raws, gts = _raws(6)
        kw = dict(SLIDE) if mode == "slide" else {}
        nets = None if mode == "slide" else [(128, 128), (64, 64), (128, 128), (64, 64)]
        T = len(E2E_THR)
        # seg.bg_thresh is ignored by the sweep: any value
        sweep = SegSweepEvaluator(SegInference(model, emb, True, bg_thresh=0.77, **kw), E2E_THR)
        assert tuple(sweep.areas.shape) == (T, 3, sweep.seg.num_classes) and sweep.areas.is_cuda
        with CountedEncodeImage(model) as calls:
            planes = sweep.update_raw(raws, gts, TF, return_labels=True, net_sizes=nets)
            sweep_calls = list(calls)
        assert [tuple(p.shape) for p in planes] == [(T, h, w) for (h, w) in RAW_SIZES] and all(p.dtype == torch.uint8 for p in planes)
        distinct = 0
        for t, thr in enumerate(E2E_THR):
            seg = SegInference(model, emb, True, bg_thresh=thr, **kw)
            ev = SegEvaluator(seg)
            with CountedEncodeImage(model) as calls:
                ev.update_raw(raws, gts, TF, net_sizes=nets)
                assert list(calls) == sweep_calls, "the sweep does not call the tower as one single evaluation does"
            assert torch.equal(sweep.areas[t], ev.areas), f"{mode}: areas slice {t} (bg_thresh {thr}) differs"
            want = seg.predict_raw(raws, TF, net_sizes=nets)
            assert all(torch.equal(p[t], w) for p, w in zip(planes, want)), f"{mode}: label planes {t} (bg_thresh {thr}) differ"
            distinct += int(t > 0 and not torch.equal(sweep.areas[t], sweep.areas[t - 1]))
        assert distinct >= 2, "the thresholds do not change the result"
        # compute(): one host copy, SegEvaluator's reduction per slice
        out = sweep.compute()
        assert out["thresholds"] == torch.tensor(E2E_THR).tolist() and len(out["metrics"]) == T
        mious = [m["mIoU"] for m in out["metrics"]]
        assert out["best"] == (mious.index(max(mious)), out["thresholds"][mious.index(max(mious))], max(mious))
        assert mious[2] == SegEvaluator.metrics_from_areas(sweep.areas[2].cpu())["mIoU"]
        # update() on pre-processed images adds the same areas; without return_labels nothing is returned
        from segclip_amd.segmentation import preprocess
        twice = sweep.areas.clone()
        assert sweep.update(preprocess(raws, TF, net_sizes=nets), gts) is None
        assert torch.equal(sweep.areas, 2 * twice)
        sweep.reset()
        assert int(sweep.areas.abs().sum()) == 0
        # allocation: beyond the single evaluation's peak only the T label planes; without them nothing the size of a plane
        single = SegEvaluator(SegInference(model, emb, True, bg_thresh=0.03, **kw))
        p_one = _peak(lambda: single.update_raw(raws, gts, TF, net_sizes=nets))
        p_none = _peak(lambda: sweep.update_raw(raws, gts, TF, net_sizes=nets))
        p_all = _peak(lambda: sweep.update_raw(raws, gts, TF, return_labels=True, net_sizes=nets))
        nbytes = sum((h * w + 3) // 4 * 4 for (h, w) in RAW_SIZES)
        areas_bytes = sweep.areas.numel() * 8
        print(f"{mode}: peak single {p_one}, sweep without labels {p_none}, with labels {p_all}; T planes {T * nbytes}, areas {areas_bytes}")
        assert p_all - p_one < T * nbytes + areas_bytes
        assert p_none - p_one < areas_bytes < 4 * min(h * w for (h, w) in RAW_SIZES)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ 7. train.sweep_bg_thresh
def test_train_sweep_bg_thresh():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        tokens = torch.from_numpy(g["prompt_ids"])
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        thr = E2E_THR + [3.0]   # 2.0 and 3.0 lie above every table_max: equal slices
        batches = []
        for k in range(2):
            raws, gts = _raws(30 + k)
            batches.append(([t.cpu() for t in raws[:2 + k]], [t.cpu() for t in gts[:2 + k]]))
        cfg = dict(bg_thresh=0.9, reduce_zero_label=True, **SLIDE)
        model.train()   # sweep_bg_thresh switches to eval mode itself
        got = sweep_bg_thresh(None, model, DEV, 1, batches, tokens, thr, cfg, transform=TF)
        assert not model.training
        hand = SegSweepEvaluator(SegInference(model, emb, True, **SLIDE), thr, reduce_zero_label=True)
        for raws, gts in batches:
            hand.update_raw([t.to(DEV) for t in raws], [t.to(DEV) for t in gts], TF)
        want = hand.compute()
        assert got["thresholds"] == want["thresholds"] and got["best"] == want["best"]
        assert [m["mIoU"] for m in got["metrics"]] == [m["mIoU"] for m in want["metrics"]]
        assert torch.equal(hand.areas[-1], hand.areas[-2])
        mious = [m["mIoU"] for m in got["metrics"]]
        assert mious[-1] == mious[-2]
        assert got["best"][0] == mious.index(max(mious)), "best is not the lowest threshold among equal mIoU"
        assert 0.0 < got["best"][2] < 1.0
        # pre-processed images instead of decoded ones
        from segclip_amd.segmentation import preprocess
        pre = [([t.cpu() for t in preprocess([r.to(DEV) for r in raws], TF)], gts) for raws, gts in batches]
        again = sweep_bg_thresh(None, model, DEV, 1, pre, tokens, thr, cfg)
        assert [m["mIoU"] for m in again["metrics"]] == mious
        with pytest.raises(ValueError, match="aug"):
            sweep_bg_thresh(None, model, DEV, 1, batches, tokens, thr, dict(aug=TestAug(flip=True), **SLIDE), transform=TF)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ 8. interface errors
def test_interface_errors():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        seg = SegInference(model, emb, True, **SLIDE)
        for bad, match in (([0.5, 0.4], "thresholds.*sorted"), ([0.4, 0.4], "thresholds.*duplicate"),
                           ([0.1, float("nan")], "thresholds.*finite"), ([0.1, float("inf")], "thresholds.*finite"),
                           ([0.01 * i for i in range(17)], "thresholds.*at most 16"), ([], "thresholds.*empty")):
            with pytest.raises(ValueError, match=match):
                SegSweepEvaluator(seg, bad)
        with pytest.raises(ValueError, match="with_bg"):
            SegSweepEvaluator(SegInference(model, emb, False, **SLIDE), [0.5])
        ev = SegSweepEvaluator(seg, [0.01, 0.5])
        raw = torch.zeros(200, 200, 3, dtype=torch.uint8, device=DEV)
        gt = torch.zeros(200, 200, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match="aug"):
            ev.update_raw([raw], [gt], TF, aug=TestAug(flip=True))
        with pytest.raises(ValueError, match="ground truths"):
            ev.update_raw([raw, raw], [gt], TF)
        with pytest.raises(ValueError, match="uint8"):
            ev.update_raw([raw], [gt.float()], TF)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ev.update_raw([raw], [gt.cpu()], TF)
        assert int(ev.areas.abs().sum()) == 0
        labels = ev.update_raw([raw], [gt], TF, return_labels=True)
        assert tuple(labels[0].shape) == (2, 200, 200) and int(ev.areas[:, 1].sum()) == 2 * 200 * 200
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
