"""The boundary kernels (csrc/segment_boundary.inc) through the C ABI and the Python layer - ops.seg_boundary, boundary_bands,
boundary_areas, SegEvaluator(boundary=) on every update path and eval_epoch(test_cfg={"boundary": ...}) - held to
tests/boundary_reference.py with torch.equal: every figure is an integer.  Inputs and outputs lie in tests/kernel_frames.py
frames: nothing outside an output is written, inputs stay as they are, bytes between two maps stay."""
import functools

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import (PAMR, Boundary, Despeckle, ImageTransform, SegEvaluator, SegInference, TestAug,
                                      boundary_areas, boundary_bands, preprocess, refine_labels)
from segclip_amd.train import eval_epoch
from tests import boundary_reference as br
from tests import kernel_frames as kf
from tests import pamr_reference as pr
from tests.helpers import CountedEncodeImage, load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SH, TW = ops.SEG_BOUNDARY_TILE
CASES = br.cases(SH, TW)
ROWS = [(name, d) for name, (_, radii) in CASES.items() for d in radii]
ERR_INVALID, ERR_UNSUPPORTED = -1, -2


@functools.lru_cache(maxsize=None)
def ref_band(name, d, flipped=False):
    m = CASES[name][0]
    return br.band(m[::-1, ::-1].copy() if flipped else m, d)


def _cat(xs):
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(x).reshape(-1) for x in xs]))


class Run:
    """One call of ops.seg_boundary on framed buffers.  The predictions lie one after the other with `gap` unused bytes
    between them, the ground truths with `gt_gap`: offsets that are no multiples of 4, and the two sides' offsets differ."""

    def __init__(self, preds, radii, gts=None, gap=3, gt_gap=5, C=1, ignore_index=255, reduce_zero=False,
                 outputs=("pred_band", "gt_band", "areas")):
        self.sizes, self.radii, self.C = [tuple(m.shape) for m in preds], list(radii), C

        def lay(maps, gap):
            offs, n = [], 0
            for m in maps:
                offs.append(n)
                n += m.size + gap
            n -= gap
            f = kf.Frame((n,), torch.uint8)
            f.v.fill_(0xEE)
            used = torch.zeros(n, dtype=torch.bool)
            for m, o in zip(maps, offs):
                f.v[o:o + m.size] = torch.from_numpy(m.copy()).reshape(-1).to(DEV)
                used[o:o + m.size] = True
            return f, offs, used

        self.fpred, self.offs, self.used = lay(preds, gap)
        self.fgt = self.gt_offs = self.gt_used = None
        if gts is not None:
            self.fgt, self.gt_offs, self.gt_used = lay(gts, gt_gap)
        self.in_bits = [f.bits() for f in (self.fpred, self.fgt) if f is not None]
        self.fpb = kf.Frame((self.fpred.v.numel(),), torch.uint8) if "pred_band" in outputs else None
        self.fgb = kf.Frame((self.fgt.v.numel(),), torch.uint8) if "gt_band" in outputs and gts is not None else None
        self.fareas = kf.Frame((2, 3, C), torch.int64) if "areas" in outputs and gts is not None else None
        self.clear_areas()
        self.table, self.n_blocks, self.side = ops.seg_boundary_table(self.sizes, self.offs, self.gt_offs, self.radii, DEV)
        v = lambda f: None if f is None else f.v
        self.call = lambda table=self.table: ops.seg_boundary(
            table, self.n_blocks, self.fpred.v, gt=v(self.fgt), num_classes=C, ignore_index=ignore_index,
            reduce_zero_label=reduce_zero, pred_band=v(self.fpb), gt_band=v(self.fgb), areas=v(self.fareas), max_side=self.side)

    def clear_areas(self):
        if self.fareas is not None:
            self.fareas.v.zero_()

    def frames(self):
        return [f for f in (self.fpb, self.fgb, self.fareas) if f is not None]

    def run(self, **kw):
        self.call(**kw)
        torch.cuda.synchronize()
        self.check_frames()
        return self

    def check_frames(self):
        assert all(f.intact() for f in self.frames()), "wrote outside an output"
        assert all(torch.equal(a, f.bits()) for a, f in zip(self.in_bits, (self.fpred, self.fgt))), "an input changed"

    def check_bands(self, pred_bands, gt_bands=None, images=None, gt_images=None):
        """torch.equal against the restatement; images: the maps that the table really describes (default: all), gt_images:
        those of them with a ground truth (default: the same).  Everything else of the band buffers, the bytes between two
        maps included, keeps the frame's fill."""
        images = list(range(len(self.sizes))) if images is None else images
        gt_images = images if gt_images is None else gt_images
        for f, offs, want, images in ((self.fpb, self.offs, pred_bands, images), (self.fgb, self.gt_offs, gt_bands, gt_images)):
            if f is None:
                continue
            got, used = f.v.cpu(), torch.zeros(f.v.numel(), dtype=torch.bool)
            for k in images:
                used[offs[k]:offs[k] + self.sizes[k][0] * self.sizes[k][1]] = True
            assert torch.equal(got[used], _cat([want[k] for k in images])), "a band differs from the restatement"
            assert bool((got[~used] == f.fill).all()), "a band written outside the maps of the table"


# ------------------------------------------------------------------------------------------------ 1. every map, every radius
@pytest.mark.parametrize("name,d", ROWS)
def test_bands_against_the_restatement(name, d):
    m = CASES[name][0]
    r = Run([m], [d], gts=[m[::-1, ::-1].copy()], outputs=("pred_band", "gt_band")).run()
    r.check_bands([ref_band(name, d)], [ref_band(name, d, True)])
    # the prediction's band alone: no ground truth, no workspace for one
    r = Run([m], [d], outputs=("pred_band",)).run()
    r.check_bands([ref_band(name, d)])


def test_mixed_call():
    maps, radii = br.mixed_call()
    gts = [np.ascontiguousarray(m.T).reshape(m.shape) for m in maps]
    r = Run(maps, radii, gts=gts, outputs=("pred_band", "gt_band")).run()
    assert all((b - a - m.size) % 4 for a, b, m in zip(r.offs, r.offs[1:], maps)), "a gap is a multiple of 4"
    assert all(a != b for a, b in zip(r.offs[1:], r.gt_offs[1:]))
    r.check_bands([br.band(m, d) for m, d in zip(maps, radii)], [br.band(g, d) for g, d in zip(gts, radii)])
    snap = [f.bits() for f in r.frames()]
    for f in r.frames():
        f.buf.fill_(f.fill)
    r.run()
    assert all(torch.equal(a, f.bits()) for a, f in zip(snap, r.frames())), "the second call differs"


# ------------------------------------------------------------------------------------------------ 2. areas
AREA_SIZES, AREA_RADII = [(37, 70), (70, 133), (1, 1)], [3, 5, 1]


@functools.lru_cache(maxsize=None)
def area_maps(C):
    rng = np.random.default_rng(100 + C)
    labels = {1: (0, 1, 2), 21: (0, 1, 2, 3, 19, 20, 21, 22, 200), 256: (0, 1, 2, 100, 254)}[C]
    pairs = [br.area_pair(rng, h, w, labels) for (h, w) in AREA_SIZES]
    return [p for p, _ in pairs], [g for _, g in pairs]


@pytest.mark.parametrize("reduce_zero", [False, True])
@pytest.mark.parametrize("C", [1, 21, 256])
def test_areas_against_the_restatement(C, reduce_zero):
    preds, gts = area_maps(C)
    want = torch.from_numpy(br.areas(preds, gts, AREA_RADII, C, 255, reduce_zero))
    assert int(want[0].sum()) > 0 and int(want[1].sum()) > 0
    r = Run(preds, AREA_RADII, gts=gts, C=C, reduce_zero=reduce_zero).run()
    assert torch.equal(r.fareas.v.cpu(), want)
    r.check_bands([br.band(m, d) for m, d in zip(preds, AREA_RADII)], [br.band(m, d) for m, d in zip(gts, AREA_RADII)])
    r.run()                                        # areas are added to
    assert torch.equal(r.fareas.v.cpu(), 2 * want)
    # the areas alone
    r = Run(preds, AREA_RADII, gts=gts, C=C, reduce_zero=reduce_zero, outputs=("areas",)).run()
    assert torch.equal(r.fareas.v.cpu(), want)


@pytest.mark.parametrize("reduce_zero", [False, True])
@pytest.mark.parametrize("C", [1, 21, 256])
def test_identities_on_the_device(C, reduce_zero):
    preds, gts = area_maps(C)
    preds, gts = [preds[0], preds[2]], [gts[0], gts[2]]
    # radius >= the larger side: slot 0 is ops.seg_areas; gapless layouts, so that the plain kernel sees the same pixels
    r = Run(preds, [70, 128], gts=gts, gap=0, gt_gap=0, C=C, reduce_zero=reduce_zero, outputs=("areas",)).run()
    plain = ops.seg_areas(r.fpred.v, r.fgt.v, C, reduce_zero_label=reduce_zero)
    assert torch.equal(r.fareas.v[0], plain) and int(plain.sum()) > 0
    # a ground truth of one byte: the trimap stays empty, Boundary IoU's label band is the frame
    flat = [np.full_like(g, 2) for g in gts]
    r = Run(preds, [3, 1], gts=flat, C=C, reduce_zero=reduce_zero, outputs=("areas",)).run()
    assert int(r.fareas.v[1].abs().sum()) == 0
    assert torch.equal(r.fareas.v.cpu(), torch.from_numpy(br.areas(preds, flat, [3, 1], C, 255, reduce_zero)))


def test_a_map_without_a_ground_truth_counts_nothing():
    preds, gts = area_maps(21)
    r = Run(preds, AREA_RADII, gts=gts, C=21)
    table = r.table.clone()
    table[1, 3] = -1
    r.run(table=table)
    keep = [0, 2]
    want = br.areas([preds[k] for k in keep], [gts[k] for k in keep], [AREA_RADII[k] for k in keep], 21)
    assert torch.equal(r.fareas.v.cpu(), torch.from_numpy(want))
    # every prediction has its band, the ground truths of the other two theirs
    r.check_bands([br.band(m, d) for m, d in zip(preds, AREA_RADII)], [br.band(m, d) for m, d in zip(gts, AREA_RADII)],
                  gt_images=keep)


# ------------------------------------------------------------------------------------------------ 3. table rows
def test_a_bad_table_row_is_skipped():
    maps, radii = br.mixed_call()
    gts = [m[::-1].copy() for m in maps]
    bands = [br.band(m, d) for m, d in zip(maps, radii)]
    gt_bands = [br.band(m, d) for m, d in zip(gts, radii)]
    probe = Run(maps, radii, gts=gts, C=3)
    n_pred, n_gt = probe.fpred.v.numel(), probe.fgt.v.numel()
    rows = [(1, 0, 0), (1, 1, 1 << 15), (2, 0, probe.side + 1), (2, 2, n_pred - 10), (0, 2, -1), (2, 3, n_gt - 10), (1, 3, -2),
            (2, 4, 0), (2, 4, 129), (1, 4, -3), (3, 5, probe.n_blocks - 1)]
    for row, col, value in rows:
        r = Run(maps, radii, gts=gts, C=3)
        bad = r.table.clone()
        bad[row, col] = value
        r.run(table=bad)
        keep = [k for k in range(4) if k != row]
        r.check_bands(bands, gt_bands, images=keep)
        want = br.areas([maps[k] for k in keep], [gts[k] for k in keep], [radii[k] for k in keep], 3)
        assert torch.equal(r.fareas.v.cpu(), torch.from_numpy(want)), (row, col, value)


# ------------------------------------------------------------------------------------------------ 4. no synchronisation
def test_the_call_does_not_synchronise():
    preds, gts = area_maps(21)
    r = Run(preds, AREA_RADII, gts=gts, C=21).run()     # the library is loaded
    want = [f.bits() for f in r.frames()]
    for f in r.frames():
        f.buf.fill_(f.fill)
    r.clear_areas()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r.call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.equal(a, f.bits()) for a, f in zip(want, r.frames()))


# ------------------------------------------------------------------------------------------------ 5. return codes
def test_refusals_leave_the_outputs_untouched():
    lib = L.load()
    preds, gts = area_maps(21)
    r = Run(preds, AREA_RADII, gts=gts, C=21)
    for f in r.frames():
        f.buf.fill_(f.fill)
    n_pred, n_gt, B = r.fpred.v.numel(), r.fgt.v.numel(), len(r.sizes)
    ws_bytes = lib.segclip_seg_boundary_ws_bytes(n_pred, n_gt)
    assert 2 * (n_pred + n_gt) <= ws_bytes <= 2 * (n_pred + n_gt) + 512
    ws = kf.Frame((ws_bytes,), torch.uint8)

    def call(C=21, side=r.side, ws_n=ws_bytes, ws_p=ws.p, images=L.ptr(r.table), pred=r.fpred.p, gt=r.fgt.p, pred_band=r.fpb.p,
             gt_band=r.fgb.p, areas=r.fareas.p, n_blocks=r.n_blocks):
        rc = lib.segclip_seg_boundary(images, B, n_blocks, side, pred, n_pred, gt, n_gt, C, 255, 0, pred_band, gt_band, areas, ws_p,
                                      ws_n, L.stream())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return all(f.untouched() for f in r.frames()) and ws.untouched()

    for kw in (dict(C=257), dict(side=0), dict(side=1 << 15), dict(ws_n=ws_bytes - 1), dict(ws_n=0)):
        assert call(**kw) == ERR_UNSUPPORTED, kw
        assert lib.segclip_last_error_string().decode().startswith("seg_boundary"), kw
        assert untouched(), kw
    inside = lambda f, k: f.v.data_ptr() + k
    for kw in (dict(gt=None), dict(gt=None, areas=None), dict(pred_band=r.fpred.p), dict(pred_band=inside(r.fgt, 8)),
               dict(gt_band=inside(r.fpred, 100)), dict(gt_band=r.fgt.p), dict(gt_band=inside(r.fpb, n_pred - 1)), dict(images=None),
               dict(pred=None), dict(ws_p=None), dict(ws_p=ws.v.data_ptr() + 1), dict(C=0), dict(n_blocks=-1)):
        assert call(**kw) == ERR_INVALID, kw
        assert lib.segclip_last_error_string().decode().startswith("seg_boundary"), kw
        assert untouched(), kw
    assert lib.segclip_seg_boundary_ws_bytes(-1, 0) == ERR_UNSUPPORTED and lib.segclip_seg_boundary_ws_bytes(0, -1) == ERR_UNSUPPORTED
    # the wrapper
    with pytest.raises(L.Unsupported, match="257 classes"):
        ops.seg_boundary(r.table, r.n_blocks, r.fpred.v, gt=r.fgt.v, num_classes=257,
                         areas=torch.zeros(2, 3, 257, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.seg_boundary(r.table, r.n_blocks, r.fpred.v, pred_band=r.fpred.v)
    with pytest.raises(ValueError, match="gt_band and areas need gt"):
        ops.seg_boundary(r.table, r.n_blocks, r.fpred.v, num_classes=21, areas=r.fareas.v)
    with pytest.raises(ValueError, match=r"areas is a contiguous \(2, 3, 21\)"):
        ops.seg_boundary(r.table, r.n_blocks, r.fpred.v, gt=r.fgt.v, num_classes=21, areas=r.fareas.v[0])
    with pytest.raises(ValueError, match="pred_band has the layout of pred"):
        ops.seg_boundary(r.table, r.n_blocks, r.fpred.v, pred_band=r.fpb.v[:-1])
    with pytest.raises(ValueError, match="gt_band has the layout of gt"):
        ops.seg_boundary(r.table, r.n_blocks, r.fpred.v, gt=r.fgt.v, gt_band=r.fpb.v)
    with pytest.raises(ValueError, match="pred is a contiguous uint8"):
        ops.seg_boundary(r.table, r.n_blocks, r.fpred.v.int(), pred_band=r.fpb.v)
    with pytest.raises(ValueError, match="table is the"):
        ops.seg_boundary(r.table[:, :7].contiguous(), r.n_blocks, r.fpred.v, pred_band=r.fpb.v)
    with pytest.raises(ValueError, match="num_classes is positive"):
        ops.seg_boundary(r.table, r.n_blocks, r.fpred.v, pred_band=r.fpb.v, num_classes=0)
    assert untouched()
    # and the accepted call on the same frames, with a workspace of exactly ws_bytes
    r.clear_areas()
    assert call() == 0
    r.check_frames()
    assert ws.intact()
    r.check_bands([br.band(m, d) for m, d in zip(preds, AREA_RADII)], [br.band(m, d) for m, d in zip(gts, AREA_RADII)])
    assert torch.equal(r.fareas.v.cpu(), torch.from_numpy(br.areas(preds, gts, AREA_RADII, 21)))


# ------------------------------------------------------------------------------------------------ 6. the Python layer
def test_bands_and_areas_of_lists():
    preds, gts = area_maps(21)
    b = Boundary(radius=4)
    want = [br.band(m, 4) for m in preds]
    maps, truths = [torch.from_numpy(m).to(DEV) for m in preds], [torch.from_numpy(m).to(DEV) for m in gts]
    keep = [m.clone() for m in maps]
    got = boundary_bands(maps, b)
    assert [tuple(t.shape) for t in got] == AREA_SIZES and all(t.dtype == torch.uint8 for t in got)
    assert len({t.untyped_storage().data_ptr() for t in got}) == 1
    assert all(torch.equal(t.cpu(), torch.from_numpy(w)) for t, w in zip(got, want))
    # views of one buffer (what predict_raw returns) are used where they lie
    flat = torch.cat([m.reshape(-1) for m in maps])
    views, o = [], 0
    for m in maps:
        views.append(flat[o:o + m.numel()].view(m.shape))
        o += m.numel()
    again = boundary_bands(views, b)
    assert all(torch.equal(t.cpu(), torch.from_numpy(w)) for t, w in zip(again, want))
    # the ratio: one radius per map
    radii = [Boundary(ratio=0.05).radius_of(h, w) for (h, w) in AREA_SIZES]
    assert radii == [4, 8, 1]
    got = boundary_bands(maps, Boundary(ratio=0.05))
    assert all(torch.equal(t.cpu(), torch.from_numpy(br.band(m, d))) for t, m, d in zip(got, preds, radii))
    areas = boundary_areas(maps, truths, 21, Boundary(ratio=0.05), reduce_zero_label=True)
    ref = torch.from_numpy(br.areas(preds, gts, radii, 21, 255, True))
    assert areas.is_cuda and areas.dtype == torch.int64 and torch.equal(areas.cpu(), ref)
    assert boundary_areas(views, truths, 21, Boundary(ratio=0.05), reduce_zero_label=True, areas=areas) is areas
    assert torch.equal(areas.cpu(), 2 * ref)
    other = boundary_areas(maps, truths, 21, b, ignore_index=2)
    assert torch.equal(other.cpu(), torch.from_numpy(br.areas(preds, gts, [4, 4, 4], 21, 2, False)))
    assert all(torch.equal(a, k) for a, k in zip(maps, keep)), "the inputs changed"
    with pytest.raises(ValueError, match="label map"):
        boundary_bands([maps[0].int()], b)
    with pytest.raises(ValueError, match="3 predictions but 2 ground truths"):
        boundary_areas(maps, truths[:2], 21, b)
    with pytest.raises(ValueError, match="a ground truth has its label map's size"):
        boundary_areas(maps, [truths[1], truths[0], truths[2]], 21, b)
    with pytest.raises(ValueError, match="image 0 of 37x70 has the radius 158"):
        boundary_bands(maps, Boundary(ratio=2.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        boundary_bands([maps[0].cpu()], b)


# ------------------------------------------------------------------------------------------------ 7. end to end
TF = ImageTransform()
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(90, 120), (130, 101), (75, 75)]
OLD_KEYS = {"mIoU", "aAcc", "mAcc", "IoU", "Acc"}
NEW_KEYS = {"bIoU", "mbIoU", "trimap_IoU", "trimap_mIoU", "trimap_aAcc"}


def _raws(seed):
    g = torch.Generator().manual_seed(seed)
    raws = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in RAW_SIZES]
    gts = [torch.from_numpy(br._blocks(np.random.default_rng(seed + i), h, w, 13, tuple(range(14)))).to(DEV)
           for i, (h, w) in enumerate(RAW_SIZES)]
    for t in gts:
        t[5:9] = 255
    return raws, gts


def test_end_to_end():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        raws, gts = _raws(11)
        seg = SegInference(model, emb, True, bg_thresh=0.02, **SLIDE)
        C = seg.num_classes
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
        for name, path in paths.items():
            ev0 = SegEvaluator(seg, reduce_zero_label=True)
            ev = SegEvaluator(seg, reduce_zero_label=True, boundary=Boundary(radius=2))
            assert ev0.boundary_areas is None and tuple(ev.boundary_areas.shape) == (2, 3, C) and ev.boundary_areas.is_cuda
            with CountedEncodeImage(model) as plain_calls:
                assert path(ev0) is None
            with CountedEncodeImage(model) as calls:
                labels = path(ev, return_labels=True)
            assert calls == plain_calls and len(calls) > 0, name
            assert [tuple(t.shape) for t in labels] == RAW_SIZES, name
            assert torch.equal(ev.areas, ev0.areas) and int(ev.areas.sum()) > 0, name
            want = torch.from_numpy(br.areas([t.cpu().numpy() for t in labels], [t.cpu().numpy() for t in gts], [2] * 3, C, 255, True))
            assert torch.equal(ev.boundary_areas.cpu(), want) and int(want[0, 0].sum()) > 0 and int(want[1, 2].sum()) > 0, name
            # inside, the labels are kept even when the caller does not want them
            with CountedEncodeImage(model) as calls:
                assert path(ev) is None
            assert calls == plain_calls, name
            assert torch.equal(ev.areas, 2 * ev0.areas) and torch.equal(ev.boundary_areas.cpu(), 2 * want), name
            out, old = ev.compute(), ev0.compute()
            assert set(old) == OLD_KEYS and set(out) == OLD_KEYS | NEW_KEYS, name
            assert out["mIoU"] == old["mIoU"] and torch.equal(out["IoU"].nan_to_num(-1.0), old["IoU"].nan_to_num(-1.0)), name
            ref = SegEvaluator.boundary_metrics_from_areas(2 * want)
            assert out["mbIoU"] == ref["mbIoU"] and out["trimap_mIoU"] == ref["trimap_mIoU"] and out["trimap_aAcc"] == ref["trimap_aAcc"]
            assert tuple(out["bIoU"].shape) == (C,) and tuple(out["trimap_IoU"].shape) == (C,)
            assert 0.0 <= out["mbIoU"] <= 1.0 and 0.0 <= out["trimap_mIoU"] <= 1.0
            ev.reset()
            assert int(ev.areas.abs().sum()) == 0 and int(ev.boundary_areas.abs().sum()) == 0
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_eval_epoch():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        tokens = torch.from_numpy(g["prompt_ids"])
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        b = Boundary(radius=3)
        batches = []
        for k in range(2):
            raws, gts = _raws(40 + k)
            batches.append(([t.cpu() for t in raws[:2 + k]], [t.cpu() for t in gts[:2 + k]]))
        cfg = dict(bg_thresh=0.02, reduce_zero_label=True, **SLIDE)
        plain = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(cfg), transform=TF)
        assert isinstance(plain, float)
        assert plain == eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(boundary=None, **cfg), transform=TF)
        got = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(boundary=b, **cfg), transform=TF)
        seg = SegInference(model, emb, True, bg_thresh=0.02, **SLIDE)
        ev = SegEvaluator(seg, reduce_zero_label=True, boundary=b)
        for raws, gts in batches:
            ev.update_raw([t.to(DEV) for t in raws], [t.to(DEV) for t in gts], TF)
        want = ev.compute()
        assert set(got) == {"mIoU"} | NEW_KEYS and got["mIoU"] == plain
        for key in ("mbIoU", "trimap_mIoU", "trimap_aAcc"):
            assert got[key] == want[key] * 100.0 and 0.0 <= got[key] <= 100.0, key
        for key in ("bIoU", "trimap_IoU"):
            assert torch.equal(got[key].nan_to_num(-1.0), (want[key] * 100.0).nan_to_num(-1.0)), key
        # without a transform: update
        pre = [(preprocess([t.to(DEV) for t in raws], TF), gts) for raws, gts in batches]
        got = eval_epoch(None, model, DEV, 1, pre, tokens, True, dict(boundary=b, **cfg))
        assert set(got) == {"mIoU"} | NEW_KEYS
        with pytest.raises(TypeError, match="boundary is a Boundary"):
            eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(boundary=0.02, **cfg), transform=TF)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ 8. what the measure is for
def test_the_scene_mbiou_sees_the_border_that_miou_hardly_sees():
    raw, labels, gt = pr.snapping_scene()
    b = Boundary()
    d = b.radius_of(*gt.shape)
    assert d == 3
    raws, maps, gts = [raw.to(DEV)], [labels.to(DEV)], [gt.to(DEV)]
    refined = refine_labels(raws, maps, 3, TF, PAMR())
    figures = {}
    for name, m in (("before", maps), ("after", refined)):
        got = boundary_areas(m, gts, 3, b).cpu()
        assert torch.equal(got, torch.from_numpy(br.areas([m[0].cpu().numpy()], [gt.numpy()], [d], 3)))
        plain = ops.seg_areas(m[0], gts[0], 3).cpu()
        figures[name] = (SegEvaluator.boundary_metrics_from_areas(got)["mbIoU"], SegEvaluator.metrics_from_areas(plain)["mIoU"])
    print(f"the scene: mbIoU {figures['before'][0]:.4f} (mIoU {figures['before'][1]:.4f}) -> mbIoU {figures['after'][0]:.4f} "
          f"(mIoU {figures['after'][1]:.4f})")
    assert figures["before"][0] < figures["before"][1]
    assert figures["after"][0] > figures["before"][0]
