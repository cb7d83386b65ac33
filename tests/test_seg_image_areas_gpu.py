"""GPU: the per-image areas of label maps - segclip_seg_image_areas / segclip_seg_image_areas_wide (csrc/segment_image_areas.inc)
through ops.seg_image_areas and segmentation.image_areas, SegEvaluator(per_image=True) on every update path and
eval_epoch(test_cfg={"per_image": True}) - held to tests/image_areas_reference.py with torch.equal: every count is an integer.
Beside the reference, row i is ops.seg_areas / seg_areas_wide of picture i alone and the rows sum to that op on all pictures.
The fp64 figures of compute() are compared at 1e-12 relative (sums of a few values in [0, 1])."""
import functools
import itertools

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import (PAMR, Despeckle, ImageTransform, SegEvaluator, SegInference, Snap, Superpixels, TestAug,
                                      image_areas, preprocess)
from segclip_amd.train import eval_epoch
from tests import confusion_reference as cr
from tests import image_areas_reference as ir
from tests import kernel_frames as kf
from tests.helpers import load_golden, tiny_seg_model
from tests.test_seg_confusion_gpu import RULES, _to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I16 = torch.uint8, torch.int16
T = ops.SEG_IA_TILE
# pixels of the pictures: shorter than a 16-byte vector, around one, a tail, around one tile, several tiles
SIZES = (1, 15, 17, 255, T - 1, T, T + 1, 2 * T + 3, 300007)
SMALL = (1, 15, 17, 255, T + 1)   # the list on which a class count meets every rule
PADS = (0, 1, 3, 7)               # elements between two pictures: a picture starts at any element
CLASSES = {U8: (1, 2, 21, 256), I16: (21, 257, 460, 1024)}
RTOL = 1e-12


def _top(dtype):
    return 255 if dtype == U8 else 65535


@functools.lru_cache(maxsize=None)
def _pictures(kind, C, dtype, sizes):
    """[(pred, gt)] as arrays of unsigned values, one pair per size; 16-bit maps also hold values with the top bit set"""
    out = []
    for k, n in enumerate(sizes):
        rng = np.random.default_rng(1000 * C + 10 * k + (7 if kind == "blocky" else 0))
        pred, gt = cr.blocky_pair(rng, n, C) if kind == "blocky" else cr.random_pair(rng, n, C, _top(dtype))
        if dtype == I16:
            pred[3::13], gt[1::17], gt[5::29] = 40000, 65535, 32768
        out.append((pred, gt))
    return out


@functools.lru_cache(maxsize=None)
def _want(kind, C, dtype, sizes, ignore_index, reduce_zero):
    pics = _pictures(kind, C, dtype, sizes)
    return torch.from_numpy(ir.image_areas([p for p, _ in pics], [g for _, g in pics], C, ignore_index, reduce_zero))


def _flat(arrays, dtype, pads, base):
    """the arrays in one device buffer that starts `base` elements after an aligned address, pads[i % len] elements of another
    value before array i -> (buffer, offsets)"""
    offs, n = [], 0
    for a, pad in zip(arrays, itertools.cycle(pads)):
        offs.append(n + pad)
        n += pad + len(a)
    values = np.full(n, 1, np.int64)
    for o, a in zip(offs, arrays):
        values[o:o + len(a)] = a
    return _to_dev(values, dtype, base), offs


def _areas(pred, gt, C, ignore_index, reduce_zero):
    return (ops.seg_areas if pred.dtype == U8 else ops.seg_areas_wide)(pred, gt, C, ignore_index, reduce_zero)


def _check_list(pics, dtype, C, rule, want, what, singles):
    preds, gts = [p for p, _ in pics], [g for _, g in pics]
    counts = [len(p) for p in preds]
    # one call of all pictures, each starting at another residue of 16 bytes, pred and gt independently
    for base_p, base_g, pads_p, pads_g in ((0, 0, PADS, PADS[::-1]), (1, 3, PADS[1:] + PADS[:1], PADS), (7, 0, (0,), PADS)):
        pred, po = _flat(preds, dtype, pads_p, base_p)
        gt, go = _flat(gts, dtype, pads_g, base_g)
        table, n_blocks = ops.seg_image_areas_table(po, go, counts, DEV)
        assert n_blocks == sum(-(-n // T) for n in counts)
        out = ops.seg_image_areas(pred, gt, table, n_blocks, C, *rule)
        assert out.dtype == torch.int64 and tuple(out.shape) == (len(pics), 3, C) and out.is_cuda and out.is_contiguous(), what
        assert torch.equal(out.cpu(), want), f"{what}: bases ({base_p}, {base_g})"
    # the identities, on the last layout: row i is seg_areas of picture i alone, the rows sum to seg_areas of all pictures
    alone = [_areas(pred[a:a + n], gt[b:b + n], C, *rule) for a, b, n in zip(po, go, counts)]
    assert torch.equal(out, torch.stack(alone)), f"{what}: row i is not seg_areas of picture i"
    together = _areas(torch.cat([pred[a:a + n] for a, n in zip(po, counts)]), torch.cat([gt[b:b + n] for b, n in zip(go, counts)]), C, *rule)
    assert torch.equal(out.sum(0), together), f"{what}: the rows do not sum to seg_areas"
    # the label kernels' layout through segmentation.image_areas: separate maps are copied to offsets that are multiples of 4
    maps = [_to_dev(p, dtype, 0).view(1, -1) for p in preds]
    truths = [_to_dev(g, dtype, 0).view(1, -1) for g in gts]
    assert torch.equal(image_areas(maps, truths, C, *rule).cpu(), want), f"{what}: multiples of 4"
    if singles:   # single-picture calls, the picture at element 3 of pred and element 1 of gt
        for i, (p, g) in enumerate(pics):
            table, n_blocks = ops.seg_image_areas_table([3], [1], [len(p)], DEV)
            one = ops.seg_image_areas(_to_dev(np.concatenate([[9, 9, 9], p]), dtype, 0), _to_dev(np.concatenate([[9], g]), dtype, 0),
                                      table, n_blocks, C, *rule)
            assert torch.equal(one.cpu(), want[i:i + 1]), f"{what}: picture {i} alone"


def _case_ids():
    return [(dtype, C) for dtype in (U8, I16) for C in CLASSES[dtype]]


@pytest.mark.parametrize("dtype,C", _case_ids(), ids=lambda v: str(v).replace("torch.", ""))
def test_kernel_against_reference(dtype, C):
    """Both kinds of map over every size with one rule each (the rule changes with the class count), and every rule of RULES
    over the short list.  Exact equality with the reference, and the identities with seg_areas."""
    rules = RULES[dtype]
    first = CLASSES[dtype].index(C)
    for k, kind in enumerate(("blocky", "random")):
        rule = rules[(2 * first + k) % len(rules)]
        want = _want(kind, C, dtype, SIZES, *rule)
        assert int(want.sum()) > 0
        _check_list(_pictures(kind, C, dtype, SIZES), dtype, C, rule, want, f"C={C} {kind} rule {rule}", singles=True)
    for k, rule in enumerate(rules):
        kind = ("blocky", "random")[k % 2]
        _check_list(_pictures(kind, C, dtype, SMALL), dtype, C, rule, _want(kind, C, dtype, SMALL, *rule),
                    f"C={C} {kind} rule {rule} (short list)", singles=False)


def test_out_of_range_values_occur_on_both_sides():
    """what the cases above rely on: values >= C in predictions and ground truths, and 16-bit values with the top bit set"""
    for dtype, C in ((U8, 21), (I16, 257)):
        pics = _pictures("random", C, dtype, SIZES)
        assert any((p >= C).any() for p, _ in pics) and any((g >= C).any() for _, g in pics)
    assert any((p >= 32768).any() and (g >= 32768).any() for p, g in _pictures("blocky", 21, I16, SIZES))


@pytest.mark.parametrize("dtype,C", [(U8, 21), (I16, 460)], ids=lambda v: str(v).replace("torch.", ""))
def test_accumulation(dtype, C):
    """A second call on the same `out` doubles it, a non-zero `out` is added to, two launches are bit-equal, and nothing outside
    the (B, 3, C) elements of a framed tensor is written."""
    rule = (_top(dtype), True)
    pics = _pictures("blocky", C, dtype, SIZES)
    want = _want("blocky", C, dtype, SIZES, *rule).to(DEV)
    pred, po = _flat([p for p, _ in pics], dtype, PADS, 1)
    gt, go = _flat([g for _, g in pics], dtype, (0,), 0)
    table, n_blocks = ops.seg_image_areas_table(po, go, [len(p) for p, _ in pics], DEV)
    frame = kf.Frame((len(pics), 3, C), torch.int64)
    frame.v.zero_()
    assert frame.v.is_contiguous()
    assert ops.seg_image_areas(pred, gt, table, n_blocks, C, *rule, out=frame.v).data_ptr() == frame.v.data_ptr()
    torch.cuda.synchronize()
    assert frame.intact(), "written outside the tensor"
    assert torch.equal(frame.v, want) and torch.equal(ops.seg_image_areas(pred, gt, table, n_blocks, C, *rule), want)
    ops.seg_image_areas(pred, gt, table, n_blocks, C, *rule, out=frame.v)
    assert torch.equal(frame.v, 2 * want) and frame.intact()
    start = torch.arange(want.numel(), dtype=torch.int64, device=DEV).view_as(want) * 3 + 5
    out = start.clone()
    ops.seg_image_areas(pred, gt, table, n_blocks, C, *rule, out=out)
    assert torch.equal(out, start + want)
    # no pictures or no workgroups: nothing is launched
    none = ops.seg_image_areas(pred, gt, table[:0], 0, C, *rule)
    assert tuple(none.shape) == (0, 3, C)
    out = start.clone()
    ops.seg_image_areas(pred, gt, table, 0, C, *rule, out=out)
    assert torch.equal(out, start)


@pytest.mark.parametrize("dtype", [U8, I16], ids=lambda v: str(v).replace("torch.", ""))
def test_bad_table_rows_are_skipped(dtype):
    """The device checks every row: a picture whose row is inconsistent is skipped and its output row stays as it was, every
    other row is exact.  Every bad row is refused by a range check before anything of it is read."""
    C, rule = 21, (_top(dtype), False)
    sizes = (T + 1, 2 * T + 3, 17, T, 255)
    pics = _pictures("blocky", C, dtype, sizes)
    want = _want("blocky", C, dtype, sizes, *rule).to(DEV)
    pred, po = _flat([p for p, _ in pics], dtype, PADS, 0)
    gt, go = _flat([g for _, g in pics], dtype, (0,), 0)
    table, n_blocks = ops.seg_image_areas_table(po, go, list(sizes), DEV)
    good = table.tolist()
    assert [r[3] for r in good] == [0, 2, 5, 6, 7] and n_blocks == 8
    bad_rows = {
        "a prediction offset past the buffer": (1, [pred.numel() - sizes[1] + 1, good[1][1], sizes[1], 2]),
        "a ground-truth offset past the buffer": (4, [good[4][0], gt.numel() - 254, 255, 7]),
        "a huge offset": (2, [1 << 62, good[2][1], 17, 5]),
        "a negative prediction offset": (0, [-1, good[0][1], sizes[0], 0]),
        "a negative ground-truth offset": (3, [good[3][0], -8, T, 6]),
        "a negative count": (2, [good[2][0], good[2][1], -17, 5]),
        "a count of 2^31": (2, [good[2][0], good[2][1], 1 << 31, 5]),
        "a first workgroup that runs backwards": (2, [good[2][0], good[2][1], 17, 1]),
        "a first workgroup of 0 in the last row": (4, [good[4][0], good[4][1], 255, 0]),
        "a negative first workgroup": (1, [good[1][0], good[1][1], sizes[1], -3]),
        "a first workgroup past the grid in the last row": (4, [good[4][0], good[4][1], 255, 8]),
    }
    for what, (i, row) in bad_rows.items():
        rows = [list(r) for r in good]
        rows[i] = row
        out = torch.full((len(sizes), 3, C), 7, dtype=torch.int64, device=DEV)
        ops.seg_image_areas(pred, gt, torch.tensor(rows, dtype=torch.int64, device=DEV), n_blocks, C, *rule, out=out)
        keep = [k for k in range(len(sizes)) if k != i]
        assert bool((out[i] == 7).all()), f"{what}: the bad picture's row was written"
        assert torch.equal(out[keep], want[keep] + 7), f"{what}: another picture's row is not exact"
    # a count of 0: the picture has no workgroup, the rows after it keep their first workgroups
    rows = [list(r) for r in good]
    rows[2] = [good[2][0], good[2][1], 0, 5]
    for r in rows[3:]:
        r[3] -= 1
    out = torch.full((len(sizes), 3, C), 7, dtype=torch.int64, device=DEV)
    ops.seg_image_areas(pred, gt, torch.tensor(rows, dtype=torch.int64, device=DEV), n_blocks - 1, C, *rule, out=out)
    assert bool((out[2] == 7).all()) and torch.equal(out[[0, 1, 3, 4]], want[[0, 1, 3, 4]] + 7), "a count of 0"
    torch.cuda.synchronize()


def test_refusals():
    lab8 = torch.zeros(64, dtype=U8, device=DEV)
    lab16 = torch.zeros(64, dtype=I16, device=DEV)
    table, n_blocks = ops.seg_image_areas_table([0], [0], [64], DEV)
    frame = kf.Frame((1, 3, 21), torch.int64)
    with pytest.raises(L.Unsupported, match="1..256 supported"):
        ops.seg_image_areas(lab8, lab8, table, n_blocks, 257)
    with pytest.raises(L.Unsupported, match="1..256 supported"):
        ops.seg_image_areas(lab8, lab8, table, n_blocks, 0)
    with pytest.raises(L.Unsupported, match="1..1024 supported"):
        ops.seg_image_areas(lab16, lab16, table, n_blocks, 1025)
    with pytest.raises(L.Unsupported, match="1..1024 supported"):
        ops.seg_image_areas(lab16, lab16, table, n_blocks, 0)
    with pytest.raises(ValueError, match="both uint8 or both int16"):
        ops.seg_image_areas(lab8, lab16, table, n_blocks, 21, out=frame.v)
    with pytest.raises(ValueError, match="both uint8 or both int16"):
        ops.seg_image_areas(lab8.int(), lab8.int(), table, n_blocks, 21, out=frame.v)
    with pytest.raises(ValueError, match="contiguous buffers"):
        ops.seg_image_areas(torch.zeros(128, dtype=U8, device=DEV)[::2], lab8, table, n_blocks, 21, out=frame.v)
    for bad in (torch.zeros(1, 3, 42, dtype=torch.int64, device=DEV)[:, :, ::2], torch.zeros(1, 3, 20, dtype=torch.int64, device=DEV),
                torch.zeros(2, 3, 21, dtype=torch.int64, device=DEV), torch.zeros(3, 21, dtype=torch.int64, device=DEV),
                torch.zeros(1, 3, 21, dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match=r"contiguous \(B, 3, C\) = \(1, 3, 21\) int64"):
            ops.seg_image_areas(lab8, lab8, table, n_blocks, 21, out=bad)
    for bad in (table.int(), table.view(-1), torch.zeros(1, 8, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match=r"\(B, 4\) int64 tensor of seg_image_areas_table"):
            ops.seg_image_areas(lab8, lab8, bad, n_blocks, 21, out=frame.v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_image_areas(lab8, lab8, table, n_blocks, 21, out=torch.zeros(1, 3, 21, dtype=torch.int64))
    with pytest.raises(ValueError, match="one dtype per list"):
        image_areas([lab8.view(8, 8), lab16.view(8, 8)], [lab8.view(8, 8)] * 2, 21)
    with pytest.raises(ValueError, match="a ground truth is an"):
        image_areas([lab8.view(8, 8)], [lab16.view(8, 8)], 21)
    with pytest.raises(ValueError, match="2 predictions but 1 ground truths"):
        image_areas([lab8.view(8, 8)] * 2, [lab8.view(8, 8)], 21)
    with pytest.raises(ValueError, match="its label map's size"):
        image_areas([lab8.view(8, 8)], [lab8.view(4, 16)], 21)
    torch.cuda.synchronize()
    assert frame.untouched(), "a refused call wrote or launched"


# ------------------------------------------------------------------------------------------------ end to end
TF = ImageTransform()
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(90, 120), (130, 101), (75, 75)]
OLD_KEYS = ["mIoU", "aAcc", "mAcc", "IoU", "Acc"]   # what compute() returns on the parent commit
FINE_KEYS = ["image_mIoU", "mIoU_I", "IoU_C", "mIoU_C", "mIoU_I_q", "mIoU_C_q"]
AGAIN = [2, 0]   # the pictures of the second update call: the rows follow the order in which the pictures were given


def _raws(seed, C, dtype=U8):
    """three decoded pictures and blocky ground truths over 0 .. C + 1 with a band of the dtype's ignore value"""
    g = torch.Generator().manual_seed(seed)
    raws = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=U8).to(DEV) for (h, w) in RAW_SIZES]
    gts = []
    for i, (h, w) in enumerate(RAW_SIZES):
        _, gt = cr.blocky_pair(np.random.default_rng(seed + i), h * w, C + 2)
        gt = gt.reshape(h, w)
        gt[5:9] = _top(dtype)
        gts.append(_to_dev(gt.reshape(-1), dtype, 0).view(h, w))
    return raws, gts


def _unsigned(t):
    t = t.cpu()
    return (t.long() & 0xFFFF).numpy() if t.dtype == I16 else t.numpy()


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern"
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok])), f"{what}: {got} != {want}"


def _check_compute(out, old, rows, what):
    assert list(old) == OLD_KEYS and list(out) == OLD_KEYS + FINE_KEYS, what
    assert out["mIoU"] == old["mIoU"] and torch.equal(out["IoU"].nan_to_num(-1.0), old["IoU"].nan_to_num(-1.0)), what
    ref = ir.fine_grained(rows)
    for key in ("image_mIoU", "IoU_C"):
        assert out[key].dtype == torch.float64 and not out[key].is_cuda
        _close(out[key].numpy(), ref[key], f"{what} {key}")
    for key in ("mIoU_I", "mIoU_C"):
        _close(out[key], ref[key], f"{what} {key}")
    for key in ("mIoU_I_q", "mIoU_C_q"):
        assert list(out[key]) == [0.05, 0.1]
        for q in (0.05, 0.1):
            _close(out[key][q], ref[key][q], f"{what} {key}[{q}]")
    assert SegEvaluator.worst_images(torch.from_numpy(rows), 2) == [(i, pytest.approx(s, rel=RTOL)) for i, s in ir.worst_images(rows, 2)]


def _run_paths(seg, paths, gts, rule, ignore_index):
    """paths: name -> call(evaluator, the indices of the pictures, **kw)"""
    C = seg.num_classes
    everything = list(range(len(gts)))
    for name, path in paths.items():
        ev0 = SegEvaluator(seg, **rule)
        ev = SegEvaluator(seg, per_image=True, **rule)
        assert ev0.image_areas is None and tuple(ev.image_areas.shape) == (0, 3, C) and ev.image_areas.is_cuda
        assert path(ev0, everything) is None and path(ev0, AGAIN) is None
        labels = path(ev, everything, return_labels=True)
        if labels is None:   # update_maps returns nothing: it scores the maps it is given
            labels = path.maps
        assert [tuple(t.shape) for t in labels] == RAW_SIZES, name
        rows = ev.image_areas
        assert rows.dtype == torch.int64 and tuple(rows.shape) == (len(gts), 3, C) and rows.is_cuda, name
        ref = ir.image_areas([_unsigned(t) for t in labels], [_unsigned(t) for t in gts], C, ignore_index, rule["reduce_zero_label"])
        assert np.array_equal(rows.cpu().numpy(), ref), name
        assert torch.equal(rows.sum(0), ev.areas) and int(ev.areas.sum()) > 0, name
        # inside, the labels are formed even when the caller does not want them; the new rows follow the old ones
        assert path(ev, AGAIN) is None
        assert torch.equal(ev.areas, ev0.areas), name
        rows = ev.image_areas
        ref = np.concatenate([ref, ref[AGAIN]])
        assert np.array_equal(rows.cpu().numpy(), ref) and torch.equal(rows.sum(0), ev.areas), name
        _check_compute(ev.compute(), ev0.compute(), ref, name)
        ev.reset()
        assert int(ev.areas.abs().sum()) == 0 and tuple(ev.image_areas.shape) == (0, 3, C), name


def _paths(raws, gts, pre, views, extra):
    def pick(things, idx):
        return [things[i] for i in idx]

    paths = {
        "update": lambda ev, idx, **kw: ev.update(pick(pre, idx), pick(gts, idx), **kw),
        "update_raw": lambda ev, idx, **kw: ev.update_raw(pick(raws, idx), pick(gts, idx), TF, **kw),
    }
    for name, stages in extra.items():
        paths["update_raw_" + name] = lambda ev, idx, stages=stages, **kw: ev.update_raw(pick(raws, idx), pick(gts, idx), TF, **stages, **kw)
    if views is not None:
        paths["update_views"] = lambda ev, idx, **kw: ev.update_views(pick(views, idx), pick(gts, idx), **kw)
    return paths


def _maps_path(seg, raws, gts):
    """update_maps over the label maps of predict_raw, as separate tensors (copied to multiples of 4) """
    maps = [m.clone() for m in seg.predict_raw(raws, TF)]

    def path(ev, idx, return_labels=False):
        return ev.update_maps([maps[i] for i in idx], [gts[i] for i in idx])

    path.maps = maps
    return path


def test_end_to_end():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.02, **SLIDE)
        raws, gts = _raws(11, seg.num_classes)
        pre = preprocess(raws, TF)
        views = [[(t, 0), (t.flip(-1).contiguous(), ops.SEG_FLIP_H)] for t in pre]
        stages = dict(aug=TestAug(flip=True), refine=PAMR(iters=2, dilations=(1, 2)), snap=Snap(Superpixels(8, 10, 3), min_share=40),
                      clean=Despeckle(12, fill=0))
        extra = {k: {k: v} for k, v in stages.items()}
        extra["all"] = stages
        paths = _paths(raws, gts, pre, views, extra)
        paths["update_maps"] = _maps_path(seg, raws, gts)
        _run_paths(seg, paths, gts, dict(reduce_zero_label=True), 255)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_end_to_end_int16():
    try:
        model = tiny_seg_model()
        e = torch.randn(300, 64, generator=torch.Generator().manual_seed(3))
        emb = (e / e.norm(dim=-1, keepdim=True)).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.0, label_dtype=I16, **SLIDE)
        assert seg.num_classes == 301
        raws, gts = _raws(12, seg.num_classes, I16)
        paths = _paths(raws, gts, preprocess(raws, TF), None, {})
        paths["update_maps"] = _maps_path(seg, raws, gts)
        _run_paths(seg, paths, gts, dict(ignore_index=65535, reduce_zero_label=False), 65535)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_with_the_other_outputs():
    """boundary=, confusion= and per_image= together: each sees the maps that leave the chain, and compute() carries all keys"""
    from segclip_amd.segmentation import Boundary
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        seg = SegInference(model, torch.from_numpy(g["text_embedding"]).to(DEV), True, bg_thresh=0.02, **SLIDE)
        raws, gts = _raws(13, seg.num_classes)
        ev = SegEvaluator(seg, reduce_zero_label=True, boundary=Boundary(radius=2), confusion=True, per_image=True)
        ev.update_raw(raws, gts, TF, clean=Despeckle(12, fill=0))
        assert torch.equal(ev.image_areas.sum(0), ev.areas) and torch.equal(SegEvaluator.areas_from_confusion(ev.confusion.cpu()), ev.areas.cpu())
        out = ev.compute()
        assert list(out)[:5] == OLD_KEYS and list(out)[-6:] == FINE_KEYS and {"mbIoU", "kappa", "confusion"} <= set(out)
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
        assert plain == eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(per_image=False, **cfg), transform=TF)
        got = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(per_image=True, **cfg), transform=TF)
        ev = SegEvaluator(seg, reduce_zero_label=True, per_image=True)
        for raws, gts in batches:
            ev.update_raw([t.to(DEV) for t in raws], [t.to(DEV) for t in gts], TF)
        want = ev.compute()
        assert list(got) == ["mIoU", "mIoU_I", "mIoU_C", "mIoU_I_q", "mIoU_C_q", "image_mIoU"] and got["mIoU"] == plain
        for key in ("mIoU_I", "mIoU_C"):
            assert got[key] == want[key] * 100.0 and 0.0 <= got[key] <= 100.0, key
        for key in ("mIoU_I_q", "mIoU_C_q"):
            assert list(got[key]) == [0.05, 0.1] and all(got[key][q] == want[key][q] * 100.0 for q in got[key]), key
        assert tuple(got["image_mIoU"].shape) == (5,) and torch.equal(got["image_mIoU"], want["image_mIoU"])
        assert got["mIoU_I_q"][0.05] == float(got["image_mIoU"].min()) * 100.0   # ceil(0.05 * 5) = 1: the worst picture
        both = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(per_image=True, confusion=True, **cfg), transform=TF)
        assert {"kappa", "confusion", "mIoU_I", "image_mIoU"} <= set(both) and both["mIoU_I"] == got["mIoU_I"]
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
