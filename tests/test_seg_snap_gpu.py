"""The superpixel and vote kernels (csrc/segment_superpixel.inc, csrc/segment_vote.inc) against the numpy restatement
(tests/superpixel_reference.py), with torch.equal and no tolerance: ids, centres and snapped maps; then superpixels,
snap_labels and snap= of predict_raw, update_raw and eval_epoch against the composition of the stand-alone functions."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import (PAMR, Boundary, Despeckle, ImageTransform, SegEvaluator, SegInference, SegSweepEvaluator,
                                      Segments, Snap, Superpixels, TestAug, boundary_areas, despeckle, refine_labels, snap_labels,
                                      superpixels)
from segclip_amd.train import eval_epoch
from tests import boundary_reference as br
from tests import pamr_reference as pr
from tests import superpixel_reference as sr
from tests.helpers import CountedEncodeImage, load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TF = ImageTransform()
ERR_UNSUPPORTED, ERR_INVALID = L.const("ERR_UNSUPPORTED"), L.const("ERR_INVALID")
SENTINEL = -0x54545455          # 0xAB in every byte of an int32
POINTS = [(4, 1, 8), (7, 1, 6), (16, 10, 5), (64, 64, 16), (16, 10, 0)]
NAMES = ["noise_37x53", "3x5", "1x200", "one_byte_40x40", "blocks_48x60", "scene_96x128", "crop_view_50x63"]


@functools.lru_cache(maxsize=None)
def _pictures():
    """The pictures of every superpixel case, on the device; the last one is a crop view of a larger tensor (strided rows)."""
    rng = np.random.default_rng(7)
    noise = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)   # noqa: E731
    host = [noise(37, 53), noise(3, 5), noise(1, 200), np.full((40, 40, 3), 93, dtype=np.uint8), sr.block_picture(),
            pr.snapping_scene()[0].numpy()]
    raws = [torch.from_numpy(p).to(DEV) for p in host]
    big = torch.from_numpy(noise(70, 90)).to(DEV)
    raws.append(big[5:55, 7:70])
    assert not raws[-1].is_contiguous() and raws[-1].stride(0) == 270
    return raws, host + [raws[-1].cpu().numpy()]


@functools.lru_cache(maxsize=None)
def _reference(S, m, T):
    """(ids, centres) of every picture, computed once per parameter point"""
    return [sr.slic(p, S, m, T) for p in _pictures()[1]]


def _padded_offsets(sizes, gap=37):
    offs, n = [], 11
    for h, w in sizes:
        offs.append(n)
        n += h * w + gap
    return offs, n


# ------------------------------------------------------------------------------------------------ 1. superpixels
@pytest.mark.parametrize("S,m,T", POINTS)
def test_superpixels_against_the_restatement(S, m, T):
    """all pictures in ONE call (mixed sizes, the first-workgroup and first-centre columns), the ids in a sentinel-filled buffer
    with padding between the images: ids and centres equal the restatement, nothing outside the maps is written"""
    raws, _ = _pictures()
    want = _reference(S, m, T)
    sizes = [tuple(r.shape[:2]) for r in raws]
    offs, n = _padded_offsets(sizes)
    table, n_blocks, side, counts = ops.seg_superpixels_table(raws, S, offs)
    assert counts == [c.shape[0] for _, c in want] and side == 200
    th, tw = ops.SEG_SP_TILE
    assert n_blocks == sum(-(-h // th) * -(-w // tw) for h, w in sizes) and table[:, 6].tolist() == list(
        itertools.accumulate([0] + [-(-h // th) * -(-w // tw) for h, w in sizes[:-1]]))
    ids = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    K = sum(counts)
    cen = torch.full((K + 2, 5), SENTINEL, dtype=torch.int32, device=DEV)
    ops.seg_superpixels(table, n_blocks, ids, K, S, m, T, centres=cen[1:K + 1], max_side=side)
    torch.cuda.synchronize()
    inside = torch.zeros(n, dtype=torch.bool, device=DEV)
    k0 = 0
    for name, (h, w), o, (wi, wc) in zip(NAMES, sizes, offs, want):
        inside[o:o + h * w] = True
        assert torch.equal(ids[o:o + h * w].view(h, w).cpu(), torch.from_numpy(wi)), f"{name} at {(S, m, T)}: ids differ"
        assert torch.equal(cen[1 + k0:1 + k0 + wc.shape[0]].cpu(), torch.from_numpy(wc)), f"{name} at {(S, m, T)}: centres differ"
        k0 += wc.shape[0]
    assert bool((ids[~inside] == SENTINEL).all()), "written outside the maps"
    assert bool((cen[0] == SENTINEL).all()) and bool((cen[K + 1] == SENTINEL).all()), "written outside the centres"
    # the public function: packed maps, the same ids and centres, and a second call gives the same bits
    seg = superpixels(raws, Superpixels(S, m, T), centres=True)
    assert seg.counts == counts and all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, (b, _) in zip(seg.maps, want))
    assert torch.equal(seg.centres, cen[1:K + 1]) and all(t.dtype == torch.int32 for t in seg.maps)
    again = superpixels(raws, Superpixels(S, m, T))
    assert again.centres is None and all(torch.equal(a, b) for a, b in zip(seg.maps, again.maps))


def test_cases_exercise_what_they_are_for():
    want = _reference(7, 1, 6)
    _, _, n = sr.slic(_pictures()[1][4], 7, 1, 6, with_counts=True)
    assert int((n == 0).sum()) >= 1, "the block picture has no empty cluster"
    assert _reference(16, 10, 5)[1][1].shape == (1, 5) and want[2][1].shape == (29, 5)
    one = _reference(16, 10, 0)[3][0]
    assert one[16, 0] == 0 and one[0, 16] == 0     # equal distances: the smallest index


def test_superpixel_refusals_leave_the_outputs_untouched():
    lib = L.load()
    raws = _pictures()[0][:2]
    table, n_blocks, side, counts = ops.seg_superpixels_table(raws, 8)
    K, n = sum(counts), 37 * 53 + 15
    ids = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    cen = torch.full((K, 5), SENTINEL, dtype=torch.int32, device=DEV)
    ws_bytes = lib.segclip_seg_superpixels_ws_bytes(K)
    assert ws_bytes >= K * 44
    ws = torch.full((ws_bytes,), 0xAB, dtype=torch.uint8, device=DEV)

    def call(S=8, m=10, T=2, side_=side, K_=K, ws_n=ws_bytes):
        rc = lib.segclip_seg_superpixels(L.ptr(table), 2, n_blocks, side_, S, m, T, L.ptr(ids), n, K_, L.ptr(cen), L.ptr(ws), ws_n,
                                         L.stream())
        torch.cuda.synchronize()
        return rc

    for kw in (dict(S=3), dict(S=65), dict(m=0), dict(m=65), dict(T=-1), dict(T=17), dict(side_=0), dict(side_=1 << 15),
               dict(ws_n=ws_bytes - 1), dict(K_=(1 << 28) + 1, ws_n=1 << 40)):
        assert call(**kw) == ERR_UNSUPPORTED, kw
        assert lib.segclip_last_error_string().decode().startswith("seg_superpixels"), kw
        assert bool((ids == SENTINEL).all()) and bool((cen == SENTINEL).all()) and bool((ws == 0xAB).all()), kw
    assert lib.segclip_seg_superpixels_ws_bytes(-1) == ERR_UNSUPPORTED
    assert lib.segclip_seg_superpixels_ws_bytes((1 << 28) + 1) == ERR_UNSUPPORTED
    # rows the device refuses are skipped: an id offset past the buffer, a first centre past K_total, a stride below 3 w
    for col, value in ((4, n - 10), (5, K), (3, 3 * 53 - 1)):
        bad = table.clone()
        bad[0, col] = value
        ids.fill_(SENTINEL)
        ops.seg_superpixels(bad, n_blocks, ids, K, 8, 10, 2, max_side=side)
        torch.cuda.synchronize()
        assert bool((ids[:37 * 53] == SENTINEL).all()), (col, value)
        assert torch.equal(ids[37 * 53:].cpu(), torch.from_numpy(sr.slic(_pictures()[1][1], 8, 10, 2)[0]).view(-1)), (col, value)
    with pytest.raises(ValueError, match="step"):
        ops.seg_superpixels(table, n_blocks, ids, K, 3, 10, 2)
    with pytest.raises(ValueError, match="centres"):
        ops.seg_superpixels(table, n_blocks, ids, K, 8, 10, 2, centres=cen[:-1])
    assert call() == 0 and not bool((ids[:37 * 53] == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ 2. the vote
VOTE_K = (1, 7, 5000)
VOTE_SIZE = (64, 80)


def _vote_inputs(C, wide, seed):
    """Three 64 x 80 maps with random ids of the caller's own, K = 1, 7 and 5000 (more pairs than the LDS stage holds), ids -1
    and K among them, and one hand-made 8 x 8 map: a segment split exactly 50 / 50, one without a voter, one with a 3 : 1
    majority and an unused id.  uint8 labels: 0 .. C - 1 and 255; 16-bit labels: values from {1, 257, 513, 1023} and 65535."""
    rng = np.random.default_rng(seed)
    dtype = np.uint16 if wide else np.uint8
    values = np.array([1, 257, 513, 1023, 65535] if wide else list(range(min(C, 255))) + [255])
    labels, segs = [], []
    for K in VOTE_K:
        lab = values[rng.integers(0, len(values), VOTE_SIZE)].astype(dtype)
        # blocks of labels as well as single pixels: runs of equal pairs and single pairs
        lab[8:40, 8:56] = values[rng.integers(0, len(values), (4, 6))].astype(dtype).repeat(8, axis=0).repeat(8, axis=1)
        seg = rng.integers(-1, K + 1, VOTE_SIZE).astype(np.int32)
        labels.append(lab)
        segs.append(seg)
    a, b = int(values[0]), int(values[1])
    top = int(values[-1])
    lab = np.empty((8, 8), dtype=dtype)
    seg = np.empty((8, 8), dtype=np.int32)
    lab[0:2, :4], lab[0:2, 4:], seg[0:2] = b, a, 0          # 8 : 8
    lab[2:4], seg[2:4] = top, 1                              # nobody votes
    lab[4:6, :6], lab[4:6, 6:], seg[4:6] = b, a, 2           # 12 : 4
    lab[6:8], seg[6] = a, -1
    seg[7] = 4                                               # K = 4: id 3 is unused, id 4 is out of range
    return labels + [lab], segs + [seg], list(VOTE_K) + [4]


@pytest.mark.parametrize("min_share", [0, 50, 51, 100])
@pytest.mark.parametrize("C,wide", [(2, False), (21, False), (256, False), (300, True), (1024, True)])
def test_vote_against_the_restatement(C, wide, min_share):
    labels, segs, counts = _vote_inputs(C, wide, 100 + C)
    want = [sr.vote(l, s, k, C, min_share) for l, s, k in zip(labels, segs, counts)]
    if C == 2 and min_share in (50, 51):   # the 50 / 50 segment decides >= against >
        assert (want[3][0:2] == want[3][0, 4]).all() == (min_share == 50)
    # (at 100 percent only a segment of one label snaps, to the label it has)
    assert (min_share == 100 or any((w != l).any() for w, l in zip(want, labels))) and (want[3][2:4] == labels[3][2:4]).all()
    tdt = torch.int16 if wide else torch.uint8
    dev_l = [torch.from_numpy(l.view(np.int16) if wide else l).to(DEV) for l in labels]
    dev_s = [torch.from_numpy(s).to(DEV) for s in segs]
    keep = [t.clone() for t in dev_l]
    got = snap_labels(dev_l, dev_s, C, counts=counts, min_share=min_share)
    assert all(g.dtype == tdt and tuple(g.shape) == l.shape for g, l in zip(got, labels))
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g.cpu(), torch.from_numpy(w.view(np.int16) if wide else w)), f"map {i} (K = {counts[i]}) differs"
    assert all(torch.equal(a, b) for a, b in zip(dev_l, keep)), "snap_labels changed its input"


def test_vote_writes_nothing_outside_the_maps():
    """the C ABI itself on sentinel-filled buffers with padding between the maps and a workspace of exactly ws_bytes"""
    lib = L.load()
    C = 21
    labels, segs, counts = _vote_inputs(C, False, 5)
    sizes = [l.shape for l in labels]
    offs, n = _padded_offsets(sizes)
    lab = torch.full((n,), 0xAB, dtype=torch.uint8, device=DEV)
    seg = torch.full((n,), 3, dtype=torch.int32, device=DEV)
    for o, l, s in zip(offs, labels, segs):
        lab[o:o + l.size] = torch.from_numpy(l).to(DEV).view(-1)
        seg[o:o + s.size] = torch.from_numpy(s).to(DEV).view(-1)
    table, n_blocks, total, top = ops.seg_vote_table(sizes, offs, counts, DEV)
    assert (total, top) == (sum(counts), 5000)
    ws_bytes = lib.segclip_seg_vote_ws_bytes(total, C)
    guard = 256
    ws = torch.full((ws_bytes + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    out = torch.full((n,), 0xCD, dtype=torch.uint8, device=DEV)

    def call(C_=C, share=50, max_k=top, total_=total, ws_n=ws_bytes, out_p=None, out_n=n):
        rc = lib.segclip_seg_vote(L.ptr(table), len(sizes), n_blocks, max_k, L.ptr(lab), n, L.ptr(seg), n, total_, C_, share,
                                  L.ptr(out) if out_p is None else out_p, out_n, L.ptr(ws[guard:]), ws_n, L.stream())
        torch.cuda.synchronize()
        return rc

    for kw in (dict(C_=0), dict(C_=257), dict(share=-1), dict(share=101), dict(max_k=0), dict(max_k=(1 << 20) + 1),
               dict(ws_n=ws_bytes - 1), dict(total_=(1 << 28) // C + 1, ws_n=1 << 40)):
        assert call(**kw) == ERR_UNSUPPORTED, kw
        assert lib.segclip_last_error_string().decode().startswith("seg_vote"), kw
        assert bool((out == 0xCD).all()) and bool((ws == 0xAB).all()), kw
    for kw in (dict(out_p=L.ptr(lab)), dict(out_p=ctypes.c_void_p(lab.data_ptr() + 8)), dict(out_n=n - 4)):
        assert call(**kw) == ERR_INVALID, kw
        assert bool((out == 0xCD).all()) and bool((ws == 0xAB).all()), kw
    assert lib.segclip_seg_vote_ws_bytes((1 << 28) // 300 + 1, 300) == ERR_UNSUPPORTED
    assert lib.segclip_seg_vote_ws_bytes(10, 1025) == ERR_UNSUPPORTED and lib.segclip_seg_vote_ws_bytes(10, 0) == ERR_UNSUPPORTED
    # an image whose K passes the caller's bound is skipped on the device, the others are voted
    assert call(max_k=4999) == 0
    inside = torch.zeros(n, dtype=torch.bool, device=DEV)
    for i, (o, l, s, k) in enumerate(zip(offs, labels, segs, counts)):
        inside[o:o + l.size] = True
        got = out[o:o + l.size].view(l.shape).cpu()
        if k == 5000:
            assert bool((got == 0xCD).all())
        else:
            assert torch.equal(got, torch.from_numpy(sr.vote(l, s, k, C, 50))), i
    assert call() == 0
    for i, (o, l, s, k) in enumerate(zip(offs, labels, segs, counts)):
        assert torch.equal(out[o:o + l.size].view(l.shape).cpu(), torch.from_numpy(sr.vote(l, s, k, C, 50))), i
    assert bool((out[~inside] == 0xCD).all()), "written outside the maps"
    assert bool((ws[:guard] == 0xAB).all()) and bool((ws[guard + ws_bytes:] == 0xAB).all()), "written outside the workspace"
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.seg_vote(table, n_blocks, lab, seg, total, C, out=lab)
    with pytest.raises(L.Unsupported, match="classes"):
        ops.seg_vote(table, n_blocks, lab, seg, total, 300)


def test_superpixel_segments_and_the_scene():
    """Segments from superpixels: a list of mixed sizes with random labels, and the snapping scene through the kernels:
    mIoU 0.8664 -> 1.0 with Snap()'s defaults"""
    raws, host = _pictures()
    rng = np.random.default_rng(3)
    labels = [rng.integers(0, 5, p.shape[:2]).astype(np.uint8) for p in host]
    for l in labels:
        l[0, 0] = 255
    sp = Superpixels(7, 1, 6)
    seg = superpixels(raws, sp)
    got = snap_labels([torch.from_numpy(l).to(DEV) for l in labels], seg, 5, min_share=30)
    for name, g, l, (ids, cen) in zip(NAMES, got, labels, _reference(7, 1, 6)):
        assert torch.equal(g.cpu(), torch.from_numpy(sr.vote(l, ids, cen.shape[0], 5, 30))), name
    raw, lab, gt = pr.snapping_scene()
    s = Snap()
    before = pr.miou(lab, gt, 3)
    out = snap_labels([lab.to(DEV)], superpixels([raw.to(DEV)], s.superpixels), 3, min_share=s.min_share)[0].cpu()
    after = pr.miou(out, gt, 3)
    print(f"snapping scene through the kernels: mIoU {before:.4f} -> {after:.4f}")
    assert round(before, 4) == 0.8664 and after == 1.0 and torch.equal(out, gt)


def test_the_calls_do_not_synchronise():
    raws, _ = _pictures()
    sizes = [tuple(r.shape[:2]) for r in raws]
    table, n_blocks, side, counts = ops.seg_superpixels_table(raws, 16)
    n, K = sum(h * w for h, w in sizes), sum(counts)
    ids = torch.empty(n, dtype=torch.int32, device=DEV)
    lab = torch.randint(0, 21, (n,), dtype=torch.uint8, device=DEV)
    offs = list(itertools.accumulate([0] + [h * w for h, w in sizes[:-1]]))
    vtable, v_blocks, total, top = ops.seg_vote_table(sizes, offs, counts, DEV)
    want_ids = ops.seg_superpixels(table, n_blocks, ids.clone(), K, 16, 10, 5, max_side=side)   # the library is loaded
    want = ops.seg_vote(vtable, v_blocks, lab, want_ids, total, 21, max_count=top)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.seg_superpixels(table, n_blocks, ids, K, 16, 10, 5, max_side=side)
        got = ops.seg_vote(vtable, v_blocks, lab, ids, total, 21, max_count=top)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(ids, want_ids) and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 3. the pipeline
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(90, 120), (130, 101), (75, 75)]
AUG, REFINE, CLEAN, BOUNDARY = TestAug(flip=True), PAMR(iters=2, dilations=(1, 2)), Despeckle(12), Boundary(radius=2)
SNAP = Snap(Superpixels(8, 10, 3), min_share=40)


@functools.lru_cache(maxsize=None)
def _setup():
    """(model, seg, raws, gts): built once, read by every case.  The pictures are smooth blobs plus noise, so that superpixels
    have something to follow."""
    model = tiny_seg_model()
    emb = torch.from_numpy(load_golden("seg_tiny.npz")["text_embedding"]).to(DEV)
    rng = np.random.default_rng(11)
    raws = []
    for i, (h, w) in enumerate(RAW_SIZES):
        blocks = br._blocks(np.random.default_rng(50 + i), h, w, 17, tuple(range(6)))
        colours = rng.integers(0, 256, (6, 3))
        pic = np.clip(colours[blocks] + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
        raws.append(torch.from_numpy(pic).to(DEV))
    gts = [torch.from_numpy(br._blocks(np.random.default_rng(11 + i), h, w, 13, tuple(range(14)))).to(DEV)
           for i, (h, w) in enumerate(RAW_SIZES)]
    for t in gts:
        t[5:9] = 255
    return model, SegInference(model, emb, True, bg_thresh=0.02, **SLIDE), raws, gts


@functools.lru_cache(maxsize=None)
def _composed(aug, refine, clean):
    """The maps of the stand-alone functions one after the other, snap included: predict_raw -> refine_labels -> snap_labels
    over superpixels -> despeckle, as clones that nothing writes to again; and the encode_image calls of the plain predict_raw."""
    model, seg, raws, gts = _setup()
    with CountedEncodeImage(model) as calls:
        maps = seg.predict_raw(raws, TF, aug=AUG if aug else None)
    calls = list(calls)
    if refine:
        maps = refine_labels(raws, maps, seg.num_classes, TF, REFINE)
    before = [m.clone() for m in maps]
    maps = snap_labels(maps, superpixels(raws, SNAP.superpixels), seg.num_classes, min_share=SNAP.min_share)
    assert any(not torch.equal(a, b) for a, b in zip(maps, before)), "the snap changes nothing: the case proves nothing"
    if clean:
        maps = despeckle(maps, CLEAN.min_area)
    return [m.clone() for m in maps], calls


@pytest.mark.parametrize("aug,refine,clean", list(itertools.product([False, True], repeat=3)))
def test_every_combination_of_stages_with_snap(aug, refine, clean):
    try:
        model, seg, raws, gts = _setup()
        C = seg.num_classes
        want, plain_calls = _composed(aug, refine, clean)
        assert len(plain_calls) > 0
        kw = dict(aug=AUG if aug else None, refine=REFINE if refine else None, clean=CLEAN if clean else None, snap=SNAP)
        want_areas = ops.seg_areas(torch.cat([m.reshape(-1) for m in want]), torch.cat([g.reshape(-1) for g in gts]), C,
                                   ignore_index=255, reduce_zero_label=True)
        assert int(want_areas[0].sum()) > 0
        with CountedEncodeImage(model) as calls:
            predicted = seg.predict_raw(raws, TF, **kw)
        assert calls == plain_calls
        assert [tuple(t.shape) for t in predicted] == RAW_SIZES and all(t.dtype == torch.uint8 for t in predicted)
        assert all(torch.equal(a, b) for a, b in zip(predicted, want)), "predict_raw differs from the composition"
        # one combination also with the boundary areas and the confusion matrix, on the maps that leave the chain
        extra = (aug, refine, clean) == (False, True, True)
        ev = SegEvaluator(seg, reduce_zero_label=True, boundary=BOUNDARY if extra else None, confusion=extra)
        with CountedEncodeImage(model) as calls:
            labels = ev.update_raw(raws, gts, TF, return_labels=True, **kw)
        assert calls == plain_calls
        assert all(torch.equal(a, b) for a, b in zip(labels, want)), "update_raw's labels differ from the composition"
        assert torch.equal(ev.areas, want_areas), "the areas are not those of the final maps, counted once"
        with CountedEncodeImage(model) as calls:
            assert ev.update_raw(raws, gts, TF, **kw) is None
        assert calls == plain_calls
        assert torch.equal(ev.areas, 2 * want_areas), "the call without return_labels counts other areas"
        if extra:
            want_b = boundary_areas(want, gts, C, BOUNDARY, reduce_zero_label=True)
            want_c = ops.seg_confusion(torch.cat([m.reshape(-1) for m in want]), torch.cat([g.reshape(-1) for g in gts]), C,
                                       ignore_index=255, reduce_zero_label=True)
            assert torch.equal(ev.boundary_areas, 2 * want_b) and int(want_b[0, 0].sum()) > 0
            assert torch.equal(ev.confusion, 2 * want_c) and int(want_c.sum()) > 0
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_snap_without_the_feature_flag_is_the_plain_path():
    """snap=None: the same maps and the same areas as the call without the argument"""
    try:
        model, seg, raws, gts = _setup()
        a, b = seg.predict_raw(raws, TF), seg.predict_raw(raws, TF, snap=None)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        e1, e2 = SegEvaluator(seg), SegEvaluator(seg)
        e1.update_raw(raws, gts, TF)
        e2.update_raw(raws, gts, TF, snap=None)
        assert torch.equal(e1.areas, e2.areas)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_eval_epoch_and_refusals_before_the_towers():
    g = load_golden("seg_tiny.npz")
    try:
        model, seg, raws, gts = _setup()
        tokens = torch.from_numpy(g["prompt_ids"])
        batches = [([t.cpu() for t in raws[:2]], [t.cpu() for t in gts[:2]]), ([raws[2].cpu()], [gts[2].cpu()])]
        cfg = dict(bg_thresh=0.02, reduce_zero_label=True, **SLIDE)
        got = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(snap=SNAP, **cfg), transform=TF)
        areas = torch.zeros(3, seg.num_classes, dtype=torch.int64, device=DEV)
        for rs, ts in batches:
            rs, ts = [t.to(DEV) for t in rs], [t.to(DEV) for t in ts]
            maps = snap_labels(seg.predict_raw(rs, TF), superpixels(rs, SNAP.superpixels), seg.num_classes, min_share=SNAP.min_share)
            for w, t in zip(maps, ts):
                ops.seg_areas(w, t, seg.num_classes, reduce_zero_label=True, areas=areas)
        assert got == SegEvaluator.metrics_from_areas(areas.cpu())["mIoU"] * 100.0 and 0.0 <= got <= 100.0
        plain = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(cfg), transform=TF)
        assert plain != got, "the snap changes no area: the case proves nothing"

        ev = SegEvaluator(seg)
        wide = SegInference(model, seg.text_embedding, True, bg_thresh=0.02, label_dtype=torch.int16, **SLIDE)
        pre = [torch.zeros(3, 128, 128, device=DEV)]
        with CountedEncodeImage(model) as calls:
            with pytest.raises(ValueError, match="snap.*transform"):
                eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(snap=SNAP, **cfg))
            with pytest.raises(ValueError, match="snap: out_shapes"):
                seg.predict_raw(raws, TF, out_shapes=[(h + 1, w) for (h, w) in RAW_SIZES], snap=SNAP)
            with pytest.raises(ValueError, match="snap: out_shapes"):
                ev.update_raw(raws, [t[:-1] for t in gts], TF, snap=SNAP)
            with pytest.raises(TypeError, match="snap is a Snap"):
                seg.predict_raw(raws, TF, snap=Superpixels())
            with pytest.raises(ValueError, match="predict_list.*snap"):
                seg.predict_list(pre, snap=SNAP)
            with pytest.raises(ValueError, match="update.*snap"):
                ev.update(pre, [gts[0]], snap=SNAP)
            with pytest.raises(ValueError, match="render_raw.*snap"):
                seg.render_raw(raws, TF, ["pred"], torch.zeros(14, 3, dtype=torch.uint8), snap=SNAP)
            with pytest.raises(ValueError, match="SegSweepEvaluator.*snap"):
                SegSweepEvaluator(seg, [0.1, 0.5]).update_raw(raws, gts, TF, snap=SNAP)
            with pytest.raises(ValueError, match="predict_raw.*snap.*16-bit"):
                wide.predict_raw(raws, TF, snap=SNAP)
            with pytest.raises(ValueError, match="update_raw.*snap.*16-bit"):
                SegEvaluator(wide).update_raw(raws, [t.to(torch.int16) for t in gts], TF, snap=SNAP)
        assert calls == [] and int(ev.areas.sum()) == 0
        # the chain for a wide vocabulary: predict_raw -> snap_labels -> despeckle on the int16 maps
        maps16 = wide.predict_raw(raws, TF)
        snapped = snap_labels(maps16, superpixels(raws, SNAP.superpixels), seg.num_classes, min_share=SNAP.min_share)
        narrow = snap_labels(seg.predict_raw(raws, TF), superpixels(raws, SNAP.superpixels), seg.num_classes, min_share=SNAP.min_share)
        assert all(a.dtype == torch.int16 and torch.equal(a.to(torch.uint8), b) for a, b in zip(snapped, narrow))
        assert all(t.dtype == torch.int16 for t in despeckle(snapped, 12))
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
