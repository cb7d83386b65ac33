"""GPU: despeckling by merging (csrc/segment_sieve.inc, segclip_seg_sieve) against the CPU restatement
tests/cc_merge_reference.py.  The definition (include/segclip_hip.h), restated: a component (those of segclip_seg_components) is
small when its area < min_area; its candidates are the kept components owning a pixel 4-adjacent to one of its pixels, whatever
the connectivity; the winner has the largest area, among equal areas the smallest label = the maximum of
(area << 8) | (255 - label); the small component takes the winner's label, without a candidate it is an orphan and keeps its
own; round r + 1 runs on the output of round r, and after the last round only the orphans become orphan_fill if one is given.
Everything is an integer, so every comparison is torch.equal.  The input and the output lie in frames (tests/kernel_frames.py):
nothing outside the maps' own pixels is written and the input stays as it is."""
import functools

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import (PAMR, Boundary, Despeckle, ImageTransform, SegEvaluator, SegInference, components, despeckle,
                                      refine_labels)
from segclip_amd.train import eval_epoch
from tests import cc_merge_reference as cm
from tests import cc_reference as cc
from tests import kernel_frames as kf
from tests.helpers import load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = ops.SEG_CC_TILE
CASES = cc.cases(TH, TW)
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
BOTH = pytest.mark.parametrize("connectivity", [4, 8])


def _cat(maps):
    return torch.from_numpy(np.concatenate([np.asarray(m).reshape(-1) for m in maps]))


@functools.lru_cache(maxsize=None)
def steps(name, connectivity, skip, min_area, rounds=3):
    """the restatement's chains of a case, computed once: per map [(map, orphans) after round 1 .. rounds]"""
    return [cm.chain(m, connectivity, skip, min_area, rounds) for m in CASES[name]]


def expected(name, connectivity, skip, min_area, orphan_fill, rounds):
    return _cat([cm.finish(s[rounds - 1], orphan_fill) for s in steps(name, connectivity, skip, min_area)])


class Run:
    """One call of ops.seg_sieve on framed buffers.  The maps lie one after the other (offsets that are no multiples of 4 where
    the sizes are not), `gap` unused bytes between them."""

    def __init__(self, maps, connectivity=8, skip=None, min_area=0, orphan_fill=None, rounds=1, gap=0):
        self.sizes = [tuple(m.shape) for m in maps]
        self.offs, n = [], 0
        for (h, w) in self.sizes:
            self.offs.append(n)
            n += h * w + gap
        n -= gap
        self.n = n
        self.used = torch.zeros(n, dtype=torch.bool)
        self.fin = kf.Frame((n,), torch.uint8)
        self.fin.v.fill_(0xEE)
        for m, o in zip(maps, self.offs):
            self.fin.v[o:o + m.size] = torch.from_numpy(np.ascontiguousarray(m)).reshape(-1).to(DEV)
            self.used[o:o + m.size] = True
        self.in_bits = self.fin.bits()
        self.fclean = kf.Frame((n,), torch.uint8)
        self.table, self.n_blocks, self.side = ops.seg_components_table(self.sizes, self.offs, DEV)
        self.kw = dict(connectivity=connectivity, skip_label=skip, min_area=min_area, orphan_fill=orphan_fill, rounds=rounds)

    def call(self, table=None, **kw):
        ops.seg_sieve(self.table if table is None else table, self.n_blocks, self.fin.v, cleaned=self.fclean.v, max_side=self.side,
                      **{**self.kw, **kw})

    def run(self, **kw):
        self.fclean.buf.fill_(self.fclean.fill)
        self.call(**kw)
        torch.cuda.synchronize()
        assert self.fclean.intact(), "wrote outside the output"
        assert torch.equal(self.in_bits, self.fin.bits()), "the input labels changed"
        return self

    def check(self, want, images=None):
        """torch.equal against the restatement; images: the maps that the table really describes (default: all)"""
        used = self.used
        if images is not None:
            used = torch.zeros_like(self.used)
            for k in images:
                used[self.offs[k]:self.offs[k] + self.sizes[k][0] * self.sizes[k][1]] = True
        got = self.fclean.v.cpu()
        assert torch.equal(got[used], want), "cleaned differs from the restatement"
        assert bool((got[~used] == self.fclean.fill).all()), "written outside the images of the table"
        return self

    def got(self, k=0):
        h, w = self.sizes[k]
        return self.fclean.v[self.offs[k]:self.offs[k] + h * w].view(h, w).cpu().numpy()


def sieve(a, connectivity=8, skip=None, min_area=0, orphan_fill=None, rounds=1):
    """one map through the kernels, checked against the restatement -> the cleaned map"""
    want = cm.merge(a, connectivity, skip, min_area, orphan_fill, rounds)
    r = Run([a], connectivity, skip, min_area, orphan_fill, rounds).run().check(_cat([want]))
    return r.got()


# ------------------------------------------------------------------------------------------------ 1. every map of the components' tests
@BOTH
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(name, connectivity):
    changed = 0
    for min_area in (3, 40):
        for rounds in (1, 3):
            for orphan_fill in (None, 200):
                want = expected(name, connectivity, None, min_area, orphan_fill, rounds)
                r = Run(CASES[name], connectivity, None, min_area, orphan_fill, rounds).run().check(want)
                changed += int((want != r.fin.v.cpu()[r.used]).sum())
    if name in ("noise_3_labels", "blocks_21_labels", "bytes_0_7_255", "mixed_batch", "tall_noise", "u_shapes"):
        assert changed > 0, "the case has nothing to merge"


def test_what_the_cases_show():
    """the 4-connected checkerboard consists of orphans (kept as they are, or all filled); three rounds differ from one on the
    noise; the offsets of the mixed batch are no multiples of 4"""
    board = CASES["checkerboard"][0]
    assert torch.equal(expected("checkerboard", 4, None, 3, None, 3), _cat([board]))
    assert bool((expected("checkerboard", 4, None, 3, 200, 1) == 200).all())
    assert not torch.equal(expected("noise_3_labels", 8, None, 40, None, 1), expected("noise_3_labels", 8, None, 40, None, 3))
    assert [o % 4 for o in Run(CASES["mixed_batch"]).offs] == [0, 3, 2, 1]


@BOTH
def test_mixed_batch_with_a_gap_between_the_maps(connectivity):
    r = Run(CASES["mixed_batch"], connectivity, None, 3, 200, 2, gap=5).run()
    assert r.offs[1] == 40
    want = _cat([cm.finish(s[1], 200) for s in steps("mixed_batch", connectivity, None, 3)])
    r.check(want)                                         # and the bytes between the maps keep the frame's fill


@BOTH
@pytest.mark.parametrize("name,skip", [("noise_3_labels", 0), ("bytes_0_7_255", 255)])
def test_skip_label(name, skip, connectivity):
    for rounds, orphan_fill in ((1, None), (2, 9)):
        want = expected(name, connectivity, skip, 5, orphan_fill, rounds)
        r = Run(CASES[name], connectivity, skip, 5, orphan_fill, rounds).run().check(want)
        skipped = _cat(CASES[name]) == skip
        assert int(skipped.sum()) > 0 and bool((r.fclean.v.cpu()[skipped] == skip).all())


# ------------------------------------------------------------------------------------------------ 2. where the vote can go wrong
@BOTH
def test_speck_at_a_tile_corner_between_four_kept_components(connectivity):
    a = cm.corner_speck(TH, TW)
    out = sieve(a, connectivity, None, 2)
    assert out[TH - 1, TW - 1] == 4 and int((out != a).sum()) == 1


@BOTH
def test_speck_across_two_tiles_sees_the_neighbour_of_the_second(connectivity):
    a = cm.speck_across_tiles(TH, TW)
    out = sieve(a, connectivity, None, 9)
    assert bool((out[:, TW - 2:TW + 2] == 2).all()) and int((out != a).sum()) == 8


@BOTH
def test_a_neighbour_whose_area_lies_in_far_tiles(connectivity):
    a = cm.serpentine_tail(TH, TW)
    out = sieve(a, connectivity, None, 2)
    zeros, ones = int((a == 0).sum()), int((a == 1).sum())
    y, x = np.argwhere(a == 7)[0]
    assert out[y, x] == (0 if zeros >= ones else 1) and 7 not in out


def test_equal_areas_give_the_smaller_label():
    a = cm.area_tie(TW - 1)                                # the speck is the last pixel of the first tile, the 3s lie in the second
    assert a.shape == (1, 2 * TW - 1) and a[0, TW - 1] == 9
    assert sieve(a, 8, None, 2)[0, TW - 1] == 3
    assert sieve(np.ascontiguousarray(a[:, ::-1]), 4, None, 2)[0, TW - 1] == 3
    assert sieve(np.ascontiguousarray(a.T), 4, None, 2)[TW - 1, 0] == 3


@BOTH
def test_a_diagonal_touch_is_no_contact(connectivity):
    a = cm.diagonal_only(TH, TW)
    out = sieve(a, connectivity, None, 2)
    assert out[TH, TW] == 9 and int((out != 0).sum()) == 1
    assert sieve(a, connectivity, None, 2, 33, 1)[TH, TW] == 33
    assert not sieve(a, connectivity, None, 2, 33, 2).any()


@BOTH
def test_specks_on_the_frame_and_beside_skipped_pixels(connectivity):
    a = cm.frame_and_skip()
    out = sieve(a, connectivity, 255, 4)
    assert out[15, 41] == 8 and bool((out[a == 255] == 255).all())
    assert sorted(np.unique(out).tolist()) == [1, 2, 8, 255]
    assert sieve(a, connectivity, 255, 4, 0, 1)[15, 41] == 0
    sieve(a, connectivity, None, 4)                        # without a skip label 255 is a class like any other


@BOTH
def test_nested_specks_need_two_rounds(connectivity):
    a = cm.nested_specks(2 * TH, 2 * TW, TH, TW)           # the ring lies around the corner of four tiles
    one = sieve(a, connectivity, None, 9)
    assert one[TH, TW] == 3 and int((one != 1).sum()) == 1
    assert bool((sieve(a, connectivity, None, 9, None, 2) == 1).all())
    assert sieve(a, connectivity, None, 9, 0, 1)[TH, TW] == 0


def test_width_one_and_height_one():
    for a in (cm.column(), cm.row()):
        for connectivity in (4, 8):
            out = sieve(a, connectivity, None, 3)
            assert sorted(np.unique(out).tolist()) == [1, 3]
            sieve(a, connectivity, 2, 3, 7, 2)


def test_areas_that_differ_above_bit_16():
    a = cm.key_above_bit_16()
    out = sieve(a, 8, None, 2)
    y, x = np.argwhere(a == 9)[0]
    assert out[y, x] == 3 and int((out != a).sum()) == 1


# ------------------------------------------------------------------------------------------------ 3. the call
@BOTH
@pytest.mark.parametrize("name", ["noise_3_labels", "mixed_batch"])
def test_two_calls_give_identical_bits(name, connectivity):
    r = Run(CASES[name], connectivity, None, 6, 7, 3).run()
    snap = r.fclean.bits()
    r.run()
    assert torch.equal(snap, r.fclean.bits()), f"{name}: the second call differs"


def test_the_call_does_not_synchronise():
    r = Run(CASES["mixed_batch"], 8, None, 6, 7, 3).run()          # the library is loaded
    want = r.fclean.bits()
    r.fclean.buf.fill_(r.fclean.fill)
    maps = [torch.from_numpy(m).to(DEV) for m in CASES["mixed_batch"]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r.call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    cleaned = despeckle(maps, 6, fill=7, merge=True, rounds=3)
    torch.cuda.synchronize()
    assert torch.equal(want, r.fclean.bits())
    assert torch.equal(torch.cat([c.reshape(-1) for c in cleaned]), r.fclean.v)


@BOTH
def test_a_bad_table_row_is_skipped(connectivity):
    per_map = [cm.finish(s[1], 200) for s in steps("mixed_batch", connectivity, None, 3)]
    for row, col, value in ((1, 0, 0), (1, 1, 1 << 15), (2, 2, None), (0, 2, -1), (1, 0, None)):
        r = Run(CASES["mixed_batch"], connectivity, None, 3, 200, 2)
        bad = r.table.clone()
        if value is None and col == 2:
            value = r.n - 10                      # the offset runs past the buffer
        if value is None:
            value = r.side + 1                    # beyond the caller's max_side
        bad[row, col] = value
        r.run(table=bad)
        keep = [k for k in range(4) if k != row]
        r.check(_cat([per_map[k] for k in keep]), images=keep)


def test_refusals_leave_the_frames_untouched():
    lib = L.load()
    r = Run(CASES["mixed_batch"], 8, None, 3, 200, 2)
    n, B = r.n, len(r.sizes)
    ws_bytes = lib.segclip_seg_sieve_ws_bytes(n, B, r.n_blocks)
    assert 21 * n <= ws_bytes <= 21 * n + 5 * 256
    ws = kf.Frame((ws_bytes,), torch.uint8)

    def call(conn=8, skip=-1, min_area=3, orphan=200, rounds=2, side=r.side, ws_n=ws_bytes, ws_p=ws.p, cleaned=r.fclean.p,
             cleaned_n=n, labels=r.fin.p, images=L.ptr(r.table)):
        rc = lib.segclip_seg_sieve(images, B, r.n_blocks, side, labels, n, conn, skip, min_area, orphan, rounds, cleaned, cleaned_n,
                                   ws_p, ws_n, L.stream())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return r.fclean.untouched() and ws.untouched() and torch.equal(r.in_bits, r.fin.bits())

    for kw in (dict(rounds=0), dict(rounds=9), dict(rounds=-1), dict(orphan=-2), dict(orphan=256), dict(conn=6), dict(conn=0),
               dict(skip=-2), dict(skip=256), dict(min_area=-1), dict(side=0), dict(side=1 << 15), dict(ws_n=ws_bytes - 1), dict(ws_n=0)):
        assert call(**kw) == ERR_UNSUPPORTED, kw
        assert lib.segclip_last_error_string().decode().startswith("seg_sieve"), kw
        assert untouched(), kw
    for kw in (dict(cleaned=r.fin.p), dict(cleaned=r.fin.v.data_ptr() + 8), dict(cleaned_n=n - 4), dict(cleaned=None),
               dict(labels=None), dict(images=None), dict(ws_p=None)):
        assert call(**kw) == ERR_INVALID, kw
        assert lib.segclip_last_error_string().decode().startswith("seg_sieve"), kw
        assert untouched(), kw
    assert lib.segclip_seg_sieve_ws_bytes(-1, 1, 1) == ERR_UNSUPPORTED and lib.segclip_seg_sieve_ws_bytes(n, 1, 1 << 31) == ERR_UNSUPPORTED
    # the wrapper
    with pytest.raises(L.Unsupported, match="rounds"):
        r.call(rounds=9)
    with pytest.raises(L.Unsupported, match="orphan_fill"):
        r.call(orphan_fill=256)
    with pytest.raises(L.Unsupported, match="connectivity"):
        r.call(connectivity=5)
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.seg_sieve(r.table, r.n_blocks, r.fin.v, min_area=3, cleaned=r.fin.v)
    with pytest.raises(ValueError, match="cleaned is a contiguous"):
        ops.seg_sieve(r.table, r.n_blocks, r.fin.v, min_area=3, cleaned=r.fclean.v.int())
    with pytest.raises(ValueError, match="table is the"):
        ops.seg_sieve(r.table[:, :7].contiguous(), r.n_blocks, r.fin.v, min_area=3, cleaned=r.fclean.v)
    assert untouched()
    # and the accepted call on the same frames, with a workspace of exactly ws_bytes
    assert call() == 0
    assert r.fclean.intact() and ws.intact() and torch.equal(r.in_bits, r.fin.bits())
    r.check(_cat([cm.finish(s[1], 200) for s in steps("mixed_batch", 8, None, 3)]))


@BOTH
def test_min_area_0_and_1_return_the_input(connectivity):
    labels = _cat(CASES["mixed_batch"])
    for min_area in (0, 1):
        for rounds, orphan_fill in ((1, None), (3, 9)):
            Run(CASES["mixed_batch"], connectivity, None, min_area, orphan_fill, rounds).run().check(labels)


@BOTH
def test_the_fill_mode_is_what_it_was(connectivity):
    """merge=False runs segclip_seg_components: the bytes of cc_reference.components, as before"""
    maps = [torch.from_numpy(m).to(DEV) for m in CASES["mixed_batch"]]
    want = _cat(cc.components(CASES["mixed_batch"], connectivity, 0, 4, 9)[3])
    for got in (despeckle(maps, 4, fill=9, connectivity=connectivity, skip_label=0),
                despeckle(maps, 4, 9, connectivity, 0, False, 1),
                despeckle(maps, 4, fill=9, connectivity=connectivity, skip_label=0, merge=False, rounds=1)):
        assert torch.equal(torch.cat([t.reshape(-1) for t in got]).cpu(), want)


@BOTH
def test_despeckle_merge(connectivity):
    """the Python layer: a list of maps, views of one buffer, keep and fill, rounds = single rounds composed"""
    maps = [torch.from_numpy(m).to(DEV) for m in CASES["mixed_batch"]]
    keep = [m.clone() for m in maps]
    for rounds, fill in ((1, None), (3, 9), (2, 0)):
        want = _cat([cm.finish(s[rounds - 1], fill) for s in steps("mixed_batch", connectivity, 0, 4)])
        got = despeckle(maps, 4, fill=fill, connectivity=connectivity, skip_label=0, merge=True, rounds=rounds)
        assert [tuple(t.shape) for t in got] == [tuple(m.shape) for m in maps] and all(t.dtype == torch.uint8 for t in got)
        assert torch.equal(torch.cat([t.reshape(-1) for t in got]).cpu(), want)
    assert all(torch.equal(a, b) for a, b in zip(maps, keep)), "the inputs changed"
    cur = maps
    for _ in range(3):
        cur = despeckle(cur, 4, fill=None, connectivity=connectivity, skip_label=0, merge=True)     # its own views, where they lie
    three = despeckle(maps, 4, fill=None, connectivity=connectivity, skip_label=0, merge=True, rounds=3)
    assert all(torch.equal(a, b) for a, b in zip(cur, three))
    with pytest.raises(ValueError, match="label map"):
        despeckle([maps[0].int()], 2, merge=True)


def test_merging_restores_the_scene_without_a_background_class():
    scene, speckled = cm.no_background_scene()
    maps = [torch.from_numpy(speckled).to(DEV)]
    merged = despeckle(maps, 16, merge=True)[0].cpu().numpy()
    filled = despeckle(maps, 16, fill=0)[0].cpu().numpy()
    assert np.array_equal(merged, scene)
    assert int((filled == 0).sum()) == 24 and 0 not in scene and int((filled != scene).sum()) == 24


# ------------------------------------------------------------------------------------------------ 4. end to end
TF = ImageTransform()
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(90, 120), (130, 101), (75, 75)]


def _raws(seed):
    g = torch.Generator().manual_seed(seed)
    raws = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in RAW_SIZES]
    gts = [torch.randint(0, 14, (h, w), generator=g).to(torch.uint8).to(DEV) for (h, w) in RAW_SIZES]
    for t in gts:
        t[5:9] = 255
    return raws, gts


def _areas(maps, gts, C):
    areas = torch.zeros(3, C, dtype=torch.int64, device=DEV)
    for m, t in zip(maps, gts):
        ops.seg_areas(m, t, C, reduce_zero_label=True, areas=areas)
    return areas


def _eq(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_end_to_end():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        tokens = torch.from_numpy(g["prompt_ids"])
        raws, gts = _raws(11)
        seg = SegInference(model, emb, True, bg_thresh=0.02, **SLIDE)
        C = seg.num_classes
        plain = seg.predict_raw(raws, TF)
        keep = [p.clone() for p in plain]
        sizes = sorted(set(components(plain).records[:, 3].tolist()))
        m = max(2, sizes[len(sizes) // 2])
        d = Despeckle(m, merge=True, rounds=2)
        want = despeckle(plain, m, merge=True, rounds=2)
        assert _eq(plain, keep), "despeckle changed its input"
        assert not _eq(want, plain), "the case has nothing to merge"
        # the restatement on this build's own label maps
        ref = [cm.merge(p.cpu().numpy(), 8, None, m, 0, 2) for p in plain]
        assert _eq([w.cpu() for w in want], [torch.from_numpy(r) for r in ref])
        got = seg.predict_raw(raws, TF, clean=d)
        assert [tuple(t.shape) for t in got] == RAW_SIZES and all(t.dtype == torch.uint8 for t in got)
        assert _eq(got, want), "predict_raw(clean=) differs from despeckle(predict_raw())"
        # the evaluator: the areas of the merged maps
        ev = SegEvaluator(seg, reduce_zero_label=True)
        maps = ev.update_raw(raws, gts, TF, return_labels=True, clean=d)
        assert _eq(maps, want)
        areas = _areas(want, gts, C)
        assert torch.equal(ev.areas, areas) and int(areas.sum()) > 0 and not torch.equal(areas, _areas(plain, gts, C))
        # refine=, clean= and boundary= together: the functions in that order
        pamr = PAMR(iters=2, dilations=(1, 2))
        both = despeckle(refine_labels(raws, plain, C, TF, pamr), m, merge=True, rounds=2)
        assert _eq(seg.predict_raw(raws, TF, refine=pamr, clean=d), both)
        ev = SegEvaluator(seg, reduce_zero_label=True, boundary=Boundary())
        assert _eq(ev.update_raw(raws, gts, TF, return_labels=True, refine=pamr, clean=d), both)
        assert torch.equal(ev.areas, _areas(both, gts, C))
        assert "bIoU" in ev.compute()
        # eval_epoch
        batches = [([t.cpu() for t in raws[:2]], [t.cpu() for t in gts[:2]]), ([t.cpu() for t in raws[2:]], [t.cpu() for t in gts[2:]])]
        cfg = dict(bg_thresh=0.02, reduce_zero_label=True, **SLIDE)
        score = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(clean=d, **cfg), transform=TF)
        ev = SegEvaluator(seg, reduce_zero_label=True)
        areas = torch.zeros_like(ev.areas)
        for rs, ts in batches:
            rs, ts = [t.to(DEV) for t in rs], [t.to(DEV) for t in ts]
            ev.update_raw(rs, ts, TF, clean=d)
            areas += _areas(despeckle(seg.predict_raw(rs, TF), m, merge=True, rounds=2), ts, C)
        assert torch.equal(ev.areas, areas)
        assert score == ev.compute()["mIoU"] * 100.0 and 0.0 <= score <= 100.0
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
