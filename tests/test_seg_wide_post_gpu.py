"""GPU: components, despeckling (fill and merge) and the boundary metrics of 16-bit label maps - segclip_seg_components_wide,
segclip_seg_sieve_wide, segclip_seg_boundary_wide (the templates of csrc/segment_objects.inc, segment_sieve.inc and
segment_boundary.inc on uint16_t), ops.seg_components / seg_sieve / seg_boundary on int16 tensors, components, despeckle,
boundary_bands, boundary_areas and SegEvaluator.update_maps - against tests/wide_post_reference.py.  Everything is an integer:
every comparison is torch.equal.  The maps are small (the Python union-find is the slow side) and cross the 16 x 64 component
tile and the 32 x 64 boundary strip in both directions; their values are those a byte kernel gets wrong: {1, 257, 513} share a low
byte, {255, 32768, 65535} have the top bit and the 16-bit pattern of -1.  Outputs lie in frames (tests/kernel_frames.py), the
maps lie in one flat buffer with gaps between them."""
import functools

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import (PAMR, Boundary, Despeckle, ImageTransform, SegEvaluator, SegInference, SegSweepEvaluator,
                                      boundary_areas, boundary_bands, components, despeckle)
from tests import boundary_reference as bd
from tests import cc_reference as cc
from tests import kernel_frames as kf
from tests import wide_post_reference as wp
from tests.helpers import tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 5          # unused elements between two maps of a flat buffer: offsets that are no multiples of 4
FRAME_FILL = 0x2BAB   # of the int16 frames: no label of any test map


def t16(m):
    """(h, w) uint16 array -> int16 device tensor with the same bits"""
    return torch.from_numpy(np.ascontiguousarray(m).view(np.int16)).to(DEV)


def n16(t):
    """int16 tensor -> uint16 array"""
    return t.cpu().contiguous().numpy().view(np.uint16)


def cat(xs):
    """arrays -> one flat CPU tensor; uint16 arrays as int16 with the same bits"""
    flat = np.concatenate([np.ascontiguousarray(x).reshape(-1) for x in xs])
    return torch.from_numpy(flat.view(np.int16) if flat.dtype == np.uint16 else flat)


class Flat:
    """maps laid into one framed flat buffer, GAP unused elements between them (filled with 0x2BAB, which the kernels never read)"""

    def __init__(self, maps, dtype=torch.int16):
        self.sizes = [tuple(m.shape) for m in maps]
        self.offs, n = [], 0
        for (h, w) in self.sizes:
            self.offs.append(n)
            n += h * w + GAP
        self.n = n - GAP
        self.dtype = dtype
        self.used = torch.zeros(self.n, dtype=torch.bool)
        self.frame = kf.Frame((self.n,), dtype, fill=FRAME_FILL if dtype == torch.int16 else None)
        for m, o in zip(maps, self.offs):
            m = np.ascontiguousarray(m)
            self.frame.v[o:o + m.size] = torch.from_numpy(m.view(np.int16) if dtype == torch.int16 else m).reshape(-1).to(DEV)
            self.used[o:o + m.size] = True
        self.bits = self.frame.bits()

    @property
    def v(self):
        return self.frame.v

    def out(self, dtype):
        return kf.Frame((self.n,), dtype, fill=FRAME_FILL if dtype == torch.int16 else None)

    def unchanged(self):
        return torch.equal(self.bits, self.frame.bits())

    def inside(self, frame):
        """the maps' own elements of an output frame laid out like this buffer; nothing else of it may be written"""
        got = frame.v.cpu()
        assert frame.intact() and bool((got[~self.used] == frame.fill).all()), "wrote outside the maps"
        return got[self.used]


# ------------------------------------------------------------------------------------------------ 1. components
CC_CASES = {"shared_low_byte": (wp.SHARED_LOW_BYTE, None), "top_bit": (wp.TOP_BIT_AND_SENTINEL, None),
            "top_bit_skip_65535": (wp.TOP_BIT_AND_SENTINEL, 65535), "top_bit_skip_255": (wp.TOP_BIT_AND_SENTINEL, 255)}
CC_MIN_AREA, CC_FILL = 3, 40000


@functools.lru_cache(maxsize=None)
def cc_maps(name):
    return wp.batch(CC_CASES[name][0], seed=sum(map(ord, name)))


@functools.lru_cache(maxsize=None)
def cc_reference(name, connectivity):
    ids, area, records, cleaned = wp.components(cc_maps(name), connectivity, CC_CASES[name][1], CC_MIN_AREA, CC_FILL)
    return cat(ids), cat(area), torch.from_numpy(records), cat(cleaned)


def run_components(flat, connectivity, skip, K, min_area=CC_MIN_AREA, fill=CC_FILL):
    out = dict(ids=flat.out(torch.int32), area=flat.out(torch.int32), cleaned=flat.out(flat.dtype),
               records=kf.Frame((K, ops.SEG_CC_RECORD), torch.int64), count=kf.Frame((1,), torch.int64))
    table, n_blocks, side = ops.seg_components_table(flat.sizes, flat.offs, DEV)
    ops.seg_components(table, n_blocks, flat.v, connectivity=connectivity, skip_label=skip, ids=out["ids"].v, area_px=out["area"].v,
                       records=out["records"].v, count=out["count"].v, min_area=min_area, fill=fill, cleaned=out["cleaned"].v,
                       max_side=side)
    torch.cuda.synchronize()
    assert flat.unchanged(), "the input labels changed"
    assert out["records"].intact() and out["count"].intact()
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(CC_CASES))
def test_components_against_the_restatement(name, connectivity):
    ids, area, records, cleaned = cc_reference(name, connectivity)
    n = records.shape[0]
    flat = Flat(cc_maps(name))
    out = run_components(flat, connectivity, CC_CASES[name][1], n + 3)
    assert torch.equal(flat.inside(out["ids"]), ids), "ids"
    assert torch.equal(flat.inside(out["area"]), area), "area_px"
    assert int(out["count"].v.cpu()[0]) == n
    got = out["records"].v.cpu()
    assert torch.equal(got[:n], records), "records (column 2 carries the 16-bit label)"
    assert bool((got[n:] == out["records"].fill).all()), "rows beyond the count were written"
    assert torch.equal(flat.inside(out["cleaned"]), cleaned), "cleaned"
    labels = set(records[:, 2].tolist())
    skip = CC_CASES[name][1]
    assert labels == set(CC_CASES[name][0]) - {skip}, "every value is a label of its own, 65535 too unless it is skipped"
    # the list overflows: the right count and exactly K rows
    K = n - 2
    short = run_components(flat, connectivity, skip, K)
    assert int(short["count"].v.cpu()[0]) == n and torch.equal(short["records"].v.cpu(), records[:K])


def test_components_public_function_and_low_values():
    """components() on int16 maps = the restatement; an int16 copy of a uint8 map gives what the uint8 map gives, everywhere"""
    maps = cc_maps("top_bit")
    obj = components([t16(m) for m in maps], connectivity=8)
    ids, _, records, _ = cc_reference("top_bit", 8)
    assert obj.count == records.shape[0] and torch.equal(obj.records.cpu(), records)
    assert torch.equal(torch.cat([i.reshape(-1) for i in obj.ids]).cpu(), ids)
    rng = np.random.default_rng(5)
    low = [cc._blocks(rng, h, w, 2, tuple(range(21))) for (h, w) in wp.SIZES]
    f8, f16 = Flat(low, torch.uint8), Flat([m.astype(np.uint16) for m in low])
    for connectivity in (4, 8):
        a, b = run_components(f8, connectivity, 0, 4096, 4, 7), run_components(f16, connectivity, 0, 4096, 4, 7)
        for key in ("ids", "area", "records", "count"):
            assert torch.equal(a[key].v, b[key].v), key
        assert torch.equal(f8.inside(a["cleaned"]).to(torch.int16), f16.inside(b["cleaned"]))


# ------------------------------------------------------------------------------------------------ 2. merge
def sieve(maps, **kw):
    """ops.seg_sieve on a flat framed buffer -> the cleaned maps as uint16 arrays (frames and gaps checked)"""
    flat = Flat(maps)
    table, n_blocks, side = ops.seg_components_table(flat.sizes, flat.offs, DEV)
    out = flat.out(torch.int16)
    ops.seg_sieve(table, n_blocks, flat.v, cleaned=out.v, max_side=side, **kw)
    torch.cuda.synchronize()
    assert flat.unchanged()
    got = flat.inside(out)
    again = flat.out(torch.int16)
    ops.seg_sieve(table, n_blocks, flat.v, cleaned=again.v, max_side=side, **kw)
    assert torch.equal(out.bits(), again.bits()), "two calls give the same bits"
    cuts = np.cumsum([h * w for h, w in flat.sizes])[:-1]
    return [p.reshape(s) for p, s in zip(np.split(n16(got), cuts), flat.sizes)]


def test_merge_scenes():
    """a 2 x 2 speck between two kept regions of equal area takes the SMALLER 16-bit label; a byte key would take 513 over 300"""
    scenes = [wp.speck_between(256, 1), wp.speck_between(1, 256), wp.speck_between(300, 513), wp.speck_between(513, 300),
              wp.speck_between(65535, 32768), wp.speck_between(9, 40000, wider_right=3)]
    winners = [1, 1, 300, 300, 32768, 40000]
    got = despeckle([t16(s) for s in scenes], 5, merge=True, connectivity=4, fill=None)
    assert all(g.dtype == torch.int16 for g in got)
    for g, s, win in zip(got, scenes, winners):
        assert np.array_equal(n16(g), wp.merge(s, 4, None, 5)) and bool((n16(g)[1:3, 6:8] == win).all()), win
    nested = wp.nested()
    one, two = (n16(despeckle([t16(nested)], 9, merge=True, rounds=r, fill=None)[0]) for r in (1, 2))
    assert np.array_equal(one, wp.merge(nested, 8, None, 9, None, 1)) and one[5, 6] == 40000 and (one != 300).sum() == 1
    assert (two == 300).all(), "the nested speck needs rounds=2"
    # orphans: walled in by the skipped 65535 (through ops: Despeckle keeps its byte range); fill=None keeps them
    walled = wp.walled_in()
    kept = sieve([walled], connectivity=8, skip_label=65535, min_area=4)[0]
    filled = sieve([walled], connectivity=8, skip_label=65535, min_area=4, orphan_fill=65535)[0]
    assert np.array_equal(kept, walled) and filled[3, 4] == 65535 and np.array_equal(filled, wp.merge(walled, 8, 65535, 4, 65535))
    unskipped = n16(despeckle([t16(walled)], 4, merge=True, fill=None)[0])   # 65535 is a label like any other: the wall wins
    assert unskipped[3, 4] == 65535 and np.array_equal(unskipped, wp.merge(walled, 8, None, 4))


@pytest.mark.parametrize("name", ["shared_low_byte", "top_bit", "top_bit_skip_65535"])
def test_merge_against_the_restatement_and_the_injection(name):
    maps, skip = cc_maps(name), CC_CASES[name][1]
    for connectivity, rounds, orphan in ((4, 2, None), (8, 1, 65535)):
        kw = dict(connectivity=connectivity, skip_label=skip, min_area=6, rounds=rounds)
        got = sieve(maps, orphan_fill=orphan, **kw)
        want = [wp.merge(m, connectivity, skip, 6, orphan, rounds) for m in maps]
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert sum(int((w != m).sum()) for w, m in zip(want, maps)) > 50, "the maps do not exercise the merge"
        # the same call on the rank-relabelled uint8 copy, mapped back
        ranked, table = wp.rank_relabel(maps)
        f8 = Flat(ranked, torch.uint8)
        tab8, n_blocks, side = ops.seg_components_table(f8.sizes, f8.offs, DEV)
        skip8 = None if skip is None else int(np.searchsorted(table, skip))
        back = f8.inside(_sieve8(tab8, n_blocks, side, f8, dict(kw, skip_label=skip8))).numpy()
        if orphan is None:
            assert np.array_equal(table[back], np.concatenate([g.reshape(-1) for g in got]))
        else:   # the orphans' fill is no rank: compare where the uint8 call did not fill
            flat16 = np.concatenate([g.reshape(-1) for g in got])
            plain = np.concatenate([wp.merge(m, connectivity, skip, 6, None, rounds).reshape(-1) for m in maps])
            assert np.array_equal(table[back], plain) and np.array_equal(flat16[flat16 != 65535], plain[flat16 != 65535])


def _sieve8(table, n_blocks, side, f8, kw):
    out = f8.out(torch.uint8)
    ops.seg_sieve(table, n_blocks, f8.v, cleaned=out.v, max_side=side, **kw)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ 3. boundary
BD_VALUES = (0, 1, 256, 257, 1023, 1024, 2000, 65535)


@pytest.mark.parametrize("name", ["shared_low_byte", "top_bit"])
def test_bands(name):
    maps = cc_maps(name)
    ranked, _ = wp.rank_relabel(maps)
    for d in (1, 3):
        got = boundary_bands([t16(m) for m in maps], Boundary(radius=d))
        got8 = boundary_bands([torch.from_numpy(r).to(DEV) for r in ranked], Boundary(radius=d))
        assert all(g.dtype == torch.uint8 for g in got)
        assert all(np.array_equal(g.cpu().numpy(), wp.band(m, d)) for g, m in zip(got, maps)), d
        assert all(torch.equal(g, g8) for g, g8 in zip(got, got8)), d
    # through ops on a buffer with gaps, both bands written
    flat = Flat(maps)
    radii = [2] * len(maps)
    table, n_blocks, side = ops.seg_boundary_table(flat.sizes, flat.offs, None, radii, DEV)
    pb = flat.out(torch.uint8)
    ops.seg_boundary(table, n_blocks, flat.v, pred_band=pb.v, max_side=side)
    torch.cuda.synchronize()
    assert torch.equal(flat.inside(pb), cat([wp.band(m, 2) for m in maps])) and flat.unchanged()


@functools.lru_cache(maxsize=None)
def bd_pairs():
    rng = np.random.default_rng(20261021)
    preds = [wp.blocks(rng, h, w, 4, BD_VALUES[:-1]) for (h, w) in wp.SIZES]
    gts = [wp.blocks(rng, h, w, 5, BD_VALUES) for (h, w) in wp.SIZES]
    for p, g in zip(preds, gts):    # agreement on about half of the pixels
        keep = wp.blocks(rng, *p.shape, 3, (0, 1)).astype(bool)
        p[keep & (g != 65535)] = g[keep & (g != 65535)]
    return preds, gts


@pytest.mark.parametrize("reduce_zero", [False, True])
@pytest.mark.parametrize("C", [257, 1024])
def test_boundary_areas(C, reduce_zero):
    """classes 256 and 1023 are present, the ground truth holds 65535 (ignored) and values >= C; gaps in both buffers"""
    preds, gts = bd_pairs()
    radii = [bd.radius(h, w, 0.05) for (h, w) in wp.SIZES]
    want = torch.from_numpy(wp.areas(preds, gts, radii, C, 65535, reduce_zero))
    assert int(want[0, 1, 256]) > 0 and int(want[1, 2, 256 - reduce_zero]) > 0 and (C == 257 or int(want[0, 2, 1023 - reduce_zero]) > 0)
    pf, gf = Flat(preds), Flat(gts)
    table, n_blocks, side = ops.seg_boundary_table(pf.sizes, pf.offs, gf.offs, radii, DEV)
    areas = kf.Frame((2, 3, C), torch.int64)
    areas.v.zero_()
    pb, gb = pf.out(torch.uint8), gf.out(torch.uint8)
    ops.seg_boundary(table, n_blocks, pf.v, gt=gf.v, num_classes=C, ignore_index=65535, reduce_zero_label=reduce_zero,
                     pred_band=pb.v, gt_band=gb.v, areas=areas.v, max_side=side)
    torch.cuda.synchronize()
    assert areas.intact() and pf.unchanged() and gf.unchanged()
    assert torch.equal(areas.v.cpu(), want)
    assert torch.equal(pf.inside(pb), cat([wp.band(m, d) for m, d in zip(preds, radii)]))
    assert torch.equal(gf.inside(gb), cat([wp.band(m, d) for m, d in zip(gts, radii)]))
    # the public function adds to what it is given
    got = boundary_areas([t16(p) for p in preds], [t16(g) for g in gts], C, Boundary(ratio=0.05), ignore_index=65535,
                         reduce_zero_label=reduce_zero, areas=areas.v.clone())
    assert torch.equal(got.cpu(), 2 * want)


def test_boundary_identities():
    preds, gts = bd_pairs()
    keep = [i for i, (h, w) in enumerate(wp.SIZES) if max(h, w) <= ops.SEG_BOUNDARY_MAX_RADIUS]
    p16, g16 = [t16(preds[i]) for i in keep], [t16(gts[i]) for i in keep]
    C = 1024
    # a radius >= max(h, w): every band byte is set and slot 0 is segclip_seg_areas_wide's
    big = boundary_areas(p16, g16, C, Boundary(radius=ops.SEG_BOUNDARY_MAX_RADIUS), ignore_index=65535)
    plain = ops.seg_areas_wide(torch.cat([p.reshape(-1) for p in p16]), torch.cat([g.reshape(-1) for g in g16]), C, 65535)
    assert torch.equal(big[0], plain) and int(plain[1, 1023]) > 0
    # a ground truth of one value has no change: slot 1 stays as it was
    uniform = [torch.full_like(g, 256) for g in g16]
    seeded = torch.arange(2 * 3 * C, dtype=torch.int64, device=DEV).view(2, 3, C)
    got = boundary_areas(p16, uniform, C, Boundary(radius=3), ignore_index=65535, areas=seeded.clone())
    assert torch.equal(got[1], seeded[1]) and not torch.equal(got[0], seeded[0])
    # low values: the (2, 3, 21) of the 16-bit entry = the uint8 entry's
    rng = np.random.default_rng(9)
    lp, lg = zip(*(bd.area_pair(rng, h, w, tuple(range(21)), ignore=20) for (h, w) in wp.SIZES[3:]))
    for rz in (False, True):
        kw = dict(ignore_index=20, reduce_zero_label=rz)
        a8 = boundary_areas([torch.from_numpy(p).to(DEV) for p in lp], [torch.from_numpy(g).to(DEV) for g in lg], 21, Boundary(radius=2), **kw)
        a16 = boundary_areas([t16(p.astype(np.uint16)) for p in lp], [t16(g.astype(np.uint16)) for g in lg], 21, Boundary(radius=2), **kw)
        assert torch.equal(a8, a16) and int(a8.sum()) > 0


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing():
    maps = cc_maps("top_bit")[3:5]
    flat = Flat(maps)
    table, n_blocks, side = ops.seg_components_table(flat.sizes, flat.offs, DEV)
    outs = [flat.out(torch.int32), flat.out(torch.int16), kf.Frame((1,), torch.int64)]
    cc_kw = dict(ids=outs[0].v, cleaned=outs[1].v, count=outs[2].v, max_side=side)
    with pytest.raises(L.Unsupported, match="skip_label"):
        ops.seg_components(table, n_blocks, flat.v, skip_label=65536, **cc_kw)
    with pytest.raises(L.Unsupported, match="fill"):
        ops.seg_components(table, n_blocks, flat.v, fill=65536, min_area=3, **cc_kw)
    with pytest.raises(L.Unsupported, match="orphan_fill"):
        ops.seg_sieve(table, n_blocks, flat.v, orphan_fill=65536, min_area=3, cleaned=outs[1].v, max_side=side)
    with pytest.raises(L.Unsupported, match="skip_label"):
        ops.seg_sieve(table, n_blocks, flat.v, skip_label=65536, min_area=3, cleaned=outs[1].v, max_side=side)
    wrong = flat.out(torch.uint8)
    with pytest.raises(ValueError, match="cleaned is a contiguous"):   # the other dtype
        ops.seg_components(table, n_blocks, flat.v, cleaned=wrong.v, max_side=side)
    with pytest.raises(ValueError, match="cleaned is a contiguous"):
        ops.seg_sieve(table, n_blocks, flat.v, cleaned=wrong.v, max_side=side)
    with pytest.raises(ValueError, match="cleaned is a contiguous"):
        ops.seg_sieve(table, n_blocks, wrong.v, cleaned=outs[1].v, max_side=side)
    for fn in (ops.seg_components, ops.seg_sieve):
        with pytest.raises(ValueError, match="labels is a contiguous uint8"):
            fn(table, n_blocks, flat.v.to(torch.int32), max_side=side)
    # boundary: the class limit, ignore_index, mixed dtypes
    btable, bblocks, bside = ops.seg_boundary_table(flat.sizes, flat.offs, flat.offs, [2, 2], DEV)
    areas = kf.Frame((2, 3, 1025), torch.int64)
    band = flat.out(torch.uint8)
    with pytest.raises(L.Unsupported, match="1025 classes"):
        ops.seg_boundary(btable, bblocks, flat.v, gt=flat.v, num_classes=1025, ignore_index=65535, areas=areas.v, pred_band=band.v,
                         max_side=bside)
    a257 = kf.Frame((2, 3, 257), torch.int64)
    with pytest.raises(L.Unsupported, match="ignore_index"):
        ops.seg_boundary(btable, bblocks, flat.v, gt=flat.v, num_classes=257, ignore_index=65536, areas=a257.v, max_side=bside)
    u8 = Flat([m.astype(np.uint8) for m in maps], torch.uint8)
    with pytest.raises(L.Unsupported, match="257 classes"):   # the uint8 entry keeps its limit
        ops.seg_boundary(btable, bblocks, u8.v, gt=u8.v, num_classes=257, areas=a257.v, max_side=bside)
    with pytest.raises(ValueError, match="both uint8 or both int16"):
        ops.seg_boundary(btable, bblocks, u8.v, gt=flat.v, num_classes=21, pred_band=band.v, max_side=bside)
    with pytest.raises(ValueError, match="pred is a contiguous uint8"):
        ops.seg_boundary(btable, bblocks, flat.v.to(torch.int32), pred_band=band.v, max_side=bside)
    torch.cuda.synchronize()
    assert all(f.untouched() for f in outs + [wrong, areas, a257, band]) and flat.unchanged() and u8.unchanged()
    # the public functions: a mixed list, another dtype, mixed predictions and ground truths
    m16, m8, m32 = t16(maps[0]), torch.from_numpy(maps[0].astype(np.uint8)).to(DEV), t16(maps[0]).to(torch.int32)
    for call in (lambda m: components(m), lambda m: despeckle(m, 4), lambda m: boundary_bands(m, Boundary()),
                 lambda m: boundary_areas(m, m, 21, Boundary())):
        with pytest.raises(ValueError, match="label maps are all uint8 or all int16"):
            call([m16, m8])
        with pytest.raises(ValueError, match="label map"):
            call([m32])
    with pytest.raises(ValueError, match="ground truth"):
        boundary_areas([m16], [m8], 21, Boundary())
    with pytest.raises(ValueError, match="ground truth"):
        boundary_areas([m8], [m16], 21, Boundary())
    with pytest.raises(L.Unsupported, match="1025 classes"):
        boundary_areas([m16], [m16], 1025, Boundary(), ignore_index=65535)


# ------------------------------------------------------------------------------------------------ 5. SegEvaluator.update_maps
SLIDE = dict(mode="slide", crop_size=(64, 64), stride=(48, 48))


def _embedding(n, seed=3, width=64):
    e = torch.randn(n, width, generator=torch.Generator().manual_seed(seed))
    return (e / e.norm(dim=-1, keepdim=True)).to(DEV)


def _raws(gen):
    return [torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).to(DEV) for (h, w) in [(70, 90), (64, 100)]]


def _ground_truths(labels, ignore, gen):
    """the labels moved by a few pixels, with an ignored block: agreement, disagreement and ignored pixels"""
    gts = []
    for lab in labels:
        g = torch.roll(lab, shifts=(3, 5), dims=(0, 1)).clone()
        g[10:20, 15:40] = ignore
        gts.append(g.contiguous())
    return gts


def test_update_maps_uint8_evaluator():
    try:
        model = tiny_seg_model()
        seg = SegInference(model, _embedding(20), True, bg_thresh=0.0, **SLIDE)
        tf = ImageTransform(img_scale=(256, 96))
        raws = _raws(torch.Generator().manual_seed(8))
        labels = seg.predict_raw(raws, tf)
        gts = _ground_truths(labels, 255, None)
        ev = SegEvaluator(seg, boundary=Boundary(), confusion=True)
        maps = ev.update_raw(raws, gts, tf, return_labels=True)
        fresh = SegEvaluator(seg, boundary=Boundary(), confusion=True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")     # no host synchronisation
        try:
            assert fresh.update_maps(maps, gts) is None
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert int(ev.areas.sum()) > 0 and int(ev.boundary_areas.sum()) > 0
        assert torch.equal(fresh.areas, ev.areas) and torch.equal(fresh.confusion, ev.confusion)
        assert torch.equal(fresh.boundary_areas, ev.boundary_areas)
        with pytest.raises(ValueError, match="label map 0 is a non-empty .* uint8"):
            fresh.update_maps([m.to(torch.int16) for m in maps], gts)
        with pytest.raises(ValueError, match="label map 1 has its ground truth's size"):
            fresh.update_maps([maps[0], maps[1][:-1]], gts)
        with pytest.raises(ValueError, match="2 label maps but 1 ground truths"):
            fresh.update_maps(maps, gts[:1])
        assert torch.equal(fresh.areas, ev.areas)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_update_maps_16_bit_evaluator_and_the_composed_chain():
    try:
        model = tiny_seg_model()
        seg = SegInference(model, _embedding(300), True, bg_thresh=0.0, label_dtype=torch.int16, **SLIDE)
        C = seg.num_classes
        tf = ImageTransform(img_scale=(256, 96))
        raws = _raws(torch.Generator().manual_seed(9))
        labels = seg.predict_raw(raws, tf)
        assert labels[0].dtype == torch.int16 and max(int(n16(m).max()) for m in labels) > 255
        gts = _ground_truths(labels, -1, None)     # 65535
        ev = SegEvaluator(seg, ignore_index=65535, confusion=True)
        maps = ev.update_raw(raws, gts, tf, return_labels=True)
        fresh = SegEvaluator(seg, ignore_index=65535, confusion=True)
        fresh.update_maps(maps, gts)
        assert int(ev.areas[0].sum()) > 0 and torch.equal(fresh.areas, ev.areas) and torch.equal(fresh.confusion, ev.confusion)
        # the chain of a wide vocabulary: predict, despeckle by merging, score the cleaned maps
        cleaned = despeckle(seg.predict_raw(raws, tf), 4, merge=True)
        assert all(np.array_equal(n16(c), wp.merge(n16(m), 8, None, 4, 0, 1)) for c, m in zip(cleaned, labels))
        chain = SegEvaluator(seg, ignore_index=65535)
        chain.update_maps(cleaned, gts)
        want = ops.seg_areas_wide(torch.cat([c.reshape(-1) for c in cleaned]), torch.cat([g.reshape(-1) for g in gts]), C, 65535)
        assert torch.equal(chain.areas, want)
        objs = components(cleaned)
        assert objs.count == wp.components([n16(c) for c in cleaned])[2].shape[0]
        bareas = boundary_areas(cleaned, gts, C, Boundary(), ignore_index=65535)
        radii = [Boundary().radius_of(*c.shape) for c in cleaned]
        assert torch.equal(bareas.cpu(), torch.from_numpy(wp.areas([n16(c) for c in cleaned], [n16(g) for g in gts], radii, C, 65535)))
        with pytest.raises(ValueError, match="label map 0 is a non-empty .* int16"):
            chain.update_maps([c.to(torch.uint8) for c in cleaned], gts)
        # the in-pipeline stages of a 16-bit SegInference stay refused, by name and before the towers
        calls = []
        model.clip.encode_image = lambda *a, **k: calls.append(1)
        try:
            for stage, call in [("clean", lambda: seg.predict_raw(raws, tf, clean=Despeckle(4))),
                                ("clean", lambda: ev.update_raw(raws, gts, tf, clean=Despeckle(4))),
                                ("refine", lambda: seg.predict_raw(raws, tf, refine=PAMR())),
                                ("boundary", lambda: SegEvaluator(seg, boundary=Boundary())),
                                ("SegSweepEvaluator", lambda: SegSweepEvaluator(seg, [0.1, 0.2]))]:
                with pytest.raises(ValueError, match=stage):
                    call()
            assert not calls
        finally:
            del model.clip.encode_image
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
