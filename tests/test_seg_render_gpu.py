"""GPU: the rendering of segmentation results - segclip_seg_blend and segclip_seg_groups_rescaled (csrc/segment_render.inc),
segmentation.blend / anchors_from_sums and SegInference.groups_list / groups_raw / render_raw - against
tests/seg_render_reference.py.

The overlay and the anchor sums are integers and must equal numpy's exactly.  The group map is an arg-max of fp32 values
against an fp64 yardstick: a pixel may differ only where the yardstick's top-two gap is below 1e-6 (TIE of
tests/test_seg_eval_gpu.py; the values are at most 1 and go through two fp32 blends of a few 2^-24 each), and such pixels
may be at most 0.05 % of a case (its CAP, a fixed condition).  GROUP_TIE_COUNTS holds the yardstick's own counts
(CPU: `python -m tests.test_seg_render_gpu`).
"""
import functools

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import (ImageTransform, SegInference, anchors_from_sums, blend, default_group_palette)
from tests import seg_render_reference as rr
from tests.helpers import CountedEncodeImage, load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8 = 0xA5
TIE, CAP = 1e-6, 5e-4
TF = ImageTransform()


# ------------------------------------------------------------------------------------------------ the blend kernel, framed
def _blend_framed(raws, maps, palette, opacity, skip_zero=False, reverse=False, sums=None, pad=8, map_pad=5):
    """The kernel on index maps and an output that lie inside guard bytes -> ([(h, w, 3)] on the CPU); the guards (and the gaps
    between the images) must stay as they were."""
    offs, n = [], map_pad
    for m in maps:
        offs.append(n)
        n += m.numel() + map_pad           # odd gaps: most maps start off a dword boundary
    flat = torch.full((n,), SENT8, dtype=torch.uint8, device=DEV)
    for m, o in zip(maps, offs):
        flat[o:o + m.numel()] = m.reshape(-1).to(DEV)
    before = flat.clone()
    table, out_offs, nbytes, n_blocks = ops.seg_blend_table(raws, offs)
    buf = torch.full((nbytes + 2 * pad,), SENT8, dtype=torch.uint8, device=DEV)
    out = buf[pad:pad + nbytes]
    ops.seg_blend(table, n_blocks, flat, palette.to(DEV), opacity, out, skip_zero=skip_zero, reverse_channels=reverse, sums=sums)
    torch.cuda.synchronize()
    assert torch.equal(flat, before), "the kernel wrote into the index maps"
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    got = []
    for o, t in zip(out_offs, raws):
        k = 3 * t.shape[0] * t.shape[1]
        keep[pad + o:pad + o + k] = False
        got.append(out[o:o + k].view(t.shape[0], t.shape[1], 3).cpu())
    assert bool((buf.cpu()[keep] == SENT8).all()), "the kernel wrote outside its output"
    return got


# ------------------------------------------------------------------------------------------------ 1. arithmetic, exhaustive
@pytest.mark.parametrize("skip_zero", [False, True])
@pytest.mark.parametrize("opacity", [0.3, 0.5, 0.6, 0.8, 1.0])
def test_blend_arithmetic_exhaustive(opacity, skip_zero):
    """Every (pixel byte, colour byte) pair: pixel = row, colour = column.  An fp32 or a fused fp64 kernel fails here."""
    rows = torch.arange(256, dtype=torch.uint8)
    img = rows[:, None, None].expand(256, 256, 3).contiguous()
    idx = rows[None, :].expand(256, 256).contiguous()
    pal = rows[:, None].expand(256, 3).contiguous()
    got = blend([img.to(DEV)], [idx.to(DEV)], pal, opacity, skip_zero=skip_zero)[0].cpu().numpy()
    want = rr.blend(img.numpy(), idx.numpy(), pal.numpy(), opacity, skip_zero=skip_zero)
    wrong = int((got != want).sum())
    print(f"opacity {opacity} skip_zero {skip_zero}: {wrong} of {want.size} bytes differ")
    assert wrong == 0


# ------------------------------------------------------------------------------------------------ 2. shapes
SHAPES = [(1, 1), (3, 5), (7, 13), (33, 67)]
P21 = 21


@functools.lru_cache(maxsize=None)
def _shape_case(i):
    h, w = SHAPES[i]
    g = torch.Generator().manual_seed(300 + i)
    img = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    idx = torch.randint(0, P21 + 6, (h, w), generator=g, dtype=torch.uint8)   # indices 21 .. 26 are outside the palette
    if h * w > 4:
        idx.view(-1)[::5] = 0
        idx.view(-1)[3] = 255
    return img, idx


@functools.lru_cache(maxsize=None)
def _palette21():
    return torch.randint(0, 256, (P21, 3), generator=torch.Generator().manual_seed(77), dtype=torch.uint8)


def _device_raw(i):
    """The picture on the device; the 33 x 67 one as a view of a larger tensor, with a row stride that is no multiple of 4."""
    img = _shape_case(i)[0]
    if SHAPES[i] != (33, 67):
        return img.to(DEV)
    h, w = SHAPES[i]
    big = torch.full((h + 2, w + 6, 3), 77, dtype=torch.uint8, device=DEV)
    big[1:h + 1, 2:w + 2] = img.to(DEV)
    view = big[1:h + 1, 2:w + 2]
    assert view.stride() == (3 * (w + 6), 3, 1) and view.stride(0) % 4 != 0
    return view


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("skip_zero", [False, True])
def test_blend_shapes(skip_zero, reverse):
    pal = _palette21()
    singles = []
    for i in range(len(SHAPES)):
        img, idx = _shape_case(i)
        assert SHAPES[i] == (1, 1) or bool((idx >= P21).any())
        got = _blend_framed([_device_raw(i)], [idx], pal, 0.6, skip_zero, reverse, pad=8 + i)[0]
        want = rr.blend(img.numpy(), idx.numpy(), pal.numpy(), 0.6, skip_zero, reverse)
        assert np.array_equal(got.numpy(), want), f"{SHAPES[i]}: {int((got.numpy() != want).sum())} bytes differ"
        singles.append(got)
    # one list of all of them, in another order, in one launch
    order = [2, 0, 3, 1]
    got = _blend_framed([_device_raw(i) for i in order], [_shape_case(i)[1] for i in order], pal, 0.6, skip_zero, reverse)
    for k, i in enumerate(order):
        assert torch.equal(got[k], singles[i]), f"{SHAPES[i]} differs inside the mixed list"
    # the public function: maps that are not views of one buffer are gathered, views are used where they lie
    raws = [_device_raw(i) for i in order]
    pub = blend(raws, [_shape_case(i)[1].to(DEV) for i in order], pal, 0.6, skip_zero=skip_zero,
                channel_order="bgr" if reverse else "rgb")
    assert all(torch.equal(a.cpu(), singles[i]) for a, i in zip(pub, order))
    assert all(a.dtype == torch.uint8 and tuple(a.shape) == (*SHAPES[i], 3) for a, i in zip(pub, order))
    assert len({a.untyped_storage().data_ptr() for a in pub}) == 1, "the results are views of one buffer"
    flat = torch.cat([_shape_case(i)[1].reshape(-1) for i in order]).to(DEV)
    views, o = [], 0
    for i in order:
        h, w = SHAPES[i]
        views.append(flat[o:o + h * w].view(h, w))
        o += h * w
    pub = blend(raws, views, pal, 0.6, skip_zero=skip_zero, channel_order="bgr" if reverse else "rgb")
    assert all(torch.equal(a.cpu(), singles[i]) for a, i in zip(pub, order))


# ------------------------------------------------------------------------------------------------ 3. anchors
def test_anchors_exact():
    P = 6
    g = torch.Generator().manual_seed(41)
    a = torch.randint(1, 4, (40, 60), generator=g, dtype=torch.uint8)   # 2400 pixels: three workgroup tiles
    a[17, 23] = 4                # a label on a single pixel
    a[39, :] = 1
    a[:, 59] = 1
    a[39, 59] = 5                # a label only in the last row and column
    a[0:3, 0:7] = 9              # indices >= P: not counted
    a[20, 30:40] = 200
    b = torch.full((5, 9), 2, dtype=torch.uint8)     # one label, the others absent
    c = torch.randint(0, 6, (7, 13), generator=g, dtype=torch.uint8)
    c[c == 3] = 0                # label 3 absent
    maps = [a, b, c]
    assert ops.SEG_RENDER_TILE < a.numel()
    raws = [torch.randint(0, 256, (*m.shape, 3), generator=g, dtype=torch.uint8).to(DEV) for m in maps]
    pal = torch.randint(0, 256, (P, 3), generator=g, dtype=torch.uint8)
    imgs, sums = blend(raws, [m.to(DEV) for m in maps], pal, 0.6, skip_zero=True, anchors=True)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (3, P, 3) and sums.is_cuda
    sums = sums.cpu()
    want = np.stack([rr.sums(m.numpy(), P) for m in maps])
    assert np.array_equal(sums.numpy(), want), (sums.tolist(), want.tolist())
    assert want[0, 4].tolist() == [1, 17, 23] and want[0, 5].tolist() == [1, 39, 59]
    assert want[1, 2, 0] == 45 and int(want[1, :, 0].sum()) == 45 and want[2, 3].tolist() == [0, 0, 0]
    assert int(want[0, :, 0].sum()) == a.numel() - 21 - 10
    got = anchors_from_sums(sums)
    assert got == [rr.anchors(m.numpy(), P) for m in maps]
    assert (4, 17, 23) in got[0] and (5, 39, 59) in got[0] and got[1] == [(2, 2, 4)]
    # the pictures of the same call are the plain blend's, and a second call adds the same integers again
    for im, raw, m in zip(imgs, raws, maps):
        assert np.array_equal(im.cpu().numpy(), rr.blend(raw.cpu().numpy(), m.numpy(), pal.numpy(), 0.6, skip_zero=True))
    again = _blend_framed(raws, maps, pal, 0.6, True, False, sums=(acc := torch.from_numpy(want).to(DEV).clone()))
    assert all(torch.equal(x, y.cpu()) for x, y in zip(again, imgs))
    assert np.array_equal(acc.cpu().numpy(), 2 * want), "sums are added to"


# ------------------------------------------------------------------------------------------------ 4. the group-map kernel
# name: (G, grid, network size, output size, seed)
GROUP_CASES = {
    "down": (8, (14, 14), (224, 224), (100, 75), 11),
    "odd": (3, (3, 5), (48, 80), (61, 37), 12),
    "up": (8, (14, 14), (224, 224), (333, 500), 16),
    "grid28": (8, (28, 28), (448, 448), (375, 500), 20),
    "one_pixel": (8, (14, 14), (224, 224), (1, 1), 15),
}
# name: (output pixels, pixels of the fp64 yardstick whose top-two gap is below TIE)
GROUP_TIE_COUNTS = {
    "down": (7500, 0),
    "odd": (2257, 0),
    "up": (166500, 1),
    "grid28": (187500, 0),
    "one_pixel": (1, 0),
}


@functools.lru_cache(maxsize=None)
def _group_case(name):
    G, grid, net, out, seed = GROUP_CASES[name]
    soft = torch.softmax(2.0 * torch.randn(G, *grid, generator=torch.Generator().manual_seed(seed)), dim=0)
    want, gap = rr.group_map(soft, net, out)
    return soft, want, gap < TIE


def _run_groups(names, pad=4):
    """One launch over the cases -> [(oh, ow) uint8 on the CPU]; the buffer's frame and gaps must stay untouched."""
    rows, floats, softs = [], 0, []
    for k, name in enumerate(names):
        G, grid, net, out, _ = GROUP_CASES[name]
        soft = _group_case(name)[0]
        rows.append(dict(first=k, count=1, net=net, out=out, win=net, grid=grid, soft_off=floats))
        floats += soft.numel()
        softs.append(soft.reshape(-1))
    G = GROUP_CASES[names[0]][0]
    assert all(GROUP_CASES[n][0] == G for n in names)
    images, offs, nbytes, n_blocks, _ = ops.seg_image_table(rows, DEV)
    buf = torch.full((nbytes + 2 * pad,), SENT8, dtype=torch.uint8, device=DEV)
    ops.seg_groups_rescaled(torch.cat(softs).to(DEV), images, n_blocks, G, buf[pad:pad + nbytes])
    torch.cuda.synchronize()
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    got = []
    host = buf.cpu()
    for o, name in zip(offs, names):
        oh, ow = GROUP_CASES[name][3]
        keep[pad + o:pad + o + oh * ow] = False
        got.append(host[pad + o:pad + o + oh * ow].view(oh, ow).clone())
    assert bool((host[keep] == SENT8).all()), "the kernel wrote outside its output"
    return got


@functools.lru_cache(maxsize=None)
def _single(name):
    return _run_groups([name], pad=4 if GROUP_CASES[name][-1] % 2 else 7)[0]


@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_group_map_against_reference(name):
    _, want, tie = _group_case(name)
    n_tie = int(tie.sum())
    got = _single(name)
    print(f"{name}: {tie.numel()} output pixels, {n_tie} near-ties, groups differ at {int((got.long() != want).sum())}, "
          f"{got.unique().numel()} distinct groups")
    assert (tie.numel(), n_tie) == GROUP_TIE_COUNTS[name], "the reference's own count changed"
    assert n_tie <= CAP * tie.numel()
    assert bool((got.long() == want)[~tie].all()), f"{name}: groups differ away from near-ties"
    if tie.numel() > 1000:
        assert got.unique().numel() == GROUP_CASES[name][0]


def test_group_maps_mixed_list():
    names = ["up", "one_pixel", "grid28", "down"]   # G = 8
    got = _run_groups(names)
    for g, name in zip(got, names):
        assert torch.equal(g, _single(name)), f"{name} differs inside the mixed list"


def test_group_kernel_limits():
    G, grid, net, out, _ = GROUP_CASES["odd"]
    soft = _group_case("odd")[0].reshape(-1).to(DEV)
    row = dict(first=0, count=1, net=net, out=out, win=net, grid=grid, soft_off=0)
    images, offs, nbytes, n_blocks, _ = ops.seg_image_table([row, row], DEV)
    ref = _single("odd")
    n = out[0] * out[1]
    # a row the device refuses is skipped and leaves the other image alone
    for col, value in ((1, 2), (9, net[0] - 1), (13, 1), (13, -1), (11, 0), (4, 1 << 30), (6, nbytes)):
        table = images.clone()
        table[1, col] = value
        buf = torch.full((nbytes,), SENT8, dtype=torch.uint8, device=DEV)
        ops.seg_groups_rescaled(soft, table, n_blocks, G, buf)
        torch.cuda.synchronize()
        host = buf.cpu()
        assert torch.equal(host[:n].view(out), ref), f"column {col} = {value}: the other image changed"
        assert bool((host[offs[1]:] == SENT8).all()), f"column {col} = {value}: a refused image was written"
    with pytest.raises(L.Unsupported, match="groups"):
        ops.seg_groups_rescaled(soft, images, n_blocks, 9, torch.empty(nbytes, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ 5., 6. end to end
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(150, 200), (97, 61), (200, 150)]
NETS = [(128, 128), (64, 64), (128, 128)]


def _raws(seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in RAW_SIZES]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_groups_list_identity():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.03)
        img = torch.randn(3, 3, 128, 128, generator=torch.Generator().manual_seed(8)).to(DEV)
        want = seg.group_map(img)
        got = seg.groups_list(list(img))
        assert [tuple(t.shape) for t in got] == [(128, 128)] * 3 and all(t.dtype == torch.uint8 for t in got)
        assert want.unique().numel() > 1
        assert _same(got, list(want)), "out size = network size must reproduce group_map bit for bit"
        # another output size: the fp64 yardstick on this build's soft assignment
        outs = [(150, 200), (31, 47), (128, 128)]
        got = seg.groups_list(list(img), outs)
        with torch.no_grad(), segclip_amd.config.scope(cross_mode="intended"):
            soft = model.clip.encode_image(img, return_hidden=True)[2]["attns"][-1]["soft_attn"]
        p = model.clip.visual.patch_size
        soft = soft.cpu().view(3, soft.shape[1], 128 // p, 128 // p)
        for i, out in enumerate(outs):
            ref, gap = rr.group_map(soft[i], (128, 128), out)
            tie = gap < TIE
            assert tuple(got[i].shape) == out
            assert bool((got[i].cpu().long() == ref)[~tie].all()) and int(tie.sum()) <= CAP * tie.numel()
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_render_raw_end_to_end():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        raws = _raws()
        seg = SegInference(model, emb, True, bg_thresh=0.03)
        pal = torch.randint(0, 256, (seg.num_classes, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
        modes = ["input", "pred", "input_pred", "input_pred_label", "all_groups", "first_group", "final_group"]
        with CountedEncodeImage(model) as calls:
            labels = seg.predict_raw(raws, TF, net_sizes=NETS)
            alone = list(calls)
            del calls[:]
            res = seg.render_raw(raws, TF, modes, pal, net_sizes=NETS)
            assert calls == alone == [2, 1], "render_raw runs the tower exactly as predict_raw does"
            del calls[:]
            gmaps = seg.groups_raw(raws, TF, net_sizes=NETS)
            assert calls == alone
        assert sorted(res) == sorted(modes)
        assert _same(res["input"], raws)
        assert _same(res["pred"], labels), "the labels of render_raw are predict_raw's"
        assert [tuple(t.shape) for t in gmaps] == RAW_SIZES
        G = int(max(int(t.max()) for t in gmaps)) + 1
        gp = default_group_palette(8)
        for i, raw in enumerate(raws):
            r, lab, grp = raw.cpu().numpy(), labels[i].cpu().numpy(), gmaps[i].cpu().numpy()
            assert np.array_equal(res["input_pred"][i].cpu().numpy(), rr.blend(r, lab, pal.numpy(), 0.8, skip_zero=True))
            assert np.array_equal(res["input_pred_label"][0][i].cpu().numpy(), rr.blend(r, lab, pal.numpy(), 0.6, skip_zero=True))
            assert res["input_pred_label"][1][i] == [a for a in rr.anchors(lab) if a[0] != 0]
            want = rr.blend(r, grp, gp.numpy(), 0.6)
            assert np.array_equal(res["final_group"][i].cpu().numpy(), want)
            assert torch.equal(res["first_group"][i], res["final_group"][i])
            assert len(res["all_groups"][i]) == 1 and torch.equal(res["all_groups"][i][0], res["final_group"][i])
        print(f"{G} groups drawn, {len(torch.cat([t.reshape(-1) for t in labels]).unique())} distinct labels")
        assert G > 1
        # a BGR source, a palette of the caller's, no background class
        bgr = ImageTransform(channel_order="bgr")
        seg_nb = SegInference(model, emb, False)
        own = torch.randint(0, 256, (12, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
        flipped = [t.flip(2).contiguous() for t in raws]
        res = seg_nb.render_raw(flipped, bgr, ["input_pred", "final_group"], pal[1:], group_palette=own, net_sizes=NETS)
        lab_nb = seg_nb.predict_raw(flipped, bgr, net_sizes=NETS)
        for i, raw in enumerate(flipped):
            assert np.array_equal(res["input_pred"][i].cpu().numpy(),
                                  rr.blend(raw.cpu().numpy(), lab_nb[i].cpu().numpy(), pal[1:].numpy(), 0.8, reverse_channels=True))
            assert np.array_equal(res["final_group"][i].cpu().numpy(),
                                  rr.blend(raw.cpu().numpy(), gmaps[i].cpu().numpy(), own[:8].numpy(), 0.6, reverse_channels=True))
        # only the input: no tower call at all
        with CountedEncodeImage(model) as calls:
            assert _same(seg.render_raw(raws, TF, ["input"], pal, net_sizes=NETS)["input"], raws) and calls == []
        with pytest.raises(ValueError, match="unknown vis mode"):
            seg.render_raw(raws, TF, ["input", "groups"], pal, net_sizes=NETS)
        with pytest.raises(ValueError, match="group palette"):
            seg.render_raw(raws, TF, ["final_group"], pal, group_palette=own[:3], net_sizes=NETS)
        # slide mode: an image of several windows has no group map; one of a single window has
        slide = SegInference(model, emb, True, bg_thresh=0.03, **SLIDE)
        with pytest.raises(ValueError, match="image 1"):
            slide.groups_raw(raws[:2], TF, net_sizes=[(128, 128), (128, 224)])
        one = slide.groups_raw(raws[:1], TF, net_sizes=[(128, 128)])
        assert _same(one, seg.groups_raw(raws[:1], TF, net_sizes=[(128, 128)]))
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ 7. rejections
def test_wrapper_rejections():
    raw = torch.zeros(6, 9, 3, dtype=torch.uint8, device=DEV)
    idx = torch.zeros(6, 9, dtype=torch.uint8, device=DEV)
    pal = torch.zeros(4, 3, dtype=torch.uint8)
    assert tuple(blend([raw], [idx], pal)[0].shape) == (6, 9, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blend([raw.cpu()], [idx], pal)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blend([raw], [idx.cpu()], pal)
    with pytest.raises(ValueError, match="uint8"):
        blend([raw.float()], [idx], pal)
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        blend([raw[:, :, :2]], [idx], pal)
    with pytest.raises(ValueError, match="index map"):
        blend([raw], [idx.long()], pal)
    with pytest.raises(ValueError, match="index map"):
        blend([raw], [idx[:, :8]], pal)
    with pytest.raises(ValueError, match="index maps"):
        blend([raw, raw], [idx], pal)
    for opacity in (0.0, 1.0001, -1.0):
        with pytest.raises(ValueError, match="opacity"):
            blend([raw], [idx], pal, opacity=opacity)
    for bad in (torch.zeros(257, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 3), torch.zeros(0, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="palette"):
            blend([raw], [idx], bad)
    with pytest.raises(ValueError, match="contiguous pixels"):
        blend([raw[:, ::2]], [idx[:, ::2]], pal)
    with pytest.raises(ValueError, match="CPU copy"):
        anchors_from_sums(torch.zeros(1, 4, 3, dtype=torch.int64, device=DEV))
    # the C entry's own checks
    table, offs, nbytes, n_blocks = ops.seg_blend_table([raw], [0])
    out = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="sums"):
        ops.seg_blend(table, n_blocks, idx.view(-1), pal.to(DEV), 0.5, out, sums=torch.zeros(1, 5, 3, dtype=torch.int64, device=DEV))
    lib = L.load()
    rc = lib.segclip_seg_blend(L.ptr(table), 1, n_blocks, L.ptr(idx), idx.numel(), L.ptr(pal.to(DEV)), 257, 0, 0.5, 0.5, 0, L.ptr(out),
                               nbytes, None, L.stream())
    assert rc == -1 and b"palette" in lib.segclip_last_error_string()
    # a row the device refuses is skipped: nothing of it is written or counted
    for col, value in ((0, 0), (3, 3 * 9 - 1), (1, 1 << 15), (2, 0), (4, 1), (5, 4)):
        bad = table.clone()
        bad[0, col] = value
        out = torch.full((nbytes,), SENT8, dtype=torch.uint8, device=DEV)
        sums = torch.zeros(1, 4, 3, dtype=torch.int64, device=DEV)
        ops.seg_blend(bad, n_blocks, idx.view(-1), pal.to(DEV), 0.5, out, sums=sums)
        torch.cuda.synchronize()
        assert bool((out == SENT8).all()) and int(sums.abs().sum()) == 0, f"column {col} = {value}"


def _reference_counts():
    """CPU: the GROUP_TIE_COUNTS table."""
    for name in GROUP_CASES:
        _, want, tie = _group_case(name)
        print(f'    "{name}": ({tie.numel()}, {int(tie.sum())}),   # {want.unique().numel()} distinct groups')


if __name__ == "__main__":
    _reference_counts()
