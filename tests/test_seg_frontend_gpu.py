"""GPU: the segmentation front end - segclip_seg_windows_from_u8 (csrc/segment_frontend.inc), ops.seg_windows_from_u8,
segmentation.preprocess / SegInference.predict_raw / SegEvaluator.update_raw and train.eval_epoch(transform=...) - against
tests/seg_frontend_reference.py (fp64).

Tolerance of the kernel: 5e-6 absolute on the normalised output, every pixel.  The values are at most 2.3 in magnitude; an
fp32 emulation of the formula stays within 6.4e-7 of fp64 on these shapes, and the margin covers fused multiply-adds and the
few fp32 roundings of at most 255 * 2^-24 grey levels each.  The value is continuous in the coordinates: there are no ties.
The identity case has every weight 0 and must equal (v - mean) * inv_std in fp32 to the last bit.
"""
import functools
import math

import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import ImageTransform, SegEvaluator, SegInference, preprocess, slide_windows
from segclip_amd.train import eval_epoch
from tests import seg_frontend_reference as sfr
from tests.helpers import CountedEncodeImage, load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-6
SENT = -12345.5   # guard pattern: no output value comes near it
TF = ImageTransform()

# name: (source (h, w), network (H, W))
CASES = {
    "down_tall": ((500, 375), (299, 224)),
    "down_wide": ((281, 500), (224, 399)),
    "strong_down": ((1200, 1600), (224, 299)),
    "up": ((37, 53), (128, 183)),
    "edges": ((5, 7), (128, 179)),
    "identity": ((64, 48), (64, 48)),
    "one_column": ((50, 1), (150, 128)),
    "one_row": ((1, 60), (128, 200)),
}
# (window, stride): mmseg's grid at crop 128 / stride 96 (overlapping windows, the last ones shifted back inside; a network
# size below 128 takes the whole side), and a window whose width is no multiple of 4 (scalar stores)
WINS = {"crop128": ((128, 128), (96, 96)), "w30": ((32, 30), (24, 22))}


def _grid(net, wkey):
    (wh, ww), stride = WINS[wkey]
    win = (min(wh, net[0]), min(ww, net[1]))
    return win, slide_windows(net[0], net[1], win, stride)


@functools.lru_cache(maxsize=None)
def _raw(name):
    g = torch.Generator().manual_seed(100 + list(CASES).index(name))
    return torch.randint(0, 256, (*CASES[name][0], 3), generator=g, dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _want(name, reverse=False):
    """(3, H, W) fp64 of a case; computed once and shared."""
    return sfr.resize_normalise(_raw(name), CASES[name][1], TF.mean, TF.inv_std, reverse)


def _launch(raws, nets, wins, win, reverse=False, pad=16, table=None):
    """The kernel into a framed buffer -> (n, 3, win_h, win_w) on the CPU; the frame (>= 64 bytes either side) is checked."""
    n = len(wins) * 3 * win[0] * win[1]
    buf = torch.full((n + 2 * pad,), SENT, dtype=torch.float32, device=DEV)
    out = buf[pad:pad + n]
    dwin = torch.tensor(wins, dtype=torch.int32, device=DEV).view(-1, 3)
    got = ops.seg_windows_from_u8(raws, nets, dwin, win, TF.mean, TF.inv_std, reverse_channels=reverse, out=out, table=table)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all()), "the kernel wrote outside its output"
    return out.view(len(wins), 3, *win).cpu()


# ------------------------------------------------------------------------------------------------ 1. kernel against fp64
@pytest.mark.parametrize("wkey", list(WINS))
@pytest.mark.parametrize("name", list(CASES))
def test_windows_against_reference(name, wkey):
    net = CASES[name][1]
    win, grid = _grid(net, wkey)
    wins = [(0, y, x) for (y, x) in grid]
    # an odd frame puts `out` off the 16-byte boundary: windows of a width that is a multiple of 4 then take scalar stores too
    got = _launch([_raw(name).to(DEV)], [net], wins, win, pad=16 if len(name) % 2 else 17)
    want = sfr.windows([_want(name)], wins, win)
    err = float((got.double() - want).abs().max())
    print(f"{name} {wkey}: {len(wins)} windows of {win}, largest error {err:.3e}, largest value {float(want.abs().max()):.3f}")
    assert float(want.abs().max()) <= 2.3
    assert err <= TOL
    if name == "identity":
        v = _raw(name).float().permute(2, 0, 1)
        exact = (v - torch.tensor(TF.mean)[:, None, None]) * torch.tensor(TF.inv_std)[:, None, None]
        assert torch.equal(got, sfr.windows([exact], wins, win)), "identity: not (v - mean) * inv_std to the last bit"


@pytest.mark.parametrize("wkey", list(WINS))
def test_several_images_in_one_launch(wkey):
    """All cases in one launch, in an order that mixes the sizes, one source a row-strided view of a larger tensor."""
    names = ["up", "down_tall", "one_row", "strong_down", "identity", "edges", "one_column", "down_wide"]
    raws = [_raw(n).to(DEV) for n in names]
    h, w = CASES["down_tall"][0]
    big = torch.full((h + 2, w + 9, 3), 77, dtype=torch.uint8, device=DEV)
    big[1:h + 1, 4:w + 4] = raws[1]
    raws[1] = big[1:h + 1, 4:w + 4]
    assert raws[1].stride() == (3 * (w + 9), 3, 1)
    nets = [CASES[n][1] for n in names]
    win = (32, 30) if wkey == "w30" else (64, 48)   # a window every network size holds
    stride = WINS[wkey][1]
    wins = [(i, y, x) for i, net in enumerate(nets) for (y, x) in slide_windows(net[0], net[1], win, stride)]
    got = _launch(raws, nets, wins, win)
    want = sfr.windows([_want(n) for n in names], wins, win)
    err = float((got.double() - want).abs().max())
    print(f"{len(names)} images, {len(wins)} windows of {win}: largest error {err:.3e}")
    assert err <= TOL
    # a window's pixels do not depend on what else the launch holds
    alone = _launch([raws[1]], [nets[1]], [(0, y, x) for (i, y, x) in wins if i == 1], win, pad=17)
    assert torch.equal(alone, got[[k for k, (i, _, _) in enumerate(wins) if i == 1]])


@pytest.mark.parametrize("name", ["down_wide", "up"])
def test_reverse_channels(name):
    net = CASES[name][1]
    win, grid = _grid(net, "crop128")
    wins = [(0, y, x) for (y, x) in grid]
    raw = _raw(name).to(DEV)
    got = _launch([raw], [net], wins, win, reverse=True)
    err = float((got.double() - sfr.windows([_want(name, True)], wins, win)).abs().max())
    print(f"{name} reversed: largest error {err:.3e}")
    assert err <= TOL
    # a BGR source read reversed = the same picture stored RGB, bit for bit
    assert torch.equal(got, _launch([raw.flip(2).contiguous()], [net], wins, win))


# ------------------------------------------------------------------------------------------------ 2. limits
def test_bad_windows_are_zero_filled():
    names = ["down_tall", "up"]
    raws, nets = [_raw(n).to(DEV) for n in names], [CASES[n][1] for n in names]
    win = (128, 128)
    good = [(0, 0, 0), (0, 171, 96), (1, 0, 55)]
    bad = [(0, 172, 0),     # one row below (299, 224)
           (1, 0, 56),      # one column right of (128, 183)
           (2, 0, 0), (7, 0, 0), (-1, 0, 0),   # no such image
           (0, -1, 0), (1, 0, -3)]
    wins = [good[0], bad[0], bad[1], good[1], bad[2], bad[3], bad[4], good[2], bad[5], bad[6]]
    got = _launch(raws, nets, wins, win)
    ref = _launch(raws, nets, good, win, pad=20)
    at = [wins.index(g) for g in good]
    assert torch.equal(got[at], ref), "a bad window changed the other windows of its launch"
    rest = [k for k in range(len(wins)) if k not in at]
    assert bool((got[rest] == 0).all()), "a window outside its image or without an image is zero-filled"
    want = sfr.windows([_want(n) for n in names], good, win)
    assert float((ref.double() - want).abs().max()) <= TOL
    # an image row the device refuses: a size of 2^15, a stride below 3 w, a null address
    for col, value in ((2, 1 << 15), (1, 0), (5, 1 << 15), (3, 3 * CASES["up"][0][1] - 1), (0, 0)):
        table = ops.seg_source_table(raws, nets)
        table[1, col] = value
        got = _launch(raws, nets, good, win, table=table)
        assert torch.equal(got[:2], ref[:2]) and bool((got[2] == 0).all()), f"image row with column {col} = {value}"
    # the scalar-store path at the same limits
    got = _launch(raws, nets, [(0, 0, 0), (0, 268, 0), (3, 0, 0), (1, 96, 153)], (32, 30))
    assert bool((got[1:3] == 0).all())
    want = sfr.windows([_want(n) for n in names], [(0, 0, 0), (1, 96, 153)], (32, 30))
    assert float((got[[0, 3]].double() - want).abs().max()) <= TOL


def test_host_wrapper_rejects():
    raw = _raw("up").to(DEV)
    net = CASES["up"][1]
    call = lambda r, n=net, w=[(0, 0, 0)], win=(32, 32): ops.seg_windows_from_u8([r], [n], w, win, TF.mean, TF.inv_std)
    assert tuple(call(raw).shape) == (1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(raw.cpu())
    with pytest.raises(TypeError, match="uint8"):
        call(raw.float())
    with pytest.raises(ValueError, match="contiguous pixels"):
        call(raw[:, ::2])                          # every second pixel: stride(1) = 6
    with pytest.raises(ValueError, match="contiguous pixels"):
        call(raw.permute(2, 0, 1).contiguous().permute(1, 2, 0))   # planar channels
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        call(raw[:, :, :2])
    with pytest.raises(ValueError, match="sizes 1"):
        call(raw, n=(1 << 15, 64))
    with pytest.raises(ValueError, match="sizes 1"):
        call(raw, n=(0, 64))
    with pytest.raises(ValueError, match="network sizes"):
        ops.seg_windows_from_u8([raw, raw], [net], [(0, 0, 0)], (32, 32), TF.mean, TF.inv_std)
    with pytest.raises(L.Unsupported):             # 2^31 pixels per window; no window, so nothing is allocated
        call(raw, w=torch.empty(0, 3, dtype=torch.int32, device=DEV), win=(1 << 16, 1 << 15))


# ------------------------------------------------------------------------------------------------ 3. end to end
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(300, 300), (500, 375), (375, 500), (281, 500)]
NET_SIZES = [(224, 224), (299, 224), (224, 299), (224, 399)]


def _raws(seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in RAW_SIZES]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_predict_raw_equals_predict_list_on_preprocessed():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        raws = _raws()
        outs = [(h + 3, w - 2) for (h, w) in RAW_SIZES]
        pre = preprocess(raws, TF)
        assert [tuple(t.shape) for t in pre] == [(3, *n) for n in NET_SIZES] and all(t.dtype == torch.float32 for t in pre)
        for i, (raw, net) in enumerate(zip(raws, NET_SIZES)):   # preprocess itself against fp64
            want = sfr.resize_normalise(raw.cpu(), net, TF.mean, TF.inv_std)
            assert float((pre[i].cpu().double() - want).abs().max()) <= TOL
        seg = SegInference(model, emb, True, bg_thresh=0.03, **SLIDE)
        total = sum(len(slide_windows(H, W, SLIDE["crop_size"], SLIDE["stride"])) for (H, W) in NET_SIZES)
        with CountedEncodeImage(model) as calls:
            want = seg.predict_list(pre, outs)
            got = seg.predict_raw(raws, TF, outs)
            assert calls == [total, total]
            assert _same(got, want), "the tower did not see bit-identical windows"
            for mw in (1, 3, 256):
                del calls[:]
                chunked = SegInference(model, emb, True, bg_thresh=0.03, max_windows=mw, **SLIDE).predict_raw(raws, TF, outs)
                assert len(calls) == math.ceil(total / mw) and max(calls) <= mw, (mw, calls)
                assert _same(chunked, want), f"max_windows={mw} differs"
        assert [tuple(t.shape) for t in got] == outs and all(t.dtype == torch.uint8 for t in got)
        print(f"{total} windows, {len(torch.cat([t.reshape(-1) for t in got]).unique())} distinct labels")
        # default output shapes: the raw images' own sizes
        own = seg.predict_raw(raws, TF)
        assert [tuple(t.shape) for t in own] == RAW_SIZES
        assert _same(own, seg.predict_list(pre, RAW_SIZES))
        # BGR sources
        bgr = ImageTransform(channel_order="bgr")
        assert _same(seg.predict_raw([t.flip(2).contiguous() for t in raws], bgr, outs), want)
        # whole mode: one tower call per distinct network size, sizes the tower takes
        nets = [(128, 128), (64, 64), (128, 128), (64, 64)]
        whole = SegInference(model, emb, True, bg_thresh=0.03)
        with CountedEncodeImage(model) as calls:
            got = whole.predict_raw(raws, TF, outs, net_sizes=nets)
            assert calls == [2, 2]
        pre_w = preprocess(raws, TF, net_sizes=nets)
        assert [tuple(t.shape) for t in pre_w] == [(3, *n) for n in nets]
        assert _same(got, whole.predict_list(pre_w, outs))
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_update_raw_and_eval_epoch():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        tokens = torch.from_numpy(g["prompt_ids"])
        raws = _raws(seed=6)
        pre = preprocess(raws, TF)
        cfg = dict(bg_thresh=0.03, **SLIDE)
        seg = SegInference(model, emb, True, **cfg)
        gts = [torch.randint(0, 14, o, generator=torch.Generator().manual_seed(9 + i)).to(torch.uint8).to(DEV)
               for i, o in enumerate(RAW_SIZES)]
        for t in gts:
            t[5:9] = 255
        ref = SegEvaluator(seg)
        ref.update(pre, gts)
        ev = SegEvaluator(seg)
        assert ev.update_raw(raws, gts, TF) is None
        assert int(ref.areas[1].sum()) > 0 and torch.equal(ev.areas, ref.areas)
        perm = [2, 0, 3, 1]
        ev2 = SegEvaluator(seg)
        labels = ev2.update_raw([raws[i] for i in perm], [gts[i] for i in perm], TF, return_labels=True)
        assert _same(labels, [seg.predict_raw(raws, TF)[i] for i in perm])
        ev3 = SegEvaluator(seg)
        for raw, t in zip(raws, gts):
            ev3.update_raw([raw], [t], TF)
        assert torch.equal(ev2.areas, ref.areas) and torch.equal(ev3.areas, ref.areas)
        # eval_epoch: raw batches with a transform = pre-processed batches without
        batches_raw = [([t.cpu() for t in raws[:2]], [t.cpu() for t in gts[:2]]), ([t.cpu() for t in raws[2:]], [t.cpu() for t in gts[2:]])]
        batches_pre = [([t.cpu() for t in pre[:2]], batches_raw[0][1]), ([t.cpu() for t in pre[2:]], batches_raw[1][1])]
        model.train()   # eval_epoch switches to eval mode itself
        got = eval_epoch(None, model, DEV, 1, batches_raw, tokens, True, cfg, transform=TF)
        want = eval_epoch(None, model, DEV, 1, batches_pre, tokens, True, cfg)
        print(f"eval_epoch: raw {got:.6f}, pre-processed {want:.6f}")
        assert got == want and 0.0 < got < 100.0
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_interface_errors():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        seg = SegInference(model, emb, True, **SLIDE)
        ev = SegEvaluator(seg)
        raw = torch.zeros(300, 300, 3, dtype=torch.uint8, device=DEV)
        gt = torch.zeros(300, 300, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match="output shapes"):
            seg.predict_raw([raw, raw], TF, [(300, 300)])
        with pytest.raises(ValueError, match="network sizes"):
            seg.predict_raw([raw, raw], TF, net_sizes=[(224, 224)])
        with pytest.raises(ValueError, match="ground truths"):
            ev.update_raw([raw, raw], [gt], TF)
        with pytest.raises(ValueError, match="empty image list"):
            seg.predict_raw([], TF)
        with pytest.raises(ValueError, match="smaller than the crop"):
            seg.predict_raw([raw], ImageTransform(img_scale=(2048, 100)))
        with pytest.raises(ValueError, match="at most 64"):
            seg.predict_raw([raw], TF, net_sizes=[(128 + 8 * 96, 128 + 8 * 96)])
        with pytest.raises(ValueError, match="multiple of the patch size"):
            SegInference(model, emb, True).predict_raw([raw], TF, net_sizes=[(100, 128)])
        with pytest.raises(ValueError, match="channel_order"):
            ImageTransform(channel_order="rbg")
        with pytest.raises(ValueError, match="uint8"):
            seg.predict_raw([raw.float()], TF)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            seg.predict_raw([raw.cpu()], TF)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ev.update_raw([raw], [gt.cpu()], TF)
        assert int(ev.areas.abs().sum()) == 0
        model.train()
        with pytest.raises(RuntimeError, match="model.eval"):
            seg.predict_raw([raw], TF)
        model.eval()
        assert tuple(seg.predict_raw([raw], TF)[0].shape) == (300, 300)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
