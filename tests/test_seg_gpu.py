"""GPU: the zero-shot segmentation kernels (csrc/segment.hip) and segclip_amd.segmentation against tests/seg_reference.py
(fp64, pinned to the real reference by tests/test_seg_reference_golden.py) and against the real reference's encode_decode
(tests/golden/seg_tiny.npz).

Near-ties.  Labels and groups are arg-maxima, so a pixel may legitimately differ from the fp64 yardstick where the top two
candidates are closer than fp32 resolves.  A differing pixel is accepted only as a VERIFIED near-tie: in the fp64 reference
the top two interpolated group values of a covering window (or, where windows overlap, the top two class sums) differ by
less than 1e-6.  Any other mismatch fails, and near-ties may be at most 0.01 % of a case's pixels (a fixed condition, not
a measurement: a seed whose reference alone exceeds it is replaced, the cap is not raised).  Counted on the CPU for the seeds used below, fp32 seg_reference against fp64 seg_reference
(tests/test_seg_gpu.py::_reference_counts, run with `python -m tests.test_seg_gpu`): pixels with a group gap below 1e-6 /
pixels where the fp32 arg-max differs - see NEAR_TIE_COUNTS (at most 4 of 301 056 = 0.0013 %); the slide cases, per window
pixel: 224 x 224: 0 / 0 of 100 352, 448 x 448: 4 / 0 of 401 408, 300 x 500: 9 / 0 of 602 112, 225 x 224: 0 / 0 of 200 704,
300 x 340 at stride 112: 4 / 0 of 602 112.  The golden's own soft_attn at the looser 1e-4 gap of the end-to-end test: 7 and
1 of 32 768 pixels (0.02 %).
"""
import math

import numpy as np
import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import SegInference, build_text_embedding
from tests import seg_reference as sr
from tests.helpers import load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8, SENTF = 0xA5, -12345.0
TIE, CAP = 1e-6, 1e-4

# (name, B, G, gh, gw, H, W, N, with_bg, seed)
PIXEL_CASES = [
    ("tiny", 2, 8, 4, 4, 64, 64, 3, True, 1),
    ("224", 1, 8, 14, 14, 224, 224, 21, True, 2),
    ("448x672", 1, 8, 28, 42, 448, 672, 21, False, 3),
    ("grid1x1", 2, 8, 1, 1, 16, 16, 3, True, 4),
    ("tails", 1, 8, 4, 4, 61, 67, 5, True, 5),
    ("tails_w2", 2, 5, 3, 5, 30, 50, 5, False, 6),
    ("n1", 2, 8, 4, 4, 64, 64, 1, True, 7),
    ("n255", 1, 8, 4, 4, 64, 64, 255, True, 8),
    ("b9", 9, 8, 4, 4, 32, 48, 12, True, 9),
]
# name -> (pixels, fp64 group gaps below 1e-6, pixels where the fp32 reference's group differs from the fp64 one)
NEAR_TIE_COUNTS = {
    "tiny": (8192, 0, 0), "224": (50176, 1, 0), "448x672": (301056, 4, 0), "grid1x1": (512, 0, 0), "tails": (4087, 0, 0),
    "tails_w2": (3000, 0, 0), "n1": (8192, 0, 0), "n255": (4096, 0, 0), "b9": (13824, 0, 0),
}


def _soft(seed, nW, G, gh, gw):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.softmax(torch.randn(nW, G, gh, gw, generator=g) * (1.0 + seed % 4), dim=1)


def _features(seed, nW, G, N, Cc):
    g = torch.Generator().manual_seed(2000 + seed)
    gt, pf = torch.randn(nW, G, Cc, generator=g), torch.randn(nW, Cc, generator=g)
    tx = torch.randn(N, Cc, generator=g)
    return gt, pf, tx / tx.norm(dim=-1, keepdim=True)


def _f32_tables(tab):
    """The reference table rounded to fp32, and everything derived from it exactly (both sides then read the same numbers)."""
    t = tab["table"].float()
    score, cls = t.max(dim=-1)
    t32 = dict(table=t, table_max=t.amax(dim=(1, 2)), best_class=cls, best_score=score)
    dev = (t.to(DEV), t32["table_max"].to(DEV), cls.int().to(DEV), score.to(DEV))
    return t32, dev


def _framed(shape, dtype, pad):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), SENT8 if dtype == torch.uint8 else SENTF, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n]


def _frame_intact(buf, pad):
    s = SENT8 if buf.dtype == torch.uint8 else SENTF
    return bool((buf[:pad] == s).all()) and bool((buf[buf.numel() - pad:] == s).all())


def _lists(wins, B):
    per = len(wins) // B
    return (torch.tensor(wins, dtype=torch.int32, device=DEV).view(-1, 3),
            torch.arange(0, len(wins) + 1, per, dtype=torch.int32, device=DEV))


def _run_pixel(soft, dev_tabs, wins, out_size, win, grid, with_bg, thr, pad=64):
    """labels, groups, logits through framed outputs, launched twice (bit-equal), frames checked."""
    B, H, W = out_size
    dw, df = _lists(wins, B)
    N = dev_tabs[0].shape[2]
    sd = soft.reshape(soft.shape[0], soft.shape[1], -1).to(DEV)
    res = []
    for _ in range(2):
        bl, vl = _framed(out_size, torch.uint8, pad)
        bg, vg = _framed(out_size, torch.uint8, pad)
        bo, vo = _framed((B, N + int(with_bg), H, W), torch.float32, pad)
        if N + int(with_bg) <= 256:
            ops.seg_label_map(sd, dev_tabs, dw, df, out_size, win, grid, with_bg, thr, labels=vl, groups=vg)
        else:
            ops.seg_label_map(sd, dev_tabs, dw, df, out_size, win, grid, with_bg, thr, labels=False, groups=vg)
        ops.seg_logits(sd, dev_tabs, dw, df, out_size, win, grid, with_bg, thr, out=vo)
        torch.cuda.synchronize()
        assert _frame_intact(bl, pad) and _frame_intact(bg, pad) and _frame_intact(bo, pad), "a kernel wrote outside its output"
        res.append((vl.view(out_size).cpu().long(), vg.view(out_size).cpu().long(), vo.view(B, -1, H, W).cpu()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b), "repeat launch differs"
    return res[0]


def _compare_maps(name, got, ref, check_labels=True):
    """Exact away from verified near-ties; near-ties capped at 0.01 % of the pixels."""
    labels, groups, logits = got
    tie = (ref["group_gap"] < TIE) | ((ref["count"] > 1) & (ref["class_gap"] < TIE))
    n_tie = int(tie.sum())
    print(f"{name}: {tie.numel()} pixels, {n_tie} near-ties, groups differ at {int((groups != ref['groups']).sum())}, "
          f"labels differ at {int((labels != ref['labels']).sum()) if check_labels else -1}")
    assert n_tie <= CAP * tie.numel(), f"{name}: {n_tie} near-ties of {tie.numel()} pixels in the reference itself"
    assert bool((groups == ref["groups"])[~tie].all()), f"{name}: groups differ away from near-ties"
    if check_labels:
        assert bool((labels == ref["labels"])[~tie].all()), f"{name}: labels differ away from near-ties"
    err = (logits.double() - ref["logits"]).abs().amax(dim=1)
    print(f"{name}: max logit error away from near-ties {float(err[~tie].max()):.3e}")
    assert float(err[~tie].max()) <= 1e-6, f"{name}: logits"


# ------------------------------------------------------------------------------------------------ 1. kernels in isolation
@pytest.mark.parametrize("nW,G,N,Cc,log_scale,topk", [
    (3, 8, 21, 512, math.log(1 / 0.07), 5), (2, 8, 1, 64, math.log(1 / 0.07), 1), (2, 8, 255, 512, math.log(1 / 0.07), 5),
    (1, 3, 12, 64, 1.0, 5), (9, 8, 5, 128, math.log(200.0), 5), (2, 8, 3, 64, math.log(1 / 0.07), 3)])
def test_group_table_against_reference(nW, G, N, Cc, log_scale, topk):
    """table / table_max / best_score to 1e-6 absolute, top-k mask equal, best_class equal wherever the reference's top two
    scores of the row differ by more than 1e-6.  log(200) exercises the clamp at 100.  Inputs are views of one
    (nW, 1 + G, C) tensor, as SegInference passes them."""
    gt, pf, tx = _features(nW * 100 + N, nW, G, N, Cc)
    ref = sr.group_table(gt, pf, tx, log_scale, topk)
    # precondition on the reference alone: the k-th and (k+1)-th pooled probabilities are not a near-tie
    if topk < N:
        pp = torch.softmax((pf.double() / pf.double().norm(dim=-1, keepdim=True)) @ tx.double().t()
                           * min(math.exp(log_scale), 100.0), dim=-1).sort(dim=-1, descending=True).values
        assert float((pp[:, topk - 1] - pp[:, topk]).min()) > 1e-6
    hidden = torch.cat([pf[:, None], gt], dim=1).to(DEV)
    ls = torch.tensor(log_scale, device=DEV)
    pad = 16
    outs = []
    for _ in range(2):
        bt, vt = _framed((nW, G, N), torch.float32, pad)
        bm, vm = _framed((nW,), torch.float32, pad)
        bs, vs = _framed((nW, G), torch.float32, pad)
        bc = torch.full((nW * G + 2 * pad,), -7, dtype=torch.int32, device=DEV)
        bk, vk = _framed((nW, N), torch.uint8, pad)
        g_view, p_view = hidden[:, 1:, :], hidden[:, 0, :]
        L.check(L.load().segclip_seg_group_table(L.ptr(g_view), g_view.stride(0), L.ptr(p_view), p_view.stride(0), L.ptr(tx.to(DEV)),
                                                 L.ptr(ls), L.ptr(vt), L.ptr(vm), L.ptr(bc[pad:]), L.ptr(vs), L.ptr(vk), nW, G, N, Cc,
                                                 topk, L.stream()), "seg_group_table")
        torch.cuda.synchronize()
        assert _frame_intact(bt, pad) and _frame_intact(bm, pad) and _frame_intact(bs, pad) and _frame_intact(bk, pad)
        assert bool((bc[:pad] == -7).all()) and bool((bc[pad + nW * G:] == -7).all())
        outs.append((vt.view(nW, G, N).cpu(), vm.cpu(), vs.view(nW, G).cpu(), bc[pad:pad + nW * G].view(nW, G).cpu().long(),
                     vk.view(nW, N).cpu().bool()))
    for a, b in zip(*outs):
        assert torch.equal(a, b), "repeat launch differs"
    table, tmax, score, cls, mask = outs[0]
    print(f"group_table N={N}: max table error {float((table.double() - ref['table']).abs().max()):.3e}")
    assert torch.equal(mask, ref["mask"])
    assert float((table.double() - ref["table"]).abs().max()) <= 1e-6
    assert float((tmax.double() - ref["table_max"]).abs().max()) <= 1e-6
    assert float((score.double() - ref["best_score"]).abs().max()) <= 1e-6
    clear = ref["row_gap"] > 1e-6
    assert torch.equal(cls[clear], ref["best_class"][clear])
    # and exactly consistent with the kernel's own table: first maximum of each row
    s2, c2 = table.max(dim=-1)
    assert torch.equal(c2, cls) and torch.equal(s2, score) and torch.equal(table.amax(dim=(1, 2)), tmax)
    # the wrapper gives the same bits
    w = ops.seg_group_table(hidden[:, 1:, :], hidden[:, 0, :], tx.to(DEV), ls, topk, want_mask=True)
    assert torch.equal(w[0].cpu(), table) and torch.equal(w[2].cpu().long(), cls) and torch.equal(w[4].cpu().bool(), mask)


def _pixel_case(case):
    name, B, G, gh, gw, H, W, N, with_bg, seed = case
    soft = _soft(seed, B, G, gh, gw)
    gt, pf, tx = _features(seed, B, G, N, 64)
    tab = sr.group_table(gt, pf, tx, math.log(1 / 0.07), min(5, N))
    return soft, tab


@pytest.mark.parametrize("case", PIXEL_CASES, ids=[c[0] for c in PIXEL_CASES])
@pytest.mark.parametrize("thr_kind", ["above", "below"])
def test_label_map_and_logits_against_reference(case, thr_kind):
    """One window per image (mode "whole"); label_map and logits read the SAME fp32 soft_attn and table as the fp64 reference.
    bg_thresh above (0.95 -> min picks the table maximum) and below (half the smallest table maximum) the maximum."""
    name, B, G, gh, gw, H, W, N, with_bg, seed = case
    soft, tab = _pixel_case(case)
    t32, dev_tabs = _f32_tables(tab)
    thr = 0.95 if thr_kind == "above" else 0.5 * float(t32["table_max"].min())
    wins, win = sr.window_list(B, H, W, "whole")
    ref = sr.assemble(soft, t32, wins, (B, H, W), win, with_bg, thr)
    got = _run_pixel(soft, dev_tabs, wins, (B, H, W), win, (gh, gw), with_bg, thr, pad=64 if seed % 2 else 3)
    _compare_maps(name, got, ref, check_labels=N + int(with_bg) <= 256)
    if N + int(with_bg) <= 256:
        assert torch.equal(got[0], got[2].argmax(dim=1)), "label map is not the first maximum of this build's logits"


def test_label_map_refuses_more_than_256_classes():
    soft, (gh, gw) = _soft(11, 1, 8, 4, 4), (4, 4)
    gt, pf, tx = _features(11, 1, 8, 256, 64)
    t32, dev_tabs = _f32_tables(sr.group_table(gt, pf, tx, 1.0, 5))
    dw, df = _lists([(0, 0, 0)], 1)
    with pytest.raises(L.Unsupported):
        ops.seg_label_map(soft.view(1, 8, -1).to(DEV), dev_tabs, dw, df, (1, 64, 64), (64, 64), (gh, gw), True, 0.9)
    ref = sr.assemble(soft, t32, [(0, 0, 0)], (1, 64, 64), (64, 64), True, 0.9)
    got = _run_pixel(soft, dev_tabs, [(0, 0, 0)], (1, 64, 64), (64, 64), (gh, gw), True, 0.9)
    _compare_maps("n256+bg", got, ref, check_labels=False)


# ------------------------------------------------------------------------------------------------ 2. slide geometry
@pytest.mark.parametrize("H,W,stride", [(224, 224, 224), (448, 448, 224), (300, 500, 224), (225, 224, 224), (300, 340, 112)])
def test_slide_geometry(H, W, stride):
    """mmseg's window grid (crop 224): one window, four without overlap, shifted last windows with 2- and 4-fold overlaps,
    and stride 112 (up to 6 windows on a pixel).  Window list equal to the reference's; maps as in the isolation test, with
    the class-sum near-tie rule in the overlaps."""
    B, G, N = 2, 8, 21
    seg = SegInference(None, torch.zeros(N, 8, device=DEV), True, mode="slide", crop_size=(224, 224), stride=(stride, stride))
    wins, win = seg.window_list(B, H, W)
    rwins, rwin = sr.window_list(B, H, W, "slide", (224, 224), (stride, stride))
    assert wins == rwins and tuple(win) == tuple(rwin)
    nW = len(wins)
    soft = _soft(H + W + stride, nW, G, 14, 14)
    gt, pf, tx = _features(H + W, nW, G, N, 64)
    t32, dev_tabs = _f32_tables(sr.group_table(gt, pf, tx, math.log(1 / 0.07), 5))
    thr = 0.5 * float(t32["table_max"].max())   # some windows above, some below their own maximum
    for with_bg in (True, False):
        ref = sr.assemble(soft, t32, wins, (B, H, W), win, with_bg, thr)
        assert float(ref["count"].min()) >= 1
        got = _run_pixel(soft, dev_tabs, wins, (B, H, W), win, (14, 14), with_bg, thr)
        _compare_maps(f"slide {H}x{W}/{stride} bg={with_bg} (max cover {int(ref['count'].max())})", got, ref)
        assert torch.equal(got[0], got[2].argmax(dim=1))


# ------------------------------------------------------------------------------------------------ 3. end to end
# label agreement of the bf16 towers with the exact-f32 run, tiny model, golden images, 12 classes + background: measured
# on an MI355X: 1.0 (128 x 128) and 0.99963 (256 x 64); floor = the smaller measurement - 10 %
BF16_AGREEMENT_MEASURED = 0.99963
BF16_AGREEMENT_FLOOR = BF16_AGREEMENT_MEASURED - 0.10


def test_end_to_end_against_reference_golden():
    """SegInference (exact-f32 towers) against the REAL reference's encode_decode: logits within 1e-3 at every pixel whose
    winning group is not a near-tie (gap below 1e-4 in the golden's own soft_attn: the encoder's 1e-5-level differences now
    sit in soft_attn); such pixels may be at most 0.25 % of a case (counted on the golden: 7 and 1 of 32 768).  predict equals
    the arg-max of this build's encode_decode exactly; build_text_embedding to 1e-4."""
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = build_text_embedding(model, torch.from_numpy(g["prompt_ids"]).to(DEV), chunk=7)
        assert float((emb.cpu() - torch.from_numpy(g["text_embedding"])).abs().max()) <= 1e-4
        for si, (H, W) in enumerate(g["sizes"].tolist()):
            image = torch.from_numpy(g[f"image_{si}"]).to(DEV)
            soft = torch.from_numpy(g[f"soft_{si}"])
            _, gap = sr.window_groups(soft.view(soft.shape[0], -1, H // 16, W // 16), H, W)
            tie = gap < 1e-4
            assert int(tie.sum()) <= 2.5e-3 * tie.numel()
            for ci, (with_bg, N, thr) in enumerate(g["cases"].tolist()):
                seg = SegInference(model, emb[:int(N)], bool(with_bg), bg_thresh=thr)
                logits = seg.encode_decode(image)
                ref = torch.from_numpy(g[f"logits_{si}_{ci}"])
                assert logits.shape == ref.shape
                err = (logits.cpu() - ref).abs().amax(dim=1)
                print(f"e2e {H}x{W} case {ci}: {int(tie.sum())} near-ties, max error elsewhere {float(err[~tie].max()):.3e}, "
                      f"label agreement {float((logits.cpu().argmax(1) == ref.argmax(1)).float().mean()):.5f}")
                assert float(err[~tie].max()) <= 1e-3
                labels = seg.predict(image)
                assert labels.dtype == torch.uint8 and tuple(labels.shape) == (image.shape[0], H, W)
                assert torch.equal(labels.cpu().long(), logits.cpu().argmax(dim=1))
                groups = seg.group_map(image)
                gref, _ = sr.window_groups(soft.view(soft.shape[0], -1, H // 16, W // 16), H, W)
                assert bool((groups.cpu().long() == gref)[~tie].all())
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_bf16_towers_label_agreement():
    """bf16 towers: predict runs; its agreement with the exact-f32 labels is printed and floored (see the constants above)."""
    g = load_golden("seg_tiny.npz")
    try:
        agree = []
        for si, (H, W) in enumerate(g["sizes"].tolist()):
            image = torch.from_numpy(g[f"image_{si}"]).to(DEV)
            labels = {}
            for dtype in (torch.float32, torch.bfloat16):
                model = tiny_seg_model(dtype)
                seg = SegInference(model, torch.from_numpy(g["text_embedding"]).to(DEV), True, bg_thresh=0.03)
                labels[dtype] = seg.predict(image).cpu()
            agree.append(float((labels[torch.float32] == labels[torch.bfloat16]).float().mean()))
        print(f"bf16 / f32 label agreement per size: {agree}")
        assert min(agree) >= BF16_AGREEMENT_FLOOR, agree
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ 4. batching invariance
@pytest.mark.parametrize("mode", ["whole", "slide"])
def test_batching_and_chunking_invariance(mode):
    """predict of B images in one call == B calls of one image == any max_windows chunking, bit for bit (exact-f32 mode)."""
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        gen = torch.Generator().manual_seed(5)
        kw = dict(mode="slide", crop_size=(64, 64), stride=(48, 40)) if mode == "slide" else {}
        image = (torch.randn(3, 3, 100, 150, generator=gen) if mode == "slide" else torch.randn(3, 3, 128, 128, generator=gen)).to(DEV)
        seg = SegInference(model, emb, True, bg_thresh=0.03, **kw)
        together = seg.predict(image)
        logits = seg.encode_decode(image)
        assert torch.equal(together.cpu().long(), logits.cpu().argmax(dim=1))
        for b in range(3):
            assert torch.equal(seg.predict(image[b:b + 1])[0], together[b]), f"image {b} alone differs"
        for mw in (1, 2, 5):
            chunked = SegInference(model, emb, True, bg_thresh=0.03, max_windows=mw, **kw)
            assert torch.equal(chunked.predict(image), together), f"max_windows={mw} differs"
            assert torch.equal(chunked.encode_decode(image), logits)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("mode", ["whole", "slide"])
def test_remembered_plan_serves_only_its_own_call_shape(mode):
    """SegInference remembers the plan and the device window list of its last call shape.  predict(a), predict(b), predict(a)
    with a and b of different shapes: the first and the third result are equal bit for bit and b's equals a fresh object's;
    predict_list of a's images straight after (the same sizes: the remembered plan serves it) equals a fresh object's."""
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        gen = torch.Generator().manual_seed(11)
        kw = dict(mode="slide", crop_size=(64, 64), stride=(48, 40)) if mode == "slide" else {}
        shape_a, shape_b = ((2, 3, 100, 150), (1, 3, 64, 64)) if mode == "slide" else ((2, 3, 128, 128), (1, 3, 256, 64))
        a, b = torch.randn(shape_a, generator=gen).to(DEV), torch.randn(shape_b, generator=gen).to(DEV)

        def fresh():
            return SegInference(model, emb, True, bg_thresh=0.03, **kw)

        seg = fresh()
        first, other, third = seg.predict(a), seg.predict(b), seg.predict(a)
        assert tuple(first.shape) == (2,) + shape_a[2:] and tuple(other.shape) == (1,) + shape_b[2:]
        assert torch.equal(first, third)
        assert torch.equal(other, fresh().predict(b))
        assert torch.equal(first, fresh().predict(a))
        listed, want = seg.predict_list(list(a)), fresh().predict_list(list(a))
        assert len(listed) == len(want) == 2
        for x, y in zip(listed, want):
            assert tuple(x.shape) == shape_a[2:] and torch.equal(x, y)
        assert torch.equal(seg.predict(b), other)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ 5. interface
def test_interface_errors_and_wide_class_lists():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        seg = SegInference(model, emb, True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            seg.predict(torch.zeros(1, 3, 128, 128))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            build_text_embedding(model, torch.from_numpy(g["prompt_ids"]))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            SegInference(model, emb.cpu(), True)
        gen = torch.Generator().manual_seed(3)
        wide = torch.randn(256, emb.shape[1], generator=gen)
        wide = (wide / wide.norm(dim=-1, keepdim=True)).to(DEV)
        image = torch.from_numpy(g["image_0"]).to(DEV)
        seg = SegInference(model, wide, True)
        with pytest.raises(L.Unsupported):
            seg.predict(image)
        logits = seg.encode_decode(image)
        assert tuple(logits.shape) == (image.shape[0], 257, 128, 128) and bool(torch.isfinite(logits).all())
        assert tuple(SegInference(model, wide[:255], True).predict(image).shape) == (image.shape[0], 128, 128)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_predict_allocates_less_than_one_fp32_plane_per_image():
    """predict's peak stays below the encoder's own peak + B * H * W * 4 bytes: no (H, W, N) / (H, W, G) tensor exists."""
    from segclip_amd import config
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        gen = torch.Generator().manual_seed(8)
        image = torch.randn(4, 3, 128, 128, generator=gen).to(DEV)
        seg = SegInference(model, emb, True)

        def encoder():
            with torch.no_grad(), config.scope(cross_mode="intended"):
                return model.clip.encode_image(image, return_hidden=True)

        def peak(fn):
            fn()
            torch.cuda.synchronize()   # warmed up: caches of the towers are filled
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            p = torch.cuda.max_memory_allocated() - base
            del out
            return p

        p_enc, p_pred = peak(encoder), peak(lambda: seg.predict(image))
        plane = image.shape[0] * 128 * 128 * 4
        print(f"encoder peak {p_enc} bytes, predict peak {p_pred} bytes, one fp32 plane per image {plane} bytes")
        assert p_pred - p_enc < plane
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def _reference_counts():
    """CPU: the NEAR_TIE_COUNTS table (fp32 seg_reference against fp64 seg_reference)."""
    for case in PIXEL_CASES:
        name, B, G, gh, gw, H, W, N, with_bg, seed = case
        soft = _soft(seed, B, G, gh, gw)
        g64, gap = sr.window_groups(soft, H, W, torch.float64)
        g32, _ = sr.window_groups(soft, H, W, torch.float32)
        print(f'"{name}": ({gap.numel()}, {int((gap < TIE).sum())}, {int((g64 != g32).sum())}),')
    for H, W, stride in [(224, 224, 224), (448, 448, 224), (300, 500, 224), (225, 224, 224), (300, 340, 112)]:
        wins, win = sr.window_list(2, H, W, "slide", (224, 224), (stride, stride))
        soft = _soft(H + W + stride, len(wins), 8, 14, 14)
        g64, gap = sr.window_groups(soft, 224, 224, torch.float64)
        g32, _ = sr.window_groups(soft, 224, 224, torch.float32)
        print(f"slide {H}x{W}/{stride}: {gap.numel()} window pixels, {int((gap < TIE).sum())} gaps below 1e-6, "
              f"{int((g64 != g32).sum())} fp32 differences")


if __name__ == "__main__":
    _reference_counts()
