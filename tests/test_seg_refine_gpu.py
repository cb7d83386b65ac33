"""GPU: the pixel-adaptive refinement - segclip_seg_refine (csrc/segment_refine.inc), ops.seg_refine, segmentation.PAMR /
refine_labels and refine= of predict_raw, update_raw and eval_epoch.

The yardstick is tests/pamr_reference.py, the definition restated in fp64 on the CPU.  On a constant picture every weight is a
power of two and every partial sum is exact in fp32, so the kernel must give fp64's planes and labels bit for bit.  Elsewhere
the final planes are held to fp64 within BOUND[case] = 4 x FLOORS[case] rounded up to one digit (kernel_frames' convention),
FLOORS[case] being max |m32 - m64| of the restatement itself run in fp32 on the CPU (measured once, recorded below: the bound
does not come from the kernel), and the labels must equal fp64's wherever fp64's top-two margin exceeds 2 x BOUND; at most 1 %
of a case's pixels may fall under that rule.  A kernel beyond its bound is a finding, not a reason to widen the bound.

All buffers the kernel writes are NaN / 0xAB-framed (tests/kernel_frames.py), the input labels too: nothing outside the outputs
is written and the inputs stay as they are.  The workgroup tile is 256 consecutive pixels of an image's flat (h, w) map."""
import ctypes
import functools

import pytest
import torch

import segclip_amd
from segclip_amd import _lib as L
from segclip_amd import ops
from segclip_amd.segmentation import PAMR, ImageTransform, SegEvaluator, SegInference, SegSweepEvaluator, TestAug, refine_labels
from segclip_amd.train import eval_epoch
from tests import kernel_frames as kf
from tests import pamr_reference as pr
from tests.helpers import CountedEncodeImage, load_golden, tiny_seg_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TF = ImageTransform()
MEAN, INV_STD = TF.mean, TF.inv_std
STD = tuple(1.0 / v for v in INV_STD)      # the kernel multiplies by exactly these fp32 numbers
ERR_INVALID, ERR_UNSUPPORTED = -1, -2

# name: sizes [(h, w)], classes, dilations, iterations, labels ("blocks": random 4-pixel blocks of all classes; a tuple: of these
# values), picture ("blocks": random 4-pixel colour blocks + noise of +-12; "random": independent bytes), options
CASES = {
    "1x1": dict(sizes=[(1, 1)], C=3, dil=(1, 2), T=3),
    "1x9": dict(sizes=[(1, 9)], C=3, dil=(1, 2), T=3),
    "7x1": dict(sizes=[(7, 1)], C=3, dil=(1, 2), T=3),
    "5x7_all_clamped": dict(sizes=[(5, 7)], C=4, dil=(8,), T=4),
    "33x47": dict(sizes=[(33, 47)], C=5, dil=(1, 2), T=3),
    "three_tiles": dict(sizes=[(5, 700)], C=5, dil=(1, 2), T=2),            # rows of 700 pixels: every row crosses three tiles
    "random_picture": dict(sizes=[(40, 56)], C=6, dil=(8, 16), T=10, picture="random"),
    "three_images": dict(sizes=[(5, 7), (9, 11), (13, 3)], C=4, dil=(1, 2), T=3),   # h w = 35, 99, 39
    "strided_bgr": dict(sizes=[(12, 10)], C=4, dil=(1, 3), T=3, pitch=17, reverse=True),
    "one_class": dict(sizes=[(6, 9)], C=1, dil=(1, 2), T=3),
    "256_classes": dict(sizes=[(10, 12)], C=256, dil=(1, 2), T=3, labels=(0, 7, 255)),
    "20_labels": dict(sizes=[(16, 18)], C=21, dil=(1, 2), T=4, labels=tuple(range(1, 21)), block=2),
    "six_dilations": dict(sizes=[(20, 24)], C=5, dil=(1, 2, 4, 8, 16, 32), T=2),
    "one_iteration": dict(sizes=[(12, 14)], C=5, dil=(1, 2), T=1),
    "32_iterations": dict(sizes=[(12, 14)], C=5, dil=(1, 2), T=32),
    "byte_beyond_C": dict(sizes=[(12, 14)], C=5, dil=(1, 2), T=3, labels=(0, 1, 2, 3, 4, 200)),
}
# max |m32 - m64| of tests/pamr_reference.py run in fp32 on the CPU, over the case's images (floors() below prints them)
FLOORS = {
    "1x1": 0.0,                   # every tap is the pixel itself: exact, the bound is 0
    "1x9": 3.58e-07,              # bound 2e-06
    "7x1": 7.61e-07,              # bound 4e-06
    "5x7_all_clamped": 5.56e-07,  # bound 3e-06
    "33x47": 7.16e-07,            # bound 3e-06
    "three_tiles": 7.47e-07,      # bound 3e-06
    "random_picture": 2.59e-06,   # bound 2e-05
    "three_images": 7.34e-07,     # bound 3e-06
    "strided_bgr": 5.03e-07,      # bound 3e-06
    "one_class": 3.58e-07,        # bound 2e-06
    "256_classes": 6.74e-07,      # bound 3e-06
    "20_labels": 6.56e-07,        # bound 3e-06
    "six_dilations": 6.46e-07,    # bound 3e-06
    "one_iteration": 2.72e-07,    # bound 2e-06
    "32_iterations": 3e-06,       # bound 2e-05
    "byte_beyond_C": 5.5e-07,     # bound 3e-06
}   # in every case no pixel's fp64 margin lies within 2 x bound: all labels are held to fp64


def bound(name):
    return kf.round_up_1(4 * FLOORS[name])


def _blocks(gen, h, w, block, draw):
    """an (h, w, ...) map that is constant on block x block squares"""
    small = draw(((h + block - 1) // block, (w + block - 1) // block))
    return small.repeat_interleave(block, 0).repeat_interleave(block, 1)[:h, :w]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> (raws [(h, w, 3) uint8 CPU], labels [(h, w) uint8 CPU]) of a case, seeded by its name"""
    c = CASES[name]
    gen = kf.seeded(name)
    values = torch.tensor(c.get("labels", tuple(range(c["C"]))), dtype=torch.uint8)
    raws, labels = [], []
    for (h, w) in c["sizes"]:
        if c.get("picture", "blocks") == "random":
            raw = torch.randint(0, 256, (h, w, 3), generator=gen)
        else:
            base = _blocks(gen, h, w, 4, lambda s: torch.randint(30, 226, s + (3,), generator=gen))
            raw = base + torch.randint(-12, 13, (h, w, 3), generator=gen)
        raws.append(raw.clamp(0, 255).to(torch.uint8).contiguous())
        idx = _blocks(gen, h, w, c.get("block", 4), lambda s: torch.randint(0, len(values), s, generator=gen))
        labels.append(values[idx].contiguous())
    return raws, labels


@functools.lru_cache(maxsize=None)
def ref64(name):
    """[(L64, m64)] per image of a case: computed once, shared, left unchanged"""
    c = CASES[name]
    raws, labels = make_case(name)
    return [pr.refine(r, l, c["C"], MEAN, STD, c["dil"], c["T"], reverse_channels=c.get("reverse", False)) for r, l in zip(raws, labels)]


def floors():
    """Prints the FLOORS table and, per case, the share of pixels whose fp64 margin is within 2 x the bound (CPU only)."""
    for name, c in CASES.items():
        raws, labels = make_case(name)
        floor, low, n = 0.0, 0, 0
        m32s = [pr.planes(r, l, c["C"], MEAN, STD, c["dil"], c["T"], c.get("reverse", False), dtype=torch.float32)
                for r, l in zip(raws, labels)]
        for (_, m64), m32 in zip(ref64(name), m32s):
            floor = max(floor, float((m32.double() - m64).abs().max()))
        b = kf.round_up_1(4 * floor)
        for _, m64 in ref64(name):
            low += int((pr.margin(m64) <= 2 * b).sum())
            n += m64.shape[1] * m64.shape[2]
        print(f'    "{name}": {floor:.3g},   # bound {b:.0e}, {low} of {n} pixels within 2 x bound')


class Run:
    """One call of ops.seg_refine on framed buffers: input labels, output labels and, for a single image, the planes."""

    def __init__(self, raws, labels, C, dil, T, reverse=False, pitch=None, probs=True, gts=None, areas=None, **kw):
        self.devraws = []
        for r in raws:
            h, w = r.shape[:2]
            if pitch:   # a view of a wider picture: the row stride is 3 * pitch bytes
                wide = torch.full((h, pitch, 3), 0xAB, dtype=torch.uint8, device=DEV)
                wide[:, :w] = r.to(DEV)
                self.devraws.append(wide[:, :w])
            else:
                self.devraws.append(r.to(DEV))
        self.sizes = [tuple(l.shape) for l in labels]
        self.offs, n = [], 0
        for (h, w) in self.sizes:
            self.offs.append(n)
            n += (h * w + 3) // 4 * 4
        self.fin, self.fout = kf.Frame((n,), torch.uint8), kf.Frame((n,), torch.uint8)
        self.fin.v.fill_(0xEE)   # padding bytes between images: never read as labels of an image
        for l, o in zip(labels, self.offs):
            self.fin.v[o:o + l.numel()] = l.reshape(-1).to(DEV)
        self.in_bits = self.fin.bits()
        h, w = self.sizes[0]
        self.fprobs = kf.Frame((C * h * w,), torch.float32) if probs and len(raws) == 1 else None
        self.table, self.n_blocks, self.side = ops.seg_refine_table(self.devraws, self.offs)
        self.gt = None if gts is None else torch.cat([g.reshape(-1) for g in gts]).to(DEV)
        self.call = lambda: ops.seg_refine(self.table, self.n_blocks, self.fin.v, C, dil, T, MEAN, INV_STD, reverse_channels=reverse,
                                           out=self.fout.v, gt=self.gt, areas=areas, max_side=self.side,
                                           probs=None if self.fprobs is None else self.fprobs.v, **kw)

    def run(self):
        self.call()
        torch.cuda.synchronize()
        self.check_frames()
        return self

    def check_frames(self):
        assert self.fout.intact() and (self.fprobs is None or (self.fprobs.intact() and self.fprobs.finite())), "wrote outside an output"
        assert torch.equal(self.in_bits, self.fin.bits()), "the input labels changed"
        for k, (o, (h, w)) in enumerate(zip(self.offs, self.sizes)):   # the padding between two images stays
            end = self.offs[k + 1] if k + 1 < len(self.offs) else self.fout.v.numel()
            assert bool((self.fout.v[o + h * w:end] == kf.IDX_FILL).all()), "wrote into the padding"

    def labels(self):
        return [self.fout.v[o:o + h * w].view(h, w).cpu() for o, (h, w) in zip(self.offs, self.sizes)]

    def planes(self, C):
        h, w = self.sizes[0]
        return self.fprobs.v.view(C, h, w).cpu()


def run_case(name, **kw):
    c = CASES[name]
    raws, labels = make_case(name)
    return Run(raws, labels, c["C"], c["dil"], c["T"], reverse=c.get("reverse", False), pitch=c.get("pitch"), **kw).run()


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("dil,T", [((1, 2), 5), ((1,), 8), ((4, 8), 5)])
def test_constant_picture_is_bit_equal_to_fp64(dil, T):
    raw = torch.full((24, 40, 3), 77, dtype=torch.uint8)
    labels = torch.randint(0, 5, (24, 40), generator=kf.seeded("exact")).to(torch.uint8)
    l64, m64 = pr.refine(raw, labels, 5, MEAN, STD, dil, T)
    l32, m32 = pr.refine(raw, labels, 5, MEAN, STD, dil, T, dtype=torch.float32)
    assert torch.equal(m32.double(), m64) and torch.equal(l32, l64), "the case is not exact in fp32"
    r = Run([raw], [labels], 5, dil, T).run()
    assert torch.equal(r.planes(5).double(), m64), "planes differ from fp64"
    assert torch.equal(r.labels()[0], l64), "labels differ from fp64"
    assert not torch.equal(l64, labels), "the refinement changed nothing"


# ------------------------------------------------------------------------------------------------ 2. against fp64
def _judge_labels(name, got, l64, m64):
    b = bound(name)
    firm = pr.margin(m64) > 2 * b
    share = 1.0 - float(firm.double().mean())
    wrong = int((got != l64)[firm].sum())
    print(f"{name}: {wrong} firm labels differ; {share:.4%} of the pixels within 2 x bound")
    assert wrong == 0, f"{name}: {wrong} labels differ from fp64 where its margin exceeds {2 * b:g}"
    assert share <= 0.01, f"{name}: {share:.2%} of the pixels are left out by the margin rule"


@pytest.mark.parametrize("name", list(CASES))
def test_against_fp64(name):
    c = CASES[name]
    r = run_case(name)
    refs = ref64(name)
    if len(refs) == 1:
        l64, m64 = refs[0]
        err = float((r.planes(c["C"]).double() - m64).abs().max())
        print(f"{name}: kernel error {err:.3g}, floor {FLOORS[name]:.3g}, bound {bound(name):.0e}")
        assert err <= bound(name), f"{name}: max |m - m64| = {err:.3g} exceeds the bound {bound(name):g}"
        _judge_labels(name, r.labels()[0], l64, m64)
    else:
        raws, labels = make_case(name)
        for k, ((l64, m64), got) in enumerate(zip(refs, r.labels())):
            one = Run([raws[k]], [labels[k]], c["C"], c["dil"], c["T"]).run()
            err = float((one.planes(c["C"]).double() - m64).abs().max())
            print(f"{name}[{k}]: kernel error {err:.3g}, floor {FLOORS[name]:.3g}, bound {bound(name):.0e}")
            assert err <= bound(name), f"{name}[{k}]: max |m - m64| = {err:.3g} exceeds the bound {bound(name):g}"
            assert torch.equal(got, one.labels()[0]), f"{name}: image {k} differs between the list call and a call of its own"
            _judge_labels(name, got, l64, m64)


def test_labels_beyond_C_and_absent_planes():
    """a byte >= C belongs to no plane: its plane does not exist, and a pixel all of whose taps see such bytes keeps its byte"""
    raw = torch.full((9, 9, 3), 50, dtype=torch.uint8)
    labels = torch.full((9, 9), 200, dtype=torch.uint8)
    labels[:, 6:] = 2
    r = Run([raw], [labels], 5, (1,), 2).run()
    l64, m64 = pr.refine(raw, labels, 5, MEAN, STD, (1,), 2)
    assert torch.equal(r.planes(5).double(), m64) and torch.equal(r.labels()[0], l64)
    assert bool((l64[:, :4] == 200).all()) and bool((l64[:, 4:] == 2).all())
    # T = 0: the labels as they are, the one-hot planes
    r = Run([raw], [labels], 5, (1,), 0).run()
    assert torch.equal(r.labels()[0], labels) and torch.equal(r.planes(5).double(), pr.one_hot(labels, 5))


# ------------------------------------------------------------------------------------------------ 3. the snapping scene
def test_refinement_snaps_a_displaced_border():
    raw, labels, gt = pr.snapping_scene()
    before = pr.miou(labels, gt, 3)
    out = Run([raw], [labels], 3, (8, 16), 10, probs=False).run().labels()[0]
    after = pr.miou(out, gt, 3)
    print(f"snapping through the kernel: mIoU {before:.4f} -> {after:.4f}")
    assert after - before > 0.05


# ------------------------------------------------------------------------------------------------ 4. two calls, the same bits
@pytest.mark.parametrize("name", ["three_images", "random_picture", "20_labels"])
def test_two_calls_give_identical_bits(name):
    c = CASES[name]
    raws, labels = make_case(name)
    r = Run(raws, labels, c["C"], c["dil"], c["T"]).run()
    frames = [r.fout] + ([] if r.fprobs is None else [r.fprobs])
    snap = [f.bits() for f in frames]
    for f in frames:
        f.buf.fill_(f.fill)
    r.run()
    assert all(torch.equal(a, f.bits()) for a, f in zip(snap, frames)), f"{name}: the second call differs"


def test_the_call_does_not_synchronise():
    """ops.seg_refine with a ground truth and 256 classes (32 chunks of launches) under torch's synchronisation check: the
    wrapper allocates and enqueues only (the C entry holds no synchronising HIP call: memsets and launches on the stream)"""
    c = CASES["256_classes"]
    raws, labels = make_case("256_classes")
    gts = [torch.zeros_like(l) for l in labels]
    areas = torch.zeros(3, c["C"], dtype=torch.int64, device=DEV)
    r = Run(raws, labels, c["C"], c["dil"], c["T"], gts=gts, areas=areas, probs=False).run()   # the library is loaded
    want = r.fout.bits()
    r.fout.buf.fill_(r.fout.fill)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r.call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(want, r.fout.bits())


# ------------------------------------------------------------------------------------------------ 5. workspace
def test_workspace_does_not_depend_on_the_class_count():
    """the C ABI itself, with a framed workspace of exactly ws_bytes: enough for 2 classes and for 256"""
    lib = L.load()
    raws, labels = make_case("256_classes")
    outs = []
    for C in (2, 256):
        r = Run(raws, labels, C, (1, 2), 3, probs=False)
        n = r.fin.v.numel()
        ws_bytes = lib.segclip_seg_refine_ws_bytes(n, 1, 2)
        assert ws_bytes > 0 and ws_bytes == lib.segclip_seg_refine_ws_bytes(n, 1, 2)
        ws = kf.Frame((ws_bytes,), torch.uint8)
        f3 = L.f32 * 3
        rc = lib.segclip_seg_refine(L.ptr(r.table), 1, r.n_blocks, r.side, r.fin.p, n, C, (ctypes.c_int32 * 2)(1, 2), 2, 3, f3(*MEAN),
                                    f3(*INV_STD), 0, r.fout.p, n, None, 0, 255, 0, None, None, 0, ws.p, ws_bytes, L.stream())
        torch.cuda.synchronize()
        assert rc == 0 and ws.intact()
        r.check_frames()
        outs.append(r.labels()[0])
    _judge_labels("256_classes", outs[1], *ref64("256_classes")[0])
    # with C = 2 the bytes 7 and 255 carry no plane: label 0 spreads, and nothing else is ever written
    assert bool((outs[0][labels[0] == 0] == 0).all()) and set(outs[0].unique().tolist()) <= {0, 7, 255}


# ------------------------------------------------------------------------------------------------ 6. areas
@pytest.mark.parametrize("reduce_zero", [False, True])
def test_areas_of_the_refined_labels(reduce_zero):
    c = CASES["three_images"]
    raws, labels = make_case("three_images")
    gen = kf.seeded("areas")
    gts = [torch.randint(0, c["C"] + 1, l.shape, generator=gen).to(torch.uint8) for l in labels]
    for g in gts:
        g[1:3] = 255   # ignore pixels
    fa = kf.Frame((3, c["C"]), torch.int64)
    fa.v.zero_()
    want = torch.zeros(3, c["C"], dtype=torch.int64, device=DEV)
    for _ in range(2):   # accumulated across two calls
        r = Run(raws, labels, c["C"], c["dil"], c["T"], gts=gts, areas=fa.v, reduce_zero_label=reduce_zero).run()
        for got, g in zip(r.labels(), gts):
            ops.seg_areas(got.to(DEV), g.to(DEV), c["C"], reduce_zero_label=reduce_zero, areas=want)
    torch.cuda.synchronize()
    assert fa.intact() and torch.equal(fa.v, want) and int(want.sum()) > 0
    # T = 0 scores the input labels
    fa.v.zero_()
    Run(raws, labels, c["C"], c["dil"], 0, gts=gts, areas=fa.v, reduce_zero_label=reduce_zero).run()
    want0 = torch.zeros_like(want)
    for l, g in zip(labels, gts):
        ops.seg_areas(l.to(DEV), g.to(DEV), c["C"], reduce_zero_label=reduce_zero, areas=want0)
    assert torch.equal(fa.v, want0)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_outputs_untouched():
    lib = L.load()
    raws, labels = make_case("33x47")
    r = Run(raws, labels, 5, (1, 2), 3)
    n = r.fin.v.numel()
    ws_bytes = lib.segclip_seg_refine_ws_bytes(n, 1, 6)
    ws = kf.Frame((ws_bytes,), torch.uint8)
    f3 = L.f32 * 3

    def call(C=5, dil=(1, 2), T=3, side=None, ws_n=ws_bytes, out=None, out_n=n):
        arr = (ctypes.c_int32 * max(len(dil), 1))(*dil)
        rc = lib.segclip_seg_refine(L.ptr(r.table), 1, r.n_blocks, r.side if side is None else side, r.fin.p, n, C, arr, len(dil), T,
                                    f3(*MEAN), f3(*INV_STD), 0, r.fout.p if out is None else out, out_n, None, 0, 255, 0, None,
                                    r.fprobs.p, r.fprobs.v.numel(), ws.p, ws_n, L.stream())
        torch.cuda.synchronize()
        return rc

    refused = [dict(dil=()), dict(dil=(1, 2, 3, 4, 5, 6, 7)), dict(dil=(0, 2)), dict(dil=(1, 33)), dict(dil=(2, 2)), dict(dil=(4, 2)),
               dict(T=-1), dict(T=33), dict(C=0), dict(C=257), dict(side=1 << 15), dict(side=0), dict(ws_n=ws_bytes // 4)]
    for kw in refused:
        assert call(**kw) == ERR_UNSUPPORTED, kw
        assert lib.segclip_last_error_string().decode().startswith("seg_refine"), kw
        assert r.fout.untouched() and r.fprobs.untouched() and ws.untouched(), kw
    # out of place only: the input labels as output, or an output that begins inside them
    for kw in (dict(out=r.fin.p), dict(out=ctypes.c_void_p(r.fin.v.data_ptr() + 8)), dict(out_n=n - 4)):
        assert call(**kw) == ERR_INVALID, kw
        assert r.fout.untouched() and r.fprobs.untouched() and ws.untouched(), kw
    assert torch.equal(r.in_bits, r.fin.bits())
    assert lib.segclip_seg_refine_ws_bytes(n, 1, 0) == ERR_UNSUPPORTED and lib.segclip_seg_refine_ws_bytes(n, 1, 7) == ERR_UNSUPPORTED
    # a row the device refuses is skipped: its bytes stay
    bad = r.table.clone()
    bad[0, 4] = n - 10   # the label offset runs past the buffer
    ops.seg_refine(bad, r.n_blocks, r.fin.v, 5, (1, 2), 3, MEAN, INV_STD, out=r.fout.v)
    torch.cuda.synchronize()
    assert r.fout.untouched()
    # the wrapper
    with pytest.raises(L.Unsupported, match="dilations"):
        ops.seg_refine(r.table, r.n_blocks, r.fin.v, 5, (2, 1), 3, MEAN, INV_STD, out=r.fout.v)
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.seg_refine(r.table, r.n_blocks, r.fin.v, 5, (1, 2), 3, MEAN, INV_STD, out=r.fin.v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_refine(r.table, r.n_blocks, r.fin.v.cpu(), 5, (1, 2), 3, MEAN, INV_STD)
    assert r.fout.untouched()
    # and the accepted call on the same frames
    assert call() == 0
    r.check_frames()
    assert not r.fout.untouched()


# ------------------------------------------------------------------------------------------------ 8. end to end
SLIDE = dict(mode="slide", crop_size=(128, 128), stride=(96, 96))
RAW_SIZES = [(90, 120), (130, 101), (75, 75)]
NETS = [(128, 128), (64, 64), (128, 128)]


def _raws(seed):
    g = torch.Generator().manual_seed(seed)
    raws = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for (h, w) in RAW_SIZES]
    gts = [torch.randint(0, 14, (h, w), generator=g).to(torch.uint8).to(DEV) for (h, w) in RAW_SIZES]
    for t in gts:
        t[5:9] = 255
    return raws, gts


@pytest.mark.parametrize("mode", ["slide", "whole", "slide_aug"])
def test_end_to_end(mode):
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        raws, gts = _raws(11)
        kw = {} if mode == "whole" else dict(SLIDE)
        nets = NETS if mode == "whole" else None
        aug = TestAug(flip=True) if mode == "slide_aug" else None
        pamr = PAMR(iters=3, dilations=(1, 2))
        seg = SegInference(model, emb, True, bg_thresh=0.02, **kw)
        with CountedEncodeImage(model) as calls:
            plain = seg.predict_raw(raws, TF, net_sizes=nets, aug=aug)
            plain_calls = list(calls)
        keep = [p.clone() for p in plain]
        want = refine_labels(raws, plain, seg.num_classes, TF, pamr)
        assert all(torch.equal(a, b) for a, b in zip(plain, keep)), "refine_labels changed its input"
        with CountedEncodeImage(model) as calls:
            got = seg.predict_raw(raws, TF, net_sizes=nets, aug=aug, refine=pamr, out_shapes=RAW_SIZES)
            assert list(calls) == plain_calls, "the refinement changes the tower calls"
        assert [tuple(t.shape) for t in got] == RAW_SIZES and all(t.dtype == torch.uint8 for t in got)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), f"{mode}: predict_raw(refine=) differs from refine_labels(predict_raw())"
        # the host-side restatement on this build's own label maps
        for r, p, w in zip(raws, plain, want):
            l64, m64 = pr.refine(r.cpu(), p.cpu(), seg.num_classes, MEAN, STD, pamr.dilations, pamr.iters)
            firm = pr.margin(m64) > 1e-4
            assert torch.equal(w.cpu()[firm], l64[firm])
        # the evaluator: the areas of the refined maps, once
        ev = SegEvaluator(seg, reduce_zero_label=True)
        with CountedEncodeImage(model) as calls:
            maps = ev.update_raw(raws, gts, TF, return_labels=True, net_sizes=nets, aug=aug, refine=pamr)
            assert list(calls) == plain_calls
        assert all(torch.equal(a, b) for a, b in zip(maps, want))
        areas = torch.zeros_like(ev.areas)
        for w, t in zip(want, gts):
            ops.seg_areas(w, t, seg.num_classes, reduce_zero_label=True, areas=areas)
        assert torch.equal(ev.areas, areas) and int(areas.sum()) > 0
        assert ev.update_raw(raws, gts, TF, net_sizes=nets, aug=aug, refine=pamr) is None
        assert torch.equal(ev.areas, 2 * areas)
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


def test_eval_epoch_and_interface_errors():
    g = load_golden("seg_tiny.npz")
    try:
        model = tiny_seg_model()
        tokens = torch.from_numpy(g["prompt_ids"])
        emb = torch.from_numpy(g["text_embedding"]).to(DEV)
        pamr = PAMR(iters=2, dilations=(1, 2))
        batches = []
        for k in range(2):
            raws, gts = _raws(40 + k)
            batches.append(([t.cpu() for t in raws[:2 + k]], [t.cpu() for t in gts[:2 + k]]))
        cfg = dict(bg_thresh=0.02, reduce_zero_label=True, **SLIDE)
        got = eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(refine=pamr, **cfg), transform=TF)
        seg = SegInference(model, emb, True, bg_thresh=0.02, **SLIDE)
        areas = torch.zeros(3, seg.num_classes, dtype=torch.int64, device=DEV)
        for raws, gts in batches:
            raws, gts = [t.to(DEV) for t in raws], [t.to(DEV) for t in gts]
            for w, t in zip(refine_labels(raws, seg.predict_raw(raws, TF), seg.num_classes, TF, pamr), gts):
                ops.seg_areas(w, t, seg.num_classes, reduce_zero_label=True, areas=areas)
        assert got == SegEvaluator.metrics_from_areas(areas.cpu())["mIoU"] * 100.0
        assert 0.0 <= got <= 100.0
        with pytest.raises(ValueError, match="refine.*transform"):
            eval_epoch(None, model, DEV, 1, batches, tokens, True, dict(refine=pamr, **cfg))

        raws, gts = _raws(50)
        ev = SegEvaluator(seg)
        with pytest.raises(ValueError, match="out_shapes"):
            seg.predict_raw(raws, TF, out_shapes=[(h + 1, w) for (h, w) in RAW_SIZES], refine=pamr)
        with pytest.raises(ValueError, match="out_shapes"):
            ev.update_raw(raws, [t[:-1] for t in gts], TF, refine=pamr)
        with pytest.raises(TypeError, match="PAMR"):
            seg.predict_raw(raws, TF, refine=(8, 16))
        pre = [torch.zeros(3, 128, 128, device=DEV)]
        with pytest.raises(ValueError, match="predict_list.*refine"):
            seg.predict_list(pre, refine=pamr)
        with pytest.raises(ValueError, match="update.*refine"):
            ev.update(pre, [gts[0]], refine=pamr)
        with pytest.raises(ValueError, match="render_raw.*refine"):
            seg.render_raw(raws, TF, ["pred"], torch.zeros(14, 3, dtype=torch.uint8), refine=pamr)
        with pytest.raises(ValueError, match="SegSweepEvaluator.*refine"):
            SegSweepEvaluator(seg, [0.1, 0.5]).update_raw(raws, gts, TF, refine=pamr)
        with pytest.raises(ValueError, match="label map"):
            refine_labels(raws, [t[:-1] for t in gts], seg.num_classes, TF, pamr)
        assert int(ev.areas.sum()) == 0
        for bad, match in ((dict(iters=-1), "iters"), (dict(iters=33), "iters"), (dict(iters=2.0), "iters"), (dict(dilations=()), "dilations"),
                           (dict(dilations=(1, 2, 3, 4, 5, 6, 7)), "dilations"), (dict(dilations=(0, 1)), "dilations"),
                           (dict(dilations=(1, 33)), "dilations"), (dict(dilations=(2, 2)), "dilations.*increasing"),
                           (dict(dilations=(1.5,)), "dilations"), (dict(dilations=4), "dilations")):
            with pytest.raises(ValueError, match=match):
                PAMR(**bad)
        assert (PAMR().iters, PAMR().dilations) == (10, (8, 16))
    finally:
        segclip_amd.set_compute_dtype(torch.float32)


if __name__ == "__main__":
    floors()
