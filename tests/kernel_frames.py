"""The machinery shared by the GPU test files that call one kernel at a time through the C ABI (tests/test_center_stage_gpu.py,
tests/test_loss_head_gpu.py, tests/test_frontend_glue_gpu.py): NaN-framed buffers, seeded host-side inputs, the call-twice
harness, and the value check with its floor-measuring mode.  Importing this module needs torch only; a frame allocates on the device."""
import math

import torch

from segclip_amd import _lib as L
from tests.helpers import _beyond, check, within

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64
IDX_FILL = 0xAB
IDX_FILL_WIDE = -0x5454545454545455   # 0xAB in every byte of an int64: for index outputs that may hold 171 themselves


def round_up_1(x):
    """x rounded up to one significant digit"""
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def units(got, ref):
    """the largest error in check() units, |err| / (|ref| + rms(ref))"""
    _, err, rms = _beyond(got, ref, 0.0)
    return float((err / (ref.double().abs() + rms)).max())


class Bounds:
    """FLOORS of one test file -> its bounds (rt: 4 x floor rounded up to one digit) and its value checks.  `stats` is None while
    the rows assert; a dict there (the file's floors() sets it) switches judge() from asserting to recording floors and errors."""

    def __init__(self, floors):
        self.rt = {k: round_up_1(4 * f) for k, f in floors.items()}
        self.stats = None

    def judge(self, key, what, got, ref, ref32=None, rtol=None):
        """the value check of a row; under floors() it records the floor and the kernel's error instead"""
        if self.stats is None:
            check(got, ref, self.rt[key] if rtol is None else rtol, what)
            return
        s = self.stats.setdefault(key, {"floor": 0.0, "kernel": 0.0, "floor_row": "", "kernel_row": ""})
        if ref32 is not None:
            f = units(ref32, ref)
            if f > s["floor"]:
                s["floor"], s["floor_row"] = f, what
        e = units(got, ref)
        if e > s["kernel"]:
            s["kernel"], s["kernel_row"] = e, what

    def rejects(self, key, what, got, wrong, rtol=None):
        assert within(got, wrong, self.rt[key] if rtol is None else rtol) is False, f"{what}: the bound accepts the defect"


class Frame:
    """a view of `shape` (rows of shape[-1] elements, `pitch` apart) inside a flat buffer filled with NaN (0xAB for integers):
    GUARD words before, two guard rows and GUARD words after.  `shift` moves the view that many elements further into the
    buffer (a view that is not 16-byte aligned); `fill` replaces the guard value of an integer frame."""

    def __init__(self, shape, dtype, pitch=None, shift=0, fill=None):
        shape = tuple(shape)
        W = shape[-1]
        pitch = pitch or W
        rows = math.prod(shape[:-1])
        self.fill = float("nan") if dtype.is_floating_point else (IDX_FILL if fill is None else fill)
        self.buf = torch.full((GUARD + shift + (rows + 2) * pitch + GUARD,), self.fill, dtype=dtype, device=DEV)
        st = [1] if len(shape) == 1 else [pitch, 1]
        for d in reversed(shape[1:-1]):
            st.insert(0, st[0] * d)
        self.v = self.buf.as_strided(shape, st, GUARD + shift)
        self.inside = torch.zeros_like(self.buf, dtype=torch.bool)
        self.inside.as_strided(shape, st, GUARD + shift).fill_(True)

    def intact(self):
        out = self.buf[~self.inside]
        return bool(out.isnan().all()) if self.buf.dtype.is_floating_point else bool((out == self.fill).all())

    def finite(self):
        return bool(self.v.isfinite().all()) if self.buf.dtype.is_floating_point else bool((self.v != self.fill).all())

    def untouched(self):
        """nothing written at all, inside or outside the view"""
        return bool(self.buf.isnan().all()) if self.buf.dtype.is_floating_point else bool((self.buf == self.fill).all())

    def bits(self):
        return self.buf.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.buf.element_size()]).clone()

    @property
    def p(self):
        return L.ptr(self.v)


def put(t, pitch=None, shift=0):
    """the input t inside a frame of its own"""
    f = Frame(t.shape, t.dtype, pitch, shift)
    f.v.copy_(t)
    return f


def draw(gen, *shape, dtype=F32, scale=1.0):
    return (torch.randn(*shape, generator=gen, dtype=F64) * scale).to(dtype).to(DEV)


def seeded(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(name)))


def run_twice(name, call, outs, finite=True):
    """the call, its frames checked, and the same call again: bit-identical, frames included.  finite=False for outputs that
    hold inf or NaN on purpose (the caller then shows by other means that every element was written)"""
    for f in outs:
        f.buf.fill_(f.fill)
    call()
    torch.cuda.synchronize()
    snap = [f.bits() for f in outs]
    call()
    torch.cuda.synchronize()
    assert all(torch.equal(a, f.bits()) for a, f in zip(snap, outs)), f"{name}: the second call differs"
    for i, f in enumerate(outs):
        assert f.intact(), f"{name}: output {i} written outside its view"
        assert not finite or f.finite(), f"{name}: output {i} not written everywhere / not finite"


def lib_call(fn_name, *args):
    L.check(getattr(L.load(), fn_name)(*args, L.stream()), fn_name)
