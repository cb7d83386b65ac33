"""GPU: every kernel instance segclip_attn_fwd / segclip_attn_bwd can launch, each reached by a row of CASES that names the
forward and the backward route it must take (ops.attn_last_route), checked against softmax attention in fp64 on the exact
values the kernel reads.

Per row: (1) the route after the forward and after the backward; (2) O, the statistics (bf16: natural-log log-sum-exp
[B][H][Tq]; fp32: the probability matrix), dQ, dK, dV and the token sums (colsum_part) against fp64 with the bound of
tests/helpers.check; (3) the bf16 emulation of the same row (below) sits within half the bound, so a row whose inputs push
the rounding floor up fails loudly; (4) the same bound rejects the fp64 reference with (a) the last valid key of every row
removed, (b) one row inside the last 32-row tile replaced by its neighbour, (c) on masked rows the mask moved by one key
(klen + 1, causal including key q + 1) - for O and for every gradient; (5) every output lives in a NaN frame (rows above, a
pitch wider than H * hd, a gap between the samples, rows below; guard words around the statistics and the token sums) that
must survive while everything inside becomes finite, the inputs carry NaN in their pitch and in the rows beyond Tq / Tk, K
and V carry 1e30 at the keys klen masks, and the backward workspace is NaN before the call; (6) the same forward and
backward a second time into the same frames is bit-identical, frames included.
All calls go through ops._attn_desc / p_attn_fwd / p_attn_bwd with explicit strides.

Instances and the rows that reach them (the forward instance of a row is independent of its backward instance):
  fwd smallq: x8_204, x8_448, x8_196_t18
  fwd pf 3 / 6 / 7 tiles: s65 s96 | s161 s192 | s193 s200 many_pf7;  causal: s77_causal | s170_causal | s200_causal
  fwd generic, one tile group, rows stored from registers (Tq <= 128): s64 s97 s128, the cross rows with Tq <= 128
  fwd generic, one tile group, rows staged through LDS (129-256 queries): s129 s160 s201 s222 s223 s224 s225 s256
  fwd generic, several tile groups (more than 256 queries, always staged): s257 .. s784, x300_40
    (several tile groups with unstaged rows is a form the kernel has and no call reaches: plan_fwd stages above 128 queries)
  fwd f32: f32_s197 f32_s77_causal f32_s40_klen f32_x40_100
  bwd smallq: as forward;  bwd dqw single: s193 s200 s201 s222 many_pf7;  bwd dqw multi: s257 s288 s449 s576 s577 s784 many_dqwm
  bwd stream pair: s319 s448 s300_causal x8_449 x8_584 x300_40;  bwd spl: s129 s160 s161 s192 many_spl many_pf6
  bwd sp<false>: s64 s65 s96 s97 s128 s223 s224 s225 s256 many_sp8 and the hd 8 / 32 / 48 rows;  bwd sp<true>: causal s77_causal, klen s77_klen_mae, both s77_both
  bwd two-pass: x40_100 x100_40 x9_204 x33_256_causal x9_204_t18 x40_100_klen;  bwd f32: as forward

Reference, emulation and bounds.  attention() below is the reference (fp64) and, with emulate=True, the same arithmetic with
the three roundings every bf16 kernel here makes: P to bf16 before P V and dV = P^T dO, dS to bf16 before dQ and dK, outputs to
bf16 (and D = rowsum(dO * O) from the stored O).  It leaves out the fp32 accumulation order and the hardware exp2 / log; the
factor of 2 between the emulated floor and the bound is for those.  Floors measured with this file's rows and inputs
(N(0, 1), drawn on the host so that they are the same on every device): the largest error in check() units,
|err| / (|ref| + rms(ref)), over the rows of a class.  The floor is a maximum over the elements of a tensor and the rms is
one number per tensor, so it grows with the number of (sample, head) items, and a masked row (causal / klen: few keys, peaked
P, large dS entries) rounds worse than a full one; hence four classes of rows.  Bound = 2 x floor rounded up to one digit:
                                  O floor -> bound      dQ, dK, dV floor -> bound
    no mask, at most 64 items     9.1e-3  -> 2e-2       1.83e-2 -> 4e-2
    masked,  at most 64 items     1.05e-2 -> 3e-2       3.80e-2 -> 8e-2
    no mask, more than 512 items  1.66e-2 -> 4e-2       4.34e-2 -> 9e-2
    masked,  more than 512 items  1.25e-2 -> 3e-2       5.65e-2 -> 1.2e-1
    token sums of dQ (all rows)   9.5e-3  -> 2e-2   (every kernel sums its fp32 dS column sums times K, never the stored dQ;
                                                     the token sums of dV are the fp32 token sums of dO: 1e-5; of dK: exactly 0)
    log-sum-exp                   fp32: 1e-5
    fp32 dtype                    torch float32 against fp64 of the same rows: 2.1e-6; 4 x that is below 1e-5, which stays
The defects of (4), measured against the emulation, sit at 0.12 (one of 584 keys removed from 8 queries) to 6 in the same units.

Contract decisions written into include/segclip_hip.h with this file:
  - klen in the forward works at any length (s288_klen_fwd asserts the values); only the bf16 backward is limited to 256
    tokens and refuses longer ones (the same row asserts the refusal and that nothing was written).
  - a masked key is loaded and multiplied by a probability of exactly 0, as the reference does with exp(-1e6): K and V must be
    finite there.  The rows therefore put 1e30 (not NaN) at masked keys; NaN stays in every place that must never be used.
  - causal with Tq != Tk is defined by all kernels as key <= query index; x33_256_causal asserts it.
  - klen[b] == 0 is outside the contract and not tested.
"""
import ctypes
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from segclip_amd import ops  # noqa: E402
from tests.helpers import _beyond, check, within  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
ABOVE, GAP, BELOW = 3, 2, 33    # sentinel rows above the first sample, after every sample, below the last one
GUARD = 64                      # sentinel words around the statistics and the token sums
MASKED_KV = 1e30                # K, V at keys >= klen[b]: finite (see the module docstring)

# bounds derived from the measured floors (module docstring): (masked, more than 512 items) -> (O, gradients)
RT_BF = {(False, False): (2e-2, 4e-2), (True, False): (3e-2, 8e-2), (False, True): (4e-2, 9e-2), (True, True): (3e-2, 1.2e-1)}
RT_CS = 2e-2
RT_LSE, RT_CS_DV = 1e-5, 1e-5
RT_F32 = 1e-5


# ---- routes ------------------------------------------------------------------------------------------------------------
def gen(tiles, waves, staged):
    return ("generic", tiles, int(staged) | waves << 8)


def pf(nt, causal=False):
    return ("pf", nt, int(causal))


def sp(tiles, masked=False):
    return ("sp", tiles, int(masked))


def dqw(multi):
    return ("dqw", 7, int(multi))


def spl(tiles):
    return ("spl", tiles, 0)


def stream(tiles):
    return ("stream", tiles, 0)


def two(tiles, waves):
    return ("twopass", tiles, waves << 8)


def f32r(tiles):
    return ("f32", tiles, 0)


SMALLQ = ("smallq", 1, 0)
REFUSED = (None, 0, 0)


@dataclasses.dataclass
class Case:
    name: str
    B: int
    H: int
    Tq: int
    Tk: int
    hd: int
    fwd: tuple
    bwd: tuple                  # REFUSED: the backward must refuse the row and write nothing
    causal: bool = False
    klen: tuple = None          # valid keys per sample
    lay: str = "packed"         # "packed": Q|K|V and dQ|dK|dV share a row; "sep": eight tensors, eight pitches;
    dtype: torch.dtype = BF     # "t18": K|V token-major (k_sb = pitch, k_st = B * pitch), the rest as "sep"


def S(name, T, fwd, bwd, B=2, H=2, hd=64, **kw):
    return Case(name, B, H, T, T, hd, fwd, bwd, **kw)


def X(name, Tq, Tk, fwd, bwd, B=2, H=2, hd=64, lay="sep", **kw):
    return Case(name, B, H, Tq, Tk, hd, fwd, bwd, lay=lay, **kw)


KL5 = lambda T: (1, 32, 33, T - 1, T)   # noqa: E731  one, a multiple of 32, a multiple of 32 plus 1, T - 1, T
CASES = [
    # -- dispatcher edges of the self-attention forward (pf at 3, 6, 7 tiles) and backward (sp | spl | dqw | sp | long)
    S("s64", 64, gen(2, 2, 0), sp(2)),
    S("s65", 65, pf(3), sp(3)),
    S("s96", 96, pf(3), sp(3)),
    S("s97", 97, gen(4, 4, 0), sp(4)),
    S("s128", 128, gen(4, 4, 0), sp(4)),
    S("s129", 129, gen(5, 5, 1), spl(5)),
    S("s160", 160, gen(5, 5, 1), spl(5)),
    S("s161", 161, pf(6), spl(6)),
    S("s192", 192, pf(6), spl(6)),
    S("s193", 193, pf(7), dqw(0)),
    # (the persistent forward's LDS holds 7 tiles up to 200 tokens, the loader-wave backward's up to 216: 201-224 tokens
    #  run the generic forward, and 223 / 224, which the dQ-wave kernel leaves, the plain single-pass backward)
    S("s200", 200, pf(7), dqw(0)),
    S("s201", 201, gen(7, 7, 1), dqw(0)),
    S("s222", 222, gen(7, 7, 1), dqw(0)),
    S("s223", 223, gen(7, 7, 1), sp(7)),
    S("s224", 224, gen(7, 7, 1), sp(7)),
    S("s225", 225, gen(8, 8, 1), sp(8)),
    S("s256", 256, gen(8, 8, 1), sp(8)),
    S("s257", 257, gen(9, 5, 1), dqw(1)),
    # -- long: T % 32 == 0, T % 32 == 31 (no room for the two token-sum rows), T % 224 == 0, one past it, ViT-L and 28 x 28
    S("s288", 288, gen(9, 5, 1), dqw(1)),
    S("s319", 319, gen(10, 5, 1), stream(10)),
    S("s448", 448, gen(14, 7, 1), stream(14)),
    S("s449", 449, gen(15, 8, 1), dqw(1)),
    S("s576", 576, gen(18, 6, 1), dqw(1), B=1),
    S("s577", 577, gen(19, 7, 1), dqw(1), B=1),
    S("s784", 784, gen(25, 7, 1), dqw(1), B=1),
    # -- masks.  klen runs inside pf / the generic forward and selects sp<true>; causal the text tower's instances
    S("s77_klen_mae", 77, pf(3), sp(3, 1), B=5, H=8, hd=48, klen=KL5(77)),
    S("s77_causal", 77, pf(3, 1), sp(3, 1), causal=True),
    S("s77_both", 77, pf(3, 1), sp(3, 1), B=5, causal=True, klen=KL5(77)),
    S("s196_klen", 196, pf(7), sp(7, 1), B=5, klen=KL5(196)),
    S("s40_klen", 40, gen(2, 2, 0), sp(2, 1), B=5, klen=KL5(40)),
    S("s256_klen", 256, gen(8, 8, 1), sp(8, 1), B=5, klen=KL5(256)),
    S("s170_causal", 170, pf(6, 1), sp(6, 1), causal=True),
    S("s200_causal", 200, pf(7, 1), sp(7, 1), causal=True),
    S("s256_causal", 256, gen(8, 8, 1), sp(8, 1), causal=True),
    S("s300_causal", 300, gen(10, 5, 1), stream(10), causal=True),
    S("s288_klen_fwd", 288, gen(9, 5, 1), REFUSED, B=5, klen=KL5(288)),
    # -- head sizes 8, 32, 48 (64 above) on the generic forward and sp; spl takes head size 64 only (these rows found
    #    non-finite gradients there: its loader copies whole 128-byte rows of Q, and the columns beyond the head were NaN)
    S("s100_hd8", 100, gen(4, 4, 0), sp(4), hd=8),
    S("s120_hd32", 120, gen(4, 4, 0), sp(4), hd=32),
    S("s40_hd48", 40, gen(2, 2, 0), sp(2), hd=48),
    S("s150_hd8", 150, gen(5, 5, 1), sp(5), hd=8),
    S("s150_hd32", 150, gen(5, 5, 1), sp(5), hd=32),
    S("s130_hd48", 130, gen(5, 5, 1), sp(5), hd=48),
    S("s200_hd48", 200, pf(7), sp(7), hd=48),
    S("s216_hd48", 216, gen(7, 7, 1), sp(7), hd=48),
    S("s217_hd48", 217, gen(7, 7, 1), sp(7), hd=48),
    # -- cross-attention: the at-most-8-queries kernel and its bounds (8 | 9 queries, 448 | 449 keys of LDS)
    X("x8_204", 8, 204, SMALLQ, SMALLQ, B=3, H=4),
    X("x8_448", 8, 448, SMALLQ, SMALLQ),
    X("x8_196_t18", 8, 196, SMALLQ, SMALLQ, B=3, H=4, lay="t18"),
    X("x9_204", 9, 204, gen(1, 1, 0), two(7, 4)),
    X("x8_449", 8, 449, gen(1, 1, 0), stream(15)),
    X("x8_584", 8, 584, gen(1, 1, 0), stream(19)),
    # -- cross-attention on the generic forward and the two-pass backward
    X("x40_100", 40, 100, gen(2, 2, 0), two(4, 4)),
    X("x100_40", 100, 40, gen(4, 4, 0), two(4, 4), hd=48),
    X("x33_256_causal", 33, 256, gen(2, 2, 0), two(8, 4), hd=48, causal=True),
    X("x9_204_t18", 9, 204, gen(1, 1, 0), two(7, 4), B=3, lay="t18"),
    X("x40_100_klen", 40, 100, gen(2, 2, 0), two(4, 4), B=5, klen=KL5(100)),
    X("x300_40", 300, 40, gen(10, 5, 1), stream(10)),
    S("s196_sep", 196, pf(7), dqw(0), lay="sep"),
    # -- more items than workgroups on the persistent kernels (540 = 2 x 256 + 28; 1200 for the short masked rows)
    S("many_pf7", 196, pf(7), dqw(0), B=45, H=12),
    S("many_pf3", 77, pf(3, 1), sp(3, 1), B=150, H=8, causal=True),
    S("many_sp8", 256, gen(8, 8, 1), sp(8), B=45, H=12),
    S("many_spl", 160, gen(5, 5, 1), spl(5), B=45, H=12),
    S("many_pf6", 192, pf(6), spl(6), B=45, H=12),
    S("many_dqwm", 288, gen(9, 5, 1), dqw(1), B=65, H=8),
    # -- exact fp32: three GEMMs and a softmax kernel forward, four GEMMs and one kernel backward
    S("f32_s197", 197, f32r(7), f32r(7), dtype=F32),
    S("f32_s77_causal", 77, f32r(3), f32r(3), dtype=F32, causal=True),
    S("f32_s40_klen", 40, f32r(2), f32r(2), B=5, dtype=F32, klen=KL5(40)),
    X("f32_x40_100", 40, 100, f32r(4), f32r(4), dtype=F32),
]
_SEEN = {}   # case name -> (forward instance, backward instance) of the routes it took


def fwd_instance(r):
    kernel, tiles, variant = r
    if kernel == "pf":
        return ("pf", tiles, "causal" if variant & 1 else "plain")
    if kernel == "generic":
        return ("generic", "one group" if tiles <= 8 else "several groups", "staged" if variant & 1 else "unstaged")
    return (kernel,)


def bwd_instance(r, case):
    kernel, tiles, variant = r
    if kernel == "dqw":
        return ("dqw", "multi" if variant & 1 else "single")
    if kernel == "sp":
        if not variant & 1:
            return ("sp<false>",)
        return ("sp<true>", "both" if case.causal and case.klen else ("causal" if case.causal else "klen"))
    return (kernel,)


FWD_INSTANCES = ([("smallq",), ("f32",)] + [("pf", nt, c) for nt in (3, 6, 7) for c in ("plain", "causal")]
                 + [("generic", "one group", "unstaged"), ("generic", "one group", "staged"),
                    ("generic", "several groups", "staged")])
BWD_INSTANCES = ([("smallq",), ("f32",), ("dqw", "single"), ("dqw", "multi"), ("stream",), ("spl",), ("sp<false>",),
                  ("twopass",)] + [("sp<true>", m) for m in ("causal", "klen", "both")])


# ---- reference and emulation ------------------------------------------------------------------------------------------
def build_mask(case, dev, klen_plus=0, causal_plus=0):
    """(B, 1, Tq, Tk) bool: key < klen[b] + klen_plus and, if causal, key <= q + causal_plus"""
    key = torch.arange(case.Tk, device=dev)
    m = torch.ones(case.B, 1, case.Tq, case.Tk, dtype=torch.bool, device=dev)
    if case.klen is not None:
        kl = torch.tensor(case.klen, device=dev).clamp(max=case.Tk) + klen_plus
        m = m & (key[None, :] < kl[:, None])[:, None, None, :]
    if case.causal:
        q = torch.arange(case.Tq, device=dev)
        m = m & (key[None, :] <= q[:, None] + causal_plus)
    return m


def drop_last_key(mask):
    """the mask without the last valid key of every row that has at least two"""
    cnt = mask.cumsum(-1)
    tot = cnt[..., -1:]
    return mask & ~((cnt == tot) & mask & (tot >= 2))


def r16(x):
    return x.to(BF).double()


def attention(Q, K, V, dO, mask, scale, emulate=False, want_p=False, chunk_elems=1 << 25):
    """softmax attention and its gradients in fp64; Q, dO (B, Tq, H, hd), K, V (B, Tk, H, hd), mask (B, 1, Tq, Tk).
    emulate: round P, dS and the outputs to bf16 where a bf16 kernel does.  Returns a dict of (B, T, H * hd) tensors, the
    log-sum-exp (B, H, Tq), the token sums of dQ before its rounding (B, H * hd) and, if asked, P (B, H, Tq, Tk)."""
    B, Tq, H, hd = Q.shape
    Tk = K.shape[1]
    rnd = r16 if emulate else (lambda x: x)
    step = max(1, chunk_elems // (H * Tq * Tk))
    outs = {k: [] for k in ("O", "lse", "dQ", "dK", "dV", "csq", "P")}
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        q, k, v, g = (t[sl].double().permute(0, 2, 1, 3) for t in (Q, K, V, dO))      # (b, H, T, hd)
        s = (scale * (q @ k.transpose(-1, -2))).masked_fill(~mask[sl], float("-inf"))
        lse = torch.logsumexp(s, -1)
        p = torch.exp(s - lse[..., None])
        pm = rnd(p)
        o = rnd(pm @ v)
        dsum = (g * o).sum(-1, keepdim=True)
        ds = rnd(p * (g @ v.transpose(-1, -2) - dsum))
        dq = scale * (ds @ k)
        flat = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], H * hd)   # noqa: E731
        outs["O"].append(flat(o))
        outs["lse"].append(lse)
        outs["dQ"].append(flat(rnd(dq)))
        outs["dK"].append(flat(rnd(scale * (ds.transpose(-1, -2) @ q))))
        outs["dV"].append(flat(rnd(pm.transpose(-1, -2) @ g)))
        outs["csq"].append(dq.sum(2).reshape(-1, H * hd))
        if want_p:
            outs["P"].append(p)
    return {k: torch.cat(v) for k, v in outs.items() if v}


# ---- frames --------------------------------------------------------------------------------------------------------------
class Buf:
    """a flat NaN buffer of `rows` rows of `pitch` elements and the mask of the elements that views handed out cover"""

    def __init__(self, rows, pitch, dtype, dev):
        self.t = torch.full((rows * pitch,), float("nan"), dtype=dtype, device=dev)
        self.inside = torch.zeros(rows * pitch, dtype=torch.bool, device=dev)
        self.pitch = pitch

    def view(self, shape, strides, off):
        self.inside.as_strided(shape, strides, off).fill_(True)
        return self.t.as_strided(shape, strides, off)


@dataclasses.dataclass
class Slot:
    buf: Buf
    v: torch.Tensor             # (B, T, H * hd) view
    strides: tuple              # (sb, st)
    off: int                    # element offset of the view in buf.t

    @property
    def base(self):             # the tensor whose data pointer is the view's first element
        return self.buf.t[self.off:]


def sample_major(B, T, W, pitch, dtype, dev, ncol=1):
    """ncol tensors of width W side by side in rows of `pitch` elements; the samples GAP rows apart"""
    buf = Buf(ABOVE + B * (T + GAP) + BELOW, pitch, dtype, dev)
    sb = (T + GAP) * pitch
    return [Slot(buf, buf.view((B, T, W), (sb, pitch, 1), ABOVE * pitch + c * W), (sb, pitch), ABOVE * pitch + c * W)
            for c in range(ncol)]


def token_major(B, T, W, pitch, dtype, dev, ncol=1):
    """the torch-1.8 key layout: row r * B + b is token r of sample b"""
    buf = Buf(ABOVE + (T + BELOW) * B, pitch, dtype, dev)
    return [Slot(buf, buf.view((B, T, W), (pitch, B * pitch, 1), ABOVE * pitch + c * W), (pitch, B * pitch),
                 ABOVE * pitch + c * W) for c in range(ncol)]


def make_slots(case, dev):
    B, Tq, Tk, W, dt = case.B, case.Tq, case.Tk, case.H * case.hd, case.dtype
    s = {}
    if case.lay == "packed":
        s["Q"], s["K"], s["V"] = sample_major(B, Tq, W, 3 * W + 8, dt, dev, 3)
        s["dQ"], s["dK"], s["dV"] = sample_major(B, Tq, W, 3 * W + 16, dt, dev, 3)
    else:
        s["Q"], = sample_major(B, Tq, W, W + 16, dt, dev)
        s["dQ"], = sample_major(B, Tq, W, W + 40, dt, dev)
        if case.lay == "t18":
            s["K"], s["V"] = token_major(B, Tk, W, 2 * W + 8, dt, dev, 2)
            s["dK"], s["dV"] = token_major(B, Tk, W, 2 * W + 24, dt, dev, 2)
        else:
            s["K"], = sample_major(B, Tk, W, W + 32, dt, dev)
            s["V"], = sample_major(B, Tk, W, W + 48, dt, dev)
            s["dK"], = sample_major(B, Tk, W, W + 56, dt, dev)
            s["dV"], = sample_major(B, Tk, W, W + 64, dt, dev)
    s["O"], = sample_major(B, Tq, W, W + 8, dt, dev)
    s["dO"], = sample_major(B, Tq, W, W + 24, dt, dev)
    return s


def guarded(n, dev):
    t = torch.full((n + 2 * GUARD,), float("nan"), dtype=F32, device=dev)
    return t, t[GUARD:GUARD + n]


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).clone()


# ---- the kernels under test --------------------------------------------------------------------------------------------
def make_desc(case, s, klen_t):
    return ops._attn_desc(s["Q"].base, s["K"].base, s["V"].base, s["O"].base, case.B, case.H, case.Tq, case.Tk, case.hd,
                          s["Q"].strides, s["K"].strides, s["V"].strides, s["O"].strides, case.hd ** -0.5, case.causal,
                          klen=klen_t)


def kernel_fwd(case, s, klen_t, stats):
    ops.p_attn_fwd(make_desc(case, s, klen_t), s["Q"].base, stats=stats)
    return ops.attn_last_route()


def kernel_bwd(case, s, klen_t, stats, colsum):
    d = make_desc(case, s, klen_t)
    nbytes = ops.L.load().segclip_attn_bwd_ws_bytes(ctypes.byref(d))
    ws = torch.full((nbytes // 4 + 1,), float("nan"), dtype=F32, device=s["Q"].v.device)
    ops.p_attn_bwd(d, stats, s["dO"].base, s["dQ"].base, s["dK"].base, s["dV"].base, s["dQ"].strides, s["dK"].strides,
                   s["dV"].strides, s["dO"].strides, colsum_part=colsum, ws=ws)
    return ops.attn_last_route()


def stats_numel(case):
    n = case.B * case.H * case.Tq
    return n if case.dtype == BF else n * case.Tk


# ---- one row -------------------------------------------------------------------------------------------------------------
def where_bad(got, ref, rtol):
    """index ranges (sample, token, column) of the elements beyond the bound, for the assertion message"""
    bad = _beyond(got, ref, rtol)[0]
    if not bool(bad.any()):
        return ""
    idx = bad.nonzero()
    return " beyond the bound at " + ", ".join(f"dim{d} {int(idx[:, d].min())}..{int(idx[:, d].max())}" for d in range(idx.shape[1]))


def check_t(got, ref, rtol, what):
    check(got, ref, rtol, what + where_bad(got, ref, rtol))


def outside_intact(bufs):
    return all(bool(b.t[~b.inside].isnan().all()) for b in bufs)


def run_case(case, fwd, bwd, dev, routes=True, floors=None):
    """the row's checks with fwd / bwd as the kernels (the test passes kernel_fwd / kernel_bwd; a CPU run can pass an
    emulation to show what the checks catch).  floors: dict that receives the emulation's error per tensor class."""
    gen_ = torch.Generator().manual_seed(sum(map(ord, case.name)))   # host generator: the same inputs on every device
    B, H, Tq, Tk, hd, W = case.B, case.H, case.Tq, case.Tk, case.hd, case.H * case.hd
    bf = case.dtype == BF
    scale = hd ** -0.5
    s = make_slots(case, dev)
    vals = {}
    for name, T in (("Q", Tq), ("K", Tk), ("V", Tk), ("dO", Tq)):
        vals[name] = torch.randn(B, T, W, generator=gen_, dtype=torch.float64).to(case.dtype).to(dev)
        s[name].v.copy_(vals[name])
    klen_t = None
    if case.klen is not None:
        klen_t = torch.tensor(case.klen, dtype=torch.int32, device=dev)
        dead = (torch.arange(Tk, device=dev)[None, :] >= klen_t[:, None])[:, :, None].expand(B, Tk, W)
        for name in ("K", "V"):    # a masked key may be loaded, never used; finite because it is multiplied by an exact 0
            s[name].v.masked_fill_(dead, MASKED_KV)
    stats_buf, stats = guarded(stats_numel(case), dev)
    cs_buf, cs = guarded(B * 3 * W, dev) if bf else (None, None)
    out_f, out_b = [s["O"].buf], list({id(s[n].buf): s[n].buf for n in ("dQ", "dK", "dV")}.values())
    refused = case.bwd == REFUSED

    def forward_backward():
        rf = fwd(case, s, klen_t, stats)
        if refused:
            with pytest.raises(RuntimeError, match="klen needs sequences of at most 256"):
                bwd(case, s, klen_t, stats, cs)
            rb = ops.attn_last_route() if routes else None
        else:
            rb = bwd(case, s, klen_t, stats, cs)
        if dev != "cpu":
            torch.cuda.synchronize()
        return rf, rb, [bits(b.t) for b in out_f + out_b] + [bits(stats_buf)] + ([bits(cs_buf)] if bf else [])

    # 1. routes
    rf, rb, snap = forward_backward()
    if routes:
        assert rf == ops.AttnRoute(case.fwd[0], None, *case.fwd[1:]), f"{case.name}: the forward took {rf}"
        assert rb == ops.AttnRoute(None, case.bwd[0], *case.bwd[1:]), f"{case.name}: the backward took {rb}"
        _SEEN[case.name] = (fwd_instance(case.fwd), None if refused else bwd_instance(case.bwd, case))

    # 6. repeatable, frames included
    again = forward_backward()[2]
    assert all(torch.equal(x, y) for x, y in zip(snap, again)), f"{case.name}: the second forward + backward differs"

    # 5. frames: nothing outside the views is written, everything inside is
    assert outside_intact(out_f), f"{case.name}: O written outside its (B, Tq, H * hd) view"
    assert bool(stats_buf[:GUARD].isnan().all() and stats_buf[GUARD + stats.numel():].isnan().all()), f"{case.name}: statistics written outside"
    assert bool(s["O"].v.isfinite().all()) and bool(stats.isfinite().all()), f"{case.name}: O / statistics not finite"
    assert outside_intact(out_b), f"{case.name}: dQ / dK / dV written outside their views"
    if refused:
        assert all(bool(b.t.isnan().all()) for b in out_b) and bool(cs_buf.isnan().all()), f"{case.name}: a refused call wrote"
    else:
        assert all(bool(s[n].v.isfinite().all()) for n in ("dQ", "dK", "dV")), f"{case.name}: gradients not finite"
        if bf:
            assert bool(cs_buf[:GUARD].isnan().all() and cs_buf[GUARD + cs.numel():].isnan().all()), f"{case.name}: token sums written outside"

    # 2. values against fp64
    shape = lambda t: t.reshape(B, -1, H, hd)   # noqa: E731
    ins = [shape(vals[n]) for n in ("Q", "K", "V", "dO")]
    mask = build_mask(case, dev)
    ref = attention(*ins, mask, scale, want_p=not bf)
    many = B * H > 512
    assert many or B * H <= 64
    rt_o, rt_g = RT_BF[(case.causal or case.klen is not None, many)] if bf else (RT_F32, RT_F32)
    got = {"O": s["O"].v}
    check_t(got["O"], ref["O"], rt_o, f"{case.name}: O")
    if bf:
        check_t(stats.view(B, H, Tq), ref["lse"], RT_LSE, f"{case.name}: log-sum-exp")
    else:
        check_t(stats.view(B, H, Tq, Tk), ref["P"], RT_F32, f"{case.name}: P")
    names = ["O"]
    if not refused:
        names += ["dQ", "dK", "dV"]
        for n in names[1:]:
            got[n] = s[n].v
            check_t(got[n], ref[n], rt_g, f"{case.name}: {n}")
        if bf:
            # every kernel forms the token sums from fp32 values by the identities sum_q dQ = sum_key K cs[key] (cs = the
            # column sums of dS), sum_key dK = 0 (the rows of dS sum to zero; written as an exact 0) and sum_key dV = sum_q dO:
            # the reference is the fp64 gradient's token sums, never the stored bf16 rows'
            c3 = cs.view(B, 3, W)
            check_t(c3[:, 0], ref["csq"], RT_CS, f"{case.name}: token sums of dQ")
            assert bool((c3[:, 1] == 0).all()), f"{case.name}: token sums of dK are not the exact 0"
            check_t(c3[:, 2], ref["dV"].sum(1), RT_CS_DV, f"{case.name}: token sums of dV")

    # 3. the rounding floor of this row's inputs is at most half the bound
    if bf:
        emu = attention(*ins, mask, scale, emulate=True)
        for n, rt in [("O", rt_o)] + ([("dQ", rt_g), ("dK", rt_g), ("dV", rt_g), ("csq", RT_CS)] if not refused else []):
            if floors is not None:
                bad, err, rms = _beyond(emu[n], ref[n], 0.0)
                cls = "O" if n == "O" else ("CS" if n == "csq" else "G")
                floors[cls] = max(floors.get(cls, 0.0), float((err / (ref[n].abs() + rms)).max()))
            assert within(emu[n], ref[n], rt / 2), f"{case.name}: the bf16 rounding floor of {n} is above half the bound"

    # 4. the bound is discriminating
    defects = {"the last valid key removed": attention(*ins, drop_last_key(mask), scale)}
    if case.causal or (case.klen is not None and min(case.klen) < Tk):
        defects["the mask moved by one key"] = attention(*ins, build_mask(case, dev, int(case.klen is not None), int(case.causal)),
                                                         scale)
    swapped = {}
    kv = torch.tensor(case.klen if case.klen is not None else [Tk] * B).clamp(max=Tk)
    for n in names:
        t = ref[n].clone()
        if n in ("O", "dQ"):
            t[:, Tq - 2] = ref[n][:, Tq - 1]
        else:                      # the last two valid keys of every sample that has two (rows of masked keys are zero);
            for b in range(B):     # under causal the middle of the valid range: the last keys' gradients are far below the rms
                j = min(int(kv[b]), Tq) // 2 if case.causal else int(kv[b]) - 1
                if j >= 1:
                    t[b, j - 1] = ref[n][b, j]
        swapped[n] = t
    defects["a row replaced by its neighbour"] = swapped
    for what, wrong in defects.items():
        for n in names:
            rt = rt_o if n == "O" else rt_g
            assert not within(got[n], wrong[n], rt), f"{case.name}: the check of {n} accepts {what}"
    return ref, got


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_attn_route_and_value(case):
    run_case(case, kernel_fwd, kernel_bwd, DEV)


def test_second_device_raises_its_own_lds_limit():
    """the streaming pair and the two-pass backward need more dynamic LDS than the default limit, and that limit is raised
    per (kernel, device): in one process, first on device 0, then on device 1, with the checks of the table's rows"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    rows = [c for c in CASES if c.name in ("s319", "x33_256_causal")]
    assert [c.bwd[0] for c in rows] == ["stream", "twopass"]
    for i in (0, 1):
        with torch.cuda.device(i):
            for case in rows:
                run_case(case, kernel_fwd, kernel_bwd, f"cuda:{i}")


def test_call_that_launches_nothing_records_no_route():
    case = S("probe", 64, gen(2, 2, 0), sp(2))
    s = make_slots(case, DEV)
    for n in ("Q", "K", "V"):
        s[n].v.zero_()
    _, stats = guarded(stats_numel(case), DEV)
    assert kernel_fwd(case, s, None, stats).fwd_kernel == "generic"
    d = make_desc(case, s, None)
    d.flags = ops.L.ATTN_FP8
    with pytest.raises(ops.L.Unsupported):    # the removed e4m3 forward
        ops.p_attn_fwd(d, s["Q"].base, stats=stats)
    assert ops.attn_last_route() == ops.AttnRoute(None, None, 0, 0)
    assert kernel_fwd(case, s, None, stats).fwd_kernel == "generic"
    d = make_desc(case, s, None)
    d.B = 0
    ops.p_attn_fwd(d, s["Q"].base, stats=stats)
    assert ops.attn_last_route() == ops.AttnRoute(None, None, 0, 0)
    assert ops.L.load().segclip_attn_last_route(None) == -2


def test_table_reaches_every_instance():
    """the routes the table's rows took (test_attn_route_and_value, run before this) cover every reachable instance"""
    expected = {c.name: (fwd_instance(c.fwd), None if c.bwd == REFUSED else bwd_instance(c.bwd, c)) for c in CASES}
    for i, inst in ((0, FWD_INSTANCES), (1, BWD_INSTANCES)):
        missing = sorted(set(inst) - {e[i] for e in expected.values()}, key=str)
        assert not missing, f"no row is meant to reach {missing}"
    not_run = sorted(set(expected) - set(_SEEN))
    assert not not_run, f"rows not run (or failed before their routes were recorded): {not_run}"
    for i, inst in ((0, FWD_INSTANCES), (1, BWD_INSTANCES)):
        missing = sorted(set(inst) - {e[i] for e in _SEEN.values()}, key=str)
        assert not missing, f"no row reached {missing}"
