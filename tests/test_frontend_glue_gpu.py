"""GPU: the kernels that feed and surround the towers - the front ends and glue of csrc/misc.hip (cast, split3, the stand-alone
activations, add, the Gumbel transform, im2col, the vision assembly, the text embedding and its backward, row gather / scatter,
mean_cat, mae_unshuffle, the MAE masking sort, the bicubic resample of the positional table) and the two multi-tensor helpers of
csrc/optim.hip (multi_cast_bf16, multi_add_f32) - one kernel at a time through the C ABI (segclip_amd._lib), the test owning every
buffer (tests/kernel_frames.py, as tests/test_loss_head_gpu.py and tests/test_center_stage_gpu.py).

Per row: (1) every output is a view inside a larger NaN buffer (0xAB in every byte for integer outputs): the guards survive and
everything inside is written; (2) the inputs sit in frames of the same kind; (3) the same call a second time into the same frames
is bit-identical, frames included - a call that accumulates (scatter_rows, the table gradient of embed_bwd, multi_add_f32) has its
destination refilled to the same contents before each call; (4) the values against a reference computed in fp64 on exactly the
fp32 / bf16 values the kernel reads, or bit for bit where the operation is a copy or one correctly rounded operation; (5) the same
bound REJECTS the reference after a small defect.

Rows (test_rows_reach_every_path restates each dispatcher and asserts that every path has a row):
  cast: f32->bf16, bf16->f32, f32->f32, bf16->bf16 x n in 1 2 3 4 5 7 1023 1024 1025 1027 and 4 x 1048576 + 1027 (past the grid cap,
      a tail of three).  Special values (+-0, +-inf, subnormals, the largest finite fp32, ties that round to even downward and
      upward, a tie that rounds to inf) stand at the front (the vector body, rounded by the hardware converter) and in the last
      n & 3 elements (the scalar tail, rounded by f2bf); the tails of the rows together walk the whole list.  Bit-exact against
      the host's .to(); one NaN in the body and one in the tail, asserted only as NaN.
  split3: (rows, cols) in (1,4) (3,8) (33,260) (200,768) x ld = cols, cols + 12 x stack x role; ties planted; every block bit-exact
      in its documented place; cols % 4 != 0 is refused and nothing is written.
  act_fwd / act_bwd: none, quick-GELU, erf-GELU x fp32, bf16 x n in 1 3 4 5 1023 1024 1028 1100003; the backward's rows split by
      n % 4 into the vec4 and the scalar kernel, one n % 4 == 0 row on views shifted by one element (scalar by misalignment), one
      vec4 row of 4 x (1048576 + 3) elements.  Inputs: Gaussian x 3 and, from n = 64 on, a ladder -90 .. 90 in steps of 3 in front
      (sigmoid and erf saturate, the hardware exp2 overflows to inf); the rows of 3, 4 and 5 start with -90, 0, 90.
  add: fp32, bf16 x the same n: one rounded add, bit-exact.
  gumbel_from_uniform: n in 1 1025 1100003; the end points 0, 1, FLT_MIN, 1 - eps; one row with out aliasing u.
  im2col / im2col_ld: layout 0, 1 x fp32, bf16 out x C in 1 3 x B in 1 3 x (p, H, W) in (8,16,24) (16,32,48) (14,28,42) (4,8,12);
      ld = kdim, kdim + 8 (vec8), kdim + 4 (the scalar kernel at p % 8 == 0) for p = 8, 16; kdim and the padding to a multiple of
      128 (588 -> 640) for p = 14; 8 x 3 x 224 x 224 at p = 16 (layout 1: past the cap on the scalar kernel; layout 0: 150528
      threads of the vec8 kernel, below its cap) and 56 x 3 x 224 x 224 (the vec8 kernel's second trip: 1053696 threads).  Bit-exact
      against unfold / the patchify einsum, pad columns exactly 0; H % p != 0 and ld < C p p refused, nothing written.
  vis_assemble: B in 1 3 x T in 1 4 49 x D in 4 65 768 x patches fp32, bf16; 8 x 196 x 768.  One add, bit-exact, CLS row included.
  embed_fwd: L in 1 5 77 x D in 4 64 260 512, B = 5, a positional table of L + 3 rows, ids with 0, V - 1, -3 and V + 5 (clamped to
      rows 0 and V - 1); 110 x 77 x 512 (more than 4 x 1048576 elements).  Bit-exact.
  embed_bwd: B in 1 3 4 5 8 9 (the four-in-flight loop alone, the tail alone, both) x the same L, D; 27 x 77 x 512 (the table
      kernel past the cap).  (a) small-integer dout, most ids the pad id: both outputs bit-exact and bit-identical across calls;
      (b) Gaussian dout with +0.0 and -0.0 behind an "EOT": dtable (dpos null) by the floor-based bound on both calls, dpos (dtable
      null) by the floor-based bound and bit-identical.  D % 4 != 0 with dpos is refused and dtable stays as it was.
  gather_rows / scatter_rows: fp32, bf16 x B in 1 3 x Ts in 1 16 197 x To in 1 7 Ts x D in 1 3 64 513; one gather row with the
      indices -1 and Ts + 3; scatter (To <= Ts, unique indices) into a nonzero prefill: the rows no index names keep their bits;
      11 x 197 x 513 past the cap.
  mean_cat_fwd / bwd: B in 1 3 x T in 1 2 7 49 196 x D in 4 36 256 260 768 1024; rows 1..T a bit-exact copy, at T = 1 the mean row
      too; 28 x 196 x 768 for the backward's second trip.
  mae_unshuffle_fwd / bwd: B in 1 3 7 8 9 16 17 x L in 1 4 77 197 x K in 1, L/4, L x D in 4 8 260 384 1024, ids a random permutation
      per sample; 22 x 197 x 1024 forward past the cap.  Forward and dx bit-exact, dpos and mpart by the floor-based bound, mpart
      exactly 0 at K = L, the column sum of mpart against the fp64 mask-token gradient.
  mask_sort: B in 1 6 x L in 1 2 255 256 257 4096 x len_keep in 0 1 L/4 L x noise uniform | eight levels | all equal | the largest
      value in column 0; against a stable host sort with column 0 set to -1; L = 4097 refused, nothing written.
  interp_bicubic: D in 1 5 768 x n -> (h, w) in 7->(7,7) 14->(14,14) (bit for bit the source) 14->(32,32) 16->(37,23) 14->(7,5)
      14->(1,1) 1->(3,3) 2->(5,3), and 14->(38,37) at D = 768 past the cap; against F.interpolate(bicubic, align_corners=False) in
      fp64.
  multi_cast_bf16 / multi_add_f32: 1, 32, 33, 36, 37, 70 tensors per call, sizes cycling through 1 3 4 5 16383 16384 16385 40001 0
      (the library counts 32 LIVE tensors per launch: 36 tensors are exactly one launch, 37 and 70 open a second), each tensor in
      a frame of its own; a source off 16 bytes is refused by the cast; one add row with every pair shifted by one float.
  grid1d is capped at 4096 blocks of 256 threads: the rows past it are named above.

Defects the bounds must reject (5): cast / split3: truncation on a tie, hi and lo swapped for one role.  act: 1.702 -> 1.7 (fp32
rows: the bf16 bound of 2^-8 is wider than that defect, 2e-4), x pdf dropped from the erf-GELU derivative, the last element from
its neighbour.  im2col: gh and gw swapped, py and px swapped, a pad column unwritten.  assemble / embed / gather / scatter: pos[t]
-> pos[t - 1], the clamp removed (Gumbel: without its clamp the end points give +-inf, which no bound measures; the defect
there is the lower clamp at FLT_EPSILON), a nonzero value skipped, the prefill dropped.  mean_cat: the mean over T + 1, the last
token left out.  mae_unshuffle: id <= K, sample 8 dropped from dpos.  mask_sort: ties to the higher index, column 0 not forced
first.  interp: A = -0.5, sx and sy swapped, border taps zeroed.  multi-tensor: the first tensor of the second launch left out,
element 16384 from its neighbour.

Bounds.  Copies, casts, gathers, im2col, integer outputs, masks: bit-exact.  One correctly rounded fp32 operation (add, the
scatter's add, assemble, embed_fwd): bit-exact against torch float32 of that operation and within 2^-24 of fp64.  bf16 outputs of
a computed value: 2^-8, as derived in tests/test_center_stage_gpu.py.  Every other fp32 output: floor = torch float32 of the same
expression against fp64 in check() units, |err| / (|ref| + rms(ref)), the maximum over the rows of the kernel; bound = 4 x floor
rounded up to one digit (the 4 covers another summation order).  The floor never involves the kernel.  Measured on an MI355X by
floors() (FLOORS holds the figures; `kernel` is this build's own error, for the record only):
    key             floor   -> bound    kernel     the floor's row
    act.quick.y     9.438e-08 -> 4e-07    9.665e-08  actf_quick_f32_n1100003
    act.quick.dx    7.894e-07 -> 4e-06    7.894e-07  actb_quick_f32_n4194316_s0
    act.erf.y       6.682e-08 -> 3e-07    6.682e-08  actf_erf_f32_n1100003
    act.erf.dx      1.955e-07 -> 8e-07    2.020e-07  actb_erf_f32_n4194316_s0
    gumbel          1.241e-07 -> 5e-07    1.489e-07  gumbel_n1100003
    embed.dpos      4.052e-07 -> 2e-06    5.636e-07  embb_b27_l77_d512
    embed.dtable    3.757e-07 -> 2e-06    3.727e-07  embb_b9_l5_d512
    meancat.mean    3.734e-07 -> 2e-06    1.362e-06  meancat_b3_t196_d768
    meancat.dx      4.907e-08 -> 2e-07    4.737e-08  meancat_b1_t7_d1024
    mae.dpos        3.010e-07 -> 2e-06    3.831e-07  mae_b17_k197_l197_d1024
    mae.mpart       2.878e-07 -> 2e-06    3.840e-07  mae_b22_k49_l197_d1024
    interp          4.937e-06 -> 2e-05    5.079e-06  interp_d768_14_to_38x37
  (embed.dtable's floor is torch's own atomic index_add_: it moves in its third digit from run to run.  act.quick.dx: torch
  float32 and the kernel reach the same figure in the same row.  The hardware exp2 and rcp of the activations, 1 ulp each as
  csrc/common.h states them, stay within 4 x the floor: no bound here is derived from those ulps.)

Fixes that came with this file:
  - segclip_embed_bwd checked D % 4 for dpos after it had launched the table kernel: the refused call had already added dout
    into dtable.  The check now comes before either launch.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segclip_amd import _lib as L  # noqa: E402
from tests.helpers import within  # noqa: E402
from tests.kernel_frames import BF, DEV, F32, F64, IDX_FILL_WIDE, Bounds, Frame, draw, lib_call, put, run_twice, seeded  # noqa: E402

Fn = torch.nn.functional
I64 = torch.int64
RT_BF = 2.0 ** -8
RT_ONE = 2.0 ** -24
GRID_CAP = 4096 * 256          # grid1d of csrc/misc.hip: at most 4096 blocks of 256 threads
CHUNK, PER_LAUNCH = 16384, 32  # csrc/optim.hip: elements per workgroup, tensors per launch

# floors measured by floors() (torch float32 against fp64 on this file's rows, maximum over the rows of the kernel)
FLOORS = {
    "act.quick.y": 9.438e-08,
    "act.quick.dx": 7.894e-07,
    "act.erf.y": 6.682e-08,
    "act.erf.dx": 1.955e-07,
    "gumbel": 1.241e-07,
    "embed.dpos": 4.052e-07,
    "embed.dtable": 3.757e-07,
    "meancat.mean": 3.734e-07,
    "meancat.dx": 4.907e-08,
    "mae.dpos": 3.010e-07,
    "mae.mpart": 2.878e-07,
    "interp": 4.937e-06,
}
BOUNDS = Bounds(FLOORS)
RT = BOUNDS.rt
judge, rejects = BOUNDS.judge, BOUNDS.rejects


def measuring():
    return BOUNDS.stats is not None


def code(dt):
    return L.F32 if dt == F32 else L.BF16


def tag(dt):
    return "f32" if dt == F32 else "bf16"


def ibits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(ibits(a), ibits(b))


def exact(what, got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {got.dtype}{tuple(got.shape)} against {ref.dtype}{tuple(ref.shape)}"
    bad = ibits(got) != ibits(ref)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements differ in their bits"


def differs(what, got, wrong):
    """the bit-exact comparison rejects the defect"""
    assert got.shape == wrong.shape, f"{what}: {tuple(got.shape)} against {tuple(wrong.shape)}"
    assert not same(got, wrong.to(got.dtype)), f"{what}: the bit-exact comparison accepts the defect"


def neighbour(ref):
    """the reference with its last element taken from the one before"""
    w = ref.clone()
    w.view(-1)[-1] = ref.reshape(-1)[-2]
    return w


def refused(fn_name, *args):
    with pytest.raises(RuntimeError):
        lib_call(fn_name, *args)
    torch.cuda.synchronize()


def sync():
    torch.cuda.synchronize()


SMALL_N = (1, 3, 4, 5, 1023, 1024, 1028)
BIG_N = 1100003

# ---- cast ---------------------------------------------------------------------------------------------------------------------
# ties first: 1 + 2^-8 (to even: down), +-(1 + 3 x 2^-8) (to even: up), the largest finite fp32 (-> inf); the last: a tie that rounds to inf
SPECIALS = (0x3f808000, 0x3f818000, 0xbf818000, 0x7f7fffff, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff,
            0x00008000, 0x00018000, 0xff7fffff, 0x3f808001, 0x3f807fff, 0x7f7f8000)
NAN_BITS = 0x7fc01234
WALK = SPECIALS + (NAN_BITS,)
FRONT = SPECIALS + (NAN_BITS,) + SPECIALS[:3]          # five vectors of four
CAST_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 4 * 1048576 + 1027)
TAIL_START = dict(zip(CAST_N, itertools.accumulate([1] + [n & 3 for n in CAST_N])))   # (from 1: no tail repeats the element before it)
CAST_CASES = [(sd, dd, n) for sd in (F32, BF) for dd in (BF, F32) for n in CAST_N]


def cast_bits(n):
    """the fp32 bit patterns of a cast row: Gaussian x 3, FRONT over the first elements of the vector body, the tail's share of WALK"""
    x = (torch.randn(n, generator=seeded(f"cast_{n}"), dtype=F64) * 3).float().numpy()
    bits = x.view(np.uint32)
    body, tail = n // 4 * 4, n & 3
    k = min(body, len(FRONT))
    bits[:k] = FRONT[:k]
    for j in range(tail):
        bits[body + j] = WALK[(TAIL_START[n] + j) % len(WALK)]
    return bits


def cast_source(n, sd):
    """the host tensor of a cast row in the source type (bf16: the upper halves of the fp32 patterns)"""
    bits = cast_bits(n)
    if sd == F32:
        return torch.from_numpy(bits.view(np.float32).copy())
    return torch.from_numpy((bits >> 16).astype(np.uint16).view(np.int16).copy()).view(BF)


def truncated(x):
    """fp32 -> bf16 by dropping the lower half"""
    return (ibits(x) & -65536).view(F32).to(BF)


@pytest.mark.parametrize("sd,dd,n", CAST_CASES, ids=[f"cast_{tag(s)}_{tag(d)}_n{n}" for s, d, n in CAST_CASES])
def test_cast(sd, dd, n):
    name = f"cast_{tag(sd)}_{tag(dd)}_n{n}"
    src = cast_source(n, sd)
    nan, want = src.isnan(), src.to(dd)            # the host's conversion
    ok = ~nan
    fs, fd = put(src.to(DEV)), Frame((n,), dd)

    def call():
        lib_call("segclip_cast", fs.p, fd.p, n, code(sd), code(dd))
    run_twice(name, call, [fd], finite=False)
    assert fs.intact()
    got = fd.v.cpu()
    exact(name, got[ok], want[ok])
    assert bool(got[nan].isnan().all()), f"{name}: a NaN must stay a NaN"
    fd.v.fill_(1.0)                                # a finite prefill: every element is written, the NaNs included
    call()
    sync()
    got = fd.v.cpu()
    exact(name + " over a finite prefill", got[ok], want[ok])
    assert bool(got[nan].isnan().all()) and fd.intact()
    if sd == F32 and dd == BF and n >= 4:
        differs(f"{name}: truncation", got[ok], truncated(src)[ok])
    if n >= 4:
        differs(f"{name}: the last element from its neighbour", got[ok], neighbour(want[ok]))


# ---- split3 ---------------------------------------------------------------------------------------------------------------------
SPLIT_SHAPES = ((1, 4), (3, 8), (33, 260), (200, 768))
SPLIT_CASES = [(r, c, pad, stack, role) for r, c in SPLIT_SHAPES for pad in (0, 12) for stack in (0, 1) for role in (0, 1)]


def split_blocks(x, role, trunc=False):
    hi = truncated(x) if trunc else x.to(BF)
    lo = (x - hi.float()).to(BF)
    return (hi, lo, hi) if role == 0 else (hi, hi, lo)


def split_input(name, rows, cols):
    x = draw(seeded(name), rows, cols)
    flat = ibits(x).view(-1)
    flat[:4] = torch.tensor([0x3f808000, 0x3f818000, 0x3f808001, -0x407e8000], dtype=torch.int32)   # ties (the last: -(1 + 3 x 2^-8))
    return flat.view(F32).reshape(rows, cols)


@pytest.mark.parametrize("rows,cols,pad,stack,role", SPLIT_CASES, ids=[f"split3_{r}x{c}_pad{p}_stack{s}_role{o}" for r, c, p, s, o in SPLIT_CASES])
def test_split3(rows, cols, pad, stack, role):
    name = f"split3_{rows}x{cols}_pad{pad}_stack{stack}_role{role}"
    x = split_input(name, rows, cols)
    fx = put(x, pitch=cols + pad)
    fd = Frame((rows, 3 * cols) if stack == 0 else (3 * rows, cols), BF)
    run_twice(name, lambda: lib_call("segclip_split3_bf16", fx.p, fd.p, rows, cols, cols + pad, stack, role), [fd])
    assert fx.intact()
    blocks = split_blocks(x, role)
    for k, blk in enumerate(blocks):
        got = fd.v[:, k * cols:(k + 1) * cols] if stack == 0 else fd.v[k * rows:(k + 1) * rows]
        exact(f"{name}: block {k}", got, blk)
    cat = 1 if stack == 0 else 0
    differs(f"{name}: hi and lo of the other role", fd.v, torch.cat(split_blocks(x, 1 - role), cat))
    differs(f"{name}: truncation", fd.v, torch.cat(split_blocks(x, role, trunc=True), cat))


def test_split3_refuses_cols_not_multiple_of_4():
    rows, cols = 3, 6
    fx, fd = put(draw(seeded("split3_gate"), rows, 8)), Frame((rows, 3 * 8), BF)
    refused("segclip_split3_bf16", fx.p, fd.p, rows, cols, 8, 0, 0)
    assert fd.untouched() and fx.intact()


# ---- activations, add -----------------------------------------------------------------------------------------------------------
ACTS = ("none", "quick", "erf")
LADDER = torch.linspace(-90, 90, 61, dtype=F64)
VEC_BIG = 4 * (1048576 + 3)


def act_code(act):
    return {"none": L.ACT_NONE, "quick": L.ACT_QUICK_GELU, "erf": L.ACT_GELU_ERF}[act]


def act_input(name, n, dt):
    """Gaussian x 3; the ladder in front from n = 64 on, -90, 0, 90 from n = 3 on; the last two elements fixed (and distinct)
    from n = 5 on"""
    x = torch.randn(n, generator=seeded(name), dtype=F64) * 3
    if n >= 64:
        x[:61] = LADDER
    elif n >= 3:
        x[:3] = torch.tensor([-90.0, 0.0, 90.0], dtype=F64)
    if n >= 5:
        x[-2], x[-1] = -0.75, 1.5
    return x.to(dt).to(DEV)


def act_expr(act, x, dt, c=1.702, drop_pdf=False):
    """(act(x), act'(x)) in dt"""
    x = x.to(dt)
    if act == "none":
        return x, torch.ones_like(x)
    if act == "quick":
        s = torch.sigmoid(c * x)
        return x * s, s * (1 + c * x * (1 - s))
    cdf = 0.5 * (1 + torch.erf(x * math.sqrt(0.5)))
    pdf = torch.exp(-0.5 * x * x) * (1 / math.sqrt(2 * math.pi))
    return x * cdf, cdf + (0 if drop_pdf else x * pdf)


def act_judge(key, name, dt, got, ref, ref32):
    if dt == BF:
        judge(key, name, got, ref, rtol=RT_BF)
    else:
        judge(key, name, got, ref, ref32)


ACT_FWD_CASES = [(a, dt, n) for a in ACTS for dt in (F32, BF) for n in SMALL_N + (BIG_N,)]


@pytest.mark.parametrize("act,dt,n", ACT_FWD_CASES, ids=[f"actf_{a}_{tag(d)}_n{n}" for a, d, n in ACT_FWD_CASES])
def test_act_fwd(act, dt, n):
    name = f"actf_{act}_{tag(dt)}_n{n}"
    x = act_input(name, n, dt)
    fx, fy = put(x), Frame((n,), dt)
    run_twice(name, lambda: lib_call("segclip_act_fwd", fx.p, fy.p, n, act_code(act), code(dt)), [fy])
    assert fx.intact()
    if act == "none":
        exact(name, fy.v, x)
        if n >= 2:
            differs(f"{name}: the last element from its neighbour", fy.v, neighbour(x))
        return
    key = f"act.{act}.y"
    ref = act_expr(act, x, F64)[0]
    act_judge(key, name, dt, fy.v, ref, act_expr(act, x, F32)[0] if measuring() and dt == F32 else None)
    rt = RT_BF if dt == BF else None
    if n >= 4:
        rejects(key, f"{name}: the last element from its neighbour", fy.v, neighbour(ref), rtol=rt)
    if act == "quick" and dt == F32 and n >= 1023:
        rejects(key, f"{name}: 1.7 for 1.702", fy.v, act_expr(act, x, F64, c=1.7)[0])


# (n, shift): the vec4 kernel needs n % 4 == 0 and 16-byte aligned pointers
ACT_BWD_ROWS = [(n, 0) for n in SMALL_N] + [(1024, 1), (VEC_BIG, 0)]
ACT_BWD_CASES = [(a, dt, n, s) for a in ACTS for dt in (F32, BF) for n, s in ACT_BWD_ROWS]


def act_bwd_route(n, ptrs):
    return "vec4" if n % 4 == 0 and all(p % 16 == 0 for p in ptrs) else "scalar"


@pytest.mark.parametrize("act,dt,n,shift", ACT_BWD_CASES, ids=[f"actb_{a}_{tag(d)}_n{n}_s{s}" for a, d, n, s in ACT_BWD_CASES])
def test_act_bwd(act, dt, n, shift):
    name = f"actb_{act}_{tag(dt)}_n{n}_s{shift}"
    x = act_input(name, n, dt)
    dy = draw(seeded(name + "dy"), n, dtype=dt)
    fx, fg, fd = put(x, shift=shift), put(dy, shift=shift), Frame((n,), dt, shift=shift)
    ptrs = [f.v.data_ptr() for f in (fx, fg, fd)]
    assert act_bwd_route(n, ptrs) == ("vec4" if n % 4 == 0 and shift == 0 else "scalar"), "the frames are not aligned as the row assumes"
    run_twice(name, lambda: lib_call("segclip_act_bwd", fg.p, fx.p, fd.p, n, act_code(act), code(dt)), [fd])
    assert fx.intact() and fg.intact()
    if act == "none":
        exact(name, fd.v, dy)
        if n >= 2:
            differs(f"{name}: the last element from its neighbour", fd.v, neighbour(dy))
        return
    key = f"act.{act}.dx"
    ref = dy.double() * act_expr(act, x, F64)[1]
    act_judge(key, name, dt, fd.v, ref, dy * act_expr(act, x, F32)[1] if measuring() and dt == F32 else None)
    rt = RT_BF if dt == BF else None
    if n >= 4:
        rejects(key, f"{name}: the last element from its neighbour", fd.v, neighbour(ref), rtol=rt)
    if act == "quick" and dt == F32 and n >= 1023:
        rejects(key, f"{name}: 1.7 for 1.702", fd.v, dy.double() * act_expr(act, x, F64, c=1.7)[1])
    if act == "erf" and n >= 1023:
        rejects(key, f"{name}: x pdf dropped", fd.v, dy.double() * act_expr(act, x, F64, drop_pdf=True)[1], rtol=rt)


ADD_CASES = [(dt, n) for dt in (F32, BF) for n in SMALL_N + (BIG_N,)]


@pytest.mark.parametrize("dt,n", ADD_CASES, ids=[f"add_{tag(d)}_n{n}" for d, n in ADD_CASES])
def test_add(dt, n):
    name = f"add_{tag(dt)}_n{n}"
    gen = seeded(name)
    a, b = draw(gen, n, dtype=dt), draw(gen, n, dtype=dt, scale=3.0)
    fa, fb, fo = put(a), put(b), Frame((n,), dt)
    run_twice(name, lambda: lib_call("segclip_add", fa.p, fb.p, fo.p, n, code(dt)), [fo])
    assert fa.intact() and fb.intact()
    want = (a.float() + b.float()).to(dt)          # one rounded add (bf16: the fp32 sum rounded once)
    exact(name, fo.v, want)
    judge("add", name, fo.v, a.double() + b.double(), rtol=RT_ONE if dt == F32 else RT_BF)
    if n >= 2:
        differs(f"{name}: the last element from its neighbour", fo.v, neighbour(want))


# ---- Gumbel transform -----------------------------------------------------------------------------------------------------------
FLT_MIN, FLT_EPS = 1.17549435e-38, 1.1920929e-07
ENDS = (0.0, 1.0, FLT_MIN, 1.0 - FLT_EPS)
GUMBEL_CASES = [(1, False), (4, False), (1025, False), (1025, True), (BIG_N, False)]


def gumbel_expr(u, dt, low=FLT_MIN):
    if low is not None:
        u = u.clamp(torch.tensor(low, dtype=F32).item(), torch.tensor(1.0 - FLT_EPS, dtype=F32).item())   # exact in fp32
    return -torch.log(-torch.log(u.to(dt)))


@pytest.mark.parametrize("n,alias", GUMBEL_CASES, ids=[f"gumbel_n{n}{'_alias' if a else ''}" for n, a in GUMBEL_CASES])
def test_gumbel(n, alias):
    """n = 4 is the four end points alone; longer rows start with them"""
    name = f"gumbel_n{n}{'_alias' if alias else ''}"
    u = torch.rand(n, generator=seeded(name), dtype=F32)
    if n >= 4:
        u[:4] = torch.tensor(ENDS, dtype=F32)
    u = u.to(DEV)
    fu, fo = put(u), Frame((n,), F32)
    if alias:
        def call():
            fo.v.copy_(u)                           # out aliases u: refilled before each call
            lib_call("segclip_gumbel_from_uniform", fo.p, fo.p, n)
    else:
        def call():
            lib_call("segclip_gumbel_from_uniform", fu.p, fo.p, n)
    run_twice(name, call, [fo])
    assert fu.intact() and same(fu.v, u)
    ref = gumbel_expr(u, F64)
    judge("gumbel", name, fo.v, ref, gumbel_expr(u, F32) if measuring() else None)
    if n >= 4:
        assert not bool(gumbel_expr(u, F64, low=None).isfinite().all()), "without the clamp the end points 0 and 1 give -inf and inf"
        rejects("gumbel", f"{name}: the lower clamp at FLT_EPSILON", fo.v, gumbel_expr(u, F64, low=FLT_EPS))
        rejects("gumbel", f"{name}: the last element from its neighbour", fo.v, neighbour(ref))


# ---- im2col ---------------------------------------------------------------------------------------------------------------------
def pad128(k):
    return (k + 127) // 128 * 128


# (p, H, W, ld as a function of kdim)
IM_GEOM = ([(p, H, W, f) for p, H, W in ((8, 16, 24), (16, 32, 48)) for f in ("k", "k+8", "k+4")] +
           [(14, 28, 42, "k"), (14, 28, 42, "pad128"), (4, 8, 12, "k")])
IM_CASES = [(lay, od, C, B) + g for lay in (0, 1) for od in (F32, BF) for C in (1, 3) for B in (1, 3) for g in IM_GEOM]
IM_BIG = [(0, BF, 3, 8, 16, 224, 224, "k"), (1, F32, 3, 8, 16, 224, 224, "k"), (0, BF, 3, 56, 16, 224, 224, "k")]


def im_ld(kdim, f):
    return {"k": kdim, "k+8": kdim + 8, "k+4": kdim + 4, "pad128": pad128(kdim)}[f]


def im2col_route(layout, p, ld, W):
    """segclip_im2col_ld's choice (the frames are 16-byte aligned)"""
    return "vec8" if layout == 0 and p % 8 == 0 and ld % 8 == 0 and W % 4 == 0 else "scalar"


def im2col_threads(layout, B, C, H, W, p, ld):
    total = B * (H // p) * (W // p) * ld
    return total // 8 if im2col_route(layout, p, ld, W) == "vec8" else total


def im2col_ref(img, p, layout, swap_grid=False, swap_pixel=False):
    B, C, H, W = img.shape
    gh, gw = H // p, W // p
    if layout == 0:
        r = Fn.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(B, gh, gw, C, p, p)   # col = c p p + py p + px
        r = r.transpose(4, 5) if swap_pixel else r
    else:
        r = torch.einsum("nchpwq->nhwpqc", img.reshape(B, C, gh, p, gw, p))                         # col = (py p + px) C + c
        r = r.transpose(3, 4) if swap_pixel else r
    r = r.transpose(1, 2) if swap_grid else r
    return r.reshape(B * gh * gw, C * p * p)


def im_id(c):
    lay, od, C, B, p, H, W, f = c
    return f"im2col_l{lay}_{tag(od)}_c{C}_b{B}_p{p}_{H}x{W}_{f}"


@pytest.mark.parametrize("case", IM_CASES + IM_BIG, ids=[im_id(c) for c in IM_CASES + IM_BIG])
def test_im2col(case):
    layout, od, C, B, p, H, W, f = case
    name = im_id(case)
    kdim = C * p * p
    ld = im_ld(kdim, f)
    rows = B * (H // p) * (W // p)
    img = draw(seeded(name), B, C, H, W)
    fi, fc = put(img), Frame((rows, ld), od)
    assert fi.v.data_ptr() % 16 == 0 and fc.v.data_ptr() % 16 == 0
    if f == "k":
        def call():
            lib_call("segclip_im2col", fi.p, fc.p, B, C, H, W, p, layout, code(od))
    else:
        def call():
            lib_call("segclip_im2col_ld", fi.p, fc.p, B, C, H, W, p, layout, code(od), ld)
    run_twice(name, call, [fc])
    assert fi.intact()
    ref = im2col_ref(img, p, layout)
    exact(name, fc.v[:, :kdim], ref.to(od))
    assert bool((ibits(fc.v[:, kdim:]) == 0).all()), f"{name}: the pad columns are not +0"
    differs(f"{name}: gh and gw swapped", fc.v[:, :kdim], im2col_ref(img, p, layout, swap_grid=True))
    differs(f"{name}: py and px swapped", fc.v[:, :kdim], im2col_ref(img, p, layout, swap_pixel=True))
    if ld > kdim:
        full = torch.cat([ref.to(od), torch.zeros(rows, ld - kdim, dtype=od, device=DEV)], 1)
        exact(name + " with its pad", fc.v, full)
        full[-1, -1] = float("nan")
        differs(f"{name}: a pad column unwritten", fc.v, full)


@pytest.mark.parametrize("what", ["H_not_divisible", "W_not_divisible", "ld_short"])
def test_im2col_refuses(what):
    B, C, p = 2, 3, 8
    H, W, ld = {"H_not_divisible": (20, 24, 192), "W_not_divisible": (16, 28, 192), "ld_short": (16, 24, 184)}[what]
    fi, fc = put(draw(seeded("im2col_gate"), B, C, H, W)), Frame((B * 2 * 3, 200), BF)
    refused("segclip_im2col_ld", fi.p, fc.p, B, C, H, W, p, 0, L.BF16, ld)
    if what != "ld_short":
        refused("segclip_im2col", fi.p, fc.p, B, C, H, W, p, 0, L.BF16)
    assert fc.untouched() and fi.intact()


# ---- vision assembly --------------------------------------------------------------------------------------------------------------
VA_CASES = [(B, T, D, pd) for B in (1, 3) for T in (1, 4, 49) for D in (4, 65, 768) for pd in (F32, BF)] + [(8, 196, 768, F32), (8, 196, 768, BF)]


def assemble_expr(patches, cls, pos, dt, shift_pos=False):
    B, T, D = patches.shape
    x = torch.cat([cls.to(dt).expand(B, 1, D), patches.to(dt)], 1)
    return x + (pos.roll(1, 0) if shift_pos else pos).to(dt)


@pytest.mark.parametrize("B,T,D,pd", VA_CASES, ids=[f"assemble_b{B}_t{T}_d{D}_{tag(pd)}" for B, T, D, pd in VA_CASES])
def test_vis_assemble(B, T, D, pd):
    name = f"assemble_b{B}_t{T}_d{D}_{tag(pd)}"
    gen = seeded(name)
    patches, cls, pos = draw(gen, B, T, D, dtype=pd), draw(gen, D), draw(gen, T + 1, D, scale=0.5)
    fp, fc, fq, fx = put(patches), put(cls), put(pos), Frame((B, T + 1, D), F32)
    run_twice(name, lambda: lib_call("segclip_vis_assemble", fp.p, fc.p, fq.p, fx.p, B, T, D, code(pd)), [fx])
    assert fp.intact() and fc.intact() and fq.intact()
    want = assemble_expr(patches, cls, pos, F32)
    exact(name, fx.v, want)
    exact(name + ": the CLS row", fx.v[:, 0], (cls + pos[0]).expand(B, D))
    judge("assemble", name, fx.v, assemble_expr(patches, cls, pos, F64), rtol=RT_ONE)
    differs(f"{name}: pos[t - 1] for pos[t]", fx.v, assemble_expr(patches, cls, pos, F32, shift_pos=True))
    rejects("assemble", f"{name}: pos[t - 1] for pos[t]", fx.v, assemble_expr(patches, cls, pos, F64, shift_pos=True), rtol=RT_ONE)


# ---- text embedding ---------------------------------------------------------------------------------------------------------------
VOCAB = 50
EMB_LD = [(Lq, D) for Lq in (1, 5, 77) for D in (4, 64, 260, 512)]
EMB_FWD_CASES = [(5, Lq, D) for Lq, D in EMB_LD] + [(110, 77, 512)]
EMB_BWD_B = (1, 3, 4, 5, 8, 9)
EMB_BWD_CASES = [(B, Lq, D) for B in EMB_BWD_B for Lq, D in EMB_LD] + [(27, 77, 512)]


def emb_ids(gen, B, Lq):
    """random ids; where there is room, 0, V - 1 and the out-of-range -3 and V + 5"""
    ids = torch.randint(0, VOCAB, (B, Lq), generator=gen)
    flat = ids.view(-1)
    plant = torch.tensor([-3, VOCAB + 5, 0, VOCAB - 1])[:min(4, flat.numel())]
    flat[:plant.numel()] = plant
    return ids.to(DEV)


def clamp_ids(ids):
    return ids.clamp(0, VOCAB - 1)


@pytest.mark.parametrize("B,Lq,D", EMB_FWD_CASES, ids=[f"embf_b{B}_l{Lq}_d{D}" for B, Lq, D in EMB_FWD_CASES])
def test_embed_fwd(B, Lq, D):
    name = f"embf_b{B}_l{Lq}_d{D}"
    gen = seeded(name)
    ids, table, pos = emb_ids(gen, B, Lq), draw(gen, VOCAB, D), draw(gen, Lq + 3, D, scale=0.5)
    fi, ft, fp, fo = put(ids), put(table), put(pos), Frame((B, Lq, D), F32)
    run_twice(name, lambda: lib_call("segclip_embed_fwd", fi.p, ft.p, fp.p, fo.p, B, Lq, D, VOCAB), [fo])
    assert fi.intact() and ft.intact() and fp.intact()
    want = table[clamp_ids(ids)] + pos[:Lq]
    exact(name, fo.v, want)
    judge("embed.out", name, fo.v, table.double()[clamp_ids(ids)] + pos.double()[:Lq], rtol=RT_ONE)
    exact(name + ": id -3 reads row 0", fo.v[0, 0], table[0] + pos[0])
    if Lq >= 2:
        exact(name + ": id V + 5 reads row V - 1", fo.v[0, 1], table[VOCAB - 1] + pos[1])
    differs(f"{name}: the clamp removed", fo.v, table[ids.remainder(VOCAB)] + pos[:Lq])
    differs(f"{name}: pos[t - 1] for pos[t]", fo.v, table[clamp_ids(ids)] + pos.roll(1, 0)[:Lq])
    rejects("embed.out", f"{name}: pos[t - 1] for pos[t]", fo.v, table.double()[clamp_ids(ids)] + pos.double().roll(1, 0)[:Lq], rtol=RT_ONE)


def emb_bwd_expr(ids, dout, dt, keep=None):
    B, Lq, D = dout.shape
    d = dout.to(dt)
    rows = d.reshape(-1, D) if keep is None else d.reshape(-1, D) * keep.reshape(-1, 1).to(dt)
    dtable = torch.zeros(VOCAB, D, dtype=dt, device=DEV).index_add_(0, clamp_ids(ids).reshape(-1), rows)
    return dtable, d.sum(0)


def emb_caption_ids(gen, B, Lq):
    """captions: up to three body tokens, an "EOT" (V - 1), then the pad id 0; -> ids, the EOT position per sample"""
    ids = torch.zeros(B, Lq, dtype=I64)
    eot = torch.zeros(B, dtype=I64)
    for b in range(B):
        body = min(Lq - 1, 1 + b % 3)
        ids[b, :body] = torch.randint(1, VOCAB - 1, (body,), generator=gen)
        ids[b, body] = VOCAB - 1
        eot[b] = body
    return ids.to(DEV), eot


@pytest.mark.parametrize("B,Lq,D", EMB_BWD_CASES, ids=[f"embb_b{B}_l{Lq}_d{D}" for B, Lq, D in EMB_BWD_CASES])
def test_embed_bwd(B, Lq, D):
    name = f"embb_b{B}_l{Lq}_d{D}"
    gen = seeded(name)
    # (a) small integers, most ids the pad id: every sum is exact in any order
    ids, _ = emb_caption_ids(gen, B, Lq)
    dout = torch.randint(-4, 5, (B, Lq, D), generator=gen).float().to(DEV)
    fi, fg = put(ids), put(dout)
    ft, fp = Frame((VOCAB, D), F32), Frame((Lq, D), F32)

    def both():
        ft.v.zero_()                                # the caller zero-initialises the table gradient: refilled before each call
        lib_call("segclip_embed_bwd", fi.p, fg.p, ft.p, fp.p, B, Lq, D, VOCAB)
    run_twice(name + " (a)", both, [ft, fp])
    assert fi.intact() and fg.intact()
    rt, rp = emb_bwd_expr(ids, dout, F64)
    exact(name + " (a): dtable", ft.v, rt.float())
    exact(name + " (a): dpos", fp.v, rp.float())
    # (b) Gaussian with exact zeros of both signs behind the EOT, ids with the out-of-range values
    ids = emb_ids(gen, B, Lq)
    dout = draw(gen, B, Lq, D)
    cut = 1 + torch.randint(0, Lq, (B,), generator=gen)
    for b in range(B):
        dout[b, int(cut[b]):] = 0.0
        dout[b, int(cut[b]):, 1::2] = -0.0
    fi, fg = put(ids), put(dout)
    rt, rp = emb_bwd_expr(ids, dout, F64)
    t32, p32 = emb_bwd_expr(ids, dout, F32) if measuring() else (None, None)
    ft = Frame((VOCAB, D), F32)
    for trip in (0, 1):                             # float atomics: each call by the bound, not by its bits
        ft.v.zero_()
        lib_call("segclip_embed_bwd", fi.p, fg.p, ft.p, None, B, Lq, D, VOCAB)
        sync()
        assert ft.intact() and ft.finite()
        judge("embed.dtable", f"{name} (b): dtable, call {trip}", ft.v, rt, t32)
    fp = Frame((Lq, D), F32)
    run_twice(name + " (b) dpos alone", lambda: lib_call("segclip_embed_bwd", fi.p, fg.p, None, fp.p, B, Lq, D, VOCAB), [fp])
    judge("embed.dpos", f"{name} (b): dpos", fp.v, rp, p32)
    assert fi.intact() and fg.intact() and ft.intact()
    first = torch.ones(B, Lq, device=DEV)
    first[0, 0] = 0                                 # (sample 0's first token is never behind its EOT)
    rejects("embed.dtable", f"{name}: a nonzero value skipped", ft.v, emb_bwd_expr(ids, dout, F64, keep=first)[0])
    wrong = torch.zeros(VOCAB, D, dtype=F64, device=DEV).index_add_(0, ids.remainder(VOCAB).reshape(-1), dout.double().reshape(-1, D))
    rejects("embed.dtable", f"{name}: the clamp removed", ft.v, wrong)
    if B >= 2:
        rejects("embed.dpos", f"{name}: the last sample left out", fp.v, rp - dout[-1].double())


def test_embed_bwd_refuses_d_not_multiple_of_4():
    B, Lq, D = 3, 5, 6
    gen = seeded("embb_gate")
    fi, fg = put(emb_ids(gen, B, Lq)), put(draw(gen, B, Lq, D))
    ft, fp = Frame((VOCAB, D), F32), Frame((Lq, D), F32)
    refused("segclip_embed_bwd", fi.p, fg.p, ft.p, fp.p, B, Lq, D, VOCAB)
    assert ft.untouched() and fp.untouched() and fi.intact() and fg.intact()
    ft.v.zero_()
    lib_call("segclip_embed_bwd", fi.p, fg.p, ft.p, None, B, Lq, D, VOCAB)      # the table kernel alone takes any D
    sync()
    judge("embed.dtable", "embb_gate: dtable at D = 6", ft.v, emb_bwd_expr(fi.v, fg.v, F64)[0])
    assert ft.intact() and fp.untouched()


# ---- row gather / scatter -----------------------------------------------------------------------------------------------------------
GS_CASES = sorted({(dt == BF, B, Ts, To, D) for dt in (F32, BF) for B in (1, 3) for Ts in (1, 16, 197) for To in (1, 7, Ts)
                   for D in (1, 3, 64, 513)}) + [(False, 11, 197, 197, 513)]


def gs_id(c):
    return f"rows_{'bf16' if c[0] else 'f32'}_b{c[1]}_ts{c[2]}_to{c[3]}_d{c[4]}"


@pytest.mark.parametrize("case", GS_CASES, ids=[gs_id(c) for c in GS_CASES])
def test_gather_scatter_rows(case):
    isbf, B, Ts, To, D = case
    dt = BF if isbf else F32
    name = gs_id(case)
    gen = seeded(name)
    src = draw(gen, B, Ts, D, dtype=dt)
    idx = torch.randint(0, Ts, (B, To), generator=gen).to(DEV)
    fs, fi, fo = put(src), put(idx), Frame((B, To, D), dt)
    run_twice(name + " gather", lambda: lib_call("segclip_gather_rows", fs.p, fi.p, fo.p, B, Ts, To, D, code(dt)), [fo])
    assert fs.intact() and fi.intact()
    pick = idx[:, :, None].expand(B, To, D)
    exact(name + " gather", fo.v, src.gather(1, pick))
    if To >= 2:                                     # the indices -1 and Ts + 3 read rows 0 and Ts - 1
        odd = idx.clone()
        odd[:, 0], odd[:, -1] = -1, Ts + 3
        fi2 = put(odd)
        run_twice(name + " gather, clamped", lambda: lib_call("segclip_gather_rows", fs.p, fi2.p, fo.p, B, Ts, To, D, code(dt)), [fo])
        exact(name + " gather, clamped", fo.v, src.gather(1, odd.clamp(0, Ts - 1)[:, :, None].expand(B, To, D)))
        exact(name + ": -1 reads row 0", fo.v[:, 0], src[:, 0])
        exact(name + ": Ts + 3 reads row Ts - 1", fo.v[:, -1], src[:, Ts - 1])
        if Ts >= 16:
            differs(f"{name}: the clamp removed", fo.v, src.gather(1, odd.remainder(Ts)[:, :, None].expand(B, To, D)))
    if To > Ts:
        return                                      # a scatter needs unique indices: its rows are those with To <= Ts
    uniq = torch.stack([torch.randperm(Ts, generator=gen)[:To] for _ in range(B)]).to(DEV)
    dout, pre = draw(gen, B, To, D, dtype=dt), draw(gen, B, Ts, D, dtype=dt, scale=2.0)
    fu, fg, fd = put(uniq), put(dout), Frame((B, Ts, D), dt)

    def scatter():
        fd.v.copy_(pre)                             # the call accumulates: the same nonzero prefill before each call
        lib_call("segclip_scatter_rows", fg.p, fu.p, fd.p, B, Ts, To, D, code(dt))
    run_twice(name + " scatter", scatter, [fd])
    assert fu.intact() and fg.intact()
    spread = torch.zeros(B, Ts, D, dtype=F32, device=DEV).scatter_(1, uniq[:, :, None].expand(B, To, D), dout.float())
    named = torch.zeros(B, Ts, device=DEV).scatter_(1, uniq, 1.0) > 0
    want = torch.where(named[:, :, None], (pre.float() + spread).to(dt), pre)      # one rounded add (bf16: the fp32 sum rounded once)
    exact(name + " scatter", fd.v, want)
    exact(name + " scatter: the rows no index names", fd.v[~named], pre[~named])
    judge("scatter", name + " scatter", fd.v, pre.double() + spread.double(), rtol=RT_ONE if dt == F32 else RT_BF)
    differs(f"{name}: the prefill dropped", fd.v, spread)
    rejects("scatter", f"{name}: the prefill dropped", fd.v, spread.double(), rtol=RT_ONE if dt == F32 else RT_BF)


# ---- mean_cat -----------------------------------------------------------------------------------------------------------------------
MC_CASES = [(B, T, D) for B in (1, 3) for T in (1, 2, 7, 49, 196) for D in (4, 36, 256, 260, 768, 1024)] + [(28, 196, 768)]


@pytest.mark.parametrize("B,T,D", MC_CASES, ids=[f"meancat_b{B}_t{T}_d{D}" for B, T, D in MC_CASES])
def test_mean_cat(B, T, D):
    name = f"meancat_b{B}_t{T}_d{D}"
    gen = seeded(name)
    x, dout = draw(gen, B, T, D), draw(gen, B, T + 1, D)
    fx, fg = put(x), put(dout)
    fo, fd = Frame((B, T + 1, D), F32), Frame((B, T, D), F32)
    run_twice(name + " fwd", lambda: lib_call("segclip_mean_cat_fwd", fx.p, fo.p, B, T, D), [fo])
    run_twice(name + " bwd", lambda: lib_call("segclip_mean_cat_bwd", fg.p, fd.p, B, T, D), [fd])
    assert fx.intact() and fg.intact()
    exact(name + ": rows 1..T", fo.v[:, 1:], x)
    if T == 1:
        exact(name + ": the mean of one token", fo.v[:, 0], x[:, 0])
    ref = x.double().mean(1)
    judge("meancat.mean", name + ": mean", fo.v[:, 0], ref, x.mean(1) if measuring() else None)
    dref = dout.double()[:, 1:] + dout.double()[:, :1] / T
    judge("meancat.dx", name + ": dx", fd.v, dref, (dout[:, 1:] + dout[:, :1] / T) if measuring() else None)
    rejects("meancat.mean", f"{name}: the mean over T + 1", fo.v[:, 0], x.double().sum(1) / (T + 1))
    rejects("meancat.dx", f"{name}: the mean's share over T + 1", fd.v, dout.double()[:, 1:] + dout.double()[:, :1] / (T + 1))
    if T >= 2:
        rejects("meancat.mean", f"{name}: the last token left out", fo.v[:, 0], x.double()[:, :-1].sum(1) / T)


# ---- mae_unshuffle ----------------------------------------------------------------------------------------------------------------
MAE_CASES = sorted({(B, K, Lq, D) for B in (1, 3, 7, 8, 9, 16, 17) for Lq in (1, 4, 77, 197) for K in (1, Lq // 4, Lq)
                    for D in (4, 8, 260, 384, 1024)}) + [(22, 49, 197, 1024)]


def perms(gen, B, Lq):
    return torch.stack([torch.randperm(Lq, generator=gen) for _ in range(B)]).to(DEV)


@pytest.mark.parametrize("B,K,Lq,D", MAE_CASES, ids=[f"mae_b{B}_k{K}_l{Lq}_d{D}" for B, K, Lq, D in MAE_CASES])
def test_mae_unshuffle(B, K, Lq, D):
    name = f"mae_b{B}_k{K}_l{Lq}_d{D}"
    gen = seeded(name)
    x, tok, pos, ids = draw(gen, B, K, D), draw(gen, D), draw(gen, Lq, D, scale=0.5), perms(gen, B, Lq)
    dout = draw(gen, B, Lq, D)
    fx, ft, fp, fi, fg = put(x), put(tok), put(pos), put(ids), put(dout)
    fo = Frame((B, Lq, D), F32)
    run_twice(name + " fwd", lambda: lib_call("segclip_mae_unshuffle_fwd", fx.p, ft.p, fi.p, fp.p, fo.p, B, K, Lq, D), [fo])
    pick = ids[:, :, None].expand(B, Lq, D)
    full = torch.cat([x, tok.expand(B, Lq - K, D)], 1)
    exact(name + " fwd", fo.v, full.gather(1, pick) + pos)
    kept = ids < K
    if K < Lq:
        wrong = torch.cat([x, tok.expand(B, Lq - K, D)], 1)
        edge = (ids == K)[:, :, None].expand(B, Lq, D)      # id <= K: the token K would be read from x, not from the mask token
        differs(f"{name}: id <= K for id < K", fo.v, torch.where(edge, torch.zeros_like(wrong), wrong.gather(1, pick)) + pos)
    fdx, fdp, fm = Frame((B, K, D), F32), Frame((Lq, D), F32), Frame((Lq, D), F32)
    run_twice(name + " bwd", lambda: lib_call("segclip_mae_unshuffle_bwd", fg.p, fi.p, fdx.p, fdp.p, fm.p, B, K, Lq, D), [fdx, fdp, fm])
    assert all(f.intact() for f in (fx, ft, fp, fi, fg))
    inv = ids.argsort(1)                            # inv[b][id] = j
    exact(name + ": dx", fdx.v, dout.gather(1, inv[:, :K, None].expand(B, K, D)))
    g64 = dout.double()
    masked = (~kept)[:, :, None].to(F64)
    rdp, rm = g64.sum(0), (g64 * masked).sum(0)
    judge("mae.dpos", name + ": dpos", fdp.v, rdp, dout.sum(0) if measuring() else None)
    if K == Lq:
        assert bool((fm.v == 0).all()), f"{name}: mpart without a mask token must be exactly 0"
    else:
        judge("mae.mpart", name + ": mpart", fm.v, rm, (dout * masked.float()).sum(0) if measuring() else None)
        judge("mae.mpart", name + ": the mask token's gradient", fm.v.double().sum(0), rm.sum(0))
        rejects("mae.mpart", f"{name}: id <= K for id < K", fm.v, (g64 * (ids > K)[:, :, None].to(F64)).sum(0))
    if B > 8:
        rejects("mae.dpos", f"{name}: sample 8 dropped", fdp.v, rdp - g64[8])
    elif B >= 2:
        rejects("mae.dpos", f"{name}: the last sample dropped", fdp.v, rdp - g64[-1])


# ---- MAE masking sort -----------------------------------------------------------------------------------------------------------
NOISES = ("uniform", "levels", "equal", "max_first")
MS_CASES = sorted({(B, Lq, keep, kind) for B in (1, 6) for Lq in (1, 2, 255, 256, 257, 4096) for keep in (0, 1, Lq // 4, Lq) for kind in NOISES})


def ms_noise(gen, kind, B, Lq):
    u = torch.rand(B, Lq, generator=gen)
    if kind == "levels":
        u = torch.floor(u * 8) / 8
    elif kind == "equal":
        u = torch.full((B, Lq), 0.5)
    elif kind == "max_first":
        u[:, 0] = 2.0
    return u


def ms_expr(noise, keep, force=True, high_wins=False):
    """host: a stable sort with column 0 set to -1 -> ids_shuffle, ids_restore, mask"""
    n = noise.clone()
    Lq = n.shape[1]
    if force:
        n[:, 0] = -1.0
    if high_wins:
        shuffle = Lq - 1 - torch.sort(n.flip(1), dim=1, stable=True).indices
    else:
        shuffle = torch.sort(n, dim=1, stable=True).indices
    restore = torch.empty_like(shuffle).scatter_(1, shuffle, torch.arange(Lq).expand_as(shuffle).contiguous())
    return shuffle, restore, (restore >= keep).float()


@pytest.mark.parametrize("B,Lq,keep,kind", MS_CASES, ids=[f"masksort_b{B}_l{Lq}_k{k}_{kind}" for B, Lq, k, kind in MS_CASES])
def test_mask_sort(B, Lq, keep, kind):
    name = f"masksort_b{B}_l{Lq}_k{keep}_{kind}"
    noise = ms_noise(seeded(name), kind, B, Lq)
    fn = put(noise.to(DEV))
    fs, fr, fm = Frame((B, Lq), I64, fill=IDX_FILL_WIDE), Frame((B, Lq), I64, fill=IDX_FILL_WIDE), Frame((B, Lq), F32)
    run_twice(name, lambda: lib_call("segclip_mask_sort", fn.p, fs.p, fr.p, fm.p, B, Lq, keep), [fs, fr, fm])
    assert fn.intact()
    shuffle, restore, mask = ms_expr(noise, keep)
    exact(name + ": ids_shuffle", fs.v.cpu(), shuffle)
    exact(name + ": ids_restore", fr.v.cpu(), restore)
    exact(name + ": mask", fm.v.cpu(), mask)
    assert bool((fs.v[:, 0] == 0).all()), f"{name}: column 0 ranks first"
    if kind in ("levels", "equal") and Lq >= 255:
        differs(f"{name}: ties to the higher index", fs.v.cpu(), ms_expr(noise, keep, high_wins=True)[0])
    if kind == "max_first" and Lq >= 2:
        differs(f"{name}: column 0 not forced first", fs.v.cpu(), ms_expr(noise, keep, force=False)[0])
        if 0 < keep < Lq:
            differs(f"{name}: column 0 not forced first (mask)", fm.v.cpu(), ms_expr(noise, keep, force=False)[2])


def test_mask_sort_refuses_l_4097():
    B, Lq = 2, 4097
    fn = put(torch.rand(B, Lq, generator=seeded("masksort_gate")).to(DEV))
    fs, fr, fm = Frame((B, Lq), I64, fill=IDX_FILL_WIDE), Frame((B, Lq), I64, fill=IDX_FILL_WIDE), Frame((B, Lq), F32)
    refused("segclip_mask_sort", fn.p, fs.p, fr.p, fm.p, B, Lq, 1024)
    assert fs.untouched() and fr.untouched() and fm.untouched() and fn.intact()


# ---- bicubic resample of the positional table -----------------------------------------------------------------------------------
GRIDS = ((7, 7, 7), (14, 14, 14), (14, 32, 32), (16, 37, 23), (14, 7, 5), (14, 1, 1), (1, 3, 3), (2, 5, 3))
INTERP_BIG = (768, 14, 38, 37)                  # 1079808 elements: the grid-stride loop's second trip
INTERP_CASES = [(D, n, h, w) for D in (1, 5, 768) for n, h, w in GRIDS] + [INTERP_BIG]


def cubic_weights(t, A):
    x0, x1, x2, x3 = t + 1, t, 1 - t, 2 - t
    return torch.stack([((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * x1 - (A + 3)) * x1 * x1 + 1,
                        ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1, ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A], -1)


def bicubic(src, h, w, A=-0.75, swap=False, zero_border=False):
    """upsample_bicubic2d(align_corners=False) on a channel-last (n, n, D) table in fp64, with the defects of the list above"""
    n, dev = src.shape[0], src.device
    src = src.double()

    def axis(m, scale):
        f = scale * (torch.arange(m, dtype=F64, device=dev) + 0.5) - 0.5
        i = torch.floor(f)
        wgt = cubic_weights(f - i, A)
        taps = i.long()[:, None] + torch.arange(-1, 3, device=dev)
        if zero_border:
            wgt = wgt * ((taps >= 0) & (taps < n)).double()
        return taps.clamp(0, n - 1), wgt
    sy, sx = (n / w, n / h) if swap else (n / h, n / w)
    iy, wy = axis(h, sy)
    ix, wx = axis(w, sx)
    rows = torch.einsum("ya,yand->ynd", wy, src[iy])              # (h, n, D)
    return torch.einsum("xb,yxbd->yxd", wx, rows[:, ix])          # (h, w, D)


def interp_torch(src, h, w, dt):
    return Fn.interpolate(src.to(dt).permute(2, 0, 1)[None], size=(h, w), mode="bicubic", align_corners=False)[0].permute(1, 2, 0)


@pytest.mark.parametrize("D,n,h,w", INTERP_CASES, ids=[f"interp_d{D}_{n}_to_{h}x{w}" for D, n, h, w in INTERP_CASES])
def test_interp_bicubic(D, n, h, w):
    name = f"interp_d{D}_{n}_to_{h}x{w}"
    src = draw(seeded(name), n, n, D)
    fs, fo = put(src), Frame((h, w, D), F32)
    run_twice(name, lambda: lib_call("segclip_interp_bicubic", fs.p, fo.p, n, h, w, D), [fo])
    assert fs.intact()
    ref = interp_torch(src, h, w, F64)
    assert within(bicubic(src, h, w), ref, 1e-12), f"{name}: the restatement that carries the defects is not torch's bicubic"
    judge("interp", name, fo.v, ref, interp_torch(src, h, w, F32) if measuring() else None)
    if (h, w) == (n, n):
        exact(name + ": the identity", fo.v, src)
        return
    if n >= 2:                                      # (one source point: the weights sum to 1 whatever A is)
        rejects("interp", f"{name}: A = -0.5", fo.v, bicubic(src, h, w, A=-0.5))
    zeroed = bicubic(src, h, w, zero_border=True)
    if not torch.equal(zeroed, bicubic(src, h, w)):  # (14 -> 1 x 1 has no tap beyond the border)
        rejects("interp", f"{name}: border taps zeroed", fo.v, zeroed)
    if h != w:
        rejects("interp", f"{name}: sx and sy swapped", fo.v, bicubic(src, h, w, swap=True))


# ---- multi-tensor cast and add --------------------------------------------------------------------------------------------------
MT_SIZES = (1, 3, 4, 5, 16383, 16384, 16385, 40001, 0)
MT_COUNTS = (1, 32, 33, 36, 37, 70)             # 36 and 37: with every ninth tensor empty, 32 and 33 live tensors
MT_ADD_CASES = [(c, 0) for c in MT_COUNTS] + [(37, 1)]


def mt_sizes(count):
    return [MT_SIZES[i % len(MT_SIZES)] for i in range(count)]


def ptr_array(frames):
    arr = (C.c_void_p * len(frames))(*[f.v.data_ptr() for f in frames])
    return arr, C.cast(arr, C.c_void_p)


def size_array(sizes):
    arr = (C.c_int64 * len(sizes))(*sizes)
    return arr, C.cast(arr, C.c_void_p)


def launches(sizes):
    """csrc/optim.hip: the live tensors in groups of 32 -> the number of launches"""
    return -(-sum(1 for n in sizes if n > 0) // PER_LAUNCH)


@pytest.mark.parametrize("count", MT_COUNTS)
def test_multi_cast_bf16(count):
    name = f"multicast_{count}"
    gen = seeded(name)
    sizes = mt_sizes(count)
    srcs = [put(draw(gen, n, scale=3.0)) for n in sizes]
    for f in srcs:                                   # ties in front of every tensor that has room
        if f.v.numel() >= 4:
            ibits(f.v)[:4] = torch.tensor([0x3f808000, 0x3f818000, 0x3f808001, 0x7f7fffff], dtype=torch.int32, device=DEV)
    dsts = [Frame((n,), BF) for n in sizes]
    keep_s, ps = ptr_array(srcs)
    keep_d, pd = ptr_array(dsts)
    keep_n, pn = size_array(sizes)
    assert all(f.v.data_ptr() % 16 == 0 for f in srcs if f.v.numel()) and all(f.v.data_ptr() % 8 == 0 for f in dsts if f.v.numel())
    run_twice(name, lambda: lib_call("segclip_multi_cast_bf16", ps, pd, pn, count), dsts, finite=False)
    for i, (s, d) in enumerate(zip(srcs, dsts)):
        assert s.intact()
        exact(f"{name}: tensor {i} of {sizes[i]}", d.v, s.v.to(BF))
        if sizes[i] >= 4:
            differs(f"{name}: tensor {i}, truncation", d.v, truncated(s.v))
        if sizes[i] > CHUNK:
            w = s.v.to(BF)
            w[CHUNK] = w[CHUNK - 1]
            differs(f"{name}: tensor {i}, element 16384 from its neighbour", d.v, w)
    if launches(sizes) >= 2:
        first = [i for i, n in enumerate(sizes) if n > 0][PER_LAUNCH]       # the first tensor of the second launch
        differs(f"{name}: tensor {first} left out", dsts[first].v, torch.full_like(dsts[first].v, float("nan")))


def test_multi_cast_refuses_unaligned_source():
    sizes = [8, 8, 8]
    gen = seeded("multicast_gate")
    srcs = [put(draw(gen, 8)), put(draw(gen, 8), shift=1), put(draw(gen, 8))]
    dsts = [Frame((8,), BF) for _ in sizes]
    keep_s, ps = ptr_array(srcs)
    keep_d, pd = ptr_array(dsts)
    keep_n, pn = size_array(sizes)
    assert srcs[1].v.data_ptr() % 16 == 4
    refused("segclip_multi_cast_bf16", ps, pd, pn, 3)
    assert all(d.untouched() for d in dsts) and all(s.intact() for s in srcs)


@pytest.mark.parametrize("count,shift", MT_ADD_CASES, ids=[f"multiadd_{c}_shift{s}" for c, s in MT_ADD_CASES])
def test_multi_add_f32(count, shift):
    name = f"multiadd_{count}_shift{shift}"
    gen = seeded(name)
    sizes = mt_sizes(count)
    srcs = [put(draw(gen, n), shift=shift) for n in sizes]
    pres = [draw(gen, n, scale=2.0) for n in sizes]
    dsts = [Frame((n,), F32, shift=shift) for n in sizes]
    keep_s, ps = ptr_array(srcs)
    keep_d, pd = ptr_array(dsts)
    keep_n, pn = size_array(sizes)
    assert all(f.v.data_ptr() % 16 == 4 * shift for f in srcs + dsts if f.v.numel()), "the frames are not aligned as the row assumes"

    def call():
        for d, pre in zip(dsts, pres):
            d.v.copy_(pre)                          # the call accumulates: the same prefill before each call
        lib_call("segclip_multi_add_f32", pd, ps, pn, count)
    run_twice(name, call, dsts)
    for i, (s, d, pre) in enumerate(zip(srcs, dsts, pres)):
        assert s.intact()
        want = pre + s.v
        exact(f"{name}: tensor {i} of {sizes[i]}", d.v, want)
        if sizes[i] >= 1:
            differs(f"{name}: tensor {i} left out", d.v, pre)
        if sizes[i] > CHUNK:
            w = want.clone()
            w[CHUNK] = w[CHUNK - 1]
            differs(f"{name}: tensor {i}, element 16384 from its neighbour", d.v, w)


# ---- the tables reach every path --------------------------------------------------------------------------------------------------
def test_rows_reach_every_path():
    # cast: the vector body alone, the tail alone, both; a second trip of the grid-stride loop; every value of WALK in some tail
    assert {(n >= 4, n & 3 != 0) for n in CAST_N} == {(False, True), (True, False), (True, True)}
    assert {n & 3 for n in CAST_N} == {0, 1, 2, 3} and sum(n // 4 > GRID_CAP for n in CAST_N) == 1 and CAST_N[-1] & 3 == 3
    assert {(s, d) for s, d, _ in CAST_CASES} == {(F32, BF), (BF, F32), (F32, F32), (BF, BF)}
    tails = [WALK[(TAIL_START[n] + j) % len(WALK)] for n in CAST_N for j in range(n & 3)]
    assert set(tails) == set(WALK) and NAN_BITS in FRONT and set(SPECIALS) <= set(FRONT)
    assert all(len(FRONT) <= n // 4 * 4 for n in CAST_N if n >= 1023) and {0x3f808000, 0x3f818000} <= set(FRONT[:4])
    # split3
    assert {(r, c) for r, c, *_ in SPLIT_CASES} == set(SPLIT_SHAPES) and all(c % 4 == 0 for _, c in SPLIT_SHAPES)
    assert {(p, s, o) for _, _, p, s, o in SPLIT_CASES} == set(itertools.product((0, 12), (0, 1), (0, 1)))
    assert sum(r * c // 4 % 256 != 0 for r, c in SPLIT_SHAPES) == 3 and sum(r * c // 4 > 256 for r, c in SPLIT_SHAPES) == 2
    # activations: every act x type on both sides of the cap; the backward on vec4, scalar by n % 4, scalar by misalignment
    assert {(a, d) for a, d, _ in ACT_FWD_CASES} == set(itertools.product(ACTS, (F32, BF)))
    assert {n for _, _, n in ACT_FWD_CASES} == set(SMALL_N) | {BIG_N} and BIG_N > GRID_CAP
    routes = {("vec4" if n % 4 == 0 and s == 0 else "scalar", "n%4" if n % 4 else ("shift" if s else "aligned"), n // 4 > GRID_CAP) for n, s in ACT_BWD_ROWS}
    assert routes == {("vec4", "aligned", False), ("vec4", "aligned", True), ("scalar", "n%4", False), ("scalar", "shift", False)}
    assert {(a, d) for a, d, _, _ in ACT_BWD_CASES} == set(itertools.product(ACTS, (F32, BF)))
    assert {n for _, n in ADD_CASES} == set(SMALL_N) | {BIG_N} and {d for d, _ in ADD_CASES} == {F32, BF}
    # Gumbel
    assert {n for n, _ in GUMBEL_CASES} == {1, 4, 1025, BIG_N} and sum(a for _, a in GUMBEL_CASES) == 1
    # im2col: both kernels at both layouts' reach, every ld kind, both sides of the cap for each kernel
    seen = set()
    for lay, od, C, B, p, H, W, f in IM_CASES + IM_BIG:
        kdim = C * p * p
        ld = im_ld(kdim, f)
        assert (H != W or B >= 8) and H % p == 0 and W % p == 0 and ld >= kdim     # (only the 224 x 224 rows are square)
        seen.add((im2col_route(lay, p, ld, W), lay, od, im2col_threads(lay, B, C, H, W, p, ld) > GRID_CAP))
        seen.add(("ld", p % 8 == 0, f))
    for od in (F32, BF):
        assert {("vec8", 0, od, False), ("scalar", 0, od, False), ("scalar", 1, od, False)} <= seen
    assert ("vec8", 0, BF, True) in seen and ("scalar", 1, F32, True) in seen
    assert {("ld", True, "k"), ("ld", True, "k+8"), ("ld", True, "k+4"), ("ld", False, "k"), ("ld", False, "pad128")} <= seen
    assert im2col_route(0, 8, 192 + 4, 24) == "scalar" and im2col_route(0, 8, 192 + 8, 24) == "vec8" and pad128(588) == 640
    assert {(C, B) for _, _, C, B, *_ in IM_CASES} == {(1, 1), (1, 3), (3, 1), (3, 3)}
    # assembly, embedding
    va = [c for c in VA_CASES if c[0] * (c[1] + 1) * c[2] <= GRID_CAP]
    assert {c[0] for c in va} == {1, 3} and {c[1] for c in va} == {1, 4, 49} and {c[2] for c in va} == {4, 65, 768}
    assert {c[3] for c in VA_CASES if c[0] * (c[1] + 1) * c[2] > GRID_CAP} == {F32, BF}
    assert sum(B * Lq * D // 4 > GRID_CAP for B, Lq, D in EMB_FWD_CASES) == 1 and {(Lq, D) for _, Lq, D in EMB_FWD_CASES} == set(EMB_LD)
    assert {(B >= 4, B % 4 != 0) for B in EMB_BWD_B} == {(False, True), (True, False), (True, True)}      # the four-in-flight loop, the tail
    assert sum(B * Lq * D > GRID_CAP for B, Lq, D in EMB_BWD_CASES) == 1
    assert {(B, Lq, D) for B, Lq, D in EMB_BWD_CASES if B in EMB_BWD_B} == set(itertools.product(EMB_BWD_B, (1, 5, 77), (4, 64, 260, 512)))
    # gather / scatter
    gs = [c for c in GS_CASES if c[1] * c[3] * c[4] <= GRID_CAP]
    assert {c[0] for c in gs} == {False, True} and {c[1] for c in gs} == {1, 3} and {c[2] for c in gs} == {1, 16, 197}
    assert {c[3] for c in gs} == {1, 7, 16, 197} and {c[4] for c in gs} == {1, 3, 64, 513} and len(GS_CASES) - len(gs) == 1
    assert any(c[3] >= 2 for c in gs) and any(c[3] <= c[2] for c in gs)
    # mean_cat: one and two 64-lane chunks (the second of one lane at D = 260), the backward past the cap
    mc = [c for c in MC_CASES if c[0] * c[1] * c[2] // 4 <= GRID_CAP]
    assert {c[0] for c in mc} == {1, 3} and {c[1] for c in mc} == {1, 2, 7, 49, 196} and {c[2] for c in mc} == {4, 36, 256, 260, 768, 1024}
    assert 260 // 4 == 65 and len(MC_CASES) - len(mc) == 1
    # mae_unshuffle: the eight-in-flight body alone, the tail alone, both; K = L; the forward past the cap
    assert {(B >= 8, B % 8 != 0) for B, *_ in MAE_CASES} == {(False, True), (True, False), (True, True)}
    mae = [c for c in MAE_CASES if c[0] * c[2] * c[3] // 4 <= GRID_CAP]
    assert {c[0] for c in mae} == {1, 3, 7, 8, 9, 16, 17} and {c[2] for c in mae} == {1, 4, 77, 197} and {c[3] for c in mae} == {4, 8, 260, 384, 1024}
    assert any(K == Lq for _, K, Lq, _ in mae) and any(K == 0 for _, K, *_ in mae) and len(MAE_CASES) - len(mae) == 1
    assert all(K <= Lq for _, K, Lq, _ in MAE_CASES)
    # mask_sort
    assert {c[0] for c in MS_CASES} == {1, 6} and {c[1] for c in MS_CASES} == {1, 2, 255, 256, 257, 4096} and {c[3] for c in MS_CASES} == set(NOISES)
    for Lq in (1, 2, 255, 256, 257, 4096):
        assert {c[2] for c in MS_CASES if c[1] == Lq} == {0, 1, Lq // 4, Lq}
    # interp
    assert {(n, h, w) for _, n, h, w in INTERP_CASES} == set(GRIDS) | {INTERP_BIG[1:]} and {D for D, *_ in INTERP_CASES} == {1, 5, 768}
    assert [c for c in INTERP_CASES if c[0] * c[2] * c[3] > GRID_CAP] == [INTERP_BIG]
    assert sum((h, w) == (n, n) for n, h, w in GRIDS) == 2 and any(h > n for n, h, w in GRIDS) and any(h < n for n, h, w in GRIDS)
    # multi-tensor: one launch, exactly 32, a second launch, a third; a skipped tensor; both branches of the add
    live = [sum(n > 0 for n in mt_sizes(c)) for c in MT_COUNTS]
    assert live == [1, 29, 30, 32, 33, 63] and [launches(mt_sizes(c)) for c in MT_COUNTS] == [1, 1, 1, 1, 2, 2]
    assert set(mt_sizes(32)) == set(MT_SIZES) and 0 in mt_sizes(32) and {c for c, _ in MT_ADD_CASES} == set(MT_COUNTS)
    assert {("aligned" if s % 4 == 0 else "unaligned") for _, s in MT_ADD_CASES} == {"aligned", "unaligned"}
    assert any(n % 4 == 0 and n > 0 for n in mt_sizes(37)) and any(n > CHUNK for n in mt_sizes(37)) and (37, 1) in MT_ADD_CASES


# ---- the measurement behind FLOORS -----------------------------------------------------------------------------------------------
def value_rows():
    """(test function, arguments) of every row that judges values by a floor-based bound"""
    rows = [(test_act_fwd, c) for c in ACT_FWD_CASES if c[1] == F32] + [(test_act_bwd, c) for c in ACT_BWD_CASES if c[1] == F32]
    rows += [(test_gumbel, c) for c in GUMBEL_CASES] + [(test_embed_bwd, c) for c in EMB_BWD_CASES]
    rows += [(test_mean_cat, c) for c in MC_CASES] + [(test_mae_unshuffle, c) for c in MAE_CASES]
    rows += [(test_interp_bicubic, c) for c in INTERP_CASES]
    return rows


def floors():
    """every such row once with BOUNDS.stats set: {key: floor of torch float32 against fp64, the kernel's error, the rows they come from}"""
    BOUNDS.stats = {}
    try:
        for fn, args in value_rows():
            fn(*args)
        return {k: v for k, v in BOUNDS.stats.items() if k in FLOORS}
    finally:
        BOUNDS.stats = None
