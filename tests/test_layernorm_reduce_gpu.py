"""GPU: LayerNorm (csrc/layernorm.hip: forward, backward, their row-mapped `_seg` forms, the three-affine `_multi` pair) and the
deterministic column reductions behind it (csrc/reduce_rows.h through segclip_colsum and the LayerNorm backward, the two-stage
column sum and segclip_reduce_multi of csrc/misc.hip), every kernel instance reached by a row of the tables below and checked
against fp64 torch on exactly the fp32 / bf16 values the kernel reads.  All kernel calls go through the C ABI
(segclip_amd._lib), the test owns every buffer (tests/kernel_frames.py, as tests/test_loss_head_gpu.py).

Per row: (1) every output is a view inside a larger NaN buffer: the guards survive and everything inside becomes finite (a
mapped output: the token slice becomes finite, every other row of the buffer is still NaN; a workspace: exactly
`*_ws_bytes` long, the part the mode writes becomes finite); (2) the inputs sit in frames of the same kind, and the rows of a
mapped dy that must not be read hold NaN; (3) the same call a second time into the same frames is bit-identical, frames
included; (4) the values against fp64 with the bound of tests/helpers.check, |err| <= rtol * (|ref| + rms(ref)); (5) the same
bound REJECTS the fp64 reference after a small defect.  A backward reads the mean / rstd its forward kernel wrote; its
reference is the fp64 autograd gradient of F.layer_norm in x, gamma and beta, never of those intermediates.

Rows (test_rows_reach_every_instance restates the coverage; instance_of() restates the dispatchers):
  layernorm_fwd: cols in 4 64 252 256 260 768 1024 1028 1280 1536 1540 1792 2048 (NV = 1 2 3 4 6 8; 1280 is 5 column groups on
      NV 6, 1792 is 7 on NV 8; 252 260 1028 1540 leave the last lane group partly live; 4 is one live lane) x rows in 1 3 4 5 197
      x (x, y) in fp32 | bf16 squared x eps 1e-5 | 1e-6; 4 * 4096 * 2 + 5 rows at cols 4 and 64 (the grid-stride walk past 4096
      workgroups, the last stride ragged: one wave takes a third row, the other waves of its workgroup and all later ones do
      not); mean and rstd are outputs in their own right.
  three input regimes: Gaussian rows (0.1 + 0.05 N(0, 1), the last four columns raised by 0.1: a variance where both eps count);
      hard rows, mean 100 and deviation 0.01 (fp32 x and y; keys *.hard: a one-pass variance would lose every digit); all-equal
      rows (x = 1.7).  The all-equal bound is derived, not measured - fp64 and torch float32 give y = beta exactly, a two-pass
      fp32 kernel need not: the fp32 row sum of `cols` equal values is off by at most cols * 2^-24 * |x| (one rounding per
      addition, each of a partial sum below cols |x|), hence |x - mu| <= cols * 2^-24 * |x|; rstd <= rsqrt(eps); so
      |y - beta| <= cols * 2^-24 * |x| * rsqrt(eps) * |gamma|, plus the final addition's own rounding 2^-23 |beta| (plus 2^-8
      |beta| for a bf16 y).  There rstd is also within 1e-3 relative of rsqrt(eps), and the backward from these statistics is
      finite.
  layernorm_fwd_seg / bwd_seg: (seg_in, seg_out) in (1, 4) (8, 13) x off in 0, interior, seg_out - seg_in, at cols 64 and 768, three
      or five samples; the whole (n * seg_out, cols) output is the NaN frame: rows outside the slice stay NaN; dy holds NaN in
      every row the mapping must not read.
  layernorm_bwd: the 8 (dy, x, dx) type combinations x the 4 (dres, dx_bf16) combinations at cols 64 and 768 (rows 5); every NV
      (the thirteen widths) with dres, dres_colsum and dx_bf16 all present; dres with dres_colsum null; rows 1 3 5 197 and, past
      the cap of 768 workgroups of 4 waves, 3072 + 1, 2 * 3072 + 5 and 3 * 3072 at cols 64 and 2 * 3072 + 5 at 768 (the two-deep
      pipeline with 1, 2 and 3 rows per wave, ragged and even); 1797 rows = 450 partial rows, where the 8-way unrolled loop of
      the second stage starts; dx_bf16 bit-equal to dx rounded; hard and all-equal rows.  Every row once more with dgamma ==
      NULL: the workspace is a frame of exactly segclip_layernorm_bwd_ws_bytes, dbeta and the column sum are not written, the
      third segment of a partial row is written only with dres, and segclip_reduce_multi(ROWS) over it is bit-identical to
      the direct call.  rows == 0: dgamma, dbeta and the column sum exactly 0, nothing else written (dgamma == NULL: the one
      partial row zeroed).
  layernorm_fwd_multi / bwd_multi: cols 768 1024 x fp32 | bf16 y and dy x rows 1 3 197, and 2048 + 1 and 2 * 2048 + 5 at 768 (past
      the 512 workgroups); per row three distinct maps: identity, (T, G + T, G) and (1, 3, 1); unwritten output rows stay NaN,
      unmapped dy rows hold NaN; dgb = [dgamma_0, dbeta_0, dgamma_1, ...]; rows == 0 zeroes dgb; n != 3, cols 512 and bf16 x
      return SEGCLIP_ERR_UNSUPPORTED with every output untouched.
  colsum: the route of every row asserted from colsum_route(), a restatement of the dispatcher.  Single pass (fp32, M <= 4096,
      aligned): M in 0 1 63 64 65 448 449 513 4096 x N in 4 12 16 20 768, ld = N and N + 4; bit-identical to
      segclip_reduce_multi(ROWS) of the same matrix (one summation order, two kernels).  Two stages: bf16 at the same M and N;
      fp32 at M 4097; N in 1 3 77 255 (scalar loads of the last column group, colsum_final_kernel); ld = N + 1 and a base
      offset by one element (scalar loads throughout); M = 65536 + 5, N = 8 (256 chunks of 257 rows: the clamp).  The
      workspace is a frame of exactly segclip_colsum_ws_bytes.
  reduce_multi: SLABS splits in 1 3 4 7 8 9 12 13 21 x width in 4 1020 1024 1028 x scale 1 | 0.37 x fp32 | bf16 out, sixteen
      entries of mixed sizes per launch (the start[] search) and launches of one entry; ROWS rows in 1 63 64 65 448 449 1000 x
      1 2 3 segments of 4 64 768 columns, ld = width and width + 8, out1 / out2 null (their frames untouched), sixteen per launch
      and one; every SEGCLIP_REQUIRE of the function as an error with untouched outputs.
  gates through ops: layer_norm at cols 770 and 2052 raises; layer_norm_multi is None at cols 512; p_colsum of a column slice;
      layer_norm of a (0, 768) input gives zero dgamma and dbeta.

Defects the bound must reject (5):
  y: the mean over cols - 4 columns; eps dropped; gamma of column c - 1
  dx: the c2 * xhat term dropped; c1 divided by cols - 4; dres not added
  dgamma / dbeta / column sums: the last row left out; the last workgroup's partial left out; dgamma and dbeta swapped
  mapped rows: the offset dropped (the slice of sample b at off = 0); for dy, the slice read at off = 0
  multi: the third incoming gradient dropped from dx; gamma_1 used for output 2
  colsum / reduce_multi: the last row or last split left out; the scale dropped; a segment written to the previous output
  (bf16 outputs, bound 2^-8: the two defects of relative size 4 / cols are asked for up to 256 columns only; eps moves these rows
  by 2e-3 at most, below bf16's resolution, and is asked of rstd on every row and of y where y is fp32.)

Bounds.  bf16 outputs: 2^-8, as derived in tests/test_center_stage_gpu.py.  Bit-exact: dx_bf16 against dx, the deferred
against the direct reductions, the single-pass colsum against reduce_multi, the exact zeros.  All-equal rows: derived above.
Every other fp32 output: floor = torch float32 of the same expression on the device (F.layer_norm and its autograd, x.mean /
x.var for the statistics, x.sum(0)) against fp64 in check() units, the maximum over the rows of the kernel; bound = 4 x floor
rounded up to one digit (the 4 covers another summation order over up to 2048 columns, 32773 rows or 768 partial rows).  The
floor never involves the kernel.  Measured on an MI355X by floors() (FLOORS holds the figures; `kernel` is this build's own
error, for the record only):
    key                floor      -> bound    kernel     the floor's row
    ln.mean            8.467e-08 -> 4e-07    8.808e-08  lnf_r197_c1540_f32_f32_eps1e-06
    ln.rstd            7.067e-07 -> 3e-06    9.046e-08  lnf_r32773_c4
    ln.y               1.890e-06 -> 8e-06    1.810e-06  lnf_r32773_c4
    ln.dx              6.113e-07 -> 3e-06    5.098e-07  lnb_r3_c252_f32_f32_f32_res1_dx21_cs1_gauss
    ln.dgamma          1.032e-06 -> 5e-06    4.494e-07  lnb_r3_c252_f32_f32_f32_res1_dx21_cs1_gauss
    ln.dbeta           1.622e-07 -> 7e-07    9.129e-08  lnb_r24_c64_f32_bf16_f32_res1_dx21_cs1_gauss_seg8-13-5
    ln.colsum          4.305e-07 -> 2e-06    3.517e-07  lnb_r6149_c768_bf16_bf16_f32_res1_dx21_cs1_gauss
    ln.mean.hard       7.883e-08 -> 4e-07    4.947e-08  lnf_hard_r5_c768_f32_f32_eps1e-06
    ln.rstd.hard       6.229e-04 -> 0.003    1.711e-06  lnf_hard_r5_c4_f32_f32_eps1e-06
    ln.y.hard          1.582e-03 -> 0.007    2.218e-03  lnf_hard_r5_c768_f32_f32_eps1e-05
    ln.dx.hard         1.384e-03 -> 0.006    4.203e-04  lnb_r5_c768_f32_f32_f32_res1_dx21_cs1_hard
    ln.dgamma.hard     2.373e-03 -> 0.01     5.884e-04  lnb_r5_c768_f32_f32_f32_res1_dx21_cs1_hard
    ln.dbeta.hard      7.636e-08 -> 4e-07    7.636e-08  lnb_r5_c768_f32_f32_f32_res1_dx21_cs1_hard
    ln.colsum.hard     7.911e-08 -> 4e-07    8.713e-08  lnb_r5_c768_f32_f32_f32_res1_dx21_cs1_hard
    lnm.mean           9.155e-08 -> 4e-07    7.650e-08  lnm_r4101_c768_bf16
    lnm.rstd           7.854e-08 -> 4e-07    6.669e-08  lnm_r2049_c768_f32
    lnm.y              4.849e-07 -> 2e-06    4.089e-07  lnm_r2049_c768_f32
    lnm.dx             1.116e-06 -> 5e-06    9.297e-07  lnm_r2049_c768_f32
    lnm.dgamma         1.029e-06 -> 5e-06    4.778e-07  lnm_r2049_c768_f32
    lnm.dbeta          9.116e-08 -> 4e-07    7.601e-08  lnm_r197_c768_f32
    colsum.out         1.627e-07 -> 7e-07    2.559e-07  cs_m4096_n768_ld772_f32
    rm.slabs           1.163e-07 -> 5e-07    1.102e-07  rm_slabs_launch0
    rm.rows            1.226e-07 -> 5e-07    8.433e-08  rm_rows_launch1
  (the bf16 outputs' largest errors, of 2^-8 = 3.91e-03: ln.y_bf16 3.08e-03, ln.dx_bf16 2.95e-03, lnm.y_bf16 3.07e-03, rm.slabs_bf16 2.69e-03)

Fixes that came with this file:
  - segclip_layernorm_bwd / _bwd_seg returned at rows == 0 before the reduction: dgamma, dbeta and the dres column sum were
    never written, and LayerNormFn.backward returned uninitialised parameter gradients for an empty batch.  They are now
    zeroed, as segclip_layernorm_bwd_multi and segclip_colsum do (dgamma == NULL: the one partial row of the workspace).
"""
import ctypes as C
import dataclasses
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from segclip_amd import _lib as L  # noqa: E402
from segclip_amd import ops  # noqa: E402
from tests.kernel_frames import BF, DEV, F32, F64, GUARD, Bounds, Frame, lib_call, put, seeded  # noqa: E402
from tests.helpers import within  # noqa: E402

Fn = torch.nn.functional
RT_BF = 2.0 ** -8
DT = {F32: L.F32, BF: L.BF16}
TN = {F32: "f32", BF: "bf16"}
WAVES = 4
FWD_CAP, BWD_CAP, MULTI_CAP = 4096, 768, 512          # workgroups of 4 waves (BWD_CAP: the cap of ln_blocks, layernorm.hip)
CS_MAXCHUNK = 256

# floors measured by floors() (torch float32 against fp64 on this file's rows, maximum over the rows of the kernel)
FLOORS = {
    "ln.mean": 8.467e-08,
    "ln.rstd": 7.067e-07,
    "ln.y": 1.890e-06,
    "ln.dx": 6.113e-07,
    "ln.dgamma": 1.032e-06,
    "ln.dbeta": 1.622e-07,
    "ln.colsum": 4.305e-07,
    "ln.mean.hard": 7.883e-08,
    "ln.rstd.hard": 6.229e-04,
    "ln.y.hard": 1.582e-03,
    "ln.dx.hard": 1.384e-03,
    "ln.dgamma.hard": 2.373e-03,
    "ln.dbeta.hard": 7.636e-08,
    "ln.colsum.hard": 7.911e-08,
    "lnm.mean": 9.155e-08,
    "lnm.rstd": 7.854e-08,
    "lnm.y": 4.849e-07,
    "lnm.dx": 1.116e-06,
    "lnm.dgamma": 1.029e-06,
    "lnm.dbeta": 9.116e-08,
    "colsum.out": 1.627e-07,
    "rm.slabs": 1.163e-07,
    "rm.rows": 1.226e-07,
}
BOUNDS = Bounds(FLOORS)
RT = BOUNDS.rt
judge, rejects = BOUNDS.judge, BOUNDS.rejects


def measuring():
    return BOUNDS.stats is not None


def cdiv(a, b):
    return -(-a // b)


def f32(v):
    """v as the C function receives it in a float argument"""
    return float(torch.tensor(v, dtype=F32))


def sync():
    torch.cuda.synchronize()


def twice(name, call, outs, partial=()):
    """kernel_frames.run_twice, with frames that a call writes only in part (`partial`: guards and repeatability only)"""
    every = list(outs) + list(partial)
    for f in every:
        f.buf.fill_(f.fill)
    call()
    sync()
    snap = [f.bits() for f in every]
    call()
    sync()
    assert all(torch.equal(a, f.bits()) for a, f in zip(snap, every)), f"{name}: the second call differs"
    for i, f in enumerate(every):
        assert f.intact(), f"{name}: output {i} written outside its view"
    for i, f in enumerate(outs):
        assert f.finite(), f"{name}: output {i} not written everywhere / not finite"


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == BF else torch.int32))


def ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ---- the dispatchers, restated ---------------------------------------------------------------------------------------------------
NV_OF_GROUPS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}
WIDTHS = (4, 64, 252, 256, 260, 768, 1024, 1028, 1280, 1536, 1540, 1792, 2048)
TYPES2 = tuple(itertools.product((F32, BF), repeat=2))
TYPES3 = tuple(itertools.product((F32, BF), repeat=3))
FLAGS2 = tuple(itertools.product((False, True), repeat=2))


def instance_of(cols, dtypes=(), flags=()):
    """the kernel instance ln_fwd_impl / ln_bwd_impl launch: (NV, element types, (HAS_RES, HAS_DX2)); None: refused.  The forward
    takes its types at run time, the backward as template parameters."""
    if cols < 4 or cols % 4 or cols > 8 * 256:
        return None
    return (NV_OF_GROUPS[cdiv(cols // 4, 64)], tuple(TN[d] for d in dtypes), tuple(bool(f) for f in flags))


def multi_instance_of(n, cols, xd, yd):
    """ln_multi_covers and the launch of the two multi functions: (NV, y / dy type); None: SEGCLIP_ERR_UNSUPPORTED"""
    if n != 3 or cols not in (768, 1024) or xd != F32 or yd not in (F32, BF):
        return None
    return (3 if cols == 768 else 4, TN[yd])


def blocks_of(rows, cap):
    return min(max(cdiv(rows, WAVES), 1), cap)


def rows_per_wave(rows, cap):
    """the numbers of rows the waves of a launch walk (a set: {2, 3} is a ragged last stride)"""
    stride = blocks_of(rows, cap) * WAVES
    return {len(range(w, rows, stride)) for w in range(stride)}


def colsum_chunks(M, N):
    c = cdiv(M, 256)
    want, most = cdiv(1024, cdiv(max(N, 1), 256)), cdiv(M, 32)
    if c < want:
        c = min(want, most)
    return min(max(c, 1), CS_MAXCHUNK)


def colsum_route(M, N, ld, dtype, x_addr, ws_addr):
    """segclip_colsum: 'single' (reduce_rows_kernel over X itself) or 'two:<loads>:<second stage>'"""
    if dtype == F32 and M <= 4096 and N % 4 == 0 and ld % 4 == 0 and x_addr % 16 == 0:
        return "single"
    esz = 4 if dtype == F32 else 2
    if ld % 4 == 0 and x_addr % (4 * esz) == 0 and N >= 4:
        loads = "vector" if N % 4 == 0 else "mixed"        # mixed: the last column group has fewer than four columns
    else:
        loads = "scalar"
    return f"two:{loads}:" + ("reduce_rows" if N % 4 == 0 and ws_addr % 16 == 0 else "final")


# ---- inputs and references -------------------------------------------------------------------------------------------------------
REGIMES = ("gauss", "hard", "equal")
EQUAL_X = 1.7


def ln_inputs(gen, rows, cols, xd, regime):
    n = torch.randn(rows, cols, generator=gen, dtype=F64)
    if regime == "gauss":
        x = 0.1 + 0.05 * n
        if cols > 4:
            x[:, -4:] += 0.1
    elif regime == "hard":
        x = 100.0 + 0.01 * n
    else:
        x = torch.full((rows, cols), EQUAL_X, dtype=F64)
    g = 1.0 + 0.2 * torch.randn(cols, generator=gen, dtype=F64)
    b = 0.3 * torch.randn(cols, generator=gen, dtype=F64)
    return x.to(xd).to(DEV), g.float().to(DEV), b.float().to(DEV)


def grads(gen, shape, dtype):
    """incoming gradients with a mean: 0.5 + N(0, 1)"""
    return (0.5 + torch.randn(*shape, generator=gen, dtype=F64)).to(dtype).to(DEV)


def ln_expr(x, g, b, eps, mean_cols=None, no_eps=False, shift_gamma=False):
    """fp64 LayerNorm of the values in x, spelled out (the defects are switches)"""
    x, g, b = x.double(), g.double(), b.double()
    mu = x[:, :mean_cols or x.shape[1]].mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + (0.0 if no_eps else eps)).rsqrt()
    return {"y": (x - mu) * rstd * (g.roll(1) if shift_gamma else g) + b, "mean": mu[:, 0], "rstd": rstd[:, 0]}


def ln_torch(x, g, b, eps, dt, dys=None, dres=None):
    """torch's own LayerNorm in precision dt (fp64: the reference; fp32: the floor), and with dys its autograd gradients.
    g, b: one affine or a list of them (the multi kernels: one x, the outputs' gradients summed into dx)"""
    many = isinstance(g, (list, tuple))
    gs, bs = (g, b) if many else ([g], [b])
    xl = x.detach().to(dt).clone().requires_grad_(dys is not None)
    gl = [t.detach().to(dt).clone().requires_grad_(dys is not None) for t in gs]
    bl = [t.detach().to(dt).clone().requires_grad_(dys is not None) for t in bs]
    ys = [Fn.layer_norm(xl, (x.shape[1],), gk, bk, eps) for gk, bk in zip(gl, bl)]
    xd = xl.detach()
    out = {"y": [y.detach() for y in ys], "mean": xd.mean(-1), "rstd": (xd.var(-1, unbiased=False) + eps).rsqrt()}
    if dys is not None:
        torch.autograd.backward(ys, [d.to(dt) for d in dys])
        out["dx"] = xl.grad if dres is None else xl.grad + dres.to(dt)
        out["dgamma"], out["dbeta"] = [t.grad for t in gl], [t.grad for t in bl]
        if dres is not None:
            out["colsum"] = dres.to(dt).sum(0)
    if not many:
        for k in ("y", "dgamma", "dbeta"):
            if k in out:
                out[k] = out[k][0]
    return out


def ln_bwd_expr(x, g, dy, dres, eps, no_c2=False, c1_cols=None, no_res=False, keep=None):
    """the fp64 LayerNorm backward spelled out (the defects are switches; keep: the rows that enter the column sums)"""
    x, g, dy = x.double(), g.double(), dy.double()
    cols = x.shape[1]
    mu = x.mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = (x - mu) * rstd
    gg = dy * g
    c1 = gg.sum(-1, keepdim=True) / (c1_cols or cols)
    c2 = 0.0 if no_c2 else (gg * xh).mean(-1, keepdim=True)
    dx = rstd * (gg - c1 - xh * c2)
    if dres is not None and not no_res:
        dx = dx + dres.double()
    k = slice(None) if keep is None else keep
    out = {"dx": dx, "dgamma": (dy * xh)[k].sum(0), "dbeta": dy[k].sum(0)}
    if dres is not None:
        out["colsum"] = dres.double()[k].sum(0)
    return out


def outside_last_block(rows, cap):
    """the rows that do NOT belong to the last workgroup of the backward's launch"""
    nb = blocks_of(rows, cap)
    return (torch.arange(rows, device=DEV) // WAVES) % nb != nb - 1


def mapped_rows(n, seg):
    """(n * seg_out,) bool: the rows of the mapped operand that the kernel touches"""
    si, so, off = seg
    live = torch.zeros(n, so, dtype=torch.bool, device=DEV)
    live[:, off:off + si] = True
    return live.view(n * so)


def mapped_frame(dense, live):
    """the (n * seg_out, cols) operand in a frame, NaN in every row outside the mapping"""
    f = put(dense)
    f.v[~live] = float("nan")
    return f


# ---- LayerNorm forward -----------------------------------------------------------------------------------------------------------
def fwd_run(name, x, g, b, eps, yd, seg=None):
    """-> the frames of y, mean, rstd and the (rows, cols) view / gather of the rows of y that belong to x"""
    rows, cols = x.shape
    fx, fg, fb = put(x), put(g), put(b)
    fm, fr = Frame((rows,), F32), Frame((rows,), F32)
    if seg is None:
        fy = Frame((rows, cols), yd)
        twice(name, lambda: lib_call("segclip_layernorm_fwd", fx.p, fg.p, fb.p, fy.p, fm.p, fr.p, rows, cols, eps, DT[x.dtype], DT[yd]),
              [fy, fm, fr])
        ys = fy.v
    else:
        n = rows // seg[0]
        fy = Frame((n * seg[1], cols), yd)
        twice(name, lambda: lib_call("segclip_layernorm_fwd_seg", fx.p, fg.p, fb.p, fy.p, fm.p, fr.p, rows, cols, eps, DT[x.dtype], DT[yd],
                                     *seg), [fm, fr], partial=[fy])
        live = mapped_rows(n, seg)
        assert bool(fy.v[live].isfinite().all()), f"{name}: the slice is not written everywhere"
        assert bool(fy.v[~live].isnan().all()), f"{name}: a row outside the slice was written"
        ys = fy.v[live]
    assert fx.intact() and fg.intact() and fb.intact()
    return fy, fm, fr, ys


def fwd_judge(name, x, g, b, eps, yd, regime, ys, fm, fr, fam="ln"):
    rows, cols = x.shape
    e = f32(eps)
    ref = ln_torch(x, g, b, e, F64)
    if regime == "equal":
        xa = float(x[0, 0].abs())
        dmu = cols * 2.0 ** -24 * xa
        cap = dmu * e ** -0.5 * g.double().abs() + 2.0 ** -23 * b.double().abs() + (RT_BF * b.double().abs() if yd == BF else 0.0)
        assert bool(((ys.double() - b.double()).abs() <= cap).all()), f"{name}: y of an all-equal row beyond the derived bound"
        assert bool(((fm.v.double() - float(x[0, 0])).abs() <= dmu).all()), f"{name}: mean of an all-equal row"
        assert bool(((fr.v.double() * math.sqrt(e) - 1.0).abs() <= 1e-3).all()), f"{name}: rstd of an all-equal row is not rsqrt(eps)"
        return
    sfx = ".hard" if regime == "hard" else ""
    r32 = ln_torch(x.float(), g, b, e, F32) if measuring() else {}
    judge(f"{fam}.mean{sfx}", f"{name}: mean", fm.v, ref["mean"], r32.get("mean"))
    judge(f"{fam}.rstd{sfx}", f"{name}: rstd", fr.v, ref["rstd"], r32.get("rstd"))
    bf = yd == BF
    if bf:
        judge(f"{fam}.y_bf16", f"{name}: y", ys, ref["y"], rtol=RT_BF)
    else:
        judge(f"{fam}.y{sfx}", f"{name}: y", ys, ref["y"], r32.get("y"))
    if regime != "gauss":
        return
    rt = RT_BF if bf else None
    if cols > 4 and (not bf or cols <= 256):
        rejects("ln.y", f"{name}: y, the mean over cols - 4 columns", ys, ln_expr(x, g, b, e, mean_cols=cols - 4)["y"], rtol=rt)
    if not bf:
        rejects("ln.y", f"{name}: y, eps dropped", ys, ln_expr(x, g, b, e, no_eps=True)["y"])
    rejects("ln.rstd", f"{name}: rstd, eps dropped", fr.v, ln_expr(x, g, b, e, no_eps=True)["rstd"])
    rejects("ln.y", f"{name}: y, gamma of column c - 1", ys, ln_expr(x, g, b, e, shift_gamma=True)["y"], rtol=rt)
    assert within(ln_expr(x, g, b, e)["y"], ref["y"], 1e-12), "the spelled-out LayerNorm is torch's"


FWD_ROWS = (1, 3, 4, 5, 197)
FWD_EPS = (1e-5, 1e-6)
FWD_LONG = 4 * FWD_CAP * 2 + 5
FWD_LONG_COLS = (4, 64)


@pytest.mark.parametrize("cols", WIDTHS)
def test_ln_fwd(cols):
    for rows, (xd, yd), eps in itertools.product(FWD_ROWS, TYPES2, FWD_EPS):
        name = f"lnf_r{rows}_c{cols}_{TN[xd]}_{TN[yd]}_eps{eps:g}"
        x, g, b = ln_inputs(seeded(name), rows, cols, xd, "gauss")
        _, fm, fr, ys = fwd_run(name, x, g, b, eps, yd)
        fwd_judge(name, x, g, b, eps, yd, "gauss", ys, fm, fr)


FWD_REGIME_CASES = [(regime, cols, xd, yd, eps) for regime in ("hard", "equal") for cols in (4, 64, 260, 768, 2048)
                    for xd, yd in (TYPES2 if regime == "equal" else TYPES2[:1]) for eps in FWD_EPS]


@pytest.mark.parametrize("regime,cols", [(r, c) for r in ("hard", "equal") for c in (4, 64, 260, 768, 2048)])
def test_ln_fwd_regimes(regime, cols):
    for _, _, xd, yd, eps in [c for c in FWD_REGIME_CASES if c[0] == regime and c[1] == cols]:
        name = f"lnf_{regime}_r5_c{cols}_{TN[xd]}_{TN[yd]}_eps{eps:g}"
        x, g, b = ln_inputs(seeded(name), 5, cols, xd, regime)
        _, fm, fr, ys = fwd_run(name, x, g, b, eps, yd)
        fwd_judge(name, x, g, b, eps, yd, regime, ys, fm, fr)


@pytest.mark.parametrize("cols", FWD_LONG_COLS)
def test_ln_fwd_grid_stride(cols):
    name = f"lnf_r{FWD_LONG}_c{cols}"
    x, g, b = ln_inputs(seeded(name), FWD_LONG, cols, F32, "gauss")
    _, fm, fr, ys = fwd_run(name, x, g, b, 1e-5, F32)
    fwd_judge(name, x, g, b, 1e-5, F32, "gauss", ys, fm, fr)


def seg_cases():
    out = []
    for (si, so), n in (((1, 4), 5), ((8, 13), 3)):
        for off in (0, (so - si) // 2, so - si):
            for cols in (64, 768):
                out.append((n, (si, so, off), cols))
    return out


SEG_CASES = seg_cases()
SEG_IDS = [f"n{n}_in{s[0]}_out{s[1]}_off{s[2]}_c{c}" for n, s, c in SEG_CASES]


def offset_dropped(ys, n, seg, full_shape):
    """the reference's slice placed at off = 0 in an otherwise zero buffer, against the kernel's buffer with NaN as 0"""
    w = torch.zeros(full_shape, dtype=F64, device=DEV)
    w.view(n, seg[1], -1)[:, :seg[0]] = ys.view(n, seg[0], -1)
    return w


@pytest.mark.parametrize("n,seg,cols", SEG_CASES, ids=SEG_IDS)
def test_ln_fwd_seg(n, seg, cols):
    rows = n * seg[0]
    for k, (xd, yd) in enumerate(TYPES2):
        eps = FWD_EPS[k % 2]
        name = f"lnfs_n{n}_{seg}_c{cols}_{TN[xd]}_{TN[yd]}"
        x, g, b = ln_inputs(seeded(name), rows, cols, xd, "gauss")
        fy, fm, fr, ys = fwd_run(name, x, g, b, eps, yd, seg=seg)
        fwd_judge(name, x, g, b, eps, yd, "gauss", ys, fm, fr)
        if seg[2] > 0:
            ref = ln_torch(x, g, b, f32(eps), F64)["y"]
            rejects("ln.y", f"{name}: the offset dropped", fy.v.nan_to_num(0.0), offset_dropped(ref, n, seg, fy.v.shape),
                    rtol=RT_BF if yd == BF else None)


# ---- LayerNorm backward ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class BW:
    rows: int
    cols: int
    types: tuple = (F32, F32, F32)          # dy, x, dx (dres has dx's type)
    res: bool = True
    dx2: bool = True
    colsum: bool = True                     # dres_colsum passed (with res)
    regime: str = "gauss"
    seg: tuple = None                       # (seg_in, seg_out, off) of dy
    eps: float = 1e-5

    @property
    def name(self):
        t = "_".join(TN[d] for d in self.types)
        s = f"_seg{'-'.join(map(str, self.seg))}" if self.seg else ""
        return f"lnb_r{self.rows}_c{self.cols}_{t}_res{int(self.res)}_dx2{int(self.dx2)}_cs{int(self.colsum)}_{self.regime}{s}"


BWD_ROWS = (1, 3, 5, 197)
BWD_WALKS = (BWD_CAP * WAVES + 1, 2 * BWD_CAP * WAVES + 5, 3 * BWD_CAP * WAVES)
BWD_UNROLL = 1797            # 450 partial rows: reduce_rows_kernel's 8-way loop runs for the first row lanes only
BW_TYPES = [BW(5, cols, types=t, res=r, dx2=d, eps=FWD_EPS[i % 2]) for cols in (64, 768)
            for i, (t, (r, d)) in enumerate(itertools.product(TYPES3, FLAGS2))]
BW_WIDTHS = [BW(3, cols) for cols in WIDTHS]
BW_NOSUM = [BW(5, cols, colsum=False) for cols in (64, 768)]
BW_ROWS = [BW(r, 64) for r in BWD_ROWS + BWD_WALKS + (BWD_UNROLL,)] + [BW(BWD_WALKS[1], 768, types=(BF, BF, F32))]
BW_REGIMES = [BW(5, cols, regime=reg) for reg in ("hard", "equal") for cols in (64, 768)] + [BW(5, 768, types=(BF, BF, BF), regime="equal")]
BW_SEG = [BW(n * s[0], cols, seg=s, types=t) for (n, s, cols), t in zip(SEG_CASES, itertools.cycle(TYPES3))]
BW_CASES = BW_TYPES + BW_WIDTHS + BW_NOSUM + BW_ROWS + BW_REGIMES + BW_SEG


def bwd_call(c, fdy, fx, fg, fm, fr, fres, fdx, fdx2, dg, db, cs, fws):
    args = (fdy.p, fx.p, fg.p, fm.p, fr.p, fres.p if fres else None, fdx.p, fdx2.p if fdx2 else None, dg, db, cs, fws.p, c.rows, c.cols,
            *(DT[d] for d in c.types))
    if c.seg is None:
        lib_call("segclip_layernorm_bwd", *args)
    else:
        lib_call("segclip_layernorm_bwd_seg", *args, *c.seg)


def ws_frame(c):
    nbytes = L.load().segclip_layernorm_bwd_ws_bytes(c.rows, c.cols)
    nb = blocks_of(c.rows, BWD_CAP)
    assert nbytes == nb * 3 * c.cols * 4, f"{c.name}: workspace size"
    return Frame((nb * 3 * c.cols,), F32), nb


def ws_written(c, fws, nb):
    """[blocks][dgamma | dbeta | colsum(dres)]: the third segment only with dres"""
    w = fws.v.view(nb, 3, c.cols)
    assert bool(w[:, :2].isfinite().all()), f"{c.name}: a partial row not written"
    assert bool(w[:, 2].isfinite().all() if c.res else w[:, 2].isnan().all()), f"{c.name}: the third segment of the partial rows"


@pytest.mark.parametrize("c", BW_CASES, ids=[c.name for c in BW_CASES])
def test_ln_bwd(c):
    dyd, xd, dxd = c.types
    rows, cols, e = c.rows, c.cols, f32(c.eps)
    gen = seeded(c.name)
    x, g, b = ln_inputs(gen, rows, cols, xd, c.regime)
    fx, fg, fb = put(x), put(g), put(b)
    fy, fm, fr = Frame((rows, cols), F32), Frame((rows,), F32), Frame((rows,), F32)
    lib_call("segclip_layernorm_fwd", fx.p, fg.p, fb.p, fy.p, fm.p, fr.p, rows, cols, c.eps, DT[xd], DT[F32])
    if c.seg is None:
        dy = grads(gen, (rows, cols), dyd)
        fdy, dy_wrong = put(dy), None
    else:
        n = rows // c.seg[0]
        dense, live = grads(gen, (n * c.seg[1], cols), dyd), mapped_rows(n, c.seg)
        fdy, dy = mapped_frame(dense, live), dense[live]
        dy_wrong = dense[mapped_rows(n, (c.seg[0], c.seg[1], 0))]
    dres = torch.randn(rows, cols, generator=gen, dtype=F64).to(dxd).to(DEV) if c.res else None
    fres = put(dres) if c.res else None
    want_cs = c.res and c.colsum
    fdx, fdx2 = Frame((rows, cols), dxd), (Frame((rows, cols), BF) if c.dx2 else None)
    fdg, fdb, fcs = Frame((cols,), F32), Frame((cols,), F32), (Frame((cols,), F32) if want_cs else None)
    fws, nb = ws_frame(c)
    outs = [f for f in (fdx, fdx2, fdg, fdb, fcs) if f is not None]
    twice(c.name, lambda: bwd_call(c, fdy, fx, fg, fm, fr, fres, fdx, fdx2, fdg.p, fdb.p, fcs.p if fcs else None, fws), outs, partial=[fws])
    ws_written(c, fws, nb)
    assert all(f.intact() for f in (fx, fg, fm, fr, fdy) + ((fres,) if fres else ()))
    if c.dx2:
        assert same_bits(fdx2.v, fdx.v.to(BF)), f"{c.name}: dx_bf16 is not dx rounded"

    # dgamma == NULL: the partial rows stay in the workspace, segclip_reduce_multi combines them - bit-identical
    gdx, gdx2 = Frame((rows, cols), dxd), (Frame((rows, cols), BF) if c.dx2 else None)
    gdb, gcs, gws = Frame((cols,), F32), Frame((cols,), F32), ws_frame(c)[0]
    twice(c.name + " dgamma null", lambda: bwd_call(c, fdy, fx, fg, fm, fr, fres, gdx, gdx2, None, gdb.p, gcs.p, gws),
          [f for f in (gdx, gdx2) if f is not None], partial=[gws])
    ws_written(c, gws, nb)
    assert gdb.untouched() and gcs.untouched(), f"{c.name}: dbeta / the column sum written though dgamma is null"
    assert same_bits(gdx.v, fdx.v) and (not c.dx2 or same_bits(gdx2.v, fdx2.v)), f"{c.name}: dx of the deferred call"
    hdg, hdb, hcs = Frame((cols,), F32), Frame((cols,), F32), Frame((cols,), F32)
    ent = rows_entry(gws.v, nb, (3 if want_cs else 2) * cols, 3 * cols, cols, (hdg.v, hdb.v, hcs.v if want_cs else None))
    twice(c.name + " combine", lambda: reduce_call([ent], L.REDUCE_ROWS), [hdg, hdb] + ([hcs] if want_cs else []))
    assert same_bits(hdg.v, fdg.v) and same_bits(hdb.v, fdb.v) and (not want_cs or same_bits(hcs.v, fcs.v)), \
        f"{c.name}: the deferred reduction differs from the direct one"
    assert want_cs or hcs.untouched()

    if c.regime == "equal":
        return                   # finite (asserted above); xhat is rounding noise over sqrt(eps) there
    sfx = ".hard" if c.regime == "hard" else ""
    ref = ln_torch(x, g, b, e, F64, [dy], dres)
    r32 = ln_torch(x.float(), g, b, e, F32, [dy.float()], dres.float() if c.res else None) if measuring() else {}
    got = {"dgamma": fdg.v, "dbeta": fdb.v}
    if want_cs:
        got["colsum"] = fcs.v
    bf = dxd == BF
    if bf:
        judge("ln.dx_bf16", f"{c.name}: dx", fdx.v, ref["dx"], rtol=RT_BF)
    else:
        judge(f"ln.dx{sfx}", f"{c.name}: dx", fdx.v, ref["dx"], r32.get("dx"))
    for k in got:
        judge(f"ln.{k}{sfx}", f"{c.name}: {k}", got[k], ref[k], r32.get(k))
    if c.regime != "gauss":
        return
    spelled = ln_bwd_expr(x, g, dy, dres, e)
    assert all(within(spelled[k], ref[k], 1e-10) for k in spelled), "the spelled-out backward is torch's autograd"
    rt = RT_BF if bf else None
    rejects("ln.dx", f"{c.name}: dx without c2 * xhat", fdx.v, ln_bwd_expr(x, g, dy, dres, e, no_c2=True)["dx"], rtol=rt)
    if cols > 4 and (not bf or cols <= 256):
        rejects("ln.dx", f"{c.name}: dx, c1 over cols - 4", fdx.v, ln_bwd_expr(x, g, dy, dres, e, c1_cols=cols - 4)["dx"], rtol=rt)
    if c.res:
        rejects("ln.dx", f"{c.name}: dx, dres not added", fdx.v, ln_bwd_expr(x, g, dy, dres, e, no_res=True)["dx"], rtol=rt)
    if dy_wrong is not None and c.seg[2] > 0:
        rejects("ln.dx", f"{c.name}: dx, dy read at off = 0", fdx.v, ln_bwd_expr(x, g, dy_wrong, dres, e)["dx"], rtol=rt)
        rejects("ln.dbeta", f"{c.name}: dbeta, dy read at off = 0", fdb.v, ln_bwd_expr(x, g, dy_wrong, dres, e)["dbeta"])
    keep_rows = torch.arange(rows, device=DEV) < rows - 1
    for what, keep in (("the last row left out", keep_rows), ("the last workgroup's partial left out", outside_last_block(rows, BWD_CAP))):
        w = ln_bwd_expr(x, g, dy, dres, e, keep=keep)
        for k in got:
            rejects(f"ln.{k}", f"{c.name}: {k}, {what}", got[k], w[k])
    rejects("ln.dgamma", f"{c.name}: dgamma and dbeta swapped", fdg.v, ref["dbeta"])
    rejects("ln.dbeta", f"{c.name}: dgamma and dbeta swapped", fdb.v, ref["dgamma"])


@pytest.mark.parametrize("c", [BW(0, 768), BW(0, 64, types=(BF, BF, BF)), BW(0, 768, seg=(8, 13, 5)), BW(0, 64, colsum=False)],
                         ids=lambda c: c.name)
def test_ln_bwd_no_rows(c):
    """rows == 0: the sums over no row are exactly 0 and nothing else is written (before this file: nothing was written at all)"""
    dyd, xd, dxd = c.types
    cols = c.cols
    empty = lambda dt: put(torch.zeros(0, cols, dtype=dt, device=DEV))      # noqa: E731
    fdy, fx, fres, fg = empty(dyd), empty(xd), empty(dxd), put(torch.ones(cols, device=DEV))
    fm, fr = Frame((0,), F32), Frame((0,), F32)
    fdx, fdx2 = Frame((0, cols), dxd), Frame((0, cols), BF)
    fdg, fdb, fcs = Frame((cols,), F32), Frame((cols,), F32), Frame((cols,), F32)
    fws, nb = ws_frame(c)
    assert nb == 1
    twice(c.name, lambda: bwd_call(c, fdy, fx, fg, fm, fr, fres, fdx, fdx2, fdg.p, fdb.p, fcs.p if c.colsum else None, fws),
          [fdg, fdb] + ([fcs] if c.colsum else []))
    for f in [fdg, fdb] + ([fcs] if c.colsum else []):
        assert bool((f.v == 0).all())
    assert c.colsum or fcs.untouched()
    assert all(f.untouched() for f in (fdx, fdx2, fws, fm, fr)) and fg.intact()
    for f in (fdg, fdb, fcs):
        f.buf.fill_(f.fill)
    twice(c.name + " dgamma null", lambda: bwd_call(c, fdy, fx, fg, fm, fr, fres, fdx, fdx2, None, fdb.p, fcs.p, fws), [fws])
    assert bool((fws.v == 0).all()) and fdg.untouched() and fdb.untouched() and fcs.untouched() and fdx.untouched() and fdx2.untouched()


# ---- three affine outputs of one normalisation -------------------------------------------------------------------------------------
MULTI_WALKS = (MULTI_CAP * WAVES + 1, 2 * MULTI_CAP * WAVES + 5)
MULTI_T = {1: 1, 3: 3, 197: 197, MULTI_WALKS[0]: 683, MULTI_WALKS[1]: 1367}      # seg_in of the second map: a divisor of rows
MULTI_G = 8
MULTI_CASES = [(rows, cols, yd) for cols in (768, 1024) for yd in (F32, BF) for rows in (1, 3, 197)] + \
              [(rows, 768, yd) for rows, yd in zip(MULTI_WALKS, (F32, BF))]


def multi_maps(rows):
    T = MULTI_T[rows]
    return [None, (T, MULTI_G + T, MULTI_G), (1, 3, 1)]


def flat_maps(maps):
    flat = [v for m in maps for v in (m or (0, 0, 0))]
    return (C.c_int64 * len(flat))(*flat)


def multi_out_rows(rows, m):
    return rows if m is None else rows // m[0] * m[1]


def multi_live(rows, m):
    return torch.ones(rows, dtype=torch.bool, device=DEV) if m is None else mapped_rows(rows // m[0], m)


@pytest.mark.parametrize("rows,cols,yd", MULTI_CASES, ids=[f"lnm_r{r}_c{c}_{TN[y]}" for r, c, y in MULTI_CASES])
def test_ln_multi(rows, cols, yd):
    name = f"lnm_r{rows}_c{cols}_{TN[yd]}"
    gen = seeded(name)
    eps = 1e-5
    e = f32(eps)
    x, g0, b0 = ln_inputs(gen, rows, cols, F32, "gauss")
    gs = [g0] + [(1.0 + 0.2 * torch.randn(cols, generator=gen, dtype=F64)).float().to(DEV) for _ in range(2)]
    bs = [b0] + [(0.3 * torch.randn(cols, generator=gen, dtype=F64)).float().to(DEV) for _ in range(2)]
    maps = multi_maps(rows)
    assert len({m for m in maps}) == 3 and all(m is None or rows % m[0] == 0 for m in maps)
    lives = [multi_live(rows, m) for m in maps]
    fx, fgs, fbs = put(x), [put(t) for t in gs], [put(t) for t in bs]
    fys = [Frame((multi_out_rows(rows, m), cols), yd) for m in maps]
    fm, fr = Frame((rows,), F32), Frame((rows,), F32)
    fmaps = flat_maps(maps)
    twice(name + " fwd", lambda: lib_call("segclip_layernorm_fwd_multi", fx.p, 3, ptrs([f.v for f in fgs]), ptrs([f.v for f in fbs]),
                                          ptrs([f.v for f in fys]), fmaps, fm.p, fr.p, rows, cols, eps, L.F32, DT[yd]), [fm, fr], partial=fys)
    ref = ln_torch(x, gs, bs, e, F64)
    r32 = ln_torch(x, gs, bs, e, F32) if measuring() else {}
    judge("lnm.mean", f"{name}: mean", fm.v, ref["mean"], r32.get("mean"))
    judge("lnm.rstd", f"{name}: rstd", fr.v, ref["rstd"], r32.get("rstd"))
    bf = yd == BF
    rt = RT_BF if bf else None
    for k in range(3):
        assert bool(fys[k].v[lives[k]].isfinite().all()) and bool(fys[k].v[~lives[k]].isnan().all()), f"{name}: the rows of output {k}"
        if bf:
            judge("lnm.y_bf16", f"{name}: y{k}", fys[k].v[lives[k]], ref["y"][k], rtol=RT_BF)
        else:
            judge("lnm.y", f"{name}: y{k}", fys[k].v[lives[k]], ref["y"][k], r32["y"][k] if r32 else None)
        if maps[k] is not None:
            rejects("lnm.y", f"{name}: y{k}, the offset dropped", fys[k].v.nan_to_num(0.0),
                    offset_dropped(ref["y"][k], rows // maps[k][0], maps[k], fys[k].v.shape), rtol=rt)
    rejects("lnm.y", f"{name}: gamma_1 used for output 2", fys[2].v[lives[2]], ln_expr(x, gs[1], bs[2], e)["y"], rtol=rt)

    dense = [grads(gen, (multi_out_rows(rows, m), cols), yd) for m in maps]
    dys = [d[lv] for d, lv in zip(dense, lives)]
    fdys = [mapped_frame(d, lv) for d, lv in zip(dense, lives)]
    nbytes = L.load().segclip_layernorm_bwd_multi_ws_bytes(rows, cols, 3)
    assert nbytes == blocks_of(rows, MULTI_CAP) * 6 * cols * 4
    fdx, fdgb, fws = Frame((rows, cols), F32), Frame((6, cols), F32), Frame((nbytes // 4,), F32)
    twice(name + " bwd", lambda: lib_call("segclip_layernorm_bwd_multi", ptrs([f.v for f in fdys]), fx.p, 3, ptrs([f.v for f in fgs]), fmaps,
                                          fm.p, fr.p, fdx.p, fdgb.p, fws.p, rows, cols, DT[yd], L.F32), [fdx, fdgb, fws])
    assert all(f.intact() for f in [fx, fm, fr] + fgs + fbs + fdys)
    ref = ln_torch(x, gs, bs, e, F64, dys)
    r32 = ln_torch(x, gs, bs, e, F32, [d.float() for d in dys]) if measuring() else {}
    judge("lnm.dx", f"{name}: dx", fdx.v, ref["dx"], r32.get("dx"))
    for k in range(3):
        judge("lnm.dgamma", f"{name}: dgamma_{k} = dgb[{2 * k}]", fdgb.v[2 * k], ref["dgamma"][k], r32["dgamma"][k] if r32 else None)
        judge("lnm.dbeta", f"{name}: dbeta_{k} = dgb[{2 * k + 1}]", fdgb.v[2 * k + 1], ref["dbeta"][k], r32["dbeta"][k] if r32 else None)
        rejects("lnm.dbeta", f"{name}: dgb[{2 * k + 1}] taken for dgamma_{k}", fdgb.v[2 * k + 1], ref["dgamma"][k])
        w = ln_bwd_expr(x, gs[k], dys[k], None, e, keep=torch.arange(rows, device=DEV) < rows - 1)
        rejects("lnm.dgamma", f"{name}: dgamma_{k}, the last row left out", fdgb.v[2 * k], w["dgamma"])
        rejects("lnm.dbeta", f"{name}: dbeta_{k}, the last row left out", fdgb.v[2 * k + 1], w["dbeta"])
    rejects("lnm.dx", f"{name}: dx without the third gradient", fdx.v, ln_torch(x, gs[:2], bs[:2], e, F64, dys[:2])["dx"])
    w = ln_torch(x, gs, bs, e, F64, [dys[0], dense[1][multi_live(rows, (maps[1][0], maps[1][1], 0))], dys[2]])
    rejects("lnm.dx", f"{name}: dx, dy_1 read at off = 0", fdx.v, w["dx"])


def test_ln_multi_no_rows():
    cols = 768
    fx, fgs = put(torch.zeros(0, cols, device=DEV)), [put(torch.ones(cols, device=DEV)) for _ in range(3)]
    fdys = [put(torch.zeros(0, cols, device=DEV)) for _ in range(3)]
    fm, fr, fdx, fdgb = Frame((0,), F32), Frame((0,), F32), Frame((0, cols), F32), Frame((6, cols), F32)
    fws = Frame((L.load().segclip_layernorm_bwd_multi_ws_bytes(0, cols, 3) // 4,), F32)
    twice("lnm rows 0", lambda: lib_call("segclip_layernorm_bwd_multi", ptrs([f.v for f in fdys]), fx.p, 3, ptrs([f.v for f in fgs]),
                                         flat_maps([None, (4, 12, 8), (1, 3, 1)]), fm.p, fr.p, fdx.p, fdgb.p, fws.p, 0, cols, L.F32, L.F32), [fdgb])
    assert bool((fdgb.v == 0).all()) and fdx.untouched() and fws.untouched()


@pytest.mark.parametrize("n,cols,xd,yd", [(2, 768, F32, F32), (4, 768, F32, F32), (3, 512, F32, F32), (3, 768, BF, F32), (3, 1024, BF, BF)],
                         ids=lambda v: TN.get(v, str(v)))
def test_ln_multi_unsupported(n, cols, xd, yd):
    assert multi_instance_of(n, cols, xd, yd) is None
    rows = 5
    gen = seeded(f"lnm_unsupported_{n}_{cols}")
    x, g, b = ln_inputs(gen, rows, cols, xd, "gauss")
    fx, fg, fb = put(x), put(g), put(b)
    fys, fdys = [Frame((rows, cols), yd) for _ in range(n)], [put(grads(gen, (rows, cols), yd)) for _ in range(n)]
    fm, fr, fdx, fdgb = Frame((rows,), F32), Frame((rows,), F32), Frame((rows, cols), F32), Frame((2 * n, cols), F32)
    fws = Frame((blocks_of(rows, MULTI_CAP) * 2 * n * cols,), F32)
    maps = flat_maps([None] * n)
    with pytest.raises(L.Unsupported):
        lib_call("segclip_layernorm_fwd_multi", fx.p, n, ptrs([fg.v] * n), ptrs([fb.v] * n), ptrs([f.v for f in fys]), maps, fm.p, fr.p,
                 rows, cols, 1e-5, DT[xd], DT[yd])
    with pytest.raises(L.Unsupported):
        lib_call("segclip_layernorm_bwd_multi", ptrs([f.v for f in fdys]), fx.p, n, ptrs([fg.v] * n), maps, fm.p, fr.p, fdx.p, fdgb.p,
                 fws.p, rows, cols, DT[yd], DT[xd])
    sync()
    assert all(f.untouched() for f in fys + [fm, fr, fdx, fdgb, fws])


# ---- column sums -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class CS:
    M: int
    N: int
    pad: int                 # ld = N + pad
    dtype: torch.dtype
    route: str
    shift: bool = False      # the base offset by one element

    @property
    def name(self):
        return f"cs_m{self.M}_n{self.N}_ld{self.N + self.pad}_{TN[self.dtype]}{'_shift' if self.shift else ''}"


CS_M = (0, 1, 63, 64, 65, 448, 449, 513, 4096)
CS_N = (4, 12, 16, 20, 768)
CS_ODD_N = (1, 3, 77, 255)
CS_TALL = 65536 + 5
CS_SINGLE = [CS(M, N, pad, F32, "single") for M in CS_M for N in CS_N for pad in (0, 4)]
CS_TWO = ([CS(M, N, pad, BF, "two:vector:reduce_rows") for M in CS_M for N in CS_N for pad in (0, 4)]
          + [CS(4097, N, pad, F32, "two:vector:reduce_rows") for N in CS_N for pad in (0, 4)]
          + [CS(M, N, 4 - N % 4, dt, "two:scalar:final" if N < 4 else "two:mixed:final")     # ld 4, 80, 256: only whole groups are vectors
             for M in (1, 65, 513, 4097) for N in CS_ODD_N[1:] for dt in (F32, BF)]
          + [CS(M, N, 1, dt, "two:mixed:final" if N == 255 else "two:scalar:final")              # ld = N + 1 (256 is a multiple of 4)
             for M in (1, 65, 513, 4097) for N in CS_ODD_N for dt in (F32, BF)]
          + [CS(M, N, 0, dt, "two:scalar:final") for M in (65, 4097) for N in (77, 255) for dt in (F32, BF)]
          + [CS(M, 1, 0, dt, "two:scalar:final") for M in (0, 65) for dt in (F32, BF)]
          + [CS(M, 16, 1, dt, "two:scalar:reduce_rows") for M in (65, 4097) for dt in (F32, BF)]
          + [CS(M, N, 0, dt, "two:scalar:reduce_rows", shift=True) for M in (65, 513) for N in (16, 768) for dt in (F32, BF)]
          + [CS(CS_TALL, 8, 0, dt, "two:vector:reduce_rows") for dt in (F32, BF)])
CS_CASES = CS_SINGLE + CS_TWO


def put_shifted(t, pitch):
    """put(), the view begun one element later (the guard rows behind the view hold the overhang)"""
    f = Frame(t.shape, t.dtype, pitch)
    f.v = f.buf.as_strided(t.shape, (pitch, 1), GUARD + 1)
    f.v.copy_(t)
    f.inside.zero_()
    f.inside.as_strided(t.shape, (pitch, 1), GUARD + 1).fill_(True)
    return f


def cs_row(c):
    M, N, ld = c.M, c.N, c.N + c.pad
    x = (0.5 + torch.randn(M, N, generator=seeded(c.name), dtype=F64)).to(c.dtype).to(DEV)
    fx = put_shifted(x, ld) if c.shift else put(x, ld)
    nchunk = colsum_chunks(M, N)
    assert L.load().segclip_colsum_ws_bytes(M, N) == nchunk * N * 4, f"{c.name}: workspace size"
    fo, fws = Frame((N,), F32), Frame((nchunk * N,), F32)
    assert colsum_route(M, N, ld, c.dtype, fx.v.data_ptr(), fws.v.data_ptr()) == c.route, f"{c.name}: not the route this row is for"
    single = c.route == "single"
    twice(c.name, lambda: lib_call("segclip_colsum", fx.p, fo.p, fws.p, M, N, ld, DT[c.dtype]), [fo] + ([] if single else [fws]))
    assert fx.intact() and (not single or fws.untouched())
    if M == 0:
        assert bool((fo.v == 0).all()), f"{c.name}: the sum over no row"
        return
    ref = x.double().sum(0)
    judge("colsum.out", f"{c.name}: out", fo.v, ref, x.float().sum(0) if measuring() else None)
    rejects("colsum.out", f"{c.name}: the last row left out", fo.v, ref - x[-1].double())
    if single:          # reduce_rows_kernel and reduce_multi_rows_kernel: one summation order
        fo2 = Frame((N,), F32)
        twice(c.name + " as reduce_multi", lambda: reduce_call([rows_entry(fx.v, M, N, ld, N, (fo2.v,))], L.REDUCE_ROWS), [fo2])
        assert same_bits(fo2.v, fo.v), f"{c.name}: reduce_rows and reduce_multi(ROWS) differ"


CS_GROUPS = sorted({(c.route, c.dtype == BF, c.N) for c in CS_CASES}, key=str)


@pytest.mark.parametrize("route,bf,N", CS_GROUPS, ids=[f"{r}_{'bf16' if b else 'f32'}_n{n}" for r, b, n in CS_GROUPS])
def test_colsum(route, bf, N):
    for c in CS_CASES:
        if (c.route, c.dtype == BF, c.N) == (route, bf, N):
            cs_row(c)


# ---- segclip_reduce_multi -----------------------------------------------------------------------------------------------------------
def rows_entry(src, rows, width, ld, seg, outs):
    e = L.ReduceEntry()
    e.src, e.rows, e.width, e.ld, e.seg = L.ptr(src), rows, width, ld, seg
    e.out0, e.out1, e.out2 = (L.ptr(o) for o in (tuple(outs) + (None, None))[:3])
    return e


def slabs_entry(src, out, splits, width, scale):
    e = L.ReduceEntry()
    e.src, e.out0, e.rows, e.width, e.scale = L.ptr(src), L.ptr(out), splits, width, scale
    e.out_dtype = L.F32 if out is None else DT[out.dtype]
    return e


def reduce_call(ents, kind, n=None):
    arr = (L.ReduceEntry * max(len(ents), 1))(*ents)
    lib_call("segclip_reduce_multi", arr, len(ents) if n is None else n, kind)


SLAB_SPLITS = (1, 3, 4, 7, 8, 9, 12, 13, 21)
SLAB_WIDTHS = (4, 1020, 1024, 1028)
SLAB_SCALES = (1.0, 0.37)
SLAB_CASES = list(itertools.product(SLAB_SPLITS, SLAB_WIDTHS, SLAB_SCALES, (F32, BF)))
SLAB_LAUNCHES = [SLAB_CASES[i::9] for i in range(9)] + [[SLAB_CASES[i]] for i in (0, 37, 143)]       # nine of sixteen entries, three of one


@pytest.mark.parametrize("k", range(len(SLAB_LAUNCHES)))
def test_reduce_multi_slabs(k):
    cases = SLAB_LAUNCHES[k]
    name = f"rm_slabs_launch{k}"
    gen = seeded(name)
    srcs = [(0.5 + torch.randn(s, w, generator=gen, dtype=F64)).float().to(DEV) for s, w, _, _ in cases]
    fsrc, fouts = [put(t) for t in srcs], [Frame((w,), od) for _, w, _, od in cases]
    ents = [slabs_entry(f.v, o.v, s, w, sc) for f, o, (s, w, sc, _) in zip(fsrc, fouts, cases)]
    twice(name, lambda: reduce_call(ents, L.REDUCE_SLABS), fouts)
    assert all(f.intact() for f in fsrc)
    assert len(cases) == 1 or len({(s, w) for s, w, _, _ in cases}) > 4, "a launch of mixed sizes"
    for (s, w, sc, od), x, fo in zip(cases, srcs, fouts):
        what = f"{name}: splits {s} width {w} scale {sc} {TN[od]}"
        s32 = f32(sc)
        ref = x.double().sum(0) * s32
        wrong = {"the last split left out": ref - x[-1].double() * s32}
        if sc != 1.0:
            wrong["the scale dropped"] = x.double().sum(0)
        if od == BF:
            judge("rm.slabs_bf16", what, fo.v, ref, rtol=RT_BF)
        else:
            judge("rm.slabs", what, fo.v, ref, (x.sum(0) * s32) if measuring() else None)
        for dname, wv in wrong.items():
            rejects("rm.slabs", f"{what}: {dname}", fo.v, wv, rtol=RT_BF if od == BF else None)


ROWS_ROWS = (1, 63, 64, 65, 448, 449, 1000)
ROWS_SEGS = (4, 64, 768)
ROWS_CASES = [(r, n, sg, 8 * (i % 2), ("all", "no1", "no2", "no12")[i % 4] if n == 3 else "all")       # rows, segments, seg, ld - width, outs
              for i, (r, n, sg) in enumerate(itertools.product(ROWS_ROWS, (1, 2, 3), ROWS_SEGS))]
ROWS_LAUNCHES = [ROWS_CASES[i::4] for i in range(4)] + [[ROWS_CASES[i]] for i in (0, 31, 62)]


@pytest.mark.parametrize("k", range(len(ROWS_LAUNCHES)))
def test_reduce_multi_rows(k):
    cases = ROWS_LAUNCHES[k]
    name = f"rm_rows_launch{k}"
    gen = seeded(name)
    srcs = [(0.5 + torch.randn(r, n * sg, generator=gen, dtype=F64)).float().to(DEV) for r, n, sg, _, _ in cases]
    fsrc = [put(t, t.shape[1] + pad) for t, (_, _, _, pad, _) in zip(srcs, cases)]
    fouts = [[Frame((sg,), F32) for _ in range(3)] for _, _, sg, _, _ in cases]
    ents, live = [], []
    for f, fo, (r, n, sg, pad, nulls) in zip(fsrc, fouts, cases):
        on = [j < n and not (j == 1 and nulls in ("no1", "no12")) and not (j == 2 and nulls in ("no2", "no12")) for j in range(3)]
        live.append(on)
        ents.append(rows_entry(f.v, r, n * sg, n * sg + pad, sg, [fo[j].v if on[j] else None for j in range(3)]))
    twice(name, lambda: reduce_call(ents, L.REDUCE_ROWS), [fo[j] for fo, on in zip(fouts, live) for j in range(3) if on[j]])
    assert all(f.intact() for f in fsrc)
    assert all(fo[j].untouched() for fo, on in zip(fouts, live) for j in range(3) if not on[j]), f"{name}: a null output's neighbour was written"
    for (r, n, sg, pad, nulls), x, fo, on in zip(cases, srcs, fouts, live):
        what = f"{name}: rows {r} x {n} segments of {sg}, ld + {pad}, {nulls}"
        ref = x.double().sum(0).view(n, sg)
        r32 = x.sum(0).view(n, sg) if measuring() else None
        for j in range(n):
            if not on[j]:
                continue
            judge("rm.rows", f"{what}: out{j}", fo[j].v, ref[j], r32[j] if measuring() else None)
            rejects("rm.rows", f"{what}: out{j}, the last row left out", fo[j].v, ref[j] - x[-1].double().view(n, sg)[j])
            if n > 1:
                rejects("rm.rows", f"{what}: out{j} holds the next segment", fo[j].v, ref[(j + 1) % n])


def test_reduce_multi_refusals():
    """every SEGCLIP_REQUIRE of segclip_reduce_multi: an error, nothing launched"""
    src = put((0.5 + torch.randn(8, 24, generator=seeded("rm_refusals"), dtype=F64)).float().to(DEV))
    outs = [Frame((8,), F32) for _ in range(3)]
    off4 = lambda t: t.view(-1)[1:]              # noqa: E731  a pointer 4 bytes past a 16-byte boundary

    def rows(**kw):
        a = dict(src=src.v, rows=8, width=24, ld=24, seg=8, outs=[o.v for o in outs])
        a.update(kw)
        return [rows_entry(a["src"], a["rows"], a["width"], a["ld"], a["seg"], a["outs"])], L.REDUCE_ROWS

    def slabs(**kw):
        a = dict(src=src.v, out=outs[0].v, splits=8, width=8, scale=1.0, dt=L.F32)
        a.update(kw)
        e = slabs_entry(a["src"], a["out"], a["splits"], a["width"], a["scale"])
        e.out_dtype = a["dt"]
        return [e], L.REDUCE_SLABS

    bad = {
        "n < 0": rows() + (-1,), "n > 16": (rows()[0] * 17, L.REDUCE_ROWS), "unknown kind": (rows()[0], 2),
        "rows: src null": rows(src=None), "rows: out0 null": rows(outs=[None, outs[1].v, outs[2].v]), "rows: rows 0": rows(rows=0),
        "rows: width 0": rows(width=0), "rows: width 22": rows(width=22), "rows: src unaligned": rows(src=off4(src.v)),
        "rows: out0 unaligned": rows(outs=[off4(outs[0].v), outs[1].v, outs[2].v]), "rows: seg 0": rows(seg=0),
        "rows: seg 6": rows(seg=6, width=12), "rows: ld 26": rows(ld=26), "rows: four segments": rows(seg=4, width=16),
        "rows: width no multiple of seg": rows(seg=16, width=24), "rows: out1 unaligned": rows(outs=[outs[0].v, off4(outs[1].v), outs[2].v]),
        "rows: out2 unaligned": rows(outs=[outs[0].v, outs[1].v, off4(outs[2].v)]),
        "rows: 2^31 workgroups": rows(width=2 ** 35, seg=2 ** 35, ld=2 ** 35),
        "slabs: src null": slabs(src=None), "slabs: out null": slabs(out=None), "slabs: splits 0": slabs(splits=0),
        "slabs: width 6": slabs(width=6), "slabs: src unaligned": slabs(src=off4(src.v)), "slabs: out unaligned": slabs(out=off4(outs[0].v)),
        "slabs: out dtype 2": slabs(dt=2),
    }
    for what, args in bad.items():
        with pytest.raises(RuntimeError):
            reduce_call(*args)
            raise AssertionError(f"{what}: accepted")
        sync()
        assert all(o.untouched() for o in outs) and src.intact(), f"{what}: something was written"
    reduce_call([], L.REDUCE_ROWS)          # no entry: nothing to do
    sync()
    assert all(o.untouched() for o in outs)
    twice("the entry the refusals vary", lambda: reduce_call(*rows()), outs)
    judge("rm.rows", "the entry the refusals vary", torch.cat([o.v for o in outs]), src.v.double().sum(0))


# ---- gates (through ops) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [770, 2052])
def test_gate_layer_norm_width(cols):
    assert instance_of(cols) is None
    gen = seeded(f"gate_ln_{cols}")
    x, g, b = ln_inputs(gen, 5, cols, F32, "gauss")
    fx = put(x)
    xv = fx.v.detach().requires_grad_()
    y = None
    with pytest.raises(RuntimeError, match="layernorm"):
        y = ops.layer_norm(xv, g, b)
    sync()
    assert y is None and xv.grad is None and fx.intact() and torch.equal(fx.v, x)
    fy, fm, fr = Frame((5, cols), F32), Frame((5,), F32), Frame((5,), F32)
    with pytest.raises(RuntimeError):
        lib_call("segclip_layernorm_fwd", fx.p, L.ptr(g), L.ptr(b), fy.p, fm.p, fr.p, 5, cols, 1e-5, L.F32, L.F32)
    sync()
    assert fy.untouched() and fm.untouched() and fr.untouched()


def test_gate_layer_norm_multi_width():
    x, g, b = ln_inputs(seeded("gate_lnm"), 6, 512, F32, "gauss")
    assert ops.layer_norm_multi(x, [(g, b)] * 3, (None, (2, 5, 3), None), 1e-5, F32) is None
    x, g, b = ln_inputs(seeded("gate_lnm"), 6, 768, F32, "gauss")
    ys = ops.layer_norm_multi(x, [(g, b)] * 3, (None, (2, 5, 3), None), 1e-5, F32)
    assert ys is not None and len(ys) == 3 and ys[1].shape == (3, 5, 768)
    judge("lnm.y", "layer_norm_multi at 768", ys[1][:, 3:5].reshape(6, 768), ln_torch(x, g, b, f32(1e-5), F64)["y"])


def test_gate_colsum_of_a_column_slice():
    gen = seeded("gate_colsum")
    for dt, M in ((F32, 65), (BF, 65), (F32, 4097)):
        big = (0.5 + torch.randn(M, 96, generator=gen, dtype=F64)).to(dt).to(DEV)
        big[:, :3] = float("nan")
        big[:, 67:] = float("nan")
        x = big[:, 3:67]
        assert not x.is_contiguous()
        judge("colsum.out", f"p_colsum of a column slice, {TN[dt]} M {M}", ops.p_colsum(x), x.double().sum(0))


def test_gate_layer_norm_of_no_rows():
    g = torch.ones(768, device=DEV, requires_grad=True)
    b = torch.zeros(768, device=DEV, requires_grad=True)
    x = torch.zeros(0, 768, device=DEV, requires_grad=True)
    for _ in range(3):      # (fresh allocations each time: what torch.empty returns is whatever was there)
        junk = [torch.full((768,), float("nan"), device=DEV) for _ in range(8)]
        del junk
        g.grad = b.grad = None
        y = ops.layer_norm(x, g, b)
        assert y.shape == (0, 768)
        y.sum().backward()
        sync()
        assert g.grad.shape == (768,) and bool((g.grad == 0).all()) and bool((b.grad == 0).all()) and x.grad.shape == (0, 768)


# ---- the tables reach every instance ------------------------------------------------------------------------------------------------
def test_rows_reach_every_instance():
    every_nv = {1, 2, 3, 4, 6, 8}
    assert set(WIDTHS) == {4, 64, 252, 256, 260, 768, 1024, 1028, 1280, 1536, 1540, 1792, 2048}
    assert {instance_of(c)[0] for c in WIDTHS} == every_nv and {cdiv(c // 4, 64) for c in WIDTHS} == set(range(1, 9))
    assert sum(c % 256 != 0 for c in WIDTHS) >= 6 and instance_of(1280)[0] == 6 and instance_of(1792)[0] == 8
    assert instance_of(770) is None and instance_of(2052) is None and instance_of(0) is None
    # forward: widths x rows x types x eps, the grid-stride rows, the regimes, the maps
    assert set(FWD_ROWS) == {1, 3, 4, 5, 197} and set(TYPES2) == {(F32, F32), (F32, BF), (BF, F32), (BF, BF)} and set(FWD_EPS) == {1e-5, 1e-6}
    assert FWD_LONG == 32773 and set(FWD_LONG_COLS) == {4, 64} and rows_per_wave(FWD_LONG, FWD_CAP) == {2, 3}
    assert all(rows_per_wave(r, FWD_CAP) <= {0, 1} for r in FWD_ROWS)
    assert {(c[0], c[2], c[3]) for c in FWD_REGIME_CASES} == {("hard", F32, F32)} | {("equal", a, b) for a, b in TYPES2}
    assert {c[1] for c in FWD_REGIME_CASES} >= {4, 2048} and {c[4] for c in FWD_REGIME_CASES} == set(FWD_EPS)
    for si, so in ((1, 4), (8, 13)):
        offs = {s[2] for _, s, _ in SEG_CASES if s[:2] == (si, so)}
        assert offs == {0, (so - si) // 2, so - si} and 0 < (so - si) // 2 < so - si
    assert {c for _, _, c in SEG_CASES} == {64, 768} and all(n >= 3 for n, _, _ in SEG_CASES)
    # backward: every template instance of the type / flag product at a narrow width and at 768; every NV with everything present
    plain = [c for c in BW_CASES if c.regime == "gauss"]
    for cols in (64, 768):
        got = {instance_of(c.cols, c.types, (c.res, c.dx2)) for c in plain if c.cols == cols}
        assert got >= {instance_of(cols, t, f) for t in TYPES3 for f in FLAGS2} and len(got) == 32
    assert {instance_of(c.cols)[0] for c in plain if c.res and c.dx2 and c.colsum} == every_nv
    assert {c.cols for c in BW_WIDTHS} == set(WIDTHS)
    assert {c.cols for c in plain if c.res and not c.colsum} >= {64, 768}
    rows64 = {c.rows for c in plain if c.cols == 64 and c.seg is None}
    assert rows64 >= {1, 3, 5, 197, 3073, 6149, 9216, BWD_UNROLL} and any(c.rows == 6149 and c.cols == 768 for c in plain)
    assert [rows_per_wave(r, BWD_CAP) for r in BWD_WALKS] == [{1, 2}, {2, 3}, {3}] and rows_per_wave(197, BWD_CAP) == {0, 1}
    assert 448 < blocks_of(BWD_UNROLL, BWD_CAP) <= 512 and blocks_of(BWD_WALKS[0], BWD_CAP) == 768
    assert {c.regime for c in BW_CASES} == set(REGIMES) and {c.seg for c in BW_SEG} == {s for _, s, _ in SEG_CASES}
    assert {c.types for c in BW_SEG} == set(TYPES3)
    # multi
    assert {multi_instance_of(3, c, F32, y) for _, c, y in MULTI_CASES} == {(3, "f32"), (3, "bf16"), (4, "f32"), (4, "bf16")}
    assert {r for r, _, _ in MULTI_CASES} == {1, 3, 197, 2049, 4101} and all(c == 768 for r, c, _ in MULTI_CASES if r > 197)
    assert [rows_per_wave(r, MULTI_CAP) for r in MULTI_WALKS] == [{1, 2}, {2, 3}]
    for r in MULTI_T:
        m = multi_maps(r)
        assert m[0] is None and m[1][1] - m[1][0] == m[1][2] == MULTI_G and 0 < m[2][2] < m[2][1] - m[2][0] and r % m[1][0] == 0
    # colsum
    single = [c for c in CS_CASES if c.route == "single"]
    assert {c.M for c in single} == set(CS_M) == {0, 1, 63, 64, 65, 448, 449, 513, 4096} and {c.N for c in single} == {4, 12, 16, 20, 768}
    assert {c.pad for c in single} == {0, 4} and all(c.dtype == F32 for c in single)
    two = [c for c in CS_CASES if c.route != "single"]
    assert {c.route for c in two} == {"two:vector:reduce_rows", "two:scalar:reduce_rows", "two:scalar:final", "two:mixed:final"}
    assert {c.M for c in two if c.dtype == BF and c.route == "two:vector:reduce_rows"} >= set(CS_M)
    assert any(c.M == 4097 and c.dtype == F32 for c in two) and {c.N for c in two if c.N % 4} == {1, 3, 77, 255}
    assert any(c.pad == 1 and c.N % 4 for c in two) and any(c.pad == 1 and c.N % 4 == 0 for c in two) and any(c.shift for c in two)
    assert {c.dtype for c in two if c.shift} == {F32, BF}
    assert cdiv(CS_TALL, 256) > CS_MAXCHUNK == colsum_chunks(CS_TALL, 8) and any(c.M == CS_TALL and c.N == 8 for c in two)
    # reduce_multi
    flat = [c for launch in SLAB_LAUNCHES[:9] for c in launch]
    assert sorted(flat, key=str) == sorted(SLAB_CASES, key=str) and all(len(x) == 16 for x in SLAB_LAUNCHES[:9])
    assert set(SLAB_SPLITS) == {1, 3, 4, 7, 8, 9, 12, 13, 21} and set(SLAB_WIDTHS) == {4, 1020, 1024, 1028} and set(SLAB_SCALES) == {1.0, 0.37}
    assert {s % 8 >= 4 for s in SLAB_SPLITS} == {True, False} and {s // 8 for s in SLAB_SPLITS} == {0, 1, 2}
    flat = [c for launch in ROWS_LAUNCHES[:4] for c in launch]
    assert sorted(flat, key=str) == sorted(ROWS_CASES, key=str) and max(len(x) for x in ROWS_LAUNCHES) == 16
    assert {c[0] for c in ROWS_CASES} == {1, 63, 64, 65, 448, 449, 1000} and {c[1] for c in ROWS_CASES} == {1, 2, 3}
    assert {c[2] for c in ROWS_CASES} == {4, 64, 768} and {c[3] for c in ROWS_CASES} == {0, 8}
    assert {c[4] for c in ROWS_CASES if c[1] == 3} == {"all", "no1", "no2", "no12"}
    assert any(len(x) == 1 for x in SLAB_LAUNCHES) and any(len(x) == 1 for x in ROWS_LAUNCHES)
    assert set(FLOORS) >= {f"ln.{k}{s}" for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta", "colsum") for s in ("", ".hard")}


# ---- the measurement behind FLOORS ---------------------------------------------------------------------------------------------------
def value_rows():
    """(test function, arguments) of every row that judges values"""
    rows = [(test_ln_fwd, (c,)) for c in WIDTHS] + [(test_ln_fwd_regimes, (r, c)) for r in ("hard", "equal") for c in (4, 64, 260, 768, 2048)]
    rows += [(test_ln_fwd_grid_stride, (c,)) for c in FWD_LONG_COLS] + [(test_ln_fwd_seg, r) for r in SEG_CASES]
    rows += [(test_ln_bwd, (c,)) for c in BW_CASES] + [(test_ln_multi, r) for r in MULTI_CASES]
    rows += [(test_colsum, g) for g in CS_GROUPS]
    rows += [(test_reduce_multi_slabs, (k,)) for k in range(len(SLAB_LAUNCHES))] + [(test_reduce_multi_rows, (k,)) for k in range(len(ROWS_LAUNCHES))]
    return rows


def floors():
    """every row once with BOUNDS.stats set: {key: floor of torch float32 against fp64, the kernel's error, the rows they come from}"""
    BOUNDS.stats = {}
    try:
        for fn, args in value_rows():
            fn(*args)
        return BOUNDS.stats
    finally:
        BOUNDS.stats = None
