"""GPU: the kernels that produce the number the training step differentiates - the contrastive head of csrc/head.hip (max over the
tokens, the stacked L2 normalisation, the two-matrix cross entropy) and the loss kernels of csrc/misc.hip (L2 normalisation, the
cross entropies with implicit and explicit labels, the superpixel KL, the masked MSE, reduce_sum and scale) - reached by a row of
the tables below and checked against fp64 torch on exactly the fp32 / bf16 values the kernel reads.  All kernel calls go through
the C ABI (segclip_amd._lib), the test owns every buffer (tests/kernel_frames.py, as tests/test_center_stage_gpu.py).

Per row: (1) every output is a view inside a larger NaN buffer (0xAB for integer outputs): the guards survive and everything
inside becomes finite; (2) the inputs sit in frames of the same kind; (3) the same call a second time into the same frames is
bit-identical, frames included; (4) the values against fp64 with the bound of tests/helpers.check, |err| <= rtol * (|ref| +
rms(ref)); (5) the same bound REJECTS the fp64 reference after a small defect.  A backward reads what its forward wrote (y and the
norms, lse); its reference is the fp64 gradient of the inputs, never of those intermediates.

Rows (test_rows_reach_every_edge restates the coverage):
  l2norm_fwd/bwd, l2norm_pair_fwd/bwd: rows / B in 1 3 4 5 33 (the last workgroup of four waves partly live) x C in 1 63 64 65 512
      768; the pair backward with dboth2 null and set; both[b][0] = v, both[b][1] = t and norms[2b + which] element by element.
      test_l2norm_out_of_range: a row scaled by 1e-18 (its squares are 1e-36: small ones are subnormal, the sum is not; it meets
      the ordinary bound) and one by 1e18 (512 squares of 1e36 exceed 3.4e38: the fp32 sum of squares is inf, the norm inf, y = x /
      inf = 0 and dx = 0 - the kernel does not rescale, and neither does x / x.norm() in torch float32, which returns the same
      zeros; fp64 gives a unit vector there).
  ce_fwd/bwd: rows in 1 3 4 5 77 x cols in 63 64 65 512 (rows <= cols), 1 x 1; label_offset 0, an interior value and cols - rows;
      gscale_ptr null and set; 77 x 16384 (1.26 M elements, beyond 4096 x 256 threads).
  clip_ce_fwd/bwd: B in 1 3 8 33 x N in B, 2B + 1, 8B; label_offset 0, B, N - B; logit_scale ln(1 / 0.07), 4.6 and 5.0 (clamped:
      dlogit_scale exactly 0); g and dlogit_scale null and set; lse, loss_rows, loss, dcos, ds_rows, dlogit_scale.
  ce_labels_fwd/bwd: rows in 1 5 77 x cols in 65 512, 5 x 49408; ignore_index -100, -1, 0; from 5 rows on one row with the ignored
      label, one with label = cols and one with label -7: loss 0, valid 0, gradient row exactly 0; 77 x 16384; every row
      ignored through ops.CrossEntropyLabelsFn (loss NaN as torch, gradient exactly 0).
  the three cross entropies in three regimes: Gaussian logits, all-equal rows, trained rows (cosines 0.7 +- 0.03 times 100, the
      label's cosine raised by 0.05, 0.10, 0.15: row losses from about 4 down to about 3e-3) under keys of their own (*.trained).
  superpixel_kl: G in 1 3 8 16 x T in 1 7 196 255 256 257 577 (one block of 256 threads per image), sp_lds_limit (B 2, G 8, T
      1666: 59976 bytes of LDS); label layouts: one label, all distinct, a few, negative, and 5 / 5 + 2^32 / 9; hard one-hot,
      real-valued in sp_g3_t196 and sp_g8_t257; B = 2 or 3 (coef = B T G).  With G = 1, T = 1 or all labels distinct the loss and
      its gradient are exactly 0 and are asserted as such (the torch expression leaves rounding noise there).
  masked_mse_fwd/bwd: (B, T) in (1,1) (5,1) (1,5) (197,1) (1,197) x Dp in 4 48 65 588 768 x pred fp32 | bf16; from B = 5 on one
      sample with an all-zero mask; mask 0.5 in one row; the CLS entry of the mask is 0.25 and the CLS row of dpred exactly 0;
      8 x 198 x 768 (1.22 M elements).
  max_tokens_fwd/bwd: T in 1 2 4 5 8 9 37 x D in 4 64 768, B = 3 (B D / 4 = 3, 48, 576: no multiple of 128); two equal maxima and
      an all-equal column (the lowest token wins); out, idx, dx and the bf16 copy bit-exact; dx / dx_bf16 null in turn; B 48, T 150,
      D 768 (1.38 M vectors: the backward's grid-stride loop).
  reduce_sum, scale: n in 1 63 1023 1024 1025 100003, scale 0.37 (sixteen vectors per n); scale also at n = 1100003.
  grid1d is capped at 4096 blocks of 256 threads = 1048576 elements; the rows of more elements above are past it
  (masked_mse_bwd, scale, and max_tokens_bwd's own cap; ce_bwd and ce_labels_bwd were grid1d launches and keep their rows).

Defects the bound must reject (5):
  cross entropies: the label column shifted by one; label_offset dropped; for the second matrix of clip_ce the label of row r
      taken as r instead of r % B; the one-hot term dropped from the gradient; the clamp removed at logit_scale 5.0; the last
      column left out of the row sum
  L2: the y (g . y) term dropped; dboth2 ignored; v and t swapped in the stack
  superpixel KL: the mean taken without the superpixel's last member; the gradient through the mean dropped; 5 and 5 + 2^32 merged
  masked MSE: the mask of token t instead of 1 + t; 1 / Dp for 2 / Dp
  max over tokens, reduce_sum, scale: the last element replaced by its neighbour's

Bounds.  Integer, mask and copy outputs (idx, valid, the max and its routed gradient, exact zeros): bit-exact.  bf16 dpred: 2^-8,
as derived in tests/test_center_stage_gpu.py.  scale: one correctly rounded product, 2^-24.  Every other fp32 output: floor =
torch float32 of the same expression (F.cross_entropy / log_softmax, clamp(exp(ls), max=100) in fp32, the kl_div expression of
tests/test_kernels_gpu.py, x / x.norm()) against fp64 in check() units, the maximum over the rows of the kernel; bound = 4 x floor
rounded up to one digit (the 4 covers another summation order over up to 49408 columns or 1666 tokens).  The floor never
involves the kernel.  Measured on an MI355X by floors() (FLOORS holds the figures; `kernel` is this build's own error, for the
record only):
    key                       floor   -> bound    kernel     before this file's kernel changes   the floor's row
    l2.y                     1.154e-07 -> 5e-07    9.688e-08  9.688e-08                          l2p_b4_c512
    l2.n                     7.383e-08 -> 3e-07    5.245e-08  5.245e-08                          l2p_b4_c512
    l2.dx                    1.490e-07 -> 6e-07    1.528e-07  1.528e-07                          l2p_b4_c512
    ce.lse                   3.452e-08 -> 2e-07    4.673e-08  4.673e-08                          ce_r77_c16384_gauss_off0
    ce.loss_rows             5.081e-08 -> 3e-07    5.581e-08  1.819e-07                          ce_r77_c512_gauss_off0
    ce.dlogits               3.779e-07 -> 2e-06    5.791e-07  1.732e-06                          ce_r77_c16384_gauss_off0
    ce.lse.trained           2.428e-08 -> 1e-07    2.437e-08  2.437e-08                          ce_r4_c512_trained_off254
    ce.loss_rows.trained     3.549e-06 -> 2e-05    3.549e-06  5.172e-05                          ce_r3_c64_trained_off0
    ce.dlogits.trained       3.224e-05 -> 0.0002   1.313e-05  2.139e-04                          ce_r3_c64_trained_off0
    clip.lse                 7.117e-08 -> 3e-07    8.976e-08  8.513e-08                          clip_b8_n17_gauss_off0_ls2.66
    clip.loss_rows           1.129e-07 -> 5e-07    1.129e-07     inf                             clip_b1_n8_gauss_off7_ls5.00
    clip.loss                7.204e-08 -> 3e-07    1.098e-07     inf                             clip_b1_n8_gauss_off7_ls5.00
    clip.dcos                4.827e-07 -> 2e-06    4.398e-07  6.350e-07                          clip_b33_n264_gauss_off231_ls5.00
    clip.ds_rows             3.118e-06 -> 2e-05    2.217e-06  2.217e-06                          clip_b1_n8_gauss_off7_ls4.60
    clip.dls                 1.436e-06 -> 6e-06    4.121e-07     inf                             clip_b1_n8_gauss_off7_ls4.60
    clip.lse.trained         4.581e-08 -> 2e-07    4.581e-08  3.399e-08                          clip_b8_n17_trained_off9_ls5.00
    clip.loss_rows.trained   1.867e-04 -> 0.0008   1.867e-04     inf                             clip_b1_n3_trained_off2_ls5.00
    clip.loss.trained        7.450e-05 -> 0.0003   7.450e-05     inf                             clip_b1_n3_trained_off2_ls5.00
    clip.dcos.trained        1.669e-04 -> 0.0007   1.672e-04     inf                             clip_b1_n3_trained_off2_ls5.00
    clip.ds_rows.trained     1.170e-03 -> 0.005    1.170e-03     inf                             clip_b1_n3_trained_off2_ls5.00
    clip.dls.trained         1.875e-04 -> 0.0008   1.871e-04     inf                             clip_b3_n24_trained_off3_ls4.60
    cel.lse                  3.569e-08 -> 2e-07    4.304e-08  4.304e-08                          cel_r5_c65_gauss_ign0
    cel.loss_rows            5.938e-08 -> 3e-07    5.938e-08  5.938e-08                          cel_r5_c65_gauss_ign-100
    cel.dlogits              4.054e-07 -> 2e-06    8.983e-07  1.477e-06                          cel_r77_c16384_gauss_ign-100
    cel.lse.trained          2.378e-08 -> 1e-07    2.419e-08  2.419e-08                          cel_r77_c65_trained_ign-100
    cel.loss_rows.trained    7.626e-08 -> 4e-07    7.626e-08  2.509e-06                          cel_r77_c512_trained_ign-100
    cel.dlogits.trained      8.369e-06 -> 4e-05    3.875e-06  1.087e-04                          cel_r77_c512_trained_ign-100
    sp.loss_rows             2.394e-06 -> 1e-05    1.739e-07  1.739e-07                          sp_g16_t196
    sp.dhard                 7.140e-07 -> 3e-06    3.239e-07  3.239e-07                          sp_g3_t7
    mse.loss_rows            1.114e-07 -> 5e-07    1.031e-07  1.031e-07                          mse_b1_t197_d4_f32
    mse.dpred                1.315e-07 -> 6e-07    1.315e-07  1.315e-07                          mse_b197_t1_d65_f32
    reduce.out               5.054e-08 -> 3e-07    6.831e-08  6.831e-08                          rs_n1023
  (`before`: the same rows on the kernels as they were - max + log(s) - z_label, exp(z - lse) - onehot, the contrastive logit
  fused into the subtraction.  inf: a nonzero result where the reference is exactly 0, the one-column rows of clip_ce.  The
  trained floors are large because fp32 cannot hold a row loss of 1e-3 or less to more than a few digits in ANY form:
  s = 1 + 1e-3 is rounded to 6e-8.  The largest come from rows of one to three samples, where rms(ref) is such a loss.)

Fixes that came with this file:
  - ce_fwd, ce_labels_fwd, clip_ce_fwd formed the row loss as (max + log s) - z_label: the sum is rounded to an ulp of |max|
    (4e-6 at logits of 85) before z_label cancels it.  Now log s - (z_label - max), the log_softmax order; lse is unchanged.
  - ce_bwd, ce_labels_bwd, clip_ce_bwd took softmax = exp(z - lse), which carries lse's rounding into every probability and
    into (softmax - 1) on the label.  Now exp(z - lse) / sum_j exp(z_j - lse), one wave per row (the two elementwise kernels
    became row kernels: one more pass over the logits, none over rows without a label).
  - clip_ce formed scale * cos inside a fused multiply-add: the row maximum was not one of the logits, and a row of one column
    had a loss of 4e-8 instead of 0.  The logit is now one rounded product everywhere.
"""
import dataclasses
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from segclip_amd import _lib as L  # noqa: E402
from segclip_amd import ops  # noqa: E402
from tests.kernel_frames import BF, DEV, F32, F64, Bounds, Frame, draw, lib_call, put, run_twice, seeded  # noqa: E402

Fn = torch.nn.functional
RT_BF = 2.0 ** -8
RT_MUL = 2.0 ** -24
GRID_CAP = 4096 * 256          # grid1d of csrc/misc.hip and the backward of max_tokens: at most 4096 blocks of 256 threads

# floors measured by floors() (torch float32 against fp64 on this file's rows, maximum over the rows of the kernel)
FLOORS = {
    "l2.y": 1.154e-07,
    "l2.n": 7.383e-08,
    "l2.dx": 1.490e-07,
    "ce.lse": 3.452e-08,
    "ce.loss_rows": 5.081e-08,
    "ce.dlogits": 3.779e-07,
    "ce.lse.trained": 2.428e-08,
    "ce.loss_rows.trained": 3.549e-06,
    "ce.dlogits.trained": 3.224e-05,
    "clip.lse": 7.117e-08,
    "clip.loss_rows": 1.129e-07,
    "clip.loss": 7.204e-08,
    "clip.dcos": 4.827e-07,
    "clip.ds_rows": 3.118e-06,
    "clip.dls": 1.436e-06,
    "clip.lse.trained": 4.581e-08,
    "clip.loss_rows.trained": 1.867e-04,
    "clip.loss.trained": 7.450e-05,
    "clip.dcos.trained": 1.669e-04,
    "clip.ds_rows.trained": 1.170e-03,
    "clip.dls.trained": 1.875e-04,
    "cel.lse": 3.569e-08,
    "cel.loss_rows": 5.938e-08,
    "cel.dlogits": 4.054e-07,
    "cel.lse.trained": 2.378e-08,
    "cel.loss_rows.trained": 7.626e-08,
    "cel.dlogits.trained": 8.369e-06,
    "sp.loss_rows": 2.394e-06,
    "sp.dhard": 7.140e-07,
    "mse.loss_rows": 1.114e-07,
    "mse.dpred": 1.315e-07,
    "reduce.out": 5.054e-08,
}
BOUNDS = Bounds(FLOORS)
RT = BOUNDS.rt
judge, rejects = BOUNDS.judge, BOUNDS.rejects


def measuring():
    return BOUNDS.stats is not None


def scalar(v, dtype=F32):
    return torch.tensor([v], dtype=dtype, device=DEV)


def exact_zero(t):
    return bool((t == 0).all())


# ---- L2 normalisation ------------------------------------------------------------------------------------------------------
L2_CASES = list(itertools.product((1, 3, 4, 5, 33), (1, 63, 64, 65, 512, 768)))


def l2_expr(x, g, dt, drop_dot=False):
    x, g = x.to(dt), g.to(dt)
    n = x.norm(dim=-1, keepdim=True)
    y = x / n
    dot = 0 if drop_dot else (g * y).sum(-1, keepdim=True)
    return {"y": y, "n": n.squeeze(-1), "dx": (g - y * dot) / n}


@pytest.mark.parametrize("rows,C", L2_CASES, ids=[f"l2_r{r}_c{c}" for r, c in L2_CASES])
def test_l2norm(rows, C):
    name = f"l2_r{rows}_c{C}"
    gen = seeded(name)
    x, g = draw(gen, rows, C), draw(gen, rows, C)
    fx, fg = put(x), put(g)
    fy, fn, fdx = Frame((rows, C), F32), Frame((rows,), F32), Frame((rows, C), F32)
    run_twice(name + " fwd", lambda: lib_call("segclip_l2norm_fwd", fx.p, fy.p, fn.p, rows, C), [fy, fn])
    run_twice(name + " bwd", lambda: lib_call("segclip_l2norm_bwd", fg.p, fy.p, fn.p, fdx.p, rows, C), [fdx])
    assert fx.intact() and fg.intact() and fy.intact() and fn.intact()
    ref = l2_expr(x, g, F64)
    r32 = l2_expr(x, g, F32) if measuring() else {}
    got = {"y": fy.v, "n": fn.v, "dx": fdx.v}
    for k in got:
        judge(f"l2.{k}", f"{name}: {k}", got[k], ref[k], r32.get(k))
    rejects("l2.dx", f"{name}: dx without y (g . y)", fdx.v, l2_expr(x, g, F64, drop_dot=True)["dx"])
    if rows >= 2:
        for k in got:
            w = ref[k].clone()
            w[-1] = w[-2]
            if not torch.equal(w, ref[k]):
                rejects(f"l2.{k}", f"{name}: {k}, the last row replaced by its neighbour", got[k], w)


def pair_expr(v, t, g1, g2, dt, drop_dot=False):
    B = v.shape[0]
    g = g1.to(dt) + (g2.to(dt) if g2 is not None else 0)
    rv, rt = l2_expr(v, g[:, 0], dt, drop_dot), l2_expr(t, g[:, 1], dt, drop_dot)
    return {"both": torch.stack([rv["y"], rt["y"]], 1), "norms": torch.stack([rv["n"], rt["n"]], 1).reshape(2 * B),
            "dv": rv["dx"], "dt": rt["dx"]}


@pytest.mark.parametrize("B,C", L2_CASES, ids=[f"l2p_b{r}_c{c}" for r, c in L2_CASES])
def test_l2norm_pair(B, C):
    name = f"l2p_b{B}_c{C}"
    gen = seeded(name)
    v, t, g1, g2 = draw(gen, B, C), draw(gen, B, C, scale=3.0), draw(gen, B, 2, C), draw(gen, B, 2, C)
    fv, ft, f1, f2 = put(v), put(t), put(g1), put(g2)
    fb, fn = Frame((B, 2, C), F32), Frame((2 * B,), F32)
    run_twice(name + " fwd", lambda: lib_call("segclip_l2norm_pair_fwd", fv.p, ft.p, fb.p, fn.p, B, C), [fb, fn])
    ref0 = pair_expr(v, t, g1, None, F64)
    r32 = pair_expr(v, t, g1, None, F32) if measuring() else {}
    judge("l2.y", f"{name}: both", fb.v, ref0["both"], r32.get("both"))
    judge("l2.n", f"{name}: norms", fn.v, ref0["norms"], r32.get("norms"))
    for b in range(B):                      # the stack, element by element: [b][0] = v, [b][1] = t, norms[2b + which]
        for which, src in enumerate((v, t)):
            one = l2_expr(src[b:b + 1], src[b:b + 1], F64)
            judge("l2.y", f"{name}: both[{b}][{which}]", fb.v[b, which], one["y"][0])
            judge("l2.n", f"{name}: norms[{2 * b + which}]", fn.v[2 * b + which:2 * b + which + 1], one["n"])
    swapped = pair_expr(t, v, g1, None, F64)
    if not torch.equal(swapped["both"], ref0["both"]):            # C = 1: both are +-1
        rejects("l2.y", f"{name}: both with v and t swapped", fb.v, swapped["both"])
    rejects("l2.n", f"{name}: norms with v and t swapped", fn.v, swapped["norms"])
    for second in (None, f2):
        what = f"{name} bwd {'with' if second else 'without'} dboth2"
        fdv, fdt = Frame((B, C), F32), Frame((B, C), F32)
        run_twice(what, lambda: lib_call("segclip_l2norm_pair_bwd", f1.p, second.p if second else None, fb.p, fn.p, fdv.p, fdt.p, B, C),
                  [fdv, fdt])
        gg = g2 if second else None
        ref = pair_expr(v, t, g1, gg, F64)
        r32 = pair_expr(v, t, g1, gg, F32) if measuring() else {}
        nodot = pair_expr(v, t, g1, gg, F64, drop_dot=True)
        for k, f in (("dv", fdv), ("dt", fdt)):
            judge("l2.dx", f"{what}: {k}", f.v, ref[k], r32.get(k))
            rejects("l2.dx", f"{what}: {k} without y (g . y)", f.v, nodot[k])
            if second and C >= 2:                   # (C = 1: the gradient of x / |x| is 0 whatever comes in)
                rejects("l2.dx", f"{what}: {k} with dboth2 ignored", f.v, ref0[k])
    assert all(f.intact() for f in (fv, ft, f1, f2, fb, fn))


def test_l2norm_out_of_range():
    """row 0 as drawn, row 1 scaled by 1e-18, row 2 by 1e18 (C = 512), through both forward kernels and both backwards.  Row 1:
    the ordinary bound.  Row 2: the fp32 sum of squares is inf - norm inf, y = 0, dx = 0, all finite but the norm; torch float32
    does the same (x / x.norm() = 0), fp64 does not (a unit vector)."""
    C = 512
    gen = seeded("l2_range")
    x, g = draw(gen, 3, C), draw(gen, 3, C)
    x[1] *= 1e-18
    x[2] *= 1e18
    fx, fg = put(x), put(g)
    fy, fn, fdx = Frame((3, C), F32), Frame((3,), F32), Frame((3, C), F32)
    lib_call("segclip_l2norm_fwd", fx.p, fy.p, fn.p, 3, C)
    lib_call("segclip_l2norm_bwd", fg.p, fy.p, fn.p, fdx.p, 3, C)
    fb, fpn, fdv, fdt = Frame((3, 2, C), F32), Frame((6,), F32), Frame((3, C), F32), Frame((3, C), F32)
    g2 = torch.stack([g, g], 1).contiguous()
    f2 = put(g2)
    lib_call("segclip_l2norm_pair_fwd", fx.p, fx.p, fb.p, fpn.p, 3, C)
    lib_call("segclip_l2norm_pair_bwd", f2.p, None, fb.p, fpn.p, fdv.p, fdt.p, 3, C)
    torch.cuda.synchronize()
    assert all(f.intact() for f in (fy, fn, fdx, fb, fpn, fdv, fdt))
    ref, r32 = l2_expr(x, g, F64), l2_expr(x, g, F32)
    print(f"l2 out of range: kernel norms {fn.v.tolist()}, torch float32 norms {r32['n'].tolist()}, fp64 {ref['n'].tolist()}")
    for ys, ns, dxs, what in ((fy.v, fn.v, fdx.v, "l2norm"), (fb.v[:, 0], fpn.v[0::2], fdv.v, "pair v"), (fb.v[:, 1], fpn.v[1::2], fdt.v, "pair t")):
        for r in (0, 1):
            judge("l2.y", f"{what}: y of row {r}", ys[r], ref["y"][r])
            judge("l2.n", f"{what}: norm of row {r}", ns[r:r + 1], ref["n"][r:r + 1])
            judge("l2.dx", f"{what}: dx of row {r}", dxs[r], ref["dx"][r])
        assert math.isinf(float(ns[2])) and float(ns[2]) > 0, f"{what}: the sum of 512 squares of 1e36 is beyond fp32"
        assert exact_zero(ys[2]) and exact_zero(dxs[2]), f"{what}: x / inf = 0 and a zero gradient"
    assert math.isinf(float(r32["n"][2])) and exact_zero(r32["y"][2]), "torch float32 leaves the range in the same way"
    assert bool(ref["y"][2].norm() > 0.999), "fp64 holds the row"


# ---- the three cross entropies ---------------------------------------------------------------------------------------------
REGIMES = ("gauss", "equal", "trained")
RAISE = (0.05, 0.10, 0.15)


def trained_cos(gen, R, N, labels):
    """(R, N) cosines in fp64: 0.7 +- 0.03, the label's raised by 0.05, 0.10, 0.15 in turn (labels outside [0, N): none raised);
    the last column, where it is not the label's, is a hard negative at 0.74, so that leaving it out of the row sum shows"""
    c = 0.7 + 0.03 * torch.randn(R, N, generator=gen, dtype=F64)
    c[:, N - 1] = 0.74
    for r in range(R):
        if 0 <= int(labels[r]) < N:
            c[r, int(labels[r])] = 0.7 + 0.03 * float(torch.randn((), generator=gen, dtype=F64)) + RAISE[r % 3]
    return c.clamp(-1.0, 1.0)


def near_max_last(z, gap):
    """the last column `gap` below the largest of the others (a column that counts in the row sum)"""
    if z.shape[1] >= 2:
        z[:, -1] = z[:, :-1].max(1).values - gap
    return z


def logits_of(regime, gen, R, N, labels):
    """fp32 logits on the device"""
    if regime == "gauss":
        z = near_max_last(torch.randn(R, N, generator=gen, dtype=F64) * 4.0, 0.5)
    elif regime == "equal":
        z = torch.full((R, N), 1.75, dtype=F64)
    else:
        z = 100.0 * trained_cos(gen, R, N, labels)
    return z.float().to(DEV)


def xent(z, labels, drop_last=False, drop_onehot=False):
    """z (R, N), labels (R,) in [0, N) -> lse, loss_rows, softmax - onehot, in z's precision"""
    lse = torch.logsumexp(z[:, :-1] if drop_last else z, -1)
    zl = z.gather(1, labels[:, None])[:, 0]
    if drop_last or z.dtype == F64:
        loss, p = lse - zl, (z - lse[:, None]).exp()
    else:       # the plain torch float32 expressions
        loss, p = Fn.cross_entropy(z, labels, reduction="none"), torch.log_softmax(z, -1).exp()
    if not drop_onehot:
        p = p - Fn.one_hot(labels, z.shape[1]).to(z.dtype)
    return lse, loss, p


def key_of(family, out, regime):
    return f"{family}.{out}" + (".trained" if regime == "trained" else "")


@dataclasses.dataclass
class CE:
    rows: int
    cols: int
    regime: str

    @property
    def name(self):
        return f"ce_r{self.rows}_c{self.cols}_{self.regime}"

    @property
    def offsets(self):
        return sorted({0, (self.cols - self.rows) // 2, self.cols - self.rows})


CE_SHAPES = [(1, 1)] + [(r, c) for r in (1, 3, 4, 5) for c in (63, 64, 65, 512)] + [(77, 512)]
CE_CASES = [CE(r, c, reg) for r, c in CE_SHAPES for reg in REGIMES] + [CE(77, 16384, "gauss")]


def ce_expr(z, labels, gs, dt, **defect):
    lse, loss, d = xent(z.to(dt), labels, **defect)
    return {"lse": lse, "loss_rows": loss, "dlogits": gs.to(dt) * d}


@pytest.mark.parametrize("c", CE_CASES, ids=[c.name for c in CE_CASES])
def test_ce(c):
    R, N = c.rows, c.cols
    gptr = scalar(0.37)
    for off in c.offsets:
        name = f"{c.name}_off{off}"
        gen = seeded(name)
        labels = torch.arange(R) + off
        z = logits_of(c.regime, gen, R, N, labels)
        labels = labels.to(DEV)
        fz, fl, fr = put(z), Frame((R,), F32), Frame((R,), F32)
        run_twice(name + " fwd", lambda: lib_call("segclip_ce_fwd", fz.p, fl.p, fr.p, R, N, off), [fl, fr])
        for gp in (None, gptr):
            what = f"{name} {'with' if gp is not None else 'without'} gscale_ptr"
            fd = Frame((R, N), F32)
            run_twice(what, lambda: lib_call("segclip_ce_bwd", fz.p, fl.p, L.ptr(gp), 1.7, fd.p, R, N, off), [fd])
            g32 = (gp[0] if gp is not None else torch.ones((), device=DEV)) * torch.tensor(1.7, dtype=F32, device=DEV)
            gs64, gs32 = g32.double() / R, g32 / R
            ref = ce_expr(z, labels, gs64, F64)
            r32 = ce_expr(z, labels, gs32, F32) if measuring() else {}
            got = {"lse": fl.v, "loss_rows": fr.v, "dlogits": fd.v}
            for k in got:
                judge(key_of("ce", k, c.regime), f"{what}: {k}", got[k], ref[k], r32.get(k))
            wrong = {}
            if N >= 2:
                wrong["the label column shifted by one"] = ce_expr(z, (labels + 1) % N, gs64, F64)
                wrong["the last column left out of the row sum"] = ce_expr(z, labels, gs64, F64, drop_last=True)
                wrong["the one-hot term dropped"] = ce_expr(z, labels, gs64, F64, drop_onehot=True)
            if off > 0:
                wrong["label_offset dropped"] = ce_expr(z, labels - off, gs64, F64)
            assert wrong or N == 1
            for dname, w in wrong.items():
                for k in ("loss_rows", "dlogits"):
                    if not torch.equal(w[k], ref[k]):
                        rejects(key_of("ce", k, c.regime), f"{what}: {k}, {dname}", got[k], w[k])
        assert fz.intact() and fl.intact() and fr.intact()


@dataclasses.dataclass
class CLIP:
    B: int
    N: int
    regime: str

    @property
    def name(self):
        return f"clip_b{self.B}_n{self.N}_{self.regime}"

    @property
    def offsets(self):
        return sorted({0, self.B, self.N - self.B} if self.N > self.B else {0})


LOGIT_SCALES = (math.log(1 / 0.07), 4.6, 5.0)
CLIP_CASES = [CLIP(B, N, reg) for B in (1, 3, 8, 33) for N in (B, 2 * B + 1, 8 * B) for reg in REGIMES]
CLIP_OUTS = ("lse", "loss_rows", "loss", "dcos", "ds_rows", "dls")


def clip_cos(regime, gen, B, N, labels):
    if regime == "gauss":
        c = near_max_last(0.03 * torch.randn(2 * B, N, generator=gen, dtype=F64), 0.005)     # logits of sigma 0.4 to 3
    elif regime == "equal":
        c = torch.full((2 * B, N), 0.5, dtype=F64)
    else:
        c = trained_cos(gen, 2 * B, N, labels)
    return c.float().to(DEV)


def clip_expr(cos, ls, g, B, labels, dt, clamp=True, **defect):
    """the contrastive loss of 2B rows of cosines: clamp(exp(ls), max=100) * cos, cross entropy against `labels`, the mean; the
    gradients of g * loss in cos and ls"""
    cos, e = cos.to(dt), ls.to(dt).exp()[0]
    sc = e.clamp(max=100.0) if clamp else e
    lse, loss, d = xent(sc * cos, labels, **defect)
    d = d * ((g.to(dt)[0] if g is not None else 1.0) / (2 * B))
    ds = (d * cos).sum(-1)
    live = bool(e <= 100.0) or not clamp
    return {"lse": lse, "loss_rows": loss, "loss": loss.mean().reshape(1), "dcos": d * sc, "ds_rows": ds,
            "dls": (ds.sum() * e if live else ds.sum() * 0).reshape(1)}


@pytest.mark.parametrize("c", CLIP_CASES, ids=[c.name for c in CLIP_CASES])
def test_clip_ce(c):
    B, N = c.B, c.N
    g = scalar(1.7)
    for n, (off, ls0) in enumerate(itertools.product(c.offsets, LOGIT_SCALES)):
        name = f"{c.name}_off{off}_ls{ls0:.2f}"
        gen = seeded(name)
        labels = torch.arange(2 * B) % B + off
        cos = clip_cos(c.regime, gen, B, N, labels)
        labels = labels.to(DEV)
        ls = scalar(ls0)
        fc, fs = put(cos.view(2, B, N)), put(ls)
        fl, fr, fo = Frame((2 * B,), F32), Frame((2 * B,), F32), Frame((1,), F32)
        run_twice(name + " fwd", lambda: lib_call("segclip_clip_ce_fwd", fc.p, fs.p, fl.p, fr.p, fo.p, B, N, off), [fl, fr, fo])
        for with_g, with_dls in ((n % 2 == 0, True), (n % 2 == 1, False)):
            what = f"{name} g {'set' if with_g else 'null'} dls {'set' if with_dls else 'null'}"
            fg = put(g)
            fd, fds, fdl = Frame((2, B, N), F32), Frame((2 * B,), F32), Frame((1,), F32)
            run_twice(what, lambda: lib_call("segclip_clip_ce_bwd", fc.p, fl.p, fs.p, fg.p if with_g else None, fd.p, fds.p,
                                             fdl.p if with_dls else None, B, N, off), [fd, fds] + ([fdl] if with_dls else []))
            if not with_dls:
                assert fdl.untouched(), f"{what}: dlogit_scale written though null was passed"
            assert fg.intact()
            gg = g if with_g else None
            ref = clip_expr(cos, ls, gg, B, labels, F64)
            r32 = clip_expr(cos, ls, gg, B, labels, F32) if measuring() else {}
            got = {"lse": fl.v, "loss_rows": fr.v, "loss": fo.v, "dcos": fd.v.view(2 * B, N), "ds_rows": fds.v}
            if with_dls:
                got["dls"] = fdl.v
                if ls0 == 5.0:
                    assert float(fdl.v) == 0.0, f"{what}: the clamped scale has no gradient"
            if c.regime == "equal":
                # every cosine is 0.5: ds_rows = 0.5 * sum_j (softmax - onehot)_j = 0 and dlogit_scale = 0, where the fp64 expression
                # leaves 1e-17 - no yardstick.  What dcos's bound allows, carried through the sum: rt * sum_j |d_j cos_j| per row
                got.pop("ds_rows")
                got.pop("dls", None)
                if not measuring():
                    e64 = ls.double().exp()[0]
                    cap = RT["clip.dcos"] * (ref["dcos"].abs() / e64.clamp(max=100.0) * cos.double().abs()).sum(-1)
                    assert bool((fds.v.double().abs() <= cap).all()), f"{what}: ds_rows of equal cosines"
                    if with_dls:
                        assert abs(float(fdl.v)) <= float(cap.sum() * e64), f"{what}: dlogit_scale of equal cosines"
            for k in got:
                judge(key_of("clip", k, c.regime), f"{what}: {k}", got[k], ref[k], r32.get(k))
            wrong = {}
            if N >= 2:
                wrong["the label column shifted by one"] = clip_expr(cos, ls, gg, B, (labels + 1) % N, F64)
                wrong["the last column left out of the row sum"] = clip_expr(cos, ls, gg, B, labels, F64, drop_last=True)
                wrong["the one-hot term dropped from dcos"] = clip_expr(cos, ls, gg, B, labels, F64, drop_onehot=True)
            if off > 0:
                wrong["label_offset dropped"] = clip_expr(cos, ls, gg, B, labels - off, F64)
            if N > B:
                wrong["label r instead of r % B in the second matrix"] = clip_expr(cos, ls, gg, B, (torch.arange(2 * B, device=DEV) + off) % N, F64)
            if ls0 == 5.0:
                wrong["the clamp removed"] = clip_expr(cos, ls, gg, B, labels, F64, clamp=False)
            assert wrong or N == 1
            for dname, w in wrong.items():      # (a far-off last column can vanish from an fp64 row sum: only what differs is asked)
                for k in ("loss_rows", "dcos"):
                    if dname == "the clamp removed" and k == "loss_rows" and c.regime == "equal":
                        continue    # equal logits at any scale: the loss is log N, only dcos carries the scale
                    if not torch.equal(w[k], ref[k]):
                        rejects(key_of("clip", k, c.regime), f"{what}: {k}, {dname}", got[k], w[k])
        assert fc.intact() and fs.intact() and fl.intact()


@dataclasses.dataclass
class CEL:
    rows: int
    cols: int
    regime: str

    @property
    def name(self):
        return f"cel_r{self.rows}_c{self.cols}_{self.regime}"


IGNORES = (-100, -1, 0)
CEL_SHAPES = [(r, c) for c in (65, 512) for r in (1, 5, 77)] + [(5, 49408)]
CEL_CASES = [CEL(r, c, reg) for r, c in CEL_SHAPES for reg in REGIMES] + [CEL(77, 16384, "gauss")]


def cel_labels(gen, R, N, ignore):
    """labels in [1, N); from 5 rows on: row 1 ignored, row 2 = N (beyond the columns), row 3 = -7 (negative, not the ignore index)"""
    lab = torch.randint(1, N, (R,), generator=gen)
    if R >= 5:
        lab[1], lab[2], lab[3] = ignore, N, -7
    return lab


def cel_expr(z, labels, ok, gs, dt, **defect):
    okf = ok.to(dt)
    lse, loss, d = xent(z.to(dt), labels, **defect)
    return {"lse": lse, "loss_rows": loss * okf, "dlogits": gs.to(dt) * d * okf[:, None]}


@pytest.mark.parametrize("c", CEL_CASES, ids=[c.name for c in CEL_CASES])
def test_ce_labels(c):
    R, N = c.rows, c.cols
    for ignore in IGNORES:
        name = f"{c.name}_ign{ignore}"
        gen = seeded(name)
        lab = cel_labels(gen, R, N, ignore)
        z = logits_of(c.regime, gen, R, N, lab)
        lab = lab.to(DEV)
        ok = (lab != ignore) & (lab >= 0) & (lab < N)
        assert int(ok.sum()) == (R - 3 if R >= 5 else R)
        safe = torch.where(ok, lab, torch.zeros_like(lab))
        g, inv = scalar(0.37), scalar(1.0) / float(ok.sum())
        fz, flab, fg, fi = put(z), put(lab), put(g), put(inv)
        fl, fr, fv, fd = Frame((R,), F32), Frame((R,), F32), Frame((R,), F32), Frame((R, N), F32)
        run_twice(name + " fwd", lambda: lib_call("segclip_ce_labels_fwd", fz.p, flab.p, ignore, fl.p, fr.p, fv.p, R, N), [fl, fr, fv])
        run_twice(name + " bwd", lambda: lib_call("segclip_ce_labels_bwd", fz.p, fl.p, flab.p, ignore, fg.p, fi.p, fd.p, R, N), [fd])
        assert all(f.intact() for f in (fz, flab, fg, fi, fl))
        assert torch.equal(fv.v, ok.float()), f"{name}: valid"
        assert exact_zero(fr.v[~ok]) and exact_zero(fd.v[~ok]), f"{name}: a row without a label has loss 0 and a zero gradient row"
        gs32 = g[0] * inv[0]
        gs64 = g[0].double() * inv[0].double()
        ref = cel_expr(z, safe, ok, gs64, F64)
        r32 = cel_expr(z, safe, ok, gs32, F32) if measuring() else {}
        got = {"lse": fl.v, "loss_rows": fr.v, "dlogits": fd.v}
        for k in got:
            judge(key_of("cel", k, c.regime), f"{name}: {k}", got[k], ref[k], r32.get(k))
        wrong = {"the label column shifted by one": cel_expr(z, (safe + 1) % N, ok, gs64, F64),
                 "the last column left out of the row sum": cel_expr(z, safe, ok, gs64, F64, drop_last=True),
                 "the one-hot term dropped": cel_expr(z, safe, ok, gs64, F64, drop_onehot=True)}
        if R >= 5:
            wrong["the row with label -7 given label 0"] = cel_expr(z, safe, ok | (lab == -7), gs64, F64)
        for dname, w in wrong.items():
            for k in ("loss_rows", "dlogits"):
                if dname.startswith("the last column") and k == "dlogits" and N == 49408:
                    continue        # one column of 49408 moves the loss by more than the bound, the probabilities by less
                if not torch.equal(w[k], ref[k]):
                    rejects(key_of("cel", k, c.regime), f"{name}: {k}, {dname}", got[k], w[k])


def test_ce_labels_every_row_ignored():
    """ops.CrossEntropyLabelsFn with no labelled row: 0 / 0 = NaN as torch's cross_entropy, and a gradient of exact zeros"""
    R, N = 5, 65
    z = draw(seeded("cel_all_ignored"), R, N).requires_grad_()
    lab = torch.full((R,), -100, dtype=torch.int64, device=DEV)
    loss = ops.CrossEntropyLabelsFn.apply(z, lab, -100)
    assert math.isnan(float(loss.detach())) and math.isnan(float(Fn.cross_entropy(z.detach(), lab, ignore_index=-100)))
    loss.backward()
    assert z.grad.shape == z.shape and exact_zero(z.grad) and bool(z.grad.isfinite().all())


# ---- superpixel KL -----------------------------------------------------------------------------------------------------------
SP_LAYOUTS = ("one", "distinct", "few", "negative", "bit32")


@dataclasses.dataclass
class SP:
    name: str
    B: int
    G: int
    T: int
    layout: str
    real: bool = False


def _sp_cases():
    cases = []
    for n, (G, T) in enumerate(itertools.product((1, 3, 8, 16), (1, 7, 196, 255, 256, 257, 577))):
        cases.append(SP(f"sp_g{G}_t{T}", 2 + n % 2, G, T, SP_LAYOUTS[n % 5], real=(G, T) in ((3, 196), (8, 257))))
    cases.append(SP("sp_lds_limit", 2, 8, 1666, "few"))
    return cases


SP_CASES = _sp_cases()


def sp_labels(gen, layout, B, T):
    if layout == "one":
        return torch.full((B, T), 11, dtype=torch.int64)
    if layout == "distinct":
        return torch.stack([torch.randperm(T, generator=gen) for _ in range(B)]) * 3 + 1
    pool = {"few": [0, 1, 2, 3, 250], "negative": [-3, -1, 2, -(2 ** 40)], "bit32": [5, 5 + 2 ** 32, 9]}[layout]
    return torch.tensor(pool, dtype=torch.int64)[torch.randint(0, len(pool), (B, T), generator=gen)]


def sp_expr(hard, seg, dt, skip_last=False, detach_mean=False):
    """the symmetric KL between hard and its superpixel mean as tests/test_kernels_gpu.py writes it, per image, and its
    gradient in hard"""
    B, G, T = hard.shape
    hr = hard.to(dt).clone().requires_grad_()
    h = hr.permute(0, 2, 1)
    eq = (seg.unsqueeze(-1) == seg.unsqueeze(-2))
    if skip_last:
        ar = torch.arange(T, device=seg.device)
        last = torch.where(eq, ar.view(1, 1, T), torch.tensor(-1, device=seg.device)).max(-1).values      # (B, T)
        eq = eq & (ar.view(1, 1, T) != last.unsqueeze(-1))
    eq = eq.to(dt)
    cm = (eq @ h) / torch.clamp_min(eq.sum(-1, keepdim=True), 1.0)
    if detach_mean:
        cm = cm.detach()
    coef = float(B * T * G)
    rows = (Fn.kl_div(Fn.log_softmax(h, -1), Fn.softmax(cm, -1), reduction="none").sum((1, 2)) / coef
            + Fn.kl_div(Fn.log_softmax(cm, -1), Fn.softmax(h, -1), reduction="none").sum((1, 2)) / coef) / 2
    rows.sum().backward()
    return {"loss_rows": rows.detach(), "dhard": hr.grad}


@pytest.mark.parametrize("c", SP_CASES, ids=[c.name for c in SP_CASES])
def test_superpixel_kl(c):
    B, G, T = c.B, c.G, c.T
    gen = seeded(c.name)
    if c.real:
        hard = draw(gen, B, G, T)
    else:
        hard = Fn.one_hot(torch.randint(0, G, (B, T), generator=gen), G).permute(0, 2, 1).float().contiguous().to(DEV)
    seg = sp_labels(gen, c.layout, B, T).to(DEV)
    fh, fs = put(hard), put(seg)
    fl, fd = Frame((B,), F32), Frame((B, G, T), F32)
    run_twice(c.name, lambda: lib_call("segclip_superpixel_kl", fh.p, fs.p, fl.p, fd.p, B, G, T), [fl, fd])
    assert fh.intact() and fs.intact()
    got = {"loss_rows": fl.v, "dhard": fd.v}
    if G == 1 or T == 1 or c.layout == "distinct":
        # one group (softmax is 1 everywhere) or every patch its own superpixel (the mean is the patch): the loss and its gradient
        # are 0, and the kernel, which forms both distributions by the same instructions, returns exact zeros.  The torch
        # expression leaves rounding noise there (log(softmax) against log_softmax: 1e-17 in fp64, 1e-9 in fp32) - no yardstick.
        assert exact_zero(fl.v) and exact_zero(fd.v), f"{c.name}: the loss and its gradient are exactly 0"
    else:
        ref = sp_expr(hard, seg, F64)
        r32 = sp_expr(hard, seg, F32) if measuring() else {}
        for k in got:
            judge(f"sp.{k}", f"{c.name}: {k}", got[k], ref[k], r32.get(k))
        rejects("sp.dhard", f"{c.name}: dhard without the path through the mean", fd.v, sp_expr(hard, seg, F64, detach_mean=True)["dhard"])
    if G == 1:
        return
    w = sp_expr(hard, seg, F64, skip_last=True)
    for k in got:       # (one member of several hundred moves the gradient by more than the bound, the loss only up to T = 257)
        if k == "dhard" or T <= 257:
            rejects(f"sp.{k}", f"{c.name}: {k}, the mean without the superpixel's last member", got[k], w[k])
    if c.layout == "bit32" and T > 1:
        w = sp_expr(hard, seg & 0xFFFFFFFF, F64)
        for k in got:
            rejects(f"sp.{k}", f"{c.name}: {k}, 5 and 5 + 2^32 merged", got[k], w[k])


# ---- masked MSE --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class MSE:
    B: int
    T: int
    Dp: int
    dtype: torch.dtype

    @property
    def name(self):
        return f"mse_b{self.B}_t{self.T}_d{self.Dp}_{'bf16' if self.dtype == BF else 'f32'}"


MSE_CASES = ([MSE(B, T, Dp, dt) for B, T in ((1, 1), (5, 1), (1, 5), (197, 1), (1, 197)) for Dp in (4, 48, 65, 588, 768) for dt in (F32, BF)]
             + [MSE(8, 197, 768, F32)])


def mse_mask(gen, B, T):
    """(B, 1 + T): the CLS entry 0.25 (never read), about 70 % ones; flat row 0 kept, flat row 1 = 0.5, sample 2 all zero"""
    m = (torch.rand(B, T + 1, generator=gen, dtype=F64) > 0.3).float()
    m[:, 0] = 0.25
    flat = m[:, 1:].reshape(-1).clone()
    flat[0] = 1.0
    if B * T >= 5:
        flat[1] = 0.5
        flat[-1] = 0.0
    m[:, 1:] = flat.view(B, T)
    if B >= 5:
        m[2, 1:] = 0.0
    return m


def mse_expr(pred, target, mask_rows, msum, g, dt, two=2.0):
    """mask_rows (B, T): the mask of the tokens; loss_rows (B T), dpred (B, 1 + T, Dp) of g * sum(loss_rows) / msum"""
    B, T, Dp = target.shape
    e = pred.to(dt)[:, 1:] - target.to(dt)
    mk = mask_rows.to(dt)
    gs = g.to(dt) / msum.to(dt) * two / Dp
    dp = torch.zeros(B, T + 1, Dp, dtype=dt, device=pred.device)
    dp[:, 1:] = gs * mk.unsqueeze(-1) * e
    return {"loss_rows": ((e * e).mean(-1) * mk).reshape(B * T), "dpred": dp}


@pytest.mark.parametrize("c", MSE_CASES, ids=[c.name for c in MSE_CASES])
def test_masked_mse(c):
    B, T, Dp = c.B, c.T, c.Dp
    gen = seeded(c.name)
    pred, target, mask = draw(gen, B, T + 1, Dp, dtype=c.dtype), draw(gen, B, T, Dp), mse_mask(gen, B, T).to(DEV)
    msum, g = mask[:, 1:].sum().reshape(1), scalar(1.3)
    fp, ft, fm, fs, fg = put(pred), put(target), put(mask), put(msum), put(g)
    fl, fd = Frame((B * T,), F32), Frame((B, T + 1, Dp), c.dtype)
    run_twice(c.name + " fwd", lambda: lib_call("segclip_masked_mse_fwd", fp.p, ft.p, fm.p, fl.p, B, T, Dp, L.dt(pred)), [fl])
    run_twice(c.name + " bwd", lambda: lib_call("segclip_masked_mse_bwd", fp.p, ft.p, fm.p, fg.p, fs.p, 1.0, fd.p, B, T, Dp, L.dt(pred)), [fd])
    assert all(f.intact() for f in (fp, ft, fm, fs, fg))
    ref = mse_expr(pred, target, mask[:, 1:], msum, g, F64)
    r32 = mse_expr(pred, target, mask[:, 1:], msum, g, F32) if measuring() else {}
    bf = c.dtype == BF
    judge("mse.loss_rows", f"{c.name}: loss_rows", fl.v, ref["loss_rows"], r32.get("loss_rows"))
    if bf:
        judge("mse.dpred_bf16", f"{c.name}: dpred", fd.v, ref["dpred"], rtol=RT_BF)
    else:
        judge("mse.dpred", f"{c.name}: dpred", fd.v, ref["dpred"], r32.get("dpred"))
    assert exact_zero(fd.v[:, 0]), f"{c.name}: the CLS row of dpred"
    dead = (mask[:, 1:] == 0)
    assert exact_zero(fl.v.view(B, T)[dead]) and exact_zero(fd.v[:, 1:][dead]), f"{c.name}: rows outside the mask"
    if B >= 5:
        assert bool(dead[2].all()) and not bool(dead.all()), "sample 2 is the one without masked tokens"
    w = mse_expr(pred, target, mask[:, :T], msum, g, F64)
    rejects("mse.loss_rows", f"{c.name}: loss_rows, the mask of token t for 1 + t", fl.v, w["loss_rows"])
    rejects("mse.dpred", f"{c.name}: dpred, the mask of token t for 1 + t", fd.v, w["dpred"], rtol=RT_BF if bf else None)
    rejects("mse.dpred", f"{c.name}: dpred, 1 / Dp for 2 / Dp", fd.v, mse_expr(pred, target, mask[:, 1:], msum, g, F64, two=1.0)["dpred"],
            rtol=RT_BF if bf else None)


# ---- max over the tokens -------------------------------------------------------------------------------------------------------
MT_CASES = [(3, T, D) for T in (1, 2, 4, 5, 8, 9, 37) for D in (4, 64, 768)] + [(48, 150, 768)]


def first_max(x):
    """index of the first maximum along dim 1, spelled out (ties: the lowest index)"""
    T = x.shape[1]
    ar = torch.arange(T, device=x.device).view(1, T, 1).expand_as(x)
    return torch.where(x == x.max(1, keepdim=True).values, ar, torch.full_like(ar, T)).min(1).values


@pytest.mark.parametrize("B,T,D", MT_CASES, ids=[f"mt_b{B}_t{T}_d{D}" for B, T, D in MT_CASES])
def test_max_tokens(B, T, D):
    name = f"mt_b{B}_t{T}_d{D}"
    gen = seeded(name)
    x, g = draw(gen, B, T, D), draw(gen, B, D)
    x[0, 0, 0] = x[0, T - 1, 0] = 9.0       # two equal maxima, the first and the last token
    x[1, :, 1] = 0.5                          # every token equal
    fx, fg = put(x), put(g)
    fo, fi = Frame((B, D), F32), Frame((B, D), torch.int32)
    run_twice(name + " fwd", lambda: lib_call("segclip_max_tokens_fwd", fx.p, fo.p, fi.p, B, T, D), [fo, fi])
    idx = first_max(x)
    assert int(idx[0, 0]) == 0 and int(idx[1, 1]) == 0, "the ties are meant to be won by the lowest index"
    assert torch.equal(fo.v, x.max(1).values), f"{name}: the maximum"
    assert torch.equal(fi.v.long(), idx), f"{name}: idx is not the first maximum at every column"
    dx = torch.where(idx.unsqueeze(1) == torch.arange(T, device=DEV).view(1, T, 1), g.unsqueeze(1), torch.zeros((), device=DEV))
    for want32, want16 in ((True, True), (False, True), (True, False)):
        what = f"{name} bwd dx {'set' if want32 else 'null'} dx_bf16 {'set' if want16 else 'null'}"
        f32, f16 = Frame((B, T, D), F32), Frame((B, T, D), BF)
        run_twice(what, lambda: lib_call("segclip_max_tokens_bwd", fg.p, fi.p, f32.p if want32 else None, f16.p if want16 else None, B, T, D),
                  ([f32] if want32 else []) + ([f16] if want16 else []))
        if want32:
            assert torch.equal(f32.v, dx), f"{what}: dx"
        else:
            assert f32.untouched()
        if want16:
            assert torch.equal(f16.v, dx.to(BF)), f"{what}: the bf16 copy"
        else:
            assert f16.untouched()
    assert fx.intact() and fg.intact() and fi.intact()
    assert B * (D // 4) % 128 != 0 or B == 48
    if T >= 2:
        assert not torch.equal(first_max(x.flip(1)), idx), "the last maximum is another index somewhere"


# ---- reduce_sum, scale ---------------------------------------------------------------------------------------------------------
RS_N = (1, 63, 1023, 1024, 1025, 100003)
RS_K = 16


@pytest.mark.parametrize("n", RS_N)
def test_reduce_sum(n):
    """sixteen vectors of n elements around 0.5, one launch each into one framed output of sixteen"""
    name = f"rs_n{n}"
    x = draw(seeded(name), RS_K, n) + 0.5
    fx, fo = put(x), Frame((RS_K,), F32)

    def call():
        for k in range(RS_K):
            lib_call("segclip_reduce_sum", L.ptr(fx.v[k]), L.ptr(fo.v[k:]), n, 0.37)
    run_twice(name, call, [fo])
    assert fx.intact()
    s32 = float(torch.tensor(0.37, dtype=F32))
    ref = x.double().sum(-1) * s32
    judge("reduce.out", f"{name}: sums", fo.v, ref, (x.sum(-1) * s32) if measuring() else None)
    if n >= 2:
        rejects("reduce.out", f"{name}: the last element replaced by its neighbour", fo.v, ref + (x[:, -2] - x[:, -1]).double() * s32)


@pytest.mark.parametrize("n", RS_N + (1100003,))
def test_scale(n):
    name = f"scale_n{n}"
    x, s = draw(seeded(name), n), scalar(0.37)
    fx, fs, fo = put(x), put(s), Frame((n,), F32)
    run_twice(name, lambda: lib_call("segclip_scale", fx.p, fs.p, fo.p, n), [fo])
    assert fx.intact() and fs.intact()
    ref = x.double() * s.double()
    judge("scale", f"{name}: out", fo.v, ref, rtol=RT_MUL)
    if n >= 2:
        w = ref.clone()
        w[-1] = ref[-2]
        rejects("scale", f"{name}: the last element replaced by its neighbour", fo.v, w, rtol=RT_MUL)


# ---- gates -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,T", [(17, 7), (8, 1667)])
def test_gate_superpixel_limits(G, T):
    """G = 16 and T = 1666 at G = 8 are rows above; one more of either is refused before anything is launched"""
    B = 2
    gen = seeded(f"gate_sp_{G}_{T}")
    fh, fs = put(draw(gen, B, G, T)), put(sp_labels(gen, "few", B, T).to(DEV))
    fl, fd = Frame((B,), F32), Frame((B, G, T), F32)
    with pytest.raises(RuntimeError):
        lib_call("segclip_superpixel_kl", fh.p, fs.p, fl.p, fd.p, B, G, T)
    with pytest.raises(RuntimeError):
        ops.SuperpixelKLFn.apply(fh.v, fs.v)
    torch.cuda.synchronize()
    assert fl.untouched() and fd.untouched() and fh.intact() and fs.intact()


@pytest.mark.parametrize("dtype,ok", [(torch.int32, True), (torch.uint8, True), (torch.float32, False), (torch.bool, False)])
def test_gate_superpixel_label_types(dtype, ok):
    B, G, T = 2, 8, 50
    gen = seeded("gate_sp_types")
    hard = draw(gen, B, G, T)
    seg = torch.randint(0, 2, (B, T), generator=gen).to(DEV)
    fh = put(hard)
    hv = fh.v.detach().requires_grad_()
    if not ok:
        with pytest.raises(TypeError):
            ops.SuperpixelKLFn.apply(hv, seg.to(dtype))
        torch.cuda.synchronize()
        assert fh.intact() and torch.equal(fh.v, hard) and hv.grad is None
        return
    loss = ops.SuperpixelKLFn.apply(hv, seg.to(dtype))
    loss.backward()
    ref = sp_expr(hard, seg, F64)
    judge("sp.loss_rows", f"{dtype} labels: loss", loss.reshape(1), ref["loss_rows"].sum().reshape(1))
    judge("sp.dhard", f"{dtype} labels: dhard", hv.grad, ref["dhard"])


def test_gate_cross_entropy_offset():
    R, N, off = 5, 65, 61
    fz = put(draw(seeded("gate_ce"), R, N))
    fl, fr = Frame((R,), F32), Frame((R,), F32)
    with pytest.raises(RuntimeError):
        lib_call("segclip_ce_fwd", fz.p, fl.p, fr.p, R, N, off)
    zv = fz.v.detach().requires_grad_()
    with pytest.raises(RuntimeError):
        ops.CrossEntropyFn.apply(zv, off)
    torch.cuda.synchronize()
    assert fl.untouched() and fr.untouched() and fz.intact() and zv.grad is None
    judge("ce.loss_rows", "offset 60 fits", ops.CrossEntropyFn.apply(zv, off - 1).reshape(1),
          Fn.cross_entropy(fz.v.double(), torch.arange(R, device=DEV) + off - 1).reshape(1))


def test_gate_clip_loss_rank():
    """one process: the gathered batch is the batch, so only rank 0 fits"""
    B, C = 4, 64
    gen = seeded("gate_clip")
    fv, ft = put(draw(gen, B, C)), put(draw(gen, B, C))
    v, t = fv.v.detach().requires_grad_(), ft.v.detach().requires_grad_()
    ls = torch.tensor(2.0, device=DEV, requires_grad=True)
    box = {}
    with pytest.raises(ValueError):
        ops.ClipLossFn.apply(v, t, ls, 1, box)
    torch.cuda.synchronize()
    assert box == {} and fv.intact() and ft.intact() and v.grad is None and ls.grad is None
    assert bool(ops.ClipLossFn.apply(v, t, ls, 0, box).isfinite()) and "cos" in box


# ---- the tables reach every edge -----------------------------------------------------------------------------------------------
def test_rows_reach_every_edge():
    assert {r for r, _ in L2_CASES} == {1, 3, 4, 5, 33} and {c for _, c in L2_CASES} == {1, 63, 64, 65, 512, 768}
    assert {r % 4 for r, _ in L2_CASES} == {0, 1, 3} and {(2 * r) % 4 for r, _ in L2_CASES} == {0, 2}
    ce = [c for c in CE_CASES if c.rows * c.cols <= GRID_CAP]
    assert {c.rows for c in ce} == {1, 3, 4, 5, 77} and {c.cols for c in ce} == {1, 63, 64, 65, 512}
    assert {c.rows % 4 for c in ce} == {0, 1, 3} and all(c.rows == 1 for c in ce if c.cols == 1)
    for fam in (CE_CASES, CLIP_CASES, CEL_CASES):
        assert {c.regime for c in fam} == set(REGIMES)
    for c in CE_CASES:
        if c.cols - c.rows >= 2:
            o = c.offsets
            assert len(o) == 3 and o[0] == 0 and 0 < o[1] < o[2] == c.cols - c.rows
    assert {c.B for c in CLIP_CASES} == {1, 3, 8, 33} and {(2 * c.B) % 4 for c in CLIP_CASES} == {0, 2}
    for B in (1, 3, 8, 33):
        assert {c.N for c in CLIP_CASES if c.B == B} == {B, 2 * B + 1, 8 * B}
    for c in CLIP_CASES:
        assert c.offsets == ([0] if c.N == c.B else sorted({0, c.B, c.N - c.B}))
    assert sum(math.exp(s) <= 100 for s in LOGIT_SCALES) == 2 and math.exp(4.6) > 99 and math.exp(5.0) > 100
    cel = [c for c in CEL_CASES if c.rows * c.cols <= GRID_CAP]
    assert {c.rows for c in cel} == {1, 5, 77} and {c.cols for c in cel} == {65, 512, 49408}
    assert all(c.rows == 5 for c in cel if c.cols == 49408) and set(IGNORES) == {-100, -1, 0}
    sp = [c for c in SP_CASES if c.name != "sp_lds_limit"]
    assert {c.G for c in sp} == {1, 3, 8, 16} and {c.T for c in sp} == {1, 7, 196, 255, 256, 257, 577}
    assert {c.layout for c in sp if c.G > 1 and c.T > 1} == set(SP_LAYOUTS) and sum(c.real for c in sp) == 2 and {c.B for c in sp} == {2, 3}
    lim = SP_CASES[-1]
    assert lim.T * lim.G * 4 + lim.T * 4 == 59976 <= 60000 < (lim.T + 1) * (lim.G * 4 + 4) and lim.B == 2
    mse = [c for c in MSE_CASES if c.B * (c.T + 1) * c.Dp <= GRID_CAP]
    assert {c.B * c.T for c in mse} == {1, 5, 197} and {c.Dp for c in mse} == {4, 48, 65, 588, 768} and {c.dtype for c in mse} == {F32, BF}
    mt = [r for r in MT_CASES if r[0] * r[1] * r[2] // 4 <= GRID_CAP]
    assert {T for _, T, _ in mt} == {1, 2, 4, 5, 8, 9, 37} and {D for _, _, D in mt} == {4, 64, 768}
    assert {(T - 1) % 4 for _, T, _ in mt} == {0, 1, 3} and all(B * (D // 4) % 128 for B, _, D in mt)
    # the grid-stride rows: one per kernel whose launch is capped at 4096 blocks of 256 threads
    assert sum(c.rows * c.cols > GRID_CAP for c in CE_CASES) == 1 and sum(c.rows * c.cols > GRID_CAP for c in CEL_CASES) == 1
    assert sum(c.B * (c.T + 1) * c.Dp > GRID_CAP for c in MSE_CASES) == 1 and sum(B * T * D // 4 > GRID_CAP for B, T, D in MT_CASES) == 1
    assert set(RS_N) == {1, 63, 1023, 1024, 1025, 100003}


# ---- the measurement behind FLOORS -----------------------------------------------------------------------------------------------
def value_rows():
    """(test function, arguments) of every row that judges values"""
    rows = [(test_l2norm, r) for r in L2_CASES] + [(test_l2norm_pair, r) for r in L2_CASES]
    rows += [(test_ce, (c,)) for c in CE_CASES] + [(test_clip_ce, (c,)) for c in CLIP_CASES] + [(test_ce_labels, (c,)) for c in CEL_CASES]
    rows += [(test_superpixel_kl, (c,)) for c in SP_CASES] + [(test_masked_mse, (c,)) for c in MSE_CASES]
    rows += [(test_reduce_sum, (n,)) for n in RS_N]
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
