"""GPU: every C-ABI kernel against a plain PyTorch fp32 reference of the same op (same seeded inputs),
through the same ctypes boundary the product uses.  Integer outputs are compared bit-exactly."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import segclip_amd  # noqa: E402
from segclip_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32


def rnd(*shape, dtype=F32, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed + 131 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def close(got, ref, rtol, atol, what=""):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = err > tol
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e}, "
                                 f"ref max {float(ref.abs().max()):.3e}")


TOL = {F32: (2e-5, 2e-5), BF: (2e-2, 2e-2)}


# ------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (200, 136, 72), (784, 2304, 768), (33, 8, 8), (1, 512, 512)])
def test_gemm_nt_bias_act_residual(dtype, M, N, K):
    if dtype == BF and K % 8:
        pytest.skip("bf16 path needs K % 8 == 0")
    x, w = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, seed=2, scale=K ** -0.5)
    b, r = rnd(N, seed=3), rnd(M, N, seed=4)
    ref_u = x.float() @ w.float().t() + b
    rt, at = TOL[dtype]
    y, _ = ops.p_linear(x, w, b)
    close(y, ref_u, rt, at, "plain")
    for act, f in ((ops.ACT_QUICK_GELU, lambda u: u * torch.sigmoid(1.702 * u)),
                   (ops.ACT_GELU_ERF, lambda u: torch.nn.functional.gelu(u))):
        y, u = ops.p_linear(x, w, b, act=act, residual=r, want_aux=True, out_dtype=F32)
        close(u, ref_u, rt, at, "aux")
        close(y, f(ref_u) + r, rt, at, f"act{act}+res")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (200, 136, 72), (784, 768, 3072), (50, 64, 8)])
def test_gemm_dgrad_wgrad_layouts(dtype, M, N, K):
    """dgrad (k-strided B via the LDS transpose read) and wgrad (both operands k-strided)."""
    if dtype == BF and (K % 8 or N % 8):
        pytest.skip("bf16 path needs 16-byte rows")
    dy, w, x = rnd(M, N, dtype=dtype, seed=5), rnd(N, K, dtype=dtype, seed=6, scale=N ** -0.5), rnd(M, K, dtype=dtype, seed=7)
    rt, at = TOL[dtype]
    dx = ops.p_dgrad(dy, w, dtype)
    close(dx, dy.float() @ w.float(), rt, at * math.sqrt(N / 64 + 1), "dgrad")
    dw = ops.p_wgrad(dy, x)
    close(dw, dy.float().t() @ x.float(), rt, at * math.sqrt(M / 64 + 1), "wgrad")
    u = rnd(M, K, dtype=dtype, seed=8)
    du = ops.p_dgrad(dy, w, dtype, aux=u, act=ops.ACT_QUICK_GELU)
    s = torch.sigmoid(1.702 * u.float())
    close(du, (dy.float() @ w.float()) * (s * (1 + 1.702 * u.float() * (1 - s))), rt, at * math.sqrt(N / 64 + 1), "dgrad*dact")
    # w stored (K_in, N_out) like visual.proj / text_projection
    wkn = rnd(K, N, dtype=dtype, seed=9, scale=K ** -0.5)
    y, _ = ops.p_linear(x, wkn, None, w_kn=True)
    close(y, x.float() @ wkn.float(), rt, at * math.sqrt(K / 64 + 1), "w_kn fwd")
    close(ops.p_dgrad(dy, wkn, dtype, w_kn=True), dy.float() @ wkn.float().t(), rt, at * math.sqrt(N / 64 + 1), "w_kn dgrad")
    close(ops.p_wgrad(dy, x, w_kn=True), x.float().t() @ dy.float(), rt, at * math.sqrt(M / 64 + 1), "w_kn wgrad")


def test_gemm_fused_colsum_epilogue():
    """dgrad * act'(u) with the bias-gradient column sums produced by the LDS epilogue."""
    M, N, K = 512, 256, 512
    dy, w, u = rnd(M, N, dtype=BF, seed=14), rnd(N, K, dtype=BF, seed=15, scale=N ** -0.5), rnd(M, K, dtype=BF, seed=16)
    du, cs = ops.p_dgrad(dy, w, BF, aux=u, act=ops.ACT_QUICK_GELU, want_colsum=True)
    s = torch.sigmoid(1.702 * u.float())
    ref = (dy.float() @ w.float()) * (s * (1 + 1.702 * u.float() * (1 - s)))
    close(du, ref, 2e-2, 2e-2, "du")
    close(cs, ref.sum(0), 2e-2, 0.05, "fused colsum")
    du2, cs2 = ops.p_dgrad(dy[:200], w, BF, aux=u[:200].contiguous(), act=ops.ACT_QUICK_GELU, want_colsum=True)  # fallback path
    close(cs2, ref[:200].sum(0), 2e-2, 0.05, "fallback colsum")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,N,K", [(512, 512, 128), (200, 136, 72), (784, 3072, 768), (256, 128, 64)])
def test_gemm_saved_activation_derivative(dtype, M, N, K):
    """aux_kind 1: the activation epilogue stores act'(u) instead of u, the act' dgrad multiplies by it as it is
    (what the residual blocks do in bf16 mode); every bf16 kernel (8-phase, one-barrier DMA, register-staged) + f32."""
    x, w, b = rnd(M, K, dtype=dtype, seed=51), rnd(N, K, dtype=dtype, seed=52, scale=K ** -0.5), rnd(N, seed=53)
    pre = x.float() @ w.float().t() + b
    sg = torch.sigmoid(1.702 * pre)
    dref = sg * (1 + 1.702 * pre * (1 - sg))
    rt, at = TOL[dtype]
    y, a1 = ops.p_linear(x, w, b, act=ops.ACT_QUICK_GELU, want_aux=True, aux_kind=1)
    close(y, pre * sg, rt, at, "act")
    close(a1, dref, rt, at, "saved derivative")
    y0, a0 = ops.p_linear(x, w, b, act=ops.ACT_QUICK_GELU, want_aux=True, aux_kind=0)
    close(a0, pre, rt, at, "saved pre-activation")
    assert torch.equal(y0, y)
    g, w2 = rnd(M, K, dtype=dtype, seed=54), rnd(K, N, dtype=dtype, seed=55, scale=K ** -0.5)   # c_proj: (D, 4D)
    du1 = ops.p_dgrad(g, w2, dtype, aux=a1, act=ops.ACT_QUICK_GELU, aux_kind=1)
    close(du1, (g.float() @ w2.float()) * a1.float(), rt, at * 2, "dgrad * saved derivative")
    du0 = ops.p_dgrad(g, w2, dtype, aux=a0, act=ops.ACT_QUICK_GELU, aux_kind=0)
    close(du0, du1, 3 * rt, at * 4, "both kinds agree")
    with pytest.raises(RuntimeError):       # erf-GELU keeps the pre-activation
        ops.p_linear(x, w, b, act=ops.ACT_GELU_ERF, want_aux=True, aux_kind=1)


@pytest.mark.parametrize("M,N,K,pad", [(512, 512, 128, 0), (1024, 3072, 768, 512), (768, 2048, 512, 0)])
def test_gemm_saved_derivative_one_byte(M, N, K, pad):
    """aux_kind 2 (what the towers keep in bf16 mode on full 256 x 256 tiles): act'(u) as one byte per element,
    q = rint((act' + 0.125) * 204): the forward output is unchanged, the decoded derivative is within half a step (1/408)
    of the bf16 one, and the act' data gradient multiplies by the decoded value; pitched outputs; ragged shapes refuse."""
    x, w, b = rnd(M, K, dtype=BF, seed=61), rnd(N, K, dtype=BF, seed=62, scale=K ** -0.5), rnd(N, seed=63)
    pre = x.float() @ w.float().t() + b
    sg = torch.sigmoid(1.702 * pre)
    dref = sg * (1 + 1.702 * pre * (1 - sg))
    y1, a1 = ops.p_linear(x, w, b, act=ops.ACT_QUICK_GELU, want_aux=True, aux_kind=1)
    y2, a2 = ops.p_linear(x, w, b, act=ops.ACT_QUICK_GELU, want_aux=True, aux_kind=2, pitched=pad > 0)
    assert a2.dtype == torch.uint8 and a2.shape == (M, N)
    assert torch.equal(y1, y2)
    dec = a2.float() / 204.0 - 0.125
    assert float((dec - dref).abs().max()) <= 0.5 / 204.0 + 2e-2 * 0.02 + 4e-3   # half a step + the bf16 accumulate noise of pre
    assert float((dec - a1.float()).abs().max()) <= 0.5 / 204.0 + 5e-3
    g, w2 = rnd(M, K, dtype=BF, seed=64), rnd(K, N, dtype=BF, seed=65, scale=K ** -0.5)
    du2, cs = ops.p_dgrad(g, w2, BF, aux=a2, act=ops.ACT_QUICK_GELU, aux_kind=2, want_colsum=True, pitched=pad > 0)
    ref = (g.float() @ w2.float()) * dec
    close(du2, ref, 2e-2, 2e-2, "dgrad * decoded derivative")
    close(cs, du2.float().sum(0), 2e-3, 2e-2 * M ** 0.5, "fused column sums")
    # not a multiple of the 256-wide tiles: the library refuses aux_kind 2 (SEGCLIP_ERR_UNSUPPORTED, nothing launched) and
    # p_linear falls back to the bf16 form of the derivative (aux_kind 1) - same output, the backward reads the dtype
    y3, a3 = ops.p_linear(x[:200], w[:136], b[:136], act=ops.ACT_QUICK_GELU, want_aux=True, aux_kind=2)
    y4, a4 = ops.p_linear(x[:200], w[:136], b[:136], act=ops.ACT_QUICK_GELU, want_aux=True, aux_kind=1)
    assert a3.dtype == BF and torch.equal(a3, a4) and torch.equal(y3, y4)
    with pytest.raises(RuntimeError):       # the raw launch still refuses
        aux = torch.empty(200, 136, dtype=torch.uint8, device=DEV)
        ops.p_gemm(x[:200], w[:136], torch.empty(200, 136, dtype=BF, device=DEV), 200, 136, K, (K, 1), (K, 1), 136, bias=b[:136],
                   aux=aux, ldaux=136, act=ops.ACT_QUICK_GELU, aux_kind=2)


@pytest.mark.parametrize("M,N,K,pad", [(16384, 1536, 384, 0), (16384 + 128, 1536, 384, 512), (32768, 768, 128, 0)])
def test_gemm_saved_derivative_one_byte_erf_gelu(M, N, K, pad):
    """aux_kind 2 with the erf-GELU of the MAE decoders (round 6; modules/module_mae.py:110-134 = timm Block with nn.GELU): the 256 x 256-
    tile GEMM evaluates erf by Abramowitz-Stegun 7.1.26 in its epilogue and stores act'(u) = Phi(u) + u phi(u) as one byte; the data
    gradient multiplies by the decoded byte.  Ragged shapes fall back to the saved pre-activation (aux_kind 0)."""
    x, w, b = rnd(M, K, dtype=BF, seed=66), rnd(N, K, dtype=BF, seed=67, scale=K ** -0.5), rnd(N, seed=68)
    pre = x.float() @ w.float().t() + b
    yref = torch.nn.functional.gelu(pre)
    cdf = 0.5 * (1 + torch.erf(pre * 2 ** -0.5))
    dref = cdf + pre * torch.exp(-0.5 * pre * pre) * (2 * math.pi) ** -0.5
    y0, a0 = ops.p_linear(x, w, b, act=ops.ACT_GELU_ERF, want_aux=True, aux_kind=0)       # the 8-phase kernel, erff
    y2, a2 = ops.p_linear(x, w, b, act=ops.ACT_GELU_ERF, want_aux=True, aux_kind=2, pitched=pad > 0)
    assert a2.dtype == torch.uint8 and a2.shape == (M, N) and a0.dtype == BF
    close(y2, yref, 2e-2, 2e-2, "erf-GELU forward")
    close(y2, y0.float(), 1.6e-2, 1e-3, "both kernels' erf-GELU agree to a bf16 step")
    dec = a2.float() / 204.0 - 0.125
    # half a step + saturation of the two extremes (act' in [-0.129, 1.129], representable [-0.125, 1.125]) + the bf16 noise of pre
    assert float((dec - dref).abs().max()) <= 0.5 / 204.0 + 0.0042 + 4e-3, float((dec - dref).abs().max())
    g, w2 = rnd(M, K, dtype=BF, seed=69), rnd(K, N, dtype=BF, seed=70, scale=K ** -0.5)
    du2, cs = ops.p_dgrad(g, w2, BF, aux=a2, act=ops.ACT_GELU_ERF, aux_kind=2, want_colsum=True, pitched=pad > 0)
    close(du2, (g.float() @ w2.float()) * dec, 2e-2, 2e-2, "dgrad * decoded derivative")
    close(cs, du2.float().sum(0), 2e-3, 2e-2 * M ** 0.5, "fused column sums")
    du0 = ops.p_dgrad(g, w2, BF, aux=a0, act=ops.ACT_GELU_ERF, aux_kind=0)
    close(du2, du0, 3e-2, 3e-2, "byte derivative against the recomputed one")
    # ragged shapes, and problems too small for the 256 x 256-tile kernel (the other kernels' byte epilogue is QuickGELU's): the byte
    # form is refused, p_linear keeps the pre-activation instead
    for r, c in ((200, 136), (512, 512)):
        y3, a3 = ops.p_linear(x[:r], w[:c], b[:c], act=ops.ACT_GELU_ERF, want_aux=True, aux_kind=2)
        y4, a4 = ops.p_linear(x[:r], w[:c], b[:c], act=ops.ACT_GELU_ERF, want_aux=True, aux_kind=0)
        assert a3.dtype == BF and torch.equal(a3, a4) and torch.equal(y3, y4)


@pytest.mark.parametrize("K", [64, 128, 192, 448])
def test_gemm_half_tile_tail_is_bit_identical(K):
    """gemm_bf16_pq.hip: a launch whose last round of 256 workgroups is at most half full runs those tiles as 128 x 256
    workgroups (3-slot operand ring, its own counted waits; K = 1, 2, 3 and 7 K-tiles walk the loop's end conditions).  Every
    epilogue of the towers (bias, + fp32 / bf16 residual, QuickGELU + one-byte derivative, data gradient, x derivative +
    column sums) must give the bits of the full-tile path: the same launch is repeated on two overlapping row ranges of 255
    tiles each (one round of full tiles, the same kernel, no tail), and checked against the fp32 torch product.  nn.Linear
    shapes of modules/module_seg_vit.py:162-196."""
    from segclip_amd import _lib
    lib = _lib.load()
    M, N, cut = 100 * 256, 768, 85 * 256
    assert lib.segclip_gemm_pq_half_tail(M // 256 * 3) == 44, "300 tiles plan no half-tile tail: the path under test is not reached"
    assert lib.segclip_gemm_pq_half_tail(cut // 256 * 3) == 0
    x, w, b = rnd(M, K, dtype=BF, seed=81), rnd(N, K, dtype=BF, seed=82, scale=K ** -0.5), rnd(N, seed=83)
    wk = rnd(K, N, dtype=BF, seed=84, scale=K ** -0.5)
    r32 = rnd(M, N, seed=85, scale=3.0)
    r16 = r32.to(BF)
    G = ops.ACT_QUICK_GELU

    def both(fn):
        whole = fn(slice(0, M))
        a, c = fn(slice(0, cut)), fn(slice(M - cut, M))      # the tail tiles are the last 15 row tiles: inside the second range
        whole = whole if isinstance(whole, tuple) else (whole,)
        a = a if isinstance(a, tuple) else (a,)
        c = c if isinstance(c, tuple) else (c,)
        return whole, a, c

    def same_rows(fn, what):
        whole, a, c = both(fn)
        for t, ta, tc in zip(whole, a, c):
            assert torch.equal(t[:cut], ta) and torch.equal(t[M - cut:], tc), what
        return whole

    y = same_rows(lambda r: ops.p_linear(x[r], w, b)[0], "bias")[0]
    close(y, x.float() @ w.float().t() + b, 2e-2, 2e-2, "bias epilogue vs fp32 torch")
    same_rows(lambda r: ops.p_linear(x[r], w, None)[0], "no bias")
    y32 = same_rows(lambda r: ops.p_linear(x[r], w, b, residual=r32[r], out_dtype=F32)[0], "fp32 residual")[0]
    close(y32, x.float() @ w.float().t() + b + r32, 2e-2, 2e-2, "fp32 residual epilogue vs fp32 torch")
    same_rows(lambda r: ops.p_linear(x[r], w, b, residual=r16[r])[0], "bf16 residual")
    dx = same_rows(lambda r: ops.p_dgrad(x[r], wk, BF), "data gradient")[0]
    close(dx, x.float() @ wk.float(), 2e-2, 2e-2, "data gradient vs fp32 torch")
    ya, u8 = same_rows(lambda r: tuple(ops.p_linear(x[r], w, b, act=G, want_aux=True, aux_kind=2)[:2]), "QuickGELU + one-byte derivative")
    assert u8.dtype == torch.uint8
    same_rows(lambda r: ops.p_dgrad(x[r], wk, BF, aux=u8[r], act=G, aux_kind=2), "x derivative")
    whole, a, c = both(lambda r: tuple(ops.p_dgrad(x[r], wk, BF, aux=u8[r], act=G, aux_kind=2, want_colsum=True)))
    assert torch.equal(whole[0][:cut], a[0]) and torch.equal(whole[0][M - cut:], c[0]), "x derivative (+ column sums)"
    close(whole[1], whole[0].float().sum(0), 2e-3, 2e-2 * M ** 0.5, "fused column sums")


@pytest.mark.parametrize("K", [64, 320])
def test_gemm_row_remainder_of_128_runs_as_half_tiles(K):
    """M = 256 q + 128 (an odd multiple of 128 samples x 197 tokens): the 256 x 256-tile kernel covers the last 128 rows with a
    row of half-tile workgroups.  Every epilogue against the same rows of a launch over 256 (q + 1) rows (one round of full
    tiles, same kernel): bit-identical; the one-byte derivative and the fused column sums are available on such shapes."""
    M2, N = 85 * 256, 768
    M = M2 - 128
    x, w, b = rnd(M2, K, dtype=BF, seed=91), rnd(N, K, dtype=BF, seed=92, scale=K ** -0.5), rnd(N, seed=93)
    wk = rnd(K, N, dtype=BF, seed=94, scale=K ** -0.5)
    r32 = rnd(M2, N, seed=95, scale=3.0)
    G = ops.ACT_QUICK_GELU

    def same(fn, what):
        big, part = fn(M2), fn(M)
        big = big if isinstance(big, tuple) else (big,)
        part = part if isinstance(part, tuple) else (part,)
        for t, u in zip(big, part):
            assert u.shape[0] == M and torch.equal(t[:M], u), what
        return part

    y = same(lambda m: ops.p_linear(x[:m], w, b)[0], "bias")[0]
    close(y, x[:M].float() @ w.float().t() + b, 2e-2, 2e-2, "bias epilogue vs fp32 torch")
    same(lambda m: ops.p_linear(x[:m], w, b, residual=r32[:m], out_dtype=F32)[0], "fp32 residual")
    same(lambda m: ops.p_dgrad(x[:m], wk, BF), "data gradient")
    ya, u8 = same(lambda m: tuple(ops.p_linear(x[:m], w, b, act=G, want_aux=True, aux_kind=2)[:2]), "QuickGELU + one-byte derivative")
    assert u8.dtype == torch.uint8, "the one-byte derivative must be available at M = 256 q + 128"
    dx, cs = ops.p_dgrad(x[:M], wk, BF, aux=u8, act=G, aux_kind=2, want_colsum=True)
    dx2, _ = ops.p_dgrad(x, wk, BF, aux=torch.cat([u8, u8[:128]], 0), act=G, aux_kind=2, want_colsum=True)
    assert torch.equal(dx, dx2[:M]), "x derivative"
    close(cs, dx.float().sum(0), 2e-3, 2e-2 * M ** 0.5, "fused column sums")


def test_gemm_bf16_fp32_A_operand_and_splitk():
    """fp32 residual-stream gradients as the A operand of the bf16 kernels; split-K wgrad (M >> tiles)."""
    M, N, K = 6272, 256, 128
    g = rnd(M, N, seed=11)
    w, h = rnd(N, K, dtype=BF, seed=12, scale=N ** -0.5), rnd(M, K, dtype=BF, seed=13)
    gb = g.to(BF).float()
    close(ops.p_dgrad(g, w, BF), gb @ w.float(), 2e-2, 2e-2, "dgrad fp32 A")
    close(ops.p_wgrad(g, h), gb.t() @ h.float(), 2e-2, 0.3, "wgrad fp32 A split-K")


@pytest.mark.parametrize("dtype", [F32, BF])
def test_bmm_strided_autograd(dtype):
    nb, M, N, K = 3, 8, 48, 64
    A = rnd(nb, M, K, dtype=dtype, seed=21).requires_grad_()
    Bm = rnd(nb, N, K, dtype=dtype, seed=22).requires_grad_()
    C1 = ops.bmm(A, Bm, transB=True, out_dtype=F32)
    ref = torch.einsum("bmk,bnk->bmn", A.float(), Bm.float())
    rt, at = TOL[dtype]
    close(C1, ref, rt, at * 4, "bmm NT")
    go = rnd(nb, M, N, seed=23)
    C1.backward(go)
    close(A.grad, torch.einsum("bmn,bnk->bmk", go, Bm.float()), rt, at * 4, "bmm dA")
    close(Bm.grad, torch.einsum("bmn,bmk->bnk", go, A.float()), rt, at * 4, "bmm dB")
    A2 = rnd(nb, M, N, dtype=dtype, seed=24).requires_grad_()
    B2 = rnd(nb, N, K, dtype=dtype, seed=25).requires_grad_()
    C2 = ops.bmm(A2, B2, transB=False, out_dtype=F32)
    close(C2, A2.float() @ B2.float(), rt, at * 4, "bmm NN")
    go2 = rnd(nb, M, K, seed=26)
    C2.backward(go2)
    close(A2.grad, go2 @ B2.float().transpose(1, 2), rt, at * 4, "bmm NN dA")
    close(B2.grad, A2.float().transpose(1, 2) @ go2, rt, at * 4, "bmm NN dB")


# ------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("cols", [64, 128, 384, 512, 768, 1024])
@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (F32, BF), (BF, F32)])
def test_layernorm_fwd_bwd(cols, xdt, ydt):
    rows = 197
    x = rnd(rows, cols, dtype=xdt, seed=31)
    w, b = 1 + 0.1 * rnd(cols, seed=32), 0.1 * rnd(cols, seed=33)
    y, mean, rstd = ops.p_ln_fwd(x, w, b, 1e-5, ydt)
    xr = x.float().requires_grad_()
    wr, br = w.clone().requires_grad_(), b.clone().requires_grad_()
    ref = torch.nn.functional.layer_norm(xr, (cols,), wr, br, 1e-5)
    rt, at = (2e-5, 2e-5) if ydt == F32 else (1e-2, 1e-2)
    close(y, ref, rt, at, "ln fwd")
    dy = rnd(rows, cols, dtype=ydt, seed=34)
    dres = rnd(rows, cols, dtype=F32, seed=35)
    dx, dw, db, dx16, dsum = ops.p_ln_bwd(dy, x, w, mean, rstd, dres=dres, dx_dtype=F32, want_bf16=True,
                                          want_dres_colsum=True)
    ref.backward(dy.float())
    close(dx, xr.grad + dres, 1e-4, 1e-4, "ln dx")
    assert torch.equal(dx16, dx.to(BF))
    close(dsum, dres.sum(0), 1e-5, 1e-4, "ln colsum(dres)")
    close(dw, wr.grad, 1e-4, 1e-3, "ln dgamma")
    close(db, br.grad, 1e-4, 1e-3, "ln dbeta")


@pytest.mark.parametrize("rows,cols", [(197, 768), (5000, 768), (77 * 9, 512), (64, 1024)])
@pytest.mark.parametrize("resdt", [None, F32, BF])
def test_layernorm_bwd_pipelined_variants(rows, cols, resdt):
    """The software-pipelined backward in the dtype combinations of the training step: bf16 dy, fp32 x, residual
    gradient / dx in fp32 (+ bf16 copy) or bf16 (the in-tower chain), with and without dres; more rows than
    waves in flight, so every wave walks several rows."""
    x = rnd(rows, cols, dtype=F32, seed=36)
    w, b = 1 + 0.1 * rnd(cols, seed=37), 0.1 * rnd(cols, seed=38)
    y, mean, rstd = ops.p_ln_fwd(x, w, b, 1e-5, BF)
    dy = rnd(rows, cols, dtype=BF, seed=39)
    xr = x.clone().requires_grad_()
    wr, br = w.clone().requires_grad_(), b.clone().requires_grad_()
    torch.nn.functional.layer_norm(xr, (cols,), wr, br, 1e-5).backward(dy.float())
    dres = rnd(rows, cols, dtype=resdt, seed=40) if resdt is not None else None
    dxd = resdt or F32
    out = ops.p_ln_bwd(dy, x, w, mean, rstd, dres=dres, dx_dtype=dxd, want_bf16=(dxd == F32), want_dres_colsum=dres is not None)
    want = xr.grad + (dres.float() if dres is not None else 0)
    rt, at = (1e-4, 1e-4) if dxd == F32 else (1e-2, 1e-2)
    close(out[0], want, rt, at, "ln dx")
    if dxd == F32:
        assert torch.equal(out[3], out[0].to(BF))
    if dres is not None:
        close(out[-1], dres.float().sum(0), 1e-5, 1e-3 * rows ** 0.5, "colsum(dres)")
    close(out[1], wr.grad, 1e-4, 1e-3 * rows ** 0.5, "ln dgamma")
    close(out[2], br.grad, 1e-4, 1e-3 * rows ** 0.5, "ln dbeta")


@pytest.mark.parametrize("M,N,K", [(512, 768, 768), (3136, 2304, 768), (1024, 768, 3072)])
def test_gemm_f32_split_against_fp64(M, N, K):
    """config.f32_split: fp32 Linear forward / data gradient / weight gradient as ONE bf16 GEMM over the operands' (hi, lo) parts
    (segclip_split3_bf16) against an fp64 product of the same fp32 operands, next to the exact fp32 GEMM: the split form must stay
    within 2e-5 of the product's scale (measured 3-5e-6 - the exact fp32 GEMM: 1-2.4e-6, both dominated by the fp32 accumulation;
    bf16 alone: 4e-3)."""
    x = rnd(M, K, dtype=F32, seed=61)
    w = rnd(N, K, dtype=F32, seed=62) * (K ** -0.5)
    b = rnd(N, dtype=F32, seed=63)
    dy = rnd(M, N, dtype=F32, seed=64)
    ref_y = (x.double() @ w.double().t() + b.double())
    ref_dx = dy.double() @ w.double()
    ref_dw = dy.double().t() @ x.double()
    errs = {}
    for split in (False, True):
        segclip_amd.config.f32_split = split
        try:
            y, _ = ops.p_linear(x, w, b)
            dx = ops.p_dgrad(dy, w, F32)
            dw = ops.p_wgrad(dy, x)
        finally:
            segclip_amd.config.f32_split = False
        errs[split] = tuple(float((got.double() - ref).abs().max() / ref.abs().max()) for got, ref in ((y, ref_y), (dx, ref_dx), (dw, ref_dw)))
    print(f"\n[f32 GEMM M={M} N={N} K={K}] max |d| / max |ref|: exact {errs[False]}, bf16 x 3 {errs[True]}")
    assert max(errs[False]) <= 5e-6, errs
    assert max(errs[True]) <= 2e-5, errs
    assert errs[True] != errs[False], "the split path was not taken"


# ------------------------------------------------------------------------------------------ attention
def _attn_ref(q, k, v, H, causal):
    B, Tq, D = q.shape
    Tk = k.shape[1]
    hd = D // H
    qh, kh, vh = (t.float().reshape(B, -1, H, hd).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(hd)
    if causal:
        s = s + torch.full((Tq, Tk), float("-inf"), device=s.device).triu_(1)
    return (torch.softmax(s, -1) @ vh).permute(0, 2, 1, 3).reshape(B, Tq, D)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,T,H,hd,causal", [(2, 196, 12, 64, False), (3, 77, 8, 64, True), (2, 8, 2, 64, False),
                                             (2, 197, 8, 48, False), (2, 17, 8, 8, False), (1, 48, 12, 64, False),
                                             (2, 256, 2, 64, True),
                                             (48, 196, 12, 64, False), (160, 77, 8, 64, True),
                                             (3, 193, 2, 64, False), (2, 222, 3, 64, False), (1, 197, 1, 64, False), (30, 200, 12, 64, False),
                                             (3, 223, 2, 64, False), (2, 224, 2, 64, False),
                                             (2, 576, 16, 64, False), (1, 300, 2, 64, True), (1, 784, 3, 64, False),
                                             (2, 577, 3, 64, False), (1, 257, 1, 64, False), (3, 449, 2, 64, False), (300, 288, 1, 64, False),
                                             (1, 448, 2, 64, False), (1, 319, 2, 64, False)])
def test_self_attention_block_packed_qkv(dtype, B, T, H, hd, causal):
    """Packed-QKV self attention exactly as ResBlockFn drives it (forward + backward)."""
    D = H * hd
    qkv = rnd(B * T, 3 * D, dtype=dtype, seed=41)
    o = torch.empty(B * T, D, dtype=dtype, device=DEV)
    s3 = (T * 3 * D, 3 * D)
    d = ops.attn_desc_packed(qkv, o, B, H, T, causal)
    stats = ops.p_attn_fwd(d, qkv)
    qr = qkv.float().view(B, T, 3, D).requires_grad_()
    ref = _attn_ref(qr[:, :, 0], qr[:, :, 1], qr[:, :, 2], H, causal)
    rt, at = (1e-4, 1e-4) if dtype == F32 else (2e-2, 2e-2)
    close(o.view(B, T, D), ref, rt, at, "attn fwd")
    do = rnd(B * T, D, dtype=dtype, seed=42)
    dqkv = torch.zeros(B * T, 3 * D, dtype=dtype, device=DEV)
    d = ops.attn_desc_packed(qkv, o, B, H, T, causal)
    part = torch.full((B, 3 * D), float("nan"), device=DEV) if dtype == BF else None
    ops.p_attn_bwd(d, stats, do, dqkv, dqkv, dqkv, s3, s3, s3, (T * D, D), 0, D, 2 * D, colsum_part=part)
    ref.backward(do.float().view(B, T, D))
    rt, at = (2e-4, 2e-4) if dtype == F32 else (3e-2, 3e-2)
    close(dqkv.view(B, T, 3, D), qr.grad, rt, at, "attn bwd dqkv")
    if part is not None:
        # fused per-sample token sums of dQ|dK|dV (in_proj bias gradient) vs the sums of the exact fp32 gradient
        want = qr.grad.sum(1).reshape(B, 3 * D)
        scale = float(qr.grad.abs().sum(1).max())
        assert float((part - want).abs().max()) <= 6e-3 * scale, (float((part - want).abs().max()), scale)
        close(part[:, 2 * D:], do.float().view(B, T, D).sum(1), 1e-3, 1e-3, "dv colsum == colsum(dO)")


@pytest.mark.parametrize("B,T,H", [(300, 196, 12), (7, 222, 3), (128, 576, 16), (40, 290, 7)])
def test_attention_dqw_backward_is_deterministic_under_memory_contention(B, T, H):
    """Race hunt for attention_dqw.inc (one barrier per step, software-counted vmcnt over mixed LDS-DMA loads and stores, fp32 workspace
    tiles across key chunks): the same backward repeated on the same inputs, every other run beside a copy loop on a second stream
    (the memory latencies vary), must give bit-identical dQ | dK | dV and token sums (tools/debug/dqw_stress.py is the long form)."""
    hd, D = 64, H * 64
    qkv = rnd(B * T, 3 * D, dtype=BF, seed=91)
    do = rnd(B * T, D, dtype=BF, seed=92)
    o = torch.empty(B * T, D, dtype=BF, device=DEV)
    s3 = (T * 3 * D, 3 * D)
    desc = lambda: ops.attn_desc_packed(qkv, o, B, H, T, False)
    stats = ops.p_attn_fwd(desc(), qkv)
    side = torch.cuda.Stream()
    junk = torch.empty(128 << 20, dtype=torch.uint8, device=DEV)
    ref = None
    for i in range(12):
        dqkv = torch.full_like(qkv, float("nan"))
        cs = torch.full((B, 3 * D), float("nan"), dtype=torch.float32, device=DEV)
        if i % 2:
            with torch.cuda.stream(side):
                for _ in range(4):
                    junk[: 64 << 20].copy_(junk[64 << 20:])
        ops.p_attn_bwd(desc(), stats, do, dqkv, dqkv, dqkv, s3, s3, s3, (T * D, D), 0, D, 2 * D, colsum_part=cs)
        torch.cuda.synchronize()
        if ref is None:
            assert not dqkv.isnan().any() and not cs.isnan().any()
            ref = (dqkv.clone(), cs.clone())
        else:
            assert torch.equal(dqkv.view(torch.int16), ref[0].view(torch.int16)), f"run {i}: dQ|dK|dV differ from run 0"
            assert torch.equal(cs.view(torch.int32), ref[1].view(torch.int32)), f"run {i}: token sums differ from run 0"


@pytest.mark.parametrize("B,T,H,hd,causal", [(2, 576, 16, 64, False), (2, 196, 12, 64, False), (3, 77, 8, 64, True),
                                             (1, 300, 2, 64, False), (2, 40, 2, 32, False)])
def test_self_attention_fp8_forward(B, T, H, hd, causal):
    """SEGCLIP_ATTN_FP8 (BASELINE configs[4] as first read) is refused: the e4m3 forward was removed (slower than bf16,
    DESIGN §8).  The refusal is SEGCLIP_ERR_UNSUPPORTED with nothing written to O or the statistics, and the bf16 forward
    on the same inputs - what configs[4] runs - holds the bf16 bounds."""
    import ctypes
    from segclip_amd import _lib
    D = H * hd
    qkv = rnd(B * T, 3 * D, dtype=BF, seed=71)
    desc = lambda o, fp8: ops.attn_desc_packed(qkv, o, B, H, T, causal, fp8=fp8)
    lib = _lib.load()
    o8 = torch.full((B * T, D), -3.0, dtype=BF, device=DEV)
    d = desc(o8, True)
    stats8 = torch.full((lib.segclip_attn_stats_bytes(ctypes.byref(d)) // 4,), 12345.0, dtype=torch.float32, device=DEV)
    d.stats = _lib.ptr(stats8)
    o8_before, stats8_before = o8.clone(), stats8.clone()
    with pytest.raises(_lib.Unsupported, match="e4m3 forward was removed"):
        _lib.check(lib.segclip_attn_fwd(ctypes.byref(d), _lib.stream()), "attn_fwd")
    torch.cuda.synchronize()
    assert torch.equal(o8.view(torch.int16), o8_before.view(torch.int16)), "the refused fp8 forward wrote O"
    assert torch.equal(stats8.view(torch.int32), stats8_before.view(torch.int32)), "the refused fp8 forward wrote the statistics"
    o = torch.empty(B * T, D, dtype=BF, device=DEV)
    ops.p_attn_fwd(desc(o, False), qkv)
    qr = qkv.float().view(B, T, 3, D)
    close(o.view(B, T, D), _attn_ref(qr[:, :, 0], qr[:, :, 1], qr[:, :, 2], H, causal), 2e-2, 2e-2, "bf16 attn fwd")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("mode", ["t18", "intended"])
@pytest.mark.parametrize("B,G,T,H", [(4, 8, 196, 12), (3, 8, 48, 2), (2, 8, 576, 16)])
def test_cross_attention_both_layouts(dtype, mode, B, G, T, H):
    """Center cross-attention with the torch-1.8 key-buffer reinterpretation and the intended layout."""
    D, S = H * 64, G + T
    qp = rnd(B * G, D, dtype=dtype, seed=51).requires_grad_()
    kv = rnd(B * S, 2 * D, dtype=dtype, seed=52).requires_grad_()
    o = ops.CrossAttnFn.apply(qp, kv, B, G, S, H, mode)
    qr = qp.detach().float().view(B, G, D).requires_grad_()
    kvr = kv.detach().float().requires_grad_()
    k3, v3 = kvr[:, :D], kvr[:, D:]
    if mode == "t18":
        k3, v3 = k3.reshape(S, B, D).permute(1, 0, 2), v3.reshape(S, B, D).permute(1, 0, 2)
    else:
        k3, v3 = k3.reshape(B, S, D), v3.reshape(B, S, D)
    ref = _attn_ref(qr, k3, v3, H, False)
    rt, at = (1e-4, 1e-4) if dtype == F32 else (2e-2, 2e-2)
    close(o.view(B, G, D), ref, rt, at, "cross fwd")
    do = rnd(B * G, D, dtype=dtype, seed=53)
    o.backward(do)
    ref.backward(do.float().view(B, G, D))
    rt, at = (2e-4, 2e-4) if dtype == F32 else (3e-2, 3e-2)
    close(qp.grad.view(B, G, D), qr.grad, rt, at, "cross dq")
    close(kv.grad, kvr.grad, rt, at, "cross dkv")


# ------------------------------------------------------------------------------------------ blocks
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,T,D,H,causal", [(2, 196, 128, 2, False), (3, 16, 64, 1, True), (2, 8, 768, 12, False)])
def test_residual_block_autograd(dtype, B, T, D, H, causal):
    """ResBlockFn (one autograd node, hand-written backward) vs torch autograd over plain ops."""
    names = ["ln1w", "ln1b", "wqkv", "bqkv", "wo", "bo", "ln2w", "ln2b", "wfc", "bfc", "wpr", "bpr"]
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,)]
    P = {}
    for i, (n, s) in enumerate(zip(names, shapes)):
        t = rnd(*s, seed=60 + i, scale=(s[-1] ** -0.5 if len(s) == 2 else 0.1))
        if n in ("ln1w", "ln2w"):
            t = 1 + t
        P[n] = t.requires_grad_()
    x = rnd(B, T, D, seed=59).requires_grad_()
    y = ops.ResBlockFn.apply(x, *[P[n] for n in names], H, causal, ops.ACT_QUICK_GELU, 1e-5, dtype)
    go = rnd(B, T, D, seed=58)
    y.backward(go)
    got = {n: P[n].grad.clone() for n in names}
    gx = x.grad.clone()
    for n in names:
        P[n].grad = None
    x.grad = None
    ln = torch.nn.functional.layer_norm
    y1 = ln(x, (D,), P["ln1w"], P["ln1b"], 1e-5)
    qkv = y1 @ P["wqkv"].t() + P["bqkv"]
    q, k, v = qkv.split(D, -1)
    x1 = x + _attn_ref(q, k, v, H, causal) @ P["wo"].t() + P["bo"]
    y2 = ln(x1, (D,), P["ln2w"], P["ln2b"], 1e-5)
    u = y2 @ P["wfc"].t() + P["bfc"]
    ref = x1 + (u * torch.sigmoid(1.702 * u)) @ P["wpr"].t() + P["bpr"]
    ref.backward(go)
    rt, at = (1e-4, 2e-4) if dtype == F32 else (5e-2, 5e-2)
    close(y, ref, rt, at, "block fwd")
    close(gx, x.grad, rt, at * 2, "block dx")
    for n in names:
        sc = float(P[n].grad.abs().max()) + 1e-6
        close(got[n] / sc, P[n].grad / sc, rt, at, f"block d{n}")


# ------------------------------------------------------------------------------------------ misc kernels
def test_cast_colsum_act():
    x = rnd(1000, 77, seed=71)
    xb = ops.p_cast(x, BF)
    assert torch.equal(xb, x.to(BF))
    assert torch.equal(ops.p_cast(xb, F32), xb.float())
    close(ops.p_colsum(x), x.sum(0), 1e-5, 1e-4, "colsum f32")
    close(ops.p_colsum(xb), xb.float().sum(0), 1e-5, 1e-3, "colsum bf16")
    xa = rnd(33, 65, seed=72).requires_grad_()
    y = ops.ActFn.apply(xa, ops.ACT_QUICK_GELU)
    y.backward(torch.ones_like(y))
    xr = xa.detach().clone().requires_grad_()
    r = xr * torch.sigmoid(1.702 * xr)
    r.backward(torch.ones_like(r))
    close(y, r, 1e-5, 1e-6, "qgelu")
    close(xa.grad, xr.grad, 1e-5, 1e-6, "qgelu grad")


def test_patch_embed_and_patchify():
    B, p, res, D = 3, 16, 64, 128
    img = rnd(B, 3, res, res, seed=81)
    w = rnd(D, 3, p, p, seed=82, scale=0.05).requires_grad_()
    cls, pos = rnd(D, seed=83).requires_grad_(), rnd(17, D, seed=84).requires_grad_()
    x = ops.PatchEmbedFn.apply(img, w, cls, pos, p, F32)
    ref = torch.nn.functional.conv2d(img, w, stride=p).reshape(B, D, -1).permute(0, 2, 1) + pos[1:]
    close(x, ref, 1e-5, 1e-5, "patch embed")
    go = rnd(B, 16, D, seed=85)
    x.backward(go)
    gw, gp = w.grad.clone(), pos.grad.clone()
    w.grad = None
    pos.grad = None
    ref.backward(go)
    close(gw, w.grad, 1e-4, 1e-4, "conv wgrad")
    close(gp, pos.grad, 1e-5, 1e-5, "pos grad")
    assert float(cls.grad.abs().max()) == 0.0
    t = ops.patchify_target(img, p)
    h = res // p
    rt = torch.einsum("nchpwq->nhwpqc", img.reshape(B, 3, h, p, h, p)).reshape(B, h * h, p * p * 3)
    assert torch.equal(t, rt)


@pytest.mark.parametrize("p,res,ldpad", [(16, 64, 0), (16, 224, 0), (14, 56, 52), (8, 32, 8)])
def test_im2col_bit_exact(p, res, ldpad):
    """conv1's im2col (module_clip_vtransformer / module_seg_vit patch embedding): the 8-pixels-per-thread kernel
    (p % 8 == 0) and the per-element kernel (p = 14, K padded to the GEMM alignment) against torch unfold."""
    from segclip_amd import _lib as L
    B, C = 3, 3
    img = rnd(B, C, res, res, seed=86)
    kdim = C * p * p
    ld = kdim + ldpad
    ref = torch.nn.functional.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, kdim)   # col = c*p*p + py*p + px
    for dt in (F32, BF):
        cols = torch.full((ref.shape[0], ld), float("nan"), dtype=dt, device=DEV)
        L.check(L.load().segclip_im2col_ld(L.ptr(img), L.ptr(cols), B, C, res, res, p, 0, L.dt(cols), ld, L.stream()), "im2col")
        assert torch.equal(cols[:, :kdim], ref.to(dt))
        assert float(cols[:, kdim:].abs().sum()) == 0.0


def test_embedding_gather_scatter():
    B, Lq, D, V = 5, 16, 64, 300
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (B, Lq), generator=g).to(DEV)
    table, pos = rnd(V, D, seed=91).requires_grad_(), rnd(Lq + 3, D, seed=92).requires_grad_()
    out = ops.EmbedFn.apply(ids, table, pos)
    ref = table[ids] + pos[:Lq]
    assert torch.equal(out, ref)
    go = rnd(B, Lq, D, seed=93)
    out.backward(go)
    gt, gp = table.grad.clone(), pos.grad.clone()
    table.grad = None
    pos.grad = None
    ref.backward(go)
    close(gt, table.grad, 1e-5, 1e-5, "dtable")
    close(gp, pos.grad, 1e-5, 1e-5, "dpos")
    src = rnd(B, Lq, D, seed=94).requires_grad_()
    idx = torch.stack([torch.randperm(Lq, generator=g)[:7] for _ in range(B)]).to(DEV)
    o = ops.GatherRowsFn.apply(src, idx)
    r = torch.gather(src, 1, idx.unsqueeze(-1).expand(-1, -1, D))
    assert torch.equal(o, r)
    go = rnd(B, 7, D, seed=95)
    o.backward(go)
    g1 = src.grad.clone()
    src.grad = None
    r.backward(go)
    assert torch.equal(g1, src.grad)


@pytest.mark.parametrize("train", [True, False])
def test_center_assignment_bit_exact(train):
    B, G, T = 4, 8, 196
    logits = rnd(B, G, T, seed=101, scale=5.0).requires_grad_()
    gum = rnd(B, G, T, seed=102) if train else None
    hard, soft, idx, counts = ops.AssignFn.apply(logits, gum, 0.9)
    assert torch.equal(counts, hard.detach().sum(-1))
    lr = logits.detach().clone().requires_grad_()
    y = ((lr + gum) / 0.9).softmax(1) if train else lr.softmax(1)
    index = y.max(1, keepdim=True)[1]
    y_hard = torch.zeros_like(lr).scatter_(1, index, 1.0)
    ref = y_hard - y.detach() + y
    assert torch.equal(idx.long(), index.squeeze(1)), "argmax over the 8 centers must be bit exact"
    assert torch.equal(hard, y_hard)
    close(soft, lr.softmax(1), 1e-5, 1e-6, "soft")
    go = rnd(B, G, T, seed=103)
    hard.backward(go)
    ref.backward(go)
    close(logits.grad, lr.grad, 1e-4, 1e-6, "straight-through grad")


def test_contrastive_pieces():
    B, E, W = 16, 64, 4
    x = rnd(B, E, seed=111).requires_grad_()
    y = ops.L2NormFn.apply(x)
    xr = x.detach().clone().requires_grad_()
    r = xr / xr.norm(dim=-1, keepdim=True)
    go = rnd(B, E, seed=112)
    y.backward(go)
    r.backward(go)
    close(y, r, 1e-5, 1e-6, "l2norm")
    close(x.grad, xr.grad, 1e-4, 1e-6, "l2norm grad")
    logits = rnd(B, B * W, seed=113, scale=4.0).requires_grad_()
    off = 2 * B
    loss = ops.CrossEntropyFn.apply(logits, off)
    lr = logits.detach().clone().requires_grad_()
    ref = torch.nn.functional.cross_entropy(lr, torch.arange(B, device=DEV) + off)
    (loss * 0.5).backward()
    (ref * 0.5).backward()
    assert abs(float(loss) - float(ref)) < 1e-5
    close(logits.grad, lr.grad, 1e-4, 1e-7, "ce grad")


def test_superpixel_kl_and_masked_mse():
    B, G, T = 3, 8, 16
    g = torch.Generator().manual_seed(7)
    idx = torch.randint(0, G, (B, T), generator=g).to(DEV)
    hard0 = torch.zeros(B, G, T, device=DEV).scatter_(1, idx.unsqueeze(1), 1.0)
    seg = torch.randint(0, 4, (B, T), generator=g).to(DEV)
    hard = hard0.clone().requires_grad_()
    loss = ops.SuperpixelKLFn.apply(hard, seg)
    hr = hard0.clone().requires_grad_()
    h = hr.permute(0, 2, 1)
    eq = ((seg.unsqueeze(-1) - seg.unsqueeze(-2)) == 0).float()
    cm = (eq @ h) / torch.clamp_min(eq.sum(-1, keepdim=True), 1.0)
    F = torch.nn.functional
    coef = float(B * T * G)
    ref = (F.kl_div(F.log_softmax(h, -1), F.softmax(cm, -1), reduction="sum") / coef
           + F.kl_div(F.log_softmax(cm, -1), F.softmax(h, -1), reduction="sum") / coef) / 2
    (loss * 3).backward()
    (ref * 3).backward()
    assert abs(float(loss) - float(ref)) < 1e-6, (float(loss), float(ref))
    close(hard.grad, hr.grad, 1e-3, 1e-7, "kl dhard")
    Dp = 48
    pred = rnd(B, T + 1, Dp, seed=121).requires_grad_()
    target = rnd(B, T, Dp, seed=122)
    mask = (torch.rand(B, T + 1, generator=g) > 0.3).float().to(DEV)
    l2 = ops.MaskedMSEFn.apply(pred, target, mask)
    pr = pred.detach().clone().requires_grad_()
    r2 = (((pr[:, 1:] - target) ** 2).mean(-1) * mask[:, 1:]).sum() / mask[:, 1:].sum()
    l2.backward()
    r2.backward()
    assert abs(float(l2) - float(r2)) < 1e-5
    close(pred.grad, pr.grad, 1e-4, 1e-7, "mse grad")


@pytest.mark.parametrize("B,T,D", [(3, 49, 768), (2, 7, 36), (4, 196, 384)])
def test_mean_cls_concat(B, T, D):
    """cat([mean(x, 1, keepdim), x], 1) (reference modules/modeling.py:240-242) as one kernel each way."""
    x = rnd(B, T, D, seed=201).requires_grad_()
    g = rnd(B, T + 1, D, seed=202)
    y = ops.mean_cat(x)
    y.backward(g)
    xr = x.detach().clone().requires_grad_()
    yr = torch.cat([torch.mean(xr, dim=1, keepdim=True), xr], dim=1)
    yr.backward(g)
    assert torch.equal(y[:, 1:], yr[:, 1:])
    close(y[:, 0], yr[:, 0], 1e-6, 1e-6, "token mean")
    close(x.grad, xr.grad, 1e-6, 1e-6, "mean-cat backward")


@pytest.mark.parametrize("B,K,L,D", [(5, 50, 197, 384), (3, 20, 77, 512), (2, 4, 4, 8)])
def test_mae_unshuffle(B, K, L, D):
    """gather(cat([x, mask_token.expand(B, L - K, D)], 1), ids_restore) + pos (reference modules/module_mae.py:310-314): forward
    bit-equal to the op-by-op expression, gradients of x exact (a permutation copy), of the mask token and the positional
    table to fp32 summation order."""
    g0 = torch.Generator().manual_seed(7)
    ids = torch.stack([torch.randperm(L, generator=g0) for _ in range(B)]).to(DEV)
    x = rnd(B, K, D, seed=211).requires_grad_()
    mt = rnd(1, 1, D, seed=212, scale=0.02).requires_grad_()
    pos = rnd(1, L, D, seed=213).requires_grad_()
    g = rnd(B, L, D, seed=214)
    y = ops.MaeUnshuffleFn.apply(x, mt, ids, pos)
    y.backward(g)
    xr, mr, pr = (t.detach().clone().requires_grad_() for t in (x, mt, pos))
    cat = torch.cat([xr, mr.expand(B, L - K, D)], dim=1)
    yr = torch.gather(cat, 1, ids.unsqueeze(-1).expand(B, L, D)) + pr
    yr.backward(g)
    assert torch.equal(y, yr)
    assert torch.equal(x.grad, xr.grad)
    close(pos.grad, pr.grad, 1e-5, 1e-5, "positional-table gradient")
    if L > K:
        close(mt.grad, mr.grad, 1e-5, 1e-4, "mask-token gradient")
    else:
        assert float(mt.grad.abs().max()) == 0.0


@pytest.mark.parametrize("B,M,D", [(5, 49, 768), (3, 196, 768), (2, 7, 40), (2, 70, 1024)])
def test_recon_mix(B, M, D):
    """a (B,M,8) @ x (B,8,D) (reference modules/module_seg_vit.py:342) as a dedicated kernel pair against torch.bmm in fp32."""
    a = rnd(B, M, 8, seed=221).requires_grad_()
    x = rnd(B, 8, D, seed=222).requires_grad_()
    g = rnd(B, M, D, seed=223)
    y = ops.recon_mix(a, x)
    y.backward(g)
    ar, xr = a.detach().clone().requires_grad_(), x.detach().clone().requires_grad_()
    yr = torch.bmm(ar, xr)
    yr.backward(g)
    close(y, yr, 1e-5, 1e-5, "recon_mix forward")
    close(a.grad, ar.grad, 1e-4, 1e-4 * D ** 0.5, "recon_mix da")
    close(x.grad, xr.grad, 1e-4, 1e-4 * M ** 0.5, "recon_mix dx")


def test_tiny_weight_gradient_over_many_rows():
    """p_wgrad with an 8 x 8 result over 12544 fp32 rows (the Linear over the center axis in the MAE branch, reference
    modules/module_seg_vit.py:338-341): 196 batched 64-row problems + a column sum instead of one workgroup walking every row."""
    dy, x = rnd(12544, 8, seed=231), rnd(12544, 8, seed=232)
    dw = ops.p_wgrad(dy, x)
    close(dw, dy.t() @ x, 1e-4, 1e-2, "tiny weight gradient")
    dy2, x2 = rnd(4000, 8, seed=233), rnd(4000, 8, seed=234)      # below the threshold: the general path
    close(ops.p_wgrad(dy2, x2), dy2.t() @ x2, 1e-4, 1e-2, "tiny weight gradient, general path")


def test_gumbel_noise_transform():
    """config.gumbel: torch's uniform draw, then -log(-log(clamp(u))) as one kernel - the values of the op-by-op expression
    (same generator state -> same noise as before), including the clamped end points."""
    from segclip_amd import config
    torch.manual_seed(5)
    g = config.gumbel((7, 8, 196), torch.device(DEV))
    torch.manual_seed(5)
    u = torch.rand((7, 8, 196), device=DEV, dtype=torch.float32)
    tiny, eps = torch.finfo(torch.float32).tiny, torch.finfo(torch.float32).eps
    ref = -torch.log(-torch.log(u.clamp(min=tiny, max=1.0 - eps)))
    close(g, ref, 2e-6, 2e-6, "gumbel transform")
    from segclip_amd import _lib as L
    e = torch.tensor([0.0, 1.0, 0.5, tiny, 1.0 - eps], device=DEV)
    out = torch.empty_like(e)
    L.check(L.load().segclip_gumbel_from_uniform(L.ptr(e), L.ptr(out), e.numel(), L.stream()), "gumbel")
    refe = -torch.log(-torch.log(e.clamp(min=tiny, max=1.0 - eps)))
    assert bool(torch.isfinite(out).all())
    close(out, refe, 2e-6, 2e-6, "gumbel transform at the clamped ends")


def test_mask_sort_bit_exact():
    B, Lq = 6, 197
    g = torch.Generator().manual_seed(3)
    noise = torch.rand(B, Lq, generator=g).to(DEV)
    ids_shuffle, ids_restore, mask = ops.mask_sort(noise, int(Lq * 0.25))
    n2 = noise.clone()
    n2[:, 0] = -1
    rs = torch.argsort(n2, dim=1)
    rr = torch.argsort(rs, dim=1)
    assert torch.equal(ids_shuffle, rs) and torch.equal(ids_restore, rr)
    m = torch.ones(B, Lq, device=DEV)
    m[:, :int(Lq * 0.25)] = 0
    assert torch.equal(mask, torch.gather(m, 1, rr))


def test_weight_shadow_registry_and_multi_cast():
    """ops.wcast keeps one bf16 copy per GEMM weight; refresh_weight_shadows re-casts them in one multi-tensor launch."""
    ws = [torch.nn.Parameter(rnd(*shape, seed=90 + i)) for i, shape in enumerate([(64, 32), (3, 5), (16385,), (40, 1000)])]
    copies = [ops.wcast(w, BF) for w in ws]
    for w, c in zip(ws, copies):
        assert torch.equal(c, w.detach().to(BF)) and ops.wcast(w, BF) is c
    ws[0].data.mul_(2.0)                       # raw write: no version bump -> the copy is stale until a forced refresh
    assert not torch.equal(copies[0], ws[0].detach().to(BF))
    assert ops.refresh_weight_shadows(force=False) == 0
    assert ops.refresh_weight_shadows(force=True) >= len(ws)
    for w, c in zip(ws, copies):
        assert torch.equal(c, w.detach().to(BF)) and ops.wcast(w, BF) is c
    with torch.no_grad():
        ws[1].add_(1.0)                        # torch-side write: version bump -> refreshed without force
    assert ops.refresh_weight_shadows(force=False) == 1
    assert torch.equal(copies[1], ws[1].detach().to(BF))
    assert ops.wcast(ws[2], F32).dtype == F32  # the f32 mode never touches the copies


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("causal", [False, True])
def test_res_stack_matches_block_by_block(dtype, causal):
    """ops.ResStackFn (N blocks as one autograd node) against N ops.ResBlockFn nodes: identical kernels in identical
    order, so outputs and every gradient are bit-equal with the fp32 residual gradient; with the bf16 residual-gradient
    chain (bf16 mode) the gradients stay within bf16 rounding of it."""
    import segclip_amd
    B, T, D, H, nblk = 3, 40, 128, 4, 3
    torch.manual_seed(7)
    blocks = []
    for _ in range(nblk):
        P = [torch.ones(D) + 0.1 * torch.randn(D), 0.1 * torch.randn(D), torch.randn(3 * D, D) * D ** -0.5,
             0.1 * torch.randn(3 * D), torch.randn(D, D) * D ** -0.5, 0.1 * torch.randn(D),
             torch.ones(D) + 0.1 * torch.randn(D), 0.1 * torch.randn(D), torch.randn(4 * D, D) * D ** -0.5,
             0.1 * torch.randn(4 * D), torch.randn(D, 4 * D) * (4 * D) ** -0.5, 0.1 * torch.randn(D)]
        blocks.append([p.to(DEV).requires_grad_() for p in P])
    x0 = torch.randn(B, T, D, device=DEV)
    gout = torch.randn(B, T, D, device=DEV)

    def run(mode):
        for P in blocks:
            for p in P:
                p.grad = None
        x = x0.clone().requires_grad_()
        if mode == "blocks":
            y = x
            for P in blocks:
                y = ops.ResBlockFn.apply(y, *P, H, causal, ops.ACT_QUICK_GELU, 1e-5, dtype)
        else:
            with segclip_amd.config.scope(bf16_resgrad=(mode == "chain")):
                y = ops.res_stack(x, blocks, H, causal, ops.ACT_QUICK_GELU, 1e-5, dtype)
        y.backward(gout)
        return y.detach(), x.grad.clone(), [[p.grad.clone() for p in P] for P in blocks]

    y0, dx0, g0 = run("blocks")
    y1, dx1, g1 = run("stack")
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for a, b in zip(g0, g1):
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    if dtype == BF:
        y2, dx2, g2 = run("chain")
        assert torch.equal(y0, y2)
        pairs = [(dx0, dx2)] + [(u, v) for a, b in zip(g0, g2) for u, v in zip(a, b)]
        for u, v in pairs:
            rel = float((u - v).norm() / u.norm().clamp_min(1e-12))
            assert rel <= 2e-2, rel


@pytest.mark.parametrize("dtype", [F32, BF])
def test_res_stack_folds_gradients_of_shared_parameters(dtype):
    """config.fold_param_grads: the same blocks applied to two inputs in ONE graph (the vision tower on the clean and on the
    masked image, reference modules/modeling.py:196,237-249): the second node adds its parameter gradients into the first
    node's tensors (segclip_multi_add_f32) and returns None, instead of one aten::add per parameter inside the autograd
    engine.  Gradients must be the bits of the engine's sums; a second pass (fresh epoch) and accumulation into existing
    .grad tensors must still work."""
    import segclip_amd
    B, D, H, nblk = 2, 128, 4, 2
    torch.manual_seed(11)
    blocks = []
    for _ in range(nblk):
        P = [torch.ones(D) + 0.1 * torch.randn(D), 0.1 * torch.randn(D), torch.randn(3 * D, D) * D ** -0.5,
             0.1 * torch.randn(3 * D), torch.randn(D, D) * D ** -0.5, 0.1 * torch.randn(D),
             torch.ones(D) + 0.1 * torch.randn(D), 0.1 * torch.randn(D), torch.randn(4 * D, D) * D ** -0.5,
             0.1 * torch.randn(4 * D), torch.randn(D, 4 * D) * (4 * D) ** -0.5, 0.1 * torch.randn(D)]
        blocks.append([p.to(DEV).requires_grad_() for p in P])
    xa, xb = torch.randn(B, 40, D, device=DEV), torch.randn(B, 24, D, device=DEV)     # two token counts, like the masked pass
    ga, gb = torch.randn(B, 40, D, device=DEV), torch.randn(B, 24, D, device=DEV)
    folded = []
    real_flush = ops._GradFold.flush

    def counting_flush(adds):
        folded.append(len(adds))
        return real_flush(adds)

    def run(fold, keep_grads=False):
        if not keep_grads:
            for P in blocks:
                for p in P:
                    p.grad = None
        with segclip_amd.config.scope(fold_param_grads=fold):
            ya = ops.res_stack(xa, blocks, H, False, ops.ACT_QUICK_GELU, 1e-5, dtype)
            yb = ops.res_stack(xb, blocks, H, False, ops.ACT_QUICK_GELU, 1e-5, dtype)
            ((ya * ga).sum() + (yb * gb).sum()).backward()
        return [[p.grad.clone() for p in P] for P in blocks]

    ref = run(False)
    ops._GradFold.flush = staticmethod(counting_flush)
    try:
        got = run(True)
        assert sum(folded) == 12 * nblk, folded            # every parameter's second gradient was folded, none left to the engine
        again = run(True)                                  # next pass: a fresh epoch, nothing stale
        twice = run(True, keep_grads=True)                 # .grad exists: AccumulateGrad adds the (folded) sum to it
    finally:
        ops._GradFold.flush = staticmethod(real_flush)
    for a, b, c, d in zip(ref, got, again, twice):
        for u, v, w, z in zip(a, b, c, d):
            assert torch.equal(u, v) and torch.equal(u, w)
            assert torch.allclose(z, 2 * u, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("causal", [False, True])
def test_res_stack_row_padding(causal, monkeypatch):
    """config.pad_rows: a stack whose B x T is not a multiple of 128 (the text tower at 96 samples: 96 x 77 = 7392) runs on the
    row count rounded up to 128 - the 256 x 256-tile GEMM kernel, the one-byte derivative, the grouped weight gradients.  Pad rows
    are zeros going in and carry zero gradients: outputs and every gradient must agree with the unpadded stack to bf16 rounding
    (the two runs use different GEMM kernels), and nothing of a pad row may leak (an uninitialised pad row would show up as
    NaN / Inf or as a large error in a weight gradient)."""
    import segclip_amd
    B, T, D, H, nblk = 16, 77, 512, 8, 2
    assert (B * T) % 128 != 0
    monkeypatch.setattr(ops, "_PAD_ROWS_MIN", 1024)      # (the default threshold is a per-GPU batch of 80 text samples)
    torch.manual_seed(13)
    blocks = []
    for _ in range(nblk):
        P = [torch.ones(D) + 0.1 * torch.randn(D), 0.1 * torch.randn(D), torch.randn(3 * D, D) * D ** -0.5,
             0.1 * torch.randn(3 * D), torch.randn(D, D) * D ** -0.5, 0.1 * torch.randn(D),
             torch.ones(D) + 0.1 * torch.randn(D), 0.1 * torch.randn(D), torch.randn(4 * D, D) * D ** -0.5,
             0.1 * torch.randn(4 * D), torch.randn(D, 4 * D) * (4 * D) ** -0.5, 0.1 * torch.randn(D)]
        blocks.append([p.to(DEV).requires_grad_() for p in P])
    x0 = torch.randn(B, T, D, device=DEV)
    gout = torch.randn(B, T, D, device=DEV)

    def run(pad):
        for P in blocks:
            for p in P:
                p.grad = None
        x = x0.clone().requires_grad_()
        with segclip_amd.config.scope(pad_rows=pad):
            y = ops.res_stack(x, blocks, H, causal, ops.ACT_QUICK_GELU, 1e-5, BF)
        assert y.shape == (B, T, D)
        y.backward(gout)
        return y.detach(), x.grad.clone(), [[p.grad.clone() for p in P] for P in blocks]

    y0, dx0, g0 = run(False)
    y1, dx1, g1 = run(True)
    pairs = [(y0, y1), (dx0, dx1)] + [(u, v) for a, b in zip(g0, g1) for u, v in zip(a, b)]
    for u, v in pairs:
        assert bool(torch.isfinite(v).all())
        rel = float((u - v).norm() / u.norm().clamp_min(1e-12))
        assert rel <= 2e-2, rel


def test_res_stack_bf16_chain_depth12_width768():
    """The bf16 residual-gradient chain (config.bf16_resgrad, the mode the bench runs) at the DEPTH and WIDTH of the
    vision tower: 12 blocks, D = 768, against the same stack with the fp32 residual gradient and against the exact-f32
    mode.  The chain rounds the residual gradient to bf16 once per LayerNorm backward (24 times here); its error must stay
    the size of the error bf16 operands cause anyway (measured on MI355X, worst GEMM-weight gradient over the 12 blocks:
    chain vs fp32 residual gradient 9.0e-3, bf16 vs exact-f32 6.9e-3; input gradient 8.9e-3 / 4.5e-3); bounds = 3x."""
    # (the whole-model effect at B = 256 is pinned in tests/test_bench_size_gpu.py: no cosine moves by more than 0.002)
    import segclip_amd
    B, T, D, H, nblk = 2, 196, 768, 12, 12
    g = torch.Generator().manual_seed(11)
    blocks = []
    for _ in range(nblk):
        P = [torch.ones(D) + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
             torch.randn(3 * D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(3 * D, generator=g),
             torch.randn(D, D, generator=g) * (D ** -0.5) * 0.5, 0.1 * torch.randn(D, generator=g),
             torch.ones(D) + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
             torch.randn(4 * D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(4 * D, generator=g),
             torch.randn(D, 4 * D, generator=g) * ((4 * D) ** -0.5) * 0.5, 0.1 * torch.randn(D, generator=g)]
        blocks.append([p.to(DEV).requires_grad_() for p in P])
    x0 = torch.randn(B, T, D, generator=g).to(DEV)
    gout = torch.randn(B, T, D, generator=g).to(DEV)

    def run(dtype, chain):
        for P in blocks:
            for p in P:
                p.grad = None
        x = x0.clone().requires_grad_()
        with segclip_amd.config.scope(bf16_resgrad=chain):
            y = ops.res_stack(x, blocks, H, False, ops.ACT_QUICK_GELU, 1e-5, dtype)
        y.backward(gout)
        return x.grad.clone(), [[p.grad.clone() for p in P] for P in blocks]

    dx32, g32 = run(F32, False)
    dxf, gf = run(BF, False)
    dxc, gc = run(BF, True)

    def rel(u, v):
        return float((u.double() - v.double()).norm() / v.double().norm().clamp_min(1e-30))
    worst_chain, worst_bf = 0.0, 0.0
    for b in range(nblk):
        for i in (2, 4, 8, 10):          # the four GEMM weights of a block
            worst_chain = max(worst_chain, rel(gc[b][i], gf[b][i]))
            worst_bf = max(worst_bf, rel(gf[b][i], g32[b][i]))
    e_dx_chain, e_dx_bf = rel(dxc, dxf), rel(dxf, dx32)
    print(f"\n[12 x 768 stack] weight grads: chain vs fp32-resgrad worst rel {worst_chain:.3e}; bf16 vs f32 worst rel {worst_bf:.3e}; "
          f"dx: chain {e_dx_chain:.3e}, bf16 {e_dx_bf:.3e}")
    assert worst_chain <= 3e-2 and e_dx_chain <= 3e-2, (worst_chain, e_dx_chain)
    assert worst_bf <= 2.5e-2 and e_dx_bf <= 1.5e-2, (worst_bf, e_dx_bf)


@pytest.mark.parametrize("shape", [(512, 768, 768), (1024, 512, 2048), (392, 768, 768)])
def test_linear_bf16_residual_stream_epilogue(shape):
    """out_proj / c_proj with the bf16 residual stream (config.bf16_resid): y = bf16(x w^T + b + r), r bf16.  Full
    256 x 256 tiles run on gemm_bf16_pq.hip (the product is rounded to bf16 before the add), other shapes on the staged
    epilogues; both against the fp32 expression, tolerance = two bf16 roundings of the result."""
    M, N, K = shape
    x, w = rnd(M, K, dtype=BF, seed=81), rnd(N, K, dtype=BF, seed=82, scale=K ** -0.5)
    b, r = rnd(N, seed=83), rnd(M, N, dtype=BF, seed=84, scale=3.0)
    y, _ = ops.p_linear(x, w, b, residual=r)
    assert y.dtype == BF
    ref = x.float() @ w.float().t() + b + r.float()
    err = (y.float() - ref).abs()
    assert float((err / (ref.abs() + 1.0)).max()) <= 2 ** -7, float((err / (ref.abs() + 1.0)).max())
    assert float(err.norm() / ref.norm()) <= 4e-3


def test_res_stack_bf16_residual_stream():
    """config.bf16_resid: the residual stream of a stack as bf16 (input / output of the node fp32), at the width of the
    vision tower and with M a multiple of 256 (so that the out_proj / c_proj launches take the gemm_bf16_pq.hip residual
    path): output and gradients against the fp32-stream bf16 mode and the exact-f32 mode.  A bf16 stream rounds x once per
    residual add; its error must stay the size of the error the bf16 GEMM operands cause anyway."""
    import segclip_amd
    B, T, D, H, nblk = 16, 64, 768, 12, 6
    g = torch.Generator().manual_seed(13)
    blocks = []
    for _ in range(nblk):
        P = [torch.ones(D) + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
             torch.randn(3 * D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(3 * D, generator=g),
             torch.randn(D, D, generator=g) * (D ** -0.5) * 0.5, 0.1 * torch.randn(D, generator=g),
             torch.ones(D) + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
             torch.randn(4 * D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(4 * D, generator=g),
             torch.randn(D, 4 * D, generator=g) * ((4 * D) ** -0.5) * 0.5, 0.1 * torch.randn(D, generator=g)]
        blocks.append([p.to(DEV).requires_grad_() for p in P])
    x0 = torch.randn(B, T, D, generator=g).to(DEV)
    gout = torch.randn(B, T, D, generator=g).to(DEV)

    def run(dtype, resid, split=False):
        for P in blocks:
            for p in P:
                p.grad = None
        x = x0.clone().requires_grad_()
        with segclip_amd.config.scope(bf16_resid=resid):
            if split:     # two stacks exchanging the bf16 stream directly (what SegViT._run_blocks does around its hook)
                y = ops.res_stack(x, blocks[:2], H, False, ops.ACT_QUICK_GELU, 1e-5, dtype, keep16=True)
                assert y.dtype == (BF if resid else F32)
                y = ops.res_stack(y, blocks[2:], H, False, ops.ACT_QUICK_GELU, 1e-5, dtype)
            else:
                y = ops.res_stack(x, blocks, H, False, ops.ACT_QUICK_GELU, 1e-5, dtype)
        assert y.dtype == F32
        y.backward(gout)
        return y.detach(), x.grad.clone(), [[p.grad.clone() for p in P] for P in blocks]

    y32, dx32, g32 = run(F32, False)
    yf, dxf, gf = run(BF, False)
    yr, dxr, gr = run(BF, True)
    ys, dxs, gs = run(BF, True, split=True)
    assert torch.equal(yr, ys) and torch.equal(dxr, dxs)     # the hand-over changes no arithmetic
    for a_, b_ in zip(gr, gs):
        for u, v in zip(a_, b_):
            assert torch.equal(u, v)

    def rel(u, v):
        return float((u.double() - v.double()).norm() / v.double().norm().clamp_min(1e-30))
    w_res = max(rel(gr[b][i], g32[b][i]) for b in range(nblk) for i in (2, 4, 8, 10))
    w_bf = max(rel(gf[b][i], g32[b][i]) for b in range(nblk) for i in (2, 4, 8, 10))
    print(f"\n[6 x 768 stack, M = 1024] y: bf16-stream {rel(yr, y32):.3e} fp32-stream {rel(yf, y32):.3e}; dx: {rel(dxr, dx32):.3e} / "
          f"{rel(dxf, dx32):.3e}; worst weight grad: {w_res:.3e} / {w_bf:.3e}")
    assert rel(yr, y32) <= 1e-2 and rel(dxr, dx32) <= 3e-2 and w_res <= 4e-2, (rel(yr, y32), rel(dxr, dx32), w_res)


@pytest.mark.parametrize("M", [1000, 4096, 12544])
def test_group_linear_pair_fused(M):
    """k_conv / v_conv of the learnable-center stage (grouped kernel-1 Conv1d, 12 groups of 64 channels) as one pass, and
    their data gradient as one pass (segclip_group_linear64), against torch's grouped conv1d in fp32 on the same bf16
    operands; M = 1000 is not a multiple of the 32-row wave blocks."""
    from segclip_amd.modules.module_seg_vit import _group_linear_pair
    D, G = 768, 12
    x = rnd(M, D, dtype=BF, seed=91).requires_grad_()
    wk = rnd(D, D // G, 1, seed=92, scale=0.125).requires_grad_()
    wv = rnd(D, D // G, 1, seed=93, scale=0.125).requires_grad_()
    gk, gv = rnd(M, D, dtype=BF, seed=94), rnd(M, D, dtype=BF, seed=95)
    k, v = _group_linear_pair(x, wk, wv, G)
    assert k.dtype == BF and v.dtype == BF
    (k.float() * gk.float()).sum().add((v.float() * gv.float()).sum()).backward()
    xr = x.detach().float().requires_grad_()
    wkr, wvr = (w.detach().to(BF).float().requires_grad_() for w in (wk, wv))
    kr = torch.nn.functional.conv1d(xr.t().unsqueeze(0), wkr, groups=G)[0].t()
    vr = torch.nn.functional.conv1d(xr.t().unsqueeze(0), wvr, groups=G)[0].t()
    ((kr * gk.float()).sum() + (vr * gv.float()).sum()).backward()
    close(k, kr, 1e-2, 1e-2, "k_conv")
    close(v, vr, 1e-2, 1e-2, "v_conv")
    close(x.grad, xr.grad, 2e-2, 2e-2, "dn = dk Wk + dv Wv")
    for w, wr, name in ((wk, wkr, "dWk"), (wv, wvr, "dWv")):
        rel = float((w.grad.float() - wr.grad).norm() / wr.grad.norm())
        assert rel <= 1e-2, (name, rel)


def test_max_tokens_pooling():
    """cls = max over the patch tokens (modules/module_seg_vit.py:441) and its backward (gradient routed to the arg-max
    token, fp32 + the bf16 copy in one pass) against torch.max."""
    B, T, D = 5, 37, 768
    x = rnd(B, T, D, seed=96).requires_grad_()
    g = rnd(B, D, seed=97)
    y = ops.MaxTokensFn.apply(x, True)
    y.backward(g)
    xr = x.detach().clone().requires_grad_()
    yr = torch.max(xr, dim=1)[0]
    yr.backward(g)
    assert torch.equal(y, yr) and torch.equal(x.grad, xr.grad)
    assert torch.equal(x.grad._segclip_bf16.float(), xr.grad.to(BF).float()) if hasattr(x.grad, "_segclip_bf16") else True


@pytest.mark.parametrize("B,C", [(8, 512), (256, 512), (33, 96)])
def test_fused_contrastive_head(B, C):
    """ops.ClipLossFn (L2-normalise, logits with clamp(exp(logit_scale), 100), two cross entropies, mean; one autograd node)
    against the torch expression of modules/modeling.py:338-362,204-209 in fp32 - loss, both feature gradients and the
    logit_scale gradient, below and above the clamp."""
    v, t = rnd(B, C, seed=98), rnd(B, C, seed=99)
    for ls0 in (math.log(1 / 0.07), 5.0):        # exp(5) = 148 > 100: clamped, zero gradient
        vv, tt = v.clone().requires_grad_(), t.clone().requires_grad_()
        ls = torch.tensor(ls0, device=DEV, requires_grad=True)
        box = {}
        loss = ops.ClipLossFn.apply(vv, tt, ls, 0, box)
        (loss * 1.7).backward()
        vr, tr = v.clone().requires_grad_(), t.clone().requires_grad_()
        lr = torch.tensor(ls0, device=DEV, requires_grad=True)
        vn, tn = vr / vr.norm(dim=-1, keepdim=True), tr / tr.norm(dim=-1, keepdim=True)
        sc = torch.clamp(lr.exp(), max=100)
        t2v, v2t = sc * tn @ vn.t(), sc * vn @ tn.t()
        lab = torch.arange(B, device=DEV)
        ref = (torch.nn.functional.cross_entropy(t2v, lab) + torch.nn.functional.cross_entropy(v2t, lab)) / 2
        (ref * 1.7).backward()
        assert abs(float(loss) - float(ref)) <= 2e-5 * max(1.0, abs(float(ref)))
        close(vv.grad, vr.grad, 1e-3, 2e-6, "d visual feature")
        close(tt.grad, tr.grad, 1e-3, 2e-6, "d text feature")
        assert abs(float(ls.grad) - float(lr.grad)) <= 1e-4 * max(1.0, abs(float(lr.grad))), (float(ls.grad), float(lr.grad))
        close(sc.detach() * box["cos"][0], t2v.detach(), 1e-5, 1e-4, "t2v logits")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,T,D", [(5, 196, 768), (3, 49, 1024), (2, 7, 64)])
def test_segment_mean_of_center_stage(dtype, B, T, D):
    """outputs = (hard @ v) / clamp_min(hard.sum(-1), 1) (modules/module_seg_vit.py:308-309) as a segment mean by center index
    (ops.SegMeanFn) against the torch expression on the same hard assignment: forward, dv, and dhard through numerator and
    normaliser; one center is left EMPTY (count 0: clamp active, no gradient through the normaliser)."""
    G = 8
    logits = rnd(B, G, T, seed=103, scale=3.0)
    logits[:, 5] = -50.0                                      # center 5 never wins: empty segment
    hard, soft, idx, counts = ops.AssignFn.apply(logits, None, 1.0)
    assert float(counts[:, 5].abs().max()) == 0.0
    v = rnd(B, T, D, dtype=dtype, seed=104)
    go = rnd(B, G, D, seed=105)
    h1 = hard.detach().clone().requires_grad_()
    v1 = v.detach().clone().requires_grad_()
    out = ops.SegMeanFn.apply(h1, idx, counts, v1)
    out.backward(go)
    h2 = hard.detach().clone().requires_grad_()
    v2 = v.detach().float().requires_grad_()
    ref = (h2 @ v2) / torch.clamp_min(h2.sum(-1, keepdim=True), 1.0)
    ref.backward(go)
    close(out, ref, 1e-5, 1e-5, "segment mean")
    tol = 1e-5 if dtype == F32 else 1e-2
    close(v1.grad, v2.grad, tol, tol, "dv")
    close(h1.grad, h2.grad, 1e-4, 1e-4 * D ** 0.5, "dhard")


@pytest.mark.parametrize("B,T,D", [(4, 196, 768), (2, 576, 1024), (3, 48, 768), (16, 784, 768), (130, 196, 768)])
def test_center_assignment_logits_token_loop(B, T, D):
    """attn = q k^T (un-scaled, fp32; modules/module_seg_vit.py:304) and its backward as per-sample token loops
    (ops.CenterLogitsFn, the bf16 mode's path) against torch in fp64."""
    G = 8
    q, k = rnd(B, G, D, seed=106).requires_grad_(), rnd(B, T, D, seed=107).requires_grad_()
    go = rnd(B, G, T, seed=108)
    attn = ops.CenterLogitsFn.apply(q, k)
    attn.backward(go)
    q2, k2 = q.detach().double().requires_grad_(), k.detach().double().requires_grad_()
    ref = q2 @ k2.transpose(1, 2)
    ref.backward(go.double())
    close(attn, ref, 1e-5, 1e-4, "logits")
    close(q.grad, q2.grad, 1e-5, 1e-4, "dq")
    close(k.grad, k2.grad, 1e-5, 1e-4, "dk")


def test_deferred_reductions_are_bit_identical():
    """segclip_reduce_multi (one launch for a block's split-K combines / row reductions) against the producers' own
    trailing reductions: same partials, same summation order -> bit-equal results."""
    M, N, K = 6272, 512, 256
    dy, x = rnd(M, N, dtype=BF, seed=61), rnd(M, K, dtype=BF, seed=62)
    dy2, x2 = rnd(M, 256, dtype=BF, seed=63), rnd(M, 768, dtype=BF, seed=64)
    ref1, ref2 = ops.p_wgrad(dy, x), ops.p_wgrad(dy2, x2)
    q = ops.ReduceQueue()
    out1, out2 = ops.p_wgrad(dy, x, defer=q), ops.p_wgrad(dy2, x2, defer=q)
    assert len(q.slabs) == 2, "both weight gradients are expected to run split-K here"
    # LayerNorm backward partials + a fused column sum in the same queue
    rows, cols = 5000, 768
    xs = rnd(rows, cols, seed=65)
    w, b = 1 + 0.1 * rnd(cols, seed=66), 0.1 * rnd(cols, seed=67)
    _, mean, rstd = ops.p_ln_fwd(xs, w, b, 1e-5, BF)
    g, dres = rnd(rows, cols, dtype=BF, seed=68), rnd(rows, cols, dtype=BF, seed=69)
    r0 = ops.p_ln_bwd(g, xs, w, mean, rstd, dres=dres, dx_dtype=BF, want_dres_colsum=True)
    r1 = ops.p_ln_bwd(g, xs, w, mean, rstd, dres=dres, dx_dtype=BF, want_dres_colsum=True, defer=q)
    r2 = ops.p_ln_bwd(g, xs, w, mean, rstd, dres=None, dx_dtype=F32, defer=q)
    r3 = ops.p_ln_bwd(g, xs, w, mean, rstd, dres=None, dx_dtype=F32)
    gy, wk, u = rnd(512, 256, dtype=BF, seed=70), rnd(256, 512, dtype=BF, seed=71, scale=256 ** -0.5), rnd(512, 512, dtype=BF, seed=72)
    du0, cs0 = ops.p_dgrad(gy, wk, BF, aux=u, act=ops.ACT_QUICK_GELU, want_colsum=True)
    du1, cs1 = ops.p_dgrad(gy, wk, BF, aux=u, act=ops.ACT_QUICK_GELU, want_colsum=True, defer=q)
    assert len(q.rows) == 3
    q.flush()
    torch.cuda.synchronize()
    assert torch.equal(out1, ref1) and torch.equal(out2, ref2)
    for a_, b_ in zip(r0, r1):
        assert torch.equal(a_, b_)
    for a_, b_ in zip(r3, r2):
        assert torch.equal(a_, b_)
    assert torch.equal(du0, du1) and torch.equal(cs0, cs1)


@pytest.mark.parametrize("out_dtype", [F32, BF])
@pytest.mark.parametrize("B,Ta,Tb,D", [(5, 8, 196, 768), (3, 8, 49, 1024), (2, 3, 5, 64)])
def test_layernorm_of_concatenation_without_the_copy(out_dtype, B, Ta, Tb, D):
    """LayerNorm(cat([a, b], dim=1)) with each part written into its token slice (ops.LayerNormCatFn; reference
    modules/module_seg_vit.py:294-296 + :211) against torch on the concatenated tensor: y, da, db, dgamma, dbeta."""
    a, b = rnd(B, Ta, D, seed=111), rnd(B, Tb, D, seed=112)
    w, bias = (1.0 + 0.1 * rnd(D, seed=113)), 0.1 * rnd(D, seed=114)
    go = rnd(B, Ta + Tb, D, seed=115)
    t1 = [t.detach().clone().requires_grad_() for t in (a, b, w, bias)]
    y = ops.layer_norm_cat(t1[0], t1[1], t1[2], t1[3], 1e-5, out_dtype)
    assert y.shape == (B, Ta + Tb, D) and y.dtype == out_dtype
    y.backward(go.to(out_dtype))
    t2 = [t.detach().double().requires_grad_() for t in (a, b, w, bias)]
    ref = torch.nn.functional.layer_norm(torch.cat([t2[0], t2[1]], 1), (D,), t2[2], t2[3], 1e-5)
    ref.backward(go.to(out_dtype).double())
    tol = 2e-5 if out_dtype == F32 else 2e-2
    close(y.float(), ref.float(), tol, tol, "y")
    for name, g1, g2 in zip(("da", "db", "dgamma", "dbeta"), t1, t2):
        close(g1.grad, g2.grad.float(), 1e-4, 1e-4 * (B * (Ta + Tb)) ** 0.5, name)


@pytest.mark.parametrize("out_dtype", [F32, BF])
@pytest.mark.parametrize("B,T,D", [(5, 196, 768), (2, 576, 1024), (1, 3, 768)])
def test_three_affine_layernorms_share_one_normalisation(out_dtype, B, T, D):
    """ops.LayerNormMultiFn + LayerNormIntoFn (the center stage's `norm` and both `ln_1(cat([q, tokens]))`,
    modules/module_seg_vit.py:289,294-296,211) against three separate torch LayerNorms in fp64: the three outputs (two of
    them token slices of (B, G+T, D) buffers completed in place by the center rows), ONE dx = the sum of the three
    backwards, the center-row gradients, and every dgamma / dbeta (ln_1's accumulate the token and the center part)."""
    G = 8
    x = rnd(B, T, D, seed=121)
    qs = [rnd(B, G, D, seed=122 + k) for k in range(2)]
    ws = [(1.0 + 0.1 * rnd(D, seed=125 + k)) for k in range(3)]
    bs = [0.1 * rnd(D, seed=128 + k) for k in range(3)]
    gos = [rnd(B, T, D, seed=131), rnd(B, G + T, D, seed=132), rnd(B, G + T, D, seed=133)]
    gos = [g.to(out_dtype) for g in gos]
    x1 = x.detach().clone().requires_grad_()
    q1 = [q.detach().clone().requires_grad_() for q in qs]
    w1 = [w.detach().clone().requires_grad_() for w in ws]
    b1 = [b.detach().clone().requires_grad_() for b in bs]
    outs = ops.layer_norm_multi(x1.view(B * T, D), list(zip(w1, b1)), [None, (T, G + T, G), (T, G + T, G)], 1e-5, out_dtype)
    assert outs is not None
    n = outs[0].view(B, T, D)
    k0 = ops.layer_norm_into(outs[1], q1[0], w1[1], b1[1], 1e-5, 0)
    k1 = ops.layer_norm_into(outs[2], q1[1], w1[2], b1[2], 1e-5, 0)
    torch.autograd.backward([n, k0, k1], gos)
    x2 = x.detach().double().requires_grad_()
    q2 = [q.detach().double().requires_grad_() for q in qs]
    w2 = [w.detach().double().requires_grad_() for w in ws]
    b2 = [b.detach().double().requires_grad_() for b in bs]
    ln = torch.nn.functional.layer_norm
    rn = ln(x2, (D,), w2[0], b2[0], 1e-5)
    r0 = ln(torch.cat([q2[0], x2], 1), (D,), w2[1], b2[1], 1e-5)
    r1 = ln(torch.cat([q2[1], x2], 1), (D,), w2[2], b2[2], 1e-5)
    torch.autograd.backward([rn, r0, r1], [g.double() for g in gos])
    tol = 2e-5 if out_dtype == F32 else 2e-2
    for name, o, r in (("norm", n, rn), ("ln_1 layer 0", k0, r0), ("ln_1 layer 1", k1, r1)):
        close(o.float(), r.float(), tol, tol, name)
    close(x1.grad, x2.grad.float(), 1e-4, 1e-4, "dx")
    for k in range(2):
        close(q1[k].grad, q2[k].grad.float(), 1e-4, 1e-4, f"dq{k}")
    for k in range(3):
        close(w1[k].grad, w2[k].grad.float(), 1e-4, 1e-4 * (B * (G + T)) ** 0.5, f"dgamma{k}")
        close(b1[k].grad, b2[k].grad.float(), 1e-4, 1e-4 * (B * (G + T)) ** 0.5, f"dbeta{k}")


def test_three_affine_layernorm_reports_unsupported_widths():
    """cols other than 768 / 1024: SEGCLIP_ERR_UNSUPPORTED, surfaced as None so the caller runs the single LayerNorms."""
    x = rnd(6, 64, seed=141)
    ws = [torch.ones(64, device=DEV) for _ in range(3)]
    assert ops.layer_norm_multi(x, list(zip(ws, ws)), [None, None, None], 1e-5, F32) is None


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("mode", ["t18", "intended"])
@pytest.mark.parametrize("B,G,T,H", [(4, 8, 196, 12), (3, 8, 48, 2)])
def test_cross_attention_with_its_input_projections(dtype, mode, B, G, T, H):
    """ops.CrossInProjAttnFn (q / kv projections of nn.MultiheadAttention with different inputs + the cross-attention core,
    modules/module_seg_vit.py:215) against the same composition in torch fp32: output, both input gradients, the ONE
    in_proj weight gradient written by two wgrads, and the bias gradient - in bf16 mode taken from the attention backward's
    token sums (sum_key dV = sum_q dO, sum_key dK = 0)."""
    D, S = H * 64, G + T
    xq, xk = rnd(B, G, D, dtype=dtype, seed=151), rnd(B, S, D, dtype=dtype, seed=152)
    w, b = rnd(3 * D, D, seed=153, scale=D ** -0.5), rnd(3 * D, seed=154, scale=0.1)
    do = rnd(B * G, D, dtype=dtype, seed=155)
    t1 = [t.detach().clone().requires_grad_() for t in (xq, xk, w, b)]
    o = ops.CrossInProjAttnFn.apply(t1[0], t1[1], t1[2], t1[3], B, G, S, H, mode, dtype)
    o.backward(do)
    wr = w.to(dtype).float() if dtype == BF else w           # the kernels see the bf16 shadow of the weight
    t2 = [t.detach().float().requires_grad_() for t in (xq, xk, wr, b)]
    qp = (t2[0].reshape(B * G, D) @ t2[2][:D].T + t2[3][:D]).view(B, G, D)
    kvp = t2[1].reshape(B * S, D) @ t2[2][D:].T + t2[3][D:]
    k3, v3 = kvp[:, :D], kvp[:, D:]
    if mode == "t18":
        k3, v3 = k3.reshape(S, B, D).permute(1, 0, 2), v3.reshape(S, B, D).permute(1, 0, 2)
    else:
        k3, v3 = k3.reshape(B, S, D), v3.reshape(B, S, D)
    ref = _attn_ref(qp, k3, v3, H, False)
    ref.backward(do.float().view(B, G, D))
    rt, at = (2e-4, 2e-4) if dtype == F32 else (3e-2, 3e-2)
    close(o.view(B, G, D), ref, rt, at, "o")
    close(t1[0].grad, t2[0].grad, rt, at, "dxq")
    close(t1[1].grad, t2[1].grad, rt, at, "dxk")
    scale = float(t2[2].grad.abs().max())
    close(t1[2].grad, t2[2].grad, rt, at * max(scale, 1.0), "dw (3D, D)")
    close(t1[3].grad, t2[3].grad, rt, at * max(float(t2[3].grad.abs().max()), 1.0), "db (3D)")
    assert float(t2[3].grad[D:2 * D].abs().max()) <= 1e-3 * max(float(t2[3].grad.abs().max()), 1.0)   # the K bias gradient is ~0


@pytest.mark.parametrize("R,shapes,pitched", [
    (6272, [(768, 256), (256, 256), (512, 768)], False),                      # few tiles: K ranges, partial tiles combined
    (19712, [(1536, 512), (512, 512), (2048, 512), (512, 2048)] * 3, True),    # three text blocks, pitched MLP operands
    (1024, [(2048, 2048)] * 4, False),                                         # 256 tiles over 16 K steps: one range, direct write
])
def test_grouped_weight_gradients(R, shapes, pitched):
    """ops.WgradGroup / segclip_wgrad_group (the weight gradients of several residual blocks as ONE launch with few K
    ranges; reference layers modules/module_seg_vit.py:162-196) against dy^T x in fp64, and run-to-run bit-reproducible."""
    lib_items = []
    for i, (M, N) in enumerate(shapes):
        dy, x = rnd(R, M, dtype=BF, seed=200 + 2 * i, scale=0.5), rnd(R, N, dtype=BF, seed=201 + 2 * i, scale=0.5)
        if pitched and M >= 2048:      # row pitch of the MLP hidden tensors (ops._empty_pitched)
            buf = torch.zeros(R, M + 512, dtype=BF, device=DEV)
            buf[:, :M] = dy
            dy = buf[:, :M]
        lib_items.append((dy, x))

    def run():
        wg = ops.WgradGroup()
        outs = [wg.add(dy, x) for dy, x in lib_items]
        assert len(wg.items) == len(shapes), "every problem here is expected to join the group"
        wg.flush()
        torch.cuda.synchronize()
        return outs
    o1, o2 = run(), run()
    for (dy, x), a, b in zip(lib_items, o1, o2):
        ref = (dy.double().t() @ x.double()).float()
        close(a, ref, 2e-3, 2e-3 * float(ref.abs().max()), f"dw {tuple(a.shape)}")
        assert torch.equal(a, b), "grouped weight gradients must be reproducible"
    # a problem the kernel does not cover (128 columns) runs on its own and is still correct
    wg = ops.WgradGroup()
    dy, x = rnd(R, 128, dtype=BF, seed=231), rnd(R, 256, dtype=BF, seed=232)
    dw = wg.add(dy, x)
    assert not wg.items
    close(dw, (dy.double().t() @ x.double()).float(), 2e-3, 2e-2, "uncovered problem")


def test_res_stack_grouped_weight_gradients_match_per_block():
    """ResStackFn with config.wgrad_group_blocks = 12 (grouped launches) against = 1 (one launch per gradient): the same
    partial products in a different K-range partition - every parameter gradient within fp32 summation noise, dx bit-equal
    (the data-gradient chain does not change)."""
    import segclip_amd
    B, T, D, H, nblk = 4, 64, 256, 4, 5
    g = torch.Generator().manual_seed(13)
    blocks = []
    for _ in range(nblk):
        P = [torch.ones(D) + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
             torch.randn(3 * D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(3 * D, generator=g),
             torch.randn(D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(D, generator=g),
             torch.ones(D) + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
             torch.randn(4 * D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(4 * D, generator=g),
             torch.randn(D, 4 * D, generator=g) * (4 * D) ** -0.5, 0.1 * torch.randn(D, generator=g)]
        blocks.append([p.to(DEV).requires_grad_() for p in P])
    x0 = torch.randn(B, T, D, generator=g).to(DEV)
    gout = torch.randn(B, T, D, generator=g).to(DEV)

    def run(group):
        for P in blocks:
            for p in P:
                p.grad = None
        x = x0.clone().requires_grad_()
        with segclip_amd.config.scope(wgrad_group_blocks=group):
            y = ops.res_stack(x, blocks, H, False, ops.ACT_QUICK_GELU, 1e-5, BF)
        y.backward(gout)
        return y.detach(), x.grad.clone(), [[p.grad.clone() for p in P] for P in blocks]
    assert ops.wgrad_group_plan(nblk, (4 * D * D + 8 * D * D) // 65536, (B * T) // 64, 12) != [1] * nblk
    y1, dx1, g1 = run(1)
    y2, dx2, g2 = run(12)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    for a, b in zip(g1, g2):
        for i, (u, v) in enumerate(zip(a, b)):
            if i in (2, 4, 8, 10):
                rel = float((u - v).norm() / u.norm().clamp_min(1e-12))
                assert rel <= 1e-5, (i, rel)
            else:
                assert torch.equal(u, v), i


@pytest.mark.parametrize("M,N,K,T", [(1024, 256, 256, 196), (12544, 768, 768, 196), (512, 512, 128, 49)])
def test_gemm_residual_table_broadcast_over_samples(M, N, K, T):
    """segclip_gemm with res_row_mod: C[m] = A[m] W^T + table[m % T] in fp32 - the positional table added to the patch
    embedding (modules/module_clip_vtransformer.py:56-64) as ONE (B*T, D) GEMM instead of B problems of T rows."""
    a, w = rnd(M, K, dtype=BF, seed=301), rnd(N, K, dtype=BF, seed=302, scale=K ** -0.5)
    table = rnd(T + 1, N, seed=303)                       # row 0 = the class-token row the caller skips (r_off)
    out = torch.empty(M, N, device=DEV)
    ops.p_gemm(a, w, out, M, N, K, (K, 1), (K, 1), N, residual=table, ldr=N, r_off=N, r_mod=T)
    ref = a.float() @ w.float().t() + table[1:][torch.arange(M, device=DEV) % T]
    close(out, ref, 1e-5, 1e-4, "gemm + table[m % T]")
    # not covered (an f32 problem, or a bf16 output): nothing is launched and the caller is told
    with pytest.raises(ops.L.Unsupported):
        ops.p_gemm(a.float(), w.float(), out, M, N, K, (K, 1), (K, 1), N, residual=table, ldr=N, r_off=N, r_mod=T)


def test_patch_embedding_one_gemm_matches_batched_form():
    """PatchEmbedFn at a batch whose token count is a multiple of 256 (one GEMM with the row-modulo residual) against the
    same Function in fp32 mode (batched form, exact-f32 GEMM): bf16-operand tolerance, and gradients flow to conv1 / pos."""
    B, p, D = 64, 16, 768
    img = rnd(B, 3, 224, 224, seed=311)
    conv_w = rnd(D, 3, p, p, seed=312, scale=(3 * p * p) ** -0.5)
    cls, pos = rnd(D, seed=313), rnd(197, D, seed=314, scale=0.1)
    outs = {}
    for dt in (F32, BF):
        t = [v.detach().clone().requires_grad_() for v in (conv_w, cls, pos)]
        x = ops.PatchEmbedFn.apply(img, t[0], t[1], t[2], p, dt)
        x.backward(torch.ones_like(x) * 1e-3)
        outs[dt] = (x.detach(), t[0].grad, t[2].grad)
    close(outs[BF][0], outs[F32][0], 2e-2, 2e-2, "patch embedding")
    close(outs[BF][1], outs[F32][1], 3e-2, 3e-2 * float(outs[F32][1].abs().max()), "d conv1")
    close(outs[BF][2], outs[F32][2], 1e-5, 1e-5, "d pos")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("mode", ["t18", "intended"])
def test_cross_attention_block_as_one_node(dtype, mode, monkeypatch):
    """ops.CrossBlockFn (a CrossAttentionBlock of the center stage, reference modules/module_seg_vit.py:199-218, as ONE autograd
    node with a hand-scheduled backward) against the same module run op by op (LayerNormFn / CrossInProjAttnFn / LinearFn
    nodes): output, the gradients of the centers and of the key/value buffer's token rows, and all 14 parameter gradients."""
    import segclip_amd
    from segclip_amd.modules import module_seg_vit as msv
    B, G, T, D, H = 4, 8, 56, 256, 4
    S = G + T
    torch.manual_seed(5)
    blk = msv.CrossAttentionBlock(D, H).to(DEV)
    for p in blk.parameters():
        torch.nn.init.normal_(p, std=0.05) if p.dim() > 1 else torch.nn.init.normal_(p, mean=1.0 if "ln" in "" else 0.0, std=0.1)
    for ln in (blk.ln_x, blk.ln_k, blk.ln_2):
        ln.weight.data.add_(1.0)
    q0, tok0 = rnd(B, G, D, seed=401), rnd(B, T, D, seed=402)
    gout = rnd(B, G, D, seed=403)
    res = {}
    segclip_amd.set_compute_dtype(dtype)
    segclip_amd.set_cross_mode(mode)
    try:
        for fused in (False, True):
            monkeypatch.setattr(msv, "_CROSS_FUSED", fused)
            for p in blk.parameters():
                p.grad = None
            q = q0.clone().requires_grad_()
            tok = tok0.clone().requires_grad_()
            tokn = ops.layer_norm(tok, blk.ln_k.weight, blk.ln_k.bias, blk.ln_k.eps, dtype)
            buf = torch.cat([torch.zeros(B, G, D, device=DEV, dtype=dtype), tokn], 1)
            out = blk(q, q, kn_buf=buf)
            out.backward(gout)
            res[fused] = (out.detach().clone(), q.grad.clone(), tok.grad.clone(), {n: p.grad.clone() for n, p in blk.named_parameters()})
    finally:
        segclip_amd.set_compute_dtype(torch.float32)
        segclip_amd.set_cross_mode("t18")
    rt = 1e-4 if dtype == F32 else 3e-2

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
    assert rel(res[True][0], res[False][0]) <= rt, ("out", rel(res[True][0], res[False][0]))
    assert rel(res[True][1], res[False][1]) <= rt, ("dq", rel(res[True][1], res[False][1]))
    assert rel(res[True][2], res[False][2]) <= rt, ("dtokens", rel(res[True][2], res[False][2]))
    for n in res[False][3]:
        e = rel(res[True][3][n], res[False][3][n])
        assert e <= rt, (n, e)
