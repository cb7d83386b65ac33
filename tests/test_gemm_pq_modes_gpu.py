"""GPU: every epilogue mode of the 256 x 256-tile bf16 GEMM (gemm_bf16_pq.hip) at the token count of the vision tower
(M = 256 x 196 = 50176 rows, B = 256 images x 196 patches) against an fp64 product of the same bf16 operands.  N = 768
gives 588 tiles: the last 76 run as 128 x 256 half-tile workgroups, so every forward / data-gradient mode below also
covers the half-tile tail.  The operand and accumulator maps of the MFMA shape the kernel is built with are checked here
element by element, on rows the tail and the full tiles both produce."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from segclip_amd import _lib, ops  # noqa: E402
from tests.helpers import check  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
M, N, K, T = 50176, 768, 128, 196
AUX_STEP = 1.0 / 204.0                # one-byte derivative: q = rint((act' + 0.125) * 204)


def rnd(*shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


@pytest.fixture(scope="module")
def data():
    assert _lib.load().segclip_gemm_pq_half_tail((M // 256) * (N // 256)) == 76, "the half-tile tail is not taken at this shape"
    x = rnd(M, K, seed=1, dtype=BF)
    w = rnd(N, K, seed=2, scale=K ** -0.5, dtype=BF)
    b = rnd(N, seed=3)
    pre = x.double() @ w.double().t() + b.double()
    return dict(x=x, w=w, b=b, pre=pre)


def test_plain_forward(data):
    y = ops.p_linear(data["x"], data["w"], data["b"])[0]
    check(y, data["pre"], 8e-3, "bias")
    y0 = ops.p_linear(data["x"], data["w"], None)[0]
    check(y0, data["pre"] - data["b"].double(), 8e-3, "no bias")


def test_bf16_residual(data):
    r16 = rnd(M, N, seed=4, scale=2.0, dtype=BF)
    y = ops.p_linear(data["x"], data["w"], data["b"], residual=r16)[0]
    check(y, data["pre"] + r16.double(), 8e-3, "+ bf16 residual")


def test_fp32_residual(data):
    r32 = rnd(M, N, seed=5, scale=2.0)
    y = ops.p_linear(data["x"], data["w"], data["b"], residual=r32, out_dtype=F32)[0]
    assert y.dtype == F32
    check(y, data["pre"] + r32.double(), 1e-5, "+ fp32 residual -> fp32")


def test_fp32_residual_row_modulo(data):
    table = rnd(T + 1, N, seed=6)          # row 0 is skipped (r_off), rows 1.. repeat every T output rows
    out = torch.empty(M, N, device=DEV)
    ops.p_gemm(data["x"], data["w"], out, M, N, K, (K, 1), (K, 1), N, residual=table, ldr=N, r_off=N, r_mod=T)
    ref = data["pre"] - data["b"].double() + table[1:].double()[torch.arange(M, device=DEV) % T]
    check(out, ref, 1e-5, "+ table[m % T] -> fp32")


@pytest.mark.parametrize("act", ["quick_gelu", "gelu_erf"])
def test_activation_and_one_byte_derivative(data, act):
    pre = data["pre"]
    if act == "quick_gelu":
        code = ops.ACT_QUICK_GELU
        s = torch.sigmoid(1.702 * pre)
        yref, dref = pre * s, s * (1 + 1.702 * pre * (1 - s))
    else:
        code = ops.ACT_GELU_ERF
        cdf = 0.5 * (1 + torch.erf(pre * 2 ** -0.5))
        yref, dref = pre * cdf, cdf + pre * torch.exp(-0.5 * pre * pre) * (2 * torch.pi) ** -0.5
    y, a = ops.p_linear(data["x"], data["w"], data["b"], act=code, want_aux=True, aux_kind=2)[:2]
    assert a.dtype == torch.uint8 and a.shape == (M, N)
    check(y, yref, 8e-3, f"{act} forward")
    dec = a.double() * AUX_STEP - 0.125
    # half a step, the saturation of the representable range [-0.125, 1.125] (erf-GELU: act' reaches -0.129 / 1.129),
    # and the bf16 operands' effect on pre is nil here (fp64 reference of the same operands): the fp32 accumulation only
    err = float((dec - dref.clamp(-0.125, 1.125)).abs().max())
    assert err <= 0.5 * AUX_STEP + 1e-4, f"{act} derivative byte: max err {err:.3e}"


def test_data_gradient_plain_and_times_derivative(data):
    dy = rnd(M, K, seed=7, dtype=BF)
    wk = rnd(K, N, seed=8, scale=K ** -0.5, dtype=BF)          # (K, N): the k-strided B operand
    ref = dy.double() @ wk.double()
    dx = ops.p_dgrad(dy, wk, BF)
    check(dx, ref, 8e-3, "data gradient")
    _, a = ops.p_linear(data["x"], data["w"], data["b"], act=ops.ACT_QUICK_GELU, want_aux=True, aux_kind=2)[:2]
    dec = a.double() * AUX_STEP - 0.125
    for colsum in (False, True):
        got = ops.p_dgrad(dy, wk, BF, aux=a, act=ops.ACT_QUICK_GELU, aux_kind=2, want_colsum=colsum)
        du = got[0] if colsum else got
        check(du, ref * dec, 8e-3, f"data gradient x derivative (colsum {colsum})")
        if colsum:   # the column sums of the stored bf16 values
            cs = got[1]
            csref = du.double().sum(0)
            assert float((cs.double() - csref).abs().max()) <= 1e-4 * float(du.double().abs().sum(0).max()), "fused column sums"


def test_weight_gradient_slabs_and_group(data):
    # the K dimension of these products is the 50176 token rows; both output dimensions are multiples of 256
    dy = rnd(M, 512, seed=9, scale=0.5, dtype=BF)
    x1 = rnd(M, 256, seed=10, scale=0.5, dtype=BF)
    x2 = rnd(M, 768, seed=11, scale=0.5, dtype=BF)
    ref1, ref2 = dy.double().t() @ x1.double(), dy.double().t() @ x2.double()
    dw = ops.p_wgrad(dy, x1)
    check(dw, ref1, 1e-4, "weight gradient (k-strided operands, fp32 slabs)")
    wg = ops.WgradGroup()
    outs = [wg.add(dy, x1), wg.add(dy, x2)]
    assert len(wg.items) == 2, "both problems are expected to join the group"
    wg.flush()
    torch.cuda.synchronize()
    check(outs[0], ref1, 1e-4, "grouped weight gradient 0")
    check(outs[1], ref2, 1e-4, "grouped weight gradient 1")
