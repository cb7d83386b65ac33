"""No GPU: segclip_resblock_fwd (csrc/exec.cpp) plans the block's four GEMMs before its first launch, so a block it has no
kernel for is refused with nothing enqueued - on a machine without a device the refusal is the planner's, not a launch error.
The descriptor is built on CPU storage, of which only the addresses are read (as in tests/test_gemm_plan_cpu.py)."""
import ctypes as C
import math

import pytest
import torch

from segclip_amd import _lib as L
from segclip_amd import ops

BF = torch.bfloat16
AUX2 = "gemm: aux_kind 2 needs full 256 x 256 tiles, 16-byte aligned operands and no split-K"


def test_resblock_fwd_refuses_before_it_launches():
    """M = 128, D = 64, H = 1, F = 256, erf-GELU: ops._aux_kind asks for the one-byte derivative (rows a multiple of 128), the
    planner picks 128-wide tiles for c_fc, whose staged epilogue has no erf byte - the one refused GEMM is the block's third"""
    M, B, T, D, H, F = 128, 2, 64, 64, 1, 256
    act = ops.ACT_GELU_ERF
    assert ops._aux_kind(BF, act, M, F) == 2
    t = {n: torch.empty(s, dtype=dt) for n, s, dt in (
        ("x", (M, D), torch.float32), ("x1", (M, D), torch.float32), ("xo", (M, D), torch.float32),
        ("y1", (M, D), BF), ("y2", (M, D), BF), ("o", (M, D), BF), ("qkv", (M, 3 * D), BF), ("h", (M, F), BF),
        ("u", (M, F), torch.uint8), ("st4", (4, M), torch.float32), ("stats", (B * H * T,), torch.float32),
        ("wqkv", (3 * D, D), BF), ("wo", (D, D), BF), ("wfc", (F, D), BF), ("wpr", (D, F), BF),
        ("bqkv", (3 * D,), torch.float32), ("bfc", (F,), torch.float32), ("vec", (6, D), torch.float32))}
    # the planner's own answer for the four GEMMs of this block: in_proj, out_proj and c_proj have a kernel, c_fc has none
    ops.gemm_plan(t["y1"], t["wqkv"], t["qkv"], M, 3 * D, D, (D, 1), (D, 1), 3 * D, bias=t["bqkv"])
    ops.gemm_plan(t["o"], t["wo"], t["x1"], M, D, D, (D, 1), (D, 1), D, bias=t["vec"][0], residual=t["x"], ldr=D)
    ops.gemm_plan(t["h"], t["wpr"], t["xo"], M, D, F, (F, 1), (F, 1), D, bias=t["vec"][1], residual=t["x1"], ldr=D)
    with pytest.raises(L.Unsupported) as e:
        ops.gemm_plan(t["y2"], t["wfc"], t["h"], M, F, D, (D, 1), (D, 1), F, bias=t["bfc"], aux=t["u"], ldaux=F, act=act, aux_kind=2)
    assert str(e.value).endswith(AUX2)

    d = L.ResBlockFwdDesc()
    for name in ("x", "x1", "xo", "y1", "y2", "o", "qkv", "h", "u", "stats", "wqkv", "wo", "wfc", "wpr", "bqkv", "bfc"):
        setattr(d, name, t[name].data_ptr())
    for i, name in enumerate(("ln1w", "ln1b", "bo", "ln2w", "ln2b", "bpr")):
        setattr(d, name, t["vec"][i].data_ptr())
    for i, name in enumerate(("mean1", "rstd1", "mean2", "rstd2")):
        setattr(d, name, t["st4"][i].data_ptr())
    d.ld_h = d.ld_u = F
    d.M, d.B, d.T, d.D, d.F, d.H = M, B, T, D, F, H
    d.eps, d.attn_scale = 1e-5, 1.0 / math.sqrt(D // H)
    d.causal, d.act, d.aux_kind, d.x_dtype = 0, act, 2, L.F32
    lib = L.load()
    assert lib.segclip_resblock_fwd(C.byref(d), None) == L.const("ERR_UNSUPPORTED")
    assert lib.segclip_last_error_string().decode() == AUX2
    with pytest.raises(L.Unsupported, match="aux_kind 2"):
        L.check(lib.segclip_resblock_fwd(C.byref(d), None), "resblock_fwd")
