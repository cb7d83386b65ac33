"""config.c_exec: the residual block's forward enqueued by ONE library call (segclip_resblock_fwd, csrc/exec.cpp) against the same
block launched kernel by kernel from ops._resblock_fwd - same buffers, same descriptors, so every saved tensor, the output and,
after one backward, every gradient must be equal bit for bit.  Also: a block the executor refuses costs no launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import segclip_amd  # noqa: E402
from segclip_amd import _lib as L  # noqa: E402
from segclip_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
PQ_ACT8 = 2          # csrc/gemm_plan.h: the pq epilogue that stores the QuickGELU derivative byte (bits 0-3 of the route variant)


def block_params(D, F, g):
    P = [torch.ones(D) + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
         torch.randn(3 * D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(3 * D, generator=g),
         torch.randn(D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(D, generator=g),
         torch.ones(D) + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
         torch.randn(F, D, generator=g) * D ** -0.5, 0.1 * torch.randn(F, generator=g),
         torch.randn(D, F, generator=g) * F ** -0.5, 0.1 * torch.randn(D, generator=g)]
    return ops.BlockParams._make(p.to(DEV).requires_grad_() for p in P)


def plan_c_fc(M, D, F, act):
    """the route of the block's c_fc GEMM as ops._resblock_fwd lays it out (pitched hidden tensors), planned on CPU storage"""
    y2, w = torch.empty(M, D, dtype=BF), torch.empty(F, D, dtype=BF)
    ak = ops._aux_kind(BF, act, M, F)
    h, u = ops._empty_pitched((M, F), BF, y2), ops._empty_pitched((M, F), torch.uint8 if ak == 2 else BF, y2)
    return ops.gemm_plan(y2, w, h, M, F, D, (D, 1), (D, 1), h.stride(0), bias=torch.empty(F), aux=u, ldaux=u.stride(0), act=act,
                         aux_kind=ak)


def plan_c_proj(M, D, F):
    h, w, xo, x1 = torch.empty(M, F, dtype=BF), torch.empty(D, F, dtype=BF), torch.empty(M, D), torch.empty(M, D)
    return ops.gemm_plan(h, w, xo, M, D, F, (F, 1), (F, 1), D, bias=torch.empty(D), residual=x1, ldr=D)


class Calls:
    """Records the Python-level calls of segclip_resblock_fwd and segclip_gemm as (name, rc, the thread's last GEMM route after
    the call): the launches inside the executor are not Python calls, but every segclip_gemm, theirs too, rewrites that route."""

    def __init__(self, monkeypatch):
        lib = L.load()
        self.log = []
        for name in ("segclip_resblock_fwd", "segclip_gemm"):
            monkeypatch.setattr(lib, name, self.wrap(name, getattr(lib, name)))

    def wrap(self, name, fn):
        def call(*args):
            rc = fn(*args)
            self.log.append((name, rc, ops.gemm_last_route()))
            return rc
        return call

    def of(self, name):
        return [c for c in self.log if c[0] == name]


def same_bits(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)), what


def run_block(c_exec, x0, P, B, T, H, act, gout, calls):
    """-> (output and BlockSaved of ops._resblock_fwd), (y, dx, the 12 gradients) of ResBlockFn, the calls of that forward, and
    the thread's last GEMM route before it (a small GEMM sets a known one: a refused executor call must leave it alone)"""
    M, D = x0.shape[0] * x0.shape[1], x0.shape[2]
    with segclip_amd.config.scope(c_exec=c_exec):
        w16 = P.wo.detach().to(BF)
        ops.p_gemm(w16, w16, torch.empty(D, D, dtype=BF, device=DEV), D, D, D, (D, 1), (D, 1), D)
        primed = ops.gemm_last_route()
        assert primed.family is not None
        calls.log.clear()
        xo, saved = ops._resblock_fwd(x0.view(M, D), tuple(p.detach() for p in P), B, T, H, False, act, 1e-5, BF, None)
        log = list(calls.log)
        for p in P:
            p.grad = None
        x = x0.clone().requires_grad_()
        y = ops.ResBlockFn.apply(x, *P, H, False, act, 1e-5, BF, None)
        y.backward(gout)
    return (xo, saved), (y.detach(), x.grad.clone(), ops.BlockParams._make(p.grad.clone() for p in P)), log, primed


def check_block_equal(r1, r0):
    (xo1, s1), (y1, dx1, g1) = r1[:2]
    (xo0, s0), (y0, dx0, g0) = r0[:2]
    assert torch.equal(xo1, xo0) and torch.equal(y1, y0) and torch.equal(y1.view_as(xo1), xo1) and bool(torch.isfinite(y1).all())
    for name in ops.BlockSaved._fields:
        same_bits(getattr(s1, name), getattr(s0, name), name)
    assert torch.equal(dx1, dx0) and bool(torch.isfinite(dx1).all())
    for name in ops.BlockParams._fields:
        assert torch.equal(getattr(g1, name), getattr(g0, name)), name


def first_pq_rows(D, F):
    """the smallest multiple of 256 rows at which the planner gives c_fc with the derivative byte to the 256 x 256 pq kernel"""
    for M in range(256, 32768, 256):
        try:
            r = plan_c_fc(M, D, F, ops.ACT_QUICK_GELU)
        except L.Unsupported:
            continue
        if r.family == "pq" and r.variant & 15 == PQ_ACT8:
            return M
    raise AssertionError("no row count up to 32768 puts c_fc on the pq kernel")


@pytest.mark.parametrize("extra", [0, 128], ids=["full_tiles", "half_tile_row"])
def test_exec_equals_launches_on_the_shipped_path(extra, monkeypatch):
    """(a) QuickGELU, fp32 stream, c_fc on the pq kernel with the one-byte derivative: the executor takes the block (one call, rc 0,
    no GEMM call from Python), and everything equals the launch-by-launch run"""
    D, H, F, T = 256, 4, 1024, 128
    M = first_pq_rows(D, F) + extra
    r = plan_c_fc(M, D, F, ops.ACT_QUICK_GELU)
    assert r.family == "pq" and r.variant & 15 == PQ_ACT8 and (r.tile_m, r.tile_n) == (256, 256), r
    B = M // T
    g = torch.Generator().manual_seed(5 + extra)
    P = block_params(D, F, g)
    x0, gout = torch.randn(B, T, D, generator=g).to(DEV), torch.randn(B, T, D, generator=g).to(DEV)
    calls = Calls(monkeypatch)
    r1 = run_block(True, x0, P, B, T, H, ops.ACT_QUICK_GELU, gout, calls)
    r0 = run_block(False, x0, P, B, T, H, ops.ACT_QUICK_GELU, gout, calls)
    assert [(n, rc) for n, rc, _ in r1[2]] == [("segclip_resblock_fwd", 0)], r1[2]
    assert [(n, rc) for n, rc, _ in r0[2]] == [("segclip_gemm", 0)] * 4, r0[2]
    assert r1[0][1].u.dtype == torch.uint8 and r0[0][1].u.dtype == torch.uint8
    check_block_equal(r1, r0)


def test_refused_block_runs_once(monkeypatch):
    """(b) erf-GELU at 128 rows: ops._aux_kind asks for the derivative byte, the planner has no kernel for it (tests/
    test_block_exec_cpu.py), the executor refuses BEFORE launching and the block runs launch by launch, once, keeping u as bf16"""
    B, T, D, H, F = 2, 64, 64, 1, 256
    M, act = B * T, ops.ACT_GELU_ERF
    assert ops._aux_kind(BF, act, M, F) == 2
    with pytest.raises(L.Unsupported, match="aux_kind 2"):
        plan_c_fc(M, D, F, act)
    g = torch.Generator().manual_seed(7)
    P = block_params(D, F, g)
    x0, gout = torch.randn(B, T, D, generator=g).to(DEV), torch.randn(B, T, D, generator=g).to(DEV)
    calls = Calls(monkeypatch)
    r1 = run_block(True, x0, P, B, T, H, act, gout, calls)
    r0 = run_block(False, x0, P, B, T, H, act, gout, calls)
    # the refused call: rc, and no segclip_gemm ran inside it (the thread's last route is still the one set before the block)
    unsupported = L.const("ERR_UNSUPPORTED")
    assert r1[2][0] == ("segclip_resblock_fwd", unsupported, r1[3]), r1[2][0]
    # then the same five GEMM calls as without the executor: in_proj, out_proj, c_fc refused with the byte, c_fc with bf16, c_proj
    want = [("segclip_gemm", rc) for rc in (0, 0, unsupported, 0, 0)]
    assert [(n, rc) for n, rc, _ in r1[2][1:]] == want and [(n, rc) for n, rc, _ in r0[2]] == want, (r1[2], r0[2])
    assert r1[2][-1][2] == r0[2][-1][2] == plan_c_proj(M, D, F)
    assert r1[0][1].u.dtype == BF and r0[0][1].u.dtype == BF
    check_block_equal(r1, r0)


def test_exec_equals_launches_in_a_padded_bf16_stack(monkeypatch):
    """(c) two blocks as one ResStackFn node: 3 x 77 = 231 token rows padded to 256, bf16 residual stream, causal, with key lengths"""
    B, T, D, H, nblk = 3, 77, 128, 2, 2
    monkeypatch.setattr(ops, "_PAD_ROWS_MIN", 128)
    g = torch.Generator().manual_seed(9)
    blocks = [block_params(D, 4 * D, g) for _ in range(nblk)]
    x0, gout = torch.randn(B, T, D, generator=g).to(DEV), torch.randn(B, T, D, generator=g).to(DEV)
    klen = torch.tensor([77, 5, 40], dtype=torch.int32, device=DEV)

    def run(c_exec, calls):
        for P in blocks:
            for p in P:
                p.grad = None
        x = x0.clone().requires_grad_()
        with segclip_amd.config.scope(c_exec=c_exec, pad_rows=True, bf16_resid=True):
            calls.log.clear()
            y = ops.res_stack(x, blocks, H, True, ops.ACT_QUICK_GELU, 1e-5, BF, klen=klen)
            n_exec = [rc for _, rc, _ in calls.of("segclip_resblock_fwd")]
            y.backward(gout)
        return n_exec, [y.detach(), x.grad.clone()] + [p.grad.clone() for P in blocks for p in P]

    calls = Calls(monkeypatch)
    n1, out1 = run(True, calls)
    n0, out0 = run(False, calls)
    assert (n1, n0) == ([0] * nblk, [])          # the executor took both blocks; without it, it is not called
    for i, (a, b) in enumerate(zip(out1, out0)):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), i
