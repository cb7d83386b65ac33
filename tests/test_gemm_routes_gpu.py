"""GPU: every kernel instance segclip_gemm can launch, each reached by a row of CASES that names the route it must take
(ops.gemm_last_route), checked against an fp64 product of the exact values the kernel reads.

Per case: (1) the route; (2) the output, the saved activation / derivative and the column sums against fp64, with the bound of
tests/helpers.check: 8e-3 for bf16 outputs, 1e-5 for fp32 outputs (1e-4 once K > 8192); a one-byte derivative to half a
step; (3) the same bound rejects the fp64 reference with one 16-wide k-slice removed and the one with one row of one tile
shifted by a row; (4) C / aux have a row pitch, rows above, between the batches and below the view, all sentinels (NaN, 0xA5
for bytes) that must survive, and the operands carry NaN outside their views; (5) the same call twice is bit-identical, and so
is the deferred split-K combine / column-sum reduction (ops.ReduceQueue) to the immediate one.
All calls go through ops.p_gemm with explicit strides (the p_linear / p_dgrad / p_wgrad wrappers allocate dense outputs, which
leave no room for the sentinel frame).

The table (CASES), the instances it must reach (INSTANCES) and the operand / frame builders are in tests/gemm_route_cases.py,
shared with tests/test_gemm_plan_cpu.py, which holds the planner to the same table without a GPU; every row here also checks
that the plan (ops.gemm_plan) is the route the launch then took.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from segclip_amd import config, ops  # noqa: E402
from tests.gemm_route_cases import (ABOVE, BF, CASES, D, ERF, F32, GAP, INSTANCES, PQ, QG, U8, expected_route,  # noqa: E402,F401
                                    frame, instance_key, operand, rnd, split3_operands)
from tests.helpers import check, within  # noqa: E402

DEV = "cuda"
AUX_STEP = 1.0 / 204.0        # one-byte derivative: q = rint((act' + 0.125) * 204)

_SEEN = {}   # case name -> instance key of the route it took


# ---- fp64 epilogue -----------------------------------------------------------------------------------------------------
def act_f(act, v):
    if act == QG:
        return v * torch.sigmoid(1.702 * v)
    return v * 0.5 * (1 + torch.erf(v * 2 ** -0.5))


def dact_f(act, v):
    if act == QG:
        s = torch.sigmoid(1.702 * v)
        return s * (1 + 1.702 * v * (1 - s))
    return 0.5 * (1 + torch.erf(v * 2 ** -0.5)) + v * torch.exp(-0.5 * v * v) * (2 * torch.pi) ** -0.5


def rtol_of(case):
    if case.c == BF:
        return 8e-3
    return 1e-4 if case.K > 8192 else 1e-5


def bits(t):
    return t.view({1: U8, 2: torch.int16, 4: torch.int32}[t.element_size()]).clone()


# ---- one case ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gemm_route_and_value(case):
    gen = torch.Generator(device=DEV).manual_seed(sum(map(ord, case.name)))
    nb1, nb2 = case.nb
    M, N, K = case.M, case.N, case.K
    a_ks, b_ks = case.lay[0] == "k", case.lay[1] == "k"
    A, Av, sa, bsA = operand(M, K, a_ks, case.a, nb1, nb2, "A" in case.bcast, DEV, gen)
    B, Bv, sb, bsB = operand(N, K, b_ks, case.b, nb1, nb2, "B" in case.bcast, DEV, gen, K ** -0.5)

    # the values the kernel multiplies, (nb1, nb2|1, rows, K'), in fp64
    if case.f32_split:
        def parts(x):
            hi = x.to(BF)
            return hi.double(), (x - hi.float()).to(BF).double()
        (ah, al), (bh, bl) = parts(Av), parts(Bv)
        Ak, Bk = torch.cat((ah, al, ah), -1), torch.cat((bh, bh, bl), -1)
    else:
        Ak = (Av.to(BF) if case.b == BF else Av).double()     # an fp32 A on a bf16 kernel is rounded to nearest even
        Bk = Bv.double()
    P = case.alpha * (Ak @ Bk.transpose(-1, -2))               # broadcasts the stride-0 batches over nb2
    P = P.expand(nb1, nb2, M, N)

    ldc = N + case.ldc_pad
    nan = float("nan")
    C, Cv, c_off, bsC, c_in = frame(case, ldc, case.c, nan, DEV)
    bias = rnd((N,), gen, 0.5).float() if case.bias else None
    res = bsR = None
    if case.res is not None:
        nbr2 = 1 if "R" in case.bcast else nb2
        res = torch.full((nb1, nbr2, M, N + 8), nan, dtype=case.res, device=DEV)
        res[..., :N] = rnd((nb1, nbr2, M, N), gen).to(case.res)
        bsR = (nbr2 * M * (N + 8), 0 if "R" in case.bcast else M * (N + 8))
    aux = auxv = a_in = None
    if case.aux is not None:
        adt = U8 if case.aux_kind == 2 else case.c
        aux, auxv, _, _, a_in = frame(case, ldc, adt, 0xA5 if adt == U8 else nan, DEV)
        if case.aux == "in":
            if case.aux_kind == 2:
                auxv.copy_(torch.randint(0, 256, auxv.shape, generator=gen, device=DEV, dtype=torch.int32))
            else:
                u = rnd(auxv.shape, gen)
                auxv.copy_(dact_f(case.act, u) if case.aux_kind == 1 else u)
    cs = torch.full((N,), nan, device=DEV) if case.colsum else None

    def epi(p):
        """fp64 epilogue of the product p: (output, saved side output or None)"""
        if case.aux == "in":
            s = auxv.double()
            d = s * AUX_STEP - 0.125 if case.aux_kind == 2 else (s if case.aux_kind == 1 else dact_f(case.act, s))
            return p * d, None
        v = p + bias.double() if bias is not None else p
        side = None
        if case.act:
            side = v if case.aux_kind == 0 else dact_f(case.act, v)
            v = act_f(case.act, v)
        if res is not None:
            v = v + res[..., :N].double()
        return v, side

    def run(Cbuf, coff, ld, bs, defer=None, auxbuf=aux, csum=cs, entry=ops.p_gemm):
        kw = dict(c_off=coff, bias=bias, residual=res, ldr=N + 8, aux=auxbuf, ldaux=ld, act=case.act, mul_dact=case.aux == "in",
                  alpha=case.alpha, colsum=csum, aux_kind=case.aux_kind, defer=defer)
        if case.f32_split and entry is ops.gemm_plan:   # the bf16 problem p_gemm turns the call into (ops._gemm_f32_split)
            return entry(*split3_operands(case, DEV, Cbuf, ld), **kw)
        with config.scope(f32_split=case.f32_split):
            return entry(A, B, Cbuf, M, N, K, sa, sb, ld, nb1=nb1, nb2=nb2, bsA=bsA, bsB=bsB, bsC=bs, bsR=bsR, **kw)

    # 1. route, and the plan of the same call
    plan = run(C, c_off, ldc, bsC, entry=ops.gemm_plan)
    run(C, c_off, ldc, bsC)
    route = ops.gemm_last_route()
    family, tm, tn, splits, variant = case.route
    assert route == ops.GemmRoute(family, a_ks, b_ks, tm, tn, splits, variant), f"{case.name}: took {route}"
    assert plan == route, f"{case.name}: planned {plan}, took {route}"
    _SEEN[case.name] = instance_key(route, case.lay)
    if case.reduce is not None:   # which combine kernel splitk_reduce picks (gemm_bf16.hip): contiguous C, one batch
        assert splits > 1 and (case.reduce == "vec") == (ldc == N and nb1 * nb2 == 1)
    torch.cuda.synchronize()

    # 5. repeatable: the same call again, bit for bit (whole frames: the sentinels included)
    snap = [bits(C)] + ([bits(aux)] if case.aux == "out" else []) + ([bits(cs)] if cs is not None else [])
    run(C, c_off, ldc, bsC)
    again = [bits(C)] + ([bits(aux)] if case.aux == "out" else []) + ([bits(cs)] if cs is not None else [])
    assert all(torch.equal(x, y) for x, y in zip(snap, again)), f"{case.name}: second call differs"

    # 4. nothing outside the views is written
    assert bool(C[~c_in].isnan().all()), f"{case.name}: C written outside the M x N view"
    if case.aux == "out":
        outside = aux[~a_in]
        assert bool((outside == 0xA5).all() if aux.dtype == U8 else outside.isnan().all()), f"{case.name}: aux written outside"

    # 2. values against fp64
    rtol = rtol_of(case)
    ref, side = epi(P)
    check(Cv, ref, rtol, f"{case.name}: C")
    if case.aux == "out":
        if case.aux_kind == 2:
            err = float((auxv.double() * AUX_STEP - 0.125 - side.clamp(-0.125, 1.125)).abs().max())
            assert err <= 0.5 * AUX_STEP + 1e-4, f"{case.name}: derivative byte, max err {err:.3e}"
        else:
            check(auxv, side, rtol, f"{case.name}: saved {'pre-activation' if case.aux_kind == 0 else 'derivative'}")
    if cs is not None:
        # the pq kernel sums the stored (rounded) outputs, dma / p8 their fp32 values before the rounding
        cref = (Cv.double() if family == PQ else ref).sum((0, 1, 2))
        check(cs, cref, 1e-5, f"{case.name}: column sums")

    # 3. the bound is discriminating: a dropped MFMA k-step and a row moved within a tile are both rejected
    k0 = 16 * ((Ak.shape[-1] - 1) // 16)
    dropped = P - case.alpha * (Ak[..., k0:k0 + 16] @ Bk[..., k0:k0 + 16].transpose(-1, -2))
    assert not within(Cv, epi(dropped)[0], rtol), f"{case.name}: the check accepts a dropped k-slice"
    shifted = ref.clone()
    r = min(tm, M) - 2
    shifted[0, 0, r, :tn] = ref[0, 0, r + 1, :tn]
    assert not within(Cv, shifted, rtol), f"{case.name}: the check accepts a row shifted within a tile"

    # 5. deferred combines, flushed, equal the immediate ones (the deferred split-K needs a contiguous C)
    if splits > 1 and nb1 * nb2 == 1:
        dense = [torch.full((M, N), nan, dtype=case.c, device=DEV) for _ in range(2)]
        run(dense[0], 0, N, (0, 0))
        q = ops.ReduceQueue()
        run(dense[1], 0, N, (0, 0), defer=q)
        assert ops.gemm_last_route() == route and len(q.slabs) == 1, f"{case.name}: split-K combine not deferred"
        torch.cuda.synchronize()
        assert bool(dense[1].isnan().all()), f"{case.name}: C written before the deferred combine"
        q.flush()
        assert torch.equal(bits(dense[0]), bits(dense[1])), f"{case.name}: deferred split-K combine differs"
    if cs is not None:
        cs2 = torch.full((N,), nan, device=DEV)
        q = ops.ReduceQueue()
        run(C, c_off, ldc, bsC, defer=q, csum=cs2)
        assert len(q.rows) == 1
        q.flush()
        assert torch.equal(bits(cs), bits(cs2)), f"{case.name}: deferred column sums differ"


def test_dgrad_wrapper_fused_colsum_rows128():
    """p_dgrad's fused bias gradient at M = 256 q + 128 with a bf16 derivative (the form p_linear falls back to when the
    one-byte derivative is refused): the column sums come from the 128-row tiles, where every tile is full"""
    gen = torch.Generator(device=DEV).manual_seed(7)
    M, N, K = 384, 256, 512
    dy = rnd((M, N), gen).to(BF)
    w = (rnd((N, K), gen) * N ** -0.5).to(BF)
    d = dact_f(QG, rnd((M, K), gen)).to(BF)
    dx, cs = ops.p_dgrad(dy, w, BF, aux=d, act=QG, aux_kind=1, want_colsum=True)
    assert ops.gemm_last_route() == ops.GemmRoute(D, False, True, 128, 128, 1, 2)
    ref = (dy.double() @ w.double()) * d.double()
    check(dx, ref, 8e-3, "dgrad x derivative")
    check(cs, ref.sum(0), 1e-5, "fused column sums")


def test_unsupported_call_records_no_route():
    x = torch.zeros(256, 128, dtype=BF, device=DEV)
    w = torch.zeros(256, 128, dtype=BF, device=DEV)
    y = torch.empty(256, 256, dtype=BF, device=DEV)
    ops.p_gemm(x, w, y, 256, 256, 128, (128, 1), (128, 1), 256)
    assert ops.gemm_last_route().family is not None
    refused = dict(bias=torch.zeros(200, device=DEV), colsum=torch.empty(200, device=DEV))   # column sums need N % 256 == 0
    with pytest.raises(ops.L.Unsupported) as launched:
        ops.p_gemm(x, w[:200], y, 256, 200, 128, (128, 1), (128, 1), 256, **refused)
    assert ops.gemm_last_route() == ops.GemmRoute(None, False, False, 0, 0, 0, 0)
    with pytest.raises(ops.L.Unsupported) as planned:   # the plan of the refused call: the same refusal
        ops.gemm_plan(x, w[:200], y, 256, 200, 128, (128, 1), (128, 1), 256, **refused)
    assert str(planned.value) == str(launched.value)


def test_table_reaches_every_instance():
    """the routes the table's rows took (test_gemm_route_and_value, run before this) cover every reachable instance"""
    expected = {c.name: instance_key(expected_route(c), c.lay) for c in CASES}
    missing = sorted(set(INSTANCES) - set(expected.values()))
    assert not missing, f"no case is meant to reach {missing}"
    not_run = sorted(set(expected) - set(_SEEN))
    assert not not_run, f"cases not run (or failed before their route was recorded): {not_run}"
    missing = sorted(set(INSTANCES) - set(_SEEN.values()))
    assert not missing, f"no case reached {missing}"
