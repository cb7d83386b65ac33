"""No GPU: the planner of segclip_gemm (csrc/gemm_plan.cpp through segclip_gemm_plan / ops.gemm_plan) against the route table of
tests/gemm_route_cases.py - the same shapes, pitches, offsets and batch strides as tests/test_gemm_routes_gpu.py launches, on
CPU storage of which only the addresses are read.  Also: the four refusals, the split-K workspace and split counts the ABI
answers on their own (segclip_gemm_ws_bytes, segclip_gemm_splits), and the half-tile tail."""
import ctypes as C

import pytest
import torch

from segclip_amd import _lib as L
from segclip_amd import ops
from tests.gemm_route_cases import BF, CASES, F32, INSTANCES, QG, U8, expected_route, frame, instance_key, operand, split3_operands

CPU = "cpu"
NO_ROUTE = ops.GemmRoute(None, False, False, 0, 0, 0, 0)


def call_of(case):
    """(positional, keyword) arguments of the ops.p_gemm call test_gemm_routes_gpu.py makes for this row, on CPU storage"""
    nb1, nb2 = case.nb
    M, N, K = case.M, case.N, case.K
    ldc = N + case.ldc_pad
    Cb, _, c_off, bsC, _ = frame(case, ldc, case.c, 0, CPU, fill=False)
    res = bsR = None
    if case.res is not None:
        nbr2 = 1 if "R" in case.bcast else nb2
        res = torch.empty((nb1, nbr2, M, N + 8), dtype=case.res)
        bsR = (nbr2 * M * (N + 8), 0 if "R" in case.bcast else M * (N + 8))
    aux = frame(case, ldc, U8 if case.aux_kind == 2 else case.c, 0, CPU, fill=False)[0] if case.aux is not None else None
    kw = dict(c_off=c_off, bias=torch.empty(N) if case.bias else None, residual=res, ldr=N + 8, aux=aux, ldaux=ldc, act=case.act,
              mul_dact=case.aux == "in", alpha=case.alpha, colsum=torch.empty(N) if case.colsum else None, aux_kind=case.aux_kind)
    if case.f32_split:
        return split3_operands(case, CPU, Cb, ldc), kw
    A, _, sa, bsA = operand(M, K, case.lay[0] == "k", case.a, nb1, nb2, "A" in case.bcast, CPU)
    B, _, sb, bsB = operand(N, K, case.lay[1] == "k", case.b, nb1, nb2, "B" in case.bcast, CPU)
    return (A, B, Cb, M, N, K, sa, sb, ldc), dict(kw, nb1=nb1, nb2=nb2, bsA=bsA, bsB=bsB, bsC=bsC, bsR=bsR)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_plan_is_the_row_s_route(case):
    args, kw = call_of(case)
    assert ops.gemm_plan(*args, **kw) == expected_route(case)
    assert ops.gemm_plan(*args, **kw, defer=ops.ReduceQueue()) == expected_route(case)   # the deferral flags change no route


def test_planned_routes_cover_every_instance():
    seen = set()
    for case in CASES:
        args, kw = call_of(case)
        seen.add(instance_key(ops.gemm_plan(*args, **kw), case.lay))
    assert not sorted(set(INSTANCES) - seen)


def desc(*args, **kw):
    """the descriptor ops.gemm_plan plans for a call, and what keeps its buffers alive"""
    d, keep = ops._gemm_desc(L.load(), False, *args, **kw)
    return d, (keep, args, kw)


def test_unknown_keyword_is_a_type_error():
    x, w, y = torch.empty(64, 64, dtype=BF), torch.empty(64, 64, dtype=BF), torch.empty(64, 64, dtype=BF)
    with pytest.raises(TypeError, match="no_such_keyword"):
        ops.gemm_plan(x, w, y, 64, 64, 64, (64, 1), (64, 1), 64, no_such_keyword=1)


def desc_of(case, ws="exact"):
    """a row's descriptor with the workspace present (its exact size), absent or one byte short"""
    args, kw = call_of(case)
    d, keep = desc(*args, **kw)
    if ws == "absent":
        d.ws, d.ws_bytes = None, 0
    elif ws == "short":
        d.ws_bytes -= 1
    return d, keep


def plan_of(d):
    lib = L.load()
    r, w = L.GemmRoute(), C.c_size_t(0)
    rc = lib.segclip_gemm_plan(C.byref(d), C.byref(r), C.byref(w))
    route = ops.GemmRoute(L.GEMM_ROUTE_FAMILIES[r.family], bool(r.a_ks), bool(r.b_ks), r.tile_m, r.tile_n, r.splits, r.variant)
    return rc, lib.segclip_last_error_string().decode(), route, w.value


SPLITK = [c for c in CASES if c.route[3] > 1]


@pytest.mark.parametrize("case", SPLITK, ids=[c.name for c in SPLITK])
def test_splitk_workspace_and_split_counts(case):
    lib = L.load()
    nb, K = case.nb[0] * case.nb[1], (3 if case.f32_split else 1) * case.K
    d, keep = desc_of(case)
    rc, _, route, ws_bytes = plan_of(d)
    assert rc == 0 and route == expected_route(case)
    # ws_bytes = splits' x nb x M x N x 4, splits' the count before empty K ranges are dropped: ranges of whole 64-steps
    unit = nb * case.M * case.N * 4
    assert ws_bytes == lib.segclip_gemm_ws_bytes(C.byref(d)) == d.ws_bytes and ws_bytes % unit == 0
    s0 = ws_bytes // unit
    kper = -(--(-K // 64) // s0) * 64
    assert 2 <= route.splits <= s0 <= 32 and -(-K // kper) == route.splits
    assert lib.segclip_gemm_splits(C.byref(d)) == route.splits == case.route[3]
    for ws in ("absent", "short"):
        d1, keep1 = desc_of(case, ws)
        rc, _, r1, ws1 = plan_of(d1)
        assert rc == 0 and r1.splits == 1 and ws1 == ws_bytes, (ws, r1)
        assert lib.segclip_gemm_splits(C.byref(d1)) == 1


def refusal(d):
    """(rc, message, route) of the plan, and the same from segclip_gemm itself, which refuses before any launch"""
    lib = L.load()
    rc, msg, route, _ = plan_of(d)
    assert lib.segclip_gemm(C.byref(d), None) == rc and lib.segclip_last_error_string().decode() == msg
    assert ops.gemm_last_route() == NO_ROUTE
    return rc, msg, route


def test_refusal_colsum_off_full_tiles():
    x, w, y = torch.empty(256, 128, dtype=BF), torch.empty(200, 128, dtype=BF), torch.empty(256, 256, dtype=BF)
    kw = dict(bias=torch.empty(200), colsum=torch.empty(200))                        # N % 256 != 0
    with pytest.raises(L.Unsupported, match="fused colsum unsupported for this shape"):
        ops.gemm_plan(x, w, y, 256, 200, 128, (128, 1), (128, 1), 256, **kw)
    d, keep = desc(x, w, y, 256, 200, 128, (128, 1), (128, 1), 256, **kw)
    assert refusal(d) == (-2, "gemm: fused colsum unsupported for this shape", NO_ROUTE)


@pytest.mark.parametrize("M,N,dt", [(4224, 2304 + 128, BF), (4096 + 64, 2304, BF), (4096, 2304, F32)],
                         ids=["n_off_tiles", "m_off_tiles", "fp32_operands"])
def test_refusal_res_row_mod(M, N, dt):
    K = 64
    x, w = torch.empty(M, K, dtype=dt), torch.empty(N, K, dtype=dt)
    y, table = torch.empty(M, N), torch.empty(192, N)
    call = (x, w, y, M, N, K, (K, 1), (K, 1), N), dict(bias=torch.empty(N), residual=table, ldr=N, r_mod=192)
    with pytest.raises(L.Unsupported) as e:
        ops.gemm_plan(*call[0], **call[1])
    want = ("gemm: res_row_mod is a bf16-operand feature" if dt == F32 else
            "gemm: res_row_mod needs the fp32-residual epilogue on full 256 x 256 bf16 tiles")
    assert str(e.value).endswith(want)
    d, keep = desc(*call[0], **call[1])
    assert refusal(d) == (-2, want, NO_ROUTE)


def test_res_row_mod_on_full_tiles_is_planned():
    """the counterpart of the refusals above: the same call on full 256 x 256 bf16 tiles takes the fp32-residual epilogue (mode 5)"""
    M, N, K = 4096, 2304, 64
    x, w, y, table = torch.empty(M, K, dtype=BF), torch.empty(N, K, dtype=BF), torch.empty(M, N), torch.empty(192, N)
    assert ops.gemm_plan(x, w, y, M, N, K, (K, 1), (K, 1), N, residual=table, ldr=N, r_mod=192) == ops.GemmRoute("pq", False, False, 256, 256, 1, 5)


def test_refusal_aux_kind_2_off_full_tiles():
    """M = 256 q + 128, k-strided A with a k-contiguous B: the pq kernel has no such layout, and the staged epilogues of dma / p8
    write the derivative byte on full 256 x 256 tiles only"""
    M, N, K = 4096 + 128, 2304, 64
    xt, w = torch.empty(K, M, dtype=BF), torch.empty(N, K, dtype=BF)
    y, aux = torch.empty(M, N, dtype=BF), torch.empty(M, N, dtype=U8)
    call = (xt, w, y, M, N, K, (1, M), (K, 1), N), dict(bias=torch.empty(N), aux=aux, ldaux=N, act=QG, aux_kind=2)
    with pytest.raises(L.Unsupported) as e:
        ops.gemm_plan(*call[0], **call[1])
    want = "gemm: aux_kind 2 needs full 256 x 256 tiles, 16-byte aligned operands and no split-K"
    assert str(e.value).endswith(want)
    d, keep = desc(*call[0], **call[1])
    assert refusal(d) == (-2, want, NO_ROUTE)


def test_refusal_no_unit_stride():
    """the descriptor of tests/test_abi.py: a bf16 operand with neither stride 1"""
    d = L.GemmDesc()
    d.M = d.N = d.K = 64
    d.A = d.B = d.C = C.c_void_p(16)
    d.sam, d.sak, d.sbn, d.sbk = 3, 5, 64, 1
    d.a_dtype = d.b_dtype = d.c_dtype = L.BF16
    assert refusal(d) == (-1, "gemm_bf16: A needs unit stride along k or m (sam=3 sak=5)", NO_ROUTE)


def test_empty_problem_plans_nothing():
    """M = 0: rc 0 and no route, from the plan and from segclip_gemm, before any tile or split arithmetic (K is long enough for split-K)"""
    d = L.GemmDesc()
    d.A = d.B = d.C = C.c_void_p(4096)
    d.M, d.N, d.K, d.sam, d.sak, d.sbn, d.sbk, d.ldc, d.nb1, d.nb2, d.alpha = 0, 256, 4096, 4096, 1, 4096, 1, 256, 1, 1, 1.0
    d.a_dtype = d.b_dtype = d.c_dtype = L.BF16
    assert plan_of(d)[::2] == (0, NO_ROUTE) and L.load().segclip_gemm(C.byref(d), None) == 0
    assert ops.gemm_last_route() == NO_ROUTE


def pitched_desc(M, a_ks):
    """bf16 M x 2304 x 64 with fake pointers and an A operand whose 256 rows (64 k-rows) span exactly 2^31 bytes - the pitch
    at which the 32-bit DMA offsets of gemm_bf16_p8.hip / gemm_bf16_pq.hip end; B k-contiguous and dense"""
    N, K = 2304, 64
    d = L.GemmDesc()
    d.A, d.B, d.C = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)   # never dereferenced
    sam, sak = (1, 1 << 24) if a_ks else (1 << 22, 1)
    assert (64 * sak if a_ks else 256 * sam) * 2 == 1 << 31
    d.M, d.N, d.K, d.sam, d.sak, d.sbn, d.sbk, d.ldc, d.nb1, d.nb2, d.alpha = M, N, K, sam, sak, K, 1, N, 1, 1, 1.0
    d.a_dtype = d.b_dtype = d.c_dtype = L.BF16
    return d


@pytest.mark.parametrize("a_ks", [False, True], ids=["sam_4Mi", "sak_16Mi"])
def test_two_gib_pitch_takes_the_256x128_dma_tiles(a_ks):
    """The one input whose route moved when the 256 x 256 instance of gemm_bf16_dma.hip left: 256-wide tiles (pick_bn) that pq
    and p8 refuse for their 32-bit operand offsets.  They run on the 256 x 128 instance, whose addresses are 64-bit; with the
    256 x 256 instance the same descriptor planned ("dma", .., 256, 256, 1, 1).
    M = 8192, not the 4096 the change was specified with: 16 x 9 = 144 tiles of 256 x 256 are fewer than the 256 of
    dma_small_tiles, so M = 4096 ran - and runs - on 128 x 128 tiles and never reached the 256 x 256 instance (second assert).
    32 x 9 = 288 tiles is past that rule and is the problem that did."""
    DMA_256x128, DMA_128x128 = 0, 2
    assert plan_of(pitched_desc(8192, a_ks))[::2] == (0, ops.GemmRoute("dma", a_ks, False, 256, 128, 1, DMA_256x128))
    assert plan_of(pitched_desc(4096, a_ks))[::2] == (0, ops.GemmRoute("dma", a_ks, False, 128, 128, 1, DMA_128x128))


@pytest.mark.parametrize("ntiles", [197 * 3, 197 * 12, 197 * 9, 256 + 128, 256 + 129, 0, 1, 154, 256, 512])
def test_half_tile_tail_is_the_plan_s(ntiles):
    """segclip_gemm_pq_half_tail (the rows of test_wgrad_plan_cpu.test_half_tile_tail_plan) against the variant of a planned
    forward GEMM over that many 256 x 256 tiles: bits 4-15 = the tail tiles run as half-tiles"""
    lib = L.load()
    tail = lib.segclip_gemm_pq_half_tail(ntiles)
    if ntiles == 0:
        assert tail == 0
        return
    M, N, K = 256 * ntiles, 256, 64                      # ntiles x 1 tiles
    d = L.GemmDesc()
    d.A, d.B, d.C = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)   # never dereferenced
    d.M, d.N, d.K, d.sam, d.sak, d.sbn, d.sbk, d.ldc, d.nb1, d.nb2, d.alpha = M, N, K, K, 1, K, 1, N, 1, 1, 1.0
    d.a_dtype = d.b_dtype = d.c_dtype = L.BF16
    rc, _, route, _ = plan_of(d)
    assert rc == 0
    if route.family == "pq":                               # the 256-wide tiles need more than 128 of them
        assert route.variant == tail << 4
    else:
        assert ntiles <= 256 and tail == 0, route
