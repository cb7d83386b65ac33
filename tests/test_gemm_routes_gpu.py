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

Instances and the cases that reach them:
  generic (gemm_bf16.hip, 128 x 128; A bf16 / fp32, aligned / ragged):
    ff: gen_ff_bf16_al, gen_ff_bf16_rag, gen_ff_f32_al, gen_ff_f32_rag
    fk: gen_fk_bf16_al, gen_fk_bf16_rag, gen_fk_f32_al_splitk, gen_fk_f32_rag
    kf: gen_kf_bf16_al, gen_kf_bf16_rag, gen_kf_f32_al_splitk, gen_kf_f32_rag_batched
    kk: gen_kk_bf16_al, gen_kk_bf16_rag_splitk, gen_kk_f32_al_batched, gen_kk_f32_rag
  dma (gemm_bf16_dma.hip) 256 x 128: dma0_ff, dma0_fk_colsum, dma0_kf_pitched, dma0_kk_batched
  dma 128 x 128: dma2_ff_res32, dma2_fk_splitk, dma2_kf_f32out, dma2_kk_batched, dma2_fk_colsum_rows128,
    dma2_ff_colsum_rows128, f32split_ff (the bf16 route of config.f32_split)
  dma 256 x 256 (all four layouts): not reachable through segclip_gemm.  The dispatcher tries it only when
    segclip_gemm_bf16_dma_pick_bn picks 256-wide tiles, and then the p8 kernel takes every problem first: p8 refuses only
    what dma refuses too (aux_kind 2 / column sums off full tiles), or with SEGCLIP_GEMM_P8=0, or operand pitches of 4 GiB.
  p8 (gemm_bf16_p8.hip): p8_ff_batched, p8_ff_colsum, p8_fk_splitk, p8_kf_f32out, p8_kk_splitk
  pq (gemm_bf16_pq.hip): forward pq_f_res_rows128, data gradient pq_k_dact8_colsum_rows128, weight gradient pq_w_splitk
  f32 (gemm_f32.hip): 32 x 128 f32_skinny, 64 x 64 f32_small_batched, 128 x 128 f32_large
The 256-wide tiles need more than 128 of them (the tile-count heuristic prefers 128-wide tiles below that), so the p8 and pq
cases are 8-9 M outputs with a short K.
"""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from segclip_amd import config, ops  # noqa: E402
from tests.helpers import check, within  # noqa: E402

DEV = "cuda"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
QG, ERF = ops.ACT_QUICK_GELU, ops.ACT_GELU_ERF
AUX_STEP = 1.0 / 204.0        # one-byte derivative: q = rint((act' + 0.125) * 204)
PQ_RES, PQ_DACT8, PQ_SLAB = 1, 3, 4
ABOVE, GAP = 3, 2             # sentinel rows above the first / after every batch of C and aux


@dataclasses.dataclass
class Case:
    name: str
    lay: str                  # "ff" / "fk" / "kf" / "kk": A, B k-contiguous (f) or k-strided (k)
    M: int
    N: int
    K: int
    route: tuple              # (family, tile_m, tile_n, splits, variant) - the layout is lay's
    a: torch.dtype = BF
    b: torch.dtype = BF
    c: torch.dtype = BF
    bias: bool = False
    alpha: float = 1.0
    act: int = ops.ACT_NONE
    aux: str = None           # "out": saved by the forward epilogue, "in": mul_dact input
    aux_kind: int = 0
    res: torch.dtype = None
    colsum: bool = False
    nb: tuple = (1, 1)
    bcast: str = ""           # operands broadcast over nb2 (batch stride 0): any of "A", "B", "R"
    ldc_pad: int = 8          # C / aux row pitch = N + ldc_pad
    f32_split: bool = False
    reduce: str = None        # split-K combine: "vec" (contiguous C) / "strided"


G, D, P8, PQ, FF = "generic", "dma", "p8", "pq", "f32"
CASES = [
    # -- generic: K % 64 != 0, an fp32 A operand, or unaligned rows keep a problem off the LDS-DMA kernels
    Case("gen_ff_bf16_al", "ff", 200, 136, 72, (G, 128, 128, 1, 2), bias=True, act=QG, aux="out"),
    Case("gen_ff_bf16_rag", "ff", 130, 20, 70, (G, 128, 128, 1, 0), c=F32, res=F32, alpha=0.75, ldc_pad=3),
    Case("gen_ff_f32_al", "ff", 256, 256, 128, (G, 128, 128, 1, 3), a=F32, bias=True, act=ERF),
    Case("gen_ff_f32_rag", "ff", 100, 60, 37, (G, 128, 128, 1, 1), a=F32, c=F32, alpha=2.0),
    Case("gen_fk_bf16_al", "fk", 192, 264, 96, (G, 128, 128, 1, 2), act=QG, aux="in", aux_kind=1),
    Case("gen_fk_bf16_rag", "fk", 300, 100, 128, (G, 128, 128, 1, 0)),
    # 17 K-steps in 4 splits of 5: the last one is 2 K-tiles
    Case("gen_fk_f32_al_splitk", "fk", 128, 128, 1088, (G, 128, 128, 4, 3), a=F32, c=F32, ldc_pad=0, reduce="vec"),
    Case("gen_fk_f32_rag", "fk", 70, 50, 33, (G, 128, 128, 1, 1), a=F32, bias=True, res=BF),
    Case("gen_kf_bf16_al", "kf", 136, 72, 80, (G, 128, 128, 1, 2), alpha=-1.5),
    Case("gen_kf_bf16_rag", "kf", 130, 200, 64, (G, 128, 128, 1, 0), c=F32),
    # K = 2000 in 8 splits of 256: the last one 208; alpha applied by the combine
    Case("gen_kf_f32_al_splitk", "kf", 264, 128, 2000, (G, 128, 128, 8, 3), a=F32, c=F32, alpha=0.25, ldc_pad=4,
         reduce="strided"),
    Case("gen_kf_f32_rag_batched", "kf", 33, 40, 50, (G, 128, 128, 1, 1), a=F32, c=F32, bias=True, act=QG, aux="out",
         aux_kind=1, nb=(2, 3), bcast="B"),
    Case("gen_kk_bf16_al", "kk", 136, 264, 72, (G, 128, 128, 1, 2), c=F32),
    Case("gen_kk_bf16_rag_splitk", "kk", 100, 132, 1536, (G, 128, 128, 6, 0), reduce="strided"),
    Case("gen_kk_f32_al_batched", "kk", 128, 256, 192, (G, 128, 128, 1, 3), a=F32, c=F32, nb=(3, 1)),
    Case("gen_kk_f32_rag", "kk", 36, 20, 300, (G, 128, 128, 1, 1), a=F32, bias=True),
    # -- dma, 256 x 128 tiles: N <= 128, M < 128 or fused column sums
    Case("dma0_ff", "ff", 1000, 72, 128, (D, 256, 128, 1, 0), c=F32, bias=True, act=QG, aux="out"),
    Case("dma0_fk_colsum", "fk", 512, 512, 192, (D, 256, 128, 1, 0), act=QG, aux="in", aux_kind=1, colsum=True),
    Case("dma0_kf_pitched", "kf", 120, 640, 192, (D, 256, 128, 1, 0), bias=True, alpha=0.5, ldc_pad=4),
    Case("dma0_kk_batched", "kk", 64, 1000, 128, (D, 256, 128, 1, 0), nb=(2, 2), bcast="B"),
    # -- dma, 128 x 128 tiles: fewer than 256 of the 256-row tiles
    Case("dma2_ff_res32", "ff", 264, 392, 64, (D, 128, 128, 1, 2), bias=True, res=F32),
    # 65 K-steps in 8 splits of 9: the last one 2 K-tiles
    Case("dma2_fk_splitk", "fk", 768, 768, 4160, (D, 128, 128, 8, 2), ldc_pad=0, reduce="vec"),
    Case("dma2_kf_f32out", "kf", 512, 384, 128, (D, 128, 128, 1, 2), c=F32, alpha=1.25, bias=True, act=ERF, aux="out",
         ldc_pad=4),
    Case("dma2_kk_batched", "kk", 256, 256, 256, (D, 128, 128, 1, 2), nb=(2, 3), bcast="A"),
    # M = 256 q + 128 with column sums: the partial 256-row tile's per-element epilogue writes no partial sums, so these run
    # on 128-row tiles (the second one is a problem the p8 kernel would take without column sums)
    Case("dma2_fk_colsum_rows128", "fk", 384, 512, 256, (D, 128, 128, 1, 2), act=QG, aux="in", aux_kind=1, colsum=True,
         ldc_pad=0),
    Case("dma2_ff_colsum_rows128", "ff", 4224, 2304, 64, (D, 128, 128, 1, 2), bias=True, colsum=True, ldc_pad=0),
    # -- p8: 256 x 256 tiles the pq kernel refuses (batched, split-K outside the weight gradient, k-strided A with a
    #    k-contiguous B, bf16 weight-gradient output, column sums without the one-byte derivative)
    Case("p8_ff_batched", "ff", 248, 1280, 128, (P8, 256, 256, 1, 0), bias=True, res=F32, nb=(3, 9), bcast="BR",
         ldc_pad=0),
    Case("p8_ff_colsum", "ff", 4096, 2304, 64, (P8, 256, 256, 1, 0), bias=True, colsum=True, ldc_pad=0),
    Case("p8_fk_splitk", "fk", 768, 1536, 4160, (P8, 256, 256, 8, 0), c=F32, alpha=-0.5, ldc_pad=0, reduce="vec"),
    Case("p8_kf_f32out", "kf", 2496, 3328, 64, (P8, 256, 256, 1, 0), c=F32, bias=True, act=ERF, ldc_pad=0),
    Case("p8_kk_splitk", "kk", 768, 1536, 4160, (P8, 256, 256, 8, 0), reduce="strided"),
    # -- pq: variant = epilogue mode | half-tail tiles << 4 | half-tiles of the last 128 rows << 16
    Case("pq_f_res_rows128", "ff", 4224, 2304, 64, (PQ, 256, 256, 1, PQ_RES | 9 << 16), bias=True, res=BF, ldc_pad=0),
    Case("pq_k_dact8_colsum_rows128", "fk", 4224, 2304, 64, (PQ, 256, 256, 1, PQ_DACT8 | 9 << 16), act=QG, aux="in",
         aux_kind=2, colsum=True, ldc_pad=0),
    # 34 K-steps in 3 splits of 12: the last one 10
    Case("pq_w_splitk", "kk", 2048, 2304, 2176, (PQ, 256, 256, 3, PQ_SLAB), c=F32, ldc_pad=0, reduce="vec"),
    # -- exact fp32
    Case("f32_skinny", "ff", 8, 200, 300, (FF, 32, 128, 1, 0), a=F32, b=F32, c=F32, bias=True, act=QG, aux="out",
         aux_kind=1),
    Case("f32_small_batched", "fk", 256, 256, 512, (FF, 64, 64, 1, 1), a=F32, b=F32, c=F32, alpha=0.5, res=F32,
         nb=(2, 2), bcast="R"),
    Case("f32_large", "kk", 1530, 1408, 96, (FF, 128, 128, 1, 2), a=F32, b=F32, c=F32, act=ERF, aux="in"),
    # config.f32_split: fp32 operands as one bf16 GEMM over their (hi | lo | hi) x (hi | hi | lo) parts, K' = 3 K
    Case("f32split_ff", "ff", 512, 768, 768, (D, 128, 128, 4, 2), a=F32, b=F32, c=F32, ldc_pad=4, f32_split=True,
         reduce="strided"),
]

_SEEN = {}   # case name -> instance key of the route it took


def instance_key(r, lay):
    if r.family == G:
        return (G, lay, "f32A" if r.variant & 1 else "bf16A", "aligned" if r.variant & 2 else "ragged")
    if r.family == D:
        return (D, lay, f"{r.tile_m}x{r.tile_n}")
    if r.family == P8:
        return (P8, lay)
    if r.family == PQ:
        return (PQ, {"ff": "f", "fk": "k", "kk": "w"}[lay])
    return (FF, f"{r.tile_m}x{r.tile_n}")


INSTANCES = ([(G, lay, a, al) for lay in ("ff", "fk", "kf", "kk") for a in ("bf16A", "f32A") for al in ("aligned", "ragged")]
             + [(D, lay, t) for lay in ("ff", "fk", "kf", "kk") for t in ("256x128", "128x128")]
             + [(P8, lay) for lay in ("ff", "fk", "kf", "kk")] + [(PQ, x) for x in "fkw"]
             + [(FF, t) for t in ("32x128", "64x64", "128x128")])


# ---- operands, frames, fp64 epilogue ---------------------------------------------------------------------------------
def rnd(shape, gen, scale=1.0):
    return torch.randn(*shape, generator=gen, device=DEV, dtype=torch.float64) * scale


def operand(rows, K, ks, dtype, nb1, nb2, bcast, gen, scale=1.0):
    """storage (nb1, nb2 or 1, R, C + 8) with NaN in the pitch: k-contiguous R = rows, C = K; k-strided R = K, C = rows.
    Returns the storage, the logical (nb1, nb2|1, rows, K) values, (s_row, s_k) and the batch strides."""
    R, C = (K, rows) if ks else (rows, K)
    nb2s = 1 if bcast else nb2
    buf = torch.full((nb1, nb2s, R, C + 8), float("nan"), dtype=dtype, device=DEV)
    buf[..., :C] = rnd((nb1, nb2s, R, C), gen, scale).to(dtype)
    vals = buf[..., :C]
    logical = vals.transpose(-1, -2) if ks else vals
    ld = C + 8
    return buf, logical, ((1, ld) if ks else (ld, 1)), (nb2s * R * ld, 0 if bcast else R * ld)


def frame(case, ld, dtype, sentinel):
    """flat buffer: ABOVE rows, then per batch M rows + GAP rows, at row pitch ld; returns (buf, view, c_off, bsC, inside)"""
    nb1, nb2 = case.nb
    plane = (case.M + GAP) * ld
    buf = torch.full(((ABOVE + nb1 * nb2 * (case.M + GAP)) * ld,), sentinel, dtype=dtype, device=DEV)
    c_off = ABOVE * ld
    size, stride = (nb1, nb2, case.M, case.N), (nb2 * plane, plane, ld, 1)
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    inside.as_strided(size, stride, c_off).fill_(True)
    return buf, buf.as_strided(size, stride, c_off), c_off, (nb2 * plane, plane), inside


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
    A, Av, sa, bsA = operand(M, K, a_ks, case.a, nb1, nb2, "A" in case.bcast, gen)
    B, Bv, sb, bsB = operand(N, K, b_ks, case.b, nb1, nb2, "B" in case.bcast, gen, K ** -0.5)

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
    C, Cv, c_off, bsC, c_in = frame(case, ldc, case.c, nan)
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
        aux, auxv, _, _, a_in = frame(case, ldc, adt, 0xA5 if adt == U8 else nan)
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

    def run(Cbuf, coff, ld, bs, defer=None, auxbuf=aux, csum=cs):
        with config.scope(f32_split=case.f32_split):
            ops.p_gemm(A, B, Cbuf, M, N, K, sa, sb, ld, c_off=coff, bias=bias, residual=res, ldr=N + 8, aux=auxbuf,
                       ldaux=ld, act=case.act, mul_dact=case.aux == "in", alpha=case.alpha, nb1=nb1, nb2=nb2, bsA=bsA,
                       bsB=bsB, bsC=bs, bsR=bsR, colsum=csum, aux_kind=case.aux_kind, defer=defer)

    # 1. route
    run(C, c_off, ldc, bsC)
    route = ops.gemm_last_route()
    family, tm, tn, splits, variant = case.route
    assert route == ops.GemmRoute(family, a_ks, b_ks, tm, tn, splits, variant), f"{case.name}: took {route}"
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
    with pytest.raises(ops.L.Unsupported):   # column sums need N % 256 == 0
        ops.p_gemm(x, w[:200], y, 256, 200, 128, (128, 1), (128, 1), 256, bias=torch.zeros(200, device=DEV),
                   colsum=torch.empty(200, device=DEV))
    assert ops.gemm_last_route() == ops.GemmRoute(None, False, False, 0, 0, 0, 0)


def test_table_reaches_every_instance():
    """the routes the table's rows took (test_gemm_route_and_value, run before this) cover every reachable instance"""
    expected = {c.name: instance_key(ops.GemmRoute(c.route[0], c.lay[0] == "k", c.lay[1] == "k", *c.route[1:]), c.lay)
                for c in CASES}
    missing = sorted(set(INSTANCES) - set(expected.values()))
    assert not missing, f"no case is meant to reach {missing}"
    not_run = sorted(set(expected) - set(_SEEN))
    assert not not_run, f"cases not run (or failed before their route was recorded): {not_run}"
    missing = sorted(set(INSTANCES) - set(_SEEN.values()))
    assert not missing, f"no case reached {missing}"
