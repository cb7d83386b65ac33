"""The route table of segclip_gemm, shared by tests/test_gemm_routes_gpu.py (which launches every row and checks its values) and
tests/test_gemm_plan_cpu.py (which plans every row without a GPU): one row per kernel instance and per way of reaching it, with
the route it must take, and the builders of a row's operands and output frames on a given device.

Instances and the cases that reach them:
  generic (gemm_bf16.hip, 128 x 128; A bf16 / fp32, aligned / ragged):
    ff: gen_ff_bf16_al, gen_ff_bf16_rag, gen_ff_f32_al, gen_ff_f32_rag
    fk: gen_fk_bf16_al, gen_fk_bf16_rag, gen_fk_f32_al_splitk, gen_fk_f32_rag
    kf: gen_kf_bf16_al, gen_kf_bf16_rag, gen_kf_f32_al_splitk, gen_kf_f32_rag_batched
    kk: gen_kk_bf16_al, gen_kk_bf16_rag_splitk, gen_kk_f32_al_batched, gen_kk_f32_rag
  dma (gemm_bf16_dma.hip) 256 x 128: dma0_ff, dma0_fk_colsum, dma0_kf_pitched, dma0_kk_batched
  dma 128 x 128: dma2_ff_res32, dma2_fk_splitk, dma2_kf_f32out, dma2_kk_batched, dma2_fk_colsum_rows128,
    dma2_ff_colsum_rows128, f32split_ff (the bf16 route of config.f32_split)
  The dma kernel has no 256 x 256 instance: a problem on 256-wide tiles that pq and p8 refuse for an operand pitch of 2 GiB or
    more per 256 rows (per 64 k-rows) runs on the 256 x 128 instance (planned in tests/test_gemm_plan_cpu.py; not launched).
  p8 (gemm_bf16_p8.hip): p8_ff_batched, p8_ff_colsum, p8_fk_splitk, p8_kf_f32out, p8_kk_splitk
  pq (gemm_bf16_pq.hip): forward pq_f_res_rows128, data gradient pq_k_dact8_colsum_rows128, weight gradient pq_w_splitk
  f32 (gemm_f32.hip): 32 x 128 f32_skinny, 64 x 64 f32_small_batched, 128 x 128 f32_large
The 256-wide tiles need more than 128 of them (the tile-count heuristic prefers 128-wide tiles below that), so the p8 and pq
cases are 8-9 M outputs with a short K.
"""
import dataclasses

import torch

from segclip_amd import ops

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
QG, ERF = ops.ACT_QUICK_GELU, ops.ACT_GELU_ERF
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


def expected_route(case):
    return ops.GemmRoute(case.route[0], case.lay[0] == "k", case.lay[1] == "k", *case.route[1:])


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


# ---- operands and frames.  gen = None: storage of the same shape and pitch only, nothing is computed (the planner reads addresses)
def rnd(shape, gen, scale=1.0):
    return torch.randn(*shape, generator=gen, device=gen.device, dtype=torch.float64) * scale


def operand(rows, K, ks, dtype, nb1, nb2, bcast, device, gen=None, scale=1.0):
    """storage (nb1, nb2 or 1, R, C + 8) with NaN in the pitch: k-contiguous R = rows, C = K; k-strided R = K, C = rows.
    Returns the storage, the logical (nb1, nb2|1, rows, K) values, (s_row, s_k) and the batch strides."""
    R, C = (K, rows) if ks else (rows, K)
    nb2s = 1 if bcast else nb2
    if gen is None:
        buf = torch.empty((nb1, nb2s, R, C + 8), dtype=dtype, device=device)
    else:
        buf = torch.full((nb1, nb2s, R, C + 8), float("nan"), dtype=dtype, device=device)
        buf[..., :C] = rnd((nb1, nb2s, R, C), gen, scale).to(dtype)
    vals = buf[..., :C]
    logical = vals.transpose(-1, -2) if ks else vals
    ld = C + 8
    return buf, logical, ((1, ld) if ks else (ld, 1)), (nb2s * R * ld, 0 if bcast else R * ld)


def frame(case, ld, dtype, sentinel, device, fill=True):
    """flat buffer: ABOVE rows, then per batch M rows + GAP rows, at row pitch ld; returns (buf, view, c_off, bsC, inside);
    fill = False: uninitialised storage and no `inside` mask"""
    nb1, nb2 = case.nb
    plane = (case.M + GAP) * ld
    n = (ABOVE + nb1 * nb2 * (case.M + GAP)) * ld
    c_off = ABOVE * ld
    size, stride = (nb1, nb2, case.M, case.N), (nb2 * plane, plane, ld, 1)
    if not fill:
        buf = torch.empty((n,), dtype=dtype, device=device)
        return buf, buf.as_strided(size, stride, c_off), c_off, (nb2 * plane, plane), None
    buf = torch.full((n,), sentinel, dtype=dtype, device=device)
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=device)
    inside.as_strided(size, stride, c_off).fill_(True)
    return buf, buf.as_strided(size, stride, c_off), c_off, (nb2 * plane, plane), inside


def split3_operands(case, device, C, ldc):
    """the positional arguments of the bf16 call ops.p_gemm turns a config.f32_split case into (ops._gemm_f32_split: dense
    (rows, 3 K) parts of k-contiguous operands, no batch); storage only"""
    assert case.lay == "ff" and case.f32_split and case.nb == (1, 1)
    K3 = 3 * case.K
    return (torch.empty((case.M, K3), dtype=BF, device=device), torch.empty((case.N, K3), dtype=BF, device=device), C,
            case.M, case.N, K3, (K3, 1), (K3, 1), ldc)
