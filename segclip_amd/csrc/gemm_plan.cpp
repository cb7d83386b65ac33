// The planner of segclip_gemm (gemm_plan.h).  Host code only: no HIP call, no memory read.  Every predicate of the dispatch
// stands here once; gemm_plan() below is the order in which they are asked.
#include "gemm_plan.h"

namespace {

constexpr int BK = GEMM_BK, BT = GEMM_BIG_TILE;
constexpr int64_t LIM31 = (int64_t)1 << 31;

const char* const MSG_COLSUM = "gemm: fused colsum unsupported for this shape";
const char* const MSG_RES_ROW_MOD = "gemm: res_row_mod needs the fp32-residual epilogue on full 256 x 256 bf16 tiles";
const char* const MSG_AUX8 = "gemm: aux_kind 2 needs full 256 x 256 tiles, 16-byte aligned operands and no split-K";

#define PLAN_FAIL(code, ...)        \
  do {                              \
    segclip_set_error(__VA_ARGS__); \
    p.rc = (code);                  \
    return p;                       \
  } while (0)
#define PLAN_REQUIRE(cond, ...)                                  \
  do {                                                           \
    if (!(cond)) PLAN_FAIL(SEGCLIP_ERR_INVALID, __VA_ARGS__);    \
  } while (0)

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // a null pointer counts as aligned
bool a_ks(const segclip_gemm_desc* d) { return d->sak != 1; }
bool b_ks(const segclip_gemm_desc* d) { return d->sbk != 1; }
int64_t lda(const segclip_gemm_desc* d) { return a_ks(d) ? d->sak : d->sam; }
int64_t ldb(const segclip_gemm_desc* d) { return b_ks(d) ? d->sbk : d->sbn; }
int64_t batches(const segclip_gemm_desc* d) { return (d->nb1 > 0 ? d->nb1 : 1) * (d->nb2 > 0 ? d->nb2 : 1); }
bool plain_epilogue(const segclip_gemm_desc* d) {
  return !(d->bias || d->residual || d->aux || d->act != SEGCLIP_ACT_NONE || d->mul_dact);
}
bool aux8(const segclip_gemm_desc* d) { return d->aux_kind == 2 && d->aux; }   // the saved derivative as one byte per element

// ---- which bf16 problems leave the register-staged kernel ----------------------------------------------------------------
// operand rows on 16-byte boundaries: the unguarded 16-byte loads of the generic kernel, and every LDS-DMA kernel
bool aligned16(const segclip_gemm_desc* d) {
  const int64_t aes = d->a_dtype == SEGCLIP_F32 ? 4 : 2;
  bool fast = al16(d->A) && al16(d->B) && lda(d) % 8 == 0 && ldb(d) % 8 == 0 && (d->bsA1 * aes) % 16 == 0 &&
              (d->bsA2 * aes) % 16 == 0 && (d->bsB1 * 2) % 16 == 0 && (d->bsB2 * 2) % 16 == 0;
  fast = fast && (a_ks(d) ? (d->M % 8 == 0 && d->M >= 8) : (d->K % 8 == 0 && d->K >= 8));
  fast = fast && (b_ks(d) ? (d->N % 8 == 0 && d->N >= 8) : (d->K % 8 == 0 && d->K >= 8));
  return fast;
}
// the LDS-DMA kernels (dma, p8, pq) take the large aligned bf16 x bf16 problems; K must be a multiple of 64, and for tiny
// problems the 128 x 128 kernel wastes less.  Everything below `want_dma` may rely on these conditions.
bool want_dma(const segclip_gemm_desc* d) {
  return d->a_dtype == SEGCLIP_BF16 && d->b_dtype == SEGCLIP_BF16 && aligned16(d) && d->K % BK == 0 && d->K >= BK &&
         d->M >= 64 && d->N >= 16;
}

// ---- split-K ------------------------------------------------------------------------------------------------------------
// the split count a sufficient workspace would give (plain epilogue only)
int choose_splits(const segclip_gemm_desc* d) {
  if (!plain_epilogue(d)) return 1;
  const int64_t nb = batches(d);
  const int64_t ksteps = cdiv(d->K, BK);
  if (want_dma(d)) {
    // 256-row tiles, long K loops: aim at one full round of the 256 CUs
    const int64_t bn = d->N > 128 ? 256 : 128;
    const int64_t tiles = cdiv(d->M, 256) * cdiv(d->N, bn) * nb;
    if (tiles >= 160 || ksteps < 32) return 1;
    int64_t s = 256 / tiles;
    if (s > ksteps / 8) s = ksteps / 8;
    if (s > 32) s = 32;
    return s < 1 ? 1 : (int)s;
  }
  const int64_t tiles = cdiv(d->M, GEMM_TILE) * cdiv(d->N, GEMM_TILE) * nb;
  if (tiles >= 384 || ksteps < 16) return 1;
  int64_t s = cdiv(768, tiles);
  if (s > ksteps / 4) s = ksteps / 4;
  if (s > 32) s = 32;
  return s < 1 ? 1 : (int)s;
}
size_t splitk_bytes(const segclip_gemm_desc* d, int splits) {
  return splits <= 1 ? 0 : (size_t)splits * batches(d) * d->M * d->N * sizeof(float);
}
// the splits of this call: 1 without a sufficient workspace; K ranges of whole K steps (so kper % 64 == 0), empty ones dropped
int resolve_splits(const segclip_gemm_desc* d, int64_t* kper) {
  int splits = choose_splits(d);
  if (splits > 1 && (d->ws == nullptr || (size_t)d->ws_bytes < splitk_bytes(d, splits))) splits = 1;
  *kper = splits > 1 ? cdiv(cdiv(d->K, BK), splits) * BK : d->K;
  return splits > 1 ? (int)cdiv(d->K, *kper) : 1;
}

// ---- tiles of the LDS-DMA kernels ---------------------------------------------------------------------------------------
// tile-count heuristic: the 256x256 tile unless it leaves the 256 CUs badly quantised and 256x128 does not
int pick_bn(const segclip_gemm_desc* d, int64_t nbatch_splits) {
  if (d->N <= 128) return 128;
  auto eff = [&](int bn) {
    const double tiles = (double)cdiv(d->M, BT) * cdiv(d->N, bn) * nbatch_splits;
    const double rounds = tiles / 256.0;
    const double q = rounds / (double)(int64_t)(rounds + 0.999999);  // quantisation efficiency
    const double pad = (double)d->N / (cdiv(d->N, bn) * bn);
    return q * pad * (bn == 256 ? 1.0 : 0.72);                       // 256x128 runs at ~0.72 of the 256x256 rate
  };
  return eff(256) >= eff(128) ? 256 : 128;
}
// 128x128 tiles, 4 waves, 68 KiB of LDS -> two workgroups per CU: the per-tile prologue / output phase of one
// overlaps the MFMA phase of the other.  In isolation (tools/bench_gemm.py, MI355X) this wins 10-25 % on the
// forward GEMMs with fewer than 4 rounds of 256x256 tiles (N=768 of the vision tower, the whole text tower) and
// loses 5-15 % on long-K dgrads and every split-K wgrad; inside the training step (text tower concurrent on a
// second stream) a shape-based choice measured 58.4 vs 58.2 ms, i.e. no gain, so the 256-wide tiles stay the default.
// Round 4: problems whose 256-row tiles cannot fill the 256 CUs (the center stage's q-side linears: M = 8 B = 2048 rows,
// 48-192 tiles) take the 128x128 tile: four times the workgroups, two per CU, half the K-loop time per tile
// (a forward + backward pass of the center stage: see DESIGN 4.4).
bool dma_small_tiles(const segclip_gemm_desc* d, int64_t nb, int splits, bool colsum, int bn_big) {
  // fused column sums come from the staged epilogue of FULL tiles only (a partial tile takes the per-element epilogue, which
  // writes no partial sums): M = 256 q + 128 runs them on the 128-row tiles, where every tile is full (colsum_shape_ok)
  if (colsum) return d->M % 256 != 0;
  return d->M >= 128 && d->N >= 128 && !aux8(d) && cdiv(d->M, 256) * cdiv(d->N, bn_big) * nb * splits < 256;
}

// ---- epilogues ----------------------------------------------------------------------------------------------------------
// fused column sums exist in the staged epilogues of full tiles, without batches and split-K
bool colsum_shape_ok(const segclip_gemm_desc* d, int64_t nb, int splits) {
  return want_dma(d) && d->M % 128 == 0 && d->N % 256 == 0 && splits == 1 && nb == 1;
}
// dma / p8: every C / aux / residual / bias access of a full tile may be a 16-byte vector (the LDS-staged epilogue)
int vec_epi(const segclip_gemm_desc* d) {
  const int64_t ce = d->c_dtype == SEGCLIP_BF16 ? 8 : 4, re = d->r_dtype == SEGCLIP_BF16 ? 8 : 4;
  if (d->residual && d->r_dtype != d->c_dtype) return 0;   // the LDS epilogue holds side operands in the output type
  return al16(d->C) && al16(d->aux) && al16(d->residual) && al16(d->bias) && d->ldc % ce == 0 &&
         (!d->aux || d->ldaux % ce == 0) && (!d->residual || d->ldr % re == 0) && d->bsC1 % ce == 0 &&
         d->bsC2 % ce == 0 && (!d->residual || (d->bsR1 % re == 0 && d->bsR2 % re == 0));
}
// what dma and p8 share: column sums and the one-byte derivative exist in the staged epilogue only
bool staged_epilogue_covers(const segclip_gemm_desc* d, int vec, int splits, bool colsum) {
  if (colsum && !vec) return false;
  if (!aux8(d)) return true;
  // the one-byte derivative of the erf-GELU is produced by gemm_bf16_pq.hip only (this epilogue: QuickGELU); decoding is generic
  if (!d->mul_dact && d->act != SEGCLIP_ACT_QUICK_GELU) return false;
  // aux_kind 2 exists in the staged epilogue of FULL tiles only (8-byte aligned rows)
  return vec && d->M % 256 == 0 && d->N % 256 == 0 && d->ldaux % 8 == 0 && d->c_dtype == SEGCLIP_BF16 && splits == 1;
}
bool dma_covers(const segclip_gemm_desc* d, int vec, int splits, bool colsum) {
  return staged_epilogue_covers(d, vec, splits, colsum);
}
// asked only where pick_bn chose 256-wide tiles (so N > 128).  Of the problems dma_covers takes, this kernel refuses two kinds:
// column sums off full 256 x 256 tiles, which dma_small_tiles sends to the 128 x 128 instance, and the operand pitches below,
// which plan_dma runs on 256 x 128 tiles (gemm_bf16_dma.hip forms every address in 64 bits)
bool p8_covers(const segclip_gemm_desc* d, int vec, int splits, bool colsum) {
  // 32-bit DMA offsets: 256 rows (or 64 k-rows) of the leading dimension must stay below 2 GiB
  if ((a_ks(d) ? 64 : 256) * lda(d) * 2 >= LIM31 || (b_ks(d) ? 64 : 256) * ldb(d) * 2 >= LIM31) return false;
  // a partial tile's per-element epilogue writes no column sums: M = 256 q + 128 goes to the 128-row tiles of gemm_bf16_dma.hip
  if (colsum && (d->M % BT != 0 || d->N % BT != 0)) return false;
  return staged_epilogue_covers(d, vec, splits, colsum);
}

// ---- gemm_bf16_pq.hip ---------------------------------------------------------------------------------------------------
// Half-tile tail plan: the r = ntiles % 256 tiles of the last, partial round run as 2 r workgroups of 128 x 256 when those fit
// one round (r <= 128): 591 tiles (N = 768 at M = 50432) are 2.3 rounds of 256 CUs and take the time of 3; the third round
// then costs a half-tile's time (about 0.6 of a tile's: 3 of 4 operand units per K-tile, half the MFMAs, half the output).
// No exchange between workgroups, results bit-identical to the full tiles'.
int pq_half_tail(int64_t ntiles) {
  if (ntiles <= 256) return 0;
  const int r = (int)(ntiles % 256);
  return r > 0 && r <= 128 ? r : 0;
}
// weight gradient: C(m,n) = sum_k A[k][m] B[k][n], fp32 out (split-K: raw partial tiles into the slabs)
bool pq_covers_wgrad(const segclip_gemm_desc* d, int splits, bool colsum) {
  if (!b_ks(d) || d->c_dtype != SEGCLIP_F32 || !plain_epilogue(d) || colsum) return false;
  if (splits == 1 && (d->alpha != 1.0f || d->ldc % 4 != 0 || !al16(d->C))) return false;
  if (splits > 1 && (d->N % 4 != 0 || !al16(d->ws))) return false;
  // 32-bit per-lane offsets: 64 k-rows of an operand and 256 rows of the output (the slab's pitch is N) stay below 2 GiB
  return 64 * d->sak * 2 < LIM31 && 64 * d->sbk * 2 < LIM31 && 256 * (splits > 1 ? d->N : d->ldc) * 4 < LIM31;
}
// forward + fp32 residual -> fp32 (the fp32 residual stream): fp32 patches, fp32 row pass
bool pq_covers_res32(const segclip_gemm_desc* d, bool colsum) {
  if (b_ks(d) || d->residual == nullptr || d->r_dtype != SEGCLIP_F32 || d->alpha != 1.0f) return false;
  if (d->aux || d->act != SEGCLIP_ACT_NONE || d->mul_dact || colsum) return false;
  if (!al16(d->C) || !al16(d->bias) || !al16(d->residual) || d->ldc % 4 != 0 || d->ldr % 4 != 0) return false;
  return 256 * d->sam * 2 < LIM31 && 256 * d->sbn * 2 < LIM31 && 256 * d->ldc * 4 < LIM31;
}
// bf16 outputs: the epilogue mode, or -1
int pq_covers_bf16(const segclip_gemm_desc* d, bool colsum) {
  if (d->c_dtype != SEGCLIP_BF16 || d->alpha != 1.0f) return -1;
  const bool gelu = d->act == SEGCLIP_ACT_QUICK_GELU || d->act == SEGCLIP_ACT_GELU_ERF;   // (the byte is decoded the same way)
  int mode = PQ_PLAIN;
  if (d->residual != nullptr) {   // + bf16 residual -> bf16 (the bf16 residual stream of the towers): forward layout only
    if (d->r_dtype != SEGCLIP_BF16 || b_ks(d) || d->mul_dact || d->act != SEGCLIP_ACT_NONE || d->aux || d->ldr % 8 != 0) return -1;
    mode = PQ_RES;
  } else if (d->mul_dact) {       // x act'(u), saved as one byte; optional fused column sums
    if (!(aux8(d) && gelu && !d->bias && b_ks(d) && d->ldaux % 16 == 0)) return -1;
    mode = PQ_DACT8;
  } else if (d->act != SEGCLIP_ACT_NONE) {   // QuickGELU / erf-GELU + saved derivative as one byte
    if (!(aux8(d) && gelu && !b_ks(d) && d->ldaux % 16 == 0)) return -1;
    mode = d->act == SEGCLIP_ACT_QUICK_GELU ? PQ_ACT8 : PQ_ACT8E;
  } else if (d->aux) {
    return -1;
  }
  if (colsum && mode != PQ_DACT8) return -1;
  if (!al16(d->C) || !al16(d->bias) || !al16(d->aux) || !al16(d->residual) || d->ldc % 8 != 0) return -1;
  // 32-bit per-lane offsets: 256 rows (64 k-rows) of an operand and 256 rows of an output stay below 2 GiB
  if (256 * d->sam * 2 >= LIM31 || (b_ks(d) ? 64 : 256) * ldb(d) * 2 >= LIM31) return -1;
  if (256 * d->ldc * 2 >= LIM31 || 256 * d->ldaux >= LIM31) return -1;
  return mode;
}
// the epilogue mode with which the accumulator-register kernel takes a `want_dma` problem, or -1: full 256 x 256 tiles, no
// batch, split-K in the weight gradient only
int pq_covers(const segclip_gemm_desc* d, int64_t nb, int splits, bool colsum) {
  if (nb != 1 || d->M < 128 || d->N % BT != 0) return -1;
  // M = 256 q + 128 (the token rows of an odd multiple of 128 samples x 197 / 577 / 77 tokens): the last 128 rows run as a
  // row of half-tiles (forward / data-gradient layouts; the weight gradient's M is a weight dimension)
  if (d->M % BT != 0 && (d->M % 128 != 0 || a_ks(d))) return -1;
  if (a_ks(d)) return pq_covers_wgrad(d, splits, colsum) ? PQ_SLAB : -1;
  if (splits != 1) return -1;
  // only the fp32-residual epilogue addresses the residual modulo a row count
  if (d->res_row_mod > 0 && !(d->c_dtype == SEGCLIP_F32 && d->residual != nullptr && d->r_dtype == SEGCLIP_F32)) return -1;
  if (d->c_dtype == SEGCLIP_F32) return pq_covers_res32(d, colsum) ? PQ_RES32 : -1;
  return pq_covers_bf16(d, colsum);
}

// ---- one family each: the route and what its launcher needs; false = not taken ------------------------------------------------
void set_route(GemmPlan& p, const segclip_gemm_desc* d, int family, int tile_m, int tile_n, int splits, int variant) {
  p.route = segclip_gemm_route{family, a_ks(d), b_ks(d), tile_m, tile_n, splits, variant};
  p.nbx = (int)cdiv(d->N, tile_n);
  p.nby = (int)cdiv(d->M, tile_m);
}
bool plan_pq(GemmPlan& p, const segclip_gemm_desc* d, int splits, bool colsum) {
  const int mode = pq_covers(d, p.nb, splits, colsum);
  if (mode < 0) return false;
  const int nbx = (int)(d->N / BT), ntiles = (int)(d->M / BT) * nbx;   // full tiles
  p.pq_mode = mode;
  if (mode == PQ_SLAB) {
    set_route(p, d, SEGCLIP_GEMM_ROUTE_PQ, BT, BT, splits, PQ_SLAB);
    p.nwg = (unsigned)(ntiles * splits);
    return true;
  }
  const int hx = d->M % BT != 0 ? nbx : 0;       // M = 256 q + 128: one more row of half-tiles
  const int hr = pq_half_tail(ntiles);
  if (hr > 0 || hx > 0) { p.half_r = hr; p.half_x = hx; p.nfull = ntiles - hr; }
  p.nwg = (unsigned)(ntiles + hr + hx);
  // variant: epilogue mode | tail tiles run as half-tiles << 4 | half-tiles of a last row of 128 rows << 16
  set_route(p, d, SEGCLIP_GEMM_ROUTE_PQ, BT, BT, 1, mode | (hr << 4) | (hx << 16));
  return true;
}
bool plan_p8(GemmPlan& p, const segclip_gemm_desc* d, int splits, bool colsum) {
  if (!p8_covers(d, p.vec_epi, splits, colsum)) return false;
  set_route(p, d, SEGCLIP_GEMM_ROUTE_P8, BT, BT, splits, 0);
  return true;
}
bool plan_dma(GemmPlan& p, const segclip_gemm_desc* d, int splits, bool colsum) {
  if (!dma_covers(d, p.vec_epi, splits, colsum)) return false;
  // bn_big = 256 here: pq and p8 refused the 256 x 256 tiles pick_bn chose - off the small-tile rule that is an operand pitch of
  // 2 GiB per 256 rows (p8_covers), and this kernel has no 256-wide instance: 256 x 128 tiles, whose addresses are 64-bit
  const int bn_big = pick_bn(d, p.nb * splits);
  if (dma_small_tiles(d, p.nb, splits, colsum, bn_big)) set_route(p, d, SEGCLIP_GEMM_ROUTE_DMA, 128, 128, splits, DMA_128x128);
  else set_route(p, d, SEGCLIP_GEMM_ROUTE_DMA, 256, 128, splits, DMA_256x128);
  return true;
}

GemmPlan plan_bf16(GemmPlan p, const segclip_gemm_desc* d) {
  PLAN_REQUIRE(!a_ks(d) || d->sam == 1, "gemm_bf16: A needs unit stride along k or m (sam=%lld sak=%lld)",
               (long long)d->sam, (long long)d->sak);
  PLAN_REQUIRE(!b_ks(d) || d->sbn == 1, "gemm_bf16: B needs unit stride along k or n (sbn=%lld sbk=%lld)",
               (long long)d->sbn, (long long)d->sbk);
  p.nb = batches(d);
  PLAN_REQUIRE(p.nb <= 65535, "gemm_bf16: batch too large (%lld)", (long long)p.nb);
  const int splits = resolve_splits(d, &p.kper);
  const bool dma = want_dma(d);
  if (d->colsum) {
    PLAN_REQUIRE(d->colsum_ws != nullptr, "gemm: colsum needs colsum_ws");
    if (!colsum_shape_ok(d, p.nb, splits)) PLAN_FAIL(SEGCLIP_ERR_UNSUPPORTED, "%s", MSG_COLSUM);
    p.colsum = true;
  }
  if (dma) p.vec_epi = vec_epi(d);
  bool taken = false;
  if (d->res_row_mod > 0) {   // only gemm_bf16_pq.hip's fp32-residual epilogue addresses the residual modulo a row count
    taken = dma && p.nb == 1 && splits == 1 && plan_pq(p, d, 1, p.colsum);
    if (!taken) PLAN_FAIL(SEGCLIP_ERR_UNSUPPORTED, "%s", MSG_RES_ROW_MOD);
  } else if (dma) {
    // 256x256 tiles: the accumulator-register kernel (gemm_bf16_pq.hip) where it takes the problem, else the phase-pipelined
    // kernel (gemm_bf16_p8.hip); 256x128 / 128x128 tiles: the one-barrier-per-K-tile kernel (gemm_bf16_dma.hip)
    if (pick_bn(d, p.nb * splits) == 256) taken = plan_pq(p, d, splits, p.colsum) || plan_p8(p, d, splits, p.colsum);
    if (!taken) taken = plan_dma(p, d, splits, p.colsum);
  }
  if (p.colsum && !taken) PLAN_FAIL(SEGCLIP_ERR_UNSUPPORTED, "%s", MSG_COLSUM);
  if (!taken && aux8(d)) PLAN_FAIL(SEGCLIP_ERR_UNSUPPORTED, "%s", MSG_AUX8);
  if (!taken) {   // the register-staged kernel: variant bit 0 = fp32 A operand, bit 1 = unguarded 16-byte operand loads
    p.vec_epi = 0;
    set_route(p, d, SEGCLIP_GEMM_ROUTE_GENERIC, GEMM_TILE, GEMM_TILE, splits,
              (d->a_dtype == SEGCLIP_F32 ? 1 : 0) | (aligned16(d) ? 2 : 0));
  }
  return p;
}

}  // namespace

size_t gemm_splitk_ws_bytes(const segclip_gemm_desc* d) {
  return d->b_dtype == SEGCLIP_BF16 ? splitk_bytes(d, choose_splits(d)) : 0;
}
int gemm_splits(const segclip_gemm_desc* d) {
  int64_t kper;
  return d->b_dtype == SEGCLIP_BF16 ? resolve_splits(d, &kper) : 1;
}
int gemm_pq_half_tail(int64_t ntiles) { return pq_half_tail(ntiles); }

GemmPlan gemm_plan_f32(const segclip_gemm_desc* d) {
  GemmPlan p;
  p.nb = batches(d);
  p.kper = d->K;
  // M <= 32: 32 x 128 tiles.  Otherwise, with fewer than half a chip of 128 x 128 tiles: 64 x 64 tiles (4x the workgroups),
  // K-step 64.  256 x 256 x 512: 94 -> 39 us (K-step 128: 47 us - the time is the LDS staging and the one-accumulator MFMA
  // chain of a wave, not the round trips)
  const bool skinny = d->M <= 32;
  const bool small = !skinny && cdiv(d->N, 128) * cdiv(d->M, 128) * p.nb < 128;
  const int bm = skinny ? 32 : (small ? 64 : 128), bn = skinny ? 128 : (small ? 64 : 128);
  PLAN_REQUIRE((unsigned)cdiv(d->M, bm) <= 65535 && p.nb <= 65535, "gemm_f32: grid too large (M=%lld batch=%lld)",
               (long long)d->M, (long long)p.nb);
  set_route(p, d, SEGCLIP_GEMM_ROUTE_F32, bm, bn, 1, skinny ? F32_32x128 : small ? F32_64x64 : F32_128x128);
  return p;
}

GemmPlan gemm_plan(const segclip_gemm_desc* d) {
  GemmPlan p;
  PLAN_REQUIRE(d != nullptr, "gemm: null descriptor");
  PLAN_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, "gemm: negative size");
  if (d->M == 0 || d->N == 0) return p;
  p.ws_bytes = gemm_splitk_ws_bytes(d);
  PLAN_REQUIRE(d->A && d->B && d->C, "gemm: null operand");
  PLAN_REQUIRE(!d->mul_dact || d->aux, "gemm: mul_dact needs aux");
  PLAN_REQUIRE(d->aux_kind == 0 || ((d->aux_kind == 1 || d->aux_kind == 2) && d->act == SEGCLIP_ACT_QUICK_GELU) ||
                   (d->aux_kind == 2 && d->act == SEGCLIP_ACT_GELU_ERF),
               "gemm: aux_kind 1 (aux = act'(pre-activation) in the output type) is implemented for QuickGELU only, aux_kind 2 for QuickGELU and erf-GELU");
  PLAN_REQUIRE(d->aux_kind != 2 || (d->a_dtype == SEGCLIP_BF16 && d->b_dtype == SEGCLIP_BF16 && d->c_dtype == SEGCLIP_BF16),
               "gemm: aux_kind 2 (one byte per element) needs bf16 operands and output");
  if (d->res_row_mod > 0 && !(d->a_dtype == SEGCLIP_BF16 && d->b_dtype == SEGCLIP_BF16))
    PLAN_FAIL(SEGCLIP_ERR_UNSUPPORTED, "gemm: res_row_mod is a bf16-operand feature");
  if (d->a_dtype == SEGCLIP_F32 && d->b_dtype == SEGCLIP_F32) {
    PLAN_REQUIRE(d->c_dtype == SEGCLIP_F32 && (!d->residual || d->r_dtype == SEGCLIP_F32), "gemm f32: output / residual must be f32");
    GemmPlan f = gemm_plan_f32(d);
    f.ws_bytes = p.ws_bytes;
    return f;
  }
  if (d->b_dtype == SEGCLIP_BF16) return plan_bf16(p, d);
  PLAN_FAIL(SEGCLIP_ERR_UNSUPPORTED, "gemm: unsupported dtype combination a=%d b=%d", d->a_dtype, d->b_dtype);
}
