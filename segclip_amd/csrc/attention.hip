// Multi-head attention core, head_dim <= 64, arbitrary (batch, token) strides for Q/K/V/O.
//
// bf16 path (flash style, never materialises the score matrix in HBM):
//   forward : block = (b, h, group of <=8 query tiles of 32 rows), one wave per query tile.  K/V of a
//             256-key chunk are staged once in LDS (swizzled 128-B rows).  Each wave computes the
//             *transposed* score tile S^T = K Q^T with v_mfma_f32_32x32x16_bf16, so a lane owns one
//             query row: the online-softmax max/sum are 16 in-lane ops + one cross-half shuffle.  P^T is
//             fed straight back as the B operand of O^T = V^T P^T; the V^T fragment comes from the LDS
//             transpose read ds_read_b64_tr_b16 with the key order permuted to match the accumulator
//             layout, so P never leaves registers.
//   backward: block = (b, h); Q, K, V, dO tiles in LDS (<=256 tokens each).  Pass A (wave owns a key
//             tile) accumulates dK, dV; pass B (wave owns a query tile) accumulates dQ.  S and dP are
//             recomputed in both passes (no atomics, deterministic).
// f32 path (exact parity mode): S = scale*Q K^T, row softmax, O = P V as three launches of the f32 MFMA
//   GEMM + a softmax kernel; P is kept for backward (5 GEMMs + one elementwise kernel).
#include <stdlib.h>
#include <algorithm>
#include <atomic>

#include "common.h"
#include "attention_tile_image.h"
#include "lds_ops.h"

int segclip_gemm_f32_launch(const segclip_gemm_desc* d, hipStream_t stream);

namespace {

constexpr int ROWB = tileimg::ROWB;  // bytes per LDS row (64 bf16)

using tileimg::swz;   // byte offset of element (row, col) in a [rows][64] bf16 LDS tile: the row image

// MFMA operand fragment, k-contiguous rows: lane l -> row rbase + (l&31), cols kc*16 + 8*(l>>5) .. +7
__device__ __forceinline__ bf16x8_t frag_rows(const char* t, int rbase, int kc, int lane) {
  return *reinterpret_cast<const bf16x8_t*>(t + tileimg::frag_rows_at(rbase, kc, lane));
}
// MFMA operand fragment of the TRANSPOSED tile: lane l -> "row" = column cbase + (l&31) of the tile,
// k = tile rows  rbase + 4*(l>>5) + {0,1,2,3, 8,9,10,11}   (the key order of the 32x32 accumulator)
__device__ __forceinline__ bf16x8_t frag_tr(const char* t, int rbase, int cbase, int lane) {
  const int row = tileimg::frag_tr_row(rbase, lane), col = tileimg::frag_tr_col(cbase, lane);
  const s16x4 lo = tr16_read(t + swz(row, col));
  const s16x4 hi = tr16_read(t + swz(tileimg::frag_tr_hi(row), col));
  return tr16_join(lo, hi);
}
typedef float v2f __attribute__((ext_vector_type(2)));
// Lane offsets of the transposed fragments of a tile's first 16 rows, kept in registers by the kernels (voff / toff):
// tileimg::frag_tr_at(0, 32 dt, lane, j).  A call of that function changes the emitted code of every kernel, so the arithmetic
// is spelled out here, once, and the static_assert holds it to the header.  attention_pf.inc and attention_dqw.inc need the very
// statements of the macro in their kernel bodies (even tr_lane_off changes their code).
#define TR_LANE_OFF(g4, q, dt, j) swz(4 * ((g4) >> 1) + ((q) >> 2) + 8 * (j), (dt) * 32 + 16 * ((g4) & 1) + 4 * ((q) & 3))
OPIMG_FN int tr_lane_off(int lane, int dt, int j) {
  const int g4 = lane >> 4, q = lane & 15;
  return TR_LANE_OFF(g4, q, dt, j);
}
constexpr bool tr_lane_off_follows_image() {
  for (int lane = 0; lane < 64; ++lane)
    for (int dt = 0; dt < 2; ++dt)
      for (int j = 0; j < 2; ++j)
        if (tr_lane_off(lane, dt, j) != tileimg::frag_tr_at(0, dt * 32, lane, j)) return false;
  return true;
}
static_assert(tr_lane_off_follows_image(), "attention: TR_LANE_OFF must be the lane offset of tileimg::frag_tr_at");
// f(r) of the row image (tileimg::row_xor) as one expression, for the loader lambdas of attention_dma_tile.inc: with any call in
// them hipcc emits other code for both kernels that include them
#define ROW_XOR(r) ((((((r) >> 1) & 7) & 1) << 2) | ((((r) >> 1) & 7) >> 1))
constexpr bool row_xor_follows_image() {
  for (int r = 0; r < 256; ++r)
    if (ROW_XOR(r) != tileimg::row_xor(r)) return false;
  return true;
}
static_assert(row_xor_follows_image(), "attention: ROW_XOR must be tileimg::row_xor");
__device__ __forceinline__ bf16x8_t pack8(const float* p) {
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = pack2bf(p[2 * j], p[2 * j + 1]);
  return __builtin_bit_cast(bf16x8_t, r);
}
using tileimg::acc_row;   // accumulator row index of register r for lane half h (32x32 tile)

// stage `nrows_pad` rows (zero-filled beyond nvalid / beyond hd) of X[row*st + d] into a swizzled tile.
// Loads are unconditional from clamped addresses and issued in batches of 4 before any LDS write (a load
// inside a divergent branch is waited for individually by hipcc and the staging becomes latency-serial).
__device__ __forceinline__ void stage_rows(char* tile, const bf16_t* __restrict__ X, int64_t st, int row0, int nvalid,
                                           int nrows_pad, int hd, int tid, int nthreads) {
  const int total = nrows_pad * 8;
  for (int base = 0; base < total; base += 4 * nthreads) {
    u32x4 v[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = tileimg::stage_index(base, it, nthreads, tid);
      const int r = tileimg::stage_row(idx), c = tileimg::stage_chunk(idx);
      const int rc = tileimg::clamp_row(r, nvalid);
      const int cc = c * 8 < hd ? c : 0;   // tileimg::clamp_chunk; as a call it changes the code of every kernel that stages rows
      v[it] = *reinterpret_cast<const u32x4*>(X + (int64_t)(row0 + rc) * st + cc * 8);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = tileimg::stage_index(base, it, nthreads, tid);
      const int r = tileimg::stage_row(idx), c = tileimg::stage_chunk(idx);
      if (idx < total) {
        const bool ok = r < nvalid && c * 8 < hd;
        *reinterpret_cast<u32x4*>(tile + swz(r, c * 8)) = ok ? v[it] : u32x4{0u, 0u, 0u, 0u};
      }
    }
  }
}

struct FwdArgs {
  const bf16_t* Q; const bf16_t* K; const bf16_t* V; bf16_t* O; float* lse;
  int H, Tq, Tk, hd;
  int64_t q_sb, q_st, k_sb, k_st, v_sb, v_st, o_sb, o_st;
  float scale; int causal;
  const int* klen;  // nullable: valid keys per sample
  int staged;       // bf16 forward: output rows through LDS (plan_fwd: more than 128 queries)
  int lean;         // bf16 forward: the lean softmax step on unmasked key tiles (segclip_attn_fwd passes 1)
};

constexpr int KCHUNK = 256;

// 4 waves per SIMD (two 7-wave workgroups per CU): at most 128 VGPRs
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_fwd_bf16_kernel(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2 * KCHUNK * ROWB];
  char* Kt = smem;
  char* Vt = smem + KCHUNK * ROWB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int q0 = (blockIdx.x * nw + wave) * 32;
  const int li = lane & 31, lh = lane >> 5;
  const bf16_t* Qp = a.Q + (int64_t)b * a.q_sb + (int64_t)h * a.hd;
  const bf16_t* Kp = a.K + (int64_t)b * a.k_sb + (int64_t)h * a.hd;
  const bf16_t* Vp = a.V + (int64_t)b * a.v_sb + (int64_t)h * a.hd;
  const int qg = q0 + li;
  const bool wave_active = q0 < a.Tq;
  const int kvalid = a.klen ? (a.klen[b] < a.Tk ? a.klen[b] : a.Tk) : a.Tk;
  const float sc2 = a.scale * 1.4426950408889634f;  // scale * log2(e): the running max m is kept in the log2 domain

  bf16x8_t qf[4];
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
    const int d = kc * 16 + 8 * lh;
    const bool ok = qg < a.Tq && d < a.hd;
    const u32x4 raw = *reinterpret_cast<const u32x4*>(Qp + (int64_t)(qg < a.Tq ? qg : a.Tq - 1) * a.q_st + (d < a.hd ? d : 0));
    const u32x4 v = ok ? raw : u32x4{0u, 0u, 0u, 0u};
    qf[kc] = __builtin_bit_cast(bf16x8_t, v);
  }
  f32x16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
  float m = -INFINITY, l = 0.f;
  // lane-constant LDS offsets of the K fragments (k chunk kc) and of the four 8-row groups of the transposed V fragments
  // (V: rows r0 and r0 + 8 of a 32-key tile per 32-column half; rows + 16 / + 24 are the same offsets + 2048 bytes, since
  // the swizzle only looks at bits 1-3 of the row)
  int koff[4], voff[2][2];
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) koff[kc] = swz(li, tileimg::frag_rows_col(kc, lh));
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int j = 0; j < 2; ++j) voff[dt][j] = tr_lane_off(lane, dt, j);

  for (int c0 = 0; c0 < a.Tk; c0 += KCHUNK) {
    const int nvalid = a.Tk - c0 < KCHUNK ? a.Tk - c0 : KCHUNK;
    const int npad = (nvalid + 31) & ~31;
    __syncthreads();
    stage_rows(Kt, Kp, a.k_st, c0, nvalid, npad, a.hd, tid, blockDim.x);
    stage_rows(Vt, Vp, a.v_st, c0, nvalid, npad, a.hd, tid, blockDim.x);
    __syncthreads();
    if (!wave_active) continue;
    // Unmasked key tiles (all but the last one of a vision sequence) take a leaner softmax step (round 4; PMC round 3: 27 VALU
    // instructions per MFMA, MFMA busy 14.7 %): the row maximum is taken over the RAW scores (the scale is positive), so that
    // scale and shift are one fused multiply-add per score (packed: two scores per instruction); the exponentials are
    // summed pairwise and packed to bf16 as they are produced; the rescale of the 32 output accumulators is skipped when no
    // row's maximum moved (wave-uniform test); and the lane-dependent LDS offsets are computed once per kernel
    // (swz(kt + r, c) = kt * ROWB + swz(r, c) for kt a multiple of 16): ~60 VALU instructions per tile instead of ~130.
    int kt = 0;
    while (kt < npad) {
      if (a.causal && c0 + kt > q0 + 31) break;
      const bool edge = c0 + kt + 32 > kvalid || (a.causal && c0 + kt + 31 > q0);
      if (!edge && a.lean) {
        const char* kb = Kt + kt * ROWB;
        const char* vb = Vt + kt * ROWB;
        f32x16 s0;
#pragma unroll
        for (int r = 0; r < 16; ++r) s0[r] = 0.f;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc)
          s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(kb + koff[kc]), qf[kc], s0, 0, 0, 0);
        float mx = fmaxf(s0[0], s0[1]);
#pragma unroll
        for (int r = 2; r < 16; ++r) mx = fmaxf(mx, s0[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx * sc2);            // finite: an unmasked tile has 32 real scores per row
        const float alpha = __builtin_amdgcn_exp2f(m - mn);   // m = -inf (first step) -> 0
        const v2f sc2v = v2f{sc2, sc2}, nmv = v2f{-mn, -mn};
        v2f rs2 = v2f{0.f, 0.f};
        u32x4 pk[2];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const v2f e0 = v2f{s0[2 * j], s0[2 * j + 1]} * sc2v + nmv;
          const v2f x0 = v2f{__builtin_amdgcn_exp2f(e0[0]), __builtin_amdgcn_exp2f(e0[1])};
          rs2 += x0;
          pk[j >> 2][j & 3] = pack2bf(x0[0], x0[1]);
        }
        float rs = rs2[0] + rs2[1];
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs;
        m = mn;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
          const v2f av = v2f{alpha, alpha};
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const v2f a0 = v2f{o[0][2 * j], o[0][2 * j + 1]} * av, a1 = v2f{o[1][2 * j], o[1][2 * j + 1]} * av;
            o[0][2 * j] = a0[0]; o[0][2 * j + 1] = a0[1]; o[1][2 * j] = a1[0]; o[1][2 * j + 1] = a1[1];
          }
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr16_frag(vb, voff[dt][0], voff[dt][1]), __builtin_bit_cast(bf16x8_t, pk[0]), o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr16_frag(vb + 16 * ROWB, voff[dt][0], voff[dt][1]), __builtin_bit_cast(bf16x8_t, pk[1]), o[dt], 0, 0, 0);
        }
        kt += 32;
        continue;
      }
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int kc = 0; kc < 4; ++kc)
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Kt, kt, kc, lane), qf[kc], s, 0, 0, 0);
      // softmax in the log2 domain (one fma + v_exp_f32 per element); the key / causal masks are only evaluated on
      // tiles that contain masked elements (wave-uniform test)
      float p[16];
      float mx = -INFINITY;
      if (edge) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = c0 + kt + acc_row(r, lh);
          const bool ok = key < kvalid && (!a.causal || key <= qg);
          p[r] = ok ? s[r] * sc2 : -INFINITY;
          mx = fmaxf(mx, p[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[r] = s[r] * sc2; mx = fmaxf(mx, p[r]); }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m, mx);
      const float msafe = mn == -INFINITY ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f(m - msafe);  // m = -inf -> 0
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(p[r] - msafe); rs += p[r]; }
      rs += __shfl_xor(rs, 32, 64);
      l = l * alpha + rs;
      m = mn;
#pragma unroll
      for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
      const bf16x8_t pb0 = pack8(p), pb1 = pack8(p + 8);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Vt, kt, dt * 32, lane), pb0, o[dt], 0, 0, 0);
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Vt, kt + 16, dt * 32, lane), pb1, o[dt], 0, 0, 0);
      }
      kt += 32;
    }
  }
  // Output.  The accumulators hold transposed tiles (lane = query row, registers = 4 consecutive columns): stored from
  // registers every instruction touches 32 rows with 8 bytes each.  With a.staged the tile goes
  // through the wave's own 4 KB of the K tile instead (free once every wave has left the key loop): 8-byte LDS writes,
  // 16-byte reads of whole 128-byte rows, 16-byte coalesced global stores.
  if (a.staged) {
    __syncthreads();
    if (!wave_active) return;
    const float inv = l > 0.f ? 1.f / l : 0.f;
    char* ot = Kt + wave * 32 * ROWB;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        u32x2 t;
        t[0] = pack2bf(o[dt][rg * 4 + 0] * inv, o[dt][rg * 4 + 1] * inv);
        t[1] = pack2bf(o[dt][rg * 4 + 2] * inv, o[dt][rg * 4 + 3] * inv);
        *reinterpret_cast<u32x2*>(ot + swz(li, tileimg::park_col(dt, rg, lh))) = t;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    bf16_t* Ob = a.O + (int64_t)b * a.o_sb + (int64_t)h * a.hd;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * 64 + lane, r = idx >> 3, c = idx & 7;
      const u32x4 v = *reinterpret_cast<const u32x4*>(ot + swz(r, c * 8));
      if (q0 + r < a.Tq && c * 8 < a.hd) *reinterpret_cast<u32x4*>(Ob + (int64_t)(q0 + r) * a.o_st + c * 8) = v;
    }
    if (lh == 0 && qg < a.Tq) a.lse[((int64_t)b * a.H + h) * a.Tq + qg] = (l > 0.f) ? m * 0.6931471805599453f + __logf(l) : -INFINITY;
    return;
  }
  if (!wave_active || qg >= a.Tq) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  bf16_t* Op = a.O + (int64_t)b * a.o_sb + (int64_t)qg * a.o_st + (int64_t)h * a.hd;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int d = tileimg::park_col(dt, rg, lh);
      if (d < a.hd) {
        u32x2 t;
        t[0] = pack2bf(o[dt][rg * 4 + 0] * inv, o[dt][rg * 4 + 1] * inv);
        t[1] = pack2bf(o[dt][rg * 4 + 2] * inv, o[dt][rg * 4 + 3] * inv);
        *reinterpret_cast<u32x2*>(Op + d) = t;
      }
    }
  if (lh == 0) a.lse[((int64_t)b * a.H + h) * a.Tq + qg] = (l > 0.f) ? m * 0.6931471805599453f + __logf(l) : -INFINITY;
}

struct BwdArgs {
  const bf16_t* Q; const bf16_t* K; const bf16_t* V; const bf16_t* O; const bf16_t* dO; const float* lse;
  bf16_t* dQ; bf16_t* dK; bf16_t* dV;
  int H, Tq, Tk, hd;
  int64_t q_sb, q_st, k_sb, k_st, v_sb, v_st, o_sb, o_st, do_sb, do_st;
  int64_t dq_sb, dq_st, dk_sb, dk_st, dv_sb, dv_st;
  float scale; int causal;
  const int* klen;     // nullable: valid keys per sample (fused kernel only)
  float* colsum_part;  // nullable: [B][3][H*hd] token sums of dQ | dK | dV (the in_proj bias gradient, per sample)
  int nitems;          // single-pass kernel: B * H items, walked by a persistent grid
  float* ws;           // attention_dqw.inc, sequences of more than 224 tokens: fp32 dQ accumulators across key chunks
};

constexpr int TMAX = 256;
// LDS bytes of the backward kernel for tiles of tp (padded) rows: two tiles (Q,dO for the dK/dV pass, then K,V for
// the dQ pass in the same space) + lse, D, cs vectors + the cross-wave reduce pad
static inline size_t bwd_lds_bytes(int tp) { return (size_t)tp * (2 * ROWB + 3 * 4) + 8 * 3 * 64 * 4; }

#include "attention_smallq.inc"

// MFMA operand fragment straight from global memory (rows that only ONE wave needs): lane l -> row row0 + (l&31),
// cols kc*16 + 8*(l>>5) .. +7; zero beyond nvalid / hd.  Unconditional load from a clamped address + select.
__device__ __forceinline__ bf16x8_t frag_rows_g(const bf16_t* __restrict__ X, int64_t st, int row0, int nvalid, int kc,
                                                int lane, int hd) {
  const int r = row0 + (lane & 31), c = kc * 16 + 8 * (lane >> 5);
  const int rc = r < nvalid ? r : nvalid - 1, cc = c < hd ? c : 0;
  u32x4 v = *reinterpret_cast<const u32x4*>(X + (int64_t)rc * st + cc);
  if (!(r < nvalid && c < hd)) v = u32x4{0u, 0u, 0u, 0u};
  return __builtin_bit_cast(bf16x8_t, v);
}

__device__ __forceinline__ void store_acc_T(bf16_t* base, int64_t st, int row, int nrows, int hd, const f32x16 (&acc)[2],
                                            int lh) {
  if (row >= nrows) return;
  bf16_t* p = base + (int64_t)row * st;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int d = tileimg::park_col(dt, rg, lh);
      if (d < hd) {
        u32x2 t;
        t[0] = pack2bf(acc[dt][rg * 4 + 0], acc[dt][rg * 4 + 1]);
        t[1] = pack2bf(acc[dt][rg * 4 + 2], acc[dt][rg * 4 + 3]);
        *reinterpret_cast<u32x2*>(p + d) = t;
      }
    }
}

__global__ __launch_bounds__(512) void attn_bwd_bf16_kernel(BwdArgs a) {
  // Dynamic LDS sized by the padded sequence length, and only TWO tiles: Q and dO (read by every wave in the dK/dV
  // pass), later overwritten by K and V (read by every wave in the dQ pass).  The rows only one wave needs (its own
  // key tile of K,V / query tile of Q,dO) come straight from global memory.  197 tokens -> 66 KB, 77 -> 31 KB, so
  // two (vision) or more (text) workgroups share a CU and one's load/store phases overlap the other's MFMAs.
  extern __shared__ __attribute__((aligned(16))) char smem_bwd[];
  const int tp0 = (((a.Tq > a.Tk ? a.Tq : a.Tk) + 31) & ~31);
  char* T0 = smem_bwd;               // Q, then K
  char* T1 = smem_bwd + tp0 * ROWB;  // dO, then V
  char* Qt = T0;
  char* Gt = T1;
  char* Kt = T0;
  char* Vt = T1;
  float* Ls = reinterpret_cast<float*>(smem_bwd + 2 * tp0 * ROWB);
  float* Ds = Ls + tp0;
  float* Cs = Ds + tp0;   // cs[key] = sum_q dS[q][key]
  float* Red = Cs + tp0;  // [8 waves][3][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int li = lane & 31, lh = lane >> 5;
  const int64_t hoff = (int64_t)h * a.hd;
  const bf16_t* Qp = a.Q + b * a.q_sb + hoff;
  const bf16_t* Kp = a.K + b * a.k_sb + hoff;
  const bf16_t* Vp = a.V + b * a.v_sb + hoff;
  const bf16_t* Op = a.O + b * a.o_sb + hoff;
  const bf16_t* Gp = a.dO + b * a.do_sb + hoff;
  const int tqp = (a.Tq + 31) & ~31, tkp = (a.Tk + 31) & ~31;
  const int kvalid = a.klen ? (a.klen[b] < a.Tk ? a.klen[b] : a.Tk) : a.Tk;

  stage_rows(Qt, Qp, a.q_st, 0, a.Tq, tqp, a.hd, tid, blockDim.x);
  // dO tile + D[q] = sum_d dO*O (8 consecutive lanes share a row); branch-free batched loads as in stage_rows
  {
    const int total = tqp * 8;
    for (int base = 0; base < total; base += 2 * (int)blockDim.x) {
      u32x4 gv[2], ov[2];
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int idx = base + it * (int)blockDim.x + tid;
        const int r = idx >> 3, c = idx & 7;
        const int rc = r < a.Tq ? r : a.Tq - 1;
        const int cc = c * 8 < a.hd ? c : 0;
        gv[it] = *reinterpret_cast<const u32x4*>(Gp + (int64_t)rc * a.do_st + cc * 8);
        ov[it] = *reinterpret_cast<const u32x4*>(Op + (int64_t)rc * a.o_st + cc * 8);
      }
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int idx = base + it * (int)blockDim.x + tid;
        const int r = idx >> 3, c = idx & 7;
        const bool ok = r < a.Tq && c * 8 < a.hd;
        const u32x4 g = ok ? gv[it] : u32x4{0u, 0u, 0u, 0u};
        const u32x4 o4 = ok ? ov[it] : u32x4{0u, 0u, 0u, 0u};
        float sdot = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sdot += __uint_as_float(g[j] << 16) * __uint_as_float(o4[j] << 16);
          sdot += __uint_as_float(g[j] & 0xffff0000u) * __uint_as_float(o4[j] & 0xffff0000u);
        }
        sdot += __shfl_xor(sdot, 1, 64); sdot += __shfl_xor(sdot, 2, 64); sdot += __shfl_xor(sdot, 4, 64);
        if (idx < total) {
          *reinterpret_cast<u32x4*>(Gt + swz(r, c * 8)) = g;
          if (c == 0) {
            Ds[r] = sdot;
            Ls[r] = r < a.Tq ? a.lse[((int64_t)b * a.H + h) * a.Tq + r] * 1.4426950408889634f : 0.f;  // log2 domain
          }
        }
      }
    }
  }
  __syncthreads();
  const float sc2 = a.scale * 1.4426950408889634f;

  // ---------------- pass A: this wave owns key tiles; dK, dV ----------------
  for (int k0 = wave * 32; k0 < tkp; k0 += nw * 32) {
    bf16x8_t kf[4], vf[4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      kf[kc] = frag_rows_g(Kp, a.k_st, k0, a.Tk, kc, lane, a.hd);
      vf[kc] = frag_rows_g(Vp, a.v_st, k0, a.Tk, kc, lane, a.hd);
    }
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }
    const int key = k0 + li;
    float csl = 0.f;
    for (int q0 = 0; q0 < tqp; q0 += 32) {
      if (a.causal && q0 + 31 < k0) continue;
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Qt, q0, kc, lane), kf[kc], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Gt, q0, kc, lane), vf[kc], dp, 0, 0, 0);
      }
      // P = exp2(S * scale*log2e - lse*log2e): one fma + v_exp_f32; dS is kept WITHOUT the softmax scale (applied once
      // to dK, the column sums and dQ at the end); masks only on tiles that contain masked elements (wave-uniform)
      const bool edge = k0 + 32 > kvalid || q0 + 32 > a.Tq || (a.causal && k0 + 31 > q0);
      float p[16], ds[16];
      if (edge) {
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int qb = q0 + 8 * rg + 4 * lh;  // 4 consecutive query rows per register group
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + qb);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(Ds + qb);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = rg * 4 + j, q = qb + j;
            const bool ok = key < kvalid && q < a.Tq && (!a.causal || key <= q);
            const float pv = ok ? __builtin_amdgcn_exp2f(s[r] * sc2 - l4[j]) : 0.f;
            p[r] = pv;
            ds[r] = pv * (dp[r] - d4[j]);
            csl += ds[r];
          }
        }
      } else {
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int qb = q0 + 8 * rg + 4 * lh;
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + qb);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(Ds + qb);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = rg * 4 + j;
            const float pv = __builtin_amdgcn_exp2f(s[r] * sc2 - l4[j]);
            p[r] = pv;
            ds[r] = pv * (dp[r] - d4[j]);
            csl += ds[r];
          }
        }
      }
      const bf16x8_t pb0 = pack8(p), pb1 = pack8(p + 8), sb0 = pack8(ds), sb1 = pack8(ds + 8);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Gt, q0, dt * 32, lane), pb0, dv[dt], 0, 0, 0);
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Gt, q0 + 16, dt * 32, lane), pb1, dv[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qt, q0, dt * 32, lane), sb0, dk[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qt, q0 + 16, dt * 32, lane), sb1, dk[dt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[0][r] *= a.scale; dk[1][r] *= a.scale; }
    store_acc_T(a.dK + b * a.dk_sb + hoff, a.dk_st, key, a.Tk, a.hd, dk, lh);
    store_acc_T(a.dV + b * a.dv_sb + hoff, a.dv_st, key, a.Tk, a.hd, dv, lh);
    csl += __shfl_xor(csl, 32, 64);
    if (lh == 0) Cs[key] = csl * a.scale;
  }

  // token sums of dV (= token sums of dO: the rows of P sum to one) while dO is still in LDS
  float accv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) accv[j] = 0.f;
  if (a.colsum_part) {
    const int c = tid & 7, nrl = (int)blockDim.x >> 3;
    for (int r = tid >> 3; r < tqp; r += nrl) {
      const u32x4 gv = *reinterpret_cast<const u32x4*>(Gt + swz(r, c * 8));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        accv[2 * j] += __uint_as_float(gv[j] << 16);
        accv[2 * j + 1] += __uint_as_float(gv[j] & 0xffff0000u);
      }
    }
  }
  __syncthreads();  // every wave is done with Q and dO: the two tiles become K and V
  stage_rows(Kt, Kp, a.k_st, 0, a.Tk, tkp, a.hd, tid, blockDim.x);
  stage_rows(Vt, Vp, a.v_st, 0, a.Tk, tkp, a.hd, tid, blockDim.x);
  __syncthreads();

  // ---------------- pass B: this wave owns query tiles; dQ ----------------
  for (int q0 = wave * 32; q0 < tqp; q0 += nw * 32) {
    bf16x8_t qf[4], gf[4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      qf[kc] = frag_rows_g(Qp, a.q_st, q0, a.Tq, kc, lane, a.hd);
      gf[kc] = frag_rows_g(Gp, a.do_st, q0, a.Tq, kc, lane, a.hd);
    }
    const int q = q0 + li;
    const float lq = Ls[q], dq_ = Ds[q];
    f32x16 dq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
    for (int k0 = 0; k0 < tkp; k0 += 32) {
      if (a.causal && k0 > q0 + 31) break;
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Kt, k0, kc, lane), qf[kc], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Vt, k0, kc, lane), gf[kc], dp, 0, 0, 0);
      }
      const bool edge = k0 + 32 > kvalid || q0 + 32 > a.Tq || (a.causal && k0 + 31 > q0);
      float ds[16];
      if (edge) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = k0 + acc_row(r, lh);
          const bool ok = key < kvalid && q < a.Tq && (!a.causal || key <= q);
          ds[r] = ok ? __builtin_amdgcn_exp2f(s[r] * sc2 - lq) * (dp[r] - dq_) : 0.f;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(s[r] * sc2 - lq) * (dp[r] - dq_);
      }
      const bf16x8_t sb0 = pack8(ds), sb1 = pack8(ds + 8);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Kt, k0, dt * 32, lane), sb0, dq[dt], 0, 0, 0);
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Kt, k0 + 16, dt * 32, lane), sb1, dq[dt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[0][r] *= a.scale; dq[1][r] *= a.scale; }
    store_acc_T(a.dQ + b * a.dq_sb + hoff, a.dq_st, q, a.Tq, a.hd, dq, lh);
  }

  // ---------------- token sums of dQ, dK, dV (in_proj bias gradient of this sample and head) ----------------
  //   sum_q dQ[q][d]   = sum_key K[key][d] cs[key]   (K is in LDS now, cs from the dK/dV pass)
  //   sum_key dV[key][d] = sum_q dO[q][d]            (accumulated above)
  //   sum_key dK[key][d] = sum_q Q[q][d] rowsum_key(dS[q][:]) = 0 exactly: the rows of dS sum to zero (softmax is
  //                        shift invariant; what the reference accumulates there is rounding noise ~1e-8)
  if (a.colsum_part) {
    const int c = tid & 7, nrl = (int)blockDim.x >> 3;
    float accq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) accq[j] = 0.f;
    for (int r = tid >> 3; r < tkp; r += nrl) {
      const u32x4 kv = *reinterpret_cast<const u32x4*>(Kt + swz(r, c * 8));
      const float w = Cs[r];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        accq[2 * j] += w * __uint_as_float(kv[j] << 16);
        accq[2 * j + 1] += w * __uint_as_float(kv[j] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float vq = accq[j], vv = accv[j];
      vq += __shfl_xor(vq, 8, 64); vv += __shfl_xor(vv, 8, 64);
      vq += __shfl_xor(vq, 16, 64); vv += __shfl_xor(vv, 16, 64);
      vq += __shfl_xor(vq, 32, 64); vv += __shfl_xor(vv, 32, 64);
      if (lane < 8) {
        Red[(wave * 3 + 0) * 64 + c * 8 + j] = vq;
        Red[(wave * 3 + 2) * 64 + c * 8 + j] = vv;
      }
    }
    __syncthreads();
    for (int t = tid; t < 192; t += (int)blockDim.x) {
      const int m = t >> 6, dd = t & 63;
      float v = 0.f;
      if (m != 1)
        for (int w = 0; w < nw; ++w) v += Red[(w * 3 + m) * 64 + dd];
      if (dd < a.hd) a.colsum_part[((int64_t)b * 3 + m) * ((int64_t)a.H * a.hd) + hoff + dd] = v;
    }
  }
}

#include "attention_sp.inc"
#include "attention_pf.inc"
#include "attention_spl.inc"
#include "attention_dqw.inc"
#include "attention_stream.inc"

// ------------------------------- f32 path helpers -------------------------------------------
// in-place row softmax of S (rows = B*H*Tq, Tk cols), causal mask by query index row % Tq
__global__ void softmax_rows_kernel(float* __restrict__ S, int64_t rows, int Tq, int Tk, int causal, const int* klen,
                                    int H) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int q = (int)(row % Tq);
  float* s = S + row * Tk;
  int lim = causal ? (q + 1 < Tk ? q + 1 : Tk) : Tk;
  if (klen) { const int kv = klen[row / ((int64_t)H * Tq)]; lim = kv < lim ? kv : lim; }
  float mx = -INFINITY;
  for (int c = lane; c < lim; c += 64) mx = fmaxf(mx, s[c]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int c = lane; c < lim; c += 64) sum += expf(s[c] - mx);
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  for (int c = lane; c < Tk; c += 64) s[c] = c < lim ? expf(s[c] - mx) * inv : 0.f;
}
// dS = P * (dP - sum_k dP*P) * scale, in place on dP
__global__ void softmax_bwd_rows_kernel(const float* __restrict__ P, float* __restrict__ dP, int64_t rows, int Tk,
                                        float scale) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = P + row * Tk;
  float* d = dP + row * Tk;
  float dot = 0.f;
  for (int c = lane; c < Tk; c += 64) dot += p[c] * d[c];
  dot = wave_sum(dot);
  for (int c = lane; c < Tk; c += 64) d[c] = p[c] * (d[c] - dot) * scale;
}

// ------------------------------- host side -------------------------------------------
// segclip_attn_fwd / segclip_attn_bwd: validate, fill the kernel arguments, plan (which kernel), launch, note the route.

bool bf16_ok(const segclip_attn_desc* d) {
  const int64_t s[] = {d->q_sb, d->q_st, d->k_sb, d->k_st, d->v_sb, d->v_st, d->o_sb, d->o_st};
  for (int64_t v : s) if (v % 8) return false;
  return d->hd % 8 == 0 && d->hd <= 64;
}

// ---- the planner: pure functions of the descriptor, no HIP call ----
struct Plan {
  int route, tiles, variant;   // what segclip_attn_route_note records after the launch
  int waves;                   // per workgroup, a loader / dQ wave included (0: the streaming pair sizes its own)
  size_t lds;                  // dynamic LDS bytes
  int staged;                  // forward: FwdArgs::staged
};
int tiles_of(const segclip_attn_desc* d) { return (int)cdiv(d->Tq > d->Tk ? d->Tq : d->Tk, 32); }
bool long_seq(const segclip_attn_desc* d) { return d->Tq > TMAX || d->Tk > TMAX; }

Plan plan_fwd(const segclip_attn_desc* d) {
  if (d->dtype != SEGCLIP_BF16) return {SEGCLIP_ATTN_ROUTE_F32, tiles_of(d)};
  // LDS-staged output rows: 117 -> 112 us at T = 196 (B = 256, H = 12), 27.8 -> 29.3 us at T = 77: on for the long sequences
  const int staged = d->Tq > 128 ? 1 : 0;
  // at most 8 queries (the learnable-center cross-attention): one wave per (batch, head), VALU
  if (smallq::covers(d)) return {SEGCLIP_ATTN_ROUTE_SMALLQ, 1, 0, smallq::WPB_FWD, smallq::lds_bytes((int)d->Tk, false), staged};
  const int tiles = (int)cdiv(d->Tq, 32);
  const size_t pf_lds = fwd_pf_lds_bytes(tiles, (int)d->Tq);
  // self-attention of 65..96 / 161..200 tokens: the persistent kernel with a loader wave (attention_pf.inc)
  if (d->Tq == d->Tk && !(d->flags & SEGCLIP_ATTN_FP8) && (tiles == 3 || tiles == 6 || tiles == 7) && pf_lds <= 160 * 1024)
    return {SEGCLIP_ATTN_ROUTE_PF, tiles, d->causal ? 1 : 0, tiles + 1, pf_lds, staged};
  // one wave per query tile, at most 8 per workgroup, spread evenly over the workgroups of a (batch, head)
  const int nw = tiles < 8 ? tiles : (tiles <= 8 ? 8 : (int)cdiv(tiles, cdiv(tiles, 8)));
  return {SEGCLIP_ATTN_ROUTE_GENERIC, tiles, (staged ? 1 : 0) | nw << 8, nw, 0, staged};
}

Plan plan_bwd(const segclip_attn_desc* d) {
  const int tiles = tiles_of(d);
  if (d->dtype != SEGCLIP_BF16) return {SEGCLIP_ATTN_ROUTE_F32, tiles};
  if (smallq::covers(d)) return {SEGCLIP_ATTN_ROUTE_SMALLQ, 1, 0, smallq::WPB_BWD, smallq::lds_bytes((int)d->Tk, true)};
  if (long_seq(d)) {
    // unmasked self-attention, head_dim 64: the dQ-wave kernel over chunks of 224 keys (attention_dqw.inc, MULTI)
    // (its token sums ride on a padded key in the last chunk and on two padded rows of the last query tile)
    if (d->Tq == d->Tk && !d->causal && d->hd == 64 && d->Tq % 32 <= 30 && d->Tq % 224 != 0)
      return {SEGCLIP_ATTN_ROUTE_DQW, 7, 1, 8, bwd_dqw_lds_bytes<7>()};
    return {SEGCLIP_ATTN_ROUTE_STREAM, tiles, 0, 0, bwd_stream_lds_bytes()};   // two streaming launches (dK,dV | dQ)
  }
  const bool masked = d->causal || d->klen;
  // self-attention: the single-pass kernels, one wave per key tile; cross-attention (Tq != Tk) takes the two-pass kernel
  if (d->Tq == d->Tk) {
    // vision tower (no mask, head_dim 64, 7 tiles, padded rows in the last tile): the query tiles as a stream with a dQ wave
    // (attention_dqw.inc, round 6)
    if (!masked && d->hd == 64 && tiles == 7 && d->Tq % 32 >= 1 && d->Tq % 32 <= 30)
      return {SEGCLIP_ATTN_ROUTE_DQW, 7, 0, 8, bwd_dqw_lds_bytes<7>()};
    // vision tower (no mask, 5-7 tiles): the variant whose memory traffic is issued by a loader wave (attention_spl.inc);
    // head_dim 64 only: its loader wave copies whole 128-byte rows of Q, so with a smaller head the columns beyond it (the next
    // head, or whatever follows the last one) would enter S = K Q^T against zeroed K columns: 0 x NaN, and a read past the
    // end of a separately allocated Q.  Smaller heads take attention_sp.inc, which selects by column.
    const size_t spl_lds = bwd_spl_lds_bytes((int)d->Tq);
    if (!masked && d->hd == 64 && tiles >= 5 && tiles <= 7 && spl_lds <= 160 * 1024)
      return {SEGCLIP_ATTN_ROUTE_SPL, tiles, 0, tiles + 1, spl_lds};
    return {SEGCLIP_ATTN_ROUTE_SP, tiles, masked ? 1 : 0, tiles, bwd_sp_lds_bytes(tiles * 32)};   // variant: instance <MASKED>
  }
  // 4 waves per workgroup (each wave walks over 1-2 tiles): two such workgroups fit the registers (2 waves per SIMD
  // at ~215 VGPRs) and the LDS of a CU, so their load / MFMA / store phases interleave
  const int nw = tiles < 4 ? tiles : 4;
  return {SEGCLIP_ATTN_ROUTE_TWOPASS, tiles, nw << 8, nw, bwd_lds_bytes(tiles * 32)};
}

// ---- per-device state (function attributes and the CU count belong to the device a launch goes to), in atomics: two host
// threads may enter at once (config.scope() is per thread); both fill an empty entry alike ----
constexpr int MAX_DEVICES = 64;
struct Device { int index, ncu; };
std::atomic<int> device_ncu[MAX_DEVICES];
std::atomic<int> pf_per_cu[MAX_DEVICES][2][8][33];   // attention_pf.inc: workgroups per CU by (causal, tiles, key tile rows / 8)

// the current device and its CU count (256 where the runtime does not tell), for the workspace query and every launcher
// alike, so that the grid of a launch and the workspace sized for it agree
bool current_device(Device& dv) {
  if (hipGetDevice(&dv.index) != hipSuccess || dv.index < 0 || dv.index >= MAX_DEVICES) return false;
  if ((dv.ncu = device_ncu[dv.index]) == 0) {
    if (hipDeviceGetAttribute(&dv.ncu, hipDeviceAttributeMultiprocessorCount, dv.index) != hipSuccess || dv.ncu <= 0) dv.ncu = 256;
    device_ncu[dv.index] = dv.ncu;
  }
  return true;
}

// raises the dynamic-LDS limit of KERNEL once per (kernel, device): 0, or the refusal of `who` (attn_fwd / attn_bwd)
template <auto KERNEL>
int raise_lds_limit(const char* who, const Device& dv, size_t bytes) {
  static std::atomic<bool> done[MAX_DEVICES];
  if (done[dv.index]) return 0;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  SEGCLIP_REQUIRE(e == hipSuccess, "%s bf16: cannot raise the dynamic LDS limit: %s", who, hipGetErrorString(e));
  done[dv.index] = true;
  return 0;
}

// KERNEL on `grid` workgroups of `waves` waves with the planned dynamic LDS
template <auto KERNEL, typename... Args>
int launch(const char* name, dim3 grid, int waves, const Plan& p, hipStream_t stream, const Args&... args) {
  hipLaunchKernelGGL(KERNEL, grid, dim3(waves * 64), p.lds, stream, args...);
  SEGCLIP_CHECK_LAUNCH(name);
  return 0;
}

// ---- forward launchers (smallq: launch<>) ----
// persistent forward (attention_pf.inc), instance <NT, CAUSAL>: as many workgroups as the device holds
template <int NT, bool CAUSAL>
int launch_fwd_pf_as(const FwdArgs& a, const Plan& p, int nitems, hipStream_t stream) {
  Device dv;
  SEGCLIP_REQUIRE(current_device(dv), "attn_fwd: cannot query the current device");
  if (int rc = raise_lds_limit<attn_fwd_pf_kernel<NT, CAUSAL>>("attn_fwd", dv, 160 * 1024)) return rc;
  std::atomic<int>& cached = pf_per_cu[dv.index][CAUSAL][NT][pf_kv_rows(a.Tq) >> 3];
  int per_cu = cached;
  if (per_cu == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, attn_fwd_pf_kernel<NT, CAUSAL>, p.waves * 64, p.lds) != hipSuccess || per_cu < 1) per_cu = 1;
    cached = per_cu;
  }
  return launch<attn_fwd_pf_kernel<NT, CAUSAL>>("attn_fwd_pf", dim3(std::min(nitems, dv.ncu * per_cu)), p.waves, p, stream, a, nitems);
}
int launch_fwd_pf(const FwdArgs& a, const Plan& p, int nitems, hipStream_t stream) {
  switch (p.tiles * 2 + p.variant) {   // variant: causal.  plan_fwd picks 3, 6 or 7 tiles
    case 3 * 2: return launch_fwd_pf_as<3, false>(a, p, nitems, stream);
    case 3 * 2 + 1: return launch_fwd_pf_as<3, true>(a, p, nitems, stream);
    case 6 * 2: return launch_fwd_pf_as<6, false>(a, p, nitems, stream);
    case 6 * 2 + 1: return launch_fwd_pf_as<6, true>(a, p, nitems, stream);
    case 7 * 2: return launch_fwd_pf_as<7, false>(a, p, nitems, stream);
    default: return launch_fwd_pf_as<7, true>(a, p, nitems, stream);
  }
}

int launch_fwd_generic(const segclip_attn_desc* d, const FwdArgs& a, const Plan& p, hipStream_t stream) {
  SEGCLIP_REQUIRE(d->B * d->H <= 65535, "attn_fwd: B*H too large");
  if (d->flags & SEGCLIP_ATTN_FP8) {
    segclip_set_error("attn_fwd: the e4m3 forward was removed (slower than bf16 at head_dim 64, DESIGN.md section 8): "
                      "configs[4] runs bf16 attention");
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  return launch<attn_fwd_bf16_kernel>("attn_fwd_bf16", dim3((unsigned)cdiv(p.tiles, p.waves), (unsigned)(d->B * d->H)), p.waves, p, stream, a);
}

// f32 path: one batched GEMM C(m,n) = alpha * sum_k A(m,k) B(n,k) over the B * H (sample, head) pairs.  An operand is
// {pointer, stride of its first index, stride of k (for C: 1), stride per sample, stride per head}
struct Mat { const void* p; int64_t s0, sk, sb, sh; };
int gemm_f32(const segclip_attn_desc* d, hipStream_t stream, int64_t M, int64_t N, int64_t K, Mat A, Mat B, Mat C, float alpha = 1.f) {
  segclip_gemm_desc g{};
  g.nb1 = d->B; g.nb2 = d->H;
  g.a_dtype = g.b_dtype = g.c_dtype = g.r_dtype = SEGCLIP_F32;
  g.alpha = alpha;
  g.A = A.p; g.B = B.p; g.C = const_cast<void*>(C.p); g.M = M; g.N = N; g.K = K;
  g.sam = A.s0; g.sak = A.sk; g.sbn = B.s0; g.sbk = B.sk; g.ldc = C.s0;
  g.bsA1 = A.sb; g.bsA2 = A.sh; g.bsB1 = B.sb; g.bsB2 = B.sh; g.bsC1 = C.sb; g.bsC2 = C.sh;
  return segclip_gemm_f32_launch(&g, stream);
}
Mat scores(const segclip_attn_desc* d, const void* p, bool transposed) {   // P, dP: [B][H][Tq][Tk], as (q, key) or as (key, q)
  return transposed ? Mat{p, 1, d->Tk, d->H * d->Tq * d->Tk, d->Tq * d->Tk} : Mat{p, d->Tk, 1, d->H * d->Tq * d->Tk, d->Tq * d->Tk};
}

// f32: S -> stats, softmax in place, O = P V
int launch_fwd_f32(const segclip_attn_desc* d, hipStream_t stream) {
  float* P = (float*)d->stats;
  if (int rc = gemm_f32(d, stream, d->Tq, d->Tk, d->hd, {d->Q, d->q_st, 1, d->q_sb, d->hd}, {d->K, d->k_st, 1, d->k_sb, d->hd}, scores(d, P, false), d->scale)) return rc;
  const int64_t rows = d->B * d->H * d->Tq;
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, stream, P, rows, (int)d->Tq,
                     (int)d->Tk, d->causal, (const int*)d->klen, (int)d->H);
  SEGCLIP_CHECK_LAUNCH("attn_softmax_rows");
  return gemm_f32(d, stream, d->Tq, d->hd, d->Tk, scores(d, P, false), {d->V, 1, d->v_st, d->v_sb, d->hd}, {d->O, d->o_st, 1, d->o_sb, d->hd});
}

// ---- backward launchers (smallq: launch<>) ----
// streaming backward with a dQ wave (attention_dqw.inc): one workgroup of 7 + 1 waves per CU walks its share of the items
template <bool MULTI>
int launch_bwd_dqw(const BwdArgs& a, const Plan& p, const Device& dv, hipStream_t stream) {
  if (int rc = raise_lds_limit<attn_bwd_dqw_bf16_kernel<7, MULTI>>("attn_bwd", dv, 160 * 1024)) return rc;
  return launch<attn_bwd_dqw_bf16_kernel<7, MULTI>>("attn_bwd_dqw_bf16", dim3(std::min(a.nitems, dv.ncu)), p.waves, p, stream, a);
}

// long sequences: two streaming launches (dK,dV | dQ), 8 owned tiles per workgroup
int launch_bwd_stream(const segclip_attn_desc* d, const BwdArgs& a, const Plan& p, const Device& dv, hipStream_t stream) {
  if (raise_lds_limit<attn_bwd_dkv_stream_kernel>("attn_bwd", dv, p.lds) || raise_lds_limit<attn_bwd_dq_stream_kernel>("attn_bwd", dv, p.lds))
    SEGCLIP_REQUIRE(false, "attn_bwd bf16: cannot raise the dynamic LDS limit");   // names no cause
  const int ktiles = (int)cdiv(d->Tk, 32), qtiles = (int)cdiv(d->Tq, 32);
  const int nwk = ktiles < 8 ? ktiles : 8, nwq = qtiles < 8 ? qtiles : 8;
  if (int rc = launch<attn_bwd_dkv_stream_kernel>("attn_bwd_dkv_stream", dim3(a.nitems, (unsigned)cdiv(ktiles, nwk)), nwk, p, stream, a, a.ws)) return rc;
  return launch<attn_bwd_dq_stream_kernel>("attn_bwd_dq_stream", dim3(a.nitems, (unsigned)cdiv(qtiles, nwq)), nwq, p, stream, a, (const float*)a.ws);
}

// persistent grid of the single-pass kernels: as many workgroups as the chip holds at once (LDS / registers: 1 per CU at
// T = 197, more for the short text sequences)
dim3 bwd_persistent_grid(int nitems, const Device& dv, int per_cu) {
  return dim3((unsigned)std::min<int64_t>(nitems, (int64_t)dv.ncu * per_cu));
}
// with a loader wave (attention_spl.inc): one workgroup per CU
int launch_bwd_spl(const BwdArgs& a, const Plan& p, const Device& dv, hipStream_t stream) {
  if (int rc = raise_lds_limit<attn_bwd_spl_bf16_kernel>("attn_bwd", dv, 160 * 1024)) return rc;
  return launch<attn_bwd_spl_bf16_kernel>("attn_bwd_spl_bf16", bwd_persistent_grid(a.nitems, dv, 1), p.waves, p, stream, a);
}
// attention_sp.inc, instance <MASKED>: as many workgroups per CU as the occupancy query allows
template <bool MASKED>
int launch_bwd_sp(const BwdArgs& a, const Plan& p, const Device& dv, hipStream_t stream) {
  if (int rc = raise_lds_limit<attn_bwd_sp_bf16_kernel<MASKED>>("attn_bwd", dv, bwd_sp_lds_bytes(TMAX))) return rc;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, attn_bwd_sp_bf16_kernel<MASKED>, p.waves * 64, p.lds) != hipSuccess || per_cu < 1) per_cu = 1;
  return launch<attn_bwd_sp_bf16_kernel<MASKED>>("attn_bwd_sp_bf16", bwd_persistent_grid(a.nitems, dv, per_cu), p.waves, p, stream, a);
}

// two-pass kernel (cross-attention): one workgroup per (batch, head)
int launch_bwd_twopass(const BwdArgs& a, const Plan& p, const Device& dv, hipStream_t stream) {
  if (int rc = raise_lds_limit<attn_bwd_bf16_kernel>("attn_bwd", dv, bwd_lds_bytes(TMAX))) return rc;
  return launch<attn_bwd_bf16_kernel>("attn_bwd_bf16", dim3(a.nitems), p.waves, p, stream, a);
}

int launch_bwd_f32(const segclip_attn_desc* d, hipStream_t stream) {
  SEGCLIP_REQUIRE(d->colsum_part == nullptr, "attn_bwd f32: colsum_part is a bf16-path feature");
  SEGCLIP_REQUIRE(d->ws != nullptr, "attn_bwd f32: workspace required");
  const float* P = (const float*)d->stats;
  float* dP = (float*)d->ws;
  const Mat dO = {d->dO, d->do_st, 1, d->do_sb, d->hd}, dO_T = {d->dO, 1, d->do_st, d->do_sb, d->hd};
  int rc;
  // dV(key,d) = sum_q P[q][key] dO[q][d]
  if ((rc = gemm_f32(d, stream, d->Tk, d->hd, d->Tq, scores(d, P, true), dO_T, {d->dV, d->dv_st, 1, d->dv_sb, d->hd}))) return rc;
  // dP[q][key] = sum_d dO[q][d] V[key][d]
  if ((rc = gemm_f32(d, stream, d->Tq, d->Tk, d->hd, dO, {d->V, d->v_st, 1, d->v_sb, d->hd}, scores(d, dP, false)))) return rc;
  const int64_t rows = d->B * d->H * d->Tq;
  hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, stream, P, dP, rows, (int)d->Tk, d->scale);
  SEGCLIP_CHECK_LAUNCH("attn_softmax_bwd_rows");
  // dQ[q][d] = sum_key dS[q][key] K[key][d]
  if ((rc = gemm_f32(d, stream, d->Tq, d->hd, d->Tk, scores(d, dP, false), {d->K, 1, d->k_st, d->k_sb, d->hd}, {d->dQ, d->dq_st, 1, d->dq_sb, d->hd}))) return rc;
  // dK[key][d] = sum_q dS[q][key] Q[q][d]
  return gemm_f32(d, stream, d->Tk, d->hd, d->Tq, scores(d, dP, true), {d->Q, 1, d->q_st, d->q_sb, d->hd}, {d->dK, d->dk_st, 1, d->dk_sb, d->hd});
}

// what the bf16 forward and backward kernels read alike
template <typename Args>
void fill_common(Args& a, const segclip_attn_desc* d) {
  a.Q = (const bf16_t*)d->Q; a.K = (const bf16_t*)d->K; a.V = (const bf16_t*)d->V;
  a.H = (int)d->H; a.Tq = (int)d->Tq; a.Tk = (int)d->Tk; a.hd = (int)d->hd;
  a.q_sb = d->q_sb; a.q_st = d->q_st; a.k_sb = d->k_sb; a.k_st = d->k_st; a.v_sb = d->v_sb; a.v_st = d->v_st;
  a.o_sb = d->o_sb; a.o_st = d->o_st; a.scale = d->scale; a.causal = d->causal;
  a.klen = (const int*)d->klen;
}

}  // namespace

// the per-device state above for the other translation units (common.h)
bool segclip_current_device(int* index, int* ncu) {
  Device dv;
  if (!current_device(dv)) return false;
  *index = dv.index; *ncu = dv.ncu;
  return true;
}

extern "C" size_t segclip_attn_stats_bytes(const segclip_attn_desc* d) {
  if (d->dtype == SEGCLIP_BF16) return (size_t)d->B * d->H * d->Tq * sizeof(float);
  return (size_t)d->B * d->H * d->Tq * d->Tk * sizeof(float);
}
extern "C" size_t segclip_attn_bwd_ws_bytes(const segclip_attn_desc* d) {
  if (d->dtype != SEGCLIP_BF16) return (size_t)d->B * d->H * d->Tq * d->Tk * sizeof(float);
  if (!long_seq(d)) return 0;
  Device dv;   // enough for either long-sequence route
  if (!current_device(dv)) dv.ncu = 256;
  const size_t stream_ws = (size_t)d->B * d->H * (d->Tq + d->Tk) * sizeof(float);  // streaming kernels: cs[key] and D[q]
  // attention_dqw.inc, key-chunked: 8 KB of fp32 dQ accumulators per query tile and workgroup (one workgroup per CU)
  const size_t dqw_ws = (size_t)dv.ncu * (size_t)(d->Tq / 32 + 1) * 8192;
  return stream_ws > dqw_ws ? stream_ws : dqw_ws;
}

extern "C" int segclip_attn_fwd(const segclip_attn_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  segclip_attn_route_note(false, SEGCLIP_ATTN_ROUTE_NONE, 0, 0);
  SEGCLIP_REQUIRE(d->hd <= 64 && d->hd > 0, "attn: head_dim %lld unsupported (<=64)", (long long)d->hd);
  SEGCLIP_REQUIRE(d->stats != nullptr, "attn_fwd: stats buffer required");
  if (d->B == 0 || d->Tq == 0) return 0;
  FwdArgs a{};
  if (d->dtype == SEGCLIP_BF16) {
    SEGCLIP_REQUIRE(bf16_ok(d), "attn_fwd bf16: head_dim and all strides must be multiples of 8");
    SEGCLIP_REQUIRE(!(d->klen && (d->flags & SEGCLIP_ATTN_FP8)), "attn_fwd: klen is not supported with SEGCLIP_ATTN_FP8");
    fill_common(a, d);
    a.O = (bf16_t*)d->O; a.lse = (float*)d->stats;
    a.lean = 1;   // 0: no lean softmax step on unmasked key tiles (the kernel argument of a settled A/B; folding it in changes device code)
  }
  const Plan p = plan_fwd(d);
  a.staged = p.staged;
  const int nitems = (int)(d->B * d->H);
  int rc;
  switch (p.route) {
    case SEGCLIP_ATTN_ROUTE_SMALLQ: rc = launch<smallq::attn_smallq_fwd_kernel>("attn_smallq_fwd", dim3((unsigned)cdiv(nitems, p.waves)), p.waves, p, stream, a, nitems); break;
    case SEGCLIP_ATTN_ROUTE_PF: rc = launch_fwd_pf(a, p, nitems, stream); break;
    case SEGCLIP_ATTN_ROUTE_GENERIC: rc = launch_fwd_generic(d, a, p, stream); break;
    default: rc = launch_fwd_f32(d, stream); break;
  }
  if (rc == 0) segclip_attn_route_note(false, p.route, p.tiles, p.variant);
  return rc;
}

extern "C" int segclip_attn_bwd(const segclip_attn_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  segclip_attn_route_note(true, SEGCLIP_ATTN_ROUTE_NONE, 0, 0);
  SEGCLIP_REQUIRE(d->hd <= 64 && d->hd > 0, "attn: head_dim %lld unsupported (<=64)", (long long)d->hd);
  if (d->B == 0 || d->Tq == 0) return 0;
  BwdArgs a{};
  if (d->dtype == SEGCLIP_BF16) {
    SEGCLIP_REQUIRE(bf16_ok(d), "attn_bwd bf16: head_dim and all strides must be multiples of 8");
    const int64_t s[] = {d->dq_sb, d->dq_st, d->dk_sb, d->dk_st, d->dv_sb, d->dv_st, d->do_sb, d->do_st};
    for (int64_t v : s) SEGCLIP_REQUIRE(v % 8 == 0, "attn_bwd bf16: gradient strides must be multiples of 8");
    fill_common(a, d);
    a.O = (const bf16_t*)d->O; a.dO = (const bf16_t*)d->dO; a.lse = (const float*)d->stats;
    a.dQ = (bf16_t*)d->dQ; a.dK = (bf16_t*)d->dK; a.dV = (bf16_t*)d->dV;
    a.do_sb = d->do_sb; a.do_st = d->do_st;
    a.dq_sb = d->dq_sb; a.dq_st = d->dq_st; a.dk_sb = d->dk_sb; a.dk_st = d->dk_st; a.dv_sb = d->dv_sb; a.dv_st = d->dv_st;
    a.colsum_part = (float*)d->colsum_part;
    a.nitems = (int)(d->B * d->H);
    a.ws = (float*)d->ws;
  }
  const Plan p = plan_bwd(d);
  if (p.route == SEGCLIP_ATTN_ROUTE_STREAM || (p.route == SEGCLIP_ATTN_ROUTE_DQW && p.variant)) {   // the long-sequence routes
    SEGCLIP_REQUIRE(d->klen == nullptr, "attn_bwd bf16: klen needs sequences of at most %d tokens", TMAX);
    SEGCLIP_REQUIRE(d->ws != nullptr, "attn_bwd bf16: workspace required for sequences longer than %d", TMAX);
  }
  Device dv{};   // the bf16 routes but smallq keep per-device state
  if (p.route != SEGCLIP_ATTN_ROUTE_SMALLQ && p.route != SEGCLIP_ATTN_ROUTE_F32)
    SEGCLIP_REQUIRE(current_device(dv), "attn_bwd: cannot query the current device");
  int rc;
  switch (p.route) {
    case SEGCLIP_ATTN_ROUTE_SMALLQ: rc = launch<smallq::attn_smallq_bwd_kernel>("attn_smallq_bwd", dim3((unsigned)cdiv(a.nitems, p.waves)), p.waves, p, stream, a, a.nitems); break;
    case SEGCLIP_ATTN_ROUTE_DQW: rc = p.variant ? launch_bwd_dqw<true>(a, p, dv, stream) : launch_bwd_dqw<false>(a, p, dv, stream); break;
    case SEGCLIP_ATTN_ROUTE_STREAM: rc = launch_bwd_stream(d, a, p, dv, stream); break;
    case SEGCLIP_ATTN_ROUTE_SPL: rc = launch_bwd_spl(a, p, dv, stream); break;
    case SEGCLIP_ATTN_ROUTE_SP: rc = p.variant ? launch_bwd_sp<true>(a, p, dv, stream) : launch_bwd_sp<false>(a, p, dv, stream); break;
    case SEGCLIP_ATTN_ROUTE_TWOPASS: rc = launch_bwd_twopass(a, p, dv, stream); break;
    default: rc = launch_bwd_f32(d, stream); break;
  }
  if (rc == 0) segclip_attn_route_note(true, p.route, p.tiles, p.variant);
  return rc;
}
