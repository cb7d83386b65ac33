// ------------------------------- single-pass backward, self-attention of <= 256 tokens ---------------------------
// Included by attention.hip inside its anonymous namespace.  One workgroup per (batch, head), ONE WAVE PER 32-KEY TILE
// (T = 197 -> 7 waves).  Every (query tile, key tile) pair is visited exactly once: S and dP are computed once and the
// softmax arithmetic (the VALU work that bounds the two-pass kernel above) once, instead of once per pass:
//     20 MFMAs per pair (S 4, dP 4, dV 4, dK 4, dQ 4) instead of 28, one exponential per score instead of two.
// Wave w owns key tile w: K / V fragments and the dK^T, dV^T accumulators live in its registers for the whole kernel.
// dQ is a sum over key tiles, i.e. over waves: it is accumulated in LDS, in MFMA-accumulator format (fp32, 8 KB per
// query tile: lane-contiguous 16-byte words, conflict-free ds_read/write_b128), with a SKEWED walk - in step s wave w
// works on query tile (w + s) mod n, so no two waves touch the same query tile in a step; one workgroup barrier per
// step orders the read-modify-writes.  Deterministic, no atomics.
// dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q] needs dS with the key index along the MFMA contraction: the wave
// writes its bf16 dS tile ([key][q], 2 KB private scratch, swizzled 64-byte rows) and reads it back with the LDS
// transpose read; K^T fragments come once per kernel from the wave's own K tile staged in LDS.
// Q and dO tiles (read by every wave) sit in LDS as in the two-pass kernel.
constexpr int SP_ACC_BYTES = 8192;    // one query tile of dQ^T in accumulator format: 2 x f32x16 x 64 lanes
constexpr int SP_SCR_BYTES = 2048;    // dS^T scratch of one wave: [32 keys][32 q] bf16

static inline size_t bwd_sp_lds_bytes(int tp) {
  const int n = tp / 32;
  return (size_t)tp * 2 * ROWB + (size_t)n * (SP_ACC_BYTES + SP_SCR_BYTES) + (size_t)tp * 3 * 4 + 8 * 3 * 64 * 4 + 64;
}

using tileimg::swz64;   // byte offset of element (row = key, col = q) in a [32][32] bf16 tile with 64-byte rows: the scratch image

// MFMA B-operand fragment of the scratch tile: lane l -> column q = l&31, k = keys rbase + 4*(l>>5) + {0..3, 8..11}
__device__ __forceinline__ bf16x8_t frag_tr64(const char* t, int rbase, int lane) {
  const int row = tileimg::frag_tr_row(rbase, lane), col = tileimg::frag_tr_col(0, lane);
  const s16x4 lo = tr16_read(t + swz64(row, col));
  const s16x4 hi = tr16_read(t + swz64(tileimg::frag_tr_hi(row), col));
  return tr16_join(lo, hi);
}

// MASKED = false: non-causal, no key-padding mask (the vision tower): the loop body has no branch and no mask test -
// padded query rows get lse = +inf (P = 0), padded key rows have zero K / V rows, whose (finite) P / dS values reach
// nothing that is stored.  S / dP of step s+1 are issued BEFORE the softmax arithmetic of step s (software pipeline:
// the matrix pipe works on the next tile while the VALU works on this one; a step is otherwise one dependent chain
// LDS -> MFMA -> exp -> LDS -> MFMA -> LDS and the two waves of a SIMD, kept in step by the barrier, hide little).
template <bool MASKED>
__global__ __launch_bounds__(512) void attn_bwd_sp_bf16_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_bwd[];
  const int tp = (a.Tq + 31) & ~31, n = tp >> 5;            // Tq == Tk (host-checked); n = blockDim.x / 64 waves
  char* Qt = smem_bwd;
  char* Gt = Qt + tp * ROWB;
  char* Acc = Gt + tp * ROWB;                                // [n][8][64 lanes] f32x4
  char* Scr = Acc + n * SP_ACC_BYTES;                        // [n waves][2 KB]
  float* Ls = reinterpret_cast<float*>(Scr + n * SP_SCR_BYTES);
  float* Ds = Ls + tp;
  float* Cs = Ds + tp;
  float* Red = Cs + tp;                                      // [8 waves][3][64]
  volatile int* Flag = reinterpret_cast<volatile int*>(Red + 8 * 3 * 64);   // [8] steps whose dQ update a wave has finished
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;   // scalar registers
  const int k0 = wave * 32;
  char* myacc = Acc + wave * SP_ACC_BYTES;
  const int nitems = a.nitems;

  // ---- PERSISTENT over (batch, head) items: workgroup g takes items g, g + gridDim.x, ...  Every global load of an
  // item is issued in one go into registers (one memory round trip; a select right behind a load would make hipcc wait
  // for it, which serialised the first version's prologue: 147 of 420 us) - and for every item but a workgroup's first
  // it is issued BEFORE the previous item's output phase, so the round trip, the store drain and the workgroup launch
  // that used to sit between two main loops (8.6 + 3.3 us of 29 us per item) overlap.
  // blockDim = 64 n threads and the tiles have 32 n rows of 8 chunks: every thread owns exactly 4 chunks of each tile.
  u32x4 rk[4], rv[4], rks[4], rq[4], rg_[4], ro[4];
  float lse_l = 0.f;
  // the K / V fragments of the own key tile ... (issuing these 32 registers one step earlier, beside the last step of the
  // previous item whose look-ahead S / dP registers are free, measured slower: 315 vs 297 us, 14 spills instead of 1)
  auto issue_kv = [&](int item, int tid) {
    const int lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int b = item / a.H, h = item - b * a.H;
    const int64_t hoff = (int64_t)h * a.hd;
    const bf16_t* Kp = a.K + b * a.k_sb + hoff;
    const bf16_t* Vp = a.V + b * a.v_sb + hoff;
    const int rr = k0 + li;                       // fragment row of this lane (K, V rows of the own key tile)
    const int rc = rr < a.Tk ? rr : a.Tk - 1;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const int c = kc * 16 + 8 * lh, cc = c < a.hd ? c : 0;
      rk[kc] = *reinterpret_cast<const u32x4*>(Kp + (int64_t)rc * a.k_st + cc);
      rv[kc] = *reinterpret_cast<const u32x4*>(Vp + (int64_t)rc * a.v_st + cc);
    }
  };
  // ... and the staged tiles (K once more for the K^T fragments, Q, dO, O) + lse: 65 registers, after the main loop
  auto issue_rest = [&](int item, int tid) {
    const int lane = tid & 63;
    const int b = item / a.H, h = item - b * a.H;
    const int64_t hoff = (int64_t)h * a.hd;
    const bf16_t* Qp = a.Q + b * a.q_sb + hoff;
    const bf16_t* Kp = a.K + b * a.k_sb + hoff;
    const bf16_t* Op = a.O + b * a.o_sb + hoff;
    const bf16_t* Gp = a.dO + b * a.do_sb + hoff;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * 64 + lane, r = idx >> 3, c = idx & 7;          // own K tile: 32 rows x 8 chunks per wave
      const int kr = k0 + r < a.Tk ? k0 + r : a.Tk - 1, cc = c * 8 < a.hd ? c : 0;
      rks[it] = *reinterpret_cast<const u32x4*>(Kp + (int64_t)kr * a.k_st + cc * 8);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * (int)blockDim.x + tid, r = idx >> 3, c = idx & 7;
      const int qr = r < a.Tq ? r : a.Tq - 1, cc = c * 8 < a.hd ? c : 0;
      rq[it] = *reinterpret_cast<const u32x4*>(Qp + (int64_t)qr * a.q_st + cc * 8);
      rg_[it] = *reinterpret_cast<const u32x4*>(Gp + (int64_t)qr * a.do_st + cc * 8);
      ro[it] = *reinterpret_cast<const u32x4*>(Op + (int64_t)qr * a.o_st + cc * 8);
    }
    // log2 domain; padded rows: P = exp2(-inf) = 0
    if (tid < tp) lse_l = tid < a.Tq ? a.lse[((int64_t)b * a.H + h) * a.Tq + tid] * 1.4426950408889634f : INFINITY;
  };
  if ((int)blockIdx.x < nitems) { issue_kv(blockIdx.x, threadIdx.x); issue_rest(blockIdx.x, threadIdx.x); }

  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
  // The lane-dependent LDS / global offsets below are loop invariants; hoisted out of the item loop they would all stay
  // live across the main loop (which already uses every register) and spill: the thread id is made opaque per item.
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, li = lane & 31, lh = lane >> 5, key = k0 + li;
  const int b = item / a.H, h = item - b * a.H;
  const int64_t hoff = (int64_t)h * a.hd;
  const int kvalid = a.klen ? (a.klen[b] < a.Tk ? a.klen[b] : a.Tk) : a.Tk;
  const int nxt_item = item + (int)gridDim.x < nitems ? item + (int)gridDim.x : item;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  bf16x8_t kf[4], vf[4];
  {
    const bool rok = k0 + li < a.Tk;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const bool ok = rok && kc * 16 + 8 * lh < a.hd;
      kf[kc] = __builtin_bit_cast(bf16x8_t, ok ? rk[kc] : zero4);
      vf[kc] = __builtin_bit_cast(bf16x8_t, ok ? rv[kc] : zero4);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * 64 + lane, r = idx >> 3, c = idx & 7;
      *reinterpret_cast<u32x4*>(myacc + swz(r, c * 8)) = (k0 + r < a.Tk && c * 8 < a.hd) ? rks[it] : zero4;
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * (int)blockDim.x + tid, r = idx >> 3, c = idx & 7;
      const bool ok = r < a.Tq && c * 8 < a.hd;
      const u32x4 q4 = ok ? rq[it] : zero4, g = ok ? rg_[it] : zero4, o4 = ok ? ro[it] : zero4;
      float sdot = 0.f;   // D[q] = sum_d dO*O: 8 consecutive lanes share a row
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sdot += __uint_as_float(g[j] << 16) * __uint_as_float(o4[j] << 16);
        sdot += __uint_as_float(g[j] & 0xffff0000u) * __uint_as_float(o4[j] & 0xffff0000u);
      }
      sdot += __shfl_xor(sdot, 1, 64); sdot += __shfl_xor(sdot, 2, 64); sdot += __shfl_xor(sdot, 4, 64);
      *reinterpret_cast<u32x4*>(Qt + swz(r, c * 8)) = q4;
      *reinterpret_cast<u32x4*>(Gt + swz(r, c * 8)) = g;
      if (c == 0) Ds[r] = sdot;
    }
    if (tid < tp) Ls[tid] = lse_l;
  }
  __syncthreads();
  // K^T fragments of the own key tile: ktr[dt][half]: lane -> d = dt*32 + (l&31), k = keys 16*half + 4*(l>>5) + {0..3, 8..11}
  bf16x8_t ktr[2][2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) ktr[dt][hf] = frag_tr(myacc, hf * 16, dt * 32, lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  {  // the slot becomes query tile `wave`'s dQ^T accumulator: zero it (8 x 16 bytes per lane)
    f32x4* z = reinterpret_cast<f32x4*>(myacc);
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8) z[tileimg::accq_index(g8, lane)] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (lane == 0) Flag[wave] = 0;
  }
  __syncthreads();

  // (Tried: an L2 touch of the NEXT item here - one 4-byte LDS-DMA load per 128-byte row of its Q, K, V, dO, O, no
  // destination register - so that the register loads after the loop hit L2: 294 vs 266 us, SLOWER.  The 32 CUs of an
  // XCD touch 4.8 MB per round and write 2.4 MB into a 4-MiB L2: the lines are gone again before they are used, and
  // the HBM traffic doubles.)
  const float sc2 = a.scale * 1.4426950408889634f;
  char* scr = Scr + wave * SP_SCR_BYTES;
  // lane-constant offsets of the row / transposed fragments inside a 32-row query tile (round 5: the tile index of the skewed
  // walk is a run-time value, and frag_rows / frag_tr recomputed the swizzle per fragment: ~55 of the loop's ~210 VALU
  // instructions per pair were address arithmetic; swz(32 j + r, c) = 32 j ROWB + swz(r, c))
  int koff[4], toff[2][2];
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) koff[kc] = swz(li, tileimg::frag_rows_col(kc, lh));
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int j = 0; j < 2; ++j) toff[dt][j] = tr_lane_off(lane, dt, j);
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }
  float csl = 0.f;

  auto tile_of = [&](int step) { const int j = wave + step; return j >= n ? j - n : j; };
  auto sdp = [&](int q0, f32x16& s, f32x16& dp) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
    const char* qb_ = Qt + q0 * ROWB;
    const char* gb_ = Gt + q0 * ROWB;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(qb_ + koff[kc]), kf[kc], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(gb_ + koff[kc]), vf[kc], dp, 0, 0, 0);
    }
  };
  // everything of a pair after S / dP: softmax, dV, dK, dQ (registers), then barrier + dQ read-modify-write
  auto finish = [&](int step, const f32x16& s, const f32x16& dp, bool skip) {
    const int jt = tile_of(step);
    const int q0 = jt * 32;
    f32x16 dq[2];
    if (!skip) {
      // P = exp2(S * scale*log2e - lse*log2e); dS kept WITHOUT the softmax scale (applied once to dK, dQ and the column
      // sums at the end); key-padding / causal masks only on tiles that contain masked elements (wave-uniform test)
      const bool edge = MASKED && (k0 + 32 > kvalid || (a.causal && k0 + 31 > q0));
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
            const bool ok = key < kvalid && (!a.causal || key <= q);
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
      // dS^T tile -> scratch [key][q]: lane (key) writes its 4 x 4 consecutive query values
      {
        const u32x4 w0 = __builtin_bit_cast(u32x4, sb0), w1 = __builtin_bit_cast(u32x4, sb1);
        const u32x2 g0 = {w0[0], w0[1]}, g1 = {w0[2], w0[3]}, g2 = {w1[0], w1[1]}, g3 = {w1[2], w1[3]};
        *reinterpret_cast<u32x2*>(scr + swz64(li, tileimg::park_col(0, 0, lh))) = g0;
        *reinterpret_cast<u32x2*>(scr + swz64(li, tileimg::park_col(0, 1, lh))) = g1;
        *reinterpret_cast<u32x2*>(scr + swz64(li, tileimg::park_col(0, 2, lh))) = g2;
        *reinterpret_cast<u32x2*>(scr + swz64(li, tileimg::park_col(0, 3, lh))) = g3;
      }
      const char* qt_ = Qt + q0 * ROWB;
      const char* gt_ = Gt + q0 * ROWB;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr16_frag(gt_, toff[dt][0], toff[dt][1]), pb0, dv[dt], 0, 0, 0);
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr16_frag(gt_ + 16 * ROWB, toff[dt][0], toff[dt][1]), pb1, dv[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr16_frag(qt_, toff[dt][0], toff[dt][1]), sb0, dk[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr16_frag(qt_ + 16 * ROWB, toff[dt][0], toff[dt][1]), sb1, dk[dt], 0, 0, 0);
      }
      // the scratch writes above are this wave's own (LDS operations of one wave execute in order)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      const bf16x8_t st0 = frag_tr64(scr, 0, lane), st1 = frag_tr64(scr, 16, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[dt][0], st0, dq[dt], 0, 0, 0);
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[dt][1], st1, dq[dt], 0, 0, 0);
      }
    }
    // dQ read-modify-write.  Query tile jt was last updated by the NEXT wave (w+1 visits it one step earlier), so this
    // wave only has to wait until that neighbour has finished its previous step - a ring of flags in LDS instead of a
    // workgroup barrier per step: the waves of a SIMD may drift apart (one in its MFMA phase, the other in its VALU
    // phase) instead of being re-aligned 7 times.  The LDS executes a wave's operations in order, so a flag value seen
    // here implies the neighbour's accumulator writes are done.  `step` = index of this pair in the wave's walk.
    if (step > 0) {
      const int nb = wave + 1 == n ? 0 : wave + 1;
      while (Flag[nb] < step) __builtin_amdgcn_s_sleep(1);
    }
    if (!skip) {
      f32x4* acc = reinterpret_cast<f32x4*>(Acc + jt * SP_ACC_BYTES);
#pragma unroll
      for (int g8 = 0; g8 < 8; ++g8) {
        f32x4 v = acc[tileimg::accq_index(g8, lane)];
        const int dt = tileimg::accq_dt(g8), rb = tileimg::accq_reg(g8);
        v[0] += dq[dt][rb]; v[1] += dq[dt][rb + 1]; v[2] += dq[dt][rb + 2]; v[3] += dq[dt][rb + 3];
        acc[tileimg::accq_index(g8, lane)] = v;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) Flag[wave] = step + 1;
  };
  if (MASKED) {
    for (int s_ = 0; s_ < n; ++s_) {
      const int jt = tile_of(s_);
      const bool skip = a.causal && jt * 32 + 31 < k0;       // every score of the pair is masked (wave-uniform)
      f32x16 s, dp;
      if (!skip) sdp(jt * 32, s, dp);
      finish(s_, s, dp, skip);
    }
  } else {
    f32x16 s, dp;
    sdp(tile_of(0) * 32, s, dp);
    for (int s_ = 0; s_ + 1 < n; ++s_) {
      f32x16 sn, dpn;
      sdp(tile_of(s_ + 1) * 32, sn, dpn);      // independent of the step finished below: overlaps its VALU / LDS work
      finish(s_, s, dp, false);
      s = sn; dp = dpn;
    }
    finish(n - 1, s, dp, false);
  }
  // the next item's loads go out now: they travel while this item's outputs are staged and stored
  // (unconditional, the last item re-reads itself: behind a condition the OLD register values would stay live across the
  // main loop on the not-taken path and spill)
  issue_kv(nxt_item, tid);
  issue_rest(nxt_item, tid);
#pragma unroll
  for (int r = 0; r < 16; ++r) { dk[0][r] *= a.scale; dk[1][r] *= a.scale; }
  csl += __shfl_xor(csl, 32, 64);
  if (lh == 0) Cs[key] = csl * a.scale;
  __syncthreads();   // all read-modify-writes of the last step are done; Cs is complete
  // Outputs.  The accumulators hold TRANSPOSED tiles (lane = row, registers = 4 consecutive columns): stored straight
  // from registers every instruction touches 32 rows with 16 bytes each (85 of 420 us in the first version).  They go
  // through the wave's own accumulator slot instead (free once its dQ has been read): 8-byte LDS writes, 16-byte reads of
  // whole 128-byte rows, 16-byte coalesced global stores.
  f32x16 dq[2];
  {
    const f32x4* acc = reinterpret_cast<const f32x4*>(myacc);
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8) {
      const f32x4 v = acc[tileimg::accq_index(g8, lane)];
      const int dt = tileimg::accq_dt(g8), rb = tileimg::accq_reg(g8);
      dq[dt][rb] = v[0] * a.scale; dq[dt][rb + 1] = v[1] * a.scale; dq[dt][rb + 2] = v[2] * a.scale; dq[dt][rb + 3] = v[3] * a.scale;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  auto put_tile = [&](char* tile, const f32x16 (&acc)[2]) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        u32x2 t;
        t[0] = pack2bf(acc[dt][rg * 4 + 0], acc[dt][rg * 4 + 1]);
        t[1] = pack2bf(acc[dt][rg * 4 + 2], acc[dt][rg * 4 + 3]);
        *reinterpret_cast<u32x2*>(tile + swz(li, tileimg::park_col(dt, rg, lh))) = t;
      }
  };
  auto flush_tile = [&](const char* tile, bf16_t* base, int64_t st, int nrows) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * 64 + lane, r = idx >> 3, c = idx & 7;
      const u32x4 v = *reinterpret_cast<const u32x4*>(tile + swz(r, c * 8));
      if (k0 + r < nrows && c * 8 < a.hd) *reinterpret_cast<u32x4*>(base + (int64_t)(k0 + r) * st + c * 8) = v;
    }
  };
  put_tile(myacc, dk);
  put_tile(myacc + 4096, dv);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  flush_tile(myacc, a.dK + b * a.dk_sb + hoff, a.dk_st, a.Tk);
  flush_tile(myacc + 4096, a.dV + b * a.dv_sb + hoff, a.dv_st, a.Tk);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  put_tile(myacc, dq);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  flush_tile(myacc, a.dQ + b * a.dq_sb + hoff, a.dq_st, a.Tq);
  // ---- token sums of dQ | dK | dV (in_proj bias gradient of this sample and head):
  //   sum_q dQ[q][d] = sum_key K[key][d] cs[key]: one more product on the matrix pipe, K^T fragments (registers) x a
  //     B operand whose columns all hold cs (split into two bf16 parts: 16 mantissa bits) - no second read of K;
  //   sum_key dV[key][d] = sum_q dO[q][d] (dO tile in LDS);  sum_key dK[key][d] = 0 (rows of dS sum to zero)
  if (a.colsum_part) {
    f32x16 cq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { cq[0][r] = 0.f; cq[1][r] = 0.f; }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const f32x4 c0 = *reinterpret_cast<const f32x4*>(Cs + k0 + 16 * hf + 4 * lh);
      const f32x4 c1 = *reinterpret_cast<const f32x4*>(Cs + k0 + 16 * hf + 4 * lh + 8);
      float hi[8], lo[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hi[j] = __uint_as_float(__float_as_uint(c0[j]) & 0xffff0000u); lo[j] = c0[j] - hi[j];
        hi[4 + j] = __uint_as_float(__float_as_uint(c1[j]) & 0xffff0000u); lo[4 + j] = c1[j] - hi[4 + j];
      }
      const bf16x8_t bh = pack8(hi), bl = pack8(lo);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        cq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[dt][hf], bh, cq[dt], 0, 0, 0);
        cq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[dt][hf], bl, cq[dt], 0, 0, 0);
      }
    }
    if (li == 0) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) Red[(wave * 3 + 0) * 64 + dt * 32 + acc_row(r, lh)] = cq[dt][r];
    }
    const int c = tid & 7, nrl = (int)blockDim.x >> 3;
    float accv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) accv[j] = 0.f;
    for (int r = tid >> 3; r < tp; r += nrl) {
      const u32x4 gv = *reinterpret_cast<const u32x4*>(Gt + swz(r, c * 8));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        accv[2 * j] += __uint_as_float(gv[j] << 16);
        accv[2 * j + 1] += __uint_as_float(gv[j] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float vv = accv[j];
      vv += __shfl_xor(vv, 8, 64);
      vv += __shfl_xor(vv, 16, 64);
      vv += __shfl_xor(vv, 32, 64);
      if (lane < 8) Red[(wave * 3 + 2) * 64 + c * 8 + j] = vv;
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
  __syncthreads();   // the next item's staging overwrites the tiles and slots read above
  }  // items
}
