// ------------------------------- single-pass backward WITH A LOADER WAVE, self-attention of 161..224 tokens ----------
// Included by attention.hip inside its anonymous namespace (round 5).  The main loop is the one of attention_sp.inc (one wave
// per 32-key tile, every (query tile, key tile) pair visited once, dQ accumulated in LDS in accumulator format by a skewed
// walk behind a flag ring); what changes is WHO MOVES THE DATA.  In attention_sp.inc every compute wave issues 25 global
// loads right behind the main loop (next item's K / V fragments, its share of Q, dO, O, lse) and 12 stores in the output
// phase; the persistent attention forward of this round measured what that costs: a wave stalls
// 200-400 cycles IN THE ISSUE of each such instruction while the CU's vector-memory path is backed up by its own misses.
// The kernel without its main loop took 145 of 297 us: the memory phases were never hidden.  Here
//   * an extra LOADER WAVE (wave n) owns the memory traffic.  During main loop i it brings item i+1's K tile into a spare
//     25-KiB LDS area by LDS-DMA, loads dO and O of item i+1 into ITS OWN registers (a wave has 256 of them: 100 hold the
//     dO tile), computes D = rowsum(dO * O), the token sums of dO (in_proj bias gradient of V) and the log2-domain lse, and
//     parks them in second copies of the small vectors.  When the main loop has ended (barrier S2) the Q / dO tiles are dead:
//     Q of item i+1 arrives by LDS-DMA, dO is written from the loader's registers, and the dK / dV tiles the compute waves
//     park in their (dead) accumulator slots leave through the loader as whole 128-byte rows;
//   * a compute wave issues 4 loads (its V fragments of the next item) and 4 stores (its dQ tile, through its 2-KB scratch in
//     two halves) per item - 8 vector-memory instructions instead of 37.
// LDS (T <= 224, n = 7): K-next 25 KB + Q 28 + dO 28 + dQ accumulators 56 + dS scratch 14 + vectors: 158 KB of 160.
// Restrictions (host-checked): no causal / key-padding mask (the vision tower), Tq == Tk, 5 <= tiles <= 7.
constexpr int SPL_MAXT = 224;

__host__ __device__ static inline size_t bwd_spl_lds_bytes(int T) {
  const int tp = (T + 31) & ~31, n = tp / 32, R = (T + 7) & ~7;
  return (size_t)R * ROWB + (size_t)tp * 2 * ROWB + (size_t)n * (SP_ACC_BYTES + SP_SCR_BYTES) + (size_t)tp * 5 * 4 + 2 * 64 * 4 +
         (size_t)n * 64 * 4 + 64;
}

__global__ __launch_bounds__(512) void attn_bwd_spl_bf16_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_bwd[];
  const int T = a.Tq;                                        // == Tk
  const int tp = (T + 31) & ~31, n = tp >> 5, R = (T + 7) & ~7;
  char* KN = smem_bwd;                                       // next item's K tile, R rows (what follows is finite bf16 data)
  char* Qt = KN + R * ROWB;
  char* Gt = Qt + tp * ROWB;
  char* Acc = Gt + tp * ROWB;                                // [n][8][64 lanes] f32x4
  char* Scr = Acc + n * SP_ACC_BYTES;                        // [n waves][2 KB]
  float* Lsb = reinterpret_cast<float*>(Scr + n * SP_SCR_BYTES);   // [2][tp] lse * log2(e) (+inf on padded rows)
  float* Dsb = Lsb + 2 * tp;                                 // [2][tp] D[q] = sum_d dO O
  float* Cs = Dsb + 2 * tp;                                  // [tp]    cs[key] = sum_q dS
  float* Gsb = Cs + tp;                                      // [2][64] token sums of dO
  float* Red = Gsb + 2 * 64;                                 // [n][64] token sums of dQ, per key-tile wave
  volatile int* Flag = reinterpret_cast<volatile int*>(Red + n * 64);   // [8] flag ring of the main loop; [8] = parked-tile counter
  const uint32_t lds0 = (uint32_t)(uintptr_t)((lds_void*)smem_bwd);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nitems = a.nitems;

  // everything a fragment read may find must be finite
  {
    const int total16 = (int)(bwd_spl_lds_bytes(T) >> 4);
    for (int i = threadIdx.x; i < total16; i += (int)blockDim.x) reinterpret_cast<u32x4*>(smem_bwd)[i] = u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();

  if (wave == n) {
    // ================================================ loader wave ================================================
    const int lane = threadIdx.x & 63, c = lane & 7;
    const int npk = R >> 3;                                  // 8-row pieces of a K tile
    const int npq = tp >> 3;                                 // 8-row pieces of the Q / dO tiles
    const bool cok = c * 8 < a.hd;
#include "attention_dma_tile.inc"   // src_off, dma_tile
    u32x4 gd[28];                                            // dO tile of the NEXT item: piece q -> row 8 q + lr, chunk c (unswizzled)
    // item `item`: K -> KN, dO -> gd registers, D / lse / token sums of dO -> the vectors' buffer `nb`
    auto prefetch = [&](int item, int nb) {
      const int b = item / a.H, h = item - b * a.H;
      const int64_t hoff = (int64_t)h * a.hd;
      dma_tile(a.K + b * a.k_sb + hoff, a.k_st, npk, lds0);
      const bf16_t* Gp = a.dO + b * a.do_sb + hoff;
      const bf16_t* Op = a.O + b * a.o_sb + hoff;
      float* Ln = Lsb + nb * tp;
      float* Dn = Dsb + nb * tp;
      const float* lg = a.lse + ((int64_t)b * a.H + h) * T;
      for (int r = lane; r < tp; r += 64) Ln[r] = r < T ? lg[r] * 1.4426950408889634f : INFINITY;   // padded rows: P = exp2(-inf) = 0
      float gs[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) gs[j] = 0.f;
      // buffer loads: ONE lane-constant offset register per tensor + a scalar offset per 8-row piece (28 x 2 flat loads would
      // keep 112 address registers next to the 112 data registers: spilled); rows beyond T are out of the descriptor's range
      // and come back as zeros
      const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(Gp), 0, (int)((((int64_t)T - 1) * a.do_st + a.hd) * 2), 0x00020000);
      const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(Op), 0, (int)((((int64_t)T - 1) * a.o_st + a.hd) * 2), 0x00020000);
      const int vG = (int)(((int64_t)lr * a.do_st + c * 8) * 2), vO = (int)(((int64_t)lr * a.o_st + c * 8) * 2);
      const int pG = (int)(8 * a.do_st * 2), pO = (int)(8 * a.o_st * 2);
      // every dO load first (the tile stays in registers anyway), then O in rounds of 4 pieces with the next round's loads
      // in flight while a round is reduced (one round trip per round would serialise 7 HBM latencies per item)
#pragma unroll
      for (int q = 0; q < 28; ++q) gd[q] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsG, vG, q * pG, 0));
      u32x4 ova[4], ovb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) ova[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsO, vO, u * pO, 0));
      auto reduce4 = [&](int q0, const u32x4 (&ov)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = (q0 + u) * 8 + lr;
          if (!cok) gd[q0 + u] = u32x4{0u, 0u, 0u, 0u};
          const u32x4 g = gd[q0 + u], o4 = ov[u];
          float sdot = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float g0 = __uint_as_float(g[j] << 16), g1 = __uint_as_float(g[j] & 0xffff0000u);
            sdot += g0 * __uint_as_float(o4[j] << 16);
            sdot += g1 * __uint_as_float(o4[j] & 0xffff0000u);
            gs[2 * j] += g0; gs[2 * j + 1] += g1;
          }
          sdot += __shfl_xor(sdot, 1, 64); sdot += __shfl_xor(sdot, 2, 64); sdot += __shfl_xor(sdot, 4, 64);
          if (c == 0 && r < tp) Dn[r] = sdot;
        }
      };
#pragma unroll
      for (int q0 = 0; q0 < 28; q0 += 8) {
        if (q0 + 4 < 28) {
#pragma unroll
          for (int u = 0; u < 4; ++u) ovb[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsO, vO, (q0 + 4 + u) * pO, 0));
        }
        reduce4(q0, ova);
        if (q0 + 8 < 28) {
#pragma unroll
          for (int u = 0; u < 4; ++u) ova[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsO, vO, (q0 + 8 + u) * pO, 0));
        }
        if (q0 + 4 < 28) reduce4(q0 + 4, ovb);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {                          // token sums of dO: over the 8 row groups (lanes c, c+8, ..)
        float v = gs[j];
        v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
        if (lane < 8) Gsb[nb * 64 + c * 8 + j] = v;
      }
    };
    // dO tile of the next item from the registers -> Gt
    auto fill_tiles = [&](int item) {
      (void)item;                                            // (Q: 4 LDS-DMA pieces per compute wave, behind S2 as well)
      // swz(8 q + lr, .) only depends on the parity of q besides the row term 1024 q: two lane-constant offsets + immediates
      int lane_o = lane;
      asm volatile("" : "+v"(lane_o));
      const int lro = lane_o >> 3, co = lane_o & 7;
      char* const ge = Gt + swz(lro, co * 8);
      char* const go = Gt + swz(8 + lro, co * 8) - 1024;
#pragma unroll
      for (int q = 0; q < 28; ++q)
        if (q < npq) *reinterpret_cast<u32x4*>(((q & 1) ? go : ge) + q * 1024) = gd[q];
    };
    // dK, dV tiles parked by the compute waves in their accumulator slots -> global, whole rows
    auto flush_kv = [&](int item) {
      const int b = item / a.H, h = item - b * a.H;
      const int64_t hoff = (int64_t)h * a.hd;
      // buffer stores: rows beyond T fall outside the descriptors and are dropped (no per-lane guards, no address registers)
      const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(a.dK + b * a.dk_sb + hoff, 0, (int)((((int64_t)T - 1) * a.dk_st + a.hd) * 2), 0x00020000);
      const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(a.dV + b * a.dv_sb + hoff, 0, (int)((((int64_t)T - 1) * a.dv_st + a.hd) * 2), 0x00020000);
      const int vK = cok ? (int)(((int64_t)lr * a.dk_st + c * 8) * 2) : 0x7fffff00, vV = cok ? (int)(((int64_t)lr * a.dv_st + c * 8) * 2) : 0x7fffff00;
      const int pK = (int)(8 * a.dk_st * 2), pV = (int)(8 * a.dv_st * 2);
      const int npv = (T + 7) >> 3;                          // pieces with at least one valid row
      for (int q = 0; q < npv; q += 2) {                     // 2 pieces x (dK, dV) per round
        u32x4 vk[2], vv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int r = (q + u) * 8 + lr, w = r >> 5, rr = r & 31;
          const char* slot = Acc + (w < n ? w : n - 1) * SP_ACC_BYTES;
          vk[u] = *reinterpret_cast<const u32x4*>(slot + swz(rr, c * 8));
          vv[u] = *reinterpret_cast<const u32x4*>(slot + 4096 + swz(rr, c * 8));
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int, vk[u]), rsK, vK, (q + u) * pK, 0);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int, vv[u]), rsV, vV, (q + u) * pV, 0);
        }
      }
    };
    // token sums of dQ | dK | dV of the item BEFORE (Red is complete behind the barrier S0 that follows its output phase)
    auto flush_colsum = [&](int item, int nb) {
      if (!a.colsum_part) return;
      const int b = item / a.H, h = item - b * a.H;
      float* dst = a.colsum_part + (int64_t)b * 3 * ((int64_t)a.H * a.hd) + (int64_t)h * a.hd;
      if (lane < a.hd) {
        float vq = 0.f;
        for (int w = 0; w < n; ++w) vq += Red[w * 64 + lane];
        dst[lane] = vq;
        dst[(int64_t)a.H * a.hd + lane] = 0.f;               // rows of dS sum to zero: the token sums of dK are exactly 0
        dst[2 * (int64_t)a.H * a.hd + lane] = Gsb[nb * 64 + lane];
      }
    };

    int item = blockIdx.x, cur = 0, prev = -1, parked = 0;
    if (item < nitems) {
      prefetch(item, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // K(item) in KN; the K fragments are read between S0 and S1
      {
        const int b0 = item / a.H, h0 = item - b0 * a.H;     // the first item's Q: all pieces from here
        dma_tile(a.Q + b0 * a.q_sb + (int64_t)h0 * a.hd, a.q_st, npq, lds0 + (uint32_t)(Qt - smem_bwd));
      }
      fill_tiles(item);
    }
    for (; item < nitems; item += gridDim.x) {
      const int nxt = item + (int)gridDim.x;
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();                                       // S0: Q / dO / K / vectors of `item` are in LDS
      if (prev >= 0) flush_colsum(prev, cur ^ 1);
      __syncthreads();                                       // S1: the K fragments are in registers, the accumulators are zero
      if (nxt < nitems) prefetch(nxt, cur ^ 1);              // during the main loop: K-next, dO-next (registers), D, lse, sums
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();                                       // S2: the main loop has ended: the Q / dO tiles are dead
      if (nxt < nitems) fill_tiles(nxt);
      // "S3" is one-way (as a barrier it made the compute waves wait ~4000 cycles per item for the loader's Q DMA issue):
      // every compute wave bumps a counter when its dK / dV tiles are parked
      ++parked;
      while (Flag[8] < parked * n) __builtin_amdgcn_s_sleep(2);
      flush_kv(item);
      prev = item;
      cur ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();                                         // final S0
    if (prev >= 0) flush_colsum(prev, cur ^ 1);
    return;
  }

  // ================================================ compute waves ================================================
  const int k0 = wave * 32;
  char* myacc = Acc + wave * SP_ACC_BYTES;
  char* scr = Scr + wave * SP_SCR_BYTES;
  const float sc2 = a.scale * 1.4426950408889634f;
  u32x4 rv[4];                                               // V fragments of the item that runs next
  auto issue_v = [&](int item, int tid) {
    const int lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int b = item / a.H, h = item - b * a.H;
    const bf16_t* Vp = a.V + b * a.v_sb + (int64_t)h * a.hd;
    const int rr = k0 + li, rc = rr < T ? rr : T - 1;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const int cc = kc * 16 + 8 * lh;
      rv[kc] = *reinterpret_cast<const u32x4*>(Vp + (int64_t)rc * a.v_st + (cc < a.hd ? cc : 0));
    }
  };
  if ((int)blockIdx.x < nitems) issue_v(blockIdx.x, threadIdx.x);
  int cur = 0;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));                            // lane-dependent offsets are not hoisted across items
    const int lane = tid & 63, li = lane & 31, lh = lane >> 5, key = k0 + li;
    const int b = item / a.H, h = item - b * a.H;
    const int nxt_item = item + (int)gridDim.x < nitems ? item + (int)gridDim.x : item;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const float* Ls = Lsb + cur * tp;
    const float* Ds = Dsb + cur * tp;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this wave's Q pieces of `item` have landed
    __syncthreads();                                         // S0
    bf16x8_t kf[4], vf[4], ktr[2][2];
    {
      const bool rok = key < T;
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const bool ok = rok && kc * 16 + 8 * lh < a.hd;
        const u32x4 kraw = *reinterpret_cast<const u32x4*>(KN + swz(key, kc * 16 + 8 * lh));
        kf[kc] = __builtin_bit_cast(bf16x8_t, ok ? kraw : zero4);
        vf[kc] = __builtin_bit_cast(bf16x8_t, ok ? rv[kc] : zero4);
      }
      // K^T fragments of the own key tile: lane -> d = dt*32 + (l&31), k = keys 16*hf + 4*(l>>5) + {0..3, 8..11}
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          u32x4 f = __builtin_bit_cast(u32x4, frag_tr(KN, k0 + hf * 16, dt * 32, lane));
          if (k0 + 32 > T) {                                 // the last key tile: keys beyond T (clamped duplicates) count as zero rows
            const int kb = k0 + hf * 16 + 4 * lh;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int ka = kb + (j & 1) * 2 + (j >> 1) * 8;   // register j holds keys ka, ka + 1
              const uint32_t msk = (ka < T ? 0x0000ffffu : 0u) | (ka + 1 < T ? 0xffff0000u : 0u);
              f[j] &= msk;
            }
          }
          if (dt * 32 + li >= a.hd) f = zero4;
          ktr[dt][hf] = __builtin_bit_cast(bf16x8_t, f);
        }
      f32x4* z = reinterpret_cast<f32x4*>(myacc);            // the slot becomes query tile `wave`'s dQ^T accumulator
#pragma unroll
      for (int g8 = 0; g8 < 8; ++g8) z[tileimg::accq_index(g8, lane)] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (lane == 0) Flag[wave] = 0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();                                         // S1

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
      // all 8 fragments in flight before the first product (left to itself hipcc waits for each ds_read right in front of its
      // MFMA: 8 serialised LDS round trips per pair)
      bf16x8_t qa[4], ga[4];
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        qa[kc] = *reinterpret_cast<const bf16x8_t*>(qb_ + koff[kc]);
        ga[kc] = *reinterpret_cast<const bf16x8_t*>(gb_ + koff[kc]);
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[kc], kf[kc], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[kc], vf[kc], dp, 0, 0, 0);
      }
    };
    // everything of a pair after S / dP (attention_sp.inc): softmax, dV, dK, dQ in registers, then the flag ring + the
    // read-modify-write of the query tile's dQ accumulator
    auto finish = [&](int step, const f32x16& s, const f32x16& dp) {
      const int jt = tile_of(step);
      const int q0 = jt * 32;
      f32x16 dq[2];
      float p[16], ds[16];
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
      const bf16x8_t pb0 = pack8(p), pb1 = pack8(p + 8), sb0 = pack8(ds), sb1 = pack8(ds + 8);
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
      bf16x8_t gtf[2][2], qtf[2][2];                        // the 16 transposed fragments of the pair in one batch
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        gtf[dt][0] = tr16_frag(gt_, toff[dt][0], toff[dt][1]);
        gtf[dt][1] = tr16_frag(gt_ + 16 * ROWB, toff[dt][0], toff[dt][1]);
        qtf[dt][0] = tr16_frag(qt_, toff[dt][0], toff[dt][1]);
        qtf[dt][1] = tr16_frag(qt_ + 16 * ROWB, toff[dt][0], toff[dt][1]);
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gtf[dt][0], pb0, dv[dt], 0, 0, 0);
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gtf[dt][1], pb1, dv[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf[dt][0], sb0, dk[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf[dt][1], sb1, dk[dt], 0, 0, 0);
      }
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
      if (step > 0) {
        const int nb = wave + 1 == n ? 0 : wave + 1;
        while (Flag[nb] < step) __builtin_amdgcn_s_sleep(1);
      }
      f32x4* acc = reinterpret_cast<f32x4*>(Acc + jt * SP_ACC_BYTES);
#pragma unroll
      for (int g8 = 0; g8 < 8; ++g8) {
        f32x4 v = acc[tileimg::accq_index(g8, lane)];
        const int dt = tileimg::accq_dt(g8), rb = tileimg::accq_reg(g8);
        v[0] += dq[dt][rb]; v[1] += dq[dt][rb + 1]; v[2] += dq[dt][rb + 2]; v[3] += dq[dt][rb + 3];
        acc[tileimg::accq_index(g8, lane)] = v;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) Flag[wave] = step + 1;
    };
    {
      f32x16 s, dp;
      sdp(tile_of(0) * 32, s, dp);
      for (int s_ = 0; s_ + 1 < n; ++s_) {
        f32x16 sn, dpn;
        sdp(tile_of(s_ + 1) * 32, sn, dpn);
        finish(s_, s, dp);
        s = sn; dp = dpn;
      }
      finish(n - 1, s, dp);
    }
    // this wave's only loads: the V fragments of the next item (they travel during the output phase)
    issue_v(nxt_item, tid);
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[0][r] *= a.scale; dk[1][r] *= a.scale; }
    csl += __shfl_xor(csl, 32, 64);
    if (lh == 0) Cs[key] = csl * a.scale;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();                                         // S2: all read-modify-writes are done; Cs is complete
    // the next item's Q rows of THIS wave's tile: 4 LDS-DMA pieces (the loader's serial path between S2 and S0 was the
    // bottleneck with all 28 pieces; here they are issued by 7 waves at once and land during the output phase)
    if (item + (int)gridDim.x < nitems) {
      const int bn = nxt_item / a.H, hn = nxt_item - bn * a.H;
      const bf16_t* Qn = a.Q + bn * a.q_sb + (int64_t)hn * a.hd;
      const int lr = lane >> 3, c = lane & 7;
#pragma unroll
      for (int p4 = 0; p4 < 4; ++p4) {
        const int r = k0 + p4 * 8 + lr;                      // k0 + tileimg::piece_row(p4, lane); as a call it changes this kernel's code
        int cc = tileimg::piece_chunk(r, c);
        if (cc * 8 >= a.hd) cc = 0;                          // tileimg::clamp_chunk; as a call it changes this kernel's code
        dma16(Qn, (uint32_t)(((int64_t)tileimg::clamp_row(r, T) * a.q_st + cc * 8) * 2), lds0 + (uint32_t)(Qt - smem_bwd) + (uint32_t)(k0 + p4 * 8) * ROWB);
      }
    }
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
    put_tile(myacc, dk);                                     // the loader stores them once all waves have parked theirs
    put_tile(myacc + 4096, dv);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) __hip_atomic_fetch_add(const_cast<int*>(Flag + 8), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // "S3"
    // dQ tile -> global through the wave's 2-KB scratch, one 32-column half at a time (the scratch image, swz64).
    // (Tried: dK and dV the same way, the loader only loading - 12 stores per compute wave: 305 vs
    // 292 us; the 84 stores of the compute waves and the loader's Q DMA then meet in the same phase of the item.)
    {
      bf16_t* dQp = a.dQ + b * a.dq_sb + (int64_t)h * a.hd;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          u32x2 t;
          t[0] = pack2bf(dq[dt][rg * 4 + 0], dq[dt][rg * 4 + 1]);
          t[1] = pack2bf(dq[dt][rg * 4 + 2], dq[dt][rg * 4 + 3]);
          *reinterpret_cast<u32x2*>(scr + swz64(li, tileimg::park_col(0, rg, lh))) = t;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const int idx = it * 64 + lane, r = idx >> 2, c4 = idx & 3;       // 32 rows x 4 chunks of 16 bytes
          const u32x4 v = *reinterpret_cast<const u32x4*>(scr + swz64(r, c4 * 8));
          if (k0 + r < T && dt * 32 + c4 * 8 < a.hd) *reinterpret_cast<u32x4*>(dQp + (int64_t)(k0 + r) * a.dq_st + dt * 32 + c4 * 8) = v;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
      }
    }
    // token sums of dQ: sum_q dQ[q][d] = sum_key K[key][d] cs[key]: one more product on the matrix pipe (attention_sp.inc)
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
          for (int r = 0; r < 16; ++r) Red[wave * 64 + dt * 32 + 8 * (r >> 2) + 4 * lh + (r & 3)] = cq[dt][r];   // acc_row(r, lh); as a call it changes this kernel's code
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    cur ^= 1;
  }
  __syncthreads();                                           // final S0 (the loader writes the last item's token sums behind it)
}
