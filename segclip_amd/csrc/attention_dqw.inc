// ------------------------------- streaming backward with a dQ wave, unmasked self-attention, head_dim 64 -------------
// Included by attention.hip inside its anonymous namespace (round 6).  Reference: modules/module_seg_vit.py:189 (the
// nn.MultiheadAttention of a vision ResidualAttentionBlock, backward).
//
// attention_spl.inc keeps a whole (batch, head) item in LDS and every key-owner wave read-modify-writes the fp32 dQ
// accumulators of the query tile it visits behind a flag ring: a (query tile, key tile) pair is one dependent chain of ~10 LDS
// round trips, 5 MFMA groups and a neighbour hand-shake (4000 cycles for 640 cycles of matrix-pipe time, MFMA busy 14 %).
// Here
//   * the QUERY TILES of all items of a workgroup are one stream g = 0, 1, 2 ...: Q, dO and O rows of tile g + 3 arrive by
//     LDS-DMA in a 4-slot ring while tile g is computed, across item boundaries; K and V of the next item land in their own
//     areas during the item;
//   * the NT key-owner waves all work on tile g in step g ; each parks its dS^T tile (bf16, 2 KB) in a double-buffered scratch;
//   * ONE EXTRA WAVE owns dQ: in step g it multiplies the dS^T tiles of tile g - 1 by the item's K^T, which it keeps IN
//     REGISTERS (NT x 16 registers) - 4 NT MFMAs, one accumulate chain per 32-column half, no fp32 accumulators in LDS, no
//     read-modify-write, no flags - and stores the bf16 tile as whole rows;
//   * WHO issues a vector-memory instruction matters more than how many there are: a CU retires only ~12 B/clk of loads and ~7 B/clk
//     of stores, and a wave that issues into the backed-up queue stalls for it.  First version, everything issued by the dQ wave
//     (LDS-DMA pieces, D pass, K / V, a burst of 56 dK / dV stores per item): it became the critical path.  Second version, everything
//     spread over the key-owners (2 tile pieces per step each): fitted over the 7-step and 19-step units of the two instantiations,
//     every instruction of a key-owner costs ~600 cycles of step time - the stall sits in the middle of the wave's dependent chain.
//     Now: the dQ wave (idle for two thirds of a step) issues ALL 13 pieces of tile g + 3 in one batch right behind the step's barrier
//     (100-150 cycles each) and its own 4 row stores; a key-owner issues only the 8 pieces of ITS OWN K / V rows of the next item and
//     the 8 row groups of its dK / dV tiles, which are parked as bf16 in the wave's own (dead) K / V rows and leave two 1-KB groups per
//     step during the next item's first four steps.  Every wave counts what it issued (s_waitcnt vmcnt(n) at the end of a step waits
//     for exactly what was issued before that step).  D = rowsum(dO * O) (v_dot2c_f32_bf16) of tile g + 1 is computed by waves 0-3
//     (8 rows each), its log2-domain lse by wave 4;
//   * one s_barrier per step is the only synchronisation.  The end of an item is folded into step 0 of the next: the dQ wave finishes
//     the last tile with the old K^T and takes the new one out of KN while the key-owners run S / dP / softmax of the step; they park
//     the finished dK in their K rows behind one extra barrier in the middle of that step (dV is parked at the end of the item).
// Token sums (in_proj bias gradient) ride on padded rows: the key-owner of the last key tile sets P = 1 on the padded key
// T (its dV^T column becomes sum_q dO[q]); in the last query tile every key-owner writes cs[key] = sum_q dS[q][key] (split
// into two bf16 parts) into the padded query columns T, T + 1 of its dS^T tile, so that the dQ wave's product delivers
// sum_key K[key] cs[key] = sum_q dQ[q] in those two columns.  Hence T mod 32 in [1, 30] (host-checked; T = 196: 4).
// LDS (NT = 7): K 28 KB + V 28 + ring 4 x 12.5 + dS^T scratch 28 + dQ patch 4 + sums: 139 KB, one workgroup per CU.
constexpr int DQW_PF = 3;                                   // tiles in flight ahead of the step
constexpr int DQW_NS = DQW_PF + 1;                          // ring slots
constexpr int DQW_SLOT = 3 * 4096 + 256 + 128 + 128;        // Q | dO | O | lse as loaded (64 f32) | lse * log2 e (32) | D (32)

template <int NT> __host__ __device__ constexpr size_t bwd_dqw_lds_bytes() {
  return (size_t)2 * NT * 32 * ROWB + (size_t)DQW_NS * DQW_SLOT + (size_t)2 * NT * SP_SCR_BYTES + 4096 + 3 * 64 * 4 + 64;
}

// stores of the dQ wave, from inline asm: hipcc must not see a vector-memory instruction in that wave (it would place its
// own s_waitcnt vmcnt in front of register reuses and drain the tiles in flight); the software count below includes them.
// (s_nop 1: a 16-byte store reads its data registers for two more cycles, a hazard hipcc only pads for its own stores.)
__device__ __forceinline__ void dqw_store16(void* base_uniform, uint32_t off, const u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(off), "v"(v), "s"(base_uniform) : "memory");
}
__device__ __forceinline__ void dqw_store4(void* base_uniform, uint32_t off, const float v) {
  asm volatile("global_store_dword %0, %1, %2\n\ts_nop 0" : : "v"(off), "v"(v), "s"(base_uniform) : "memory");
}
// MULTI (sequences of more than NT * 32 tokens; ViT-L/14@336: 577): the work unit is (item, CHUNK of NT * 32 keys).  The key-owners hold
// the chunk's K / V fragments and stream ALL NQ = ceil(T / 32) query tiles past them (Q, dO, O are re-streamed once per chunk:
// NC x the reads, still ~1/10 of a CU's load rate); dK / dV of the chunk are final at the end of the unit and leave as for an
// item.  dQ of a query tile is the sum over the chunks: the dQ wave keeps it as fp32 accumulator registers in a per-workgroup
// global workspace (8 KB per query tile: stored by chunk 0, load-add-stored by the middle chunks, load-added and written out as
// bf16 rows by the last chunk; L2-resident, 3 x 8 KB per 7300-cycle step).  The padded-key column (sum of dO) lives in the last
// chunk; the padded-query columns of the last tile (cs[key] parts) accumulate through the workspace like the rest of dQ.
template <int NT, bool MULTI>
__global__ __launch_bounds__((NT + 1) * 64) void attn_bwd_dqw_bf16_kernel(BwdArgs a) {
  static_assert(NT == 7, "the flush / K / V schedule below is written for 7 steps per item");
  // who issues the 13 Q / dO / O / lse pieces of a ring tile: the dQ wave in one batch (same-box T = 196: 222 us against 245-257 with
  // two pieces per key-owner and step), or the key-owners (MULTI: the dQ wave also moves the fp32 workspace tiles and waits for them;
  // T = 576: 1095 against 1135 us)
  constexpr bool RING_DQ = !MULTI;
  extern __shared__ __attribute__((aligned(16))) char smem_bwd[];
  constexpr int TP = NT * 32;
  const int T = a.Tq;                                        // == Tk; !MULTI: (NT - 1) * 32 < T < NT * 32 - 1
  // query tiles (steps) per unit.  MULTI: the last tile always has two padded rows for the cs[key] parts - a sequence of a multiple
  // of 32 tokens (ViT-L/14@336 without a class token: 576) gets one all-padded tile (lse = inf: P = 0) per unit for them
  const int NQ = MULTI ? (T + 32) >> 5 : NT;
  const int NC = MULTI ? (T + TP - 1) / TP : 1;              // key chunks per item
  const int qp = T - (NQ - 1) * 32;                          // first padded row of the last query tile: 1..30 (MULTI: 0..30)
  const int kl = T - (NC - 1) * TP;                          // the padded key T inside the last chunk (!MULTI: T)
  const int wsum = MULTI ? kl >> 5 : NT - 1, lsum = MULTI ? (kl & 31) : qp;   // its key-owner wave and lane
  char* KN = smem_bwd;                                       // K of the item whose fragments are taken next, TP rows; then dK on its way out
  char* VN = KN + TP * ROWB;                                 // V likewise; then dV on its way out
  char* Ring = VN + TP * ROWB;                               // [DQW_NS] slots
  char* Scr = Ring + DQW_NS * DQW_SLOT;                      // [2][NT][2 KB] dS^T tiles
  char* Pat = Scr + 2 * NT * SP_SCR_BYTES;                   // dQ tile on its way out
  float* Red = reinterpret_cast<float*>(Pat + 4096);         // [3][64]: columns T, T+1 of the last dQ^T tile; token sums of dO
  const uint32_t lds0 = (uint32_t)(uintptr_t)((lds_void*)smem_bwd);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nitems = a.nitems;
  const int nloc = ((int)blockIdx.x < nitems) ? (nitems - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;   // items of this workgroup
  const int nunits = nloc * NC;                              // (item, chunk) units of this workgroup
  const int ntiles = nunits * NQ;

  {  // everything a fragment read may find must be finite
    const int total16 = (int)(bwd_dqw_lds_bytes<NT>() >> 4);
    for (int i = threadIdx.x; i < total16; i += (NT + 1) * 64) reinterpret_cast<u32x4*>(smem_bwd)[i] = u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();
  if (nloc == 0) return;
  // The kernel arguments as a LANE TABLE: lane l of `atab` holds dword l of the argument struct (62 dwords), an argument is read
  // with v_readlane where it is used.  Left to itself hipcc re-reads an argument from the argument segment at every use inside the
  // loops (s_load + s_waitcnt lgkmcnt(0): ~250 cycles each, up to three dependent ones in front of a single LDS-DMA piece, and the
  // wave's LDS reads in flight drain with every one of them); pinned in scalar registers the ~40 values spill.
  static_assert(sizeof(BwdArgs) <= 256, "the argument table is one register");
  uint32_t atab;
  {
    typedef __attribute__((address_space(4))) const uint32_t dqw_karg_t;
    dqw_karg_t* kp = (dqw_karg_t*)__builtin_amdgcn_kernarg_segment_ptr();
    const int l_ = (int)(threadIdx.x & 63);
    atab = kp[l_ < (int)(sizeof(BwdArgs) / 4) ? l_ : 0];
    asm volatile("" : "+v"(atab));
  }
#define DQW_ARG32(f) ((uint32_t)__builtin_amdgcn_readlane((int)atab, (int)(offsetof(BwdArgs, f) / 4)))
#define DQW_ARG64(f) ((int64_t)((uint64_t)DQW_ARG32(f) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)atab, (int)(offsetof(BwdArgs, f) / 4 + 1)) << 32)))
#define DQW_ARGP(type, f) (reinterpret_cast<type*>((uintptr_t)DQW_ARG64(f)))

#define aQ DQW_ARGP(const bf16_t, Q)
#define aG DQW_ARGP(const bf16_t, dO)
#define aO DQW_ARGP(const bf16_t, O)
#define aL DQW_ARGP(const float, lse)
#define q_sb DQW_ARG64(q_sb)
#define g_sb DQW_ARG64(do_sb)
#define o_sb DQW_ARG64(o_sb)
#define q_st ((int)DQW_ARG32(q_st))
#define g_st ((int)DQW_ARG32(do_st))
#define o_st ((int)DQW_ARG32(o_st))
#define aH ((int)DQW_ARG32(H))
  if (wave == NT) {
    // ================================================ dQ wave ================================================
    const int lane = threadIdx.x & 63, lr = lane >> 3, c = lane & 7, li = lane & 31, lh = lane >> 5;
    int lro = lr, co = c, lio = li;                          // re-derived per step from an opaque copy of the lane id (issue_tile: see the key-owners)
    // kernel arguments used in the loop come from the lane table `atab` (see below)
#define adQ DQW_ARGP(bf16_t, dQ)
#define acs DQW_ARGP(float, colsum_part)
#define dq_sb DQW_ARG64(dq_sb)
#define dq_st ((int)DQW_ARG32(dq_st))
    const float ascale = a.scale;
    int ib = 0, ih = 0;                                      // (batch, head) of the item being worked on
    int ibN = 0, ihN = 0;                                    // ... of the next unit
    uint32_t nvmq = 0;                                       // vector-memory instructions this wave issued in the current step
    // ---- the Q / dO / O / lse pieces of the ring: ALL 13 of a tile are issued by this wave, in one batch right behind the step's
    // barrier.  (Second version: two pieces per key-owner and step.  Fitted over the 7-step and the 19-step units of the two variants,
    // every vector-memory instruction of a key-owner costs ~600 cycles of STEP time - its issue stalls the wave in the middle of its
    // dependent chain - while this wave idles for two thirds of a step and pays ~100-150 cycles per instruction of a batch.)
    auto ring_src = [&](int r, uint32_t st) {                // source chunk of (row r, LDS chunk lane & 7): the tiles' swizzle
      return (uint32_t)(((uint32_t)tileimg::clamp_row(r, T) * st + (uint32_t)(tileimg::piece_chunk(r, co) * 8)) * 2u);
    };
    auto issue_tile = [&](int t, int unC) {                  // unC: the unit (ib, ih) belongs to
      const bool nx = t >= (unC + 1) * NQ;                   // (tile t belongs to the current or to the next unit)
      const int j = t - (nx ? unC + 1 : unC) * NQ;
      const int b = nx ? ibN : ib, h = nx ? ihN : ih;
      const uint32_t slot = lds0 + (uint32_t)(Ring - smem_bwd) + (uint32_t)(t % DQW_NS) * DQW_SLOT;
#pragma unroll
      for (int kind = 0; kind < 3; ++kind) {
        const bf16_t* base = (kind == 0 ? aQ + b * q_sb : (kind == 1 ? aG + b * g_sb : aO + b * o_sb)) + (int64_t)h * 64;
        const uint32_t st = (uint32_t)(kind == 0 ? q_st : (kind == 1 ? g_st : o_st));
#pragma unroll
        for (int u = 0; u < 4; ++u) dma16(base, ring_src(j * 32 + u * 8 + lro, st), slot + (uint32_t)(kind * 4096 + u * 1024));
      }
      const int q = j * 32 + lio;
      dma4(aL + ((int64_t)b * aH + h) * T, (uint32_t)((q < T ? q : T - 1) * 4), slot + 12288);
      nvmq += 13;
    };
    auto set_next = [&](int un) {                            // (ibN, ihN) of unit un
      const int il = MULTI ? un / NC : un;
      const int item = (int)blockIdx.x + il * (int)gridDim.x;
      ibN = item / aH; ihN = item - ibN * aH;
    };
    // K^T fragments of the item in KN: ktr[kw][dt][hf]: lane -> d = dt*32 + (l&31), keys kw*32 + 16*hf + 4*(l>>5) + {0..3, 8..11}
    bf16x8_t ktr[NT][2][2];
    int toff[2][2];
    {
      const int g4 = lane >> 4, q = lane & 15;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) toff[dt][jj] = TR_LANE_OFF(g4, q, dt, jj);
    }
    auto load_ktr = [&](int kbase) {                         // kbase: first key of the chunk in KN
      int lhk = lane >> 5;
      asm volatile("" : "+v"(lhk));                          // (MULTI: the 28 lane-dependent key indices of the masks are not to be hoisted and spilled)
#pragma unroll
      for (int kw = 0; kw < NT; ++kw)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            u32x4 f = __builtin_bit_cast(u32x4, tr16_frag(KN + (kw * 32 + hf * 16) * ROWB, toff[dt][0], toff[dt][1]));
            if (MULTI || kw == NT - 1) {                     // keys beyond T (clamped duplicates / stale rows) count as zero rows
              const int kb = kbase + kw * 32 + hf * 16 + 4 * lhk;
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) {
                const int ka = kb + (jj & 1) * 2 + (jj >> 1) * 8;   // register jj holds keys ka, ka + 1
                f[jj] &= (ka < T ? 0x0000ffffu : 0u) | (ka + 1 < T ? 0xffff0000u : 0u);
              }
            }
            ktr[kw][dt][hf] = __builtin_bit_cast(bf16x8_t, f);
          }
    };
    // lane offset of the dS^T fragments inside a 2-KB scratch tile (frag_tr64): rows r0, r0 + 8, r0 + 16, r0 + 24 are + 512 bytes each
    const int soff = tileimg::frag_tr64_at(0, lane, 0);
    auto sfrag = [&](const char* t, int r16) { return tr16_frag(t + soff + r16 * 1024, 512); };
    // dQ^T of tile t: one product over all keys; the bf16 tile -> patch -> global as whole 128-byte rows
    auto product = [&](int t, int jt, int cch, int b, int h) {
      f32x16 dq[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
      const char* sbase = Scr + (t & 1) * NT * SP_SCR_BYTES;
#pragma unroll
      for (int kw = 0; kw < NT; ++kw) {
        const bf16x8_t st0 = sfrag(sbase + kw * SP_SCR_BYTES, 0), st1 = sfrag(sbase + kw * SP_SCR_BYTES, 1);
        dq[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[kw][0][0], st0, dq[0], 0, 0, 0);
        dq[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[kw][1][0], st0, dq[1], 0, 0, 0);
        dq[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[kw][0][1], st1, dq[0], 0, 0, 0);
        dq[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[kw][1][1], st1, dq[1], 0, 0, 0);
      }
      if (MULTI) {
        // the tile's fp32 accumulators across the chunks of the item: [workgroup][query tile][8 register quads][64 lanes]
        float* wsp = DQW_ARGP(float, ws) + ((int64_t)blockIdx.x * NQ + jt) * 2048 + lane * 4;
        if (cch > 0) {
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              const f32x4 pv = *reinterpret_cast<const f32x4*>(wsp + (dt * 4 + rg) * 256);
#pragma unroll
              for (int u = 0; u < 4; ++u) dq[dt][rg * 4 + u] += pv[u];
            }
        }
        if (cch < NC - 1) {
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
              *reinterpret_cast<f32x4*>(wsp + (dt * 4 + rg) * 256) = f32x4{dq[dt][rg * 4], dq[dt][rg * 4 + 1], dq[dt][rg * 4 + 2], dq[dt][rg * 4 + 3]};
          nvmq += 8;
          return;
        }
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          u32x2 w;
          w[0] = pack2bf(dq[dt][rg * 4 + 0] * ascale, dq[dt][rg * 4 + 1] * ascale);
          w[1] = pack2bf(dq[dt][rg * 4 + 2] * ascale, dq[dt][rg * 4 + 3] * ascale);
          *reinterpret_cast<u32x2*>(Pat + swz(li, tileimg::park_col(dt, rg, lh))) = w;
        }
      if (jt == NQ - 1 && (li == qp || li == qp + 1)) {      // columns T, T + 1: the two bf16 parts of sum_key K[key] cs[key]
        float* dst = Red + (li - qp) * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) dst[dt * 32 + acc_row(r, lh)] = dq[dt][r];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      {
        bf16_t* dQp = adQ + b * dq_sb + (int64_t)h * 64;
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const u32x4*>(Pat + swz(u * 8 + lr, c * 8));
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (jt * 32 + u * 8 < T) {                         // (wave-uniform: the software vmcnt counts what is really issued)
            const int r = jt * 32 + u * 8 + lr;
            if (r < T) dqw_store16(dQp, (uint32_t)((r * dq_st + c * 8) * 2), v[u]);
            ++nvmq;
          }
      }
      if (jt == NQ - 1 && acs) {                             // token sums of dQ | dK | dV of the item
        float* dst = acs + (int64_t)b * 3 * ((int64_t)aH * 64) + (int64_t)h * 64;
        const float vq = (Red[lane] + Red[64 + lane]) * ascale;
        const float vv = Red[128 + lane];
        dqw_store4(dst, (uint32_t)(lane * 4), vq);
        dqw_store4(dst, (uint32_t)((aH * 64 + lane) * 4), 0.f);   // rows of dS sum to zero: the token sums of dK are exactly 0
        dqw_store4(dst, (uint32_t)((2 * aH * 64 + lane) * 4), vv);
        nvmq += 3;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the patch / Red have been read
    };

    // prologue: the first DQW_PF tiles
    set_next(0);
    ib = ibN; ih = ihN;
    if (nunits > 1) set_next(1);
    if (RING_DQ)
      for (int t = 0; t < DQW_PF && t < ntiles; ++t) issue_tile(t, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                            // B_P: K of the first item has landed
    load_ktr(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int cch = 0;
    for (int un = 0; un < nunits; ++un) {
      const int ibP = ib, ihP = ih, cchP = cch;              // the unit whose last tile is still to be finished
      const int il = MULTI ? un / NC : un;
      cch = MULTI ? un - il * NC : 0;
      if (un > 0) {
        ib = ibN; ih = ihN;
        if (un + 1 < nunits) set_next(un + 1);
      }
      for (int j = 0; j < NQ; ++j) {
        __builtin_amdgcn_s_barrier();                        // B_g
        nvmq = 0;
        {
          int lane_o = lane;
          asm volatile("" : "+v"(lane_o));
          lro = lane_o >> 3; co = lane_o & 7; lio = lane_o & 31;
        }
        if (RING_DQ && un * NQ + j + DQW_PF < ntiles) issue_tile(un * NQ + j + DQW_PF, un);
        if (j >= 1) {
          product(un * NQ + j - 1, j - 1, cch, ib, ih);
        } else if (un > 0) {
          // the previous unit's last tile with the OLD K^T, then this unit's K^T out of KN - under the key-owners' S / dP / softmax of
          // the step; they park the previous unit's dK in those rows behind the barrier K.  (First version: an extra barrier at the end
          // of a unit, this product and the reload behind it while the key-owners waited: ~2300 exposed cycles per unit)
          product(un * NQ - 1, NQ - 1, cchP, ibP, ihP);
          load_ktr(MULTI ? cch * TP : 0);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();                      // K
        }
        if (RING_DQ) wait_vm(nvmq);                          // what this wave issued BEFORE this step has landed / left
      }
    }
    __builtin_amdgcn_s_barrier();                            // F: the last dS^T tiles are parked
    product(ntiles - 1, NQ - 1, cch, ib, ih);
#undef adQ
#undef acs
#undef dq_sb
#undef dq_st
    return;
  }

  // ================================================ key-owner waves ================================================
  // (measured: s_setprio 1 for key-owners 4-6 - the second-dispatched half - leaves the ratio to the round-5 kernel at 0.90)
  const int k0 = wave * 32;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, li = lane & 31, lh = lane >> 5, key = k0 + li;
  // the lane parts the memory-issue code uses are re-derived per step from an OPAQUE copy of the lane id: as loop invariants their
  // address arithmetic was hoisted out of the step loop and spilled (38 registers; a scratch reload is a vector-memory instruction
  // - hipcc waits for it with vmcnt(0), i.e. for every LDS-DMA piece in flight)
  int lr = lane >> 3, c = lane & 7, lic = lane & 31, lho = lane >> 5;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const int R = (T + 7) & ~7;                                // rows of a K / V tile that are loaded
  // kernel arguments used in the loop come from the lane table `atab`
#define aK DQW_ARGP(const bf16_t, K)
#define aV DQW_ARGP(const bf16_t, V)
#define adK DQW_ARGP(bf16_t, dK)
#define adV DQW_ARGP(bf16_t, dV)
#define k_sb DQW_ARG64(k_sb)
#define v_sb DQW_ARG64(v_sb)
#define dk_sb DQW_ARG64(dk_sb)
#define dv_sb DQW_ARG64(dv_sb)
#define k_st ((int)DQW_ARG32(k_st))
#define v_st ((int)DQW_ARG32(v_st))
#define dk_st ((int)DQW_ARG32(dk_st))
#define dv_st ((int)DQW_ARG32(dv_st))
  const float ascale = a.scale;
  // (batch, head) of the previous / current / next local item (one scalar division per item instead of one per memory instruction)
  // (MULTI: plus the key chunk of the unit; cX * TP is the first key of the chunk)
  int bP = 0, hP = 0, bC = 0, hC = 0, bN = 0, hN = 0, cP = 0, cC = 0, cN = 0;
  auto set_bh = [&](int un, int& b, int& h, int& cc) {
    const int il = MULTI ? un / NC : un;
    const int item = (int)blockIdx.x + il * (int)gridDim.x;
    b = item / aH; h = item - b * aH;
    cc = MULTI ? un - il * NC : 0;
  };
  set_bh(0, bC, hC, cC);
  if (nunits > 1) set_bh(1, bN, hN, cN);
  int ilC = 0;                                               // the local unit (bC, hC, cC) belongs to
  auto src_off = [&](int r, uint32_t st) {                   // source chunk of (row r, LDS chunk lane & 7): the tiles' swizzle
    return (uint32_t)(((uint32_t)tileimg::clamp_row(r, T) * st + (uint32_t)(tileimg::piece_chunk(r, c) * 8)) * 2u);
  };
  uint32_t nvm = 0;                                          // vector-memory instructions this wave issued in the current step
  // !RING_DQ: piece idx of tile t: 0-3 Q rows, 4-7 dO rows, 8-11 O rows (8 rows each), 12 lse
  auto issue_piece = [&](int t, int idx) {
    const int il = MULTI ? (t >= (ilC + 1) * NQ ? ilC + 1 : ilC) : t / NT, j = t - il * NQ;
    const int b = il == ilC ? bC : bN, h = il == ilC ? hC : hN;   // (tile t belongs to the current or to the next unit)
    const uint32_t slot = lds0 + (uint32_t)(Ring - smem_bwd) + (uint32_t)(t % DQW_NS) * DQW_SLOT;
    if (idx < 12) {
      const int kind = idx >> 2, u = idx & 3;
      const bf16_t* base = kind == 0 ? aQ + b * q_sb : (kind == 1 ? aG + b * g_sb : aO + b * o_sb);
      const uint32_t st = (uint32_t)(kind == 0 ? q_st : (kind == 1 ? g_st : o_st));
      dma16(base + (int64_t)h * 64, src_off(j * 32 + u * 8 + lr, st), slot + (uint32_t)(kind * 4096 + u * 1024));
    } else {
      const int q = j * 32 + lic;
      dma4(aL + ((int64_t)b * aH + h) * T, (uint32_t)((q < T ? q : T - 1) * 4), slot + 12288);
    }
    ++nvm;
  };
  auto issue_tile_share = [&](int t) {
    issue_piece(t, wave);
    if (wave + NT < 13) issue_piece(t, wave + NT);
  };
  // 8-row pieces u0 .. u1-1 of this wave's own K (which = 0) / V (1) rows of local item il -> KN / VN
  auto issue_own_kv = [&](int b, int h, int cch, int which, int u0, int u1) {
    const bf16_t* base = (which == 0 ? aK + b * k_sb : aV + b * v_sb) + (int64_t)h * 64;
    const uint32_t st = (uint32_t)(which == 0 ? k_st : v_st);
    const int kb = MULTI ? cch * TP + k0 : k0;               // first global key row of this wave
    for (int u = u0; u < u1; ++u)
      if (kb + u * 8 < R) {                                  // (wave-uniform; rows beyond R are never read unmasked)
        dma16(base, src_off(kb + u * 8 + lr, st), lds0 + (uint32_t)(which * TP * ROWB) + (uint32_t)((k0 + u * 8) * ROWB));
        ++nvm;
      }
  };
  // 8-row groups u0 .. u1-1 of the parked dK (which = 0) / dV (1) tile of local item il -> global, whole 128-byte rows
  auto store_groups = [&](int b, int h, int cch, int which, int u0, int u1) {
    bf16_t* base = (which == 0 ? adK + b * dk_sb : adV + b * dv_sb) + (int64_t)h * 64;
    const int st = which == 0 ? dk_st : dv_st;
    const char* tile = (which == 0 ? KN : VN) + k0 * ROWB;
    const int kb = MULTI ? cch * TP + k0 : k0;               // first global key row of this wave
    for (int u = u0; u < u1; ++u)
      if (kb + u * 8 < T) {                                  // (wave-uniform: the software vmcnt counts what is really issued)
        const int r = u * 8 + lr;
        const u32x4 v = *reinterpret_cast<const u32x4*>(tile + swz(r, c * 8));
        if (kb + r < T) dqw_store16(base, (uint32_t)(((kb + r) * st + c * 8) * 2), v);
        ++nvm;
      }
  };
  auto put_tile = [&](char* tile, const f32x16 (&acc)[2], float mul) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        u32x2 w;
        w[0] = pack2bf(acc[dt][rg * 4 + 0] * mul, acc[dt][rg * 4 + 1] * mul);
        w[1] = pack2bf(acc[dt][rg * 4 + 2] * mul, acc[dt][rg * 4 + 3] * mul);
        *reinterpret_cast<u32x2*>(tile + swz(li, tileimg::park_col(dt, rg, lh))) = w;
      }
  };
  // D = rowsum(dO * O) of rows 8 wave .. 8 wave + 7 of tile t (waves 0-3) / its log2-domain lse (wave 4) -> the slot's vectors
  auto dpass_share = [&](int t) {
    const int jt = MULTI ? (t >= (ilC + 1) * NQ ? t - (ilC + 1) * NQ : t - ilC * NQ) : t % NT;
    char* sl = Ring + (t % DQW_NS) * DQW_SLOT;
    float* Lraw = reinterpret_cast<float*>(sl + 12288);
    if (wave < 4) {
      const u32x4 gv = *reinterpret_cast<const u32x4*>(sl + 4096 + (wave * 8 + lr) * ROWB + c * 16);   // (the swizzle permutes the
      const u32x4 ov = *reinterpret_cast<const u32x4*>(sl + 8192 + (wave * 8 + lr) * ROWB + c * 16);   //  chunks of a row alike in both tiles)
      // (from inline asm: __builtin_amdgcn_fdot2_f32_bf16 on the elements of a loaded vector came out of hipcc 7.2 as four
      // v_dot2c of the SAME element pair.  A dot instruction may feed the next one's accumulator back to back; a different
      // VALU instruction reading its result needs 3 wait states, which hipcc cannot see behind an asm statement.)
      float sdot = 0.f;
      asm volatile("v_dot2c_f32_bf16 %0, %1, %5\n\tv_dot2c_f32_bf16 %0, %2, %6\n\tv_dot2c_f32_bf16 %0, %3, %7\n\t"
                   "v_dot2c_f32_bf16 %0, %4, %8\n\ts_nop 3"
                   : "+v"(sdot)
                   : "v"(gv[0]), "v"(gv[1]), "v"(gv[2]), "v"(gv[3]), "v"(ov[0]), "v"(ov[1]), "v"(ov[2]), "v"(ov[3]));
      // sum over the row's 8 lanes on the VALU (DPP: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror)
      sdot += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(sdot), 0xB1, 0xf, 0xf, true));
      sdot += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(sdot), 0x4E, 0xf, 0xf, true));
      sdot += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(sdot), 0x141, 0xf, 0xf, true));
      if (c == 0) Lraw[96 + wave * 8 + lr] = sdot;
    } else if (wave == 4) {
      const float lse_r = Lraw[lic];
      if (lr < 4) Lraw[64 + lic] = (jt * 32 + lic < T) ? lse_r * 1.4426950408889634f : INFINITY;   // padded rows: P = 0
    }
  };

  // ---- prologue: this wave's K / V rows of the first item and its share of the first DQW_PF tiles
  issue_own_kv(bC, hC, 0, 0, 0, 4);
  issue_own_kv(bC, hC, 0, 1, 0, 4);
  if (!RING_DQ)
    for (int t = 0; t < DQW_PF && t < ntiles; ++t) issue_tile_share(t);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                              // B_P

  int koff[4], toff[2][2], woff[4];
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) koff[kc] = swz(li, tileimg::frag_rows_col(kc, lh));
  {
    const int g4 = lane >> 4, q = lane & 15;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) toff[dt][jj] = TR_LANE_OFF(g4, q, dt, jj);
  }
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) woff[rg] = swz64(li, tileimg::park_col(0, rg, lh));
  bf16x8_t kf[4], vf[4];
  auto load_kv = [&](int cch) {
    const bool rok = (MULTI ? cch * TP + key : key) < T;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      int ko = koff[kc];
      asm volatile("" : "+v"(ko));                           // (the four hoisted sums KN + k0 * ROWB + koff[kc] were spilled: a scratch reload
                                                             //  is a vector-memory instruction, hipcc drains vmcnt behind it)
      const u32x4 kraw = *reinterpret_cast<const u32x4*>(KN + k0 * ROWB + ko);
      const u32x4 vraw = *reinterpret_cast<const u32x4*>(VN + k0 * ROWB + ko);
      kf[kc] = __builtin_bit_cast(bf16x8_t, rok ? kraw : zero4);
      vf[kc] = __builtin_bit_cast(bf16x8_t, rok ? vraw : zero4);
    }
  };
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }
  float csl = 0.f;
  const float sc2 = ascale * 1.4426950408889634f;

  load_kv(0);
  dpass_share(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int uS = 0, jS = 0;                                        // MULTI: (unit, step) of tile g without a division by NQ
  for (int g = 0; g < ntiles; ++g) {
    __builtin_amdgcn_s_barrier();                            // B_g
    const int il = MULTI ? uS : g / NT, j = MULTI ? jS : g - il * NT;   // il: the local UNIT (MULTI: (item, chunk)) of tile g
    nvm = 0;
    {
      int lane_o = lane;
      asm volatile("" : "+v"(lane_o));
      lr = lane_o >> 3; c = lane_o & 7; lic = lane_o & 31; lho = lane_o >> 5;
    }
    if (il > 0 && j == 0) {
      bP = bC; hP = hC; cP = cC; bC = bN; hC = hN; cC = cN; ilC = il;
      if (il + 1 < nunits) set_bh(il + 1, bN, hN, cN);
      csl = 0.f;                                             // (the previous unit's dK stays in its registers until barrier K below)
    }
    // this wave's memory instructions of the step.  They are issued at one of four places of the step, by wave index: issued by all
    // waves right behind the barrier they queue up behind each other (~470 cycles per instruction and wave: 2000 cycles per step
    // in which no wave computes)
    auto mem_issue = [&]() {
      if (!RING_DQ && g + DQW_PF < ntiles) issue_tile_share(g + DQW_PF);
      if (il > 0) {                                          // the previous item's parked gradients: two row groups per step
        // (dV was parked at the end of the unit, dK is parked in the middle of step 0)
        if (j == 0) store_groups(bP, hP, cP, 1, 0, 2);
        else if (j == 1) store_groups(bP, hP, cP, 1, 2, 4);
        else if (j == 2) store_groups(bP, hP, cP, 0, 0, 2);
        else if (j == 3) store_groups(bP, hP, cP, 0, 2, 4);
      }
      if (il + 1 < nunits) {
        // the next item's V / K rows of this wave, behind the stores that read the parked tiles from the same rows
        if (j == 2 || j == 3) issue_own_kv(bN, hN, cN, 1, (j - 2) * 2, (j - 2) * 2 + 2);
        else if (j == 4) issue_own_kv(bN, hN, cN, 0, 0, 4);
      }
    };
    const int mpos = wave & 3;
    if (mpos == 0) mem_issue();
    // S and dP of THIS tile.  (First version: S / dP of tile g + 1 were issued a step ahead, "so that the matrix pipe has work during
    // the softmax arithmetic".  The 32 registers of the second accumulator pair left hipcc ONE register quad for the eight Q / dO
    // fragments: ds_read_b128 -> s_waitcnt lgkmcnt(0) -> v_mfma, eight times in a row - eight serialised LDS round trips per step.)
    f32x16 s, dp;
    // (Tried: waves 4-6 issue S / dP of the next tile LAST in the step instead of first, so that the two waves of a SIMD are not in
    // their matrix phases and in their softmax arithmetic at the same time: compute alone 193.9 = 191.9 us, the kernel slower.)
    // EVERY LDS read of the step is issued here, in the order of use (the LDS returns a wave's reads in order): the eight Q / dO
    // fragments of S / dP, the sixteen transposed fragments of dV / dK, the row vectors lse / D; the statements that "modify" a group
    // pin where it must have arrived (left to itself hipcc reads and waits one register quad at a time)
    const char* qs = Ring + (g % DQW_NS) * DQW_SLOT;
    const char* gsl = qs + 4096;
    bf16x8_t gtf[2][2], qtf[2][2];
    f32x4 l4v[4], d4v[4];
    {
      const float* Lv = reinterpret_cast<const float*>(qs + 3 * 4096 + 256);
      const float* Dv = Lv + 32;
      bf16x8_t qa[4], ga[4];
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        qa[kc] = *reinterpret_cast<const bf16x8_t*>(qs + koff[kc]);
        ga[kc] = *reinterpret_cast<const bf16x8_t*>(gsl + koff[kc]);
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        gtf[dt][0] = tr16_frag(gsl, toff[dt][0], toff[dt][1]);
        gtf[dt][1] = tr16_frag(gsl + 16 * ROWB, toff[dt][0], toff[dt][1]);
        qtf[dt][0] = tr16_frag(qs, toff[dt][0], toff[dt][1]);
        qtf[dt][1] = tr16_frag(qs + 16 * ROWB, toff[dt][0], toff[dt][1]);
      }
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        l4v[rg] = *reinterpret_cast<const f32x4*>(Lv + 8 * rg + 4 * lh);
        d4v[rg] = *reinterpret_cast<const f32x4*>(Dv + 8 * rg + 4 * lh);
      }
      asm volatile("" : "+v"(qa[0]), "+v"(qa[1]), "+v"(qa[2]), "+v"(qa[3]), "+v"(ga[0]), "+v"(ga[1]), "+v"(ga[2]), "+v"(ga[3]) : : "memory");
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[kc], kf[kc], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[kc], vf[kc], dp, 0, 0, 0);
      }
      if (g + 1 < ntiles) dpass_share(g + 1);
    }
    if (mpos == 1) mem_issue();
    {
      float p[16], ds[16];
      asm volatile("" : "+v"(l4v[0]), "+v"(l4v[1]), "+v"(l4v[2]), "+v"(l4v[3]), "+v"(d4v[0]), "+v"(d4v[1]), "+v"(d4v[2]), "+v"(d4v[3]) : : "memory");
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 l4 = l4v[rg], d4 = d4v[rg];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = rg * 4 + u;
          const float pv = __builtin_amdgcn_exp2f(s[r] * sc2 - l4[u]);
          p[r] = pv;
          ds[r] = pv * (dp[r] - d4[u]);
          csl += ds[r];
        }
      }
      u32x4 pb0 = __builtin_bit_cast(u32x4, pack8(p)), pb1 = __builtin_bit_cast(u32x4, pack8(p + 8));
      const bf16x8_t sb0 = pack8(ds), sb1 = pack8(ds + 8);
      u32x4 w0 = __builtin_bit_cast(u32x4, sb0), w1 = __builtin_bit_cast(u32x4, sb1);
      if (j == NQ - 1) {
        // the padded query columns T, T + 1 of the parked tile carry cs[key] = sum_q dS[q][key] in two bf16 parts
        const float tot = pf_xsum(csl);
        const float hi = __uint_as_float(__float_as_uint(tot) & 0xffff0000u), lo = tot - hi;
        float dw[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = 8 * (r >> 2) + 4 * lh + (r & 3);   // acc_row(r, lh); as a call it changes this kernel's code
          dw[r] = ql == qp ? hi : (ql == qp + 1 ? lo : ds[r]);
        }
        w0 = __builtin_bit_cast(u32x4, pack8(dw));
        w1 = __builtin_bit_cast(u32x4, pack8(dw + 8));
      }
      if (wave == wsum && (!MULTI || cC == NC - 1)) {
        // padded key T: P = 1 on every real query row -> its dV^T column is sum_q dO[q]
        const bool mine = lic == lsum;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          uint32_t one = 0x3F803F80u;
          if (j == NQ - 1) {
            const int r0 = 2 * i, r1 = 2 * i + 1;
            const int q0 = 8 * (r0 >> 2) + 4 * lho + (r0 & 3), q1 = 8 * (r1 >> 2) + 4 * lho + (r1 & 3);   // acc_row; (lho: not hoisted, not spilled)
            one = (q0 < qp ? 0x00003F80u : 0u) | (q1 < qp ? 0x3F800000u : 0u);
          }
          if (i < 4) pb0[i] = mine ? one : pb0[i];
          else pb1[i - 4] = mine ? one : pb1[i - 4];
        }
      }
      {
        char* scr = Scr + ((g & 1) * NT + wave) * SP_SCR_BYTES;
        *reinterpret_cast<u32x2*>(scr + woff[0]) = u32x2{w0[0], w0[1]};
        *reinterpret_cast<u32x2*>(scr + woff[1]) = u32x2{w0[2], w0[3]};
        *reinterpret_cast<u32x2*>(scr + woff[2]) = u32x2{w1[0], w1[1]};
        *reinterpret_cast<u32x2*>(scr + woff[3]) = u32x2{w1[2], w1[3]};
      }
      if (mpos == 2) mem_issue();
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gtf[dt][0], __builtin_bit_cast(bf16x8_t, pb0), dv[dt], 0, 0, 0);
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gtf[dt][1], __builtin_bit_cast(bf16x8_t, pb1), dv[dt], 0, 0, 0);
      }
      if (j == 0 && il > 0) {
        // K: the dQ wave has finished the previous unit's last tile and taken this unit's K^T out of KN: the previous unit's dK leaves
        // its registers for this wave's (now dead) K rows
        __builtin_amdgcn_s_barrier();
        put_tile(KN + k0 * ROWB, dk, ascale);
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; }
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf[dt][0], sb0, dk[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf[dt][1], sb1, dk[dt], 0, 0, 0);
      }
      if (j == NQ - 1 && wave == wsum && li == lsum && (!MULTI || cC == NC - 1)) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) Red[128 + dt * 32 + acc_row(r, lh)] = dv[dt][r];
      }
    }
    if (mpos == 3) mem_issue();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vm(nvm);                                            // what this wave issued BEFORE this step has landed / left
    if (j == NQ - 1) {
      // end of the unit (no barrier: this wave's own rows only)
      if (il + 1 < nunits) load_kv(cN);                       // the next item's K / V fragments, then this wave's V rows are dead
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      put_tile(VN + k0 * ROWB, dv, 1.0f);
#pragma unroll
      for (int r = 0; r < 16; ++r) { dv[0][r] = 0.f; dv[1][r] = 0.f; }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (MULTI) { if (++jS == NQ) { jS = 0; ++uS; } }
  }
  // the last item's gradients (the dQ wave is past its K^T fragments: both tiles leave at once)
  __builtin_amdgcn_s_barrier();                              // F
  put_tile(KN + k0 * ROWB, dk, ascale);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  store_groups(bC, hC, cC, 0, 0, 4);
  store_groups(bC, hC, cC, 1, 0, 4);
#undef aQ
#undef aG
#undef aO
#undef aL
#undef aK
#undef aV
#undef adK
#undef adV
#undef q_sb
#undef g_sb
#undef o_sb
#undef k_sb
#undef v_sb
#undef dk_sb
#undef dv_sb
#undef q_st
#undef g_st
#undef o_st
#undef k_st
#undef v_st
#undef dk_st
#undef dv_st
#undef aH
#undef DQW_ARG32
#undef DQW_ARG64
#undef DQW_ARGP
}
