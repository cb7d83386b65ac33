// ------------------------------- persistent forward, self-attention of 65..96 / 161..200 tokens ---------------------
// Included by attention.hip inside its anonymous namespace (round 5).
//
// The one-workgroup-per-(batch, head) forward above is a latency chain per workgroup: Q/K/V round trip -> LDS staging ->
// barrier -> 7 key tiles -> store drain, and two resident workgroups per CU do not hide it (111 us at B = 256, T = 196,
// H = 12 against an HBM floor of 49 us: 308 MB at 6.3 TB/s; MFMA busy 15 %).  Here the (batch, head) items are a STREAM:
//   * a persistent grid (as many workgroups as the chip holds: one per CU at T = 196) walks the items;
//   * ONE LOADER WAVE per workgroup issues every memory instruction: K, V and Q of item i+1 arrive by LDS-DMA
//     (global_load_lds_dwordx4, 1 KiB per wave instruction; the swizzle of the tiles is applied on the source side) into
//     the other half of a two-slot ring while item i is computed, and O of item i-1 leaves from LDS as whole 128-byte
//     rows.  The NT compute waves (one per 32-row query tile) touch LDS and registers only.  Measured on the way here:
//     with the 12 loads + 5 stores of an item issued by the compute waves themselves, each wave spent 6-9 thousand of
//     its 18 thousand cycles per item stalled IN THE ISSUE of those instructions (the CU's vector-memory path is
//     back-pressured by its own outstanding misses), wherever in the item
//     they were placed (one burst behind the barrier: 103 us; spread over the key steps: 122 us);
//   * one workgroup barrier per item: "item i has landed" (the loader arrives behind its vmcnt(0)) and "every compute
//     wave is done with item i-1" (its slot and its O tile may be recycled).
// Key tiles are processed in PAIRS (64 keys per softmax step: one row maximum, one exchange between the two lanes of a
// row - v_permlane32_swap, not the ds_bpermute of __shfl_xor -, one rescale of the output accumulators, two independent
// MFMA chains); fragment loads are issued in batches.  Rows beyond T come from clamped addresses (finite duplicates) and
// are masked as edge tiles; the K/V tiles hold ceil(T/8)*8 rows, what a fragment read finds behind them is finite by
// construction (zero-initialised LDS, then bf16 data of the neighbouring region) and multiplied by P = 0.
constexpr int PF_QO_BYTES = 4096;          // per compute wave: Q tile, later O tile: [32 rows][128 B]

static inline int pf_kv_rows(int T) { return (T + 7) & ~7; }
static inline size_t fwd_pf_lds_bytes(int n, int T) {
  return (size_t)4 * pf_kv_rows(T) * 128 + (size_t)2 * n * PF_QO_BYTES + (size_t)2 * n * 128;
}

// exchange between the two lanes (l, l + 32) that share a query row, on the VALU.  After the swap of a value with itself
// the two results hold {own, partner} in either order in every lane.
__device__ __forceinline__ float pf_xmax(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float pf_xsum(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <int NT, bool CAUSAL>
__global__ __launch_bounds__((NT + 1) * 64) __attribute__((amdgpu_waves_per_eu(2))) void attn_fwd_pf_kernel(FwdArgs a, int nitems) {
  extern __shared__ __attribute__((aligned(16))) char smem_pf[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int T = a.Tq;                                      // == Tk (host-checked)
  const int R = (T + 7) & ~7;                              // rows of a K / V tile in LDS
  const int TILE = R * ROWB;
  const uint32_t lds0 = (uint32_t)(uintptr_t)((lds_void*)smem_pf);
  // layout: [K0][V0][K1][V1] [QO0: NT x 4 KB][QO1] [lse0: NT x 128 B][lse1]
  const int QO_OFF = 4 * TILE, LSE_OFF = QO_OFF + 2 * NT * PF_QO_BYTES;

  // everything a fragment read may find must be finite: zero the whole allocation once
  {
    const int total16 = (LSE_OFF + 2 * NT * 128) >> 4;
    for (int i = threadIdx.x; i < total16; i += (NT + 1) * 64) reinterpret_cast<u32x4*>(smem_pf)[i] = u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();

  if (wave == NT) {
    // ================================ loader wave ================================
    const int npk = R >> 3;                                // pieces per K / V tile
    const int npq = NT * 4;                                // pieces of the Q buffer (NT x 32 rows)
#include "attention_dma_tile.inc"   // src_off, dma_tile
    auto issue_kv = [&](int item, int slot) {
      const int b = item / a.H, h = item - b * a.H;
      dma_tile(a.K + (int64_t)b * a.k_sb + (int64_t)h * a.hd, a.k_st, npk, lds0 + slot * 2 * TILE);
      dma_tile(a.V + (int64_t)b * a.v_sb + (int64_t)h * a.hd, a.v_st, npk, lds0 + slot * 2 * TILE + TILE);
    };
    auto issue_q = [&](int item, int slot) {
      const int b = item / a.H, h = item - b * a.H;
      dma_tile(a.Q + (int64_t)b * a.q_sb + (int64_t)h * a.hd, a.q_st, npq, lds0 + QO_OFF + slot * NT * PF_QO_BYTES);
    };
    // O tiles (+ lse) of item `item`, parked by the compute waves in QO[slot] / lse[slot] -> global, whole 128-byte rows
    auto flush = [&](int item, int slot) {
      const int b = item / a.H, h = item - b * a.H;
      bf16_t* Ob = a.O + (int64_t)b * a.o_sb + (int64_t)h * a.hd;
      const char* qo = smem_pf + QO_OFF + slot * NT * PF_QO_BYTES;
      const int c = lane & 7;
      for (int q = 0; q < npk; q += 4) {                   // 4 pieces (32 rows) per round: loads first, then stores
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = (q + u) * 8 + (lane >> 3);
          v[u] = *reinterpret_cast<const u32x4*>(qo + swz(r, c * 8));    // rows beyond R: inside the buffer (NT x 32 rows)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = (q + u) * 8 + (lane >> 3);
          if (r < T && c * 8 < a.hd) *reinterpret_cast<u32x4*>(Ob + (int64_t)r * a.o_st + c * 8) = v[u];
        }
      }
      const float* ls = reinterpret_cast<const float*>(smem_pf + LSE_OFF + slot * NT * 128);
      float* lg = a.lse + ((int64_t)b * a.H + h) * T;
      for (int r = lane; r < T; r += 64) lg[r] = ls[r];
    };

    int item = blockIdx.x, slot = 0, prev = -1;
    if (item < nitems) { issue_kv(item, 0); issue_q(item, 0); }
    for (; item < nitems; item += gridDim.x) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // item `item` has landed (and the stores of item - 2 grid steps)
      __builtin_amdgcn_s_barrier();                        // B_i
      const int nxt = item + (int)gridDim.x;
      const bool has_next = nxt < nitems;
      if (has_next) issue_kv(nxt, slot ^ 1);               // that slot's readers (item i-1) are past the barrier
      if (prev >= 0) flush(prev, slot ^ 1);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the flush has read QO[slot ^ 1] before Q(i+1) lands in it
      if (has_next) issue_q(nxt, slot ^ 1);
      prev = item;
      slot ^= 1;
    }
    __builtin_amdgcn_s_barrier();                          // the last item's O tiles are parked
    if (prev >= 0) flush(prev, slot ^ 1);
    return;
  }

  // ================================ compute waves ================================
  const int q0 = wave * 32;
  const float sc2 = a.scale * 1.4426950408889634f;
  const int* klen = a.klen;
  int slot = 0;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    __builtin_amdgcn_s_barrier();                          // B_i: item i has landed
    // Lane-dependent offsets are loop invariants; hoisted out of the item loop they are ~30 registers that hipcc spills
    // around it.  They are recomputed per item from an OPAQUE copy of the lane id (a few integer operations each).
    int lane_i = lane;
    asm volatile("" : "+v"(lane_i));
    const int lh_i = lane_i >> 5, li_i = lane_i & 31, qg_i = q0 + li_i;
    int koff[4], voff[2][2];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) koff[kc] = swz(li_i, tileimg::frag_rows_col(kc, lh_i));
    {
      const int g4 = lane_i >> 4, q = lane_i & 15;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int j = 0; j < 2; ++j) voff[dt][j] = TR_LANE_OFF(g4, q, dt, j);
    }
    char* const qo = smem_pf + QO_OFF + (slot * NT + wave) * PF_QO_BYTES;
    float* const lse_w = reinterpret_cast<float*>(smem_pf + LSE_OFF) + (slot * NT + wave) * 32;
    bf16x8_t qf[4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(qo + koff[kc]);
      qf[kc] = __builtin_bit_cast(bf16x8_t, kc * 16 + 8 * lh_i < a.hd ? raw : u32x4{0u, 0u, 0u, 0u});
    }
    int kvalid = T;
    if (klen) { const int b = item / a.H; kvalid = klen[b] < T ? klen[b] : T; }

    const char* Kt = smem_pf + slot * 2 * TILE;
    const char* Vt = Kt + TILE;
    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    float m = -INFINITY, l = 0.f;
    int ntile = CAUSAL ? wave + 1 : NT;   // causal: key tiles beyond the wave's own query tile are fully masked

    // fragment loads are issued in BATCHES (all K fragments of a step before its first MFMA, all V^T fragments before the
    // softmax arithmetic; the asm statements with a memory clobber pin the issue points)
    auto kload = [&](int kt, bf16x8_t (&kf)[4]) {
      const char* kb = Kt + kt * 32 * ROWB;
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) kf[kc] = *reinterpret_cast<const bf16x8_t*>(kb + koff[kc]);
    };
    auto vload = [&](int kt, bf16x8_t (&vf)[2][2]) {
      const char* vb = Vt + kt * 32 * ROWB;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        vf[dt][0] = tr16_frag(vb, voff[dt][0], voff[dt][1]);
        vf[dt][1] = tr16_frag(vb + 16 * ROWB, voff[dt][0], voff[dt][1]);
      }
    };
    auto qk = [&](const bf16x8_t (&kf)[4]) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kc], qf[kc], s, 0, 0, 0);
      return s;
    };
    auto pv = [&](const bf16x8_t (&vf)[2][2], const u32x4 (&pk)[2]) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[dt][0], __builtin_bit_cast(bf16x8_t, pk[0]), o[dt], 0, 0, 0);
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[dt][1], __builtin_bit_cast(bf16x8_t, pk[1]), o[dt], 0, 0, 0);
      }
    };
    auto rescale = [&](float alpha) {       // skipped when no row's maximum moved (wave-uniform test)
      if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
        const v2f av = v2f{alpha, alpha};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const v2f a0 = v2f{o[0][2 * j], o[0][2 * j + 1]} * av, a1 = v2f{o[1][2 * j], o[1][2 * j + 1]} * av;
          o[0][2 * j] = a0[0]; o[0][2 * j + 1] = a0[1]; o[1][2 * j] = a1[0]; o[1][2 * j + 1] = a1[1];
        }
      }
    };
    // exponentials of one unmasked tile against the (new) row maximum mn: packed P + this lane's partial row sum
    auto exps = [&](const f32x16& s0, float mn, u32x4 (&pk)[2], v2f& rs2) {
      const v2f sc2v = v2f{sc2, sc2}, nmv = v2f{-mn, -mn};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const v2f e0 = v2f{s0[2 * j], s0[2 * j + 1]} * sc2v + nmv;
        const v2f x0 = v2f{__builtin_amdgcn_exp2f(e0[0]), __builtin_amdgcn_exp2f(e0[1])};
        rs2 += x0;
        pk[j >> 2][j & 3] = pack2bf(x0[0], x0[1]);
      }
    };
    auto max16 = [&](const f32x16& s0) {
      float mx = fmaxf(s0[0], s0[1]);
#pragma unroll
      for (int r = 2; r < 16; ++r) mx = fmaxf(mx, s0[r]);
      return mx;
    };
    bf16x8_t kfa[4], kfb[4];       // K fragments of the step that runs next (prefetched during the previous step)
    // TWO unmasked key tiles per softmax step
    auto step2 = [&](int kt, bool more) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const f32x16 sa = qk(kfa), sb = qk(kfb);
      bf16x8_t vfa[2][2], vfb[2][2];
      vload(kt, vfa);
      vload(kt + 1, vfb);
      asm volatile("" ::: "memory");
      const float mx = pf_xmax(fmaxf(max16(sa), max16(sb)));
      const float mn = fmaxf(m, mx * sc2);                  // finite: unmasked tiles have real scores in every row
      const float alpha = __builtin_amdgcn_exp2f(m - mn);   // m = -inf (first step) -> 0
      u32x4 pka[2], pkb[2];
      v2f rs2 = v2f{0.f, 0.f};
      exps(sa, mn, pka, rs2);
      exps(sb, mn, pkb, rs2);
      // the next pair's K fragments travel under the rescale and the PV products (S is dead: its registers are free)
      if (more) { kload(kt + 2, kfa); kload(kt + 3, kfb); asm volatile("" ::: "memory"); }
      l = l * alpha + pf_xsum(rs2[0] + rs2[1]);
      m = mn;
      rescale(alpha);
      pv(vfa, pka);
      pv(vfb, pkb);
    };
    auto step1 = [&](int kt) {
      kload(kt, kfa);
      bf16x8_t vfa[2][2];
      vload(kt, vfa);
      asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");    // the 4 K fragments; the V^T fragments keep travelling
      const f32x16 s0 = qk(kfa);
      const bool edge = kt * 32 + 32 > kvalid || (CAUSAL && kt * 32 + 31 > q0);
      u32x4 pk[2];
      if (!edge) {
        const float mx = pf_xmax(max16(s0));
        const float mn = fmaxf(m, mx * sc2);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        v2f rs2 = v2f{0.f, 0.f};
        exps(s0, mn, pk, rs2);
        l = l * alpha + pf_xsum(rs2[0] + rs2[1]);
        m = mn;
        rescale(alpha);
      } else {
        // key-padding / causal masks only here (wave-uniform test); a row may be fully masked: m stays -inf, P = 0
        float p[16];
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + acc_row(r, lh_i);
          const bool ok = key < kvalid && (!CAUSAL || key <= qg_i);
          p[r] = ok ? s0[r] * sc2 : -INFINITY;
          mx = fmaxf(mx, p[r]);
        }
        mx = pf_xmax(mx);
        const float mn = fmaxf(m, mx);
        const float msafe = mn == -INFINITY ? 0.f : mn;
        const float alpha = __builtin_amdgcn_exp2f(m - msafe);  // m = -inf -> 0
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(p[r] - msafe); rs += p[r]; }
        l = l * alpha + pf_xsum(rs);
        m = mn;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
        pk[0] = __builtin_bit_cast(u32x4, pack8(p));
        pk[1] = __builtin_bit_cast(u32x4, pack8(p + 8));
      }
      pv(vfa, pk);
    };

    {
      int nlean = kvalid >> 5;                              // tiles without a masked element
      if (CAUSAL && wave < nlean) nlean = wave;
      if (ntile > ((kvalid + 31) >> 5)) ntile = (kvalid + 31) >> 5;   // tiles behind the last valid key: P = 0
      int kt = 0;
      if (nlean >= 2) { kload(0, kfa); kload(1, kfb); }
      for (; kt + 2 <= nlean; kt += 2) step2(kt, kt + 4 <= nlean);
      for (; kt < ntile; ++kt) step1(kt);
    }

    // normalised O tile -> the wave's Q/O patch (its Q rows are in registers), lse -> its 32 floats; the loader wave
    // stores them during the next item
    {
      const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          u32x2 t;
          t[0] = pack2bf(o[dt][rg * 4 + 0] * inv, o[dt][rg * 4 + 1] * inv);
          t[1] = pack2bf(o[dt][rg * 4 + 2] * inv, o[dt][rg * 4 + 3] * inv);
          *reinterpret_cast<u32x2*>(qo + swz(li_i, tileimg::park_col(dt, rg, lh_i))) = t;
        }
      if (lh_i == 0) lse_w[li_i] = (l > 0.f) ? m * 0.6931471805599453f + __logf(l) : -INFINITY;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // parked before the barrier the loader flushes behind
    slot ^= 1;
  }
  __builtin_amdgcn_s_barrier();
}
