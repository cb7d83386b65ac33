// bf16 MFMA GEMM, 256x256x64 tile, phase-pipelined LDS-DMA ring (the fast path for the large aligned shapes of the
// training step; same contract as gemm_bf16_dma.hip: C[z](m,n) = epi(alpha * sum_k A(m,k) * B(n,k)), A and B bf16, each
// k-contiguous or k-strided, K a multiple of 64).
//
// What bounds the older kernel (gemm_bf16_dma.hip, one barrier per K-tile): the 64 KiB DMA burst of K-tile t+1 is issued
// after barrier t and must have landed by barrier t+1, so a K-step lasts one loaded L2->LDS round trip (1.65 us measured
// against 1.0 us of MFMA time) and the queue drains every step.  Here the tile's operands are four 16-KiB HALF-TILES
//      A0 = rows 0-127, A1 = rows 128-255, B0 = columns 0-127, B1 = columns 128-255     (each [128][64 k])
// and a wave (wr = wave/4, wc = wave%4) owns a 2x2 set of 64x32 blocks: rows {h*128 + wr*64 ..+63}, columns
// {h*128 + wc*32 ..+31}.  A K-tile is four PHASES, one C quadrant each - (A0,B0) (A0,B1) (A1,B1) (A1,B0) - so every
// half-tile is read from LDS in exactly ONE phase (A0,B0: phase 1, B1: phase 2, A1: phase 3; phase 4 re-uses registers)
// and its slot can be refilled two phases later.  A phase is an R segment (LDS fragment reads, the DMA issue of one
// half-tile = 2 instructions per wave, one counted vmcnt wait) and an M segment (8 MFMAs, s_setprio 1) separated by
// barriers.  The two wave groups (wr = 0 / 1; one wave of each per SIMD) run half a phase apart: while one group is in
// M the other is in R, so the matrix pipe of every SIMD is fed alternately by its two waves and the issue cost of the
// loads (measured: ~16 cycles per ds_read_b128, ~80 per LDS-DMA piece; an in-order wave cannot hide them in its own
// MFMA gaps - a variant with the loads inside M ran 18 % slower) is paid under the partner's MFMAs.  For that the R
// segments must all be shorter than an M segment (256 cycles), i.e. the load work must be spread evenly:
//      R1: read A0(t)   (8) + DMA A1(t+1)        M1: quadrant (A0,B0)
//      R2: read B1(t)   (4) + DMA B0(t+2)        M2: quadrant (A0,B1)
//      R3: read A1(t)   (8) + DMA A0(t+2)        M3: quadrant (A1,B1)
//      R4: read B0(t+1) (4) + DMA B1(t+2)        M4: quadrant (A1,B0)      (the two B register sets alternate per tile)
// Every half-tile is issued 5 phases ahead of the R segment that reads it, at the first moment its slot is free, and is
// retired by a COUNTED s_waitcnt vmcnt(10) one phase before that read, so 80 KiB stay in flight across the barriers at
// all times (2 buffers x 4 half-tiles = 128 KiB of LDS, as in the older kernel).
// Ordering rules (MI355X guide, LDS-DMA): data is read one phase after the vmcnt that retires it (wait in R(q), every
// wave passes a barrier, read in R(q+1)); a slot is refilled >= 2 phases after its last read (the reads' lgkmcnt(0) sits
// after the barrier that follows them).
// Which problems come here is decided by gemm_plan.cpp (pick_bn == 256, after pq_covers refused, p8_covers); the launcher at
// the end of this file fills Args from the plan and decides nothing.
#include <stdlib.h>

#include <type_traits>

#include "gemm_bf16_common.h"
#include "gemm_bf16_lds.h"

namespace {

constexpr int BK = GEMM_BK, BT = GEMM_BIG_TILE, NWV = 8;
constexpr int UNIT = 128 * BK * 2;            // one half-tile: 16 KiB
constexpr int BUF = 4 * UNIT;                 // A0 A1 B0 B1
constexpr int RING = 2 * BUF;                 // 128 KiB

// Per-lane byte offset (relative to the tile's first element of the operand) of DMA piece `idx` (1 KiB) of half-tile h
// (128 rows: direct image / ks image at pitch 256 B, gemm_operand_image.h); rows beyond nrows are clamped.
// (off_direct spells the direct piece map out: through the header's functions hipcc emits the same instructions in another
// order; the static_assert below holds it to the header)
constexpr __device__ __forceinline__ uint32_t off_direct(int h, int idx, int lane, int64_t ld, int64_t row0, int64_t nrows) {
  const int u = idx * 8 + (lane >> 3);
  const int chunk = (lane & 7) ^ ((u >> 1) & 7);
  int64_t r = row0 + h * 128 + u;
  r = r < nrows ? r : nrows - 1;
  return (uint32_t)(((r - row0) * ld + chunk * 8) * 2);
}
constexpr bool p8_off_direct_follows_image() {   // full tile (no row clamped), two pitches, as in gemm_bf16_pq.hip
  for (int h = 0; h < 2; ++h)
    for (int idx = 0; idx < 16; ++idx)
      for (int l = 0; l < 64; ++l)
        for (int ld = 64; ld <= 72; ld += 8) {
          const int row = opimg::piece_direct_row(idx, l);
          if (off_direct(h, idx, l, ld, 256, 1024) != (uint32_t)(((h * 128 + row) * ld + opimg::piece_direct_k(row, l)) * 2)) return false;
        }
  return true;
}
static_assert(p8_off_direct_follows_image(), "gemm_bf16_p8.hip: off_direct must be the direct piece map of gemm_operand_image.h");
__device__ __forceinline__ uint32_t off_ks(int h, int idx, int lane, int64_t ld, int64_t row0, int64_t nrows) {
  const int krow = opimg::piece_ks_krow<128>(idx, lane);
  int64_t r = row0 + h * 128 + opimg::piece_ks_row<128>(krow, lane);
  r = r + 8 <= nrows ? r : nrows - 8;
  return (uint32_t)((krow * ld + (r - row0)) * 2);
}

// ---- operand fragments.  The K loop reads 24 fragments per K-tile and wave; with the address arithmetic done per read
// (row * pitch + swizzle) it spent ~94 VALU instructions per K-tile on addresses - in the R segments, which must stay
// shorter than the partner group's 8 MFMAs.  Every fragment address is   lane base (VGPR, computed ONCE per kernel)
// + compile-time constant (ring buffer, half-tile unit, 32-row block, k chunk), i.e. `ds_read ... offset:imm`:
//   direct image: the chunk index c = 2 kc + (l>>5) enters through the XOR, so there is one base per kc (4 VGPRs per
//     operand and ring buffer; the 16-bit DS offset cannot reach the second 64-KiB buffer from the first one's base);
//     a 32-row block is an immediate (4096 B: rbase does not enter the XOR);
//   ks image: kc is a pure row offset (kc * 16 * 256), the 32-row block index flips a swizzled bit: one base per block.
__device__ __forceinline__ uint32_t fragbase_direct(int rbase, int kc, int lane) {
  return (uint32_t)opimg::frag_direct<false>(rbase, kc, lane);
}
__device__ __forceinline__ uint32_t fragbase_ks(int rbase, int lane) {   // kc = 0; + kc * 4096 for the others
  return (uint32_t)opimg::frag_ks<256, true, false>(rbase, 0, lane);
}

template <bool A_KS, bool B_KS>
__global__ __launch_bounds__(NWV * 64) void gemm_bf16_p8_kernel(Args g) {
  constexpr int LDS_BYTES = RING > NWV * EPI_WAVE_BYTES ? RING : NWV * EPI_WAVE_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  // Workgroups go to the XCDs round-robin in dispatch order (x fastest, then y): the (tile, K-split) space is walked
  // split-major and cut into 8 contiguous chunks, one per XCD, so that the tiles that share an A row slab / B column
  // slab - and, with split-K, the SAME K range - sit behind one L2.
  const int nt = gridDim.x;
  const int nwg = nt * gridDim.y, bid = blockIdx.x + nt * blockIdx.y;
  const int unit_id = opimg::xcd_chunked(bid, nwg);
  const int wg = unit_id % nt, ksplit = unit_id / nt;
  // Tile order inside the sequence that is cut into the 8 XCD chunks: row-major over all nbx column tiles.
  const int tcol = wg % g.nbx, trow = wg / g.nbx;
  const int64_t n0 = (int64_t)tcol * BT, m0 = (int64_t)trow * BT;
  const int64_t z = blockIdx.z, z1 = z / g.nb2, z2 = z % g.nb2;
  const bf16_t* A = reinterpret_cast<const bf16_t*>(g.A) + z1 * g.bsA1 + z2 * g.bsA2;
  const bf16_t* B = g.B + z1 * g.bsB1 + z2 * g.bsB2;
  const int64_t coff = z1 * g.bsC1 + z2 * g.bsC2;
  const int64_t roff = z1 * g.bsR1 + z2 * g.bsR2;

  const int64_t kbeg = (int64_t)ksplit * g.kper;
  const int64_t kend = kbeg + g.kper < g.K ? kbeg + g.kper : g.K;
  const int nk = (int)((kend - kbeg) / BK);

  // uniform tile bases (bytes) + per-lane 32-bit offsets: the DMA address is SGPR base + VGPR offset
  const char* baseA = reinterpret_cast<const char*>(A_KS ? A + kbeg * g.lda + m0 : A + m0 * g.lda + kbeg);
  const char* baseB = reinterpret_cast<const char*>(B_KS ? B + kbeg * g.ldb + n0 : B + n0 * g.ldb + kbeg);
  const int64_t stepA = A_KS ? (int64_t)BK * g.lda * 2 : BK * 2;   // bytes per K-tile
  const int64_t stepB = B_KS ? (int64_t)BK * g.ldb * 2 : BK * 2;
  uint32_t offA[2][2], offB[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      offA[h][i] = A_KS ? off_ks(h, wave * 2 + i, lane, g.lda, m0, g.M) : off_direct(h, wave * 2 + i, lane, g.lda, m0, g.M);
      offB[h][i] = B_KS ? off_ks(h, wave * 2 + i, lane, g.ldb, n0, g.N) : off_direct(h, wave * 2 + i, lane, g.ldb, n0, g.N);
    }
  // half-tile `u` (0: A0, 1: A1, 2: B0, 3: B1) of K-tile t -> ring buffer t&1
  const uint32_t lds_ring = (uint32_t)(uintptr_t)((lds_void*)smem) + wave * 2048;
  auto stage = [&](int u, int t) {
    const uint32_t dst = lds_ring + (t & 1) * BUF + u * UNIT;
    if (u < 2) dma16x2(baseA + (int64_t)t * stepA, offA[u][0], offA[u][1], dst);
    else dma16x2(baseB + (int64_t)t * stepB, offB[u - 2][0], offB[u - 2][1], dst);
  };

  f32x16 acc[2][2][2];  // [A half][32-row tile][B half]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int ri = 0; ri < 2; ++ri)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][ri][j][r] = 0.f;

  // The first round of workgroups (one per CU) starts with a bounded, staggered delay so that the CUs do not all reach
  // their store phase at the same moment in every later round (kept from gemm_bf16_dma.hip, where it measured +5..10 %).
  if (g.stagger > 0 && bid < 256 && gridDim.x * gridDim.y * gridDim.z > 256) {
    const long long t_tile = (long long)nk * 3000 + 20000;
    const long long cap = (long long)g.stagger;
    const long long unit = t_tile / 8 < cap ? t_tile / 8 : cap;
    // tiles of one block row share their A rows through the XCD's L2: they get the SAME delay and stay in lockstep
    const long long wait = (trow & 7) * unit;
    const long long t0 = clock64();
    while (clock64() - t0 < wait) __builtin_amdgcn_s_sleep(32);
  }

  // prologue: the issue order continues into the steady state (... B0 A0 B1 A1 ...): K-tile 0 and, of K-tile 1,
  // everything but A1 (issued in R1 of tile 0)
  stage(2, 0);
  stage(0, 0);
  stage(3, 0);
  stage(1, 0);
  if (nk > 1) {
    stage(2, 1);
    stage(0, 1);
    stage(3, 1);
    wait_vm<10>();   // B0(0), A0(0) have landed
  } else {
    wait_vm<4>();
  }
  GEMM_RING_BAR();

  bf16x8_t fa[2][4], fbx[4], fby[4];
  // lane bases of the fragment reads (see the fragment helpers): [ring buffer][kc] for a k-contiguous operand,
  // [ring buffer][32-row block] for a k-strided one; made opaque so that the compiler keeps them in registers instead
  // of re-deriving them in the K loop
  lds_cchar* const sm3 = (lds_cchar*)smem;
  lds_cchar* abase[2][4];
  lds_cchar* bbase[2][4];
#pragma unroll
  for (int bf = 0; bf < 2; ++bf)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      uint32_t oa = A_KS ? fragbase_ks(wr * 64 + (x & 1) * 32, lane) : fragbase_direct(wr * 64, x, lane);
      uint32_t ob = B_KS ? fragbase_ks(wc * 32, lane) : fragbase_direct(wc * 32, x, lane);
      oa += bf * BUF; ob += bf * BUF;
      if ((!A_KS || x < 2)) asm volatile("" : "+v"(oa));
      if ((!B_KS || x < 1)) asm volatile("" : "+v"(ob));
      abase[bf][x] = sm3 + oa;
      bbase[bf][x] = sm3 + ob;
    }
  // U: byte offset of the half-tile unit inside its ring buffer
  auto read_a = [&](auto bfc, auto uc) {
    constexpr int BF_ = decltype(bfc)::value, U = decltype(uc)::value;
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
      if constexpr (A_KS) {
        fa[ri][0] = frag_ks_at<U + 0 * 4096>(abase[BF_][ri]);
        fa[ri][1] = frag_ks_at<U + 1 * 4096>(abase[BF_][ri]);
        fa[ri][2] = frag_ks_at<U + 2 * 4096>(abase[BF_][ri]);
        fa[ri][3] = frag_ks_at<U + 3 * 4096>(abase[BF_][ri]);
      } else {
        if (ri == 0) {
          fa[0][0] = frag_direct_at<U>(abase[BF_][0]); fa[0][1] = frag_direct_at<U>(abase[BF_][1]);
          fa[0][2] = frag_direct_at<U>(abase[BF_][2]); fa[0][3] = frag_direct_at<U>(abase[BF_][3]);
        } else {
          fa[1][0] = frag_direct_at<U + 4096>(abase[BF_][0]); fa[1][1] = frag_direct_at<U + 4096>(abase[BF_][1]);
          fa[1][2] = frag_direct_at<U + 4096>(abase[BF_][2]); fa[1][3] = frag_direct_at<U + 4096>(abase[BF_][3]);
        }
      }
    }
  };
  auto read_b = [&](auto bfc, auto uc, bf16x8_t (&fb)[4]) {
    constexpr int BF_ = decltype(bfc)::value, U = decltype(uc)::value;
    if constexpr (B_KS) {
      fb[0] = frag_ks_at<U + 0 * 4096>(bbase[BF_][0]); fb[1] = frag_ks_at<U + 1 * 4096>(bbase[BF_][0]);
      fb[2] = frag_ks_at<U + 2 * 4096>(bbase[BF_][0]); fb[3] = frag_ks_at<U + 3 * 4096>(bbase[BF_][0]);
    } else {
      fb[0] = frag_direct_at<U>(bbase[BF_][0]); fb[1] = frag_direct_at<U>(bbase[BF_][1]);
      fb[2] = frag_direct_at<U>(bbase[BF_][2]); fb[3] = frag_direct_at<U>(bbase[BF_][3]);
    }
  };
  auto quadrant = [&](f32x16 (&c)[2][2], int j, const bf16x8_t (&fb)[4]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kc = 0; kc < 4; ++kc)
#pragma unroll
      for (int ri = 0; ri < 2; ++ri) c[ri][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ri][kc], fb[kc], c[ri][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  using std::integral_constant;
  typedef integral_constant<int, 0> I0;
  typedef integral_constant<int, 1> I1;
  read_b(I0{}, integral_constant<int, 2 * UNIT>{}, fbx);   // B0 of K-tile 0 (in the loop this read sits in R4 of the previous tile)
  if (wr == 1) GEMM_RING_BAR();     // group 1 runs one barrier interval behind group 0

  // one K-tile: fbp holds B0(t) on entry and fbq is free; on exit fbq holds B0(t+1)
  // (bc = t & 1 as a type: the ring-buffer offset of every fragment read is a compile-time constant)
  auto ktile = [&](auto bc, int t, bf16x8_t (&fbp)[4], bf16x8_t (&fbq)[4]) {
    typedef decltype(bc) CB;
    typedef integral_constant<int, 1 - CB::value> NB;
    const bool n1 = t + 1 < nk, n2 = t + 2 < nk;
    // ---- phase 1: quadrant (A0, B0)
    read_a(CB{}, integral_constant<int, 0>{});
    if (n1) { stage(1, t + 1); wait_vm<10>(); } else { wait_vm<2>(); }          // retires B1(t), read in R2
    GEMM_RING_BAR();
    quadrant(acc[0], 0, fbp);
    GEMM_RING_BAR();
    // ---- phase 2: quadrant (A0, B1)
    read_b(CB{}, integral_constant<int, 3 * UNIT>{}, fbq);
    if (n2) { stage(2, t + 2); wait_vm<10>(); } else if (n1) { wait_vm<8>(); } else { wait_vm<0>(); }   // retires A1(t)
    GEMM_RING_BAR();
    quadrant(acc[0], 1, fbq);
    GEMM_RING_BAR();
    // ---- phase 3: quadrant (A1, B1)
    read_a(CB{}, integral_constant<int, UNIT>{});
    if (n2) { stage(0, t + 2); wait_vm<10>(); } else if (n1) { wait_vm<6>(); }   // retires B0(t+1), read in R4
    GEMM_RING_BAR();
    quadrant(acc[1], 1, fbq);
    GEMM_RING_BAR();
    // ---- phase 4: quadrant (A1, B0); B1's registers are free: B0(t+1) goes there
    if (n1) read_b(NB{}, integral_constant<int, 2 * UNIT>{}, fbq);
    if (n2) { stage(3, t + 2); wait_vm<10>(); } else if (n1) { wait_vm<4>(); }   // retires A0(t+1), read in R1
    GEMM_RING_BAR();
    quadrant(acc[1], 0, fbp);
    GEMM_RING_BAR();
  };
  int t = 0;
  for (; t + 1 < nk; t += 2) {
    ktile(I0{}, t, fbx, fby);
    ktile(I1{}, t + 1, fby, fbx);
  }
  if (t < nk) ktile(I0{}, t, fbx, fby);
  if (wr == 0) GEMM_RING_BAR();  // group 0 catches up: both groups have executed the same number of barriers

  const int64_t nw = n0 + wc * 32;  // this wave's first column (second strip at +128)
  if (g.splits > 1) {
    const int li = lane & 31, lk = lane >> 5;
    float* slab = g.slab + ((int64_t)ksplit * gridDim.z + z) * g.M * g.N;
    // full tiles: the raw fp32 partial tile goes through the staged epilogue (park, 16-byte row stores: 32 store
    // instructions per wave instead of 128 one-dword stores); g.slab_staged = 0 keeps the per-element stores
    if (g.slab_staged && m0 + BT <= g.M && n0 + BT <= g.N && g.N % 4 == 0) {
      Args g2 = g;
      g2.C = slab; g2.ldc = g.N; g2.c_dtype = SEGCLIP_F32; g2.bias = nullptr; g2.residual = nullptr; g2.aux = nullptr;
      g2.act = SEGCLIP_ACT_NONE; g2.mul_dact = 0; g2.colsum_part = nullptr; g2.alpha = 1.0f;
      __syncthreads();  // every wave is done with the operand ring
      float* tps = reinterpret_cast<float*>(smem + wave * EPI_WAVE_BYTES);
      epilogue_lds2<float, EPI_PLAIN, 128>(g2, acc[0], acc[1], tps, m0 + wr * 64, m0 + 128 + wr * 64, nw, lane, 0, 0);
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int ri = 0; ri < 2; ++ri)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int64_t n = nw + j * 128 + li;
          if (n >= g.N) continue;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + i * 128 + wr * 64 + ri * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (m < g.M) __builtin_nontemporal_store(acc[i][ri][j][r], &slab[m * g.N + n]);
          }
        }
    return;
  }
  const bool full = m0 + BT <= g.M && n0 + BT <= g.N;  // uniform over the workgroup
  const bool vec = full && g.vec_epi;
  if (vec) __syncthreads();  // every wave is done with the operand ring: the LDS is reused as 8 private patches
  float* tp = reinterpret_cast<float*>(smem + wave * EPI_WAVE_BYTES);
  const int64_t mw0 = m0 + wr * 64, mw1 = m0 + 128 + wr * 64;
  if (vec) {
    if (g.c_dtype == SEGCLIP_BF16)
      epilogue_lds2_mode<bf16_t, 128>(g, acc[0], acc[1], tp, mw0, mw1, nw, lane, coff, roff,
                                      g.xw_epi ? reinterpret_cast<const float*>(smem) : nullptr, wr, wc, n0);
    else epilogue_lds2_mode<float, 128>(g, acc[0], acc[1], tp, mw0, mw1, nw, lane, coff, roff);
    return;
  }
  // two explicit copies (a loop over the A half would index the accumulators at run time -> scratch)
#define P8_EPI(I)                                                                                              \
  do {                                                                                                         \
    const int64_t mw = m0 + (I) * 128 + wr * 64;                                                               \
    if (g.c_dtype == SEGCLIP_BF16) epilogue_mode<bf16_t, false>(g, acc[I], mw, nw, 0, 0, lane, coff, roff, 128); \
    else epilogue_mode<float, false>(g, acc[I], mw, nw, 0, 0, lane, coff, roff, 128);                          \
  } while (0)
  P8_EPI(0);
  __builtin_amdgcn_wave_barrier();
  P8_EPI(1);
#undef P8_EPI
}

}  // namespace

// The file is compiled once per P8_PART (segclip_amd/csrc/build.sh) so that the four operand-layout instances - each
// carries every epilogue variant and takes over a minute of hipcc time - build in parallel:
//   P8_PART 0..3 : kernel instance <A_KS = part>>1, B_KS = part&1> and its launcher
//   P8_PART 4    : the family's launcher below (no device code)
#ifndef P8_PART
#error "compile with -DP8_PART=0..4 (see build.sh)"
#endif
#define P8_LAUNCHER(NAME, A_KS, B_KS)                                               \
  void NAME(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream) {    \
    hipLaunchKernelGGL((gemm_bf16_p8_kernel<A_KS, B_KS>), gemm_grid(p), dim3(512), 0, stream, gemm_args(d, p)); \
  }
#if P8_PART == 0
P8_LAUNCHER(segclip_p8_launch_ff, false, false)
#elif P8_PART == 1
P8_LAUNCHER(segclip_p8_launch_fk, false, true)
#elif P8_PART == 2
P8_LAUNCHER(segclip_p8_launch_kf, true, false)
#elif P8_PART == 3
P8_LAUNCHER(segclip_p8_launch_kk, true, true)
#endif

#if P8_PART == 4
void segclip_p8_launch_ff(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_p8_launch_fk(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_p8_launch_kf(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_p8_launch_kk(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);

void segclip_gemm_launch_p8(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream) {
  static const gemm_layout_launcher layouts[4] = {segclip_p8_launch_ff, segclip_p8_launch_fk, segclip_p8_launch_kf, segclip_p8_launch_kk};
  layouts[gemm_layout_index(p)](d, p, stream);
}
#endif  // P8_PART == 4
