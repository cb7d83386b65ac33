// bf16 MFMA GEMM, LDS-DMA pipeline (the fast path for the large, aligned shapes of the training step).
// C[z](m,n) = epi(alpha * sum_k A(m,k) * B(n,k)),  A and B bf16, each k-contiguous or k-strided.
//
// Tile 256 x 128 x 64, 512 threads = 8 waves (two per SIMD): waves 4(m) x 2(n), each 64x64 = 2x2 MFMA 32x32x16 accumulators;
// or 128 x 128 x 64 on 4 waves 2(m) x 2(n).  (256 x 256 tiles run in gemm_bf16_p8.hip / gemm_bf16_pq.hip; the template
// still states the 128x64 wave tile that a BN = 256 instance would have, but none is built.)
// Operand tiles go L2 -> LDS directly (global_load_lds_dwordx4: 1 KiB per wave instruction, no VGPR round
// trip) into a double buffer (2 x 64 KiB): the DMA of K-tile t+1 is issued right after the barrier that
// publishes tile t and lands under tile t's MFMAs.  Measured on MI355X (tools/ubench/dma_bw.hip): an
// LDS-DMA stream of >=128-byte row pieces sustains ~84 GB/s per CU (21 TB/s chip) from L2, the same
// stream in 64-byte pieces only 40 GB/s - hence BK = 64 (128-byte rows of a k-contiguous operand) and the
// 256x256 tile (64 KiB per 2048 MFMA-cycles keeps the DMA engine at ~75 % while the matrix pipe is full).
// The LDS images (direct / ks with XOR, swizzled on the per-lane SOURCE address): gemm_operand_image.h.
// MFMA operand fragments are register double-buffered (chunk kc+1 is requested before the MFMAs of kc).
// Full tiles leave through the LDS-staged coalesced epilogue (gemm_bf16_common.h).
// Rows beyond M / N are clamped to valid addresses (their products are never stored); K must be a
// multiple of 64.  Which problems come here, and on which of the two tiles, is decided by gemm_plan.cpp (want_dma,
// pick_bn, dma_small_tiles, dma_covers); the launcher at the end of this file fills Args from the plan and decides nothing.
#include <stdlib.h>

#include "gemm_bf16_common.h"
#include "gemm_bf16_lds.h"

namespace {

constexpr int BK = GEMM_BK;

__device__ __forceinline__ void dma16(const bf16_t* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)lds_wave_base, 16, 0, 0);
}

// issue_direct takes its piece map from gemm_operand_image.h.  issue_ks and the fragment maps spell theirs out: called through
// the header, hipcc forms the addresses in another order and these kernels' code changes.  The arithmetic sits in constexpr
// helpers that keep the terms of each address apart as the kernels add them, and dma_maps_follow_image() below holds the
// helpers to the header.
struct PieceSrc { int row, chunk; };   // what a lane of a 1-KiB ks piece fetches: k-row and 16-byte chunk (8 rows) of it
template <int ROWS> constexpr __device__ __forceinline__ PieceSrc piece_ks_src(int idx, int lane) {
  constexpr int CHUNKS = ROWS / 8;              // 16-B chunks per k-row
  const int krow = idx * (512 / ROWS) + lane / CHUNKS;
  const int chunk = (lane % CHUNKS) ^ ((krow & 3) << 2);
  return PieceSrc{krow, chunk};
}
// k-contiguous operand with ROWS rows: X(row,k) = X[row*ld + k]; [ROWS][128 B]; ROWS/64 pieces per wave.
template <int ROWS, int NWV>
__device__ __forceinline__ void issue_direct(const bf16_t* __restrict__ X, int64_t ld, int64_t row0, int64_t nrows,
                                             int64_t k0, char* lds, int wave, int lane) {
  constexpr int PER_WAVE = ROWS / (8 * NWV);
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int idx = wave * PER_WAVE + i;        // 1-KiB piece = 8 rows of 128 B
    const int row = opimg::piece_direct_row(idx, lane);
    const int k = opimg::piece_direct_k(row, lane);
    int64_t r = row0 + row;
    r = r < nrows ? r : nrows - 1;
    dma16(X + r * ld + k0 + k, lds + idx * 1024);
  }
}
// k-strided operand with ROWS rows: X(row,k) = X[k*ld + row]; LDS image [64 k][ROWS], k-row = ROWS*2 bytes.
template <int ROWS, int NWV>
__device__ __forceinline__ void issue_ks(const bf16_t* __restrict__ X, int64_t ld, int64_t row0, int64_t nrows,
                                         int64_t k0, char* lds, int wave, int lane) {
  constexpr int PER_WAVE = ROWS / (8 * NWV);    // 64 k-rows * ROWS*2 B / 1 KiB / NWV waves
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int idx = wave * PER_WAVE + i;
    const PieceSrc s = piece_ks_src<ROWS>(idx, lane);
    int64_t r = row0 + s.chunk * 8;
    r = r + 8 <= nrows ? r : nrows - 8;
    dma16(X + (k0 + s.row) * ld + r, lds + idx * 1024);
  }
}

// 32x32x16 fragments: lane l -> row rbase + (l&31), k = kc*16 + 8*(l>>5) .. +7
struct LdsOff { int row, chunk, in_chunk; };   // byte offsets: of the (k-)row, of the 16-byte slot in it, inside the slot
constexpr __device__ __forceinline__ LdsOff frag_direct_off(int rbase, int kc, int lane) {
  const int r = rbase + (lane & 31);
  const int c = kc * 2 + (lane >> 5);
  return LdsOff{r * 128, (c ^ ((r >> 1) & 7)) << 4, 0};
}
template <int ROWS> constexpr __device__ __forceinline__ LdsOff frag_ks_off(int rbase, int kc, int lane) {
  const int g4 = lane >> 4, q = lane & 15;
  const int krow = kc * 16 + 8 * (g4 >> 1) + (q >> 2);
  const int col = rbase + 16 * (g4 & 1) + 4 * (q & 3);
  return LdsOff{krow * (ROWS * 2), (((col >> 3) ^ ((krow & 3) << 2))) << 4, (col & 7) << 1};
}
template <int ROWS> constexpr bool dma_maps_follow_image() {
  for (int l = 0; l < 64; ++l) {
    for (int idx = 0; idx < ROWS / 8; ++idx) {
      const PieceSrc k = piece_ks_src<ROWS>(idx, l);
      if (k.row != opimg::piece_ks_krow<ROWS>(idx, l) || k.chunk * 8 != opimg::piece_ks_row<ROWS>(k.row, l)) return false;
    }
    for (int rbase = 0; rbase < ROWS; rbase += 32)
      for (int kc = 0; kc < 4; ++kc) {
        const LdsOff d = frag_direct_off(rbase, kc, l), k = frag_ks_off<ROWS>(rbase, kc, l);
        if (d.row + d.chunk + d.in_chunk != opimg::frag_direct<false>(rbase, kc, l)) return false;
        if (k.row + k.chunk + k.in_chunk != opimg::frag_ks<ROWS * 2, true, false>(rbase, kc, l)) return false;
      }
  }
  return true;
}
static_assert(dma_maps_follow_image<128>() && dma_maps_follow_image<256>(),
              "gemm_bf16_dma.hip: piece_ks_src / frag_*_off must be the piece and fragment maps of gemm_operand_image.h");
__device__ __forceinline__ bf16x8_t frag_direct(const char* lds, int rbase, int kc, int lane) {
  const LdsOff o = frag_direct_off(rbase, kc, lane);
  return *reinterpret_cast<const bf16x8_t*>(lds + o.row + o.chunk);
}
template <int ROWS>
__device__ __forceinline__ bf16x8_t frag_ks(const char* lds, int rbase, int kc, int lane) {
  const LdsOff o = frag_ks_off<ROWS>(rbase, kc, lane);
  const char* p = lds + o.row + o.chunk + o.in_chunk;
  return tr16_frag(p, 4 * (ROWS * 2));
}

// <BM, BN, NWV>: <256,128,8> owns a CU (139 KB of LDS: the eight epilogue patches, over a 96 KiB operand ring);
// <128,128,4> (waves 2x2, 64x64 each) needs 68 KiB, so two workgroups share a CU and one's output phase overlaps
// the other's MFMA phase.
template <bool A_KS, bool B_KS, int BM, int BN, int NWV>
__global__ __launch_bounds__(NWV * 64, NWV == 4 ? 2 : 1) void gemm_bf16_dma_kernel(Args g) {
  constexpr int SZA = BM * BK * 2;
  constexpr int SZB = BN * BK * 2;
  constexpr int SZS = SZA + SZB;
  constexpr int WN = BN / 64;                          // waves along n (64 columns each)
  constexpr int WM = NWV / WN;                         // waves along m
  constexpr int TM = BM / (WM * 32);                   // 32-row MFMA tiles per wave along m
  constexpr int WROWS = TM * 32;                       // rows per wave
  static_assert(TM == 2 || TM == 4, "wave tile must be 64x64 or 128x64");
  constexpr int LDS_BYTES = 2 * SZS > NWV * EPI_WAVE_BYTES ? 2 * SZS : NWV * EPI_WAVE_BYTES;   // two-stage operand ring
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN;
  const int wn = wave % WN;
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wg = opimg::xcd_chunked(bid, nwg);
  const int64_t n0 = (int64_t)(wg % g.nbx) * BN, m0 = (int64_t)(wg / g.nbx) * BM;
  const int64_t z = blockIdx.z, z1 = z / g.nb2, z2 = z % g.nb2;
  const bf16_t* A = reinterpret_cast<const bf16_t*>(g.A) + z1 * g.bsA1 + z2 * g.bsA2;
  const bf16_t* B = g.B + z1 * g.bsB1 + z2 * g.bsB2;
  const int64_t coff = z1 * g.bsC1 + z2 * g.bsC2;
  const int64_t roff = z1 * g.bsR1 + z2 * g.bsR2;

  f32x16 acc[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int64_t kbeg = (int64_t)blockIdx.y * g.kper;
  const int64_t kend = kbeg + g.kper < g.K ? kbeg + g.kper : g.K;
  const int nk = (int)((kend - kbeg) / BK);

  auto issue = [&](int t) {
    char* la = smem + (t % 2) * SZS;
    char* lb = la + SZA;
    const int64_t k0 = kbeg + (int64_t)t * BK;
    if constexpr (A_KS) issue_ks<BM, NWV>(A, g.lda, m0, g.M, k0, la, wave, lane);
    else issue_direct<BM, NWV>(A, g.lda, m0, g.M, k0, la, wave, lane);
    if constexpr (B_KS) issue_ks<BN, NWV>(B, g.ldb, n0, g.N, k0, lb, wave, lane);
    else issue_direct<BN, NWV>(B, g.ldb, n0, g.N, k0, lb, wave, lane);
  };

  // The first round of workgroups (one per CU) starts with a bounded, staggered delay: tiles all take the same
  // time, so without it every CU reaches its store phase at the same moment and the HBM write burst (not
  // overlapped with any MFMA: one workgroup per CU) is paid in full by every tile round (+5..10 % measured).
  if (NWV == 8 && bid < 256 && gridDim.x * gridDim.y * gridDim.z > 256) {
    const long long t_tile = (long long)nk * 4000 + 20000;
    const long long unit = t_tile / 8 < 5000 ? t_tile / 8 : 5000;
    const long long wait = ((bid >> 3) & 7) * unit;
    const long long t0 = clock64();
    while (clock64() - t0 < wait) __builtin_amdgcn_s_sleep(32);
  }
  issue(0);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of tile t has landed
    __builtin_amdgcn_s_barrier();                       // ... and everybody else's; buffer (t-1)%2 is free
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) issue(t + 1);
    const char* la = smem + (t % 2) * SZS;
    const char* lb = la + SZA;
    // fragments of k16-chunk kc+1 are requested before the MFMAs of chunk kc (register double buffer)
    bf16x8_t fa[2][TM], fb[2][2];
    auto ldfrag = [&](int kc, bf16x8_t (&a)[TM], bf16x8_t (&b)[2]) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a[i] = A_KS ? frag_ks<BM>(la, wm * WROWS + i * 32, kc, lane) : frag_direct(la, wm * WROWS + i * 32, kc, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j] = B_KS ? frag_ks<BN>(lb, wn * 64 + j * 32, kc, lane) : frag_direct(lb, wn * 64 + j * 32, kc, lane);
    };
    ldfrag(0, fa[0], fb[0]);
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      // hipcc waits with lgkmcnt(0) at the first MFMA that uses a fragment, i.e. also for whatever was requested
      // after it.  Consuming chunk kc's registers here puts that wait BEFORE the request of chunk kc+1, whose LDS
      // latency is then covered by the MFMAs of chunk kc instead of being exposed.
#pragma unroll
      for (int i = 0; i < TM; ++i) asm volatile("" ::"v"(__builtin_bit_cast(u32x4, fa[kc & 1][i])));
#pragma unroll
      for (int j = 0; j < 2; ++j) asm volatile("" ::"v"(__builtin_bit_cast(u32x4, fb[kc & 1][j])));
      if (kc < 3) ldfrag(kc + 1, fa[(kc + 1) & 1], fb[(kc + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch above the MFMAs (else hipcc re-serialises it)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kc & 1][i], fb[kc & 1][j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  const int64_t mw = m0 + wm * WROWS;  // this wave's WROWS x 64 sub-tile
  const int64_t nw = n0 + wn * 64;
  if (g.splits > 1) {
    const int li = lane & 31, lk = lane >> 5;
    float* slab = g.slab + ((int64_t)blockIdx.y * gridDim.z + z) * g.M * g.N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t n = nw + j * 32 + li;
        if (n >= g.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t m = mw + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (m < g.M) __builtin_nontemporal_store(acc[i][j][r], &slab[m * g.N + n]);
        }
      }
    return;
  }
  const bool full = m0 + BM <= g.M && n0 + BN <= g.N;  // uniform over the workgroup
  const bool vec = full && g.vec_epi;
  if (vec) __syncthreads();  // every wave is done with the operand ring: the LDS is reused as 8 private patches
  float* t = reinterpret_cast<float*>(smem + wave * EPI_WAVE_BYTES);
#define RUN_EPI(SUB, MROW)                                                                              \
  do {                                                                                                  \
    if (vec) {                                                                                          \
      if (g.c_dtype == SEGCLIP_BF16) epilogue_lds_mode<bf16_t>(g, SUB, t, MROW, nw, lane, coff, roff);  \
      else epilogue_lds_mode<float>(g, SUB, t, MROW, nw, lane, coff, roff);                             \
    } else {                                                                                            \
      if (g.c_dtype == SEGCLIP_BF16) epilogue_mode<bf16_t, false>(g, SUB, MROW, nw, 0, 0, lane, coff, roff); \
      else epilogue_mode<float, false>(g, SUB, MROW, nw, 0, 0, lane, coff, roff);                       \
    }                                                                                                   \
  } while (0)
  if constexpr (TM == 2) {
    RUN_EPI(acc, mw);
  } else {
    f32x16 lo[2][2] = {{acc[0][0], acc[0][1]}, {acc[1][0], acc[1][1]}};
    RUN_EPI(lo, mw);
    __builtin_amdgcn_wave_barrier();
    f32x16 hi[2][2] = {{acc[2][0], acc[2][1]}, {acc[3][0], acc[3][1]}};
    RUN_EPI(hi, mw + 64);
  }
#undef RUN_EPI
}

}  // namespace

// Compiled once per DMA_PART (build.sh), like gemm_bf16_p8.hip: parts 0..3 hold the kernel instances of one operand
// layout <A_KS = part>>1, B_KS = part&1> behind a launcher, part 4 the family's launcher (no device code).
#ifndef DMA_PART
#error "compile with -DDMA_PART=0..4 (see build.sh)"
#endif
// the two instances by route variant (gemm_plan.h): DMA_128x128 (4 waves) first, which is the order in which the code object
// holds them
#define DMA_LAUNCHER(NAME, AK, BKS)                                                                             \
  void NAME(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream) {                                \
    typedef void (*kernel_t)(Args);                                                                             \
    static const kernel_t kernels[2] = {gemm_bf16_dma_kernel<AK, BKS, 128, 128, 4>, gemm_bf16_dma_kernel<AK, BKS, 256, 128, 8>}; \
    const bool small = p.route.variant == DMA_128x128;                                                          \
    hipLaunchKernelGGL(kernels[small ? 0 : 1], gemm_grid(p), dim3(small ? 256 : 512), 0, stream, gemm_args(d, p)); \
  }
#if DMA_PART == 0
DMA_LAUNCHER(segclip_dma_launch_ff, false, false)
#elif DMA_PART == 1
DMA_LAUNCHER(segclip_dma_launch_fk, false, true)
#elif DMA_PART == 2
DMA_LAUNCHER(segclip_dma_launch_kf, true, false)
#elif DMA_PART == 3
DMA_LAUNCHER(segclip_dma_launch_kk, true, true)
#endif

#if DMA_PART == 4
void segclip_dma_launch_ff(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_dma_launch_fk(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_dma_launch_kf(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_dma_launch_kk(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);

void segclip_gemm_launch_dma(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream) {
  static const gemm_layout_launcher layouts[4] = {segclip_dma_launch_ff, segclip_dma_launch_fk, segclip_dma_launch_kf, segclip_dma_launch_kk};
  layouts[gemm_layout_index(p)](d, p, stream);
}
#endif  // DMA_PART == 4
