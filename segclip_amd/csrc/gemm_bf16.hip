// bf16 MFMA GEMM (v_mfma_f32_32x32x16_bf16, fp32 accumulate) with fused epilogue.
// C[z](m,n) = epi(alpha * sum_k A(m,k) * B(n,k)).
//
// One kernel template covers the three layouts of a training step:
//   forward  Y = X W^T      : A k-contiguous, B k-contiguous          <A_KS=0, B_KS=0>
//   dgrad    dX = dY W      : A k-contiguous, B k-strided (W[n][k])   <A_KS=0, B_KS=1>
//   wgrad    dW = dY^T X    : A k-strided,   B k-strided             <A_KS=1, B_KS=1>
// k-contiguous operands are staged as the direct LDS image, k-strided ones as the ks image at pitch 320 B without XOR
// (gemm_operand_image.h) and read with the gfx950 LDS transpose read ds_read_b64_tr_b16, so neither W nor the
// activations are ever transposed in HBM.
// The A operand may be fp32 in HBM (residual-stream gradients): it is rounded to bf16 while staging.
//
// Tile 128x128x64, 256 threads = 4 waves (2x2), each wave 64x64 = 2x2 MFMA tiles (64 acc VGPRs).
// Register-staged double buffer: the 8 global loads of tile t+1 are issued before the MFMAs of tile t
// and stay in flight under them; conversion / zero-masking / ds_write happen after the MFMAs (one
// barrier per K-step).  All loads are unconditional from clamped addresses (no divergent branch around a
// load).  Workgroup ids are remapped so each XCD walks a contiguous run of tiles (A panel reuse in its L2).
// Split-K (grid.y) for the wgrad shapes, combined by a deterministic slab reduction.
// This kernel takes what the planner (gemm_plan.cpp) gives to no LDS-DMA kernel; its launcher at the end of this file fills
// Args from the plan and decides nothing.  The trailing reductions of every bf16 family (segclip_gemm, capi.cpp) are here too.
#include <stdlib.h>

#include "gemm_bf16_common.h"
#include "gemm_bf16_lds.h"
#include "reduce_rows.h"

namespace {

constexpr int BM = GEMM_TILE, BN = GEMM_TILE, BK = GEMM_BK, NT = 256;
constexpr int KS_PITCH = 160;                 // elements per k-row of a k-strided image (320 B)
constexpr int SZ_DIRECT = BM * BK * 2;        // 16384 B
constexpr int SZ_KS = BK * KS_PITCH * 2;      // 20480 B

// raw staged data of one operand tile: 4 chunks of 8 elements per thread (+ validity bits)
template <typename T> struct Stage;
template <> struct Stage<bf16_t> { u32x4 v[4]; unsigned ok; };
template <> struct Stage<float> { f32x4 lo[4], hi[4]; unsigned ok; };

template <typename T> __device__ __forceinline__ void ld8(Stage<T>& s, int i, const T* p);
template <> __device__ __forceinline__ void ld8<bf16_t>(Stage<bf16_t>& s, int i, const bf16_t* p) {
  s.v[i] = *reinterpret_cast<const u32x4*>(p);
}
template <> __device__ __forceinline__ void ld8<float>(Stage<float>& s, int i, const float* p) {
  s.lo[i] = *reinterpret_cast<const f32x4*>(p);
  s.hi[i] = *reinterpret_cast<const f32x4*>(p + 4);
}
__device__ __forceinline__ u32x4 chunk(const Stage<bf16_t>& s, int i) {
  return ((s.ok >> i) & 1u) ? s.v[i] : u32x4{0u, 0u, 0u, 0u};
}
__device__ __forceinline__ u32x4 chunk(const Stage<float>& s, int i) {
  u32x4 v;
  v[0] = pack2bf(s.lo[i][0], s.lo[i][1]); v[1] = pack2bf(s.lo[i][2], s.lo[i][3]);
  v[2] = pack2bf(s.hi[i][0], s.hi[i][1]); v[3] = pack2bf(s.hi[i][2], s.hi[i][3]);
  return ((s.ok >> i) & 1u) ? v : u32x4{0u, 0u, 0u, 0u};
}

// ---- global -> registers (FAST: 16-byte aligned rows, branch-free) ----------------------------
// k-contiguous operand: X(row,k) = X[row*ld + k]; thread -> chunk c = tid&7 (8 k), rows tid>>3 + 32*i
template <typename T>
__device__ __forceinline__ void gload_direct_fast(Stage<T>& s, const T* __restrict__ X, int64_t ld, int64_t row0,
                                                  int64_t nrows, int64_t k0, int64_t K, int tid) {
  const int64_t k = k0 + (tid & 7) * 8;
  const bool kok = k < K;
  const int64_t kc = kok ? k : K - 8;
  unsigned ok = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + (tid >> 3) + 32 * i;
    ok |= (unsigned)(kok && r < nrows) << i;
    ld8<T>(s, i, X + (r < nrows ? r : nrows - 1) * ld + kc);
  }
  s.ok = ok;
}
// k-strided operand: X(row,k) = X[k*ld + row]; thread -> chunk c = tid&15 (8 rows), k = tid>>4 + 16*i
template <typename T>
__device__ __forceinline__ void gload_ks_fast(Stage<T>& s, const T* __restrict__ X, int64_t ld, int64_t row0,
                                              int64_t nrows, int64_t k0, int64_t K, int tid) {
  const int64_t r = row0 + (tid & 15) * 8;
  const bool rok = r < nrows;
  const int64_t rc = rok ? r : nrows - 8;
  unsigned ok = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t k = k0 + (tid >> 4) + 16 * i;
    ok |= (unsigned)(rok && k < K) << i;
    ld8<T>(s, i, X + (k < K ? k : K - 1) * ld + rc);
  }
  s.ok = ok;
}

// ---- global -> registers (generic: any alignment / ragged K; element-wise guarded) -------------
template <typename T> __device__ __forceinline__ void put8(Stage<T>& s, int i, const float* e);
template <> __device__ __forceinline__ void put8<bf16_t>(Stage<bf16_t>& s, int i, const float* e) {
#pragma unroll
  for (int j = 0; j < 4; ++j) s.v[i][j] = pack2bf(e[2 * j], e[2 * j + 1]);
}
template <> __device__ __forceinline__ void put8<float>(Stage<float>& s, int i, const float* e) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { s.lo[i][j] = e[j]; s.hi[i][j] = e[4 + j]; }
}
template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }

template <typename T>
__device__ __forceinline__ void gload_direct_slow(Stage<T>& s, const T* __restrict__ X, int64_t ld, int64_t row0,
                                                  int64_t nrows, int64_t k0, int64_t K, int tid) {
  const int64_t k = k0 + (tid & 7) * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + (tid >> 3) + 32 * i;
    float e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = (r < nrows && k + j < K) ? ldf<T>(X + r * ld + k + j) : 0.f;
    put8<T>(s, i, e);
  }
  s.ok = 0xF;
}
template <typename T>
__device__ __forceinline__ void gload_ks_slow(Stage<T>& s, const T* __restrict__ X, int64_t ld, int64_t row0,
                                              int64_t nrows, int64_t k0, int64_t K, int tid) {
  const int64_t r = row0 + (tid & 15) * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t k = k0 + (tid >> 4) + 16 * i;
    float e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = (k < K && r + j < nrows) ? ldf<T>(X + k * ld + r + j) : 0.f;
    put8<T>(s, i, e);
  }
  s.ok = 0xF;
}

// ---- registers -> LDS -----------------------------------------------------------------------
// The two stores spell the image addresses of gemm_operand_image.h out: called through the header, hipcc forms the address
// in another order and the kernels' code changes.  The arithmetic sits in constexpr helpers that keep the two
// terms of an address apart as the kernels add them, and gb_maps_follow_image() below holds the helpers to the header.
struct LdsOff { int row, in_row; };   // byte offset of the (k-)row, byte offset inside it
constexpr __device__ __forceinline__ LdsOff sstore_direct_off(int tid, int i) {
  const int c = tid & 7;
  const int r = (tid >> 3) + 32 * i;
  return LdsOff{r * 128, (c ^ ((r >> 1) & 7)) << 4};
}
constexpr __device__ __forceinline__ LdsOff sstore_ks_off(int tid, int i) {
  const int c = tid & 15;
  const int k = (tid >> 4) + 16 * i;
  return LdsOff{k * (KS_PITCH * 2), c * 16};
}
template <typename T>
__device__ __forceinline__ void sstore_direct(const Stage<T>& s, char* lds, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u32x4 v = chunk(s, i);
    const LdsOff o = sstore_direct_off(tid, i);
    *reinterpret_cast<u32x4*>(lds + o.row + o.in_row) = v;
  }
}
template <typename T>
__device__ __forceinline__ void sstore_ks(const Stage<T>& s, char* lds, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u32x4 v = chunk(s, i);
    const LdsOff o = sstore_ks_off(tid, i);
    *reinterpret_cast<u32x4*>(lds + o.row + o.in_row) = v;
  }
}

// ---- LDS -> MFMA fragments (32x32x16) of the 32-row sub-tile starting at `rbase`, k16-chunk kc --------
__device__ __forceinline__ bf16x8_t frag_direct(const char* lds, int rbase, int kc, int lane) {
  return *reinterpret_cast<const bf16x8_t*>(lds + opimg::frag_direct<false>(rbase, kc, lane));
}
__device__ __forceinline__ bf16x8_t frag_ks(const char* lds, int rbase, int kc, int lane) {
  const char* p = lds + opimg::frag_ks<KS_PITCH * 2, false, false>(rbase, kc, lane);
  return tr16_frag(p, 4 * (KS_PITCH * 2));
}

// a thread stores the chunks it loaded (gload_*: chunk tid & 7 of rows (tid >> 3) + 32 i / rows 8 (tid & 15) .. of k-rows
// (tid >> 4) + 16 i) at their image addresses
constexpr bool gb_maps_follow_image() {
  for (int tid = 0; tid < NT; ++tid)
    for (int i = 0; i < 4; ++i) {
      const LdsOff d = sstore_direct_off(tid, i), k = sstore_ks_off(tid, i);
      if (d.row + d.in_row != opimg::direct_chunk((tid >> 3) + 32 * i, tid & 7)) return false;
      if (k.row + k.in_row != opimg::ks_at<KS_PITCH * 2, false>((tid >> 4) + 16 * i, (tid & 15) * 8)) return false;
    }
  return true;
}
static_assert(gb_maps_follow_image(), "gemm_bf16.hip: sstore_*_off must be the image addresses of gemm_operand_image.h");

template <bool A_KS, bool B_KS, bool A_F32, bool FAST>
__global__ __launch_bounds__(NT) void gemm_bf16_kernel(Args g) {
  constexpr int SZA = A_KS ? SZ_KS : SZ_DIRECT;
  constexpr int SZB = B_KS ? SZ_KS : SZ_DIRECT;
  __shared__ __attribute__((aligned(16))) char smem[2 * (SZA + SZB)];
  using TA = typename std::conditional<A_F32, float, bf16_t>::type;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wg = opimg::xcd_chunked(bid, nwg);   // each XCD walks a contiguous run of tiles
  const int64_t n0 = (int64_t)(wg % g.nbx) * BN, m0 = (int64_t)(wg / g.nbx) * BM;
  const int64_t z = blockIdx.z, z1 = z / g.nb2, z2 = z % g.nb2;
  const TA* A = reinterpret_cast<const TA*>(g.A) + z1 * g.bsA1 + z2 * g.bsA2;
  const bf16_t* B = g.B + z1 * g.bsB1 + z2 * g.bsB2;
  const int64_t coff = z1 * g.bsC1 + z2 * g.bsC2;
  const int64_t roff = z1 * g.bsR1 + z2 * g.bsR2;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int64_t kbeg = (int64_t)blockIdx.y * g.kper;
  const int64_t kend = kbeg + g.kper < g.K ? kbeg + g.kper : g.K;
  const int64_t nk = (kend - kbeg + BK - 1) / BK;

  Stage<TA> sa;
  Stage<bf16_t> sb;
  auto gload = [&](int64_t k0) {
    if constexpr (FAST) {
      if constexpr (A_KS) gload_ks_fast<TA>(sa, A, g.lda, m0, g.M, k0, kend, tid);
      else gload_direct_fast<TA>(sa, A, g.lda, m0, g.M, k0, kend, tid);
      if constexpr (B_KS) gload_ks_fast<bf16_t>(sb, B, g.ldb, n0, g.N, k0, kend, tid);
      else gload_direct_fast<bf16_t>(sb, B, g.ldb, n0, g.N, k0, kend, tid);
    } else {
      if constexpr (A_KS) gload_ks_slow<TA>(sa, A, g.lda, m0, g.M, k0, kend, tid);
      else gload_direct_slow<TA>(sa, A, g.lda, m0, g.M, k0, kend, tid);
      if constexpr (B_KS) gload_ks_slow<bf16_t>(sb, B, g.ldb, n0, g.N, k0, kend, tid);
      else gload_direct_slow<bf16_t>(sb, B, g.ldb, n0, g.N, k0, kend, tid);
    }
  };
  auto sstore = [&](int buf) {
    char* la = smem + buf * (SZA + SZB);
    char* lb = la + SZA;
    if constexpr (A_KS) sstore_ks(sa, la, tid); else sstore_direct(sa, la, tid);
    if constexpr (B_KS) sstore_ks(sb, lb, tid); else sstore_direct(sb, lb, tid);
  };

  gload(kbeg);
  sstore(0);
  __syncthreads();
  for (int64_t t = 0; t < nk; ++t) {
    const int buf = (int)(t & 1);
    if (t + 1 < nk) gload(kbeg + (t + 1) * BK);
    const char* la = smem + buf * (SZA + SZB);
    const char* lb = la + SZA;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      bf16x8_t a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        a[i] = A_KS ? frag_ks(la, wm * 64 + i * 32, kc, lane) : frag_direct(la, wm * 64 + i * 32, kc, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j] = B_KS ? frag_ks(lb, wn * 64 + j * 32, kc, lane) : frag_direct(lb, wn * 64 + j * 32, kc, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (t + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }

  // C/D map of a 32x32 tile: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  if (g.splits > 1) {
    const int li = lane & 31, lk = lane >> 5;
    float* slab = g.slab + ((int64_t)blockIdx.y * gridDim.z + z) * g.M * g.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t n = n0 + wn * 64 + j * 32 + li;
        if (n >= g.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (m < g.M) slab[m * g.N + n] = acc[i][j][r];
        }
      }
    return;
  }
  const bool full = m0 + BM <= g.M && n0 + BN <= g.N && ((g.ldc | g.ldaux | coff) & 1) == 0;
  if (g.c_dtype == SEGCLIP_BF16) {
    if (full) epilogue_mode<bf16_t, true>(g, acc, m0, n0, wm, wn, lane, coff, roff);
    else epilogue_mode<bf16_t, false>(g, acc, m0, n0, wm, wn, lane, coff, roff);
  } else {
    if (full) epilogue_mode<float, true>(g, acc, m0, n0, wm, wn, lane, coff, roff);
    else epilogue_mode<float, false>(g, acc, m0, n0, wm, wn, lane, coff, roff);
  }
}

#if GB_PART == 4
// C = alpha * sum_s slab[s]  (split-K combine; deterministic order)
__global__ void splitk_reduce_kernel(const float* __restrict__ slab, void* C, int64_t M, int64_t N, int64_t ldc,
                                     int64_t nb2, int64_t bsC1, int64_t bsC2, int splits, int64_t nz, float alpha,
                                     int c_dtype) {
  const int64_t total = nz * M * N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += slab[(int64_t)s * total + i];
    v *= alpha;
    const int64_t z = i / (M * N), rem = i % (M * N), m = rem / N, n = rem % N;
    const int64_t o = (z / nb2) * bsC1 + (z % nb2) * bsC2 + m * ldc + n;
    if (c_dtype == SEGCLIP_BF16) ((bf16_t*)C)[o] = f2bf(v); else ((float*)C)[o] = v;
  }
}

// contiguous fp32/bf16 C (ldc == N, one batch): 16-byte loads, four slabs in flight, no index arithmetic
__global__ __launch_bounds__(256) void splitk_reduce_vec_kernel(const float* __restrict__ slab, void* __restrict__ C,
                                                                int64_t total4, int splits, float alpha, int c_dtype) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(slab) + i;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  int s = 0;
#pragma unroll 1
  for (; s + 8 <= splits; s += 8) {
    f32x4 t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = p[(int64_t)(s + u) * total4];
    v += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
  }
  if (s + 4 <= splits) {
    const f32x4 a = p[(int64_t)s * total4], b = p[(int64_t)(s + 1) * total4], c = p[(int64_t)(s + 2) * total4],
                d = p[(int64_t)(s + 3) * total4];
    v += (a + b) + (c + d);
    s += 4;
  }
  for (; s < splits; ++s) v += p[(int64_t)s * total4];
  v *= alpha;
  if (c_dtype == SEGCLIP_BF16)
    reinterpret_cast<u32x2*>(C)[i] = u32x2{pack2bf(v.x, v.y), pack2bf(v.z, v.w)};
  else
    reinterpret_cast<f32x4*>(C)[i] = v;
}

#endif  // GB_PART == 4 (reduction kernels)
}  // namespace

// Compiled once per GB_PART (build.sh), like gemm_bf16_p8.hip: parts 0..3 hold the four kernel instances (fp32 / bf16
// left operand x aligned / ragged) of one operand layout <A_KS = part>>1, B_KS = part&1> behind a launcher; part 4 is
// the split-K reduction kernels, the family's launcher and the trailing reductions of segclip_gemm.
#ifndef GB_PART
#error "compile with -DGB_PART=0..4 (see build.sh)"
#endif
// route variant (gemm_plan.cpp): bit 0 = fp32 A operand, bit 1 = 16-byte aligned (unguarded) operand loads
#define GB_LAUNCHER(NAME, AK, BKS)                                                                    \
  void NAME(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream) {                      \
    typedef void (*kernel_t)(Args);                                                                   \
    static const kernel_t kernels[2][2] = {{gemm_bf16_kernel<AK, BKS, true, true>, gemm_bf16_kernel<AK, BKS, true, false>},   \
                                           {gemm_bf16_kernel<AK, BKS, false, true>, gemm_bf16_kernel<AK, BKS, false, false>}}; \
    const int v = p.route.variant;   /* [bf16 A][ragged]: the order in which the code object holds the instances */  \
    hipLaunchKernelGGL(kernels[!(v & 1)][!(v & 2)], gemm_grid(p), dim3(NT), 0, stream, gemm_args(d, p));               \
  }
#if GB_PART == 0
GB_LAUNCHER(segclip_gb_launch_ff, false, false)
#elif GB_PART == 1
GB_LAUNCHER(segclip_gb_launch_fk, false, true)
#elif GB_PART == 2
GB_LAUNCHER(segclip_gb_launch_kf, true, false)
#elif GB_PART == 3
GB_LAUNCHER(segclip_gb_launch_kk, true, true)
#endif

#if GB_PART == 4
void segclip_gb_launch_ff(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_gb_launch_fk(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_gb_launch_kf(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
void segclip_gb_launch_kk(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);

void segclip_gemm_launch_generic(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream) {
  static const gemm_layout_launcher layouts[4] = {segclip_gb_launch_ff, segclip_gb_launch_fk, segclip_gb_launch_kf, segclip_gb_launch_kk};
  layouts[gemm_layout_index(p)](d, p, stream);
}

// after the GEMM kernel of any bf16 family: the column-sum reduction and the split-K combine, unless the caller deferred them
int segclip_gemm_launch_reductions(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream) {
  if (p.colsum && !(d->flags & SEGCLIP_GEMM_DEFER_COLSUM)) {
    launch_reduce_rows((const float*)d->colsum_ws, d->M / 64, d->N, d->N, d->colsum, nullptr, nullptr, d->N, stream);
    SEGCLIP_CHECK_LAUNCH("gemm_colsum_reduce");
  }
  if (p.route.splits > 1 && !(d->flags & SEGCLIP_GEMM_DEFER_SPLITK)) {
    const int64_t total = p.nb * d->M * d->N;
    const int blocks = (int)(cdiv(total, 256) < 2048 ? cdiv(total, 256) : 2048);
    const int64_t cal = d->c_dtype == SEGCLIP_BF16 ? 7 : 15;
    if (p.nb == 1 && d->ldc == d->N && total % 4 == 0 && (reinterpret_cast<uintptr_t>(d->C) & cal) == 0 &&
        (reinterpret_cast<uintptr_t>(d->ws) & 15) == 0)
      hipLaunchKernelGGL(splitk_reduce_vec_kernel, dim3((unsigned)cdiv(total / 4, 256)), dim3(256), 0, stream,
                         (const float*)d->ws, d->C, total / 4, p.route.splits, d->alpha, d->c_dtype);
    else
      hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, stream, (const float*)d->ws, d->C, d->M,
                       d->N, d->ldc, d->nb2 > 0 ? d->nb2 : 1, d->bsC1, d->bsC2, p.route.splits, p.nb, d->alpha, d->c_dtype);
    SEGCLIP_CHECK_LAUNCH("splitk_reduce");
  }
  return 0;
}
#endif  // GB_PART == 4
