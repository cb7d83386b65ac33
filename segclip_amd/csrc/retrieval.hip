// Image-text retrieval evaluation (Recall@K, median and mean rank, both directions) without a similarity matrix.
//   V (Ni, E) image embeddings, T (Nt, E) caption embeddings, g (Nt) the image of every caption, sim[t, j] = <T[t], V[j]>
//   rank_t2i[t] = #{ j != g[t] : sim[t, j] > sim[t, g[t]] }
//   rank_i2t[j] = #{ t : g[t] != j and sim[t, j] > best[j] },  best[j] = max{ sim[t, j] : g[t] == j }
// Three entries: the thresholds (thr_t[t] = sim[t, g[t]], best = their segment maximum), the tiled count pass on the exact-f32
// matrix cores (v_mfma_f32_32x32x2_f32, the engine of gemm_f32.hip) whose epilogue compares instead of storing, and the
// histograms the metrics are read from.  Every sum that crosses a workgroup is an integer atomic: the result does not depend
// on scheduling.
#include "common.h"

namespace {

constexpr int NT = 256;           // 4 waves in a 2 x 2 arrangement, each 2 x 2 MFMA tiles of 32 x 32
constexpr int BT = 128;           // captions and images of a tile
constexpr int BK = 32;            // K-slice staged through LDS
constexpr int PITCH = BT + 1;     // k-major LDS image [k][row]: the one-float-per-lane MFMA operand is a conflict-free read
constexpr int NCH = BT * BK / (4 * NT);  // 16-byte chunks of a slice per thread
constexpr int HIST_LDS = 2048;    // ranks below it are counted in LDS first (a trained model's ranks are small)

#define RETRIEVAL_BAD_INDEX SEGCLIP_RETRIEVAL_BAD_INDEX     // status bit: a g[t] outside [0, Ni)

// order-preserving map of a float onto unsigned integers: the segment maximum is an integer atomicMax
__device__ __forceinline__ uint32_t ord_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_val(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void retrieval_init_kernel(uint32_t* best_key, int32_t* n_cap, int Ni) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < Ni) { best_key[j] = 0u; n_cap[j] = 0; }
}

// One lane per caption: the dot product as the k-ordered fmaf chain from 0 that the MFMA of the count pass forms for the same
// pair, so a threshold is the very number the tile would have produced.  A caption whose image index is out of range gets
// +inf (it counts nothing and is counted by no image) and sets the status bit.
__global__ __launch_bounds__(256) void retrieval_thr_kernel(const float* __restrict__ V, const float* __restrict__ T,
                                                            const int32_t* __restrict__ g, int Ni, int Nt, int E,
                                                            float* __restrict__ thr, uint32_t* best_key, int32_t* n_cap,
                                                            int32_t* status) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Nt) return;
  const int j = g[t];
  if (j < 0 || j >= Ni) {
    thr[t] = INFINITY;
    atomicOr(status, RETRIEVAL_BAD_INDEX);
    return;
  }
  const float4* a = reinterpret_cast<const float4*>(T + (int64_t)t * E);
  const float4* b = reinterpret_cast<const float4*>(V + (int64_t)j * E);
  float s = 0.f;
#pragma unroll 8
  for (int k = 0; k < E / 4; ++k) {
    const float4 x = a[k], y = b[k];
    s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
  }
  thr[t] = s;
  atomicMax(&best_key[j], ord_key(s));
  atomicAdd(&n_cap[j], 1);
}

// keys -> floats in place; an image without captions gets +inf: nothing is counted for it
__global__ __launch_bounds__(256) void retrieval_best_kernel(uint32_t* best_key, const int32_t* n_cap, int Ni) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Ni) return;
  reinterpret_cast<float*>(best_key)[j] = n_cap[j] > 0 ? ord_val(best_key[j]) : INFINITY;
}

// [BT x BK] slice of X (row-major, E floats per row, 16-byte aligned rows) -> registers; rows past nrows are zeros
__device__ __forceinline__ void slice_load(const float* __restrict__ X, int row0, int nrows, int k0, int E, int tid,
                                           float4 (&v)[NCH]) {
#pragma unroll
  for (int it = 0; it < NCH; ++it) {
    const int c = it * NT + tid, r = c / (BK / 4), kq = (c % (BK / 4)) * 4;
    v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + r < nrows) v[it] = *reinterpret_cast<const float4*>(X + (int64_t)(row0 + r) * E + (k0 + kq));
  }
}
__device__ __forceinline__ void slice_store(float* lds, int tid, const float4 (&v)[NCH]) {
#pragma unroll
  for (int it = 0; it < NCH; ++it) {
    const int c = it * NT + tid, r = c / (BK / 4), kq = (c % (BK / 4)) * 4;
    lds[(kq + 0) * PITCH + r] = v[it].x; lds[(kq + 1) * PITCH + r] = v[it].y;
    lds[(kq + 2) * PITCH + r] = v[it].z; lds[(kq + 3) * PITCH + r] = v[it].w;
  }
}

// acc = the [BT x BT] tile  A[m0.., :] B[n0.., :]^T  of two row-major (rows, E) matrices: gemm_f32.hip's 128 x 128 x 32 schedule
// (the next slice travels in registers while this one is multiplied).  Every entry is the k-ordered fmaf chain from 0.  C/D map
// of a 32 x 32 MFMA tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); acc[i][j] is the tile at rows
// wm * 64 + i * 32, columns wn * 64 + j * 32.  Ends behind a barrier: As and Bs are free again.
__device__ __forceinline__ void tile_product(const float* __restrict__ A, int m0, int M, const float* __restrict__ B, int n0,
                                             int N, int E, float* As, float* Bs, f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lk = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[NCH], rb[NCH];
  slice_load(A, m0, M, 0, E, tid, ra);
  slice_load(B, n0, N, 0, E, tid, rb);
  for (int k0 = 0; k0 < E; k0 += BK) {
    slice_store(As, tid, ra);
    slice_store(Bs, tid, rb);
    __syncthreads();
    if (k0 + BK < E) {
      slice_load(A, m0, M, k0 + BK, E, tid, ra);
      slice_load(B, n0, N, k0 + BK, E, tid, rb);
    }
#pragma unroll 4
    for (int kk = 0; kk < BK; kk += 2) {
      float x[2], y[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) x[i] = As[(kk + lk) * PITCH + wm * 64 + i * 32 + li];
#pragma unroll
      for (int j = 0; j < 2; ++j) y[j] = Bs[(kk + lk) * PITCH + wn * 64 + j * 32 + li];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[i], y[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
}

struct CountArgs {
  const float* V; const float* T; const int32_t* g; const float* thr; const float* best;
  int32_t* rank_t2i; int32_t* rank_i2t;
  int Ni, Nt, E, image_tiles;
};

// blockIdx.x: a tile of 128 captions, kept for the workgroup's life; blockIdx.y strides over the tiles of 128 images.
// Epilogue on tile_product's accumulators.  A lane owns two columns:
// its column hits are summed in registers.  The hits of a row lie in the 32 lanes of one half-wave: a ballot counts them.
// Both go to per-tile counters in LDS, and every row and column with hits gets ONE global integer add.
__global__ __launch_bounds__(NT) void retrieval_count_kernel(CountArgs a) {
  __shared__ __attribute__((aligned(16))) float As[BK * PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[BK * PITCH];
  __shared__ float s_thr[BT], s_best[BT];
  __shared__ int s_g[BT], s_row[BT], s_col[BT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lk = lane >> 5;
  const int m0 = blockIdx.x * BT;

  if (tid < BT) {
    const bool ok = m0 + tid < a.Nt;
    s_thr[tid] = ok ? a.thr[m0 + tid] : INFINITY;
    s_g[tid] = ok ? a.g[m0 + tid] : -1;
    s_row[tid] = 0;
  }
  for (int it = blockIdx.y; it < a.image_tiles; it += gridDim.y) {
    const int n0 = it * BT;
    if (tid >= BT) {
      const int c = tid - BT;
      s_best[c] = n0 + c < a.Ni ? a.best[n0 + c] : INFINITY;
      s_col[c] = 0;
    }
    f32x16 acc[2][2];
    // (the product's first barrier also publishes s_thr, s_g, s_best and the zeroed counters)
    tile_product(a.T, m0, a.Nt, a.V, n0, a.Ni, a.E, As, Bs, acc);

    int col_hits[2] = {0, 0};
    float bst[2];
    int n[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      n[j] = n0 + wn * 64 + j * 32 + li;
      bst[j] = s_best[wn * 64 + j * 32 + li];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        const float th = s_thr[row];
        const int gg = s_g[row];
        const bool row_ok = m0 + row < a.Nt;
        int lo = 0, hi = 0;   // hits of the row of the lower and of the upper half-wave
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float v = acc[i][j][r];
          const bool other = row_ok && n[j] < a.Ni && n[j] != gg;   // the ground-truth pair counts in neither direction
          col_hits[j] += (other && v > bst[j]) ? 1 : 0;
          const unsigned long long mk = __ballot(other && v > th);
          lo += __popc((unsigned)mk);
          hi += __popc((unsigned)(mk >> 32));
        }
        if (li == 0) {
          const int c = lk ? hi : lo;
          if (c) atomicAdd(&s_row[row], c);
        }
      }
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (col_hits[j]) atomicAdd(&s_col[wn * 64 + j * 32 + li], col_hits[j]);
    __syncthreads();
    if (tid >= BT) {
      const int c = tid - BT;
      if (s_col[c] != 0 && n0 + c < a.Ni) atomicAdd(&a.rank_i2t[n0 + c], s_col[c]);
    }
  }
  __syncthreads();
  if (tid < BT && s_row[tid] != 0 && m0 + tid < a.Nt) atomicAdd(&a.rank_t2i[m0 + tid], s_row[tid]);
}

// rank -> histogram bin, the small ranks through LDS; an image without captions leaves with rank -1 and in no bin
__global__ __launch_bounds__(256) void retrieval_hist_kernel(const int32_t* __restrict__ rank_t2i, int32_t* rank_i2t,
                                                             const int32_t* __restrict__ n_cap, int Ni, int Nt,
                                                             unsigned long long* hist_t2i, unsigned long long* hist_i2t) {
  __shared__ int s_t[HIST_LDS], s_i[HIST_LDS];
  const int tid = threadIdx.x;
  for (int b = tid; b < HIST_LDS; b += 256) s_t[b] = s_i[b] = 0;
  __syncthreads();
  const int step = gridDim.x * 256;
  for (int t = blockIdx.x * 256 + tid; t < Nt; t += step) {
    const int r = rank_t2i[t];
    if (r < 0 || r >= Ni) continue;   // (cannot happen with ranks of the count pass; the histogram has Ni bins)
    if (r < HIST_LDS) atomicAdd(&s_t[r], 1); else atomicAdd(&hist_t2i[r], 1ull);
  }
  for (int j = blockIdx.x * 256 + tid; j < Ni; j += step) {
    if (n_cap[j] <= 0) { rank_i2t[j] = -1; continue; }
    const int r = rank_i2t[j];
    if (r < 0 || r > Nt) continue;
    if (r < HIST_LDS) atomicAdd(&s_i[r], 1); else atomicAdd(&hist_i2t[r], 1ull);
  }
  __syncthreads();
  for (int b = tid; b < HIST_LDS; b += 256) {
    if (s_t[b] != 0 && b < Ni) atomicAdd(&hist_t2i[b], (unsigned long long)s_t[b]);
    if (s_i[b] != 0 && b <= Nt) atomicAdd(&hist_i2t[b], (unsigned long long)s_i[b]);
  }
}

int retrieval_check(const char* what, int64_t Ni, int64_t Nt, int64_t E, const void* V, const void* T) {
  if (E < 32 || E % 32 != 0 || E > 1024) {
    segclip_set_error("%s: E=%lld: the embedding width E is a multiple of 32 and at most 1024", what, (long long)E);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  if (Ni < 0 || Ni >= (1 << 24)) {
    segclip_set_error("%s: Ni=%lld: the image count Ni lies in [0, 2^24)", what, (long long)Ni);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  if (Nt < 0 || Nt >= (1 << 24)) {
    segclip_set_error("%s: Nt=%lld: the caption count Nt lies in [0, 2^24)", what, (long long)Nt);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  SEGCLIP_REQUIRE(((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(T)) & 15) == 0,
                  "%s: V and T are 16-byte aligned", what);
  return 0;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int segclip_retrieval_thresholds(const float* V, const float* T, const int32_t* g, int64_t Ni, int64_t Nt, int64_t E,
                                            float* thr_t, float* best, int32_t* n_cap, int32_t* status, void* stream) {
  if (int rc = retrieval_check("retrieval_thresholds", Ni, Nt, E, V, T)) return rc;
  SEGCLIP_REQUIRE(status != nullptr, "retrieval_thresholds: status is required");
  uint32_t* key = reinterpret_cast<uint32_t*>(best);
  if (Ni > 0) {
    hipLaunchKernelGGL(retrieval_init_kernel, dim3((unsigned)cdiv(Ni, 256)), dim3(256), 0, ST, key, n_cap, (int)Ni);
    SEGCLIP_CHECK_LAUNCH("retrieval_thresholds (init)");
  }
  if (Nt > 0) {
    hipLaunchKernelGGL(retrieval_thr_kernel, dim3((unsigned)cdiv(Nt, 256)), dim3(256), 0, ST, V, T, g, (int)Ni, (int)Nt, (int)E,
                       thr_t, key, n_cap, status);
    SEGCLIP_CHECK_LAUNCH("retrieval_thresholds");
  }
  if (Ni > 0) {
    hipLaunchKernelGGL(retrieval_best_kernel, dim3((unsigned)cdiv(Ni, 256)), dim3(256), 0, ST, key, n_cap, (int)Ni);
    SEGCLIP_CHECK_LAUNCH("retrieval_thresholds (best)");
  }
  return 0;
}

extern "C" int segclip_retrieval_count(const float* V, const float* T, const int32_t* g, const float* thr_t, const float* best,
                                       int64_t Ni, int64_t Nt, int64_t E, int32_t* rank_t2i, int32_t* rank_i2t, void* stream) {
  if (int rc = retrieval_check("retrieval_count", Ni, Nt, E, V, T)) return rc;
  if (Ni == 0 || Nt == 0) return 0;
  CountArgs a;
  a.V = V; a.T = T; a.g = g; a.thr = thr_t; a.best = best; a.rank_t2i = rank_t2i; a.rank_i2t = rank_i2t;
  a.Ni = (int)Ni; a.Nt = (int)Nt; a.E = (int)E; a.image_tiles = (int)cdiv(Ni, BT);
  const dim3 grid((unsigned)cdiv(Nt, BT), (unsigned)(a.image_tiles < 65535 ? a.image_tiles : 65535));
  hipLaunchKernelGGL(retrieval_count_kernel, grid, dim3(NT), 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("retrieval_count");
  return 0;
}

extern "C" int segclip_retrieval_hist(const int32_t* rank_t2i, int32_t* rank_i2t, const int32_t* n_cap, int64_t Ni, int64_t Nt,
                                      int64_t* hist_t2i, int64_t* hist_i2t, void* stream) {
  if (Ni < 0 || Ni >= (1 << 24)) {
    segclip_set_error("retrieval_hist: Ni=%lld: the image count Ni lies in [0, 2^24)", (long long)Ni);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  if (Nt < 0 || Nt >= (1 << 24)) {
    segclip_set_error("retrieval_hist: Nt=%lld: the caption count Nt lies in [0, 2^24)", (long long)Nt);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  const int64_t most = Ni > Nt ? Ni : Nt;
  if (most == 0) return 0;
  const int64_t blocks = cdiv(most, 256) < 256 ? cdiv(most, 256) : 256;
  hipLaunchKernelGGL(retrieval_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, ST, rank_t2i, rank_i2t, n_cap, (int)Ni, (int)Nt,
                     reinterpret_cast<unsigned long long*>(hist_t2i), reinterpret_cast<unsigned long long*>(hist_i2t));
  SEGCLIP_CHECK_LAUNCH("retrieval_hist");
  return 0;
}

#include "retrieval_topk.inc"   // segclip_retrieval_topk: the same product with a selecting epilogue
