// Top-K image-text search (included at the end of retrieval.hip): for queries Q (Nq, E) and a gallery X (Nx, E), the first
// min(k, Nx) gallery rows of every query under "higher score first, equal scores: lower index first", with their scores, and
// no (Nq, Nx) array.  The product is tile_product, so a score is the very number the count pass compares; the epilogue selects.
//   key = ord_key(score) << 32 | (0xFFFFFFFF - index): one unsigned order, total, 0 = empty (no real key is 0: index < 2^24)
// A workgroup keeps 128 queries and a sorted list of 64 keys per query in LDS (64 KiB) while it walks the gallery tiles of its
// split (blockIdx.y).  The list's first k keys are always the k best of what the row has seen; its k-th key is the admission
// threshold, and a candidate that does not beat it can never be among the k best.  Only vector stores, plain C++ and builtins.
#include <atomic>

namespace {

constexpr int TOPK_MAX = 64;           // k <= 64: a list is one key per lane
constexpr int TOPK_MAX_SPLITS = 64;    // auto: the workspace stays a small multiple of the outputs
constexpr size_t TOPK_OPERAND_BYTES = 2 * BK * PITCH * sizeof(float);            // As and Bs; the parked scores alias them
constexpr size_t TOPK_LDS_BYTES = TOPK_OPERAND_BYTES + (size_t)BT * TOPK_MAX * 8;   // 33,024 + 65,536 of the 160 KiB of a CU
static_assert(BT * 64 * sizeof(float) <= TOPK_OPERAND_BYTES, "a [128 x 64] score sub-block fits the operand slices");
static_assert(TOPK_OPERAND_BYTES % 16 == 0, "the lists are 16-byte aligned");

__device__ __forceinline__ uint64_t topk_key(float s, int col) {
  return ((uint64_t)ord_key(s) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)col);
}
__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// one key per lane, bitonic -> descending (lane 0 the largest): 6 exchange stages
__device__ __forceinline__ uint64_t wave_bitonic_merge(uint64_t v, int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const uint64_t o = __shfl_xor(v, j, 64);
    v = (lane & j) == 0 ? max_u64(v, o) : min_u64(v, o);
  }
  return v;
}
// one key per lane, any order -> descending: the 21 exchange stages of a bitonic sort
__device__ __forceinline__ uint64_t wave_sort(uint64_t v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint64_t o = __shfl_xor(v, j, 64);
      v = ((lane & j) == 0) == ((lane & k) == 0) ? max_u64(v, o) : min_u64(v, o);
    }
  return v;
}
// two descending lists -> the 64 largest keys of both, descending: max(list[i], cand[63 - i]) is bitonic and holds them
__device__ __forceinline__ uint64_t wave_merge_lists(uint64_t list, uint64_t cand, int lane) {
  return wave_bitonic_merge(max_u64(list, __shfl(cand, 63 - lane, 64)), lane);
}

__device__ __forceinline__ void topk_write(uint64_t key, int32_t* idx, float* val) {
  *idx = key != 0 ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
  *val = key != 0 ? ord_val((uint32_t)(key >> 32)) : -INFINITY;
}

struct TopkArgs {
  const float* Q; const float* X; int32_t* idx; float* val; uint64_t* ws;
  int Nq, Nx, E, k, tiles;
};

// blockIdx.x: a tile of 128 queries; blockIdx.y: the split, which strides over the tiles of 128 gallery rows.  Wave w owns the
// lists of rows 32 w .. 32 w + 31 from the first to the last instruction: no barrier guards them.  After a tile's product the
// accumulators are parked in LDS in two sub-blocks of 64 columns (sub-block j = the j-th 32 columns of either wave column;
// any partition serves, the key carries the index), over the operand slices behind the product's closing barrier.  A wave then
// takes its rows in turn, a lane holding one candidate: one ballot against the threshold skips the row; otherwise the 64
// candidates are sorted and merged into the list.  One split: the lists are the result.  Several: they go to the workspace,
// (padded query, split, k) keys, and retrieval_topk_merge_kernel finishes.
__global__ __launch_bounds__(NT) void retrieval_topk_kernel(TopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
  float* As = reinterpret_cast<float*>(topk_lds);
  float* Bs = As + BK * PITCH;
  float* sc = As;   // [128][64] parked scores
  uint64_t* lists = reinterpret_cast<uint64_t*>(topk_lds + TOPK_OPERAND_BYTES);   // [128][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lk = lane >> 5;
  const int m0 = blockIdx.x * BT, splits = gridDim.y;
  const int own = min(32, a.Nq - m0 - wave * 32);   // the wave's rows that are queries (<= 0: none)

  for (int r = 0; r < 32; ++r) lists[(wave * 32 + r) * TOPK_MAX + lane] = 0;
  for (int it = blockIdx.y; it < a.tiles; it += splits) {
    const int n0 = it * BT;
    f32x16 acc[2][2];
    tile_product(a.Q, m0, a.Nq, a.X, n0, a.Nx, a.E, As, Bs, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          sc[(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk) * 64 + wn * 32 + li] = acc[i][j][r];
      __syncthreads();
      const int col = n0 + lk * 64 + j * 32 + li;
      for (int r = 0; r < own; ++r) {
        const int row = wave * 32 + r;
        uint64_t* list = lists + row * TOPK_MAX;
        uint64_t key = col < a.Nx ? topk_key(sc[row * 64 + lane], col) : 0;
        const uint64_t thr = list[a.k - 1];
        if (__ballot(key > thr) == 0) continue;
        key = key > thr ? key : 0;
        list[lane] = wave_merge_lists(list[lane], wave_sort(key, lane), lane);
      }
      __syncthreads();   // the scores are read: the next sub-block, or the next tile's operands, may overwrite them
    }
  }
  if (lane < a.k)
    for (int r = 0; r < 32; ++r) {
      const int row = wave * 32 + r;
      const int64_t q = m0 + row;
      const uint64_t key = lists[row * TOPK_MAX + lane];
      if (splits > 1) a.ws[(q * splits + blockIdx.y) * a.k + lane] = key;
      else if (q < a.Nq) topk_write(key, a.idx + q * a.k + lane, a.val + q * a.k + lane);
    }
}

// one wave per query: the S sorted partial lists of k keys -> idx, val.  S = 0 writes the padding alone.
__global__ __launch_bounds__(256) void retrieval_topk_merge_kernel(const uint64_t* __restrict__ ws, int S, int Nq, int k,
                                                                   int32_t* idx, float* val) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= Nq) return;
  uint64_t v = 0;
  for (int s = 0; s < S; ++s) v = wave_merge_lists(v, lane < k ? ws[(q * S + s) * k + lane] : 0, lane);
  if (lane < k) topk_write(v, idx + q * k + lane, val + q * k + lane);
}

int topk_check(const char* what, int64_t Nq, int64_t Nx, int64_t k, int64_t splits) {
  if (k < 1 || k > TOPK_MAX) {
    segclip_set_error("%s: k=%lld: k lies in [1, %d]", what, (long long)k, TOPK_MAX);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  if (Nq < 0 || Nq >= (1 << 24)) {
    segclip_set_error("%s: Nq=%lld: the query count Nq lies in [0, 2^24)", what, (long long)Nq);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  if (Nx < 0 || Nx >= (1 << 24)) {
    segclip_set_error("%s: Nx=%lld: the gallery size Nx lies in [0, 2^24)", what, (long long)Nx);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  SEGCLIP_REQUIRE(splits >= 0, "%s: splits=%lld: 0 (auto) or the number of partial lists", what, (long long)splits);
  return 0;
}

// the partial lists of a call.  Auto: as many as fill the CUs with one workgroup each (the LDS admits one), so that a call
// with few queries still uses the device; at most 64.  Never more than there are gallery tiles.
int64_t topk_splits(int64_t Nq, int64_t Nx, int64_t splits) {
  const int64_t tiles = cdiv(Nx, BT), q_tiles = cdiv(Nq, BT);
  if (tiles == 0 || q_tiles == 0) return 1;
  if (splits == 0) {
    int dev = 0, ncu = 256;
    if (!segclip_current_device(&dev, &ncu)) ncu = 256;
    splits = ncu / q_tiles;
    splits = splits < 1 ? 1 : splits > TOPK_MAX_SPLITS ? TOPK_MAX_SPLITS : splits;
  }
  splits = splits < tiles ? splits : tiles;
  return splits < 65535 ? splits : 65535;
}

int64_t topk_ws_bytes(int64_t Nq, int64_t k, int64_t splits) { return splits > 1 ? cdiv(Nq, BT) * BT * splits * k * 8 : 0; }

}  // namespace

extern "C" int64_t segclip_retrieval_topk_ws_bytes(int64_t Nq, int64_t Nx, int64_t k, int64_t splits) {
  if (int rc = topk_check("retrieval_topk_ws_bytes", Nq, Nx, k, splits)) return rc;   // negative
  return topk_ws_bytes(Nq, k, topk_splits(Nq, Nx, splits));
}

extern "C" int segclip_retrieval_topk(const float* Q, const float* X, int64_t Nq, int64_t Nx, int64_t E, int64_t k, int64_t splits,
                                      int32_t* idx, float* val, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = topk_check("retrieval_topk", Nq, Nx, k, splits)) return rc;
  if (E < 32 || E % 32 != 0 || E > 1024) {
    segclip_set_error("retrieval_topk: E=%lld: the embedding width E is a multiple of 32 and at most 1024", (long long)E);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  if (((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(X)) & 15) != 0) {
    segclip_set_error("retrieval_topk: Q=%p, X=%p: the rows are 16-byte aligned", (const void*)Q, (const void*)X);
    return SEGCLIP_ERR_UNSUPPORTED;
  }
  if (Nq == 0) return 0;
  SEGCLIP_REQUIRE(idx != nullptr && val != nullptr, "retrieval_topk: idx and val are required");
  const int S = (int)topk_splits(Nq, Nx, splits);
  const int64_t need = topk_ws_bytes(Nq, k, S);
  SEGCLIP_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
                  "retrieval_topk: workspace_bytes=%lld: segclip_retrieval_topk_ws_bytes asks for %lld", (long long)workspace_bytes,
                  (long long)need);
  SEGCLIP_REQUIRE(need == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "retrieval_topk: the workspace is 8-byte aligned");
  uint64_t* ws = reinterpret_cast<uint64_t*>(workspace);
  if (Nx > 0) {
    int dev = 0, ncu = 0;
    SEGCLIP_REQUIRE(segclip_current_device(&dev, &ncu), "retrieval_topk: cannot query the current device");
    static std::atomic<bool> raised[64];
    if (!raised[dev]) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(retrieval_topk_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOPK_LDS_BYTES);
      SEGCLIP_REQUIRE(e == hipSuccess, "retrieval_topk: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
      raised[dev] = true;
    }
    TopkArgs a;
    a.Q = Q; a.X = X; a.idx = idx; a.val = val; a.ws = ws;
    a.Nq = (int)Nq; a.Nx = (int)Nx; a.E = (int)E; a.k = (int)k; a.tiles = (int)cdiv(Nx, BT);
    hipLaunchKernelGGL(retrieval_topk_kernel, dim3((unsigned)cdiv(Nq, BT), (unsigned)S), dim3(NT), TOPK_LDS_BYTES, ST, a);
    SEGCLIP_CHECK_LAUNCH("retrieval_topk");
  }
  if (Nx == 0 || S > 1) {
    hipLaunchKernelGGL(retrieval_topk_merge_kernel, dim3((unsigned)cdiv(Nq, 4)), dim3(256), 0, ST, ws, Nx == 0 ? 0 : S, (int)Nq,
                       (int)k, idx, val);
    SEGCLIP_CHECK_LAUNCH("retrieval_topk (merge)");
  }
  return 0;
}
