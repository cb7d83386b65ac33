// Majority voting of label maps inside segments (segment.hip): every segment of a segment map (superpixels, or ids of the
// caller's own) gives its pixels the label most of them carry, for maps of mixed sizes in one call.  The reference has no such
// op: the definition is this project's (include/segclip_hip.h, segclip_seg_vote) and tests/superpixel_reference.py restates it.
//   seg_vote_count_kernel  : the (segment, class) pairs of SEG_VOTE_TILE consecutive pixels, counted into the (K_total, C) int32
//                            table of the workspace
//   seg_vote_winner_kernel : one wave per segment: lane l takes the classes l, l + 64, ...; a shuffle reduction to the largest
//                            count, among equal counts the lowest class (as segment_wide.inc resolves a pixel), and the total
//                            -> the winner, or -1 for a segment that has no voter or does not reach min_share
//   seg_vote_apply_kernel  : the output map
// Counting: a caller's segment map gives no bound on the segments of a tile, so the workgroup's stage in LDS is the open-
// addressing table of segment_confusion.inc's sparse route: SEG_VOTE_SLOTS (key, count) slots (8 KiB static), key =
// segment * C + class < 2^30, claimed with a compare-and-swap, linear probing, SEG_VOTE_PROBES probes; a pair that finds no slot
// is added to the global table at once, so the counts are exact whatever the map holds.  A lane owns SEG_VOTE_RUN consecutive
// pixels and counts equal consecutive pairs once.  The flush is one global integer atomic per (tile, pair).  Integer counts: no
// dependence on the order of arrival.
// Traffic per pixel: count 4 + 1 (or 2) B read, apply 4 + 1 (2) B read, the winner gathered, 1 (2) B written; K_total * C * 4 B
// of table cleared and read once.  Measured on 12.0 M pixels, 48,896 superpixels, 21 classes (profiles/seg_snap.txt): count
// 44.6 us (1.35 TB/s of that traffic), winner 12.2 us, apply 27.3 us (2.64 TB/s, 0.33 of the HBM peak).
// The kernels that read or write labels are templates on the label element L (uint8_t, or uint16_t for int16 tensors read as
// unsigned).  Plain C++, no inline assembly.  gfx950 (hipcc -Rpass-analysis=kernel-resource-usage): at the kernels below.

#define SEG_VOTE_COLS SEGCLIP_SEG_VOTE_COLS   // int64 columns of one image row of the table (segclip_hip.h)
#define SEG_VOTE_TILE SEGCLIP_SEG_VOTE_TILE   // pixels of one workgroup
#define SEG_VOTE_MAX_K SEGCLIP_SEG_VOTE_MAX_SEGMENTS
#define SEG_VOTE_THREADS 256
#define SEG_VOTE_RUN (SEG_VOTE_TILE / SEG_VOTE_THREADS)
#define SEG_VOTE_SLOTS 1024                   // a power of two: half a tile's pixels, far above the pairs of a tile of a real map
#define SEG_VOTE_SLOT_BITS 10
#define SEG_VOTE_PROBES 8
#define SEG_VOTE_EMPTY 0xffffffffu            // no key: segment * C + class < 2^20 * 2^10
enum { VT_OFF, VT_N, VT_SEG, VT_K, VT_BLK };
static_assert(SEG_VOTE_TILE % SEG_VOTE_THREADS == 0 && (1 << SEG_VOTE_SLOT_BITS) == SEG_VOTE_SLOTS, "seg_vote tile");
static_assert((long long)SEG_VOTE_MAX_K * SEG_WIDE_MAX_CLASSES <= (1ll << 30), "seg_vote key");

struct SegVoteArgs {
  const int64_t* images;    // (B, SEG_VOTE_COLS)
  const void* labels;       // flat, elements of L
  const int32_t* seg;       // flat segment ids, the labels' offsets
  void* out;                // flat, elements of L, the labels' offsets
  int32_t* cnt;             // (K_total, C)
  int32_t* win;             // (K_total)
  int64_t n, K_total, n_blocks;   // n: elements of labels, seg and out
  int B, C, max_k, min_share;
};

// The pixels of one workgroup, range-checked: the host entry cannot inspect device memory.
struct SegVoteTile { int64_t off, p0, total, k0; int K; bool ok; };
__device__ __forceinline__ SegVoteTile seg_vote_tile(const SegVoteArgs& A, int img) {
  const int64_t* D = A.images + (int64_t)img * SEG_VOTE_COLS;
  const int64_t total = D[VT_N], K = D[VT_K], blk = D[VT_BLK];
  SegVoteTile T;
  T.off = D[VT_OFF]; T.k0 = D[VT_SEG];
  T.ok = total >= 1 && total < (1ll << 30) && T.off >= 0 && T.off <= A.n - total && K >= 1 && K <= A.max_k && K <= SEG_VOTE_MAX_K &&
         T.k0 >= 0 && T.k0 <= A.K_total - K;
  T.total = T.ok ? total : 0; T.K = T.ok ? (int)K : 0;
  const int64_t tiles = (T.total + SEG_VOTE_TILE - 1) / SEG_VOTE_TILE;
  T.ok = T.ok && blk >= 0 && blk <= A.n_blocks - tiles;
  T.p0 = ((int64_t)blockIdx.x - blk) * SEG_VOTE_TILE;
  if (T.p0 < 0 || T.p0 >= T.total) T.ok = false;
  return T;
}

// a key goes from EMPTY to its pair once and never changes again (seg_conf_count)
__device__ __forceinline__ void seg_vote_count(uint32_t* s, int32_t* cnt, uint32_t key, int n) {
  uint32_t slot = (key * 2654435761u) >> (32 - SEG_VOTE_SLOT_BITS);
  for (int i = 0; i < SEG_VOTE_PROBES; ++i, slot = (slot + 1) & (SEG_VOTE_SLOTS - 1)) {
    uint32_t k = __hip_atomic_load(&s[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == SEG_VOTE_EMPTY) k = atomicCAS(&s[slot], SEG_VOTE_EMPTY, key);
    if (k == SEG_VOTE_EMPTY || k == key) {
      atomicAdd(&s[SEG_VOTE_SLOTS + slot], (uint32_t)n);
      return;
    }
  }
  atomicAdd(&cnt[key], n);
}

// gfx950: <uint8_t> 17 VGPRs, <uint16_t> 17; scratch 0; LDS 8,196 bytes static; 8 waves per SIMD
template <class L>
__global__ __launch_bounds__(SEG_VOTE_THREADS) void seg_vote_count_kernel(SegVoteArgs A) {
  __shared__ int s_img;
  __shared__ uint32_t s_tab[2 * SEG_VOTE_SLOTS];   // keys | counts
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_VOTE_COLS, VT_BLK, (int64_t)blockIdx.x);
  for (int i = tid; i < 2 * SEG_VOTE_SLOTS; i += SEG_VOTE_THREADS) s_tab[i] = i < SEG_VOTE_SLOTS ? SEG_VOTE_EMPTY : 0u;
  __syncthreads();
  const SegVoteTile T = seg_vote_tile(A, s_img);
  if (!T.ok) return;  // block-uniform
  const L* lab = static_cast<const L*>(A.labels) + T.off;
  const int32_t* seg = A.seg + T.off;
  int32_t* cnt = A.cnt + T.k0 * A.C;   // the image's rows: key = segment * C + class indexes them
  const int64_t p = T.p0 + (int64_t)tid * SEG_VOTE_RUN;
  uint32_t key = SEG_VOTE_EMPTY;
  int n = 0;
#pragma unroll
  for (int e = 0; e < SEG_VOTE_RUN; ++e) {
    if (p + e >= T.total) break;
    const int c = (int)lab[p + e], s = seg[p + e];
    if (c >= A.C || s < 0 || s >= T.K) continue;   // no voter
    const uint32_t k = (uint32_t)s * (uint32_t)A.C + (uint32_t)c;
    if (k == key) { ++n; continue; }
    if (n) seg_vote_count(s_tab, cnt, key, n);
    key = k; n = 1;
  }
  if (n) seg_vote_count(s_tab, cnt, key, n);
  __syncthreads();
  for (int i = tid; i < SEG_VOTE_SLOTS; i += SEG_VOTE_THREADS)
    if (s_tab[i] != SEG_VOTE_EMPTY && s_tab[SEG_VOTE_SLOTS + i]) atomicAdd(&cnt[s_tab[i]], (int32_t)s_tab[SEG_VOTE_SLOTS + i]);
}

// Every one of the K_total rows gets its winner, also the rows no image of the table owns (they are all zero: -1).
// gfx950: 12 VGPRs, scratch 0, LDS 0
__global__ __launch_bounds__(SEG_VOTE_THREADS) void seg_vote_winner_kernel(SegVoteArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * (SEG_VOTE_THREADS / 64) + (threadIdx.x >> 6);
  if (k >= A.K_total) return;  // wave-uniform
  const int32_t* row = A.cnt + k * A.C;
  int top = 0, arg = 0x7fffffff, tot = 0;
  for (int c = lane; c < A.C; c += 64) {
    const int v = row[c];
    tot += v;
    if (v > top) { top = v; arg = c; }   // ascending c: the first class that reaches the lane's maximum
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int ot = __shfl_xor(top, d, 64), oa = __shfl_xor(arg, d, 64);
    tot += __shfl_xor(tot, d, 64);
    if (ot > top || (ot == top && oa < arg)) { top = ot; arg = oa; }
  }
  if (lane == 0) {
    const bool snaps = tot > 0 && 100ll * top >= (long long)A.min_share * tot;
    A.win[k] = snaps ? arg : -1;
  }
}

// gfx950: <uint8_t> 17 VGPRs, <uint16_t> 17; scratch 0; LDS 4 bytes
template <class L>
__global__ __launch_bounds__(SEG_VOTE_THREADS) void seg_vote_apply_kernel(SegVoteArgs A) {
  __shared__ int s_img;
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_VOTE_COLS, VT_BLK, (int64_t)blockIdx.x);
  __syncthreads();
  const SegVoteTile T = seg_vote_tile(A, s_img);
  if (!T.ok) return;  // block-uniform
  const L* lab = static_cast<const L*>(A.labels) + T.off;
  L* out = static_cast<L*>(A.out) + T.off;
  const int32_t* seg = A.seg + T.off;
  const int32_t* win = A.win + T.k0;
  // consecutive lanes consecutive pixels
#pragma unroll
  for (int e = 0; e < SEG_VOTE_RUN; ++e) {
    const int64_t p = T.p0 + e * SEG_VOTE_THREADS + tid;
    if (p >= T.total) break;
    const int c = (int)lab[p], s = seg[p];
    int v = c;
    if (c < A.C && s >= 0 && s < T.K) {
      const int w = win[s];
      if (w >= 0) v = w;
    }
    out[p] = (L)v;
  }
}
