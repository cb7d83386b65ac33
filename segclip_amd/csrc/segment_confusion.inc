// The confusion matrix of label maps (segment.hip): segclip_seg_confusion and segclip_seg_confusion_wide count the pairs
// (ground-truth class, predicted class) of n pixels into a (C + 1, C + 1) int64 matrix, row = ground truth, column = prediction,
// index C on either axis the "out of range" bin.  The ground-truth rule is seg_area_add's (segment_tile.inc), so segclip_seg_areas
// is a projection of the matrix: areas[0][c] = conf[c][c], areas[1][c] = the sum of column c, areas[2][c] = the sum of row c.
//
// Design (the kernel reads 2 or 4 bytes per pixel and is meant to sit on HBM reads; CDNA4: 160 KiB of LDS per CU, wave of 64):
//   - loads: a lane reads 16 bytes of `pred` and 16 bytes of `gt` per step (16 uint8 or 8 uint16 pixels), two steps in flight,
//     consecutive lanes consecutive vectors.  The body starts where `pred` is 16-byte aligned; `gt` is read with aligned 16-byte
//     loads where it is aligned there too, and as 16 bytes of element alignment otherwise (views into a flat label buffer start
//     at any element, the two independently: gfx950 serves such a global load, the compiler still emits one dwordx4).  The
//     elements before the body and after its last whole vector, fewer than two vectors, are counted one by one by workgroup 0.
//   - run-length counting: a lane counts equal consecutive (g, p) pairs once (SegConfRun, after SegAreaRun); a vector whose
//     elements all equal the first is one comparison.  Label maps are piecewise constant: LDS atomics stay far below the pixels.
//   - privatisation: per-workgroup 32-bit counters in dynamic LDS, one global 64-bit integer atomicAdd per touched cell at the
//     flush (integer sums: no dependence on the order of arrival).  Two routes, the host's choice (seg_conf_plan):
//       dense  (C <= 180): the whole (C + 1)^2 matrix, (C + 1)^2 * 4 bytes: 1.9 KiB at 21 classes, 26 KiB at 81, 90 KiB at 151,
//              128 KiB at 180 (a workgroup may have all 160 KiB of the CU; past 64 KiB the limit is raised with
//              hipFuncSetAttribute, and where that fails the sparse route is taken).
//       sparse (above, and every real 16-bit vocabulary): an open-addressing table of 4096 (cell, count) slots, 32 KiB.  A cell
//              is claimed with a compare-and-swap on its key, linear probing, 8 probes; a pair that finds no slot is added to
//              the global matrix at once.  A tile of a real label map holds a few dozen pairs; independent random labels hold
//              nearly one per pixel and are counted, exactly, mostly by the overflow path.
//   - grid: grid-stride over 16-byte vectors, 512 threads.  A workgroup is given at least max(16384, 2 x LDS cells) pixels, so
//     that zeroing and flushing its LDS image (16-byte stores; one read per cell) stay a fraction of its counting, and the grid
//     is at most CUs x min(4, 160 KiB / LDS bytes): one workgroup per CU at 151 classes, four (32 waves) on the small images.
//   - no overflow: one launch counts at most 2^30 pixels (the host entry splits a longer input, at multiples of 2^30 elements,
//     which keep the alignment), so no 32-bit counter and no lane's run length can pass 2^30 whatever the distribution.
// Plain C++, no inline assembly.  Registers, scratch and LDS (hipcc -Rpass-analysis=kernel-resource-usage): at the kernel below.

#define SEG_CONF_THREADS 512
#define SEG_CONF_DENSE_MAX_CLASSES 180      // 181^2 * 4 = 131,044 bytes <= 128 KiB
#define SEG_CONF_SLOTS 4096                 // a power of two
#define SEG_CONF_SLOT_BITS 12
#define SEG_CONF_PROBES 8
#define SEG_CONF_EMPTY 0xffffffffu          // no cell: (C + 1)^2 <= 1025^2
#define SEG_CONF_LAUNCH_PIXELS (1ll << 30)  // a multiple of 16
#define SEG_CONF_MIN_WG_PIXELS 16384

// 16 bytes of labels that are aligned to their element only
struct __attribute__((packed, aligned(1))) SegConfBytes16 { u32x4 v; };
struct __attribute__((packed, aligned(2))) SegConfShorts8 { u32x4 v; };

template <typename T> struct SegConfVec;
template <> struct SegConfVec<uint8_t> {
  static constexpr int N = 16;
  static constexpr uint32_t REP = 0x01010101u;
  static __device__ __forceinline__ int elem(const u32x4& v, int e) { return (int)((v[e >> 2] >> (8 * (e & 3))) & 255u); }
  static __device__ __forceinline__ u32x4 load_any(const uint8_t* p) { return reinterpret_cast<const SegConfBytes16*>(p)->v; }
};
template <> struct SegConfVec<uint16_t> {
  static constexpr int N = 8;
  static constexpr uint32_t REP = 0x00010001u;
  static __device__ __forceinline__ int elem(const u32x4& v, int e) { return (int)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu); }
  static __device__ __forceinline__ u32x4 load_any(const uint16_t* p) { return reinterpret_cast<const SegConfShorts8*>(p)->v; }
};

// The workgroup's counters.  DENSE: cnt[cell].  Sparse: keys[SEG_CONF_SLOTS] | counts[SEG_CONF_SLOTS]; a key goes from EMPTY to
// its cell once and never changes again, so a relaxed read that finds the cell may add without the compare-and-swap.
template <bool DENSE>
__device__ __forceinline__ void seg_conf_count(uint32_t* s, unsigned long long* conf, uint32_t cell, uint32_t n) {
  if (DENSE) {
    atomicAdd(&s[cell], n);
    return;
  }
  uint32_t slot = (cell * 2654435761u) >> (32 - SEG_CONF_SLOT_BITS);
  for (int i = 0; i < SEG_CONF_PROBES; ++i, slot = (slot + 1) & (SEG_CONF_SLOTS - 1)) {
    uint32_t k = __hip_atomic_load(&s[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == SEG_CONF_EMPTY) k = atomicCAS(&s[slot], SEG_CONF_EMPTY, cell);
    if (k == SEG_CONF_EMPTY || k == cell) {
      atomicAdd(&s[SEG_CONF_SLOTS + slot], n);
      return;
    }
  }
  atomicAdd(&conf[cell], (unsigned long long)n);
}

// Equal (prediction, ground truth) pairs that a lane meets one after the other are counted once: add() per pixel or per
// constant vector, flush() after the last.  The rule of seg_area_add, then both sides clamped to the bin C.
template <bool DENSE>
struct SegConfRun {
  uint32_t* s;
  unsigned long long* conf;
  int C, ignore_index, reduce_zero;
  int p = -1, g = -1, n = 0;
  __device__ __forceinline__ void flush() {
    if (!n || g == ignore_index) return;
    int gg = g;
    if (reduce_zero) {
      if (gg == 0) return;
      gg -= 1;
    }
    const int row = gg < C ? gg : C, col = p < C ? p : C;
    seg_conf_count<DENSE>(s, conf, (uint32_t)(row * (C + 1) + col), (uint32_t)n);
  }
  __device__ __forceinline__ void add(int lab, int gt, int k) {
    if (lab == p && gt == g) { n += k; return; }
    flush();
    p = lab; g = gt; n = k;
  }
  template <typename T>
  __device__ __forceinline__ void add_vec(const u32x4& a, const u32x4& b) {
    typedef SegConfVec<T> V;
    const int p0 = V::elem(a, 0), g0 = V::elem(b, 0);
    const uint32_t pa = (uint32_t)p0 * V::REP, gb = (uint32_t)g0 * V::REP;
    if (a[0] == pa && a[1] == pa && a[2] == pa && a[3] == pa && b[0] == gb && b[1] == gb && b[2] == gb && b[3] == gb) {
      add(p0, g0, V::N);
      return;
    }
#pragma unroll
    for (int e = 0; e < V::N; ++e) add(V::elem(a, e), V::elem(b, e), 1);
  }
};

// n <= SEG_CONF_LAUNCH_PIXELS.  Dynamic LDS: DENSE (C + 1)^2 counters rounded up to 16 bytes, else the 32 KiB table.
// gfx950: <uint8, dense> 37 VGPRs, <uint8, sparse> 39, <uint16, dense> 35, <uint16, sparse> 38; scratch 0 and 8 waves per SIMD
// by registers in all four; LDS all dynamic (0 static).  Measured: profiles/seg_confusion.txt.
template <typename T, bool DENSE>
__global__ __launch_bounds__(SEG_CONF_THREADS) void seg_confusion_kernel(const T* __restrict__ pred, const T* __restrict__ gt, int64_t n,
                                                                         int C, int ignore_index, int reduce_zero,
                                                                         unsigned long long* conf) {
  typedef SegConfVec<T> V;
  extern __shared__ u32x4 s_conf4[];
  uint32_t* const s = reinterpret_cast<uint32_t*>(s_conf4);
  const int tid = threadIdx.x;
  const int cells = DENSE ? (C + 1) * (C + 1) : 2 * SEG_CONF_SLOTS;
  const int quads = (cells + 3) >> 2;
  for (int i = tid; i < quads; i += SEG_CONF_THREADS) {
    const uint32_t fill = (!DENSE && i < SEG_CONF_SLOTS / 4) ? SEG_CONF_EMPTY : 0u;
    s_conf4[i] = u32x4{fill, fill, fill, fill};
  }
  __syncthreads();

  SegConfRun<DENSE> run = {s, conf, C, ignore_index, reduce_zero};
  // the body: whole 16-byte vectors from the first aligned address of pred on
  int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(pred) & 15)) & 15) / (int64_t)sizeof(T);
  if (head > n) head = n;
  const int64_t nvec = (n - head) / V::N;
  const T* const pb = pred + head;
  const T* const gb = gt + head;
  const bool gt_aligned = (reinterpret_cast<uintptr_t>(gb) & 15) == 0;  // kernel-uniform
  const int64_t stride = (int64_t)gridDim.x * SEG_CONF_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * SEG_CONF_THREADS + tid; v < nvec; v += 2 * stride) {
    const int64_t w = v + stride;
    const bool two = w < nvec;
    const int64_t w1 = two ? w : v;
    const u32x4 a0 = *reinterpret_cast<const u32x4*>(pb + v * V::N);
    const u32x4 a1 = *reinterpret_cast<const u32x4*>(pb + w1 * V::N);
    u32x4 b0, b1;
    if (gt_aligned) {
      b0 = *reinterpret_cast<const u32x4*>(gb + v * V::N);
      b1 = *reinterpret_cast<const u32x4*>(gb + w1 * V::N);
    } else {
      b0 = V::load_any(gb + v * V::N);
      b1 = V::load_any(gb + w1 * V::N);
    }
    run.template add_vec<T>(a0, b0);
    if (two) run.template add_vec<T>(a1, b1);
  }
  // the elements before the body and after its last vector: fewer than 2 * V::N <= 32, one lane each
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + nvec * V::N;
    int64_t i = -1;
    if (tid < head) i = tid;
    else if (tail0 + (tid - head) < n) i = tail0 + (tid - head);
    if (i >= 0) run.add((int)pred[i], (int)gt[i], 1);
  }
  run.flush();
  __syncthreads();

  if (DENSE) {
    for (int i = tid; i < cells; i += SEG_CONF_THREADS)
      if (s[i]) atomicAdd(&conf[i], (unsigned long long)s[i]);
  } else {
    for (int i = tid; i < SEG_CONF_SLOTS; i += SEG_CONF_THREADS)
      if (s[i] != SEG_CONF_EMPTY && s[SEG_CONF_SLOTS + i]) atomicAdd(&conf[s[i]], (unsigned long long)s[SEG_CONF_SLOTS + i]);
  }
}
