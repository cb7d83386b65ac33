// Per-image areas of label maps (segment.hip): segclip_seg_image_areas and segclip_seg_image_areas_wide add, for every picture of
// a list, the (3, C) areas of segclip_seg_areas of that picture alone to its row of a (B, 3, C) int64 tensor, in one launch.  The
// counting is seg_area_add's through SegAreaRun (segment_tile.inc), so a row equals that entry's result by construction.
//
// Design (the kernel reads 2 or 4 bytes per pixel and is meant to sit on HBM reads):
//   - table: one (B, SEG_IA_COLS) int64 row per picture: offset in pred, offset in gt, pixels, first workgroup.  pred and gt have
//     offsets of their own: a label buffer has gaps between its maps, ground truths lie gapless.
//   - workgroups: 256 threads, one tile of SEG_IA_TILE consecutive pixels of ONE picture; lane 0 finds the picture by the binary
//     search of the other table kernels (seg_block_image) and checks the row (seg_ia_row); a search that a bad first-workgroup
//     column misled is repeated as a look through all rows by the whole workgroup, which only a bad table ever pays for.
//   - loads: 16 bytes of each map per lane and step with element alignment only (SegConfVec<T>::load_any of
//     segment_confusion.inc: a picture starts at any element, pred and gt independently), two steps in flight; the elements
//     after a tile's last whole vector, fewer than 16, and pictures shorter than a vector are read one by one.
//   - counting: equal consecutive (g, p) pairs of a lane are counted once, a constant vector is one comparison; 3 x C int32
//     counters per workgroup in static LDS (3 KiB for the uint8 kernel, 12 KiB for the uint16 one), one 64-bit integer global
//     atomicAdd per non-zero counter into the picture's row (seg_area_flush): the sums depend on no schedule, and a tile holds
//     far fewer than 2^31 pixels, so no counter and no run length overflows.
//   - tile: 8192 pixels, by measurement.  The design began at 32768, so that zeroing and scanning 3 x 848 counters (10 per lane
//     each way) stay small beside a lane's 8-16 steps of counting.  Measured on 64 VOC-sized piecewise-constant maps, 12.0 M
//     pixels, device events around 50 back-to-back launches, 7 repeats, builds alternating (uint8 at 21 classes / uint16 at
//     848): tile 8192 11.7 / 14.5 us, 16384 14.5 / 17.7 us, 32768 23.3 / 26.5 us, 65536 41.4 / 47.2 us; against per-pixel noise
//     20.3 / 24.1, 25.8 / 30.7, 26.4 / 31.7 and 45.7 / 51.7 us.  With large tiles a CU holds one or two workgroups whose lanes
//     walk a chain of dependent steps; at 8192 a lane has its one or two steps in flight at once and 1496 workgroups are
//     resident together.  The counters' fixed passes cost 0.9 us of the 14.5 at 848 classes.  Tiles below 8192: unmeasured.
// Plain C++, no inline assembly.  gfx950 (hipcc -Rpass-analysis=kernel-resource-usage): at the kernel below.

#define SEG_IA_COLS SEGCLIP_SEG_IA_COLS
#define SEG_IA_TILE SEGCLIP_SEG_IA_TILE
#define SEG_IA_THREADS 256          // seg_area_flush strides by it
#define SEG_IA_NONE 0x7fffffff      // no picture
enum { IA_PRED, IA_GT, IA_COUNT, IA_BLK };
static_assert(SEG_IA_TILE % (SEG_IA_THREADS * 16) == 0 && SEG_IA_TILE < (1 << 30), "seg_image_areas tile: whole steps of 16 bytes per lane");

// Kernel arguments; pred and gt are elements of the kernel's T.
struct SegIAArgs {
  const void* pred;
  const void* gt;
  const int64_t* images;       // (B, SEG_IA_COLS)
  int64_t pred_n, gt_n, n_blocks;
  int B, C, ignore_index, reduce_zero;
  unsigned long long* out;     // (B, 3, C)
};

// the workgroups of a picture of n pixels; 0 for a count the kernel refuses
__device__ __forceinline__ int64_t seg_ia_tiles(int64_t n) {
  return n >= 1 && n < (1ll << 31) ? (n + SEG_IA_TILE - 1) / SEG_IA_TILE : 0;
}

// Row `img`, range-checked (the host entry cannot inspect device memory), as workgroup `block` sees it: ok where the row passes
// AND holds the workgroup, which is then tile t of its n pixels.
struct SegIARow { int64_t po, go; int n, t; bool ok; };
__device__ __forceinline__ SegIARow seg_ia_row(const SegIAArgs& A, int img, int64_t block) {
  const int64_t* D = A.images + (int64_t)img * SEG_IA_COLS;
  const int64_t n = D[IA_COUNT], blk = D[IA_BLK], tiles = seg_ia_tiles(n);
  SegIARow R;
  R.po = D[IA_PRED]; R.go = D[IA_GT];
  R.ok = tiles >= 1 && R.po >= 0 && R.po <= A.pred_n - n && R.go >= 0 && R.go <= A.gt_n - n && blk >= 0 && blk <= A.n_blocks - tiles;
  // its workgroups do not begin before those of the row before it end
  if (R.ok && img > 0) R.ok = blk - seg_ia_tiles(D[IA_COUNT - SEG_IA_COLS]) >= D[IA_BLK - SEG_IA_COLS];
  const int64_t t = block - blk;
  R.ok = R.ok && t >= 0 && t < tiles;
  R.n = R.ok ? (int)n : 0;
  R.t = R.ok ? (int)t : 0;
  return R;
}

// SegAreaRun with runs that grow by more than one pixel: a constant 16-byte vector of both maps is one add.
struct SegIARun : SegAreaRun {
  __device__ __forceinline__ void add_n(int lab, int gt, int k) {
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
      add_n(p0, g0, V::N);
      return;
    }
#pragma unroll
    for (int e = 0; e < V::N; ++e) add_n(V::elem(a, e), V::elem(b, e), 1);
  }
};

// gfx950: <uint8_t> 37 VGPRs, 47 SGPRs, 3080 bytes of LDS; <uint16_t> 36 VGPRs, 46 SGPRs, 12296 bytes of LDS; scratch 0, no
// spills and 8 waves per SIMD in both.
// Measured: profiles/seg_per_image.txt.
template <typename T>
__global__ __launch_bounds__(SEG_IA_THREADS) void seg_image_areas_kernel(SegIAArgs A) {
  typedef SegConfVec<T> V;
  __shared__ int s_cnt[3 * SegLabel<T>::MAX_CLASSES];
  __shared__ int s_img, s_alt;
  const int tid = threadIdx.x, C = A.C;
  const int64_t block = blockIdx.x;
  if (tid == 0) {
    const int i = seg_block_image(A.images, A.B, SEG_IA_COLS, IA_BLK, block);
    s_img = seg_ia_row(A, i, block).ok ? i : SEG_IA_NONE;
    s_alt = SEG_IA_NONE;
  }
  for (int i = tid; i < 3 * C; i += SEG_IA_THREADS) s_cnt[i] = 0;
  __syncthreads();
  int img = s_img;
  if (img == SEG_IA_NONE) {  // block-uniform; a bad table only: the first passing row that holds this workgroup, if any
    for (int j = tid; j < A.B; j += SEG_IA_THREADS)
      if (seg_ia_row(A, j, block).ok) atomicMin(&s_alt, j);
    __syncthreads();
    img = s_alt;
    if (img == SEG_IA_NONE) return;
  }
  const SegIARow R = seg_ia_row(A, img, block);

  const int64_t first = (int64_t)R.t * SEG_IA_TILE;
  const int m = R.n - first < SEG_IA_TILE ? (int)(R.n - first) : SEG_IA_TILE;  // this tile's pixels, >= 1
  const T* const p = static_cast<const T*>(A.pred) + R.po + first;
  const T* const g = static_cast<const T*>(A.gt) + R.go + first;
  SegIARun run = {{s_cnt, C, A.ignore_index, A.reduce_zero}};
  const int nvec = m / V::N;
  for (int v = tid; v < nvec; v += 2 * SEG_IA_THREADS) {
    const int w = v + SEG_IA_THREADS;
    const bool two = w < nvec;
    const int w1 = two ? w : v;
    const u32x4 a0 = V::load_any(p + v * V::N), a1 = V::load_any(p + w1 * V::N);
    const u32x4 b0 = V::load_any(g + v * V::N), b1 = V::load_any(g + w1 * V::N);
    run.template add_vec<T>(a0, b0);
    if (two) run.template add_vec<T>(a1, b1);
  }
  // the elements after the last whole vector: fewer than V::N <= 16, one lane each
  const int i = nvec * V::N + tid;
  if (i < m) run.add_n((int)p[i], (int)g[i], 1);
  run.flush();
  __syncthreads();
  seg_area_flush(s_cnt, C, A.out + (int64_t)img * 3 * C, tid);
}
