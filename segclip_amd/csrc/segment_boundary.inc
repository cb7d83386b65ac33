// Boundary bands of label maps and the areas of Boundary IoU and trimap mIoU (segment.hip), for maps of mixed sizes in one call.
// The reference has no such op: the definition is this project's (include/segclip_hip.h, segclip_seg_boundary) and
// tests/boundary_reference.py restates it with the brute-force window.
//   seg_bd_rows_kernel : a wave owns whole rows: S[y, x] = the number of x' in 1..x with M[y, x'] != M[y, x' - 1], 64 columns at
//                        a time (a ballot of "differs from the left neighbour", a carry from chunk to chunk), as uint16: the
//                        row part [xl, xr] of a row is constant exactly when S[y, xl] == S[y, xr]
//   seg_bd_band_kernel : a wave owns a strip of SEG_BD_SH rows x 64 columns, a lane one column.  The (2d+1)^2 window of (y, x)
//                        is constant exactly when no row y' of [y - d, y + d] (clipped) has a row part [x - d, x + d] (clipped)
//                        that is not constant, and no y' of (y - d, y + d] has M[y', x] != M[y' - 1, x]: the lane walks down its
//                        column once, d rows ahead of the pixel it emits, and remembers the last row of either kind.  Prediction
//                        and ground truth walk together; the areas are counted in LDS ((2, 3, C) per workgroup, equal
//                        consecutive pixels of a lane counted once) and added with one global atomic per touched counter.
// Work per pixel: the rows pass O(1), the band pass (SEG_BD_SH + 2 d) / SEG_BD_SH row visits of one byte and two uint16, all
// coalesced across the lanes.  Integer sums: the result depends on no schedule.
// The kernels are templates on the label element L of pred AND gt: uint8_t, or uint16_t for 16-bit label maps (an int16 tensor
// read as unsigned).  The bands stay one byte per pixel.  What follows L: the run key (32 bits hold two bytes and the flags, two
// 16-bit values need 64), the class limit and with it the counters in LDS (6 x 256 ints, or 6 x 1024 = 24 KB for uint16_t only).

#define SEG_BD_COLS SEGCLIP_SEG_BOUNDARY_COLS            // int64 columns of one image row of the table (segclip_hip.h)
#define SEG_BD_SH SEGCLIP_SEG_BOUNDARY_TILE_H             // rows of a wave's strip
#define SEG_BD_TW SEGCLIP_SEG_BOUNDARY_TILE_W             // its columns: the wave
#define SEG_BD_WAVES SEGCLIP_SEG_BOUNDARY_WAVES           // strips of a workgroup, consecutive in the image's raster order of strips
#define SEG_BD_LIMIT SEGCLIP_SEG_SOURCE_LIMIT
#define SEG_BD_MAX_RADIUS SEGCLIP_SEG_BOUNDARY_MAX_RADIUS
enum { BD_H, BD_W, BD_PRED, BD_GT, BD_RADIUS, BD_BLK };
static_assert(SEG_BD_TW == SEGCLIP_WAVE && SEG_BD_LIMIT <= 65536, "seg_bd: a row's change count fits uint16");

struct SegBdArgs {
  const int64_t* images;       // (B, SEG_BD_COLS)
  const void* pred;            // flat, elements of L
  const void* gt;              // flat, or null
  int64_t pred_n, gt_n, n_blocks;   // elements of pred and of gt
  int B, max_side, C, ignore_index, reduce_zero;
  uint8_t* pred_band;          // at pred's offsets, or null
  uint8_t* gt_band;            // at gt's offsets, or null
  unsigned long long* areas;   // (2, 3, C), or null
  uint16_t* pred_s;            // workspace: S at pred's offsets
  uint16_t* gt_s;              // S at gt's offsets
};

// One image's share of a workgroup, range-checked: the host entry cannot inspect device memory.
struct SegBdImage { int h, w, d, strips_x, strips, blocks, t; int64_t poff, goff; bool ok, has_gt; };
__device__ __forceinline__ SegBdImage seg_bd_image(const SegBdArgs& A, int img) {
  const int64_t* D = A.images + (int64_t)img * SEG_BD_COLS;
  const int64_t h = D[BD_H], w = D[BD_W], d = D[BD_RADIUS], blk = D[BD_BLK];
  SegBdImage I;
  I.poff = D[BD_PRED]; I.goff = D[BD_GT];
  I.ok = h >= 1 && w >= 1 && h <= A.max_side && w <= A.max_side && h < SEG_BD_LIMIT && w < SEG_BD_LIMIT && d >= 1 &&
         d <= SEG_BD_MAX_RADIUS;
  I.h = I.ok ? (int)h : 1; I.w = I.ok ? (int)w : 1; I.d = I.ok ? (int)d : 1;
  const int64_t px = (int64_t)I.h * I.w;
  I.strips_x = (I.w + SEG_BD_TW - 1) / SEG_BD_TW;
  I.strips = I.strips_x * ((I.h + SEG_BD_SH - 1) / SEG_BD_SH);
  I.blocks = (I.strips + SEG_BD_WAVES - 1) / SEG_BD_WAVES;
  I.ok = I.ok && I.poff >= 0 && I.poff <= A.pred_n - px && blk >= 0 && blk <= A.n_blocks - I.blocks;
  // without a ground truth to read the column is not looked at; -1 = this map has none
  I.has_gt = A.gt && (A.gt_band || A.areas) && I.goff != -1;
  if (I.has_gt && !(I.goff >= 0 && I.goff <= A.gt_n - px)) I.ok = false;
  const int64_t t = (int64_t)blockIdx.x - blk;
  if (t < 0 || t >= I.blocks) I.ok = false;
  I.t = I.ok ? (int)t : 0;
  return I;
}

#define SEG_BD_PROLOGUE(A)                                                                                  \
  __shared__ int s_img;                                                                                     \
  const int tid = threadIdx.x;                                                                              \
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_BD_COLS, BD_BLK, (int64_t)blockIdx.x);           \
  __syncthreads();                                                                                          \
  const SegBdImage I = seg_bd_image(A, s_img);                                                              \
  if (!I.ok) return; /* block-uniform */                                                                    \
  const int lane = tid & 63, wv = tid >> 6;

// ---------------------------------------------------------------- label changes along a row, counted from its left end
template <class L>
__device__ __forceinline__ void seg_bd_scan_row(const L* __restrict__ m, uint16_t* __restrict__ s, int w, int lane) {
  int carry = 0, last = 0;
  for (int x0 = 0; x0 < w; x0 += SEG_BD_TW) {  // wave-uniform
    const int x = x0 + lane;
    const bool in = x < w;
    const int b = in ? m[x] : 0;
    int before = __shfl_up(b, 1, 64);
    if (lane == 0) before = last;
    const unsigned long long changes = __ballot(in && x > 0 && b != before);
    if (in) s[x] = (uint16_t)(carry + __popcll(changes & (~0ull >> (63 - lane))));
    carry += __popcll(changes);
    last = __shfl(b, 63, 64);
  }
}

// The image's SEG_BD_WAVES * blocks waves share its rows round robin.
template <class L>
__global__ __launch_bounds__(256) void seg_bd_rows_kernel(SegBdArgs A) {
  SEG_BD_PROLOGUE(A)
  const L* pred = static_cast<const L*>(A.pred);
  const L* gt = static_cast<const L*>(A.gt);
  const int waves = SEG_BD_WAVES * I.blocks;
  for (int y = SEG_BD_WAVES * I.t + wv; y < I.h; y += waves) {
    const int64_t row = (int64_t)y * I.w;
    seg_bd_scan_row(pred + I.poff + row, A.pred_s + I.poff + row, I.w, lane);
    if (I.has_gt) seg_bd_scan_row(gt + I.goff + row, A.gt_s + I.goff + row, I.w, lane);
  }
}

// ---------------------------------------------------------------- bands and areas
// What a lane remembers of its column above the row it has read last: the last row whose row part is not constant, the last
// row whose label differs from the row above it, and the label of the last row.
struct SegBdColumn { int bad, change, byte; };
template <class L>
__device__ __forceinline__ void seg_bd_visit(const L* __restrict__ m, const uint16_t* __restrict__ s, int64_t row, int y,
                                             int x, int xl, int xr, bool first, SegBdColumn& c) {
  const int b = m[row + x];
  if (s[row + xl] != s[row + xr]) c.bad = y;
  if (!first && b != c.byte) c.change = y;
  c.byte = b;
}

// key: q | g << BITS | (bp != 0) << 2 BITS | (bg != 0) << (2 BITS + 1) | (bg & 1) << (2 BITS + 2), for n pixels.  The
// ground-truth rule is seg_area_add's.
template <class L>
__device__ __forceinline__ void seg_bd_count(int* cnt, int C, typename SegLabel<L>::key_t key, int n, int ignore_index,
                                             int reduce_zero) {
  typedef typename SegLabel<L>::key_t key_t;
  constexpr int BITS = SegLabel<L>::BITS;
  constexpr key_t ONE = 1;
  const int q = (int)(key & ((ONE << BITS) - 1));
  int g = (int)((key >> BITS) & ((ONE << BITS) - 1));
  if (g == ignore_index) return;
  if (reduce_zero) {
    if (g == 0) return;
    g -= 1;
  }
  const bool in_p = key & (ONE << (2 * BITS)), in_g = key & (ONE << (2 * BITS + 1));
  if (q < C && in_p) atomicAdd(&cnt[C + q], n);
  if (g < C && in_g) {
    atomicAdd(&cnt[2 * C + g], n);
    if (q == g && in_p) atomicAdd(&cnt[q], n);
  }
  if (key & (ONE << (2 * BITS + 2))) {
    int* tri = cnt + 3 * C;
    if (q < C) atomicAdd(&tri[C + q], n);
    if (g < C) {
      atomicAdd(&tri[2 * C + g], n);
      if (q == g) atomicAdd(&tri[q], n);
    }
  }
}

template <class L>
__global__ __launch_bounds__(256) void seg_bd_band_kernel(SegBdArgs A) {
  typedef typename SegLabel<L>::key_t key_t;
  constexpr int BITS = SegLabel<L>::BITS;
  __shared__ int s_cnt[6 * SegLabel<L>::MAX_CLASSES];
  SEG_BD_PROLOGUE(A)
  const int C = A.C;
  const bool count = A.areas && I.has_gt;  // block-uniform
  if (count) {
    for (int i = tid; i < 6 * C; i += 256) s_cnt[i] = 0;
    __syncthreads();
  }
  const int strip = SEG_BD_WAVES * I.t + wv;
  if (strip < I.strips) {  // wave-uniform
    const int h = I.h, w = I.w, d = I.d;
    const int sy = strip / I.strips_x, ya = sy * SEG_BD_SH, yb = min(h, ya + SEG_BD_SH);
    const int xs = (strip - sy * I.strips_x) * SEG_BD_TW + lane;
    const bool in = xs < w;
    const int x = in ? xs : w - 1;  // a lane past the row reads its last column and writes nothing
    const int xl = max(0, x - d), xr = min(w - 1, x + d);
    const bool frame_x = x < d || x >= w - d;
    const L* pm = static_cast<const L*>(A.pred) + I.poff;
    const uint16_t* ps = A.pred_s + I.poff;
    const L* gm = I.has_gt ? static_cast<const L*>(A.gt) + I.goff : pm;
    const uint16_t* gs = I.has_gt ? A.gt_s + I.goff : ps;
    SegBdColumn P = {-1, -1, 0}, G = {-1, -1, 0};
    const int top = max(0, ya - d);  // the first row any window of this strip reaches: its own change lies outside all of them
    int seen = top - 1;
    key_t run_key = -1;
    int run_n = 0;
    for (int y = ya; y < yb; ++y) {
      const int ylo = max(0, y - d), yhi = min(h - 1, y + d);
      while (seen < yhi) {  // wave-uniform; 2 d + 1 rows at most before the strip's first pixel, then one per pixel
        ++seen;
        const int64_t row = (int64_t)seen * w;
        seg_bd_visit(pm, ps, row, seen, x, xl, xr, seen == top, P);
        if (I.has_gt) seg_bd_visit(gm, gs, row, seen, x, xl, xr, seen == top, G);
      }
      const int frame = (frame_x || y < d || y >= h - d) ? 2 : 0;
      const int64_t at = (int64_t)y * w + x;
      const int bp = ((P.bad >= ylo || P.change > ylo) ? 1 : 0) | frame;
      if (in && A.pred_band) A.pred_band[I.poff + at] = (uint8_t)bp;
      if (!I.has_gt) continue;
      const int bg = ((G.bad >= ylo || G.change > ylo) ? 1 : 0) | frame;
      if (in && A.gt_band) A.gt_band[I.goff + at] = (uint8_t)bg;
      if (!count || !in) continue;
      const key_t key = (key_t)pm[at] | (key_t)gm[at] << BITS | (key_t)(bp != 0) << (2 * BITS) | (key_t)(bg != 0) << (2 * BITS + 1) |
                        (key_t)(bg & 1) << (2 * BITS + 2);
      if (key == run_key) {
        ++run_n;
      } else {
        if (run_n) seg_bd_count<L>(s_cnt, C, run_key, run_n, A.ignore_index, A.reduce_zero);
        run_key = key; run_n = 1;
      }
    }
    if (run_n) seg_bd_count<L>(s_cnt, C, run_key, run_n, A.ignore_index, A.reduce_zero);
  }
  if (count) {
    __syncthreads();
    for (int i = tid; i < 6 * C; i += 256)
      if (s_cnt[i]) atomicAdd(&A.areas[i], (unsigned long long)s_cnt[i]);
  }
}
