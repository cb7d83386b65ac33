// Superpixels of decoded pictures (segment.hip): an integer SLIC on the RGB bytes, for pictures of mixed sizes in one call.
// The reference has no such op: the definition is this project's (include/segclip_hip.h, segclip_seg_superpixels) and
// tests/superpixel_reference.py restates it in numpy.  Everything is integer arithmetic and every sum is an integer sum, so
// the order in which the atomics arrive cannot change a result: two calls give the same bits.
//   seg_sp_init_kernel   : the centres at the middle of their cells with the picture's bytes there; their accumulators cleared
//   seg_sp_assign_kernel : <false> a round's assignment: every pixel's nearest of the (up to) 9 candidate centres, and the sums
//                          (n, sum y, sum x, sum r, sum g, sum b) of every centre's members; <true> the final assignment, which
//                          writes the ids and sums nothing
//   seg_sp_update_kernel : a centre with members becomes the floor-divided means; its accumulators are cleared for the next round
// A workgroup owns a SEG_SP_TH x SEG_SP_TW tile of one image, all images in one grid (the table names an image's first
// workgroup).  The cell whose first pixel lies in a tile belongs to that tile: its workgroup initialises and updates the cell's
// centre, one lane per cell, so these two kernels need no table of their own.
// The assignment stages the centres of the cells its tile touches plus one ring in LDS (at most SEG_SP_STAGE_H x
// SEG_SP_STAGE_W of them, at step 4; 11 words per centre: 7.9 KiB static).  A lane owns one column of 8 rows and walks down it,
// so a wave's load of a row is one run of 192 bytes; members it meets one after the other for the same centre are summed in
// registers and added with one set of 6 LDS atomics per run.  The rows of the LDS image that are not zero then go out with one
// set of 6 global integer atomics per (tile, centre): a partial reduction per workgroup, then one atomic per workgroup.
// Traffic per round: 3 B per pixel read, 20 B per staged centre read, 24 B of atomics per (tile, centre with members); the
// final assignment adds 4 B per pixel of ids.
// Measured on 64 pictures, 12.0 M pixels, step 16 (profiles/seg_snap.txt): assign-and-sum 105.5 us (0.34 TB/s of the design
// traffic), the final assignment 87.7 us (0.96 TB/s), init and update 16 us each: bound by the 9 candidate distances per pixel
// and their LDS reads, NOT by memory.
// Plain C++, no inline assembly.  gfx950 (hipcc -Rpass-analysis=kernel-resource-usage): at the kernels below.

#define SEG_SP_COLS SEGCLIP_SEG_SP_COLS     // int64 columns of one image row of the table (segclip_hip.h)
#define SEG_SP_TH SEGCLIP_SEG_SP_TILE_H
#define SEG_SP_TW SEGCLIP_SEG_SP_TILE_W     // the wave: a tile row is one wave's lanes
#define SEG_SP_MIN_STEP SEGCLIP_SEG_SP_MIN_STEP
#define SEG_SP_MAX_STEP SEGCLIP_SEG_SP_MAX_STEP
#define SEG_SP_MAX_COMPACT SEGCLIP_SEG_SP_MAX_COMPACTNESS
#define SEG_SP_MAX_T SEGCLIP_SEG_SP_MAX_ITERS
#define SEG_SP_LIMIT SEGCLIP_SEG_SOURCE_LIMIT
#define SEG_SP_THREADS 256
#define SEG_SP_ROWS (SEG_SP_TH * SEG_SP_TW / SEG_SP_THREADS)   // rows of one lane's column
// cells that n pixels starting at a multiple of n touch, at most: n / step when step divides n, else (n - 1) / step + 2
#define SEG_SP_STAGE_H (SEG_SP_TH / SEG_SP_MIN_STEP + 2)
#define SEG_SP_STAGE_W (SEG_SP_TW / SEG_SP_MIN_STEP + 2)
#define SEG_SP_STAGE (SEG_SP_STAGE_H * SEG_SP_STAGE_W)
enum { SP_SRC, SP_H, SP_W, SP_STRIDE, SP_IDS, SP_CEN, SP_BLK };
static_assert(SEG_SP_TW == SEGCLIP_WAVE && SEG_SP_TH * SEG_SP_TW % SEG_SP_THREADS == 0 && SEG_SP_THREADS % SEG_SP_TW == 0, "seg_sp tile");
static_assert((SEG_SP_TH / SEG_SP_MIN_STEP) * (SEG_SP_TW / SEG_SP_MIN_STEP) <= SEG_SP_THREADS, "one lane per cell of a tile");
static_assert((SEG_SP_TH - 1) / (SEG_SP_MIN_STEP + 1) + 2 <= SEG_SP_TH / SEG_SP_MIN_STEP &&
              (SEG_SP_TW - 1) / (SEG_SP_MIN_STEP + 1) + 2 <= SEG_SP_TW / SEG_SP_MIN_STEP, "the smallest step stages the most centres");
static_assert(SEG_SP_STAGE * 11 * 4 <= 64 * 1024, "the staged centres fit the static LDS");
// D = S^2 dc^2 + m^2 ds^2 < 2^31: dc^2 <= 3 * 255^2, and a candidate centre lies within its own 3 x 3 cells, which lie within
// the 5 x 5 around the pixel's home cell: |dy|, |dx| < 3 S, ds^2 < 18 S^2
static_assert((long long)SEG_SP_MAX_STEP * SEG_SP_MAX_STEP * 195075 +
              (long long)SEG_SP_MAX_COMPACT * SEG_SP_MAX_COMPACT * 18 * SEG_SP_MAX_STEP * SEG_SP_MAX_STEP < (1ll << 31), "seg_sp distance");
// a centre's members come from its 3 x 3 cells: at most 9 S^2 of them, each coordinate below 2^15
static_assert(9ll * SEG_SP_MAX_STEP * SEG_SP_MAX_STEP * (SEG_SP_LIMIT - 1) < (1ll << 32), "seg_sp sums");

struct SegSpArgs {
  const int64_t* images;   // (B, SEG_SP_COLS)
  int32_t* ids;            // flat segment ids
  int32_t* centres;        // (K_total, 5): y, x, r, g, b
  uint32_t* acc;           // (K_total, 6): n, sum y, sum x, sum r, sum g, sum b
  int64_t ids_n, K_total, n_blocks;
  int B, max_side, S, m2;  // m2 = compactness^2
};

// One tile of one image, range-checked: the host entry cannot inspect device memory.
struct SegSpTile {
  const uint8_t* src;
  int h, w, gh, gw, y0, x0, th, tw;
  int64_t stride, ids, cen;
  bool ok;
};
__device__ __forceinline__ SegSpTile seg_sp_tile(const SegSpArgs& A, int img) {
  const int64_t* D = A.images + (int64_t)img * SEG_SP_COLS;
  const int64_t h = D[SP_H], w = D[SP_W], blk = D[SP_BLK];
  SegSpTile T;
  T.src = reinterpret_cast<const uint8_t*>(D[SP_SRC]);
  T.stride = D[SP_STRIDE]; T.ids = D[SP_IDS]; T.cen = D[SP_CEN];
  T.ok = T.src != nullptr && h >= 1 && w >= 1 && h <= A.max_side && w <= A.max_side && h < SEG_SP_LIMIT && w < SEG_SP_LIMIT &&
         T.stride >= 3 * w && T.stride < (1ll << 31);
  T.h = T.ok ? (int)h : 1; T.w = T.ok ? (int)w : 1;
  T.gh = (T.h + A.S - 1) / A.S; T.gw = (T.w + A.S - 1) / A.S;
  const int tiles_x = (T.w + SEG_SP_TW - 1) / SEG_SP_TW;
  const int tiles = tiles_x * ((T.h + SEG_SP_TH - 1) / SEG_SP_TH);
  T.ok = T.ok && T.ids >= 0 && T.ids <= A.ids_n - (int64_t)T.h * T.w && T.cen >= 0 && T.cen <= A.K_total - (int64_t)T.gh * T.gw &&
         blk >= 0 && blk <= A.n_blocks - tiles;
  const int64_t t = (int64_t)blockIdx.x - blk;
  if (t < 0 || t >= tiles) T.ok = false;
  const int ty = T.ok ? (int)t / tiles_x : 0, tx = T.ok ? (int)t - ty * tiles_x : 0;
  T.y0 = ty * SEG_SP_TH; T.x0 = tx * SEG_SP_TW;
  T.th = min(SEG_SP_TH, T.h - T.y0); T.tw = min(SEG_SP_TW, T.w - T.x0);
  return T;
}

// The cells whose first pixel lies in the tile: rows ci0 .. ci0 + ni - 1, columns cj0 .. cj0 + nj - 1; lane t owns one of them.
// -> the cell's centre index in the image, or -1 for a lane without a cell
__device__ __forceinline__ int seg_sp_own_cell(const SegSpTile& T, int S, int tid, int& ci, int& cj) {
  const int ci0 = (T.y0 + S - 1) / S, cj0 = (T.x0 + S - 1) / S;
  const int ni = (T.y0 + T.th - 1) / S - ci0 + 1, nj = (T.x0 + T.tw - 1) / S - cj0 + 1;   // >= 0
  if (ni <= 0 || nj <= 0 || tid >= ni * nj) return -1;
  ci = ci0 + tid / nj; cj = cj0 + tid % nj;
  return ci * T.gw + cj;
}

// gfx950: 12 VGPRs, scratch 0, LDS 4 bytes
__global__ __launch_bounds__(SEG_SP_THREADS) void seg_sp_init_kernel(SegSpArgs A) {
  __shared__ int s_img;
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_SP_COLS, SP_BLK, (int64_t)blockIdx.x);
  __syncthreads();
  const SegSpTile T = seg_sp_tile(A, s_img);
  if (!T.ok) return;  // block-uniform
  int ci, cj;
  const int k = seg_sp_own_cell(T, A.S, tid, ci, cj);
  if (k < 0) return;
  const int y = min(ci * A.S + A.S / 2, T.h - 1), x = min(cj * A.S + A.S / 2, T.w - 1);
  const uint8_t* p = T.src + (int64_t)y * T.stride + 3 * x;
  int32_t* c = A.centres + (T.cen + k) * 5;
  c[0] = y; c[1] = x; c[2] = p[0]; c[3] = p[1]; c[4] = p[2];
  uint32_t* a = A.acc + (T.cen + k) * 6;
#pragma unroll
  for (int i = 0; i < 6; ++i) a[i] = 0u;
}

// gfx950: 13 VGPRs, scratch 0, LDS 4 bytes
__global__ __launch_bounds__(SEG_SP_THREADS) void seg_sp_update_kernel(SegSpArgs A) {
  __shared__ int s_img;
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_SP_COLS, SP_BLK, (int64_t)blockIdx.x);
  __syncthreads();
  const SegSpTile T = seg_sp_tile(A, s_img);
  if (!T.ok) return;  // block-uniform
  int ci, cj;
  const int k = seg_sp_own_cell(T, A.S, tid, ci, cj);
  if (k < 0) return;
  uint32_t* a = A.acc + (T.cen + k) * 6;
  const uint32_t n = a[0];
  if (n == 0) return;   // a centre without members keeps its values
  int32_t* c = A.centres + (T.cen + k) * 5;
#pragma unroll
  for (int i = 0; i < 5; ++i) c[i] = (int32_t)(a[i + 1] / n);
#pragma unroll
  for (int i = 0; i < 6; ++i) a[i] = 0u;
}

// Members that a lane meets one after the other for the same staged centre: summed in registers, one set of LDS atomics per run
struct SegSpRun {
  uint32_t* s_acc;
  int c = -1;
  uint32_t n = 0, y = 0, x = 0, r = 0, g = 0, b = 0;
  __device__ __forceinline__ void flush() {
    if (c < 0) return;
    uint32_t* a = s_acc + c * 6;
    atomicAdd(a + 0, n); atomicAdd(a + 1, y); atomicAdd(a + 2, x); atomicAdd(a + 3, r); atomicAdd(a + 4, g); atomicAdd(a + 5, b);
  }
  __device__ __forceinline__ void add(int cc, int py, int px, int pr, int pg, int pb) {
    if (cc != c) {
      flush();
      c = cc; n = y = x = r = g = b = 0;
    }
    n += 1; y += (uint32_t)py; x += (uint32_t)px; r += (uint32_t)pr; g += (uint32_t)pg; b += (uint32_t)pb;
  }
};

// gfx950: <false> 35 VGPRs and 7,924 bytes of static LDS, <true> 27 and 3,604 (no accumulators); scratch 0 and 8 waves per SIMD in both
template <bool FINAL>
__global__ __launch_bounds__(SEG_SP_THREADS) void seg_sp_assign_kernel(SegSpArgs A) {
  __shared__ int s_img;
  __shared__ int s_cen[SEG_SP_STAGE * 5];
  __shared__ uint32_t s_acc[SEG_SP_STAGE * 6];
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_SP_COLS, SP_BLK, (int64_t)blockIdx.x);
  __syncthreads();
  const SegSpTile T = seg_sp_tile(A, s_img);
  if (!T.ok) return;  // block-uniform
  const int S = A.S;
  // the staged window of cells: the cells the tile touches and one ring, clipped to the grid
  const int si0 = max(T.y0 / S - 1, 0), sj0 = max(T.x0 / S - 1, 0);
  const int si1 = min((T.y0 + T.th - 1) / S + 1, T.gh - 1), sj1 = min((T.x0 + T.tw - 1) / S + 1, T.gw - 1);
  const int sh = si1 - si0 + 1, sw = sj1 - sj0 + 1, staged = sh * sw;
  if (sh > SEG_SP_STAGE_H || sw > SEG_SP_STAGE_W) return;  // block-uniform; cannot happen for a step >= SEG_SP_MIN_STEP
  for (int i = tid; i < staged; i += SEG_SP_THREADS) {
    const int k = (si0 + i / sw) * T.gw + sj0 + i % sw;
    const int32_t* c = A.centres + (T.cen + k) * 5;
#pragma unroll
    for (int e = 0; e < 5; ++e) s_cen[i * 5 + e] = c[e];
    if (!FINAL) {
#pragma unroll
      for (int e = 0; e < 6; ++e) s_acc[i * 6 + e] = 0u;
    }
  }
  __syncthreads();

  const int lx = tid & (SEG_SP_TW - 1), ly0 = (tid / SEG_SP_TW) * SEG_SP_ROWS;
  const int x = T.x0 + lx;
  if (x < T.w) {
    const int cj = x / S;
    const int j0 = max(cj - 1, 0), j1 = min(cj + 1, T.gw - 1);
    SegSpRun run = {s_acc};
    for (int r = 0; r < SEG_SP_ROWS; ++r) {
      const int y = T.y0 + ly0 + r;
      if (y >= T.h) break;
      const uint8_t* p = T.src + (int64_t)y * T.stride + 3 * x;
      const int pr = p[0], pg = p[1], pb = p[2];
      const int ci = y / S;
      const int i0 = max(ci - 1, 0), i1 = min(ci + 1, T.gh - 1);
      // increasing centre index, strict <: among equal distances the smallest index
      int best = 0x7fffffff, bi = 0, bj = 0;
      for (int i = i0; i <= i1; ++i)
        for (int j = j0; j <= j1; ++j) {
          const int* c = s_cen + ((i - si0) * sw + (j - sj0)) * 5;
          const int dy = y - c[0], dx = x - c[1], d0 = pr - c[2], d1 = pg - c[3], d2 = pb - c[4];
          const int D = S * S * (d0 * d0 + d1 * d1 + d2 * d2) + A.m2 * (dy * dy + dx * dx);
          if (D < best) { best = D; bi = i; bj = j; }
        }
      if (FINAL) A.ids[T.ids + (int64_t)y * T.w + x] = bi * T.gw + bj;
      else run.add((bi - si0) * sw + (bj - sj0), y, x, pr, pg, pb);
    }
    if (!FINAL) run.flush();
  }
  if (FINAL) return;
  __syncthreads();
  for (int i = tid; i < staged; i += SEG_SP_THREADS) {
    if (!s_acc[i * 6]) continue;
    const int k = (si0 + i / sw) * T.gw + sj0 + i % sw;
    uint32_t* a = A.acc + (T.cen + k) * 6;
#pragma unroll
    for (int e = 0; e < 6; ++e) atomicAdd(a + e, s_acc[i * 6 + e]);
  }
}
