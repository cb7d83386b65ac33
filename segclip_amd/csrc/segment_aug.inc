// Test-time augmentation of the zero-shot evaluation (segment.hip): mmseg's aug_test for flip and multi-scale views without a
// (C, oh, ow), (C, H, W) or per-view probability array.  Every view of an image is one row of the image table of
// segment_tile.inc (its own network size, windows, window size, grid and soft_attn offset) plus a flag word; an output pixel
// mirrors its position per view, forms the view's class logits at the four source taps by the device functions of
// segment_pixel.inc (the four-tap blend of segclip_seg_label_map_rescaled), takes their soft-max, and the mean over the views
// decides the label.  segclip_seg_view_probs is the same kernel writing the mean instead of its first maximum.
//
// A lane cannot hold a vector of class probabilities (up to 256), and the mean needs every view's soft-max denominator before
// the first class can be summed.  So per pixel and view: the covering windows of the four taps (LDS, as in the rescaled
// kernel), then the maximum and the sum over all classes, then the view's probabilities added to per-lane accumulators in LDS,
// acc[class][lane].  The accumulators hold a chunk of the classes; with more classes than a chunk the views are walked once
// per chunk and every view's (maximum, sum) is kept in LDS from the first walk.  Bound: ALU, about 3 * V * C logit
// evaluations and V * C expf per output pixel; one byte of HBM written.

#define SEG_MAX_VIEWS SEGCLIP_SEG_MAX_VIEWS
#define SEG_VIEW_COLS SEGCLIP_SEG_VIEW_COLS                   // int64 columns of one row of the view table: first image-table row, view count
#define SEG_AUG_LDS_BYTES (96 * 1024)     // dynamic LDS the launch may ask for (beside about 7 KiB of static LDS)
enum { VG_H, VG_W, VG_WIN_H, VG_WIN_W, VG_GH, VG_GW, VG_FLAGS, VG_FIRST, VG_COUNT, VG_N };

struct SegViewsArgs {
  SegEvalArgs e;          // images: one row per view; labels / gt / areas as in the rescaled entry
  const int64_t* views;   // (B, SEG_VIEW_COLS)
  int n_rows;             // rows of e.images
  int acc_classes;        // classes of one accumulator chunk
  int ms_views;           // views whose (maximum, sum) are kept in LDS: 0 when one chunk holds every class
  int max_views;          // the caller's bound on an image's view count: the (maximum, sum) slots are sized by it
  float* probs;           // (C, oh, ow) of the single image   [DENSE]
  int64_t probs_floats;
};

// the one place a soft-max numerator is formed: p = seg_exp_shift(v, max) / sum of seg_exp_shift over the classes
__device__ __forceinline__ float seg_exp_shift(float v, float m) { return expf(v - m); }

// The four taps of one output pixel in one view: covering-window lists and weights.  This kernel keeps its own statement of
// seg_pixel_taps / seg_blend_taps (segment_tile.inc) and its own pixel loop: segclip_seg_view_probs writes the floats
// themselves, and built from the shared pair the kernel rounded a few of them differently in the last bits and ran slower
// (profiles/seg_tile_refactor.txt).  The row check, the window compaction and the table staging are the shared ones.
struct SegViewTaps {
  const uint16_t *c0, *c1, *c2, *c3;
  int n0, n1, n2, n3;
  float hy, ly, hx, lx;
};

// class c's logit at the pixel: the blend of segclip_seg_label_map_rescaled, a tap evaluated once however often it is shared
__device__ __forceinline__ float seg_view_logit(const SegTables& tb, int c, const SegViewTaps& t, int tid) {
  const float v00 = t.n0 ? seg_class_logit(tb, c, t.n0, t.c0, tid) : 0.f;
  const float v01 = t.c1 == t.c0 ? v00 : (t.n1 ? seg_class_logit(tb, c, t.n1, t.c1, tid) : 0.f);
  const float v10 = t.c2 == t.c0 ? v00 : (t.n2 ? seg_class_logit(tb, c, t.n2, t.c2, tid) : 0.f);
  const float v11 = t.c3 == t.c1 ? v01 : (t.c3 == t.c2 ? v10 : (t.n3 ? seg_class_logit(tb, c, t.n3, t.c3, tid) : 0.f));
  return t.hy * (t.hx * v00 + t.lx * v01) + t.ly * (t.hx * v10 + t.lx * v11);
}

// A workgroup owns SEG_EVAL_TILE consecutive pixels of one image's flat (oh, ow) output.  Labels: a lane owns four consecutive
// pixels (one dword store); probabilities: pixel q * 256 + lane of the tile, so that a wave stores 256 consecutive bytes per
// class.  Every entry of both tables is range-checked here (the view rows by seg_tile_row); an image with one inconsistent
// view is skipped.
template <bool DENSE>
__global__ __launch_bounds__(256) void seg_views_kernel(SegViewsArgs VA) {
  const SegEvalArgs& A = VA.e;
  __shared__ int s_wy[SEG_MAX_IMG_WIN], s_wx[SEG_MAX_IMG_WIN], s_wi[SEG_MAX_IMG_WIN], s_row[SEG_MAX_IMG_WIN];
  const SegWinLists L = {s_wy, s_wx, s_wi, s_row};
  __shared__ uint8_t s_bg[SEG_MAX_IMG_WIN * SEG_MAX_G];
  __shared__ int s_cnt[3 * SEG_MAX_CLASSES];
  __shared__ int s_img;
  __shared__ int s_vfirst[SEG_MAX_VIEWS + 1];   // view -> its first entry of the block's window list
  __shared__ int s_vgeo[SEG_MAX_VIEWS][VG_N];
  __shared__ int64_t s_vsoft[SEG_MAX_VIEWS];    // window k of the view at soft + s_vsoft[v] + k * G * gh * gw (k: index in `windows`)
  // dynamic LDS: table copies | accumulators (acc_classes, 256) | (maximum, sum) (ms_views, 2, 256) | four taps x cover_slots x 256
  extern __shared__ float s_dyn[];
  float* s_tab = s_dyn;
  float* s_acc = s_dyn + A.tab_floats;
  float* s_ms = s_acc + VA.acc_classes * 256;
  uint16_t* s_cov = reinterpret_cast<uint16_t*>(s_ms + VA.ms_views * 2 * 256);

  const int tid = threadIdx.x;
  const int off = A.with_bg ? 1 : 0;
  const int C = A.N + off;
  const int64_t last_row = VA.n_rows - 1;
  if (tid == 0) {  // the last image whose first workgroup is not after this one
    int lo = 0, hi = A.B - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      int64_t r = VA.views[(int64_t)mid * SEG_VIEW_COLS];
      r = r < 0 ? 0 : (r > last_row ? last_row : r);
      if (A.images[r * SEG_IMG_COLS + SI_BLK] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_img = lo;
  }
  for (int i = tid; i < 3 * C; i += 256) s_cnt[i] = 0;
  __syncthreads();

  const int64_t row0 = VA.views[(int64_t)s_img * SEG_VIEW_COLS], nv64 = VA.views[(int64_t)s_img * SEG_VIEW_COLS + 1];
  // block-uniform; an image with more views than the caller stated is skipped: the (maximum, sum) slots would not hold them
  if (row0 < 0 || nv64 < 1 || nv64 > SEG_MAX_VIEWS || nv64 > VA.max_views || row0 + nv64 > VA.n_rows) return;
  const int nv = (int)nv64;
  const int64_t* D0 = A.images + row0 * SEG_IMG_COLS;
  const int64_t oh = D0[SI_OH], ow = D0[SI_OW], lab_off = D0[SI_LAB], gt_off = D0[SI_GT];
  const int64_t lim = 1ll << 30;
  if (!(oh >= 1 && ow >= 1 && oh < lim && ow < lim && oh * ow < (1ll << 31))) return;
  const int64_t total = oh * ow;
  const int64_t p0 = ((int64_t)blockIdx.x - D0[SI_BLK]) * SEG_EVAL_TILE;
  if (p0 < 0 || p0 >= total) return;
  const bool write = DENSE ? (VA.probs && (int64_t)C * total <= VA.probs_floats)
                           : (A.labels && lab_off >= 0 && lab_off + total <= A.labels_bytes);
  const bool score = !DENSE && A.gt && A.areas && gt_off >= 0 && gt_off + total <= A.gt_bytes;
  if (!(write || score)) return;

  // every view's row, checked as the single-view kernels check their image's
  bool okv = true;
  if (tid < nv) {
    const int64_t* D = D0 + (int64_t)tid * SEG_IMG_COLS;
    SegTileRow r;
    okv = seg_tile_row(D, A.n_windows, A.G, A.soft_floats, r) && D[SI_OH] == oh && D[SI_OW] == ow;
    if (okv) {
      int* g = s_vgeo[tid];
      g[VG_H] = r.H; g[VG_W] = r.W; g[VG_WIN_H] = r.win_h; g[VG_WIN_W] = r.win_w; g[VG_GH] = r.gh; g[VG_GW] = r.gw;
      g[VG_FLAGS] = (int)(D[SI_FLAGS] & 3); g[VG_FIRST] = r.first; g[VG_COUNT] = r.n_img;
      s_vsoft[tid] = r.soft;
    }
  }
  if (!__syncthreads_and(okv ? 1 : 0)) return;

  // per view the windows that touch the source rows of this tile's output rows, in window order, one list for the block
  if (tid < 64) {
    const int64_t p_last = p0 + SEG_EVAL_TILE - 1 < total - 1 ? p0 + SEG_EVAL_TILE - 1 : total - 1;
    const int ya = (int)((uint32_t)p0 / (uint32_t)ow), yb = (int)((uint32_t)p_last / (uint32_t)ow);
    int n = 0;
    for (int v = 0; v < nv; ++v) {
      const int* g = s_vgeo[v];
      if (tid == 0) s_vfirst[v] = n;
      const bool vflip = (g[VG_FLAGS] & 2) != 0;
      const float ry = (float)g[VG_H] / (float)oh;
      int sy_lo, sy_hi, t;
      float l;
      seg_axis_taps(vflip ? (int)oh - 1 - yb : ya, ry, g[VG_H], sy_lo, t, l);
      seg_axis_taps(vflip ? (int)oh - 1 - ya : yb, ry, g[VG_H], t, sy_hi, l);
      n = seg_window_compact(A.windows, g[VG_FIRST], g[VG_COUNT], g[VG_WIN_H], sy_lo, sy_hi, L, n, tid);
    }
    if (tid == 0) s_vfirst[nv] = n;
  }
  __syncthreads();
  const int nwin = s_vfirst[nv];
  for (int i = tid; i < nwin * A.G; i += 256) {  // the background indicator, as in seg_pixel_kernel
    const int k = i / A.G, g = i % A.G;
    const float sc = A.best_score[(int64_t)s_wi[k] * A.G + g];
    s_bg[k * SEG_MAX_G + g] = (A.with_bg && sc < fminf(A.bg_thresh, A.table_max[s_wi[k]])) ? 1 : 0;
  }
  const bool staged = seg_stage_tables(A.table, A.G, A.N, L, nwin, s_tab, A.tab_floats, tid);
  __syncthreads();

  const int slots = A.cover_slots;
  uint16_t* const b0 = s_cov;
  uint16_t* const b1 = s_cov + slots * 256;
  uint16_t* const b2 = s_cov + 2 * slots * 256;
  uint16_t* const b3 = s_cov + 3 * slots * 256;
  const int CH = VA.acc_classes;
  const float n_views = (float)nv;

  const int64_t pq = p0 + (int64_t)tid * SEG_EVAL_PPL;
  uint32_t pack = 0;
  int run_p = -1, run_g = -1, run_n = 0;
  for (int q = 0; q < SEG_EVAL_PPL; ++q) {
    const int64_t p = DENSE ? p0 + q * 256 + tid : pq + q;
    if (p >= total) break;  // later pixels of the lane lie further on in both numberings
    const int y = (int)((uint32_t)p / (uint32_t)ow), x = (int)((uint32_t)p % (uint32_t)ow);
    float best = -INFINITY;
    int lab = 0;
    for (int c0 = 0; c0 < C; c0 += CH) {
      const int cn = C - c0 < CH ? C - c0 : CH;
      for (int j = 0; j < cn; ++j) s_acc[j * 256 + tid] = 0.f;
      for (int v = 0; v < nv; ++v) {
        const int* g = s_vgeo[v];
        const int H = g[VG_H], W = g[VG_W], win_h = g[VG_WIN_H], win_w = g[VG_WIN_W], gh = g[VG_GH], gw = g[VG_GW];
        // mmseg flips the probability map back at the output size: the view is read at the mirrored output position
        const int ys = (g[VG_FLAGS] & 2) ? (int)oh - 1 - y : y, xs = (g[VG_FLAGS] & 1) ? (int)ow - 1 - x : x;
        const int vf = s_vfirst[v];
        SegBlockWindows bw = {s_wy + vf, s_wx + vf, s_wi + vf, s_vfirst[v + 1] - vf};
        SegTables tb = {staged ? (const float*)s_tab : A.table, s_row + vf, s_bg + vf * SEG_MAX_G, A.G, A.N, off};
        const float* soft = A.soft + s_vsoft[v];
        const float sy = (float)gh / (float)win_h, sx = (float)gw / (float)win_w;
        int ya, yb, xa, xb;
        SegViewTaps t;
        seg_axis_taps(ys, (float)H / (float)oh, H, ya, yb, t.ly);
        seg_axis_taps(xs, (float)W / (float)ow, W, xa, xb, t.lx);
        if (t.ly == 0.f) yb = ya;  // a tap of weight 0 is not evaluated
        if (t.lx == 0.f) xb = xa;
        t.hy = 1.f - t.ly; t.hx = 1.f - t.lx;
#define SEG_COVER(yy, xx, buf) seg_pixel_cover(bw, soft, yy, xx, win_h, win_w, gh, gw, A.G, sy, sx, buf, slots, tid)
        t.c0 = t.c1 = t.c2 = b0;
        t.n0 = SEG_COVER(ya, xa, b0);
        t.n1 = t.n2 = t.n0;
        if (xb != xa) { t.n1 = SEG_COVER(ya, xb, b1); t.c1 = b1; }
        if (yb != ya) { t.n2 = SEG_COVER(yb, xa, b2); t.c2 = b2; }
        if (yb == ya) { t.c3 = t.c1; t.n3 = t.n1; }
        else if (xb == xa) { t.c3 = t.c2; t.n3 = t.n2; }
        else { t.n3 = SEG_COVER(yb, xb, b3); t.c3 = b3; }
#undef SEG_COVER
        float m, s;
        if (c0 == 0) {
          m = -INFINITY;
          for (int c = 0; c < C; ++c) m = fmaxf(m, seg_view_logit(tb, c, t, tid));
          s = 0.f;
          for (int c = 0; c < C; ++c) s += seg_exp_shift(seg_view_logit(tb, c, t, tid), m);
          if (v < VA.ms_views) { s_ms[(2 * v) * 256 + tid] = m; s_ms[(2 * v + 1) * 256 + tid] = s; }
        } else {  // a second chunk exists: ms_views = max_views >= nv, checked above
          m = s_ms[(2 * v) * 256 + tid];
          s = s_ms[(2 * v + 1) * 256 + tid];
        }
        for (int j = 0; j < cn; ++j) s_acc[j * 256 + tid] += seg_exp_shift(seg_view_logit(tb, c0 + j, t, tid), m) / s;
      }
      for (int j = 0; j < cn; ++j) {
        const float mean = s_acc[j * 256 + tid] / n_views;
        if (DENSE) {
          if (write) VA.probs[(int64_t)(c0 + j) * total + p] = mean;
        } else if (mean > best) { best = mean; lab = c0 + j; }
      }
    }
    if (DENSE) continue;
    pack |= (uint32_t)(lab & 255) << (8 * q);
    if (score) {
      const int g = A.gt[gt_off + p];
      if (lab == run_p && g == run_g) {
        ++run_n;
      } else {
        if (run_n) seg_area_add(s_cnt, C, run_p, run_g, A.ignore_index, A.reduce_zero, run_n);
        run_p = lab; run_g = g; run_n = 1;
      }
    }
  }
  if (DENSE) return;
  if (run_n) seg_area_add(s_cnt, C, run_p, run_g, A.ignore_index, A.reduce_zero, run_n);
  if (write && pq < total) {
    uint8_t* o = A.labels + lab_off + pq;
    if (pq + SEG_EVAL_PPL <= total && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(o) = pack;
    } else {
      for (int q = 0; q < SEG_EVAL_PPL && pq + q < total; ++q) o[q] = (uint8_t)(pack >> (8 * q));
    }
  }
  if (score) {
    __syncthreads();
    seg_area_flush(s_cnt, C, A.areas, tid);
  }
}
