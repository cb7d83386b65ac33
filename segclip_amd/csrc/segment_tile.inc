// The parts that the label-map kernels of segment.hip are assembled from: the descriptor table and its one device-side row check,
// the block's window list, table copies and per-(window, group) labels, the four taps of a rescaled pixel and their one blend,
// the mIoU counters with the run-length counting of a lane's pixels, and the packed store of a lane's four labels.  The kernels
// promise each other bit-equal labels (wide = narrow below 257 classes, sweep = the single threshold, label = first maximum of
// the dense logits): every expression a label depends on is written here once.  One text is not one rounding - the compiler
// contracts a blend to FMAs per inlining context - so the equality tests of the entries remain what guards the promise.

#define SEG_IMG_COLS SEGCLIP_SEG_IMAGE_COLS        // int64 columns of one image row of the descriptor table (segclip_hip.h)
#define SEG_EVAL_PPL 4         // consecutive output pixels of a lane
#define SEG_EVAL_TILE SEGCLIP_SEG_EVAL_TILE     // output pixels of a workgroup
// the columns of enum segclip_seg_image_col (segclip_hip.h) under the kernels' short names
#define SI_(X) SI_##X = SEGCLIP_SI_##X
enum { SI_(FIRST), SI_(COUNT), SI_(H), SI_(W), SI_(OH), SI_(OW), SI_(LAB), SI_(GT), SI_(BLK), SI_(WIN_H), SI_(WIN_W), SI_(GH), SI_(GW), SI_(SOFT),
       SI_(FLAGS) };
#undef SI_

struct SegEvalArgs {
  const float* soft;           // flat; window k of image i at soft + row[SI_SOFT] + (k - row[SI_FIRST]) * G * gh * gw
  const float* table;          // (n_windows, G, N)
  const float* table_max;      // (n_windows)
  const int32_t* best_class;   // (n_windows, G)
  const float* best_score;     // (n_windows, G)
  const int32_t* windows;      // (n_windows, 3): image, y0, x0
  const int64_t* images;       // (B, SEG_IMG_COLS)
  int64_t soft_floats, labels_bytes, gt_bytes;
  int n_windows, B, G, N, with_bg;
  int tab_floats, cover_slots;
  float bg_thresh;
  uint8_t* labels;             // flat, or null
  const uint8_t* gt;           // flat, or null
  int ignore_index, reduce_zero;
  unsigned long long* areas;   // (3, N + with_bg), or null
};

// ---------------------------------------------------------------- the descriptor table
// The workgroups of all images are numbered through, and a table row names its image's first workgroup (column `col` of a table
// of `cols` columns): -> the last image whose first workgroup is not after this one.
__device__ __forceinline__ int seg_block_image(const int64_t* images, int B, int cols, int col, int64_t block) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (images[(int64_t)mid * cols + col] <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The network side of a table row (an image, or one view of it), range-checked: the host entry cannot inspect device memory.
struct SegTileRow {
  int H, W, win_h, win_w, gh, gw;
  int first, n_img;   // its windows in the window list, at most SEG_MAX_IMG_WIN of them
  int64_t soft;       // window k of the window list at soft + this + k * G * gh * gw (seg_pixel_cover indexes soft by k)
};
__device__ __forceinline__ bool seg_tile_row(const int64_t* D, int n_windows, int G, int64_t soft_floats, SegTileRow& r) {
  const int64_t H = D[SI_H], W = D[SI_W], win_h = D[SI_WIN_H], win_w = D[SI_WIN_W], gh = D[SI_GH], gw = D[SI_GW];
  const int64_t soft_off = D[SI_SOFT];
  int64_t first = D[SI_FIRST], count = D[SI_COUNT];
  first = first < 0 ? 0 : (first > n_windows ? n_windows : first);
  count = count < 0 ? 0 : (count > n_windows - first ? n_windows - first : count);
  const int64_t lim = 1ll << 30;
  bool ok = H >= 1 && W >= 1 && win_h >= 1 && win_w >= 1 && gh >= 1 && gw >= 1 && H < lim && W < lim && win_h < lim && win_w < lim &&
            gh * gw * G < lim;
  ok = ok && soft_off >= 0 && soft_off + count * G * gh * gw <= soft_floats;
  r.H = (int)H; r.W = (int)W; r.win_h = (int)win_h; r.win_w = (int)win_w; r.gh = (int)gh; r.gw = (int)gw;
  r.first = (int)first;
  r.n_img = (int)(count < SEG_MAX_IMG_WIN ? count : SEG_MAX_IMG_WIN);
  r.soft = soft_off - first * G * gh * gw;
  return ok;
}

// The output side of a row: a workgroup owns SEG_EVAL_TILE consecutive pixels of its image's flat (oh, ow) output.
struct SegTileOut {
  int oh, ow;
  int64_t total;             // oh * ow; 0: the row is refused, and no workgroup has a pixel of it
  int64_t p0;                // this workgroup's first pixel; it has work where 0 <= p0 < total
  int64_t lab_off, gt_off;   // in elements; checked against the buffers by the kernel, whose element types differ
};
__device__ __forceinline__ SegTileOut seg_tile_out(const int64_t* D) {
  const int64_t oh = D[SI_OH], ow = D[SI_OW], lim = 1ll << 30;
  const bool ok = oh >= 1 && ow >= 1 && oh < lim && ow < lim && oh * ow < (1ll << 31);
  SegTileOut o;
  o.oh = (int)oh; o.ow = (int)ow;
  o.total = ok ? oh * ow : 0;
  o.p0 = ((int64_t)blockIdx.x - D[SI_BLK]) * SEG_EVAL_TILE;
  o.lab_off = D[SI_LAB]; o.gt_off = D[SI_GT];
  return o;
}

// The row check of the single-view kernels: both sides of row `img`.
struct SegTile : SegTileRow, SegTileOut {};
__device__ __forceinline__ SegTile seg_tile_load(const SegEvalArgs& A, int img) {
  const int64_t* D = A.images + (int64_t)img * SEG_IMG_COLS;
  SegTile t;
  static_cast<SegTileOut&>(t) = seg_tile_out(D);
  if (!seg_tile_row(D, A.n_windows, A.G, A.soft_floats, t)) t.total = 0;
  return t;
}

// The scales of the two resamplings of a row: output -> network pixels (ry, rx), window pixels -> grid cells (sy, sx).
struct SegScales { float ry, rx, sy, sx; };
__device__ __forceinline__ SegScales seg_row_scales(const SegTileRow& r, int oh, int ow) {
  return {(float)r.H / (float)oh, (float)r.W / (float)ow, (float)r.gh / (float)r.win_h, (float)r.gw / (float)r.win_w};
}

// ---------------------------------------------------------------- the block's windows
struct SegWinLists {   // LDS arrays of SEG_MAX_IMG_WIN entries each
  int *wy, *wx;   // y0, x0
  int* wi;        // index into the window list (= row of soft_attn and of the tables)
  int* row;       // row of the table the kernel reads (seg_stage_tables)
};

// The windows first .. first + n - 1 of the window list (n <= 64 = one wave: ordered compaction by ballot) that touch the rows
// y_lo .. y_hi, appended in window order to the lists from position `base` on, of which SEG_MAX_IMG_WIN are kept.  All 64 lanes
// of the block's first wave call it; -> the lists' new length.
__device__ __forceinline__ int seg_window_compact(const int32_t* windows, int first, int n, int win_h, int y_lo, int y_hi,
                                                  const SegWinLists& L, int base, int lane) {
  bool p = false;
  int wy = 0, wx = 0;
  if (lane < n) {
    wy = windows[3 * (first + lane) + 1];
    wx = windows[3 * (first + lane) + 2];
    p = wy <= y_hi && (int64_t)wy + win_h > y_lo;
  }
  const unsigned long long m = __ballot(p);
  const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
  if (p && pos < SEG_MAX_IMG_WIN) { L.wy[pos] = wy; L.wx[pos] = wx; L.wi[pos] = first + lane; }
  const int end = base + __popcll(m);
  return end < SEG_MAX_IMG_WIN ? end : SEG_MAX_IMG_WIN;
}

// seg_window_compact for the windows of row `r` that touch the source rows of the output rows ya .. yb.
__device__ __forceinline__ int seg_row_windows(const int32_t* windows, const SegTileRow& r, int oh, int ya, int yb, const SegWinLists& L,
                                               int base, int lane) {
  const float ry = (float)r.H / (float)oh;
  int sy_lo, sy_hi, t;
  float l;
  seg_axis_taps(ya, ry, r.H, sy_lo, t, l);
  seg_axis_taps(yb, ry, r.H, t, sy_hi, l);
  return seg_window_compact(windows, r.first, r.n_img, r.win_h, sy_lo, sy_hi, L, base, lane);
}

// The output rows of a tile.
__device__ __forceinline__ void seg_tile_rows(const SegTileOut& o, int& ya, int& yb) {
  const int64_t p_last = o.p0 + SEG_EVAL_TILE - 1 < o.total - 1 ? o.p0 + SEG_EVAL_TILE - 1 : o.total - 1;
  ya = (int)((uint32_t)o.p0 / (uint32_t)o.ow);
  yb = (int)((uint32_t)p_last / (uint32_t)o.ow);
}

// The windows of a single-view tile, with the barrier that publishes them.  Every thread calls it; -> their number.
__device__ __forceinline__ int seg_tile_windows(const int32_t* windows, const SegTile& T, const SegWinLists& L, int* s_n, int tid) {
  if (tid < 64) {
    int ya, yb;
    seg_tile_rows(T, ya, yb);
    const int n = seg_row_windows(windows, T, T.oh, ya, yb, L, 0, tid);
    if (tid == 0) *s_n = n;
  }
  __syncthreads();
  return *s_n;
}

// Per (window, group) of the block's list: the background indicator and the single-window label, which is the first maximum of
// [bg, row]: bg = 1 beats every table entry (score < table_max <= 1); an all-zero row gives 0.
template <typename T>
__device__ __forceinline__ void seg_window_labels(const float* best_score, const float* table_max, const int32_t* best_class,
                                                  int with_bg, float bg_thresh, int G, const SegWinLists& L, int nwin, uint8_t* s_bg,
                                                  T* s_lab, int tid) {
  for (int i = tid; i < nwin * G; i += 256) {
    const int k = i / G, g = i % G;
    const int64_t wg = (int64_t)L.wi[k] * G + g;
    const float score = best_score[wg];
    const bool bg = with_bg && score < fminf(bg_thresh, table_max[L.wi[k]]);
    s_bg[k * SEG_MAX_G + g] = bg ? 1 : 0;
    s_lab[k * SEG_MAX_G + g] = (T)(with_bg ? ((bg || !(score > 0.f)) ? 0 : best_class[wg] + 1) : best_class[wg]);
  }
}

// The tables of the block's windows in LDS when they fit `room` floats (overlaps and the dense logits read N entries per pixel
// from them), and L.row.  Every thread calls it, a barrier follows; -> whether the kernel reads the copy, row k of which is
// the table of local window k, or the global table.
__device__ __forceinline__ bool seg_stage_tables(const float* table, int G, int N, const SegWinLists& L, int nwin, float* s_tab,
                                                 int room, int tid) {
  const bool staged = (int64_t)nwin * G * N <= room;
  if (staged) {
    const int per = G * N;
    for (int i = tid; i < nwin * per; i += 256) s_tab[i] = table[(int64_t)L.wi[i / per] * per + i % per];
  }
  for (int k = tid; k < nwin; k += 256) L.row[k] = staged ? k : L.wi[k];
  return staged;
}

// ---------------------------------------------------------------- the four taps of a rescaled pixel
// Their covering-window lists (aliases of one another where two taps are one source pixel) and the weights of the second tap
// per axis.
struct SegTaps {
  const uint16_t *c0, *c1, *c2, *c3;
  int n0, n1, n2, n3;
  float ly, lx;
};

// Output pixel (y, x) of row `r`.  cov: four lists of `slots` x 256 entries; the lane writes column `tid` of those it needs.
__device__ __forceinline__ SegTaps seg_pixel_taps(const SegBlockWindows& bw, const float* soft, const SegTileRow& r, const SegScales& sc,
                                                  int G, int y, int x, uint16_t* cov, int slots, int tid) {
  uint16_t* const b1 = cov + slots * 256;
  uint16_t* const b2 = cov + 2 * slots * 256;
  uint16_t* const b3 = cov + 3 * slots * 256;
  SegTaps t;
  int ya, yb, xa, xb;
  seg_axis_taps(y, sc.ry, r.H, ya, yb, t.ly);
  seg_axis_taps(x, sc.rx, r.W, xa, xb, t.lx);
  // a tap of weight 0 adds 0 * (a finite logit): it may be any pixel, so take the one already resolved
  if (t.ly == 0.f) yb = ya;
  if (t.lx == 0.f) xb = xa;
#define SEG_COVER(yy, xx, buf) seg_pixel_cover(bw, soft, yy, xx, r.win_h, r.win_w, r.gh, r.gw, G, sc.sy, sc.sx, buf, slots, tid)
  t.c0 = t.c1 = t.c2 = cov;
  t.n0 = SEG_COVER(ya, xa, cov);
  t.n1 = t.n2 = t.n0;
  if (xb != xa) { t.n1 = SEG_COVER(ya, xb, b1); t.c1 = b1; }
  if (yb != ya) { t.n2 = SEG_COVER(yb, xa, b2); t.c2 = b2; }
  if (yb == ya) { t.c3 = t.c1; t.n3 = t.n1; }
  else if (xb == xa) { t.c3 = t.c2; t.n3 = t.n2; }
  else { t.n3 = SEG_COVER(yb, xb, b3); t.c3 = b3; }
#undef SEG_COVER
  return t;
}

// equal covering-window lists: the two source pixels have the same class logits
__device__ __forceinline__ bool seg_same_cover(const uint16_t* a, int na, const uint16_t* b, int nb, int tid) {
  if (a == b) return true;
  if (na != nb) return false;
  for (int j = 0; j < na; ++j)
    if (a[j * 256 + tid] != b[j * 256 + tid]) return false;
  return true;
}

// The four source pixels have one logit vector v.  The blend is monotone in v, so its first maximum is v's (two classes can
// change places only where the blend rounds their different logits to one value): such a pixel is decided without the blend.
__device__ __forceinline__ bool seg_taps_same(const SegTaps& t, int tid) {
  return seg_same_cover(t.c0, t.n0, t.c1, t.n1, tid) && seg_same_cover(t.c0, t.n0, t.c2, t.n2, tid) &&
         seg_same_cover(t.c0, t.n0, t.c3, t.n3, tid);
}

// The value of a class at an output pixel from tap(n, cov), its logit at a source pixel with n >= 1 covering windows: the plain
// logit where the taps have one logit vector (`same`), else the blend of the taps' logits in ATen's operation order, a tap
// evaluated once however often it is shared.
template <typename F>
__device__ __forceinline__ float seg_blend_taps(const SegTaps& t, bool same, F tap) {
  if (same) return tap(t.n0, t.c0);
  const float hy = 1.f - t.ly, hx = 1.f - t.lx;
  const float v00 = t.n0 ? tap(t.n0, t.c0) : 0.f;
  const float v01 = t.c1 == t.c0 ? v00 : (t.n1 ? tap(t.n1, t.c1) : 0.f);
  const float v10 = t.c2 == t.c0 ? v00 : (t.n2 ? tap(t.n2, t.c2) : 0.f);
  const float v11 = t.c3 == t.c1 ? v01 : (t.c3 == t.c2 ? v10 : (t.n3 ? tap(t.n3, t.c3) : 0.f));
  return hy * (hx * v00 + t.lx * v01) + t.ly * (hx * v10 + t.lx * v11);
}

// Class c.  col: the column of the cover lists, the thread that owns the pixel - every lane of a wave passes the same one in
// the wide kernel's cooperative scan (a same-address LDS read).
__device__ __forceinline__ float seg_blend_logit(const SegTables& tb, int c, const SegTaps& t, bool same, int col) {
  return seg_blend_taps(t, same, [&](int n, const uint16_t* cov) { return seg_class_logit(tb, c, n, cov, col); });
}

// ---------------------------------------------------------------- mIoU areas
// mmseg intersect_and_union on one pixel: prediction p, raw ground truth g.  The ignore value and, with reduce_zero_label,
// 0 contribute nothing; every other g is shifted down by one.  g >= C (histc drops it) counts in the prediction area only.
// cnt: (3, C) counters of the workgroup in LDS.
__device__ __forceinline__ void seg_area_add(int* cnt, int C, int p, int g, int ignore_index, int reduce_zero, int n) {
  if (g == ignore_index) return;
  if (reduce_zero) {
    if (g == 0) return;
    g -= 1;
  }
  if (p < C) atomicAdd(&cnt[C + p], n);
  if (g < C) {
    atomicAdd(&cnt[2 * C + g], n);
    if (p == g) atomicAdd(&cnt[p], n);
  }
}

// one global add per counter the workgroup touched; integer sums do not depend on the order of arrival
__device__ __forceinline__ void seg_area_flush(const int* cnt, int C, unsigned long long* areas, int tid) {
  for (int i = tid; i < 3 * C; i += 256)
    if (cnt[i]) atomicAdd(&areas[i], (unsigned long long)cnt[i]);
}

// Equal (prediction, ground truth) pairs of a lane's consecutive pixels are counted once: add() per pixel, flush() after the last.
struct SegAreaRun {
  int* cnt;
  int C, ignore_index, reduce_zero;
  int p = -1, g = -1, n = 0;
  __device__ __forceinline__ void flush() {
    if (n) seg_area_add(cnt, C, p, g, ignore_index, reduce_zero, n);
  }
  __device__ __forceinline__ void add(int lab, int gt) {
    if (lab == p && gt == g) { ++n; return; }
    flush();
    p = lab; g = gt; n = 1;
  }
};

// ---------------------------------------------------------------- a lane's four labels
// Label q in bits [q * 8 * sizeof(T), ...) of `pack`, `left` >= 1 pixels of the image from the lane's first on: one store where
// all four exist and the address allows it (the host aligns every image's label offset to 4), else one by one.
template <typename T, typename P>
__device__ __forceinline__ void seg_store_labels4(T* o, P pack, int64_t left) {
  static_assert(sizeof(P) == SEG_EVAL_PPL * sizeof(T), "four labels to a pack");
  if (left >= SEG_EVAL_PPL && (reinterpret_cast<uintptr_t>(o) & (sizeof(P) - 1)) == 0) {
    *reinterpret_cast<P*>(o) = pack;
  } else {
    for (int q = 0; q < SEG_EVAL_PPL && q < left; ++q) o[q] = (T)(pack >> (8 * sizeof(T) * q));
  }
}
