// Zero-shot segmentation evaluation (segment.hip): label maps at the ground truth's size for images of mixed sizes, and the
// per-class areas of the mIoU (mmseg's resize(size=ori_shape) -> arg-max -> intersect_and_union), without a (C, oh, ow) or
// (C, H, W) tensor: every output pixel blends the class logits of its four source pixels, which are formed by the device
// functions of segment_pixel.inc exactly as segclip_seg_logits writes them.

#define SEG_IMG_COLS 16        // int64 columns of one image row of the descriptor table (segclip_hip.h)
#define SEG_EVAL_PPL 4         // consecutive output pixels of a lane
#define SEG_EVAL_TILE 1024     // output pixels of a workgroup
#define SEG_EVAL_TAB_FLOATS 4096
#define SEG_MAX_CLASSES 256
enum { SI_FIRST, SI_COUNT, SI_H, SI_W, SI_OH, SI_OW, SI_LAB, SI_GT, SI_BLK, SI_WIN_H, SI_WIN_W, SI_GH, SI_GW, SI_SOFT };

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

__global__ __launch_bounds__(256) void seg_areas_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t n,
                                                        int C, int ignore_index, int reduce_zero, unsigned long long* areas) {
  __shared__ int s_cnt[3 * SEG_MAX_CLASSES];
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * C; i += 256) s_cnt[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256)
    seg_area_add(s_cnt, C, pred[i], gt[i], ignore_index, reduce_zero, 1);
  __syncthreads();
  seg_area_flush(s_cnt, C, areas, tid);
}

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

// equal covering-window lists: the two source pixels have the same class logits
__device__ __forceinline__ bool seg_same_cover(const uint16_t* a, int na, const uint16_t* b, int nb, int tid) {
  if (a == b) return true;
  if (na != nb) return false;
  for (int j = 0; j < na; ++j)
    if (a[j * 256 + tid] != b[j * 256 + tid]) return false;
  return true;
}

// A workgroup owns SEG_EVAL_TILE consecutive pixels of one image's flat (oh, ow) output, a lane four of them (one dword store:
// the host aligns every image's label offset to 4).  The workgroups of all images are numbered through; row[SI_BLK] of the
// table is an image's first workgroup.  Every table entry is range-checked here: the host entry cannot inspect device memory.
__global__ __launch_bounds__(256) void seg_rescaled_kernel(SegEvalArgs A) {
  __shared__ int s_wy[SEG_MAX_IMG_WIN], s_wx[SEG_MAX_IMG_WIN], s_wi[SEG_MAX_IMG_WIN], s_row[SEG_MAX_IMG_WIN];
  __shared__ int s_n, s_img;
  __shared__ uint8_t s_bg[SEG_MAX_IMG_WIN * SEG_MAX_G];
  __shared__ uint8_t s_lab[SEG_MAX_IMG_WIN * SEG_MAX_G];
  __shared__ int s_cnt[3 * SEG_MAX_CLASSES];
  // dynamic LDS: A.tab_floats floats of table copies, then four taps x A.cover_slots x 256 covering-window entries
  extern __shared__ float s_dyn[];
  float* s_tab = s_dyn;
  uint16_t* s_cov = reinterpret_cast<uint16_t*>(s_dyn + A.tab_floats);

  const int tid = threadIdx.x;
  const int off = A.with_bg ? 1 : 0;
  const int C = A.N + off;
  if (tid == 0) {  // the last image whose first workgroup is not after this one
    int lo = 0, hi = A.B - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (A.images[(int64_t)mid * SEG_IMG_COLS + SI_BLK] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_img = lo;
  }
  for (int i = tid; i < 3 * C; i += 256) s_cnt[i] = 0;
  __syncthreads();

  const int64_t* D = A.images + (int64_t)s_img * SEG_IMG_COLS;
  const int64_t H = D[SI_H], W = D[SI_W], oh = D[SI_OH], ow = D[SI_OW], win_h = D[SI_WIN_H], win_w = D[SI_WIN_W];
  const int64_t gh = D[SI_GH], gw = D[SI_GW], soft_off = D[SI_SOFT], lab_off = D[SI_LAB], gt_off = D[SI_GT];
  int64_t first = D[SI_FIRST], count = D[SI_COUNT];
  first = first < 0 ? 0 : (first > A.n_windows ? A.n_windows : first);
  count = count < 0 ? 0 : (count > A.n_windows - first ? A.n_windows - first : count);
  const int n_img = (int)(count < SEG_MAX_IMG_WIN ? count : SEG_MAX_IMG_WIN);
  const int64_t lim = 1ll << 30;
  bool ok = H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && win_h >= 1 && win_w >= 1 && gh >= 1 && gw >= 1 && H < lim && W < lim &&
            oh < lim && ow < lim && win_h < lim && win_w < lim && gh * gw * A.G < lim && oh * ow < (1ll << 31);
  ok = ok && soft_off >= 0 && soft_off + count * A.G * gh * gw <= A.soft_floats;
  const int64_t total = ok ? oh * ow : 0;
  const int64_t p0 = ((int64_t)blockIdx.x - D[SI_BLK]) * SEG_EVAL_TILE;
  const bool active = p0 >= 0 && p0 < total;
  const bool write = A.labels && lab_off >= 0 && lab_off + total <= A.labels_bytes;
  const bool score = A.gt && A.areas && gt_off >= 0 && gt_off + total <= A.gt_bytes;
  if (!active || !(write || score)) return;  // block-uniform, and nothing was counted

  const float ry = (float)H / (float)oh, rx = (float)W / (float)ow;
  // source rows of this tile's output rows -> the image's windows that touch them, in window order
  int sy_lo, sy_hi;
  {
    const int64_t p_last = p0 + SEG_EVAL_TILE - 1 < total - 1 ? p0 + SEG_EVAL_TILE - 1 : total - 1;
    int t;
    float l;
    seg_axis_taps((int)((uint32_t)p0 / (uint32_t)ow), ry, (int)H, sy_lo, t, l);
    seg_axis_taps((int)((uint32_t)p_last / (uint32_t)ow), ry, (int)H, t, sy_hi, l);
  }
  if (tid < 64) {
    bool p = false;
    int wy = 0, wx = 0;
    if (tid < n_img) {
      wy = A.windows[3 * (first + tid) + 1];
      wx = A.windows[3 * (first + tid) + 2];
      p = wy <= sy_hi && (int64_t)wy + win_h > sy_lo;
    }
    const unsigned long long m = __ballot(p);
    if (p) {
      const int pos = __popcll(m & ((1ull << tid) - 1ull));
      s_wy[pos] = wy; s_wx[pos] = wx; s_wi[pos] = (int)first + tid;
    }
    if (tid == 0) s_n = __popcll(m);
  }
  __syncthreads();
  const int nwin = s_n;
  for (int i = tid; i < nwin * A.G; i += 256) {  // as in seg_pixel_kernel
    const int k = i / A.G, g = i % A.G;
    const int64_t wg = (int64_t)s_wi[k] * A.G + g;
    const float sc = A.best_score[wg];
    const bool bg = A.with_bg && sc < fminf(A.bg_thresh, A.table_max[s_wi[k]]);
    s_bg[k * SEG_MAX_G + g] = bg ? 1 : 0;
    s_lab[k * SEG_MAX_G + g] = (uint8_t)(A.with_bg ? ((bg || !(sc > 0.f)) ? 0 : A.best_class[wg] + 1) : A.best_class[wg]);
  }
  const bool staged = (int64_t)nwin * A.G * A.N <= A.tab_floats;
  if (staged) {
    const int per = A.G * A.N;
    for (int i = tid; i < nwin * per; i += 256) s_tab[i] = A.table[(int64_t)s_wi[i / per] * per + i % per];
  }
  for (int k = tid; k < nwin; k += 256) s_row[k] = staged ? k : s_wi[k];
  __syncthreads();

  SegBlockWindows bw = {s_wy, s_wx, s_wi, nwin};
  SegTables tb = {staged ? (const float*)s_tab : A.table, s_row, s_bg, A.G, A.N, off};
  const float sy = (float)gh / (float)win_h, sx = (float)gw / (float)win_w;
  // seg_pixel_cover indexes soft by the window's number in the list
  const float* soft = A.soft + (soft_off - first * A.G * gh * gw);
  const int slots = A.cover_slots;
  uint16_t* const c0 = s_cov;
  uint16_t* const b1 = s_cov + slots * 256;
  uint16_t* const b2 = s_cov + 2 * slots * 256;
  uint16_t* const b3 = s_cov + 3 * slots * 256;

  const int64_t pq = p0 + (int64_t)tid * SEG_EVAL_PPL;
  uint32_t pack = 0;
  int run_p = -1, run_g = -1, run_n = 0;  // equal (prediction, ground truth) pairs of the lane's pixels are counted once
  for (int q = 0; q < SEG_EVAL_PPL; ++q) {
    const int64_t p = pq + q;
    if (p >= total) break;
    const int y = (int)((uint32_t)p / (uint32_t)ow), x = (int)((uint32_t)p % (uint32_t)ow);
    int ya, yb, xa, xb;
    float ly, lx;
    seg_axis_taps(y, ry, (int)H, ya, yb, ly);
    seg_axis_taps(x, rx, (int)W, xa, xb, lx);
    // a tap of weight 0 adds 0 * (a finite logit): it may be any pixel, so take the one already resolved
    if (ly == 0.f) yb = ya;
    if (lx == 0.f) xb = xa;
#define SEG_COVER(yy, xx, buf) seg_pixel_cover(bw, soft, yy, xx, (int)win_h, (int)win_w, (int)gh, (int)gw, A.G, sy, sx, buf, slots, tid)
    const uint16_t *c1 = c0, *c2 = c0, *c3;
    const int n0 = SEG_COVER(ya, xa, c0);
    int n1 = n0, n2 = n0, n3;
    if (xb != xa) { n1 = SEG_COVER(ya, xb, b1); c1 = b1; }
    if (yb != ya) { n2 = SEG_COVER(yb, xa, b2); c2 = b2; }
    if (yb == ya) { c3 = c1; n3 = n1; }
    else if (xb == xa) { c3 = c2; n3 = n2; }
    else { n3 = SEG_COVER(yb, xb, b3); c3 = b3; }
#undef SEG_COVER
    int lab = 0;
    if (seg_same_cover(c0, n0, c1, n1, tid) && seg_same_cover(c0, n0, c2, n2, tid) && seg_same_cover(c0, n0, c3, n3, tid)) {
      // the four source pixels have one logit vector v, and the blend is monotone in v: its first maximum is v's (two
      // classes can change places only where the blend rounds their different logits to one value)
      if (n0 == 1) {
        const int e = c0[tid];
        lab = s_lab[(e >> 8) * SEG_MAX_G + (e & 255)];
      } else if (n0 > 1) {
        float best = -INFINITY;
        for (int c = 0; c < C; ++c) {
          const float v = seg_class_logit(tb, c, n0, c0, tid);
          if (v > best) { best = v; lab = c; }
        }
      }
    } else {
      const float hy = 1.f - ly, hx = 1.f - lx;
      float best = -INFINITY;
      for (int c = 0; c < C; ++c) {
        const float v00 = n0 ? seg_class_logit(tb, c, n0, c0, tid) : 0.f;
        const float v01 = c1 == c0 ? v00 : (n1 ? seg_class_logit(tb, c, n1, c1, tid) : 0.f);
        const float v10 = c2 == c0 ? v00 : (n2 ? seg_class_logit(tb, c, n2, c2, tid) : 0.f);
        const float v11 = c3 == c1 ? v01 : (c3 == c2 ? v10 : (n3 ? seg_class_logit(tb, c, n3, c3, tid) : 0.f));
        const float v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
        if (v > best) { best = v; lab = c; }
      }
    }
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
