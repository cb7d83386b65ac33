// Background-threshold sweep (segment.hip): the label maps and mIoU areas of segclip_seg_label_map_rescaled for T ascending
// values of bg_thresh in ONE launch.  The threshold enters a pixel's logits through the background indicators of its covering
// (window, group) pairs alone, and over ascending thresholds an indicator can only switch on.  The class-0 logit is a monotone
// fp32 function of the indicators (weights >= 0; fp32 multiply, add and fma are monotone), the other classes do not see the
// threshold: a pixel has ONE foreground label f (its first maximum over the classes >= 1) and ONE switch index s, and its label
// is f for the thresholds t < s and 0 for t >= s.  Covers, taps and the foreground scan run once per pixel, by the device
// functions of segment_pixel.inc / segment_eval.inc; only the class-0 logit is evaluated per threshold, until it wins.

#define SEG_SWEEP_MAX_T 16
// dynamic LDS the launch may ask for: 16 KiB of tables + 32 KiB of cover lists + (2 * 17 + 1) * 256 counters, beside 3 KiB static
#define SEG_SWEEP_LDS_BYTES (88 * 1024)

struct SegSweepArgs {
  SegEvalArgs e;   // labels_bytes: of ONE plane; areas: (T, 3, N + 1); with_bg = 1, bg_thresh unused
  float thr[SEG_SWEEP_MAX_T];
  int T;
};

// class-0 logit of a tap at threshold index t: seg_class_logit's sum of the 1.f / 0.f indicators in window order, divided by the
// window count - the indicator of an entry is on from its switch index
__device__ __forceinline__ float seg_sweep_bg_logit(const uint8_t* sw, int t, int cnt, const uint16_t* cov, int tid) {
  float s = 0.f;
  for (int j = 0; j < cnt; ++j) {
    const int e = cov[j * 256 + tid];
    s += sw[(e >> 8) * SEG_MAX_G + (e & 255)] <= t ? 1.f : 0.f;
  }
  return s / (float)cnt;
}

// seg_area_add for the T slices at once.  A pixel (f, s) predicts f in the slices t < s and 0 in the slices t >= s (f == 0: s == 0),
// so it is counted in bucket [s][f] and, where it ever switches, in bucket [s][0]; seg_sweep_flush sums the buckets s > t of a class
// >= 1 and the buckets s <= t of class 0.  pre / inter: (T + 1, C) buckets, lab: (C) - the label area does not see the threshold.
__device__ __forceinline__ void seg_sweep_area_add(int* pre, int* inter, int* lab, int C, int T, int f, int s, int g, int ignore_index,
                                                   int reduce_zero, int n) {
  if (g == ignore_index) return;
  if (reduce_zero) {
    if (g == 0) return;
    g -= 1;
  }
  atomicAdd(&pre[s * C + f], n);
  if (f && s < T) atomicAdd(&pre[s * C], n);
  if (g < C) {
    atomicAdd(&lab[g], n);
    if (g == f) atomicAdd(&inter[s * C + f], n);
    else if (g == 0 && s < T) atomicAdd(&inter[s * C], n);
  }
}

// buckets -> slices, one global add per touched counter (integer sums: the order of arrival does not matter)
__device__ __forceinline__ void seg_sweep_flush(const int* pre, const int* inter, const int* lab, int C, int T,
                                                unsigned long long* areas, int tid) {
  for (int i = tid; i < T * 3 * C; i += 256) {
    const int t = i / (3 * C), k = (i % (3 * C)) / C, c = i % C;
    int v = 0;
    if (k == 2) {
      v = lab[c];
    } else {
      const int* b = k ? pre : inter;
      if (c) for (int s = t + 1; s <= T; ++s) v += b[s * C + c];
      else for (int s = 0; s <= t; ++s) v += b[s * C];
    }
    if (v) atomicAdd(&areas[i], (unsigned long long)v);
  }
}

// The tile, descriptor tables and range checks of seg_rescaled_kernel.  Dynamic LDS: A.tab_floats floats of table copies, four
// taps x A.cover_slots x 256 covering-window entries, then the counters (2 * (T + 1) + 1) * C.
__global__ __launch_bounds__(256) void seg_sweep_kernel(SegSweepArgs S) {
  const SegEvalArgs& A = S.e;
  __shared__ int s_wy[SEG_MAX_IMG_WIN], s_wx[SEG_MAX_IMG_WIN], s_wi[SEG_MAX_IMG_WIN], s_row[SEG_MAX_IMG_WIN];
  __shared__ int s_n, s_img;
  __shared__ uint8_t s_sw[SEG_MAX_IMG_WIN * SEG_MAX_G];   // first threshold index whose indicator is on, or T
  __shared__ uint8_t s_fl[SEG_MAX_IMG_WIN * SEG_MAX_G];   // the single-window foreground label
  extern __shared__ float s_dyn[];
  const int slots = A.cover_slots;
  const int T = S.T, C = A.N + 1;
  float* s_tab = s_dyn;
  uint16_t* s_cov = reinterpret_cast<uint16_t*>(s_dyn + A.tab_floats);
  int* s_pre = reinterpret_cast<int*>(s_cov + 4 * slots * 256);
  int* s_int = s_pre + (T + 1) * C;
  int* s_cl = s_int + (T + 1) * C;

  const int tid = threadIdx.x;
  if (tid == 0) {  // the last image whose first workgroup is not after this one
    int lo = 0, hi = A.B - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (A.images[(int64_t)mid * SEG_IMG_COLS + SI_BLK] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_img = lo;
  }
  for (int i = tid; i < (2 * (T + 1) + 1) * C; i += 256) s_pre[i] = 0;
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
  for (int i = tid; i < nwin * A.G; i += 256) {
    const int k = i / A.G, g = i % A.G;
    const int64_t wg = (int64_t)s_wi[k] * A.G + g;
    const float sc = A.best_score[wg], tmax = A.table_max[s_wi[k]];
    int sw = T;   // the indicator of seg_rescaled_kernel at bg_thresh = thr[t]; constant indices: thr stays in the kernel arguments
#pragma unroll
    for (int t = SEG_SWEEP_MAX_T - 1; t >= 0; --t)
      if (t < T && sc < fminf(S.thr[t], tmax)) sw = t;
    s_sw[k * SEG_MAX_G + g] = (uint8_t)sw;
    s_fl[k * SEG_MAX_G + g] = (uint8_t)(sc > 0.f ? A.best_class[wg] + 1 : 0);
  }
  const bool staged = (int64_t)nwin * A.G * A.N <= A.tab_floats;
  if (staged) {
    const int per = A.G * A.N;
    for (int i = tid; i < nwin * per; i += 256) s_tab[i] = A.table[(int64_t)s_wi[i / per] * per + i % per];
  }
  for (int k = tid; k < nwin; k += 256) s_row[k] = staged ? k : s_wi[k];
  __syncthreads();

  SegBlockWindows bw = {s_wy, s_wx, s_wi, nwin};
  SegTables tb = {staged ? (const float*)s_tab : A.table, s_row, s_sw, A.G, A.N, 1};   // classes >= 1 only: bg is not read
  const float sy = (float)gh / (float)win_h, sx = (float)gw / (float)win_w;
  const float* soft = A.soft + (soft_off - first * A.G * gh * gw);
  uint16_t* const c0 = s_cov;
  uint16_t* const b1 = s_cov + slots * 256;
  uint16_t* const b2 = s_cov + 2 * slots * 256;
  uint16_t* const b3 = s_cov + 3 * slots * 256;

  const int64_t pq = p0 + (int64_t)tid * SEG_EVAL_PPL;
  uint32_t fpack = 0, spack = 0;
  int run_f = -1, run_s = -1, run_g = -1, run_n = 0;  // equal (label, switch, ground truth) triples of the lane's pixels are counted once
  for (int q = 0; q < SEG_EVAL_PPL; ++q) {
    const int64_t p = pq + q;
    if (p >= total) break;
    const int y = (int)((uint32_t)p / (uint32_t)ow), x = (int)((uint32_t)p % (uint32_t)ow);
    int ya, yb, xa, xb;
    float ly, lx;
    seg_axis_taps(y, ry, (int)H, ya, yb, ly);
    seg_axis_taps(x, rx, (int)W, xa, xb, lx);
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
    // f: the first maximum over the classes >= 1; s: the first threshold index at which class 0, which comes first and so wins
    // ties, is not below it (the strict > scan of seg_rescaled_kernel)
    int f = 0, s = 0;
    if (seg_same_cover(c0, n0, c1, n1, tid) && seg_same_cover(c0, n0, c2, n2, tid) && seg_same_cover(c0, n0, c3, n3, tid)) {
      if (n0 == 1) {
        const int e = c0[tid];
        f = s_fl[(e >> 8) * SEG_MAX_G + (e & 255)];
        s = s_sw[(e >> 8) * SEG_MAX_G + (e & 255)];
      } else if (n0 > 1) {
        float best = -INFINITY;
        for (int c = 1; c < C; ++c) {
          const float v = seg_class_logit(tb, c, n0, c0, tid);
          if (v > best) { best = v; f = c; }
        }
        while (s < T && best > seg_sweep_bg_logit(s_sw, s, n0, c0, tid)) ++s;
      }
    } else {
      const float hy = 1.f - ly, hx = 1.f - lx;
      float best = -INFINITY;
      for (int c = 1; c < C; ++c) {
        const float v00 = n0 ? seg_class_logit(tb, c, n0, c0, tid) : 0.f;
        const float v01 = c1 == c0 ? v00 : (n1 ? seg_class_logit(tb, c, n1, c1, tid) : 0.f);
        const float v10 = c2 == c0 ? v00 : (n2 ? seg_class_logit(tb, c, n2, c2, tid) : 0.f);
        const float v11 = c3 == c1 ? v01 : (c3 == c2 ? v10 : (n3 ? seg_class_logit(tb, c, n3, c3, tid) : 0.f));
        const float v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
        if (v > best) { best = v; f = c; }
      }
      for (; s < T; ++s) {
        const float v00 = n0 ? seg_sweep_bg_logit(s_sw, s, n0, c0, tid) : 0.f;
        const float v01 = c1 == c0 ? v00 : (n1 ? seg_sweep_bg_logit(s_sw, s, n1, c1, tid) : 0.f);
        const float v10 = c2 == c0 ? v00 : (n2 ? seg_sweep_bg_logit(s_sw, s, n2, c2, tid) : 0.f);
        const float v11 = c3 == c1 ? v01 : (c3 == c2 ? v10 : (n3 ? seg_sweep_bg_logit(s_sw, s, n3, c3, tid) : 0.f));
        const float v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
        if (!(best > v)) break;
      }
    }
    if (f == 0) s = 0;   // background at every threshold: one canonical pair
    if (s == 0) f = 0;
    fpack |= (uint32_t)(f & 255) << (8 * q);
    spack |= (uint32_t)s << (8 * q);
    if (score) {
      const int g = A.gt[gt_off + p];
      if (f == run_f && s == run_s && g == run_g) {
        ++run_n;
      } else {
        if (run_n) seg_sweep_area_add(s_pre, s_int, s_cl, C, T, run_f, run_s, run_g, A.ignore_index, A.reduce_zero, run_n);
        run_f = f; run_s = s; run_g = g; run_n = 1;
      }
    }
  }
  if (run_n) seg_sweep_area_add(s_pre, s_int, s_cl, C, T, run_f, run_s, run_g, A.ignore_index, A.reduce_zero, run_n);
  if (write && pq < total) {
    for (int t = 0; t < T; ++t) {
      uint32_t pack = 0;
      for (int q = 0; q < SEG_EVAL_PPL; ++q)
        if (t < (int)((spack >> (8 * q)) & 255u)) pack |= fpack & (255u << (8 * q));
      uint8_t* o = A.labels + (int64_t)t * A.labels_bytes + lab_off + pq;
      if (pq + SEG_EVAL_PPL <= total && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(o) = pack;
      } else {
        for (int q = 0; q < SEG_EVAL_PPL && pq + q < total; ++q) o[q] = (uint8_t)(pack >> (8 * q));
      }
    }
  }
  if (score) {
    __syncthreads();
    seg_sweep_flush(s_pre, s_int, s_cl, C, T, A.areas, tid);
  }
}
