// Background-threshold sweep (segment.hip): the label maps and mIoU areas of segclip_seg_label_map_rescaled for T ascending
// values of bg_thresh in ONE launch.  The threshold enters a pixel's logits through the background indicators of its covering
// (window, group) pairs alone, and over ascending thresholds an indicator can only switch on.  The class-0 logit is a monotone
// fp32 function of the indicators (weights >= 0; fp32 multiply, add and fma are monotone), the other classes do not see the
// threshold: a pixel has ONE foreground label f (its first maximum over the classes >= 1) and ONE switch index s, and its label
// is f for the thresholds t < s and 0 for t >= s.  Covers, taps and the foreground scan run once per pixel, by the device
// functions of segment_pixel.inc / segment_tile.inc; only the class-0 logit is evaluated per threshold, until it wins.

#define SEG_SWEEP_MAX_T SEGCLIP_SEG_MAX_THRESHOLDS
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

// The tile and the row check of seg_tile_load, as seg_rescaled_kernel.  Dynamic LDS: A.tab_floats floats of table copies, four
// taps x A.cover_slots x 256 covering-window entries, then the counters (2 * (T + 1) + 1) * C.
__global__ __launch_bounds__(256) void seg_sweep_kernel(SegSweepArgs S) {
  const SegEvalArgs& A = S.e;
  __shared__ int s_wy[SEG_MAX_IMG_WIN], s_wx[SEG_MAX_IMG_WIN], s_wi[SEG_MAX_IMG_WIN], s_row[SEG_MAX_IMG_WIN];
  const SegWinLists L = {s_wy, s_wx, s_wi, s_row};
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
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_IMG_COLS, SI_BLK, (int64_t)blockIdx.x);
  for (int i = tid; i < (2 * (T + 1) + 1) * C; i += 256) s_pre[i] = 0;
  __syncthreads();

  const SegTile R = seg_tile_load(A, s_img);
  const int64_t total = R.total;
  const bool write = A.labels && R.lab_off >= 0 && R.lab_off + total <= A.labels_bytes;
  const bool score = A.gt && A.areas && R.gt_off >= 0 && R.gt_off + total <= A.gt_bytes;
  if (R.p0 < 0 || R.p0 >= total || !(write || score)) return;  // block-uniform, and nothing was counted

  const int nwin = seg_tile_windows(A.windows, R, L, &s_n, tid);
  for (int i = tid; i < nwin * A.G; i += 256) {
    const int k = i / A.G, g = i % A.G;
    const int64_t wg = (int64_t)s_wi[k] * A.G + g;
    const float sc = A.best_score[wg], tmax = A.table_max[s_wi[k]];
    int sw = T;   // the indicator of seg_window_labels at bg_thresh = thr[t]; constant indices: thr stays in the kernel arguments
#pragma unroll
    for (int t = SEG_SWEEP_MAX_T - 1; t >= 0; --t)
      if (t < T && sc < fminf(S.thr[t], tmax)) sw = t;
    s_sw[k * SEG_MAX_G + g] = (uint8_t)sw;
    s_fl[k * SEG_MAX_G + g] = (uint8_t)(sc > 0.f ? A.best_class[wg] + 1 : 0);
  }
  const bool staged = seg_stage_tables(A.table, A.G, A.N, L, nwin, s_tab, A.tab_floats, tid);
  __syncthreads();

  SegBlockWindows bw = {s_wy, s_wx, s_wi, nwin};
  SegTables tb = {staged ? (const float*)s_tab : A.table, s_row, s_sw, A.G, A.N, 1};   // classes >= 1 only: bg is not read
  const SegScales sc = seg_row_scales(R, R.oh, R.ow);
  const float* soft = A.soft + R.soft;

  const int64_t pq = R.p0 + (int64_t)tid * SEG_EVAL_PPL;
  uint32_t fpack = 0, spack = 0;
  int run_f = -1, run_s = -1, run_g = -1, run_n = 0;  // equal (label, switch, ground truth) triples of the lane's pixels are counted once
  for (int q = 0; q < SEG_EVAL_PPL; ++q) {
    const int64_t p = pq + q;
    if (p >= total) break;
    const int y = (int)((uint32_t)p / (uint32_t)R.ow), x = (int)((uint32_t)p % (uint32_t)R.ow);
    const SegTaps t = seg_pixel_taps(bw, soft, R, sc, A.G, y, x, s_cov, slots, tid);
    const bool same = seg_taps_same(t, tid);
    // f: the first maximum over the classes >= 1; s: the first threshold index at which class 0, which comes first and so wins
    // ties, is not below it (the strict > scan of seg_rescaled_kernel)
    int f = 0, s = 0;
    if (same && t.n0 == 1) {
      const int e = t.c0[tid];
      f = s_fl[(e >> 8) * SEG_MAX_G + (e & 255)];
      s = s_sw[(e >> 8) * SEG_MAX_G + (e & 255)];
    } else if (!same || t.n0 > 1) {
      float best = -INFINITY;
      for (int c = 1; c < C; ++c) {
        const float v = seg_blend_logit(tb, c, t, same, tid);
        if (v > best) { best = v; f = c; }
      }
      const auto bg = [&](int n, const uint16_t* cov) { return seg_sweep_bg_logit(s_sw, s, n, cov, tid); };
      while (s < T && best > seg_blend_taps(t, same, bg)) ++s;
    }
    if (f == 0) s = 0;   // background at every threshold: one canonical pair
    if (s == 0) f = 0;
    fpack |= (uint32_t)(f & 255) << (8 * q);
    spack |= (uint32_t)s << (8 * q);
    if (score) {
      const int g = A.gt[R.gt_off + p];
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
      seg_store_labels4(A.labels + (int64_t)t * A.labels_bytes + R.lab_off + pq, pack, total - pq);
    }
  }
  if (score) {
    __syncthreads();
    seg_sweep_flush(s_pre, s_int, s_cl, C, T, A.areas, tid);
  }
}
