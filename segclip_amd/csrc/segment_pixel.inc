// Per-pixel device functions of the zero-shot segmentation kernels (segment.hip): shared by segclip_seg_label_map and
// segclip_seg_logits so that the label map is, by construction, the first maximum of the dense logits.

// One axis of F.interpolate(mode="bilinear", align_corners=False): destination index d of an axis resampled from n source
// samples with scale = n / n_dst.  Source coordinate scale * (d + 0.5) - 0.5 clamped below at 0; the second tap stays on the
// last sample at the edge (ATen upsample_bilinear2d: area_pixel_compute_source_index + the `< n - 1` step).
__device__ __forceinline__ void seg_axis_taps(int d, float scale, int n, int& i0, int& i1, float& lambda) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i0 = i0 > n - 1 ? n - 1 : i0;
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  lambda = s - (float)i0;
}

// Group of one output pixel inside one window: the G channels of `a` (G, gh * gw) interpolated at the four taps in ATen's
// operation order, first maximum over G (torch.argmax; the AssignFn convention of center.hip).
__device__ __forceinline__ int seg_pixel_group(const float* __restrict__ a, int G, int plane, int o00, int o01, int o10, int o11,
                                               float ly, float lx) {
  const float hy = 1.f - ly, hx = 1.f - lx;
  float best = -INFINITY;
  int arg = 0;
  for (int g = 0; g < G; ++g) {
    const float* p = a + (int64_t)g * plane;
    const float v = hy * (hx * p[o00] + lx * p[o01]) + ly * (hx * p[o10] + lx * p[o11]);
    if (v > best) { best = v; arg = g; }
  }
  return arg;
}

// The covering windows of one pixel, in window order, as (local window << 8 | group) entries of cov[slot * 256 + tid].
// Returns their number (at most `slots` <= SEG_MAX_COVER are kept).
struct SegBlockWindows {
  const int* wy;     // LDS: y0 of the block's windows
  const int* wx;     // LDS: x0
  const int* wi;     // LDS: index into the window list (= row of soft_attn and of the tables)
  int n;
};
__device__ __forceinline__ int seg_pixel_cover(const SegBlockWindows& bw, const float* __restrict__ soft, int y, int x, int win_h,
                                               int win_w, int gh, int gw, int G, float sy, float sx, uint16_t* cov, int slots, int tid) {
  int cnt = 0;
  const int plane = gh * gw;
  for (int k = 0; k < bw.n; ++k) {
    const int dy = y - bw.wy[k], dx = x - bw.wx[k];
    if (dy < 0 || dy >= win_h || dx < 0 || dx >= win_w) continue;
    int y0, y1, x0, x1;
    float ly, lx;
    seg_axis_taps(dy, sy, gh, y0, y1, ly);
    seg_axis_taps(dx, sx, gw, x0, x1, lx);
    const int g = seg_pixel_group(soft + (int64_t)bw.wi[k] * G * plane, G, plane, y0 * gw + x0, y0 * gw + x1, y1 * gw + x0,
                                  y1 * gw + x1, ly, lx);
    if (cnt < slots) cov[cnt * 256 + tid] = (uint16_t)((k << 8) | g);
    ++cnt;
  }
  return cnt < slots ? cnt : slots;
}

// Logit of class c at a pixel with cnt >= 1 covering windows: the windows' table rows (class 0 with background: their
// background indicators) summed in window order, divided by the window count (mmseg slide_inference: preds / count_mat).
struct SegTables {
  const float* tab;      // (windows, G, N): LDS copy of the block's windows, or the global table
  const int* row_win;    // LDS: local window -> window index of `tab` (identity for the LDS copy)
  const uint8_t* bg;     // LDS: [local window * SEG_MAX_G + g] background indicator
  int G, N, off;
};
__device__ __forceinline__ float seg_class_logit(const SegTables& t, int c, int cnt, const uint16_t* cov, int tid) {
  float s = 0.f;
  for (int j = 0; j < cnt; ++j) {
    const int e = cov[j * 256 + tid], k = e >> 8, g = e & 255;
    s += c < t.off ? (t.bg[k * SEG_MAX_G + g] ? 1.f : 0.f) : t.tab[((int64_t)t.row_win[k] * t.G + g) * t.N + (c - t.off)];
  }
  return s / (float)cnt;
}
