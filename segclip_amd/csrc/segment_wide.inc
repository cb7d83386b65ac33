// 16-bit label maps (segment.hip): segclip_seg_label_map_rescaled and segclip_seg_areas for vocabularies of up to 1024 classes
// (Pascal-Context-459, ADE20K-847: 460 and 848 classes with the background).  The definition of a label, the ground-truth rule,
// the tile, the descriptor table and the range checks are those of seg_rescaled_kernel (segment_eval.inc); what differs:
//   - labels and ground truths are uint16, a lane's four labels one 8-byte store;
//   - the counters are 3 x 1024 int32 (12 KiB static);
//   - an undecided pixel (taps that disagree, or several covering windows) is resolved by its WAVE: lane l evaluates the classes
//     l, l + 64, ... by the per-class expression of the narrow kernel, so a table row is read as consecutive floats by
//     consecutive lanes (the narrow kernel's lane walks all classes itself, 4 bytes at a time from rows that differ from lane to
//     lane: up to windows x G rows of 3.4 KB at 847 classes, which do not fit the table copy), and a shuffle reduction takes the
//     maximum, among equal values the lowest class: the first maximum of the scalar scan.  (Up to 32 classes every lane scans
//     its own pixel as in the narrow kernel: there the cooperative pass costs more than it saves.)
// LDS: 14.5 KiB static (window lists 1 KiB, indicators 0.5 KiB, single-window labels 1 KiB, counters 12 KiB) + at most 16 KiB of
// table copies + 32 KiB of cover lists = 62.5 KiB, inside the 64 KiB a kernel gets without asking.  Where one window's G x N
// table alone exceeds the copy (G * N > 4096) nothing can ever be staged and the launch asks for no copy: 46.5 KiB, three
// workgroups per CU as the narrow kernel.

#define SEG_WIDE_MAX_CLASSES 1024
// build-time switch of tools/bench_seg.py --wide: 1 = every lane scans the classes of its own undecided pixels (the narrow
// kernel's scheme) instead of the wave-cooperative scan
#ifndef SEG_WIDE_LANE_SCAN
#define SEG_WIDE_LANE_SCAN 0
#endif
// At most this many classes: the per-lane scan in every build.  Measured on 12.0 M output pixels (profiles/seg_wide.txt): the
// per-lane scan takes 2.5 ms at 21 classes and 20.2 ms at 151, about 0.14 ms per class; the cooperative scan 4.2 ms and 10.0 ms,
// about 1.3 ms + 2.9 ms per 64 classes; the two lines meet near 33 classes.
// (0 at build time: the cooperative scan at every class count, the tool's other switch.)
#ifndef SEG_WIDE_LANE_SCAN_CLASSES
#define SEG_WIDE_LANE_SCAN_CLASSES 32
#endif

struct SegWideArgs {
  SegEvalArgs e;        // e.labels / e.gt stay null; e.labels_bytes and e.gt_bytes count ELEMENTS here
  uint16_t* labels;     // flat, or null
  const uint16_t* gt;   // flat, or null
};

// The four taps of one output pixel: their covering-window lists (aliases of one another where two taps are one source pixel)
// and the weights of the second tap per axis.
struct SegTaps {
  const uint16_t *c0, *c1, *c2, *c3;
  int n0, n1, n2, n3;
  float ly, lx;
};

// The value of class c at an output pixel, bit for bit the per-class expression of seg_rescaled_kernel: the plain logit where the
// four taps have one logit vector (`same`), else the blend of the taps' logits.  col: the column of the cover lists, the
// thread that owns the pixel - every lane of a wave passes the same one in the cooperative scan (a same-address LDS read).
__device__ __forceinline__ float seg_blend_logit(const SegTables& tb, int c, const SegTaps& t, bool same, int col) {
  if (same) return seg_class_logit(tb, c, t.n0, t.c0, col);
  const float hy = 1.f - t.ly, hx = 1.f - t.lx;
  const float v00 = t.n0 ? seg_class_logit(tb, c, t.n0, t.c0, col) : 0.f;
  const float v01 = t.c1 == t.c0 ? v00 : (t.n1 ? seg_class_logit(tb, c, t.n1, t.c1, col) : 0.f);
  const float v10 = t.c2 == t.c0 ? v00 : (t.n2 ? seg_class_logit(tb, c, t.n2, t.c2, col) : 0.f);
  const float v11 = t.c3 == t.c1 ? v01 : (t.c3 == t.c2 ? v10 : (t.n3 ? seg_class_logit(tb, c, t.n3, t.c3, col) : 0.f));
  return hy * (hx * v00 + t.lx * v01) + t.ly * (hx * v10 + t.lx * v11);
}

__global__ __launch_bounds__(256) void seg_areas_wide_kernel(const uint16_t* __restrict__ pred, const uint16_t* __restrict__ gt,
                                                             int64_t n, int C, int ignore_index, int reduce_zero,
                                                             unsigned long long* areas) {
  __shared__ int s_cnt[3 * SEG_WIDE_MAX_CLASSES];
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * C; i += 256) s_cnt[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256)
    seg_area_add(s_cnt, C, pred[i], gt[i], ignore_index, reduce_zero, 1);
  __syncthreads();
  seg_area_flush(s_cnt, C, areas, tid);
}

// The tile, descriptor table and range checks of seg_rescaled_kernel.  No lane leaves the pixel loop early: the lanes of a wave
// meet at the ballot of every one of their four pixels.
__global__ __launch_bounds__(256) void seg_rescaled_wide_kernel(SegWideArgs S) {
  const SegEvalArgs& A = S.e;
  __shared__ int s_wy[SEG_MAX_IMG_WIN], s_wx[SEG_MAX_IMG_WIN], s_wi[SEG_MAX_IMG_WIN], s_row[SEG_MAX_IMG_WIN];
  __shared__ int s_n, s_img;
  __shared__ uint8_t s_bg[SEG_MAX_IMG_WIN * SEG_MAX_G];
  __shared__ uint16_t s_lab[SEG_MAX_IMG_WIN * SEG_MAX_G];
  __shared__ int s_cnt[3 * SEG_WIDE_MAX_CLASSES];
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
  const bool write = S.labels && lab_off >= 0 && lab_off + total <= A.labels_bytes;
  const bool score = S.gt && A.areas && gt_off >= 0 && gt_off + total <= A.gt_bytes;
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
  for (int i = tid; i < nwin * A.G; i += 256) {  // as in seg_pixel_kernel; the label of class N is N with the background
    const int k = i / A.G, g = i % A.G;
    const int64_t wg = (int64_t)s_wi[k] * A.G + g;
    const float sc = A.best_score[wg];
    const bool bg = A.with_bg && sc < fminf(A.bg_thresh, A.table_max[s_wi[k]]);
    s_bg[k * SEG_MAX_G + g] = bg ? 1 : 0;
    s_lab[k * SEG_MAX_G + g] = (uint16_t)(A.with_bg ? ((bg || !(sc > 0.f)) ? 0 : A.best_class[wg] + 1) : A.best_class[wg]);
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
  const bool lane_scan = SEG_WIDE_LANE_SCAN || C <= SEG_WIDE_LANE_SCAN_CLASSES;
  unsigned long long pack = 0, todo;
  int run_p = -1, run_g = -1, run_n = 0;  // equal (prediction, ground truth) pairs of the lane's pixels are counted once
  for (int q = 0; q < SEG_EVAL_PPL; ++q) {
    const int64_t p = pq + q;
    const bool valid = p < total;
    SegTaps t = {c0, c0, c0, c0, 0, 0, 0, 0, 0.f, 0.f};
    bool same = true;
    if (valid) {
      const int y = (int)((uint32_t)p / (uint32_t)ow), x = (int)((uint32_t)p % (uint32_t)ow);
      int ya, yb, xa, xb;
      seg_axis_taps(y, ry, (int)H, ya, yb, t.ly);
      seg_axis_taps(x, rx, (int)W, xa, xb, t.lx);
      // a tap of weight 0 adds 0 * (a finite logit): it may be any pixel, so take the one already resolved
      if (t.ly == 0.f) yb = ya;
      if (t.lx == 0.f) xb = xa;
#define SEG_COVER(yy, xx, buf) seg_pixel_cover(bw, soft, yy, xx, (int)win_h, (int)win_w, (int)gh, (int)gw, A.G, sy, sx, buf, slots, tid)
      t.n0 = SEG_COVER(ya, xa, c0);
      t.n1 = t.n2 = t.n0;
      if (xb != xa) { t.n1 = SEG_COVER(ya, xb, b1); t.c1 = b1; }
      if (yb != ya) { t.n2 = SEG_COVER(yb, xa, b2); t.c2 = b2; }
      if (yb == ya) { t.c3 = t.c1; t.n3 = t.n1; }
      else if (xb == xa) { t.c3 = t.c2; t.n3 = t.n2; }
      else { t.n3 = SEG_COVER(yb, xb, b3); t.c3 = b3; }
#undef SEG_COVER
      same = seg_same_cover(t.c0, t.n0, t.c1, t.n1, tid) && seg_same_cover(t.c0, t.n0, t.c2, t.n2, tid) &&
             seg_same_cover(t.c0, t.n0, t.c3, t.n3, tid);
    }
    int lab = 0;
    // the four source pixels have one logit vector v, and the blend is monotone in v: its first maximum is v's; one covering
    // window: the label staged per (window, group)
    if (valid && same && t.n0 == 1) {
      const int e = c0[tid];
      lab = s_lab[(e >> 8) * SEG_MAX_G + (e & 255)];
    }
    const bool undecided = valid && (!same || t.n0 > 1);
    // few classes: every lane scans the classes of its own pixel, as the narrow kernel does (the lanes of a wave work side by
    // side, and a cooperative pass would leave most of its 64 lanes without a class)
    if (lane_scan) {  // block-uniform
      if (undecided) {
        float best = -INFINITY;
        for (int c = 0; c < C; ++c) {
          const float v = seg_blend_logit(tb, c, t, same, tid);
          if (v > best) { best = v; lab = c; }
        }
      }
      todo = 0;
    } else {
      todo = __ballot(undecided);
    }
    // the wave resolves its undecided pixels together, one after the other: the owner's taps are broadcast, its cover lists are
    // read from its column, lane l takes the classes l, l + 64, ...
    if (todo) {  // wave-uniform
      const int lane = tid & 63;
      // which list a tap aliases travels as its index (0 = c0, 1 = b1, 2 = b2, 3 = b3) beside the four counts
      const int i1 = t.c1 == c0 ? 0 : 1, i2 = t.c2 == c0 ? 0 : 2, i3 = t.c3 == c0 ? 0 : (t.c3 == b1 ? 1 : (t.c3 == b2 ? 2 : 3));
      const int state = t.n0 | (t.n1 << 5) | (t.n2 << 10) | (t.n3 << 15) | (i1 << 20) | (i2 << 22) | (i3 << 24) | ((same ? 1 : 0) << 26);
      // the owners' cover lists are read by the other lanes of their wave
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int st = __shfl(state, owner, 64);
        SegTaps o;
        o.ly = __shfl(t.ly, owner, 64);
        o.lx = __shfl(t.lx, owner, 64);
        o.n0 = st & 31; o.n1 = (st >> 5) & 31; o.n2 = (st >> 10) & 31; o.n3 = (st >> 15) & 31;
        o.c0 = c0;
        o.c1 = s_cov + ((st >> 20) & 3) * slots * 256;
        o.c2 = s_cov + ((st >> 22) & 3) * slots * 256;
        o.c3 = s_cov + ((st >> 24) & 3) * slots * 256;
        const bool o_same = (st >> 26) & 1;
        const int col = (tid & ~63) | owner;
        float best = -INFINITY;
        int arg = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
          const float v = seg_blend_logit(tb, c, o, o_same, col);
          if (v > best) { best = v; arg = c; }
        }
        wave_argmax_first(best, arg);
        if (lane == owner) lab = arg < C ? arg : 0;  // no class above -inf: 0, as the scalar scan leaves it
      }
      __builtin_amdgcn_wave_barrier();  // the next pixel's lists overwrite these
    }
    pack |= (unsigned long long)(lab & 0xffff) << (16 * q);
    if (valid && score) {
      const int g = S.gt[gt_off + p];
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
    uint16_t* o = S.labels + lab_off + pq;
    if (pq + SEG_EVAL_PPL <= total && (reinterpret_cast<uintptr_t>(o) & 7) == 0) {
      *reinterpret_cast<unsigned long long*>(o) = pack;
    } else {
      for (int q = 0; q < SEG_EVAL_PPL && pq + q < total; ++q) o[q] = (uint16_t)(pack >> (16 * q));
    }
  }
  if (score) {
    __syncthreads();
    seg_area_flush(s_cnt, C, A.areas, tid);
  }
}
