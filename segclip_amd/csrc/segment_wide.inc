// 16-bit label maps (segment.hip): segclip_seg_label_map_rescaled and segclip_seg_areas for vocabularies of up to 1024 classes
// (Pascal-Context-459, ADE20K-847: 460 and 848 classes with the background).  The definition of a label, the ground-truth rule,
// the tile, the descriptor table and the range checks (seg_tile_load) are those of segment_tile.inc; what differs:
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

#define SEG_WIDE_MAX_CLASSES SEGCLIP_SEG_WIDE_MAX_CLASSES
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

__global__ __launch_bounds__(256) void seg_areas_wide_kernel(const uint16_t* __restrict__ pred, const uint16_t* __restrict__ gt,
                                                             int64_t n, int C, int ignore_index, int reduce_zero,
                                                             unsigned long long* areas) {
  seg_areas_body<uint16_t, SEG_WIDE_MAX_CLASSES>(pred, gt, n, C, ignore_index, reduce_zero, areas);
}

// The tile and the row check of seg_tile_load, as seg_rescaled_kernel.  No lane leaves the pixel loop early: the lanes of a wave
// meet at the ballot of every one of their four pixels.
__global__ __launch_bounds__(256) void seg_rescaled_wide_kernel(SegWideArgs S) {
  const SegEvalArgs& A = S.e;
  __shared__ int s_wy[SEG_MAX_IMG_WIN], s_wx[SEG_MAX_IMG_WIN], s_wi[SEG_MAX_IMG_WIN], s_row[SEG_MAX_IMG_WIN];
  const SegWinLists L = {s_wy, s_wx, s_wi, s_row};
  __shared__ int s_n, s_img;
  __shared__ uint8_t s_bg[SEG_MAX_IMG_WIN * SEG_MAX_G];
  __shared__ uint16_t s_lab[SEG_MAX_IMG_WIN * SEG_MAX_G];   // the label of class N is N with the background
  __shared__ int s_cnt[3 * SEG_WIDE_MAX_CLASSES];
  // dynamic LDS: A.tab_floats floats of table copies, then four taps x A.cover_slots x 256 covering-window entries
  extern __shared__ float s_dyn[];
  float* s_tab = s_dyn;
  uint16_t* s_cov = reinterpret_cast<uint16_t*>(s_dyn + A.tab_floats);

  const int tid = threadIdx.x;
  const int off = A.with_bg ? 1 : 0;
  const int C = A.N + off;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_IMG_COLS, SI_BLK, (int64_t)blockIdx.x);
  for (int i = tid; i < 3 * C; i += 256) s_cnt[i] = 0;
  __syncthreads();

  const SegTile T = seg_tile_load(A, s_img);
  const int64_t total = T.total;
  const bool write = S.labels && T.lab_off >= 0 && T.lab_off + total <= A.labels_bytes;
  const bool score = S.gt && A.areas && T.gt_off >= 0 && T.gt_off + total <= A.gt_bytes;
  if (T.p0 < 0 || T.p0 >= total || !(write || score)) return;  // block-uniform, and nothing was counted

  const int nwin = seg_tile_windows(A.windows, T, L, &s_n, tid);
  seg_window_labels(A.best_score, A.table_max, A.best_class, A.with_bg, A.bg_thresh, A.G, L, nwin, s_bg, s_lab, tid);
  const bool staged = seg_stage_tables(A.table, A.G, A.N, L, nwin, s_tab, A.tab_floats, tid);
  __syncthreads();

  SegBlockWindows bw = {s_wy, s_wx, s_wi, nwin};
  SegTables tb = {staged ? (const float*)s_tab : A.table, s_row, s_bg, A.G, A.N, off};
  const SegScales sc = seg_row_scales(T, T.oh, T.ow);
  const float* soft = A.soft + T.soft;
  const int slots = A.cover_slots;
  uint16_t* const c0 = s_cov;   // the four cover lists of seg_pixel_taps
  uint16_t* const b1 = s_cov + slots * 256;
  uint16_t* const b2 = s_cov + 2 * slots * 256;

  const int64_t pq = T.p0 + (int64_t)tid * SEG_EVAL_PPL;
  const bool lane_scan = SEG_WIDE_LANE_SCAN || C <= SEG_WIDE_LANE_SCAN_CLASSES;
  unsigned long long pack = 0, todo;
  SegAreaRun run = {s_cnt, C, A.ignore_index, A.reduce_zero};
  for (int q = 0; q < SEG_EVAL_PPL; ++q) {
    const int64_t p = pq + q;
    const bool valid = p < total;
    SegTaps t = {c0, c0, c0, c0, 0, 0, 0, 0, 0.f, 0.f};
    bool same = true;
    if (valid) {
      const int y = (int)((uint32_t)p / (uint32_t)T.ow), x = (int)((uint32_t)p % (uint32_t)T.ow);
      t = seg_pixel_taps(bw, soft, T, sc, A.G, y, x, s_cov, slots, tid);
      same = seg_taps_same(t, tid);
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
    if (valid && score) run.add(lab, S.gt[T.gt_off + p]);
  }
  run.flush();
  if (write && pq < total) seg_store_labels4(S.labels + T.lab_off + pq, pack, total - pq);
  if (score) {
    __syncthreads();
    seg_area_flush(s_cnt, C, A.areas, tid);
  }
}
