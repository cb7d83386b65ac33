// Zero-shot segmentation evaluation (segment.hip): label maps at the ground truth's size for images of mixed sizes, and the
// per-class areas of the mIoU (mmseg's resize(size=ori_shape) -> arg-max -> intersect_and_union), without a (C, oh, ow) or
// (C, H, W) tensor: every output pixel blends the class logits of its four source pixels, which are formed by the device
// functions of segment_pixel.inc exactly as segclip_seg_logits writes them.  The tile, the descriptor table and its range
// checks, the taps and the blend are those of segment_tile.inc.

#define SEG_EVAL_TAB_FLOATS 4096
#define SEG_MAX_CLASSES 256

// segclip_seg_areas and segclip_seg_areas_wide: T the label element, MAX_CLASSES the counters of the workgroup
template <typename T, int MAX_CLASSES>
__device__ __forceinline__ void seg_areas_body(const T* __restrict__ pred, const T* __restrict__ gt, int64_t n, int C, int ignore_index,
                                               int reduce_zero, unsigned long long* areas) {
  __shared__ int s_cnt[3 * MAX_CLASSES];
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * C; i += 256) s_cnt[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256)
    seg_area_add(s_cnt, C, pred[i], gt[i], ignore_index, reduce_zero, 1);
  __syncthreads();
  seg_area_flush(s_cnt, C, areas, tid);
}

__global__ __launch_bounds__(256) void seg_areas_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t n,
                                                        int C, int ignore_index, int reduce_zero, unsigned long long* areas) {
  seg_areas_body<uint8_t, SEG_MAX_CLASSES>(pred, gt, n, C, ignore_index, reduce_zero, areas);
}

// A workgroup owns SEG_EVAL_TILE consecutive pixels of one image's flat (oh, ow) output, a lane four of them (one dword store:
// the host aligns every image's label offset to 4).  seg_tile_load range-checks the image's table row.
__global__ __launch_bounds__(256) void seg_rescaled_kernel(SegEvalArgs A) {
  __shared__ int s_wy[SEG_MAX_IMG_WIN], s_wx[SEG_MAX_IMG_WIN], s_wi[SEG_MAX_IMG_WIN], s_row[SEG_MAX_IMG_WIN];
  const SegWinLists L = {s_wy, s_wx, s_wi, s_row};
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
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_IMG_COLS, SI_BLK, (int64_t)blockIdx.x);
  for (int i = tid; i < 3 * C; i += 256) s_cnt[i] = 0;
  __syncthreads();

  const SegTile T = seg_tile_load(A, s_img);
  const int64_t total = T.total;
  const bool write = A.labels && T.lab_off >= 0 && T.lab_off + total <= A.labels_bytes;
  const bool score = A.gt && A.areas && T.gt_off >= 0 && T.gt_off + total <= A.gt_bytes;
  if (T.p0 < 0 || T.p0 >= total || !(write || score)) return;  // block-uniform, and nothing was counted

  const int nwin = seg_tile_windows(A.windows, T, L, &s_n, tid);
  seg_window_labels(A.best_score, A.table_max, A.best_class, A.with_bg, A.bg_thresh, A.G, L, nwin, s_bg, s_lab, tid);
  const bool staged = seg_stage_tables(A.table, A.G, A.N, L, nwin, s_tab, A.tab_floats, tid);
  __syncthreads();

  SegBlockWindows bw = {s_wy, s_wx, s_wi, nwin};
  SegTables tb = {staged ? (const float*)s_tab : A.table, s_row, s_bg, A.G, A.N, off};
  const SegScales sc = seg_row_scales(T, T.oh, T.ow);
  const float* soft = A.soft + T.soft;

  const int64_t pq = T.p0 + (int64_t)tid * SEG_EVAL_PPL;
  uint32_t pack = 0;
  SegAreaRun run = {s_cnt, C, A.ignore_index, A.reduce_zero};
  for (int q = 0; q < SEG_EVAL_PPL; ++q) {
    const int64_t p = pq + q;
    if (p >= total) break;
    const int y = (int)((uint32_t)p / (uint32_t)T.ow), x = (int)((uint32_t)p % (uint32_t)T.ow);
    const SegTaps t = seg_pixel_taps(bw, soft, T, sc, A.G, y, x, s_cov, A.cover_slots, tid);
    const bool same = seg_taps_same(t, tid);
    int lab = 0;
    if (same && t.n0 == 1) {  // one covering window: the label staged per (window, group)
      const int e = t.c0[tid];
      lab = s_lab[(e >> 8) * SEG_MAX_G + (e & 255)];
    } else if (!same || t.n0 > 1) {
      float best = -INFINITY;
      for (int c = 0; c < C; ++c) {
        const float v = seg_blend_logit(tb, c, t, same, tid);
        if (v > best) { best = v; lab = c; }
      }
    }
    pack |= (uint32_t)(lab & 255) << (8 * q);
    if (score) run.add(lab, A.gt[T.gt_off + p]);
  }
  run.flush();
  if (write && pq < total) seg_store_labels4(A.labels + T.lab_off + pq, pack, total - pq);
  if (score) {
    __syncthreads();
    seg_area_flush(s_cnt, C, A.areas, tid);
  }
}
