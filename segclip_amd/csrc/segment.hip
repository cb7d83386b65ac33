// Zero-shot segmentation inference: class prompts + the center stage's soft assignment -> label map
// (reference seg_segmentation/evaluation/vit_seg.py:202-256 [ViTSegInference.encode_decode], :30-58 [resize_attn_map], and
// mmseg's slide_inference for overlapping windows).  Forward only, all math fp32: the outputs are arg-maxima.
//
// Every pixel's class logits are row g(pixel) of a G x N table per window, so the eager (H, W, G) upsampling, (H, W, G)
// one-hot, (H, W, N) product and (N + 1, H, W) logit volume never have to exist: segclip_seg_group_table builds the tables
// (latency-bound: G * N dot products of 512 per window), segclip_seg_label_map interpolates G numbers per pixel, takes the
// first maximum and looks one row up (bound: 1-2 bytes of HBM writes per pixel).
// segment_tile.inc holds what the rescaled kernels share: the image table's row check (seg_tile_load), the block's window list,
// table copies and labels, the four taps and their blend, the area counters and the packed label store.
// The other .inc files hold the kernels built on these: evaluation at the ground truth's size with the mIoU areas (segment_eval.inc),
// the same for a list of background thresholds in one launch (segment_sweep.inc), test-time augmentation (segment_aug.inc), the
// uint8 front end (segment_frontend.inc), rendering (segment_render.inc), pixel-adaptive refinement of the label maps
// (segment_refine.inc), their connected components (segment_objects.inc), despeckling by merging (segment_sieve.inc), the training front end (train_frontend.inc),
// the 16-bit label maps of vocabularies of up to 1024 classes (segment_wide.inc), the confusion matrix of label maps
// (segment_confusion.inc) and their per-image areas (segment_image_areas.inc).
#include "common.h"

#include <atomic>

#define SEG_MAX_G SEGCLIP_SEG_MAX_GROUPS          // groups per window (the center stage has 8)
#define SEG_MAX_COVER 16     // windows covering one pixel
#define SEG_MAX_IMG_WIN SEGCLIP_SEG_MAX_IMAGE_WINDOWS   // windows per image
#define SEG_TAB_FLOATS 8192  // LDS budget of the block's table copies

namespace {

#include "segment_pixel.inc"
#include "segment_tile.inc"

__device__ __forceinline__ float seg_clip_scale(const float* ls) { return fminf(expf(*ls), 100.f); }

// lowest index wins among equal values
__device__ __forceinline__ void wave_argmax_first(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// ---------------------------------------------------------------- (a) group-class table, one workgroup per window
// LDS: rows (G + 1, C) normalised | logits (G + 1, N) | prob (N) | mask (N) | best (SEG_MAX_G)
__global__ __launch_bounds__(256) void seg_group_table_kernel(const float* __restrict__ group_tokens, int64_t gt_stride,
                                                              const float* __restrict__ pooled, int64_t pooled_stride,
                                                              const float* __restrict__ text, const float* __restrict__ logit_scale,
                                                              float* __restrict__ table, float* __restrict__ table_max,
                                                              int32_t* __restrict__ best_class, float* __restrict__ best_score,
                                                              uint8_t* __restrict__ topk_mask, int G, int N, int C, int topk) {
  extern __shared__ float sm[];
  float* rows = sm;
  float* logit = rows + (G + 1) * C;
  float* prob = logit + (G + 1) * N;
  int* mask = reinterpret_cast<int*>(prob + N);
  float* gbest = reinterpret_cast<float*>(mask + N);
  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // F.normalize(dim=-1): x / max(|x|, 1e-12)
  for (int r = wave; r <= G; r += 4) {
    const float* x = r < G ? group_tokens + w * gt_stride + (int64_t)r * C : pooled + w * pooled_stride;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(x[c], x[c], s);
    const float nrm = fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    for (int c = lane; c < C; c += 64) rows[r * C + c] = x[c] / nrm;
  }
  __syncthreads();

  const float sc = seg_clip_scale(logit_scale);
  for (int n = wave; n < N; n += 4) {
    const float* t = text + (int64_t)n * C;
    float acc[SEG_MAX_G + 1];
#pragma unroll
    for (int r = 0; r <= SEG_MAX_G; ++r) acc[r] = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float tv = t[c];
#pragma unroll
      for (int r = 0; r <= SEG_MAX_G; ++r)
        if (r <= G) acc[r] = fmaf(rows[r * C + c], tv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r <= SEG_MAX_G; ++r)
      if (r <= G) {
        const float d = wave_sum(acc[r]);
        if (lane == 0) logit[r * N + n] = d * sc;
      }
  }
  for (int n = tid; n < N; n += 256) mask[n] = 0;
  __syncthreads();

  // softmax of the pooled row, then its top-k (ties: lowest class index) - wave 0, the block keeps step at the barriers
  if (wave == 0) {
    const float* x = logit + G * N;
    float m = -INFINITY;
    for (int n = lane; n < N; n += 64) m = fmaxf(m, x[n]);
    m = wave_max(m);
    float s = 0.f;
    for (int n = lane; n < N; n += 64) s += expf(x[n] - m);
    s = wave_sum(s);
    for (int n = lane; n < N; n += 64) prob[n] = expf(x[n] - m) / s;
  }
  __syncthreads();
  for (int k = 0; k < topk; ++k) {
    if (wave == 0) {
      float v = -INFINITY;
      int i = 0x7fffffff;
      for (int n = lane; n < N; n += 64)
        if (!mask[n] && prob[n] > v) { v = prob[n]; i = n; }
      wave_argmax_first(v, i);
      if (lane == 0 && i < N) mask[i] = 1;
    }
    __syncthreads();
  }
  if (topk_mask)
    for (int n = tid; n < N; n += 256) topk_mask[w * N + n] = (uint8_t)mask[n];

  // per group: softmax over all classes x softmax over the kept classes
  for (int g = wave; g < G; g += 4) {
    const float* x = logit + g * N;
    float m1 = -INFINITY, m2 = -INFINITY;
    for (int n = lane; n < N; n += 64) {
      m1 = fmaxf(m1, x[n]);
      if (mask[n]) m2 = fmaxf(m2, x[n]);
    }
    m1 = wave_max(m1);
    m2 = wave_max(m2);
    float s1 = 0.f, s2 = 0.f;
    for (int n = lane; n < N; n += 64) {
      s1 += expf(x[n] - m1);
      if (mask[n]) s2 += expf(x[n] - m2);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int n = lane; n < N; n += 64) {
      const float pre = expf(x[n] - m1) / s1;
      const float v = mask[n] ? (expf(x[n] - m2) / s2) * pre : 0.f;
      table[(w * G + g) * N + n] = v;
      if (v > bv) { bv = v; bi = n; }
    }
    wave_argmax_first(bv, bi);
    if (lane == 0) {
      if (bi >= N) { bi = 0; bv = 0.f; }
      best_class[w * G + g] = bi;
      best_score[w * G + g] = bv;
      gbest[g] = bv;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float m = gbest[0];
    for (int g = 1; g < G; ++g) m = fmaxf(m, gbest[g]);
    table_max[w] = m;
  }
}

// ---------------------------------------------------------------- (b), (c) the pixel kernels
struct SegPixelArgs {
  const float* soft;         // (n_windows, G, gh * gw)
  const float* table;        // (n_windows, G, N)
  const float* table_max;    // (n_windows)
  const int32_t* best_class; // (n_windows, G)
  const float* best_score;   // (n_windows, G)
  const int32_t* windows;    // (n_windows, 3): image, y0, x0; the windows of an image are consecutive
  const int32_t* image_first;  // (B + 1): windows image_first[b] .. image_first[b + 1] - 1 belong to image b
  int n_windows, B, H, W, win_h, win_w, gh, gw, G, N, with_bg;
  int tab_floats, cover_slots;  // dynamic LDS layout (seg_lds)
  float bg_thresh;
  uint8_t* labels;  // (B, H, W) or null
  uint8_t* groups;  // (B, H, W) or null
  float* logits;    // (B, N + with_bg, H, W)   [LOGITS kernel]
};

// A lane owns PPL consecutive pixels of one row; the units of an image are numbered row by row, so with W a multiple of 4
// a wave of the label kernel stores 256 consecutive bytes (one dword per lane), and a wave of the logits kernel (PPL = 1)
// stores 64 consecutive floats per class.
template <int PPL, bool LOGITS>
__global__ __launch_bounds__(256) void seg_pixel_kernel(SegPixelArgs A) {
  __shared__ int s_wy[SEG_MAX_IMG_WIN], s_wx[SEG_MAX_IMG_WIN], s_wi[SEG_MAX_IMG_WIN], s_row[SEG_MAX_IMG_WIN];
  const SegWinLists L = {s_wy, s_wx, s_wi, s_row};
  __shared__ int s_n;
  __shared__ uint8_t s_bg[SEG_MAX_IMG_WIN * SEG_MAX_G];
  __shared__ uint8_t s_lab[SEG_MAX_IMG_WIN * SEG_MAX_G];
  // dynamic LDS, sized by the host: A.tab_floats floats of table copies, then A.cover_slots * 256 covering-window entries
  // (one window per image and labels only: no table copy and one slot, so the block's LDS does not limit the occupancy)
  extern __shared__ float s_dyn[];
  float* s_tab = s_dyn;
  uint16_t* s_cov = reinterpret_cast<uint16_t*>(s_dyn + A.tab_floats);

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int upr = (A.W + PPL - 1) / PPL;  // units per row
  const int64_t total = (int64_t)A.H * upr;
  const int64_t u0 = (int64_t)blockIdx.x * 256;
  const int y_lo = (int)(u0 / upr);
  const int64_t u_last = u0 + 255 < total - 1 ? u0 + 255 : total - 1;
  const int y_hi = (int)(u_last / upr);
  const int off = A.with_bg ? 1 : 0;

  // the image's windows that touch this block's rows
  if (tid < 64) {
    int first = A.image_first[b], last = A.image_first[b + 1];
    first = first < 0 ? 0 : (first > A.n_windows ? A.n_windows : first);
    last = last < first ? first : (last > A.n_windows ? A.n_windows : last);
    const int cnt = last - first < SEG_MAX_IMG_WIN ? last - first : SEG_MAX_IMG_WIN;
    const int n = seg_window_compact(A.windows, first, cnt, A.win_h, y_lo, y_hi, L, 0, tid);
    if (tid == 0) s_n = n;
  }
  __syncthreads();
  const int nwin = s_n;
  seg_window_labels(A.best_score, A.table_max, A.best_class, A.with_bg, A.bg_thresh, A.G, L, nwin, s_bg, s_lab, tid);
  // one window and labels only: no table row is read, and no copy is made
  const bool staged = seg_stage_tables(A.table, A.G, A.N, L, nwin, s_tab, (LOGITS || nwin > 1) ? A.tab_floats : -1, tid);
  __syncthreads();

  SegBlockWindows bw = {s_wy, s_wx, s_wi, nwin};
  SegTables tb = {staged ? (const float*)s_tab : A.table, s_row, s_bg, A.G, A.N, off};
  const float sy = (float)A.gh / (float)A.win_h, sx = (float)A.gw / (float)A.win_w;

  const int64_t unit = u0 + tid;
  if (unit >= total) return;
  const int y = (int)(unit / upr);
  const int xq = (int)(unit % upr) * PPL;
  uint32_t lab_pack = 0, grp_pack = 0;
#pragma unroll
  for (int p = 0; p < PPL; ++p) {
    const int x = xq + p;
    if (x >= A.W) break;
    const int cnt = seg_pixel_cover(bw, A.soft, y, x, A.win_h, A.win_w, A.gh, A.gw, A.G, sy, sx, s_cov, A.cover_slots, tid);
    if (LOGITS) {
      const int64_t plane = (int64_t)A.H * A.W;
      float* o = A.logits + (int64_t)b * (A.N + off) * plane + (int64_t)y * A.W + x;
      for (int c = 0; c < A.N + off; ++c) o[c * plane] = cnt ? seg_class_logit(tb, c, cnt, s_cov, tid) : 0.f;
    } else {
      int lab = 0, grp = 0;
      if (cnt >= 1) {
        const int e = s_cov[tid];
        grp = e & 255;
        if (cnt == 1) {
          lab = s_lab[(e >> 8) * SEG_MAX_G + grp];
        } else if (A.labels) {
          float best = -INFINITY;
          for (int c = 0; c < A.N + off; ++c) {
            const float v = seg_class_logit(tb, c, cnt, s_cov, tid);
            if (v > best) { best = v; lab = c; }
          }
        }
      }
      lab_pack |= (uint32_t)(lab & 255) << (8 * p);
      grp_pack |= (uint32_t)grp << (8 * p);
    }
  }
  if (!LOGITS) {
    const int64_t o = ((int64_t)b * A.H + y) * A.W + xq;
    const bool dword = PPL == 4 && (A.W & 3) == 0 && ((reinterpret_cast<uintptr_t>(A.labels) | reinterpret_cast<uintptr_t>(A.groups)) & 3) == 0;
    if (dword) {  // rows are dword multiples on dword boundaries: one 4-byte store per lane
      if (A.labels) *reinterpret_cast<uint32_t*>(A.labels + o) = lab_pack;
      if (A.groups) *reinterpret_cast<uint32_t*>(A.groups + o) = grp_pack;
    } else {
      for (int p = 0; p < PPL && xq + p < A.W; ++p) {
        if (A.labels) A.labels[o + p] = (uint8_t)(lab_pack >> (8 * p));
        if (A.groups) A.groups[o + p] = (uint8_t)(grp_pack >> (8 * p));
      }
    }
  }
}

int seg_pixel_check(const char* what, int64_t n_windows, int64_t B, int64_t H, int64_t W, int64_t win_h, int64_t win_w,
                    int64_t gh, int64_t gw, int64_t G, int64_t N) {
  SEGCLIP_REQUIRE(B >= 0 && n_windows >= 0 && H >= 1 && W >= 1 && win_h >= 1 && win_w >= 1 && gh >= 1 && gw >= 1 && N >= 1,
                  "%s: sizes must be positive", what);
  SEGCLIP_REQUIRE(G >= 1 && G <= SEG_MAX_G, "%s: G=%lld groups, 1..%d supported", what, (long long)G, SEG_MAX_G);
  SEGCLIP_REQUIRE(B <= 65535 && n_windows <= (1 << 24) && H * W < (1ll << 31) && gh * gw * G < (1ll << 31) && N <= (1 << 20),
                  "%s: size out of range", what);
  return 0;
}

#include "segment_eval.inc"
#include "segment_wide.inc"
#include "segment_sweep.inc"
#include "segment_aug.inc"
#include "segment_frontend.inc"
#include "segment_render.inc"
#include "segment_refine.inc"
#include "segment_objects.inc"
#include "segment_sieve.inc"
#include "segment_superpixel.inc"
#include "segment_vote.inc"
#include "segment_boundary.inc"
#include "segment_confusion.inc"
#include "segment_image_areas.inc"
#include "train_frontend.inc"

}  // namespace

#define ST ((hipStream_t)stream)

// a size or count the kernels do not support (SEGCLIP_REQUIRE: an argument that is invalid)
#define SEG_REFUSE(cond, ...)          \
  do {                                 \
    if (cond) {                        \
      segclip_set_error(__VA_ARGS__);  \
      return SEGCLIP_ERR_UNSUPPORTED;  \
    }                                  \
  } while (0)

// More dynamic LDS than the 64 KiB a kernel gets without asking: the limit of `fn` is raised once per device (raised[64]).
static int seg_raise_lds(const char* what, const void* fn, int bytes, std::atomic<bool>* raised) {
  int dev = 0;
  SEGCLIP_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "%s: cannot query the current device", what);
  if (!raised[dev]) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    SEGCLIP_REQUIRE(e == hipSuccess, "%s: cannot raise the dynamic LDS limit: %s", what, hipGetErrorString(e));
    raised[dev] = true;
  }
  return 0;
}

extern "C" int segclip_seg_group_table(const float* group_tokens, int64_t group_stride, const float* pooled, int64_t pooled_stride,
                                       const float* text, const float* logit_scale, float* table, float* table_max,
                                       int32_t* best_class, float* best_score, uint8_t* topk_mask, int64_t n_windows, int64_t G,
                                       int64_t N, int64_t C, int64_t topk, void* stream) {
  SEGCLIP_REQUIRE(n_windows >= 0 && N >= 1 && C >= 1 && topk >= 1 && topk <= N, "seg_group_table: need N, C >= 1 and 1 <= topk <= N");
  SEGCLIP_REQUIRE(G >= 1 && G <= SEG_MAX_G, "seg_group_table: G=%lld groups, 1..%d supported", (long long)G, SEG_MAX_G);
  const int64_t lds = ((G + 1) * C + (G + 1) * N + 2 * N + SEG_MAX_G) * 4;
  SEG_REFUSE(lds > 64 * 1024, "seg_group_table: N=%lld classes x C=%lld need %lld bytes of LDS (64 KiB available)", (long long)N,
             (long long)C, (long long)lds);
  if (n_windows == 0) return 0;
  hipLaunchKernelGGL(seg_group_table_kernel, dim3((unsigned)n_windows), dim3(256), (size_t)lds, ST, group_tokens, group_stride, pooled,
                     pooled_stride, text, logit_scale, table, table_max, best_class, best_score, topk_mask, (int)G, (int)N, (int)C,
                     (int)topk);
  SEGCLIP_CHECK_LAUNCH("seg_group_table");
  return 0;
}

static SegPixelArgs seg_args(const float* soft_attn, const float* table, const float* table_max, const int32_t* best_class,
                             const float* best_score, const int32_t* windows, const int32_t* image_first, int64_t n_windows, int64_t B,
                             int64_t H, int64_t W, int64_t win_h, int64_t win_w, int64_t gh, int64_t gw, int64_t G, int64_t N,
                             int with_bg, float bg_thresh) {
  SegPixelArgs a;
  a.soft = soft_attn; a.table = table; a.table_max = table_max; a.best_class = best_class; a.best_score = best_score;
  a.windows = windows; a.image_first = image_first;
  a.n_windows = (int)n_windows; a.B = (int)B; a.H = (int)H; a.W = (int)W; a.win_h = (int)win_h; a.win_w = (int)win_w;
  a.gh = (int)gh; a.gw = (int)gw; a.G = (int)G; a.N = (int)N; a.with_bg = with_bg ? 1 : 0; a.bg_thresh = bg_thresh;
  a.labels = nullptr; a.groups = nullptr; a.logits = nullptr;
  return a;
}

// LDS of a pixel-kernel block.  With one window per image (n_windows <= B) a pixel has one covering window and the label
// kernel never reads a table row: no table copy, one slot.  Otherwise the tables of up to all windows of an image, capped.
static size_t seg_lds(SegPixelArgs& a, bool logits) {
  const bool multi = a.n_windows > a.B;
  a.cover_slots = multi ? SEG_MAX_COVER : 1;
  int64_t want = 0;
  if (logits || multi) {
    const int64_t per_image = multi ? (a.n_windows + a.B - 1) / a.B : 1;
    want = (per_image < SEG_MAX_IMG_WIN ? per_image : SEG_MAX_IMG_WIN) * a.G * a.N;
    if (want > SEG_TAB_FLOATS) want = SEG_TAB_FLOATS;
  }
  a.tab_floats = (int)((want + 1) & ~1ll);
  return (size_t)a.tab_floats * 4 + (size_t)a.cover_slots * 256 * 2;
}

extern "C" int segclip_seg_label_map(const float* soft_attn, const float* table, const float* table_max, const int32_t* best_class,
                                     const float* best_score, const int32_t* windows, const int32_t* image_first, int64_t n_windows,
                                     int64_t B, int64_t H, int64_t W, int64_t win_h, int64_t win_w, int64_t grid_h, int64_t grid_w,
                                     int64_t G, int64_t N, int with_bg, float bg_thresh, uint8_t* labels, uint8_t* groups,
                                     void* stream) {
  if (int rc = seg_pixel_check("seg_label_map", n_windows, B, H, W, win_h, win_w, grid_h, grid_w, G, N)) return rc;
  SEGCLIP_REQUIRE(labels || groups, "seg_label_map: one of labels, groups is required");
  SEG_REFUSE(labels && N + (with_bg ? 1 : 0) > 256, "seg_label_map: %lld classes do not fit the uint8 label map (use segclip_seg_logits)",
             (long long)(N + (with_bg ? 1 : 0)));
  if (B == 0) return 0;
  SegPixelArgs a = seg_args(soft_attn, table, table_max, best_class, best_score, windows, image_first, n_windows, B, H, W, win_h, win_w,
                            grid_h, grid_w, G, N, with_bg, bg_thresh);
  a.labels = labels; a.groups = groups;
  const int64_t units = H * cdiv(W, 4);
  const size_t lds = seg_lds(a, false);
  hipLaunchKernelGGL((seg_pixel_kernel<4, false>), dim3((unsigned)cdiv(units, 256), (unsigned)B), dim3(256), lds, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_label_map");
  return 0;
}

extern "C" int segclip_seg_logits(const float* soft_attn, const float* table, const float* table_max, const int32_t* best_class,
                                  const float* best_score, const int32_t* windows, const int32_t* image_first, int64_t n_windows,
                                  int64_t B, int64_t H, int64_t W, int64_t win_h, int64_t win_w, int64_t grid_h, int64_t grid_w,
                                  int64_t G, int64_t N, int with_bg, float bg_thresh, float* logits, void* stream) {
  if (int rc = seg_pixel_check("seg_logits", n_windows, B, H, W, win_h, win_w, grid_h, grid_w, G, N)) return rc;
  SEGCLIP_REQUIRE(logits != nullptr, "seg_logits: logits is required");
  if (B == 0) return 0;
  SegPixelArgs a = seg_args(soft_attn, table, table_max, best_class, best_score, windows, image_first, n_windows, B, H, W, win_h, win_w,
                            grid_h, grid_w, G, N, with_bg, bg_thresh);
  a.logits = logits;
  const size_t lds = seg_lds(a, true);
  hipLaunchKernelGGL((seg_pixel_kernel<1, true>), dim3((unsigned)cdiv(H * W, 256), (unsigned)B), dim3(256), lds, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_logits");
  return 0;
}

// What the rescaled entries require of their arguments (labels_n, gt_n: elements) ...
static int seg_eval_check(const char* what, int64_t soft_floats, int64_t labels_n, int64_t gt_n, int64_t n_windows, int64_t B,
                          int64_t n_blocks, int64_t G, int64_t N, bool labels, bool gt, bool areas) {
  SEGCLIP_REQUIRE(B >= 0 && n_windows >= 0 && n_blocks >= 0 && N >= 1 && soft_floats >= 0 && labels_n >= 0 && gt_n >= 0,
                  "%s: sizes must not be negative, N >= 1", what);
  SEGCLIP_REQUIRE(G >= 1 && G <= SEG_MAX_G, "%s: G=%lld groups, 1..%d supported", what, (long long)G, SEG_MAX_G);
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_windows <= (1 << 24) && n_blocks < (1ll << 31), "%s: size out of range", what);
  SEGCLIP_REQUIRE(labels || gt, "%s: one of labels, gt is required", what);
  SEGCLIP_REQUIRE(!gt || areas, "%s: a ground truth needs the areas to add to", what);
  return 0;
}

// ... and what they refuse: more classes C than the label element `elem` and the counters hold, too many windows in an image.
static int seg_eval_limits(const char* what, int64_t C, int max_classes, const char* elem, int64_t max_image_windows) {
  SEG_REFUSE(C > max_classes, "%s: %lld classes, at most %d (%s labels, per-class counters in LDS)", what, (long long)C, max_classes, elem);
  SEG_REFUSE(max_image_windows > SEG_MAX_IMG_WIN, "%s: %lld windows per image, at most %d", what, (long long)max_image_windows,
             SEG_MAX_IMG_WIN);
  return 0;
}

// The arguments every tile kernel takes; labels and gt stay null: their element type is the entry's.
static SegEvalArgs seg_eval_args(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                 const int32_t* best_class, const float* best_score, const int32_t* windows, const int64_t* images,
                                 int64_t n_windows, int64_t B, int64_t G, int64_t N, int with_bg, float bg_thresh, int64_t labels_n,
                                 int64_t gt_n, int ignore_index, int reduce_zero_label, int64_t* areas) {
  SegEvalArgs a;
  a.soft = soft_attn; a.table = table; a.table_max = table_max; a.best_class = best_class; a.best_score = best_score;
  a.windows = windows; a.images = images; a.soft_floats = soft_floats; a.labels_bytes = labels_n; a.gt_bytes = gt_n;
  a.n_windows = (int)n_windows; a.B = (int)B; a.G = (int)G; a.N = (int)N; a.with_bg = with_bg ? 1 : 0; a.bg_thresh = bg_thresh;
  a.labels = nullptr; a.gt = nullptr; a.ignore_index = ignore_index; a.reduce_zero = reduce_zero_label ? 1 : 0;
  a.areas = reinterpret_cast<unsigned long long*>(areas);
  return a;
}

// LDS of a tile kernel: the tables of the windows that touch a tile's source rows (a tile of 1024 output pixels spans few rows,
// so these are one or two rows of the window grid; more than the budget: the kernel reads the global table), and the
// covering-window lists of the four taps (one slot when no image has more than one window).  -> the bytes of both
static size_t seg_eval_lds(SegEvalArgs& a, int64_t max_image_windows, int64_t G, int64_t N) {
  const int64_t per_image = max_image_windows < 1 ? 1 : max_image_windows;
  a.cover_slots = per_image > 1 ? SEG_MAX_COVER : 1;
  int64_t want = per_image * G * N;
  if (want > SEG_EVAL_TAB_FLOATS) want = SEG_EVAL_TAB_FLOATS;
  a.tab_floats = (int)((want + 1) & ~1ll);
  return (size_t)a.tab_floats * 4 + (size_t)4 * a.cover_slots * 256 * 2;
}

extern "C" int segclip_seg_label_map_rescaled(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                              const int32_t* best_class, const float* best_score, const int32_t* windows,
                                              const int64_t* images, int64_t n_windows, int64_t B, int64_t n_blocks,
                                              int64_t max_image_windows, int64_t G, int64_t N, int with_bg, float bg_thresh,
                                              uint8_t* labels, int64_t labels_bytes, const uint8_t* gt, int64_t gt_bytes,
                                              int ignore_index, int reduce_zero_label, int64_t* areas, void* stream) {
  const char* what = "seg_label_map_rescaled";
  if (int rc = seg_eval_check(what, soft_floats, labels_bytes, gt_bytes, n_windows, B, n_blocks, G, N, labels, gt, areas)) return rc;
  if (int rc = seg_eval_limits(what, N + (with_bg ? 1 : 0), SEG_MAX_CLASSES, "uint8", max_image_windows)) return rc;
  if (B == 0 || n_blocks == 0) return 0;
  SegEvalArgs a = seg_eval_args(soft_attn, soft_floats, table, table_max, best_class, best_score, windows, images, n_windows, B, G, N,
                                with_bg, bg_thresh, labels_bytes, gt_bytes, ignore_index, reduce_zero_label, areas);
  a.labels = labels; a.gt = gt;
  const size_t lds = seg_eval_lds(a, max_image_windows, G, N);
  hipLaunchKernelGGL(seg_rescaled_kernel, dim3((unsigned)n_blocks), dim3(256), lds, ST, a);
  SEGCLIP_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int segclip_seg_label_map_rescaled_sweep(const float* soft_attn, int64_t soft_floats, const float* table,
                                                    const float* table_max, const int32_t* best_class, const float* best_score,
                                                    const int32_t* windows, const int64_t* images, int64_t n_windows, int64_t B,
                                                    int64_t n_blocks, int64_t max_image_windows, int64_t G, int64_t N,
                                                    const float* thresholds, int64_t T, uint8_t* labels, int64_t labels_bytes,
                                                    const uint8_t* gt, int64_t gt_bytes, int ignore_index, int reduce_zero_label,
                                                    int64_t* areas, void* stream) {
  const char* what = "seg_label_map_rescaled_sweep";
  if (int rc = seg_eval_check(what, soft_floats, labels_bytes, gt_bytes, n_windows, B, n_blocks, G, N, labels, gt, areas)) return rc;
  SEGCLIP_REQUIRE(thresholds && T >= 1, "%s: thresholds is a host array of T >= 1 floats", what);
  SEG_REFUSE(T > SEG_SWEEP_MAX_T, "%s: %lld thresholds, at most %d (they travel in the kernel arguments)", what, (long long)T,
             SEG_SWEEP_MAX_T);
  for (int64_t t = 0; t < T; ++t)
    SEGCLIP_REQUIRE(std::isfinite(thresholds[t]) && (t == 0 || thresholds[t] > thresholds[t - 1]),
                    "%s: thresholds must be finite and strictly increasing (entry %lld)", what, (long long)t);
  const int64_t C = N + 1;
  if (int rc = seg_eval_limits(what, C, SEG_MAX_CLASSES, "uint8", max_image_windows)) return rc;
  if (B == 0 || n_blocks == 0) return 0;
  SegSweepArgs s;
  s.e = seg_eval_args(soft_attn, soft_floats, table, table_max, best_class, best_score, windows, images, n_windows, B, G, N, 1, 0.f,
                      labels_bytes, gt_bytes, ignore_index, reduce_zero_label, areas);
  s.e.labels = labels; s.e.gt = gt;
  s.T = (int)T;
  for (int t = 0; t < SEG_SWEEP_MAX_T; ++t) s.thr[t] = t < T ? thresholds[t] : 0.f;
  // then the (T + 1, C) prediction and intersection buckets and the C label counters
  const size_t lds = seg_eval_lds(s.e, max_image_windows, G, N) + (size_t)(2 * (T + 1) + 1) * C * 4;
  SEGCLIP_REQUIRE(lds <= SEG_SWEEP_LDS_BYTES, "%s: internal LDS plan of %lld bytes", what, (long long)lds);
  if (lds > 56 * 1024) {  // beside 3 KiB of static LDS: past the 64 KiB a kernel gets without asking
    static std::atomic<bool> raised[64];
    if (int rc = seg_raise_lds(what, reinterpret_cast<const void*>(seg_sweep_kernel), SEG_SWEEP_LDS_BYTES, raised)) return rc;
  }
  hipLaunchKernelGGL(seg_sweep_kernel, dim3((unsigned)n_blocks), dim3(256), lds, ST, s);
  SEGCLIP_CHECK_LAUNCH(what);
  return 0;
}

// The launch of both view entries.  LDS: the covering-window lists of the four taps first, then the accumulators - every class
// when they fit beside the table copy, otherwise chunks of classes with every view's (maximum, sum) kept beside them.  (The
// kernel reads the global table when its windows' rows do not fit the copy.)
static int seg_views_launch(const char* what, bool dense, SegViewsArgs& v, int64_t max_image_windows, int64_t max_view_windows,
                            int64_t max_views, int64_t n_blocks, void* stream) {
  SegEvalArgs& a = v.e;
  const int64_t C = a.N + a.with_bg;
  // a.tab_floats as every tile kernel plans it; the byte count it returns and its cover_slots are for one view per image:
  // here a pixel's covering windows are those of ONE view (no view has two windows: no pixel has two covering windows)
  seg_eval_lds(a, max_image_windows, a.G, a.N);
  a.cover_slots = max_view_windows > 1 ? SEG_MAX_COVER : 1;
  const int64_t cov_bytes = (int64_t)4 * a.cover_slots * 256 * 2;
  const int64_t want = a.tab_floats;
  int64_t left = SEG_AUG_LDS_BYTES - cov_bytes;
  v.acc_classes = (int)C; v.ms_views = 0; v.max_views = (int)max_views;
  if (C * 1024 + want * 4 > left) {
    v.ms_views = (int)max_views;
    left -= max_views * 2 * 1024;
    const int64_t ch = (left - want * 4) / 1024;  // >= 16: 96 KiB less 32 of lists, 32 of (maximum, sum), 16 of tables
    v.acc_classes = (int)(ch < C ? ch : C);
  }
  const size_t lds = (size_t)a.tab_floats * 4 + (size_t)v.acc_classes * 1024 + (size_t)v.ms_views * 2048 + (size_t)cov_bytes;
  SEGCLIP_REQUIRE(v.acc_classes >= 1 && lds <= SEG_AUG_LDS_BYTES, "%s: internal LDS plan of %lld bytes", what, (long long)lds);
  static std::atomic<bool> raised[2][64];
  const void* fn = dense ? reinterpret_cast<const void*>(seg_views_kernel<true>) : reinterpret_cast<const void*>(seg_views_kernel<false>);
  if (int rc = seg_raise_lds(what, fn, SEG_AUG_LDS_BYTES, raised[dense])) return rc;
  if (dense) hipLaunchKernelGGL(seg_views_kernel<true>, dim3((unsigned)n_blocks), dim3(256), lds, ST, v);
  else hipLaunchKernelGGL(seg_views_kernel<false>, dim3((unsigned)n_blocks), dim3(256), lds, ST, v);
  SEGCLIP_CHECK_LAUNCH(what);
  return 0;
}

static int seg_views_check(const char* what, int64_t soft_floats, int64_t n_rows, int64_t n_windows, int64_t B, int64_t n_blocks,
                           int64_t max_image_windows, int64_t max_view_windows, int64_t max_views, int64_t G, int64_t N, int with_bg) {
  SEGCLIP_REQUIRE(B >= 0 && n_rows >= 0 && n_windows >= 0 && n_blocks >= 0 && N >= 1 && soft_floats >= 0,
                  "%s: sizes must not be negative, N >= 1", what);
  SEGCLIP_REQUIRE(G >= 1 && G <= SEG_MAX_G, "%s: G=%lld groups, 1..%d supported", what, (long long)G, SEG_MAX_G);
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_rows <= (1 << 24) && n_windows <= (1 << 24) && n_blocks < (1ll << 31), "%s: size out of range", what);
  SEG_REFUSE(N + (with_bg ? 1 : 0) > SEG_MAX_CLASSES, "%s: %lld classes, at most %d", what, (long long)(N + (with_bg ? 1 : 0)),
             SEG_MAX_CLASSES);
  SEG_REFUSE(max_views < 1 || max_views > SEG_MAX_VIEWS, "%s: %lld views of an image, 1..%d supported", what, (long long)max_views,
             SEG_MAX_VIEWS);
  SEG_REFUSE(max_image_windows > SEG_MAX_IMG_WIN, "%s: %lld windows over all views of an image, at most %d", what,
             (long long)max_image_windows, SEG_MAX_IMG_WIN);
  SEGCLIP_REQUIRE(max_view_windows <= max_image_windows, "%s: %lld windows in one view but %lld over all views of an image", what,
                  (long long)max_view_windows, (long long)max_image_windows);
  return 0;
}

static SegViewsArgs seg_views_args(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                   const float* best_score, const int32_t* windows, const int64_t* images, int64_t n_rows,
                                   const int64_t* views, int64_t n_windows, int64_t B, int64_t G, int64_t N, int with_bg, float bg_thresh) {
  SegViewsArgs v;
  v.e = seg_eval_args(soft_attn, soft_floats, table, table_max, nullptr, best_score, windows, images, n_windows, B, G, N, with_bg,
                      bg_thresh, 0, 0, 255, 0, nullptr);
  v.views = views; v.n_rows = (int)n_rows; v.probs = nullptr; v.probs_floats = 0;
  return v;
}

extern "C" int segclip_seg_label_map_views(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                           const float* best_score, const int32_t* windows, const int64_t* images, int64_t n_rows,
                                           const int64_t* views, int64_t n_windows, int64_t B, int64_t n_blocks,
                                           int64_t max_image_windows, int64_t max_view_windows, int64_t max_views, int64_t G,
                                           int64_t N, int with_bg, float bg_thresh, uint8_t* labels, int64_t labels_bytes, const uint8_t* gt, int64_t gt_bytes,
                                           int ignore_index, int reduce_zero_label, int64_t* areas, void* stream) {
  const char* what = "seg_label_map_views";
  if (int rc = seg_views_check(what, soft_floats, n_rows, n_windows, B, n_blocks, max_image_windows, max_view_windows, max_views, G, N,
                               with_bg))
    return rc;
  SEGCLIP_REQUIRE(labels_bytes >= 0 && gt_bytes >= 0, "%s: sizes must not be negative", what);
  SEGCLIP_REQUIRE(labels || gt, "%s: one of labels, gt is required", what);
  SEGCLIP_REQUIRE(!gt || areas, "%s: a ground truth needs the areas to add to", what);
  if (B == 0 || n_blocks == 0 || n_rows == 0) return 0;
  SEGCLIP_REQUIRE(soft_attn && table && table_max && best_score && windows && images && views, "%s: the tables are required", what);
  SegViewsArgs v = seg_views_args(soft_attn, soft_floats, table, table_max, best_score, windows, images, n_rows, views, n_windows, B, G, N,
                                  with_bg, bg_thresh);
  v.e.labels = labels; v.e.labels_bytes = labels_bytes; v.e.gt = gt; v.e.gt_bytes = gt_bytes; v.e.ignore_index = ignore_index;
  v.e.reduce_zero = reduce_zero_label ? 1 : 0; v.e.areas = reinterpret_cast<unsigned long long*>(areas);
  return seg_views_launch(what, false, v, max_image_windows, max_view_windows, max_views, n_blocks, stream);
}

extern "C" int segclip_seg_view_probs(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                      const float* best_score, const int32_t* windows, const int64_t* images, int64_t n_rows,
                                      const int64_t* views, int64_t n_windows, int64_t n_blocks, int64_t max_image_windows,
                                      int64_t max_view_windows, int64_t max_views, int64_t G, int64_t N, int with_bg, float bg_thresh, float* probs,
                                      int64_t probs_floats, void* stream) {
  const char* what = "seg_view_probs";
  if (int rc = seg_views_check(what, soft_floats, n_rows, n_windows, 1, n_blocks, max_image_windows, max_view_windows, max_views, G, N,
                               with_bg))
    return rc;
  SEGCLIP_REQUIRE(probs && probs_floats >= 0, "%s: probs is required", what);
  if (n_blocks == 0 || n_rows == 0) return 0;
  SEGCLIP_REQUIRE(soft_attn && table && table_max && best_score && windows && images && views, "%s: the tables are required", what);
  SegViewsArgs v = seg_views_args(soft_attn, soft_floats, table, table_max, best_score, windows, images, n_rows, views, n_windows, 1, G, N,
                                  with_bg, bg_thresh);
  v.probs = probs; v.probs_floats = probs_floats;
  return seg_views_launch(what, true, v, max_image_windows, max_view_windows, max_views, n_blocks, stream);
}

extern "C" int segclip_seg_areas(const uint8_t* pred, const uint8_t* gt, int64_t n, int64_t C, int ignore_index, int reduce_zero_label,
                                 int64_t* areas, void* stream) {
  SEGCLIP_REQUIRE(n >= 0 && n <= (1ll << 40) && C >= 1, "seg_areas: need 0 <= n <= 2^40 and C >= 1");
  SEGCLIP_REQUIRE(n == 0 || (pred && gt && areas), "seg_areas: pred, gt and areas are required");
  SEG_REFUSE(C > SEG_MAX_CLASSES, "seg_areas: %lld classes, at most %d", (long long)C, SEG_MAX_CLASSES);
  if (n == 0) return 0;
  const int64_t blocks = cdiv(n, SEG_EVAL_TILE) < 1024 ? cdiv(n, SEG_EVAL_TILE) : 1024;
  hipLaunchKernelGGL(seg_areas_kernel, dim3((unsigned)blocks), dim3(256), 0, ST, pred, gt, n, (int)C, ignore_index,
                     reduce_zero_label ? 1 : 0, reinterpret_cast<unsigned long long*>(areas));
  SEGCLIP_CHECK_LAUNCH("seg_areas");
  return 0;
}

extern "C" int segclip_seg_label_map_rescaled_wide(const float* soft_attn, int64_t soft_floats, const float* table,
                                                   const float* table_max, const int32_t* best_class, const float* best_score,
                                                   const int32_t* windows, const int64_t* images, int64_t n_windows, int64_t B,
                                                   int64_t n_blocks, int64_t max_image_windows, int64_t G, int64_t N, int with_bg,
                                                   float bg_thresh, uint16_t* labels, int64_t labels_elems, const uint16_t* gt,
                                                   int64_t gt_elems, int ignore_index, int reduce_zero_label, int64_t* areas,
                                                   void* stream) {
  const char* what = "seg_label_map_rescaled_wide";
  if (int rc = seg_eval_check(what, soft_floats, labels_elems, gt_elems, n_windows, B, n_blocks, G, N, labels, gt, areas)) return rc;
  if (int rc = seg_eval_limits(what, N + (with_bg ? 1 : 0), SEG_WIDE_MAX_CLASSES, "uint16", max_image_windows)) return rc;
  if (B == 0 || n_blocks == 0) return 0;
  SegWideArgs s;
  s.e = seg_eval_args(soft_attn, soft_floats, table, table_max, best_class, best_score, windows, images, n_windows, B, G, N, with_bg,
                      bg_thresh, labels_elems, gt_elems, ignore_index, reduce_zero_label, areas);
  s.labels = labels; s.gt = gt;
  size_t lds = seg_eval_lds(s.e, max_image_windows, G, N);
  // a table copy no single window fits (G * N > the copy) is not asked for: the kernel reads the global table then, and the
  // workgroup stays at three per CU beside its 14.5 KiB of static LDS
  if (G * N > SEG_EVAL_TAB_FLOATS) {
    lds -= (size_t)s.e.tab_floats * 4;
    s.e.tab_floats = 0;
  }
  SEGCLIP_REQUIRE(lds <= 48 * 1024, "%s: internal LDS plan of %lld bytes", what, (long long)lds);  // + 14.5 KiB static <= 64 KiB
  hipLaunchKernelGGL(seg_rescaled_wide_kernel, dim3((unsigned)n_blocks), dim3(256), lds, ST, s);
  SEGCLIP_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int segclip_seg_areas_wide(const uint16_t* pred, const uint16_t* gt, int64_t n, int64_t C, int ignore_index,
                                      int reduce_zero_label, int64_t* areas, void* stream) {
  SEGCLIP_REQUIRE(n >= 0 && n <= (1ll << 40) && C >= 1, "seg_areas_wide: need 0 <= n <= 2^40 and C >= 1");
  SEGCLIP_REQUIRE(n == 0 || (pred && gt && areas), "seg_areas_wide: pred, gt and areas are required");
  SEG_REFUSE(C > SEG_WIDE_MAX_CLASSES, "seg_areas_wide: %lld classes, at most %d", (long long)C, SEG_WIDE_MAX_CLASSES);
  if (n == 0) return 0;
  const int64_t blocks = cdiv(n, SEG_EVAL_TILE) < 1024 ? cdiv(n, SEG_EVAL_TILE) : 1024;
  hipLaunchKernelGGL(seg_areas_wide_kernel, dim3((unsigned)blocks), dim3(256), 0, ST, pred, gt, n, (int)C, ignore_index,
                     reduce_zero_label ? 1 : 0, reinterpret_cast<unsigned long long*>(areas));
  SEGCLIP_CHECK_LAUNCH("seg_areas_wide");
  return 0;
}

// The route of a confusion count and its launch shape: dense where the (C + 1)^2 counters fit the LDS a workgroup obtains on the
// current device (past 64 KiB the limit of both dense kernels is raised, once per device; a failure is remembered and gives the
// sparse route), the grid as segment_confusion.inc states it.
struct SegConfPlan {
  bool dense;
  size_t lds;
  int64_t max_blocks, wg_pixels;
};
static int seg_conf_plan(const char* what, int64_t C, SegConfPlan& p) {
  int dev = 0, ncu = 0;
  SEGCLIP_REQUIRE(segclip_current_device(&dev, &ncu) && ncu >= 1, "%s: cannot query the current device", what);
  const size_t dense_lds = (size_t)(((C + 1) * (C + 1) * 4 + 15) & ~15ll);
  p.dense = C <= SEG_CONF_DENSE_MAX_CLASSES;
  if (p.dense && dense_lds > 64 * 1024) {
    static std::atomic<int> raised[64];   // 0 not tried, 1 raised, 2 refused
    if (!raised[dev]) {
      const int most = (((SEG_CONF_DENSE_MAX_CLASSES + 1) * (SEG_CONF_DENSE_MAX_CLASSES + 1) * 4 + 15) & ~15);
      const hipError_t e8 = hipFuncSetAttribute(reinterpret_cast<const void*>(seg_confusion_kernel<uint8_t, true>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, most);
      const hipError_t e16 = hipFuncSetAttribute(reinterpret_cast<const void*>(seg_confusion_kernel<uint16_t, true>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, most);
      if (e8 != hipSuccess || e16 != hipSuccess) (void)hipGetLastError();   // not this call's error: the sparse route runs
      raised[dev] = (e8 == hipSuccess && e16 == hipSuccess) ? 1 : 2;
    }
    p.dense = raised[dev] == 1;
  }
  p.lds = p.dense ? dense_lds : (size_t)SEG_CONF_SLOTS * 8;
  const int64_t cells = (int64_t)p.lds / 4, per_cu = (160 * 1024) / (int64_t)p.lds;
  p.max_blocks = (int64_t)ncu * (per_cu < 4 ? per_cu : 4);
  p.wg_pixels = 2 * cells > SEG_CONF_MIN_WG_PIXELS ? 2 * cells : SEG_CONF_MIN_WG_PIXELS;
  return 0;
}

template <typename T>
static int seg_confusion_launch(const char* what, const T* pred, const T* gt, int64_t n, int64_t C, int max_classes, int ignore_index,
                                int reduce_zero_label, int64_t* conf, void* stream) {
  SEGCLIP_REQUIRE(n >= 0 && n <= (1ll << 40) && C >= 1, "%s: need 0 <= n <= 2^40 and C >= 1", what);
  SEGCLIP_REQUIRE(n == 0 || (pred && gt && conf), "%s: pred, gt and conf are required", what);
  SEGCLIP_REQUIRE(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) & (sizeof(T) - 1)) == 0 &&
                      (reinterpret_cast<uintptr_t>(conf) & 7) == 0,
                  "%s: pred and gt are aligned to their element, conf to 8 bytes", what);
  SEG_REFUSE(C > max_classes, "%s: %lld classes, at most %d", what, (long long)C, max_classes);
  if (n == 0) return 0;
  SegConfPlan p;
  if (int rc = seg_conf_plan(what, C, p)) return rc;
  // at most 2^30 pixels per launch: no 32-bit counter of a workgroup can overflow
  for (int64_t at = 0; at < n; at += SEG_CONF_LAUNCH_PIXELS) {
    const int64_t m = n - at < SEG_CONF_LAUNCH_PIXELS ? n - at : SEG_CONF_LAUNCH_PIXELS;
    const int64_t want = cdiv(m, p.wg_pixels);
    const dim3 grid((unsigned)(want < p.max_blocks ? want : p.max_blocks));
    if (p.dense)
      hipLaunchKernelGGL((seg_confusion_kernel<T, true>), grid, dim3(SEG_CONF_THREADS), p.lds, ST, pred + at, gt + at, m, (int)C,
                         ignore_index, reduce_zero_label ? 1 : 0, reinterpret_cast<unsigned long long*>(conf));
    else
      hipLaunchKernelGGL((seg_confusion_kernel<T, false>), grid, dim3(SEG_CONF_THREADS), p.lds, ST, pred + at, gt + at, m, (int)C,
                         ignore_index, reduce_zero_label ? 1 : 0, reinterpret_cast<unsigned long long*>(conf));
    SEGCLIP_CHECK_LAUNCH(what);
  }
  return 0;
}

extern "C" int segclip_seg_confusion(const uint8_t* pred, const uint8_t* gt, int64_t n, int64_t C, int ignore_index,
                                     int reduce_zero_label, int64_t* conf, void* stream) {
  return seg_confusion_launch("seg_confusion", pred, gt, n, C, SEG_MAX_CLASSES, ignore_index, reduce_zero_label, conf, stream);
}

extern "C" int segclip_seg_confusion_wide(const uint16_t* pred, const uint16_t* gt, int64_t n, int64_t C, int ignore_index,
                                          int reduce_zero_label, int64_t* conf, void* stream) {
  return seg_confusion_launch("seg_confusion_wide", pred, gt, n, C, SEG_WIDE_MAX_CLASSES, ignore_index, reduce_zero_label, conf, stream);
}

extern "C" int segclip_seg_confusion_route(int64_t C, int wide) {
  const char* what = "seg_confusion_route";
  const int max_classes = wide ? SEG_WIDE_MAX_CLASSES : SEG_MAX_CLASSES;
  SEGCLIP_REQUIRE(C >= 1, "%s: need C >= 1", what);
  SEG_REFUSE(C > max_classes, "%s: %lld classes, at most %d", what, (long long)C, max_classes);
  SegConfPlan p;
  if (int rc = seg_conf_plan(what, C, p)) return rc;
  return p.dense ? 0 : 1;
}

// per-image areas (segment_image_areas.inc): one launch of n_blocks workgroups, every table row checked on the device
template <typename T>
static int seg_image_areas_launch(const char* what, const T* pred, int64_t pred_elems, const T* gt, int64_t gt_elems,
                                  const int64_t* images, int64_t B, int64_t n_blocks, int64_t C, int max_classes, int ignore_index,
                                  int reduce_zero_label, int64_t* out, void* stream) {
  SEG_REFUSE(C < 1 || C > max_classes, "%s: %lld classes, 1..%d supported", what, (long long)C, max_classes);
  const int64_t lim = 1ll << 31;
  SEGCLIP_REQUIRE(B >= 0 && B < lim && n_blocks >= 0 && n_blocks < lim && pred_elems >= 0 && gt_elems >= 0,
                  "%s: need 0 <= B, n_blocks < 2^31 and buffer sizes that are not negative", what);
  if (B == 0 || n_blocks == 0) return 0;
  SEGCLIP_REQUIRE(pred && gt && images && out, "%s: pred, gt, images and out are required", what);
  SEGCLIP_REQUIRE(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) & (sizeof(T) - 1)) == 0 &&
                      ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(images)) & 7) == 0,
                  "%s: pred and gt are aligned to their element, images and out to 8 bytes", what);
  SegIAArgs a;
  a.pred = pred; a.gt = gt; a.images = images;
  a.pred_n = pred_elems; a.gt_n = gt_elems; a.n_blocks = n_blocks;
  a.B = (int)B; a.C = (int)C; a.ignore_index = ignore_index; a.reduce_zero = reduce_zero_label ? 1 : 0;
  a.out = reinterpret_cast<unsigned long long*>(out);
  hipLaunchKernelGGL(seg_image_areas_kernel<T>, dim3((unsigned)n_blocks), dim3(SEG_IA_THREADS), 0, ST, a);
  SEGCLIP_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int segclip_seg_image_areas(const uint8_t* pred, int64_t pred_elems, const uint8_t* gt, int64_t gt_elems,
                                       const int64_t* images, int64_t B, int64_t n_blocks, int64_t C, int ignore_index,
                                       int reduce_zero_label, int64_t* out, void* stream) {
  return seg_image_areas_launch("seg_image_areas", pred, pred_elems, gt, gt_elems, images, B, n_blocks, C, SEG_MAX_CLASSES, ignore_index,
                                reduce_zero_label, out, stream);
}

extern "C" int segclip_seg_image_areas_wide(const uint16_t* pred, int64_t pred_elems, const uint16_t* gt, int64_t gt_elems,
                                            const int64_t* images, int64_t B, int64_t n_blocks, int64_t C, int ignore_index,
                                            int reduce_zero_label, int64_t* out, void* stream) {
  return seg_image_areas_launch("seg_image_areas_wide", pred, pred_elems, gt, gt_elems, images, B, n_blocks, C, SEG_WIDE_MAX_CLASSES,
                                ignore_index, reduce_zero_label, out, stream);
}

// views: the (B, 7) table with a flag word per row and the kernel that mirrors (segment_frontend.inc)
static int seg_front_launch(const char* what, bool views, const int64_t* images, const int32_t* windows, int64_t n_windows, int64_t B, int64_t win_h,
                            int64_t win_w, const float* mean, const float* inv_std, int reverse_channels, float* out, void* stream) {
  const int64_t lim = 1ll << 31;
  SEGCLIP_REQUIRE(n_windows >= 0 && n_windows <= (1 << 24) && B >= 0 && B <= (1 << 24) && win_h >= 1 && win_w >= 1, "%s: sizes out of range", what);
  SEGCLIP_REQUIRE(mean && inv_std, "%s: mean and inv_std are required", what);
  SEG_REFUSE(win_h >= lim || win_w >= lim || win_h * win_w >= lim, "%s: a window of %lld x %lld pixels, fewer than 2^31 supported", what,
             (long long)win_h, (long long)win_w);
  if (n_windows == 0) return 0;
  SEGCLIP_REQUIRE(windows && out && (images || B == 0), "%s: images, windows and out are required", what);
  SegFrontArgs a;
  a.images = images; a.windows = windows; a.out = out;
  a.B = (int)B; a.win_h = (int)win_h; a.win_w = (int)win_w; a.upr = (int)cdiv(win_w, SEG_FE_PPL);
  const int64_t per_window = cdiv(win_h * a.upr, 256);
  SEGCLIP_REQUIRE(n_windows * per_window < lim, "%s: %lld windows of %lld x %lld pixels exceed one launch", what,
                  (long long)n_windows, (long long)win_h, (long long)win_w);
  a.blocks_per_window = (int)per_window;
  a.reverse = reverse_channels ? 1 : 0;
  a.vec = (win_w % SEG_FE_PPL == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.inv_std[c] = inv_std[c]; }
  if (views) hipLaunchKernelGGL(seg_front_kernel<true>, dim3((unsigned)(n_windows * per_window)), dim3(256), 0, ST, a);
  else hipLaunchKernelGGL(seg_front_kernel<false>, dim3((unsigned)(n_windows * per_window)), dim3(256), 0, ST, a);
  SEGCLIP_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int segclip_seg_windows_from_u8(const int64_t* images, const int32_t* windows, int64_t n_windows, int64_t B, int64_t win_h,
                                           int64_t win_w, const float* mean, const float* inv_std, int reverse_channels, float* out,
                                           void* stream) {
  return seg_front_launch("seg_windows_from_u8", false, images, windows, n_windows, B, win_h, win_w, mean, inv_std, reverse_channels, out, stream);
}

extern "C" int segclip_seg_view_windows_from_u8(const int64_t* images, const int32_t* windows, int64_t n_windows, int64_t B,
                                                int64_t win_h, int64_t win_w, const float* mean, const float* inv_std,
                                                int reverse_channels, float* out, void* stream) {
  return seg_front_launch("seg_view_windows_from_u8", true, images, windows, n_windows, B, win_h, win_w, mean, inv_std, reverse_channels, out, stream);
}

extern "C" int segclip_seg_groups_rescaled(const float* soft_attn, int64_t soft_floats, const int64_t* images, int64_t B,
                                           int64_t n_blocks, int64_t G, uint8_t* groups, int64_t groups_bytes, void* stream) {
  SEGCLIP_REQUIRE(B >= 0 && n_blocks >= 0 && soft_floats >= 0 && groups_bytes >= 0, "seg_groups_rescaled: sizes must not be negative");
  SEGCLIP_REQUIRE(G >= 1, "seg_groups_rescaled: G >= 1");
  SEG_REFUSE(G > SEG_MAX_G, "seg_groups_rescaled: G=%lld groups, 1..%d supported", (long long)G, SEG_MAX_G);
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_blocks < (1ll << 31), "seg_groups_rescaled: size out of range");
  if (B == 0 || n_blocks == 0) return 0;
  SEGCLIP_REQUIRE(soft_attn && images && groups, "seg_groups_rescaled: soft_attn, images and groups are required");
  SegGroupsArgs a;
  a.soft = soft_attn; a.images = images; a.soft_floats = soft_floats; a.groups_bytes = groups_bytes;
  a.B = (int)B; a.G = (int)G; a.groups = groups;
  hipLaunchKernelGGL(seg_groups_kernel, dim3((unsigned)n_blocks), dim3(256), 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_groups_rescaled");
  return 0;
}

extern "C" int segclip_seg_blend(const int64_t* images, int64_t B, int64_t n_blocks, const uint8_t* maps, int64_t maps_bytes,
                                 const uint8_t* palette, int64_t P, int reverse_channels, double a, double b, int skip_zero,
                                 uint8_t* out, int64_t out_bytes, int64_t* sums, void* stream) {
  SEGCLIP_REQUIRE(B >= 0 && n_blocks >= 0 && maps_bytes >= 0 && out_bytes >= 0, "seg_blend: sizes must not be negative");
  SEGCLIP_REQUIRE(P >= 1 && P <= SEG_MAX_PALETTE, "seg_blend: a palette has 1..%d colours, got %lld", SEG_MAX_PALETTE, (long long)P);
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_blocks < (1ll << 31), "seg_blend: size out of range");
  SEGCLIP_REQUIRE(a >= 0.0 && a < 1.0 && b > 0.0 && b <= 1.0, "seg_blend: a = 1 - opacity in [0, 1), b = opacity in (0, 1]");
  if (B == 0 || n_blocks == 0) return 0;
  SEGCLIP_REQUIRE(images && maps && palette && out, "seg_blend: images, maps, palette and out are required");
  SegBlendArgs k;
  k.images = images; k.maps = maps; k.palette = palette; k.maps_bytes = maps_bytes; k.out_bytes = out_bytes;
  k.B = (int)B; k.P = (int)P; k.reverse = reverse_channels ? 1 : 0; k.skip_zero = skip_zero ? 1 : 0; k.a = a; k.b = b;
  k.out = out; k.sums = reinterpret_cast<unsigned long long*>(sums);
  hipLaunchKernelGGL(seg_blend_kernel, dim3((unsigned)n_blocks), dim3(256), 0, ST, k);
  SEGCLIP_CHECK_LAUNCH("seg_blend");
  return 0;
}

// ---------------------------------------------------------------- pixel-adaptive refinement (segment_refine.inc)
struct SegRefineWs { int64_t pres, wts, plane0, plane1, bestv, bestl, total; };
static SegRefineWs seg_refine_ws(int64_t n, int64_t B, int64_t D) {
  const auto up = [](int64_t v) { return (v + 255) & ~255ll; };
  SegRefineWs w;
  w.pres = 0;
  w.wts = up(B * 8 * 4);
  w.plane0 = w.wts + up(8 * D * n * 4);
  w.plane1 = w.plane0 + up(n * SEG_REFINE_PLANES * 4);
  w.bestv = w.plane1 + up(n * SEG_REFINE_PLANES * 4);
  w.bestl = w.bestv + up(n * 4);
  w.total = w.bestl + up(n);
  return w;
}

extern "C" int64_t segclip_seg_refine_ws_bytes(int64_t labels_bytes, int64_t B, int64_t D) {
  SEG_REFUSE(labels_bytes < 0 || labels_bytes > (1ll << 40) || B < 0 || B > (1 << 24) || D < 1 || D > SEG_REFINE_MAX_D,
             "seg_refine_ws_bytes: need 0 <= labels_bytes <= 2^40, 0 <= B <= 2^24 and 1 <= D <= %d", SEG_REFINE_MAX_D);
  return seg_refine_ws(labels_bytes, B, D).total;
}

template <bool FIRST, bool LAST>
static void seg_refine_step(const SegRefineArgs& a, int64_t n_blocks, int chunk, int parity, void* stream) {
  hipLaunchKernelGGL((seg_refine_step_kernel<FIRST, LAST>), dim3((unsigned)n_blocks), dim3(256), 0, ST, a, chunk, parity);
}

extern "C" int segclip_seg_refine(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint8_t* labels,
                                  int64_t labels_bytes, int64_t C, const int32_t* dilations, int64_t D, int64_t T, const float* mean,
                                  const float* inv_std, int reverse_channels, uint8_t* out, int64_t out_bytes, const uint8_t* gt,
                                  int64_t gt_bytes, int ignore_index, int reduce_zero_label, int64_t* areas, float* probs,
                                  int64_t probs_floats, void* ws, int64_t ws_bytes, void* stream) {
  SEGCLIP_REQUIRE(B >= 0 && n_blocks >= 0 && labels_bytes >= 0 && out_bytes >= 0 && gt_bytes >= 0 && probs_floats >= 0 && ws_bytes >= 0,
                  "seg_refine: sizes must not be negative");
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_blocks < (1ll << 31) && labels_bytes <= (1ll << 40), "seg_refine: size out of range");
  SEGCLIP_REQUIRE(dilations && mean && inv_std, "seg_refine: dilations, mean and inv_std are required");
  SEGCLIP_REQUIRE(!gt || areas, "seg_refine: a ground truth needs the areas to add to");
  SEGCLIP_REQUIRE(!probs || B == 1, "seg_refine: probs holds the planes of one image, got %lld images", (long long)B);
  for (int c = 0; c < 3; ++c)
    SEGCLIP_REQUIRE(inv_std[c] > 0.f && inv_std[c] < INFINITY && mean[c] == mean[c], "seg_refine: inv_std is positive and finite");
  SEG_REFUSE(D < 1 || D > SEG_REFINE_MAX_D, "seg_refine: %lld dilations, 1..%d supported", (long long)D, SEG_REFINE_MAX_D);
  for (int64_t i = 0; i < D; ++i)
    SEG_REFUSE(dilations[i] < 1 || dilations[i] > SEG_REFINE_MAX_DIL || (i > 0 && dilations[i] <= dilations[i - 1]),
               "seg_refine: dilations are increasing values in 1..%d, got %d at position %lld", SEG_REFINE_MAX_DIL, dilations[i],
               (long long)i);
  SEG_REFUSE(T < 0 || T > SEG_REFINE_MAX_T, "seg_refine: %lld iterations, 0..%d supported", (long long)T, SEG_REFINE_MAX_T);
  SEG_REFUSE(C < 1 || C > SEG_MAX_CLASSES, "seg_refine: %lld classes, 1..%d supported (uint8 labels)", (long long)C, SEG_MAX_CLASSES);
  SEG_REFUSE(max_side < 1 || max_side >= SEG_REFINE_LIMIT, "seg_refine: sides of 1..%d pixels supported, got a bound of %lld",
             SEG_REFINE_LIMIT - 1, (long long)max_side);
  const SegRefineWs w = seg_refine_ws(labels_bytes, B, D);
  SEG_REFUSE(T > 0 && ws_bytes < w.total, "seg_refine: the workspace has %lld bytes, segclip_seg_refine_ws_bytes asks for %lld",
             (long long)ws_bytes, (long long)w.total);
  if (B == 0 || n_blocks == 0) return 0;
  SEGCLIP_REQUIRE(images && labels && out, "seg_refine: images, labels and out are required");
  SEGCLIP_REQUIRE(out_bytes == labels_bytes, "seg_refine: out has the layout of labels: %lld bytes, got %lld", (long long)labels_bytes,
                  (long long)out_bytes);
  SEGCLIP_REQUIRE(out + out_bytes <= labels || labels + labels_bytes <= out, "seg_refine: out overlaps labels (the refinement is out of place)");
  SEGCLIP_REQUIRE(T == 0 || (ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0), "seg_refine: the workspace is required, 16-byte aligned");

  SegRefineArgs a;
  a.images = images; a.labels = labels; a.out = out; a.gt = gt; a.areas = reinterpret_cast<unsigned long long*>(areas);
  a.probs = probs; a.labels_bytes = labels_bytes; a.gt_bytes = gt_bytes; a.probs_floats = probs_floats;
  a.B = (int)B; a.C = (int)C; a.D = (int)D; a.max_side = (int)max_side; a.ignore_index = ignore_index;
  a.reduce_zero = reduce_zero_label ? 1 : 0;
  for (int i = 0; i < SEG_REFINE_MAX_D; ++i) a.dil[i] = i < D ? dilations[i] : 0;
  // the picture's channel s is the transform's channel 2 - s when the picture is BGR (segclip_seg_windows_from_u8)
  for (int s = 0; s < 3; ++s) a.isd[s] = inv_std[reverse_channels ? 2 - s : s];
  char* base = static_cast<char*>(ws);
  a.pres = reinterpret_cast<uint32_t*>(base + w.pres);
  a.wts = reinterpret_cast<float*>(base + w.wts);
  a.plane[0] = reinterpret_cast<float*>(base + w.plane0);
  a.plane[1] = reinterpret_cast<float*>(base + w.plane1);
  a.bestv = reinterpret_cast<float*>(base + w.bestv);
  a.bestl = reinterpret_cast<uint8_t*>(base + w.bestl);
  if (T == 0) { a.pres = nullptr; a.wts = a.plane[0] = a.plane[1] = a.bestv = nullptr; a.bestl = nullptr; }

  if (probs && probs_floats > 0) {  // the planes of the labels that do not occur
    const hipError_t e = hipMemsetAsync(probs, 0, (size_t)probs_floats * sizeof(float), ST);
    SEGCLIP_REQUIRE(e == hipSuccess, "seg_refine: clearing probs failed: %s", hipGetErrorString(e));
  }
  const dim3 grid((unsigned)n_blocks), block(256);
  if (T == 0) {
    hipLaunchKernelGGL(seg_refine_copy_kernel, grid, block, 0, ST, a);
    SEGCLIP_CHECK_LAUNCH("seg_refine");
    return 0;
  }
  {
    const hipError_t e = hipMemsetAsync(a.pres, 0, (size_t)B * 8 * sizeof(uint32_t), ST);
    SEGCLIP_REQUIRE(e == hipSuccess, "seg_refine: clearing the label presence maps failed: %s", hipGetErrorString(e));
  }
  switch (D) {
    case 1: hipLaunchKernelGGL(seg_refine_weights_kernel<1>, grid, block, 0, ST, a); break;
    case 2: hipLaunchKernelGGL(seg_refine_weights_kernel<2>, grid, block, 0, ST, a); break;
    case 3: hipLaunchKernelGGL(seg_refine_weights_kernel<3>, grid, block, 0, ST, a); break;
    case 4: hipLaunchKernelGGL(seg_refine_weights_kernel<4>, grid, block, 0, ST, a); break;
    case 5: hipLaunchKernelGGL(seg_refine_weights_kernel<5>, grid, block, 0, ST, a); break;
    default: hipLaunchKernelGGL(seg_refine_weights_kernel<6>, grid, block, 0, ST, a); break;
  }
  SEGCLIP_CHECK_LAUNCH("seg_refine (weights)");
  // a chunk's T steps follow each other on the stream, and the chunks share the plane pair; a chunk beyond an image's label
  // count costs that image T launches of workgroups that exit at once
  const int chunks = (int)cdiv(C, SEG_REFINE_PLANES);
  for (int chunk = 0; chunk < chunks; ++chunk)
    for (int t = 0; t < (int)T; ++t) {
      const bool first = t == 0, last = t == (int)T - 1;
      if (first && last) seg_refine_step<true, true>(a, n_blocks, chunk, t & 1, stream);
      else if (first) seg_refine_step<true, false>(a, n_blocks, chunk, t & 1, stream);
      else if (last) seg_refine_step<false, true>(a, n_blocks, chunk, t & 1, stream);
      else seg_refine_step<false, false>(a, n_blocks, chunk, t & 1, stream);
      SEGCLIP_CHECK_LAUNCH("seg_refine (step)");
    }
  return 0;
}

// ---------------------------------------------------------------- connected components (segment_objects.inc)
// The entries of the three post-processing stages exist for uint8_t and uint16_t labels: one body each, a template on the label
// element L.  Sizes and offsets count elements; a workspace part that holds labels has sizeof(L) bytes per pixel.
// What differs between the two is SegLabel<L> (segment_objects.inc); the uint8 entries keep their messages word for word.
struct SegCCWs { int64_t parent, root, area, rank, seg, part, total; };
static SegCCWs seg_cc_ws(int64_t n, int64_t n_blocks) {
  const auto up = [](int64_t v) { return (v + 255) & ~255ll; };
  SegCCWs w;
  w.seg = 0;  // first: the one part that is cleared
  w.part = up(n_blocks * SEG_CC_TH * 8);
  w.parent = w.part + up(cdiv(n_blocks * SEG_CC_TH, SEG_CC_SCAN_CHUNK) * 8);
  w.root = w.parent + up(n * 4);
  w.area = w.root + up(n * 4);
  w.rank = w.area + up(n * 4);
  w.total = w.rank + up(n * 4);
  return w;
}

extern "C" int64_t segclip_seg_components_ws_bytes(int64_t labels_bytes, int64_t B, int64_t n_blocks) {
  SEG_REFUSE(labels_bytes < 0 || labels_bytes > (1ll << 40) || B < 0 || B > (1 << 24) || n_blocks < 0 || n_blocks >= (1ll << 31),
             "seg_components_ws_bytes: need 0 <= labels_bytes <= 2^40, 0 <= B <= 2^24 and 0 <= n_blocks < 2^31");
  return seg_cc_ws(labels_bytes, n_blocks).total;
}

// `what`: the entry's name in messages; labels_bytes, cleaned_bytes: ELEMENTS of L (the uint8 entry's argument names)
template <class L>
static int seg_components_run(const char* what, const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const L* labels,
                              int64_t labels_bytes, int connectivity, int skip_label, int32_t* ids, int32_t* area_px,
                              int64_t px_count, int64_t* records, int64_t K, int64_t* count, int64_t min_area, int fill,
                              L* cleaned, int64_t cleaned_bytes, void* ws, int64_t ws_bytes, void* stream) {
  const char* unit = SegLabel<L>::unit;
  SEGCLIP_REQUIRE(B >= 0 && n_blocks >= 0 && labels_bytes >= 0 && px_count >= 0 && K >= 0 && cleaned_bytes >= 0 && ws_bytes >= 0,
                  "%s: sizes must not be negative", what);
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_blocks < (1ll << 31) && labels_bytes <= (1ll << 40), "%s: size out of range", what);
  SEGCLIP_REQUIRE(!records || count, "%s: records need count, the number of rows that exist", what);
  SEGCLIP_REQUIRE(!(ids || area_px) || px_count == labels_bytes,
                  "%s: ids and area_px have one entry per label%s: %lld, got %lld", what, sizeof(L) == 1 ? " byte" : "", (long long)labels_bytes,
                  (long long)px_count);
  SEGCLIP_REQUIRE(!cleaned || cleaned_bytes == labels_bytes, "%s: cleaned has the layout of labels: %lld %s, got %lld", what,
                  (long long)labels_bytes, unit, (long long)cleaned_bytes);
  SEGCLIP_REQUIRE(!cleaned || !labels || cleaned + cleaned_bytes <= labels || labels + labels_bytes <= cleaned,
                  "%s: cleaned overlaps labels (the despeckling is out of place)", what);
  SEG_REFUSE(connectivity != 4 && connectivity != 8, "%s: connectivity is 4 or 8, got %d", what, connectivity);
  SEG_REFUSE(skip_label < -1 || skip_label > SegLabel<L>::TOP, "%s: skip_label is %s or -1, got %d", what, SegLabel<L>::word, skip_label);
  SEG_REFUSE(fill < 0 || fill > SegLabel<L>::TOP, "%s: fill is %s, got %d", what, SegLabel<L>::word, fill);
  SEG_REFUSE(min_area < 0, "%s: min_area must not be negative, got %lld", what, (long long)min_area);
  SEG_REFUSE(max_side < 1 || max_side >= SEG_CC_LIMIT, "%s: sides of 1..%d pixels supported, got a bound of %lld", what,
             SEG_CC_LIMIT - 1, (long long)max_side);
  const SegCCWs w = seg_cc_ws(labels_bytes, n_blocks);
  SEG_REFUSE(ws_bytes < w.total, "%s: the workspace has %lld bytes, segclip_seg_components_ws_bytes asks for %lld", what,
             (long long)ws_bytes, (long long)w.total);
  if (B == 0 || n_blocks == 0) {
    if (count) {
      const hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), ST);
      SEGCLIP_REQUIRE(e == hipSuccess, "%s: clearing count failed: %s", what, hipGetErrorString(e));
    }
    return 0;
  }
  SEGCLIP_REQUIRE(images && labels, "%s: images and labels are required", what);
  SEGCLIP_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace is required, 16-byte aligned", what);
  if (!ids && !area_px && !count && !cleaned) return 0;  // nothing asked for

  SegCCArgs a;
  a.images = images; a.labels = labels; a.labels_n = labels_bytes; a.n_blocks = n_blocks; a.n_seg = n_blocks * SEG_CC_TH;
  a.B = (int)B; a.max_side = (int)max_side; a.conn8 = connectivity == 8; a.skip = skip_label;
  char* base = static_cast<char*>(ws);
  a.seg = reinterpret_cast<int64_t*>(base + w.seg);
  a.parent = reinterpret_cast<int32_t*>(base + w.parent);
  a.root = ids ? ids : reinterpret_cast<int32_t*>(base + w.root);
  a.area = reinterpret_cast<int32_t*>(base + w.area);
  a.rank = reinterpret_cast<int32_t*>(base + w.rank);
  a.area_px = area_px; a.records = records; a.K = records ? K : 0; a.min_area = min_area; a.fill = fill; a.cleaned = cleaned;

  const dim3 grid((unsigned)n_blocks), block(256);
  hipLaunchKernelGGL(seg_cc_local_kernel<L>, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_components (local)");
  hipLaunchKernelGGL(seg_cc_merge_kernel<L>, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_components (merge)");
  if (count) {
    // the entries of a table row that the device skips, and those past an image's last row, count nothing
    const hipError_t e = hipMemsetAsync(a.seg, 0, (size_t)a.n_seg * sizeof(int64_t), ST);
    SEGCLIP_REQUIRE(e == hipSuccess, "%s: clearing the segment counts failed: %s", what, hipGetErrorString(e));
    hipLaunchKernelGGL((seg_cc_roots_kernel<false, L>), grid, block, 0, ST, a);
    SEGCLIP_CHECK_LAUNCH("seg_components (count)");
    int64_t* part = reinterpret_cast<int64_t*>(base + w.part);
    const int64_t chunks = cdiv(a.n_seg, SEG_CC_SCAN_CHUNK);
    hipLaunchKernelGGL(seg_cc_chunk_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, ST, a.seg, a.n_seg, part);
    SEGCLIP_CHECK_LAUNCH("seg_components (chunk totals)");
    hipLaunchKernelGGL(seg_cc_scan_kernel, dim3(1), dim3(1024), 0, ST, part, chunks, count);
    SEGCLIP_CHECK_LAUNCH("seg_components (scan)");
    hipLaunchKernelGGL(seg_cc_chunk_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, ST, a.seg, a.n_seg, part);
    SEGCLIP_CHECK_LAUNCH("seg_components (chunk scans)");
    if (records && K > 0) {
      hipLaunchKernelGGL((seg_cc_roots_kernel<true, L>), grid, block, 0, ST, a);
      SEGCLIP_CHECK_LAUNCH("seg_components (rank)");
    }
  }
  if (records && K > 0) hipLaunchKernelGGL(seg_cc_stats_kernel<true>, grid, block, 0, ST, a);
  else hipLaunchKernelGGL(seg_cc_stats_kernel<false>, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_components (stats)");
  if (area_px || cleaned) {
    hipLaunchKernelGGL(seg_cc_final_kernel<L>, grid, block, 0, ST, a);
    SEGCLIP_CHECK_LAUNCH("seg_components (final)");
  }
  return 0;
}

extern "C" int segclip_seg_components(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint8_t* labels,
                                      int64_t labels_bytes, int connectivity, int skip_label, int32_t* ids, int32_t* area_px,
                                      int64_t px_count, int64_t* records, int64_t K, int64_t* count, int64_t min_area, int fill,
                                      uint8_t* cleaned, int64_t cleaned_bytes, void* ws, int64_t ws_bytes, void* stream) {
  return seg_components_run<uint8_t>("seg_components", images, B, n_blocks, max_side, labels, labels_bytes, connectivity, skip_label, ids,
                                     area_px, px_count, records, K, count, min_area, fill, cleaned, cleaned_bytes, ws, ws_bytes, stream);
}

// The workspace holds no labels: the size is segclip_seg_components_ws_bytes of the element count, and there is no wide query.
extern "C" int segclip_seg_components_wide(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint16_t* labels,
                                           int64_t labels_n, int connectivity, int skip_label, int32_t* ids, int32_t* area_px,
                                           int64_t px_count, int64_t* records, int64_t K, int64_t* count, int64_t min_area, int fill,
                                           uint16_t* cleaned, int64_t cleaned_n, void* ws, int64_t ws_bytes, void* stream) {
  return seg_components_run<uint16_t>("seg_components_wide", images, B, n_blocks, max_side, labels, labels_n, connectivity, skip_label,
                                      ids, area_px, px_count, records, K, count, min_area, fill, cleaned, cleaned_n, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- despeckling by merging (segment_sieve.inc)
struct SegSieveWs { int64_t slot, parent, root, area, tmp, total; };
// n pixels; the map between two rounds has `width` bytes per pixel
static SegSieveWs seg_sieve_ws(int64_t n, int64_t width) {
  const auto up = [](int64_t v) { return (v + 255) & ~255ll; };
  SegSieveWs w;
  w.slot = 0;
  w.parent = up(n * 8);
  w.root = w.parent + up(n * 4);
  w.area = w.root + up(n * 4);
  w.tmp = w.area + up(n * 4);
  w.total = w.tmp + up(n * width);
  return w;
}

extern "C" int64_t segclip_seg_sieve_ws_bytes(int64_t labels_bytes, int64_t B, int64_t n_blocks) {
  SEG_REFUSE(labels_bytes < 0 || labels_bytes > (1ll << 40) || B < 0 || B > (1 << 24) || n_blocks < 0 || n_blocks >= (1ll << 31),
             "seg_sieve_ws_bytes: need 0 <= labels_bytes <= 2^40, 0 <= B <= 2^24 and 0 <= n_blocks < 2^31");
  return seg_sieve_ws(labels_bytes, 1).total;
}

extern "C" int64_t segclip_seg_sieve_wide_ws_bytes(int64_t labels_n, int64_t B, int64_t n_blocks) {
  SEG_REFUSE(labels_n < 0 || labels_n > (1ll << 40) || B < 0 || B > (1 << 24) || n_blocks < 0 || n_blocks >= (1ll << 31),
             "seg_sieve_wide_ws_bytes: need 0 <= labels_n <= 2^40, 0 <= B <= 2^24 and 0 <= n_blocks < 2^31");
  return seg_sieve_ws(labels_n, 2).total;
}

// `what`: the entry's name in messages; labels_bytes, cleaned_bytes: ELEMENTS of L (the uint8 entry's argument names)
template <class L>
static int seg_sieve_run(const char* what, const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const L* labels,
                         int64_t labels_bytes, int connectivity, int skip_label, int64_t min_area, int orphan_fill, int rounds,
                         L* cleaned, int64_t cleaned_bytes, void* ws, int64_t ws_bytes, void* stream) {
  const char* unit = SegLabel<L>::unit;
  SEGCLIP_REQUIRE(B >= 0 && n_blocks >= 0 && labels_bytes >= 0 && cleaned_bytes >= 0 && ws_bytes >= 0,
                  "%s: sizes must not be negative", what);
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_blocks < (1ll << 31) && labels_bytes <= (1ll << 40), "%s: size out of range", what);
  SEGCLIP_REQUIRE(cleaned_bytes == labels_bytes, "%s: cleaned has the layout of labels: %lld %s, got %lld", what,
                  (long long)labels_bytes, unit, (long long)cleaned_bytes);
  SEGCLIP_REQUIRE(!cleaned || !labels || cleaned + cleaned_bytes <= labels || labels + labels_bytes <= cleaned,
                  "%s: cleaned overlaps labels (the despeckling is out of place)", what);
  SEG_REFUSE(connectivity != 4 && connectivity != 8, "%s: connectivity is 4 or 8, got %d", what, connectivity);
  SEG_REFUSE(skip_label < -1 || skip_label > SegLabel<L>::TOP, "%s: skip_label is %s or -1, got %d", what,
             SegLabel<L>::word, skip_label);
  SEG_REFUSE(orphan_fill < -1 || orphan_fill > SegLabel<L>::TOP, "%s: orphan_fill is %s or -1, got %d", what,
             SegLabel<L>::word, orphan_fill);
  SEG_REFUSE(rounds < 1 || rounds > SEG_SIEVE_MAX_ROUNDS, "%s: 1..%d rounds supported, got %d", what, SEG_SIEVE_MAX_ROUNDS, rounds);
  SEG_REFUSE(min_area < 0, "%s: min_area must not be negative, got %lld", what, (long long)min_area);
  SEG_REFUSE(max_side < 1 || max_side >= SEG_CC_LIMIT, "%s: sides of 1..%d pixels supported, got a bound of %lld", what,
             SEG_CC_LIMIT - 1, (long long)max_side);
  const SegSieveWs w = seg_sieve_ws(labels_bytes, (int64_t)sizeof(L));
  SEG_REFUSE(ws_bytes < w.total, "%s: the workspace has %lld bytes, segclip_%s_ws_bytes asks for %lld", what,
             (long long)ws_bytes, what, (long long)w.total);
  if (B == 0 || n_blocks == 0) return 0;
  SEGCLIP_REQUIRE(images && labels && cleaned, "%s: images, labels and cleaned are required", what);
  SEGCLIP_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace is required, 16-byte aligned", what);

  SegSieveArgs s;
  SegCCArgs& a = s.cc;
  a.images = images; a.labels_n = labels_bytes; a.n_blocks = n_blocks; a.n_seg = n_blocks * SEG_CC_TH;
  a.B = (int)B; a.max_side = (int)max_side; a.conn8 = connectivity == 8; a.skip = skip_label;
  char* base = static_cast<char*>(ws);
  a.seg = nullptr; a.rank = nullptr; a.area_px = nullptr; a.records = nullptr; a.K = 0; a.fill = 0; a.cleaned = nullptr;
  a.parent = reinterpret_cast<int32_t*>(base + w.parent);
  a.root = reinterpret_cast<int32_t*>(base + w.root);
  a.area = reinterpret_cast<int32_t*>(base + w.area);
  a.min_area = min_area;
  s.slot = reinterpret_cast<unsigned long long*>(base + w.slot);
  L* tmp = reinterpret_cast<L*>(base + w.tmp);

  // round r reads what round r - 1 wrote; the outputs alternate so that the last round's is `cleaned`.  A kernel touches the
  // pixels of the table's images only, so the labels between the maps are read and written by none.
  const dim3 grid((unsigned)n_blocks), block(256);
  const L* in = labels;
  for (int r = 1; r <= rounds; ++r) {
    a.labels = in;
    L* out = (rounds - r) % 2 == 0 ? cleaned : tmp;
    s.out = out;
    s.orphan = r == rounds ? orphan_fill : -1;
    const hipError_t e = hipMemsetAsync(s.slot, 0, (size_t)labels_bytes * sizeof(unsigned long long), ST);
    SEGCLIP_REQUIRE(e == hipSuccess, "%s: clearing the slots failed: %s", what, hipGetErrorString(e));
    hipLaunchKernelGGL(seg_cc_local_kernel<L>, grid, block, 0, ST, a);
    SEGCLIP_CHECK_LAUNCH("seg_sieve (local)");
    hipLaunchKernelGGL(seg_cc_merge_kernel<L>, grid, block, 0, ST, a);
    SEGCLIP_CHECK_LAUNCH("seg_sieve (merge)");
    hipLaunchKernelGGL(seg_cc_stats_kernel<false>, grid, block, 0, ST, a);
    SEGCLIP_CHECK_LAUNCH("seg_sieve (stats)");
    hipLaunchKernelGGL(seg_sieve_vote_kernel<L>, grid, block, 0, ST, s);
    SEGCLIP_CHECK_LAUNCH("seg_sieve (vote)");
    hipLaunchKernelGGL(seg_sieve_final_kernel<L>, grid, block, 0, ST, s);
    SEGCLIP_CHECK_LAUNCH("seg_sieve (final)");
    in = out;
  }
  return 0;
}

extern "C" int segclip_seg_sieve(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint8_t* labels,
                                 int64_t labels_bytes, int connectivity, int skip_label, int64_t min_area, int orphan_fill,
                                 int rounds, uint8_t* cleaned, int64_t cleaned_bytes, void* ws, int64_t ws_bytes, void* stream) {
  return seg_sieve_run<uint8_t>("seg_sieve", images, B, n_blocks, max_side, labels, labels_bytes, connectivity, skip_label, min_area,
                                orphan_fill, rounds, cleaned, cleaned_bytes, ws, ws_bytes, stream);
}

extern "C" int segclip_seg_sieve_wide(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint16_t* labels,
                                      int64_t labels_n, int connectivity, int skip_label, int64_t min_area, int orphan_fill,
                                      int rounds, uint16_t* cleaned, int64_t cleaned_n, void* ws, int64_t ws_bytes, void* stream) {
  return seg_sieve_run<uint16_t>("seg_sieve_wide", images, B, n_blocks, max_side, labels, labels_n, connectivity, skip_label, min_area,
                                 orphan_fill, rounds, cleaned, cleaned_n, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- superpixels (segment_superpixel.inc)
#define SEG_SP_MAX_CENTRES (1ll << 28)
struct SegSpWs { int64_t centres, acc, total; };
static SegSpWs seg_sp_ws(int64_t K_total) {
  const auto up = [](int64_t v) { return (v + 255) & ~255ll; };
  SegSpWs w;
  w.centres = 0;
  w.acc = up(K_total * 5 * 4);
  w.total = w.acc + up(K_total * 6 * 4);
  return w;
}

extern "C" int64_t segclip_seg_superpixels_ws_bytes(int64_t K_total) {
  SEG_REFUSE(K_total < 0 || K_total > SEG_SP_MAX_CENTRES, "seg_superpixels_ws_bytes: need 0 <= K_total <= 2^28");
  return seg_sp_ws(K_total).total;
}

extern "C" int segclip_seg_superpixels(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, int64_t step,
                                       int64_t compactness, int64_t iters, int32_t* ids, int64_t ids_n, int64_t K_total,
                                       int32_t* centres, void* ws, int64_t ws_bytes, void* stream) {
  SEGCLIP_REQUIRE(B >= 0 && n_blocks >= 0 && ids_n >= 0 && K_total >= 0 && ws_bytes >= 0, "seg_superpixels: sizes must not be negative");
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_blocks < (1ll << 31) && ids_n <= (1ll << 40), "seg_superpixels: size out of range");
  SEG_REFUSE(step < SEG_SP_MIN_STEP || step > SEG_SP_MAX_STEP, "seg_superpixels: a step of %lld, %d..%d supported", (long long)step,
             SEG_SP_MIN_STEP, SEG_SP_MAX_STEP);
  SEG_REFUSE(compactness < 1 || compactness > SEG_SP_MAX_COMPACT, "seg_superpixels: a compactness of %lld, 1..%d supported",
             (long long)compactness, SEG_SP_MAX_COMPACT);
  SEG_REFUSE(iters < 0 || iters > SEG_SP_MAX_T, "seg_superpixels: %lld iterations, 0..%d supported", (long long)iters, SEG_SP_MAX_T);
  SEG_REFUSE(max_side < 1 || max_side >= SEG_SP_LIMIT, "seg_superpixels: sides of 1..%d pixels supported, got a bound of %lld",
             SEG_SP_LIMIT - 1, (long long)max_side);
  SEG_REFUSE(K_total > SEG_SP_MAX_CENTRES, "seg_superpixels: %lld centres, at most 2^28 supported", (long long)K_total);
  const SegSpWs w = seg_sp_ws(K_total);
  SEG_REFUSE(ws_bytes < w.total, "seg_superpixels: the workspace has %lld bytes, segclip_seg_superpixels_ws_bytes asks for %lld",
             (long long)ws_bytes, (long long)w.total);
  if (B == 0 || n_blocks == 0 || K_total == 0) return 0;
  SEGCLIP_REQUIRE(images && ids, "seg_superpixels: images and ids are required");
  SEGCLIP_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "seg_superpixels: the workspace is required, 16-byte aligned");

  SegSpArgs a;
  char* base = static_cast<char*>(ws);
  a.images = images; a.ids = ids;
  a.centres = centres ? centres : reinterpret_cast<int32_t*>(base + w.centres);
  a.acc = reinterpret_cast<uint32_t*>(base + w.acc);
  a.ids_n = ids_n; a.K_total = K_total; a.n_blocks = n_blocks;
  a.B = (int)B; a.max_side = (int)max_side; a.S = (int)step; a.m2 = (int)(compactness * compactness);
  const dim3 grid((unsigned)n_blocks), block(SEG_SP_THREADS);
  hipLaunchKernelGGL(seg_sp_init_kernel, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_superpixels (init)");
  for (int t = 0; t < (int)iters; ++t) {
    hipLaunchKernelGGL(seg_sp_assign_kernel<false>, grid, block, 0, ST, a);
    SEGCLIP_CHECK_LAUNCH("seg_superpixels (assign)");
    hipLaunchKernelGGL(seg_sp_update_kernel, grid, block, 0, ST, a);
    SEGCLIP_CHECK_LAUNCH("seg_superpixels (update)");
  }
  hipLaunchKernelGGL(seg_sp_assign_kernel<true>, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_superpixels (ids)");
  return 0;
}

// ---------------------------------------------------------------- majority voting inside segments (segment_vote.inc)
#define SEG_VOTE_MAX_CELLS (1ll << 28)
struct SegVoteWs { int64_t cnt, win, total; };
static SegVoteWs seg_vote_ws(int64_t K_total, int64_t C) {
  const auto up = [](int64_t v) { return (v + 255) & ~255ll; };
  SegVoteWs w;
  w.cnt = 0;
  w.win = up(K_total * C * 4);
  w.total = w.win + up(K_total * 4);
  return w;
}

extern "C" int64_t segclip_seg_vote_ws_bytes(int64_t K_total, int64_t C) {
  SEG_REFUSE(K_total < 0 || C < 1 || C > SEG_WIDE_MAX_CLASSES || K_total > SEG_VOTE_MAX_CELLS || K_total * C > SEG_VOTE_MAX_CELLS,
             "seg_vote_ws_bytes: need 1 <= C <= %d and 0 <= K_total * C <= 2^28", SEG_WIDE_MAX_CLASSES);
  return seg_vote_ws(K_total, C).total;
}

// `what`: the entry's name in messages; labels_n, out_n: ELEMENTS of L
template <class L>
static int seg_vote_run(const char* what, const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_k, const L* labels,
                        int64_t labels_n, const int32_t* segments, int64_t segments_n, int64_t K_total, int64_t C, int min_share, L* out,
                        int64_t out_n, void* ws, int64_t ws_bytes, void* stream) {
  const char* unit = SegLabel<L>::unit;
  SEGCLIP_REQUIRE(B >= 0 && n_blocks >= 0 && labels_n >= 0 && segments_n >= 0 && K_total >= 0 && out_n >= 0 && ws_bytes >= 0,
                  "%s: sizes must not be negative", what);
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_blocks < (1ll << 31) && labels_n <= (1ll << 40), "%s: size out of range", what);
  SEG_REFUSE(C < 1 || C > SegLabel<L>::MAX_CLASSES, "%s: %lld classes, 1..%d supported", what, (long long)C, SegLabel<L>::MAX_CLASSES);
  SEG_REFUSE(min_share < 0 || min_share > 100, "%s: min_share is a percentage in 0..100, got %d", what, min_share);
  SEG_REFUSE(max_k < 1 || max_k > SEG_VOTE_MAX_K, "%s: 1..%d segments per image supported, got a bound of %lld", what, SEG_VOTE_MAX_K,
             (long long)max_k);
  SEG_REFUSE(K_total > SEG_VOTE_MAX_CELLS || K_total * C > SEG_VOTE_MAX_CELLS,
             "%s: %lld segments x %lld classes, at most 2^28 counters supported", what, (long long)K_total, (long long)C);
  const SegVoteWs w = seg_vote_ws(K_total, C);
  SEG_REFUSE(ws_bytes < w.total, "%s: the workspace has %lld bytes, segclip_seg_vote_ws_bytes asks for %lld", what, (long long)ws_bytes,
             (long long)w.total);
  if (B == 0 || n_blocks == 0 || K_total == 0) return 0;   // without a segment nobody votes and nothing is written
  SEGCLIP_REQUIRE(images && labels && segments && out, "%s: images, labels, segments and out are required", what);
  SEGCLIP_REQUIRE(out_n == labels_n && segments_n == labels_n, "%s: segments and out have the layout of labels: %lld %s, got %lld and %lld",
                  what, (long long)labels_n, unit, (long long)segments_n, (long long)out_n);
  SEGCLIP_REQUIRE(out + out_n <= labels || labels + labels_n <= out, "%s: out overlaps labels (the vote is out of place)", what);
  SEGCLIP_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace is required, 16-byte aligned", what);

  SegVoteArgs a;
  char* base = static_cast<char*>(ws);
  a.images = images; a.labels = labels; a.seg = segments; a.out = out;
  a.cnt = reinterpret_cast<int32_t*>(base + w.cnt);
  a.win = reinterpret_cast<int32_t*>(base + w.win);
  a.n = labels_n; a.K_total = K_total; a.n_blocks = n_blocks;
  a.B = (int)B; a.C = (int)C; a.max_k = (int)max_k; a.min_share = min_share;
  const dim3 grid((unsigned)n_blocks), block(SEG_VOTE_THREADS);
  const hipError_t e = hipMemsetAsync(a.cnt, 0, (size_t)(K_total * C) * sizeof(int32_t), ST);
  SEGCLIP_REQUIRE(e == hipSuccess, "%s: clearing the counts failed: %s", what, hipGetErrorString(e));
  hipLaunchKernelGGL(seg_vote_count_kernel<L>, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_vote (count)");
  hipLaunchKernelGGL(seg_vote_winner_kernel, dim3((unsigned)cdiv(K_total, SEG_VOTE_THREADS / 64)), block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_vote (winner)");
  hipLaunchKernelGGL(seg_vote_apply_kernel<L>, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_vote (apply)");
  return 0;
}

extern "C" int segclip_seg_vote(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_k, const uint8_t* labels,
                                int64_t labels_bytes, const int32_t* segments, int64_t segments_n, int64_t K_total, int64_t C,
                                int min_share, uint8_t* out, int64_t out_bytes, void* ws, int64_t ws_bytes, void* stream) {
  return seg_vote_run<uint8_t>("seg_vote", images, B, n_blocks, max_k, labels, labels_bytes, segments, segments_n, K_total, C, min_share,
                               out, out_bytes, ws, ws_bytes, stream);
}

extern "C" int segclip_seg_vote_wide(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_k, const uint16_t* labels,
                                     int64_t labels_n, const int32_t* segments, int64_t segments_n, int64_t K_total, int64_t C,
                                     int min_share, uint16_t* out, int64_t out_n, void* ws, int64_t ws_bytes, void* stream) {
  return seg_vote_run<uint16_t>("seg_vote_wide", images, B, n_blocks, max_k, labels, labels_n, segments, segments_n, K_total, C,
                                min_share, out, out_n, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- boundary bands and areas (segment_boundary.inc)
struct SegBdWs { int64_t pred_s, gt_s, total; };
static SegBdWs seg_bd_ws(int64_t pred_bytes, int64_t gt_bytes) {
  const auto up = [](int64_t v) { return (v + 255) & ~255ll; };
  SegBdWs w;
  w.pred_s = 0;
  w.gt_s = up(pred_bytes * 2);
  w.total = w.gt_s + up(gt_bytes * 2);
  return w;
}

extern "C" int64_t segclip_seg_boundary_ws_bytes(int64_t pred_bytes, int64_t gt_bytes) {
  SEG_REFUSE(pred_bytes < 0 || pred_bytes > (1ll << 40) || gt_bytes < 0 || gt_bytes > (1ll << 40),
             "seg_boundary_ws_bytes: need 0 <= pred_bytes, gt_bytes <= 2^40");
  return seg_bd_ws(pred_bytes, gt_bytes).total;
}

// byte ranges
static bool seg_bd_overlap(const void* pa, int64_t na, const void* pb, int64_t nb) {
  const char* a = static_cast<const char*>(pa);
  const char* b = static_cast<const char*>(pb);
  return a && b && na > 0 && nb > 0 && a < b + nb && b < a + na;
}

// `what`: the entry's name in messages; pred_bytes, gt_bytes: ELEMENTS of L (the uint8 entry's argument names).  The bands are
// bytes, one per element.
template <class L>
static int seg_boundary_run(const char* what, const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const L* pred,
                            int64_t pred_bytes, const L* gt, int64_t gt_bytes, int64_t C, int ignore_index, int reduce_zero_label,
                            uint8_t* pred_band, uint8_t* gt_band, int64_t* areas, void* ws, int64_t ws_bytes, void* stream) {
  constexpr int64_t EL = (int64_t)sizeof(L);
  SEGCLIP_REQUIRE(B >= 0 && n_blocks >= 0 && pred_bytes >= 0 && gt_bytes >= 0 && ws_bytes >= 0 && C >= 1,
                  "%s: sizes must not be negative, and C >= 1", what);
  SEGCLIP_REQUIRE(B <= (1 << 24) && n_blocks < (1ll << 31) && pred_bytes <= (1ll << 40) && gt_bytes <= (1ll << 40),
                  "%s: size out of range", what);
  SEGCLIP_REQUIRE(!areas || gt, "%s: areas need gt", what);
  SEGCLIP_REQUIRE(!gt_band || gt, "%s: gt_band needs gt", what);
  SEGCLIP_REQUIRE(!seg_bd_overlap(pred_band, pred_bytes, pred, pred_bytes * EL) && !seg_bd_overlap(pred_band, pred_bytes, gt, gt_bytes * EL) &&
                      !seg_bd_overlap(gt_band, gt_bytes, pred, pred_bytes * EL) && !seg_bd_overlap(gt_band, gt_bytes, gt, gt_bytes * EL) &&
                      !seg_bd_overlap(pred_band, pred_bytes, gt_band, gt_bytes),
                  "%s: a band output overlaps an input or the other band", what);
  SEG_REFUSE(C > SegLabel<L>::MAX_CLASSES, "%s: %lld classes, at most %d", what, (long long)C, SegLabel<L>::MAX_CLASSES);
  // the uint8 entry has always taken any ignore_index (one outside 0..255 ignores nothing)
  SEG_REFUSE(EL == 2 && (ignore_index < 0 || ignore_index > 65535), "%s: ignore_index is a 16-bit value, got %d", what, ignore_index);
  SEG_REFUSE(max_side < 1 || max_side >= SEG_BD_LIMIT, "%s: sides of 1..%d pixels supported, got a bound of %lld", what,
             SEG_BD_LIMIT - 1, (long long)max_side);
  const SegBdWs w = seg_bd_ws(pred_bytes, gt_bytes);
  SEG_REFUSE(ws_bytes < w.total, "%s: the workspace has %lld bytes, segclip_seg_boundary_ws_bytes asks for %lld", what,
             (long long)ws_bytes, (long long)w.total);
  if (B == 0 || n_blocks == 0) return 0;
  SEGCLIP_REQUIRE(images && pred, "%s: images and pred are required", what);
  SEGCLIP_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace is required, 16-byte aligned", what);
  if (!pred_band && !gt_band && !areas) return 0;  // nothing asked for

  SegBdArgs a;
  a.images = images; a.pred = pred; a.gt = gt; a.pred_n = pred_bytes; a.gt_n = gt ? gt_bytes : 0; a.n_blocks = n_blocks;
  a.B = (int)B; a.max_side = (int)max_side; a.C = (int)C; a.ignore_index = ignore_index; a.reduce_zero = reduce_zero_label ? 1 : 0;
  a.pred_band = pred_band; a.gt_band = gt_band; a.areas = reinterpret_cast<unsigned long long*>(areas);
  char* base = static_cast<char*>(ws);
  a.pred_s = reinterpret_cast<uint16_t*>(base + w.pred_s);
  a.gt_s = reinterpret_cast<uint16_t*>(base + w.gt_s);
  const dim3 grid((unsigned)n_blocks), block(256);
  hipLaunchKernelGGL(seg_bd_rows_kernel<L>, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_boundary (rows)");
  hipLaunchKernelGGL(seg_bd_band_kernel<L>, grid, block, 0, ST, a);
  SEGCLIP_CHECK_LAUNCH("seg_boundary (bands)");
  return 0;
}

extern "C" int segclip_seg_boundary(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint8_t* pred,
                                    int64_t pred_bytes, const uint8_t* gt, int64_t gt_bytes, int64_t C, int ignore_index,
                                    int reduce_zero_label, uint8_t* pred_band, uint8_t* gt_band, int64_t* areas, void* ws,
                                    int64_t ws_bytes, void* stream) {
  return seg_boundary_run<uint8_t>("seg_boundary", images, B, n_blocks, max_side, pred, pred_bytes, gt, gt_bytes, C, ignore_index,
                                   reduce_zero_label, pred_band, gt_band, areas, ws, ws_bytes, stream);
}

// The workspace is segclip_seg_boundary_ws_bytes of the element counts (2 bytes per element of pred and of gt).
extern "C" int segclip_seg_boundary_wide(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint16_t* pred,
                                         int64_t pred_n, const uint16_t* gt, int64_t gt_n, int64_t C, int ignore_index,
                                         int reduce_zero_label, uint8_t* pred_band, uint8_t* gt_band, int64_t* areas, void* ws,
                                         int64_t ws_bytes, void* stream) {
  return seg_boundary_run<uint16_t>("seg_boundary_wide", images, B, n_blocks, max_side, pred, pred_n, gt, gt_n, C, ignore_index,
                                    reduce_zero_label, pred_band, gt_band, areas, ws, ws_bytes, stream);
}

extern "C" int segclip_train_images_from_u8(const int64_t* images, int64_t B, int64_t out_h, int64_t out_w, const float* lut, float* out,
                                            void* stream) {
  SEGCLIP_REQUIRE(B >= 0 && B <= (1 << 24) && out_h >= 1 && out_w >= 1 && out_h < TF_LIMIT, "train_images_from_u8: sizes out of range");
  SEG_REFUSE(out_w > TF_MAX_OUT_W, "train_images_from_u8: an output of %lld columns, at most %d (coefficients and 33 rows of bytes in LDS)",
             (long long)out_w, TF_MAX_OUT_W);
  if (B == 0) return 0;
  SEGCLIP_REQUIRE(images && lut && out, "train_images_from_u8: images, lut and out are required");
  const int64_t bands = cdiv(out_h, TF_BAND);
  SEGCLIP_REQUIRE(B * bands < (1ll << 31), "train_images_from_u8: %lld images of %lld rows exceed one launch", (long long)B, (long long)out_h);
  static std::atomic<bool> raised[64];
  if (int rc = seg_raise_lds("train_images_from_u8", reinterpret_cast<const void*>(train_front_kernel), TF_LDS_BYTES, raised)) return rc;
  TrainFrontArgs a;
  a.images = images; a.lut = lut; a.out = out; a.out_h = (int)out_h; a.out_w = (int)out_w; a.bands = (int)bands;
  a.vec = (out_w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(train_front_kernel, dim3((unsigned)(B * bands)), dim3(256), TF_LDS_BYTES, ST, a);
  SEGCLIP_CHECK_LAUNCH("train_images_from_u8");
  return 0;
}

extern "C" int segclip_train_patch_labels(const int64_t* maps, int64_t B, int64_t size, int64_t patch, int64_t* out, void* stream) {
  SEGCLIP_REQUIRE(B >= 0 && B <= (1 << 24) && size >= 1 && size < TF_LIMIT && patch >= 1 && patch <= size && size % patch == 0,
                  "train_patch_labels: need 1 <= patch <= size < 2^15 and size a multiple of patch");
  if (B == 0) return 0;
  SEGCLIP_REQUIRE(maps && out, "train_patch_labels: maps and out are required");
  const int64_t pp = patch * patch;
  int shift = -1;  // log2(patch^2), or the division path
  if ((pp & (pp - 1)) == 0)
    for (shift = 0; (1ll << shift) < pp; ++shift) {}
  hipLaunchKernelGGL(train_labels_kernel, dim3((unsigned)B), dim3(256), 0, ST, maps, out, (int)size, (int)patch, shift);
  SEGCLIP_CHECK_LAUNCH("train_patch_labels");
  return 0;
}
