// Pixel-adaptive refinement of label maps (segment.hip): PAMR (Araslanov & Roth, CVPR 2020) as the zero-shot segmentation
// systems after SegCLIP apply it to their masks, for images of mixed sizes in one call, from the decoded uint8 picture and the
// uint8 label map that predict_raw / update_raw already hold on the device.  The reference ships no refinement: the definition
// is this project's (include/segclip_hip.h, segclip_seg_refine) and tests/pamr_reference.py restates it in fp64.
//   seg_refine_weights_kernel : the 8 D soft-max weights of every pixel from the raw bytes, once per call, and the image's
//                               256-bit map of the labels present
//   seg_refine_step_kernel    : one iteration over one chunk of 8 class planes; the first step reads the label bytes (no
//                               one-hot pass), the last one keeps a running (best value, best label) pair and, in an image's
//                               last chunk, writes the label and adds the mIoU areas
//   seg_refine_copy_kernel    : T = 0
// No (C, h, w) tensor: the planes of different classes never meet before the arg-max, so they go through the iterations 8 at a
// time in one fp32 buffer pair of 8 planes (two float4 per pixel), whatever C is.  Only the labels present in an image carry a plane that is
// not zero: they get compact ids in ascending label order (so the first maximum over the ids is the first over the labels), and
// the workgroups of a chunk beyond an image's label count exit at once.
// Traffic per pixel, iteration and chunk: 32 D bytes of weights (tap-major, so a wave's load of one tap is contiguous), 32
// bytes of planes written and 8 D taps of 32 bytes read (two float4: planes 0-3 of all pixels lie before planes 4-7, so that a
// wave's load of one tap is one run of memory); with dilations up to 32 a halo tile in LDS would not pay, and the taps of a
// picture's working set are served by L2 / the infinity cache.

#define SEG_REFINE_COLS SEGCLIP_SEG_REFINE_COLS        // int64 columns of one image row of the refine table (segclip_hip.h)
#define SEG_REFINE_TILE SEGCLIP_SEG_REFINE_TILE      // pixels of a workgroup: one per lane
#define SEG_REFINE_LIMIT SEGCLIP_SEG_SOURCE_LIMIT
#define SEG_REFINE_MAX_D SEGCLIP_SEG_REFINE_MAX_DILATIONS
#define SEG_REFINE_MAX_DIL SEGCLIP_SEG_REFINE_MAX_DILATION
#define SEG_REFINE_MAX_T SEGCLIP_SEG_REFINE_MAX_ITERS
#define SEG_REFINE_PLANES 8      // class planes of one chunk
enum { RF_SRC, RF_H, RF_W, RF_STRIDE, RF_LAB, RF_GT, RF_BLK };

struct SegRefineArgs {
  const int64_t* images;     // (B, SEG_REFINE_COLS)
  const uint8_t* labels;     // flat input labels
  uint8_t* out;              // flat refined labels, same offsets
  const uint8_t* gt;         // flat, or null
  unsigned long long* areas; // (3, C), or null
  float* probs;              // (C, h, w) of the single image, or null
  int64_t labels_bytes, gt_bytes, probs_floats;
  int B, C, D, max_side, ignore_index, reduce_zero;
  int dil[SEG_REFINE_MAX_D];
  float isd[3];              // 1 / std per SOURCE channel
  // workspace
  uint32_t* pres;            // (B, 8): bit b of an image's 256 = label b < C occurs in it
  float* wts;                // (8 D, labels_bytes): tap-major
  float* plane[2];           // (2, labels_bytes) float4 each: planes 0-3 of every pixel, then planes 4-7
  float* bestv;              // (labels_bytes)
  uint8_t* bestl;            // (labels_bytes)
};

// One image row, range-checked: the host entry cannot inspect device memory.
struct SegRefineImage { const uint8_t* src; int h, w; int64_t stride, lab, gt, total, p0; bool ok; };
__device__ __forceinline__ SegRefineImage seg_refine_image(const SegRefineArgs& A, int img) {
  const int64_t* D = A.images + (int64_t)img * SEG_REFINE_COLS;
  SegRefineImage I;
  I.src = reinterpret_cast<const uint8_t*>(D[RF_SRC]);
  const int64_t h = D[RF_H], w = D[RF_W];
  I.stride = D[RF_STRIDE]; I.lab = D[RF_LAB]; I.gt = D[RF_GT];
  I.ok = I.src != nullptr && h >= 1 && w >= 1 && h <= A.max_side && w <= A.max_side && h < SEG_REFINE_LIMIT && w < SEG_REFINE_LIMIT &&
         I.stride >= 3 * w && I.stride < (1ll << 31);
  I.h = (int)h; I.w = (int)w;
  I.total = I.ok ? h * w : 0;
  I.ok = I.ok && I.lab >= 0 && I.lab + I.total <= A.labels_bytes;
  I.p0 = ((int64_t)blockIdx.x - D[RF_BLK]) * SEG_REFINE_TILE;
  if (I.p0 < 0 || I.p0 >= I.total) I.ok = false;
  return I;
}

// neighbour n of a dilation: the 3 x 3 ring in (row, column) order without its centre
__device__ __forceinline__ void seg_refine_offset(int o, int& oy, int& ox) {
  const int j = o < 4 ? o : o + 1;
  oy = j / 3 - 1; ox = j % 3 - 1;
}
__device__ __forceinline__ int seg_refine_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---------------------------------------------------------------- weights and label presence
// a(p, n) = -(1/3) sum_c |x_c(p) - x_c(q_n)| / (1e-8 + 0.1 sigma_c(p)), w = softmax_n a.  x enters only through differences to
// the centre, (R(p) - R(q)) / std: the mean cancels, and the differences of bytes are integers, so sigma's two sums are formed
// exactly: var = (9 D sum d^2 - (sum d)^2) / (9 D (9 D - 1)) / std^2 with D zeros for the centre copies.  A flat region gives
// exactly sigma = 0, a = 0 and w = 1 / (8 D).
template <int D>
__global__ __launch_bounds__(256) void seg_refine_weights_kernel(SegRefineArgs A) {
  __shared__ int s_img;
  __shared__ uint32_t s_pres[8];
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_REFINE_COLS, RF_BLK, (int64_t)blockIdx.x);
  if (tid < 8) s_pres[tid] = 0;
  __syncthreads();
  const SegRefineImage I = seg_refine_image(A, s_img);
  if (!I.ok) return;  // block-uniform
  const int64_t pix = I.p0 + tid;
  const bool active = pix < I.total;
  if (active) {
    const int b = A.labels[I.lab + pix];
    if (b < A.C) atomicOr(&s_pres[b >> 5], 1u << (b & 31));
    const int y = (int)((uint32_t)pix / (uint32_t)I.w), x = (int)pix - y * I.w;
    const uint8_t* cp = I.src + (int64_t)y * I.stride + 3 * x;
    const int c0 = cp[0], c1 = cp[1], c2 = cp[2];
    int s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
    uint32_t ad[8 * D];  // |d| of the three channels of every tap
#pragma unroll
    for (int di = 0; di < D; ++di) {
      const int d = A.dil[di];
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        int oy, ox;
        seg_refine_offset(o, oy, ox);
        const uint8_t* q = I.src + (int64_t)seg_refine_clamp(y + d * oy, I.h - 1) * I.stride + 3 * seg_refine_clamp(x + d * ox, I.w - 1);
        const int d0 = c0 - (int)q[0], d1 = c1 - (int)q[1], d2 = c2 - (int)q[2];
        s1[0] += d0; s1[1] += d1; s1[2] += d2;
        s2[0] += d0 * d0; s2[1] += d1 * d1; s2[2] += d2 * d2;
        ad[di * 8 + o] = (uint32_t)abs(d0) | ((uint32_t)abs(d1) << 8) | ((uint32_t)abs(d2) << 16);
      }
    }
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int num = 9 * D * s2[c] - s1[c] * s1[c];   // <= 54 * 48 * 255^2 < 2^31
      const float sigma = A.isd[c] * sqrtf((float)num / (float)(9 * D * (9 * D - 1)));
      r[c] = A.isd[c] / (1e-8f + 0.1f * sigma);
    }
    float a[8 * D], mx = -INFINITY;
#pragma unroll
    for (int n = 0; n < 8 * D; ++n) {
      const float t = r[0] * (float)(ad[n] & 255u) + r[1] * (float)((ad[n] >> 8) & 255u) + r[2] * (float)(ad[n] >> 16);
      a[n] = -t / 3.f;
      mx = fmaxf(mx, a[n]);
    }
    float sum = 0.f;
#pragma unroll
    for (int n = 0; n < 8 * D; ++n) {
      a[n] = expf(a[n] - mx);
      sum += a[n];
    }
    float* wp = A.wts + I.lab + pix;
#pragma unroll
    for (int n = 0; n < 8 * D; ++n) wp[(int64_t)n * A.labels_bytes] = a[n] / sum;
  }
  __syncthreads();
  if (tid < 8 && s_pres[tid]) atomicOr(&A.pres[(int64_t)s_img * 8 + tid], s_pres[tid]);
}

// ---------------------------------------------------------------- one iteration of one chunk of planes
// m'_k(p) = sum_n w(p, n) m_k(q_n(p)) in the order of n, fused multiply-adds: a fixed order per pixel, no float atomics.
// FIRST: m_k(q) = [compact id of the label byte at q = 8 chunk + k].  LAST: no planes out; the running best over the chunks
// so far (chunk 0 starts from (0, input byte): a pixel without a positive plane keeps its byte), and in the image's last chunk
// the label, the areas and nothing else.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void seg_refine_step_kernel(SegRefineArgs A, int chunk, int parity) {
  __shared__ int s_img;
  __shared__ short s_lut[256];                 // label byte -> plane of this chunk, or -1
  __shared__ int s_ids[SEG_REFINE_PLANES];     // plane of this chunk -> label, or -1
  __shared__ int s_cnt[3 * SEG_MAX_CLASSES];
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_REFINE_COLS, RF_BLK, (int64_t)blockIdx.x);
  if (tid < SEG_REFINE_PLANES) s_ids[tid] = -1;
  __syncthreads();
  const SegRefineImage I = seg_refine_image(A, s_img);
  if (!I.ok) return;  // block-uniform
  // the image's labels in ascending order are its compact ids: lane t ranks label t
  int n_labels = 0, rank = 0;
  bool present;
  {
    const uint32_t* pw = A.pres + (int64_t)s_img * 8;
    const int word = tid >> 5;
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t v = pw[i];
      n_labels += __popc(v);
      if (i < word) rank += __popc(v);
      if (i == word) mine = v;
    }
    present = (mine >> (tid & 31)) & 1u;
    rank += __popc(mine & ((1u << (tid & 31)) - 1u));
  }
  const int n_chunks = n_labels > 0 ? (n_labels + SEG_REFINE_PLANES - 1) / SEG_REFINE_PLANES : 1;
  if (chunk >= n_chunks) return;  // block-uniform: an idle chunk
  const int slot = present ? rank - chunk * SEG_REFINE_PLANES : -1;
  const bool mine = slot >= 0 && slot < SEG_REFINE_PLANES;
  s_lut[tid] = (short)(mine ? slot : -1);
  if (mine) s_ids[slot] = tid;
  const bool final_chunk = LAST && chunk == n_chunks - 1;
  const bool score = final_chunk && A.gt && A.areas && I.gt >= 0 && I.gt + I.total <= A.gt_bytes;
  if (score)
    for (int i = tid; i < 3 * A.C; i += 256) s_cnt[i] = 0;
  __syncthreads();

  const int64_t pix = I.p0 + tid;
  if (pix < I.total) {
    const int y = (int)((uint32_t)pix / (uint32_t)I.w), x = (int)pix - y * I.w;
    const float* wp = A.wts + I.lab + pix;
    // planes 0-3 of all pixels, then planes 4-7: a wave's float4 load of one tap is one run of memory
    const float4* pin = reinterpret_cast<const float4*>(A.plane[parity]) + I.lab;
    const float4* pin_hi = pin + A.labels_bytes;
    const uint8_t* lin = A.labels + I.lab;
    float m[SEG_REFINE_PLANES];
#pragma unroll
    for (int k = 0; k < SEG_REFINE_PLANES; ++k) m[k] = 0.f;
    for (int di = 0; di < A.D; ++di) {
      const int d = A.dil[di];
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        int oy, ox;
        seg_refine_offset(o, oy, ox);
        const int q = seg_refine_clamp(y + d * oy, I.h - 1) * I.w + seg_refine_clamp(x + d * ox, I.w - 1);
        const float wn = wp[(int64_t)(di * 8 + o) * A.labels_bytes];
        if (FIRST) {
          const int k = s_lut[lin[q]];
#pragma unroll
          for (int kk = 0; kk < SEG_REFINE_PLANES; ++kk) m[kk] += k == kk ? wn : 0.f;
        } else {
          const float4 u = pin[q], v = pin_hi[q];
          m[0] = fmaf(wn, u.x, m[0]); m[1] = fmaf(wn, u.y, m[1]); m[2] = fmaf(wn, u.z, m[2]); m[3] = fmaf(wn, u.w, m[3]);
          m[4] = fmaf(wn, v.x, m[4]); m[5] = fmaf(wn, v.y, m[5]); m[6] = fmaf(wn, v.z, m[6]); m[7] = fmaf(wn, v.w, m[7]);
        }
      }
    }
    if (!LAST) {
      float4* po = reinterpret_cast<float4*>(A.plane[parity ^ 1]) + I.lab + pix;
      po[0] = make_float4(m[0], m[1], m[2], m[3]);
      po[A.labels_bytes] = make_float4(m[4], m[5], m[6], m[7]);
    } else {
      float bv = 0.f;
      int bl;
      if (chunk == 0) { bl = lin[pix]; } else { bv = A.bestv[I.lab + pix]; bl = A.bestl[I.lab + pix]; }
      const bool dense = A.probs && (int64_t)A.C * I.total <= A.probs_floats;
#pragma unroll
      for (int k = 0; k < SEG_REFINE_PLANES; ++k) {
        const int id = s_ids[k];
        if (id >= 0) {
          if (m[k] > bv) { bv = m[k]; bl = id; }
          if (dense) A.probs[(int64_t)id * I.total + pix] = m[k];
        }
      }
      if (final_chunk) {
        A.out[I.lab + pix] = (uint8_t)bl;
        if (score) seg_area_add(s_cnt, A.C, bl, A.gt[I.gt + pix], A.ignore_index, A.reduce_zero, 1);
      } else {
        A.bestv[I.lab + pix] = bv;
        A.bestl[I.lab + pix] = (uint8_t)bl;
      }
    }
  }
  if (score) {  // block-uniform
    __syncthreads();
    seg_area_flush(s_cnt, A.C, A.areas, tid);
  }
}

// ---------------------------------------------------------------- T = 0: the labels as they are, scored
__global__ __launch_bounds__(256) void seg_refine_copy_kernel(SegRefineArgs A) {
  __shared__ int s_img;
  __shared__ int s_cnt[3 * SEG_MAX_CLASSES];
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_REFINE_COLS, RF_BLK, (int64_t)blockIdx.x);
  __syncthreads();
  const SegRefineImage I = seg_refine_image(A, s_img);
  if (!I.ok) return;  // block-uniform
  const bool score = A.gt && A.areas && I.gt >= 0 && I.gt + I.total <= A.gt_bytes;
  if (score) {
    for (int i = tid; i < 3 * A.C; i += 256) s_cnt[i] = 0;
    __syncthreads();
  }
  const int64_t pix = I.p0 + tid;
  if (pix < I.total) {
    const int b = A.labels[I.lab + pix];
    A.out[I.lab + pix] = (uint8_t)b;
    if (A.probs && b < A.C && (int64_t)A.C * I.total <= A.probs_floats) A.probs[(int64_t)b * I.total + pix] = 1.f;
    if (score) seg_area_add(s_cnt, A.C, b, A.gt[I.gt + pix], A.ignore_index, A.reduce_zero, 1);
  }
  if (score) {
    __syncthreads();
    seg_area_flush(s_cnt, A.C, A.areas, tid);
  }
}
