// Front end of the zero-shot evaluation (segment.hip): decoded uint8 images -> the vision tower's input windows.  Replaces the
// test pipeline's Resize(keep_ratio=True) + Normalize(mean, std, to_rgb=True) of the reference
// (seg_segmentation/configs/_base_/datasets/pascal_voc12.py:19-34, done there by mmcv / cv2) and the window slicing of mmseg's
// slide_inference: every window pixel is resized bilinearly from its image and normalised on the way, so neither the resized
// image nor a float copy of the source exists.
//
// Bound: HBM writes, 12 bytes per window pixel.  The source bytes are not staged in LDS: the 256 pixels of a wave lie in at
// most two window rows, hence in at most four source rows of a few hundred contiguous bytes each, which the four taps of a
// pixel and of its neighbours re-read from L1 (12 byte loads per pixel, every cache line fetched from L2 / HBM about once); an
// LDS stage would add a barrier and a second pass over the same bytes without removing a byte of the bound.  Measured
// (profiles/seg_frontend.txt): 1.28 TB/s written, 0.16 of the peak - the byte loads, not the writes, set the time; it is 0.6 %
// of an evaluation call, so the simple form stays (DESIGN.md section 8 names the next step).

#define SEG_FE_COLS SEGCLIP_SEG_SOURCE_COLS    // int64 columns of one image row of the source table (segclip_hip.h)
#define SEG_FE_VIEW_COLS SEGCLIP_SEG_SOURCE_VIEW_COLS  // ... of the view entry's table: the same row and a flag word (bit 0 horizontal, bit 1 vertical flip)
#define SEG_FE_PPL 4     // consecutive window pixels of a lane: one 16-byte store per channel
#define SEG_FE_LIMIT SEGCLIP_SEG_SOURCE_LIMIT
enum { FE_SRC, FE_H, FE_W, FE_STRIDE, FE_NET_H, FE_NET_W, FE_FLAGS };

struct SegFrontArgs {
  const int64_t* images;   // (B, SEG_FE_COLS), or (B, SEG_FE_VIEW_COLS) for the view kernel
  const int32_t* windows;  // (n_windows, 3): image, y0, x0
  float* out;              // (n_windows, 3, win_h, win_w)
  int B, win_h, win_w, upr, blocks_per_window, reverse, vec;
  float mean[3], inv_std[3];
};

// Destination d of m along an axis of n source pixels: the source coordinate is the rational ((2 d + 1) n - m) / (2 m),
// cv2 INTER_LINEAR's and upsample_bilinear2d(align_corners=False)'s, split in integers into q = its floor + 1 (so that q >= 0:
// the coordinate is > -1) and the remainder r of 2 m.  n, m < 2^15: every product stays below 2^31.
__device__ __forceinline__ void seg_fe_coord(int d, int n, int m, int& q, int& r) {
  const unsigned num = (unsigned)((2 * d + 1) * n + m), den = (unsigned)(2 * m);
  q = (int)(num / den);
  r = (int)(num - (unsigned)q * den);
}

// (q, r) -> taps s0 <= s1 and the weight f of s1; outside [0, n - 1] the edge pixel alone
__device__ __forceinline__ void seg_fe_taps(int q, int r, int n, int m, int& s0, int& s1, float& f) {
  s0 = q - 1;
  f = (float)r / (float)(2 * m);
  if (s0 < 0) { s0 = 0; f = 0.f; }
  if (s0 >= n - 1) { s0 = n - 1; f = 0.f; }
  s1 = s0 + 1 < n - 1 ? s0 + 1 : n - 1;
}

// One operation order for every pixel, whichever window or store path asks for it: the fused multiply-adds are written out,
// and nothing else here can be contracted (a window of predict_raw and the same pixels of preprocess agree bit for bit).
__device__ __forceinline__ float seg_fe_blend(float a, float b, float c, float d, float fx, float fy) {
  const float top = fmaf(b, fx, a * (1.f - fx));
  const float bot = fmaf(d, fx, c * (1.f - fx));
  return fmaf(bot, fy, top * (1.f - fy));
}

// A lane owns SEG_FE_PPL consecutive pixels of one window row, a workgroup 256 consecutive such units of one window; a wave
// stores 1 KiB of consecutive floats per channel.  Every table entry is range-checked here (the host entry cannot inspect
// device memory): a window that fails is zero-filled, and a source byte is read only inside the (h, w) the row states.
// VIEWS: the rows carry a flag word, and window pixel (Y, X) of a flipped view reads the resized image at (Y, W - 1 - X) and /
// or (H - 1 - Y, X): mmseg flips after the resize, so the geometry is the unflipped image's.  The coordinates are exact
// integers whichever way they are reached: flags 0 give the bytes of the plain kernel.
template <bool VIEWS>
__global__ __launch_bounds__(256) void seg_front_kernel(SegFrontArgs A) {
  const int tid = threadIdx.x;
  const int64_t k = blockIdx.x / A.blocks_per_window;
  const int64_t unit = (int64_t)(blockIdx.x % A.blocks_per_window) * 256 + tid;
  if (unit >= (int64_t)A.win_h * A.upr) return;
  const int y = (int)((uint32_t)unit / (uint32_t)A.upr);
  const int xq = ((int)unit - y * A.upr) * SEG_FE_PPL;

  const int img = A.windows[3 * k], y0 = A.windows[3 * k + 1], x0 = A.windows[3 * k + 2];
  bool ok = img >= 0 && img < A.B;
  const uint8_t* src = nullptr;
  int64_t stride = 0;
  int h = 1, w = 1, H = 1, W = 1, flags = 0;
  if (ok) {
    const int64_t* D = A.images + (int64_t)img * (VIEWS ? SEG_FE_VIEW_COLS : SEG_FE_COLS);
    if (VIEWS) flags = (int)(D[FE_FLAGS] & 3);
    const int64_t h64 = D[FE_H], w64 = D[FE_W], H64 = D[FE_NET_H], W64 = D[FE_NET_W];
    src = reinterpret_cast<const uint8_t*>(D[FE_SRC]);
    stride = D[FE_STRIDE];
    ok = src != nullptr && h64 >= 1 && w64 >= 1 && H64 >= 1 && W64 >= 1 && h64 < SEG_FE_LIMIT && w64 < SEG_FE_LIMIT &&
         H64 < SEG_FE_LIMIT && W64 < SEG_FE_LIMIT && stride >= 3 * w64 && y0 >= 0 && x0 >= 0 && (int64_t)y0 + A.win_h <= H64 &&
         (int64_t)x0 + A.win_w <= W64;
    if (ok) { h = (int)h64; w = (int)w64; H = (int)H64; W = (int)W64; }
  }

  float v[3][SEG_FE_PPL];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int p = 0; p < SEG_FE_PPL; ++p) v[c][p] = 0.f;
  if (ok) {  // block-uniform
    int qy, ry, ya, yb, qx, rx;
    float fy;
    seg_fe_coord((flags & 2) ? H - 1 - (y0 + y) : y0 + y, h, H, qy, ry);
    seg_fe_taps(qy, ry, h, H, ya, yb, fy);
    const uint8_t* ra = src + (int64_t)ya * stride;
    const uint8_t* rb = src + (int64_t)yb * stride;
    seg_fe_coord(x0 + xq, w, W, qx, rx);
    const int step_q = (2 * w) / (2 * W), step_r = 2 * w - step_q * 2 * W;  // the coordinate's advance per destination pixel
#pragma unroll
    for (int p = 0; p < SEG_FE_PPL; ++p) {
      if (xq + p < A.win_w) {
        int xa, xb;
        float fx;
        if (flags & 1) seg_fe_coord(W - 1 - (x0 + xq + p), w, W, qx, rx);
        seg_fe_taps(qx, rx, w, W, xa, xb, fx);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int cs = A.reverse ? 2 - c : c;
          const float r = seg_fe_blend((float)ra[3 * xa + cs], (float)ra[3 * xb + cs], (float)rb[3 * xa + cs], (float)rb[3 * xb + cs],
                                       fx, fy);
          v[c][p] = (r - A.mean[c]) * A.inv_std[c];
        }
      }
      qx += step_q;
      rx += step_r;
      if (rx >= 2 * W) { rx -= 2 * W; ++qx; }
    }
  }

  const int64_t plane = (int64_t)A.win_h * A.win_w;
  float* o = A.out + (k * 3) * plane + (int64_t)y * A.win_w + xq;
  if (A.vec) {  // win_w % 4 == 0 and out on a 16-byte boundary: every unit is whole and aligned
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      for (int p = 0; p < SEG_FE_PPL && xq + p < A.win_w; ++p) o[c * plane + p] = v[c][p];
  }
}
