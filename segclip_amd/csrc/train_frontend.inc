// Front end of training (segment.hip): decoded uint8 images and int32 segment maps -> the model's `image` and `image_seg`.
// Replaces the CPU pipeline of the reference's data loader (dataloaders/rawimage_util.py:33-53 RawImageExtractor: Pillow BICUBIC
// resized_crop or Resize + CenterCrop, ToTensor, Normalize; :100-144 get_felzenszwalb_from_cache).  Both are integer algorithms
// and are reproduced to the last bit.
//
// (a) train_front_kernel restates Pillow's ImagingResample for 8-bit pixels: per axis the bicubic coefficients are formed in
// fp64 (precompute_coeffs), rounded to 22-bit integers (normalize_coeffs_8bpc), the horizontal pass accumulates in int32 and
// rounds to bytes, the vertical pass does the same on those bytes.  The output value is lut[byte][c]: no floating-point
// arithmetic touches a pixel.  The crop box is the whole image for the filter (crop() then resize(), torchvision's
// resized_crop), so the taps clamp at the box's edges.
//
// A workgroup owns one image's band of TF_BAND rows of the output window.  It writes both axes' integer coefficients into LDS
// (only the window's columns and the band's rows), then walks the band in sub-bands: the horizontal pass over exactly the
// source rows the sub-band's vertical taps reach goes into a byte tile in LDS, the vertical pass reads the tile.  The sub-band
// is the whole band while its source rows fit the tile (scales up to about 4 at 224 columns) and shrinks beyond that, down to
// one row at scale 8.  Design bound: the crop bytes read once + 12 bytes written per output pixel; the horizontal pass reads
// the source with byte loads (each row segment again from L1 for every tap), which a dword path would cut by four.
// Unmeasured until profiles/train_frontend.txt says otherwise.

#define TF_COLS SEGCLIP_TRAIN_SOURCE_COLS        // int64 columns of one image row of the table (segclip_hip.h)
#define TF_BAND 16        // output rows of a workgroup: one patch row of the 16-pixel patches
#define TF_MAX_SCALE SEGCLIP_TRAIN_MAX_SCALE    // crop side / resized side, per axis
#define TF_MAX_TAPS 33    // (int)ceil(2 * 8) * 2 + 1
#define TF_MAX_OUT_W SEGCLIP_TRAIN_MAX_OUT_W  // columns of the output window: the coefficient table and 33 tile rows fit the LDS
#define TF_LDS_BYTES (80 * 1024)  // two workgroups per CU
#define TF_PBITS 22       // Pillow's PRECISION_BITS = 32 - 8 - 2
#define TF_LIMIT SEGCLIP_SEG_SOURCE_LIMIT
enum { TF_SRC, TF_H, TF_W, TF_STRIDE, TF_X0, TF_Y0, TF_BW, TF_BH, TF_RW, TF_RH, TF_OX, TF_OY, TF_FLAGS };

struct TrainFrontArgs {
  const int64_t* images;  // (B, TF_COLS)
  const float* lut;       // (256, 3)
  float* out;             // (B, 3, out_h, out_w)
  int out_h, out_w, bands, vec;
};

__device__ __forceinline__ double tf_bicubic(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Pillow's coefficients of destination xx along an axis of n_in source and n_out destination pixels: the first tap and the
// tap count into lo / cnt, the integer weights into k[0 .. cnt), cnt <= ks = Pillow's ksize.  Two sweeps over the taps (the sum, then the weights) instead
// of Pillow's stored doubles: the filter is a pure function, so the values are the same.
__device__ __forceinline__ void tf_coeffs(int xx, int n_in, int n_out, int ks, int* k, int& lo, int& cnt) {
#pragma clang fp contract(off)
  const double scale = (double)n_in / (double)n_out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs, ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > n_in) xmax = n_in;
  xmax -= xmin;
  if (xmax > ks) xmax = ks;  // cannot happen (xmax - xmin <= 2 support + 1 <= ksize); keeps the LDS write inside its row regardless
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += tf_bicubic((x + xmin - center + 0.5) * ss);
  for (int x = 0; x < xmax; ++x) {
    double w = tf_bicubic((x + xmin - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << TF_PBITS)) : (int)(0.5 + w * (double)(1 << TF_PBITS));
  }
  lo = xmin;
  cnt = xmax;
}

// Pillow's ksize = (int)ceil(support) * 2 + 1 with support = 2 max(in / out, 1), in integers (2 in / out is an integer or at
// least 2^-15 away from one, so the double's ceiling is the rational's): 5 .. TF_MAX_TAPS at scale <= 8
__device__ __forceinline__ int tf_ksize(int64_t n_in, int64_t n_out) {
  return n_in <= n_out ? 5 : 2 * (int)((2 * n_in + n_out - 1) / n_out) + 1;
}

__device__ __forceinline__ int tf_clip8(int acc) {
  const int v = acc >> TF_PBITS;  // arithmetic
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// LDS: lut (768 floats) | ky (TF_BAND * ksy) | ylo, ycnt (TF_BAND each) | xlo, xcnt (out_w each) | kx (out_w * ksx) | byte tile
__global__ __launch_bounds__(256) void train_front_kernel(TrainFrontArgs A) {
  extern __shared__ int tf_lds[];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / A.bands;
  const int j0 = (blockIdx.x % A.bands) * TF_BAND;                     // first window row of the band, before any flip
  const int nj = A.out_h - j0 < TF_BAND ? A.out_h - j0 : TF_BAND;
  const int64_t plane = (int64_t)A.out_h * A.out_w;
  float* out = A.out + (int64_t)b * 3 * plane;
  const int upr = (A.out_w + 3) / 4;  // 4-pixel units per row

  const int64_t* D = A.images + (int64_t)b * TF_COLS;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(D[TF_SRC]);
  const int64_t h = D[TF_H], w = D[TF_W], stride = D[TF_STRIDE], x0 = D[TF_X0], y0 = D[TF_Y0], bw = D[TF_BW], bh = D[TF_BH];
  const int64_t RW = D[TF_RW], RH = D[TF_RH], ox = D[TF_OX], oy = D[TF_OY], flags = D[TF_FLAGS];
  const bool ok = src != nullptr && h >= 1 && w >= 1 && h < TF_LIMIT && w < TF_LIMIT && stride >= 3 * w && x0 >= 0 && y0 >= 0 &&
                  bw >= 1 && bh >= 1 && x0 + bw <= w && y0 + bh <= h && RW >= 1 && RH >= 1 && RW < TF_LIMIT && RH < TF_LIMIT &&
                  ox >= 0 && oy >= 0 && ox + A.out_w <= RW && oy + A.out_h <= RH && bw <= TF_MAX_SCALE * RW &&
                  bh <= TF_MAX_SCALE * RH && flags >= 0 && flags <= 3;
  if (!ok) {  // block-uniform: the band is zero-filled
    for (int u = tid; u < nj * A.out_w; u += 256) {
      const int64_t o = (int64_t)(j0 + u / A.out_w) * A.out_w + u % A.out_w;
      out[o] = 0.f; out[plane + o] = 0.f; out[2 * plane + o] = 0.f;
    }
    return;
  }
  const bool fh = flags & 1, fv = flags & 2;
  const int ksx = tf_ksize(bw, RW), ksy = tf_ksize(bh, RH);  // row strides of the coefficient tables

  float* s_lut = reinterpret_cast<float*>(tf_lds);
  int* s_ky = tf_lds + 768;
  int* s_ylo = s_ky + TF_BAND * ksy;
  int* s_ycnt = s_ylo + TF_BAND;
  int* s_xlo = s_ycnt + TF_BAND;
  int* s_xcnt = s_xlo + A.out_w;
  int* s_kx = s_xcnt + A.out_w;
  uint8_t* s_tile = reinterpret_cast<uint8_t*>(s_kx + A.out_w * ksx);
  const int row_bytes = (3 * A.out_w + 3) & ~3;
  const int tile_rows = (int)((TF_LDS_BYTES - (int64_t)(s_tile - reinterpret_cast<uint8_t*>(tf_lds))) / row_bytes);  // >= 33 (host)

  for (int i = tid; i < 768; i += 256) s_lut[i] = A.lut[i];
  for (int i = tid; i < A.out_w + nj; i += 256) {
    if (i < A.out_w) tf_coeffs((int)ox + i, (int)bw, (int)RW, ksx, s_kx + i * ksx, s_xlo[i], s_xcnt[i]);
    else tf_coeffs((int)oy + j0 + (i - A.out_w), (int)bh, (int)RH, ksy, s_ky + (i - A.out_w) * ksy, s_ylo[i - A.out_w], s_ycnt[i - A.out_w]);
  }
  __syncthreads();

  const uint8_t* box = src + y0 * stride + 3 * x0;  // the crop's first byte; rows `stride` apart
  for (int ja = 0; ja < nj;) {
    // the sub-band [ja, jb): as many rows as the tile holds source rows for (first and last taps grow with the row)
    const int ylo = s_ylo[ja];
    int jb = ja + 1;
    while (jb < nj && s_ylo[jb] + s_ycnt[jb] - ylo <= tile_rows) ++jb;
    int nrows = s_ylo[jb - 1] + s_ycnt[jb - 1] - ylo;
    if (nrows > tile_rows) nrows = tile_rows;  // cannot happen: one row has at most 33 taps

    // horizontal pass: source rows ylo .. ylo + nrows of the crop, the window's columns -> bytes
    for (int u = tid; u < nrows * A.out_w; u += 256) {
      const int r = u / A.out_w, i = u - r * A.out_w;
      const int cnt = s_xcnt[i];
      const int* k = s_kx + i * ksx;
      const uint8_t* p = box + (int64_t)(ylo + r) * stride + 3 * s_xlo[i];
      int a0 = 1 << (TF_PBITS - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < cnt; ++t) {
        const int kk = k[t];
        a0 += (int)p[3 * t] * kk;
        a1 += (int)p[3 * t + 1] * kk;
        a2 += (int)p[3 * t + 2] * kk;
      }
      uint8_t* q = s_tile + r * row_bytes + 3 * i;
      q[0] = (uint8_t)tf_clip8(a0); q[1] = (uint8_t)tf_clip8(a1); q[2] = (uint8_t)tf_clip8(a2);
    }
    __syncthreads();

    // vertical pass: a lane owns 4 consecutive output pixels of one row
    for (int u = tid; u < (jb - ja) * upr; u += 256) {
      const int jj = ja + u / upr, xq = (u % upr) * 4;
      const int cnt = s_ycnt[jj];
      const int* k = s_ky + jj * ksy;
      const uint8_t* col = s_tile + (s_ylo[jj] - ylo) * row_bytes;
      float v[3][4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int x = xq + p < A.out_w ? xq + p : A.out_w - 1;
        const int i = fh ? A.out_w - 1 - x : x;
        int a0 = 1 << (TF_PBITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < cnt; ++t) {
          const int kk = k[t];
          const uint8_t* q = col + t * row_bytes + 3 * i;
          a0 += (int)q[0] * kk;
          a1 += (int)q[1] * kk;
          a2 += (int)q[2] * kk;
        }
        v[0][p] = s_lut[3 * tf_clip8(a0)];
        v[1][p] = s_lut[3 * tf_clip8(a1) + 1];
        v[2][p] = s_lut[3 * tf_clip8(a2) + 2];
      }
      const int y = fv ? A.out_h - 1 - (j0 + jj) : j0 + jj;
      float* o = out + (int64_t)y * A.out_w + xq;
      if (A.vec) {  // out_w % 4 == 0 and out on a 16-byte boundary
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          for (int p = 0; p < 4 && xq + p < A.out_w; ++p) o[c * plane + p] = v[c][p];
      }
    }
    __syncthreads();  // the tile is rewritten by the next sub-band
    ja = jb;
  }
}

// (b) get_felzenszwalb_from_cache for a batch: crop (or the whole map), flips, ATen's `nearest` resample to size x size, the
// integer mean of every patch x patch tile.  One workgroup per image, one wave per patch in turn; the kernel is tiny.
#define TL_COLS SEGCLIP_TRAIN_MAP_COLS  // int64 columns of one map row of the table (segclip_hip.h)
enum { TL_SRC, TL_H, TL_W, TL_STRIDE, TL_X0, TL_Y0, TL_X1, TL_Y1, TL_FLAGS };

// upsample_nearest's source index: both the quotient and the product in fp32
__device__ __forceinline__ int tl_nearest(int d, float scale, int n_in) {
#pragma clang fp contract(off)
  const int s = (int)floorf((float)d * scale);
  return s < n_in - 1 ? s : n_in - 1;
}

__global__ __launch_bounds__(256) void train_labels_kernel(const int64_t* __restrict__ maps, int64_t* __restrict__ out, int size,
                                                           int patch, int shift) {
  __shared__ int s_neg;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int P = size / patch, pp = patch * patch;
  int64_t* o = out + (int64_t)b * P * P;
  const int64_t* D = maps + (int64_t)b * TL_COLS;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(D[TL_SRC]);
  const int64_t h = D[TL_H], w = D[TL_W], stride = D[TL_STRIDE], flags = D[TL_FLAGS];
  int64_t x0 = D[TL_X0], y0 = D[TL_Y0], x1 = D[TL_X1], y1 = D[TL_Y1];
  bool ok = src != nullptr && (reinterpret_cast<uintptr_t>(src) & 3) == 0 && h >= 1 && w >= 1 && h < TF_LIMIT && w < TF_LIMIT &&
            stride >= 4 * w && (stride & 3) == 0 && flags >= 0 && flags <= 3;
  if (ok && (x1 - x0 < 2 || y1 - y0 < 2)) { x0 = 0; y0 = 0; x1 = w; y1 = h; }  // rawimage_util.py:122: the whole map
  ok = ok && x0 >= 0 && y0 >= 0 && x1 <= w && y1 <= h && x1 > x0 && y1 > y0;
  if (tid == 0) s_neg = ok ? 0 : 1;
  __syncthreads();
  if (ok) {
    const int cw = (int)(x1 - x0), ch = (int)(y1 - y0);
    const float sx = (float)cw / (float)size, sy = (float)ch / (float)size;
    const bool fh = flags & 1, fv = flags & 2;
    for (int q = wave; q < P * P; q += 4) {
      const int py = q / P, px = q - py * P;
      long long sum = 0;
      int neg = 0;
      for (int e = lane; e < pp; e += 64) {
        const int ey = e / patch, ex = e - ey * patch;
        int yy = tl_nearest(py * patch + ey, sy, ch), xx = tl_nearest(px * patch + ex, sx, cw);
        if (fv) yy = ch - 1 - yy;
        if (fh) xx = cw - 1 - xx;
        const int v = *reinterpret_cast<const int32_t*>(src + (y0 + yy) * stride + 4 * (x0 + xx));
        neg |= v < 0;
        sum += v;
      }
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        sum += __shfl_xor(sum, m, 64);
        neg |= __shfl_xor(neg, m, 64);
      }
      if (lane == 0) {
        o[q] = shift >= 0 ? (int64_t)(sum >> shift) : (int64_t)(sum / pp);
        if (neg) atomicOr(&s_neg, 1);
      }
    }
  }
  __syncthreads();
  if (s_neg)  // a row the device refuses, or a negative label (the mean of the reference truncates towards zero there): all -1
    for (int q = tid; q < P * P; q += 256) o[q] = -1;
}
