// Rendering of segmentation results (segment.hip): what the reference's demo draws (seg_segmentation/evaluation/vit_seg.py,
// show_result :286-377), for images of mixed sizes in one launch each, without leaving the device.
//   seg_groups_kernel : the group map at every image's output size (get_attn_maps :144-200 + the resize and arg-max of
//                       :359-362), without the (G, H, W) and (G, oh, ow) intermediates
//   seg_blend_kernel  : the overlay of blend_result (:258-284) in numpy's fp64 arithmetic, and optionally the per-index pixel
//                       count, sum of y and sum of x that seg2coord (:100-115) averages
// Both are bandwidth-bound and reuse the descriptor-table scheme of segment_tile.inc: the workgroups of all images are numbered
// through, a table row names an image's first workgroup, and every row is range-checked on the device.

#define SEG_RENDER_TILE SEGCLIP_SEG_RENDER_TILE         // pixels of a workgroup (a lane owns 4 consecutive ones)
#define SEG_RENDER_PPL 4
#define SEG_RENDER_SOFT_FLOATS 6400  // LDS budget of the staged soft assignment: 8 x 28 x 28 floats fit
#define SEG_BLEND_COLS SEGCLIP_SEG_BLEND_COLS             // int64 columns of one image row of the blend table (segclip_hip.h)
#define SEG_BLEND_LIMIT SEGCLIP_SEG_SOURCE_LIMIT
#define SEG_MAX_PALETTE 256
enum { BL_SRC, BL_H, BL_W, BL_STRIDE, BL_MAP, BL_OUT, BL_BLK };

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- group maps at the output size
struct SegGroupsArgs {
  const float* soft;       // flat; the one window of image i is the (G, gh * gw) planes at soft + row[SI_SOFT]
  const int64_t* images;   // (B, SEG_IMG_COLS), the table of segclip_seg_label_map_rescaled
  int64_t soft_floats, groups_bytes;
  int B, G;
  uint8_t* groups;         // flat
};

// One channel of the soft assignment at network pixel (Y, X): the four grid values blended as seg_pixel_group blends them.
struct SegGridTaps { int o00, o01, o10, o11; float ly, lx; };
__device__ __forceinline__ float seg_grid_value(const float* p, const SegGridTaps& t) {
  const float hy = 1.f - t.ly, hx = 1.f - t.lx;
  return hy * (hx * p[t.o00] + t.lx * p[t.o01]) + t.ly * (hx * p[t.o10] + t.lx * p[t.o11]);
}

// A workgroup owns SEG_RENDER_TILE consecutive pixels of one image's flat (oh, ow) output, a lane four of them (one dword
// store: the host aligns every image's offset to 4).  The tile's output rows reach a few rows of the network size and those a
// few rows of the grid: these grid rows of all G channels are staged in LDS when they fit the budget (the whole window of
// 8 x 28 x 28 does), otherwise the lanes read the global array.
__global__ __launch_bounds__(256) void seg_groups_kernel(SegGroupsArgs A) {
  __shared__ float s_soft[SEG_RENDER_SOFT_FLOATS];
  __shared__ int s_img;
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_IMG_COLS, SI_BLK, (int64_t)blockIdx.x);
  __syncthreads();

  const int64_t* D = A.images + (int64_t)s_img * SEG_IMG_COLS;
  const int64_t H = D[SI_H], W = D[SI_W], oh = D[SI_OH], ow = D[SI_OW], gh = D[SI_GH], gw = D[SI_GW];
  const int64_t soft_off = D[SI_SOFT], grp_off = D[SI_LAB];
  const int64_t lim = 1ll << 30;
  // exactly one window, which is the image: its soft assignment is the image's
  bool ok = D[SI_COUNT] == 1 && D[SI_WIN_H] == H && D[SI_WIN_W] == W && H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && gh >= 1 &&
            gw >= 1 && H < lim && W < lim && oh < lim && ow < lim && gh < lim && gw < lim && gh * gw * A.G < lim &&
            oh * ow < (1ll << 31);
  ok = ok && soft_off >= 0 && soft_off + A.G * gh * gw <= A.soft_floats;
  const int64_t total = ok ? oh * ow : 0;
  ok = ok && grp_off >= 0 && grp_off + total <= A.groups_bytes;
  const int64_t p0 = ((int64_t)blockIdx.x - D[SI_BLK]) * SEG_RENDER_TILE;
  if (!ok || p0 < 0 || p0 >= total) return;  // block-uniform

  const float ry = (float)H / (float)oh, rx = (float)W / (float)ow;
  const float sy = (float)gh / (float)H, sx = (float)gw / (float)W;
  // grid rows of this tile: the taps are monotone in the destination index, so the first row's first tap and the last row's
  // second tap bound them
  int g_lo, g_hi;
  {
    const int64_t p_last = p0 + SEG_RENDER_TILE - 1 < total - 1 ? p0 + SEG_RENDER_TILE - 1 : total - 1;
    int n_lo, n_hi, t;
    float l;
    seg_axis_taps((int)((uint32_t)p0 / (uint32_t)ow), ry, (int)H, n_lo, t, l);
    seg_axis_taps((int)((uint32_t)p_last / (uint32_t)ow), ry, (int)H, t, n_hi, l);
    seg_axis_taps(n_lo, sy, (int)gh, g_lo, t, l);
    seg_axis_taps(n_hi, sy, (int)gh, t, g_hi, l);
  }
  const int rows = g_hi - g_lo + 1, igw = (int)gw;
  const bool staged = (int64_t)A.G * rows * igw <= SEG_RENDER_SOFT_FLOATS;
  const float* src = A.soft + soft_off;
  if (staged) {
    const int per = rows * igw;
    for (int i = tid; i < A.G * per; i += 256) s_soft[i] = src[(int64_t)(i / per) * (gh * gw) + (int64_t)g_lo * igw + i % per];
  }
  __syncthreads();
  const float* base = staged ? (const float*)s_soft : src;
  const int plane = staged ? rows * igw : (int)(gh * gw);
  const int row0 = staged ? g_lo : 0;

  const int64_t pq = p0 + (int64_t)tid * SEG_RENDER_PPL;
  if (pq >= total) return;
  uint32_t pack = 0;
  for (int q = 0; q < SEG_RENDER_PPL; ++q) {
    const int64_t p = pq + q;
    if (p >= total) break;
    const int y = (int)((uint32_t)p / (uint32_t)ow), x = (int)((uint32_t)p % (uint32_t)ow);
    int ya, yb, xa, xb;
    float ly, lx;
    seg_axis_taps(y, ry, (int)H, ya, yb, ly);
    seg_axis_taps(x, rx, (int)W, xa, xb, lx);
    // a tap of weight 0 adds 0 * (a finite value): take the pixel already resolved (segment_eval.inc)
    if (ly == 0.f) yb = ya;
    if (lx == 0.f) xb = xa;
    int gya0, gya1, gyb0, gyb1, gxa0, gxa1, gxb0, gxb1;
    float lya, lyb, lxa, lxb;
    seg_axis_taps(ya, sy, (int)gh, gya0, gya1, lya);
    seg_axis_taps(yb, sy, (int)gh, gyb0, gyb1, lyb);
    seg_axis_taps(xa, sx, igw, gxa0, gxa1, lxa);
    seg_axis_taps(xb, sx, igw, gxb0, gxb1, lxb);
    const int ra0 = (gya0 - row0) * igw, ra1 = (gya1 - row0) * igw, rb0 = (gyb0 - row0) * igw, rb1 = (gyb1 - row0) * igw;
    int grp;
    if (ya == yb && xa == xb) {
      // one network pixel: its group exactly as segclip_seg_label_map forms it
      grp = seg_pixel_group(base, A.G, plane, ra0 + gxa0, ra0 + gxa1, ra1 + gxa0, ra1 + gxa1, lya, lxa);
    } else {
      const SegGridTaps t00 = {ra0 + gxa0, ra0 + gxa1, ra1 + gxa0, ra1 + gxa1, lya, lxa};
      const SegGridTaps t01 = {ra0 + gxb0, ra0 + gxb1, ra1 + gxb0, ra1 + gxb1, lya, lxb};
      const SegGridTaps t10 = {rb0 + gxa0, rb0 + gxa1, rb1 + gxa0, rb1 + gxa1, lyb, lxa};
      const SegGridTaps t11 = {rb0 + gxb0, rb0 + gxb1, rb1 + gxb0, rb1 + gxb1, lyb, lxb};
      const float hy = 1.f - ly, hx = 1.f - lx;
      float best = -INFINITY;
      grp = 0;
      for (int g = 0; g < A.G; ++g) {
        const float* c = base + (int64_t)g * plane;
        const float v00 = seg_grid_value(c, t00);
        const float v01 = xb == xa ? v00 : seg_grid_value(c, t01);
        const float v10 = yb == ya ? v00 : seg_grid_value(c, t10);
        const float v11 = yb == ya ? v01 : (xb == xa ? v10 : seg_grid_value(c, t11));
        const float v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
        if (v > best) { best = v; grp = g; }
      }
    }
    pack |= (uint32_t)(grp & 255) << (8 * q);
  }
  uint8_t* o = A.groups + grp_off + pq;
  if (pq + SEG_RENDER_PPL <= total && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(o) = pack;
  } else {
    for (int q = 0; q < SEG_RENDER_PPL && pq + q < total; ++q) o[q] = (uint8_t)(pack >> (8 * q));
  }
}

// ---------------------------------------------------------------- overlay and anchor sums
struct SegBlendArgs {
  const int64_t* images;   // (B, SEG_BLEND_COLS)
  const uint8_t* maps;     // flat index maps
  const uint8_t* palette;  // (P, 3) RGB
  int64_t maps_bytes, out_bytes;
  int B, P, reverse, skip_zero;
  double a, b;             // 1.0 - opacity and opacity, rounded on the host as numpy rounds them
  uint8_t* out;            // flat
  unsigned long long* sums;  // (B, P, 3): count, sum of y, sum of x; or null
};

// numpy's img * (1 - opacity) + color * opacity on one byte, then astype(uint8): two rounded fp64 products, one rounded sum,
// truncation.  `cb` is the rounded product color * opacity.  A fused multiply-add would skip one rounding and change bytes,
// so contraction is off here.
__device__ __forceinline__ uint32_t seg_blend_byte(uint32_t p, double a, double cb) {
#pragma clang fp contract(off)
  const double pa = (double)p * a;
  const double v = pa + cb;
  return (uint32_t)(int)v;
}

// one anchor contribution into the workgroup's (P, 3) counters
__device__ __forceinline__ void seg_anchor_add(int* cnt, int idx, int n, int sy, int sx) {
  atomicAdd(&cnt[3 * idx], n);
  if (sy) atomicAdd(&cnt[3 * idx + 1], sy);
  if (sx) atomicAdd(&cnt[3 * idx + 2], sx);
}

// A workgroup owns SEG_RENDER_TILE consecutive pixels of one image's flat (h, w) index map, a lane four of them: 4 map bytes
// and 12 source bytes in, 12 bytes out, as dwords where the addresses are dword multiples (the host aligns the map and output
// offsets of every image to 4; a contiguous source of a dword-aligned address then is aligned at every unit, a padded row
// stride decides per unit) and as bytes otherwise.  The anchor sums of a tile stay below 2^31: 1024 pixels x coordinates < 2^15
// (the limit of this scheme is a tile of 2^16 pixels).
__global__ __launch_bounds__(256) void seg_blend_kernel(SegBlendArgs A) {
  __shared__ double s_cb[SEG_MAX_PALETTE * 3];   // color * opacity per (index, image channel); 0 from index P on
  __shared__ int s_cnt[SEG_MAX_PALETTE * 3];
  __shared__ int s_img;
  const int tid = threadIdx.x;
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_BLEND_COLS, BL_BLK, (int64_t)blockIdx.x);
  for (int i = tid; i < SEG_MAX_PALETTE * 3; i += 256) {
    const int idx = i / 3, c = i - 3 * idx;
    s_cb[i] = idx < A.P ? (double)A.palette[3 * idx + (A.reverse ? 2 - c : c)] * A.b : 0.0;
    s_cnt[i] = 0;
  }
  __syncthreads();

  const int img = s_img;
  const int64_t* D = A.images + (int64_t)img * SEG_BLEND_COLS;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(D[BL_SRC]);
  const int64_t h = D[BL_H], w = D[BL_W], stride = D[BL_STRIDE], map_off = D[BL_MAP], out_off = D[BL_OUT];
  bool ok = src != nullptr && h >= 1 && w >= 1 && h < SEG_BLEND_LIMIT && w < SEG_BLEND_LIMIT && stride >= 3 * w;
  const int64_t total = ok ? h * w : 0;
  ok = ok && map_off >= 0 && map_off + total <= A.maps_bytes && out_off >= 0 && out_off + 3 * total <= A.out_bytes;
  const int64_t p0 = ((int64_t)blockIdx.x - D[BL_BLK]) * SEG_RENDER_TILE;
  if (!ok || p0 < 0 || p0 >= total) return;  // block-uniform, and nothing was counted

  const int64_t pq = p0 + (int64_t)tid * SEG_RENDER_PPL;
  const int iw = (int)w;
  int run_i = -1, run_n = 0, run_y = 0, run_x = 0;   // the lane's pixels of one index are counted once
  if (pq < total) {
    const bool whole = pq + SEG_RENDER_PPL <= total;
    int y = (int)((uint32_t)pq / (uint32_t)iw), x = (int)pq - y * iw;
    // the unit's indices
    uint32_t idx4 = 0;
    const uint8_t* m = A.maps + map_off + pq;
    if (whole && (reinterpret_cast<uintptr_t>(m) & 3) == 0) {
      idx4 = *reinterpret_cast<const uint32_t*>(m);
    } else {
      for (int q = 0; q < SEG_RENDER_PPL && pq + q < total; ++q) idx4 |= (uint32_t)m[q] << (8 * q);
    }
    // its 12 source bytes: one run of memory when the unit lies in one row or the rows follow each other without padding
    uint32_t s[3] = {0, 0, 0};
    const uint8_t* sp = src + (int64_t)y * stride + 3 * x;
    if (whole && (x + SEG_RENDER_PPL <= iw || stride == 3 * w) && (reinterpret_cast<uintptr_t>(sp) & 3) == 0) {
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(sp);
      s[0] = s4[0]; s[1] = s4[1]; s[2] = s4[2];
    } else {
      int yy = y, xx = x;
      for (int q = 0; q < SEG_RENDER_PPL && pq + q < total; ++q) {
        const uint8_t* b = src + (int64_t)yy * stride + 3 * xx;
        for (int c = 0; c < 3; ++c) {
          const int k = 3 * q + c;
          s[k >> 2] |= (uint32_t)b[c] << (8 * (k & 3));
        }
        if (++xx == iw) { xx = 0; ++yy; }
      }
    }
    uint32_t o[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < SEG_RENDER_PPL; ++q) {
      const int idx = (int)((idx4 >> (8 * q)) & 255u);
      const bool keep = A.skip_zero && idx == 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int k = 3 * q + c;
        const uint32_t p = (s[k >> 2] >> (8 * (k & 3))) & 255u;
        const uint32_t v = keep ? p : seg_blend_byte(p, A.a, s_cb[3 * idx + c]);
        o[k >> 2] |= (v & 255u) << (8 * (k & 3));
      }
      if (A.sums && pq + q < total) {
        if (idx == run_i) {
          ++run_n; run_y += y; run_x += x;
        } else {
          if (run_n && run_i < A.P) seg_anchor_add(s_cnt, run_i, run_n, run_y, run_x);
          run_i = idx; run_n = 1; run_y = y; run_x = x;
        }
        if (++x == iw) { x = 0; ++y; }
      }
    }
    uint8_t* op = A.out + out_off + 3 * pq;
    if (whole && (reinterpret_cast<uintptr_t>(op) & 3) == 0) {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(op);
      o4[0] = o[0]; o4[1] = o[1]; o4[2] = o[2];
    } else {
      for (int k = 0; k < 3 * SEG_RENDER_PPL && pq + k / 3 < total; ++k) op[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
  }
  if (A.sums) {  // block-uniform
    // a wave whose pixels all carry one index (the inside of a segment) adds once, not 64 times to one LDS address
    if (run_n && run_i >= A.P) run_n = 0;
    const int first = __shfl(run_i, 0, 64);
    if (__all(run_n == 0 || run_i == first)) {
      const int n = wave_sum_int(run_n), sy = wave_sum_int(run_n ? run_y : 0), sx = wave_sum_int(run_n ? run_x : 0);
      if ((tid & 63) == 0 && n) seg_anchor_add(s_cnt, first, n, sy, sx);
    } else if (run_n) {
      seg_anchor_add(s_cnt, run_i, run_n, run_y, run_x);
    }
    __syncthreads();
    unsigned long long* dst = A.sums + (int64_t)img * A.P * 3;
    for (int i = tid; i < 3 * A.P; i += 256)
      if (s_cnt[i]) atomicAdd(&dst[i], (unsigned long long)s_cnt[i]);
  }
}
