// Connected components of label maps (segment.hip): ids, areas, a compact record list (boxes, coordinate sums) and despeckled
// maps, for images of mixed sizes in one call.  The reference has no such op: the definition is this project's
// (include/segclip_hip.h, segclip_seg_components) and tests/cc_reference.py restates it with a plain union-find.
//   seg_cc_local_kernel : one workgroup per SEG_CC_TH x SEG_CC_TW tile: union-find of the tile in LDS; every pixel's parent is
//                         its tile-local root (the component's first pixel of the tile in raster order), as an in-image index
//   seg_cc_merge_kernel : the pixels on a tile's rim union their tile-local root with that of every forward neighbour (right,
//                         down-left, down, down-right) in another tile: atomicMin on the parent array
//   seg_cc_roots_kernel : roots (parent = own index) per tile row = one wave's ballot; <false> counts them per row segment,
//                         <true>, after the scan, ranks them and writes the fixed columns of their record rows
//   seg_cc_chunk_kernel, seg_cc_scan_kernel : exclusive scan of the segment counts (chunk totals, their scan by one workgroup,
//                         the chunks' own scans) and the total
//   seg_cc_stats_kernel : final root of every pixel; area, box and coordinate sums reduced in LDS per (tile, tile-local root)
//                         and added with ONE set of global integer atomics per such pair
//   seg_cc_final_kernel : area_px and cleaned
// A row segment (y, tile column) of an image precedes another exactly when its pixels do in raster order, so the scan over
// (image, y, tile column) gives ranks in ascending (image, id) order whatever the tiles' schedule.
// Parents only ever decrease and only a root's parent is ever changed (atomicMin), so inside the merge kernel a stale parent
// is still an ancestor: the find loop is right on stale values (it loads with relaxed agent-scope atomics all the same).  Every
// retry of a union continues from a strictly smaller index, a find follows a parent only downwards: every loop ends whatever
// the schedule and whatever the memory holds, and no workgroup ever waits for another.
// Traffic per pixel with every output: local 1 B read + 8 written, roots 2 x 4 read, stats 4 read + 4 written, final 8-9 read +
// 5 written; the merge touches the rims only.
// The kernels that read or write labels are templates on the label element L: uint8_t, or uint16_t for the maps of
// SegInference(label_dtype=torch.int16) (an int16 tensor read as unsigned).  A label enters only through equality, the record's
// label column and `cleaned`; with uint16_t a label read or written is one byte more, everything else is the same code.

#define SEG_CC_COLS SEGCLIP_SEG_CC_COLS   // int64 columns of one image row of the table (segclip_hip.h)
#define SEG_CC_TH SEGCLIP_SEG_CC_TILE_H
#define SEG_CC_TW SEGCLIP_SEG_CC_TILE_W             // the wave: a tile row is one wave's lanes
#define SEG_CC_PIX (SEG_CC_TH * SEG_CC_TW)
#define SEG_CC_LIMIT SEGCLIP_SEG_SOURCE_LIMIT
#define SEG_CC_SCAN_ITEMS 8
#define SEG_CC_SCAN_CHUNK (256 * SEG_CC_SCAN_ITEMS)   // entries of the segment counts that one workgroup scans
enum { CC_H, CC_W, CC_OFF, CC_BLK };
static_assert(SEG_CC_TW == SEGCLIP_WAVE && SEG_CC_TH % 4 == 0 && 2 * (SEG_CC_TW + SEG_CC_TH) <= 256, "seg_cc tile");

// What follows the label element, stated once for the three files and their host entries (segment.hip):
//   tile_t      : a tile's labels in LDS (seg_cc_local_kernel): every label value and -1, which no label equals
//   key_t       : the boundary kernel's run key, q | g << BITS | flags << 2 BITS (segment_boundary.inc)
//   BITS, TOP   : of a label in the sieve's and the boundary's keys; TOP is the largest label
//   MAX_CLASSES : of the boundary areas (the counters in LDS)
//   word, unit  : how the host entries' messages call a label value and the elements of a label buffer
template <class L> struct SegLabel;
template <> struct SegLabel<uint8_t> {
  typedef short tile_t;
  typedef int key_t;
  static constexpr int BITS = 8, TOP = 255, MAX_CLASSES = SEG_MAX_CLASSES;
  static constexpr const char* word = "a byte";
  static constexpr const char* unit = "bytes";
};
template <> struct SegLabel<uint16_t> {
  typedef int tile_t;
  typedef long long key_t;
  static constexpr int BITS = 16, TOP = 65535, MAX_CLASSES = SEG_WIDE_MAX_CLASSES;
  static constexpr const char* word = "a 16-bit value";
  static constexpr const char* unit = "elements";
};

struct SegCCArgs {
  const int64_t* images;     // (B, SEG_CC_COLS)
  const void* labels;        // flat input labels, elements of L
  int64_t labels_n, n_blocks, n_seg;   // labels_n: elements of `labels`
  int B, max_side, conn8, skip;
  // per pixel, at the labels' offsets
  int32_t* parent;           // in-image index of an ancestor, -1 for a skipped pixel
  int32_t* root;             // the id (= ids when the caller wants them)
  int32_t* area;             // at a root: its component's pixel count
  int32_t* rank;             // at a root: its record row, or -1
  int64_t* seg;              // (n_blocks * SEG_CC_TH): roots per row segment, then their exclusive prefix sums
  int32_t* area_px;
  int64_t* records;
  int64_t K;
  int64_t min_area;
  int fill;
  void* cleaned;             // elements of L
};
template <class L> __device__ __forceinline__ const L* seg_cc_labels(const SegCCArgs& A) { return static_cast<const L*>(A.labels); }


// One tile of one image, range-checked: the host entry cannot inspect device memory.
struct SegCCTile { int img, h, w, y0, x0, th, tw, tiles_x, tx; int64_t off, seg0; bool ok; };
__device__ __forceinline__ SegCCTile seg_cc_tile(const SegCCArgs& A, int img) {
  const int64_t* D = A.images + (int64_t)img * SEG_CC_COLS;
  const int64_t h = D[CC_H], w = D[CC_W], blk = D[CC_BLK];
  SegCCTile T;
  T.img = img; T.off = D[CC_OFF];
  T.ok = h >= 1 && w >= 1 && h <= A.max_side && w <= A.max_side && h < SEG_CC_LIMIT && w < SEG_CC_LIMIT;
  T.h = T.ok ? (int)h : 1; T.w = T.ok ? (int)w : 1;
  T.tiles_x = (T.w + SEG_CC_TW - 1) / SEG_CC_TW;
  const int tiles = T.tiles_x * ((T.h + SEG_CC_TH - 1) / SEG_CC_TH);
  T.ok = T.ok && T.off >= 0 && T.off <= A.labels_n - (int64_t)T.h * T.w && blk >= 0 && blk <= A.n_blocks - tiles;
  const int64_t t = (int64_t)blockIdx.x - blk;
  if (t < 0 || t >= tiles) T.ok = false;
  const int ty = T.ok ? (int)t / T.tiles_x : 0;
  T.tx = T.ok ? (int)t - ty * T.tiles_x : 0;
  T.y0 = ty * SEG_CC_TH; T.x0 = T.tx * SEG_CC_TW;
  T.th = min(SEG_CC_TH, T.h - T.y0); T.tw = min(SEG_CC_TW, T.w - T.x0);
  T.seg0 = blk * SEG_CC_TH;  // the image's h * tiles_x row segments fit the SEG_CC_TH entries of each of its tiles
  return T;
}

// SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP on the LDS copy of a tile, __HIP_MEMORY_SCOPE_AGENT on the global parent array.
// A parent is followed only downwards (0 <= parent < index), so the walk ends on any memory contents.
template <int SCOPE>
__device__ __forceinline__ int seg_cc_find(int* p, int a) {
  for (;;) {
    const int q = __hip_atomic_load(p + a, __ATOMIC_RELAXED, SCOPE);
    if (q < 0 || q >= a) return a;
    a = q;
  }
}
// after the merge kernel nothing changes a parent any more: plain loads
__device__ __forceinline__ int seg_cc_find_plain(const int* p, int a) {
  for (;;) {
    const int q = p[a];
    if (q < 0 || q >= a) return a;
    a = q;
  }
}
// Hang the larger root under the smaller.  The atomic's return value says whether `a` was still a root; if not, somebody
// lowered it to old < a first and the union continues from there: a + b falls with every retry.
template <int SCOPE>
__device__ __forceinline__ void seg_cc_union(int* p, int a, int b) {
  for (;;) {
    a = seg_cc_find<SCOPE>(p, a);
    b = seg_cc_find<SCOPE>(p, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a || old < 0 || old > a) return;  // joined (or no parent at all: only in memory that no kernel of this call wrote)
    a = old;
  }
}

#define SEG_CC_PROLOGUE(A)                                                                                  \
  __shared__ int s_img;                                                                                     \
  const int tid = threadIdx.x;                                                                              \
  if (tid == 0) s_img = seg_block_image(A.images, A.B, SEG_CC_COLS, CC_BLK, (int64_t)blockIdx.x);           \
  __syncthreads();                                                                                          \
  const SegCCTile T = seg_cc_tile(A, s_img);                                                                \
  if (!T.ok) return; /* block-uniform */

// ---------------------------------------------------------------- the tile in LDS
template <class L>
__global__ __launch_bounds__(256) void seg_cc_local_kernel(SegCCArgs A) {
  typedef typename SegLabel<L>::tile_t tile_t;
  __shared__ int s_par[SEG_CC_PIX];
  __shared__ tile_t s_lab[SEG_CC_PIX];
  SEG_CC_PROLOGUE(A)
  const L* lab = seg_cc_labels<L>(A) + T.off;
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k, ly = i / SEG_CC_TW, lx = i % SEG_CC_TW;
    int b = -1;
    if (ly < T.th && lx < T.tw) b = lab[(T.y0 + ly) * T.w + T.x0 + lx];
    if (b == A.skip) b = -1;
    s_lab[i] = (tile_t)b;
    // a tile row is one wave: a pixel starts under the first pixel of its horizontal run, so no union goes sideways
    const int before = __shfl_up(b, 1, 64);
    const unsigned long long starts = __ballot(lx == 0 || before != b);
    s_par[i] = ly * SEG_CC_TW + 63 - __clzll((long long)(starts & (~0ull >> (63 - lx))));
  }
  __syncthreads();
  // runs join upwards.  A union is left to the run's pixel one to the left (or right) where that one sees the same two runs:
  // two runs that overlap in many columns cost one union
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k, ly = i / SEG_CC_TW, lx = i % SEG_CC_TW;
    const int b = s_lab[i];
    if (b < 0 || ly == 0) continue;
    const bool left = lx > 0 && s_lab[i - 1] == b, right = lx < SEG_CC_TW - 1 && s_lab[i + 1] == b;
    const bool up = s_lab[i - SEG_CC_TW] == b;
    const bool up_left = lx > 0 && s_lab[i - SEG_CC_TW - 1] == b, up_right = lx < SEG_CC_TW - 1 && s_lab[i - SEG_CC_TW + 1] == b;
    if (up && !(left && up_left)) seg_cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, i, i - SEG_CC_TW);
    if (A.conn8 && !up) {
      if (up_left && !left) seg_cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, i, i - SEG_CC_TW - 1);
      if (up_right && !right) seg_cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, i, i - SEG_CC_TW + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k, ly = i / SEG_CC_TW, lx = i % SEG_CC_TW;
    if (ly >= T.th || lx >= T.tw) continue;
    const int64_t at = T.off + (T.y0 + ly) * T.w + T.x0 + lx;
    int g = -1;
    if (s_lab[i] >= 0) {
      const int r = seg_cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, i);
      g = (T.y0 + r / SEG_CC_TW) * T.w + T.x0 + r % SEG_CC_TW;
    }
    A.parent[at] = g;
    A.area[at] = 0;
  }
}

// ---------------------------------------------------------------- across the tiles' rims
// Every adjacent pair of pixels has one forward direction, and both pixels of a pair that crosses tiles lie on a rim: the rim
// pixels looking forward see every such pair once.  A lane whose (own root, neighbour's root) pair equals its predecessor's in
// the same direction, or its own in an earlier direction, leaves the union to that one: a rim inside one component costs one.
template <class L>
__global__ __launch_bounds__(256) void seg_cc_merge_kernel(SegCCArgs A) {
  SEG_CC_PROLOGUE(A)
  int ly = -1, lx = 0;
  if (tid < SEG_CC_TW) { ly = 0; lx = tid; }
  else if (tid < 2 * SEG_CC_TW) { ly = T.th > 1 ? T.th - 1 : -1; lx = tid - SEG_CC_TW; }
  else if (tid < 2 * SEG_CC_TW + SEG_CC_TH) { ly = tid - 2 * SEG_CC_TW; lx = 0; if (ly == 0 || ly >= T.th - 1) ly = -1; }
  else if (tid < 2 * SEG_CC_TW + 2 * SEG_CC_TH) {
    ly = tid - 2 * SEG_CC_TW - SEG_CC_TH; lx = T.tw - 1;
    if (ly == 0 || ly >= T.th - 1 || T.tw == 1) ly = -1;
  }
  bool act = ly >= 0 && ly < T.th && lx < T.tw;
  const int y = T.y0 + ly, x = T.x0 + lx;
  const L* lab = seg_cc_labels<L>(A) + T.off;
  int* par = A.parent + T.off;
  int b = -1, ra = -1;
  if (act) {
    b = lab[y * T.w + x];
    if (b == A.skip) act = false;
  }
  if (act) ra = __hip_atomic_load(par + y * T.w + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ra < 0) act = false;
  const int lane = tid & 63;
  const unsigned long long none = ~0ull;
  unsigned long long mine[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int ny = y + (d == 0 ? 0 : 1), nx = x + (d == 0 ? 1 : d - 2);
    unsigned long long key = none;
    int rb = -1;
    if (act && (A.conn8 || d == 0 || d == 2) && nx >= 0 && nx < T.w && ny < T.h &&
        (ny / SEG_CC_TH != y / SEG_CC_TH || nx / SEG_CC_TW != x / SEG_CC_TW) && lab[ny * T.w + nx] == b) {
      rb = __hip_atomic_load(par + ny * T.w + nx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (rb >= 0) key = ((unsigned long long)(unsigned)ra << 32) | (unsigned)rb;
    }
    mine[d] = key;
    const unsigned long long before = __shfl_up(key, 1, 64);  // every lane takes part
    bool dup = lane > 0 && before == key;
#pragma unroll
    for (int e = 0; e < d; ++e) dup = dup || mine[e] == key;
    if (key != none && !dup) seg_cc_union<__HIP_MEMORY_SCOPE_AGENT>(par, ra, rb);
  }
}

// ---------------------------------------------------------------- roots per row segment: count, then rank
template <bool RANK, class L>
__global__ __launch_bounds__(256) void seg_cc_roots_kernel(SegCCArgs A) {
  SEG_CC_PROLOGUE(A)
  const int lane = tid & 63, wv = tid >> 6;
  for (int r = 0; r < SEG_CC_TH / 4; ++r) {
    const int ly = wv * (SEG_CC_TH / 4) + r;
    if (ly >= T.th) break;  // wave-uniform
    const int y = T.y0 + ly, idx = y * T.w + T.x0 + lane;
    const bool is_root = lane < T.tw && A.parent[T.off + idx] == idx;
    const unsigned long long m = __ballot(is_root);
    const int64_t s = T.seg0 + (int64_t)y * T.tiles_x + T.tx;  // < n_seg: seg_cc_tile checked the image's tiles against n_blocks
    if (!RANK) {
      if (lane == 0) A.seg[s] = __popcll(m);
    } else if (is_root) {
      const int64_t rank = A.seg[s] + __popcll(m & ((1ull << lane) - 1ull));
      const bool row = rank < A.K && rank <= 0x7fffffffll;
      A.rank[T.off + idx] = row ? (int)rank : -1;
      if (row) {
        int64_t* R = A.records + 10 * rank;
        R[0] = T.img; R[1] = idx; R[2] = seg_cc_labels<L>(A)[T.off + idx]; R[3] = 0;
        R[4] = SEG_CC_LIMIT; R[5] = SEG_CC_LIMIT; R[6] = 0; R[7] = 0; R[8] = 0; R[9] = 0;
      }
    }
  }
}

// The scan of the segment counts in three launches: the totals of chunks of SEG_CC_SCAN_CHUNK entries (one workgroup each),
// one workgroup's exclusive scan of those totals (and the grand total = count), the chunks' own scans from their totals' prefix.
// the workgroup's exclusive prefix of t (NW waves) and, in every thread, its total
template <int NW>
__device__ __forceinline__ int64_t seg_cc_block_scan(int64_t t, int64_t* s_wave, int64_t& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int64_t incl = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  int64_t before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int64_t u = s_wave[k];
    if (k < wv) before += u;
    total += u;
  }
  __syncthreads();  // s_wave may be written again
  return before + incl - t;
}

// APPLY false: part[chunk] = the chunk's total.  APPLY true: the chunk's exclusive prefix sums in place, from part[chunk].
template <bool APPLY>
__global__ __launch_bounds__(256) void seg_cc_chunk_kernel(int64_t* seg, int64_t n, int64_t* part) {
  __shared__ int64_t s_wave[4];
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * SEG_CC_SCAN_ITEMS;
  int64_t v[SEG_CC_SCAN_ITEMS], t = 0, total;
#pragma unroll
  for (int j = 0; j < SEG_CC_SCAN_ITEMS; ++j) {
    v[j] = i0 + j < n ? seg[i0 + j] : 0;
    t += v[j];
  }
  const int64_t excl = seg_cc_block_scan<4>(t, s_wave, total);
  if (!APPLY) {
    if (threadIdx.x == 0) part[blockIdx.x] = total;
    return;
  }
  int64_t run = part[blockIdx.x] + excl;
#pragma unroll
  for (int j = 0; j < SEG_CC_SCAN_ITEMS; ++j) {
    if (i0 + j < n) seg[i0 + j] = run;
    run += v[j];
  }
}

// Exclusive prefix sums of part[0 .. n) in place, and the total: one workgroup, SEG_CC_SCAN_ITEMS consecutive entries per lane.
__global__ __launch_bounds__(1024) void seg_cc_scan_kernel(int64_t* part, int64_t n, int64_t* count) {
  __shared__ int64_t s_wave[16];
  const int tid = threadIdx.x;
  int64_t carry = 0;  // the same in every thread
  for (int64_t base = 0; base < n; base += 1024 * SEG_CC_SCAN_ITEMS) {
    const int64_t i0 = base + (int64_t)tid * SEG_CC_SCAN_ITEMS;
    int64_t v[SEG_CC_SCAN_ITEMS], t = 0, total;
#pragma unroll
    for (int j = 0; j < SEG_CC_SCAN_ITEMS; ++j) {
      v[j] = i0 + j < n ? part[i0 + j] : 0;
      t += v[j];
    }
    int64_t run = carry + seg_cc_block_scan<16>(t, s_wave, total);
#pragma unroll
    for (int j = 0; j < SEG_CC_SCAN_ITEMS; ++j) {
      if (i0 + j < n) part[i0 + j] = run;
      run += v[j];
    }
    carry += total;
  }
  if (tid == 0 && count) count[0] = carry;
}

// ---------------------------------------------------------------- final roots, areas, boxes, sums
// Pixels of a tile are grouped by key: the parent where it lies in the tile (the tile-local root, or a root's new parent that
// happens to lie in the tile too), otherwise the pixel itself (a tile-local root that now hangs under another tile).  A group
// lies inside one component, so ONE find from the key's pixel and ONE set of global atomics serve all its pixels.  A tile row
// whose pixels share one key (the usual case) is reduced by the wave and costs one set of LDS atomics.
template <bool REC>
__global__ __launch_bounds__(256) void seg_cc_stats_kernel(SegCCArgs A) {
  __shared__ int s_cnt[SEG_CC_PIX], s_root[SEG_CC_PIX];
  __shared__ int s_y0[REC ? SEG_CC_PIX : 1], s_x0[REC ? SEG_CC_PIX : 1], s_y1[REC ? SEG_CC_PIX : 1], s_x1[REC ? SEG_CC_PIX : 1];
  __shared__ int s_sy[REC ? SEG_CC_PIX : 1], s_sx[REC ? SEG_CC_PIX : 1];
  SEG_CC_PROLOGUE(A)
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k;
    s_cnt[i] = 0;
    if (REC) { s_y0[i] = SEG_CC_TH; s_x0[i] = SEG_CC_TW; s_y1[i] = -1; s_x1[i] = -1; s_sy[i] = 0; s_sx[i] = 0; }
  }
  __syncthreads();
  int key[SEG_CC_TH / 4];
#pragma unroll
  for (int r = 0; r < SEG_CC_TH / 4; ++r) {
    const int ly = wv * (SEG_CC_TH / 4) + r;
    int k = -1;
    if (ly < T.th && lane < T.tw) {
      const int p = A.parent[T.off + (T.y0 + ly) * T.w + T.x0 + lane];
      if (p >= 0) {
        const int py = (int)((uint32_t)p / (uint32_t)T.w) - T.y0, px = p - (py + T.y0) * T.w - T.x0;
        const bool inside = py >= 0 && py < SEG_CC_TH && px >= 0 && px < SEG_CC_TW;
        k = inside ? py * SEG_CC_TW + px : ly * SEG_CC_TW + lane;
      }
    }
    key[r] = k;
    const unsigned long long m = __ballot(k >= 0);
    if (m == 0) continue;  // wave-uniform
    const int first = __ffsll((long long)m) - 1;
    const int k0 = __shfl(k, first, 64);
    if (__ballot(k >= 0 && k != k0) == 0) {
      const int sx = REC ? wave_sum_int(k >= 0 ? lane : 0) : 0;
      if (lane == first) {
        const int c = __popcll(m);
        atomicAdd(&s_cnt[k0], c);
        if (REC) {
          atomicMin(&s_y0[k0], ly); atomicMax(&s_y1[k0], ly);
          atomicMin(&s_x0[k0], first); atomicMax(&s_x1[k0], 63 - __clzll((long long)m));
          atomicAdd(&s_sy[k0], c * ly); atomicAdd(&s_sx[k0], sx);
        }
      }
    } else if (k >= 0) {
      atomicAdd(&s_cnt[k], 1);
      if (REC) {
        atomicMin(&s_y0[k], ly); atomicMax(&s_y1[k], ly); atomicMin(&s_x0[k], lane); atomicMax(&s_x1[k], lane);
        atomicAdd(&s_sy[k], ly); atomicAdd(&s_sx[k], lane);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k, c = s_cnt[i];
    if (c == 0) continue;
    const int root = seg_cc_find_plain(A.parent + T.off, (T.y0 + i / SEG_CC_TW) * T.w + T.x0 + i % SEG_CC_TW);
    s_root[i] = root;
    atomicAdd(&A.area[T.off + root], c);
    if (REC) {
      const int rk = A.rank[T.off + root];
      if (rk >= 0 && rk < A.K) {
        int64_t* R = A.records + 10 * (int64_t)rk;
        atomicAdd(reinterpret_cast<unsigned long long*>(R + 3), (unsigned long long)c);
        atomicMin(reinterpret_cast<long long*>(R + 4), (long long)(T.y0 + s_y0[i]));
        atomicMin(reinterpret_cast<long long*>(R + 5), (long long)(T.x0 + s_x0[i]));
        atomicMax(reinterpret_cast<long long*>(R + 6), (long long)(T.y0 + s_y1[i] + 1));
        atomicMax(reinterpret_cast<long long*>(R + 7), (long long)(T.x0 + s_x1[i] + 1));
        atomicAdd(reinterpret_cast<unsigned long long*>(R + 8), (unsigned long long)((int64_t)c * T.y0 + s_sy[i]));
        atomicAdd(reinterpret_cast<unsigned long long*>(R + 9), (unsigned long long)((int64_t)c * T.x0 + s_sx[i]));
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SEG_CC_TH / 4; ++r) {
    const int ly = wv * (SEG_CC_TH / 4) + r;
    if (ly < T.th && lane < T.tw) A.root[T.off + (T.y0 + ly) * T.w + T.x0 + lane] = key[r] >= 0 ? s_root[key[r]] : -1;
  }
}

// ---------------------------------------------------------------- area per pixel, despeckled labels
template <class L>
__global__ __launch_bounds__(256) void seg_cc_final_kernel(SegCCArgs A) {
  SEG_CC_PROLOGUE(A)
  const L* lab = seg_cc_labels<L>(A);
  L* cleaned = static_cast<L*>(A.cleaned);
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k, ly = i / SEG_CC_TW, lx = i % SEG_CC_TW;
    if (ly >= T.th || lx >= T.tw) continue;
    const int64_t at = T.off + (T.y0 + ly) * T.w + T.x0 + lx;
    const int r = A.root[at];
    const bool in_image = r >= 0 && r < T.h * T.w;
    const int a = in_image ? A.area[T.off + r] : 0;
    if (A.area_px) A.area_px[at] = a;
    if (cleaned) cleaned[at] = in_image && a < A.min_area ? (L)A.fill : lab[at];
  }
}
