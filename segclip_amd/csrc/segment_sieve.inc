// Despeckling by merging (segment.hip, segclip_seg_sieve): every small component takes the label of its largest kept
// 4-neighbour, in rounds.  The reference has no such op: the definition is this project's (include/segclip_hip.h) and
// tests/cc_merge_reference.py restates it.  A round runs seg_cc_local_kernel, seg_cc_merge_kernel and seg_cc_stats_kernel<false>
// of segment_objects.inc on the round's input (every pixel's root, every root's area) and then
//   seg_sieve_vote_kernel  : every pixel of a small component forms the key (area << 8) | (255 - label) of its kept 4-neighbours;
//                            the keys are reduced with 64-bit atomicMax in LDS per (tile, tile-local group: the key of the
//                            stats kernel) and reach the component's slot, at its root, with ONE global 64-bit atomicMax per
//                            such pair.  A component that spans tiles collects the contacts of all of them there.
//   seg_sieve_final_kernel : a small pixel takes 255 - (slot & 255), or the orphan rule where the slot is still zero
// Both are templates on the label element L (segment_objects.inc): with uint16_t the key is (area << 16) | (65535 - label) and
// the winner 65535 - (slot & 65535).  An area is below 2^30, so the key fits 46 bits; zero remains "no contact".
// The maximum of integers depends on no order: two calls give the same bits.  No loop depends on memory contents and no
// workgroup waits for another.
// Traffic per pixel and round beyond the three component kernels: 8 B of slot cleared; vote 4 B of root + the gathered area (4 B
// lines that neighbours share); only the pixels of small components read their four neighbours' roots, areas and labels, and
// only those with a contact their parent (4 B) for the group; one 8 B atomic per (tile, voting group).  final: 4 B of root +
// the gathered area + 1 B of label read, 1 B written, 8 B of slot per small pixel.

#define SEG_SIEVE_MAX_ROUNDS SEGCLIP_SEG_SIEVE_MAX_ROUNDS

struct SegSieveArgs {
  SegCCArgs cc;                  // labels = the round's input; parent, root and area as the component kernels left them
  unsigned long long* slot;      // per pixel, at the labels' offsets: at a small root the largest key of its contacts, else 0
  void* out;                     // the round's output, laid out like the labels (elements of L)
  int orphan;                    // the label of a small component without a candidate, or -1: its own
};

template <class L>
__global__ __launch_bounds__(256) void seg_sieve_vote_kernel(SegSieveArgs S) {
  __shared__ unsigned long long s_vote[SEG_CC_PIX];
  __shared__ int s_root[SEG_CC_PIX];
  const SegCCArgs& A = S.cc;
  SEG_CC_PROLOGUE(A)
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) s_vote[tid + 256 * k] = 0ull;
  __syncthreads();
  const int n = T.h * T.w;
  const L* lab = seg_cc_labels<L>(A) + T.off;
  const int* root = A.root + T.off;
  const int* area = A.area + T.off;
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k, ly = i / SEG_CC_TW, lx = i % SEG_CC_TW;
    if (ly >= T.th || lx >= T.tw) continue;
    const int y = T.y0 + ly, x = T.x0 + lx, at = y * T.w + x;
    const int r = root[at];
    if (r < 0 || r >= n || area[r] >= A.min_area) continue;   // skipped, or kept
    unsigned long long best = 0ull;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int ny = y + (d == 2 ? -1 : d == 3 ? 1 : 0), nx = x + (d == 0 ? -1 : d == 1 ? 1 : 0);
      if (ny < 0 || ny >= T.h || nx < 0 || nx >= T.w) continue;
      const int q = ny * T.w + nx, rq = root[q];
      if (rq < 0 || rq >= n || rq == r) continue;
      const int aq = area[rq];
      if (aq < A.min_area) continue;
      const unsigned long long key = ((unsigned long long)(unsigned)aq << SegLabel<L>::BITS) | (unsigned)(SegLabel<L>::TOP - lab[q]);
      best = key > best ? key : best;
    }
    if (best == 0ull) continue;
    // the group of the stats kernel: the parent where it lies in the tile, otherwise the pixel itself
    const int p = A.parent[T.off + at];
    int g = i;
    if (p >= 0) {
      const int py = (int)((uint32_t)p / (uint32_t)T.w) - T.y0, px = p - (py + T.y0) * T.w - T.x0;
      if (py >= 0 && py < SEG_CC_TH && px >= 0 && px < SEG_CC_TW) g = py * SEG_CC_TW + px;
    }
    s_root[g] = r;               // every pixel of a group has the same root
    atomicMax(&s_vote[g], best);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k;
    const unsigned long long v = s_vote[i];
    if (v != 0ull) atomicMax(S.slot + T.off + s_root[i], v);
  }
}

template <class L>
__global__ __launch_bounds__(256) void seg_sieve_final_kernel(SegSieveArgs S) {
  const SegCCArgs& A = S.cc;
  SEG_CC_PROLOGUE(A)
  const int n = T.h * T.w;
#pragma unroll
  for (int k = 0; k < SEG_CC_PIX / 256; ++k) {
    const int i = tid + 256 * k, ly = i / SEG_CC_TW, lx = i % SEG_CC_TW;
    if (ly >= T.th || lx >= T.tw) continue;
    const int64_t at = T.off + (T.y0 + ly) * T.w + T.x0 + lx;
    const int r = A.root[at];
    int b = seg_cc_labels<L>(A)[at];
    if (r >= 0 && r < n && A.area[T.off + r] < A.min_area) {
      const unsigned long long v = S.slot[T.off + r];
      if (v != 0ull) b = SegLabel<L>::TOP - (int)(v & (unsigned long long)SegLabel<L>::TOP);
      else if (S.orphan >= 0) b = S.orphan;
    }
    static_cast<L*>(S.out)[at] = (L)b;
  }
}
