// Build-time checks of the attention kernels' LDS tile images (attention_tile_image.h): nothing but static_asserts, no code
// is emitted.  A wrong image stops the build.  One assertion = one image, one configuration, one base.
//   1. writers land where the image says: LDS-DMA pieces, the register-staged stores, the u32x2 parking stores;
//   2. fragments hold the right elements (transposed ones: through opimg::tr16_source, what ds_read_b64_tr_b16 delivers);
//   3. the hinge: the rows a transposed fragment delivers as contraction index are the accumulator rows of the registers
//      pack8 puts at the same elements;
//   4. bank-conflict degree of every fragment read and of the parking stores by the rule of lds_bank_model.h.  A MODEL, not a
//      counter reading.
#include "attention_tile_image.h"
#include "lds_bank_model.h"

#ifndef __HIP_DEVICE_COMPILE__   // once, in the host pass
namespace {
using namespace tileimg;
using namespace ldsbank;
using opimg::TrSrc;
using opimg::tr16_source;

constexpr int TILE_ROWS = 256;   // the largest tile of the kernels (KCHUNK, TMAX)

// ---- 0. the images are injective: equal addresses mean equal elements ----------------------------------------------------
constexpr bool row_image_bijective() {
  bool seen[TILE_ROWS * ROWB / 2] = {};
  for (int r = 0; r < TILE_ROWS; ++r)
    for (int c = 0; c < 64; ++c) {
      const int a = swz(r, c);
      if (a < 0 || a >= TILE_ROWS * ROWB || a % 2 != 0 || a / ROWB != r || seen[a / 2]) return false;
      if (c % 8 == 0 && a != row_chunk(r, c / 8)) return false;
      seen[a / 2] = true;
    }
  return true;
}
constexpr bool scr_image_bijective() {
  bool seen[32 * SCRB / 2] = {};
  for (int r = 0; r < 32; ++r)
    for (int c = 0; c < 32; ++c) {
      const int a = swz64(r, c);
      if (a < 0 || a >= 32 * SCRB || a % 2 != 0 || a / SCRB != r || seen[a / 2]) return false;
      seen[a / 2] = true;
    }
  return true;
}
static_assert(row_image_bijective(), "row image: every element of a 256-row tile has its own address inside its row");
static_assert(scr_image_bijective(), "scratch image: every element of the 32 x 32 tile has its own address inside its row");

// ---- 1. writers ----------------------------------------------------------------------------------------------------------
constexpr bool pieces_land() {
  for (int q = 0; q < TILE_ROWS / 8; ++q)
    for (int l = 0; l < 64; ++l) {
      const int r = piece_row(q, l), c = piece_chunk(r, l & 7);
      if (r < 0 || r >= TILE_ROWS || c < 0 || c >= 8 || row_chunk(r, c) != q * 1024 + l * 16) return false;
    }
  return true;
}
// the clamps choose another SOURCE and never another place: in range they are the identity, out of range chunk 0 / row T - 1
constexpr bool piece_clamps_hold() {
  for (int hd = 8; hd <= 64; hd += 8)
    for (int c = 0; c < 8; ++c)
      if (clamp_chunk(c, hd) != (c * 8 + 8 <= hd ? c : 0)) return false;
  for (int T = 1; T <= TILE_ROWS; ++T)
    for (int r = 0; r < TILE_ROWS + 8; ++r)
      if (clamp_row(r, T) != (r < T ? r : T - 1)) return false;
  return true;
}
static_assert(pieces_land(), "row image: a DMA lane must fetch the chunk the image stores at q * 1024 + lane * 16");
static_assert(piece_clamps_hold(), "row image: the loaders' clamps are chunk 0 beyond the head dimension and row T - 1 beyond the sequence");

// stage_rows: nthreads threads, batches of 4 iterations; every chunk of the (padded) tile is written once, at its image address
constexpr bool stage_covers(int nthreads, int nrows) {
  bool seen[TILE_ROWS * 8] = {};
  const int total = nrows * 8;
  for (int base = 0; base < total; base += 4 * nthreads)
    for (int it = 0; it < 4; ++it)
      for (int tid = 0; tid < nthreads; ++tid) {
        const int idx = stage_index(base, it, nthreads, tid);
        if (idx >= total) continue;
        const int r = stage_row(idx), c = stage_chunk(idx), a = swz(r, c * 8);
        if (r >= nrows || a != row_chunk(r, c) || seen[a / 16]) return false;
        seen[a / 16] = true;
      }
  for (int i = 0; i < total; ++i)
    if (!seen[i]) return false;
  return true;
}
static_assert(stage_covers(64, 32), "stage_rows, 1 wave, 32 rows: every chunk once");
static_assert(stage_covers(192, 96), "stage_rows, 3 waves, 96 rows: every chunk once");
static_assert(stage_covers(448, 224), "stage_rows, 7 waves, 224 rows: every chunk once");
static_assert(stage_covers(512, 32), "stage_rows, 8 waves, 32 rows: every chunk once");
static_assert(stage_covers(512, 256), "stage_rows, 8 waves, 256 rows: every chunk once");

// parking stores of one wave: 64 lanes x 2 accumulators x 4 register groups, 8 bytes each, tile the 4-KB tile; what is stored
// at column park_col + u is register 4 rg + u, i.e. accumulator row acc_row(4 rg + u, lh) of half dt
constexpr bool parking_covers() {
  bool seen[32 * ROWB / 8] = {};
  for (int l = 0; l < 64; ++l)
    for (int dt = 0; dt < 2; ++dt)
      for (int rg = 0; rg < 4; ++rg) {
        const int a = park_at(l & 31, l >> 5, dt, rg);
        if (a < 0 || a >= 32 * ROWB || a % 8 != 0 || seen[a / 8]) return false;
        seen[a / 8] = true;
        for (int u = 0; u < 4; ++u)
          if (a + 2 * u != swz(l & 31, dt * 32 + acc_row(4 * rg + u, l >> 5))) return false;
      }
  for (int i = 0; i < 32 * ROWB / 8; ++i)
    if (!seen[i]) return false;
  return true;
}
constexpr bool parking_scr_covers() {
  bool seen[32 * SCRB / 8] = {};
  for (int l = 0; l < 64; ++l)
    for (int rg = 0; rg < 4; ++rg) {
      const int a = park64_at(l & 31, l >> 5, rg);
      if (a < 0 || a >= 32 * SCRB || a % 8 != 0 || seen[a / 8]) return false;
      seen[a / 8] = true;
      for (int u = 0; u < 4; ++u)
        if (a + 2 * u != swz64(l & 31, acc_row(4 * rg + u, l >> 5))) return false;
    }
  for (int i = 0; i < 32 * SCRB / 8; ++i)
    if (!seen[i]) return false;
  return true;
}
static_assert(parking_covers(), "row image: the u32x2 parking stores are disjoint, cover the tile and hold (lane row, accumulator row)");
static_assert(parking_scr_covers(), "scratch image: the u32x2 parking stores are disjoint, cover the tile and hold (lane row, accumulator row)");

// accumulator-format image: 8 quads x 64 lanes cover the 512 f32x4 of a slot once, and the quads walk both accumulators
constexpr bool accq_covers() {
  bool seen[512] = {}, reg[2][16] = {};
  for (int g8 = 0; g8 < 8; ++g8) {
    for (int l = 0; l < 64; ++l) {
      const int i = accq_index(g8, l);
      if (i < 0 || i >= 512 || seen[i]) return false;
      seen[i] = true;
    }
    for (int u = 0; u < 4; ++u) {
      if (accq_dt(g8) < 0 || accq_dt(g8) > 1 || reg[accq_dt(g8)][accq_reg(g8) + u]) return false;
      reg[accq_dt(g8)][accq_reg(g8) + u] = true;
    }
  }
  return true;
}
static_assert(accq_covers(), "accumulator-format image: every f32x4 of the 8-KB slot and every register of the pair once");

// ---- 2. fragments, 3. the hinge ------------------------------------------------------------------------------------------
constexpr bool frag_rows_holds(int rbase) {
  for (int kc = 0; kc < 4; ++kc)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j)
        if (frag_rows_at(rbase, kc, l) + 2 * j != swz(rbase + (l & 31), 16 * kc + 8 * (l >> 5) + j)) return false;
  return true;
}
// the address element j of lane l of a transposed fragment comes from: the one lane tr16_source(l, j & 3).lane supplied to the
// first (j < 4) or second read
constexpr int tr_elem(int rbase, int cbase, int l, int j) {
  const TrSrc s = tr16_source(l, j & 3);
  return frag_tr_at(rbase, cbase, s.lane, j >> 2) + s.byte;
}
constexpr int scr_elem(int rbase, int l, int j) {
  const TrSrc s = tr16_source(l, j & 3);
  return frag_tr64_at(rbase, s.lane, j >> 2) + s.byte;
}
// row k of {0..3, 8..11} + 4 (l >> 5), column l & 31: stated without acc_row
constexpr bool frag_tr_holds(int rbase) {
  for (int cbase = 0; cbase < 64; cbase += 32)
    for (int l = 0; l < 64; ++l) {
      if (frag_tr_at(rbase, cbase, l, 0) % 8 != 0 || frag_tr_at(rbase, cbase, l, 1) % 8 != 0) return false;
      for (int j = 0; j < 8; ++j)
        if (tr_elem(rbase, cbase, l, j) != swz(rbase + 4 * (l >> 5) + (j & 3) + 8 * (j >> 2), cbase + (l & 31))) return false;
    }
  return true;
}
constexpr bool frag_scr_holds(int rbase) {
  for (int l = 0; l < 64; ++l) {
    if (frag_tr64_at(rbase, l, 0) % 8 != 0 || frag_tr64_at(rbase, l, 1) % 8 != 0) return false;
    for (int j = 0; j < 8; ++j)
      if (scr_elem(rbase, l, j) != swz64(rbase + 4 * (l >> 5) + (j & 3) + 8 * (j >> 2), l & 31)) return false;
  }
  return true;
}
// The hinge.  A score tile S^T = K Q^T (or S = Q K^T) leaves the matrix pipe with register r of lane l holding contraction row
// acc_row(r, l >> 5) of the NEXT product; pack8(p + 8 half) puts registers 8 half + j at elements j = 0..7 of the other
// operand.  The transposed fragment of the 16-row block `half` of a 32-row tile must contract over the same rows, element by
// element and for both lane halves: row image (V, dO, Q, K tiles) and scratch image (the parked dS^T tile).
constexpr bool hinge_row_image(int tile) {
  for (int half = 0; half < 2; ++half)
    for (int cbase = 0; cbase < 64; cbase += 32)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j)
          if (tr_elem(tile + 16 * half, cbase, l, j) != swz(tile + acc_row(8 * half + j, l >> 5), cbase + (l & 31))) return false;
  return true;
}
constexpr bool hinge_scr_image() {
  for (int half = 0; half < 2; ++half)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j)
        if (scr_elem(16 * half, l, j) != swz64(acc_row(8 * half + j, l >> 5), l & 31)) return false;
  return true;
}
static_assert(hinge_scr_image(), "hinge, scratch image: frag_tr64 must contract over acc_row(8 half + j, lane >> 5), the rows pack8 puts at element j");

// ---- 4. bank-conflict degree (model) ---------------------------------------------------------------------------------------
// the degree every read of this base has (all kc / both column halves, both reads of a transpose pair), or -1 if they differ
constexpr int degree_rows(int rbase) {
  int deg = 0;
  for (int kc = 0; kc < 4; ++kc) {
    Wave w = {};
    for (int l = 0; l < 64; ++l) w.a[l] = frag_rows_at(rbase, kc, l);
    const int d = degree(w, true);
    if (kc > 0 && d != deg) return -1;
    deg = d;
  }
  return deg;
}
constexpr int degree_tr(int rbase) {
  int deg = 0;
  for (int cbase = 0; cbase < 64; cbase += 32)
    for (int h = 0; h < 2; ++h) {
      Wave w = {};
      for (int l = 0; l < 64; ++l) w.a[l] = frag_tr_at(rbase, cbase, l, h);
      const int d = degree(w, false);
      if ((cbase > 0 || h > 0) && d != deg) return -1;
      deg = d;
    }
  return deg;
}
constexpr int degree_scr(int rbase) {
  int deg = 0;
  for (int h = 0; h < 2; ++h) {
    Wave w = {};
    for (int l = 0; l < 64; ++l) w.a[l] = frag_tr64_at(rbase, l, h);
    const int d = degree(w, false);
    if (h > 0 && d != deg) return -1;
    deg = d;
  }
  return deg;
}

// the u32x2 parking stores (ds_write_b64), one per accumulator half and register group
constexpr int degree_park() {
  int deg = 0;
  for (int dt = 0; dt < 2; ++dt)
    for (int rg = 0; rg < 4; ++rg) {
      Wave w = {};
      for (int l = 0; l < 64; ++l) w.a[l] = park_at(l & 31, l >> 5, dt, rg);
      const int d = degree_write_b64(w);
      if ((dt > 0 || rg > 0) && d != deg) return -1;
      deg = d;
    }
  return deg;
}
constexpr int degree_park64() {
  int deg = 0;
  for (int rg = 0; rg < 4; ++rg) {
    Wave w = {};
    for (int l = 0; l < 64; ++l) w.a[l] = park64_at(l & 31, l >> 5, rg);
    const int d = degree_write_b64(w);
    if (rg > 0 && d != deg) return -1;
    deg = d;
  }
  return deg;
}
// 2 is what the images cost there: 16 lanes are 16 rows, and both swizzles repeat after 8 (row image: 8 slots of 16 B in the
// 128-byte bank window of a write; scratch image: 4 slots in each half of it)
static_assert(degree_park() == 2, "row image: modelled bank-conflict degree of the u32x2 parking stores (ds_write_b64)");
static_assert(degree_park64() == 2, "scratch image: modelled bank-conflict degree of the u32x2 parking stores (ds_write_b64)");

// one 32-row tile of the row image: frag_rows at its base, frag_tr at both of its 16-row blocks
#define CHECK_TILE(RBASE, DEG_ROWS, DEG_TR)                                                                                    \
  static_assert(frag_rows_holds(RBASE), "row image: frag_rows must hold (rbase + (lane & 31), 16 kc + 8 (lane >> 5) + j)");    \
  static_assert(frag_tr_holds(RBASE) && frag_tr_holds(RBASE + 16), "row image: frag_tr must deliver (rbase + 4 (lane >> 5) + {0..3, 8..11}, cbase + (lane & 31))"); \
  static_assert(hinge_row_image(RBASE), "hinge, row image: frag_tr must contract over acc_row(8 half + j, lane >> 5), the rows pack8 puts at element j"); \
  static_assert(degree_rows(RBASE) == DEG_ROWS, "row image: modelled bank-conflict degree of frag_rows (ds_read_b128)");         \
  static_assert(degree_tr(RBASE) == DEG_TR && degree_tr(RBASE + 16) == DEG_TR, "row image: modelled bank-conflict degree of frag_tr (ds_read_b64_tr_b16)")

CHECK_TILE(0, 1, 1); CHECK_TILE(32, 1, 1); CHECK_TILE(64, 1, 1); CHECK_TILE(96, 1, 1);
CHECK_TILE(128, 1, 1); CHECK_TILE(160, 1, 1); CHECK_TILE(192, 1, 1); CHECK_TILE(224, 1, 1);

static_assert(frag_scr_holds(0) && frag_scr_holds(16), "scratch image: frag_tr64 must deliver (rbase + 4 (lane >> 5) + {0..3, 8..11}, lane & 31)");
static_assert(degree_scr(0) == 1 && degree_scr(16) == 1, "scratch image: modelled bank-conflict degree of frag_tr64 (ds_read_b64_tr_b16)");

// what the kernels add to a lane offset as pointer steps / instruction immediates instead of calling the map again
constexpr bool immediates_hold() {
  for (int l = 0; l < 64; ++l) {
    for (int rbase = 0; rbase < TILE_ROWS; rbase += 16) {
      for (int kc = 0; kc < 4; ++kc)
        if (rbase % 32 == 0 && frag_rows_at(rbase, kc, l) != rbase * ROWB + frag_rows_at(0, kc, l)) return false;
      for (int cbase = 0; cbase < 64; cbase += 32)
        for (int h = 0; h < 2; ++h)
          if (frag_tr_at(rbase, cbase, l, h) != rbase * ROWB + frag_tr_at(0, cbase, l, h)) return false;
    }
    // scratch: rows + 8 are 512 B on (the swizzle looks at bits 1-2 of the row), 16-row blocks 1024 B
    if (frag_tr64_at(0, l, 1) != frag_tr64_at(0, l, 0) + 512 || frag_tr64_at(16, l, 0) != frag_tr64_at(0, l, 0) + 1024) return false;
    // the register-staged dO writer of the spl loader: piece q of lane l, even / odd pieces from two lane constants
    for (int q = 0; q < 28; ++q)
      if (swz(piece_row(q, l), (l & 7) * 8) != swz(piece_row(q & 1, l), (l & 7) * 8) - (q & 1) * 1024 + q * 1024) return false;
  }
  return true;
}
static_assert(immediates_hold(), "fragment maps: 16-row blocks must be rbase * 128 B (row image) / 1024 B, + 8 rows 512 B (scratch) from the lane constants");

}  // namespace
#endif
