// Build-time checks of the bf16 GEMM's LDS operand images (gemm_operand_image.h): nothing but static_asserts, no code is
// emitted.  A wrong image stops the build.  One assertion = one image, one configuration, one rbase.
//   1. writer and reader agree: what a lane of an LDS-DMA piece fetches is what the image stores where the lane lands;
//   2. fragments hold the right elements for both MFMA shapes (ks images: through the transpose-read model);
//   3. bank-conflict degree of every fragment read, by the rule of lds_bank_model.h.  A MODEL, not a counter reading;
//   4. the XCD chunking of workgroup ids is a bijection.
#include "gemm_operand_image.h"
#include "lds_bank_model.h"

#ifndef __HIP_DEVICE_COMPILE__   // once, in the host pass
namespace {
using namespace opimg;
using namespace ldsbank;

// ---- 1. writer and reader agree ------------------------------------------------------------------------------------------
constexpr bool pieces_direct_land(int npieces) {
  for (int idx = 0; idx < npieces; ++idx)
    for (int l = 0; l < 64; ++l) {
      const int row = piece_direct_row(idx, l), k = piece_direct_k(row, l);
      if (k < 0 || k >= 64 || k % 8 != 0 || direct_at(row, k) != idx * 1024 + l * 16) return false;
    }
  return true;
}
template <int ROWS> constexpr bool pieces_ks_land() {
  for (int idx = 0; idx < ROWS / 8; ++idx)
    for (int l = 0; l < 64; ++l) {
      const int krow = piece_ks_krow<ROWS>(idx, l), row = piece_ks_row<ROWS>(krow, l);
      if (krow >= 64 || row < 0 || row >= ROWS || row % 8 != 0 || ks_at<ROWS * 2, true>(krow, row) != idx * 1024 + l * 16) return false;
    }
  return true;
}
static_assert(pieces_direct_land(32), "direct image: a DMA lane must fetch the chunk the image stores at idx * 1024 + lane * 16");
static_assert(pieces_ks_land<128>(), "ks image, 128 rows: a DMA lane must fetch the chunk the image stores at idx * 1024 + lane * 16");
static_assert(pieces_ks_land<256>(), "ks image, 256 rows: a DMA lane must fetch the chunk the image stores at idx * 1024 + lane * 16");

// register-staged kernel (256 threads, 4 chunks each): thread tid stores chunk tid & 7 of rows (tid >> 3) + 32 i at its image
// address / chunk tid & 15 of k-rows (tid >> 4) + 16 i; every 16-byte slot of the tile is written once
constexpr bool sstore_direct_covers() {
  bool seen[1024] = {};
  for (int tid = 0; tid < 256; ++tid)
    for (int i = 0; i < 4; ++i) {
      const int r = (tid >> 3) + 32 * i, c = tid & 7, a = direct_chunk(r, c);
      if (a != direct_at(r, 8 * c) || a % 16 != 0 || a < 0 || a >= 16384 || seen[a / 16]) return false;
      seen[a / 16] = true;
    }
  return true;
}
constexpr bool sstore_ks_disjoint() {
  bool seen[64 * 20] = {};
  for (int tid = 0; tid < 256; ++tid)
    for (int i = 0; i < 4; ++i) {
      const int a = ks_at<320, false>((tid >> 4) + 16 * i, (tid & 15) * 8);
      if (a % 16 != 0 || a < 0 || a >= 64 * 320 || seen[a / 16]) return false;
      seen[a / 16] = true;
    }
  return true;
}
static_assert(sstore_direct_covers(), "direct image: the register-staged stores must write every chunk once, at its image address");
static_assert(sstore_ks_disjoint(), "ks image, pitch 320: the register-staged stores must not overlap");

// ---- 2. fragments --------------------------------------------------------------------------------------------------------
constexpr int frag_row(bool m16, int rbase, int l) { return rbase + (m16 ? (l & 15) : (l & 31)); }
constexpr int frag_k(bool m16, int kc, int l, int j) { return m16 ? 32 * kc + 8 * (l >> 4) + j : 16 * kc + 8 * (l >> 5) + j; }
constexpr int nkc(bool m16) { return m16 ? 2 : 4; }

template <bool M16> constexpr bool frag_direct_holds(int rbase) {
  constexpr bool m16 = M16;
  for (int kc = 0; kc < nkc(m16); ++kc)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j)
        if (frag_direct<M16>(rbase, kc, l) + 2 * j != direct_at(frag_row(m16, rbase, l), frag_k(m16, kc, l, j))) return false;
  return true;
}
// element j of lane l comes from the address lane tr16_source(l, j & 3).lane supplied to the first (j < 4) or second read
template <int PITCH, bool XOR, bool M16> constexpr bool frag_ks_holds(int rbase) {
  constexpr bool m16 = M16;
  for (int kc = 0; kc < nkc(m16); ++kc)
    for (int l = 0; l < 64; ++l) {
      if (frag_ks<PITCH, XOR, M16>(rbase, kc, l) % 8 != 0) return false;
      for (int j = 0; j < 8; ++j) {
        const TrSrc s = tr16_source(l, j & 3);
        const int a = frag_ks<PITCH, XOR, M16>(rbase, kc, s.lane) + (j >> 2) * 4 * PITCH + s.byte;
        if (a != ks_at<PITCH, XOR>(frag_k(m16, kc, l, j), frag_row(m16, rbase, l))) return false;
      }
    }
  return true;
}

// ---- 3. bank-conflict degree (model) -------------------------------------------------------------------------------------
// the degree every fragment read of this rbase has (all kc, both halves of a transpose read), or -1 if they differ
template <bool M16> constexpr int degree_direct(int rbase) {
  constexpr bool m16 = M16;
  int deg = 0;
  for (int kc = 0; kc < nkc(m16); ++kc) {
    Wave w = {};
    for (int l = 0; l < 64; ++l) w.a[l] = frag_direct<M16>(rbase, kc, l);
    const int d = degree(w, true);
    if (kc > 0 && d != deg) return -1;
    deg = d;
  }
  return deg;
}
template <int PITCH, bool XOR, bool M16> constexpr int degree_ks(int rbase) {
  constexpr bool m16 = M16;
  int deg = 0;
  for (int kc = 0; kc < nkc(m16); ++kc)
    for (int h = 0; h < 2; ++h) {
      Wave w = {};
      for (int l = 0; l < 64; ++l) w.a[l] = frag_ks<PITCH, XOR, M16>(rbase, kc, l) + h * 4 * PITCH;
      const int d = degree(w, false);
      if ((kc > 0 || h > 0) && d != deg) return -1;
      deg = d;
    }
  return deg;
}

#define CHECK_DIRECT(M16, RBASE, DEG)                                                                                     \
  static_assert(frag_direct_holds<M16>(RBASE), "direct image: the fragment must hold (rbase + lane row, k chunk of the lane)"); \
  static_assert(degree_direct<M16>(RBASE) == DEG, "direct image: modelled bank-conflict degree of ds_read_b128")
#define CHECK_KS(PITCH, XOR, M16, RBASE, DEG)                                                                             \
  static_assert(frag_ks_holds<PITCH, XOR, M16>(RBASE), "ks image: the transpose reads must deliver (rbase + lane row, k chunk of the lane)"); \
  static_assert(degree_ks<PITCH, XOR, M16>(RBASE) == DEG, "ks image: modelled bank-conflict degree of ds_read_b64_tr_b16")

// direct, 32x32x16: every family; rbase up to 224 (256-row tiles of gemm_bf16_dma.hip)
CHECK_DIRECT(false, 0, 1); CHECK_DIRECT(false, 32, 1); CHECK_DIRECT(false, 64, 1); CHECK_DIRECT(false, 96, 1);
CHECK_DIRECT(false, 128, 1); CHECK_DIRECT(false, 160, 1); CHECK_DIRECT(false, 192, 1); CHECK_DIRECT(false, 224, 1);
// direct, 16x16x32: gemm_bf16_pq.hip, half-tiles of 128 rows
CHECK_DIRECT(true, 0, 1); CHECK_DIRECT(true, 16, 1); CHECK_DIRECT(true, 32, 1); CHECK_DIRECT(true, 48, 1);
CHECK_DIRECT(true, 64, 1); CHECK_DIRECT(true, 80, 1); CHECK_DIRECT(true, 96, 1); CHECK_DIRECT(true, 112, 1);
// ks with XOR, pitch 256 B, 32x32x16: gemm_bf16_p8.hip, gemm_bf16_pq.hip (SEGCLIP_PQ_MFMA32), gemm_bf16_dma.hip at 128 rows
CHECK_KS(256, true, false, 0, 1); CHECK_KS(256, true, false, 32, 1); CHECK_KS(256, true, false, 64, 1); CHECK_KS(256, true, false, 96, 1);
// ks with XOR, pitch 512 B, 32x32x16: gemm_bf16_dma.hip at 256 rows
CHECK_KS(512, true, false, 0, 1); CHECK_KS(512, true, false, 32, 1); CHECK_KS(512, true, false, 64, 1); CHECK_KS(512, true, false, 96, 1);
CHECK_KS(512, true, false, 128, 1); CHECK_KS(512, true, false, 160, 1); CHECK_KS(512, true, false, 192, 1); CHECK_KS(512, true, false, 224, 1);
// ks with XOR, pitch 256 B, 16x16x32: gemm_bf16_pq.hip.  2 is the known cost of this image: a 32-lane half reads k-rows kr
// and kr + 8 of the same columns, which the 4-periodic XOR leaves on the same banks.  A conflict-free image flips this number.
CHECK_KS(256, true, true, 0, 2); CHECK_KS(256, true, true, 16, 2); CHECK_KS(256, true, true, 32, 2); CHECK_KS(256, true, true, 48, 2);
CHECK_KS(256, true, true, 64, 2); CHECK_KS(256, true, true, 80, 2); CHECK_KS(256, true, true, 96, 2); CHECK_KS(256, true, true, 112, 2);
// ks without XOR, pitch 320 B, 32x32x16: gemm_bf16.hip
CHECK_KS(320, false, false, 0, 1); CHECK_KS(320, false, false, 32, 1); CHECK_KS(320, false, false, 64, 1); CHECK_KS(320, false, false, 96, 1);

// what the ring kernels add to a lane base as instruction immediates instead of calling the map again
constexpr bool immediates_hold() {
  for (int l = 0; l < 64; ++l)
    for (int rbase = 0; rbase < 96; rbase += 16) {
      for (int kc = 0; kc < 4; ++kc) {
        if (frag_direct<false>(rbase + 32, kc, l) != frag_direct<false>(rbase, kc, l) + 4096) return false;
        if (frag_ks<256, true, false>(rbase, kc, l) != frag_ks<256, true, false>(rbase, 0, l) + kc * 4096) return false;
      }
      for (int kc = 0; kc < 2; ++kc) {
        if (frag_direct<true>(rbase + 16, kc, l) != frag_direct<true>(rbase, kc, l) + 2048) return false;
        if (frag_ks<256, true, true>(rbase, kc, l) != frag_ks<256, true, true>(rbase, 0, l) + kc * 8192) return false;
      }
      if (rbase % 32 == 0 && frag_ks<256, true, true>(rbase + 16, 0, l) != frag_ks<256, true, true>(rbase, 0, l) + 32) return false;
    }
  return true;
}
static_assert(immediates_hold(), "fragment maps: row-block and k-chunk steps must be the constants the ring kernels use as immediates");

// ---- 4. XCD chunking -----------------------------------------------------------------------------------------------------
constexpr bool xcd_bijective(int nwg) {
  bool seen[1000] = {};
  for (int b = 0; b < nwg; ++b) {
    const int u = xcd_chunked(b, nwg);
    if (u < 0 || u >= nwg || seen[u]) return false;
    seen[u] = true;
  }
  return true;
}
static_assert(xcd_bijective(1) && xcd_bijective(7) && xcd_bijective(8) && xcd_bijective(9) && xcd_bijective(255) &&
                  xcd_bijective(256) && xcd_bijective(1000),
              "XCD chunking must map [0, nwg) onto itself");

}  // namespace
#endif
