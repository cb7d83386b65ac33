// LDS operand images of the bf16 GEMM families (gemm_bf16.hip, gemm_bf16_dma.hip, gemm_bf16_p8.hip, gemm_bf16_pq.hip),
// stated once: where element (row, k) of an operand tile lies in LDS, which source chunk a lane of an LDS-DMA piece
// fetches, and which address a lane hands to the fragment read of an MFMA shape.  Plain constexpr functions of integers,
// no HIP builtins: the kernels use them on the device, gemm_image_check.cpp proves at build time that writer, image and
// reader agree and what bank-conflict degree the reads have.
//
// A K-tile is 64 k = 128 bytes = 8 chunks of 16 bytes (8 bf16) per operand row.
//
// direct image (k-contiguous operand X(row, k) = X[row * ld + k]): [rows][128 B].  Chunk c of row r is stored at slot
//   c ^ ((r >> 1) & 7).  A ds_read_b128 of a fragment takes one chunk index from 16 or 32 consecutive rows; unswizzled,
//   all of them would sit 128 B apart on 2 x 4 of the 64 banks.  The XOR spreads 8 row pairs over the 8 slots of a row,
//   and the two rows of a pair lie in the two halves of the 256-byte bank window.
// ks image (k-strided operand X(row, k) = X[k * ld + row]): [64 k-rows][PITCH B], a chunk is 8 ROWS of one k-row.  Chunk c
//   of k-row kr is stored at slot c ^ ((kr & 3) << 2).  It is read with two ds_read_b64_tr_b16 (k-rows +0..3, +4..7); the
//   4 k-rows a 16-lane group addresses are a multiple of 256 B apart, i.e. on the same banks, and the XOR moves them to
//   the 4 quadrants (16 banks each) of the bank window.  The register-staged kernel pads its k-rows to 320 B instead
//   (consecutive k-rows 16 banks apart) and applies no XOR.
// Why the swizzle sits on the SOURCE address: an LDS-DMA write (global_load_lds_dwordx4) is lane-linear - lane l of piece
//   idx (1 KiB) lands at idx * 1024 + l * 16, whatever it fetched.  So the lane that owns slot s of a row fetches the
//   chunk that the image stores at s: the same XOR, applied to the chunk index of the global address.
//
// The conflict degrees asserted in gemm_image_check.cpp are this MODEL (bank = (a / 4) mod 64, fixed lane groups, equal
// dwords broadcast) applied to these maps.  They have not been confirmed with a hardware counter.
//
// The kernels call these functions wherever that leaves their code as it was.  A function boundary changes the order in which
// hipcc simplifies an address, and with it the emitted code; where that happens the kernel spells the same arithmetic out in a
// constexpr helper that computes nothing but offsets, and a static_assert beside it holds the helper to these functions over
// its whole domain: sstore_direct / sstore_ks of gemm_bf16.hip, issue_ks / frag_direct / frag_ks of gemm_bf16_dma.hip,
// off_direct of gemm_bf16_p8.hip, fragbase_ks of gemm_bf16_pq.hip.  An image change starts here; the build then names every
// copy that no longer agrees.  The one thing spelled out and NOT checked by the build: two XCD expressions in pq_main of
// gemm_bf16_pq.hip (they read gridDim / blockIdx), marked there.
#pragma once

// always_inline: left to its cost model, hipcc keeps some of these as calls inside the large kernels; a call returns in a
// vector register, and a workgroup-uniform value (the tile base of an LDS-DMA) must stay in scalar ones
#define OPIMG_FN constexpr __attribute__((always_inline))

namespace opimg {

// ---- images: LDS byte address --------------------------------------------------------------------------------------
OPIMG_FN int direct_xor(int r) { return (r >> 1) & 7; }     // slot = chunk ^ this, for row r
OPIMG_FN int ks_xor(int kr) { return (kr & 3) << 2; }        // slot = chunk ^ this, for k-row kr

OPIMG_FN int direct_chunk(int r, int c) { return r * 128 + ((c ^ direct_xor(r)) << 4); }      // chunk c of row r
OPIMG_FN int direct_at(int row, int k) { return direct_chunk(row, k >> 3) + ((k & 7) << 1); }  // element (row, k)

// element (row, k-row kr); row = 8 * chunk for a whole chunk.  PITCH 256 / 512 with XOR: the LDS-DMA families at 128 / 256
// rows; PITCH 320 without: the register-staged kernel
template <int PITCH, bool XOR> OPIMG_FN int ks_at(int kr, int row) {
  return XOR ? kr * PITCH + ((((row >> 3) ^ ks_xor(kr))) << 4) + ((row & 7) << 1) : kr * PITCH + row * 2;
}

// ---- LDS-DMA piece maps: what lane `lane` of piece `idx` must fetch so that it lands in place ----------------------------
// direct: a piece = 8 rows of 128 B; the lane fetches the 8 elements from k = piece_direct_k of operand row piece_direct_row
OPIMG_FN int piece_direct_row(int idx, int lane) { return idx * 8 + (lane >> 3); }
OPIMG_FN int piece_direct_k(int row, int lane) { return ((lane & 7) ^ direct_xor(row)) * 8; }
// ks with ROWS = 128 / 256 rows: a piece = 512 / ROWS k-rows of ROWS * 2 B; the lane fetches the 8 rows from piece_ks_row of
// k-row piece_ks_krow
template <int ROWS> OPIMG_FN int piece_ks_krow(int idx, int lane) {
  static_assert(ROWS == 128 || ROWS == 256, "k-strided DMA images have 128 or 256 rows");
  return idx * (512 / ROWS) + (lane >> (ROWS == 128 ? 4 : 5));
}
template <int ROWS> OPIMG_FN int piece_ks_row(int krow, int lane) { return ((lane & (ROWS / 8 - 1)) ^ ks_xor(krow)) * 8; }

// ---- fragment maps: the byte offset lane `lane` hands to the read -------------------------------------------------------
// Fragment of lane l, element j = 0..7:   32x32x16 (M16 = false): (rbase + (l & 31), 16 kc + 8 (l >> 5) + j)
//                                         16x16x32 (M16 = true) : (rbase + (l & 15), 32 kc + 8 (l >> 4) + j)
// direct image, ds_read_b128.  The XOR repeats every 16 rows: blocks of 16 rows of one base are 2048 B apart.
template <bool M16> OPIMG_FN int frag_direct(int rbase, int kc, int lane) {
  const int r = rbase + (M16 ? (lane & 15) : (lane & 31));
  const int c = M16 ? kc * 4 + (lane >> 4) : kc * 2 + (lane >> 5);
  return direct_chunk(r, c);
}
// ks image, ds_read_b64_tr_b16 at this offset (elements 0..3) and at + 4 * PITCH (elements 4..7): lane 4 i + p of 16-lane
// group g4 addresses k-row i, rows 4 p .. 4 p + 3 of its group's block.  32x32x16: group g4 = k half g4 >> 1, 16-row half
// g4 & 1.  16x16x32: group g4 = k-rows 8 g4 ..  A k chunk is a pure k-row offset (it does not enter the XOR):
// + kc * 16 * PITCH (32x32x16) / + kc * 32 * PITCH (16x16x32); the next 16 rows are 32 B on.
template <int PITCH, bool XOR, bool M16> OPIMG_FN int frag_ks(int rbase, int kc, int lane) {
  const int g4 = lane >> 4, q = lane & 15;
  const int krow = M16 ? kc * 32 + 8 * g4 + (q >> 2) : kc * 16 + 8 * (g4 >> 1) + (q >> 2);
  const int col = M16 ? rbase + 4 * (q & 3) : rbase + 16 * (g4 & 1) + 4 * (q & 3);
  return ks_at<PITCH, XOR>(krow, col);
}

// ---- what ds_read_b64_tr_b16 delivers ----------------------------------------------------------------------------------
// Within a 16-lane group, lane s supplies the address of 4 consecutive b16 of k-row s >> 2 of a 4 x 16 block; lane q receives
// column q of the block.  So element j = 0..3 of lane l is b16 number l & 3 at the address that lane
// (l & ~15) + 4 j + ((l & 15) >> 2) supplied.
struct TrSrc { int lane, byte; };
OPIMG_FN TrSrc tr16_source(int lane, int j) { return TrSrc{(lane & ~15) + 4 * j + ((lane & 15) >> 2), (lane & 3) * 2}; }

// ---- workgroup ids ------------------------------------------------------------------------------------------------------
// Workgroup b runs on XCD b % 8.  A sequence of nwg units is cut into 8 contiguous chunks, one per XCD (the first nwg % 8 one
// longer), so that neighbouring units - tiles that share an A row slab or a B column slab - sit behind one L2.  A bijection of
// [0, nwg).
OPIMG_FN int xcd_chunked(int bid, int nwg) {
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

}  // namespace opimg
