// LDS tile images of the bf16 attention kernels (attention.hip and its attention_*.inc files), stated once: where element
// (row, col) of a tile lies in LDS, which source chunk a lane of an LDS-DMA piece fetches, which address a lane hands to a
// fragment read, and which score an accumulator register holds.  Plain constexpr functions of integers, no HIP builtins:
// the kernels use them on the device, attention_image_check.cpp proves at build time that writers, images and readers
// agree and what bank-conflict degree the fragment reads have (a MODEL, see lds_bank_model.h; no counter reading).
//
// row image: [rows][128 B], a row is 64 bf16 = 8 chunks of 16 bytes (head_dim <= 64; Q, K, V, dO, O tiles, and the bf16
//   tiles parked on their way out).  Chunk c of row r is stored at slot c ^ f(r), f = rotr3((r >> 1) & 7).  f repeats every
//   16 rows: blocks of 16 rows are 2048 B apart, which the kernels use as instruction immediates.
// scratch image: [32 keys][64 B], 4 chunks per row (the dS^T tile of one wave, and the dQ half-tiles on their way out).
//   Chunk c of row r is stored at slot c ^ ((r >> 1) & 3).
// Both are read two ways: as rows (ds_read_b128: lane -> one row, 8 consecutive elements) and transposed (two
//   ds_read_b64_tr_b16: lane -> one COLUMN, 8 rows).
// The hinge of every bf16 kernel: the rows a transposed fragment delivers as elements 0..7 are
//   4 * (lane >> 5) + {0..3, 8..11} = acc_row(j, lane >> 5), the rows that registers 0..7 of a 32x32 accumulator hold for
//   the same lane half.  So a score tile leaves the matrix pipe in exactly the key order in which the transposed V, dO, Q,
//   K fragments contract: pack8 of accumulator registers IS the other operand, and P^T and dS^T never leave registers.
// As in gemm_operand_image.h the swizzle of an LDS-DMA write sits on the SOURCE address (the write is lane-linear), and a
// kernel calls these functions wherever that leaves its code as it was.  hipcc is touchy here: a function that calls another
// one, or that takes the lane where the kernel already holds lane & 31 and lane >> 5, changes the emitted code.  Hence the maps
// of sub-expressions (frag_tr_row / _col / _hi, frag_rows_col, park_col) that the kernels put around their own swz, next to the
// composed maps (frag_tr_at, frag_rows_at, park_at) the checks are stated on.  What could not become a call stays spelled out
// in attention.hip (TR_LANE_OFF, ROW_XOR), held to this header by a *_follows_image static_assert; the few places that are
// neither are marked where they stand.  An image change starts here; the build then names what no longer agrees.
#pragma once
#include "gemm_operand_image.h"   // OPIMG_FN (why always_inline: see there), opimg::tr16_source

namespace tileimg {

constexpr int ROWB = 128;   // bytes per row of the row image
constexpr int SCRB = 64;    // bytes per row of the scratch image

// ---- images: LDS byte address --------------------------------------------------------------------------------------------
// ds_read_b128 of 16 rows is conflict-free under f, and the 4-row transpose reads of a 32-lane half land in disjoint banks
// (swz is written in one piece, its f not a function of its own: the kernels call it several hundred times, and hipcc emits
// other code for a call that itself calls)
OPIMG_FN int swz(int row, int col) {   // element (row, col) of the row image
  const int t = (row >> 1) & 7;
  const int f = ((t & 1) << 2) | (t >> 1);
  return row * ROWB + ((((col >> 3) ^ f)) << 4) + ((col & 7) << 1);
}
OPIMG_FN int row_xor(int r) { return (swz(r, 0) - r * ROWB) >> 4; }                                  // f(r): the slot of chunk 0
OPIMG_FN int row_chunk(int r, int c) { return r * ROWB + ((c ^ row_xor(r)) << 4); }                   // chunk c of row r
OPIMG_FN int swz64(int row, int col) { return row * SCRB + ((((col >> 3) ^ ((row >> 1) & 3))) << 4) + ((col & 7) << 1); }   // scratch image

// ---- LDS-DMA piece map of the row image -------------------------------------------------------------------------------
// Piece q is 8 rows (1 KiB): lane `lane` lands at q * 1024 + lane * 16, i.e. in slot lane & 7 of row piece_row, and must
// fetch the chunk the image stores there.  On top of the map the loaders clamp: a chunk beyond the head dimension reads
// chunk 0 and a row beyond the sequence reads row T - 1 (finite duplicates, masked or multiplied by zero by the kernel -
// never whole rows beyond hd, which once read past the end of the tensor).
OPIMG_FN int piece_row(int q, int lane) { return q * 8 + (lane >> 3); }
OPIMG_FN int piece_chunk(int r, int slot) { return slot ^ row_xor(r); }                   // slot = lane & 7
OPIMG_FN int clamp_chunk(int c, int hd) { return c * 8 < hd ? c : 0; }
OPIMG_FN int clamp_row(int r, int T) { return r < T ? r : T - 1; }

// ---- register-staged writer (stage_rows and the loops written like it) -----------------------------------------------------
// thread tid of nthreads, iteration it of a batch starting at chunk index base: one 16-byte chunk
OPIMG_FN int stage_index(int base, int it, int nthreads, int tid) { return base + it * nthreads + tid; }
OPIMG_FN int stage_row(int idx) { return idx >> 3; }
OPIMG_FN int stage_chunk(int idx) { return idx & 7; }

// ---- accumulator maps -------------------------------------------------------------------------------------------------
// 32x32 accumulator (v_mfma_f32_32x32x16_bf16): register r of lane l holds C[acc_row(r, l >> 5)][l & 31]
OPIMG_FN int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// accumulator-format image of a [64 d][32 q] fp32 tile pair (dQ^T of one query tile, 8 KB): [8 quads][64 lanes] f32x4.
// Quad g8 of a lane = registers accq_reg(g8) .. + 3 of its accumulator accq_dt(g8) (the 32-column half of d)
OPIMG_FN int accq_index(int g8, int lane) { return g8 * 64 + lane; }    // in units of f32x4
OPIMG_FN int accq_dt(int g8) { return g8 >> 2; }
OPIMG_FN int accq_reg(int g8) { return (g8 & 3) * 4; }
// u32x2 parking store of a transposed accumulator pair into a row-image tile [32 rows][64 d]: lane (li = l & 31, lh = l >> 5)
// packs registers 4 rg .. 4 rg + 3 of accumulator dt (d = 32 dt + acc_row(4 rg + u, lh)) into 8 bytes of row li
OPIMG_FN int park_col(int dt, int rg, int lh) { return dt * 32 + 8 * rg + 4 * lh; }
OPIMG_FN int park_at(int li, int lh, int dt, int rg) { return swz(li, park_col(dt, rg, lh)); }
// the same into the scratch image, one 32-column half
OPIMG_FN int park64_at(int li, int lh, int rg) { return swz64(li, park_col(0, rg, lh)); }

// ---- fragment maps: the byte offset lane `lane` hands to the read ------------------------------------------------------
// frag_rows, ds_read_b128: element j of lane l is (rbase + (l & 31), 16 kc + 8 (l >> 5) + j)
// (koff of the kernels: swz(lane & 31, frag_rows_col), the tile's rows in the pointer)
OPIMG_FN int frag_rows_col(int kc, int lh) { return kc * 16 + 8 * lh; }
OPIMG_FN int frag_rows_at(int rbase, int kc, int lane) { return swz(rbase + (lane & 31), frag_rows_col(kc, lane >> 5)); }
// frag_tr, two ds_read_b64_tr_b16 (hi = 0: elements 0..3, hi = 1: elements 4..7): element j of lane l is
// (rbase + acc_row(j, l >> 5), cbase + (l & 31)).  Lane 4 i + p of a 16-lane group g4 addresses row 4 (g4 >> 1) + i, columns
// 4 p .. 4 p + 3 of the group's 16 columns; the second read is 8 rows on.  toff / voff of the kernels: rbase = 0, the tile's
// 16-row block in the pointer
OPIMG_FN int frag_tr_row(int rbase, int lane) {
  const int g4 = lane >> 4, q = lane & 15;
  return rbase + 4 * (g4 >> 1) + (q >> 2);
}
OPIMG_FN int frag_tr_col(int cbase, int lane) {
  const int g4 = lane >> 4, q = lane & 15;
  return cbase + 16 * (g4 & 1) + 4 * (q & 3);
}
OPIMG_FN int frag_tr_hi(int row) { return row + 8; }
OPIMG_FN int frag_tr_at(int rbase, int cbase, int lane, int hi) {
  const int row = frag_tr_row(rbase, lane), col = frag_tr_col(cbase, lane);
  return hi ? swz(frag_tr_hi(row), col) : swz(row, col);
}
// frag_tr64, the same on the scratch image (32 columns)
OPIMG_FN int frag_tr64_at(int rbase, int lane, int hi) {
  const int row = frag_tr_row(rbase, lane), col = frag_tr_col(0, lane);
  return hi ? swz64(frag_tr_hi(row), col) : swz64(row, col);
}

}  // namespace tileimg
