// ------------------------------- the LDS-DMA writer of the row image, one loader wave -------------------------------
// Included INSIDE the loader wave's scope of attention_pf.inc and attention_spl.inc, which provide `a` (kernel arguments with
// hd), `lane` and `T` (valid rows); it leaves them `lr` = lane >> 3, src_off and dma_tile.  Two lambdas and not functions of attention.hip: hipcc emits other code
// for both kernels when the same statements sit behind a function boundary.
// dma_tile brings np 8-row pieces of X[row * st + d] to LDS byte address dst.  Piece q: lane l -> row r = 8 q + (l >> 3), LDS
// chunk l & 7 <- source chunk (l & 7) ^ f(r) (tileimg::piece_row, tileimg::piece_chunk); a chunk beyond hd reads chunk 0, a row
// beyond T reads row T - 1 (tileimg::clamp_chunk, tileimg::clamp_row).  With ANY call inside src_off hipcc emits other code for
// both kernels, so f(r) is the ROW_XOR expression of attention.hip (held to the header there) and the two clamps and the piece
// rows stay spelled out, not checked by the build.
    // Source offsets: the swizzle term f(r) only depends on r & 15, i.e. on the parity of the piece: two lane constants
    // (even / odd pieces) + a uniform step per pair of pieces; only pieces that reach beyond row T clamp their rows.
    const int lr = lane >> 3;
    auto src_off = [&](int r, int64_t st) {
      int c = (lane & 7) ^ ROW_XOR(r);
      if (c * 8 >= a.hd) c = 0;
      const int rc = r < T ? r : T - 1;
      return (uint32_t)(((int64_t)rc * st + c * 8) * 2);
    };
    auto dma_tile = [&](const bf16_t* base, int64_t st, int np, uint32_t dst) {
      uint32_t o0 = src_off(lr, st), o1 = src_off(8 + lr, st);
      const uint32_t step = (uint32_t)(16 * st * 2);
      const int nfull = T >> 4;                             // pairs of pieces entirely below row T
      int q = 0;
      for (; q < 2 * nfull && q + 2 <= np; q += 2) {
        dma16x2(base, o0, o1, dst + q * 1024);
        o0 += step; o1 += step;
      }
      for (; q < np; ++q) dma16(base, src_off(q * 8 + lr, st), dst + q * 1024);
    };
