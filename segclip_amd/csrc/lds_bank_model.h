// Bank-conflict model of an LDS read, shared by the build-time image checks (gemm_image_check.cpp,
// attention_image_check.cpp).  The documented rule: bank = (a / 4) mod 64; a lane occupies 4 banks (ds_read_b128) or 2
// (ds_read_b64_tr_b16); lanes conflict only within a group - ds_read_b128: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the
// same + 32; ds_read_b64_tr_b16: the two 32-lane halves; equal dwords broadcast; degree = most distinct dwords on one bank
// within a group.  ds_write_b64 (the parking stores of the attention kernels): 2 banks of 32 ((a / 4) mod 32) per lane, four
// groups of 16 contiguous lanes.  A MODEL, not a counter reading.  Host constexpr only, no code is emitted.
#pragma once

namespace ldsbank {

struct Wave { int a[64]; };   // the byte address every lane hands to one instruction
constexpr int b128_group(int l) {
  const int m = l & 31;
  return (l >> 5) * 2 + ((m < 4 || (m >= 12 && m < 16) || (m >= 20 && m < 28)) ? 0 : 1);
}
constexpr int half_group(int l) { return l >> 5; }
constexpr int quarter_group(int l) { return l >> 4; }
// ngroups lane groups, ndw dwords per lane, nbanks banks
constexpr int degree_of(const Wave& w, int ngroups, int ndw, int nbanks, int (*group)(int)) {
  int worst = 0;
  for (int g = 0; g < ngroups; ++g) {
    int dw[128] = {}, n = 0, cnt[64] = {};
    for (int l = 0; l < 64; ++l) {
      if (group(l) != g) continue;
      for (int d = 0; d < ndw; ++d) {
        const int x = w.a[l] / 4 + d;
        bool dup = false;
        for (int i = 0; i < n && !dup; ++i) dup = dw[i] == x;
        if (dup) continue;
        dw[n++] = x;
        if (++cnt[x % nbanks] > worst) worst = cnt[x % nbanks];
      }
    }
  }
  return worst;
}
// ds_read_b128 (b128) / ds_read_b64_tr_b16
constexpr int degree(const Wave& w, bool b128) { return b128 ? degree_of(w, 4, 4, 64, b128_group) : degree_of(w, 2, 2, 64, half_group); }
// ds_write_b64: 4 groups of 16 contiguous lanes, bank = (a / 4) mod 32
constexpr int degree_write_b64(const Wave& w) { return degree_of(w, 4, 2, 32, quarter_group); }

}  // namespace ldsbank
