// Device helpers for moving tiles through LDS that the bf16 GEMM families and the attention kernels share: address-space
// types, the LDS-DMA pieces, the counted vmcnt wait and the transpose-read fragment.  Where the bytes lie is stated in
// gemm_operand_image.h and attention_tile_image.h.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) const char lds_cchar;
typedef __attribute__((address_space(3))) const bf16x8_t lds_bf16x8;

// LDS-DMA pieces (lane l writes 16 B at lds + l * 16: 1 KiB per wave instruction), issued from INLINE ASM on purpose:
// hipcc (ROCm 7.2) tracks an outstanding __builtin_amdgcn_global_load_lds as a pending LDS write and puts
// `s_waitcnt vmcnt(0)` in front of the next ds_read_b64_tr_b16 (the transpose-read builtin carries no alias
// information), which drains the whole ring every phase - the k-strided variants of gemm_bf16_dma.hip have exactly that
// wait in every K-step.  Hidden from the compiler, the DMA is neither counted nor waited for by hipcc: it is ordered only
// by the counted vmcnt waits and barriers of its kernel.  Nothing here has a VGPR destination: an asm load into registers
// lets hipcc copy those registers before the data has landed.
//   s_nop 4: SGPR base written by SALU -> read by VMEM; s_nop 0: M0 written by SALU -> read by the LDS-DMA.
// M0 is not used by anything else in these kernels (no movrel / GWS), so it is not preserved.
// one piece: 16 bytes per lane from base + off to LDS byte address lds_dst + 16 l
__device__ __forceinline__ void dma16(const void* base_uniform, uint32_t off, uint32_t lds_dst) {
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(off), "s"(base_uniform), "s"(lds_dst) : "memory");
}
// two pieces, to lds0 and lds0 + 1 KiB
__device__ __forceinline__ void dma16x2(const void* base_uniform, uint32_t off0, uint32_t off1, uint32_t lds0) {
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %2\n\t"
      "s_add_u32 m0, %3, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2"
      :
      : "v"(off0), "v"(off1), "s"(base_uniform), "s"(lds0)
      : "memory", "scc");
}
// one 256-byte piece: 4 bytes per lane from base + off to LDS byte address lds_dst + 4 l
__device__ __forceinline__ void dma4(const void* base_uniform, uint32_t off, uint32_t lds_dst) {
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" : : "v"(off), "s"(base_uniform), "s"(lds_dst) : "memory");
}

// s_waitcnt vmcnt(N): the instruction takes an immediate
template <int N> __device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt has 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory");
}
// ... for a wave-uniform run-time n (63 and above: 63)
template <int N = 0> __device__ __forceinline__ void wait_vm(uint32_t n) {
  if constexpr (N == 63) {
    wait_vm<63>();
  } else {
    if (n == N) wait_vm<N>();
    else wait_vm<N + 1>(n);
  }
}

// fragment of a transposed tile: two ds_read_b64_tr_b16, at p + off_lo (elements 0..3) and p + off_hi (elements 4..7);
// p: char pointer, generic or LDS (opimg::tr16_source: what a lane receives).  A caller that forms its second address only
// after the first read (the order of the statements is the order hipcc schedules from) uses the two halves itself.
template <typename P> __device__ __forceinline__ s16x4 tr16_read(P p) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p)); }
__device__ __forceinline__ bf16x8_t tr16_join(s16x4 lo, s16x4 hi) {
  s16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return __builtin_bit_cast(bf16x8_t, r);
}
template <typename P> __device__ __forceinline__ bf16x8_t tr16_frag(P p, int off_lo, int off_hi) {
  const s16x4 lo = tr16_read(p + off_lo);
  const s16x4 hi = tr16_read(p + off_hi);
  return tr16_join(lo, hi);
}
template <typename P> __device__ __forceinline__ bf16x8_t tr16_frag(P p, int hi_off) { return tr16_frag(p, 0, hi_off); }

}  // namespace
