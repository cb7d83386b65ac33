// Device helpers the bf16 GEMM families share for moving operand tiles through LDS: address-space types, the LDS-DMA
// piece pair, counted vmcnt waits, the scheduling-fenced barrier and the transpose-read fragment.  Where the bytes lie is
// stated in gemm_operand_image.h.
#pragma once
#include "common.h"
#include "gemm_operand_image.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) const char lds_cchar;
typedef __attribute__((address_space(3))) const bf16x8_t lds_bf16x8;

// Two LDS-DMA pieces (1 KiB each: lane l writes 16 B at lds + l*16) of one half-tile, issued from INLINE ASM on purpose:
// hipcc (ROCm 7.2) tracks an outstanding __builtin_amdgcn_global_load_lds as a pending LDS write and puts
// `s_waitcnt vmcnt(0)` in front of the next ds_read_b64_tr_b16 (the transpose-read builtin carries no alias
// information), which drains the whole ring every phase - the k-strided variants of gemm_bf16_dma.hip have exactly that
// wait in every K-step.  Hidden from the compiler, the DMA is ordered only by the counted vmcnt waits and barriers of its
// kernel.  Nothing here has a VGPR destination: an asm load into registers lets hipcc copy those registers before the data
// has landed.
//   s_nop 4: SGPR base written by SALU -> read by VMEM; s_nop 0: M0 written by SALU -> read by the LDS-DMA.
// M0 is not used by anything else in these kernels (no movrel / GWS), so it is not preserved.
__device__ __forceinline__ void dma16x2(const char* base_uniform, uint32_t off0, uint32_t off1, uint32_t lds0) {
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

template <int N> __device__ __forceinline__ void wait_vm() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  else static_assert(N < 0, "unsupported vmcnt");
}

// workgroup barrier that the compiler moves nothing across
#define GEMM_RING_BAR()                  \
  do {                                   \
    __builtin_amdgcn_sched_barrier(0);   \
    __builtin_amdgcn_s_barrier();        \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)

// fragment of a ks image: two ds_read_b64_tr_b16, at p (elements 0..3) and p + hi_off = 4 k-rows on (elements 4..7);
// p: char pointer, generic or LDS (opimg::frag_ks, opimg::tr16_source)
template <typename P> __device__ __forceinline__ bf16x8_t tr16_frag(P p, int hi_off) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + hi_off));
  s16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return __builtin_bit_cast(bf16x8_t, r);
}

// fragment reads of the 256 x 256 ring kernels (half-tiles of 128 rows: ks pitch 256 B): lane base from opimg::frag_*,
// everything else - ring buffer, half-tile, row block, k chunk - in the instruction's immediate OFF
template <int OFF> __device__ __forceinline__ bf16x8_t frag_direct_at(lds_cchar* base) {
  return *reinterpret_cast<lds_bf16x8*>(base + OFF);
}
template <int OFF> __device__ __forceinline__ bf16x8_t frag_ks_at(lds_cchar* base) { return tr16_frag(base + OFF, 4 * 256); }

}  // namespace
