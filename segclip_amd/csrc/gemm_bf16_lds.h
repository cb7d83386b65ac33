// Device helpers the bf16 GEMM families share for moving operand tiles through LDS: the scheduling-fenced barrier and the
// fragment reads of the ring kernels, on top of the LDS-DMA pieces, counted vmcnt waits and transpose-read fragment of
// lds_ops.h.  Where the bytes lie is stated in gemm_operand_image.h.
#pragma once
#include "common.h"
#include "gemm_operand_image.h"
#include "lds_ops.h"

namespace {

// workgroup barrier that the compiler moves nothing across
#define GEMM_RING_BAR()                  \
  do {                                   \
    __builtin_amdgcn_sched_barrier(0);   \
    __builtin_amdgcn_s_barrier();        \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)

// fragment reads of the 256 x 256 ring kernels (half-tiles of 128 rows: ks pitch 256 B): lane base from opimg::frag_*,
// everything else - ring buffer, half-tile, row block, k chunk - in the instruction's immediate OFF
template <int OFF> __device__ __forceinline__ bf16x8_t frag_direct_at(lds_cchar* base) {
  return *reinterpret_cast<lds_bf16x8*>(base + OFF);
}
template <int OFF> __device__ __forceinline__ bf16x8_t frag_ks_at(lds_cchar* base) { return tr16_frag(base + OFF, 4 * 256); }

}  // namespace
