// Kernel selection of segclip_gemm (gemm_plan.cpp): which of the five kernel families runs a descriptor, on which tiles, with
// how many K splits - or which error the call returns.  The planner makes no HIP call and reads no memory; the launchers
// (one per family, in the kernel files) fill their argument structs from the descriptor and the plan and decide nothing.
#pragma once
#include "common.h"

// tile constants the planner shares with the kernels
constexpr int GEMM_BK = 64;        // K step of every bf16 kernel; K ranges of a split-K launch are multiples of it
constexpr int GEMM_TILE = 128;     // register-staged kernel (gemm_bf16.hip): 128 x 128
constexpr int GEMM_BIG_TILE = 256; // 256-row tiles of gemm_bf16_dma.hip, 256 x 256 of gemm_bf16_p8.hip / gemm_bf16_pq.hip

// epilogue modes of gemm_bf16_pq.hip (bits 0-3 of its route variant)
enum { PQ_PLAIN = 0, PQ_RES = 1, PQ_ACT8 = 2, PQ_DACT8 = 3, PQ_SLAB = 4, PQ_RES32 = 5, PQ_ACT8E = 6 };
// PQ_ACT8E: PQ_ACT8 with the erf-GELU of the MAE decoders (modules/module_mae.py:110-134: timm Block, nn.GELU) instead of QuickGELU
// route variants of gemm_bf16_dma.hip (DMA_128x128: 4 waves, for problems too small to fill the chip with 256-row tiles; 1 was
// the retired 256 x 256 instance, and the route tables of the tests hold the other two values) ...
enum { DMA_256x128 = 0, DMA_128x128 = 2 };
// ... and of gemm_f32.hip
enum { F32_32x128 = 0, F32_64x64 = 1, F32_128x128 = 2 };

struct GemmPlan {
  int rc = 0;                  // what segclip_gemm returns before launching: 0, SEGCLIP_ERR_INVALID or SEGCLIP_ERR_UNSUPPORTED
                               // (the message is set through segclip_set_error)
  segclip_gemm_route route = {SEGCLIP_GEMM_ROUTE_NONE, 0, 0, 0, 0, 0, 0};   // as segclip_gemm_last_route reports it; NONE with
                               // rc 0: nothing to launch (M or N = 0)
  size_t ws_bytes = 0;         // the workspace that enables split-K (segclip_gemm_ws_bytes)
  // what the launchers need beyond the route
  int64_t nb = 1;              // nb1 * nb2: grid.z
  int nbx = 0, nby = 0;        // tiles along n / m
  int64_t kper = 0;            // K elements per split (K itself without split-K)
  int vec_epi = 0;             // dma / p8: every C / aux / residual / bias access of a full tile may be a 16-byte vector
  bool colsum = false;         // the epilogue writes partial column sums to colsum_ws
  int pq_mode = PQ_PLAIN;      // pq: epilogue mode, the half-tile tail (PQArgs::nfull / half_r / half_x) and the workgroup count
  int nfull = 0, half_r = 0, half_x = 0;
  unsigned nwg = 0;
};

// The plan of segclip_gemm(d): a pure function of the descriptor - it reads no environment variable and keeps no state.  Of the
// pointers, ws and colsum_ws it reads presence and alignment only.
GemmPlan gemm_plan(const segclip_gemm_desc* d);
// the same for a descriptor with fp32 operands that is known to be valid (attention.hip's fp32 path)
GemmPlan gemm_plan_f32(const segclip_gemm_desc* d);
// pieces of the plan that the ABI also answers on their own (segclip_gemm_ws_bytes, segclip_gemm_splits,
// segclip_gemm_pq_half_tail); gemm_plan uses the same functions
size_t gemm_splitk_ws_bytes(const segclip_gemm_desc* d);
int gemm_splits(const segclip_gemm_desc* d);
int gemm_pq_half_tail(int64_t ntiles);

// One launcher per family: fills the kernel's argument struct from the descriptor and the plan, and launches.
void segclip_gemm_launch_generic(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream);   // gemm_bf16.hip
void segclip_gemm_launch_dma(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream);       // gemm_bf16_dma.hip
void segclip_gemm_launch_p8(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream);        // gemm_bf16_p8.hip
void segclip_gemm_launch_pq(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream);        // gemm_bf16_pq.hip
void segclip_gemm_launch_f32(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream);       // gemm_f32.hip
// the trailing launches of a planned GEMM: column-sum reduction and split-K combine, unless deferred (gemm_bf16.hip)
int segclip_gemm_launch_reductions(const segclip_gemm_desc* d, const GemmPlan& p, hipStream_t stream);
// the function table of a family's four operand layouts, indexed by a_ks * 2 + b_ks (ff, fk, kf, kk)
typedef void (*gemm_layout_launcher)(const segclip_gemm_desc*, const GemmPlan&, hipStream_t);
inline int gemm_layout_index(const GemmPlan& p) { return p.route.a_ks * 2 + p.route.b_ks; }
