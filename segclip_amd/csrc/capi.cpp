// C-ABI glue: version / error string / GEMM dispatch.  Compiled with hipcc like the kernels.
#include <stdarg.h>
#include <stdio.h>

#include "gemm_plan.h"

static thread_local char g_err[512] = "";

void segclip_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int segclip_version(void) { return SEGCLIP_ABI_VERSION; }
extern "C" const char* segclip_last_error_string(void) { return g_err; }

// reads of the planner (gemm_plan.cpp), which segclip_gemm consults through gemm_plan()
extern "C" size_t segclip_gemm_ws_bytes(const segclip_gemm_desc* d) { return gemm_splitk_ws_bytes(d); }
extern "C" int segclip_gemm_splits(const segclip_gemm_desc* d) { return gemm_splits(d); }
// the number of tail tiles a launch over `ntiles` 256 x 256 tiles runs as half-tiles (0 = none); its grid is ntiles + that
extern "C" int segclip_gemm_pq_half_tail(int64_t ntiles) { return gemm_pq_half_tail(ntiles); }

static const segclip_gemm_route NO_ROUTE = {SEGCLIP_GEMM_ROUTE_NONE, 0, 0, 0, 0, 0, 0};
static thread_local segclip_gemm_route g_route = NO_ROUTE;

void segclip_gemm_route_note(const segclip_gemm_route& route) { g_route = route; }

extern "C" int segclip_gemm_last_route(segclip_gemm_route* out) {
  if (out) *out = g_route;
  return g_route.family == SEGCLIP_GEMM_ROUTE_NONE ? SEGCLIP_ERR_UNSUPPORTED : 0;
}

extern "C" int segclip_gemm_plan(const segclip_gemm_desc* d, segclip_gemm_route* out, size_t* ws_bytes) {
  const GemmPlan p = gemm_plan(d);
  if (out) *out = p.route;
  if (ws_bytes) *ws_bytes = p.ws_bytes;
  return p.rc;
}

static thread_local segclip_attn_route g_attn_route = {SEGCLIP_ATTN_ROUTE_NONE, SEGCLIP_ATTN_ROUTE_NONE, 0, 0};

void segclip_attn_route_note(bool bwd, int kernel, int tiles, int variant) {
  g_attn_route = segclip_attn_route{bwd ? SEGCLIP_ATTN_ROUTE_NONE : kernel, bwd ? kernel : SEGCLIP_ATTN_ROUTE_NONE, tiles, variant};
}

extern "C" int segclip_attn_last_route(segclip_attn_route* out) {
  if (out) *out = g_attn_route;
  return g_attn_route.fwd_kernel == SEGCLIP_ATTN_ROUTE_NONE && g_attn_route.bwd_kernel == SEGCLIP_ATTN_ROUTE_NONE ? SEGCLIP_ERR_UNSUPPORTED : 0;
}

// plan (gemm_plan.cpp: every decision), note the route, one launcher per family, the trailing reductions
extern "C" int segclip_gemm(const segclip_gemm_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  g_route = NO_ROUTE;
  const GemmPlan p = gemm_plan(d);
  if (p.rc != 0 || p.route.family == SEGCLIP_GEMM_ROUTE_NONE) return p.rc;
  g_route = p.route;
  switch (p.route.family) {
    case SEGCLIP_GEMM_ROUTE_GENERIC: segclip_gemm_launch_generic(d, p, stream); break;
    case SEGCLIP_GEMM_ROUTE_DMA: segclip_gemm_launch_dma(d, p, stream); break;
    case SEGCLIP_GEMM_ROUTE_P8: segclip_gemm_launch_p8(d, p, stream); break;
    case SEGCLIP_GEMM_ROUTE_PQ: segclip_gemm_launch_pq(d, p, stream); break;
    default: segclip_gemm_launch_f32(d, p, stream);
  }
  SEGCLIP_CHECK_LAUNCH(p.route.family == SEGCLIP_GEMM_ROUTE_F32 ? "gemm_f32" : "gemm_bf16");
  return segclip_gemm_launch_reductions(d, p, stream);
}
