// Launch executors: the launch SEQUENCE of one pre-LN residual attention block, enqueued by ONE C-ABI call.
// Reference: modules/module_seg_vit.py:175-196, modules/module_clip_ttransformer.py:20-37 (ResidualAttentionBlock.forward:
//   x += out_proj(MHA(ln_1 x));  x += c_proj(QuickGELU(c_fc(ln_2 x)))).
// No new kernel: segclip_resblock_fwd issues exactly the launches ops._resblock_fwd issues through the Python layer
// (LayerNorm, in_proj GEMM + bias, attention forward, out_proj GEMM + bias + residual, LayerNorm, c_fc GEMM + bias + activation
// + saved derivative, c_proj GEMM + bias + residual), with the same descriptors, into caller-owned buffers - results are
// bit-identical (tests/test_block_exec_gpu.py).  What it removes is host time: a launch costs 10-11 us through the Python layer (ctypes descriptor fill,
// torch.empty, checks) and the training step has ~590 of them; at the reference recipe's 96 samples per GPU (and below) the
// step is bound by that enqueue time, not by the GPU.
#include <initializer_list>

#include "common.h"
#include "gemm_plan.h"

namespace {

void gemm_base(segclip_gemm_desc& g, const void* A, int64_t lda, const void* W, int64_t ldw, void* Cc, int64_t ldc, int c_dtype,
               const float* bias, int64_t M, int64_t N, int64_t K) {
  g = segclip_gemm_desc{};
  g.A = A; g.B = W; g.C = Cc; g.bias = bias;
  g.M = M; g.N = N; g.K = K;
  g.sam = lda; g.sak = 1; g.sbn = ldw; g.sbk = 1;
  g.ldc = ldc; g.ldaux = N;
  g.nb1 = 1; g.nb2 = 1;
  g.a_dtype = SEGCLIP_BF16; g.b_dtype = SEGCLIP_BF16; g.c_dtype = c_dtype; g.r_dtype = SEGCLIP_F32;
  g.act = SEGCLIP_ACT_NONE; g.alpha = 1.0f;
}

}  // namespace

// Refusal precedes launch: the four GEMM descriptors are built and planned (gemm_plan.h: a pure host function) before anything
// is enqueued, and the first refusal is returned with its message - SEGCLIP_ERR_UNSUPPORTED from this call means "nothing was
// launched", as from segclip_gemm.  Not separated from their launches (both are SEGCLIP_ERR_INVALID, argument errors no other
// path would accept either): segclip_layernorm_fwd's column limits (D % 4, D <= its register budget) and segclip_attn_fwd's
// shape checks (head_dim <= 64; head_dim and strides multiples of 8).
extern "C" int segclip_resblock_fwd(const segclip_resblock_fwd_desc* d, void* stream) {
  SEGCLIP_REQUIRE(d != nullptr, "resblock_fwd: null descriptor");
  SEGCLIP_REQUIRE(d->M >= d->B * d->T && d->B > 0 && d->T > 0 && d->D > 0 && d->F > 0 && d->H > 0 && d->D % d->H == 0,
                  "resblock_fwd: bad sizes");
  SEGCLIP_REQUIRE(d->x && d->y1 && d->qkv && d->o && d->stats && d->x1 && d->y2 && d->h && d->xo && d->mean1 && d->rstd1 &&
                  d->mean2 && d->rstd2, "resblock_fwd: null buffer");
  SEGCLIP_REQUIRE(d->x_dtype == SEGCLIP_F32 || d->x_dtype == SEGCLIP_BF16, "resblock_fwd: residual stream must be f32 or bf16");
  const int64_t M = d->M, D = d->D, F = d->F, hd = D / d->H;
  segclip_gemm_desc in_proj, out_proj, c_fc, c_proj;
  gemm_base(in_proj, d->y1, D, d->wqkv, D, d->qkv, 3 * D, SEGCLIP_BF16, d->bqkv, M, 3 * D, D);
  // out_proj + residual
  gemm_base(out_proj, d->o, D, d->wo, D, d->x1, D, d->x_dtype, d->bo, M, D, D);
  out_proj.residual = d->x; out_proj.ldr = D; out_proj.r_dtype = d->x_dtype;
  // c_fc + activation (+ what the backward needs of the pre-activation)
  gemm_base(c_fc, d->y2, D, d->wfc, D, d->h, d->ld_h, SEGCLIP_BF16, d->bfc, M, F, D);
  c_fc.act = d->act; c_fc.aux = d->u; c_fc.ldaux = d->u ? d->ld_u : F; c_fc.aux_kind = d->aux_kind;
  // c_proj + residual
  gemm_base(c_proj, d->h, d->ld_h, d->wpr, F, d->xo, D, d->x_dtype, d->bpr, M, D, F);
  c_proj.residual = d->x1; c_proj.ldr = D; c_proj.r_dtype = d->x_dtype;
  int rc;
  for (const segclip_gemm_desc* g : {&in_proj, &out_proj, &c_fc, &c_proj})
    if ((rc = gemm_plan(g).rc)) return rc;
  // ln_1
  rc = segclip_layernorm_fwd(d->x, d->ln1w, d->ln1b, d->y1, d->mean1, d->rstd1, M, D, d->eps, d->x_dtype, SEGCLIP_BF16, stream);
  if (rc) return rc;
  if ((rc = segclip_gemm(&in_proj, stream))) return rc;
  // attention core on the packed (M, 3D) projection; pad rows of a row-padded stack stay zero
  if (M > d->B * d->T) {
    hipError_t e = hipMemsetAsync((char*)d->o + (size_t)d->B * d->T * D * 2, 0, (size_t)(M - d->B * d->T) * D * 2, (hipStream_t)stream);
    SEGCLIP_REQUIRE(e == hipSuccess, "resblock_fwd: memset failed: %s", hipGetErrorString(e));
  }
  segclip_attn_desc a = segclip_attn_desc{};
  a.Q = d->qkv; a.K = (const char*)d->qkv + (size_t)D * 2; a.V = (const char*)d->qkv + (size_t)2 * D * 2; a.O = d->o;
  a.stats = d->stats;
  a.B = d->B; a.H = d->H; a.Tq = d->T; a.Tk = d->T; a.hd = hd;
  a.q_sb = a.k_sb = a.v_sb = d->T * 3 * D; a.q_st = a.k_st = a.v_st = 3 * D;
  a.o_sb = d->T * D; a.o_st = D;
  a.scale = d->attn_scale; a.causal = d->causal; a.dtype = SEGCLIP_BF16; a.flags = 0;
  a.klen = (decltype(a.klen))d->klen;
  if ((rc = segclip_attn_fwd(&a, stream))) return rc;
  if ((rc = segclip_gemm(&out_proj, stream))) return rc;
  // ln_2
  rc = segclip_layernorm_fwd(d->x1, d->ln2w, d->ln2b, d->y2, d->mean2, d->rstd2, M, D, d->eps, d->x_dtype, SEGCLIP_BF16, stream);
  if (rc) return rc;
  if ((rc = segclip_gemm(&c_fc, stream))) return rc;
  return segclip_gemm(&c_proj, stream);
}
