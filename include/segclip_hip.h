/* libsegclip_hip.so - C ABI of the MI355X (gfx950) SegCLIP hot-path kernels.
 *
 * Boundary contract:
 *   - plain pointers + sizes, no torch / C++ types; every entry point is extern "C".
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library never allocates,
 *     frees or retains device pointers and never synchronises the device.
 *   - kernels are enqueued on the hipStream_t passed as `stream` (void*).
 *   - return 0 on success, non-zero otherwise; segclip_last_error_string() describes the failure.
 *   - stateless and re-entrant (forward thread + autograd thread may call concurrently).
 *
 * Each entry point replaces an *implicit* torch op group of the reference (the reference is pure
 * Python and has no native interface of its own); the reference call site is cited per function
 * (paths relative to the ArrowLuo/SegCLIP tree).
 *
 * dtypes: SEGCLIP_F32 activations run the exact-f32 MFMA path (v_mfma_f32_32x32x2_f32, parity
 * gate 1e-3); SEGCLIP_BF16 activations run the bf16 MFMA path (v_mfma_f32_32x32x16_bf16,
 * fp32 accumulate).  Parameters / gradients of parameters are always fp32.
 */
#ifndef SEGCLIP_HIP_H
#define SEGCLIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGCLIP_ABI_VERSION 1

#define SEGCLIP_F32 0
#define SEGCLIP_BF16 1

#define SEGCLIP_ACT_NONE 0
#define SEGCLIP_ACT_QUICK_GELU 1 /* x*sigmoid(1.702x), modules/module_clip_util.py:134-136 */
#define SEGCLIP_ACT_GELU_ERF 2   /* nn.GELU(), modules/module_seg_vit.py:128 */

#define SEGCLIP_ERR_INVALID (-1)
#define SEGCLIP_ERR_UNSUPPORTED (-2)

int segclip_version(void);
const char* segclip_last_error_string(void);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused epilogue.   C[z](m,n) = epi( alpha * sum_k A[z](m,k) * B[z](n,k) )
 *   epi(v): v += bias[n];  if act: (aux ? aux(m,n) = v : 0), v = act(v);   v += residual(m,n)
 *   mul_dact: v = v * act'(aux(m,n))   (aux is an INPUT: the saved pre-activation; bias/residual unused)
 *   aux_kind 1: aux holds act'(pre-activation) instead of the pre-activation - the forward epilogue stores the
 *               derivative (its exponential is already computed there) and mul_dact multiplies by aux as it is
 *   aux_kind 2: as 1, but aux is ONE BYTE per element, q = rint((act'(v) + 0.125) * 204) (QuickGELU': [-0.10, 1.10],
 *               absolute error <= 0.0025; erf-GELU': [-0.129, 1.129], the two extremes saturate: <= 0.0065); ldaux in bytes; bf16 operands and output, full 256 x 256 tiles (M, N
 *               multiples of 256), 16-byte aligned operands, ldaux % 8 == 0, no split-K - otherwise
 *               SEGCLIP_ERR_UNSUPPORTED (callers fall back to aux_kind 1)
 * Replaces nn.Linear / MHA in-proj / out-proj / the einsum + Conv1d contractions:
 *   modules/module_seg_vit.py:166-172,189,266-269,304,309 ; modules/module_clip_ttransformer.py:24-30 ;
 *   modules/module_clip.py:91-94,131-134 ; modules/modeling.py:356-357 and their autograd backward
 *   (dgrad: A = dY, B(n,k) = W^T via strides; wgrad: A = dY^T, B = X^T via strides).
 * Operand strides are in elements.  f32 operands: any strides.  bf16 operands: each of A, B must
 * have unit stride along k (sak == 1) or along its row index (sam == 1).  a_dtype may be F32 with
 * b_dtype BF16 (fp32 residual-stream gradients are rounded to bf16 while staging).
 * Batch index z = z1*nb2 + z2 with independent strides for both levels (heads / groups).
 * ------------------------------------------------------------------------------------------ */
typedef struct segclip_gemm_desc {
  const void* A;
  const void* B;
  void* C;
  const float* bias;    /* [N] fp32 or NULL */
  const void* residual; /* (M,N) leading dim ldr, dtype r_dtype, or NULL */
  void* aux;            /* (M,N) leading dim ldaux, dtype c_dtype, or NULL */
  int64_t M, N, K;
  int64_t sam, sak;
  int64_t sbn, sbk;
  int64_t ldc, ldr, ldaux;
  int64_t nb1, nb2;
  int64_t bsA1, bsA2, bsB1, bsB2, bsC1, bsC2; /* aux uses the C batch strides */
  int64_t bsR1, bsR2;                         /* residual batch strides (0 = broadcast over the batch) */
  int32_t a_dtype, b_dtype, c_dtype, r_dtype;
  int32_t act;
  int32_t mul_dact;
  float alpha;
  int32_t aux_kind; /* 0: aux = pre-activation; 1: aux = act'(pre-activation); 2: the same as one byte per element */
  void* ws;         /* optional split-K scratch (bf16 path, plain epilogue only); NULL = no split-K */
  int64_t ws_bytes; /* size of ws; segclip_gemm_ws_bytes(d) is the amount that enables split-K */
  float* colsum;    /* optional [N] fp32: column sums of the stored C (bias gradient fused into the epilogue).
                       Needs colsum_ws = (M/64)*N floats, M % 128 == 0, N % 256 == 0 and the LDS-DMA bf16 path;
                       otherwise segclip_gemm returns SEGCLIP_ERR_UNSUPPORTED without launching. */
  float* colsum_ws;
  int32_t flags;    /* SEGCLIP_GEMM_DEFER_*: leave the trailing reduction launches to the caller (segclip_reduce_multi):
                       the split-K slabs stay in ws, the column-sum partials in colsum_ws */
  int32_t res_row_mod; /* > 0: the residual of output row m is residual row (m % res_row_mod) - a (T, N) table broadcast over
                          the B samples of an (B*T, N) output (the positional table added to the patch embedding,
                          modules/module_clip_vtransformer.py:56-64) without a batched launch.  Honoured for fp32 outputs
                          with an fp32 residual on full 256 x 256 bf16 tiles; otherwise SEGCLIP_ERR_UNSUPPORTED. */
} segclip_gemm_desc;

#define SEGCLIP_GEMM_DEFER_SPLITK 1 /* do not launch the split-K combine: C is NOT written; combine ws later */
#define SEGCLIP_GEMM_DEFER_COLSUM 2 /* do not launch the column-sum reduction of colsum_ws ((M/64) x N partials) */

size_t segclip_gemm_ws_bytes(const segclip_gemm_desc* d);
/* number of K splits segclip_gemm(d) uses with the ws / ws_bytes given in d: ws then holds that many (nb1*nb2*M*N) fp32
 * slabs before the combine (SEGCLIP_GEMM_DEFER_SPLITK leaves them there); 1 = no split-K */
int segclip_gemm_splits(const segclip_gemm_desc* d);
int segclip_gemm(const segclip_gemm_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Deferred reductions, many per launch.  The backward of a residual block ends in ~8 small reductions (4 split-K
 * combines of the weight gradients, the dgamma|dbeta|column-sum partials of 2 LayerNorm backwards, fused bias-gradient
 * column sums): their producers can leave the partials in their workspaces (SEGCLIP_GEMM_DEFER_*,
 * segclip_layernorm_bwd with dgamma == NULL) and the caller combines them with ONE launch per kind.
 *   kind SEGCLIP_REDUCE_SLABS: out[i] = scale * sum_s src[s*width + i], i < width (width % 4 == 0; fp32 or bf16 out)
 *   kind SEGCLIP_REDUCE_ROWS : out_k[c] = sum_r src[r*ld + k*seg + c] for k < nseg, c < seg (fp32 out, seg % 4 == 0):
 *                              column sums of a (rows x nseg*seg) partial matrix, split into up to 3 output arrays
 * Deterministic (fixed summation order), n <= SEGCLIP_REDUCE_MAX entries per call, all of one kind.
 * Replaces nothing in the reference (torch sums these inside its autograd kernels); it is the second stage of
 * modules/module_clip_util.py:126-132 (LayerNorm backward) and of every nn.Linear weight / bias gradient.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_REDUCE_SLABS 0
#define SEGCLIP_REDUCE_ROWS 1
#define SEGCLIP_REDUCE_MAX 16
typedef struct segclip_reduce_entry {
  const float* src;
  void* out0;
  float* out1;
  float* out2;
  int64_t rows;   /* SLABS: number of slabs; ROWS: number of partial rows */
  int64_t width;  /* SLABS: elements per slab; ROWS: nseg * seg */
  int64_t ld;     /* ROWS: leading dimension of src (floats) */
  int64_t seg;    /* ROWS: columns per output array */
  float scale;    /* SLABS only */
  int32_t out_dtype; /* SLABS: SEGCLIP_F32 / SEGCLIP_BF16 */
} segclip_reduce_entry;
int segclip_reduce_multi(const segclip_reduce_entry* entries, int n, int kind, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last axis (fp32 statistics).  modules/module_clip_util.py:126-132,
 * modules/module_seg_vit.py:150-156 (eps 1e-5), modules/modeling.py:152 (eps 1e-6).
 * bwd: dx = LN'(dy) (+ dres if given);  dgamma/dbeta (fp32, [cols]) are fully reduced.
 *      dx_bf16 (optional): a bf16 copy of dx for the GEMMs that consume it next;
 *      dres_colsum (optional, needs dres): column sums of dres = the bias gradient of the Linear whose
 *      output gradient dres is (fused here because this kernel streams dres anyway).
 * ws: segclip_layernorm_bwd_ws_bytes(rows, cols) bytes of scratch.
 * dgamma == NULL: the final reduction is left to the caller - ws then holds segclip_layernorm_bwd_ws_bytes / (3*cols*4)
 *      partial rows of [dgamma | dbeta | dres column sums] (3*cols floats each), see segclip_reduce_multi.
 * rows == 0: dgamma, dbeta and dres_colsum (where passed) are zeroed; dgamma == NULL: the one partial row of ws is.
 * ------------------------------------------------------------------------------------------ */
int segclip_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                          float* rstd, int64_t rows, int64_t cols, float eps, int x_dtype, int y_dtype,
                          void* stream);
size_t segclip_layernorm_bwd_ws_bytes(int64_t rows, int64_t cols);
int segclip_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                          const float* rstd, const void* dres, void* dx, void* dx_bf16, float* dgamma,
                          float* dbeta, float* dres_colsum, void* ws, int64_t rows, int64_t cols, int dy_dtype,
                          int x_dtype, int dx_dtype, void* stream);
/* Row-mapped variants: row r of the kernel's row space is row (r / seg_in) * seg_out + seg_off + r % seg_in of y
 * (forward) / of dy (backward); x, mean, rstd, dres, dx keep plain rows.  LayerNorm(cat([centers, tokens], dim=1))
 * without the concatenated copy - modules/module_seg_vit.py:294-296 (`kv = torch.cat([q, inputs], dim=1)`) with
 * :211 (`self.ln_1(k)`): one call per part writes its token slice of every sample of the (B, seg_out, cols) buffer. */
int segclip_layernorm_fwd_seg(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                              float* rstd, int64_t rows, int64_t cols, float eps, int x_dtype, int y_dtype,
                              int64_t seg_in, int64_t seg_out, int64_t seg_off, void* stream);
int segclip_layernorm_bwd_seg(const void* dy, const void* x, const float* gamma, const float* mean,
                              const float* rstd, const void* dres, void* dx, void* dx_bf16, float* dgamma,
                              float* dbeta, float* dres_colsum, void* ws, int64_t rows, int64_t cols, int dy_dtype,
                              int x_dtype, int dx_dtype, int64_t seg_in, int64_t seg_out, int64_t seg_off,
                              void* stream);

/* Three affine outputs of ONE normalisation (n must be 3; fp32 x; cols 768 or 1024; y / dy all fp32 or all bf16 - otherwise
 * SEGCLIP_ERR_UNSUPPORTED and nothing is launched).  The learnable-center stage normalises the same token rows with
 * `self.norm` (modules/module_seg_vit.py:289) and with `ln_1` of both cross-attention layers (:211 over :294-296): one
 * read of x in the forward, and ONE dx = sum of the three LayerNorm backwards in the backward.
 * gamma / beta / y / dy: arrays of n device pointers; maps: n x {seg_in, seg_out, seg_off} (seg_in = 0: identity) - the row
 * mapping of output k / gradient k as in segclip_layernorm_fwd_seg.
 * dgb: (2n, cols) fp32 <- [dgamma_0, dbeta_0, dgamma_1, dbeta_1, ...];  ws: segclip_layernorm_bwd_multi_ws_bytes. */
int segclip_layernorm_fwd_multi(const void* x, int n, const float* const* gamma, const float* const* beta,
                                void* const* y, const int64_t* maps, float* mean, float* rstd, int64_t rows,
                                int64_t cols, float eps, int x_dtype, int y_dtype, void* stream);
size_t segclip_layernorm_bwd_multi_ws_bytes(int64_t rows, int64_t cols, int n);
int segclip_layernorm_bwd_multi(const void* const* dy, const void* x, int n, const float* const* gamma,
                                const int64_t* maps, const float* mean, const float* rstd, void* dx, float* dgb,
                                void* ws, int64_t rows, int64_t cols, int dy_dtype, int x_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-head attention core  O = softmax(scale * Q K^T [+ causal mask]) V,  head_dim <= 64.
 * Replaces the inside of nn.MultiheadAttention: modules/module_seg_vit.py:189 (self, 12x64),
 * :215 (center cross-attention; K/V addressed with explicit (batch, token) strides so that both
 * the torch-1.8 "t18" buffer reinterpretation and the intended layout run on the same kernel,
 * SURVEY.md finding 0.4), modules/module_clip_ttransformer.py:46 (causal, mask of
 * modules/module_clip_util.py:199-205 generated in-kernel), modules/module_mae.py:124-130 (8x48).
 * Element strides: *_sb batch, *_st token; head h lives at offset h*hd.
 * stats: fp32 scratch kept for backward, segclip_attn_stats_bytes() bytes
 *        (bf16: log-sum-exp per row; f32: the full probability matrix).
 * bwd ws: segclip_attn_bwd_ws_bytes() bytes (f32: dP; bf16 with more than 256 tokens: the streaming kernels' D and
 *         column-sum vectors; 0 otherwise).
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_ATTN_FP8 1
typedef struct segclip_attn_desc {
  const void* Q;
  const void* K;
  const void* V;
  void* O;
  void* stats;
  const void* dO;
  void* dQ;
  void* dK;
  void* dV;
  void* ws;
  int64_t B, H, Tq, Tk, hd;
  int64_t q_sb, q_st, k_sb, k_st, v_sb, v_st, o_sb, o_st;
  int64_t dq_sb, dq_st, dk_sb, dk_st, dv_sb, dv_st, do_sb, do_st;
  float scale;
  int32_t causal;
  int32_t dtype;
  /* SEGCLIP_ATTN_FP8 (bf16 dtype, forward only; BASELINE configs[4]): asked for an e4m3 forward, which was removed
   * (slower than bf16).  segclip_attn_fwd refuses it with SEGCLIP_ERR_UNSUPPORTED and writes nothing. */
  int32_t flags;
  /* bwd, bf16 only, nullable: fp32 [B][3][H*hd] receives, per sample, the token sums of dQ | dK | dV
   * (= that sample's contribution to the in_proj bias gradient of nn.MultiheadAttention), computed from the
   * tiles already in LDS instead of a separate column-sum pass over dQ/dK/dV. */
  void* colsum_part;
  /* nullable: int32 [B] number of valid keys per sample (keys >= klen[b] are masked out).  The key-padding mask of the
   * text-MAE decoder blocks, modules/module_mae.py:213-219: (1 - attention_mask) * -1e6 added to the logits, where
   * attention_mask is a prefix mask (captions are padded at the end) and exp(-1e6) == 0 in fp32.
   * The forward accepts klen at any length (but never takes the at-most-8-queries kernel with it); the bf16 backward needs
   * at most 256 queries and keys and refuses longer ones with SEGCLIP_ERR_INVALID.  1 <= klen[b] (the reference always has
   * a CLS key; klen[b] == 0 is outside the contract), values above Tk mean Tk.  A masked key is still loaded and enters
   * the products with a probability of exactly 0, as in the reference (which multiplies it by exp(-1e6) == 0), so K and V
   * must hold finite values at masked keys; rows at or beyond Tq / Tk are never used.
   * causal with Tq != Tk is defined on every path: query q sees keys 0 .. min(q, Tk - 1) (indices aligned at 0). */
  const int32_t* klen;
} segclip_attn_desc;

size_t segclip_attn_stats_bytes(const segclip_attn_desc* d);
size_t segclip_attn_bwd_ws_bytes(const segclip_attn_desc* d);
int segclip_attn_fwd(const segclip_attn_desc* d, void* stream);
int segclip_attn_bwd(const segclip_attn_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Launch executor: the forward of one pre-LN residual attention block (modules/module_seg_vit.py:175-196,
 * modules/module_clip_ttransformer.py:20-37; bf16 mode) as ONE call - LayerNorm, in_proj, attention, out_proj + residual,
 * LayerNorm, c_fc + activation + saved derivative, c_proj + residual: the seven launches the Python layer would issue, with the
 * same descriptors, into caller-owned buffers (bit-identical results; what it saves is ~250 us of host time per block).
 * The four GEMMs are planned before the first launch: SEGCLIP_ERR_UNSUPPORTED means that nothing was enqueued (as from
 * segclip_gemm) and the caller may issue the launches one by one, in another form.  Only argument errors of the LayerNorm and
 * attention entry points (SEGCLIP_ERR_INVALID: D % 4, head_dim <= 64 and a multiple of 8) can surface after a launch.
 * x, x1, xo: the residual stream (M, D) in x_dtype (fp32, or bf16 with config.bf16_resid); everything else bf16 unless noted.
 * M may exceed B*T (row-padded stack): the attention touches the B*T token rows, the pad rows of o are zeroed.
 * Weights are the (out, in) bf16 copies of the reference's parameters; biases and LayerNorm affines fp32.
 * ------------------------------------------------------------------------------------------ */
typedef struct segclip_resblock_fwd_desc {
  const void* x;                 /* (M, D) x_dtype */
  const float* ln1w; const float* ln1b; const void* wqkv; const float* bqkv; const void* wo; const float* bo;
  const float* ln2w; const float* ln2b; const void* wfc; const float* bfc; const void* wpr; const float* bpr;
  void* y1; float* mean1; float* rstd1;   /* ln_1 output (M, D) and its row statistics */
  void* qkv;                     /* (M, 3D) */
  void* o;                       /* (M, D) attention output */
  void* stats;                   /* segclip_attn_stats_bytes: the attention's softmax statistics */
  void* x1;                      /* (M, D) x_dtype: the stream after the attention branch */
  void* y2; float* mean2; float* rstd2;
  void* h; int64_t ld_h;         /* (M, F) activation output, row pitch ld_h */
  void* u; int64_t ld_u;         /* nullable: what the backward keeps of the pre-activation (aux_kind as in segclip_gemm_desc) */
  void* xo;                      /* (M, D) x_dtype: the block's output */
  const void* klen;              /* nullable: int32 [B] valid keys per sample */
  int64_t M, B, T, D, F, H;
  float eps, attn_scale;
  int32_t causal, act, aux_kind, x_dtype;
} segclip_resblock_fwd_desc;
int segclip_resblock_fwd(const segclip_resblock_fwd_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise / reduction helpers
 * ------------------------------------------------------------------------------------------ */
/* dst[i] = (dst_dtype) src[i] */
int segclip_cast(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, void* stream);
/* fp32 operand -> its two bf16 parts, three blocks along the contraction dimension (role 0: hi|lo|hi, role 1: hi|hi|lo; stack 0:
 * blocks side by side in a row of 3*cols, stack 1: three (rows x cols) blocks one after the other).  With both operands split this
 * way ONE bf16 GEMM of contraction length 3K computes A_hi B_hi + A_lo B_hi + A_hi B_lo in fp32 accumulators: the fp32 parity mode
 * of the Linear layers (reference arithmetic: main_task_align.py:102, fp32 torch.nn.Linear) on the bf16 matrix pipe. */
int segclip_split3_bf16(const float* src, void* dst, int64_t rows, int64_t cols, int64_t ld, int stack, int role, void* stream);
/* out[n] = sum_m X[m*ld + n]  (bias gradients; deterministic two-stage).  ws: colsum_ws_bytes */
size_t segclip_colsum_ws_bytes(int64_t M, int64_t N);
int segclip_colsum(const void* X, float* out, void* ws, int64_t M, int64_t N, int64_t ld, int dtype,
                   void* stream);
/* y = act(x) ; dx = dy * act'(x)  (stand-alone activation, modules/module_seg_vit.py:274,330) */
int segclip_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, void* stream);
int segclip_act_bwd(const void* dy, const void* x, void* dx, int64_t n, int act, int dtype, void* stream);
/* out = a + b (same dtype) */
int segclip_add(const void* a, const void* b, void* out, int64_t n, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Vision front end.  modules/module_clip_vtransformer.py:56-64.
 * im2col: image (B,3,H,W) fp32 -> cols (B*gh*gw, 3*p*p), column order (c,py,px) [layout 0, conv1]
 *         or (py,px,c) [layout 1, MAE target `patchify`, modules/module_mae.py:18-29].
 * assemble: x[b,0,:] = cls + pos[0];  x[b,1+t,:] = patches[b,t,:] + pos[1+t]   (fp32 out)
 * ------------------------------------------------------------------------------------------ */
int segclip_im2col(const float* image, void* cols, int64_t B, int64_t C, int64_t H, int64_t W, int64_t p,
                   int layout, int out_dtype, void* stream);
/* same, with rows of `ld` >= 3*p*p elements whose tail columns are zero-filled: the contraction dimension of the
 * patch-embedding GEMM padded to the kernel's alignment (ViT-L/14: 3*14*14 = 588 -> 640). */
int segclip_im2col_ld(const float* image, void* cols, int64_t B, int64_t C, int64_t H, int64_t W, int64_t p,
                      int layout, int out_dtype, int64_t ld, void* stream);
int segclip_vis_assemble(const void* patches, const float* cls, const float* pos, float* x, int64_t B,
                         int64_t T, int64_t D, int p_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Text front end.  modules/module_clip.py:109-112 (nn.Embedding gather + positional add) and its
 * backward (scatter-add into the fp32 table gradient, which must be zero-initialised by the caller;
 * dpos (L,D) is fully written).
 * ------------------------------------------------------------------------------------------ */
int segclip_embed_fwd(const int64_t* ids, const float* table, const float* pos, float* out, int64_t B,
                      int64_t L, int64_t D, int64_t vocab, void* stream);
int segclip_embed_bwd(const int64_t* ids, const float* dout, float* dtable, float* dpos, int64_t B,
                      int64_t L, int64_t D, int64_t vocab, void* stream);

/* MAE glue of the full loss, fp32, D a multiple of 4 (reference modules/modeling.py:240-242: mean over the tokens prepended as
 * the CLS row; modules/module_mae.py:310-314: mask tokens appended, un-shuffled by ids_restore, + positional table).
 *   mean_cat:      out (B,T+1,D): out[b][0] = mean_t x[b][t], out[b][1+t] = x[b][t];  bwd: dx[b][t] = dout[b][1+t] + dout[b][0] / T
 *   mae_unshuffle: out (B,L,D)[b][j] = (ids[b][j] < K ? x[b][ids[b][j]] : mask_token) + pos[j]   (x (B,K,D), ids a permutation of 0..L-1
 *                  per sample); bwd: dx (B,K,D), dpos (L,D) = sum_b dout, mpart (L,D) = the mask-token share of that sum per
 *                  position - the mask token's gradient is the column sum of mpart (segclip_colsum). */
int segclip_mean_cat_fwd(const float* x, float* out, int64_t B, int64_t T, int64_t D, void* stream);
int segclip_mean_cat_bwd(const float* dout, float* dx, int64_t B, int64_t T, int64_t D, void* stream);
int segclip_mae_unshuffle_fwd(const float* x, const float* mask_token, const int64_t* ids, const float* pos, float* out, int64_t B,
                              int64_t K, int64_t L, int64_t D, void* stream);
int segclip_mae_unshuffle_bwd(const float* dout, const int64_t* ids, float* dx, float* dpos, float* mpart, int64_t B, int64_t K,
                              int64_t L, int64_t D, void* stream);

/* Row gather / scatter-add with int64 indices (EOT pick modules/module_clip.py:136, MAE keep /
 * un-shuffle gathers modules/module_clip_util.py:110, modules/module_mae.py:310).
 * gather: out[b, j, :] = src[b, idx[b,j], :] ; scatter_add: dsrc[b, idx[b,j], :] += dout[b, j, :]
 * (dsrc zero-initialised by the caller; indices within one b must be unique -> no atomics). */
int segclip_gather_rows(const void* src, const int64_t* idx, void* out, int64_t B, int64_t Tsrc,
                        int64_t Tout, int64_t D, int dtype, void* stream);
int segclip_scatter_rows(const void* dout, const int64_t* idx, void* dsrc, int64_t B, int64_t Tsrc,
                         int64_t Tout, int64_t D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Learnable-center hard assignment.  modules/module_seg_vit.py:304-310 + gumbel_softmax :221-242.
 *   logits (B,G,T) fp32 = q k^T (un-scaled; computed by segclip_gemm in fp32 always)
 *   training: y = softmax((logits + gumbel)/tau, dim=G);  eval (gumbel NULL): y = softmax(logits)
 *   idx[b,t] = argmax_g y (first max wins, like torch.max);  hard = onehot(idx)
 *   soft = softmax(logits, dim=G)   (consumed by the segmentation evaluation only)
 *   counts[b,g] = sum_t hard[b,g,t]   (the token count, NOT clamped: an empty center has 0; the segment mean clamps)
 * Limits: G <= 255 (idx is uint8); any B, T.  y_soft, soft, hard: (B,G,T) fp32; idx (B,T); counts (B,G), zeroed by the call.
 * bwd (straight-through): dlogits = dy_soft-path gradient of y given dhard (B,G,T):
 *   dlogits[b,:,t] = (y * (dhard - sum_g dhard*y)) / tau
 * ------------------------------------------------------------------------------------------ */
int segclip_assign_fwd(const float* logits, const float* gumbel, float tau, float* y_soft, float* soft,
                       uint8_t* idx, float* hard, float* counts, int64_t B, int64_t G, int64_t T,
                       void* stream);
int segclip_assign_bwd(const float* dhard, const float* y_soft, float tau, float* dlogits, int64_t B,
                       int64_t G, int64_t T, void* stream);

/* ------------------------------------------------------------------------------------------
 * Losses.
 * l2norm: y = x / ||x||  rows (modules/modeling.py:341-345).
 * ce: mean over rows of -log softmax(logits)[label], label = row + label_offset
 *     (modules/modeling.py:205-209).  fwd writes loss (1 float) and lse per row; bwd writes
 *     dlogits = gscale * (softmax - onehot) / rows.
 * superpixel_kl: modules/modeling.py:212-224 on the hard assignment indices (label-histogram
 *     formulation).  Output is a constant w.r.t. parameters only through hard's straight-through
 *     gradient: bwd returns dhard (B,G,T).
 * masked_mse: MAE loss modules/module_mae.py:323-328: pred (B,1+T,Dp) (row 0 = CLS, skipped),
 *     target (B,T,Dp), mask (B,1+T).
 * ------------------------------------------------------------------------------------------ */
int segclip_l2norm_fwd(const float* x, float* y, float* norm, int64_t rows, int64_t cols, void* stream);
int segclip_l2norm_bwd(const float* dy, const float* y, const float* norm, float* dx, int64_t rows,
                       int64_t cols, void* stream);
int segclip_ce_fwd(const float* logits, float* lse, float* loss_rows, int64_t rows, int64_t cols,
                   int64_t label_offset, void* stream);
/* dlogits = (*gscale_ptr) * gscale * (softmax - onehot) / rows ; gscale_ptr (device scalar, upstream
 * gradient) may be NULL */
int segclip_ce_bwd(const float* logits, const float* lse, const float* gscale_ptr, float gscale,
                   float* dlogits, int64_t rows, int64_t cols, int64_t label_offset, void* stream);
/* nn.CrossEntropyLoss(ignore_index) with explicit labels (text-MAE vocabulary loss, modules/module_mae.py:353):
 * fwd: lse[r], loss_rows[r] = (labels[r] == ignore ? 0 : lse[r] - logits[r][labels[r]]), valid[r] = labels[r] != ignore
 *      (the mean over valid rows is taken by the caller: sum(loss_rows) / sum(valid));
 * bwd: dlogits[r][c] = (labels[r] == ignore ? 0 : softmax[r][c] - [c == labels[r]]) * gscale[0] * inv_count[0]. */
int segclip_ce_labels_fwd(const float* logits, const int64_t* labels, int64_t ignore_index, float* lse, float* loss_rows,
                          float* valid, int64_t rows, int64_t cols, void* stream);
int segclip_ce_labels_bwd(const float* logits, const float* lse, const int64_t* labels, int64_t ignore_index,
                          const float* gscale, const float* inv_count, float* dlogits, int64_t rows, int64_t cols,
                          void* stream);
/* loss_rows[b] = this image's share of the loss (already / (2*B*T*G)); dhard = d(sum loss_rows)/dhard */
int segclip_superpixel_kl(const float* hard, const int64_t* seg, float* loss_rows, float* dhard,
                          int64_t B, int64_t G, int64_t T, void* stream);
/* loss_rows[b*T+t] = mask[b,1+t] * mean_d (pred[b,1+t,d]-target[b,t,d])^2 ; loss = sum(loss_rows)/sum(mask[:,1:]) */
int segclip_masked_mse_fwd(const void* pred, const float* target, const float* mask, float* loss_rows,
                           int64_t B, int64_t T, int64_t Dp, int pred_dtype, void* stream);
int segclip_masked_mse_bwd(const void* pred, const float* target, const float* mask,
                           const float* gscale_ptr, const float* mask_sum, float gscale, void* dpred,
                           int64_t B, int64_t T, int64_t Dp, int pred_dtype, void* stream);
/* out[i] = x[i] * (*s)  (device scalar) ;  out[0] = scale * sum(x)  (deterministic single block) */
int segclip_scale(const float* x, const float* s, float* out, int64_t n, void* stream);
/* out = -log(-log(clamp(u, FLT_MIN, 1 - FLT_EPSILON))): Gumbel(0,1) noise of the hard assignment from uniform samples
 * (reference modules/module_seg_vit.py:223-226, torch.distributions.Gumbel(0, 1).sample); u and out may alias */
int segclip_gumbel_from_uniform(const float* u, float* out, int64_t n, void* stream);
int segclip_reduce_sum(const float* x, float* out, int64_t n, float scale, void* stream);

/* Evaluation tier: positional table at another grid, modules/module_clip_vtransformer.py:35-53 =
 * F.interpolate(table (n x n x D, channel-last), size=(h, w), mode='bicubic', align_corners=False). */
int segclip_interp_bicubic(const float* src, float* dst, int64_t n_in, int64_t h, int64_t w, int64_t D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Zero-shot segmentation inference (segment.hip): class prompts + the center stage's soft assignment -> label map.
 * Forward only; all math fp32.  A "window" is one image handed to the vision tower: the whole image, or one crop of mmseg's
 * sliding-window grid; all windows of a call have the same size (win_h, win_w) and the same patch grid (grid_h, grid_w).
 *
 * segclip_seg_group_table: per window the G x N group-class table of ViTSegInference.encode_decode
 * (seg_segmentation/evaluation/vit_seg.py:218-254).  One workgroup per window, latency-bound.
 *   group_tokens : row r of window w at group_tokens + w * group_stride + r * C   (= patch_features[:, 1:, :], :214)
 *   pooled       : window w at pooled + w * pooled_stride                          (= image_features, :215)
 *   text         : (N, C), already L2-normalised (evaluation/builder.py:59-66);  logit_scale: device scalar,
 *                  clamp(exp(.), max=100) applied inside (:232)
 *   F.normalize of the G + 1 rows (:221-222); logits = cosines * scale (:234, :237); pre = softmax of the group logits
 *   (:235); softmax of the pooled row and its top-`topk` classes (:238-241; the reference passes min(5, N)) - among EQUAL
 *   probabilities the LOWEST class index is kept (torch.topk leaves ties unspecified); group logits outside the mask
 *   -> -inf, softmax (:242-244), times pre (:247).
 *   table (W, G, N);  table_max (W) = its maximum (the device-side operand of min(bg_thresh, .), :253 without the .item()
 *   synchronisation);  best_class (W, G) = first maximum over N of each row, best_score (W, G) its value;
 *   topk_mask (W, N) uint8 or NULL.
 *   SEGCLIP_ERR_UNSUPPORTED: ((G + 1) * (C + N) + 2 N + 8) * 4 bytes exceed 64 KiB of LDS.  G <= SEGCLIP_SEG_MAX_GROUPS.
 *
 * segclip_seg_label_map: the fused pixel kernel.  For every output pixel and every window covering it: the G channels of
 * soft_attn (W, G, grid_h * grid_w) interpolated with F.interpolate(mode="bilinear", align_corners=False) semantics in
 * ATen's fp32 operation order (vit_seg.py:54 and :191), first maximum over G (:225).  One covering window: label =
 * best_score < min(bg_thresh, table_max) ? 0 : best_class + 1 with background (:252-254), best_class without.  Several
 * (mmseg slide_inference): class logits = sum over the windows, in window order, of the window's table row (class 0: its
 * background indicator) / window count; first maximum.  labels (B, H, W) uint8 (NULL = skip; N + with_bg > 256:
 * SEGCLIP_ERR_UNSUPPORTED), groups (B, H, W) uint8 (NULL = skip) = the group in the first covering window (what
 * show_result(vis_mode="final_group") draws, :346-375).  A pixel no window covers gets label 0, group 0.
 *   windows     : (n_windows, 3) int32 rows (image, y0, x0); the windows of one image are consecutive.  The kernels read y0
 *                 and x0 only: which image a window belongs to comes from image_first alone, the image column is carried
 *                 for the caller's bookkeeping and is IGNORED.
 *   image_first : (B + 1) int32, windows image_first[b] .. image_first[b + 1] - 1 belong to image b
 *   Limits of the device-side lists, which the host entry cannot inspect - what exceeds them is SILENTLY IGNORED, the caller
 *   checks them (segclip_amd/segmentation.py does): at most SEGCLIP_SEG_MAX_IMAGE_WINDOWS windows per image (later ones are
 *   dropped); at most 16
 *   windows covering one pixel (later ones are dropped); with n_windows <= B every image is taken to have at most one
 *   window covering a pixel (the block then keeps one slot and no table copy in LDS).  Out-of-range entries cannot make
 *   the kernels read or write out of bounds.  Bound: HBM writes, 1-2 bytes per pixel.
 *
 * segclip_seg_logits: the dense output, logits (B, N + with_bg, H, W) fp32 exactly as encode_decode (:249-256) and
 * slide_inference define them; same device functions as the label map, which is its first maximum over the classes.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_MAX_GROUPS 8         /* groups per window (the center stage has 8) */
#define SEGCLIP_SEG_MAX_IMAGE_WINDOWS 64 /* windows of one image (over all its views, where it has views) */
int segclip_seg_group_table(const float* group_tokens, int64_t group_stride, const float* pooled, int64_t pooled_stride,
                            const float* text, const float* logit_scale, float* table, float* table_max,
                            int32_t* best_class, float* best_score, uint8_t* topk_mask, int64_t n_windows, int64_t G,
                            int64_t N, int64_t C, int64_t topk, void* stream);
int segclip_seg_label_map(const float* soft_attn, const float* table, const float* table_max, const int32_t* best_class,
                          const float* best_score, const int32_t* windows, const int32_t* image_first, int64_t n_windows,
                          int64_t B, int64_t H, int64_t W, int64_t win_h, int64_t win_w, int64_t grid_h, int64_t grid_w,
                          int64_t G, int64_t N, int with_bg, float bg_thresh, uint8_t* labels, uint8_t* groups, void* stream);
int segclip_seg_logits(const float* soft_attn, const float* table, const float* table_max, const int32_t* best_class,
                       const float* best_score, const int32_t* windows, const int32_t* image_first, int64_t n_windows,
                       int64_t B, int64_t H, int64_t W, int64_t win_h, int64_t win_w, int64_t grid_h, int64_t grid_w,
                       int64_t G, int64_t N, int with_bg, float bg_thresh, float* logits, void* stream);

/* ------------------------------------------------------------------------------------------
 * Zero-shot segmentation evaluation (segment_eval.inc): label maps at the ground truth's size for images of mixed sizes in
 * ONE launch, and the per-class areas of the mIoU (mmseg: resize(logits, size=ori_shape) -> arg-max -> intersect_and_union).
 *
 * The rescaled label map.  Output pixel (y, x) of an image with network size (H, W) and output size (oh, ow): taps and weights
 * of upsample_bilinear2d(align_corners=False, no scale factors) on the (H, W) grid, scales (float)H / oh and (float)W / ow;
 * at each tap the class logits exactly as the dense-logits entry above defines them (same device functions); per class the
 * blend h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11) in fp32; first maximum over the classes; one byte.  A tap of
 * weight 0 is not evaluated, so (oh, ow) = (H, W) reproduces the label-map entry above bit for bit.  Where the four taps have
 * the same covering windows and groups, hence one logit vector v, the label is v's first maximum without the blend (the blend
 * is monotone in v; two classes can change places only where it rounds two different logits to one value).  No
 * (C, oh, ow) or (C, H, W) array exists.
 *   soft_attn : flat fp32 of soft_floats elements; the windows of one image are consecutive (G, grid_h * grid_w) planes
 *   images    : (B, SEGCLIP_SEG_IMAGE_COLS) int64 rows on the device (columns by name: enum segclip_seg_image_col):
 *               0 first window  1 window count  2 H  3 W  4 oh  5 ow  6 offset of the image's oh * ow labels in `labels`
 *               7 offset of its ground truth in `gt`, or -1  8 its first workgroup = the sum of ceil(oh * ow / SEGCLIP_SEG_EVAL_TILE) over the
 *               images before it  9 win_h  10 win_w  11 grid_h  12 grid_w  13 offset of its first window in soft_attn  14 flag word
 *               of a view (read by segclip_seg_label_map_views alone; 0 here)  15 0
 *               Windows, tables and the window list (image, y0, x0) are as above, but the window size and grid are per image.
 *   n_blocks  : the sum of ceil(oh * ow / SEGCLIP_SEG_EVAL_TILE) over all images;  max_image_windows: the largest window count of
 *               an image (sizes the LDS; 1 = no image has overlapping windows)
 *   labels    : flat uint8 of labels_bytes, or NULL; a label offset that is a multiple of 4 gives dword stores
 *   gt, areas : flat uint8 of gt_bytes and (3, N + with_bg) int64, or both NULL.  areas is ADDED to: [0] intersection,
 *               [1] prediction area, [2] label area per class.  Ground-truth rule of both entries: the value ignore_index
 *               contributes nothing; with reduce_zero_label 0 contributes nothing as well and every other value counts as
 *               g - 1; a value >= the class count adds to the prediction area only (torch.histc drops it from the others).
 *               Per-workgroup integer counters in LDS, one global add per touched counter: the sums do not depend on order.
 *   Every entry of `images` is range-checked on the device; an image whose row is inconsistent with soft_floats,
 *   labels_bytes or gt_bytes is skipped.  SEGCLIP_ERR_UNSUPPORTED: N + with_bg > 256, max_image_windows > 64.  At most 16
 *   windows covering one pixel, G <= 8.  H, W, oh, ow < 2^30 and oh * ow < 2^31.
 *
 * The areas alone: the same accumulation for n pixels of label maps the caller already has.  SEGCLIP_ERR_UNSUPPORTED: C > 256.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_IMAGE_COLS 16  /* int64 columns of one row of the image table */
#define SEGCLIP_SEG_EVAL_TILE 1024 /* output pixels of one workgroup */
enum segclip_seg_image_col {
  SEGCLIP_SI_FIRST, SEGCLIP_SI_COUNT, SEGCLIP_SI_H, SEGCLIP_SI_W, SEGCLIP_SI_OH, SEGCLIP_SI_OW, SEGCLIP_SI_LAB, SEGCLIP_SI_GT,
  SEGCLIP_SI_BLK, SEGCLIP_SI_WIN_H, SEGCLIP_SI_WIN_W, SEGCLIP_SI_GH, SEGCLIP_SI_GW, SEGCLIP_SI_SOFT, SEGCLIP_SI_FLAGS
};
int segclip_seg_label_map_rescaled(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                   const int32_t* best_class, const float* best_score, const int32_t* windows,
                                   const int64_t* images, int64_t n_windows, int64_t B, int64_t n_blocks,
                                   int64_t max_image_windows, int64_t G, int64_t N, int with_bg, float bg_thresh,
                                   uint8_t* labels, int64_t labels_bytes, const uint8_t* gt, int64_t gt_bytes,
                                   int ignore_index, int reduce_zero_label, int64_t* areas, void* stream);
int segclip_seg_areas(const uint8_t* pred, const uint8_t* gt, int64_t n, int64_t C, int ignore_index, int reduce_zero_label,
                      int64_t* areas, void* stream);

/* ------------------------------------------------------------------------------------------
 * 16-bit label maps (segment_wide.inc): the two entries above for vocabularies of up to SEGCLIP_SEG_WIDE_MAX_CLASSES classes, such as
 * Pascal-Context-459 (460 classes with the background) and ADE20K-847 (848), without the dense (C, H, W) logits.
 *
 * segclip_seg_label_map_rescaled_wide: the arguments, the (B, 16) image table, the tile of 1024 output pixels, the definition
 * of a label and the ground-truth rule of segclip_seg_label_map_rescaled.  Below 257 classes its labels and areas equal that
 * entry's, value for value: the per-class value is formed by the same fp32 operations in the same order.
 *   labels    : flat uint16 of labels_elems ELEMENTS, or NULL.  Columns 6 (label offset) and 7 (ground-truth offset) of
 *               `images` count elements.  A lane's four labels are one 8-byte store where the address is a multiple of 8 (a
 *               label offset that is a multiple of 4 on a base aligned to 8), 2-byte stores otherwise.
 *   gt, areas : flat uint16 of gt_elems ELEMENTS and (3, N + with_bg) int64, or both NULL.  A ground-truth element is read as an
 *               UNSIGNED 16-bit value g, and ignore_index is compared with that value: an ignore_index outside 0 .. 65535
 *               ignores nothing.  reduce_zero_label and g >= the class count as above.  Integer counters, 3 x 1024 per
 *               workgroup in LDS, one global add per touched counter: the sums do not depend on order.
 *   How.  A pixel whose four taps have one covering window and one group takes the label staged per (window, group), per lane.
 *   Every other pixel - taps that disagree, or several covering windows - is resolved by its wave: the owner's tap weights and
 *   cover lists are broadcast, lane l evaluates the classes l, l + 64, ... (a table row is read as consecutive floats by
 *   consecutive lanes) and a shuffle reduction takes the maximum, among equal values the lowest class = the first maximum.
 *   Up to 32 classes every lane scans the classes of its own pixel instead, as the uint8 entry does (measured faster there).
 *   Every entry of `images` is range-checked on the device against soft_floats, labels_elems and gt_elems; an image whose row
 *   is inconsistent is skipped.  What exceeds the device-side lists is SILENTLY IGNORED as above: at most 64 windows per
 *   image, at most 16 windows covering one pixel.  G <= 8.  H, W, oh, ow < 2^30 and oh * ow < 2^31.
 *   LDS: 14.5 KiB static + at most 48 KiB dynamic (no table copy where G * N > 4096: the global table is read).
 *   Bound: the class scan of the undecided pixels, (covering windows x taps) x (N + with_bg) table reads each, from L2;
 *   2 bytes of HBM writes per pixel.  Measured: profiles/seg_wide.txt.
 * SEGCLIP_ERR_UNSUPPORTED (no launch): N + with_bg > SEGCLIP_SEG_WIDE_MAX_CLASSES, max_image_windows > 64.
 *
 * segclip_seg_areas_wide: segclip_seg_areas for n uint16 elements.  SEGCLIP_ERR_UNSUPPORTED: C > SEGCLIP_SEG_WIDE_MAX_CLASSES.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_WIDE_MAX_CLASSES 1024 /* classes of a 16-bit label map, the background included */
int segclip_seg_label_map_rescaled_wide(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                        const int32_t* best_class, const float* best_score, const int32_t* windows,
                                        const int64_t* images, int64_t n_windows, int64_t B, int64_t n_blocks,
                                        int64_t max_image_windows, int64_t G, int64_t N, int with_bg, float bg_thresh,
                                        uint16_t* labels, int64_t labels_elems, const uint16_t* gt, int64_t gt_elems,
                                        int ignore_index, int reduce_zero_label, int64_t* areas, void* stream);
int segclip_seg_areas_wide(const uint16_t* pred, const uint16_t* gt, int64_t n, int64_t C, int ignore_index,
                           int reduce_zero_label, int64_t* areas, void* stream);

/* ------------------------------------------------------------------------------------------
 * Background-threshold sweep (segment_sweep.inc): segclip_seg_label_map_rescaled for T values of bg_thresh in ONE launch, for
 * tuning the one hyperparameter of the zero-shot evaluation (the reference's configurations use 0.80, 0.25 and 0.65:
 * the dataset files of seg_segmentation/configs/_base_/datasets, test_cfg) without repeating towers, front end and group tables per value.
 * The arguments, descriptor tables, tile, range checks and limits are those of segclip_seg_label_map_rescaled; the background
 * class is implied (no with_bg argument, N + 1 classes).
 *   thresholds : HOST pointer to T finite, strictly increasing floats, 1 <= T <= SEGCLIP_SEG_MAX_THRESHOLDS; they travel in the
 *                kernel arguments
 *   labels     : NULL, or T planes of labels_bytes each; plane t is, byte for byte, what segclip_seg_label_map_rescaled writes
 *                with bg_thresh = thresholds[t] (the label offsets of `images` are offsets in a plane; dword stores where
 *                plane base + offset is a multiple of 4, byte stores otherwise)
 *   gt, areas  : flat uint8 of gt_bytes and (T, 3, N + 1) int64, or both NULL.  areas is ADDED to; slice t equals, integer for
 *                integer, what segclip_seg_label_map_rescaled adds with bg_thresh = thresholds[t].
 * How.  The threshold decides only the background indicator best_score < min(bg_thresh, table_max[window]) of a (window, group)
 * pair, which over ascending thresholds can only switch on; the class-0 logit is a monotone fp32 function of the indicators and
 * the other classes do not see the threshold.  So a pixel has one foreground label f (first maximum over the classes >= 1)
 * and one switch index s: its label is f for t < s and 0 for t >= s.  Covers, taps and the foreground scan run once per pixel
 * (the device functions of the single-threshold entry); the class-0 logit is evaluated per threshold until it is not below the
 * foreground maximum (class 0 comes first and wins ties, as the strict > scan decides).  Areas: LDS buckets by (s, class),
 * turned into the T slices by a prefix sum at flush time, one integer global add per touched counter.
 *   LDS: tables and cover lists as the single-threshold entry, plus (2 (T + 1) + 1) (N + 1) counters: at most 83 KiB dynamic
 *   (the limit is raised once per device when a launch needs more than 56 KiB).
 *   Bound: as the single-threshold entry (covers and class scan) plus T bytes of label stores per pixel; design figure.
 * SEGCLIP_ERR_INVALID (no launch): T < 1, thresholds NULL, a non-finite or non-increasing threshold.
 * SEGCLIP_ERR_UNSUPPORTED (no launch): T > SEGCLIP_SEG_MAX_THRESHOLDS, N + 1 > 256, max_image_windows > 64.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_MAX_THRESHOLDS 16 /* background thresholds of one launch */
int segclip_seg_label_map_rescaled_sweep(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                         const int32_t* best_class, const float* best_score, const int32_t* windows,
                                         const int64_t* images, int64_t n_windows, int64_t B, int64_t n_blocks,
                                         int64_t max_image_windows, int64_t G, int64_t N, const float* thresholds, int64_t T,
                                         uint8_t* labels, int64_t labels_bytes, const uint8_t* gt, int64_t gt_bytes,
                                         int ignore_index, int reduce_zero_label, int64_t* areas, void* stream);

/* ------------------------------------------------------------------------------------------
 * Flip and multi-scale test-time augmentation (segment_aug.inc): mmseg's MultiScaleFlipAug + EncoderDecoder.aug_test, the
 * wrapper of every test configuration of the reference (seg_segmentation/configs/_base_/datasets/pascal_voc12.py:24-26,
 * evaluation/builder.py:121-123): every view is segmented, its logits are resized to the original size and passed through a
 * soft-max, flipped back, the probabilities are averaged over the views and the arg-max is taken.  ONE launch for a list of
 * images of mixed sizes; no (C, oh, ow), (C, H, W) or per-view probability array exists.
 *
 * segclip_seg_label_map_views: the arguments of segclip_seg_label_map_rescaled, except that `images` holds one row PER VIEW
 * (the view's own network size, windows, window size, grid and soft_attn offset; column 14 = flag word, SEGCLIP_SEG_FLIP_H =
 * bit 0 horizontal flip, SEGCLIP_SEG_FLIP_V = bit 1 vertical flip) and `views` groups them:
 *   views   : (B, SEGCLIP_SEG_VIEW_COLS) int64 rows on the device: 0 the image's first row of `images` (its views are consecutive rows)  1 V
 *   images  : (n_rows, 16); columns 4-8 (oh, ow, label offset, ground-truth offset, first workgroup) are the IMAGE's and are
 *             read from its first view's row; every view row must state the same (oh, ow)
 *   Output pixel (y, x) of an image with output size (oh, ow):
 *   1. per view v in list order the source position (y', x') = (y, x) mirrored in (oh, ow) along each flagged axis (mmseg flips
 *      the probability map back at the original size, after the resize and the soft-max);
 *   2. at (y', x') the view's class logits exactly as segclip_seg_label_map_rescaled defines them: same device functions, the
 *      four-tap fp32 blend h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11) at every pixel, a tap of weight 0 not evaluated;
 *   3. p_v = soft-max over the N + with_bg classes in fp32: maximum subtracted, expf, divided by the sum (class order);
 *   4. the sum over the views in view order divided by (float)V; its first maximum is the label, one byte.
 *   labels / gt / areas / ignore_index / reduce_zero_label: as in segclip_seg_label_map_rescaled (dword stores at label offsets
 *   that are multiples of 4; per-workgroup counters in LDS).  best_class is not needed: the entry takes best_score only.
 *   Limits.  SEGCLIP_ERR_UNSUPPORTED: N + with_bg > 256; max_views > SEGCLIP_SEG_MAX_VIEWS; max_image_windows >
 *   SEGCLIP_SEG_MAX_IMAGE_WINDOWS, where
 *   max_image_windows = the largest number of windows of one image over ALL its views, max_view_windows = the largest of one
 *   view (1 = no view has overlapping windows: one list slot per tap), max_views = the largest V.  The device-side lists are
 *   not inspected by the host entry: a view's windows beyond 64, an image's windows beyond 64 over its views and covering windows
 *   beyond 16 are SILENTLY IGNORED - the caller checks (segclip_amd/ops.py seg_view_tables, segmentation.py).  Every row of
 *   both tables is range-checked on the device: an image whose view row is outside `images`, whose V is outside 1..16 or
 *   above the stated max_views (the (maximum, sum) slots in LDS are sized by it), or one of whose views is inconsistent (sizes, another (oh, ow), soft_floats, labels_bytes, gt_bytes) is SKIPPED.
 *   LDS: up to 96 KiB dynamic - the covering-window lists, a table copy, and per-lane accumulators acc[class][lane]; when the
 *   classes do not fit (C KiB) they are walked in chunks and every view's (maximum, sum) is kept from the first walk.
 *   Bound: ALU - about 3 V C logit evaluations (1-4 LDS reads each) and V C expf per output pixel; design figure, unmeasured.
 *
 * segclip_seg_view_probs: the dense twin for ONE image (views has one row): probs (N + with_bg, oh, ow) fp32 = the mean of step
 * 4, by the same kernel body, so the label above is its first maximum over the classes by construction.  An inconsistent
 * table or probs_floats < C * oh * ow: nothing is written.  Bound: HBM writes, 4 C bytes per pixel, beside the same ALU work.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_MAX_VIEWS 16 /* views of one image */
#define SEGCLIP_SEG_VIEW_COLS 2  /* int64 columns of one row of the view table */
#define SEGCLIP_SEG_FLIP_H 1     /* flag word of a view: horizontal flip */
#define SEGCLIP_SEG_FLIP_V 2     /* vertical flip */
int segclip_seg_label_map_views(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                                const float* best_score, const int32_t* windows, const int64_t* images, int64_t n_rows,
                                const int64_t* views, int64_t n_windows, int64_t B, int64_t n_blocks, int64_t max_image_windows,
                                int64_t max_view_windows, int64_t max_views, int64_t G, int64_t N, int with_bg, float bg_thresh,
                                uint8_t* labels, int64_t labels_bytes, const uint8_t* gt, int64_t gt_bytes, int ignore_index,
                                int reduce_zero_label, int64_t* areas, void* stream);
int segclip_seg_view_probs(const float* soft_attn, int64_t soft_floats, const float* table, const float* table_max,
                           const float* best_score, const int32_t* windows, const int64_t* images, int64_t n_rows,
                           const int64_t* views, int64_t n_windows, int64_t n_blocks, int64_t max_image_windows,
                           int64_t max_view_windows, int64_t max_views, int64_t G, int64_t N, int with_bg, float bg_thresh,
                           float* probs, int64_t probs_floats, void* stream);

/* ------------------------------------------------------------------------------------------
 * Front end of the zero-shot evaluation (segment_frontend.inc): decoded uint8 images -> the vision tower's input windows in ONE
 * launch.  Replaces the test pipeline's Resize(keep_ratio=True) + Normalize(mean, std, to_rgb=True)
 * (seg_segmentation/configs/_base_/datasets/pascal_voc12.py:19-34, mmcv / cv2 there) and the window slicing of mmseg's
 * slide_inference; the resized image is never materialised.
 *   images  : (B, SEGCLIP_SEG_SOURCE_COLS) int64 rows on the device: 0 address of the source (uint8, HWC, 3 interleaved
 *             channels)  1 h  2 w  3 row stride in bytes (>= 3 w)  4 H  5 W, the network size the image is resized to
 *   windows : (n_windows, 3) int32 rows (image, y0, x0) as above; here the image column IS read
 *   mean, inv_std : 3 host floats each, copied into the launch
 *   out     : (n_windows, 3, win_h, win_w) fp32, the layout segclip_im2col reads
 * out[k, c, y, x] = (r - mean[c]) * inv_std[c] with r the source channel c (2 - c with reverse_channels: BGR sources) of image
 * i resized to (H, W) at (Y, X) = (y0 + y, x0 + x).  Geometry of cv2 INTER_LINEAR = F.interpolate(mode="bilinear",
 * align_corners=False, antialias=False), the scale taken from the two sizes: along an axis of n source and m destination pixels
 * the coordinate of destination d is the rational ((2 d + 1) n - m) / (2 m), split in integers into s0 = its floor and
 * f = (float)remainder / (float)(2 m); s0 < 0 -> s0 = 0, f = 0; s0 >= n - 1 -> s0 = n - 1, f = 0; s1 = min(s0 + 1, n - 1).
 * In fp32: top = a (1 - fx) + b fx, bot = c (1 - fx) + d fx, r = top (1 - fy) + bot fy, each sum one fused multiply-add.  r is
 * NOT rounded back to uint8 as cv2's 8-bit fixed-point resize does (about one grey level, 0.015 normalised; unmeasured).
 *   Every table row is range-checked on the device.  A window is ZERO-FILLED when its image index is outside [0, B), when it
 *   does not lie inside (H, W), or when its image row has a null address, a stride below 3 w, or one of h, w, H, W outside
 *   [1, SEGCLIP_SEG_SOURCE_LIMIT).  Nothing is read outside the (h, w, stride) a row states and nothing written outside `out`.
 *   16-byte stores when win_w % 4 == 0 and out is 16-byte aligned, scalar stores otherwise (any win_w).  Bound: HBM writes,
 *   12 bytes per window pixel.  SEGCLIP_ERR_UNSUPPORTED: win_h * win_w >= 2^31.  n_windows, B <= 2^24.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_SOURCE_COLS 6      /* int64 columns of one row of the source table */
#define SEGCLIP_SEG_SOURCE_LIMIT 32768 /* 2^15: the sides of every picture, map and resized image of the table-driven entries stay below it */
int segclip_seg_windows_from_u8(const int64_t* images, const int32_t* windows, int64_t n_windows, int64_t B, int64_t win_h,
                                int64_t win_w, const float* mean, const float* inv_std, int reverse_channels, float* out,
                                void* stream);

/* The front end for flipped views (MultiScaleFlipAug's RandomFlip after its Resize): segclip_seg_windows_from_u8 with
 * (B, SEGCLIP_SEG_SOURCE_VIEW_COLS) rows - the six columns above and 6 = flag word.  With bit 0 window pixel (Y, X) reads the resized image at (Y, W - 1 - X),
 * with bit 1 at (H - 1 - Y, X); the resize geometry is the unflipped image's.  A multi-scale view needs nothing here: it is the
 * same source address with another (H, W).  Same kernel body (the coordinates are exact integers however they are reached):
 * flags 0 give the entry above bit for bit.  One row per view: an image with V views has V rows.  Same checks, limits and bound. */
#define SEGCLIP_SEG_SOURCE_VIEW_COLS 7 /* int64 columns of one row of the view entry's source table */
int segclip_seg_view_windows_from_u8(const int64_t* images, const int32_t* windows, int64_t n_windows, int64_t B, int64_t win_h,
                                     int64_t win_w, const float* mean, const float* inv_std, int reverse_channels, float* out,
                                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Rendering of segmentation results (segment_render.inc): what the reference's demo draws, for images of mixed sizes in ONE
 * launch per entry.
 *
 * segclip_seg_groups_rescaled: the group map at each image's output size.  Replaces get_attn_maps
 * (seg_segmentation/evaluation/vit_seg.py:144-200: resize_attn_map to the network size, :180) and the group branch of
 * show_result (:359-362: F.interpolate to the picture's size, arg-max over the groups).  An output pixel of an image with
 * network size (H, W), grid (grid_h, grid_w) and output size (oh, ow): taps and weights on the (H, W) grid as in
 * segclip_seg_label_map_rescaled; at each tap, per group, the value of soft_attn resized to (H, W) as segclip_seg_label_map
 * forms it (four grid values); per group the blend h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11) in fp32; first
 * maximum over the groups; one byte.  A tap of weight 0 is not evaluated, and where one network pixel remains the group is
 * formed by the label-map entry's own device function: (oh, ow) = (H, W) reproduces its `groups` bit for bit.  Neither the
 * (G, H, W) nor the (G, oh, ow) array exists.
 *   soft_attn : flat fp32 of soft_floats elements
 *   images    : the (B, 16) int64 table of segclip_seg_label_map_rescaled, with column 6 = offset of the image's oh * ow
 *               group bytes in `groups` (a multiple of 4 gives dword stores), column 8 = its first workgroup = the sum of
 *               ceil(oh * ow / 1024) over the images before it, column 13 = offset of its window in soft_attn; 0 and 7 unused
 *   n_blocks  : the sum of ceil(oh * ow / SEGCLIP_SEG_RENDER_TILE) over all images;  groups: flat uint8 of groups_bytes
 *   Group maps are defined for exactly ONE window per image, the image itself.  Every row is range-checked on the device: an
 *   image whose window count (column 1) is not 1, whose window size (9, 10) is not (H, W), whose sizes are outside
 *   [1, 2^30) or oh * ow >= 2^31, or whose offsets are inconsistent with soft_floats or groups_bytes is SKIPPED (its bytes
 *   stay as they were).  The grid rows a workgroup's 1024 pixels reach are staged in LDS when G * rows * grid_w <= 6400
 *   floats (a whole 8 x 28 x 28 window fits), read from global memory otherwise.
 *   SEGCLIP_ERR_UNSUPPORTED: G > 8.  Bound: HBM writes, 1 byte per output pixel.
 *
 * segclip_seg_blend: the overlay of blend_result (vit_seg.py:258-284) on the decoded images and, with `sums`, the sums that
 * seg2coord (:100-115) averages into the label anchors of vis_mode="input_pred_label" (:299-320), in the same pass.
 *   images  : (B, SEGCLIP_SEG_BLEND_COLS) int64 rows on the device: 0 address of the source (uint8, HWC, 3 interleaved
 *             channels)  1 h  2 w  3 row stride in bytes (>= 3 w)  4 offset of the image's h * w indices in `maps`  5 offset of its 3 * h * w
 *             output bytes in `out`  6 its first workgroup = the sum of ceil(h * w / 1024) over the images before it  7 0
 *   n_blocks: the sum of ceil(h * w / SEGCLIP_SEG_RENDER_TILE) over all images
 *   maps    : flat uint8 of maps_bytes: per pixel the palette index (a label or a group)
 *   palette : (P, 3) uint8, RGB, 1 <= P <= 256 (checked on the host).  reverse_channels: the source is BGR, palette channel c
 *             meets image channel 2 - c (:272)
 *   a, b    : 1.0 - opacity and opacity as fp64, computed by the caller as numpy computes them; 0 <= a < 1, 0 < b <= 1
 *   out     : flat uint8 of out_bytes, (h, w, 3) per image in the source's channel order; must not overlap a source
 *   out = (uint8) trunc(fl(fl(p * a) + fl(c * b))) in fp64 with p the source byte and c the palette byte: two rounded
 *   products and one rounded sum, NOT a fused multiply-add (:276-279; fp32 or a fused sum give other bytes).  An index >= P
 *   has colour (0, 0, 0) (color_seg stays zero, :268-270).  With skip_zero a pixel of index 0 is copied (fg_mask, :274-276).
 *   sums    : (B, P, 3) int64 or NULL, ADDED to: per image and index the pixel count, the sum of y and the sum of x.  Index 0
 *             is counted whatever skip_zero says; an index >= P is not counted.  Per-workgroup int32 counters in LDS, one
 *             64-bit global add per touched counter: the sums do not depend on order.  A workgroup's tile is 1024 pixels;
 *             with h, w < 2^15 its sums stay below 2^25 (the scheme's limit is a tile of 2^16 pixels: 2^16 * 2^15 = 2^31).
 *   Every row is range-checked on the device.  An image whose row has a null address, a stride below 3 w, h or w outside
 *   [1, 2^15), or offsets inconsistent with maps_bytes or out_bytes is SKIPPED: nothing of it is read, written or counted.
 *   A lane owns 4 consecutive pixels of the flat (h, w) image: dword accesses where the unit is whole and its map, source
 *   and output addresses are multiples of 4 (offsets that are multiples of 4 and a contiguous dword-aligned source give
 *   that at every unit; with a padded row stride the source decides per unit), byte accesses otherwise - any w, any stride.
 *   Bound: HBM traffic, 3 + 1 bytes read and 3 written per pixel.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_RENDER_TILE 1024 /* pixels of one workgroup of both entries */
#define SEGCLIP_SEG_BLEND_COLS 8     /* int64 columns of one row of the blend table */
int segclip_seg_groups_rescaled(const float* soft_attn, int64_t soft_floats, const int64_t* images, int64_t B, int64_t n_blocks,
                                int64_t G, uint8_t* groups, int64_t groups_bytes, void* stream);
int segclip_seg_blend(const int64_t* images, int64_t B, int64_t n_blocks, const uint8_t* maps, int64_t maps_bytes,
                      const uint8_t* palette, int64_t P, int reverse_channels, double a, double b, int skip_zero, uint8_t* out,
                      int64_t out_bytes, int64_t* sums, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pixel-adaptive refinement of label maps (segment_refine.inc): PAMR (Araslanov & Roth, CVPR 2020), the post-processing step
 * with which the zero-shot segmentation systems after SegCLIP report their numbers.  THE REFERENCE HAS NO SUCH OP: the
 * definition is this project's, stated here and restated in fp64 by tests/pamr_reference.py.
 *
 * Per image: picture R (h, w, 3) uint8, label map L (h, w) uint8, C <= 256 classes, the transform's mean[3] and 1 / std[3]
 * (RGB order; with reverse_channels the picture is BGR and its channel s meets entry 2 - s, as in
 * segclip_seg_windows_from_u8), dilations d_1 < ... < d_D, T iterations.
 *   x_c(p)   = (R_c(p) - mean_c) / std_c
 *   q_n(p)   = clamp(p + d o), the 8 D neighbours of p, dilation-major, o over (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1),
 *              (1,0), (1,1) in (row, column) order; coordinates clamped to the picture (replicate padding)
 *   sigma_c(p) = the unbiased standard deviation (divisor 9 D - 1) over the 8 D values x_c(q_n(p)) and D copies of x_c(p)
 *   a(p, n)  = -(1/3) sum_c |x_c(p) - x_c(q_n(p))| / (1e-8 + 0.1 sigma_c(p));   w(p, .) = softmax_n a(p, n)
 *   m0_k(p)  = [L(p) = k] for k < C;   m(t+1)_k(p) = sum_n w(p, n) mt_k(q_n(p))
 *   L'(p)    = the smallest k that attains max_k mT_k(p)
 *   T = 0 gives L' = L.  A byte >= C belongs to no plane.  A pixel whose planes are all zero keeps its input byte.
 * x enters through differences to the centre only, so the mean cancels (it is taken for the definition's sake), and sigma is
 * formed from the integer byte differences d to the centre, exactly: var = (9 D sum d^2 - (sum d)^2) / (9 D (9 D - 1)) / std^2
 * with D zeros for the centre copies - never E[x^2] - E[x]^2 of the normalised values.  All other math is fp32; a pixel's sum
 * over n runs in the order of n with fused multiply-adds and there are no float atomics: two calls give the same bits.
 *
 *   images   : (B, SEGCLIP_SEG_REFINE_COLS) int64 rows on the device: 0 address of the picture (uint8, HWC, 3 interleaved
 *              channels)  1 h  2 w  3 row stride in bytes (>= 3 w)  4 offset of the image's h * w bytes in `labels` AND `out` (and its pixel index
 *              in the workspace)  5 offset of its h * w bytes in `gt`, or -1  6 its first workgroup = the sum of
 *              ceil(h * w / SEGCLIP_SEG_REFINE_TILE) over the images before it  7 0
 *   n_blocks : the sum of ceil(h * w / SEGCLIP_SEG_REFINE_TILE) over all images;  max_side: the caller's bound on every h and w
 *   labels   : flat uint8 of labels_bytes, read only;  out: flat uint8 of out_bytes = labels_bytes, must not overlap labels
 *   gt/areas : optional flat uint8 ground truth and the (3, C) int64 areas of segclip_seg_areas, ADDED to for the refined
 *              labels by the last kernel (integer adds: no order dependence)
 *   probs    : optional, B = 1 only: (C, h, w) fp32, the final planes mT (cleared, then written; for tests and inspection)
 *   ws       : segclip_seg_refine_ws_bytes(labels_bytes, B, D) bytes, 16-byte aligned; not needed for T = 0.  It does NOT
 *              depend on C: the planes of different classes never meet before the arg-max, so they pass through the
 *              iterations in chunks of 8, in one fp32 buffer pair of 8 planes (two float4 per pixel), with a running (best value, best
 *              label) pair per pixel.  Only labels present in an image carry a non-zero plane: a 256-bit presence map per
 *              image is built on the device, the present labels get compact ids in ascending order, and the workgroups of a
 *              chunk beyond an image's label count exit at once.
 *   The entry enqueues the whole sequence without a host synchronisation: two clears, the weights kernel (once), and
 *   ceil(C / 8) * T step kernels; the first step reads the label bytes (no one-hot pass), the last one of an image's last
 *   chunk writes the label and counts the areas.
 *   Every table row is range-checked on the device: an image with a null address, h or w outside [1, min(max_side, 2^15 - 1)],
 *   a stride below 3 w or offsets inconsistent with labels_bytes is SKIPPED (nothing of it read, written or counted); with gt
 *   offsets inconsistent with gt_bytes it is refined but not counted.
 *   SEGCLIP_ERR_UNSUPPORTED, nothing launched and nothing written: D outside 1..SEGCLIP_SEG_REFINE_MAX_DILATIONS, a dilation
 *   outside 1..SEGCLIP_SEG_REFINE_MAX_DILATION or not increasing, T outside 0..SEGCLIP_SEG_REFINE_MAX_ITERS, C outside 1..256, max_side outside [1, 2^15), a workspace smaller than ws_bytes.  SEGCLIP_ERR_INVALID:
 *   out overlapping labels, out_bytes != labels_bytes, probs with B != 1, gt without areas, missing pointers.
 *   Traffic per pixel, iteration and chunk of 8 planes: 32 D bytes of weights + 32 bytes of planes written from / to memory,
 *   and 8 D taps of 32 bytes served by the caches (dilations up to 32: an LDS halo tile does not pay).
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_REFINE_TILE 256        /* pixels of one workgroup */
#define SEGCLIP_SEG_REFINE_COLS 8          /* int64 columns of one row of the image table */
#define SEGCLIP_SEG_REFINE_MAX_DILATIONS 6 /* D */
#define SEGCLIP_SEG_REFINE_MAX_DILATION 32 /* the largest d */
#define SEGCLIP_SEG_REFINE_MAX_ITERS 32    /* T */
int64_t segclip_seg_refine_ws_bytes(int64_t labels_bytes, int64_t B, int64_t D);
int segclip_seg_refine(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint8_t* labels,
                       int64_t labels_bytes, int64_t C, const int32_t* dilations, int64_t D, int64_t T, const float* mean,
                       const float* inv_std, int reverse_channels, uint8_t* out, int64_t out_bytes, const uint8_t* gt,
                       int64_t gt_bytes, int ignore_index, int reduce_zero_label, int64_t* areas, float* probs,
                       int64_t probs_floats, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of label maps (segment_objects.inc): component ids, areas, a compact list of objects with their boxes
 * and coordinate sums, and despeckled maps, for images of mixed sizes in one call.  THE REFERENCE HAS NO SUCH OP: the
 * definition is this project's, stated here and restated with a plain union-find by tests/cc_reference.py.
 *
 * Per image: label map L (h, w) uint8, connectivity 4 or 8, skip_label in 0..255 or -1 for none.
 *   A component is a maximal set of pixels with the same byte that is connected under the connectivity (4: left / right /
 *   up / down; 8: the diagonals too).  Pixels whose byte is skip_label belong to no component.
 *   The id of a component is the smallest flat in-image index y * w + x of its pixels: its first pixel in raster order.
 *   Ids, areas, boxes and sums are integers and the ids depend on no scheduling: two calls give the same bits.
 *   ids[p]     = the id of p's component, or -1 for a skipped pixel
 *   area_px[p] = the pixel count of p's component, or 0 for a skipped pixel
 *   records    : one row of SEGCLIP_SEG_CC_RECORD int64 per component, rows in ascending (image, id) order:
 *                image, id, label, area, y0, x0, y1, x1, sum of y, sum of x over its pixels; y1 and x1 are EXCLUSIVE (the box
 *                is rows y0..y1-1, columns x0..x1-1, as scipy.ndimage.find_objects gives slices)
 *   count[0]   = the number of components of all images, also when it exceeds K; then exactly the first K rows in that order
 *                are written and nothing beyond records + 10 K
 *   cleaned[p] = fill where p is not skipped and area_px[p] < min_area, otherwise L[p].  ONE PASS: pixels that become `fill`
 *                are not merged again with neighbours that carry `fill` already, and nothing is labelled twice.
 *
 *   images   : (B, SEGCLIP_SEG_CC_COLS) int64 rows on the device: 0 h  1 w  2 offset of the image's h * w entries in `labels`,
 *              `ids`, `area_px` AND `cleaned`  3 its first workgroup = the sum of ceil(h / SEGCLIP_SEG_CC_TILE_H) *
 *              ceil(w / SEGCLIP_SEG_CC_TILE_W) over the images before it  4-7 0
 *   n_blocks : that sum over all images (the tile is SEGCLIP_SEG_CC_TILE_H rows x SEGCLIP_SEG_CC_TILE_W columns);  max_side: the caller's bound on every h and w
 *   labels   : flat uint8 of labels_bytes, read only
 *   ids, area_px : optional flat int32 of px_count = labels_bytes entries
 *   records  : optional (K, 10) int64; needs count.  count: optional, one int64
 *   cleaned  : optional flat uint8 of cleaned_bytes = labels_bytes, must not overlap labels; min_area >= 0, fill in 0..255
 *   ws       : segclip_seg_components_ws_bytes(labels_bytes, B, n_blocks) bytes (16 per pixel + about 130 per workgroup), 16-byte
 *              aligned
 *   Every output is optional; the entry enqueues its kernels without a host synchronisation: the tiles' union-find in LDS,
 *   the merge across the tiles' rims (atomicMin on a flat int32 parent array; parents only ever decrease, every retry
 *   continues from a strictly smaller index, and no workgroup waits for another), with count a root count per row segment,
 *   one scan and the ranks, then areas / boxes / sums reduced in LDS and added with one set of integer atomics per (tile,
 *   tile-local component), and the pass that writes area_px and cleaned.
 *   Every table row is range-checked on the device: an image with h or w outside [1, min(max_side, 2^15 - 1)], offsets
 *   inconsistent with labels_bytes or workgroups beyond n_blocks is SKIPPED (nothing of it read, written or counted).
 *   SEGCLIP_ERR_UNSUPPORTED, nothing launched and nothing written: connectivity other than 4 or 8, skip_label outside
 *   -1..255, fill outside 0..255, min_area < 0, max_side outside [1, 2^15), a workspace smaller than ws_bytes.
 *   SEGCLIP_ERR_INVALID: records without count, cleaned overlapping labels, cleaned_bytes != labels_bytes,
 *   px_count != labels_bytes with ids or area_px, missing pointers.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_CC_TILE_H 16 /* rows and */
#define SEGCLIP_SEG_CC_TILE_W 64 /* columns of one workgroup's tile */
#define SEGCLIP_SEG_CC_COLS 8    /* int64 columns of one row of the image table */
#define SEGCLIP_SEG_CC_RECORD 10 /* int64 columns of a record */
int64_t segclip_seg_components_ws_bytes(int64_t labels_bytes, int64_t B, int64_t n_blocks);
int segclip_seg_components(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint8_t* labels,
                           int64_t labels_bytes, int connectivity, int skip_label, int32_t* ids, int32_t* area_px,
                           int64_t px_count, int64_t* records, int64_t K, int64_t* count, int64_t min_area, int fill,
                           uint8_t* cleaned, int64_t cleaned_bytes, void* ws, int64_t ws_bytes, void* stream);
/* segclip_seg_components_wide: the definition above for 16-bit label maps (those of segclip_seg_label_map_rescaled_wide), with
 * "byte" read as "16-bit value".  labels and cleaned are flat uint16 (an int16 tensor is read as unsigned); labels_n, cleaned_n,
 * px_count and the table's offsets count ELEMENTS.  skip_label is in -1..65535 and fill in 0..65535: 65535 and every value with
 * the top bit set are labels like any other.  Column 2 of a record carries the 16-bit label.  The same table, the same
 * device-side range checks, the same refusals with these ranges.  The workspace holds no labels: it is
 * segclip_seg_components_ws_bytes(labels_n, B, n_blocks). */
int segclip_seg_components_wide(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint16_t* labels,
                                int64_t labels_n, int connectivity, int skip_label, int32_t* ids, int32_t* area_px,
                                int64_t px_count, int64_t* records, int64_t K, int64_t* count, int64_t min_area, int fill,
                                uint16_t* cleaned, int64_t cleaned_n, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Despeckling by merging (segment_sieve.inc): every small connected component of a label map takes the label of its largest
 * neighbour, in 1..SEGCLIP_SEG_SIEVE_MAX_ROUNDS rounds, for images of mixed sizes in one call: what a sieve filter does in the raster toolkits.  It is for
 * vocabularies without a background class, where segclip_seg_components' constant `fill` paints the specks with a real class.
 * THE REFERENCE HAS NO SUCH OP: the definition is this project's, stated here and restated by tests/cc_merge_reference.py.
 *
 * A ROUND, per image: label map L (h, w) uint8, connectivity 4 or 8, skip_label in 0..255 or -1 for none, min_area >= 0.
 *   Components and areas are exactly those of segclip_seg_components.  Skipped pixels belong to no component: they are never
 *   changed and never voted for.  A component is SMALL when its area < min_area, otherwise it is KEPT.
 *   The CANDIDATES of a small component S are the kept components that own at least one pixel 4-adjacent (left, right, up,
 *   down, inside the image) to a pixel of S.  Contacts are 4-adjacent whatever the connectivity of the components (a
 *   4-neighbour in another component therefore always carries another byte); a diagonal touch is no contact.
 *   The WINNER is the candidate with the largest area, among equal areas the one with the smallest label (two candidates
 *   that tie in both give the same byte): in integers the maximum of (area << 8) | (255 - label) over all contacts, so the
 *   result depends on no scheduling and two calls give the same bits.
 *   Every pixel of a small component with a winner takes the winner's label.  A small component without a candidate is an
 *   ORPHAN and keeps its label.  All other pixels keep theirs.
 * ROUNDS: round r + 1 runs on the output of round r with the components formed anew (a speck nested in a speck needs two).
 *   After the LAST round only, the orphans become orphan_fill if it is 0..255; with -1 they stay.  A round that changes nothing
 *   is a fixed point.  min_area 0 and 1 return the input.
 *
 *   images, n_blocks, max_side, labels, labels_bytes, connectivity, skip_label: as for segclip_seg_components (the same table)
 *   cleaned  : flat uint8 of cleaned_bytes = labels_bytes with the labels' offsets, must not overlap labels; only the pixels of
 *              the table's images are written
 *   ws       : segclip_seg_sieve_ws_bytes(labels_bytes, B, n_blocks) bytes = 21 per pixel (8 slot, 4 parent, 4 root, 4 area, 1
 *              for the map between two rounds), each part rounded up to 256; 16-byte aligned
 *   Every round enqueues, without a host synchronisation: the clearing of the slots, the component kernels of
 *   segclip_seg_components up to the areas (no root count, scan or ranks), the vote (keys reduced with 64-bit atomicMax in LDS
 *   per tile-local group, then ONE global 64-bit atomicMax per (tile, group) on the slot at the component's root, which is
 *   how a component that spans tiles sees a neighbour that touches it in another tile) and the pass that writes the winners.
 *   The rounds alternate between `cleaned` and the workspace so that the last one lands in `cleaned`.
 *   Traffic per pixel and round beyond the component kernels (13 B read + 12 written): 8 B of slot cleared; vote: 4 B of
 *   root + the gathered area; a pixel of a small component also reads its 4 neighbours' roots, areas and labels; 8 B per
 *   (tile, voting group); final: 4 B of root + the gathered area + 1 B read, 1 B written, 8 B of slot per small pixel.
 *   A bad table row is SKIPPED on the device as in segclip_seg_components (nothing of that image read or written).
 *   SEGCLIP_ERR_UNSUPPORTED, nothing launched and nothing written: rounds outside 1..SEGCLIP_SEG_SIEVE_MAX_ROUNDS, orphan_fill outside -1..255,
 *   connectivity other than 4 or 8, skip_label outside -1..255, min_area < 0, max_side outside [1, 2^15), a workspace smaller
 *   than ws_bytes.  SEGCLIP_ERR_INVALID: cleaned overlapping labels, cleaned_bytes != labels_bytes, missing pointers.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_SIEVE_MAX_ROUNDS 8
int64_t segclip_seg_sieve_ws_bytes(int64_t labels_bytes, int64_t B, int64_t n_blocks);
int segclip_seg_sieve(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint8_t* labels,
                      int64_t labels_bytes, int connectivity, int skip_label, int64_t min_area, int orphan_fill, int rounds,
                      uint8_t* cleaned, int64_t cleaned_bytes, void* ws, int64_t ws_bytes, void* stream);
/* segclip_seg_sieve_wide: the definition above for 16-bit label maps, with "byte" read as "16-bit value".  labels and cleaned
 * are flat uint16 (an int16 tensor is read as unsigned); labels_n, cleaned_n and the table's offsets count ELEMENTS.  The winner
 * is the maximum of (area << 16) | (65535 - label) over all contacts (an area is below 2^30: 46 bits; zero remains "no contact").
 * skip_label and orphan_fill are in -1..65535.  The same table, the same device-side range checks, the same refusals with these
 * ranges.  ws: segclip_seg_sieve_wide_ws_bytes(labels_n, B, n_blocks) bytes = 22 per pixel (2 for the map between two rounds). */
int64_t segclip_seg_sieve_wide_ws_bytes(int64_t labels_n, int64_t B, int64_t n_blocks);
int segclip_seg_sieve_wide(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint16_t* labels,
                           int64_t labels_n, int connectivity, int skip_label, int64_t min_area, int orphan_fill, int rounds,
                           uint16_t* cleaned, int64_t cleaned_n, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Superpixels of decoded pictures (segment_superpixel.inc): an integer SLIC (after Achanta et al., TPAMI 2012) on the RGB bytes,
 * for pictures of mixed sizes in one call.  THE REFERENCE HAS NO SUCH OP: the definition is this project's, stated here and
 * restated in numpy by tests/superpixel_reference.py.  Everything is integer arithmetic - no float appears anywhere - so the
 * order of the atomics cannot change a result and two calls give the same bits.
 *
 * Per image: picture R (h, w, 3) uint8, step S, compactness m, T rounds.
 *   Grid     : gh = ceil(h / S), gw = ceil(w / S), K = gh gw.  Centre k = i gw + j belongs to cell (i, j) for good.
 *   A centre is five integers (y, x, r, g, b).  Initially y = min(i S + S / 2, h - 1), x = min(j S + S / 2, w - 1) (integer
 *   division) and (r, g, b) the picture's bytes there.
 *   Assignment of pixel (y, x): its home cell is (y / S, x / S); its candidates are the centres of the 3 x 3 cells around the
 *   home cell that lie inside the grid, wherever those centres have moved.  D = S^2 dc^2 + m^2 ds^2 with dc^2 the sum of the
 *   three squared byte differences and ds^2 = dy^2 + dx^2.  The pixel takes the candidate with the smallest D, among equal D
 *   the smallest centre index.
 *   Update   : a centre with n > 0 members becomes the floor-divided means (sum / n) of its members' y, x, r, g, b; a centre
 *   without members keeps its values.
 *   T rounds of (assignment, update), then one final assignment: ids[p] = the index k of p's centre, in [0, K).  Ids may be
 *   unused and a segment need not be connected: NO CONNECTIVITY PASS belongs to this definition (segclip_seg_components gives
 *   the connected parts of any id map to a caller who wants them).
 *   Limits   : SEGCLIP_SEG_SP_MIN_STEP <= S <= SEGCLIP_SEG_SP_MAX_STEP, 1 <= m <= SEGCLIP_SEG_SP_MAX_COMPACTNESS,
 *   0 <= T <= SEGCLIP_SEG_SP_MAX_ITERS, sides below SEGCLIP_SEG_SOURCE_LIMIT = 2^15.  Under them
 *     D < 2^31   : a centre's members come from its 3 x 3 cells, so it stays inside them and ds^2 <= 18 S^2 for a candidate;
 *                  S^2 195075 + m^2 18 S^2 < 2^31 at S = m = 64 (195075 = 3 * 255^2)
 *     sums < 2^32: a centre has at most 9 S^2 = 36,864 members, each coordinate below 2^15 and each byte below 2^8
 *
 *   images   : (B, SEGCLIP_SEG_SP_COLS) int64 rows on the device: 0 address of the picture (uint8, HWC, 3 interleaved channels)
 *              1 h  2 w  3 row stride in bytes (>= 3 w)  4 offset of the image's h * w entries in `ids`  5 its first centre =
 *              the sum of K over the images before it (its rows in `centres`)  6 its first workgroup = the sum of
 *              ceil(h / SEGCLIP_SEG_SP_TILE_H) * ceil(w / SEGCLIP_SEG_SP_TILE_W) over the images before it  7 0
 *   n_blocks : that sum over all images;  max_side: the caller's bound on every h and w
 *   ids      : flat int32 of ids_n entries; only the pixels of the table's images are written
 *   K_total  : the sum of K over all images (at most 2^28);  centres: optional (K_total, 5) int32, the final centres
 *   ws       : segclip_seg_superpixels_ws_bytes(K_total) bytes (44 per centre), 16-byte aligned
 *   The entry enqueues, without a host synchronisation and with all images in every launch: the initialisation, T x (assign and
 *   sum, update) and the final assignment.  A workgroup owns a tile of SEGCLIP_SEG_SP_TILE_H x SEGCLIP_SEG_SP_TILE_W pixels of
 *   one image, stages the centres of the cells its tile touches plus one ring in LDS (at step 4, which puts the most centres in
 *   a tile, (TILE_H / 4 + 2) * (TILE_W / 4 + 2) = 180 of them in 7.9 KiB of static LDS), sums (n, y, x, r, g, b) per staged
 *   centre with LDS integer atomics and adds the rows that are not zero with one set of global integer atomics per (tile,
 *   centre).  Traffic per round: 3 B per pixel read + the per-tile atomics; the final assignment adds 4 B per pixel of ids.
 *   Every table row is range-checked on the device: an image with a null address, h or w outside [1, min(max_side, 2^15 - 1)],
 *   a stride below 3 w, offsets inconsistent with ids_n or K_total or workgroups beyond n_blocks is SKIPPED (nothing of it
 *   read or written).
 *   SEGCLIP_ERR_UNSUPPORTED, nothing launched and nothing written: S, m or T outside the limits, max_side outside [1, 2^15),
 *   K_total above 2^28, a workspace smaller than ws_bytes.  SEGCLIP_ERR_INVALID: negative sizes, missing pointers.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_SP_TILE_H 32 /* rows and */
#define SEGCLIP_SEG_SP_TILE_W 64 /* columns of one workgroup's tile */
#define SEGCLIP_SEG_SP_COLS 8    /* int64 columns of one row of the image table */
#define SEGCLIP_SEG_SP_MIN_STEP 4
#define SEGCLIP_SEG_SP_MAX_STEP 64
#define SEGCLIP_SEG_SP_MAX_COMPACTNESS 64
#define SEGCLIP_SEG_SP_MAX_ITERS 16
int64_t segclip_seg_superpixels_ws_bytes(int64_t K_total);
int segclip_seg_superpixels(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, int64_t step, int64_t compactness,
                            int64_t iters, int32_t* ids, int64_t ids_n, int64_t K_total, int32_t* centres, void* ws, int64_t ws_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Majority voting of label maps inside segments (segment_vote.inc): every segment gives its pixels the label most of them
 * carry.  The segments are superpixels of segclip_seg_superpixels or ids of the caller's own (Felzenszwalb maps, flattened
 * instance masks).  THE REFERENCE HAS NO SUCH OP: the definition is this project's, stated here and restated in numpy by
 * tests/superpixel_reference.py.  Integer counts: no dependence on the order of the atomics.
 *
 * Per image: label map L (n pixels), segment map G (n int32), the image's segment count K, C classes, min_share in 0..100.
 *   A pixel VOTES when L(p) < C and 0 <= G(p) < K.
 *   For a segment with tot > 0 voters: top = the largest per-class count, win = the smallest class that reaches it; the segment
 *   SNAPS when 100 top >= min_share tot.
 *   A voting pixel of a snapping segment takes win.  Every other pixel keeps its value: a label >= C (255 as an ignore value),
 *   an id outside [0, K), a segment that does not snap.
 *
 *   images   : (B, SEGCLIP_SEG_VOTE_COLS) int64 rows on the device: 0 offset of the image's n entries in `labels`, `segments`
 *              AND `out`  1 n = h * w  2 its first segment = the sum of K over the images before it (its rows of the count
 *              table)  3 K  4 its first workgroup = the sum of ceil(n / SEGCLIP_SEG_VOTE_TILE) over the images before it  5-7 0
 *   n_blocks : that sum over all images;  max_k: the caller's bound on every K, at most SEGCLIP_SEG_VOTE_MAX_SEGMENTS
 *   labels   : flat uint8 of labels_bytes, read only;  segments: flat int32 of segments_n = labels_bytes entries
 *   K_total  : the sum of K over all images;  1 <= C <= 256
 *   out      : flat uint8 of out_bytes = labels_bytes, must not overlap labels; only the pixels of the table's images are written
 *   ws       : segclip_seg_vote_ws_bytes(K_total, C) bytes: the (K_total, C) int32 counts and K_total int32 winners, 16-byte
 *              aligned; cleared inside the call
 *   Three passes, enqueued without a host synchronisation: the count (a workgroup stages the (segment, class) pairs of its
 *   pixels in an open-addressing table in LDS - a caller's map gives no bound on the segments of a tile - and adds each with
 *   one global atomic; a pair that finds no slot is added at once), the winner (one wave per segment: lanes stride the
 *   classes, a shuffle reduction to the largest count and among equal counts the lowest class; -1 for "does not snap") and
 *   the pass that writes `out`.  Traffic: about 9 B per pixel (11 with 16-bit labels) + K_total * C * 4 B of table cleared and read.
 *   Every table row is range-checked on the device: an image with n outside [1, 2^30), K outside [1, max_k], offsets
 *   inconsistent with labels_bytes or K_total or workgroups beyond n_blocks is SKIPPED (nothing of it read, written or counted).
 *   SEGCLIP_ERR_UNSUPPORTED, nothing launched and nothing written: C outside 1..256, min_share outside 0..100, max_k outside
 *   1..SEGCLIP_SEG_VOTE_MAX_SEGMENTS, K_total * C above 2^28, a workspace smaller than ws_bytes.  SEGCLIP_ERR_INVALID: out
 *   overlapping labels, out_bytes or segments_n != labels_bytes, missing pointers.
 * segclip_seg_vote_wide: the same for 16-bit label maps: labels and out are flat uint16 (an int16 tensor is read as unsigned),
 * labels_n, out_n and the table's offsets count ELEMENTS, 1 <= C <= SEGCLIP_SEG_WIDE_MAX_CLASSES.  The same table, workspace
 * query, range checks and refusals.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_VOTE_TILE 2048            /* pixels of one workgroup */
#define SEGCLIP_SEG_VOTE_COLS 8               /* int64 columns of one row of the image table */
#define SEGCLIP_SEG_VOTE_MAX_SEGMENTS 1048576 /* 2^20: K of one image */
int64_t segclip_seg_vote_ws_bytes(int64_t K_total, int64_t C);
int segclip_seg_vote(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_k, const uint8_t* labels, int64_t labels_bytes,
                     const int32_t* segments, int64_t segments_n, int64_t K_total, int64_t C, int min_share, uint8_t* out,
                     int64_t out_bytes, void* ws, int64_t ws_bytes, void* stream);
int segclip_seg_vote_wide(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_k, const uint16_t* labels, int64_t labels_n,
                          const int32_t* segments, int64_t segments_n, int64_t K_total, int64_t C, int min_share, uint16_t* out,
                          int64_t out_n, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Boundary metrics of label maps (segment_boundary.inc): the boundary bands of a prediction and a ground truth, and the
 * per-class areas of Boundary IoU (Cheng et al., CVPR 2021) and of the trimap mIoU of the DeepLab papers, for maps of mixed
 * sizes in one call.  THE REFERENCE HAS NO SUCH OP: the definition is this project's, stated here and restated with the
 * brute-force window by tests/boundary_reference.py.
 *
 * Per map M (h, w) uint8 and radius d >= 1, the BAND BYTE of the pixel p = (y, x):
 *   bit 0: some pixel p' = (y', x') OF THE MAP with |y - y'| <= d and |x - x'| <= d has M[p'] != M[p]
 *   bit 1: the (2d+1)^2 window around p leaves the map: y < d, x < d, y >= h - d or x >= w - d
 *   band != 0 is, for every class k at once, the official mask_to_boundary(M == k, d) of Boundary IoU (one ring of zeros
 *   around the mask, d erosions with a 3 x 3 kernel, the mask minus its erosion): that result equals (M == k) & (band != 0).
 *   The radius of a map is the caller's; Boundary IoU takes d = max(1, round(0.02 * sqrt(h * h + w * w))).
 * Areas: a (2, 3, C) int64 tensor that is ADDED to.  q = the prediction's byte, g = the ground truth's, bp and bg their band
 *   bytes.  The bands are formed on the raw bytes: an ignored region is a region like any other.  The ground-truth rule is
 *   segclip_seg_areas': a pixel with g == ignore_index contributes nothing; with reduce_zero_label a pixel with g == 0
 *   contributes nothing either and every other g counts as g' = g - 1 (otherwise g' = g); a value >= C adds to the other
 *   side's areas only.
 *   areas[0] Boundary IoU: I[k] += [q = k, g' = k, bp != 0, bg != 0]   P[k] += [q = k, bp != 0]   L[k] += [g' = k, bg != 0]
 *   areas[1] trimap      : the I / P / L of segclip_seg_areas over the pixels with bg & 1, those within d of a change of the
 *                          ground truth's byte (the picture frame is no change)
 *   With d >= max(h, w) every band byte is non-zero and areas[0] is segclip_seg_areas'; a ground truth of one single byte
 *   leaves areas[1] as it was.
 *
 *   images   : (B, SEGCLIP_SEG_BOUNDARY_COLS) int64 rows on the device: 0 h  1 w  2 offset of the map's h * w bytes in `pred` AND
 *              `pred_band`
 *              3 its offset in `gt` AND `gt_band`, or -1 for a map without a ground truth (not looked at when gt is null)
 *              4 its radius d  5 its first workgroup = the sum of ceil(ceil(h / 32) * ceil(w / 64) / 4) over the maps
 *              before it  6-7 0
 *   n_blocks : that sum over all maps (a wave owns a strip of SEGCLIP_SEG_BOUNDARY_TILE_H rows x SEGCLIP_SEG_BOUNDARY_TILE_W
 *              columns, a workgroup SEGCLIP_SEG_BOUNDARY_WAVES consecutive strips of a map);  max_side: the caller's bound on every h and w
 *   pred, gt : flat uint8 of pred_bytes / gt_bytes, read only; gt optional.  They have offsets of their own because an
 *              evaluator's label buffer has gaps between its maps and its ground truths lie gapless.
 *   pred_band, gt_band : optional flat uint8 with the layout of pred / gt; gt_band needs gt
 *   areas    : optional (2, 3, C) int64; needs gt.  1 <= C <= 256
 *   ws       : segclip_seg_boundary_ws_bytes(pred_bytes, gt_bytes) bytes (2 per byte of pred and of gt), 16-byte aligned
 *   The entry enqueues two kernels without a host synchronisation.  The first counts, per row, the changes of byte from its
 *   left end to every pixel (uint16 in ws): the part [x - d, x + d] of a row is constant exactly when the counts at its two
 *   ends agree.  The second walks down the columns: the window of p is constant exactly when every row of it has a constant
 *   row part and the byte of p's column does not change over it; a lane remembers the last row of either kind, d rows ahead
 *   of the pixel it emits.  Work per pixel is (32 + 2 d) / 32 row visits, never d^2.  The areas are counted in LDS and added
 *   with one integer atomic per touched counter and workgroup: the sums depend on no schedule.
 *   Every table row is range-checked on the device: a map with h or w outside [1, min(max_side, 2^15 - 1)], a radius outside
 *   [1, SEGCLIP_SEG_BOUNDARY_MAX_RADIUS], offsets inconsistent with pred_bytes / gt_bytes or workgroups beyond n_blocks is SKIPPED (nothing of it read,
 *   written or counted).
 *   SEGCLIP_ERR_UNSUPPORTED, nothing launched and nothing written: C > 256, max_side outside [1, 2^15), a workspace smaller
 *   than ws_bytes.
 *   SEGCLIP_ERR_INVALID: areas or gt_band without gt, a band output overlapping an input or the other band, C < 1, missing
 *   pointers.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_BOUNDARY_TILE_H 32      /* rows and */
#define SEGCLIP_SEG_BOUNDARY_TILE_W 64      /* columns of one wave's strip */
#define SEGCLIP_SEG_BOUNDARY_WAVES 4        /* consecutive strips of a map that share a workgroup */
#define SEGCLIP_SEG_BOUNDARY_COLS 8         /* int64 columns of one row of the image table */
#define SEGCLIP_SEG_BOUNDARY_MAX_RADIUS 128
int64_t segclip_seg_boundary_ws_bytes(int64_t pred_bytes, int64_t gt_bytes);
int segclip_seg_boundary(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint8_t* pred,
                         int64_t pred_bytes, const uint8_t* gt, int64_t gt_bytes, int64_t C, int ignore_index,
                         int reduce_zero_label, uint8_t* pred_band, uint8_t* gt_band, int64_t* areas, void* ws, int64_t ws_bytes,
                         void* stream);
/* segclip_seg_boundary_wide: the definition above for 16-bit label maps, with "byte" read as "16-bit value" for M, q and g.
 * pred and gt are BOTH flat uint16 (an int16 tensor is read as unsigned) of pred_n / gt_n ELEMENTS, which the table's offsets
 * count too; the bands stay one byte per pixel, with the layout of pred / gt.  1 <= C <= SEGCLIP_SEG_WIDE_MAX_CLASSES (the
 * counters are 24 KB of LDS, which only this entry pays for) and ignore_index in 0..65535: SEGCLIP_ERR_UNSUPPORTED otherwise,
 * nothing launched and nothing written.  The same table, the same device-side range checks, every other refusal as above.
 * ws: segclip_seg_boundary_ws_bytes(pred_n, gt_n) bytes (2 per element). */
int segclip_seg_boundary_wide(const int64_t* images, int64_t B, int64_t n_blocks, int64_t max_side, const uint16_t* pred,
                              int64_t pred_n, const uint16_t* gt, int64_t gt_n, int64_t C, int ignore_index,
                              int reduce_zero_label, uint8_t* pred_band, uint8_t* gt_band, int64_t* areas, void* ws,
                              int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Confusion matrix of label maps (segment_confusion.inc): which class the pixels of a class went to.  THE REFERENCE HAS NO
 * SUCH OP (mmseg's eval_metrics stops at the per-class areas); the definition is this project's, restated by
 * tests/confusion_reference.py.
 *
 * segclip_seg_confusion: n pixels of uint8 label maps, prediction p and raw ground truth g.
 *   conf : a contiguous (C + 1, C + 1) int64 matrix that is ADDED to: row = ground-truth class, column = predicted class,
 *          index C on either axis the "out of range" bin.  The ground-truth rule is segclip_seg_areas', pixel for pixel: a
 *          pixel with g == ignore_index contributes nothing; with reduce_zero_label a pixel with g == 0 contributes nothing
 *          either and every other g counts as g - 1; after that g >= C goes to row C, and p >= C goes to column C.
 *   The areas are a projection of the matrix, for c < C:  areas[0][c] = conf[c][c];  areas[1][c] = the sum of column c over
 *   ALL rows, row C included;  areas[2][c] = the sum of row c over ALL columns, column C included.
 *   How.  A lane reads 16 bytes of pred and of gt per step, two steps in flight; the vector body starts where pred is 16-byte
 *   aligned, gt is read aligned where it is aligned there too and as 16 bytes of element alignment otherwise, and the fewer
 *   than two vectors of elements before and after the body are counted one by one: pred and gt may start at any element,
 *   independently.  Equal consecutive (g, p) pairs of a lane are counted once.  Counters are 32-bit and per workgroup in LDS,
 *   one 64-bit integer atomic per touched cell at the flush: the sums depend on no schedule.  Two routes:
 *     dense  (C <= 180): the whole matrix in LDS, (C + 1)^2 * 4 bytes (90 KiB at 151 classes; past 64 KiB the kernel's limit
 *            is raised, and where the runtime refuses that the sparse route is taken);
 *     sparse (above): an open-addressing table of 4096 (cell, count) slots, 32 KiB, 8 probes; a pair that finds no slot is
 *            added to `conf` directly, so independent random labels are counted exactly as well, only slower.
 *   Grid: grid-stride, 512 threads, at least max(16384, 2 x LDS cells) pixels per workgroup and at most
 *   CUs x min(4, 160 KiB / LDS bytes) workgroups.  One launch counts at most 2^30 pixels - a longer input is split by the
 *   entry - so that no 32-bit counter overflows.  Bound: HBM reads, 2 bytes per pixel (4 for the wide entry).
 *   Measured: profiles/seg_confusion.txt.
 *   0 <= n <= 2^40, C >= 1; n == 0 launches nothing.  SEGCLIP_ERR_UNSUPPORTED (no launch): C > 256.
 *
 * segclip_seg_confusion_wide: the same for n uint16 elements; g is compared with ignore_index as an UNSIGNED 16-bit value.
 *   SEGCLIP_ERR_UNSUPPORTED: C > 1024.
 *
 * segclip_seg_confusion_route: the route the entry takes for C classes on the current device (wide != 0: the uint16 entry):
 *   0 dense, 1 sparse; negative where the entry would refuse (SEGCLIP_ERR_INVALID: C < 1 or no device;
 *   SEGCLIP_ERR_UNSUPPORTED: too many classes).  Launches nothing.
 * ------------------------------------------------------------------------------------------ */
int segclip_seg_confusion(const uint8_t* pred, const uint8_t* gt, int64_t n, int64_t C, int ignore_index, int reduce_zero_label,
                          int64_t* conf, void* stream);
int segclip_seg_confusion_wide(const uint16_t* pred, const uint16_t* gt, int64_t n, int64_t C, int ignore_index,
                               int reduce_zero_label, int64_t* conf, void* stream);
int segclip_seg_confusion_route(int64_t C, int wide);

/* ------------------------------------------------------------------------------------------
 * Per-image areas of label maps (segment_image_areas.inc): the (3, C) areas of segclip_seg_areas for every picture of a list
 * on its own, in one launch - what mmseg's pre_eval hands back per image.  The worst pictures of an evaluation, the
 * fine-grained mIoU figures (the mean of per-image mIoU, the per-class mean over the pictures that contain the class, their
 * worst-case variants) and a bootstrap interval over pictures are reductions of these rows.
 *
 * segclip_seg_image_areas: B pictures of uint8 label maps in two flat buffers.
 *   images   : (B, SEGCLIP_SEG_IA_COLS) int64 rows on the device: 0 the offset of the picture's prediction in `pred`, in
 *              elements  1 the offset of its ground truth in `gt`  2 its pixel count n  3 its first workgroup = the sum of
 *              ceil(n / SEGCLIP_SEG_IA_TILE) over the pictures before it
 *   n_blocks : that sum over all pictures, the grid
 *   pred, gt : flat uint8 of pred_elems / gt_elems elements, read only.  They have offsets of their own because an evaluator's
 *              label buffer has gaps between its maps (the label kernels start every map at a multiple of 4) and its ground
 *              truths lie gapless; a picture may start at any element of either.
 *   out      : a contiguous (B, 3, C) int64 tensor that is ADDED to.  Row i is, value for value, what segclip_seg_areas adds
 *              for picture i alone: the same ground-truth rule pixel for pixel (a pixel with g == ignore_index contributes
 *              nothing; with reduce_zero_label a pixel with g == 0 contributes nothing either and every other g counts as
 *              g - 1; a value >= C on one side counts in the other side's area only) - the kernel counts with that entry's
 *              own device functions.  The sum of the rows is segclip_seg_areas of all the pictures.
 *   How.  256 threads; a workgroup owns one tile of SEGCLIP_SEG_IA_TILE consecutive pixels of one picture, which lane 0 finds
 *   by a binary search over column 3.  A lane reads 16 bytes of pred and of gt per step (element alignment suffices), two
 *   steps in flight; the fewer than 16 elements after a tile's last whole vector are read one by one.  Equal consecutive
 *   (g, p) pairs of a lane are counted once, a constant vector in one comparison.  3 x C 32-bit counters per workgroup in LDS
 *   (a tile is far below 2^31 pixels: none overflows), one 64-bit integer atomic per non-zero counter into the picture's
 *   row: the sums depend on no schedule.  Bound: HBM reads, 2 bytes per pixel (4 for the wide entry).
 *   Measured: profiles/seg_per_image.txt.
 *   Every table row is range-checked on the device.  A row passes when its offsets are >= 0, offset + n stays within
 *   pred_elems / gt_elems, 1 <= n < 2^31, and its workgroups lie within [0, n_blocks) and do not begin before those of the
 *   row before it end; a workgroup whose search ends on a row that does not pass or does not hold it looks through all rows
 *   for the first passing row that does.  A picture whose row does not pass is SKIPPED: nothing of it is read, and its row of
 *   `out` stays as it was.  With one row whose offsets or count are refused, or whose first workgroup lies too far back, the
 *   other pictures are counted exactly; a first workgroup that lies too far forward also fails the row after it.
 *   B == 0 or n_blocks == 0: success, nothing launched.  SEGCLIP_ERR_UNSUPPORTED (no launch): C < 1, C > 256.
 *   SEGCLIP_ERR_INVALID: negative sizes, B or n_blocks of 2^31 or more, missing pointers.
 *
 * segclip_seg_image_areas_wide: the same for uint16 elements (an int16 tensor is read as unsigned); g is compared with
 *   ignore_index as an UNSIGNED 16-bit value.  SEGCLIP_ERR_UNSUPPORTED: C < 1, C > SEGCLIP_SEG_WIDE_MAX_CLASSES.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_SEG_IA_COLS 4     /* int64 columns of one row of the image table */
#define SEGCLIP_SEG_IA_TILE 8192  /* pixels of one workgroup */
int segclip_seg_image_areas(const uint8_t* pred, int64_t pred_elems, const uint8_t* gt, int64_t gt_elems, const int64_t* images,
                            int64_t B, int64_t n_blocks, int64_t C, int ignore_index, int reduce_zero_label, int64_t* out,
                            void* stream);
int segclip_seg_image_areas_wide(const uint16_t* pred, int64_t pred_elems, const uint16_t* gt, int64_t gt_elems,
                                 const int64_t* images, int64_t B, int64_t n_blocks, int64_t C, int ignore_index,
                                 int reduce_zero_label, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image-text retrieval evaluation (retrieval.hip): Recall@K, median and mean rank in both directions from the contrastive
 * embeddings, without the (Nt, Ni) similarity matrix.  The reference trains "SegCLIP on Retrieval Task": its model carries
 * get_similarity_logits / _loose_similarity for it (modules/modeling.py:338-372) and its COCO loader builds the
 * multi-caption layout (sentences_dict, cut_off_points, sentence_num, image_num, multi_sentence_per_image;
 * dataloaders/dataloader_coco_retrieval.py:85-104); it ships no evaluator, so the definition is this project's:
 *   V (Ni, E), T (Nt, E) fp32, contiguous, 16-byte aligned;  g (Nt) int32, the image of every caption (any number of
 *   captions per image, zero included);  sim[t, j] = <T[t], V[j]> (the logit scale is a positive factor and left out)
 *   rank_t2i[t] = #{ j != g[t] : sim[t, j] > sim[t, g[t]] }                      (0-based; a tie favours the ground truth)
 *   rank_i2t[j] = #{ t : g[t] != j and sim[t, j] > best[j] },  best[j] = max{ sim[t, j] : g[t] == j };  -1 without captions
 *
 * segclip_retrieval_thresholds (modules/modeling.py:338-372 restricted to the ground-truth pairs): thr_t[t] = sim[t, g[t]] as
 *   the k-ordered fp32 fused-multiply-add chain the matrix cores form; n_cap[j] = the captions of image j; best[j] = the
 *   maximum of thr_t over them, an integer atomic maximum on an order-preserving key (no float atomics), +inf where
 *   n_cap[j] = 0.  A g[t] outside [0, Ni) is found on the device: SEGCLIP_RETRIEVAL_BAD_INDEX of *status is set (status is OR-ed into, never
 *   cleared here), thr_t[t] = +inf, and the caption counts for no image.  thr_t (Nt), best (Ni) fp32, n_cap (Ni) int32 are
 *   written whole.
 * segclip_retrieval_count (modules/modeling.py:356-357, the logits product, and the ranking a consumer of
 *   dataloaders/dataloader_coco_retrieval.py:85-104 forms from it): tiles of 128 captions x 128 images on
 *   v_mfma_f32_32x32x2_f32 (fp32 operands and accumulation), K in slices of 32 through LDS.  No similarity is stored: a lane
 *   compares its accumulators with its rows' thr_t and its columns' best, skipping j == g[t]; a tile sums the hits per row
 *   and column in registers and LDS and ADDS them to rank_t2i (Nt) and rank_i2t (Ni), int32, with one integer atomic per row
 *   and column that has hits.  The caller zeroes both before the call.  Integer sums: independent of scheduling.
 * segclip_retrieval_hist (the rank layout of dataloaders/dataloader_coco_retrieval.py:85-104 turned into the metrics' input):
 *   ADDS every rank_t2i to hist_t2i (Ni) and every rank_i2t of an image with captions to hist_i2t (Nt + 1), int64; sets
 *   rank_i2t[j] = -1 where n_cap[j] = 0.  R@K, median and mean rank follow from the histograms exactly.
 * SEGCLIP_ERR_UNSUPPORTED, naming the argument: E not a multiple of 32 or above 1024; Ni or Nt >= 2^24.
 * Bound of the count pass: 2 Nt Ni E flop at the f32-MFMA rate (256 flop / clock / CU).
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_RETRIEVAL_BAD_INDEX 1 /* status bit: an image index outside [0, Ni) */
int segclip_retrieval_thresholds(const float* V, const float* T, const int32_t* g, int64_t Ni, int64_t Nt, int64_t E, float* thr_t,
                                 float* best, int32_t* n_cap, int32_t* status, void* stream);
int segclip_retrieval_count(const float* V, const float* T, const int32_t* g, const float* thr_t, const float* best, int64_t Ni,
                            int64_t Nt, int64_t E, int32_t* rank_t2i, int32_t* rank_i2t, void* stream);
int segclip_retrieval_hist(const int32_t* rank_t2i, int32_t* rank_i2t, const int32_t* n_cap, int64_t Ni, int64_t Nt,
                           int64_t* hist_t2i, int64_t* hist_i2t, void* stream);

/* ------------------------------------------------------------------------------------------
 * Top-K image-text search (retrieval_topk.inc): what was retrieved, again without the similarity matrix.  Both entries
 * consume the similarity of modules/modeling.py:338-372 (get_similarity_logits / _loose_similarity, the logit scale left out).
 * The definition is this project's (tests/retrieval_topk_reference.py restates it in fp64):
 *   Q (Nq, E) queries, X (Nx, E) gallery, fp32, contiguous, 16-byte aligned;  s[q, j] = <Q[q], X[j]>
 *   Row q of idx (Nq, k) int32 holds the first min(k, Nx) gallery indices under the total order "higher score first, equal
 *   scores: lower index first"; val (Nq, k) fp32 holds their scores.  Positions from min(k, Nx) on hold idx = -1, val = -inf.
 *   The order is total, so the result is a function of the inputs alone: never of scheduling, tile order or the number of
 *   partial lists.  val[q, p] is bit for bit the k-ordered fp32 fused-multiply-add chain from 0 that
 *   segclip_retrieval_thresholds and the matrix cores of segclip_retrieval_count form for that pair: the search and the ranks
 *   agree exactly.  "Equal scores" means equal fp32 bits, compared through the order-preserving integer key of the segment
 *   maximum (sign-magnitude bits mapped onto unsigned integers): -0 sorts below +0, and a NaN sorts where its bits put it,
 *   above +inf with the sign bit clear and below -inf with it set.
 * segclip_retrieval_topk (modules/modeling.py:338-372, the logits product, and the selection a consumer forms from it): the
 *   128 x 128 x 32 product of segclip_retrieval_count on v_mfma_f32_32x32x2_f32 with a selecting epilogue.  A workgroup keeps
 *   128 queries and, per query, a sorted list of 64-bit keys (score key << 32 | 0xFFFFFFFF - index) in LDS; the k-th key is
 *   the row's admission threshold.  After a tile the scores pass through LDS, a wave takes a row at a time with one candidate
 *   per lane, one ballot against the threshold skips the row, and otherwise a bitonic sort and merge in lane exchanges
 *   updates the list.  The gallery tiles are dealt to `splits` partial lists per query (0 = auto: enough to fill the CUs when
 *   the queries alone do not, at most 64, never more than there are tiles); with more than one, the lists go through the
 *   workspace, (Nq rounded up to 128) * splits * k * 8 bytes, and a second kernel merges them.  splits is part of the ABI so
 *   that a test can hold every partition count to one result; nothing else passes a non-zero value.
 * segclip_retrieval_topk_ws_bytes (modules/modeling.py:338-372, sized for the same consumer): the workspace of that call, 0
 *   with one partial list; a negative error code where segclip_retrieval_topk would refuse the same arguments.
 * Nq = 0 or Nx = 0 is a successful call; the second fills idx and val with the padding.  idx and val are written whole.
 * SEGCLIP_ERR_UNSUPPORTED, naming the value: k outside [1, 64]; E not a multiple of 32 or above 1024; Nq or Nx >= 2^24; Q or X
 * not 16-byte aligned.  SEGCLIP_ERR_INVALID: a workspace smaller than segclip_retrieval_topk_ws_bytes says (nothing is launched).
 * Bound: 2 Nq Nx E flop at the f32-MFMA rate, as the count pass; the selection adds, per row and tile, two LDS reads and a
 * ballot where nothing is admitted and ~30 lane-exchange stages where something is.
 * ------------------------------------------------------------------------------------------ */
int64_t segclip_retrieval_topk_ws_bytes(int64_t Nq, int64_t Nx, int64_t k, int64_t splits);
int segclip_retrieval_topk(const float* Q, const float* X, int64_t Nq, int64_t Nx, int64_t E, int64_t k, int64_t splits, int32_t* idx,
                           float* val, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Front end of training (train_frontend.inc): decoded uint8 images and int32 segment maps -> the model's `image` and
 * `image_seg`, each in ONE launch for a batch of mixed sizes.  Both entries are integer algorithms and reproduce the
 * reference's CPU pipeline to the last bit.
 *
 * segclip_train_images_from_u8: RawImageExtractor's transforms (dataloaders/rawimage_util.py:40-52: RandomResizedCropCoord
 * with Image.BICUBIC :45, :347-361, or Resize + CenterCrop :47; ToTensor and Normalize :49) = Pillow's 8-bit BICUBIC resize of
 * a crop, a window of the result, a value table.
 *   images : (B, SEGCLIP_TRAIN_SOURCE_COLS) int64 rows on the device: 0 address of the source (uint8, HWC, 3 interleaved channels)  1 h  2 w
 *            3 row stride in bytes (>= 3 w)  4 x0  5 y0  6 bw  7 bh, the crop box inside the source - the filter sees the box
 *            as the whole image (crop() then resize(), NOT resize(box=...))  8 RW  9 RH, the size the box is resized to
 *            10 ox  11 oy, the offset of the (out_h, out_w) output window inside (RH, RW)  12 flags: bit 0 = horizontal,
 *            bit 1 = vertical flip of the window
 *   lut    : (256, 3) fp32 on the device; out[b, c, y, x] = lut[byte][c]: no floating-point arithmetic touches a pixel
 *   out    : (B, 3, out_h, out_w) fp32, contiguous
 * Per axis with in = crop side and out = RW or RH, in fp64 without contraction (Pillow's precompute_coeffs):
 * scale = in / out, fs = max(scale, 1), support = 2 fs, center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0),
 * xmax = min((int)(center + support + 0.5), in), weights bicubic((x + xmin - center + 0.5) * (1 / fs)) with a = -0.5, summed in
 * index order, each divided by the sum, each rounded to (int)(w * 2^22 +- 0.5) with the sign of w.  A pass is
 * clamp((2^21 + sum byte * k) >> 22, 0, 255) in int32; the horizontal pass runs first and is rounded to bytes.
 *   Every row is range-checked on the device.  An image is ZERO-FILLED when its row has a null address, a stride below 3 w,
 *   one of h, w, RW, RH outside [1, 2^15), a box not inside (h, w), a window not inside (RH, RW), bw or bh above
 *   SEGCLIP_TRAIN_MAX_SCALE times RW or RH (at most 33 taps), or flags outside 0..3; the other images are unaffected.  Nothing is read outside the box.
 *   16-byte stores when out_w % 4 == 0 and out is 16-byte aligned, scalar stores otherwise.  Design bound: the crop bytes
 *   read once + 12 bytes written per output pixel.  SEGCLIP_ERR_UNSUPPORTED: out_w > SEGCLIP_TRAIN_MAX_OUT_W.  out_h < 2^15, B <= 2^24.
 *
 * segclip_train_patch_labels: get_felzenszwalb_from_cache (dataloaders/rawimage_util.py:100-144) given the integer box of
 * :119-120, which the host computes.
 *   maps   : (B, SEGCLIP_TRAIN_MAP_COLS) int64 rows on the device: 0 address of the map (int32, (h, w), 4-byte aligned)  1 h  2 w  3 row stride in
 *            bytes (>= 4 w, a multiple of 4)  4 x0  5 y0  6 x1  7 y1, the box; x1 - x0 < 2 or y1 - y0 < 2 takes the whole
 *            map (:122)  8 flags: bit 0 = horizontal, bit 1 = vertical flip of the cropped map (:127-128)
 *   out    : (B, 1, size / patch, size / patch) int64
 * The crop is resampled to size x size with ATen's nearest index min((int64) floorf(d * ((float) in / size)), in - 1), product
 * and quotient in fp32 (:132); every patch x patch tile gives sum >> log2(patch^2), or a 64-bit division where patch^2 is no
 * power of two, the sum taken in 64 bits (:136-139, np.mean(...).astype(long) for labels in [0, 2^31)).
 *   A row with a null or unaligned address, a stride below 4 w, h or w outside [1, 2^15), a box outside the map, flags outside
 *   0..3, or a NEGATIVE label among the pixels read gives -1 in all its entries; the other rows are unaffected.
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_TRAIN_SOURCE_COLS 13 /* int64 columns of one row of the source table */
#define SEGCLIP_TRAIN_MAP_COLS 9     /* int64 columns of one row of the map table */
#define SEGCLIP_TRAIN_MAX_SCALE 8    /* crop side / resized side, per axis */
#define SEGCLIP_TRAIN_MAX_OUT_W 256  /* columns of the output window */
int segclip_train_images_from_u8(const int64_t* images, int64_t B, int64_t out_h, int64_t out_w, const float* lut, float* out,
                                 void* stream);
int segclip_train_patch_labels(const int64_t* maps, int64_t B, int64_t size, int64_t patch, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * MAE random masking (integer path, bit-exact given the noise).  modules/module_clip_util.py:91-124
 * with keep_cls: noise[:,0] = -1; ids_shuffle = argsort(noise) (stable); ids_restore =
 * argsort(ids_shuffle); mask = 1 except the first len_keep of the shuffle.
 * ------------------------------------------------------------------------------------------ */
int segclip_mask_sort(const float* noise, int64_t* ids_shuffle, int64_t* ids_restore, float* mask,
                      int64_t B, int64_t L, int64_t len_keep, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-step tail with no host synchronisation:
 *   torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad)      main_task_align.py:326
 *   AdaptAdamW.step()                                                   modules/optimization_adamw.py:111-174
 *   "skip the loss with NAN manually"                                   main_task_align.py:331-339
 *   torch.clamp_(logit_scale, max=ln 100), total_loss += float(loss)    main_task_align.py:323, 343-347
 * All tensors fp32 (the master copy); `shadow_bf16`, when non-NULL, receives the bf16 rounding of
 * the updated parameter (the compute-dtype copy the next forward's GEMMs read).
 *
 * One segclip_train_ctrl lives in device memory, zeroed once by the caller.  A NaN loss makes
 * segclip_adamw_step leave param/exp_avg/exp_avg_sq untouched and segclip_train_step_finish count
 * the skip; the bias corrections and the schedule use  step = tensor.step - ctrl->nan_skips, i.e.
 * exactly the reference's state['step'] (which is not advanced on skipped iterations).
 * ------------------------------------------------------------------------------------------ */
enum { SEGCLIP_SCHED_WARMUP_COSINE = 0, SEGCLIP_SCHED_WARMUP_CONSTANT = 1, SEGCLIP_SCHED_WARMUP_LINEAR = 2 };

typedef struct segclip_train_ctrl {
  float grad_sqnorm; /* sum of squares of all gradients (segclip_grad_sqnorm) */
  float clip_coef;   /* min(1, max_norm / (sqrt(grad_sqnorm) + 1e-6)) */
  int32_t nan_skips; /* iterations skipped so far because the loss was NaN */
  int32_t steps;     /* iterations finished (skipped ones included) */
  float loss_sum;    /* running sum of the non-NaN losses (train_epoch's total_loss) */
  float last_loss;
  int32_t reserved[2];
} segclip_train_ctrl;

typedef struct segclip_adamw_group { /* one torch param_group: optimization_adamw.py:70-73 */
  double lr, weight_decay, b1, b2, eps, warmup, lr_start, lr_end;
  int64_t t_total;  /* -1: constant lr */
  int32_t schedule; /* SEGCLIP_SCHED_* */
  int32_t reserved;
} segclip_adamw_group;

typedef struct segclip_adamw_tensor {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  void* shadow_bf16; /* nullable */
  int64_t n;
  int32_t step;  /* host-side count of steps (this one included) in which this tensor had a grad */
  int32_t group; /* index into groups[] */
} segclip_adamw_tensor;

/* Grouped 64-channel linear layers on channel-last rows = nn.Conv1d(D, D, kernel_size 1, groups = D/64, bias=False), the
 * k_conv / v_conv of the learnable-center stage (reference modules/module_seg_vit.py:266,269 applied at :299,302):
 *   out_o(m, g*64 + n) = sum_i sum_k in_i(m, g*64 + k) * w[i*n_out + o][g*64 + n][k],   bf16 in / out, fp32 accumulation.
 * (n_in, n_out) = (1, 1), (1, 2): one or two convolutions of the same input in one pass; (2, 1): sum of two - their data
 * gradient when w holds the per-group TRANSPOSED weights.  in/out/w and the pitches are HOST arrays; w[.]: (groups*64, 64)
 * bf16 row-major; all pointers 16-byte aligned, pitches multiples of 8 elements and at least groups*64 (columns of a row beyond
 * groups*64 are neither read nor written); any M >= 0 and groups >= 1.  A violation is an ERROR (-1), nothing is launched. */
int segclip_group_linear64(const void* const* in, const int64_t* ld_in, int n_in, void* const* out, const int64_t* ld_out,
                           int n_out, const void* const* w, int64_t M, int groups, void* stream);

/* ---- pooled-feature head and contrastive loss (csrc/head.hip) ------------------------------------------------------
 * out[b][d] = max_t x[b][t][d], idx = first arg-max token (torch.max(x, dim=1), reference modules/module_seg_vit.py:441);
 * backward: dx[b][t][d] = dout[b][d] if t == idx[b][d] else 0, written as fp32 (dx, nullable) and / or bf16 (dx_bf16). */
int segclip_max_tokens_fwd(const float* x, float* out, int32_t* idx, int64_t B, int64_t T, int64_t D, void* stream);
int segclip_max_tokens_bwd(const float* dout, const int32_t* idx, float* dx, void* dx_bf16, int64_t B, int64_t T, int64_t D,
                           void* stream);
/* both[b][0] = v[b] / |v[b]|, both[b][1] = t[b] / |t[b]| (B, 2, C) - the stacked message of the embedding all-gather
 * (reference modules/modeling.py:341-345,352-354); norms (2B).  Backward: dv, dt from dboth (+ dboth2, nullable). */
int segclip_l2norm_pair_fwd(const float* v, const float* t, float* both, float* norms, int64_t B, int64_t C, void* stream);
int segclip_l2norm_pair_bwd(const float* dboth, const float* dboth2, const float* both, const float* norms, float* dv,
                            float* dt, int64_t B, int64_t C, void* stream);
/* cos (2, B, N) raw cosines ([0] = t v_all^T, [1] = v t_all^T); logits = min(exp(*logit_scale), 100) * cos; row r of either
 * matrix has label r + label_offset; *loss = mean of the 2B row losses = (CE(t2v) + CE(v2t)) / 2 (reference
 * modules/modeling.py:204-209,346-362).  Backward: dcos = (*g / 2B) * scale * (softmax - onehot); *dlogit_scale (nullable)
 * = d loss / d logit_scale through the clamp.  lse, loss_rows, ds_rows: (2B) workspaces / saved statistics. */
int segclip_clip_ce_fwd(const float* cos, const float* logit_scale, float* lse, float* loss_rows, float* loss, int64_t B,
                        int64_t N, int64_t label_offset, void* stream);
int segclip_clip_ce_bwd(const float* cos, const float* lse, const float* logit_scale, const float* g, float* dcos,
                        float* ds_rows, float* dlogit_scale, int64_t B, int64_t N, int64_t label_offset, void* stream);

/* Segment mean of the learnable-center stage (reference modules/module_seg_vit.py:308-309):
 *   out[b][g][:] = (sum_t [idx[b][t] == g] v[b][t][:]) / max(counts[b][g], 1)       (hard assignment = one-hot of idx)
 * and its backward: dv[b][t][:] = dN[b][idx[b][t]][:], dhard[b][g][t] = dN[b][g] . v[b][t] + dc[b][g] with dN = dout / max(count, 1),
 * dc = -[count >= 1] (dout[b][g] . out[b][g]) / max(count, 1).  idx (B,T) uint8, counts (B,G) fp32 as segclip_assign_fwd leaves
 * them; v / dv (B,T,D) fp32 or bf16; out, dout (B,G,D) and dhard (B,G,T) fp32.
 * Limits.  Forward: G <= 8, D a multiple of 4, T >= 1; any T.  Backward: the same and D <= 1024 and (T + 1) * 32 <= 60000 bytes
 * of LDS, i.e. T <= 1874.  Either reports a violation as an ERROR (-1), not as SEGCLIP_ERR_UNSUPPORTED, and launches nothing:
 * the caller must choose another path before the forward whenever the backward will be needed. */
int segclip_segmean_fwd(const uint8_t* idx, const void* v, int v_dtype, const float* counts, float* out, int64_t B, int64_t G,
                        int64_t T, int64_t D, void* stream);
int segclip_segmean_bwd(const float* dout, const float* out, const uint8_t* idx, const void* v, int v_dtype, const float* counts,
                        void* dv, float* dhard, int64_t B, int64_t G, int64_t T, int64_t D, void* stream);

/* Token rows from the centers (MAE branch, reference modules/module_seg_vit.py:338-342): out (B,M,D) = a (B,M,G) @ x (B,G,D), fp32,
 * and the backward da (B,M,G) = dout x^T, dx (B,G,D) = a^T dout.
 * Limits, the same both ways: G = 8, D a multiple of 4, 4 <= D <= 4096 (the backward runs one lane per 4 columns in one
 * workgroup of at most 1024 threads); any M.  Other shapes return SEGCLIP_ERR_UNSUPPORTED (use segclip_gemm). */
int segclip_recon_mix_fwd(const float* a, const float* x, float* out, int64_t B, int64_t M, int64_t G, int64_t D, void* stream);
int segclip_recon_mix_bwd(const float* a, const float* x, const float* dout, float* da, float* dx, int64_t B, int64_t M, int64_t G,
                          int64_t D, void* stream);

/* Assignment logits of the center stage: attn[b][g][t] = q[b][g][:] . k[b][t][:] (fp32, un-scaled; reference
 * modules/module_seg_vit.py:304) and the backward dq = dl k, dk = dl^T q.  Not the summation order of the exact-fp32 GEMM.
 * Limits.  Both: G = 8, D = 768 | 1024.  Forward: T * 32 <= 60000 bytes of LDS, i.e. T <= 1875.  Backward: (8 T + 8 D) * 4 <=
 * 64000 bytes of LDS, i.e. T <= 1232 at D = 768 and T <= 976 at D = 1024 - LOWER than the forward's: a caller that will need the
 * backward must test the backward's limit before it takes this forward (ops.center_logits_covers).  Other shapes return
 * SEGCLIP_ERR_UNSUPPORTED (use segclip_gemm) and launch nothing. */
int segclip_center_logits_fwd(const float* q, const float* k, float* attn, int64_t B, int64_t G, int64_t T, int64_t D, void* stream);
int segclip_center_logits_bwd(const float* dl, const float* q, const float* k, float* dq, float* dk, int64_t B, int64_t G,
                              int64_t T, int64_t D, void* stream);

/* dst[i][:] = bf16(src[i][:]) for `count` fp32 tensors in ceil(count/32) launches (the compute-dtype copies of the
 * GEMM weights, refreshed once per forward instead of one cast launch per weight).  src/dst/n are HOST arrays. */
int segclip_multi_cast_bf16(const float* const* src, void* const* dst, const int64_t* n, int64_t count, void* stream);

/* dst[i][:] += src[i][:] for `count` fp32 tensor pairs in ceil(count/32) launches: a parameter used by two passes of one
 * step (the vision tower runs on the clean and on the masked image when the MAE loss is on, reference modules/modeling.py:
 * 196,237-249) receives two gradients; autograd would add them with one launch per parameter.  dst/src/n are HOST arrays. */
int segclip_multi_add_f32(float* const* dst, const float* const* src, const int64_t* n, int64_t count, void* stream);

/* number of fp32 partial sums segclip_grad_sqnorm needs in `ws` for these tensor sizes */
size_t segclip_grad_sqnorm_ws_bytes(const int64_t* n, int64_t count);
/* ctrl->grad_sqnorm = sum_i |grads[i]|^2 (deterministic two-level reduction), ctrl->clip_coef as above
 * (max_norm <= 0: coef = 1).  grads/n are HOST arrays of device pointers / element counts. */
int segclip_grad_sqnorm(const float* const* grads, const int64_t* n, int64_t count, float* ws,
                        segclip_train_ctrl* ctrl, float max_norm, void* stream);
/* fused multi-tensor AdaptAdamW step.  tensors/groups are HOST arrays (passed to the kernels by
 * value, 32 tensors per launch).  g = grad * ctrl->clip_coef; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g g;
 * denom = sqrt(v)/sqrt(1-b2^step) + eps; p = p (1 - lr_t wd) - (lr_t/(1-b1^step)) m/denom, where
 * lr_t = lr * schedule(step/t_total).  ctrl may be NULL (coef 1, no NaN logic, step = tensor.step);
 * loss may be NULL.  zero_grads != 0 also clears every grad (even on a skipped iteration). */
int segclip_adamw_step(const segclip_adamw_tensor* tensors, int64_t count, const segclip_adamw_group* groups,
                       int64_t ngroups, const segclip_train_ctrl* ctrl, const float* loss, int zero_grads,
                       void* stream);
/* bookkeeping after the step: ctrl->nan_skips += isnan(*loss); ctrl->steps++; loss_sum/last_loss;
 * *logit_scale = min(*logit_scale, clamp_max) when logit_scale != NULL. */
int segclip_train_step_finish(segclip_train_ctrl* ctrl, const float* loss, float* logit_scale, float clamp_max,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * Grouped weight gradients (bf16 operands, fp32 results):  dw_i (M_i, N_i) = dy_i^T x_i  for n problems over the SAME R token
 * rows, as ONE launch.  The four nn.Linear weight gradients of a residual block (modules/module_seg_vit.py:162-196: in_proj,
 * out_proj, c_fc, c_proj; the text blocks of modules/module_clip_ttransformer.py:20-37) have 9-36 output tiles each: launched
 * one by one, each needs 7-28 K ranges to fill the 256 CUs and leaves 64 MB of fp32 partial tiles to be combined; the gradients
 * of several consecutive blocks together fill the chip with 1-4 K ranges.
 *   segclip_wgrad_group_splits(tiles, ksteps): the K-range count the library recommends for a group with `tiles` 256x256
 *       output tiles in total over ksteps = R / 64 steps.
 *   splits == 1: results go to dw_i (row pitch ld_dw).  splits > 1: K range s of problem i is left, raw, at
 *       ws + (sum_{j<i} splits*M_j*N_j + s*M_i*N_i) floats; the caller sums the ranges in order (segclip_reduce_multi, kind 0).
 *   Not covered (SEGCLIP_ERR_UNSUPPORTED, nothing launched): M_i or N_i not multiples of 256, R not a multiple of 64, operands
 *       off 16-byte boundaries, leading dimensions not multiples of 8, n > 48.
 * ------------------------------------------------------------------------------------------ */
typedef struct segclip_wgrad_item {
  const void* dy;   /* (R, M) bf16, row pitch ld_dy */
  const void* x;    /* (R, N) bf16, row pitch ld_x  */
  float* dw;        /* (M, N) fp32, row pitch ld_dw (written when splits == 1) */
  int64_t M, N, ld_dy, ld_x, ld_dw;
} segclip_wgrad_item;
int segclip_wgrad_group_splits(int64_t tiles, int64_t ksteps);
/* the time model behind that choice (microseconds on MI355X, fitted to profiles/r04_wgrad_group.txt: rounds of 256 workgroups x (K loop + output) + the partial tiles
 * written and read back); callers use it to decide how many blocks to group */
double segclip_wgrad_group_model_us(int64_t tiles, int64_t ksteps, int splits);
size_t segclip_wgrad_group_ws_bytes(const segclip_wgrad_item* items, int n, int splits);
int segclip_wgrad_group(const segclip_wgrad_item* items, int n, int64_t R, int splits, void* ws, size_t ws_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Half-tile tail of the 256 x 256-tile bf16 GEMM (segclip_gemm with bf16 operands, M and N multiples of 256; the nn.Linear
 * products of modules/module_seg_vit.py:162-196).  A launch over `ntiles` output tiles whose last round of 256 workgroups is
 * at most half full (ntiles > 256, 0 < ntiles % 256 <= 128: out_proj / c_proj and the data gradients of in_proj / c_fc at
 * 256 x 197 token rows are 591 tiles) runs those tail tiles as twice as many 128 x 256 workgroups.  Results are bit-identical
 * to the full tiles'.  Returns the number of tail tiles run that way (0 = none).
 * The same half-tile workgroups cover a last row of 128 token rows: M = 256 q + 128 (128 samples x 197 / 577 / 77 tokens)
 * runs on this kernel as q rows of full tiles + N / 256 half-tiles.
 * ------------------------------------------------------------------------------------------ */
int segclip_gemm_pq_half_tail(int64_t ntiles);

/* ------------------------------------------------------------------------------------------
 * Test hook: which GEMM kernel instance the last segclip_gemm call on the calling thread launched (one host-side store per
 * launch; nothing on the GPU).  A call that launched nothing (an error, SEGCLIP_ERR_UNSUPPORTED, M or N = 0) leaves family
 * SEGCLIP_GEMM_ROUTE_NONE, and segclip_gemm_last_route then returns SEGCLIP_ERR_UNSUPPORTED (out is filled either way).
 *   a_ks / b_ks : the operand is k-strided (A(m,k) = A[k*sak + m], B(n,k) = B[k*sbk + n]) rather than k-contiguous
 *   tile_m/_n   : output tile of one workgroup;  splits: K splits (> 1: fp32 slabs in ws and a combine)
 *   variant     : GENERIC: bit 0 = fp32 A operand, bit 1 = 16-byte aligned (unguarded) operand loads
 *                 DMA    : 0 = 256 x 128 tiles, 1 = 256 x 256, 2 = 128 x 128
 *                 P8     : 0
 *                 PQ     : bits 0-3 the epilogue mode (0 plain, 1 + bf16 residual, 2 QuickGELU + derivative byte, 3 x derivative
 *                          byte, 4 fp32 partial tiles / weight gradient, 5 + fp32 residual -> fp32, 6 erf-GELU + derivative
 *                          byte), bits 4-15 the tail tiles run as half-tiles, bits 16-31 the half-tiles of a last row of
 *                          128 rows (M = 256 q + 128)
 *                 F32    : 0 = 32 x 128 tiles (M <= 32), 1 = 64 x 64, 2 = 128 x 128
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_GEMM_ROUTE_NONE 0
#define SEGCLIP_GEMM_ROUTE_GENERIC 1 /* register-staged 128 x 128 bf16 kernel (gemm_bf16.hip) */
#define SEGCLIP_GEMM_ROUTE_DMA 2     /* LDS-DMA bf16 kernel (gemm_bf16_dma.hip) */
#define SEGCLIP_GEMM_ROUTE_P8 3      /* phase-pipelined 256 x 256 bf16 kernel (gemm_bf16_p8.hip) */
#define SEGCLIP_GEMM_ROUTE_PQ 4      /* accumulator-register 256 x 256 bf16 kernel (gemm_bf16_pq.hip) */
#define SEGCLIP_GEMM_ROUTE_F32 5     /* exact-fp32 kernel (gemm_f32.hip) */
typedef struct segclip_gemm_route {
  int32_t family;
  int32_t a_ks, b_ks;
  int32_t tile_m, tile_n;
  int32_t splits;
  int32_t variant;
} segclip_gemm_route;
int segclip_gemm_last_route(segclip_gemm_route* out);
/* Test hook: the plan of segclip_gemm(d) without the launch - a pure function of the descriptor (its pointers, ws and colsum_ws
 * are read for presence and alignment, never dereferenced) and the tuning switches; runs on a machine without a GPU.  *out (nullable)
 * is the route segclip_gemm(d) would note, family NONE where it would launch nothing; *ws_bytes (nullable) is
 * segclip_gemm_ws_bytes(d) (0 for an empty problem, M or N = 0, and for a null descriptor or negative sizes).  Returns what segclip_gemm(d) would return before launching (0, SEGCLIP_ERR_INVALID,
 * SEGCLIP_ERR_UNSUPPORTED) and sets the same message. */
int segclip_gemm_plan(const segclip_gemm_desc* d, segclip_gemm_route* out, size_t* ws_bytes);

/* ------------------------------------------------------------------------------------------
 * Test hook: which attention kernel instance the last segclip_attn_fwd / segclip_attn_bwd call on the calling thread launched
 * (one host-side store per launch; nothing on the GPU).  Every call clears the record first, so after a forward bwd_kernel
 * is NONE and after a backward fwd_kernel is NONE.  A call that launched nothing (B or Tq = 0, an error, the refused
 * SEGCLIP_ATTN_FP8 flag) leaves both NONE, and segclip_attn_last_route then returns SEGCLIP_ERR_UNSUPPORTED (out is filled
 * either way).  The fp32 path records F32 here and its inner products through segclip_gemm_last_route.
 *   tiles   : 32-row tiles of the longer of Tq, Tk (PF / DQW: the template argument NT; GENERIC: query tiles)
 *   variant : PF      : bit 0 = the causal instance
 *             GENERIC : bit 0 = output rows staged through LDS, bits 8-15 = waves (query tiles) per workgroup
 *             DQW     : bit 0 = MULTI (key chunks of 224, fp32 dQ workspace)
 *             SP      : bit 0 = the masked instance (causal and / or klen)
 *             TWOPASS : bits 8-15 = waves per workgroup
 *             others  : 0
 * ------------------------------------------------------------------------------------------ */
#define SEGCLIP_ATTN_ROUTE_NONE 0
#define SEGCLIP_ATTN_ROUTE_SMALLQ 1  /* fwd, bwd: at most 8 queries, one wave per (batch, head) (attention_smallq.inc) */
#define SEGCLIP_ATTN_ROUTE_PF 2      /* fwd: persistent kernel with a loader wave, 3 / 6 / 7 tiles (attention_pf.inc) */
#define SEGCLIP_ATTN_ROUTE_GENERIC 3 /* fwd: attn_fwd_bf16_kernel, any Tq, Tk (attention.hip) */
#define SEGCLIP_ATTN_ROUTE_F32 4     /* fwd, bwd: fp32 GEMMs + row softmax kernels */
#define SEGCLIP_ATTN_ROUTE_DQW 5     /* bwd: query tiles as a stream with a dQ wave (attention_dqw.inc) */
#define SEGCLIP_ATTN_ROUTE_STREAM 6  /* bwd: dkv_stream + dq_stream, more than 256 tokens (attention_stream.inc) */
#define SEGCLIP_ATTN_ROUTE_SPL 7     /* bwd: single pass with a loader wave, 5-7 tiles, head_dim 64 (attention_spl.inc) */
#define SEGCLIP_ATTN_ROUTE_SP 8      /* bwd: single pass, one wave per key tile (attention_sp.inc) */
#define SEGCLIP_ATTN_ROUTE_TWOPASS 9 /* bwd: attn_bwd_bf16_kernel, Tq != Tk, both at most 256 (attention.hip) */
typedef struct segclip_attn_route {
  int32_t fwd_kernel;
  int32_t bwd_kernel;
  int32_t tiles;
  int32_t variant;
} segclip_attn_route;
int segclip_attn_last_route(segclip_attn_route* out);

#ifdef __cplusplus
}
#endif
#endif /* SEGCLIP_HIP_H */
