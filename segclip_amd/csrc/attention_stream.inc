// ------------------------------- backward for sequences longer than 256 tokens ----------------------------------
// (ViT-L/14 at 336^2: 576 patch tokens; SegCLIP eval at 448^2: 784.)  Included by attention.hip inside its anonymous
// namespace.  Same arithmetic as the fused backward kernel, as two launches that STREAM the operand a wave does not own
// through LDS in chunks of 256 rows:
//   dkv kernel: grid (B*H, key-tile groups); a wave owns one 32-key tile, Q / dO (+ lse, D) chunks pass through LDS.
//   dq  kernel: grid (B*H, query-tile groups); a wave owns one 32-query tile, K / V chunks pass through LDS.
// D[q] = sum_d dO*O and cs[key] = sum_q dS[q][key] (needed for the in_proj-bias token sums) go through a small fp32
// workspace (ws: [B*H][Tk] cs, then [B*H][Tq] D).  Deterministic, no atomics.
constexpr int SCHUNK = 256;

__global__ __launch_bounds__(512) void attn_bwd_dkv_stream_kernel(BwdArgs a, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem_bwd[];
  char* Qt = smem_bwd;
  char* Gt = smem_bwd + SCHUNK * ROWB;
  float* Ls = reinterpret_cast<float*>(smem_bwd + 2 * SCHUNK * ROWB);
  float* Ds = Ls + SCHUNK;
  float* Red = Ds + 2 * SCHUNK;  // [8 waves][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int li = lane & 31, lh = lane >> 5;
  const int64_t hoff = (int64_t)h * a.hd;
  const bf16_t* Qp = a.Q + b * a.q_sb + hoff;
  const bf16_t* Kp = a.K + b * a.k_sb + hoff;
  const bf16_t* Vp = a.V + b * a.v_sb + hoff;
  const bf16_t* Op = a.O + b * a.o_sb + hoff;
  const bf16_t* Gp = a.dO + b * a.do_sb + hoff;
  float* cs_ws = ws + (int64_t)bh * a.Tk;
  float* d_ws = ws + (int64_t)gridDim.x * a.Tk + (int64_t)bh * a.Tq;
  const int k0 = (blockIdx.y * nw + wave) * 32;
  const bool active = k0 < a.Tk;
  const bool first = blockIdx.y == 0;
  bf16x8_t kf[4], vf[4];
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
    kf[kc] = frag_rows_g(Kp, a.k_st, active ? k0 : 0, a.Tk, kc, lane, a.hd);
    vf[kc] = frag_rows_g(Vp, a.v_st, active ? k0 : 0, a.Tk, kc, lane, a.hd);
  }
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }
  const int key = k0 + li;
  float csl = 0.f;
  float accv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) accv[j] = 0.f;

  for (int c0 = 0; c0 < a.Tq; c0 += SCHUNK) {
    const int nq = a.Tq - c0 < SCHUNK ? a.Tq - c0 : SCHUNK;
    const int nqp = (nq + 31) & ~31;
    __syncthreads();
    stage_rows(Qt, Qp, a.q_st, c0, nq, nqp, a.hd, tid, blockDim.x);
    {
      const int total = nqp * 8;
      for (int base = 0; base < total; base += 2 * (int)blockDim.x) {
        u32x4 gv[2], ov[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const int idx = base + it * (int)blockDim.x + tid;
          const int r = idx >> 3, c = idx & 7;
          const int rc = c0 + (r < nq ? r : nq - 1);
          const int cc = c * 8 < a.hd ? c : 0;
          gv[it] = *reinterpret_cast<const u32x4*>(Gp + (int64_t)rc * a.do_st + cc * 8);
          ov[it] = *reinterpret_cast<const u32x4*>(Op + (int64_t)rc * a.o_st + cc * 8);
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const int idx = base + it * (int)blockDim.x + tid;
          const int r = idx >> 3, c = idx & 7;
          const bool ok = r < nq && c * 8 < a.hd;
          const u32x4 g = ok ? gv[it] : u32x4{0u, 0u, 0u, 0u};
          const u32x4 o4 = ok ? ov[it] : u32x4{0u, 0u, 0u, 0u};
          float sdot = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            sdot += __uint_as_float(g[j] << 16) * __uint_as_float(o4[j] << 16);
            sdot += __uint_as_float(g[j] & 0xffff0000u) * __uint_as_float(o4[j] & 0xffff0000u);
          }
          sdot += __shfl_xor(sdot, 1, 64); sdot += __shfl_xor(sdot, 2, 64); sdot += __shfl_xor(sdot, 4, 64);
          if (idx < total) {
            *reinterpret_cast<u32x4*>(Gt + swz(r, c * 8)) = g;
            if (c == 0) {
              Ds[r] = sdot;
              Ls[r] = r < nq ? a.lse[((int64_t)b * a.H + h) * a.Tq + c0 + r] : 0.f;
              if (first && r < nq) d_ws[c0 + r] = sdot;
            }
          }
        }
      }
    }
    __syncthreads();
    if (first && a.colsum_part) {  // token sums of dV = token sums of dO (the rows of P sum to one)
      const int c = tid & 7, nrl = (int)blockDim.x >> 3;
      for (int r = tid >> 3; r < nqp; r += nrl) {
        const u32x4 gv = *reinterpret_cast<const u32x4*>(Gt + swz(r, c * 8));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          accv[2 * j] += __uint_as_float(gv[j] << 16);
          accv[2 * j + 1] += __uint_as_float(gv[j] & 0xffff0000u);
        }
      }
    }
    if (!active) continue;
    for (int q0 = 0; q0 < nqp; q0 += 32) {
      if (a.causal && c0 + q0 + 31 < k0) continue;
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Qt, q0, kc, lane), kf[kc], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Gt, q0, kc, lane), vf[kc], dp, 0, 0, 0);
      }
      float p[16], ds[16];
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int qb = q0 + 8 * rg + 4 * lh;
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + qb);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(Ds + qb);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = rg * 4 + j, q = c0 + qb + j;
          const bool ok = key < a.Tk && q < a.Tq && (!a.causal || key <= q);
          const float pv = ok ? __expf(s[r] * a.scale - l4[j]) : 0.f;
          p[r] = pv;
          ds[r] = pv * (dp[r] - d4[j]) * a.scale;
          csl += ds[r];
        }
      }
      const bf16x8_t pb0 = pack8(p), pb1 = pack8(p + 8), sb0 = pack8(ds), sb1 = pack8(ds + 8);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Gt, q0, dt * 32, lane), pb0, dv[dt], 0, 0, 0);
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Gt, q0 + 16, dt * 32, lane), pb1, dv[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qt, q0, dt * 32, lane), sb0, dk[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qt, q0 + 16, dt * 32, lane), sb1, dk[dt], 0, 0, 0);
      }
    }
  }
  if (active) {
    store_acc_T(a.dK + b * a.dk_sb + hoff, a.dk_st, key, a.Tk, a.hd, dk, lh);
    store_acc_T(a.dV + b * a.dv_sb + hoff, a.dv_st, key, a.Tk, a.hd, dv, lh);
    csl += __shfl_xor(csl, 32, 64);
    if (lh == 0 && key < a.Tk) cs_ws[key] = csl;
  }
  if (first && a.colsum_part) {
    const int c = tid & 7;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float vv = accv[j];
      vv += __shfl_xor(vv, 8, 64); vv += __shfl_xor(vv, 16, 64); vv += __shfl_xor(vv, 32, 64);
      if (lane < 8) Red[wave * 64 + c * 8 + j] = vv;
    }
    __syncthreads();
    for (int t = tid; t < 64; t += (int)blockDim.x) {
      float v = 0.f;
      for (int w = 0; w < nw; ++w) v += Red[w * 64 + t];
      if (t < a.hd) {
        a.colsum_part[((int64_t)b * 3 + 2) * ((int64_t)a.H * a.hd) + hoff + t] = v;
        a.colsum_part[((int64_t)b * 3 + 1) * ((int64_t)a.H * a.hd) + hoff + t] = 0.f;  // sum_key dK = 0 exactly
      }
    }
  }
}

__global__ __launch_bounds__(512) void attn_bwd_dq_stream_kernel(BwdArgs a, const float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem_bwd[];
  char* Kt = smem_bwd;
  char* Vt = smem_bwd + SCHUNK * ROWB;
  float* Cs = reinterpret_cast<float*>(smem_bwd + 2 * SCHUNK * ROWB);
  float* Red = Cs + 3 * SCHUNK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int li = lane & 31, lh = lane >> 5;
  const int64_t hoff = (int64_t)h * a.hd;
  const bf16_t* Qp = a.Q + b * a.q_sb + hoff;
  const bf16_t* Kp = a.K + b * a.k_sb + hoff;
  const bf16_t* Vp = a.V + b * a.v_sb + hoff;
  const bf16_t* Gp = a.dO + b * a.do_sb + hoff;
  const float* cs_ws = ws + (int64_t)bh * a.Tk;
  const float* d_ws = ws + (int64_t)gridDim.x * a.Tk + (int64_t)bh * a.Tq;
  const int q0 = (blockIdx.y * nw + wave) * 32;
  const bool active = q0 < a.Tq;
  const bool first = blockIdx.y == 0;
  bf16x8_t qf[4], gf[4];
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
    qf[kc] = frag_rows_g(Qp, a.q_st, active ? q0 : 0, a.Tq, kc, lane, a.hd);
    gf[kc] = frag_rows_g(Gp, a.do_st, active ? q0 : 0, a.Tq, kc, lane, a.hd);
  }
  const int q = q0 + li;
  const int qc = q < a.Tq ? q : a.Tq - 1;
  const float lq = a.lse[((int64_t)b * a.H + h) * a.Tq + qc], dq_ = d_ws[qc];
  f32x16 dq[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
  float accq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) accq[j] = 0.f;

  for (int c0 = 0; c0 < a.Tk; c0 += SCHUNK) {
    const int nk = a.Tk - c0 < SCHUNK ? a.Tk - c0 : SCHUNK;
    const int nkp = (nk + 31) & ~31;
    __syncthreads();
    stage_rows(Kt, Kp, a.k_st, c0, nk, nkp, a.hd, tid, blockDim.x);
    stage_rows(Vt, Vp, a.v_st, c0, nk, nkp, a.hd, tid, blockDim.x);
    if (first && a.colsum_part)
      for (int r = tid; r < nkp; r += (int)blockDim.x) Cs[r] = r < nk ? cs_ws[c0 + r] : 0.f;
    __syncthreads();
    if (first && a.colsum_part) {  // sum_q dQ[q][d] = sum_key K[key][d] cs[key]
      const int c = tid & 7, nrl = (int)blockDim.x >> 3;
      for (int r = tid >> 3; r < nkp; r += nrl) {
        const u32x4 kv = *reinterpret_cast<const u32x4*>(Kt + swz(r, c * 8));
        const float w = Cs[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          accq[2 * j] += w * __uint_as_float(kv[j] << 16);
          accq[2 * j + 1] += w * __uint_as_float(kv[j] & 0xffff0000u);
        }
      }
    }
    if (!active) continue;
    for (int kk = 0; kk < nkp; kk += 32) {
      if (a.causal && c0 + kk > q0 + 31) break;
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Kt, kk, kc, lane), qf[kc], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Vt, kk, kc, lane), gf[kc], dp, 0, 0, 0);
      }
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = c0 + kk + acc_row(r, lh);
        const bool ok = key < a.Tk && q < a.Tq && (!a.causal || key <= q);
        const float pv = ok ? __expf(s[r] * a.scale - lq) : 0.f;
        ds[r] = pv * (dp[r] - dq_) * a.scale;
      }
      const bf16x8_t sb0 = pack8(ds), sb1 = pack8(ds + 8);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Kt, kk, dt * 32, lane), sb0, dq[dt], 0, 0, 0);
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Kt, kk + 16, dt * 32, lane), sb1, dq[dt], 0, 0, 0);
      }
    }
  }
  if (active) store_acc_T(a.dQ + b * a.dq_sb + hoff, a.dq_st, q, a.Tq, a.hd, dq, lh);
  if (first && a.colsum_part) {
    const int c = tid & 7;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float vq = accq[j];
      vq += __shfl_xor(vq, 8, 64); vq += __shfl_xor(vq, 16, 64); vq += __shfl_xor(vq, 32, 64);
      if (lane < 8) Red[wave * 64 + c * 8 + j] = vq;
    }
    __syncthreads();
    for (int t = tid; t < 64; t += (int)blockDim.x) {
      float v = 0.f;
      for (int w = 0; w < nw; ++w) v += Red[w * 64 + t];
      if (t < a.hd) a.colsum_part[((int64_t)b * 3 + 0) * ((int64_t)a.H * a.hd) + hoff + t] = v;
    }
  }
}
static inline size_t bwd_stream_lds_bytes() { return (size_t)SCHUNK * (2 * ROWB + 3 * 4) + 8 * 64 * 4; }
