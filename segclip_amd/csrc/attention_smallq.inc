// Attention with at most 8 queries per (batch, head) - the learnable-center cross-attention (8 centers against 8 + 196 keys,
// reference modules/module_seg_vit.py:199-218, twice per step) - bf16, head_dim 64, no mask.  Included by attention.hip.
//
// The flash kernels above pad the 8 queries to a 32-row MFMA tile and stage the keys of ONE (batch, head) through 64 KiB of
// LDS with one wave: two workgroups per CU, six rounds of a latency chain - 115 us forward / 196 us backward per launch for
// 0.2 GFLOP and 160 MB.  Here ONE WAVE owns a (batch, head) item and everything is VALU work in two lane mappings:
//   lanes over KEYS  (a lane reads whole 128-byte K / V rows of its keys):   S = Q K^T,  dP = dO V^T
//   lanes over the 64 head dims (a key's row is one coalesced 128-byte read): O = P V,  dV = P^T dO,  dK = dS^T Q,  dQ = dS K
// with Q / dO (fp32) and the probabilities in LDS ([key][8] floats: one 32-byte broadcast read per key).  Four items per
// workgroup, ~25 KiB of LDS each at 204 keys: many waves per CU hide the row latencies (K / V rows are 786 KB apart in the
// reference's "t18" layout).
namespace smallq {

constexpr int QMAX = 8, WPB_FWD = 4, WPB_BWD = 2;   // waves (= items) per workgroup: 34 KiB of LDS either way at 204 keys

// LDS per wave: Q (or dO) [8][64] fp32, a second [8][64] (backward), P [S][8] fp32, dS [S][8] fp32 (backward)
static inline size_t lds_bytes(int S, bool bwd) {
  return (size_t)(bwd ? WPB_BWD : WPB_FWD) * ((bwd ? 2 : 1) * QMAX * 64 + (bwd ? 2 : 1) * (size_t)S * QMAX) * sizeof(float);
}

__device__ __forceinline__ void unpack8f(const u32x4 v, float* f) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[2 * j] = __uint_as_float(v[j] << 16); f[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u); }
}
// 8 query rows x 64 dims of bf16 -> fp32 [8][64] in LDS: lane l loads chunk (l & 7) of row (l >> 3); rows >= nq are zero
__device__ __forceinline__ void stage_q(float* dst, const bf16_t* base, int64_t st, int nq, int lane) {
  const int r = lane >> 3, c = lane & 7;
  float f[8];
  if (r < nq) unpack8f(*reinterpret_cast<const u32x4*>(base + (int64_t)r * st + c * 8), f);
  else {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = 0.f;
  }
  *reinterpret_cast<f32x4*>(dst + r * 64 + c * 8) = f32x4{f[0], f[1], f[2], f[3]};
  *reinterpret_cast<f32x4*>(dst + r * 64 + c * 8 + 4) = f32x4{f[4], f[5], f[6], f[7]};
}
// dots of ONE 64-dim bf16 row (this lane's key) with the 8 fp32 rows in LDS, on register PAIRS (v_pk_fma_f32: two
// multiply-adds per instruction; the kernel is VALU work)
__device__ __forceinline__ void row_dots(const bf16_t* row, const float* qs, float (&s)[QMAX]) {
  v2f acc[QMAX];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) acc[q] = v2f{0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float kf[8];
    unpack8f(*reinterpret_cast<const u32x4*>(row + c * 8), kf);
    const v2f k0 = v2f{kf[0], kf[1]}, k1 = v2f{kf[2], kf[3]}, k2 = v2f{kf[4], kf[5]}, k3 = v2f{kf[6], kf[7]};
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(qs + q * 64 + c * 8), b = *reinterpret_cast<const f32x4*>(qs + q * 64 + c * 8 + 4);
      acc[q] += k0 * v2f{a[0], a[1]};
      acc[q] += k1 * v2f{a[2], a[3]};
      acc[q] += k2 * v2f{b[0], b[1]};
      acc[q] += k3 * v2f{b[2], b[3]};
    }
  }
#pragma unroll
  for (int q = 0; q < QMAX; ++q) s[q] = acc[q][0] + acc[q][1];
}

__global__ __launch_bounds__(WPB_FWD * 64) void attn_smallq_fwd_kernel(FwdArgs a, int nitems) {
  extern __shared__ float smq[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = blockIdx.x * WPB_FWD + wave;
  if (item >= nitems) return;
  const int b = item / a.H, h = item % a.H, S = a.Tk, nq = a.Tq;
  float* qs = smq + (size_t)wave * (QMAX * 64 + (size_t)S * QMAX);
  float* ps = qs + QMAX * 64;                                     // [S][8]
  const bf16_t* Qp = a.Q + (int64_t)b * a.q_sb + (int64_t)h * 64;
  const bf16_t* Kp = a.K + (int64_t)b * a.k_sb + (int64_t)h * 64;
  const bf16_t* Vp = a.V + (int64_t)b * a.v_sb + (int64_t)h * 64;
  stage_q(qs, Qp, a.q_st, nq, lane);
  __builtin_amdgcn_wave_barrier();
  // ---- S = scale * Q K^T, lanes over keys; running row maxima per lane
  float mx[QMAX];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) mx[q] = -INFINITY;
  for (int key = lane; key < S; key += 64) {
    float s[QMAX];
    row_dots(Kp + (int64_t)key * a.k_st, qs, s);
#pragma unroll
    for (int q = 0; q < QMAX; ++q) { s[q] *= a.scale; mx[q] = fmaxf(mx[q], s[q]); }
    *reinterpret_cast<f32x4*>(ps + (size_t)key * QMAX) = f32x4{s[0], s[1], s[2], s[3]};
    *reinterpret_cast<f32x4*>(ps + (size_t)key * QMAX + 4) = f32x4{s[4], s[5], s[6], s[7]};
  }
  float sum[QMAX];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) { mx[q] = wave_max(mx[q]); sum[q] = 0.f; }
  for (int key = lane; key < S; key += 64) {
    float* p = ps + (size_t)key * QMAX;
#pragma unroll
    for (int q = 0; q < QMAX; ++q) { const float e = __expf(p[q] - mx[q]); p[q] = e; sum[q] += e; }
  }
  float inv[QMAX];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) {
    sum[q] = wave_sum(sum[q]);
    inv[q] = 1.f / sum[q];
    if (lane == q && q < nq) a.lse[((int64_t)b * a.H + h) * nq + q] = mx[q] + __logf(sum[q]);
  }
  __builtin_amdgcn_wave_barrier();
  // ---- O = P V, lanes over the head dims: one coalesced 128-byte row per key
  v2f o2[QMAX / 2];
#pragma unroll
  for (int q = 0; q < QMAX / 2; ++q) o2[q] = v2f{0.f, 0.f};
  const bf16_t* vcol = Vp + lane;
  // (batches of 8 or 16 rows per round trip measured SLOWER here - 125 vs 74 us per layer - while the backward's loop gains)
  int key = 0;
#define SMQ_FWD_BATCH(U)                                                                                                  \
  for (; key + U <= S; key += U) {                                                                                        \
    float v[U];                                                                                                           \
    _Pragma("unroll") for (int u = 0; u < U; ++u) v[u] = bf2f(vcol[(int64_t)(key + u) * a.v_st]);                       \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                                                                      \
      const f32x4 p0 = *reinterpret_cast<const f32x4*>(ps + (size_t)(key + u) * QMAX),                                    \
                  p1 = *reinterpret_cast<const f32x4*>(ps + (size_t)(key + u) * QMAX + 4);                                \
      const v2f vv = v2f{v[u], v[u]};                                                                                     \
      o2[0] += v2f{p0[0], p0[1]} * vv; o2[1] += v2f{p0[2], p0[3]} * vv;                                                   \
      o2[2] += v2f{p1[0], p1[1]} * vv; o2[3] += v2f{p1[2], p1[3]} * vv;                                                   \
    }                                                                                                                     \
  }
  SMQ_FWD_BATCH(4)
#undef SMQ_FWD_BATCH
  for (; key < S; ++key) {
    const float v = bf2f(vcol[(int64_t)key * a.v_st]);
    const float* p = ps + (size_t)key * QMAX;
    const v2f vv = v2f{v, v};
#pragma unroll
    for (int q = 0; q < QMAX / 2; ++q) o2[q] += v2f{p[2 * q], p[2 * q + 1]} * vv;
  }
  bf16_t* Op = a.O + (int64_t)b * a.o_sb + (int64_t)h * 64 + lane;
#pragma unroll
  for (int q = 0; q < QMAX; ++q)
    if (q < nq) Op[(int64_t)q * a.o_st] = f2bf(o2[q >> 1][q & 1] * inv[q]);
}

__global__ __launch_bounds__(WPB_BWD * 64) void attn_smallq_bwd_kernel(BwdArgs a, int nitems) {
  extern __shared__ float smq[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = blockIdx.x * WPB_BWD + wave;
  if (item >= nitems) return;
  const int b = item / a.H, h = item % a.H, S = a.Tk, nq = a.Tq;
  float* qs = smq + (size_t)wave * (2 * QMAX * 64 + 2 * (size_t)S * QMAX);
  float* dos = qs + QMAX * 64;                                    // dO [8][64]
  float* ps = dos + QMAX * 64;                                    // P  [S][8]
  float* dss = ps + (size_t)S * QMAX;                             // dS [S][8] (scale folded in)
  const bf16_t* Qp = a.Q + (int64_t)b * a.q_sb + (int64_t)h * 64;
  const bf16_t* Kp = a.K + (int64_t)b * a.k_sb + (int64_t)h * 64;
  const bf16_t* Vp = a.V + (int64_t)b * a.v_sb + (int64_t)h * 64;
  const bf16_t* Op = a.O + (int64_t)b * a.o_sb + (int64_t)h * 64;
  const bf16_t* dOp = a.dO + (int64_t)b * a.do_sb + (int64_t)h * 64;
  stage_q(qs, Qp, a.q_st, nq, lane);
  stage_q(dos, dOp, a.do_st, nq, lane);
  // D[q] = dO[q] . O[q], lanes over dims
  float dd[QMAX], lse[QMAX];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) {
    const float ov = q < nq ? bf2f(Op[(int64_t)q * a.o_st + lane]) : 0.f, gv = q < nq ? bf2f(dOp[(int64_t)q * a.do_st + lane]) : 0.f;
    dd[q] = wave_sum(ov * gv);
    lse[q] = q < nq ? a.lse[((int64_t)b * a.H + h) * nq + q] : INFINITY;   // padded query rows: P = 0
  }
  __builtin_amdgcn_wave_barrier();
  // ---- lanes over keys: P = exp(scale S - lse), dP = dO V^T, dS = P (dP - D)
  for (int key = lane; key < S; key += 64) {
    float s[QMAX], dp[QMAX];
    row_dots(Kp + (int64_t)key * a.k_st, qs, s);
    row_dots(Vp + (int64_t)key * a.v_st, dos, dp);
    float p[QMAX], ds[QMAX];
#pragma unroll
    for (int q = 0; q < QMAX; ++q) { p[q] = __expf(s[q] * a.scale - lse[q]); ds[q] = p[q] * (dp[q] - dd[q]) * a.scale; }
    *reinterpret_cast<f32x4*>(ps + (size_t)key * QMAX) = f32x4{p[0], p[1], p[2], p[3]};
    *reinterpret_cast<f32x4*>(ps + (size_t)key * QMAX + 4) = f32x4{p[4], p[5], p[6], p[7]};
    *reinterpret_cast<f32x4*>(dss + (size_t)key * QMAX) = f32x4{ds[0], ds[1], ds[2], ds[3]};
    *reinterpret_cast<f32x4*>(dss + (size_t)key * QMAX + 4) = f32x4{ds[4], ds[5], ds[6], ds[7]};
  }
  __builtin_amdgcn_wave_barrier();
  // ---- lanes over dims: dV = P^T dO, dK = dS^T Q (rows written as they are produced), dQ = dS K
  float qd[QMAX], god[QMAX];
  v2f dq2[QMAX / 2], qd2[QMAX / 2], god2[QMAX / 2];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) { qd[q] = qs[q * 64 + lane]; god[q] = dos[q * 64 + lane]; }
#pragma unroll
  for (int q = 0; q < QMAX / 2; ++q) { dq2[q] = v2f{0.f, 0.f}; qd2[q] = v2f{qd[2 * q], qd[2 * q + 1]}; god2[q] = v2f{god[2 * q], god[2 * q + 1]}; }
  const bf16_t* kcol = Kp + lane;
  bf16_t* dKp = a.dK + (int64_t)b * a.dk_sb + (int64_t)h * 64 + lane;
  bf16_t* dVp = a.dV + (int64_t)b * a.dv_sb + (int64_t)h * 64 + lane;
  int key = 0;
#define SMQ_BWD_BATCH(U)                                                                                                  \
  for (; key + U <= S; key += U) {                                                                                        \
    float kv[U];                                                                                                          \
    _Pragma("unroll") for (int u = 0; u < U; ++u) kv[u] = bf2f(kcol[(int64_t)(key + u) * a.k_st]);                      \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                                                                      \
      const float* p = ps + (size_t)(key + u) * QMAX;                                                                     \
      const float* ds = dss + (size_t)(key + u) * QMAX;                                                                   \
      const f32x4 p0 = *reinterpret_cast<const f32x4*>(p), p1 = *reinterpret_cast<const f32x4*>(p + 4);                  \
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(ds), s1 = *reinterpret_cast<const f32x4*>(ds + 4);                \
      const v2f pa = v2f{p0[0], p0[1]}, pb = v2f{p0[2], p0[3]}, pc = v2f{p1[0], p1[1]}, pd = v2f{p1[2], p1[3]};           \
      const v2f sa = v2f{s0[0], s0[1]}, sb = v2f{s0[2], s0[3]}, sc = v2f{s1[0], s1[1]}, sd = v2f{s1[2], s1[3]};           \
      const v2f dv2 = (pa * god2[0] + pb * god2[1]) + (pc * god2[2] + pd * god2[3]);                                      \
      const v2f dk2 = (sa * qd2[0] + sb * qd2[1]) + (sc * qd2[2] + sd * qd2[3]);                                          \
      dVp[(int64_t)(key + u) * a.dv_st] = f2bf(dv2[0] + dv2[1]);                                                          \
      dKp[(int64_t)(key + u) * a.dk_st] = f2bf(dk2[0] + dk2[1]);                                                          \
      const v2f kk = v2f{kv[u], kv[u]};                                                                                   \
      dq2[0] += sa * kk; dq2[1] += sb * kk; dq2[2] += sc * kk; dq2[3] += sd * kk;                                         \
    }                                                                                                                     \
  }
  SMQ_BWD_BATCH(16)
  SMQ_BWD_BATCH(4)
#undef SMQ_BWD_BATCH
  for (; key < S; ++key) {
    const float kv = bf2f(kcol[(int64_t)key * a.k_st]);
    const float* p = ps + (size_t)key * QMAX;
    const float* ds = dss + (size_t)key * QMAX;
    float dv = 0.f, dk = 0.f;
#pragma unroll
    for (int q = 0; q < QMAX; ++q) { dv += p[q] * god[q]; dk += ds[q] * qd[q]; dq2[q >> 1][q & 1] += ds[q] * kv; }
    dVp[(int64_t)key * a.dv_st] = f2bf(dv);
    dKp[(int64_t)key * a.dk_st] = f2bf(dk);
  }
  bf16_t* dQp = a.dQ + (int64_t)b * a.dq_sb + (int64_t)h * 64 + lane;
#pragma unroll
  for (int q = 0; q < QMAX; ++q)
    if (q < nq) dQp[(int64_t)q * a.dq_st] = f2bf(dq2[q >> 1][q & 1]);
  // token sums of dQ | dK | dV of this (sample, head) = the in_proj bias gradient per sample, by the identities of the
  // tiled kernel (attention.hip): sum_key dV = sum_q dO (rows of P sum to 1), sum_key dK = 0 (rows of dS sum to 0)
  if (a.colsum_part) {
    float sq = 0.f, sv = 0.f;
#pragma unroll
    for (int q = 0; q < QMAX; ++q)
      if (q < nq) { sq += dq2[q >> 1][q & 1]; sv += god[q]; }
    float* cp = a.colsum_part + (int64_t)b * 3 * ((int64_t)a.H * 64) + (int64_t)h * 64 + lane;
    cp[0] = sq;
    cp[(int64_t)a.H * 64] = 0.f;
    cp[2 * (int64_t)a.H * 64] = sv;
  }
}

// the cases these kernels cover: bf16, head_dim 64, at most 8 queries, no causal / key-count mask (the planner of attention.hip
// asks this)
static inline bool covers(const segclip_attn_desc* d) {
  return d->dtype == SEGCLIP_BF16 && d->hd == 64 && d->Tq >= 1 && d->Tq <= QMAX && d->Tk >= 1 && !d->causal && d->klen == nullptr &&
         !(d->flags & SEGCLIP_ATTN_FP8) && lds_bytes((int)d->Tk, true) <= 64 * 1024 && lds_bytes((int)d->Tk, false) <= 64 * 1024;
}

}  // namespace smallq
