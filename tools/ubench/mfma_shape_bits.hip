// Do a v_mfma_f32_16x16x32_bf16 chain and a v_mfma_f32_32x32x16_bf16 chain over the same k order give the same fp32 bits?
// One wave per trial: C(i, j) = sum_k A(i, k) B(j, k), i, j < 16, K = 64 .. 768 (the GEMM K loop's accumulation: one MFMA
// per k chunk into the same accumulators), random bf16 operands of the GEMMs' magnitudes.  Prints, per K, how many of the
// 256 x trials results differ and the largest difference in units of the last place.
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/mfma_shape_bits.hip -o tools/ubench/mfma_shape_bits && tools/ubench/mfma_shape_bits
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int KMAX = 768, TRIALS = 256;

// A, B: [TRIALS][32][K] bf16 (rows 16..31 feed the 32x32 form only); c16, c32: [TRIALS][16][16]
__global__ __launch_bounds__(64) void probe(const __bf16* A, const __bf16* B, int K, float* c16, float* c32) {
  const int l = threadIdx.x, t = blockIdx.x;
  const __bf16* a = A + (size_t)t * 32 * K;
  const __bf16* b = B + (size_t)t * 32 * K;
  f32x4 acc4 = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {   // lane l: row l&15, k = k0 + 8 (l>>4) + j
    const bf16x8 fa = *reinterpret_cast<const bf16x8*>(a + (l & 15) * K + k0 + 8 * (l >> 4));
    const bf16x8 fb = *reinterpret_cast<const bf16x8*>(b + (l & 15) * K + k0 + 8 * (l >> 4));
    acc4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc4, 0, 0, 0);
  }
  f32x16 acc16 = {};
  for (int k0 = 0; k0 < K; k0 += 16) {   // lane l: row l&31, k = k0 + 8 (l>>5) + j
    const bf16x8 fa = *reinterpret_cast<const bf16x8*>(a + (l & 31) * K + k0 + 8 * (l >> 5));
    const bf16x8 fb = *reinterpret_cast<const bf16x8*>(b + (l & 31) * K + k0 + 8 * (l >> 5));
    acc16 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc16, 0, 0, 0);
  }
  // C/D maps: 16x16: column l&15, row 4 (l>>4) + r; 32x32: column l&31, row (r&3) + 8 (r>>2) + 4 (l>>5)
  float* o16 = c16 + t * 256;
  float* o32 = c32 + t * 256;
  for (int r = 0; r < 4; ++r) o16[(4 * (l >> 4) + r) * 16 + (l & 15)] = acc4[r];
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col = l & 31;
    if (row < 16 && col < 16) o32[row * 16 + col] = acc16[r];
  }
}

static uint16_t to_bf16(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

int main() {
  const size_t nel = (size_t)TRIALS * 32 * KMAX;
  std::vector<uint16_t> ha(nel), hb(nel);
  std::mt19937 rng(1234);
  std::normal_distribution<float> nd(0.f, 1.f);
  for (size_t i = 0; i < nel; ++i) ha[i] = to_bf16(nd(rng));
  for (size_t i = 0; i < nel; ++i) hb[i] = to_bf16(nd(rng) * 0.036f);   // ~ K^-1/2 weights
  __bf16 *da, *db;
  float *d16, *d32;
  CK(hipMalloc(&da, nel * 2));
  CK(hipMalloc(&db, nel * 2));
  CK(hipMalloc(&d16, TRIALS * 256 * 4));
  CK(hipMalloc(&d32, TRIALS * 256 * 4));
  CK(hipMemcpy(da, ha.data(), nel * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(db, hb.data(), nel * 2, hipMemcpyHostToDevice));
  std::vector<float> h16(TRIALS * 256), h32(TRIALS * 256);
  int differ_any = 0;
  for (int K : {64, 128, 768}) {   // A and B are read as [TRIALS][32][K]: K <= KMAX keeps every read inside the buffers
    hipLaunchKernelGGL(probe, dim3(TRIALS), dim3(64), 0, 0, da, db, K, d16, d32);
    CK(hipGetLastError());
    CK(hipMemcpy(h16.data(), d16, TRIALS * 256 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h32.data(), d32, TRIALS * 256 * 4, hipMemcpyDeviceToHost));
    int diff = 0;
    double ulp = 0.0;
    for (int i = 0; i < TRIALS * 256; ++i) {
      if (memcmp(&h16[i], &h32[i], 4) == 0) continue;
      ++diff;
      const double u = std::ldexp(1.0, std::ilogb(h32[i]) - 23);
      ulp = std::fmax(ulp, std::fabs((double)h16[i] - (double)h32[i]) / u);
    }
    printf("K=%d: %d of %d results differ in their bits (max %.1f ulp)\n", K, diff, TRIALS * 256, ulp);
    differ_any |= diff != 0;
  }
  printf("16x16x32 vs 32x32x16 chains: %s\n", differ_any ? "NOT bit-identical" : "bit-identical");
  CK(hipFree(da));
  CK(hipFree(db));
  CK(hipFree(d16));
  CK(hipFree(d32));
  return 0;
}
