// Probe: lane maps of v_mfma_f32_32x32x16_bf16 on gfx950 and the accumulator-as-operand chaining csrc/k_attn.hip builds on:
//   A (32 x 16): element j of lane l is A[i = l % 32][k = 8 (l / 32) + j];  B (16 x 32): element j of lane l is B[k = 8 (l / 32) + j][n = l % 32];
//   D (32 x 32): register r of lane l holds D[i = rmap(r, l / 32)][n = l % 32], rmap(r, h) = (r & 3) + 8 (r >> 2) + 4 h.
//   Chaining (csrc/dq_mfma.h: split_tile, xty6): a tile with its rows in the 16 registers (row rmap(r, half)) and its column on the lane is
//   the operand of a product over its ROW index, registers 8 s .. 8 s + 7 being K-step s; the accumulator of one product is such a tile.
// Exact integer data, asymmetric.  Prints the mismatches against host products and the dependent issue cadence.
//   hipcc --offload-arch=gfx950 -O3 -o mfma32x32x16_bf16 mfma32x32x16_bf16.hip
#include "../../diffusion-deconvolution-dia-msms-data_amd/csrc/dq_mfma.h"
#include <cstdio>
using namespace dq;
__global__ void k(const float* A, const float* B, const float* X, const float* Y, const float* R, float* D, float* Z, float* W, long long* cyc) {
  const int l = threadIdx.x, col = l & 31, half = l >> 5;
  // 1. the raw instruction: one K = 16 step of small integers (exact in bf16)
  bf16x8 a, b;
  for (int j = 0; j < 8; ++j) { a[j] = (__bf16)A[col * 16 + 8 * half + j]; b[j] = (__bf16)B[(8 * half + j) * 32 + col]; }
  f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, f32x16{0}, 0, 0, 0);
  for (int r = 0; r < 16; ++r) D[rmap(r, half) * 32 + col] = d[r];
  // 2. Z = X^T Y on split tiles (9-bit integers: the H and M planes both carry bits), then W = Z'^T R with the accumulator Z' of a
  // product of small integers as the operand
  f32x16 x, y, rr, xs, ys;
  for (int r = 0; r < 16; ++r) {
    x[r] = X[rmap(r, half) * 32 + col]; y[r] = Y[rmap(r, half) * 32 + col]; rr[r] = R[rmap(r, half) * 32 + col];
    xs[r] = (float)((int)x[r] % 4); ys[r] = (float)((int)y[r] % 3);
  }
  const f32x16 z = xty6(split_tile(x), split_tile(y), f32x16{0});
  for (int r = 0; r < 16; ++r) Z[rmap(r, half) * 32 + col] = z[r];
  const f32x16 zs = xty6(split_tile(xs), split_tile(ys), f32x16{0});  // rows = X's columns, col = Y's column
  const f32x16 w = xty6(split_tile(zs), split_tile(rr), f32x16{0});   // W[n][m] = sum_i Z'[i][n] R[i][m]
  for (int r = 0; r < 16; ++r) W[rmap(r, half) * 32 + col] = w[r];
  // 3. cadence of a dependent chain
  f32x16 c0 = d;
  __builtin_amdgcn_sched_barrier(0);
  long long t0 = clock64();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 64; ++i) c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c0, 0, 0, 0);
  const float last = c0[0] + c0[5];  // waits for the chain
  __builtin_amdgcn_sched_barrier(0);
  long long t1 = clock64();
  D[1024 + l] = last + (float)(t1 & 1);
  if (l == 0) cyc[0] = t1 - t0;
}
int main() {
  static float hA[512], hB[512], hX[1024], hY[1024], hR[1024], hD[1088], hZ[1024], hW[1024];
  for (int i = 0; i < 512; ++i) { hA[i] = (float)((i * 7) % 13) - 6.f; hB[i] = (float)((i * 5) % 11) - 5.f; }
  for (int i = 0; i < 1024; ++i) { hX[i] = (float)((i * 37) % 601) - 300.f; hY[i] = (float)((i * 53) % 587) - 293.f; hR[i] = (float)((i * 29) % 397) - 198.f; }
  float *dA, *dB, *dX, *dY, *dR, *dD, *dZ, *dW; long long* dc;
  (void)hipMalloc(&dA, 2048); (void)hipMalloc(&dB, 2048); (void)hipMalloc(&dX, 4096); (void)hipMalloc(&dY, 4096); (void)hipMalloc(&dR, 4096);
  (void)hipMalloc(&dD, 4352); (void)hipMalloc(&dZ, 4096); (void)hipMalloc(&dW, 4096); (void)hipMalloc(&dc, 8);
  (void)hipMemcpy(dA, hA, 2048, hipMemcpyHostToDevice); (void)hipMemcpy(dB, hB, 2048, hipMemcpyHostToDevice);
  (void)hipMemcpy(dX, hX, 4096, hipMemcpyHostToDevice); (void)hipMemcpy(dY, hY, 4096, hipMemcpyHostToDevice); (void)hipMemcpy(dR, hR, 4096, hipMemcpyHostToDevice);
  k<<<1, 64>>>(dA, dB, dX, dY, dR, dD, dZ, dW, dc);
  long long hc = 0;
  (void)hipMemcpy(hD, dD, 4352, hipMemcpyDeviceToHost); (void)hipMemcpy(hZ, dZ, 4096, hipMemcpyDeviceToHost);
  (void)hipMemcpy(hW, dW, 4096, hipMemcpyDeviceToHost); (void)hipMemcpy(&hc, dc, 8, hipMemcpyDeviceToHost);
  int bad_d = 0, bad_z = 0, bad_w = 0;
  static double zs[1024];
  for (int i = 0; i < 32; ++i) for (int j = 0; j < 32; ++j) {
    double s = 0; for (int kk = 0; kk < 16; ++kk) s += (double)hA[i * 16 + kk] * hB[kk * 32 + j];
    bad_d += (double)hD[i * 32 + j] != s;
    double z = 0, q = 0;
    for (int kk = 0; kk < 32; ++kk) { z += (double)hX[kk * 32 + i] * hY[kk * 32 + j]; q += (double)((int)hX[kk * 32 + i] % 4) * ((int)hY[kk * 32 + j] % 3); }
    bad_z += (double)hZ[i * 32 + j] != z;
    zs[i * 32 + j] = q;
  }
  for (int n = 0; n < 32; ++n) for (int m = 0; m < 32; ++m) {
    double s = 0; for (int i = 0; i < 32; ++i) s += zs[i * 32 + n] * hR[i * 32 + m];
    bad_w += (double)hW[n * 32 + m] != s;
  }
  printf("mfma_f32_32x32x16_bf16 lane map: %d mismatches of 1024\n", bad_d);
  printf("split-bf16 X^T Y (xty6): %d mismatches of 1024; accumulator as operand: %d mismatches of 1024\n", bad_z, bad_w);
  printf("64 MFMAs on one accumulator: %lld clocks (%.1f each)\n", hc, hc / 64.0);
  return (bad_d | bad_z | bad_w) != 0;
}
