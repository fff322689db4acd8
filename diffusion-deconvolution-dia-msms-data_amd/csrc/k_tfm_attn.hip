// Fused inference attention of the CustomTransformer's sampling path: per (sample, head)
// o = softmax(q k^T / sqrt(dh)) v in ONE launch, nothing but `o` written to HBM.  The training path keeps its three launches (scores GEMM,
// k_softmax_rows, PV GEMM: dq_tfm.hip), which save `prob` for the backward.
//
// Layout: a block of four waves owns one (sample, head) and a range of query rows.  It stages the head's K (row pitch dh + 4 floats: a
// lane reads ITS key's row as float4, and the pad spreads the 64 rows over the banks) and V (pitch dh: lanes read consecutive columns)
// in LDS once; then every wave takes query rows in turn: scores (lane = key, the dot product over dh in fp32 FMAs, four partial sums
// added in a fixed order), max-subtracted softmax across the wave (the arithmetic of k_softmax_rows: expf(scale * s - max), one
// reciprocal of the sum), P V (lane = output column, the sum over the keys in fp32 FMAs, four partial sums in a fixed order).  fp32 VALU
// throughout, also when the handle runs its GEMMs in bf16x3.  Every output element is formed by one lane in an order that depends on
// nothing but (Sk, dh): bitwise repeatable, and independent of how the rows are cut into blocks.
#include "dq_common.h"
#include "dq_tfm.h"
#include <algorithm>
#include <mutex>
#include <vector>

namespace dq {

namespace {
inline int64_t up4l(int64_t v) { return (v + 3) & ~(int64_t)3; }
constexpr int ATTN_WAVES = 4;
constexpr int64_t ATTN_LDS_BUDGET = 160 * 1024;  // bytes of LDS a CU has (gfx950); one block per CU at the bound

__global__ void __launch_bounds__(64 * ATTN_WAVES) k_tfm_attn_fwd(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ o,
                                                                 int S1, int Sk, int H, int heads, int dh, int rpb, float scale) {
  extern __shared__ float4 attn_lds4[];
  float* lds = reinterpret_cast<float*>(attn_lds4);
  const int kp = dh + 4, ldp = (Sk + 3) & ~3, d4 = dh >> 2;
  float* Ks = lds;
  float* Vs = Ks + Sk * kp;
  float* Qs = Vs + Sk * dh;
  float* Ps = Qs + ATTN_WAVES * dh;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* kvb = kv + (int64_t)b * Sk * 2 * H + (int64_t)h * dh;
  for (int i = threadIdx.x; i < Sk * d4; i += 64 * ATTN_WAVES) {
    const int j = i / d4, c = i - j * d4;
    const float* src = kvb + (int64_t)j * 2 * H + 4 * c;
    *reinterpret_cast<float4*>(Ks + j * kp + 4 * c) = *reinterpret_cast<const float4*>(src);
    *reinterpret_cast<float4*>(Vs + j * dh + 4 * c) = *reinterpret_cast<const float4*>(src + H);
  }
  __syncthreads();
  float* qs = Qs + wave * dh;
  float* ps = Ps + wave * ldp;
  const int r0 = blockIdx.y * rpb, r1 = min(S1, r0 + rpb);
  for (int r = r0 + wave; r < r1; r += ATTN_WAVES) {  // (wave-uniform: what follows crosses lanes of ONE wave only)
    const float* qr = q + ((int64_t)b * S1 + r) * H + (int64_t)h * dh;
    float* orow = o + ((int64_t)b * S1 + r) * H + (int64_t)h * dh;
    __builtin_amdgcn_wave_barrier();  // the previous row's reads of qs / ps are done before they are overwritten (LDS is in order per wave)
    for (int c = lane; c < d4; c += 64) reinterpret_cast<float4*>(qs)[c] = reinterpret_cast<const float4*>(qr)[c];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float m = -INFINITY;
    for (int j = lane; j < Sk; j += 64) {
      const float4* kr = reinterpret_cast<const float4*>(Ks + j * kp);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int c = 0; c < d4; ++c) {
        const float4 qv = reinterpret_cast<const float4*>(qs)[c], kk = kr[c];
        a0 = fmaf(qv.x, kk.x, a0); a1 = fmaf(qv.y, kk.y, a1); a2 = fmaf(qv.z, kk.z, a2); a3 = fmaf(qv.w, kk.w, a3);
      }
      const float sc = ((a0 + a1) + (a2 + a3)) * scale;
      ps[j] = sc;  // (this lane's own entries until the barrier below)
      m = fmaxf(m, sc);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < Sk; j += 64) {
      const float e = expf(ps[j] - m);
      ps[j] = e;
      sum += e;
    }
    const float inv = 1.0f / wave_sum(sum);
    for (int j = lane; j < Sk; j += 64) ps[j] *= inv;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int d = lane; d < dh; d += 64) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int j = 0;
      for (; j + 4 <= Sk; j += 4) {
        const float4 p = *reinterpret_cast<const float4*>(ps + j);
        a0 = fmaf(p.x, Vs[j * dh + d], a0); a1 = fmaf(p.y, Vs[(j + 1) * dh + d], a1);
        a2 = fmaf(p.z, Vs[(j + 2) * dh + d], a2); a3 = fmaf(p.w, Vs[(j + 3) * dh + d], a3);
      }
      for (; j < Sk; ++j) a0 = fmaf(ps[j], Vs[j * dh + d], a0);
      orow[d] = (a0 + a1) + (a2 + a3);
    }
  }
}
}  // namespace

int64_t tfm_attn_lds_bytes(int Sk, int dh) {
  return (int64_t)sizeof(float) * ((int64_t)Sk * (2 * (int64_t)dh + 4) + (int64_t)ATTN_WAVES * dh + (int64_t)ATTN_WAVES * up4l(Sk));
}

int tfm_attn_form(int S1, int Sk, int dh) {
  if (S1 < 1 || Sk < 1 || dh < 4) return -1;
  return (dh % 4 == 0 && tfm_attn_lds_bytes(Sk, dh) <= ATTN_LDS_BUDGET) ? TFM_ATTN_FUSED : TFM_ATTN_GEMM;
}

int tfm_attn_prepare() {
  static std::mutex mu;
  static std::vector<int> done;  // devices whose limit is raised
  int dev = 0;
  DQ_HIP_OK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (std::find(done.begin(), done.end(), dev) != done.end()) return 0;
  DQ_HIP_OK(hipFuncSetAttribute((const void*)k_tfm_attn_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_LDS_BUDGET));
  done.push_back(dev);
  return 0;
}

int launch_tfm_attn_fwd(const float* q, const float* kv, float* o, int B, int S1, int Sk, int H, int heads, hipStream_t s) {
  DQ_REQUIRE(B > 0 && heads > 0 && H % heads == 0, "tfm_attn_fwd: H must be divisible by heads");
  const int dh = H / heads;
  DQ_REQUIRE(tfm_attn_form(S1, Sk, dh) == TFM_ATTN_FUSED, "tfm_attn_fwd: the fused form does not take this shape (dq_tfm_attn_form)");
  DQ_REQUIRE(H % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)kv & 15) == 0, "tfm_attn_fwd: q and kv must be 16-byte aligned");
  const size_t lds = (size_t)tfm_attn_lds_bytes(Sk, dh);
  if (int rc = tfm_attn_prepare()) return rc;
  // rows per block: about 512 blocks in all (two per CU) when the batch alone does not give them; a multiple of the wave count.  The cut
  // changes no result: a row is one wave's work whichever block it lands in.
  const int64_t bh = (int64_t)B * heads;
  const int want = (int)std::max<int64_t>(1, cdiv(512, bh));
  int rpb = std::max(ATTN_WAVES, cdiv(S1, want));
  rpb = (rpb + ATTN_WAVES - 1) / ATTN_WAVES * ATTN_WAVES;
  hipLaunchKernelGGL(k_tfm_attn_fwd, dim3((unsigned)bh, (unsigned)cdiv(S1, rpb)), dim3(64 * ATTN_WAVES), lds, s, q, kv, o, S1, Sk, H, heads, dh, rpb,
                     1.0f / sqrtf((float)dh));
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
