// The CustomTransformer handle and what its passes share (dq_tfm.hip: forward and backward; dq_tfm_sample.hip: the sampling loop).
// Internal: not installed.
#pragma once
#include "dq_common.h"
#include "dq_tfm.h"
#include "dq_unet.h"  // StepUpdate, StepGraph
#include <string>
#include <vector>

namespace dq {

struct TfmParam { std::string name; int64_t offset; int ndim; int64_t shape[2]; int64_t numel; };
struct TfmLayer { int64_t in_w, in_b, out_w, out_b, n1_g, n1_b, f0_w, f0_b, f2_w, f2_b, n2_g, n2_b; };

// Everything a captured sampling step of the transformer has baked into its kernel arguments or its dispatch (StepKey's counterpart).
// num_steps: the workspace is carved by it (the time table sits in front of the sampler's state), so the baked addresses move with it
struct TfmStepKey {
  const void* params = nullptr; const void* ws = nullptr; const void* rope_sin = nullptr; const void* rope_cos = nullptr;
  int B = 0, S1 = 0, S2 = 0, num_steps = 0, normalize = -1, pred = -1, precision = -1;
  StepUpdate update = StepUpdate::DDIM;
  float clip = 0.f;
  unsigned opt_epoch = 0;
  bool operator==(const TfmStepKey& o) const {
    return params == o.params && ws == o.ws && rope_sin == o.rope_sin && rope_cos == o.rope_cos && B == o.B && S1 == o.S1 && S2 == o.S2 && num_steps == o.num_steps &&
           normalize == o.normalize && pred == o.pred && precision == o.precision && update == o.update && clip == o.clip && opt_epoch == o.opt_epoch;
  }
};

}  // namespace dq

struct dq_tfm {
  int D = 0, H = 0, heads = 0, layers = 0;
  std::vector<dq::TfmParam> params;
  int64_t total = 0;
  int64_t in_w, in_b, out_w, out_b, c_w, c_b, t1_w, t1_b, t2_w, t2_b;
  std::vector<dq::TfmLayer> L;
  // which training workspaces hold a forward's saved activations (one entry per workspace; several forwards may be in flight before
  // their backwards run: micro-batches whose losses are summed).  An entry stays until the same workspace takes another forward.
  struct Saved { const void* ws; int B, S1, S2; };
  std::vector<Saved> saved;
  int precision = dq::GEMM_FP32;  // arithmetic of the dense products (dq_tfm_set_precision)
  dq::StepGraph step;  // the captured sampling step of dq_tfm_sample; valid while step_key holds
  dq::TfmStepKey step_key;
};

namespace dq {

constexpr int64_t TFM_PARTIAL_FLOATS = (int64_t)(768 + 256) * 128 * 128;  // bound of launch_gemm's split-K scratch (k_gemm.hip: choose())
inline int64_t up4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// workspace: carved in a fixed order; `training` keeps one set of layer buffers per layer (read by the backward)
struct Ws {
  float *cp, *tfeat, *th, *tg, *temb, *x0, *tmp, *partial, *colscr, *lnscr;
  struct Layer { float *comb, *q, *kv, *prob, *ao, *y1, *st1, *x1, *hpre, *hact, *y2, *st2, *xo; };
  std::vector<Layer> L;
  // backward only
  float *dxa, *dxb, *dh, *dq, *dkv, *dprob, *dao, *dcomb, *dcp, *dtemb, *dtg;
  int64_t floats = 0;
};
Ws carve(const dq_tfm& p, float* base, int B, int S1, int S2, bool training);

// y (M, N) = x (M, K) W^T + b   with W an nn.Linear weight (N, K); partial: TFM_PARTIAL_FLOATS floats of split-K scratch
int tfm_linear(const float* x, const float* w, const float* b, float* y, int M, int N, int K, float* partial, hipStream_t s);

struct AttnDims { int B, S1, Sk, H, heads, dh; int64_t ldp; };
// batched (sample, head) products of the attention; `which`: 0 scores = Q K^T, 1 O = P V, 2 dP = dO V^T, 3 dV = P^T dO,
// 4 dQ = dS K, 5 dK = dS^T Q
int attn_gemm(int which, const AttnDims& d, const float* q, const float* kv, float* prob, float* o, float* partial, hipStream_t s);
// the attention of an inference pass by form (TfmAttnForm): one fused launch, or scores GEMM -> softmax rows -> PV GEMM through `prob`
// ((B heads S1) rows of up4(Sk) floats; unused by the fused form)
int tfm_attention_fwd(int form, const AttnDims& d, const float* q, const float* kv, float* prob, float* o, float* partial, hipStream_t s);

// the handle's precision as the thread's GEMM default for the duration of one call
struct PrecisionScope {
  int old;
  explicit PrecisionScope(int p) : old(set_gemm_precision(p)) {}
  ~PrecisionScope() { set_gemm_precision(old); }
};

}  // namespace dq
