// Sampling from the CustomTransformer inside the library: dq_tfm_sample runs the call's record as the
// U-Net's entry does (dq_sampler.h: the shared refusals, tables and captured-or-eager tail around this network's layout, prologue and
// forward), one update per step behind a sampling forward of the network -- and the stand-alone entry of the fused inference attention
// (k_tfm_attn.hip).  What does not depend on the step is computed once per call, before the loop: the conditional
// embedding cp of the MS1 chromatogram, every layer's K | V rows of it, and the time embedding of every step.  The forward itself is the
// one walk of the network (tfm_walk, dq_tfm.hip) that dq_tfm_fwd makes too, here with its K | V rows cached.
// Held-out evaluation: dq_tfm_eval_step runs the same prologue and the same forward once over R repeats of a batch
// stacked into R * B samples -- the conditional rows computed for the B windows and copied to the other repeats, the time table one row per
// sample -- between the stacked noising head and the stacked per-window MSE of k_stream.hip.
#include "../../include/dq_hip.h"
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_net.h"  // DQ_TRY
#include "dq_options.h"
#include "dq_sampler.h"
#include "dq_tfm.h"
#include "dq_tfm_net.h"
#include <cmath>
#include <vector>

namespace dq {
namespace {

// workspace of a sampling call: the inference buffers of carve() (its comb and kv stay unused), then the L persistent kv_l, the time table
// and its inputs, then the sampler's state; carved in a fixed order
struct SampleWs {
  Ws net;
  std::vector<float*> kv;  // per layer (B, Sk, 2H): rows [0, S2) the call's conditional K | V, rows [S2, Sk) the step's
  int64_t* t64;            // (num_steps) the timesteps as the time-feature kernel reads them
  TimeBufs time;           // time MLP over all steps: temb is the (num_steps, H) table
  float *xa, *xb, *eps, *coef, *sigma;
  int *ts_tab, *step;
  uint64_t* seed_stage;
  int64_t* ids_stage;
  int64_t floats = 0;
};

SampleWs carve_sample(const dq_tfm& p, float* base, int B, int S1, int S2, int ns) {
  SampleWs w;
  Carver c{base};
  w.net = carve(p, c, B, S1, S2, false);
  const int64_t H = p.H, n = (int64_t)B * S1 * p.D;
  w.kv = carve_kv(p, c, B, S1 + S2);
  w.t64 = c.take<int64_t>(ns);
  w.time.tfeat = c.take(ns * H); w.time.th = c.take(ns * 4 * H); w.time.tg = c.take(ns * 4 * H); w.time.temb = c.take(ns * H);
  w.xa = c.take(n); w.xb = c.take(n); w.eps = c.take(n);
  w.coef = c.take(4 * (int64_t)ns); w.sigma = c.take(ns);
  w.ts_tab = c.take<int>(ns);
  w.step = c.take<int>(4);
  w.seed_stage = c.take<uint64_t>(2);
  w.ids_stage = c.take<int64_t>(B);
  w.floats = c.off;
  return w;
}

// workspace of an evaluation call over N = R * B stacked samples: the inference buffers of carve() at batch N (its time buffers hold the
// per-sample time table; its comb and kv stay unused), the L kv_l, x_t, the network output (unused when the caller passes net_out) and the
// slice sums of the per-window MSE
struct EvalWs {
  Ws net;
  std::vector<float*> kv;  // per layer (N, Sk, 2H)
  float *xt, *out;
  double* slices;
  int64_t floats = 0;
};

EvalWs carve_eval(const dq_tfm& p, float* base, int B, int S1, int S2, int R) {
  EvalWs w;
  Carver c{base};
  const int N = R * B;
  const int64_t per = (int64_t)S1 * p.D;
  w.net = carve(p, c, N, S1, S2, false);
  w.kv = carve_kv(p, c, N, S1 + S2);
  w.xt = c.take(N * per); w.out = c.take(N * per);
  w.slices = c.take<double>(mse_per_window_scratch_bytes(N, per) / (int64_t)sizeof(double));
  w.floats = c.off;
  return w;
}

// A call's forwards as the walk sees them: the cached form of K | V (the conditional rows of k.kv are the prologue's), every layer in buffer
// set 0, no LayerNorm stats; time_per_sample says how the walk adds temb -- sampling: a (num_steps, H) table, the step's row to every
// sample; evaluation: one row per stacked sample
TfmWalk cached_walk(const dq_tfm* p, const float* P, const float* sin_t, const float* cos_t, const Ws& net, float* const* kv, const float* temb,
                    bool time_per_sample, int B, int S1, int S2) {
  TfmWalk k{p, P, sin_t, cos_t, &net, B, S1, S2};
  k.kv = kv; k.attn_form = tfm_attn_form(S1, S1 + S2, p->H / p->heads); k.temb = temb; k.time_per_sample = time_per_sample;
  return k;
}

// once per call, eagerly: cp = rope((cm x_cond + ca) w + b) of the first Bc of the walk's B samples, every layer's K | V rows of it (copied to
// the other B / Bc - 1 repeats; sampling: Bc == B), the time embedding of the nt timesteps at t64 into tb.temb (== k.temb)
int sample_prologue(const TfmWalk& k, int Bc, const float* ms1, float cm, float ca, const float* time_freqs, const int64_t* t64, int nt,
                    const TimeBufs& tb, hipStream_t s) {
  const dq_tfm& p = *k.p;
  const Ws& n = *k.w;
  const int H = p.H, Sk = k.S1 + k.S2;
  DQ_TRY(launch_cond_embed_affine(ms1, cm, ca, k.P + p.c_w, k.P + p.c_b, k.sin_t, k.cos_t, n.cp, Bc, k.S2, H, s));
  for (int l = 0; l < p.layers; ++l) {
    DQ_TRY(tfm_kv_rows(p, k.P, l, n.cp, k.S2, 0, Bc, k.kv[l], Sk, n.partial, s));
    DQ_TRY(launch_tfm_kv_broadcast(k.kv[l], Bc, k.B / Bc, k.S2, Sk, H, s));  // (one repeat: no launch)
  }
  return tfm_time_mlp(p, k.P, t64, time_freqs, tb, nt, n.partial, s);  // "batch" = the steps, or the stacked samples
}

}  // namespace
}  // namespace dq

using namespace dq;

extern "C" {

int dq_tfm_attn_form(int S1, int Sk, int dh) { return tfm_attn_form(S1, Sk, dh); }

int dq_tfm_attn_fwd(const float* q, const float* kv, float* o, float* prob_scratch, int B, int S1, int Sk, int H, int heads, int form,
                    void* stream) {
  DQ_REQUIRE(q && kv && o, "dq_tfm_attn_fwd: null argument");
  DQ_REQUIRE(B > 0 && S1 > 0 && Sk > 0 && H > 0 && heads > 0 && H % heads == 0 && (H / heads) % 4 == 0,
             "dq_tfm_attn_fwd: sizes must be positive, H divisible by heads, the head width a multiple of 4");
  DQ_REQUIRE(form >= -1 && form <= 1, "dq_tfm_attn_fwd: form must be -1 (chosen), 0 (three launches) or 1 (fused)");
  DQ_REQUIRE((((uintptr_t)q | (uintptr_t)kv | (uintptr_t)o) & 15) == 0, "dq_tfm_attn_fwd: q, kv and o must be 16-byte aligned");
  const int dh = H / heads, chosen = tfm_attn_form(S1, Sk, dh);
  DQ_REQUIRE(form != TFM_ATTN_FUSED || chosen == TFM_ATTN_FUSED, "dq_tfm_attn_fwd: the fused form does not take this shape (dq_tfm_attn_form): K, V and the waves' rows exceed the LDS of a CU");
  const int f = form < 0 ? chosen : form;
  DQ_REQUIRE(f == TFM_ATTN_FUSED || prob_scratch, "dq_tfm_attn_fwd: the three-launch form needs prob_scratch (B heads S1 up4(Sk) floats)");
  const AttnDims ad{B, S1, Sk, H, heads, dh, up4(Sk)};
  return tfm_attention_fwd(f, ad, q, kv, prob_scratch, o, nullptr, (hipStream_t)stream);  // (the attention products are never split: no scratch)
}

int64_t dq_tfm_sample_workspace_bytes(const dq_tfm* p, int B, int S1, int S2, int num_steps) {
  if (!p || B <= 0 || S1 <= 0 || S2 <= 0 || num_steps < 1 || num_steps > 1024) return 0;
  return carve_sample(*p, nullptr, B, S1, S2, num_steps).floats * (int64_t)sizeof(float);
}

int dq_tfm_sample(dq_tfm* p, const float* params, const float* rope_sin, const float* rope_cos, const float* time_freqs, int S2,
                  const dq_sample_call* call) {
  SampleCall q;
  DQ_TRY(sample_call_open(call, "dq_tfm_sample", false, &q));
  const int B = q.B, S1 = q.RT, num_steps = q.num_steps, auto_normalize = q.auto_normalize;
  SamplerChoice sc;
  DQ_TRY(sample_check(q, p && params && rope_sin && rope_cos && time_freqs, &sc));
  // what the record can say and this network's loop is not built for: refused, never silently ignored
  DQ_REQUIRE(!q.guided, "dq_tfm_sample: guided sampling is built for the U-Net (dq_ddim_sample); guidance for this network is the follow-up");
  DQ_REQUIRE(!q.per_window(), "dq_tfm_sample: guidance_rescale and threshold_quantile are built for the U-Net (dq_ddim_sample); the per-window "
                              "statistics step for this network is the follow-up");
  DQ_REQUIRE(q.consistency == DQ_CONSIST_NONE, "dq_tfm_sample: consistency is built for the U-Net (dq_ddim_sample); the group pass for this network is the follow-up");
  DQ_REQUIRE(B > 0 && S1 > 0 && S2 > 0 && num_steps >= 1 && num_steps <= 1024, "dq_tfm_sample: need B, S1, S2 > 0 and 1 <= num_steps <= 1024");
  DQ_REQUIRE(q.num_timesteps >= 1, "dq_tfm_sample: num_timesteps must be >= 1");
  DQ_REQUIRE(((uintptr_t)params & 15) == 0 && ((uintptr_t)q.workspace & 15) == 0, "dq_tfm_sample: params and workspace must be 16-byte aligned");
  const SampleWs w = carve_sample(*p, (float*)q.workspace, B, S1, S2, num_steps);
  DQ_REQUIRE(q.workspace_bytes >= w.floats * (int64_t)sizeof(float), "dq_tfm_sample: workspace too small (dq_tfm_sample_workspace_bytes)");
  PrecisionScope prec(p->precision);
  hipStream_t s = q.s();
  const int64_t per = (int64_t)S1 * p->D;
  const float cm = auto_normalize ? 2.f : 1.f, ca = auto_normalize ? -1.f : 0.f;
  const TfmWalk net = cached_walk(p, params, rope_sin, rope_cos, w.net, w.kv.data(), w.time.temb, false, B, S1, S2);
  // the steps' timesteps for the time table (the copy is done when sample_begin returns: it synchronises the stream)
  std::vector<int64_t> t64(q.timesteps_host, q.timesteps_host + num_steps);
  DQ_HIP_OK(hipMemcpyAsync(w.t64, t64.data(), sizeof(int64_t) * t64.size(), hipMemcpyHostToDevice, s));
  DQ_TRY(sample_begin(q, sc, per, w.coef, w.sigma, w.xa));
  if (net.attn_form == TFM_ATTN_FUSED) DQ_TRY(tfm_attn_prepare());  // (the LDS limit of this device, before any capture)
  // every call, outside any capture: a changed MS1, or changed weights behind the same pointer, cannot meet a stale cache
  DQ_TRY(sample_prologue(net, B, q.ms1_cond, cm, ca, time_freqs, w.t64, num_steps, w.time, s));
  // the forward of this network: a linear graph when captured (one stream, no branches); the time row is `row`, or read at *step_ptr
  const StepForward forward = [&](const float* x, float*, int row, const int* step_ptr, float* net_out, bool, bool* fused, hipStream_t fs) {
    *fused = false;  // (the update is never in this network's launches)
    TfmWalk step = net;
    step.time_row = row; step.step_ptr = step_ptr;
    return tfm_walk(step, x, net_out, fs);
  };
  const SampleLoop loop{forward, StepUpdateArgs{sc.kind, w.coef, w.sigma, w.xb, sc.clip_x0, sc.pred, B, per}, w.xa, w.eps, sc.clip,
                        num_steps, q.ms2_cond, q.out_x, q.out_noise, auto_normalize};
  TfmStepKey key;
  key.params = params; key.ws = q.workspace; key.rope_sin = rope_sin; key.rope_cos = rope_cos; key.B = B; key.S1 = S1; key.S2 = S2;
  key.num_steps = num_steps; key.normalize = auto_normalize; key.pred = q.pred_type; key.precision = p->precision; key.update = sc.kind; key.clip = sc.clip_x0;
  key.opt_epoch = options_epoch();
  bool captured;
  const int rc = sample_run(q, loop, sc.sto, p->step, p->step.exec && p->step_key == key, StepStage{w.step, w.seed_stage, w.ids_stage}, &captured);
  if (captured) p->step_key = key;
  return rc;
}

int dq_tfm_kv_broadcast(float* kv, int B, int repeats, int S2, int Sk, int H, void* stream) {
  return launch_tfm_kv_broadcast(kv, B, repeats, S2, Sk, H, (hipStream_t)stream);
}

int64_t dq_tfm_eval_workspace_bytes(const dq_tfm* p, int B, int S1, int S2, int repeats) {
  if (!p || B <= 0 || S1 <= 0 || S2 <= 0 || repeats < 1 || (int64_t)repeats * B > 65535) return 0;
  return carve_eval(*p, nullptr, B, S1, S2, repeats).floats * (int64_t)sizeof(float);
}

int dq_tfm_eval_step(dq_tfm* p, const float* params, const float* rope_sin, const float* rope_cos, const float* time_freqs,
                     const float* alpha_bars_dev, const float* x0, const float* ms1_cond, const int64_t* t, const float* noise,
                     const uint64_t* seed_dev, const int64_t* window_ids_dev, int first_draw, int auto_normalize, int pred_type,
                     const float* loss_weight_dev, float* loss_out, float* per_window_out, float* net_out, void* workspace,
                     int64_t workspace_bytes, int B, int S1, int S2, int repeats, void* stream) {
  DQ_REQUIRE(p && params && rope_sin && rope_cos && time_freqs && alpha_bars_dev && x0 && ms1_cond && t && loss_out && per_window_out && workspace,
             "dq_tfm_eval_step: null argument");
  DQ_REQUIRE(pred_type == DQ_PRED_EPS || pred_type == DQ_PRED_X0, "dq_tfm_eval_step: Unknown pred_type");
  DQ_REQUIRE(pred_type == DQ_PRED_EPS || loss_weight_dev, "dq_tfm_eval_step: pred_type x0 needs the loss-weight (SNR) table");
  DQ_REQUIRE(B > 0 && S1 > 0 && S2 > 0, "dq_tfm_eval_step: B, S1 and S2 must be positive");
  DQ_REQUIRE(repeats >= 1, "dq_tfm_eval_step: repeats must be >= 1");
  DQ_REQUIRE((int64_t)repeats * B <= 65535, "dq_tfm_eval_step: repeats * B must not exceed 65535");
  DQ_REQUIRE(noise || seed_dev, "dq_tfm_eval_step: a null noise needs the seed (device memory)");
  DQ_REQUIRE(first_draw >= 0, "dq_tfm_eval_step: first_draw must be >= 0");
  DQ_REQUIRE(((uintptr_t)params & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)x0 & 15) == 0 && ((uintptr_t)noise & 15) == 0 &&
                 ((uintptr_t)net_out & 15) == 0,
             "dq_tfm_eval_step: params, workspace, x0, noise and net_out must be 16-byte aligned");
  const int R = repeats, N = R * B;
  DQ_REQUIRE((int64_t)N * (S1 + S2) <= INT32_MAX / 4, "dq_tfm_eval_step: repeats * B * (S1 + S2) too large");
  const EvalWs w = carve_eval(*p, (float*)workspace, B, S1, S2, R);
  DQ_REQUIRE(workspace_bytes >= w.floats * (int64_t)sizeof(float), "dq_tfm_eval_step: workspace too small (dq_tfm_eval_workspace_bytes)");
  PrecisionScope prec(p->precision);
  hipStream_t s = (hipStream_t)stream;
  const int64_t per = (int64_t)S1 * p->D;
  const float cm = auto_normalize ? 2.f : 1.f, ca = auto_normalize ? -1.f : 0.f;
  // the time table: one row per stacked sample, in carve()'s time buffers (batch N); t is read where it lies
  const TfmWalk net = cached_walk(p, params, rope_sin, rope_cos, w.net, w.kv.data(), w.net.time.temb, true, N, S1, S2);
  float* out = net_out ? net_out : w.out;
  if (net.attn_form == TFM_ATTN_FUSED) DQ_TRY(tfm_attn_prepare());
  const NoiseStack st{R, window_ids_dev, seed_dev, first_draw};
  DQ_TRY(launch_q_sample(alpha_bars_dev, x0, t, noise, w.xt, B, per, auto_normalize, s, &st));
  // every call, eagerly: nothing of it outlives the call, so a changed MS1 or changed weights behind the same pointer meet no stale state
  DQ_TRY(sample_prologue(net, B, ms1_cond, cm, ca, time_freqs, t, N, w.net.time, s));
  DQ_TRY(tfm_walk(net, w.xt, out, s));
  // the objective's target over the stack: the clean window is shared by the repeats, the noise has one row per stacked window (or none:
  // loss_target then says DRAWN)
  LossTarget tg = loss_target(pred_type, x0, noise, alpha_bars_dev, cm, ca, loss_weight_dev, t);
  tg.stacked = true; tg.Bt = tg.shared ? B : N; tg.ids = window_ids_dev; tg.seed = seed_dev; tg.first_draw = first_draw;
  return launch_mse_per_window(out, tg, per_window_out, loss_out, w.slices, mse_per_window_scratch_bytes(N, per), B, R, per, s);
}

}  // extern "C"
