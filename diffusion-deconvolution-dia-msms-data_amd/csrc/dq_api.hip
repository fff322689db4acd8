// The C ABI (include/dq_hip.h) but the samplers (dq_sampler.hip, dq_sampler_tables.cpp), the stand-alone op entry points (dq_ops_api.hip) and
// the debug entry points that need the network file's private types (dq_unet.hip): errors, the device queries of dq_launch.h (CU count, occupancy
// cache, one resident round, the dynamic-LDS limit), plan lifetime and queries,
// options, the thin wrappers of the stream kernels, and the network passes -- forward, backward, the fused train step and the evaluation step.
#include "dq_dev.h"
#include "dq_launch.h"
#include "dq_net.h"
#include "dq_options.h"
#include "../../include/dq_hip.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace dq {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

int occ_blocks_per_cu(const void* fn, int threads, size_t lds) {
  struct Key { const void* fn; size_t lds; int threads, dev; };
  struct Ent { Key k; int nb; };
  static std::mutex mu;
  static std::vector<Ent> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("occ_blocks_per_cu: hipGetDevice failed"); return -1; }
  std::lock_guard<std::mutex> lock(mu);
  for (const Ent& e : cache)
    if (e.k.fn == fn && e.k.lds == lds && e.k.threads == threads && e.k.dev == dev) return e.nb;
  if (lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    set_error("occ_blocks_per_cu: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    return -1;
  }
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds);
  if (e != hipSuccess) { set_error(std::string("hipOccupancyMaxActiveBlocksPerMultiprocessor failed: ") + hipGetErrorString(e)); return -1; }
  cache.push_back({{fn, lds, threads, dev}, std::max(1, nb)});
  return std::max(1, nb);
}

int device_cus() {
  static const int v = [] {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    return cus;
  }();
  return v;
}

int resident_blocks(const void* fn, int threads, size_t lds) {
  const int nb = occ_blocks_per_cu(fn, threads, lds);
  return nb < 0 ? -1 : nb * device_cus();
}

int ensure_dynamic_lds(const void* fn, size_t bytes) {
  struct Ent { const void* fn; int dev; };
  static std::mutex mu;
  static std::vector<Ent> done;
  int dev = 0;
  DQ_HIP_OK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  for (const Ent& e : done)
    if (e.fn == fn && e.dev == dev) return 0;
  DQ_HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  done.push_back({fn, dev});
  return 0;
}
}  // namespace dq

using namespace dq;

extern "C" {

const char* dq_last_error(void) { return g_err.c_str(); }
int dq_abi_version(void) { return DQ_ABI_VERSION; }

dq_plan* dq_plan_create_ex(int dim, int n_mults, const int* dim_mults, int mz, int num_timesteps, int attn_cond_channels) {
  dq_plan* h = new dq_plan();
  std::string err = build_plan(h->plan, dim, n_mults, dim_mults, mz, num_timesteps, attn_cond_channels);
  if (!err.empty()) {
    set_error("dq_plan_create: " + err);
    delete h;
    return nullptr;
  }
  return h;
}
dq_plan* dq_plan_create(int dim, int n_mults, const int* dim_mults, int mz, int num_timesteps) {
  return dq_plan_create_ex(dim, n_mults, dim_mults, mz, num_timesteps, 1);
}
int dq_plan_attn_cond_channels(const dq_plan* plan) { return plan ? plan->plan.ms1_channels : -1; }

void dq_plan_destroy(dq_plan* plan) {
  if (!plan) return;
  if (plan->dev.ss_w_off) (void)hipFree(plan->dev.ss_w_off);
  if (plan->dev.ss_b_off) (void)hipFree(plan->dev.ss_b_off);
  plan->step.destroy();
  if (plan->side_stream) {
    (void)hipStreamDestroy(plan->side_stream);
    for (auto& e : plan->events) if (e) (void)hipEventDestroy(e);
  }
  delete plan;
}

int dq_plan_num_params(const dq_plan* plan) { return (int)plan->plan.params.size(); }
int64_t dq_plan_param_floats(const dq_plan* plan) { return plan->plan.total_floats; }

int dq_plan_param_info(const dq_plan* plan, int i, char* name, int name_cap, int64_t* offset, int* ndim, int64_t* shape) {
  DQ_REQUIRE(plan && i >= 0 && i < (int)plan->plan.params.size(), "dq_plan_param_info: index out of range");
  const ParamInfo& pi = plan->plan.params[i];
  DQ_REQUIRE((int)pi.name.size() + 1 <= name_cap, "dq_plan_param_info: name buffer too small");
  std::strcpy(name, pi.name.c_str());
  *offset = pi.offset;
  *ndim = pi.ndim;
  for (int k = 0; k < 4; ++k) shape[k] = pi.shape[k];
  return 0;
}

static_assert(FINAL_IDENTITY == DQ_FINAL_IDENTITY && FINAL_SOFTPLUS == DQ_FINAL_SOFTPLUS, "FinalAct mirrors include/dq_hip.h");
int dq_plan_set_final_act(dq_plan* plan, int act) {
  DQ_REQUIRE(plan, "dq_plan_set_final_act: null plan");
  DQ_REQUIRE(act == DQ_FINAL_IDENTITY || act == DQ_FINAL_SOFTPLUS,
             "dq_plan_set_final_act: act must be 0 (DQ_FINAL_IDENTITY) or 1 (DQ_FINAL_SOFTPLUS), got " + std::to_string(act));
  // a captured sampling step has the head's kernels baked in: never replay one captured under the other activation
  plan->step.drop();
  plan->plan.final_act = act;
  return 0;
}
int dq_plan_final_act(const dq_plan* plan) { return plan ? plan->plan.final_act : -1; }

int64_t dq_unet_workspace_bytes(dq_plan* plan, int B, int RT, int training) {
  if (!plan || B < 0 || RT < 0) return -1;
  Arena a;
  layout_arena(plan->plan, B, RT, a);
  return (int64_t)sizeof(float) * a.floats * (training ? 2 : 1);
}

int dq_q_sample(const float* alpha_bars_dev, const float* x0, const int64_t* t, const float* noise, float* x_t, int B,
                int64_t per_sample, int normalize_x0, void* stream) {
  return launch_q_sample(alpha_bars_dev, x0, t, noise, x_t, B, per_sample, normalize_x0, (hipStream_t)stream);
}

int dq_unet_fwd(dq_plan* plan, const float* params, const float* rope_freqs, const float* x, const int64_t* t, int t_scalar,
                const float* init_cond, const float* attn_cond, float cond_mul, float cond_add, float* out, int save_for_bwd,
                void* workspace, int64_t workspace_bytes, int B, int RT, void* stream) {
  DQ_REQUIRE(plan && params && x && init_cond && attn_cond && out && workspace, "dq_unet_fwd: null argument");
  DQ_REQUIRE(B > 0 && RT > 0, "dq_unet_fwd: B and RT must be positive");
  DQ_TRY(ensure_arena(plan, B, RT));
  DQ_REQUIRE(workspace_bytes >= (int64_t)sizeof(float) * plan->arena.floats, "dq_unet_fwd: workspace too small");
  Ctx c{plan->plan, plan->arena, params, (float*)workspace, nullptr, nullptr, B, RT, (hipStream_t)stream};
  c.save = save_for_bwd != 0;
  return unet_forward(c, rope_freqs, x, t, t_scalar, init_cond, attn_cond, cond_mul, cond_add, plan->dev, out);
}

int dq_unet_bwd(dq_plan* plan, const float* params, const float* rope_freqs, const float* init_cond, float cond_mul,
                float cond_add, const float* grad_out, float* grads, float* grad_x, void* workspace, int64_t workspace_bytes,
                int B, int RT, void* stream) {
  DQ_REQUIRE(plan && params && init_cond && grad_out && grads && workspace, "dq_unet_bwd: null argument");
  DQ_TRY(ensure_arena(plan, B, RT));
  DQ_REQUIRE(workspace_bytes >= 2 * (int64_t)sizeof(float) * plan->arena.floats, "dq_unet_bwd: workspace too small (training=1)");
  float* W = (float*)workspace;
  Ctx c{plan->plan, plan->arena, params, W, W + plan->arena.floats, grads, B, RT, (hipStream_t)stream};
  c.owner = plan->no_side ? nullptr : plan;
  plan->twin_zeroed = nullptr;  // (only a forked forward of the SAME dq_train_step call clears the twin ahead of its backward)
  return unet_backward(c, rope_freqs, init_cond, cond_mul, cond_add, plan->dev, grad_out, grad_x);
}

int dq_mse_loss_fwd_bwd(const float* eps, const float* noise, float* loss_out, float* grad_out, float* scratch, int64_t n,
                        void* stream) {
  DQ_REQUIRE(eps && noise && loss_out && scratch, "dq_mse_loss_fwd_bwd: null argument");
  LossTarget tg;
  tg.z = noise;
  return launch_mse_fwd_bwd(eps, tg, loss_out, grad_out, scratch, 1, n, (hipStream_t)stream);
}

int dq_ms1_loss_fwd_bwd(const float* pred, const float* x_t, const float* ms1_cond, float cond_mul, float cond_add,
                        const float* loss_weight_dev, const int64_t* t, float ms1_loss_weight, float* loss_inout, float* grad_inout,
                        float* scratch, int B, int RT, int MZ, void* stream) {
  DQ_REQUIRE(pred && ms1_cond && loss_inout && scratch, "dq_ms1_loss_fwd_bwd: null argument");
  DQ_REQUIRE(ms1_loss_weight > 0.f && ms1_loss_weight <= 1.f, "dq_ms1_loss_fwd_bwd: ms1_loss_weight must lie in (0, 1]");
  // (this entry has no plan: ms1_cond is the (B, RT) chromatogram the term is defined on; a multi-channel MS1 has no such term yet)
  return launch_ms1_loss(pred, x_t, ms1_cond, cond_mul, cond_add, loss_weight_dev, t, ms1_loss_weight, B, RT, MZ, grad_inout, loss_inout,
                         scratch, (hipStream_t)stream);
}

int dq_mse_loss_weighted_fwd_bwd(const float* pred, const float* target, float target_mul, float target_add,
                                 const float* loss_weight_dev, const int64_t* t, float* loss_out, float* grad_out, float* scratch,
                                 int B, int64_t per_sample, void* stream) {
  DQ_REQUIRE(pred && target && loss_weight_dev && t && loss_out && scratch, "dq_mse_loss_weighted_fwd_bwd: null argument");
  DQ_REQUIRE(B > 0 && per_sample > 0, "dq_mse_loss_weighted_fwd_bwd: B and per_sample must be positive");
  LossTarget tg;
  tg.z = target; tg.tm = target_mul; tg.ta = target_add; tg.lw = loss_weight_dev; tg.t = t;
  return launch_mse_fwd_bwd(pred, tg, loss_out, grad_out, scratch, B, per_sample, (hipStream_t)stream);
}

// The four AdamW entries: one launch_adamw (k_adamw.hip), the host's scalars or the device's, with or without the average
static AdamwStep adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch, float grad_scale,
                            float max_norm, double beta1, double beta2, double eps, double weight_decay, float* gnorm_out) {
  AdamwStep a;
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.n = n; a.partials = scratch; a.gscale = grad_scale; a.max_norm = max_norm;
  a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.wd = weight_decay; a.gnorm_out = gnorm_out;
  return a;
}

int dq_adamw_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch,
                       float grad_scale, float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                       int step, float* gnorm_out, void* stream) {
  DQ_REQUIRE(params && grads && exp_avg && exp_avg_sq && scratch, "dq_adamw_clip_step: null argument");
  AdamwStep a = adamw_step(params, grads, exp_avg, exp_avg_sq, n, scratch, grad_scale, max_norm, beta1, beta2, eps, weight_decay, gnorm_out);
  a.lr = lr; a.step = step;
  return launch_adamw(a, (hipStream_t)stream);
}

int dq_adamw_clip_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch, float grad_scale,
                           float max_norm, const float* lr_dev, double beta1, double beta2, double eps, double weight_decay, int* step_dev,
                           float* gnorm_out, void* stream) {
  DQ_REQUIRE(params && grads && exp_avg && exp_avg_sq && scratch && lr_dev && step_dev, "dq_adamw_clip_step_dev: null argument");
  AdamwStep a = adamw_step(params, grads, exp_avg, exp_avg_sq, n, scratch, grad_scale, max_norm, beta1, beta2, eps, weight_decay, gnorm_out);
  a.lr_dev = lr_dev; a.step_dev = step_dev;
  return launch_adamw(a, (hipStream_t)stream);
}

int dq_adamw_clip_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch,
                           float grad_scale, float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                           int step, float* gnorm_out, float* ema, float ema_decay, int ema_warmup, void* stream) {
  DQ_REQUIRE(params && grads && exp_avg && exp_avg_sq && scratch, "dq_adamw_clip_ema_step: null argument");
  DQ_REQUIRE(ema, "adamw + ema: the EMA buffer is null");
  AdamwStep a = adamw_step(params, grads, exp_avg, exp_avg_sq, n, scratch, grad_scale, max_norm, beta1, beta2, eps, weight_decay, gnorm_out);
  a.lr = lr; a.step = step; a.ema = ema; a.ema_decay = ema_decay; a.ema_warmup = ema_warmup;
  return launch_adamw(a, (hipStream_t)stream);
}

int dq_adamw_clip_ema_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch,
                               float grad_scale, float max_norm, const float* lr_dev, double beta1, double beta2, double eps,
                               double weight_decay, int* step_dev, float* gnorm_out, float* ema, float ema_decay, int ema_warmup,
                               void* stream) {
  DQ_REQUIRE(params && grads && exp_avg && exp_avg_sq && scratch && lr_dev && step_dev, "dq_adamw_clip_ema_step_dev: null argument");
  DQ_REQUIRE(ema, "adamw + ema: the EMA buffer is null");
  AdamwStep a = adamw_step(params, grads, exp_avg, exp_avg_sq, n, scratch, grad_scale, max_norm, beta1, beta2, eps, weight_decay, gnorm_out);
  a.lr_dev = lr_dev; a.step_dev = step_dev; a.ema = ema; a.ema_decay = ema_decay; a.ema_warmup = ema_warmup;
  return launch_adamw(a, (hipStream_t)stream);
}

int dq_set_option(const char* key, int64_t value) {
  const int i = option_index(key);
  DQ_REQUIRE(i >= 0, "dq_set_option: unknown key");
  set_option(i, value);
  return 0;
}
int64_t dq_get_option(const char* key) {
  const int i = option_index(key);
  if (i < 0) { set_error("dq_get_option: unknown key"); return INT64_MIN; }
  return option((Option)i);
}
int64_t dq_get_option_effective(const char* key) {
  switch (option_index(key)) {
    case OPT_LA_SMALL_MIN_ROWS: return la_small_min_rows();
    case OPT_LA_ROWS_BWD_MIN_ROWS: return la_rows_bwd_min_rows();
    case OPT_RES_ROWS_BWD_MIN_ROWS: return res_rows_bwd_min_rows();
    default: set_error("dq_get_option_effective: unknown key"); return -1;
  }
}

int dq_debug_side_tail_store(dq_plan* plan, float* addr, float value, int delay_us) {
  DQ_REQUIRE(plan && delay_us >= 0 && delay_us <= 100000, "dq_debug_side_tail_store: null plan / delay out of range");
  plan->debug_tail_addr = addr; plan->debug_tail_value = value; plan->debug_tail_us = delay_us;
  return 0;
}

int dq_plan_set_side_stream(dq_plan* plan, int on) {
  DQ_REQUIRE(plan, "dq_plan_set_side_stream: null plan");
  plan->no_side = on ? false : true;
  return 0;
}

int dq_train_step(dq_plan* plan, const float* params, const float* rope_freqs, const float* alpha_bars_dev, const float* x0,
                  const float* ms2_cond, const float* ms1_cond, const int64_t* t, const float* noise, int auto_normalize,
                  int pred_type, const float* loss_weight_dev, float ms1_loss_weight, float* grads, float* loss_out, void* workspace,
                  int64_t workspace_bytes, int B, int RT, void* stream) {
  // (the objective first: these two refusals need no operand)
  DQ_REQUIRE(pred_type == DQ_PRED_EPS || pred_type == DQ_PRED_X0 || pred_type == DQ_PRED_V, "dq_train_step: Unknown pred_type");
  DQ_REQUIRE(pred_type != DQ_PRED_V || !(ms1_loss_weight > 0.f),
             "dq_train_step: ms1_loss_weight > 0 with pred_type v_prediction is not built (DESIGN.md section 12 defines the MS1 term for eps and x0 only)");
  DQ_REQUIRE(plan && params && alpha_bars_dev && x0 && ms2_cond && ms1_cond && t && noise && grads && loss_out && workspace,
             "dq_train_step: null argument");
  DQ_REQUIRE(pred_type != DQ_PRED_X0 || loss_weight_dev, "dq_train_step: pred_type x0 needs the loss-weight (SNR) table");
  DQ_REQUIRE(B > 0 && RT > 0, "dq_train_step: B and RT must be positive");
  DQ_REQUIRE(ms1_loss_weight >= 0.f && ms1_loss_weight <= 1.f, "dq_train_step: ms1_loss_weight must lie in [0, 1]");
  DQ_REQUIRE(ms1_loss_weight == 0.f || plan->plan.ms1_channels == 1,
             "dq_train_step: ms1_loss_weight > 0 with attn_cond_channels > 1 is not built (the MS1 term is defined on a chromatogram)");
  plan->twin_zeroed = nullptr;  // (a step that failed between its forked forward and its backward must not leave "already cleared" behind)
  DQ_TRY(ensure_arena(plan, B, RT));
  const Arena& a = plan->arena;
  DQ_REQUIRE(workspace_bytes >= 2 * (int64_t)sizeof(float) * a.floats, "dq_train_step: workspace too small (training=1)");
  hipStream_t s = (hipStream_t)stream;
  float* W = (float*)workspace;
  Ctx c{plan->plan, a, params, W, W + a.floats, grads, B, RT, s};
  c.owner = plan->no_side ? nullptr : plan;
  const int64_t per = (int64_t)RT * plan->plan.mz;
  const float cm = auto_normalize ? 2.f : 1.f, ca = auto_normalize ? -1.f : 0.f;
  const bool qs_fused_on = !DQ_DEV_FLAG("DQ_NO_QSAMPLE_FUSE", '1');  // (dev switch)
  Ctx::QSample qs;
  qs.alpha_bars = alpha_bars_dev; qs.x0 = x0; qs.t = t; qs.noise = noise; qs.normalize = auto_normalize; qs.per = per;
  if (qs_fused_on && ms1_loss_weight == 0.f) c.qsample = &qs;  // model.py:349-352 (the MS1 term reads x_t: it keeps the launch)
  else DQ_TRY(launch_q_sample(alpha_bars_dev, x0, t, noise, c.w(a.xa), B, per, auto_normalize, s));
  const bool head_loss_on = !DQ_DEV_FLAG("DQ_NO_HEAD_LOSS", '1');  // (dev switch)
  Ctx::HeadLoss hl;
  if (head_loss_on && pred_type != DQ_PRED_X0 && ms1_loss_weight == 0.f) {
    hl.z = noise; hl.grad_out = c.w(a.xb); hl.part = c.w(a.head_part); hl.gscale = 2.0f / (float)(B * per);  // (launch_mse_fwd_bwd's scale)
    if (pred_type == DQ_PRED_V) {  // the target sa_b noise - sb_b (x0 cm + ca) is formed in the head launch (k_mse_fwd_bwd<MseV>'s arithmetic)
      hl.x0 = x0; hl.alpha_bars = alpha_bars_dev; hl.t = t; hl.lw = loss_weight_dev; hl.tm = cm; hl.ta = ca;
    }
    c.head_loss = &hl;
  }
  DQ_TRY(unet_forward(c, rope_freqs, c.w(a.xa), t, 0, ms2_cond, ms1_cond, cm, ca, plan->dev, c.w(a.eps)));   // model.py:359
  // the gradient twin is zeroed inside unet_backward, so the loss gradient goes to a forward-arena buffer (xb)
  if (hl.done) {  // (loss and its gradient came with the forward's last launch; the sum of the partials rides on the side stream: unet_backward)
    c.loss_sum.partials = hl.part; c.loss_sum.count = hl.nparts; c.loss_sum.scale = 1.0f / (float)(B * per); c.loss_sum.out = loss_out;
  } else {  // model.py:361 / 372-376, 404 / DESIGN.md section 35
    // (eps on the fork: the sum of the partials -> loss_out rides on the side stream, unet_backward)
    const bool defer = pred_type == DQ_PRED_EPS && c.owner && ms1_loss_weight == 0.f && tail_fork_enabled();
    int nparts = 0;
    DQ_TRY(launch_mse_fwd_bwd(c.w(a.eps), loss_target(pred_type, x0, noise, alpha_bars_dev, cm, ca, loss_weight_dev, t), loss_out, c.w(a.xb),
                              c.w(a.partials), B, per, s, defer ? &nparts : nullptr));
    if (defer) { c.loss_sum.partials = c.w(a.partials); c.loss_sum.count = nparts; c.loss_sum.scale = 1.0f / (float)(B * per); c.loss_sum.out = loss_out; }
  }
  if (ms1_loss_weight > 0.f)  // model.py:364-371 / 379-386, 398-402 (semantics: DESIGN.md section 12)
    DQ_TRY(launch_ms1_loss(c.w(a.eps), pred_type == DQ_PRED_X0 ? nullptr : c.w(a.xa), ms1_cond, cm, ca,
                           pred_type == DQ_PRED_X0 ? loss_weight_dev : nullptr, t, ms1_loss_weight, B, RT, plan->plan.mz, c.w(a.xb), loss_out,
                           c.w(a.ms1_scratch), s));
  DQ_TRY(unet_backward(c, rope_freqs, ms2_cond, cm, ca, plan->dev, c.w(a.xb), nullptr));
  return 0;
}

// The forward-only counterpart of dq_train_step: q_sample, the network forward in its no-save mode (the inference arena alone: no gradient
// twin, no side queue, dq_plan::twin_zeroed untouched), then the per-window MSE.  The slice sums live in the arena's second sampling buffer
// (xb: B * per floats rounded up to 64, which an inference forward never touches); a window of fewer than 8192 elements needs one
// double, so only a B * per below 64 with per == 1 could fall short, and the launcher checks the size it is given.
int dq_eval_step(dq_plan* plan, const float* params, const float* rope_freqs, const float* alpha_bars_dev, const float* x0,
                 const float* ms2_cond, const float* ms1_cond, const int64_t* t, const float* noise, int auto_normalize, int pred_type,
                 const float* loss_weight_dev, float* loss_out, float* per_window_out, void* workspace, int64_t workspace_bytes, int B, int RT,
                 void* stream) {
  DQ_REQUIRE(pred_type == DQ_PRED_EPS || pred_type == DQ_PRED_X0 || pred_type == DQ_PRED_V, "dq_eval_step: Unknown pred_type");
  DQ_REQUIRE(plan && params && alpha_bars_dev && x0 && ms2_cond && ms1_cond && t && noise && loss_out && per_window_out && workspace,
             "dq_eval_step: null argument");
  DQ_REQUIRE(pred_type != DQ_PRED_X0 || loss_weight_dev, "dq_eval_step: pred_type x0 needs the loss-weight (SNR) table");
  DQ_REQUIRE(B > 0 && RT > 0, "dq_eval_step: B and RT must be positive");
  DQ_TRY(ensure_arena(plan, B, RT));
  const Arena& a = plan->arena;
  DQ_REQUIRE(workspace_bytes >= (int64_t)sizeof(float) * a.floats, "dq_eval_step: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Ctx c{plan->plan, a, params, (float*)workspace, nullptr, nullptr, B, RT, s};
  c.save = false;
  const int64_t per = (int64_t)RT * plan->plan.mz;
  const float cm = auto_normalize ? 2.f : 1.f, ca = auto_normalize ? -1.f : 0.f;
  DQ_TRY(launch_q_sample(alpha_bars_dev, x0, t, noise, c.w(a.xa), B, per, auto_normalize, s));                 // model.py:349-352
  DQ_TRY(unet_forward(c, rope_freqs, c.w(a.xa), t, 0, ms2_cond, ms1_cond, cm, ca, plan->dev, c.w(a.eps)));  // model.py:359
  const int64_t slice_bytes = (int64_t)sizeof(float) * ((B * per + 63) / 64 * 64);
  // model.py:361 / 372-376 / DESIGN.md section 35: the objective's target, weighted as in training
  return launch_mse_per_window(c.w(a.eps), loss_target(pred_type, x0, noise, alpha_bars_dev, cm, ca, loss_weight_dev, t), per_window_out, loss_out,
                               c.w(a.xb), slice_bytes, B, 1, per, s);
}

int64_t dq_mse_per_window_scratch_bytes(int B, int64_t per) { return mse_per_window_scratch_bytes(B, per); }

int dq_mse_per_window(const float* out, const float* target, float tm, float ta, const float* lw, const int64_t* t, float* per_window_out,
                      float* loss_out, void* scratch, int B, int64_t per, void* stream) {
  DQ_REQUIRE(B > 0 && per > 0, "dq_mse_per_window: B and per must be positive");
  LossTarget tg;
  tg.z = target; tg.tm = tm; tg.ta = ta; tg.lw = lw; tg.t = t;
  return launch_mse_per_window(out, tg, per_window_out, loss_out, scratch, mse_per_window_scratch_bytes(B, per), B, 1, per, (hipStream_t)stream);
}

int dq_mse_loss_v_fwd_bwd(const float* pred, const float* x0, const float* noise, const float* alpha_bars_dev, float tm, float ta, const float* lw,
                          const int64_t* t, float* loss_out, float* grad_out, float* scratch, int B, int64_t per, void* stream) {
  DQ_REQUIRE(pred && x0 && noise && alpha_bars_dev && t && loss_out && scratch, "dq_mse_loss_v_fwd_bwd: null argument");
  DQ_REQUIRE(B > 0 && per > 0, "dq_mse_loss_v_fwd_bwd: B and per must be positive");
  return launch_mse_fwd_bwd(pred, loss_target(DQ_PRED_V, x0, noise, alpha_bars_dev, tm, ta, lw, t), loss_out, grad_out, scratch, B, per,
                            (hipStream_t)stream);
}

int dq_mse_per_window_v(const float* out, const float* x0, const float* noise, const float* alpha_bars_dev, float tm, float ta, const float* lw,
                        const int64_t* t, float* per_window_out, float* loss_out, void* scratch, int B, int64_t per, void* stream) {
  DQ_REQUIRE(B > 0 && per > 0, "dq_mse_per_window_v: B and per must be positive");
  return launch_mse_per_window(out, loss_target(DQ_PRED_V, x0, noise, alpha_bars_dev, tm, ta, lw, t), per_window_out, loss_out, scratch,
                               mse_per_window_scratch_bytes(B, per), B, 1, per, (hipStream_t)stream);
}

int dq_q_sample_repeats(const float* alpha_bars_dev, const float* x0, const int64_t* t, const float* noise, const uint64_t* seed_dev,
                        const int64_t* window_ids_dev, int first_draw, float* x_t, int B, int repeats, int64_t per_window, int normalize_x0,
                        void* stream) {
  const NoiseStack st{repeats, window_ids_dev, seed_dev, first_draw};
  return launch_q_sample(alpha_bars_dev, x0, t, noise, x_t, B, per_window, normalize_x0, (hipStream_t)stream, &st);
}

int dq_mse_per_window_repeats(const float* out, const float* target, int target_windows, float tm, float ta, const uint64_t* seed_dev,
                              const int64_t* window_ids_dev, int first_draw, const float* lw, const int64_t* t, float* per_window_out,
                              float* loss_out, void* scratch, int B, int repeats, int64_t per, void* stream) {
  DQ_REQUIRE(B > 0 && repeats > 0 && (int64_t)repeats * B <= 65535 && per > 0, "dq_mse_per_window_repeats: need B, repeats, per > 0 and repeats * B <= 65535");
  LossTarget tg;
  tg.kind = target ? TargetKind::READ : TargetKind::DRAWN;
  tg.z = target; tg.tm = tm; tg.ta = ta; tg.lw = lw; tg.t = t;
  tg.stacked = true; tg.Bt = target_windows; tg.ids = window_ids_dev; tg.seed = seed_dev; tg.first_draw = first_draw;
  return launch_mse_per_window(out, tg, per_window_out, loss_out, scratch, mse_per_window_scratch_bytes(repeats * B, per), B, repeats, per,
                               (hipStream_t)stream);
}

int64_t dq_recon_metrics_scratch_bytes(int B, int RT, int MZ) { return recon_metrics_scratch_bytes(B, RT, MZ); }

int dq_recon_metrics(const float* pred, const float* target, float* out, void* scratch, int64_t scratch_bytes, int B, int RT, int MZ,
                     void* stream) {
  return launch_recon_metrics(pred, target, out, scratch, scratch_bytes, B, RT, MZ, (hipStream_t)stream);
}

}  // extern "C"
