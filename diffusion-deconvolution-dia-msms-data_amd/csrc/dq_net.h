// What the entry points outside the network file need of it (dq_api.hip, dq_sampler.hip): the context a pass runs in and the passes
// themselves (dq_unet.hip).  Internal: not installed.
#pragma once
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_unet.h"

#include <functional>
#include <vector>

namespace dq {

struct Ctx {
  const Plan& p;
  const Arena& ar;
  const float* P;   // params
  float* W;         // forward arena
  float* G;         // gradient twin of the arena (null in inference)
  float* dP;        // flat grads
  int B, RT;
  hipStream_t s;
  bool save = true;  // keep what the backward needs (pre-norm conv outputs, LinearAttention pre-norm output)
  dq_plan* owner = nullptr;  // side stream + events for the weight-gradient kernels (null => everything on s)
  struct LaDefer { LaReduceItem items[LA_REDUCE_MAX]; int count = 0; int64_t cursor = 0; };
  LaDefer* la_defer = nullptr;  // set by unet_backward: LinearAttention slot reductions collected for one launch at the end
  // set by unet_backward: the side-stream launches (weight gradients, norm-gain reduces) are collected and issued by side_flush
  // behind ONE event per group instead of one per ResnetBlock / conv (an event record costs ~4 us on the main stream: 29 + 14
  // of them were 0.13 ms per step); everything they read is final when it is queued and stays untouched until the join
  // forks: the item runs behind the group's fork event (all but the ResnetBlock partial-sum reduce, which opens no fork of its own: it goes
  // to the side stream if that exists, else to the main stream)
  struct SideFn { std::function<int(hipStream_t)> fn; bool forks = true; };
  std::vector<SideFn>* side_defer = nullptr;
  // set by unet_backward: the slot reductions of the ResnetBlock backwards that form their own weight gradients (k_res_bwd_wg),
  // collected for ONE launch at the end of the pass (null: each is reduced right behind its launch)
  std::vector<ResWgReduce>* wg_defer = nullptr;
  // sampling (dq_ddim_sample): the DDIM update rides in the head launch (x_out may alias x_t), and the step-invariant MS1 feature path
  // (unet1d.py:1120-1130) + to_k + RoPE(k) were computed once before the loop
  struct StepIO { const float* x_t = nullptr; float* x_out = nullptr; const float* coef = nullptr; const int* step_ptr = nullptr; int pred = 0;
                  bool prologue = false; bool fused_update = false; bool want_eps = true; };  // prologue: unet_prepare and the MS1 path ran before the loop
  StepIO* step_io = nullptr;
  // dq_train_step: the scalar loss (sum of the MSE kernel's partials) is needed by nobody on the gradient chain: it rides on the side stream
  struct LossSum { const float* partials = nullptr; int count = 0; float scale = 0.f; float* out = nullptr; };
  LossSum loss_sum;
  // dq_train_step: final_conv, the squared error against `z` and the first two steps of the backward (d eps -> grad_out, d fin.out) ride in
  // the final block's launch when it can take them (k_level_fwd's training head); `done` / `nparts` tell the caller
  struct HeadLoss {
    const float* z = nullptr; float* grad_out = nullptr; float* part = nullptr; float gscale = 0.f; int nparts = 0; bool done = false;
    // the v objective (x0 set): z is the noise, the target is formed in the launch (LevelFwd::vt_*)
    const float* x0 = nullptr; const float* alpha_bars = nullptr; const int64_t* t = nullptr; const float* lw = nullptr; float tm = 1.f, ta = 0.f;
  };
  HeadLoss* head_loss = nullptr;
  // dq_train_step: x_t = q_sample(x0, t, noise) (model.py:349-352) is formed by level 0's INIT stage when that stage runs (`x` of unet_forward is
  // then only the buffer x_t would have gone to); otherwise unet_forward launches k_q_sample into `x` first
  struct QSample { const float* alpha_bars = nullptr; const float* x0 = nullptr; const int64_t* t = nullptr; const float* noise = nullptr; int normalize = 0; int64_t per = 0; };
  const QSample* qsample = nullptr;
  float* w(int64_t off) const { return W + off; }
  float* g(int64_t off) const { return G + off; }
  const float* prm(int64_t off) const { return P + off; }
  float* dprm(int64_t off) const { return dP + off; }
};

#define DQ_TRY(expr)            \
  do {                          \
    int _rc = (expr);           \
    if (_rc) return _rc;        \
  } while (0)

// Lays out the arena for (B, RT) and, on the first call of a plan, uploads the offset tables of the scale/shift heads
int ensure_arena(dq_plan* plan, int B, int RT);
int ensure_dev_tables(dq_plan* plan);  // (the tables alone)
int unet_forward(const Ctx& c, const float* rope, const float* x, const int64_t* t, int t_scalar, const float* init_cond,
                 const float* attn_cond, float cm, float ca, const DevTables& dt, float* out, const int* step_tab = nullptr,
                 const int* step_ptr = nullptr);
int unet_backward(const Ctx& c_in, const float* rope, const float* init_cond, float cm, float ca, const DevTables& dt,
                  const float* grad_out, float* grad_x);
bool tail_fork_enabled();
// The step-invariant part of a sampling call, once in front of its steps; *ran: it did (StepIO::prologue), false for the wide bottleneck
int unet_sample_prologue(const Ctx& c, const float* ms1, float cm, float ca, const float* rope, bool* ran);

}  // namespace dq
