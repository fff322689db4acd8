// Host-side state of one network instance: plan, device tables and the activation arena layout.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "dq_plan.h"

namespace dq {

constexpr int TBUF_FLOATS = 100;  // per-sample scratch of the time-embedding kernels (see k_time.hip)

struct DevTables {
  int64_t* ss_w_off = nullptr;  // [ss_total] offset of row r's 16 weights in the flat parameter buffer
  int64_t* ss_b_off = nullptr;  // [ss_total] offset of row r's bias
};

int launch_time_embed_fwd(const Plan& p, const DevTables& dt, const float* params, const int64_t* t, int t_scalar, float* tbuf,
                          float* ss, int B, const int* step_tab, const int* step_ptr, hipStream_t s);
int launch_ss_heads(const float* temb, const float* w, const float* bias, float* ss, int B, int m, hipStream_t s);
int launch_ss_heads_strided(const float* temb, const float* w, const float* bias, float* ss, int stride, int B, int m, hipStream_t s);
int launch_time_mlp_fwd(const float* w1, const float* b1, const float* w2, const float* b2, const int64_t* t, float* tbuf, int B,
                        hipStream_t s);
int launch_time_embed_bwd(const Plan& p, const DevTables& dt, const float* params, float* grads, float* tbuf, const float* dss,
                          int B, hipStream_t s);

// Activation arena: offsets (in floats) of every tensor the forward produces for a given (B, RT).  The backward's
// gradient of a tensor lives at the same offset in a second arena of the same size ("twin").
struct ResBuf {
  int64_t u1, a1, u2, out;
  int64_t gpart = 0, gpart_floats = 0;  // per-block norm-gain sums of the backward (k_res_bwd / k_res_bwd_cp / k_block_bwd)
  int64_t wpart = 0, wpart_floats = 0;  // per-workgroup slots of the backward that forms its weight gradients itself (k_res_bwd_wg); 0: not that path
};
struct LevelBuf {
  ResBuf r0, r1; int64_t la, la_pre, la_tmp, rs;
  int64_t cpart = 0, cpart_floats = 0;  // per-workgroup slots of the resample conv's backward (k_conv_bwd_wg); 0: not that path
};
struct WideResBuf { int64_t u1 = 0, a1 = 0, u2 = 0, out = 0; };  // (B, mid_c, P) each: a ResnetBlock of the wide bottleneck  // la_pre: saved pre-norm LA output; la_tmp: backward scratch (twin only)
struct Arena {
  int B = 0, RT = 0;
  int64_t floats = 0;       // total arena size
  int64_t zero_floats = 0;  // prefix whose gradient twin must be zeroed before a backward (the accumulated-into tensors)
  int64_t tbuf, ss, cat0, ms1n, ms1_u, ms1_a, ms1f, h0;
  std::vector<LevelBuf> downs, ups;
  int64_t mid_in, xn, qv, kk, o, lse, delta, attn_out, mid_back, eps, partials, head_part, loss, coef, xa, xb, wg, wg_floats, la_part, la_part_floats, ts_tab, step, c2_stage, c1_stage, wtmp, la_prep, wimg, timg, bb_part, bb_part_floats, ms1_scratch;
  int64_t ms1_wpart = 0, ms1_wpart_floats = 0;  // attn_cond_channels > 1: the slots of k_ms1_feat_wgrad
  // stochastic sampling (eta > 0; k_update.hip, k_noise.hip): sigma per step beside `coef`; the seed (uint64) and the window ids (B int64) staged at fixed
  // addresses for the captured step.  Last in the arena: every other offset is what it was without them.
  int64_t sigma = 0, seed_stage = 0, ids_stage = 0;
  ResBuf mid1, mid2, fin;
  // wide bottleneck (Plan::wide_mid): P = RT padded to a multiple of 4; every tensor below is (B, channels, P)
  int P = 0;
  WideResBuf wmid1, wmid2;
  int64_t w_mid_in = 0, w_xcol = 0, w_xn = 0, w_qv = 0, w_o = 0, w_attn_out = 0, w_stats = 0, w_gemm_part = 0, w_gemm_part_floats = 0;
};
void layout_arena(const Plan& p, int B, int RT, Arena& a);

// The update of one sampling step (dq_sampler.hip): DDIM is the deterministic update (eta == 0; the reference and the strided table alike), in
// the head launch or k_update.hip's Ddim family behind it; STOCHASTIC its Sto family (eta > 0); SOLVER_1 / SOLVER_2M its Solver family without / with the x0
// history (a clamped x0 at first order / DPM-Solver++(2M))
enum class StepUpdate { DDIM, STOCHASTIC, SOLVER_1, SOLVER_2M };

// Everything a captured sampling step has baked into its kernel arguments or its dispatch.  clip: the clamp of the Solver update (0: off);
// guidance: the scale the guided update takes by value (< 0: not a guided step; B is then the caller's, not the doubled, batch);
// opt_epoch: options_epoch() at capture time (a dq_set_option call may change the dispatch)
struct StepKey {
  const void* params = nullptr; const void* rope = nullptr; const void* ws = nullptr;
  int B = 0, RT = 0, normalize = -1, pred = -1;
  StepUpdate update = StepUpdate::DDIM;
  float clip = 0.f;
  float guidance = -1.f;
  // the per-window statistics step: phi, quantile, cap by value and the scratch by address (all 0: none)
  double rescale = 0.0; float quantile = 0.f, cap = 0.f; const void* stat_scratch = nullptr;
  // the consistency pass: members per group, mode (0: none) and blend by value
  int group_size = 1, consistency = 0; float strength = 1.f;
  unsigned opt_epoch = 0;
  bool operator==(const StepKey& o) const {
    return params == o.params && rope == o.rope && ws == o.ws && B == o.B && RT == o.RT && normalize == o.normalize && pred == o.pred &&
           update == o.update && clip == o.clip && guidance == o.guidance && rescale == o.rescale && quantile == o.quantile && cap == o.cap &&
           stat_scratch == o.stat_scratch && group_size == o.group_size && consistency == o.consistency && strength == o.strength &&
           opt_epoch == o.opt_epoch;
  }
};

// hipGraph of ONE sampling step (network forward + update + step counter), replayed num_steps times; valid while every pointer baked into
// its kernel arguments is unchanged (the owner's key).  cap_stream: capture-only (the caller's may be the uncapturable legacy default stream)
struct StepGraph {
  hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; hipStream_t cap_stream = nullptr;
  void drop() {  // drops the captured step: the next graph call captures again
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
  }
  void destroy() { drop(); if (cap_stream) { (void)hipStreamDestroy(cap_stream); cap_stream = nullptr; } }
};

}  // namespace dq

struct dq_plan {
  dq::Plan plan;
  dq::DevTables dev;
  float* alpha_bars_dev = nullptr;          // (T) fp32, for q_sample
  std::vector<float> alpha_bars_host;
  dq::Arena arena;                           // cached for the last (B, RT)
  dq::StepGraph step;    // the captured sampling step
  dq::StepKey step_key;  // what it was captured for
  // side stream for the weight-gradient kernels of the backward (forked / joined with events from this ring)
  static constexpr int NUM_EVENTS = 256;
  hipStream_t side_stream = nullptr;
  hipEvent_t events[NUM_EVENTS] = {};
  unsigned ev_next = 0;
  bool side_used = false;
  const void* twin_zeroed = nullptr;  // the gradient twin a forked forward (dq_train_step) cleared on the side stream; consumed by unet_backward
  float* debug_tail_addr = nullptr; float debug_tail_value = 0.f; int debug_tail_us = 0;  // dq_debug_side_tail_store (test hook)
  bool no_side = false;  // dq_plan_set_side_stream(plan, 0): weight-gradient launches on the caller's stream (captured train steps)
};
