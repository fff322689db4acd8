// What the sampling loops share (dq_sampler.hip): the refusals made before anything touches the device, the upload of a sampler's tables,
// the staging of seed and window ids for a captured step, the update behind a network forward, and the loop itself -- the captured step
// with its replay, and the eager steps.  The U-Net loop (dq_ddim_sample_solver) and the transformer loop (dq_tfm_sample, dq_tfm_sample.hip)
// differ in the forward they put in front of the update, literally: each hands the two functions below its StepForward, and in what it stages in front
// of the loop.  Internal: not installed.
#pragma once
#include "dq_common.h"
#include "dq_unet.h"  // StepUpdate, StepGraph
#include <functional>

namespace dq {

// What every step's update of one sampling call shares: the tables (extra: sigma per row, or the solver's c1), the x0 history of the 2M
// solver (updated in place), the clamp (0: off) and the shape.  guided: the forward ran at 2 B windows -- rows
// [0, B) under the caller's condition, rows [B, 2B) under the null -- and the update combines the two outputs with the scale w inside its
// kernel, over the B windows of the first half; x and the network output are then 2 * B * per floats each.
// The per-window statistics of a step (k_winstat.hip), run by launch_step_update between the forward and the update:
// rescale (guided calls): m_b of rescaled guidance at phi; q > 0: dynamic thresholding at that quantile with floor f and cap.  The scratch is
// dq_sample_stat_scratch_bytes(B, per) bytes at a fixed address; the update then runs in its per-window form over the table at its head.
struct StepStats {
  double phi = 0.0;
  float q = 0.f, floor = 1.f, cap = 0.f;
  void* scratch = nullptr; int64_t scratch_bytes = 0;
  bool rescale = false;
  bool on() const { return rescale || q > 0.f; }
};

struct StepUpdateArgs {
  StepUpdate kind;
  const float* coef; const float* extra;
  float* hist;
  float clip;
  int pred, B;  // pred: DQ_PRED_*
  int64_t per;
  bool guided = false;
  float w = 1.f;
  StepStats stats;
};

// The noise of the stochastic update: the windows' ids and the seed (device memory) and the draw index (the kernel adds the step counter)
struct StepNoise { const int64_t* ids; const uint64_t* seed; int draw; };

// The update of one step behind the network forward: x_out from x and the network output.  The row is `row` of the tables (the eager loop)
// or, with step_ptr, the one the device-side step counter names (the captured step: row 0).  eps_out (nullable): where the step's eps goes
// when it is not the network output itself; fused: the deterministic update went with the head launch (StepIO::fused_update), nothing is
// left to do.  Guided (u.guided): net_out is the conditional output, net_u the unconditional one, x_mirror (nullable) receives x_out's values
// as well (the unconditional half's x of the next forward), and eps_out (nullable) the guided eps; never fused (the head launch of window b
// cannot see the output of window B + b).  Both are null otherwise.
int launch_step_update(const StepUpdateArgs& u, const float* x, const float* net_out, const float* net_u, float* x_out, float* x_mirror,
                       float* eps_out, int row, const int* step_ptr, const StepNoise& z, bool fused, hipStream_t s);

// What a call's (eta, sampler, clip_x0) select.  clip_x0: the clamp as the kernels take it (0: off)
struct SamplerChoice { StepUpdate kind = StepUpdate::DDIM; bool sto = false, clip = false; float clip_x0 = 0.f; int pred = 0; };  // pred: DQ_PRED_*
// (clip: x0 is clamped by clip_x0 or thresholded -- either way the Solver family runs and the derived eps is the trajectory's)
// The refusals every sampling loop makes, in one order, before anything touches the device; `who` prefixes the messages.  args_ok: the
// caller's required pointers are all there; allow_v: DQ_PRED_V is a known objective for this caller (dq_ddim_sample_v).  threshold: the call
// asks for dynamic thresholding (dq_ddim_sample_adaptive), refused where clip_x0 is and selecting the update clip_x0 selects.
int sampler_check(const char* who, bool args_ok, float eta, int sampler, float clip_x0, const int32_t* timesteps_host, int num_steps,
                  bool have_seed, bool have_xT, int pred_type, bool allow_v, SamplerChoice* out, bool threshold = false);
// Forms the call's coefficient rows on the host and copies them to coef_dev (4 per step) and extra_dev (1 per step; nullable: not needed);
// returns after the copies are done (the host vectors are the function's own)
int sampler_upload_tables(const char* who, const float* alpha_bars_host, int T, const int32_t* ts, int num_steps, int sampler, const SamplerChoice& c,
                          float eta, float* coef_dev, float* extra_dev, hipStream_t s);
// Seed and window ids (null: 0 .. B-1) copied into the workspace, so that a new seed or other windows replay the same captured step; returns
// after the copies are done
int sampler_stage_noise(uint64_t* seed_stage, int64_t* ids_stage, const uint64_t* seed_dev, const int64_t* window_ids_dev, int B, hipStream_t s);

// One step's network forward on stream s, the one thing a loop brings of its own: the network output of x into net_out, at timestep and
// table row `row` (the eager loop) or, with step_ptr, at the ones the device-side step counter names (the captured step).  A forward that
// takes the update into its own launch writes the next x to x_out and sets *fused; want_eps: net_out is read behind the step (a trajectory).
using StepForward = std::function<int(const float* x, float* x_out, int row, const int* step_ptr, float* net_out, bool want_eps, bool* fused, hipStream_t s)>;
// What one call's steps run over.  xa: x_T on entry; upd.hist is xb: the 2M solver's x0 history, otherwise the other half of the ping-pong.
// clip: the x0 estimate is clamped (the derived eps goes to the trajectory, as for the x0 objective).  The rest is launch_sample_finish's.
struct SampleLoop {
  StepForward forward;
  StepUpdateArgs upd;
  float *xa, *eps;
  bool clip;
  int num_steps;
  const float* ms2_cond; float *out_x, *out_noise; int normalize;
};
// The captured step: unless `reusable` (the caller's g.exec && stored key == key) drops g's graph and captures forward, update (x in place,
// the staged noise at draw 0: the kernel adds the step counter) and launch_inc_step(step) on g.cap_stream; then num_steps replays on s and
// launch_sample_finish.  *captured: it captured anew and instantiated -- only then does the caller store its key, whatever is returned.
int replay_captured_step(StepGraph& g, bool reusable, const SampleLoop& L, int* step, const StepNoise& staged, hipStream_t s, bool* captured);
// The eager steps: x per step into its trajectory slot (copied back to xa), in place (the solvers) or ping-pong; eps into its trajectory slot
// or the scratch; the caller's ids and seed, step i drawing at index 1 + i; then launch_sample_finish.
int eager_steps(const SampleLoop& L, float* traj_x, float* traj_eps, const int64_t* window_ids_dev, const uint64_t* seed_dev, hipStream_t s);
}  // namespace dq
