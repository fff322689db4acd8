// What the sampling loops share (dq_sampler.hip): the refusals made before anything touches the device, the upload of a sampler's tables,
// the staging of seed and window ids for a captured step, and the update behind a network forward.  The U-Net loop (dq_ddim_sample_solver)
// and the transformer loop (dq_tfm_sample, dq_tfm_sample.hip) differ in the forward they put in front of it.  Internal: not installed.
#pragma once
#include "dq_common.h"
#include "dq_unet.h"  // StepUpdate

namespace dq {

// What every step's update of one sampling call shares: the tables (extra: sigma per row, or the solver's c1), the x0 history of the 2M
// solver (updated in place), the clamp (0: off) and the shape
struct StepUpdateArgs {
  StepUpdate kind;
  const float* coef; const float* extra;
  float* hist;
  float clip;
  int px0, B;
  int64_t per;
};

// The noise of the stochastic update: the windows' ids and the seed (device memory) and the draw index (the kernel adds the step counter)
struct StepNoise { const int64_t* ids; const uint64_t* seed; int draw; };

// The update of one step behind the network forward: x_out from x and the network output.  The row is `row` of the tables (the eager loop)
// or, with step_ptr, the one the device-side step counter names (the captured step: row 0).  eps_out (nullable): where the step's eps goes
// when it is not the network output itself; fused: the deterministic update went with the head launch (StepIO::fused_update), nothing is
// left to do.
int launch_step_update(const StepUpdateArgs& u, const float* x, const float* net_out, float* x_out, float* eps_out, int row, const int* step_ptr,
                       const StepNoise& z, bool fused, hipStream_t s);

// What a call's (eta, sampler, clip_x0) select.  clip_x0: the clamp as the kernels take it (0: off)
struct SamplerChoice { StepUpdate kind = StepUpdate::DDIM; bool sto = false, clip = false; float clip_x0 = 0.f; int px0 = 0; };
// The refusals every sampling loop makes, in one order, before anything touches the device; `who` prefixes the messages.  args_ok: the
// caller's required pointers are all there.
int sampler_check(const char* who, bool args_ok, float eta, int sampler, float clip_x0, const int32_t* timesteps_host, int num_steps,
                  bool have_seed, bool have_xT, int pred_type, SamplerChoice* out);
// Forms the call's coefficient rows on the host and copies them to coef_dev (4 per step) and extra_dev (1 per step; nullable: not needed);
// returns after the copies are done (the host vectors are the function's own)
int sampler_upload_tables(const char* who, const float* alpha_bars_host, int T, const int32_t* ts, int num_steps, int sampler, const SamplerChoice& c,
                          float eta, float* coef_dev, float* extra_dev, hipStream_t s);
// Seed and window ids (null: 0 .. B-1) copied into the workspace, so that a new seed or other windows replay the same captured step; returns
// after the copies are done
int sampler_stage_noise(uint64_t* seed_stage, int64_t* ids_stage, const uint64_t* seed_dev, const int64_t* window_ids_dev, int B, hipStream_t s);

}  // namespace dq
