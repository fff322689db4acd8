// What the two sampling calls share (dq_sampler.hip).  A call travels as one record, the dq_sample_call its caller filled; from it
// come, once each, the refusals made before anything touches the device (sample_check), the sampler's tables with x_T (sample_begin) and
// the captured-or-eager tail (sample_run).  The U-Net's call (unet_sample) and the transformer's (dq_tfm_sample) differ in their workspace
// layout, in the forward they hand the loop as its StepForward, and in what they stage in front of it.  Internal: not installed.
#pragma once
#include "../../include/dq_hip.h"  // dq_sample_call
#include "dq_common.h"
#include "dq_kernels.h"  // WinStatScratch
#include "dq_unet.h"     // StepUpdate, StepGraph
#include <functional>

namespace dq {

// One sampling call inside the library: the caller's record itself (dq_sample_call, include/dq_hip.h: its fields and their off values are
// described there, once), with what is not the caller's: who, the entry's name and the prefix of every refusal; allow_v: DQ_PRED_V is an
// objective of this entry's network.  Made by sample_call_open from the entry's pointer; nothing is copied field by field.
struct SampleCall : dq_sample_call {
  const char* who = "";
  bool allow_v = false;
  hipStream_t s() const { return (hipStream_t)stream; }
  bool per_window() const { return guidance_rescale != 0.0 || threshold_quantile != 0.f; }  // a live per-window option (NaN: set, refused by sample_check)
  bool graph() const { return use_graph && !traj_x && !traj_eps; }  // one step captured and replayed; otherwise the eager steps
};
// An entry's first two refusals, before any other field is read: a null record, then a struct_bytes that is not this library's
// sizeof(dq_sample_call) (the message names both); *out is then the record under the entry's name
int sample_call_open(const dq_sample_call* call, const char* who, bool allow_v, SampleCall* out);

// The per-window statistics of a step (k_winstat.hip), run between the forward and the update: rescale (guided
// calls): m_b of rescaled guidance at phi; q > 0: dynamic thresholding at that quantile with floor f and cap.  S: the call's scratch at a
// fixed address, carved once per call by its entry (win_stat_carve); the update then runs in its per-window form over the table at its head.
struct StepStats {
  double phi = 0.0;
  float q = 0.f, floor = 1.f, cap = 0.f;
  bool rescale = false;
  WinStatScratch S{};
  bool on() const { return rescale || q > 0.f; }
};

// The mixture-consistency pass of a step (k_group.hip), run in place on the network output between the forward and
// the update, which then runs in its x0-objective form: P members per group, the mode (DQ_CONSIST_*; 0: off) and the blend; pred: the
// network's objective, what the pass reads the output as; mix: the call's ms2_cond at the address the forward reads it from
struct StepGroup {
  int P = 1, mode = 0, pred = 0, normalize = 0;
  float strength = 1.f;
  const float* mix = nullptr;
  bool on() const { return mode != 0; }
};

// What a call's options select.  clip_x0: the clamp as the kernels take it (0: off); clip: x0 is clamped by clip_x0 or thresholded --
// either way the Solver family runs and the derived eps is the trajectory's.  stats: the per-window step (S is the entry's to carve);
// group: the consistency pass (sample_check_group's to fill; mix is the entry's to set)
struct SamplerChoice { StepUpdate kind = StepUpdate::DDIM; bool sto = false, clip = false; float clip_x0 = 0.f; int pred = 0; StepStats stats; StepGroup group; };
// Every refusal that does not need the network's shape, in one order, before anything touches the device: a null argument (net_args_ok:
// the network's own pointers are there), eta, the sampler and what it combines with (thresholding is refused where clip_x0 is and selects
// its update), the decreasing timesteps, the seed, the objective, the guidance scale, the per-window options' ranges and scratch pointer
int sample_check(const SampleCall& c, bool net_args_ok, SamplerChoice* out);
// The refusals of a call over groups, made behind every other one its entry makes before anything touches the device (sample_check's, the
// batch and step counts): group_size outside [1, 8], B % group_size != 0, an unknown mode, strength outside (0, 1] or NaN.
// Fills out->group (off, and nothing refused, at consistency 0)
int sample_check_group(const SampleCall& c, SamplerChoice* out);
// Tables up, x_T in place: the coefficient rows formed on the host and copied to coef_dev (4 per step) and extra_dev (sigma, or the solver's
// c1: 1 per step; nullable), the stream synchronised (a caller's pageable copy queued in front is done too), x_T copied to xa or drawn (draw 0)
int sample_begin(const SampleCall& c, const SamplerChoice& sc, int64_t per, float* coef_dev, float* extra_dev, float* xa);

// What every step's update of one sampling call shares: the tables (extra: sigma per row, or the solver's c1), the x0 history of the 2M
// solver (updated in place), the clamp (0: off) and the shape.  guided: the forward ran at 2 B windows -- rows
// [0, B) under the caller's condition, rows [B, 2B) under the null -- and the update combines the two outputs with the scale w inside its
// kernel, over the B windows of the first half; x and the network output are then 2 * B * per floats each.
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
  StepGroup group;  // on: `pred` above is DQ_PRED_X0, the form the update takes over the projected estimate
};

// One step's network forward on stream s, the one thing a call brings of its own: the network output of x into net_out, at timestep and
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
// What a captured step reads at fixed workspace addresses: the step counter, the staged seed and window ids (other ones replay the same step)
struct StepStage { int* step; uint64_t* seed; int64_t* ids; };
// The tail of a call, behind the network's own prologue.  c.graph(): the step counter zeroed, seed and ids staged (sto: the update draws;
// null ids: 0 .. B-1), and unless `reusable` (the handle's g.exec && stored key == key) one step -- forward, update with x in place, the
// counter's increment -- captured anew on g.cap_stream; then num_steps replays on the call's stream.  *captured: only then does the caller
// store its key, whatever is returned.  Otherwise the eager steps, step i drawing at index 1 + i.  launch_sample_finish ends both.
int sample_run(const SampleCall& c, const SampleLoop& L, bool sto, StepGraph& g, bool reusable, const StepStage& st, bool* captured);
}  // namespace dq
