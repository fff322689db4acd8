// The U-Net's sampling entry of the C ABI (include/dq_hip.h) and what both networks' calls share (dq_sampler.h): the stand-alone updates,
// each a StepUpdateLaunch filled by update_launch; the refusals, tables and tail of a sampling call, read from its record; and the loop
// with its captured step -- a network forward with one of the four StepUpdate kinds in or behind its head launch, plain, guided or per window.
#include "dq_net.h"
#include "dq_options.h"
#include "dq_sampler.h"
#include "dq_sampler_tables.h"
#include "../../include/dq_hip.h"

#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace dq;

namespace {

static_assert((int)StepUpdate::DDIM == DQ_UPDATE_DDIM && (int)StepUpdate::STOCHASTIC == DQ_UPDATE_STOCHASTIC &&
              (int)StepUpdate::SOLVER_1 == DQ_UPDATE_SOLVER_1 && (int)StepUpdate::SOLVER_2M == DQ_UPDATE_SOLVER_2M, "DQ_UPDATE_* are StepUpdate's values");

bool guidance_ok(float w) { return w >= 0.f && std::isfinite(w); }  // (false for NaN)

// The noise of the stochastic update: the windows' ids and the seed (device memory) and the draw index (the kernel adds the step counter)
struct StepNoise { const int64_t* ids = nullptr; const uint64_t* seed = nullptr; int draw = 0; };

// One update launch, filled in this one place: the family of `kind` (DQ_UPDATE_* are its values), guided iff net_u is given (x_mirror is dropped
// otherwise), the x0 history for the 2M kind alone, coef / extra the rows to read.  clip, w, step_ptr and win are left for the caller to set.
StepUpdateLaunch update_launch(StepUpdate kind, int pred, const float* x_t, const float* net, const float* net_u, float* x_prev, float* x_mirror,
                               float* hist, float* eps_out, const float* coef, const float* extra, const StepNoise& z, int B, int64_t per) {
  StepUpdateLaunch a;
  a.family = kind == StepUpdate::DDIM ? UpdateFamily::DDIM : kind == StepUpdate::STOCHASTIC ? UpdateFamily::STOCHASTIC : UpdateFamily::SOLVER;
  a.guided = net_u != nullptr; a.pred = pred;
  a.x_t = x_t; a.net = net; a.net_u = net_u;
  a.x_prev = x_prev; a.x_mirror = net_u ? x_mirror : nullptr; a.eps_out = eps_out;
  a.hist = kind == StepUpdate::SOLVER_2M ? hist : nullptr;
  a.coef = coef; a.extra = extra;
  a.ids = z.ids; a.seed = z.seed; a.draw = z.draw;
  a.B = B; a.per = per;
  return a;
}

// The update of one step behind the network forward: x_out from x and the network output.  The row is `row` of the tables (the eager loop)
// or, with step_ptr, the one the device-side step counter names (the captured step: row 0).  eps_out (nullable): where the step's eps goes
// when it is not the network output itself; fused: the deterministic update went with the head launch (StepIO::fused_update), nothing is
// left to do.  Guided (u.guided): net_out is the conditional output, net_u the unconditional one, x_mirror (nullable) receives x_out's values
// as well (the unconditional half's x of the next forward), and eps_out (nullable) the guided eps; never fused (the head launch of window b
// cannot see the output of window B + b).  Both are null otherwise.  Over groups (u.group.on()) net_out is first rewritten in place by the
// consistency pass.  Nothing is refused per step: the call's checks are made before the loop.
int launch_step_update(const StepUpdateArgs& u, const float* x, float* net_out, const float* net_u, float* x_out, float* x_mirror,
                       float* eps_out, int row, const int* step_ptr, const StepNoise& z, bool fused, hipStream_t s) {
  if (fused && u.kind == StepUpdate::DDIM && !u.guided) return 0;  // (the head launch has done it; a guided update never rides there)
  if (u.group.on()) {
    // the consistency pass: the network output becomes the group's projected x0 estimate in place; u.pred is DQ_PRED_X0
    const StepGroup& g = u.group;
    GroupProject p;
    p.x_t = x; p.net = net_out; p.x0_out = net_out; p.mix = g.mix; p.coef = u.coef + 4 * row; p.step_ptr = step_ptr;
    p.pred = g.pred; p.normalize = g.normalize; p.G = u.B / g.P; p.P = g.P; p.per = u.per; p.mode = g.mode; p.strength = g.strength;
    DQ_TRY(launch_group_project(p, s));
  }
  StepUpdateLaunch a = update_launch(u.kind, u.pred, x, net_out, net_u, x_out, x_mirror, u.hist, eps_out, u.coef + 4 * row, u.extra + row, z, u.B, u.per);
  a.clip = u.clip; a.w = u.w; a.step_ptr = step_ptr;
  if (u.stats.on()) {
    // the statistics step: m_b from the two network outputs, then s_b and rho_b from the x0 the update will form
    const StepStats& st = u.stats;
    const WinStatScratch& S = st.S;
    const bool thr = st.q > 0.f;
    if (st.rescale) DQ_TRY(launch_win_rescale(net_out, net_u, u.w, st.phi, u.B, u.per, S, S.tab, u.clip > 0.f ? u.clip : INFINITY, !thr, nullptr, s));
    if (thr) {
      WinQuantile q;
      q.x = x; q.c = net_out; q.u = net_u; q.coef = a.coef; q.step_ptr = step_ptr; q.m_tab = st.rescale ? S.tab : nullptr;
      q.w = u.w; q.pred = u.pred; q.guided = u.guided;
      q.q = st.q; q.floor = st.floor; q.cap = st.cap; q.tab = S.tab; q.init_m = !st.rescale;
      DQ_TRY(launch_win_quantile(q, u.B, u.per, S, s));
    }
    a.win = S.tab;
  }
  return launch_update(a, s);  // model.py:273-289
}

// Seed and window ids (null: 0 .. B-1) copied into the workspace; returns after the copies are done
int sampler_stage_noise(const StepStage& st, const uint64_t* seed_dev, const int64_t* window_ids_dev, int B, hipStream_t s) {
  DQ_HIP_OK(hipMemcpyAsync(st.seed, seed_dev, sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  if (window_ids_dev) {
    DQ_HIP_OK(hipMemcpyAsync(st.ids, window_ids_dev, sizeof(int64_t) * B, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  std::vector<int64_t> iota((size_t)B);
  for (int b = 0; b < B; ++b) iota[b] = b;
  DQ_HIP_OK(hipMemcpyAsync(st.ids, iota.data(), sizeof(int64_t) * B, hipMemcpyHostToDevice, s));
  DQ_HIP_OK(hipStreamSynchronize(s));  // (the vector is this function's own)
  return 0;
}

// (the one loop of both networks, dq_tfm_sample.hip's too: sample_run)
int finish(const SampleLoop& L, const float* x, hipStream_t s) {  // model.py:319-322
  return launch_sample_finish(x, L.ms2_cond, L.out_x, L.out_noise, L.upd.B * L.upd.per, L.normalize, s);
}

int replay_captured_step(StepGraph& g, bool reusable, const SampleLoop& L, int* step, const StepNoise& staged, hipStream_t s, bool* captured) {
  if (!reusable) {
    g.drop();
    // the caller's stream may be the legacy default stream, which cannot be captured: capture on a stream of our own (created on first use;
    // nothing executes during capture) and launch the instantiated graph on the caller's stream
    if (!g.cap_stream) DQ_HIP_OK(hipStreamCreateWithFlags(&g.cap_stream, hipStreamNonBlocking));
    hipStream_t cs = g.cap_stream;
    DQ_HIP_OK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    bool fused = false;
    int rc = L.forward(L.xa, L.xa, 0, step, L.eps, false, &fused, cs);  // (x in place: element-wise, read and written by the same lane; no eps out)
    const int64_t n = L.upd.B * L.upd.per;  // guided: the unconditional halves of the network output and of x lie n floats behind the conditional ones
    if (!rc) rc = launch_step_update(L.upd, L.xa, L.eps, L.upd.guided ? L.eps + n : nullptr, L.xa, L.upd.guided ? L.xa + n : nullptr, nullptr, 0, step,
                                     staged, fused, cs);
    if (!rc) rc = launch_inc_step(step, cs);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(cs, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }  // (the forward failed: the capture is ended, its graph gone)
    DQ_HIP_OK(ce);
    g.graph = graph;
    DQ_HIP_OK(hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0));
    *captured = true;
  }
  for (int i = 0; i < L.num_steps; ++i) DQ_HIP_OK(hipGraphLaunch(g.exec, s));
  return finish(L, L.xa, s);
}

int eager_steps(const SampleLoop& L, float* traj_x, float* traj_eps, const int64_t* window_ids_dev, const uint64_t* seed_dev, hipStream_t s) {
  const StepUpdateArgs& u = L.upd;
  const bool in_place = u.kind == StepUpdate::SOLVER_1 || u.kind == StepUpdate::SOLVER_2M;  // the solver loop keeps x in xa: xb holds the x0 history
  const int64_t n = u.B * u.per;
  float *xa = L.xa, *xb = u.hist;
  for (int i = 0; i < L.num_steps; ++i) {
    // eps objective: the network output IS the trajectory's eps; x0 objective, or a clamped x0: the derived eps goes to the trajectory.
    // Guided: the network output is two halves in the scratch (2 n floats), the trajectory's eps is always the update's guided one
    float* eps = (traj_eps && !u.guided) ? traj_eps + (int64_t)i * n : L.eps;
    float* xn = traj_x ? traj_x + (int64_t)i * n : (in_place ? xa : xb);
    bool fused = false;
    DQ_TRY(L.forward(xa, xn, i, nullptr, eps, traj_eps != nullptr, &fused, s));  // model.py:271 / :276
    float* eps_out = !traj_eps ? nullptr : u.guided ? traj_eps + (int64_t)i * n : (u.pred != DQ_PRED_EPS || L.clip) ? eps : nullptr;
    // (the mirror: the second half of the buffer the next forward reads -- xa when the step's x goes to a trajectory slot and is copied back)
    float* mirror = u.guided ? (traj_x ? xa : xn) + n : nullptr;
    DQ_TRY(launch_step_update(u, xa, eps, u.guided ? eps + n : nullptr, xn, mirror, eps_out, i, nullptr, StepNoise{window_ids_dev, seed_dev, 1 + i},
                              fused, s));
    if (traj_x) {
      DQ_HIP_OK(hipMemcpyAsync(xa, xn, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    } else if (!in_place) {
      std::swap(xa, xb);
    }
  }
  return finish(L, xa, s);
}

}  // namespace

namespace dq {

int sample_call_open(const dq_sample_call* call, const char* who, bool allow_v, SampleCall* out) {
  const std::string w(who);
  DQ_REQUIRE(call, w + ": null argument (call)");
  DQ_REQUIRE(call->struct_bytes == (int32_t)sizeof(dq_sample_call),
             w + ": call->struct_bytes is " + std::to_string(call->struct_bytes) + ", sizeof(dq_sample_call) of this library is " +
                 std::to_string(sizeof(dq_sample_call)) + " (a binding of another ABI version?)");
  *out = SampleCall{*call, who, allow_v};
  return 0;
}

int sample_check(const SampleCall& c, bool net_args_ok, SamplerChoice* out) {
  const std::string w(c.who);
  const float eta = c.eta;
  const int sampler = c.sampler;
  const bool threshold = c.threshold_quantile != 0.f;  // (NaN: on, then refused below)
  DQ_REQUIRE(net_args_ok && c.alpha_bars_host && c.ms2_cond && c.ms1_cond && c.timesteps_host && c.out_x && c.out_noise && c.workspace, w + ": null argument");
  DQ_REQUIRE(eta >= 0.f && eta <= 1.f, w + ": eta must satisfy 0 <= eta <= 1");  // (false for NaN)
  const bool sto = eta > 0.f;  // the update draws noise
  // step-consistent samplers: refused here, before anything touches the device
  DQ_REQUIRE(sampler == DQ_SAMPLER_REFERENCE || sampler == DQ_SAMPLER_DDIM || sampler == DQ_SAMPLER_DPMPP_2M, w + ": unknown sampler");
  const bool clip = c.clip_x0 > 0.f;  // (<= 0 and NaN: off)
  DQ_REQUIRE(sampler != DQ_SAMPLER_DPMPP_2M || !sto, w + ": DPM-Solver++(2M) is deterministic: eta must be 0");
  DQ_REQUIRE(!clip || sampler != DQ_SAMPLER_REFERENCE, w + ": clip_x0 needs the ddim or dpmpp_2m sampler");
  DQ_REQUIRE(!clip || !sto, w + ": clip_x0 needs eta == 0");
  DQ_REQUIRE(!threshold || sampler != DQ_SAMPLER_REFERENCE, w + ": threshold_quantile needs the ddim or dpmpp_2m sampler");
  DQ_REQUIRE(!threshold || !sto, w + ": threshold_quantile needs eta == 0");
  if (sampler != DQ_SAMPLER_REFERENCE && c.num_steps <= 1024)  // (a step count out of range is the entry's refusal: its list is not read)
    for (int i = 1; i < c.num_steps; ++i)
      DQ_REQUIRE(c.timesteps_host[i] < c.timesteps_host[i - 1], w + ": the timesteps of this sampler must be strictly decreasing");
  // the update: the Solver family (k_update.hip) behind the forward (2M, or a clamped x0 at first order); else the reference's kernels over this sampler's table
  out->kind = sampler == DQ_SAMPLER_DPMPP_2M ? StepUpdate::SOLVER_2M : (clip || threshold) ? StepUpdate::SOLVER_1 : sto ? StepUpdate::STOCHASTIC : StepUpdate::DDIM;
  out->sto = sto; out->clip = clip || threshold; out->clip_x0 = clip ? c.clip_x0 : 0.f;
  DQ_REQUIRE(c.seed_dev || (c.x_T && !sto), w + ": eta > 0 and a null x_T need the seed (device memory)");
  DQ_REQUIRE(c.pred_type == DQ_PRED_EPS || c.pred_type == DQ_PRED_X0 || (c.allow_v && c.pred_type == DQ_PRED_V), w + ": Unknown pred_type");
  out->pred = c.pred_type;
  DQ_REQUIRE(!c.guided || guidance_ok(c.guidance_scale), w + ": the guidance scale must be finite and >= 0");
  StepStats& st = out->stats = StepStats{};
  if (!c.per_window()) return 0;  // (both at their off value: threshold_max is not looked at, stat_scratch may be null)
  DQ_REQUIRE(c.guidance_rescale >= 0.0 && c.guidance_rescale <= 1.0, w + ": guidance_rescale must satisfy 0 <= guidance_rescale <= 1");  // (false for NaN)
  DQ_REQUIRE(!threshold || (c.threshold_quantile > 0.f && c.threshold_quantile <= 1.f), w + ": threshold_quantile must satisfy 0 < threshold_quantile <= 1 (0: off)");
  st.floor = clip ? c.clip_x0 : 1.f;
  DQ_REQUIRE(!threshold || c.threshold_max >= st.floor, w + ": threshold_max must be >= the floor (clip_x0, or 1 without it)");  // (false for NaN)
  st.phi = c.guidance_rescale; st.rescale = c.guided && c.guidance_rescale > 0.0;  // (unguided: g = c, m = 1 -- nothing to do)
  st.q = threshold ? c.threshold_quantile : 0.f; st.cap = c.threshold_max;
  DQ_REQUIRE(!st.on() || c.stat_scratch, w + ": null argument (stat_scratch)");
  return 0;
}

int sample_check_group(const SampleCall& c, SamplerChoice* out) {
  const std::string w(c.who);
  out->group = StepGroup{};
  if (c.consistency == DQ_CONSIST_NONE) return 0;
  DQ_REQUIRE(!c.guided && !c.per_window(),
             w + ": consistency together with guided, guidance_rescale or threshold_quantile is not implemented (follow-up: the guided form of "
                 "the group pass, which needs the mirror half written, and the per-window statistics over projected estimates)");
  DQ_REQUIRE(c.group_size >= 1 && c.group_size <= DQ_GROUP_MAX, w + ": group_size must be 1..8");
  DQ_REQUIRE(c.B % c.group_size == 0, w + ": the batch must be a whole number of groups (B % group_size == 0)");
  DQ_REQUIRE(group_mode_ok(c.consistency), w + ": unknown consistency mode");
  DQ_REQUIRE(group_strength_ok(c.consistency_strength), w + ": consistency strength must satisfy 0 < strength <= 1");
  StepGroup& g = out->group;
  g.P = c.group_size; g.mode = c.consistency; g.strength = c.consistency_strength; g.pred = out->pred; g.normalize = c.auto_normalize;
  return 0;
}

int sample_begin(const SampleCall& c, const SamplerChoice& sc, int64_t per, float* coef_dev, float* extra_dev, float* xa) {
  hipStream_t s = c.s();
  // coefficient table, fp32 like the reference, and sigma (eta > 0) or c1 (the solver) per step
  std::vector<float> coef(4 * (size_t)c.num_steps), extra((size_t)c.num_steps);
  if (c.sampler == DQ_SAMPLER_REFERENCE) DQ_TRY(dq_ddim_coef_table(c.alpha_bars_host, c.num_timesteps, c.timesteps_host, c.num_steps, c.eta, coef.data(), extra.data()));
  else DQ_TRY(sampler_rows(c.alpha_bars_host, c.num_timesteps, c.timesteps_host, c.num_steps, sc.kind == StepUpdate::SOLVER_1 ? SOLVER_ORDER1 : c.sampler, c.eta, coef.data(),
                           extra.data(), c.who));
  DQ_HIP_OK(hipMemcpyAsync(coef_dev, coef.data(), sizeof(float) * coef.size(), hipMemcpyHostToDevice, s));
  if (extra_dev) DQ_HIP_OK(hipMemcpyAsync(extra_dev, extra.data(), sizeof(float) * extra.size(), hipMemcpyHostToDevice, s));
  // the host vector must outlive the copy: pageable H2D copies are staged synchronously by the runtime, but make it explicit
  DQ_HIP_OK(hipStreamSynchronize(s));
  if (c.x_T) DQ_HIP_OK(hipMemcpyAsync(xa, c.x_T, sizeof(float) * c.B * per, hipMemcpyDeviceToDevice, s));
  else DQ_TRY(launch_randn(xa, c.window_ids_dev, c.seed_dev, 0, c.B, per, s));  // draw index 0 is x_T's
  return 0;
}

int sample_run(const SampleCall& c, const SampleLoop& L, bool sto, StepGraph& g, bool reusable, const StepStage& st, bool* captured) {
  *captured = false;
  if (!c.graph()) return eager_steps(L, c.traj_x, c.traj_eps, c.window_ids_dev, c.seed_dev, c.s());
  // ---- hipGraph path: one step captured once, replayed per step; the step index lives on the device (*step, bumped by k_inc_step)
  DQ_HIP_OK(hipMemsetAsync(st.step, 0, sizeof(int), c.s()));
  if (sto) DQ_TRY(sampler_stage_noise(st, c.seed_dev, c.window_ids_dev, c.B, c.s()));
  return replay_captured_step(g, reusable, L, st.step, StepNoise{st.ids, st.seed, 0}, c.s(), captured);
}

}  // namespace dq

namespace {

// The U-Net's sampling call, under dq_ddim_sample.  Guided, the arena and the forward run at NB = 2 B windows: rows [0, B)
// carry the caller's MS1, rows [B, 2B) q.null_ms1 in every element (a raw value: it goes through the same cm, ca normalisation); both
// halves see the same mixture and the same x, which the update keeps equal by writing x_prev to both (x_mirror).  The update / hist /
// trajectories / outputs cover B windows, and a guided update never rides in the head launch.
int unet_sample(dq_plan* plan, const float* params, const float* rope_freqs, const SampleCall& q) {
  const std::string wh(q.who);
  SamplerChoice sc;
  DQ_TRY(sample_check(q, plan && params, &sc));
  const int B = q.B, RT = q.RT, num_steps = q.num_steps;
  const bool g = q.guided != 0;
  if (sc.stats.on()) {  // the statistics scratch, carved here for every step of the call
    DQ_REQUIRE(B > 0 && RT > 0, wh + ": need B, RT > 0 and 1 <= num_steps <= 1024");
    DQ_TRY(win_stat_carve(wh, q.stat_scratch, q.stat_scratch_bytes, B, (int64_t)RT * plan->plan.mz, &sc.stats.S));
  }
  DQ_REQUIRE(B > 0 && RT > 0 && num_steps >= 1 && num_steps <= 1024, wh + ": need B, RT > 0 and 1 <= num_steps <= 1024");
  DQ_REQUIRE(!g || B <= INT32_MAX / 2, wh + ": batch too large");
  DQ_TRY(sample_check_group(q, &sc));  // (the last refusals made on the host alone: ensure_arena brings the plan's tables to the device)
  const bool grp = sc.group.on();
  const int NB = g ? 2 * B : B;  // the windows of the arena and of the forward
  DQ_TRY(ensure_arena(plan, NB, RT));
  const Arena& a = plan->arena;
  DQ_REQUIRE(q.workspace_bytes >= (int64_t)sizeof(float) * a.floats, wh + ": workspace too small");
  DQ_REQUIRE(q.num_timesteps >= 1, wh + ": num_timesteps must be >= 1");
  hipStream_t s = q.s();
  float* W = (float*)q.workspace;
  Ctx c{plan->plan, a, params, W, nullptr, nullptr, NB, RT, s};
  c.save = false;
  const int64_t per = (int64_t)RT * plan->plan.mz, n = B * per;
  const int64_t n1 = (int64_t)B * RT * plan->plan.ms1_channels;  // the caller's MS1
  const float cm = q.auto_normalize ? 2.f : 1.f, ca = q.auto_normalize ? -1.f : 0.f;
  // the head launch takes the update when it can (StepIO::x_t); the others, every guided one and every one over groups (the pass comes
  // between the two) run behind the forward
  const bool in_head = sc.kind == StepUpdate::DDIM && !g && !grp;
  float* xa = c.w(a.xa);
  DQ_TRY(sample_begin(q, sc, per, c.w(a.coef), in_head ? nullptr : c.w(a.sigma), xa));
  if (g) DQ_HIP_OK(hipMemcpyAsync(xa + n, xa, sizeof(float) * n, hipMemcpyDeviceToDevice, s));  // the unconditional half starts from the same x_T
  // the conditions staged at fixed addresses: for the captured step, and for every guided call (the mixture twice; the caller's MS1, then
  // the null's raw value in every element of the second half); an unguided eager call reads the caller's
  const bool staged = q.graph() || g;
  const float* c2 = staged ? c.w(a.c2_stage) : q.ms2_cond;
  const float* c1 = staged ? c.w(a.c1_stage) : q.ms1_cond;
  // The step index of a captured step lives on the device: k_time_fwd reads ts_tab[*step], the update its coefficient row, k_inc_step bumps it.
  int* ts_tab = reinterpret_cast<int*>(c.w(a.ts_tab));
  if (q.graph()) DQ_HIP_OK(hipMemcpyAsync(ts_tab, q.timesteps_host, sizeof(int32_t) * num_steps, hipMemcpyHostToDevice, s));
  if (staged) {
    DQ_HIP_OK(hipMemcpyAsync(c.w(a.c2_stage), q.ms2_cond, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    DQ_HIP_OK(hipMemcpyAsync(c.w(a.c1_stage), q.ms1_cond, sizeof(float) * n1, hipMemcpyDeviceToDevice, s));
  }
  if (g) {
    uint32_t bits;
    std::memcpy(&bits, &q.null_ms1, sizeof bits);
    DQ_HIP_OK(hipMemcpyAsync(c.w(a.c2_stage) + n, q.ms2_cond, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    DQ_HIP_OK(hipMemsetD32Async((hipDeviceptr_t)(c.w(a.c1_stage) + n1), (int)bits, (size_t)n1, s));
  }
  if (q.graph()) DQ_HIP_OK(hipStreamSynchronize(s));  // ts is caller memory; also keeps the capture free of pending copies of the conditions
  Ctx::StepIO io; io.pred = sc.pred;
  DQ_TRY(unet_sample_prologue(c, c1, cm, ca, rope_freqs, &io.prologue));
  // the forward of this network: captured at the step the device-side counter names (all pointers inside the arena / parameter buffers),
  // eagerly at the caller's timestep
  const StepForward forward = [&](const float* x, float* x_out, int row, const int* step_ptr, float* net_out, bool want_eps, bool* fused, hipStream_t fs) {
    Ctx fc{plan->plan, a, params, W, nullptr, nullptr, NB, RT, fs};
    fc.save = false; fc.step_io = &io;
    io.x_t = in_head ? x : nullptr; io.x_out = x_out; io.coef = c.w(a.coef) + 4 * row; io.step_ptr = step_ptr; io.want_eps = want_eps; io.fused_update = false;
    const int rc = step_ptr ? unet_forward(fc, rope_freqs, x, nullptr, 0, c2, c1, cm, ca, plan->dev, net_out, ts_tab, step_ptr)
                            : unet_forward(fc, rope_freqs, x, nullptr, q.timesteps_host[row], c2, c1, cm, ca, plan->dev, net_out);
    *fused = io.fused_update;
    return rc;
  };
  sc.group.mix = c2;  // the group's mixture: row g of the tensor the network reads
  // (over groups the update runs in its x0-objective form over the projected estimate; the pass reads the output by the network's objective)
  const SampleLoop loop{forward, StepUpdateArgs{sc.kind, c.w(a.coef), c.w(a.sigma), c.w(a.xb), sc.clip_x0, grp ? DQ_PRED_X0 : sc.pred, B, per, g,
                                                g ? q.guidance_scale : 1.f, sc.stats, sc.group},
                        xa, c.w(a.eps), sc.clip, num_steps, q.ms2_cond, q.out_x, q.out_noise, q.auto_normalize};
  StepKey key;
  key.params = params; key.rope = rope_freqs; key.ws = q.workspace; key.B = B; key.RT = RT; key.normalize = q.auto_normalize; key.pred = q.pred_type;
  key.update = sc.kind; key.clip = sc.clip_x0; key.guidance = g ? q.guidance_scale : -1.f; key.opt_epoch = options_epoch();
  if (sc.stats.on()) { key.rescale = sc.stats.rescale ? sc.stats.phi : 0.0; key.quantile = sc.stats.q; key.cap = sc.stats.cap; key.stat_scratch = q.stat_scratch; }
  if (grp) { key.group_size = sc.group.P; key.consistency = sc.group.mode; key.strength = sc.group.strength; }
  const StepStage stage{reinterpret_cast<int*>(c.w(a.step)), reinterpret_cast<uint64_t*>(c.w(a.seed_stage)), reinterpret_cast<int64_t*>(c.w(a.ids_stage))};
  bool captured;
  const int rc = sample_run(q, loop, sc.sto, plan->step, plan->step.exec && plan->step_key == key, stage, &captured);
  if (captured) plan->step_key = key;
  return rc;
}

// The refusals of the stand-alone guided and per-window updates, in one order; args_ok: the entry's required pointers are all there;
// guided: net_u is given (the per-window entry alone takes it null, and then for the solver kinds alone)
int update_check(const std::string& who, bool args_ok, int kind, bool guided, const void* seed_dev, const void* x0_hist, int pred_type, float w,
                 int B, int64_t per_window) {
  DQ_REQUIRE(args_ok, who + ": null argument");
  DQ_REQUIRE(kind == DQ_UPDATE_DDIM || kind == DQ_UPDATE_STOCHASTIC || kind == DQ_UPDATE_SOLVER_1 || kind == DQ_UPDATE_SOLVER_2M,
             who + ": unknown update kind");
  DQ_REQUIRE(guided || kind == DQ_UPDATE_SOLVER_1 || kind == DQ_UPDATE_SOLVER_2M,
             who + ": the unguided per-window form is the solver kinds' (thresholding); net_u is needed");
  DQ_REQUIRE(kind != DQ_UPDATE_STOCHASTIC || seed_dev, who + ": the stochastic update needs the seed (device memory)");
  DQ_REQUIRE(kind != DQ_UPDATE_SOLVER_2M || x0_hist, who + ": the 2M update needs the x0 history");
  DQ_REQUIRE(pred_type == DQ_PRED_EPS || pred_type == DQ_PRED_X0 || pred_type == DQ_PRED_V, who + ": Unknown pred_type");
  DQ_REQUIRE(!guided || guidance_ok(w), who + ": the guidance scale must be finite and >= 0");
  DQ_REQUIRE(B >= 0 && per_window >= 0, who + ": negative size");
  return 0;
}

// dq_guided_update and dq_guided_update_v: `who` prefixes the refusals
int guided_update(const std::string& who, int kind, const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror,
                  float* x0_hist, float* eps_out, const float* coef_dev, float w, float clip_x0, const int64_t* window_ids_dev,
                  const uint64_t* seed_dev, int draw, int pred_type, int B, int64_t per_window, void* stream) {
  DQ_TRY(update_check(who, x_t && net_c && net_u && x_prev && coef_dev, kind, true, seed_dev, x0_hist, pred_type, w, B, per_window));
  StepUpdateLaunch a = update_launch((StepUpdate)kind, pred_type, x_t, net_c, net_u, x_prev, x_mirror, x0_hist, eps_out, coef_dev, coef_dev + 4,
                                     StepNoise{window_ids_dev, seed_dev, draw}, B, per_window);
  a.clip = clip_x0; a.w = w;
  return launch_update(a, (hipStream_t)stream);
}

}  // namespace

extern "C" {

// The stand-alone updates: one step over caller-supplied tensors, row 0 of coef_dev (with sigma / c1 as a fifth float behind it); a plain
// element count n is one window of n elements
int dq_ddim_step(const float* x_t, const float* eps, float* x_prev, const float* coef_dev, int64_t n, void* stream) {
  return launch_update(update_launch(StepUpdate::DDIM, DQ_PRED_EPS, x_t, eps, nullptr, x_prev, nullptr, nullptr, nullptr, coef_dev, coef_dev + 4, {}, 1, n),
                       (hipStream_t)stream);
}

int dq_ddim_step_x0(const float* x_t, const float* x0_pred, float* x_prev, float* eps_out, const float* coef_dev, int64_t n,
                    void* stream) {
  DQ_REQUIRE(x_t && x0_pred && x_prev && coef_dev, "dq_ddim_step_x0: null argument");
  return launch_update(update_launch(StepUpdate::DDIM, DQ_PRED_X0, x_t, x0_pred, nullptr, x_prev, nullptr, nullptr, eps_out, coef_dev, coef_dev + 4, {}, 1, n),
                       (hipStream_t)stream);
}

int dq_ddim_step_v(const float* x_t, const float* v_pred, float* x_prev, float* eps_out, const float* coef_dev, int64_t n, void* stream) {
  DQ_REQUIRE(x_t && v_pred && x_prev && coef_dev, "dq_ddim_step_v: null argument");
  return launch_update(update_launch(StepUpdate::DDIM, DQ_PRED_V, x_t, v_pred, nullptr, x_prev, nullptr, nullptr, eps_out, coef_dev, coef_dev + 4, {}, 1, n),
                       (hipStream_t)stream);
}

int dq_randn(float* out, const int64_t* window_ids_dev, const uint64_t* seed_dev, int draw, int B, int64_t per_window, void* stream) {
  return launch_randn(out, window_ids_dev, seed_dev, draw, B, per_window, (hipStream_t)stream);
}

int dq_ddim_step_sto(const float* x_t, const float* net_out, float* x_prev, float* eps_out, const float* coef_dev,
                     const int64_t* window_ids_dev, const uint64_t* seed_dev, int draw, int pred_type, int B, int64_t per_window,
                     void* stream) {
  DQ_REQUIRE(x_t && net_out && x_prev && coef_dev && seed_dev, "dq_ddim_step_sto: null argument");
  DQ_REQUIRE(pred_type == DQ_PRED_EPS || pred_type == DQ_PRED_X0 || pred_type == DQ_PRED_V, "dq_ddim_step_sto: Unknown pred_type");
  // (refused by launch_update: a per-window count that is no multiple of 4, tensors that are not 16-byte aligned)
  return launch_update(update_launch(StepUpdate::STOCHASTIC, pred_type, x_t, net_out, nullptr, x_prev, nullptr, nullptr,
                                     pred_type != DQ_PRED_EPS ? eps_out : nullptr, coef_dev, coef_dev + 4, StepNoise{window_ids_dev, seed_dev, draw},
                                     B, per_window),
                       (hipStream_t)stream);
}

int dq_solver_step_v(const float* x_t, const float* v_pred, float* x_prev, float* x0_hist, float* eps_out, const float* coef_dev, float clip_x0,
                     int64_t n, void* stream) {
  DQ_REQUIRE(x_t && v_pred && x_prev && coef_dev, "dq_solver_step_v: null argument");
  // (a history makes it the 2M update, none the first-order one)
  StepUpdateLaunch a = update_launch(x0_hist ? StepUpdate::SOLVER_2M : StepUpdate::SOLVER_1, DQ_PRED_V, x_t, v_pred, nullptr, x_prev, nullptr, x0_hist,
                                     eps_out, coef_dev, coef_dev + 4, {}, 1, n);
  a.clip = clip_x0;
  return launch_update(a, (hipStream_t)stream);
}

int dq_solver_step(const float* x_t, const float* net_out, float* x_prev, float* x0_hist, float* eps_out, const float* coef_dev, float clip_x0,
                   int pred_type, int64_t n, void* stream) {
  DQ_REQUIRE(x_t && net_out && x_prev && coef_dev, "dq_solver_step: null argument");
  DQ_REQUIRE(pred_type == DQ_PRED_EPS || pred_type == DQ_PRED_X0, "dq_solver_step: Unknown pred_type");  // (DQ_PRED_V: dq_solver_step_v)
  StepUpdateLaunch a = update_launch(x0_hist ? StepUpdate::SOLVER_2M : StepUpdate::SOLVER_1, pred_type, x_t, net_out, nullptr, x_prev, nullptr, x0_hist,
                                     eps_out, coef_dev, coef_dev + 4, {}, 1, n);
  a.clip = clip_x0;
  return launch_update(a, (hipStream_t)stream);
}

int dq_ddim_sample(dq_plan* plan, const float* params, const float* rope_freqs, const dq_sample_call* call) {
  SampleCall q;
  DQ_TRY(sample_call_open(call, "dq_ddim_sample", true, &q));
  return unet_sample(plan, params, rope_freqs, q);
}

// The record's layout as compiled here: sizeof, then (offsetof, size) per field in declaration order
int dq_debug_sample_call_layout(int32_t* out, int cap) {
  int n = 0;
  int32_t v[1 + 2 * 64];
  v[n++] = (int32_t)sizeof(dq_sample_call);
#define DQ_F(f) v[n++] = (int32_t)offsetof(dq_sample_call, f); v[n++] = (int32_t)sizeof(((dq_sample_call*)nullptr)->f);
  DQ_F(struct_bytes) DQ_F(alpha_bars_host) DQ_F(num_timesteps) DQ_F(x_T) DQ_F(ms2_cond) DQ_F(ms1_cond) DQ_F(auto_normalize) DQ_F(pred_type)
  DQ_F(timesteps_host) DQ_F(num_steps) DQ_F(out_x) DQ_F(out_noise) DQ_F(traj_x) DQ_F(traj_eps) DQ_F(use_graph) DQ_F(workspace)
  DQ_F(workspace_bytes) DQ_F(B) DQ_F(RT) DQ_F(stream) DQ_F(eta) DQ_F(seed_dev) DQ_F(window_ids_dev) DQ_F(sampler) DQ_F(clip_x0) DQ_F(guided)
  DQ_F(guidance_scale) DQ_F(null_ms1) DQ_F(guidance_rescale) DQ_F(threshold_quantile) DQ_F(threshold_max) DQ_F(stat_scratch)
  DQ_F(stat_scratch_bytes) DQ_F(group_size) DQ_F(consistency) DQ_F(consistency_strength)
#undef DQ_F
  if (!out || cap < n) return -1;
  std::memcpy(out, v, sizeof(int32_t) * n);
  return n;
}

int dq_guided_update(int kind, const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror, float* x0_hist,
                     float* eps_out, const float* coef_dev, float w, float clip_x0, const int64_t* window_ids_dev, const uint64_t* seed_dev,
                     int draw, int pred_type, int B, int64_t per_window, void* stream) {
  // (this entry's pred_type names the reference's two objectives; DQ_PRED_V: dq_guided_update_v)
  return guided_update("dq_guided_update", kind, x_t, net_c, net_u, x_prev, x_mirror, x0_hist, eps_out, coef_dev, w, clip_x0, window_ids_dev, seed_dev,
                       draw, pred_type == DQ_PRED_V ? -1 : pred_type, B, per_window, stream);
}

int dq_guided_update_v(int kind, const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror, float* x0_hist,
                       float* eps_out, const float* coef_dev, float w, float clip_x0, const int64_t* window_ids_dev, const uint64_t* seed_dev,
                       int draw, int B, int64_t per_window, void* stream) {
  return guided_update("dq_guided_update_v", kind, x_t, net_c, net_u, x_prev, x_mirror, x0_hist, eps_out, coef_dev, w, clip_x0, window_ids_dev,
                       seed_dev, draw, DQ_PRED_V, B, per_window, stream);
}

// ---- per-window sampler control
int64_t dq_sample_stat_scratch_bytes(int B, int64_t per_window) { return win_stat_scratch_bytes(B, per_window); }

int dq_window_rescale(const float* net_c, const float* net_u, float w, double phi, int B, int64_t per_window, float* m_out, void* scratch,
                      int64_t scratch_bytes, void* stream) {
  const std::string who = "dq_window_rescale";
  DQ_REQUIRE(net_c && net_u && m_out && scratch, who + ": null argument");
  DQ_REQUIRE(guidance_ok(w), who + ": the guidance scale must be finite and >= 0");
  DQ_REQUIRE(phi >= 0.0 && phi <= 1.0, who + ": guidance_rescale must satisfy 0 <= guidance_rescale <= 1");
  WinStatScratch S;
  DQ_TRY(win_stat_carve(who, scratch, scratch_bytes, B, per_window, &S));
  DQ_REQUIRE((((uintptr_t)net_c | (uintptr_t)net_u | (uintptr_t)m_out) & 3) == 0, who + ": tensors must be 4-byte aligned");
  return launch_win_rescale(net_c, net_u, w, phi, B, per_window, S, nullptr, 0.f, false, m_out, (hipStream_t)stream);
}

int dq_window_abs_quantile(const float* x, int B, int64_t per_window, float q, float* out, void* scratch, int64_t scratch_bytes, void* stream) {
  const std::string who = "dq_window_abs_quantile";
  DQ_REQUIRE(x && out && scratch, who + ": null argument");
  DQ_REQUIRE(q > 0.f && q <= 1.f, who + ": threshold_quantile must satisfy 0 < threshold_quantile <= 1");
  WinStatScratch S;
  DQ_TRY(win_stat_carve(who, scratch, scratch_bytes, B, per_window, &S));
  DQ_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 3) == 0, who + ": tensors must be 4-byte aligned");
  WinQuantile qa;
  qa.x = x; qa.q = q; qa.q_out = out;
  return launch_win_quantile(qa, B, per_window, S, (hipStream_t)stream);
}

int dq_step_update_adaptive(int kind, const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror, float* x0_hist,
                            float* eps_out, const float* coef_dev, float w, const float* table_dev, const int64_t* window_ids_dev,
                            const uint64_t* seed_dev, int draw, int pred_type, int B, int64_t per_window, void* stream) {
  DQ_TRY(update_check("dq_step_update_adaptive", x_t && net_c && x_prev && coef_dev && table_dev, kind, net_u != nullptr, seed_dev, x0_hist, pred_type,
                      w, B, per_window));
  StepUpdateLaunch a = update_launch((StepUpdate)kind, pred_type, x_t, net_c, net_u, x_prev, x_mirror, x0_hist, eps_out, coef_dev, coef_dev + 4,
                                     StepNoise{window_ids_dev, seed_dev, draw}, B, per_window);
  a.w = w; a.win = table_dev;
  return launch_update(a, (hipStream_t)stream);
}

int dq_ms1_cond_drop(const float* ms1_in, float* ms1_out, const int64_t* window_ids_dev, const uint64_t* seed_dev, int draw, double p,
                     float null_value, int B, int64_t per_ms1, void* stream) {
  DQ_REQUIRE(ms1_in && ms1_out && seed_dev, "dq_ms1_cond_drop: null argument");
  return launch_cond_drop(ms1_in, ms1_out, window_ids_dev, seed_dev, draw, p, null_value, B, per_ms1, (hipStream_t)stream);
}

}  // extern "C"
