// Internal launch API of libdq_hip.so (host side).  Every launcher is asynchronous on the given stream,
// allocates nothing and returns 0 on success (non-zero after dq::set_error()).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

namespace dq {

constexpr int MSE_MAX_BLOCKS = 1024;  // size of the partial-sum scratch used by the loss / grad-norm reductions

// ---- k_stream.hip: q_sample, the sample epilogue, the two loss forms and the MS1 term
// x_t (B, per) = sa_b * norm(x0) + sb_b * noise, sa_b = sqrt(alpha_bars[t_b]), sb_b = sqrt(1 - alpha_bars[t_b]); any per (16 bytes per lane
// iff per % 4 == 0), an empty call launches nothing.  With a stack (dq_tfm_eval_step): R repeats of the B windows,
// repeat-major (sample n = r * B + b; x0 (B, per) shared by the repeats, t and x_t (R, B)); noise (R, B, per), or nullptr: drawn in the
// kernel at draw index first_draw + r from seed (device memory) and ids (nullable: 0 .. B-1) and never written.  The stacked form wants
// B, R > 0, per % 4 == 0 below 2^32 and 16-byte aligned tensors.
struct NoiseStack { int R = 1; const int64_t* ids = nullptr; const uint64_t* seed = nullptr; int first_draw = 0; };
int launch_q_sample(const float* alpha_bars, const float* x0, const int64_t* t, const float* noise, float* x_t, int B, int64_t per,
                    int normalize, hipStream_t s, const NoiseStack* stack = nullptr);
int launch_sample_finish(const float* x, const float* ms2_cond, float* out_x, float* out_noise, int64_t n, int normalize,
                         hipStream_t s);
// What a loss compares the network output with, weighted per sample by lw[t_b] (lw nullable: 1):
//   READ   z * tm + ta.  launch_mse_fwd_bwd applies the map only when lw is given (z * 1 + 0 is not z: it loses the sign of a -0);
//          launch_mse_per_window always does
//   V      sa_b * z - sb_b * (x0 * tm + ta) with z the noise, formed per element and never written
//   DRAWN  launch_mse_per_window only: z is not read but drawn again as launch_q_sample's stack drew it, then mapped like READ
// stacked (launch_mse_per_window; READ or DRAWN): R repeats of B windows as above, t (R, B); a READ target has Bt = B windows (shared by
// the repeats) or R * B (one each).  shared: z holds one row per window of the batch (the clean x0), not one per sample (the noise).
enum class TargetKind { READ, V, DRAWN };
struct LossTarget {
  TargetKind kind = TargetKind::READ;
  const float* z = nullptr; const float* x0 = nullptr; const float* alpha_bars = nullptr;
  float tm = 1.f, ta = 0.f;
  const float* lw = nullptr; const int64_t* t = nullptr;
  bool shared = false, stacked = false; int Bt = 0; const int64_t* ids = nullptr; const uint64_t* seed = nullptr; int first_draw = 0;
};
// the target of an objective (DQ_PRED_*), stated once: eps -- the noise, weight 1 (a null noise: DRAWN); x0 -- x0 * cm + ca weighted by
// lw[t_b], shared; v -- sa_b noise - sb_b (x0 * cm + ca) weighted by lw[t_b] (lw null: 1)
LossTarget loss_target(int pred_type, const float* x0, const float* noise, const float* alpha_bars, float cm, float ca, const float* lw,
                       const int64_t* t);
// loss_out = mean over the B * per elements of w_b (pred - target)^2, grad_out (nullable) = its gradient; partials: MSE_MAX_BLOCKS floats.
// defer_sum: the kernel leaves its per-block partials, *defer_sum receives their count and loss_out is NOT written -- the caller runs
// launch_sum_partials(partials, count, 1 / n, loss_out, stream) when it suits (dq_train_step: on the side stream)
int launch_mse_fwd_bwd(const float* pred, const LossTarget& target, float* loss_out, float* grad_out, float* partials, int B, int64_t per,
                       hipStream_t s, int* defer_sum = nullptr);
int launch_sum_partials(const float* partials, int count, float scale, float* out, hipStream_t s);
// the MS1 term of train_step with ms1_loss_weight = w > 0: on entry loss_out / grad hold the MSE part, on exit the
// combined loss (1 - w) * MSE + w * additional and its gradient w.r.t. the network output; x_t null = x0 objective;
// scratch: 5 * B * RT + B floats
int launch_ms1_loss(const float* out, const float* x_t, const float* ms1, float cm, float ca, const float* lw, const int64_t* t, float w,
                    int B, int RT, int MZ, float* grad, float* loss_out, float* scratch, hipStream_t s);
// held-out loss, forward only: per_window[n] = MSE of window n of out (R * B, per) against the target, loss_out[r] = mean_b lw[t[r, b]] *
// MSE[r, b], fp64 sums in a fixed order; R = 1 unless the target is stacked.  scratch: mse_per_window_scratch_bytes(R * B, per) = 8 * R * B *
// ceil(per / MSE_PW_SLICE) bytes
constexpr int MSE_PW_SLICE = 8192;  // elements of a window one block of k_mse_per_window sums
int64_t mse_per_window_scratch_bytes(int B, int64_t per);
int launch_mse_per_window(const float* out, const LossTarget& target, float* per_window, float* loss_out, void* scratch, int64_t scratch_bytes,
                          int B, int R, int64_t per, hipStream_t s);
int launch_axpy(float* dst, const float* src, int64_t n, hipStream_t s);  // dst += src
int launch_zero(float* dst, int64_t n, hipStream_t s);  // dst = 0 (a kernel, not a memset node)
int launch_copy(float* dst, const float* src, int64_t n, hipStream_t s);  // dst = src (a kernel, not a memcpy node)
// ---- k_update.hip: the update of one sampling step, x_prev from x_t and the network output, for the three families
//   DDIM        rows [sa, sb, sap, sbp] of coef (extra unused)
//   STOCHASTIC  the same plus sigma * z: rows [sa, sb, sap, c], extra = sigma, one float per row; z from Philox4x32-10 / Box-Muller normals
//               keyed by (seed, window id, element, draw index), seed and ids (nullable: 0 .. B-1) in device memory
//   SOLVER      x_prev = cx*x + c0*x0 + c1*hist: rows [sa, sb, cx, c0], extra = c1, one float per row; x0 clamped to [-clip, clip] when
//               clip > 0; hist (nullable when every c1 is 0) receives x0
// step_ptr (nullable): the row index on the device (STOCHASTIC: and the draw index 1 + step), else row 0 and `draw`.  pred (DQ_PRED_*): what `net`
// is -- the network's eps, x0 or v prediction.  eps_out (nullable) receives the step's eps when it is not the network output itself (always, for a guided or
// SOLVER step).  guided (dq_guide.h): the same arithmetic on g = net_u + w (net - net_u) in place of the network
// output, x_mirror (nullable) receives x_prev too.  Element-wise: x_prev may alias x_t, eps_out the network output.  Any count and any
// 4-byte aligned tensors, except that the unguided STOCHASTIC form wants per % 4 == 0 and 16-byte aligned tensors; 16-byte accesses iff
// the count (STOCHASTIC: per) is a multiple of 4 and every tensor given is 16-byte aligned, one element per lane otherwise.
enum class UpdateFamily { DDIM, STOCHASTIC, SOLVER };
struct StepUpdateLaunch {
  UpdateFamily family = UpdateFamily::DDIM;
  bool guided = false;
  int pred = 0;  // DQ_PRED_*
  const float* x_t = nullptr; const float* net = nullptr; const float* net_u = nullptr;
  float* x_prev = nullptr; float* x_mirror = nullptr; float* hist = nullptr; float* eps_out = nullptr;
  const float* coef = nullptr; const float* extra = nullptr;
  const int64_t* ids = nullptr; const uint64_t* seed = nullptr; int draw = 0;
  float clip = 0.f, w = 1.f;
  int B = 0; int64_t per = 0;  // B windows of per elements (a plain count n: B = 1, per = n)
  const int* step_ptr = nullptr;
  const float* win = nullptr;  // the per-window form: the (B, 4) table [m_b, s_b, rho_b, -] of k_winstat.hip (guided, or the SOLVER family)
};
int launch_update(const StepUpdateLaunch& a, hipStream_t s);
int launch_inc_step(int* p, hipStream_t s);
// ---- k_winstat.hip: the per-window statistics in front of the per-window form of the update.  A window is cut
// into chunks of WS_CHUNK elements whatever the batch.  The scratch, carved at fixed offsets (a captured step replays): the (B, 4) table
// [m_b, s_b, rho_b, -], the select state of each radix pass, WS_MOMENTS fp64 partials per chunk, two buffers of 2 x 256 counts per chunk.
constexpr int WS_CHUNK = 8192, WS_MOMENTS = 4;
struct WinSelState { uint32_t prefA, rankA, prefB, rankB; };  // the key bits found so far and the rank left under them, for ranks j and j + 1
struct WinStatScratch { float* tab; WinSelState* st; double* part; uint32_t* hist[2]; int nch; };
int64_t win_stat_scratch_bytes(int B, int64_t per);  // 80 B + 4128 B ceil(per / WS_CHUNK); -1 for B < 1 or per < 1
int win_stat_carve(const std::string& who, void* scratch, int64_t scratch_bytes, int B, int64_t per, WinStatScratch* out);  // refuses; no device call
// m_b = (float)(phi * sqrt(var_c / var_g) + (1 - phi)) of c and g = guide(c, u, w) per window -> tab[4 b] (nullable) and m_out[b] (nullable);
// init_rest: tab's row becomes [m_b, s_init, 1, 0]
int launch_win_rescale(const float* c, const float* u, float w, double phi, int B, int64_t per, const WinStatScratch& S, float* tab, float s_init,
                       bool init_rest, float* m_out, hipStream_t s);
// The q-quantile Q (linear interpolation between the two exact order statistics) of |x| per window (c null), or of |x0| with x0 formed as the
// update forms it: from x, the network output c (guided: and u, scale w, times m_tab[4 b] when m_tab is given) under objective `pred` with
// row [sa, sb, ..] of coef (step_ptr: the row the device-side step counter names).  q_out (nullable): Q; tab (nullable): s_b = min(max(Q,
// floor), cap) and rho_b = floor / s_b into columns 1 and 2, with init_m the whole row [1, s_b, rho_b, 0].
struct WinQuantile {
  const float* x = nullptr; const float* c = nullptr; const float* u = nullptr;
  const float* coef = nullptr; const int* step_ptr = nullptr; const float* m_tab = nullptr;
  float w = 1.f; int pred = 0; bool guided = false;
  float q = 1.f, floor = 1.f, cap = 0.f;
  float* q_out = nullptr; float* tab = nullptr; bool init_m = false;
};
int launch_win_quantile(const WinQuantile& qa, int B, int64_t per, const WinStatScratch& S, hipStream_t s);
// ---- k_group.hip: mixture consistency over the P members of G groups, between the forward and the update.  The batch
// is member-major (member p of group g: row p * G + g of x_t / net / x0_out, G * per floats apart); mix: row g of the caller's ms2_cond.
// x0_out (may alias net) receives the projected x0 estimate of every member, formed from (x_t, net) under objective `pred` with row [sa, sb]
// of coef (step_ptr: the row the device-side step counter names); mode: DQ_CONSIST_*; 0 < strength <= 1.  Any 4-byte aligned tensors;
// 16-byte accesses iff per % 4 == 0 and every tensor is 16-byte aligned.
struct GroupProject {
  const float* x_t = nullptr; const float* net = nullptr; float* x0_out = nullptr; const float* mix = nullptr;
  const float* coef = nullptr; const int* step_ptr = nullptr;
  int pred = 0, normalize = 0;  // pred: DQ_PRED_*, what `net` is
  int G = 0, P = 0; int64_t per = 0;
  int mode = 0; float strength = 1.f;
};
bool group_mode_ok(int mode);
bool group_strength_ok(float strength);  // (false for NaN)
int launch_group_project(const GroupProject& a, hipStream_t s);
// ---- k_noise.hip: out (B, per_window) = the normals of draw index `draw` (the generator of the STOCHASTIC update above)
int launch_randn(float* out, const int64_t* ids, const uint64_t* seed_dev, int draw, int B, int64_t per_window, hipStream_t s);
// ---- k_cond_drop.hip: out (B, per) = in with window b replaced by null_value iff the third Philox word of (seed, id, draw) < floor(p 2^32)
int launch_cond_drop(const float* in, float* out, const int64_t* ids, const uint64_t* seed_dev, int draw, double p, float null_value, int B,
                     int64_t per, hipStream_t s);
// ---- k_adamw.hip: global-norm clip + AdamW over flat buffers of n floats (partials: MSE_MAX_BLOCKS floats of scratch).  step_dev / lr_dev
// null: lr and the step count t >= 1 are the host's; else both live in device memory (graph replay): *step_dev is incremented, then used,
// lr_dev is a (hi, lo) float pair, and the step's scalars are kept at partials[MSE_MAX_BLOCKS - 8 ..].  ema (nullable): an exponential
// moving average of the parameters updated in the same pass, ema <- ema + w_t (p_new - ema), w_t = (float)(1 - beta_t), beta_t =
// min(ema_decay, (1 + t) / (10 + t)) with ema_warmup, ema_decay without (p, m, v, the norm: the same bits with and without it; the device
// variant keeps w_t at index 3 of its scalars).  gnorm_out (nullable): the pre-clip norm.
struct AdamwStep {
  float* p = nullptr; const float* g = nullptr; float* m = nullptr; float* v = nullptr; float* ema = nullptr;
  int64_t n = 0;
  float* partials = nullptr;
  float gscale = 1.f, max_norm = 0.f;
  double lr = 0.0; int step = 0;                               // the host's scalars, or
  const float* lr_dev = nullptr; int* step_dev = nullptr;    // the device's
  double b1 = 0.0, b2 = 0.0, eps = 0.0, wd = 0.0;
  float ema_decay = 0.f; int ema_warmup = 0;
  float* gnorm_out = nullptr;
};
int launch_adamw(const AdamwStep& a, hipStream_t s);
// ---- k_metrics.hip: per-window reconstruction metrics of pred against target (B, RT, MZ) -> out (B, METRIC_COUNT)
constexpr int METRIC_COUNT = 9;         // DQ_METRIC_COUNT
constexpr int METRIC_ROW_SEG = 4096;    // m/z columns of a scan one wave of k_metric_rows sums
constexpr int METRIC_COL_ROWS = 64;     // scans of a column one lane of k_metric_cols sums
constexpr int METRIC_ROW_MOMENTS = 10;  // doubles per (scan, segment)
constexpr int METRIC_COL_MOMENTS = 5;   // doubles per (column, scan chunk)
int64_t recon_metrics_scratch_bytes(int B, int RT, int MZ);
int launch_recon_metrics(const float* pred, const float* target, float* out, void* scratch, int64_t scratch_bytes, int B, int RT, int MZ,
                         hipStream_t s);

// ---- k_conv.hip
enum ConvMode { CONV_S1 = 0, CONV_DOWN = 1, CONV_UP = 2 };  // stride-1 'same' | k4 s2 p1 | nearest x2 then k3 p1
enum Act { ACT_NONE = 0, ACT_SILU = 1, ACT_GELU = 2, ACT_SOFTPLUS = 3 };  // ACT_SOFTPLUS: the network's final_conv only (k_conv_fwd<1, 1, 0>)

struct ConvFwd {
  // input = channel-concat of A (cinA) and B (cinB); tensors are (rows, C, n) with n contiguous
  const float* inA = nullptr; const float* inB = nullptr; int cinA = 0, cinB = 0;
  const float* w = nullptr;     // (cout, cinA+cinB, K)
  const float* bias = nullptr;  // (cout) or null
  int cout = 0, K = 1, mode = CONV_S1;
  int rows = 0, n_in = 0, n_out = 0;
  float* u_out = nullptr;       // pre-norm conv output (saved for backward) or null
  float* y_out = nullptr;
  const float* g = nullptr;     // RMSNorm gain (cout) or null => no norm
  const float* ss = nullptr;    // per-sample [scale(cout) | shift(cout)] or null
  int ss_stride = 0, rows_per_sample = 1;
  int act = ACT_NONE;
  // residual added after the activation: identity (resA has cout channels, res_w null) or 1x1 conv over cat(resA,resB)
  const float* resA = nullptr; const float* resB = nullptr; int rcinA = 0, rcinB = 0;
  const float* res_w = nullptr; const float* res_b = nullptr;
};
int launch_conv_fwd(const ConvFwd& a, hipStream_t s);

// pointwise backward of [RMSNorm -> scale/shift -> act] (any of them optional): du from (u, dy)
struct BlockBwd {
  const float* u = nullptr; const float* dy = nullptr; float* du = nullptr;
  int C = 0, rows = 0, n = 0, rows_per_sample = 1;
  const float* g = nullptr; float* dg = nullptr;                           // norm gain and its grad (+=)
  const float* ss = nullptr; float* dss = nullptr; int ss_stride = 0;     // per-sample scale/shift and grads (+=)
  int act = ACT_NONE;
  float* dbias = nullptr;  // optional: sum of du over rows and positions (+=)
  int accumulate = 0;      // 1: du += instead of du =
  const float* add_src = nullptr;  // accumulate: the addend is read from HERE instead of du (du = add_src + d; du itself is only written)
  // per-block partial sums [dg | dscale | dshift | dbias] (needed when any of dg / dss / dbias is set): >= 64 * groups * 4 C
  // floats; the launcher sums them in block order right behind the kernel (no float atomics: repeatable to the bit)
  float* part = nullptr; int64_t part_floats = 0;
  struct PartReduce* defer_reduce = nullptr;  // nullable: the launcher hands the reduction of `part` back instead of launching it (the caller runs it, e.g. on a side stream)
};
int launch_block_bwd(const BlockBwd& a, hipStream_t s);

// ordered sums of per-block partials part[(b * gx + x) * nv + i] (b < B groups, x < gx blocks per group): up to three "global"
// segments [start, start + len) -> dst[j] += sum over every block, and one per-group segment [s0, s0 + sn) ->
// sdst[b * sstride + j] += sum over the group's blocks.  Fixed summation order.
struct PartReduce {
  const float* part = nullptr; int B = 0, gx = 0, nv = 0;
  int nseg = 0; int seg_start[3] = {0, 0, 0}, seg_len[3] = {0, 0, 0}; float* seg_dst[3] = {nullptr, nullptr, nullptr};
  int s0 = 0, sn = 0; float* sdst = nullptr; int sstride = 0;
};
int launch_part_reduce(const PartReduce& a, hipStream_t s);

// dX (+=) of a conv: dinA/dinB receive the gradient of the concat input (either may be null => skipped)
struct ConvBwdData {
  const float* du = nullptr; const float* w = nullptr;
  int cout = 0, K = 1, mode = CONV_S1, rows = 0, n_in = 0, n_out = 0;
  float* dinA = nullptr; float* dinB = nullptr; int cinA = 0, cinB = 0;
  int accumulate = 1;  // 1: += ; 0: =
};
int launch_conv_bwd_data(const ConvBwdData& a, hipStream_t s);

// dW (+=) and dbias (+=; optional) of a conv: per-block partials + an ordered reduce (no atomics)
struct ConvWgrad {
  const float* du = nullptr; const float* inA = nullptr; const float* inB = nullptr; int cinA = 0, cinB = 0;
  int cout = 0, K = 1, mode = CONV_S1, rows = 0, n_in = 0, n_out = 0;
  float* dw = nullptr; float* dbias = nullptr;
  float* scratch = nullptr; int64_t scratch_floats = 0;  // >= WGRAD_MAX_PARTS * (cout*cin*K + cout) floats
};
constexpr int WGRAD_MAX_PARTS = 512;
// the ordered sum of nblk slots [dW (nelem_w) | dbias (cout)] into dw / dbias (+=): k_wgrad_reduce with one item
int launch_wgrad_reduce(const float* part, int nblk, int nelem_w, int cout, float* dw, float* dbias, hipStream_t s);
int launch_conv_wgrad(const ConvWgrad& a, hipStream_t s);
bool conv_wgrad_vec4(const ConvWgrad& a);  // launch_conv_wgrad takes k_conv_wgrad_v4 (4 positions per thread and step), not k_conv_wgrad
// up to three stride-1 convs over the same (rows, n) in one launch + one merged reduce (each with its own scratch region)
int launch_conv_wgrad_multi(const ConvWgrad* w, int count, hipStream_t s);

// backward of the Softplus behind final_conv (1x1, cin -> 1, with bias): dpre (rows, n) = dy * softplus'(pre), the pre-activation
// recomputed from the conv's input fin (rows, cin, n), weight w (cin) and bias b (1) -- nothing of the forward is stored for it
int launch_softplus_head_bwd(const float* fin, const float* w, const float* b, int cin, const float* dy, float* dpre, int rows, int n,
                             hipStream_t s);

// ---- a ResnetBlock's operands (k_res*.hip; k_level.hip reads the fields of its blocks)
struct ResFwd {
  const float* inA = nullptr; const float* inB = nullptr; int cinA = 0, cinB = 0;  // input = cat(A, B)
  const float* w1 = nullptr; const float* b1 = nullptr; const float* g1 = nullptr;   // block1 conv (C, cin, 3), bias, norm gain
  const float* w2 = nullptr; const float* b2 = nullptr; const float* g2 = nullptr;   // block2 conv (C, C, 3)
  const float* wr = nullptr; const float* br = nullptr;                              // res_conv (C, cin) or null => identity
  const float* ss = nullptr; int ss_stride = 0;                                      // per-sample [scale(C) | shift(C)] of block1
  float* u1 = nullptr; float* a1 = nullptr; float* u2 = nullptr;                     // saved for the backward (nullable)
  float* out = nullptr;
  int C = 0, rows = 0, n = 0, rows_per_sample = 1;
};
struct ResBwd {
  const float* dout = nullptr; const float* u1 = nullptr; const float* u2 = nullptr;
  const float* w1 = nullptr; const float* w2 = nullptr; const float* wr = nullptr;
  const float* g1 = nullptr; const float* g2 = nullptr; const float* ss = nullptr; int ss_stride = 0;
  float* du1 = nullptr; float* du2 = nullptr;          // written (the weight-gradient kernels read them)
  float* dA = nullptr; float* dB = nullptr; int cinA = 0, cinB = 0;  // += gradient of the block input (nullable)
  // dA_store / dB_store: this launch is the FIRST writer of that gradient tensor in the backward pass -> plain store, the old
  // contents (zeros) are not read (13 MB per tensor and launch at the wide levels)
  int dA_store = 0, dB_store = 0;
  float* dg1 = nullptr; float* dg2 = nullptr; float* dss = nullptr;  // destinations of the ordered sums (res_part_reduce)
  // gpart: every block's sums go to gpart[block][4 C] = [dg2 | dg1 | dscale | dshift] (block = sample * blocks_per_sample + x)
  // instead of float atomics (2 C of them per block on one cache line from 3,200 blocks cost 0.17 ms per step, and atomics
  // are not repeatable); *gblocks receives the blocks per sample; launch_part_reduce (res_part_reduce) adds the ordered sums
  // to dg2 / dg1 / dss
  float* gpart = nullptr; int64_t gpart_floats = 0; int* gblocks = nullptr;
  int C = 0, rows = 0, n = 0, rows_per_sample = 1;
};
// Which ResnetBlock kernel runs (in order of preference).  Forward: k_res_rt.hip, a one-block k_level_fwd launch (LEVEL), k_res_v4.hip or the
// conv launches of dq_ops.hip (UNFUSED).  Backward: k_res_{wg,rt,rows,cp}.hip, k_res.hip (PLAIN) or UNFUSED; wg: the block's buffers were
// laid out for k_res_bwd_wg (ResBuf::wpart_floats != 0).
enum ResFwdForm { RES_FWD_RT, RES_FWD_LEVEL, RES_FWD_V4, RES_FWD_UNFUSED };
ResFwdForm res_fwd_form(int C, int cinA, int cinB, bool has_wr, int rows, int n, int rows_per_sample);
enum ResBwdForm { RES_BWD_WG, RES_BWD_RT, RES_BWD_ROWS, RES_BWD_CP, RES_BWD_PLAIN, RES_BWD_UNFUSED };
ResBwdForm res_bwd_form(const ResBwd& a, bool wg);
// k_res_rt.hip: the bottleneck's 16-channel blocks (one RT row per sample, identity residual, no skip input) with the RT position as the lane
// column of v_mfma_f32_16x16x4
bool res_rt_usable(int C, int cinA, int cinB, bool has_wr, int rows_per_sample);
// the front of the bottleneck's Residual(PreNorm(Attention)) behind the first block: xn = RMSNorm(out) gn -> qv = W_qv xn (B, 256, RT), RoPE on
// q; k = W_k ms1f (B, 128, RT) + RoPE when kk is given
struct ResRtQkv {
  const float* gn = nullptr; const float* wqv = nullptr; float* xn = nullptr; float* qv = nullptr; const float* rope = nullptr;
  const float* wk = nullptr; const float* ms1f = nullptr; float* kk = nullptr;
};
// the back of the attention with the SECOND block: forward -- the block's input attn_out = res + W_o o + b_o is formed in the launch (and written
// to `out`); backward -- d o = W_o^T d attn_out follows the block's d x
struct ResRtOut {
  const float* o = nullptr; const float* w = nullptr; const float* b = nullptr; const float* res = nullptr; float* out = nullptr;  // forward
  float* d_o = nullptr;                                                                                                              // backward
};
int launch_res_rt_fwd(const ResFwd& a, hipStream_t s, const ResRtQkv* q = nullptr, const ResRtOut* ao = nullptr);
// the back of that front in front of the first block's backward: d out = add + PreNorm^T(W_qv^T RoPE^T(dqv)); d gn partials to
// gn_part[(sample * gblocks + workgroup) * 16 + c] (launch_part_reduce)
struct ResRtPre {
  const float* dqv = nullptr; const float* wqv = nullptr; const float* x = nullptr; const float* gn = nullptr; const float* add = nullptr;
  const float* rope = nullptr; float* gn_part = nullptr; int64_t gn_part_floats = 0;
};
int launch_res_rt_bwd(const ResBwd& a, hipStream_t s, const ResRtPre* q = nullptr, const ResRtOut* ao = nullptr);
// k_res_cp.hip: channel-parallel backward for the deep levels (n <= 8, C = 12 / 16)
bool res_cp_usable(int n, int C, int cinA, int cinB);
int launch_res_bwd_cp(const ResBwd& a, hipStream_t s);
// k_res_rows.hip: the deep levels' backward data path with the m/z row as the lane column of v_mfma_f32_16x16x4 (12 / 16 channels, rows of
// 2 / 4 / 8 positions, 16-byte aligned tensors)
bool res_rows_bwd_usable(const ResBwd& a);
int res_rows_bwd_min_rows();  // res_rows_bwd_usable takes this form from that many rows on (option res_rows_bwd_min_rows)
int launch_res_rows_bwd(const ResBwd& a, hipStream_t s);
// k_res_v4.hip: 4-positions-per-thread forward for the wide levels (C = 4 / 8, n >= 8)
bool res_v4_usable(int n, int C, int cinA, int cinB);
int launch_res_fwd_v4(const ResFwd& a, hipStream_t s);
enum LevelPre { LEVEL_PRE_NONE = 0, LEVEL_PRE_DOWN = 1, LEVEL_PRE_UP = 2, LEVEL_PRE_S1 = 3, LEVEL_PRE_INIT = 4 };
enum FinalAct { FINAL_IDENTITY = 0, FINAL_SOFTPLUS = 1 };  // = DQ_FINAL_* of include/dq_hip.h (Plan::final_act)
// k_level.hip: [resample conv that produces the level's input] -> ResnetBlock (-> ResnetBlock) in ONE launch, convolutions on the
// matrix pipe (rows of 1..64 positions).  blk[i].inA / cinA are unused (a block's first input is in registers); blk[i].out == null:
// that block's output is not written (inference, up path); pre_out: where the input stage's result is kept (training) or null.
struct LevelFwd {
  const float* in = nullptr; int cp = 0;                    // stage input (rows, cp, n_in); NONE: the first block's input (rows, C, n)
  const float* pw = nullptr; const float* pb = nullptr;     // stage conv weight (C, cp, K) and bias (C)
  const float* params = nullptr;                            // the flat parameter buffer every weight / bias / gain pointer points into
  float* pre_out = nullptr;
  int pre = LEVEL_PRE_NONE, nblocks = 1;
  ResFwd blk[2];
  // LEVEL_PRE_INIT (C == 4, inference): in = x_t (rows, n); cond = the mixture (rows, n), normalised as cond * cm + ca and conditioned with
  // init_cond_proj's per-sample [scale, shift] at ss_init (same buffer / stride as the blocks' vectors); pw / pb = init_conv (4, 2, 7);
  // pre_out = h0 (always written)
  const float* cond = nullptr; float cm = 1.f, ca = 0.f; const float* ss_init = nullptr;
  // ... in a train step the stage also stores its two input channels [conditioned mixture | x_t] as cat0 (rows, 2, n): the init conv's weight
  // gradient and the input affine's backward read them (what k_prep_inputs + k_conv_fwd<4,7,0> produced in two launches in front of this one)
  float* cat0_out = nullptr;
  // ... and may form x_t itself (model.py:349-352, k_q_sample's arithmetic): in = x0 (rows, n), qs_noise (rows, n), qs_ab = the alpha-bar table,
  // qs_t = the samples' timesteps, qs_norm: x0 -> 2 x0 - 1 first
  const float* qs_noise = nullptr; const float* qs_ab = nullptr; const int64_t* qs_t = nullptr; int qs_norm = 0;
  // head epilogue (C == 4, inference; behind the last block): eps = final_conv(out) (ew (1, 4, 1), eb) -> eps_out (nullable), and with
  // x_t set the DDIM update of model.py:265-289 into x_out (coef: [sa, sb, sap, sbp] rows; step_ptr nullable: row index on the device)
  const float* ew = nullptr; const float* eb = nullptr; float* eps_out = nullptr;
  const float* x_t = nullptr; float* x_out = nullptr; const float* coef = nullptr; const int* step_ptr = nullptr; int pred = 0;
  // training head (with ew / eb; the block's output is still written): loss_z = the regression target (rows, n).  d = eps - z; the squared-error
  // sums go to loss_part, one float per WAVE of the grid (*loss_parts_out receives their number: sum them in index order); grad_out (rows, n) =
  // d * loss_gscale (= d loss / d eps) -- times softplus'(pre) under final_act = FINAL_SOFTPLUS: always d loss / d (final_conv's output, before
  // the activation) -- and dout (rows, 4, n) = ew[c] * grad_out (final_conv's backward data path): what k_conv_fwd<1,1,0>,
  // k_mse_fwd_bwd and k_conv_bwd_data<4,1,0> did in three launches behind this one
  const float* loss_z = nullptr; float* loss_part = nullptr; float* grad_out = nullptr; float* dout = nullptr; float loss_gscale = 0.f;
  int* loss_parts_out = nullptr;
  // ... under the v objective (vt_x0 set): loss_z is the NOISE and the target z = sa_b * noise - sb_b * (x0 * vt_tm + vt_ta),
  // sa_b = sqrt(vt_ab[vt_t[b]]), sb_b = sqrt(1 - vt_ab[vt_t[b]]), is formed per element in the launch (never written); vt_lw (nullable: all
  // ones) weights sample b's squared error and gradient by vt_lw[vt_t[b]] -- k_mse_fwd_bwd<MseV>'s arithmetic
  const float* vt_x0 = nullptr; const float* vt_ab = nullptr; const int64_t* vt_t = nullptr; const float* vt_lw = nullptr; float vt_tm = 1.f, vt_ta = 0.f;
  // output activation of the head (FINAL_IDENTITY | FINAL_SOFTPLUS, with ew): with Softplus, eps_out, the DDIM update and the training
  // head's loss see y = softplus(final_conv(out))
  int final_act = 0;
  int C = 0, rows = 0, n = 0, rows_per_sample = 1;
  // nullable: this launch's MFMA operand image (level_img_floats floats, 16-byte aligned) as launch_level_images built it from the SAME
  // parameter values -- the kernel's workgroups then copy it to LDS instead of gathering it from the parameter tensors themselves
  const float* img = nullptr;
};
// the shapes launch_level_fwd takes (the (C, stage, stage input width) triples: k_level.hip's table of built instantiations): block b's
// input is cat(x of C channels, cinB[b] skip channels), has_wr[b]: it has a res_conv
bool level_fwd_usable(int C, int rows, int n, int rows_per_sample, int pre_mode, int cp, int nblocks, const int* cinB, const bool* has_wr);
bool level_fwd_usable(const LevelFwd& a);
int launch_level_fwd(const LevelFwd& a, hipStream_t s);
// what launch_level_fwd and launch_tiny_fwd (`who`: the message prefix) ask of a block: operands present, its scale / shift vector in the buffer
// at ssb with that stride, parameters inside the flat buffer.  poff: a parameter's offset in the flat buffer, -1 for null.  (k_level.hip)
int check_level_block(const char* who, const ResFwd& r, const float* params, const float* ssb, int ss_stride);
inline int poff(const float* params, const float* ptr) { return ptr ? (int)(ptr - params) : -1; }
constexpr int LEVEL_LOSS_PARTS = 8192;     // floats behind LevelFwd::loss_part (one per wave of a resident round: 6 x 256 workgroups x 4)
constexpr int LEVEL_IMG_MAX = 20;          // launches per launch_level_images call
constexpr int LEVEL_IMG_FLOATS = 8192;     // upper bound of level_img_floats over the built instantiations (16 channels, 32-channel blocks)
int64_t level_img_floats(const LevelFwd& a);
int launch_level_images(const LevelFwd* calls, int count, hipStream_t s);  // writes calls[i].img (must be set) for every call, ONE launch
int launch_res_fwd(const ResFwd& a, hipStream_t s);  // the RT and V4 forms
int launch_res_bwd(const ResBwd& a, hipStream_t s);

// k_tiny.hip: the levels with rows of 1 or 2 positions as a chain of dense layers on v_mfma_f32_32x32x2 (lane = (position | row half, row),
// register = channel): [resample conv] -> ResnetBlock -> ResnetBlock in ONE launch like k_level_fwd and, at n == 1,
// Residual(PreNorm(LinearAttention)) (linear over one position) and the last down level's k3 conv written in the bottleneck's
// (B, C, RT) layout.  `lv` carries the stage and the blocks exactly as for launch_level_fwd (its img field is unused).
struct TinyFwd {
  LevelFwd lv;
  int la = 0;  // n == 1: the level's LinearAttention rides along
  const float* w_qkv = nullptr; const float* w_out = nullptr; const float* b_out = nullptr; const float* g_pre = nullptr; const float* g_out = nullptr;
  float* la_y = nullptr; float* la_ypre = nullptr;  // (rows, C, 1); la_ypre nullable (training: the pre-norm output the backward reads)
  const float* post_w = nullptr; const float* post_b = nullptr; float* post_out = nullptr;  // n == 1, behind the LinearAttention: k3 conv (C, C, 3) -> (B, C, RT)
  int in_folded = 0;          // LEVEL_PRE_NONE, n == 1: lv.in is (B, C, RT)
  float* in_copy = nullptr;   // nullable: the input again as (rows, C, 1) (training: the backward reads it in that layout)
  const float* img = nullptr; // operand image (tiny_img_floats floats, 16-byte aligned) from launch_tiny_images on the SAME parameter values
};
constexpr int TINY_IMG_MAX = 6;  // four forward launches + two backward ones
constexpr int TINY_IMG_FLOATS = 16384;  // (whole rounds of 256 x 16 bytes: the kernels copy a slot without guards)
bool tiny_fwd_usable(const TinyFwd& t);
int64_t tiny_img_floats(const TinyFwd& t);
int launch_tiny_images(const TinyFwd* calls, int count, hipStream_t s);
int launch_tiny_fwd(const TinyFwd& t, hipStream_t s);

// k_tiny.hip, backward: the DATA path of a level with rows of one position in one launch ([last down level's k3 conv] -> LinearAttention ->
// ResnetBlock 1 -> ResnetBlock 0 -> [Downsample]); weight gradients stay with the side-stream kernels, which read the d u1 / d u2 / d rs /
// d out tensors this launch writes; norm gains and per-sample d(scale, shift) leave as ResBwd::gpart partials (*gblocks = blocks per
// sample), the LinearAttention's gradients as one k_linattn_bwd1-format slot per workgroup (tiny_bwd_slots of them).
struct TinyBwd {
  const float* params = nullptr; const float* img = nullptr;
  int C = 0, rows = 0, rows_per_sample = 1, pre = LEVEL_PRE_NONE, cp = 0, cs = 0;
  const float* x = nullptr; const float* ypre = nullptr; const float* dy = nullptr;      // block-1 output, saved pre-norm LinearAttention output, d la
  const float* w_qkv = nullptr; const float* w_out = nullptr; const float* g_pre = nullptr; const float* g_out = nullptr;
  float* la_part = nullptr; int64_t la_part_floats = 0;
  const float* post_w = nullptr; const float* dmid = nullptr; float* drs_out = nullptr;   // LEVEL_PRE_DOWN (last down level): its k3 conv, d mid_in (B, C, RT), d rs (rows, C) out
  float* dfold = nullptr;                                                                 // LEVEL_PRE_NONE: input gradient as (B, C, RT)
  float* din_rows = nullptr; float* dprev = nullptr; const float* stage_w = nullptr;      // LEVEL_PRE_DOWN: input gradient (rows, C); previous level's d la (rows, cp, 2) +=; Downsample weight
  const float* r0out_g = nullptr;                                                         // nullable: skip gradient already in d r0.out
  // LEVEL_PRE_NONE, nullable pair: the Upsample conv BEHIND this level (nearest x2 + k3, 16 -> 16, rows of 2 positions) -- its backward data path runs
  // in front of the LinearAttention part: d la = Upsample^T d rs with dup = d rs (rows, C, 2), and dy is not read
  const float* up_w = nullptr; const float* dup = nullptr;
  struct Blk {
    const float* w1 = nullptr; const float* w2 = nullptr; const float* wr = nullptr; const float* g1 = nullptr; const float* g2 = nullptr;
    const float* ss = nullptr; int ss_stride = 0;
    const float* u1 = nullptr; const float* u2 = nullptr; float* du1 = nullptr; float* du2 = nullptr;
    float* dB = nullptr; int dB_acc = 0; float* dout_st = nullptr; float* gpart = nullptr; int64_t gpart_floats = 0;
  } blk[2];
  int* gblocks = nullptr;
};
bool tiny_bwd_usable(const TinyBwd& t);
int tiny_bwd_slots(const TinyBwd& t);
int64_t tiny_bwd_img_floats(const TinyBwd& t);
int launch_tiny_bwd_images(const TinyBwd* calls, int count, hipStream_t s);
int launch_tiny_bwd(const TinyBwd& t, hipStream_t s);
// k_res_wg.hip: ResnetBlock backward of the wide levels (C = 4 / 8 only, rows of 8..64 positions) with the block's weight gradients formed
// in the same launch on the 4x4x1 matrix pipe.  Every workgroup leaves [c1.w | c1.b | g1 | c2.w | c2.b | g2 | res.w | res.b | dscale |
// dshift] in its own slot of `part`; launch_res_wg_reduce adds the slots up in block order into the flat gradient buffer (the
// block's parameters are contiguous there, in this order) and into the per-sample d(scale, shift).
struct ResBwdWg {
  const float* dout = nullptr; const float* u1 = nullptr; const float* u2 = nullptr;
  const float* inA = nullptr; const float* inB = nullptr; int cinA = 0, cinB = 0;   // the block's input (forward activations)
  const float* w1 = nullptr; const float* w2 = nullptr; const float* wr = nullptr;
  const float* g1 = nullptr; const float* g2 = nullptr; const float* ss = nullptr; int ss_stride = 0;
  float* dA = nullptr; float* dB = nullptr; int dA_store = 0, dB_store = 0;         // as ResBwd
  float* part = nullptr; int64_t part_floats = 0;                                   // >= res_wg_part_floats(...)
  float* dparams = nullptr;   // gradient of block1.proj.weight in the flat gradient buffer (the slot's first tensor)
  float* dss = nullptr;       // this block's [dscale | dshift] of sample 0 (stride ss_stride)
  int C = 0, rows = 0, n = 0, rows_per_sample = 1;
  int tiles_ps = 0, tpb = 0, nv = 0;  // (filled by the launcher)
};
struct ResWgReduce { const float* part; int B, gx, nv, nglob, C; float* dst; float* dss; int ss_stride; };
constexpr int RES_WG_REDUCE_MAX = 32;
struct ResWgReduceMulti { ResWgReduce it[RES_WG_REDUCE_MAX]; };
bool res_wg_usable(int n, int C, int cinA, int cinB, int rows_per_sample);
int64_t res_wg_part_floats(int C, int cin, bool wr, int B, int rows_per_sample, int n);
// launches the backward; *red_out receives the descriptor of the slot reduction (launch_res_wg_reduce: right away or collected)
int launch_res_bwd_wg(const ResBwdWg& a, hipStream_t s, ResWgReduce* red_out);
int launch_res_wg_reduce(const ResWgReduce* items, int count, hipStream_t s);
// k_conv_wg.hip: backward of a level's resample conv (data gradient + weight / bias gradient in one launch, matrix pipe).  `n` is the
// conv's OUTPUT row length; pre = LEVEL_PRE_DOWN (k4 s2) / _UP (nearest x2 + k3) / _S1 (k3).  Slots [dW | dbias] -> launch_res_wg_reduce.
struct ConvBwdWg {
  const float* dy = nullptr;   // (rows, C, n) gradient of the conv output
  const float* in = nullptr;   // (rows, cp, n_in) forward input
  const float* w = nullptr;    // (C, cp, K)
  float* din = nullptr; int accumulate = 0;   // (rows, cp, n_in): = or += ; null: not needed
  float* part = nullptr; int64_t part_floats = 0;
  float* dparams = nullptr;    // gradient of the conv weight in the flat gradient buffer (the bias gradient follows it)
  int C = 0, pre = 0, cp = 0, rows = 0, n = 0, rows_per_sample = 1;
  int tiles_ps = 0, tpb = 0, nv = 0;  // (filled by the launcher)
};
bool conv_wg_usable(int C, int pre, int cp, int n, int rows_per_sample);
int64_t conv_wg_part_floats(int C, int pre, int cp, int B, int rows_per_sample, int n);
int launch_conv_bwd_wg(const ConvBwdWg& a, hipStream_t s, ResWgReduce* red_out);
// the descriptor of a fused ResnetBlock backward's partial sums for launch_part_reduce
inline PartReduce res_part_reduce(const float* gpart, int gx, int B, int C, float* dg2, float* dg1, float* dss, int ss_stride) {
  PartReduce r;
  r.part = gpart; r.B = B; r.gx = gx; r.nv = 4 * C; r.nseg = 2;
  r.seg_start[0] = 0; r.seg_len[0] = C; r.seg_dst[0] = dg2;
  r.seg_start[1] = C; r.seg_len[1] = C; r.seg_dst[1] = dg1;
  r.s0 = 2 * C; r.sn = 2 * C; r.sdst = dss; r.sstride = ss_stride;
  return r;
}

// standalone RMSNorm forward (PreNorm of the bottleneck attention)
int launch_rmsnorm_fwd(const float* x, const float* g, float* y, int C, int rows, int n, hipStream_t s);

// (rows=B*RT, C, n) <-> (B, C*n, RT) fold of the bottleneck (unet1d.py:1144-1148); add=1 accumulates; pitch: row pitch of the
// (B, C*n, .) side (0 = RT; the wide bottleneck pads it, and the pad columns of a to_mid output are zeroed)
int launch_fold(const float* in, float* out, int B, int RT, int cn, int to_mid, int add, hipStream_t s, int pitch = 0);

// first layer inputs: cat0 = [cond_n*(scale+1)+shift, x] as (rows, 2, MZ); ms1n = ms1*cm+ca
int launch_prep_inputs(const float* x, const float* cond, const float* ms1, const float* ss, int ss_stride, int ss_off, float cm,
                       float ca, float* cat0, float* ms1n, int B, int RT, int MZ, hipStream_t s);
int launch_ms1_norm(const float* ms1, float cm, float ca, float* ms1n, int64_t n, hipStream_t s);  // ms1n = ms1 * cm + ca
// ---- k_ms1_feat.hip: attn_cond_proj.1.0 (k7 'same', M1 -> 8 channels) + GELU on a multi-channel MS1 (B, RT, M1), M1 contiguous (M1 > 1)
constexpr int MS1_MAX_CHANNELS = 4096;
constexpr int MS1_FWD_TP = 8, MS1_FWD_WAVES = 4;      // positions per wave / waves per workgroup of the forward
constexpr int MS1_WG_T = 64, MS1_WG_MAX_PARTS = 256;  // positions per unit / most slots of the weight gradient
struct Ms1FeatFwd {
  const float* ms1 = nullptr;                          // (B, RT, M1), raw: normalised on the fly as v * cm + ca
  const float* w = nullptr; const float* bias = nullptr;  // (8, M1, 7), (8)
  float cm = 1.f, ca = 0.f;
  float* ms1n_out = nullptr;  // nullable: the normalised MS1 (B, RT, M1) the weight gradient reads (training)
  float* u_out = nullptr;     // nullable: pre-activation (B, 8, RT)
  float* a_out = nullptr;     // GELU(u) (B, 8, RT)
  int B = 0, RT = 0, M1 = 0;
};
int launch_ms1_feat_fwd(const Ms1FeatFwd& a, hipStream_t s);
struct Ms1FeatWgrad {
  const float* ms1n = nullptr; const float* du = nullptr;  // (B, RT, M1) normalised, (B, 8, RT)
  float* dw = nullptr; float* dbias = nullptr;             // += (8, M1, 7), (8)
  float* part = nullptr; int64_t part_floats = 0;          // >= ms1_feat_wgrad_part_floats(B, RT, M1)
  int B = 0, RT = 0, M1 = 0;
};
int ms1_feat_wgrad_parts(int B, int RT, int M1);  // slots (= workgroups) of the launch
int64_t ms1_feat_wgrad_part_floats(int B, int RT, int M1);
int launch_ms1_feat_wgrad(const Ms1FeatWgrad& a, hipStream_t s);
// d(scale), d(shift) of init_cond_proj from dcat0 channel 0 (+= into dss; part: >= 64 * B floats of per-block partials)
int launch_prep_inputs_bwd(const float* dcat0, const float* cond, float cm, float ca, float* dss, int ss_stride, int ss_off, int B,
                           int RT, int MZ, float* part, int64_t part_floats, hipStream_t s);

// ---- k_wide.hip : the bottleneck when it is wide (mid_dim * downsampled_n channels not in {16, 32, 64}); tensors (B, C, P), P = RT
// padded to a multiple of 4, pad columns written as zeros
int launch_im2col3(const float* x, float* xcol, int B, int C, int RT, int P, hipStream_t s);                  // (B,C,P) -> (B,3C,P)
int launch_col2im3(const float* dxcol, float* dx, int B, int C, int RT, int P, int accumulate, hipStream_t s);  // transpose of it
int launch_repitch(float* dst, int dpitch, const float* src, int spitch, int64_t rows, int n, hipStream_t s);
int launch_zero_pads(float* x, int64_t rows, int RT, int P, hipStream_t s);  // (rows, P): columns t >= RT <- 0
int launch_wnorm_fwd(const float* u, const float* g, const float* ss, int ss_stride, int act, const float* res, float* y, int B, int C,
                     int RT, int P, hipStream_t s);
// scratch: B * (2 P + 2 C) floats; dg / dss / dbias +=
int launch_wnorm_bwd(const float* u, const float* dy, const float* g, const float* ss, int ss_stride, int act, float* du, float* dg,
                     float* dss, float* dbias, float* scratch, int B, int C, int RT, int P, hipStream_t s);
int launch_rowsum(const float* x, int64_t rows, int RT, int P, float* out, hipStream_t s);
int launch_sum_b(const float* part, int B, int C, float* dst, hipStream_t s);  // dst[c] += sum_b part[b][c]: launch_ordered_sum

// ---- k_tfm.hip : the index-order sum  out[i] (+)= sum_b part[b * stride + i], b = 0, 1, ... from 0 (k_partial_reduce; one thread per i)
int launch_ordered_sum(const float* part, int nb, int64_t stride, int n, float* out, int accumulate, hipStream_t s);

// ---- k_time.hip (declared in dq_unet.h: needs the plan)

// ---- k_linattn.hip
struct LinAttn {
  const float* x = nullptr; float* y = nullptr;  // (rows, C, n)
  const float* w_qkv = nullptr; const float* w_out = nullptr; const float* b_out = nullptr;
  const float* g_pre = nullptr; const float* g_out = nullptr;
  int C = 0, rows = 0, n = 0;
  float* ypre = nullptr;  // optional: pre-norm output Wo*out + b (rows, C, n), saved for the backward
  // optional: this layer's LA_PREP_FLOATS prepared weights from launch_linattn_prepare (W2 = Wo Wv per head and the MFMA operand
  // image of Wq | Wk); without it every block of the forward derives them itself (a 64-load-deep prologue per 4 rows)
  const float* prep = nullptr;
};
// rows the register-resident kernels take (k_linattn.hip / k_la_bwd.hip); any other length goes through the sweep kernels (k_la_long.hip)
inline bool la_short_row(int n) { return n <= 64 && (n & (n - 1)) == 0; }
// the kernel launch_linattn_fwd takes for these operands (values mirror DQ_LA_FWD_* of include/dq_hip.h; dq_linattn_forms asks the same)
enum LaFwdForm { LA_FWD_LONG, LA_FWD_SMALL, LA_FWD_ROWS, LA_FWD_REG };
LaFwdForm la_fwd_form(const LinAttn& a);
int launch_linattn_fwd(const LinAttn& a, hipStream_t s);
// k_la_small.hip: rows of 2 / 4 (/ 8) positions at 8 / 12 / 16 channels with a prepared image (LinAttn::prep): every product on
// v_mfma_f32_32x32x2 with lane = (channel half, row) and one group of registers per position
bool la_small_usable(int C, int n);
int la_small_min_rows();  // la_fwd_form takes this path from that many rows on
int launch_la_small_fwd(const LinAttn& a, hipStream_t s);
// k_la_rows_bwd.hip: the backward in the same spirit (one m/z row per lane column, every product on v_mfma_f32_16x16x4_f32); one slot per
// wave in the la_slot(C) layout, when the layer's prepared weights are at hand
struct LinAttnBwd;
bool la_rows_bwd_usable(int C, int n);
int la_rows_bwd_min_rows();
// k_la_rows_fwd.hip: the forward in the same layout (rows of 2 / 4 positions below la_small_min_rows)
bool la_rows_fwd_usable(int C, int n);
int launch_la_rows_fwd(const LinAttn& a, hipStream_t s);
int launch_la_rows_bwd(const LinAttnBwd& a, int max_slots, int* slots_out, hipStream_t s);
constexpr int LA_PREP_BOUNDED = 1024 + 4096;          // 1.0f when the layer's softmax logits are bounded by 64 for every input (k_linattn_prepare)
constexpr int LA_PREP_BF16 = 1024 + 4096 + 8;         // split-bf16 operand image of Wq | Wk for 4 / 8 channels: 2048 la_nu(C) <= 6144 dwords (k_linattn.hip)
constexpr int LA_PREP_SMALL = 1024 + 4096 + 8 + 6144;  // operand image of k_la_small (rows of <= 8 positions, C = 8 / 12 / 16): [q | k | W2][head][step < C / 2][64 lanes] <= 6144 floats
// operand image of k_la_rows_bwd (rows of 2 / 4 positions, C = 8 / 12 / 16; v_mfma_f32_16x16x4_f32 A operands): [head][lane][LA_ROWS_LANE_FLOATS] =
// [Wq log2(e): 8 | Wk log2(e): 8 | W2^T: 4 | Wq^T: 8 | Wk^T: 8] (the first three groups hold 2 CPL / 2 CPL / CPL values, CPL = C / 4; k_la_rows_bwd.hip has the index algebra)
constexpr int LA_ROWS_LANE_FLOATS = 36;  // (b128 reads at this lane pitch are bank-conflict-free)
constexpr int LA_PREP_ROWS = 1024 + 4096 + 8 + 6144 + 6144;
constexpr int LA_PREP_FLOATS = LA_PREP_ROWS + 4 * 64 * LA_ROWS_LANE_FLOATS;  // [w2: 4 * 16 * 16][wqk: 2 * 4 * 8 * 2 * 32][bounded, 7 unused][bf16 image][small-row image][rows-backward image]
struct LaPrepItem { const float* w_qkv; const float* w_out; int C; float* prep; const float* g_pre; };
constexpr int LA_PREP_MAX = 16;
struct PrepCopy { const float* src; float* dst; int n; };  // plain copies riding in the same launch (aligned weight slots)
constexpr int PREP_COPY_MAX = 4;
// all LinearAttention layers of a forward (+ up to PREP_COPY_MAX copies): one launch
int launch_linattn_prepare(const LaPrepItem* items, int count, hipStream_t s, const PrepCopy* copies = nullptr, int n_copies = 0);
struct LinAttnBwd {
  LinAttn f;
  const float* dy = nullptr; float* dx = nullptr;  // dx += (dx_store: the only writer of dx in this backward -> plain store)
  int dx_store = 0;
  const float* ypre = nullptr;                     // saved by the forward
  float* dyp = nullptr; float* dxh = nullptr;      // scratch (rows, C, n) each
  float* part = nullptr; int64_t part_floats = 0;  // per-wave dW partial slots: >= LA_MAX_WAVES * 512 * C floats
  // defer_reduce: rows of <= 64 positions leave their slots unreduced and report the slot count in *waves_out (0 when the
  // launch reduced them itself: the long-row path); the caller sums them later with launch_linattn_dw_reduce_multi, and then
  // part_floats only needs la_part_reserve(C)
  int defer_reduce = 0; int* waves_out = nullptr;
  float* dw_qkv = nullptr; float* dw_out = nullptr; float* db_out = nullptr; float* dg_pre = nullptr; float* dg_out = nullptr;
};
// rows of 128 / 256 positions (k_la_long.hip)
int launch_linattn_fwd_long(const LinAttn& a, hipStream_t s);
int launch_linattn_bwd_long(const float* x, const float* dyp, float* dxh, const float* w_qkv, const float* w_out, const float* g_pre,
                            float* part, int C, int rows, int n, int* waves_out, hipStream_t s);
constexpr int LA_MAX_WAVES = 2048;  // the backward grid is one resident round: <= 1024 waves, one partial slot each
// the kernel launch_linattn_bwd takes for these operands (values mirror DQ_LA_BWD_* of include/dq_hip.h)
enum LaBwdForm { LA_BWD_LONG, LA_BWD_ROWS, LA_BWD_REG };
LaBwdForm la_bwd_form(const LinAttnBwd& a);
int launch_linattn_bwd(const LinAttnBwd& a, hipStream_t s);
// the deferred slot reductions of up to LA_REDUCE_MAX LinearAttention backwards in ONE launch (grad += ordered slot sums)
// w2sum: 4 C C floats of scratch (the summed dW2 of the four heads; the launcher places it right behind the layer's slots);
// w_qkv / w_out: the layer's weights (dWv = Wo^T dW2, dWo = dW2 Wv^T are formed from the sum)
struct LaReduceItem {
  const float* part; int nslots, C; float* dw_qkv; float* dw_out; float* dg_out; float* db_out; float* dg_pre;
  float* w2sum; const float* w_qkv; const float* w_out;
};
// floats of one partial slot of a LinearAttention backward (k_la_bwd.hip, k_la_rows_bwd.hip, k_tiny.hip; a slot per workgroup or per wave):
// dWq | dWk (256 C) | dW2 of the four heads (4 C C) | d g_out | d b_out | d g_pre; la_slot_gains: where the three gain / bias sums start
constexpr int la_slot_gains(int C) { return 256 * C + 4 * C * C; }
constexpr int la_slot(int C) { return la_slot_gains(C) + 3 * C; }
// the reduce item of a launch that left `slots` slots at `part`: the summed-dW2 scratch lies right behind them
inline LaReduceItem la_reduce_item(float* part, int slots, int C, float* dw_qkv, float* dw_out, float* dg_out, float* db_out, float* dg_pre,
                                   const float* w_qkv, const float* w_out) {
  return LaReduceItem{part, slots, C, dw_qkv, dw_out, dg_out, db_out, dg_pre, part + (int64_t)slots * la_slot(C), w_qkv, w_out};
}
constexpr int LA_REDUCE_MAX = 16;
int64_t la_part_reserve(int C);  // floats of slot scratch one deferred launch with C channels can use
int launch_linattn_dw_reduce_multi(const LaReduceItem* items, int count, hipStream_t s);
// the slots of launch_linattn_bwd_long (512 C floats per wave: dWqkv | dWo), summed into the gradient buffers (+=)
int launch_linattn_dw_reduce(const float* part, int nslots, int C, float* dw_qkv, float* dw_out, hipStream_t s);

// ---- k_attn.hip : softmax attention over RT of the bottleneck (q,k,v,o in (B, 128, RT) conv layout)
int launch_rope(float* qk, const float* freqs, int B, int64_t batch_stride, int RT, float sign, hipStream_t s);
int launch_rope2(float* q, int64_t q_bs, float* k, int64_t k_bs, const float* freqs, int B, int RT, float sign, hipStream_t s);
int launch_attn_fwd(const float* q, int64_t q_bs, const float* k, int64_t k_bs, const float* v, int64_t v_bs, float* o, float* lse,
                    int B, int RT, hipStream_t s);
int launch_attn_bwd(const float* q, int64_t q_bs, const float* k, int64_t k_bs, const float* v, int64_t v_bs, const float* o,
                    const float* d_o, const float* lse, float* delta, float* dq, int64_t dq_bs, float* dk, int64_t dk_bs, float* dv,
                    int64_t dv_bs, int B, int RT, hipStream_t s);

}  // namespace dq
