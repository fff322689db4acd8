/* libdq_hip.so -- C ABI of the MI355X (gfx950) implementation of dquartic's DDIM hot path.
 *
 * The reference (Roestlab/diffusion-deconvolution-dia-msms-data, "dquartic") is pure PyTorch and has no FFI of
 * its own; its boundary for this path is the Python object protocol of dquartic/model/model.py and
 * dquartic/model/unet1d.py.  Each entry point below names the reference method whose arithmetic it replaces
 * (file:line relative to the reference checkout).  The host-side mirror of that protocol
 * (diffusion-deconvolution-dia-msms-data_amd/dquartic/) binds these symbols with ctypes; INTEGRATION.md shows the stub
 * a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only: device pointers (float* / int64_t*), sizes, a HIP stream passed as void*;
 *   - every call is asynchronous on the given stream and keeps no pointer after it returns, with two documented
 *     exceptions: dq_ddim_sample synchronises the stream twice on entry (its host-side coefficient / timestep tables must
 *     be on the device before the caller's arrays go out of scope, and a hipGraph capture must not see pending copies), and
 *     caches the captured step graph inside the plan;
 *   - the caller supplies every workspace (sizes from dq_unet_workspace_bytes / dq_tfm_workspace_bytes /
 *     dq_resblock_workspace_floats).  The library's only device allocation is made by the first call that uses a plan:
 *     two ~10 KB tables of parameter offsets (hipMalloc, freed by dq_plan_destroy); a side stream and its events are
 *     created by the first backward;
 *   - returns 0 on success; non-zero => dq_last_error() (thread-local text) says why;
 *   - tensors are contiguous fp32; MS2 windows are (B, RT, MZ) with MZ contiguous, MS1 chromatograms (B, RT),
 *     timesteps int64 (B);
 *   - parameters/gradients/AdamW moments are single flat fp32 buffers whose layout is described by
 *     dq_plan_param_info (tensor names == the reference's state_dict keys, reference registration order).  SURVEY 8b
 *     sketched a packed-weights handle (dq_weights_pack / dq_weights_free); the flat buffer replaces it: the caller's
 *     tensor IS the packed form, so there is nothing to pack, free or keep in sync;
 *   - calls that share a dq_plan must not run concurrently; distinct plans are independent.
 */
#ifndef DQ_HIP_H
#define DQ_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dq_plan dq_plan;

/* Text of the last error on this thread ("" if none). */
const char* dq_last_error(void);
/* ABI version of this header (bumped on any signature change).  2: pred_type arguments, dq_ddim_step_x0,
 * dq_mse_loss_weighted_fwd_bwd, dq_pair_batch.  3: dq_tfm_* (CustomTransformer), dq_gemm.
 * 4: dq_tfm_bwd takes an accumulate flag.  5: dq_ddim_sample takes num_timesteps (the plan no longer fixes T); stand-alone
 * building blocks (dq_rmsnorm_fwd, dq_time_mlp_fwd, dq_scale_shift_fwd, dq_prep_inputs_fwd, dq_conv_fwd, dq_resblock_*,
 * dq_rope, dq_attn_*); dq_train_step takes ms1_loss_weight, dq_ms1_loss_fwd_bwd;
 * dq_tfm_set_precision, dq_gemm_bf16x3.  8: dq_tfm_bwd_buckets, dq_tfm_num_buckets, dq_tfm_bucket_info.  9: dq_linattn_prepare,
 * dq_linattn_fwd_prepared.  10: dq_set_option, dq_get_option, dq_debug_side_tail_store (later, additive: dq_plan_set_final_act,
 * dq_plan_final_act, dq_get_option_effective, dq_resblock_forms, dq_linattn_forms, dq_linattn_bwd_store, dq_plan_create_ex,
 * dq_plan_attn_cond_channels, dq_ms1_feat_fwd, dq_ms1_feat_wgrad, dq_ms1_feat_wgrad_scratch_floats).  11: dq_conv_bwd,
 * dq_conv_bwd_workspace_floats, dq_conv_bwd_forms (later, additive: dq_adamw_clip_ema_step, dq_adamw_clip_ema_step_dev; dq_randn,
 * dq_ddim_step_sto, dq_ddim_coef_table, dq_ddim_sample_ex).  12: dq_debug_level_plan (later, additive: dq_gemm_ex,
 * dq_debug_gemm_plan; DQ_SAMPLER_*, dq_sampler_coef_table, dq_solver_step, dq_ddim_sample_solver; dq_debug_layout, dq_debug_mid_forms,
 * dq_debug_mid_fwd, dq_debug_mid_bwd; dq_tfm_layernorm_form and the stand-alone kernels of the transformer: dq_tfm_rope_add,
 * dq_tfm_cond_embed, dq_tfm_cond_embed_bwd, dq_tfm_time_features, dq_tfm_gelu, dq_tfm_gelu_bwd, dq_tfm_layernorm_fwd,
 * dq_tfm_layernorm_bwd, dq_tfm_softmax_rows, dq_tfm_softmax_rows_bwd, dq_tfm_colsum, dq_tfm_seqsum; the transformer's sampler:
 * dq_tfm_attn_form, dq_tfm_attn_fwd, dq_tfm_sample_workspace_bytes, dq_tfm_sample; the wide bottleneck alone: dq_wide_im2col3,
 * dq_wide_col2im3, dq_wide_repitch, dq_wide_norm_fwd, dq_wide_norm_bwd, dq_wide_norm_bwd_scratch_floats, dq_wide_rowsum, dq_wide_sum_b,
 * dq_debug_wide_mid_fwd, dq_debug_wide_mid_bwd; the transformer's held-out evaluation: dq_tfm_eval_workspace_bytes, dq_tfm_eval_step,
 * dq_q_sample_repeats, dq_mse_per_window_repeats, dq_tfm_kv_broadcast; classifier-free guidance: DQ_UPDATE_*, dq_guided_update,
 * dq_ms1_cond_drop, dq_ddim_sample_guided; K-component mixtures: dq_mix_batch_scratch_bytes, dq_mix_batch; the v objective: DQ_PRED_V,
 * dq_ddim_step_v, dq_solver_step_v, dq_guided_update_v, dq_ddim_sample_v, dq_mse_loss_v_fwd_bwd, dq_mse_per_window_v; whole
 * chromatograms: dq_run_window_count, dq_run_windows_scratch_bytes, dq_run_windows, dq_run_stitch; per-window sampler control:
 * dq_sample_stat_scratch_bytes, dq_window_rescale, dq_window_abs_quantile, dq_step_update_adaptive, dq_ddim_sample_adaptive; joint
 * sampling of a window's precursors: DQ_CONSIST_*, dq_group_project, dq_ddim_sample_joint; the time embedding and the input affine alone:
 * DQ_TBUF_*, dq_debug_time_fwd, dq_debug_time_bwd, dq_prep_inputs_bwd, dq_prep_inputs_bwd_scratch_floats; evaluating joint sampling:
 * dq_mix_group_batch_scratch_bytes, dq_mix_group_batch, DQ_GROUP_*, dq_group_metrics_scratch_bytes, dq_group_metrics).  13: a sampling call
 * crosses as one record, dq_sample_call: dq_ddim_sample and dq_tfm_sample take it, dq_ddim_sample_ex / _solver / _guided / _v / _adaptive /
 * _joint are gone (their arguments are the record's fields); dq_debug_sample_call_layout. */
int dq_abi_version(void);
#define DQ_ABI_VERSION 13

/* Process-wide tuning options (no reference counterpart: the reference has one code path per op).  The library reads NO environment
 * variable for its dispatch; what can be tuned is set here, takes effect from the next call on, and invalidates cached sampling graphs.
 *   "la_small_min_rows"     rows (B * RT) from which LinearAttention over m/z rows of 2 / 4 / 8 positions runs in the
 *                           one-register-group-per-position form (k_la_small.hip) instead of the register-resident one (k_linattn.hip);
 *                           < 0 (default): the device rule, one 32-row tile per SIMD (32,768 rows on MI355X)
 *   "la_rows_bwd_min_rows"  the same for its backward (k_la_rows_bwd.hip against k_la_bwd.hip); < 0 (default): every row count
 *   "res_rows_bwd_min_rows" rows (B * rows_per_sample) from which the ResnetBlock backward over m/z rows of 2 / 4 / 8 positions at 12 / 16
 *                           channels runs with the row as the lane column (k_res_rows.hip) instead of channel-parallel (k_res_cp.hip);
 *                           < 0 (default): the device rule, one 16-row tile per compute unit (4,096 rows on MI355X)
 * Both forms compute the same function (parity tests run both at every size).  Unknown key: non-zero / INT64_MIN. */
int dq_set_option(const char* key, int64_t value);
int64_t dq_get_option(const char* key);
/* The threshold the library applies right now for the key above: the set value (clamped to INT32_MAX), or with the option < 0 the
 * resolved default rule.  Unknown key: -1. */
int64_t dq_get_option_effective(const char* key);

/* DDIMDiffusionModel.pred_type (model.py:205-213, 269-280, 354-389); any other value is rejected ("Unknown pred_type").
 * DQ_PRED_V ("v_prediction", no reference counterpart; Salimans & Ho 2022): the network output is v = sa eps - sb x0 with sa = sqrt(ab_t),
 * sb = sqrt(1 - ab_t); x0 = sa x_t - sb v and eps = sb x_t + sa v are recovered without a division.  dq_train_step, dq_eval_step and
 * dq_ddim_step_sto and dq_ddim_sample take the value as their pred_type.  dq_solver_step and dq_guided_update are called by the test suite
 * with 2 as an unknown objective, on operands that must not be touched, and keep refusing it: their v forms are dq_solver_step_v and
 * dq_guided_update_v.  dq_tfm_sample and dq_tfm_eval_step (the CustomTransformer, not built for this objective) refuse it as unknown. */
enum { DQ_PRED_EPS = 0, DQ_PRED_X0 = 1, DQ_PRED_V = 2 };

/* ---- network description -------------------------------------------------------------------------------------
 * Replaces UNet1d.__init__ (unet1d.py:918-1084) for simple=True, conditional=True, channels=1,
 * init_cond_channels=1: builds the layer list and the flat parameter layout.
 * mz == downsample_dim.  num_timesteps is informational (kept for ABI continuity): the schedule tables come with each call.
 * Returns NULL on an unsupported configuration (see dq_last_error).  dq_plan_create is dq_plan_create_ex(..., 1). */
dq_plan* dq_plan_create(int dim, int n_mults, const int* dim_mults, int mz, int num_timesteps);
/* attn_cond_channels = M1 in 1..4096 (anything else: NULL, the error names the argument): the MS1 conditioning of every entry point
 * that takes attn_cond / ms1_cond is (B, RT, M1) with M1 contiguous -- what the reference folds to (B, M1, RT) in front of
 * attn_cond_proj (unet1d.py:1122-1130) -- and attn_cond_proj.1.0.weight is (8, M1, 7).  M1 = 1 is the (B, RT) chromatogram and the code
 * path of dq_plan_create, launch for launch.  M1 > 1: k_ms1_feat.hip reads the (B, RT, M1) layout directly; ms1_loss_weight > 0 is rejected
 * (dq_train_step), the MS1 term being defined on a chromatogram. */
dq_plan* dq_plan_create_ex(int dim, int n_mults, const int* dim_mults, int mz, int num_timesteps, int attn_cond_channels);
/* The plan's attn_cond_channels; -1 for a NULL plan. */
int dq_plan_attn_cond_channels(const dq_plan* plan);
void dq_plan_destroy(dq_plan* plan);
/* Number of trainable tensors / total trainable floats in the flat buffer. */
int dq_plan_num_params(const dq_plan* plan);
int64_t dq_plan_param_floats(const dq_plan* plan);
/* Tensor i: state_dict key (NUL-terminated into name[name_cap]), offset in floats, ndim, shape[4]. */
int dq_plan_param_info(const dq_plan* plan, int i, char* name, int name_cap, int64_t* offset, int* ndim, int64_t* shape);
/* Bytes of workspace dq_unet_fwd / dq_unet_bwd / dq_train_step / dq_ddim_sample need for (B, RT).
 * training != 0 adds the gradient twin of the activation arena. */
int64_t dq_unet_workspace_bytes(dq_plan* plan, int B, int RT, int training);

/* Output activation of the network (UNet1d pos_output_only, unet1d.py:1084, 1166): what final_act applies to final_conv's output.
 *   DQ_FINAL_IDENTITY (default): the network output is final_conv's output;
 *   DQ_FINAL_SOFTPLUS: torch.nn.Softplus() (beta 1, threshold 20): y = x for x > 20, else log1p(exp(x)); dy/dx = 1 for x > 20,
 *                      else sigmoid(x).
 * Per plan.  It applies to every entry point that forms or differentiates the network output: dq_unet_fwd, dq_unet_bwd (grad_out is
 * d loss / d y, the activated output), dq_train_step (its losses are taken on y) and dq_ddim_sample (eps or, with DQ_PRED_X0, x0 is y; DQ_PRED_V: v is y).
 * Workspace sizes do not depend on it.  A call drops the plan's cached sampling graph.  Any other value: non-zero (dq_last_error). */
enum { DQ_FINAL_IDENTITY = 0, DQ_FINAL_SOFTPLUS = 1 };
int dq_plan_set_final_act(dq_plan* plan, int act);
/* The plan's output activation (DQ_FINAL_*); -1 for a NULL plan. */
int dq_plan_final_act(const dq_plan* plan);

/* ---- K0: DDIMDiffusionModel.q_sample (model.py:225-242) ---------------------------------------------------------
 * x_t = sqrt(ab[t_b]) * x0' + sqrt(1 - ab[t_b]) * noise, x0' = 2*x0-1 if normalize_x0 (model.py:349) else x0. */
int dq_q_sample(const float* alpha_bars_dev, const float* x0, const int64_t* t, const float* noise, float* x_t, int B,
                int64_t per_sample, int normalize_x0, void* stream);

/* ---- K9: the update of DDIMDiffusionModel.p_sample (model.py:265-289, pred_type "eps") ---------------------------
 * coef_dev: 4 device floats [sqrt(ab_t), sqrt(1-ab_t), sqrt(ab_{t-1}), sqrt(1-ab_{t-1})]; coef_dev[2] < 0 means t == 0
 * (x_prev = x0_pred). */
int dq_ddim_step(const float* x_t, const float* eps, float* x_prev, const float* coef_dev, int64_t n, void* stream);
/* pred_type "x0" (model.py:274-278): the network output is x0_pred; eps = (x_t - sqrt(ab_t)*x0_pred)/sqrt(1-ab_t) is derived
 * and written to eps_out (nullable); x_prev as above. */
int dq_ddim_step_x0(const float* x_t, const float* x0_pred, float* x_prev, float* eps_out, const float* coef_dev, int64_t n,
                    void* stream);
/* pred_type "v_prediction": the network output is v_pred; x0 = sa*x_t - sb*v_pred and eps = sb*x_t + sa*v_pred (sa, sb = coef_dev[0], [1])
 * are derived, eps written to eps_out (nullable); x_prev as above. */
int dq_ddim_step_v(const float* x_t, const float* v_pred, float* x_prev, float* eps_out, const float* coef_dev, int64_t n, void* stream);

/* ---- K1-K8: UNet1d.forward (unet1d.py:1086-1166) ---------------------------------------------------------------
 * params: flat parameter buffer; rope_freqs: the 8 non-trainable RoPE frequencies (device).
 * x, init_cond (B,RT,MZ); attn_cond (B,RT,M1), M1 = the plan's attn_cond_channels ((B,RT) at M1 = 1); t (B) int64 or NULL => every sample uses t_scalar.
 * init_cond/attn_cond are mapped v*cond_mul+cond_add on the fly (2,-1 reproduces model.py:310-311/350-351; 1,0 = raw).
 * out (B,RT,MZ) receives the prediction.  save_for_bwd != 0 also keeps the pre-norm tensors dq_unet_bwd reads. */
int dq_unet_fwd(dq_plan* plan, const float* params, const float* rope_freqs, const float* x, const int64_t* t, int t_scalar,
                const float* init_cond, const float* attn_cond, float cond_mul, float cond_add, float* out, int save_for_bwd,
                void* workspace, int64_t workspace_bytes, int B, int RT, void* stream);
/* Backward of the call above (same plan/workspace/arguments, workspace sized with training=1): accumulates
 * d loss / d params into grads (+=; zero it first) given grad_out = d loss / d out.  grad_x (optional, may be NULL)
 * receives d loss / d x.  Replaces loss.backward() through the network (model_interface.py:1120). */
int dq_unet_bwd(dq_plan* plan, const float* params, const float* rope_freqs, const float* init_cond, float cond_mul,
                float cond_add, const float* grad_out, float* grads, float* grad_x, void* workspace, int64_t workspace_bytes,
                int B, int RT, void* stream);

/* ---- K10: F.mse_loss(eps_pred, noise) and its gradient (model.py:361) ------------------------------------------
 * loss_out: 1 device float (mean over all n elements); grad_out (nullable): 2*(eps-noise)/n.
 * scratch: >= 1024 device floats. */
int dq_mse_loss_fwd_bwd(const float* eps, const float* noise, float* loss_out, float* grad_out, float* scratch, int64_t n,
                        void* stream);
/* pred_type "x0" (model.py:372-376, 404): loss = mean over samples b of loss_weight_dev[t_b] * MSE_b(pred, target*target_mul +
 * target_add); loss_weight_dev: the T-entry table DDIMDiffusionModel.loss_weight (SNR, model.py:205-210); grad_out nullable. */
int dq_mse_loss_weighted_fwd_bwd(const float* pred, const float* target, float target_mul, float target_add,
                                 const float* loss_weight_dev, const int64_t* t, float* loss_out, float* grad_out, float* scratch,
                                 int B, int64_t per_sample, void* stream);
/* pred_type "v_prediction": loss = mean over samples b of lw[t_b] * MSE_b(pred, z), z = sa_b * noise - sb_b * (x0 * tm + ta) with
 * sa_b = sqrt(alpha_bars_dev[t_b]), sb_b = sqrt(1 - alpha_bars_dev[t_b]) formed per element inside the kernel (never written).  lw: a
 * T-entry table or NULL (all ones, DDIMDiffusionModel.loss_weight for this objective); grad_out (nullable) = 2 lw[t_b] (pred - z) / (B per).
 * scratch: >= 1024 device floats.  16-byte accesses when per % 4 == 0 and every tensor is 16-byte aligned, else one element per lane. */
int dq_mse_loss_v_fwd_bwd(const float* pred, const float* x0, const float* noise, const float* alpha_bars_dev, float tm, float ta,
                          const float* lw, const int64_t* t, float* loss_out, float* grad_out, float* scratch, int B, int64_t per,
                          void* stream);

/* ---- K11: clip_grad_norm_(max_norm) + AdamW step (model_interface.py:1121-1122, torch defaults) ----------------
 * grads are first multiplied by grad_scale (1/world_size after a summing all-reduce), the global L2 norm of the
 * scaled grads goes to gnorm_out (nullable, 1 device float), then coef = min(1, max_norm/(norm+1e-6)) (max_norm <= 0
 * disables clipping) and the decoupled-decay AdamW update with bias correction for `step` (1-based).
 * scratch: >= 1024 device floats. */
int dq_adamw_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch,
                       float grad_scale, float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                       int step, float* gnorm_out, void* stream);
/* The same step with the learning rate (lr_dev[0] + lr_dev[1]: the host's double lr as a (hi, lo) fp32 pair, so the scalar factors formed
 * from it in double match dq_adamw_clip_step's bit for bit) and the step count (*step_dev, int32: incremented by the call, 0 before the first
 * step) in device memory: the call's arguments do not change from step to step, so a captured graph of it can be replayed.  scratch as above. */
int dq_adamw_clip_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch, float grad_scale,
                           float max_norm, const float* lr_dev, double beta1, double beta2, double eps, double weight_decay, int* step_dev,
                           float* gnorm_out, void* stream);
/* Both steps with an exponential moving average of the parameters kept in the same pass over the buffers (no reference counterpart: the
 * reference trains without one).  ema: n device floats with the layout of params.  After the AdamW update of step t (1-based; the device
 * variant: the incremented *step_dev), with p the updated parameter:
 *   beta_t = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay      (double; ema_decay is promoted from the float passed)
 *   w_t    = (float)(1.0 - beta_t)
 *   ema    = fmaf(w_t, p - ema, ema)                                           (one fp32 subtraction, one fmaf)
 * 0 <= ema_decay < 1, anything else (NaN included) and a null ema are errors and launch nothing.  params, exp_avg, exp_avg_sq and
 * gnorm_out receive bit for bit what dq_adamw_clip_step / dq_adamw_clip_step_dev write, for any n and alignment; the update runs with
 * 16-byte accesses when params, grads, exp_avg, exp_avg_sq and ema are all 16-byte aligned.  The device variant keeps w_t behind its three
 * scalars (scratch[1016 + 3]).  scratch as above. */
int dq_adamw_clip_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch,
                           float grad_scale, float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                           int step, float* gnorm_out, float* ema, float ema_decay, int ema_warmup, void* stream);
int dq_adamw_clip_ema_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch,
                               float grad_scale, float max_norm, const float* lr_dev, double beta1, double beta2, double eps,
                               double weight_decay, int* step_dev, float* gnorm_out, float* ema, float ema_decay, int ema_warmup,
                               void* stream);
/* on = 0: the backward's remaining weight-gradient launches run on the caller's stream instead of the plan's side stream (a captured train
 * step is then one chain; the fork / join inside a graph was measured slower than the chain).  Default 1. */
int dq_plan_set_side_stream(dq_plan* plan, int on);

/* ---- the MS1 term of train_step with ms1_loss_weight = w in (0, 1] (model.py:364-371, 379-386, 398-402) -----------------
 * The reference's branch raises (torch.max(x, dim=-1) returns a tuple that is then divided), so the semantics are chosen
 * (DESIGN.md section 12): per sample b, D = x_t - pred ('eps': pass x_t) or pred ('x0': x_t = NULL), s_f[rt] = f over m/z of
 * D[rt][:] for f in {sum, mean, max (values)}, ms1n = ms1_cond*cond_mul+cond_add (B, RT),
 *   additional_b = sum_f mean_rt (s_f[rt] / max_rt s_f - ms1n[rt] / max_rt ms1n)^2 .
 * On entry loss_inout (1 device float) / grad_inout (B,RT,MZ; nullable) hold the MSE part (dq_mse_loss[_weighted]_fwd_bwd);
 * on exit loss = (1-w) * MSE + w * mean_b lw_b additional_b and its gradient w.r.t. pred (lw = loss_weight_dev[t_b], NULL = 1).
 * scratch: 5*B*RT + B floats. */
int dq_ms1_loss_fwd_bwd(const float* pred, const float* x_t, const float* ms1_cond, float cond_mul, float cond_add,
                        const float* loss_weight_dev, const int64_t* t, float ms1_loss_weight, float* loss_inout, float* grad_inout,
                        float* scratch, int B, int RT, int MZ, void* stream);

/* ---- DDIMDiffusionModel.train_step (model.py:326-406) fused with its backward ----------------------------------------
 * normalise x0/conds, q_sample, network forward, MSE loss, backward into grads (+=).  t (B) int64 and noise (B,RT,MZ) are
 * drawn by the caller (the reference draws randint then randn_like, model.py:344-346).  pred_type DQ_PRED_EPS: target =
 * noise, loss_weight_dev ignored (may be NULL); DQ_PRED_X0: target = normalised x0, every sample weighted by
 * loss_weight_dev[t_b] (model.py:209-210, 404); DQ_PRED_V: target = sa_b noise - sb_b (normalised x0), weighted by
 * loss_weight_dev[t_b] when the table is given (NULL: all ones), ms1_loss_weight > 0 refused.  ms1_loss_weight in [0, 1]: 0 = the MSE alone; > 0 adds the MS1 term
 * (dq_ms1_loss_fwd_bwd above).  loss_out: 1 device float = mean over the batch of the per-sample loss. */
int dq_train_step(dq_plan* plan, const float* params, const float* rope_freqs, const float* alpha_bars_dev, const float* x0,
                  const float* ms2_cond, const float* ms1_cond, const int64_t* t, const float* noise, int auto_normalize,
                  int pred_type, const float* loss_weight_dev, float ms1_loss_weight, float* grads, float* loss_out, void* workspace,
                  int64_t workspace_bytes, int B, int RT, void* stream);

/* ---- held-out evaluation (no reference counterpart: the reference's TODOS list "eval metrics ... separate from training"; DESIGN.md
 * section 24).  Additive at ABI version 12: dq_eval_step, dq_mse_per_window, dq_mse_per_window_scratch_bytes, dq_recon_metrics,
 * dq_recon_metrics_scratch_bytes.
 * dq_eval_step: the forward-only counterpart of dq_train_step -- q_sample (normalising as auto_normalize says), the network forward without
 * anything kept for a backward, then dq_mse_per_window.  Arguments as dq_train_step without grads and ms1_loss_weight; two outputs:
 *   per_window_out  B device floats: the unweighted MSE of window b between the network output and its target (DQ_PRED_EPS: the noise;
 *                   DQ_PRED_X0: the normalised x0; DQ_PRED_V: sa_b noise - sb_b (normalised x0), dq_mse_per_window_v);
 *   loss_out        1 device float: mean_b loss_weight_dev[t_b] * per_window[b]; the table is required for DQ_PRED_X0, applied when given (NULL: all
 *                   ones) for DQ_PRED_V and ignored (may be NULL: all ones) for DQ_PRED_EPS, as in the train step.
 * It reports the MSE part only: the MS1 term of the training loss (ms1_loss_weight > 0) is not evaluated.  workspace: the INFERENCE size,
 * dq_unet_workspace_bytes(plan, B, RT, 0).  It touches no gradient buffer and nothing of the backward's side queue: called between two
 * train steps it leaves the second bit for bit what it would have been.  params is read by pointer (pass the EMA buffer to evaluate the
 * averaged weights).  A window's per_window value does not depend on the batch it is computed in. */
int dq_eval_step(dq_plan* plan, const float* params, const float* rope_freqs, const float* alpha_bars_dev, const float* x0,
                 const float* ms2_cond, const float* ms1_cond, const int64_t* t, const float* noise, int auto_normalize, int pred_type,
                 const float* loss_weight_dev, float* loss_out, float* per_window_out, void* workspace, int64_t workspace_bytes, int B, int RT,
                 void* stream);
/* The reduction of dq_eval_step on caller-supplied tensors (k_mse_per_window, k_stream.hip): out, target (B, per) fp32;
 * target' = target * tm + ta in fp32 as in dq_mse_loss_weighted_fwd_bwd; per element d = (double)out - (double)target', d * d summed in fp64.
 * A window is cut into slices of 8192 elements (a function of per alone, never of B), one workgroup each; the slice sums are added in index
 * order (no atomics) and per_window_out[b] = (float)(sum / per) is rounded once.  loss_out = (float)(sum_b lw[t_b] * (sum_b / per) / B), the
 * sum over windows in fp64 in index order; lw NULL: all ones (t is then not read).  0 < B <= 65535.
 * scratch: dq_mse_per_window_scratch_bytes(B, per) = 8 * B * ceil(per / 8192) bytes, 8-byte aligned (-1 for B or per < 1). */
int64_t dq_mse_per_window_scratch_bytes(int B, int64_t per);
int dq_mse_per_window(const float* out, const float* target, float tm, float ta, const float* lw, const int64_t* t, float* per_window_out,
                      float* loss_out, void* scratch, int B, int64_t per, void* stream);
/* The same under DQ_PRED_V: the target is sa_b * noise - sb_b * (x0 * tm + ta) in fp32 (dq_mse_loss_v_fwd_bwd's arithmetic), formed per
 * element; lw nullable (all ones).  Scratch and summation order as dq_mse_per_window. */
int dq_mse_per_window_v(const float* out, const float* x0, const float* noise, const float* alpha_bars_dev, float tm, float ta,
                        const float* lw, const int64_t* t, float* per_window_out, float* loss_out, void* scratch, int B, int64_t per,
                        void* stream);
/* Reconstruction metrics of pred against target, both (B, RT, MZ) fp32 (k_metrics.hip): out (B, DQ_METRIC_COUNT) floats per window, every sum
 * in fp64 over the fp32 inputs (n = RT * MZ), every output rounded to fp32 once:
 *   0 mse         sum (P - T)^2 / n
 *   1 mae         sum |P - T| / n
 *   2 cosine      sum P T / sqrt(sum P^2 * sum T^2); 0 if either norm is 0
 *   3 sa          1 - 2 acos(clamp(cosine, -1, 1)) / pi   (spectral angle)
 *   4 pearson     Pearson r over all n elements, from sums shifted by the window's first element (a constant window has variance exactly 0);
 *                 0 if either variance is 0
 *   5 scan_sa     mean over the valid scans of sa between P[r, :] and T[r, :]; a scan (RT row) is valid if sum T[r, :]^2 > 0, a valid scan
 *                 with an all-zero P row scores 0; 0 without a valid scan
 *   6 scan_count  number of valid scans
 *   7 xic_r       mean over the valid XICs of Pearson r along RT between P[:, c] and T[:, c] (sums shifted by the column's first element); an
 *                 XIC (m/z column) is valid if Var_r T[:, c] > 0 and scores 0 when Var_r P[:, c] = 0; 0 without a valid XIC
 *   8 xic_count   number of valid XICs
 * RT, MZ any positive values.  No atomics; the work partition depends on (RT, MZ) only: a window's row is bit for bit the same in any batch.
 * scratch: dq_recon_metrics_scratch_bytes(B, RT, MZ) = 8 * B * (10 * RT * ceil(MZ / 4096) + 5 * MZ * ceil(RT / 64)) bytes, 8-byte aligned
 * (-1 for a size < 1). */
enum { DQ_METRIC_MSE = 0, DQ_METRIC_MAE = 1, DQ_METRIC_COSINE = 2, DQ_METRIC_SA = 3, DQ_METRIC_PEARSON = 4, DQ_METRIC_SCAN_SA = 5,
       DQ_METRIC_SCAN_COUNT = 6, DQ_METRIC_XIC_R = 7, DQ_METRIC_XIC_COUNT = 8, DQ_METRIC_COUNT = 9 };
int64_t dq_recon_metrics_scratch_bytes(int B, int RT, int MZ);
int dq_recon_metrics(const float* pred, const float* target, float* out, void* scratch, int64_t scratch_bytes, int B, int RT, int MZ,
                     void* stream);

/* ---- stochastic sampling (no reference counterpart) -----------------------------------------
 * Noise is Philox4x32-10 (Random123 constants) evaluated inside the kernels: for element e of its window (0 <= e < per_window < 2^32),
 * draw index d, window id w (int64) and seed s (uint64): counter (e, d, w lo, w hi), key (s lo, s hi); output words r0, r1 give
 * u1 = ((r0 >> 9) + 0.5) 2^-23, u2 = (r1 >> 8) 2^-24, z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2).  d = 0 is x_T's, step i of the loop
 * (0-based) draws at d = 1 + i.  seed_dev (1 uint64) and window_ids_dev (B int64; NULL: 0 .. B-1) are DEVICE memory: a window draws the
 * same noise at any batch position, and a captured step is replayed unchanged under a new seed.
 * dq_randn: out (B, per_window) = z at draw index `draw`; out 4-byte aligned (16-byte stores when it is 16-byte aligned). */
int dq_randn(float* out, const int64_t* window_ids_dev, const uint64_t* seed_dev, int draw, int B, int64_t per_window, void* stream);
/* K9 with noise: x0 / eps as dq_ddim_step (DQ_PRED_EPS) or dq_ddim_step_x0 / dq_ddim_step_v (DQ_PRED_X0 / DQ_PRED_V; eps_out nullable, ignored under DQ_PRED_EPS) form
 * them, then x_prev = sap*x0 + c*eps + sigma*z.  coef_dev: 5 device floats [sa, sb, sap, c, sigma]; sap < 0 means t == 0: x_prev = x0, no
 * noise drawn (dq_ddim_step's result bit for bit).  per_window a multiple of 4; tensors 16-byte aligned; x_prev may alias x_t. */
int dq_ddim_step_sto(const float* x_t, const float* net_out, float* x_prev, float* eps_out, const float* coef_dev,
                     const int64_t* window_ids_dev, const uint64_t* seed_dev, int draw, int pred_type, int B, int64_t per_window,
                     void* stream);
/* The sampler's coefficient rows (host only, no GPU call; the function dq_ddim_sample uses under DQ_SAMPLER_REFERENCE): per step i at t = timesteps_host[i],
 * coef_out[4i..] = [sqrt(ab), sqrt(1-ab), sqrt(abp), c] and sigma_out[i], ab = alpha_bars[t], abp = alpha_bars[t-1];
 *   sigma = eta sqrt((1-abp)/(1-ab)) sqrt(1 - ab/abp), c = sqrt(max(0, 1 - abp - sigma^2))   (double, from the fp32 table values);
 * eta == 0: c = sqrt(1-abp) in fp32 (model.py:284-286, what the sampling loop always used) and sigma = 0.  t == 0: [.., -1, 0], sigma 0.
 * 0 <= eta <= 1, anything else (NaN included): non-zero (dq_last_error). */
int dq_ddim_coef_table(const float* alpha_bars_host, int num_timesteps, const int32_t* timesteps_host, int num_steps, float eta,
                       float* coef_out, float* sigma_out);

/* ---- step-consistent sampling (no reference counterpart) ------------------------------------
 * The reference's update at timestep t lands on alpha_bars[t-1] while the next step relabels the state as the next entry of the strided
 * list: exact only at num_steps == num_timesteps.  The samplers below land step i of the list ts[0..n-1] on alpha_bars[ts[i+1]];
 * the last step of the list returns the x0 estimate, whatever its t.  Their lists must be strictly decreasing.
 *   DQ_SAMPLER_REFERENCE  the update as it always was (dq_ddim_coef_table)
 *   DQ_SAMPLER_DDIM       the same update with abp = alpha_bars[ts[i+1]] (any eta in [0, 1])
 *   DQ_SAMPLER_DPMPP_2M   DPM-Solver++(2M) (Lu et al. 2022; data prediction, multistep, first order on the first step; eta == 0):
 *                         x_prev = cx x + c0 x0 + c1 x0_hist, with a = sqrt(ab), s = sqrt(1-ab), lambda = log(a / s), h = lambda_{i+1} - lambda_i,
 *                         r = h_{i-1} / h_i:  cx = s_{i+1} / s_i,  c0 = a_{i+1} (1 - e^-h) (1 + 1/(2r)),  c1 = -a_{i+1} (1 - e^-h) / (2r);
 *                         first step: c0 = a_{i+1} (1 - e^-h), c1 = 0 (the strided DDIM step); last row: cx = -1 (x_prev = x0).
 *                         Formed in double from the fp32 table values (expm1), rounded to fp32 once. */
enum { DQ_SAMPLER_REFERENCE = 0, DQ_SAMPLER_DDIM = 1, DQ_SAMPLER_DPMPP_2M = 2 };
/* The samplers' coefficient rows (host only, no GPU call).  Sampler 0: dq_ddim_coef_table's output exactly (extra_out = sigma).  Sampler 1:
 * rows [sqrt(ab), sqrt(1-ab), sqrt(abp), c] and extra_out = sigma with dq_ddim_coef_table's expressions at abp = alpha_bars[ts[i+1]]; last
 * row [.., -1, 0].  Sampler 2: rows [sa, sb, cx, c0], extra_out = c1.  Non-zero (dq_last_error): timesteps that do not strictly decrease
 * (samplers 1, 2), eta != 0 with sampler 2, eta outside [0, 1], an unknown sampler. */
int dq_sampler_coef_table(const float* alpha_bars_host, int num_timesteps, const int32_t* timesteps_host, int num_steps, int sampler,
                          float eta, float* coef_out, float* extra_out);
/* One solver update on caller-supplied tensors (the Solver family of k_update.hip).  coef_dev: 5 device floats [sa, sb, cx, c0, c1].  x0 = net_out (DQ_PRED_X0)
 * or (x_t - sb net_out) / sa (DQ_PRED_EPS; the v objective: dq_solver_step_v); clip_x0 > 0: x0 clamped to [-clip_x0, clip_x0] first; x_prev = (cx x_t + c0 x0) + c1 x0_hist,
 * or x0 when cx < 0.  x0_hist (nullable only when c1 == 0; not read when c1 == 0) receives x0.  eps_out (nullable): (x_t - sa x0) / sb under
 * DQ_PRED_X0 and for a clamped element, else net_out.  x_prev may alias x_t and eps_out net_out.  Any n; tensors 4-byte aligned (16-byte
 * accesses when n % 4 == 0 and all are 16-byte aligned). */
int dq_solver_step(const float* x_t, const float* net_out, float* x_prev, float* x0_hist, float* eps_out, const float* coef_dev, float clip_x0,
                   int pred_type, int64_t n, void* stream);
/* The same under the v objective: x0 = sa x_t - sb v_pred, eps = sb x_t + sa v_pred (eps_out, nullable, always the derived eps; where x0
 * was clamped, (x_t - sa x0) / sb).  Everything else as dq_solver_step. */
int dq_solver_step_v(const float* x_t, const float* v_pred, float* x_prev, float* x0_hist, float* eps_out, const float* coef_dev,
                     float clip_x0, int64_t n, void* stream);

/* ---- classifier-free guidance on MS1 (no reference counterpart) ------------------------------
 * MS1 is the one input that names the component to extract (the mixture is the same whichever precursor is asked for).  A network trained
 * with its MS1 randomly replaced by a null (dq_ms1_cond_drop) has a conditional output c and an unconditional output u; the guided sampler
 * runs every update on g = u + w (c - u): one fp32 subtraction and one fused multiply-add per element inside the update kernels, the same
 * rule for DQ_PRED_EPS and DQ_PRED_X0 (guidance commutes with the affine map between them; the v objective: dq_guided_update_v).  w = 1 is the conditional model, w = 0 the
 * unconditional one, w > 1 pushes towards the component MS1 names.  The null is a CONSTANT raw MS1 value in every element, normalised like
 * real MS1: no learned token, the checkpoint layout stays the reference's.
 *
 * dq_guided_update: one guided update on caller-supplied tensors.  kind: which of the four updates the sampling loop runs; coef_dev: the
 * layout of that kind's stand-alone entry -- DQ_UPDATE_DDIM 4 floats [sa, sb, sap, sbp] (dq_ddim_step / dq_ddim_step_x0), DQ_UPDATE_STOCHASTIC 5
 * floats [sa, sb, sap, c, sigma] (dq_ddim_step_sto; needs seed_dev; window_ids_dev nullable: 0 .. B-1; draw as there), DQ_UPDATE_SOLVER_1 /
 * DQ_UPDATE_SOLVER_2M 5 floats [sa, sb, cx, c0, c1] (dq_solver_step; clip_x0 > 0 clamps the guided x0; _2M reads (c1 != 0) and writes x0_hist,
 * _1 ignores it).  net_c / net_u: the conditional / unconditional network outputs (B, per_window).  x_prev, and x_mirror when non-NULL,
 * receive the same values; eps_out (nullable) the guided eps ((x_t - sa x0) / sb under DQ_PRED_X0 and for a clamped element, else g).
 * x0_hist, clip_x0, window_ids_dev, seed_dev and draw are ignored by the kinds that do not use them.  x_prev may alias x_t, eps_out net_c,
 * net_u net_c (then every output is the unguided entry's bit for bit).  Any sizes; tensors 4-byte aligned (16-byte accesses when
 * per_window % 4 == 0 -- B * per_window % 4 == 0 for the kinds without noise -- and all are 16-byte aligned).  Refused before any launch: a
 * NULL among x_t, net_c, net_u, x_prev, coef_dev (seed_dev: stochastic; x0_hist: 2M), an unknown kind or pred_type, w negative, NaN or
 * infinite. */
enum { DQ_UPDATE_DDIM = 0, DQ_UPDATE_STOCHASTIC = 1, DQ_UPDATE_SOLVER_1 = 2, DQ_UPDATE_SOLVER_2M = 3 };
int dq_guided_update(int kind, const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror, float* x0_hist,
                     float* eps_out, const float* coef_dev, float w, float clip_x0, const int64_t* window_ids_dev, const uint64_t* seed_dev,
                     int draw, int pred_type, int B, int64_t per_window, void* stream);
/* The same under the v objective: g = net_u + w (net_c - net_u) is formed on the v predictions, then x0 = sa x_t - sb g, eps = sb x_t + sa g
 * and the kind's update; dq_guided_update's arguments without pred_type, its refusals under this entry's name. */
int dq_guided_update_v(int kind, const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror, float* x0_hist,
                       float* eps_out, const float* coef_dev, float w, float clip_x0, const int64_t* window_ids_dev,
                       const uint64_t* seed_dev, int draw, int B, int64_t per_window, void* stream);
/* Conditioning dropout (k_cond_drop.hip): ms1_out (B, per_ms1) = ms1_in, with window b replaced as a whole by null_value iff r2 < thresh.
 * r2: the THIRD output word of Philox4x32-10 on counter (0, draw, id lo, id hi) under key (seed lo, seed hi), id = window_ids_dev[b] (NULL:
 * b); the normals above use words 0 and 1 only, so the decision never correlates with a noise draw under the same seed.  thresh = (uint32)
 * floor(p 2^32), in double; 0 <= p < 1 (anything else, NaN included: refused); p == 0 drops nothing.  A kept window is a bit copy;
 * ms1_out may alias ms1_in.  seed_dev: 1 uint64 of DEVICE memory; draw >= 0; tensors 4-byte aligned (16-byte accesses when both are
 * 16-byte aligned).  A window decides alone: the same under its id in any batch. */
int dq_ms1_cond_drop(const float* ms1_in, float* ms1_out, const int64_t* window_ids_dev, const uint64_t* seed_dev, int draw, double p,
                     float null_value, int B, int64_t per_ms1, void* stream);

/* ---- per-window sampler control: rescaled guidance, dynamic x0 thresholding (no reference counterpart) -------
 * Two options that need a window as a whole: a statistics pass (csrc/k_winstat.hip) between the network forward and the update leaves two
 * scalars per window in a (B, 4) device table [m_b, s_b, rho_b, -], which the update kernel's per-window form reads.  Per window b of
 * per = RT * MZ elements, at one step:
 *  1. g = u + w (c - u) per element as above; unguided g = c.
 *  2. Rescale (Lin et al. 2024, section 3.4), guidance_rescale = phi in [0, 1], guided calls only: var_c, var_g the variances of the
 *     window's c and of its fp32 g, from fp64 sums over the fp32 values shifted by the window's first element (dq_recon_metrics' form: a
 *     constant window has variance exactly 0); m_b = (float)(phi * sqrt(var_c / var_g) + (1 - phi)), formed in fp64 and rounded once,
 *     m_b = 1 when var_g <= 0; g <- m_b * g, one fp32 multiply.  Defined on the network output whatever the objective; in every update kind.
 *  3. x0 (and eps) from (x, g) by the objective, as always.
 *  4. Threshold (Saharia et al. 2022), threshold_quantile = q, a float32 in (0, 1]; solver kinds only.  Floor f = clip_x0 if given, else
 *     1; cap = threshold_max >= f (+inf: none).  a_0 <= .. <= a_{n-1} the window's |x0|; h = (double)q (n - 1), j = floor(h); Q = a_j if
 *     j == n - 1, else a_j + (a_{j+1} - a_j) (h - j) in fp64, every operation rounded on its own, Q rounded to fp32 once; the two order
 *     statistics are elements of the window, bit for bit (an exact radix select).  s_b = min(max(Q, f), cap), rho_b = f / s_b;
 *     x0 <- clamp(x0, -s_b, s_b) * rho_b; eps is re-derived, (x_t - sa x0) / sb, wherever x0 was clamped or rho_b != 1.  The thresholded
 *     x0 enters the update and the 2M history.  Inputs are assumed finite.
 * Where no window's Q exceeds f the step is the clip_x0 = f step bit for bit.  m_b and s_b depend on the window's elements and on per
 * only (the reductions are cut by per, never by B, and folded in a fixed order; no floating-point atomics): a window alone gives the bits
 * it gives in any batch.
 *
 * scratch of every entry below: dq_sample_stat_scratch_bytes(B, per_window) = 80 B + 4128 B ceil(per_window / 8192) bytes (-1 for
 * B < 1 or per_window < 1), 16-byte aligned; 1 <= B <= 65535, 1 <= per_window < 2^31. */
int64_t dq_sample_stat_scratch_bytes(int B, int64_t per_window);
/* Step 2 alone: m_out[b] (B floats) from net_c, net_u (B, per_window) at scale w.  Refused: a NULL, w negative, NaN or infinite, phi outside
 * [0, 1] or NaN, the sizes above, a scratch too small or misaligned. */
int dq_window_rescale(const float* net_c, const float* net_u, float w, double phi, int B, int64_t per_window, float* m_out, void* scratch,
                      int64_t scratch_bytes, void* stream);
/* Step 4's Q alone, of |x| itself: out[b] (B floats) from x (B, per_window).  Refused: a NULL, q outside (0, 1] or NaN, the sizes above,
 * a scratch too small or misaligned. */
int dq_window_abs_quantile(const float* x, int B, int64_t per_window, float q, float* out, void* scratch, int64_t scratch_bytes, void* stream);
/* One update in its per-window form over a table the caller supplies: dq_guided_update's arguments (kinds, coef_dev layouts, aliasing) with
 * table_dev (B, 4) = [m_b, s_b, rho_b, -] in place of clip_x0 (s_b > 0; +inf: no clamp).  net_u NULL: the unguided form, solver kinds only
 * (m_b is not read).  pred_type: DQ_PRED_EPS, DQ_PRED_X0 or DQ_PRED_V.  Rows [1, f, 1, -] give dq_guided_update (dq_solver_step) at
 * clip_x0 = f bit for bit, rows [1, +inf, 1, -] the unclamped one.  16-byte accesses when per_window % 4 == 0 and all tensors are 16-byte
 * aligned.  Refusals as dq_guided_update's, plus a NULL table and an unguided kind that is no solver. */
int dq_step_update_adaptive(int kind, const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror, float* x0_hist,
                            float* eps_out, const float* coef_dev, float w, const float* table_dev, const int64_t* window_ids_dev,
                            const uint64_t* seed_dev, int draw, int pred_type, int B, int64_t per_window, void* stream);

/* ---- joint sampling of a window's precursors under mixture consistency (no reference counterpart) -------------
 * data.mixture with scale_target trains the network to predict a precursor's contribution n_0 w_0 to the mixture it sees, and the
 * contributions of a window's precursors add up to that mixture.  Sampling the P precursors of a window as one group lets every step use
 * it: one streaming pass (csrc/k_group.hip) between the network forward and the update redistributes the step's x0 estimates -- the
 * proportional soft-mask form of the mixture-consistency projection (Wisdom et al. 2019).  A batch of B = G * P windows is G groups of P
 * members, 1 <= P <= 8, MEMBER-MAJOR: member p of group g is row p * G + g, so a joint batch is the concatenation of P ordinary batches.
 * The group's mixture m is row g of ms2_cond in the caller's units ([0, 1] after min-max), the tensor the network reads; rows p * G + g are
 * expected to repeat it and are not read by the pass.  Per element of a group, with the step's row [sa, sb]:
 *  1. x0_p from (x_p, net_p) by the objective, in the update's arithmetic: eps (x - sb net) / sa; x0 net; v sa x - sb net.
 *  2. y_p = auto_normalize ? (x0_p + 1) * 0.5f : x0_p, the image units of ms2_cond.
 *  3. yp_p = y_p > 0 ? y_p : 0;  S = ((yp_0 + yp_1) + yp_2) + ... in member order;  m <- m > 0 ? m : 0.
 *  4. DQ_CONSIST_BOUND: S > m: f = m / S, z_p = y_p > 0 ? y_p * f : y_p; else z_p = y_p.  Negatives are never touched, nothing is ever
 *     raised; P = 1 is the plain physical bound "a prediction may not exceed the observation".
 *     DQ_CONSIST_SUM: S > 0: f = m / S, z_p = yp_p * f; else z_p = m / P.  Negatives go to 0 and the group explains the whole mixture.
 *  5. y'_p = strength == 1 ? z_p : y_p + strength * (z_p - y_p), 0 < strength <= 1.
 *  6. x0'_p = y'_p == y_p ? x0_p : (auto_normalize ? 2 * y'_p - 1 : y'_p): an element the projection does not move keeps its x0 bits.
 * Every operation is one rounded fp32 operation in this order (no FMA contraction, correctly rounded division); inputs are assumed finite.
 * At strength 1, where the rule acts, sum_p max(y'_p, 0) equals m within (P + 1) 2^-24 m. */
enum { DQ_CONSIST_NONE = 0, DQ_CONSIST_BOUND = 1, DQ_CONSIST_SUM = 2 };
#define DQ_GROUP_MAX 8
/* The pass alone: x0_out (P * G, per_window) = x0' from x_t, net (P * G, per_window; what pred_type says) and mix (G, per_window).
 * coef_dev: a row whose first two floats are [sa, sb].  x0_out may alias net (element-wise); x_t and mix must not alias x0_out.  Under
 * DQ_PRED_X0 x_t is not read.  16-byte accesses when per_window % 4 == 0 and all tensors are 16-byte aligned.  Refused, in this order and
 * before anything touches the device: a NULL argument, an unknown pred_type, P outside [1, 8], G < 0 or per_window < 0, an unknown mode
 * (DQ_CONSIST_NONE included), strength outside (0, 1] or NaN, tensors that are not 4-byte aligned. */
int dq_group_project(const float* x_t, const float* net, float* x0_out, const float* mix, const float* coef_dev, int pred_type,
                     int auto_normalize, int G, int P, int64_t per_window, int mode, float strength, void* stream);

/* ---- DDIMDiffusionModel.sample (model.py:293-324): one sampling call, one record -----------------------
 * Runs the whole strided loop natively over timesteps_host[num_steps]: each step = network forward + update, then the epilogue
 * (model.py:319-322): out_x = denoised in [0, 1], out_noise = mixture - denoised.  The call crosses the ABI as the record below; both
 * networks' entries read the same one.  The caller sets struct_bytes = sizeof(dq_sample_call), the required fields, and leaves every
 * option it does not use at its "off" value (a zero-initialised record with group_size = 1 has every option off): the call is then the
 * reference's loop, the default update riding in the network's last launch.  Options combine freely except where a refusal says
 * otherwise.  The entry synchronises the stream twice on entry (its host-side tables must be on the device before the caller's arrays go
 * out of scope, and a capture must not see pending copies).
 * Refused, in this order and before anything touches the device: a NULL record; struct_bytes != sizeof(dq_sample_call) (the message
 * names both sizes; no other field is read before it); a NULL required argument; then each field's own refusals in the order of the
 * fields' paragraphs below (eta, sampler and what it combines with, the timesteps' order, the seed, pred_type, guidance_scale, the
 * per-window options); the per-window scratch; B, RT, num_steps; the group options; last the workspace size and num_timesteps. */
typedef struct dq_sample_call {
  int32_t struct_bytes;            /* sizeof(dq_sample_call) */
  const float* alpha_bars_host;    /* num_timesteps HOST floats (DDIMDiffusionModel.alpha_bars); every timestep must lie in [0, num_timesteps) */
  int32_t num_timesteps;           /* >= 1 */
  const float* x_T;                /* (B, RT, MZ), not modified; NULL (needs seed_dev): drawn, dq_randn at draw index 0 */
  const float* ms2_cond;           /* (B, RT, MZ) the mixture */
  const float* ms1_cond;           /* (B, RT, M1) the U-Net's, (B, S2) the transformer's */
  int32_t auto_normalize;
  int32_t pred_type;               /* DQ_PRED_EPS, DQ_PRED_X0; dq_ddim_sample also DQ_PRED_V (traj_eps then holds the derived eps); else "Unknown pred_type" */
  const int32_t* timesteps_host;   /* num_steps HOST ints; the caller forms them as trunc(linspace(T-1, 0, num_steps)), model.py:313 */
  int32_t num_steps;               /* 1 .. 1024 */
  float* out_x;
  float* out_noise;
  /* traj_x / traj_eps (nullable; off: NULL): (num_steps, B, RT, MZ) per-step x_{t-1} and eps (the derived eps where the network predicts
   * x0 or v or x0 is clamped; the guided eps under guidance; (x - sa x0') / sb over groups) */
  float* traj_x;
  float* traj_eps;
  /* use_graph != 0 and no trajectory: one step is captured into a hipGraph, cached on the handle (by params, workspace, shape, objective,
   * update kind, clip value, and every live option's values) and replayed num_steps times; the conditions, seed and ids are staged inside
   * the workspace, the step index lives on the device. */
  int32_t use_graph;
  void* workspace;                 /* dq_unet_workspace_bytes(plan, guided ? 2 * B : B, RT, 0) / dq_tfm_sample_workspace_bytes bytes */
  int64_t workspace_bytes;
  int32_t B;
  int32_t RT;                      /* the transformer's S1 */
  void* stream;
  /* eta (off: 0): the DDIM eta (Song et al. 2021, eq. 16; 1: ancestral DDPM-like sampling), 0 <= eta <= 1.
   * eta > 0: the update runs as dq_ddim_step_sto behind the forward (one more launch per step) and needs seed_dev; step i draws at index
   * 1 + i.  seed_dev (1 uint64) and window_ids_dev (B int64; NULL: 0 .. B-1) are DEVICE memory (off: NULL both).  Graphs captured with
   * eta > 0 and eta == 0 are cached apart, the value of eta itself lives in the coefficient tables. */
  float eta;
  const uint64_t* seed_dev;
  const int64_t* window_ids_dev;
  /* sampler (off: DQ_SAMPLER_REFERENCE = 0) and clip_x0 (off: <= 0 or NaN).  DQ_SAMPLER_DDIM with the clamp off runs
   * the reference's kernels and captured graph over the strided table.  DQ_SAMPLER_DPMPP_2M, and DQ_SAMPLER_DDIM with clip_x0 > 0
   * (first-order rows), run dq_solver_step behind the forward (one more launch per step), x in place and the x0 history in the
   * workspace.  Refused: an unknown sampler, eta > 0 with DQ_SAMPLER_DPMPP_2M or with clip_x0 > 0, clip_x0 > 0 with DQ_SAMPLER_REFERENCE,
   * timesteps that do not strictly decrease (samplers 1, 2). */
  int32_t sampler;
  float clip_x0;
  /* guided (off: 0): sampling from g = u + w (c - u) with guidance_scale = w (finite, >= 0) and the null's raw MS1
   * value null_ms1; both are ignored at guided == 0.  The arena and the forward run at 2 B windows -- rows [0, B) carry ms1_cond, rows
   * [B, 2B) null_ms1 in every element; both see the same mixture and the same x -- so the workspace is that of 2 * B windows.  One
   * forward and one update launch per step: the update runs behind the forward (never in the head launch) in its guided form
   * (dq_guided_update) over the B windows of the first half and keeps the second half's x equal to the first's.  x_T, the outputs and
   * the trajectories are B windows.  w = 1 is the conditional model at twice the cost: callers wanting that leave guided at 0. */
  int32_t guided;
  float guidance_scale;
  float null_ms1;
  /* The per-window options (off: guidance_rescale == 0 and threshold_quantile == 0; NaN counts as set):
   * guidance_rescale = phi in [0, 1] (without `guided` a no-op: g = c, m = 1), threshold_quantile = q in (0, 1] and threshold_max >= the
   * floor (not looked at when both are 0).  With either live, every step runs the statistics launches between the forward and the update
   * (rescale: 2; threshold: 5 -- four radix passes and the fold), inside the captured step too, and the update in its per-window form
   * behind the forward; thresholding selects the update clip_x0 selects and is refused exactly where clip_x0 is (DQ_SAMPLER_REFERENCE,
   * eta > 0).  stat_scratch (dq_sample_stat_scratch_bytes(B, RT * MZ) bytes; nullable with both off) holds the table, the partials and
   * the histograms at fixed addresses. */
  double guidance_rescale;
  float threshold_quantile;
  float threshold_max;
  void* stat_scratch;
  int64_t stat_scratch_bytes;
  /* Sampling over groups (off: consistency == DQ_CONSIST_NONE, group_size 1 -- the other two are then ignored):
   * group_size = P in [1, 8] dividing B, consistency a DQ_CONSIST_* mode, consistency_strength in (0, 1].  Every step runs the forward,
   * then the pass above in place on the network output, then the update in its x0-objective form over x0' behind the forward, whatever
   * the network's objective: the projected estimate enters x_prev, the 2M history and the derived eps; clip_x0 clamps after the
   * projection.  Refused: group_size outside [1, 8], B % group_size != 0, an unknown mode, a strength outside (0, 1] or NaN; and, first
   * of them, consistency together with `guided` or a live per-window option -- not implemented (follow-up: the guided form of the group
   * pass, which needs the mirror half written, and the per-window statistics over projected estimates). */
  int32_t group_size;
  int32_t consistency;
  float consistency_strength;
} dq_sample_call;
/* The U-Net's only sampling entry (x_T (B, RT, MZ), mz the plan's).  The captured step is cached in the plan. */
int dq_ddim_sample(dq_plan* plan, const float* params, const float* rope_freqs, const dq_sample_call* call);
/* Test hook: the record's layout as this library was compiled -- sizeof(dq_sample_call), then (offsetof, size) of every field in
 * declaration order -- so that a binding's mirror can be checked on any machine without a compiler.  Returns the number of ints written
 * (1 + 2 * fields), or -1 when cap is smaller. */
int dq_debug_sample_call_layout(int32_t* out, int cap);

/* ---- batch formation from an HBM-resident dataset (the step right before the hot path) ------------
 * Replaces, for B (window 1, window 2) pairs, DIAMSDataset.__getitem__'s min-max normalisation (utils/data_loader.py:70-79:
 * MS2 min/max over both windows, MS1 min/max over window 1 only, (x - min) / (max - min), no epsilon: a constant pair gives
 * NaN like the reference) and the mixture ms2_cond = w1*ms2_1 + w2*ms2_2 of _train_one_epoch (model_interface.py:1073-1075).
 * Bit-identical to the reference's numpy/torch arithmetic on float32 data without NaNs.
 * ms2_data (n_windows, RT, MZ), ms1_data (n_windows, ms1_per_window) fp32 on the device; idx_dev: 2*B device int64
 * [idx1 (B) | idx2 (B)] -- a pair with an index outside [0, n_windows) is never dereferenced, its outputs are NaN.
 * Outputs (device): ms2_1, ms2_2, ms2_cond (B, RT, MZ); ms1_1, ms1_2 (B, ms1_per_window); ms2_2 / ms1_2 / ms2_cond nullable.
 * scratch: dq_pair_batch_scratch_bytes(B) bytes.  Asynchronous on stream, no host synchronisation. */
int64_t dq_pair_batch_scratch_bytes(int B);
int dq_pair_batch(const float* ms2_data, const float* ms1_data, int64_t n_windows, const int64_t* idx_dev, int B, int RT, int MZ,
                  int64_t ms1_per_window, float w1, float w2, float* ms2_1, float* ms1_1, float* ms2_2, float* ms1_2,
                  float* ms2_cond, void* scratch, int64_t scratch_bytes, void* stream);

/* K-component mixtures with per-window weights (csrc/k_mix.hip; additive at ABI version 12): dq_pair_batch's batch
 * formation for 1..K windows per item, K in 2..8.  idx_dev: (K, B) device int64, row j = component j of every window, row 0 the target;
 * count_dev: (B) device int32, the components present in window b (1..K; NULL: K everywhere).  Rows j >= count[b] are never read.  A window
 * with a used index outside [0, n_windows), or a count outside [1, K], is never dereferenced: every output of it, weights_out included, is
 * NaN.  n_j = (x_j - lo) / (hi - lo): MS2 lo / hi over all present components, MS1 lo / hi over component 0 only, no epsilon (a constant
 * window set gives NaN).
 * Weights: weights_host != NULL: w_j = weights_host[j] for j < count[b] (K host floats, read before the call returns; not renormalised).
 * weights_host == NULL: drawn.  a_j = (1 + m 2^-23) 2^e with m = r3 & 0x7fffff, e = ((r3 >> 23) * E) >> 9, E = max_ratio_log2 (E == 0:
 * a_j = 1), r3 the FOURTH output word of Philox4x32-10 on counter (j, draw, id lo, id hi) under key (seed lo, seed hi), id =
 * window_ids_dev[b] (NULL: b) -- the normals use words 0 and 1, dq_ms1_cond_drop word 2 of counter (0, ...).  s = ((a_0 + a_1) + a_2) + ...
 * in fp32 over the present components, w_j = a_j / s: max w / min w < 2^E.  seed_dev: 1 uint64 of DEVICE memory.  A window decides from
 * (seed, id, draw) alone, wherever it sits in a batch.
 * Outputs (device): ms2_cond (B, RT, MZ) = ((n_0 w_0 + n_1 w_1) + n_2 w_2) + ..., every product and every sum rounded; ms2_rest (nullable)
 * the same sum from j = 1 (0 for count 1); ms2_target = n_0 (scale_target == 0) or the product n_0 w_0 that entered ms2_cond; ms1_target
 * (B, ms1_per_window) the normalised MS1 of component 0; weights_out (B, K) = w_j, 0 for absent components.  A numpy fp32 transcription of
 * these rules gives every bit (tests/test_mix_host.py); K = 2 with fixed weights and scale_target == 0 is dq_pair_batch bit for bit.
 * scratch: dq_mix_batch_scratch_bytes(B, K) bytes (0 for a B or K the call refuses).  Two launches, asynchronous on stream.
 * Refused before any launch (dq_last_error), in this order: a NULL among ms2_data, ms1_data, idx_dev, ms2_target, ms1_target, ms2_cond,
 * weights_out, scratch; K outside 2..8; max_ratio_log2 outside 0..16 (fixed weights too); draw < 0; B outside 1..65535; a non-positive
 * size; RT*MZ % 4 != 0; weights_host == NULL without seed_dev; scratch too small. */
int64_t dq_mix_batch_scratch_bytes(int B, int K);
int dq_mix_batch(const float* ms2_data, const float* ms1_data, int64_t n_windows, const int64_t* idx_dev, const int32_t* count_dev, int B,
                 int K, int RT, int MZ, int64_t ms1_per_window, const float* weights_host, int max_ratio_log2, const uint64_t* seed_dev,
                 const int64_t* window_ids_dev, int draw, int scale_target, float* ms2_target, float* ms1_target, float* ms2_cond,
                 float* ms2_rest, float* weights_out, void* scratch, int64_t scratch_bytes, void* stream);

/* Group mixtures (csrc/k_mix.hip; additive at ABI version 12): dq_mix_batch's rule for G groups.  A group is ONE
 * mixture of count[g] components whose first P are the members that joint sampling (dq_ddim_sample, group_size = P) is asked for:
 * 1 <= P <= K, K in 2..8.  Arguments as dq_mix_batch with G in place of B, plus P.  idx_dev (K, G): rows 0 .. P-1 are the members.  A group
 * whose count lies outside [P, K], or that uses an index outside [0, n_windows), is never dereferenced: every output of it is NaN, and no
 * output of another group is affected.  MS2 lo / hi over all present components (symmetric in the members); the weights are exactly
 * dq_mix_batch's, drawn or fixed, keyed by (seed, id, draw, j) with id = window_ids_dev[g] (NULL: g); MS1 of member p is normalised by that
 * member's own lo / hi -- what the member would see as the target of its own window.
 * Outputs (device), member-major -- member p of group g is row p * G + g, the layout dq_ddim_sample takes over groups:
 *   ms2_cond    (P*G, RT, MZ)  the mixture ((n_0 w_0 + n_1 w_1) + ...), written to all P member slices (the network reads every row)
 *   ms2_target  (P*G, RT, MZ)  n_p, or under scale_target the product n_p w_p that entered the mixture
 *   ms1_target  (P*G, ms1_per_window)
 *   ms2_rest    (G, RT, MZ), nullable: (n_P w_P + n_{P+1} w_{P+1}) + ..., the part no member explains; 0 when count == P
 *   weights_out (G, K)
 * Every operation is one rounded fp32 operation in this order, so a numpy fp32 transcription gives every bit (tests/group_eval_ref.py).
 * ms2_cond in every slice, weights_out and member 0's target and MS1 are dq_mix_batch's outputs on the same arguments bit for bit; with
 * fixed weights member p's are dq_mix_batch's with rows 0 and p of idx and weights_host[0] / [p] swapped; with scale_target and count == P
 * the members' targets added in order are ms2_cond.
 * Two launches, no atomics, asynchronous on stream.  Algorithmic bytes per group: (count + 2 P + 1) * RT*MZ*4 + the MS1 rows.
 * scratch: dq_mix_group_batch_scratch_bytes(G, K, P) = 8 * G * (8 + P) bytes (0 for arguments the call refuses).
 * Refused before any launch (dq_last_error), in dq_mix_batch's order with P directly behind K: a NULL among ms2_data, ms1_data, idx_dev,
 * ms2_target, ms1_target, ms2_cond, weights_out, scratch; K outside 2..8; P outside 1..K; max_ratio_log2 outside 0..16; draw < 0; G outside
 * 1..65535; a non-positive size; RT*MZ % 4 != 0; weights_host == NULL without seed_dev; scratch too small. */
int64_t dq_mix_group_batch_scratch_bytes(int G, int K, int P);
int dq_mix_group_batch(const float* ms2_data, const float* ms1_data, int64_t n_windows, const int64_t* idx_dev, const int32_t* count_dev,
                       int G, int K, int P, int RT, int MZ, int64_t ms1_per_window, const float* weights_host, int max_ratio_log2,
                       const uint64_t* seed_dev, const int64_t* window_ids_dev, int draw, int scale_target, float* ms2_target,
                       float* ms1_target, float* ms2_cond, float* ms2_rest, float* weights_out, void* scratch, int64_t scratch_bytes,
                       void* stream);

/* What a group's P predictions do together (csrc/k_group_metrics.hip; additive at ABI version 12).  pred, target
 * (P*G, RT, MZ) fp32, member-major; mix (G, RT, MZ): row g is read, the members' repeats are not.  All in the caller's image units.  Every
 * sum in fp64 over the fp32 inputs, every output rounded to fp32 once:
 *   cross (G, P, P)  cross[g, p, q] = sum pred_p target_q / sqrt(sum pred_p^2 * sum target_q^2); 0 if either norm is 0.  The diagonal is
 *                    dq_recon_metrics' cosine of window p G + g.
 *   group (G, 3)     with S = sum_p max(pred_p, 0) (p ascending) and m+ = max(mix, 0) per element:
 *                    0 excess       sum max(S - m+, 0) / sum m+
 *                    1 unexplained  sum max(m+ - S, 0) / sum m+
 *                    2 mix_total    sum m+                          (the two ratios are 0 when sum m+ == 0)
 * P in 1..8; RT, MZ any positive values; any 4-byte alignment (16-byte accesses where RT*MZ % 4 == 0 and pred, target and mix are 16-byte
 * aligned, 4-byte ones otherwise: the same bits either way).  No atomics; the work partition depends on (RT, MZ, P) only and partials are
 * folded in index order: a group's rows are bit for bit the same in any batch and on every repeat.
 * scratch: dq_group_metrics_scratch_bytes(G, P, RT, MZ) = 8 * G * (P + 1) * (P + 2) * ceil(RT*MZ / 4096) bytes, 8-byte aligned (-1 for a
 * size < 1 or P outside 1..8).
 * Refused before anything touches the device, in this order: a NULL argument; P outside 1..8; a size below 1; scratch too small; pred,
 * target, mix, cross or group not 4-byte aligned (scratch: 8-byte). */
enum { DQ_GROUP_EXCESS = 0, DQ_GROUP_UNEXPLAINED = 1, DQ_GROUP_MIX_TOTAL = 2, DQ_GROUP_METRIC_COUNT = 3 };
int64_t dq_group_metrics_scratch_bytes(int G, int P, int RT, int MZ);
int dq_group_metrics(const float* pred, const float* target, const float* mix, float* cross, float* group, void* scratch,
                     int64_t scratch_bytes, int G, int P, int RT, int MZ, void* stream);

/* Whole chromatograms (csrc/k_run.hip; additive at ABI version 12): one observed run ms2_run (RT_total, MZ) with its
 * MS1 trace ms1_run (RT_total, M1), fp32 on the device, cut into windows of W scans every `step` scans, and the windows' predictions
 * folded back into one chromatogram.  Window rule: 1 <= step <= W <= RT_total; n = ceil((RT_total - W) / step) + 1 windows
 * (dq_run_window_count; 0 for sizes outside the rule); window i starts at scan s_i = min(i * step, RT_total - W), the last one pulled
 * back to end on the last scan.  Every scan is covered and no two starts coincide.  Both calls work on windows i0 .. i0 + B - 1 and
 * recompute s_i themselves: no index array is passed.
 * dq_run_windows writes ms2_win (B, W, MZ), ms1_win (B, W, M1) and scale (B, 4) = (MS2 lo, MS2 hi, MS1 lo, MS1 hi) of each window:
 * n = (x - lo) / (hi - lo) in fp32 (dq_pair_batch's expression), MS2 lo / hi over the window's own W * MZ values, MS1 lo / hi over its
 * W * M1 values.  Unlike dq_pair_batch a constant window (hi == lo: an empty stretch of a run) gives zeros, not NaN; scale still records
 * lo == hi.  Any MZ >= 1 and M1 >= 1 (float4 accesses when MZ % 4 == 0, scalar ones otherwise).  Inputs are assumed finite: fminf /
 * fmaxf return the other operand for a NaN, so a NaN does not enter lo / hi and comes out as NaN; an infinity makes the range infinite
 * (finite values become 0, the infinity NaN).  scratch: dq_run_windows_scratch_bytes(B) bytes (0 for a B the call refuses).  Two launches.
 * dq_run_stitch folds pred (B, W, MZ), the predictions for those windows in the windows' normalised units, into the running state mean
 * (RT_total, MZ), m2 (RT_total, MZ), wsum (RT_total), which the caller zeroes before the first call.  scale: dq_run_windows' (B, 4) rows of
 * the same windows; taper: W positive device floats, the weight of a window's scan k.  For output element (r, m), over the call's windows
 * that cover r in ascending i, every operation rounded on its own (West's weighted running mean and variance):
 *   v = pred[i, r - s_i, m] * (hi_i - lo_i);  w = taper[r - s_i];  wn = wsum + w;  d = v - mean;
 *   mean = mean + (w / wn) * d;  m2 = m2 + (w * d) * (v - mean);  wsum = wn
 * so windows fed in ascending order give the same bits in any grouping into calls.  mean is the prediction in intensity units ABOVE each
 * window's floor (p * (hi - lo), not lo + p * (hi - lo)); m2 / wsum is the weighted variance among the windows that cover a scan; wsum
 * the sum of their taper weights.  One launch; scans no window of the call covers are not touched.
 * Both are asynchronous on stream.  Refused before any launch (dq_last_error), in this order: a NULL pointer (stream aside); MZ or M1 < 1;
 * sizes outside 1 <= step <= W <= RT_total; i0 < 0, B < 1 or i0 + B > n; B > 65535; (dq_run_windows) scratch too small. */
int64_t dq_run_window_count(int RT_total, int W, int step);
int64_t dq_run_windows_scratch_bytes(int B);
int dq_run_windows(const float* ms2_run, const float* ms1_run, int RT_total, int MZ, int M1, int W, int step, int64_t i0, int B,
                   float* ms2_win, float* ms1_win, float* scale, void* scratch, int64_t scratch_bytes, void* stream);
int dq_run_stitch(const float* pred, const float* scale, const float* taper, int RT_total, int MZ, int W, int step, int64_t i0, int B,
                  float* mean, float* m2, float* wsum, void* stream);

/* ---- CustomTransformer (dquartic/model/building_blocks.py:179-260) ----------------------------------
 * The reference's alternative noise predictor: forward(x_t (B,S1,input_dim), t (B) int64, x_cond (B,S2)) -> (B,S1,input_dim).
 * The handle fixes the parameter layout: one flat fp32 buffer, tensors under the reference's state_dict keys in its
 * registration order (dq_tfm_param_info).  Needs input_dim % 4 == 0, hidden_dim % 8 == 0, (hidden_dim / num_heads) % 4 == 0;
 * NULL otherwise (dq_last_error).  Calls that share a handle must not run concurrently. */
typedef struct dq_tfm dq_tfm;
dq_tfm* dq_tfm_create(int input_dim, int hidden_dim, int num_heads, int num_layers);
void dq_tfm_destroy(dq_tfm* tfm);
int dq_tfm_num_params(const dq_tfm* tfm);
int64_t dq_tfm_param_floats(const dq_tfm* tfm);
/* name_cap bytes of name; shape: 2 entries (a vector has shape[1] = 1). */
int dq_tfm_param_info(const dq_tfm* tfm, int i, char* name, int name_cap, int64_t* offset, int* ndim, int64_t* shape);
int64_t dq_tfm_workspace_bytes(const dq_tfm* tfm, int B, int S1, int S2, int training);
/* Forward (building_blocks.py:224-260).  rope_sin / rope_cos: (max(S1,S2), hidden_dim/2) device tables of apply_rope's angles
 * (:31-49) and time_freqs: (hidden_dim/2) of TimeEmbedding (:104-106) -- formed by the caller with the reference's own torch
 * expressions so that they are bit-identical.  save_for_bwd != 0 keeps every layer's activations in the workspace. */
int dq_tfm_fwd(dq_tfm* tfm, const float* params, const float* rope_sin, const float* rope_cos, const float* time_freqs,
               const float* x_t, const int64_t* t, const float* x_cond, float* out, int save_for_bwd, void* workspace,
               int64_t workspace_bytes, int B, int S1, int S2, void* stream);
/* Backward of the last dq_tfm_fwd(save_for_bwd = 1) on the same workspace.  grads: flat, same layout as params; accumulate != 0:
 * += (autograd's convention); accumulate == 0: plain stores -- every parameter gradient is produced exactly once per backward,
 * so a training step needs no zeroing pass over the 764 MB buffer of the reference configuration.
 * dx_t (B,S1,input_dim) and dx_cond (B,S2) are plain stores and may be NULL. */
int dq_tfm_bwd(dq_tfm* tfm, const float* params, const float* rope_sin, const float* rope_cos, const float* x_t,
               const float* x_cond, const float* dout, float* grads, int accumulate, float* dx_t, float* dx_cond,
               void* workspace, int64_t workspace_bytes, int B, int S1, int S2, void* stream);
/* The same backward for data-parallel training (the reference wraps the model in DistributedDataParallel, model_interface.py
 * :953-957, whose reducer all-reduces gradient buckets while the backward is still running): the flat gradient buffer is cut into
 * dq_tfm_num_buckets() = num_layers + 1 contiguous slices -- bucket i < num_layers is layer num_layers-1-i, the last bucket is
 * everything registered before the layers -- and on_bucket(user, i, offset, count) is called ON THE CALLING THREAD as soon as every
 * kernel writing grads[offset .. offset+count) has been enqueued on `stream`, in bucket order.  The callback typically records an
 * event on `stream` and starts that slice's all-reduce on a communication stream; it must not touch other slices. */
typedef void (*dq_tfm_bucket_fn)(void* user, int bucket, int64_t offset, int64_t count);
int dq_tfm_bwd_buckets(dq_tfm* tfm, const float* params, const float* rope_sin, const float* rope_cos, const float* x_t,
                       const float* x_cond, const float* dout, float* grads, int accumulate, float* dx_t, float* dx_cond,
                       void* workspace, int64_t workspace_bytes, int B, int S1, int S2, void* stream,
                       dq_tfm_bucket_fn on_bucket, void* user);
int dq_tfm_num_buckets(const dq_tfm* tfm);
int dq_tfm_bucket_info(const dq_tfm* tfm, int i, int64_t* offset, int64_t* count); /* floats, into the flat buffer */
/* Arithmetic of the transformer's dense products: DQ_PRECISION_FP32 (default) = exact fp32 on v_mfma_f32_32x32x2_f32, the precision
 * every parity statement of this library is made in; DQ_PRECISION_BF16X3 = three bf16 matrix-core passes over operands split into
 * hi + lo bf16 halves with fp32 accumulation (~16 mantissa bits per operand, relative error ~1e-5 per product term): a separate,
 * faster mode with its own stated tolerance, never the default. */
enum { DQ_PRECISION_FP32 = 0, DQ_PRECISION_BF16X3 = 1 };
int dq_tfm_set_precision(dq_tfm* tfm, int precision);
/* The kernels between the transformer's GEMMs (csrc/k_tfm.hip), one launcher each on tensors the caller chooses (additive at ABI
 * version 12; exported for the parity tests).  Asynchronous on `stream`, nothing is allocated; null operands, non-positive sizes, an odd H
 * where channel pairs are rotated and a short scratch are refused with an error.  All tensors fp32 and contiguous unless a stride is given.
 *   rope_add:       x (B, S, H) in place: adjacent channel pairs rotated by the tables sin / cos (S, H/2), then += temb[b] (B, H; nullable);
 *                   inverse != 0: the transposed rotation (the gradient), temb ignored.  x 8-byte aligned.
 *   cond_embed:     c (B, S, H) = rope(x_cond[b][s] * w + bias), w and bias (H); its backward from dc (B, S, H): dw, db (H each) and
 *                   dx_cond (B, S; nullable, a plain store).  scratch: 2 * H * 64 floats.  c and dc 8-byte aligned.
 *   time_features:  e (B, H) = [sin(t_b f) | cos(t_b f)], t (B) int64, f (H/2), the product t_b f formed in fp32.
 *   gelu:           y = x Phi(x) (exact erf form); gelu_bwd: dx = dy * gelu'(x), dx may be dy itself.
 *   layernorm_fwd:  y = x + r (r nullable), out = (y - mean) * rstd * g + b over rows of H (biased variance, eps 1e-5 inside the root),
 *                   stats (rows, 2) = mean, rstd (nullable).  layernorm_bwd: dy (rows, H) a plain store; dg, db (H each) from y, stats and
 *                   dout.  scratch: 2 * H * 256 floats.  dq_tfm_layernorm_form: which kernels both take for rows of H floats whose row
 *                   operands are (aligned16 != 0) or are not all 16-byte aligned -- forward: x, r, g, b, y, out; backward: y, g, dout, dy.
 *   softmax_rows:   rows of n floats at stride ld, in place: p = softmax(scale * p); columns n .. ld-1 are neither read nor written.
 *                   softmax_rows_bwd: dp = p * (dp - sum(p dp)) * scale in place of dp.
 *   colsum:         out[n] = sum over m < M of x[m * ld + n]; scratch: 64 * N floats.  seqsum: out (B, N) = sum over s of x (B, S, N).
 * accumulate != 0: `+=` into dw / db, dg / db, out; 0: plain stores. */
enum { DQ_LN_REG4 = 0, DQ_LN_REG16 = 1, DQ_LN_BLK = 2, DQ_LN_ROWS = 3 };
int dq_tfm_layernorm_form(int H, int aligned16);
int dq_tfm_rope_add(float* x, const float* rope_sin, const float* rope_cos, const float* temb, int B, int S, int H, int inverse,
                    void* stream);
int dq_tfm_cond_embed(const float* x_cond, const float* w, const float* bias, const float* rope_sin, const float* rope_cos, float* c,
                      int B, int S, int H, void* stream);
int dq_tfm_cond_embed_bwd(const float* dc, const float* x_cond, const float* w, const float* rope_sin, const float* rope_cos, float* dw,
                          float* db, float* dx_cond, float* scratch, int64_t scratch_floats, int B, int S, int H, int accumulate,
                          void* stream);
int dq_tfm_time_features(const int64_t* t, const float* freqs, float* e, int B, int H, void* stream);
int dq_tfm_gelu(const float* x, float* y, int64_t n, void* stream);
int dq_tfm_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
int dq_tfm_layernorm_fwd(const float* x, const float* r, const float* g, const float* b, float* y, float* out, float* stats, int rows,
                         int H, void* stream);
int dq_tfm_layernorm_bwd(const float* y, const float* stats, const float* g, const float* dout, float* dy, float* dg, float* db,
                         float* scratch, int64_t scratch_floats, int rows, int H, int accumulate, void* stream);
int dq_tfm_softmax_rows(float* p, int64_t rows, int n, int ld, float scale, void* stream);
int dq_tfm_softmax_rows_bwd(const float* p, float* dp, int64_t rows, int n, int ld, float scale, void* stream);
int dq_tfm_colsum(const float* x, int M, int N, int64_t ld, float* out, float* scratch, int64_t scratch_floats, int accumulate,
                  void* stream);
int dq_tfm_seqsum(const float* x, int B, int S, int N, float* out, void* stream);
/* The inference attention of the transformer's sampling path (csrc/k_tfm_attn.hip; additive at ABI version 12): per (sample, head)
 * o = softmax(q k^T / sqrt(dh)) v with q (B, S1, H), kv (B, Sk, 2H) = the K | V halves, o (B, S1, H), dh = H / heads; all 16-byte aligned.
 * Two forms, both fp32 with a max-subtracted softmax and bitwise repeatable: DQ_TFM_ATTN_FUSED one launch that writes nothing but o (fp32
 * VALU also when the handle's GEMMs run in bf16x3); DQ_TFM_ATTN_GEMM the training path's three launches (scores GEMM, softmax rows, PV GEMM)
 * through prob_scratch (B * heads * S1 * up4(Sk) floats; unused and nullable for the fused form).  dq_tfm_attn_form (host only, no device
 * needed): the form a sampling forward takes -- fused when dh % 4 == 0 and
 *   4 * (Sk * (2 dh + 4) + 4 dh + 4 up4(Sk)) <= 160 KiB   (K, V and four waves' q and p rows in one CU's LDS),
 * which holds for every Sk <= 68 at dh <= 128; -1 for a non-positive size.  dq_tfm_attn_fwd: form -1 = the chosen one, 0 / 1 forced;
 * a forced fused form on a shape the predicate refuses is an error, never a silent fallback. */
enum { DQ_TFM_ATTN_GEMM = 0, DQ_TFM_ATTN_FUSED = 1 };
int dq_tfm_attn_form(int S1, int Sk, int dh);
int dq_tfm_attn_fwd(const float* q, const float* kv, float* o, float* prob_scratch, int B, int S1, int Sk, int H, int heads, int form,
                    void* stream);
/* Sampling from the transformer in one call (csrc/dq_tfm_sample.hip): dq_ddim_sample's loop -- the same record, the same
 * tables, updates, draw indexing (x_T at 0, step i at 1 + i), refusals (worded alike, before anything touches the device) and final
 * un-normalisation -- around a sampling forward of this network; the same code, not a copy (csrc/dq_sampler.h: the captured step and the
 * eager steps take the network's forward as a callable).  x_T (B, S1, input_dim; NULL: drawn from the seed), ms2_cond like x_T (the
 * network ignores it: out_noise = mixture - out_x), ms1_cond (B, S2).  Once per call, before the loop: the conditional embedding of ms1_cond
 * (2c - 1 first when auto_normalize), every layer's K | V rows of it, and the time embedding of every step; a step then projects only the x_t
 * rows and runs the attention by dq_tfm_attn_form.  use_graph != 0 without trajectories: one step is captured once, cached on the handle
 * (dropped by dq_tfm_set_precision and dq_tfm_destroy) and replayed num_steps times; seed and ids are staged in the workspace.
 * workspace: dq_tfm_sample_workspace_bytes(tfm, B, S1, S2, num_steps) bytes, 16-byte aligned.  call->RT is S1.  eta, seed, ids, the sampler
 * and clip_x0 are served; `guided`, a live per-window option and consistency != DQ_CONSIST_NONE are refused (not built for this network
 * yet), behind the refusals the shared checks make and in front of the size checks -- never silently ignored. */
int64_t dq_tfm_sample_workspace_bytes(const dq_tfm* tfm, int B, int S1, int S2, int num_steps);
int dq_tfm_sample(dq_tfm* tfm, const float* params, const float* rope_sin, const float* rope_cos, const float* time_freqs, int S2,
                  const dq_sample_call* call);
/* Held-out evaluation of the transformer in one call per batch (csrc/dq_tfm_sample.hip, csrc/k_stream.hip, DESIGN.md sections 31 and 36;
 * additive at ABI version 12): dq_eval_step's semantics for `repeats` = R repeats of a batch of B windows stacked into N = R * B samples,
 * sample n = r * B + b (repeat-major), through ONE forward -- dq_tfm_sample's prologue and forward, the same code.
 *   x0 (B, S1, input_dim), shared by the repeats and not replicated; ms1_cond (B, S2) raw (2c - 1 first when auto_normalize); t (R, B) int64
 *   on the device; noise (R, B, S1, input_dim) or NULL: then seed_dev is required and the noise of (r, b) is
 *   philox_normal(seed, window_ids ? ids[b] : b, e, first_draw + r) -- what dq_randn(draw = first_draw + r) writes -- evaluated inside the
 *   kernels and never written to memory.  There is no ms2_cond: this network has no input for it.
 *   per_window_out (R, B): the unweighted MSE of the network output against its target (DQ_PRED_EPS: the noise; DQ_PRED_X0: x0 * cm + ca);
 *   loss_out (R): (float)(sum_b lw[t[r, b]] * mse[r, b] / B), summed in fp64 in index order; loss_weight_dev is required for x0 and ignored
 *   for eps.  The MSE part only.  net_out (nullable): receives the network output (R, B, S1, input_dim); otherwise it lives in the workspace.
 * The conditional embedding and every layer's K | V rows of it are computed once for the B windows and copied to the other R - 1 repeats
 * (R == 1: no copy); the time MLP runs once over the N timesteps.  Eager only, nothing cached across calls; neither the handle's saved
 * forwards nor any training workspace is touched; honours dq_tfm_set_precision.  Refused with a message: a null required argument, an
 * unknown pred_type, repeats < 1, R * B > 65535, noise == NULL without seed_dev, first_draw < 0, params / workspace / x0 (noise, net_out)
 * not 16-byte aligned, a workspace below dq_tfm_eval_workspace_bytes(tfm, B, S1, S2, repeats) (0 on a bad argument; host only).
 * Two identical calls give identical bits; a window's value at another B or R agrees to rounding only (the GEMM plan follows the row count). */
int64_t dq_tfm_eval_workspace_bytes(const dq_tfm* tfm, int B, int S1, int S2, int repeats);
int dq_tfm_eval_step(dq_tfm* tfm, const float* params, const float* rope_sin, const float* rope_cos, const float* time_freqs,
                     const float* alpha_bars_dev, const float* x0, const float* ms1_cond, const int64_t* t, const float* noise,
                     const uint64_t* seed_dev, const int64_t* window_ids_dev, int first_draw, int auto_normalize, int pred_type,
                     const float* loss_weight_dev, float* loss_out, float* per_window_out, float* net_out, void* workspace,
                     int64_t workspace_bytes, int B, int S1, int S2, int repeats, void* stream);
/* Its three streaming kernels alone (csrc/k_stream.hip, csrc/k_tfm.hip).  per_window % 4 == 0 and 16-byte aligned tensors for the first, like
 * dq_ddim_step_sto.
 * dq_q_sample_repeats: x_t (R, B, per_window) = sa * norm(x0[b]) + sb * z[r, b] with sa, sb from alpha_bars[t[r, b]]: dq_q_sample's
 * arithmetic on x0 (B, per_window); z read from noise (R, B, per_window) or, noise == NULL, drawn at draw index first_draw + r.
 * dq_mse_per_window_repeats: dq_mse_per_window per repeat on out (R, B, per): the target has target_windows = B (shared by the repeats) or
 * R * B windows, or is drawn (target == NULL: the noise above); per_window_out (R, B), loss_out (R); scratch:
 * dq_mse_per_window_scratch_bytes(R * B, per) bytes.  Bit for bit dq_mse_per_window applied to each repeat.
 * dq_tfm_kv_broadcast: kv (R * B, Sk, 2H), 16-byte aligned: rows [0, S2) of samples 0 .. B-1 copied to samples B .. R * B - 1; nothing else
 * is written, and nothing at all when repeats == 1. */
int dq_q_sample_repeats(const float* alpha_bars_dev, const float* x0, const int64_t* t, const float* noise, const uint64_t* seed_dev,
                        const int64_t* window_ids_dev, int first_draw, float* x_t, int B, int repeats, int64_t per_window, int normalize_x0,
                        void* stream);
int dq_mse_per_window_repeats(const float* out, const float* target, int target_windows, float tm, float ta, const uint64_t* seed_dev,
                              const int64_t* window_ids_dev, int first_draw, const float* lw, const int64_t* t, float* per_window_out,
                              float* loss_out, void* scratch, int B, int repeats, int64_t per, void* stream);
int dq_tfm_kv_broadcast(float* kv, int B, int repeats, int S2, int Sk, int H, void* stream);
/* The fp32 matrix-core GEMM underneath (exported for the parity tests and the roofline measurement):
 * C (M,N; ldc) = A B (+ bias[n]) with A(m,k) = a_kmajor ? A[m*lda+k] : A[k*lda+m] and B(k,n) = b_kmajor ? B[n*ldb+k] :
 * B[k*ldb+n]; splits = 0 lets the library choose a split-K factor; scratch: dq_gemm_scratch_floats(M,N,K) floats. */
int64_t dq_gemm_scratch_floats(int M, int N, int K);
int dq_gemm(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int64_t lda, int64_t ldb,
            int64_t ldc, int a_kmajor, int b_kmajor, int accumulate, int splits, float* scratch, int64_t scratch_floats,
            void* stream);
/* The same product in the DQ_PRECISION_BF16X3 arithmetic. */
int dq_gemm_bf16x3(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int64_t lda, int64_t ldb,
                   int64_t ldc, int a_kmajor, int b_kmajor, int accumulate, int splits, float* scratch, int64_t scratch_floats,
                   void* stream);
/* The same launcher with every operand mode the library itself uses, on a caller-filled descriptor (additive at ABI version 12; exported
 * for the parity tests).  Zero-initialise the struct, then set batch = inner = kbatch = 1 and alpha = 1 for a plain product.
 *   C[z](m, n) (+)= alpha * sum over b < kbatch, k < K of A[z][b](m, k) B[z][b](k, n) + bias[n] + bias_m[m] (+ add[z](m, n))
 * z = zo * inner + zi < batch; operand offsets in floats: A[z][b] = A + zo sAo + zi sAi + b sAk, B likewise, C[z] = C + zo sCo + zi sCi;
 * add is laid out like C.  Required (refused with an error otherwise): lda, ldb, the strides of A and B multiples of 4, A and B 16-byte
 * aligned, K > 0 (any length), inner > 0, kbatch >= 1, not (a_kmajor = 0 with b_kmajor = 1), add only with accumulate = 0 and an unsplit
 * plan, batch x splits <= 65535, scratch of at least the floats dq_debug_gemm_plan reports.  M, N or batch <= 0: nothing to do, returns 0.
 * Rows / columns beyond M, N, K are never read into a result, and nothing outside the (M x N) window of a C[z] is written. */
typedef struct dq_gemm_desc {
  const float* A; const float* B; float* C;
  const float* bias;   /* (N), nullable */
  const float* bias_m; /* (M), nullable */
  const float* add;    /* nullable */
  float* scratch;      /* split-K partial tiles; nullable when the plan is unsplit */
  int64_t scratch_floats;
  int64_t lda, ldb, ldc;
  int64_t sAo, sAi, sBo, sBi, sCo, sCi;
  int64_t sAk, sBk;
  int32_t M, N, K;
  int32_t a_kmajor, b_kmajor;
  int32_t batch, inner, kbatch;
  int32_t accumulate;
  int32_t splits;      /* 0: chosen by the library; > 0: forced (capped at the number of k-tiles) */
  int32_t precision;   /* DQ_PRECISION_FP32 or DQ_PRECISION_BF16X3 */
  float alpha;
} dq_gemm_desc;
int dq_gemm_ex(const dq_gemm_desc* desc, void* stream);
/* Test hook: what the launcher does with a product of this shape -- evaluated by the launcher's own planning function, without a launch
 * or a device.  A product runs as up to two launches over disjoint ranges of its tile grid (cdiv(M, bm) x cdiv(N, 128) tiles, m fastest):
 * `full`, the whole rounds of 256 tiles, unsplit, and `rest`, the remaining tiles, possibly with the reduction split.  out receives
 * DQ_GEMM_PLAN_INTS ints: bm (32, 64 or 128), kv (the reduction length the splits cut: K, or kbatch * (K rounded up to 32) when
 * kbatch > 1), then tile_base, ntiles, splits, k_per_split of `full` and of `rest`.  *scratch_floats (nullable) receives the floats
 * dq_gemm_ex asks of `scratch` for this product (0: none), for any batch -- dq_gemm_scratch_floats covers batch = kbatch = 1, splits = 0.
 * Returns the number of ints written, or -1 (null out, cap too small, M, N, K, batch or kbatch < 1, splits < 0). */
enum { DQ_GEMM_PLAN_INTS = 10 };
int dq_debug_gemm_plan(int M, int N, int K, int batch, int kbatch, int splits, int32_t* out, int cap, int64_t* scratch_floats);

/* ---- building blocks exported for the per-block parity tests (tests/test_blocks_gpu.py) ------------------------
 * Each runs the SAME kernels / dispatch the network uses, on caller-supplied tensors, so that the reference's per-block
 * fixtures (tests/golden/blocks.npz) reach the HIP code directly.
 * Residual(PreNorm(LinearAttention)) (unet1d.py:446-496, 1017) on (rows, C, n). */
int dq_linattn_fwd(const float* x, float* y, float* ypre /* nullable: pre-norm output saved for the backward */,
                   const float* w_qkv, const float* w_out, const float* b_out, const float* g_pre, const float* g_out, int C,
                   int rows, int n, void* stream);
/* The same block the way the network runs it: the layer's derived weights (W2 = Wo Wv per head, the MFMA operand images of Wq | Wk --
 * fp32 and, for 4 / 8 channels, split-bf16 -- and the bounded-logit flag) are formed ONCE per parameter state by dq_linattn_prepare into
 * `prep` (dq_linattn_prep_floats() floats, 16-byte aligned) and every forward launch copies them instead of deriving them per workgroup.
 * n: a power of two <= 64. */
int64_t dq_linattn_prep_floats(void);
int dq_linattn_prepare(const float* w_qkv, const float* w_out, const float* g_pre, int C, float* prep, void* stream);
int dq_linattn_fwd_prepared(const float* x, float* y, float* ypre, const float* w_qkv, const float* w_out, const float* b_out,
                            const float* g_pre, const float* g_out, const float* prep, int C, int rows, int n, void* stream);
/* Backward: dx += d/dx, parameter gradients +=.  ypre from the forward; scratch: 2*rows*C*n + 2048*512*C floats. */
int dq_linattn_bwd(const float* x, const float* ypre, const float* dy, float* dx, const float* w_qkv, const float* w_out,
                   const float* b_out, const float* g_pre, const float* g_out, float* dw_qkv, float* dw_out, float* db_out,
                   float* dg_pre, float* dg_out, float* scratch, int C, int rows, int n, void* stream);
/* The same backward with dx written instead of accumulated (its prior contents are ignored), the way the network runs it; parameter
 * gradients still +=. */
int dq_linattn_bwd_store(const float* x, const float* ypre, const float* dy, float* dx, const float* w_qkv, const float* w_out,
                         const float* b_out, const float* g_pre, const float* g_out, float* dw_qkv, float* dw_out, float* db_out,
                         float* dg_pre, float* dg_out, float* scratch, int C, int rows, int n, void* stream);
/* Which kernels the calls above take for this shape under the current options (16-byte aligned caller tensors assumed): *fwd_form =
 * DQ_LA_FWD_* of dq_linattn_fwd_prepared (prepared != 0; rows of 1 .. 64 positions, powers of two) or of dq_linattn_fwd (prepared == 0),
 * *bwd_form = DQ_LA_BWD_* of dq_linattn_bwd / dq_linattn_bwd_store.  Forward: k_la_long.hip (LONG), k_la_small.hip (SMALL),
 * k_la_rows_fwd.hip (ROWS), k_linattn.hip (REG).  Backward: k_la_long.hip between two norm-backward launches (LONG), k_la_rows_bwd.hip
 * (ROWS), k_la_bwd.hip (REG).  Launches nothing.  Bad shape: non-zero. */
enum { DQ_LA_FWD_LONG = 0, DQ_LA_FWD_SMALL = 1, DQ_LA_FWD_ROWS = 2, DQ_LA_FWD_REG = 3 };
enum { DQ_LA_BWD_LONG = 0, DQ_LA_BWD_ROWS = 1, DQ_LA_BWD_REG = 2 };
int dq_linattn_forms(int C, int rows, int n, int prepared, int* fwd_form, int* bwd_form);
/* RMSNorm (unet1d.py:113-140): y = x / max(||x||_2 over C, 1e-12) * g * sqrt(C) on (rows, C, n); C in {4, 8, 12, 16, 32}. */
int dq_rmsnorm_fwd(const float* x, const float* g, float* y, int C, int rows, int n, void* stream);
/* SinusoidalPosEmb(4) -> Linear(4,16) -> GELU -> Linear(16,16) (unet1d.py:196-218, 956-960): t (B) int64 -> sinu_out (B,4),
 * temb_out (B,16) (either nullable).  scratch: 100 * B floats. */
int dq_time_mlp_fwd(const float* w1, const float* b1, const float* w2, const float* b2, const int64_t* t, float* sinu_out,
                    float* temb_out, float* scratch, int B, void* stream);
/* SiLU -> Linear(16, m) head hanging off the time embedding (ResnetBlock.mlp unet1d.py:292-296; ConditionalScaleShift
 * :662-678): temb (B,16), w (m,16), b (m) -> ss (B,m). */
int dq_scale_shift_fwd(const float* temb, const float* w, const float* b, float* ss, int B, int m, void* stream);
/* attn_cond_proj.1.0 + GELU on a multi-channel MS1 (k_ms1_feat.hip; unet1d.py:976, 1122-1130), 1 <= M1 <= 4096: ms1 (B, RT, M1) raw,
 * w (8, M1, 7), bias (8):  u[b][c][rt] = bias[c] + sum_tap sum_m w[c][m][tap] * n(ms1[b][rt+tap-3][m]),  n(v) = v*cond_mul+cond_add, rows
 * outside 0..RT-1 contributing nothing.  a_out (B, 8, RT) = GELU(u); u_out (B, 8, RT) and ms1n_out (B, RT, M1) = n(ms1) nullable. */
int dq_ms1_feat_fwd(const float* ms1, const float* w, const float* bias, float cond_mul, float cond_add, float* ms1n_out, float* u_out,
                    float* a_out, int B, int RT, int M1, void* stream);
/* Its weight and bias gradient: dw (8, M1, 7) += sum_{b,rt} du[b][c][rt] * ms1n[b][rt+tap-3][m], dbias (8) += sum du, from the NORMALISED
 * ms1n (B, RT, M1) and du (B, 8, RT).  One slot per workgroup in `scratch` (dq_ms1_feat_wgrad_scratch_floats floats; -1 for arguments
 * out of range) and an ordered sum: no float atomics, bitwise repeatable. */
int64_t dq_ms1_feat_wgrad_scratch_floats(int B, int RT, int M1);
int dq_ms1_feat_wgrad(const float* ms1n, const float* du, float* dw, float* dbias, float* scratch, int64_t scratch_floats, int B, int RT,
                      int M1, void* stream);
/* The first layer's inputs at attn_cond_channels = 1 (unet1d.py:1107-1115, 1122-1124): cat0 (B*RT, 2, MZ) = [ (cond*cond_mul+cond_add) * (scale_b + 1) +
 * shift_b , x ], ms1n (B, RT) = ms1*cond_mul+cond_add; ss (B, 2) = [scale, shift] per sample. */
int dq_prep_inputs_fwd(const float* x, const float* cond, const float* ms1, const float* ss, float cond_mul, float cond_add, float* cat0,
                       float* ms1n, int B, int RT, int MZ, void* stream);
/* Its backward for the per-sample [scale, shift] (k_prep_inputs_bwd + the ordered sum of its per-block partials): from dcat0 (B*RT, 2, MZ),
 * of which channel 0 is read, and the RAW cond (B, RT, MZ):  dss[b * ss_stride + ss_off] += sum d * (cond*cond_mul+cond_add),
 * dss[b * ss_stride + ss_off + 1] += sum d, the sums over sample b's RT * MZ elements in a fixed order (bitwise repeatable).  ss_stride >=
 * ss_off + 2.  scratch: dq_prep_inputs_bwd_scratch_floats(B, RT, MZ) floats (-1 for arguments out of range). */
int64_t dq_prep_inputs_bwd_scratch_floats(int B, int RT, int MZ);
int dq_prep_inputs_bwd(const float* dcat0, const float* cond, float cond_mul, float cond_add, float* dss, int ss_stride, int ss_off, int B,
                       int RT, int MZ, float* scratch, int64_t scratch_floats, void* stream);
/* Conv1d (+ optional fused RMSNorm with gain norm_g, + optional activation) on (rows, cin, n_in) -> (rows, cout, n_out):
 * mode 0 = stride 1 'same' (K in {1,3,7}), 1 = Downsample k4 s2 p1 (unet1d.py:99-110), 2 = Upsample nearest x2 then k3 p1
 * (:82-96).  act: 0 none, 1 SiLU, 2 GELU.  bias / norm_g nullable. */
int dq_conv_fwd(const float* x, const float* w, const float* bias, const float* norm_g, int act, float* y, int cout, int cin, int K, int mode,
                int rows, int n_in, int n_out, void* stream);
/* Backward of dq_conv_fwd without norm / act (norm_g = NULL, act = 0) on the input cat(xA (rows, cinA, n_in), xB (rows, cinB, n_in)) (xB
 * nullable with cinB = 0), through the network's own dispatch: the one-launch k_conv_bwd_wg (k_conv_wg.hip) where a level's resample conv
 * takes it, else the data gradient on the batched GEMM (the bottleneck attention's bias-free 1x1 projections; needs a 16-byte aligned w) or
 * k_conv_bwd_data, and the weight gradient by k_conv_wgrad[_v4] + k_wgrad_reduce -- all on `stream`.
 * w (cout, cinA + cinB, K); dy (rows, cout, n_out) = d loss / d y.  dxA / dxB (nullable): accumulate != 0: +=, else plain stores.
 * dparams: [dW (cout, cinA + cinB, K) | dbias (cout) iff has_bias], contiguous as in the flat gradient buffer, += always.
 * rows_per_sample: RT at the m/z levels (rows = B * rows_per_sample).  workspace: dq_conv_bwd_workspace_floats floats, 16-byte aligned
 * (-1 for a bad shape). */
int64_t dq_conv_bwd_workspace_floats(int cout, int cinA, int cinB, int K, int mode, int rows, int n_in, int n_out, int rows_per_sample);
int dq_conv_bwd(const float* xA, int cinA, const float* xB, int cinB, const float* w, const float* dy, float* dxA, float* dxB, float* dparams,
                int has_bias, int cout, int K, int mode, int rows, int n_in, int n_out, int rows_per_sample, int accumulate, float* workspace,
                int64_t workspace_floats, void* stream);
/* Which kernels dq_conv_bwd takes for this shape (w 16-byte aligned iff w_aligned != 0, every other tensor aligned): *data_form =
 * DQ_CONV_BWD_DATA_* (k_conv_bwd_wg | the batched GEMM | k_conv_bwd_data), *wgrad_form = DQ_CONV_WGRAD_* (k_conv_bwd_wg | k_conv_wgrad_v4 |
 * k_conv_wgrad).  WG is both or neither.  Launches nothing.  Bad shape: non-zero. */
enum { DQ_CONV_BWD_DATA_WG = 0, DQ_CONV_BWD_DATA_GEMM = 1, DQ_CONV_BWD_DATA_PLAIN = 2 };
enum { DQ_CONV_WGRAD_WG = 0, DQ_CONV_WGRAD_V4 = 1, DQ_CONV_WGRAD_SCALAR = 2 };
int dq_conv_bwd_forms(int cout, int cinA, int cinB, int K, int mode, int rows, int n_in, int n_out, int rows_per_sample, int has_bias,
                      int w_aligned, int* data_form, int* wgrad_form);
/* ResnetBlock (unet1d.py:271-323) on input cat(xA (rows,cinA,n), xB (rows,cinB,n)) (xB nullable with cinB = 0) with the time
 * embedding temb (rows / rows_per_sample, 16).  params: the block's tensors in state_dict order as ONE flat buffer
 * [mlp.1.weight, mlp.1.bias, block1.proj.weight, block1.proj.bias, block1.norm.g, block2.proj.weight, block2.proj.bias,
 * block2.norm.g (, res_conv.weight, res_conv.bias iff cinA+cinB != cout)].  rows_per_sample: RT at the m/z levels, 1 at the
 * bottleneck.  workspace: dq_resblock_workspace_floats floats, shared by the forward (save_for_bwd = 1) and its backward. */
int64_t dq_resblock_workspace_floats(int cin, int cout, int rows, int n, int rows_per_sample);
int dq_resblock_fwd(const float* params, const float* xA, int cinA, const float* xB, int cinB, const float* temb, float* out, int cout,
                    int rows, int n, int rows_per_sample, int save_for_bwd, float* workspace, int64_t workspace_floats, void* stream);
/* Backward of the call above: dxA / dxB += (zero them first; nullable), grads (same layout as params) += for the conv / norm
 * tensors; dss (rows / rows_per_sample, 2*cout) = d loss / d [scale | shift] (the mlp's gradients follow from it:
 * d mlp.1.bias = sum_b dss_b, d mlp.1.weight = sum_b dss_b (x) SiLU(temb_b); the network does that in its time-embedding backward). */
/* dout == NULL (benchmarks): the gradient of the block output is already in the workspace at dq_resblock_dout_offset(...) floats;
 * dxA / dxB are then plain stores, dss is not copied out, and the call consists of the backward launches only. */
int64_t dq_resblock_dout_offset(int cin, int cout, int rows, int n, int rows_per_sample);
int dq_resblock_bwd(const float* params, const float* xA, int cinA, const float* xB, int cinB, const float* dout, float* dxA, float* dxB,
                    float* grads, float* dss, int cout, int rows, int n, int rows_per_sample, float* workspace, int64_t workspace_floats,
                    void* stream);
/* Which kernels dq_resblock_fwd / dq_resblock_bwd take for this shape under the current options (16-byte aligned caller tensors assumed):
 * *fwd_form = DQ_RES_FWD_*, *bwd_form = DQ_RES_BWD_*.  Forward: k_res_rt.hip (RT), a one-block k_level.hip launch (LEVEL), k_res_v4.hip (V4),
 * the conv launches (UNFUSED).  Backward: k_res_wg.hip (WG), k_res_rt.hip (RT), k_res_rows.hip (ROWS), k_res_cp.hip (CP), k_res.hip (PLAIN),
 * the step-by-step launches (UNFUSED).  Launches nothing.  Bad shape: non-zero. */
enum { DQ_RES_FWD_RT = 0, DQ_RES_FWD_LEVEL = 1, DQ_RES_FWD_V4 = 2, DQ_RES_FWD_UNFUSED = 3 };
enum { DQ_RES_BWD_WG = 0, DQ_RES_BWD_RT = 1, DQ_RES_BWD_ROWS = 2, DQ_RES_BWD_CP = 3, DQ_RES_BWD_PLAIN = 4, DQ_RES_BWD_UNFUSED = 5 };
int dq_resblock_forms(int cinA, int cinB, int cout, int rows, int n, int rows_per_sample, int* fwd_form, int* bwd_form);
/* The convolutional part of a U-Net level in ONE launch (unet1d.py:1134-1142, 1150-1158, 1160-1163; k_level.hip):
 *   out_i = ResnetBlock_i(cat(h, skip_i)),  h = stage(x) for i = 0, h = out_0 for i = 1
 * pre: 0 none (x is (rows, C, n)), 1 Downsample k4 s2 (x is (rows, cp, 2n)), 2 Upsample nearest x2 + k3 (x is (rows, cp, n/2)), 3 k3 conv
 * (x is (rows, cp, n)); skip_i (rows, cs, n), nullable with cs = 0 (then the residual is the identity); temb (rows / rows_per_sample, 16).
 * params: [stage weight (C, cp, K) | stage bias (C)] (pre != 0), then nblocks (1 or 2) blocks in the dq_resblock_fwd layout with
 * cin = C + cs (dq_level_param_floats floats in all).  out0 nullable when nblocks = 2 (inference on the way up keeps only out1).
 * n: a power of two <= 64; C in {4, 8, 12, 16}.  workspace: 2 * (rows / rows_per_sample) * 2 * C floats; with 8256 floats more (and 16-byte
 * aligned) the MFMA operand image of the weights is built there by one launch of its own and the workgroups copy it, as in the network
 * path, instead of each gathering it from the parameter tensors. */
int64_t dq_level_param_floats(int pre, int C, int cp, int cs, int nblocks);
int dq_level_fwd(const float* params, int pre, const float* x, int cp, const float* skip0, const float* skip1, int cs, const float* temb,
                 float* out0, float* out1, int C, int nblocks, int rows, int n, int rows_per_sample, float* workspace,
                 int64_t workspace_floats, void* stream);
/* RoPE of the bottleneck attention (rotary_embedding_torch 'lang' mode as restated in DESIGN.md section 5; unet1d.py:529,
 * 560-561), in place on the 4 heads x 32 channels at the start of each sample of qk (B, >=128, RT); batch_stride in floats;
 * sign +1 forward, -1 the transposed rotation (backward). */
int dq_rope(float* qk, const float* freqs, int B, int64_t batch_stride, int RT, float sign, void* stream);
/* softmax(q k^T 32^-0.5) v over RT (unet1d.py:428-443) for q, k, v, o (B, 128, RT) = 4 heads x 32 channels, RT contiguous;
 * lse (B*4*RT) receives the log-sum-exp the backward needs. */
int dq_attn_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int RT, void* stream);
/* Backward: dq, dk, dv (B, 128, RT) are plain stores; delta: B*4*RT floats of scratch. */
int dq_attn_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o, const float* lse, float* delta,
                float* dq, float* dk, float* dv, int B, int RT, void* stream);

/* ---- the wide bottleneck's kernels alone (csrc/k_wide.hip; tests/test_wide_mid.py) ------------------------------------------------
 * The launchers the wide bottleneck (every mid_c but 16 and 32) is made of, on caller tensors.  A tensor is (B, C, P): P = RT rounded up to a
 * multiple of 4 floats (RT <= P < RT + 4), columns t < RT valid, the rest pad.  Every kernel writes ZERO into the pad columns of its outputs
 * and never lets an input's pad columns reach a valid output.  All reductions are fixed-order: a repeated call is bitwise identical.  Each
 * entry refuses null required operands, non-positive sizes, a P that is not the multiple of 4 in [RT, RT + 4) and (dq_wide_norm_bwd) a
 * short scratch before any launch.
 *
 * dq_wide_im2col3: xcol (B, 3 C, P), xcol[b][3 c + k][t] = x[b][c][t + k - 1], zero outside [0, RT): Conv1d(k 3, padding 1) as a product.
 * dq_wide_col2im3: its transpose, dx[b][c][t] (+)= sum_k dxcol[b][3 c + k][t - k + 1]; accumulate != 0: += on the valid columns.
 * dq_wide_repitch: dst (rows, dpitch) <- src (rows, spitch), n valid columns, the rest of a dst row zero (one pitch is n .. n + 3 rounded to
 *   a multiple of 4, the other anything in [n, n + 4): the attention kernels read rows of RT floats).
 * dq_wide_norm_fwd: y = act(u / max(||u[b][:][t]||_2, 1e-12) * g[c] * sqrt(C) * (ss[b][c] + 1) + ss[b][C + c]) + res  (unet1d.py:113-140,
 *   302-323).  ss (nullable): sample b's [scale (C) | shift (C)] at ss + b * ss_stride; act 0 none, 1 SiLU; res (nullable) (B, C, P).
 * dq_wide_norm_bwd: du (B, C, P) = d loss / d u from dy = d loss / d y (without the residual); dg (C) += ; dss (same layout and stride as
 *   ss; required with ss) += d [scale | shift]; dbias (C, nullable) += sum over (b, t) of du (the bias gradient of the conv that made u).
 *   du may be dy (in place).  Where ||u|| < 1e-12 the forward is linear in u (the clamp) and so is du.  scratch:
 *   dq_wide_norm_bwd_scratch_floats(B, C, P) = B (2 P + 2 C) floats (-1 for non-positive sizes).
 * dq_wide_rowsum: out[r] = sum over t < RT of x (rows, P)[r][t].
 * dq_wide_sum_b: dst[c] += sum over b (in order) of part (B, C)[b][c]. */
int dq_wide_im2col3(const float* x, float* xcol, int B, int C, int RT, int P, void* stream);
int dq_wide_col2im3(const float* dxcol, float* dx, int B, int C, int RT, int P, int accumulate, void* stream);
int dq_wide_repitch(float* dst, int dpitch, const float* src, int spitch, int64_t rows, int n, void* stream);
int dq_wide_norm_fwd(const float* u, const float* g, const float* ss, int ss_stride, int act, const float* res, float* y, int B, int C, int RT,
                     int P, void* stream);
int64_t dq_wide_norm_bwd_scratch_floats(int B, int C, int P);
int dq_wide_norm_bwd(const float* u, const float* dy, const float* g, const float* ss, int ss_stride, int act, float* du, float* dg, float* dss,
                     float* dbias, float* scratch, int64_t scratch_floats, int B, int C, int RT, int P, void* stream);
int dq_wide_rowsum(const float* x, int64_t rows, int RT, int P, float* out, void* stream);
int dq_wide_sum_b(const float* part, int B, int C, float* dst, void* stream);

/* Test hook: offset (in floats) of a named activation inside the workspace laid out by the last call on this plan
 * ("h0", "ms1f", "down3", "down3.la", "mid1", "mid1.u1", "mid2.a1", "lse", "attn_out", "mid_back", "up0", "fin", "eps", ...; on a wide plan also its (B, channels, P) slots "w_mid_in", "wmid1", "wmid1.u1", "wmid1.a1",
 * "wmid1.u2", the same of "wmid2", "w_xn", "w_qv", "w_o", "w_attn_out" and its scratch "w_xcol", "w_stats", "w_gemm_part"), or -1.  "@twin": the
 * distance in floats from the start of a training workspace to its gradient twin (a tensor's gradient lies at the tensor's offset there). */
int64_t dq_debug_tensor_offset(dq_plan* plan, const char* name);

/* Test hook: lays the plan's workspace out for (B, RT) as the first pass at that shape would, on the host alone: dq_debug_tensor_offset
 * answers for that shape afterwards, before any call at it.  Returns 0, or -1 (null plan, B or RT < 1). */
int dq_debug_layout(dq_plan* plan, int B, int RT);

/* Test hooks: the narrow bottleneck (mid_block1, Residual(PreNorm(Attention)), mid_block2 over (B, mid_c, RT), mid_c 16 or 32) alone.
 *
 * dq_debug_mid_forms: what both passes decide for (B, RT), without a workspace, a launch or a device.  out receives DQ_MID_FORMS_INTS ints:
 *   qkv_fused, out_fused, pre_fused (the attention's front / back / the front's transpose ride in a ResnetBlock's launch), wide_mid, mid_c,
 *   cond_dim, prep_ok (the prepare launch fills the aligned weight slots), the offsets of mid_block1's and mid_block2's [scale | shift] in a
 *   sample's ss vector, ss_total (that vector's length).  Returns the number of ints written, or -1 (null argument, B or RT < 1, cap too small).
 *
 * dq_debug_mid_fwd: the caller has laid out the workspace (dq_unet_workspace_bytes) and written mid_in (B, mid_c, RT) and ms1f (B, cond_dim, RT)
 * -- with skip_ms1, also the rotated kk (B, 128, RT) -- at their dq_debug_tensor_offset.  Runs the time embedding for t (B int64 on the
 * device; fills every scale / shift head), unless skip_ms1 the once-per-parameter-state launches (a skip_ms1 call follows a call without it
 * on the same workspace and parameters, as a sampling step follows the prologue), then the bottleneck: mid1, xn, qv, kk, o, lse, attn_out,
 * mid2 and, with save_for_bwd, the blocks' u1 / a1 / u2 are in the workspace afterwards.  Refuses a wide bottleneck, a short workspace and
 * null arguments before any device call.
 *
 * dq_debug_mid_bwd: behind a dq_debug_mid_fwd with save_for_bwd on the same training workspace, the caller has written d mid2.out into the
 * twin of "mid2" (the twin starts dq_debug_tensor_offset(plan, "@twin") floats behind the workspace).  The rest of the twin's
 * accumulated-into region is cleared, then the bottleneck's backward runs as it does inside dq_unet_bwd: grad_x_mode 0 with the side queue,
 * 1 with everything on `stream`, as when the caller asked for d loss / d x.  Everything is joined onto `stream` at return.  Neither the
 * time-embedding backward nor the MS1 path's runs: the twins of mid_in, ms1f and o hold their gradients, the twin of "ss" the two blocks'
 * per-sample d(scale, shift), and grads (the flat layout) has received += of mid_block1.*, mid_block2.* (but mlp.*) and mid_attn.*. */
enum { DQ_MID_FORMS_INTS = 10 };
int dq_debug_mid_forms(dq_plan* plan, int B, int RT, int32_t* out, int cap);
int dq_debug_mid_fwd(dq_plan* plan, const float* params, const float* rope_freqs, const int64_t* t, int save_for_bwd, int skip_ms1,
                     void* workspace, int64_t workspace_bytes, int B, int RT, void* stream);
int dq_debug_mid_bwd(dq_plan* plan, const float* params, const float* rope_freqs, float* grads, int grad_x_mode, void* workspace,
                     int64_t workspace_bytes, int B, int RT, void* stream);

/* Test hooks: the wide bottleneck (Plan::wide_mid, every mid_c but 16 and 32) alone: mid_forward_wide / mid_backward_wide as the passes call
 * them, inside the scaffolding of dq_debug_mid_fwd / dq_debug_mid_bwd (time embedding, arena, the backward's queues, the clearing of the twin).
 *
 * dq_debug_wide_mid_fwd: the caller has written the last down level's output (B * RT, mid_c / mid_n, mid_n) into "down{L-1}" and ms1f
 * (B, cond_dim, RT) into "ms1f".  Afterwards "mid_back" (B * RT, mid_c / mid_n, mid_n) holds the bottleneck's output, every wide slot its
 * tensor (pads zero), "qv", "kk", "o", "lse" the attention's.
 *
 * dq_debug_wide_mid_bwd: behind it on the same training workspace, the caller has written d mid_back into the twin of "mid_back".
 * grad_x_mode 0: with the side queue, 1: everything on `stream`.  The twins of "down{L-1}", "ms1f", "ss" and of every wide slot hold their
 * gradients; grads has received += of mid_block1.*, mid_block2.* (but mlp.*) and mid_attn.*.
 *
 * Both refuse a narrow bottleneck, a short workspace, null arguments and B or RT < 1 before any device call. */
int dq_debug_wide_mid_fwd(dq_plan* plan, const float* params, const float* rope_freqs, const int64_t* t, int save_for_bwd, void* workspace,
                          int64_t workspace_bytes, int B, int RT, void* stream);
int dq_debug_wide_mid_bwd(dq_plan* plan, const float* params, const float* rope_freqs, float* grads, int grad_x_mode, void* workspace,
                          int64_t workspace_bytes, int B, int RT, void* stream);

/* Test hooks: the time embedding alone (k_time.hip), through the two launchers every pass calls first and last, on caller buffers.  Both
 * upload the plan's head-offset tables on first use, as the first pass on a plan does; neither needs a workspace.
 *
 * tbuf: B x DQ_TBUF_FLOATS floats, per sample the slots DQ_TBUF_* below (16 floats each but the `dim` sinusoidal features).  ss: B x ss_total
 * (dq_debug_mid_forms), row r of a sample = the r-th SiLU -> Linear(16, .) output in the plan's parameter order.
 *
 * dq_debug_time_fwd: the timestep of sample b is t[b] (B int64 on the device), or with t = NULL step_tab[*step_ptr] (both on the device, as
 * a captured sampling graph reads it), or with both NULL t_scalar.  Fills the forward slots of tbuf and, unless ss = NULL, every head row.
 *
 * dq_debug_time_bwd: behind it, from dss (B x ss_total): tbuf gains d temb and d h_pre; grads (the flat layout) receives += of every head's
 * weight and bias and of time_mlp.{1,3}.*. */
enum { DQ_TBUF_FLOATS = 100, DQ_TBUF_SINU = 0, DQ_TBUF_H_PRE = 4, DQ_TBUF_H_ACT = 20, DQ_TBUF_TEMB = 36, DQ_TBUF_SILU = 52, DQ_TBUF_DTEMB = 68,
       DQ_TBUF_DH_PRE = 84 };
int dq_debug_time_fwd(dq_plan* plan, const float* params, const int64_t* t, int t_scalar, const int* step_tab, const int* step_ptr, float* tbuf,
                      float* ss, int B, void* stream);
int dq_debug_time_bwd(dq_plan* plan, const float* params, float* grads, float* tbuf, const float* dss, int B, void* stream);

/* Test hook: which launch takes each U-Net level in a pass over (B, RT) windows -- the plan unet_forward / unet_backward / the sampler's
 * prologue build for themselves (the same rules, evaluated by the same function), without a workspace, a launch or a device.
 * save: the pass keeps what a backward needs (training forward, and the backward itself); twin: it has the gradient arena at hand
 * (dq_train_step: 1, 1; dq_unet_fwd with training: 1, 1; inference and dq_ddim_sample: 0, 0).  out receives
 *   out[0]                          L, the number of levels;
 *   DQ_LEVEL_PLAN_FORM_INTS ints    per launch, for the down levels 0 .. L-1, then the up levels 0 .. L-1, then the final ResnetBlock:
 *                                   kind (DQ_LEVEL_*), img (operand-image slot or -1), la, post_w, in_folded (the n = 1 extras of a
 *                                   DQ_LEVEL_TINY launch), resample (0: the level's resample conv is not launched -- it is the input
 *                                   stage of the next launch, or post_w);
 *   DQ_LEVEL_PLAN_FLAG_INTS ints    prep_ok, init_fused, head_shape, head_train, use_tb_up, use_tb_dn, tb_up_w.
 * Returns the number of ints written, or -1 (null argument, B or RT < 1, cap too small: 1 + 6 (2 L + 1) + 7 <= 134 ints). */
enum { DQ_LEVEL_UNFUSED = 0, DQ_LEVEL_KERNEL = 1, DQ_LEVEL_TINY = 2 };
enum { DQ_LEVEL_PLAN_FORM_INTS = 6, DQ_LEVEL_PLAN_FLAG_INTS = 7 };
int dq_debug_level_plan(dq_plan* plan, int B, int RT, int save, int twin, int32_t* out, int cap);

/* Test hook: from now on the backward's side stream ends with a store of `value` to `addr`, delayed by delay_us microseconds, right in
 * front of the join with the caller's stream (addr = NULL switches it off).  A launch the caller makes on its own stream after
 * dq_train_step / dq_unet_bwd returned -- the flat gradient all-reduce of data-parallel training -- must see the value: that is the
 * ordering the all-reduce relies on (tests/test_dp_gloo.py). */
int dq_debug_side_tail_store(dq_plan* plan, float* addr, float value, int delay_us);

#ifdef __cplusplus
}
#endif
#endif /* DQ_HIP_H */
