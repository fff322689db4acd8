// The stand-alone op entry points of the C ABI (include/dq_hip.h): single kernels and single ops -- LinearAttention, convs, ResnetBlock, a level's
// forward, the bottleneck attention -- for the per-op tests and benchmarks.  They call the op wrappers of dq_ops.hip and know nothing of the
// walk (dq_unet.hip).
#include "dq_ops.h"
#include "../../include/dq_hip.h"

using namespace dq;

extern "C" {

int dq_linattn_fwd(const float* x, float* y, float* ypre, const float* w_qkv, const float* w_out, const float* b_out,
                   const float* g_pre, const float* g_out, int C, int rows, int n, void* stream) {
  LinAttn a;
  a.x = x; a.y = y; a.ypre = ypre; a.w_qkv = w_qkv; a.w_out = w_out; a.b_out = b_out; a.g_pre = g_pre; a.g_out = g_out; a.C = C; a.rows = rows; a.n = n;
  return launch_linattn_fwd(a, (hipStream_t)stream);
}

int64_t dq_linattn_prep_floats(void) { return LA_PREP_FLOATS; }
int dq_linattn_prepare(const float* w_qkv, const float* w_out, const float* g_pre, int C, float* prep, void* stream) {
  DQ_REQUIRE(w_qkv && w_out && g_pre && prep && ((uintptr_t)prep & 15) == 0, "dq_linattn_prepare: null or unaligned argument (prep: 16-byte aligned)");
  const LaPrepItem it{w_qkv, w_out, C, prep, g_pre};
  return launch_linattn_prepare(&it, 1, (hipStream_t)stream);
}
int dq_linattn_fwd_prepared(const float* x, float* y, float* ypre, const float* w_qkv, const float* w_out, const float* b_out,
                            const float* g_pre, const float* g_out, const float* prep, int C, int rows, int n, void* stream) {
  DQ_REQUIRE(prep && ((uintptr_t)prep & 15) == 0 && la_short_row(n), "dq_linattn_fwd_prepared: prepared weights are used by rows of 1 .. 64 positions (powers of two)");
  LinAttn a;
  a.x = x; a.y = y; a.ypre = ypre; a.w_qkv = w_qkv; a.w_out = w_out; a.b_out = b_out; a.g_pre = g_pre; a.g_out = g_out; a.C = C; a.rows = rows; a.n = n;
  a.prep = prep;
  return launch_linattn_fwd(a, (hipStream_t)stream);
}

static_assert(LA_FWD_LONG == DQ_LA_FWD_LONG && LA_FWD_SMALL == DQ_LA_FWD_SMALL && LA_FWD_ROWS == DQ_LA_FWD_ROWS && LA_FWD_REG == DQ_LA_FWD_REG,
              "LaFwdForm mirrors include/dq_hip.h");
static_assert(LA_BWD_LONG == DQ_LA_BWD_LONG && LA_BWD_ROWS == DQ_LA_BWD_ROWS && LA_BWD_REG == DQ_LA_BWD_REG, "LaBwdForm mirrors include/dq_hip.h");
int dq_linattn_forms(int C, int rows, int n, int prepared, int* fwd_form, int* bwd_form) {
  DQ_REQUIRE(fwd_form && bwd_form && (C == 4 || C == 8 || C == 12 || C == 16) && rows >= 0 && n > 0,
             "dq_linattn_forms: null argument / unsupported channel count / bad shape");
  DQ_REQUIRE(!prepared || la_short_row(n), "dq_linattn_forms: prepared weights are used by rows of 1 .. 64 positions (powers of two)");
  // the caller's tensors and the prepared weights as stand-ins: the operands dq_linattn_fwd / dq_linattn_fwd_prepared / dq_linattn_bwd hand
  // over (the backward prepares the weights itself for short rows)
  float* const base = STAND_IN;
  LinAttn f;
  f.x = f.y = f.ypre = base; f.w_qkv = f.w_out = f.b_out = f.g_pre = f.g_out = base; f.C = C; f.rows = rows; f.n = n;
  f.prep = prepared ? base : nullptr;
  *fwd_form = la_fwd_form(f);
  LinAttnBwd b;
  b.f = f;
  b.f.prep = la_short_row(n) ? base : nullptr;
  b.ypre = b.dy = b.dyp = b.dxh = b.dx = base;
  *bwd_form = la_bwd_form(b);
  return 0;
}

static int linattn_bwd(const float* x, const float* ypre, const float* dy, float* dx, const float* w_qkv, const float* w_out,
                       const float* b_out, const float* g_pre, const float* g_out, float* dw_qkv, float* dw_out, float* db_out,
                       float* dg_pre, float* dg_out, float* scratch, int C, int rows, int n, int dx_store, hipStream_t s) {
  LinAttnBwd a;
  a.f.x = x; a.f.w_qkv = w_qkv; a.f.w_out = w_out; a.f.b_out = b_out; a.f.g_pre = g_pre; a.f.g_out = g_out; a.f.C = C; a.f.rows = rows;
  a.f.n = n;
  a.ypre = ypre; a.dyp = scratch; a.dxh = scratch + (int64_t)rows * C * n;
  a.part = scratch + 2 * (int64_t)rows * C * n; a.part_floats = (int64_t)LA_MAX_WAVES * 512 * C;
  a.dy = dy; a.dx = dx; a.dw_qkv = dw_qkv; a.dw_out = dw_out; a.db_out = db_out; a.dg_pre = dg_pre; a.dg_out = dg_out;
  a.dx_store = dx_store;
  if (la_short_row(n) && C % 4 == 0 && C <= 16) {
    // the prepared weights of the network path (W2, the bounded-logit flag: k_linattn_prepare), so that this entry point runs the very
    // kernel code a train step runs: carved from the tail of the slot scratch, of which short rows use a few per cent
    constexpr int64_t PREP = (LA_PREP_FLOATS + 63) / 64 * 64;
    a.part_floats -= PREP;
    float* prep = a.part + a.part_floats;
    const LaPrepItem it{w_qkv, w_out, C, prep, g_pre};
    DQ_TRY(launch_linattn_prepare(&it, 1, s));
    a.f.prep = prep;
  }
  return launch_linattn_bwd(a, s);
}
int dq_linattn_bwd(const float* x, const float* ypre, const float* dy, float* dx, const float* w_qkv, const float* w_out,
                   const float* b_out, const float* g_pre, const float* g_out, float* dw_qkv, float* dw_out, float* db_out,
                   float* dg_pre, float* dg_out, float* scratch, int C, int rows, int n, void* stream) {
  return linattn_bwd(x, ypre, dy, dx, w_qkv, w_out, b_out, g_pre, g_out, dw_qkv, dw_out, db_out, dg_pre, dg_out, scratch, C, rows, n, 0,
                     (hipStream_t)stream);
}
// dx written, not accumulated: the mode la_bwd runs the backward in inside the network
int dq_linattn_bwd_store(const float* x, const float* ypre, const float* dy, float* dx, const float* w_qkv, const float* w_out,
                         const float* b_out, const float* g_pre, const float* g_out, float* dw_qkv, float* dw_out, float* db_out,
                         float* dg_pre, float* dg_out, float* scratch, int C, int rows, int n, void* stream) {
  return linattn_bwd(x, ypre, dy, dx, w_qkv, w_out, b_out, g_pre, g_out, dw_qkv, dw_out, db_out, dg_pre, dg_out, scratch, C, rows, n, 1,
                     (hipStream_t)stream);
}

// ---- stand-alone building blocks for the per-block parity tests (tests/test_blocks_gpu.py) ---------------------------------
int dq_rmsnorm_fwd(const float* x, const float* g, float* y, int C, int rows, int n, void* stream) {
  DQ_REQUIRE(x && g && y, "dq_rmsnorm_fwd: null argument");
  return launch_rmsnorm_fwd(x, g, y, C, rows, n, (hipStream_t)stream);
}

int dq_time_mlp_fwd(const float* w1, const float* b1, const float* w2, const float* b2, const int64_t* t, float* sinu_out,
                    float* temb_out, float* scratch, int B, void* stream) {
  DQ_REQUIRE(w1 && b1 && w2 && b2 && t && scratch && B > 0, "dq_time_mlp_fwd: null argument");
  hipStream_t s = (hipStream_t)stream;
  DQ_TRY(launch_time_mlp_fwd(w1, b1, w2, b2, t, scratch, B, s));
  // per-sample scratch layout (k_time.hip): [0, 4) sinusoidal features, [36, 52) time embedding
  if (sinu_out) DQ_HIP_OK(hipMemcpy2DAsync(sinu_out, 4 * sizeof(float), scratch, TBUF_FLOATS * sizeof(float), 4 * sizeof(float), B, hipMemcpyDeviceToDevice, s));
  if (temb_out) DQ_HIP_OK(hipMemcpy2DAsync(temb_out, 16 * sizeof(float), scratch + 36, TBUF_FLOATS * sizeof(float), 16 * sizeof(float), B, hipMemcpyDeviceToDevice, s));
  return 0;
}

int dq_scale_shift_fwd(const float* temb, const float* w, const float* b, float* ss, int B, int m, void* stream) {
  DQ_REQUIRE(temb && w && b && ss, "dq_scale_shift_fwd: null argument");
  return launch_ss_heads(temb, w, b, ss, B, m, (hipStream_t)stream);
}

int dq_ms1_feat_fwd(const float* ms1, const float* w, const float* bias, float cond_mul, float cond_add, float* ms1n_out, float* u_out,
                    float* a_out, int B, int RT, int M1, void* stream) {
  Ms1FeatFwd f;
  f.ms1 = ms1; f.w = w; f.bias = bias; f.cm = cond_mul; f.ca = cond_add; f.ms1n_out = ms1n_out; f.u_out = u_out; f.a_out = a_out;
  f.B = B; f.RT = RT; f.M1 = M1;
  return launch_ms1_feat_fwd(f, (hipStream_t)stream);
}
int64_t dq_ms1_feat_wgrad_scratch_floats(int B, int RT, int M1) {
  if (B <= 0 || RT <= 0 || M1 < 1 || M1 > MS1_MAX_CHANNELS) return -1;
  return ms1_feat_wgrad_part_floats(B, RT, M1);
}
int dq_ms1_feat_wgrad(const float* ms1n, const float* du, float* dw, float* dbias, float* scratch, int64_t scratch_floats, int B, int RT,
                      int M1, void* stream) {
  Ms1FeatWgrad g;
  g.ms1n = ms1n; g.du = du; g.dw = dw; g.dbias = dbias; g.part = scratch; g.part_floats = scratch_floats; g.B = B; g.RT = RT; g.M1 = M1;
  return launch_ms1_feat_wgrad(g, (hipStream_t)stream);
}

int dq_prep_inputs_fwd(const float* x, const float* cond, const float* ms1, const float* ss, float cond_mul, float cond_add, float* cat0,
                       float* ms1n, int B, int RT, int MZ, void* stream) {
  DQ_REQUIRE(x && cond && ms1 && ss && cat0 && ms1n, "dq_prep_inputs_fwd: null argument");
  return launch_prep_inputs(x, cond, ms1, ss, 2, 0, cond_mul, cond_add, cat0, ms1n, B, RT, MZ, (hipStream_t)stream);
}

// the partial-sum slot of launch_prep_inputs_bwd: [dscale, dshift] per block, at most 32 blocks per sample
int64_t dq_prep_inputs_bwd_scratch_floats(int B, int RT, int MZ) {
  if (B <= 0 || RT <= 0 || MZ <= 0) return -1;
  return (int64_t)B * 2 * std::max(1, std::min(32, cdiv((int64_t)RT * MZ, 1024)));
}
int dq_prep_inputs_bwd(const float* dcat0, const float* cond, float cond_mul, float cond_add, float* dss, int ss_stride, int ss_off, int B,
                       int RT, int MZ, float* scratch, int64_t scratch_floats, void* stream) {
  DQ_REQUIRE(dcat0 && cond && dss && scratch, "dq_prep_inputs_bwd: null argument");
  DQ_REQUIRE(B > 0 && RT > 0 && MZ > 0, "dq_prep_inputs_bwd: B, RT and MZ must be positive");
  DQ_REQUIRE(ss_off >= 0 && ss_stride >= ss_off + 2, "dq_prep_inputs_bwd: a sample's [scale, shift] lies inside its stride: ss_stride >= ss_off + 2");
  return launch_prep_inputs_bwd(dcat0, cond, cond_mul, cond_add, dss, ss_stride, ss_off, B, RT, MZ, scratch, scratch_floats, (hipStream_t)stream);
}

int dq_conv_fwd(const float* x, const float* w, const float* bias, const float* norm_g, int act, float* y, int cout, int cin, int K, int mode,
                int rows, int n_in, int n_out, void* stream) {
  DQ_REQUIRE(x && w && y && rows > 0 && n_in > 0 && n_out > 0, "dq_conv_fwd: null argument");
  DQ_REQUIRE(mode == CONV_S1 || mode == CONV_DOWN || mode == CONV_UP, "dq_conv_fwd: mode must be 0 (stride 1), 1 (down) or 2 (up)");
  DQ_REQUIRE(act == ACT_NONE || act == ACT_SILU || act == ACT_GELU, "dq_conv_fwd: act must be 0 (none), 1 (SiLU) or 2 (GELU)");
  ConvFwd f;
  f.inA = x; f.cinA = cin; f.w = w; f.bias = bias; f.cout = cout; f.K = K; f.mode = mode; f.rows = rows; f.n_in = n_in; f.n_out = n_out;
  f.y_out = y; f.g = norm_g; f.act = act;
  return launch_conv_fwd(f, (hipStream_t)stream);
}

namespace {
// the stand-alone conv backward: the operands of dq_conv_bwd as the network's own dispatch takes them.  Workspace: [weight-gradient partial
// blocks | k_conv_bwd_wg's slots (where the shape admits that kernel)]
int conv_bwd_standalone(ConvBwdOps& o, const float* xA, int cinA, const float* xB, int cinB, const float* w, const float* dy, float* dxA,
                        float* dxB, float* dparams, int has_bias, int cout, int K, int mode, int rows, int n_in, int n_out, int rows_per_sample,
                        int accumulate, float* workspace, int64_t* workspace_floats) {
  DQ_REQUIRE(cout > 0 && cinA > 0 && cinB >= 0 && rows > 0 && n_in > 0 && n_out > 0 && rows_per_sample > 0 && rows % rows_per_sample == 0,
             "dq_conv_bwd: bad shape");
  DQ_REQUIRE((mode == CONV_S1 && (K == 1 || K == 3 || K == 7) && n_in == n_out) || (mode == CONV_DOWN && K == 4 && n_in == 2 * n_out) ||
             (mode == CONV_UP && K == 3 && n_out == 2 * n_in), "dq_conv_bwd: (mode, K, n_in, n_out) must be stride 1 (K 1 / 3 / 7, n_out = n_in), down (K 4, n_in = 2 n_out) or up (K 3, n_out = 2 n_in)");
  const int cin = cinA + cinB;
  const int64_t nelem_w = (int64_t)cout * cin * K;
  o.w = w; o.w_gemm = ((uintptr_t)w & 15) == 0 ? w : nullptr;
  o.dw = dparams; o.dbias = has_bias ? dparams + nelem_w : nullptr;
  o.inA = xA; o.inB = cinB ? xB : nullptr; o.cinA = cinA; o.cinB = cinB; o.dinA = dxA; o.dinB = cinB ? dxB : nullptr; o.accumulate = accumulate != 0;
  o.dout = dy; o.cout = cout; o.K = K; o.mode = mode; o.rows = rows; o.n_in = n_in; o.n_out = n_out; o.rows_per_sample = rows_per_sample;
  o.wg_floats = ((int64_t)WGRAD_MAX_PARTS * (nelem_w + cout) + 63) / 64 * 64;
  o.wg = workspace;
  const int pre = conv_level_pre(mode, K);
  if (pre >= 0 && cinB == 0 && conv_wg_usable(cout, pre, cinA, n_out, rows_per_sample)) {
    o.cpart_floats = conv_wg_part_floats(cout, pre, cinA, rows / rows_per_sample, rows_per_sample, n_out);
    o.cpart = workspace + o.wg_floats;
  }
  *workspace_floats = o.wg_floats + o.cpart_floats;
  return 0;
}
}  // namespace

int64_t dq_conv_bwd_workspace_floats(int cout, int cinA, int cinB, int K, int mode, int rows, int n_in, int n_out, int rows_per_sample) {
  ConvBwdOps o;
  int64_t need = 0;
  if (conv_bwd_standalone(o, nullptr, cinA, nullptr, cinB, nullptr, nullptr, nullptr, nullptr, nullptr, 1, cout, K, mode, rows, n_in, n_out,
                          rows_per_sample, 0, nullptr, &need)) return -1;
  return need;
}

static_assert(CONV_BWD_DATA_WG == DQ_CONV_BWD_DATA_WG && CONV_BWD_DATA_GEMM == DQ_CONV_BWD_DATA_GEMM && CONV_BWD_DATA_PLAIN == DQ_CONV_BWD_DATA_PLAIN &&
              CONV_WGRAD_WG == DQ_CONV_WGRAD_WG && CONV_WGRAD_V4 == DQ_CONV_WGRAD_V4 && CONV_WGRAD_SCALAR == DQ_CONV_WGRAD_SCALAR,
              "ConvBwdDataForm / ConvWgradForm mirror include/dq_hip.h");
int dq_conv_bwd_forms(int cout, int cinA, int cinB, int K, int mode, int rows, int n_in, int n_out, int rows_per_sample, int has_bias,
                      int w_aligned, int* data_form, int* wgrad_form) {
  DQ_REQUIRE(data_form && wgrad_form, "dq_conv_bwd_forms: null argument");
  // the caller's tensors and the workspace as stand-ins, the weight one float off when !w_aligned
  float* const base = STAND_IN;
  ConvBwdOps o;
  int64_t need = 0;
  DQ_TRY(conv_bwd_standalone(o, base, cinA, base, cinB, base + (w_aligned ? 0 : 1), base, base, base, base, has_bias, cout, K, mode, rows, n_in,
                             n_out, rows_per_sample, 0, base, &need));
  conv_bwd_forms(o, data_form, wgrad_form);
  return 0;
}

int dq_conv_bwd(const float* xA, int cinA, const float* xB, int cinB, const float* w, const float* dy, float* dxA, float* dxB, float* dparams,
                int has_bias, int cout, int K, int mode, int rows, int n_in, int n_out, int rows_per_sample, int accumulate, float* workspace,
                int64_t workspace_floats, void* stream) {
  DQ_REQUIRE(xA && (cinB == 0 || xB) && w && dy && dparams && workspace, "dq_conv_bwd: null argument");
  DQ_REQUIRE(((uintptr_t)workspace & 15) == 0, "dq_conv_bwd: the workspace must be 16-byte aligned");
  ConvBwdOps o;
  int64_t need = 0;
  DQ_TRY(conv_bwd_standalone(o, xA, cinA, xB, cinB, w, dy, dxA, dxB, dparams, has_bias, cout, K, mode, rows, n_in, n_out, rows_per_sample,
                             accumulate, workspace, &need));
  DQ_REQUIRE(workspace_floats >= need, "dq_conv_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int pre = conv_level_pre(mode, K);
  return pre >= 0 ? resample_bwd(o, pre, s) : conv_plain_bwd(o, s);  // (everything on s: no side stream)
}

namespace {
// workspace of the stand-alone ResnetBlock calls: a forward arena and its gradient twin, laid out like the network's
struct BlockWs { Plan plan; ResP r; Arena ar; ResBuf rb; int64_t half = 0; int B = 0; };
int block_ws(BlockWs& w, int cin, int cout, int rows, int n, int rows_per_sample) {
  DQ_REQUIRE(cin > 0 && cout > 0 && rows > 0 && n > 0 && rows_per_sample > 0 && rows % rows_per_sample == 0, "dq_resblock: bad shape");
  build_resblock_plan(w.plan, w.r, cin, cout);
  w.B = rows / rows_per_sample;
  int64_t off = 0;
  auto take = [&](int64_t f) { int64_t o = off; off += (f + 63) / 64 * 64; return o; };
  w.ar.ss = take((int64_t)w.B * w.plan.ss_total);
  w.rb = layout_res(w.B, rows_per_sample, cin, cout, n, take, take);
  w.ar.wg_floats = (int64_t)WGRAD_MAX_PARTS * ((int64_t)cout * std::max(cin, cout) * 3 + cout) * 3;
  w.ar.wg = take(w.ar.wg_floats);
  w.ar.B = w.B; w.ar.RT = rows_per_sample;
  w.half = off;
  return 0;
}
}  // namespace

int64_t dq_resblock_workspace_floats(int cin, int cout, int rows, int n, int rows_per_sample) {
  BlockWs w;
  if (block_ws(w, cin, cout, rows, n, rows_per_sample)) return -1;
  return 2 * w.half;
}

int64_t dq_resblock_dout_offset(int cin, int cout, int rows, int n, int rows_per_sample) {
  BlockWs w;
  if (block_ws(w, cin, cout, rows, n, rows_per_sample)) return -1;
  return w.half + w.rb.out;
}

int dq_resblock_fwd(const float* params, const float* xA, int cinA, const float* xB, int cinB, const float* temb, float* out, int cout,
                    int rows, int n, int rows_per_sample, int save_for_bwd, float* workspace, int64_t workspace_floats, void* stream) {
  DQ_REQUIRE(params && xA && temb && out && workspace, "dq_resblock_fwd: null argument");
  BlockWs w;
  DQ_TRY(block_ws(w, cinA + cinB, cout, rows, n, rows_per_sample));
  DQ_REQUIRE(workspace_floats >= 2 * w.half, "dq_resblock_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Ctx c{w.plan, w.ar, params, workspace, workspace + w.half, nullptr, w.B, rows_per_sample, s};
  c.save = save_for_bwd != 0;
  DQ_TRY(launch_ss_heads(temb, params + w.r.mlp_w, params + w.r.mlp_b, c.w(w.ar.ss), w.B, 2 * cout, s));  // unet1d.py:315-318
  DQ_TRY(res_fwd(c, w.r, w.rb, xA, cinA, cinB ? xB : nullptr, cinB, rows, n, rows_per_sample));
  return launch_copy(out, c.w(w.rb.out), (int64_t)rows * cout * n, s);
}

static_assert(RES_FWD_RT == DQ_RES_FWD_RT && RES_FWD_LEVEL == DQ_RES_FWD_LEVEL && RES_FWD_V4 == DQ_RES_FWD_V4 && RES_FWD_UNFUSED == DQ_RES_FWD_UNFUSED,
              "ResFwdForm mirrors include/dq_hip.h");
static_assert(RES_BWD_WG == DQ_RES_BWD_WG && RES_BWD_RT == DQ_RES_BWD_RT && RES_BWD_ROWS == DQ_RES_BWD_ROWS && RES_BWD_CP == DQ_RES_BWD_CP &&
              RES_BWD_PLAIN == DQ_RES_BWD_PLAIN && RES_BWD_UNFUSED == DQ_RES_BWD_UNFUSED, "ResBwdForm mirrors include/dq_hip.h");
int dq_resblock_forms(int cinA, int cinB, int cout, int rows, int n, int rows_per_sample, int* fwd_form, int* bwd_form) {
  DQ_REQUIRE(fwd_form && bwd_form && cinA > 0 && cinB >= 0, "dq_resblock_forms: null argument / bad channel split");
  BlockWs w;
  DQ_TRY(block_ws(w, cinA + cinB, cout, rows, n, rows_per_sample));
  *fwd_form = res_fwd_form(cout, cinA, cinB, w.r.res.cout != 0, rows, n, rows_per_sample);
  // the caller's tensors and the workspace as stand-ins: the operands dq_resblock_bwd hands over
  float* const base = STAND_IN;
  Ctx c{w.plan, w.ar, base, base, base + w.half, base, w.B, rows_per_sample, nullptr};
  const ResBwd k = res_bwd_args(c, w.r, w.rb, base, cinA, cinB ? base : nullptr, cinB, rows, n, rows_per_sample, 0, 0);
  *bwd_form = res_bwd_form(k, w.rb.wpart_floats != 0);
  return 0;
}

int dq_resblock_bwd(const float* params, const float* xA, int cinA, const float* xB, int cinB, const float* dout, float* dxA, float* dxB,
                    float* grads, float* dss, int cout, int rows, int n, int rows_per_sample, float* workspace, int64_t workspace_floats,
                    void* stream) {
  DQ_REQUIRE(params && xA && grads && workspace, "dq_resblock_bwd: null argument");
  BlockWs w;
  DQ_TRY(block_ws(w, cinA + cinB, cout, rows, n, rows_per_sample));
  DQ_REQUIRE(workspace_floats >= 2 * w.half, "dq_resblock_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Ctx c{w.plan, w.ar, params, workspace, workspace + w.half, grads, w.B, rows_per_sample, s};  // no side stream: everything on s
  // dout == NULL: the gradient of the block output is already in the workspace (at dq_resblock_dout_offset floats; a benchmark fills it
  // once), dxA / dxB are plain stores and dss (nullable) is not copied out: the call is then the backward launches and nothing else
  const int first_writer = dout ? 0 : 1;
  if (dout) {
    DQ_TRY(launch_zero(c.g(w.ar.ss), (int64_t)w.B * w.plan.ss_total, s));
    DQ_TRY(launch_copy(c.g(w.rb.out), dout, (int64_t)rows * cout * n, s));
  }
  DQ_TRY(res_bwd(c, w.r, w.rb, xA, dxA, cinA, cinB ? xB : nullptr, cinB ? dxB : nullptr, cinB, rows, n, rows_per_sample, first_writer, first_writer));
  if (!dout || !dss) return 0;
  return launch_copy(dss, c.g(w.ar.ss), (int64_t)w.B * w.plan.ss_total, s);
}

// ---- stand-alone level forward (tests, bench): y = ResnetBlock_1(cat(ResnetBlock_0(cat(stage(x), skip0)), skip1)) in ONE launch -------
// params: [stage conv weight (C, cp, K) | bias (C)] (pre != 0) followed by the two blocks, each laid out as dq_resblock_* expects
// (cin = C + cs).  workspace: 2 * B * (4 C) floats (the blocks' scale / shift vectors).
int64_t dq_level_param_floats(int pre, int C, int cp, int cs, int nblocks) {
  const int K = pre == LEVEL_PRE_DOWN ? 4 : 3;
  Plan p; ResP r;
  build_resblock_plan(p, r, C + cs, C);
  return (pre ? (int64_t)C * cp * K + C : 0) + (int64_t)nblocks * p.total_floats;
}
int dq_level_fwd(const float* params, int pre, const float* x, int cp, const float* skip0, const float* skip1, int cs, const float* temb,
                 float* out0, float* out1, int C, int nblocks, int rows, int n, int rows_per_sample, float* workspace,
                 int64_t workspace_floats, void* stream) {
  DQ_REQUIRE(params && x && temb && workspace && (nblocks == 1 || nblocks == 2) && (nblocks == 1 ? out0 != nullptr : out1 != nullptr),
             "dq_level_fwd: null argument");
  DQ_REQUIRE(rows > 0 && rows_per_sample > 0 && rows % rows_per_sample == 0, "dq_level_fwd: bad rows");
  const int B = rows / rows_per_sample, K = pre == LEVEL_PRE_DOWN ? 4 : 3;
  Plan p; ResP r;
  build_resblock_plan(p, r, C + cs, C);
  DQ_REQUIRE(workspace_floats >= (int64_t)2 * B * p.ss_total, "dq_level_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const float* blk0 = params + (pre ? (int64_t)C * cp * K + C : 0);
  LevelFwd f;
  f.params = params; f.in = x; f.pre = pre; f.nblocks = nblocks; f.C = C; f.rows = rows; f.n = n; f.rows_per_sample = rows_per_sample;
  if (pre) { f.cp = cp; f.pw = params; f.pb = params + (int64_t)C * cp * K; }
  for (int i = 0; i < nblocks; ++i) {
    const float* bp = blk0 + (int64_t)i * p.total_floats;
    float* ss = workspace + (int64_t)i * p.ss_total;  // [b][2 blocks][2 C]: stride 2 * ss_total
    ResFwd k;  // (parameters of a bare buffer, scale / shift at a stride of its own: not res_operands, which reads a Ctx)
    k.inB = cs ? (i == 0 ? skip0 : skip1) : nullptr; k.cinB = cs;
    k.w1 = bp + r.c1.w; k.b1 = bp + r.c1.b; k.g1 = bp + r.g1; k.w2 = bp + r.c2.w; k.b2 = bp + r.c2.b; k.g2 = bp + r.g2;
    if (r.res.cout) { k.wr = bp + r.res.w; k.br = bp + r.res.b; }
    k.ss = ss; k.ss_stride = 2 * p.ss_total;
    k.out = i == 0 ? out0 : out1;
    f.blk[i] = k;
    DQ_TRY(launch_ss_heads_strided(temb, bp + r.mlp_w, bp + r.mlp_b, ss, 2 * p.ss_total, B, 2 * C, s));  // unet1d.py:315-318
  }
  // a workspace with room for the operand image behind the scale / shift vectors: built by its own launch first, as the network path does
  const int64_t img_at = ((int64_t)2 * B * p.ss_total + 63) / 64 * 64;
  if (((uintptr_t)workspace & 15) == 0 && workspace_floats >= img_at + level_img_floats(f) && level_fwd_usable(f)) {
    f.img = workspace + img_at;
    DQ_TRY(launch_level_images(&f, 1, s));
  }
  return launch_level_fwd(f, s);
}

int dq_rope(float* qk, const float* freqs, int B, int64_t batch_stride, int RT, float sign, void* stream) {
  DQ_REQUIRE(qk && freqs, "dq_rope: null argument");
  return launch_rope(qk, freqs, B, batch_stride, RT, sign, (hipStream_t)stream);
}

int dq_attn_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int RT, void* stream) {
  DQ_REQUIRE(q && k && v && o && lse, "dq_attn_fwd: null argument");
  const int64_t bs = (int64_t)HID * RT;
  return launch_attn_fwd(q, bs, k, bs, v, bs, o, lse, B, RT, (hipStream_t)stream);
}

int dq_attn_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o, const float* lse, float* delta,
                float* dq_, float* dk, float* dv, int B, int RT, void* stream) {
  DQ_REQUIRE(q && k && v && o && d_o && lse && delta && dq_ && dk && dv, "dq_attn_bwd: null argument");
  const int64_t bs = (int64_t)HID * RT;
  return launch_attn_bwd(q, bs, k, bs, v, bs, o, d_o, lse, delta, dq_, bs, dk, bs, dv, bs, B, RT, (hipStream_t)stream);
}

// ---- the wide bottleneck's kernels (k_wide.hip) alone, for tests/test_wide_mid.py: the launchers wide_res_fwd / wide_res_bwd / mid_*_wide call,
// on caller tensors (B, C, P).  Every entry checks its arguments before it launches.
namespace {
bool wide_shape_ok(int B, int C, int RT, int P) { return B > 0 && C > 0 && RT > 0 && P >= RT && P < RT + 4 && P % 4 == 0; }
}  // namespace

int dq_wide_im2col3(const float* x, float* xcol, int B, int C, int RT, int P, void* stream) {
  DQ_REQUIRE(x && xcol, "dq_wide_im2col3: null argument");
  DQ_REQUIRE(wide_shape_ok(B, C, RT, P), "dq_wide_im2col3: B, C, RT positive, P the multiple of 4 in [RT, RT + 4)");
  return launch_im2col3(x, xcol, B, C, RT, P, (hipStream_t)stream);
}
int dq_wide_col2im3(const float* dxcol, float* dx, int B, int C, int RT, int P, int accumulate, void* stream) {
  DQ_REQUIRE(dxcol && dx, "dq_wide_col2im3: null argument");
  DQ_REQUIRE(wide_shape_ok(B, C, RT, P), "dq_wide_col2im3: B, C, RT positive, P the multiple of 4 in [RT, RT + 4)");
  return launch_col2im3(dxcol, dx, B, C, RT, P, accumulate != 0, (hipStream_t)stream);
}
int dq_wide_repitch(float* dst, int dpitch, const float* src, int spitch, int64_t rows, int n, void* stream) {
  DQ_REQUIRE(dst && src, "dq_wide_repitch: null argument");
  DQ_REQUIRE(rows > 0 && n > 0 && dpitch >= n && spitch >= n && dpitch < n + 4 && spitch < n + 4 && (dpitch % 4 == 0 || spitch % 4 == 0),
             "dq_wide_repitch: rows, n positive, both pitches in [n, n + 4), the padded one a multiple of 4");
  return launch_repitch(dst, dpitch, src, spitch, rows, n, (hipStream_t)stream);
}
int dq_wide_norm_fwd(const float* u, const float* g, const float* ss, int ss_stride, int act, const float* res, float* y, int B, int C, int RT,
                     int P, void* stream) {
  DQ_REQUIRE(u && g && y, "dq_wide_norm_fwd: null argument");
  DQ_REQUIRE(wide_shape_ok(B, C, RT, P), "dq_wide_norm_fwd: B, C, RT positive, P the multiple of 4 in [RT, RT + 4)");
  DQ_REQUIRE(!ss || ss_stride >= 2 * C, "dq_wide_norm_fwd: a sample's [scale | shift] is 2 C floats: ss_stride >= 2 C");
  DQ_REQUIRE(act == ACT_NONE || act == ACT_SILU, "dq_wide_norm_fwd: act must be 0 (none) or 1 (SiLU)");
  return launch_wnorm_fwd(u, g, ss, ss_stride, act, res, y, B, C, RT, P, (hipStream_t)stream);
}
int64_t dq_wide_norm_bwd_scratch_floats(int B, int C, int P) {
  if (B <= 0 || C <= 0 || P <= 0) return -1;
  return (int64_t)B * (2 * (int64_t)P + 2 * (int64_t)C);
}
int dq_wide_norm_bwd(const float* u, const float* dy, const float* g, const float* ss, int ss_stride, int act, float* du, float* dg, float* dss,
                     float* dbias, float* scratch, int64_t scratch_floats, int B, int C, int RT, int P, void* stream) {
  DQ_REQUIRE(u && dy && g && du && dg && scratch, "dq_wide_norm_bwd: null argument");
  DQ_REQUIRE(wide_shape_ok(B, C, RT, P), "dq_wide_norm_bwd: B, C, RT positive, P the multiple of 4 in [RT, RT + 4)");
  DQ_REQUIRE(!ss || dss, "dq_wide_norm_bwd: scale / shift needs a gradient buffer (dss)");
  DQ_REQUIRE(!ss || ss_stride >= 2 * C, "dq_wide_norm_bwd: a sample's [scale | shift] is 2 C floats: ss_stride >= 2 C");
  DQ_REQUIRE(act == ACT_NONE || act == ACT_SILU, "dq_wide_norm_bwd: act must be 0 (none) or 1 (SiLU)");
  DQ_REQUIRE(scratch_floats >= dq_wide_norm_bwd_scratch_floats(B, C, P), "dq_wide_norm_bwd: scratch too small");
  return launch_wnorm_bwd(u, dy, g, ss, ss_stride, act, du, dg, dss, dbias, scratch, B, C, RT, P, (hipStream_t)stream);
}
int dq_wide_rowsum(const float* x, int64_t rows, int RT, int P, float* out, void* stream) {
  DQ_REQUIRE(x && out, "dq_wide_rowsum: null argument");
  DQ_REQUIRE(rows > 0 && wide_shape_ok(1, 1, RT, P), "dq_wide_rowsum: rows, RT positive, P the multiple of 4 in [RT, RT + 4)");
  return launch_rowsum(x, rows, RT, P, out, (hipStream_t)stream);
}
int dq_wide_sum_b(const float* part, int B, int C, float* dst, void* stream) {
  DQ_REQUIRE(part && dst, "dq_wide_sum_b: null argument");
  DQ_REQUIRE(B > 0 && C > 0, "dq_wide_sum_b: B and C must be positive");
  return launch_sum_b(part, B, C, dst, (hipStream_t)stream);
}

}  // extern "C"
