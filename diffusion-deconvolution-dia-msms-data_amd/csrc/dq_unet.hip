// Host orchestration of the U-Net: the arena layout, the two bottlenecks, the level-launch plan and the two passes (what the entry points of
// dq_api.hip and dq_sampler.hip call is declared in dq_net.h), over the op wrappers and the side queue of dq_ops.hip, and the debug entry
// points of the C ABI that ask this file's private types.  Follows UNet1d.forward (dquartic/model/unet1d.py:1086-1166) op by op; the
// comments name the reference lines each stage replaces.
#include "dq_dev.h"
#include "dq_tfm.h"
#include "dq_ops.h"
#include "dq_options.h"
#include "../../include/dq_hip.h"

#include <algorithm>
#include <functional>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace dq {

// ---------------------------------------------------------------------------------------------------------------
// arena
// ---------------------------------------------------------------------------------------------------------------
void layout_arena(const Plan& p, int B, int RT, Arena& a) {
  // Two regions: [0, zero_floats) holds every tensor whose GRADIENT twin is accumulated into (+=) and therefore has to start
  // at zero each backward; the rest (pre-norm saves, whose twins are written with "=", and pure scratch) follows, so that the
  // backward clears one contiguous ~1/3 of the twin instead of all of it.  Pass 0 sizes the first region, pass 1 assigns.
  int64_t zero_total = 0;
  for (int pass = 0; pass < 2; ++pass) {
  a = Arena();
  a.B = B; a.RT = RT;
  int64_t off = 0, off_nz = zero_total;
  auto take = [&](int64_t n) { int64_t o = off; off += (n + 63) / 64 * 64; return o; };  // 256-B aligned
  auto take_nz = [&](int64_t n) { int64_t o = off_nz; off_nz += (n + 63) / 64 * 64; return o; };
  const int64_t R = (int64_t)B * RT;
  // zero_out: the gradient of the block's output is accumulated into before anything stores to it (the bottleneck blocks'
  // step-by-step backward); everywhere else the first writer of a gradient tensor stores (unet_backward), so the twin of that
  // tensor needs no clearing -- the zero-fill per backward went from 452 MB to the few small tensors that are left in `take`.
  // One gpart slot per ResnetBlock (the ordered reduce runs on the side stream and may lag behind the next block's backward).
  auto res = [&](int rows_per_sample, int cin, int c, int n, bool zero_out = false) {
    return layout_res(B, rows_per_sample, cin, c, n, take_nz, [&](int64_t f) { return zero_out ? take(f) : take_nz(f); });
  };
  // a level's buffers; pre: the stage its resample conv is for the level kernels (LEVEL_PRE_DOWN / LEVEL_PRE_UP; the k3 conv of a last level: S1)
  auto level = [&](const LevelP& l, int pre) {
    LevelBuf b;
    b.r0 = res(RT, l.r0.cin, l.r0.cout, l.n); b.r1 = res(RT, l.r1.cin, l.r1.cout, l.n);
    b.la = take_nz(R * l.la.C * l.n); b.la_pre = take_nz(R * l.la.C * l.n); b.la_tmp = take_nz(R * l.la.C * l.n);
    b.rs = take_nz(R * l.resample.cout * l.n_next);
    if (l.last) pre = LEVEL_PRE_S1;
    if (B > 0 && conv_wg_usable(l.resample.cout, pre, l.resample.cin, l.n_next, RT)) {
      b.cpart_floats = conv_wg_part_floats(l.resample.cout, pre, l.resample.cin, B, RT, l.n_next);
      b.cpart = take_nz(b.cpart_floats);
    }
    return b;
  };
  a.tbuf = take((int64_t)B * TBUF_FLOATS);
  a.ss = take((int64_t)B * p.ss_total);
  a.cat0 = take(R * 2 * p.mz);
  const int M1 = p.ms1_channels;
  // (M1 > 1: the normalised (B, RT, M1) conditioning a training forward keeps for the weight gradient -- no gradient with respect to MS1 is
  // formed, so it stays out of the region whose twin is cleared every backward; M1 = 1 keeps its place)
  a.ms1n = M1 > 1 ? take_nz(R * M1) : take(R);
  a.ms1_u = take(R * p.cond_dim); a.ms1_a = take(R * p.cond_dim); a.ms1f = take(R * p.cond_dim);
  a.h0 = take_nz(R * p.dim * p.mz);
  for (const LevelP& l : p.downs) a.downs.push_back(level(l, LEVEL_PRE_DOWN));
  if (p.wide_mid) {
    // the wide bottleneck (k_wide.hip): padded (B, C, P) tensors; every gradient twin is stored by its first writer
    const int P = (RT + 3) / 4 * 4, Cm = p.mid_c;
    a.P = P;
    const int64_t t = (int64_t)B * Cm * P;
    a.w_mid_in = take_nz(t);
    for (WideResBuf* w : {&a.wmid1, &a.wmid2}) { w->u1 = take_nz(t); w->a1 = take_nz(t); w->u2 = take_nz(t); w->out = take_nz(t); }
    a.w_xcol = take_nz(3 * t);
    a.w_xn = take_nz(t);
    a.w_qv = take_nz((int64_t)B * 2 * HID * P);
    a.w_o = take_nz((int64_t)B * HID * P);
    a.w_attn_out = take_nz(t);
    a.w_stats = take_nz((int64_t)B * (2 * P + 2 * std::max(Cm, 2 * HID)) + 64);
    int64_t gp = 0;
    const int Kw = B * ((RT + 31) / 32 * 32);  // the weight gradients reduce over all samples in one product (Gemm::kbatch: B blocks of RT, each padded to the k-tile)
    const int shapes[9][4] = {{Cm, RT, 3 * Cm, B}, {3 * Cm, RT, Cm, B}, {Cm, 3 * Cm, Kw, 1}, {2 * HID, RT, Cm, B}, {Cm, RT, 2 * HID, B},
                              {2 * HID, Cm, Kw, 1}, {Cm, RT, HID, B}, {HID, RT, Cm, B}, {Cm, HID, Kw, 1}};
    for (const auto& sh : shapes) gp = std::max(gp, gemm_partial_floats(sh[0], sh[1], sh[2], sh[3]));
    a.w_gemm_part_floats = gp;
    a.w_gemm_part = take_nz(gp + 64);
  }
  a.mid_in = take(R * (p.wide_mid ? 1 : p.mid_c));
  a.mid1 = res(1, p.wide_mid ? 4 : p.mid_c, p.wide_mid ? 4 : p.mid_c, RT, true);
  a.xn = take(R * (p.wide_mid ? 1 : p.mid_c));
  a.qv = take(R * 2 * HID); a.kk = take(R * HID); a.o = take(R * HID);
  a.lse = take(R * HEADS); a.delta = take(R * HEADS);
  a.attn_out = take(R * (p.wide_mid ? 1 : p.mid_c));
  a.mid2 = res(1, p.wide_mid ? 4 : p.mid_c, p.wide_mid ? 4 : p.mid_c, RT, true);
  a.mid_back = take(R * p.mid_c);
  for (const LevelP& l : p.ups) a.ups.push_back(level(l, LEVEL_PRE_UP));
  a.fin = res(RT, 2 * p.dim, p.dim, p.mz);
  a.eps = take(R * p.mz);
  a.xa = take_nz(R * p.mz);   // sampling ping-pong / train-step x_t
  a.xb = take_nz(R * p.mz);
  a.partials = take_nz(MSE_MAX_BLOCKS);
  a.head_part = take_nz(LEVEL_LOSS_PARTS);  // per-wave squared-error sums of the training head (k_level_fwd)
  a.loss = take_nz(64);
  a.coef = take_nz(4 * 1024);  // DDIM coefficient table (<= 1024 steps)
  // (the wide bottleneck's weight gradients are GEMMs into the gradient buffer itself: no partial sums)
  a.wg_floats = (int64_t)WGRAD_MAX_PARTS * (std::max({16 * 32 * 3, p.wide_mid ? HID * p.cond_dim : p.mid_c * p.mid_c * 3,
                                                        p.wide_mid ? 0 : 2 * HID * p.mid_c}) + 2 * HID);
  a.wg = take_nz(a.wg_floats);  // partial sums of the weight-gradient kernels
  // per-wave dW partial slots of the LinearAttention backward: one reservation per LinearAttention layer, so that all slot
  // reductions of a backward pass can be deferred into ONE launch at its end (15 launches of ~14 us on the main stream before)
  a.la_part_floats = 0;
  for (const LevelP& l : p.downs) a.la_part_floats += la_part_reserve(l.la.C);
  for (const LevelP& l : p.ups) a.la_part_floats += la_part_reserve(l.la.C);
  a.la_part_floats = std::max<int64_t>(a.la_part_floats, (int64_t)LA_MAX_WAVES * 512 * 16);
  a.la_part = take_nz(a.la_part_floats);
  a.la_prep = take_nz((int64_t)LA_PREP_MAX * LA_PREP_FLOATS);  // prepared LinearAttention weights, one slot per layer (downs, then ups)
  a.wimg = take_nz((int64_t)LEVEL_IMG_MAX * LEVEL_IMG_FLOATS);  // MFMA operand images of the level kernels' weights, one slot per launch (downs, then ups, then the head)
  a.timg = take_nz((int64_t)TINY_IMG_MAX * TINY_IMG_FLOATS);  // operand images of the tiny-level launches (k_tiny.hip)
  a.bb_part_floats = (int64_t)64 * B * 4 * std::max(p.wide_mid ? 2 : p.mid_c, 2);  // partial sums of the PreNorm backward / the input affine
  a.bb_part = take_nz(a.bb_part_floats);
  a.ms1_scratch = take_nz(5 * R + B + 64);  // the MS1 loss term (ms1_loss_weight > 0): per-row sums / maxima and their gradients
  a.wtmp = take_nz(3 * WTMP_SLOT);  // 16-byte aligned copy of a projection weight for the GEMM route of the wide 1x1 convs
  a.ts_tab = take_nz(1024); a.step = take_nz(64);  // graph replay: timestep table (int32) and the device-side step counter
  a.c2_stage = take_nz(R * p.mz); a.c1_stage = take_nz(R * M1);  // conditions staged at fixed addresses for the captured step
  if (M1 > 1 && B > 0) { a.ms1_wpart_floats = ms1_feat_wgrad_part_floats(B, RT, M1); a.ms1_wpart = take_nz(a.ms1_wpart_floats); }
  a.sigma = take_nz(1024); a.seed_stage = take_nz(64); a.ids_stage = take_nz(2 * (int64_t)B);  // stochastic sampling (256-B aligned: 8-byte words fit)
  a.zero_floats = off;
  a.floats = off_nz;
  zero_total = off;
  }  // pass
}

bool tail_fork_enabled() {
  return !DQ_DEV_FLAG("DQ_NO_TAIL_FORK", '1');  // (dev switch)
}

namespace {

// flush after every second level (measured, ms per step: every level 4.876, the three widest + every second deeper one 4.858, every
// second 4.836, every third 4.90 -- the side stream then starts too late); level 0 always flushes
static inline bool side_flush_here(int lv) { return (lv & 1) == 0; }

// The tiny backward (k_tiny.hip) of the two levels with rows of one position: `up` = the first up level (its input gradient goes straight into
// the bottleneck's layout), otherwise the last down level (with its k3 conv and the Downsample in front of it).  Image slots 4 / 5 of the
// tiny-image region.  Gradient-arena pointers are filled only when the context has one (the forward builds the images from the weights alone).
// Whether a pass takes it is LevelPlan::use_tb_up / use_tb_dn; up_w (LevelPlan::tb_up_w): the Upsample transpose rides along.
TinyBwd tiny_bwd_desc(const Ctx& c, bool up, bool up_w) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int L = p.levels;
  const LevelP& l = up ? p.ups[0] : p.downs[L - 1];
  const LevelBuf& b = up ? a.ups[0] : a.downs[L - 1];
  TinyBwd t;
  t.params = c.P; t.img = c.w(a.timg) + (int64_t)(up ? 4 : 5) * TINY_IMG_FLOATS;
  t.C = 16; t.rows = c.B * c.RT; t.rows_per_sample = c.RT;
  t.pre = up ? LEVEL_PRE_NONE : LEVEL_PRE_DOWN;
  t.cs = l.r0.cin - l.r0.cout;
  la_operands(c, l.la, t);
  t.x = c.w(b.r1.out); t.ypre = c.w(b.la_pre);
  const ResP* rp[2] = {&l.r0, &l.r1};
  const ResBuf* rb[2] = {&b.r0, &b.r1};
  for (int i = 0; i < 2; ++i) {
    TinyBwd::Blk& k = t.blk[i];
    const ResP& r = *rp[i];
    res_operands(c, r, k);
    k.u1 = c.w(rb[i]->u1); k.u2 = c.w(rb[i]->u2);
    k.gpart = c.w(rb[i]->gpart); k.gpart_floats = rb[i]->gpart_floats;
    if (c.G) { k.du1 = c.g(rb[i]->u1); k.du2 = c.g(rb[i]->u2); k.dout_st = r.res.cout ? c.g(rb[i]->out) : nullptr; }
  }
  if (up) {
    // the Upsample conv behind the level (nearest x2 + k3, 16 -> 16): its backward data path in the same launch, its weight gradient on the side stream
    if (up_w) {
      t.up_w = c.prm(l.resample.w);
      if (c.G) t.dup = c.g(b.rs);
    }
    if (c.G) {
      t.dy = c.g(b.la); t.dfold = c.g(a.mid2.out);
      t.blk[1].dB = c.g(a.downs[L - 1].r0.out); t.blk[1].dB_acc = 0;  // the up path is the first writer of the skip gradients (unet_backward)
      t.blk[0].dB = c.g(a.downs[L - 1].la); t.blk[0].dB_acc = 0;
    }
  } else {
    const LevelP& lp = p.downs[L - 2];
    t.cp = lp.resample.cin;
    t.post_w = c.prm(l.resample.w); t.stage_w = c.prm(lp.resample.w);
    if (c.G) {
      t.dy = c.g(b.la); t.dmid = c.g(a.mid_in); t.drs_out = c.g(b.rs);
      t.din_rows = c.g(a.downs[L - 2].rs); t.dprev = c.g(a.downs[L - 2].la);
      t.r0out_g = c.g(b.r0.out);
    }
  }
  return t;
}


// launches the tiny backward of one level and queues what stays on the side stream / in the deferred reductions: the LinearAttention slot
// reduce, both blocks' weight gradients + partial-sum reduces, and (down level) the weight gradients of its k3 conv and of the Downsample
int tiny_bwd_run(const Ctx& c, TinyBwd t, bool up) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int L = p.levels, R = c.B * c.RT;
  const LevelP& l = up ? p.ups[0] : p.downs[L - 1];
  const LevelBuf& b = up ? a.ups[0] : a.downs[L - 1];
  DQ_REQUIRE(c.la_defer, "tiny_bwd_run: needs the deferred LinearAttention reduction");
  const int64_t need = la_part_reserve(l.la.C);
  DQ_TRY(la_reserve(c, need, &t.la_part, &t.la_part_floats));
  int gblocks = 0;
  t.gblocks = &gblocks;
  DQ_TRY(launch_tiny_bwd(t, c.s));
  const int slots = tiny_bwd_slots(t), C = l.la.C;
  DQ_REQUIRE((int64_t)slots * la_slot(C) + 4 * C * C <= need, "tiny_bwd_run: more LinearAttention slots than a layer's reservation holds");
  la_commit(c, la_reduce_item(t.la_part, slots, C, c.dprm(l.la.qkv_w), c.dprm(l.la.out_w), c.dprm(l.la.g_out), c.dprm(l.la.out_b),
                              c.dprm(l.la.g_pre), c.prm(l.la.qkv_w), c.prm(l.la.out_w)), need);
  if (up) {
    const int cs = l.r0.cin - l.r0.cout;
    DQ_TRY(res_bwd_side(c, l.r1, b.r1, c.w(b.r0.out), l.r1.cout, c.w(a.downs[L - 1].r0.out), cs, R, l.n, c.RT, gblocks));
    DQ_TRY(res_bwd_side(c, l.r0, b.r0, c.w(a.mid_back), l.r0.cout, c.w(a.downs[L - 1].la), cs, R, l.n, c.RT, gblocks));
  } else {
    const LevelP& lp = p.downs[L - 2];
    const LevelBuf& bp = a.downs[L - 2];
    // the level's k3 conv (centre tap at one position) and the Downsample in front of the level: weight gradients from the d rs tensors
    ConvWgrad wg;
    wg.scratch = c.w(a.wg); wg.scratch_floats = a.wg_floats;
    wg.du = c.g(b.rs); wg.inA = c.w(b.la); wg.cinA = l.resample.cin; wg.cout = l.resample.cout; wg.K = l.resample.k; wg.mode = CONV_S1;
    wg.rows = R; wg.n_in = l.n; wg.n_out = l.n_next; wg.dw = c.dprm(l.resample.w); wg.dbias = l.resample.b >= 0 ? c.dprm(l.resample.b) : nullptr;
    DQ_TRY(wgrad_async(c, wg));
    DQ_TRY(res_bwd_side(c, l.r1, b.r1, c.w(b.r0.out), l.r1.cin, nullptr, 0, R, l.n, c.RT, gblocks));
    DQ_TRY(res_bwd_side(c, l.r0, b.r0, c.w(bp.rs), l.r0.cin, nullptr, 0, R, l.n, c.RT, gblocks));
    ConvWgrad wd;
    wd.scratch = c.w(a.wg); wd.scratch_floats = a.wg_floats;
    wd.du = c.g(bp.rs); wd.inA = c.w(bp.la); wd.cinA = lp.resample.cin; wd.cout = lp.resample.cout; wd.K = lp.resample.k; wd.mode = CONV_DOWN;
    wd.rows = R; wd.n_in = lp.n; wd.n_out = lp.n_next; wd.dw = c.dprm(lp.resample.w); wd.dbias = lp.resample.b >= 0 ? c.dprm(lp.resample.b) : nullptr;
    DQ_TRY(wgrad_async(c, wd));
  }
  return 0;
}


int mid_forward_wide(const Ctx& c, const float* rope, const float* cur) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int B = c.B, RT = c.RT, P = a.P, Cm = p.mid_c;
  const int64_t t = (int64_t)B * Cm * P;
  DQ_TRY(launch_fold(cur, c.w(a.w_mid_in), B, RT, Cm, 1, 0, c.s, P));
  DQ_TRY(wide_res_fwd(c, p.mid1, a.wmid1, c.w(a.w_mid_in)));
  // Residual(PreNorm(Attention(use_xattn))) (unet1d.py:552-567): q | v from the normed state, k from the MS1 features
  DQ_TRY(launch_wnorm_fwd(c.w(a.wmid1.out), c.prm(p.ag), nullptr, 0, ACT_NONE, nullptr, c.w(a.w_xn), B, Cm, RT, P, c.s));
  DQ_TRY(wide_gemm(c, c.prm(p.qv_w), 1, Cm, c.w(a.w_xn), Cm, c.w(a.w_qv), 2 * HID, 2 * HID, RT, Cm, nullptr, 0));
  DQ_TRY(launch_repitch(c.w(a.qv), RT, c.w(a.w_qv), P, (int64_t)B * 2 * HID, RT, c.s));  // the attention kernels read rows of RT floats
  DQ_TRY(conv_plain_fwd(c, proj(p.k_w, HID, p.cond_dim), CONV_S1, c.w(a.ms1f), c.w(a.kk), B, RT, RT));
  if (rope) {
    DQ_TRY(launch_rope2(c.w(a.qv), (int64_t)2 * HID * RT, c.w(a.kk), (int64_t)HID * RT, rope, B, RT, 1.f, c.s));
  }
  const int64_t qvbs = (int64_t)2 * HID * RT, kbs = (int64_t)HID * RT;
  DQ_TRY(launch_attn_fwd(c.w(a.qv), qvbs, c.w(a.kk), kbs, c.w(a.qv) + kbs, qvbs, c.w(a.o), c.w(a.lse), B, RT, c.s));
  DQ_TRY(launch_repitch(c.w(a.w_o), P, c.w(a.o), RT, (int64_t)B * HID, RT, c.s));
  DQ_TRY(launch_copy(c.w(a.w_attn_out), c.w(a.wmid1.out), t, c.s));  // the residual; attn_out += Wo o + b
  DQ_TRY(wide_gemm(c, c.prm(p.ao_w), 1, HID, c.w(a.w_o), HID, c.w(a.w_attn_out), Cm, Cm, RT, HID, c.prm(p.ao_b), 1));
  DQ_TRY(wide_res_fwd(c, p.mid2, a.wmid2, c.w(a.w_attn_out)));
  return launch_fold(c.w(a.wmid2.out), c.w(a.mid_back), B, RT, Cm, 0, 0, c.s, P);
}

// d(mid_back) is complete; leaves d(downs[L-1].rs) (plain store) and all bottleneck parameter gradients (+=)
int mid_backward_wide(const Ctx& c, const float* rope) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int B = c.B, RT = c.RT, P = a.P, Cm = p.mid_c, L = p.levels;
  const int64_t t = (int64_t)B * Cm * P;
  float* st = c.w(a.w_stats);
  DQ_TRY(launch_fold(c.g(a.mid_back), c.g(a.wmid2.out), B, RT, Cm, 1, 0, c.s, P));
  DQ_TRY(wide_res_bwd(c, p.mid2, a.wmid2, c.w(a.w_attn_out), c.g(a.w_attn_out)));
  // attn_out = mid1.out + Wo o + b
  float* dao = c.g(a.w_attn_out);
  DQ_TRY(wide_wgrad(c, dao, c.w(a.w_o), c.dprm(p.ao_w), Cm, HID));
  DQ_TRY(launch_rowsum(dao, (int64_t)B * Cm, RT, P, st, c.s));
  DQ_TRY(launch_sum_b(st, B, Cm, c.dprm(p.ao_b), c.s));
  DQ_TRY(wide_gemm(c, c.prm(p.ao_w), 0, HID, dao, Cm, c.g(a.w_o), HID, HID, RT, Cm, nullptr, 0));
  DQ_TRY(launch_repitch(c.g(a.o), RT, c.g(a.w_o), P, (int64_t)B * HID, RT, c.s));
  DQ_TRY(launch_copy(c.g(a.wmid1.out), dao, t, c.s));  // the residual branch: first writer of d(mid1.out)
  const int64_t qvbs = (int64_t)2 * HID * RT, kbs = (int64_t)HID * RT;
  DQ_TRY(launch_attn_bwd(c.w(a.qv), qvbs, c.w(a.kk), kbs, c.w(a.qv) + kbs, qvbs, c.w(a.o), c.g(a.o), c.w(a.lse), c.w(a.delta), c.g(a.qv),
                         qvbs, c.g(a.kk), kbs, c.g(a.qv) + kbs, qvbs, B, RT, c.s));
  if (rope) {
    DQ_TRY(launch_rope2(c.g(a.qv), (int64_t)2 * HID * RT, c.g(a.kk), (int64_t)HID * RT, rope, B, RT, -1.f, c.s));
  }
  DQ_TRY(conv_plain_bwd(c, proj(p.k_w, HID, p.cond_dim), CONV_S1, c.w(a.ms1f), c.g(a.kk), c.g(a.ms1f), B, RT, RT, 0));
  DQ_TRY(launch_repitch(c.g(a.w_qv), P, c.g(a.qv), RT, (int64_t)B * 2 * HID, RT, c.s));
  DQ_TRY(wide_wgrad(c, c.g(a.w_qv), c.w(a.w_xn), c.dprm(p.qv_w), 2 * HID, Cm));
  DQ_TRY(wide_gemm(c, c.prm(p.qv_w), 0, Cm, c.g(a.w_qv), 2 * HID, c.g(a.w_xn), Cm, Cm, RT, 2 * HID, nullptr, 0));
  // PreNorm backward (no scale/shift, no activation), in place on d(xn); then into d(mid1.out)
  DQ_TRY(launch_wnorm_bwd(c.w(a.wmid1.out), c.g(a.w_xn), c.prm(p.ag), nullptr, 0, ACT_NONE, c.g(a.w_xn), c.dprm(p.ag), nullptr, nullptr, st, B,
                          Cm, RT, P, c.s));
  DQ_TRY(launch_axpy(c.g(a.wmid1.out), c.g(a.w_xn), t, c.s));
  DQ_TRY(wide_res_bwd(c, p.mid1, a.wmid1, c.w(a.w_mid_in), c.g(a.w_mid_in)));
  return launch_fold(c.g(a.w_mid_in), c.g(a.downs[L - 1].rs), B, RT, Cm, 0, 0, c.s, P);
}

// ---------------------------------------------------------------------------------------------------------------
// the narrow (register-resident) bottleneck: mid_block1, Residual(PreNorm(Attention(use_xattn))), mid_block2 over (B, mid_c, RT) tensors
// (unet1d.py:1144-1148).  The folds into and out of that layout stay with the passes: the tiny levels next to the bottleneck may have done them.
// ---------------------------------------------------------------------------------------------------------------
// 16 channels (the default U-Net): which pieces of the attention ride in the neighbouring ResnetBlock's launch (k_res_rt.hip).  Both passes ask
// here, so the backward agrees with what the forward of the same step stored.
struct MidForms {
  bool qkv_fused;  // forward: PreNorm, to_qv, to_k and RoPE behind mid_block1
  bool out_fused;  // forward: to_out + bias + the residual in front of mid_block2; backward: d o = W_o^T d attn_out behind mid_block2's d x
  bool pre_fused;  // backward: RoPE^T, d xn = W_qv^T d qv, the PreNorm backward and the residual add in front of mid_block1's backward
};
MidForms mid_forms(const Plan& p, const Arena& a, int B, int RT) {
  auto rt = [&](const ResP& r) { return res_fwd_form(p.mid_c, p.mid_c, 0, r.res.cout != 0, B, RT, 1) == RES_FWD_RT && HID == 128; };
  MidForms f;
  f.qkv_fused = rt(p.mid1) && p.cond_dim == 8 && !DQ_DEV_FLAG("DQ_NO_MID_QKV", '1');  // (dev switch)
  f.out_fused = rt(p.mid2) && !DQ_DEV_FLAG("DQ_NO_MID_OUT", '1');  // (dev switch)
  f.pre_fused = rt(p.mid1) && a.bb_part_floats >= (int64_t)64 * B * p.mid_c && !DQ_DEV_FLAG("DQ_NO_MID_PRE", '1');  // (dev switch)
  return f;
}

// mid_in -> mid2.out.  skip_ms1: the sampling prologue formed (and rotated) k already; prep_ok: the prepare launch filled the aligned weight slots
int mid_forward(const Ctx& c, const float* rope, bool skip_ms1, bool prep_ok) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int B = c.B, RT = c.RT;
  const MidForms mf = mid_forms(p, a, B, RT);
  // 16 channels (the default U-Net): PreNorm, to_qv, to_k and RoPE ride behind mid_block1 (k_res_rt.hip)
  if (mf.qkv_fused) {
    ResRtQkv q;
    q.gn = c.prm(p.ag); q.wqv = c.prm(p.qv_w); q.xn = c.save ? c.w(a.xn) : nullptr; q.qv = c.w(a.qv); q.rope = rope;
    if (!skip_ms1) { q.wk = c.prm(p.k_w); q.ms1f = c.w(a.ms1f); q.kk = c.w(a.kk); }
    DQ_TRY(res_fwd(c, p.mid1, a.mid1, c.w(a.mid_in), p.mid_c, nullptr, 0, B, RT, 1, &q));
  } else {
    DQ_TRY(res_fwd(c, p.mid1, a.mid1, c.w(a.mid_in), p.mid_c, nullptr, 0, B, RT, 1));
    // Residual(PreNorm(Attention(use_xattn))) (unet1d.py:552-567)
    DQ_TRY(launch_rmsnorm_fwd(c.w(a.mid1.out), c.prm(p.ag), c.w(a.xn), p.mid_c, B, RT, c.s));
    DQ_TRY(conv_plain_fwd(c, proj(p.qv_w, 2 * HID, p.mid_c), CONV_S1, c.w(a.xn), c.w(a.qv), B, RT, RT, prep_ok ? 0 : -1));
    if (!skip_ms1) DQ_TRY(conv_plain_fwd(c, proj(p.k_w, HID, p.cond_dim), CONV_S1, c.w(a.ms1f), c.w(a.kk), B, RT, RT, prep_ok ? 1 : -1));
    if (rope) {
      // q = first 128 channels of each sample's 256; k rides in the same launch unless the sampling prologue rotated it already
      if (!skip_ms1) DQ_TRY(launch_rope2(c.w(a.qv), (int64_t)2 * HID * RT, c.w(a.kk), (int64_t)HID * RT, rope, B, RT, 1.f, c.s));
      else DQ_TRY(launch_rope(c.w(a.qv), rope, B, (int64_t)2 * HID * RT, RT, 1.f, c.s));
    }
  }
  const int64_t qvbs = (int64_t)2 * HID * RT, kbs = (int64_t)HID * RT;
  DQ_TRY(launch_attn_fwd(c.w(a.qv), qvbs, c.w(a.kk), kbs, c.w(a.qv) + kbs, qvbs, c.w(a.o), c.w(a.lse), B, RT, c.s));
  // 16 channels: to_out (1x1 + bias) and the residual are formed in FRONT of mid_block2, inside its launch (k_res_rt.hip)
  if (mf.out_fused) {
    ResRtOut ao;
    ao.o = c.w(a.o); ao.w = c.prm(p.ao_w); ao.b = c.prm(p.ao_b); ao.res = c.w(a.mid1.out); ao.out = c.w(a.attn_out);
    return res_fwd(c, p.mid2, a.mid2, c.w(a.attn_out), p.mid_c, nullptr, 0, B, RT, 1, nullptr, &ao);
  }
  const ConvP ao = proj(p.ao_w, p.mid_c, HID);
  if (conv_is_gemm(c, ao, CONV_S1, RT, RT) && (prep_ok || ((uintptr_t)c.prm(ao.w) & 15) == 0)) {
    // to_out (1x1 conv, 128 -> mid_c channels, with bias) + the residual: attn_out = x ; attn_out += W o + b as a GEMM per sample
    Gemm g;
    DQ_TRY(gemm_weight(c, ao, &g.A, 2));
    g.lda = HID; g.B = c.w(a.o); g.b_kmajor = 0; g.ldb = RT; g.C = c.w(a.attn_out); g.ldc = RT; g.M = p.mid_c; g.N = RT; g.K = HID;
    g.batch = B; g.sBo = (int64_t)HID * RT; g.sCo = (int64_t)p.mid_c * RT; g.bias_m = c.prm(p.ao_b);
    g.add = c.w(a.mid1.out); g.splits = 1;  // the residual is read by the epilogue (was: a copy launch + "+=")
    DQ_TRY(launch_gemm(g, c.s));
  } else {
    ConvFwd f;
    f.inA = c.w(a.o); f.cinA = HID; f.w = c.prm(p.ao_w); f.bias = c.prm(p.ao_b); f.cout = p.mid_c; f.K = 1;
    f.rows = B; f.n_in = RT; f.n_out = RT; f.y_out = c.w(a.attn_out);
    f.resA = c.w(a.mid1.out); f.rcinA = p.mid_c;
    DQ_TRY(launch_conv_fwd(f, c.s));
  }
  return res_fwd(c, p.mid2, a.mid2, c.w(a.attn_out), p.mid_c, nullptr, 0, B, RT, 1);
}

// d(mid2.out) is complete; leaves d(mid_in) and all bottleneck parameter gradients (+=).  grad_x: the caller asked for d loss / d x: what would
// ride on the side queue then stays on the main stream, as in unet_backward; prep_ok: as for mid_forward, from the same LevelPlan
int mid_backward(const Ctx& c, const float* rope, bool grad_x, bool prep_ok) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int B = c.B, RT = c.RT;
  const MidForms mf = mid_forms(p, a, B, RT);
  // 16 channels: d o = W_o^T d attn_out follows mid_block2's d x inside its launch (k_res_rt.hip); to_out's weight gradient stays below
  if (mf.out_fused) {
    ResRtOut ao;
    ao.w = c.prm(p.ao_w); ao.d_o = c.g(a.o);
    DQ_TRY(res_bwd(c, p.mid2, a.mid2, c.w(a.attn_out), c.g(a.attn_out), p.mid_c, nullptr, nullptr, 0, B, RT, 1, 0, 0, nullptr, nullptr, &ao));
  } else {
    DQ_TRY(res_bwd(c, p.mid2, a.mid2, c.w(a.attn_out), c.g(a.attn_out), p.mid_c, nullptr, nullptr, 0, B, RT, 1));
  }
  const int64_t qvbs = (int64_t)2 * HID * RT, kbs = (int64_t)HID * RT;
  // to_out (1x1 + bias) and the residual
  ConvP ao = proj(p.ao_w, p.mid_c, HID);
  ao.b = p.ao_b;
  const int ws_ok = prep_ok ? 0 : -3;  // aligned weight slots as the forward of this step filled them (0: q|v, 1: k, 2: to_out)
  DQ_TRY(conv_plain_bwd(c, ao, CONV_S1, c.w(a.o), c.g(a.attn_out), mf.out_fused ? nullptr : c.g(a.o), B, RT, RT, 0, ws_ok + 2));  // (fused: the weight / bias gradient only)
  // (d mid1.out = d attn_out [the residual] + the PreNorm path: formed by the PreNorm backward below, which reads d attn_out as its addend --
  // was a k_axpy launch here plus one behind that kernel)
  DQ_TRY(launch_attn_bwd(c.w(a.qv), qvbs, c.w(a.kk), kbs, c.w(a.qv) + kbs, qvbs, c.w(a.o), c.g(a.o), c.w(a.lse), c.w(a.delta),
                         c.g(a.qv), qvbs, c.g(a.kk), kbs, c.g(a.qv) + kbs, qvbs, B, RT, c.s));
  const bool side = !grad_x && tail_fork_enabled();  // (the conditions under which the MS1 path's backward rides on the side queue too)
  if (!mf.pre_fused) {
    if (rope) {
      DQ_TRY(launch_rope2(c.g(a.qv), (int64_t)2 * HID * RT, c.g(a.kk), (int64_t)HID * RT, rope, B, RT, -1.f, c.s));
    }
    DQ_TRY(conv_plain_bwd(c, proj(p.k_w, HID, p.cond_dim), CONV_S1, c.w(a.ms1f), c.g(a.kk), c.g(a.ms1f), B, RT, RT, 0, ws_ok + 1));
    DQ_TRY(conv_plain_bwd(c, proj(p.qv_w, 2 * HID, p.mid_c), CONV_S1, c.w(a.xn), c.g(a.qv), c.g(a.xn), B, RT, RT, 0, ws_ok));
    // PreNorm backward: xn = rmsnorm(mid1.out) * g  (pointwise kernel, no scale/shift, no activation)
    BlockBwd nb;
    // (du accumulates straight into d mid1.out -- the residual branch's gradient is there already: was a separate k_axpy launch behind this one)
    nb.u = c.w(a.mid1.out); nb.dy = c.g(a.xn); nb.du = c.g(a.mid1.out); nb.accumulate = 1; nb.add_src = c.g(a.attn_out); nb.C = p.mid_c; nb.rows = B; nb.n = RT; nb.rows_per_sample = 1;
    nb.g = c.prm(p.ag); nb.dg = c.dprm(p.ag);
    nb.part = c.w(a.bb_part); nb.part_floats = a.bb_part_floats;
    // (the gain's slot reduction feeds nothing on the chain: with the next side-stream flush.  The slot's other users: the MS1 path's backward, on
    // the side stream behind it, and the input-affine backward at the end of the pass -- on the side stream too, or on the main stream behind the
    // event that marks the side queue's state in front of the tail: unet_backward's `ev_ss`)
    PartReduce gred;
    const bool defer = side_open(c, side);
    if (defer) nb.defer_reduce = &gred;
    DQ_TRY(launch_block_bwd(nb, c.s));
    if (defer && gred.part) DQ_TRY(on_side(c, true, [gred](hipStream_t ss) { return launch_part_reduce(gred, ss); }));  // (behind the flush's fork event whatever precedes it)
    return res_bwd(c, p.mid1, a.mid1, c.w(a.mid_in), c.g(a.mid_in), p.mid_c, nullptr, nullptr, 0, B, RT, 1);
  }
  // 16 channels with a side queue at hand: RoPE^T, d xn = W_qv^T d qv, the PreNorm backward and the residual add run as the PROLOGUE of
  // mid_block1's backward (k_res_rt.hip), which reads d q in the rotated frame.  What is left needs nothing of the main chain any more:
  // RoPE^T in memory (the weight gradients of to_qv / to_k want d q, d k in the unrotated frame), d ms1f and both weight gradients go to
  // the side queue -- behind the next flush's fork event, i.e. behind mid_block1's backward, which has read d q by then.
  // (without a side queue -- the captured step, a plan without an owner -- the same launches follow mid_block1's backward on the main stream:
  // the arithmetic, and with it every bit of the step, does not depend on the schedule)
  const ConvP kp = proj(p.k_w, HID, p.cond_dim), qp = proj(p.qv_w, 2 * HID, p.mid_c);
  auto mid_rest = [&a, rope, B, RT, kp, qp, ws_ok](const Ctx& cc) -> int {  // (on cc.s; weight gradients wherever cc sends them)
    if (rope) DQ_TRY(launch_rope2(cc.g(a.qv), (int64_t)2 * HID * RT, cc.g(a.kk), (int64_t)HID * RT, rope, B, RT, -1.f, cc.s));
    DQ_TRY(conv_plain_bwd(cc, kp, CONV_S1, cc.w(a.ms1f), cc.g(a.kk), cc.g(a.ms1f), B, RT, RT, 0, ws_ok + 1));
    return conv_plain_bwd(cc, qp, CONV_S1, cc.w(a.xn), cc.g(a.qv), nullptr, B, RT, RT, 0, ws_ok);  // (weight gradient only)
  };
  ResRtPre q;
  q.dqv = c.g(a.qv); q.wqv = c.prm(p.qv_w); q.x = c.w(a.mid1.out); q.gn = c.prm(p.ag); q.add = c.g(a.attn_out); q.rope = rope;
  q.gn_part = c.w(a.bb_part); q.gn_part_floats = a.bb_part_floats;
  int gblocks = 0;
  DQ_TRY(res_bwd(c, p.mid1, a.mid1, c.w(a.mid_in), c.g(a.mid_in), p.mid_c, nullptr, nullptr, 0, B, RT, 1, 0, 0, &q, &gblocks));
  PartReduce gred;  // d (PreNorm gain): the workgroups' sums in block order
  gred.part = c.w(a.bb_part); gred.B = B; gred.gx = gblocks; gred.nv = p.mid_c; gred.nseg = 1;
  gred.seg_start[0] = 0; gred.seg_len[0] = p.mid_c; gred.seg_dst[0] = c.dprm(p.ag);
  // without the side queue: on the main stream (d ms1f is read there next); the two weight gradients go where they always go (wgrad_async: the
  // side queue's shared partial-sum scratch belongs to one stream)
  DQ_TRY(on_side(c, side, mid_rest));
  return on_side(c, side, [gred](hipStream_t ss) { return launch_part_reduce(gred, ss); });
}

// ---------------------------------------------------------------------------------------------------------------
// one launch per level for [the resample conv that produces the level's input] + the level's ResnetBlocks (k_level.hip)
// ---------------------------------------------------------------------------------------------------------------
// One launch of the walk as Plan and Arena describe it: the input stage, the ResnetBlocks and where their operands lie (arena offsets; -1: none)
struct LevelCall {
  int pre = LEVEL_PRE_NONE; const ConvP* pc = nullptr; int64_t in = -1, pre_out = -1;
  int C = 0, n = 0, nblocks = 0;
  const ResP* r[2] = {nullptr, nullptr}; const ResBuf* rb[2] = {nullptr, nullptr};
  int64_t inB[2] = {-1, -1}; int cinB[2] = {0, 0}; bool write_out[2] = {true, true};
  const float* x = nullptr; const float* cond = nullptr; float cm = 1.f, ca = 0.f;  // LEVEL_PRE_INIT: the caller's x_t and mixture (the walk sets them)
  const ConvP* head = nullptr; float* eps_out = nullptr;      // head epilogue (final_conv)
};
// A level whose ResnetBlocks the level kernel takes also computes its own input from the previous level's LinearAttention
// output (Downsample, unet1d.py:1141): that conv is then not launched and, in inference, its result never exists in memory.
// Level 0 with `init`: the mixture conditioning + concat + init_conv (unet1d.py:1107-1118) are that launch's input stage.
LevelCall down_call(const Plan& p, const Arena& a, int lv, bool init) {
  LevelCall lc;
  const LevelP& l = p.downs[lv];
  lc.C = l.r0.cout; lc.n = l.n; lc.nblocks = 2;
  lc.r[0] = &l.r0; lc.r[1] = &l.r1; lc.rb[0] = &a.downs[lv].r0; lc.rb[1] = &a.downs[lv].r1;
  if (lv > 0) { lc.pre = LEVEL_PRE_DOWN; lc.pc = &p.downs[lv - 1].resample; lc.in = a.downs[lv - 1].la; lc.pre_out = a.downs[lv - 1].rs; }
  else if (init) { lc.pre = LEVEL_PRE_INIT; lc.pc = &p.init_conv; lc.pre_out = a.h0; }
  else lc.in = a.h0;
  return lc;
}
// up path (unet1d.py:1150-1158): first pop = post-attention skip, second pop = post-block1 skip
LevelCall up_call(const Plan& p, const Arena& a, int ui) {  // ui == L: the final ResnetBlock behind the last level's k3 conv (unet1d.py:1160-1163)
  LevelCall lc;
  const int L = p.levels;
  if (ui < L) {
    const LevelP& l = p.ups[ui];
    const int lv = L - 1 - ui, cs = l.r0.cin - l.r0.cout;
    lc.C = l.r0.cout; lc.n = l.n; lc.nblocks = 2;
    lc.r[0] = &l.r0; lc.r[1] = &l.r1; lc.rb[0] = &a.ups[ui].r0; lc.rb[1] = &a.ups[ui].r1;
    lc.inB[0] = a.downs[lv].la; lc.inB[1] = a.downs[lv].r0.out; lc.cinB[0] = lc.cinB[1] = cs;
    lc.write_out[0] = false;  // (inference: only the second block's output leaves the launch)
  } else {
    lc.C = p.fin.cout; lc.n = p.mz; lc.nblocks = 1;
    lc.r[0] = &p.fin; lc.rb[0] = &a.fin; lc.inB[0] = a.h0; lc.cinB[0] = p.dim;
  }
  if (ui == 0) { lc.in = a.mid_back; }
  else {
    const LevelP& lp = p.ups[ui - 1];
    lc.pre = lp.last ? LEVEL_PRE_S1 : LEVEL_PRE_UP; lc.pc = &lp.resample; lc.in = a.ups[ui - 1].la; lc.pre_out = a.ups[ui - 1].rs;
  }
  return lc;
}
// what the *_usable predicates and level_img_floats read of a descriptor: its shape, and WHETHER a pointer is set (SHAPE_ONLY stands for "set")
const float SHAPE_ONLY[1] = {0.f};
LevelFwd level_shape(const LevelCall& lc, int B, int RT) {
  LevelFwd f;
  f.params = SHAPE_ONLY; f.pre = lc.pre; f.nblocks = lc.nblocks; f.C = lc.C; f.rows = B * RT; f.n = lc.n; f.rows_per_sample = RT;
  if (lc.pc) f.cp = lc.pc->cin;
  for (int i = 0; i < lc.nblocks; ++i) { f.blk[i].cinB = lc.cinB[i]; f.blk[i].wr = lc.r[i]->res.cout ? SHAPE_ONLY : nullptr; }
  return f;
}
// img_slot: the launch's slot of the operand-image region (LevelForm::img), or -1
LevelFwd level_desc(const Ctx& c, const LevelCall& lc, int img_slot = -1) {
  LevelFwd f = level_shape(lc, c.B, c.RT);
  f.params = c.P; f.in = lc.in >= 0 ? c.w(lc.in) : lc.x;
  float* pre_out = lc.pre_out >= 0 ? c.w(lc.pre_out) : nullptr;
  if (lc.pc) { f.pw = c.prm(lc.pc->w); f.pb = lc.pc->b >= 0 ? c.prm(lc.pc->b) : nullptr; f.pre_out = c.save ? pre_out : nullptr; }
  if (lc.pre == LEVEL_PRE_INIT) {
    f.cond = lc.cond; f.cm = lc.cm; f.ca = lc.ca; f.ss_init = c.w(c.ar.ss) + c.p.ss_init; f.pre_out = pre_out;
    f.cat0_out = c.save ? c.w(c.ar.cat0) : nullptr;  // (train step: kept for init_conv's weight gradient and the input affine's backward)
    if (c.qsample && f.cat0_out) {
      f.in = c.qsample->x0; f.qs_noise = c.qsample->noise; f.qs_ab = c.qsample->alpha_bars; f.qs_t = c.qsample->t; f.qs_norm = c.qsample->normalize;
    }
  }
  if (lc.head) {
    f.ew = c.prm(lc.head->w); f.eb = c.prm(lc.head->b); f.final_act = c.p.final_act;
    if (c.step_io && c.step_io->x_t) {
      f.x_t = c.step_io->x_t; f.x_out = c.step_io->x_out; f.coef = c.step_io->coef; f.step_ptr = c.step_io->step_ptr; f.pred = c.step_io->pred;
      f.eps_out = c.step_io->want_eps ? lc.eps_out : nullptr;  // (the trajectory's eps, when the caller keeps one)
    } else {
      f.eps_out = lc.eps_out;
    }
  }
  for (int i = 0; i < lc.nblocks; ++i)
    f.blk[i] = level_block(c, *lc.r[i], *lc.rb[i], lc.cinB[i] ? c.w(lc.inB[i]) : nullptr, lc.cinB[i], lc.write_out[i]);
  if (img_slot >= 0) f.img = c.w(c.ar.wimg) + (int64_t)img_slot * LEVEL_IMG_FLOATS;
  return f;
}

// Which launch takes each level, decided ONCE per pass: unet_forward, unet_backward and the sampler's prologue build a LevelPlan with level_plan
// and everything they call reads it.  Nothing else asks a *_usable predicate during the walk, so the backward agrees with what the forward of
// the same step ran and stored (same Plan, Arena, batch and switches => same plan).
enum LevelKind { LEVEL_UNFUSED, LEVEL_KERNEL, LEVEL_TINY };  // res_fwd calls | k_level_fwd | k_tiny_fwd
struct LevelForm {
  LevelKind kind = LEVEL_UNFUSED;
  int img = -1;  // operand-image slot: LEVEL_KERNEL in Arena::wimg (level on the way down, L + ui on the way up, 2 L the head; -1: the kernel gathers
                 // its weights itself), LEVEL_TINY in Arena::timg (0..3; slots 4, 5 are the backward's)
  // LEVEL_TINY at n == 1: the LinearAttention rides along; the last down level also applies its k3 conv and writes the bottleneck's (B, C, RT)
  // layout directly (no k_conv_fwd, no k_fold); the first up level reads that layout (no k_fold behind the bottleneck either)
  bool la = false, post_w = false, in_folded = false;
  bool resample = true;  // the level's own resample conv is launched (false: it is the input stage of the next launch, or post_w)
};
struct LevelPlan {
  LevelForm dn[16], up[17];  // up[L]: the final ResnetBlock (build_plan: L <= 10)
  bool prep_ok = false;      // la_prepare_all has a slot for every LinearAttention layer (and fills the aligned weight slots of the bottleneck's GEMMs)
  bool init_fused = false;   // level 0's launch forms its own input (LEVEL_PRE_INIT)
  bool head_shape = false, head_train = false;  // the final block's launch can apply final_conv; head_train: and the loss + d fin.out of a train step
  bool use_tb_up = false, use_tb_dn = false, tb_up_w = false;  // backward of the first up / last down level in one k_tiny_bwd launch; the Upsample transpose rides along
};
bool level_ok(const LevelCall& lc, int B, int RT) {
  if (DQ_DEV_FLAG("DQ_NO_LEVEL_FWD", '1')) return false;  // (dev switch)
  for (int i = 0; i < lc.nblocks; ++i)
    if (lc.r[i]->cout != lc.C || lc.r[i]->cin != lc.C + lc.cinB[i]) return false;
  if (lc.pc && (lc.pc->cout != lc.C || lc.pc->b < 0)) return false;
  return level_fwd_usable(level_shape(lc, B, RT));
}
bool tiny_bwd_ok(const Plan& p, int B, int RT, bool up, bool* up_w) {
  const int L = p.levels;
  if (L < 2 || p.wide_mid || p.mid_n != 1) return false;
  const LevelP& l = up ? p.ups[0] : p.downs[L - 1];
  const ConvP& rs = l.resample;
  if (l.n != 1 || l.la.C != 16 || l.r0.cout != 16 || l.r1.cout != 16 || l.r1.cin != l.r0.cin) return false;
  TinyBwd t;
  t.params = SHAPE_ONLY; t.C = 16; t.rows = B * RT; t.rows_per_sample = RT; t.pre = up ? LEVEL_PRE_NONE : LEVEL_PRE_DOWN; t.cs = l.r0.cin - l.r0.cout;
  if (!up) {
    const LevelP& lp = p.downs[L - 2];
    if (rs.k != 3 || rs.cout != 16 || rs.cin != 16 || lp.resample.k != 4 || lp.resample.cout != 16 || lp.n != 2) return false;
    t.cp = lp.resample.cin;
  }
  if (!tiny_bwd_usable(t)) return false;
  const bool upt_on = !DQ_DEV_FLAG("DQ_NO_TINY_UPT", '1');  // (dev switch)
  if (up) *up_w = upt_on && !l.last && rs.k == 3 && rs.cin == 16 && rs.cout == 16 && l.n_next == 2;  // the Upsample conv behind the level (nearest x2 + k3, 16 -> 16)
  return true;
}
// save: the pass keeps what a backward needs (a backward itself: true); twin: it has the gradient arena at hand
LevelPlan level_plan(const Plan& p, const Arena& a, int B, int RT, bool save, bool twin) {
  LevelPlan lp;
  const int L = p.levels;
  lp.prep_ok = (int)(p.downs.size() + p.ups.size()) <= LA_PREP_MAX;
  // the levels with rows of 1 or 2 positions (k_tiny.hip): stage + both ResnetBlocks as a chain of dense layers
  const bool mid1 = !p.wide_mid && p.mid_n == 1;
  int n_tiny = 0;
  auto tiny = [&](LevelForm& f, const LevelCall& lc, bool la, bool post_w, bool in_folded) {
    TinyFwd t;
    t.lv = level_shape(lc, B, RT); t.la = la; t.post_w = post_w ? SHAPE_ONLY : nullptr; t.in_folded = in_folded;
    if (L > 16 || n_tiny >= 4 || !tiny_fwd_usable(t)) return;
    f.kind = LEVEL_TINY; f.img = n_tiny++; f.la = la; f.post_w = post_w; f.in_folded = in_folded;
  };
  for (int lv = 1; lv < L; ++lv) {
    const LevelP& l = p.downs[lv];
    const bool la = l.n == 1 && lv == L - 1 && mid1 && l.resample.k == 3 && l.resample.b >= 0 && l.resample.cout == l.la.C;
    tiny(lp.dn[lv], down_call(p, a, lv, false), la, la, false);
  }
  for (int ui = 0; ui < L; ++ui) {
    const bool la = p.ups[ui].n == 1 && ui == 0 && mid1;
    tiny(lp.up[ui], up_call(p, a, ui), la, false, la);
  }
  // everything else the level kernel can take (k_level.hip), with an operand image when the region has a slot for every launch
  auto level = [&](LevelForm& f, const LevelCall& lc, int slot) {
    if (f.kind == LEVEL_TINY || !level_ok(lc, B, RT)) return;
    f.kind = LEVEL_KERNEL;
    if (2 * L + 1 <= LEVEL_IMG_MAX && level_img_floats(level_shape(lc, B, RT)) <= LEVEL_IMG_FLOATS) f.img = slot;
  };
  const bool train_init = !DQ_DEV_FLAG("DQ_NO_TRAIN_INIT", '1');  // (dev switch)
  const bool init = (!save || train_init) && p.dim == 4 && p.init_conv.cout == 4 && p.init_conv.cin == 2 && p.init_conv.k == 7 && p.init_conv.b >= 0;
  level(lp.dn[0], down_call(p, a, 0, init), 0);
  lp.init_fused = init && lp.dn[0].kind == LEVEL_KERNEL;
  for (int lv = 1; lv < L; ++lv) level(lp.dn[lv], down_call(p, a, lv, false), lv);
  for (int ui = 0; ui <= L; ++ui) level(lp.up[ui], up_call(p, a, ui), L + ui);
  // a launch that is not a chain of res_fwd calls applies the resample conv in front of it itself
  for (int lv = 0; lv < L; ++lv) lp.dn[lv].resample = lv + 1 < L ? lp.dn[lv + 1].kind == LEVEL_UNFUSED : !lp.dn[lv].post_w;
  for (int ui = 0; ui < L; ++ui) lp.up[ui].resample = lp.up[ui + 1].kind == LEVEL_UNFUSED;
  // head (unet1d.py:1160-1166)
  lp.head_shape = p.dim == 4 && p.final_conv.cout == 1 && p.final_conv.cin == 4 && p.final_conv.k == 1 && p.final_conv.b >= 0 && lp.up[L].kind == LEVEL_KERNEL;
  // (built for the (4, k3 conv, 4) launch; one partial sum per wave: beyond a resident round the grid is B workgroups)
  lp.head_train = save && twin && lp.head_shape && p.ups[L - 1].last && p.ups[L - 1].resample.cin == 4 && (int64_t)B * 4 <= LEVEL_LOSS_PARTS;
  // the tiny backward reads what the tiny forward of the same level stored, through images the same forward built
  lp.use_tb_up = save && lp.up[0].kind == LEVEL_TINY && tiny_bwd_ok(p, B, RT, true, &lp.tb_up_w);
  lp.use_tb_dn = save && lp.dn[L - 1].kind == LEVEL_TINY && tiny_bwd_ok(p, B, RT, false, nullptr);
  return lp;
}

// the k_tiny_fwd launch of a LEVEL_TINY level
TinyFwd tiny_desc(const Ctx& c, const LevelPlan& lp, bool up, int i) {
  const Arena& a = c.ar;
  const LevelForm& f = up ? lp.up[i] : lp.dn[i];
  const LevelP& l = up ? c.p.ups[i] : c.p.downs[i];
  const LevelBuf& b = up ? a.ups[i] : a.downs[i];
  TinyFwd t;
  t.lv = level_desc(c, up ? up_call(c.p, a, i) : down_call(c.p, a, i, false));
  t.img = c.w(a.timg) + (int64_t)f.img * TINY_IMG_FLOATS;
  if (f.la) { t.la = 1; la_operands(c, l.la, t, &t.b_out); t.la_y = c.w(b.la); t.la_ypre = c.save ? c.w(b.la_pre) : nullptr; }
  if (f.post_w) { t.post_w = c.prm(l.resample.w); t.post_b = c.prm(l.resample.b); t.post_out = c.w(a.mid_in); }
  if (f.in_folded) { t.in_folded = 1; t.lv.in = c.w(a.mid2.out); t.in_copy = c.save ? c.w(a.mid_back) : nullptr; }
  return t;
}

// The launches that depend on the parameter values only -- W2 / the q | k operand images of the LinearAttention layers, the MFMA operand
// images of the level and tiny launches, the transposed images of the tiny backward -- once per parameter state: every forward in training,
// once per dq_ddim_sample call.  ps: the stream of all but the level images (the side stream of a forked train step); ev_prep (forked only):
// receives an event behind la_prepare_all -- level 0's LinearAttention waits for THAT, the tiny images are needed five levels later.
int unet_prepare(const Ctx& c, const LevelPlan& lp, hipStream_t ps, hipEvent_t* ev_prep = nullptr) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int L = p.levels;
  DQ_TRY(la_prepare_all(c, lp.prep_ok, ps));
  if (ev_prep) DQ_TRY(side_mark(c, ev_prep));
  LevelFwd calls[LEVEL_IMG_MAX];
  int nc = 0, nt = 0, nb = 0;
  for (int lv = 0; lv < L; ++lv)
    if (lp.dn[lv].kind == LEVEL_KERNEL && lp.dn[lv].img >= 0) calls[nc++] = level_desc(c, down_call(p, a, lv, lp.init_fused), lp.dn[lv].img);
  for (int ui = 0; ui <= L; ++ui)
    if (lp.up[ui].kind == LEVEL_KERNEL && lp.up[ui].img >= 0) calls[nc++] = level_desc(c, up_call(p, a, ui), lp.up[ui].img);
  DQ_TRY(launch_level_images(calls, nc, c.s));
  TinyFwd tc[TINY_IMG_MAX];
  for (int lv = 0; lv < L; ++lv) if (lp.dn[lv].kind == LEVEL_TINY) tc[nt++] = tiny_desc(c, lp, false, lv);
  for (int ui = 0; ui < L; ++ui) if (lp.up[ui].kind == LEVEL_TINY) tc[nt++] = tiny_desc(c, lp, true, ui);
  DQ_TRY(launch_tiny_images(tc, nt, ps));
  if (!c.save) return 0;
  TinyBwd tb[2];
  if (lp.use_tb_up) tb[nb++] = tiny_bwd_desc(c, true, lp.tb_up_w);
  if (lp.use_tb_dn) tb[nb++] = tiny_bwd_desc(c, false, false);
  return launch_tiny_bwd_images(tb, nb, ps);
}

// MS1 features (unet1d.py:1120-1130) on stream s: (B, RT, M1) -> conv k7 -> GELU -> conv k1 = ms1f; what the backward reads is kept only when c.save.
// norm (one channel): the normalised chromatogram is formed here (else k_prep_inputs left it in ms1n)
int ms1_features(const Ctx& c, const float* ms1, float cm, float ca, bool norm, hipStream_t s) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int B = c.B, RT = c.RT, M1 = p.ms1_channels;
  if (M1 > 1) {  // (B, RT, M1) read as it is: k_ms1_feat.hip
    Ms1FeatFwd f;
    f.ms1 = ms1; f.w = c.prm(p.ms1_c0.w); f.bias = c.prm(p.ms1_c0.b); f.cm = cm; f.ca = ca; f.B = B; f.RT = RT; f.M1 = M1;
    f.ms1n_out = c.save ? c.w(a.ms1n) : nullptr; f.u_out = c.save ? c.w(a.ms1_u) : nullptr; f.a_out = c.w(a.ms1_a);
    DQ_TRY(launch_ms1_feat_fwd(f, s));
  } else {
    if (norm) DQ_TRY(launch_ms1_norm(ms1, cm, ca, c.w(a.ms1n), (int64_t)B * RT, s));
    ConvFwd f;
    f.inA = c.w(a.ms1n); f.cinA = 1; f.w = c.prm(p.ms1_c0.w); f.bias = c.prm(p.ms1_c0.b); f.cout = p.cond_dim; f.K = 7;
    f.rows = B; f.n_in = RT; f.n_out = RT; f.u_out = c.save ? c.w(a.ms1_u) : nullptr; f.y_out = c.w(a.ms1_a); f.act = ACT_GELU;
    DQ_TRY(launch_conv_fwd(f, s));
  }
  Ctx cs = c;
  cs.s = s;
  return conv_plain_fwd(cs, p.ms1_c1, CONV_S1, c.w(a.ms1_a), c.w(a.ms1f), B, RT, RT);
}

// ---------------------------------------------------------------------------------------------------------------
// the scaffolding of a backward pass: what its pieces queue instead of launching at once, the clearing of the twin, the end of the pass.
// unet_backward and the bottleneck-only entry (dq_debug_mid_bwd) run inside the same three functions.
// ---------------------------------------------------------------------------------------------------------------
struct BwdQueues {
  Ctx::LaDefer la;                 // LinearAttention slot reductions: one launch at the end (la_flush / la_flush_side)
  std::vector<Ctx::SideFn> side;   // side-stream launches behind the next side_flush (only with an owner: else they run where they are issued)
  std::vector<ResWgReduce> wg;     // slot reductions of the ResnetBlock backwards that form their own weight gradients
};
Ctx bwd_open(const Ctx& c_in, BwdQueues& q) {
  Ctx c = c_in;
  c.la_defer = &q.la;
  c.wg_defer = &q.wg;
  if (c.owner) c.side_defer = &q.side;
  return c;
}
// only the accumulated-into region of the twin (offsets are multiples of 64 floats); a forked forward of the same step cleared it already.
// keep >= 0: the extent [keep, keep + keep_floats) holds what the caller put there (the bottleneck-only entry's d mid2.out) and stays
int bwd_clear_twin(const Ctx& c, int64_t keep = -1, int64_t keep_floats = 0) {
  if (c.owner && c.owner->twin_zeroed == c.G) { c.owner->twin_zeroed = nullptr; return 0; }
  const int64_t z = c.ar.zero_floats;
  if (keep < 0) return launch_zero(c.G, z, c.s);
  const int64_t end = std::min(z, (keep + keep_floats + 63) / 64 * 64);
  if (keep > 0) DQ_TRY(launch_zero(c.G, std::min(keep, z), c.s));
  if (end < z) DQ_TRY(launch_zero(c.G + end, z - end, c.s));
  return 0;
}
// The end of a pass: the last weight-gradient launches go to the side stream BEFORE the LinearAttention slot reduce is queued on the main
// stream: the side stream waits for an event recorded here, and recorded behind the reduce it made those launches (init_conv, the MS1 convs:
// ~80 us) start only when the ~100 us reduce had finished -- an exposed tail in front of the join
int bwd_close(const Ctx& c, BwdQueues& q) {
  DQ_TRY(side_flush(c));
  DQ_TRY(la_flush(c));
  DQ_TRY(res_wg_reduce_all(q.wg, c.s));
  return join_side(c);
}

}  // namespace

int unet_forward(const Ctx& c, const float* rope, const float* x, const int64_t* t, int t_scalar, const float* init_cond,
                 const float* attn_cond, float cm, float ca, const DevTables& dt, float* out, const int* step_tab, const int* step_ptr) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int B = c.B, RT = c.RT, R = B * RT, L = p.levels;
  const LevelPlan lp = level_plan(p, a, B, RT, c.save, c.G != nullptr);
  const bool skip_ms1 = c.step_io && c.step_io->prologue;  // the sampler's prologue ran: the once-per-parameter-state launches, the MS1 features, to_k, RoPE(k)
  // Training steps (dq_train_step: side stream + gradient twin at hand): what the first level does not wait for runs on the side stream --
  // the LinearAttention / tiny-level operand preparation, the MS1 feature path (needed at the bottleneck) and the clearing of the
  // gradient twin's accumulated-into region (needed by the backward) were ~55 us at the head of the main queue, in front of or between
  // launches that do not depend on them.  One event forks; the main stream waits for `ev_prep` in front of the first LinearAttention and
  // for `ev_rest` in front of the first launch that reads the MS1 features.
  const bool fwd_fork_on = !DQ_DEV_FLAG("DQ_NO_FWD_FORK", '1');  // (dev switch)
  const bool fwd_fork = fwd_fork_on && c.owner && c.save && c.G && !c.step_io;
  hipStream_t ps = c.s;
  hipEvent_t ev_prep = nullptr, ev_rest = nullptr;
  bool wait_prep = fwd_fork, wait_rest = false;
  if (fwd_fork) { DQ_TRY(fork_side(c)); ps = c.owner->side_stream; }
  if (!skip_ms1) DQ_TRY(unet_prepare(c, lp, ps, fwd_fork ? &ev_prep : nullptr));  // (a fork has no step_io: it always prepares)
  // ---- input stage.  K1: time embedding + every scale/shift head (unet1d.py:1105, 315-318, 677)
  DQ_TRY(launch_time_embed_fwd(p, dt, c.P, t, t_scalar, c.w(a.tbuf), c.w(a.ss), B, step_tab, step_ptr, c.s));
  // K2: mixture conditioning + concat (unet1d.py:1107-1115), then init_conv k7 (:1117) -- level 0's INIT stage, or two launches here
  if (c.qsample && !(lp.init_fused && c.save))  // (the INIT stage of a train step forms x_t itself)
    DQ_TRY(launch_q_sample(c.qsample->alpha_bars, c.qsample->x0, c.qsample->t, c.qsample->noise, const_cast<float*>(x), B, c.qsample->per, c.qsample->normalize, c.s));
  const bool ms1n_here = !lp.init_fused && !fwd_fork && p.ms1_channels == 1;  // (forked: the MS1 normalisation goes with the MS1 path to the side stream)
  if (!lp.init_fused) {
    DQ_TRY(launch_prep_inputs(x, init_cond, attn_cond, c.w(a.ss), p.ss_total, p.ss_init, cm, ca, c.w(a.cat0), ms1n_here ? c.w(a.ms1n) : nullptr, B, RT, p.mz, c.s));
    DQ_TRY(conv_plain_fwd(c, p.init_conv, CONV_S1, c.w(a.cat0), c.w(a.h0), R, p.mz, p.mz));
  }
  // K3: MS1 features, unless the sampling prologue formed them
  if (!skip_ms1) DQ_TRY(ms1_features(c, attn_cond, cm, ca, !ms1n_here, ps));
  if (fwd_fork) {
    DQ_TRY(launch_zero(c.G, a.zero_floats, ps));  // (unet_backward skips its own clearing: dq_plan::twin_zeroed)
    c.owner->twin_zeroed = c.G;
    DQ_TRY(side_mark(c, &ev_rest));
    wait_rest = true;
  }
  // ---- down path (unet1d.py:1134-1142)
  const float* cur = c.w(a.h0);
  for (int lv = 0; lv < L; ++lv) {
    const LevelP& l = p.downs[lv];
    const LevelBuf& b = a.downs[lv];
    const LevelForm& f = lp.dn[lv];
    const int C = l.r0.cin;
    if (f.kind == LEVEL_TINY) {
      if (wait_rest) { DQ_HIP_OK(hipStreamWaitEvent(c.s, ev_rest, 0)); wait_rest = false; c.owner->side_used = false; }  // (its operand image came from the side stream)
      DQ_TRY(launch_tiny_fwd(tiny_desc(c, lp, false, lv), c.s));
      if (f.post_w) continue;  // (the last level: its k3 conv went into the bottleneck's layout)
    } else if (f.kind == LEVEL_KERNEL) {
      LevelCall lc = down_call(p, a, lv, lp.init_fused);
      if (lc.pre == LEVEL_PRE_INIT) { lc.x = x; lc.cond = init_cond; lc.cm = cm; lc.ca = ca; }
      DQ_TRY(launch_level_fwd(level_desc(c, lc, f.img), c.s));
    } else {
      DQ_TRY(res_fwd(c, l.r0, b.r0, cur, C, nullptr, 0, R, l.n, RT));
      DQ_TRY(res_fwd(c, l.r1, b.r1, c.w(b.r0.out), C, nullptr, 0, R, l.n, RT));
    }
    if (wait_prep) { DQ_HIP_OK(hipStreamWaitEvent(c.s, ev_prep, 0)); wait_prep = false; }  // (in front of lv 0's LinearAttention: the tiny levels come later)
    if (!f.la) DQ_TRY(la_fwd(c, l.la, c.w(b.r1.out), c.w(b.la), c.save ? c.w(b.la_pre) : nullptr, R, l.n, lp.prep_ok ? lv : -1));
    if (!f.resample) continue;  // the next level's launch applies this level's Downsample itself
    DQ_TRY(conv_plain_fwd(c, l.resample, l.last ? CONV_S1 : CONV_DOWN, c.w(b.la), c.w(b.rs), R, l.n, l.n_next));
    cur = c.w(b.rs);
  }
  // ---- bottleneck (unet1d.py:1144-1148)
  if (wait_rest) { DQ_HIP_OK(hipStreamWaitEvent(c.s, ev_rest, 0)); wait_rest = false; c.owner->side_used = false; }
  if (p.wide_mid) {
    DQ_TRY(mid_forward_wide(c, rope, cur));
  } else {
    if (!lp.dn[L - 1].post_w) DQ_TRY(launch_fold(cur, c.w(a.mid_in), B, RT, p.mid_c, 1, 0, c.s));
    DQ_TRY(mid_forward(c, rope, skip_ms1, lp.prep_ok));
    if (!lp.up[0].in_folded) DQ_TRY(launch_fold(c.w(a.mid2.out), c.w(a.mid_back), B, RT, p.mid_c, 0, 0, c.s));
  }
  // ---- up path (unet1d.py:1150-1158)
  cur = c.w(a.mid_back);
  for (int ui = 0; ui < L; ++ui) {
    const LevelP& l = p.ups[ui];
    const LevelBuf& b = a.ups[ui];
    const LevelForm& f = lp.up[ui];
    const int lv = L - 1 - ui;
    const int cx = l.r0.cout, cs = l.r0.cin - l.r0.cout;
    if (f.kind == LEVEL_TINY) {
      DQ_TRY(launch_tiny_fwd(tiny_desc(c, lp, true, ui), c.s));
    } else if (f.kind == LEVEL_KERNEL) {
      DQ_TRY(launch_level_fwd(level_desc(c, up_call(p, a, ui), f.img), c.s));
    } else {
      DQ_TRY(res_fwd(c, l.r0, b.r0, cur, cx, c.w(a.downs[lv].la), cs, R, l.n, RT));
      DQ_TRY(res_fwd(c, l.r1, b.r1, c.w(b.r0.out), cx, c.w(a.downs[lv].r0.out), cs, R, l.n, RT));
    }
    if (!f.la) DQ_TRY(la_fwd(c, l.la, c.w(b.r1.out), c.w(b.la), c.save ? c.w(b.la_pre) : nullptr, R, l.n, lp.prep_ok ? L + ui : -1));
    if (!f.resample) continue;  // the next launch applies this level's Upsample / k3 conv itself
    DQ_TRY(conv_plain_fwd(c, l.resample, l.last ? CONV_S1 : CONV_UP, c.w(b.la), c.w(b.rs), R, l.n, l.n_next));
    cur = c.w(b.rs);
  }
  // ---- head (unet1d.py:1160-1166)
  LevelCall lh = up_call(p, a, L);
  if (lp.head_train && c.head_loss) {
    // train step: final_conv, loss and d fin.out in the final block's launch (its output IS stored)
    lh.head = &p.final_conv;
    LevelFwd f = level_desc(c, lh, lp.up[L].img);
    Ctx::HeadLoss& hl = *c.head_loss;
    f.loss_z = hl.z; f.grad_out = hl.grad_out; f.dout = c.g(a.fin.out); f.loss_part = hl.part; f.loss_gscale = hl.gscale; f.loss_parts_out = &hl.nparts;
    f.vt_x0 = hl.x0; f.vt_ab = hl.alpha_bars; f.vt_t = hl.t; f.vt_lw = hl.lw; f.vt_tm = hl.tm; f.vt_ta = hl.ta;
    DQ_TRY(launch_level_fwd(f, c.s));
    hl.done = true;
    return 0;
  }
  if (!c.save && lp.head_shape) {  // inference: final_conv (and, while sampling, the DDIM update) in the final block's launch; its output is not stored
    lh.head = &p.final_conv; lh.eps_out = out; lh.write_out[0] = false;
    if (c.step_io && c.step_io->x_t) c.step_io->fused_update = true;
    return launch_level_fwd(level_desc(c, lh, lp.up[L].img), c.s);
  }
  if (lp.up[L].kind == LEVEL_KERNEL) DQ_TRY(launch_level_fwd(level_desc(c, lh, lp.up[L].img), c.s));
  else DQ_TRY(res_fwd(c, p.fin, a.fin, cur, p.dim, c.w(a.h0), p.dim, R, p.mz, RT));
  return conv_plain_fwd(c, p.final_conv, CONV_S1, c.w(a.fin.out), out, R, p.mz, p.mz, -1, p.final_act == FINAL_SOFTPLUS ? ACT_SOFTPLUS : ACT_NONE);
}

int unet_backward(const Ctx& c_in, const float* rope, const float* init_cond, float cm, float ca, const DevTables& dt,
                  const float* grad_out, float* grad_x) {
  BwdQueues queues;
  const Ctx c = bwd_open(c_in, queues);
  std::vector<ResWgReduce>& wg_items = queues.wg;
  if (c.loss_sum.out) {
    const Ctx::LossSum ls = c.loss_sum;
    DQ_TRY(on_side(c, true, [ls](hipStream_t ss) { return launch_sum_partials(ls.partials, ls.count, ls.scale, ls.out, ss); }));
  }
  const Plan& p = c.p;
  const Arena& a = c.ar;
  const int B = c.B, RT = c.RT, R = B * RT, L = p.levels;
  const LevelPlan lp = level_plan(p, a, B, RT, true, true);  // (what the forward of this step built with save: the same levels took the same launches)
  DQ_TRY(bwd_clear_twin(c));
  // the ResnetBlock / resample-conv slot reductions collected so far as one side-stream item
  auto wg_to_side = [&c, &wg_items]() -> int {
    const bool wg_off = DQ_DEV_FLAG("DQ_NO_LA_FLUSH_SIDE", '1');  // (dev switch)
    if (wg_items.empty() || !side_open(c, !wg_off && tail_fork_enabled())) return 0;  // (else they stay for the end of the pass)
    std::vector<ResWgReduce> part;
    part.swap(wg_items);
    return on_side(c, true, [part](hipStream_t ss) { return res_wg_reduce_all(part, ss); });
  };
  // the two levels with rows of one position: their backward data path in one launch each (k_tiny.hip), when their forward ran there
  // head
  // (d fin.out came with the forward's last launch when the training head ran: only the weight gradient is left)
  const bool head_done = c.head_loss && c.head_loss->done;
  const float* d_pre = grad_out;  // d loss / d (final_conv's output)
  if (p.final_act == FINAL_SOFTPLUS && !head_done) {
    // pos_output_only: grad_out is d loss / d softplus(pre) -- every loss term (the MSE, the MS1 term) has accumulated into it.  The
    // pre-activation is recomputed from fin.out; the result goes to the gradient twin of the `eps` slot, which no backward launch
    // otherwise touches (the network output's gradient is the caller's grad_out), so the caller's buffer stays as it was
    DQ_REQUIRE(p.final_conv.b >= 0, "unet_backward: the Softplus head needs final_conv's bias");
    DQ_TRY(launch_softplus_head_bwd(c.w(a.fin.out), c.prm(p.final_conv.w), c.prm(p.final_conv.b), p.final_conv.cin, grad_out, c.g(a.eps), R,
                                    p.mz, c.s));
    d_pre = c.g(a.eps);
  }
  DQ_TRY(conv_plain_bwd(c, p.final_conv, CONV_S1, c.w(a.fin.out), d_pre, head_done ? nullptr : c.g(a.fin.out), R, p.mz, p.mz, 0));
  const LevelBuf& lastup = a.ups[L - 1];
  DQ_TRY(res_bwd(c, p.fin, a.fin, c.w(lastup.rs), c.g(lastup.rs), p.dim, c.w(a.h0), c.g(a.h0), p.dim, R, p.mz, RT, 1, 1));  // first writers of d rs, d h0
  // up path, reversed
  for (int ui = L - 1; ui >= 0; --ui) {
    const LevelP& l = p.ups[ui];
    const LevelBuf& b = a.ups[ui];
    const int lv = L - 1 - ui;
    const int cx = l.r0.cout, cs = l.r0.cin - l.r0.cout;
    const int64_t in_off = ui == 0 ? a.mid_back : a.ups[ui - 1].rs;
    if (ui == 0 && lp.use_tb_up && lp.tb_up_w)  // (the tiny backward applies Upsample^T itself: only the conv's weight / bias gradient is left, on the side stream)
      DQ_TRY(conv_plain_bwd(c, l.resample, CONV_UP, c.w(b.la), c.g(b.rs), nullptr, R, l.n, l.n_next, 0));
    else
      DQ_TRY(resample_bwd(c, l.resample, l.last ? LEVEL_PRE_S1 : LEVEL_PRE_UP, b, l.n, l.n_next, 0));  // only writer of d la (up): store
    if (ui == 0 && lp.use_tb_up) {
      DQ_TRY(tiny_bwd_run(c, tiny_bwd_desc(c, true, lp.tb_up_w), true));  // LinearAttention + both ResnetBlocks; the input gradient lands in the bottleneck's layout
    } else {
      DQ_TRY(la_bwd(c, l.la, b, c.w(b.r1.out), c.g(b.la), c.g(b.r1.out), R, l.n, lp.prep_ok ? L + ui : -1));
      // the up path is the first writer of its own tensors AND of the skip tensors (the down path accumulates into them later)
      DQ_TRY(res_bwd(c, l.r1, b.r1, c.w(b.r0.out), c.g(b.r0.out), cx, c.w(a.downs[lv].r0.out), c.g(a.downs[lv].r0.out), cs, R, l.n, RT, 1, 1));
      DQ_TRY(res_bwd(c, l.r0, b.r0, c.w(in_off), c.g(in_off), cx, c.w(a.downs[lv].la), c.g(a.downs[lv].la), cs, R, l.n, RT, 1, 1));
    }
    // the resample-conv and ResnetBlock weight gradients of two levels behind one event: an event record holds the main queue for ~6 us
    // (kernel trace)
    if (side_flush_here(lv)) DQ_TRY(side_flush(c));
  }
  // bottleneck
  if (p.wide_mid) {
    DQ_TRY(mid_backward_wide(c, rope));
  } else {
    if (!lp.use_tb_up) DQ_TRY(launch_fold(c.g(a.mid_back), c.g(a.mid2.out), B, RT, p.mid_c, 1, 1, c.s));  // (the tiny backward wrote d mid2.out itself)
    DQ_TRY(mid_backward(c, rope, grad_x != nullptr, lp.prep_ok));
    if (!lp.use_tb_dn) DQ_TRY(launch_fold(c.g(a.mid_in), c.g(a.downs[L - 1].rs), B, RT, p.mid_c, 0, 0, c.s));  // first and only writer: store (the tiny backward reads d mid_in itself)
  }
  // MS1 feature path (unet1d.py:1120-1130): its gradient d ms1f is final behind the bottleneck (to_k is its only consumer) and nothing on
  // the main chain reads what it produces -- data path and weight gradients go to the side stream with the next flush, instead of standing
  // at the end of the pass in front of the join (~24 us of the main queue and ~35 us of the side queue's tail)
  auto ms1_bwd = [&p, &a, B, RT](const Ctx& cc) -> int {
    DQ_TRY(conv_plain_bwd(cc, p.ms1_c1, CONV_S1, cc.w(a.ms1_a), cc.g(a.ms1f), cc.g(a.ms1_a), B, RT, RT, 0));
    BlockBwd gb;
    gb.u = cc.w(a.ms1_u); gb.dy = cc.g(a.ms1_a); gb.du = cc.g(a.ms1_u); gb.C = p.cond_dim; gb.rows = B; gb.n = RT; gb.rows_per_sample = 1;
    gb.act = ACT_GELU;
    DQ_TRY(launch_block_bwd(gb, cc.s));
    if (p.ms1_channels > 1) {  // weight / bias gradient from the (B, RT, M1) conditioning the forward kept (no gradient with respect to MS1)
      Ms1FeatWgrad w;
      w.ms1n = cc.w(a.ms1n); w.du = cc.g(a.ms1_u); w.dw = cc.dprm(p.ms1_c0.w); w.dbias = cc.dprm(p.ms1_c0.b);
      w.part = cc.w(a.ms1_wpart); w.part_floats = a.ms1_wpart_floats; w.B = B; w.RT = RT; w.M1 = p.ms1_channels;
      return launch_ms1_feat_wgrad(w, cc.s);
    }
    return conv_plain_bwd(cc, p.ms1_c0, CONV_S1, cc.w(a.ms1n), cc.g(a.ms1_u), nullptr, B, RT, RT, 0);
  };
  DQ_TRY(on_side(c, tail_fork_enabled(), ms1_bwd));
  // down path, reversed
  for (int lv = L - 1; lv >= 0; --lv) {
    const LevelP& l = p.downs[lv];
    const LevelBuf& b = a.downs[lv];
    const int C = l.r0.cin;
    const int64_t in_off = lv == 0 ? a.h0 : a.downs[lv - 1].rs;
    if (lv == L - 1 && lp.use_tb_dn) {  // k3 conv, LinearAttention, both ResnetBlocks and the Downsample in front of the level: one launch
      DQ_TRY(tiny_bwd_run(c, tiny_bwd_desc(c, false, false), false));
      if (side_flush_here(lv)) DQ_TRY(side_flush(c));
      continue;
    }
    if (!(lv == L - 2 && lp.use_tb_dn))  // (that Downsample's backward rode in the launch above)
      DQ_TRY(resample_bwd(c, l.resample, l.last ? LEVEL_PRE_S1 : LEVEL_PRE_DOWN, b, l.n, l.n_next, 1));
    if (lv == 0) DQ_TRY(side_flush(c));  // (last level: the resample conv's weight gradient under the LinearAttention backward, not in the tail)
    DQ_TRY(la_bwd(c, l.la, b, c.w(b.r1.out), c.g(b.la), c.g(b.r1.out), R, l.n, lp.prep_ok ? lv : -1));
    DQ_TRY(res_bwd(c, l.r1, b.r1, c.w(b.r0.out), c.g(b.r0.out), C, nullptr, nullptr, 0, R, l.n, RT));
    // (the last level's weight gradients are the tail of the side stream, in front of the join: hand them over block by block, so that
    // r1's run under r0's data path instead of behind it)
    if (lv == 0) DQ_TRY(side_flush(c));
    DQ_TRY(res_bwd(c, l.r0, b.r0, c.w(in_off), c.g(in_off), C, nullptr, nullptr, 0, R, l.n, RT, lv > 0 ? 1 : 0, 0));  // (d h0 has the final block's part already)
    // (a second early flush in front of the last level measured neutral at batch 32 and +25 us at batch 1 / 4, where the host's launch count is the limit)
    if (lv == 2 && p.mz <= 64) {  // (short rows only: the sweep kernels of longer rows use the whole slot buffer per layer)
      DQ_TRY(la_flush_side(c));
      // the ResnetBlock / resample-conv slot reductions collected so far ride along (every block has its own slots and its own parameters)
      DQ_TRY(wg_to_side());
    }
    if (side_flush_here(lv)) DQ_TRY(side_flush(c));
  }
  // init conv + mixture conditioning: d h0 is final here and only d(scale, shift) of init_cond_proj (read by the time-embedding backward
  // behind the join) and the init_conv weight gradient depend on it -- on the side stream when nobody asked for d loss / d x, under the
  // LinearAttention / ResnetBlock slot reductions of the main stream
  auto init_bwd = [&p, &a, init_cond, cm, ca, B, RT, R](const Ctx& cc) -> int {
    DQ_TRY(conv_plain_bwd(cc, p.init_conv, CONV_S1, cc.w(a.cat0), cc.g(a.h0), cc.g(a.cat0), R, p.mz, p.mz, 0));
    return launch_prep_inputs_bwd(cc.g(a.cat0), init_cond, cm, ca, cc.g(a.ss), p.ss_total, p.ss_init, B, RT, p.mz, cc.w(a.bb_part),
                                  a.bb_part_floats, cc.s);
  };
  const bool tail_swap = !DQ_DEV_FLAG("DQ_NO_TAIL_SWAP", '1');  // (dev switch)
  if (side_open(c, tail_swap && !grad_x && tail_fork_enabled())) {
    // The chain that ends the pass is  d h0 -> d cat0 (init conv, data) -> d(scale, shift) of init_cond_proj -> time-embedding backward -> norm -> update;
    // the LinearAttention slot reductions and the init conv's weight gradient only have to be there for the norm.  So the MAIN queue runs that chain and
    // the side queue those (they stood on the main queue in front of the join, the chain's first half on the side queue behind the
    // weight gradient: the main queue idled ~50 us in front of the time-embedding backward).  That backward needs the side queue only up to
    // HERE (the per-sample scale / shift sums of the ResnetBlocks): one event marks the place.
    DQ_TRY(side_flush(c));
    hipEvent_t ev_ss = nullptr;
    if (c.owner->side_used) DQ_TRY(side_mark(c, &ev_ss));
    DQ_TRY(conv_plain_bwd(c, p.init_conv, CONV_S1, c.w(a.cat0), c.g(a.h0), nullptr, R, p.mz, p.mz, 0));  // (weight gradient only: queued)
    DQ_TRY(la_flush_side(c));
    DQ_TRY(side_flush(c));
    // (the ResnetBlock slot reduce stays on this queue: it also forms those blocks' per-sample d(scale, shift), which the time-embedding backward reads)
    DQ_TRY(conv_plain_bwd(c, p.init_conv, CONV_S1, c.w(a.cat0), c.g(a.h0), c.g(a.cat0), R, p.mz, p.mz, 0, -1, false));
    // (the wait stands in front of the input affine's backward already: its partial-sum scratch is the PreNorm backward's, whose reduce is on the side queue)
    if (ev_ss) DQ_HIP_OK(hipStreamWaitEvent(c.s, ev_ss, 0));
    DQ_TRY(launch_prep_inputs_bwd(c.g(a.cat0), init_cond, cm, ca, c.g(a.ss), p.ss_total, p.ss_init, B, RT, p.mz, c.w(a.bb_part), a.bb_part_floats,
                                  c.s));
    DQ_TRY(la_flush(c));  // (nothing left unless DQ_NO_LA_FLUSH_SIDE)
    DQ_TRY(res_wg_reduce_all(wg_items, c.s));
    DQ_TRY(launch_time_embed_bwd(p, dt, c.P, c.dP, c.w(a.tbuf), c.g(a.ss), B, c.s));
    return join_side(c);
  }
  DQ_TRY(on_side(c, !grad_x && tail_fork_enabled(), init_bwd));
  if (grad_x) {
    // channel 1 of d(cat0) is d loss / d x
    DQ_HIP_OK(hipMemcpy2DAsync(grad_x, sizeof(float) * p.mz, c.g(a.cat0) + p.mz, sizeof(float) * 2 * p.mz, sizeof(float) * p.mz, R,
                               hipMemcpyDeviceToDevice, c.s));
  }
  DQ_TRY(bwd_close(c, queues));
  // time embedding: all scale/shift heads + the MLP -- after the join: the per-sample d(scale, shift) of the fused ResnetBlocks are
  // summed on the side stream
  return launch_time_embed_bwd(p, dt, c.P, c.dP, c.w(a.tbuf), c.g(a.ss), B, c.s);
}

// The step-invariant part of a sampling call (dq_sampler.hip), once in front of its steps: the once-per-parameter-state launches, the MS1
// feature path (unet1d.py:1120-1130), to_k and RoPE(k) (:555, 561) depend on neither t nor x_t.  unet_forward skips them under StepIO::prologue.
int unet_sample_prologue(const Ctx& c, const float* ms1, float cm, float ca, const float* rope, bool* ran) {
  const Plan& p = c.p;
  const Arena& a = c.ar;
  *ran = false;
  if (p.wide_mid) return 0;  // (the wide bottleneck keeps its projections inside the step, and prepares there)
  const LevelPlan lp = level_plan(p, a, c.B, c.RT, false, false);
  DQ_TRY(unet_prepare(c, lp, c.s));  // W2 / operand images / the aligned copy of to_k's weight for the GEMM route
  DQ_TRY(ms1_features(c, ms1, cm, ca, true, c.s));
  DQ_TRY(conv_plain_fwd(c, proj(p.k_w, HID, p.cond_dim), CONV_S1, c.w(a.ms1f), c.w(a.kk), c.B, c.RT, c.RT, lp.prep_ok ? 1 : -1));
  if (rope) DQ_TRY(launch_rope(c.w(a.kk), rope, c.B, (int64_t)HID * c.RT, c.RT, 1.f, c.s));
  *ran = true;
  return 0;
}

// Lays out the arena for (B, RT) and, on the first call of a plan, uploads the ~10 KB offset tables of the scale/shift
// heads (the only device allocation the library ever makes; dq_plan_create itself never touches the GPU).
int ensure_arena(dq_plan* plan, int B, int RT) {
  if (plan->arena.B != B || plan->arena.RT != RT) layout_arena(plan->plan, B, RT, plan->arena);
  return ensure_dev_tables(plan);
}

// the offset tables alone (dq_debug_time_fwd / _bwd run the time-embedding launches without an arena)
int ensure_dev_tables(dq_plan* plan) {
  if (!plan->dev.ss_w_off) {
    const Plan& p = plan->plan;
    std::vector<int64_t> woff(p.ss_total), boff(p.ss_total);
    for (const auto& l : p.ss_lins)
      for (int r = 0; r < l.rows; ++r) {
        woff[l.ss_off + r] = l.w + (int64_t)r * p.time_dim;
        boff[l.ss_off + r] = l.b + r;
      }
    DQ_HIP_OK(hipMalloc(&plan->dev.ss_w_off, sizeof(int64_t) * p.ss_total));
    DQ_HIP_OK(hipMalloc(&plan->dev.ss_b_off, sizeof(int64_t) * p.ss_total));
    DQ_HIP_OK(hipMemcpy(plan->dev.ss_w_off, woff.data(), sizeof(int64_t) * p.ss_total, hipMemcpyHostToDevice));
    DQ_HIP_OK(hipMemcpy(plan->dev.ss_b_off, boff.data(), sizeof(int64_t) * p.ss_total, hipMemcpyHostToDevice));
  }
  return 0;
}

}  // namespace dq

using namespace dq;

extern "C" {

// The LevelPlan a pass at (B, RT) builds: the SAME level_plan() call as unet_forward (save, twin as the pass has them), unet_backward (1, 1)
// and the sampler's prologue (0, 0), on an arena laid out as dq_unet_workspace_bytes lays it out -- no workspace, no launch, no device.
int dq_debug_level_plan(dq_plan* plan, int B, int RT, int save, int twin, int32_t* out, int cap) {
  if (!plan || !out || B <= 0 || RT <= 0) return -1;
  const int L = plan->plan.levels;
  const int need = 1 + DQ_LEVEL_PLAN_FORM_INTS * (2 * L + 1) + DQ_LEVEL_PLAN_FLAG_INTS;
  if (cap < need) return -1;
  Arena a;
  layout_arena(plan->plan, B, RT, a);
  const LevelPlan lp = level_plan(plan->plan, a, B, RT, save != 0, twin != 0);
  static_assert(LEVEL_UNFUSED == DQ_LEVEL_UNFUSED && LEVEL_KERNEL == DQ_LEVEL_KERNEL && LEVEL_TINY == DQ_LEVEL_TINY, "LevelKind mirrors include/dq_hip.h");
  int n = 0;
  out[n++] = L;
  auto put = [&](const LevelForm& f) {
    out[n++] = f.kind; out[n++] = f.img; out[n++] = f.la; out[n++] = f.post_w; out[n++] = f.in_folded; out[n++] = f.resample;
  };
  for (int lv = 0; lv < L; ++lv) put(lp.dn[lv]);
  for (int ui = 0; ui <= L; ++ui) put(lp.up[ui]);
  for (bool b : {lp.prep_ok, lp.init_fused, lp.head_shape, lp.head_train, lp.use_tb_up, lp.use_tb_dn, lp.tb_up_w}) out[n++] = b;
  return n;
}

// Lays the plan's cached arena out for (B, RT), as the first pass at that shape would (host only: no device table is uploaded here), so that
// dq_debug_tensor_offset answers for the shape before any call at it -- a caller of dq_debug_mid_fwd fills workspace slots first.
int dq_debug_layout(dq_plan* plan, int B, int RT) {
  if (!plan || B <= 0 || RT <= 0) return -1;
  if (plan->arena.B != B || plan->arena.RT != RT) layout_arena(plan->plan, B, RT, plan->arena);
  return 0;
}

// What mid_forms() answers for a pass at (B, RT) -- the function mid_forward / mid_backward ask --, on a local arena laid out as
// dq_unet_workspace_bytes lays it out, with the few plan constants a caller of the two entries below needs: no workspace, no launch, no
// device, no change of the plan.
int dq_debug_mid_forms(dq_plan* plan, int B, int RT, int32_t* out, int cap) {
  if (!plan || !out || B <= 0 || RT <= 0 || cap < DQ_MID_FORMS_INTS) return -1;
  const Plan& p = plan->plan;
  Arena a;
  layout_arena(p, B, RT, a);
  MidForms mf{false, false, false};
  if (!p.wide_mid) mf = mid_forms(p, a, B, RT);
  int n = 0;
  out[n++] = mf.qkv_fused; out[n++] = mf.out_fused; out[n++] = mf.pre_fused; out[n++] = p.wide_mid; out[n++] = p.mid_c; out[n++] = p.cond_dim;
  out[n++] = level_plan(p, a, B, RT, false, false).prep_ok;  // (depends on the plan alone: the same for every pass)
  out[n++] = p.mid1.ss_off; out[n++] = p.mid2.ss_off; out[n++] = p.ss_total;
  static_assert(DQ_MID_FORMS_INTS == 10, "dq_debug_mid_forms writes DQ_MID_FORMS_INTS ints");
  return n;
}

// The bottleneck alone, forward: the time embedding (tbuf and every scale / shift head), then -- unless skip_ms1, as in unet_forward, where
// the sampler's prologue has done it -- unet_prepare (of which the narrow bottleneck reads the aligned copies of the attention's projection
// weights; the level and tiny operand images it also writes belong to launches these entries never make), then the bottleneck as
// unet_forward calls it.  Narrow (dq_debug_mid_fwd): mid_forward on the mid_in / ms1f the caller wrote into their workspace slots; skip_ms1:
// the rotated kk too is the caller's, and a call without skip_ms1 has run on this workspace with these parameters before (the prepared
// weight slots are its).  Wide (dq_debug_wide_mid_fwd): mid_forward_wide on the last down level's output, folds included.
static int debug_mid_fwd(const char* who, bool wide, dq_plan* plan, const float* params, const float* rope_freqs, const int64_t* t,
                         int save_for_bwd, int skip_ms1, void* workspace, int64_t workspace_bytes, int B, int RT, void* stream) {
  const std::string w(who);
  DQ_REQUIRE(plan && params && t && workspace, w + ": null argument");
  DQ_REQUIRE(B > 0 && RT > 0, w + ": B and RT must be positive");
  DQ_REQUIRE(plan->plan.wide_mid == wide, w + (wide ? ": the narrow bottleneck (16 / 32 channels) is not this entry's"
                                                    : ": the wide bottleneck (k_wide.hip) is not this entry's"));
  Arena probe;
  layout_arena(plan->plan, B, RT, probe);
  DQ_REQUIRE(workspace_bytes >= (int64_t)sizeof(float) * probe.floats, w + ": workspace too small");
  DQ_TRY(ensure_arena(plan, B, RT));
  Ctx c{plan->plan, plan->arena, params, (float*)workspace, nullptr, nullptr, B, RT, (hipStream_t)stream};
  c.save = save_for_bwd != 0;
  const LevelPlan lp = level_plan(c.p, c.ar, B, RT, c.save, false);
  DQ_TRY(launch_time_embed_fwd(c.p, plan->dev, c.P, t, 0, c.w(c.ar.tbuf), c.w(c.ar.ss), B, nullptr, nullptr, c.s));
  if (!skip_ms1) DQ_TRY(unet_prepare(c, lp, c.s));
  if (wide) return mid_forward_wide(c, rope_freqs, c.w(c.ar.downs[c.p.levels - 1].rs));
  return mid_forward(c, rope_freqs, skip_ms1 != 0, lp.prep_ok);
}

// The bottleneck alone, backward: the gradient of the bottleneck's output is what the caller wrote into the twin (narrow: of mid2; wide: of
// mid_back); everything else of the twin's accumulated-into region is cleared, as unet_backward clears it; then mid_backward /
// mid_backward_wide inside unet_backward's scaffolding (bwd_open / bwd_close), with the side queue (grad_x_mode 0) or all on the caller's
// stream (1).  No time-embedding backward, no MS1 path: the twin keeps d mid_in (wide: d of the last down level's output), d ms1f and, in
// the twin of ss, both blocks' per-sample d(scale, shift); grads receives += of the bottleneck's parameter gradients.
static int debug_mid_bwd(const char* who, bool wide, dq_plan* plan, const float* params, const float* rope_freqs, float* grads,
                         int grad_x_mode, void* workspace, int64_t workspace_bytes, int B, int RT, void* stream) {
  const std::string w(who);
  DQ_REQUIRE(plan && params && grads && workspace, w + ": null argument");
  DQ_REQUIRE(B > 0 && RT > 0, w + ": B and RT must be positive");
  DQ_REQUIRE(plan->plan.wide_mid == wide, w + (wide ? ": the narrow bottleneck (16 / 32 channels) is not this entry's"
                                                    : ": the wide bottleneck (k_wide.hip) is not this entry's"));
  Arena probe;
  layout_arena(plan->plan, B, RT, probe);
  DQ_REQUIRE(workspace_bytes >= 2 * (int64_t)sizeof(float) * probe.floats, w + ": workspace too small (training=1)");
  DQ_TRY(ensure_arena(plan, B, RT));
  const Arena& a = plan->arena;
  float* W = (float*)workspace;
  Ctx c_in{plan->plan, a, params, W, W + a.floats, grads, B, RT, (hipStream_t)stream};
  // (the wide bottleneck's backward takes no grad_x: what it queues rides on the side queue whenever the pass has one)
  c_in.owner = plan->no_side || (wide && grad_x_mode) ? nullptr : plan;
  plan->twin_zeroed = nullptr;
  BwdQueues queues;
  const Ctx c = bwd_open(c_in, queues);
  const LevelPlan lp = level_plan(c.p, a, B, RT, true, true);
  DQ_TRY(bwd_clear_twin(c, wide ? a.mid_back : a.mid2.out, (int64_t)B * c.p.mid_c * RT));
  if (wide) DQ_TRY(mid_backward_wide(c, rope_freqs));
  else DQ_TRY(mid_backward(c, rope_freqs, grad_x_mode != 0, lp.prep_ok));
  return bwd_close(c, queues);
}

int dq_debug_mid_fwd(dq_plan* plan, const float* params, const float* rope_freqs, const int64_t* t, int save_for_bwd, int skip_ms1,
                     void* workspace, int64_t workspace_bytes, int B, int RT, void* stream) {
  return debug_mid_fwd("dq_debug_mid_fwd", false, plan, params, rope_freqs, t, save_for_bwd, skip_ms1, workspace, workspace_bytes, B, RT, stream);
}
int dq_debug_mid_bwd(dq_plan* plan, const float* params, const float* rope_freqs, float* grads, int grad_x_mode, void* workspace,
                     int64_t workspace_bytes, int B, int RT, void* stream) {
  return debug_mid_bwd("dq_debug_mid_bwd", false, plan, params, rope_freqs, grads, grad_x_mode, workspace, workspace_bytes, B, RT, stream);
}
int dq_debug_wide_mid_fwd(dq_plan* plan, const float* params, const float* rope_freqs, const int64_t* t, int save_for_bwd, void* workspace,
                          int64_t workspace_bytes, int B, int RT, void* stream) {
  return debug_mid_fwd("dq_debug_wide_mid_fwd", true, plan, params, rope_freqs, t, save_for_bwd, 0, workspace, workspace_bytes, B, RT, stream);
}
int dq_debug_wide_mid_bwd(dq_plan* plan, const float* params, const float* rope_freqs, float* grads, int grad_x_mode, void* workspace,
                          int64_t workspace_bytes, int B, int RT, void* stream) {
  return debug_mid_bwd("dq_debug_wide_mid_bwd", true, plan, params, rope_freqs, grads, grad_x_mode, workspace, workspace_bytes, B, RT, stream);
}

// The time embedding alone (k_time.hip), on caller buffers: the two launchers every pass calls first (forward) and last (backward), with the
// plan's head-offset tables.  No arena, no workspace.
static_assert(TBUF_FLOATS == DQ_TBUF_FLOATS && DQ_TBUF_DH_PRE + 16 == DQ_TBUF_FLOATS, "the tbuf slots of include/dq_hip.h mirror k_time.hip");
int dq_debug_time_fwd(dq_plan* plan, const float* params, const int64_t* t, int t_scalar, const int* step_tab, const int* step_ptr, float* tbuf,
                      float* ss, int B, void* stream) {
  DQ_REQUIRE(plan && params && tbuf, "dq_debug_time_fwd: null argument");
  DQ_REQUIRE(B > 0, "dq_debug_time_fwd: B must be positive");
  DQ_REQUIRE(!step_tab || step_ptr, "dq_debug_time_fwd: a step table needs the step it is read at");
  DQ_TRY(ensure_dev_tables(plan));
  return launch_time_embed_fwd(plan->plan, plan->dev, params, t, t_scalar, tbuf, ss, B, step_tab, step_ptr, (hipStream_t)stream);
}
int dq_debug_time_bwd(dq_plan* plan, const float* params, float* grads, float* tbuf, const float* dss, int B, void* stream) {
  DQ_REQUIRE(plan && params && grads && tbuf && dss, "dq_debug_time_bwd: null argument");
  DQ_REQUIRE(B > 0, "dq_debug_time_bwd: B must be positive");
  DQ_TRY(ensure_dev_tables(plan));
  return launch_time_embed_bwd(plan->plan, plan->dev, params, grads, tbuf, dss, B, (hipStream_t)stream);
}

int64_t dq_debug_tensor_offset(dq_plan* plan, const char* name) {
  if (!plan || !name) return -1;
  const Arena& a = plan->arena;
  const std::string n(name);
  if (n == "tbuf") return a.tbuf;
  if (n == "ss") return a.ss;
  if (n == "cat0") return a.cat0;
  if (n == "h0") return a.h0;
  if (n == "ms1f") return a.ms1f;
  if (n == "mid_in") return a.mid_in;
  if (n == "mid1") return a.mid1.out;
  if (n == "xn") return a.xn;
  if (n == "qv") return a.qv;
  if (n == "kk") return a.kk;
  if (n == "o") return a.o;
  if (n == "attn_out") return a.attn_out;
  if (n == "mid2") return a.mid2.out;
  if (n == "mid1.u1") return a.mid1.u1;
  if (n == "mid1.u2") return a.mid1.u2;
  if (n == "mid1.a1") return a.mid1.a1;
  if (n == "mid2.u1") return a.mid2.u1;
  if (n == "mid2.u2") return a.mid2.u2;
  if (n == "mid2.a1") return a.mid2.a1;
  if (n == "lse") return a.lse;
  if (n == "mid_back") return a.mid_back;
  if (a.P > 0) {  // the wide bottleneck's (B, channels, P) slots
    if (n == "w_mid_in") return a.w_mid_in;
    if (n == "w_xn") return a.w_xn;
    if (n == "w_qv") return a.w_qv;
    if (n == "w_o") return a.w_o;
    if (n == "w_attn_out") return a.w_attn_out;
    if (n == "w_xcol") return a.w_xcol;  // (scratch: the im2col buffer, the norm backward's sums, the GEMM's partial products)
    if (n == "w_stats") return a.w_stats;
    if (n == "w_gemm_part") return a.w_gemm_part;
    for (int i = 0; i < 2; ++i) {
      const WideResBuf& w = i ? a.wmid2 : a.wmid1;
      const std::string k = i ? "wmid2" : "wmid1";
      if (n == k) return w.out;
      if (n == k + ".u1") return w.u1;
      if (n == k + ".a1") return w.a1;
      if (n == k + ".u2") return w.u2;
    }
  }
  if (n == "@twin") return a.floats;  // the gradient twin G starts this many floats behind the workspace's start (a training workspace)
  if (n == "fin") return a.fin.out;
  if (n == "eps") return a.eps;  // (its gradient twin: d loss / d final_conv's output when the Softplus head's backward ran)
  for (int i = 0; i < (int)a.downs.size(); ++i) {
    if (n == "down" + std::to_string(i)) return a.downs[i].rs;
    if (n == "down" + std::to_string(i) + ".r0") return a.downs[i].r0.out;
    if (n == "down" + std::to_string(i) + ".r1") return a.downs[i].r1.out;
    if (n == "down" + std::to_string(i) + ".la") return a.downs[i].la;
    if (n == "up" + std::to_string(i)) return a.ups[i].rs;
    if (n == "up" + std::to_string(i) + ".r0") return a.ups[i].r0.out;
    if (n == "up" + std::to_string(i) + ".r1") return a.ups[i].r1.out;
    if (n == "up" + std::to_string(i) + ".la") return a.ups[i].la;
  }
  return -1;
}

}  // extern "C"
