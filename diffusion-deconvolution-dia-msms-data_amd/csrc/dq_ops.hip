// The op wrappers of the U-Net's host side -- ResnetBlock, LinearAttention, the convs, the wide bottleneck's block ops: each knows a Ctx and
// nothing of the walk -- and the side queue they issue their weight gradients on (dq_ops.h).  The network (dq_unet.hip) and the stand-alone op
// entry points of the C ABI (dq_ops_api.hip) call them.
#include "dq_dev.h"
#include "dq_tfm.h"
#include "dq_ops.h"

#include <array>

namespace dq {

// ---------------------------------------------------------------------------------------------------------------
// the side queue.  The weight-gradient kernels depend only on tensors that are final when they are issued (dU, forward activations) and
// nothing on the data-gradient chain depends on them: they run on a side stream, forked by an event, joined at the end.
// ---------------------------------------------------------------------------------------------------------------
namespace {
int ensure_side(dq_plan* pl) {
  if (pl->side_stream) return 0;
    // Own priority class => own hardware queue.  Normal-priority streams share a small round-robin pool of HSA queues,
    // and once RCCL has taken its streams from that pool a plain stream can land on the caller's queue, which serialises
    // the weight-gradient kernels behind the main chain (measured: 15.7 vs 13.0 ms/step under torch.distributed.run).
    int prio_least = 0, prio_greatest = 0;
    DQ_HIP_OK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    // LOWEST priority since round 4: the side queue carries what the main chain does not wait for, so it should fill the main queue's gaps, not take
    // compute units from it (three same-call pairs at batch 32: 3.695 / 3.681 / 3.679 ms against 3.697 / 3.696 / 3.954 with the highest priority, whose
    // occasional slow run is the side queue's kernels winning the arbitration against a resident-round grid of the main chain).  Either class is a
    // queue of its own.  DQ_SIDE_PRIO=h: the old setting (A-B switch).
    const bool low = !DQ_DEV_FLAG("DQ_SIDE_PRIO", 'h');  // (dev switch)
    DQ_HIP_OK(hipStreamCreateWithPriority(&pl->side_stream, hipStreamNonBlocking, low ? prio_least : prio_greatest));
    for (auto& e : pl->events) DQ_HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return 0;
}
}  // namespace
int fork_side(const Ctx& c) {
  dq_plan* pl = c.owner;
  DQ_TRY(ensure_side(pl));
  hipEvent_t ev = pl->events[pl->ev_next++ % dq_plan::NUM_EVENTS];
  DQ_HIP_OK(hipEventRecord(ev, c.s));
  DQ_HIP_OK(hipStreamWaitEvent(pl->side_stream, ev, 0));
  pl->side_used = true;
  return 0;
}
int side_mark(const Ctx& c, hipEvent_t* ev) {
  dq_plan* pl = c.owner;
  *ev = pl->events[pl->ev_next++ % dq_plan::NUM_EVENTS];
  DQ_HIP_OK(hipEventRecord(*ev, pl->side_stream));
  return 0;
}

// a bare launch: fn(the side stream) behind the flush, or fn(c.s) now
int on_side(const Ctx& c, bool allowed, std::function<int(hipStream_t)> fn, bool forks) {
  if (!side_open(c, allowed)) return fn(c.s);
  c.side_defer->push_back(Ctx::SideFn{std::move(fn), forks});
  return 0;
}
// a piece of the pass: body(a copy of c without owner / queue whose stream is the side stream) behind the flush -- everything it launches,
// its weight gradients included, stays on that stream --, or body(c) now
int on_side(const Ctx& c, bool allowed, const std::function<int(const Ctx&)>& body) {
  if (!side_open(c, allowed)) return body(c);
  Ctx side = c;
  side.owner = nullptr; side.side_defer = nullptr;
  c.side_defer->push_back(Ctx::SideFn{[side, body](hipStream_t ss) mutable { side.s = ss; return body(side); }, true});
  return 0;
}

// (a context with an owner always has the queue: unet_backward installs it, and what the queue runs has neither)
int wgrad_async(const Ctx& c, const ConvWgrad& w) {
  return on_side(c, true, [w](hipStream_t s) { return launch_conv_wgrad(w, s); });
}

int wgrad_async_multi(const Ctx& c, ConvWgrad* w, int count) {
  DQ_REQUIRE(count >= 1 && count <= 3, "wgrad_async_multi: one to three convs");
  std::array<ConvWgrad, 3> ws;
  std::copy(w, w + count, ws.begin());
  return on_side(c, true, [ws, count](hipStream_t s) { return launch_conv_wgrad_multi(ws.data(), count, s); });
}

// issue the queued side-stream work behind one event recorded now on the main stream
int side_flush(const Ctx& c) {
  dq_plan* pl = c.owner;
  if (!pl || !c.side_defer || c.side_defer->empty()) return 0;
  std::vector<Ctx::SideFn> items;
  items.swap(*c.side_defer);  // (nothing an item calls can re-enter the queue)
  bool forked = false;
  for (Ctx::SideFn& it : items) {
    if (it.forks && !forked) { DQ_TRY(fork_side(c)); forked = true; }  // one event for the whole group (creates the stream on first use)
    DQ_TRY(it.fn(pl->side_stream ? pl->side_stream : c.s));  // (no side stream yet: only in front of a group's first forking item)
  }
  return 0;
}

namespace {
// test hook (dq_debug_side_tail_store): the LAST thing the side stream does before the join is a delayed store -- a caller whose next
// launch on its own stream sees the value has proof that dq_train_step / dq_unet_bwd order the side stream in front of their return
__global__ void k_debug_delay_store(float* addr, float value, long long ticks) {
  const long long t0 = wall_clock64();  // (100 MHz; the loop ends after `ticks` whatever the data)
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  *addr = value;
}
}  // namespace

int join_side(const Ctx& c) {
  dq_plan* pl = c.owner;
  if (!pl || !pl->side_used) return 0;
  if (pl->debug_tail_addr) {
    hipLaunchKernelGGL(k_debug_delay_store, dim3(1), dim3(1), 0, pl->side_stream, pl->debug_tail_addr, pl->debug_tail_value, (long long)pl->debug_tail_us * 100);
    DQ_LAUNCH_CHECK();
  }
  hipEvent_t ev = pl->events[pl->ev_next++ % dq_plan::NUM_EVENTS];
  DQ_HIP_OK(hipEventRecord(ev, pl->side_stream));
  DQ_HIP_OK(hipStreamWaitEvent(c.s, ev, 0));
  pl->side_used = false;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// ResnetBlock
// ---------------------------------------------------------------------------------------------------------------
// the collected ResnetBlock / resample-conv slot reductions (one launch for the network's <= 32 such blocks)
int res_wg_reduce_all(const std::vector<ResWgReduce>& items, hipStream_t s) {
  for (size_t i = 0; i < items.size(); i += RES_WG_REDUCE_MAX)
    DQ_TRY(launch_res_wg_reduce(items.data() + i, (int)std::min<size_t>(RES_WG_REDUCE_MAX, items.size() - i), s));
  return 0;
}

// a ResnetBlock's operands but its first input (what a block of the level kernel reads): the second input (skip channels), the parameters and
// where its results go (wpart: the backward recomputes a1)
ResFwd level_block(const Ctx& c, const ResP& r, const ResBuf& b, const float* inB, int cinB, bool write_out) {
  ResFwd k;
  k.inB = cinB ? inB : nullptr; k.cinB = cinB;
  res_operands(c, r, k);
  if (c.save) { k.u1 = c.w(b.u1); k.a1 = b.wpart_floats ? nullptr : c.w(b.a1); k.u2 = c.w(b.u2); }
  k.out = (write_out || c.save) ? c.w(b.out) : nullptr;
  return k;
}

// ResnetBlock forward (unet1d.py:302-323): input = cat(A, B)
// qkv / aout: the attention's front rides behind the block / its back in front of it (k_res_rt.hip; the caller checked for RES_FWD_RT)
int res_fwd(const Ctx& c, const ResP& r, const ResBuf& b, const float* inA, int cinA, const float* inB, int cinB, int rows, int n,
            int rows_per_sample, const ResRtQkv* qkv, const ResRtOut* aout) {
  const ResFwdForm form = res_fwd_form(r.cout, cinA, cinB, r.res.cout != 0, rows, n, rows_per_sample);
  DQ_REQUIRE(form == RES_FWD_RT || (!qkv && !aout), "res_fwd: the attention front / back needs the fused 16-channel block");
  if (form != RES_FWD_UNFUSED) {  // one fused launch
    ResFwd k = level_block(c, r, b, inB, cinB, /*write_out=*/true);
    if (form == RES_FWD_LEVEL) {  // one block of the level kernel, no input stage
      LevelFwd f;
      f.params = c.P; f.in = inA; f.pre = LEVEL_PRE_NONE; f.nblocks = 1; f.blk[0] = k;
      f.C = r.cout; f.rows = rows; f.n = n; f.rows_per_sample = rows_per_sample;
      return launch_level_fwd(f, c.s);
    }
    k.inA = inA; k.cinA = cinA;
    k.C = r.cout; k.rows = rows; k.n = n; k.rows_per_sample = rows_per_sample;
    if (qkv || aout) return launch_res_rt_fwd(k, c.s, qkv, aout);
    return launch_res_fwd(k, c.s);
  }
  DQ_REQUIRE(b.a1 != b.u1, "res_fwd: a block laid out for the fused weight-gradient backward has no a1 tensor (cat(x, skip) with x of cout channels)");
  ConvFwd f;
  f.inA = inA; f.inB = inB; f.cinA = cinA; f.cinB = cinB;
  f.w = c.prm(r.c1.w); f.bias = c.prm(r.c1.b); f.cout = r.cout; f.K = 3; f.mode = CONV_S1;
  f.rows = rows; f.n_in = n; f.n_out = n;
  f.u_out = c.save ? c.w(b.u1) : nullptr; f.y_out = c.w(b.a1);
  f.g = c.prm(r.g1);
  f.ss = c.w(c.ar.ss) + r.ss_off; f.ss_stride = c.p.ss_total; f.rows_per_sample = rows_per_sample;
  f.act = ACT_SILU;
  DQ_TRY(launch_conv_fwd(f, c.s));
  ConvFwd f2;
  f2.inA = c.w(b.a1); f2.cinA = r.cout;
  f2.w = c.prm(r.c2.w); f2.bias = c.prm(r.c2.b); f2.cout = r.cout; f2.K = 3; f2.mode = CONV_S1;
  f2.rows = rows; f2.n_in = n; f2.n_out = n;
  f2.u_out = c.save ? c.w(b.u2) : nullptr; f2.y_out = c.w(b.out);
  f2.g = c.prm(r.g2); f2.act = ACT_SILU;
  f2.resA = inA; f2.resB = inB; f2.rcinA = cinA; f2.rcinB = cinB;
  if (r.res.cout) { f2.res_w = c.prm(r.res.w); f2.res_b = c.prm(r.res.b); }
  DQ_TRY(launch_conv_fwd(f2, c.s));
  return 0;
}

namespace {
// A ResnetBlock's weight-gradient launches from the d u2 / d u1 / d out tensors its data path left: conv2, conv1 and, where the block has one,
// res_conv; returns how many.  Launch i gets scratch_floats of the weight-gradient scratch at i * stride (0: each the same extent, one at a time).
int res_wgrads(const Ctx& c, const ResP& r, const ResBuf& b, const float* inA, int cinA, const float* inB, int cinB, int rows, int n,
               int64_t stride, int64_t scratch_floats, ConvWgrad w[3]) {
  ConvWgrad& w2 = w[0];
  w2.scratch = c.w(c.ar.wg); w2.scratch_floats = scratch_floats;
  w2.du = c.g(b.u2); w2.inA = c.w(b.a1); w2.cinA = r.cout; w2.cout = r.cout; w2.K = 3; w2.mode = CONV_S1;
  w2.rows = rows; w2.n_in = n; w2.n_out = n; w2.dw = c.dprm(r.c2.w); w2.dbias = c.dprm(r.c2.b);
  w[1] = w2;
  ConvWgrad& w1 = w[1];
  w1.scratch = c.w(c.ar.wg) + stride;
  w1.du = c.g(b.u1); w1.inA = inA; w1.inB = inB; w1.cinA = cinA; w1.cinB = cinB; w1.dw = c.dprm(r.c1.w); w1.dbias = c.dprm(r.c1.b);
  if (!r.res.cout) return 2;
  w[2] = w1;
  w[2].scratch = c.w(c.ar.wg) + 2 * stride;
  w[2].du = c.g(b.out); w[2].K = 1; w[2].dw = c.dprm(r.res.w); w[2].dbias = c.dprm(r.res.b);
  return 3;
}
}  // namespace

// the side-stream part of a fused ResnetBlock backward: the block's weight gradients from the d u1 / d u2 / d out tensors the data-path launch
// left, and the ordered sums of its per-workgroup [d g2 | d g1 | d scale | d shift] partials (gblocks workgroups per sample)
int res_bwd_side(const Ctx& c, const ResP& r, const ResBuf& b, const float* inA, int cinA, const float* inB, int cinB, int rows, int n,
                 int rows_per_sample, int gblocks) {
  // the block's three weight gradients (conv2, conv1, res_conv) in ONE launch + one reduce; each gets a third of the scratch
  ConvWgrad w[3];
  const int64_t third = c.ar.wg_floats / 3 / 64 * 64;
  DQ_TRY(wgrad_async_multi(c, w, res_wgrads(c, r, b, inA, cinA, inB, cinB, rows, n, third, third, w)));
  // the ordered sums of the per-block partials (norm gains, this block's d(scale), d(shift) of every sample): behind the
  // weight gradients on the side stream (which has waited for the event recorded after k_res_bwd), or on the main stream
  // without one.  The time-embedding backward, which reads d(scale, shift), runs after the join.
  if (gblocks > 0) {
    const PartReduce red = res_part_reduce(c.w(b.gpart), gblocks, rows / rows_per_sample, r.cout, c.dprm(r.g2), c.dprm(r.g1),
                                           c.g(c.ar.ss) + r.ss_off, c.p.ss_total);
    DQ_TRY(on_side(c, true, [red](hipStream_t rs) { return launch_part_reduce(red, rs); }, /*forks=*/false));
  }
  return 0;
}

// the data-path operands of a ResnetBlock backward (what res_bwd_form decides on; dq_resblock_forms asks the same question)
ResBwd res_bwd_args(const Ctx& c, const ResP& r, const ResBuf& b, float* dA, int cinA, float* dB, int cinB, int rows, int n, int rows_per_sample,
                    int storeA, int storeB) {
  ResBwd k;
  k.dout = c.g(b.out); k.u1 = c.w(b.u1); k.u2 = c.w(b.u2);
  res_operands(c, r, k);
  k.du1 = c.g(b.u1); k.du2 = c.g(b.u2); k.dA = dA; k.dB = dB; k.cinA = cinA; k.cinB = cinB;
  k.dA_store = storeA; k.dB_store = storeB;
  k.dg1 = c.dprm(r.g1); k.dg2 = c.dprm(r.g2); k.dss = c.g(c.ar.ss) + r.ss_off;
  k.C = r.cout; k.rows = rows; k.n = n; k.rows_per_sample = rows_per_sample;
  return k;
}

// ResnetBlock backward: d(out) is complete in the twin of b.out; adds into dA / dB (twins of the inputs; null => skipped)
// storeA / storeB: this block is the first writer of dA / dB in the backward pass (fused path only; the step-by-step path
// below accumulates into the cleared buffers as before)
int res_bwd(const Ctx& c, const ResP& r, const ResBuf& b, const float* inA, float* dA, int cinA, const float* inB, float* dB, int cinB,
            int rows, int n, int rows_per_sample, int storeA, int storeB, const ResRtPre* pre, int* gblocks_out, const ResRtOut* aout) {
  const float* dout = c.g(b.out);
  ResBwd k = res_bwd_args(c, r, b, dA, cinA, dB, cinB, rows, n, rows_per_sample, storeA, storeB);
  const ResBwdForm form = res_bwd_form(k, b.wpart_floats != 0);
  if (form == RES_BWD_WG) {
    // wide m/z levels: the data path AND the block's weight gradients in one launch; its slots are summed by one launch per pass.  (The
    // layout keeps no a1 tensor for such a block: it assumes cat(x, skip) with x of cout channels, as everywhere in the network.)
    ResBwdWg w;
    w.dout = dout; w.u1 = k.u1; w.u2 = k.u2; w.inA = inA; w.inB = inB; w.cinA = cinA; w.cinB = cinB;
    res_operands(c, r, w);
    w.dA = dA; w.dB = dB; w.dA_store = storeA; w.dB_store = storeB; w.part = c.w(b.wpart); w.part_floats = b.wpart_floats;
    // the slot order is the order of the block's tensors in the flat buffer (dq_plan.cpp, Builder::res)
    const int64_t cw = (int64_t)r.cout * r.cin * 3, C = r.cout;
    DQ_REQUIRE(r.c1.b == r.c1.w + cw && r.g1 == r.c1.b + C && r.c2.w == r.g1 + C && r.c2.b == r.c2.w + C * C * 3 && r.g2 == r.c2.b + C &&
               (!r.res.cout || (r.res.w == r.g2 + C && r.res.b == r.res.w + C * r.cin)), "res_bwd: the block's parameters are not contiguous");
    w.dparams = c.dprm(r.c1.w); w.dss = k.dss; w.C = r.cout; w.rows = rows; w.n = n; w.rows_per_sample = rows_per_sample;
    ResWgReduce red;
    DQ_TRY(launch_res_bwd_wg(w, c.s, &red));
    if (c.wg_defer) { c.wg_defer->push_back(red); return 0; }
    return launch_res_wg_reduce(&red, 1, c.s);
  }
  if (form != RES_BWD_UNFUSED) {
    // the whole data path in one launch, then the three weight-gradient launches
    int gblocks = 0;
    k.gpart = c.w(b.gpart); k.gpart_floats = b.gpart_floats; k.gblocks = &gblocks;
    if (pre || aout) DQ_TRY(launch_res_rt_bwd(k, c.s, pre, aout));  // (the caller checked for RES_FWD_RT: d out formed by the launch's prologue / d o by its epilogue)
    else DQ_TRY(launch_res_bwd(k, c.s));
    if (gblocks_out) *gblocks_out = gblocks;
    return res_bwd_side(c, r, b, inA, cinA, inB, cinB, rows, n, rows_per_sample, gblocks);
  }
  DQ_REQUIRE(!pre && !aout, "res_bwd: the attention front / back needs the fused 16-channel block");
  ConvWgrad wg[3];  // conv2, conv1, res_conv: each behind the launch that leaves its d u, one at a time over the whole scratch
  res_wgrads(c, r, b, inA, cinA, inB, cinB, rows, n, 0, c.ar.wg_floats, wg);
  // block2: norm -> silu
  BlockBwd bb;
  bb.u = c.w(b.u2); bb.dy = dout; bb.du = c.g(b.u2); bb.C = r.cout; bb.rows = rows; bb.n = n; bb.rows_per_sample = rows_per_sample;
  bb.g = c.prm(r.g2); bb.dg = c.dprm(r.g2); bb.act = ACT_SILU;
  bb.part = c.w(b.gpart); bb.part_floats = b.gpart_floats;
  DQ_TRY(launch_block_bwd(bb, c.s));
  DQ_TRY(wgrad_async(c, wg[0]));
  ConvBwdData bd;
  bd.du = c.g(b.u2); bd.w = c.prm(r.c2.w); bd.cout = r.cout; bd.K = 3; bd.mode = CONV_S1; bd.rows = rows; bd.n_in = n; bd.n_out = n;
  bd.dinA = c.g(b.a1); bd.cinA = r.cout; bd.accumulate = 0;
  DQ_TRY(launch_conv_bwd_data(bd, c.s));
  // block1: norm -> scale/shift -> silu
  BlockBwd b1;
  b1.u = c.w(b.u1); b1.dy = c.g(b.a1); b1.du = c.g(b.u1); b1.C = r.cout; b1.rows = rows; b1.n = n; b1.rows_per_sample = rows_per_sample;
  b1.g = c.prm(r.g1); b1.dg = c.dprm(r.g1); b1.act = ACT_SILU;
  b1.ss = c.w(c.ar.ss) + r.ss_off; b1.dss = c.g(c.ar.ss) + r.ss_off; b1.ss_stride = c.p.ss_total;
  b1.part = c.w(b.gpart); b1.part_floats = b.gpart_floats;
  DQ_TRY(launch_block_bwd(b1, c.s));
  DQ_TRY(wgrad_async(c, wg[1]));
  if (dA || dB) {
    ConvBwdData d1;
    d1.du = c.g(b.u1); d1.w = c.prm(r.c1.w); d1.cout = r.cout; d1.K = 3; d1.mode = CONV_S1; d1.rows = rows; d1.n_in = n; d1.n_out = n;
    // first writer of dA / dB in this backward pass (the m/z levels whose row length the fused kernels do not take): plain store;
    // otherwise (the bottleneck blocks: cleared twins) accumulate
    d1.dinA = dA; d1.dinB = dB; d1.cinA = cinA; d1.cinB = cinB; d1.accumulate = (storeA || storeB) ? 0 : 1;
    DQ_TRY(launch_conv_bwd_data(d1, c.s));
  }
  // residual path
  if (r.res.cout) {
    DQ_TRY(wgrad_async(c, wg[2]));
    if (dA || dB) {
      ConvBwdData dr;
      dr.du = dout; dr.w = c.prm(r.res.w); dr.cout = r.cout; dr.K = 1; dr.mode = CONV_S1; dr.rows = rows; dr.n_in = n; dr.n_out = n;
      dr.dinA = dA; dr.dinB = dB; dr.cinA = cinA; dr.cinB = cinB; dr.accumulate = 1;
      DQ_TRY(launch_conv_bwd_data(dr, c.s));
    }
  } else if (dA) {
    DQ_TRY(launch_axpy(dA, dout, (int64_t)rows * r.cout * n, c.s));
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// LinearAttention
// ---------------------------------------------------------------------------------------------------------------
// slot: this layer's index in the prepared-weights buffer (la_prepare_all), or -1
int la_fwd(const Ctx& c, const LAP& l, const float* x, float* y, float* ypre, int rows, int n, int slot) {
  LinAttn a;
  a.x = x; a.y = y; a.ypre = ypre; la_operands(c, l, a, &a.b_out); a.C = l.C; a.rows = rows; a.n = n;
  if (slot >= 0 && la_short_row(n)) a.prep = c.w(c.ar.la_prep) + (int64_t)slot * LA_PREP_FLOATS;
  return launch_linattn_fwd(a, c.s);
}
// W2 = Wo Wv and the MFMA operand image of Wq | Wk of every LinearAttention layer, once per forward (one launch) instead of once
// per block of every layer's kernel
int la_prepare_all(const Ctx& c, bool prep_ok, hipStream_t ps) {
  const Plan& p = c.p;
  LaPrepItem items[LA_PREP_MAX];
  int count = 0;
  auto add = [&](const LAP& l) {
    items[count] = LaPrepItem{c.prm(l.qkv_w), c.prm(l.out_w), l.C, c.w(c.ar.la_prep) + (int64_t)count * LA_PREP_FLOATS, c.prm(l.g_pre)};
    ++count;
  };
  if (!prep_ok) return 0;  // (LevelPlan::prep_ok: callers then pass slot -1)
  for (const LevelP& l : p.downs) add(l.la);
  for (const LevelP& l : p.ups) add(l.la);
  // aligned copies of the bottleneck attention's projection weights for the GEMM route (slots 0: q|v, 1: k, 2: to_out), when
  // the flat parameter buffer leaves them off a 16-byte boundary
  PrepCopy cps[PREP_COPY_MAX];
  int nc = 0;
  const int64_t wsrc[3] = {p.qv_w, p.k_w, p.ao_w};
  const int wn[3] = {2 * HID * p.mid_c, HID * p.cond_dim, p.mid_c * HID};
  for (int i = 0; i < 3; ++i)
    if (((uintptr_t)c.prm(wsrc[i]) & 15) != 0 && wn[i] <= WTMP_SLOT) cps[nc++] = PrepCopy{c.prm(wsrc[i]), c.w(c.ar.wtmp) + i * WTMP_SLOT, wn[i]};
  return launch_linattn_prepare(items, count, ps, cps, nc);
}

// the collected slot reductions, one launch
int la_flush(const Ctx& c) {
  Ctx::LaDefer* d = c.la_defer;
  if (!d || d->count == 0) return 0;
  DQ_TRY(launch_linattn_dw_reduce_multi(d->items, d->count, c.s));
  d->count = 0; d->cursor = 0;
  return 0;
}

// The slot reductions collected so far as ONE side-stream item (unet_backward, in front of the last two levels of the down path): every layer
// reduces into its own parameters' gradients, the slots are final when the item is queued, and the side queue has room there -- at the end of
// the pass the reduce of all fourteen layers stood on the main queue in front of the join (~22 us + k_linattn_dwvo); the two levels that are
// left take a third of that.  The slot cursor keeps running (every layer has its own reservation), so nothing the queued reduce reads is reused.
int la_flush_side(const Ctx& c) {
  Ctx::LaDefer* d = c.la_defer;
  const bool off = DQ_DEV_FLAG("DQ_NO_LA_FLUSH_SIDE", '1');  // (dev switch)
  if (!d || d->count == 0 || !side_open(c, !off && tail_fork_enabled())) return 0;  // (else they stay for la_flush)
  std::vector<LaReduceItem> items(d->items, d->items + d->count);
  d->count = 0;
  return on_side(c, true, [items](hipStream_t ss) { return launch_linattn_dw_reduce_multi(items.data(), (int)items.size(), ss); });
}

// A launch's slot scratch in the deferred reduce (Ctx::la_defer).  la_reserve: the region at the cursor, after a flush of what is collected if
// the item table is full or `need` floats no longer fit; la_commit: the launch's reduce item, and the cursor moves past its `need` floats.
int la_reserve(const Ctx& c, int64_t need, float** part, int64_t* part_floats) {
  Ctx::LaDefer* d = c.la_defer;
  if (d->count == LA_REDUCE_MAX || d->cursor + need > c.ar.la_part_floats) DQ_TRY(la_flush(c));
  *part = c.w(c.ar.la_part) + d->cursor; *part_floats = c.ar.la_part_floats - d->cursor;
  return 0;
}
void la_commit(const Ctx& c, const LaReduceItem& item, int64_t need) {
  Ctx::LaDefer* d = c.la_defer;
  d->items[d->count++] = item;
  d->cursor += need;
}

int la_bwd(const Ctx& c, const LAP& l, const LevelBuf& b, const float* x, const float* dy, float* dx, int rows, int n, int slot) {
  LinAttnBwd a;
  a.ypre = c.w(b.la_pre); a.dyp = c.g(b.la_pre); a.dxh = c.g(b.la_tmp);
  a.part = c.w(c.ar.la_part); a.part_floats = c.ar.la_part_floats;
  a.f.x = x; la_operands(c, l, a.f, &a.f.b_out); a.f.C = l.C; a.f.rows = rows; a.f.n = n;
  a.dy = dy; a.dx = dx;
  // W2 of this layer as the forward of this step prepared it (la_prepare_all): same weights, same numbers
  if (slot >= 0 && la_short_row(n)) a.f.prep = c.w(c.ar.la_prep) + (int64_t)slot * LA_PREP_FLOATS;
  a.dw_qkv = c.dprm(l.qkv_w); a.dw_out = c.dprm(l.out_w); a.db_out = c.dprm(l.out_b); a.dg_pre = c.dprm(l.g_pre);
  a.dg_out = c.dprm(l.g_out);
  a.dx_store = 1;  // the block's input feeds nothing else: this launch is the only writer of its gradient (not pre-cleared)
  if (!c.la_defer) return launch_linattn_bwd(a, c.s);
  const int64_t need = la_short_row(n) ? la_part_reserve(l.C) : c.ar.la_part_floats;  // (long rows use the whole buffer)
  DQ_TRY(la_reserve(c, need, &a.part, &a.part_floats));
  int waves = 0;  // (stays 0 when the launch reduced its slots itself: the long-row path)
  a.defer_reduce = 1; a.waves_out = &waves;
  DQ_TRY(launch_linattn_bwd(a, c.s));
  if (waves > 0)
    la_commit(c, la_reduce_item(a.part, waves, l.C, a.dw_qkv, a.dw_out, a.dg_out, a.db_out, a.dg_pre, a.f.w_qkv, a.f.w_out), need);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// convs
// ---------------------------------------------------------------------------------------------------------------
// A bias-free 1x1 conv with many channels on one side (the bottleneck attention's q|v, k and output projections: 16 <-> 256 / 128
// channels over (B, C, RT)) is a per-sample matrix product Y_b (cout x n) = W (cout x cin) X_b (cin x n): it goes to the fp32
// matrix-core GEMM (k_gemm.hip), batched over the samples.  The per-thread channel loop of the generic conv kernels is a serial
// chain of 128-256 dependent FMAs there (47 us forward, 108 us data gradient at batch 32; ~10 us as a GEMM).
bool conv_is_gemm(int cout, int cin, int k, bool has_bias, int mode, int n_in, int n_out) {
  return k == 1 && mode == CONV_S1 && !has_bias && n_in == n_out && n_in % 4 == 0 && cin % 4 == 0 && (cout >= 64 || cin >= 64) &&
         (int64_t)cout * cin <= WTMP_SLOT;
}
bool conv_is_gemm(const Ctx&, const ConvP& cp, int mode, int n_in, int n_out) {
  return conv_is_gemm(cp.cout, cp.cin, cp.k, cp.b >= 0, mode, n_in, n_out);
}
// the GEMM reads its operands with 16-byte loads; a weight slice of the flat parameter buffer that does not start on a 16-byte
// boundary is copied (<= 32 KB, device to device, same stream) to an aligned slot of the arena first
// slot (0: q|v, 1: k, 2: to_out): the copy was made by the forward's prepare launch (la_prepare_all) -- the backward of the same
// step reads the same slot
int gemm_weight(const Ctx& c, const ConvP& cp, const float** w, int slot) {
  *w = c.prm(cp.w);
  if (((uintptr_t)*w & 15) != 0) *w = c.w(c.ar.wtmp) + (int64_t)slot * WTMP_SLOT;
  return 0;
}

// wslot: aligned weight slot prepared by the forward (-1: none; the GEMM route is then only taken for an aligned weight)
// act: ACT_NONE, or ACT_SOFTPLUS for final_conv of a pos_output_only network (the epilogue of its k_conv_fwd<1, 1, 0>)
int conv_plain_fwd(const Ctx& c, const ConvP& cp, int mode, const float* in, float* out, int rows, int n_in, int n_out, int wslot, int act) {
  if (act == ACT_NONE && conv_is_gemm(c, cp, mode, n_in, n_out) && (wslot >= 0 || ((uintptr_t)c.prm(cp.w) & 15) == 0)) {
    Gemm g;
    DQ_TRY(gemm_weight(c, cp, &g.A, wslot));
    g.lda = cp.cin; g.B = in; g.b_kmajor = 0; g.ldb = n_in; g.C = out; g.ldc = n_in;
    g.M = cp.cout; g.N = n_in; g.K = cp.cin; g.batch = rows; g.sBo = (int64_t)cp.cin * n_in; g.sCo = (int64_t)cp.cout * n_in;
    return launch_gemm(g, c.s);
  }
  ConvFwd f;
  f.inA = in; f.cinA = cp.cin; f.w = c.prm(cp.w); f.bias = cp.b >= 0 ? c.prm(cp.b) : nullptr;
  f.cout = cp.cout; f.K = cp.k; f.mode = mode; f.rows = rows; f.n_in = n_in; f.n_out = n_out; f.y_out = out; f.act = act;
  return launch_conv_fwd(f, c.s);
}

// ---- backward of a plain conv over a ConvBwdOps (dq_ops.h)
int conv_level_pre(int mode, int K) {  // the LEVEL_PRE_* stage a (mode, K) conv is, or -1
  if (mode == CONV_DOWN && K == 4) return LEVEL_PRE_DOWN;
  if (mode == CONV_UP && K == 3) return LEVEL_PRE_UP;
  return mode == CONV_S1 && K == 3 ? LEVEL_PRE_S1 : -1;
}
namespace {
// data, weight and bias gradient in one k_conv_bwd_wg launch: a single input, slots laid out, and the bias gradient right behind the weight's
bool conv_bwd_takes_wg(const ConvBwdOps& o, int pre) {
  const bool off = DQ_DEV_FLAG("DQ_NO_CONV_WG", '1');  // (dev switch)
  return !off && o.cpart_floats && o.cinB == 0 && o.dbias == o.dw + (int64_t)o.cout * o.cinA * o.K &&
         conv_wg_usable(o.cout, pre, o.cinA, o.n_out, o.rows_per_sample);
}
// dX_b (cin x n) (+)= W^T (cin x cout) dY_b (cout x n) on the GEMM (a bias does not enter the DATA gradient: to_out's ran on the generic
// kernel because of it, 32 us against ~6 us on the GEMM)
bool conv_bwd_data_is_gemm(const ConvBwdOps& o) {
  return o.cinB == 0 && conv_is_gemm(o.cout, o.cinA, o.K, false, o.mode, o.n_in, o.n_out) && o.w_gemm;
}
ConvWgrad conv_bwd_wgrad_args(const ConvBwdOps& o) {
  ConvWgrad wg;
  wg.scratch = o.wg; wg.scratch_floats = o.wg_floats;
  wg.du = o.dout; wg.inA = o.inA; wg.inB = o.inB; wg.cinA = o.cinA; wg.cinB = o.cinB; wg.cout = o.cout; wg.K = o.K; wg.mode = o.mode;
  wg.rows = o.rows; wg.n_in = o.n_in; wg.n_out = o.n_out; wg.dw = o.dw; wg.dbias = o.dbias;
  return wg;
}
}  // namespace
void conv_bwd_forms(const ConvBwdOps& o, int* data_form, int* wgrad_form) {
  const int pre = conv_level_pre(o.mode, o.K);
  if (pre >= 0 && conv_bwd_takes_wg(o, pre)) { *data_form = CONV_BWD_DATA_WG; *wgrad_form = CONV_WGRAD_WG; return; }
  *data_form = conv_bwd_data_is_gemm(o) ? CONV_BWD_DATA_GEMM : CONV_BWD_DATA_PLAIN;
  *wgrad_form = conv_wgrad_vec4(conv_bwd_wgrad_args(o)) ? CONV_WGRAD_V4 : CONV_WGRAD_SCALAR;
}

int conv_plain_bwd(const ConvBwdOps& o, hipStream_t s) {
  if (o.with_wgrad) {
    const ConvWgrad wg = conv_bwd_wgrad_args(o);
    DQ_TRY(o.wgrad ? o.wgrad(wg) : launch_conv_wgrad(wg, s));
  }
  if (o.dinA && conv_bwd_data_is_gemm(o)) {
    Gemm g;
    g.A = o.w_gemm;
    g.a_kmajor = 0; g.lda = o.cinA; g.B = o.dout; g.b_kmajor = 0; g.ldb = o.n_in; g.C = o.dinA; g.ldc = o.n_in;
    g.M = o.cinA; g.N = o.n_in; g.K = o.cout; g.batch = o.rows; g.sBo = (int64_t)o.cout * o.n_in; g.sCo = (int64_t)o.cinA * o.n_in;
    g.accumulate = o.accumulate;
    return launch_gemm(g, s);
  }
  if (o.dinA || o.dinB) {
    ConvBwdData bd;
    bd.du = o.dout; bd.w = o.w; bd.cout = o.cout; bd.K = o.K; bd.mode = o.mode; bd.rows = o.rows; bd.n_in = o.n_in; bd.n_out = o.n_out;
    bd.dinA = o.dinA; bd.dinB = o.dinB; bd.cinA = o.cinA; bd.cinB = o.cinB; bd.accumulate = o.accumulate;
    DQ_TRY(launch_conv_bwd_data(bd, s));
  }
  return 0;
}

// backward of a level's resample conv: one launch for the data and the weight / bias gradient when the shape allows it
int resample_bwd(const ConvBwdOps& o, int pre, hipStream_t s) {
  if (conv_bwd_takes_wg(o, pre)) {
    ConvBwdWg k;
    k.dy = o.dout; k.in = o.inA; k.w = o.w; k.din = o.dinA; k.accumulate = o.accumulate;
    k.part = o.cpart; k.part_floats = o.cpart_floats; k.dparams = o.dw;
    k.C = o.cout; k.pre = pre; k.cp = o.cinA; k.rows = o.rows; k.n = o.n_out; k.rows_per_sample = o.rows_per_sample;
    ResWgReduce red;
    DQ_TRY(launch_conv_bwd_wg(k, s, &red));
    if (o.wg_defer) { o.wg_defer->push_back(red); return 0; }
    return launch_res_wg_reduce(&red, 1, s);
  }
  return conv_plain_bwd(o, s);
}

namespace {
// the network's operands of a conv's backward
// wslot: aligned weight slot prepared by the forward (-1: none; the GEMM route is then only taken for an aligned weight)
ConvBwdOps conv_bwd_ops(const Ctx& c, const ConvP& cp, int mode, const float* in, const float* dout, float* din, int rows, int n_in, int n_out,
                        int accumulate, int wslot, bool with_wgrad) {
  ConvBwdOps o;
  o.w = c.prm(cp.w); o.dw = c.dprm(cp.w); o.dbias = cp.b >= 0 ? c.dprm(cp.b) : nullptr;
  if (wslot >= 0) gemm_weight(c, cp, &o.w_gemm, wslot);
  else if (((uintptr_t)o.w & 15) == 0) o.w_gemm = o.w;
  o.inA = in; o.cinA = cp.cin; o.dinA = din; o.accumulate = accumulate; o.dout = dout;
  o.cout = cp.cout; o.K = cp.k; o.mode = mode; o.rows = rows; o.n_in = n_in; o.n_out = n_out; o.rows_per_sample = c.RT;
  o.wg = c.w(c.ar.wg); o.wg_floats = c.ar.wg_floats;
  o.with_wgrad = with_wgrad;
  o.wgrad = [&c](const ConvWgrad& w) { return wgrad_async(c, w); };
  o.wg_defer = c.wg_defer;
  return o;
}
}  // namespace
int conv_plain_bwd(const Ctx& c, const ConvP& cp, int mode, const float* in, const float* dout, float* din, int rows, int n_in,
                   int n_out, int accumulate, int wslot, bool with_wgrad) {
  return conv_plain_bwd(conv_bwd_ops(c, cp, mode, in, dout, din, rows, n_in, n_out, accumulate, wslot, with_wgrad), c.s);
}
int resample_bwd(const Ctx& c, const ConvP& cp, int pre, const LevelBuf& b, int n_in, int n_out, int accumulate) {
  const int mode = pre == LEVEL_PRE_DOWN ? CONV_DOWN : (pre == LEVEL_PRE_UP ? CONV_UP : CONV_S1);
  ConvBwdOps o = conv_bwd_ops(c, cp, mode, c.w(b.la), c.g(b.rs), c.g(b.la), c.B * c.RT, n_in, n_out, accumulate, -1, true);
  o.cpart = b.cpart_floats ? c.w(b.cpart) : nullptr; o.cpart_floats = b.cpart_floats;
  return resample_bwd(o, pre, c.s);
}

// ---------------------------------------------------------------------------------------------------------------
// the wide bottleneck (Plan::wide_mid; k_wide.hip): ResnetBlocks and attention projections over (B, mid_c, P) tensors as
// im2col + GEMM + channel-axis norm.  Same op order as the register-resident path (unet1d.py:1144-1148, 302-323, 552-567).
// ---------------------------------------------------------------------------------------------------------------
// C_b (M x N; ldc) (+)= op(A) op(B_b) for every sample b; A is a weight (shared), B and C are (B, rows, P) tensors
int wide_gemm(const Ctx& c, const float* A, int a_kmajor, int64_t lda, const float* Bm, int64_t b_rows, float* C, int64_t c_rows, int M,
              int N, int K, const float* bias_m, int accumulate) {
  Gemm g;
  g.A = A; g.a_kmajor = a_kmajor; g.lda = lda; g.B = Bm; g.b_kmajor = 0; g.ldb = c.ar.P; g.C = C; g.ldc = c.ar.P;
  g.M = M; g.N = N; g.K = K; g.batch = c.B; g.sBo = b_rows * c.ar.P; g.sCo = c_rows * c.ar.P;
  g.bias_m = bias_m; g.accumulate = accumulate;
  g.partial = c.w(c.ar.w_gemm_part); g.partial_floats = c.ar.w_gemm_part_floats;
  DQ_TRY(launch_gemm(g, c.s));
  // the product stores its N valid columns: a stored C is a first writer and owes the slot its zero pads (an accumulated-into C has them)
  return accumulate ? 0 : launch_zero_pads(C, (int64_t)c.B * c_rows, N, c.ar.P, c.s);
}
// dW (M x N; ldc = N) += sum_b dY_b (M x RT) X_b^T (RT x N): dY, X are (B, ., P) tensors.  ONE product whose reduction runs over the
// samples (Gemm::kbatch): dW -- 1.2 GB for the shipped 10000 x 30000 conv -- is read and written once, not once per sample.
int wide_wgrad(const Ctx& c, const float* dY, const float* X, float* dW, int M, int N) {
  Gemm g;
  g.A = dY; g.a_kmajor = 1; g.lda = c.ar.P; g.sAk = (int64_t)M * c.ar.P;
  g.B = X; g.b_kmajor = 1; g.ldb = c.ar.P; g.sBk = (int64_t)N * c.ar.P;
  g.kbatch = c.B;
  g.C = dW; g.ldc = N; g.M = M; g.N = N; g.K = c.RT; g.accumulate = 1;
  g.partial = c.w(c.ar.w_gemm_part); g.partial_floats = c.ar.w_gemm_part_floats;
  return launch_gemm(g, c.s);
}

int wide_res_fwd(const Ctx& c, const ResP& r, const WideResBuf& wb, const float* in) {
  const int B = c.B, RT = c.RT, P = c.ar.P, Cm = r.cout;
  float* xcol = c.w(c.ar.w_xcol);
  DQ_TRY(launch_im2col3(in, xcol, B, Cm, RT, P, c.s));
  DQ_TRY(wide_gemm(c, c.prm(r.c1.w), 1, 3 * Cm, xcol, 3 * Cm, c.w(wb.u1), Cm, Cm, RT, 3 * Cm, c.prm(r.c1.b), 0));
  DQ_TRY(launch_wnorm_fwd(c.w(wb.u1), c.prm(r.g1), c.w(c.ar.ss) + r.ss_off, c.p.ss_total, ACT_SILU, nullptr, c.w(wb.a1), B, Cm, RT, P, c.s));
  DQ_TRY(launch_im2col3(c.w(wb.a1), xcol, B, Cm, RT, P, c.s));
  DQ_TRY(wide_gemm(c, c.prm(r.c2.w), 1, 3 * Cm, xcol, 3 * Cm, c.w(wb.u2), Cm, Cm, RT, 3 * Cm, c.prm(r.c2.b), 0));
  // block2's norm + SiLU, then the identity residual (mid blocks: dim -> dim, unet1d.py:300, 1045, 1057)
  return launch_wnorm_fwd(c.w(wb.u2), c.prm(r.g2), nullptr, 0, ACT_SILU, in, c.w(wb.out), B, Cm, RT, P, c.s);
}

// d(out) is complete in the twin of wb.out; din (B, Cm, P) receives the gradient of the block input (plain store)
int wide_res_bwd(const Ctx& c, const ResP& r, const WideResBuf& wb, const float* in, float* din) {
  const int B = c.B, RT = c.RT, P = c.ar.P, Cm = r.cout;
  const int64_t t = (int64_t)B * Cm * P;
  float* xcol = c.w(c.ar.w_xcol);
  float* dxcol = c.g(c.ar.w_xcol);
  float* st = c.w(c.ar.w_stats);
  const float* dout = c.g(wb.out);
  // block2: out = silu(norm(u2)) + in ; u2 = W2 col(a1) + b2
  DQ_TRY(launch_wnorm_bwd(c.w(wb.u2), dout, c.prm(r.g2), nullptr, 0, ACT_SILU, c.g(wb.u2), c.dprm(r.g2), nullptr, c.dprm(r.c2.b), st, B, Cm,
                          RT, P, c.s));
  DQ_TRY(launch_im2col3(c.w(wb.a1), xcol, B, Cm, RT, P, c.s));
  DQ_TRY(wide_wgrad(c, c.g(wb.u2), xcol, c.dprm(r.c2.w), Cm, 3 * Cm));
  DQ_TRY(wide_gemm(c, c.prm(r.c2.w), 0, 3 * Cm, c.g(wb.u2), Cm, dxcol, 3 * Cm, 3 * Cm, RT, Cm, nullptr, 0));
  DQ_TRY(launch_col2im3(dxcol, c.g(wb.a1), B, Cm, RT, P, 0, c.s));
  // block1: a1 = silu(norm(u1) (scale + 1) + shift) ; u1 = W1 col(in) + b1
  DQ_TRY(launch_wnorm_bwd(c.w(wb.u1), c.g(wb.a1), c.prm(r.g1), c.w(c.ar.ss) + r.ss_off, c.p.ss_total, ACT_SILU, c.g(wb.u1), c.dprm(r.g1),
                          c.g(c.ar.ss) + r.ss_off, c.dprm(r.c1.b), st, B, Cm, RT, P, c.s));
  DQ_TRY(launch_im2col3(in, xcol, B, Cm, RT, P, c.s));
  DQ_TRY(wide_wgrad(c, c.g(wb.u1), xcol, c.dprm(r.c1.w), Cm, 3 * Cm));
  DQ_TRY(wide_gemm(c, c.prm(r.c1.w), 0, 3 * Cm, c.g(wb.u1), Cm, dxcol, 3 * Cm, 3 * Cm, RT, Cm, nullptr, 0));
  DQ_TRY(launch_col2im3(dxcol, din, B, Cm, RT, P, 0, c.s));
  return launch_axpy(din, dout, t, c.s);  // identity residual
}

}  // namespace dq
