// The op wrappers and the side queue (dq_ops.hip): what the network (dq_unet.hip) and the stand-alone op entry points of the C ABI
// (dq_ops_api.hip) share.  The wrappers know a Ctx and nothing of the walk.  Internal: not installed.
#pragma once
#include "dq_net.h"

#include <algorithm>
#include <type_traits>

namespace dq {

constexpr int64_t WTMP_SLOT = 2 * HID * 64;  // floats per aligned weight slot (conv_is_gemm admits no larger weight)
// a 16-byte aligned stand-in for a caller's tensor where only a kernel form is asked for: nothing is dereferenced
inline float* const STAND_IN = reinterpret_cast<float*>(uintptr_t{1} << 20);

// The buffers of one ResnetBlock over B samples of rows_per_sample rows: take(floats) -> offset; take_out: the output's (layout_arena: zero_out)
template <class Take, class TakeOut>
ResBuf layout_res(int B, int rows_per_sample, int cin, int c, int n, Take take, TakeOut take_out) {
  ResBuf r;
  const int64_t t = (int64_t)B * rows_per_sample * c * n;
  // (blocks whose backward forms the weight gradients itself recompute a1 from u1: no a1 tensor)
  const bool wg = B > 0 && res_wg_usable(n, c, c, cin - c, rows_per_sample);
  r.u1 = take(t); r.a1 = wg ? r.u1 : take(t); r.u2 = take(t);
  if (wg) { r.wpart_floats = res_wg_part_floats(c, cin, cin != c, B, rows_per_sample, n); r.wpart = take(r.wpart_floats); }
  r.out = take_out(t);
  // per-block partial sums [dg2 | dg1 | dscale | dshift]: the fused grids, or the <= 64 blocks per sample of k_block_bwd on the unfused path
  r.gpart_floats = (int64_t)B * std::max<int64_t>({((int64_t)rows_per_sample * n + 255) / 256, (rows_per_sample + 15) / 16, 64}) * 4 * c;
  r.gpart = take(r.gpart_floats);
  return r;
}

// ---- the side queue: side-stream launches collected behind one fork event per group, joined at the end of the pass
int wgrad_async(const Ctx& c, const ConvWgrad& w);
int wgrad_async_multi(const Ctx& c, ConvWgrad* w, int count);  // <= 3 stride-1 convs over the same rows: one launch + one reduce
int join_side(const Ctx& c);
int side_flush(const Ctx& c);
int fork_side(const Ctx& c);                      // the side stream continues from this point of the main stream
int side_mark(const Ctx& c, hipEvent_t* ev);      // an event behind what the side stream has been given so far
// "On the side queue if there is one": a piece of the backward that nothing on the main chain waits for.  `allowed` is the call site's own
// condition; with it and a side queue at hand (unet_backward of a plan with an owner) the piece is queued for the next side_flush, else it runs now.
inline bool side_open(const Ctx& c, bool allowed) { return allowed && c.owner && c.side_defer; }
int on_side(const Ctx& c, bool allowed, std::function<int(hipStream_t)> fn, bool forks = true);  // a bare launch
int on_side(const Ctx& c, bool allowed, const std::function<int(const Ctx&)>& body);             // a piece of the pass

// ---- ResnetBlock
// the parameter pointers of a ResnetBlock in a ResFwd, ResBwd, ResBwdWg or TinyBwd::Blk (the biases where the descriptor keeps them)
template <class T, class = void> struct has_res_biases : std::false_type {};
template <class T> struct has_res_biases<T, std::void_t<decltype(T::b1)>> : std::true_type {};
template <class T> void res_operands(const Ctx& c, const ResP& r, T& k) {
  k.w1 = c.prm(r.c1.w); k.w2 = c.prm(r.c2.w); k.wr = r.res.cout ? c.prm(r.res.w) : nullptr;
  k.g1 = c.prm(r.g1); k.g2 = c.prm(r.g2); k.ss = c.w(c.ar.ss) + r.ss_off; k.ss_stride = c.p.ss_total;
  if constexpr (has_res_biases<T>::value) { k.b1 = c.prm(r.c1.b); k.b2 = c.prm(r.c2.b); k.br = r.res.cout ? c.prm(r.res.b) : nullptr; }
}
int res_wg_reduce_all(const std::vector<ResWgReduce>& items, hipStream_t s);
ResFwd level_block(const Ctx& c, const ResP& r, const ResBuf& b, const float* inB, int cinB, bool write_out);
int res_fwd(const Ctx& c, const ResP& r, const ResBuf& b, const float* inA, int cinA, const float* inB, int cinB, int rows, int n,
            int rows_per_sample, const ResRtQkv* qkv = nullptr, const ResRtOut* aout = nullptr);
int res_bwd_side(const Ctx& c, const ResP& r, const ResBuf& b, const float* inA, int cinA, const float* inB, int cinB, int rows, int n,
                 int rows_per_sample, int gblocks);
ResBwd res_bwd_args(const Ctx& c, const ResP& r, const ResBuf& b, float* dA, int cinA, float* dB, int cinB, int rows, int n, int rows_per_sample,
                    int storeA, int storeB);
int res_bwd(const Ctx& c, const ResP& r, const ResBuf& b, const float* inA, float* dA, int cinA, const float* inB, float* dB, int cinB,
            int rows, int n, int rows_per_sample, int storeA = 0, int storeB = 0, const ResRtPre* pre = nullptr, int* gblocks_out = nullptr,
            const ResRtOut* aout = nullptr);

// ---- LinearAttention
// the parameter pointers of a LinearAttention layer in a LinAttn, TinyFwd or TinyBwd (b_out: where the descriptor keeps the output bias, if it does)
template <class T> void la_operands(const Ctx& c, const LAP& l, T& t, const float** b_out = nullptr) {
  t.w_qkv = c.prm(l.qkv_w); t.w_out = c.prm(l.out_w); t.g_pre = c.prm(l.g_pre); t.g_out = c.prm(l.g_out);
  if (b_out) *b_out = c.prm(l.out_b);
}
int la_fwd(const Ctx& c, const LAP& l, const float* x, float* y, float* ypre, int rows, int n, int slot = -1);
int la_prepare_all(const Ctx& c, bool prep_ok, hipStream_t ps);
int la_reserve(const Ctx& c, int64_t need, float** part, int64_t* part_floats);
void la_commit(const Ctx& c, const LaReduceItem& item, int64_t need);
int la_flush(const Ctx& c);
int la_flush_side(const Ctx& c);
int la_bwd(const Ctx& c, const LAP& l, const LevelBuf& b, const float* x, const float* dy, float* dx, int rows, int n, int slot = -1);

// ---- convs
bool conv_is_gemm(int cout, int cin, int k, bool has_bias, int mode, int n_in, int n_out);
bool conv_is_gemm(const Ctx&, const ConvP& cp, int mode, int n_in, int n_out);
int gemm_weight(const Ctx& c, const ConvP& cp, const float** w, int slot);
int conv_plain_fwd(const Ctx& c, const ConvP& cp, int mode, const float* in, float* out, int rows, int n_in, int n_out, int wslot = -1,
                   int act = ACT_NONE);
// backward of a plain conv, free of the network's context: the operands, and where the weight-gradient launches go.  The network
// (conv_plain_bwd / resample_bwd over a Ctx) and the stand-alone dq_conv_bwd fill one of these, so both take the same kernels by the same rule.
struct ConvBwdOps {
  const float* w = nullptr;        // (cout, cinA + cinB, K)
  const float* w_gemm = nullptr;   // the same weight behind a 16-byte aligned address (w itself, or the forward's copy); null: none
  float* dw = nullptr; float* dbias = nullptr;  // += ; dbias null: the conv has no bias
  const float* inA = nullptr; const float* inB = nullptr; int cinA = 0, cinB = 0;  // forward input = cat(A, B)
  float* dinA = nullptr; float* dinB = nullptr; int accumulate = 0;                // its gradient (either nullable): = or +=
  const float* dout = nullptr;
  int cout = 0, K = 1, mode = CONV_S1, rows = 0, n_in = 0, n_out = 0, rows_per_sample = 1;
  float* wg = nullptr; int64_t wg_floats = 0;        // partial blocks of launch_conv_wgrad
  float* cpart = nullptr; int64_t cpart_floats = 0;  // per-workgroup slots of k_conv_bwd_wg; 0: that path was not laid out
  bool with_wgrad = true;
  std::function<int(const ConvWgrad&)> wgrad;        // issues the weight-gradient launch (the network: its side stream); empty: on the call's stream
  std::vector<ResWgReduce>* wg_defer = nullptr;      // collects k_conv_bwd_wg's slot reduction instead of launching it
};
enum ConvBwdDataForm { CONV_BWD_DATA_WG, CONV_BWD_DATA_GEMM, CONV_BWD_DATA_PLAIN };
enum ConvWgradForm { CONV_WGRAD_WG, CONV_WGRAD_V4, CONV_WGRAD_SCALAR };
int conv_level_pre(int mode, int K);
void conv_bwd_forms(const ConvBwdOps& o, int* data_form, int* wgrad_form);
int conv_plain_bwd(const ConvBwdOps& o, hipStream_t s);
int resample_bwd(const ConvBwdOps& o, int pre, hipStream_t s);
int conv_plain_bwd(const Ctx& c, const ConvP& cp, int mode, const float* in, const float* dout, float* din, int rows, int n_in,
                   int n_out, int accumulate, int wslot = -1, bool with_wgrad = true);
int resample_bwd(const Ctx& c, const ConvP& cp, int pre, const LevelBuf& b, int n_in, int n_out, int accumulate);
inline ConvP proj(int64_t w, int cout, int cin) { ConvP c; c.w = w; c.b = -1; c.cout = cout; c.cin = cin; c.k = 1; return c; }

// ---- the wide bottleneck's block ops (Plan::wide_mid; k_wide.hip)
int wide_gemm(const Ctx& c, const float* A, int a_kmajor, int64_t lda, const float* Bm, int64_t b_rows, float* C, int64_t c_rows, int M,
              int N, int K, const float* bias_m, int accumulate);
int wide_wgrad(const Ctx& c, const float* dY, const float* X, float* dW, int M, int N);
int wide_res_fwd(const Ctx& c, const ResP& r, const WideResBuf& wb, const float* in);
int wide_res_bwd(const Ctx& c, const ResP& r, const WideResBuf& wb, const float* in, float* din);

}  // namespace dq
