// K5 backward: gradient of Residual(PreNorm(LinearAttention)) (reference forward: dquartic/model/unet1d.py:446-496; the
// reference's backward is autograd over those ops).  Same wave-per-row scheme and the same re-associated forward as
// k_linattn.hip (per head: M[d][c] = sum_n K[d][n] xh[c][n], P[c][n] = sum_d M[d][c] Q[d][n], ypre = sum_h W2_h P_h + b with
// W2_h = Wo_h Wv_h), differentiated in that form -- no 32x32 context / value tiles exist in either direction.
//
// One launch does the whole block (rows of up to 64 positions; longer rows: k_la_long.hip + two k_block_bwd).  A workgroup is FOUR
// waves = the FOUR heads of the same units (a unit = one row of 32 / 64 positions, or 32 / n rows of n < 32 positions): every wave
//   (1) does the post-norm backward from the saved pre-norm output (per position, over channels: in-lane + one swap with lane^32;
//       the four waves load the same x / ypre / dy at the same time: HBM sees them once)      -> dYpre ; d g_out, d b_out (head 0's wave)
//   (2) for ITS head, recomputing the forward in registers:
//         dP[c][n] = sum_c' W2[c'][c] dYpre[c'][n]                  VALU, C x C per position
//         dW2[c'][c] += sum_n dYpre[c'][n] P[c][n]                  4x4x1 MFMA, both operands staged [c][n] in LDS
//         dQ[d][n] = sum_c M[d][c] dP[c][n]   ; dK^T[n][d] = sum_c xh[c][n] dM[d][c]      32x32x2 MFMA with K = C
//         dM^T[c][d] = sum_n dP[c][n] Q[d][n]                       4x4x1 MFMA (B = Q^T tile)
//         softmax backward of q (over d, in-lane) and k (over n, in-lane in the K^T orientation)
//         dXh_h = Wq^T dq_raw + Wk^T dk_raw + sum_d K[d][n] dM[d][c]                       4x4x1 MFMA
//         dWq += xh dq_raw^T, dWk += xh dk_raw^T                     4x4x1 MFMA
//       Short rows (n < 32, 32/n rows per wave): the masked quadratic form S^T[n'][n] = sum_d K[d][n'] Q[d][n],
//       R[c][n] = sum_n' xh[c][n'] S^T[n'][n] in place of M / P.
//   (3) publishes dXh_h to an LDS exchange buffer; behind ONE workgroup barrier per unit the last head's wave sums the four heads (in
//       head order) and does the residual + pre-norm backward -> dx (+)= dy + d/dx ; d g_pre.  dXh never goes through HBM.
// (Until round 2 every wave walked its units once per head: x / ypre / dy were loaded and normalised four times by different waves at
// different times, dXh was read-modified-written through HBM per head, and a wave flushed its weight-gradient registers four times --
// 25-40 % of a wave's life at 12 / 16 channels.  Heads across the waves of a block: one flush per wave, a slot per BLOCK instead of per
// wave (4x less slot traffic for the reduce), 10-25 % per launch, tools/probe/la_bwd_time.hip.)
// dWv and dWo follow from the summed dW2 once per layer (k_linattn_dwvo): dWo_h = dW2_h Wv_h^T, dWv_h = Wo_h^T dW2_h.
// All parameter gradients go to the block's partial slot (plain stores, each head's wave its own sections) and are summed by
// k_linattn_dw_reduce_multi (k_la_reduce.hip) in a fixed order: no atomics, bitwise repeatable.  Orientation changes (q -> q^T etc.) go
// through a wave-private LDS tile of pitch 36 (transpose_tile36, dq_mfma.h).  Rows of ONE position have a closed form: k_la_bwd1.h.
//
// This header holds the kernel TEMPLATE; it is instantiated by k_la_bwd.hip (the host dispatch: every (C, N) but two) and by
// k_la_bwd_big.hip (<12,64>, <16,64>, built without -amdgpu-mfma-vgpr-form), and by tools/probe/la_bwd_time.hip with -DDQ_LA_PROBE.
// The three forms of the kernel body, by row length (banner comments "FORM ..." below), and what each (C, N) runs with:
//   form    N          C    waves per SIMD   PREFETCH   EX2   note
//   ROW     32, 64     4    2                no         yes   one row per unit, M / P form
//           32         8    2                no         yes
//           64         8    1                yes        yes
//           32         12   1                yes        yes
//           32         16   1                no         yes
//           64         12   1                no         no    k_la_bwd_big.hip
//           64         16   1                no         no    k_la_bwd_big.hip
//   SEG16   16         4    2                no         yes   two rows per unit, M / P form per row (register segment)
//                      8    2                no         yes
//                      12   1                yes        yes
//                      16   1                no         yes
//   QUAD    2, 4, 8    4    2                no         yes   32 / N rows per unit, masked quadratic form; SERIAL tile chains
//           8          8    2                no         yes   SERIAL
//           2, 4       8    1                yes        yes   interleaved tile chains
//           2, 4, 8    12   1                yes        yes   interleaved
//           2, 4, 8    16   1                no         yes   interleaved
// waves per SIMD: the launch bound (la_two_waves); PREFETCH: x / ypre / dy of the next unit requested one unit ahead; EX2: two exchange
// buffers (one workgroup barrier per unit instead of two).  What else was tried: DESIGN.md section 17.2.
#pragma once
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_mfma.h"

namespace dq {

struct LinAttnBwdK {
  const float* x; const float* ypre; const float* dy;  // (rows, C, n): block input, saved pre-norm output, d loss / d y
  float* dx;                                            // += d loss / d x (incl. the residual)
  const float* w_qkv; const float* w_out; const float* g_pre; const float* g_out;
  float* part;  // partial slots (per block; per wave for rows of one position): [slot][la_slot(C)] (dq_kernels.h)
  int rows; int units_per_wave;  // units per BLOCK in k_linattn_bwd (its four waves share them), per wave in k_linattn_bwd1
  const float* prep;  // nullable: this layer's LA_PREP_FLOATS prepared by launch_linattn_prepare (W2 = 4 C C floats, the bounded-logit flag)
  int dx_store;       // dx is written, not accumulated into (its old contents are not read)
#ifdef DQ_LA_PROBE
  unsigned long long* probe;  // tools/probe/la_bwd_time.hip: [wave][16] shader-clock stamps
#endif
};
#ifdef DQ_LA_PROBE
#define DQ_STAMP(i) do { if (a.probe && (threadIdx.x & 63) == 0) a.probe[(int64_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + (i)] = clock64(); } while (0)
#else
#define DQ_STAMP(i) do {} while (0)
#endif

// The two largest instantiations (C >= 12 with 64-position rows; no BASELINE config uses them) crash this compiler's
// "AMDGPU Rewrite AGPR-Copy-MFMA" pass under -amdgpu-mfma-vgpr-form=1: k_la_bwd_big.hip, built without that option (see the Makefile).
void launch_linattn_bwd_big(const LinAttnBwdK& kk, int C, int waves, hipStream_t s);

// Two waves per SIMD (a 256-register budget, enforced through the launch bounds) where the spills that costs stay small: C = 4, and
// C = 8 with rows of 32 / 16 / 8 positions (measured with tools/probe/la_bwd_time.hip, 12,800 rows: <8,16> 183 -> 161 us with 44 B of
// scratch per lane; C = 12 / 16 need 386 / 466 registers and keep one wave per SIMD).  The partner wave covers the latencies the
// one-unit-ahead prefetch was there for, so those variants run without it.
constexpr bool la_two_waves(int C, int N) { return C == 4 || (C == 8 && (N == 32 || N == 16 || N == 8)); }
template <int C, int N>
__global__ void __launch_bounds__(256, la_two_waves(C, N) ? 2 : 1) k_linattn_bwd(LinAttnBwdK a) {
  static_assert(N >= 2, "rows of one position: k_linattn_bwd1");
  constexpr int NB = N >= 32 ? N / 32 : 1;
  constexpr int RW = N >= 32 ? 1 : 32 / N;
  constexpr int NJ = la_nj(C);  // x registers per lane; register j holds channel la_chan(C, j, half)
  constexpr int SEG = N >= 32 ? 16 : (N >= 8 ? N / 2 : N);
  // rows of 16 positions in the M / P form per ROW (a row = register segment s of k^T), as in the forward.  (Rows of 8: measured slower
  // than the masked quadratic form -- four rows per unit mean 2 x 4 C cross-half sums and four short chains per product: <8,8> 90 -> 98 us,
  // <12,8> 132 -> 200 us per 12,800 rows; <8,16> 160 -> 141 us.)
  constexpr bool SEGM = N == 16;
  constexpr int MS_ROW = C * 32 + 8;        // one row's M as [c][d]; + 8 floats: the rows of a unit start in different LDS banks
  constexpr int MS_FLOATS = SEGM ? (RW * MS_ROW > 2 * C * 32 ? RW * MS_ROW : 2 * C * 32) : 2 * C * 32;  // M | dM ; SEGM: M_s, then dM_s over them
  constexpr bool PARTNER = N >= 8;
  constexpr bool SERIAL = la_two_waves(C, N);  // quadratic form: one tile chain at a time (fewer live tiles) instead of interleaved chains
  // C = 4 runs two waves per SIMD instead (the partner wave hides the latency); C = 16 and the 64-position C = 12 variant have
  // no registers to spare
  constexpr bool PREFETCH = (C == 8 && !la_two_waves(C, N)) || (C == 12 && N < 64);
  constexpr int CG = C / 4;      // channel groups of 4 (one 4x4x1 MFMA chain each)
  constexpr int NP = NB * 32;    // positions (lanes x blocks) of one unit
  static_assert(NB <= 2, "rows longer than 64 are not built");
  static_assert(C % 4 == 0, "channel count must be a multiple of 4");

  __shared__ __attribute__((aligned(16))) float wp_lds[2 * 4 * 2 * C * 16];  // [q|k][head][half][c][r] = Wqkv[m*128 + head*32 + rmap(r,half)][c]
  __shared__ __attribute__((aligned(16))) float w2_lds[4 * C * C];           // [head][c'][c] = sum_e Wo[c'][head*32+e] Wv[head*32+e][c]
  __shared__ __attribute__((aligned(16))) float tiles[4][32 * TRP36];
  // per wave: xh | dYpre | P (normalised) | dP as [c][n] ; M | dM as [c][d] ; dW2 of the head being flushed [c'][c] and [c][c']
  __shared__ __attribute__((aligned(16))) float stage[4][4 * C * NP + MS_FLOATS + 2 * C * C];
  // d xh of the four heads of one unit, [parity of the unit][head][c][n]: double-buffered so that ONE barrier per unit is enough (a
  // wave that runs ahead writes the other parity; it cannot reach this parity again before the barrier of the unit in between).
  // The 64-position C >= 12 variants have no LDS left for the second buffer and pay a second barrier instead.
  constexpr bool EX2 = !(C >= 12 && N == 64);
  __shared__ float exch[(EX2 ? 2 : 1) * 4 * C * NP];
  DQ_STAMP(0);
  {  // (every load of a thread requested before its first store: a loop striding by blockDim.x cannot be unrolled -- 4..16 round trips in a row)
    constexpr int NW = 2 * 4 * 2 * C * 16 / 256;
    float v[NW];
#pragma unroll
    for (int u = 0; u < NW; ++u) {
      const int i = u * 256 + (int)threadIdx.x;
      const int r = i & 15, c = (i >> 4) % C, hh = (i / (16 * C)) & 1, hd = (i / (32 * C)) & 3, m = i / (128 * C);
      v[u] = a.w_qkv[(m * 128 + hd * 32 + rmap(r, hh)) * C + c];
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) wp_lds[u * 256 + (int)threadIdx.x] = v[u];
  }
  if (a.prep) {
    for (int i = threadIdx.x; i < 4 * C * C; i += 256) w2_lds[i] = a.prep[i];
  } else {
    for (int i = threadIdx.x; i < 4 * C * C; i += blockDim.x) {
      const int c = i % C, cp = (i / C) % C, hd = i / (C * C);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 32; ++e) s = fmaf(a.w_out[cp * 128 + hd * 32 + e], a.w_qkv[(256 + hd * 32 + e) * C + c], s);
      w2_lds[i] = s;
    }
  }
  __syncthreads();
  DQ_STAMP(1);

  const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  float* tile = tiles[wv];
  float* xs = stage[wv];
  float* dys = xs + C * NP;
  float* ps = dys + C * NP;
  float* dps = ps + C * NP;
  float* ms = dps + C * NP;
  float* dms = SEGM ? ms : ms + C * 32;
  float* w2g = ms + MS_FLOATS;
  const int n_units = (a.rows + RW - 1) / RW;
  const int u0 = blockIdx.x * a.units_per_wave;  // (units per BLOCK here: its four waves walk the same units, one head each)
  if (u0 >= n_units) return;                     // (the whole block)
  const int u1 = min(n_units, u0 + a.units_per_wave);
  const float sqC = sqrtf((float)C);
  const bool bounded = a.prep && a.prep[LA_PREP_BOUNDED] != 0.f;  // (wave-uniform)
  const int rl = N >= 32 ? 0 : col / N;
  // norm gains of this lane's channels, once per wave (a load inside the row loop cannot be hoisted past the loop's stores
  // by the compiler and would sit on the critical path of every row)
  float gpre[NJ], gout[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = la_chan(C, j, half);
    gpre[j] = c < C ? a.g_pre[c] : 0.f;
    gout[j] = c < C ? a.g_out[c] : 0.f;
  }

  // chain4 (the 4x4x1 operand chain over an LDS image [c][pitch], dq_mfma.h) for this lane.  (A binding lambda on purpose: with the 16 call
  // sites calling chain4 directly, 20 of the 22 instantiations come out of the compiler in another instruction order -- up to 6 registers
  // more or 3 fewer -- and would have to be timed again; profiles/wave_header_parity.md.)
  auto chain = [&](const float* src, int pitch, int off, int g, const f32x16& t) { return chain4(src, pitch, off, g, t, lane, half); };
  // its static-weight variant: A = wp_lds[m][hd][half][c = 4*g + (lane&3)][r] (16 consecutive r)
  auto chainw = [&](int m, int hd, int g, const f32x16& t) {
    const float* wr = wp_lds + (((m * 4 + hd) * 2 + half) * C + g * 4 + (lane & 3)) * 16;
    f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const float4 w4 = *reinterpret_cast<const float4*>(wr + r4 * 4);
      t0 = mfma4(w4.x, t[r4 * 4 + 0], t0); t1 = mfma4(w4.y, t[r4 * 4 + 1], t1);
      t0 = mfma4(w4.z, t[r4 * 4 + 2], t0); t1 = mfma4(w4.w, t[r4 * 4 + 3], t1);
    }
    return t0 + t1;
  };

  {
    const int hd = wv;  // this wave's head
    const bool first = hd == 0, last = hd == 3;
    float wq[NJ], wk[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = la_chan(C, j, half);
      const bool ok = c < C;
      wq[j] = ok ? a.w_qkv[(hd * 32 + col) * C + c] * LOG2E : 0.f;   // log2(e) folded in: the softmaxes use exp2 like the forward
      wk[j] = ok ? a.w_qkv[(128 + hd * 32 + col) * C + c] * LOG2E : 0.f;
    }
    // weight-gradient accumulators of this head, 4x4x1 form: register i of group g = channel 4*g + i, lane = (half, d);
    // each lane-half sums its own 16 positions of every 32-block, the halves are added at the flush
    f32x4 gq[CG], gk[CG];
    f32x4 gw2[CG][CG];  // dW2[c' = 4*g1 + i][c = 4*g2 + (lane&3)], partial over the positions of this 4-lane block
#pragma unroll
    for (int g = 0; g < CG; ++g) {
      gq[g] = gk[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g2 = 0; g2 < CG; ++g2) gw2[g][g2] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float nacc0[NJ], nacc1[NJ];  // norm-gain / bias gradient partials: head 0's wave: (d g_out, d b_out); head 3's: (d g_pre, -)
#pragma unroll
    for (int j = 0; j < NJ; ++j) nacc0[j] = nacc1[j] = 0.f;

    // raw operands of one unit (row block): loaded one unit AHEAD when the registers allow it (C <= 8), so that the global
    // latency hides behind the previous unit's MFMAs -- with one wave per SIMD nothing else would cover it
    float px[NB][NJ], pu[NB][NJ], pd[NB][NJ];
    auto load_unit = [&](int u) {
      const int row = u * RW + rl;
      const bool row_ok = row < a.rows;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int pos = N >= 32 ? b * 32 + col : col % N;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = la_chan(C, j, half);
          const bool ok = row_ok && c < C;
          // (predicated on purpose: the unpredicated form -- clamped row, select afterwards -- was measured: <8,32> 207 -> 290 us, the other
          // instantiations unchanged)
          const int64_t off = ((int64_t)row * C + c) * N + pos;
          px[b][j] = ok ? a.x[off] : 0.f;
          pu[b][j] = ok ? a.ypre[off] : 0.f;
          pd[b][j] = ok ? a.dy[off] : 0.f;
        }
      }
    };
    if (PREFETCH) load_unit(u0);

#pragma unroll 1
    for (int u = u0; u < u1; ++u) {
      const int row = u * RW + rl;
      const bool row_ok = row < a.rows;
      // ---- x, ypre, dy; pre-norm recompute; post-norm backward (same arithmetic as k_block_bwd) -> DY = dYpre
      float Xh[NB][NJ], DY[NB][NJ];
      float cx[NB][NJ], cu[NB][NJ], cd[NB][NJ];
      if (!PREFETCH) load_unit(u);
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < NJ; ++j) { cx[b][j] = px[b][j]; cu[b][j] = pu[b][j]; cd[b][j] = pd[b][j]; }
      if (PREFETCH && u + 1 < u1) load_unit(u + 1);
      // what the tail of this iteration reads back -- dx, in the last head's wave when it accumulates -- is requested now, so that
      // its latency hides behind the MFMA work instead of stalling the read-modify-write at the end
      float pdx[NB][NJ];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = la_chan(C, j, half);
          const int64_t off = ((int64_t)row * C + c) * N + (N >= 32 ? b * 32 + col : col % N);
          pdx[b][j] = (PREFETCH && row_ok && c < C && last && !a.dx_store) ? a.dx[off] : 0.f;
        }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float xv[NJ], uv[NJ], dv_[NJ];
        float ssq = 0.f, usq = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          xv[j] = cx[b][j]; uv[j] = cu[b][j]; dv_[j] = cd[b][j];
          ssq = fmaf(xv[j], xv[j], ssq);
          usq = fmaf(uv[j], uv[j], usq);
        }
        ssq += swap_half(ssq);
        usq += swap_half(usq);
        // (v_sqrt / v_rcp, 1 ulp each, as the forward kernel: a correctly rounded division or square root is ~10 instructions, and this
        // kernel issued 13 of them per unit and head)
        const float inv = rms_inv(ssq, sqC);
        const float unrm = fast_sqrt(usq);
        const float uinv = fast_rcp(fmaxf(unrm, RMS_EPS));
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          Xh[b][j] = xv[j] * inv * gpre[j];
          const float uh = uv[j] * uinv;
          if (first) nacc0[j] = fmaf(dv_[j], uh * sqC, nacc0[j]);  // d g_out
          const float gd = dv_[j] * gout[j] * sqC;
          uv[j] = uh;
          dv_[j] = gd;
          dot = fmaf(gd, uh, dot);
        }
        dot += swap_half(dot);
        const bool clamped = unrm < RMS_EPS;  // F.normalize clamps the norm: below eps the map is linear
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          DY[b][j] = clamped ? dv_[j] * uinv : uinv * (dv_[j] - uv[j] * dot);
          if (first) nacc1[j] += DY[b][j];  // d b_out (bias of to_out)
        }
      }
      // stage xh and dYpre as [c][n]: 4x4x1 A operands, and every lane needs ALL channels of dYpre at its position
      wave_fence();
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = la_chan(C, j, half);
          if (c < C) {
            xs[c * NP + b * 32 + col] = Xh[b][j];
            dys[c * NP + b * 32 + col] = DY[b][j];
          }
        }
      wave_fence();

      // dP[c][n] = sum_c' W2[hd][c'][c] dYpre[c'][n] at this lane's position of block b (identical in both lane halves)
      auto make_dp = [&](int b, float (&dp)[C]) {
        float dya[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { dya[c] = dys[c * NP + b * 32 + col]; dp[c] = 0.f; }
#pragma unroll
        for (int cp = 0; cp < C; ++cp) {
          const float* w = w2_lds + (hd * C + cp) * C;
#pragma unroll
          for (int c4 = 0; c4 < CG; ++c4) {
            const float4 w4 = *reinterpret_cast<const float4*>(w + 4 * c4);
            dp[4 * c4 + 0] = fmaf(w4.x, dya[cp], dp[4 * c4 + 0]); dp[4 * c4 + 1] = fmaf(w4.y, dya[cp], dp[4 * c4 + 1]);
            dp[4 * c4 + 2] = fmaf(w4.z, dya[cp], dp[4 * c4 + 2]); dp[4 * c4 + 3] = fmaf(w4.w, dya[cp], dp[4 * c4 + 3]);
          }
        }
      };

      f32x4 part[NB][CG];  // d xh partial sums of this lane-half (this head): register i = channel 4*g + i, lane = position
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int g = 0; g < CG; ++g) part[b][g] = f32x4{0.f, 0.f, 0.f, 0.f};
      // part[c][n] += sum_r W[m][hd][rmap(r,half)][c] * t[r][n]: B = the tile register (rows d, col n), A = the weight column
      auto add_dxh = [&](int b, int m, const f32x16& t) {
#pragma unroll
        for (int g = 0; g < CG; ++g) part[b][g] += chainw(m, hd, g, t);
      };
      // dW[c][d] += sum_n xh[c][n] * tt[n][d] over the positions of 32-block b (B = register r of the (rows n, col d) tile)
      auto add_dw = [&](f32x4 (&acc)[CG], int b, const f32x16& tt) {
#pragma unroll
        for (int g = 0; g < CG; ++g) acc[g] += chain(xs, NP, b * 32, g, tt);
      };
      // dW2[c'][c] += sum_n dYpre[c'][n] p[c][n] over all staged positions: position n = 16 * s + (lane >> 2)
      auto add_dw2 = [&]() {
#pragma unroll
        for (int s = 0; s < NP / 16; ++s) {
          const int n = 16 * s + (lane >> 2);
#pragma unroll
          for (int g1 = 0; g1 < CG; ++g1) {
            const float av = dys[(4 * g1 + (lane & 3)) * NP + n];
#pragma unroll
            for (int g2 = 0; g2 < CG; ++g2) gw2[g1][g2] = mfma4(av, ps[(4 * g2 + (lane & 3)) * NP + n], gw2[g1][g2]);
          }
        }
      };

      // ---- K^T (rows n, col d): exps, then normalised in place (softmax over the positions of each row)
      f32x16 kT[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        f32x16 ak = {0};
#pragma unroll
        for (int j = 0; j < NJ; ++j) ak = mfma32(Xh[b][j], wk[j], ak);
        kT[b] = ak;
      }
#pragma unroll
      for (int s0 = 0; s0 < 16; s0 += SEG) {
        float ssum = 0.f;
        if (bounded) {  // |logit| <= 64 for every input (LA_PREP_BOUNDED, k_linattn_prepare): no shift by the row maximum, as in the forward
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = s0; r < s0 + SEG; ++r) {
              const float e = __builtin_amdgcn_exp2f(kT[b][r]);
              kT[b][r] = e;
              ssum += e;
            }
        } else {
          float m = -INFINITY;
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = s0; r < s0 + SEG; ++r) m = fmaxf(m, kT[b][r]);
          if (PARTNER) m = fmaxf(m, swap_half(m));
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = s0; r < s0 + SEG; ++r) {
              const float e = __builtin_amdgcn_exp2f(kT[b][r] - m);
              kT[b][r] = e;
              ssum += e;
            }
        }
        if (PARTNER) ssum += swap_half(ssum);
        const float rs = fast_rcp(ssum);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int r = s0; r < s0 + SEG; ++r) kT[b][r] *= rs;
      }
      // q (rows d, col n) with its softmax (normalised, incl. 32^-0.5)
      auto make_q = [&](int b) {
        f32x16 q = {0};
#pragma unroll
        for (int j = 0; j < NJ; ++j) q = mfma32(wq[j], Xh[b][j], q);
        float ssum = 0.f;
        if (bounded) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            q[r] = __builtin_amdgcn_exp2f(q[r]);
            ssum += q[r];
          }
        } else {
          float m = q[0];
#pragma unroll
          for (int r = 1; r < 16; ++r) m = fmaxf(m, q[r]);
          m = fmaxf(m, swap_half(m));
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            q[r] = __builtin_amdgcn_exp2f(q[r] - m);
            ssum += q[r];
          }
        }
        ssum += swap_half(ssum);
        const float qs = ATT_SCALE * fast_rcp(ssum);
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] *= qs;
        return q;
      };
      // the same with the sum over d taken from the C-row side: sum_d q dq = sum_d q sum_c M[d][c] dP[c] = sum_c dP[c] P[c] (P = M^T q, both in every
      // lane of the position already): C FMAs in place of 16 + a cross-half swap
      auto q_softmax_bwd_pp = [&](const f32x16& q, const f32x16& dq, const float (&dP)[C], const float (&P)[C]) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) t = fmaf(dP[c], P[c], t);
        t *= (1.0f / ATT_SCALE);
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = q[r] * (dq[r] - t);
        return o;
      };
      auto q_softmax_bwd = [&](const f32x16& q, const f32x16& dq) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t = fmaf(q[r], dq[r], t);
        t = (t + swap_half(t)) * (1.0f / ATT_SCALE);
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = q[r] * (dq[r] - t);
        return o;
      };

      if (N >= 32) {
        // ================= FORM ROW (N = 32, 64) -- one row per wave: M / P form =================
        // M[d = col][c] (both lane halves hold the total) and its [c][d] image for the P chains
        float Mr[C];
#pragma unroll
        for (int g = 0; g < CG; ++g) {
          f32x4 mt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int b = 0; b < NB; ++b) mt += chain(xs, NP, b * 32, g, kT[b]);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            Mr[g * 4 + i] = mt[i] + swap_half(mt[i]);
            if (half == 0) ms[(g * 4 + i) * 32 + col] = Mr[g * 4 + i];
          }
        }
        wave_fence();
        // (Round 4: no tile is carried from one phase to the next any more.  Q^T of a block was kept for dM = sum_b dP_b Q_b^T and dK^T of
        // both blocks for the k-softmax backward's sum over the row -- 64 registers at two blocks; now dM accumulates inside the block loop
        // (same order of additions: bit-identical) and dK^T is formed twice (the sum, then the gradient: 2 NJ more K = C MFMAs per unit).)
        f32x4 mtd[CG];  // dM^T[c][d] partial sums of this lane-half: sum over the blocks of dP Q^T
#pragma unroll
        for (int g = 0; g < CG; ++g) mtd[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const f32x16 q = make_q(b);
          float dP[C], P[C];
          make_dp(b, dP);
#pragma unroll
          for (int g = 0; g < CG; ++g) {
            const f32x4 pp = chain(ms, 32, 0, g, q);
#pragma unroll
            for (int i = 0; i < 4; ++i) P[g * 4 + i] = pp[i] + swap_half(pp[i]);
          }
          if (half == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) { ps[c * NP + b * 32 + col] = P[c]; dps[c * NP + b * 32 + col] = dP[c]; }
          }
          // dQ[d][n] = sum_c M[d][c] dP[c][n] (K = C on the 32x32x2 pipe), softmax backward, Wq paths
          f32x16 dq = {0};
#pragma unroll
          for (int j = 0; j < NJ; ++j) dq = mfma32(own_of<C>(Mr, j, half), own_of<C>(dP, j, half), dq);
          const f32x16 dq_raw = q_softmax_bwd_pp(q, dq, dP, P);
          add_dxh(b, 0, dq_raw);
          add_dw(gq, b, transpose_tile36(dq_raw, tile, col, half));
          const f32x16 qT = transpose_tile36(q, tile, col, half);  // Q^T (rows n, col d); (the fences inside tr32 also complete this block's ps / dps stores)
#pragma unroll
          for (int g = 0; g < CG; ++g) mtd[g] += chain(dps, NP, b * 32, g, qT);  // dM^T[c][d] += sum_(n in block b) dP[c][n] Q[d][n]
        }
        wave_fence();  // ps / dps complete
        add_dw2();
        // dM: both halves ; its [c][d] image for the dXh chain
        float dMr[C];
#pragma unroll
        for (int g = 0; g < CG; ++g) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            dMr[g * 4 + i] = mtd[g][i] + swap_half(mtd[g][i]);
            if (half == 0) dms[(g * 4 + i) * 32 + col] = dMr[g * 4 + i];
          }
        }
        wave_fence();
        // dK^T[n][d] = sum_c xh[c][n] dM[d][c] ; softmax backward over the positions of the row.  Its sum over the row needs no tile:
        // sum_n K[d][n] dK[d][n] = sum_c dM[d][c] sum_n K[d][n] xh[c][n] = sum_c dM[d][c] M[d][c]  (this lane's d; both halves hold M, dM)
        float dl = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) dl = fmaf(dMr[c], Mr[c], dl);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const f32x16 kTb = kT[b];
          f32x16 dk_rawT = {0};
#pragma unroll
          for (int j = 0; j < NJ; ++j) dk_rawT = mfma32(Xh[b][j], own_of<C>(dMr, j, half), dk_rawT);
#pragma unroll
          for (int r = 0; r < 16; ++r) dk_rawT[r] = kTb[r] * (dk_rawT[r] - dl);
          add_dw(gk, b, dk_rawT);
          add_dxh(b, 1, transpose_tile36(dk_rawT, tile, col, half));
          const f32x16 Kd = transpose_tile36(kTb, tile, col, half);  // rows d, col n
#pragma unroll
          for (int g = 0; g < CG; ++g) part[b][g] += chain(dms, 32, 0, g, Kd);  // dXh[c][n] += sum_d K[d][n] dM[d][c]
        }
      } else if (SEGM) {
        // ================= FORM SEG16 (N = 16) -- two rows per unit: M / P form per ROW =================
        // Row s of the unit is register segment s of k^T in both lane halves (the forward's mapping), so M_s / dM_s are the 4x4x1 chains
        // restricted to that segment, and a position contracts with the M of its own row (a 4-lane block never straddles rows).  The
        // products with K = C that mix rows -- dQ = M_row(n) dP, dK^T = xh dM_row(n) -- run once per row with the other rows' columns
        // zeroed: 2 NJ + 2 RW NJ 32x32x2 MFMAs per unit instead of the 64 + 4 NJ of the masked S tiles, no S / dS tiles at all.
        auto seg_chain = [&](const float* src, int g, int s, const f32x16& t) {  // sum over the registers of segment s
          const float* ar = src + (g * 4 + (lane & 3)) * NP + 4 * half;
          f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int q4 = s * SEG / 4; q4 < (s + 1) * SEG / 4; ++q4) {
            const float4 a4 = *reinterpret_cast<const float4*>(ar + 8 * q4);
            t0 = mfma4(a4.x, t[q4 * 4 + 0], t0); t1 = mfma4(a4.y, t[q4 * 4 + 1], t1);
            t0 = mfma4(a4.z, t[q4 * 4 + 2], t0); t1 = mfma4(a4.w, t[q4 * 4 + 3], t1);
          }
          return t0 + t1;
        };
        // M_s[d = col][c] = sum_(n in row s) k[d][n] xh[c][n], staged [s][c][d]
#pragma unroll
        for (int s = 0; s < RW; ++s)
#pragma unroll
          for (int g = 0; g < CG; ++g) {
            const f32x4 mt = seg_chain(xs, g, s, kT[0]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float v = mt[i] + swap_half(mt[i]);
              if (half == 0) ms[s * MS_ROW + (g * 4 + i) * 32 + col] = v;
            }
          }
        wave_fence();
        const f32x16 q = make_q(0);
        float dP[C], P[C];
        make_dp(0, dP);
#pragma unroll
        for (int g = 0; g < CG; ++g) {
          const f32x4 pp = chain(ms + rl * MS_ROW, 32, 0, g, q);  // P[c][n] = sum_d M_row(n)[d][c] q[d][n]
#pragma unroll
          for (int i = 0; i < 4; ++i) P[g * 4 + i] = pp[i] + swap_half(pp[i]);
        }
        if (half == 0) {
#pragma unroll
          for (int c = 0; c < C; ++c) { ps[c * NP + col] = P[c]; dps[c * NP + col] = dP[c]; }
        }
        // dQ[d][n] = sum_c M_row(n)[d][c] dP[c][n]: row by row, the columns of the other rows zeroed
        f32x16 dq = {0};
#pragma unroll
        for (int s = 0; s < RW; ++s)
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int c = la_chan(C, j, half);
            const float mv = c < C ? ms[s * MS_ROW + (c < C ? c : 0) * 32 + col] : 0.f;
            dq = mfma32(mv, rl == s ? own_of<C>(dP, j, half) : 0.f, dq);
          }
        const f32x16 dq_raw = q_softmax_bwd_pp(q, dq, dP, P);
        add_dxh(0, 0, dq_raw);
        add_dw(gq, 0, transpose_tile36(dq_raw, tile, col, half));
        const f32x16 qT = transpose_tile36(q, tile, col, half);  // rows n, col d
        wave_fence();  // ps / dps complete; every read of M_s is done (dM_s goes over it)
        add_dw2();
        // dM_s^T[c][d] = sum_(n in row s) dP[c][n] Q[d][n], staged [s][c][d] over M_s
#pragma unroll
        for (int s = 0; s < RW; ++s)
#pragma unroll
          for (int g = 0; g < CG; ++g) {
            const f32x4 mt = seg_chain(dps, g, s, qT);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float v = mt[i] + swap_half(mt[i]);
              if (half == 0) dms[s * MS_ROW + (g * 4 + i) * 32 + col] = v;
            }
          }
        wave_fence();
        // dK^T[n][d] = sum_c xh[c][n] dM_row(n)[d][c]: row by row, the rows (positions) of the other rows zeroed
        f32x16 dkT = {0};
#pragma unroll
        for (int s = 0; s < RW; ++s)
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int c = la_chan(C, j, half);
            const float dmv = c < C ? dms[s * MS_ROW + (c < C ? c : 0) * 32 + col] : 0.f;
            dkT = mfma32(rl == s ? Xh[0][j] : 0.f, dmv, dkT);
          }
        f32x16 dk_rawT;  // softmax over the positions of each row: a lane's own register segment (+ lane^32)
#pragma unroll
        for (int s0 = 0; s0 < 16; s0 += SEG) {
          float dl = 0.f;
#pragma unroll
          for (int r = s0; r < s0 + SEG; ++r) dl = fmaf(dkT[r], kT[0][r], dl);
          dl += swap_half(dl);
#pragma unroll
          for (int r = s0; r < s0 + SEG; ++r) dk_rawT[r] = kT[0][r] * (dkT[r] - dl);
        }
        add_dw(gk, 0, dk_rawT);
        add_dxh(0, 1, transpose_tile36(dk_rawT, tile, col, half));
        const f32x16 Kd = transpose_tile36(kT[0], tile, col, half);  // rows d, col n
#pragma unroll
        for (int g = 0; g < CG; ++g) part[0][g] += chain(dms + rl * MS_ROW, 32, 0, g, Kd);  // dXh[c][n] += sum_d K[d][n] dM_row(n)[d][c]
      } else {
        // ================= FORM QUAD (N = 2, 4, 8) -- 32/N rows per wave, one block: masked quadratic form =================
        // Two waves per SIMD (SERIAL): one 32x32 tile chain at a time (round 4): S^T -> R, then S -> its dXh chain, then dS^T -> dQ and the whole q side, then dS -> dK^T.
        // Each 16-deep chain runs back to back on one accumulator (this MFMA needs no interleaving with a second chain), the same sums in
        // the same order as before -- but at most four tiles are live (q, K, K^T and the chain's accumulator) instead of nine.
        // One wave per SIMD (12 / 16 channels) keeps the interleaved order: nothing else overlaps a chain's latencies there, and the serial
        // order measured 2-6 % slower (<12,8> 151 -> 159 us, <12,2> 68 -> 73 us stand-alone).
        if constexpr (SERIAL) {
          const f32x16 q = make_q(0);
          const f32x16 Kd = transpose_tile36(kT[0], tile, col, half);
          float dR[C];
          {
            f32x16 st = {0};
  #pragma unroll
            for (int r = 0; r < 16; ++r) st = mfma32(Kd[r], q[r], st);  // S^T : rows n', col n
            st = mask_same_row<N>(st, col, half);
            float R[C];
  #pragma unroll
            for (int g = 0; g < CG; ++g) {
              const f32x4 rr = chain(xs, NP, 0, g, st);  // R[c][n] = sum_n' xh[c][n'] S^T[n'][n]
  #pragma unroll
              for (int i = 0; i < 4; ++i) R[g * 4 + i] = rr[i] + swap_half(rr[i]);
            }
            make_dp(0, dR);
            if (half == 0) {
  #pragma unroll
              for (int c = 0; c < C; ++c) { ps[c * NP + col] = R[c]; dps[c * NP + col] = dR[c]; }
            }
          }
          wave_fence();
          add_dw2();
          __builtin_amdgcn_sched_barrier(0);
          {
            f32x16 sm = {0};
  #pragma unroll
            for (int r = 0; r < 16; ++r) sm = mfma32(q[r], Kd[r], sm);  // S   : rows n,  col n'
            sm = mask_same_row<N>(sm, col, half);
            // dXh[c][n'] += sum_n S[n][n'] dR[c][n]
  #pragma unroll
            for (int g = 0; g < CG; ++g) part[0][g] += chain(dps, NP, 0, g, sm);
          }
          __builtin_amdgcn_sched_barrier(0);
          // dS^T[n'][n] = sum_c xh[c][n'] dR[c][n] (K = C product), masked to pairs of the same row ; dQ ; the q side
          f32x16 qT;
          {
            f32x16 dst = {0};
  #pragma unroll
            for (int j = 0; j < NJ; ++j) dst = mfma32(Xh[0][j], own_of<C>(dR, j, half), dst);
            dst = mask_same_row<N>(dst, col, half);
            f32x16 dq = {0};
  #pragma unroll
            for (int r = 0; r < 16; ++r) dq = mfma32(kT[0][r], dst[r], dq);    // rows d,  col n
            const f32x16 dq_raw = q_softmax_bwd(q, dq);
            add_dxh(0, 0, dq_raw);
            add_dw(gq, 0, transpose_tile36(dq_raw, tile, col, half));
            qT = transpose_tile36(q, tile, col, half);  // (only now: one tile fewer is live across the S / dS products)
          }
          __builtin_amdgcn_sched_barrier(0);
          // dS = the transpose of dS^T (the K = C product with the operands swapped) ; dK^T ; the k side
          f32x16 dkT = {0};
          {
            f32x16 dsm = {0};
  #pragma unroll
            for (int j = 0; j < NJ; ++j) dsm = mfma32(own_of<C>(dR, j, half), Xh[0][j], dsm);
            dsm = mask_same_row<N>(dsm, col, half);
  #pragma unroll
            for (int r = 0; r < 16; ++r) dkT = mfma32(dsm[r], qT[r], dkT);     // rows n', col d
          }
          f32x16 dk_rawT;  // softmax over the positions of each row: a lane's own register segment (+ lane^32)
  #pragma unroll
          for (int s0 = 0; s0 < 16; s0 += SEG) {
            float dl = 0.f;
  #pragma unroll
            for (int r = s0; r < s0 + SEG; ++r) dl = fmaf(dkT[r], kT[0][r], dl);
            if (PARTNER) dl += swap_half(dl);
  #pragma unroll
            for (int r = s0; r < s0 + SEG; ++r) dk_rawT[r] = kT[0][r] * (dkT[r] - dl);
          }
          add_dw(gk, 0, dk_rawT);
          add_dxh(0, 1, transpose_tile36(dk_rawT, tile, col, half));
      
        } else {
          const f32x16 q = make_q(0);
          const f32x16 qT = transpose_tile36(q, tile, col, half);
          const f32x16 Kd = transpose_tile36(kT[0], tile, col, half);
          f32x16 st = {0}, sm = {0};
  #pragma unroll
          for (int r = 0; r < 16; ++r) {
            st = mfma32(Kd[r], q[r], st);  // S^T : rows n', col n
            sm = mfma32(q[r], Kd[r], sm);  // S   : rows n,  col n'
          }
          st = mask_same_row<N>(st, col, half);
          sm = mask_same_row<N>(sm, col, half);
          float dR[C], R[C];
          make_dp(0, dR);
  #pragma unroll
          for (int g = 0; g < CG; ++g) {
            const f32x4 rr = chain(xs, NP, 0, g, st);  // R[c][n] = sum_n' xh[c][n'] S^T[n'][n]
  #pragma unroll
            for (int i = 0; i < 4; ++i) R[g * 4 + i] = rr[i] + swap_half(rr[i]);
          }
          if (half == 0) {
  #pragma unroll
            for (int c = 0; c < C; ++c) { ps[c * NP + col] = R[c]; dps[c * NP + col] = dR[c]; }
          }
          wave_fence();
          add_dw2();
          // dS^T[n'][n] = sum_c xh[c][n'] dR[c][n] and dS = its transpose (K = C products), masked to pairs of the same row
          f32x16 dst = {0}, dsm = {0};
  #pragma unroll
          for (int j = 0; j < NJ; ++j) {
            dst = mfma32(Xh[0][j], own_of<C>(dR, j, half), dst);
            dsm = mfma32(own_of<C>(dR, j, half), Xh[0][j], dsm);
          }
          dst = mask_same_row<N>(dst, col, half);
          dsm = mask_same_row<N>(dsm, col, half);
          // dXh[c][n'] += sum_n S[n][n'] dR[c][n]
  #pragma unroll
          for (int g = 0; g < CG; ++g) part[0][g] += chain(dps, NP, 0, g, sm);
          f32x16 dq = {0}, dkT = {0};
  #pragma unroll
          for (int r = 0; r < 16; ++r) {
            dq = mfma32(kT[0][r], dst[r], dq);    // rows d,  col n
            dkT = mfma32(dsm[r], qT[r], dkT);     // rows n', col d
          }
          const f32x16 dq_raw = q_softmax_bwd(q, dq);
          add_dxh(0, 0, dq_raw);
          add_dw(gq, 0, transpose_tile36(dq_raw, tile, col, half));
          f32x16 dk_rawT;  // softmax over the positions of each row: a lane's own register segment (+ lane^32)
  #pragma unroll
          for (int s0 = 0; s0 < 16; s0 += SEG) {
            float dl = 0.f;
  #pragma unroll
            for (int r = s0; r < s0 + SEG; ++r) dl = fmaf(dkT[r], kT[0][r], dl);
            if (PARTNER) dl += swap_half(dl);
  #pragma unroll
            for (int r = s0; r < s0 + SEG; ++r) dk_rawT[r] = kT[0][r] * (dkT[r] - dl);
          }
          add_dw(gk, 0, dk_rawT);
          add_dxh(0, 1, transpose_tile36(dk_rawT, tile, col, half));
      
        }
      }

      // ---- d xh of this head: both halves' partial sums; each lane publishes its own channels to the block's exchange buffer, and
      // the last head's wave sums the four heads (in head order) behind the barrier.  Nothing of d xh goes through HBM.
      float* ex = exch + ((EX2 ? ((u - u0) & 1) : 0) * 4 + hd) * (C * NP);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float full[C];
#pragma unroll
        for (int c = 0; c < C; ++c) full[c] = part[b][c >> 2][c & 3] + swap_half(part[b][c >> 2][c & 3]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = la_chan(C, j, half);
          if (c < C) ex[c * NP + b * 32 + col] = own_of<C>(full, j, half);
          // (no registers to hold dx across the MFMA work in these variants: requested here, in front of the barrier)
          if (!PREFETCH && row_ok && c < C && last && !a.dx_store)
            pdx[b][j] = a.dx[((int64_t)row * C + c) * N + (N >= 32 ? b * 32 + col : col % N)];
        }
      }
      lds_barrier();  // (LDS-only: __syncthreads() would also wait for the dx values just requested and for a prefetched next unit)
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int pos = N >= 32 ? b * 32 + col : col % N;
        float tot[NJ];
        if (last) {
          const float* e0 = exch + (EX2 ? ((u - u0) & 1) : 0) * 4 * (C * NP);
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int c = la_chan(C, j, half);
            const int e = (c < C ? c : 0) * NP + b * 32 + col;
            const float v = ((e0[e] + e0[C * NP + e]) + e0[2 * C * NP + e]) + e0[3 * C * NP + e];
            tot[j] = (row_ok && c < C) ? v : 0.f;
          }
          // ---- residual + pre-norm backward on the completed dXh (own channels c = la_chan(C, j, half)); dx += dy + d/dx
          float xv[NJ];
          float ssq = 0.f;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            xv[j] = cx[b][j];  // raw x of this unit (zero for masked rows / channels), still in registers
            ssq = fmaf(xv[j], xv[j], ssq);
          }
          ssq += swap_half(ssq);
          const float nrm = fast_sqrt(ssq);
          const float inv = fast_rcp(fmaxf(nrm, RMS_EPS));
          float dot = 0.f;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const float uh = xv[j] * inv;
            nacc0[j] = fmaf(tot[j], uh * sqC, nacc0[j]);  // d g_pre (this wave's nacc0: d g_out lives in head 0's wave)
            const float gd = tot[j] * gpre[j] * sqC;
            xv[j] = uh;
            tot[j] = gd;
            dot = fmaf(gd, uh, dot);
          }
          dot += swap_half(dot);
          const bool clamped = nrm < RMS_EPS;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int c = la_chan(C, j, half);
            if (row_ok && c < C) {
              const int64_t off = ((int64_t)row * C + c) * N + pos;
              const float du = clamped ? tot[j] * inv : inv * (tot[j] - xv[j] * dot);
              a.dx[off] = (pdx[b][j] + cd[b][j]) + du;  // cd: raw dy of this unit, still in registers
            }
          }
        }
      }
      if (!EX2) lds_barrier();  // (single exchange buffer: nobody overwrites it before the last head's wave has read it)
    }

    DQ_STAMP(2);
    // ---- flush this head's gradients to its sections of the BLOCK's partial slot (plain stores; the ordered reduce kernel sums the
    // slots): once per wave -- with the heads walked one after the other by every wave this was four flushes per wave
    float* slot = a.part + (int64_t)blockIdx.x * la_slot(C);
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 4 * g + i;
        // (dq_raw / dk_raw are gradients w.r.t. the natural-log logits: the log2(e) folded into the projection operands only
        // changes how the softmax is evaluated, not the function)
        const float vq = gq[g][i] + swap_half(gq[g][i]), vk = gk[g][i] + swap_half(gk[g][i]);
        if (half == 0) {  // lane = d
          slot[(hd * 32 + col) * C + c] = vq;
          slot[(128 + hd * 32 + col) * C + c] = vk;
        }
      }
    DQ_STAMP(10);
    // dW2 of this head: sum the 16 position blocks (lanes with equal lane & 3) and publish [c'][c] to the slot.  dWv = Wo^T dW2 and
    // dWo = dW2 Wv^T are linear in dW2, so they are formed ONCE per layer from the slot SUM (k_linattn_dwvo, after the ordered
    // reduce) instead of once per (wave, head) here: that was 2 C loads + C^2 FMAs + 2 C stores per lane and head (3-5 k of a
    // 7-12 k cycle flush at 12 / 16 channels, tools/probe/la_bwd_time.hip) and 256 C of the 515 C floats of a slot.
    // Inside a row of 16 lanes: two DPP rotations (by 4 and by 8 lanes) leave every lane with the sum of its (lane & 3) class;
    // across the four rows: through the wave-private tile (4 x 16 C^2 / 4 floats <= 1024).  The four-step ds_bpermute butterfly
    // this replaces was 4 C^2 dependent LDS round trips per head: 8 us of a 25 us head at 16 channels (tools/probe/la_bwd_time.hip).
    constexpr int NV4 = CG * CG * 16;  // floats one row contributes: [value vi = (g1 * CG + g2) * 4 + i][j = lane & 3]
    wave_fence();
#pragma unroll
    for (int g1 = 0; g1 < CG; ++g1)
#pragma unroll
      for (int g2 = 0; g2 < CG; ++g2)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v = gw2[g1][g2][i];
          v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xF, 0xF, false));  // row_ror:4
          v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false));  // row_ror:8
          if ((lane & 15) < 4) tile[(lane >> 4) * NV4 + ((g1 * CG + g2) * 4 + i) * 4 + (lane & 3)] = v;
        }
    wave_fence();
#pragma unroll
    for (int t = 0; t < (NV4 + 63) / 64; ++t) {
      const int e = lane + 64 * t;
      if (e < NV4) {
        const float v = (tile[e] + tile[NV4 + e]) + (tile[2 * NV4 + e] + tile[3 * NV4 + e]);
        const int vi = e >> 2, j = e & 3, i = vi & 3, g2 = (vi >> 2) % CG, g1 = (vi >> 2) / CG;
        w2g[(4 * g1 + i) * C + 4 * g2 + j] = v;
      }
    }
    wave_fence();
    DQ_STAMP(11);
    for (int i = lane; i < C * C; i += 64) slot[256 * C + hd * C * C + i] = w2g[i];
    constexpr int GB = la_slot_gains(C);  // [d g_out | d b_out | d g_pre]
    if (first || last) {  // norm gains / bias: sum over the 32 positions-lanes of this half, one lane stores
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = la_chan(C, j, half);
        const float s0 = half_sum(nacc0[j]), s1 = half_sum(nacc1[j]);
        if (col == 0 && c < C) {
          if (first) { slot[GB + c] = s0; slot[GB + C + c] = s1; }  // d g_out, d b_out
          else slot[GB + 2 * C + c] = s0;                          // d g_pre
        }
      }
    }
    DQ_STAMP(3);
  }
}

}  // namespace dq
