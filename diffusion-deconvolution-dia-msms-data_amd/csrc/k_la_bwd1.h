// LinearAttention backward for rows of ONE position (the deepest level of the default U-Net): the closed form of k_la_bwd.h, a kernel
// template instantiated by the host dispatch (k_la_bwd.hip; tools/probe/la_bwd_time.hip times it).
#pragma once
#include "k_la_bwd.h"  // LinAttnBwdK

namespace dq {

// Rows of ONE position (the deepest level of the default U-Net): a closed form.  The softmax over a single position is 1 and the q
// softmax sums to 1, so S = 32^-0.5 whatever Wq and Wk are: R = 32^-0.5 xh, dWq = dWk = 0, dXh = 32^-0.5 (sum_h W2_h)^T dYpre and
// dW2_h = dYpre (32^-0.5 xh)^T for every head.  One wave per 32 rows (lane = (row, channel half)), per-WAVE slots in the layout of
// k_linattn_bwd (the q / k sections are written as zeros, the dW2 section four times).
template <int C>
__global__ void __launch_bounds__(256) k_linattn_bwd1(LinAttnBwdK a) {
  constexpr int NJ = la_nj(C), CG = C / 4, NP = 32;
  __shared__ __attribute__((aligned(16))) float w2_lds[4 * C * C];
  __shared__ __attribute__((aligned(16))) float tiles[4][32 * TRP36];
  __shared__ __attribute__((aligned(16))) float stage[4][3 * C * NP + C * C];  // per wave: xh | dYpre | 32^-0.5 xh as [c][row] ; dW2
  if (a.prep) {
    for (int i = threadIdx.x; i < 4 * C * C; i += blockDim.x) w2_lds[i] = a.prep[i];
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
  for (int i = threadIdx.x; i < C * C; i += blockDim.x)  // sum_h W2_h into slot 0
    w2_lds[i] = ((w2_lds[i] + w2_lds[C * C + i]) + w2_lds[2 * C * C + i]) + w2_lds[3 * C * C + i];
  __syncthreads();

  const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  float* tile = tiles[wv];
  float* xs = stage[wv];
  float* dys = xs + C * NP;
  float* ps = dys + C * NP;
  float* w2g = ps + C * NP;
  const int wave_id = blockIdx.x * (blockDim.x >> 6) + wv;
  const int n_units = (a.rows + 31) / 32;
  const int u0 = wave_id * a.units_per_wave;
  if (u0 >= n_units) return;
  const int u1 = min(n_units, u0 + a.units_per_wave);
  const float sqC = sqrtf((float)C);
  float gpre[NJ], gout[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = la_chan(C, j, half);
    gpre[j] = c < C ? a.g_pre[c] : 0.f;
    gout[j] = c < C ? a.g_out[c] : 0.f;
  }
  f32x4 gw2[CG][CG];  // dW2[c' = 4*g1 + i][c = 4*g2 + (lane&3)], partial over the rows of this 4-lane block
#pragma unroll
  for (int g = 0; g < CG; ++g)
#pragma unroll
    for (int g2 = 0; g2 < CG; ++g2) gw2[g][g2] = f32x4{0.f, 0.f, 0.f, 0.f};
  float nacc0[NJ], nacc1[NJ], nacc2[NJ];  // d g_out, d b_out, d g_pre
#pragma unroll
  for (int j = 0; j < NJ; ++j) nacc0[j] = nacc1[j] = nacc2[j] = 0.f;

#pragma unroll 1
  for (int u = u0; u < u1; ++u) {
    const int row = u * 32 + col;
    const bool row_ok = row < a.rows;
    float xv[NJ], uv[NJ], dv_[NJ], Xh[NJ], DY[NJ], pdx[NJ];
    float ssq = 0.f, usq = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = la_chan(C, j, half);
      const bool ok = row_ok && c < C;
      const int64_t off = (int64_t)row * C + c;
      xv[j] = ok ? a.x[off] : 0.f;
      uv[j] = ok ? a.ypre[off] : 0.f;
      dv_[j] = ok ? a.dy[off] : 0.f;
      pdx[j] = (ok && !a.dx_store) ? a.dx[off] : 0.f;
      ssq = fmaf(xv[j], xv[j], ssq);
      usq = fmaf(uv[j], uv[j], usq);
    }
    // ---- pre-norm recompute; post-norm backward (same arithmetic as k_block_bwd) -> DY = dYpre
    ssq += swap_half(ssq);
    usq += swap_half(usq);
    const float nrm = fast_sqrt(ssq);
    const float inv = sqC * fast_rcp(fmaxf(nrm, RMS_EPS));
    const float unrm = fast_sqrt(usq);
    const float uinv = fast_rcp(fmaxf(unrm, RMS_EPS));
    float dot = 0.f;
    float gdv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      Xh[j] = xv[j] * inv * gpre[j];
      const float uh = uv[j] * uinv;
      nacc0[j] = fmaf(dv_[j], uh * sqC, nacc0[j]);  // d g_out
      gdv[j] = dv_[j] * gout[j] * sqC;
      uv[j] = uh;
      dot = fmaf(gdv[j], uh, dot);
    }
    dot += swap_half(dot);
    const bool uclamped = unrm < RMS_EPS;  // F.normalize clamps the norm: below eps the map is linear
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      DY[j] = uclamped ? gdv[j] * uinv : uinv * (gdv[j] - uv[j] * dot);
      nacc1[j] += DY[j];  // d b_out (bias of to_out)
    }
    // stage xh, 32^-0.5 xh and dYpre as [c][row]: 4x4x1 operands, and every lane needs ALL channels of dYpre of its row
    wave_fence();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = la_chan(C, j, half);
      if (c < C) {
        xs[c * NP + col] = Xh[j];
        ps[c * NP + col] = ATT_SCALE * Xh[j];
        dys[c * NP + col] = DY[j];
      }
    }
    wave_fence();
    // dR[c] = sum_c' (sum_h W2_h)[c'][c] dYpre[c'] ; dXh = 32^-0.5 dR
    float dR[C];
    {
      float dya[C];
#pragma unroll
      for (int c = 0; c < C; ++c) { dya[c] = dys[c * NP + col]; dR[c] = 0.f; }
#pragma unroll
      for (int cp = 0; cp < C; ++cp)
#pragma unroll
        for (int c = 0; c < C; ++c) dR[c] = fmaf(w2_lds[cp * C + c], dya[cp], dR[c]);
    }
    // dW2[c'][c] += sum_rows dYpre[c'][row] (32^-0.5 xh)[c][row]: row = 16 * s + (lane >> 2)
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
    // ---- residual + pre-norm backward on dXh (own channels); dx += dy + d/dx
    const float pinv = fast_rcp(fmaxf(nrm, RMS_EPS));
    float tot[NJ], uh2[NJ];
    float dot2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c0 = la_chan(C, j, 0), c1 = la_chan(C, j, 1);
      const float lo = c0 < C ? dR[c0 < C ? c0 : 0] : 0.f, hi = c1 < C ? dR[c1 < C ? c1 : 0] : 0.f;
      const float dxh = row_ok ? ATT_SCALE * (half ? hi : lo) : 0.f;
      uh2[j] = xv[j] * pinv;
      nacc2[j] = fmaf(dxh, uh2[j] * sqC, nacc2[j]);  // d g_pre
      tot[j] = dxh * gpre[j] * sqC;
      dot2 = fmaf(tot[j], uh2[j], dot2);
    }
    dot2 += swap_half(dot2);
    const bool clamped = nrm < RMS_EPS;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = la_chan(C, j, half);
      if (row_ok && c < C) {
        const float du = clamped ? tot[j] * pinv : pinv * (tot[j] - uh2[j] * dot2);
        a.dx[(int64_t)row * C + c] = (pdx[j] + dv_[j]) + du;
      }
    }
  }

  // ---- flush: zeros for dWq | dWk, the block sum of dW2 for each of the four heads, the gains
  float* slot = a.part + (int64_t)wave_id * la_slot(C);
  for (int i = lane; i < 256 * C; i += 64) slot[i] = 0.f;
  constexpr int NV4 = CG * CG * 16;
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
  for (int i = lane; i < C * C; i += 64) {
    const float v = w2g[i];
#pragma unroll
    for (int hd = 0; hd < 4; ++hd) slot[256 * C + hd * C * C + i] = v;
  }
  constexpr int GB = la_slot_gains(C);  // [d g_out | d b_out | d g_pre]
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = la_chan(C, j, half);
    const float s0 = half_sum(nacc0[j]), s1 = half_sum(nacc1[j]), s2 = half_sum(nacc2[j]);
    if (col == 0 && c < C) { slot[GB + c] = s0; slot[GB + C + c] = s1; slot[GB + 2 * C + c] = s2; }
  }
}

}  // namespace dq
