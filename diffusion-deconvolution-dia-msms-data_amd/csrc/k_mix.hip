// K-component training mixtures with per-window weights, formed on the GPU from a dataset that is resident in HBM:
// k_pairs.hip's batch formation for 1..K (K <= 8) windows per item instead of two, and for weights that are either K fixed scalars or
// drawn per window by the library's counter-based generator.  Window b mixes the components idx[j * B + b], j < count[b]; component 0 is
// the target.
//   n_j        = (x_j - lo) / (hi - lo)      MS2 lo / hi over all present components, MS1 lo / hi over component 0 only; no epsilon
//   ms2_cond   = ((n_0 w_0 + n_1 w_1) + n_2 w_2) + ...      every product rounded, every sum rounded (the library is built without FMA
//   ms2_rest   = (n_1 w_1 + n_2 w_2) + ...                  contraction), 0 for a single component
//   ms2_target = n_0, or the product n_0 w_0 that entered ms2_cond (scale_target)
// Drawn weights: a_j = (1 + m 2^-23) 2^e with m = r3 & 0x7fffff and e = ((r3 >> 23) * E) >> 9, r3 the FOURTH output word of philox4x32_10
// on counter (j, draw, id lo, id hi) under key (seed lo, seed hi) -- the normals read words 0 and 1, conditioning dropout word 2 of
// counter (0, ...), so no draw of a seed is shared; uniform within an octave and over E octaves, exact in fp32, no transcendental.
// s = ((a_0 + a_1) + a_2) + ... in fp32, w_j = a_j / s (correctly rounded division).  A window decides from (seed, id, draw) alone.
// A window with a used index outside [0, n_windows), or a count outside [1, K], is never dereferenced: every output of it is NaN.
//
// Two launches, like the pair form: (1) k_mix_minmax, grid (MIX_CHUNKS, B): each block reduces its chunk of every present component to a
// partial (min, max); block 0 of a window also reduces MS1 of component 0 and its first lane forms the window's weights once and writes
// weights_out.  (2) k_mix, grid (blocks per window, B): a block belongs to ONE window, so its count, indices, weights and the fold of the
// MIX_CHUNKS partials (fixed order) are wave-uniform scalar work done once per block, not per element; no Philox and no division of
// weights per element.  Both kernels run their element loop in a body instantiated per count (mix_dispatch), so that the loads of all
// present components of an element are in flight together.
// HBM-bound; algorithmic bytes per window: read count windows + write ms2_target, ms2_cond (and ms2_rest) = (count + 2 or 3) * RT*MZ*4 B
// (+ MS1 rows); the second read of the components in (2) comes from L2 / Infinity Cache.  No LDS beyond the block reduce, no atomics.
// dq_mix_group_batch (below) is the same rule for groups: one mixture, P targets, member-major outputs.
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_philox.h"
#include "../../include/dq_hip.h"
#include <algorithm>

namespace dq {

constexpr int MIX_CHUNKS = 8;
constexpr int MIX_MAX_K = 8;
constexpr int MIX_MAX_BLOCKS_X = 64;  // blocks of k_mix per window; a longer window is walked with this stride

struct MixWeights { float w[MIX_MAX_K]; };  // the fixed weights, by value
struct MixIdx {                               // a window's component indices
  int64_t v[MIX_MAX_K];
  __device__ __forceinline__ int64_t& operator[](int j) { return v[j]; }
  __device__ __forceinline__ int64_t operator[](int j) const { return v[j]; }
};

__device__ __forceinline__ float mix_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float mix_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float min4(float4 a) { return fminf(fminf(a.x, a.y), fminf(a.z, a.w)); }
__device__ __forceinline__ float max4(float4 a) { return fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)); }

// the abundance of component j of window `id` at draw `draw`: in [1, 2^E), exact in fp32 (a 24-bit significand times a power of two)
__device__ __forceinline__ float mix_abundance(uint64_t seed, int64_t id, uint32_t draw, uint32_t j, uint32_t E) {
  uint32_t c0 = j, c1 = draw, c2 = (uint32_t)((uint64_t)id & 0xffffffffu), c3 = (uint32_t)((uint64_t)id >> 32);
  philox4x32_10(c0, c1, c2, c3, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  if (E == 0) return 1.0f;
  const uint32_t m = c3 & 0x7fffffu, e = ((c3 >> 23) * E) >> 9;  // e in [0, E)
  return (1.0f + (float)m * 1.1920928955078125e-07f) * (float)(1u << e);
}

// window b's indices into ix (rows j >= count are never read: 0 stands in) and its count, or 0 if the count is outside [1, K] or a used
// index outside [0, n_windows).  b is the block's window: everything here is wave-uniform.
__device__ __forceinline__ int mix_window_indices(const int64_t* __restrict__ idx, const int32_t* __restrict__ count_p, int64_t n_windows,
                                                  int B, int K, int b, MixIdx& ix) {
  const int count = count_p ? count_p[b] : K;
  bool ok = count >= 1 && count <= K;
#pragma unroll
  for (int j = 0; j < MIX_MAX_K; ++j) {
    ix[j] = (ok && j < count) ? idx[(int64_t)j * B + b] : 0;
    ok = ok && ix[j] >= 0 && ix[j] < n_windows;
  }
  return ok ? count : 0;
}

// f.template operator()<C>() for C = count (1 .. MIX_MAX_K)
template <class F>
__device__ __forceinline__ void mix_dispatch(int count, F f) {
  switch (count) {
    case 1: f.template operator()<1>(); break;
    case 2: f.template operator()<2>(); break;
    case 3: f.template operator()<3>(); break;
    case 4: f.template operator()<4>(); break;
    case 5: f.template operator()<5>(); break;
    case 6: f.template operator()<6>(); break;
    case 7: f.template operator()<7>(); break;
    case 8: f.template operator()<8>(); break;
    default: break;
  }
}

struct MixMinMaxBody {
  const float4* base;
  MixIdx ix;
  int64_t per4, lo_i, hi_i;
  float &mn, &mx;
  template <int C>
  __device__ __forceinline__ void operator()() const {
    for (int64_t i = lo_i + threadIdx.x; i < hi_i; i += blockDim.x) {
      float4 a[C];
#pragma unroll
      for (int j = 0; j < C; ++j) a[j] = base[ix[j] * per4 + i];
#pragma unroll
      for (int j = 0; j < C; ++j) { mn = fminf(min4(a[j]), mn); mx = fmaxf(max4(a[j]), mx); }
    }
  }
};

// part: B * (MIX_CHUNKS + 1) * 2 floats ((min, max) per chunk, last slot = MS1).  wout: (B, K).
__global__ void __launch_bounds__(256) k_mix_minmax(const float* __restrict__ ms2, const float* __restrict__ ms1,
                                                    const int64_t* __restrict__ idx, const int32_t* __restrict__ count_p, int64_t n_windows,
                                                    int B, int K, int64_t per4, int64_t ms1_per, MixWeights fixed, int drawn, uint32_t E,
                                                    const uint64_t* __restrict__ seed_p, const int64_t* __restrict__ ids, uint32_t draw,
                                                    float* __restrict__ part, float* __restrict__ wout) {
  const int b = blockIdx.y, c = blockIdx.x;
  MixIdx ix;
  const int count = mix_window_indices(idx, count_p, n_windows, B, K, b, ix);
  float* pp = part + ((int64_t)b * (MIX_CHUNKS + 1) + c) * 2;
  if (count == 0) {  // never read out of bounds: poison the window instead
    if (threadIdx.x == 0) {
      pp[0] = pp[1] = NAN;
      if (c == 0) {
        pp[2 * MIX_CHUNKS] = pp[2 * MIX_CHUNKS + 1] = NAN;
        for (int j = 0; j < K; ++j) wout[(int64_t)b * K + j] = NAN;
      }
    }
    return;
  }
  float mn = INFINITY, mx = -INFINITY;
  mix_dispatch(count, MixMinMaxBody{reinterpret_cast<const float4*>(ms2), ix, per4, per4 * c / MIX_CHUNKS, per4 * (c + 1) / MIX_CHUNKS, mn, mx});
  __shared__ float red[2][4];
  mn = mix_wave_min(mn); mx = mix_wave_max(mx);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    pp[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    pp[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
  if (c != 0) return;
  // the window's weights, once
  if (threadIdx.x == 0) {
    float a[MIX_MAX_K];
    float* wb = wout + (int64_t)b * K;
    if (drawn) {
      const uint64_t seed = seed_p[0];
      const int64_t id = ids ? ids[b] : (int64_t)b;
      float s = 0.0f;
      for (int j = 0; j < count; ++j) {
        a[j] = mix_abundance(seed, id, draw, (uint32_t)j, E);
        s = j == 0 ? a[0] : s + a[j];
      }
      for (int j = 0; j < K; ++j) wb[j] = j < count ? a[j] / s : 0.0f;
    } else {
      for (int j = 0; j < K; ++j) wb[j] = j < count ? fixed.w[j] : 0.0f;
    }
  }
  // MS1 of component 0 only
  __syncthreads();
  const float* m = ms1 + ix[0] * ms1_per;
  mn = INFINITY; mx = -INFINITY;
  for (int64_t i = threadIdx.x; i < ms1_per; i += blockDim.x) { mn = fminf(mn, m[i]); mx = fmaxf(mx, m[i]); }
  mn = mix_wave_min(mn); mx = mix_wave_max(mx);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* p1 = part + ((int64_t)b * (MIX_CHUNKS + 1) + MIX_CHUNKS) * 2;
    p1[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    p1[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

__device__ __forceinline__ float4 mix_norm4(float4 v, float lo, float rng) {
  return make_float4((v.x - lo) / rng, (v.y - lo) / rng, (v.z - lo) / rng, (v.w - lo) / rng);
}
__device__ __forceinline__ float4 mul4(float4 v, float w) { return make_float4(v.x * w, v.y * w, v.z * w, v.w * w); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

struct MixBody {
  const float4* base;
  MixIdx ix;
  const float* wb;  // this window's row of weights_out
  float lo, rng;
  int64_t per4, first, stride;
  int scale_target;
  float4 *o_target, *o_cond, *o_rest;  // this window's; o_rest nullable
  template <int C>
  __device__ __forceinline__ void operator()() const {
    float w[C];
#pragma unroll
    for (int j = 0; j < C; ++j) w[j] = wb[j];
    for (int64_t e = first; e < per4; e += stride) {
      float4 v[C];
#pragma unroll
      for (int j = 0; j < C; ++j) v[j] = base[ix[j] * per4 + e];
      const float4 n0 = mix_norm4(v[0], lo, rng);
      float4 cond = mul4(n0, w[0]), rest = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      // (selected per component: a select between two float4 aggregates is compiled into an indexed private array, i.e. scratch)
      o_target[e] = make_float4(scale_target ? cond.x : n0.x, scale_target ? cond.y : n0.y, scale_target ? cond.z : n0.z,
                                scale_target ? cond.w : n0.w);
#pragma unroll
      for (int j = 1; j < C; ++j) {
        const float4 p = mul4(mix_norm4(v[j], lo, rng), w[j]);
        cond = add4(cond, p);
        rest = j == 1 ? p : add4(rest, p);
      }
      o_cond[e] = cond;
      if (o_rest) o_rest[e] = rest;
    }
  }
};

__global__ void __launch_bounds__(256) k_mix(const float* __restrict__ ms2, const float* __restrict__ ms1, const int64_t* __restrict__ idx,
                                             const int32_t* __restrict__ count_p, int64_t n_windows, int B, int K, int64_t per4,
                                             int64_t ms1_per, const float* __restrict__ part, const float* __restrict__ wout,
                                             int scale_target, float* __restrict__ o_target, float* __restrict__ o_ms1,
                                             float* __restrict__ o_cond, float* __restrict__ o_rest) {
  const int b = blockIdx.y;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  MixIdx ix;
  const int count = mix_window_indices(idx, count_p, n_windows, B, K, b, ix);
  float4* t4 = reinterpret_cast<float4*>(o_target) + (int64_t)b * per4;
  float4* c4 = reinterpret_cast<float4*>(o_cond) + (int64_t)b * per4;
  float4* r4 = o_rest ? reinterpret_cast<float4*>(o_rest) + (int64_t)b * per4 : nullptr;
  float* m1 = o_ms1 + (int64_t)b * ms1_per;
  if (count == 0) {
    const float4 nan4 = make_float4(NAN, NAN, NAN, NAN);
    for (int64_t e = first; e < per4; e += stride) {
      t4[e] = nan4;
      c4[e] = nan4;
      if (r4) r4[e] = nan4;
    }
    for (int64_t e = first; e < ms1_per; e += stride) m1[e] = NAN;
    return;
  }
  const float* pp = part + (int64_t)b * (MIX_CHUNKS + 1) * 2;
  float lo = pp[0], hi = pp[1];
#pragma unroll
  for (int c = 1; c < MIX_CHUNKS; ++c) { lo = fminf(lo, pp[2 * c]); hi = fmaxf(hi, pp[2 * c + 1]); }
  {
    const float lo1 = pp[2 * MIX_CHUNKS], rng1 = pp[2 * MIX_CHUNKS + 1] - lo1;
    const float* src = ms1 + ix[0] * ms1_per;
    for (int64_t e = first; e < ms1_per; e += stride) m1[e] = (src[e] - lo1) / rng1;
  }
  mix_dispatch(count, MixBody{reinterpret_cast<const float4*>(ms2), ix, wout + (int64_t)b * K, lo, hi - lo, per4, first, stride, scale_target,
                              t4, c4, r4});
}

// ---- groups: one mixture of count[g] components whose first P are the MEMBERS that joint sampling asks for.  The same
// rule as above for lo / hi, the weights and ms2_cond; every member gets its own target n_p (or n_p w_p), its own MS1 under its own MS1
// lo / hi, and a copy of the mixture; ms2_rest is what no member explains.  Outputs are member-major: member p of group g is row p * G + g.
// A group's count must lie in [P, K].  part: G * (MIX_CHUNKS + P) * 2 floats ((min, max) per chunk, then one pair per member's MS1).

__device__ __forceinline__ int mix_group_indices(const int64_t* __restrict__ idx, const int32_t* __restrict__ count_p, int64_t n_windows,
                                                 int G, int K, int P, int g, MixIdx& ix) {
  const int count = mix_window_indices(idx, count_p, n_windows, G, K, g, ix);
  return count >= P ? count : 0;
}

__global__ void __launch_bounds__(256) k_mix_group_minmax(const float* __restrict__ ms2, const float* __restrict__ ms1,
                                                          const int64_t* __restrict__ idx, const int32_t* __restrict__ count_p,
                                                          int64_t n_windows, int G, int K, int P, int64_t per4, int64_t ms1_per,
                                                          MixWeights fixed, int drawn, uint32_t E, const uint64_t* __restrict__ seed_p,
                                                          const int64_t* __restrict__ ids, uint32_t draw, float* __restrict__ part,
                                                          float* __restrict__ wout) {
  const int g = blockIdx.y, c = blockIdx.x;
  MixIdx ix;
  const int count = mix_group_indices(idx, count_p, n_windows, G, K, P, g, ix);
  float* pg = part + (int64_t)g * (MIX_CHUNKS + P) * 2;
  float* pp = pg + c * 2;
  if (count == 0) {  // never read out of bounds: poison the group instead
    if (threadIdx.x == 0) {
      pp[0] = pp[1] = NAN;
      if (c == 0) {
        for (int p = 0; p < P; ++p) pg[2 * (MIX_CHUNKS + p)] = pg[2 * (MIX_CHUNKS + p) + 1] = NAN;
        for (int j = 0; j < K; ++j) wout[(int64_t)g * K + j] = NAN;
      }
    }
    return;
  }
  float mn = INFINITY, mx = -INFINITY;
  mix_dispatch(count, MixMinMaxBody{reinterpret_cast<const float4*>(ms2), ix, per4, per4 * c / MIX_CHUNKS, per4 * (c + 1) / MIX_CHUNKS, mn, mx});
  __shared__ float red[2][4];
  mn = mix_wave_min(mn); mx = mix_wave_max(mx);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    pp[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    pp[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
  if (c != 0) return;
  // the group's weights, once: k_mix_minmax's, keyed by the group's id
  if (threadIdx.x == 0) {
    float a[MIX_MAX_K];
    float* wb = wout + (int64_t)g * K;
    if (drawn) {
      const uint64_t seed = seed_p[0];
      const int64_t id = ids ? ids[g] : (int64_t)g;
      float s = 0.0f;
      for (int j = 0; j < count; ++j) {
        a[j] = mix_abundance(seed, id, draw, (uint32_t)j, E);
        s = j == 0 ? a[0] : s + a[j];
      }
      for (int j = 0; j < K; ++j) wb[j] = j < count ? a[j] / s : 0.0f;
    } else {
      for (int j = 0; j < K; ++j) wb[j] = j < count ? fixed.w[j] : 0.0f;
    }
  }
  // MS1 of every member, each under its own lo / hi
  for (int p = 0; p < P; ++p) {
    __syncthreads();
    const float* m = ms1 + idx[(int64_t)p * G + g] * ms1_per;  // (checked above; ix[p] with a run-time p would make ix an indexed array)
    mn = INFINITY; mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < ms1_per; i += blockDim.x) { mn = fminf(mn, m[i]); mx = fmaxf(mx, m[i]); }
    mn = mix_wave_min(mn); mx = mix_wave_max(mx);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      pg[2 * (MIX_CHUNKS + p)] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
      pg[2 * (MIX_CHUNKS + p) + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
  }
}

struct MixGroupBody {
  const float4* base;
  MixIdx ix;
  const float* wb;  // this group's row of weights_out
  float lo, rng;
  int64_t per4, first, stride, member;  // member: the float4 between two members of a group, G * per4
  int P, scale_target;
  float4 *o_target, *o_cond, *o_rest;  // member 0's slice of this group; o_rest (nullable) the group's
  template <int C>
  __device__ __forceinline__ void operator()() const {
    float w[C];
#pragma unroll
    for (int j = 0; j < C; ++j) w[j] = wb[j];
    for (int64_t e = first; e < per4; e += stride) {
      float4 v[C];
#pragma unroll
      for (int j = 0; j < C; ++j) v[j] = base[ix[j] * per4 + e];
      float4 cond = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rest = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int j = 0; j < C; ++j) {
        const float4 n = mix_norm4(v[j], lo, rng);
        const float4 p = mul4(n, w[j]);
        cond = j == 0 ? p : add4(cond, p);
        if (j < P) {  // (P is uniform over the block: a scalar branch around one store)
          o_target[j * member + e] = make_float4(scale_target ? p.x : n.x, scale_target ? p.y : n.y, scale_target ? p.z : n.z,
                                                 scale_target ? p.w : n.w);
        } else if (j == P) {
          rest = p;
        } else {
          rest = add4(rest, p);
        }
      }
#pragma unroll
      for (int j = 0; j < C; ++j)
        if (j < P) o_cond[j * member + e] = cond;
      if (o_rest) o_rest[e] = rest;
    }
  }
};

__global__ void __launch_bounds__(256) k_mix_group(const float* __restrict__ ms2, const float* __restrict__ ms1,
                                                   const int64_t* __restrict__ idx, const int32_t* __restrict__ count_p, int64_t n_windows,
                                                   int G, int K, int P, int64_t per4, int64_t ms1_per, const float* __restrict__ part,
                                                   const float* __restrict__ wout, int scale_target, float* __restrict__ o_target,
                                                   float* __restrict__ o_ms1, float* __restrict__ o_cond, float* __restrict__ o_rest) {
  const int g = blockIdx.y;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  MixIdx ix;
  const int count = mix_group_indices(idx, count_p, n_windows, G, K, P, g, ix);
  const int64_t member = (int64_t)G * per4;
  float4* t4 = reinterpret_cast<float4*>(o_target) + (int64_t)g * per4;
  float4* c4 = reinterpret_cast<float4*>(o_cond) + (int64_t)g * per4;
  float4* r4 = o_rest ? reinterpret_cast<float4*>(o_rest) + (int64_t)g * per4 : nullptr;
  float* m1 = o_ms1 + (int64_t)g * ms1_per;
  if (count == 0) {
    const float4 nan4 = make_float4(NAN, NAN, NAN, NAN);
    for (int64_t e = first; e < per4; e += stride) {
      for (int p = 0; p < P; ++p) {
        t4[p * member + e] = nan4;
        c4[p * member + e] = nan4;
      }
      if (r4) r4[e] = nan4;
    }
    for (int p = 0; p < P; ++p)
      for (int64_t e = first; e < ms1_per; e += stride) m1[(int64_t)p * G * ms1_per + e] = NAN;
    return;
  }
  const float* pg = part + (int64_t)g * (MIX_CHUNKS + P) * 2;
  float lo = pg[0], hi = pg[1];
#pragma unroll
  for (int c = 1; c < MIX_CHUNKS; ++c) { lo = fminf(lo, pg[2 * c]); hi = fmaxf(hi, pg[2 * c + 1]); }
  for (int p = 0; p < P; ++p) {
    const float lo1 = pg[2 * (MIX_CHUNKS + p)], rng1 = pg[2 * (MIX_CHUNKS + p) + 1] - lo1;
    const float* src = ms1 + idx[(int64_t)p * G + g] * ms1_per;
    float* dst = m1 + (int64_t)p * G * ms1_per;
    for (int64_t e = first; e < ms1_per; e += stride) dst[e] = (src[e] - lo1) / rng1;
  }
  mix_dispatch(count, MixGroupBody{reinterpret_cast<const float4*>(ms2), ix, wout + (int64_t)g * K, lo, hi - lo, per4, first, stride, member, P,
                                   scale_target, t4, c4, r4});
}

}  // namespace dq

extern "C" {

int64_t dq_mix_group_batch_scratch_bytes(int G, int K, int P) {
  if (G <= 0 || G > 65535 || K < 2 || K > dq::MIX_MAX_K || P < 1 || P > K) return 0;
  return (int64_t)G * (dq::MIX_CHUNKS + P) * 2 * (int64_t)sizeof(float);
}

int dq_mix_group_batch(const float* ms2_data, const float* ms1_data, int64_t n_windows, const int64_t* idx_dev, const int32_t* count_dev,
                       int G, int K, int P, int RT, int MZ, int64_t ms1_per_window, const float* weights_host, int max_ratio_log2,
                       const uint64_t* seed_dev, const int64_t* window_ids_dev, int draw, int scale_target, float* ms2_target,
                       float* ms1_target, float* ms2_cond, float* ms2_rest, float* weights_out, void* scratch, int64_t scratch_bytes,
                       void* stream) {
  using namespace dq;
  DQ_REQUIRE(ms2_data && ms1_data && idx_dev && ms2_target && ms1_target && ms2_cond && weights_out && scratch,
             "dq_mix_group_batch: null argument");
  DQ_REQUIRE(K >= 2 && K <= MIX_MAX_K, "dq_mix_group_batch: K must be 2..8 components");
  DQ_REQUIRE(P >= 1 && P <= K, "dq_mix_group_batch: group_size must be 1..K members");
  DQ_REQUIRE(max_ratio_log2 >= 0 && max_ratio_log2 <= 16, "dq_mix_group_batch: max_ratio_log2 must be 0..16");
  DQ_REQUIRE(draw >= 0, "dq_mix_group_batch: the draw index must be >= 0");
  DQ_REQUIRE(G >= 1 && G <= 65535, "dq_mix_group_batch: 1..65535 groups per call");
  DQ_REQUIRE(RT > 0 && MZ > 0 && ms1_per_window > 0 && n_windows > 0, "dq_mix_group_batch: sizes must be positive");
  const int64_t per = (int64_t)RT * MZ;
  DQ_REQUIRE(per % 4 == 0, "dq_mix_group_batch: RT*MZ must be a multiple of 4");
  DQ_REQUIRE(weights_host || seed_dev, "dq_mix_group_batch: drawn weights need the seed (seed_dev)");
  DQ_REQUIRE(scratch_bytes >= dq_mix_group_batch_scratch_bytes(G, K, P),
             "dq_mix_group_batch: scratch too small (dq_mix_group_batch_scratch_bytes)");
  hipStream_t s = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(scratch);
  MixWeights fixed{};
  if (weights_host)
    for (int j = 0; j < K; ++j) fixed.w[j] = weights_host[j];
  hipLaunchKernelGGL(k_mix_group_minmax, dim3(MIX_CHUNKS, G), dim3(256), 0, s, ms2_data, ms1_data, idx_dev, count_dev, n_windows, G, K, P,
                     per / 4, ms1_per_window, fixed, weights_host ? 0 : 1, (uint32_t)max_ratio_log2, seed_dev, window_ids_dev, (uint32_t)draw,
                     part, weights_out);
  DQ_LAUNCH_CHECK();
  // k_mix's grid: a block's group is blockIdx.y; the members' MS1 rows ride in the same blocks as the group's per / 4 float4
  const int gx = (int)std::min<int64_t>(cdiv(std::max(per / 4, ms1_per_window), 256), MIX_MAX_BLOCKS_X);
  hipLaunchKernelGGL(k_mix_group, dim3(gx, G), dim3(256), 0, s, ms2_data, ms1_data, idx_dev, count_dev, n_windows, G, K, P, per / 4,
                     ms1_per_window, part, weights_out, scale_target, ms2_target, ms1_target, ms2_cond, ms2_rest);
  DQ_LAUNCH_CHECK();
  return 0;
}

// (the partials do not depend on K: the weights live in weights_out.  K is part of the signature so that a form that needs it can ask.)
int64_t dq_mix_batch_scratch_bytes(int B, int K) {
  if (B <= 0 || K < 2 || K > dq::MIX_MAX_K) return 0;
  return (int64_t)B * (dq::MIX_CHUNKS + 1) * 2 * (int64_t)sizeof(float);
}

int dq_mix_batch(const float* ms2_data, const float* ms1_data, int64_t n_windows, const int64_t* idx_dev, const int32_t* count_dev, int B,
                 int K, int RT, int MZ, int64_t ms1_per_window, const float* weights_host, int max_ratio_log2, const uint64_t* seed_dev,
                 const int64_t* window_ids_dev, int draw, int scale_target, float* ms2_target, float* ms1_target, float* ms2_cond,
                 float* ms2_rest, float* weights_out, void* scratch, int64_t scratch_bytes, void* stream) {
  using namespace dq;
  DQ_REQUIRE(ms2_data && ms1_data && idx_dev && ms2_target && ms1_target && ms2_cond && weights_out && scratch,
             "dq_mix_batch: null argument");
  DQ_REQUIRE(K >= 2 && K <= MIX_MAX_K, "dq_mix_batch: K must be 2..8 components");
  DQ_REQUIRE(max_ratio_log2 >= 0 && max_ratio_log2 <= 16, "dq_mix_batch: max_ratio_log2 must be 0..16");
  DQ_REQUIRE(draw >= 0, "dq_mix_batch: the draw index must be >= 0");
  DQ_REQUIRE(B >= 1 && B <= 65535, "dq_mix_batch: 1..65535 windows per call");
  DQ_REQUIRE(RT > 0 && MZ > 0 && ms1_per_window > 0 && n_windows > 0, "dq_mix_batch: sizes must be positive");
  const int64_t per = (int64_t)RT * MZ;
  DQ_REQUIRE(per % 4 == 0, "dq_mix_batch: RT*MZ must be a multiple of 4");
  DQ_REQUIRE(weights_host || seed_dev, "dq_mix_batch: drawn weights need the seed (seed_dev)");
  DQ_REQUIRE(scratch_bytes >= dq_mix_batch_scratch_bytes(B, K), "dq_mix_batch: scratch too small (dq_mix_batch_scratch_bytes)");
  hipStream_t s = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(scratch);
  MixWeights fixed{};
  if (weights_host)
    for (int j = 0; j < K; ++j) fixed.w[j] = weights_host[j];
  hipLaunchKernelGGL(k_mix_minmax, dim3(MIX_CHUNKS, B), dim3(256), 0, s, ms2_data, ms1_data, idx_dev, count_dev, n_windows, B, K, per / 4,
                     ms1_per_window, fixed, weights_host ? 0 : 1, (uint32_t)max_ratio_log2, seed_dev, window_ids_dev, (uint32_t)draw, part,
                     weights_out);
  DQ_LAUNCH_CHECK();
  // one block's window is blockIdx.y; MS1 (ms1_per elements) rides in the same blocks as the window's per / 4 float4
  const int gx = (int)std::min<int64_t>(cdiv(std::max(per / 4, ms1_per_window), 256), MIX_MAX_BLOCKS_X);
  hipLaunchKernelGGL(k_mix, dim3(gx, B), dim3(256), 0, s, ms2_data, ms1_data, idx_dev, count_dev, n_windows, B, K, per / 4, ms1_per_window,
                     part, weights_out, scale_target, ms2_target, ms1_target, ms2_cond, ms2_rest);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
