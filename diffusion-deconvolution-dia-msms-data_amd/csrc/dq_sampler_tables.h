// The samplers' per-step coefficient rows (dq_sampler_tables.cpp; host only, free of HIP).
#pragma once
#include <cstdint>

namespace dq {

// a row kind beside DQ_SAMPLER_* (include/dq_hip.h), not part of the ABI: the first-order solver rows, DQ_SAMPLER_DPMPP_2M's with c1 = 0
// everywhere (strided DDIM as a solver row: what clip_x0 runs)
constexpr int SOLVER_ORDER1 = 3;

// Fills coef_out (4 n floats) and extra_out (n floats) for the steps ts[0 .. n); `who` prefixes the refusals.  Non-zero after set_error().
int sampler_rows(const float* alpha_bars, int T, const int32_t* ts, int n, int kind, float eta, float* coef_out, float* extra_out, const char* who);

}  // namespace dq
