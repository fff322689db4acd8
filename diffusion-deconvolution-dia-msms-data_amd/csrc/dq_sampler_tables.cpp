// The samplers' per-step coefficient tables: dq_ddim_coef_table, dq_sampler_coef_table (include/dq_hip.h) and the one row builder behind
// them and behind dq_ddim_sample (dq_sampler.hip).  Host C++ alone: no HIP call, and it compiles with a plain host compiler.
#include "dq_sampler_tables.h"
#include "dq_error.h"
#include "../../include/dq_hip.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace dq {

// Step i runs at t = ts[i].  Where it lands and which row is terminal (returns x0: [sa, sb, -1, 0]) depend on the kind:
//   DQ_SAMPLER_REFERENCE  lands on alpha_bars[t - 1], terminal iff t == 0, any list (model.py:265-267, 284-286);
//   every other kind      lands on alpha_bars[ts[i + 1]], terminal iff i == n - 1, ts strictly decreasing.
// DQ_SAMPLER_REFERENCE and DQ_SAMPLER_DDIM, [sa, sb, sap, c] and sigma: sa, sb, sap and, at eta == 0, c the fp32 expressions they always were
// (x0 and eps are derived as before); eta > 0: sigma and c in double from the fp32 table values.  DQ_SAMPLER_DPMPP_2M, [sa, sb, cx, c0] and c1:
// in double from the fp32 table values; SOLVER_ORDER1: the same rows with c1 = 0 everywhere.
int sampler_rows(const float* ab_tab, int T, const int32_t* ts, int n, int kind, float eta, float* coef_out, float* extra_out, const char* who) {
  const bool strided = kind != DQ_SAMPLER_REFERENCE;
  for (int i = 0; i < n; ++i) {
    if (ts[i] < 0 || ts[i] >= T) { set_error(std::string(who) + ": timestep out of range"); return 1; }
    if (strided && i > 0 && ts[i] >= ts[i - 1]) { set_error(std::string(who) + ": the timesteps of this sampler must be strictly decreasing"); return 1; }
  }
  double h_prev = 0.0;
  for (int i = 0; i < n; ++i) {
    const int t = ts[i];
    const float ab = ab_tab[t];
    const bool last = strided ? i == n - 1 : t == 0;
    extra_out[i] = 0.f;
    if (kind == DQ_SAMPLER_REFERENCE || kind == DQ_SAMPLER_DDIM) {
      coef_out[4 * i + 0] = std::sqrt(ab);
      coef_out[4 * i + 1] = std::sqrt(1.0f - ab);
      if (last) { coef_out[4 * i + 2] = -1.f; coef_out[4 * i + 3] = 0.f; continue; }
      const float abp = ab_tab[strided ? ts[i + 1] : t - 1];
      coef_out[4 * i + 2] = std::sqrt(abp);
      coef_out[4 * i + 3] = std::sqrt(1.0f - abp);
      if (eta > 0.f) {
        const double a = (double)ab, ap = (double)abp;
        // (a degenerate schedule -- alpha_bar of 0 or 1, or one that rises -- gets sigma = 0 instead of a NaN)
        const double ratio = ap > 0.0 ? std::min(a / ap, 1.0) : 1.0;
        const double sg = (1.0 - a) > 0.0 ? (double)eta * std::sqrt((1.0 - ap) / (1.0 - a)) * std::sqrt(1.0 - ratio) : 0.0;
        coef_out[4 * i + 3] = (float)std::sqrt(std::max(0.0, 1.0 - ap - sg * sg));
        extra_out[i] = (float)sg;
      }
      continue;
    }
    const double al = std::sqrt((double)ab), sg = std::sqrt(1.0 - (double)ab);
    coef_out[4 * i + 0] = (float)al;
    coef_out[4 * i + 1] = (float)sg;
    if (last) { coef_out[4 * i + 2] = -1.f; coef_out[4 * i + 3] = 0.f; continue; }
    const double abp = (double)ab_tab[ts[i + 1]];
    const double alp = std::sqrt(abp), sgp = std::sqrt(1.0 - abp);
    // h = lambda_{i+1} - lambda_i, lambda = log(alpha / sigma); a schedule end with sigma or alpha exactly 0 gives h = inf: 1 - e^-h = 1
    const double h = std::log(alp / sgp) - std::log(al / sg);
    const double em = std::isnan(h) ? 1.0 : -std::expm1(-h);
    const double base = alp * em;
    double c0 = base, c1 = 0.0;
    const bool second = kind == DQ_SAMPLER_DPMPP_2M && i >= 1 && std::isfinite(h) && h > 0.0 && std::isfinite(h_prev) && h_prev > 0.0;
    if (second) {
      const double r = h_prev / h;
      c0 = base * (1.0 + 1.0 / (2.0 * r));
      c1 = -base / (2.0 * r);
    }
    coef_out[4 * i + 2] = sg > 0.0 ? (float)(sgp / sg) : 0.f;
    coef_out[4 * i + 3] = (float)c0;
    extra_out[i] = (float)c1;
    h_prev = h;
  }
  return 0;
}

}  // namespace dq

extern "C" {

int dq_ddim_coef_table(const float* alpha_bars_host, int num_timesteps, const int32_t* timesteps_host, int num_steps, float eta,
                       float* coef_out, float* sigma_out) {
  DQ_REQUIRE(alpha_bars_host && timesteps_host && coef_out && sigma_out, "dq_ddim_coef_table: null argument");
  DQ_REQUIRE(num_timesteps >= 1 && num_steps >= 1, "dq_ddim_coef_table: num_timesteps and num_steps must be >= 1");
  DQ_REQUIRE(eta >= 0.f && eta <= 1.f, "dq_ddim_coef_table: eta must satisfy 0 <= eta <= 1");  // (false for NaN)
  for (int i = 0; i < num_steps; ++i) {  // (this entry's own refusal, as it always read; the builder's check then never fires)
    const int t = timesteps_host[i];
    DQ_REQUIRE(t >= 0 && t < num_timesteps, "dq_ddim_coef_table: timestep out of range");
  }
  return dq::sampler_rows(alpha_bars_host, num_timesteps, timesteps_host, num_steps, DQ_SAMPLER_REFERENCE, eta, coef_out, sigma_out,
                          "dq_ddim_coef_table");
}

int dq_sampler_coef_table(const float* alpha_bars_host, int num_timesteps, const int32_t* timesteps_host, int num_steps, int sampler,
                          float eta, float* coef_out, float* extra_out) {
  DQ_REQUIRE(alpha_bars_host && timesteps_host && coef_out && extra_out, "dq_sampler_coef_table: null argument");
  DQ_REQUIRE(num_timesteps >= 1 && num_steps >= 1, "dq_sampler_coef_table: num_timesteps and num_steps must be >= 1");
  DQ_REQUIRE(sampler == DQ_SAMPLER_REFERENCE || sampler == DQ_SAMPLER_DDIM || sampler == DQ_SAMPLER_DPMPP_2M,
             "dq_sampler_coef_table: unknown sampler");
  DQ_REQUIRE(eta >= 0.f && eta <= 1.f, "dq_sampler_coef_table: eta must satisfy 0 <= eta <= 1");  // (false for NaN)
  if (sampler == DQ_SAMPLER_REFERENCE) return dq_ddim_coef_table(alpha_bars_host, num_timesteps, timesteps_host, num_steps, eta, coef_out, extra_out);
  DQ_REQUIRE(sampler != DQ_SAMPLER_DPMPP_2M || eta == 0.f, "dq_sampler_coef_table: DPM-Solver++(2M) is deterministic: eta must be 0");
  return dq::sampler_rows(alpha_bars_host, num_timesteps, timesteps_host, num_steps, sampler, eta, coef_out, extra_out, "dq_sampler_coef_table");
}

}  // extern "C"
