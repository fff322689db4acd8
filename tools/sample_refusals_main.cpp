// Stand-alone host program for a sanitizer build (see the comment at `asan-sample` in the Makefile): both sampling entries of the C ABI on
// dummy records along every refusal they make before anything touches the device.  Every pointer is a dummy address that is never
// dereferenced (the two host arrays are real); a call that passed its checks would go on to the device, so each case must be refused.
// Prints one line per case; exit status 1 if a case was not refused or was refused in other words.
#include "../include/dq_hip.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

namespace {
float ab[1000];
int32_t ts_ok[3] = {999, 500, 0}, ts_flat[3] = {999, 500, 500}, ts_long[1100];
void* const D = (void*)4096;
int failures = 0;

dq_sample_call base() {
  dq_sample_call q;
  std::memset(&q, 0, sizeof q);
  q.struct_bytes = (int32_t)sizeof q;
  q.alpha_bars_host = ab; q.num_timesteps = 1000;
  q.x_T = (const float*)D; q.ms2_cond = (const float*)D; q.ms1_cond = (const float*)D;
  q.auto_normalize = 1; q.timesteps_host = ts_ok; q.num_steps = 3;
  q.out_x = (float*)D; q.out_noise = (float*)D; q.workspace = D; q.workspace_bytes = (int64_t)1 << 40;
  q.B = 4; q.RT = 8; q.seed_dev = (const uint64_t*)D; q.group_size = 1;
  return q;
}

struct Case { const char* word; std::function<void(dq_sample_call&)> set; bool unet, tfm; };

void expect(const char* who, int rc, const char* word) {
  const char* err = dq_last_error();
  const bool ok = rc != 0 && std::strstr(err, word) && std::strncmp(err, who, std::strlen(who)) == 0;
  std::printf("%s %-16s %-44s | %s\n", ok ? "ok  " : "FAIL", who, word, err);
  if (!ok) ++failures;
}
}  // namespace

int main() {
  for (int i = 0; i < 1000; ++i) ab[i] = std::pow(0.999f, (float)(i + 1));
  for (int i = 0; i < 1100; ++i) ts_long[i] = 1099 - i;
  int mults[2] = {1, 2};
  dq_plan* plan = dq_plan_create(4, 2, mults, 8, 1000);
  dq_tfm* tfm = dq_tfm_create(64, 32, 2, 2);
  if (!plan || !tfm) { std::printf("FAIL handles: %s\n", dq_last_error()); return 1; }
  const float* P = (const float*)D;
  const float nan = std::nanf("");
  const std::vector<Case> cases = {
      {"call->struct_bytes is", [](dq_sample_call& q) { q.struct_bytes += 4; }, true, true},
      {"call->struct_bytes is", [](dq_sample_call& q) { q.struct_bytes -= 4; q.alpha_bars_host = nullptr; }, true, true},
      {"null argument", [](dq_sample_call& q) { q.ms2_cond = nullptr; }, true, true},
      {"null argument", [](dq_sample_call& q) { q.timesteps_host = nullptr; }, true, true},
      {"eta must satisfy", [](dq_sample_call& q) { q.eta = 1.5f; }, true, true},
      {"eta must satisfy", [=](dq_sample_call& q) { q.eta = nan; }, true, true},
      {"unknown sampler", [](dq_sample_call& q) { q.sampler = 7; }, true, true},
      {"eta must be 0", [](dq_sample_call& q) { q.sampler = 2; q.eta = 0.5f; }, true, true},
      {"clip_x0 needs the ddim", [](dq_sample_call& q) { q.clip_x0 = 1.f; }, true, true},
      {"clip_x0 needs eta == 0", [](dq_sample_call& q) { q.sampler = 1; q.clip_x0 = 1.f; q.eta = 0.5f; }, true, true},
      {"threshold_quantile needs the ddim", [](dq_sample_call& q) { q.threshold_quantile = 0.9f; }, true, true},
      {"threshold_quantile needs eta == 0", [](dq_sample_call& q) { q.sampler = 1; q.threshold_quantile = 0.9f; q.eta = 0.5f; }, true, true},
      {"strictly decreasing", [](dq_sample_call& q) { q.sampler = 1; q.timesteps_host = ts_flat; }, true, true},
      {"need the seed", [](dq_sample_call& q) { q.x_T = nullptr; q.seed_dev = nullptr; }, true, true},
      {"need the seed", [](dq_sample_call& q) { q.eta = 0.5f; q.seed_dev = nullptr; }, true, true},
      {"Unknown pred_type", [](dq_sample_call& q) { q.pred_type = 3; }, true, true},
      {"Unknown pred_type", [](dq_sample_call& q) { q.pred_type = DQ_PRED_V; }, false, true},
      {"guidance scale must be finite", [](dq_sample_call& q) { q.guided = 1; q.guidance_scale = -1.f; }, true, true},
      {"guidance scale must be finite", [=](dq_sample_call& q) { q.guided = 1; q.guidance_scale = nan; }, true, true},
      {"guidance_rescale must satisfy", [](dq_sample_call& q) { q.guidance_rescale = 1.5; }, true, true},
      {"guidance_rescale must satisfy", [=](dq_sample_call& q) { q.guidance_rescale = nan; }, true, true},
      {"threshold_quantile must satisfy", [](dq_sample_call& q) { q.sampler = 1; q.threshold_quantile = 1.5f; }, true, true},
      {"threshold_max must be >= the floor", [](dq_sample_call& q) { q.sampler = 1; q.threshold_quantile = 0.9f; q.threshold_max = 0.5f; }, true, true},
      {"null argument (stat_scratch)", [](dq_sample_call& q) { q.sampler = 1; q.threshold_quantile = 0.9f; q.threshold_max = 2.f; }, true, true},
      {"scratch too small", [](dq_sample_call& q) { q.sampler = 1; q.threshold_quantile = 0.9f; q.threshold_max = 2.f; q.stat_scratch = D; q.stat_scratch_bytes = 16; }, true, false},
      {"guided sampling is built for the U-Net", [](dq_sample_call& q) { q.guided = 1; q.guidance_scale = 2.f; }, false, true},
      {"guidance_rescale and threshold_quantile are built for the U-Net", [](dq_sample_call& q) { q.guidance_rescale = 0.5; }, false, true},
      {"consistency is built for the U-Net", [](dq_sample_call& q) { q.consistency = DQ_CONSIST_SUM; q.group_size = 2; }, false, true},
      {"need B, RT > 0", [](dq_sample_call& q) { q.B = 0; }, true, false},
      {"need B, S1, S2 > 0", [](dq_sample_call& q) { q.B = 0; }, false, true},
      {"num_steps <= 1024", [](dq_sample_call& q) { q.timesteps_host = ts_long; q.num_steps = 1100; }, true, true},
      {"consistency together with guided", [](dq_sample_call& q) { q.consistency = DQ_CONSIST_BOUND; q.group_size = 2; q.guided = 1; q.guidance_scale = 2.f; }, true, false},
      {"consistency together with guided", [](dq_sample_call& q) { q.consistency = DQ_CONSIST_BOUND; q.group_size = 2; q.guidance_rescale = 0.5; }, true, false},
      {"group_size must be 1..8", [](dq_sample_call& q) { q.consistency = DQ_CONSIST_BOUND; q.group_size = 9; }, true, false},
      {"whole number of groups", [](dq_sample_call& q) { q.consistency = DQ_CONSIST_BOUND; q.group_size = 3; }, true, false},
      {"unknown consistency mode", [](dq_sample_call& q) { q.consistency = 5; q.group_size = 2; }, true, false},
      {"0 < strength <= 1", [=](dq_sample_call& q) { q.consistency = DQ_CONSIST_SUM; q.group_size = 2; q.consistency_strength = nan; }, true, false},
      {"workspace too small", [](dq_sample_call& q) { q.workspace_bytes = 64; }, false, true},
      {"num_timesteps must be >= 1", [](dq_sample_call& q) { q.num_timesteps = 0; }, false, true},
  };
  expect("dq_ddim_sample", dq_ddim_sample(plan, P, P, nullptr), "null argument (call)");
  expect("dq_tfm_sample", dq_tfm_sample(tfm, P, P, P, P, 7, nullptr), "null argument (call)");
  for (const Case& c : cases) {
    dq_sample_call q = base();
    c.set(q);
    if (c.unet) expect("dq_ddim_sample", dq_ddim_sample(plan, P, P, &q), c.word);
    if (c.tfm) { q.RT = 10; expect("dq_tfm_sample", dq_tfm_sample(tfm, P, P, P, P, 7, &q), c.word); }
  }
  dq_sample_call q = base();
  expect("dq_ddim_sample", dq_ddim_sample(nullptr, P, P, &q), "null argument");
  expect("dq_tfm_sample", dq_tfm_sample(nullptr, P, P, P, P, 7, &q), "null argument");
  int32_t layout[128];
  const int n = dq_debug_sample_call_layout(layout, 128);
  if (n != 1 + 2 * 36 || layout[0] != (int32_t)sizeof(dq_sample_call) || dq_debug_sample_call_layout(layout, 8) != -1) { std::printf("FAIL layout %d\n", n); ++failures; }
  dq_plan_destroy(plan);
  dq_tfm_destroy(tfm);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
