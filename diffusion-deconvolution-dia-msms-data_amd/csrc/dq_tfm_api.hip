// The stand-alone entry points of the C ABI (include/dq_hip.h) on the transformer's side: the dense product (dq_gemm*, its scratch size and its
// plan) and the kernels between the GEMMs, one launcher each on tensors the caller chooses -- for the per-kernel tests and benchmarks
// (tests/test_gemm_paths.py, tests/test_tfm_kernels.py).  Thin: argument checks, then the launcher of dq_tfm.h that the network's passes call;
// nothing is allocated.  They know nothing of the network (dq_tfm.hip); dq_ops_api.hip is the U-Net's counterpart.
#include "../../include/dq_hip.h"
#include "dq_common.h"
#include "dq_tfm.h"
#include <algorithm>

using namespace dq;

extern "C" {

int64_t dq_gemm_scratch_floats(int M, int N, int K) { return std::max<int64_t>(gemm_partial_floats(M, N, K, 1), 4); }
// the descriptor of the C ABI -> the launcher's own (field for field)
static int run_desc(const dq_gemm_desc& d, void* stream) {
  DQ_REQUIRE(d.precision == DQ_PRECISION_FP32 || d.precision == DQ_PRECISION_BF16X3, "dq_gemm_ex: precision must be DQ_PRECISION_FP32 or DQ_PRECISION_BF16X3");
  Gemm g;
  g.A = d.A; g.B = d.B; g.C = d.C; g.M = d.M; g.N = d.N; g.K = d.K; g.lda = d.lda; g.ldb = d.ldb; g.ldc = d.ldc;
  g.a_kmajor = d.a_kmajor; g.b_kmajor = d.b_kmajor; g.batch = d.batch; g.inner = d.inner;
  g.sAo = d.sAo; g.sAi = d.sAi; g.sBo = d.sBo; g.sBi = d.sBi; g.sCo = d.sCo; g.sCi = d.sCi;
  g.kbatch = d.kbatch; g.sAk = d.sAk; g.sBk = d.sBk;
  g.bias = d.bias; g.bias_m = d.bias_m; g.alpha = d.alpha; g.accumulate = d.accumulate; g.add = d.add;
  g.splits = d.splits; g.partial = d.scratch; g.partial_floats = d.scratch_floats;
  g.precision = d.precision == DQ_PRECISION_BF16X3 ? GEMM_BF16X3 : GEMM_FP32;
  return launch_gemm(g, (hipStream_t)stream);
}
static dq_gemm_desc plain_desc(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int64_t lda, int64_t ldb,
                               int64_t ldc, int a_kmajor, int b_kmajor, int accumulate, int splits, float* scratch, int64_t scratch_floats,
                               int precision) {
  dq_gemm_desc d = {};
  d.A = A; d.B = B; d.C = C; d.bias = bias; d.M = M; d.N = N; d.K = K; d.lda = lda; d.ldb = ldb; d.ldc = ldc;
  d.a_kmajor = a_kmajor; d.b_kmajor = b_kmajor; d.batch = 1; d.inner = 1; d.kbatch = 1; d.alpha = 1.f;
  d.accumulate = accumulate; d.splits = splits; d.scratch = scratch; d.scratch_floats = scratch_floats; d.precision = precision;
  return d;
}
int dq_gemm(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
            int a_kmajor, int b_kmajor, int accumulate, int splits, float* scratch, int64_t scratch_floats, void* stream) {
  return run_desc(plain_desc(A, B, C, bias, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, accumulate, splits, scratch, scratch_floats,
                             DQ_PRECISION_FP32), stream);
}
int dq_gemm_bf16x3(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                   int a_kmajor, int b_kmajor, int accumulate, int splits, float* scratch, int64_t scratch_floats, void* stream) {
  return run_desc(plain_desc(A, B, C, bias, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, accumulate, splits, scratch, scratch_floats,
                             DQ_PRECISION_BF16X3), stream);
}
int dq_gemm_ex(const dq_gemm_desc* desc, void* stream) {
  DQ_REQUIRE(desc, "dq_gemm_ex: null descriptor");
  return run_desc(*desc, stream);
}
int dq_debug_gemm_plan(int M, int N, int K, int batch, int kbatch, int splits, int32_t* out, int cap, int64_t* scratch_floats) {
  if (!out || cap < DQ_GEMM_PLAN_INTS || M < 1 || N < 1 || K < 1 || batch < 1 || kbatch < 1 || splits < 0) return -1;
  const GemmShape sh = gemm_plan(M, N, K, batch, kbatch, splits);
  int n = 0;
  out[n++] = sh.bm;
  out[n++] = sh.kv;
  for (const GemmPart* p : {&sh.full, &sh.rest}) {
    out[n++] = p->tile_base; out[n++] = p->ntiles; out[n++] = p->splits; out[n++] = p->k_per_split;
  }
  if (scratch_floats) *scratch_floats = sh.scratch;
  return n;
}

int dq_tfm_layernorm_form(int H, int aligned16) { return H > 0 ? layernorm_form(H, H % 4 == 0 && aligned16 != 0) : -1; }

int dq_tfm_rope_add(float* x, const float* sin_t, const float* cos_t, const float* temb, int B, int S, int H, int inverse, void* stream) {
  DQ_REQUIRE(x && sin_t && cos_t, "dq_tfm_rope_add: null argument");
  DQ_REQUIRE(B > 0 && S > 0 && H > 0 && H % 2 == 0, "dq_tfm_rope_add: B, S positive, H positive and even");
  DQ_REQUIRE(((uintptr_t)x & 7) == 0, "dq_tfm_rope_add: x must be 8-byte aligned (channel pairs move as float2)");
  return launch_rope_add(x, sin_t, cos_t, temb, B, S, H, inverse, (hipStream_t)stream);
}
int dq_tfm_cond_embed(const float* x_cond, const float* w, const float* bias, const float* sin_t, const float* cos_t, float* c, int B, int S,
                      int H, void* stream) {
  DQ_REQUIRE(x_cond && w && bias && sin_t && cos_t && c, "dq_tfm_cond_embed: null argument");
  DQ_REQUIRE(B > 0 && S > 0 && H > 0 && H % 2 == 0, "dq_tfm_cond_embed: B, S positive, H positive and even");
  DQ_REQUIRE(((uintptr_t)c & 7) == 0, "dq_tfm_cond_embed: c must be 8-byte aligned (channel pairs move as float2)");
  return launch_cond_embed(x_cond, w, bias, sin_t, cos_t, c, B, S, H, (hipStream_t)stream);
}
int dq_tfm_cond_embed_bwd(const float* dc, const float* x_cond, const float* w, const float* sin_t, const float* cos_t, float* dw, float* db,
                          float* dx_cond, float* scratch, int64_t scratch_floats, int B, int S, int H, int accumulate, void* stream) {
  DQ_REQUIRE(dc && x_cond && w && sin_t && cos_t && dw && db && scratch, "dq_tfm_cond_embed_bwd: null argument");
  DQ_REQUIRE(B > 0 && S > 0 && H > 0 && H % 2 == 0, "dq_tfm_cond_embed_bwd: B, S positive, H positive and even");
  DQ_REQUIRE(((uintptr_t)dc & 7) == 0, "dq_tfm_cond_embed_bwd: dc must be 8-byte aligned (channel pairs move as float2)");
  DQ_REQUIRE(scratch_floats >= (int64_t)2 * H * 64, "dq_tfm_cond_embed_bwd: scratch needs 2 * H * 64 floats");
  return launch_cond_embed_bwd(dc, x_cond, w, sin_t, cos_t, dw, db, dx_cond, scratch, B, S, H, (hipStream_t)stream, accumulate ? 1 : 0);
}
int dq_tfm_time_features(const int64_t* t, const float* freqs, float* e, int B, int H, void* stream) {
  DQ_REQUIRE(t && freqs && e, "dq_tfm_time_features: null argument");
  DQ_REQUIRE(B > 0 && H > 0 && H % 2 == 0, "dq_tfm_time_features: B positive, H positive and even");
  return launch_time_features(t, freqs, e, B, H, (hipStream_t)stream);
}
int dq_tfm_gelu(const float* x, float* y, int64_t n, void* stream) {
  DQ_REQUIRE(x && y && n >= 0, "dq_tfm_gelu: null argument");
  return launch_gelu(x, y, n, (hipStream_t)stream);
}
int dq_tfm_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream) {
  DQ_REQUIRE(x && dy && dx && n >= 0, "dq_tfm_gelu_bwd: null argument");
  return launch_gelu_bwd(x, dy, dx, n, (hipStream_t)stream);
}
int dq_tfm_layernorm_fwd(const float* x, const float* r, const float* g, const float* b, float* y, float* out, float* stats, int rows, int H,
                         void* stream) {
  DQ_REQUIRE(x && g && b && y && out, "dq_tfm_layernorm_fwd: null argument");
  DQ_REQUIRE(rows > 0 && H > 0, "dq_tfm_layernorm_fwd: rows and H must be positive");
  return launch_layernorm_fwd(x, r, g, b, y, out, stats, rows, H, (hipStream_t)stream);
}
int dq_tfm_layernorm_bwd(const float* y, const float* stats, const float* g, const float* dout, float* dy, float* dg, float* db, float* scratch,
                         int64_t scratch_floats, int rows, int H, int accumulate, void* stream) {
  DQ_REQUIRE(y && stats && g && dout && dy && dg && db && scratch, "dq_tfm_layernorm_bwd: null argument");
  DQ_REQUIRE(rows > 0 && H > 0, "dq_tfm_layernorm_bwd: rows and H must be positive");
  DQ_REQUIRE(scratch_floats >= (int64_t)2 * H * LN_BWD_BLOCKS, "dq_tfm_layernorm_bwd: scratch needs 2 * H * 256 floats");
  return launch_layernorm_bwd(y, stats, g, dout, dy, dg, db, scratch, rows, H, (hipStream_t)stream, accumulate ? 1 : 0);
}
int dq_tfm_softmax_rows(float* p, int64_t rows, int n, int ld, float scale, void* stream) {
  DQ_REQUIRE(p, "dq_tfm_softmax_rows: null argument");
  DQ_REQUIRE(rows > 0 && n > 0 && ld >= n, "dq_tfm_softmax_rows: rows, n positive, ld >= n");
  return launch_softmax_rows(p, rows, n, ld, scale, (hipStream_t)stream);
}
int dq_tfm_softmax_rows_bwd(const float* p, float* dp, int64_t rows, int n, int ld, float scale, void* stream) {
  DQ_REQUIRE(p && dp, "dq_tfm_softmax_rows_bwd: null argument");
  DQ_REQUIRE(rows > 0 && n > 0 && ld >= n, "dq_tfm_softmax_rows_bwd: rows, n positive, ld >= n");
  return launch_softmax_rows_bwd(p, dp, rows, n, ld, scale, (hipStream_t)stream);
}
int dq_tfm_colsum(const float* x, int M, int N, int64_t ld, float* out, float* scratch, int64_t scratch_floats, int accumulate, void* stream) {
  DQ_REQUIRE(x && out && scratch, "dq_tfm_colsum: null argument");
  DQ_REQUIRE(M > 0 && N > 0 && ld >= N, "dq_tfm_colsum: M, N positive, ld >= N");
  DQ_REQUIRE(scratch_floats >= (int64_t)COLSUM_BLOCKS * N, "dq_tfm_colsum: scratch needs 64 * N floats");
  return launch_colsum(x, M, N, ld, out, scratch, (hipStream_t)stream, accumulate ? 1 : 0);
}
int dq_tfm_seqsum(const float* x, int B, int S, int N, float* out, void* stream) {
  DQ_REQUIRE(x && out, "dq_tfm_seqsum: null argument");
  DQ_REQUIRE(B > 0 && S > 0 && N > 0, "dq_tfm_seqsum: B, S, N must be positive");
  return launch_seqsum(x, B, S, N, out, (hipStream_t)stream);
}


}  // extern "C"
