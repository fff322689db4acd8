// Host dispatch of the LinearAttention backward: which kernel form takes a call (la_bwd_form: k_la_long.hip, k_la_rows_bwd.hip or the
// register-resident kernels), the launch geometry of the register-resident kernels (k_la_bwd.h, k_la_bwd1.h: one resident round of
// workgroups, a partial slot each) and the slot reduction behind them (k_la_reduce.hip).  This file instantiates k_linattn_bwd<C, N> for every
// (C, N) but <12,64> and <16,64> (k_la_bwd_big.hip): LINATTN_BWD_BUILT is the list.
#include "k_la_bwd.h"
#include "k_la_bwd1.h"
#include "dq_launch.h"
#include <algorithm>
#include <cstdlib>

namespace dq {

// The register-resident kernels built in this translation unit: k_linattn_bwd<C, N>, and k_linattn_bwd1<C> for rows of one position.
using LinAttnBwdFn = decltype(&k_linattn_bwd<4, 2>);
static const Inst<LinAttnBwdFn, 2> LINATTN_BWD_BUILT[] = {
    DQ_INST(k_linattn_bwd, 4, 2), DQ_INST(k_linattn_bwd, 4, 4), DQ_INST(k_linattn_bwd, 4, 8), DQ_INST(k_linattn_bwd, 4, 16), DQ_INST(k_linattn_bwd, 4, 32),
    DQ_INST(k_linattn_bwd, 4, 64),
    DQ_INST(k_linattn_bwd, 8, 2), DQ_INST(k_linattn_bwd, 8, 4), DQ_INST(k_linattn_bwd, 8, 8), DQ_INST(k_linattn_bwd, 8, 16), DQ_INST(k_linattn_bwd, 8, 32),
    DQ_INST(k_linattn_bwd, 8, 64),
    DQ_INST(k_linattn_bwd, 12, 2), DQ_INST(k_linattn_bwd, 12, 4), DQ_INST(k_linattn_bwd, 12, 8), DQ_INST(k_linattn_bwd, 12, 16), DQ_INST(k_linattn_bwd, 12, 32),
    DQ_INST(k_linattn_bwd, 16, 2), DQ_INST(k_linattn_bwd, 16, 4), DQ_INST(k_linattn_bwd, 16, 8), DQ_INST(k_linattn_bwd, 16, 16), DQ_INST(k_linattn_bwd, 16, 32)};
static const Inst<LinAttnBwdFn, 1> LINATTN_BWD1_BUILT[] = {DQ_INST(k_linattn_bwd1, 4), DQ_INST(k_linattn_bwd1, 8), DQ_INST(k_linattn_bwd1, 12), DQ_INST(k_linattn_bwd1, 16)};

static int linattn_bwd_reg(const LinAttnBwdK& k, int C, int n, const LinAttnBwd& g, hipStream_t s) {
  // one resident round of blocks of four waves (= the four heads): 1-3 per CU, as the kernel's registers / LDS allow; a partial slot per
  // block.  Rows of one position: a wave per 32 rows, a slot per wave.
  const auto* inst1 = find_inst(LINATTN_BWD1_BUILT, {C});
  if (!inst1) { set_error("linattn_bwd: unsupported channel count " + std::to_string(C)); return 2; }
  const bool big = C >= 12 && n == 64;  // (k_la_bwd_big.hip's two kernels: one wave per SIMD, 256 resident blocks)
  const auto* inst = find_inst(LINATTN_BWD_BUILT, {C, n});
  if (n != 1 && !big && !inst) { set_error("linattn_bwd: m/z length " + std::to_string(n) + " is not built (powers of two up to 64)"); return 2; }
  const int slots_max = (int)((g.part_floats - 4 * C * C) / la_slot(C));
  LinAttnBwdK kk = k;
  int slots = 0;
  if (n == 1) {
    const int units = cdiv(k.rows, 32);
    kk.units_per_wave = std::max(1, cdiv(units, std::min(1024, slots_max)));
    slots = cdiv(units, kk.units_per_wave);
    hipLaunchKernelGGL(inst1->fn, dim3(cdiv(slots, 4)), dim3(256), 0, s, kk);
  } else {
    const int units = cdiv(k.rows, n >= 32 ? 1 : 32 / n);
    const int resident = big ? 256 : resident_blocks((const void*)inst->fn, 256, 0);
    if (resident < 0) return 1;
    kk.units_per_wave = std::max(1, cdiv(units, std::min(resident, slots_max)));
    slots = cdiv(units, kk.units_per_wave);
    if (big) launch_linattn_bwd_big(kk, C, 4 * slots, s);
    else hipLaunchKernelGGL(inst->fn, dim3(slots), dim3(256), 0, s, kk);
  }
  DQ_LAUNCH_CHECK();
  /* (4 C C floats behind the slots hold the summed dW2 between the reduce and k_linattn_dwvo) */
  if (g.defer_reduce) {
    *g.waves_out = slots;
    return 0;
  }
  const LaReduceItem it = la_reduce_item(kk.part, slots, C, g.dw_qkv, g.dw_out, g.dg_out, g.db_out, g.dg_pre, k.w_qkv, k.w_out);
  return launch_linattn_dw_reduce_multi(&it, 1, s);
}


// Which kernel runs the backward: k_la_long.hip, k_la_rows_bwd.hip or the register-resident one, each only when its launcher takes every argument
LaBwdForm la_bwd_form(const LinAttnBwd& a) {
  const int C = a.f.C, rows = a.f.rows, n = a.f.n;
  if (!la_short_row(n)) return LA_BWD_LONG;
  // rows of 2 / 4 positions at 8 / 12 / 16 channels: one m/z row per lane column (k_la_rows_bwd.hip), when the layer's prepared weights are at
  // hand; otherwise the register-resident kernel, which reads them with scalar loads
  if (a.f.prep && la_rows_bwd_usable(C, n) && rows >= la_rows_bwd_min_rows() &&
      (((uintptr_t)a.f.prep | (uintptr_t)a.f.x | (uintptr_t)a.ypre | (uintptr_t)a.dy | (uintptr_t)a.dx) & 15) == 0 &&
      (int64_t)rows * C * n * 4 < (1ll << 32))
    return LA_BWD_ROWS;
  return LA_BWD_REG;
}

// a.f.y is unused; needs: a.ypre (saved pre-norm output), the (rows, C, n) scratch dxh (and dyp for rows longer than 64) and
// the partial-slot scratch
int launch_linattn_bwd(const LinAttnBwd& a, hipStream_t s) {
  DQ_REQUIRE(a.f.x && a.dy && a.dx && a.ypre && a.dyp && a.dxh && a.dw_qkv && a.dw_out && a.db_out && a.dg_pre && a.dg_out,
             "linattn_bwd: missing operand");
  if (a.f.rows == 0) return 0;
  const int C = a.f.C, rows = a.f.rows, n = a.f.n;
  if (a.waves_out) *a.waves_out = 0;
  // (a slot per block; the sweep kernel of longer rows: 512 C floats per wave)
  DQ_REQUIRE(a.part && a.part_floats >= (la_short_row(n) ? la_part_reserve(C) : (int64_t)LA_MAX_WAVES * 512 * C),
             "linattn_bwd: partial-sum scratch missing or too small");
  static_assert((int64_t)LA_MAX_WAVES * 512 * 4 >= 2048 * (int64_t)la_slot(4) + 64, "slot scratch: a resident round of slots must fit");
  const LaBwdForm form = la_bwd_form(a);
  if (form == LA_BWD_LONG) {
    // rows of 128 / 256 positions: the sweep kernel between two pointwise norm-backward launches
    // (these launches accumulate into dx: a caller that asked for a plain store gets a cleared dx first)
    DQ_REQUIRE(a.part_floats >= (int64_t)LA_MAX_WAVES * 512 * C, "linattn_bwd: partial-sum scratch too small for the sweep kernel");
    if (a.dx_store)
      if (int rz = launch_zero(a.dx, (int64_t)rows * C * n, s)) return rz;
    BlockBwd b2;  // (1) post-norm backward: dyp = d loss / d ypre, d g_out, d b_out
    b2.u = a.ypre; b2.dy = a.dy; b2.du = a.dyp; b2.C = C; b2.rows = rows; b2.n = n; b2.rows_per_sample = rows;
    b2.g = a.f.g_out; b2.dg = a.dg_out; b2.dbias = a.db_out;
    b2.part = a.part; b2.part_floats = a.part_floats;  // per-block partial sums: the slot scratch is free until the sweep kernel runs
    if (int rc = launch_block_bwd(b2, s)) return rc;
    int waves = 0;
    if (int rc = launch_linattn_bwd_long(a.f.x, a.dyp, a.dxh, a.f.w_qkv, a.f.w_out, a.f.g_pre, a.part, C, rows, n, &waves, s)) return rc;
    if (int rc = launch_linattn_dw_reduce(a.part, waves, C, a.dw_qkv, a.dw_out, s)) return rc;
    // (3) residual + pre-norm backward, accumulated into dx
    if (int r2 = launch_axpy(a.dx, a.dy, (int64_t)rows * C * n, s)) return r2;
    BlockBwd b1;
    b1.u = a.f.x; b1.dy = a.dxh; b1.du = a.dx; b1.C = C; b1.rows = rows; b1.n = n; b1.rows_per_sample = rows;
    b1.g = a.f.g_pre; b1.dg = a.dg_pre; b1.accumulate = 1;
    b1.part = a.part; b1.part_floats = a.part_floats;  // (free again: the slot reduce above has consumed it, in stream order)
    return launch_block_bwd(b1, s);
  }
  if (form == LA_BWD_ROWS) {
    const int slots_max = (int)std::min<int64_t>((a.part_floats - 4 * C * C) / la_slot(C), C <= 8 ? 2048 : 1024);
    int slots = 0;
    if (int rc = launch_la_rows_bwd(a, slots_max, &slots, s)) return rc;
    if (a.defer_reduce) {
      *a.waves_out = slots;
      return 0;
    }
    const LaReduceItem it = la_reduce_item(a.part, slots, C, a.dw_qkv, a.dw_out, a.dg_out, a.db_out, a.dg_pre, a.f.w_qkv, a.f.w_out);
    return launch_linattn_dw_reduce_multi(&it, 1, s);
  }
  LinAttnBwdK k;
  k.x = a.f.x; k.ypre = a.ypre; k.dy = a.dy; k.dx = a.dx; k.w_qkv = a.f.w_qkv; k.w_out = a.f.w_out;
  k.g_pre = a.f.g_pre; k.g_out = a.f.g_out; k.part = a.part; k.rows = rows; k.units_per_wave = 1;
  k.prep = a.f.prep; k.dx_store = a.dx_store;
  return linattn_bwd_reg(k, C, n, a, s);
}

}  // namespace dq
