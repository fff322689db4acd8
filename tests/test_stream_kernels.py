"""The streaming kernels of csrc/k_stream.hip, the unguided DDIM update of csrc/k_update.hip and the optimiser step of csrc/k_adamw.hip at
their loop edges, each against a float64 evaluation of the same fp32 inputs.

Entry points (dquartic._native): dq_q_sample (k_q_sample), dq_ddim_step / dq_ddim_step_x0 (k_step_update<Ddim, false|true, false, V>),
dq_ddim_sample's epilogue (k_sample_finish), dq_mse_loss_fwd_bwd / dq_mse_loss_weighted_fwd_bwd (k_mse_fwd_bwd + k_sum_partials),
dq_ms1_loss_fwd_bwd (k_ms1_rows / _sample / _apply), dq_adamw_clip_step (k_sumsq + k_adamw_clip<false>), dq_adamw_clip_step_dev
(k_adamw_hyper + k_sumsq + k_adamw_clip<false>).

Sizes come from the launch code: T = 256 threads, V elements per thread and trip, G the grid cap (constants below).  Every entry point
runs at the smallest legal size, T*V -+ V and T*V, G*T*V -+ V, and two sweeps of the capped grid plus a ragged remainder; k_sumsq also at
n = 4 * (5 * G * T + 77) + r, r in 1..3 (its paired loop twice, then the single loop, then a scalar tail), with grads aligned and one
float off 16 bytes (its designed scalar branch).  q_sample, the DDIM update and the MSE send an element count (q_sample, weighted MSE: a
per-sample count) that is no multiple of 4 to forms with V = 1 (k_q_sample<1, false>, k_step_update<..., 1>, k_mse_fwd_bwd<MseRead, 1>): those run at the
V = 1 edges that are such sizes, and at 3 x 37 x 2, the shape tests/test_level_plan.py met them at.  The DDIM update takes V = 1 for
tensors that are not 16-byte aligned as well (n = 4 and a block + 4, every tensor one float off).  k_adamw_clip moves 16 bytes per lane
when p, g, m, v are all 16-byte aligned and has a scalar loop for the tail and for every other alignment: both plain entries run with p, m
and v in turn one float off.  Outputs are views between canaries, plain-store outputs start as NaN, scratch buffers
have exactly the documented size (NaN, then a canary compared through an int view).

References: oracle.dq_oracle (q_sample, ddim_update, ddim_update_x0, ms1_term, adamw_clip_step) and the plain MSE formula, in float64
on the promoted fp32 inputs (alpha_bars, loss-weight table included).

Tolerances (none taken from a kernel's output; tests/test_oracle_golden.py holds the fp32 CPU restatement of every case to half of each,
three short paths to 0.55 - 0.65 as listed there):
  * element-wise outputs: |out - ref| <= K * 2^-24 * S per element, S = the float64 expression with every term replaced by its absolute
    value, K = fp32 roundings on the longest path through the kernel's expression + 1 for the comparison (K_* below, counted beside each);
    where clip_grad_norm_ is active the AdamW outputs add (R + 4) * 2^-24 * |d out / d log coef| for the clip coefficient, which inherits
    the norm's reduction error R (below) and 4 roundings of its own (sqrt, + 1e-6, /, * grad_scale);
  * reductions (loss, gnorm): relative R * 2^-24 on the sum of absolute terms, R = serial adds per thread + log2(256) + ceil(grid / 64)
    + log2(64) + 2 (block tree, serial partials per lane, wave tree, scale and sqrt);
  * MS1 term: the gradient chains divisions by the normalisers, so the bound is 4 x the largest distance of the fp32 CPU oracle from the
    float64 oracle over all cases (max-abs over max |grad|): the factor covers the other summation order and the fused multiply-adds.
    The loss gets that plus the reduction bound of its MSE part.  Measured on the CPU (fp32 oracle vs float64 oracle):
        largest gradient distance  2.9e-7 (rounded up to 3.0e-7)  ->  MS1_GRAD_TOL 1.2e-6
        largest loss distance      2.1e-7                         ->  MS1_LOSS_TOL 8.4e-7 (+ (1 - w) x the reduction bound of the MSE part)
  * caps (what the older tests demand of the same quantity; the tighter of cap and derived bound holds): q_sample 2e-7 and ddim 1e-6 of the
    output maximum, loss 1e-5, MS1 gradient 2e-5, gnorm 1e-4, parameters 2e-6 absolute at lr 1e-3 (see adamw_ratios).
  Measured fp32 CPU restatements, worst element of all cases, in units of 2^-24 * S: q_sample 2.6, ddim (eps) 4.1, ddim (x0) 3.6 / eps_out
  3.6, MSE gradient 2.5 / 2.7 (weighted), AdamW m 2.2, v 2.6, p 3.6 (with the fp32 scalars in the oracle)."""
import math

import numpy as np
import pytest
import torch

from conftest import sub

pytestmark = pytest.mark.gpu

T_ = 256                      # every launch in k_stream.hip, k_update.hip and k_adamw.hip: dim3(256)
GRID_STREAM = 2048            # launch_q_sample / launch_update / launch_sample_finish: std::min(cdiv(n4, 256), 2048)
MSE_MAX_BLOCKS = 1024         # dq_kernels.h: constexpr int MSE_MAX_BLOCKS (launch_mse_fwd_bwd's grid cap, the scratch size)
GRID_ADAMW = MSE_MAX_BLOCKS - 8  # launch_adamw: std::min(cdiv(n, 256), MSE_MAX_BLOCKS - 8)
GRID_MS1_APPLY = 4096         # launch_ms1_loss: k_ms1_apply's grid, std::min(cdiv(rows * MZ, 256), 4096)
SCRATCH = 1024                # include/dq_hip.h: "scratch: >= 1024 device floats" (MSE, AdamW)
U = 2.0 ** -24
HEAD, TAIL, CANARY = 64, 4096, 7251.0
NUM_T = 1000
B1, B2, EPS = 0.9, 0.999, 1e-8

# fp32 roundings on the longest path (+ 1 for the comparison in fp32)
K_Q = 5       # sb = sqrt(1 - ab): 2 | sb * nz: 1 | + : 1                                  (the sa path: sqrt, 2x-1, *, + is as long)
K_DDIM = 10   # sb: 2 | sb * eps: 1 | x - .: 1 | sa: 1, / sa: 1 | sap: 1, sap * x0: 1 | + : 1
K_DDIM_X0 = 11  # sa: 1 | sa * x0: 1 | x - .: 1 | sb: 2, / sb: 1 | sbp: 2, sbp * eps: 1 | + : 1
K_DDIM_EPS = 7  # the first six of the line above
K_MSE = 4     # d = e - z: 1 | gscale = 2 / n: 1 | d * gs: 1
K_WMSE = 7    # z * tm: 1, + ta: 1 | e - z: 1 | 2 / n: 1, * w: 1 | d * gs: 1
K_M = 5       # gi = g * coef: 1 | gi - m: 1 | * (1 - b1): 1 | m + .: 1
K_V = 6       # gi: 1 (twice in gi^2: 2) | (1 - b2) * gi: 1 | b2 * v: 1, fma: 1  -> 5 on the longer path
K_P = 14      # m: 4 | denom: v 5 / 2 (sqrt halves it), sqrt 1, / 1, + 1 = 5.5 | m / denom: 1 | * step_size: 1 | p * decay - .: 1  -> 12.5
CAP_Q, CAP_DDIM, CAP_LOSS, CAP_MS1_GRAD, CAP_GNORM, CAP_P = 2e-7, 1e-6, 1e-5, 2e-5, 1e-4, 2e-6
CAP_P_SCALE = 5.0  # max |p| + the largest update of tests/test_hip_backward.py::test_adamw_clip_matches_torch, the test CAP_P comes from

# the fp32 CPU oracle's distance from the float64 oracle over MS1_CASES + MS1_TIES (tests/test_oracle_golden.py re-measures and holds
# every case to half of the bound, i.e. to twice these figures)
MS1_GRAD_DIST, MS1_LOSS_DIST = 3.0e-7, 2.1e-7
MS1_GRAD_TOL = min(4 * MS1_GRAD_DIST, CAP_MS1_GRAD)
MS1_LOSS_TOL = 4 * MS1_LOSS_DIST


def cdiv(a, b):
    return -(-a // b)


def edge_sizes(V, G, smallest):
    """smallest | a block -+ one vector and exactly | the capped grid's sweep -+ one vector | two sweeps + a ragged remainder"""
    blk, sweep = T_ * V, G * T_ * V
    return [smallest, blk - V, blk, blk + V, sweep - V, sweep + V, 2 * sweep + 333 * V]


def reduction_units(serial, grid):
    return serial + 8 + cdiv(grid, 64) + 6 + 2


def ratio(out, ref, S, K, cap=None, extra=None):
    """max over the elements of |out - ref| / bound (<= 1 passes; NaN fails), bound = K * 2^-24 * S (+ extra), at most cap * max |ref|"""
    out, ref = out.detach().cpu().double().reshape(-1), ref.reshape(-1)
    bound = K * U * S.reshape(-1)
    if extra is not None:
        bound = bound + extra.reshape(-1)
    if cap is not None:
        bound = bound.clamp(max=cap * float(ref.abs().max()))
    err = (out - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max())


def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * k for s, k in zip(seed, (1, 1000003, 10007, 101, 7))) % (2 ** 62))


_SCHED = {}


def alpha_bars(kind="cosine"):
    from oracle import dq_oracle as O

    if kind not in _SCHED:
        _SCHED[kind] = O.make_schedule(NUM_T, kind)["alpha_bars"]
    return _SCHED[kind]


def snr_table():
    """DDIMDiffusionModel(pred_type='x0').loss_weight on the cosine schedule: 2.4e-9 at t = 999 to 2.4e4 at t = 0"""
    ab = alpha_bars()
    return ab / (1 - ab)


def timesteps(B, pattern):
    return torch.tensor([pattern[i % len(pattern)] for i in range(B)], dtype=torch.int64)


# ---- cases (CPU): fp32 inputs, the float64 reference, S, and the fp32 restatement ------------------------------------------------------

# (B, per_sample): per_sample = 4, blocks serving many samples, a sample spanning sweeps
Q_CASES = [(1, 4), (7, 4), (5, 204), (4, 256), (1, 1028), (257, 4), (1, 2097148), (524287, 4), (3, 699052), (5, 839128)]
# per_sample % 4 != 0 (k_q_sample<1, false>, one element per thread and trip): the smallest, MZ = 2 at RT = 37, B * per_sample a multiple of 4 all
# the same, a block + 1, beyond one sweep of the capped grid
Q_CASES += [(1, 1), (3, 74), (2, 6), (1, 257), (3, 174767)]


def q_case(B, per, normalize, kind, fp32=False):
    from oracle import dq_oracle as O

    g = gen(B, per, normalize, kind == "linear")
    ab = alpha_bars(kind)
    x0, nz = torch.rand(B, 1, per, generator=g), torch.randn(B, 1, per, generator=g)
    t = timesteps(B, [NUM_T - 1, 0, 500, 0, NUM_T - 1, 17, 998, 1]) if B > 1 else torch.tensor([NUM_T - 1 if kind == "cosine" else 0])
    c = {"ab": ab, "x0": x0, "nz": nz, "t": t}
    x64 = O.normalize(x0.double()) if normalize else x0.double()
    c["ref"] = O.q_sample(ab.double(), x64, t, nz.double())
    sa, sb = ab.double()[t].sqrt()[:, None, None], (1 - ab.double()[t]).sqrt()[:, None, None]
    c["S"] = sa * ((2 * x0.double()).abs() + 1 if normalize else x0.double().abs()) + sb * nz.double().abs()
    if fp32:
        c["fp32"] = O.q_sample(ab, O.normalize(x0) if normalize else x0, t, nz)
    return c


# n % 4 != 0 (k_step_update<..., 1>, V = 1): the same edges where they are no multiple of 4, and 3 x 37 x 2
ODD = lambda sizes: [n for n in sizes if n % 4]
DDIM_SIZES = edge_sizes(4, GRID_STREAM, 4) + ODD(edge_sizes(1, GRID_STREAM, 1)) + [222]
DDIM_T = [999, 998, 500, 1, 0]  # 999: / sqrt(ab) = 4.9e-5; 0: the coef[2] < 0 branch


def coef_row(t):
    """the row dq_ddim_sample / p_sample build, fp32 throughout"""
    ab = alpha_bars()
    a = ab[t]
    return torch.stack([a.sqrt(), (1 - a).sqrt(), ab[t - 1].sqrt() if t > 0 else torch.tensor(-1.0),
                        (1 - ab[t - 1]).sqrt() if t > 0 else torch.tensor(0.0)]).float()


def ddim_case(n, t, fp32=False):
    from oracle import dq_oracle as O

    g = gen(n, t, 3)
    ab = alpha_bars()
    x, e, x0 = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.rand(n, generator=g) * 2 - 1
    c = {"x": x, "eps": e, "x0": x0, "coef": coef_row(t)}
    a64 = ab.double()
    sa, sb = a64[t].sqrt(), (1 - a64[t]).sqrt()
    sap, sbp = (a64[t - 1].sqrt(), (1 - a64[t - 1]).sqrt()) if t > 0 else (None, None)
    X, E, X0 = x.double(), e.double(), x0.double()
    c["ref"] = O.ddim_update(a64, X, E, t)
    s_x0 = (X.abs() + sb * E.abs()) / sa
    c["S"] = sap * s_x0 + sbp * E.abs() if t > 0 else s_x0
    c["ref_xp"], c["ref_eps"] = O.ddim_update_x0(a64, X, X0, t)
    c["S_eps"] = (X.abs() + sa * X0.abs()) / sb
    c["S_xp"] = sap * X0.abs() + sbp * c["S_eps"] if t > 0 else X0.abs()
    if fp32:
        c["fp32"] = O.ddim_update(ab, x, e, t)
        c["fp32_xp"], c["fp32_eps"] = O.ddim_update_x0(ab, x, x0, t)
    return c


MSE_SIZES = edge_sizes(4, MSE_MAX_BLOCKS, 4) + ODD(edge_sizes(1, MSE_MAX_BLOCKS, 1)) + [222]  # (n % 4 != 0: k_mse_fwd_bwd<MseRead, 1>)
# (B, per_sample): from per_sample = 4 (a block serves 256 samples) to one sample spanning several sweeps of the 1024-block grid
WMSE_CASES = [(1, 4), (255, 4), (4, 256), (1, 1028), (3, 349524), (262145, 4), (1, 2098484), (7, 299784)]
WMSE_CASES += [(1, 1), (3, 74), (2, 6), (257, 1), (7, 74899)]  # per_sample % 4 != 0 (V = 1), B * per_sample = 12 included
WMSE_MAPS = [(2.0, -1.0), (1.0, 0.0)]


def mse_units(n, V=4):
    """V = 4 elements per thread and trip; 1 where n (weighted form: per_sample) is no multiple of 4"""
    grid = min(cdiv(n // V, T_), MSE_MAX_BLOCKS)
    return reduction_units(V * cdiv(n // V, grid * T_), grid)


def mse_case(B, per, tm=None, ta=None, fp32=False):
    """tm None: the plain MSE (B = 1); else the weighted form with the SNR table and t mixing both of its ends"""
    weighted = tm is not None
    g = gen(B, per, 0 if not weighted else 1 + int(tm))
    n = B * per
    e = torch.randn(B, per, generator=g)
    z = torch.rand(B, per, generator=g) if weighted and tm == 2.0 else torch.randn(B, per, generator=g)
    c = {"e": e, "z": z, "n": n}
    if weighted:
        c["lw"] = snr_table()
        c["t"] = timesteps(B, [0, NUM_T - 1, 0, 500, NUM_T - 1, 3, 996]) if B > 1 else torch.tensor([0 if tm == 2.0 else NUM_T - 1])
        w = c["lw"].double()[c["t"]][:, None]
    else:
        tm, ta, w = 1.0, 0.0, torch.ones(1, 1, dtype=torch.float64)
    E, Z = e.double(), z.double()
    d = E - (Z * tm + ta)
    c["loss"] = float((w * d * d).sum() / n)
    c["grad"] = 2 * d * w / n
    absd = E.abs() + (Z * tm).abs() + abs(ta)
    c["S_grad"] = 2 * absd * w / n
    c["loss_bound"] = min(mse_units(n, 1 if per % 4 else 4) * U * float((w * absd * absd).sum() / n), CAP_LOSS * abs(c["loss"]))
    if fp32:
        w32 = c["lw"][c["t"]][:, None] if weighted else 1.0
        d32 = e - (z * tm + ta)
        c["fp32_loss"] = float((w32 * d32 * d32).sum() / n)
        c["fp32_grad"] = d32 * ((2.0 / n) * w32)
    return c


# (B, RT, MZ, form, weights, w, grad): every RT of {1, 3, 255, 256, 257, 400, 2000} and every MZ of {4, 8, 64, 100, 256} at least twice,
# B * RT % 4 != 0 in eight of them, (3, 2000, 256) beyond 4096 * 256 elements; grad False: grad_inout = NULL
MS1_CASES = [(1, 1, 4, "eps", False, 0.25, True), (3, 1, 64, "x0", True, 0.25, True), (2, 3, 8, "eps", True, 0.25, True),
             (5, 3, 100, "x0", False, 1.0, True), (1, 255, 100, "eps", False, 0.25, True), (2, 255, 4, "x0", True, 0.25, True),
             (3, 256, 256, "eps", True, 1.0, True), (1, 256, 8, "x0", False, 0.25, True), (3, 257, 64, "eps", False, 0.25, True),
             (2, 257, 4, "x0", True, 1.0, True), (3, 400, 64, "x0", True, 0.25, True), (2, 400, 100, "eps", False, 1.0, False),
             (3, 2000, 256, "eps", True, 0.25, True), (1, 2000, 8, "x0", False, 0.25, True)]
MS1_TIES = [(2, 6, 100, "eps", False, 0.25, True), (2, 6, 100, "x0", True, 1.0, True)]
TIE_ROWS, TIE_MZ, TIE_MS1 = (1, 4), (7, 70), (2, 5)  # equal maxima: two RT rows of a sample, two m/z of a row, two RT of the chromatogram


def ms1_loss(pred, x_t, target, ms1n, lw_t, w):
    """the whole objective of the stand-alone calls, dtype-generic: mean_b lw_b ((1 - w) MSE_b + w additional_b)"""
    from oracle import dq_oracle as O

    per = ((pred - target) ** 2).flatten(1).mean(dim=1)
    per = (1 - w) * per + w * O.ms1_term(x_t - pred if x_t is not None else pred, ms1n)
    return (per * lw_t).mean() if lw_t is not None else per.mean()


def ms1_case(B, RT, MZ, form, weights, w, grad=True, ties=False, fp32=False):
    g = gen(B, RT, MZ, form == "x0", ties)
    shape = (B, RT, MZ)
    if ties:  # a 1/64 grid: fp32 and float64 see the same differences, sums and maxima exactly
        q = lambda *s: torch.randint(-32, 33, s, generator=g).float() / 64
        pred, x_t, target, ms1 = q(*shape), (q(*shape) if form == "eps" else None), q(*shape), torch.randint(0, 60, (B, RT), generator=g).float() / 64
        d = pred if form == "x0" else x_t  # the tensor to plant in: D = x_t - pred or pred
        if form == "eps":
            pred[:, TIE_ROWS[0]] = 0.0
        d[:, TIE_ROWS[0]] = q(B, MZ) + 2.0
        d[:, TIE_ROWS[0], TIE_MZ[0]] = d[:, TIE_ROWS[0], TIE_MZ[1]] = 5.0
        if form == "eps":
            pred[:, TIE_ROWS[1]] = pred[:, TIE_ROWS[0]]
        d[:, TIE_ROWS[1]] = d[:, TIE_ROWS[0]]
        ms1[:, TIE_MS1[0]] = ms1[:, TIE_MS1[1]] = 62.0 / 64
        for r in TIE_ROWS:  # no MSE gradient in the two rows: what lands there is the MS1 term's alone
            target[:, r] = pred[:, r]
        cm, ca = 1.0, 0.0
    else:  # D with a positive mean, so that the normalisers stay away from 0
        if form == "eps":
            pred, x_t = torch.randn(shape, generator=g) * 0.3, torch.randn(shape, generator=g) + 0.5
        else:
            pred, x_t = torch.randn(shape, generator=g) * 0.5 + 0.4, None
        target, ms1 = torch.randn(shape, generator=g), torch.rand(B, RT, generator=g)
        cm, ca = 2.0, -1.0
    c = {"pred": pred, "x_t": x_t, "target": target, "ms1": ms1, "cm": cm, "ca": ca, "w": w, "grad_wanted": grad}
    if weights:
        c["lw"], c["t"] = snr_table(), timesteps(B, [300, 50, 620])
    f64 = lambda v: None if v is None else v.double()
    p64 = pred.double().requires_grad_()
    lw_t = c["lw"].double()[c["t"]] if weights else None
    loss = ms1_loss(p64, f64(x_t), f64(target), ms1.double() * cm + ca, lw_t, w)
    loss.backward()
    c["loss"], c["grad"] = float(loss), p64.grad
    D = (f64(x_t) - pred.double()) if x_t is not None else pred.double()
    s_sum, s_max, m1 = D.sum(-1), D.max(-1).values, ms1.double() * cm + ca
    c["normalisers"] = torch.stack([s_sum.max(-1).values, s_sum.max(-1).values / MZ, s_max.max(-1).values, m1.max(-1).values])
    n = B * RT * MZ
    d = pred.double() - target.double()
    wv = lw_t[:, None, None] if weights else 1.0
    absd = pred.double().abs() + target.double().abs()
    mse_abs = float((wv * absd * absd).sum() / n)
    c["loss_bound"] = min(MS1_LOSS_TOL * abs(c["loss"]) + (1 - w) * mse_units(n) * U * mse_abs, CAP_LOSS * abs(c["loss"]))
    if fp32:
        p32 = pred.clone().requires_grad_()
        l32 = ms1_loss(p32, x_t, target, ms1 * cm + ca, c["lw"][c["t"]] if weights else None, w)
        l32.backward()
        c["fp32_loss"], c["fp32_grad"] = float(l32), p32.grad
    return c


ADAMW_BASE = dict(mode="active", grad_scale=1.0, max_norm=10.0, lr=1e-3, step=10, wd=0.01, gnorm=True, zero=False)
ADAMW_VARIANTS = [dict(), dict(mode="inactive"), dict(mode="disabled", max_norm=0.0), dict(mode="disabled", max_norm=-1.0),
                  dict(grad_scale=0.125), dict(grad_scale=0.125, mode="inactive"), dict(gnorm=False), dict(wd=0.0), dict(zero=True, step=1)]
# k_adamw_clip and k_sumsq: V = 4 over n // 4 vectors, then a scalar loop (V = 1) over the n % 4 elements left.  The V = 4 edges walk the
# vector loop, the V = 1 edges leave tails of 1 - 3 elements behind it
ADAMW_SIZES = sorted(set(edge_sizes(1, GRID_ADAMW, 1)) | set(edge_sizes(4, GRID_ADAMW, 4)) - {4})
ADAMW_ALL_VARIANTS_AT = (257, GRID_ADAMW * T_ + 1)  # a block + 1; the capped grid + 1
# one of p, m, v a float off 16 bytes (k_adamw_clip's scalar loop over everything, V = 1): a block + 1, the capped grid's second scalar trip;
# and the size at which the aligned run they are compared with takes its second vector trip plus a tail
ADAMW_OFF16_SIZES = (257, GRID_ADAMW * T_ + 1, 4 * GRID_ADAMW * T_ + 5)
SUMSQ_BIG = [4 * (5 * GRID_ADAMW * T_ + 77) + r for r in (1, 2, 3)]  # paired loop twice (three times for 77 threads), single loop, tail r
ADAMW_LR, ADAMW_STEP = [1e-5, 1e-3, 0.1], [1, 2, 10, 1000, 1000000]


def _adamw_matrix():
    m = []
    for i, n in enumerate(ADAMW_SIZES):
        for j, var in enumerate(ADAMW_VARIANTS):
            if n in ADAMW_ALL_VARIANTS_AT or j == i % len(ADAMW_VARIANTS):
                m.append((n, 0, j))
    for i, n in enumerate(SUMSQ_BIG):  # grads aligned / one float off 16 bytes: base, grad_scale 0.125, clipping inactive
        m += [(n, 0, (0, 4, 1)[i]), (n, 1, (4, 1, 0)[i])]
    return m


ADAMW_MATRIX = _adamw_matrix()


def sumsq_units(n, aligned=True):
    grid = min(cdiv(n, T_), GRID_ADAMW)
    n4 = n // 4 if aligned else 0
    return reduction_units(4 * cdiv(n4, grid * T_) + cdiv(n - 4 * n4, grid * T_), grid)


def adamw_case(n, cfg, aligned=True, fp32=False, seed=0):
    """one step from a random state (p ~ N(0,1), m ~ 0.1 N(0,1), v = (0.1 N(0,1))^2; zero moments at step 1) with a gradient scaled to a
    norm of 3 max_norm (clipping active), max_norm / 2 (inactive) or 20 (disabled), counted after grad_scale"""
    from oracle import dq_oracle as O

    cfg = {**ADAMW_BASE, **cfg}
    g_ = gen(n, cfg["step"], int(cfg["lr"] * 1e6), int(cfg["grad_scale"] * 8), seed + (0 if aligned else 1))
    p = torch.randn(n, generator=g_)
    m, v = 0.1 * torch.randn(n, generator=g_), (0.1 * torch.randn(n, generator=g_)) ** 2
    if cfg["step"] == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    gr = torch.randn(n, generator=g_).double()
    target = {"active": 3 * cfg["max_norm"], "inactive": 0.5 * cfg["max_norm"], "disabled": 20.0}[cfg["mode"]]
    gr = (gr * (target / (float(gr.norm()) * cfg["grad_scale"]))).float()
    if cfg["zero"]:
        gr, m = torch.zeros(n), torch.zeros(n)
    c = {"p": p, "g": gr, "m": m, "v": v, "cfg": cfg}
    hyper = (cfg["grad_scale"], cfg["max_norm"], cfg["lr"], B1, B2, EPS, cfg["wd"], cfg["step"])
    P, G, M, V = p.double(), gr.double(), m.double(), v.double()
    c["ref_p"], c["ref_m"], c["ref_v"], norm = O.adamw_clip_step(P, G, M, V, *hyper)
    c["ref_norm"] = float(norm)
    active = cfg["max_norm"] > 0 and c["ref_norm"] + 1e-6 > cfg["max_norm"]
    assert active == (cfg["mode"] == "active" and not cfg["zero"]), (c["ref_norm"], cfg)
    # S and the sensitivity to the clip coefficient, from the oracle's own intermediates
    f = lambda x: float(np.float32(x))
    bc1, bc2 = 1 - B1 ** cfg["step"], 1 - B2 ** cfg["step"]
    coef = min(1.0, cfg["max_norm"] / (c["ref_norm"] + f(1e-6))) if cfg["max_norm"] > 0 else 1.0
    gi = (G * cfg["grad_scale"] * coef).abs()
    s_m = M.abs() + f(1 - B1) * (gi + M.abs())
    denom = c["ref_v"].sqrt() / f(math.sqrt(bc2)) + f(EPS)
    c["S_m"], c["S_v"] = s_m, c["ref_v"]
    c["S_p"] = P.abs() * f(1 - cfg["lr"] * cfg["wd"]) + f(cfg["lr"] / bc1) * s_m / denom
    units = (sumsq_units(n, aligned) + 4) * U if active else 0.0
    sg_m, sg_v = f(1 - B1) * gi, 2 * f(1 - B2) * gi * gi
    rootv = c["ref_v"].sqrt() * f(math.sqrt(bc2))
    d_denom = torch.where(sg_v > 0, sg_v / (2 * rootv).clamp_min(1e-300), torch.zeros_like(sg_v))
    c["X_m"], c["X_v"] = units * sg_m, units * sg_v
    c["X_p"] = units * f(cfg["lr"] / bc1) * (sg_m / denom + c["ref_m"].abs() * d_denom / (denom * denom))
    c["cap_p"] = CAP_P * max(1.0, cfg["lr"] / 1e-3)
    c["norm_bound"] = min(sumsq_units(n, aligned) * U, CAP_GNORM) * c["ref_norm"]
    if fp32:
        c["fp32"] = O.adamw_clip_step(p, gr, m, v, *hyper)
    return c


def adamw_ratios(c, p, m, v):
    """p is held to the older test's absolute cap as well (CAP_P at lr 1e-3, in proportion above it) wherever the step is one that test could
    have seen: S_p <= CAP_P_SCALE, a unit-scale parameter moved by a few lr.  (m / sqrt(v) of an independent random m and v is heavy-tailed;
    where v is tiny the update, and S_p with it, is as large as it likes, and no absolute figure can hold.)"""
    r = {"m": ratio(m, c["ref_m"], c["S_m"], K_M, extra=c["X_m"]), "v": ratio(v, c["ref_v"], c["S_v"], K_V, extra=c["X_v"]),
         "p": ratio(p, c["ref_p"], c["S_p"], K_P, extra=c["X_p"])}
    err = (p.detach().cpu().double() - c["ref_p"]).abs()
    r["p cap"] = float(torch.where(c["S_p"] <= CAP_P_SCALE, err, torch.zeros_like(err)).max()) / c["cap_p"]
    return r


# ---- GPU plumbing -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


CANARY_BITS = int(np.float32(CANARY).view(np.int32))


class Pad:
    """n floats between canaries (compared bitwise through an int view); offset 1: the view starts one float off 16 bytes"""

    def __init__(self, src, offset=0):
        n = src if isinstance(src, int) else src.numel()
        self.buf = torch.full((HEAD + offset + n + TAIL,), CANARY, device="cuda")
        self.lo, self.n = HEAD + offset, n
        self.view = self.buf[self.lo:self.lo + n]
        assert (self.view.data_ptr() % 16 == 0) == (offset % 4 == 0)
        if isinstance(src, int):
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(src.reshape(-1))

    def intact(self):
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        return bool((bits[:self.lo] == CANARY_BITS).all()) and bool((bits[self.lo + self.n:] == CANARY_BITS).all())

    def all_nan(self):
        return bool(torch.isnan(self.view).all())


def call(N, name, *args):
    N.check(getattr(N.lib(), name)(*args, N.stream_ptr()), name)
    torch.cuda.synchronize()


# ---- q_sample -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["cosine", "linear"])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("B,per", Q_CASES)
def test_q_sample(N, B, per, normalize, kind):
    c = q_case(B, per, normalize, kind)
    ab, x0, t, nz = c["ab"].cuda(), c["x0"].cuda(), c["t"].cuda(), c["nz"].cuda()
    out = Pad(B * per)
    call(N, "dq_q_sample", N.ptr(ab), N.ptr(x0), N.ptr(t), N.ptr(nz), N.ptr(out.view), B, per, normalize)
    r = ratio(out.view, c["ref"], c["S"], K_Q, CAP_Q)
    print(f"q_sample B {B} per_sample {per} normalize {normalize} {kind}: err / bound {r:.3f}")
    assert r <= 1.0
    assert out.intact() and torch.equal(x0.cpu(), c["x0"]) and torch.equal(nz.cpu(), c["nz"])


# ---- ddim_step / ddim_step_x0 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", DDIM_T)
@pytest.mark.parametrize("n", DDIM_SIZES)
def test_ddim_step(N, n, t):
    c = ddim_case(n, t)
    x, e, x0, coef = c["x"].cuda(), c["eps"].cuda(), c["x0"].cuda(), c["coef"].cuda()
    # pred_type 'eps': out of place, then in place (x_prev == x_t, as dq_ddim_sample's graph path calls it)
    out = Pad(n)
    call(N, "dq_ddim_step", N.ptr(x), N.ptr(e), N.ptr(out.view), N.ptr(coef), n)
    r = {"eps-form": ratio(out.view, c["ref"], c["S"], K_DDIM, CAP_DDIM)}
    inp = Pad(x)
    call(N, "dq_ddim_step", N.ptr(inp.view), N.ptr(e), N.ptr(inp.view), N.ptr(coef), n)
    assert torch.equal(inp.view, out.view)
    # pred_type 'x0': eps_out given / NULL, out of place / in place
    xp, eo = Pad(n), Pad(n)
    call(N, "dq_ddim_step_x0", N.ptr(x), N.ptr(x0), N.ptr(xp.view), N.ptr(eo.view), N.ptr(coef), n)
    r["x0-form"] = ratio(xp.view, c["ref_xp"], c["S_xp"], K_DDIM_X0, CAP_DDIM)
    r["eps_out"] = ratio(eo.view, c["ref_eps"], c["S_eps"], K_DDIM_EPS, CAP_DDIM)
    xp2 = Pad(n)
    call(N, "dq_ddim_step_x0", N.ptr(x), N.ptr(x0), N.ptr(xp2.view), None, N.ptr(coef), n)
    assert torch.equal(xp2.view, xp.view)
    for eps_out in (Pad(n), None):
        inp2 = Pad(x)
        call(N, "dq_ddim_step_x0", N.ptr(inp2.view), N.ptr(x0), N.ptr(inp2.view), None if eps_out is None else N.ptr(eps_out.view), N.ptr(coef), n)
        assert torch.equal(inp2.view, xp.view) and inp2.intact()
        assert eps_out is None or (torch.equal(eps_out.view, eo.view) and eps_out.intact())
    print(f"ddim n {n} t {t}: err / bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert all(b.intact() for b in (out, inp, xp, eo, xp2))
    assert torch.equal(x.cpu(), c["x"]) and torch.equal(e.cpu(), c["eps"]) and torch.equal(x0.cpu(), c["x0"])


@pytest.mark.parametrize("t", DDIM_T)
@pytest.mark.parametrize("n", [4, 4 * T_ + 4])
def test_ddim_step_one_float_off_16_bytes(N, n, t):
    """n % 4 == 0 with x_t, the network output, x_prev (and eps_out) one float off 16 bytes: the one-element form, never 16-byte accesses at
    such addresses.  The bounds of test_ddim_step, and the aligned run's results bit for bit (the arithmetic of an element does not depend
    on the form)."""
    c = ddim_case(n, t)
    coef = c["coef"].cuda()
    res = {}
    for off in (0, 1):
        x, e, x0 = Pad(c["x"], off), Pad(c["eps"], off), Pad(c["x0"], off)
        out, xp, eo = Pad(n, off), Pad(n, off), Pad(n, off)
        call(N, "dq_ddim_step", N.ptr(x.view), N.ptr(e.view), N.ptr(out.view), N.ptr(coef), n)
        call(N, "dq_ddim_step_x0", N.ptr(x.view), N.ptr(x0.view), N.ptr(xp.view), N.ptr(eo.view), N.ptr(coef), n)
        assert all(b.intact() for b in (x, e, x0, out, xp, eo))
        assert torch.equal(x.view.cpu(), c["x"]) and torch.equal(e.view.cpu(), c["eps"]) and torch.equal(x0.view.cpu(), c["x0"])
        res[off] = (out.view.clone(), xp.view.clone(), eo.view.clone())
    out, xp, eo = res[1]
    r = {"eps-form": ratio(out, c["ref"], c["S"], K_DDIM, CAP_DDIM), "x0-form": ratio(xp, c["ref_xp"], c["S_xp"], K_DDIM_X0, CAP_DDIM),
         "eps_out": ratio(eo, c["ref_eps"], c["S_eps"], K_DDIM_EPS, CAP_DDIM)}
    print(f"ddim n {n} t {t}, one float off 16 bytes: err / bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


# ---- MSE ----------------------------------------------------------------------------------------------------------------------------

def _run_mse(N, c, weighted, B, per, tm, ta):
    """three calls: with grad_out, again (the loss must repeat bit for bit), with grad_out = NULL; scratch of exactly 1024 floats"""
    e, z = c["e"].cuda(), c["z"].cuda()
    lw, t = (c["lw"].cuda(), c["t"].cuda()) if weighted else (None, None)
    losses, grad = [], None
    for want_grad in (True, True, False):
        lo, gr, sc = Pad(1), Pad(c["n"]), Pad(SCRATCH)
        g_ptr = N.ptr(gr.view) if want_grad else None
        if weighted:
            call(N, "dq_mse_loss_weighted_fwd_bwd", N.ptr(e), N.ptr(z), tm, ta, N.ptr(lw), N.ptr(t), N.ptr(lo.view), g_ptr, N.ptr(sc.view), B, per)
        else:
            call(N, "dq_mse_loss_fwd_bwd", N.ptr(e), N.ptr(z), N.ptr(lo.view), g_ptr, N.ptr(sc.view), c["n"])
        assert lo.intact() and gr.intact() and sc.intact()
        assert want_grad or gr.all_nan()
        losses.append(lo.view.clone())
        grad = gr.view.clone() if want_grad and grad is None else grad
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2]), losses
    assert torch.equal(e.cpu(), c["e"]) and torch.equal(z.cpu(), c["z"])
    return float(losses[0]), grad


@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse(N, n):
    c = mse_case(1, n)
    loss, grad = _run_mse(N, c, False, 1, n, 1.0, 0.0)
    r = {"loss": abs(loss - c["loss"]) / c["loss_bound"], "grad": ratio(grad, c["grad"], c["S_grad"], K_MSE)}
    print(f"mse n {n}: loss {loss:.8g} (float64 {c['loss']:.8g}) err / bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("tm,ta", WMSE_MAPS)
@pytest.mark.parametrize("B,per", WMSE_CASES)
def test_mse_weighted(N, B, per, tm, ta):
    c = mse_case(B, per, tm, ta)
    loss, grad = _run_mse(N, c, True, B, per, tm, ta)
    r = {"loss": abs(loss - c["loss"]) / c["loss_bound"], "grad": ratio(grad, c["grad"], c["S_grad"], K_WMSE)}
    print(f"weighted mse B {B} per_sample {per} map ({tm}, {ta}): loss {loss:.8g} (float64 {c['loss']:.8g}) err / bound "
          + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


def _negative_zeros(n, weighted):
    c = {"e": torch.full((1, n), -0.0), "z": torch.full((1, n), -0.0), "n": n}
    if weighted:
        c["lw"], c["t"] = snr_table(), torch.tensor([500])
    return c


@pytest.mark.parametrize("n", [4, 5])
def test_mse_negative_zero(N, n):
    """pred and target -0.0 in every element (V = 4 and V = 1): the unweighted form takes the target as it lies, d = -0 - -0 = +0, and the
    gradient is +0.0 to the sign bit.  (A target mapped as z * 1 + 0 would be +0, d = -0 - +0 = -0, and the gradient -0.0.)"""
    loss, grad = _run_mse(N, _negative_zeros(n, False), False, 1, n, 1.0, 0.0)
    g = grad.cpu().numpy()
    assert loss == 0.0 and not np.signbit(np.float32(loss))
    assert np.array_equal(g, np.zeros(n, np.float32)) and not np.signbit(g).any(), g


@pytest.mark.parametrize("n", [4, 5])
def test_mse_weighted_negative_zero(N, n):
    """the same inputs through the weighted form with the map (1, 0): it applies the map, so the sign of the zero gradient is that of
    (pred - (z * 1 + 0)) * ((2 / n) * w) evaluated in fp32"""
    c = _negative_zeros(n, True)
    loss, grad = _run_mse(N, c, True, 1, n, 1.0, 0.0)
    one, zero = np.float32(1.0), np.float32(0.0)
    d = c["e"].numpy().reshape(-1) - (c["z"].numpy().reshape(-1) * one + zero)
    want = d * (np.float32(2.0) / np.float32(n) * c["lw"][c["t"]].numpy().astype(np.float32)[0])
    g = grad.cpu().numpy()
    assert want.dtype == np.float32 and np.signbit(want).all()  # (-0 - +0 = -0: the case tells the two forms apart)
    assert loss == 0.0
    assert np.array_equal(g, want) and np.array_equal(np.signbit(g), np.signbit(want)), (g, want)


# ---- the MS1 term -------------------------------------------------------------------------------------------------------------------

def _run_ms1(N, c, B, RT, MZ):
    dev = lambda v: None if v is None else v.cuda()
    pred, x_t, target, ms1 = dev(c["pred"]), dev(c["x_t"]), dev(c["target"]), dev(c["ms1"])
    lw, t = dev(c.get("lw")), dev(c.get("t"))
    n = B * RT * MZ
    lo, gr, sc, sc2 = Pad(1), Pad(n), Pad(SCRATCH), Pad(5 * B * RT + B)
    g_ptr = N.ptr(gr.view) if c["grad_wanted"] else None
    if lw is None:
        call(N, "dq_mse_loss_fwd_bwd", N.ptr(pred), N.ptr(target), N.ptr(lo.view), g_ptr, N.ptr(sc.view), n)
    else:
        call(N, "dq_mse_loss_weighted_fwd_bwd", N.ptr(pred), N.ptr(target), 1.0, 0.0, N.ptr(lw), N.ptr(t), N.ptr(lo.view), g_ptr, N.ptr(sc.view), B, RT * MZ)
    call(N, "dq_ms1_loss_fwd_bwd", N.ptr(pred), N.ptr(x_t), N.ptr(ms1), c["cm"], c["ca"], N.ptr(lw), N.ptr(t), c["w"], N.ptr(lo.view), g_ptr,
         N.ptr(sc2.view), B, RT, MZ)
    assert all(b.intact() for b in (lo, gr, sc, sc2))
    assert torch.equal(pred.cpu(), c["pred"])
    return float(lo.view), gr.view


def _ms1_errors(c, loss, grad):
    e = {"loss": abs(loss - c["loss"]) / c["loss_bound"]}
    if c["grad_wanted"]:
        e["grad"] = float((grad.cpu().double() - c["grad"].reshape(-1)).abs().max() / c["grad"].abs().max()) / MS1_GRAD_TOL
    else:
        assert bool(torch.isnan(grad).all())
    return e


@pytest.mark.parametrize("B,RT,MZ,form,weights,w,grad", MS1_CASES)
def test_ms1_term(N, B, RT, MZ, form, weights, w, grad):
    c = ms1_case(B, RT, MZ, form, weights, w, grad)
    assert float(c["normalisers"].abs().min()) >= 0.1, c["normalisers"]  # (a precondition of the case, checked on its float64 reference)
    loss, g = _run_ms1(N, c, B, RT, MZ)
    e = _ms1_errors(c, loss, g)
    print(f"ms1 ({B}, {RT}, {MZ}) {form} weights {weights} w {w}: loss {loss:.8g} (float64 {c['loss']:.8g}) err / bound "
          + " ".join(f"{k} {v:.3f}" for k, v in e.items()))
    assert all(v <= 1.0 for v in e.values()), e


@pytest.mark.parametrize("B,RT,MZ,form,weights,w,grad", MS1_TIES)
def test_ms1_term_ties_go_to_the_first_maximum(N, B, RT, MZ, form, weights, w, grad):
    """equal maxima at two m/z positions of a row and at two RT rows of a sample: the gradient lands on the first, as torch.max does"""
    c = ms1_case(B, RT, MZ, form, weights, w, grad, ties=True)
    ref, scale = c["grad"], float(c["grad"].abs().max())
    (r1, r2), (m1, m2) = TIE_ROWS, TIE_MZ
    # the reference itself tells the two choices apart by far more than the tolerance
    assert float((ref[:, r1, m1] - ref[:, r1, m2]).abs().min()) > 100 * MS1_GRAD_TOL * scale
    assert float((ref[:, r1] - ref[:, r2]).abs().max(-1).values.min()) > 100 * MS1_GRAD_TOL * scale
    loss, g = _run_ms1(N, c, B, RT, MZ)
    e = _ms1_errors(c, loss, g)
    print(f"ms1 ties ({B}, {RT}, {MZ}) {form}: err / bound " + " ".join(f"{k} {v:.3f}" for k, v in e.items()))
    assert all(v <= 1.0 for v in e.values()), e
    g = g.cpu().double().reshape(B, RT, MZ)
    for a, b in ((g[:, r1, m1], ref[:, r1, m1]), (g[:, r1, m2], ref[:, r1, m2]), (g[:, r2], ref[:, r2])):
        assert float((a - b).abs().max()) <= MS1_GRAD_TOL * scale


# ---- AdamW --------------------------------------------------------------------------------------------------------------------------

class AdamWBufs:
    """offset: of the gradient; off16: the one of p, m, v that starts one float off 16 bytes"""

    def __init__(self, c, offset=0, off16=None):
        self.p, self.m, self.v = (Pad(c[k], 1 if k == off16 else 0) for k in ("p", "m", "v"))
        self.g = Pad(c["g"], offset)
        self.sc, self.gn = Pad(SCRATCH), Pad(1)

    def intact(self, c):
        return all(b.intact() for b in (self.p, self.m, self.v, self.g, self.sc, self.gn)) and torch.equal(self.g.view.cpu(), c["g"])


def _host_step(N, c, b, n, step=None, gnorm=True):
    cfg = c["cfg"]
    call(N, "dq_adamw_clip_step", N.ptr(b.p.view), N.ptr(b.g.view), N.ptr(b.m.view), N.ptr(b.v.view), n, N.ptr(b.sc.view), cfg["grad_scale"],
         cfg["max_norm"], cfg["lr"], B1, B2, EPS, cfg["wd"], cfg["step"] if step is None else step, N.ptr(b.gn.view) if gnorm else None)


@pytest.mark.parametrize("n,offset,variant", ADAMW_MATRIX)
def test_adamw_clip_step(N, n, offset, variant):
    c = adamw_case(n, ADAMW_VARIANTS[variant], aligned=offset == 0)
    cfg = c["cfg"]
    b = AdamWBufs(c, offset)
    _host_step(N, c, b, n, gnorm=cfg["gnorm"])
    r = adamw_ratios(c, b.p.view, b.m.view, b.v.view)
    if cfg["gnorm"]:
        gn = float(b.gn.view)
        r["gnorm"] = abs(gn - c["ref_norm"]) / c["norm_bound"] if c["ref_norm"] > 0 else (0.0 if gn == 0.0 else math.inf)
    else:
        assert b.gn.all_nan()
    print(f"adamw n {n} grads offset {offset} {ADAMW_VARIANTS[variant] or 'base'}: norm {c['ref_norm']:.6g} err / bound "
          + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    if cfg["zero"]:  # an all-zero gradient with m = 0: finite, and p moves by the decay alone
        assert torch.equal(b.p.view.cpu(), c["p"] * float(np.float32(1 - cfg["lr"] * cfg["wd"])))
        assert torch.equal(b.m.view.cpu(), torch.zeros(n)) and bool(torch.isfinite(b.v.view).all())
    assert b.intact(c)


@pytest.mark.parametrize("lr", ADAMW_LR)
@pytest.mark.parametrize("step", ADAMW_STEP)
def test_adamw_step_dev_is_bitwise_the_host_step(N, step, lr):
    """dq_adamw_clip_step at (step, lr) against the oracle; dq_adamw_clip_step_dev with *step_dev = step - 1 and lr as a (hi, lo) pair must
    equal it bit for bit (include/dq_hip.h), count the step, and do so again at step + 1"""
    n = GRID_ADAMW * T_ + 1
    c = adamw_case(n, dict(lr=lr, step=step), seed=5)
    cfg = c["cfg"]
    host, dev = AdamWBufs(c), AdamWBufs(c)
    hi = np.float32(lr)
    lr_dev = torch.tensor([float(hi), float(np.float32(lr - float(hi)))], device="cuda")
    step_dev = torch.tensor([step - 1], dtype=torch.int32, device="cuda")
    for k in (0, 1):
        _host_step(N, c, host, n, step=step + k)
        if k == 0:
            r = adamw_ratios(c, host.p.view, host.m.view, host.v.view)
            r["gnorm"] = abs(float(host.gn.view) - c["ref_norm"]) / c["norm_bound"]
            print(f"adamw step {step} lr {lr}: err / bound " + " ".join(f"{k_} {v:.3f}" for k_, v in r.items()))
            assert all(v <= 1.0 for v in r.values()), r
        call(N, "dq_adamw_clip_step_dev", N.ptr(dev.p.view), N.ptr(dev.g.view), N.ptr(dev.m.view), N.ptr(dev.v.view), n, N.ptr(dev.sc.view),
             cfg["grad_scale"], cfg["max_norm"], N.ptr(lr_dev), B1, B2, EPS, cfg["wd"], N.ptr(step_dev), N.ptr(dev.gn.view))
        assert int(step_dev) == step + k
        s = step + k
        bc1, bc2 = 1.0 - B1 ** s, 1.0 - B2 ** s
        casts = np.array([1.0 - lr * cfg["wd"], lr / bc1, math.sqrt(bc2)]).astype(np.float32)  # launch_adamw's (float)(...) scalars
        hyp = dev.sc.view[GRID_ADAMW:GRID_ADAMW + 3].cpu().numpy()
        assert np.array_equal(hyp, casts), (s, lr, hyp.tolist(), casts.tolist())
        for name in ("p", "m", "v", "gn"):
            assert torch.equal(getattr(dev, name).view, getattr(host, name).view), (name, s, lr, hyp.tolist(), casts.tolist())
    assert host.intact(c) and dev.intact(c)


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("off16", ["p", "m", "v"])
@pytest.mark.parametrize("n", ADAMW_OFF16_SIZES)
def test_adamw_one_buffer_off_16_bytes(N, n, off16, entry):
    """k_adamw_clip takes 16-byte accesses only when p, g, m and v are all 16-byte aligned: with one of p, m, v a float off, both plain
    entries run its scalar loop over the whole buffer.  The bounds of test_adamw_clip_step (the per-element bound does not depend on the
    path), and the aligned run's p, m, v and norm bit for bit."""
    c = adamw_case(n, {}, seed=7)
    cfg = c["cfg"]
    runs = []
    for off in (None, off16):
        b = AdamWBufs(c, 0, off)
        if entry == "host":
            _host_step(N, c, b, n)
        else:
            hi = np.float32(cfg["lr"])
            lr_dev = torch.tensor([float(hi), float(np.float32(cfg["lr"] - float(hi)))], device="cuda")
            step_dev = torch.tensor([cfg["step"] - 1], dtype=torch.int32, device="cuda")
            call(N, "dq_adamw_clip_step_dev", N.ptr(b.p.view), N.ptr(b.g.view), N.ptr(b.m.view), N.ptr(b.v.view), n, N.ptr(b.sc.view),
                 cfg["grad_scale"], cfg["max_norm"], N.ptr(lr_dev), B1, B2, EPS, cfg["wd"], N.ptr(step_dev), N.ptr(b.gn.view))
            assert int(step_dev) == cfg["step"]
        assert b.intact(c)
        runs.append(b)
    al, b = runs
    r = adamw_ratios(c, b.p.view, b.m.view, b.v.view)
    r["gnorm"] = abs(float(b.gn.view) - c["ref_norm"]) / c["norm_bound"]
    print(f"adamw {entry} n {n} {off16} one float off 16 bytes: err / bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    for name in ("p", "m", "v", "gn"):
        assert torch.equal(getattr(b, name).view, getattr(al, name).view), name


# ---- the sample epilogue ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("auto_normalize", [1, 0])
def test_sample_finish_beyond_one_sweep(golden, auto_normalize):
    """k_sample_finish through dq_ddim_sample (2-level toy network, one step, no graph) at B * RT * 8 > 2048 * 256 * 4 elements: out_noise
    and, with the trajectory requested in a second call, out_x, bit for bit from the device's own tensors"""
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)
    net.load_state_dict(sub(golden("tiny_diffusion.npz"), "w/"))
    dm = DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=NUM_T, beta_schedule_type="cosine", pred_type="eps",
                            auto_normalize=bool(auto_normalize), ms1_loss_weight=0.0, device="cuda")
    dm.use_graph = False
    B, RT, MZ = 657, 400, 8
    assert B * RT * MZ > GRID_STREAM * T_ * 4 and (B * RT * MZ // 4) % (GRID_STREAM * T_) != 0
    g = gen(B, RT, auto_normalize)
    x_T, c2, c1 = torch.randn(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, generator=g).cuda()
    out_x, out_n = dm.sample(x_T, c2, c1, num_steps=1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_x).all()) and bool(torch.isfinite(out_n).all())
    want_n = (((c2 * 2.0 - 1.0) + 1.0) * 0.5 - out_x) if auto_normalize else (c2 - out_x)
    assert torch.equal(out_n, want_n)
    x2, n2, traj_x, _ = dm.sample(x_T, c2, c1, num_steps=1, return_trajectory=True)
    torch.cuda.synchronize()
    x_last = traj_x[0]
    assert torch.equal(x2, (x_last + 1.0) * 0.5 if auto_normalize else x_last)
    assert torch.equal(x2, out_x) and torch.equal(n2, out_n)


# ---- rejections: host-side checks, nothing is launched ------------------------------------------------------------------------------

def test_rejections_leave_the_outputs_alone(N):
    L = N.lib()
    s = N.stream_ptr()
    ab, lw = alpha_bars().cuda(), snr_table().cuda()
    a, b = torch.randn(64, device="cuda"), torch.randn(64, device="cuda")
    t = torch.zeros(16, dtype=torch.int64, device="cuda")
    coef = coef_row(500).cuda()
    lr_dev, step_dev = torch.tensor([1e-3, 0.0], device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    out, out2, sc = Pad(64), Pad(64), Pad(SCRATCH)
    o, o2, scp = N.ptr(out.view), N.ptr(out2.view), N.ptr(sc.view)
    pa, pb = N.ptr(a), N.ptr(b)
    adam = (0.9, 0.999, 1e-8, 0.01)
    calls = {
        "q_sample, per_sample -4": lambda: L.dq_q_sample(N.ptr(ab), pa, N.ptr(t), pb, o, 2, -4, 1, s),
        "ddim_step, n -4": lambda: L.dq_ddim_step(pa, pb, o, N.ptr(coef), -4, s),
        "ddim_step_x0, n -4": lambda: L.dq_ddim_step_x0(pa, pb, o, o2, N.ptr(coef), -4, s),
        "mse, n -4": lambda: L.dq_mse_loss_fwd_bwd(pa, pb, o2, o, scp, -4, s),
        "mse, n 0": lambda: L.dq_mse_loss_fwd_bwd(pa, pb, o2, o, scp, 0, s),
        "weighted mse, per_sample 0": lambda: L.dq_mse_loss_weighted_fwd_bwd(pa, pb, 1.0, 0.0, N.ptr(lw), N.ptr(t), o2, o, scp, 3, 0, s),
        "weighted mse, B 0": lambda: L.dq_mse_loss_weighted_fwd_bwd(pa, pb, 1.0, 0.0, N.ptr(lw), N.ptr(t), o2, o, scp, 0, 8, s),
        "adamw, n 0": lambda: L.dq_adamw_clip_step(o, pa, o2, o2, 0, scp, 1.0, 10.0, 1e-3, *adam, 1, None, s),
        "adamw, step 0": lambda: L.dq_adamw_clip_step(o, pa, o2, o2, 16, scp, 1.0, 10.0, 1e-3, *adam, 0, None, s),
        "adamw_dev, n 0": lambda: L.dq_adamw_clip_step_dev(o, pa, o2, o2, 0, scp, 1.0, 10.0, N.ptr(lr_dev), *adam, N.ptr(step_dev), None, s),
        "ms1, w 0": lambda: L.dq_ms1_loss_fwd_bwd(pa, pb, pa, 2.0, -1.0, None, None, 0.0, o2, o, scp, 1, 2, 8, s),
        "ms1, w 1.5": lambda: L.dq_ms1_loss_fwd_bwd(pa, pb, pa, 2.0, -1.0, None, None, 1.5, o2, o, scp, 1, 2, 8, s),
    }
    for what, fn in calls.items():
        rc = fn()
        torch.cuda.synchronize()
        assert rc != 0, what
        assert L.dq_last_error(), what
        assert out.all_nan() and out2.all_nan() and sc.all_nan(), what
        assert out.intact() and out2.intact() and sc.intact() and int(step_dev) == 0, what
    # an empty call is no error, and writes nothing
    for what, fn in {"q_sample, B 0": lambda: L.dq_q_sample(N.ptr(ab), pa, N.ptr(t), pb, o, 0, 8, 1, s),
                     "q_sample, per_sample 0": lambda: L.dq_q_sample(N.ptr(ab), pa, N.ptr(t), pb, o, 2, 0, 1, s),
                     "ddim_step, n 0": lambda: L.dq_ddim_step(pa, pb, o, N.ptr(coef), 0, s),
                     "ddim_step_x0, n 0": lambda: L.dq_ddim_step_x0(pa, pb, o, o2, N.ptr(coef), 0, s)}.items():
        rc = fn()
        torch.cuda.synchronize()
        assert rc == 0, (what, L.dq_last_error())
        assert out.all_nan() and out2.all_nan() and out.intact() and out2.intact(), what
