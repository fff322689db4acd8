"""References of the mixture-consistency rule (csrc/k_group.hip), shared by tests/test_joint_host.py,
tests/test_joint_kernel.py and tests/test_joint_sample.py.  No test lives here.

``project_f32``: the numpy float32 transcription -- every operation one rounded fp32 operation in the kernel's order, so the kernel must
reproduce every bit.  ``project_f64``: the rule in float64 over the same fp32 inputs, with a running error bound for the fp32 evaluation.

The bound (u = 2^-24; every fp32 operation contributes u |its result|, every operand's error is carried to first order through the
operation that reads it; nothing here is measured):
  x0    eps objective (x - sb v) / sa: product, difference, quotient      3 u (|x| + sb |v|) / sa
        v objective sa x - sb v: a product and the difference on a path   2 u (sa |x| + sb |v|)
        x0 objective: the operand itself                                  0
  y     (x0 + 1) * 0.5: the sum rounds, the halving is exact              b_y = (b_x0 + u (|x0| + 1)) / 2      (no normalisation: b_x0)
  S     P - 1 sums over the positive parts                                b_S = sum_p b_y,p + (P - 1) u S
  f     m / S: the quotient rounds, S's error enters relatively           b_f = f (u + b_S / (S - b_S))
  z     y f (or yp f): one product                                        b_z = |y| b_f + f b_y + u |y f|       (m / P: u m / P)
  y'    y + s (z - y): difference, product, sum (s == 1: y' = z)          b_y' = b_y + s (b_z + b_y + u |z - y|) + u |s (z - y)| + u |y'|
  x0'   2 y' - 1: the doubling is exact, the difference rounds            2 b_y' + u |2 y' - 1|                (no normalisation: b_y')
An element that the rule does not move is x0 itself, bound b_x0.  A decision of the rule taken the other way in fp32 moves the result by
no more than the distance between the two branches at the threshold, which is added where the float64 operands lie within their bounds of
it: |S - m| <= b_S (BOUND: z is y f with f within b_f of 1, against y), |y| <= b_y (the branches differ by at most b_y (1 + f)).  Where
S <= 4 b_S the quotient's bound is meaningless and ``bound`` is +inf: such elements are not compared (the bit-for-bit check covers them)."""
import numpy as np

F = np.float32
U = 2.0 ** -24
MODES = {"bound": 1, "sum": 2}
PREDS = {"eps": 0, "x0": 1, "v_prediction": 2}


def x0_f32(pred, sa, sb, x, net):
    """net_x0<PRED> of csrc/dq_x0.h in float32, operation by operation"""
    sa, sb = F(sa), F(sb)
    if pred == "x0":
        return net.astype(F, copy=True)
    if pred == "eps":
        return (x - sb * net) / sa
    return sa * x - sb * net


def project_f32(x0, mix, mode, strength=1.0, normalize=True):
    """x0 (P, G, per) fp32, mix (G, per) fp32 -> (x0' (P, G, per) fp32, parts): the rule, step by step.  parts: y, y' (image units), S,
    m and where the rule acted, for the properties"""
    assert x0.dtype == F and mix.dtype == F and mode in MODES
    P = x0.shape[0]
    y = (x0 + F(1)) * F(0.5) if normalize else x0
    yp = np.where(y > 0, y, F(0))
    S = yp[0].copy()
    for p in range(1, P):
        S = S + yp[p]
    m = np.where(mix > 0, mix, F(0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        f = m / S
        if mode == "bound":
            act = S > m
            z = np.where(act[None] & (y > 0), y * f[None], y)
        else:
            act = S > 0
            z = np.where(act[None], yp * f[None], np.broadcast_to((m / F(P))[None], y.shape))
    s = F(strength)
    yn = z if s == F(1) else y + s * (z - y)
    back = F(2) * yn - F(1) if normalize else yn
    out = np.where(yn == y, x0, back)
    assert out.dtype == F and yn.dtype == F and S.dtype == F
    return out, dict(y=y, yn=yn, S=S, m=m, act=act)


def project_f64(pred, sa, sb, x, net, mix, mode, strength=1.0, normalize=True):
    """The rule in float64 from the fp32 operands (sa, sb the fp32 row values) -> (x0' float64, bound): see the module docstring"""
    sa, sb = float(F(sa)), float(F(sb))
    x, v, mix = x.astype(np.float64), net.astype(np.float64), mix.astype(np.float64)
    P = v.shape[0]
    if pred == "x0":
        x0, b0 = v, np.zeros_like(v)
    elif pred == "eps":
        x0, b0 = (x - sb * v) / sa, 3 * U * (np.abs(x) + sb * np.abs(v)) / sa
    else:
        x0, b0 = sa * x - sb * v, 2 * U * (sa * np.abs(x) + sb * np.abs(v))
    if normalize:
        y, by = (x0 + 1) * 0.5, (b0 + U * (np.abs(x0) + 1)) * 0.5
    else:
        y, by = x0, b0
    yp = np.maximum(y, 0)
    S, m = yp.sum(axis=0), np.maximum(mix, 0)
    bS = by.sum(axis=0) + (P - 1) * U * S
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        f = m / S
        bf = f * (U + bS / (S - bS))
        if mode == "bound":
            act = S > m
            z = np.where(act[None] & (y > 0), y * f[None], y)
            bz = np.where(act[None] & (y > 0), np.abs(y) * bf[None] + f[None] * by + U * np.abs(y * f[None]), by)
            # a decision taken the other way: z is y f against y, f within its bound of 1 where S is within b_S of m
            flip = np.where((np.abs(S - m) <= bS)[None], np.abs(y) * (bf + np.abs(1 - f))[None], 0.0)
            flip = flip + np.where(act[None] & (np.abs(y) <= by), by * (1 + f[None]), 0.0)
            unsafe = act & ~(S > 4 * bS)
        else:
            act = S > 0
            even = np.broadcast_to((m / P)[None], y.shape)
            z = np.where(act[None], yp * f[None], even)
            bz = np.where(act[None], np.abs(yp) * bf[None] + f[None] * by + U * np.abs(yp * f[None]), U * even)
            flip = np.where(act[None] & (np.abs(y) <= by), by * (1 + f[None]), 0.0)
            # (S == 0 with every member clearly below 0 is the m / P branch in both; with a member within its bound of 0 either may be taken)
            unsafe = ~(S > 4 * bS) & ((S > 0) | (np.abs(y) <= by).any(axis=0))
    s = float(F(strength))
    if s == 1.0:
        yn, byn = z, bz + flip
    else:
        d = z - y
        yn = y + s * d
        byn = by + s * (bz + flip + by + U * np.abs(d)) + U * np.abs(s * d) + U * np.abs(yn)
    if normalize:
        out, bound = 2 * yn - 1, 2 * byn + U * np.abs(2 * yn - 1)
    else:
        out, bound = yn, byn
    moved = yn != y
    # (not moved in float64: x0 itself -- unless a decision may flip, then fp32 may have moved it, by no more than the moved form's bound)
    out, bound = np.where(moved, out, x0), np.where(moved | (flip > 0), np.maximum(bound, b0), b0)
    bound = np.where(np.broadcast_to(unsafe[None], bound.shape), np.inf, bound)
    return out, bound


def inputs(rng, P, G, per, spread=1.0):
    """x_t, net (P, G, per) and a mixture (G, per) in [0, 1] with exact zeros in it, fp32: estimates on both sides of 0 and of the mixture"""
    x = rng.standard_normal((P, G, per)).astype(F)
    net = (spread * rng.standard_normal((P, G, per))).astype(F)
    mix = rng.random((G, per)).astype(F)
    mix[rng.random((G, per)) < 0.05] = 0
    return x, net, mix
