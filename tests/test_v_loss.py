"""The loss kernels of the v objective (csrc/k_stream.hip): dq_mse_loss_v_fwd_bwd (k_mse_fwd_bwd<MseV, 4> / <MseV, 1>) and
dq_mse_per_window_v (k_mse_per_window<PwV>).  The target z = sa_b * noise - sb_b * (x0 * tm + ta), sa_b = sqrt(ab[t_b]), sb_b = sqrt(1 - ab[t_b]),
is formed inside the kernels.

Shapes: B = 3 with t = [0, 500, 999] at per = 8 (the vector form; a window boundary inside a block's float4 stride) and per = 5 (the
one-element form, n % 4 != 0), and the grid-stride and scratch edges of tests/test_stream_kernels.py (WMSE_CASES) and tests/test_eval_step.py
(PER_EDGES, B_EDGES); with and without the weight table, at (tm, ta) = (2, -1) and (1, 0).

Reference: float64 over the same fp32 inputs (sa, sb from the fp32 alpha-bar table in float64).  Tolerances: those of the weighted form in
tests/test_stream_kernels.py, imported -- the gradient K_WMSE 2^-24 S with S the gradient's sum of magnitudes 2 w (|e| + sa |noise| + sb (|x0 tm| +
|ta|)) / n, the loss mse_units 2^-24 sum w S_d^2 / n capped at CAP_LOSS |loss|.  The per-window sums are fp64 (tests/test_eval_step.py: one fp32
rounding, 2 * 2^-24 |ref| + 1e-9) over fp32 differences whose target carries the roundings above: |d_fp32 - d| <= K_WMSE 2^-24 S_d, so a
window's mean of squares moves by at most 2 K_WMSE 2^-24 mean(S_d^2), which is added.  A table of all ones gives the bits of lw = NULL."""
import numpy as np
import pytest
import torch

from test_eval_step import B_EDGES, MSE_PW_SLICE, PER_EDGES
from test_stream_kernels import CAP_LOSS, K_WMSE, NUM_T, SCRATCH, U, WMSE_CASES, WMSE_MAPS, Pad, alpha_bars, call, cdiv, gen, mse_units, ratio, timesteps

pytestmark = pytest.mark.gpu

T3 = [0, 500, NUM_T - 1]
SMALL = [(3, 8), (3, 5)]
# the weighted form's cases with at most ~2M elements each side of its sweep edges (a case there costs three tensors, not two)
LOSS_CASES = SMALL + WMSE_CASES


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


def v_case(B, per, tm, ta, weighted):
    g = gen(B, per, 11 + int(tm), weighted)
    ab = alpha_bars()
    e, nz = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g)
    x0 = torch.rand(B, per, generator=g) if tm == 2.0 else torch.rand(B, per, generator=g) * 2 - 1
    t = torch.tensor(T3) if B == 3 else timesteps(B, [0, NUM_T - 1, 0, 500, NUM_T - 1, 3, 996]) if B > 1 else torch.tensor([500])
    lw = (torch.rand(NUM_T, generator=g) * 50 + 0.01) if weighted else None
    a = ab.double()[t][:, None]
    sa, sb = a.sqrt(), (1 - a).sqrt()
    w = lw.double()[t][:, None] if weighted else torch.ones(B, 1, dtype=torch.float64)
    n = B * per
    d = e.double() - (sa * nz.double() - sb * (x0.double() * tm + ta))
    absd = e.double().abs() + sa * nz.double().abs() + sb * ((x0.double() * tm).abs() + abs(ta))
    c = dict(ab=ab, e=e, nz=nz, x0=x0, t=t, lw=lw, n=n, d=d, absd=absd, w=w)
    c["loss"] = float((w * d * d).sum() / n)
    c["grad"], c["S_grad"] = 2 * d * w / n, 2 * absd * w / n
    c["loss_bound"] = min(mse_units(n, 1 if per % 4 else 4) * U * float((w * absd * absd).sum() / n), CAP_LOSS * abs(c["loss"]))
    c["pw"] = (d * d).mean(dim=1)
    c["pw_bound"] = 2 * K_WMSE * U * (absd * absd).mean(dim=1) + 2 * U * c["pw"] + 1e-9
    c["pw_loss"] = float((w[:, 0] * c["pw"]).mean())
    c["pw_loss_bound"] = float((w[:, 0] * c["pw_bound"]).mean()) + 2 * U * abs(c["pw_loss"])
    return c


def run_loss(N, c, B, per, tm, ta, lw):
    """three calls as tests/test_stream_kernels.py::_run_mse: with grad_out, again (bit for bit), with grad_out = NULL; 1024 floats of scratch"""
    dev = {k: c[k].cuda() for k in ("e", "x0", "nz", "ab", "t")}
    lw_d = None if lw is None else lw.cuda()
    losses, grad = [], None
    for want_grad in (True, True, False):
        lo, gr, sc = Pad(1), Pad(c["n"]), Pad(SCRATCH)
        call(N, "dq_mse_loss_v_fwd_bwd", N.ptr(dev["e"]), N.ptr(dev["x0"]), N.ptr(dev["nz"]), N.ptr(dev["ab"]), tm, ta, N.ptr(lw_d), N.ptr(dev["t"]),
             N.ptr(lo.view), N.ptr(gr.view) if want_grad else None, N.ptr(sc.view), B, per)
        assert lo.intact() and gr.intact() and sc.intact()
        assert want_grad or gr.all_nan()
        losses.append(lo.view.clone())
        grad = gr.view.clone() if want_grad and grad is None else grad
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2]), losses
    assert all(torch.equal(dev[k].cpu(), c[k]) for k in ("e", "x0", "nz"))
    return losses[0], grad


@pytest.mark.parametrize("weighted", [0, 1])
@pytest.mark.parametrize("tm,ta", WMSE_MAPS)
@pytest.mark.parametrize("B,per", LOSS_CASES)
def test_mse_v_fwd_bwd(N, B, per, tm, ta, weighted):
    c = v_case(B, per, tm, ta, weighted)
    loss, grad = run_loss(N, c, B, per, tm, ta, c["lw"])
    r = {"loss": abs(float(loss) - c["loss"]) / c["loss_bound"], "grad": ratio(grad, c["grad"], c["S_grad"], K_WMSE)}
    print(f"v mse B {B} per {per} map ({tm}, {ta}) weighted {weighted}: loss {float(loss):.8g} (float64 {c['loss']:.8g}) err / bound "
          + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    if not weighted:  # a table of all ones: the bits of lw = NULL
        loss1, grad1 = run_loss(N, c, B, per, tm, ta, torch.ones(NUM_T))
        assert torch.equal(loss1, loss) and torch.equal(grad1, grad)


def test_mse_v_one_float_off_16_bytes(N):
    """per % 4 == 0 with the prediction one float off 16 bytes: the one-element form, and the aligned run's bits"""
    B, per = 3, 8
    c = v_case(B, per, 2.0, -1.0, 1)
    res = []
    for off in (0, 1):
        e, gr, lo, sc = Pad(c["e"], off), Pad(c["n"], off), Pad(1), Pad(SCRATCH)
        x0, nz, ab, t, lw = (c[k].cuda() for k in ("x0", "nz", "ab", "t", "lw"))
        call(N, "dq_mse_loss_v_fwd_bwd", N.ptr(e.view), N.ptr(x0), N.ptr(nz), N.ptr(ab), 2.0, -1.0, N.ptr(lw), N.ptr(t), N.ptr(lo.view), N.ptr(gr.view),
             N.ptr(sc.view), B, per)
        assert e.intact() and gr.intact() and lo.intact() and sc.intact()
        res.append((lo.view.clone(), gr.view.clone()))
    assert torch.equal(res[0][1], res[1][1])  # (an element's arithmetic does not depend on the form; the loss sums in another order)
    assert abs(float(res[1][0]) - c["loss"]) <= c["loss_bound"]


def run_pw(N, c, B, per, tm, ta, lw):
    nbytes = 8 * B * cdiv(per, MSE_PW_SLICE)
    assert N.lib().dq_mse_per_window_scratch_bytes(B, per) == nbytes
    pw, loss, scratch = Pad(B), Pad(1), Pad(nbytes // 4)
    dev = {k: c[k].cuda() for k in ("e", "x0", "nz", "ab", "t")}
    lw_d = None if lw is None else lw.cuda()
    call(N, "dq_mse_per_window_v", N.ptr(dev["e"]), N.ptr(dev["x0"]), N.ptr(dev["nz"]), N.ptr(dev["ab"]), tm, ta, N.ptr(lw_d), N.ptr(dev["t"]),
         N.ptr(pw.view), N.ptr(loss.view), N.ptr(scratch.view), B, per)
    assert pw.intact() and loss.intact() and scratch.intact()
    return pw.view.clone(), loss.view.clone()


@pytest.mark.parametrize("weighted", [0, 1])
@pytest.mark.parametrize("tm,ta", WMSE_MAPS)
@pytest.mark.parametrize("B,per", SMALL + [(3, p) for p in PER_EDGES] + [(b, 5) for b in B_EDGES] + [(1, 3 * 37 * 2)])
def test_mse_per_window_v(N, B, per, tm, ta, weighted):
    c = v_case(B, per, tm, ta, weighted)
    pw, loss = run_pw(N, c, B, per, tm, ta, c["lw"])
    r = {"per_window": float(((pw.cpu().double() - c["pw"]).abs() / c["pw_bound"]).max()),
         "loss": abs(float(loss) - c["pw_loss"]) / c["pw_loss_bound"]}
    print(f"v per-window B {B} per {per} map ({tm}, {ta}) weighted {weighted}: err / bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    if not weighted:
        pw1, loss1 = run_pw(N, c, B, per, tm, ta, torch.ones(NUM_T))
        assert torch.equal(pw1, pw) and torch.equal(loss1, loss)
    if B == 3:  # a window alone: its value in the batch, bit for bit (the partition of a window depends on per alone)
        for b in range(3):
            one = {k: (c[k][b:b + 1].contiguous() if k in ("e", "x0", "nz", "t") else c[k]) for k in ("e", "x0", "nz", "t", "ab")}
            pwb, _ = run_pw(N, one, 1, per, tm, ta, c["lw"])
            assert torch.equal(pwb, pw[b:b + 1]), b
