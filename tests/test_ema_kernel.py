"""dq_adamw_clip_ema_step / dq_adamw_clip_ema_step_dev (csrc/k_adamw.hip: k_adamw_clip<true>, k_adamw_hyper): the fused clip + AdamW
step that also keeps an exponential moving average e of the parameters.

  * p, m, v and the norm equal dq_adamw_clip_step's bit for bit from the same state: every size of SIZES (a block edge, the capped grid's
    second trip, a vector tail), all five buffers 16-byte aligned (the 16-byte path) and each of p, g, m, v, e in turn one float off (the
    scalar path), clipping active / inactive / disabled; canaries around every buffer, g unchanged.
  * e against float64, from the kernel's own fp32 p_new and the input e:  ref = e + w (p_new - e),
        |e_out - ref| <= 2 * 2^-24 * (w |p_new - e| + |ref|)
    -- one rounding of the difference carried through the product plus one rounding of the fmaf, times a margin of 2 (nothing here comes
    from the kernel's output).  w = float32(1 - beta_t) formed in double, beta_t = min(beta, (1 + t) / (10 + t)) with warm-up, beta
    without; beta is the float32 the C ABI takes, promoted to double.
  * the device-scalar variant from *step_dev = t - 1 equals the host variant at t bit for bit, counts the step, keeps w at index 3 behind
    the partial sums and the three AdamW scalars of tests/test_stream_kernels.py at 0..2; again at t + 1.
  * rejections launch nothing."""
import math

import numpy as np
import pytest
import torch

from test_stream_kernels import B1, B2, EPS, GRID_ADAMW, SCRATCH, T_, U, Pad, adamw_case, call

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 255, 256, 257, 1023, GRID_ADAMW * T_, GRID_ADAMW * T_ + 1, 4 * GRID_ADAMW * T_ + 5]
ALL_AT = (257, GRID_ADAMW * T_ + 1)  # every offset and every clipping mode: a block + 1, the capped grid + 1
MODES = [dict(), dict(mode="inactive"), dict(mode="disabled", max_norm=0.0)]  # clipping active, inactive, disabled
NAMES = ("p", "g", "m", "v", "e")  # offset k > 0: NAMES[k - 1] starts one float off 16 bytes, the other four are aligned
BETAS, STEPS = [0.0, 0.9, 0.9999], [1, 2, 10, 1000, 1000000]


def _matrix():
    out = []
    for i, n in enumerate(SIZES):
        for off in range(6):
            if n in ALL_AT:
                out += [(n, off, k) for k in range(3)]
            elif off == 0 or off == 1 + i % 5:
                out.append((n, off, (i + off) % 3))
    assert {n for n, _, _ in out} == set(SIZES) and {o for _, o, _ in out} == set(range(6))
    return out


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


def ema_weight(beta, warmup, t):
    """(float)(1 - beta_t) as include/dq_hip.h states it"""
    b = float(np.float32(beta))
    bt = min(b, (1 + t) / (10 + t)) if warmup else b
    return np.float32(1.0 - bt)


def ema_input(c, seed):
    g = torch.Generator().manual_seed(7919 * seed + c["p"].numel())
    return c["p"] + 0.05 * torch.randn(c["p"].numel(), generator=g)


class Bufs:
    def __init__(self, c, e, off=0):
        o = {name: int(off == k + 1) for k, name in enumerate(NAMES)}
        self.p, self.g, self.m, self.v = Pad(c["p"], o["p"]), Pad(c["g"], o["g"]), Pad(c["m"], o["m"]), Pad(c["v"], o["v"])
        self.e = Pad(e, o["e"])
        self.sc, self.gn = Pad(SCRATCH), Pad(1)

    def intact(self, c):
        return all(b.intact() for b in (self.p, self.g, self.m, self.v, self.e, self.sc, self.gn)) and torch.equal(self.g.view.cpu(), c["g"])


def plain_step(N, c, b, step):
    cfg = c["cfg"]
    call(N, "dq_adamw_clip_step", N.ptr(b.p.view), N.ptr(b.g.view), N.ptr(b.m.view), N.ptr(b.v.view), c["p"].numel(), N.ptr(b.sc.view),
         cfg["grad_scale"], cfg["max_norm"], cfg["lr"], B1, B2, EPS, cfg["wd"], step, N.ptr(b.gn.view))


def ema_step(N, c, b, step, beta, warmup):
    cfg = c["cfg"]
    call(N, "dq_adamw_clip_ema_step", N.ptr(b.p.view), N.ptr(b.g.view), N.ptr(b.m.view), N.ptr(b.v.view), c["p"].numel(), N.ptr(b.sc.view),
         cfg["grad_scale"], cfg["max_norm"], cfg["lr"], B1, B2, EPS, cfg["wd"], step, N.ptr(b.gn.view), N.ptr(b.e.view), beta, int(warmup))


def ema_step_dev(N, c, b, lr_dev, step_dev, beta, warmup):
    cfg = c["cfg"]
    call(N, "dq_adamw_clip_ema_step_dev", N.ptr(b.p.view), N.ptr(b.g.view), N.ptr(b.m.view), N.ptr(b.v.view), c["p"].numel(),
         N.ptr(b.sc.view), cfg["grad_scale"], cfg["max_norm"], N.ptr(lr_dev), B1, B2, EPS, cfg["wd"], N.ptr(step_dev), N.ptr(b.gn.view),
         N.ptr(b.e.view), beta, int(warmup))


def ema_ratio(e_out, p_new, e_in, w):
    """max |e_out - ref| / bound, the float64 reference taken from the kernel's own fp32 p_new"""
    P, E, w = p_new.detach().cpu().double(), e_in.double(), float(w)
    ref = E + w * (P - E)
    bound = 2 * U * (w * (P - E).abs() + ref.abs())
    err = (e_out.detach().cpu().double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("n,off,mode", _matrix())
def test_p_m_v_norm_are_bitwise_the_plain_step(N, n, off, mode):
    beta, warmup = 0.9, True
    c = adamw_case(n, MODES[mode], aligned=off != 2, seed=3)
    step = c["cfg"]["step"]
    e_in = ema_input(c, off)
    old, new = Bufs(c, e_in, off), Bufs(c, e_in, off)
    assert [getattr(new, k).view.data_ptr() % 16 == 0 for k in NAMES] == [off != k + 1 for k in range(5)]
    plain_step(N, c, old, step)
    ema_step(N, c, new, step, beta, warmup)
    for name in ("p", "m", "v", "gn"):
        assert torch.equal(getattr(new, name).view, getattr(old, name).view), (name, n, off, mode)
    assert torch.equal(old.e.view.cpu(), e_in)  # (the plain step knows no e)
    r = ema_ratio(new.e.view, new.p.view, e_in, ema_weight(beta, warmup, step))
    print(f"adamw + ema n {n} {'aligned' if off == 0 else NAMES[off - 1] + ' off by one float'} clipping {c['cfg']['mode']}: e err / bound {r:.3f}")
    assert r <= 1.0
    assert old.intact(c) and new.intact(c)


@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("beta", BETAS)
def test_ema_against_float64_and_the_device_scalar_variant(N, beta, warmup, t):
    n = 4 * T_ + 3  # four float4 per lane of the first block's worth, a tail of three, more than one block
    lr = 1e-3
    c = adamw_case(n, dict(step=t, lr=lr), seed=11)
    cfg = c["cfg"]
    e_in = ema_input(c, t % 97)
    host, dev = Bufs(c, e_in), Bufs(c, e_in)
    hi = np.float32(lr)
    lr_dev = torch.tensor([float(hi), float(np.float32(lr - float(hi)))], device="cuda")
    step_dev = torch.tensor([t - 1], dtype=torch.int32, device="cuda")
    if warmup and t == 1 and beta > 2 / 11:  # beta_1 = 2 / 11 (beta = 0 caps it at once)
        assert ema_weight(beta, warmup, t) == np.float32(1.0 - 2.0 / 11.0)
    if warmup and t == 1000000:
        assert ema_weight(beta, warmup, t) == np.float32(1.0 - float(np.float32(beta)))  # capped by beta
    for k in (0, 1):
        s = t + k
        w = ema_weight(beta, warmup, s)
        e_before = host.e.view.cpu().clone()
        ema_step(N, c, host, s, beta, warmup)
        r = ema_ratio(host.e.view, host.p.view, e_before, w)
        print(f"ema beta {beta} warm-up {warmup} step {s}: w {float(w):.9g} e err / bound {r:.3f}")
        assert r <= 1.0
        ema_step_dev(N, c, dev, lr_dev, step_dev, beta, warmup)
        assert int(step_dev) == s
        bc1, bc2 = 1.0 - B1 ** s, 1.0 - B2 ** s
        casts = np.array([1.0 - lr * cfg["wd"], lr / bc1, math.sqrt(bc2)]).astype(np.float32)  # as in test_stream_kernels.py
        hyp = dev.sc.view[GRID_ADAMW:GRID_ADAMW + 4].cpu().numpy()
        assert np.array_equal(hyp[:3], casts), (s, hyp.tolist(), casts.tolist())
        assert hyp[3].view(np.int32) == w.view(np.int32), (s, float(hyp[3]), float(w))
        for name in ("p", "m", "v", "e", "gn"):
            assert torch.equal(getattr(dev, name).view, getattr(host, name).view), (name, s, beta, warmup)
    assert host.intact(c) and dev.intact(c)


@pytest.mark.parametrize("n", [3, 4 * T_ + 3])
def test_ema_equal_to_the_parameters_stays_put_under_a_null_update(N, n):
    """e == p, a zero gradient, zero moments and wd = 0: p does not move and p - e = 0 leaves e as it is, bit for bit"""
    c = adamw_case(n, dict(zero=True, step=1, wd=0.0), seed=2)
    b = Bufs(c, c["p"])
    ema_step(N, c, b, 1, 0.9, True)
    assert torch.equal(b.p.view.cpu(), c["p"]) and torch.equal(b.e.view.cpu(), c["p"])
    assert b.intact(c)


def test_rejections_launch_nothing(N):
    L, s = N.lib(), N.stream_ptr()
    a = torch.randn(64, device="cuda")
    lr_dev, step_dev = torch.tensor([1e-3, 0.0], device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    out, out2, out3, sc = Pad(64), Pad(64), Pad(64), Pad(SCRATCH)
    o, o2, o3, scp = N.ptr(out.view), N.ptr(out2.view), N.ptr(out3.view), N.ptr(sc.view)
    adam = (0.9, 0.999, 1e-8, 0.01)
    bad = {"beta 1": (o3, 1.0), "beta -0.1": (o3, -0.1), "beta NaN": (o3, float("nan")), "null ema": (None, 0.9)}
    for what, (e, beta) in bad.items():
        for name, fn in {
            "host": lambda: L.dq_adamw_clip_ema_step(o, N.ptr(a), o2, o2, 64, scp, 1.0, 10.0, 1e-3, *adam, 1, None, e, beta, 1, s),
            "dev": lambda: L.dq_adamw_clip_ema_step_dev(o, N.ptr(a), o2, o2, 64, scp, 1.0, 10.0, N.ptr(lr_dev), *adam, N.ptr(step_dev), None,
                                                        e, beta, 1, s),
        }.items():
            rc = fn()
            torch.cuda.synchronize()
            assert rc != 0 and L.dq_last_error(), (what, name)
            assert out.all_nan() and out2.all_nan() and out3.all_nan() and sc.all_nan(), (what, name)
            assert out.intact() and out2.intact() and out3.intact() and sc.intact() and int(step_dev) == 0, (what, name)
