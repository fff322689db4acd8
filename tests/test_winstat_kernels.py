"""The per-window statistics kernels and the per-window form of the update (csrc/k_winstat.hip, k_update.hip).

Quantile: ``dq_window_abs_quantile`` BIT FOR BIT against tests/test_winstat_host.py's transcription of the rule, at B in {1, 3} x
per_window in {1, 2, 5, 8, 260, 8452, 8453} (the last two: past one chunk of 8192 elements and past a block stride of 256 inside the second
chunk, as a multiple of 4 and not) x q in {1e-3, 0.5, 0.995, 1} x seven kinds of input; the input, the output and the scratch lie
between canaries that stay; a window alone gives the bits it gives as row 1 of 3.

Rescale: ``dq_window_rescale`` against float64 over the same fp32 inputs, held to
    |m - m64| <= 1.01 * 2^-24 * (m64 + phi (sigma_c / sigma_g) rms(w |c - u| + |g|) / sigma_g)
(one rounding of the result, plus the fp32 rounding of g carried through a 1-Lipschitz standard deviation); a constant-g window gives
m = 1 exactly; windows alone and in a batch give the same bits.

Update: ``dq_step_update_adaptive`` with the table computed in float64 (rounded to the fp32 the kernel reads) against the float64
restatements of tests/test_guided_update.py and tests/test_v_update.py -- the rescale enters them as c, u scaled by m_b in float64, so
every network-output magnitude and with it every bound carries the factor m_b; the thresholded solver step is restated here in their
pattern, K and (1 + 2 w) theirs, with one rounding more per multiply the per-window form adds under the v objective's counted K (m_b g,
x0 rho_b).  With table rows (1, f, 1) every form equals today's guided or clamped update bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from test_guided_update import B, CLIP, DRAW, IDS, KINDS, SEED, U, f64, inputs, randn_of, rows
from test_solver_sampler import K_SOLVER
from test_stochastic_sampler import _dev_ids, _dev_seed
from test_v_update import K_V0, K_V_SOLVER, f64_v
from test_winstat_host import abs_quantile_ref, stat_scratch_bytes

pytestmark = pytest.mark.gpu

PERS = (1, 2, 5, 8, 260, 8452, 8453)
QS = (1e-3, 0.5, 0.995, 1.0)
PREDS = ("eps", "x0", "v_prediction")


class Scratch:
    """the statistics scratch between canaries: 0xA5 bytes in front of and behind the bytes the size rule names"""

    def __init__(self, nb, per):
        from dquartic import _native as N

        self.n = N.lib().dq_sample_stat_scratch_bytes(nb, per)
        assert self.n == stat_scratch_bytes(nb, per)
        self.buf = torch.full((self.n + 512,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 256)

    def check(self):
        b = self.buf.cpu()
        assert (b[:256] == 0xA5).all() and (b[256 + self.n:] == 0xA5).all()


def between_nans(a):
    """a (numpy float32) on the device with 8 NaNs on either side: (buffer, view)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.full((t.numel() + 16,), float("nan"))
    buf[8:8 + t.numel()] = t
    buf = buf.cuda()
    return buf, buf[8:8 + t.numel()]


def nans_stay(buf, n):
    b = buf.cpu()
    assert torch.isnan(b[:8]).all() and torch.isnan(b[8 + n:]).all()


def quantile_dev(x, q):
    """dq_window_abs_quantile on x (nb, per): the nb float32 results"""
    from dquartic import _native as N

    nb, per = x.shape
    xb, xv = between_nans(x)
    ob, ov = between_nans(np.zeros(nb, dtype=np.float32))
    sc = Scratch(nb, per)
    N.check(N.lib().dq_window_abs_quantile(ctypes.c_void_p(xv.data_ptr()), nb, per, ctypes.c_float(q), ctypes.c_void_p(ov.data_ptr()), sc.ptr, sc.n,
                                           N.stream_ptr()), "dq_window_abs_quantile")
    out = ov.cpu().numpy().copy()
    nans_stay(xb, x.size), nans_stay(ob, nb), sc.check()
    assert np.array_equal(xv.cpu().numpy().view(np.uint32), x.reshape(-1).view(np.uint32))  # the input is read only
    return out


def make(kind, nb, per, rng):
    sign = np.where(rng.random((nb, per)) < 0.5, -1.0, 1.0).astype(np.float32)
    if kind == "normal":
        return (3.0 * rng.standard_normal((nb, per))).astype(np.float32)
    if kind == "equal":
        return np.float32(1.25) * sign
    if kind == "zeros":  # half zeros, -0.0 among them
        x = rng.standard_normal((nb, per)).astype(np.float32)
        z = rng.random((nb, per)) < 0.5
        x[z] = 0.0
        return x * sign
    if kind == "denormal":
        return rng.integers(1, 2 ** 23, (nb, per), dtype=np.uint32).view(np.float32) * sign
    if kind == "low8":  # values that differ only in their lowest 8 bits: the select is decided in its last pass
        return (np.uint32(0x3F9E3700) | rng.integers(0, 256, (nb, per), dtype=np.uint32)).view(np.float32) * sign
    if kind == "huge":
        return (rng.standard_normal((nb, per)) * 10.0 ** rng.uniform(-30, 30, (nb, per))).astype(np.float32).clip(-1e30, 1e30)
    assert kind == "ties"  # a handful of distinct values: the selected rank sits inside a run of equal ones
    return rng.integers(0, 4, (nb, per)).astype(np.float32) * np.float32(0.37) * sign


@pytest.mark.parametrize("kind", ["normal", "equal", "zeros", "denormal", "low8", "huge", "ties"])
def test_abs_quantile_bit_for_bit(kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    for per in PERS:
        x = make(kind, 3, per, rng)
        if kind == "zeros":
            assert per < 8 or (np.signbit(x) & (x == 0)).any()
        for q in QS:
            ref = np.array([abs_quantile_ref(x[b], q) for b in range(3)], dtype=np.float32)
            got = quantile_dev(x, q)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (kind, per, q, got, ref)
            one = quantile_dev(x[1:2].copy(), q)  # B = 1: the window alone is row 1 of 3, bit for bit
            assert one.view(np.uint32)[0] == got.view(np.uint32)[1], (kind, per, q)


def rescale_dev(c, u, w, phi):
    from dquartic import _native as N

    nb, per = c.shape
    cb, cv = between_nans(c)
    ub, uv = between_nans(u)
    ob, ov = between_nans(np.zeros(nb, dtype=np.float32))
    sc = Scratch(nb, per)
    N.check(N.lib().dq_window_rescale(ctypes.c_void_p(cv.data_ptr()), ctypes.c_void_p(uv.data_ptr()), ctypes.c_float(w), ctypes.c_double(phi), nb, per,
                                      ctypes.c_void_p(ov.data_ptr()), sc.ptr, sc.n, N.stream_ptr()), "dq_window_rescale")
    out = ov.cpu().numpy().copy()
    nans_stay(cb, c.size), nans_stay(ub, u.size), nans_stay(ob, nb), sc.check()
    return out


def rescale_f64(c, u, w, phi):
    """(m64, bound) per window"""
    c, u = c.astype(np.float64), u.astype(np.float64)
    g = u + w * (c - u)
    sc, sg = c.std(axis=1), g.std(axis=1)
    m = phi * sc / sg + (1.0 - phi)
    rms = np.sqrt(((w * np.abs(c - u) + np.abs(g)) ** 2).mean(axis=1))
    return m, 1.01 * U * (m + phi * (sc / sg) * rms / sg)


@pytest.mark.parametrize("w", [0.0, 3.0, 7.5])
def test_rescale_vs_float64(w):
    worst = 0.0
    for per in (5, 260, 8453, 25600):
        rng = np.random.default_rng(int(10 * w) + per)
        c, u = (rng.standard_normal((3, per)).astype(np.float32) for _ in range(2))
        for phi in (0.7, 1.0):
            m64, bound = rescale_f64(c, u, w, phi)
            m = rescale_dev(c, u, w, phi)
            frac = np.abs(m.astype(np.float64) - m64) / bound
            print("dq_window_rescale[w=%g, per=%d, phi=%g]: error / bound" % (w, per, phi), frac)
            worst = max(worst, float(frac.max()))
            assert (frac <= 1.0).all(), (w, per, phi, frac)
            for b in range(3):  # alone: the same bits
                one = rescale_dev(c[b:b + 1].copy(), u[b:b + 1].copy(), w, phi)
                assert one.view(np.uint32)[0] == m.view(np.uint32)[b], (w, per, phi, b)
        assert np.array_equal(rescale_dev(c, u, w, 0.0), np.ones(3, dtype=np.float32))  # phi = 0: (float)(0 * r + 1)
    print("dq_window_rescale[w=%g]: worst error / bound %.3f" % (w, worst))


def test_rescale_of_a_constant_g_is_one():
    rng = np.random.default_rng(5)
    for per in (5, 8453):
        c, u = (rng.standard_normal((3, per)).astype(np.float32) for _ in range(2))
        u[1] = c[1] = np.float32(0.3)  # window 1: c == u == a constant, g constant at every w
        m = rescale_dev(c, u, 3.0, 0.7)
        assert m[1] == 1.0 and m[0] != 1.0
        uc = np.full((3, per), np.float32(-0.7))  # w = 0: g = u, a constant, whatever c is
        assert np.array_equal(rescale_dev(c, uc, 0.0, 1.0)[[0, 2]], np.ones(2, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- the update
class RunA:
    """one dq_step_update_adaptive call on device copies (u None: the unguided form); x_prev and the mirror between canaries"""

    def __init__(self, kind, pred, x, c, u, w, row, tab, h=None, ids=IDS):
        from dquartic import _native as N

        nb, per = x.shape
        n = x.numel()
        xd, cd = x.cuda(), c.cuda()
        ud = None if u is None else u.cuda()
        hd = None if h is None else h.clone().cuda()
        coef = torch.tensor([float(r) for r in row], dtype=torch.float32).cuda()
        td = torch.tensor(np.asarray(tab, dtype=np.float32)).reshape(nb, 4).contiguous().cuda()
        buf = torch.full((n + 8,), 12345.0, device="cuda")
        md = torch.full((n + 8,), 12345.0, device="cuda")
        ed = torch.empty(n, device="cuda")
        ids_d, seed_d = _dev_ids(list(ids)), _dev_seed(SEED)
        N.check(N.lib().dq_step_update_adaptive(N.UPDATE_KINDS[kind], N.ptr(xd), N.ptr(cd), N.ptr(ud), N.ptr(buf), N.ptr(md), N.ptr(hd), N.ptr(ed),
                                                N.ptr(coef), ctypes.c_float(w), N.ptr(td), N.ptr(ids_d), N.ptr(seed_d), DRAW, N.PRED_TYPES[pred], nb,
                                                per, N.stream_ptr()), "dq_step_update_adaptive")
        assert (buf[n:] == 12345.0).all() and (md[n:] == 12345.0).all()
        self.xp = buf[:n].cpu().numpy().reshape(nb, per)
        self.mirror = md[:n].cpu().numpy().reshape(nb, per) if u is not None else None
        self.hist = None if hd is None else hd.cpu().numpy()
        self.eps = ed.cpu().numpy().reshape(nb, per)


def today(kind, pred, x, c, u, w, row, h, clip):
    """today's entries on the same operands: dq_guided_update(_v), or (u None) dq_solver_step(_v): x_prev, hist, eps"""
    from dquartic import _native as N

    L = N.lib()
    nb, per = x.shape
    xd, cd = x.cuda(), c.cuda()
    hd = None if h is None else h.clone().cuda()
    coef = torch.tensor([float(r) for r in row], dtype=torch.float32).cuda()
    out, eo = torch.empty_like(xd), torch.empty_like(xd)
    f = ctypes.c_float
    if u is None:
        if pred == "v_prediction":
            N.check(L.dq_solver_step_v(N.ptr(xd), N.ptr(cd), N.ptr(out), N.ptr(hd), N.ptr(eo), N.ptr(coef), f(clip), x.numel(), N.stream_ptr()), "solver_v")
        else:
            N.check(L.dq_solver_step(N.ptr(xd), N.ptr(cd), N.ptr(out), N.ptr(hd), N.ptr(eo), N.ptr(coef), f(clip), N.PRED_TYPES[pred], x.numel(),
                                     N.stream_ptr()), "solver")
    else:
        ud = u.cuda()
        ids_d, seed_d = _dev_ids(list(IDS)), _dev_seed(SEED)
        head = (N.UPDATE_KINDS[kind], N.ptr(xd), N.ptr(cd), N.ptr(ud), N.ptr(out), None, N.ptr(hd), N.ptr(eo), N.ptr(coef), f(w), f(clip), N.ptr(ids_d),
                N.ptr(seed_d), DRAW)
        if pred == "v_prediction":
            N.check(L.dq_guided_update_v(*head, nb, per, N.stream_ptr()), "guided_v")
        else:
            N.check(L.dq_guided_update(*head, N.PRED_TYPES[pred], nb, per, N.stream_ptr()), "guided")
    return out.cpu().numpy(), (None if hd is None else hd.cpu().numpy()), eo.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("w", [1.0, 3.0])
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("kind", KINDS)
def test_neutral_table_is_todays_update_bit_for_bit(kind, pred, w):
    solver = kind.startswith("solver")
    for per in (8, 5):
        x, c, u, h = inputs("x0" if pred == "x0" else "eps", per, 300 + per)
        for name, row in rows(kind).items():
            h_in = h if kind == "solver_2m" else None
            for clip, s in ((CLIP, CLIP), (0.0, np.inf)) if solver else ((0.0, np.inf),):
                tab = np.tile(np.array([1.0, s, 1.0, 0.0], dtype=np.float32), (B, 1))
                r = RunA(kind, pred, x, c, u, w, row, tab, h=h_in)
                xp, hh, ep = today(kind, pred, x, c, u, w, row, h_in, clip)
                tag = (per, name, clip)
                assert same_bits(r.xp, xp) and same_bits(r.mirror, xp) and same_bits(r.eps, ep), tag
                assert hh is None or same_bits(r.hist, hh), tag
                if solver:  # the unguided form
                    r1 = RunA(kind, pred, x, c, None, 1.0, row, tab, h=h_in)
                    xp1, hh1, ep1 = today(kind, pred, x, c, None, 1.0, row, h_in, clip)
                    assert same_bits(r1.xp, xp1) and same_bits(r1.eps, ep1) and (hh1 is None or same_bits(r1.hist, hh1)), tag


def table_f64(pred, x, c, u, w, row, phi, q, f, cap):
    """the (B, 4) table of steps 2 and 4 in float64 from the fp32 operands, rounded to the fp32 the kernel reads; thresholding with q"""
    x, c, u = (v.numpy().astype(np.float64) for v in (x, c, u))
    g = u + w * (c - u)
    m = np.float32(phi * c.std(axis=1) / g.std(axis=1) + (1.0 - phi)) if phi else np.ones(x.shape[0], dtype=np.float32)
    g = m.astype(np.float64)[:, None] * g
    sa, sb = float(row[0]), float(row[1])
    x0 = g if pred == "x0" else sa * x - sb * g if pred == "v_prediction" else (x - sb * g) / sa
    if q is None:
        s = np.full(x.shape[0], f, dtype=np.float32)
    else:
        s = np.minimum(np.maximum(np.float32(np.quantile(np.abs(x0), q, axis=1)), np.float32(f)), np.float32(cap))
    rho = np.float32(f) / s  # (fp32, correctly rounded)
    return np.stack([m, s, rho.astype(np.float32), np.zeros_like(m)], axis=1).astype(np.float32)


def f64_threshold(pred, x, c, u, w, row, h, tab):
    """the solver step with steps 2 and 4, restated in float64 over the fp32 operands and table; the pattern of test_guided_update.f64"""
    x, c, u = (v.astype(np.float64) for v in (x, c, u))
    m, s_, rho = (tab[:, k].astype(np.float64)[:, None] for k in range(3))
    g0 = u + w * (c - u)
    g = m * g0
    V = np.maximum(np.maximum(np.abs(c), np.abs(u)), np.abs(g0)) * np.maximum(1.0, m)
    v_obj = pred == "v_prediction"
    sf = (1.0 + 2.0 * w) * np.maximum(1.0, m)
    K0, K = (K_V0 + 2.0, K_V_SOLVER + 2.0) if v_obj else (K_SOLVER, K_SOLVER)  # (v: the counted K plus the two multiplies this form adds)
    r = [float(v) for v in row]
    sa, sb = r[0], r[1]
    if pred == "x0":
        x0u, m0 = g, V
    elif v_obj:
        x0u, m0 = sa * x - sb * g, sa * np.abs(x) + sb * V
    else:
        x0u, m0 = (x - sb * g) / sa, (np.abs(x) + sb * V) / sa
    bx0 = sf * K0 * U * m0
    x0c = np.clip(x0u, -s_, s_)
    near = np.abs(np.abs(x0u) - s_) <= bx0
    x0 = x0c * rho
    changed = (x0c != x0u) | (rho != 1.0)
    mx0 = np.maximum(m0, np.abs(x0))
    ep, me = (x - sa * x0) / sb, (np.abs(x) + sa * mx0) / sb
    if pred == "eps":
        ep, me = np.where(changed, ep, g), np.where(changed, me, V)
    elif v_obj:
        ep, me = np.where(changed, ep, sb * x + sa * g), np.where(changed, me, sb * np.abs(x) + sa * V)
    cx, c0, c1 = r[2], r[3], r[4]
    if cx < 0:
        xp, mag, c0 = x0, mx0, 1.0
    else:
        xp, mag = cx * x + c0 * x0, np.abs(cx * x) + np.abs(c0) * mx0
        if c1 != 0:
            xp, mag = xp + c1 * h.astype(np.float64), mag + np.abs(c1 * h)
    return dict(xp=xp, x0=x0, ep=ep, bxp=sf * K * U * mag + np.where(near, np.abs(c0) * bx0, 0.0), bx0=bx0 + U * np.abs(x0), bep=sf * K * U * me,
                near=near, s=s_, rho=rho)


@pytest.mark.parametrize("w", [1.0, 3.0])
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_update_vs_float64(kind, pred, w):
    solver = kind.startswith("solver")
    worst, above, scaled = {}, 0, 0
    for per in (8, 5):
        x, c, u, h = inputs("x0" if pred == "x0" else "eps", per, 500 + per)
        z = randn_of(IDS, per) if kind == "stochastic" else None
        for name, row in rows(kind).items():
            h_in = h if kind == "solver_2m" else None
            for phi, q in ((0.7, None), (0.0, 0.6), (0.7, 0.6)) if solver else ((0.7, None),):
                tab = table_f64(pred, x, c, u, w, row, phi, q, CLIP, 3.0)
                r = RunA(kind, pred, x, c, u, w, row, tab, h=h_in)
                m = tab[:, 0].astype(np.float64)[:, None]
                if solver:
                    ref = f64_threshold(pred, x.numpy(), c.numpy(), u.numpy(), w, row, h.numpy(), tab)
                    above += int((tab[:, 1] > CLIP).sum())
                    scaled += int((tab[:, 2] < 1.0).sum())
                elif pred == "v_prediction":  # the rescale as c, u scaled in float64; one rounding more (m g) under the counted K
                    ref = f64_v(kind, x.numpy(), c.numpy() * m, u.numpy() * m, w, row, h.numpy(), z, extra=1.0)
                else:
                    ref = f64(kind, pred, x.numpy(), c.numpy() * m, u.numpy() * m, w, row, h.numpy(), z)
                tag = (per, name, phi, q)
                grow = np.maximum(1.0, m) if not solver else 1.0  # (f64_threshold carries max(1, m_b) itself)
                e = np.abs(r.xp.astype(np.float64) - ref["xp"]) / (ref["bxp"] * grow)
                ee = (np.abs(r.eps.astype(np.float64) - ref["ep"]) / (ref["bep"] * grow))[~ref["near"]]
                worst["xp"], worst["eps"] = max(worst.get("xp", 0.0), float(e.max())), max(worst.get("eps", 0.0), float(ee.max()))
                assert np.isfinite(r.xp).all() and (e <= 1.0).all(), (tag, float(e.max()))
                assert (ee <= 1.0).all(), (tag, float(ee.max()))
                assert same_bits(r.mirror, r.xp), tag
                if kind == "solver_2m":  # the history is the rescaled, thresholded x0
                    eh = np.abs(r.hist.astype(np.float64) - ref["x0"])
                    assert (eh <= np.where(ref["near"], 2 * ref["bx0"], ref["bx0"])).all(), tag
                    assert (np.abs(r.hist) <= CLIP * (1 + 2 * U)).all(), tag  # s_b rho_b = f up to the rounding of rho_b
                    if name == "last":
                        assert same_bits(r.xp, r.hist), tag
    if solver:  # the threshold rose above the floor in some windows and stayed on it in others
        assert above > 0 and scaled > 0, (above, scaled)
    print("dq_step_update_adaptive[%s, %s, w=%g]: worst error / bound:" % (kind, pred, w), worst)
