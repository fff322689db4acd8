"""The guided forms of the three update kernels through ``dq_guided_update``: every update kind x both objectives x
w in {0, 1, 3} at B = 3, in the vector form (per_window = 8), the one-element form (per_window = 5) and the one-element form forced by an
x_prev that sits 4 bytes behind a 16-byte aligned address (per_window = 8), each on a middle row and on the last row of its table.

Reference: float64 over the SAME fp32 inputs and coefficients, g = u + w (c - u) and then the update as tests/test_stream_kernels.py,
tests/test_stochastic_sampler.py and tests/test_solver_sampler.py restate it.  Tolerance: theirs for the same update, K 2^-24 sum |terms|,
times (1 + 2 w) -- the fp32 g differs from the float64 one by at most 2^-24 (w |c - u| + |g|) <= (1 + 2 w) 2^-24 max(|c|, |u|) (the
rounding of c - u, scaled by w, and the rounding of the multiply-add), i.e. by (1 + 2 w) times the rounding error of an operand of that
size -- with the network-output term of every magnitude taken at V = max(|c|, |u|, |g|), the size of those operands (c == u: |c|, the
unguided bound).  The numbers:
  DDIM        K = 10 (eps objective), 11 (x0 objective), 7 (the derived eps), capped at 1e-6 max |ref|  -> x1, x3, x7 for w = 0, 1, 3
  STOCHASTIC  K = 4 * 3.54 = 14.16, plus sigma * 4 * 8.59e-07 for the normal (not scaled: the noise does not pass through g)
  SOLVER_*    K = 4 * 3.78 = 15.12; an x0 within that bound of +-clip may be clamped either way (the slack of test_solver_sampler.py)
so e.g. the solver's x_prev at w = 3 is held to 105.84 * 2^-24 sum |terms|.  The noise of the stochastic reference is dq_randn's own
output for the windows' ids at that draw, so a wrong key, draw or element index shows as an error of the size of sigma."""
import ctypes

import numpy as np
import pytest
import torch

from test_sampler_tables import alpha_bars, sampler_table, timesteps
from test_solver_sampler import K_SOLVER
from test_stochastic_sampler import K_STEP, SEED, TOL_Z, _coef_table, _dev_ids, _dev_seed
from test_stream_kernels import CAP_DDIM, K_DDIM, K_DDIM_EPS, K_DDIM_X0

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B = 3
IDS = [7, 2 ** 33 + 1, 0]
DRAW = 3
CLIP = 1.0
KINDS = ("ddim", "stochastic", "solver_1", "solver_2m")


def rows(kind):
    """{name: 5 floats} -- a middle row and the last row of the kind's table, in the layout of its stand-alone entry"""
    ab = alpha_bars("cosine")
    if kind in ("ddim", "stochastic"):
        eta = 1.0 if kind == "stochastic" else 0.0
        _, cf, sg = _coef_table(ab, [500, 0], eta)
        out = {"mid": list(cf[0]) + [sg[0]], "last": list(cf[1]) + [sg[1]]}
        assert out["last"][2] < 0 and (kind == "ddim" or out["mid"][4] > 0)
        return out
    _, c4, e4 = sampler_table(ab, timesteps(1000, 4), "dpmpp_2m")
    if kind == "solver_1":
        out = {"mid": list(c4[1]) + [0.0], "last": list(c4[3]) + [0.0]}
    else:
        out = {"mid": list(c4[1]) + [e4[1]], "last": list(c4[3]) + [e4[3]]}
        assert out["mid"][4] < 0
    assert out["last"][2] == -1
    return out


def f64(kind, pred, x, c, u, w, row, h, z):
    """the float64 restatement; returns dict(xp, x0, ep, bxp, bx0, bep, near): values, their bounds (already times 1 + 2 w) and the elements
    whose clamp decision is within the bound of +-clip"""
    x, c, u = (v.astype(np.float64) for v in (x, c, u))
    g = u + w * (c - u)
    V = np.maximum(np.maximum(np.abs(c), np.abs(u)), np.abs(g))
    s = 1.0 + 2.0 * w
    r = [float(v) for v in row]
    sa, sb = r[0], r[1]
    near = np.zeros(x.shape, dtype=bool)
    if pred == "x0":
        x0, m0 = g, V
    else:
        x0, m0 = (x - sb * g) / sa, (np.abs(x) + sb * V) / sa
    x0u = x0
    solver = kind.startswith("solver")
    K0 = K_SOLVER if solver else K_STEP if kind == "stochastic" else 1.0  # (DDIM's x0 is compared only through x_prev)
    bx0 = s * K0 * U * m0
    if solver:
        x0 = np.clip(x0u, -CLIP, CLIP)
        near = np.abs(np.abs(x0u) - CLIP) <= bx0
    clamped = x0 != x0u
    mx0 = np.where(clamped, np.abs(x0), np.maximum(m0, np.abs(x0)))  # (a clamped x0 is exactly +-clip)
    ep = (x - sa * x0) / sb
    me = (np.abs(x) + sa * mx0) / sb  # the derived eps
    if pred == "eps":  # the guided network output itself unless the element was clamped
        ep = np.where(clamped, ep, g)
        me = np.where(clamped, me, V)
    if kind == "ddim":
        sap, sbp = r[2], r[3]
        K = K_DDIM_X0 if pred == "x0" else K_DDIM
        if sap < 0:
            xp, mag = x0, m0
        else:
            xp, mag = sap * x0 + sbp * ep, sap * m0 + sbp * me
        bxp = np.minimum(s * K * U * mag, s * CAP_DDIM * np.abs(xp).max())
        bep = np.minimum(s * K_DDIM_EPS * U * me, s * CAP_DDIM * np.abs(ep).max())
    elif kind == "stochastic":
        sap, cc, sg = r[2], r[3], r[4]
        if sap < 0:
            xp, bxp = x0, s * K_STEP * U * m0
        else:
            xp = sap * x0 + cc * ep + sg * z
            bxp = s * K_STEP * U * (np.abs(sap) * m0 + np.abs(cc) * me + np.abs(sg * z)) + sg * TOL_Z
        bep = s * K_STEP * U * me
    else:
        cx, c0, c1 = r[2], r[3], r[4]
        if cx < 0:
            xp, mag, c0 = x0, mx0, 1.0
        else:
            xp, mag = cx * x + c0 * x0, np.abs(cx * x) + np.abs(c0) * mx0
            if c1 != 0:
                xp, mag = xp + c1 * h.astype(np.float64), mag + np.abs(c1 * h)
        bxp = s * K_SOLVER * U * mag + np.where(near, np.abs(c0) * bx0, 0.0)
        bep = s * K_SOLVER * U * me
    return dict(xp=xp, x0=x0, x0u=x0u, ep=ep, bxp=bxp, bx0=bx0, bep=bep, near=near, clamped=clamped)


class Run:
    """one dq_guided_update call on device copies; x_prev sits `offset` floats behind a 16-byte aligned address between canaries"""

    def __init__(self, kind, pred, x, c, u, w, row, h=None, ids=IDS, alias_u=False, in_place=False, mirror=True, offset=0, want_eps=True,
                 draw=DRAW):
        from dquartic import _native as N

        nb, per = x.shape
        n = x.numel()
        xd, cd = x.cuda(), c.cuda()
        ud = cd if alias_u else u.cuda()
        hd = None if h is None else h.cuda()
        coef = torch.tensor([float(r) for r in row], dtype=torch.float32).cuda()
        buf = torch.full((n + 8,), 12345.0, device="cuda")
        md = torch.full((n + 8,), 12345.0, device="cuda") if mirror else None
        ed = torch.empty(n, device="cuda") if want_eps else None
        assert all(t.data_ptr() % 16 == 0 for t in (xd, cd, ud, buf) + (() if hd is None else (hd,)))
        out_ptr = xd.data_ptr() if in_place else buf.data_ptr() + 4 * offset
        ids_d, seed_d = _dev_ids(list(ids)), _dev_seed(SEED)
        N.check(N.lib().dq_guided_update(N.UPDATE_KINDS[kind], N.ptr(xd), N.ptr(cd), N.ptr(ud), ctypes.c_void_p(out_ptr),
                                         None if md is None else ctypes.c_void_p(md.data_ptr() + 4 * offset), N.ptr(hd), N.ptr(ed), N.ptr(coef),
                                         ctypes.c_float(w), ctypes.c_float(CLIP if kind.startswith("solver") else 0.0), N.ptr(ids_d), N.ptr(seed_d),
                                         draw, N.PRED_TYPES[pred], nb, per, N.stream_ptr()), "dq_guided_update")

        def between(b):
            b = b.cpu()
            assert (b[:offset] == 12345.0).all() and (b[offset + n:] == 12345.0).all()
            return b[offset:offset + n].reshape(nb, per).numpy()

        self.xp = xd.cpu().numpy() if in_place else between(buf)
        self.mirror = None if md is None else between(md)
        self.hist = None if hd is None else hd.cpu().numpy()
        self.eps = None if ed is None else ed.cpu().numpy().reshape(nb, per)


def unguided(kind, pred, x, c, row, h, per_pad=None):
    """the stand-alone entry of the kind on (x, c): x_prev, hist, eps (None where the entry writes none)"""
    from dquartic import _native as N

    L = N.lib()
    nb, per = x.shape
    if kind == "stochastic" and per % 4:  # that entry wants per_window % 4 == 0: pad the windows (element e of a window keeps its noise)
        pad = lambda t: torch.cat([t, torch.zeros(nb, 8 - per)], dim=1).contiguous()
        xp, hh, ep = unguided(kind, pred, pad(x), pad(c), row, h)
        return xp[:, :per], hh, None if ep is None else ep[:, :per]
    xd, cd = x.cuda(), c.cuda()
    out, eo = torch.empty_like(xd), torch.empty_like(xd)
    hd = None if h is None else h.cuda()
    coef = torch.tensor([float(r) for r in row], dtype=torch.float32).cuda()
    ids_d, seed_d = _dev_ids(IDS), _dev_seed(SEED)
    s = N.stream_ptr()
    if kind == "ddim" and pred == "eps":
        N.check(L.dq_ddim_step(N.ptr(xd), N.ptr(cd), N.ptr(out), N.ptr(coef), x.numel(), s), "dq_ddim_step")
        return out.cpu().numpy(), None, None
    if kind == "ddim":
        N.check(L.dq_ddim_step_x0(N.ptr(xd), N.ptr(cd), N.ptr(out), N.ptr(eo), N.ptr(coef), x.numel(), s), "dq_ddim_step_x0")
        return out.cpu().numpy(), None, eo.cpu().numpy()
    if kind == "stochastic":
        N.check(L.dq_ddim_step_sto(N.ptr(xd), N.ptr(cd), N.ptr(out), N.ptr(eo) if pred == "x0" else None, N.ptr(coef), N.ptr(ids_d), N.ptr(seed_d),
                                   DRAW, N.PRED_TYPES[pred], nb, per, s), "dq_ddim_step_sto")
        return out.cpu().numpy(), None, (eo.cpu().numpy() if pred == "x0" else None)
    N.check(L.dq_solver_step(N.ptr(xd), N.ptr(cd), N.ptr(out), N.ptr(hd), N.ptr(eo), N.ptr(coef), ctypes.c_float(CLIP), N.PRED_TYPES[pred],
                             x.numel(), s), "dq_solver_step")
    return out.cpu().numpy(), (None if hd is None else hd.cpu().numpy()), eo.cpu().numpy()


def randn_of(ids, per, draw=DRAW):
    from dquartic import _native as N

    out = torch.empty(len(ids), per, device="cuda")
    ids_d, seed_d = _dev_ids(list(ids)), _dev_seed(SEED)
    N.check(N.lib().dq_randn(N.ptr(out), N.ptr(ids_d), N.ptr(seed_d), draw, len(ids), per, N.stream_ptr()), "dq_randn")
    return out.cpu().numpy().astype(np.float64)


def inputs(pred, per, seed):
    g = torch.Generator().manual_seed(seed)
    x, c, d, h = (torch.randn(B, per, generator=g) for _ in range(4))
    if pred == "x0":
        c = 1.2 * c  # an x0 prediction that exceeds a clamp of 1 on some elements and stays inside on others
    return x, c, (c + 0.5 * d).contiguous(), h


@pytest.mark.parametrize("w", [0.0, 1.0, 3.0])
@pytest.mark.parametrize("pred", ["eps", "x0"])
@pytest.mark.parametrize("kind", KINDS)
def test_guided_update(kind, pred, w):
    table = rows(kind)
    solver = kind.startswith("solver")
    worst = {}
    engaged = left = 0
    for per, offset in ((8, 0), (5, 0), (8, 1)):  # the vector form, the one-element form, the one-element form by alignment
        x, c, u, h = inputs(pred, per, 100 * per + offset)
        z = randn_of(IDS, per) if kind == "stochastic" else None
        for name, row in table.items():
            uses_h = kind == "solver_2m"
            h_in = h if uses_h else None
            r = Run(kind, pred, x, c, u, w, row, h=h_in, offset=offset)
            ref = f64(kind, pred, x.numpy(), c.numpy(), u.numpy(), w, row, h.numpy(), z)
            tag = (per, offset, name)
            assert np.isfinite(r.xp).all(), tag
            e = np.abs(r.xp.astype(np.float64) - ref["xp"])
            worst["xp"] = max(worst.get("xp", 0.0), float((e / ref["bxp"]).max()))
            assert (e <= ref["bxp"]).all(), (tag, float((e / ref["bxp"]).max()))
            # eps_out sees the guided quantities, under either objective
            ee = np.abs(r.eps.astype(np.float64) - ref["ep"])
            sel = ~ref["near"]
            worst["eps"] = max(worst.get("eps", 0.0), float((ee[sel] / ref["bep"][sel]).max()))
            assert (ee[sel] <= ref["bep"][sel]).all(), (tag, float((ee[sel] / ref["bep"][sel]).max()))
            # the mirror is x_prev, bit for bit; a NULL mirror, no eps_out and x_prev in x_t's place change nothing
            assert np.array_equal(r.mirror, r.xp), tag
            for kw in (dict(mirror=False), dict(want_eps=False), dict(in_place=True)):
                if kw.get("in_place") and offset:
                    continue  # (x_t itself is aligned: that is the vector form again, covered at offset 0)
                q = Run(kind, pred, x, c, u, w, row, h=h_in, offset=offset, **kw)
                assert np.array_equal(q.xp, r.xp), (tag, kw)
                assert q.hist is None or np.array_equal(q.hist, r.hist), (tag, kw)
            if offset:  # the one-element form on the vector form's inputs: the same expressions, the same bits
                v = Run(kind, pred, x, c, u, w, row, h=h_in)
                assert np.array_equal(v.xp, r.xp) and np.array_equal(v.eps, r.eps), tag
            if uses_h:
                # the history is written from the guided, clamped x0: +-clip exactly where float64 clamps, within the bound elsewhere
                eh = np.abs(r.hist.astype(np.float64) - ref["x0"])
                assert (eh <= np.where(ref["near"], 2 * ref["bx0"], np.where(ref["clamped"], 0.0, ref["bx0"]))).all(), tag
                assert (np.abs(r.hist) <= CLIP).all()
                if name == "last":
                    assert np.array_equal(r.xp, r.hist), tag  # the last row (cx < 0) returns x0
            if solver:
                engaged += int((ref["clamped"] & ~ref["near"]).sum())
                left += int((~ref["clamped"] & ~ref["near"]).sum())
            if name == "last":  # every kind's last row returns its x0
                assert (np.abs(r.xp.astype(np.float64) - ref["x0"]) <= ref["bxp"]).all(), tag
            # net_u aliased to net_c: c - u is exactly 0, every output is the unguided stand-alone entry's, bit for bit
            a = Run(kind, pred, x, c, u, w, row, h=h_in, offset=offset, alias_u=True)
            xp0, h0, e0 = unguided(kind, pred, x, c, row, h_in)
            assert np.array_equal(a.xp, xp0) and np.array_equal(a.mirror, xp0), tag
            assert h0 is None or np.array_equal(a.hist, h0), tag
            if e0 is not None:
                assert np.array_equal(a.eps, e0), tag
            elif pred == "eps":
                assert np.array_equal(a.eps, c.numpy()), tag  # (entries that write no eps under this objective: it is the network output)
    if solver:  # the clamp engaged on some elements and left others alone (on the float64 side)
        assert engaged > 0 and left > 0, (engaged, left)
    print("dq_guided_update[%s, %s, w=%g]: worst error / bound:" % (kind, pred, w), worst)


@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_stochastic_noise_is_keyed_by_the_window(pred):
    """window b's noise is dq_randn's for its id at that draw: under other ids, at another draw, at another batch position and alone"""
    row = rows("stochastic")["mid"]
    for per in (8, 5):
        x, c, u, h = inputs(pred, per, 7 + per)
        full = Run("stochastic", pred, x, c, u, 3.0, row)
        for ids, draw in (([5, 9, 2 ** 40 + 3], DRAW), (IDS, DRAW + 1)):
            r = Run("stochastic", pred, x, c, u, 3.0, row, ids=ids, draw=draw)
            ref = f64("stochastic", pred, x.numpy(), c.numpy(), u.numpy(), 3.0, row, None, randn_of(ids, per, draw))
            assert (np.abs(r.xp.astype(np.float64) - ref["xp"]) <= ref["bxp"]).all(), (per, ids, draw)
            assert not np.array_equal(r.xp, full.xp)
            assert np.array_equal(r.eps, full.eps)  # (the eps does not depend on the noise)
        for b in range(B):  # a batch of one, under its id: the window's result in the batch, bit for bit
            one = Run("stochastic", pred, x[b:b + 1].contiguous(), c[b:b + 1].contiguous(), u[b:b + 1].contiguous(), 3.0, row, ids=IDS[b:b + 1])
            assert np.array_equal(one.xp, full.xp[b:b + 1]) and np.array_equal(one.mirror, full.mirror[b:b + 1]), (per, b)
        # NULL ids are 0 .. B-1
        from dquartic import _native as N

        xd, cd, ud, out = x.cuda(), c.cuda(), u.cuda(), torch.empty(B, per, device="cuda")
        coef, seed_d = torch.tensor([float(v) for v in row]).cuda(), _dev_seed(SEED)
        N.check(N.lib().dq_guided_update(N.UPDATE_KINDS["stochastic"], N.ptr(xd), N.ptr(cd), N.ptr(ud), N.ptr(out), None, None, None, N.ptr(coef),
                                         ctypes.c_float(3.0), ctypes.c_float(0.0), None, N.ptr(seed_d), DRAW, N.PRED_TYPES[pred], B, per,
                                         N.stream_ptr()), "dq_guided_update")
        assert np.array_equal(out.cpu().numpy(), Run("stochastic", pred, x, c, u, 3.0, row, ids=[0, 1, 2]).xp)
