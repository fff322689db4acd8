"""The update kernels under the v objective: k_step_update<family, DQ_PRED_V, GUIDED, V> through the stand-alone
entries (dq_ddim_step_v, dq_ddim_step_sto, dq_solver_step_v: w = None below) and through dq_guided_update_v at w in {0, 1, 3}, for every kind
(ddim, stochastic, solver_1, solver_2m) at B = 3 -- the pattern of tests/test_guided_update.py, whose rows, inputs and device harness are
imported: the vector form (per_window = 8), the one-element form (per_window = 5) and the one-element form forced by an x_prev 4 bytes off
16-byte alignment (per_window = 8), each on a middle row and on the last row of the kind's table; the Solver kinds clamp at clip_x0 = 1.
x_prev, eps_out and the Solver history are checked.

Reference: float64 over the SAME fp32 inputs and coefficients.  Tolerance (derived, not measured): K 2^-24 sum |terms| per output, times
(1 + 2 w) guided as tests/test_guided_update.py derives it (w = None: 1), with the network-output term at V = max(|c|, |u|, |g|).  Counting the
roundings on the longest path to an output:
  x0 = sa x - sb v, eps = sb x + sa v    two products, one sum -- a product and the sum lie on a path: 2, + 1 for the operand v itself (the
                                         rounding the (1 + 2 w) factor scales; unguided it is slack)                        K_V0 = 3
  ddim       x_prev = sap x0 + sbp eps   K_V0 | the product: 1 | the sum: 1                                                 K_V_DDIM = 5
  stochastic (sap x0 + c eps) + sigma z  K_V0 | product: 1 | sum: 1 | second sum: 1, plus sigma TOL_Z for the normal        K_V_STO = 6
  solver     (cx x + c0 x0) + c1 h       K_V0 | product: 1 | sum: 1 | second sum: 1                                         K_V_SOLVER = 6
  eps_out                                K_V0; where the Solver clamped x0, eps = (x - sa x0) / sb: product, difference, quotient: 3 = K_V0
sum |terms| is sa |x| + sb V for x0, sb |x| + sa V for eps and the update's own combination of those for x_prev.  With or without
contraction: an FMA drops a rounding, never adds one.  An x0 within its bound of +-clip may be clamped either way (the slack of
tests/test_solver_sampler.py); its eps is then not compared.

Consistency: from one float64 (x0, eps) at |x0| <= 0.8 (no clamp engages) and x_t = sa x0 + sb eps, the fp32 roundings of eps, x0 and
v = sa eps - sb x0 go through the three objectives of the same kind and row.  Each x_prev lies within its own bound of the float64 truth
sap x0 + sbp eps (+ ...), with one more rounding per term for the rounded inputs (K + 1; the eps and x0 objectives at the K of
tests/test_guided_update.py), so any two agree within the sum of their bounds.  A wrong sign or swapped sa / sb is off by O(1).

Head epilogue: the tiny network of tests/test_hip_x0.py, B = 3: one default sampling step through the fused head launch against
dq_unet_fwd's output pushed through dq_ddim_step_v (within K_V_DDIM / K_V0 of the float64 update of that output), graph == eager bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import sub
from test_guided_update import B, CLIP, DRAW, IDS, KINDS, SEED, U, inputs, randn_of, rows
from test_guided_update import Run as RunOther  # (dq_guided_update: the eps and x0 objectives)
from test_guided_update import f64 as f64_other
from test_stochastic_sampler import TOL_Z, _dev_ids, _dev_seed

pytestmark = pytest.mark.gpu

PRED = "v_prediction"
K_V0, K_V_DDIM, K_V_STO, K_V_SOLVER = 3.0, 5.0, 6.0, 6.0
WORST = {}


def f64_v(kind, x, c, u, w, row, h, z, extra=0.0):
    """the float64 restatement under the v objective; w None: unguided (u unused).  extra: roundings added to every K (the consistency test)"""
    x, c = x.astype(np.float64), c.astype(np.float64)
    if w is None:
        g, V, s = c, np.abs(c), 1.0
    else:
        u = u.astype(np.float64)
        g = u + w * (c - u)
        V, s = np.maximum(np.maximum(np.abs(c), np.abs(u)), np.abs(g)), 1.0 + 2.0 * w
    r = [float(v) for v in row]
    sa, sb = r[0], r[1]
    k0 = K_V0 + extra
    x0u, m0 = sa * x - sb * g, sa * np.abs(x) + sb * V
    ep, me = sb * x + sa * g, sb * np.abs(x) + sa * V
    bx0 = s * k0 * U * m0
    solver = kind.startswith("solver")
    x0, near = x0u, np.zeros(x.shape, dtype=bool)
    if solver:
        x0 = np.clip(x0u, -CLIP, CLIP)
        near = np.abs(np.abs(x0u) - CLIP) <= bx0
    clamped = x0 != x0u
    mx0 = np.where(clamped, np.abs(x0), m0)
    if solver:  # eps consistent with the clamped x0
        ep = np.where(clamped, (x - sa * x0) / sb, ep)
        me = np.where(clamped, (np.abs(x) + sa * np.abs(x0)) / sb, me)
    bep = s * k0 * U * me
    if kind == "ddim":
        sap, sbp = r[2], r[3]
        if sap < 0:
            xp, bxp = x0, bx0
        else:
            xp, bxp = sap * x0 + sbp * ep, s * (K_V_DDIM + extra) * U * (sap * m0 + sbp * me)
    elif kind == "stochastic":
        sap, cc, sg = r[2], r[3], r[4]
        if sap < 0:
            xp, bxp = x0, bx0
        else:
            xp = sap * x0 + cc * ep + sg * z
            bxp = s * (K_V_STO + extra) * U * (np.abs(sap) * m0 + np.abs(cc) * me + np.abs(sg * z)) + sg * TOL_Z
    else:
        cx, c0, c1 = r[2], r[3], r[4]
        if cx < 0:
            xp, bxp = x0, np.where(clamped, 0.0, bx0) + np.where(near, bx0, 0.0)
        else:
            xp, mag = cx * x + c0 * x0, np.abs(cx * x) + np.abs(c0) * mx0
            if c1 != 0:
                xp, mag = xp + c1 * h.astype(np.float64), mag + np.abs(c1 * h)
            bxp = s * (K_V_SOLVER + extra) * U * mag + np.where(near, np.abs(c0) * bx0, 0.0)
    return dict(xp=xp, x0=x0, ep=ep, bxp=bxp, bx0=bx0, bep=bep, near=near, clamped=clamped)


class Run:
    """one dq_guided_update_v call on device copies; x_prev (and the mirror) sit `offset` floats behind a 16-byte aligned address between
    canaries.  The attributes tests/test_guided_update.py::Run has: xp, mirror, hist, eps."""

    def __init__(self, kind, pred, x, c, u, w, row, h=None, alias_u=False, offset=0):
        from dquartic import _native as N

        assert pred == PRED
        nb, per = x.shape
        n = x.numel()
        xd, cd = x.cuda(), c.cuda()
        ud = cd if alias_u else u.cuda()
        hd = None if h is None else h.cuda()
        coef = torch.tensor([float(r) for r in row], dtype=torch.float32).cuda()
        buf, md = torch.full((n + 8,), 12345.0, device="cuda"), torch.full((n + 8,), 12345.0, device="cuda")
        ed = torch.full((n,), float("nan"), device="cuda")
        ids_d, seed_d = _dev_ids(IDS), _dev_seed(SEED)
        assert all(t.data_ptr() % 16 == 0 for t in (xd, cd, ud, buf, md))
        N.check(N.lib().dq_guided_update_v(N.UPDATE_KINDS[kind], N.ptr(xd), N.ptr(cd), N.ptr(ud), ctypes.c_void_p(buf.data_ptr() + 4 * offset),
                                           ctypes.c_void_p(md.data_ptr() + 4 * offset), N.ptr(hd), N.ptr(ed), N.ptr(coef), ctypes.c_float(w),
                                           ctypes.c_float(CLIP if kind.startswith("solver") else 0.0), N.ptr(ids_d), N.ptr(seed_d), DRAW, nb, per,
                                           N.stream_ptr()), "dq_guided_update_v")

        def between(t):
            t = t.cpu()
            assert (t[:offset] == 12345.0).all() and (t[offset + n:] == 12345.0).all()
            return t[offset:offset + n].reshape(nb, per).numpy()

        self.xp, self.mirror = between(buf), between(md)
        self.hist = None if hd is None else hd.cpu().numpy()
        self.eps = ed.cpu().numpy().reshape(nb, per)
        assert torch.equal(xd.cpu(), x) and torch.equal(cd.cpu(), c)


class Alone:
    """the stand-alone entry of the kind under pred on device copies; x_prev `offset` floats behind a 16-byte aligned address between canaries"""

    def __init__(self, kind, pred, x, c, row, h=None, offset=0):
        from dquartic import _native as N

        L = N.lib()
        nb, per = x.shape
        n = x.numel()
        xd, cd = x.cuda(), c.cuda()
        hd = None if h is None else h.cuda()
        coef = torch.tensor([float(r) for r in row], dtype=torch.float32).cuda()
        buf, ed = torch.full((n + 8,), 12345.0, device="cuda"), torch.full((n,), float("nan"), device="cuda")
        out = ctypes.c_void_p(buf.data_ptr() + 4 * offset)
        s = N.stream_ptr()
        if kind == "ddim":
            assert pred == PRED
            N.check(L.dq_ddim_step_v(N.ptr(xd), N.ptr(cd), out, N.ptr(ed), N.ptr(coef), n, s), "dq_ddim_step_v")
        elif kind == "stochastic":
            ids_d, seed_d = _dev_ids(IDS), _dev_seed(SEED)  # (held until the copies below have synchronised)
            N.check(L.dq_ddim_step_sto(N.ptr(xd), N.ptr(cd), out, N.ptr(ed), N.ptr(coef), N.ptr(ids_d), N.ptr(seed_d), DRAW, N.PRED_TYPES[pred],
                                       nb, per, s), "dq_ddim_step_sto")
        else:
            assert pred == PRED
            N.check(L.dq_solver_step_v(N.ptr(xd), N.ptr(cd), out, N.ptr(hd), N.ptr(ed), N.ptr(coef), ctypes.c_float(CLIP), n, s), "dq_solver_step_v")
        b = buf.cpu()
        assert (b[:offset] == 12345.0).all() and (b[offset + n:] == 12345.0).all()
        self.xp = b[offset:offset + n].reshape(nb, per).numpy()
        self.hist = None if hd is None else hd.cpu().numpy()
        self.eps = ed.cpu().numpy().reshape(nb, per)
        assert torch.equal(xd.cpu(), x) and torch.equal(cd.cpu(), c)


def forms(kind, w):
    """(per_window, offset): the vector form, the one-element form, the one-element form by alignment (the unguided stochastic entry takes
    the vector form only: per_window % 4 == 0 and 16-byte aligned tensors)"""
    return ((8, 0),) if (kind == "stochastic" and w is None) else ((8, 0), (5, 0), (8, 1))


@pytest.mark.parametrize("w", [None, 0.0, 1.0, 3.0])
@pytest.mark.parametrize("kind", KINDS)
def test_v_update(kind, w):
    table = rows(kind)
    solver = kind.startswith("solver")
    worst = {}
    engaged = left = 0
    for per, offset in forms(kind, w):
        x, c, u, h = inputs("x0", per, 100 * per + offset)  # (the 1.2-sigma network output: the derived x0 passes the clamp on some elements)
        z = randn_of(IDS, per) if kind == "stochastic" else None
        for name, row in table.items():
            h_in = h if kind == "solver_2m" else None
            r = Alone(kind, PRED, x, c, row, h=h_in, offset=offset) if w is None else Run(kind, PRED, x, c, u, w, row, h=h_in, offset=offset)
            ref = f64_v(kind, x.numpy(), c.numpy(), u.numpy(), w, row, h.numpy(), z)
            tag = (per, offset, name)
            assert np.isfinite(r.xp).all() and np.isfinite(r.eps).all(), tag
            e = np.abs(r.xp.astype(np.float64) - ref["xp"])
            ok = e <= ref["bxp"]
            worst["xp"] = max(worst.get("xp", 0.0), float((e[ref["bxp"] > 0] / ref["bxp"][ref["bxp"] > 0]).max()))
            assert ok.all(), (tag, float(e.max()))
            sel = ~ref["near"]
            ee = np.abs(r.eps.astype(np.float64) - ref["ep"])
            worst["eps"] = max(worst.get("eps", 0.0), float((ee[sel] / ref["bep"][sel]).max()))
            assert (ee[sel] <= ref["bep"][sel]).all(), (tag, float((ee[sel] / ref["bep"][sel]).max()))
            if h_in is not None:  # the history is the clamped x0: +-clip exactly where float64 clamps, within the bound elsewhere
                eh = np.abs(r.hist.astype(np.float64) - ref["x0"])
                worst["hist"] = max(worst.get("hist", 0.0), float((eh[sel & ~ref["clamped"]] / ref["bx0"][sel & ~ref["clamped"]]).max()))
                assert (eh <= np.where(ref["near"], 2 * ref["bx0"], np.where(ref["clamped"], 0.0, ref["bx0"]))).all(), tag
                assert (np.abs(r.hist) <= CLIP).all()
                if name == "last":
                    assert np.array_equal(r.xp, r.hist), tag
            if solver:
                engaged += int((ref["clamped"] & ~ref["near"]).sum())
                left += int((~ref["clamped"] & ~ref["near"]).sum())
            if offset:  # the one-element form on the vector form's inputs: the same expressions, the same bits
                v = Alone(kind, PRED, x, c, row, h=h_in) if w is None else Run(kind, PRED, x, c, u, w, row, h=h_in)
                assert np.array_equal(v.xp, r.xp) and np.array_equal(v.eps, r.eps), tag
            if w is not None:  # net_u aliased to net_c: c - u is exactly 0, every output is the stand-alone entry's, bit for bit
                a = Run(kind, PRED, x, c, u, w, row, h=h_in, offset=offset, alias_u=True)
                assert np.array_equal(a.mirror, a.xp), tag
                if not (kind == "stochastic" and (per % 4 or offset)):
                    o = Alone(kind, PRED, x, c, row, h=h_in, offset=offset)
                    assert np.array_equal(a.xp, o.xp) and np.array_equal(a.eps, o.eps), tag
                    assert o.hist is None or np.array_equal(a.hist, o.hist), tag
    if solver:
        assert engaged > 0 and left > 0, (engaged, left)
    WORST[(kind, w)] = worst
    print("v update[%s, w=%s]: worst error / bound:" % (kind, w), worst)


@pytest.mark.parametrize("kind", KINDS)
def test_three_objectives_agree(kind):
    from test_solver_sampler import K_SOLVER
    from test_stochastic_sampler import K_STEP
    from test_stream_kernels import K_DDIM, K_DDIM_X0

    per = 8
    g = torch.Generator().manual_seed(77)
    x0 = (torch.rand(B, per, generator=g, dtype=torch.float64) * 1.6 - 0.8).numpy()
    eps = torch.randn(B, per, generator=g, dtype=torch.float64).numpy()
    h = torch.randn(B, per, generator=g)
    z = randn_of(IDS, per) if kind == "stochastic" else None
    h_in = h if kind == "solver_2m" else None
    worst = 0.0
    for name, row in rows(kind).items():
        r = [float(v) for v in row]
        sa, sb = r[0], r[1]
        x_t = torch.from_numpy(sa * x0 + sb * eps).float()
        nets = {"eps": torch.from_numpy(eps).float(), "x0": torch.from_numpy(x0).float(), PRED: torch.from_numpy(sa * eps - sb * x0).float()}
        # the float64 truth of this kind and row from (x0, eps) themselves
        if r[2] < 0:
            truth = x0
        elif kind == "ddim":
            truth = r[2] * x0 + r[3] * eps
        elif kind == "stochastic":
            truth = r[2] * x0 + r[3] * eps + r[4] * z
        else:
            truth = r[2] * (sa * x0 + sb * eps) + r[3] * x0 + (r[4] * h.numpy().astype(np.float64) if r[4] != 0 else 0.0)
        got, bound = {}, {}
        for pred, net in nets.items():
            if pred == PRED:
                got[pred] = Alone(kind, pred, x_t, net, row, h=h_in).xp
                bound[pred] = f64_v(kind, x_t.numpy(), net.numpy(), None, None, row, h.numpy(), z, extra=1.0)["bxp"]
            else:
                got[pred] = RunOther(kind, pred, x_t, net, net, 1.0, row, h=h_in, alias_u=True).xp  # (aliased halves: the unguided update, bit for bit)
                ref = f64_other(kind, pred, x_t.numpy(), net.numpy(), net.numpy(), 0.0, row, h.numpy(), z)
                K = {"ddim": K_DDIM_X0 if pred == "x0" else K_DDIM, "stochastic": K_STEP}.get(kind, K_SOLVER)
                bound[pred] = ref["bxp"] * (K + 1.0) / K
                assert not ref["clamped"].any()
            e = np.abs(got[pred].astype(np.float64) - truth)
            worst = max(worst, float((e / bound[pred]).max()))
            assert (e <= bound[pred]).all(), (name, pred, float((e / bound[pred]).max()))
        for a, b in (("eps", "x0"), ("eps", PRED), ("x0", PRED)):
            d = np.abs(got[a].astype(np.float64) - got[b].astype(np.float64))
            assert (d <= bound[a] + bound[b]).all(), (name, a, b, float((d / (bound[a] + bound[b])).max()))
        if r[2] >= 0:  # (the figures are O(1): a sign or a swap would show)
            assert float(np.abs(truth).max()) > 0.5
    print("three objectives[%s]: worst error / bound against the float64 truth: %.3f" % (kind, worst))


def _tiny_v(golden):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    g = golden("tiny_x0.npz")
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)
    net.load_state_dict(sub(g, "w/"))
    return DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=1000, beta_schedule_type="cosine", pred_type=PRED, auto_normalize=True,
                              device="cuda"), g


def test_head_epilogue(golden):
    from dquartic import _native as N

    dm, g = _tiny_v(golden)
    net = dm.model
    net.eval()
    RT, MZ = g["ms2_cond"].shape[-2:]
    gen = torch.Generator().manual_seed(9)
    x_T = torch.randn(B, RT, MZ, generator=gen).cuda()
    c2, c1 = torch.rand(B, RT, MZ, generator=gen).cuda(), torch.rand(B, RT, generator=gen).cuda()
    # one default step, eager with the trajectory: traj_x is the head launch's x_prev, traj_eps its derived eps
    dm.use_graph = False
    s_e, n_e, tx, te = dm.sample(x_T, c2, c1, num_steps=1, return_trajectory=True)
    # the network output alone (dq_unet_fwd, nothing saved), then the stand-alone update on the step's row (t = 999)
    with torch.no_grad():
        v = net(x_T, torch.full((B,), 999, device="cuda", dtype=torch.long), dm.normalize(c2), dm.normalize(c1))
    cf, _ = dm.ddim_coef_table([999], 0.0)
    row = [float(a) for a in cf[0]] + [0.0]
    xp, ep = torch.empty_like(x_T), torch.empty_like(x_T)
    N.check(N.lib().dq_ddim_step_v(N.ptr(x_T), N.ptr(v), N.ptr(xp), N.ptr(ep), N.ptr(cf[0].cuda()), x_T.numel(), N.stream_ptr()), "dq_ddim_step_v")
    ref = f64_v("ddim", x_T.cpu().numpy().reshape(B, -1), v.cpu().numpy().reshape(B, -1), None, None, row, None, None)
    for name, got, alone, want, bound in (("x_prev", tx[0], xp, ref["xp"], ref["bxp"]), ("eps", te[0], ep, ref["ep"], ref["bep"])):
        e = np.abs(got.cpu().numpy().reshape(B, -1).astype(np.float64) - want)
        print(f"head epilogue {name}: worst error / bound {float((e / bound).max()):.3f}; bitwise the stand-alone kernel: {torch.equal(got, alone)}")
        assert (e <= bound).all(), (name, float((e / bound).max()))
    assert torch.equal(s_e, (tx[0] + 1) * 0.5)
    # the same step without the trajectory, eager and as a captured graph: bit for bit
    s_0, n_0 = dm.sample(x_T, c2, c1, num_steps=1)
    dm.use_graph = True
    s_g, n_g = dm.sample(x_T, c2, c1, num_steps=1)
    assert torch.equal(s_0, s_e) and torch.equal(s_g, s_e) and torch.equal(n_g, n_e) and torch.equal(n_0, n_e)
    # ... and over three steps
    dm.use_graph = False
    s3, _ = dm.sample(x_T, c2, c1, num_steps=3)
    dm.use_graph = True
    s3g, _ = dm.sample(x_T, c2, c1, num_steps=3)
    assert torch.equal(s3, s3g)
