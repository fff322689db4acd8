"""Step-consistent samplers on the GPU: ``dq_solver_step`` against float64 at its loop and path edges, the float64 toy
of tests/test_sampler_tables.py run through the kernel, ``dq_ddim_sample`` with a sampler per step against the float64 oracle network and the float64
update (graph == eager == trajectory, the captured-step cache keyed by update kind and clamp), and ``predict`` / ``evaluate``.

Bounds.  An update is compared with the float64 expression over the SAME fp32 inputs and coefficients; the bound is K 2^-24 sum |terms|, the
terms of an x0 that is reconstructed from eps -- (x - sb e) / sa -- scaled by the coefficient that multiplies x0:
  mag = |cx x| + |c0| X0 + |c1 h|,  X0 = |x0| (x0 objective) or (|x| + |sb e|) / sa (eps objective); last row: X0 alone;
  the derived eps: (|x| + |sa x0|) / sb.
K_SOLVER is four times the worst ratio the MI355X showed over the cases of test_solver_step_vs_float64 (the convention of K_STEP in
tests/test_stochastic_sampler.py; the test prints the ratio before it asserts): measured 3.78 (eps objective), 2.75 (x0 objective).
TOY_TOL is four times the worst |x_fp32 - x_float64| / max |x_float64| of the toy runs: measured 1.05e-06
(100 steps, each a few roundings of a state of the size of x_T)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_sampler_tables import S_DATA, alpha_bars, sampler_table, timesteps, toy_exact
from test_stochastic_sampler import EPS_TOL, K_STEP, MZ, RT, _model

pytestmark = pytest.mark.gpu

K_SOLVER = 4 * 3.78
TOY_TOL = 4 * 1.05e-06
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the kernel alone
def solver_f64(x, v, h, row, clip, pred):
    """float64 update over fp32 inputs; row = (sa, sb, cx, c0, c1).  Returns x_prev, x0 (clamped), eps, the unclamped x0, and the magnitudes
    the bounds scale with (of x_prev, of x0 and of the derived eps)"""
    sa, sb, cx, c0, c1 = (float(r) for r in row)
    x, v = x.astype(np.float64), v.astype(np.float64)
    if pred == "x0":
        x0u, mag0 = v, np.abs(v)
    else:
        x0u, mag0 = (x - sb * v) / sa, (np.abs(x) + np.abs(sb * v)) / sa
    x0 = np.clip(x0u, -clip, clip) if clip > 0 else x0u
    clamped = x0 != x0u
    ep = (x - sa * x0) / sb
    if pred == "eps":
        ep = np.where(clamped, ep, v)
    mag_e = (np.abs(x) + np.abs(sa * x0)) / sb
    magx0 = np.where(clamped, 0.0, mag0)  # (a clamped x0 is exactly +-clip)
    if cx < 0:
        return x0, x0, ep, x0u, magx0, mag0, mag_e
    xp = cx * x + c0 * x0
    mag = np.abs(cx * x) + np.abs(c0) * np.maximum(magx0, np.abs(x0))
    if c1 != 0:
        xp = xp + c1 * h.astype(np.float64)
        mag = mag + np.abs(c1 * h)
    return xp, x0, ep, x0u, mag, mag0, mag_e


def run_solver(x, v, h, row, clip, pred, alias=False, offset=0, want_eps=True):
    """dq_solver_step on device copies.  alias: x_prev is x_t's buffer; offset: x_prev sits `offset` floats behind a 16-byte aligned address
    (the floats around it must stay untouched).  Returns x_prev, hist, eps as numpy (hist None when h is None)."""
    from dquartic import _native as N

    n = x.numel()
    xd, vd = x.cuda(), v.cuda()
    hd = None if h is None else h.cuda()
    ed = torch.empty(n, device="cuda") if want_eps else None
    coef = torch.tensor([float(r) for r in row], dtype=torch.float32).cuda()
    buf = torch.full((n + 8,), 12345.0, device="cuda")
    assert buf.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == 0
    out_ptr = xd.data_ptr() if alias else buf.data_ptr() + 4 * offset
    N.check(N.lib().dq_solver_step(N.ptr(xd), N.ptr(vd), ctypes.c_void_p(out_ptr), N.ptr(hd), N.ptr(ed), N.ptr(coef), ctypes.c_float(clip),
                                   N.PRED_TYPES[pred], n, N.stream_ptr()), "dq_solver_step")
    if alias:
        xp = xd.cpu().numpy()
    else:
        b = buf.cpu()
        assert (b[:offset] == 12345.0).all() and (b[offset + n:] == 12345.0).all()
        xp = b[offset:offset + n].numpy()
    return xp, (None if hd is None else hd.cpu().numpy()), (None if ed is None else ed.cpu().numpy())


SIZES = [1, 3, 4, 74, 1023, 1024, 1025, 2097156]  # 74: the window of DESIGN.md section 23; the last wraps the grid-stride loop of 2048 blocks


def solver_rows():
    """rows of the library's own 2M table at 4 steps (the first lands from alpha_bar = 2.4e-9: sa = 4.9e-5) and at 50 steps"""
    ab = alpha_bars("cosine")
    rows = {}
    _, c4, e4 = sampler_table(ab, timesteps(1000, 4), "dpmpp_2m")
    _, c50, e50 = sampler_table(ab, timesteps(1000, 50), "dpmpp_2m")
    rows["first_T"] = list(c4[0]) + [e4[0]]          # order 1, c1 = 0, sa tiny
    rows["second"] = list(c4[1]) + [e4[1]]           # order 2, r != 1
    rows["second_50"] = list(c50[25]) + [e50[25]]    # order 2, a short step
    rows["first_mid"] = list(c50[25]) + [0.0]        # order 1 in the middle of the schedule
    rows["last"] = list(c4[3]) + [e4[3]]
    assert rows["first_T"][4] == 0 and rows["second"][4] < 0 and rows["last"][2] == -1
    return rows


@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_solver_step_vs_float64(pred):
    rows = solver_rows()
    worst, bad = 0.0, []
    g = torch.Generator().manual_seed(11)
    for n in SIZES:
        x, v, h = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
        if pred == "x0":
            v = 1.5 * v  # exceeds a clamp of 1 on about half of the elements
        nan_h = torch.full((n,), float("nan"))
        for name, row in rows.items():
            uses_h = row[4] != 0 and row[2] >= 0
            for clip in (0.0, 1.0):
                variants = [dict()]
                if name == "second":
                    variants += [dict(alias=True), dict(offset=1), dict(want_eps=False)]
                for kw in variants:
                    hist_in = h if uses_h else nan_h  # c1 == 0 and the last row: a NaN-filled history must not be read
                    xp, hist, ep = run_solver(x, v, hist_in, row, clip, pred, **kw)
                    ref, x0, epr, x0u, mag, mag0, mag_e = solver_f64(x.numpy(), v.numpy(), h.numpy(), row, clip, pred)
                    # elements whose float64 x0 lies within the bound of +-clip may be clamped either way: x0 then differs by <= that bound
                    bx0 = K_SOLVER * U * mag0
                    near = (np.abs(np.abs(x0u) - clip) <= bx0) if clip > 0 else np.zeros(n, dtype=bool)
                    c0 = abs(float(row[3])) if row[2] >= 0 else 1.0
                    slack = np.where(near, c0 * bx0, 0.0)
                    err = np.abs(xp.astype(np.float64) - ref)
                    assert np.isfinite(xp).all(), (n, name, clip, kw)
                    ok = mag > 0
                    if ok.any():
                        worst = max(worst, float((np.maximum(err - slack, 0)[ok] / (U * mag[ok])).max()))
                    if not (err <= K_SOLVER * U * mag + slack).all():
                        bad.append((n, name, clip, kw, "x_prev"))
                    # the new history is x0: exactly +-clip where float64 clamps, within the bound of the unclamped value elsewhere
                    eh = np.abs(hist.astype(np.float64) - x0)
                    assert (eh <= np.where(near, 2 * bx0, np.where(x0 != x0u, 0.0, bx0))).all(), (n, name, clip, kw)
                    if clip > 0:
                        far = ~near
                        assert ((np.abs(hist) == clip)[far] == (x0 != x0u)[far]).all(), (n, name, clip, kw)  # the clamp decisions agree
                        assert (np.abs(hist) <= clip).all()
                    if ep is not None:
                        ee = np.abs(ep.astype(np.float64) - epr)
                        if pred == "eps":  # the network output unless the element was clamped
                            unclamped = (x0 == x0u) & ~near
                            assert (ep[unclamped] == v.numpy()[unclamped]).all()
                            sel = (x0 != x0u) & ~near
                        else:
                            sel = ~near
                        worst = max(worst, float((ee[sel] / (U * mag_e[sel])).max()) if sel.any() else 0.0)
                        if not (ee[sel] <= K_SOLVER * U * mag_e[sel]).all():
                            bad.append((n, name, clip, kw, "eps"))
    print("dq_solver_step[%s]: worst error in units of 2^-24 sum |terms| =" % pred, worst)
    assert not bad and worst <= K_SOLVER, (worst, bad[:8])


def test_solver_step_null_history_and_refusals():
    from dquartic import _native as N

    rows = solver_rows()
    g = torch.Generator().manual_seed(12)
    x, v = torch.randn(1024, generator=g), torch.randn(1024, generator=g)
    a, _, _ = run_solver(x, v, None, rows["first_mid"], 0.0, "x0")  # c1 == 0: no history needed, none written
    b, hist, _ = run_solver(x, v, torch.full((1024,), float("nan")), rows["first_mid"], 0.0, "x0")
    assert np.array_equal(a, b) and np.array_equal(hist, v.numpy())
    xd = x.cuda()
    coef = torch.zeros(5, device="cuda")
    assert N.lib().dq_solver_step(N.ptr(xd), N.ptr(xd), N.ptr(xd), None, None, N.ptr(coef), ctypes.c_float(0.0), 2, 1024, N.stream_ptr()) != 0
    assert b"pred_type" in N.lib().dq_last_error()
    assert N.lib().dq_solver_step(N.ptr(xd), None, N.ptr(xd), None, None, N.ptr(coef), ctypes.c_float(0.0), 0, 1024, N.stream_ptr()) != 0
    assert N.lib().dq_solver_step(N.ptr(xd), N.ptr(xd), N.ptr(xd), None, None, N.ptr(coef), ctypes.c_float(0.0), 0, 0, N.stream_ptr()) == 0


# ---------------------------------------------------------------------------------------------------------------- the toy through the kernel
def toy_rows(ab, ts, sampler):
    """every sampler as rows [sa, sb, cx, c0, c1] of the kernel: 2M as the library forms them; the two DDIM updates
    sap x0 + c (x - sa x0) / sb rewritten as cx = c / sb, c0 = sap - c sa / sb (float64, rounded to fp32 once)"""
    rc, coef, extra = sampler_table(ab, ts, sampler)
    assert rc == 0
    if sampler == "dpmpp_2m":
        return np.concatenate([coef, extra[:, None]], axis=1).astype(np.float32)
    rows = np.zeros((len(ts), 5), dtype=np.float32)
    for i in range(len(ts)):
        sa, sb, sap, c = (float(v) for v in coef[i])
        rows[i] = [sa, sb, -1.0, 0.0, 0.0] if sap < 0 else [sa, sb, c / sb, sap - c * sa / sb, 0.0]
    return rows


def toy_run(ab, ns, sampler, xT):
    """(fp32 result of the kernel loop, float64 recurrence over the same rows): x0 objective, the analytic predictor evaluated on the device"""
    from dquartic import _native as N

    ts = timesteps(len(ab), ns)
    rows = toy_rows(ab, ts, sampler)
    rows_d = torch.from_numpy(rows).cuda().contiguous()
    x = xT.cuda().clone()
    hist = torch.full_like(x, float("nan"))
    x64, h64 = xT.numpy().astype(np.float64), None
    s2 = S_DATA ** 2
    for i, t in enumerate(ts):
        a = float(ab[t])
        k = math.sqrt(a) * s2 / (a * s2 + 1 - a)
        pred = (x * k).contiguous()  # fp32 on the device
        N.check(N.lib().dq_solver_step(N.ptr(x), N.ptr(pred), N.ptr(x), N.ptr(hist), None, ctypes.c_void_p(rows_d.data_ptr() + 20 * i),
                                       ctypes.c_float(0.0), N.PRED_TYPES["x0"], x.numel(), N.stream_ptr()), "dq_solver_step")
        sa, sb, cx, c0, c1 = (float(v) for v in rows[i])
        p64 = x64 * k
        x64, h64 = (p64 if cx < 0 else cx * x64 + c0 * p64 + (c1 * h64 if c1 != 0 else 0.0)), p64
    return x.cpu().numpy().astype(np.float64), x64


def test_toy_through_the_kernel():
    ab = alpha_bars("cosine")
    xT = torch.randn(1024, generator=torch.Generator().manual_seed(13))
    exact = toy_exact(ab) * xT.numpy().astype(np.float64)
    err, worst = {}, 0.0
    for sampler in ("reference", "ddim", "dpmpp_2m"):
        for ns in (50, 100):
            got, want = toy_run(ab, ns, sampler, xT)
            err[sampler, ns] = float(np.abs(got - exact).max() / np.abs(exact).max())
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print("toy through dq_solver_step:", {k: float("%.3g" % v) for k, v in err.items()}, "worst fp32 - float64:", worst)
    assert err["reference", 50] > 0.9 and err["ddim", 50] < 0.04 and err["dpmpp_2m", 50] < 0.02
    assert err["dpmpp_2m", 100] < 0.3 * err["dpmpp_2m", 50]
    assert err["ddim", 100] > 0.4 * err["ddim", 50]
    assert worst <= TOY_TOL, worst


# ---------------------------------------------------------------------------------------------------------------- the whole sampler
NS = 4  # [999, 666, 333, 0]: one first-order step, two second-order steps with r != 1, the final step
_ORACLE = {}


def oracle_net(pred, x, t, c2, c1):
    """the float64 oracle network (float64 parameters and inputs) at state x"""
    from oracle import dq_oracle as O

    if pred not in _ORACLE:
        params = _model(pred)[1]
        _ORACLE[pred] = O.Diffusion({k: v.double() for k, v in params.items()}, O.UNetConfig(downsample_dim=MZ))
    with torch.no_grad():
        return _ORACLE[pred].net(x.double(), torch.full((x.shape[0],), t, dtype=torch.long), O.normalize(c2.double()), O.normalize(c1.double()))


def check_trajectory(dm, pred, sampler, xT, c2, c1, tx, te, clip=0.0):
    """per step: eps against the oracle network at the GPU's own previous state, the state against the float64 update of the GPU's own
    previous state, eps and history (x0 and the history reconstructed from eps: their terms scale as the module docstring says)"""
    ts = [int(v) for v in dm.sampler_timesteps(dm.num_timesteps, NS)]
    cf, ex = dm.sampler_coef_table(ts, sampler)
    tx, te = tx.cpu().numpy().astype(np.float64), te.cpu().numpy().astype(np.float64)
    prev, hist, hmag = xT.numpy().astype(np.float64), None, None
    for i, t in enumerate(ts):
        sa, sb, c2_, c3_ = (float(v) for v in cf[i])
        o = oracle_net(pred, torch.from_numpy(prev), t, c2, c1).numpy()
        eps_o = o if pred == "eps" else (prev - sa * o) / sb
        rel = float(np.abs(te[i] - eps_o).max() / np.abs(eps_o).max())
        assert rel < EPS_TOL, (pred, sampler, i, rel)
        e = te[i]
        x0 = (prev - sb * e) / sa
        x0mag = (np.abs(prev) + np.abs(sb * e)) / sa
        if c2_ < 0:
            ref, mag, K = x0, x0mag, max(K_STEP, K_SOLVER)
        elif sampler == "ddim":
            ref, mag, K = c2_ * x0 + c3_ * e, abs(c2_) * x0mag + np.abs(c3_ * e), K_STEP
        else:
            c1_ = float(ex[i])
            ref, mag, K = c2_ * prev + c3_ * x0, np.abs(c2_ * prev) + abs(c3_) * x0mag, K_SOLVER
            if c1_ != 0:
                ref, mag = ref + c1_ * hist, mag + abs(c1_) * hmag
        err = np.abs(tx[i] - ref)
        assert (err <= K * U * mag).all(), (pred, sampler, i, float((err / mag).max() / U))
        prev, hist, hmag = tx[i], x0, x0mag


@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_sampler_steps_graph_and_cache(pred):
    dm, _, xT, c2, c1 = _model(pred)
    x, a, b = xT[:2].cuda(), c2[:2].cuda(), c1[:2].cuda()
    settings = [dict(sampler="ddim"), dict(sampler="dpmpp_2m"), dict(sampler="ddim", clip_x0=1.0), dict(sampler="dpmpp_2m", clip_x0=1.0),
                dict(sampler="dpmpp_2m", clip_x0=0.5)]
    try:
        with torch.no_grad():
            d0 = dm.sample(x, a, b, num_steps=NS)  # the default call, before anything else
            eager, traj = [], []
            dm.use_graph = False
            for kw in settings:
                eager.append(dm.sample(x, a, b, num_steps=NS, **kw))
                traj.append(dm.sample(x, a, b, num_steps=NS, return_trajectory=True, **kw))
            dm.use_graph = True
            # each setting twice in a row (the second call replays the cached step), then interleaved: every switch recaptures or reuses the
            # step of ITS setting
            for _ in range(2):
                for kw, (se, ne) in zip(settings, eager):
                    for _ in range(2):
                        sg, ng = dm.sample(x, a, b, num_steps=NS, **kw)
                        assert torch.equal(sg, se) and torch.equal(ng, ne), kw
            d1 = dm.sample(x, a, b, num_steps=NS)
            dm.use_graph = False
            d2 = dm.sample(x, a, b, num_steps=NS)
    finally:
        dm.use_graph = True
    assert torch.equal(d0[0], d1[0]) and torch.equal(d0[1], d1[1]) and torch.equal(d0[0], d2[0])  # the default is what it was
    for kw, (se, ne), (st, nt, tx, te) in zip(settings, eager, traj):
        assert torch.equal(st, se) and torch.equal(nt, ne), kw  # the trajectory call is the same loop
        assert bool(torch.isfinite(se).all()) and float((ne - (a - se)).abs().max()) <= 1e-6 * max(1.0, float(se.abs().max()))
        assert torch.equal(se, (tx[-1] + 1) * 0.5)
        if "clip_x0" in kw:
            # every x0 estimate is inside the clamp, so the returned sample is inside [(1 - c) / 2, (1 + c) / 2]
            c = kw["clip_x0"]
            assert float(se.min()) >= (1 - c) / 2 and float(se.max()) <= (1 + c) / 2
        else:
            check_trajectory(dm, pred, kw["sampler"], xT[:2], c2[:2], c1[:2], tx, te)
    assert not torch.equal(eager[0][0], d0[0]) and not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[3][0], eager[4][0])


@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_cache_key_over_all_four_updates(pred):
    """one plan, the four update kinds of the captured step (deterministic, stochastic, first-order solver, 2M) over both tables, in two
    interleaved orders: every call replays or recaptures the step of ITS setting -- equal to that setting's eager result, bit for bit"""
    dm, _, xT, c2, c1 = _model(pred)
    x, a, b = xT[:2].cuda(), c2[:2].cuda(), c1[:2].cuda()
    settings = [dict(), dict(eta=1.0, seed=77), dict(sampler="ddim"), dict(sampler="ddim", eta=1.0, seed=77), dict(sampler="ddim", clip_x0=1.0),
                dict(sampler="dpmpp_2m")]
    try:
        with torch.no_grad():
            dm.use_graph = False
            eager = [dm.sample(x, a, b, num_steps=NS, **kw) for kw in settings]
            dm.use_graph = True
            for order in ([0, 1, 2, 3, 4, 5, 0], [5, 3, 1, 4, 0, 2, 3, 5, 1]):  # every setting follows a different one in each order
                for k in order:
                    sg, ng = dm.sample(x, a, b, num_steps=NS, **settings[k])
                    assert torch.equal(sg, eager[k][0]) and torch.equal(ng, eager[k][1]), (order, settings[k])
    finally:
        dm.use_graph = True
    # the settings are six different samplers: a stale step of another setting would not have passed unnoticed
    for i in range(len(settings)):
        for j in range(i):
            assert not torch.equal(eager[i][0], eager[j][0]), (settings[i], settings[j])


@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_strided_ddim_eta1(pred):
    dm, _, xT, c2, c1 = _model(pred)
    x, a, b = xT[:2].cuda(), c2[:2].cuda(), c1[:2].cuda()
    kw = dict(num_steps=NS, eta=1.0, seed=77, window_ids=[3, 9], sampler="ddim")
    try:
        with torch.no_grad():
            sg, ng = dm.sample(x, a, b, **kw)
            sg2, _ = dm.sample(x, a, b, **kw)
            dm.use_graph = False
            se, ne = dm.sample(x, a, b, **kw)
            dm.use_graph = True
            sr, _ = dm.sample(x, a, b, **dict(kw, sampler="reference"))
            so, _ = dm.sample(x, a, b, **dict(kw, seed=78))
            s0, _ = dm.sample(x, a, b, num_steps=NS, sampler="ddim")
    finally:
        dm.use_graph = True
    assert torch.equal(sg, se) and torch.equal(ng, ne) and torch.equal(sg, sg2)
    assert not torch.equal(sg, sr) and not torch.equal(sg, so) and not torch.equal(sg, s0)
    assert bool(torch.isfinite(sg).all())


@pytest.mark.parametrize("pred", ["eps", "x0"])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_one_step_returns_the_x0_estimate(pred, sampler):
    dm, _, xT, c2, c1 = _model(pred)
    x, a, b = xT[:2].cuda(), c2[:2].cuda(), c1[:2].cuda()
    with torch.no_grad():
        s, _ = dm.sample(x, a, b, num_steps=1, sampler=sampler)
        st, _, tx, te = dm.sample(x, a, b, num_steps=1, sampler=sampler, return_trajectory=True)
    assert torch.equal(s, st) and torch.equal(s, (tx[0] + 1) * 0.5)
    t = int(dm.sampler_timesteps(dm.num_timesteps, 1)[0])
    cf, _ = dm.sampler_coef_table([t], sampler)
    sa, sb = float(cf[0, 0]), float(cf[0, 1])
    assert cf[0, 2] == -1
    prev, e = xT[:2].numpy().astype(np.float64), te[0].cpu().numpy().astype(np.float64)
    x0, mag = (prev - sb * e) / sa, (np.abs(prev) + np.abs(sb * e)) / sa
    assert (np.abs(tx[0].cpu().numpy() - x0) <= max(K_STEP, K_SOLVER) * U * mag).all()
    o = oracle_net(pred, xT[:2], t, c2[:2], c1[:2]).numpy()
    eps_o = o if pred == "eps" else (prev - sa * o) / sb
    assert float(np.abs(e - eps_o).max() / np.abs(eps_o).max()) < EPS_TOL


# ---------------------------------------------------------------------------------------------------------------- predict / evaluate
def test_predict_and_evaluate_pass_the_sampler_through():
    from torch.utils.data import DataLoader

    from dquartic.utils.synthetic import FrozenPairDataset, SyntheticDIAMSDataset

    dm = _model("eps")[0]
    held_out = FrozenPairDataset(SyntheticDIAMSDataset(n_windows=4, RT=RT, MZ=MZ, start=5000), 4)
    l2, l4 = DataLoader(held_out, batch_size=2, shuffle=False), DataLoader(held_out, batch_size=4, shuffle=False)
    a = dm.evaluate(l2, num_steps=NS, sampler="ddim")
    b = dm.evaluate(l4, num_steps=NS, sampler="ddim")
    assert a["sampler"] == "ddim" and "clip_x0" not in a and a["num_steps"] == NS
    assert np.array_equal(a["per_window"].view(np.int32), b["per_window"].view(np.int32)) and a["val_loss"] == b["val_loss"]
    assert np.isfinite(a["per_window"]).all()
    r = dm.evaluate(l4, num_steps=NS)
    assert "sampler" not in r and "clip_x0" not in r and not np.array_equal(r["per_window"], a["per_window"])
    c = dm.evaluate(l4, num_steps=NS, sampler="dpmpp_2m", clip_x0=1.0)
    assert c["sampler"] == "dpmpp_2m" and c["clip_x0"] == 1.0 and not np.array_equal(c["per_window"], a["per_window"])
    # predict: a window's prediction under a seed does not depend on the batch size (item 0 of each batch is returned)
    p2 = dm.predict(l2, num_steps=NS, seed=5, sampler="dpmpp_2m")
    p4 = dm.predict(l4, num_steps=NS, seed=5, sampler="dpmpp_2m")
    pr = dm.predict(l4, num_steps=NS, seed=5)
    assert np.array_equal(p2[0]["pred"], p4[0]["pred"]) and np.isfinite(p4[0]["pred"]).all()
    assert not np.array_equal(pr[0]["pred"], p4[0]["pred"]) and set(p4[0]) == {"ms2_1", "ms1_1", "mixture", "pred"}
    # the default x_T path (torch's generator) takes the sampler too
    torch.manual_seed(5)
    q = dm.predict(l4, num_steps=NS, sampler="ddim", clip_x0=1.0)
    assert q[0]["pred"].min() >= 0 and q[0]["pred"].max() <= 1
