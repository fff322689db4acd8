"""Step-consistent samplers, everything that needs no GPU: ``dq_sampler_coef_table`` against the float64 formulas
written out here, the refusals (all made before any device call), and the float64 toy of the section run from the library's own tables.

The toy.  Data x0 ~ N(0, s^2), s = 0.5: the optimal x0 predictor is ``sa s^2 x / (ab s^2 + 1 - ab)`` and the probability-flow solution is
linear, ``x(t) = x_T sqrt(var(t) / var(T-1))`` with ``var = ab s^2 + 1 - ab``, so the exact sample is ``x_T s / sqrt(var(T-1))`` and every
sampler's relative error is one number that does not depend on x_T."""
import ctypes
import math

import numpy as np
import pytest
import torch

SAMPLERS = {"reference": 0, "ddim": 1, "dpmpp_2m": 2}
S_DATA = 0.5


def alpha_bars(kind, T=1000):
    from dquartic.model import model as M

    betas = (M.get_linear_beta_schedule(T) if kind == "linear" else M.get_cosine_beta_schedule(T)).to(torch.float32)
    return M.get_alpha_bars(M.get_alphas(betas).to(torch.float32)).to(torch.float32).numpy()


def timesteps(T, ns):
    from dquartic.model.model import DDIMDiffusionModel

    return [int(v) for v in DDIMDiffusionModel.sampler_timesteps(T, ns)]


def sampler_table(ab, ts, sampler, eta=0.0):
    """(rc, coef (n, 4) float32, extra (n,) float32) of dq_sampler_coef_table"""
    from dquartic import _native as N

    ab_c = (ctypes.c_float * len(ab))(*ab.tolist())
    ts_c = (ctypes.c_int32 * len(ts))(*ts)
    coef, extra = (ctypes.c_float * (4 * len(ts)))(), (ctypes.c_float * len(ts))()
    rc = N.lib().dq_sampler_coef_table(ab_c, len(ab), ts_c, len(ts), SAMPLERS[sampler] if isinstance(sampler, str) else sampler,
                                       ctypes.c_float(eta), coef, extra)
    return rc, np.array(coef, dtype=np.float32).reshape(-1, 4), np.array(extra, dtype=np.float32)


def rows_f64(ab, ts, sampler, eta=0.0):
    """the float64 formulas of the issue, from the fp32 table values: per step [sa, sb, c2, c3, extra]"""
    out = []
    n = len(ts)
    lam = lambda a: math.log(math.sqrt(a) / math.sqrt(1 - a))
    h_prev = None
    for i, t in enumerate(ts):
        a = float(ab[t])
        sa, sb = math.sqrt(a), math.sqrt(1 - a)
        if i == n - 1:
            out.append([sa, sb, -1.0, 0.0, 0.0])
            continue
        ap = float(ab[ts[i + 1]])
        sap, sbp = math.sqrt(ap), math.sqrt(1 - ap)
        if sampler == "ddim":
            sg = eta * math.sqrt((1 - ap) / (1 - a)) * math.sqrt(1 - a / ap)
            out.append([sa, sb, sap, math.sqrt(max(0.0, 1 - ap - sg * sg)), sg])
            continue
        h = lam(ap) - lam(a)
        base = -sap * math.expm1(-h)
        if i == 0:
            c0, c1 = base, 0.0
        else:
            r = h_prev / h
            c0, c1 = base * (1 + 1 / (2 * r)), -base / (2 * r)
        out.append([sa, sb, sbp / sb, c0, c1])
        h_prev = h
    return out


def ulp(w):
    return float(np.spacing(np.float32(abs(w))))


STEP_COUNTS = [1, 2, 3, 4, 50]


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_sampler_0_is_dq_ddim_coef_table(kind):
    from dquartic import _native as N

    ab = alpha_bars(kind)
    ab_c = (ctypes.c_float * len(ab))(*ab.tolist())
    for ns in STEP_COUNTS:
        ts = timesteps(1000, ns)
        for eta in (0.0, 0.5, 1.0):
            rc, coef, extra = sampler_table(ab, ts, "reference", eta)
            ts_c = (ctypes.c_int32 * ns)(*ts)
            c0, s0 = (ctypes.c_float * (4 * ns))(), (ctypes.c_float * ns)()
            assert rc == 0 and N.lib().dq_ddim_coef_table(ab_c, len(ab), ts_c, ns, ctypes.c_float(eta), c0, s0) == 0
            assert coef.tobytes() == np.array(c0, dtype=np.float32).tobytes() and extra.tobytes() == np.array(s0, dtype=np.float32).tobytes()
    # the reference table takes any list (a repeated timestep: num_steps > num_timesteps)
    assert sampler_table(ab, [5, 5, 0], "reference")[0] == 0


@pytest.mark.parametrize("kind", ["cosine", "linear"])
@pytest.mark.parametrize("T", [1, 2, 3, 7, 50, 1000])
def test_full_list_reference_is_strided_ddim(kind, T):
    """on ts = T-1 .. 0 the two landings coincide (ts[i + 1] == t - 1, and the last of the list is t == 0): one row builder serves both
    tables, so they are equal bit for bit"""
    ab = alpha_bars(kind, T)
    ts = list(range(T - 1, -1, -1))
    for eta in (0.0, 0.5, 1.0):
        rc0, c0, e0 = sampler_table(ab, ts, "reference", eta)
        rc1, c1, e1 = sampler_table(ab, ts, "ddim", eta)
        assert rc0 == 0 and rc1 == 0
        assert c0.tobytes() == c1.tobytes() and e0.tobytes() == e1.tobytes(), (kind, T, eta)
        assert c0[-1, 2] == -1 and (c0[:-1, 2] >= 0).all()


@pytest.mark.parametrize("kind", ["cosine", "linear"])
@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp_2m", 0.0)])
def test_rows_within_one_ulp_of_float64(kind, sampler, eta):
    ab = alpha_bars(kind)
    for ns in STEP_COUNTS:
        ts = timesteps(1000, ns)
        rc, coef, extra = sampler_table(ab, ts, sampler, eta)
        assert rc == 0 and np.isfinite(coef).all() and np.isfinite(extra).all()
        want = rows_f64(ab, ts, sampler, eta)
        for i in range(ns):
            got = [float(v) for v in coef[i]] + [float(extra[i])]
            for g, w in zip(got, want[i]):
                assert abs(g - w) <= ulp(w), (ns, i, got, want[i])
        assert coef[-1, 2] == -1 and coef[-1, 3] == 0 and extra[-1] == 0  # the last step returns x0, whatever its t
        if sampler == "dpmpp_2m":
            assert extra[0] == 0  # first order on the first step: the history is not read
            if ns >= 3:
                assert (extra[1:-1] < 0).all() and (coef[1:-1, 3] > 0).all()
        if sampler == "ddim" and eta > 0 and ns > 1:
            assert (extra[:-1] > 0).all()
    # a list that does not end at t = 0: the last row still returns x0
    rc, coef, extra = sampler_table(ab, [900, 500, 200], sampler, eta)
    assert rc == 0 and coef[-1, 2] == -1 and coef[0, 2] > 0


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_order_1_row_is_strided_ddim(kind):
    """cx x + c0 x0 == sap x0 + sbp (x - sa x0) / sb: row 0 of the 2M table (c1 = 0) against row 0 of the strided table, for random x, x0,
    to the rounding of the fp32 coefficients (each off its float64 value by at most 2^-24 relative, times the term it multiplies)"""
    ab = alpha_bars(kind)
    rng = np.random.default_rng(5)
    x, x0 = rng.standard_normal(1000), rng.standard_normal(1000)
    for ns in [2, 3, 4, 50]:
        ts = timesteps(1000, ns)
        _, cm, em = sampler_table(ab, ts, "dpmpp_2m")
        _, cd, _ = sampler_table(ab, ts, "ddim")
        sa, sb, cx, c0 = (float(v) for v in cm[0])
        da, db, sap, sbp = (float(v) for v in cd[0])
        assert em[0] == 0
        lhs = cx * x + c0 * x0
        rhs = sap * x0 + sbp * (x - da * x0) / db
        mag = abs(cx * x) + abs(c0 * x0) + abs(sap * x0) + (abs(sbp * x) + abs(sbp * da * x0)) / db * 3
        assert (np.abs(lhs - rhs) <= 2.0 ** -24 * mag).all(), (ns, float((np.abs(lhs - rhs) / mag).max()))


def test_table_refusals():
    from dquartic import _native as N

    ab = alpha_bars("cosine")
    for sampler in ("ddim", "dpmpp_2m"):
        for ts in ([999, 500, 500, 0], [999, 0, 1], [0, 999], [500, 500]):
            rc, _, _ = sampler_table(ab, ts, sampler)
            assert rc != 0 and b"strictly decreasing" in N.lib().dq_last_error(), (sampler, ts)
        assert sampler_table(ab, [999, 1000], sampler)[0] != 0 and sampler_table(ab, [5, -1], sampler)[0] != 0
    rc, _, _ = sampler_table(ab, [999, 0], "dpmpp_2m", 0.5)
    assert rc != 0 and b"eta" in N.lib().dq_last_error()
    for eta in (-0.1, 1.5, float("nan")):
        assert sampler_table(ab, [999, 0], "ddim", eta)[0] != 0
    rc, _, _ = sampler_table(ab, [999, 0], 3)
    assert rc != 0 and b"sampler" in N.lib().dq_last_error()
    assert sampler_table(ab, [999, 0], -1)[0] != 0


def test_python_surface_refusals():
    """every refusal is a ValueError / NotImplementedError raised on the host: the tensors here are host tensors, nothing reaches the device"""
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)
    dm = DDIMDiffusionModel(model_class=net, device="cpu")
    x, c2, c1 = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 8)
    with pytest.raises(ValueError, match="sampler"):
        dm.sample(x, c2, c1, num_steps=2, sampler="euler")
    with pytest.raises(ValueError, match="eta"):
        dm.sample(x, c2, c1, num_steps=2, sampler="dpmpp_2m", eta=0.5)
    with pytest.raises(ValueError, match="eta"):
        dm.sample(x, c2, c1, num_steps=2, sampler="ddim", eta=0.5, clip_x0=1.0)
    with pytest.raises(ValueError, match="clip_x0"):
        dm.sample(x, c2, c1, num_steps=2, clip_x0=1.0)  # the reference update has no clamp
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="clip_x0"):
            dm.sample(x, c2, c1, num_steps=2, sampler="ddim", clip_x0=bad)
    for sampler in ("ddim", "dpmpp_2m"):
        with pytest.raises(ValueError, match="strictly decreasing"):
            dm.sample(x, c2, c1, num_steps=1001, sampler=sampler)  # more steps than timesteps: the list repeats
        with pytest.raises(NotImplementedError, match="native"):
            dm.sample(x, c2, c1, num_steps=2, sampler=sampler)  # host tensors
        with pytest.raises(NotImplementedError, match="native"):
            dm.sample(x, None, None, num_steps=2, sampler=sampler)  # no conditions: the generic loop
    with pytest.raises(NotImplementedError, match="native"):
        dm.sample(x, c2, c1, num_steps=2, sampler="ddim", clip_x0=1.0)
    with pytest.raises(ValueError, match="sampler"):
        dm.sampler_coef_table([999, 0], "euler")
    with pytest.raises(ValueError, match="strictly decreasing"):
        dm.sampler_coef_table([5, 5], "ddim")
    with pytest.raises(ValueError, match="eta"):
        dm.sampler_coef_table([999, 0], "dpmpp_2m", 1.0)
    cf, ex = dm.sampler_coef_table([999, 500, 0], "dpmpp_2m")
    assert cf.shape == (3, 4) and ex.shape == (3,) and ex[0] == 0 and ex[1] < 0 and cf[2, 2] == -1
    r0, s0 = dm.sampler_coef_table([999, 500, 0], "reference", 1.0)
    r1, s1 = dm.ddim_coef_table([999, 500, 0], 1.0)
    assert torch.equal(r0, r1) and torch.equal(s0, s1)


def dummy_record(ab_c, ts_c, **fields):
    """a ``dq_sample_call`` over the host schedule ``ab_c`` and list ``ts_c`` whose required device pointers (and the seed) are the dummy
    address 4096, never dereferenced: a call that passed its checks would fault, so every use refuses something first.  B = 1, RT = 8,
    a workspace of 2^40 bytes; then ``fields``"""
    from dquartic import _native as N

    base = dict(alpha_bars_host=ctypes.addressof(ab_c), num_timesteps=len(ab_c), x_T=4096, ms2_cond=4096, ms1_cond=4096, auto_normalize=1,
                timesteps_host=ctypes.addressof(ts_c), num_steps=len(ts_c), out_x=4096, out_noise=4096, workspace=4096, workspace_bytes=1 << 40,
                B=1, RT=8, seed_dev=4096)
    base.update(fields)
    return N.sample_call(**base)


def test_sample_solver_refusals_come_before_the_device():
    """dq_ddim_sample's sampler and clamp fields with dummy (never dereferenced) pointers: each refusal names its reason and nothing is
    launched -- the process has no GPU context here and must not need one"""
    from dquartic import _native as N

    lib = N.lib()
    dims = (ctypes.c_int * 2)(1, 2)
    plan = lib.dq_plan_create(4, 2, dims, 8, 1000)
    assert plan
    try:
        ab = alpha_bars("cosine")
        ab_c = (ctypes.c_float * len(ab))(*ab.tolist())
        dummy = ctypes.c_void_p(4096)

        def call(ts, eta, sampler, clip):
            ts_c = (ctypes.c_int32 * len(ts))(*ts)
            return lib.dq_ddim_sample(plan, dummy, dummy, ctypes.byref(dummy_record(ab_c, ts_c, eta=eta, sampler=sampler, clip_x0=clip)))

        for args, word in ((([999, 0], 0.0, 7, 0.0), b"unknown sampler"), (([999, 0], 0.5, 2, 0.0), b"eta must be 0"),
                           (([999, 0], 0.5, 1, 1.0), b"clip_x0 needs eta"), (([999, 0], 0.0, 0, 1.0), b"clip_x0 needs the ddim"),
                           (([999, 999], 0.0, 1, 0.0), b"strictly decreasing"), (([0, 999], 0.0, 2, 0.0), b"strictly decreasing")):
            assert call(*args) != 0
            assert word in lib.dq_last_error() and lib.dq_last_error().startswith(b"dq_ddim_sample: "), (args, lib.dq_last_error())
    finally:
        lib.dq_plan_destroy(plan)


# ---------------------------------------------------------------------------------------------------------------- the toy
def toy_predictor(x, ab):
    return math.sqrt(ab) * S_DATA ** 2 * x / (ab * S_DATA ** 2 + 1 - ab)


def toy_exact(ab):
    """the exact sample per unit x_T: the probability-flow solution from t = T-1 to alpha_bar = 1"""
    return S_DATA / math.sqrt(float(ab[-1]) * S_DATA ** 2 + 1 - float(ab[-1]))


def toy_error(ab, ns, sampler):
    """relative error of the float64 recurrence over the library's fp32 rows, started at x_T = 1"""
    ts = timesteps(len(ab), ns)
    rc, coef, extra = sampler_table(ab, ts, sampler)
    assert rc == 0
    x, hist = 1.0, 0.0
    for i, t in enumerate(ts):
        sa, sb, c2, c3 = (float(v) for v in coef[i])
        x0 = toy_predictor(x, float(ab[t]))
        if c2 < 0:
            x = x0
        elif sampler == "dpmpp_2m":
            x = c2 * x + c3 * x0 + float(extra[i]) * hist
        else:
            x = c2 * x0 + c3 * (x - sa * x0) / sb
        hist = x0
    exact = toy_exact(ab)
    return abs(x - exact) / exact


def test_toy_orders_the_three_samplers():
    ab = alpha_bars("cosine")
    err = {(s, n): toy_error(ab, n, s) for s in SAMPLERS for n in (10, 50, 100, 1000)}
    print({k: float("%.3g" % v) for k, v in err.items()})
    assert err["reference", 50] > 0.9 and err["ddim", 50] < 0.04 and err["dpmpp_2m", 50] < 0.02
    assert err["dpmpp_2m", 100] < 0.3 * err["dpmpp_2m", 50]  # second order
    assert err["ddim", 100] > 0.4 * err["ddim", 50]          # first order
    # (DESIGN.md section 26 tabulates these figures; from the fp32 tables they are 0.933 / 0.0309 / 0.0162 at 50 steps, 0.867 / 0.0155 /
    # 0.00386 at 100 and 0.00162 / 0.00162 / 4.4e-05 at 1000 -- the reference update is exact only there)
    assert abs(err["reference", 1000] - err["ddim", 1000]) < 1e-6 and err["dpmpp_2m", 1000] < 0.1 * err["ddim", 1000]
