"""Stochastic DDIM sampling (eta > 0) with the noise of a counter-based generator inside the update kernel.

Without a GPU: this file's numpy transcription of Philox4x32-10 / Box-Muller against the Random123 known-answer vectors, and the host-only
coefficient table ``dq_ddim_coef_table`` (eta = 0: the sampler's fp32 expressions bit for bit; eta > 0: the float64 formula to 1 ulp).
On the GPU: ``dq_randn`` and ``dq_ddim_step_sto`` against the transcription in float64, ``dq_ddim_sample`` with eta = 0 set by name against
the plain ``dq_ddim_sample`` call bit for bit, an eta = 1 trajectory against a loop over the oracle's network with transcription noise, graph == eager,
seed and window-placement properties, and the Python surface (``sample`` / ``predict``).

Tolerances.  TOL_Z and K_STEP are four times the worst figure the MI355X showed on exactly these cases (the tests print the figure before
they assert); the margin is for logf / cosf implementations that differ between ROCm versions:
  TOL_Z   worst |z_gpu - z_float64| over the dq_randn cases: measured 8.59e-07 (|z| reaches 5 there, where an ulp is 4.8e-07).
  K_STEP  worst error of dq_ddim_step_sto in units of 2^-24 (|sap x0| + |c eps| + |sigma z|), the noise term's sigma * TOL_Z allowed for
          separately at the measured z error: measured 3.54 (eps objective), 2.74 (x0 objective).
The per-step eps / x tolerances of the trajectory test are those of tests/test_hip_sample.py (1e-4 / 5e-4 relative)."""
import ctypes
import math

import numpy as np
import pytest
import torch

TOL_Z = 4 * 8.59e-07
K_STEP = 4 * 3.54
EPS_TOL, X_TOL = 1e-4, 5e-4  # tests/test_hip_sample.py: per-step eps, and x (the first step amplifies an eps error ~31.6x)
SEED = 0x9E3779B97F4A7C15  # both halves non-zero
IDS = [7, 2 ** 33 + 1, 0]

# ---------------------------------------------------------------------------------------------------------------- transcription
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(c, k):
    """counter c = (c0, c1, c2, c3), key k = (k0, k1): uint64 numpy arrays (or ints) holding 32-bit words -> the four output words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in c)
    k0, k1 = (np.asarray(v, dtype=np.uint64) for v in k)
    m = np.uint64(_MASK)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(_W0)) & m, (k1 + np.uint64(_W1)) & m
    return c0, c1, c2, c3


def normal_f64(seed, w, e, d):
    """z of element(s) e of window w at draw index d: u1, u2 exact, everything after them in float64"""
    e = np.asarray(e, dtype=np.uint64)
    w = int(w) & (2 ** 64 - 1)
    r0, r1, _, _ = philox4x32_10((e, np.full_like(e, d), np.full_like(e, w & _MASK), np.full_like(e, w >> 32)),
                                 (np.full_like(e, seed & _MASK), np.full_like(e, seed >> 32)))
    u1 = ((r0 >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (r1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(float(np.float32(6.2831855)) * u2)


def noise_f64(seed, ids, per_window, d):
    return np.stack([normal_f64(seed, w, np.arange(per_window), d) for w in ids])


# ---------------------------------------------------------------------------------------------------------------- without a GPU
def test_transcription_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((_MASK,) * 4, (_MASK,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for c, k, want in kat:
        assert tuple(int(v) for v in philox4x32_10(c, k)) == want
    z = normal_f64(SEED, 3, np.arange(1 << 16), 1)
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1) < 0.03 and abs((z ** 4).mean() - 3) < 0.2  # (a normal, not a proof of one)


def _alpha_bars(kind, T=1000):
    from dquartic.model import model as M

    betas = (M.get_linear_beta_schedule(T) if kind == "linear" else M.get_cosine_beta_schedule(T)).to(torch.float32)
    return M.get_alpha_bars(M.get_alphas(betas).to(torch.float32)).to(torch.float32).numpy()


def _coef_table(ab, ts, eta):
    from dquartic import _native as N

    ab_c = (ctypes.c_float * len(ab))(*ab.tolist())
    ts_c = (ctypes.c_int32 * len(ts))(*ts)
    coef, sigma = (ctypes.c_float * (4 * len(ts)))(), (ctypes.c_float * len(ts))()
    rc = N.lib().dq_ddim_coef_table(ab_c, len(ab), ts_c, len(ts), ctypes.c_float(eta), coef, sigma)
    return rc, np.array(coef, dtype=np.float32).reshape(-1, 4), np.array(sigma, dtype=np.float32)


def _timesteps(T, ns):
    from dquartic.model.model import DDIMDiffusionModel

    return [int(v) for v in DDIMDiffusionModel.sampler_timesteps(T, ns)]


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_coef_table_eta0_is_the_samplers_fp32_table(kind):
    """model.py:265-267, 284-286 in fp32 (what dq_ddim_sample always uploaded), bit for bit; t == 0: sap = -1, c = 0; sigma = 0"""
    ab = _alpha_bars(kind)
    for ts in (_timesteps(1000, 1), _timesteps(1000, 2), _timesteps(1000, 50), [0]):
        rc, coef, sigma = _coef_table(ab, ts, 0.0)
        assert rc == 0
        want = np.empty_like(coef)
        one = np.float32(1.0)
        for i, t in enumerate(ts):  # (numpy's float32 sqrt is the correctly rounded IEEE one, like the library's std::sqrt(float))
            a = np.float32(ab[t])
            want[i, 0], want[i, 1] = np.sqrt(a), np.sqrt(one - a)
            if t > 0:
                ap = np.float32(ab[t - 1])
                want[i, 2], want[i, 3] = np.sqrt(ap), np.sqrt(one - ap)
            else:
                want[i, 2], want[i, 3] = -1.0, 0.0
        assert coef.tobytes() == want.tobytes()
        assert not sigma.any()
    assert 0 in _timesteps(1000, 50) and 0 in _timesteps(1000, 2)  # (the t == 0 row was among them)


@pytest.mark.parametrize("kind", ["cosine", "linear"])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_coef_table_eta_matches_float64(kind, eta):
    ab = _alpha_bars(kind)
    for ts in (_timesteps(1000, 1), _timesteps(1000, 2), _timesteps(1000, 50), list(range(999, -1, -1))):
        rc, coef, sigma = _coef_table(ab, ts, eta)
        assert rc == 0 and np.isfinite(coef).all() and np.isfinite(sigma).all()
        for i, t in enumerate(ts):
            a = float(ab[t])
            if t == 0:
                want = [math.sqrt(a), math.sqrt(1 - a), -1.0, 0.0, 0.0]
            else:
                ap = float(ab[t - 1])
                sg = eta * math.sqrt((1 - ap) / (1 - a)) * math.sqrt(1 - a / ap)
                want = [math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap), math.sqrt(max(0.0, 1 - ap - sg * sg)), sg]
                # c^2 + sigma^2 <= 1 - abp up to the rounding of c and sigma to fp32 (2^-24 relative each, doubled by the square)
                assert float(coef[i, 3]) ** 2 + float(sigma[i]) ** 2 <= (1 - ap) * (1 + 2.0 ** -22)
                assert sigma[i] > 0
            got = list(coef[i]) + [sigma[i]]
            for g, w in zip(got, want):
                assert abs(float(g) - w) <= float(np.spacing(np.float32(abs(w)))), (t, got, want)


@pytest.mark.parametrize("eta", [-0.1, 1.5, float("nan")])
def test_coef_table_rejects_eta_outside_0_1(eta):
    from dquartic import _native as N

    rc, _, _ = _coef_table(_alpha_bars("cosine"), [999, 0], eta)
    assert rc != 0 and b"eta" in N.lib().dq_last_error()


def test_python_surface_rejects_what_it_cannot_do():
    """eta outside [0, 1] is a ValueError; eta > 0 outside the native sampler raises instead of sampling deterministically"""
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)
    dm = DDIMDiffusionModel(model_class=net, device="cpu")
    x, c2, c1 = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 8)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            dm.sample(x, c2, c1, num_steps=2, eta=bad)
    with pytest.raises(NotImplementedError, match="native"):
        dm.sample(x, c2, c1, num_steps=2, eta=0.5)  # host tensors: the generic loop
    with pytest.raises(NotImplementedError, match="native"):
        dm.sample(x, None, None, num_steps=2, eta=1.0, seed=3)  # no conditions: the generic loop
    cf, sg = dm.ddim_coef_table([999, 0], 1.0)
    assert cf.shape == (2, 4) and sg.shape == (2,) and sg[0] > 0 and sg[1] == 0 and cf[1, 2] == -1


# ---------------------------------------------------------------------------------------------------------------- on the GPU
gpu = pytest.mark.gpu


def _dev_seed(seed):
    return torch.tensor([seed - 2 ** 64 if seed >= 2 ** 63 else seed], dtype=torch.int64, device="cuda")


def _dev_ids(ids):
    return torch.tensor(ids, dtype=torch.int64, device="cuda")


def _randn(ids, per_window, d, seed=SEED, offset=0):
    """dq_randn into a buffer `offset` floats behind a 16-byte aligned address; the floats around the output must stay untouched"""
    from dquartic import _native as N

    B = len(ids)
    buf = torch.full((B * per_window + 8,), 12345.0, device="cuda")
    assert buf.data_ptr() % 16 == 0
    ids_d, seed_d = _dev_ids(ids), _dev_seed(seed)  # (named: the pointers must outlive the launch)
    N.check(N.lib().dq_randn(ctypes.c_void_p(buf.data_ptr() + 4 * offset), N.ptr(ids_d), N.ptr(seed_d), d, B, per_window, N.stream_ptr()),
            "dq_randn")
    out = buf.cpu()
    assert (out[:offset] == 12345.0).all() and (out[offset + B * per_window:] == 12345.0).all()
    return out[offset:offset + B * per_window].reshape(B, per_window).numpy()


@gpu
def test_randn_matches_the_transcription():
    worst = 0.0
    for per in (4, 252, 256, 260, 4100):
        for d in (0, 51):
            ref = noise_f64(SEED, IDS, per, d)
            for off in (0, 1):  # 16-byte aligned, and 4 bytes behind that (the scalar path)
                z = _randn(IDS, per, d, offset=off)
                assert np.isfinite(z).all()
                worst = max(worst, float(np.abs(z.astype(np.float64) - ref).max()))
    print("dq_randn: worst |z_gpu - z_f64| =", worst)
    assert worst <= TOL_Z, worst


@gpu
def test_randn_null_ids_and_window_alone_equals_window_in_batch():
    for per in (252, 4100):
        z = _randn(IDS, per, 51)
        for pos, w in enumerate(IDS):  # alone (position 0 of 1), through both store paths, and inside the batch at another position
            assert np.array_equal(_randn([w], per, 51), z[pos:pos + 1])
            assert np.array_equal(_randn([w], per, 51, offset=1), z[pos:pos + 1])
        assert np.array_equal(_randn([5, 9, 0, 11, 7], per, 51)[4], z[0])
    from dquartic import _native as N

    out = torch.empty(3, 256, device="cuda")  # NULL ids: 0 .. B-1
    seed_d = _dev_seed(SEED)
    N.check(N.lib().dq_randn(N.ptr(out), None, N.ptr(seed_d), 2, 3, 256, N.stream_ptr()), "dq_randn")
    assert np.array_equal(out.cpu().numpy(), _randn([0, 1, 2], 256, 2))
    assert not np.array_equal(_randn([0], 256, 2), _randn([0], 256, 3)) and not np.array_equal(_randn([0], 256, 2), _randn([0], 256, 2, seed=SEED + 1))


def _step_sto(x, o, coef5, ids, d, pred, seed=SEED):
    from dquartic import _native as N

    B, per = x.shape
    xp, eo = torch.empty_like(x), torch.empty_like(x)
    ids_d, seed_d = _dev_ids(ids), _dev_seed(seed)
    N.check(N.lib().dq_ddim_step_sto(N.ptr(x), N.ptr(o), N.ptr(xp), N.ptr(eo) if pred == "x0" else None, N.ptr(coef5), N.ptr(ids_d),
                                     N.ptr(seed_d), d, N.PRED_TYPES[pred], B, per, N.stream_ptr()), "dq_ddim_step_sto")
    return xp, (eo if pred == "x0" else None)


def _update_f64(x, o, coef5, z, pred):
    """float64 update from the fp32 coefficients; returns x_prev, eps and the magnitude the bound scales with"""
    sa, sb, sap, c, sg = (float(v) for v in coef5)
    x, o = x.astype(np.float64), o.astype(np.float64)
    if pred == "x0":
        x0, ep = o, (x - sa * o) / sb
    else:
        ep, x0 = o, (x - sb * o) / sa
    if sap < 0:
        return x0, ep, np.abs(x0)
    return sap * x0 + c * ep + sg * z, ep, np.abs(sap * x0) + np.abs(c * ep) + np.abs(sg * z)


@gpu
@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_ddim_step_sto_vs_float64(pred):
    from dquartic import _native as N

    ids, per, d = [7, 2 ** 33 + 1, 0, 5, 9], 8 * 64, 3
    ab = _alpha_bars("cosine")
    g = torch.Generator().manual_seed(21)
    x, o = torch.randn(len(ids), per, generator=g), torch.randn(len(ids), per, generator=g)
    if pred == "x0":
        o = o.clamp(-1, 1)
    z = noise_f64(SEED, ids, per, d)
    xd, od = x.cuda(), o.cuda()
    worst_k = 0.0
    for t in (999, 500, 1):
        for eta in (0.5, 1.0):
            rc, cf, sg = _coef_table(ab, [t], eta)
            coef5 = torch.tensor(list(cf[0]) + [sg[0]])
            c5d = coef5.cuda()
            xp, eo = _step_sto(xd, od, c5d, ids, d, pred)
            ref, ep, mag = _update_f64(x.numpy(), o.numpy(), coef5.numpy(), z, pred)
            err = np.abs(xp.cpu().numpy().astype(np.float64) - ref)
            worst_k = max(worst_k, float((np.maximum(err - float(sg[0]) * TOL_Z / 4, 0) / (2.0 ** -24 * mag)).max()))
            assert (err <= K_STEP * 2.0 ** -24 * mag + float(sg[0]) * TOL_Z).all(), (t, eta, float((err / mag).max()))
            if pred == "x0":  # the derived eps does not depend on the noise: dq_ddim_step_x0's, bit for bit
                xq, eq = torch.empty_like(x).cuda(), torch.empty_like(x).cuda()
                N.check(N.lib().dq_ddim_step_x0(N.ptr(xd), N.ptr(od), N.ptr(xq), N.ptr(eq), N.ptr(c5d), x.numel(), N.stream_ptr()),
                        "dq_ddim_step_x0")
                assert torch.equal(eo, eq)
            # the same window at another batch position, alone: bit for bit (no row-count dispatch in this kernel)
            x1, _ = _step_sto(xd[3:4].contiguous(), od[3:4].contiguous(), c5d, ids[3:4], d, pred)
            assert torch.equal(x1, xp[3:4])
    print("dq_ddim_step_sto[%s]: worst error in units of 2^-24 (|sap x0| + |c eps| + |sigma z|) =" % pred, worst_k)
    # t == 0: x_prev = x0, no noise: dq_ddim_step / dq_ddim_step_x0 bit for bit
    rc, cf, sg = _coef_table(ab, [0], 1.0)
    coef5 = torch.tensor(list(cf[0]) + [sg[0]]).cuda()
    xp, eo = _step_sto(xd, od, coef5, ids, d, pred)
    xq, eq = torch.empty_like(xp), torch.empty_like(xp)
    if pred == "eps":
        N.check(N.lib().dq_ddim_step(N.ptr(xd), N.ptr(od), N.ptr(xq), N.ptr(coef5), x.numel(), N.stream_ptr()), "dq_ddim_step")
    else:
        N.check(N.lib().dq_ddim_step_x0(N.ptr(xd), N.ptr(od), N.ptr(xq), N.ptr(eq), N.ptr(coef5), x.numel(), N.stream_ptr()), "dq_ddim_step_x0")
        assert torch.equal(eo, eq)
    assert torch.equal(xp, xq)


RT, MZ = 8, 64


def _net(seed, perturb=0.05):
    """the 7-level network of the other sampling tests (tests/test_scale_parity.py), every tensor moved off its init"""
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True)
    with torch.no_grad():
        for p in net.parameters():
            if p.requires_grad:
                p.add_(perturb * torch.randn_like(p))
    return net, {k: v.detach().clone().cpu() for k, v in net.state_dict().items()}


_MODELS = {}


def _model(pred):
    """one network + diffusion model per objective for the whole module (its inputs ride along); nothing below modifies them"""
    if pred not in _MODELS:
        from dquartic.model.model import DDIMDiffusionModel

        net, params = _net(31)
        dm = DDIMDiffusionModel(model_class=net.cuda(), pred_type=pred, device="cuda")
        net.eval()
        g = torch.Generator().manual_seed(17)
        B = 5
        xT, c2, c1 = torch.randn(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
        _MODELS[pred] = (dm, params, xT, c2, c1)
    return _MODELS[pred]


@gpu
@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_sample_ex_eta0_is_dq_ddim_sample(pred):
    """the record with eta = 0 and null seed and ids written by name against the plain call, bit for bit: graph and eager, both objectives"""
    dm, _, xT, c2, c1 = _model(pred)
    x, a, b = xT[:2].cuda(), c2[:2].cuda(), c1[:2].cuda()
    try:
        for graph in (True, False):
            dm.use_graph = graph
            with torch.no_grad():
                s0, n0 = dm.sample(x, a, b, num_steps=3)                                  # the plain call
                s1, n1 = dm._sample_native(x, a, b, 3, eta=0.0)                          # eta, seed and ids written: 0, NULL, NULL
                s2, n2 = dm.sample(x, a, b, num_steps=3, eta=0.0, seed=5, window_ids=[4, 9])  # ... with a seed it never reads
            assert torch.equal(s0, s1) and torch.equal(n0, n1) and torch.equal(s0, s2) and torch.equal(n0, n2)
        with torch.no_grad():
            t0 = dm.sample(x, a, b, num_steps=3, return_trajectory=True)
            t1 = dm._sample_native(x, a, b, 3, True, eta=0.0)
        assert all(torch.equal(u, v) for u, v in zip(t0, t1))
    finally:
        dm.use_graph = True


def _oracle_loop(dm, params, xT, c2, c1, ns, eta, seed, ids):
    """the sampler written out: the oracle's network per step, the float64 update with transcription noise; (x, eps) per step"""
    from oracle import dq_oracle as O

    od = O.Diffusion(params, O.UNetConfig(downsample_dim=MZ))
    ts = [int(v) for v in dm.sampler_timesteps(dm.num_timesteps, ns)]
    cf, sg = dm.ddim_coef_table(ts, eta)
    c2n, c1n = O.normalize(c2), O.normalize(c1)
    x = xT.clone()
    out = []
    for i, t in enumerate(ts):
        with torch.no_grad():
            o = od.net(x, torch.full((x.shape[0],), t, dtype=torch.long), c2n, c1n)
        z = noise_f64(seed, ids, RT * MZ, 1 + i).reshape(x.shape)
        xp, ep, _ = _update_f64(x.numpy(), o.numpy(), list(cf[i]) + [sg[i]], z, dm.pred_type)
        x = torch.from_numpy(xp).float()
        out.append((x, torch.from_numpy(ep).float()))
    return out


def _rel(a, b):
    return float((a.detach().float().cpu() - b).abs().max() / b.abs().max())


@gpu
@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_eta1_trajectory_graph_and_seeds(pred):
    from dquartic import _native as N

    dm, params, xT, c2, c1 = _model(pred)
    ids, ns = [11, 2 ** 33 + 4], 3
    x, a, b = xT[:2].cuda(), c2[:2].cuda(), c1[:2].cuda()
    kw = dict(num_steps=ns, eta=1.0, seed=SEED, window_ids=ids)
    try:
        with torch.no_grad():
            s, pn, tx, te = dm.sample(x, a, b, return_trajectory=True, **kw)
            dm.use_graph = False
            se, ne = dm.sample(x, a, b, **kw)
            dm.use_graph = True
            sg, ng = dm.sample(x, a, b, **kw)
            sg2, ng2 = dm.sample(x, a, b, **kw)
            # another seed: the cached graph is replayed (seed and ids are staged in device memory) and gives the eager result of that seed
            so, no = dm.sample(x, a, b, **dict(kw, seed=SEED + 1))
            dm.use_graph = False
            soe, noe = dm.sample(x, a, b, **dict(kw, seed=SEED + 1))
            dm.use_graph = True
            # x_T = NULL is dq_randn at draw index 0
            xr = torch.empty_like(x)
            ids_d, seed_d = _dev_ids(ids), _dev_seed(SEED)
            N.check(N.lib().dq_randn(N.ptr(xr), N.ptr(ids_d), N.ptr(seed_d), 0, 2, RT * MZ, N.stream_ptr()), "dq_randn")
            sn, _ = dm.sample(None, a, b, **kw)
            sx, _ = dm.sample(xr, a, b, **kw)
    finally:
        dm.use_graph = True
    for i, (xo, eo) in enumerate(_oracle_loop(dm, params, xT[:2], c2[:2], c1[:2], ns, 1.0, SEED, ids)):
        assert _rel(te[i], eo) < EPS_TOL, (i, _rel(te[i], eo))
        assert _rel(tx[i], xo) < X_TOL, (i, _rel(tx[i], xo))
    assert torch.equal(s, se) and torch.equal(pn, ne)          # the trajectory call is the eager loop
    assert torch.equal(sg, se) and torch.equal(ng, ne)         # graph == eager
    assert torch.equal(sg2, sg) and torch.equal(ng2, ng)       # same seed twice
    assert not torch.equal(so, sg) and torch.equal(so, soe) and torch.equal(no, noe)
    assert torch.equal(sn, sx)
    assert bool(torch.isfinite(s).all()) and float((pn - (a - s)).abs().max()) < 1e-6
    with torch.no_grad():  # eta = 1 is not eta = 0
        sd, _ = dm.sample(x, a, b, num_steps=ns)
    assert not torch.equal(sd, sg)


@gpu
def test_window_placement_does_not_change_its_noise():
    """window id w at position 0 of a batch of 1 and at position 3 of a batch of 5, eta = 1: the injected noise of every step -- the residual
    x_prev - (sap x0 + c eps) of each trajectory -- is sigma z of the transcription to the step kernel's tolerance in both (the network's
    kernels may differ with the row count, so the trajectories themselves are compared through their own x0 / eps); x_T is bit-identical."""
    dm, params, xT, c2, c1 = _model("eps")
    w, ns = 2 ** 33 + 4, 3
    ids5 = [3, 1, 4, w, 5]
    ts = [int(v) for v in dm.sampler_timesteps(dm.num_timesteps, ns)]
    cf, sg = dm.ddim_coef_table(ts, 1.0)
    x0s = []
    for ids, sel in (([w], slice(3, 4)), (ids5, slice(0, 5))):
        pos = ids.index(w)
        a, b = c2[sel].cuda().contiguous(), c1[sel].cuda().contiguous()
        xr = torch.from_numpy(_randn(ids, RT * MZ, 0)).reshape(len(ids), RT, MZ)
        x0s.append(xr[pos])
        with torch.no_grad():
            _, _, tx, te = dm.sample(None, a, b, num_steps=ns, eta=1.0, seed=SEED, window_ids=ids, return_trajectory=True)
        prev = xr[pos].numpy()
        for i in range(ns):
            z = normal_f64(SEED, w, np.arange(RT * MZ), 1 + i).reshape(RT, MZ)
            coef5 = list(cf[i]) + [sg[i]]
            ref, _, mag = _update_f64(prev, te[i][pos].cpu().numpy(), coef5, z, "eps")
            cur = tx[i][pos].cpu().numpy()
            if ts[i] > 0:
                resid = cur.astype(np.float64) - (ref - float(sg[i]) * z)
                assert (np.abs(resid - float(sg[i]) * z) <= K_STEP * 2.0 ** -24 * mag + float(sg[i]) * TOL_Z).all(), (ids, i)
            prev = cur
    assert torch.equal(x0s[0], x0s[1])


@gpu
def test_predict_draws_mean_and_std():
    dm, _, xT, c2, c1 = _model("eps")
    g = torch.Generator().manual_seed(3)
    data = [(torch.rand(2, RT, MZ, generator=g), torch.rand(2, RT, generator=g), torch.rand(2, RT, MZ, generator=g), torch.rand(2, RT, generator=g))
            for _ in range(2)]
    p4 = dm.predict(data, num_steps=3, eta=1.0, seed=77, n_draws=4)
    p1 = dm.predict(data, num_steps=3, eta=1.0, seed=77, n_draws=1)
    p1b = dm.predict(data, num_steps=3, eta=1.0, seed=78)
    for d4, d1, d1b in zip(p4, p1, p1b):
        assert "pred_mean" not in d1 and "pred_std" not in d1  # n_draws == 1: the two keys are absent
        assert d4["pred_mean"].shape == d4["pred"].shape == d4["pred_std"].shape == (RT, MZ)
        assert np.isfinite(d4["pred_mean"]).all() and np.isfinite(d4["pred_std"]).all() and (d4["pred_std"] > 0).any()
        assert np.array_equal(d4["pred"], d1["pred"]) and not np.array_equal(d1["pred"], d1b["pred"])  # "pred" is draw 0 = seed + 0
    # the second batch's first window has id 2: sampled alone under that id it is the same prediction up to the kernels' row-count dispatch
    ms2_1, ms1_1, ms2_2, _ = data[1]
    mix = (ms2_1 * 0.5 + ms2_2 * 0.5).cuda()
    with torch.no_grad():
        s, _ = dm.sample(None, mix, ms1_1.cuda(), num_steps=3, eta=1.0, seed=77, window_ids=[2, 3])
    assert np.array_equal(s[0].cpu().numpy(), p1[1]["pred"])
    # the defaults are the call as it always was: x_T from torch's generator
    torch.manual_seed(5)
    q0 = dm.predict(data[:1], num_steps=3)
    torch.manual_seed(5)
    xt = torch.randn_like(data[0][0].cuda())
    with torch.no_grad():
        s, _ = dm.sample(xt, (data[0][0] * 0.5 + data[0][2] * 0.5).cuda(), data[0][1].cuda(), num_steps=3)
    assert np.array_equal(q0[0]["pred"], s[0].cpu().numpy()) and set(q0[0]) == {"ms2_1", "ms1_1", "mixture", "pred"}


@gpu
def test_p_sample_eta_goes_through_the_step_kernel():
    dm, _, xT, c2, c1 = _model("eps")
    x, a, b = xT[:2].cuda(), dm.normalize(c2[:2].cuda()), dm.normalize(c1[:2].cuda())
    ids = [11, 2 ** 33 + 4]
    with torch.no_grad():
        xp, ep = dm.p_sample(x, 500, a, b, eta=1.0, seed=SEED, window_ids=ids, draw=2)
        xd, ed = dm.p_sample(x, 500, a, b)
    assert torch.equal(ep, ed)
    cf, sg = dm.ddim_coef_table([500], 1.0)
    z = noise_f64(SEED, ids, RT * MZ, 2).reshape(2, RT, MZ)
    ref, _, mag = _update_f64(x.cpu().numpy(), ep.cpu().numpy(), list(cf[0]) + [sg[0]], z, "eps")
    assert (np.abs(xp.cpu().numpy() - ref) <= K_STEP * 2.0 ** -24 * mag + float(sg[0]) * TOL_Z).all()
    with torch.no_grad(), pytest.raises(ValueError, match="draw"):
        dm.p_sample(x, 500, a, b, eta=1.0, seed=SEED)
