"""Classifier-free guidance through the whole sampler and the training loop: ``sample(..., guidance_scale=w)`` =
``dq_ddim_sample`` with its guidance fields against a float64 oracle built here from ``oracle/dq_oracle.py`` -- two ``Diffusion.net`` calls per step (the
caller's MS1, and the null's constant), g = u + w (c - u), then the update as the existing sampler tests restate it -- and conditioning
dropout in ``_train_one_batch`` / ``TrainStepGraph`` against ``train_step_fused`` on MS1 dropped by hand with the transcription of
tests/test_guidance_host.py.

Network: dim_mults = (1, 2), downsample_dim = 8, RT = 4, B = 3, 4 steps of num_timesteps = 20, every parameter moved off its init so that
MS1 matters: the oracle's conditional and null outputs differ by more than 100 times the comparison tolerance (asserted first; with
c ~ u the whole file would show nothing).

Tolerance: per step, against the oracle evaluated at the GPU's own previous state, tests/test_hip_sample.py's 1e-4 (eps) and 5e-4 (x)
relative to the largest reference value, times (1 + 2 w): 1e-4 / 5e-4 at w = 0, 7e-4 / 3.5e-3 at w = 3 (the combination carries at most
(1 + 2 w) times the rounding error of the two network outputs)."""
import ctypes

import numpy as np
import pytest
import torch

from test_guidance_host import DROP_P, cond_drop_ref, drop_mask
from test_stochastic_sampler import SEED, _dev_ids, _dev_seed

pytestmark = pytest.mark.gpu

EPS_TOL, X_TOL = 1e-4, 5e-4  # tests/test_hip_sample.py
B, RT, MZ, NS, T = 3, 4, 8, 4, 20
NULL = 0.25  # the null's raw MS1 value: (2 * 0.25 - 1) = -0.5 after the normalisation real MS1 goes through
IDS = [11, 2 ** 33 + 4, 5]


def _rel(a, b):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


_MODELS = {}


def model(pred="eps", M1=1):
    """(dm, float64 oracle, x_T, ms2, ms1) per objective and MS1 width for the whole module; nothing below modifies them"""
    key = (pred, M1)
    if key not in _MODELS:
        from dquartic.model.model import DDIMDiffusionModel
        from dquartic.model.unet1d import UNet1d
        from oracle import dq_oracle as O

        torch.manual_seed(41 + M1)
        net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=M1, downsample_dim=MZ,
                     simple=True)
        with torch.no_grad():
            for p in net.parameters():
                if p.requires_grad:
                    p.add_(0.3 * torch.randn_like(p))
        params = {k: v.detach().clone().cpu().double() for k, v in net.state_dict().items()}
        dm = DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=T, pred_type=pred, device="cuda")
        net.eval()
        od = O.Diffusion(params, O.UNetConfig(dim_mults=(1, 2), downsample_dim=MZ, attn_cond_channels=M1), T=T, pred_type=pred)
        g = torch.Generator().manual_seed(17)
        xT, c2 = torch.randn(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g)
        c1 = torch.rand(B, RT, generator=g) if M1 == 1 else torch.rand(B, RT, M1, generator=g)
        _MODELS[key] = (dm, od, xT, c2, c1)
    return _MODELS[key]


def oracle_pair(od, x, t, c2, c1):
    """the float64 oracle network at state x under the caller's MS1 and under the null"""
    from oracle import dq_oracle as O

    tt = torch.full((x.shape[0],), t, dtype=torch.long)
    x, c2n = torch.as_tensor(x).double(), O.normalize(c2.double())
    with torch.no_grad():
        c = od.net(x, tt, c2n, O.normalize(c1.double()))
        u = od.net(x, tt, c2n, O.normalize(torch.full_like(c1, NULL).double()))
    return c.numpy(), u.numpy()


def randn_of(ids, per, draw):
    from dquartic import _native as N

    out = torch.empty(len(ids), per, device="cuda")
    ids_d, seed_d = _dev_ids(list(ids)), _dev_seed(SEED)
    N.check(N.lib().dq_randn(N.ptr(out), N.ptr(ids_d), N.ptr(seed_d), draw, len(ids), per, N.stream_ptr()), "dq_randn")
    return out.cpu().numpy().astype(np.float64)


def check_trajectory(dm, od, xT, c2, c1, tx, te, w, sampler="reference", eta=0.0, clip=None, ids=None):
    """per step: the guided eps against the oracle at the GPU's own previous state, and the state against the float64 update of that
    previous state with the oracle's guided output (and, for the 2M rows, the oracle's own clamped x0 of the step before)"""
    ts = [int(v) for v in dm.sampler_timesteps(dm.num_timesteps, NS)]
    solver = sampler == "dpmpp_2m" or clip is not None
    cf, ex = dm.sampler_coef_table(ts, sampler, eta)
    if solver and sampler == "ddim":  # the clamped first-order rows: the 2M table's form [sa, sb, cx, c0] at order 1
        cf = torch.tensor(solver_order1_rows(dm, ts))
        ex = torch.zeros(len(ts))
    pred = dm.pred_type
    s = 1.0 + 2.0 * w
    tx, te = tx.double().cpu().numpy(), te.double().cpu().numpy()
    prev, hist = xT.double().numpy(), None
    gap = 0.0
    for i, t in enumerate(ts):
        sa, sb, k2, k3 = (float(v) for v in cf[i])
        c, u = oracle_pair(od, prev, t, c2, c1)
        gap = max(gap, float(np.abs(c - u).max() / np.abs(c).max()))
        g = u + w * (c - u)
        x0 = g if pred == "x0" else (prev - sb * g) / sa
        clamped = np.zeros_like(x0, dtype=bool)
        if clip is not None:
            clamped = np.abs(x0) > clip
            x0 = np.clip(x0, -clip, clip)
        ep = (prev - sa * x0) / sb
        if pred == "eps":
            ep = np.where(clamped, ep, g)
        assert _rel(te[i], ep) < s * EPS_TOL, (i, _rel(te[i], ep))
        if k2 < 0:
            ref = x0
        elif solver:
            ref = k2 * prev + k3 * x0 + (float(ex[i]) * hist if float(ex[i]) != 0 else 0.0)
        else:
            ref = k2 * x0 + k3 * ep
            if eta > 0:
                ref = ref + float(ex[i]) * randn_of(ids, RT * MZ, 1 + i).reshape(ref.shape)
        assert _rel(tx[i], ref) < s * X_TOL, (i, _rel(tx[i], ref))
        prev, hist = tx[i], x0
    return gap


def solver_order1_rows(dm, ts):
    """[sa, sb, cx, c0] of the first-order (strided DDIM, eta = 0) step in the solver's form, in float64 from the fp32 schedule: what a
    clamped 'ddim' call runs (x_prev = cx x + c0 x0 with cx = s' / s, c0 = a' - cx a; the last row returns x0)"""
    ab = dm.alpha_bars.detach().cpu().double().numpy()
    rows = []
    for i, t in enumerate(ts):
        a, sg = np.sqrt(ab[t]), np.sqrt(1 - ab[t])
        if i + 1 == len(ts):
            rows.append([a, sg, -1.0, 0.0])
        else:
            a2, s2 = np.sqrt(ab[ts[i + 1]]), np.sqrt(1 - ab[ts[i + 1]])
            rows.append([a, sg, s2 / sg, a2 - s2 / sg * a])
    return rows


@pytest.fixture
def multi(monkeypatch):
    """the oracle with ``ms1_features`` replaced by tests/test_ms1_channels.py's transcription for a (B, RT, M1) condition"""
    from oracle import dq_oracle
    from test_ms1_channels import ms1_features_multi

    monkeypatch.setattr(dq_oracle, "ms1_features", ms1_features_multi)


def test_ms1_matters_in_the_oracle(multi):
    """the premise: at every step of an unguided oracle trajectory the conditional and the null outputs differ by > 100x the loosest tolerance"""
    for key in (("eps", 1), ("x0", 1), ("eps", 3)):
        dm, od, xT, c2, c1 = model(*key)
        x = xT.double().numpy()
        for t in [int(v) for v in dm.sampler_timesteps(T, NS)]:
            c, u = oracle_pair(od, x, t, c2, c1)
            gap = float(np.abs(c - u).max() / np.abs(c).max())
            assert gap > 100 * 7 * EPS_TOL, (key, t, gap)


CASES = [dict(sampler=s, w=w) for s in ("reference", "ddim", "dpmpp_2m") for w in (0.0, 3.0)]


@pytest.mark.parametrize("pred", ["eps", "x0"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-w%g" % (c["sampler"], c["w"]))
def test_guided_trajectory_vs_oracle(case, pred):
    dm, od, xT, c2, c1 = model(pred)
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
    with torch.no_grad():
        s, pn, tx, te = dm.sample(x, a, b, num_steps=NS, return_trajectory=True, sampler=case["sampler"], guidance_scale=case["w"], null_ms1=NULL)
        sg, ng = dm.sample(x, a, b, num_steps=NS, sampler=case["sampler"], guidance_scale=case["w"], null_ms1=NULL)  # the captured step
    gap = check_trajectory(dm, od, xT, c2, c1, tx, te, case["w"], sampler=case["sampler"])
    assert gap > 100 * (1 + 2 * case["w"]) * EPS_TOL, gap
    assert torch.equal(s, (tx[-1] + 1) * 0.5) and float((pn - (a - s)).abs().max()) <= 1e-6 * max(1.0, float(s.abs().max()))
    assert torch.equal(sg, s) and torch.equal(ng, pn)  # graph replay == the eager loop the trajectory call runs
    assert torch.equal(x.cpu(), xT)


def test_guided_eta1_noise_is_dq_randn():
    dm, od, xT, c2, c1 = model("eps")
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
    kw = dict(num_steps=NS, eta=1.0, seed=SEED, window_ids=IDS, guidance_scale=3.0, null_ms1=NULL)
    try:
        with torch.no_grad():
            s, pn, tx, te = dm.sample(x, a, b, return_trajectory=True, **kw)
            sg, ng = dm.sample(x, a, b, **kw)
            sg2, _ = dm.sample(x, a, b, **kw)
            # another seed, the same w: the cached step is replayed (seed and ids are staged) and gives that seed's eager result
            so, no = dm.sample(x, a, b, **dict(kw, seed=SEED + 1))
            dm.use_graph = False
            soe, noe = dm.sample(x, a, b, **dict(kw, seed=SEED + 1))
            dm.use_graph = True
            sn, _ = dm.sample(None, a, b, **kw)  # x_T = None: dq_randn at draw 0, mirrored into the second half
    finally:
        dm.use_graph = True
    check_trajectory(dm, od, xT, c2, c1, tx, te, 3.0, eta=1.0, ids=IDS)
    assert torch.equal(sg, s) and torch.equal(ng, pn) and torch.equal(sg2, sg)
    assert not torch.equal(so, sg) and torch.equal(so, soe) and torch.equal(no, noe)
    xr = torch.from_numpy(randn_of(IDS, RT * MZ, 0)).float().reshape(B, RT, MZ).cuda()
    with torch.no_grad():
        sx, _ = dm.sample(xr, a, b, **kw)
    assert torch.equal(sn, sx)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_guided_clip_x0(sampler):
    dm, od, xT, c2, c1 = model("eps")
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
    clip = 0.5
    with torch.no_grad():
        s, pn, tx, te = dm.sample(x, a, b, num_steps=NS, return_trajectory=True, sampler=sampler, clip_x0=clip, guidance_scale=3.0, null_ms1=NULL)
        sg, _ = dm.sample(x, a, b, num_steps=NS, sampler=sampler, clip_x0=clip, guidance_scale=3.0, null_ms1=NULL)
        free, _ = dm.sample(x, a, b, num_steps=NS, sampler=sampler, guidance_scale=3.0, null_ms1=NULL)
    check_trajectory(dm, od, xT, c2, c1, tx, te, 3.0, sampler=sampler, clip=clip)
    assert torch.equal(sg, s)
    assert float(s.min()) >= (1 - clip) / 2 and float(s.max()) <= (1 + clip) / 2  # the last step returns the clamped guided x0
    assert not torch.equal(free, s)  # the clamp engaged


def test_guided_three_ms1_channels(multi):
    dm, od, xT, c2, c1 = model("eps", 3)
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
    with torch.no_grad():
        s, pn, tx, te = dm.sample(x, a, b, num_steps=NS, return_trajectory=True, guidance_scale=3.0, null_ms1=NULL)
        sg, _ = dm.sample(x, a, b, num_steps=NS, guidance_scale=3.0, null_ms1=NULL)
    gap = check_trajectory(dm, od, xT, c2, c1, tx, te, 3.0)
    assert gap > 100 * 7 * EPS_TOL and torch.equal(sg, s)


def test_graph_replay_equals_eager_loop_and_cache_by_scale():
    """as tests/test_hip_sample.py::test_graph_replay_equals_eager_loop: bit for bit, also on a second call with other inputs (the same
    captured step, conditions re-staged) and for another step count; another w captures again, the unguided call in between is its own"""
    dm, _, xT, c2, c1 = model("eps")
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
    try:
        with torch.no_grad():
            for ns, xx, cc, w in ((NS, x, a, 3.0), (3, x * 0.5, 1 - a, 3.0), (NS, x, a, 0.0), (NS, x, a, None), (NS, x, a, 3.0), (NS, x, a, 1.5)):
                dm.use_graph = True
                sg, ng = dm.sample(xx, cc, b, num_steps=ns, guidance_scale=w, null_ms1=NULL)
                dm.use_graph = False
                se, ne = dm.sample(xx, cc, b, num_steps=ns, guidance_scale=w, null_ms1=NULL)
                assert torch.equal(sg, se) and torch.equal(ng, ne), (ns, w)
            s3, _ = dm.sample(x, a, b, num_steps=NS, guidance_scale=3.0, null_ms1=NULL)
            s15, _ = dm.sample(x, a, b, num_steps=NS, guidance_scale=1.5, null_ms1=NULL)
            other_null, _ = dm.sample(x, a, b, num_steps=NS, guidance_scale=3.0, null_ms1=0.75)
    finally:
        dm.use_graph = True
    assert not torch.equal(s3, s15) and not torch.equal(s3, other_null)


def test_none_and_one_are_the_call_as_it_is():
    dm, _, xT, c2, c1 = model("eps")
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
    with torch.no_grad():
        for kw in (dict(), dict(sampler="dpmpp_2m"), dict(eta=1.0, seed=7)):
            base = dm.sample(x, a, b, num_steps=NS, **kw)
            for w in (None, 1.0, 1):
                got = dm.sample(x, a, b, num_steps=NS, guidance_scale=w, null_ms1=NULL, **kw)
                assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (kw, w)
        t0 = dm.sample(x, a, b, num_steps=NS, return_trajectory=True)
        t1 = dm.sample(x, a, b, num_steps=NS, return_trajectory=True, guidance_scale=1.0)
    assert all(torch.equal(p, q) for p, q in zip(t0, t1))


def test_w0_is_the_unguided_sample_under_the_null():
    """w = 0 is the unconditional model: the unguided sample given a constant null_ms1 MS1, within the tolerance (the plans differ between B
    and 2 B windows, so not bit for bit)"""
    for sampler in ("reference", "dpmpp_2m"):
        dm, _, xT, c2, c1 = model("eps")
        x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
        with torch.no_grad():
            s0, n0 = dm.sample(x, a, b, num_steps=NS, sampler=sampler, guidance_scale=0.0, null_ms1=NULL)
            su, nu = dm.sample(x, a, torch.full_like(b, NULL), num_steps=NS, sampler=sampler)
            sc, _ = dm.sample(x, a, b, num_steps=NS, sampler=sampler)
        assert _rel(s0, su) < X_TOL, (sampler, _rel(s0, su))
        assert _rel(s0, sc) > 100 * X_TOL  # (and not the conditional one)


def test_a_window_alone_is_the_window_in_the_batch():
    """the criterion of tests/test_scale_parity.py's batch-independence check: bit for bit (graph and eager), also with per-window noise"""
    dm, _, xT, c2, c1 = model("eps")
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
    for kw in (dict(), dict(eta=1.0, seed=SEED)):
        with torch.no_grad():
            s, pn = dm.sample(x, a, b, num_steps=NS, guidance_scale=3.0, null_ms1=NULL, window_ids=IDS if kw else None, **kw)
            for j in range(B):
                sel = slice(j, j + 1)
                s1, p1 = dm.sample(x[sel].contiguous(), a[sel].contiguous(), b[sel].contiguous(), num_steps=NS, guidance_scale=3.0, null_ms1=NULL,
                                   window_ids=IDS[sel] if kw else None, **kw)
                assert torch.equal(s1, s[sel]) and torch.equal(p1, pn[sel]), (kw, j)


def test_workspace_rule():
    """the guided call needs exactly dq_unet_workspace_bytes(plan, 2 B, RT, 0): one float less is refused, that size runs"""
    from dquartic import _native as N

    dm, _, xT, c2, c1 = model("eps")
    net = dm.model
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()[..., None].contiguous()
    need = N.lib().dq_unet_workspace_bytes(net._plan, 2 * B, RT, 0)
    assert need == net.workspace(2 * B, RT, False).numel() and need > N.lib().dq_unet_workspace_bytes(net._plan, B, RT, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    flat = net.read_params()
    ts = dm.sampler_timesteps(T, NS).to(torch.int32).tolist()
    ts_c = (ctypes.c_int32 * NS)(*ts)
    out, noise = torch.empty_like(a), torch.empty_like(a)

    def call(nbytes, w=3.0):
        q = N.sample_call(alpha_bars_host=ctypes.addressof(dm._alpha_bars_host()), num_timesteps=T, x_T=N.ptr(x), ms2_cond=N.ptr(a), ms1_cond=N.ptr(b),
                          auto_normalize=1, pred_type=0, timesteps_host=ctypes.addressof(ts_c), num_steps=NS, out_x=N.ptr(out), out_noise=N.ptr(noise),
                          workspace=N.ptr(ws), workspace_bytes=nbytes, B=B, RT=RT, stream=N.stream_ptr(), guided=1, guidance_scale=w, null_ms1=NULL)
        return N.lib().dq_ddim_sample(net._plan, N.ptr(flat), N.ptr(net.rope_freqs()), ctypes.byref(q))

    assert call(need - 4) != 0 and b"workspace too small" in N.lib().dq_last_error()
    assert call(N.lib().dq_unet_workspace_bytes(net._plan, B, RT, 0)) != 0  # the unguided size is not enough
    assert call(need) == 0
    torch.cuda.synchronize()
    with torch.no_grad():
        dm.use_graph = False
        try:
            s, _ = dm.sample(x, a, c1.cuda(), num_steps=NS, guidance_scale=3.0, null_ms1=NULL)
        finally:
            dm.use_graph = True
    assert torch.equal(out, s)


def _loader():
    g = torch.Generator().manual_seed(23)
    return [(torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g))
            for _ in range(2)]


def test_predict_and_evaluate_pass_the_scale_through():
    dm, _, _, _, _ = model("eps")
    loader = _loader()
    p0 = dm.predict(loader, num_steps=NS, seed=5, n_draws=2)
    p2 = dm.predict(loader, num_steps=NS, seed=5, n_draws=2, guidance_scale=2, null_ms1=NULL)
    p2b = dm.predict(loader, num_steps=NS, seed=5, n_draws=2, guidance_scale=2, null_ms1=NULL)
    assert len(p2) == 2 and set(p2[0]) == set(p0[0]) and "pred_std" in p2[0]
    for d0, d2, d2b in zip(p0, p2, p2b):
        assert np.isfinite(d2["pred"]).all() and not np.array_equal(d2["pred"], d0["pred"]) and not np.array_equal(d2["pred_mean"], d0["pred_mean"])
        assert np.array_equal(d2["pred"], d2b["pred"]) and np.array_equal(d2["pred_std"], d2b["pred_std"])
    e0 = dm.evaluate(loader, n_t=2, seed=3, num_steps=NS)
    e2 = dm.evaluate(loader, n_t=2, seed=3, num_steps=NS, guidance_scale=2, null_ms1=NULL)
    assert e2["guidance_scale"] == 2.0 and e2["null_ms1"] == NULL and "guidance_scale" not in e0
    assert e2["val_loss"] == e0["val_loss"]  # the loss stays conditional
    assert e2["per_window"].shape == e0["per_window"].shape and np.isfinite(e2["per_window"]).all()
    assert not np.array_equal(e2["per_window"], e0["per_window"])
    e1 = dm.evaluate(loader, n_t=2, seed=3, num_steps=NS, guidance_scale=1.0)
    assert np.array_equal(e1["per_window"], e0["per_window"])


def _trainer(seed=3):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=MZ,
                 simple=True).cuda()
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=T, device="cuda")
    dm._set_optimizer(1e-3)
    return net, dm


def _train_data(steps=3):
    g = torch.Generator().manual_seed(5)
    return [(torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g),
             torch.randint(0, T, (B,), generator=g), torch.rand(B, RT, MZ, generator=g)) for _ in range(steps)]


def test_training_with_cond_dropout_is_the_step_on_hand_dropped_ms1():
    data = _train_data()
    masks = np.stack([drop_mask(SEED, range(B), i, DROP_P) for i in range(len(data))])
    assert masks.any() and not masks.all() and any(0 < int(m.sum()) < B for m in masks), masks  # on the transcription: some dropped, some kept
    net_d, dm_d = _trainer()
    net_h, dm_h = _trainer()
    assert torch.equal(net_d.flat_params, net_h.flat_params)
    dm_d.set_cond_dropout(DROP_P, seed=SEED, null_ms1=NULL)
    for i, (x0, c2, c1, t, nz) in enumerate(data):
        ld = dm_d._train_one_batch(x0.cuda(), ms2_cond=c2.cuda(), ms1_cond=c1.cuda(), noise=nz.cuda(), t=t.cuda(), sync=False)
        c1h = torch.from_numpy(cond_drop_ref(c1.numpy(), SEED, range(B), i, DROP_P, NULL)).cuda()
        lh = dm_h.train_step_fused(x0.cuda(), c2.cuda(), c1h, t=t.cuda(), noise=dm_h.normalize(nz.cuda()), zero_grads=True)
        dm_h.optimizer.grad_scale = 1.0
        dm_h.optimizer.step()
        assert torch.equal(ld, lh), (i, float(ld), float(lh))
    assert dm_d.optimizer._step == dm_h.optimizer._step == len(data)
    assert torch.equal(net_d.flat_params, net_h.flat_params)
    # and it is not the step without the dropout
    net_p, dm_p = _trainer()
    for x0, c2, c1, t, nz in data:
        dm_p._train_one_batch(x0.cuda(), ms2_cond=c2.cuda(), ms1_cond=c1.cuda(), noise=nz.cuda(), t=t.cuda(), sync=False)
    assert not torch.equal(net_p.flat_params, net_d.flat_params)
    # the validation loss stays conditional: eval_step reads the MS1 it is given
    dm_d.set_cond_dropout(0)
    assert not dm_d.cond_dropout_enabled


def test_captured_train_step_with_cond_dropout_equals_eager():
    """as tests/test_hip_backward.py::test_captured_train_step_equals_eager_bit_for_bit, with the dropout in front of the step: outside the
    graph in the captured path, by hand (the transcription) in the eager one"""
    data = _train_data(4)
    net_e, dm_e = _trainer()
    torch.manual_seed(11)
    losses_e = []
    for i, (x0, c2, c1, _, _) in enumerate(data):
        c1h = torch.from_numpy(cond_drop_ref(c1.numpy(), SEED, range(B), i, DROP_P, NULL)).cuda()
        losses_e.append(dm_e.train_step_fused(x0.cuda(), c2.cuda(), c1h, zero_grads=True).clone())
        dm_e.optimizer.step_dev()
    net_g, dm_g = _trainer()
    dm_g.set_cond_dropout(DROP_P, seed=SEED, null_ms1=NULL)
    dm_g.enable_train_graph()
    try:
        torch.manual_seed(11)
        losses_g = [dm_g._train_one_batch(x0.cuda(), ms2_cond=c2.cuda(), ms1_cond=c1.cuda(), sync=False).clone() for x0, c2, c1, _, _ in data]
        torch.cuda.synchronize()
        assert dm_g.optimizer._step == dm_e.optimizer._step == len(data)
        for p, q in zip(losses_g, losses_e):
            assert torch.equal(p, q), (float(p), float(q))
        assert torch.equal(net_g.flat_params, net_e.flat_params)
    finally:
        dm_g.enable_train_graph(False)
