"""Rescaled guidance and dynamic x0 thresholding through the whole sampler: ``sample(..., guidance_rescale=phi,
threshold_quantile=q, threshold_max=cap)`` = ``dq_ddim_sample`` with its per-window fields on the small network of tests/test_guided_sample.py, 4 steps.

Trajectory: tests/test_guided_sample.py's construction -- per step, from the GPU's own previous state, the float64 oracle network under the
caller's MS1 and under the null, then the step in float64 -- with the two steps added: m_b from the population standard deviations of a
window's c and g, and the window's q-quantile of |x0| (``torch.quantile``, linear) clamped to [f, cap], x0 <- clamp(x0, -s, s) f / s, eps
re-derived wherever x0 changed.  No bound is derived for a quantile of network outputs, so the yardstick is a float32 torch replay of the
same step from the same state around the float32 network (``dm.model`` under either condition), and the rule is tests/test_tfm_sample.py's:
the native step's max-abs error against float64 is at most twice the replay's plus one fp32 ulp of the largest reference value, for the
state and for the eps.  Observed ratios: DESIGN.md section 38.

The rest is bit for bit: the captured step against the eager loop (and the cache keyed by (phi, q, cap)), a window alone against the window
in a batch of 3, a floor nothing exceeds against ``clip_x0``, the defaults against today's call, phi without guidance against the unguided
call; then the pass-through of ``predict``, ``evaluate`` and ``deconvolve_run``, and the statistics scratch between canaries."""
import ctypes

import numpy as np
import pytest
import torch

from test_guided_sample import B, IDS, MZ, NS, NULL, RT, T, model, randn_of, solver_order1_rows
from test_stochastic_sampler import SEED
from test_winstat_host import stat_scratch_bytes

pytestmark = pytest.mark.gpu

_V = {}


def model3(pred):
    """tests/test_guided_sample.py's (dm, oracle, x_T, ms2, ms1); under the v objective the same construction with the oracle built for its
    network alone (``od.net``: the objective lives in the steps restated below)"""
    if pred != "v_prediction":
        return model(pred)
    if not _V:
        from dquartic.model.model import DDIMDiffusionModel
        from dquartic.model.unet1d import UNet1d
        from oracle import dq_oracle as O

        torch.manual_seed(42)
        net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=MZ, simple=True)
        with torch.no_grad():
            for p in net.parameters():
                if p.requires_grad:
                    p.add_(0.3 * torch.randn_like(p))
        params = {k: v.detach().clone().cpu().double() for k, v in net.state_dict().items()}
        dm = DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=T, pred_type=pred, device="cuda")
        net.eval()
        od = O.Diffusion(params, O.UNetConfig(dim_mults=(1, 2), downsample_dim=MZ, attn_cond_channels=1), T=T, pred_type="eps")
        g = torch.Generator().manual_seed(17)
        _V["m"] = (dm, od, torch.randn(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g))
    return _V["m"]


def net64(od, x, t, c2, c1, null):
    from oracle import dq_oracle as O

    tt = torch.full((x.shape[0],), t, dtype=torch.long)
    ms1 = torch.full_like(c1, NULL) if null else c1
    with torch.no_grad():
        return od.net(x.double(), tt, O.normalize(c2.double()), O.normalize(ms1.double()))


def net32(dm, x, t, c2, c1, null):
    tt = torch.full((x.shape[0],), t, device="cuda", dtype=torch.long)
    ms1 = torch.full_like(c1, NULL) if null else c1
    with torch.no_grad():
        return dm.model(x.cuda().float().contiguous(), tt, dm.normalize(c2.cuda()), dm.normalize(ms1.cuda())).cpu()


def one_step(prev, c, u, row, extra, hist, z, pred, solver, w, phi, q, f, cap):
    """one step of sections 32 and 38 in the dtype of its tensors: (x_prev, eps, x0 that is the history, s_b or None)"""
    nb = prev.shape[0]
    win = lambda v: v.reshape(nb, 1, 1)
    g = c if w is None else u + w * (c - u)
    if w is not None and phi:
        sc, sg = c.reshape(nb, -1).std(dim=1, unbiased=False), g.reshape(nb, -1).std(dim=1, unbiased=False)
        g = win(torch.where(sg > 0, phi * sc / sg + (1.0 - phi), torch.ones_like(sg))) * g
    sa, sb, k2, k3 = (float(v) for v in row)
    if pred == "x0":
        x0, ep = g, None
    elif pred == "v_prediction":
        x0, ep = sa * prev - sb * g, sb * prev + sa * g
    else:
        x0, ep = (prev - sb * g) / sa, g
    changed, s = torch.zeros_like(x0, dtype=torch.bool), None
    if q is not None or f is not None:
        floor = 1.0 if f is None else f
        s = torch.full((nb,), floor, dtype=prev.dtype)
        if q is not None:
            s = torch.quantile(x0.abs().reshape(nb, -1), float(np.float32(q)), dim=1).clamp(min=floor, max=cap)
        rho = floor / s
        x0c = torch.minimum(torch.maximum(x0, -win(s)), win(s))
        changed = (x0c != x0) | (win(rho) != 1.0)
        x0 = x0c * win(rho)
    derived = (prev - sa * x0) / sb
    ep = derived if ep is None else torch.where(changed, derived, ep)
    if k2 < 0:
        xp = x0
    elif solver:
        xp = k2 * prev + k3 * x0
        if float(extra) != 0:
            xp = xp + float(extra) * hist
    else:
        xp = k2 * x0 + k3 * ep
        if z is not None:
            xp = xp + float(extra) * z
    return xp, ep, x0, s


def check(pred, sampler, w=None, eta=0.0, phi=0.0, q=None, clip=None, cap=None, expect_threshold=False):
    dm, od, xT, c2, c1 = model3(pred)
    kw = dict(num_steps=NS, sampler=sampler, guidance_rescale=phi, threshold_quantile=q, threshold_max=cap, clip_x0=clip)
    if w is not None:
        kw.update(guidance_scale=w, null_ms1=NULL)
    if eta:
        kw.update(eta=eta, seed=SEED, window_ids=IDS)
    x, a, b = xT.cuda(), c2.cuda(), c1.cuda()
    with torch.no_grad():
        s, pn, tx, te = dm.sample(x, a, b, return_trajectory=True, **kw)
        sg, ng = dm.sample(x, a, b, **kw)  # the captured step
    assert torch.equal(sg, s) and torch.equal(ng, pn)
    ts = [int(v) for v in dm.sampler_timesteps(T, NS)]
    solver = sampler == "dpmpp_2m" or clip is not None or q is not None
    cf, ex = dm.sampler_coef_table(ts, sampler, eta)
    if solver and sampler == "ddim":
        cf, ex = torch.tensor(solver_order1_rows(dm, ts)), torch.zeros(len(ts))
    tx, te = tx.cpu(), te.cpu()
    prev, hist64, hist32 = xT, None, None
    rose, worst = 0, 0.0
    inf = float("inf")
    for i, t in enumerate(ts):
        z = torch.from_numpy(randn_of(IDS, RT * MZ, 1 + i)).reshape(B, RT, MZ) if eta else None
        args = (pred, solver, w, phi, q, clip, inf if cap is None else cap)
        c64, u64 = net64(od, prev, t, c2, c1, False), (net64(od, prev, t, c2, c1, True) if w is not None else None)
        rx, re, h64, s64 = one_step(prev.double(), c64, u64, cf[i].double(), ex[i].double(), hist64, z, *args)
        c32, u32 = net32(dm, prev, t, c2, c1, False), (net32(dm, prev, t, c2, c1, True) if w is not None else None)
        yx, ye, h32, _ = one_step(prev.float(), c32, u32, cf[i].float(), ex[i].float(), hist32, None if z is None else z.float(), *args)
        if q is not None:
            rose += int((s64 > (1.0 if clip is None else clip)).sum())
        for name, got, yard, ref in (("x", tx[i], yx, rx), ("eps", te[i], ye, re)):
            e_nat, e_yard = float((got.double() - ref).abs().max()), float((yard.double() - ref).abs().max())
            ulp = float(np.spacing(np.float32(ref.abs().max())))
            worst = max(worst, e_nat / (2.0 * e_yard + ulp))
            assert e_nat <= 2.0 * e_yard + ulp, (pred, sampler, i, name, e_nat, e_yard, ulp)
        # the next step starts from the GPU's state; the histories are each side's own x0 of this step
        prev, hist64, hist32 = tx[i], h64, h32
    assert torch.equal(s.cpu(), (tx[-1] + 1) * 0.5)
    if expect_threshold:
        assert rose > 0  # q is low enough that windows are thresholded above the floor
    print("adaptive trajectory %s: worst err_native / (2 err_yardstick + ulp) = %.3f" % ((pred, sampler, w, eta, phi, q, clip), worst))


@pytest.mark.parametrize("pred", ["eps", "x0", "v_prediction"])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_threshold_trajectory(sampler, pred):
    check(pred, sampler, q=0.9, expect_threshold=True)


@pytest.mark.parametrize("pred", ["eps", "x0", "v_prediction"])
@pytest.mark.parametrize("sampler,eta", [("reference", 0.0), ("ddim", 0.0), ("dpmpp_2m", 0.0), ("reference", 1.0), ("ddim", 1.0)])
def test_rescale_trajectory(sampler, eta, pred):
    check(pred, sampler, w=3.0, eta=eta, phi=0.7)


@pytest.mark.parametrize("pred", ["eps", "x0", "v_prediction"])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_both_trajectory(sampler, pred):
    check(pred, sampler, w=3.0, phi=0.7, q=0.9, clip=0.75, cap=4.0, expect_threshold=True)


def _xab(pred="eps"):
    dm, _, xT, c2, c1 = model3(pred)
    return dm, xT.cuda(), c2.cuda(), c1.cuda()


def test_captured_step_equals_eager_and_the_cache_tells_the_options_apart():
    dm, x, a, b = _xab()
    base = dict(num_steps=NS, sampler="dpmpp_2m", guidance_scale=3.0, null_ms1=NULL)
    opts = (dict(guidance_rescale=0.7), dict(guidance_rescale=0.3), dict(guidance_rescale=0.7, threshold_quantile=0.9),
            dict(guidance_rescale=0.7, threshold_quantile=0.5), dict(guidance_rescale=0.7, threshold_quantile=0.5, threshold_max=1.5),
            dict(threshold_quantile=0.5, threshold_max=1.5), dict(), dict(guidance_rescale=0.7))
    got = []
    try:
        with torch.no_grad():
            for o in opts:
                dm.use_graph = True
                sg, ng = dm.sample(x, a, b, **base, **o)
                sg2, _ = dm.sample(x * 0.5, 1 - a, b, **base, **o)  # the same captured step on other inputs
                dm.use_graph = False
                se, ne = dm.sample(x, a, b, **base, **o)
                se2, _ = dm.sample(x * 0.5, 1 - a, b, **base, **o)
                assert torch.equal(sg, se) and torch.equal(ng, ne) and torch.equal(sg2, se2), o
                got.append(sg)
    finally:
        dm.use_graph = True
    assert torch.equal(got[0], got[-1])
    for i in range(len(opts) - 1):
        for j in range(i + 1, len(opts) - 1):
            assert not torch.equal(got[i], got[j]), (opts[i], opts[j])  # every option changes the result: none was served by another's graph


def test_a_window_alone_is_the_window_in_the_batch():
    dm, x, a, b = _xab()
    for kw in (dict(sampler="dpmpp_2m", guidance_scale=3.0, null_ms1=NULL, guidance_rescale=0.7, threshold_quantile=0.9),
               dict(sampler="ddim", threshold_quantile=0.5), dict(eta=1.0, seed=SEED, guidance_scale=3.0, null_ms1=NULL, guidance_rescale=1.0)):
        ids = IDS if "seed" in kw else None
        with torch.no_grad():
            s, pn = dm.sample(x, a, b, num_steps=NS, window_ids=ids, **kw)
            for j in range(B):
                sel = slice(j, j + 1)
                s1, p1 = dm.sample(x[sel].contiguous(), a[sel].contiguous(), b[sel].contiguous(), num_steps=NS,
                                   window_ids=None if ids is None else ids[sel], **kw)
                assert torch.equal(s1, s[sel]) and torch.equal(p1, pn[sel]), (kw, j)


def test_neutral_options_are_todays_calls_bit_for_bit():
    for pred in ("eps", "v_prediction"):
        dm, x, a, b = _xab(pred)
        with torch.no_grad():
            for kw in (dict(sampler="ddim"), dict(sampler="dpmpp_2m", guidance_scale=3.0, null_ms1=NULL)):
                # a floor so high that no window's quantile exceeds it: the clip_x0 = f step
                base = dm.sample(x, a, b, num_steps=NS, clip_x0=1e4, **kw)
                thr = dm.sample(x, a, b, num_steps=NS, clip_x0=1e4, threshold_quantile=0.9, **kw)
                assert torch.equal(thr[0], base[0]) and torch.equal(thr[1], base[1]), (pred, kw)
                t0 = dm.sample(x, a, b, num_steps=NS, clip_x0=1e4, return_trajectory=True, **kw)
                t1 = dm.sample(x, a, b, num_steps=NS, clip_x0=1e4, threshold_quantile=0.9, return_trajectory=True, **kw)
                assert all(torch.equal(p, q) for p, q in zip(t0, t1)), (pred, kw)
            for kw in (dict(), dict(sampler="dpmpp_2m"), dict(eta=1.0, seed=7), dict(sampler="ddim", clip_x0=0.5),
                       dict(sampler="dpmpp_2m", guidance_scale=3.0, null_ms1=NULL)):
                base = dm.sample(x, a, b, num_steps=NS, **kw)
                # phi = 0 with q unset is the call as it is; without guidance (None, 1.0) phi > 0 is too: g = c, m = 1
                variants = [dict(guidance_rescale=0.0, threshold_quantile=None, threshold_max=None)]
                if "guidance_scale" not in kw:
                    variants += [dict(guidance_rescale=0.7), dict(guidance_rescale=0.7, guidance_scale=1.0, null_ms1=NULL)]
                for v in variants:
                    got = dm.sample(x, a, b, num_steps=NS, **kw, **v)
                    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (pred, kw, v)


def test_the_options_do_something():
    """the premise of the bit-for-bit tests above: at w = 3 the rescale shrinks the guided output, and a low floor is exceeded"""
    dm, x, a, b = _xab()
    with torch.no_grad():
        g = dict(num_steps=NS, sampler="dpmpp_2m", guidance_scale=3.0, null_ms1=NULL)
        plain, _ = dm.sample(x, a, b, **g)
        resc, _ = dm.sample(x, a, b, guidance_rescale=0.7, **g)
        clip, _ = dm.sample(x, a, b, clip_x0=0.25, **g)
        thr, _ = dm.sample(x, a, b, clip_x0=0.25, threshold_quantile=0.5, **g)
        capped, _ = dm.sample(x, a, b, clip_x0=0.25, threshold_quantile=0.5, threshold_max=0.25, **g)
    assert not torch.equal(plain, resc) and not torch.equal(clip, thr)
    assert torch.equal(capped, clip)  # cap == floor: s_b = f, rho_b = 1 in every window
    assert float(thr.min()) >= (1 - 0.25) / 2 - 1e-6 and float(thr.max()) <= (1 + 0.25) / 2 + 1e-6  # the last step returns x0 within the floor


def test_predict_evaluate_and_deconvolve_run_pass_the_options_through():
    from test_guided_sample import _loader

    dm, _, _, _, _ = model3("eps")
    loader = _loader()
    opt = dict(sampler="ddim", guidance_scale=3, null_ms1=NULL, guidance_rescale=0.7, clip_x0=0.25, threshold_quantile=0.5, threshold_max=2.0)
    off = dict(sampler="ddim", guidance_scale=3, null_ms1=NULL, clip_x0=0.25)
    p0 = dm.predict(loader, num_steps=NS, seed=5, **off)
    p1 = dm.predict(loader, num_steps=NS, seed=5, **opt)
    p1b = dm.predict(loader, num_steps=NS, seed=5, **opt)
    for d0, d1, d1b in zip(p0, p1, p1b):
        assert np.isfinite(d1["pred"]).all() and not np.array_equal(d1["pred"], d0["pred"]) and np.array_equal(d1["pred"], d1b["pred"])
    e0 = dm.evaluate(loader, n_t=2, seed=3, num_steps=NS, **off)
    e1 = dm.evaluate(loader, n_t=2, seed=3, num_steps=NS, **opt)
    assert (e1["guidance_rescale"], e1["threshold_quantile"], e1["threshold_max"]) == (0.7, 0.5, 2.0)
    assert not any(k in e0 for k in ("guidance_rescale", "threshold_quantile", "threshold_max"))
    assert e1["val_loss"] == e0["val_loss"] and np.isfinite(e1["per_window"]).all() and not np.array_equal(e1["per_window"], e0["per_window"])
    g = torch.Generator().manual_seed(9)
    ms2, ms1 = torch.rand(3 * RT, MZ, generator=g).cuda(), torch.rand(3 * RT, generator=g).cuda()
    run = dict(window=RT, step=2, batch_size=2, num_steps=NS, seed=11)
    r0 = dm.deconvolve_run(ms2, ms1, **run, **off)
    r1 = dm.deconvolve_run(ms2, ms1, **run, **opt)
    r1b = dm.deconvolve_run(ms2, ms1, **run, **opt)
    assert torch.isfinite(r1["pred"]).all() and not torch.equal(r1["pred"], r0["pred"]) and torch.equal(r1["pred"], r1b["pred"])


def test_the_scratch_between_canaries():
    """a direct call on a scratch of exactly dq_sample_stat_scratch_bytes(B, RT * MZ) bytes between canaries: one byte less is refused, the
    canaries stay, the result is sample()'s"""
    from dquartic import _native as N

    dm, x, a, b = _xab()
    net = dm.model
    c1 = b[..., None].contiguous()
    need = N.lib().dq_sample_stat_scratch_bytes(B, RT * MZ)
    assert need == stat_scratch_bytes(B, RT * MZ)
    buf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = net.workspace(2 * B, RT, False)
    flat = net.read_params()
    ts_c = (ctypes.c_int32 * NS)(*dm.sampler_timesteps(T, NS).to(torch.int32).tolist())
    out, noise = torch.empty_like(a), torch.empty_like(a)

    def call(nbytes, graph):
        q = N.sample_call(alpha_bars_host=ctypes.addressof(dm._alpha_bars_host()), num_timesteps=T, x_T=N.ptr(x), ms2_cond=N.ptr(a), ms1_cond=N.ptr(c1),
                          auto_normalize=1, pred_type=0, timesteps_host=ctypes.addressof(ts_c), num_steps=NS, out_x=N.ptr(out), out_noise=N.ptr(noise),
                          use_graph=graph, workspace=N.ptr(ws), workspace_bytes=ws.numel(), B=B, RT=RT, stream=N.stream_ptr(), sampler=2, guided=1,
                          guidance_scale=3.0, null_ms1=NULL, guidance_rescale=0.7, threshold_quantile=0.9, threshold_max=float("inf"),
                          stat_scratch=buf.data_ptr() + 256, stat_scratch_bytes=nbytes)
        return N.lib().dq_ddim_sample(net._plan, N.ptr(flat), N.ptr(net.rope_freqs()), ctypes.byref(q))

    assert call(need - 1, 0) != 0 and b"scratch too small" in N.lib().dq_last_error()
    with torch.no_grad():
        want, _ = dm.sample(x, a, b, num_steps=NS, sampler="dpmpp_2m", guidance_scale=3.0, null_ms1=NULL, guidance_rescale=0.7, threshold_quantile=0.9)
    for graph in (0, 1):
        out.zero_()
        assert call(need, graph) == 0, N.last_error()
        torch.cuda.synchronize()
        assert torch.equal(out, want), graph
        h = buf.cpu()
        assert (h[:256] == 0xA5).all() and (h[256 + need:] == 0xA5).all(), graph
