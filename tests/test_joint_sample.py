"""``dq_ddim_sample`` over groups, ``sample(group_size=, consistency=)``, ``deconvolve_run_joint`` and ``dquartic deconvolve --joint`` on the GPU
(DESIGN.md section 40).

Network: the small one of tests/test_deconvolve_gpu.py (dim_mults = (1, 2), downsample_dim = 8), every parameter moved off its init, one
model per objective.  A joint batch is G = 2 groups of P = 3 members, member-major: rows p * G + g share the mixture of row g and carry
their own MS1.  RT = 4, so a window is 32 elements (the 16-byte form of the pass; the one-element form is tests/test_joint_kernel.py's).

What the call IS: with ``return_trajectory`` every step equals, bit for bit, ``dq_unet_fwd`` at the step's timestep, ``dq_group_project``
in place on its output, then the stand-alone update of the sampler's kind at DQ_PRED_X0 over the projected estimate -- ``dq_ddim_step_x0``
(eta = 0), ``dq_ddim_step_sto`` (eta = 1), ``dq_solver_step`` with a history (dpmpp_2m) -- over the rows of the sampler's own table;
``traj_eps`` is that update's derived eps.  Then: captured == eager, repeat == repeat, a mixture nothing reaches leaves the plain call's bits
(x0 objective, bound), consistency = 0 is the call without the group fields in result and launch count, and the members' positive parts end within the
mixture."""
import ctypes
import json

import numpy as np
import pytest
import torch

import joint_ref as R
from joint_ref import U
from test_deconvolve_gpu import UNET, equal
from test_mix_batch import same
from test_stochastic_sampler import _dev_ids, _dev_seed

pytestmark = pytest.mark.gpu

P, G, RT, MZ, NS, T, SEED = 3, 2, 4, 8, 3, 20, 987654321
B = P * G
IDS = [5, 2 ** 33 + 1, 0, 9, 77, 3]
_CACHE = {}


def model(pred, normalize=True, quiet=False):
    """one model per (objective, auto_normalize) for the module: the same weights under each.  quiet: final_conv scaled by 0.01, a
    network whose estimates stay near 0 (y near 1 / 2 in image units) whatever it is shown"""
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    if (pred, normalize, quiet) not in _CACHE:
        torch.manual_seed(41)
        net = UNet1d(**UNET)
        with torch.no_grad():
            for p in net.parameters():
                if p.requires_grad:
                    p.add_(0.3 * torch.randn_like(p))
            scaled = [p.mul_(0.01) for n, p in net.trainable_named() if quiet and n.startswith("final_conv")]
            assert len(scaled) == (2 if quiet else 0)
        dm = DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=T, pred_type=pred, auto_normalize=normalize, device="cuda")
        net.eval()
        _CACHE[(pred, normalize, quiet)] = dm
    return _CACHE[(pred, normalize, quiet)]


def inputs(scale=1.0):
    """(x_T, ms2_cond, ms1_cond) of a joint batch, device tensors: the mixture of group g repeated in rows p G + g; small enough that
    the estimates of the untrained network exceed it in places"""
    g = torch.Generator().manual_seed(23)
    xT = torch.randn(B, RT, MZ, generator=g)
    mix = scale * torch.rand(G, RT, MZ, generator=g)
    c1 = torch.rand(B, RT, generator=g)
    return xT.cuda(), mix.repeat(P, 1, 1).contiguous().cuda(), c1.cuda()


def no_graph(dm, fn):
    dm.use_graph = False
    try:
        with torch.no_grad():
            return fn()
    finally:
        dm.use_graph = True


def step_loop(dm, xT, c2, c1, sampler, eta, mode, strength, clip=0.0, seed=SEED, ids=IDS):
    """the call written out with the stand-alone entries; returns ([x after step i], [eps of step i])"""
    from dquartic import _native as N

    L, net = N.lib(), dm.model
    ts = [int(v) for v in dm.sampler_timesteps(dm.num_timesteps, NS)]
    cf, ex = dm.ddim_coef_table(ts, eta) if sampler == "reference" else dm.sampler_coef_table(ts, sampler, eta)
    rows = torch.cat([cf, ex[:, None]], dim=1).contiguous().cuda()  # 5 floats per step: the row, then sigma / c1
    cm, ca = (2.0, -1.0) if dm.auto_normalize else (1.0, 0.0)
    x = xT.clone()
    hist = torch.zeros_like(x)
    ids_d, seed_d = _dev_ids(ids), _dev_seed(seed)
    per, n = RT * MZ, x.numel()
    xs, es = [], []
    for i, t in enumerate(ts):
        row = ctypes.c_void_p(rows.data_ptr() + 20 * i)
        out = net._run_fwd(x, torch.full((B,), t, device="cuda", dtype=torch.int64), c2, c1, training=False, cond_mul=cm, cond_add=ca)
        N.check(L.dq_group_project(N.ptr(x), N.ptr(out), N.ptr(out), N.ptr(c2), row, N.PRED_TYPES[dm.pred_type], 1 if dm.auto_normalize else 0,
                                   G, P, per, R.MODES[mode], ctypes.c_float(strength), N.stream_ptr()), "dq_group_project")
        xn, ep = torch.empty_like(x), torch.empty_like(x)
        if sampler == "dpmpp_2m":
            N.check(L.dq_solver_step(N.ptr(x), N.ptr(out), N.ptr(xn), N.ptr(hist), N.ptr(ep), row, ctypes.c_float(clip), N.PRED_TYPES["x0"], n,
                                     N.stream_ptr()), "dq_solver_step")
        elif eta > 0:
            N.check(L.dq_ddim_step_sto(N.ptr(x), N.ptr(out), N.ptr(xn), N.ptr(ep), row, N.ptr(ids_d), N.ptr(seed_d), 1 + i, N.PRED_TYPES["x0"], B, per,
                                       N.stream_ptr()), "dq_ddim_step_sto")
        else:
            N.check(L.dq_ddim_step_x0(N.ptr(x), N.ptr(out), N.ptr(xn), N.ptr(ep), row, n, N.stream_ptr()), "dq_ddim_step_x0")
        x = xn
        xs.append(xn)
        es.append(ep)
    return xs, es


CASES = [("reference", 0.0, "bound", 1.0, 0.0), ("reference", 1.0, "sum", 1.0, 0.0), ("ddim", 0.0, "sum", 0.5, 0.0), ("ddim", 1.0, "bound", 0.5, 0.0),
         ("dpmpp_2m", 0.0, "bound", 1.0, 0.0), ("dpmpp_2m", 0.0, "sum", 1.0, 1.0)]


@pytest.mark.parametrize("pred", ["eps", "x0", "v_prediction"])
@pytest.mark.parametrize("sampler,eta,mode,strength,clip", CASES, ids=[f"{c[0]}-eta{c[1]:g}-{c[2]}-s{c[3]:g}-clip{c[4]:g}" for c in CASES])
def test_the_call_is_forward_project_update(pred, sampler, eta, mode, strength, clip):
    dm = model(pred)
    xT, c2, c1 = inputs(0.6)
    kw = dict(num_steps=NS, eta=eta, seed=SEED, window_ids=IDS, sampler=sampler, clip_x0=clip or None, group_size=P, consistency=mode,
              consistency_strength=strength)
    with torch.no_grad():
        s, pn, tx, te = dm.sample(xT, c2, c1, return_trajectory=True, **kw)
        xs, es = step_loop(dm, xT, c2, c1, sampler, eta, mode, strength, clip)
    for i in range(NS):
        assert torch.equal(tx[i], xs[i]), (i, float((tx[i] - xs[i]).abs().max()))
        assert torch.equal(te[i], es[i]), (i, float((te[i] - es[i]).abs().max()))
    assert torch.equal(s, (xs[-1] + 1) * 0.5) and bool(torch.isfinite(s).all())
    # the pass did something: the plain call ends elsewhere
    with torch.no_grad():
        plain, _ = dm.sample(xT, c2, c1, **{k: v for k, v in kw.items() if not k.startswith(("group", "consistency"))})
    assert not torch.equal(plain, s)
    # captured == eager == the trajectory call, and a repeat replays the cached step
    with torch.no_grad():
        g1, n1 = dm.sample(xT, c2, c1, **kw)
        g2, n2 = dm.sample(xT, c2, c1, **kw)
    e1, m1 = no_graph(dm, lambda: dm.sample(xT, c2, c1, **kw))
    assert torch.equal(g1, s) and torch.equal(n1, pn) and torch.equal(g2, s) and torch.equal(n2, pn) and torch.equal(e1, s) and torch.equal(m1, pn)


def test_the_captured_step_is_cached_by_the_three_options():
    """one handle, calls that differ in the group size, the mode or the strength only: each equals its eager call (a stale captured step
    would replay the other's pass), and going back replays the first one's result"""
    dm = model("x0")
    xT, c2, c1 = inputs(0.6)
    base = dict(num_steps=NS, sampler="ddim")
    variants = [dict(group_size=P, consistency="bound"), dict(group_size=P, consistency="sum"), dict(group_size=P, consistency="sum", consistency_strength=0.5),
                dict(group_size=1, consistency="sum"), dict(consistency="bound"), dict(), dict(group_size=P, consistency="bound")]
    eager = [no_graph(dm, lambda v=v: dm.sample(xT, c2, c1, **base, **v))[0] for v in variants]
    with torch.no_grad():
        graph = [dm.sample(xT, c2, c1, **base, **v)[0] for v in variants]
    for i, (a, b) in enumerate(zip(graph, eager)):
        assert torch.equal(a, b), (i, variants[i])
    assert torch.equal(graph[0], graph[-1])
    assert len({g.cpu().numpy().tobytes() for g in graph[:6]}) == 6  # (every variant is a result of its own)


@pytest.mark.parametrize("kw", [dict(), dict(sampler="ddim"), dict(eta=1.0, seed=SEED, window_ids=IDS), dict(sampler="dpmpp_2m", clip_x0=1.0)],
                         ids=["reference", "ddim", "eta1", "dpmpp_2m_clip"])
def test_a_mixture_nothing_reaches_leaves_the_plain_call(kw):
    """x0 objective, bound: where no group's positive parts exceed the mixture no element moves, every x0 keeps its bits, and the x0-form
    update over them is the plain call's update -- the head launch's fused one included.  The quiet network's estimates stay near
    y = 1 / 2, three of them far below a mixture of 3 .. 4"""
    dm = model("x0", quiet=True)
    xT, c2, c1 = inputs(1.0)
    c2 = c2 + 3.0
    for graph in (True, False):
        plain = (lambda: dm.sample(xT, c2, c1, num_steps=NS, **kw))
        joint = (lambda: dm.sample(xT, c2, c1, num_steps=NS, group_size=P, consistency="bound", **kw))
        with torch.no_grad():
            a, b = (plain(), joint()) if graph else (no_graph(dm, plain), no_graph(dm, joint))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), graph
    with torch.no_grad():
        ta, tb = dm.sample(xT, c2, c1, num_steps=NS, return_trajectory=True, **kw), dm.sample(xT, c2, c1, num_steps=NS, return_trajectory=True,
                                                                                                group_size=P, consistency="bound", **kw)
    assert all(torch.equal(u, v) for u, v in zip(ta, tb))
    assert float(ta[0].max()) < 0.8  # (image units: the premise -- three such members stay below the mixture)


@pytest.mark.parametrize("mode", ["bound", "sum"])
@pytest.mark.parametrize("pred", ["eps", "x0", "v_prediction"])
def test_the_members_end_within_the_mixture(pred, mode):
    """strength 1, the reference sampler (its last row returns the x0 estimate: traj_x[-1] IS the last pass's output).  Without
    auto_normalize x is in the mixture's units and the rule's bound is asked as it stands: the members' positive parts sum to at most
    m (1 + (P + 1) 2^-24) -- in "sum" mode to m within that, wherever any member is positive.  With auto_normalize the estimate is mapped back
    by 2 y' - 1, one more rounding at the scale of |x0'|, not of m -- per member 2^-24 |x0'| / 2 in image units -- and an element the pass
    left alone entered the sum as the fp32 (x0 + 1) * 0.5, 2^-24 |x0 + 1| / 2 from the float64 value formed here: both are added to the
    bound (derived, not measured; for a small m they dominate, so the bound as it stands cannot hold in those units)."""
    for normalize in (False, True):
        dm = model(pred, normalize)
        xT, c2, c1 = inputs(0.6)
        with torch.no_grad():
            _, _, tx, _ = dm.sample(xT, c2, c1, num_steps=NS, return_trajectory=True, group_size=P, consistency=mode)
        x0 = tx[-1].cpu().numpy().astype(np.float64).reshape(P, G, RT * MZ)
        m = np.maximum(c2[:G].cpu().numpy().astype(np.float64).reshape(G, RT * MZ), 0)
        y = (x0 + 1) / 2 if normalize else x0
        total = np.maximum(y, 0).sum(axis=0)
        slack = (U * (np.abs(x0) + np.abs(x0 + 1)) / 2).sum(axis=0) if normalize else 0.0
        assert (total <= m * (1 + (P + 1) * U) + slack).all(), float(((total - m) / m).max() / U)
        if mode == "sum":
            live = total > 0
            assert live.any() and (np.abs(total - m)[live] <= m[live] * (P + 1) * U + (slack[live] if normalize else 0.0)).all()
        else:
            assert (total < m * (1 - 1e-3)).any() and (total >= m * (1 - (P + 1) * U) - slack).any()  # some groups under, some on the bound


def launches(fn):
    """kernel events of one call as torch.profiler records them (tools/time_v_objective.py's count)"""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


@pytest.mark.parametrize("pred", ["eps", "v_prediction"])
def test_consistency_0_is_dq_ddim_sample_v(pred):
    """result and launch count; group_size and strength are ignored (7 does not divide the batch, NaN is no strength).  With the pass on, a
    step gains the pass and -- where the plain update rides in the head launch -- the update: 2 launches per step, 1 where it already ran
    behind the forward"""
    dm = model(pred)
    xT, c2, c1 = inputs(0.6)
    for kw, extra in ((dict(), 2), (dict(sampler=2), 1)):
        v = lambda: dm._sample_native(xT, c2, c1, NS, eta=0.0, **kw)[0]                                    # noqa: E731  (the call without the group fields)
        off = lambda: dm._sample_native(xT, c2, c1, NS, eta=0.0, joint=(7, 0, float("nan")), **kw)[0]     # noqa: E731
        on = lambda: dm._sample_native(xT, c2, c1, NS, eta=0.0, joint=(P, 1, 1.0), **kw)[0]               # noqa: E731
        for graph in (True, False):
            a, b = (v(), off()) if graph else (no_graph(dm, v), no_graph(dm, off))
            assert torch.equal(a, b), (kw, graph)
        n_v, n_off, n_on = (no_graph(dm, lambda f=f: launches(f)) for f in (v, off, on))
        assert n_v > 0 and n_off == n_v, (n_v, n_off)
        # (dpmpp_2m: exactly the pass; the reference update leaves the head launch where it rode there, one launch more)
        assert (n_on == n_v + NS) if extra == 1 else (n_v + NS <= n_on <= n_v + 2 * NS), (n_v, n_on)


# ---------------------------------------------------------------------------------------------------------------- whole runs
RT_TOTAL, W, STEP = 11, 4, 3
N_WIN = 4


def runs():
    rng = np.random.default_rng(5)
    return ((rng.lognormal(0, 1, (RT_TOTAL, MZ)) * 50).astype(np.float32), (rng.lognormal(0, 1, (P, RT_TOTAL)) * 500).astype(np.float32))


def run_joint(dm, ms2, ms1, **kw):
    res = dm.deconvolve_run_joint(torch.from_numpy(ms2).cuda(), torch.from_numpy(ms1).cuda(), window=W, step=STEP, num_steps=NS, **kw)
    assert res["n_windows"] == (len(ms2) - W + STEP - 1) // STEP + 1
    return {k: res[k].cpu().numpy() for k in ("pred", "overlap_var", "coverage", "scales")}


def test_deconvolve_run_joint_without_consistency_is_p_deconvolve_runs():
    dm = model("eps")
    ms2, ms1 = runs()
    for opts in (dict(seed=SEED), dict(seed=SEED, eta=1.0, sampler="ddim")):
        got = run_joint(dm, ms2, ms1, consistency=None, id_offset=7, batch_size=3, **opts)
        assert got["pred"].shape == (P, RT_TOTAL, MZ) == got["overlap_var"].shape and got["scales"].shape == (P, N_WIN, 4)
        assert got["coverage"].shape == (RT_TOTAL,)
        for p in range(P):
            res = dm.deconvolve_run(torch.from_numpy(ms2).cuda(), torch.from_numpy(ms1[p]).cuda(), window=W, step=STEP, num_steps=NS,
                                    id_offset=7 + p * N_WIN, batch_size=3, **opts)
            want = {k: res[k].cpu().numpy() for k in got}
            assert same(got["pred"][p], want["pred"]) and same(got["overlap_var"][p], want["overlap_var"]), (opts, p)
            assert same(got["scales"][p], want["scales"]) and same(got["coverage"], want["coverage"])
        assert same(got["scales"][0][:, :2], got["scales"][1][:, :2]) and not np.array_equal(got["scales"][0][:, 2:], got["scales"][1][:, 2:])
    # a (P, RT_total, 1) MS1 is the same call
    assert equal(run_joint(dm, ms2, ms1[:, :, None], consistency=None, id_offset=7, batch_size=3, **opts), got)


@pytest.mark.parametrize("mode", ["bound", "sum"])
def test_deconvolve_run_joint_does_not_depend_on_the_batch_size(mode):
    dm = model("x0")
    ms2, ms1 = runs()
    opts = dict(seed=SEED, eta=1.0, consistency=mode)
    whole = run_joint(dm, ms2, ms1, batch_size=N_WIN, **opts)
    for bs in (1, 2, 3):
        assert equal(run_joint(dm, ms2, ms1, batch_size=bs, **opts), whole), bs
    free = run_joint(dm, ms2, ms1, batch_size=3, seed=SEED, eta=1.0, consistency=None)
    assert not np.array_equal(free["pred"], whole["pred"]) and np.array_equal(free["scales"], whole["scales"])
    assert not any(np.isnan(v).any() for v in whole.values())
    if mode == "bound":
        # the default, and what it is for: window by window the members' positive parts stay within the observed window, so the stitched
        # members cannot explain more than the run above each window's floor by more than rounding (stitching is a convex blend per scan)
        assert equal(run_joint(dm, ms2, ms1, batch_size=3, seed=SEED, eta=1.0), whole)


def test_cli_round_trip_on_a_three_member_run(tmp_path):
    from click.testing import CliRunner

    from dquartic.cli import build_model, cli

    rt_total = 40
    cfg_path, ck_path = str(tmp_path / "c.json"), str(tmp_path / "m.ckpt")
    assert CliRunner().invoke(cli, ["generate-config", cfg_path]).exit_code == 0
    cfg = json.load(open(cfg_path))
    cfg["model"]["num_timesteps"] = T
    cfg["model"]["UNet1d"].update(dim_mults=[1, 2], downsample_dim=MZ)
    json.dump(cfg, open(cfg_path, "w"))
    torch.manual_seed(3)
    dm = build_model(cfg["model"], torch.device("cuda"))
    with torch.no_grad():
        for p in dm.model.parameters():
            if p.requires_grad:
                p.add_(0.3 * torch.randn_like(p))
    torch.save({"model_state_dict": dm.model.state_dict()}, ck_path)
    rng = np.random.default_rng(9)
    ms2 = (rng.lognormal(0, 1, (rt_total, MZ)) * 50).astype(np.float32)
    ms1 = (rng.lognormal(0, 1, (P, rt_total)) * 500).astype(np.float32)
    p2, p1, out = str(tmp_path / "ms2.npy"), str(tmp_path / "ms1.npy"), str(tmp_path / "o.npz")
    np.save(p2, ms2)
    np.save(p1, ms1)
    n_win = (rt_total - W + STEP - 1) // STEP + 1
    common = ["--window", str(W), "--step", str(STEP), "--num-steps", str(NS), "--eta", "1.0", "--seed", "3", "--batch-size", "5"]
    dm.model.eval()
    for flags, kw in ((["--joint"], dict(consistency="bound")), (["--joint", "--consistency", "sum", "--consistency-strength", "0.5"],
                                                                 dict(consistency="sum", consistency_strength=0.5))):
        r = CliRunner().invoke(cli, ["deconvolve", "--checkpoint", ck_path, "--ms2", p2, "--ms1", p1, "--out", out] + common + flags + [cfg_path])
        assert r.exit_code == 0, (r.output, r.exception)
        lines = [ln for ln in r.output.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert set(line) == {"runs", "windows", "windows_per_s"} and line["runs"] == P and line["windows"] == P * n_win and line["windows_per_s"] > 0
        z = np.load(out)
        assert set(z.files) == {"pred", "overlap_var", "coverage", "scales", "starts"} and len(z["starts"]) == n_win
        assert z["pred"].shape == (P, rt_total, MZ) and z["coverage"].shape == (rt_total,) and z["scales"].shape == (P, n_win, 4)
        want = run_joint(dm, ms2, ms1, seed=3, eta=1.0, batch_size=2, **kw)
        assert all(same(z[k], want[k]) for k in want), flags
