"""Sampling from the CustomTransformer inside the library (dq_tfm_sample), on the GPU.

Ground truth: a float64 loop written here -- oracle.dq_oracle_tfm.forward on double parameters (read-only use of the oracle) around the float64
update over the rows of dm.ddim_coef_table / dm.sampler_coef_table at dm.sampler_timesteps.  Yardstick: the path that exists without this
feature -- the generic Python loop (sample() with native_tfm_sampler off and default arguments: dq_tfm_fwd plus one stand-alone update kernel per
step) for the reference sampler; for the samplers that loop cannot run, a float32 torch replay of the same rows around net(...) per step,
written here.  Pass condition per case: the native result's max-abs error against float64 is at most TWICE the yardstick's on the same case,
plus one fp32 ulp of the largest value.  Both run the same fp32 arithmetic; what differs is the order of sums (the fused attention, the K | V
rows projected per sample, the time MLP over the steps instead of over the samples), which the factor 2 covers.  No absolute tolerance: an
untrained network's first step amplifies its eps error by 1 / sqrt(alpha_bar_T).  Measured values: DESIGN.md section 29.

Shapes: CustomTransformer(64, 32, heads 2, layers 2) at B = 3, S1 = 10, S2 = 7; (64, 128, 1, 1) at S1 = 5, S2 = 9; and (64, 128, 1, 1) at B = 1,
S1 = S2 = 77, whose Sk = 154 is one past what the fused attention takes (the three-launch form through the same loop).  3 and 5 steps.

Bitwise claims: the captured step equals the eager loop and the trajectory's last entry for all four update kinds; a changed MS1, parameters
changed in place behind the same pointer and ema_scope() never meet a stale cache or graph; seeds repeat; x_t=None is dq_randn's draw 0; eta = 0
ignores the seed; a window's noise follows its id, not its place in the batch (through a zeroed output projection, so that no GEMM plan enters
the comparison); with native_tfm_sampler off and default arguments sample() is the generic loop, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import dq_oracle_tfm as OT

pytestmark = pytest.mark.gpu

T = 1000
CFG = {
    "two_layers": dict(D=64, H=32, heads=2, layers=2, B=3, S1=10, S2=7),
    "wide_head": dict(D=64, H=128, heads=1, layers=1, B=3, S1=5, S2=9),
    "three_launch": dict(D=64, H=128, heads=1, layers=1, B=1, S1=77, S2=77),
}


@functools.lru_cache(maxsize=None)
def _params(name):
    c = CFG[name]
    return OT.init_params(c["D"], c["H"], c["layers"], seed=11 + c["H"])


def _model(name, pred="eps", norm=True):
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    c = CFG[name]
    tf = CustomTransformer(input_dim=c["D"], hidden_dim=c["H"], num_heads=c["heads"], num_layers=c["layers"])
    tf.load_state_dict(_params(name))
    dm = DDIMDiffusionModel(model_class=DDIMTransformerAdapter(tf).cuda(), num_timesteps=T, beta_schedule_type="cosine", pred_type=pred,
                            auto_normalize=norm, ms1_loss_weight=0.0, device="cuda")
    return dm


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = CFG[name]
    g = torch.Generator().manual_seed(5 + c["S1"])
    return (torch.randn(c["B"], c["S1"], c["D"], generator=g), torch.rand(c["B"], c["S1"], c["D"], generator=g),
            torch.rand(c["B"], c["S2"], generator=g))


def _rows(dm, num_steps, sampler):
    ts = [int(v) for v in dm.sampler_timesteps(T, num_steps)]
    cf, ex = dm.ddim_coef_table(ts, 0.0) if sampler == "reference" else dm.sampler_coef_table(ts, sampler)
    return ts, cf.double().numpy(), ex.double().numpy()


def _update(x, out, row, c1, hist, pred, solver, clip):
    """one update in the dtype of x (torch): the expressions of ddim_elem / solver_elem (csrc/k_update.hip).  Returns x_prev and the x0 that is the history"""
    sa, sb, a2, a3 = (float(v) for v in row)
    if pred == "x0":
        x0 = out
        ep = (x - sa * x0) / sb
    else:
        ep = out
        x0 = (x - sb * ep) / sa
    if clip:
        x0c = x0.clamp(-clip, clip)
        ep = torch.where(x0c != x0, (x - sa * x0c) / sb, ep)
        x0 = x0c
    if a2 < 0:
        return x0, x0
    if not solver:
        return a2 * x0 + a3 * ep, x0
    y = a2 * x + a3 * x0
    return (y + float(c1) * hist if float(c1) != 0.0 else y), x0


@functools.lru_cache(maxsize=None)
def _truth(name, pred, norm, num_steps, sampler, clip):
    """the float64 loop: (denoised, mixture - denoised) as sample() returns them"""
    dm = _model(name, pred, norm)
    c = CFG[name]
    p64 = {k: v.double() for k, v in _params(name).items()}
    xT, c2, c1 = _inputs(name)
    ts, cf, ex = _rows(dm, num_steps, sampler)
    x, hist = xT.double(), None
    cn = (c1.double() * 2 - 1) if norm else c1.double()
    for i, t in enumerate(ts):
        with torch.no_grad():
            out = OT.forward(p64, x, torch.full((c["B"],), float(t), dtype=torch.float64), cn, c["heads"])  # (a double t: float64 time features)
        x, hist = _update(x, out, cf[i], ex[i], hist, pred, sampler == "dpmpp_2m", clip)
    if norm:
        x = (x + 1) * 0.5
    return x, c2.double() - x


def _replay32(dm, name, num_steps, sampler, clip):
    """the yardstick for what the generic loop cannot run: the same rows in float32 torch around net(...) per step"""
    xT, c2, c1 = (v.cuda() for v in _inputs(name))
    ts, cf, ex = _rows(dm, num_steps, sampler)
    x, hist = xT.clone(), None
    ms2n, ms1n = dm.normalize(c2), dm.normalize(c1)
    with torch.no_grad():
        for i, t in enumerate(ts):
            out = dm.model(x, torch.full((x.shape[0],), t, device="cuda", dtype=torch.long), ms2n, ms1n)
            x, hist = _update(x, out, cf[i].astype(np.float32), np.float32(ex[i]), hist, dm.pred_type, sampler == "dpmpp_2m", clip)
    return dm.unnormalize(x)


def _err(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max())


SAMPLERS = [("reference", None), ("ddim", None), ("dpmpp_2m", None), ("ddim", 1.0)]


# the two small shapes in full; the three-launch form runs the same loop: one step count, normalised
LOOP_CASES = [(name, sampler, clip, pred, norm, steps) for name in ("two_layers", "wide_head") for sampler, clip in SAMPLERS for pred in ("eps", "x0")
              for norm in (True, False) for steps in (3, 5)]
LOOP_CASES += [("three_launch", sampler, clip, pred, True, 3) for sampler, clip in SAMPLERS for pred in ("eps", "x0")]


@pytest.mark.parametrize("name,sampler,clip,pred,norm,num_steps", LOOP_CASES,
                         ids=[f"{n}-{s}{'-clip' if c else ''}-{p}-{'norm' if m else 'raw'}-{k}" for n, s, c, p, m, k in LOOP_CASES])
def test_native_loop_vs_float64(name, sampler, clip, pred, norm, num_steps):
    from dquartic import _native as N

    c = CFG[name]
    fused = N.lib().dq_tfm_attn_form(c["S1"], c["S1"] + c["S2"], c["H"] // c["heads"])
    assert fused == (0 if name == "three_launch" else 1)
    dm = _model(name, pred, norm)
    xT, c2, c1 = (v.cuda() for v in _inputs(name))
    ref_x, ref_n = _truth(name, pred, norm, num_steps, sampler, clip)
    kw = {} if sampler == "reference" else {"sampler": sampler}
    if clip:
        kw["clip_x0"] = clip
    with torch.no_grad():
        if sampler == "reference":
            yard, _ = dm.sample(xT, c2, c1, num_steps=num_steps)  # the generic loop: today's path
        else:
            yard = _replay32(dm, name, num_steps, sampler, clip)
        dm.native_tfm_sampler = True
        got_x, got_n = dm.sample(xT, c2, c1, num_steps=num_steps, **kw)
    e_nat, e_yard = _err(got_x, ref_x), _err(yard, ref_x)
    ulp = float(np.spacing(np.float32(ref_x.abs().max())))
    print(f"tfm_sample {name} {sampler} clip={clip} {pred} norm={norm} steps={num_steps}: native={e_nat:.3e} yardstick={e_yard:.3e} "
          f"max|ref|={float(ref_x.abs().max()):.3e}")
    assert torch.isfinite(got_x).all()
    assert e_nat <= 2.0 * e_yard + ulp, (e_nat, e_yard, ulp)
    assert _err(got_n, ref_n) <= 2.0 * e_yard + ulp + float(np.spacing(np.float32(ref_n.abs().max())))  # mixture - denoised


KINDS = [dict(), dict(eta=1.0, seed=77), dict(sampler="ddim", clip_x0=1.0), dict(sampler="dpmpp_2m")]  # DDIM, STOCHASTIC, SOLVER_1, SOLVER_2M


@pytest.mark.parametrize("pred", ["eps", "x0"])
@pytest.mark.parametrize("name", ["two_layers", "wide_head"])
def test_captured_step_equals_eager_and_trajectory(name, pred):
    dm = _model(name, pred)
    dm.native_tfm_sampler = True
    xT, c2, c1 = (v.cuda() for v in _inputs(name))
    with torch.no_grad():
        dm.use_graph = False
        eager = [dm.sample(xT, c2, c1, num_steps=4, **kw) for kw in KINDS]
        traj = [dm.sample(xT, c2, c1, num_steps=4, return_trajectory=True, **kw) for kw in KINDS]
        dm.use_graph = True
        for order in ([0, 1, 2, 3, 0], [3, 1, 2, 0, 3, 3]):  # every kind recaptures or replays the step of ITS setting
            for k in order:
                sg, ng = dm.sample(xT, c2, c1, num_steps=4, **KINDS[k])
                assert torch.equal(sg, eager[k][0]) and torch.equal(ng, eager[k][1]), (order, KINDS[k])
    for (se, ne), (st, nt, tx, te) in zip(eager, traj):
        assert tx.shape == (4,) + tuple(xT.shape) and te.shape == tx.shape
        assert torch.equal(st, se) and torch.equal(nt, ne)
        assert torch.equal(se, (tx[-1] + 1) * 0.5) and torch.isfinite(te).all()
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[2][0], eager[3][0])


def test_no_stale_cache():
    """same workspace, graph on: each call against a fresh eager call on the same state, bit for bit"""
    dm = _model("two_layers")
    dm.native_tfm_sampler = True
    tfm = dm.model.transformer
    xT, c2, c1 = (v.cuda() for v in _inputs("two_layers"))
    c1b = torch.flip(c1, dims=[1]).contiguous() * 0.5

    def both(ms1):
        dm.use_graph = True
        g = dm.sample(xT, c2, ms1, num_steps=3)
        dm.use_graph = False
        e = dm.sample(xT, c2, ms1, num_steps=3)
        dm.use_graph = True
        assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1])
        return g[0]

    with torch.no_grad():
        a = both(c1)
        ws = tfm.sample_workspace(3, 10, 7, 3).data_ptr()
        b = both(c1b)  # another MS1 through the same captured step
        assert not torch.equal(a, b)
        assert torch.equal(both(c1), a)
        ptr = tfm.flat_params.data_ptr()
        tfm.flat_params.mul_(1.25)  # the weights change behind the same pointer
        assert tfm.flat_params.data_ptr() == ptr
        c = both(c1)
        assert not torch.equal(c, a)
        tfm.flat_params.div_(1.25)
        assert tfm.sample_workspace(3, 10, 7, 3).data_ptr() == ws
    # the averaged weights: inside ema_scope() and outside
    x0 = torch.rand(3, 10, 64, device="cuda")
    dm._set_optimizer(1e-3)
    dm.enable_ema(0.9)
    dm._train_one_batch(x0, ms2_cond=c2, ms1_cond=c1, sync=False)
    assert not torch.equal(dm.optimizer.ema_buffer(), tfm.flat_params)
    with torch.no_grad():
        outside = both(c1)
        with dm.ema_scope():
            inside = both(c1)
        assert not torch.equal(inside, outside)
        assert torch.equal(both(c1), outside)


@pytest.mark.parametrize("kw", KINDS, ids=["ddim", "stochastic", "solver_1", "solver_2m"])
def test_another_step_count_recaptures(kw):
    """the workspace is carved by num_steps, so the addresses a captured step bakes in move with it: 5 steps, then 3, then 5 on one model with the
    graph on, each against an eager call, bit for bit (the smaller workspace may well get the freed one's address)"""
    dm = _model("two_layers")
    dm.native_tfm_sampler = True
    xT, c2, c1 = (v.cuda() for v in _inputs("two_layers"))
    with torch.no_grad():
        dm.use_graph = False
        eager = {n: dm.sample(xT, c2, c1, num_steps=n, **kw) for n in (5, 3)}
        dm.use_graph = True
        for n in (5, 3, 5, 3):
            g = dm.sample(xT, c2, c1, num_steps=n, **kw)
            assert torch.equal(g[0], eager[n][0]) and torch.equal(g[1], eager[n][1]), n
    assert not torch.equal(eager[5][0], eager[3][0])


def test_stochastic_path():
    from dquartic import _native as N

    dm = _model("two_layers")
    xT, c2, c1 = (v.cuda() for v in _inputs("two_layers"))
    with torch.no_grad():
        a = dm.sample(xT, c2, c1, num_steps=4, eta=1.0, seed=7)
        b = dm.sample(xT, c2, c1, num_steps=4, eta=1.0, seed=7)
        c = dm.sample(xT, c2, c1, num_steps=4, eta=1.0, seed=8)
        assert dm.last_seed == 8
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
        assert torch.isfinite(a[0]).all()
        # x_t=None: x_T is draw 0 of the same generator
        drawn = torch.empty_like(xT)
        seed_dev = dm._seed_tensor(7, "cuda")
        N.check(N.lib().dq_randn(N.ptr(drawn), None, N.ptr(seed_dev), 0, xT.shape[0], xT[0].numel(), N.stream_ptr()), "dq_randn")
        for kw in (dict(eta=1.0), dict(), dict(sampler="dpmpp_2m")):
            n = dm.sample(None, c2, c1, num_steps=4, seed=7, **kw)
            e = dm.sample(drawn, c2, c1, num_steps=4, seed=7, **kw)
            assert torch.equal(n[0], e[0]) and torch.equal(n[1], e[1]), kw
        # eta = 0 ignores the seed
        dm.native_tfm_sampler = True
        plain = dm.sample(xT, c2, c1, num_steps=4)
        seeded = dm.sample(xT, c2, c1, num_steps=4, eta=0.0, seed=123)
        assert torch.equal(plain[0], seeded[0]) and torch.equal(plain[1], seeded[1])


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_noise_follows_the_window_id(use_graph):
    """output projection zeroed: the network returns exactly 0, every update is element-wise in x and the window's noise -- a window's result
    may then not depend on its place in the batch, bit for bit"""
    dm = _model("two_layers")
    dm.use_graph = use_graph
    tfm = dm.model.transformer
    with torch.no_grad():
        tfm._by_name["output_projection.weight"].zero_()
        tfm._by_name["output_projection.bias"].zero_()
    _, c2, c1 = (v.cuda() for v in _inputs("two_layers"))
    ids = torch.tensor([5, 9, 2])
    perm = torch.tensor([2, 0, 1])
    with torch.no_grad():
        a, _ = dm.sample(None, c2, c1, num_steps=4, eta=1.0, seed=21, window_ids=ids)
        b, _ = dm.sample(None, c2[perm], c1[perm], num_steps=4, eta=1.0, seed=21, window_ids=ids[perm])
        d, _ = dm.sample(None, c2, c1, num_steps=4, eta=1.0, seed=21)  # ids 0 .. B-1
    assert torch.equal(b, a[perm]) and torch.isfinite(a).all()
    assert not torch.equal(a[0], a[1]) and not torch.equal(a, d)


def test_predict_draws_end_to_end():
    dm = _model("two_layers")
    g = torch.Generator().manual_seed(3)
    loader = [tuple(torch.rand(2, 10, 64, generator=g) if k % 2 == 0 else torch.rand(2, 7, generator=g) for k in range(4)) for _ in range(2)]
    preds = dm.predict(loader, num_steps=3, eta=1.0, seed=7, n_draws=3, sampler="ddim")
    assert len(preds) == 2
    for d in preds:
        assert d["pred"].shape == (10, 64) and d["pred_mean"].shape == (10, 64) and d["pred_std"].shape == (10, 64)
        assert np.isfinite(d["pred_mean"]).all() and float(d["pred_std"].max()) > 0.0
    again = dm.predict(loader, num_steps=3, eta=1.0, seed=7, n_draws=1, sampler="ddim")
    assert np.array_equal(again[0]["pred"], preds[0]["pred"]) and "pred_std" not in again[0]


@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_default_call_is_the_generic_loop(pred):
    """native_tfm_sampler off, default arguments: the parent's loop, replayed here with p_sample, bit for bit"""
    dm = _model("two_layers", pred)
    assert dm.native_tfm_sampler is False
    xT, c2, c1 = (v.cuda() for v in _inputs("two_layers"))
    with torch.no_grad():
        got_x, got_n = dm.sample(xT, c2, c1, num_steps=5)
        ms2n, ms1n = dm.normalize(c2), dm.normalize(c1)
        x, e = xT, None
        for t in dm.sampler_timesteps(T, 5):
            x, e = dm.p_sample(x, int(t.item()), ms2n, ms1n)
        x = dm.unnormalize(x)
        n = dm.unnormalize(ms2n) - x
        dm.native_tfm_sampler = True
        nat_x, _ = dm.sample(xT, c2, c1, num_steps=5)
    assert torch.equal(got_x, x) and torch.equal(got_n, n)
    assert nat_x.shape == got_x.shape  # (the library's loop differs in the order of its sums: compared in test_native_loop_vs_float64)
