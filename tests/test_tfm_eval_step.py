"""dq_tfm_eval_step, the CustomTransformer's held-out loss in one native call per batch, on the GPU.

Ground truth: oracle.dq_oracle_tfm.forward on float64 parameters (read-only use of the oracle) applied to the float64 x_t formed from the same
t and noise.  Yardstick: the path that exists without this feature, run per repeat on the same inputs -- dq_q_sample, dm.model(...) under
no_grad (dq_tfm_fwd), dq_mse_per_window.  Pass condition per case: the max-abs error of net_out against float64 is at most TWICE the
yardstick's on the same case, plus one fp32 ulp of the largest reference value -- the rule of tests/test_tfm_sample.py, for its reason: both
run the same fp32 arithmetic, what differs is the order of sums (the fused attention, the K | V rows projected per sample, GEMM plans that
follow the stacked row count).  per_window and loss are then covered by the bitwise tail claim: they equal dq_mse_per_window applied per
repeat to net_out[r] and its target.  Measured values: DESIGN.md section 31.

Shapes: the three configurations of tests/test_tfm_sample.py -- (64, 32, heads 2, layers 2) at B = 3, S1 = 10, S2 = 7; (64, 128, 1, 1) at S1 = 5,
S2 = 9; (64, 128, 1, 1) at B = 1, S1 = S2 = 77 (the three-launch attention) -- at R = 1 and 3, both objectives, auto_normalize on and off.

Bitwise claims: noise = NULL equals dq_randn's tensors stacked; two calls repeat; eval_step inside ema_scope() is the other weights' result;
a changed MS1 and parameters changed in place give what a fresh model gives; an eval_steps call between two train_step_fused calls, or between
a grad-enabled forward and its backward, changes neither.  NOT bitwise, and only bounded here: a window's value at another batch size."""
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


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


@functools.lru_cache(maxsize=None)
def _params(name):
    c = CFG[name]
    return OT.init_params(c["D"], c["H"], c["layers"], seed=11 + c["H"])


def _model(name, pred="eps", norm=True, params=None):
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    c = CFG[name]
    tf = CustomTransformer(input_dim=c["D"], hidden_dim=c["H"], num_heads=c["heads"], num_layers=c["layers"])
    tf.load_state_dict(_params(name) if params is None else params)
    return DDIMDiffusionModel(model_class=DDIMTransformerAdapter(tf).cuda(), num_timesteps=T, beta_schedule_type="cosine", pred_type=pred,
                              auto_normalize=norm, ms1_loss_weight=0.0, device="cuda")


@functools.lru_cache(maxsize=None)
def _inputs(name, R, B=None):
    """x0 (B, S1, D), ms1 (B, S2), t (R, B) with 0 and T-1 in it, noise (R, B, S1, D); host tensors"""
    c = CFG[name]
    B = c["B"] if B is None else B
    g = torch.Generator().manual_seed(5 + c["S1"] + R)
    x0, c1 = torch.rand(B, c["S1"], c["D"], generator=g), torch.rand(B, c["S2"], generator=g)
    t = torch.randint(0, T, (R, B), generator=g)
    t.view(-1)[0] = 0
    t.view(-1)[-1] = T - 1 if R * B > 1 else 0
    return x0, c1, t, torch.randn(R, B, c["S1"], c["D"], generator=g)


def _truth_for(dm, name, norm, x0, c1, t, nz):
    """float64: x_t from the model's own alpha-bar table, then the oracle's forward; (R, B, S1, D)"""
    c = CFG[name]
    p64 = {k: v.double() for k, v in _params(name).items()}
    ab = dm.alpha_bars.detach().cpu().double()
    xn = x0.double() * 2 - 1 if norm else x0.double()
    cn = c1.double() * 2 - 1 if norm else c1.double()
    outs = []
    with torch.no_grad():
        for r in range(t.shape[0]):
            a = ab[t[r]]
            x_t = a.sqrt()[:, None, None] * xn + (1 - a).sqrt()[:, None, None] * nz[r].double()
            outs.append(OT.forward(p64, x_t, t[r].double(), cn, c["heads"]))  # (a double t: float64 time features)
    return torch.stack(outs)


@functools.lru_cache(maxsize=None)
def _truth(name, norm, R):
    return _truth_for(_model(name, "eps", norm), name, norm, *_inputs(name, R))  # (the network output does not depend on the objective)


def _native(N, dm, x0, c1, t, noise=None, seed=None, ids=None, first_draw=0):
    """dq_tfm_eval_step with net_out: (loss (R), per_window (R, B), net_out (R, B, S1, D))"""
    tfm = dm.model.transformer
    B, S1, D = x0.shape
    S2, R = c1.shape[1], t.shape[0]
    flat = tfm.read_params(False)  # (first: it re-establishes the flat buffer on the device the module was moved to)
    ws = tfm.eval_workspace(B, S1, S2, R)
    assert ws.is_cuda and flat.is_cuda
    sin, cos, freqs = tfm.tables(max(S1, S2), x0.device)
    loss, pw = torch.full((R,), float("nan"), device="cuda"), torch.full((R, B), float("nan"), device="cuda")
    out = torch.full((R, B, S1, D), float("nan"), device="cuda")
    lw = dm.loss_weight.to(device="cuda", dtype=torch.float32).contiguous()
    N.check(N.lib().dq_tfm_eval_step(tfm._tfm, N.ptr(flat), N.ptr(sin), N.ptr(cos), N.ptr(freqs), N.ptr(dm.alpha_bars), N.ptr(x0),
                                     N.ptr(c1), N.ptr(t), N.ptr(noise), N.ptr(seed), N.ptr(ids), first_draw, int(dm.auto_normalize),
                                     N.PRED_TYPES[dm.pred_type], N.ptr(lw), N.ptr(loss), N.ptr(pw), N.ptr(out), N.ptr(ws), ws.numel(), B, S1, S2, R,
                                     N.stream_ptr()), "dq_tfm_eval_step")
    torch.cuda.synchronize()
    return loss, pw, out


def _per_window(N, dm, out, x0, t, nz):
    """dq_mse_per_window on one repeat's output and its target: what the tail must equal bit for bit"""
    B, per = out.shape[0], out[0].numel()
    pw, loss = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
    scratch = torch.empty(N.lib().dq_mse_per_window_scratch_bytes(B, per), dtype=torch.uint8, device="cuda")
    px0 = dm.pred_type == "x0"
    tm, ta = (2.0, -1.0) if (px0 and dm.auto_normalize) else (1.0, 0.0)
    lw = dm.loss_weight.to(device="cuda", dtype=torch.float32).contiguous() if px0 else None
    N.check(N.lib().dq_mse_per_window(N.ptr(out), N.ptr(x0 if px0 else nz), tm, ta, N.ptr(lw), N.ptr(t), N.ptr(pw), N.ptr(loss), N.ptr(scratch), B,
                                      per, N.stream_ptr()), "dq_mse_per_window")
    return loss[0], pw


def _yardstick(N, dm, x0, c1, t, nz):
    """per repeat: dq_q_sample, the network through dq_tfm_fwd, dq_mse_per_window"""
    outs, pws, losses = [], [], []
    B, per = x0.shape[0], x0[0].numel()
    with torch.no_grad():
        ms1n = dm.normalize(c1)
        for r in range(t.shape[0]):
            x_t = torch.empty_like(x0)
            N.check(N.lib().dq_q_sample(N.ptr(dm.alpha_bars), N.ptr(x0), N.ptr(t[r]), N.ptr(nz[r]), N.ptr(x_t), B, per, int(dm.auto_normalize),
                                        N.stream_ptr()), "dq_q_sample")
            out = dm.model(x_t, t[r], None, ms1n)
            loss, pw = _per_window(N, dm, out, x0, t[r], nz[r])
            outs.append(out), pws.append(pw), losses.append(loss)
    return torch.stack(losses), torch.stack(pws), torch.stack(outs)


def _err(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max())


def _bits(v):
    return v.contiguous().view(torch.int32)


CASES = [(name, R, pred, norm) for name in CFG for R in (1, 3) for pred in ("eps", "x0") for norm in (True, False)]


@pytest.mark.parametrize("name,R,pred,norm", CASES, ids=[f"{n}-R{r}-{p}-{'norm' if m else 'raw'}" for n, r, p, m in CASES])
def test_stacked_forward_vs_float64(N, name, R, pred, norm):
    c = CFG[name]
    assert N.lib().dq_tfm_attn_form(c["S1"], c["S1"] + c["S2"], c["H"] // c["heads"]) == (0 if name == "three_launch" else 1)
    dm = _model(name, pred, norm)
    x0, c1, t, nz = (v.cuda() for v in _inputs(name, R))
    ref = _truth(name, norm, R)
    y_loss, y_pw, y_out = _yardstick(N, dm, x0, c1, t, nz)
    loss, pw, out = _native(N, dm, x0, c1, t, noise=nz)
    e_nat, e_yard = _err(out, ref), _err(y_out, ref)
    ulp = float(np.spacing(np.float32(ref.abs().max())))
    print(f"tfm_eval {name} R={R} {pred} norm={norm}: native={e_nat:.3e} yardstick={e_yard:.3e} max|ref|={float(ref.abs().max()):.3e} "
          f"loss native={loss.tolist()} yardstick={y_loss.tolist()}")
    assert torch.isfinite(out).all() and torch.isfinite(pw).all() and torch.isfinite(loss).all()
    assert e_nat <= 2.0 * e_yard + ulp, (e_nat, e_yard, ulp)
    # the tail, bit for bit: dq_mse_per_window on each repeat of the call's own network output
    for r in range(R):
        l_r, pw_r = _per_window(N, dm, out[r], x0, t[r], nz[r])
        assert torch.equal(_bits(pw[r]), _bits(pw_r)) and torch.equal(_bits(loss[r]), _bits(l_r)), r
    # the Python entry returns the same numbers and never materialises the network output
    if R == 1:
        l1, p1 = dm.eval_step(x0, None, c1, t=t[0], noise=nz[0])
        assert l1.shape == () and p1.shape == (c["B"],) and torch.equal(_bits(l1), _bits(loss[0])) and torch.equal(_bits(p1), _bits(pw[0]))
        l3, p3 = dm.eval_step(x0, None, c1[..., None], t=t[0], noise=nz[0])  # ms1_cond (B, RT, 1)
        assert torch.equal(_bits(p3), _bits(p1)) and torch.equal(_bits(l3), _bits(l1))


@pytest.mark.parametrize("pred", ["eps", "x0"])
@pytest.mark.parametrize("name,R", [("two_layers", 3), ("wide_head", 1), ("three_launch", 3)])
def test_drawn_noise_is_dq_randn_and_calls_repeat(N, name, R, pred):
    c = CFG[name]
    dm = _model(name, pred)
    x0, c1, t, _ = (v.cuda() for v in _inputs(name, R))
    seed = dm._seed_tensor(1234567, "cuda")
    ids = torch.tensor([17, 3, 1 << 35][:c["B"]], dtype=torch.int64, device="cuda")
    first = 2
    z = torch.empty(R, *x0.shape, device="cuda")
    for r in range(R):
        N.check(N.lib().dq_randn(N.ptr(z[r]), N.ptr(ids), N.ptr(seed), first + r, c["B"], x0[0].numel(), N.stream_ptr()), "dq_randn")
    a = _native(N, dm, x0, c1, t, noise=z)
    b = _native(N, dm, x0, c1, t, seed=seed, ids=ids, first_draw=first)
    again = _native(N, dm, x0, c1, t, seed=seed, ids=ids, first_draw=first)
    for u, v, w in zip(a, b, again):
        assert torch.equal(_bits(u), _bits(v)) and torch.equal(_bits(v), _bits(w))
    other = _native(N, dm, x0, c1, t, seed=seed, ids=ids, first_draw=first + 1)
    assert not torch.equal(other[1], b[1])
    # eval_steps is that call
    loss, pw = dm.eval_steps(x0, None, c1, t, seed, ids, first_draw=first)
    assert loss.shape == (R,) and pw.shape == (R, c["B"])
    assert torch.equal(_bits(loss), _bits(b[0])) and torch.equal(_bits(pw), _bits(b[1]))
    # default window ids are 0 .. B-1
    d0 = dm.eval_steps(x0, None, c1, t, seed, None)
    d1 = dm.eval_steps(x0, None, c1, t, seed, torch.arange(c["B"], device="cuda"))
    assert torch.equal(_bits(d0[1]), _bits(d1[1]))


def test_eval_step_reads_the_average_inside_ema_scope(N):
    other_params = OT.init_params(64, 32, 2, seed=99)
    dm, other = _model("two_layers"), _model("two_layers", params=other_params)
    x0, c1, t, nz = (v.cuda() for v in _inputs("two_layers", 1))
    dm._set_lr(1e-3)
    dm.enable_ema(0.99)
    with torch.no_grad():
        dm.optimizer.ema_buffer().copy_(other.model.flat_params)  # visibly different weights
    plain = dm.eval_step(x0, None, c1, t=t[0], noise=nz[0])
    with dm.ema_scope():
        averaged = dm.eval_step(x0, None, c1, t=t[0], noise=nz[0])
    expect = other.eval_step(x0, None, c1, t=t[0], noise=nz[0])
    assert torch.equal(_bits(averaged[1]), _bits(expect[1])) and torch.equal(averaged[0], expect[0])
    assert not torch.equal(averaged[1], plain[1])
    again = dm.eval_step(x0, None, c1, t=t[0], noise=nz[0])
    assert torch.equal(_bits(again[1]), _bits(plain[1]))


def test_needs_no_optimizer_and_sets_no_grad(N):
    dm = _model("two_layers", "x0")
    x0, c1, t, nz = (v.cuda() for v in _inputs("two_layers", 3))
    tfm = dm.model.transformer
    assert torch.is_grad_enabled()
    loss, pw = dm.eval_steps(x0, None, c1, t, dm._seed_tensor(5, "cuda"), None)
    l1, p1 = dm.eval_step(x0, None, c1)  # t and noise drawn from torch's generator
    assert not loss.requires_grad and not pw.requires_grad and torch.isfinite(l1) and p1.shape == (3,)
    assert dm.optimizer is None and all(p.grad is None for p in dm.model.parameters())
    assert "train" not in tfm.cached_workspaces() and not tfm._ws_pool  # no training workspace came into being


def test_no_stale_state(N):
    """nothing is cached across calls: a changed MS1 and weights changed in place behind the same pointer give what a fresh model gives"""
    dm = _model("two_layers")
    tfm = dm.model.transformer
    x0, c1, t, nz = (v.cuda() for v in _inputs("two_layers", 3))
    c1b = torch.flip(c1, dims=[1]).contiguous() * 0.5
    seed = dm._seed_tensor(8, "cuda")
    a = dm.eval_steps(x0, None, c1, t, seed, None)
    b = dm.eval_steps(x0, None, c1b, t, seed, None)
    assert not torch.equal(a[1], b[1])
    fresh = _model("two_layers").eval_steps(x0, None, c1b, t, seed, None)
    assert torch.equal(_bits(b[1]), _bits(fresh[1])) and torch.equal(_bits(b[0]), _bits(fresh[0]))
    assert torch.equal(_bits(dm.eval_steps(x0, None, c1, t, seed, None)[1]), _bits(a[1]))
    ptr, ws = tfm.flat_params.data_ptr(), tfm.eval_workspace(3, 10, 7, 3).data_ptr()
    with torch.no_grad():
        tfm.flat_params.mul_(1.25)
    assert tfm.flat_params.data_ptr() == ptr
    c = dm.eval_steps(x0, None, c1, t, seed, None)
    assert tfm.eval_workspace(3, 10, 7, 3).data_ptr() == ws and not torch.equal(c[1], a[1])
    scaled = {k: v * 1.25 for k, v in _params("two_layers").items()}
    fresh = _model("two_layers", params=scaled).eval_steps(x0, None, c1, t, seed, None)
    assert torch.equal(_bits(c[1]), _bits(fresh[1])) and torch.equal(_bits(c[0]), _bits(fresh[0]))


def test_eval_steps_leaves_the_train_step_alone(N):
    x0, c1, t, nz = (v.cuda() for v in _inputs("two_layers", 1))
    xe, c1e, te, nze = (v.cuda() for v in _inputs("two_layers", 3))
    c2 = torch.zeros_like(x0)

    def two_steps(with_eval):
        dm = _model("two_layers")
        first = dm.train_step_fused(x0, c2, c1, t=t[0], noise=nz[0])
        if with_eval:
            before = dm.model.flat_grads().clone()
            dm.eval_steps(xe, None, c1e, te, dm._seed_tensor(3, "cuda"), None)
            dm.eval_step(x0, None, c1, t=t[0], noise=nz[0])  # the train step's own shape
            torch.cuda.synchronize()
            assert torch.equal(_bits(before), _bits(dm.model.flat_grads()))
        second = dm.train_step_fused(xe, c2, c1e, t=te[1], noise=nze[1])
        torch.cuda.synchronize()
        return first.clone(), second.clone(), dm.model.flat_grads().clone()

    for u, v in zip(two_steps(False), two_steps(True)):
        assert torch.equal(_bits(u), _bits(v))


def test_eval_steps_between_a_forward_and_its_backward(N):
    """the autograd bridge keeps its forward's activations in a training workspace until the backward: an evaluation in between reads none
    of it and writes none of it"""
    x0, c1, t, nz = (v.cuda() for v in _inputs("two_layers", 3))
    g = torch.Generator().manual_seed(4)
    gout = torch.randn(3, 10, 64, generator=g).cuda()

    def run(with_eval):
        dm = _model("two_layers")
        tfm = dm.model.transformer
        out = dm.model(x0, t[0], None, c1)
        assert out.requires_grad
        if with_eval:
            dm.eval_steps(x0, None, c1, t, dm._seed_tensor(3, "cuda"), None)
            dm.eval_step(x0, None, c1, t=t[0], noise=nz[0])
        out.backward(gout)
        torch.cuda.synchronize()
        return out.detach().clone(), torch.cat([p.grad.reshape(-1) for _, p in tfm.trainable_named()])

    (o_a, g_a), (o_b, g_b) = run(False), run(True)
    assert torch.equal(_bits(o_a), _bits(o_b)) and torch.equal(_bits(g_a), _bits(g_b)) and float(g_a.abs().max()) > 0


@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_another_batch_size_agrees_to_rounding(N, pred):
    """B = 2 against B = 1, per window: the GEMM plans follow the row count, so this is NOT bitwise -- each stays within the yardstick rule"""
    name, R, B = "two_layers", 2, 2
    dm = _model(name, pred)
    x0h, c1h, th, nzh = _inputs(name, R, B)
    ref = _truth_for(dm, name, True, x0h, c1h, th, nzh)
    x0, c1, t, nz = (v.cuda() for v in (x0h, c1h, th, nzh))
    _, pw2, out2 = _native(N, dm, x0, c1, t, noise=nz)
    _, _, y_out = _yardstick(N, dm, x0, c1, t, nz)
    for b in range(B):
        s = slice(b, b + 1)
        _, pw1, out1 = _native(N, dm, x0[s].contiguous(), c1[s].contiguous(), t[:, s].contiguous(), noise=nz[:, s].contiguous())
        e2, e1, e_yard = _err(out2[:, s], ref[:, s]), _err(out1, ref[:, s]), _err(y_out[:, s], ref[:, s])
        ulp = float(np.spacing(np.float32(ref[:, s].abs().max())))
        rel = float(((pw2[:, s] - pw1).abs() / pw1.abs()).max())
        print(f"tfm_eval window {b} {pred}: B=2 {e2:.3e} B=1 {e1:.3e} yardstick {e_yard:.3e}; per_window B=2 vs B=1 rel {rel:.3e} "
              f"bitwise={torch.equal(_bits(pw2[:, s]), _bits(pw1))}")
        assert e2 <= 2.0 * e_yard + ulp and e1 <= 2.0 * e_yard + ulp, (e2, e1, e_yard, ulp)
