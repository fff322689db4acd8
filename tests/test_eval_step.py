"""dq_mse_per_window (k_mse_per_window, csrc/k_stream.hip) and dq_eval_step, the forward-only counterpart of dq_train_step.

dq_mse_per_window runs at the loop edges of its own launch code (constants below): a slice of MSE_PW_SLICE elements -1 / exact / +1, a
block's 256-thread stride, two slices and a ragged third, and the finish kernel's 256 windows per stage; weighted and unweighted, with
`per` no multiple of 4.  Reference: float64 on the promoted fp32 inputs, target' = target * tm + ta formed in fp32 as the header says.
Bound (derived): the sums are fp64, so a result carries one fp32 rounding plus fp64 noise of at most n 2^-53 relative:
|out - ref| <= 2 * 2^-24 * |ref| + 1e-9 for per_window_out and loss_out alike.

dq_eval_step on UNet1d(dim=4, dim_mults=(1,2,2,3,3,4,4), downsample_dim=64) at B = 3, RT = 16 with t = (0, 999, 500): per_window_out
against the float64 MSE of dq_unet_fwd's no-save output on the same x_t (same bound), loss_out against dq_train_step's for the same t and
noise (1e-5 relative, the cap the older tests demand of the loss); it leaves the next train step bitwise alone, does not depend on the
batch, and reads the averaged weights inside ema_scope()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MSE_PW_SLICE = 8192    # dq_kernels.h: elements of a window one block of k_mse_per_window sums
T_ = 256               # k_mse_per_window: dim3(256), a thread takes every 256th element of its slice
FINISH_STAGE = 256     # k_mse_per_window_finish: 256 windows are staged at a time
U = 2.0 ** -24
HEAD, TAIL, CANARY = 64, 4096, 7251.0
CANARY_BITS = int(np.float32(CANARY).view(np.int32))
NUM_T = 1000

PER_EDGES = [1, T_ - 1, T_ + 1, MSE_PW_SLICE - 1, MSE_PW_SLICE, MSE_PW_SLICE + 1, 2 * MSE_PW_SLICE + 333]
B_EDGES = [FINISH_STAGE - 1, FINISH_STAGE, FINISH_STAGE + 1]


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


class Pad:
    def __init__(self, n):
        self.buf = torch.full((HEAD + n + TAIL,), CANARY, device="cuda")
        self.n = n
        self.view = self.buf[HEAD:HEAD + n]
        self.view.fill_(float("nan"))

    def intact(self):
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        return bool((bits[:HEAD] == CANARY_BITS).all()) and bool((bits[HEAD + self.n:] == CANARY_BITS).all())


def close(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    print(f"max |out - ref| / bound = {(np.abs(got - ref) / (2 * U * np.abs(ref) + 1e-9)).max():.3f}")
    return bool(np.all(np.abs(got - ref) <= 2 * U * np.abs(ref) + 1e-9))


def run_pw(N, out, target, tm, ta, lw, t):
    B, per = out.shape
    nbytes = 8 * B * cdiv(per, MSE_PW_SLICE)  # include/dq_hip.h: 8 * B * ceil(per / 8192) bytes
    assert N.lib().dq_mse_per_window_scratch_bytes(B, per) == nbytes
    pw, loss, scratch = Pad(B), Pad(1), Pad(nbytes // 4)
    o, z = torch.from_numpy(out).cuda(), torch.from_numpy(target).cuda()
    lw_d = None if lw is None else torch.from_numpy(lw).cuda()
    t_d = None if t is None else torch.from_numpy(t).cuda()
    N.check(N.lib().dq_mse_per_window(N.ptr(o), N.ptr(z), tm, ta, N.ptr(lw_d), N.ptr(t_d), N.ptr(pw.view), N.ptr(loss.view),
                                      N.ptr(scratch.view), B, per, N.stream_ptr()), "dq_mse_per_window")
    assert pw.intact() and loss.intact() and scratch.intact()
    return pw.view.cpu().numpy().copy(), float(loss.view.cpu()[0])


def pw_case(B, per, weighted, seed=0):
    rng = np.random.default_rng(17 * B + per + 5 * weighted + seed)
    out = rng.standard_normal((B, per)).astype(np.float32)
    target = rng.random((B, per), dtype=np.float32)
    tm, ta = (2.0, -1.0) if weighted else (1.0, 0.0)
    lw = (rng.random(NUM_T, dtype=np.float32) * 50 + np.float32(0.01)) if weighted else None
    t = rng.integers(0, NUM_T, size=B).astype(np.int64)
    t[0], t[-1] = 0, NUM_T - 1
    return out, target, tm, ta, lw, t


def pw_reference(out, target, tm, ta, lw, t):
    tp = (target * np.float32(tm)).astype(np.float32) + np.float32(ta)  # fp32: one multiply, one add
    d = out.astype(np.float64) - tp.astype(np.float64)
    pw = (d * d).mean(axis=1)
    w = np.ones(len(pw)) if lw is None else lw[t].astype(np.float64)
    return pw, float((w * pw).mean())


@pytest.mark.parametrize("weighted", [0, 1])
@pytest.mark.parametrize("B,per", [(3, p) for p in PER_EDGES] + [(b, 5) for b in B_EDGES] + [(1, 3 * 37 * 2)])
def test_mse_per_window(N, B, per, weighted):
    out, target, tm, ta, lw, t = pw_case(B, per, weighted)
    pw, loss = run_pw(N, out, target, tm, ta, lw, t)
    ref_pw, ref_loss = pw_reference(out, target, tm, ta, lw, t)
    assert close(pw, ref_pw)
    assert close(loss, ref_loss)


def test_mse_per_window_ignores_t_without_a_table_and_the_batch(N):
    out, target, tm, ta, lw, t = pw_case(3, 2 * MSE_PW_SLICE + 333, 1)
    pw3, _ = run_pw(N, out, target, tm, ta, None, None)
    for j in range(3):
        pw1, loss1 = run_pw(N, out[j:j + 1].copy(), target[j:j + 1].copy(), tm, ta, None, None)
        assert pw1.view(np.int32)[0] == pw3.view(np.int32)[j]
        assert np.float32(loss1).view(np.int32) == pw1.view(np.int32)[0]  # B = 1, weight 1: the same double rounded once


# ---- dq_eval_step -------------------------------------------------------------------------------------------------------------------

B_, RT_, MZ_ = 3, 16, 64
T_CASE = (0, 999, 500)


def make_dm(pred_type="eps", auto_normalize=True, pos_output_only=False, attn_cond_channels=1, seed=0):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1,
                 attn_cond_channels=attn_cond_channels, downsample_dim=MZ_, simple=True, pos_output_only=pos_output_only).cuda()
    return DDIMDiffusionModel(model_class=net, pred_type=pred_type, auto_normalize=auto_normalize, device="cuda")


def make_batch(M1=1, B=B_, seed=1):
    g = torch.Generator().manual_seed(seed)
    x0, c2 = torch.rand(B, RT_, MZ_, generator=g), torch.rand(B, RT_, MZ_, generator=g)
    c1 = torch.rand(B, RT_, generator=g) if M1 == 1 else torch.rand(B, RT_, M1, generator=g)
    nz = torch.randn(B, RT_, MZ_, generator=g)
    t = torch.tensor((T_CASE * B)[:B])
    return x0.cuda(), c2.cuda(), c1.cuda(), t.cuda(), nz.cuda()


CONFIGS = [(p, a, s, 1) for p in ("eps", "x0") for a in (True, False) for s in (False, True)] + [("eps", True, False, 3), ("x0", True, True, 3)]


@pytest.mark.parametrize("pred_type,auto_normalize,pos_output_only,M1", CONFIGS)
def test_eval_step_matches_the_forward_and_the_train_step(N, pred_type, auto_normalize, pos_output_only, M1):
    dm = make_dm(pred_type, auto_normalize, pos_output_only, M1)
    net = dm.model
    x0, c2, c1, t, nz = make_batch(M1)
    loss, pw = dm.eval_step(x0, c2, c1, t=t, noise=nz)
    assert loss.shape == () and pw.shape == (B_,) and loss.is_cuda and pw.is_cuda
    # the same x_t (dq_q_sample, the kernel the step launches), then dq_unet_fwd without anything saved, conditions mapped on the fly
    x_t = torch.empty_like(x0)
    N.check(N.lib().dq_q_sample(N.ptr(dm.alpha_bars), N.ptr(x0), N.ptr(t), N.ptr(nz), N.ptr(x_t), B_, RT_ * MZ_, int(auto_normalize),
                                N.stream_ptr()), "dq_q_sample")
    cm, ca = (2.0, -1.0) if auto_normalize else (1.0, 0.0)
    net._ensure_flat()
    with torch.no_grad():
        out = net._run_fwd(x_t, t, c2, net._check_inputs(c1, B_, RT_).contiguous(), training=False, cond_mul=cm, cond_add=ca)
    target = nz if pred_type == "eps" else x0 * cm + ca  # fp32: one multiply, one add
    ref_pw = ((out.double() - target.double()) ** 2).flatten(1).mean(dim=1).cpu().numpy()
    assert close(pw.cpu().numpy(), ref_pw)
    lw = dm.loss_weight.double().cpu().numpy()[t.cpu().numpy()]
    assert close(float(loss), float((lw * ref_pw).mean()))
    # ... and the train step's loss for the same t and noise
    train_loss = float(dm.train_step_fused(x0, c2, c1, t=t, noise=nz))
    print(f"eval loss {float(loss):.8g}, train loss {train_loss:.8g}")
    assert abs(float(loss) - train_loss) <= 1e-5 * abs(train_loss)


def test_eval_step_leaves_training_alone(N):
    x0, c2, c1, t, nz = make_batch()
    xe, c2e, c1e, te, nze = make_batch(seed=5)

    def two_steps(with_eval):
        dm = make_dm(seed=3)
        dm._set_lr(1e-3)
        first = dm.train_step_fused(x0, c2, c1, t=t, noise=nz)
        dm.optimizer.grad_scale = 1.0
        dm.optimizer.step()
        if with_eval:
            before = dm.model.flat_grads().clone()
            dm.eval_step(xe, c2e, c1e, t=te, noise=nze)
            torch.cuda.synchronize()
            assert torch.equal(before.view(torch.int32), dm.model.flat_grads().view(torch.int32))
        second = dm.train_step_fused(xe, c2e, c1e, t=te, noise=nze)
        torch.cuda.synchronize()
        return first.clone(), second.clone(), dm.model.flat_grads().clone()

    a, b = two_steps(False), two_steps(True)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_eval_step_needs_no_optimizer_and_sets_no_grad(N):
    dm = make_dm()
    x0, c2, c1, t, nz = make_batch()
    dm.eval_step(x0, c2, c1, t=t, noise=nz)
    assert dm.optimizer is None
    assert all(p.grad is None for p in dm.model.parameters())
    assert list(dm.model.cached_workspaces()) == ["infer"]  # the inference workspace only


def test_a_window_does_not_depend_on_its_batch(N):
    dm = make_dm()
    x0, c2, c1, t, nz = make_batch()
    _, pw3 = dm.eval_step(x0, c2, c1, t=t, noise=nz)
    pw3 = pw3.cpu()
    for j in range(B_):
        s = slice(j, j + 1)
        _, pw1 = dm.eval_step(x0[s], c2[s], c1[s], t=t[s], noise=nz[s])
        assert torch.equal(pw1.cpu().view(torch.int32), pw3[s].view(torch.int32)), j


def test_eval_step_reads_the_average_inside_ema_scope(N):
    dm, other = make_dm(seed=0), make_dm(seed=11)
    x0, c2, c1, t, nz = make_batch()
    dm._set_lr(1e-3)
    dm.enable_ema(0.99)
    with torch.no_grad():
        dm.optimizer.ema_buffer().copy_(other.model.flat_params)  # visibly different weights
    plain = dm.eval_step(x0, c2, c1, t=t, noise=nz)
    with dm.ema_scope():
        averaged = dm.eval_step(x0, c2, c1, t=t, noise=nz)
    expect = other.eval_step(x0, c2, c1, t=t, noise=nz)
    assert torch.equal(averaged[1].view(torch.int32), expect[1].view(torch.int32)) and torch.equal(averaged[0], expect[0])
    assert not torch.equal(averaged[1], plain[1])
    again = dm.eval_step(x0, c2, c1, t=t, noise=nz)
    assert torch.equal(again[1], plain[1])


def test_eval_step_is_native_only(N):
    from dquartic.model.model import DDIMDiffusionModel

    dm = DDIMDiffusionModel(model_class=torch.nn.Linear(4, 4).cuda(), device="cuda")
    x = torch.rand(1, 4, 4, device="cuda")
    with pytest.raises(NotImplementedError, match="native"):
        dm.eval_step(x, x, x[..., 0])
