"""The one sampling loop under both networks (csrc/dq_sampler.h: replay_captured_step, eager_steps).

The U-Net's and the transformer's entry run the same capture function, each over the StepGraph of its own handle.  What the other sampling
tests do not see is the two in one process, one after the other:
  * graph calls of the two networks interleaved, every one bit for bit the eager call (use_graph = False) of its setting on its model;
  * a handle destroyed with a live graph and capture stream, and the same model built again from the same seed: the same result.
Models: test_stochastic_sampler's U-Net at batch 2 and test_tfm_sample's "two_layers" transformer, 3 steps each.

Without a GPU: which entry ``DDIMDiffusionModel._sample_native`` reaches for (eta, sampler), over a recorder in place of the library -- the
three take one argument list (the first 22 arguments), which is what lets test_sample_ex_eta0_is_dq_ddim_sample compare two entries."""
import ctypes
import gc

import pytest
import torch

gpu = pytest.mark.gpu
STEPS = 3


def _unet(pred):
    from test_stochastic_sampler import _model

    dm, _, xT, c2, c1 = _model(pred)
    return dm, (xT[:2].cuda(), c2[:2].cuda(), c1[:2].cuda())


def _tfm():
    import test_tfm_sample as TS

    dm = TS._model("two_layers")
    dm.native_tfm_sampler = True
    return dm, tuple(v.cuda() for v in TS._inputs("two_layers"))


def _sample(dm, inputs, graph, **kw):
    dm.use_graph = graph
    try:
        with torch.no_grad():
            return dm.sample(*inputs, num_steps=STEPS, **kw)
    finally:
        dm.use_graph = True


@gpu
@pytest.mark.parametrize("pred", ["eps", "x0"])
def test_interleaved_graph_calls(pred):
    """U-Net, transformer, U-Net (another seed, eta = 0.5), transformer (dpmpp_2m), U-Net (the first setting): each handle recaptures or
    replays the step of ITS setting, whatever the other has captured in between; then both once more, the U-Net's a pure replay"""
    unet, tfm = _unet(pred), _tfm()
    u_first, u_sto, t_first, t_2m = dict(seed=11), dict(seed=12, eta=0.5), dict(), dict(sampler="dpmpp_2m")
    order = [(unet, u_first), (tfm, t_first), (unet, u_sto), (tfm, t_2m), (unet, u_first), (tfm, t_first), (unet, u_first)]
    eager = [_sample(*net, False, **kw) for net, kw in order[:4]]
    eager += [eager[0], eager[1], eager[0]]
    assert not torch.equal(eager[0][0], eager[2][0]) and not torch.equal(eager[1][0], eager[3][0])  # (the settings differ in their result)
    for i, ((net, kw), want) in enumerate(zip(order, eager)):
        got = _sample(*net, True, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (i, kw)


@gpu
def test_handles_die_with_a_live_graph():
    """sample with the graph, destroy the handle (dq_plan_destroy / dq_tfm_destroy with a captured step and its capture stream alive), build the
    same model from the same seed, sample with the graph: the same bits"""
    import test_stochastic_sampler as SS
    from dquartic.model.model import DDIMDiffusionModel

    def unet():
        net, _ = SS._net(31)
        dm = DDIMDiffusionModel(model_class=net.cuda(), pred_type="eps", device="cuda")
        net.eval()
        return dm, _unet("eps")[1]

    for build, kw in ((unet, dict(seed=11, eta=0.5)), (_tfm, dict(sampler="dpmpp_2m"))):
        dm, inputs = build()
        first = _sample(dm, inputs, True, **kw)
        del dm
        gc.collect()
        dm, inputs = build()
        again = _sample(dm, inputs, True, **kw)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        assert torch.isfinite(first[0]).all()


class _Recorder:
    """stands in for the library: a sampling entry returns 0 and leaves its name and arguments.  Anything else is a handle of an earlier test
    that the collector frees meanwhile: that goes to the library the handle came from"""

    def __init__(self, real):
        self.calls, self.real = [], real

    def __getattr__(self, name):
        if not name.startswith("dq_ddim_sample"):
            return getattr(self.real(), name)
        return lambda *args: self.calls.append((name, args)) or 0


def _plain(v):
    if isinstance(v, ctypes.c_void_p):
        return ("ptr", v.value)
    if isinstance(v, ctypes.Array):
        return (type(v)._type_, list(v))
    return v


def test_entry_choice(monkeypatch):
    """eta=None -> dq_ddim_sample, eta=0.0 -> dq_ddim_sample_ex (+ eta, seed, ids), sampler=1 -> dq_ddim_sample_solver (+ sampler, clip_x0);
    the first 22 arguments of the three calls are the same"""
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel

    rec = _Recorder(N.lib)
    monkeypatch.setattr(N, "lib", lambda: rec)
    monkeypatch.setattr(N, "stream_ptr", lambda: ctypes.c_void_p(0x5EED))
    B, RT, MZ = 2, 4, 8
    g = torch.Generator().manual_seed(3)
    flat, ws, rope = torch.rand(16, generator=g), torch.empty(64), torch.rand(4, generator=g)
    net = torch.nn.Identity()  # (what _sample_native asks of UNet1d, over host tensors)
    net._plan = ctypes.c_void_p(0xABC0)
    net._check_inputs = lambda c, b, rt: c[..., None]
    net.read_params, net.rope_freqs, net.workspace = (lambda: flat), (lambda: rope), (lambda b, rt, training: ws)
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=50, pred_type="x0", device="cpu")
    xT, c2, c1 = torch.randn(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    keep = []  # (outputs stay alive, so that no two calls' buffers share an address by reuse)
    keep.append(dm._sample_native(xT, c2, c1, STEPS))
    keep.append(dm._sample_native(xT, c2, c1, STEPS, eta=0.0))
    keep.append(dm._sample_native(xT, c2, c1, STEPS, eta=0.0, sampler=1, clip_x0=1.5))
    assert [name for name, _ in rec.calls] == ["dq_ddim_sample", "dq_ddim_sample_ex", "dq_ddim_sample_solver"]
    a0, a1, a2 = (args for _, args in rec.calls)
    assert (len(a0), len(a1), len(a2)) == (22, 25, 27)
    assert [_plain(v) for v in a1[22:]] == [0.0, None, None] and [_plain(v) for v in a2[22:]] == [0.0, None, None, 1, 1.5]
    # the shared list: what the caller owns is the same object or address in all three, what a call allocates (out_x, out_noise) differs
    own = [i for i in range(22) if i not in (12, 13)]
    for other in (a1, a2):
        assert [_plain(other[i]) for i in own] == [_plain(a0[i]) for i in own]
        assert other[0] is a0[0] and other[3] is a0[3]  # the plan handle, the host schedule
    want = [("ptr", 0xABC0), ("ptr", flat.data_ptr()), ("ptr", rope.data_ptr()), None, 50, ("ptr", xT.data_ptr()), ("ptr", c2.data_ptr()), None,
            1, N.PRED_TYPES["x0"], (ctypes.c_int32, [49, 24, 0]), STEPS, None, None, None, None, 1, ("ptr", ws.data_ptr()), ws.numel(), B, RT,
            ("ptr", 0x5EED)]
    for i, w in enumerate(want):
        if w is not None:
            assert _plain(a0[i]) == w, i
    for (x, n), args in zip(keep, (a0, a1, a2)):
        assert (args[12].value, args[13].value) == (x.data_ptr(), n.data_ptr()) and args[14] is None and args[15] is None
    # return_trajectory: the trajectories go in, the graph flag goes off
    x, n, tx, te = dm._sample_native(xT, c2, c1, STEPS, True, eta=0.0)
    args = rec.calls[-1][1]
    assert (args[14].value, args[15].value, args[16]) == (tx.data_ptr(), te.data_ptr(), 0) and tx.shape == (STEPS, B, RT, MZ) == te.shape
