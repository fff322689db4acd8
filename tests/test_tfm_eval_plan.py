"""The host-only side of the CustomTransformer's held-out evaluation; no device is touched: the workspace size of
dq_tfm_eval_step, every refusal of the call (each returns before any HIP call, so dummy host pointers are safe), and the Python refusals of
eval_step / eval_steps on a network the library does not run."""
import ctypes
import re

import pytest
import torch


def _lib():
    from dquartic import _native as N

    return N.lib()


def test_eval_workspace_bytes():
    lib = _lib()
    tfm = lib.dq_tfm_create(64, 32, 2, 2)
    assert tfm
    try:
        ws = lib.dq_tfm_eval_workspace_bytes
        base = ws(tfm, 3, 10, 7, 2)
        assert base > 0 and base % 16 == 0
        # the inference buffers at the stacked batch are in it, and so are the L K | V buffers, x_t and the network output
        assert base >= lib.dq_tfm_workspace_bytes(tfm, 6, 10, 7, 0) + 4 * (2 * 6 * 17 * 64 + 2 * 6 * 10 * 64)
        assert ws(tfm, 4, 10, 7, 2) > base and ws(tfm, 3, 11, 7, 2) > base and ws(tfm, 3, 10, 8, 2) > base and ws(tfm, 3, 10, 7, 3) > base
        for k in range(4):
            grow = [ws(tfm, *[(v + d if i == k else v) for i, v in enumerate((3, 10, 7, 2))]) for d in (0, 1, 2, 5)]
            assert grow == sorted(grow) and len(set(grow)) == 4, (k, grow)
        one = lib.dq_tfm_create(64, 32, 2, 1)
        assert base - ws(one, 3, 10, 7, 2) >= 4 * 6 * 17 * 64  # one more layer: one more K | V buffer
        lib.dq_tfm_destroy(one)
        for bad in [(0, 10, 7, 2), (-1, 10, 7, 2), (3, 0, 7, 2), (3, 10, 0, 2), (3, 10, 7, 0), (3, 10, 7, -4), (256, 10, 7, 256), (65536, 10, 7, 1)]:
            assert ws(tfm, *bad) == 0, bad
        assert ws(None, 3, 10, 7, 2) == 0
        assert ws(tfm, 255, 1, 1, 257) > 0  # R * B = 65535: the last size admitted
    finally:
        lib.dq_tfm_destroy(tfm)


@pytest.mark.parametrize("cfg,shape,num_steps,repeats,expect", [
    ((64, 32, 2, 2), (3, 10, 7), 5, 3, (67300000, 67438336, 67355808, 67610160)),
    ((8, 16, 2, 1), (1, 1, 1), 1, 1, (67160192, 67161504, 67161296, 67160528))])
def test_workspace_bytes_are_pinned(cfg, shape, num_steps, repeats, expect):
    """The four size queries go through one carver: the byte counts are the ones the three separate carvers gave (inference, training,
    sampling, evaluation), read off the library before they were merged."""
    lib = _lib()
    tfm = lib.dq_tfm_create(*cfg)
    assert tfm
    try:
        got = (lib.dq_tfm_workspace_bytes(tfm, *shape, 0), lib.dq_tfm_workspace_bytes(tfm, *shape, 1),
               lib.dq_tfm_sample_workspace_bytes(tfm, *shape, num_steps), lib.dq_tfm_eval_workspace_bytes(tfm, *shape, repeats))
        assert got == expect
    finally:
        lib.dq_tfm_destroy(tfm)


class _Call:
    """dq_tfm_eval_step on dummy non-null HOST pointers: a call that passed its checks would fault, so every case here must be refused before
    anything touches the device."""

    def __init__(self):
        from dquartic import _native as N

        self.N, self.lib = N, N.lib()
        self.tfm = self.lib.dq_tfm_create(64, 32, 2, 2)
        assert self.tfm
        self.dummy = (ctypes.c_float * 64)()

    def close(self):
        self.lib.dq_tfm_destroy(self.tfm)

    def __call__(self, **kw):
        base = ctypes.addressof(self.dummy)
        base += (-base) % 16
        d = ctypes.c_void_p(base)
        a = dict(handle=True, params=d, sin=d, cos=d, freqs=d, ab=d, x0=d, ms1=d, t=d, noise=d, seed=d, ids=None, first_draw=0, norm=1, pred=0,
                 lw=d, loss=d, pw=d, net_out=None, ws=d, ws_bytes=1 << 40, B=3, S1=10, S2=7, R=2)
        a.update(kw)
        for k, v in a.items():
            if v == "odd":
                a[k] = ctypes.c_void_p(base + 4)
        rc = self.lib.dq_tfm_eval_step(self.tfm if a["handle"] else None, a["params"], a["sin"], a["cos"], a["freqs"], a["ab"], a["x0"], a["ms1"],
                                       a["t"], a["noise"], a["seed"], a["ids"], a["first_draw"], a["norm"], a["pred"], a["lw"], a["loss"], a["pw"],
                                       a["net_out"], a["ws"], a["ws_bytes"], a["B"], a["S1"], a["S2"], a["R"], None)
        return rc, self.N.last_error()


@pytest.fixture(scope="module")
def call():
    c = _Call()
    yield c
    c.close()


def _text(msg):
    """a refusal without the condition and the source line DQ_REQUIRE appends"""
    return re.sub(r" \[.*$", "", msg, flags=re.S)


REFUSALS = [(dict(**{k: (False if k == "handle" else None)}), "null argument")
            for k in ("handle", "params", "sin", "cos", "freqs", "ab", "x0", "ms1", "t", "loss", "pw", "ws")]
REFUSALS += [
    (dict(pred=2), "Unknown pred_type"),
    (dict(pred=-1), "Unknown pred_type"),
    (dict(pred=1, lw=None), "pred_type x0 needs the loss-weight (SNR) table"),
    (dict(B=0), "B, S1 and S2 must be positive"),
    (dict(S1=0), "B, S1 and S2 must be positive"),
    (dict(S2=-1), "B, S1 and S2 must be positive"),
    (dict(R=0), "repeats must be >= 1"),
    (dict(R=-2), "repeats must be >= 1"),
    (dict(B=256, R=256), "repeats * B must not exceed 65535"),
    (dict(B=65536, R=1), "repeats * B must not exceed 65535"),
    (dict(B=1 << 20, R=1 << 20), "repeats * B must not exceed 65535"),  # (no 32-bit overflow in the product)
    (dict(noise=None, seed=None), "a null noise needs the seed (device memory)"),
    (dict(first_draw=-1), "first_draw must be >= 0"),
    (dict(params="odd"), "params, workspace, x0, noise and net_out must be 16-byte aligned"),
    (dict(ws="odd"), "params, workspace, x0, noise and net_out must be 16-byte aligned"),
    (dict(x0="odd"), "params, workspace, x0, noise and net_out must be 16-byte aligned"),
    (dict(noise="odd"), "params, workspace, x0, noise and net_out must be 16-byte aligned"),
    (dict(net_out="odd"), "params, workspace, x0, noise and net_out must be 16-byte aligned"),
]


@pytest.mark.parametrize("kw,what", REFUSALS, ids=[f"{i}-{'-'.join(k)}" for i, (k, _) in enumerate(REFUSALS)])
def test_refusals(call, kw, what):
    rc, msg = call(**kw)
    assert rc != 0 and _text(msg) == "dq_tfm_eval_step: " + what, msg


def test_refuses_a_short_workspace(call):
    need = call.lib.dq_tfm_eval_workspace_bytes(call.tfm, 3, 10, 7, 2)
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=call.lib.dq_tfm_eval_workspace_bytes(call.tfm, 3, 10, 7, 1), R=2)):
        rc, msg = call(**kw)
        assert rc != 0 and "dq_tfm_eval_step: workspace too small (dq_tfm_eval_workspace_bytes)" in msg, msg
    # (ignored for eps: a null loss-weight table with the eps objective passes that check and is refused by the next one that fails)
    rc, msg = call(lw=None, ws_bytes=0)
    assert rc != 0 and "workspace too small" in msg


def test_stand_alone_kernels_refuse_before_a_launch(call):
    """dummy host pointers again: each of these returns before its launch"""
    N, lib, d = call.N, call.lib, ctypes.c_void_p(ctypes.addressof(call.dummy) + (-ctypes.addressof(call.dummy)) % 16)
    odd = ctypes.c_void_p(d.value + 4)
    q = lib.dq_q_sample_repeats
    for args, what in [((d, d, d, None, None, None, 0, d, 2, 2, 8, 1, None), "a null noise needs the seed"),
                       ((d, None, d, d, d, None, 0, d, 2, 2, 8, 1, None), "null argument"),
                       ((d, d, d, d, d, None, 0, d, 2, 2, 6, 1, None), "multiple of 4"),
                       ((d, d, d, d, d, None, 0, d, 2, 0, 8, 1, None), "multiple of 4"),
                       ((d, d, d, d, d, None, -1, d, 2, 2, 8, 1, None), "draw index"),
                       ((d, odd, d, d, d, None, 0, d, 2, 2, 8, 1, None), "16-byte aligned"),
                       ((d, d, d, d, d, None, 0, odd, 2, 2, 8, 1, None), "16-byte aligned")]:
        assert q(*args) != 0 and what in N.last_error(), (args, N.last_error())
    m = lib.dq_mse_per_window_repeats
    for args, what in [((d, None, 2, 1.0, 0.0, None, None, 0, None, None, d, d, d, 2, 2, 8, None), "a null target needs the seed"),
                       ((d, d, 3, 1.0, 0.0, None, None, 0, None, None, d, d, d, 2, 2, 8, None), "the target has B or repeats * B windows"),
                       ((d, d, 2, 1.0, 0.0, None, None, 0, d, None, d, d, d, 2, 2, 8, None), "the weighted form needs t"),
                       ((d, d, 2, 1.0, 0.0, None, None, 0, None, None, d, d, d, 256, 256, 8, None), "repeats * B <= 65535"),
                       ((None, d, 2, 1.0, 0.0, None, None, 0, None, None, d, d, d, 2, 2, 8, None), "null argument")]:
        assert m(*args) != 0 and what in N.last_error(), (args, N.last_error())
    k = lib.dq_tfm_kv_broadcast
    for args, what in [((None, 2, 2, 3, 5, 8, None), "null buffer"), ((odd, 2, 2, 3, 5, 8, None), "16-byte aligned"),
                       ((d, 2, 0, 3, 5, 8, None), "need B, repeats, S2 > 0"), ((d, 2, 2, 6, 5, 8, None), "Sk >= S2")]:
        assert k(*args) != 0 and what in N.last_error(), (args, N.last_error())
    assert k(d, 2, 1, 3, 5, 8, None) == 0  # one repeat: nothing to copy, no launch


def _adapter_model(**kw):
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    net = DDIMTransformerAdapter(CustomTransformer(input_dim=8, hidden_dim=8, num_heads=1, num_layers=1))
    return DDIMDiffusionModel(model_class=net, num_timesteps=20, device="cpu", **kw)


def test_python_refusals():
    from dquartic.model.model import DDIMDiffusionModel

    dm = DDIMDiffusionModel(model_class=torch.nn.Linear(4, 4), num_timesteps=20, device="cpu")
    x = torch.rand(1, 4, 4)
    with pytest.raises(NotImplementedError, match="native"):
        dm.eval_step(x, x, x[..., 0])
    with pytest.raises(NotImplementedError, match="native"):
        dm.eval_steps(x, x, x[..., 0], torch.zeros(2, 1, dtype=torch.long), torch.zeros(1, dtype=torch.int64), None)
    # the transformer behind its adapter is served, on the GPU only: host tensors are refused, never computed in torch
    tf = _adapter_model()
    x, c1 = torch.rand(2, 4, 8), torch.rand(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tf.eval_step(x, x, c1, t=torch.tensor([0, 19]), noise=torch.randn(2, 4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tf.eval_steps(x, x, c1, torch.zeros(2, 2, dtype=torch.long), torch.zeros(1, dtype=torch.int64), None)
    with pytest.raises(ValueError, match=r"t must be \(repeats, batch = 2\)"):
        tf.eval_steps(x, x, c1, torch.zeros(2, 3, dtype=torch.long), torch.zeros(1, dtype=torch.int64), None)
    with pytest.raises(ValueError, match="Unknown pred_type"):
        DDIMDiffusionModel(model_class=torch.nn.Linear(4, 4), num_timesteps=20, device="cpu", pred_type="v")


def test_eval_workspace_is_cached():
    from dquartic.model.building_blocks import CustomTransformer

    net = CustomTransformer(input_dim=8, hidden_dim=8, num_heads=1, num_layers=1)
    a = net.eval_workspace(2, 4, 3, 4)
    assert a.dtype == torch.uint8 and a.numel() == _lib().dq_tfm_eval_workspace_bytes(net._tfm, 2, 4, 3, 4)
    assert net.eval_workspace(2, 4, 3, 4) is a
    b = net.eval_workspace(2, 4, 3, 1)
    held = net.cached_workspaces()
    assert b is not a and net.eval_workspace(2, 4, 3, 1) is b and list(held) == ["eval"] and held["eval"] is b
    with pytest.raises(RuntimeError):
        net.eval_workspace(2, 4, 3, 0)
