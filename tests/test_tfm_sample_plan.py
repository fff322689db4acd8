"""The host-only side of the CustomTransformer's native sampler; no device is touched: the attention form query, the
sampling workspace size, every refusal of dq_tfm_sample (worded like dq_ddim_sample's, which refuses the same calls), the Python
argument checks of sample() on the adapter, and the config key that switches the sampler on."""
import ctypes
import re

import pytest
import torch


def _lib():
    from dquartic import _native as N

    return N.lib()


def _lds_bytes(Sk, dh):
    """include/dq_hip.h: K (pitch dh + 4), V, and four waves' q and p rows"""
    return 4 * (Sk * (2 * dh + 4) + 4 * dh + 4 * ((Sk + 3) & ~3))


def test_attention_form_query():
    form = _lib().dq_tfm_attn_form
    # the shapes of tests/test_tfm_attn.py: (S1, Sk, dh)
    for S1, Sk, dh in [(1, 2, 4), (5, 8, 16), (7, 13, 32), (17, 33, 16), (33, 65, 32), (34, 68, 128)]:
        assert form(S1, Sk, dh) == 1, (S1, Sk, dh)
    # every Sk <= 68 at every head width the handle can have up to 128
    for Sk in range(1, 69):
        for dh in range(4, 129, 4):
            assert form(max(1, Sk - 1), Sk, dh) == 1, (Sk, dh)
    # the one bound: LDS bytes <= 160 KiB
    assert _lds_bytes(153, 128) <= 160 * 1024 < _lds_bytes(154, 128)
    assert form(77, 153, 128) == 1 and form(77, 154, 128) == 0
    assert _lds_bytes(2558, 4) <= 160 * 1024 < _lds_bytes(2559, 4)
    assert form(3, 2558, 4) == 1 and form(3, 2559, 4) == 0
    for Sk in (1, 50, 200, 1000, 5000):
        for dh in (4, 8, 64, 128, 256, 512):
            assert form(1, Sk, dh) == int(_lds_bytes(Sk, dh) <= 160 * 1024), (Sk, dh)
    # a head width that is no multiple of 4 has no vector rows: three launches; non-positive sizes: -1
    assert form(4, 8, 6) == 0 and form(4, 8, 130) == 0
    assert form(0, 8, 4) == -1 and form(4, 0, 4) == -1 and form(4, 8, 0) == -1


def test_sample_workspace_bytes():
    lib = _lib()
    tfm = lib.dq_tfm_create(64, 32, 2, 2)
    assert tfm
    try:
        ws = lib.dq_tfm_sample_workspace_bytes
        base = ws(tfm, 3, 10, 7, 5)
        assert base > 0 and base % 16 == 0
        assert base >= lib.dq_tfm_workspace_bytes(tfm, 3, 10, 7, 0)
        assert ws(tfm, 4, 10, 7, 5) > base and ws(tfm, 3, 10, 7, 6) >= base and ws(tfm, 3, 10, 7, 50) > base
        assert [ws(tfm, b, 10, 7, 5) for b in (1, 2, 3, 8)] == sorted(ws(tfm, b, 10, 7, 5) for b in (1, 2, 3, 8))
        assert [ws(tfm, 3, 10, 7, n) for n in (1, 2, 9, 1024)] == sorted(ws(tfm, 3, 10, 7, n) for n in (1, 2, 9, 1024))
        # the L persistent K | V buffers are in it
        one = lib.dq_tfm_create(64, 32, 2, 1)
        assert base - ws(one, 3, 10, 7, 5) >= 4 * 3 * 17 * 64
        lib.dq_tfm_destroy(one)
        for bad in [(0, 10, 7, 5), (3, 0, 7, 5), (3, 10, 0, 5), (3, 10, 7, 0), (3, 10, 7, 1025)]:
            assert ws(tfm, *bad) == 0
        assert ws(None, 3, 10, 7, 5) == 0
    finally:
        lib.dq_tfm_destroy(tfm)


class _Call:
    """dq_tfm_sample / dq_ddim_sample on one record of dummy non-null HOST pointers: a call that passed its checks would fault, so every case here
    must be refused before anything touches the device."""

    def __init__(self):
        from dquartic import _native as N

        self.N, self.lib = N, N.lib()
        self.tfm = self.lib.dq_tfm_create(64, 32, 2, 2)
        mults = (ctypes.c_int * 2)(1, 2)
        self.plan = self.lib.dq_plan_create(4, 2, mults, 64, 1000)
        assert self.tfm and self.plan
        self.dummy = (ctypes.c_float * 64)()
        self.ab = (ctypes.c_float * 1000)(*[0.999 ** (i + 1) for i in range(1000)])

    def close(self):
        self.lib.dq_tfm_destroy(self.tfm)
        self.lib.dq_plan_destroy(self.plan)

    def args(self, **kw):
        d = ctypes.cast(self.dummy, ctypes.c_void_p)
        a = dict(handle=True, params=d, x_T=d, ms2=d, ms1=d, pred=0, ts=[999, 500, 0], num_steps=None, out=d, ws=d, ws_bytes=1 << 40, B=3, S1=10, S2=7,
                 eta=0.0, seed=d, sampler=0, clip=0.0, T=1000)
        a.update(kw)
        if a["num_steps"] is None:
            a["num_steps"] = len(a["ts"])
        a["ts_c"] = (ctypes.c_int32 * max(1, len(a["ts"])))(*a["ts"])
        ptr = lambda v: None if v is None else v.value  # noqa: E731
        fields = dict(alpha_bars_host=ctypes.addressof(self.ab), num_timesteps=a["T"], x_T=ptr(a["x_T"]), ms2_cond=ptr(a["ms2"]),
                      ms1_cond=ptr(a["ms1"]), auto_normalize=1, pred_type=a["pred"], timesteps_host=ctypes.addressof(a["ts_c"]),
                      out_x=ptr(a["out"]), out_noise=d.value, use_graph=1, workspace=ptr(a["ws"]), workspace_bytes=a["ws_bytes"],
                      clip_x0=a["clip"], seed_dev=ptr(a["seed"]))
        fields.update({k: a[k] for k, _ in self.N.SampleCall._fields_ if k in a})  # (the keywords that are the record's own names)
        q = self.N.sample_call(**fields)
        return a, d, q

    def tfm_sample(self, **kw):
        a, d, q = self.args(**kw)
        q.RT = a["S1"]
        rc = self.lib.dq_tfm_sample(self.tfm if a["handle"] else None, a["params"], d, d, d, a["S2"], ctypes.byref(q))
        return rc, self.N.last_error()

    def unet_sample(self, **kw):
        a, d, q = self.args(**kw)
        q.RT = 16
        rc = self.lib.dq_ddim_sample(self.plan if a["handle"] else None, a["params"], d, ctypes.byref(q))
        return rc, self.N.last_error()


@pytest.fixture(scope="module")
def call():
    c = _Call()
    yield c
    c.close()


def _text(msg):
    """a refusal without the condition and the source line DQ_REQUIRE appends"""
    return re.sub(r" \[.*$", "", msg, flags=re.S)


SHARED_REFUSALS = [  # (keyword arguments, the message behind the function name)
    (dict(handle=False), "null argument"),
    (dict(params=None), "null argument"),
    (dict(ms2=None), "null argument"),
    (dict(ms1=None), "null argument"),
    (dict(out=None), "null argument"),
    (dict(ws=None), "null argument"),
    (dict(eta=-0.25), "eta must satisfy 0 <= eta <= 1"),
    (dict(eta=1.5), "eta must satisfy 0 <= eta <= 1"),
    (dict(eta=float("nan")), "eta must satisfy 0 <= eta <= 1"),
    (dict(sampler=3), "unknown sampler"),
    (dict(sampler=-1), "unknown sampler"),
    (dict(sampler=2, eta=0.5), "DPM-Solver++(2M) is deterministic: eta must be 0"),
    (dict(sampler=0, clip=1.0), "clip_x0 needs the ddim or dpmpp_2m sampler"),
    (dict(sampler=1, clip=1.0, eta=0.5), "clip_x0 needs eta == 0"),
    (dict(sampler=1, ts=[999, 500, 500]), "the timesteps of this sampler must be strictly decreasing"),
    (dict(sampler=2, ts=[10, 500, 0]), "the timesteps of this sampler must be strictly decreasing"),
    (dict(pred=3), "Unknown pred_type"),  # (DQ_PRED_V = 2 is the U-Net's objective, not the transformer's: test_v_is_the_unets_objective_alone)
    (dict(eta=0.5, seed=None), "eta > 0 and a null x_T need the seed (device memory)"),
    (dict(x_T=None, seed=None), "eta > 0 and a null x_T need the seed (device memory)"),
]


@pytest.mark.parametrize("kw,what", SHARED_REFUSALS, ids=[f"{i}-{w[:24]}" for i, (_, w) in enumerate(SHARED_REFUSALS)])
def test_refusals_worded_like_the_unet_loop(call, kw, what):
    rc, msg = call.tfm_sample(**kw)
    assert rc != 0 and _text(msg) == "dq_tfm_sample: " + what, msg
    rc_u, msg_u = call.unet_sample(**kw)
    assert rc_u != 0 and _text(msg_u) == "dq_ddim_sample: " + what, msg_u  # the same wording apart from the function name


def test_v_is_the_unets_objective_alone(call):
    """the transformer's entry refuses DQ_PRED_V as unknown; the U-Net's takes it: the same record gets to the refusal behind the objective"""
    rc, msg = call.tfm_sample(pred=2)
    assert rc != 0 and _text(msg) == "dq_tfm_sample: Unknown pred_type", msg
    rc, msg = call.unet_sample(pred=2, B=0)
    assert rc != 0 and _text(msg) == "dq_ddim_sample: need B, RT > 0 and 1 <= num_steps <= 1024", msg


NOT_THE_TRANSFORMERS = [  # what the record can say and dq_tfm_sample is not built for: refused by name, never ignored
    (dict(guided=1, guidance_scale=2.0), "guided sampling is built for the U-Net (dq_ddim_sample); guidance for this network is the follow-up"),
    (dict(guidance_rescale=0.5), "guidance_rescale and threshold_quantile are built for the U-Net (dq_ddim_sample); the per-window statistics step for "
                                 "this network is the follow-up"),
    (dict(sampler=1, threshold_quantile=0.5, threshold_max=2.0, stat_scratch=4096, stat_scratch_bytes=1 << 30),
     "guidance_rescale and threshold_quantile are built for the U-Net (dq_ddim_sample); the per-window statistics step for this network is the "
     "follow-up"),
    (dict(consistency=1, group_size=3), "consistency is built for the U-Net (dq_ddim_sample); the group pass for this network is the follow-up"),
]


@pytest.mark.parametrize("kw,what", NOT_THE_TRANSFORMERS, ids=["guided", "rescale", "threshold", "consistency"])
def test_refuses_what_only_the_unet_serves(call, kw, what):
    """behind every refusal the shared checks make (SHARED_REFUSALS: each still comes first) and in front of the size checks"""
    rc, msg = call.tfm_sample(**kw)
    assert rc != 0 and _text(msg) == "dq_tfm_sample: " + what, msg
    rc, msg = call.tfm_sample(B=0, S2=-1, ws_bytes=0, T=0, **kw)  # in front of the sizes, the workspace and the schedule length
    assert rc != 0 and _text(msg) == "dq_tfm_sample: " + what, msg
    for kw2, first in SHARED_REFUSALS:
        if set(kw2) & set(kw):
            continue
        if "threshold_quantile" in kw and kw2.get("eta", 0.0) > 0.0 and first.startswith("eta > 0 and a null"):
            first = "threshold_quantile needs eta == 0"  # (thresholding is refused where clip_x0 is, in front of the seed)
        rc, msg = call.tfm_sample(**kw2, **kw)
        assert rc != 0 and _text(msg) == "dq_tfm_sample: " + first, (kw2, msg)
    # a field's own refusal is one of those that come first
    rc, msg = call.tfm_sample(guided=1, guidance_scale=-1.0)
    assert rc != 0 and "the guidance scale must be finite" in msg
    rc, msg = call.tfm_sample(guidance_rescale=1.5)
    assert rc != 0 and "guidance_rescale must satisfy" in msg


@pytest.mark.parametrize("kw", [dict(ts=[], num_steps=0), dict(ts=[5], num_steps=1025), dict(ts=[5], num_steps=1 << 30, sampler=1),  # (its list is not read)
                                 dict(ts=[5], num_steps=-3), dict(B=0), dict(S1=0), dict(S2=-1)])
def test_refuses_bad_sizes(call, kw):
    rc, msg = call.tfm_sample(**kw)
    assert rc != 0 and _text(msg) == "dq_tfm_sample: need B, S1, S2 > 0 and 1 <= num_steps <= 1024", msg


def test_refuses_a_short_workspace_and_a_bad_schedule_length(call):
    rc, msg = call.tfm_sample(ws_bytes=1024)
    assert rc != 0 and "dq_tfm_sample: workspace too small" in msg
    rc, msg = call.tfm_sample(T=0)
    assert rc != 0 and "dq_tfm_sample: num_timesteps must be >= 1" in msg


def _adapter_model(**kw):
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    net = DDIMTransformerAdapter(CustomTransformer(input_dim=8, hidden_dim=8, num_heads=1, num_layers=1))
    return DDIMDiffusionModel(model_class=net, num_timesteps=20, device="cpu", **kw)


def test_sample_argument_checks_on_the_adapter():
    dm = _adapter_model()
    assert dm.native_tfm_sampler is False and dm._native_tfm and not dm.native
    x, c2, c1 = torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), torch.zeros(1, 4)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            dm.sample(x, c2, c1, num_steps=2, eta=bad, sampler="ddim")
    with pytest.raises(ValueError, match="Unknown sampler"):
        dm.sample(x, c2, c1, num_steps=2, sampler="heun")
    with pytest.raises(ValueError, match="deterministic"):
        dm.sample(x, c2, c1, num_steps=2, sampler="dpmpp_2m", eta=0.5)
    with pytest.raises(ValueError, match="clip_x0"):
        dm.sample(x, c2, c1, num_steps=2, clip_x0=1.0)
    with pytest.raises(ValueError, match="strictly decreasing"):
        dm.sample(x, c2, c1, num_steps=50, sampler="ddim")
    # valid arguments, host tensors: the refusal now names the transformer's sampler as a way out (it runs on the GPU only)
    for kw in (dict(sampler="ddim"), dict(sampler="dpmpp_2m"), dict(eta=0.5), dict(seed=3)):
        with pytest.raises(NotImplementedError, match="CustomTransformer behind DDIMTransformerAdapter"):
            dm.sample(x, c2, c1, num_steps=2, **kw)


def test_sample_workspace_is_cached():
    from dquartic.model.building_blocks import CustomTransformer

    net = CustomTransformer(input_dim=8, hidden_dim=8, num_heads=1, num_layers=1)
    a = net.sample_workspace(2, 4, 3, 5)
    assert a.dtype == torch.uint8 and a.numel() == _lib().dq_tfm_sample_workspace_bytes(net._tfm, 2, 4, 3, 5)
    assert net.sample_workspace(2, 4, 3, 5) is a
    b = net.sample_workspace(2, 4, 3, 6)
    assert b is not a and net.sample_workspace(2, 4, 3, 6) is b
    with pytest.raises(RuntimeError):
        net.sample_workspace(2, 4, 3, 0)


def test_config_key_sets_the_attribute():
    from dquartic.cli import build_model

    m = {"use_model": "CustomTransformer", "num_timesteps": 20, "beta_schedule_type": "cosine", "pred_type": "eps", "auto_normalize": True,
         "ms1_loss_weight": 0.0, "CustomTransformer": {"input_dim": 8, "hidden_dim": 8, "num_heads": 1, "num_layers": 1}}
    assert build_model(m, "cpu").native_tfm_sampler is False  # off by default
    m["CustomTransformer"]["native_sampler"] = True
    assert build_model(m, "cpu").native_tfm_sampler is True
