"""The one sampling loop under both networks (csrc/dq_sampler.h: replay_captured_step, eager_steps).

The U-Net's and the transformer's entry run the same capture function, each over the StepGraph of its own handle.  What the other sampling
tests do not see is the two in one process, one after the other:
  * graph calls of the two networks interleaved, every one bit for bit the eager call (use_graph = False) of its setting on its model;
  * a handle destroyed with a live graph and capture stream, and the same model built again from the same seed: the same result.
Models: test_stochastic_sampler's U-Net at batch 2 and test_tfm_sample's "two_layers" transformer, 3 steps each.

Without a GPU: what ``DDIMDiffusionModel._sample_native`` writes into the call's record (``dq_sample_call``) for (eta, sampler), over a
recorder in place of the library -- the fields that are no option are the same in every call, which is what lets
test_sample_ex_eta0_is_dq_ddim_sample compare two calls; and likewise for guidance, the v objective and the per-window options, each
setting exactly its own fields and leaving every other option at its off value.  The options that are
not at their defaults: one rule (``SampleOptions.non_default``) under ``_sampler_kwargs``, ``evaluate``'s report and the command line."""
import ctypes
import gc
import inspect

import numpy as np
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
    """stands in for the library: a sampling entry returns 0 and leaves ``(name, fields)`` -- the record it received, field by name as it
    stood at the call (pointers as integers or None), with ``_head`` (the network's own arguments in front of the record) and
    ``_timesteps`` (the host list behind ``timesteps_host``).  Anything else is a handle of an earlier test that the collector frees
    meanwhile: that goes to the library the handle came from"""

    def __init__(self, real):
        self.calls, self.real = [], real

    def __getattr__(self, name):
        if not (name.startswith("dq_ddim_sample") or name == "dq_tfm_sample"):
            return getattr(self.real(), name)

        def entry(*args):
            q = args[-1]._obj
            fields = {k: getattr(q, k) for k, _ in type(q)._fields_}
            fields["_head"] = [_plain(v) for v in args[:-1]]
            fields["_timesteps"] = list((ctypes.c_int32 * q.num_steps).from_address(q.timesteps_host))
            self.calls.append((name, fields))
            return 0
        return entry


def _plain(v):
    if isinstance(v, ctypes.c_void_p):
        return ("ptr", v.value)
    return v


# every option of the record by the group it belongs to, at its off value (include/dq_hip.h)
OPTIONS_OFF = {
    "noise": dict(eta=0.0, seed_dev=None, window_ids_dev=None),
    "sampler": dict(sampler=0, clip_x0=0.0),
    "guided": dict(guided=0, guidance_scale=0.0, null_ms1=0.0),
    "per_window": dict(guidance_rescale=0.0, threshold_quantile=0.0, threshold_max=0.0, stat_scratch=None, stat_scratch_bytes=0),
    "joint": dict(group_size=1, consistency=0, consistency_strength=0.0),
}
ALLOCATED = ("out_x", "out_noise", "traj_x", "traj_eps", "timesteps_host")  # what a call allocates itself (the list's values: _timesteps)


def _options(fields, **live):
    """the record's option fields are exactly ``live`` (group -> its fields' values) and, in every other group, the off values"""
    assert set(live) <= set(OPTIONS_OFF)
    for group, off in OPTIONS_OFF.items():
        want = live.get(group, off)
        assert set(want) == set(off), group
        assert {k: fields[k] for k in off} == want, (group, {k: fields[k] for k in off})


def _shared(fields):
    """what every call of one model on the same inputs fills alike: all but the options and what a call allocates"""
    opt = {k for off in OPTIONS_OFF.values() for k in off}
    return {k: v for k, v in fields.items() if k not in opt and k not in ALLOCATED}


def _host_model(monkeypatch, pred="x0"):
    """test_entry_choice's stand-ins once more: the recorder in place of the library, an Identity carrying what _sample_native asks of
    UNet1d (the statistics scratch too), host tensors at B, RT, MZ = 2, 4, 8.  ``pred``: set on the built model, whose constructor
    takes the v objective for a UNet1d only"""
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel

    rec = _Recorder(N.lib)
    monkeypatch.setattr(N, "lib", lambda: rec)
    monkeypatch.setattr(N, "stream_ptr", lambda: ctypes.c_void_p(0x5EED))
    g = torch.Generator().manual_seed(3)
    flat, ws, rope, stat = torch.rand(16, generator=g), torch.empty(64), torch.rand(4, generator=g), torch.empty(32)
    net = torch.nn.Identity()
    net._plan = ctypes.c_void_p(0xABC0)
    net._check_inputs = lambda c, b, rt: c[..., None]
    net.read_params, net.rope_freqs, net.workspace, net.stat_scratch = (lambda: flat), (lambda: rope), (lambda b, rt, training: ws), (lambda b, per: stat)
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=50, pred_type="x0", device="cpu")
    dm.pred_type = pred
    inputs = torch.randn(2, 4, 8, generator=g), torch.rand(2, 4, 8, generator=g), torch.rand(2, 4, generator=g)
    return rec, dm, inputs, stat


def test_entry_choice_guided_and_per_window(monkeypatch):
    """every call reaches dq_ddim_sample; guidance sets (guided, scale, null_ms1), a live per-window option (phi, q, cap, the scratch and
    its size), guided or not; every option that is not live holds its off value, and what is not an option is the default call's"""
    rec, dm, inputs, stat = _host_model(monkeypatch)
    INF = float("inf")
    keep = [dm._sample_native(*inputs, STEPS),
            dm._sample_native(*inputs, STEPS, eta=0.0, sampler=1, clip_x0=1.5, guidance=(3.0, 0.25)),
            dm._sample_native(*inputs, STEPS, eta=0.0, guidance=(0.5, 0.0)),
            dm._sample_native(*inputs, STEPS, eta=0.0, sampler=1, clip_x0=1.5, guidance=(3.0, 0.25), adaptive=(0.7, 0.5, 2.0)),
            dm._sample_native(*inputs, STEPS, eta=0.0, sampler=2, adaptive=(0.0, 0.5, INF))]
    scratch = dict(stat_scratch=stat.data_ptr(), stat_scratch_bytes=stat.numel())
    f32 = lambda v: ctypes.c_float(v).value  # noqa: E731  (phi travels as a double, the rest as floats)
    want = [dict(),
            dict(sampler=dict(sampler=1, clip_x0=1.5), guided=dict(guided=1, guidance_scale=3.0, null_ms1=0.25)),
            dict(guided=dict(guided=1, guidance_scale=0.5, null_ms1=0.0)),
            dict(sampler=dict(sampler=1, clip_x0=1.5), guided=dict(guided=1, guidance_scale=3.0, null_ms1=0.25),
                 per_window=dict(guidance_rescale=0.7, threshold_quantile=0.5, threshold_max=2.0, **scratch)),
            dict(sampler=dict(sampler=2, clip_x0=0.0), per_window=dict(guidance_rescale=0.0, threshold_quantile=0.5, threshold_max=INF, **scratch))]
    assert len(rec.calls) == len(want) == len(keep) and f32(0.25) == 0.25
    for (name, fields), live in zip(rec.calls, want):
        assert name == "dq_ddim_sample", name
        _options(fields, **live)
        assert _shared(fields) == _shared(rec.calls[0][1]), live


def test_entry_choice_v_prediction(monkeypatch):
    """a v_prediction model reaches dq_ddim_sample with pred_type DQ_PRED_V in all four forms -- plain, eta, sampler, guided -- and
    nothing but the live options set; a seed travels as the device word, and is recorded"""
    from dquartic import _native as N

    rec, dm, inputs, _ = _host_model(monkeypatch, "v_prediction")
    keep = [dm._sample_native(*inputs, STEPS), dm._sample_native(*inputs, STEPS, eta=0.0), dm._sample_native(*inputs, STEPS, eta=0.0, sampler=2),
            dm._sample_native(*inputs, STEPS, eta=0.0, sampler=1, clip_x0=1.5, guidance=(3.0, 0.25))]
    lives = [dict(), dict(), dict(sampler=dict(sampler=2, clip_x0=0.0)),
             dict(sampler=dict(sampler=1, clip_x0=1.5), guided=dict(guided=1, guidance_scale=3.0, null_ms1=0.25))]
    assert len(rec.calls) == len(keep) == 4
    for (name, fields), live in zip(rec.calls, lives):
        assert name == "dq_ddim_sample"
        _options(fields, **live)
        assert _shared(fields) == _shared(rec.calls[0][1]) and fields["pred_type"] == N.PRED_TYPES["v_prediction"] == 2
    dm._sample_native(*inputs, STEPS, eta=0.5, seed=7)
    fields = rec.calls[-1][1]
    assert fields["eta"] == 0.5 and isinstance(fields["seed_dev"], int) and fields["seed_dev"] != 0 and fields["window_ids_dev"] is None
    assert dm.last_seed == 7
    _options(fields, noise=dict(eta=0.5, seed_dev=fields["seed_dev"], window_ids_dev=None))


def test_one_rule_for_the_options_that_are_not_at_their_defaults():
    """over every subset of the seven options at a live value: SampleOptions.non_default, _sampler_kwargs (predict / evaluate /
    _predict_one_batch), the keys evaluate reports and the ``sample_kw`` that ``cli.sampling_options`` hands cli.evaluate and
    cli.deconvolve (which forward it as it is) are one set with the same values -- an option at its default is absent, null_ms1 goes with
    guidance_scale and never without it"""
    import dataclasses
    import itertools

    from dquartic import cli
    from dquartic.model.model import SampleOptions
    from dquartic.model.model_interface import _reported_options, _sampler_kwargs

    default = dict(sampler="reference", clip_x0=None, guidance_scale=None, null_ms1=0.0, guidance_rescale=0.0, threshold_quantile=None,
                   threshold_max=None)
    live = dict(sampler="ddim", clip_x0=1.5, guidance_scale=3.0, null_ms1=0.25, guidance_rescale=0.7, threshold_quantile=0.9, threshold_max=4.0)
    assert [f.name for f in dataclasses.fields(SampleOptions)] == list(default) and dataclasses.asdict(SampleOptions()) == default
    command = cli.sampling_options(lambda **kw: kw)  # what a command body is called with: the seven options gone, sample_kw in their place
    for on in itertools.product((False, True), repeat=len(default)):
        opts = {k: (live if o else default)[k] for k, o in zip(default, on)}
        want = {k: opts[k] for k, o in zip(default, on) if o and k != "null_ms1"}
        if "guidance_scale" in want:
            want["null_ms1"] = opts["null_ms1"]
        assert SampleOptions(**opts).non_default() == want, opts
        assert _sampler_kwargs(opts["sampler"], opts["clip_x0"], opts["guidance_scale"], opts["null_ms1"], opts["guidance_rescale"],
                               opts["threshold_quantile"], opts["threshold_max"]) == want, opts
        assert _sampler_kwargs(**opts) == want
        shown = _reported_options(want)
        assert shown == want and all(type(v) is (str if k == "sampler" else float) for k, v in shown.items())
        assert command(eta=0.5, seed=3, use_ema=None, **opts) == dict(eta=0.5, seed=3, use_ema=None, sample_kw=want), opts
    # evaluate reports plain values whatever the Python caller passed: an int clamp, a numpy scale
    shown = _reported_options(_sampler_kwargs("ddim", 2, np.float32(3.0), 1))
    assert shown == dict(sampler="ddim", clip_x0=2.0, guidance_scale=3.0, null_ms1=1.0) and all(type(shown[k]) is float for k in list(shown)[1:])
    # the command line declares the options once, at the record's defaults (what it forwards at its defaults is nothing), and both
    # commands are bodies behind that decorator: they take sample_kw and none of the seven
    for cmd in (cli.evaluate, cli.deconvolve):
        params = {o.name: o for o in cmd.params}
        body = inspect.signature(cmd.callback.__wrapped__).parameters
        assert "sample_kw" in body and not set(default) & set(body), cmd.name
        assert inspect.getsource(cmd.callback.__wrapped__).count("**sample_kw") == 1, cmd.name
        assert {k: params[k].default for k in default} == default, cmd.name
        assert [o.name for o in cmd.params].count("eta") == 1 and params["eta"].default == 0.0 and params["seed"].default == 0
    source = inspect.getsource(cli)
    for flag in ("--eta", "--sampler", "--clip-x0", "--guidance-scale", "--null-ms1", "--guidance-rescale", "--threshold-quantile",
                 "--threshold-max", "--seed"):
        assert source.count(f'click.option("{flag}"') == 1, flag


def test_entry_choice(monkeypatch):
    """eta=None, eta=0.0 and sampler=1 all reach dq_ddim_sample: the first two with every option off (eta 0, null seed and ids), the third
    with (sampler, clip_x0) alone; what is not an option is the same in the three records"""
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
    assert [name for name, _ in rec.calls] == ["dq_ddim_sample"] * 3
    a0, a1, a2 = (fields for _, fields in rec.calls)
    _options(a0)
    _options(a1)
    _options(a2, sampler=dict(sampler=1, clip_x0=1.5))
    # the shared fields: what the caller owns is the same value or address in all three, what a call allocates (out_x, out_noise) differs
    assert _shared(a1) == _shared(a0) and _shared(a2) == _shared(a0)
    want = dict(struct_bytes=ctypes.sizeof(N.SampleCall), alpha_bars_host=ctypes.addressof(dm._alpha_bars_host()), num_timesteps=50,
                x_T=xT.data_ptr(), ms2_cond=c2.data_ptr(), auto_normalize=1, pred_type=N.PRED_TYPES["x0"], num_steps=STEPS, use_graph=1,
                workspace=ws.data_ptr(), workspace_bytes=ws.numel(), B=B, RT=RT, stream=0x5EED, _timesteps=[49, 24, 0],
                _head=[("ptr", 0xABC0), ("ptr", flat.data_ptr()), ("ptr", rope.data_ptr())])
    assert set(_shared(a0)) == set(want) | {"ms1_cond"}  # (the staged MS1 is the call's own)
    for k, w in want.items():
        assert a0[k] == w, k
    for (x, n), fields in zip(keep, (a0, a1, a2)):
        assert (fields["out_x"], fields["out_noise"]) == (x.data_ptr(), n.data_ptr()) and fields["traj_x"] is None and fields["traj_eps"] is None
    # return_trajectory: the trajectories go in, the graph flag goes off
    x, n, tx, te = dm._sample_native(xT, c2, c1, STEPS, True, eta=0.0)
    fields = rec.calls[-1][1]
    assert (fields["traj_x"], fields["traj_eps"], fields["use_graph"]) == (tx.data_ptr(), te.data_ptr(), 0)
    assert tx.shape == (STEPS, B, RT, MZ) == te.shape
