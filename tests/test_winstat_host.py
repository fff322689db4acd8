"""Per-window sampler control, everything that needs no device: the refusals of ``dq_window_rescale``,
``dq_window_abs_quantile``, ``dq_step_update_adaptive`` and ``dq_ddim_sample`` with the per-window fields (dummy pointers, never dereferenced: each refusal
names its reason and nothing is launched), the scratch size rule, the Python surface's argument checks and routing, the command line, and
this file's numpy transcription of the quantile rule (``abs_quantile_ref``, which tests/test_winstat_kernels.py holds the kernels to bit
for bit) against ``np.quantile(..., method="linear")``."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

INF = float("inf")
NAN = float("nan")


def abs_quantile_ref(x, q):
    """The rule of include/dq_hip.h for one window: a = sort(|x|) in float32, h = (double)(float)q (n - 1), j = floor(h), Q = a_j if
    j == n - 1 else a_j + (a_{j+1} - a_j) (h - j) with every float64 operation rounded on its own, rounded to float32 once."""
    a = np.sort(np.abs(np.asarray(x, dtype=np.float32).reshape(-1)))
    n = a.size
    h = np.float64(np.float32(q)) * np.float64(n - 1)
    j = int(np.floor(h))
    if j == n - 1:
        return np.float32(a[j])
    d = np.float64(a[j + 1]) - np.float64(a[j])
    p = d * (h - np.float64(j))
    return np.float32(np.float64(a[j]) + p)


def stat_scratch_bytes(B, per):
    """the size rule of include/dq_hip.h"""
    return 80 * B + 4128 * B * ((per + 8191) // 8192)


@pytest.mark.parametrize("q", [1e-3, 0.5, 0.995, 1.0])
@pytest.mark.parametrize("n", [1, 2, 5, 8, 260, 25600])
def test_quantile_rule_is_numpys_linear_method(n, q):
    a = np.abs(3.0 * np.random.default_rng(1000 * n + int(1e4 * q)).standard_normal(n)).astype(np.float32)
    ref = np.float32(np.quantile(a.astype(np.float64), np.float64(np.float32(q)), method="linear"))
    got = abs_quantile_ref(a, q)
    assert got.dtype == np.float32
    assert abs(np.float64(got) - np.float64(ref)) <= np.spacing(np.abs(ref)), (n, q, got, ref)
    # sign, order and a -0.0 do not matter; the two order statistics are elements of the window
    b = a.copy()
    b[::2] *= -1
    assert abs_quantile_ref(b[::-1], q) == got
    assert abs_quantile_ref(np.array([-0.0, 0.0, -0.0], dtype=np.float32), q).tobytes() == np.float32(0.0).tobytes()
    assert abs_quantile_ref(a, 1.0) == a.max() and (n < 2 or abs_quantile_ref(a, 1e-12) >= a.min())


def test_scratch_size_rule():
    from dquartic import _native as N

    lib = N.lib()
    for B, per in ((1, 1), (3, 8191), (3, 8192), (3, 8193), (256, 25600), (65535, 1), (2, 2 ** 31 - 1)):
        assert lib.dq_sample_stat_scratch_bytes(B, per) == stat_scratch_bytes(B, per), (B, per)
    for B, per in ((0, 8), (-1, 8), (2, 0), (2, -5)):
        assert lib.dq_sample_stat_scratch_bytes(B, per) == -1


def test_the_stand_alone_entries_refuse_by_message():
    from dquartic import _native as N

    lib = N.lib()
    f, dbl = ctypes.c_float, ctypes.c_double
    d = ctypes.c_void_p(4096)
    big = 1 << 40

    def resc(c=d, u=d, w=3.0, phi=0.7, B=2, per=8, out=d, scratch=d, nbytes=big):
        return lib.dq_window_rescale(c, u, f(w), dbl(phi), B, per, out, scratch, nbytes, None)

    for kw, word in ((dict(c=None), b"null argument"), (dict(u=None), b"null argument"), (dict(out=None), b"null argument"),
                     (dict(scratch=None), b"null argument"), (dict(w=-1.0), b"guidance scale"), (dict(w=NAN), b"guidance scale"),
                     (dict(w=INF), b"guidance scale"), (dict(phi=-0.01), b"0 <= guidance_rescale <= 1"), (dict(phi=1.01), b"0 <= guidance_rescale <= 1"),
                     (dict(phi=NAN), b"0 <= guidance_rescale <= 1"), (dict(B=0), b"1 <= B <= 65535"), (dict(B=65536), b"1 <= B <= 65535"),
                     (dict(per=0), b"per_window < 2^31"), (dict(per=2 ** 31), b"per_window < 2^31"),
                     (dict(nbytes=stat_scratch_bytes(2, 8) - 1), b"scratch too small"), (dict(scratch=ctypes.c_void_p(4104)), b"16-byte aligned"),
                     (dict(c=ctypes.c_void_p(4098)), b"4-byte aligned")):
        assert resc(**kw) != 0, kw
        err = lib.dq_last_error()
        assert word in err and b"dq_window_rescale" in err, (kw, err)

    def quant(x=d, B=2, per=8, q=0.5, out=d, scratch=d, nbytes=big):
        return lib.dq_window_abs_quantile(x, B, per, f(q), out, scratch, nbytes, None)

    for kw, word in ((dict(x=None), b"null argument"), (dict(out=None), b"null argument"), (dict(scratch=None), b"null argument"),
                     (dict(q=0.0), b"0 < threshold_quantile <= 1"), (dict(q=-0.5), b"0 < threshold_quantile <= 1"),
                     (dict(q=1.0001), b"0 < threshold_quantile <= 1"), (dict(q=NAN), b"0 < threshold_quantile <= 1"),
                     (dict(B=0), b"1 <= B <= 65535"), (dict(per=0), b"per_window < 2^31"),
                     (dict(nbytes=stat_scratch_bytes(2, 8) - 1), b"scratch too small"), (dict(scratch=ctypes.c_void_p(4104)), b"16-byte aligned"),
                     (dict(x=ctypes.c_void_p(4098)), b"4-byte aligned")):
        assert quant(**kw) != 0, kw
        err = lib.dq_last_error()
        assert word in err and b"dq_window_abs_quantile" in err, (kw, err)

    def upd(kind=0, x=d, c=d, u=d, out=d, hist=d, coef=d, w=3.0, tab=d, seed=d, pred=0, B=1, per=8):
        return lib.dq_step_update_adaptive(kind, x, c, u, out, None, hist, None, coef, f(w), tab, None, seed, 1, pred, B, per, None)

    for kw, word in ((dict(x=None), b"null argument"), (dict(c=None), b"null argument"), (dict(out=None), b"null argument"),
                     (dict(coef=None), b"null argument"), (dict(tab=None), b"null argument"), (dict(kind=4), b"unknown update kind"),
                     (dict(kind=-1), b"unknown update kind"), (dict(kind=0, u=None), b"unguided per-window form"),
                     (dict(kind=1, u=None), b"unguided per-window form"), (dict(kind=1, seed=None), b"needs the seed"),
                     (dict(kind=3, hist=None), b"x0 history"), (dict(pred=3), b"Unknown pred_type"), (dict(pred=-1), b"Unknown pred_type"),
                     (dict(w=-0.5), b"guidance scale"), (dict(w=NAN), b"guidance scale"), (dict(w=INF), b"guidance scale"),
                     (dict(B=-1), b"negative size"), (dict(tab=ctypes.c_void_p(4098)), b"4-byte aligned")):
        assert upd(**kw) != 0, kw
        err = lib.dq_last_error()
        assert word in err, (kw, err)
    assert upd(B=0) == 0 and upd(per=0) == 0 and upd(kind=2, u=None, B=0) == 0  # nothing to do: no launch
    assert ctypes.c_int(lib.dq_abi_version()).value == N.ABI_VERSION == 13


def test_the_sampling_entry_refuses_in_sampler_checks_order():
    from dquartic import _native as N
    from test_sampler_tables import alpha_bars

    lib = N.lib()
    d, D = ctypes.c_void_p(4096), 4096
    dims = (ctypes.c_int * 2)(1, 2)
    plan = lib.dq_plan_create(4, 2, dims, 8, 1000)
    assert plan
    try:
        ab = alpha_bars("cosine")
        ab_c = (ctypes.c_float * len(ab))(*ab.tolist())

        def call(ts=(999, 0), eta=0.0, sampler=1, clip=0.0, guided=1, w=3.0, phi=0.0, q=0.0, cap=INF, params=d, pred=0, scratch=D, nbytes=1 << 40,
                 B=1):
            ts_c = (ctypes.c_int32 * len(ts))(*ts)
            rec = N.sample_call(alpha_bars_host=ctypes.addressof(ab_c), num_timesteps=len(ab), x_T=D, ms2_cond=D, ms1_cond=D, auto_normalize=1,
                                pred_type=pred, timesteps_host=ctypes.addressof(ts_c), num_steps=len(ts), out_x=D, out_noise=D, workspace=D,
                                workspace_bytes=1 << 40, B=B, RT=8, eta=eta, seed_dev=D, sampler=sampler, clip_x0=clip, guided=guided,
                                guidance_scale=w, guidance_rescale=phi, threshold_quantile=q, threshold_max=cap, stat_scratch=scratch,
                                stat_scratch_bytes=nbytes)
            return lib.dq_ddim_sample(plan, params, d, ctypes.byref(rec))

        cases = (
            # sampler_check's refusals, in its order, under the entry's name
            (dict(params=None), b"null argument"), (dict(eta=1.5), b"eta must satisfy"), (dict(sampler=7), b"unknown sampler"),
            (dict(eta=0.5, sampler=2), b"eta must be 0"), (dict(clip=1.0, sampler=0), b"clip_x0 needs the ddim or dpmpp_2m sampler"),
            (dict(clip=1.0, eta=0.5), b"clip_x0 needs eta == 0"),
            # thresholding is refused exactly where clip_x0 is, in the same words
            (dict(q=0.9, sampler=0), b"threshold_quantile needs the ddim or dpmpp_2m sampler"),
            (dict(q=0.9, eta=0.5), b"threshold_quantile needs eta == 0"),
            (dict(ts=(999, 999)), b"strictly decreasing"), (dict(pred=3), b"Unknown pred_type"), (dict(w=-1.0), b"guidance scale"),
            # then the options' own
            (dict(phi=-0.1), b"0 <= guidance_rescale <= 1"), (dict(phi=1.5), b"0 <= guidance_rescale <= 1"), (dict(phi=NAN), b"0 <= guidance_rescale <= 1"),
            (dict(q=-0.1), b"0 < threshold_quantile <= 1"), (dict(q=1.5), b"0 < threshold_quantile <= 1"), (dict(q=NAN), b"0 < threshold_quantile <= 1"),
            (dict(q=0.9, cap=0.5), b"threshold_max must be >= the floor"), (dict(q=0.9, clip=2.0, cap=1.5), b"threshold_max must be >= the floor"),
            (dict(q=0.9, cap=NAN), b"threshold_max must be >= the floor"),
            (dict(q=0.9, scratch=None), b"null argument"), (dict(phi=0.5, scratch=None), b"null argument"),
            (dict(q=0.9, nbytes=stat_scratch_bytes(1, 64) - 1), b"scratch too small"),
            (dict(phi=0.5, B=3, nbytes=stat_scratch_bytes(3, 64) - 1), b"scratch too small"),
            (dict(q=0.9, scratch=4104), b"16-byte aligned"),
        )
        for kw, word in cases:
            assert call(**kw) != 0, kw
            err = lib.dq_last_error()
            assert word in err and err.startswith(b"dq_ddim_sample: "), (kw, err)
        assert call(sampler=7, phi=2.0) != 0 and b"unknown sampler" in lib.dq_last_error()  # (the sampler's refusal comes first)
        assert call(q=0.9, sampler=0, cap=0.5) != 0 and b"threshold_quantile needs the ddim" in lib.dq_last_error()
        # with both options at 0 the per-window checks are not made: threshold_max is not looked at and the scratch may be null -- the call
        # gets as far as the refusal behind them (the batch count)
        for guided in (0, 1):
            assert call(cap=NAN, scratch=None, nbytes=0, guided=guided, B=0) != 0 and b"need B, RT > 0" in lib.dq_last_error()
        # the workspace and its size query are what they were
        assert lib.dq_unet_workspace_bytes(plan, 3, 4, 1) == 2 * lib.dq_unet_workspace_bytes(plan, 3, 4, 0)
    finally:
        lib.dq_plan_destroy(plan)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
KW = dict(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)


def _dm():
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    return DDIMDiffusionModel(model_class=UNet1d(**KW), device="cpu")


def test_python_argument_checks():
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    dm = _dm()
    x, c2, c1 = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 8)
    for bad in (-0.1, 1.0001, NAN, INF, "much", [0.5], None):
        with pytest.raises(ValueError, match="guidance_rescale"):
            dm.sample(x, c2, c1, num_steps=2, guidance_scale=3.0, guidance_rescale=bad)
    for bad in (0.0, -0.5, 1.0001, NAN, INF, 1e-60, "high", [0.5]):  # (1e-60 is 0 as the float32 the kernels take it as)
        with pytest.raises(ValueError, match="threshold_quantile"):
            dm.sample(x, c2, c1, num_steps=2, sampler="ddim", threshold_quantile=bad)
    for kw in (dict(threshold_max=0.5), dict(threshold_max=NAN), dict(clip_x0=2.0, threshold_max=1.5)):
        with pytest.raises(ValueError, match="threshold_max"):
            dm.sample(x, c2, c1, num_steps=2, sampler="ddim", threshold_quantile=0.9, **kw)
    with pytest.raises(ValueError, match="threshold_max needs threshold_quantile"):
        dm.sample(x, c2, c1, num_steps=2, sampler="ddim", threshold_max=2.0)
    # refused exactly where clip_x0 is, in the same words
    with pytest.raises(ValueError, match="threshold_quantile needs sampler 'ddim' or 'dpmpp_2m'"):
        dm.sample(x, c2, c1, num_steps=2, threshold_quantile=0.9)
    with pytest.raises(ValueError, match="threshold_quantile needs eta == 0"):
        dm.sample(x, c2, c1, num_steps=2, sampler="ddim", eta=0.5, threshold_quantile=0.9)
    with pytest.raises(ValueError, match="clip_x0 needs eta == 0"):
        dm.sample(x, c2, c1, num_steps=2, sampler="ddim", eta=0.5, clip_x0=1.0, threshold_quantile=0.9)  # (the earlier refusals keep their place)
    assert dm._check_adaptive(0.0, None, None, "reference", 0.0, 0.0) == (0.0, 0.0, INF)
    assert dm._check_adaptive(1, 1, None, "ddim", 0.0, 0.0) == (1.0, 1.0, INF)
    phi, q, cap = dm._check_adaptive(0.7, 0.995, 4, "dpmpp_2m", 0.0, 2.0)
    assert (phi, cap) == (0.7, 4.0) and q == float(np.float32(0.995))  # q is the float32 the library takes
    # host tensors: the generic loop serves neither option
    for kw in (dict(guidance_scale=3.0, guidance_rescale=0.5), dict(sampler="ddim", threshold_quantile=0.9)):
        with pytest.raises(NotImplementedError, match="native sampler"):
            dm.sample(x, c2, c1, num_steps=2, **kw)
    tfm = DDIMDiffusionModel(model_class=DDIMTransformerAdapter(CustomTransformer(input_dim=8, hidden_dim=8, num_heads=1, num_layers=1)),
                             device="cpu")
    with pytest.raises(NotImplementedError, match=r"dq_ddim_sample\).*follow-up"):
        tfm.sample(x, c2, c1, num_steps=2, sampler="ddim", threshold_quantile=0.9)
    with pytest.raises(NotImplementedError, match="follow-up"):
        tfm.sample(x, c2, c1, num_steps=2, guidance_scale=3.0, guidance_rescale=0.5)  # (guidance itself is the transformer's follow-up too)


def test_the_defaults_route_to_the_existing_entries(monkeypatch):
    """phi = 0 with q unset -- and phi > 0 without guidance, where g = c and m = 1 -- is the call as it is today: the same
    record; only a live option sets the three values and the scratch (the fields behind null_ms1: test_abi's layout test; what
    _sample_native writes for them: test_sample_loop.test_entry_choice_guided_and_per_window)"""
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel

    dm = _dm()
    seen = []

    def fake(self, *a, **kw):
        seen.append(kw)
        return None, None

    monkeypatch.setattr(DDIMDiffusionModel, "_sample_native", fake)

    class Cuda:  # stands in for a device tensor: only .is_cuda is read before the native call
        is_cuda = True

    t = Cuda()
    base = dict(num_steps=2, sampler="ddim", clip_x0=1.0)
    for extra in (dict(), dict(guidance_rescale=0.0), dict(guidance_rescale=0.7), dict(guidance_rescale=0.7, guidance_scale=1.0),
                  dict(guidance_rescale=0.7, guidance_scale=None), dict(threshold_quantile=None, threshold_max=None)):
        seen.clear()
        dm.sample(t, t, t, **base, **extra)
        assert len(seen) == 1 and "adaptive" not in seen[0] and seen[0].get("guidance") is None, (extra, seen)
    seen.clear()
    dm.sample(t, t, t, **base, guidance_scale=3.0, guidance_rescale=0.0)
    assert "adaptive" not in seen[0] and seen[0]["guidance"] == (3.0, 0.0)  # the guided call as it is
    for extra, want in ((dict(guidance_scale=3.0, guidance_rescale=0.7), (0.7, 0.0, INF)),
                        (dict(threshold_quantile=0.5), (0.0, 0.5, INF)),
                        (dict(guidance_scale=3.0, guidance_rescale=1, threshold_quantile=0.5, threshold_max=2), (1.0, 0.5, 2.0)),
                        (dict(guidance_rescale=0.7, threshold_quantile=0.5), (0.0, 0.5, INF))):  # unguided: the rescale is a no-op
        seen.clear()
        dm.sample(t, t, t, **base, **extra)
        assert seen[0]["adaptive"] == want, (extra, seen)
        assert (seen[0]["guidance"] is None) == ("guidance_scale" not in extra)
    # the record takes (phi, q, cap, scratch, bytes) behind the guidance fields
    names = [k for k, _ in N.SampleCall._fields_]
    i = names.index("null_ms1") + 1
    assert N.SampleCall._fields_[i:i + 5] == [("guidance_rescale", ctypes.c_double), ("threshold_quantile", ctypes.c_float), ("threshold_max", ctypes.c_float),
                                              ("stat_scratch", ctypes.c_void_p), ("stat_scratch_bytes", ctypes.c_int64)]


def test_signatures_and_pass_through():
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.model_interface import ModelInterface, _sampler_kwargs

    new = ("guidance_rescale", "threshold_quantile", "threshold_max")
    for fn in (DDIMDiffusionModel.sample, ModelInterface.predict, ModelInterface.evaluate, ModelInterface._predict_one_batch):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in new] == [0.0, None, None], fn.__name__
    assert all(k in ModelInterface._RUN_SAMPLE_OPTIONS for k in new)
    assert _sampler_kwargs("reference", None) == {} and _sampler_kwargs("reference", None, None, 0.0, 0.0, None, None) == {}
    assert _sampler_kwargs("ddim", None, 3.0, 0.5, 0.7, 0.995, 4.0) == {"sampler": "ddim", "guidance_scale": 3.0, "null_ms1": 0.5,
                                                                        "guidance_rescale": 0.7, "threshold_quantile": 0.995, "threshold_max": 4.0}
    dm = _dm()
    with pytest.raises(TypeError, match="unknown option"):
        dm.deconvolve_run(torch.zeros(8, 8), torch.zeros(8), window=4, threshold=0.9)


def test_cli_options():
    from click.testing import CliRunner

    from dquartic import cli

    for cmd in (cli.evaluate, cli.deconvolve):
        opts = {o.name: o for o in cmd.params}
        assert opts["guidance_rescale"].default == 0.0 and opts["threshold_quantile"].default is None and opts["threshold_max"].default is None
        assert "--guidance-rescale" in opts["guidance_rescale"].opts and "--threshold-quantile" in opts["threshold_quantile"].opts
        assert "--threshold-max" in opts["threshold_max"].opts
        res = CliRunner().invoke(cli.cli, [cmd.name, "--help"])
        assert res.exit_code == 0
        for flag in ("--guidance-rescale", "--threshold-quantile", "--threshold-max"):
            assert flag in res.output, (cmd.name, flag)
        bad = CliRunner().invoke(cli.cli, [cmd.name, "--threshold-quantile", "often"])
        assert bad.exit_code == 2 and "threshold-quantile" in bad.output
