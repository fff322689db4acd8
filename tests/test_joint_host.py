"""Joint sampling of a window's precursors under mixture consistency, everything that needs no device: the numpy
fp32 transcription's own properties (tests/joint_ref.py), the refusals of ``dq_group_project`` and of ``dq_ddim_sample`` over groups on dummy pointers
(never dereferenced: each refusal is made before anything touches the device) and their order, the Python surface, the member-major id rule
and the command line's argument shapes."""
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

import joint_ref as R
from joint_ref import F, U

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- the rule itself
def _x0(rng, P, n):
    """estimates on both sides of 0 in image units (x0 in [-1, 1] space: y = (x0 + 1) / 2 around 0 .. 1), mixtures with exact zeros"""
    x0 = (rng.standard_normal((P, 1, n)) * 1.2 - 0.6).astype(F)
    mix = rng.random((1, n)).astype(F)
    mix[0, rng.random(n) < 0.05] = 0
    return x0, mix


@pytest.mark.parametrize("mode", ["bound", "sum"])
@pytest.mark.parametrize("P", range(1, 9))
def test_the_transcription_has_the_rules_properties(P, mode):
    rng = np.random.default_rng(100 * P + len(mode))
    x0, mix = _x0(rng, P, 20000)
    for normalize in (True, False):
        out, q = R.project_f32(x0, mix, mode, 1.0, normalize)
        y, yn, S, m, act = q["y"], q["yn"], q["S"], q["m"], q["act"]
        assert act.any() and (~act).any() or mode == "sum"
        # where the rule acts the members' positive parts add up to the mixture within (P + 1) 2^-24 m
        total = np.maximum(yn, 0).astype(np.float64).sum(axis=0)
        m64 = m.astype(np.float64)
        assert (np.abs(total - m64)[act] <= (P + 1) * U * m64[act]).all(), float((np.abs(total - m64)[act] / np.maximum(m64[act], 1e-300)).max() / U)
        if mode == "bound":
            assert (yn <= y).all()                                             # nothing is ever raised
            assert np.array_equal(yn[y <= 0].view(np.uint32), y[y <= 0].view(np.uint32))  # negatives are never touched
            assert np.array_equal(yn[:, ~act].view(np.uint32), y[:, ~act].view(np.uint32))  # under the mixture: nothing happens
            assert (total <= m64 * (1 + (P + 1) * U))[act].all() and (total[~act] <= m64[~act] * (1 + (P - 1) * U)).all()
        else:
            assert (yn >= 0).all()                                             # negatives go to 0
            allneg = ~act                                                      # S == 0: nothing positive to scale -> m / P each
            assert np.array_equal(yn[:, allneg], np.broadcast_to((m / F(P))[None], yn.shape)[:, allneg])
        # m == 0: the group explains nothing
        zero = m == 0
        assert zero.any() and (np.maximum(yn, 0)[:, zero] == 0).all()
        # strength 1 is z itself, not y + 1 (z - y)
        if mode == "sum":
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(y > 0, y, F(0)) * (m / S)[None]
            assert np.array_equal(yn[:, act].view(np.uint32), z[:, act].view(np.uint32))
        # an element the projection does not move keeps its x0 bits -- also where the map back would not return them
        still = yn == y
        assert np.array_equal(out[still].view(np.uint32), x0[still].view(np.uint32))
        if mode == "bound":  # (sum moves nearly everything; bound leaves every negative and every group under its mixture)
            assert still.any() and (not normalize or (((F(2) * y - F(1)) != x0) & still).any())
        assert np.array_equal(out[~still], (F(2) * yn - F(1) if normalize else yn)[~still])
        # a blend lies between the estimate and its projection, and moves exactly the elements the projection moves
        half, qh = R.project_f32(x0, mix, mode, 0.5, normalize)
        lo, hi = np.minimum(y, yn), np.maximum(y, yn)
        assert ((qh["yn"] >= lo) & (qh["yn"] <= hi)).all() and half.dtype == F
        assert np.array_equal(half[still].view(np.uint32), x0[still].view(np.uint32))


def test_all_nonpositive_group_in_sum_mode_and_p1_bound():
    x0 = np.array([[[-3.0, -1.0, -1.0]], [[-1.5, -1.0, -2.0]]], dtype=F)  # y <= 0 everywhere (y = 0 at x0 = -1)
    mix = np.array([[0.5, 0.25, 0.0]], dtype=F)
    out, q = R.project_f32(x0, mix, "sum", 1.0, True)
    assert np.array_equal(q["yn"], np.array([[[0.25, 0.125, 0.0]], [[0.25, 0.125, 0.0]]], dtype=F)) and not q["act"].any()
    # (the last column: member 0's y' == y == 0 keeps its own x0 = -1; member 1's y = -0.5 moves to 0, which maps back to -1)
    assert np.array_equal(out, np.array([[[-0.5, -0.75, -1.0]], [[-0.5, -0.75, -1.0]]], dtype=F))
    # P = 1, bound: a prediction may not exceed the observation
    x0 = np.array([[[1.0, 0.2, -0.3, 0.0]]], dtype=F)
    mix = np.array([[0.5, 0.5, 0.5, 0.0]], dtype=F)
    out, q = R.project_f32(x0, mix, "bound", 1.0, False)
    assert np.array_equal(out, np.array([[[0.5, 0.2, -0.3, 0.0]]], dtype=F))


def test_all_nonpositive_group_keeps_or_maps_back():
    """(the expected values of the case above, spelled out: y = (x0 + 1) / 2; S = 0; z = m / 2; x0' = 2 z - 1 unless z == y)"""
    x0 = np.array([[[-3.0]], [[-1.0]]], dtype=F)
    out, q = R.project_f32(x0, np.array([[0.0]], dtype=F), "sum", 1.0, True)
    assert q["y"].ravel().tolist() == [-1.0, 0.0] and q["yn"].ravel().tolist() == [0.0, 0.0]
    assert out.ravel().tolist() == [-1.0, -1.0]  # member 0 moved to y' = 0 -> x0' = -1; member 1 not moved: its own -1


def test_the_float64_rule_brackets_the_transcription():
    """joint_ref.project_f64's bound holds for the transcription itself (what the kernel test then asks of the kernel), and is tight enough
    to mean something: below 2^-18 of the values' scale for nearly every element"""
    rng = np.random.default_rng(7)
    for P in (1, 2, 3, 8):
        for pred in R.PREDS:
            for mode in R.MODES:
                for normalize in (True, False):
                    for strength in (1.0, 0.5):
                        x, net, mix = R.inputs(rng, P, 3, 500)
                        sa, sb = F(0.8), F(0.6)
                        got, _ = R.project_f32(R.x0_f32(pred, sa, sb, x, net), mix, mode, strength, normalize)
                        ref, bound = R.project_f64(pred, sa, sb, x, net, mix, mode, strength, normalize)
                        ok = np.isfinite(bound)
                        assert ok.mean() > 0.97, (P, pred, mode)
                        assert (np.abs(got - ref)[ok] <= bound[ok]).all(), (P, pred, mode, normalize, strength)
                        assert np.median(bound[ok] / (1 + np.abs(ref[ok]))) < 2.0 ** -18


# ---------------------------------------------------------------------------------------------------------------- the C refusals
def test_group_project_refuses_in_order():
    from dquartic import _native as N

    lib = N.lib()
    d, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    f = ctypes.c_float

    def call(x=d, net=d, out=d, mix=d, coef=d, pred=0, G=2, P=2, per=8, mode=1, strength=1.0):
        return lib.dq_group_project(x, net, out, mix, coef, pred, 1, G, P, per, mode, f(strength), None)

    order = ((dict(x=None), b"null argument"), (dict(net=None), b"null argument"), (dict(out=None), b"null argument"),
             (dict(mix=None), b"null argument"), (dict(coef=None), b"null argument"),
             (dict(pred=3), b"Unknown pred_type"), (dict(pred=-1), b"Unknown pred_type"),
             (dict(P=0), b"group_size must be 1..8"), (dict(P=9), b"group_size must be 1..8"),
             (dict(G=-1), b"negative size"), (dict(per=-1), b"negative size"),
             (dict(mode=0), b"unknown consistency mode"), (dict(mode=3), b"unknown consistency mode"),
             (dict(strength=0.0), b"0 < strength <= 1"), (dict(strength=-0.5), b"0 < strength <= 1"), (dict(strength=1.5), b"0 < strength <= 1"),
             (dict(strength=NAN), b"0 < strength <= 1"),
             (dict(x=odd), b"4-byte aligned"), (dict(net=odd), b"4-byte aligned"), (dict(out=odd), b"4-byte aligned"), (dict(mix=odd), b"4-byte aligned"))
    for kw, word in order:
        assert call(**kw) != 0, kw
        err = lib.dq_last_error()
        assert word in err and b"dq_group_project" in err, (kw, err)
    # each refusal comes before every later one: break one argument of every later kind as well
    for i, (kw, word) in enumerate(order):
        later = {}
        for kw2, word2 in order[i + 1:]:
            if word2 != word and not set(kw2) & set(later) and not set(kw2) & set(kw):
                later.update(kw2)
        assert call(**kw, **later) != 0 and word in lib.dq_last_error(), (kw, later, lib.dq_last_error())
    # nothing to do is not refused, and touches nothing: G = 0, per = 0 on pointers that cannot be read
    assert call(G=0) == 0 and call(per=0) == 0


def test_the_sampling_entry_refuses_dq_ddim_sample_vs_first_then_its_own():
    """(the name is from when the group options had an entry of their own: the order it pins is now the one entry's -- every refusal that
    needs no group first, then the group's)"""
    from dquartic import _native as N
    from test_sampler_tables import alpha_bars

    lib = N.lib()
    f = ctypes.c_float
    d, D = ctypes.c_void_p(4096), 4096
    dims = (ctypes.c_int * 2)(1, 2)
    plan = lib.dq_plan_create(4, 2, dims, 8, 1000)
    assert plan
    try:
        ab = alpha_bars("cosine")
        ab_c = (ctypes.c_float * len(ab))(*ab.tolist())

        def call(ts=(999, 0), eta=0.0, sampler=1, clip=0.0, params=d, pred=0, B=4, P=2, mode=1, strength=1.0, **more):
            ts_c = (ctypes.c_int32 * len(ts))(*ts)
            q = N.sample_call(alpha_bars_host=ctypes.addressof(ab_c), num_timesteps=len(ab), x_T=D, ms2_cond=D, ms1_cond=D, auto_normalize=1,
                              pred_type=pred, timesteps_host=ctypes.addressof(ts_c), num_steps=len(ts), out_x=D, out_noise=D, workspace=D,
                              workspace_bytes=1 << 40, B=B, RT=8, eta=eta, seed_dev=D, sampler=sampler, clip_x0=clip, group_size=P,
                              consistency=mode, consistency_strength=strength, **more)
            return lib.dq_ddim_sample(plan, params, d, ctypes.byref(q))

        own = ((dict(P=0), b"group_size must be 1..8"), (dict(P=9), b"group_size must be 1..8"), (dict(P=3), b"whole number of groups"),
               (dict(mode=3), b"unknown consistency mode"), (dict(mode=-1), b"unknown consistency mode"),
               (dict(strength=0.0), b"0 < strength <= 1"), (dict(strength=1.25), b"0 < strength <= 1"), (dict(strength=NAN), b"0 < strength <= 1"))
        theirs = ((dict(params=None), b"null argument"), (dict(eta=1.5), b"eta must satisfy"), (dict(sampler=7), b"unknown sampler"),
                  (dict(eta=0.5, sampler=2), b"eta must be 0"), (dict(clip=1.0, sampler=0), b"clip_x0 needs the ddim or dpmpp_2m sampler"),
                  (dict(clip=1.0, eta=0.5), b"clip_x0 needs eta == 0"), (dict(ts=(999, 999)), b"strictly decreasing"),
                  (dict(pred=3), b"Unknown pred_type"), (dict(B=0), b"need B, RT > 0"), (dict(ts=(999,) + tuple(range(998, -27, -1))), b"num_steps <= 1024"))
        for kw, word in theirs + own:
            assert call(**kw) != 0, kw
            err = lib.dq_last_error()
            assert word in err and err.startswith(b"dq_ddim_sample: "), (kw, err)
        # the refusals that need no group and no device, the batch and step counts included, come before every one of the group's own
        for kw, word in theirs:
            for kw2, _ in own:
                if set(kw) & set(kw2):
                    continue
                assert call(**kw, **kw2) != 0 and word in lib.dq_last_error(), (kw, kw2, lib.dq_last_error())
        # and its own in the order stated: the group size, the batch, the mode, the strength
        assert call(P=9, mode=3, strength=NAN) != 0 and b"group_size must be 1..8" in lib.dq_last_error()
        assert call(P=3, mode=3, strength=NAN) != 0 and b"whole number of groups" in lib.dq_last_error()
        assert call(mode=3, strength=NAN) != 0 and b"unknown consistency mode" in lib.dq_last_error()
        # the v objective is this entry's: refused only behind it
        assert call(pred=2, P=9) != 0 and b"group_size" in lib.dq_last_error()
        # what no entry could express is refused here, on the host: consistency together with guidance or a live per-window option (the
        # reason is sample()'s), behind every refusal that needs no group and in front of the group's own; without consistency the same
        # records pass every host check and end at the workspace (the plan's tables would go to the device first: not asked for here)
        scratch = dict(stat_scratch=D, stat_scratch_bytes=1 << 30)
        together = (dict(guided=1, guidance_scale=2.0), dict(guidance_rescale=0.5), dict(guidance_rescale=0.25, guided=1, guidance_scale=2.0, **scratch),
                    dict(threshold_quantile=0.5, threshold_max=2.0, **scratch))
        reason = b"consistency together with guided, guidance_rescale or threshold_quantile is not implemented (follow-up: the guided form"
        for more in together:
            assert call(**more) != 0
            err = lib.dq_last_error()
            assert err.startswith(b"dq_ddim_sample: " + reason), (more, err)
            assert call(P=9, mode=3, strength=NAN, **more) != 0 and reason in lib.dq_last_error(), more  # in front of the group's own
            for kw, word in theirs:
                assert call(**kw, **more) != 0 and word in lib.dq_last_error(), (kw, more, lib.dq_last_error())  # behind the others
        assert call(guided=1, guidance_scale=NAN) != 0 and b"guidance scale must be finite" in lib.dq_last_error()
        assert call(guidance_rescale=1.5) != 0 and b"guidance_rescale must satisfy" in lib.dq_last_error()
    finally:
        lib.dq_plan_destroy(plan)


def test_abi_has_the_two_entries():
    from dquartic import _native as N
    from test_abi import declared

    decl = declared()
    assert decl["dq_group_project"] == 13 and "dq_ddim_sample_joint" not in decl and decl["dq_ddim_sample"] == 4
    # the group options are the record's last three fields (their layout: test_abi.test_sample_call_layout_is_the_librarys)
    assert N.SampleCall._fields_[-3:] == [("group_size", ctypes.c_int32), ("consistency", ctypes.c_int32), ("consistency_strength", ctypes.c_float)]
    assert N.lib().dq_abi_version() == N.ABI_VERSION == 13
    assert N.CONSISTENCY_MODES == R.MODES and N.GROUP_MAX == 8
    header = open(inspect.getsourcefile(declared).replace("tests/test_abi.py", "include/dq_hip.h")).read()
    assert "DQ_CONSIST_NONE = 0, DQ_CONSIST_BOUND = 1, DQ_CONSIST_SUM = 2" in header and "#define DQ_GROUP_MAX 8" in header


# ---------------------------------------------------------------------------------------------------------------- the Python surface
KW = dict(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)


def _dm():
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    return DDIMDiffusionModel(model_class=UNet1d(**KW), device="cpu")


def test_python_argument_checks_and_the_three_named_refusals():
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    dm = _dm()
    x, c2, c1 = torch.zeros(4, 8, 8), torch.zeros(4, 8, 8), torch.zeros(4, 8)
    for bad in (0, 9, -1, 2.0, "2", True, [2]):
        with pytest.raises(ValueError, match="group_size"):
            dm.sample(x, c2, c1, num_steps=2, group_size=bad, consistency="bound")
        with pytest.raises(ValueError, match="group_size"):
            dm.sample(x, c2, c1, num_steps=2, group_size=bad)  # checked without a consistency too
    for bad in ("bounded", "BOUND", 1, True):
        with pytest.raises(ValueError, match="Unknown consistency"):
            dm.sample(x, c2, c1, num_steps=2, group_size=2, consistency=bad)
    for bad in (0.0, -0.5, 1.0001, NAN, INF, 1e-60, "full", [0.5], None):  # (1e-60 is 0 as the float32 the kernel takes it as)
        with pytest.raises(ValueError, match="consistency_strength"):
            dm.sample(x, c2, c1, num_steps=2, group_size=2, consistency="sum", consistency_strength=bad)
    with pytest.raises(ValueError, match="whole number of groups"):
        dm.sample(x, c2, c1, num_steps=2, group_size=3, consistency="bound")
    with pytest.raises(ValueError, match="whole number of groups"):
        dm.sample(None, c2, c1, num_steps=2, seed=1, shape=(5, 8, 8), group_size=2)
    assert dm._check_joint(None, None, 1.0) is None and dm._check_joint(4, None, 0.5) is None
    assert dm._check_joint(None, "bound", 1) == (1, 1, 1.0) and dm._check_joint(8, "sum", 0.3) == (8, 2, float(F(0.3)))
    with pytest.raises(ValueError, match="eta"):
        dm.sample(x, c2, c1, num_steps=2, group_size=2, consistency="bound", sampler="dpmpp_2m", eta=0.5)  # the earlier refusals keep their place
    # refused by name, with the follow-up stated: together with guidance and the per-window options ...
    for kw in (dict(guidance_scale=3.0), dict(guidance_scale=3.0, guidance_rescale=0.5), dict(sampler="ddim", threshold_quantile=0.9)):
        with pytest.raises(NotImplementedError, match="consistency together with guidance_scale, guidance_rescale or threshold_quantile.*follow-up"):
            dm.sample(x, c2, c1, num_steps=2, group_size=2, consistency="bound", **kw)
    # ... on the generic host loop ...
    with pytest.raises(NotImplementedError, match="group_size / consistency need the native sampler"):
        dm.sample(x, c2, c1, num_steps=2, group_size=2, consistency="bound")
    with pytest.raises(NotImplementedError, match="native sampler"):
        dm.sample(x, c2, c1, num_steps=2, consistency="sum")  # groups of one
    # ... and on the CustomTransformer
    tfm = DDIMDiffusionModel(model_class=DDIMTransformerAdapter(CustomTransformer(input_dim=8, hidden_dim=8, num_heads=1, num_layers=1)),
                             device="cpu")
    with pytest.raises(NotImplementedError, match=r"dq_ddim_sample\).*CustomTransformer.*follow-up"):
        tfm.sample(x, c2, c1, num_steps=2, group_size=2, consistency="bound")


def test_options_record():
    from dquartic.model.model import JointSampleOptions, SampleOptions
    from dquartic.model.model_interface import ModelInterface, _reported_options, _sampler_kwargs

    dm = _dm()
    assert issubclass(JointSampleOptions, SampleOptions) and JointSampleOptions().non_default() == {}
    assert JointSampleOptions(group_size=3).non_default() == {"group_size": 3}
    assert JointSampleOptions(consistency="sum").non_default() == {"consistency": "sum"}
    assert JointSampleOptions(consistency_strength=0.5).non_default() == {"consistency_strength": 0.5}
    full = JointSampleOptions(sampler="ddim", clip_x0=2.0, group_size=4, consistency="bound", consistency_strength=0.25)
    assert full.non_default() == dict(sampler="ddim", clip_x0=2.0, group_size=4, consistency="bound", consistency_strength=0.25)
    assert full.resolve(0.0, dm) == SampleOptions(sampler="ddim", clip_x0=2.0).resolve(0.0, dm)  # the older options resolve as they did
    assert full.resolve_joint(dm) == (4, 1, 0.25) and JointSampleOptions(group_size=4).resolve_joint(dm) is None
    assert JointSampleOptions(consistency="sum").resolve_joint(dm) == (1, 2, 1.0)  # consistency without group_size: P = 1
    with pytest.raises(ValueError, match="group_size"):
        JointSampleOptions(group_size=9).resolve_joint(dm)
    assert _sampler_kwargs("reference", None, group_size=2, consistency="bound") == {"group_size": 2, "consistency": "bound"}
    shown = _reported_options({"sampler": "ddim", "group_size": 2, "consistency": "sum", "consistency_strength": 1})
    assert shown == {"sampler": "ddim", "group_size": 2, "consistency": "sum", "consistency_strength": 1.0} and type(shown["group_size"]) is int
    # keyword parameters of sample / predict / _predict_one_batch at the defaults that mean "off"
    for fn in (type(dm).sample, ModelInterface.predict, ModelInterface._predict_one_batch):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("group_size", "consistency", "consistency_strength")] == [None, None, 1.0], fn.__name__
    p = inspect.signature(ModelInterface.deconvolve_run_joint).parameters
    assert p["consistency"].default == "bound" and p["consistency_strength"].default == 1.0 and p["step"].default == 5


def test_entry_choice(monkeypatch):
    """a live consistency sets (group_size, consistency, consistency_strength) in the record beside what the call sets anyway, and every
    other option holds its off value; without one the call is the one it always was, whatever group_size says"""
    from dquartic.model.model import DDIMDiffusionModel
    from test_sample_loop import STEPS, _host_model, _options, _shared

    rec, dm, inputs, _ = _host_model(monkeypatch)
    keep = [dm._sample_native(*inputs, STEPS), dm._sample_native(*inputs, STEPS, eta=0.0, sampler=1, clip_x0=1.5, joint=(2, 1, 0.5)),
            dm._sample_native(*inputs, STEPS, eta=0.5, seed=7, joint=(1, 2, 1.0))]
    assert [name for name, _ in rec.calls] == ["dq_ddim_sample"] * 3 and len(keep) == 3
    a0, a1, a2 = (fields for _, fields in rec.calls)
    _options(a0)
    _options(a1, sampler=dict(sampler=1, clip_x0=1.5), joint=dict(group_size=2, consistency=1, consistency_strength=0.5))
    assert a2["eta"] == 0.5 and isinstance(a2["seed_dev"], int) and a2["seed_dev"] != 0
    _options(a2, noise=dict(eta=0.5, seed_dev=a2["seed_dev"], window_ids_dev=None), joint=dict(group_size=1, consistency=2, consistency_strength=1.0))
    assert _shared(a1) == _shared(a0) == _shared(a2)
    # sample(): which options reach _sample_native
    seen = []
    monkeypatch.setattr(DDIMDiffusionModel, "_sample_native", lambda self, *a, **kw: seen.append(kw) or (None, None))
    dm.model = _dm().model  # a UNet1d: the native route

    class Cuda:  # stands in for a device tensor: .is_cuda and .shape are all that is read before the native call
        is_cuda, shape = True, (4, 8, 8)

    t = Cuda()
    for extra in (dict(), dict(group_size=2), dict(group_size=4, consistency=None, consistency_strength=0.5)):
        seen.clear()
        dm.sample(t, t, t, num_steps=2, **extra)
        assert len(seen) == 1 and "joint" not in seen[0] and seen[0]["eta"] is None, (extra, seen)  # the default call
    seen.clear()
    dm.sample(t, t, t, num_steps=2, group_size=2, consistency="sum", consistency_strength=0.5)
    assert seen[0]["joint"] == (2, 2, 0.5) and seen[0]["eta"] == 0.0 and seen[0]["guidance"] is None and "adaptive" not in seen[0]
    seen.clear()
    dm.sample(t, t, t, num_steps=2, consistency="bound", guidance_scale=1.0, guidance_rescale=0.7)  # (scale 1 is the conditional model: no guidance)
    assert seen[0]["joint"] == (1, 1, 1.0)


def test_member_major_ids():
    from dquartic.model.model_interface import ModelInterface

    ids = ModelInterface.joint_window_ids
    assert ids(0, 4, 3, 0, 4).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]       # one batch: member p, window i -> p n + i
    assert ids(0, 4, 3, 1, 2).tolist() == [1, 2, 5, 6, 9, 10]                           # windows 1, 2 of every member
    assert ids(100, 7, 2, 5, 2).tolist() == [105, 106, 112, 113] and ids(5, 3, 1, 0, 3).tolist() == [5, 6, 7]
    assert ids(0, 4, 3, 0, 4).dtype == np.int64
    n, P = 7, 3
    for bs in (1, 2, 3, 7):  # whatever the batch size, member p's windows carry id_offset + p n + i: member 0 the ids of deconvolve_run
        got = {p: [] for p in range(P)}
        for i0 in range(0, n, bs):
            G = min(bs, n - i0)
            batch = ids(10, n, P, i0, G).reshape(P, G)
            for p in range(P):
                got[p] += batch[p].tolist()
        assert all(got[p] == list(range(10 + p * n, 10 + (p + 1) * n)) for p in range(P)), bs
    # the first 2^31 ids do not wrap
    assert ids(2 ** 40, 2 ** 20, 2, 0, 1).tolist() == [2 ** 40, 2 ** 40 + 2 ** 20]


def test_deconvolve_run_joint_refuses_before_the_device():
    dm = _dm()
    ms2 = torch.zeros(8, 8)
    with pytest.raises(TypeError, match="deconvolve_run_joint: unknown option"):
        dm.deconvolve_run_joint(ms2, torch.zeros(2, 8), window=4, threshold=0.9)
    with pytest.raises(ValueError, match=r"ms1_runs must be \(P, RT_total\) or \(P, RT_total, M1\)"):
        dm.deconvolve_run_joint(ms2, torch.zeros(8), window=4)
    with pytest.raises(ValueError, match="ms1_runs must be"):
        dm.deconvolve_run_joint(ms2, torch.zeros(2, 7), window=4)
    with pytest.raises(ValueError, match="ms1_runs has 2 channel"):
        dm.deconvolve_run_joint(ms2, torch.zeros(2, 8, 2), window=4)
    with pytest.raises(ValueError, match="window"):
        dm.deconvolve_run_joint(ms2, torch.zeros(2, 8))
    with pytest.raises(NotImplementedError, match="deconvolve_run_joint runs in the native library only"):
        dm.deconvolve_run_joint(ms2, torch.zeros(2, 8), window=4, step=2)
    with pytest.raises(NotImplementedError, match="deconvolve_run runs in the native library only"):
        dm.deconvolve_run(ms2, torch.zeros(8), window=4, step=2)  # (the single-trace call refuses under its own name, as it did)


def test_cli_argument_shapes(tmp_path):
    from click.testing import CliRunner

    from dquartic import cli

    for cmd in (cli.evaluate, cli.deconvolve):
        opts = {o.name: o for o in cmd.params}
        assert opts["consistency"].default is None and opts["consistency_strength"].default == 1.0
        assert "--consistency" in opts["consistency"].opts and "--consistency-strength" in opts["consistency_strength"].opts
        bad = CliRunner().invoke(cli.cli, [cmd.name, "--consistency", "tight"])
        assert bad.exit_code == 2 and "consistency" in bad.output
    assert "joint" in {o.name for o in cli.deconvolve.params} and "joint" not in {o.name for o in cli.evaluate.params}
    source = inspect.getsource(cli)
    for flag in ("--consistency", "--consistency-strength", "--joint"):  # declared once
        assert source.count(f'click.option("{flag}"') == 1, flag
    # what the decorator hands a command body: the two options when live, nothing at the defaults; group_size is not a flag
    command = cli.sampling_options(lambda **kw: kw)
    base = dict(sampler="reference", clip_x0=None, guidance_scale=None, null_ms1=0.0, guidance_rescale=0.0, threshold_quantile=None, threshold_max=None)
    assert command(eta=0.0, seed=0, consistency=None, consistency_strength=1.0, **base) == dict(eta=0.0, seed=0, sample_kw={})
    assert command(eta=0.0, seed=0, consistency="sum", consistency_strength=0.5, **base)["sample_kw"] == dict(consistency="sum", consistency_strength=0.5)
    # the shapes of --joint, refused before a device is asked for
    cfg, ck = str(tmp_path / "c.json"), str(tmp_path / "m.ckpt")
    assert CliRunner().invoke(cli.cli, ["generate-config", cfg]).exit_code == 0
    open(ck, "wb").close()
    p2, p1, out = str(tmp_path / "ms2.npy"), str(tmp_path / "ms1.npy"), str(tmp_path / "o.npz")

    def run(ms2, ms1, *flags):
        np.save(p2, ms2.astype(np.float32))
        np.save(p1, ms1.astype(np.float32))
        r = CliRunner().invoke(cli.cli, ["deconvolve", "--checkpoint", ck, "--ms2", p2, "--ms1", p1, "--out", out, "--window", "4", *flags, cfg])
        assert r.exit_code == 1, (r.output, r.exception)  # a ClickException, not a usage error or a traceback
        return r.output

    z = np.zeros
    assert "--joint expects one run (RT_total, MZ)" in run(z((2, 12, 8)), z((3, 12)), "--joint")
    assert "--joint expects (P, RT_total) or (P, RT_total, M1) with RT_total = 12" in run(z((12, 8)), z(12), "--joint")
    assert "with RT_total = 12" in run(z((12, 8)), z((3, 11)), "--joint")
    assert "with RT_total = 12" in run(z((12, 8)), z((3, 11, 1)), "--joint")
    assert "1 .. 8 members, got 9" in run(z((12, 8)), z((9, 12)), "--joint")
    assert "need 1 <= --step <= --window <= RT_total" in run(z((3, 8)), z((2, 3)), "--joint")
    assert "need --joint" in run(z((12, 8)), z(12), "--consistency", "bound")
    assert "need --joint" in run(z((12, 8)), z(12), "--consistency-strength", "0.5")
    # without --joint a (P, RT_total) MS1 against one run is what it was: a shape error of the single-trace call
    assert "--ms1: expected (RT_total,)" in run(z((12, 8)), z((3, 12)))
    r = CliRunner().invoke(cli.cli, ["evaluate", "--checkpoint", ck, "--consistency", "bound", cfg])
    assert r.exit_code == 1 and "groups inside evaluate are not implemented" in r.output and "follow-up" in r.output
    assert json.load(open(cfg))["model"]["use_model"] == "UNet1d"
