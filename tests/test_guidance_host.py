"""Classifier-free guidance on MS1, everything that needs no device: the refusals of ``dq_guided_update``,
``dq_ms1_cond_drop`` and ``dq_ddim_sample`` with the guidance fields (dummy pointers, never dereferenced: each refusal names its reason and nothing is
launched), the Python surface's refusals, the train config's ``model.cond_drop_prob``, the unchanged ``generate-config`` output and
checkpoint key set, and this file's numpy transcription of the drop rule of ``k_cond_drop`` (over the Philox transcription of
tests/test_stochastic_sampler.py), which the GPU tests compare the kernel with.

The drop rule: window b (id = ids[b], or b) of draw d under seed s is replaced by the null iff the THIRD output word of
philox4x32_10((0, d, id lo, id hi), (s lo, s hi)) is below floor(p 2^32)."""
import ctypes
import inspect
import json
import math

import numpy as np
import pytest
import torch

from test_stochastic_sampler import SEED, philox4x32_10

_MASK = 0xFFFFFFFF
DROP_P = 0.5  # the probability the GPU tests train and drop with, under SEED


# ---------------------------------------------------------------------------------------------------------------- transcription
def drop_threshold(p):
    return int(math.floor(float(p) * 4294967296.0))


def drop_mask(seed, ids, draw, p):
    """(B,) bool: which windows the kernel replaces"""
    ids = np.asarray([int(i) & (2 ** 64 - 1) for i in ids], dtype=np.uint64)
    z = np.zeros_like(ids)
    seed = int(seed) & (2 ** 64 - 1)
    r = philox4x32_10((z, np.full_like(ids, draw), ids & np.uint64(_MASK), ids >> np.uint64(32)),
                      (np.full_like(ids, seed & _MASK), np.full_like(ids, seed >> 32)))
    return np.asarray(r[2]) < np.uint64(drop_threshold(p))


def cond_drop_ref(ms1, seed, ids, draw, p, null_value):
    """what dq_ms1_cond_drop returns for ms1 (B, ...): dropped windows are null_value in every element, kept ones bit copies"""
    out = np.array(ms1, dtype=np.float32, copy=True)
    out[drop_mask(seed, ids, draw, p)] = np.float32(null_value)
    return out


def test_drop_rule_transcription():
    ids = np.arange(5)
    assert drop_threshold(0.0) == 0 and drop_threshold(0.5) == 1 << 31 and drop_threshold(1 - 2.0 ** -40) == (1 << 32) - 1
    for d in range(8):
        assert not drop_mask(SEED, ids, d, 0.0).any()  # p = 0 drops nothing, whatever the word
    m = drop_mask(SEED, ids, 0, DROP_P)
    assert 1 <= int(m.sum()) <= 4, m  # the seed of the GPU tests, B = 5, p = 0.5: at least one dropped, at least one kept
    assert any(not np.array_equal(drop_mask(SEED, ids, d, DROP_P), m) for d in (1, 2, 3))  # another draw, another pattern
    # the decision word is the third of the counter (0, d, id): the normals of the same seed read words 0 and 1 of counters (e, d, id)
    r = philox4x32_10((0, 3, 7, 0), (SEED & _MASK, SEED >> 32))
    assert bool(drop_mask(SEED, [7], 3, 0.25)[0]) == (int(r[2]) < (1 << 30))
    # a window decides under its id, wherever it sits
    assert drop_mask(SEED, [9, 2 ** 33 + 1, 4], 2, DROP_P)[1] == drop_mask(SEED, [2 ** 33 + 1], 2, DROP_P)[0]
    # the frequency is p (a Bernoulli, not a proof of one)
    big = drop_mask(SEED, np.arange(1 << 14), 0, 0.25)
    assert abs(big.mean() - 0.25) < 0.02
    x = np.arange(20, dtype=np.float32).reshape(5, 4)
    y = cond_drop_ref(x, SEED, ids, 0, DROP_P, -3.0)
    assert (y[m] == -3.0).all() and np.array_equal(y[~m], x[~m])


# ---------------------------------------------------------------------------------------------------------------- the C entries
def test_native_refusals_come_before_the_device():
    from dquartic import _native as N

    lib = N.lib()
    d = ctypes.c_void_p(4096)
    f = ctypes.c_float

    def upd(kind=0, x=d, c=d, u=d, xp=d, hist=None, coef=d, w=1.0, seed=d, pred=0, B=1, per=8):
        return lib.dq_guided_update(kind, x, c, u, xp, None, hist, None, coef, f(w), f(0.0), None, seed, 1, pred, B, per, None)

    for kw, word in ((dict(x=None), b"null argument"), (dict(c=None), b"null argument"), (dict(u=None), b"null argument"),
                     (dict(xp=None), b"null argument"), (dict(coef=None), b"null argument"), (dict(kind=4), b"unknown update kind"),
                     (dict(kind=-1), b"unknown update kind"), (dict(kind=1, seed=None), b"needs the seed"),
                     (dict(kind=3, hist=None), b"x0 history"), (dict(pred=2), b"Unknown pred_type"), (dict(w=-0.5), b"guidance scale"),
                     (dict(w=float("nan")), b"guidance scale"), (dict(w=float("inf")), b"guidance scale"), (dict(B=-1), b"negative size")):
        assert upd(**kw) != 0, kw
        assert word in lib.dq_last_error(), (kw, lib.dq_last_error())

    def drop(src=d, dst=d, seed=d, draw=0, p=0.5, B=1, per=4):
        return lib.dq_ms1_cond_drop(src, dst, None, seed, draw, ctypes.c_double(p), f(0.0), B, per, None)

    for kw, word in ((dict(src=None), b"null argument"), (dict(dst=None), b"null argument"), (dict(seed=None), b"null argument"),
                     (dict(p=1.0), b"0 <= p < 1"), (dict(p=-0.1), b"0 <= p < 1"), (dict(p=float("nan")), b"0 <= p < 1"),
                     (dict(draw=-1), b"draw index"), (dict(B=-1), b"negative size"), (dict(src=ctypes.c_void_p(4098)), b"4-byte aligned")):
        assert drop(**kw) != 0, kw
        assert word in lib.dq_last_error(), (kw, lib.dq_last_error())
    assert drop(B=0) == 0 and drop(per=0) == 0  # nothing to do: no launch

    dims = (ctypes.c_int * 2)(1, 2)
    plan = lib.dq_plan_create(4, 2, dims, 8, 1000)
    assert plan
    try:
        from test_sampler_tables import alpha_bars, dummy_record

        ab = alpha_bars("cosine")
        ab_c = (ctypes.c_float * len(ab))(*ab.tolist())

        def call(ts=(999, 0), eta=0.0, sampler=0, clip=0.0, w=2.0, params=d):
            ts_c = (ctypes.c_int32 * len(ts))(*ts)
            q = dummy_record(ab_c, ts_c, eta=eta, sampler=sampler, clip_x0=clip, guided=1, guidance_scale=w)
            return lib.dq_ddim_sample(plan, params, d, ctypes.byref(q))

        # sampler_check's refusals, in its order, under the entry's name; then the scale
        for kw, word in ((dict(params=None), b"null argument"), (dict(eta=1.5), b"eta must satisfy"), (dict(sampler=7), b"unknown sampler"),
                         (dict(eta=0.5, sampler=2), b"eta must be 0"), (dict(clip=1.0), b"clip_x0 needs the ddim"),
                         (dict(ts=(999, 999), sampler=1), b"strictly decreasing"), (dict(w=-1.0), b"guidance scale"),
                         (dict(w=float("nan")), b"guidance scale"), (dict(w=float("inf")), b"guidance scale")):
            assert call(**kw) != 0, kw
            err = lib.dq_last_error()
            assert word in err and err.startswith(b"dq_ddim_sample: "), (kw, err)
        assert call(sampler=7, w=-1.0) != 0 and b"unknown sampler" in lib.dq_last_error()  # (the sampler's refusal comes first)
        # the workspace a guided call needs is the unguided one of twice the batch; the entry point for it is unchanged
        assert lib.dq_unet_workspace_bytes(plan, 6, 4, 0) > lib.dq_unet_workspace_bytes(plan, 3, 4, 0) > 0
        assert lib.dq_unet_workspace_bytes(plan, 3, 4, 1) == 2 * lib.dq_unet_workspace_bytes(plan, 3, 4, 0)
    finally:
        lib.dq_plan_destroy(plan)
    assert N.UPDATE_KINDS == {"ddim": 0, "stochastic": 1, "solver_1": 2, "solver_2m": 3}


# ---------------------------------------------------------------------------------------------------------------- the Python surface
KW = dict(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)


def _dm(cls=None):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    return (cls or DDIMDiffusionModel)(model_class=UNet1d(**KW), device="cpu")


def test_python_surface_refusals():
    """raised on the host: the tensors are host tensors, nothing reaches the device"""
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.model_interface import ModelInterface

    dm = _dm()
    x, c2, c1 = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 8)
    for bad in (-1.0, -1e-9, float("nan"), float("inf"), 1e39, "high", [2.0]):
        with pytest.raises(ValueError, match="guidance_scale"):
            dm.sample(x, c2, c1, num_steps=2, guidance_scale=bad)
    assert dm._check_guidance(None) is None and dm._check_guidance(1.0) is None and dm._check_guidance(1) is None  # the call as it is today
    assert dm._check_guidance(0) == 0.0 and dm._check_guidance(3) == 3.0
    with pytest.raises(NotImplementedError, match="native sampler"):
        dm.sample(x, c2, c1, num_steps=2, guidance_scale=2.0)  # host tensors: the generic loop
    with pytest.raises(NotImplementedError, match="native sampler"):
        dm.sample(x, None, None, num_steps=2, guidance_scale=0.0)  # no conditions
    with pytest.raises(ValueError, match="eta"):
        dm.sample(x, c2, c1, num_steps=2, guidance_scale=2.0, sampler="dpmpp_2m", eta=0.5)  # the other refusals keep their place
    tfm = DDIMDiffusionModel(model_class=DDIMTransformerAdapter(CustomTransformer(input_dim=8, hidden_dim=8, num_heads=1, num_layers=1)),
                             device="cpu")
    with pytest.raises(NotImplementedError, match="follow-up"):
        tfm.sample(x, c2, c1, num_steps=2, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="UNet1d"):
        tfm.set_cond_dropout(0.1)

    class Generic(ModelInterface):  # a network the library does not run
        def __init__(self):
            super().__init__(device="cpu")
            self.build(torch.nn.Linear(2, 2))

    with pytest.raises(NotImplementedError, match="UNet1d"):
        Generic().set_cond_dropout(0.1)
    for bad in (1.0, 1.5, -0.1, float("nan"), "often"):
        with pytest.raises(ValueError, match="0 <= p < 1"):
            dm.set_cond_dropout(bad)
    assert not dm.cond_dropout_enabled  # off by default, and after every refusal
    dm.set_cond_dropout(0.25, seed=5, null_ms1=-1.0)
    assert dm.cond_dropout_enabled and (dm._cond_drop["p"], dm._cond_drop["seed"], dm._cond_drop["null_ms1"]) == (0.25, 5, -1.0)
    with pytest.raises(RuntimeError, match="device tensor"):
        dm._cond_drop_ms1(c1)  # the kernel is the only implementation
    dm.set_cond_dropout(0)
    assert not dm.cond_dropout_enabled
    Generic().set_cond_dropout(0.0)  # turning it off is always allowed
    # the new parameters are keyword parameters appended at the end
    for fn, tail in ((DDIMDiffusionModel.sample, ["guidance_scale", "null_ms1"]), (ModelInterface.predict, ["guidance_scale", "null_ms1"]),
                     (ModelInterface.evaluate, ["guidance_scale", "null_ms1"]), (ModelInterface._predict_one_batch, ["guidance_scale", "null_ms1"])):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == tail, (fn.__name__, names)
    from dquartic.model.model_interface import _sampler_kwargs

    assert _sampler_kwargs("reference", None) == {} and _sampler_kwargs("reference", None, None, 0.5) == {}
    assert _sampler_kwargs("ddim", 2.0, 3.0, 0.5) == {"sampler": "ddim", "clip_x0": 2.0, "guidance_scale": 3.0, "null_ms1": 0.5}


def test_config_and_cli(tmp_path):
    from click.testing import CliRunner

    from dquartic import cli
    from dquartic.utils.config_loader import generate_train_config, load_train_config

    p = str(tmp_path / "c.json")
    generate_train_config(p)
    raw = json.load(open(p))
    assert not any(k in raw["model"] for k in ("cond_drop_prob", "cond_drop_seed", "null_ms1"))  # generate-config writes what it wrote
    p2 = str(tmp_path / "via_cli.json")
    assert CliRunner().invoke(cli.cli, ["generate-config", p2]).exit_code == 0
    assert json.load(open(p2)) == raw
    dm = _dm()
    assert cli.enable_cond_dropout_from_config(dm, load_train_config(p)["model"]) is False and not dm.cond_dropout_enabled
    raw["model"].update(cond_drop_prob=0.1, cond_drop_seed=11, null_ms1=-0.5)
    json.dump(raw, open(p, "w"))
    m = load_train_config(p)["model"]
    assert cli.enable_cond_dropout_from_config(dm, m) is True
    assert (dm._cond_drop["p"], dm._cond_drop["seed"], dm._cond_drop["null_ms1"]) == (0.1, 11, -0.5)
    assert cli.enable_cond_dropout_from_config(dm, {**m, "cond_drop_prob": 0}) is False and not dm.cond_dropout_enabled
    dm.set_cond_dropout(0.1)
    assert dm._cond_drop["seed"] == 0 and dm._cond_drop["null_ms1"] == 0.0  # the defaults
    with pytest.raises(ValueError, match="0 <= p < 1"):
        cli.enable_cond_dropout_from_config(dm, {**m, "cond_drop_prob": 1.0})
    opts = {o.name: o for o in cli.evaluate.params}
    assert opts["guidance_scale"].default is None and opts["null_ms1"].default == 0.0
    assert "--guidance-scale" in opts["guidance_scale"].opts and "--null-ms1" in opts["null_ms1"].opts


def test_checkpoint_keys_unchanged_with_dropout_on(tmp_path):
    """training with conditioning dropout on writes the checkpoints it always wrote (a stubbed step: no device)"""
    from dquartic.model.model import DDIMDiffusionModel

    seen = []

    class Stub(DDIMDiffusionModel):
        def _train_one_batch(self, x_0, ms2_cond=None, ms1_cond=None, noise=None, ms1_loss_weight=0.0, **kw):
            seen.append(self.cond_dropout_enabled)
            return 0.5

    class DS(list):
        def reset_epoch(self):
            pass

    class Loader(list):
        dataset = DS()

    def keys(path):
        ck = torch.load(path, weights_only=False)
        return set(ck), set(ck["model_state_dict"]), set(ck["optimizer_state_dict"])

    z = torch.zeros(1, 8, 8)
    got = {}
    for on in (False, True):
        dm = _dm(Stub)
        if on:
            dm.set_cond_dropout(DROP_P, seed=SEED, null_ms1=0.25)
        d = tmp_path / ("on" if on else "off")
        d.mkdir()
        dm.train_with_warmup(Loader([(z, z[..., 0], z, z[..., 0])]), 2, 1, 1e-3, False, 100, str(d / "best.ckpt"))
        got[on] = (keys(str(d / "best.ckpt")), keys(str(d / "dquartic_latest_checkpoint.ckpt")))
    assert seen == [False, False, True, True]
    assert got[True] == got[False]
    assert got[True][0][0] == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "best_loss"}
