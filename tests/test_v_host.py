"""The v-prediction objective (pred_type="v_prediction") where no GPU is needed: the name and its enum value, the
all-ones loss weight, the refusals made in Python and by the C entries before anything touches the device, the config loader, and the host /
autograd arm of p_sample in float64."""
import ctypes
import json

import pytest
import torch

KW = dict(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)


def _dm(**kw):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    return DDIMDiffusionModel(model_class=UNet1d(**KW), device="cpu", **kw)


def test_the_name_and_the_loss_weight():
    from dquartic import _native as N

    assert N.PRED_TYPES == {"eps": 0, "x0": 1, "v_prediction": 2}
    dm = _dm(pred_type="v_prediction")
    assert dm.pred_type == "v_prediction"
    assert torch.equal(dm.loss_weight, torch.ones(1000))
    with pytest.raises(ValueError, match="Unknown pred_type"):
        _dm(pred_type="v")  # the short name stays an unknown objective


def test_other_networks_and_the_ms1_term_are_refused_by_name():
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    tfm = DDIMTransformerAdapter(CustomTransformer(input_dim=8, hidden_dim=8, num_heads=1, num_layers=1))
    for net in (tfm, torch.nn.Linear(4, 4)):
        with pytest.raises(NotImplementedError, match="UNet1d only.*CustomTransformer"):
            DDIMDiffusionModel(model_class=net, num_timesteps=20, device="cpu", pred_type="v_prediction")
        DDIMDiffusionModel(model_class=net, num_timesteps=20, device="cpu", pred_type="x0")  # (the refusal is the objective's, not the network's)
    with pytest.raises(NotImplementedError, match="ms1_loss_weight > 0 with pred_type 'v_prediction'"):
        _dm(pred_type="v_prediction", ms1_loss_weight=0.25)
    dm = _dm(pred_type="v_prediction")
    x = torch.zeros(1, 4, 8)
    for step in (dm.train_step, dm.train_step_fused):  # the per-call weight is refused before anything is staged
        with pytest.raises(NotImplementedError, match="ms1_loss_weight > 0 with pred_type 'v_prediction'"):
            step(x, x, torch.zeros(1, 4), ms1_loss_weight=0.25)


def test_the_c_entries_refuse_by_message():
    """null pointers throughout: every call here must be refused before it reads an operand"""
    from dquartic import _native as N

    lib = N.lib()
    f = ctypes.c_float

    def train(pred, w):
        return lib.dq_train_step(None, None, None, None, None, None, None, None, None, 1, pred, None, f(w), None, None, None, 0, 1, 1, None)

    def evals(pred):
        return lib.dq_eval_step(None, None, None, None, None, None, None, None, None, 1, pred, None, None, None, None, 0, 1, 1, None)

    for rc, word in ((lambda: train(7, 0.0), b"dq_train_step: Unknown pred_type"), (lambda: train(3, 0.0), b"dq_train_step: Unknown pred_type"),
                     (lambda: train(-1, 0.0), b"dq_train_step: Unknown pred_type"),
                     (lambda: train(2, 0.25), b"ms1_loss_weight > 0 with pred_type v_prediction is not built"),
                     (lambda: train(2, 0.0), b"dq_train_step: null argument"),  # (the objective itself is known)
                     (lambda: evals(7), b"dq_eval_step: Unknown pred_type"), (lambda: evals(2), b"dq_eval_step: null argument")):
        assert rc() != 0
        assert word in lib.dq_last_error(), lib.dq_last_error()
    d = ctypes.c_void_p(4096)
    # the stand-alone updates whose pred_type names the reference's two objectives refuse DQ_PRED_V (2) as they always did: their v forms are entries of their own
    named = {
        "dq_solver_step": lambda p: lib.dq_solver_step(d, d, d, None, None, d, f(0.0), p, 8, None),
        "dq_guided_update": lambda p: lib.dq_guided_update(0, d, d, d, d, None, None, None, d, f(1.0), f(0.0), None, d, 1, p, 1, 8, None),
    }
    for name, fn in named.items():
        for p in (2, 3, 7, -1):
            assert fn(p) != 0, (name, p)
            assert name.encode() + b": Unknown pred_type" in lib.dq_last_error(), (name, p, lib.dq_last_error())
    for p in (3, 7, -1):  # (this one takes the value 2)
        assert lib.dq_ddim_step_sto(d, d, d, None, d, None, d, 1, p, 1, 8, None) != 0
        assert b"dq_ddim_step_sto: Unknown pred_type" in lib.dq_last_error()
    from test_sampler_tables import dummy_record

    ab = (ctypes.c_float * 4)(0.9, 0.8, 0.7, 0.6)
    ts = (ctypes.c_int32 * 1)(3)

    # every required pointer there (never read: the objective is refused first), so the objective is what is refused
    def loop_v(pred, **kw):
        return lib.dq_ddim_sample(d, d, d, ctypes.byref(dummy_record(ab, ts, pred_type=pred, RT=1, seed_dev=None, **kw)))

    def loop_tfm(pred):
        return lib.dq_tfm_sample(d, d, d, d, d, 4, ctypes.byref(dummy_record(ab, ts, pred_type=pred, RT=1, seed_dev=None)))

    for p in (3, 7, -1):
        assert loop_v(p) != 0
        assert b"dq_ddim_sample: Unknown pred_type" in lib.dq_last_error(), lib.dq_last_error()
    # the transformer's entry refuses v, the U-Net's takes it: the same record gets past the objective there, to the next refusal
    for p in (2, 3, 7, -1):
        assert loop_tfm(p) != 0
        assert b"dq_tfm_sample: Unknown pred_type" in lib.dq_last_error(), lib.dq_last_error()
    assert loop_v(2, B=0) != 0 and b"dq_ddim_sample: need B, RT > 0" in lib.dq_last_error(), lib.dq_last_error()
    assert loop_v(2, guided=1, guidance_scale=-1.0) != 0 and b"dq_ddim_sample: the guidance scale" in lib.dq_last_error()
    # the v entries refuse like the entries they mirror, under their own names
    nulls = {
        "dq_ddim_step_v": lambda: lib.dq_ddim_step_v(None, None, None, None, None, 8, None),
        "dq_solver_step_v": lambda: lib.dq_solver_step_v(None, None, None, None, None, None, f(0.0), 8, None),
        "dq_guided_update_v": lambda: lib.dq_guided_update_v(0, None, None, None, None, None, None, None, None, f(1.0), f(0.0), None, None, 1, 1, 8, None),
        "dq_ddim_sample": lambda: lib.dq_ddim_sample(None, None, None, ctypes.byref(N.sample_call(num_timesteps=1000, pred_type=2, num_steps=1, B=1, RT=1))),
        "dq_mse_loss_v_fwd_bwd": lambda: lib.dq_mse_loss_v_fwd_bwd(None, None, None, None, f(2.0), f(-1.0), None, None, None, None, None, 3, 8, None),
    }
    for name, fn in nulls.items():
        assert fn() != 0, name
        assert name.encode() + b": null argument" in lib.dq_last_error(), (name, lib.dq_last_error())
    assert lib.dq_mse_per_window_v(None, None, None, None, f(2.0), f(-1.0), None, None, None, None, None, 3, 8, None) != 0
    for kw, word in ((dict(kind=4), b"dq_guided_update_v: unknown update kind"), (dict(kind=3), b"dq_guided_update_v: the 2M update needs the x0 history"),
                     (dict(w=-0.5), b"dq_guided_update_v: the guidance scale"), (dict(B=-1), b"dq_guided_update_v: negative size")):
        a = dict(kind=0, w=1.0, B=1)
        a.update(kw)
        assert lib.dq_guided_update_v(a["kind"], d, d, d, d, None, None, None, d, f(a["w"]), f(0.0), None, d, 1, a["B"], 8, None) != 0, kw
        assert word in lib.dq_last_error(), (kw, lib.dq_last_error())
    assert lib.dq_mse_loss_v_fwd_bwd(d, d, d, d, f(1.0), f(0.0), None, d, d, None, d, 0, 8, None) != 0
    assert b"B and per must be positive" in lib.dq_last_error()
    assert ctypes.c_int(lib.dq_abi_version()).value == N.ABI_VERSION == 13


def test_the_config_loader_knows_the_objective(tmp_path):
    from dquartic.utils.config_loader import generate_train_config, load_train_config

    path = tmp_path / "train.json"
    generate_train_config(str(path))
    cfg = json.loads(path.read_text())
    assert load_train_config(str(path))["model"]["pred_type"] == "eps"
    for name in ("x0", "v_prediction"):
        cfg["model"]["pred_type"] = name
        path.write_text(json.dumps(cfg))
        assert load_train_config(str(path))["model"]["pred_type"] == name
    for name in ("v", "V_PREDICTION", None):
        cfg["model"]["pred_type"] = name
        path.write_text(json.dumps(cfg))
        with pytest.raises(ValueError, match="Unknown pred_type"):
            load_train_config(str(path))


class _Stub(torch.nn.Module):
    """a network that returns the v of known (x0, eps) at the timestep it is asked for"""

    def __init__(self, ab, x0, eps):
        super().__init__()
        self.ab, self.x0, self.eps = ab, x0, eps

    def forward(self, x_t, t, init_cond=None, attn_cond=None):
        a = self.ab[int(t[0])]
        return torch.sqrt(a) * self.eps - torch.sqrt(1.0 - a) * self.x0


def test_p_sample_host_arm_in_float64():
    dm = _dm(pred_type="v_prediction")
    dm.alpha_bars = dm.alpha_bars.double()  # the host arm is tensor expressions: float64 in, float64 through
    g = torch.Generator().manual_seed(3)
    x0 = torch.rand(3, 4, 8, generator=g, dtype=torch.float64) * 2 - 1
    eps = torch.randn(3, 4, 8, generator=g, dtype=torch.float64)
    dm.model = _Stub(dm.alpha_bars, x0, eps)
    for t in (999, 500, 1, 0):
        a = dm.alpha_bars[t]
        x_t = torch.sqrt(a) * x0 + torch.sqrt(1.0 - a) * eps
        xp, ep = dm.p_sample(x_t, t)
        assert xp.dtype == torch.float64
        want = x0 if t == 0 else torch.sqrt(dm.alpha_bars[t - 1]) * x0 + torch.sqrt(1.0 - dm.alpha_bars[t - 1]) * eps
        assert float((xp - want).abs().max()) < 1e-13, t
        assert float((ep - eps).abs().max()) < 1e-13, t
    # ... and it carries autograd history: d x_prev / d x_t at t = 0 is sa (x0 = sa x_t - sb v)
    x_t = (torch.sqrt(dm.alpha_bars[0]) * x0 + torch.sqrt(1.0 - dm.alpha_bars[0]) * eps).requires_grad_(True)
    xp, _ = dm.p_sample(x_t, 0)
    xp.sum().backward()
    assert float((x_t.grad - torch.sqrt(dm.alpha_bars[0])).abs().max()) < 1e-15
