"""UNet1d(pos_output_only=True): Softplus behind final_conv (reference unet1d.py:1084, 1166) through every path that forms or
differentiates the network output -- the plain head (k_conv_fwd<1,1,0> + the recomputing backward), the fused training head and the
inference / sampling head of k_level_fwd (eager and hipGraph), the unfused train steps (x0 objective, the MS1 term), the CLI.

The oracle is the package's own (oracle/dq_oracle.py) with F.softplus applied to its network output; nn.Softplus is a single torch
primitive behind final_conv, so no reference fixture is needed.  Tolerances are those of tests/test_scale_parity.py."""
import ctypes
import json

import pytest
import torch
import torch.nn.functional as F
from torch import nn

GRAD_TOL = 2e-5
EPS_TOL = 1e-4
MULTS = (1, 2, 2, 3, 3, 4, 4)


def _unet(mz, pos, **kw):
    from dquartic.model.unet1d import UNet1d

    return UNet1d(dim=4, channels=1, dim_mults=MULTS, conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=mz,
                  simple=True, pos_output_only=pos, **kw)


def _net(mz, seed, perturb=0.05, bias_shift=0.0):
    torch.manual_seed(seed)
    net = _unet(mz, True)
    with torch.no_grad():  # every tensor off its init (as tests/test_scale_parity.py::_net)
        for p in net.parameters():
            if p.requires_grad:
                p.add_(perturb * torch.randn_like(p))
        net.final_conv.bias.add_(bias_shift)
    params = {k: v.detach().clone().cpu() for k, v in net.state_dict().items()}
    return net, params


def _softplus_diffusion(**kw):
    from oracle import dq_oracle as O

    class SoftplusDiffusion(O.Diffusion):
        def net(self, x_t, t, ms2_cond, ms1_cond):
            return F.softplus(super().net(x_t, t, ms2_cond, ms1_cond))

    return SoftplusDiffusion(**kw)


def _check_grads(named_grads, po, tol=GRAD_TOL):
    from oracle import dq_oracle as O

    keys = O.trainable_keys(po)
    assert len(keys) == 395
    gmax = max(float(po[k].grad.abs().max()) for k in keys)
    worst = ("", 0.0)
    for k in keys:
        ref = po[k].grad
        e = float((named_grads[k].cpu().to(ref.dtype) - ref).abs().max()) / max(float(ref.abs().max()), 1e-4 * gmax)
        if e > worst[1]:
            worst = (k, e)
    assert worst[1] <= tol, worst
    return worst


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_abi_final_act_setting_and_workspace():
    from dquartic import _native as N

    lib = N.lib()
    mults = (ctypes.c_int * len(MULTS))(*MULTS)
    for mz, B, RT in ((64, 32, 400), (256, 8, 2000)):
        plan = lib.dq_plan_create(4, len(MULTS), mults, mz, 1000)
        assert plan
        try:
            assert lib.dq_plan_final_act(plan) == 0
            ws = [lib.dq_unet_workspace_bytes(plan, B, RT, tr) for tr in (0, 1)]
            assert lib.dq_plan_set_final_act(plan, 1) == 0 and lib.dq_plan_final_act(plan) == 1
            assert [lib.dq_unet_workspace_bytes(plan, B, RT, tr) for tr in (0, 1)] == ws
            for bad in (2, -1):
                assert lib.dq_plan_set_final_act(plan, bad) != 0
                assert b"dq_plan_set_final_act" in lib.dq_last_error()
                assert lib.dq_plan_final_act(plan) == 1  # (a rejected value leaves the setting alone)
            assert lib.dq_plan_set_final_act(plan, 0) == 0 and lib.dq_plan_final_act(plan) == 0
            assert [lib.dq_unet_workspace_bytes(plan, B, RT, tr) for tr in (0, 1)] == ws
        finally:
            lib.dq_plan_destroy(plan)


def test_module_surface_and_state_dict():
    torch.manual_seed(3)
    a = _unet(64, True)
    torch.manual_seed(3)
    b = _unet(64, False)
    assert isinstance(a.final_act, nn.Softplus) and isinstance(b.final_act, nn.Identity)
    assert a.final_act.beta == 1 and a.final_act.threshold == 20
    from dquartic import _native as N

    assert N.lib().dq_plan_final_act(a._plan) == 1 and N.lib().dq_plan_final_act(b._plan) == 0
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
    b.load_state_dict(sa)  # a checkpoint of either kind loads into the other
    a.load_state_dict(sb)
    with pytest.raises(NotImplementedError, match="learned_variance") as ei:
        _unet(64, True, learned_variance=True)
    assert "pos_output_only" not in str(ei.value)
    with pytest.raises(NotImplementedError, match="dropout"):
        _unet(64, True, dropout=0.1)


# ---------------------------------------------------------------------------------------------------------------- GPU


def _bridge_run(net, x, t, ic, ac, gy):
    xg = x.cuda().requires_grad_()
    y = net(xg, t.cuda(), ic.cuda(), ac.cuda())
    (y * gy.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), xg.grad.cpu(), {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.requires_grad}


@pytest.mark.gpu
@pytest.mark.parametrize("B,RT,MZ", [(2, 34, 64), (1, 64, 256)])
def test_autograd_plain_head_vs_float64_oracle(B, RT, MZ):
    """The autograd bridge (dq_unet_fwd with save_for_bwd -> the plain head, k_conv_fwd<1,1,0> with the Softplus epilogue; dq_unet_bwd ->
    k_softplus_head_bwd in front of final_conv's backward): output >= 0, output, d/dx and all 395 gradients vs the float64 oracle.  Three
    settings of final_conv's bias: as perturbed; shifted by ~+20, so that the pre-activations straddle the threshold (both branches, forward and
    backward); -30, so that softplus' is ~1e-13 and the relative tolerance still has to hold."""
    from oracle import dq_oracle as O

    g = torch.Generator().manual_seed(B * 100 + RT)
    x, ic, ac = torch.randn(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    gy = torch.randn(B, RT, MZ, generator=g)
    med = None
    for case in ("as is", "threshold", "far below"):
        # (the threshold case centres the pre-activations on 20: about half of them on either side)
        shift = {"as is": 0.0, "threshold": 20.0 - (med or 0.0), "far below": -30.0}[case]
        net, params = _net(MZ, 21, bias_shift=shift)
        net = net.cuda()
        y, dx, grads = _bridge_run(net, x, t, ic, ac, gy)
        p64 = {k: v.double().clone().requires_grad_(not k.endswith("freqs")) for k, v in params.items()}
        x64 = x.double().requires_grad_()
        pre64 = O.unet_forward(p64, O.UNetConfig(downsample_dim=MZ), x64, t, ic.double(), ac.double())
        y64 = F.softplus(pre64)
        (y64 * gy.double()).sum().backward()
        if case == "as is":
            med = float(pre64.detach().median())
        if case == "threshold":
            assert 0.2 < float((pre64 > 20).double().mean()) < 0.8
        assert bool((y >= 0).all())
        assert rel_err(y, y64) < EPS_TOL, (case, rel_err(y, y64))
        assert rel_err(dx, x64.grad) < GRAD_TOL * 5, (case, rel_err(dx, x64.grad))
        _check_grads(grads, p64)


def _train_inputs(B, RT, MZ, seed):
    g = torch.Generator().manual_seed(seed)
    x0, c2, c1 = torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[0] = 0
    nz = torch.randn(B, RT, MZ, generator=g)
    return x0, c2, c1, t, nz


def _oracle_train(params, MZ, pred_type, w, x0, c2, c1, t, nz):
    """the oracle's batched train_loss: every term is per sample (per-sample time embedding, MS1 maxima per sample) and the loss is the mean
    over samples -- the per-sample loop of the B = 1 oracle in one call"""
    from oracle import dq_oracle as O

    po = {k: v.clone().requires_grad_(not k.endswith("freqs")) for k, v in params.items()}
    od = _softplus_diffusion(params=po, cfg=O.UNetConfig(downsample_dim=MZ), pred_type=pred_type)
    lo, _ = od.train_loss(x0, c2, c1, t, nz, ms1_loss_weight=w)
    lo.backward()
    return float(lo.detach()), po


def _twin_eps(net, B, RT):
    """the gradient twin of the arena's `eps` slot after a train step: d loss / d final_conv's output if k_softplus_head_bwd ran, else the
    zeros unet_backward cleared it to"""
    from dquartic import _native as N

    ws = net.workspace(B, RT, True).view(torch.float32)
    floats = ws.numel() // 2
    off = N.lib().dq_debug_tensor_offset(net._plan, b"eps")
    assert off >= 0
    return ws[floats + off: floats + off + B * RT * net.downsample_dim]


@pytest.mark.gpu
@pytest.mark.parametrize("pred_type,w", [("eps", 0.0), ("x0", 0.0), ("eps", 0.3)])
def test_train_step_vs_oracle(pred_type, w):
    """dq_train_step at (4, 400, 64): loss and all 395 gradients vs the per-sample Softplus oracle.
    ("eps", 0): the fused training head of k_level_fwd (final_conv, softplus, the squared error and d pre in the final block's launch) --
    asserted through the workspace: k_softplus_head_bwd did not run, the `eps` slot's gradient twin is still zero.
    ("x0", 0) and ("eps", 0.3): the plain head and the weighted MSE / the MS1 term on y, then softplus' once, after every loss term has
    accumulated (k_softplus_head_bwd: the twin holds d loss / d pre, non-zero)."""
    from dquartic.model.model import DDIMDiffusionModel

    B, RT, MZ = 4, 400, 64
    net, params = _net(MZ, 31)
    dm = DDIMDiffusionModel(model_class=net.cuda(), pred_type=pred_type, ms1_loss_weight=w, device="cuda")
    x0, c2, c1, t, nz = _train_inputs(B, RT, MZ, 7)
    loss = dm.train_step_fused(x0.cuda(), c2.cuda(), c1.cuda(), t=t.cuda(), noise=nz.cuda(), ms1_loss_weight=w)
    torch.cuda.synchronize()
    fused_head = not bool(_twin_eps(net, B, RT).any())
    assert fused_head == (pred_type == "eps" and w == 0.0)
    lo, po = _oracle_train(params, MZ, pred_type, w, x0, c2, c1, t, nz)
    assert abs(float(loss) - lo) < 2e-5 * abs(lo), (float(loss), lo)
    _check_grads({k: p.grad for k, p in net.named_parameters() if p.requires_grad}, po)


@pytest.mark.gpu
@pytest.mark.parametrize("pred_type", ["eps", "x0"])
def test_sampling_vs_oracle_graph_and_cache(pred_type):
    """sample() at B = 4, (400, 64), 10 steps: windows 0 and 3 vs the oracle (per-step eps), the hipGraph replay equals the eager loop bit
    for bit, the eps trajectory is >= 0 under "eps".  Then: a graph captured under Softplus, the activation switched off and on through
    the ABI, sampled again with the graph -- equal to a fresh eager run (the cached graph was dropped, and re-captured correctly)."""
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel
    from oracle import dq_oracle as O

    B, RT, MZ, NS = 4, 400, 64, 10
    net, params = _net(MZ, 41)
    dm = DDIMDiffusionModel(model_class=net.cuda(), pred_type=pred_type, device="cuda")
    g = torch.Generator().manual_seed(8)
    xT, c2, c1 = torch.randn(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    xT_, c2_, c1_ = xT.cuda(), c2.cuda(), c1.cuda()
    net.eval()
    with torch.no_grad():
        dm.use_graph = False
        s_e, n_e, tx, te = dm.sample(xT_, c2_, c1_, num_steps=NS, return_trajectory=True)
        s_e2, n_e2 = dm.sample(xT_, c2_, c1_, num_steps=NS)
        dm.use_graph = True
        s_g, n_g = dm.sample(xT_, c2_, c1_, num_steps=NS)
        assert torch.equal(s_g, s_e2) and torch.equal(n_g, n_e2)
        if pred_type == "eps":
            assert bool((te >= 0).all())
        od = _softplus_diffusion(params=params, cfg=O.UNetConfig(downsample_dim=MZ), pred_type=pred_type)
        for b in (0, 3):
            tr = []
            so, _ = od.sample(xT[b:b + 1], c2[b:b + 1], c1[b:b + 1], NS, trace=tr)
            for i, (_, _, eo) in enumerate(tr):
                assert rel_err(te[i, b:b + 1], eo) < EPS_TOL, (b, i, rel_err(te[i, b:b + 1], eo))
            assert rel_err(s_e[b:b + 1], so) < 1e-3
        lib = N.lib()
        N.check(lib.dq_plan_set_final_act(net._plan, 0), "dq_plan_set_final_act")
        N.check(lib.dq_plan_set_final_act(net._plan, 1), "dq_plan_set_final_act")
        s_g2, n_g2 = dm.sample(xT_, c2_, c1_, num_steps=NS)
        assert torch.equal(s_g2, s_e2) and torch.equal(n_g2, n_e2)
        # the identity graph must not survive a switch either: the activation changes what a replay computes
        N.check(lib.dq_plan_set_final_act(net._plan, 0), "dq_plan_set_final_act")
        s_id, _ = dm.sample(xT_, c2_, c1_, num_steps=NS)
        N.check(lib.dq_plan_set_final_act(net._plan, 1), "dq_plan_set_final_act")
        assert not torch.equal(s_id, s_e2)


@pytest.mark.gpu
def test_identity_after_softplus_is_bitwise_default():
    """A plan set to Softplus and back to identity computes what a fresh default plan computes, bit for bit: dq_unet_fwd output and
    dq_train_step loss / gradients at (4, 400, 64)."""
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel

    B, RT, MZ = 4, 400, 64
    x0, c2, c1, t, nz = (v.cuda() for v in _train_inputs(B, RT, MZ, 9))
    outs = []
    for toggle in (False, True):
        torch.manual_seed(51)
        net = _unet(MZ, False).cuda()
        if toggle:
            N.check(N.lib().dq_plan_set_final_act(net._plan, 1), "dq_plan_set_final_act")
            N.check(N.lib().dq_plan_set_final_act(net._plan, 0), "dq_plan_set_final_act")
        dm = DDIMDiffusionModel(model_class=net, device="cuda")
        with torch.no_grad():
            y = net(x0, t, c2, c1[..., None]).clone()
        loss = dm.train_step_fused(x0, c2, c1, t=t, noise=nz).clone()
        torch.cuda.synchronize()
        outs.append((y, loss, net.flat_grads().clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_cli_train_with_pos_output_only(tmp_path, monkeypatch):
    """``dquartic train`` on synthetic windows at (34, 64), 2 epochs: "pos_output_only": true builds and trains the Softplus model (a config
    without the key, the identity one); the latest checkpoint reloads into UNet1d(pos_output_only=True) and gives the trained model's
    output, which is >= 0."""
    from click.testing import CliRunner

    from dquartic.cli import cli
    from dquartic.model.model import DDIMDiffusionModel

    trained = []
    orig = DDIMDiffusionModel.train

    def record(self, *a, **k):
        trained.append(self.model)
        return orig(self, *a, **k)

    monkeypatch.setattr(DDIMDiffusionModel, "train", record)
    for pos in (True, None):
        d = tmp_path / ("pos" if pos else "default")
        d.mkdir()
        cfg_path = str(d / "c.json")
        r = CliRunner().invoke(cli, ["generate-config", cfg_path])
        assert r.exit_code == 0, r.output
        cfg = json.load(open(cfg_path))
        assert "pos_output_only" not in cfg["model"]["UNet1d"]  # (generate-config writes the reference's defaults)
        cfg["model"]["UNet1d"]["downsample_dim"] = 64
        if pos:
            cfg["model"]["UNet1d"]["pos_output_only"] = True
        cfg["model"].update(num_epochs=2, warmup_epochs=1, checkpoint_path=str(d / "best.ckpt"))
        cfg["data"]["synthetic"] = {"n_windows": 6, "RT": 34, "MZ": 64}
        cfg["wandb"]["use_wandb"] = False
        cfg["threads"] = 0
        json.dump(cfg, open(cfg_path, "w"))
        r = CliRunner().invoke(cli, ["train", cfg_path])
        assert r.exit_code == 0, (r.output, r.exception)
        assert "Epoch=2" in r.output
        assert isinstance(trained[-1].final_act, nn.Softplus if pos else nn.Identity)
    net_t = trained[0]
    ck = torch.load(str(tmp_path / "pos" / "dquartic_latest_checkpoint.ckpt"), map_location="cpu", weights_only=False)
    net_l = _unet(64, True)
    net_l.load_state_dict(ck["model_state_dict"])
    net_l = net_l.cuda()
    g = torch.Generator().manual_seed(4)
    x, ic, ac = torch.randn(2, 34, 64, generator=g).cuda(), torch.rand(2, 34, 64, generator=g).cuda(), torch.rand(2, 34, generator=g).cuda()
    t = torch.tensor([3, 700]).cuda()
    net_t.eval()
    net_l.eval()
    with torch.no_grad():
        y_t, y_l = net_t(x, t, ic, ac), net_l(x, t, ic, ac)
    assert bool((y_l >= 0).all())
    assert torch.equal(y_t, y_l)
