"""Training, evaluation and sampling under the v objective (pred_type="v_prediction") through DDIMDiffusionModel,
against float64: ``O.unet_forward`` in float64 with the v arithmetic written out here (v = sa eps - sb x0; x0 = sa x_t - sb v, eps = sb x_t +
sa v; the oracle's Diffusion refuses the objective).

Tiny network: dim_mults=(1, 2), downsample_dim=8, B = 3, RT = 9, t = [0, 500, 999].  k_level_fwd's grid is (workgroups per window, B): a
workgroup never spans two windows, so what can go wrong per window is the lookup of its own sa_b, sb_b and weight -- three different t -- and
the tile edge inside a window: RT * MZ = 72 is one full 64-position tile and a partly filled one per window, the second taken by another wave.
Tolerances: those of tests/test_hip_x0.py::test_default_net_vs_oracle (loss 5e-5 relative, gradients 1e-3 * max(|ref|, 1e-4 * gmax), sample
5e-4), tests/test_hip_sample.py's per-step ones (eps 1e-4, x and the sample 1e-3 relative), times 1 + 2 w guided as tests/test_guided_sample.py
states."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

pytestmark = pytest.mark.gpu

PRED = "v_prediction"
DEV_LIB = os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd", "build", "dev", "libdq_hip_dev.so")
B, RT, MZ = 3, 9, 8
T3 = (0, 500, 999)
KW = dict(dim=4, channels=1, conditional=True, init_cond_channels=1, attn_cond_channels=1, simple=True)
TINY = dict(KW, dim_mults=(1, 2), downsample_dim=MZ)


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def make_dm(seed=5, softplus=False, pred=PRED, **net_kw):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    net = UNet1d(**{**TINY, **net_kw}, pos_output_only=softplus)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    po = {k: v.detach().clone().cpu() for k, v in net.state_dict().items()}
    return DDIMDiffusionModel(model_class=net.cuda(), pred_type=pred, device="cuda"), po


def batch(rt=RT, mz=MZ, seed=1, t=T3):
    g = torch.Generator().manual_seed(seed)
    x0, c2, c1 = torch.rand(B, rt, mz, generator=g), torch.rand(B, rt, mz, generator=g), torch.rand(B, rt, generator=g)
    return x0, c2, c1, torch.tensor(t), torch.randn(B, rt, mz, generator=g)


class F64:
    """the float64 side: the network through O.unet_forward on float64 copies of the weights, the objective written out"""

    def __init__(self, po, dm, softplus=False, **cfg):
        from oracle import dq_oracle as O

        self.O, self.softplus = O, softplus
        self.p = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in po.items()}
        self.keys = O.trainable_keys(po)
        self.cfg = O.UNetConfig(**cfg)
        self.ab = dm.alpha_bars.detach().cpu().double()  # the fp32 table both sides read

    def net(self, x, t, c2n, c1n):
        out = self.O.unet_forward(self.p, self.cfg, x, t, c2n, c1n)
        return F.softplus(out) if self.softplus else out

    def per_window(self, x0, c2, c1, t, nz):
        x0n, c2n, c1n, nz = (2 * x0.double() - 1), (2 * c2.double() - 1), (2 * c1.double() - 1), nz.double()
        sa, sb = self.ab[t].sqrt()[:, None, None], (1 - self.ab[t]).sqrt()[:, None, None]
        out = self.net(sa * x0n + sb * nz, t, c2n, c1n)
        return ((out - (sa * nz - sb * x0n)) ** 2).flatten(1).mean(dim=1)

    def loss_and_grads(self, x0, c2, c1, t, nz):
        for k in self.keys:
            self.p[k].requires_grad_(True)
            self.p[k].grad = None
        loss = self.per_window(x0, c2, c1, t, nz).mean()  # loss_weight is all ones
        loss.backward()
        grads = {k: self.p[k].grad.clone() for k in self.keys}
        for k in self.keys:
            self.p[k].requires_grad_(False)
        return float(loss), grads

    def v_to_x0_eps(self, x, v, sa, sb):
        return sa * x - sb * v, sb * x + sa * v

    @torch.no_grad()
    def sample(self, x_T, c2, c1, coef, extra, kind, ts, clip=None, z=None, guidance=None):
        """the loop over the sampler's own fp32 table rows (float64 arithmetic); returns (sample, traj_x, traj_eps)"""
        c2n, c1n = 2 * c2.double() - 1, 2 * c1.double() - 1
        x, hist, tx, te = x_T.double(), None, [], []
        for i, t in enumerate(ts):
            tt = torch.full((x.shape[0],), int(t), dtype=torch.long)
            v = self.net(x, tt, c2n, c1n)
            if guidance is not None:  # g = u + w (c - u) on the network output; the null MS1 is the raw value in every element
                w, null = guidance
                u = self.net(x, tt, c2n, torch.full_like(c1n, 2 * null - 1))
                v = u + w * (v - u)
            sa, sb, r2, r3 = (float(a) for a in coef[i])
            x0, ep = self.v_to_x0_eps(x, v, sa, sb)
            if kind == "solver":
                if clip is not None:
                    x0c = x0.clamp(-clip, clip)
                    ep = torch.where(x0c != x0, (x - sa * x0c) / sb, ep)
                    x0 = x0c
                c1_ = float(extra[i])
                x = x0 if r2 < 0 else r2 * x + r3 * x0 + (c1_ * hist if c1_ != 0 else 0.0)
                hist = x0
            else:
                x = x0 if r2 < 0 else r2 * x0 + r3 * ep + (float(extra[i]) * z[i] if z is not None else 0.0)
            tx.append(x.clone()); te.append(ep.clone())
        return (x + 1) / 2, torch.stack(tx), torch.stack(te)


def check_grads(net, grads, tag):
    gmax = max(float(g.abs().max()) for g in grads.values())
    named = dict(net.named_parameters())
    worst = 0.0
    for k, ref in grads.items():
        err = float((named[k].grad.cpu().double() - ref).abs().max())
        tol = 1e-3 * max(float(ref.abs().max()), 1e-4 * gmax)
        worst = max(worst, err / tol)
        assert err <= tol, (tag, k, err, tol)
    return worst


@pytest.mark.parametrize("softplus", [False, True])
def test_tiny_train_step_vs_float64(softplus):
    dm, po = make_dm(softplus=softplus)
    net = dm.model
    net.train()
    ref = F64(po, dm, softplus, dim_mults=(1, 2), downsample_dim=MZ)
    x0, c2, c1, t, nz = batch()
    lo, grads = ref.loss_and_grads(x0, c2, c1, t, nz)
    dev = [v.cuda() for v in (x0, c2, c1)]
    loss = dm.train_step_fused(*dev, t=t.cuda(), noise=nz.cuda())
    fused = net.flat_grads().clone()
    wf = check_grads(net, grads, "fused")
    assert abs(float(loss) - lo) < 5e-5 * abs(lo), (float(loss), lo)
    # two identical steps: the same bits
    loss2 = dm.train_step_fused(*dev, t=t.cuda(), noise=nz.cuda())
    assert torch.equal(loss2, loss) and torch.equal(net.flat_grads(), fused)
    # the autograd path (train_step maps a passed noise 2 n - 1 like the reference: feed (n + 1) / 2)
    net.flat_grads(zero=True)
    la = dm.train_step(*dev, noise=(nz.cuda() + 1) / 2, t=t.cuda())
    la.backward()
    wa = check_grads(net, grads, "autograd")
    assert abs(float(la) - lo) < 5e-5 * abs(lo) and abs(float(la) - float(loss)) < 5e-5 * abs(lo)
    print(f"v train step (softplus {softplus}): loss {float(loss):.8g} autograd {float(la):.8g} float64 {lo:.8g}; worst grad err / tol fused {wf:.3f} "
          f"autograd {wa:.3f}; fused vs autograd grads rel {rel_err(net.flat_grads(), fused):.2e}")
    assert rel_err(net.flat_grads(), fused) < 1e-3
    # eval_step: per_window and loss against float64, and the train step's loss
    el, pw = dm.eval_step(*dev, t=t.cuda(), noise=nz.cuda())
    ref_pw = ref.per_window(x0, c2, c1, t, nz).detach()
    assert rel_err(pw, ref_pw) < 5e-5 and abs(float(el) - lo) < 5e-5 * abs(lo) and abs(float(el) - float(loss)) < 5e-5 * abs(float(loss))


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[3])
import test_v_train as T
dm, _ = T.make_dm(softplus=bool(int(sys.argv[4])))
dm.model.train()
x0, c2, c1, t, nz = T.batch()
loss = dm.train_step_fused(x0.cuda(), c2.cuda(), c1.cuda(), t=t.cuda(), noise=nz.cuda())
torch.cuda.synchronize()
np.savez(sys.argv[2], loss=float(loss), grads=dm.model.flat_grads().cpu().numpy())
"""


@pytest.mark.parametrize("softplus", [0, 1])
def test_fused_head_vs_the_unfused_path(tmp_path, softplus):
    """the loss and the first two backward steps in the forward's last launch against k_conv_fwd / k_mse_fwd_bwd<MseV> / k_conv_bwd_data behind it
    (the development build's DQ_NO_HEAD_LOSS=1): one child process each on build/dev/libdq_hip_dev.so, whose default paths are the product's"""
    assert os.path.exists(DEV_LIB), "build the development library first (make dev, or __graft_entry__.build())"
    res = {}
    for tag, env in (("head", {}), ("nohead", {"DQ_NO_HEAD_LOSS": "1"})):
        out = str(tmp_path / f"{tag}.npz")
        e = {**os.environ, **env, "DQ_HIP_LIB": DEV_LIB}
        r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd"), out,
                            os.path.join(REPO, "tests"), str(softplus)], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = dict(np.load(out))
    a, b = res["head"], res["nohead"]
    gmax = float(np.abs(b["grads"]).max())
    print(f"fused head vs un-fused (softplus {softplus}): loss {a['loss']:.8g} / {b['loss']:.8g}, grads max |diff| {float(np.abs(a['grads'] - b['grads']).max()):.3g} "
          f"of {gmax:.3g}, bitwise {np.array_equal(a['grads'], b['grads'])}")
    assert abs(a["loss"] - b["loss"]) < 5e-5 * abs(b["loss"])  # (summed in another fixed order)
    # the per-element arithmetic of the head is k_mse_fwd_bwd<MseV>'s and k_conv_bwd_data's: every gradient bit for bit, as
    # tests/test_tiny_levels.py finds for the eps head
    assert np.array_equal(a["grads"], b["grads"])


def test_captured_step_equals_the_eager_one():
    """two optimiser steps, eager and as the captured TrainStepGraph, from the same generator state: parameters and moments bit for bit"""
    x0, c2, c1, _, _ = batch()
    dev = [v.cuda() for v in (x0, c2, c1)]

    def make():
        dm, _ = make_dm()
        dm.model.train()
        dm._set_optimizer(1e-3)
        return dm

    eager = make()
    torch.manual_seed(11)
    for _ in range(2):
        le = eager.train_step_fused(*dev, zero_grads=True)
        eager.optimizer.step_dev()
    graph = make()
    graph.enable_train_graph()
    torch.manual_seed(11)
    for _ in range(2):
        graph._train_one_batch(dev[0], ms2_cond=dev[1], ms1_cond=dev[2], sync=False)
    torch.cuda.synchronize()
    assert graph.optimizer._step == eager.optimizer._step == 2 and bool(torch.isfinite(le))
    assert torch.equal(graph.model.flat_params, eager.model.flat_params)
    assert torch.equal(graph.optimizer._m, eager.optimizer._m) and torch.equal(graph.optimizer._v, eager.optimizer._v)


def test_default_net_vs_float64():
    """the default 7-level network at RT = 24, B = 3 (the shape of tests/test_hip_x0.py): loss, every gradient and a 3-step sample"""
    big = dict(dim_mults=(1, 2, 2, 3, 3, 4, 4), downsample_dim=64)
    dm, po = make_dm(**big)
    net = dm.model
    net.train()
    ref = F64(po, dm, **big)
    x0, c2, c1, t, nz = batch(24, 64, t=(7, 500, 950))
    lo, grads = ref.loss_and_grads(x0, c2, c1, t, nz)
    loss = dm.train_step_fused(x0.cuda(), c2.cuda(), c1.cuda(), t=t.cuda(), noise=nz.cuda())
    assert abs(float(loss) - lo) < 5e-5 * abs(lo), (float(loss), lo)
    worst = check_grads(net, grads, "default")
    ts = dm.sampler_timesteps(1000, 3).tolist()
    coef, extra = dm.ddim_coef_table(ts, 0.0)
    so, _, _ = ref.sample(nz, c2, c1, coef, extra * 0, "ddim", ts)
    s, n = dm.sample(nz.cuda(), c2.cuda(), c1.cuda(), num_steps=3)
    print(f"default net, v objective: loss {float(loss):.8g} (float64 {lo:.8g}), worst grad err / tol {worst:.3f}, sample rel err {rel_err(s, so):.2e}")
    assert rel_err(s, so) < 5e-4 and rel_err(n, c2.double() - so) < 5e-4


def _randn(dm, seed, draw, shape):
    from dquartic import _native as N

    out, seed_d = torch.empty(shape, device="cuda"), dm._seed_tensor(seed, "cuda")
    N.check(N.lib().dq_randn(N.ptr(out), None, N.ptr(seed_d), draw, shape[0], out[0].numel(), N.stream_ptr()), "dq_randn")
    return out.cpu().double()


SAMPLERS = [("dpmpp_2m", dict(sampler="dpmpp_2m", clip_x0=1.0)), ("eta1", dict(eta=1.0, seed=1234)), ("guided", dict(guidance_scale=3.0))]


@pytest.mark.parametrize("name,kw", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_tiny_sampling_vs_float64(name, kw):
    dm, po = make_dm()
    dm.model.eval()
    ref = F64(po, dm, dim_mults=(1, 2), downsample_dim=MZ)
    _, c2, c1, _, x_T = batch(seed=3)
    steps = 4
    ts = dm.sampler_timesteps(1000, steps).tolist()
    scale = 1.0
    if name == "dpmpp_2m":
        coef, extra = dm.sampler_coef_table(ts, "dpmpp_2m")
        so, tx, te = ref.sample(x_T, c2, c1, coef, extra, "solver", ts, clip=1.0)
    elif name == "eta1":
        coef, extra = dm.ddim_coef_table(ts, 1.0)
        z = [_randn(dm, 1234, 1 + i, (B, RT, MZ)) for i in range(steps)]
        so, tx, te = ref.sample(x_T, c2, c1, coef, extra, "ddim", ts, z=z)
    else:
        coef, extra = dm.ddim_coef_table(ts, 0.0)
        so, tx, te = ref.sample(x_T, c2, c1, coef, extra * 0, "ddim", ts, guidance=(3.0, 0.0))
        scale = 1.0 + 2 * 3.0
    dev = [v.cuda() for v in (x_T, c2, c1)]
    dm.use_graph = False
    s, n, gx, ge = dm.sample(*dev, num_steps=steps, return_trajectory=True, **kw)
    r = dict(eps=rel_err(ge, te), x=rel_err(gx, tx), sample=rel_err(s, so))
    print(f"v sampling [{name}], 4 steps on the tiny network: relative errors " + " ".join(f"{k} {v:.2e}" for k, v in r.items()))
    assert r["eps"] < scale * 1e-4 and r["x"] < scale * 1e-3 and r["sample"] < scale * 1e-3, r
    # the captured step: the eager loop's bits
    s0, n0 = dm.sample(*dev, num_steps=steps, **kw)
    dm.use_graph = True
    sg, ng = dm.sample(*dev, num_steps=steps, **kw)
    assert torch.equal(s0, s) and torch.equal(sg, s) and torch.equal(ng, n)
    # a window alone equals the same window in the batch
    for b in range(B):
        extra_kw = dict(kw, window_ids=[b]) if name == "eta1" else kw
        sb, _ = dm.sample(*(v[b:b + 1].contiguous() for v in dev), num_steps=steps, **extra_kw)
        assert torch.equal(sb, s[b:b + 1]), (name, b)


def test_cli_train_with_the_v_objective(tmp_path):
    """``dquartic train`` for two epochs on the synthetic data with "pred_type": "v_prediction" and a data.validation block"""
    from click.testing import CliRunner
    from dquartic.cli import cli

    cfg_path, ckpt = str(tmp_path / "c.json"), str(tmp_path / "best.ckpt")
    assert CliRunner().invoke(cli, ["generate-config", cfg_path]).exit_code == 0
    cfg = json.load(open(cfg_path))
    cfg["model"]["UNet1d"].update(downsample_dim=64)
    cfg["model"].update(num_epochs=2, warmup_epochs=1, checkpoint_path=ckpt, batch_size=4, pred_type=PRED)
    cfg["data"]["synthetic"] = {"n_windows": 8, "RT": 16, "MZ": 64}
    cfg["data"]["validation"] = {"synthetic": {"n_windows": 4, "RT": 16, "MZ": 64}}
    cfg["wandb"]["use_wandb"] = False
    cfg["threads"] = 0
    json.dump(cfg, open(cfg_path, "w"))
    r = CliRunner().invoke(cli, ["train", cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    assert "Epoch=2" in r.output and "val_loss=" in r.output and os.path.exists(ckpt)
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert np.isfinite(ck["val_loss"]) and "pred_type" not in ck  # the objective is not part of a checkpoint
