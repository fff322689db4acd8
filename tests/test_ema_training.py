"""The exponential moving average of the weights through the Python layers: FlatAdamW (ema_decay, ema_state_dict), TrainStepGraph,
ModelInterface (enable_ema, ema_scope, predict, checkpoints), the CLI's config keys.  The kernel itself: tests/test_ema_kernel.py.

The float64 replay of the recurrence E_t = E_{t-1} + w_t (p_t - E_{t-1}) runs over the recorded fp32 parameters p_t; its bound is the
kernel test's per-step bound carried along: B_t = (1 - w_t) B_{t-1} + 2 * 2^-24 * (w_t |p_t - E_{t-1}| + |E_t|), B_0 = 0 (an error
already in e is scaled by 1 - w_t by the next step)."""
import json

import numpy as np
import pytest
import torch

U = 2.0 ** -24
TINY = dict(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)
B, RT, MZ = 2, 8, 8
TFM = dict(input_dim=24, hidden_dim=16, num_heads=2, num_layers=1)


def tiny_dm(device, seed=3, lr=1e-3):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    dm = DDIMDiffusionModel(model_class=UNet1d(**TINY).to(device), device=device)
    dm._set_optimizer(lr)
    return dm


def tfm_dm(device, seed=3, lr=1e-3):
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    torch.manual_seed(seed)
    dm = DDIMDiffusionModel(model_class=DDIMTransformerAdapter(CustomTransformer(**TFM)).to(device), device=device)
    dm._set_optimizer(lr)
    return dm


def batches(n, mz=MZ, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [dict(x0=torch.rand(B, RT, mz, generator=g).cuda(), c2=torch.rand(B, RT, mz, generator=g).cuda(), c1=torch.rand(B, RT, generator=g).cuda(),
                 t=torch.randint(0, 1000, (B,), generator=g).cuda(), noise=torch.rand(B, RT, mz, generator=g).cuda()) for _ in range(n)]


def step(dm, b):
    return dm._train_one_batch(b["x0"], ms2_cond=b["c2"], ms1_cond=b["c1"], noise=b["noise"], t=b["t"], sync=False)


def ema_weight(beta, warmup, t):
    b = float(np.float32(beta))
    return float(np.float32(1.0 - (min(b, (1 + t) / (10 + t)) if warmup else b)))


# ---- no GPU ---------------------------------------------------------------------------------------------------------------------------

def test_flat_adamw_ema_arguments():
    from dquartic.model.model_interface import FlatAdamW
    from dquartic.model.unet1d import UNet1d

    net = UNet1d(**TINY)
    for bad in (1.0, -0.1, float("nan"), 1.5, 1.0 - 1e-9):  # (the last one is 1 as a float32, which is what the kernel is given)
        with pytest.raises(ValueError, match="ema_decay"):
            FlatAdamW(net, ema_decay=bad)
    for bad in ("0.9", True):
        with pytest.raises(TypeError, match="ema_decay"):
            FlatAdamW(net, ema_decay=bad)
    off = FlatAdamW(net)
    assert off.ema_decay is None and off._ema is None and not off.ema_enabled
    with pytest.raises(RuntimeError, match="not enabled"):
        off.ema_state_dict()
    opt = FlatAdamW(net, ema_decay=0.999, ema_warmup=False)
    assert opt.ema_enabled and (opt.ema_decay, opt.ema_warmup) == (0.999, False)
    assert torch.equal(opt._ema, net.flat_params) and opt._ema.data_ptr() != net.flat_params.data_ptr()  # a copy at that moment
    kept = opt._ema
    opt.enable_ema(0.0)  # the allowed edge; an existing average is kept
    assert opt._ema is kept and opt.ema_warmup is True
    opt.disable_ema()
    assert not opt.ema_enabled and opt._ema is None


@pytest.mark.parametrize("make", [tiny_dm, tfm_dm])
def test_ema_state_dict_has_the_models_keys_and_shapes(make):
    dm = make("cpu")
    dm.enable_ema(0.9)
    with torch.no_grad():
        dm.optimizer._ema.mul_(2.0)
    sd, esd = dm.model.state_dict(), dm.optimizer.ema_state_dict()
    assert [(k, tuple(v.shape)) for k, v in esd.items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    trained = {n for n, _ in dm.model.trainable_named()}
    for k in sd:
        assert torch.equal(esd[k], sd[k] * 2.0 if k in trained else sd[k]), k
    # a view: the optimiser's buffer is what it shows; and the counterpart writes it
    assert all(esd[n].data_ptr() == dm.optimizer._ema.data_ptr() + 4 * o for n, o, _ in dm.model._layout)
    dm.optimizer.load_ema_state_dict({k: v * 0.5 for k, v in esd.items()})
    assert torch.equal(dm.optimizer._ema, dm.model.flat_params)
    with pytest.raises(KeyError):
        dm.optimizer.load_ema_state_dict({})


def test_optimizer_state_dict_is_unchanged_by_ema():
    dm = tiny_dm("cpu")
    dm.optimizer._buffers()
    before = dm.optimizer.state_dict()
    dm.enable_ema(0.9)
    after = dm.optimizer.state_dict()
    assert before["param_groups"] == after["param_groups"] and list(before["state"]) == list(after["state"])
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in after["state"].values())


def test_enable_ema_needs_the_flat_optimizer():
    from dquartic.model.model import DDIMDiffusionModel

    dm = DDIMDiffusionModel(model_class=torch.nn.Linear(2, 2), device="cpu")
    with pytest.raises(RuntimeError, match="FlatAdamW"):
        dm.enable_ema()
    dm._set_optimizer(1e-3)
    with pytest.raises(RuntimeError, match="FlatAdamW"):
        dm.enable_ema()
    with pytest.raises(RuntimeError, match="not enabled"):
        with tiny_dm("cpu").ema_scope():
            pass


def test_cli_reads_ema_from_the_config_and_generate_config_is_unchanged(tmp_path):
    from dquartic.cli import enable_ema_from_config
    from dquartic.utils.config_loader import generate_train_config, load_train_config

    p = str(tmp_path / "c.json")
    generate_train_config(p)
    assert "ema" not in open(p).read()
    m = load_train_config(p)["model"]
    dm = tiny_dm("cpu")
    dm.optimizer = None
    assert enable_ema_from_config(dm, m) is False and dm.optimizer is None  # absent: off, nothing is created
    assert enable_ema_from_config(dm, {**m, "ema_decay": None}) is False and dm.optimizer is None
    raw = json.load(open(p))
    raw["model"].update(ema_decay=0.99, ema_warmup=False)
    json.dump(raw, open(p, "w"))
    m = load_train_config(p)["model"]
    assert enable_ema_from_config(dm, m) is True
    assert dm.ema_enabled and (dm.optimizer.ema_decay, dm.optimizer.ema_warmup) == (0.99, False)
    assert dm.optimizer.param_groups[0]["lr"] == m["learning_rate"]
    dm2 = tiny_dm("cpu")
    assert enable_ema_from_config(dm2, {"learning_rate": 1e-4, "ema_decay": 0.5}) and dm2.optimizer.ema_warmup is True


def test_checkpoint_round_trip(tmp_path):
    """with EMA: the average comes back; an EMA-less file into an EMA-enabled model: the average is the loaded weights; EMA off: today's keys"""
    a = tiny_dm("cpu", seed=1)
    a.enable_ema(0.99, warmup=False)
    a.optimizer._buffers()
    with torch.no_grad():
        a.optimizer._ema.uniform_(-1, 1)
    sch = a._get_lr_schedule_with_warmup(2, 10)
    with_ema, without = str(tmp_path / "ema.ckpt"), str(tmp_path / "plain.ckpt")
    a.save_checkpoint(sch, 3, 0.25, with_ema)
    ck = torch.load(with_ema, weights_only=False)
    today = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "best_loss"}
    assert set(ck) == today | {"ema_state_dict", "ema_decay", "ema_warmup"} and (ck["ema_decay"], ck["ema_warmup"]) == (0.99, False)
    assert list(ck["ema_state_dict"]) == list(ck["model_state_dict"])
    b = tiny_dm("cpu", seed=2)
    b.enable_ema(0.99)
    b.load_checkpoint(b._get_lr_schedule_with_warmup(2, 10), with_ema, "cpu")
    assert torch.equal(b.optimizer._ema, a.optimizer._ema) and torch.equal(b.model.flat_params, a.model.flat_params)
    assert not torch.equal(b.optimizer._ema, b.model.flat_params)
    a.disable_ema()
    a.save_checkpoint(sch, 3, 0.25, without)
    assert set(torch.load(without, weights_only=False)) == today
    c = tiny_dm("cpu", seed=4)
    c.enable_ema(0.99)
    c.load_checkpoint(c._get_lr_schedule_with_warmup(2, 10), without, "cpu")
    assert torch.equal(c.model.flat_params, a.model.flat_params) and torch.equal(c.optimizer._ema, a.model.flat_params)
    d = tiny_dm("cpu", seed=4)  # EMA off: a file that has an average loads as before
    d.load_checkpoint(d._get_lr_schedule_with_warmup(2, 10), with_ema, "cpu")
    assert not d.ema_enabled and torch.equal(d.model.flat_params, a.model.flat_params)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_training_is_unaffected_and_the_average_follows_the_recurrence():
    beta, warmup = 0.9, True
    on, off = tiny_dm("cuda"), tiny_dm("cuda")
    on.enable_ema(beta, warmup)
    assert torch.equal(on.model.flat_params, off.model.flat_params)
    traj = [on.model.flat_params.detach().cpu().clone()]
    assert torch.equal(on.optimizer.ema_buffer().cpu(), traj[0])
    for b in batches(5):
        la, lb = step(on, b), step(off, b)
        assert torch.equal(la, lb)
        assert torch.equal(on.model.flat_params, off.model.flat_params)
        assert torch.equal(on.optimizer._m, off.optimizer._m) and torch.equal(on.optimizer._v, off.optimizer._v)
        traj.append(on.model.flat_params.detach().cpu().clone())
    E, bound = traj[0].double(), torch.zeros_like(traj[0], dtype=torch.float64)
    for t in range(1, 6):
        w, P = ema_weight(beta, warmup, t), traj[t].double()
        E_new = E + w * (P - E)
        bound = (1 - w) * bound + 2 * U * (w * (P - E).abs() + E_new.abs())
        E = E_new
    e = on.optimizer.ema_buffer().cpu().double()
    err = (e - E).abs()
    print(f"ema after 5 steps: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, bound max {float(bound.max()):.3g}, "
          + " ".join(f"|e - p_{k}| {float((e - traj[k].double()).abs().max()):.3g}" for k in (1, 2, 5)))
    assert bool((err <= bound).all())
    for k in (1, 2, 5):  # not the raw weights of any step: e = p cannot pass
        assert float((e - traj[k].double()).abs().max()) > 100 * float(bound.max()), k


@pytest.mark.gpu
def test_captured_step_keeps_the_same_average():
    """four steps, eager (device-state optimiser step) and as one captured graph per step, from the same generator state: p, m, v, e bit for bit"""
    data = batches(4)

    def make():
        dm = tiny_dm("cuda")
        dm.enable_ema(0.9)
        return dm

    eager = make()
    torch.manual_seed(11)
    for b in data:
        eager.train_step_fused(b["x0"], b["c2"], b["c1"], zero_grads=True)
        eager.optimizer.step_dev()
    graph = make()
    graph.enable_train_graph()
    torch.manual_seed(11)
    for b in data:
        graph._train_one_batch(b["x0"], ms2_cond=b["c2"], ms1_cond=b["c1"], sync=False)
    torch.cuda.synchronize()
    assert graph.optimizer._step == eager.optimizer._step == 4 and int(graph.optimizer._step_dev.item()) == 4
    assert torch.equal(graph.model.flat_params, eager.model.flat_params)
    assert torch.equal(graph.optimizer._m, eager.optimizer._m) and torch.equal(graph.optimizer._v, eager.optimizer._v)
    assert torch.equal(graph.optimizer.ema_buffer(), eager.optimizer.ema_buffer())
    assert not torch.equal(graph.optimizer.ema_buffer(), graph.model.flat_params)
    # a graph captured with EMA on does not serve a step with EMA off, and the reverse
    (tg,) = graph._train_graphs.values()
    b = data[0]
    assert tg.matches(b["x0"], b["c1"], 0.0, 1.0)
    kept = graph.optimizer._ema
    graph.optimizer.ema_decay, graph.optimizer._ema = None, None
    assert not tg.matches(b["x0"], b["c1"], 0.0, 1.0)
    graph.optimizer.ema_decay, graph.optimizer._ema = 0.9, kept
    assert tg.matches(b["x0"], b["c1"], 0.0, 1.0)
    graph.optimizer.enable_ema(0.99)
    assert not tg.matches(b["x0"], b["c1"], 0.0, 1.0)
    graph.enable_train_graph(False)
    plain = tiny_dm("cuda")
    plain.enable_train_graph()
    torch.manual_seed(11)
    plain._train_one_batch(b["x0"], ms2_cond=b["c2"], ms1_cond=b["c1"], sync=False)
    (tp,) = plain._train_graphs.values()
    plain.enable_ema(0.9)
    assert not tp.matches(b["x0"], b["c1"], 0.0, 1.0)
    plain.enable_train_graph(False)


@pytest.mark.gpu
def test_ema_scope_reads_the_average_by_pointer():
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    dm = tiny_dm("cuda")
    dm.enable_ema(0.9)
    for b in batches(2):
        step(dm, b)
    net, opt = dm.model, dm.optimizer
    ref = UNet1d(**TINY)
    ref.load_state_dict({k: v.cpu() for k, v in opt.ema_state_dict().items()})
    dm_ref = DDIMDiffusionModel(model_class=ref.cuda(), device="cuda")
    before, ptr = net.flat_params.detach().clone(), net.flat_params.data_ptr()
    assert not torch.equal(opt.ema_buffer(), before)
    g = torch.Generator().manual_seed(9)
    x_T, c2, c1 = torch.randn(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, generator=g).cuda()
    tt = torch.tensor([3, 700]).cuda()
    assert net.read_params().data_ptr() == ptr
    with dm.ema_scope():
        assert net.read_params().data_ptr() == opt.ema_buffer().data_ptr() != ptr
        assert net.flat_params.data_ptr() == ptr  # the training weights stay where and what they are
        with torch.no_grad():
            assert torch.equal(net(x_T, tt, c2, c1), ref(x_T, tt, c2, c1))
        for use_graph in (False, True):
            dm.use_graph = dm_ref.use_graph = use_graph
            got, want = dm.sample(x_T, c2, c1, num_steps=3), dm_ref.sample(x_T, c2, c1, num_steps=3)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), use_graph
        with pytest.raises(RuntimeError, match="ema_scope"):
            net(x_T.clone().requires_grad_(), tt, c2, c1)
        with pytest.raises(RuntimeError, match="ema_scope"):
            net(x_T, tt, c2, c1)  # grad mode on, trainable parameters: it would record history
        with pytest.raises(RuntimeError, match="ema_scope"):
            step(dm, batches(1)[0])
    assert net._param_override is None and net.read_params().data_ptr() == ptr
    assert net.flat_params.data_ptr() == ptr and torch.equal(net.flat_params, before)
    with pytest.raises(ZeroDivisionError):
        with dm.ema_scope():
            1 / 0
    assert net._param_override is None
    # outside the scope sample() reads the training weights; _predict_one_batch defaults to the average
    out = dm.sample(x_T, c2, c1, num_steps=3)
    assert not torch.equal(out[0], want[0])
    torch.manual_seed(2)
    a, _ = dm._predict_one_batch(x_T, ms2_cond=c2, ms1_cond=c1, num_steps=3)
    torch.manual_seed(2)
    r, _ = dm_ref._predict_one_batch(x_T, ms2_cond=c2, ms1_cond=c1, num_steps=3)
    torch.manual_seed(2)
    raw, _ = dm._predict_one_batch(x_T, ms2_cond=c2, ms1_cond=c1, num_steps=3, use_ema=False)
    assert np.array_equal(a, r) and not np.array_equal(raw, r)


@pytest.mark.gpu
def test_transformer_average_behind_the_adapter():
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter

    D = TFM["input_dim"]
    dm = tfm_dm("cuda")
    dm.enable_ema(0.9)
    p0 = dm.model.flat_params.detach().clone()
    for b in batches(2, mz=D):
        step(dm, b)
    e = dm.optimizer.ema_buffer()
    assert not torch.equal(e, p0) and not torch.equal(e, dm.model.flat_params)
    ref = DDIMTransformerAdapter(CustomTransformer(**TFM))
    ref.load_state_dict({k: v.cpu() for k, v in dm.optimizer.ema_state_dict().items()})
    ref = ref.cuda()
    g = torch.Generator().manual_seed(9)
    x, c1, tt = torch.randn(B, RT, D, generator=g).cuda(), torch.rand(B, RT, generator=g).cuda(), torch.tensor([3, 700]).cuda()
    before = dm.model.flat_params.detach().clone()
    with torch.no_grad():
        raw = dm.model(x, tt, None, c1)
        with dm.ema_scope():
            got = dm.model(x, tt, None, c1)
        want = ref(x, tt, None, c1)
    assert torch.equal(got, want) and not torch.equal(raw, want)
    with dm.ema_scope(), pytest.raises(RuntimeError, match="ema_scope"):
        dm.model(x, tt, None, c1)
    assert torch.equal(dm.model.flat_params, before)
