"""ModelInterface.evaluate, train(..., val_dataloader=...) and the command line's evaluate for a CustomTransformer(64, 32, heads 2, 1 layer) behind
its adapter, on the 8-window synthetic held-out set of tests/test_evaluate_gpu.py (RT 16, MZ 64): every repeat of a batch goes through one
dq_tfm_eval_step.  Reproducible bit for bit at a given batch size; across batch sizes to fp32 rounding only."""
import json

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

RT, MZ, N_WINDOWS = 16, 64, 8
OLD_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "best_loss"}  # tests/test_host_logic.py


def make_dm(seed=0, native_sampler=False, pred_type="eps"):
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel

    torch.manual_seed(seed)
    net = DDIMTransformerAdapter(CustomTransformer(input_dim=MZ, hidden_dim=32, num_heads=2, num_layers=1)).cuda()
    dm = DDIMDiffusionModel(model_class=net, pred_type=pred_type, device="cuda")
    dm.native_tfm_sampler = native_sampler
    return dm


@pytest.fixture(scope="module")
def held_out():
    from dquartic.utils.synthetic import FrozenPairDataset, SyntheticDIAMSDataset

    return FrozenPairDataset(SyntheticDIAMSDataset(n_windows=N_WINDOWS, RT=RT, MZ=MZ, start=5000), N_WINDOWS)


@pytest.fixture(scope="module")
def dm():
    return make_dm()


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("native_sampler", [False, True], ids=["generic_sampler", "native_sampler"])
def test_two_calls_return_the_same_dict(held_out, native_sampler):
    dm = make_dm(native_sampler=native_sampler)
    loader = DataLoader(held_out, batch_size=4, shuffle=False)
    a, b = dm.evaluate(loader, num_steps=3), dm.evaluate(loader, num_steps=3)
    same(a, b)
    assert a["n_windows"] == N_WINDOWS and len(a["val_loss_by_t"]["mse"]) == 4 and len(a["val_loss_by_t"]["edges"]) == 5
    assert np.isfinite(a["val_loss"]) and a["val_loss"] > 0 and np.all(np.isfinite(a["val_loss_by_t"]["mse"]))
    # eps objective: the weights are 1, so the loss is the mean of the bucket means
    assert a["val_loss"] == pytest.approx(np.mean(a["val_loss_by_t"]["mse"]), rel=1e-12)
    assert dm.evaluate(loader, seed=1)["val_loss"] != a["val_loss"]
    assert dm.evaluate(loader, max_batches=1)["n_windows"] == 4
    assert dm.evaluate(loader, n_t=1)["n_t"] == 1  # one repeat: no K | V copy, the same call


def test_the_repeats_are_the_draws_of_dq_randn(dm, held_out):
    """evaluate's numbers are eval_step's on evaluation.window_noise, repeat k at draw index k: the stacked call changes how, not what"""
    from dquartic.model import evaluation as E

    loader = DataLoader(held_out, batch_size=N_WINDOWS, shuffle=False)
    res = dm.evaluate(loader, n_t=3, seed=7)
    ms2_1, ms1_1, _, _ = next(iter(loader))
    x_0, ms1 = ms2_1.cuda(), ms1_1.cuda()
    ids = np.arange(N_WINDOWS, dtype=np.int64)
    seed_dev, ids_dev = dm._seed_tensor(7, "cuda"), torch.from_numpy(ids).cuda()
    for k in range(3):
        t = torch.from_numpy(E.stratified_timesteps(ids, k, 3, 1000)).cuda()
        _, pw = dm.eval_step(x_0, None, ms1, t=t, noise=E.window_noise(seed_dev, ids_dev, k, x_0.shape))
        got, ref = res["val_loss_by_t"]["mse"][k], float(pw.double().mean())
        # R = 1 against R = 3: another GEMM plan, so to rounding only (2^-24 per window would be bitwise; 1e-5 is the bound of the test below)
        print(f"bucket {k}: stacked {got:.9g} single {ref:.9g} rel {abs(got - ref) / ref:.2e}")
        assert got == pytest.approx(ref, rel=1e-5)


def test_the_batch_size_changes_rounding_only(dm, held_out):
    a = dm.evaluate(DataLoader(held_out, batch_size=2, shuffle=False))
    b = dm.evaluate(DataLoader(held_out, batch_size=8, shuffle=False))
    rel = abs(a["val_loss"] - b["val_loss"]) / abs(b["val_loss"])
    print(f"val_loss batch 2: {a['val_loss']:.9g}  batch 8: {b['val_loss']:.9g}  rel diff {rel:.3e}")
    # rel=1e-5: the rounding of fp32 GEMM plans that follow the row count (each output differs by a few ulp of 6e-8), not a measured
    # tolerance of the feature; the U-Net's evaluate is bitwise here (tests/test_evaluate_gpu.py) because its forward's plans are not
    assert a["val_loss"] == pytest.approx(b["val_loss"], rel=1e-5)
    assert a["val_loss_by_t"]["mse"] == pytest.approx(b["val_loss_by_t"]["mse"], rel=1e-5)


@pytest.mark.parametrize("kw", [dict(eta=1.0), dict(sampler="dpmpp_2m")], ids=["eta1", "dpmpp_2m"])
@pytest.mark.parametrize("native_sampler", [False, True], ids=["generic_sampler", "native_sampler"])
def test_num_steps_fills_all_nine_metrics(held_out, native_sampler, kw):
    from dquartic import _native as N

    dm = make_dm(native_sampler=native_sampler)
    loader = DataLoader(held_out, batch_size=4, shuffle=False)
    assert "per_window" not in dm.evaluate(loader)
    res = dm.evaluate(loader, num_steps=3, **kw)
    assert res["per_window"].shape == (N_WINDOWS, 9) and res["per_window"].dtype == np.float32
    assert np.all(np.isfinite(res["per_window"]))
    for name in N.METRIC_NAMES:
        assert np.isfinite(res[name]), name
    assert 0 < res["scan_count"] <= RT and 0 < res["xic_count"] <= MZ
    assert res["num_steps"] == 3 and np.isfinite(res["val_loss"])


def test_x0_objective_weights_the_loss(held_out):
    dm = make_dm(pred_type="x0")
    res = dm.evaluate(DataLoader(held_out, batch_size=4, shuffle=False))
    assert np.isfinite(res["val_loss"]) and res["val_loss"] > 0
    assert res["val_loss"] != pytest.approx(np.mean(res["val_loss_by_t"]["mse"]), rel=1e-3)  # the SNR weights are not 1


def test_train_chooses_and_records_the_checkpoint_by_val_loss(held_out, tmp_path, capsys):
    from dquartic.utils.synthetic import SyntheticDIAMSDataset

    train_loader = DataLoader(SyntheticDIAMSDataset(n_windows=4, RT=RT, MZ=MZ), batch_size=2, shuffle=False)
    val_loader = DataLoader(held_out, batch_size=4, shuffle=False)
    dm = make_dm(seed=2)
    ck_path = tmp_path / "val" / "best.ckpt"
    ck_path.parent.mkdir()
    dm.train(train_loader, 2, 2, warmup_epochs=0, learning_rate=1e-3, use_wandb=False, checkpoint_path=str(ck_path),
             val_dataloader=val_loader, val_every=1)
    out = capsys.readouterr().out
    assert out.count("val_loss=") == 2
    best = torch.load(ck_path, map_location="cpu", weights_only=False)
    latest = torch.load(ck_path.parent / "dquartic_latest_checkpoint.ckpt", map_location="cpu", weights_only=False)
    assert set(best) == OLD_KEYS | {"val_loss"} and set(latest) == OLD_KEYS | {"val_loss"}
    assert best["best_loss"] == best["val_loss"] and np.isfinite(best["val_loss"])
    assert best["val_loss"] <= latest["val_loss"]
    assert dm.model.training  # evaluate() hands the network back in the mode it found it
    # the held-out loss of the weights as they are now is what the last epoch recorded
    assert dm.evaluate(val_loader)["val_loss"] == latest["val_loss"]


@pytest.mark.parametrize("native_sampler", [False, True], ids=["generic_sampler", "native_sampler"])
def test_cli_train_with_validation_then_evaluate(tmp_path, native_sampler):
    """``dquartic train`` with a data.validation block, then ``dquartic evaluate`` on the checkpoint it chose: one JSON line"""
    from click.testing import CliRunner
    from dquartic.cli import cli

    cfg_path = str(tmp_path / "c.json")
    r = CliRunner().invoke(cli, ["generate-config", cfg_path])
    assert r.exit_code == 0, r.output
    cfg = json.load(open(cfg_path))
    cfg["model"].update(use_model="CustomTransformer", batch_size=2, num_epochs=1, warmup_epochs=0, checkpoint_path=str(tmp_path / "best.ckpt"))
    cfg["model"]["CustomTransformer"] = {"input_dim": MZ, "hidden_dim": 32, "num_heads": 2, "num_layers": 1, "native_sampler": native_sampler}
    cfg["data"]["synthetic"] = {"n_windows": 4, "RT": RT, "MZ": MZ}
    cfg["data"]["validation"] = {"synthetic": {"n_windows": 4, "RT": RT, "MZ": MZ}, "n_pairs": 4}
    cfg["wandb"]["use_wandb"] = False
    cfg["threads"] = 0
    json.dump(cfg, open(cfg_path, "w"))
    r = CliRunner().invoke(cli, ["train", cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    assert r.output.count("val_loss=") == 1
    # (options first: the command group is chained, which ends a command's options at its positional argument)
    r = CliRunner().invoke(cli, ["evaluate", "--checkpoint", str(tmp_path / "best.ckpt"), "--num-steps", "2", cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    lines = [ln for ln in r.output.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert np.isfinite(res["val_loss"]) and res["n_windows"] == 4 and res["n_t"] == 4 and np.isfinite(res["pearson"])
    assert res["val_loss"] == torch.load(tmp_path / "best.ckpt", map_location="cpu", weights_only=False)["val_loss"]
