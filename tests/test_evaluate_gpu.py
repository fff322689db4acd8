"""ModelInterface.evaluate and train(..., val_dataloader=...) on an 8-window synthetic held-out set (RT 16, MZ 64): reproducible,
independent of the batch size bit for bit, nine finite metrics with num_steps, and a checkpoint chosen by and holding val_loss."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

RT, MZ, N_WINDOWS = 16, 64, 8
OLD_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "best_loss"}  # tests/test_host_logic.py


def make_dm(seed=0):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True).cuda()
    return DDIMDiffusionModel(model_class=net, device="cuda")


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


def test_two_calls_return_the_same_dict(dm, held_out):
    loader = DataLoader(held_out, batch_size=4, shuffle=False)
    a, b = dm.evaluate(loader, num_steps=3), dm.evaluate(loader, num_steps=3)
    same(a, b)
    assert a["n_windows"] == N_WINDOWS and len(a["val_loss_by_t"]["mse"]) == 4 and len(a["val_loss_by_t"]["edges"]) == 5
    assert np.isfinite(a["val_loss"]) and a["val_loss"] > 0
    # eps objective: the weights are 1, so the loss is the mean of the bucket means
    assert a["val_loss"] == pytest.approx(np.mean(a["val_loss_by_t"]["mse"]), rel=1e-12)
    assert dm.evaluate(loader, seed=1)["val_loss"] != a["val_loss"]
    assert dm.evaluate(loader, max_batches=1)["n_windows"] == 4


def test_the_batch_size_does_not_change_a_bit(dm, held_out):
    a = dm.evaluate(DataLoader(held_out, batch_size=2, shuffle=False), num_steps=3)
    b = dm.evaluate(DataLoader(held_out, batch_size=8, shuffle=False), num_steps=3)
    assert np.array_equal(a["per_window"].view(np.int32), b["per_window"].view(np.int32))
    assert a["val_loss_by_t"] == b["val_loss_by_t"] and a["val_loss"] == b["val_loss"]


def test_num_steps_fills_all_nine_metrics(dm, held_out):
    from dquartic import _native as N

    loader = DataLoader(held_out, batch_size=4, shuffle=False)
    assert "per_window" not in dm.evaluate(loader) and "mse" not in dm.evaluate(loader)
    res = dm.evaluate(loader, num_steps=3, eta=1.0)
    assert res["per_window"].shape == (N_WINDOWS, 9) and res["per_window"].dtype == np.float32
    assert np.all(np.isfinite(res["per_window"]))
    for name in N.METRIC_NAMES:
        assert np.isfinite(res[name]), name
    assert 0 < res["scan_count"] <= RT and 0 < res["xic_count"] <= MZ
    assert -1 <= res["pearson"] <= 1 and -1 <= res["xic_r"] <= 1 and -1 <= res["sa"] <= 1
    assert res["num_steps"] == 3 and res["eta"] == 1.0


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

    dm2 = make_dm(seed=2)
    ck2 = tmp_path / "plain" / "best.ckpt"
    ck2.parent.mkdir()
    dm2.train(train_loader, 2, 2, warmup_epochs=0, learning_rate=1e-3, use_wandb=False, checkpoint_path=str(ck2))
    out = capsys.readouterr().out
    assert "val_loss" not in out
    assert set(torch.load(ck2, map_location="cpu", weights_only=False)) == OLD_KEYS
    assert set(torch.load(ck2.parent / "dquartic_latest_checkpoint.ckpt", map_location="cpu", weights_only=False)) == OLD_KEYS
