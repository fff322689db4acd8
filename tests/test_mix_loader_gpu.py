"""``ResidentMixLoader`` through the train, predict and evaluate loops and the command line: the default network at
RT = 16, MZ = 64 on 8 synthetic windows.  What the kernel computes is tests/test_mix_batch.py's business; here the loops must hand it on
unchanged, the held-out form must be the same set at every batch size, and a config without a ``data.mixture`` block must give what it
gave."""
import json

import numpy as np
import pytest
import torch

from test_mix_batch import same
from test_mix_host import mix_batch_ref

pytestmark = pytest.mark.gpu

RT, MZ, N_WINDOWS = 16, 64, 8
OLD_EVAL_KEYS = {"val_loss", "val_loss_by_t", "n_windows", "n_t", "seed"}


@pytest.fixture(scope="module")
def dataset():
    from dquartic.utils.synthetic import SyntheticDIAMSDataset

    return SyntheticDIAMSDataset(n_windows=N_WINDOWS, RT=RT, MZ=MZ)


def _model(cls=None):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True).cuda()
    return (cls or DDIMDiffusionModel)(model_class=net, device="cuda")


@pytest.fixture(scope="module")
def dm():
    return _model()


def test_train_one_epoch_gets_the_kernels_batches(dataset):
    """the spy of test_pairs.py: target, mixture and MS1 reach _train_one_batch as the kernel wrote them, and a seed names the epochs"""
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.utils.data_loader import ResidentMixLoader, draw_mix_indices

    seen = []

    class Cap(DDIMDiffusionModel):
        def _train_one_batch(self, x_0, ms2_cond=None, ms1_cond=None, noise=None, ms1_loss_weight=0.0, **kw):
            seen.append((x_0.cpu().numpy(), ms2_cond.cpu().numpy(), ms1_cond.cpu().numpy()))
            return 0.0

    cap = _model(Cap)
    runs = []
    for _ in range(2):
        seen.clear()
        loader = ResidentMixLoader(dataset, 3, n_components=(1, 4), max_ratio_log2=4, seed=5, device="cuda")
        assert len(loader) == 3  # ceil(8 / 3)
        cap._train_one_epoch(0, loader)
        cap._train_one_epoch(1, loader)
        runs.append(list(seen))
    assert len(runs[0]) == 6 and [b[0].shape[0] for b in runs[0]] == [3, 3, 2, 3, 3, 2]
    for a, b in zip(*runs):  # two epochs under one seed repeat bit for bit
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    assert not np.array_equal(runs[0][0][1], runs[0][3][1])  # and the second epoch is not the first
    # the batches are the transcription's for the indices the host function draws and the weights of (seed + rank, batch number, position)
    rng = np.random.default_rng((5, 0))
    for draw, (x0, c2, c1) in enumerate(runs[0]):
        idx, count = draw_mix_indices(N_WINDOWS, x0.shape[0], (1, 4), rng, dataset.valid_pair)
        ref = mix_batch_ref(dataset.ms2, dataset.ms1, idx, count, 4, None, 4, 5, None, draw, True)
        assert same(x0, ref["ms2_target"]) and same(c2, ref["ms2_cond"]) and same(c1, ref["ms1_target"]), draw
    # scale_target=False hands the unscaled target on; fixed weights are the kernel's fixed form
    seen.clear()
    cap._train_one_epoch(0, ResidentMixLoader((dataset.ms2, dataset.ms1), 8, n_components=(2, 2), weights=(0.7, 0.3), scale_target=False, seed=1))
    idx, count = draw_mix_indices(N_WINDOWS, 8, (2, 2), np.random.default_rng((1, 0)))
    ref = mix_batch_ref(dataset.ms2, dataset.ms1, idx, count, 2, (0.7, 0.3), 3, None, None, 0, False)
    assert len(seen) == 1 and same(seen[0][0], ref["ms2_target"]) and same(seen[0][1], ref["ms2_cond"])


def test_frozen_loader_evaluates_the_same_set_at_every_batch_size(dataset, dm):
    from dquartic.utils.data_loader import MixBatch, ResidentMixLoader

    frozen = lambda bs: ResidentMixLoader(dataset, bs, n_components=(1, 4), max_ratio_log2=4, seed=3, frozen_items=N_WINDOWS, device="cuda")
    batches = list(frozen(8))
    assert len(batches) == 1 and isinstance(batches[0], MixBatch) and batches[0][3] is None and batches[0].weights.shape == (8, 4)
    halves = list(frozen(2))
    assert len(frozen(2)) == 4 and len(frozen(3)) == 3
    for part in ("ms2_cond", "weights"):  # item k is item k, whatever the batch it arrives in
        assert torch.equal(torch.cat([getattr(b, part) for b in halves]), getattr(batches[0], part))
    assert torch.equal(torch.cat([b[0] for b in halves]), batches[0][0]) and torch.equal(torch.cat([b[2] for b in halves]), batches[0][2])
    res = [dm.evaluate(frozen(bs), n_t=2, seed=1) for bs in (2, 8, 8)]
    for r in res:
        assert set(r) == OLD_EVAL_KEYS | {"target_weight", "val_loss_by_weight"}
        assert r["target_weight"].dtype == np.float32 and r["target_weight"].shape == (N_WINDOWS,)
        assert np.array_equal(r["target_weight"], batches[0].weights[:, 0].cpu().numpy())
        by = r["val_loss_by_weight"]
        assert by["edges"] == [0, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 1] and set(by) == {"edges", "mse", "n"}
        assert sum(by["n"]) == r["n_windows"] == N_WINDOWS
        assert all((m is None) == (n == 0) for m, n in zip(by["mse"], by["n"])) and all(np.isfinite(m) for m in by["mse"] if m is not None)
    for r in res[1:]:
        assert r["val_loss"] == res[0]["val_loss"] and np.array_equal(r["target_weight"], res[0]["target_weight"])
        assert r["val_loss_by_weight"] == res[0]["val_loss_by_weight"] and r["val_loss_by_t"] == res[0]["val_loss_by_t"]
    # with sampling: the mean spectral angle per bucket beside the loss
    r = dm.evaluate(frozen(8), n_t=2, seed=1, num_steps=2)
    by = r["val_loss_by_weight"]
    assert set(by) == {"edges", "mse", "n", "sa"} and by["mse"] == res[0]["val_loss_by_weight"]["mse"]
    sa = r["per_window"][:, 3].astype(np.float64)
    which = np.searchsorted([1 / 16, 1 / 8, 1 / 4, 1 / 2], r["target_weight"].astype(np.float64), side="left")
    assert by["sa"] == [float(sa[which == k].mean()) if (which == k).any() else None for k in range(5)]
    # predict hands the weights on; a pair loader's dicts have the keys they had
    preds = dm.predict(frozen(4), num_steps=2)
    assert len(preds) == 2 and set(preds[0]) == {"ms2_1", "ms1_1", "mixture", "pred", "weights"}
    assert np.array_equal(np.concatenate([p["weights"] for p in preds]), batches[0].weights.cpu().numpy())
    assert np.array_equal(preds[1]["mixture"], batches[0].ms2_cond[4:].cpu().numpy())


def test_without_weights_evaluate_and_predict_return_what_they_returned(dataset, dm):
    from torch.utils.data import DataLoader

    from dquartic.utils.synthetic import FrozenPairDataset

    pairs = DataLoader(FrozenPairDataset(dataset, 4, seed=0), batch_size=2, shuffle=False)
    assert set(dm.evaluate(pairs, n_t=2, seed=1)) == OLD_EVAL_KEYS
    assert set(dm.predict(pairs, num_steps=2)[0]) == {"ms2_1", "ms1_1", "mixture", "pred"}


def test_cli_train_and_evaluate_with_a_mixture_block(tmp_path):
    from click.testing import CliRunner

    from dquartic.cli import cli

    cfg_path = str(tmp_path / "c.json")
    assert CliRunner().invoke(cli, ["generate-config", cfg_path]).exit_code == 0
    cfg = json.load(open(cfg_path))
    cfg["model"].update(batch_size=4, num_epochs=1, warmup_epochs=0, checkpoint_path=str(tmp_path / "best.ckpt"))
    cfg["model"]["UNet1d"]["downsample_dim"] = MZ
    cfg["data"]["synthetic"] = {"n_windows": N_WINDOWS, "RT": RT, "MZ": MZ}
    cfg["data"]["mixture"] = {"n_components": [1, 4], "max_ratio_log2": 4, "seed": 2}
    cfg["data"]["validation"] = {"synthetic": {"n_windows": N_WINDOWS, "RT": RT, "MZ": MZ}, "n_pairs": 6, "seed": 9}
    cfg["wandb"]["use_wandb"] = False
    cfg["threads"] = 0
    json.dump(cfg, open(cfg_path, "w"))
    r = CliRunner().invoke(cli, ["train", cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    assert r.output.count("val_loss=") == 1
    ck = torch.load(tmp_path / "best.ckpt", map_location="cpu", weights_only=False)
    assert np.isfinite(ck["val_loss"])
    out_path = str(tmp_path / "res.json")
    r = CliRunner().invoke(cli, ["evaluate", "--checkpoint", str(tmp_path / "best.ckpt"), "--num-steps", "2", "--out", out_path, cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    lines = [ln for ln in r.output.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_windows"] == 6 and res["val_loss"] == ck["val_loss"]  # the held-out set of the training run, item for item
    by = res["val_loss_by_weight"]
    assert sum(by["n"]) == 6 and set(by) == {"edges", "mse", "n", "sa"} and "target_weight" not in res and "per_window" not in res
    full = json.load(open(out_path))
    assert len(full["target_weight"]) == 6 and all(0 < w <= 1 for w in full["target_weight"]) and len(full["per_window"]) == 6
    assert full["val_loss_by_weight"] == by
    # the same files without the block: pairs as ever, and the result has the keys it had
    del cfg["data"]["mixture"]
    json.dump(cfg, open(cfg_path, "w"))
    r = CliRunner().invoke(cli, ["evaluate", "--checkpoint", str(tmp_path / "best.ckpt"), cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    res = json.loads([ln for ln in r.output.splitlines() if ln.startswith("{")][0])
    assert set(res) == OLD_EVAL_KEYS and res["n_windows"] == 6
