"""Host side of the held-out evaluation (no GPU): the stratified timestep helper, the count-weighted aggregation of the per-window
metrics, the data.validation block of a train config, and the command line."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from dquartic import _native as N
from dquartic.cli import cli
from dquartic.model import evaluation as E
from dquartic.utils import config_loader as C


@pytest.mark.parametrize("n_t,T", [(4, 1000), (1, 1000), (3, 1000), (7, 50), (4, 4)])
def test_stratified_timesteps(n_t, T):
    ids = np.arange(0, 500)
    ts = np.stack([E.stratified_timesteps(ids, k, n_t, T) for k in range(n_t)])  # (n_t, windows)
    assert ts.dtype == np.int64 and ts.min() >= 0 and ts.max() <= T - 1
    edges = E.bucket_edges(n_t, T)
    assert len(edges) == n_t + 1 and edges[0] == 0 and edges[-1] == T
    for k in range(n_t):  # one value per bucket per window: the integer part of a point of [edges[k], edges[k + 1])
        assert np.all(ts[k] >= np.floor(edges[k])) and np.all(ts[k] < edges[k + 1])
    phi = (5 ** 0.5 - 1) / 2
    expect = np.minimum(np.floor(((ids * phi) % 1.0 + 2 % n_t) / n_t * T), T - 1).astype(np.int64)
    assert np.array_equal(ts[2 % n_t], expect)
    # reproducible, and a window's timesteps do not depend on the windows around it
    assert np.array_equal(ts, np.stack([E.stratified_timesteps(ids, k, n_t, T) for k in range(n_t)]))
    assert np.array_equal(E.stratified_timesteps([137], 0, n_t, T), ts[0, 137:138])
    assert np.array_equal(E.stratified_timesteps(ids[::-1], n_t - 1, n_t, T), ts[n_t - 1, ::-1])
    if T >= 100 * n_t:  # the offsets spread over the bucket: the windows do not all sit at one timestep
        assert len(np.unique(ts[0])) > 50


def test_stratified_timesteps_rejects_bad_arguments():
    for k, n_t, T in [(4, 4, 1000), (-1, 4, 1000), (0, 0, 1000), (0, 4, 0)]:
        with pytest.raises(ValueError):
            E.stratified_timesteps([0], k, n_t, T)


def test_aggregation_weights_scan_and_xic_scores_by_their_counts():
    names = N.METRIC_NAMES
    assert names == ("mse", "mae", "cosine", "sa", "pearson", "scan_sa", "scan_count", "xic_r", "xic_count")
    a = np.zeros((3, 9))
    a[:, names.index("mse")] = [1.0, 2.0, 6.0]
    a[:, names.index("scan_sa")] = [0.5, 0.9, 0.0]
    a[:, names.index("scan_count")] = [10, 30, 0]
    a[:, names.index("xic_r")] = [0.2, -0.4, 1.0]
    a[:, names.index("xic_count")] = [0, 1, 3]
    m = E.aggregate_metrics(a)
    assert m["mse"] == 3.0
    assert m["scan_sa"] == pytest.approx((0.5 * 10 + 0.9 * 30) / 40, rel=1e-15)
    assert m["xic_r"] == pytest.approx((-0.4 + 3.0) / 4, rel=1e-15)
    assert m["scan_count"] == pytest.approx(40 / 3) and m["xic_count"] == pytest.approx(4 / 3)
    a[:, names.index("scan_count")] = 0
    assert E.aggregate_metrics(a)["scan_sa"] == 0.0
    with pytest.raises(ValueError):
        E.aggregate_metrics(np.zeros((0, 9)))
    with pytest.raises(ValueError):
        E.aggregate_metrics(np.zeros((2, 8)))


def _config(tmp_path, validation=None):
    path = tmp_path / "cfg.json"
    C.generate_train_config(str(path))
    cfg = json.loads(path.read_text())
    if validation is not None:
        cfg["data"]["validation"] = validation
        path.write_text(json.dumps(cfg))
    return C.load_train_config(str(path))


def test_validation_block_is_parsed(tmp_path):
    assert C.validation_config(_config(tmp_path)) is None
    v = C.validation_config(_config(tmp_path, {"synthetic": {"n_windows": 8, "RT": 16}, "n_pairs": "8"}))
    assert v["synthetic"] == {"n_windows": 8, "RT": 16, "start": C.VALIDATION_SYNTHETIC_START}
    assert v["normalize"] == "minmax" and v["n_pairs"] == 8 and v["val_every"] == 1 and v["parquet_directory"] is None
    assert v["seed"] == 0 and C.validation_config(_config(tmp_path, {"synthetic": {"n_windows": 8}, "seed": "5"}))["seed"] == 5
    v = C.validation_config(_config(tmp_path, {"parquet_directory": "held_out/", "ms2_data_path": "a.npy", "ms1_data_path": "b.npy",
                                               "normalize": "minmax", "val_every": 5}))
    assert (v["parquet_directory"], v["ms2_data_path"], v["ms1_data_path"], v["val_every"]) == ("held_out/", "a.npy", "b.npy", 5)
    assert v["synthetic"] is None and v["n_pairs"] is None
    v = C.validation_config(_config(tmp_path, {"synthetic": {"n_windows": 4, "start": 77}}))
    assert v["synthetic"]["start"] == 77
    for bad in ({"synthetic": {"n_windows": 4}, "batch": 3}, {"normalize": "minmax"}, {"synthetic": {}, "n_pairs": 0},
                {"synthetic": {"n_windows": 2}, "val_every": 0}, "held_out/"):
        with pytest.raises(ValueError):
            C.validation_config(_config(tmp_path, bad))


def test_default_config_has_no_validation_block(tmp_path):
    """generate-config writes what it always wrote: the validation block is opt-in."""
    assert "validation" not in C.DEFAULT_CONFIG["data"]
    assert set(C.DEFAULT_CONFIG["data"]) == {"parquet_directory", "ms2_data_path", "ms1_data_path", "normalize"}
    path = tmp_path / "generated.json"
    res = CliRunner().invoke(cli, ["generate-config", str(path)])
    assert res.exit_code == 0, res.output
    assert json.loads(path.read_text()) == C.DEFAULT_CONFIG


def test_frozen_pairs_serve_the_same_windows_every_time():
    import torch

    from dquartic.utils.synthetic import FrozenPairDataset, SyntheticDIAMSDataset

    ds = FrozenPairDataset(SyntheticDIAMSDataset(n_windows=4, RT=8, MZ=16, start=1000), 6)
    assert len(ds) == 6
    again = [ds[i] for i in range(6)]
    assert all(torch.equal(a, b) for i in range(6) for a, b in zip(ds[i], again[i]))
    assert not torch.equal(ds[0][0], ds[1][0]) or not torch.equal(ds[0][2], ds[1][2])
    held_out = SyntheticDIAMSDataset(n_windows=2, RT=8, MZ=16, start=1000).ms2
    train = SyntheticDIAMSDataset(n_windows=2, RT=8, MZ=16).ms2
    assert not np.array_equal(held_out, train)


def test_cli_lists_the_evaluate_command():
    res = CliRunner().invoke(cli, ["--help"])
    assert res.exit_code == 0 and "evaluate" in res.output
    res = CliRunner().invoke(cli, ["evaluate", "--help"])
    assert res.exit_code == 0
    for opt in ("--checkpoint", "--num-steps", "--eta", "--seed", "--use-ema", "--no-use-ema", "--max-batches", "--out"):
        assert opt in res.output, opt


def test_frozen_pairs_of_a_file_dataset_are_the_same_in_every_construction(tmp_path):
    """DIAMSDataset draws its pairs from the process-wide `random` module; a held-out set over it must not: the index pairs come from a
    generator of their own, so two constructions (two processes, two runs, a restart) serve identical items whatever `random` did between."""
    import random

    import torch

    from dquartic.utils.data_loader import DIAMSDataset
    from dquartic.utils.synthetic import FrozenPairDataset

    rng = np.random.default_rng(3)
    np.save(tmp_path / "ms2.npy", rng.random((6, 5, 8), dtype=np.float32))
    np.save(tmp_path / "ms1.npy", rng.random((6, 5), dtype=np.float32))
    make = lambda: DIAMSDataset(None, str(tmp_path / "ms2.npy"), str(tmp_path / "ms1.npy"), normalize="minmax")
    random.seed(1)
    a = FrozenPairDataset(make(), 7, seed=0)
    first = [a[k] for k in range(len(a))]
    random.seed(99)
    [random.random() for _ in range(11)]
    b = FrozenPairDataset(make(), 7, seed=0)
    assert a.index_pairs == b.index_pairs and len(b) == 7
    assert all(i != j and 0 <= i < 6 and 0 <= j < 6 for i, j in a.index_pairs)
    for k in range(7):
        assert all(torch.equal(u, v) for u, v in zip(first[k], b[k]))
        assert all(torch.equal(u, v) for u, v in zip(first[k], a[k]))  # ... and on every access
    assert FrozenPairDataset(make(), 7, seed=1).index_pairs != a.index_pairs
    assert len(FrozenPairDataset(make())) == 6  # n_pairs None: one pair per window
    # item k is the dataset's own normalised pair of those two windows
    i, j = a.index_pairs[0]
    assert all(torch.equal(u, v) for u, v in zip(first[0], make().pair(i, j)))
