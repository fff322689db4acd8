"""``deconvolve_run`` and ``dquartic deconvolve`` on the GPU: the whole call against the numpy transcription of the
two kernels (tests/test_run_tiles_host.py) around ``dm.sample`` itself -- the transcription's windows sampled under the same ids and seed,
then the transcription's stitch -- bit for bit.  What ``sample`` computes is other files' business; here the call must cut, hand on, and
fold exactly what it says.

Network: the small one of tests/test_guided_sample.py (dim_mults = (1, 2), downsample_dim = 8), every parameter moved off its init so
that the conditions matter.  W = 4, RT_total = 11, step = 3: four windows starting at 0, 3, 6, 7 (a pulled-back tail; scans 3 and 6 .. 9
lie in two windows, the others in one).  4 sampling steps of num_timesteps = 20."""
import json

import numpy as np
import pytest
import torch

from test_mix_batch import same
from test_run_tiles_host import new_state, run_stitch_ref, run_windows_ref, starts_of

pytestmark = pytest.mark.gpu

RT_TOTAL, W, STEP, MZ, NS, T, SEED = 11, 4, 3, 8, 4, 20, 1234567
N_WIN = 4
UNET = dict(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=MZ, simple=True)

_CACHE = {}


def make_dm(seed):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    net = UNet1d(**UNET)
    with torch.no_grad():
        for p in net.parameters():
            if p.requires_grad:
                p.add_(0.3 * torch.randn_like(p))
    dm = DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=T, device="cuda")
    net.eval()
    return dm


def setup():
    """(dm, ms2 run, ms1 run) for the whole module; nothing below modifies them"""
    if not _CACHE:
        rng = np.random.default_rng(5)
        _CACHE["v"] = (make_dm(41), (rng.lognormal(0, 1, (RT_TOTAL, MZ)) * 50).astype(np.float32),
                       (rng.lognormal(0, 1, RT_TOTAL) * 500).astype(np.float32))
    return _CACHE["v"]


def reference(dm, ms2, ms1, taper="hann", id_offset=0, **opts):
    """the transcription's windows -> dm.sample under the ids and seed of the call -> the transcription's stitch"""
    from dquartic.utils.run_tiles import taper_table

    w2, w1, scale = run_windows_ref(ms2, ms1, W, STEP)
    ids = torch.arange(id_offset, id_offset + len(w2), dtype=torch.int64, device="cuda")
    pred, _ = dm.sample(None, ms2_cond=torch.from_numpy(w2).cuda(), ms1_cond=torch.from_numpy(w1).cuda(), num_steps=NS, window_ids=ids, **opts)
    mean, m2, wsum = run_stitch_ref(new_state(RT_TOTAL, MZ), pred.cpu().numpy(), scale, taper_table(taper, W), W, STEP)
    return {"pred": mean, "overlap_var": m2 / wsum[:, None], "coverage": wsum, "scales": scale}


def run(dm, ms2, ms1, **kw):
    res = dm.deconvolve_run(torch.from_numpy(ms2).cuda(), torch.from_numpy(ms1).cuda(), window=W, step=STEP, num_steps=NS, **kw)
    assert res["n_windows"] == N_WIN and res["starts"].tolist() == [0, 3, 6, 7] == starts_of(RT_TOTAL, W, STEP).tolist()
    return {k: res[k].cpu().numpy() for k in ("pred", "overlap_var", "coverage", "scales")}


def equal(a, b):
    return all(same(a[k], b[k]) for k in ("pred", "overlap_var", "coverage", "scales"))


@pytest.mark.parametrize("opts", [dict(seed=SEED), dict(seed=SEED, eta=1.0), dict(seed=SEED, sampler="dpmpp_2m", clip_x0=1.0)],
                         ids=["default", "eta1", "dpmpp_2m_clip"])
def test_the_call_is_windows_sample_stitch(opts):
    dm, ms2, ms1 = setup()
    for taper in ("hann", "uniform"):
        got, ref = run(dm, ms2, ms1, taper=taper, **opts), reference(dm, ms2, ms1, taper=taper, **opts)
        assert equal(got, ref), taper
        assert not any(np.isnan(v).any() for v in got.values())
        assert got["pred"].shape == (RT_TOTAL, MZ) and got["overlap_var"].shape == (RT_TOTAL, MZ) and got["coverage"].shape == (RT_TOTAL,)
        # scans 0 .. 2, 4, 5 and 10 lie in one window: no disagreement there; the others in two: some
        assert (got["overlap_var"][[0, 1, 2, 4, 5, 10]] == 0).all() and (got["overlap_var"][[3, 6, 7, 8, 9]] > 0).any()
    assert dm.last_seed == SEED
    # a 2-D MS1 of one channel and a custom taper table are the same call
    two_d = run(dm, ms2, ms1[:, None], taper=np.ones(W), **opts)
    assert equal(two_d, got)


def test_batch_size_and_id_offset():
    dm, ms2, ms1 = setup()
    opts = dict(seed=SEED, eta=1.0)
    whole = run(dm, ms2, ms1, batch_size=N_WIN, **opts)
    for bs in (1, 3):
        assert equal(run(dm, ms2, ms1, batch_size=bs, **opts), whole), bs
    # the ids are id_offset + i: another offset is another noise, and the reference's under the same ids
    shifted = run(dm, ms2, ms1, id_offset=5, batch_size=3, **opts)
    assert not np.array_equal(shifted["pred"], whole["pred"]) and np.array_equal(shifted["scales"], whole["scales"])
    assert equal(shifted, reference(dm, ms2, ms1, id_offset=5, **opts))
    # no seed: one is drawn, kept in last_seed, and gives the call again
    torch.manual_seed(0)
    drawn = run(dm, ms2, ms1)
    assert dm.last_seed is not None and equal(run(dm, ms2, ms1, seed=dm.last_seed), drawn)


def test_the_averaged_weights():
    dm, ms2, ms1 = setup()
    mine, other = make_dm(41), make_dm(7)
    mine._set_lr(1e-3)
    mine.enable_ema(0.99)
    with torch.no_grad():
        mine.optimizer.ema_buffer().copy_(other.model.flat_params)  # visibly different weights
    want = run(other, ms2, ms1, seed=SEED)  # the averaged weights loaded as the network's
    assert equal(run(mine, ms2, ms1, seed=SEED), want)  # use_ema=None: the average, because it is enabled
    assert equal(run(mine, ms2, ms1, seed=SEED, use_ema=True), want)
    with mine.ema_scope():
        assert equal(run(mine, ms2, ms1, seed=SEED, use_ema=False), want)
    plain = run(mine, ms2, ms1, seed=SEED, use_ema=False)
    assert equal(plain, run(dm, ms2, ms1, seed=SEED)) and not np.array_equal(plain["pred"], want["pred"])


def test_an_empty_run_gives_zeros():
    dm, _, _ = setup()
    got = run(dm, np.zeros((RT_TOTAL, MZ), np.float32), np.zeros(RT_TOTAL, np.float32), seed=SEED, eta=1.0)
    assert (got["pred"] == 0).all() and (got["overlap_var"] == 0).all() and (got["scales"] == 0).all() and (got["coverage"] > 0).all()
    assert not any(np.isnan(v).any() for v in got.values())


def test_cli_round_trip_on_two_runs(tmp_path):
    from click.testing import CliRunner

    from dquartic.cli import build_model, cli

    cfg_path, ck_path = str(tmp_path / "c.json"), str(tmp_path / "m.ckpt")
    assert CliRunner().invoke(cli, ["generate-config", cfg_path]).exit_code == 0
    cfg = json.load(open(cfg_path))
    cfg["model"]["num_timesteps"] = T
    cfg["model"]["UNet1d"].update(dim_mults=[1, 2], downsample_dim=MZ)
    json.dump(cfg, open(cfg_path, "w"))
    torch.manual_seed(3)
    dm = build_model(cfg["model"], torch.device("cuda"))
    with torch.no_grad():
        for p in dm.model.parameters():
            if p.requires_grad:
                p.add_(0.3 * torch.randn_like(p))
    torch.save({"model_state_dict": dm.model.state_dict()}, ck_path)
    rng = np.random.default_rng(9)
    ms2 = (rng.lognormal(0, 1, (2, RT_TOTAL, MZ)) * 50).astype(np.float32)
    ms1 = (rng.lognormal(0, 1, (2, RT_TOTAL)) * 500).astype(np.float32)
    p2, p1, out = str(tmp_path / "ms2.npy"), str(tmp_path / "ms1.npy"), str(tmp_path / "o.npz")
    np.save(p2, ms2)
    np.save(p1, ms1)
    common = ["--window", str(W), "--step", str(STEP), "--num-steps", str(NS), "--eta", "1.0", "--seed", "3", "--batch-size", "3"]
    r = CliRunner().invoke(cli, ["deconvolve", "--checkpoint", ck_path, "--ms2", p2, "--ms1", p1, "--out", out] + common + [cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    lines = [ln for ln in r.output.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert set(line) == {"runs", "windows", "windows_per_s"} and line["runs"] == 2 and line["windows"] == 2 * N_WIN and line["windows_per_s"] > 0
    z = np.load(out)
    assert set(z.files) == {"pred", "overlap_var", "coverage", "scales", "starts"} and z["starts"].tolist() == [0, 3, 6, 7]
    assert z["pred"].shape == (2, RT_TOTAL, MZ) and z["coverage"].shape == (2, RT_TOTAL) and z["scales"].shape == (2, N_WIN, 4)
    dm.model.eval()
    for r_i in range(2):  # run r's windows sample under the ids after those of the runs before it
        want = run(dm, ms2[r_i], ms1[r_i], seed=3, eta=1.0, id_offset=r_i * N_WIN)
        assert all(same(z[k][r_i], want[k]) for k in want), r_i
    # one run as a 2-D file: the arrays are not stacked
    np.save(p2, ms2[1])
    np.save(p1, ms1[1])
    r = CliRunner().invoke(cli, ["deconvolve", "--checkpoint", ck_path, "--ms2", p2, "--ms1", p1, "--out", out] + common + [cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    z = np.load(out)
    want = run(dm, ms2[1], ms1[1], seed=3, eta=1.0)
    assert all(same(z[k], want[k]) for k in want)
