"""``ModelInterface.evaluate_joint`` and ``dquartic evaluate-joint`` on the GPU: the small network of
tests/test_joint_sample.py, 4 steps, 6 frozen groups of P = 2 members out of mixtures of 2 .. 3 components (K = 3)."""
import json

import numpy as np
import pytest
import torch

from joint_ref import U
from test_joint_sample import MZ, RT, T, model

pytestmark = pytest.mark.gpu

NS, N_GROUPS, P, SEED, N_POOL = 4, 6, 2, 99, 9
LOADER = dict(n_components=(2, 3), max_ratio_log2=3, seed=5, scale_target=True, frozen_items=N_GROUPS, device="cuda")
SCALARS = {"mse", "mae", "cosine", "sa", "pearson", "scan_sa", "scan_count", "xic_r", "xic_count", "excess", "unexplained", "id_acc", "leak",
           "sa_by_weight"}
ARRAYS = {"per_window", "cross", "group"}
_CACHE = {}


def arrays():
    rng = np.random.default_rng(17)
    return (rng.lognormal(0, 1, (N_POOL, RT, MZ)) * 50).astype(np.float32), (rng.lognormal(0, 1, (N_POOL, RT)) * 500).astype(np.float32)


def groups(per_batch, group_size=P):
    from dquartic.utils.data_loader import ResidentGroupLoader

    return ResidentGroupLoader(arrays(), per_batch, group_size, **LOADER)


def result(per_batch, consistency="bound", normalize=True, **kw):
    """evaluate_joint of the eps model over the frozen groups, computed once per configuration for the module and left unchanged"""
    key = (per_batch, consistency, normalize, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = model("eps", normalize).evaluate_joint(groups(per_batch), NS, consistency=consistency, seed=SEED, **kw)
    return _CACHE[key]


def same_result(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            same_result(a[k], b[k])
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


def test_the_result_and_its_keys():
    r = result(4)
    assert set(r) == {"joint", "independent", "n_groups", "group_size", "num_steps", "eta", "seed", "consistency", "consistency_strength",
                      "member_weight"}
    assert (r["n_groups"], r["group_size"], r["num_steps"], r["eta"], r["seed"], r["consistency"], r["consistency_strength"]) == (
        N_GROUPS, P, NS, 0.0, SEED, "bound", 1.0)
    assert r["member_weight"].shape == (P * N_GROUPS,) and r["member_weight"].dtype == np.float32 and (r["member_weight"] > 0).all()
    for leg in ("joint", "independent"):
        assert set(r[leg]) == SCALARS | ARRAYS
        assert r[leg]["per_window"].shape == (P * N_GROUPS, 9) and r[leg]["cross"].shape == (N_GROUPS, P, P) and r[leg]["group"].shape == (N_GROUPS, 3)
        assert all(np.isfinite(r[leg][k]).all() for k in ARRAYS) and 0.0 <= r[leg]["id_acc"] <= 1.0 and sum(r[leg]["sa_by_weight"]["n"]) == P * N_GROUPS
        assert r[leg]["excess"] == float(r[leg]["group"][:, 0].astype(np.float64).mean())
        json.dumps({k: v for k, v in r[leg].items() if k not in ARRAYS})
    assert not np.array_equal(r["joint"]["per_window"], r["independent"]["per_window"])  # the pass did something
    assert r["joint"]["excess"] < r["independent"]["excess"]  # and what it is for: the untrained members over-explain, the bound stops them
    assert "independent" not in result(4, independent=False)
    same_result(result(4, independent=False)["joint"], r["joint"])
    other = result(4, consistency="sum", consistency_strength=0.5, sampler="ddim")
    assert (other["consistency"], other["consistency_strength"], other["sampler"]) == ("sum", 0.5, "ddim") and "clip_x0" not in other


@pytest.mark.parametrize("per_batch", [1, 2])
def test_nothing_depends_on_the_groups_per_batch(per_batch):
    """6 groups in batches of 4 (a tail batch of 2), 2 and 1: every scalar and every array bit for bit"""
    same_result(result(per_batch), result(4))


def test_member_0_of_the_independent_leg_is_evaluate_on_the_mixture_loader():
    from dquartic.utils.data_loader import ResidentMixLoader

    dm = model("eps")
    ev = dm.evaluate(ResidentMixLoader(arrays(), 4, **LOADER), num_steps=NS, seed=SEED, n_t=1)
    r = result(4)
    assert ev["per_window"].shape == (N_GROUPS, 9)
    assert ev["per_window"].tobytes() == r["independent"]["per_window"][:N_GROUPS].tobytes()
    assert ev["target_weight"].tobytes() == r["member_weight"][:N_GROUPS].tobytes()


@pytest.mark.parametrize("group_size", [2, 1])
def test_the_bound_leg_is_the_hand_loop(group_size):
    """form, sample(group_size=, consistency="bound"), dq_recon_metrics, dq_group_metrics, batch by batch; at P = 1 the loader's groups are
    the mixture loader's windows, every member is identified and there is no leak"""
    from dquartic import _native as N
    from dquartic.model import evaluation as E

    dm, Pg = model("eps"), group_size
    loader = groups(4, Pg)
    got = dm.evaluate_joint(groups(4, Pg), NS, consistency="bound", independent=False, seed=SEED)
    idx, count = loader.frozen
    pw, cross, group = [], [], []
    dm.model.eval()
    for first in range(0, N_GROUPS, 4):
        last = min(first + 4, N_GROUPS)
        G = last - first
        batch = loader.form(idx[:, first:last], count[first:last], draw=0, window_ids=np.arange(first, last, dtype=np.int64))
        ids = torch.tensor([p * N_GROUPS + k for p in range(Pg) for k in range(first, last)], dtype=torch.int64, device="cuda")
        with torch.no_grad():
            s, _ = dm.sample(None, ms2_cond=batch.ms2_cond, ms1_cond=batch[1], num_steps=NS, eta=0.0, seed=SEED, window_ids=ids,
                             shape=tuple(batch[0].shape), group_size=Pg, consistency="bound")
        m = E.recon_metrics(s, batch[0])
        c = torch.empty(G, Pg, Pg, device="cuda")
        g = torch.empty(G, 3, device="cuda")
        nbytes = N.lib().dq_group_metrics_scratch_bytes(G, Pg, RT, MZ)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        N.check(N.lib().dq_group_metrics(N.ptr(s), N.ptr(batch[0]), N.ptr(batch.ms2_cond), N.ptr(c), N.ptr(g), N.ptr(scratch), nbytes, G, Pg, RT, MZ,
                                         N.stream_ptr()), "dq_group_metrics")
        pw.append(m.view(Pg, G, 9).cpu().numpy())
        cross.append(c.cpu().numpy())
        group.append(g.cpu().numpy())
    j = got["joint"]
    assert j["per_window"].tobytes() == np.concatenate(pw, axis=1).reshape(Pg * N_GROUPS, 9).tobytes()
    assert j["cross"].tobytes() == np.concatenate(cross).tobytes() and j["group"].tobytes() == np.concatenate(group).tobytes()
    assert got["group_size"] == Pg and got["n_groups"] == N_GROUPS
    if Pg == 1:
        assert j["id_acc"] == 1.0 and "leak" not in j and j["cross"].shape == (N_GROUPS, 1, 1)
        cos = j["per_window"][:, 2]  # one member: the cross matrix is the window's cosine (another summation order: within 1 ulp)
        assert (np.abs(j["cross"][:, 0, 0].astype(np.float64) - cos) <= np.spacing(np.abs(cos))).all()
    else:
        assert "leak" in j and same_bits(got, result(4, independent=False))


def same_bits(a, b):
    same_result(a, b)
    return True


@pytest.mark.parametrize("normalize", [False, True])
def test_the_excess_of_the_bound_leg_stays_within_the_rule(normalize):
    """tests/test_joint_sample.py's bound for the final sample, in its configuration (strength 1, the reference sampler, whose last row
    returns the projected x0 estimate): per element the members' positive parts sum to at most m (1 + (P + 1) 2^-24), plus -- with
    auto_normalize -- the roundings of the map back to the network's units, 2^-24 (|x0| + |x0 + 1|) / 2 per member.  Summed over a group and
    divided by sum m+ that is the bound on `excess`; one more 2^-24 for the output's own rounding."""
    dm = model("eps", normalize)
    loader = groups(N_GROUPS)
    batch = next(iter(loader))
    r = result(N_GROUPS, normalize=normalize, independent=False)["joint"]
    ids = torch.from_numpy(dm.joint_window_ids(0, N_GROUPS, P, 0, N_GROUPS)).cuda()
    with torch.no_grad():
        s, _ = dm.sample(None, ms2_cond=batch.ms2_cond, ms1_cond=batch[1], num_steps=NS, seed=SEED, window_ids=ids, shape=tuple(batch[0].shape),
                         group_size=P, consistency="bound")
    y = s.cpu().numpy().astype(np.float64).reshape(P, N_GROUPS, RT * MZ)
    m = np.maximum(batch.ms2_cond[:N_GROUPS].cpu().numpy().astype(np.float64).reshape(N_GROUPS, RT * MZ), 0)
    x0 = 2 * y - 1
    slack = (U * (np.abs(x0) + np.abs(x0 + 1)) / 2).sum(axis=0) if normalize else np.zeros_like(m)
    bound = ((m * (P + 1) * U + slack).sum(axis=1) / m.sum(axis=1)) * (1 + U) + U
    print("excess", r["group"][:, 0].tolist(), "bound", bound.tolist())
    assert (r["group"][:, 0].astype(np.float64) <= bound).all()
    assert (result(N_GROUPS, normalize=normalize)["independent"]["group"][:, 0] > 1e-3).all()  # (without the pass the same members exceed it)


def test_evaluate_joint_through_the_command(tmp_path):
    from click.testing import CliRunner

    from dquartic.cli import build_model, cli

    cfg_path, ck_path, out_path = str(tmp_path / "c.json"), str(tmp_path / "m.ckpt"), str(tmp_path / "o.json")
    assert CliRunner().invoke(cli, ["generate-config", cfg_path]).exit_code == 0
    cfg = json.load(open(cfg_path))
    cfg["model"].update(num_timesteps=T, batch_size=4)
    cfg["model"]["UNet1d"].update(dim_mults=[1, 2], downsample_dim=MZ)
    cfg["data"]["validation"] = {"synthetic": {"n_windows": 8, "RT": RT, "MZ": MZ}, "n_pairs": N_GROUPS, "seed": 9,
                                 "mixture": {"n_components": [2, 3], "max_ratio_log2": 3}}
    json.dump(cfg, open(cfg_path, "w"))
    torch.manual_seed(3)
    dm = build_model(cfg["model"], torch.device("cuda"))
    with torch.no_grad():
        for p in dm.model.parameters():
            if p.requires_grad:
                p.add_(0.3 * torch.randn_like(p))
    torch.save({"model_state_dict": dm.model.state_dict()}, ck_path)
    r = CliRunner().invoke(cli, ["evaluate-joint", "--checkpoint", ck_path, "--num-steps", str(NS), "--group-size", str(P), "--seed", "3",
                                 "--out", out_path, cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    lines = [ln for ln in r.output.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert set(line) == {"joint", "independent", "n_groups", "group_size", "num_steps", "eta", "seed", "consistency", "consistency_strength"}
    assert (line["n_groups"], line["group_size"], line["num_steps"], line["seed"], line["consistency"]) == (N_GROUPS, P, NS, 3, "bound")
    assert set(line["joint"]) == SCALARS == set(line["independent"])
    full = json.load(open(out_path))
    assert len(full["member_weight"]) == P * N_GROUPS and set(full["joint"]) == SCALARS | ARRAYS
    assert np.asarray(full["joint"]["cross"]).shape == (N_GROUPS, P, P) and np.asarray(full["independent"]["per_window"]).shape == (P * N_GROUPS, 9)
    assert {k: full["joint"][k] for k in SCALARS} == line["joint"]
    r = CliRunner().invoke(cli, ["evaluate-joint", "--checkpoint", ck_path, "--num-steps", str(NS), "--group-size", "1", "--consistency", "sum",
                                 "--no-independent", "--max-batches", "1", cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    line = json.loads([ln for ln in r.output.splitlines() if ln.startswith("{")][0])
    assert "independent" not in line and line["consistency"] == "sum" and line["n_groups"] == 4 and line["joint"]["id_acc"] == 1.0
    assert "leak" not in line["joint"]
