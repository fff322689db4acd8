"""K-component mixtures, everything that needs no device: the numpy fp32 transcription of ``dq_mix_batch``'s rules
(``mix_weights_ref`` / ``mix_batch_ref``, which tests/test_mix_batch.py holds the kernel to bit for bit) and its own properties, the
refusals of the C entry (all before any launch), ``draw_mix_indices``, the ``data.mixture`` config block, and ``_batch_inputs``."""
import ctypes
import json

import numpy as np
import pytest
import torch

from test_guidance_host import _dm
from test_stochastic_sampler import SEED, philox4x32_10

_MASK = 0xFFFFFFFF
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- transcription
def mix_weights_ref(seed, ids, draw, counts, K, E):
    """(B, K) float32: w_j of every window.  a_j = (1 + m 2^-23) 2^e from the FOURTH Philox word of counter (j, draw, id lo, id hi);
    s = ((a_0 + a_1) + a_2) + ... in fp32 over the present components; w_j = a_j / s, 0 for j >= count."""
    ids = np.asarray([int(i) & (2 ** 64 - 1) for i in ids], dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.int64)
    seed = int(seed) & (2 ** 64 - 1)
    key = (np.full_like(ids, seed & _MASK), np.full_like(ids, seed >> 32))
    a = np.ones((len(ids), K), dtype=F32)
    for j in range(K):
        r3 = np.asarray(philox4x32_10((np.full_like(ids, j), np.full_like(ids, draw), ids & np.uint64(_MASK), ids >> np.uint64(32)), key)[3])
        if E > 0:
            m, e = r3 & np.uint64(0x7FFFFF), ((r3 >> np.uint64(23)) * np.uint64(E)) >> np.uint64(9)
            exact = (1.0 + m.astype(np.float64) * 2.0 ** -23) * 2.0 ** e.astype(np.float64)  # 24 significant bits: exact in fp32
            a[:, j] = exact.astype(F32)
            assert np.array_equal(a[:, j].astype(np.float64), exact)
    s = a[:, 0].copy()
    for j in range(1, K):
        s = np.where(j < counts, s + a[:, j], s).astype(F32)
    return np.where(np.arange(K)[None, :] < counts[:, None], a / s[:, None], F32(0)).astype(F32)


def mix_batch_ref(ms2, ms1, idx, count, K, weights, E, seed, ids, draw, scale_target):
    """What dq_mix_batch writes: dict of ms2_target, ms1_target, ms2_cond, ms2_rest, weights_out (all float32).  idx (K, B); count (B) or
    None; weights: K fixed floats or None (drawn under seed / ids (None: b) / draw)."""
    ms2, ms1 = np.asarray(ms2, dtype=F32), np.asarray(ms1, dtype=F32)
    n, B = len(ms2), idx.shape[1]
    counts = np.full(B, K) if count is None else np.asarray(count)
    if weights is None:
        w_all = mix_weights_ref(seed, range(B) if ids is None else ids, draw, counts, K, E)
    else:
        w_all = np.where(np.arange(K)[None, :] < counts[:, None], np.asarray(weights, dtype=F32)[None, :], F32(0)).astype(F32)
    out = {"ms2_target": np.empty((B,) + ms2.shape[1:], F32), "ms1_target": np.empty((B,) + ms1.shape[1:], F32),
           "weights_out": w_all.copy()}
    out["ms2_cond"], out["ms2_rest"] = np.empty_like(out["ms2_target"]), np.empty_like(out["ms2_target"])
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            c = int(counts[b])
            used = [int(idx[j, b]) for j in range(c)]  # rows j >= count are never read
            if not 1 <= c <= K or any(i < 0 or i >= n for i in used):
                for v in out.values():
                    v[b] = np.nan
                continue
            lo, hi = min(ms2[i].min() for i in used), max(ms2[i].max() for i in used)
            norm = [(ms2[i] - lo) / (hi - lo) for i in used]
            lo1, hi1 = ms1[used[0]].min(), ms1[used[0]].max()
            w = w_all[b]
            prod = [norm[j] * w[j] for j in range(c)]
            cond = prod[0]
            for j in range(1, c):
                cond = cond + prod[j]
            rest = np.zeros_like(cond)
            for j in range(1, c):
                rest = prod[j] if j == 1 else rest + prod[j]
            out["ms2_target"][b] = prod[0] if scale_target else norm[0]
            out["ms1_target"][b] = (ms1[used[0]] - lo1) / (hi1 - lo1)
            out["ms2_cond"][b], out["ms2_rest"][b] = cond, rest
    assert all(v.dtype == F32 for v in out.values())
    return out


@pytest.mark.parametrize("E", [0, 1, 4, 16])
def test_transcription_weight_properties(E):
    """over 10,000 ids: positive, summing to 1 within K 2^-23, max / min < 2^E (E = 0: all equal, exactly 1 / count)"""
    ids = np.arange(10_000) + (np.arange(10_000) % 7 == 0) * 2 ** 33
    K = 8
    for count in (1, 2, 3, 4, 8):
        w = mix_weights_ref(SEED, ids, 2, np.full(len(ids), count), K, E)
        p = w[:, :count].astype(np.float64)
        assert (p > 0).all() and (w[:, count:] == 0).all()
        assert np.abs(p.sum(axis=1) - 1.0).max() <= K * 2.0 ** -23
        ratio = p.max(axis=1) / p.min(axis=1)
        if E == 0:
            assert (w[:, :count] == (F32(1) / F32(count))).all()  # {1, 2, 4, 8}: exactly 1 / count; 3: fp32(1/3)
            assert (ratio == 1.0).all()
        else:
            assert (ratio < 2.0 ** E).all()
            if count > 1:
                assert ratio.max() > 2.0 ** (E - 1)  # the range is used: some window of 10,000 spans more than half of it (in octaves)
    assert mix_weights_ref(SEED, [5], 0, [3], 4, 0)[0].tolist() == [F32(1 / 3), F32(1 / 3), F32(1 / 3), 0.0]
    # the word is the fourth of counter (j, draw, id): spelled out for one window
    if E:
        r3 = int(philox4x32_10((1, 2, 7, 0), (SEED & _MASK, SEED >> 32))[3])
        a1 = (1 + (r3 & 0x7FFFFF) * 2.0 ** -23) * 2.0 ** (((r3 >> 23) * E) >> 9)
        r3 = int(philox4x32_10((0, 2, 7, 0), (SEED & _MASK, SEED >> 32))[3])
        a0 = (1 + (r3 & 0x7FFFFF) * 2.0 ** -23) * 2.0 ** (((r3 >> 23) * E) >> 9)
        w = mix_weights_ref(SEED, [7], 2, [2], 2, E)[0]
        assert w[0] == F32(a0) / (F32(a0) + F32(a1)) and w[1] == F32(a1) / (F32(a0) + F32(a1))
    # a window decides from (seed, id, draw) alone; another draw or seed is another weight
    w5 = mix_weights_ref(SEED, [9, 2 ** 33 + 1, 4], 2, [3, 3, 3], 3, E)
    assert np.array_equal(w5[1], mix_weights_ref(SEED, [2 ** 33 + 1], 2, [3], 3, E)[0])
    if E:
        assert not np.array_equal(w5, mix_weights_ref(SEED, [9, 2 ** 33 + 1, 4], 3, [3, 3, 3], 3, E))
        assert not np.array_equal(w5, mix_weights_ref(SEED + 1, [9, 2 ** 33 + 1, 4], 2, [3, 3, 3], 3, E))


def test_transcription_of_the_batch_rules():
    rng = np.random.default_rng(0)
    ms2, ms1 = rng.random((6, 3, 4), dtype=F32), rng.random((6, 3), dtype=F32)
    idx = np.array([[0, 1, 2], [3, 4, 6], [5, -1, 1]])
    r = mix_batch_ref(ms2, ms1, idx, [3, 1, 2], 3, None, 3, SEED, None, 0, True)
    w = r["weights_out"]
    # window 0: three components; the target is the product that entered the mixture, and cond = target + rest up to one rounding
    lo, hi = ms2[[0, 3, 5]].min(), ms2[[0, 3, 5]].max()
    assert np.array_equal(r["ms2_target"][0], ((ms2[0] - lo) / (hi - lo)) * w[0, 0])
    assert np.abs(r["ms2_cond"][0] - (r["ms2_target"][0] + r["ms2_rest"][0])).max() <= 2.0 ** -23
    # window 1: alone (its unused rows hold -1 and 4: never read) -> weight 1, the mixture is the target, nothing else
    assert w[1].tolist() == [1.0, 0.0, 0.0] and np.array_equal(r["ms2_cond"][1], r["ms2_target"][1]) and (r["ms2_rest"][1] == 0).all()
    assert r["ms2_target"][1].min() == 0 and r["ms2_target"][1].max() == 1 and r["ms1_target"][1].min() == 0 and r["ms1_target"][1].max() == 1
    # window 2: a used index of 6 = n_windows poisons it, every output
    assert all(np.isnan(v[2]).all() for v in r.values())
    # fixed weights are used as they are; unscaled target
    r = mix_batch_ref(ms2, ms1, idx[:2, :2], None, 2, (0.7, 0.3), 0, None, None, 0, False)
    lo, hi = ms2[[0, 3]].min(), ms2[[0, 3]].max()
    n0, n1 = (ms2[0] - lo) / (hi - lo), (ms2[3] - lo) / (hi - lo)
    assert np.array_equal(r["ms2_target"][0], n0) and np.array_equal(r["ms2_cond"][0], n0 * F32(0.7) + n1 * F32(0.3))
    assert np.array_equal(r["weights_out"], np.array([[0.7, 0.3]] * 2, dtype=F32))


# ---------------------------------------------------------------------------------------------------------------- the C entry
def test_native_refusals_and_scratch_size():
    from dquartic import _native as N

    lib = N.lib()
    d = ctypes.c_void_p(4096)
    w2 = (ctypes.c_float * 8)(*([0.5] * 8))

    def call(ms2=d, ms1=d, n=4, idx=d, count=None, B=2, K=2, RT=2, MZ=4, ms1_per=2, weights=None, E=3, seed=d, ids=None, draw=0, tgt=d,
             m1=d, cond=d, rest=None, wout=d, scratch=d, nbytes=1 << 20):
        return lib.dq_mix_batch(ms2, ms1, n, idx, count, B, K, RT, MZ, ms1_per, weights, E, seed, ids, draw, 1, tgt, m1, cond, rest, wout,
                                scratch, nbytes, None)

    cases = [(dict(ms2=None), b"null argument"), (dict(ms1=None), b"null argument"), (dict(idx=None), b"null argument"),
             (dict(tgt=None), b"null argument"), (dict(m1=None), b"null argument"), (dict(cond=None), b"null argument"),
             (dict(wout=None), b"null argument"), (dict(scratch=None), b"null argument"),
             (dict(K=1), b"K must be 2..8"), (dict(K=9), b"K must be 2..8"),
             (dict(E=-1), b"max_ratio_log2 must be 0..16"), (dict(E=17), b"max_ratio_log2 must be 0..16"),
             (dict(E=17, weights=w2), b"max_ratio_log2 must be 0..16"),
             (dict(draw=-1), b"draw index"), (dict(B=0), b"1..65535 windows"), (dict(B=65536), b"1..65535 windows"),
             (dict(RT=0), b"sizes must be positive"), (dict(MZ=-4), b"sizes must be positive"), (dict(ms1_per=0), b"sizes must be positive"),
             (dict(n=0), b"sizes must be positive"), (dict(RT=3, MZ=5), b"multiple of 4"),
             (dict(seed=None), b"need the seed"),
             (dict(nbytes=lib.dq_mix_batch_scratch_bytes(2, 2) - 1), b"scratch too small")]
    for kw, word in cases:
        assert call(**kw) != 0, kw
        err = lib.dq_last_error()
        assert word in err and b"dq_mix_batch" in err, (kw, err)
    # the order of the refusals: the earlier one speaks
    assert call(K=9, E=17) != 0 and b"K must be" in lib.dq_last_error()
    assert call(E=17, draw=-1) != 0 and b"max_ratio_log2" in lib.dq_last_error()
    assert call(seed=None, nbytes=0) != 0 and b"need the seed" in lib.dq_last_error()
    # (min, max) per chunk and one pair for MS1, per window: 8 chunks -> 72 bytes a window, whatever K; 0 for what the call refuses
    for K in (2, 3, 8):
        assert lib.dq_mix_batch_scratch_bytes(1, K) == 72 and lib.dq_mix_batch_scratch_bytes(512, K) == 512 * 72
        assert lib.dq_mix_batch_scratch_bytes(65535, K) == 65535 * 72
    assert lib.dq_mix_batch_scratch_bytes(0, 2) == 0 and lib.dq_mix_batch_scratch_bytes(-3, 2) == 0
    assert lib.dq_mix_batch_scratch_bytes(4, 1) == 0 and lib.dq_mix_batch_scratch_bytes(4, 9) == 0
    assert lib.dq_mix_batch_scratch_bytes(32, 2) == lib.dq_pair_batch_scratch_bytes(32)  # the pair form's layout


# ---------------------------------------------------------------------------------------------------------------- the index draw
def test_draw_mix_indices():
    from dquartic.utils.data_loader import draw_mix_indices

    idx, count = draw_mix_indices(10, 500, (2, 4), np.random.default_rng(3))
    idx2, count2 = draw_mix_indices(10, 500, (2, 4), np.random.default_rng(3))
    assert np.array_equal(idx, idx2) and np.array_equal(count, count2)  # a pure function of its arguments
    assert idx.shape == (4, 500) and idx.dtype == np.int64 and count.shape == (500,) and count.dtype == np.int32
    assert set(count.tolist()) == {2, 3, 4}
    assert abs((count == 2).mean() - 1 / 3) < 0.08 and abs((count == 4).mean() - 1 / 3) < 0.08  # uniform in [kmin, kmax]
    for b in range(500):
        used = idx[:count[b], b]
        assert len(set(used.tolist())) == count[b] and used.min() >= 0 and used.max() < 10  # distinct windows of the dataset
        assert (idx[count[b]:, b] == -1).all()  # unused rows: an index the kernel would refuse
    assert set(idx[0].tolist()) == set(range(10))  # every window is a target sooner or later
    assert not np.array_equal(idx, draw_mix_indices(10, 500, (2, 4), np.random.default_rng(4))[0])
    # the dataset's rule for pairs holds between the target and every other component
    rule = lambda i, j: i != j and (i % 2) != (j % 2)
    idx, count = draw_mix_indices(10, 200, (1, 3), np.random.default_rng(0), rule)
    assert set(count.tolist()) == {1, 2, 3}
    for b in range(200):
        assert all(rule(int(idx[0, b]), int(idx[j, b])) for j in range(1, count[b]))
        assert len(set(idx[:count[b], b].tolist())) == count[b]
    # kmin = 1: lone targets among the pairs; kmax = 1 is refused like the config block refuses it (K = kmax is the kernel's K, 2..8)
    idx, count = draw_mix_indices(3, 50, (1, 2), np.random.default_rng(0))
    assert idx.shape == (2, 50) and set(count.tolist()) == {1, 2} and (idx[1][count == 1] == -1).all()
    # the synthetic dataset's and the file dataset's valid_pair are accepted as they are
    from dquartic.utils.synthetic import SyntheticDIAMSDataset

    ds = SyntheticDIAMSDataset(n_windows=4, RT=8, MZ=8)
    idx, count = draw_mix_indices(len(ds), 20, (4, 4), np.random.default_rng(1), ds.valid_pair)
    assert all(sorted(idx[:, b].tolist()) == [0, 1, 2, 3] for b in range(20))
    for bad, word in ((dict(n_windows=3, n_components=(2, 4)), "at least 4 windows"), (dict(n_components=(0, 2)), "kmin"),
                      (dict(n_components=(3, 2)), "kmin"), (dict(n_components=(2, 9)), "kmin"), (dict(n_components=(1, 1)), "kmin"),
                      (dict(n_items=0), "at least one item")):
        kw = {"n_windows": 10, "n_items": 4, "n_components": (2, 4), **bad}
        with pytest.raises(ValueError, match=word):
            draw_mix_indices(kw["n_windows"], kw["n_items"], kw["n_components"], np.random.default_rng(0))
    with pytest.raises(ValueError, match="may be mixed with"):
        draw_mix_indices(4, 2, (2, 2), np.random.default_rng(0), lambda i, j: False)


# ---------------------------------------------------------------------------------------------------------------- config
def test_mixture_config_and_unchanged_default(tmp_path):
    from click.testing import CliRunner

    from dquartic import cli
    from dquartic.utils import config_loader as C

    assert C.mixture_config(None) is None
    assert C.mixture_config({}) == {"n_components": [2, 4], "max_ratio_log2": 3, "seed": 0, "scale_target": True}
    got = C.mixture_config({"n_components": [1, 8], "max_ratio_log2": 0, "seed": 7, "scale_target": False})
    assert got == {"n_components": [1, 8], "max_ratio_log2": 0, "seed": 7, "scale_target": False}
    for bad, word in (({"components": [2, 4]}, "unknown key"), ({"n_components": [0, 2]}, "n_components"), ({"n_components": [3, 2]}, "n_components"),
                      ({"n_components": [1, 1]}, "n_components"), ({"n_components": [2, 9]}, "n_components"), ({"n_components": 3}, "n_components"),
                      ({"n_components": [2.0, 4]}, "n_components"), ({"max_ratio_log2": 17}, "max_ratio_log2"), ({"max_ratio_log2": -1}, "max_ratio_log2"),
                      ({"max_ratio_log2": 2.5}, "max_ratio_log2"), ({"seed": "x"}, "seed"), ({"scale_target": 1}, "scale_target"), ([2, 4], "object")):
        with pytest.raises(ValueError, match=word):
            C.mixture_config(bad)
    # the default config and generate-config's output are what they were: no mixture, no validation
    p, p2 = str(tmp_path / "c.json"), str(tmp_path / "via_cli.json")
    C.generate_train_config(p)
    raw = json.load(open(p))
    assert raw == C.DEFAULT_CONFIG and set(raw["data"]) == {"parquet_directory", "ms2_data_path", "ms1_data_path", "normalize"}
    assert CliRunner().invoke(cli.cli, ["generate-config", p2]).exit_code == 0
    assert open(p2).read() == open(p).read() == json.dumps(C.DEFAULT_CONFIG, indent=4)
    assert C.mixture_config(C.load_train_config(p)["data"].get("mixture")) is None and C.validation_config(C.load_train_config(p)) is None

    def cfg(mixture, val):
        c = json.loads(json.dumps(C.DEFAULT_CONFIG))
        if mixture is not None:
            c["data"]["mixture"] = mixture
        c["data"]["validation"] = val
        return c

    syn = {"synthetic": {"n_windows": 8}}
    # the held-out set mixes what the training set mixes, under the validation block's own seed
    v = C.validation_config(cfg({"n_components": [2, 6], "max_ratio_log2": 5, "seed": 3, "scale_target": False}, {**syn, "seed": 11}))
    assert v["mixture"] == {"n_components": [2, 6], "max_ratio_log2": 5, "seed": 11, "scale_target": False}
    v = C.validation_config(cfg({"max_ratio_log2": 5}, {**syn, "mixture": {"n_components": [3, 3], "seed": 4}}))
    assert v["mixture"] == {"n_components": [3, 3], "max_ratio_log2": 5, "seed": 4, "scale_target": True}
    assert C.validation_config(cfg(None, {**syn, "mixture": {}}))["mixture"] == {**C.MIXTURE_DEFAULTS, "seed": 0}
    # no mixture anywhere, or an explicit null: the dict has the keys it always had
    old_keys = {"parquet_directory", "ms2_data_path", "ms1_data_path", "normalize", "synthetic", "n_pairs", "val_every", "seed"}
    assert set(C.validation_config(cfg(None, syn))) == old_keys and set(C.validation_config(cfg({}, {**syn, "mixture": None}))) == old_keys
    with pytest.raises(ValueError, match="data.validation.mixture"):
        C.validation_config(cfg(None, {**syn, "mixture": {"max_ratio_log2": 99}}))
    with pytest.raises(ValueError, match="data.mixture"):
        C.validation_config(cfg({"oops": 1}, syn))


# ---------------------------------------------------------------------------------------------------------------- the loops' helper
def test_batch_inputs_and_weight_buckets():
    from dquartic.model import evaluation as E
    from dquartic.utils.data_loader import MixBatch, PairBatch

    dm = _dm()
    g = torch.Generator().manual_seed(0)
    a, m1, b, m2 = torch.rand(3, 8, 8, generator=g), torch.rand(3, 8, generator=g), torch.rand(3, 8, 8, generator=g), torch.rand(3, 8, generator=g)
    for w in ((0.5, 0.5), (0.7, 0.3)):
        x0, cond, c1, weights = dm._batch_inputs((a, m1, b, m2), w)
        want = (a * w[0]).to(dm.device) + (b * w[1]).to(dm.device)  # the expression the three loops have always used
        assert weights is None and torch.equal(x0, a) and torch.equal(c1, m1) and torch.equal(cond.view(torch.int32), want.view(torch.int32))
        assert torch.equal(dm._batch_inputs([a, m1, b, m2], w)[1], want)  # a DataLoader's list
    formed = torch.full_like(a, 7.0)
    assert dm._batch_inputs(PairBatch((a, m1, b, m2), formed, (0.5, 0.5)))[1] is formed  # formed for these weights: taken
    x0, cond, c1, weights = dm._batch_inputs(PairBatch((a, m1, b, m2), formed, (0.5, 0.5)), (0.7, 0.3))  # for others: formed again
    assert weights is None and torch.equal(cond, a * 0.7 + b * 0.3)
    wk = torch.tensor([[0.25, 0.75, 0.0]] * 3)
    mb = MixBatch((a, m1, b, None), formed, wk)
    assert isinstance(mb, PairBatch) and len(mb) == 4 and mb[3] is None and mb.mixture_final and mb.ms2_cond is formed and mb.weights is wk
    for w in ((0.5, 0.5), (0.7, 0.3)):  # a final mixture is used as it is, whatever the loop's pair weights
        x0, cond, c1, weights = dm._batch_inputs(mb, w)
        assert cond is formed and weights is wk and torch.equal(x0, a) and torch.equal(c1, m1)
    # the buckets (lo, hi] of the target weight
    tw = np.array([1.0, 0.5, 0.500001, 0.25, 0.2, 1 / 16, 0.01, 0.13], dtype=np.float32)
    mse = np.arange(8, dtype=np.float64)
    r = E.by_target_weight(tw, mse)
    assert r["edges"] == [0, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 1] and r["n"] == [2, 0, 3, 1, 2] and sum(r["n"]) == 8 and "sa" not in r
    assert r["mse"] == [5.5, None, (3 + 4 + 7) / 3, 1.0, 1.0]
    pw = np.zeros((8, 9))
    pw[:, 3] = mse * 2
    assert E.by_target_weight(tw, mse, pw)["sa"] == [11.0, None, 2 * (3 + 4 + 7) / 3, 2.0, 2.0]
    json.dumps(r)
