"""Deconvolving a whole chromatogram, everything that needs no device: the window rule against a brute-force loop
(Python's and the library's count), the refusals of the two C entries (all before any launch) and the scratch size, the numpy fp32
transcription of both kernels' rules (``run_windows_ref`` / ``run_stitch_ref``, which tests/test_run_tiles.py holds the kernels to bit
for bit and tests/test_deconvolve_gpu.py the whole call) with its own properties, ``deconvolve_run``'s argument checks and the CLI's
surface."""
import ctypes

import numpy as np
import pytest
import torch

from test_guidance_host import _dm

F32 = np.float32
U = 2.0 ** -24  # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------------------- transcription
def starts_of(RT_total, W, step):
    from dquartic.utils.run_tiles import run_window_starts

    return run_window_starts(RT_total, W, step)


def run_windows_ref(ms2_run, ms1_run, W, step, i0=0, B=None):
    """What dq_run_windows writes for windows i0 .. i0 + B - 1 (B None: to the last): (ms2_win (B, W, MZ), ms1_win (B, W, M1), scale (B, 4)),
    all float32.  n = (x - lo) / (hi - lo), every operation in fp32; a constant window gives zeros."""
    ms2_run, ms1_run = np.asarray(ms2_run, dtype=F32), np.asarray(ms1_run, dtype=F32)
    if ms1_run.ndim == 1:
        ms1_run = ms1_run[:, None]
    starts = starts_of(len(ms2_run), W, step)
    B = len(starts) - i0 if B is None else B
    w2, w1 = np.empty((B, W, ms2_run.shape[1]), F32), np.empty((B, W, ms1_run.shape[1]), F32)
    scale = np.empty((B, 4), F32)

    def norm(x):
        lo, hi = x.min(), x.max()
        rng = F32(hi - lo)
        return (np.zeros_like(x) if rng == 0 else (x - lo) / rng), lo, hi

    for b in range(B):
        s = int(starts[i0 + b])
        w2[b], scale[b, 0], scale[b, 1] = norm(ms2_run[s:s + W])
        w1[b], scale[b, 2], scale[b, 3] = norm(ms1_run[s:s + W])
    assert w2.dtype == w1.dtype == scale.dtype == F32
    return w2, w1, scale


def new_state(RT_total, MZ):
    """(mean, m2, wsum), zeroed as the caller of dq_run_stitch must"""
    return np.zeros((RT_total, MZ), F32), np.zeros((RT_total, MZ), F32), np.zeros(RT_total, F32)


def run_stitch_ref(state, pred, scale, taper, W, step, i0=0):
    """dq_run_stitch on ``state`` = (mean, m2, wsum), in place: the windows i0 .. i0 + len(pred) - 1 in ascending order, every operation
    rounded to fp32 on its own.  (A window's scans are distinct elements, so window by window is per element in ascending i.)"""
    mean, m2, wsum = state
    pred, scale, taper = np.asarray(pred, dtype=F32), np.asarray(scale, dtype=F32), np.asarray(taper, dtype=F32)
    starts = starts_of(len(mean), W, step)
    for b in range(len(pred)):
        s = int(starts[i0 + b])
        rng = F32(scale[b, 1] - scale[b, 0])
        for k in range(W):
            r = s + k
            v = pred[b, k] * rng
            w = taper[k]
            wn = F32(wsum[r] + w)
            d = v - mean[r]
            mean[r] = mean[r] + F32(w / wn) * d
            m2[r] = m2[r] + (w * d) * (v - mean[r])
            wsum[r] = wn
    assert mean.dtype == m2.dtype == wsum.dtype == F32
    return state


def tapers(W):
    from dquartic.utils.run_tiles import taper_table

    return {"hann": taper_table("hann", W), "uniform": taper_table("uniform", W)}


def groupings(n):
    """the windows 0 .. n - 1 as lists of (i0, B): all at once, one by one, in fours with a remainder"""
    return {"all": [(0, n)], "ones": [(i, 1) for i in range(n)], "fours": [(i, min(4, n - i)) for i in range(0, n, 4)]}


# ---------------------------------------------------------------------------------------------------------------- the window rule
def test_window_rule_against_brute_force():
    from dquartic import _native as N

    lib = N.lib()
    for RT_total in range(1, 41):
        for W in range(1, RT_total + 1):
            for step in range(1, W + 1):
                s = starts_of(RT_total, W, step)
                brute = []  # slide by step until a window reaches the last scan; that one is pulled back onto it
                i = 0
                while i * step + W < RT_total:
                    brute.append(i * step)
                    i += 1
                brute.append(RT_total - W)
                assert s.dtype == np.int64 and s.tolist() == brute, (RT_total, W, step)
                assert lib.dq_run_window_count(RT_total, W, step) == len(s)
                covered = np.zeros(RT_total, dtype=int)
                for a in s:
                    covered[a:a + W] += 1
                assert covered.min() >= 1  # every scan is covered
                assert (np.diff(s) > 0).all() and (np.diff(s) <= step).all()  # strictly increasing, never further apart than a step
                assert s[0] == 0 and s[-1] + W == RT_total  # the last window ends on the last scan
    for bad in ((10, 4, 0), (10, 4, 5), (10, 11, 3), (0, 0, 0), (10, 0, 0), (10, 4, -1)):
        assert lib.dq_run_window_count(*bad) == 0
        with pytest.raises(ValueError, match="1 <= step <= W <= RT_total"):
            starts_of(*bad)
    assert lib.dq_run_window_count(2 ** 31 - 1, 1, 1) == 2 ** 31 - 1  # no 32-bit intermediate


def test_taper_tables():
    from dquartic.utils.run_tiles import taper_table

    for W in (1, 2, 5, 34, 400):
        h = taper_table("hann", W)
        assert h.dtype == F32 and h.shape == (W,) and (h > 0).all() and h.max() <= 1
        assert np.abs(h.astype(np.float64) - np.sin(np.pi * (np.arange(W) + 1.0) / (W + 1)) ** 2).max() <= U  # float64, then one cast
        assert np.allclose(h, h[::-1], rtol=0, atol=2 * U)  # symmetric
        assert np.array_equal(taper_table("uniform", W), np.ones(W, F32))
    assert taper_table("hann", 1)[0] == 1
    assert np.array_equal(taper_table([1, 2.5, 3], 3), np.array([1, 2.5, 3], F32))
    for bad, word in (("hamming", "Unknown taper"), ([1, 2], "positive numbers"), ([1, 0, 1], "positive finite"), ([1, -1, 1], "positive finite"),
                      ([1, float("nan"), 1], "positive finite"), ([1, float("inf"), 1], "positive finite"), ([1, 1e-50, 1], "positive finite")):
        with pytest.raises(ValueError, match=word):
            taper_table(bad, 3)


# ---------------------------------------------------------------------------------------------------------------- the C entries
def test_native_refusals_and_scratch_size():
    from dquartic import _native as N

    lib = N.lib()
    d = ctypes.c_void_p(4096)

    def windows(ms2=d, ms1=d, RT_total=24, MZ=8, M1=1, W=8, step=3, i0=0, B=7, w2=d, w1=d, scale=d, scratch=d, nbytes=1 << 20):
        return lib.dq_run_windows(ms2, ms1, RT_total, MZ, M1, W, step, i0, B, w2, w1, scale, scratch, nbytes, None)

    def stitch(pred=d, scale=d, taper=d, RT_total=24, MZ=8, W=8, step=3, i0=0, B=7, mean=d, m2=d, wsum=d):
        return lib.dq_run_stitch(pred, scale, taper, RT_total, MZ, W, step, i0, B, mean, m2, wsum, None)

    assert lib.dq_run_window_count(24, 8, 3) == 7
    rule = [(dict(step=0), b"1 <= step <= W <= RT_total"), (dict(step=9), b"1 <= step <= W <= RT_total"),
            (dict(W=25, step=3), b"1 <= step <= W <= RT_total"), (dict(W=0, step=0), b"1 <= step <= W <= RT_total"),
            (dict(RT_total=0), b"1 <= step <= W <= RT_total"), (dict(step=-3), b"1 <= step <= W <= RT_total"),
            (dict(i0=-1), b"must lie in 0 .. n - 1"), (dict(B=0), b"must lie in 0 .. n - 1"), (dict(B=-2), b"must lie in 0 .. n - 1"),
            (dict(B=8), b"must lie in 0 .. n - 1"), (dict(i0=7, B=1), b"must lie in 0 .. n - 1"), (dict(i0=3, B=5), b"must lie in 0 .. n - 1"),
            (dict(i0=2 ** 62, B=1), b"must lie in 0 .. n - 1"), (dict(i0=2 ** 63 - 1, B=1), b"must lie in 0 .. n - 1"),
            (dict(i0=2 ** 63 - 7, B=7), b"must lie in 0 .. n - 1"),
            (dict(RT_total=70000, W=1, step=1, B=65536), b"at most 65535 windows")]
    cases_w = ([(dict([(k, None)]), b"null argument") for k in ("ms2", "ms1", "w2", "w1", "scale", "scratch")]
               + [(dict(MZ=0), b"MZ and M1 must be >= 1"), (dict(M1=0), b"MZ and M1 must be >= 1"), (dict(MZ=-4), b"MZ and M1 must be >= 1")]
               + rule + [(dict(nbytes=lib.dq_run_windows_scratch_bytes(7) - 1), b"scratch too small"), (dict(nbytes=0), b"scratch too small")])
    for kw, word in cases_w:
        assert windows(**kw) != 0, kw
        err = lib.dq_last_error()
        assert word in err and b"dq_run_windows" in err, (kw, err)
    cases_s = ([(dict([(k, None)]), b"null argument") for k in ("pred", "scale", "taper", "mean", "m2", "wsum")]
               + [(dict(MZ=0), b"MZ must be >= 1")] + rule)
    for kw, word in cases_s:
        assert stitch(**kw) != 0, kw
        err = lib.dq_last_error()
        assert word in err and b"dq_run_stitch" in err, (kw, err)
    # the order of the refusals: the earlier one speaks
    assert windows(ms2=None, MZ=0) != 0 and b"null argument" in lib.dq_last_error()
    assert windows(MZ=0, step=0) != 0 and b"MZ and M1" in lib.dq_last_error()
    assert windows(step=0, B=0) != 0 and b"1 <= step" in lib.dq_last_error()
    assert windows(B=8, nbytes=0) != 0 and b"must lie in" in lib.dq_last_error()
    assert stitch(mean=None, MZ=0) != 0 and b"null argument" in lib.dq_last_error()
    assert stitch(MZ=0, W=30) != 0 and b"MZ must be" in lib.dq_last_error()
    assert stitch(W=30, i0=-1) != 0 and b"1 <= step" in lib.dq_last_error()
    # the last window alone, and the last of a range, are accepted by the rule: they fail only at the scratch size here
    assert windows(i0=6, B=1, nbytes=0) != 0 and b"scratch too small" in lib.dq_last_error()
    # (min, max) per chunk and one pair for MS1, per window: 8 chunks -> 72 bytes a window; 0 for what the call refuses
    assert lib.dq_run_windows_scratch_bytes(1) == 72 and lib.dq_run_windows_scratch_bytes(32) == 32 * 72
    assert lib.dq_run_windows_scratch_bytes(65535) == 65535 * 72
    assert lib.dq_run_windows_scratch_bytes(0) == 0 and lib.dq_run_windows_scratch_bytes(-3) == 0 and lib.dq_run_windows_scratch_bytes(65536) == 0


# ---------------------------------------------------------------------------------------------------------------- the rules' own properties
SHAPES = [(8, 8, 8), (24, 8, 3), (23, 8, 3), (16, 8, 8), (12, 4, 1), (11, 4, 3)]


def test_windows_transcription():
    rng = np.random.default_rng(0)
    ms2, ms1 = (rng.random((24, 6), dtype=F32) * 900 + 3), rng.random((24, 3), dtype=F32) * 50
    ms2[:8], ms1[:8] = 0, 0  # window 0: an empty stretch
    ms2[16:] = 7.5  # the last window: constant at a non-zero value
    w2, w1, scale = run_windows_ref(ms2, ms1, 8, 3)
    assert w2.shape == (7, 8, 6) and w1.shape == (7, 8, 3) and scale.shape == (7, 4)
    assert (w2[0] == 0).all() and (w1[0] == 0).all() and scale[0].tolist() == [0, 0, 0, 0]
    assert (w2[6] == 0).all() and scale[6, 0] == scale[6, 1] == F32(7.5) and w1[6].min() == 0 and w1[6].max() == 1
    for b in range(1, 6):
        assert w2[b].min() == 0 and w2[b].max() == 1 and w1[b].min() == 0 and w1[b].max() == 1
        s = 3 * b
        assert scale[b].tolist() == [ms2[s:s + 8].min(), ms2[s:s + 8].max(), ms1[s:s + 8].min(), ms1[s:s + 8].max()]
        assert np.array_equal(w2[b], (ms2[s:s + 8] - scale[b, 0]) / (scale[b, 1] - scale[b, 0]))
    assert not np.isnan(w2).any() and not np.isnan(w1).any()
    # a range of windows is those rows of the whole; a 1-D MS1 is one channel
    p2, p1, ps = run_windows_ref(ms2, ms1, 8, 3, i0=2, B=3)
    assert np.array_equal(p2, w2[2:5]) and np.array_equal(p1, w1[2:5]) and np.array_equal(ps, scale[2:5])
    assert np.array_equal(run_windows_ref(ms2, ms1[:, 0], 8, 3)[1], run_windows_ref(ms2, ms1[:, :1], 8, 3)[1])


@pytest.mark.parametrize("RT_total,W,step", SHAPES)
def test_constant_prediction_is_returned_exactly(RT_total, W, step):
    n = len(starts_of(RT_total, W, step))
    scale = np.tile(np.array([0, 1, 0, 1], F32), (n, 1))
    for name, tp in tapers(W).items():
        for c in (F32(0.3), F32(-17.25), F32(1e-30)):
            mean, m2, wsum = run_stitch_ref(new_state(RT_total, 5), np.full((n, W, 5), c, F32), scale, tp, W, step)
            assert (mean == c).all() and (m2 == 0).all(), (name, c)


@pytest.mark.parametrize("RT_total,W,step", SHAPES)
def test_coverage_is_the_taper_sums_and_any_grouping_gives_the_same_bits(RT_total, W, step):
    rng = np.random.default_rng(RT_total * 100 + step)
    starts = starts_of(RT_total, W, step)
    n, MZ = len(starts), 6
    pred = rng.standard_normal((n, W, MZ)).astype(F32)
    scale = np.stack([rng.random(n), 1 + rng.random(n) * 900, rng.random(n), 1 + rng.random(n)], axis=1).astype(F32)
    for name, tp in tapers(W).items():
        got = {}
        for g, calls in groupings(n).items():
            st = new_state(RT_total, MZ)
            for i0, B in calls:
                run_stitch_ref(st, pred[i0:i0 + B], scale[i0:i0 + B], tp, W, step, i0)
            got[g] = st
        for g in ("ones", "fours"):
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[g], got["all"])), (name, g)
        mean, m2, wsum = got["all"]
        want = np.zeros(RT_total, F32)  # the fp32 sum of the covering windows' weights, in window order
        exact = np.zeros(RT_total)
        count = np.zeros(RT_total, dtype=int)
        for s in starts:
            want[s:s + W] = want[s:s + W] + tp
            exact[s:s + W] += tp.astype(np.float64)
            count[s:s + W] += 1
        assert np.array_equal(wsum, want) and np.abs(wsum - exact).max() <= count.max() * U * exact.max()
        if name == "uniform":
            assert np.array_equal(wsum, count.astype(F32))  # the number of windows on a scan
        assert (m2[count == 1] == 0).all() and (m2 >= 0).all()  # one window: no disagreement
        # the weighted mean and variance of the covering windows' values, in float64
        v = pred.astype(np.float64) * (scale[:, 1] - scale[:, 0]).astype(np.float64)[:, None, None]
        num, sq = np.zeros((RT_total, MZ)), np.zeros((RT_total, MZ))
        for i, s in enumerate(starts):
            num[s:s + W] += tp[:, None] * v[i]
        mu = num / exact[:, None]
        for i, s in enumerate(starts):
            sq[s:s + W] += tp[:, None] * (v[i] - mu[s:s + W]) ** 2
        # |v| <= R, so |d| and |v - mean| <= 2 R =: D.  A step of the mean makes four roundings of quantities <= D (d, w / wn, the product,
        # the sum), v itself one: |mean - mu| <= (1 + 4 K) u D at K covering windows.  A term (w d) (v - mean) of m2 is <= w D^2; it carries
        # four roundings of its own and twice the error of the mean relative to D: (6 + 8 K) u w D^2, and w / wsum <= 1 for each of K terms.
        K, D = count.max(), 2 * np.abs(v).max()
        assert np.abs(mean - mu).max() <= (1 + 4 * K) * U * D
        assert np.abs(m2 / wsum[:, None] - sq / exact[:, None]).max() <= K * (6 + 8 * K) * U * D ** 2


@pytest.mark.parametrize("RT_total,W,step", SHAPES)
def test_identity_sampler_round_trip(RT_total, W, step):
    """pred = ms2_win, the uniform taper: mean is run - lo_i where one window covers the scan, and elsewhere the mean of run - lo_i over the
    covering windows.  Bound: n_i = fl(fl(x - lo) / rng) and v = fl(n_i rng) carry three roundings, |v - (x - lo)| <= 3 u (1 + 2u) (x - lo)
    <= 3.01 u R with R the largest window range and u = 2^-24.  The first window on a scan enters exactly (w / wn = 1, d = v - 0); each
    further one adds four roundings of quantities bounded by R (d, w / wn, their product, the sum): 4 u R (1 + small).  So
    |mean - exact| <= (3.01 + 4.01 (K - 1)) u R at K covering windows; where K = 1 the bound is 3.01 u (x - lo) element by element."""
    rng = np.random.default_rng(7)
    MZ = 6
    run = (rng.lognormal(0, 1, (RT_total, MZ)) * 50).astype(F32)
    ms1 = rng.random(RT_total, dtype=F32)
    w2, _, scale = run_windows_ref(run, ms1, W, step)
    starts = starts_of(RT_total, W, step)
    mean, m2, wsum = run_stitch_ref(new_state(RT_total, MZ), w2, scale, tapers(W)["uniform"], W, step)
    count = np.zeros(RT_total, dtype=int)
    exact = np.zeros((RT_total, MZ))
    for i, s in enumerate(starts):
        count[s:s + W] += 1
        exact[s:s + W] += run[s:s + W].astype(np.float64) - float(scale[i, 0])
    exact /= count[:, None]
    R = float((scale[:, 1] - scale[:, 0]).max())
    one = count == 1
    assert (np.abs(mean[one] - exact[one]) <= 3.01 * U * exact[one]).all()
    bound = (3.01 + 4.01 * (count - 1)) * U * R
    err = np.abs(mean - exact)
    assert (err <= bound[:, None]).all(), float((err / bound[:, None]).max())
    assert np.array_equal(wsum, count.astype(F32))


# ---------------------------------------------------------------------------------------------------------------- surface
def test_deconvolve_run_argument_checks():
    """raised on the host: the tensors are host tensors, nothing reaches the device"""
    dm = _dm()
    ms2, ms1 = torch.zeros(20, 8), torch.zeros(20)
    for kw, exc, word in ((dict(ms2_run=torch.zeros(2, 20, 8)), ValueError, r"ms2_run must be \(RT_total, MZ\)"),
                          (dict(ms2_run=ms2.numpy()), TypeError, "torch tensors"),
                          (dict(ms1_run=torch.zeros(19)), ValueError, "ms1_run must be"),
                          (dict(ms1_run=torch.zeros(20, 1, 1)), ValueError, "ms1_run must be"),
                          (dict(ms1_run=torch.zeros(20, 3)), ValueError, "attn_cond_channels=1"),
                          (dict(window=None), ValueError, "window .* must be given"),
                          (dict(window=21), ValueError, "1 <= step <= W <= RT_total"),
                          (dict(step=0), ValueError, "1 <= step <= W <= RT_total"),
                          (dict(step=9), ValueError, "1 <= step <= W <= RT_total"),
                          (dict(batch_size=0), ValueError, "batch_size must be >= 1"),
                          (dict(taper="hamming"), ValueError, "Unknown taper"),
                          (dict(taper=[1.0] * 7), ValueError, "positive numbers"),
                          (dict(taper=[0.0] * 8), ValueError, "positive finite"),
                          (dict(n_draws=2), TypeError, "unknown option"),
                          (dict(window_ids=[0]), TypeError, "unknown option")):
        args = {"ms2_run": ms2, "ms1_run": ms1, "window": 8, "step": 5, **kw}
        with pytest.raises(exc, match=word):
            dm.deconvolve_run(**args)
    # everything in order, host tensors: the native-only refusal, in the words of the other native-only entries
    with pytest.raises(NotImplementedError, match=r"runs in the native library only \(device tensors\)"):
        dm.deconvolve_run(ms2, ms1, window=8, num_steps=4, seed=1)
    with pytest.raises(NotImplementedError, match="native library only"):
        dm.deconvolve_run(ms2, ms1[:, None], window=8, taper=np.arange(1, 9), batch_size=3, id_offset=5, eta=1.0, use_ema=False)


def test_cli_surface(tmp_path):
    from click.testing import CliRunner

    from dquartic.cli import cli

    res = CliRunner().invoke(cli, ["--help"])
    assert res.exit_code == 0 and "deconvolve" in res.output and "evaluate" in res.output
    res = CliRunner().invoke(cli, ["deconvolve", "--help"])
    assert res.exit_code == 0
    for opt in ("--checkpoint", "--ms2", "--ms1", "--out", "--window", "--step", "--taper", "--batch-size", "--num-steps", "--eta", "--sampler",
                "--clip-x0", "--guidance-scale", "--null-ms1", "--seed", "--use-ema"):
        assert opt in res.output, opt
    cfg, ck = str(tmp_path / "c.json"), str(tmp_path / "x.ckpt")
    assert CliRunner().invoke(cli, ["generate-config", cfg]).exit_code == 0
    open(ck, "wb").close()
    p2, p1, out = str(tmp_path / "ms2.npy"), str(tmp_path / "ms1.npy"), str(tmp_path / "o.npz")
    np.save(p2, np.zeros((20, 8), F32))
    np.save(p1, np.zeros(20, F32))
    # (the group chains its commands: a command's options come before its CONFIG argument, as the other commands are called)
    base = ["deconvolve", "--checkpoint", ck, "--ms2", p2, "--ms1", p1, "--out", out]
    for args, word in ((base, "--window"), (base[:-2] + ["--window", "8"], "--out"),
                       (["deconvolve", "--checkpoint", str(tmp_path / "none"), "--ms2", p2, "--ms1", p1, "--out", out, "--window", "8"], "none"),
                       (base + ["--window", "8", "--taper", "hamming"], "hamming"),
                       (base + ["--window", "21"], "1 <= --step <= --window <= RT_total"),
                       (base + ["--window", "8", "--step", "9"], "1 <= --step <= --window <= RT_total"),
                       (base + ["--window", "8", "--step", "0"], "1 <= --step <= --window <= RT_total")):
        res = CliRunner().invoke(cli, args + [cfg])
        assert res.exit_code != 0 and word in res.output, (args, res.output)
    np.save(p1, np.zeros(19, F32))
    res = CliRunner().invoke(cli, base + ["--window", "8", cfg])
    assert res.exit_code != 0 and "--ms1: expected (RT_total,)" in res.output
    np.save(p2, np.zeros((2, 3, 20, 8), F32))
    res = CliRunner().invoke(cli, base + ["--window", "8", cfg])
    assert res.exit_code != 0 and "--ms2: expected" in res.output
    np.save(p2, np.zeros((2, 20, 8), F32))
    np.save(p1, np.zeros((3, 20), F32))
    res = CliRunner().invoke(cli, base + ["--window", "8", cfg])
    assert res.exit_code != 0 and "--ms1: expected (R, RT_total)" in res.output
