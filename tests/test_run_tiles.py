"""``dq_run_windows`` and ``dq_run_stitch`` (k_run.hip) on the GPU, bit for bit against the numpy fp32 transcription of
their rules (tests/test_run_tiles_host.py).  The run is a slice of a larger allocation whose neighbours are canaries, so a read outside it
lands in allocated memory and shows in the result (NaN in anything normalised from it; the min / max reduction drops a NaN, so the full
call also runs with a large finite canary); every output and the stitch's state sit between NaN canaries, and every call checks that none
of them changed.

Shapes, the smallest that reach every branch: (RT_total, W, step) = (8, 8, 8) one window; (24, 8, 3) a pulled-back tail and up to three
windows on a scan; (23, 8, 3) an exact tail; (16, 8, 8) no overlap; (12, 4, 1) every scan in up to W windows.  MZ = 1 and 6: the scalar
path (6: a window of 48 floats that is a multiple of 4 while its start is not 16-byte aligned); 8: float4 with chunks of two float4;
260: 65 float4 a chunk of the reduction, three blocks of the normalise pass per window and 65 float4 a scan in the stitch (a block of 128
threads, some idle).  M1 = 1, 3.  Four more cases reach the loops' second trips: a scan longer than a block of the stitch (MZ = 262 scalar,
1028 float4: 257) and a window longer than the 64 x 256 elements the normalise pass covers in one stride (8 x 2049 scalar, 8 x 8196 / 4)."""
import numpy as np
import pytest
import torch

from test_mix_batch import same
from test_run_tiles_host import groupings, new_state, run_stitch_ref, run_windows_ref, starts_of, tapers

pytestmark = pytest.mark.gpu

PAD = 64  # floats around every buffer (a multiple of 4: what lies between stays 16-byte aligned)
SHAPES = [(8, 8, 8), (24, 8, 3), (23, 8, 3), (16, 8, 8), (12, 4, 1)]
MZS = [1, 6, 8, 260]
CASES = [s + (mz,) for s in SHAPES for mz in MZS] + [(12, 4, 1, 262), (12, 4, 1, 1028), (8, 8, 8, 2049), (8, 8, 8, 8196)]


def padded(shape, fill=float("nan"), canary=float("nan")):
    """(the whole allocation, the view of `shape` in its middle filled with `fill`)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), canary, device="cuda")
    view = buf[PAD:PAD + n].view(*shape)
    view.fill_(fill)
    return buf, view


def resident(a, canary):
    buf, view = padded(a.shape, canary=canary)
    view.copy_(torch.from_numpy(a))
    return view


def untouched(buf, canary=float("nan")):
    h = torch.cat([buf[:PAD], buf[-PAD:]]).cpu()
    return bool(torch.isnan(h).all()) if np.isnan(canary) else bool((h == canary).all())


def runs(RT_total, W, MZ, M1, seed=0):
    """the inputs of a shape: positive random intensities -- with, where two windows fit side by side, a stretch of all-zero scans that
    holds window 0 and the last window constant at a non-zero value; where they do not, an all-zero and a constant run of their own"""
    rng = np.random.default_rng(seed)
    ms2 = (rng.lognormal(0, 1, (RT_total, MZ)) * 50).astype(np.float32)
    ms1 = (rng.lognormal(0, 1, (RT_total, M1)) * 500).astype(np.float32)
    out = {"random": (ms2, ms1)}
    if RT_total >= 2 * W:
        m2, m1 = ms2.copy(), ms1.copy()
        m2[:W], m1[:W] = 0, 0
        m2[-W:], m1[-W:] = 7.5, 3.25
        out["mixed"] = (m2, m1)
    else:
        out["zero"] = (np.zeros_like(ms2), np.zeros_like(ms1))
        out["constant"] = (np.full_like(ms2, 7.5), np.full_like(ms1, 3.25))
    return out


def dev_windows(d2, d1, W, step, i0, B):
    """one dq_run_windows call on the resident run -> (ms2_win, ms1_win, scale) as numpy"""
    from dquartic import _native as N

    (RT_total, MZ), M1 = d2.shape, d1.shape[1]
    bufs = [padded((B, W, MZ)), padded((B, W, M1)), padded((B, 4)), padded((N.lib().dq_run_windows_scratch_bytes(B) // 4,))]
    N.check(N.lib().dq_run_windows(N.ptr(d2), N.ptr(d1), RT_total, MZ, M1, W, step, i0, B, *(N.ptr(v) for _, v in bufs),
                                   bufs[3][1].numel() * 4, N.stream_ptr()), "dq_run_windows")
    torch.cuda.synchronize()
    assert all(untouched(buf) for buf, _ in bufs)  # nothing outside an output is written
    return tuple(v.cpu().numpy() for _, v in bufs[:3])


def dev_stitch(state, pred, scale, taper, W, step, calls):
    """dq_run_stitch for every (i0, B) of `calls` on the padded device state [(buf, mean), (buf, m2), (buf, wsum)]; pred / scale are the
    device tensors of ALL windows, a call is handed its rows"""
    from dquartic import _native as N

    RT_total, MZ = state[0][1].shape
    for i0, B in calls:
        p, sc = pred[i0:i0 + B].contiguous(), scale[i0:i0 + B].contiguous()
        N.check(N.lib().dq_run_stitch(N.ptr(p), N.ptr(sc), N.ptr(taper), RT_total, MZ, W, step, i0, B, *(N.ptr(v) for _, v in state),
                                      N.stream_ptr()), "dq_run_stitch")
    torch.cuda.synchronize()
    assert all(untouched(buf) for buf, _ in state)
    return tuple(v.cpu().numpy() for _, v in state)


def zero_state(RT_total, MZ):
    return [padded((RT_total, MZ), fill=0.0), padded((RT_total, MZ), fill=0.0), padded((RT_total,), fill=0.0)]


@pytest.mark.parametrize("RT_total,W,step,MZ", CASES)
def test_windows_match_the_transcription(RT_total, W, step, MZ):
    n = len(starts_of(RT_total, W, step))
    for M1 in (1, 3):
        for name, (ms2, ms1) in runs(RT_total, W, MZ, M1).items():
            ref = run_windows_ref(ms2, ms1, W, step)
            assert not any(np.isnan(v).any() for v in ref)
            if name in ("zero", "constant"):
                assert (ref[0] == 0).all() and (ref[1] == 0).all() and (ref[2][:, 0] == ref[2][:, 1]).all()
            if name == "mixed":
                assert (ref[0][0] == 0).all() and (ref[0][-1] == 0).all() and ref[2][-1].tolist() == [7.5, 7.5, 3.25, 3.25]
            d2, d1 = resident(ms2, float("nan")), resident(ms1, float("nan"))
            whole = dev_windows(d2, d1, W, step, 0, n)
            assert all(same(g, r) for g, r in zip(whole, ref)), (M1, name)
            # a read outside the run that the reduction (which drops a NaN) would hide
            big = dev_windows(resident(ms2, 1e30), resident(ms1, 1e30), W, step, 0, n)
            assert all(same(g, r) for g, r in zip(big, ref)), (M1, name)
            # one by one and in fours with a remainder (each a window range i0 > 0 from the second call on): the rows of the whole call
            for g, calls in groupings(n).items():
                for i0, B in calls:
                    part = dev_windows(d2, d1, W, step, i0, B)
                    assert all(same(p, w[i0:i0 + B]) for p, w in zip(part, whole)), (M1, name, g, i0)
            if n >= 3:  # a range inside: neither the first nor the last window
                part = dev_windows(d2, d1, W, step, 1, n - 2)
                assert all(same(p, w[1:n - 1]) for p, w in zip(part, whole)), (M1, name)


@pytest.mark.parametrize("RT_total,W,step,MZ", CASES)
def test_stitch_matches_the_transcription(RT_total, W, step, MZ):
    n = len(starts_of(RT_total, W, step))
    rng = np.random.default_rng(RT_total + MZ)
    pred = rng.standard_normal((n, W, MZ)).astype(np.float32)
    ms2, ms1 = list(runs(RT_total, W, MZ, 1).values())[-1]  # "mixed" where it fits (ranges of 0 among the windows), else a constant run
    scales = [run_windows_ref(ms2, ms1, W, step)[2],
              np.stack([rng.random(n), 1 + rng.random(n) * 900, rng.random(n), 1 + rng.random(n)], axis=1).astype(np.float32)]
    assert (scales[0][:, 0] == scales[0][:, 1]).any()
    pred_d = torch.from_numpy(pred).cuda()
    for scale in scales:
        scale_d = torch.from_numpy(scale).cuda()
        for name, tp in tapers(W).items():
            tp_d = torch.from_numpy(tp).cuda()
            ref = run_stitch_ref(new_state(RT_total, MZ), pred, scale, tp, W, step)
            assert not any(np.isnan(v).any() for v in ref)
            got = {g: dev_stitch(zero_state(RT_total, MZ), pred_d, scale_d, tp_d, W, step, calls) for g, calls in groupings(n).items()}
            for g, st in got.items():
                assert all(same(a, r) for a, r in zip(st, ref)), (name, g)  # so every grouping gives the same bits
            # a window range i0 > 0 on a zeroed state: those windows alone; the scans they do not cover stay as they were
            if n >= 2:
                i0, B = 1, max(1, n - 2)
                part_ref = run_stitch_ref(new_state(RT_total, MZ), pred[i0:i0 + B], scale[i0:i0 + B], tp, W, step, i0)
                part = dev_stitch(zero_state(RT_total, MZ), pred_d, scale_d, tp_d, W, step, [(i0, B)])
                assert all(same(a, r) for a, r in zip(part, part_ref)), name
                # ... and on a state that holds something: the canary value where no window of the call lies
                st = [padded((RT_total, MZ), fill=3.0), padded((RT_total, MZ), fill=3.0), padded((RT_total,), fill=3.0)]
                after = dev_stitch(st, pred_d, scale_d, tp_d, W, step, [(n - 1, 1)])
                s_last = int(starts_of(RT_total, W, step)[-1])
                assert all((a[:s_last] == 3.0).all() for a in after)
