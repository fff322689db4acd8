"""Tiling a whole chromatogram into windows: the window rule and the taper tables, host only.  The kernels of
csrc/k_run.hip recompute the starts from the same rule (``dq_run_window_count`` is its count); nothing here touches a device."""
import math

import numpy as np

TAPERS = ("hann", "uniform")


def run_window_starts(RT_total: int, W: int, step: int) -> np.ndarray:
    """The first scan of every window of a run of ``RT_total`` scans cut into windows of ``W`` scans every ``step`` scans: an int64 array
    of ``n = ceil((RT_total - W) / step) + 1`` strictly increasing starts ``s_i = min(i * step, RT_total - W)``.  The last window is pulled
    back so that it ends on the last scan; every scan lies in at least one window.  Needs ``1 <= step <= W <= RT_total`` (a larger step
    would leave scans uncovered)."""
    RT_total, W, step = int(RT_total), int(W), int(step)
    if not 1 <= step <= W <= RT_total:
        raise ValueError(f"run_window_starts: need 1 <= step <= W <= RT_total, got step={step}, W={W}, RT_total={RT_total}")
    n = -((W - RT_total) // step) + 1
    return np.minimum(np.arange(n, dtype=np.int64) * step, RT_total - W)


def taper_table(taper, W: int) -> np.ndarray:
    """The stitch's weight of scan k of a window as ``W`` positive float32: ``"hann"`` = sin^2(pi (k + 1) / (W + 1)) (strictly positive
    at both ends), computed in float64 and cast; ``"uniform"`` = 1; or a length-``W`` sequence of positive finite numbers, taken as it is."""
    W = int(W)
    if isinstance(taper, str):
        if taper == "hann":
            t = np.array([math.sin(math.pi * (k + 1) / (W + 1)) ** 2 for k in range(W)], dtype=np.float64)
        elif taper == "uniform":
            t = np.ones(W, dtype=np.float64)
        else:
            raise ValueError(f"Unknown taper: {taper!r} (one of {list(TAPERS)}, or {W} positive numbers)")
    else:
        t = np.asarray(taper, dtype=np.float64)
        if t.shape != (W,):
            raise ValueError(f"taper must be one of {list(TAPERS)} or {W} positive numbers (one per scan of a window), got shape {t.shape}")
    t32 = t.astype(np.float32)
    if not (np.isfinite(t32).all() and (t32 > 0).all()):
        raise ValueError("taper: every weight must be a positive finite float32")
    return t32
