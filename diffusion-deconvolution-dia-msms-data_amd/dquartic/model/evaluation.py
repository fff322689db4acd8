"""Held-out evaluation helpers (no reference counterpart: the reference's TODOS list "eval metrics ... separate from
training").  The host side is small and pure -- which timestep a window is evaluated at, how per-window metrics are averaged -- and the
arithmetic on the tensors is native: ``dq_randn`` for the noise, ``dq_recon_metrics`` for the metrics."""
import numpy as np
import torch

from .. import _native as N

GOLDEN_CONJUGATE = (5.0 ** 0.5 - 1.0) / 2.0  # frac(w * this) is a low-discrepancy sequence over the windows w = 0, 1, 2, ...


def stratified_timesteps(window_ids, k: int, n_t: int, num_timesteps: int) -> np.ndarray:
    """Timestep of repeat ``k`` (0 <= k < n_t) of each window: ``floor(((w * phi mod 1) + k) / n_t * T)`` with phi the golden-ratio
    conjugate.  RNG-free: a window is evaluated at the same ``n_t`` timesteps whatever the batch it arrives in, one in each of the
    ``n_t`` equal buckets of [0, T), and the offsets inside the buckets spread evenly over the windows.  int64, in [0, T)."""
    n_t, T, k = int(n_t), int(num_timesteps), int(k)
    if n_t < 1 or T < 1 or not 0 <= k < n_t:
        raise ValueError(f"stratified_timesteps: need n_t >= 1, num_timesteps >= 1 and 0 <= k < n_t, got n_t={n_t}, T={T}, k={k}")
    w = np.asarray(window_ids, dtype=np.int64).reshape(-1)
    frac = np.mod(w.astype(np.float64) * GOLDEN_CONJUGATE, 1.0)
    t = np.floor((frac + k) / n_t * T).astype(np.int64)
    return np.minimum(t, T - 1)  # (frac < 1, so only a rounding of the float64 expression could reach T)


def bucket_edges(n_t: int, num_timesteps: int):
    """The ``n_t + 1`` edges k T / n_t of the timestep buckets: repeat k of a window is evaluated at the integer part of a point of
    [edges[k], edges[k + 1])."""
    return [k * int(num_timesteps) / int(n_t) for k in range(int(n_t) + 1)]


def aggregate_metrics(per_window) -> dict:
    """Means over the windows of an ``(n_windows, 9)`` array of ``dq_recon_metrics`` rows, keyed by ``_native.METRIC_NAMES``.  ``scan_sa``
    and ``xic_r`` are means over a window's valid scans / XICs, so across windows they are weighted by ``scan_count`` / ``xic_count`` (the
    mean over all valid scans / XICs of the set; 0 when there is none); everything else, the counts included, is a plain mean.  float64."""
    a = np.asarray(per_window, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != len(N.METRIC_NAMES) or a.shape[0] < 1:
        raise ValueError(f"aggregate_metrics: need an (n_windows >= 1, {len(N.METRIC_NAMES)}) array, got shape {a.shape}")
    out = {name: float(a[:, i].mean()) for i, name in enumerate(N.METRIC_NAMES)}
    for score, count in (("scan_sa", "scan_count"), ("xic_r", "xic_count")):
        s, c = a[:, N.METRIC_NAMES.index(score)], a[:, N.METRIC_NAMES.index(count)]
        out[score] = float((s * c).sum() / c.sum()) if c.sum() > 0 else 0.0
    return out


TARGET_WEIGHT_EDGES = [0.0, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 1.0]  # buckets of the target's share of its mixture, one octave each above 1/16


def by_target_weight(target_weight, mse_per_window, per_window=None) -> dict:
    """Held-out loss by target abundance: the windows are put into the buckets (edges[i], edges[i + 1]] of ``TARGET_WEIGHT_EDGES`` by their
    target weight w_0 (closed on the right: a single-component window, w_0 = 1, lands in the last one; anything at or below 1/16 in the
    first, anything above 1/2 in the last), and each bucket reports its count ``n`` and the mean of the per-window unweighted MSE, ``mse``.
    With ``per_window`` (the ``(n_windows, 9)`` reconstruction metrics) it also reports ``sa``, the bucket's mean spectral angle.  An empty
    bucket has ``n`` 0 and None for its means.  float64 sums in window order."""
    w = np.asarray(target_weight, dtype=np.float64)
    m = np.asarray(mse_per_window, dtype=np.float64)
    if w.ndim != 1 or m.shape != w.shape:
        raise ValueError(f"by_target_weight: need one weight and one MSE per window, got shapes {w.shape} and {m.shape}")
    which = np.searchsorted(np.asarray(TARGET_WEIGHT_EDGES[1:-1]), w, side="left")  # w <= 1/16 -> 0, ..., w > 1/2 -> 4
    nb = len(TARGET_WEIGHT_EDGES) - 1
    mean = lambda v, k: float(v[which == k].mean()) if (which == k).any() else None
    out = {"edges": list(TARGET_WEIGHT_EDGES), "mse": [mean(m, k) for k in range(nb)], "n": [int((which == k).sum()) for k in range(nb)]}
    if per_window is not None:
        sa = np.asarray(per_window, dtype=np.float64)[:, N.METRIC_NAMES.index("sa")]
        out["sa"] = [mean(sa, k) for k in range(nb)]
    return out


def window_noise(seed_dev: torch.Tensor, window_ids_dev: torch.Tensor, draw: int, shape) -> torch.Tensor:
    """``dq_randn``: standard normals of ``shape`` (B, ...) keyed by (seed, window id, element, draw index): a window's noise is the same in
    any batch."""
    out = torch.empty(tuple(shape), dtype=torch.float32, device=window_ids_dev.device)
    B = int(shape[0])
    N.check(N.lib().dq_randn(N.ptr(out), N.ptr(window_ids_dev), N.ptr(seed_dev), int(draw), B, out[0].numel(), N.stream_ptr()), "dq_randn")
    return out


def recon_metrics(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``dq_recon_metrics``: per-window reconstruction metrics of ``pred`` against ``target`` (both (B, RT, MZ) on the GPU) as a (B, 9)
    float32 device tensor, columns in the order of ``_native.METRIC_NAMES``."""
    if pred.shape != target.shape or pred.dim() != 3:
        raise ValueError(f"recon_metrics: pred and target must both be (B, RT, MZ), got {tuple(pred.shape)} and {tuple(target.shape)}")
    if not pred.is_cuda:
        raise NotImplementedError("recon_metrics runs in the native library only (device tensors)")
    p, t = pred.detach().to(torch.float32).contiguous(), target.detach().to(device=pred.device, dtype=torch.float32).contiguous()
    B, RT, MZ = p.shape
    nbytes = N.lib().dq_recon_metrics_scratch_bytes(B, RT, MZ)
    if nbytes < 0:
        raise RuntimeError("dq_recon_metrics_scratch_bytes failed")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=p.device)
    out = torch.empty((B, len(N.METRIC_NAMES)), dtype=torch.float32, device=p.device)
    N.check(N.lib().dq_recon_metrics(N.ptr(p), N.ptr(t), N.ptr(out), N.ptr(scratch), nbytes, B, RT, MZ, N.stream_ptr()), "dq_recon_metrics")
    return out


# ---- groups: what the P predictions of a group do together
def group_metrics(pred: torch.Tensor, target: torch.Tensor, mix: torch.Tensor, group_size: int):
    """``dq_group_metrics``: ``(cross (G, P, P), group (G, 3))`` float32 device tensors for ``pred`` / ``target`` ``(P*G, RT, MZ)``,
    member-major, and ``mix`` with at least G rows, of which rows 0 .. G-1 are read (a joint batch's ``ms2_cond`` as it is).  ``cross[g, p,
    q]`` is the cosine of member p's prediction against member q's target; ``group`` holds ``_native.GROUP_METRIC_NAMES``."""
    P = int(group_size)
    if pred.shape != target.shape or pred.dim() != 3 or P < 1 or pred.shape[0] % P:
        raise ValueError(f"group_metrics: pred and target must both be (P*G, RT, MZ) with P = {group_size}, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    G, RT, MZ = pred.shape[0] // P, pred.shape[1], pred.shape[2]
    if mix.dim() != 3 or mix.shape[0] < G or tuple(mix.shape[1:]) != (RT, MZ):
        raise ValueError(f"group_metrics: mix must be (>= {G}, {RT}, {MZ}), got {tuple(mix.shape)}")
    if not pred.is_cuda:
        raise NotImplementedError("group_metrics runs in the native library only (device tensors)")
    conv = lambda a: a.detach().to(device=pred.device, dtype=torch.float32).contiguous()
    p, t, m = conv(pred), conv(target), conv(mix)
    nbytes = N.lib().dq_group_metrics_scratch_bytes(G, P, RT, MZ)
    if nbytes < 0:
        raise ValueError(f"group_metrics: group_size must be 1..{N.GROUP_MAX} and the sizes positive, got P = {P}, (G, RT, MZ) = {(G, RT, MZ)}")
    scratch = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=p.device)
    cross = torch.empty((G, P, P), dtype=torch.float32, device=p.device)
    group = torch.empty((G, len(N.GROUP_METRIC_NAMES)), dtype=torch.float32, device=p.device)
    N.check(N.lib().dq_group_metrics(N.ptr(p), N.ptr(t), N.ptr(m), N.ptr(cross), N.ptr(group), N.ptr(scratch), nbytes, G, P, RT, MZ,
                                     N.stream_ptr()), "dq_group_metrics")
    return cross, group


def identification(cross) -> dict:
    """From a ``(groups, P, P)`` array of ``dq_group_metrics``' ``cross``: ``id_acc``, the share of members p whose prediction looks most
    like their own target, ``argmax_q cross[p, q] == p`` with ties going to the lowest q (over groups of one it is 1), and -- for P > 1 --
    ``leak``, the mean over the members of ``max_{q != p} cross[p, q]``: how much a member's prediction looks like another member's
    target.  float64."""
    c = np.asarray(cross, dtype=np.float64)
    if c.ndim != 3 or c.shape[1] != c.shape[2] or c.shape[0] < 1 or c.shape[1] < 1:
        raise ValueError(f"identification: need a (groups >= 1, P, P) array, got shape {c.shape}")
    P = c.shape[1]
    out = {"id_acc": float((np.argmax(c, axis=2) == np.arange(P)[None, :]).mean())}  # (numpy's argmax returns the first maximum)
    if P > 1:
        off = np.where(np.eye(P, dtype=bool)[None], -np.inf, c)
        out["leak"] = float(off.max(axis=2).mean())
    return out


def aggregate_joint(per_window, cross, group, member_weight) -> dict:
    """The scalars of one leg of ``evaluate_joint``: the nine window metrics over all members (``aggregate_metrics``), the means of
    ``excess`` and ``unexplained`` over the groups, ``id_acc`` / ``leak`` (``identification``) and ``sa_by_weight``, the spectral angle by
    the members' own share w_p of their mixture (``by_target_weight``'s buckets).  ``per_window`` (n, 9), ``cross`` (groups, P, P),
    ``group`` (groups, 3), ``member_weight`` (n,), all in the same member-major order."""
    pw, g = np.asarray(per_window, dtype=np.float64), np.asarray(group, dtype=np.float64)
    out = aggregate_metrics(pw)
    out["excess"] = float(g[:, N.GROUP_METRIC_NAMES.index("excess")].mean())
    out["unexplained"] = float(g[:, N.GROUP_METRIC_NAMES.index("unexplained")].mean())
    out.update(identification(cross))
    by = by_target_weight(member_weight, pw[:, N.METRIC_NAMES.index("mse")], pw)
    out["sa_by_weight"] = {"edges": by["edges"], "sa": by["sa"], "n": by["n"]}
    return out
