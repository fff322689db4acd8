"""Times ``deconvolve_run`` on two whole chromatograms with the benchmark's network, batch 32 and 50 sampling steps:

  long_windows    2,000 scans x 64 m/z at W = 400, step = 100: 17 windows, one batch
  reference_cut   600 scans x 64 m/z at W = 34, step = 5 (the reference's --window-size / --sliding-step): 115 windows, four batches

Per workload, after one warm-up call of everything that is timed:

  whole call      ``deconvolve_run`` between a device synchronise and the next, --repeats times: windows per second, median and spread
  sample only     the same batches through ``sample`` alone on windows formed beforehand, alternating with the whole call: the share of
                  the whole call spent outside ``sample`` is 1 - sample_only / whole_call
  native pair     ``dq_run_windows`` + ``dq_run_stitch`` for one batch (the first min(32, n) windows), timing windows of back-to-back calls
                  between two device events, each at least --window seconds long
  torch pair      the same work as the torch composition a user would write on the same device: ``unfold`` + index select, ``amin`` /
                  ``amax``, the normalising arithmetic, and three ``index_add_`` of w, w v and w v^2 (the sums-of-squares form of the
                  blend); alternating with the native pair, window after window, so that a drift of the machine hits both alike

and the algorithmic bytes of the native pair (every window read once and written once, every prediction read once, the state of the
covered scans read and written once) with the rate they imply.

    python tools/time_deconvolve.py --out profiles/deconvolve.json

Needs the GPU; it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd"))

from dquartic import _native as N  # noqa: E402
from dquartic.utils.run_tiles import run_window_starts, taper_table  # noqa: E402

WORKLOADS = {"long_windows": (2000, 64, 400, 100), "reference_cut": (600, 64, 34, 5)}  # RT_total, MZ, W, step


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters  # seconds per call


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(v, scale=1.0):
    return {"median": scale * statistics.median(v), "min_max": [scale * min(v), scale * max(v)]}


def build_dm(MZ):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 tfer_dim_mult=620, downsample_dim=MZ, simple=True).cuda()
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=1000, beta_schedule_type="cosine", pred_type="eps", auto_normalize=True,
                            device="cuda")
    net.eval()
    return dm


def time_pair(a, run2, run1, W, step, B):
    """the native pair and the torch composition for windows 0 .. B - 1, alternating"""
    RT_total, MZ = run2.shape
    lib, st = N.lib(), N.stream_ptr()
    starts = torch.from_numpy(run_window_starts(RT_total, W, step)[:B]).cuda()
    taper = torch.from_numpy(taper_table("hann", W)).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    pred = torch.rand(B, W, MZ, device="cuda", generator=g)
    new = lambda *s: torch.zeros(s, device="cuda")
    win2, win1, scale = new(B, W, MZ), new(B, W, 1), new(B, 4)
    mean, m2, wsum = new(RT_total, MZ), new(RT_total, MZ), new(RT_total)
    scratch = new(lib.dq_run_windows_scratch_bytes(B) // 4)
    sw, swv, swv2 = new(RT_total), new(RT_total, MZ), new(RT_total, MZ)
    rows = (starts[:, None] + torch.arange(W, device="cuda")[None, :]).reshape(-1)

    def native():
        N.check(lib.dq_run_windows(N.ptr(run2), N.ptr(run1), RT_total, MZ, 1, W, step, 0, B, N.ptr(win2), N.ptr(win1), N.ptr(scale),
                                   N.ptr(scratch), scratch.numel() * 4, st), "dq_run_windows")
        N.check(lib.dq_run_stitch(N.ptr(pred), N.ptr(scale), N.ptr(taper), RT_total, MZ, W, step, 0, B, N.ptr(mean), N.ptr(m2), N.ptr(wsum),
                                  st), "dq_run_stitch")

    def norm(x):
        lo, hi = x.amin(dim=(1, 2), keepdim=True), x.amax(dim=(1, 2), keepdim=True)
        rng = hi - lo
        return torch.where(rng == 0, torch.zeros_like(x), (x - lo) / rng), rng

    def composed():
        w2 = run2.unfold(0, W, 1)[starts].permute(0, 2, 1)  # (B, W, MZ)
        w1 = run1.unfold(0, W, 1)[starts].permute(0, 2, 1)
        n2, rng = norm(w2)
        n1, _ = norm(w1)
        v = (pred * rng).reshape(-1, MZ)
        w = taper.repeat(B)
        sw.index_add_(0, rows, w)
        swv.index_add_(0, rows, v * w[:, None])
        swv2.index_add_(0, rows, v * v * w[:, None])
        return n2, n1

    paths = {"native": native, "torch": composed}
    iters, times = {}, {k: [] for k in paths}
    for k, fn in paths.items():
        window(fn, 3)
        iters[k] = max(1, int(a.window / window(fn, 20)) + 1)
    for _ in range(a.windows):
        for k, fn in paths.items():
            times[k].append(window(fn, iters[k]))
    covered = int(starts[-1]) + W  # the scans windows 0 .. B - 1 cover
    bytes_ = 4 * (B * (2 * W * MZ + 2 * W) + B * W * MZ + 4 * covered * MZ + 2 * covered)
    out = {"windows_in_batch": B, "iters_per_window": iters, "algorithmic_bytes": bytes_,
           "bytes_per_window_each_way": 2 * W * MZ * 4}
    for k, v in times.items():
        out[k] = {"us": summary(v, 1e6)}
    out["native"]["GBps"] = summary([bytes_ / t for t in times["native"]], 1e-9)
    out["native_over_torch"] = out["native"]["us"]["median"] / out["torch"]["us"]["median"]
    out["native_spread"] = out["native"]["us"]["min_max"][1] / out["native"]["us"]["min_max"][0]
    out["torch_spread"] = out["torch"]["us"]["min_max"][1] / out["torch"]["us"]["min_max"][0]
    return out


def time_workload(a, name):
    RT_total, MZ, W, step = WORKLOADS[name]
    rng = np.random.default_rng(0)
    run2 = torch.from_numpy((rng.lognormal(0, 1, (RT_total, MZ)) * 50).astype(np.float32)).cuda()
    run1 = torch.from_numpy((rng.lognormal(0, 1, (RT_total, 1)) * 500).astype(np.float32)).cuda()
    dm = build_dm(MZ)
    n = len(run_window_starts(RT_total, W, step))
    kw = dict(window=W, step=step, batch_size=a.batch, num_steps=a.steps, seed=7)
    res = {}

    def whole():
        res["out"] = dm.deconvolve_run(run2, run1, **kw)

    # the windows of every batch, formed beforehand, for the sample-only loop
    lib = N.lib()
    batches = []
    for i0 in range(0, n, a.batch):
        B = min(a.batch, n - i0)
        c2, c1, sc = (torch.empty(s, device="cuda") for s in ((B, W, MZ), (B, W, 1), (B, 4)))
        scratch = torch.empty(lib.dq_run_windows_scratch_bytes(B) // 4, device="cuda")
        N.check(lib.dq_run_windows(N.ptr(run2), N.ptr(run1), RT_total, MZ, 1, W, step, i0, B, N.ptr(c2), N.ptr(c1), N.ptr(sc), N.ptr(scratch),
                                   scratch.numel() * 4, N.stream_ptr()), "dq_run_windows")
        batches.append((c2, c1, torch.arange(i0, i0 + B, dtype=torch.int64, device="cuda")))

    def sample_only():
        with torch.no_grad():
            for c2, c1, ids in batches:
                dm.sample(None, ms2_cond=c2, ms1_cond=c1, window_ids=ids, num_steps=a.steps, seed=7)

    wall(whole)
    wall(sample_only)
    assert bool(torch.isfinite(res["out"]["pred"]).all()) and res["out"]["n_windows"] == n
    t_whole, t_sample = [], []
    for _ in range(a.repeats):
        t_whole.append(wall(whole))
        t_sample.append(wall(sample_only))
    entry = {"RT_total": RT_total, "MZ": MZ, "W": W, "step": step, "n_windows": n, "batches": len(batches),
             "whole_call_s": summary(t_whole), "sample_only_s": summary(t_sample),
             "windows_per_s": summary([n / t for t in t_whole]),
             "outside_sample_share": summary([1.0 - s / w for s, w in zip(t_sample, t_whole)]),
             "pair": time_pair(a, run2, run1, W, step, min(a.batch, n))}
    entry["pair_share_of_whole_call"] = entry["pair"]["native"]["us"]["median"] * 1e-6 * len(batches) / entry["whole_call_s"]["median"]
    print(json.dumps({name: {"windows_per_s": round(entry["windows_per_s"]["median"], 1),
                             "outside_sample_share": round(entry["outside_sample_share"]["median"], 4),
                             "native_us": round(entry["pair"]["native"]["us"]["median"], 2),
                             "torch_us": round(entry["pair"]["torch"]["us"]["median"], 2),
                             "native_over_torch": round(entry["pair"]["native_over_torch"], 3)}}), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "deconvolve.json"))
    ap.add_argument("--repeats", type=int, default=5, help="timed whole calls per workload")
    ap.add_argument("--windows", type=int, default=7, help="timing windows per path of the pair")
    ap.add_argument("--window", type=float, default=0.3, help="least length of a timing window of the pair in seconds")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_deconvolve needs the GPU")
    res = {"config": {"batch": a.batch, "steps": a.steps, "repeats": a.repeats, "windows": a.windows, "window_s": a.window},
           "device": torch.cuda.get_device_name(0), "build_id": N.build_id(), "workloads": {}}
    for name in a.workloads:
        res["workloads"][name] = time_workload(a, name)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
