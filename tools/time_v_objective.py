"""Times the v objective (pred_type="v_prediction") beside the eps objective on the default U-Net at the bench shape
(400 x 64 windows): the fused train step at batch 32 (the training head carries the loss for both), the v train step with the head loss
switched off (the un-fused path: final_conv, k_mse_fwd_bwd<MseV> and final_conv's backward data path as launches of their own), and the default
sampling step at batch 512.  It also counts the kernel launches of one train step and of one sampling step for both objectives.

The un-fused path exists in the development build only (csrc/dq_dev.h, `make dev`: DQ_NO_HEAD_LOSS=1, read once per process), so it is timed
in a fresh child process on build/dev/libdq_hip_dev.so -- next to the same build's fused step, so that the pair shares a library.

Timing: all paths of a process are warmed up, then timed in turn, window after window, so that a drift of the machine hits them alike.  A
window is `iters` back-to-back calls between two device events; `iters` is chosen from the warm-up so that a window lasts at least --window
seconds.  Reported: the median and (min, max) over the windows.  Launch counts: kernel events torch.profiler records for one eager call (the
sampling step: the difference between a 3-step and a 2-step call, which leaves the loop's prologue and epilogue out).

    python tools/time_v_objective.py --out profiles/v_objective.json

Needs the GPU; it does not fall back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd")
sys.path.insert(0, PKG)

from dquartic import _native as N  # noqa: E402
from dquartic.model.model import DDIMDiffusionModel  # noqa: E402
from dquartic.model.unet1d import UNet1d  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters  # seconds per call


def time_paths(paths, windows, least):
    iters, times = {}, {k: [] for k in paths}
    for k, fn in paths.items():
        fn()
        window(fn, 1)
        iters[k] = max(1, int(least / window(fn, 2)) + 1)
    for _ in range(windows):
        for k, fn in paths.items():
            times[k].append(window(fn, iters[k]))
    return {k: {"ms": 1e3 * statistics.median(v), "ms_min_max": [1e3 * min(v), 1e3 * max(v)], "iters_per_window": iters[k]} for k, v in times.items()}


def count_launches(fn):
    """kernel events of one call (None where the profiler records no device events)"""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as err:  # (reported, not hidden: the count is then missing from the result)
        print(f"launch count unavailable: {err!r}", file=sys.stderr)
        return None


def models(MZ):
    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True).cuda()
    return {p: DDIMDiffusionModel(model_class=net, pred_type=p, device="cuda") for p in ("eps", "v_prediction")}, net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "v_objective.json"))
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--sample-batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10, help="sampling steps per timed call")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--shape", type=int, nargs=2, default=[400, 64], metavar=("RT", "MZ"))
    ap.add_argument("--child", action="store_true", help="(internal) the train steps of this process's library only, as one JSON line")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_v_objective needs the GPU")
    RT, MZ = a.shape
    dms, net = models(MZ)
    B = a.train_batch
    g = torch.Generator().manual_seed(1)
    x0, c2, c1 = torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, generator=g).cuda()
    net.train()
    train = {p: (lambda dm=dm: dm.train_step_fused(x0, c2, c1)) for p, dm in dms.items()}
    if a.child:
        print(json.dumps(time_paths(train, a.windows, a.window)))
        return
    res = {"config": {"RT": RT, "MZ": MZ, "train_batch": B, "sample_batch": a.sample_batch, "sample_steps": a.steps, "windows": a.windows,
                      "window_s": a.window}, "device": torch.cuda.get_device_name(0), "build_id": N.build_id()}
    res["train_step_ms"] = time_paths(train, a.windows, a.window)
    res["launches_per_train_step"] = {p: count_launches(fn) for p, fn in train.items()}
    # the development build in fresh child processes: its fused step, and the same step with the head loss off
    dev_lib = os.path.join(PKG, "build", "dev", "libdq_hip_dev.so")
    for tag, env in (("dev_build_fused", {}), ("dev_build_unfused", {"DQ_NO_HEAD_LOSS": "1"})):
        if not os.path.exists(dev_lib):
            res[tag] = None
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--train-batch", str(B), "--windows", str(a.windows), "--window",
                            str(a.window), "--shape", str(RT), str(MZ)], env={**os.environ, **env, "DQ_HIP_LIB": dev_lib}, capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"child {tag} failed: {r.stderr[-2000:]}")
        res[tag] = {"train_step_ms": json.loads(r.stdout.strip().splitlines()[-1])}
    # sampling
    net.eval()
    Bs = a.sample_batch
    xT, s2, s1 = torch.randn(Bs, RT, MZ, generator=g).cuda(), torch.rand(Bs, RT, MZ, generator=g).cuda(), torch.rand(Bs, RT, generator=g).cuda()
    with torch.no_grad():
        samp = {p: (lambda dm=dm: dm.sample(xT, s2, s1, num_steps=a.steps)) for p, dm in dms.items()}
        t = time_paths(samp, a.windows, a.window)
        res["sampling_step_ms"] = {p: {"ms": v["ms"] / a.steps, "ms_min_max": [x / a.steps for x in v["ms_min_max"]], "iters_per_window": v["iters_per_window"]}
                                   for p, v in t.items()}
        counts = {}
        small = [v[:8].contiguous() for v in (xT, s2, s1)]
        for p, dm in dms.items():
            dm.use_graph = False
            n3, n2 = (count_launches(lambda k=k: dm.sample(*small, num_steps=k)) for k in (3, 2))
            dm.use_graph = True
            counts[p] = None if n3 is None or n2 is None else n3 - n2
        res["launches_per_sampling_step"] = counts
    res["v_over_eps"] = {"train_step": res["train_step_ms"]["v_prediction"]["ms"] / res["train_step_ms"]["eps"]["ms"],
                         "sampling_step": res["sampling_step_ms"]["v_prediction"]["ms"] / res["sampling_step_ms"]["eps"]["ms"]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
