"""Times the per-window sampler options of the default U-Net at the bench shape (400 x 64 windows, 50 steps,
captured step), interleaved with the plain call they extend:

  plain      sample(..., sampler="ddim", clip_x0=1): guided (guidance_scale=w) at batch B, unguided at batch 2 B -- the same forward size
  rescale    the guided plain call plus guidance_rescale=phi      (2 more launches per step: moments, fold)
  threshold  the plain call plus threshold_quantile=q             (5 more launches per step: four radix passes, fold)
  both       the guided plain call plus both                      (7 more)

at B = 256 (unguided 512) and B = 1 (unguided 2).  All legs are warmed up per shape, then timed in turn, window after window, in one
process, so that a drift of the machine hits them alike.  A timing window is `iters` back-to-back calls between two device events, the
second followed by a synchronise; `iters` is chosen per leg and shape from the warm-up so that a window lasts at least --window seconds.
Reported per leg: the median and the spread (min, max) over the windows as ms per step, and the leg's cost over its plain call.

    python tools/time_adaptive_sample.py --out profiles/adaptive_sample.json
    python tools/time_adaptive_sample.py --plain-only --package <another tree's package directory> --out <file>   # the parent's plain legs

Needs the GPU; it does not fall back."""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "adaptive_sample.json"))
    ap.add_argument("--package", default=os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd"),
                    help="directory that holds the dquartic package and its built library")
    ap.add_argument("--plain-only", action="store_true", help="time the plain legs alone (a tree without the options)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--rescale", type=float, default=0.7)
    ap.add_argument("--quantile", type=float, default=0.995)
    ap.add_argument("--windows", type=int, default=7, help="timing windows per leg and shape")
    ap.add_argument("--window", type=float, default=0.3, help="least length of a timing window in seconds")
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--shape", type=int, nargs=2, default=[400, 64], metavar=("RT", "MZ"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    if not torch.cuda.is_available():
        raise SystemExit("time_adaptive_sample needs the GPU")
    RT, MZ = a.shape
    ns, w, phi, q = a.steps, a.scale, a.rescale, a.quantile
    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True).cuda()
    dm = DDIMDiffusionModel(model_class=net, device="cuda")
    net.eval()
    try:
        build_id = N.build_id()
    except OSError:  # (a --package directory that holds the package and the library without their sources)
        build_id = None
    res = {"config": {"RT": RT, "MZ": MZ, "steps": ns, "sampler": "ddim", "clip_x0": 1.0, "guidance_scale": w, "guidance_rescale": phi,
                      "threshold_quantile": q, "windows": a.windows, "window_s": a.window, "plain_only": a.plain_only},
           # what a step launches behind the network forward: the statistics, the update, the step counter
           "launches_behind_forward": {"plain": 2, "rescale": 4, "threshold": 7, "both": 9},
           "device": torch.cuda.get_device_name(0), "build_id": build_id, "batches": {}}
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        xT, c2, c1 = (torch.randn(2 * B, RT, MZ, generator=g).cuda(), torch.rand(2 * B, RT, MZ, generator=g).cuda(),
                      torch.rand(2 * B, RT, generator=g).cuda())
        x1, a1, b1 = xT[:B].contiguous(), c2[:B].contiguous(), c1[:B].contiguous()
        base = dict(num_steps=ns, sampler="ddim", clip_x0=1.0)

        def leg(guided, **opts):
            if guided:
                return lambda: dm.sample(x1, a1, b1, guidance_scale=w, null_ms1=0.0, **base, **opts)[0]
            return lambda: dm.sample(xT, c2, c1, **base, **opts)[0]

        legs = {"guided_plain": leg(True), "unguided_plain": leg(False)}
        if not a.plain_only:
            legs.update({"guided_rescale": leg(True, guidance_rescale=phi), "guided_threshold": leg(True, threshold_quantile=q),
                         "guided_both": leg(True, guidance_rescale=phi, threshold_quantile=q),
                         "unguided_threshold": leg(False, threshold_quantile=q)})

        def window(fn, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / iters  # seconds per call

        iters, times = {}, {k: [] for k in legs}
        with torch.no_grad():
            for k, fn in legs.items():  # warm-up: workspaces, the captured step, then the size of a window
                fn()
                window(fn, 1)
                iters[k] = max(1, int(a.window / window(fn, 2)) + 1)
            for _ in range(a.windows):
                for k, fn in legs.items():
                    times[k].append(window(fn, iters[k]))
        entry = {"batch": {"guided": B, "unguided": 2 * B}, "iters_per_window": iters}
        for k, v in times.items():
            med = statistics.median(v)
            entry[k] = {"ms_per_step": 1e3 * med / ns, "ms_per_step_min_max": [1e3 * min(v) / ns, 1e3 * max(v) / ns]}
        for k in legs:
            plain = "guided_plain" if k.startswith("guided") else "unguided_plain"
            if k != plain:
                entry[k]["over_plain"] = entry[k]["ms_per_step"] / entry[plain]["ms_per_step"]
                entry[k]["ms_per_step_added"] = entry[k]["ms_per_step"] - entry[plain]["ms_per_step"]
        res["batches"][str(B)] = entry
        print(json.dumps({"B": B, **{k: [round(entry[k]["ms_per_step"], 4)] + [round(x, 4) for x in entry[k]["ms_per_step_min_max"]] for k in legs}}),
              flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (after every shape: a later one that fails leaves the earlier results)
            json.dump(res, f, indent=1)
            f.write("\n")
        del xT, c2, c1, x1, a1, b1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
