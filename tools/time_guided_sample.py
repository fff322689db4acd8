"""Times classifier-free guided sampling of the default U-Net at the bench shape (400 x 64 windows, 50 steps) three
ways, at batch B = 256 and B = 1:

  guided        sample(..., guidance_scale=w) at batch B: dq_ddim_sample with `guided` set -- one captured step per timestep, the forward at 2 B
                windows, the combination inside the update kernel
  unguided_2B   sample(...) at batch 2 B: the same forward size without guidance (the update in the head launch) -- what the guided call
                should cost
  python        the composition a user would write without the option: per step two forwards at batch B through UNet1d.forward (the
                caller's MS1, then the null's), g = u + w (c - u) and the reference update in torch arithmetic; no captured graph

All paths are warmed up per shape, then timed in turn, window after window, in one process, so that a drift of the machine hits them
alike.  A timing window is `iters` back-to-back calls between two device events, the second followed by a synchronise; `iters` is chosen per
path and shape from the warm-up so that a window lasts at least --window seconds.  Reported per path: the median and the spread (min, max)
over the windows as ms per step.  The claim to check is guided / unguided_2B ~ 1 within that spread.

    python tools/time_guided_sample.py --out profiles/guided_sample.json

Needs the GPU; it does not fall back."""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd"))

from dquartic import _native as N  # noqa: E402
from dquartic.model.model import DDIMDiffusionModel  # noqa: E402
from dquartic.model.unet1d import UNet1d  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "guided_sample.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--null-ms1", type=float, default=0.0)
    ap.add_argument("--windows", type=int, default=7, help="timing windows per path and shape")
    ap.add_argument("--window", type=float, default=0.3, help="least length of a timing window in seconds")
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--shape", type=int, nargs=2, default=[400, 64], metavar=("RT", "MZ"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_guided_sample needs the GPU")
    RT, MZ = a.shape
    ns, w, null = a.steps, a.scale, a.null_ms1
    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True).cuda()
    dm = DDIMDiffusionModel(model_class=net, device="cuda")
    net.eval()
    res = {"config": {"RT": RT, "MZ": MZ, "steps": ns, "guidance_scale": w, "null_ms1": null, "windows": a.windows, "window_s": a.window},
           "device": torch.cuda.get_device_name(0), "build_id": N.build_id(), "batches": {}}
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        xT, c2, c1 = (torch.randn(2 * B, RT, MZ, generator=g).cuda(), torch.rand(2 * B, RT, MZ, generator=g).cuda(),
                      torch.rand(2 * B, RT, generator=g).cuda())
        x1, a1, b1 = xT[:B].contiguous(), c2[:B].contiguous(), c1[:B].contiguous()
        ts = [int(t) for t in dm.sampler_timesteps(dm.num_timesteps, ns)]
        ab = dm.alpha_bars

        def guided():
            return dm.sample(x1, a1, b1, num_steps=ns, guidance_scale=w, null_ms1=null)[0]

        def unguided_2B():
            return dm.sample(xT, c2, c1, num_steps=ns)[0]

        def python():
            c2n, c1n, un = dm.normalize(a1), dm.normalize(b1), dm.normalize(torch.full_like(b1, null))
            x = x1
            for t in ts:
                tt = torch.full((B,), t, device=x.device, dtype=torch.long)
                c, u = net(x, tt, c2n, c1n), net(x, tt, c2n, un)
                e = u + w * (c - u)
                sa, sb = torch.sqrt(ab[t]), torch.sqrt(1.0 - ab[t])
                x0 = (x - sb * e) / sa
                x = torch.sqrt(ab[t - 1]) * x0 + torch.sqrt(1.0 - ab[t - 1]) * e if t > 0 else x0
            return dm.unnormalize(x)

        paths = {"guided": guided, "unguided_2B": unguided_2B, "python": python}

        def window(fn, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / iters  # seconds per call

        iters, times, vals = {}, {k: [] for k in paths}, {}
        with torch.no_grad():
            for k, fn in paths.items():  # warm-up: workspaces, the captured step, then the size of a window
                vals[k] = fn().clone()
                window(fn, 1)
                iters[k] = max(1, int(a.window / window(fn, 2)) + 1)
            for _ in range(a.windows):
                for k, fn in paths.items():
                    times[k].append(window(fn, iters[k]))
        # (the guided call and the Python composition compute the same sample up to fp32 rounding: the plans differ between B and 2 B)
        rel = float((vals["guided"] - vals["python"]).abs().max() / vals["python"].abs().max())
        entry = {"guided_vs_python_max_rel_diff": rel, "iters_per_window": iters,
                 "workspace_bytes": {"guided": int(N.lib().dq_unet_workspace_bytes(net._plan, 2 * B, RT, 0)),
                                     "unguided_2B": int(N.lib().dq_unet_workspace_bytes(net._plan, 2 * B, RT, 0)),
                                     "unguided_B": int(N.lib().dq_unet_workspace_bytes(net._plan, B, RT, 0))}}
        for k, v in times.items():
            med = statistics.median(v)
            entry[k] = {"ms_per_step": 1e3 * med / ns, "ms_per_step_min_max": [1e3 * min(v) / ns, 1e3 * max(v) / ns]}
        entry["guided_over_unguided_2B"] = entry["guided"]["ms_per_step"] / entry["unguided_2B"]["ms_per_step"]
        entry["python_over_guided"] = entry["python"]["ms_per_step"] / entry["guided"]["ms_per_step"]
        res["batches"][str(B)] = entry
        print(json.dumps({"B": B, **{k: [round(entry[k]["ms_per_step"], 4)] + [round(x, 4) for x in entry[k]["ms_per_step_min_max"]] for k in paths},
                          "guided_over_unguided_2B": round(entry["guided_over_unguided_2B"], 4), "guided_vs_python_max_rel_diff": rel}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (after every shape: a later one that fails leaves the earlier results)
            json.dump(res, f, indent=1)
            f.write("\n")
        del xT, c2, c1, x1, a1, b1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
