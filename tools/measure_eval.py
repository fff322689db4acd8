"""HIP-event timings of the held-out evaluation entry points (profiles/eval_metrics.md):
dq_recon_metrics at (512, 400, 64) and (8, 2000, 256) against its algorithmic bytes, dq_eval_step against dq_train_step at batch 32,
400 x 64.  Median of `--reps` timed calls after `--warmup`; prints one JSON line per measurement.

    python tools/measure_eval.py [--reps 50] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd"))

from dquartic import _native as N  # noqa: E402
from dquartic.model import evaluation as E  # noqa: E402
from dquartic.model.model import DDIMDiffusionModel  # noqa: E402
from dquartic.model.unet1d import UNet1d  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    for B, RT, MZ in ((512, 400, 64), (8, 2000, 256)):
        # the inputs rotate through enough (pred, target) pairs to exceed the 256 MB last-level cache twice over: a call never finds its
        # inputs left there by the call before it, so the figure is against HBM
        pair_bytes = 8 * B * RT * MZ
        sets = [(torch.rand(B, RT, MZ, device="cuda"), torch.rand(B, RT, MZ, device="cuda")) for _ in range(-(-(600 << 20) // pair_bytes) + 1)]
        nbytes = N.lib().dq_recon_metrics_scratch_bytes(B, RT, MZ)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        out = torch.empty(B, 9, device="cuda")
        turn = [0]

        def fn():
            p, t = sets[turn[0] % len(sets)]
            turn[0] += 1
            N.check(N.lib().dq_recon_metrics(N.ptr(p), N.ptr(t), N.ptr(out), N.ptr(scratch), nbytes, B, RT, MZ, N.stream_ptr()), "dq_recon_metrics")

        med, best = timed(fn, a.reps, a.warmup)
        del sets
        algo = 16 * B * RT * MZ + 2 * nbytes  # P and T read by both passes; every moment slot written once and read once
        print(json.dumps({"what": "dq_recon_metrics", "shape": [B, RT, MZ], "median_ms": round(med, 4), "min_ms": round(best, 4),
                          "input_sets": -(-(600 << 20) // pair_bytes) + 1, "algorithmic_MB": round(algo / 1e6, 2), "GB_per_s_at_median": round(algo / med / 1e6, 1), "build_id": N.build_id()}))
    B, RT, MZ = 32, 400, 64
    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True).cuda()
    dm = DDIMDiffusionModel(model_class=net, device="cuda")
    x0, c2, c1 = torch.rand(B, RT, MZ, device="cuda"), torch.rand(B, RT, MZ, device="cuda"), torch.rand(B, RT, device="cuda")
    t, nz = torch.randint(0, 1000, (B,), device="cuda"), torch.randn(B, RT, MZ, device="cuda")
    for name, fn in (("dq_train_step", lambda: dm.train_step_fused(x0, c2, c1, t=t, noise=nz)),
                     ("dq_eval_step", lambda: dm.eval_step(x0, c2, c1, t=t, noise=nz))):
        med, best = timed(fn, a.reps, a.warmup)
        print(json.dumps({"what": name, "shape": [B, RT, MZ], "median_ms": round(med, 4), "min_ms": round(best, 4), "build_id": N.build_id()}))


if __name__ == "__main__":
    main()
