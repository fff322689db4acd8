#!/usr/bin/env python3
"""Device-event timings of the q_sample and loss entry points (csrc/k_stream.hip) under the library DQ_HIP_LIB
names, and the comparison of two libraries from four or more such runs.

    DQ_HIP_LIB=<parent> python tools/time_stream.py run p1.json
    DQ_HIP_LIB=<this>   python tools/time_stream.py run t1.json
    DQ_HIP_LIB=<parent> python tools/time_stream.py run p2.json
    DQ_HIP_LIB=<this>   python tools/time_stream.py run t2.json
    python tools/time_stream.py combine profiles/stream_skeleton.json p1.json t1.json p2.json t2.json [p3.json t3.json ...]

run: each entry is warmed up for 0.2 s, then timed over 15 windows of back-to-back calls between two device events (a window lasts at least
3 ms); the figure is the median over the windows of microseconds per call.  Entries: dq_q_sample, the three dq_mse_loss_* entries and
the two dq_mse_per_window* entries at (32, 400 * 64) and (512, 400 * 64); dq_eval_step at batch 32, 400 x 64 (tools/measure_eval.py's
network); dq_q_sample_repeats, dq_mse_per_window_repeats and dq_tfm_eval_step at tools/time_tfm_eval.py's sizes.
combine: per entry the parent's and this tree's median over their runs (two or more alternating pairs), the spread = the range of the
parent's runs, within = this tree's median lies within the spread of the parent's, and pass = within, or faster than the parent.  Exit status 1 when an entry does not pass.  Needs the GPU."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd"))


def run(path, windows=15, window_ms=3.0):
    import torch

    from dquartic import _native as N
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    L, s = N.lib(), N.stream_ptr()
    res = {"lib": os.environ.get("DQ_HIP_LIB", ""), "build_id": N.build_id(), "device": torch.cuda.get_device_name(0), "us_per_call": {}}

    def window(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def timed(name, fn):
        t0 = time.perf_counter()  # (warm-up by time, not by count: the clocks need some 50 ms of work to settle, bench.py --warmup)
        while time.perf_counter() - t0 < 0.2:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
        iters = max(1, int(window_ms * 1e3 / window(fn, 5)) + 1)
        us = [window(fn, iters) for _ in range(windows)]
        res["us_per_call"][name] = {"median": statistics.median(us), "min": min(us), "max": max(us), "iters": iters}
        print(json.dumps({"entry": name, "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3)}), flush=True)

    T = 1000
    g = torch.Generator().manual_seed(0)
    ab = torch.linspace(0.9999, 0.0001, T).cuda()
    lw = (ab / (1 - ab)).contiguous()
    seed, per = torch.tensor([7], dtype=torch.int64, device="cuda"), 400 * 64
    for B in (32, 512):
        n = B * per
        x0, nz, e = torch.rand(n, generator=g).cuda(), torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
        t = torch.randint(0, T, (B,), generator=g).cuda()
        o, lo, sc, pw = torch.empty(n, device="cuda"), torch.empty(1, device="cuda"), torch.empty(1024, device="cuda"), torch.empty(B, device="cuda")
        sl = torch.empty(L.dq_mse_per_window_scratch_bytes(B, per) // 8, dtype=torch.float64, device="cuda")
        P = N.ptr
        timed(f"dq_q_sample/{B}", lambda: L.dq_q_sample(P(ab), P(x0), P(t), P(nz), P(o), B, per, 1, s))
        timed(f"dq_mse_loss_fwd_bwd/{B}", lambda: L.dq_mse_loss_fwd_bwd(P(e), P(nz), P(lo), P(o), P(sc), n, s))
        timed(f"dq_mse_loss_weighted_fwd_bwd/{B}", lambda: L.dq_mse_loss_weighted_fwd_bwd(P(e), P(x0), 2.0, -1.0, P(lw), P(t), P(lo), P(o), P(sc), B, per, s))
        timed(f"dq_mse_loss_v_fwd_bwd/{B}", lambda: L.dq_mse_loss_v_fwd_bwd(P(e), P(x0), P(nz), P(ab), 2.0, -1.0, P(lw), P(t), P(lo), P(o), P(sc), B, per, s))
        timed(f"dq_mse_per_window/{B}", lambda: L.dq_mse_per_window(P(e), P(x0), 2.0, -1.0, P(lw), P(t), P(pw), P(lo), P(sl), B, per, s))
        timed(f"dq_mse_per_window_v/{B}", lambda: L.dq_mse_per_window_v(P(e), P(x0), P(nz), P(ab), 2.0, -1.0, P(lw), P(t), P(pw), P(lo), P(sl), B, per, s))
        del x0, nz, e, o, sl

    B, RT, MZ = 32, 400, 64
    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True).cuda()
    dm = DDIMDiffusionModel(model_class=net, device="cuda")
    x0, c2, c1 = torch.rand(B, RT, MZ, device="cuda"), torch.rand(B, RT, MZ, device="cuda"), torch.rand(B, RT, device="cuda")
    t, nz = torch.randint(0, 1000, (B,), device="cuda"), torch.randn(B, RT, MZ, device="cuda")
    timed("dq_eval_step/32", lambda: dm.eval_step(x0, c2, c1, t=t, noise=nz))
    del net, dm

    D, H, heads, layers, S, R = 40000, 1024, 8, 8, 34, 4
    torch.manual_seed(0)
    net = DDIMTransformerAdapter(CustomTransformer(input_dim=D, hidden_dim=H, num_heads=heads, num_layers=layers)).cuda()
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=T, beta_schedule_type="cosine", pred_type="eps", auto_normalize=True, device="cuda")
    per = S * D
    for B in (1, 8, 32):
        g = torch.Generator().manual_seed(B)
        x0, c1 = torch.rand(B, S, D, generator=g).cuda(), torch.rand(B, S, generator=g).cuda()
        t = torch.randint(0, T, (R, B), generator=g).cuda()
        ids = torch.arange(B, device="cuda")
        o, pw, lo = torch.randn(R * B * per, device="cuda"), torch.empty(R * B, device="cuda"), torch.empty(R, device="cuda")
        sl = torch.empty(L.dq_mse_per_window_scratch_bytes(R * B, per) // 8, dtype=torch.float64, device="cuda")
        xt = torch.empty(R * B * per, device="cuda")
        P = N.ptr
        timed(f"dq_q_sample_repeats/{B}", lambda: L.dq_q_sample_repeats(P(dm.alpha_bars), P(x0), P(t), None, P(seed), P(ids), 0, P(xt), B, R, per, 1, s))
        timed(f"dq_mse_per_window_repeats/{B}", lambda: L.dq_mse_per_window_repeats(P(o), None, R * B, 1.0, 0.0, P(seed), P(ids), 0, None, P(t), P(pw), P(lo),
                                                                                    P(sl), B, R, per, s))
        del o, xt, sl
        with torch.no_grad():
            timed(f"dq_tfm_eval_step/{B}", lambda: dm.eval_steps(x0, None, c1, t, seed, ids))
        net.transformer.drop_workspaces()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


def combine(out, *paths):
    runs = [json.load(open(p)) for p in paths]
    med = [{k: v["median"] for k, v in r["us_per_call"].items()} for r in runs]
    res = {"device": runs[0]["device"], "parent_lib": os.path.basename(os.path.dirname(runs[0]["lib"])), "build_id": runs[1]["build_id"],
           "order": "parent, this, ... : %d alternating fresh processes" % len(runs), "entries": {}}
    ok = True
    for k in med[0]:
        ps, ts = [m[k] for m in med[0::2]], [m[k] for m in med[1::2]]
        parent, this, spread = statistics.median(ps), statistics.median(ts), max(ps) - min(ps)
        e = {"parent_us": ps, "this_us": ts, "parent_median_us": parent, "this_median_us": this, "spread_us": spread,
             "within": abs(this - parent) <= spread, "pass": abs(this - parent) <= spread or this <= parent}
        ok = ok and e["pass"]
        res["entries"][k] = e
        print(f"{k:38s} parent {parent:10.3f} us  this {this:10.3f} us  spread {spread:8.3f} us  {'pass' if e['pass'] else 'OUTSIDE'}")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        sys.exit(run(sys.argv[2]))
    if len(sys.argv) >= 7 and len(sys.argv) % 2 == 1 and sys.argv[1] == "combine":
        sys.exit(combine(*sys.argv[2:]))
    sys.exit(__doc__)
