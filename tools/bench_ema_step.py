"""What the EMA of the weights costs.  Two measurements, each with HIP events, the forms interleaved in one process:

  optimiser   dq_adamw_clip_step_dev | dq_adamw_clip_ema_step_dev | the unfused alternative (the plain step, then e.lerp_(p, w) on the
              flat buffer) at n = 128,847 (the U-Net) and n = 191 M (the reference transformer's size): buffers allocated once, warmed
              up, every round times each form once, the order rotating; median and spread over the rounds.
  step        dq_train_step + step_dev at (32, 400, 64), EMA on and off alternating in blocks of 20 steps, 200 timed steps each; the same
              with the step captured (enable_train_graph).

    python tools/bench_ema_step.py [--skip-big] [--out FILE]      (run it twice: the acceptance is relative to the spread of two runs)"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd")]

from dquartic import _native as N  # noqa: E402

ADAM = (0.9, 0.999, 1e-8, 0.01)
BETA = 0.999


def optimiser_forms(n, rounds, warm):
    dev = "cuda"
    g_ = torch.Generator(device=dev).manual_seed(n % 1000003)
    p, g = torch.randn(n, device=dev, generator=g_), torch.randn(n, device=dev, generator=g_) * 1e-3
    m, v, e = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
    sc, gn = torch.empty(1024, device=dev), torch.zeros((), device=dev)
    lr_dev, step_dev = torch.tensor([1e-5, 0.0], device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    L, s = N.lib(), N.stream_ptr()
    head = (N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), n, N.ptr(sc), 1.0, 10.0, N.ptr(lr_dev), *ADAM, N.ptr(step_dev), N.ptr(gn))

    def plain():
        N.check(L.dq_adamw_clip_step_dev(*head, s), "dq_adamw_clip_step_dev")

    def fused():
        N.check(L.dq_adamw_clip_ema_step_dev(*head, N.ptr(e), BETA, 1, s), "dq_adamw_clip_ema_step_dev")

    def unfused():
        plain()
        e.lerp_(p, 1.0 - BETA)

    forms = {"plain": plain, "fused": fused, "unfused": unfused}
    names = list(forms)
    for _ in range(warm):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for r in range(rounds):
        marks = []
        for k in names[r % 3:] + names[:r % 3]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            forms[k]()
            b.record()
            marks.append((k, a, b))
        torch.cuda.synchronize()
        for k, a, b in marks:
            times[k].append(a.elapsed_time(b) * 1e3)
    out = {"n": n, "rounds": rounds}
    for k, t in times.items():
        t.sort()
        out[k] = {"median_us": statistics.median(t), "p10_us": t[len(t) // 10], "p90_us": t[(9 * len(t)) // 10]}
    out["fused_over_unfused"] = out["fused"]["median_us"] / out["unfused"]["median_us"]
    return out


def train_step_cost(captured, blocks=10, per_block=20):
    from bench import MZ, RT, TRAIN_BATCH, build_model, make_batches

    data = make_batches(4, TRAIN_BATCH, 0, 1, "cuda")
    dms = {}
    for mode in ("off", "on"):
        torch.manual_seed(0)
        _, dm = build_model("cuda")
        dm._set_optimizer(1e-5)
        if mode == "on":
            dm.enable_ema(BETA)
        if captured:
            dm.enable_train_graph()
        dms[mode] = dm

    def run(dm, k):
        for i in range(k):
            x0, c2, c1 = data[i % len(data)]
            if captured:
                dm._train_one_batch(x0, ms2_cond=c2, ms1_cond=c1, sync=False)
            else:
                dm.train_step_fused(x0, c2, c1, zero_grads=True)
                dm.optimizer.step_dev()

    for dm in dms.values():
        run(dm, 30)
    torch.cuda.synchronize()
    per = {"off": [], "on": []}
    for b in range(blocks):
        for mode in (("off", "on") if b % 2 == 0 else ("on", "off")):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(dms[mode], per_block)
            z.record()
            torch.cuda.synchronize()
            per[mode].append(a.elapsed_time(z) * 1e3 / per_block)
    out = {"shape": [TRAIN_BATCH, RT, MZ], "captured": captured, "timed_steps_each": blocks * per_block}
    for mode, t in per.items():
        out[mode] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    out["ema_cost_us"] = out["on"]["median_us"] - out["off"]["median_us"]
    for dm in dms.values():
        if captured:
            dm.enable_train_graph(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-big", action="store_true", help="leave out n = 191 M (six 764 MB buffers)")
    ap.add_argument("--skip-step", action="store_true", help="leave out the train-step measurement")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"build_id": N.build_id(), "device": torch.cuda.get_device_name(0), "optimiser": [], "step": []}
    res["optimiser"].append(optimiser_forms(128847, rounds=300, warm=20))
    if not a.skip_big:
        res["optimiser"].append(optimiser_forms(191_000_000, rounds=30, warm=3))
    if not a.skip_step:
        res["step"] = [train_step_cost(False), train_step_cost(True)]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
