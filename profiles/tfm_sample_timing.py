"""Times sampling from the CustomTransformer three ways at the reference's configuration (input 40000, hidden 1024, 8 heads, 8 layers, 34-row
windows, 50 steps):

  generic         sample() with native_tfm_sampler off: the Python loop, one dq_tfm_fwd and one stand-alone update kernel per step
  native_eager    dq_tfm_sample, use_graph off
  native_captured dq_tfm_sample, one captured step replayed

at B = 1 and B = 32.  Each path is warmed up with one whole call (the captured path captures there), then the paths are timed in turn, round
after round, so that a drift of the machine hits all three alike; a call is timed with the host clock around work that ends in a device
synchronise.  Reported per path: the median and the spread (min, max) of the calls, as ms per step and windows per second.  The script also
counts the launches of one step before and after from the shapes (every GEMM through the library's own plan: a split product is two launches).

    python profiles/tfm_sample_timing.py --out profiles/tfm_sample.json

Needs the GPU; it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd"))

from dquartic import _native as N  # noqa: E402
from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter  # noqa: E402
from dquartic.model.model import DDIMDiffusionModel  # noqa: E402


def gemm_launches(M, Nn, K, batch=1):
    p = N.gemm_plan(M, Nn, K, batch=batch, splits=1 if batch > 1 else 0)
    n = 0
    for part in (p["full"], p["rest"]):
        if part["ntiles"]:
            n += 2 if part["splits"] > 1 else 1
    return n


def launches_per_step(B, S1, S2, D, H, heads, layers, fused):
    """(generic loop, native loop): kernel launches of one step, counted from the launch sequences of dq_tfm_fwd and dq_tfm_sample"""
    R1, Sk, dh = B * S1, S1 + S2, H // heads
    ff = gemm_launches(R1, 4 * H, H) + 1 + gemm_launches(R1, H, 4 * H)  # ff.0, GELU, ff.2
    attn3 = gemm_launches(S1, Sk, dh, B * heads) + 1 + gemm_launches(S1, dh, Sk, B * heads)
    before_layer = 1 + gemm_launches(R1, H, H) + gemm_launches(B * Sk, 2 * H, H) + attn3 + gemm_launches(R1, H, H) + 1 + ff + 1
    time_mlp = 1 + gemm_launches(B, 4 * H, H) + 1 + gemm_launches(B, H, 4 * H)
    before = time_mlp + gemm_launches(R1, H, D) + 1 + 1 + layers * before_layer + gemm_launches(R1, D, H) + 1  # ... + the update
    kv = gemm_launches(S1, 2 * H, H, B)
    after_layer = gemm_launches(R1, H, H) + kv + (1 if fused else attn3) + gemm_launches(R1, H, H) + 1 + ff + 1
    after = gemm_launches(R1, H, D) + 1 + layers * after_layer + gemm_launches(R1, D, H) + 1  # ... + the update (captured: + the step counter)
    return before, after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "tfm_sample.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tfm_sample_timing needs the GPU")
    D, H, heads, layers, S = 40000, 1024, 8, 8, 34
    torch.manual_seed(0)
    net = DDIMTransformerAdapter(CustomTransformer(input_dim=D, hidden_dim=H, num_heads=heads, num_layers=layers)).cuda()
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=1000, beta_schedule_type="cosine", pred_type="eps", auto_normalize=True, device="cuda")
    fused = N.lib().dq_tfm_attn_form(S, 2 * S, H // heads)
    res = {"config": {"input_dim": D, "hidden_dim": H, "num_heads": heads, "num_layers": layers, "S1": S, "S2": S, "num_steps": a.steps,
                      "rounds": a.rounds}, "device": torch.cuda.get_device_name(0), "build_id": N.build_id(), "attention_form": int(fused),
           "batches": {}}

    def setting(native, graph):
        dm.native_tfm_sampler, dm.use_graph = native, graph

    paths = {"generic": (False, True), "native_eager": (True, False), "native_captured": (True, True)}
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        xT, c2, c1 = torch.randn(B, S, D, generator=g).cuda(), torch.rand(B, S, D, generator=g).cuda(), torch.rand(B, S, generator=g).cuda()
        times = {k: [] for k in paths}
        outs = {}
        with torch.no_grad():
            for k, s in paths.items():  # warm-up: every shape the timed window uses, and the capture
                setting(*s)
                outs[k] = dm.sample(xT, c2, c1, num_steps=a.steps)[0]
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, s in paths.items():
                    setting(*s)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    dm.sample(xT, c2, c1, num_steps=a.steps)
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
        before, after = launches_per_step(B, S, S, D, H, heads, layers, fused)
        scale = float(outs["generic"].abs().max())
        entry = {"launches_per_step": {"generic": before, "native_eager": after, "native_captured": after + 1},
                 "captured_equals_eager": bool(torch.equal(outs["native_eager"], outs["native_captured"])),
                 "native_vs_generic_max_abs_diff": float((outs["native_captured"] - outs["generic"]).abs().max()), "generic_max_abs": scale}
        for k, v in times.items():
            med = statistics.median(v)
            entry[k] = {"call_s": {"median": med, "min": min(v), "max": max(v)}, "ms_per_step": 1e3 * med / a.steps,
                        "ms_per_step_min_max": [1e3 * min(v) / a.steps, 1e3 * max(v) / a.steps], "windows_per_s": B / med}
        res["batches"][str(B)] = entry
        print(json.dumps({"B": B, **{k: round(entry[k]["ms_per_step"], 4) for k in paths}, "launches": entry["launches_per_step"]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
