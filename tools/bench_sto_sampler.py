"""What stochastic sampling (eta > 0) costs.  One process, HIP events around whole sampling calls, the forms
interleaved (the order rotates every round), median and 10th-90th percentile over the rounds; B = 512 windows of (400, 64), 50 steps,
graph path:

  b  dq_ddim_sample at eta = 0 (eta, seed and ids written into the record)
  c  dq_ddim_sample at eta = 1
  d  eta = 1 the torch way: per step the network forward, the deterministic update (dq_ddim_step) and x += sigma * torch.randn_like(x)
     (no graph: a fresh torch.randn per step is what a captured step cannot hold)

Form "a" -- dq_ddim_sample of the commit before stochastic sampling, loaded from a second library through its 22-argument signature -- is
gone: since ABI version 13 a sampling call crosses as a record (dq_sample_call), and a library that old cannot be called through this
tree's bindings.  Its recorded results stay (profiles/sto_sampler_run1.json, run2.json).

    python tools/bench_sto_sampler.py [--rounds N] [--out FILE]      (run it twice: the spread of two runs is the yardstick)"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd")]

from dquartic import _native as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    from bench import MZ, RT, build_model, make_batches

    torch.manual_seed(0)
    net, dm = build_model("cuda")
    net.eval()
    _, c2, c1 = make_batches(1, a.batch, 0, 1, "cuda")[0]
    x = torch.randn(a.batch, RT, MZ, device="cuda")
    ns = a.steps
    ts = [int(v) for v in dm.sampler_timesteps(dm.num_timesteps, ns)]
    _, sigma = dm.ddim_coef_table(ts, 1.0)
    c2n, c1n = dm.normalize(c2), dm.normalize(c1)
    res = {}

    def ex(eta):
        def run():
            with torch.no_grad():
                res[eta] = dm._sample_native(x, c2, c1, ns, eta=eta, seed=1234)
        return run

    def torch_way():
        with torch.no_grad():
            xt = x
            for i, t in enumerate(ts):
                xt, _ = dm.p_sample(xt, t, c2n, c1n)
                if t > 0:
                    xt += float(sigma[i]) * torch.randn_like(xt)
            res["d"] = xt

    forms = {}
    forms["b_ex_eta0"] = ex(0.0)
    forms["c_ex_eta1"] = ex(1.0)
    forms["d_torch_randn_unfused"] = torch_way
    names = list(forms)
    for _ in range(2):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for r in range(a.rounds):
        k0 = r % len(names)
        for k in names[k0:] + names[:k0]:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            forms[k]()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e))
    out = {"build_id": N.build_id(), "device": torch.cuda.get_device_name(0), "shape": [a.batch, RT, MZ], "steps": ns, "rounds": a.rounds,
           "bytes_per_step_of_k_ddim_step_sto": 12 * a.batch * RT * MZ}
    for k, t in times.items():
        t.sort()
        out[k] = {"median_ms": statistics.median(t), "p10_ms": t[len(t) // 10], "p90_ms": t[(9 * len(t)) // 10],
                  "median_ms_per_step": statistics.median(t) / ns}
    out["c_minus_b_us_per_step"] = (out["c_ex_eta1"]["median_ms"] - out["b_ex_eta0"]["median_ms"]) / ns * 1e3
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
