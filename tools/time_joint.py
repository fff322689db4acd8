"""Times joint sampling under mixture consistency on the default U-Net at 256 windows of 400 x 64 -- G = 64 groups of
P = 4 members -- alternating in one process:
  plain_step        a sampling step of the plain call, sampler "ddim" (the update rides in the network's head launch)
  joint_step        the same step with group_size = 4, consistency = "bound": forward, the pass, the x0-form update behind the forward
  pass_alone        dq_group_project on a network-output-sized tensor, in place (the pass's own time)
  update_alone      dq_ddim_step_x0 over the same tensors (what leaves the head launch)
  torch_rule        the same rule composed from torch ops on the same tensors
Steps are timed as `--steps`-step captured calls divided by the step count, so a call's prologue and finish are spread over its steps.

Timing as tools/time_v_objective.py: all paths warmed up, then timed in turn, window after window, so that a drift of the machine hits them
alike; a window is `iters` back-to-back calls between two device events, `iters` chosen so that a window lasts at least --window seconds.
Reported: the median and [min, max] over the windows, and the pass's algorithmic bytes ((3 P + 1) / P * 4 per element of a member) over
its time.

    python tools/time_joint.py --out profiles/joint_sample.json

Needs the GPU; it does not fall back."""
import argparse
import ctypes
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, HERE)

from dquartic import _native as N  # noqa: E402
from time_v_objective import models, time_paths  # noqa: E402


def torch_rule(x0, mix):
    """consistency = "bound" at strength 1 under auto_normalize, from torch ops: x0 (P, G, per), mix (G, per)"""
    y = (x0 + 1) * 0.5
    S = y.clamp_min(0).sum(dim=0)
    m = mix.clamp_min(0)
    z = torch.where((S > m) & (y > 0), y * (m / S), y)
    return torch.where(z == y, x0, 2 * z - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "joint_sample.json"))
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="sampling steps per timed call")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--shape", type=int, nargs=2, default=[400, 64], metavar=("RT", "MZ"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_joint needs the GPU")
    RT, MZ = a.shape
    G, P = a.groups, a.members
    B, per = G * P, RT * MZ
    dms, net = models(MZ)
    dm = dms["eps"]
    net.eval()
    g = torch.Generator().manual_seed(1)
    xT = torch.randn(B, RT, MZ, generator=g).cuda()
    c2 = (0.5 * torch.rand(G, RT, MZ, generator=g)).repeat(P, 1, 1).contiguous().cuda()
    c1 = torch.rand(B, RT, generator=g).cuda()
    out = torch.randn(B, RT, MZ, generator=g).cuda()  # stands for a network output
    coef = torch.tensor([0.8, 0.6, 0.9, 0.43589], dtype=torch.float32).cuda()
    xp, ep = torch.empty_like(xT), torch.empty_like(xT)
    L = N.lib()

    def pass_alone():
        N.check(L.dq_group_project(N.ptr(xT), N.ptr(out), N.ptr(out), N.ptr(c2), N.ptr(coef), N.PRED_TYPES["eps"], 1, G, P, per,
                                   N.CONSISTENCY_MODES["bound"], ctypes.c_float(1.0), N.stream_ptr()), "dq_group_project")

    def update_alone():
        N.check(L.dq_ddim_step_x0(N.ptr(xT), N.ptr(out), N.ptr(xp), N.ptr(ep), N.ptr(coef), xT.numel(), N.stream_ptr()), "dq_ddim_step_x0")

    x0v, mixv = out.view(P, G, per), c2[:G].view(G, per)
    with torch.no_grad():
        paths = {"plain_step": lambda: dm.sample(xT, c2, c1, num_steps=a.steps, sampler="ddim"),
                 "joint_step": lambda: dm.sample(xT, c2, c1, num_steps=a.steps, sampler="ddim", group_size=P, consistency="bound"),
                 "pass_alone": pass_alone, "update_alone": update_alone, "torch_rule": lambda: torch_rule(x0v, mixv)}
        t = time_paths(paths, a.windows, a.window)
    for k in ("plain_step", "joint_step"):  # per step
        t[k] = {"ms": t[k]["ms"] / a.steps, "ms_min_max": [v / a.steps for v in t[k]["ms_min_max"]], "iters_per_window": t[k]["iters_per_window"]}
    nbytes = (3 * P + 1) * 4 * G * per
    res = {"config": {"RT": RT, "MZ": MZ, "groups": G, "members": P, "windows_per_call": B, "steps_per_call": a.steps, "windows": a.windows,
                      "window_s": a.window, "sampler": "ddim", "consistency": "bound", "pred_type": "eps"},
           "device": torch.cuda.get_device_name(0), "build_id": N.build_id(), "ms": t,
           "joint_over_plain": t["joint_step"]["ms"] / t["plain_step"]["ms"],
           "pass_share_of_plain_step": t["pass_alone"]["ms"] / t["plain_step"]["ms"],
           "pass_algorithmic_bytes": nbytes, "pass_GBps": nbytes / (t["pass_alone"]["ms"] * 1e-3) / 1e9,
           "torch_rule_over_pass": t["torch_rule"]["ms"] / t["pass_alone"]["ms"]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
