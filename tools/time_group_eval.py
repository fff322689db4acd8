"""Times the two kernels behind the evaluation of joint sampling at G = 64 groups of P = 4 members out of K = 4
components, 400 x 64 windows, from a dataset of --resident windows held in HBM:

  group_batch    one dq_mix_group_batch call: count + 2 P + 1 = 13 windows of traffic per group
  p_mix_batches  the same targets from P dq_mix_batch calls on indices whose row 0 is swapped with row p (fixed weights swapped alike:
                 the bit-exact anchor of tests/test_group_batch.py): P (count + 2) = 24 windows per group
  group_metrics  one dq_group_metrics call on (P G, RT, MZ) predictions / targets and the (G, RT, MZ) mixture
  torch_fp32/64  the same quantities from torch ops on the device (einsum for the P x P inner products, clamp / sum for the rest), in the
                 input precision and in float64 (the precision dq_group_metrics sums in)

The paths of a comparison are warmed up, then timed in turn, window after window, in one process (tools/time_mix_batch.py's scheme): a
timing window is `iters` back-to-back calls between two device events, `iters` chosen from the warm-up so that a window lasts at least
--window seconds.  Reported per path: median [min, max] over the windows in ms per call, and whether the two ranges separate.

    python tools/time_group_eval.py --out profiles/group_eval.json

Needs the GPU; it does not fall back."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd"))

from dquartic import _native as N  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters  # seconds per call


def alternate(paths, a):
    """{name: {"ms": {"median", "min_max"}, "iters_per_window"}} of the paths timed in turn"""
    iters, times = {}, {k: [] for k in paths}
    for k, fn in paths.items():
        window(fn, 3)
        iters[k] = max(1, int(a.window / window(fn, 10)) + 1)
    for _ in range(a.windows):
        for k, fn in paths.items():
            times[k].append(window(fn, iters[k]))
    return {k: {"ms": {"median": 1e3 * statistics.median(v), "min_max": [1e3 * min(v), 1e3 * max(v)]}, "iters_per_window": iters[k]}
            for k, v in times.items()}


def separated(x, y):
    """the ranges of two paths do not overlap"""
    return x["ms"]["min_max"][1] < y["ms"]["min_max"][0] or y["ms"]["min_max"][1] < x["ms"]["min_max"][0]


def time_group_batch(a, res):
    RT, MZ = a.shape
    G, P, K, n, per = a.groups, a.members, a.components, a.resident, RT * MZ
    g = torch.Generator(device="cuda").manual_seed(0)
    ms2 = torch.rand(n, RT, MZ, device="cuda", generator=g) * 50
    ms1 = torch.rand(n, RT, device="cuda", generator=g) * 500
    lib, st = N.lib(), N.stream_ptr()
    rng = np.random.default_rng(G)
    sets = [np.stack([rng.permutation(n)[:K] for _ in range(G)], axis=1).astype(np.int64) for _ in range(a.index_sets)]
    swapped = []  # per set, per member: rows 0 and p swapped
    for s in sets:
        per_member = []
        for p in range(P):
            t = s.copy()
            t[[0, p]] = t[[p, 0]]
            per_member.append(torch.from_numpy(t).cuda())
        swapped.append(per_member)
    sets = [torch.from_numpy(s).cuda() for s in sets]
    w = [0.5 ** (j + 1) for j in range(K)]
    fixed = (ctypes.c_float * K)(*w)
    fixed_p = []
    for p in range(P):
        v = list(w)
        v[0], v[p] = v[p], v[0]
        fixed_p.append((ctypes.c_float * K)(*v))
    new = lambda *s: torch.empty(s, device="cuda")
    tgt, cond, m1, rest, wout = new(P * G, RT, MZ), new(P * G, RT, MZ), new(P * G, RT), new(G, RT, MZ), new(G, K)
    tgt_p, cond_p, m1_p, rest_p = new(P * G, RT, MZ), new(P * G, RT, MZ), new(P * G, RT), new(G, RT, MZ)
    sc = new(max(lib.dq_mix_group_batch_scratch_bytes(G, K, P), lib.dq_mix_batch_scratch_bytes(G, K)) // 4)
    turn = {"group_batch": 0, "p_mix_batches": 0}

    def group_batch():
        turn["group_batch"] = (turn["group_batch"] + 1) % len(sets)
        N.check(lib.dq_mix_group_batch(N.ptr(ms2), N.ptr(ms1), n, N.ptr(sets[turn["group_batch"]]), None, G, K, P, RT, MZ, RT, fixed, 0, None, None,
                                       0, 1, N.ptr(tgt), N.ptr(m1), N.ptr(cond), N.ptr(rest), N.ptr(wout), N.ptr(sc), sc.numel() * 4, st),
                "dq_mix_group_batch")

    def p_mix_batches():
        turn["p_mix_batches"] = (turn["p_mix_batches"] + 1) % len(sets)
        for p in range(P):
            N.check(lib.dq_mix_batch(N.ptr(ms2), N.ptr(ms1), n, N.ptr(swapped[turn["p_mix_batches"]][p]), None, G, K, RT, MZ, RT, fixed_p[p], 0,
                                     None, None, 0, 1, N.ptr(tgt_p[p * G:]), N.ptr(m1_p[p * G:]), N.ptr(cond_p[p * G:]), None, N.ptr(wout),
                                     N.ptr(sc), sc.numel() * 4, st), "dq_mix_batch")

    # the two forms agree bit for bit on the targets and the MS1 rows before anything is timed
    turn["group_batch"] = turn["p_mix_batches"] = 0
    group_batch()
    p_mix_batches()
    torch.cuda.synchronize()
    assert torch.equal(tgt.view(torch.int32), tgt_p.view(torch.int32)) and torch.equal(m1.view(torch.int32), m1_p.view(torch.int32))
    entry = alternate({"group_batch": group_batch, "p_mix_batches": p_mix_batches}, a)
    entry["algorithmic_bytes"] = {"group_batch": G * 4 * ((K + 2 * P + 1) * per + 2 * P * RT), "p_mix_batches": G * 4 * P * ((K + 2) * per + 2 * RT)}
    entry["group_over_p_calls"] = entry["group_batch"]["ms"]["median"] / entry["p_mix_batches"]["ms"]["median"]
    entry["ranges_separate"] = separated(entry["group_batch"], entry["p_mix_batches"])
    res["group_batch"] = entry
    print(json.dumps({"group_batch": entry}), flush=True)


def time_group_metrics(a, res):
    RT, MZ = a.shape
    G, P = a.groups, a.members
    g = torch.Generator(device="cuda").manual_seed(1)
    target = torch.rand(P * G, RT, MZ, device="cuda", generator=g)
    pred = target + 0.3 * torch.randn(P * G, RT, MZ, device="cuda", generator=g)
    mix = target.view(P, G, RT, MZ).sum(0) * 0.9
    lib, st = N.lib(), N.stream_ptr()
    nbytes = lib.dq_group_metrics_scratch_bytes(G, P, RT, MZ)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    cross, group = torch.empty(G, P, P, device="cuda"), torch.empty(G, 3, device="cuda")

    def group_metrics():
        N.check(lib.dq_group_metrics(N.ptr(pred), N.ptr(target), N.ptr(mix), N.ptr(cross), N.ptr(group), N.ptr(scratch), nbytes, G, P, RT, MZ, st),
                "dq_group_metrics")

    def with_torch(dtype):
        def fn():
            pr, tg, mx = pred.view(P, G, -1).to(dtype), target.view(P, G, -1).to(dtype), mix.view(G, -1).to(dtype)
            pt = torch.einsum("pgn,qgn->gpq", pr, tg)
            pp, tt = (pr * pr).sum(-1), (tg * tg).sum(-1)
            den = torch.sqrt(pp.t()[:, :, None] * tt.t()[:, None, :])
            c = torch.where(den > 0, pt / den, torch.zeros_like(pt))
            S, mp = pr.clamp(min=0).sum(0), mx.clamp(min=0)
            tot = mp.sum(-1)
            ex, un = (S - mp).clamp(min=0).sum(-1) / tot, (mp - S).clamp(min=0).sum(-1) / tot
            return c.float(), torch.stack([ex, un, tot], dim=1).float()
        return fn

    group_metrics()
    c64, g64 = with_torch(torch.float64)()
    torch.cuda.synchronize()
    assert float((cross - c64).abs().max()) < 1e-6 and float(((group - g64).abs() / g64.abs().clamp(min=1e-30)).max()) < 1e-6
    entry = alternate({"group_metrics": group_metrics, "torch_fp32": with_torch(torch.float32), "torch_fp64": with_torch(torch.float64)}, a)
    entry["algorithmic_bytes"] = G * 4 * (2 * P + 1) * RT * MZ
    for k in ("torch_fp32", "torch_fp64"):
        entry[f"kernel_over_{k}"] = entry["group_metrics"]["ms"]["median"] / entry[k]["ms"]["median"]
        entry[f"ranges_separate_{k}"] = separated(entry["group_metrics"], entry[k])
    res["group_metrics"] = entry
    print(json.dumps({"group_metrics": entry}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "group_eval.json"))
    ap.add_argument("--windows", type=int, default=7, help="timing windows per path")
    ap.add_argument("--window", type=float, default=0.3, help="least length of a timing window in seconds")
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--shape", type=int, nargs=2, default=[400, 64], metavar=("RT", "MZ"))
    ap.add_argument("--resident", type=int, default=8192, help="windows of the resident dataset")
    ap.add_argument("--index-sets", type=int, default=8, help="index sets a path walks through")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_group_eval needs the GPU")
    res = {"config": {"RT": a.shape[0], "MZ": a.shape[1], "G": a.groups, "P": a.members, "K": a.components, "windows": a.windows,
                      "window_s": a.window, "resident_windows": a.resident, "index_sets": a.index_sets},
           "device": torch.cuda.get_device_name(0), "build_id": N.build_id()}
    time_group_batch(a, res)
    time_group_metrics(a, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
