"""Times the formation of K-component mixture batches on 400 x 64 windows at B = 32 and B = 512, from a dataset
of --resident windows held in HBM:

  pair          dq_pair_batch: two windows, fixed weights, five output streams (ms2_1, ms2_2, ms2_cond, ms1_1, ms1_2) -- the entry this
                library has always had, unchanged here: the yardstick
  mix2_fixed    dq_mix_batch at K = 2 with the same fixed weights and the same index pairs, scale_target = 0: four output streams
                (ms2_target, ms2_rest, ms2_cond, ms1_target) -- what the pair form computes, bit for bit
  mix4_drawn    dq_mix_batch at K = 4, every component present, weights drawn (max_ratio_log2 = 3), scale_target = 1

All paths are warmed up per shape, then timed in turn, window after window, in one process, so that a drift of the machine hits them
alike.  A timing window is `iters` back-to-back calls between two device events, the second followed by a synchronise; `iters` is chosen
per path and shape from the warm-up so that a window lasts at least --window seconds.  Successive calls of a path walk through --index-sets
different index sets (the same ones for every path), so that a call does not find its own windows of the call before in the caches; at
B = 32 the sets together are still smaller than the Infinity Cache, which all three paths enjoy alike.  Reported per path: the median and
the spread (min, max) over the windows in ms per call, and the same as GB/s of the call's algorithmic bytes (every window read once, every
output written once).  The claim to check is mix2_fixed / pair ~ 1 within that spread.

Then the batch-32 train step of the default U-Net, fed by ResidentMixLoader (its defaults: 2..4 components, drawn weights) and by
ResidentPairLoader over the same windows: one epoch of each in turn, --windows times, in windows per second of wall time (host work of the
loaders included).

    python tools/time_mix_batch.py --out profiles/mix_batch.json

Needs the GPU; it does not fall back."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

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


def summary(v, scale=1.0):
    return {"median": scale * statistics.median(v), "min_max": [scale * min(v), scale * max(v)]}


def time_kernels(a, res):
    RT, MZ = a.shape
    per, n = RT * MZ, a.resident
    g = torch.Generator(device="cuda").manual_seed(0)
    ms2 = torch.rand(n, RT, MZ, device="cuda", generator=g) * 50
    ms1 = torch.rand(n, RT, device="cuda", generator=g) * 500
    seed = torch.tensor([12345], dtype=torch.int64, device="cuda")
    lib = N.lib()
    for B in a.batches:
        rng = np.random.default_rng(B)
        sets4 = [torch.from_numpy(np.stack([rng.permutation(n)[:4] for _ in range(B)], axis=1).astype(np.int64)).cuda() for _ in range(a.index_sets)]
        sets2 = [s[:2].contiguous() for s in sets4]  # rows (2, B) = [idx1 | idx2]: the pair form's layout too
        new = lambda *s: torch.empty(s, device="cuda")
        o = [new(B, RT, MZ) for _ in range(3)]
        m1, m2, wout2, wout4 = new(B, RT), new(B, RT), new(B, 2), new(B, 4)
        sc = new(max(lib.dq_pair_batch_scratch_bytes(B), lib.dq_mix_batch_scratch_bytes(B, 4)) // 4)
        half = (ctypes.c_float * 2)(0.5, 0.5)
        turn = {"pair": 0, "mix2_fixed": 0, "mix4_drawn": 0}
        st = N.stream_ptr()

        def nxt(k, sets):
            turn[k] = (turn[k] + 1) % len(sets)
            return sets[turn[k]]

        def pair():
            N.check(lib.dq_pair_batch(N.ptr(ms2), N.ptr(ms1), n, N.ptr(nxt("pair", sets2)), B, RT, MZ, RT, 0.5, 0.5, N.ptr(o[0]), N.ptr(m1),
                                      N.ptr(o[1]), N.ptr(m2), N.ptr(o[2]), N.ptr(sc), sc.numel() * 4, st), "dq_pair_batch")

        def mix2_fixed():
            N.check(lib.dq_mix_batch(N.ptr(ms2), N.ptr(ms1), n, N.ptr(nxt("mix2_fixed", sets2)), None, B, 2, RT, MZ, RT, half, 0, None, None, 0, 0,
                                     N.ptr(o[0]), N.ptr(m1), N.ptr(o[2]), N.ptr(o[1]), N.ptr(wout2), N.ptr(sc), sc.numel() * 4, st), "dq_mix_batch")

        def mix4_drawn():
            N.check(lib.dq_mix_batch(N.ptr(ms2), N.ptr(ms1), n, N.ptr(nxt("mix4_drawn", sets4)), None, B, 4, RT, MZ, RT, None, 3, N.ptr(seed), None,
                                     turn["mix4_drawn"], 1, N.ptr(o[0]), N.ptr(m1), N.ptr(o[2]), N.ptr(o[1]), N.ptr(wout4), N.ptr(sc),
                                     sc.numel() * 4, st), "dq_mix_batch")

        paths = {"pair": pair, "mix2_fixed": mix2_fixed, "mix4_drawn": mix4_drawn}
        # windows read + MS2 outputs written, then the MS1 rows read + written
        bytes_ = {"pair": B * 4 * (5 * per + 4 * RT), "mix2_fixed": B * 4 * (5 * per + 2 * RT), "mix4_drawn": B * 4 * (7 * per + 2 * RT)}
        iters, times = {}, {k: [] for k in paths}
        for k, fn in paths.items():
            window(fn, 3)
            iters[k] = max(1, int(a.window / window(fn, 20)) + 1)
        # the two forms of the pair agree bit for bit on this data before anything is timed
        turn["pair"] = turn["mix2_fixed"] = 0
        pair()
        ref = [o[0].clone(), o[2].clone(), m1.clone()]
        mix2_fixed()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ref, (o[0], o[2], m1)))
        for _ in range(a.windows):
            for k, fn in paths.items():
                times[k].append(window(fn, iters[k]))
        entry = {"iters_per_window": iters, "algorithmic_bytes": bytes_}
        for k, v in times.items():
            entry[k] = {"ms": summary(v, 1e3), "GBps": summary([bytes_[k] / t for t in v], 1e-9)}
        entry["mix2_fixed_over_pair"] = entry["mix2_fixed"]["ms"]["median"] / entry["pair"]["ms"]["median"]
        entry["pair_spread"] = entry["pair"]["ms"]["min_max"][1] / entry["pair"]["ms"]["min_max"][0]
        res["batches"][str(B)] = entry
        print(json.dumps({"B": B, **{k: [round(entry[k]["ms"]["median"], 4)] + [round(x, 4) for x in entry[k]["ms"]["min_max"]] +
                                      [round(entry[k]["GBps"]["median"], 1)] for k in paths},
                          "mix2_fixed_over_pair": round(entry["mix2_fixed_over_pair"], 4)}), flush=True)
        del sets4, sets2, o
    del ms2, ms1
    torch.cuda.empty_cache()


def time_train_step(a, res):
    from dquartic.utils.data_loader import DIAMSDataset, ResidentMixLoader, ResidentPairLoader

    RT, MZ = a.shape
    B, n = 32, 32 * a.train_steps
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:  # (the loaders upload the files' windows once; the dataset object only draws indices after that)
        np.save(os.path.join(tmp, "ms2.npy"), (rng.random((n, RT, MZ), dtype=np.float32) * 50))
        np.save(os.path.join(tmp, "ms1.npy"), (rng.random((n, RT), dtype=np.float32) * 500))
        ds = DIAMSDataset(ms2_file=os.path.join(tmp, "ms2.npy"), ms1_file=os.path.join(tmp, "ms1.npy"), normalize="minmax")
        loaders = {"mix": ResidentMixLoader(ds, B, device="cuda"), "pair": ResidentPairLoader(ds, B, device="cuda")}
        return _train_epochs(a, res, ds, loaders, n)


def _train_epochs(a, res, ds, loaders, n):
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    MZ = a.shape[1]
    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                 downsample_dim=MZ, simple=True).cuda()
    dm = DDIMDiffusionModel(model_class=net, device="cuda")
    dm._prepare_training(1e-5)

    def epoch(loader):
        ds.reset_epoch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = dm._train_one_epoch(0, loader)
        torch.cuda.synchronize()
        assert len(losses) == a.train_steps and all(np.isfinite(v) for v in losses)
        return n / (time.perf_counter() - t0)

    rates = {k: [] for k in loaders}
    for ld in loaders.values():
        epoch(ld)  # warm-up: workspaces, the optimiser's state
    for _ in range(a.windows):
        for k, ld in loaders.items():
            rates[k].append(epoch(ld))
    res["train_step_b32"] = {"steps_per_epoch": a.train_steps, **{k: {"windows_per_s": summary(v)} for k, v in rates.items()},
                             "mix_over_pair": statistics.median(rates["mix"]) / statistics.median(rates["pair"])}
    print(json.dumps({"train_step_b32": {k: round(statistics.median(v), 1) for k, v in rates.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "mix_batch.json"))
    ap.add_argument("--windows", type=int, default=7, help="timing windows per path and shape")
    ap.add_argument("--window", type=float, default=0.3, help="least length of a timing window in seconds")
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 512])
    ap.add_argument("--shape", type=int, nargs=2, default=[400, 64], metavar=("RT", "MZ"))
    ap.add_argument("--resident", type=int, default=8192, help="windows of the resident dataset")
    ap.add_argument("--index-sets", type=int, default=8, help="index sets a path walks through")
    ap.add_argument("--train-steps", type=int, default=16, help="steps of a timed epoch of the train step (0: skip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mix_batch needs the GPU")
    res = {"config": {"RT": a.shape[0], "MZ": a.shape[1], "windows": a.windows, "window_s": a.window, "resident_windows": a.resident,
                      "index_sets": a.index_sets},
           "device": torch.cuda.get_device_name(0), "build_id": N.build_id(), "batches": {}}
    time_kernels(a, res)
    if a.train_steps > 0:
        time_train_step(a, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
