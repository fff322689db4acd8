"""Times the held-out loss of one batch of the CustomTransformer two ways at the reference's configuration (input 40000, hidden 1024, 8 heads,
8 layers, 34-row windows), n_t = 4 repeats per window:

  stacked     one dq_tfm_eval_step with noise = NULL: the repeats through one forward, the noise drawn inside the kernels
  per_repeat  the calls that exist without it, n_t times: dq_randn, dq_q_sample, dq_tfm_fwd (inference), dq_mse_per_window

at B = 1, 8 and 32.  Both paths are warmed up per shape, then timed in turn, window after window, in one process, so that a drift of the
machine hits both alike.  A timing window is `iters` back-to-back batches between two device events, the second followed by a synchronise;
`iters` is chosen per path and shape from the warm-up so that a window lasts at least --window seconds.  Reported per path: the median and
the spread (min, max) over the windows as ms per batch and windows per second, the kernel launches of a batch counted from the launch
sequences (every GEMM through the library's own plan: a split product is two launches), and the peak bytes of workspace and temporaries.

    python tools/time_tfm_eval.py --out profiles/tfm_eval.json

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
from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter  # noqa: E402
from dquartic.model.model import DDIMDiffusionModel  # noqa: E402


def gemm_launches(M, Nn, K, batch=1):
    p = N.gemm_plan(M, Nn, K, batch=batch, splits=1 if batch > 1 else 0)
    return sum((2 if part["splits"] > 1 else 1) for part in (p["full"], p["rest"]) if part["ntiles"])


def launches(B, R, S1, S2, D, H, heads, layers, fused):
    """(stacked, per_repeat): kernel launches of one batch, from the launch sequences of dq_tfm_eval_step and of the four calls per repeat"""
    Sk, dh = S1 + S2, H // heads

    def ff(rows):
        return gemm_launches(rows, 4 * H, H) + 1 + gemm_launches(rows, H, 4 * H)  # ff.0, GELU, ff.2

    def attn3(n):
        return gemm_launches(S1, Sk, dh, n * heads) + 1 + gemm_launches(S1, dh, Sk, n * heads)

    def time_mlp(n):
        return 1 + gemm_launches(n, 4 * H, H) + 1 + gemm_launches(n, H, 4 * H)

    n, rows = R * B, R * B * S1
    layer = gemm_launches(rows, H, H) + gemm_launches(S1, 2 * H, H, n) + (1 if fused else attn3(n)) + gemm_launches(rows, H, H) + 1 + ff(rows) + 1
    prologue = 1 + layers * (gemm_launches(S2, 2 * H, H, B) + (1 if R > 1 else 0)) + time_mlp(n)
    stacked = 1 + prologue + gemm_launches(rows, H, D) + 1 + layers * layer + gemm_launches(rows, D, H) + 2
    rows = B * S1
    layer = 1 + gemm_launches(rows, H, H) + gemm_launches(B * Sk, 2 * H, H) + attn3(B) + gemm_launches(rows, H, H) + 1 + ff(rows) + 1
    fwd = time_mlp(B) + gemm_launches(rows, H, D) + 1 + 1 + layers * layer + gemm_launches(rows, D, H)
    return stacked, R * (1 + 1 + fwd + 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "tfm_eval.json"))
    ap.add_argument("--n-t", type=int, default=4)
    ap.add_argument("--windows", type=int, default=7, help="timing windows per path and shape")
    ap.add_argument("--window", type=float, default=0.3, help="least length of a timing window in seconds")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--dims", type=int, nargs=5, default=[40000, 1024, 8, 8, 34], metavar=("D", "H", "HEADS", "LAYERS", "S"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tfm_eval needs the GPU")
    D, H, heads, layers, S = a.dims
    R, T = a.n_t, 1000
    torch.manual_seed(0)
    net = DDIMTransformerAdapter(CustomTransformer(input_dim=D, hidden_dim=H, num_heads=heads, num_layers=layers)).cuda()
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=T, beta_schedule_type="cosine", pred_type="eps", auto_normalize=True, device="cuda")
    tfm, lib = net.transformer, N.lib()
    fused = lib.dq_tfm_attn_form(S, 2 * S, H // heads)
    res = {"config": {"input_dim": D, "hidden_dim": H, "num_heads": heads, "num_layers": layers, "S1": S, "S2": S, "n_t": R, "windows": a.windows,
                      "window_s": a.window}, "device": torch.cuda.get_device_name(0), "build_id": N.build_id(), "attention_form": int(fused),
           "param_bytes": 4 * tfm.flat_params.numel(), "batches": {}}
    per = S * D
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        x0, c1 = torch.rand(B, S, D, generator=g).cuda(), torch.rand(B, S, generator=g).cuda()
        t = torch.randint(0, T, (R, B), generator=g).cuda()
        seed, ids = dm._seed_tensor(1, "cuda"), torch.arange(B, device="cuda")
        noise, x_t = torch.empty(B, S, D, device="cuda"), torch.empty(B, S, D, device="cuda")
        pw_y, loss_y = torch.empty(R, B, device="cuda"), torch.empty(R, device="cuda")
        scratch = torch.empty(lib.dq_mse_per_window_scratch_bytes(B, per), dtype=torch.uint8, device="cuda")
        ab = dm.alpha_bars

        def stacked():
            return dm.eval_steps(x0, None, c1, t, seed, ids)

        def per_repeat():
            c1n = dm.normalize(c1)
            for r in range(R):
                N.check(lib.dq_randn(N.ptr(noise), N.ptr(ids), N.ptr(seed), r, B, per, N.stream_ptr()), "dq_randn")
                N.check(lib.dq_q_sample(N.ptr(ab), N.ptr(x0), N.ptr(t[r]), N.ptr(noise), N.ptr(x_t), B, per, 1, N.stream_ptr()), "dq_q_sample")
                out = tfm._run_fwd(x_t, t[r], c1n, training=False)
                N.check(lib.dq_mse_per_window(N.ptr(out), N.ptr(noise), 1.0, 0.0, None, N.ptr(t[r]), N.ptr(pw_y[r]), N.ptr(loss_y[r:r + 1]),
                                              N.ptr(scratch), B, per, N.stream_ptr()), "dq_mse_per_window")
            return loss_y, pw_y

        paths = {"stacked": stacked, "per_repeat": per_repeat}

        def window(fn, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / iters  # seconds per batch

        iters, times, vals = {}, {k: [] for k in paths}, {}
        with torch.no_grad():
            for k, fn in paths.items():  # warm-up: every shape the timed windows use, then the size of a window
                vals[k] = [v.clone() for v in fn()]
                window(fn, 2)
                iters[k] = max(1, int(a.window / window(fn, 3)) + 1)
            for _ in range(a.windows):
                for k, fn in paths.items():
                    times[k].append(window(fn, iters[k]))
        n_st, n_pr = launches(B, R, S, S, D, H, heads, layers, fused)
        ws_st = lib.dq_tfm_eval_workspace_bytes(tfm._tfm, B, S, S, R)
        ws_pr = lib.dq_tfm_workspace_bytes(tfm._tfm, B, S, S, 0) + 3 * 4 * B * per + scratch.numel()  # + noise, x_t, the network output
        rel = float(((vals["stacked"][1] - vals["per_repeat"][1]).abs() / vals["per_repeat"][1].abs()).max())
        entry = {"per_window_max_rel_diff": rel, "launches": {"stacked": n_st, "per_repeat": n_pr},
                 "peak_workspace_bytes": {"stacked": int(ws_st), "per_repeat": int(ws_pr)}, "iters_per_window": iters}
        for k, v in times.items():
            med = statistics.median(v)
            entry[k] = {"ms_per_batch": 1e3 * med, "ms_per_batch_min_max": [1e3 * min(v), 1e3 * max(v)], "windows_per_s": B / med}
        entry["per_repeat_over_stacked"] = entry["per_repeat"]["ms_per_batch"] / entry["stacked"]["ms_per_batch"]
        res["batches"][str(B)] = entry
        print(json.dumps({"B": B, **{k: [round(entry[k]["ms_per_batch"], 4)] + [round(x, 4) for x in entry[k]["ms_per_batch_min_max"]] for k in paths},
                          "launches": entry["launches"], "per_window_max_rel_diff": rel}), flush=True)
        with open(a.out, "w") as f:  # (after every shape: a later one that fails leaves the earlier results)
            json.dump(res, f, indent=1)
            f.write("\n")
        del x0, noise, x_t
        tfm.drop_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
