"""The report DESIGN.md section 40 left open: does sampling the precursors of a mixture jointly help?  Trains the small test network
(dim 4, dim_mults (1, 2)) on ``data.mixture``-style windows of the synthetic dataset for a few hundred steps -- target = one component's
contribution n_0 w_0, conditions = the mixture and that component's MS1 -- then scores held-out groups of P members with
``ModelInterface.evaluate_joint`` under ``bound`` and ``sum`` against P independent calls, on one frozen
``ResidentGroupLoader``, and writes every scalar to ``profiles/joint_eval_demo.json``.

    python tools/demo_joint.py --out profiles/joint_eval_demo.json

A report, not a gate: nothing is asserted about which leg wins.  Needs the GPU; it does not fall back."""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd"))

ARRAYS = ("per_window", "cross", "group")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "joint_eval_demo.json"))
    ap.add_argument("--steps", type=int, default=800, help="training steps")
    ap.add_argument("--pred-type", default="x0", choices=["eps", "x0", "v_prediction"], help="training objective")
    ap.add_argument("--sampler", default="ddim", choices=["reference", "ddim", "dpmpp_2m"])
    ap.add_argument("--clip-x0", type=float, default=1.0, help="clamp of every step's x0 estimate (ddim / dpmpp_2m; 0: none)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--shape", type=int, nargs=2, default=[32, 64], metavar=("RT", "MZ"))
    ap.add_argument("--train-windows", type=int, default=256)
    ap.add_argument("--groups", type=int, default=64, help="held-out groups")
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--components", type=int, nargs=2, default=[2, 3], metavar=("KMIN", "KMAX"))
    ap.add_argument("--num-steps", type=int, default=20, help="sampling steps")
    ap.add_argument("--lr", type=float, default=2e-3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("demo_joint needs the GPU")
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d
    from dquartic.utils.data_loader import ResidentGroupLoader, ResidentMixLoader
    from dquartic.utils.synthetic import SyntheticDIAMSDataset

    RT, MZ = a.shape
    mixture = dict(n_components=tuple(a.components), max_ratio_log2=3, scale_target=True)
    train = SyntheticDIAMSDataset(n_windows=a.train_windows, RT=RT, MZ=MZ)
    held_out = SyntheticDIAMSDataset(n_windows=max(a.groups, 16), RT=RT, MZ=MZ, start=a.train_windows)  # windows the training never saw
    torch.manual_seed(0)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=MZ,
                 simple=True).cuda()
    dm = DDIMDiffusionModel(model_class=net, pred_type=a.pred_type, device="cuda")
    dm._prepare_training(a.lr)
    loader = ResidentMixLoader(train, a.batch, seed=1, device="cuda", drop_last=True, **mixture)
    t0, losses, epoch = time.perf_counter(), [], 0
    while len(losses) < a.steps:
        losses += [float(v) for v in dm._train_one_epoch(epoch, loader)]
        epoch += 1
    torch.cuda.synchronize()
    res = {"config": {**vars(a), "out": None}, "device": torch.cuda.get_device_name(0), "build_id": N.build_id(),
           "train": {"steps": len(losses), "seconds": time.perf_counter() - t0, "first_loss": sum(losses[:10]) / 10, "last_loss": sum(losses[-10:]) / 10}}
    for mode in ("bound", "sum"):
        groups = ResidentGroupLoader(held_out, a.batch, a.members, seed=2, frozen_items=a.groups, device="cuda", **mixture)
        r = dm.evaluate_joint(groups, a.num_steps, consistency=mode, independent=True, seed=3, sampler=a.sampler,
                              clip_x0=a.clip_x0 if a.clip_x0 > 0 and a.sampler != "reference" else None)
        r.pop("member_weight")
        for leg in ("joint", "independent"):
            for k in ARRAYS:
                r[leg].pop(k)
        res[mode] = r
        print(json.dumps({mode: {leg: {k: r[leg][k] for k in ("sa", "cosine", "mse", "excess", "unexplained", "id_acc", "leak") if k in r[leg]}
                                 for leg in ("joint", "independent")}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
