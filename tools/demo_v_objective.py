"""Training demonstration of DESIGN.md section 35 (a report of one run each, not a gate): the default network on the synthetic dataset, the
same seed and number of optimiser steps for pred_type "eps" and "v_prediction" through ``dm.train``, then ``evaluate(..., num_steps=50)`` on
a frozen held-out set of other windows.  Writes the two result dicts as JSON.

    python tools/demo_v_objective.py --out profiles/v_objective_demo.json

Needs the GPU; it does not fall back."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch
from torch.utils.data import DataLoader

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "diffusion-deconvolution-dia-msms-data_amd"))

from dquartic.model.model import DDIMDiffusionModel  # noqa: E402
from dquartic.model.unet1d import UNet1d  # noqa: E402
from dquartic.utils.synthetic import FrozenPairDataset, SyntheticDIAMSDataset  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "v_objective_demo.json"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--shape", type=int, nargs=2, default=[64, 64], metavar=("RT", "MZ"))
    ap.add_argument("--lr", type=float, default=1e-3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("demo_v_objective needs the GPU")
    RT, MZ = a.shape
    epochs = a.steps // (a.windows // a.batch)
    out = {"config": {"RT": RT, "MZ": MZ, "train_windows": a.windows, "batch": a.batch, "steps": epochs * (a.windows // a.batch), "lr": a.lr, "seed": 0,
                      "held_out_pairs": 32, "sample_steps": 50}}
    for pred in ("eps", "v_prediction"):
        torch.manual_seed(0)
        net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1,
                     downsample_dim=MZ, simple=True).cuda()
        dm = DDIMDiffusionModel(model_class=net, pred_type=pred, device="cuda")
        net.train()
        train = DataLoader(SyntheticDIAMSDataset(n_windows=a.windows, RT=RT, MZ=MZ), batch_size=a.batch, shuffle=False)
        t0 = time.time()
        with tempfile.TemporaryDirectory() as ck:
            dm.train(train, a.batch, epochs, warmup_epochs=0, learning_rate=a.lr, use_wandb=False, checkpoint_path=os.path.join(ck, "best.ckpt"))
        torch.cuda.synchronize()
        held = FrozenPairDataset(SyntheticDIAMSDataset(n_windows=32, RT=RT, MZ=MZ, start=1_000_000), 32)
        res = dm.evaluate(DataLoader(held, batch_size=16, shuffle=False), num_steps=50)
        keep = {k: res[k] for k in ("val_loss", "val_loss_by_t", "sa", "mse", "cosine", "pearson", "n_windows") if k in res}
        keep["train_seconds"] = time.time() - t0
        out[pred] = keep
        print(pred, json.dumps(keep), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, allow_nan=False)
        f.write("\n")


if __name__ == "__main__":
    main()
