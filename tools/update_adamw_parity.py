#!/usr/bin/env python3
"""Every output of the sampler-update and AdamW entry points, written to an .npz, and the byte-for-byte comparison of two such files.

    DQ_HIP_LIB=<library A> python tools/update_adamw_parity.py dump a.npz
    DQ_HIP_LIB=<library B> python tools/update_adamw_parity.py dump b.npz
    python tools/update_adamw_parity.py compare a.npz b.npz        (exit status 1 when an array differs)

What is dumped: dq_ddim_step, dq_ddim_step_x0, dq_ddim_step_sto and dq_solver_step on caller-supplied tensors; dq_guided_update for the four
kinds x both objectives x (16-byte aligned | every tensor one float off | a count that is no multiple of 4); DDIMDiffusionModel.sample on a
tiny U-Net (dq_ddim_sample) for every update kind, unguided and guided, as the eager loop, the captured step
and with trajectories; the same for a tiny CustomTransformer (dq_tfm_sample); the four AdamW entries over two steps with the scratch
(partial sums and the device variant's scalars) and the norm.  Arrays of more than 65536 elements are kept as the SHA-256 of their bytes.  Inputs come from seeded CPU generators, so two processes see the same ones."""
import hashlib
import os
import sys

import numpy as np

BIG = 1 << 16  # elements above which an array is stored as the digest of its bytes
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    keys = sorted(set(a.files) | set(b.files))
    bad = [k for k in keys if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
           or a[k].tobytes() != b[k].tobytes()]
    for k in bad:
        print("DIFFERS:", k)
    print(f"{len(keys)} arrays, {len(keys) - len(bad)} equal byte for byte, {len(bad)} differ")
    return 1 if bad else 0


def dump(path):
    import torch

    from dquartic import _native as N

    L = N.lib()
    s = N.stream_ptr()
    out = {}

    def keep(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            if t is None:
                continue
            a = t.detach().cpu().numpy().copy()
            if a.size > BIG:  # (kept as the SHA-256 of its bytes: the file stays small, the comparison as decisive)
                a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            out[f"{name}/{i}"] = a

    def gen(seed):
        return torch.Generator().manual_seed(seed)

    def off(t, o):
        """a copy of t on the device that starts o floats off 16 bytes"""
        buf = torch.zeros(t.numel() + 8, device="cuda")
        v = buf[o:o + t.numel()]
        v.copy_(t.reshape(-1))
        assert v.data_ptr() % 16 == 4 * o
        return v

    seed = torch.tensor([20240607], dtype=torch.int64, device="cuda")
    ids = torch.tensor([11, 2 ** 33 + 4, 5], dtype=torch.int64, device="cuda")
    rows = {"mid": [0.8, 0.6, 0.9, 0.43, 0.3], "last": [0.99, 0.14, -1.0, 0.0, 0.0]}  # [sa, sb, sap, sbp | c, sigma]
    srows = {"first": [0.8, 0.6, 0.7, 0.25, 0.0], "2m": [0.8, 0.6, 0.7, 0.35, -0.1], "last": [0.99, 0.14, -1.0, 0.0, 0.0]}  # [sa, sb, cx, c0, c1]

    # ---- the stand-alone updates
    for n in (4, 1028, 1027, 3 * 2048 * 256 + 5, 4 * 2048 * 256 + 8):
        g = gen(n)
        x, e = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
        for rname, row in rows.items():
            coef = torch.tensor(row, device="cuda")
            xp, eo = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
            N.check(L.dq_ddim_step(N.ptr(x), N.ptr(e), N.ptr(xp), N.ptr(coef), n, s), "dq_ddim_step")
            keep(f"ddim_step/{n}/{rname}", xp)
            N.check(L.dq_ddim_step_x0(N.ptr(x), N.ptr(e), N.ptr(xp), N.ptr(eo), N.ptr(coef), n, s), "dq_ddim_step_x0")
            keep(f"ddim_step_x0/{n}/{rname}", xp, eo)
        for rname, row in srows.items():
            coef = torch.tensor(row, device="cuda")
            for pred in (0, 1):
                for clip in (0.0, 0.5):
                    xp, eo, hist = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.full((n,), 0.25, device="cuda")
                    N.check(L.dq_solver_step(N.ptr(x), N.ptr(e), N.ptr(xp), N.ptr(hist), N.ptr(eo), N.ptr(coef), clip, pred, n, s), "dq_solver_step")
                    keep(f"solver_step/{n}/{rname}/{pred}/{clip}", xp, eo, hist)
    for B, per in ((3, 8), (3, 1028), (2, 2048 * 256 * 2 + 4)):
        g = gen(B * per)
        x, e = torch.randn(B * per, generator=g).cuda(), torch.randn(B * per, generator=g).cuda()
        for rname, row in rows.items():
            coef = torch.tensor(row, device="cuda")
            for pred in (0, 1):
                for idp in (None, ids[:B]):
                    xp, eo = torch.zeros(B * per, device="cuda"), torch.zeros(B * per, device="cuda")
                    N.check(L.dq_ddim_step_sto(N.ptr(x), N.ptr(e), N.ptr(xp), N.ptr(eo), N.ptr(coef), N.ptr(idp), N.ptr(seed), 3, pred, B, per, s),
                            "dq_ddim_step_sto")
                    keep(f"ddim_step_sto/{B}x{per}/{rname}/{pred}/{idp is not None}", xp, eo)

    # ---- dq_guided_update: kinds x objectives x (aligned | one float off | count % 4 != 0)
    for kind in range(4):
        table = rows if kind < 2 else srows
        for pred in (0, 1):
            for shape, (B, per, o) in {"aligned": (3, 344, 0), "off": (3, 344, 1), "odd": (3, 343, 0), "sweeps": (2, 2048 * 256 * 2 + 4, 0)}.items():
                g = gen(1000 + B * per)
                n = B * per
                x, c, u = (off(torch.randn(n, generator=g), o) for _ in range(3))
                for rname, row in table.items():
                    coef = torch.tensor(row, device="cuda")
                    xp, xm, eo = (off(torch.zeros(n), o) for _ in range(3))
                    hist = off(torch.full((n,), 0.25), o)
                    N.check(L.dq_guided_update(kind, N.ptr(x), N.ptr(c), N.ptr(u), N.ptr(xp), N.ptr(xm), N.ptr(hist), N.ptr(eo), N.ptr(coef), 3.0,
                                               0.5 if kind >= 2 else 0.0, N.ptr(ids[:B]), N.ptr(seed), 2, pred, B, per, s), "dq_guided_update")
                    keep(f"guided_update/{kind}/{pred}/{shape}/{rname}", xp, xm, eo, hist)

    # ---- the sampling loops: the tiny U-Net of the sampler tests, then a tiny CustomTransformer
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d
    from oracle import dq_oracle_tfm as OT

    kinds = {"reference": dict(), "eta1": dict(eta=1.0, seed=7), "ddim": dict(sampler="ddim"), "ddim_clip": dict(sampler="ddim", clip_x0=0.8),
             "dpmpp_2m": dict(sampler="dpmpp_2m"), "dpmpp_2m_clip": dict(sampler="dpmpp_2m", clip_x0=0.8)}

    def loops(name, dm, xT, c2, c1, guided):
        for kname, kw in kinds.items():
            for w in (None, 3.0) if guided else (None,):
                kw2 = dict(kw) if w is None else dict(kw, guidance_scale=w, null_ms1=0.25)
                for mode in ("eager", "captured", "captured_again", "trajectory"):
                    dm.use_graph = mode.startswith("captured")
                    res = dm.sample(xT, c2, c1, num_steps=4, return_trajectory=mode == "trajectory", **kw2)
                    keep(f"{name}/{kname}/{w}/{mode}", *res)

    for pred in ("eps", "x0"):
        torch.manual_seed(41)
        net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)
        with torch.no_grad():
            for p in net.parameters():
                if p.requires_grad:
                    p.add_(0.3 * torch.randn_like(p))
        dm = DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=20, pred_type=pred, device="cuda")
        net.eval()
        g = gen(17)
        xT, c2, c1 = torch.randn(3, 4, 8, generator=g).cuda(), torch.rand(3, 4, 8, generator=g).cuda(), torch.rand(3, 4, generator=g).cuda()
        loops(f"unet_sample/{pred}", dm, xT, c2, c1, True)
        tf = CustomTransformer(input_dim=64, hidden_dim=32, num_heads=2, num_layers=2)
        tf.load_state_dict(OT.init_params(64, 32, 2, seed=43))
        dm = DDIMDiffusionModel(model_class=DDIMTransformerAdapter(tf).cuda(), num_timesteps=1000, beta_schedule_type="cosine", pred_type=pred,
                                auto_normalize=True, ms1_loss_weight=0.0, device="cuda")
        dm.native_tfm_sampler = True
        g = gen(15)
        xT, c2, c1 = torch.randn(3, 10, 64, generator=g).cuda(), torch.rand(3, 10, 64, generator=g).cuda(), torch.rand(3, 7, generator=g).cuda()
        loops(f"tfm_sample/{pred}", dm, xT, c2, c1, False)

    # ---- the four AdamW entries over two steps
    adam = (0.9, 0.999, 1e-8, 0.01)
    for n in (4099, 1016 * 256 + 1, 4 * 1016 * 256 + 8):
        g = gen(n)
        p0, m0, v0, e0 = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g), (0.1 * torch.randn(n, generator=g)) ** 2, torch.randn(n, generator=g)
        grads = [torch.randn(n, generator=g).cuda() * (30.0 / n ** 0.5) for _ in range(2)]
        for entry in ("dq_adamw_clip_step", "dq_adamw_clip_step_dev", "dq_adamw_clip_ema_step", "dq_adamw_clip_ema_step_dev"):
            p, m, v, e = p0.cuda(), m0.cuda(), v0.cuda(), e0.cuda()
            sc, gn = torch.zeros(1024, device="cuda"), torch.zeros(1, device="cuda")
            lr_dev, step_dev = torch.tensor([1e-3, 0.0], device="cuda"), torch.tensor([9], dtype=torch.int32, device="cuda")
            for k, gr in enumerate(grads):
                scalars = (N.ptr(lr_dev), *adam, N.ptr(step_dev)) if entry.endswith("_dev") else (1e-3, *adam, 10 + k)
                ema = (N.ptr(e), 0.999, 1) if "_ema_" in entry else ()
                N.check(getattr(L, entry)(N.ptr(p), N.ptr(gr), N.ptr(m), N.ptr(v), n, N.ptr(sc), 0.5, 10.0, *scalars, N.ptr(gn), *ema, s), entry)
                keep(f"{entry}/{n}/{k}", p, m, v, e if ema else None, sc, gn, step_dev)

    np.savez(path, **out)
    print(f"{len(out)} arrays written to {path}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.exit(dump(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
