#!/usr/bin/env python3
"""Every output of the q_sample, sample-epilogue and loss entry points (csrc/k_stream.hip), written to an .npz, and the
byte-for-byte comparison of two such files -- tools/update_adamw_parity.py's scheme for the streaming kernels.

    DQ_HIP_LIB=<library A> python tools/stream_parity.py dump a.npz
    DQ_HIP_LIB=<library B> python tools/stream_parity.py dump b.npz
    python tools/stream_parity.py compare a.npz b.npz        (exit status 1 when an array differs)

What is dumped: dq_q_sample at the sizes of tests/test_stream_kernels.py plus one count beyond a sweep of each form, both normalisations;
dq_q_sample_repeats with the noise read and drawn, ids given and null; dq_mse_loss_fwd_bwd / _weighted_ / _v_ (loss, gradient, all 1024
scratch floats) at the tests' sizes plus one beyond a sweep of each form, one tensor a float off 16 bytes, with and without the gradient,
inputs with +-0.0 planted; dq_mse_per_window / _v / _repeats (per-window, loss, every slice double) at the slice and staging edges, weighted
and not, the target read and drawn; dq_eval_step and dq_train_step on a tiny U-Net for the three objectives (the MS1 term at 0 and 0.3);
dq_tfm_eval_step on a tiny CustomTransformer at 1 and 3 repeats; DDIMDiffusionModel.sample with and without auto_normalize (the epilogue).
Arrays of more than 65536 elements are kept as the SHA-256 of their bytes.  Inputs come from seeded CPU generators.

Under the development build (make dev) with DQ_NO_HEAD_LOSS=1 in the environment the eps and v train steps leave the fused head and run
k_mse_fwd_bwd themselves, eps with its partial sums handed to the side stream: the same dump then covers that path."""
import hashlib
import os
import sys

import numpy as np

BIG = 1 << 16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

T_, SLICE = 256, 8192
Q_CASES = [(1, 4), (7, 4), (5, 204), (4, 256), (1, 1028), (257, 4), (1, 2097148), (524287, 4), (3, 699052), (5, 839128),
           (1, 1), (3, 74), (2, 6), (1, 257), (3, 174767), (2, 2048 * 256 * 2 + 4), (1, 2048 * 256 + 3)]


def edge_sizes(V, G, smallest):
    blk, sweep = T_ * V, G * T_ * V
    return [smallest, blk - V, blk, blk + V, sweep - V, sweep + V, 2 * sweep + 333 * V]


MSE_SIZES = edge_sizes(4, 1024, 4) + [n for n in edge_sizes(1, 1024, 1) if n % 4] + [222, 1024 * 256 * 4 + 8, 1024 * 256 + 5]
WMSE_CASES = [(1, 4), (255, 4), (4, 256), (1, 1028), (3, 349524), (262145, 4), (1, 2098484), (7, 299784), (1, 1), (3, 74), (2, 6), (257, 1),
              (7, 74899), (2, 1024 * 256 * 2 + 4), (1, 1024 * 256 + 5)]
LOSS_CASES = [(3, 8), (3, 5)] + WMSE_CASES
PER_EDGES = [1, T_ - 1, T_ + 1, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 333]


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
            if a.size > BIG:
                a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            out[f"{name}/{i}"] = a

    def gen(*seed):
        return torch.Generator().manual_seed(sum(int(v) * k for v, k in zip(seed, (1, 1000003, 10007, 101))) % (2 ** 62))

    def off(t, o=1):
        """a copy of t on the device that starts o floats off 16 bytes"""
        buf = torch.zeros(t.numel() + 8, device="cuda")
        v = buf[o:o + t.numel()]
        v.copy_(t.reshape(-1))
        assert v.data_ptr() % 16 == 4 * o
        return v

    def zeros_planted(t):
        """+0.0 and -0.0 at the front of t, and wherever the two operands of a difference then meet"""
        t = t.clone().reshape(-1)
        k = min(t.numel(), 8)
        t[:k] = torch.tensor([0.0, -0.0, -0.0, 0.0, -0.0, 0.0, 0.0, -0.0])[:k]
        return t

    T = 1000
    ab = torch.cos((torch.arange(T + 1, dtype=torch.float64) / T + 0.008) / 1.008 * np.pi / 2) ** 2
    ab = (ab[1:] / ab[0]).clamp(1e-5, 0.99999).float().cuda()
    lw = (ab / (1 - ab)).contiguous()
    pattern = [T - 1, 0, 500, 0, T - 1, 17, 998, 1]

    def steps(n):
        return torch.tensor([pattern[i % len(pattern)] for i in range(n)], dtype=torch.int64, device="cuda")

    seed = torch.tensor([20240607], dtype=torch.int64, device="cuda")
    ids = torch.tensor([11, 2 ** 33 + 4, 5], dtype=torch.int64, device="cuda")

    # ---- dq_q_sample
    for B, per in Q_CASES:
        g = gen(B, per)
        x0, nz, t = torch.rand(B * per, generator=g).cuda(), torch.randn(B * per, generator=g).cuda(), steps(B)
        for norm in (0, 1):
            xt = torch.full((B * per,), float("nan"), device="cuda")
            N.check(L.dq_q_sample(N.ptr(ab), N.ptr(x0), N.ptr(t), N.ptr(nz), N.ptr(xt), B, per, norm, s), "dq_q_sample")
            keep(f"q_sample/{B}x{per}/{norm}", xt)

    # ---- dq_q_sample_repeats: noise read | drawn, ids given | null
    for R, B in ((1, 1), (1, 3), (3, 2)):
        for per in (4, 8188, 8196):
            g = gen(R, B, per)
            x0, nz, t = torch.rand(B * per, generator=g).cuda(), torch.randn(R * B * per, generator=g).cuda(), steps(R * B)
            for noise in (nz, None):
                for idp in (None, ids[:B]):
                    xt = torch.full((R * B * per,), float("nan"), device="cuda")
                    N.check(L.dq_q_sample_repeats(N.ptr(ab), N.ptr(x0), N.ptr(t), N.ptr(noise), N.ptr(seed), N.ptr(idp), 2, N.ptr(xt), B, R, per, 1, s),
                            "dq_q_sample_repeats")
                    keep(f"q_sample_repeats/{R}x{B}x{per}/{noise is not None}/{idp is not None}", xt)

    # ---- the three fwd_bwd losses: loss, gradient, scratch; aligned | the prediction a float off 16 bytes; gradient given | null
    def fwd_bwd(name, call, n, e, *rest):
        for shape, ev in (("aligned", e), ("off", off(e))):
            for want in (True, False):
                lo, gr, sc = torch.full((1,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda"), torch.zeros(1024, device="cuda")
                call(ev, N.ptr(lo), N.ptr(gr) if want else None, N.ptr(sc))
                keep(f"{name}/{shape}/{want}", lo, gr, sc)

    for n in MSE_SIZES:
        g = gen(n, 1)
        e, z = zeros_planted(torch.randn(n, generator=g)).cuda(), zeros_planted(torch.randn(n, generator=g)).cuda()
        fwd_bwd(f"mse/{n}", lambda ev, lo, gr, sc: N.check(L.dq_mse_loss_fwd_bwd(N.ptr(ev), N.ptr(z), lo, gr, sc, n, s), "dq_mse_loss_fwd_bwd"), n, e)
    for B, per in WMSE_CASES:
        for tm, ta in ((2.0, -1.0), (1.0, 0.0)):
            g = gen(B, per, 2)
            n, t = B * per, steps(B)
            e, z = zeros_planted(torch.randn(n, generator=g)).cuda(), zeros_planted(torch.rand(n, generator=g)).cuda()
            fwd_bwd(f"wmse/{B}x{per}/{tm}", lambda ev, lo, gr, sc: N.check(
                L.dq_mse_loss_weighted_fwd_bwd(N.ptr(ev), N.ptr(z), tm, ta, N.ptr(lw), N.ptr(t), lo, gr, sc, B, per, s), "dq_mse_loss_weighted_fwd_bwd"), n, e)
    for B, per in LOSS_CASES:
        for lwp in (lw, None):
            g = gen(B, per, 3)
            n, t = B * per, steps(B)
            e, x0, nz = (zeros_planted(f(n, generator=g)).cuda() for f in (torch.randn, torch.rand, torch.randn))
            fwd_bwd(f"vmse/{B}x{per}/{lwp is not None}", lambda ev, lo, gr, sc: N.check(
                L.dq_mse_loss_v_fwd_bwd(N.ptr(ev), N.ptr(x0), N.ptr(nz), N.ptr(ab), 2.0, -1.0, N.ptr(lwp), N.ptr(t), lo, gr, sc, B, per, s),
                "dq_mse_loss_v_fwd_bwd"), n, e)

    # ---- the per-window losses: per-window, loss, every slice double
    for per in PER_EDGES:
        for B in (1, 255, 256, 257):
            g = gen(B, per, 4)
            n, t = B * per, steps(B)
            o, x0, nz = (f(n, generator=g).cuda() for f in (torch.randn, torch.rand, torch.randn))
            nsl = L.dq_mse_per_window_scratch_bytes(B, per) // 8
            for lwp in (lw, None):
                pw, lo, sc = torch.full((B,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda"), torch.zeros(nsl, dtype=torch.float64, device="cuda")
                N.check(L.dq_mse_per_window(N.ptr(o), N.ptr(x0), 2.0, -1.0, N.ptr(lwp), N.ptr(t), N.ptr(pw), N.ptr(lo), N.ptr(sc), B, per, s), "dq_mse_per_window")
                keep(f"pw/{B}x{per}/{lwp is not None}", pw, lo, sc)
                sc.zero_()
                N.check(L.dq_mse_per_window_v(N.ptr(o), N.ptr(x0), N.ptr(nz), N.ptr(ab), 2.0, -1.0, N.ptr(lwp), N.ptr(t), N.ptr(pw), N.ptr(lo), N.ptr(sc), B, per, s),
                        "dq_mse_per_window_v")
                keep(f"pw_v/{B}x{per}/{lwp is not None}", pw, lo, sc)
    for per in PER_EDGES:
        for R, B in ((1, 1), (1, 255), (1, 256), (1, 257), (3, 2), (2, 128), (3, 85), (2, 256), (3, 257)):
            g = gen(R, B, per, 5)
            NB, t = R * B, steps(R * B)
            o, x0, nz = torch.randn(NB * per, generator=g).cuda(), torch.rand(B * per, generator=g).cuda(), torch.randn(NB * per, generator=g).cuda()
            nsl = L.dq_mse_per_window_scratch_bytes(NB, per) // 8
            idp = ids[:B] if B <= 3 else None
            for what, target, Bt, tm, ta in (("shared", x0, B, 2.0, -1.0), ("each", nz, NB, 1.0, 0.0), ("drawn", None, NB, 1.0, 0.0)):
                for lwp in (lw, None):
                    pw, lo, sc = torch.full((NB,), float("nan"), device="cuda"), torch.full((R,), float("nan"), device="cuda"), torch.zeros(nsl, dtype=torch.float64, device="cuda")
                    N.check(L.dq_mse_per_window_repeats(N.ptr(o), N.ptr(target), Bt, tm, ta, N.ptr(seed), N.ptr(idp), 2, N.ptr(lwp), N.ptr(t), N.ptr(pw),
                                                        N.ptr(lo), N.ptr(sc), B, R, per, s), "dq_mse_per_window_repeats")
                    keep(f"pw_repeats/{R}x{B}x{per}/{what}/{lwp is not None}", pw, lo, sc)

    # ---- the steps: the tiny U-Net of the sampler tests, a tiny CustomTransformer
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d
    from oracle import dq_oracle_tfm as OT

    for pred in ("eps", "x0", "v_prediction"):
        for auto in (True, False):
            torch.manual_seed(41)
            net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)
            with torch.no_grad():
                for p in net.parameters():
                    if p.requires_grad:
                        p.add_(0.3 * torch.randn_like(p))
            dm = DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=20, pred_type=pred, auto_normalize=auto, device="cuda")
            g = gen(17)
            x0, c2, c1 = torch.rand(3, 4, 8, generator=g).cuda(), torch.rand(3, 4, 8, generator=g).cuda(), torch.rand(3, 4, generator=g).cuda()
            nz, t = torch.randn(3, 4, 8, generator=g).cuda(), torch.tensor([19, 0, 7], device="cuda")
            keep(f"eval_step/{pred}/{auto}", *dm.eval_step(x0, c2, c1, t=t, noise=nz))
            for w in (0.0, 0.3) if pred != "v_prediction" else (0.0,):
                loss = dm.train_step_fused(x0, c2, c1, t=t, noise=nz, ms1_loss_weight=w)
                keep(f"train_step/{pred}/{auto}/{w}", loss, net.flat_grads())
            if pred == "eps":
                net.eval()
                dm.use_graph = False
                keep(f"sample/{auto}", *dm.sample(nz, c2, c1, num_steps=3))
    for pred in ("eps", "x0"):
        tf = CustomTransformer(input_dim=64, hidden_dim=32, num_heads=2, num_layers=2)
        tf.load_state_dict(OT.init_params(64, 32, 2, seed=43))
        dm = DDIMDiffusionModel(model_class=DDIMTransformerAdapter(tf).cuda(), num_timesteps=1000, beta_schedule_type="cosine", pred_type=pred,
                                auto_normalize=True, ms1_loss_weight=0.0, device="cuda")
        g = gen(15)
        x0, c1 = torch.rand(3, 10, 64, generator=g).cuda(), torch.rand(3, 7, generator=g).cuda()
        for R in (1, 3):
            t, nz = steps(R * 3).reshape(R, 3), torch.randn(R, 3, 10, 64, generator=g).cuda()
            keep(f"tfm_eval_step/{pred}/{R}/read", *dm._eval_steps_tfm(x0, c1, t, noise=nz))
            keep(f"tfm_eval_step/{pred}/{R}/drawn", *dm.eval_steps(x0, None, c1, t, seed, ids, first_draw=1))

    np.savez(path, **out)
    print(f"{len(out)} arrays written to {path}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.exit(dump(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
