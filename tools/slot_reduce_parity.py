#!/usr/bin/env python3
"""Every parameter gradient and every d(scale, shift) that passes through an ordered slot sum (csrc/dq_slots.h, launch_ordered_sum; DESIGN.md
section 42), written to an .npz, and the byte-for-byte comparison of two such files -- the scheme of tools/stream_parity.py, whose compare
this reuses.

    DQ_HIP_LIB=<library A> python tools/slot_reduce_parity.py dump a.npz
    DQ_HIP_LIB=<library B> python tools/slot_reduce_parity.py dump b.npz
    python tools/slot_reduce_parity.py compare a.npz b.npz        (exit status 1 when an array differs)

What is dumped (normal inputs from seeded CPU generators, through the harnesses of tests/test_conv_forms.py, test_res_forms.py and
test_la_forms.py): dq_conv_bwd at 1, 16, 17, 33 and 512 slots (scalar) and 17 (v4), plus one case of k_conv_bwd_wg and of the three-conv
launch inside dq_resblock_bwd; dq_resblock_bwd in the one-launch form at 1 .. 241 slots, 17 workgroups per sample, C = 8 with res_conv;
dq_linattn_bwd in the register form at 1 .. 121 slots and in the long-row form at 1, 17, 113, 129 waves; dq_wide_norm_bwd and dq_wide_sum_b;
dq_tfm_layernorm_bwd, dq_tfm_cond_embed_bwd and dq_tfm_colsum at the sizes of tests/test_tfm_kernels.py; the flat gradient of one
dq_train_step on the 2-level U-Net of the sampler tests (three objectives) and of one CustomTransformer train step."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "diffusion-deconvolution-dia-msms-data_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from stream_parity import compare  # noqa: E402


def dump(path):
    import torch

    import test_conv_forms as TC
    import test_la_forms as TL
    import test_res_forms as TR
    import test_tfm_kernels as TK
    from dquartic import _native as N

    L, s, P = N.lib(), N.stream_ptr(), N.ptr
    out = {}

    def keep(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            if t is not None:
                out[f"{name}/{i}"] = t.detach().cpu().numpy().copy()

    def dev(*shape, seed, f=torch.randn):
        return f(*shape, generator=torch.Generator().manual_seed(seed)).cuda()

    # ---- dq_conv_bwd: [dW | dbias] over a prefill
    convs = [c for c, _, _ in TC.SLOT_EDGES] + [TC._wg_case(TC.DOWN, 8, 4, 16, "rt34"), TC.Case(6, 20, 12, 4, TC.DOWN, 3, 171, 8)]
    for c in convs:
        x, w, gy, pre_x, pre_p = TC.draw(c, "normal", 0)
        cv = TC.Conv(N, c, x, w, gy)
        cv.fill(float("nan"), pre_p)
        cv.run()
        keep(f"conv_bwd/{c}/{cv.forms()}", cv.dp)

    # ---- dq_resblock_bwd: the flat parameter gradient and d(scale, shift); the one-launch form, then two blocks of the channel-parallel form
    res = list(TR.WG_SLOT_EDGES) + [(16, 16, 6, 4, 34, 3), (12, 12, 8, 8, 34, 3)]
    for C, cinA, cinB, n, rps, B in res:
        blk, wd, x, temb, gy = TR._case(N, C, cinA, cinB, n, rps, B=B)
        blk.forward()
        blk.fill("zero")
        gd, dss = blk.backward(gy)
        keep(f"resblock_bwd/{(C, cinA, cinB, n, rps, B)}/{blk.forms()[1]}", torch.cat([g.reshape(-1) for g in gd.values()]), dss)

    # ---- dq_linattn_bwd: the five parameter gradients
    for form, C, n, rows, ws in TL.SLOT_EDGES + [("rows", 16, 4, 34, 0.4), ("register", 12, 2, 40007, 0.4), ("long", 8, 128, 2049, 0.4)]:
        small, rmin = TL.FORCE[form]
        N.set_option("la_small_min_rows", small)
        N.set_option("la_rows_bwd_min_rows", rmin)
        x, w, gy = TL.make_case(C, n, rows, ws)
        la = TL.LA(N, x, w, gy)
        assert la.forms(form != "long")[1] == form
        la.forward()
        _, g = la.backward(store=True)
        keep(f"linattn_bwd/{form}/{C}/{n}/{rows}", *[g[k] for k in TL.KEYS])
    N.set_option("la_small_min_rows", -1)
    N.set_option("la_rows_bwd_min_rows", -1)

    # ---- dq_wide_norm_bwd (d g, d(scale, shift), d bias) and dq_wide_sum_b
    for B, C, RT in ((1, 12, 34), (3, 20, 34), (3, 80, 65), (1, 4, 3)):
        Pp = (RT + 3) // 4 * 4
        u, dy, g = dev(B, C, Pp, seed=B * C), dev(B, C, Pp, seed=B * C + 1), dev(C, seed=B * C + 2)
        u[..., RT:], dy[..., RT:] = 0, 0
        ss, du = dev(B, 2 * C, seed=B * C + 3) * 0.3, torch.empty(B, C, Pp, device="cuda")
        dg, dss, db = dev(C, seed=5), dev(B, 2 * C, seed=6), dev(C, seed=7)
        need = int(L.dq_wide_norm_bwd_scratch_floats(B, C, Pp))
        sc = torch.zeros(need, device="cuda")
        N.check(L.dq_wide_norm_bwd(P(u), P(dy), P(g), P(ss), 2 * C, 1, P(du), P(dg), P(dss), P(db), P(sc), need, B, C, RT, Pp, s), "dq_wide_norm_bwd")
        keep(f"wide_norm_bwd/{B}x{C}x{RT}", dg, dss, db)
    for B in (1, 7, 8, 9, 17):
        for C in (1, 255, 256, 257):
            part, dst = dev(B, C, seed=1000 * B + C), dev(C, seed=B + C)
            N.check(L.dq_wide_sum_b(P(part), B, C, P(dst), s), "dq_wide_sum_b")
            keep(f"wide_sum_b/{B}x{C}", dst)

    # ---- the transformer's column sums, stored and accumulated
    for H, rows, _ in TK.LN_CASES:
        y, st, g, do = dev(rows, H, seed=H + rows), dev(rows, 2, seed=H + rows + 1), dev(H, seed=2), dev(rows, H, seed=H * rows)
        sc = torch.zeros(2 * H * TK.LN_BWD_BLOCKS, device="cuda")
        for acc in (0, 1):
            for adjacent in (True, False):
                dy, dgb = torch.empty(rows, H, device="cuda"), dev(3 * H, seed=9)
                dg, db = dgb[:H], dgb[H:2 * H] if adjacent else dgb[2 * H:]
                N.check(L.dq_tfm_layernorm_bwd(P(y), P(st), P(g), P(do), P(dy), P(dg), P(db), P(sc), sc.numel(), rows, H, acc, s), "dq_tfm_layernorm_bwd")
                keep(f"layernorm_bwd/{H}x{rows}/{acc}/{adjacent}", dg, db)
    for H, rows in TK.COND_CASES:
        B, S = TK.COND_BS[rows]
        dc, xc, w = dev(rows, H, seed=H + rows), dev(rows, seed=rows), dev(H, seed=H)
        sin, cos = dev(S, H // 2, seed=3), dev(S, H // 2, seed=4)
        sc = torch.zeros(2 * H * TK.COND_BLOCKS, device="cuda")
        for acc in (0, 1):
            dw, db = dev(H, seed=5), dev(H, seed=6)
            N.check(L.dq_tfm_cond_embed_bwd(P(dc), P(xc), P(w), P(sin), P(cos), P(dw), P(db), None, P(sc), sc.numel(), B, S, H, acc, s), "dq_tfm_cond_embed_bwd")
            keep(f"cond_embed_bwd/{H}x{rows}/{acc}", dw, db)
    for M in TK.COLSUM_M:
        for Nn in TK.COLSUM_N:
            x, sc = dev(M, Nn + 3, seed=M * Nn), torch.zeros(TK.COLSUM_BLOCKS * Nn, device="cuda")
            for acc in (0, 1):
                o = dev(Nn, seed=8)
                N.check(L.dq_tfm_colsum(P(x), M, Nn, Nn + 3, P(o), P(sc), sc.numel(), acc, s), "dq_tfm_colsum")
                keep(f"colsum/{M}x{Nn}/{acc}", o)

    # ---- whole steps: the 2-level U-Net of the sampler tests, a small CustomTransformer
    from dquartic.model.building_blocks import CustomTransformer, DDIMTransformerAdapter
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d
    from oracle import dq_oracle_tfm as OT

    for pred in ("eps", "x0", "v_prediction"):
        torch.manual_seed(41)
        net = UNet1d(dim=4, channels=1, dim_mults=(1, 2), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=8, simple=True)
        with torch.no_grad():
            for p in net.parameters():
                if p.requires_grad:
                    p.add_(0.3 * torch.randn_like(p))
        dm = DDIMDiffusionModel(model_class=net.cuda(), num_timesteps=20, pred_type=pred, device="cuda")
        g = torch.Generator().manual_seed(17)
        x0, c2, c1 = torch.rand(3, 4, 8, generator=g).cuda(), torch.rand(3, 4, 8, generator=g).cuda(), torch.rand(3, 4, generator=g).cuda()
        nz, t = torch.randn(3, 4, 8, generator=g).cuda(), torch.tensor([19, 0, 7], device="cuda")
        keep(f"train_step/{pred}", dm.train_step_fused(x0, c2, c1, t=t, noise=nz), net.flat_grads())
    tf = CustomTransformer(input_dim=48, hidden_dim=32, num_heads=4, num_layers=2)
    tf.load_state_dict(OT.init_params(48, 32, 2, seed=3))
    net = DDIMTransformerAdapter(tf).cuda()
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=1000, beta_schedule_type="cosine", pred_type="eps", auto_normalize=True, ms1_loss_weight=0.0,
                            device="cuda")
    g = torch.Generator().manual_seed(11)
    x0, c2, c1 = torch.rand(3, 6, 48, generator=g), torch.rand(3, 6, 48, generator=g), torch.rand(3, 6, generator=g)
    nz, t = torch.randn(3, 6, 48, generator=g), torch.tensor([999, 400, 3])
    keep("tfm_train_step", dm.train_step_fused(x0.cuda(), c2.cuda(), c1.cuda(), t=t.cuda(), noise=nz.cuda()), net.flat_grads())

    np.savez(path, **out)
    print(f"{len(out)} arrays written to {path}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.exit(dump(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
