"""``UNet1d(attn_cond_channels=M1)``, M1 > 1: the MS1 conditioning as the ``(B, RT, M1)`` slices the reference's data generator writes
(DESIGN.md section 20).  The reference folds them to ``(B, M1, RT)`` in front of ``attn_cond_proj`` (unet1d.py:1122-1130); here
k_ms1_feat.hip reads the layout as it is.

Without a GPU: the plan / C ABI, the float64 reference (oracle/dq_oracle.py with ``ms1_features`` replaced by the transcription of those lines)
pinned against tests/golden/ms1_channels.npz -- captured from the reference by tools/make_golden_ms1_channels.py --, the default initialisation
and the synthetic data.  On the GPU: the two kernels alone against float64, the whole net against the fixture, train steps and sampling against
that float64 reference, and the end-to-end command.

Bounds of the stand-alone kernels (fp32, -ffp-contract=off: a product and its addition round separately), per element
``|out - ref| <= K * 2^-24 * S`` with S = the float64 expression with every term replaced by its absolute value and K = the roundings on the
longest path of the kernel's own add chain + 1 for the comparison:
  * forward u: a lane adds 7 taps x ceil(M1 / 64) chunks in a chain, six additions of the cross-lane tree and the bias follow; a term carries
    the rounding of its product and of the fused normalisation (counted against |w| (|v cm| + |ca|)):  K = 7 ceil(M1 / 64) + 6 + 1 + 2 + 1;
  * GELU: a = 0.5 u (1 + erf(u / sqrt 2)) from the kernel's own u: u / sqrt 2, erff (<= 2 ulp), 1 +, the product, the comparison and one
    spare: K = 8 against S = |u|;
  * weight gradient: a workgroup adds the rows of its units in a chain (<= ceil(units / parts) x (64 + 6) rows), k_wgrad_reduce adds
    ceil(parts / 32) + 1 slots per thread, 16 group sums and the gradient buffer:  K = chain + ceil(parts / 32) + 1 + 16 + 1 + 1 (product) + 1.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

T = torch.from_numpy
U = 2.0 ** -24
KW10 = dict(dim=4, dim_mults=(1, 2, 2, 3), channels=1, conditional=True, init_cond_channels=1, attn_cond_channels=10, downsample_dim=64,
            simple=True)
KW7 = dict(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1, downsample_dim=64, simple=True)
WG_T, WG_MAX_PARTS = 64, 256  # MS1_WG_T / MS1_WG_MAX_PARTS of csrc/dq_kernels.h


def ms1_features_multi(p, ms1):
    """unet1d.py:1122-1130 for a 3-D attn_cond: (B, RT, M1) -> transpose -> Conv1d(M1 -> 8, k7, p3) -> exact GELU -> Conv1d(8 -> 8, k1);
    a 2-D chromatogram as oracle.dq_oracle.ms1_features has it."""
    a = ms1.transpose(1, 2) if ms1.dim() == 3 else ms1[:, None, :]
    a = F.conv1d(a, p["attn_cond_proj.1.0.weight"], p["attn_cond_proj.1.0.bias"], padding=3)
    return F.conv1d(F.gelu(a), p["attn_cond_proj.1.2.weight"], p["attn_cond_proj.1.2.bias"])


@pytest.fixture
def O(monkeypatch):
    from oracle import dq_oracle

    monkeypatch.setattr(dq_oracle, "ms1_features", ms1_features_multi)
    return dq_oracle


@pytest.fixture(scope="module")
def fixture10():
    sys.path.insert(0, REPO)
    from tools.make_golden_ms1_channels import unpack

    z = np.load(os.path.join(REPO, "tests", "golden", "ms1_channels.npz"))
    g = {k: z[k] for k in z.files}
    sd, grads, isum, ihead = unpack(g)
    return g, {k: T(np.array(v)) for k, v in sd.items()}, {k: T(np.array(v)) for k, v in grads.items()}, isum, ihead


def rel_err(a, b):
    b = torch.as_tensor(b)
    return float((a.detach().cpu().double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)


# ------------------------------------------------------------------------------------------------------------ 1. plan (no GPU)
def _plan_rows(lib, plan):
    name = ctypes.create_string_buffer(256)
    off, nd, shp = ctypes.c_int64(), ctypes.c_int(), (ctypes.c_int64 * 4)()
    rows = []
    for i in range(lib.dq_plan_num_params(plan)):
        assert lib.dq_plan_param_info(plan, i, name, 256, ctypes.byref(off), ctypes.byref(nd), shp) == 0
        rows.append((name.value.decode(), int(off.value), tuple(int(shp[k]) for k in range(nd.value))))
    return rows


@pytest.mark.parametrize("mults", [(1, 2, 2, 3, 3, 4, 4), (1, 2, 2, 3)])  # register-resident / wide (16-byte aligned) bottleneck
def test_plan_with_ms1_channels(mults):
    from dquartic import _native as N

    lib = N.lib()
    m = (ctypes.c_int * len(mults))(*mults)
    p1, p1x, p10 = lib.dq_plan_create(4, len(mults), m, 64, 1000), lib.dq_plan_create_ex(4, len(mults), m, 64, 1000, 1), lib.dq_plan_create_ex(4, len(mults), m, 64, 1000, 10)
    assert p1 and p1x and p10
    r1, r1x, r10 = _plan_rows(lib, p1), _plan_rows(lib, p1x), _plan_rows(lib, p10)
    assert r1 == r1x and lib.dq_plan_param_floats(p1) == lib.dq_plan_param_floats(p1x)
    assert lib.dq_plan_attn_cond_channels(p1) == 1 and lib.dq_plan_attn_cond_channels(p10) == 10
    assert [n for n, _, _ in r10] == [n for n, _, _ in r1]
    d1, d10 = {n: (o, s) for n, o, s in r1}, {n: (o, s) for n, o, s in r10}
    assert d10["attn_cond_proj.1.0.weight"][1] == (8, 10, 7) and d1["attn_cond_proj.1.0.weight"][1] == (8, 1, 7)
    assert all(d10[n][1] == d1[n][1] for n in d1 if n != "attn_cond_proj.1.0.weight")
    # the total: 8 * 9 * 7 more weights plus the floats skipped in front of 16-byte aligned tensors, found by name
    def gaps(rows):
        out, end = {}, 0
        for n, o, s in rows:
            if o != end:
                out[n] = o - end
            end = o + math.prod(s)
        return out, end
    g1, e1 = gaps(r1)
    g10, e10 = gaps(r10)
    assert e1 == lib.dq_plan_param_floats(p1) and e10 == lib.dq_plan_param_floats(p10)
    assert e10 - e1 == 8 * 9 * 7 + sum(g10.values()) - sum(g1.values())
    wide = mults == (1, 2, 2, 3)
    assert set(g10) | set(g1) <= {n for n in d1 if n.startswith("mid_")} and (wide or not (g1 or g10))
    if wide:  # every bottleneck tensor starts on a 16-byte boundary
        assert all(d10[n][0] % 4 == 0 for n in d10 if n.startswith("mid_"))
    for bad in (0, 4097, -3):
        assert not lib.dq_plan_create_ex(4, len(mults), m, 64, 1000, bad)
        assert b"attn_cond_channels" in lib.dq_last_error()
    assert lib.dq_plan_create_ex(4, len(mults), m, 64, 1000, 4096)
    for B, RT in ((1, 16), (32, 400)):
        for tr in (0, 1):
            assert lib.dq_unet_workspace_bytes(p10, B, RT, tr) >= lib.dq_unet_workspace_bytes(p1, B, RT, tr) > 0
    # the graph sampling path stages the whole (B, RT, M1) conditioning
    p150 = lib.dq_plan_create_ex(4, len(mults), m, 64, 1000, 150)
    assert lib.dq_unet_workspace_bytes(p150, 32, 400, 0) - lib.dq_unet_workspace_bytes(p1, 32, 400, 0) >= 4 * 32 * 400 * 149
    for p in (p1, p1x, p10, p150):
        lib.dq_plan_destroy(p)


# ------------------------------------------------------------------------------------------------------------ 2. float64 reference (no GPU)
def test_float64_reference_against_the_reference_fixture(O, fixture10):
    """tolerances: those of test_oracle_golden.test_whole_net_forward_and_grads (y 2e-5 + 2e-6, gradients 1e-4 + 2e-6, of max(1, max |ref|))"""
    g, sd, grads, _, _ = fixture10

    def close(a, b, rtol=2e-5, atol=2e-6):
        scale = max(1.0, float(b.abs().max()))
        assert a.shape == b.shape
        err = float((a.detach().double() - b.double()).abs().max())
        assert err <= (atol + rtol) * scale, f"max abs err {err:.3e} (scale {scale:.3g})"

    p = {k: v.double().clone().requires_grad_(not k.endswith("freqs")) for k, v in sd.items()}
    x, c2, c1 = (T(g[k]).double().clone().requires_grad_(True) for k in ("x", "init_cond", "attn_cond"))
    assert c1.shape == (1, 16, 10) and p["attn_cond_proj.1.0.weight"].shape == (8, 10, 7)
    y = O.unet_forward(p, O.UNetConfig(dim_mults=(1, 2, 2, 3), downsample_dim=64), x, T(g["t"]), c2, c1, use_rope=False)
    close(y, T(g["y"]))
    (y * T(g["gout"]).double()).sum().backward()
    close(x.grad, T(g["dx"]), rtol=1e-4)
    close(c2.grad, T(g["dinit_cond"]), rtol=1e-4)
    close(c1.grad, T(g["dattn_cond"]), rtol=1e-4)
    assert len(grads) == len(sd) - 1
    for k, v in grads.items():
        close(p[k].grad, v, rtol=1e-4)


def test_state_dict_and_default_init_equal_the_reference(fixture10):
    """keys, shapes, order and -- under the same seed -- the default initialisation (the RNG is consumed in the reference's construction
    order; the k7 conv's fan-in is 7 * M1)"""
    from dquartic.model.unet1d import UNet1d

    _, sd_ref, _, isum, ihead = fixture10
    torch.manual_seed(123)
    net = UNet1d(**KW10)
    sd = net.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in sd_ref.items()]
    for k, v in sd.items():
        n = min(4, v.numel())
        assert np.array_equal(v.reshape(-1)[:n].numpy(), ihead[k][:n]), k
        assert abs(v.double().sum().item() - float(isum[k])) <= 1e-9 * max(1.0, abs(float(isum[k]))), k
    # a checkpoint of an M1 = 10 network reloads; an M1 = 1 network refuses it with torch's shape error
    net.load_state_dict(sd_ref)
    assert torch.equal(net.state_dict()["attn_cond_proj.1.0.weight"], sd_ref["attn_cond_proj.1.0.weight"])
    with pytest.raises(RuntimeError, match="size mismatch"):
        UNet1d(**{**KW10, "attn_cond_channels": 1}).load_state_dict(sd_ref)
    assert UNet1d(**{**KW10, "attn_cond_channels": np.int64(10)}).attn_cond_channels == 10
    for bad in (0, 4097, None, 2.5, True):
        with pytest.raises(NotImplementedError, match="attn_cond_channels"):
            UNet1d(**{**KW10, "attn_cond_channels": bad})


# ------------------------------------------------------------------------------------------------------------ 3. synthetic data (no GPU)
def test_synthetic_ms1_channels():
    from dquartic.utils import synthetic as S

    for i in (0, 5):
        ms2_d, ms1_d = S.make_window(i, 40, 16)              # the unchanged default path
        ms2_n, ms1_n = S.make_window(i, 40, 16, ms1_channels=None)
        ms2_c, ms1_c = S.make_window(i, 40, 16, ms1_channels=10)
        assert ms1_d.shape == (40,) and ms1_c.shape == (40, 10) and ms1_c.dtype == np.float32
        assert np.array_equal(ms2_d, ms2_n) and np.array_equal(ms1_d, ms1_n) and np.array_equal(ms2_d, ms2_c)  # the MS2 draws do not move
        assert np.array_equal(ms1_c, S.make_window(i, 40, 16, ms1_channels=10)[1]) and float(ms1_c.min()) >= 0 and float(ms1_c.max()) > 0
        assert (ms1_c.max(axis=0) > 0).sum() >= 2  # spread over channels
        assert S.make_window(i, 40, 16, ms1_channels=1)[1].shape == (40, 1)
    # the default window is what it was before the option existed: the float32 bit patterns of make_window(0, 8, 4) recorded from the code as
    # it stood without ms1_channels
    w = S.make_window(0, 8, 4)
    MS1_BITS = [1103166828, 1103540649, 1103676591, 1103579097, 1103274004, 1102797543, 1102186298, 1101472075]
    MS2_BITS = [1111466113, 1107834044, 1110767866, 1113523666, 1111906834, 1108158951, 1110885331, 1114015284, 1112079719, 1108268992, 1110589258, 1114046106, 1111974780, 1108181350, 1109937009, 1113638929, 1111609614, 1107935089, 1109033176, 1112870258, 1111022756, 1107573626, 1107997278, 1111843514, 1110264900, 1106965074, 1106571721, 1110662284, 1109391102, 1105954829, 1104536798, 1109413432]
    assert w[1].dtype == np.float32 and w[1].view(np.uint32).tolist() == MS1_BITS
    assert w[0].dtype == np.float32 and w[0].reshape(-1).view(np.uint32).tolist() == MS2_BITS
    assert w[1].shape == (8,) and np.array_equal(S.make_pool(2, 8, 4)[1][0], w[1]) and S.make_pool(2, 8, 4, ms1_channels=3)[1].shape == (2, 8, 3)
    a, b = S.SyntheticDIAMSDataset(6, 24, 8, seed=3, ms1_channels=10), S.SyntheticDIAMSDataset(6, 24, 8, seed=3, ms1_channels=10)
    ia, ib = a[0], b[0]
    assert [tuple(v.shape) for v in ia] == [(24, 8), (24, 10), (24, 8), (24, 10)]
    assert all(torch.equal(u, v) for u, v in zip(ia, ib))
    d0, d1 = S.SyntheticDIAMSDataset(6, 24, 8, seed=3), S.SyntheticDIAMSDataset(6, 24, 8, seed=3, ms1_channels=None)
    assert d0.ms1.shape == (6, 24) and np.array_equal(d0.ms1, d1.ms1) and all(torch.equal(u, v) for u, v in zip(d0[0], d1[0]))
    with pytest.raises(ValueError):
        S.make_window(0, 8, 4, ms1_channels=0)


# ------------------------------------------------------------------------------------------------------------ 4. the kernels alone (GPU)
def _feat_ref(ms1, w, b, cm, ca):
    """float64: u, S (the sum of absolute terms) and the fp32-normalised conditioning the kernel hands to the weight gradient"""
    n64 = ms1.double() * cm + ca
    u = F.conv1d(n64.transpose(1, 2), w.double(), b.double(), padding=3)
    nabs = ms1.double().abs() * abs(cm) + abs(ca)
    S = F.conv1d(nabs.transpose(1, 2), w.double().abs(), b.double().abs(), padding=3)
    return u, S


@pytest.mark.gpu
@pytest.mark.parametrize("RT", [1, 3, 7, 34, 400])
@pytest.mark.parametrize("M1", [2, 10, 64, 67, 150])
def test_ms1_feat_kernels_against_float64(M1, RT):
    from dquartic import _native as N

    lib = N.lib()
    gen = torch.Generator().manual_seed(1000 * M1 + RT)
    worst = {"u": 0.0, "a": 0.0, "dw": 0.0, "db": 0.0}
    for B in (1, 3, 32):
        for cm, ca in ((2.0, -1.0), (1.0, 0.0)):
            ms1 = torch.rand(B, RT, M1, generator=gen) * 3 + 0.5  # away from zero: padding the RAW tensor (then n(0) = ca) would show
            w, b = torch.randn(8, M1, 7, generator=gen) / math.sqrt(7 * M1), torch.randn(8, generator=gen)
            du = torch.randn(B, 8, RT, generator=gen)
            d = lambda v: v.cuda().contiguous()
            ms1_d, w_d, b_d, du_d = d(ms1), d(w), d(b), d(du)
            n_d, u_d, a_d = torch.full((B, RT, M1), float("nan"), device="cuda"), torch.empty(B, 8, RT, device="cuda"), torch.empty(B, 8, RT, device="cuda")
            N.check(lib.dq_ms1_feat_fwd(N.ptr(ms1_d), N.ptr(w_d), N.ptr(b_d), cm, ca, N.ptr(n_d), N.ptr(u_d), N.ptr(a_d), B, RT, M1, N.stream_ptr()), "dq_ms1_feat_fwd")
            a2 = torch.empty_like(a_d)  # inference form: nothing saved, the same activations
            N.check(lib.dq_ms1_feat_fwd(N.ptr(ms1_d), N.ptr(w_d), N.ptr(b_d), cm, ca, None, None, N.ptr(a2), B, RT, M1, N.stream_ptr()), "dq_ms1_feat_fwd")
            assert torch.equal(a2, a_d)
            u64, S = _feat_ref(ms1, w, b, cm, ca)
            K = 7 * math.ceil(M1 / 64) + 6 + 1 + 2 + 1
            e = float(((u_d.cpu().double() - u64).abs() / (K * U * S)).max())
            worst["u"] = max(worst["u"], e)
            assert e <= 1.0, (B, cm, ca, e)
            if ca != 0.0:  # sensitivity: the same sum with the RAW tensor zero-padded (rows outside contribute ca) lies outside the bound
                wrong = F.conv1d(F.pad(ms1.double().transpose(1, 2), (3, 3)) * cm + ca, w.double(), b.double())
                assert float(((wrong - u64).abs() / (K * U * S)).max()) > 100.0
            ug = u_d.cpu().double()
            e = float(((a_d.cpu().double() - F.gelu(ug)).abs() / (8 * U * ug.abs() + 1e-300)).max())
            worst["a"] = max(worst["a"], e)
            assert e <= 1.0, (B, cm, ca, e)
            n32 = n_d.cpu()
            assert float((n32.double() - (ms1.double() * cm + ca)).abs().max()) <= U * (abs(cm) * 3.5 + abs(ca)) * 2  # one rounding of the fused multiply-add
            # weight / bias gradient from the kernel's own normalised copy
            floats = lib.dq_ms1_feat_wgrad_scratch_floats(B, RT, M1)
            slot = 56 * M1 + 8
            assert floats > 0 and floats % slot == 0
            parts, units = floats // slot, B * math.ceil(RT / WG_T)
            assert 1 <= parts <= min(units, WG_MAX_PARTS)
            runs = []
            for _ in range(2):
                dw, db, sc = torch.zeros(8, M1, 7, device="cuda"), torch.zeros(8, device="cuda"), torch.full((floats,), float("nan"), device="cuda")
                N.check(lib.dq_ms1_feat_wgrad(N.ptr(n_d), N.ptr(du_d), N.ptr(dw), N.ptr(db), N.ptr(sc), floats, B, RT, M1, N.stream_ptr()), "dq_ms1_feat_wgrad")
                runs.append((dw.cpu(), db.cpu()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # bit for bit
            npad = F.pad(n32.double(), (0, 0, 3, 3))  # zero rows AFTER the normalisation
            win = torch.stack([npad[:, tap:tap + RT, :] for tap in range(7)], dim=-1)  # (B, RT, M1, 7)
            dw64 = torch.einsum("bcr,brmt->cmt", du.double(), win)
            Sw = torch.einsum("bcr,brmt->cmt", du.double().abs(), win.abs())
            red = math.ceil(parts / 32) + 1 + 16 + 1
            Kw = math.ceil(units / parts) * (WG_T + 6) + red + 1 + 1
            e = float(((runs[0][0].double() - dw64).abs() / (Kw * U * Sw + 1e-300)).max())
            worst["dw"] = max(worst["dw"], e)
            assert e <= 1.0, (B, cm, ca, e)
            Kb = math.ceil(units / parts) * WG_T + red + 1
            e = float(((runs[0][1].double() - du.double().sum((0, 2))).abs() / (Kb * U * du.double().abs().sum((0, 2)))).max())
            worst["db"] = max(worst["db"], e)
            assert e <= 1.0, (B, cm, ca, e)
    print(f"ms1_feat M1={M1} RT={RT}: worst error / bound", worst)


# ------------------------------------------------------------------------------------------------------------ 5. whole net vs the fixture (GPU)
@pytest.mark.gpu
def test_whole_net_against_the_reference_fixture(fixture10):
    """forward, d/dx and all gradients through the autograd bridge at M1 = 10; tolerances of test_whole_net_grads_golden: y 2e-5, dx 1e-4,
    gradients 2e-4 of max(|ref|, 1e-4 x the largest gradient)"""
    from dquartic.model.unet1d import UNet1d

    g, sd, grads, _, _ = fixture10
    net = UNet1d(**KW10)
    net.load_state_dict(sd)
    net = net.cuda()
    net.use_rope = False
    x = T(g["x"]).cuda().requires_grad_()
    y = net(x, T(g["t"]).cuda(), T(g["init_cond"]).cuda(), T(g["attn_cond"]).cuda())
    ey = rel_err(y, g["y"])
    (y * T(g["gout"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    edx = rel_err(x.grad, g["dx"])
    floor = 1e-4 * max(float(v.abs().max()) for v in grads.values())
    named = dict(net.named_parameters())
    worst = ("", 0.0)
    for k, v in grads.items():
        e = float((named[k].grad.cpu() - v).abs().max()) / max(float(v.abs().max()), floor)
        if e > worst[1]:
            worst = (k, e)
    print("whole net M1=10: y", ey, "dx", edx, "worst gradient", worst)
    assert ey < 2e-5 and edx < 1e-4 and worst[1] < 2e-4, (ey, edx, worst)


# ------------------------------------------------------------------------------------------------------------ 6. train step (GPU)
def _net7(M1, seed, perturb=0.05):
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    net = UNet1d(**KW7, attn_cond_channels=M1)
    with torch.no_grad():
        for p in net.parameters():
            if p.requires_grad:
                p.add_(perturb * torch.randn_like(p))
    return net, {k: v.detach().clone().cpu() for k, v in net.state_dict().items()}


def _oracle_train(O, params, x0, c2, c1, t, nz):
    """the float64 reference per sample: loss = mean_b loss_b, gradients accumulated"""
    po = {k: v.double().clone().requires_grad_(not k.endswith("freqs")) for k, v in params.items()}
    od = O.Diffusion(po, O.UNetConfig(downsample_dim=64))
    B, loss = x0.shape[0], 0.0
    for b in range(B):
        lb, _ = od.train_loss(x0[b:b + 1].double(), c2[b:b + 1].double(), c1[b:b + 1].double(), t[b:b + 1], nz[b:b + 1].double())
        (lb / B).backward()
        loss += float(lb.detach()) / B
    return loss, po


def _check_grads(O, net, po, what):
    keys = O.trainable_keys(po)
    gmax = max(float(po[k].grad.abs().max()) for k in keys)
    named = dict(net.named_parameters())
    worst = ("", 0.0)
    for k in keys:
        ref = po[k].grad
        e = float((named[k].grad.cpu().double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-4 * gmax)
        if e > worst[1]:
            worst = (k, e)
    print(what, "worst gradient", worst)
    assert len(keys) == 395 and worst[1] <= 2e-5, (what, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("B,RT,M1", [(4, 34, 10), (32, 400, 150)])
def test_train_step_against_float64(O, B, RT, M1):
    """loss 2e-5, gradients 2e-5 of max(|ref|, 1e-4 x the largest gradient) per tensor (the rule of test_scale_parity.py), through the fused
    step and through the autograd bridge; three fused steps repeat bit for bit"""
    from dquartic.model.model import DDIMDiffusionModel

    MZ = 64
    net, params = _net7(M1, 21 + M1)
    dm = DDIMDiffusionModel(model_class=net.cuda(), device="cuda")
    g = torch.Generator().manual_seed(7 + M1)
    x0, c2, c1 = torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, M1, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[0], t[1] = 0, 999
    nzp = torch.rand(B, RT, MZ, generator=g) * 4 - 1.5  # train_step maps a passed noise 2 n - 1 (model.py:346): both paths see nz
    nz = nzp * 2 - 1
    lo, po = _oracle_train(O, params, x0, c2, c1, t, nz)
    net.train()
    runs = []
    for _ in range(3):
        loss = dm.train_step_fused(x0.cuda(), c2.cuda(), c1.cuda(), t=t.cuda(), noise=nz.cuda())
        runs.append((loss.clone(), net.flat_grads().clone()))
    print(f"fused train step ({B}, {RT}, {MZ}) M1={M1}: loss", float(runs[0][0]), "float64", lo)
    assert abs(float(runs[0][0]) - lo) < 2e-5 * abs(lo)
    _check_grads(O, net, po, "fused")
    assert all(torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) for r in runs[1:])
    net.flat_grads(zero=True)
    loss = dm.train_step(x0.cuda(), ms2_cond=c2.cuda(), ms1_cond=c1.cuda(), noise=nzp.cuda(), t=t.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - lo) < 2e-5 * abs(lo), (float(loss), lo)
    _check_grads(O, net, po, "autograd bridge")


@pytest.mark.gpu
def test_captured_train_step_equals_eager_with_ms1_channels():
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    def make():
        torch.manual_seed(3)
        dm = DDIMDiffusionModel(model_class=UNet1d(**KW7, attn_cond_channels=10).cuda(), device="cuda")
        dm._set_optimizer(1e-3)
        return dm.model, dm

    g = torch.Generator().manual_seed(5)
    B, RT, MZ = 4, 48, 64
    data = [(torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, 10, generator=g).cuda()) for _ in range(4)]
    net_e, dm_e = make()
    torch.manual_seed(11)
    losses_e = []
    for x0, c2, c1 in data:
        loss = dm_e.train_step_fused(x0, c2, c1, zero_grads=True)
        dm_e.optimizer.step_dev()
        losses_e.append(loss.clone())
    net_g, dm_g = make()
    dm_g.enable_train_graph()
    torch.manual_seed(11)
    losses_g = [dm_g._train_one_batch(x0, ms2_cond=c2, ms1_cond=c1, sync=False).clone() for x0, c2, c1 in data]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(losses_g, losses_e))
    assert torch.equal(net_g.flat_params, net_e.flat_params)
    assert torch.equal(dm_g.optimizer._m, dm_e.optimizer._m) and torch.equal(dm_g.optimizer._v, dm_e.optimizer._v)
    dm_g.enable_train_graph(False)


# ------------------------------------------------------------------------------------------------------------ 7. sampling (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("pred_type", ["eps", "x0"])
def test_sampling_with_ms1_channels(O, pred_type):
    """10 steps, M1 = 10, B = 8: per-step eps within 1e-4 (of the step's eps scale) of the float64 reference for every window; graph == eager and windows {0, 7}
    == a re-run of exactly those windows, bit for bit"""
    from dquartic.model.model import DDIMDiffusionModel

    B, RT, MZ, M1, steps = 8, 34, 64, 10, 10
    net, params = _net7(M1, 77)
    dm = DDIMDiffusionModel(model_class=net.cuda(), pred_type=pred_type, device="cuda")
    g = torch.Generator().manual_seed(9)
    xT, c2, c1 = torch.randn(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, M1, generator=g)
    dm.use_graph = False
    out_e, noise_e, traj_x, traj_e = dm.sample(xT.cuda(), ms2_cond=c2.cuda(), ms1_cond=c1.cuda(), num_steps=steps, return_trajectory=True)
    out_p, noise_p = dm.sample(xT.cuda(), ms2_cond=c2.cuda(), ms1_cond=c1.cuda(), num_steps=steps)
    dm.use_graph = True
    out_g, noise_g = dm.sample(xT.cuda(), ms2_cond=c2.cuda(), ms1_cond=c1.cuda(), num_steps=steps)
    assert torch.equal(out_p, out_e) and torch.equal(out_g, out_e) and torch.equal(noise_g, noise_e)
    for use_graph in (False, True):
        dm.use_graph = use_graph
        sel = [0, 7]
        o2, n2 = dm.sample(xT[sel].cuda(), ms2_cond=c2[sel].cuda(), ms1_cond=c1[sel].cuda(), num_steps=steps)
        assert torch.equal(o2, out_e[sel]) and torch.equal(n2, noise_e[sel]), use_graph
    po = {k: v.double() for k, v in params.items()}
    od = O.Diffusion(po, O.UNetConfig(downsample_dim=64), pred_type=pred_type)
    worst = 0.0
    with torch.no_grad():
        for b in range(B):
            tr = []
            s, _ = od.sample(xT[b:b + 1].double(), c2[b:b + 1].double(), c1[b:b + 1].double(), steps, trace=tr)
            for i, (_, _, eps) in enumerate(tr):
                worst = max(worst, rel_err(traj_e[i, b:b + 1], eps))
            assert rel_err(out_e[b:b + 1], s) < 1e-4
    print(f"sampling M1=10 {pred_type}: worst per-step eps error", worst)
    assert worst < 1e-4


# ------------------------------------------------------------------------------------------------------------ 8. end to end, rejections
@pytest.mark.gpu
@pytest.mark.parametrize("resident", [False, True])
def test_cli_train_with_ms1_channels(tmp_path, resident):
    """``dquartic train`` on synthetic (RT, 10) MS1 slices for two epochs, then the checkpoint reloads (and an M1 = 1 network refuses it)"""
    import json

    from click.testing import CliRunner
    from dquartic.cli import cli
    from dquartic.model.unet1d import UNet1d

    cfg_path, ckpt = str(tmp_path / "c.json"), str(tmp_path / "best.ckpt")
    assert CliRunner().invoke(cli, ["generate-config", cfg_path]).exit_code == 0
    cfg = json.load(open(cfg_path))
    cfg["model"]["UNet1d"].update(downsample_dim=64, attn_cond_channels=10)
    cfg["model"].update(num_epochs=2, warmup_epochs=1, checkpoint_path=ckpt, batch_size=4)
    cfg["data"]["synthetic"] = {"n_windows": 8, "RT": 34, "MZ": 64, "ms1_channels": 10}
    cfg["wandb"]["use_wandb"] = False
    cfg["threads"] = 0
    json.dump(cfg, open(cfg_path, "w"))
    r = CliRunner().invoke(cli, ["train"] + (["--resident-dataset"] if resident else []) + [cfg_path])
    assert r.exit_code == 0, (r.output, r.exception)
    assert "Epoch=2" in r.output and os.path.exists(ckpt)
    sd = torch.load(ckpt, map_location="cpu", weights_only=False)["model_state_dict"]
    assert tuple(sd["attn_cond_proj.1.0.weight"].shape) == (8, 10, 7)
    kw = dict(KW7, dim_mults=tuple(cfg["model"]["UNet1d"]["dim_mults"]))
    UNet1d(**kw, attn_cond_channels=10).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="size mismatch"):
        UNet1d(**kw, attn_cond_channels=1).load_state_dict(sd)


@pytest.mark.gpu
def test_rejections_before_any_launch():
    from dquartic.model.model import DDIMDiffusionModel
    from dquartic.model.unet1d import UNet1d

    net = UNet1d(**KW7, attn_cond_channels=10).cuda()
    dm = DDIMDiffusionModel(model_class=net, device="cuda")
    B, RT, MZ = 2, 8, 64
    x, c2 = torch.rand(B, RT, MZ, device="cuda"), torch.rand(B, RT, MZ, device="cuda")
    t = torch.zeros(B, dtype=torch.long, device="cuda")
    for bad in (torch.rand(B, RT, 7, device="cuda"), torch.rand(B, RT, device="cuda"), torch.rand(B, RT + 1, 10, device="cuda")):
        for call in (lambda: net(x, t, c2, bad), lambda: dm.train_step_fused(x, c2, bad), lambda: dm.sample(x, ms2_cond=c2, ms1_cond=bad, num_steps=2),
                     lambda: dm.train_step(x, ms2_cond=c2, ms1_cond=bad)):
            with pytest.raises(ValueError, match="attn_cond"):
                call()
    with pytest.raises(ValueError, match=r"7.*10|10.*7"):
        net(x, t, c2, torch.rand(B, RT, 7, device="cuda"))
    ok = torch.rand(B, RT, 10, device="cuda")
    dm._set_optimizer(1e-3)
    for call in (lambda: dm.train_step_fused(x, c2, ok, ms1_loss_weight=0.5), lambda: dm.train_step(x, ms2_cond=c2, ms1_cond=ok, ms1_loss_weight=0.5),
                 lambda: dm._train_one_batch(x, ms2_cond=c2, ms1_cond=ok, ms1_loss_weight=0.5)):
        with pytest.raises(NotImplementedError, match="ms1_loss_weight"):
            call()
    # the library says the same to a caller of the C ABI
    from dquartic import _native as N

    ws = net.workspace(B, RT, True)
    z = torch.zeros(B, RT, MZ, device="cuda")
    rc = N.lib().dq_train_step(net._plan, N.ptr(net.flat_params), None, N.ptr(dm.alpha_bars.cuda()), N.ptr(z), N.ptr(z), N.ptr(ok), N.ptr(t), N.ptr(z), 1, 0,
                               None, 0.5, N.ptr(net.flat_grads()), N.ptr(torch.zeros((), device="cuda")), N.ptr(ws), ws.numel(), B, RT, N.stream_ptr())
    assert rc != 0 and b"ms1_loss_weight" in N.lib().dq_last_error() and b"attn_cond_channels" in N.lib().dq_last_error()
    # M1 = 1 still takes both the chromatogram and its (B, RT, 1) form
    net1 = UNet1d(**KW7, attn_cond_channels=1).cuda()
    c = torch.rand(B, RT, device="cuda")
    assert torch.equal(net1(x, t, c2, c), net1(x, t, c2, c[..., None]))
