"""Every kind of LevelPlan (csrc/dq_unet.hip: which launch takes each U-Net level, decided once per pass) against the oracle in float64.

The rest of the suite builds three shapes of ``dim_mults`` which all plan alike (kernel levels, the four tiny levels at the bottom, the fused
head).  The six networks here are chosen by reading the predicates level_plan() asks (level_fwd_usable / level_cp_built, tiny_fwd_usable,
tiny_bwd_ok, the LEVEL_IMG_MAX / LA_PREP_MAX / LEVEL_LOSS_PARTS limits), one per corner the walk of the two passes can reach:

  A  (1,2,2,3,3,4,4) MZ 64   the control: all fused, four tiny levels, tiny backward on both sides
  B  (1,3,3,4,4)     MZ 16   unfused -> tiny going down (4 -> 12 channels is no built stage), tiny -> kernel going up, kernel -> unfused -> head
  C  (1,2,4)         MZ 4    rows of ONE position in k_level_fwd (no tiny shape matches), the bottleneck folded by the stand-alone kernels
  D  (4,4)           MZ 2    a tiny up level (LinearAttention + folded input + the Upsample transpose in k_tiny_bwd) whose neighbours are an
                             unfused down twin and a kernel level; the final block unfused: no fused head at all
  E  (1,)*10         MZ 512  rows of 512 .. 128 positions stay unfused; 21 launches: no operand-image slot; 20 LinearAttention layers: no
                             prepare slot (and a 4-channel, wide bottleneck)
  F  (1,2)           MZ 8    at B = 2049 the fused head without the fused loss (4 B partial sums > LEVEL_LOSS_PARTS)

``test_plan_*`` pin the plan the library reports (dq_debug_level_plan: the function the passes call, no device needed); the gpu test runs
one train step, one inference forward and a 3-step deterministic sampling pass per case and compares loss, eps, every gradient tensor
and the samples with the float64 oracle, at the bounds the default network is held to elsewhere in tests/.  The oracle's own
fp32-versus-float64 distance is checked (CPU) to stay under half of each bound, so the bounds have room for a correct fp32 kernel."""
import ctypes
import functools

import pytest
import torch

DEFAULT = (1, 2, 2, 3, 3, 4, 4)
K, U, T = "kernel", "unfused", "tiny"
_KIND = {"K": K, "U": U, "T": T}

# the "must produce" column, re-derived from the predicates (dims = [4] + [4 m]; down level lv: C = dims[lv], stage from dims[lv-1],
# n = MZ >> lv; up level ui, lv = L-1-ui: C = dims[lv+1], skip dims[lv], stage from dims[lv+2]; final block: C = 4 behind a conv from dims[1]).
# dn / up: one letter per launch (up: the L levels, then the final ResnetBlock); flags: those that are TRUE with (save, twin) = (1, 1)
CONFIGS = {
    "A": dict(mults=DEFAULT, mz=64, dn="KKKKKTT", up="TTKKKKK" + "K",
              flags={"prep_ok", "init_fused", "head_shape", "head_train", "use_tb_up", "use_tb_dn", "tb_up_w"}),
    "B": dict(mults=(1, 3, 3, 4, 4), mz=16, dn="KKUTT", up="TTKKU" + "K",
              flags={"prep_ok", "init_fused", "head_shape", "head_train", "use_tb_up", "use_tb_dn", "tb_up_w"}),
    "C": dict(mults=(1, 2, 4), mz=4, dn="KKK", up="KUK" + "K", flags={"prep_ok", "init_fused", "head_shape", "head_train"}),
    "D": dict(mults=(4, 4), mz=2, dn="KU", up="TK" + "U", flags={"prep_ok", "init_fused", "use_tb_up", "tb_up_w"}),
    "E": dict(mults=(1,) * 10, mz=512, dn="UUUKKKKKKK", up="KKKKKKKUUU" + "U", flags=set()),
    "F": dict(mults=(1, 2), mz=8, dn="KK", up="KK" + "K", flags={"prep_ok", "init_fused", "head_shape", "head_train"}),
}
# (head_train: the final block's launch is KERNEL behind the last level's k3 conv from 4 channels -- A, B, C, F -- and 4 B <= LEVEL_LOSS_PARTS)
SAVE_ONLY = {"head_train", "use_tb_up", "use_tb_dn", "tb_up_w"}  # decided for a pass that keeps what the backward needs
LEVEL_LOSS_PARTS = 8192  # csrc/dq_kernels.h

# (config, B, RT) of the numeric cases.  RT = 37: every 32-row and 64-row tile is partial, rows unaligned; RT = 130: three 64-row tiles per
# sample, the last one partial (B and D: the configs whose tiny levels have non-tiny neighbours); F: both sides of the loss-partials limit
CASES = [("A", 3, 37), ("B", 3, 37), ("C", 3, 37), ("D", 3, 37), ("E", 3, 37), ("B", 2, 130), ("D", 2, 130), ("F", 2049, 2), ("F", 3, 2)]
CASE_IDS = [f"{c}-B{b}-RT{rt}" for c, b, rt in CASES]
STEPS = 3
# what the project holds its default network to against the oracle (test_hip_backward.py, test_generic_config.py, test_tiny_levels.py)
TOL = {"loss": 2e-5, "eps": 5e-5, "grad": 2e-4, "sample": 2e-5 * STEPS}


def _make_plan(cfg):
    from dquartic import _native as N

    m = CONFIGS[cfg]["mults"]
    plan = N.lib().dq_plan_create(4, len(m), (ctypes.c_int * len(m))(*m), CONFIGS[cfg]["mz"], 1000)
    assert plan, N.lib().dq_last_error()
    return plan


def _expected(cfg, B, save):
    """(dn kinds, up kinds, flags) of the table for a pass over B windows"""
    c = CONFIGS[cfg]
    flags = set(c["flags"])
    if 4 * B > LEVEL_LOSS_PARTS:
        flags.discard("head_train")
    if not save:
        flags -= SAVE_ONLY
    return [_KIND[k] for k in c["dn"]], [_KIND[k] for k in c["up"]], flags


def _assert_table(cfg, lp, B, save):
    from dquartic import _native as N

    dn, up, flags = _expected(cfg, B, save)
    L = len(dn)
    assert lp["levels"] == L
    assert [f["kind"] for f in lp["dn"]] == dn, (cfg, "dn", [f["kind"] for f in lp["dn"]])
    assert [f["kind"] for f in lp["up"]] == up, (cfg, "up", [f["kind"] for f in lp["up"]])
    assert {k for k in N.LEVEL_PLAN_FLAGS if lp[k]} == flags, (cfg, B, save, {k: lp[k] for k in N.LEVEL_PLAN_FLAGS})
    # the n = 1 extras: the last down level (LinearAttention + its k3 conv into the bottleneck's layout) and the first up level
    # (LinearAttention + the bottleneck's layout as input) when they are tiny; nobody else
    for i, f in enumerate(lp["dn"]):
        last_tiny = i == L - 1 and f["kind"] == T
        assert (f["la"], f["post_w"], f["in_folded"]) == (last_tiny, last_tiny, False), (cfg, "dn", i, f)
    for i, f in enumerate(lp["up"]):
        first_tiny = i == 0 and f["kind"] == T
        assert (f["la"], f["post_w"], f["in_folded"]) == (first_tiny, False, first_tiny), (cfg, "up", i, f)
    # operand images: a slot per kernel launch (level on the way down, L + ui on the way up) while all 2 L + 1 launches fit the region
    for i, f in enumerate(lp["dn"] + lp["up"]):
        if f["kind"] == K:
            assert f["img"] == (i if 2 * L + 1 <= 20 else -1), (cfg, i, f)
        elif f["kind"] == U:
            assert f["img"] == -1, (cfg, i, f)
    if cfg == "E":
        assert all(f["img"] == -1 for f in lp["dn"] + lp["up"]) and not lp["prep_ok"] and not lp["init_fused"]
    if cfg == "C":  # rows of one position, and nothing tiny: the stand-alone conv and fold kernels sit around the bottleneck
        assert lp["dn"][2]["resample"] and not lp["dn"][2]["post_w"] and not lp["up"][0]["in_folded"]


def _assert_invariants(lp, save):
    L = lp["levels"]
    dn, up = lp["dn"], lp["up"]
    tiny = [f for f in dn + up if f["kind"] == T]
    assert len(tiny) <= 4 and len({f["img"] for f in tiny}) == len(tiny) and all(0 <= f["img"] < 4 for f in tiny)
    for lv in range(L):
        want = (dn[lv + 1]["kind"] == U) if lv + 1 < L else not dn[lv]["post_w"]
        assert dn[lv]["resample"] == want, ("dn", lv, dn)
    for ui in range(L):
        assert up[ui]["resample"] == (up[ui + 1]["kind"] == U), ("up", ui, up)
    if lp["use_tb_up"]:
        assert up[0]["kind"] == T and save
    if lp["use_tb_dn"]:
        assert dn[L - 1]["kind"] == T and save
    if lp["tb_up_w"]:
        assert lp["use_tb_up"]
    if not save:
        assert not (lp["head_train"] or lp["use_tb_up"] or lp["use_tb_dn"])
    if lp["head_train"]:
        assert lp["head_shape"]
    if lp["head_shape"]:
        assert up[L]["kind"] == K
    if lp["init_fused"]:
        assert dn[0]["kind"] == K
    for f in dn + up:  # the extras belong to tiny launches
        if f["la"] or f["post_w"] or f["in_folded"]:
            assert f["kind"] == T


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_plan_is_the_one_the_predicates_give(cfg):
    """the table above, exactly, for a training pass (save, twin) = (1, 1) and an inference pass (0, 0) at the shapes the numeric cases run"""
    from dquartic import _native as N

    plan = _make_plan(cfg)
    try:
        for c, B, RT in CASES:
            if c != cfg:
                continue
            for save in (1, 0):
                lp = N.level_plan(plan, B, RT, save, save)
                _assert_table(cfg, lp, B, save)
                _assert_invariants(lp, save)
        if cfg == "F":  # the two sides of the limit differ in head_train and in nothing else
            a, b = N.level_plan(plan, 2049, 2, 1, 1), N.level_plan(plan, 3, 2, 1, 1)
            assert a["head_shape"] and not a["head_train"] and b["head_train"]
            assert {k: v for k, v in a.items() if k != "head_train"} == {k: v for k, v in b.items() if k != "head_train"}
            assert N.level_plan(plan, 2048, 2, 1, 1)["head_train"]  # 4 B == LEVEL_LOSS_PARTS still fits
        # a gradient arena without saving does not exist; saving without the arena (dq_unet_fwd's training forward keeps both) plans the
        # levels alike and leaves the loss to its own launch
        lp10 = N.level_plan(plan, 3, 37 if cfg != "F" else 2, 1, 0)
        assert not lp10["head_train"]
        assert [f["kind"] for f in lp10["dn"] + lp10["up"]] == [_KIND[k] for k in CONFIGS[cfg]["dn"] + CONFIGS[cfg]["up"]]
    finally:
        N.lib().dq_plan_destroy(plan)


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_plan_invariants_over_batch_and_window_length(cfg):
    """what unet_forward, unet_backward and unet_prepare rely on, at every (B, RT, save, twin): B = 1100 is past the tiny backward's slot
    reservation, RT = 2 the shortest window a fused launch takes, RT = 130 three 64-row tiles"""
    from dquartic import _native as N

    plan = _make_plan(cfg)
    try:
        for B in (1, 3, 1100):
            for RT in (2, 37, 130):
                for save, twin in ((1, 1), (1, 0), (0, 0)):
                    lp = N.level_plan(plan, B, RT, save, twin)
                    _assert_invariants(lp, save)
                    assert [f["kind"] for f in lp["dn"] + lp["up"]] == [_KIND[k] for k in CONFIGS[cfg]["dn"] + CONFIGS[cfg]["up"]], (B, RT)
                    if B == 1100:  # (test_tiny_levels.py: one LinearAttention slot per workgroup, 1000 at the most)
                        assert not lp["use_tb_up"] and not lp["use_tb_dn"]
    finally:
        N.lib().dq_plan_destroy(plan)


def test_level_plan_call_rejects_bad_arguments():
    from dquartic import _native as N

    plan = _make_plan("B")
    buf = (ctypes.c_int32 * 134)()
    lib = N.lib()
    try:
        need = 1 + 6 * 11 + 7
        assert lib.dq_debug_level_plan(plan, 3, 37, 1, 1, buf, 134) == need
        assert lib.dq_debug_level_plan(plan, 3, 37, 1, 1, buf, need - 1) == -1
        assert lib.dq_debug_level_plan(plan, 0, 37, 1, 1, buf, 134) == -1 and lib.dq_debug_level_plan(plan, 3, 0, 1, 1, buf, 134) == -1
        assert lib.dq_debug_level_plan(None, 3, 37, 1, 1, buf, 134) == -1 and lib.dq_debug_level_plan(plan, 3, 37, 1, 1, None, 134) == -1
    finally:
        lib.dq_plan_destroy(plan)


# ---------------------------------------------------------------------------------------------------------------------------------
# numbers
# ---------------------------------------------------------------------------------------------------------------------------------
def _net(cfg, seed):
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    c = CONFIGS[cfg]
    net = UNet1d(dim=4, channels=1, dim_mults=c["mults"], conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=c["mz"],
                 simple=True)
    with torch.no_grad():
        for _, p in net.trainable_named():
            p.add_(0.05 * torch.randn_like(p))  # biases and gains off their initial 0 and 1
    return net


def _inputs(cfg, B, RT):
    MZ = CONFIGS[cfg]["mz"]
    g = torch.Generator().manual_seed(1000 * B + RT)
    x0, c2, c1 = torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    t = torch.tensor([0, 999, 417] * ((B + 2) // 3), dtype=torch.long)[:B] if B != 2 else torch.tensor([999, 0])
    nz, xT = torch.randn(B, RT, MZ, generator=g), torch.randn(B, RT, MZ, generator=g)
    return x0, c2, c1, t, nz, xT


def _oracle(cfg, B, RT, dtype):
    """loss, eps, per-tensor gradients, the 3-step sample and its predicted noise from oracle.dq_oracle in ``dtype``"""
    from oracle import dq_oracle as O

    c = CONFIGS[cfg]
    sd = {k: v.detach().clone() for k, v in _net(cfg, SEEDS[cfg]).state_dict().items()}
    x0, c2, c1, t, nz, xT = _inputs(cfg, B, RT)
    po = {k: v.to(dtype).requires_grad_(not k.endswith("freqs")) for k, v in sd.items()}
    ocfg = O.UNetConfig(dim_mults=c["mults"], downsample_dim=c["mz"])
    lo, eps = O.Diffusion(po, ocfg).train_loss(x0.to(dtype), c2.to(dtype), c1.to(dtype), t, nz.to(dtype))
    lo.backward()
    grads = {k: po[k].grad.double() for k in O.trainable_keys(po)}
    with torch.no_grad():
        pd = {k: v.detach() for k, v in po.items()}
        xs, pn = O.Diffusion(pd, ocfg).sample(xT.to(dtype), c2.to(dtype), c1.to(dtype), STEPS)
    return {"loss": float(lo.detach()), "eps": eps.detach().double(), "grads": grads, "xs": xs.double(), "pn": pn.double()}


@functools.lru_cache(maxsize=None)
def _reference(cfg, B, RT):
    """the float64 yardstick of a case: computed once per process, shared by the tests below, never written to"""
    return _oracle(cfg, B, RT, torch.float64)


SEEDS = {"A": 3, "B": 5, "C": 7, "D": 11, "E": 13, "F": 17}


def _distances(got, ref):
    """{quantity: (error in the units of TOL, where)}: the loss relative; eps and the samples against the reference's largest entry; every
    gradient tensor against max(its own largest entry, 1e-4 of the largest gradient) -- test_default_net_grads_multiblock_attention's rule"""
    rel = lambda a, b: float((a.double() - b).abs().max()) / float(b.abs().max())
    gmax = max(float(v.abs().max()) for v in ref["grads"].values())
    worst = ("", 0.0)
    for k, r in ref["grads"].items():
        e = float((got["grads"][k].double() - r).abs().max()) / max(float(r.abs().max()), 1e-4 * gmax)
        if not e <= worst[1]:  # (a NaN takes the place and fails the bound)
            worst = (k, e)
    assert set(got["grads"]) == set(ref["grads"])
    return {"loss": (abs(got["loss"] - ref["loss"]) / abs(ref["loss"]), ""), "eps": (rel(got["eps"], ref["eps"]), ""), "grad": (worst[1], worst[0]),
            "sample": (max(rel(got["xs"], ref["xs"]), rel(got["pn"], ref["pn"])), "")}


def _report(tag, d):
    print(f"{tag}: " + "  ".join(f"{k} {e:.2e}/{TOL[k]:.0e}" + (f" ({w})" if w else "") for k, (e, w) in d.items()))


@pytest.mark.parametrize("cfg,B,RT", CASES, ids=CASE_IDS)
def test_bounds_leave_room_for_fp32(cfg, B, RT):
    """the oracle evaluated in fp32 stays within HALF of every bound of its own float64 evaluation, tensor by tensor: the bounds below are
    not at the noise floor of the arithmetic for these seeds (a heavily cancelling gradient would show here, not as a kernel's fault)"""
    d = _distances(_oracle(cfg, B, RT, torch.float32), _reference(cfg, B, RT))
    _report(f"fp32 oracle vs float64 {cfg} B={B} RT={RT}", d)
    for k, (e, w) in d.items():
        assert e < 0.5 * TOL[k], (k, e, w)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,B,RT", CASES, ids=CASE_IDS)
def test_every_plan_against_the_float64_oracle(cfg, B, RT):
    """one fused train step (loss, all gradients), one inference forward (eps) and a 3-step DDIM sampling pass through the launches the plan
    of this (config, B, RT) names, against the float64 oracle.  Prints the plan and the four errors of the case (DESIGN.md section 23 keeps
    the table; its device columns are still to be filled from a first run on an MI355X)"""
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel

    ref = _reference(cfg, B, RT)
    net = _net(cfg, SEEDS[cfg]).cuda()
    for save in (1, 0):  # the plan this case runs: the table's, so no case passes by quietly taking other launches
        lp = N.level_plan(net._plan, B, RT, save, save)
        _assert_table(cfg, lp, B, save)
        _assert_invariants(lp, save)
        print(f"{cfg} B={B} RT={RT} save={save}: dn {' '.join(f['kind'][0].upper() for f in lp['dn'])} | up "
              f"{' '.join(f['kind'][0].upper() for f in lp['up'])} | " + " ".join(k for k in N.LEVEL_PLAN_FLAGS if lp[k]))
    dm = DDIMDiffusionModel(model_class=net, device="cuda")
    x0, c2, c1, t, nz, xT = (v.cuda() for v in _inputs(cfg, B, RT))
    net.eval()
    with torch.no_grad():
        eps = net(dm.q_sample(dm.normalize(x0), t, nz), t, dm.normalize(c2), dm.normalize(c1))
    net.train()
    loss = dm.train_step_fused(x0, c2, c1, t=t, noise=nz, zero_grads=True)
    grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.requires_grad}
    net.eval()
    xs, pn = dm.sample(xT, c2, c1, num_steps=STEPS)
    torch.cuda.synchronize()
    d = _distances({"loss": float(loss), "eps": eps.cpu(), "grads": grads, "xs": xs.cpu(), "pn": pn.cpu()}, ref)
    _report(f"gpu vs float64 {cfg} B={B} RT={RT}", d)
    for k, (e, w) in d.items():
        assert e < TOL[k], (k, e, w)
