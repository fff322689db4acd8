"""The narrow bottleneck alone -- mid_block1, Residual(PreNorm(Attention)), mid_block2 over (B, mid_c, RT) -- launch by launch against the
oracle in float64 (dq_debug_mid_fwd / dq_debug_mid_bwd: mid_forward and mid_backward of csrc/dq_unet.hip on tensors the test chooses).

The 16-channel bottleneck of the default U-Net runs on csrc/k_res_rt.hip, whose four fused forms (<QKV>, <OUT> forward; <PRE>, <OUT>
backward) the rest of the suite reaches only through whole networks, off every tile edge and never with two tiles per wave.  Here:

  A  edges: a wave is a 16-lane tile with 14 own positions (<QKV>, plain forward) or 12 (<OUT> forward, every backward), a workgroup 56
     or 48 positions of one sample.  RT = 1, 2, 3 (one tile, mostly padding), 11/12/13 and 14/15 (one tile full / the second wave's first
     lane), 24/25 and 28/29 (two tiles), 47/48/49 and 56/57 (a workgroup full / the second one's first position), 96/97, 413.  At each the
     `own` mask, the halo lanes, the zero padding, the `inr ? .. : 1.f` fillers of the norm inputs and the positions that count in the
     gain and scale / shift sums are decided differently.  Every case with and without RoPE.
  B  two tiles per wave: a sample gets at most 64 workgroups, so the tile loop runs twice only past RT = 3072 (own 12) / 3584 (own 14).
     3072 and 3073 straddle the first (at 3073 the last workgroup's first wave runs one tile and breaks on the second); 3585: own 14 too.
  C  the unfused narrow branch: 32 channels, two networks (k_rmsnorm_fwd, the GEMM / conv projections, launch_rope2, k_block_bwd with
     add_src).  64 channels are a wide plan (csrc/dq_plan.cpp), which the entries refuse.
  D  structure: nothing the forward writes stays unwritten, inputs untouched, save / no-save, skip_ms1, a sample alone against the batch,
     repeatability, the two schedules of the backward, `+=` into the flat gradient and nothing outside the bottleneck's tensors.

Inputs: mid_in and ms1f standard normal, all channels of ONE position per sample zero, t from {0, 417, 999}, d mid2.out standard normal;
parameters: the default initialisation plus 0.05 x normal noise.  With biases off zero the first norm's input at the zero column is the
bias plus the neighbours' taps: the RMS-norm clamp is NOT reached by this file.  At RT = 1 only sample 0 gets the column (with all
three the input would vanish, and with it the reference of conv1's weight gradient).

RoPE frequencies: the network's table (1 / 10000^(2 i / 16)) up to RT = 130; the dyadic table 2^-i at RT = 413 and in the cases B, for
which position x frequency is exact in fp32.  With the network's table the angle of pair 1 at position 412 is ~130 rad, half an fp32 ulp
of it 8e-6 rad, and the fp32 ORACLE is 4.7e-6 of max|qv| from its float64 self (~2e-5 past RT 3000): above cap / 16 = 3.1e-6, so
test_bounds_leave_room_for_fp32 fails on the reference alone and the angle's rounding, which every fp32 implementation shares, would
be the whole bound.  The dyadic table keeps a distinct frequency per channel pair (a wrong pair index or position still shows).  The
network's own table is therefore not compared with float64 beyond RT 130 here.

Bounds: per tensor max|got - ref| / max|ref| < 16 d_k, d_k = the same distance of the oracle in fp32 from the oracle in float64 for that
tensor and case (one CPU thread, see _yardstick), floored at 2^-24, never above 5e-5 (activations) / 2e-4 (gradients), what the whole
network is held to; the CPU test holds every d_k under cap / 16.  16: the kernels replace IEEE divide, sqrt and exp by hardware
approximations of a few ulp each, about ten times per block, and the attention runs on split-bf16 products (tests/test_attn_split.py
allows those 2 x the fp32 kernels).  RT = 1 makes two references identically zero (softmax over one key: d sim = g - g, so d ms1f and
to_k's gradient vanish); a kernel forms the two g by different sums, so there the bound is absolute: 16 x 2^-24 x the largest entry the
gradient would have with |terms| in place of the terms that cancel (_cancel_scale).

pre_fused needs bb_part_floats >= 64 B 16 and the arena reserves 64 B 4 max(mid_c, 2) floats: no B makes it false for the 16-channel
network (test_mid_forms_tables asks up to B = 100000), so there is no such GPU case.

References: all float64 and fp32 oracle evaluations of the file take 12 s (8 CPU threads), the three cases B most of it: their attention
is evaluated one (sample, head) at a time under checkpointing (4 RT^2 scores several times over under autograd would be gigabytes);
peak resident memory of the CPU part 1.4 GB.  Observed errors and the mutation table: DESIGN.md section 27."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

# name: dim_mults, MZ, seed;  mid_c = 16 / 32 / 32 / 64.  c64 is a WIDE plan (csrc/dq_plan.cpp: everything but 16 and 32 channels runs on
# k_wide.hip since 64 channels moved there), which the two entries refuse: it stays here for that refusal; c32b is a second 32-channel network
# in its place (another depth, so other offsets -- and another 16-byte alignment -- of the projection weights in the flat buffer)
NETS = {"c16": ((1, 2, 4), 4, 7), "c32": ((1, 2), 8, 17), "c32b": ((1, 2, 2), 16, 23), "c64": ((1, 4), 8, 19)}
MID_C = {"c16": 16, "c32": 32, "c32b": 32, "c64": 64}
EDGE_RT = (1, 2, 3, 11, 12, 13, 14, 15, 24, 25, 28, 29, 47, 48, 49, 56, 57, 96, 97)
# (net, B, RT, rope): rope None | "net" (the network's table) | "dyadic" (2^-i)
CASES_A = [("c16", 3, rt, r) for rt in EDGE_RT for r in ("net", None)] + [("c16", 2, 413, "dyadic"), ("c16", 2, 413, None)]
CASES_B = [("c16", 2, 3072, "dyadic"), ("c16", 2, 3073, "dyadic"), ("c16", 1, 3585, "dyadic")]
CASES_C = [(n, 3, rt, "net") for n in ("c32", "c32b") for rt in (1, 13, 37, 130)] + [("c32", 3, 37, None), ("c32b", 3, 37, None)]
ALL_CASES = CASES_A + CASES_B + CASES_C
_id = lambda c: f"{c[0]}-B{c[1]}-RT{c[2]}-{c[3] or 'norope'}"

CAP = {"act": 5e-5, "grad": 2e-4}  # what the project holds the whole network to (tests/test_level_plan.py: eps, gradients)
FACTOR = 16.0
FLOOR = 2.0 ** -24
ACTS = ("mid1", "mid1.u1", "mid1.a1", "mid1.u2", "xn", "qv", "kk", "o", "attn_out", "mid2.u1", "mid2.a1", "mid2.u2", "mid2")
BWD = ("d.o", "d.mid_in", "d.ms1f", "d.ss1", "d.ss2", "d.mid1.u1", "d.mid1.u2", "d.mid2.u1", "d.mid2.u2")
HEADS, DH = 4, 32


# ---------------------------------------------------------------------------------------------------------------------------------
# networks, inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net(name):
    """as tests/test_level_plan.py::_net: default init plus 0.05 x normal noise, so gains and biases are off 1 and 0"""
    from dquartic.model.unet1d import UNet1d

    mults, mz, seed = NETS[name]
    torch.manual_seed(seed)
    net = UNet1d(dim=4, channels=1, dim_mults=mults, conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=mz, simple=True)
    with torch.no_grad():
        for _, p in net.trainable_named():
            p.add_(0.05 * torch.randn_like(p))
    return net


def _mid_names(net):
    """the bottleneck's parameter tensors: mid_block1.*, mid_block2.* except mlp.* (the time embedding's backward forms those), mid_attn.*"""
    return [n for n, _, _ in net._layout if n.split(".")[0] in ("mid_block1", "mid_block2", "mid_attn") and ".mlp." not in n]


def _freqs(rope):
    if rope is None:
        return None
    if rope == "dyadic":
        return 2.0 ** -torch.arange(8, dtype=torch.float32)
    return 1.0 / (10000 ** (torch.arange(0, 16, 2)[:8].float() / 16))


def _inputs(name, B, RT):
    C = MID_C[name]
    g = torch.Generator().manual_seed(100003 * C + 1000 * B + RT)
    mid_in, ms1f, dout = torch.randn(B, C, RT, generator=g), torch.randn(B, 8, RT, generator=g), torch.randn(B, C, RT, generator=g)
    for b in range(B if RT > 1 else 1):  # (RT = 1: sample 0 alone -- a column per sample would make the whole input zero)
        mid_in[b, :, (5 * b + 1) % RT] = 0.0
    t = torch.tensor([0, 417, 999] * ((B + 2) // 3), dtype=torch.long)[:B]
    return mid_in, ms1f, t, dout


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference: oracle.dq_oracle's functions; the ResnetBlock and the attention restated where an intermediate is compared
# ---------------------------------------------------------------------------------------------------------------------------------
def _resnet_taps(p, prefix, x, temb, taps, tag):
    """oracle.resnet_block(p, prefix, x, temb, 1) with ss, u1, a1, u2 kept (test_restated_functions_are_the_oracles: equal bit for bit)"""
    from oracle import dq_oracle as O

    ss = F.linear(F.silu(temb), p[prefix + ".mlp.1.weight"], p[prefix + ".mlp.1.bias"])  # (B, 2 C): [scale | shift], as the kernels keep it
    sc, sh = ss[:, :, None].chunk(2, dim=1)
    u1 = F.conv1d(x, p[prefix + ".block1.proj.weight"], p[prefix + ".block1.proj.bias"], padding=1)
    a1 = F.silu(O.rmsnorm(u1, p[prefix + ".block1.norm.g"]) * (sc + 1) + sh)
    u2 = F.conv1d(a1, p[prefix + ".block2.proj.weight"], p[prefix + ".block2.proj.bias"], padding=1)
    out = F.silu(O.rmsnorm(u2, p[prefix + ".block2.norm.g"])) + x
    taps.update({tag + ".ss": ss, tag + ".u1": u1, tag + ".a1": a1, tag + ".u2": u2, tag: out})
    return out


def _one_head(q, k, v):  # (N, D) each
    return ((q @ k.t()) * (DH ** -0.5)).softmax(dim=-1) @ v


def _attention_taps(p, x, cond, freqs, taps, per_head):
    """oracle.mid_attention with xn, qv (q rotated, v not), kk (rotated), o kept, in the kernels' (B, channels, RT) layouts"""
    from torch.utils.checkpoint import checkpoint

    from oracle import dq_oracle as O

    B, _, n = x.shape
    xn = O.rmsnorm(x, p["mid_attn.fn.norm.g"])
    qv = F.conv1d(xn, p["mid_attn.fn.fn.to_qv.weight"])
    q, v = (t.reshape(B, HEADS, DH, n).transpose(2, 3) for t in qv.chunk(2, dim=1))  # b h n c
    k = F.conv1d(cond, p["mid_attn.fn.fn.to_k.weight"]).reshape(B, HEADS, DH, n).transpose(2, 3)
    if freqs is not None:
        q, k = O.rope_rotate(q, freqs), O.rope_rotate(k, freqs)
    flat = lambda t: t.transpose(2, 3).reshape(B, HEADS * DH, n)
    if per_head:
        out = torch.stack([torch.stack([checkpoint(_one_head, q[b, h], k[b, h], v[b, h], use_reentrant=False) for h in range(HEADS)])
                           for b in range(B)])
    else:
        attn = (torch.einsum("bhid,bhjd->bhij", q, k) * (DH ** -0.5)).softmax(dim=-1)
        out = torch.einsum("bhij,bhjd->bhid", attn, v)
    o = flat(out)
    y = F.conv1d(o, p["mid_attn.fn.fn.to_out.weight"], p["mid_attn.fn.fn.to_out.bias"]) + x
    taps.update({"xn": xn, "qv": torch.cat((flat(q), flat(v)), dim=1), "kk": flat(k), "o": o, "attn_out": y})
    return y


def _cancel_scale(p, taps, d_o, ms1f):
    """RT = 1: the largest entry d ms1f / to_k's gradient could have if the terms of dP - delta (both sum_d d o_d v_d there) did not cancel"""
    B = d_o.shape[0]
    q, v = taps["qv"].chunk(2, dim=1)
    a = (d_o * v).abs().reshape(B, HEADS, DH).sum(-1)  # (B, H): the magnitude of the terms that cancel
    dkk = (a[:, :, None] * q.abs().reshape(B, HEADS, DH) * DH ** -0.5).reshape(B, HEADS * DH)  # (position 0: RoPE is the identity)
    wk = p["mid_attn.fn.fn.to_k.weight"][:, :, 0].abs()
    return {"d.ms1f": float((dkk @ wk).max()), "mid_attn.fn.fn.to_k.weight": float((dkk.t() @ ms1f[:, :, 0].abs()).max())}


def _oracle(name, B, RT, rope, dtype, per_head=None):
    from oracle import dq_oracle as O

    net = _net(name)
    mults, mz, _ = NETS[name]
    names = _mid_names(net)
    p = {k: v.detach().to(dtype) for k, v in net.state_dict().items() if not k.endswith("freqs")}
    for k in names + [f"mid_block{i}.mlp.1.{w}" for i in (1, 2) for w in ("weight", "bias")]:  # (mlp: so that ss carries a gradient)
        p[k].requires_grad_(True)
    mid_in, ms1f, t, dout = _inputs(name, B, RT)
    x, cond = mid_in.to(dtype).requires_grad_(True), ms1f.to(dtype).requires_grad_(True)
    fr = _freqs(rope)
    taps = {}
    temb = O.time_mlp(p, t, O.UNetConfig(dim_mults=mults, downsample_dim=mz))
    m = _resnet_taps(p, "mid_block1", x, temb, taps, "mid1")
    m = _attention_taps(p, m, cond, fr, taps, RT > 3000 if per_head is None else per_head)
    m = _resnet_taps(p, "mid_block2", m, temb, taps, "mid2")
    wrt = [taps["o"], x, cond, taps["mid1.ss"], taps["mid2.ss"], taps["mid1.u1"], taps["mid1.u2"], taps["mid2.u1"], taps["mid2.u2"]]
    gr = torch.autograd.grad(m, wrt + [p[k] for k in names], grad_outputs=dout.to(dtype))
    out = {k: taps[k].detach().double() for k in ACTS}
    out.update({k: g.double() for k, g in zip(BWD, gr)})
    out.update({k: g.double() for k, g in zip(names, gr[len(BWD):])})
    if RT == 1 and dtype == torch.float64:
        out["@cancel"] = _cancel_scale({k: v.detach() for k, v in p.items()}, {k: v.detach() for k, v in taps.items()}, out["d.o"], ms1f.double())
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, B, RT, rope):
    """the float64 yardstick of a case: computed once per process, shared by the tests below, never written to"""
    return _oracle(name, B, RT, rope, torch.float64)


def _kind(k):
    return "act" if k in ACTS else "grad"


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def _yardstick(name, B, RT, rope):
    """{tensor: d_k}: the fp32 oracle's distance from the float64 one, max|.| / max|ref| (a reference that is identically zero: 0)"""
    ref = _reference(name, B, RT, rope)
    # one thread: an fp32 sum over thousands of positions depends on how the CPU library splits it, and d_k is ONE draw of that rounding
    # (the PreNorm gain's gradient at RT = 3585: 1.1e-7 .. 3.5e-7 with 1 .. 16 threads, 6.8e-8 on a 16-thread machine) -- the yardstick has to
    # be the same number wherever the suite runs
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        f32 = _oracle(name, B, RT, rope, torch.float32)
    finally:
        torch.set_num_threads(nt)
    return {k: (_rel(f32[k], r) if float(r.abs().max()) > 0 else 0.0) for k, r in ref.items() if k != "@cancel"}


def _bound(k, d):
    return min(FACTOR * max(d, FLOOR), CAP[_kind(k)])


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restated_functions_are_the_oracles():
    """the tapped ResnetBlock and attention above ARE oracle.resnet_block / oracle.mid_attention (bit for bit in float64), and the attention
    evaluated one (sample, head) at a time is the batched one up to the order of its sums"""
    from oracle import dq_oracle as O

    for name, rope in (("c16", "net"), ("c32b", None)):
        net = _net(name)
        mults, mz, _ = NETS[name]
        p = {k: v.detach().double() for k, v in net.state_dict().items()}
        mid_in, ms1f, t, _ = _inputs(name, 3, 29)
        temb = O.time_mlp(p, t, O.UNetConfig(dim_mults=mults, downsample_dim=mz))
        taps = {}
        a = _resnet_taps(p, "mid_block1", mid_in.double(), temb, taps, "mid1")
        assert torch.equal(a, O.resnet_block(p, "mid_block1", mid_in.double(), temb, 1))
        b = _attention_taps(p, a, ms1f.double(), _freqs(rope), taps, False)
        assert torch.equal(b, O.mid_attention(p, a, ms1f.double(), rope is not None))
        assert torch.equal(_resnet_taps(p, "mid_block2", b, temb, taps, "mid2"), O.resnet_block(p, "mid_block2", b, temb, 1))
    one, batched = _oracle("c16", 3, 29, "net", torch.float64, per_head=True), _reference("c16", 3, 29, "net")
    for k, r in batched.items():
        assert _rel(one[k], r) < 1e-12, k


def test_mid_forms_tables():
    """the 16-channel network reports all three fused forms at every (B, RT) of the cases below (and pre_fused at every B: see the docstring),
    the 32-channel ones none, the 64-channel one is wide; the call refuses what dq_debug_level_plan refuses"""
    from dquartic import _native as N

    lib = N.lib()
    c64 = N.mid_forms(_net("c64")._plan, 3, 37)
    assert c64["wide_mid"] and c64["mid_c"] == 64 and not (c64["qkv_fused"] or c64["out_fused"] or c64["pre_fused"])
    for name in ("c16", "c32", "c32b"):
        plan = _net(name)._plan
        shapes = {(B, RT) for n, B, RT, _ in ALL_CASES if n == name} | {(1, 13), (1, 49), (1, 3073), (3, 3073)}
        for B, RT in sorted(shapes):
            f = N.mid_forms(plan, B, RT)
            fused = name == "c16"
            assert (f["qkv_fused"], f["out_fused"], f["pre_fused"]) == (fused,) * 3, (name, B, RT, f)
            assert (f["wide_mid"], f["mid_c"], f["cond_dim"], f["prep_ok"]) == (False, MID_C[name], 8, True), f
            assert 0 <= f["ss_mid1"] and f["ss_mid1"] + 2 * MID_C[name] <= f["ss_mid2"] and f["ss_mid2"] + 2 * MID_C[name] <= f["ss_total"], f
            assert N.resblock_forms(MID_C[name], 0, MID_C[name], B, RT, 1)[0] == ("rt" if fused else "unfused")
            assert lib.dq_debug_layout(plan, B, RT) == 0
            assert lib.dq_debug_tensor_offset(plan, b"@twin") * 8 == lib.dq_unet_workspace_bytes(plan, B, RT, 1)
    plan = _net("c16")._plan
    for B in (1, 2, 7, 64, 1000, 4097, 100000):
        assert N.mid_forms(plan, B, 34)["pre_fused"], B
    assert lib.dq_debug_layout(None, 3, 37) == -1 and lib.dq_debug_layout(plan, 0, 37) == -1 and lib.dq_debug_layout(plan, 3, 0) == -1
    lib.dq_debug_layout(plan, 3, 37)
    before = lib.dq_debug_tensor_offset(plan, b"@twin")
    N.mid_forms(plan, 5, 99)  # (a query: the plan's layout stays)
    assert lib.dq_debug_tensor_offset(plan, b"@twin") == before
    buf = (ctypes.c_int32 * 16)()
    need = len(N.MID_FORMS_FIELDS)
    assert lib.dq_debug_mid_forms(plan, 3, 37, buf, 16) == need
    assert lib.dq_debug_mid_forms(plan, 3, 37, buf, need - 1) == -1
    assert lib.dq_debug_mid_forms(plan, 0, 37, buf, 16) == -1 and lib.dq_debug_mid_forms(plan, 3, 0, buf, 16) == -1
    assert lib.dq_debug_mid_forms(None, 3, 37, buf, 16) == -1 and lib.dq_debug_mid_forms(plan, 3, 37, None, 16) == -1


def test_mid_entries_refuse_before_any_device_call():
    """null arguments, a short workspace and a wide bottleneck are refused on the host (this test runs without a GPU)"""
    from dquartic import _native as N

    lib = N.lib()
    plan = _net("c16")._plan
    one = ctypes.c_void_p(64)  # never dereferenced: every call below is refused first
    nbytes = lib.dq_unet_workspace_bytes(plan, 3, 37, 1)
    assert lib.dq_debug_mid_fwd(plan, one, None, one, 1, 0, one, nbytes // 2 - 4, 3, 37, None) != 0 and "too small" in N.last_error()
    assert lib.dq_debug_mid_bwd(plan, one, None, one, 0, one, nbytes - 4, 3, 37, None) != 0 and "too small" in N.last_error()
    for args in ((None, one, one, one), (plan, None, one, one), (plan, one, None, one), (plan, one, one, None)):
        assert lib.dq_debug_mid_fwd(args[0], args[1], None, args[2], 1, 0, args[3], nbytes, 3, 37, None) != 0
        assert lib.dq_debug_mid_bwd(args[0], args[1], None, args[2], 0, args[3], nbytes, 3, 37, None) != 0
    assert lib.dq_debug_mid_fwd(plan, one, None, one, 1, 0, one, nbytes, 0, 37, None) != 0
    assert lib.dq_debug_mid_bwd(plan, one, None, one, 0, one, nbytes, 3, 0, None) != 0
    wide, big = _net("c64")._plan, 1 << 40
    assert N.mid_forms(wide, 3, 37)["wide_mid"]
    assert lib.dq_debug_mid_fwd(wide, one, None, one, 1, 0, one, big, 3, 37, None) != 0 and "wide" in N.last_error()
    assert lib.dq_debug_mid_bwd(wide, one, None, one, 0, one, big, 3, 37, None) != 0 and "wide" in N.last_error()


@pytest.mark.parametrize("case", ALL_CASES, ids=_id)
def test_bounds_leave_room_for_fp32(case):
    """the yardstick: the oracle in fp32 against itself in float64, tensor by tensor; 16 d_k stays under the cap for every tensor (a tensor
    whose inputs cancelled too heavily for these seeds would show here, not as a kernel's fault)"""
    d = _yardstick(*case)
    worst = {}
    for k, e in d.items():
        kind = "act" if k in ACTS else "bwd" if k in BWD else "param"
        if e >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (e, k)
    print(f"fp32 oracle vs float64 {_id(case)}: " + "  ".join(f"{k} {e:.2e} ({w})" for k, (e, w) in sorted(worst.items())))
    for k, e in d.items():
        assert e < CAP[_kind(k)] / FACTOR, (k, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
_CHANNELS = {"ms1f": 8, "qv": 2 * HEADS * DH, "kk": HEADS * DH, "o": HEADS * DH}
_WRITTEN = ACTS  # what the forward writes (with save_for_bwd: all of them), besides lse


@functools.lru_cache(maxsize=None)
def _gpu_net(name):
    net = _net(name)
    gpu = type(net)(dim=4, channels=1, dim_mults=NETS[name][0], conditional=True, init_cond_channels=1, attn_cond_channels=1,
                    downsample_dim=NETS[name][1], simple=True)
    gpu.load_state_dict(net.state_dict())
    return gpu.cuda()


class _Bottleneck:
    """a training workspace of one (net, B, RT) with the case's inputs in their slots"""

    def __init__(self, name, B, RT, rope, samples=None):
        from dquartic import _native as N

        self.N, self.lib, self.name, self.B, self.RT = N, N.lib(), name, B, RT
        self.net = _gpu_net(name)
        self.plan, self.C = self.net._plan, MID_C[name]
        self.params = self.net.flat_params
        self.forms = N.mid_forms(self.plan, B, RT)
        assert self.lib.dq_debug_layout(self.plan, B, RT) == 0  # (the offsets below are this shape's)
        fused = name == "c16"
        assert (self.forms["qkv_fused"], self.forms["out_fused"], self.forms["pre_fused"]) == (fused,) * 3, self.forms
        assert N.resblock_forms(self.C, 0, self.C, B, RT, 1)[0] == ("rt" if fused else "unfused")
        names = ("ss", "ms1f", "mid_in", "lse") + ACTS
        self.off = {k: int(self.lib.dq_debug_tensor_offset(self.plan, k.encode())) for k in names}
        assert min(self.off.values()) >= 0, self.off
        self.twin = int(self.lib.dq_debug_tensor_offset(self.plan, b"@twin"))
        self.nbytes = int(self.lib.dq_unet_workspace_bytes(self.plan, B, RT, 1))
        assert self.nbytes == 8 * self.twin
        self.ws = torch.zeros(2 * self.twin, dtype=torch.float32, device="cuda")
        fr = _freqs(rope)
        self.freqs = None if fr is None else fr.cuda()
        mid_in, ms1f, t, dout = _inputs(name, 3 if samples is not None else B, RT)
        if samples is not None:  # one sample of the B = 3 case on its own
            mid_in, ms1f, t, dout = (v[samples].contiguous() for v in (mid_in, ms1f, t, dout))
        self.inputs = tuple(v.cuda() for v in (mid_in, ms1f, t, dout))
        self.t = self.inputs[2]

    def view(self, k, twin=False):
        C = _CHANNELS.get(k, self.C)
        o = self.off[k] + (self.twin if twin else 0)
        return self.ws[o:o + self.B * C * self.RT].view(self.B, C, self.RT)

    def dss(self, which):
        o = self.off["ss"] + self.twin
        v = self.ws[o:o + self.B * self.forms["ss_total"]].view(self.B, self.forms["ss_total"])
        return v[:, self.forms[which]:self.forms[which] + 2 * self.C]

    def fwd(self, save=1, skip_ms1=0):
        """NaN into everything the forward writes (kk: unless it is the prepared input), the inputs into their slots, the call; asserts that
        no NaN is left and that the inputs are untouched"""
        N = self.N
        for k in _WRITTEN:
            if not (skip_ms1 and k == "kk"):
                self.view(k).fill_(float("nan"))
        lse = self.ws[self.off["lse"]:self.off["lse"] + self.B * HEADS * self.RT]
        lse.fill_(float("nan"))
        self.view("mid_in").copy_(self.inputs[0])
        self.view("ms1f").copy_(self.inputs[1])
        N.check(self.lib.dq_debug_mid_fwd(self.plan, N.ptr(self.params), N.ptr(self.freqs), N.ptr(self.t), save, skip_ms1, N.ptr(self.ws),
                                          self.nbytes, self.B, self.RT, N.stream_ptr()), "dq_debug_mid_fwd")
        torch.cuda.synchronize()
        kept = [k for k in _WRITTEN if save or k.count(".") == 0 and k != "xn"]  # (no save: u1 / a1 / u2 / xn are the backward's)
        for k in kept:
            assert not torch.isnan(self.view(k)).any(), (k, "NaN left")
        assert not torch.isnan(lse).any()
        assert torch.equal(self.view("mid_in"), self.inputs[0]) and torch.equal(self.view("ms1f"), self.inputs[1])
        return {k: self.view(k).clone() for k in kept}

    def bwd(self, mode=0, grads=None):
        N = self.N
        if grads is None:
            grads = torch.zeros_like(self.params)
        self.view("mid2", twin=True).copy_(self.inputs[3])
        N.check(self.lib.dq_debug_mid_bwd(self.plan, N.ptr(self.params), N.ptr(self.freqs), N.ptr(grads), mode, N.ptr(self.ws), self.nbytes,
                                          self.B, self.RT, N.stream_ptr()), "dq_debug_mid_bwd")
        torch.cuda.synchronize()
        out = {"d.o": self.view("o", True), "d.mid_in": self.view("mid_in", True), "d.ms1f": self.view("ms1f", True),
               "d.ss1": self.dss("ss_mid1"), "d.ss2": self.dss("ss_mid2"), "d.mid1.u1": self.view("mid1.u1", True),
               "d.mid1.u2": self.view("mid1.u2", True), "d.mid2.u1": self.view("mid2.u1", True), "d.mid2.u2": self.view("mid2.u2", True)}
        out = {k: v.clone() for k, v in out.items()}
        for n, o, shape in self.net._layout:
            if n in _mid_names(self.net):
                out[n] = grads[o:o + torch.Size(shape).numel()].view(shape).clone()
        out["@flat"] = grads
        return out


_WORST = {}  # tensor kind -> (err / d_k, case, tensor): the table of DESIGN.md


def _compare(case, got):
    """every tensor of `got` against the float64 reference at 16 d_k; prints the case's worst err / d_k per kind of tensor"""
    ref, d = _reference(*case), _yardstick(*case)
    fails, worst = [], {}
    for k, r in ref.items():
        if k == "@cancel":
            continue
        g = got[k].detach().cpu().double()
        assert g.shape == r.shape, (k, g.shape, r.shape)
        rmax = float(r.abs().max())
        if rmax == 0.0:  # (RT = 1: see the docstring)
            assert case[2] == 1 and k in ref["@cancel"], (k, "reference identically zero")
            e, bound = float(g.abs().max()) / ref["@cancel"][k], FACTOR * FLOOR
            ratio = e / FLOOR
        else:
            e, bound = float((g - r).abs().max()) / rmax, _bound(k, d[k])
            ratio = e / max(d[k], FLOOR)
        if not e < bound:  # (a NaN fails)
            fails.append((k, e, bound))
        kind = k if k in ACTS + BWD else "d." + k.split(".", 1)[1].replace("fn.fn.", "").replace("fn.", "")
        kind = kind.replace("mid1", "mid*").replace("mid2", "mid*").replace("ss1", "ss*").replace("ss2", "ss*")
        if not ratio <= worst.get(kind, (0.0,))[0]:
            worst[kind] = (ratio, e)
        if not ratio <= _WORST.get(kind, (0.0,))[0]:
            _WORST[kind] = (ratio, e, _id(case), k)
    print(f"gpu vs float64 {_id(case)}  err/d_k (err): " + "  ".join(f"{k} {r:.2f} ({e:.1e})" for k, (r, e) in sorted(worst.items())))
    assert not fails, (_id(case), fails)


def _run_case(case):
    name, B, RT, rope = case
    bn = _Bottleneck(name, B, RT, rope)
    got = bn.fwd()
    got.update(bn.bwd())
    _compare(case, got)
    return bn, got


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_A, ids=_id)
def test_fused_forms_at_tile_edges(case):
    """A: forward and backward of the fused 16-channel bottleneck at every tile edge, every intermediate against float64"""
    _run_case(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_B, ids=_id)
def test_two_tiles_per_wave(case):
    """B: the tile loop's second iteration, its wave-uniform break and the sums that run across tiles"""
    _run_case(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_C, ids=_id)
def test_unfused_narrow_branch(case):
    """C: 32 channels -- none of the fused launches (asserted from dq_debug_mid_forms and dq_resblock_forms in _Bottleneck)"""
    bn, _ = _run_case(case)
    assert not (bn.forms["qkv_fused"] or bn.forms["out_fused"] or bn.forms["pre_fused"])


def _equal(a, b, keys=None):
    for k in (keys or a.keys()):
        if k != "@flat":
            assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("c16", 3, 13, "net"), ("c16", 3, 49, "net"), ("c16", 2, 3073, "dyadic"), ("c32", 3, 37, "net")], ids=_id)
def test_structure_of_the_calls(case):
    """D: (every fwd() already checks: no NaN left in what the forward writes, mid_in and ms1f bit for bit) save_for_bwd = 0 gives the same
    mid2; skip_ms1 with the kk of the full run gives the same qv, o and mid2 and leaves kk alone; a repeated call is bitwise identical, forward
    and backward; the two schedules of the backward agree bit for bit"""
    name, B, RT, rope = case
    bn = _Bottleneck(name, B, RT, rope)
    f1 = bn.fwd()
    b1 = bn.bwd(0)
    f2 = bn.fwd()
    b2 = bn.bwd(0)
    _equal(f1, f2)
    _equal(b1, b2)
    b3 = bn.bwd(1)  # (the forward's saves are still in place: the backward only reads them)
    _equal(b1, b3)
    assert torch.equal(b1["@flat"], b3["@flat"])
    kk = bn.view("kk").clone()
    f3 = bn.fwd(save=1, skip_ms1=1)
    assert torch.equal(bn.view("kk"), kk)
    _equal(f1, f3, ("qv", "o", "mid2", "attn_out", "mid1"))
    f0 = bn.fwd(save=0)
    assert torch.equal(f0["mid2"], f1["mid2"])


@pytest.mark.gpu
@pytest.mark.parametrize("RT,rope", [(13, "net"), (49, "net"), (3073, "dyadic")])
def test_a_sample_alone_is_the_sample_in_the_batch(RT, rope):
    """D: sample b of the B = 3 call equals a B = 1 call on that sample bit for bit: forward tensors, d mid_in, d ms1f, d(scale, shift)"""
    full = _Bottleneck("c16", 3, RT, rope)
    ff = full.fwd()
    fb = full.bwd()
    for b in range(3):
        one = _Bottleneck("c16", 1, RT, rope, samples=slice(b, b + 1))
        of = one.fwd()
        ob = one.bwd()
        for k, v in of.items():
            assert torch.equal(v[0], ff[k][b]), (RT, b, k)
        for k in ("d.mid_in", "d.ms1f", "d.ss1", "d.ss2", "d.o"):
            assert torch.equal(ob[k][0], fb[k][b]), (RT, b, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("c16", 3, 49, "net"), ("c16", 2, 3073, "dyadic"), ("c32b", 3, 37, "net")], ids=_id)
def test_gradients_accumulate_into_the_bottlenecks_tensors_only(case):
    """D: grads prefilled with a pattern: every float outside the bottleneck's tensors, and inside their mlp.* rows, is untouched bit for bit;
    inside, the result is fl(prefill + gradient of a run into zeros) bit for bit: every reduction of the bottleneck's backward forms its sum
    in scratch and ends in ONE `dst += sum`"""
    name, B, RT, rope = case
    bn = _Bottleneck(name, B, RT, rope)
    bn.fwd()
    zero = bn.bwd(0)
    pre = (((torch.arange(bn.params.numel(), device="cuda") % 7) - 3).float() * 0.25)
    got = bn.bwd(0, grads=pre.clone())
    inside = torch.zeros(bn.params.numel(), dtype=torch.bool, device="cuda")
    mid = _mid_names(bn.net)
    for n, o, shape in bn.net._layout:
        if n in mid:
            inside[o:o + torch.Size(shape).numel()] = True
    assert torch.equal(got["@flat"][~inside], pre[~inside])
    g0, g1 = zero["@flat"][inside], got["@flat"][inside]
    assert float(g0.abs().max()) > 0
    assert torch.equal(g1, pre[inside] + g0)


@pytest.mark.gpu
def test_report_worst_ratios():
    """prints the worst err / d_k per kind of tensor over the cases run so far in this process (DESIGN.md keeps the table); asserts nothing
    the case tests have not asserted"""
    for k, (r, e, where, t) in sorted(_WORST.items()):
        print(f"worst err/d_k  {k:28s} {r:8.2f}  (err {e:.2e}, {where}, {t})")
