"""The wide bottleneck (Plan::wide_mid: every bottleneck width but 16 and 32 channels; csrc/k_wide.hip, wide_res_fwd / wide_res_bwd of
csrc/dq_ops.hip, mid_forward_wide / mid_backward_wide of csrc/dq_unet.hip) launch by launch against float64, at its edges.

Kernel level (dq_wide_*: the launchers of k_wide.hip on tensors the test chooses, (B, C, P), P = RT rounded up to a multiple of 4):

  RT   1, 2, 3       the im2col taps fall outside the row; P - RT = 3, 2, 1
       4, 5          P - RT = 0 and 3
       31, 32, 33    k_wnorm_fwd / _bwd_stats: one 32-position block short / full / the second block's first lane
       34            the shipped RT: the second block with two live lanes
       63, 64, 65    k_wnorm_bwd_apply / k_rowsum: the 64-lane loop's one trip short / full / the second trip's first lane
       130           a third trip, a fifth block
  C    4             four of the norm kernels' 8 channel slices stay empty
       8, 64, 80     every slice the same length (1, 8, 10 channels)
       12, 20        ragged slices (2 / 1 and 3 / 2 channels)
  B    1, 3          launch_sum_b over one sample / three; the per-sample scale / shift and its stride

  The product is thinned: every RT at C = 12 and 80 (B = 3), every C at RT = 34 and 65 (B = 3), and B = 1 at C in {4, 12, 80} x RT in
  {3, 34, 130}.  Tensors are views inside larger buffers with guard bands (checked bitwise), inputs are checked untouched, output
  buffers start as NaN, input pad columns hold finite garbage.  Every launch runs twice -- the second time with OTHER garbage in the
  input pads -- and the two results are bitwise equal: repeatable, and no pad column reaches an output.

  The norm's input has three special columns per sample where RT allows (see _special): all channels of one position exactly zero, one
  position scaled by 1e-14 (||u|| < 1e-12: the clamp of F.normalize, where forward and backward are LINEAR in u) and one by 1e-6 (small, not
  clamped).  d loss / d u at a clamped position is ~1e12 times its neighbours', so y and du are measured per position: max over channels of
  |got - ref| over max over channels of |ref| at that (b, t); where the reference is exactly zero the kernel's value has to be.  The sums
  (d g, d scale / shift, d bias, row and sample sums) are measured per tensor, max|got - ref| / max|ref|.

  torch.sqrt has no finite derivative at 0, so the file's _rmsnorm takes the root of 1 where the sum of squares is 0 (and multiplies by 0):
  the same VALUE as oracle.rmsnorm bit for bit (test_restated_references_are_the_oracles), and the derivative F.normalize has there.

Bottleneck level (dq_debug_wide_mid_fwd / _bwd: mid_forward_wide and mid_backward_wide exactly as the passes call them):

  widths 4 (below the 8 slices), 8, 12 and 24 (12: not a multiple of 8), 64, 80; B = 3; RT 1, 3, 4, 33, 34, 65, 130 with and without RoPE at
  12 and 80 channels, RT 34 and 65 at the other widths.  Inputs and parameters as tests/test_mid_forms.py: default initialisation plus 0.05 x
  normal noise, standard-normal mid_in / ms1f / d out, one zero position per sample (RT = 1: sample 0 alone).  The network's RoPE table
  (RT <= 130: see that file's docstring).  Compared: every saved intermediate, the output, d input, d ms1f, both blocks' d(scale, shift),
  d u1 / d u2 of both blocks and every bottleneck parameter gradient.  Structure: NaN against zero prefill of every wide slot (bitwise),
  pads zero, a sample alone against the batch, `+=` into the bottleneck's tensors only, the flat gradient's alignment gaps, the two schedules.

Bounds (the project's rule, tests/test_mid_forms.py / tests/test_level_plan.py): error < 16 d, d = the same distance of the fp32 CPU
reference from the float64 reference for that quantity and case (one CPU thread), floored at 2^-24, never above 5e-5 (activations) / 2e-4
(gradients); test_bounds_leave_room_for_fp32 holds every d under cap / 16 without a GPU.  Measured d, the errors the GPU reaches and the
mutation table: DESIGN.md section 30."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

RMS_EPS = 1e-12
CAP = {"act": 5e-5, "grad": 2e-4}
FACTOR = 16.0
FLOOR = 2.0 ** -24
HEADS, DH = 4, 32
HID = HEADS * DH

ALL_RT = (1, 2, 3, 4, 5, 31, 32, 33, 34, 63, 64, 65, 130)
ALL_C = (4, 8, 12, 20, 64, 80)
# (C, B, RT)
KCASES = ([(C, 3, RT) for C in (12, 80) for RT in ALL_RT] + [(C, 3, RT) for C in (4, 8, 20, 64) for RT in (34, 65)]
          + [(C, 1, RT) for C in (4, 12, 80) for RT in (3, 34, 130)])
_kid = lambda c: f"C{c[0]}-B{c[1]}-RT{c[2]}"


def _P(RT):
    return (RT + 3) // 4 * 4


def test_the_thinned_product_keeps_what_it_must():
    """every RT at C = 12 and 80, every C at RT = 34 and 65, both B, every P - RT"""
    have = set(KCASES)
    assert all(any((C, B, RT) in have for B in (1, 3)) for C in (12, 80) for RT in ALL_RT)
    assert all(any((C, B, RT) in have for B in (1, 3)) for C in ALL_C for RT in (34, 65))
    assert {B for _, B, _ in KCASES} == {1, 3} and {_P(RT) - RT for _, _, RT in KCASES} == {0, 1, 2, 3}
    assert len(have) == len(KCASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel level: inputs and float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def _rmsnorm(x, g):
    """oracle.rmsnorm (the same value bit for bit) with the derivative of F.normalize where a whole column is zero: see the docstring"""
    ssq = (x * x).sum(dim=1, keepdim=True)
    pos = ssq > 0
    nrm = (torch.sqrt(torch.where(pos, ssq, torch.ones_like(ssq))) * pos).clamp_min(RMS_EPS)
    return x / nrm * g * (x.shape[1] ** 0.5)


def _norm_ref(u, g, ss, act, res):
    """k_wnorm_fwd's function: u (B, C, RT), g (C), ss (B, 2 C) = [scale | shift] or None, act 0 / 1 (SiLU), res (B, C, RT) or None; the op
    order of oracle.block behind its conv (test_restated_references_are_the_oracles)"""
    y = _rmsnorm(u, g.view(1, -1, 1))
    if ss is not None:
        sc, sh = ss[:, :, None].chunk(2, dim=1)
        y = y * (sc + 1) + sh
    if act:
        y = F.silu(y)
    return y if res is None else y + res


def _im2col3_ref(x):
    """(B, C, RT) -> (B, 3 C, RT): row 3 c + k holds x[b][c][t + k - 1], zero outside the row"""
    B, C, RT = x.shape
    xp = F.pad(x, (1, 1))
    return torch.stack([xp[..., k:k + RT] for k in range(3)], dim=2).reshape(B, 3 * C, RT)


def _col2im3_ref(d):
    """the transpose: (B, 3 C, RT) -> (B, C, RT), dx[t] = sum_k d[3 c + k][t - k + 1]"""
    B, C3, RT = d.shape
    dp = F.pad(d.view(B, C3 // 3, 3, RT), (1, 1))
    return dp[:, :, 0, 2:RT + 2] + dp[:, :, 1, 1:RT + 1] + dp[:, :, 2, 0:RT]


def _special(B, RT):
    """{(b, t): scale}: per sample up to three special positions, one normal position always left: 0 (exactly zero), 1e-14 (clamped), 1e-6
    (small).  Places: the sample's index, the middle, the end -- so that at RT = 65 / 130 they sit in the second and third 64-lane trip and
    at RT = 33 / 34 in the second 32-position block.  The kinds rotate with the sample.  RT = 1: sample 0 zero, sample 1 clamped, the rest
    normal (a zero column in every sample would make the gain gradient's reference identically zero)"""
    kinds = (0.0, 1e-14, 1e-6)
    if RT == 1:
        return {(b, 0): kinds[b] for b in range(min(B, 2))}
    out = {}
    for b in range(B):
        places = []
        for t in (b % RT, (RT // 2 + b) % RT, RT - 1 - b % RT):
            if t not in places:
                places.append(t)
        for k, t in enumerate(places[:min(3, RT - 1)]):
            out[(b, t)] = kinds[(k + b) % 3]
    return out


@functools.lru_cache(maxsize=None)
def _kin(C, B, RT):
    """the fp32 inputs of a kernel-level case (never written to)"""
    g = torch.Generator().manual_seed(7919 * C + 131 * B + RT)
    r = lambda *s: torch.randn(*s, generator=g)
    u = r(B, C, RT)
    for (b, t), s in _special(B, RT).items():
        u[b, :, t] *= s
    d = {"u": u, "dy": r(B, C, RT), "res": r(B, C, RT), "x": r(B, C, RT), "dxcol": r(B, 3 * C, RT), "dx0": r(B, C, RT),
         "g": 1.0 + 0.3 * r(C), "ss": 0.5 * r(B, 2 * C), "part": r(B, C), "dst0": r(C)}
    return d


NORM_FWD = [(ss, act, res) for ss in (0, 1) for act in (0, 1) for res in (0, 1)]
NORM_BWD = [(ss, act, db) for ss in (0, 1) for act in (0, 1) for db in (0, 1)]


def _kref(C, B, RT, dtype):
    """every kernel-level reference of a case in `dtype`, as float64 tensors"""
    k = {n: v.to(dtype) for n, v in _kin(C, B, RT).items()}
    out = {"col2im3.0": _col2im3_ref(k["dxcol"]), "col2im3.1": _col2im3_ref(k["dxcol"]) + k["dx0"],
           "rowsum": k["u"].reshape(B * C, RT).sum(dim=1), "sum_b": k["part"].sum(dim=0)}
    for ss, act, res in NORM_FWD:
        out[f"y.{ss}{act}{res}"] = _norm_ref(k["u"], k["g"], k["ss"] if ss else None, act, k["res"] if res else None)
    for ss, act in ((0, 0), (0, 1), (1, 0), (1, 1)):
        u, g, s = k["u"].clone().requires_grad_(True), k["g"].clone().requires_grad_(True), k["ss"].clone().requires_grad_(True)
        y = _norm_ref(u, g, s if ss else None, act, None)
        gr = torch.autograd.grad(y, [u, g] + ([s] if ss else []), grad_outputs=k["dy"])
        out[f"du.{ss}{act}"], out[f"dg.{ss}{act}"] = gr[0], gr[1]
        out[f"dbias.{ss}{act}"] = gr[0].sum(dim=(0, 2))
        if ss:
            out[f"dss.{ss}{act}"] = gr[2]
    return {n: v.detach().double() for n, v in out.items()}


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def _pos_rel(got, ref):
    """(B, C, RT): max over (b, t) of max_c |got - ref| / max_c |ref|; a position whose reference is exactly zero has to be exactly zero"""
    num, den = (got.double() - ref).abs().amax(dim=1), ref.abs().amax(dim=1)
    zero = den == 0
    if bool((num[zero] != 0).any()) or bool(torch.isnan(num).any()):
        return float("inf")
    return float((num[~zero] / den[~zero]).max()) if bool((~zero).any()) else 0.0


def _kmeasure(name, got, ref):
    return _pos_rel(got, ref) if name.split(".")[0] in ("y", "du") else _rel(got, ref)


def _kkind(name):
    return "act" if name.split(".")[0] in ("y", "rowsum", "sum_b") else "grad"


@functools.lru_cache(maxsize=None)
def _kreference(C, B, RT):
    return _kref(C, B, RT, torch.float64)


def _one_thread(fn):
    """an fp32 sum depends on how the CPU library splits it over threads: the yardstick has to be the same number wherever the suite runs"""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(nt)


@functools.lru_cache(maxsize=None)
def _kyardstick(C, B, RT):
    ref = _kreference(C, B, RT)
    f32 = _one_thread(lambda: _kref(C, B, RT, torch.float32))
    return {n: _kmeasure(n, f32[n], r) for n, r in ref.items()}


def _bound(kind, d):
    return min(FACTOR * max(d, FLOOR), CAP[kind])


# ---------------------------------------------------------------------------------------------------------------------------------
# bottleneck level: networks, inputs, the float64 reference (as tests/test_mid_forms.py, restated here)
# ---------------------------------------------------------------------------------------------------------------------------------
# name: dim_mults, MZ, seed, mid_c
NETS = {"w4": ((1, 1), 2, 29, 4), "w8": ((1, 2), 2, 31, 8), "w12": ((1, 3), 2, 37, 12), "w24": ((1, 2), 6, 41, 24), "w64": ((1, 4), 8, 19, 64),
        "w80": ((1, 2, 2, 3, 3, 4, 4), 320, 43, 80)}
MID_RT = (1, 3, 4, 33, 34, 65, 130)
# (net, B, RT, rope)
MCASES = ([(n, 3, rt, r) for n in ("w12", "w80") for rt in MID_RT for r in ("net", None)]
          + [(n, 3, rt, r) for n in ("w4", "w8", "w24", "w64") for rt in (34, 65) for r in ("net", None)])
_mid = lambda c: f"{c[0]}-B{c[1]}-RT{c[2]}-{c[3] or 'norope'}"
SLOTS = ("w_mid_in", "wmid1.u1", "wmid1.a1", "wmid1.u2", "wmid1", "w_xn", "w_qv", "w_o", "w_attn_out", "wmid2.u1", "wmid2.a1", "wmid2.u2", "wmid2")
ACTS = SLOTS + ("qv", "kk", "o", "mid_back")
BWD = ("d.o", "d.in", "d.ms1f", "d.ss1", "d.ss2", "d.wmid1.u1", "d.wmid1.u2", "d.wmid2.u1", "d.wmid2.u2")
_CH = {"ms1f": 8, "qv": 2 * HID, "kk": HID, "o": HID, "w_qv": 2 * HID, "w_o": HID}


@functools.lru_cache(maxsize=None)
def _net(name):
    from dquartic.model.unet1d import UNet1d

    mults, mz, seed, _ = NETS[name]
    torch.manual_seed(seed)
    net = UNet1d(dim=4, channels=1, dim_mults=mults, conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=mz, simple=True)
    with torch.no_grad():
        for _, p in net.trainable_named():
            p.add_(0.05 * torch.randn_like(p))
    return net


def _mid_names(net):
    return [n for n, _, _ in net._layout if n.split(".")[0] in ("mid_block1", "mid_block2", "mid_attn") and ".mlp." not in n]


def _freqs(rope):
    return None if rope is None else 1.0 / (10000 ** (torch.arange(0, 16, 2)[:8].float() / 16))


def _inputs(name, B, RT):
    C = NETS[name][3]
    g = torch.Generator().manual_seed(100003 * C + 1000 * B + RT)
    mid_in, ms1f, dout = torch.randn(B, C, RT, generator=g), torch.randn(B, 8, RT, generator=g), torch.randn(B, C, RT, generator=g)
    for b in range(B if RT > 1 else 1):
        mid_in[b, :, (5 * b + 1) % RT] = 0.0
    t = torch.tensor([0, 417, 999] * ((B + 2) // 3), dtype=torch.long)[:B]
    return mid_in, ms1f, t, dout


def _resnet_taps(p, prefix, x, temb, taps, tag):
    """oracle.resnet_block(p, prefix, x, temb, 1) with ss, u1, a1, u2 kept"""
    ss = F.linear(F.silu(temb), p[prefix + ".mlp.1.weight"], p[prefix + ".mlp.1.bias"])
    u1 = F.conv1d(x, p[prefix + ".block1.proj.weight"], p[prefix + ".block1.proj.bias"], padding=1)
    a1 = _norm_ref(u1, p[prefix + ".block1.norm.g"].reshape(-1), ss, 1, None)
    u2 = F.conv1d(a1, p[prefix + ".block2.proj.weight"], p[prefix + ".block2.proj.bias"], padding=1)
    out = _norm_ref(u2, p[prefix + ".block2.norm.g"].reshape(-1), None, 1, x)
    taps.update({tag + ".ss": ss, tag + ".u1": u1, tag + ".a1": a1, tag + ".u2": u2, tag: out})
    return out


def _attention_taps(p, x, cond, freqs, taps):
    """oracle.mid_attention with xn, the unrotated q | v (w_qv), the rotated q | v (qv), the rotated k (kk) and o kept, as (B, channels, RT)"""
    from oracle import dq_oracle as O

    B, _, n = x.shape
    xn = _rmsnorm(x, p["mid_attn.fn.norm.g"])
    qv = F.conv1d(xn, p["mid_attn.fn.fn.to_qv.weight"])
    q, v = (t.reshape(B, HEADS, DH, n).transpose(2, 3) for t in qv.chunk(2, dim=1))
    k = F.conv1d(cond, p["mid_attn.fn.fn.to_k.weight"]).reshape(B, HEADS, DH, n).transpose(2, 3)
    if freqs is not None:
        q, k = O.rope_rotate(q, freqs), O.rope_rotate(k, freqs)
    flat = lambda t: t.transpose(2, 3).reshape(B, HID, n)
    attn = (torch.einsum("bhid,bhjd->bhij", q, k) * (DH ** -0.5)).softmax(dim=-1)
    o = flat(torch.einsum("bhij,bhjd->bhid", attn, v))
    y = F.conv1d(o, p["mid_attn.fn.fn.to_out.weight"], p["mid_attn.fn.fn.to_out.bias"]) + x
    taps.update({"w_xn": xn, "w_qv": qv, "qv": torch.cat((flat(q), flat(v)), dim=1), "kk": flat(k), "o": o, "w_o": o, "w_attn_out": y})
    return y


def _cancel_scale(p, taps, d_o, ms1f):
    """RT = 1 (softmax over one key: d sim = g - g, so d ms1f and to_k's gradient vanish): the largest entry they could have if the terms did
    not cancel, as tests/test_mid_forms.py"""
    B = d_o.shape[0]
    q, v = taps["qv"].chunk(2, dim=1)
    a = (d_o * v).abs().reshape(B, HEADS, DH).sum(-1)
    dkk = (a[:, :, None] * q.abs().reshape(B, HEADS, DH) * DH ** -0.5).reshape(B, HID)
    wk = p["mid_attn.fn.fn.to_k.weight"][:, :, 0].abs()
    return {"d.ms1f": float((dkk @ wk).max()), "mid_attn.fn.fn.to_k.weight": float((dkk.t() @ ms1f[:, :, 0].abs()).max())}


def _oracle(name, B, RT, rope, dtype):
    from oracle import dq_oracle as O

    net = _net(name)
    mults, mz, _, _ = NETS[name]
    names = _mid_names(net)
    p = {k: v.detach().to(dtype) for k, v in net.state_dict().items() if not k.endswith("freqs")}
    for k in names + [f"mid_block{i}.mlp.1.{w}" for i in (1, 2) for w in ("weight", "bias")]:
        p[k].requires_grad_(True)
    mid_in, ms1f, t, dout = _inputs(name, B, RT)
    x, cond = mid_in.to(dtype).requires_grad_(True), ms1f.to(dtype).requires_grad_(True)
    taps = {"w_mid_in": x}
    temb = O.time_mlp(p, t, O.UNetConfig(dim_mults=mults, downsample_dim=mz))
    m = _resnet_taps(p, "mid_block1", x, temb, taps, "wmid1")
    m = _attention_taps(p, m, cond, _freqs(rope), taps)
    m = _resnet_taps(p, "mid_block2", m, temb, taps, "wmid2")
    taps["mid_back"] = m
    wrt = [taps["o"], x, cond, taps["wmid1.ss"], taps["wmid2.ss"], taps["wmid1.u1"], taps["wmid1.u2"], taps["wmid2.u1"], taps["wmid2.u2"]]
    gr = torch.autograd.grad(m, wrt + [p[k] for k in names], grad_outputs=dout.to(dtype))
    out = {k: taps[k].detach().double() for k in ACTS}
    out.update({k: g.double() for k, g in zip(BWD, gr)})
    out.update({k: g.double() for k, g in zip(names, gr[len(BWD):])})
    if RT == 1 and dtype == torch.float64:
        out["@cancel"] = _cancel_scale({k: v.detach() for k, v in p.items()}, {k: v.detach() for k, v in taps.items()}, out["d.o"], ms1f.double())
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, B, RT, rope):
    return _oracle(name, B, RT, rope, torch.float64)


@functools.lru_cache(maxsize=None)
def _yardstick(name, B, RT, rope):
    ref = _reference(name, B, RT, rope)
    f32 = _one_thread(lambda: _oracle(name, B, RT, rope, torch.float32))
    return {k: (_rel(f32[k], r) if float(r.abs().max()) > 0 else 0.0) for k, r in ref.items() if k != "@cancel"}


def _mkind(k):
    return "act" if k in ACTS else "grad"


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restated_references_are_the_oracles():
    """_rmsnorm, _norm_ref and the tapped blocks ARE oracle.rmsnorm / oracle.block / oracle.resnet_block / oracle.mid_attention bit for bit in
    float64; _im2col3_ref with the weight viewed as (cout, 3 cin) is Conv1d(k 3, padding 1); _col2im3_ref is its transpose"""
    from oracle import dq_oracle as O

    g = torch.Generator().manual_seed(5)
    x, gn = torch.randn(3, 12, 34, generator=g, dtype=torch.float64), torch.randn(1, 12, 1, generator=g, dtype=torch.float64)
    x[1, :, 7] *= 1e-14
    assert torch.equal(_rmsnorm(x, gn), O.rmsnorm(x, gn))
    z = x.clone()
    z[0, :, 3] = 0.0
    assert torch.equal(_rmsnorm(z, gn), O.rmsnorm(z, gn))
    w, b = torch.randn(12, 12, 3, generator=g, dtype=torch.float64), torch.randn(12, generator=g, dtype=torch.float64)
    p = {"k.proj.weight": w, "k.proj.bias": b, "k.norm.g": gn}
    ss = torch.randn(3, 24, generator=g, dtype=torch.float64)
    u = F.conv1d(x, w, b, padding=1)
    assert torch.equal(_norm_ref(u, gn.reshape(-1), ss, 1, None), O.block(p, "k", x, ss[:, :, None].chunk(2, dim=1)))
    assert torch.equal(_norm_ref(u, gn.reshape(-1), None, 1, None), O.block(p, "k", x))
    col = _im2col3_ref(x)
    assert _rel(torch.einsum("om,bmt->bot", w.reshape(12, 36), col) + b[None, :, None], u) < 1e-14
    y = torch.randn(3, 36, 34, generator=g, dtype=torch.float64)
    assert abs(float((col * y).sum() - (x * _col2im3_ref(y)).sum())) < 1e-11
    for name, rope in (("w12", "net"), ("w64", None)):
        net = _net(name)
        mults, mz, _, _ = NETS[name]
        pp = {k: v.detach().double() for k, v in net.state_dict().items()}
        mid_in, ms1f, t, _ = _inputs(name, 3, 34)
        temb = O.time_mlp(pp, t, O.UNetConfig(dim_mults=mults, downsample_dim=mz))
        taps = {}
        a = _resnet_taps(pp, "mid_block1", mid_in.double(), temb, taps, "wmid1")
        assert torch.equal(a, O.resnet_block(pp, "mid_block1", mid_in.double(), temb, 1))
        m = _attention_taps(pp, a, ms1f.double(), _freqs(rope), taps)
        assert torch.equal(m, O.mid_attention(pp, a, ms1f.double(), rope is not None))
        assert torch.equal(_resnet_taps(pp, "mid_block2", m, temb, taps, "wmid2"), O.resnet_block(pp, "mid_block2", m, temb, 1))


def test_wide_plans():
    """every network of the file is a wide plan of the width its name says, host side"""
    from dquartic import _native as N

    for name, (_, _, _, C) in NETS.items():
        plan = _net(name)._plan
        for B, RT in ((3, 1), (3, 34), (1, 130)):
            f = N.mid_forms(plan, B, RT)
            assert f["wide_mid"] and f["mid_c"] == C and f["cond_dim"] == 8, (name, f)
            assert not (f["qkv_fused"] or f["out_fused"] or f["pre_fused"])
            assert 0 <= f["ss_mid1"] and f["ss_mid1"] + 2 * C <= f["ss_mid2"] and f["ss_mid2"] + 2 * C <= f["ss_total"], f
    assert {C < 8 for *_, C in NETS.values()} == {True, False} and any(C % 8 for *_, C in NETS.values() if C > 8)
    assert {64, 80} <= {C for *_, C in NETS.values()}
    lib, plan = N.lib(), _net("w12")._plan
    assert lib.dq_debug_layout(plan, 3, 34) == 0
    P, t = 36, 3 * 12 * 36
    off = {k: int(lib.dq_debug_tensor_offset(plan, k.encode())) for k in SLOTS + ("w_xcol", "w_stats", "w_gemm_part", "mid_back", "down1")}
    assert min(off.values()) >= 0, off
    order = ("w_mid_in", "wmid1.u1", "wmid1.a1", "wmid1.u2", "wmid1", "wmid2.u1", "wmid2.a1", "wmid2.u2", "wmid2", "w_xcol", "w_xn", "w_qv", "w_o",
             "w_attn_out", "w_stats", "w_gemm_part")
    size = {"w_xcol": 3 * t, "w_qv": 3 * 2 * HID * P, "w_o": 3 * HID * P}
    for a, b in zip(order, order[1:]):
        assert off[b] >= off[a] + size.get(a, t) and off[a] % 64 == 0, (a, b, off)
    narrow = _net_narrow()._plan
    assert lib.dq_debug_layout(narrow, 3, 34) == 0 and lib.dq_debug_tensor_offset(narrow, b"w_mid_in") == -1
    assert lib.dq_debug_tensor_offset(narrow, b"mid_back") >= 0


@functools.lru_cache(maxsize=None)
def _net_narrow():
    from dquartic.model.unet1d import UNet1d

    return UNet1d(dim=4, channels=1, dim_mults=(1, 2, 4), conditional=True, init_cond_channels=1, attn_cond_channels=1, downsample_dim=4, simple=True)


def test_entries_refuse_before_any_device_call():
    """null required operands, P % 4 != 0, P < RT (or past RT + 3), non-positive sizes, ss without dss, a short scratch, a narrow plan, a short
    workspace: refused on the host (this test runs without a GPU; `one` is never dereferenced)"""
    from dquartic import _native as N

    lib = N.lib()
    one = ctypes.c_void_p(64)
    ok = (3, 12, 34, 36)  # B, C, RT, P
    bad_shapes = [(0, 12, 34, 36), (3, 0, 34, 36), (3, 12, 0, 0), (3, 12, 34, 35), (3, 12, 34, 32), (3, 12, 34, 40), (-1, 12, 34, 36)]
    refused = lambda rc: rc != 0 and len(N.last_error()) > 0
    # im2col3 / col2im3
    for x, y in ((None, one), (one, None)):
        assert refused(lib.dq_wide_im2col3(x, y, *ok, None)) and refused(lib.dq_wide_col2im3(x, y, *ok, 0, None))
    for s in bad_shapes:
        assert refused(lib.dq_wide_im2col3(one, one, *s, None)) and refused(lib.dq_wide_col2im3(one, one, *s, 1, None)), s
    # repitch(dst, dpitch, src, spitch, rows, n)
    assert refused(lib.dq_wide_repitch(None, 36, one, 34, 5, 34, None)) and refused(lib.dq_wide_repitch(one, 36, None, 34, 5, 34, None))
    for dp, sp, rows, n in ((36, 34, 0, 34), (36, 34, 5, 0), (32, 34, 5, 34), (36, 33, 5, 34), (35, 34, 5, 34), (40, 34, 5, 34), (36, 38, 5, 34)):
        assert refused(lib.dq_wide_repitch(one, dp, one, sp, rows, n, None)), (dp, sp, rows, n)
    # norm forward (u, g, ss, ss_stride, act, res, y)
    for u, g, y in ((None, one, one), (one, None, one), (one, one, None)):
        assert refused(lib.dq_wide_norm_fwd(u, g, None, 0, 1, None, y, *ok, None))
    for s in bad_shapes:
        assert refused(lib.dq_wide_norm_fwd(one, one, None, 0, 1, None, one, *s, None)), s
    assert refused(lib.dq_wide_norm_fwd(one, one, one, 23, 1, None, one, *ok, None))  # (a stride below 2 C)
    assert refused(lib.dq_wide_norm_fwd(one, one, None, 0, 2, None, one, *ok, None))  # (GELU is not this kernel's)
    # norm backward (u, dy, g, ss, ss_stride, act, du, dg, dss, dbias, scratch, scratch_floats)
    need = lib.dq_wide_norm_bwd_scratch_floats(3, 12, 36)
    assert need == 3 * (2 * 36 + 2 * 12)
    assert lib.dq_wide_norm_bwd_scratch_floats(0, 12, 36) == -1 and lib.dq_wide_norm_bwd_scratch_floats(3, 0, 36) == -1
    assert lib.dq_wide_norm_bwd_scratch_floats(3, 12, 0) == -1
    full = [one, one, one, None, 0, 1, one, one, None, None, one, need]
    for i in (0, 1, 2, 6, 7, 10):
        a = list(full)
        a[i] = None
        assert refused(lib.dq_wide_norm_bwd(*a, *ok, None)), i
    for s in bad_shapes:
        assert refused(lib.dq_wide_norm_bwd(*full, *s, None)), s
    a = list(full)
    a[3], a[4] = one, 24
    assert refused(lib.dq_wide_norm_bwd(*a, *ok, None)) and "dss" in N.last_error()  # (ss without dss)
    a[8], a[4] = one, 23
    assert refused(lib.dq_wide_norm_bwd(*a, *ok, None))
    a = list(full)
    a[11] = need - 1
    assert refused(lib.dq_wide_norm_bwd(*a, *ok, None)) and "scratch" in N.last_error()
    a = list(full)
    a[5] = 2
    assert refused(lib.dq_wide_norm_bwd(*a, *ok, None))
    # rowsum(x, rows, RT, P, out) / sum_b(part, B, C, dst)
    assert refused(lib.dq_wide_rowsum(None, 5, 34, 36, one, None)) and refused(lib.dq_wide_rowsum(one, 5, 34, 36, None, None))
    for rows, RT, P in ((0, 34, 36), (5, 0, 0), (5, 34, 35), (5, 34, 32), (5, 34, 40)):
        assert refused(lib.dq_wide_rowsum(one, rows, RT, P, one, None)), (rows, RT, P)
    assert refused(lib.dq_wide_sum_b(None, 3, 12, one, None)) and refused(lib.dq_wide_sum_b(one, 3, 12, None, None))
    assert refused(lib.dq_wide_sum_b(one, 0, 12, one, None)) and refused(lib.dq_wide_sum_b(one, 3, 0, one, None))
    # the bottleneck entries
    plan = _net("w12")._plan
    nbytes = lib.dq_unet_workspace_bytes(plan, 3, 34, 1)
    assert refused(lib.dq_debug_wide_mid_fwd(plan, one, None, one, 1, one, nbytes // 2 - 4, 3, 34, None)) and "too small" in N.last_error()
    assert refused(lib.dq_debug_wide_mid_bwd(plan, one, None, one, 0, one, nbytes - 4, 3, 34, None)) and "too small" in N.last_error()
    for args in ((None, one, one, one), (plan, None, one, one), (plan, one, None, one), (plan, one, one, None)):
        assert refused(lib.dq_debug_wide_mid_fwd(args[0], args[1], None, args[2], 1, args[3], nbytes, 3, 34, None))
        assert refused(lib.dq_debug_wide_mid_bwd(args[0], args[1], None, args[2], 0, args[3], nbytes, 3, 34, None))
    assert refused(lib.dq_debug_wide_mid_fwd(plan, one, None, one, 1, one, nbytes, 0, 34, None))
    assert refused(lib.dq_debug_wide_mid_bwd(plan, one, None, one, 0, one, nbytes, 3, 0, None))
    narrow, big = _net_narrow()._plan, 1 << 40
    assert not N.mid_forms(narrow, 3, 34)["wide_mid"]
    assert refused(lib.dq_debug_wide_mid_fwd(narrow, one, None, one, 1, one, big, 3, 34, None)) and "narrow" in N.last_error()
    assert refused(lib.dq_debug_wide_mid_bwd(narrow, one, None, one, 0, one, big, 3, 34, None)) and "narrow" in N.last_error()


def _kbounds_case(case):
    d = _kyardstick(*case)
    worst = {}
    for n, e in d.items():
        q = n.split(".")[0]
        if e >= worst.get(q, -1.0):
            worst[q] = e
    print(f"fp32 reference vs float64 {_kid(case)}: " + "  ".join(f"{q} {e:.2e}" for q, e in sorted(worst.items())))
    for n, e in d.items():
        assert e < CAP[_kkind(n)] / FACTOR, (n, e)


@pytest.mark.parametrize("case", KCASES, ids=_kid)
def test_bounds_leave_room_for_fp32_kernels(case):
    """kernel level: the fp32 CPU reference against float64, quantity by quantity, under cap / 16 (a condition on the inputs)"""
    _kbounds_case(case)


@pytest.mark.parametrize("case", MCASES, ids=_mid)
def test_bounds_leave_room_for_fp32(case):
    """bottleneck level: the oracle in fp32 against itself in float64, tensor by tensor, under cap / 16"""
    d = _yardstick(*case)
    worst = {}
    for k, e in d.items():
        kind = "act" if k in ACTS else "bwd" if k in BWD else "param"
        if e >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (e, k)
    print(f"fp32 oracle vs float64 {_mid(case)}: " + "  ".join(f"{k} {e:.2e} ({w})" for k, (e, w) in sorted(worst.items())))
    for k, e in d.items():
        assert e < CAP[_mkind(k)] / FACTOR, (k, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU, kernel level
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 64  # floats on either side of every tensor
SENTINEL = -12345.678
GARBAGE = (7.5e8, -3.25e-3)  # what the input pads hold in the first / the second run


class _Dev:
    """device tensors as views inside larger buffers with guard bands; inputs are remembered and checked untouched"""

    def __init__(self):
        self.all, self.ins = [], []

    def _alloc(self, shape):
        n = int(torch.Size(shape).numel())
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.all.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def inp(self, x):
        v = self._alloc(x.shape)
        v.copy_(x)
        self.ins.append((v, v.clone()))
        return v

    def out(self, shape, fill=float("nan")):
        v = self._alloc(shape)
        v.fill_(fill)
        return v

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.all:
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "a guard band was written"
        for v, keep in self.ins:
            assert torch.equal(v, keep), "an input was written"


def _padded(x, P, garbage):
    """(.., RT) -> (.., P) with `garbage` in the pad columns"""
    out = torch.full(x.shape[:-1] + (P,), garbage, dtype=torch.float32)
    out[..., :x.shape[-1]] = x
    return out


def _valid(y, RT):
    """the valid columns of a padded result, after asserting that its pad columns are exactly zero"""
    assert bool((y[..., RT:] == 0).all()), "a pad column is not zero"
    return y[..., :RT]


_KWORST = {}


def _kcompare(case, name, got):
    """a kernel's result against float64 at 16 d; keeps the worst err / d per quantity for the report"""
    ref, d = _kreference(*case)[name], _kyardstick(*case)[name]
    e = _kmeasure(name, got.detach().cpu(), ref)
    print(f"{_kid(case)} {name}: err {e:.2e}  d {d:.2e}  bound {_bound(_kkind(name), d):.2e}")
    q = name.split(".")[0]
    if not e / max(d, FLOOR) <= _KWORST.get(q, (0.0,))[0]:
        _KWORST[q] = (e / max(d, FLOOR), e, _kid(case), name)
    assert e < _bound(_kkind(name), d), (_kid(case), name, e, d)


def _twice(fn):
    """fn(garbage) -> {name: tensor}: run with each of the two pad fillings; the results are bitwise equal; returns the first"""
    a, b = fn(GARBAGE[0]), fn(GARBAGE[1])
    for k in a:
        assert torch.equal(a[k], b[k]), (k, "differs between two runs (other garbage in the input pads)")
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("case", KCASES, ids=_kid)
def test_moves(case):
    """k_im2col3, k_repitch (both directions): pure moves, bitwise equal to the reference, pad columns exactly zero"""
    from dquartic import _native as N

    C, B, RT = case
    P, lib, k = _P(RT), N.lib(), _kin(*case)

    def run(garbage):
        dv = _Dev()
        x = dv.inp(_padded(k["x"], P, garbage))
        xcol, wide, narrow = dv.out((B, 3 * C, P)), dv.out((B, C, P)), dv.out((B, C, RT))
        tight = dv.inp(k["x"])
        N.check(lib.dq_wide_im2col3(N.ptr(x), N.ptr(xcol), B, C, RT, P, N.stream_ptr()), "dq_wide_im2col3")
        N.check(lib.dq_wide_repitch(N.ptr(wide), P, N.ptr(tight), RT, B * C, RT, N.stream_ptr()), "dq_wide_repitch")
        N.check(lib.dq_wide_repitch(N.ptr(narrow), RT, N.ptr(x), P, B * C, RT, N.stream_ptr()), "dq_wide_repitch")
        dv.check()
        return {"xcol": xcol.cpu(), "wide": wide.cpu(), "narrow": narrow.cpu()}

    got = _twice(run)
    assert torch.equal(_valid(got["xcol"], RT), _im2col3_ref(k["x"]))
    assert torch.equal(_valid(got["wide"], RT), k["x"]) and torch.equal(got["narrow"], k["x"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", KCASES, ids=_kid)
def test_col2im_and_sums(case):
    """k_col2im3 (store and accumulate), k_rowsum, dq_wide_sum_b (onto zero and onto non-zero contents) against float64, garbage in the input pads"""
    from dquartic import _native as N

    C, B, RT = case
    P, lib, k = _P(RT), N.lib(), _kin(*case)

    def run(garbage):
        dv = _Dev()
        dxcol, u, part = dv.inp(_padded(k["dxcol"], P, garbage)), dv.inp(_padded(k["u"], P, garbage)), dv.inp(k["part"])
        dx_st = dv.out((B, C, P))
        dx_acc = dv.out((B, C, P))
        dx_acc.copy_(_padded(k["dx0"], P, garbage))
        rows, s0, s1 = dv.out((B * C,)), dv.out((C,), 0.0), dv.out((C,))
        s1.copy_(k["dst0"])
        N.check(lib.dq_wide_col2im3(N.ptr(dxcol), N.ptr(dx_st), B, C, RT, P, 0, N.stream_ptr()), "dq_wide_col2im3")
        N.check(lib.dq_wide_col2im3(N.ptr(dxcol), N.ptr(dx_acc), B, C, RT, P, 1, N.stream_ptr()), "dq_wide_col2im3")
        N.check(lib.dq_wide_rowsum(N.ptr(u), B * C, RT, P, N.ptr(rows), N.stream_ptr()), "dq_wide_rowsum")
        N.check(lib.dq_wide_sum_b(N.ptr(part), B, C, N.ptr(s0), N.stream_ptr()), "dq_wide_sum_b")
        N.check(lib.dq_wide_sum_b(N.ptr(part), B, C, N.ptr(s1), N.stream_ptr()), "dq_wide_sum_b")
        dv.check()
        return {"st": dx_st.cpu(), "acc": dx_acc.cpu(), "rows": rows.cpu(), "s0": s0.cpu(), "s1": s1.cpu()}

    got = _twice(run)
    _kcompare(case, "col2im3.0", _valid(got["st"], RT))
    _kcompare(case, "col2im3.1", _valid(got["acc"], RT))
    _kcompare(case, "rowsum", got["rows"])
    _kcompare(case, "sum_b", got["s0"])
    assert torch.equal(got["s1"], k["dst0"] + got["s0"])  # dst += ONE sum formed in registers


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 7, 8, 9, 17])
def test_sum_b_is_the_index_order_sum_bit_for_bit(B):
    """dq_wide_sum_b (launch_ordered_sum: eight loads in flight from 8 partial rows on, a tail loop) against a float32 numpy loop in index
    order from 0, then ONE dst + s: exact, at C around a 256-thread block"""
    import numpy as np

    from dquartic import _native as N

    for C in (1, 255, 256, 257):
        gen = torch.Generator().manual_seed(1000 * B + C)
        part, dst0 = torch.randn(B, C, generator=gen), torch.randn(C, generator=gen)
        s = np.zeros(C, dtype=np.float32)
        for b in range(B):
            s = s + part[b].numpy()
        assert s.dtype == np.float32
        want = dst0.numpy() + s
        dv = _Dev()
        pd, dst = dv.inp(part), dv.out((C,))
        dst.copy_(dst0)
        N.check(N.lib().dq_wide_sum_b(N.ptr(pd), B, C, N.ptr(dst), N.stream_ptr()), "dq_wide_sum_b")
        dv.check()
        assert np.array_equal(dst.cpu().numpy(), want), (B, C)


def _ss_buffer(dv, k, C, B, fill=None):
    """a sample's [scale | shift] inside a longer per-sample vector, as in the network: stride 2 C + 10, offset 3"""
    stride, off = 2 * C + 10, 3
    host = torch.full((B, stride), SENTINEL * 2, dtype=torch.float32)
    host[:, off:off + 2 * C] = k["ss"] if fill is None else fill
    buf = dv.inp(host) if fill is None else dv.out((B, stride))
    if fill is not None:
        buf.copy_(host)
    return buf, buf[:, off:off + 2 * C], stride


@pytest.mark.gpu
@pytest.mark.parametrize("case", KCASES, ids=_kid)
def test_norm_forward(case):
    """k_wnorm_fwd: ss null / present (at a stride), act none / SiLU, res null / present, gains off 1, the three special columns"""
    from dquartic import _native as N

    C, B, RT = case
    P, lib, k = _P(RT), N.lib(), _kin(*case)

    def run(garbage):
        dv = _Dev()
        u, res, g = dv.inp(_padded(k["u"], P, garbage)), dv.inp(_padded(k["res"], P, garbage)), dv.inp(k["g"])
        _, ss, stride = _ss_buffer(dv, k, C, B)
        out = {}
        for s, act, r in NORM_FWD:
            y = dv.out((B, C, P))
            N.check(lib.dq_wide_norm_fwd(N.ptr(u), N.ptr(g), N.ptr(ss) if s else None, stride if s else 0, act, N.ptr(res) if r else None, N.ptr(y),
                                         B, C, RT, P, N.stream_ptr()), "dq_wide_norm_fwd")
            out[f"y.{s}{act}{r}"] = y
        dv.check()
        return {n: v.cpu() for n, v in out.items()}

    got = _twice(run)
    for n, y in got.items():
        _kcompare(case, n, _valid(y, RT))


@pytest.mark.gpu
@pytest.mark.parametrize("case", KCASES, ids=_kid)
def test_norm_backward(case):
    """k_wnorm_bwd_stats / _apply / launch_sum_b: ss and dbias null / present, act none / SiLU; du == dy against du != dy bitwise; d g, d scale /
    shift and d bias as `+=` onto non-zero contents (bitwise fl(contents + the sum onto zero)); the special columns, the clamp among them"""
    from dquartic import _native as N

    C, B, RT = case
    P, lib, k = _P(RT), N.lib(), _kin(*case)
    need = int(lib.dq_wide_norm_bwd_scratch_floats(B, C, P))
    pre_g, pre_b = 0.25 * ((torch.arange(C) % 7) - 3).float(), 0.5 * ((torch.arange(C) % 5) - 2).float()
    pre_ss = 0.125 * ((torch.arange(B * 2 * C) % 9) - 4).float().view(B, 2 * C)

    def run(garbage):
        dv = _Dev()
        u, dy, g = dv.inp(_padded(k["u"], P, garbage)), dv.inp(_padded(k["dy"], P, garbage)), dv.inp(k["g"])
        _, ss, stride = _ss_buffer(dv, k, C, B)
        out = {}

        def call(s, act, db, du, dyv, dg, dss, dbias):
            scratch = dv.out((need,))
            N.check(lib.dq_wide_norm_bwd(N.ptr(u), N.ptr(dyv), N.ptr(g), N.ptr(ss) if s else None, stride if s else 0, act, N.ptr(du), N.ptr(dg),
                                         N.ptr(dss) if s else None, N.ptr(dbias) if db else None, N.ptr(scratch), need, B, C, RT, P,
                                         N.stream_ptr()), "dq_wide_norm_bwd")

        for s, act, db in NORM_BWD:
            tag = f"{s}{act}{db}"
            # onto zero, du apart from dy
            du, dg, dbias = dv.out((B, C, P)), dv.out((C,), 0.0), dv.out((C,), 0.0)
            dss_buf, dss, _ = _ss_buffer(dv, k, C, B, fill=0.0)
            call(s, act, db, du, dy, dg, dss, dbias)
            # in place: du is dy
            dy2, dg2, dbias2 = dv.out((B, C, P)), dv.out((C,), 0.0), dv.out((C,), 0.0)
            dy2.copy_(dy)
            dss2_buf, dss2, _ = _ss_buffer(dv, k, C, B, fill=0.0)
            call(s, act, db, dy2, dy2, dg2, dss2, dbias2)
            # onto non-zero contents
            du3, dg3, dbias3 = dv.out((B, C, P)), dv.out((C,)), dv.out((C,))
            dg3.copy_(pre_g)
            dbias3.copy_(pre_b)
            dss3_buf, dss3, _ = _ss_buffer(dv, k, C, B, fill=pre_ss)
            call(s, act, db, du3, dy, dg3, dss3, dbias3)
            out.update({"du." + tag: du, "dg." + tag: dg, "dbias." + tag: dbias, "dss." + tag: dss_buf, "du2." + tag: dy2, "dg2." + tag: dg2,
                        "dbias2." + tag: dbias2, "dss2." + tag: dss2_buf, "du3." + tag: du3, "dg3." + tag: dg3, "dbias3." + tag: dbias3,
                        "dss3." + tag: dss3_buf})
        dv.check()
        return {n: v.cpu() for n, v in out.items()}

    got = _twice(run)
    sl = slice(3, 3 + 2 * C)
    for s, act, db in NORM_BWD:
        tag, rt = f"{s}{act}{db}", f"{s}{act}"
        _kcompare(case, "du." + rt, _valid(got["du." + tag], RT))
        _kcompare(case, "dg." + rt, got["dg." + tag])
        if db:
            _kcompare(case, "dbias." + rt, got["dbias." + tag])
        else:
            assert bool((got["dbias." + tag] == 0).all()) and torch.equal(got["dbias3." + tag], pre_b)  # (null: not this call's)
        outside = torch.ones(2 * C + 10, dtype=torch.bool)
        outside[sl] = False
        for name in ("dss.", "dss2.", "dss3."):
            assert bool((got[name + tag][:, outside] == SENTINEL * 2).all()), "d scale / shift written outside the block's slice"
        if s:
            _kcompare(case, "dss." + rt, got["dss." + tag][:, sl])
        else:
            assert bool((got["dss." + tag][:, sl] == 0).all()) and torch.equal(got["dss3." + tag][:, sl], pre_ss)
        # in place == apart, bit for bit
        for q in ("du", "dg", "dbias", "dss"):
            assert torch.equal(got[q + "2." + tag], got[q + "." + tag]), (q, tag, "du == dy differs from du != dy")
        # += : contents + (the sum onto zero), one rounding
        assert torch.equal(got["du3." + tag], got["du." + tag])
        assert torch.equal(got["dg3." + tag], pre_g + got["dg." + tag]), ("dg", tag)
        if db:
            assert torch.equal(got["dbias3." + tag], pre_b + got["dbias." + tag]), ("dbias", tag)
        if s:
            assert torch.equal(got["dss3." + tag][:, sl], pre_ss + got["dss." + tag][:, sl]), ("dss", tag)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU, bottleneck level
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_net(name):
    net = _net(name)
    gpu = type(net)(dim=4, channels=1, dim_mults=NETS[name][0], conditional=True, init_cond_channels=1, attn_cond_channels=1,
                    downsample_dim=NETS[name][1], simple=True)
    gpu.load_state_dict(net.state_dict())
    return gpu.cuda()


class _Wide:
    """a training workspace of one (net, B, RT) with the case's inputs in their slots"""

    def __init__(self, name, B, RT, rope, samples=None):
        from dquartic import _native as N

        self.N, self.lib, self.name, self.B, self.RT, self.P = N, N.lib(), name, B, RT, _P(RT)
        self.net = _gpu_net(name)
        self.plan, self.C = self.net._plan, NETS[name][3]
        self.params = self.net.flat_params
        self.forms = N.mid_forms(self.plan, B, RT)
        assert self.forms["wide_mid"] and self.forms["mid_c"] == self.C, self.forms
        assert self.lib.dq_debug_layout(self.plan, B, RT) == 0
        self.down = f"down{len(NETS[name][0]) - 1}"
        names = ("ss", "ms1f", "lse", "w_xcol", "w_stats", "w_gemm_part", self.down) + ACTS
        self.off = {k: int(self.lib.dq_debug_tensor_offset(self.plan, k.encode())) for k in names}
        assert min(self.off.values()) >= 0, self.off
        self.twin = int(self.lib.dq_debug_tensor_offset(self.plan, b"@twin"))
        self.nbytes = int(self.lib.dq_unet_workspace_bytes(self.plan, B, RT, 1))
        assert self.nbytes == 8 * self.twin
        self.ws = torch.zeros(2 * self.twin, dtype=torch.float32, device="cuda")
        fr = _freqs(rope)
        self.freqs = None if fr is None else fr.cuda()
        mid_in, ms1f, t, dout = _inputs(name, 3 if samples is not None else B, RT)
        if samples is not None:
            mid_in, ms1f, t, dout = (v[samples].contiguous() for v in (mid_in, ms1f, t, dout))
        self.inputs = tuple(v.cuda() for v in (mid_in, ms1f, t, dout))
        self.t = self.inputs[2]

    def view(self, k, twin=False):
        o = self.off[k] + (self.twin if twin else 0)
        if k in (self.down, "mid_back"):  # (B * RT, mid_c) rows: the m/z levels' layout
            return self.ws[o:o + self.B * self.RT * self.C].view(self.B, self.RT, self.C).transpose(1, 2)
        C = _CH.get(k, self.C)
        n = self.P if k in SLOTS else self.RT
        return self.ws[o:o + self.B * C * n].view(self.B, C, n)

    def wide_region(self, twin=False):
        """every wide slot (the named ones, the im2col buffer, the norm backward's scratch) and the alignment gaps between them"""
        o = self.twin if twin else 0
        return self.ws[o + self.off["w_mid_in"]:o + self.off["w_gemm_part"]]

    def dss(self, which):
        o = self.off["ss"] + self.twin
        v = self.ws[o:o + self.B * self.forms["ss_total"]].view(self.B, self.forms["ss_total"])
        return v[:, self.forms[which]:self.forms[which] + 2 * self.C]

    def fwd(self, fill=float("nan")):
        """`fill` into every wide slot and everything else the forward writes, the inputs into their slots, the call; the results with their
        pad columns (asserted zero); inputs untouched"""
        N = self.N
        self.wide_region().fill_(fill)
        for k in ("qv", "kk", "o", "mid_back"):
            self.view(k).fill_(fill)
        lse = self.ws[self.off["lse"]:self.off["lse"] + self.B * HEADS * self.RT]
        lse.fill_(fill)
        self.view(self.down).copy_(self.inputs[0])
        self.view("ms1f").copy_(self.inputs[1])
        N.check(self.lib.dq_debug_wide_mid_fwd(self.plan, N.ptr(self.params), N.ptr(self.freqs), N.ptr(self.t), 1, N.ptr(self.ws), self.nbytes,
                                               self.B, self.RT, N.stream_ptr()), "dq_debug_wide_mid_fwd")
        torch.cuda.synchronize()
        out = {k: self.view(k).clone() for k in ACTS}
        for k in SLOTS:
            assert not torch.isnan(out[k]).any(), (k, "NaN left")
            assert bool((out[k][..., self.RT:] == 0).all()), (k, "a pad column is not zero")
        assert not torch.isnan(lse).any()
        assert torch.equal(self.view(self.down), self.inputs[0]) and torch.equal(self.view("ms1f"), self.inputs[1])
        return out

    def bwd(self, mode=0, grads=None, fill=float("nan")):
        """`fill` into every wide slot of the twin and into the twin of the input, d out into the twin of mid_back, the call"""
        N = self.N
        if grads is None:
            grads = torch.zeros_like(self.params)
        self.wide_region(twin=True).fill_(fill)
        self.view(self.down, twin=True).fill_(fill)
        self.view("mid_back", twin=True).copy_(self.inputs[3])
        N.check(self.lib.dq_debug_wide_mid_bwd(self.plan, N.ptr(self.params), N.ptr(self.freqs), N.ptr(grads), mode, N.ptr(self.ws), self.nbytes,
                                               self.B, self.RT, N.stream_ptr()), "dq_debug_wide_mid_bwd")
        torch.cuda.synchronize()
        out = {"d.o": self.view("o", True), "d.in": self.view(self.down, True), "d.ms1f": self.view("ms1f", True), "d.ss1": self.dss("ss_mid1"),
               "d.ss2": self.dss("ss_mid2")}
        out.update({"d." + k: self.view(k, True) for k in ("wmid1.u1", "wmid1.u2", "wmid2.u1", "wmid2.u2")})
        out = {k: v.clone() for k, v in out.items()}
        for k in ("wmid1.u1", "wmid1.u2", "wmid2.u1", "wmid2.u2"):
            assert bool((out["d." + k][..., self.RT:] == 0).all()), (k, "a pad column of the gradient is not zero")
        for n, o, shape in self.net._layout:
            if n in _mid_names(self.net):
                out[n] = grads[o:o + torch.Size(shape).numel()].view(shape).clone()
        out["@flat"] = grads
        return out


_WORST = {}


def _compare(case, got):
    """every tensor of `got` against the float64 reference at 16 d_k (valid columns); prints the case's worst err / d_k per kind of tensor"""
    ref, d = _reference(*case), _yardstick(*case)
    RT = case[2]
    fails, worst = [], {}
    for k, r in ref.items():
        if k == "@cancel":
            continue
        g = got[k].detach().cpu().double()
        if k in SLOTS or k.startswith("d.wmid"):
            g = g[..., :RT]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        rmax = float(r.abs().max())
        if rmax == 0.0:  # (RT = 1: see _cancel_scale)
            assert RT == 1 and k in ref["@cancel"], (k, "reference identically zero")
            e, bound = float(g.abs().max()) / ref["@cancel"][k], FACTOR * FLOOR
            ratio = e / FLOOR
        else:
            e, bound = float((g - r).abs().max()) / rmax, _bound(_mkind(k), d[k])
            ratio = e / max(d[k], FLOOR)
        if not e < bound:
            fails.append((k, e, bound))
        kind = k if k in ACTS + BWD else "d." + k.split(".", 1)[1].replace("fn.fn.", "").replace("fn.", "")
        kind = kind.replace("wmid1", "wmid*").replace("wmid2", "wmid*").replace("ss1", "ss*").replace("ss2", "ss*")
        if not ratio <= worst.get(kind, (0.0,))[0]:
            worst[kind] = (ratio, e)
        if not ratio <= _WORST.get(kind, (0.0,))[0]:
            _WORST[kind] = (ratio, e, _mid(case), k)
    print(f"gpu vs float64 {_mid(case)}  err/d_k (err): " + "  ".join(f"{k} {r:.2f} ({e:.1e})" for k, (r, e) in sorted(worst.items())))
    assert not fails, (_mid(case), fails)


def _equal(a, b, keys=None):
    for k in (keys or a.keys()):
        if k != "@flat":
            assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MCASES, ids=_mid)
def test_wide_bottleneck(case):
    """forward and backward of the wide bottleneck, every intermediate, gradient and parameter gradient against float64; NaN in every wide
    slot of the workspace and of the twin beforehand (fwd / bwd assert none is left, pads zero); w_o is o re-pitched bit for bit"""
    bn = _Wide(*case)
    got = bn.fwd()
    assert torch.equal(got["w_o"][..., :bn.RT], got["o"])
    got.update(bn.bwd())
    _compare(case, got)


STRUCT = [("w12", 3, 34, "net"), ("w80", 3, 65, "net"), ("w4", 3, 34, None), ("w12", 3, 3, "net"), ("w80", 3, 4, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", STRUCT, ids=_mid)
def test_structure_of_the_calls(case):
    """every take_nz slot is written before it is read, pads included: NaN against zero prefill of every wide slot (workspace and twin) gives
    bitwise the same; a repeated call is bitwise identical; the side queue on and off agree bit for bit, flat gradient included"""
    bn = _Wide(*case)
    f1 = bn.fwd(float("nan"))
    b1 = bn.bwd(0, fill=float("nan"))
    f2 = bn.fwd(0.0)
    b2 = bn.bwd(0, fill=0.0)
    _equal(f1, f2)
    _equal(b1, b2)
    assert torch.equal(b1["@flat"], b2["@flat"])
    f3 = bn.fwd(float("nan"))
    b3 = bn.bwd(1, fill=float("nan"))
    _equal(f1, f3)
    _equal(b1, b3)
    assert torch.equal(b1["@flat"], b3["@flat"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,RT,rope", [("w12", 34, "net"), ("w80", 65, "net"), ("w12", 3, None)])
def test_a_sample_alone_is_the_sample_in_the_batch(name, RT, rope):
    """sample b of the B = 3 call equals a B = 1 call on that sample bit for bit: forward tensors, d input, d ms1f, d(scale, shift)"""
    full = _Wide(name, 3, RT, rope)
    ff = full.fwd()
    fb = full.bwd()
    for b in range(3):
        one = _Wide(name, 1, RT, rope, samples=slice(b, b + 1))
        of = one.fwd()
        ob = one.bwd()
        for k, v in of.items():
            assert torch.equal(v[0], ff[k][b]), (RT, b, k)
        for k in ("d.in", "d.ms1f", "d.ss1", "d.ss2", "d.o", "d.wmid1.u1", "d.wmid2.u2"):
            assert torch.equal(ob[k][0], fb[k][b]), (RT, b, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("w12", 3, 34, "net"), ("w80", 3, 65, "net"), ("w24", 3, 34, None)], ids=_mid)
def test_gradients_accumulate_into_the_bottlenecks_tensors_only(case):
    """onto zeros: every float outside the bottleneck's tensors -- the alignment gaps of at most 3 floats between tensors among them -- stays
    zero.  Onto a pattern: outside untouched bit for bit, inside fl(pattern + gradient onto zeros) to a few ulp of the larger of the two (the
    weight gradients are GEMMs that accumulate into the gradient buffer: the pattern is one more addend of their sums)"""
    bn = _Wide(*case)
    bn.fwd()
    zero = bn.bwd(0)
    inside = torch.zeros(bn.params.numel(), dtype=torch.bool, device="cuda")
    mid, ends = _mid_names(bn.net), []
    for n, o, shape in bn.net._layout:
        ends.append((o, o + torch.Size(shape).numel()))
        if n in mid:
            inside[o:o + torch.Size(shape).numel()] = True
    gaps = [b0 - a1 for (_, a1), (b0, _) in zip(ends, ends[1:])]
    assert min(gaps) >= 0 and max(gaps) <= 3 and ends[-1][1] <= bn.params.numel()
    assert bool((zero["@flat"][~inside] == 0).all())
    pre = (((torch.arange(bn.params.numel(), device="cuda") % 7) - 3).float() * 0.25)
    got = bn.bwd(0, grads=pre.clone())
    assert torch.equal(got["@flat"][~inside], pre[~inside])
    g0, g1 = zero["@flat"][inside], got["@flat"][inside]
    assert float(g0.abs().max()) > 0
    want = pre[inside].double() + g0.double()
    tol = 8 * 2.0 ** -24 * torch.maximum(torch.maximum(pre[inside].abs(), g0.abs()).double(), want.abs())
    assert bool(((g1.double() - want).abs() <= tol).all()), float(((g1.double() - want).abs() - tol).max())


@pytest.mark.gpu
def test_report_worst_ratios():
    """prints the worst err / d per quantity over the cases run so far in this process (DESIGN.md keeps the table); asserts nothing the case
    tests have not asserted"""
    for k, (r, e, where, t) in sorted(_KWORST.items()):
        print(f"kernel worst err/d  {k:10s} {r:8.2f}  (err {e:.2e}, {where}, {t})")
    for k, (r, e, where, t) in sorted(_WORST.items()):
        print(f"bottleneck worst err/d_k  {k:28s} {r:8.2f}  (err {e:.2e}, {where}, {t})")
