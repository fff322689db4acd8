"""The kernels between the CustomTransformer's GEMMs (csrc/k_tfm.hip), one at a time against float64 at their edges, through the stand-alone
entries dq_tfm_rope_add .. dq_tfm_seqsum (include/dq_hip.h: thin wrappers over the launchers dq_tfm_fwd / dq_tfm_bwd call).

tests/test_tfm.py judges these kernels through whole models by one number per tensor; from the code, what no test ran before this file:
k_layernorm_fwd_reg<16> / k_layernorm_bwd_rows_reg<16> (the fallback of 256 < H <= 1024 for H % 4 != 0 or a misaligned operand), the second trip
of every grid-stride loop (above 2^21 elements), k_layernorm_bwd_cols with more rows than LN_BWD_BLOCKS = 256, the two-launch gain / bias
reduction (db != dg + H), stats == nullptr, accumulate 0 against 1 per kernel, and the softmax's padding columns.

References: plain torch float64 on the CPU, written here (the RoPE tables alone come from oracle.dq_oracle_tfm: they are the kernels' INPUT);
every backward reference is held against float64 autograd of its forward (test_references_are_the_gradients_of_their_forwards).  Every buffer
a kernel writes lies between two bands of 64 floats of a sentinel that must be bit-identical afterwards (_Buf).

Bounds: err = max|got - ref| / max|ref| per tensor <= 16 d, d = the same distance of the same operation in torch fp32 on the CPU (one thread)
from float64, floored at 2^-24, never above 2e-5 (forward outputs) / 1e-4 (gradients): the whole-model allowances of tests/test_tfm.py, which a
single kernel must not use up.  16 is the factor of tests/test_mid_forms.py and tests/test_level_plan.py.  The CPU tests hold 16 d under the
caps for every case.  GELU and GELU' are measured the same way (absolute error over the tensor's largest entry, not per element: in the
negative tail 1 + erf cancels in fp32, in torch as in the kernel).  Bitwise claims need no bound: y = fp32(x + r); accumulate = 1 is
fp32(prefill + the accumulate = 0 result) because k_partial_reduce ends in ONE `out[i] + s`; a repeated launch repeats.

Observed errors on an MI355X and the mutations this file catches: DESIGN.md section 28."""
import contextlib
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from oracle import dq_oracle_tfm as OT  # rope_tables only

DEV = "cuda"
SENT = -2.5e33
_SENT_BITS = int(torch.tensor(SENT, dtype=torch.float32).view(torch.int32))
FACTOR, FLOOR = 16.0, 2.0 ** -24
CAP = {"act": 2e-5, "grad": 1e-4}  # tests/test_tfm.py: output / gradients of the whole model
REG4, REG16, BLK, ROWS = range(4)  # DQ_LN_*
FORM_NAMES = ("REG4", "REG16", "BLK", "ROWS")
LN_BWD_BLOCKS, COLSUM_BLOCKS, COND_BLOCKS = 256, 64, 64  # csrc/dq_tfm.h


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _one_thread():
    """the fp32 yardstick is ONE draw of a sum's rounding: the split of the sum over CPU threads must not pick it (tests/test_mid_forms.py)"""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(nt)


class _Buf:
    """n elements between two bands of a sentinel (64 before -- 65 with off1, so that the tensor starts one float past a 16-byte boundary -- and
    64 after); `t` is the tensor a kernel gets"""

    def __init__(self, n, init=None, off1=False, dtype=torch.float32):
        self.lo = 64 + int(off1)
        self.all = torch.full((self.lo + n + 64,), SENT if dtype == torch.float32 else -77, dtype=dtype, device=DEV)
        self.t = self.all[self.lo:self.lo + n]
        if init is not None:
            self.t.copy_(init.reshape(-1).to(dtype))
        self.before = self.all.clone()
        if DEV == "cuda":
            assert self.t.data_ptr() % 16 == (4 if off1 else 0)

    def intact(self):
        hi = self.lo + self.t.numel()
        view = (lambda v: v.view(torch.int32)) if self.all.dtype == torch.float32 else (lambda v: v)
        return torch.equal(view(self.all[:self.lo]), view(self.before[:self.lo])) and torch.equal(view(self.all[hi:]), view(self.before[hi:]))

    def unchanged(self):
        """an input: every bit as it was"""
        return torch.equal(self.all.view(torch.int32) if self.all.dtype == torch.float32 else self.all,
                           self.before.view(torch.int32) if self.all.dtype == torch.float32 else self.before)

    def cpu(self, *shape):
        return self.t.detach().cpu().clone().view(*shape)


def _launch(name, *args):
    """tensors (views included) go as their data pointers, None as NULL; the current stream is appended"""
    from dquartic import _native as N

    conv = [N.ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args]
    N.check(getattr(N.lib(), name)(*conv, N.stream_ptr()), name)


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max()) / float(ref.double().abs().max())


def _bound(d, kind):
    return min(FACTOR * max(d, FLOOR), CAP[kind])


_WORST = {}  # (kernel, form, tensor) -> (err, d, case): the table of DESIGN.md section 28


def _check(kernel, form, name, case, got, ref, d, kind):
    """one tensor against its float64 reference at 16 d; prints err and d; a NaN fails"""
    assert got.shape == ref.shape, (kernel, name, got.shape, ref.shape)
    if float(ref.abs().max()) == 0.0:  # (only where the test says the result is exactly zero)
        assert float(got.abs().max()) == 0.0, (kernel, form, name, case)
        return 0.0
    e, b = _rel(got, ref), _bound(d, kind)
    print(f"{kernel:18s} {form:5s} {name:8s} {str(case):28s} err {e:.2e}  d {d:.2e}  bound {b:.2e}")
    key = (kernel, form, name)
    if not e <= _WORST.get(key, (0.0,))[0]:
        _WORST[key] = (e, d, case)
    assert e <= b, (kernel, form, name, case, e, d, b)
    return e


def _yard(f32, f64):
    return {k: (_rel(f32[k], v) if float(v.abs().max()) > 0 else 0.0) for k, v in f64.items()}


def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 1000003 + int(v)
    return torch.Generator().manual_seed(s % (2 ** 62))


# ---------------------------------------------------------------------------------------------------------------------------------
# references: every function runs in the dtype of its arguments (float64: the reference, float32: the yardstick)
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_fwd(x, r, g, b):
    y = x if r is None else x + r
    mean = y.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean(-1, keepdim=True) + 1e-5)  # biased variance, eps inside the root (nn.LayerNorm)
    return {"y": y, "out": (y - mean) * rstd * g + b, "mean": mean[:, 0], "rstd": rstd[:, 0]}


def _ln_bwd(y, g, dout):
    """gradients of sum(dout * LayerNorm(y) * g + b) with respect to y, g, b"""
    mean = y.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
    xh, dxh = (y - mean) * rstd, dout * g
    dy = rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))
    return {"dy": dy, "dg": (dout * xh).sum(0), "db": dout.sum(0)}


def _softmax_fwd(s, scale):
    z = s * scale
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def _softmax_bwd(p, dp, scale):
    return p * (dp - (p * dp).sum(-1, keepdim=True)) * scale


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def _gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _rope(x, sin, cos, temb=None, inverse=False):
    """x (B, S, H): channel pairs (2j, 2j+1) rotated by the angle of (position, j); inverse: the transposed rotation"""
    x1, x2 = x[..., 0::2], x[..., 1::2]
    if inverse:
        o1, o2 = x1 * cos + x2 * sin, x2 * cos - x1 * sin
    else:
        o1, o2 = x1 * cos - x2 * sin, x1 * sin + x2 * cos
    out = torch.stack((o1, o2), dim=-1).reshape(x.shape)
    return out if temb is None or inverse else out + temb[:, None, :]


def _cond_fwd(xc, w, b, sin, cos):
    return _rope(xc[..., None] * w + b, sin, cos)


def _cond_bwd(dc, xc, w, sin, cos):
    d = _rope(dc, sin, cos, inverse=True)  # gradient at the Linear(1, H)'s output
    return {"dw": (d * xc[..., None]).sum((0, 1)), "db": d.sum((0, 1)), "dxc": (d * w).sum(-1)}


def _tables(S, H, dtype):
    sin, cos = OT.rope_tables(S, H)  # fp32: what the module hands the kernels
    return sin.to(dtype), cos.to(dtype)


def _time_freqs(H):
    half = H // 2
    return torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1)))


# ---------------------------------------------------------------------------------------------------------------------------------
# cases and their (cached, never written) data, references and yardsticks
# ---------------------------------------------------------------------------------------------------------------------------------
LN_H = (8, 64, 72, 256, 258, 260, 264, 1024, 1025, 1028)
LN_ROWS = (1, 3, 5, 257, 600)  # a partial last block of four waves; one and 2 1/3 trips of the 256-block column loop
LN_CASES = [(H, rows, False) for H in LN_H for rows in LN_ROWS] + \
           [(H, rows, True) for H in LN_H if 256 < H <= 1024 and H % 4 == 0 for rows in LN_ROWS]  # (off1: one float into the buffers)
_ln_id = lambda c: f"H{c[0]}-rows{c[1]}-{'off1' if c[2] else 'aligned'}"


def _ln_form(H, off1):
    """the form this file EXPECTS (asserted against dq_tfm_layernorm_form before every launch)"""
    if H <= 256:
        return REG4
    if H <= 1024:
        return BLK if H % 4 == 0 and not off1 else REG16
    return ROWS


@functools.lru_cache(maxsize=None)
def _ln_data(H, rows):
    g = _gen(1, H, rows)
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"x": 1.5 * rn(rows, H) + 3.0, "r": rn(rows, H), "g": rn(H), "b": rn(H), "dout": rn(rows, H), "dg0": rn(H), "db0": rn(H),
            "dy0": rn(rows, H)}


@functools.lru_cache(maxsize=None)
def _ln_ref(H, rows, with_r):
    """float64 references of a case, the fp32 inputs of its backward (y32 = fp32(x + r), stats of y32 formed in float64), and d per tensor"""
    D = _ln_data(H, rows)
    r = D["r"] if with_r else None
    dd = lambda t: None if t is None else t.double()
    y32 = D["x"] + r if with_r else D["x"].clone()
    f64 = _ln_fwd(dd(D["x"]), dd(r), dd(D["g"]), dd(D["b"]))
    s64 = _ln_fwd(y32.double(), None, dd(D["g"]), dd(D["b"]))
    f64.update(_ln_bwd(y32.double(), dd(D["g"]), dd(D["dout"])))
    with _one_thread():
        f32 = _ln_fwd(D["x"], r, D["g"], D["b"])
        f32.update(_ln_bwd(y32, D["g"], D["dout"]))
    d = _yard(f32, f64)
    return {"ref": f64, "d": d, "y32": y32, "stats32": torch.stack((s64["mean"], s64["rstd"]), dim=1).float()}


SM_ROWS, SM_N, SM_DH = (1, 3, 5, 130), (1, 5, 63, 64, 65, 130, 200), (4, 64)
_up4 = lambda v: (v + 3) // 4 * 4


def _sm_draw(rows, n, dh, k):
    g = _gen(2, rows, n, k)
    s = 30.0 * torch.randn(rows, n, generator=g)  # |scale * s| reaches ~60 at dh = 4: without the max subtraction the row sum leaves fp32's range
    if rows >= 3:
        s[1] = 7.25  # all equal: every entry fp32(1 / n)
        s[2] = -1e4  # one +1e4 among -1e4: one-hot, no NaN
        s[2, n // 2] = 1e4
    dp = torch.randn(rows, n, generator=g)
    scale = dh ** -0.5
    p64 = _softmax_fwd(s.double(), scale)
    p32 = p64.float()  # the backward's input
    ds64 = _softmax_bwd(p32.double(), dp.double(), scale)
    with _one_thread():
        d = _yard({"p": _softmax_fwd(s, scale), "ds": _softmax_bwd(p32, dp, scale)}, {"p": p64, "ds": ds64})
    return {"s": s, "dp": dp, "scale": scale, "p": p64, "p32": p32, "ds": ds64, "d": d, "draw": k}


@functools.lru_cache(maxsize=None)
def _sm_ref(rows, n, dh):
    """scores at std 30 make a row all but one-hot; when EVERY row of a case is (rows = 1: there is no all-equal row), ds = p (dp - sum p dp) is
    what is left of a cancellation -- max|ds| down to 1e-4 -- and fp32 itself is 1e-5 of it away from float64 (rows 1, n 65, dh 4 at draw 0).
    The condition on the inputs (docstring of the file): the first draw k = 0, 1, .. whose 16 d is under HALF the caps; the kernels' results
    have no part in it, and test_bounds_leave_room_rowwise_and_pointwise holds whatever draw was taken under the caps themselves"""
    for k in range(16):
        R = _sm_draw(rows, n, dh, k)
        if FACTOR * R["d"]["p"] < CAP["act"] / 2 and FACTOR * R["d"]["ds"] < CAP["grad"] / 2:
            return R
    raise AssertionError(("no well-conditioned softmax inputs in 16 draws", rows, n, dh))


GELU_BIG = 2 ** 21 + 3 * 256 + 5  # grid_for caps the grid at 8192 blocks of 256: the second grid-stride trip, 3 blocks and 5 lanes of it


@functools.lru_cache(maxsize=None)
def _gelu_ref(which):
    g = _gen(3, len(which))
    if which == "grid":
        x = torch.cat((torch.linspace(-12.0, 12.0, 4801), torch.tensor([0.0, -0.0, 1e-30, -5.5, -9.0])))
    else:
        x = 3.0 * torch.randn(GELU_BIG, generator=g)
    dy = torch.randn(x.numel(), generator=g)
    y64, dx64 = _gelu(x.double()), dy.double() * _gelu_grad(x.double())
    with _one_thread():
        d = _yard({"y": _gelu(x), "dx": dy * _gelu_grad(x)}, {"y": y64, "dx": dx64})
    return {"x": x, "dy": dy, "y": y64, "dx": dx64, "d": d}


ROPE_H, ROPE_BS = (8, 72, 1032), ((1, 1), (3, 5), (2, 70))
ROPE_BIG = (2, 33001, 64)  # B S H / 2 = 2^21 + 14912: a second grid-stride trip of 58 1/4 blocks; x is 16.9 MB
ROPE_CASES = [(B, S, H) for H in ROPE_H for B, S in ROPE_BS] + [ROPE_BIG]


@functools.lru_cache(maxsize=2)
def _rope_ref(B, S, H):
    g = _gen(4, B, S, H)
    x, yv, temb = torch.randn(B, S, H, generator=g), torch.randn(B, S, H, generator=g), torch.randn(B, H, generator=g)
    sin, cos = _tables(S, H, torch.float32)
    sd, cd = sin.double(), cos.double()
    f64 = {"fwd": _rope(x.double(), sd, cd), "fwd_t": _rope(x.double(), sd, cd, temb.double()), "inv": _rope(yv.double(), sd, cd, inverse=True)}
    with _one_thread():
        f32 = {"fwd": _rope(x, sin, cos), "fwd_t": _rope(x, sin, cos, temb), "inv": _rope(yv, sin, cos, inverse=True)}
    return {"x": x, "y": yv, "temb": temb, "sin": sin, "cos": cos, "ref": f64, "d": _yard(f32, f64)}


COND_BS = {1: (1, 1), 7: (1, 7), 64: (2, 32), 65: (5, 13), 130: (2, 65)}  # rows = B S2: nb = min(rows, 64) partials at 1, 7, 64; a second trip
COND_CASES = [(H, rows) for H in ROPE_H for rows in COND_BS]


@functools.lru_cache(maxsize=None)
def _cond_ref(H, rows):
    B, S = COND_BS[rows]
    g = _gen(5, H, rows)
    rn = lambda *s: torch.randn(*s, generator=g)
    D = {"xc": rn(B, S), "w": rn(H), "b": rn(H), "dc": rn(B, S, H), "dw0": rn(H), "db0": rn(H)}
    sin, cos = _tables(S, H, torch.float32)
    dd = lambda k: D[k].double()
    f64 = {"c": _cond_fwd(dd("xc"), dd("w"), dd("b"), sin.double(), cos.double())}
    f64.update(_cond_bwd(dd("dc"), dd("xc"), dd("w"), sin.double(), cos.double()))
    with _one_thread():
        f32 = {"c": _cond_fwd(D["xc"], D["w"], D["b"], sin, cos)}
        f32.update(_cond_bwd(D["dc"], D["xc"], D["w"], sin, cos))
    D.update({"sin": sin, "cos": cos, "ref": f64, "d": _yard(f32, f64), "B": B, "S": S})
    return D


@functools.lru_cache(maxsize=1)
def _cond_big_ref():
    """k_cond_embed's own second grid-stride trip: the shape of ROPE_BIG, forward only"""
    B, S, H = ROPE_BIG
    g = _gen(9, B, S, H)
    xc, w, b = torch.randn(B, S, generator=g), torch.randn(H, generator=g), torch.randn(H, generator=g)
    sin, cos = _tables(S, H, torch.float32)
    c64 = _cond_fwd(xc.double(), w.double(), b.double(), sin.double(), cos.double())
    with _one_thread():
        d = _yard({"c": _cond_fwd(xc, w, b, sin, cos)}, {"c": c64})
    return {"xc": xc, "w": w, "b": b, "sin": sin, "cos": cos, "c": c64, "d": d}


TIME_CASES = ((1, 8), (3, 200), (5, 1032))  # B H / 2 = 4, 300, 2580: one block, a partial second, eleven
TIME_T = (0, 1, 400, 999)


@functools.lru_cache(maxsize=None)
def _time_ref(B, H):
    t = torch.tensor([TIME_T[i % 4] for i in range(B)], dtype=torch.int64)
    f = _time_freqs(H)
    a = t[:, None].float() * f[None, :]  # fp32, as the kernel and the reference module form it; sin and cos of THAT angle in float64
    e64 = torch.cat((torch.sin(a.double()), torch.cos(a.double())), dim=1)
    with _one_thread():
        d = _yard({"e": torch.cat((torch.sin(a), torch.cos(a)), dim=1)}, {"e": e64})
    return {"t": t, "f": f, "e": e64, "d": d}


COLSUM_M, COLSUM_N = (1, 7, 64, 65, 200), (1, 255, 256, 257)
SEQSUM_CASES = ((1, 1, 8), (3, 70, 100), (2, 5, 257))


@functools.lru_cache(maxsize=None)
def _colsum_ref(M, N):
    g = _gen(6, M, N)
    x = torch.randn(M, N + 4, generator=g) + 0.25  # (off zero mean: a column sum that cancels to nothing would make max|ref| a draw)
    out0 = torch.randn(N, generator=g)
    s64 = x[:, :N].double().sum(0)
    with _one_thread():
        d = _yard({"s": x[:, :N].sum(0)}, {"s": s64})
    return {"x": x, "out0": out0, "s": s64, "d": d}


@functools.lru_cache(maxsize=None)
def _seqsum_ref(B, S, N):
    x = torch.randn(B, S, N, generator=_gen(7, B, S, N)) + 0.25
    s64 = x.double().sum(1)
    with _one_thread():
        d = _yard({"s": x.sum(1)}, {"s": s64})
    return {"x": x, "s": s64, "d": d}


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_layernorm_form_table():
    """dq_tfm_layernorm_form: the one rule both launchers take; every form has a case in LN_CASES"""
    from dquartic import _native as N

    form = N.lib().dq_tfm_layernorm_form
    for H in (8, 256):
        assert form(H, 1) == form(H, 0) == REG4
    for H in (260, 1024):
        assert form(H, 1) == BLK and form(H, 0) == REG16
    assert form(258, 1) == form(258, 0) == REG16
    for H in (1025, 1028):
        assert form(H, 1) == form(H, 0) == ROWS
    assert form(0, 1) == -1
    for H, rows, off1 in LN_CASES:
        assert form(H, int(not off1)) == _ln_form(H, off1), (H, off1)
    assert {_ln_form(H, off1) for H, _, off1 in LN_CASES} == {REG4, REG16, BLK, ROWS}


def test_entries_refuse_before_any_device_call():
    """null operands, an odd H where pairs are rotated, a short scratch: refused on the host (this test runs without a GPU)"""
    from dquartic import _native as N

    lib = N.lib()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused first
    bad = lambda rc, word: rc != 0 and word in N.last_error()
    assert bad(lib.dq_tfm_rope_add(p, p, p, None, 2, 3, 7, 0, None), "even")
    assert bad(lib.dq_tfm_rope_add(None, p, p, None, 2, 3, 8, 0, None), "null")
    assert bad(lib.dq_tfm_rope_add(p, None, p, None, 2, 3, 8, 0, None), "null")
    assert bad(lib.dq_tfm_cond_embed(p, p, p, p, p, p, 2, 3, 9, None), "even")
    assert bad(lib.dq_tfm_cond_embed(p, p, p, p, p, None, 2, 3, 8, None), "null")
    assert bad(lib.dq_tfm_cond_embed_bwd(p, p, p, p, p, p, p, None, p, 2 * 8 * 64 - 1, 2, 3, 8, 0, None), "scratch")
    assert bad(lib.dq_tfm_cond_embed_bwd(p, p, p, p, p, p, p, None, p, 2 * 8 * 64, 2, 3, 7, 0, None), "even")
    assert bad(lib.dq_tfm_cond_embed_bwd(p, p, p, p, p, None, p, None, p, 2 * 8 * 64, 2, 3, 8, 0, None), "null")
    assert bad(lib.dq_tfm_time_features(p, p, None, 2, 8, None), "null") and bad(lib.dq_tfm_time_features(p, p, p, 2, 7, None), "even")
    assert bad(lib.dq_tfm_gelu(p, None, 4, None), "null") and bad(lib.dq_tfm_gelu_bwd(p, p, None, 4, None), "null")
    assert bad(lib.dq_tfm_layernorm_fwd(p, None, p, p, p, None, None, 3, 8, None), "null")
    assert bad(lib.dq_tfm_layernorm_fwd(p, None, p, p, p, p, None, 0, 8, None), "positive")
    assert bad(lib.dq_tfm_layernorm_bwd(p, p, p, p, p, p, p, p, 2 * 8 * LN_BWD_BLOCKS - 1, 3, 8, 0, None), "scratch")
    assert bad(lib.dq_tfm_layernorm_bwd(p, None, p, p, p, p, p, p, 2 * 8 * LN_BWD_BLOCKS, 3, 8, 0, None), "null")
    assert bad(lib.dq_tfm_softmax_rows(None, 3, 5, 8, 0.5, None), "null") and bad(lib.dq_tfm_softmax_rows(p, 3, 9, 8, 0.5, None), "ld")
    assert bad(lib.dq_tfm_softmax_rows_bwd(p, None, 3, 5, 8, 0.5, None), "null")
    assert bad(lib.dq_tfm_colsum(p, 3, 5, 5, p, p, COLSUM_BLOCKS * 5 - 1, 0, None), "scratch")
    assert bad(lib.dq_tfm_colsum(p, 3, 5, 4, p, p, COLSUM_BLOCKS * 5, 0, None), "ld") and bad(lib.dq_tfm_colsum(p, 3, 5, 5, None, p, 999, 0, None), "null")
    assert bad(lib.dq_tfm_seqsum(p, 2, 3, 4, None, None), "null") and bad(lib.dq_tfm_seqsum(p, 2, 0, 4, p, None), "positive")


def _close12(a, b):
    assert _rel(a, b) < 1e-12, _rel(a, b)


def test_references_are_the_gradients_of_their_forwards():
    """every backward reference above equals torch float64 autograd of the matching forward to 1e-12 (this validates them without a GPU)"""
    g = _gen(8)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    # LayerNorm
    y, gn, b, dout = (1.5 * rn(7, 72) + 3).requires_grad_(), rn(72).requires_grad_(), rn(72).requires_grad_(), rn(7, 72)
    gr = torch.autograd.grad(_ln_fwd(y, None, gn, b)["out"], (y, gn, b), grad_outputs=dout)
    mine = _ln_bwd(y.detach(), gn.detach(), dout)
    for a, k in zip(gr, ("dy", "dg", "db")):
        _close12(mine[k], a)
    # softmax
    s, dp = (30 * rn(5, 65)).requires_grad_(), rn(5, 65)
    p = _softmax_fwd(s, 0.125)
    _close12(_softmax_bwd(p.detach(), dp, 0.125), torch.autograd.grad(p, s, grad_outputs=dp)[0])
    _close12(p.detach(), torch.softmax(s.detach() * 0.125, dim=-1))
    # GELU'
    x = torch.cat((torch.linspace(-12, 12, 481, dtype=torch.float64), rn(50))).requires_grad_()
    _close12(_gelu_grad(x.detach()), torch.autograd.grad(_gelu(x).sum(), x)[0])
    _close12(_gelu(x.detach()), torch.nn.functional.gelu(x.detach()))
    # RoPE inverse = the transpose = the gradient of the forward
    sin, cos = _tables(9, 72, torch.float64)
    x, yv = rn(3, 9, 72).requires_grad_(), rn(3, 9, 72)
    _close12(_rope(yv, sin, cos, inverse=True), torch.autograd.grad(_rope(x, sin, cos, rn(3, 72)), x, grad_outputs=yv)[0])
    assert _rel(_rope(x.detach().float(), sin.float(), cos.float()), OT.apply_rope(x.detach().float())) < 1e-6  # the module's pairing
    # conditional embedding
    xc, w, bb, dc = rn(3, 9).requires_grad_(), rn(72).requires_grad_(), rn(72).requires_grad_(), rn(3, 9, 72)
    gr = torch.autograd.grad(_cond_fwd(xc, w, bb, sin, cos), (w, bb, xc), grad_outputs=dc)
    mine = _cond_bwd(dc, xc.detach(), w.detach(), sin, cos)
    for a, k in zip(gr, ("dw", "db", "dxc")):
        _close12(mine[k], a)


def _report(label, ds):
    worst = {}
    for d in ds:
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"fp32 torch vs float64, {label}: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    return worst


_KIND = {"out": "act", "mean": "act", "rstd": "act", "y": "act", "p": "act", "fwd": "act", "fwd_t": "act", "c": "act", "e": "act"}


def _assert_room(ds):
    for d in ds:
        for k, v in d.items():
            assert FACTOR * v < CAP[_KIND.get(k, "grad")], (k, v)


def test_bounds_leave_room_layernorm():
    """16 d under the caps for every (H, rows) and tensor; r null and non-null"""
    ds = [_ln_ref(H, rows, wr)["d"] for H in LN_H for rows in LN_ROWS for wr in (True, False)]
    _report("LayerNorm", ds)
    _assert_room(ds)


def test_bounds_leave_room_rowwise_and_pointwise():
    """16 d under the caps for the softmax, GELU, RoPE, conditional-embedding, time-feature and sum cases"""
    fam = {"softmax": [_sm_ref(r, n, dh)["d"] for r in SM_ROWS for n in SM_N for dh in SM_DH],
           "gelu": [_gelu_ref(w)["d"] for w in ("grid", "big")],
           "rope": [_rope_ref(*c)["d"] for c in ROPE_CASES],
           "cond_embed": [_cond_ref(*c)["d"] for c in COND_CASES] + [_cond_big_ref()["d"]],
           "time": [_time_ref(*c)["d"] for c in TIME_CASES],
           "colsum": [_colsum_ref(M, N)["d"] for M in COLSUM_M for N in COLSUM_N],
           "seqsum": [_seqsum_ref(*c)["d"] for c in SEQSUM_CASES]}
    for label, ds in fam.items():
        _report(label, ds)
        _assert_room(ds)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def _assert_ln_form(H, off1):
    from dquartic import _native as N

    form = _ln_form(H, off1)
    assert N.lib().dq_tfm_layernorm_form(H, int(not off1)) == form
    return FORM_NAMES[form]


def _ln_fwd_gpu(H, rows, off1, x, r, g, b, stats=True):
    """one forward launch; returns y, out (rows, H), stats (rows, 2) or None on the CPU; bands and inputs asserted"""
    _assert_ln_form(H, off1)
    X, G, Bb = _Buf(rows * H, x, off1), _Buf(H, g, off1), _Buf(H, b, off1)
    R = _Buf(rows * H, r, off1) if r is not None else None
    Y, O = _Buf(rows * H, None, off1), _Buf(rows * H, None, off1)
    St = _Buf(rows * 2) if stats else None
    _launch("dq_tfm_layernorm_fwd", X.t, R.t if R else None, G.t, Bb.t, Y.t, O.t, St.t if St else None, rows, H)
    for buf in (Y, O) + ((St,) if St else ()):
        assert buf.intact()
    for buf in (X, G, Bb) + ((R,) if R else ()):
        assert buf.unchanged()
    return Y.cpu(rows, H), O.cpu(rows, H), St.cpu(rows, 2) if St else None


def _ln_bwd_gpu(H, rows, off1, y32, stats32, D, adjacent, acc):
    """one backward launch: dy, dg, db on the CPU.  dy, dg, db start from the prefills dy0, dg0, db0 (dy is a plain store in either mode)"""
    _assert_ln_form(H, off1)
    Y, G, Do = _Buf(rows * H, y32, off1), _Buf(H, D["g"], off1), _Buf(rows * H, D["dout"], off1)
    St = _Buf(rows * 2, stats32)
    Dy = _Buf(rows * H, D["dy0"], off1)
    if adjacent:
        Dgb = _Buf(2 * H, torch.cat((D["dg0"], D["db0"])))
        dg, db, outs = Dgb.t[:H], Dgb.t[H:], (Dgb,)
    else:
        Dg, Db = _Buf(H, D["dg0"]), _Buf(H, D["db0"])
        dg, db, outs = Dg.t, Db.t, (Dg, Db)
        assert db.data_ptr() != dg.data_ptr() + 4 * H
    Sc = _Buf(2 * H * LN_BWD_BLOCKS)
    _launch("dq_tfm_layernorm_bwd", Y.t, St.t, G.t, Do.t, Dy.t, dg, db, Sc.t, Sc.t.numel(), rows, H, acc)
    for buf in (Dy, Sc) + outs:
        assert buf.intact()
    for buf in (Y, G, Do, St):
        assert buf.unchanged()
    return {"dy": Dy.cpu(rows, H), "dg": dg.detach().cpu().clone(), "db": db.detach().cpu().clone()}


def _ln_case(H, rows, off1):
    """everything of one case, checked; returns the tensors the BLK / REG16 comparison needs"""
    form = _assert_ln_form(H, off1)
    D = _ln_data(H, rows)
    case = _ln_id((H, rows, off1))
    keep = {}
    for with_r in (True, False):
        R = _ln_ref(H, rows, with_r)
        r = D["r"] if with_r else None
        y, out, st = _ln_fwd_gpu(H, rows, off1, D["x"], r, D["g"], D["b"])
        assert torch.equal(y, R["y32"]), "y is not fp32(x + r)"
        tag = "" if with_r else "/r0"
        _check("layernorm_fwd", form, "out" + tag, case, out, R["ref"]["out"], R["d"]["out"], "act")
        _check("layernorm_fwd", form, "mean" + tag, case, st[:, 0], R["ref"]["mean"], R["d"]["mean"], "act")
        _check("layernorm_fwd", form, "rstd" + tag, case, st[:, 1], R["ref"]["rstd"], R["d"]["rstd"], "act")
        y2, out2, st2 = _ln_fwd_gpu(H, rows, off1, D["x"], r, D["g"], D["b"])
        assert torch.equal(y2, y) and torch.equal(out2, out) and torch.equal(st2, st), "the forward does not repeat"
        y3, out3, _ = _ln_fwd_gpu(H, rows, off1, D["x"], r, D["g"], D["b"], stats=False)
        assert torch.equal(y3, y) and torch.equal(out3, out), "stats == NULL changes the result"
        if with_r:
            keep["out"] = out
    R = _ln_ref(H, rows, True)
    base = _ln_bwd_gpu(H, rows, off1, R["y32"], R["stats32"], D, adjacent=True, acc=0)
    for k in ("dy", "dg", "db"):
        _check("layernorm_bwd", form, k, case, base[k], R["ref"][k], R["d"][k], "grad")
    for adjacent, acc in ((True, 0), (False, 0), (True, 1), (False, 1)):
        got = _ln_bwd_gpu(H, rows, off1, R["y32"], R["stats32"], D, adjacent, acc)
        what = f"adjacent={adjacent} accumulate={acc}"
        assert torch.equal(got["dy"], base["dy"]), what
        if acc:  # the kernel's last operation is out[i] + s
            assert torch.equal(got["dg"], D["dg0"] + base["dg"]) and torch.equal(got["db"], D["db0"] + base["db"]), what
        else:
            assert torch.equal(got["dg"], base["dg"]) and torch.equal(got["db"], base["db"]), what
    keep.update(base)
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_layernorm_forms_against_float64(case):
    """forward (r null / non-null, stats null / non-null) and backward (dg, db adjacent / separate, accumulate 0 / 1) of one (H, rows) in
    the form asserted from dq_tfm_layernorm_form; the off1 cases also hold REG16 against BLK on the same numbers"""
    H, rows, off1 = case
    got = _ln_case(H, rows, off1)
    if off1:
        R = _ln_ref(H, rows, True)
        assert _assert_ln_form(H, False) == "BLK" and _assert_ln_form(H, True) == "REG16"
        blk = _ln_case(H, rows, False)
        for k, kind in (("out", "act"), ("dy", "grad"), ("dg", "grad"), ("db", "grad")):
            e = float((got[k].double() - blk[k].double()).abs().max()) / float(R["ref"][k].abs().max())
            assert e <= _bound(R["d"][k], kind), ("REG16 against BLK", k, e)


@pytest.mark.gpu
@pytest.mark.parametrize("H,off1", [(64, False), (260, False), (260, True), (1028, False)], ids=lambda v: str(v))
def test_layernorm_all_zero_row(H, off1):
    """an all-zero row with r null: mean 0, variance 0, so out = 0 * rstd * g + b = b bit for bit and rstd = 1 / sqrt(1e-5) as fp32 evaluates it
    (fp32 eps, correctly rounded root and quotient: 316.22778; the double value rounded once would be 316.22775)"""
    _assert_ln_form(H, off1)
    rows = 5
    D = _ln_data(H, rows)
    x = D["x"].clone()
    x[2] = 0.0
    y, out, st = _ln_fwd_gpu(H, rows, off1, x, None, D["g"], D["b"])
    assert torch.equal(y, x)
    assert torch.equal(out[2], D["b"])
    assert float(st[2, 0]) == 0.0
    assert float(st[2, 1]) == float(np.float32(1.0) / np.sqrt(np.float32(1e-5)))
    assert torch.isfinite(out).all() and torch.isfinite(st).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: softmax
# ---------------------------------------------------------------------------------------------------------------------------------
def _padded(vals, ld):
    """(rows, ld) with the sentinel in the padding columns"""
    m = torch.full((vals.shape[0], ld), SENT)
    m[:, :vals.shape[1]] = vals
    return m


def _padding_intact(buf, rows, n, ld):
    pad = buf.t.view(rows, ld)[:, n:]
    return bool((pad.contiguous().view(torch.int32) == _SENT_BITS).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n", SM_N)
@pytest.mark.parametrize("rows", SM_ROWS)
def test_softmax_rows_against_float64(rows, n):
    for ld in (_up4(n), n + 8):
        for dh in SM_DH:
            R = _sm_ref(rows, n, dh)
            case = f"rows{rows}-n{n}-ld{ld}-dh{dh}"
            # forward, in place
            P = _Buf(rows * ld, _padded(R["s"], ld))
            _launch("dq_tfm_softmax_rows", P.t, rows, n, ld, R["scale"])
            assert P.intact() and _padding_intact(P, rows, n, ld), "the forward wrote outside its n columns"
            p = P.cpu(rows, ld)[:, :n]
            assert torch.isfinite(p).all()
            _check("softmax_rows", "", "p", case, p, R["p"], R["d"]["p"], "act")
            assert float((p.double().sum(-1) - 1.0).abs().max()) <= n * 2.0 ** -23
            if rows >= 3:
                assert torch.equal(p[1], torch.full((n,), float(np.float32(1.0) / np.float32(n)))), "an all-equal row is not fp32(1 / n)"
                hot = torch.zeros(n)
                hot[n // 2] = 1.0
                assert torch.equal(p[2], hot), "one +1e4 among -1e4 is not one-hot"
            P2 = _Buf(rows * ld, _padded(R["s"], ld))
            _launch("dq_tfm_softmax_rows", P2.t, rows, n, ld, R["scale"])
            assert torch.equal(P2.cpu(rows, ld)[:, :n], p)
            # backward, in place of dp
            Pin, Dp = _Buf(rows * ld, _padded(R["p32"], ld)), _Buf(rows * ld, _padded(R["dp"], ld))
            _launch("dq_tfm_softmax_rows_bwd", Pin.t, Dp.t, rows, n, ld, R["scale"])
            assert Dp.intact() and _padding_intact(Dp, rows, n, ld) and Pin.unchanged(), "the backward wrote outside its n columns"
            ds = Dp.cpu(rows, ld)[:, :n]
            _check("softmax_rows_bwd", "", "ds", case, ds, R["ds"], R["d"]["ds"], "grad")  # (n = 1: p = 1, t = dp exactly, ds = 0 exactly)
            # a row of ds sums to 0: sum ds = scale (t' - t sum p) with t' the kernel's fp32 dot product (n fused multiply-adds and a 6-level
            # wave sum: |t' - t| <= (n + 6) u sum|p dp|), each entry two roundings (2 u |ds_i|), u = 2^-24; sum p = 1 within u
            u, pd, dpd = 2.0 ** -24, R["p32"].double(), R["dp"].double()
            room = 1.01 * u * ((n + 6) * R["scale"] * (pd * dpd).abs().sum(-1) + 2 * R["ds"].abs().sum(-1) + R["scale"] * (pd * dpd).sum(-1).abs())
            assert bool((ds.double().sum(-1).abs() <= room).all()), (case, ds.double().sum(-1).abs().max(), room.min())


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: GELU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["grid", "big"])
def test_gelu_and_its_derivative_against_float64(which):
    """grid: [-12, 12] in steps of 0.005 and {0, -0, 1e-30, -5.5, -9}; big: 2^21 + 773 elements (the second grid-stride trip), all of it and
    its last 1024 on their own.  GELU' with dx apart from dy and in place of it, as the model calls it: bit for bit the same"""
    R = _gelu_ref(which)
    n = R["x"].numel()
    X, Y = _Buf(n, R["x"]), _Buf(n)
    _launch("dq_tfm_gelu", X.t, Y.t, n)
    assert Y.intact() and X.unchanged()
    y = Y.cpu(n)
    _check("gelu", "", "y", which, y, R["y"], R["d"]["y"], "act")
    Dy, Dx = _Buf(n, R["dy"]), _Buf(n)
    _launch("dq_tfm_gelu_bwd", X.t, Dy.t, Dx.t, n)
    assert Dx.intact() and Dy.unchanged() and X.unchanged()
    dx = Dx.cpu(n)
    _check("gelu_bwd", "", "dx", which, dx, R["dx"], R["d"]["dx"], "grad")
    if which == "big":  # the tail alone: against the WHOLE tensor's largest entry and bound (a tail that was never written is O(1) off)
        for name, got, ref, kind in (("y", y, R["y"], "act"), ("dx", dx, R["dx"], "grad")):
            e = float((got[-1024:].double() - ref[-1024:]).abs().max()) / float(ref.abs().max())
            assert e <= _bound(R["d"][name], kind), (name, "last 1024", e)
    _launch("dq_tfm_gelu_bwd", X.t, Dy.t, Dy.t, n)  # dx == dy (csrc/dq_tfm.hip: launch_gelu_bwd(.., w.dh, w.dh, ..))
    assert Dy.intact()
    assert torch.equal(Dy.cpu(n), dx), "GELU' in place of dy differs from GELU' into another tensor"
    Y2 = _Buf(n)
    _launch("dq_tfm_gelu", X.t, Y2.t, n)
    assert torch.equal(Y2.cpu(n), y)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: RoPE (+ time embedding), conditional embedding, time features
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ROPE_CASES, ids=lambda c: f"B{c[0]}-S{c[1]}-H{c[2]}")
def test_rope_add_and_its_inverse_against_float64(case):
    B, S, H = case
    R = _rope_ref(B, S, H)
    n = B * S * H
    sin, cos, temb = R["sin"].to(DEV), R["cos"].to(DEV), R["temb"].to(DEV)

    def run(src, t, inverse):
        X = _Buf(n, src)
        _launch("dq_tfm_rope_add", X.t, sin, cos, t, B, S, H, inverse)
        assert X.intact()
        return X.cpu(B, S, H)

    fwd, fwd_t, inv = run(R["x"], None, 0), run(R["x"], temb, 0), run(R["y"], None, 1)
    assert torch.equal(sin.cpu(), R["sin"]) and torch.equal(temb.cpu(), R["temb"])
    _check("rope_add", "", "fwd", case, fwd, R["ref"]["fwd"], R["d"]["fwd"], "act")
    _check("rope_add", "", "fwd+temb", case, fwd_t, R["ref"]["fwd_t"], R["d"]["fwd_t"], "act")
    _check("rope_add", "", "inverse", case, inv, R["ref"]["inv"], R["d"]["inv"], "grad")
    assert torch.equal(fwd[:, 0], R["x"][:, 0]), "position 0 (sin 0, cos 1) is not the identity"
    assert torch.equal(run(R["y"], temb, 1), inv), "the inverse reads temb"
    assert torch.equal(run(R["x"], temb, 0), fwd_t)
    bf, bi = _bound(R["d"]["fwd"], "act"), _bound(R["d"]["inv"], "grad")
    xd, yd = R["x"].double(), R["y"].double()
    # <R x, y> = <x, R^T y>: every entry of R x is within bf max|R x| and every entry of R^T y within bi max|R^T y| of its float64 value
    lhs, rhs = float((fwd.double() * yd).sum()), float((xd * inv.double()).sum())
    room = bf * float(R["ref"]["fwd"].abs().max()) * float(yd.abs().sum()) + bi * float(R["ref"]["inv"].abs().max()) * float(xd.abs().sum())
    assert abs(lhs - rhs) <= room, (lhs, rhs, room)
    # inverse(forward(x)) = x: the forward's error (<= bf max|R x| per entry, sqrt 2 of it after a rotation of the pair) plus the inverse's own
    back = run(fwd, None, 1)
    e = float((back.double() - xd).abs().max()) / float(xd.abs().max())
    assert e <= math.sqrt(2.0) * bf * float(R["ref"]["fwd"].abs().max()) / float(xd.abs().max()) + bi, e


@pytest.mark.gpu
@pytest.mark.parametrize("case", COND_CASES, ids=lambda c: f"H{c[0]}-rows{c[1]}")
def test_cond_embed_and_its_backward_against_float64(case):
    H, rows = case
    R = _cond_ref(H, rows)
    B, S = R["B"], R["S"]
    sin, cos = R["sin"].to(DEV), R["cos"].to(DEV)
    Xc, W, Bi = _Buf(rows, R["xc"]), _Buf(H, R["w"]), _Buf(H, R["b"])
    C = _Buf(rows * H)
    _launch("dq_tfm_cond_embed", Xc.t, W.t, Bi.t, sin, cos, C.t, B, S, H)
    assert C.intact() and Xc.unchanged() and W.unchanged() and Bi.unchanged()
    c = C.cpu(B, S, H)
    _check("cond_embed", "", "c", case, c, R["ref"]["c"], R["d"]["c"], "act")
    C2 = _Buf(rows * H)
    _launch("dq_tfm_cond_embed", Xc.t, W.t, Bi.t, sin, cos, C2.t, B, S, H)
    assert torch.equal(C2.cpu(B, S, H), c)

    def bwd(with_dx, acc):
        Dc, Dw, Db = _Buf(rows * H, R["dc"]), _Buf(H, R["dw0"]), _Buf(H, R["db0"])
        Dx = _Buf(rows) if with_dx else None
        Sc = _Buf(2 * H * COND_BLOCKS)
        _launch("dq_tfm_cond_embed_bwd", Dc.t, Xc.t, W.t, sin, cos, Dw.t, Db.t, Dx.t if Dx else None, Sc.t, Sc.t.numel(), B, S, H, acc)
        for buf in (Dw, Db, Sc) + ((Dx,) if Dx else ()):
            assert buf.intact()
        assert Dc.unchanged() and Xc.unchanged() and W.unchanged()
        return Dw.cpu(H), Db.cpu(H), Dx.cpu(B, S) if Dx else None

    dw, db, dxc = bwd(True, 0)
    _check("cond_embed_bwd", "", "dw", case, dw, R["ref"]["dw"], R["d"]["dw"], "grad")
    _check("cond_embed_bwd", "", "db", case, db, R["ref"]["db"], R["d"]["db"], "grad")
    _check("cond_embed_bwd", "", "dx_cond", case, dxc, R["ref"]["dxc"], R["d"]["dxc"], "grad")
    for with_dx, acc in ((True, 0), (False, 0), (True, 1), (False, 1)):
        w2, b2, x2 = bwd(with_dx, acc)
        what = f"dx_cond={with_dx} accumulate={acc}"
        if acc:  # k_partial_reduce ends in out[i] + s
            assert torch.equal(w2, R["dw0"] + dw) and torch.equal(b2, R["db0"] + db), what
        else:
            assert torch.equal(w2, dw) and torch.equal(b2, db), what
        assert x2 is None or torch.equal(x2, dxc), what  # (dx_cond is a plain store in either mode)


@pytest.mark.gpu
def test_cond_embed_second_grid_stride_trip():
    """B S2 H / 2 = 2^21 + 14912 (the issue's list has this size for k_rope_add and k_gelu only; k_cond_embed has the same loop and cap)"""
    B, S, H = ROPE_BIG
    R = _cond_big_ref()
    Xc, W, Bi, C = _Buf(B * S, R["xc"]), _Buf(H, R["w"]), _Buf(H, R["b"]), _Buf(B * S * H)
    _launch("dq_tfm_cond_embed", Xc.t, W.t, Bi.t, R["sin"].to(DEV), R["cos"].to(DEV), C.t, B, S, H)
    assert C.intact() and Xc.unchanged()
    c = C.cpu(B, S, H)
    _check("cond_embed", "", "c", ROPE_BIG, c, R["c"], R["d"]["c"], "act")
    e = float((c[-1, -64:].double() - R["c"][-1, -64:]).abs().max()) / float(R["c"].abs().max())  # the last 4096 elements on their own
    assert e <= _bound(R["d"]["c"], "act"), e


@pytest.mark.gpu
@pytest.mark.parametrize("B,H", TIME_CASES)
def test_time_features_against_float64(B, H):
    R = _time_ref(B, H)
    T, F, E = _Buf(B, R["t"], dtype=torch.int64), _Buf(H // 2, R["f"]), _Buf(B * H)
    _launch("dq_tfm_time_features", T.t, F.t, E.t, B, H)
    assert E.intact() and T.unchanged() and F.unchanged()
    e = E.cpu(B, H)
    _check("time_features", "", "e", f"B{B}-H{H}", e, R["e"], R["d"]["e"], "act")
    for b in range(B):
        if int(R["t"][b]) == 0:
            assert torch.equal(e[b, :H // 2], torch.zeros(H // 2)) and torch.equal(e[b, H // 2:], torch.ones(H // 2)), "t = 0 is not (0, 1)"
    E2 = _Buf(B * H)
    _launch("dq_tfm_time_features", T.t, F.t, E2.t, B, H)
    assert torch.equal(E2.cpu(B, H), e)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: column and sequence sums
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", COLSUM_N)
@pytest.mark.parametrize("M", COLSUM_M)
def test_colsum_against_float64(M, N):
    """M <= 64: the rows are the partial vectors (k_partial_reduce alone: the eight-wide body and its tail at M = 1, 7, 64); above, k_colsum first"""
    R = _colsum_ref(M, N)
    for ld in (N, N + 4):
        x = R["x"][:, :ld].contiguous()
        X = _Buf(M * ld, x)

        def run(acc):
            O, Sc = _Buf(N, R["out0"]), _Buf(COLSUM_BLOCKS * N)
            _launch("dq_tfm_colsum", X.t, M, N, ld, O.t, Sc.t, Sc.t.numel(), acc)
            assert O.intact() and Sc.intact() and X.unchanged()
            return O.cpu(N)

        s = run(0)
        _check("colsum", "rows" if M <= COLSUM_BLOCKS else "parts", "out", f"M{M}-N{N}-ld{ld}", s, R["s"], R["d"]["s"], "grad")
        assert torch.equal(run(0), s)
        assert torch.equal(run(1), R["out0"] + s), "accumulate = 1 is not fp32(out + the accumulate = 0 sum)"


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,N", SEQSUM_CASES)
def test_seqsum_against_float64(B, S, N):
    R = _seqsum_ref(B, S, N)
    X = _Buf(B * S * N, R["x"])

    def run():
        O = _Buf(B * N)
        _launch("dq_tfm_seqsum", X.t, B, S, N, O.t)
        assert O.intact() and X.unchanged()
        return O.cpu(B, N)

    s = run()
    _check("seqsum", "", "out", f"B{B}-S{S}-N{N}", s, R["s"], R["d"]["s"], "grad")
    assert torch.equal(run(), s)


@pytest.mark.gpu
def test_report_worst_errors():
    """prints the worst error per (kernel, form, tensor) over the cases run so far in this process (DESIGN.md section 28 keeps the table);
    asserts nothing the case tests have not asserted"""
    for (kernel, form, name), (e, d, case) in sorted(_WORST.items()):
        print(f"worst  {kernel:18s} {form:5s} {name:10s} err {e:.2e}  d {d:.2e}  err/max(d, 2^-24) {e / max(d, FLOOR):6.2f}  ({case})")
