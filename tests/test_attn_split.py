"""The bottleneck attention's three kernels (k_attn_fwd, k_attn_bwd_q, k_attn_bwd_kv: every 32 x 32 product in the six-term split-bf16
form, csrc/k_attn.hip) through the stand-alone entry points dq_attn_fwd / dq_attn_bwd, against a float64 evaluation of the same formulas
(torch on the CPU).

Inputs: ``default`` -- standard normal q, k, v, dO; ``wide`` -- the same with q, k and v scaled by 2^-12 .. 2^12 across positions (the
exponent runs through all 25 values inside every 32-position tile), so that a three-term split (without mid.mid, hi.lo, lo.hi) or any
coarser form would show: its error is 2^-16 of a product's largest term, the six-term form's 2^-23 in the worst case.

Bound: the error of the exact-fp32 kernels (v_mfma_f32_32x32x2_f32) this form replaced, measured on exactly these inputs against the same
float64 result, times 2 -- the six-term form adds a few 2^-24 roundings per product to an fp32 chain of comparable length.  The measured
errors (max |x - ref| / max |ref| per output) are the two tables below: PARENT_ERR, the fp32 kernels, which sets the bound, and
ERRORS_MEASURED, the split-bf16 kernels (a record; the test computes its own).  The largest ratio new / old is 1.16 (dQ, default, RT 400).

Two things the wide set found while this form was built, both fixed in csrc/dq_mfma.h: parts cut off by truncation left o and dQ at RT 33
at 4 - 5 x the fp32 error (the parts are now rounded to nearest); and dK/dV's recomputed scores must be the forward's bit for bit
(xty6<true>), or P = exp(S - lse) is off by e^(ulp of S): dV was wrong by 3e-2.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

OUTPUTS = ("o", "lse", "dq", "dk", "dv")
# max |x - float64| / max |float64| of the exact-fp32 product kernels on the inputs of _inputs(), one MI355X: (kind, RT) -> o, lse, dq, dk, dv
PARENT_ERR = {
    ("default", 31): (4.098e-07, 1.458e-07, 5.191e-07, 5.412e-07, 3.479e-07),
    ("default", 33): (3.264e-07, 9.635e-08, 3.852e-07, 5.403e-07, 4.655e-07),
    ("default", 400): (7.101e-07, 1.166e-07, 7.157e-07, 4.650e-07, 4.343e-07),
    ("default", 413): (1.031e-06, 1.066e-07, 9.579e-07, 5.863e-07, 8.681e-07),
    ("default", 2000): (1.282e-06, 1.389e-07, 1.228e-06, 1.215e-06, 9.025e-07),
    ("wide", 31): (5.892e-07, 1.317e-07, 9.038e-07, 5.253e-02, 7.808e-07),
    ("wide", 33): (1.384e-06, 1.586e-07, 1.820e-06, 2.198e-02, 6.827e-07),
    ("wide", 400): (5.622e-05, 1.555e-07, 5.958e-05, 1.269e-02, 2.590e-05),
    ("wide", 413): (1.666e-05, 1.307e-07, 1.534e-05, 1.115e-01, 1.044e-05),
    ("wide", 2000): (7.052e-04, 2.109e-07, 1.105e-04, 9.553e-03, 1.183e-04),
}
# the split-bf16 kernels on the same inputs and box (o, lse, dq, dk, dv).  In the wide set a score reaches 2^24, where one fp32 ulp of it is a
# factor of e in the softmax weight: dK there is dominated, in both forms alike, by the rounding of the scores themselves.
ERRORS_MEASURED = {
    ("default", 31): (1.673e-07, 1.208e-07, 2.163e-07, 3.697e-07, 1.616e-07),
    ("default", 33): (1.571e-07, 9.395e-08, 3.327e-07, 3.185e-07, 2.003e-07),
    ("default", 400): (5.749e-07, 1.037e-07, 8.310e-07, 2.940e-07, 3.563e-07),
    ("default", 413): (4.740e-07, 1.211e-07, 7.785e-07, 6.696e-07, 2.322e-07),
    ("default", 2000): (1.247e-06, 1.296e-07, 1.199e-06, 6.273e-07, 6.659e-07),
    ("wide", 31): (3.429e-07, 5.237e-08, 4.959e-07, 5.253e-02, 5.114e-07),
    ("wide", 33): (1.384e-06, 8.070e-08, 1.633e-06, 2.090e-02, 7.036e-07),
    ("wide", 400): (7.207e-06, 7.394e-08, 9.158e-06, 9.389e-03, 2.613e-05),
    ("wide", 413): (8.568e-06, 5.690e-08, 6.516e-06, 1.109e-01, 1.048e-05),
    ("wide", 2000): (1.258e-04, 5.457e-08, 3.179e-05, 7.395e-03, 3.447e-05),
}


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


def _inputs(kind, B, RT):
    gen = torch.Generator().manual_seed(1000 + RT)
    q, k, v, go = (torch.randn(B, 128, RT, generator=gen) for _ in range(4))
    if kind == "wide":
        p = torch.arange(RT)
        sc = lambda mul, add: torch.exp2((((p * mul + add) % 25) - 12).float())  # exact powers of two, all 25 inside every tile
        q, k, v = q * sc(7, 0), k * sc(11, 3), v * sc(13, 5)
    return q, k, v, go


def _ref64(q, k, v, go):
    """o, lse, dq, dk, dv of softmax(q k^T / sqrt(32)) v per head, in float64"""
    B, _, RT = q.shape
    q, k, v = (t.double().requires_grad_() for t in (q, k, v))
    h = lambda t: t.reshape(B, 4, 32, RT).transpose(2, 3)  # b (h c) n -> b h n c
    sim = torch.einsum("bhid,bhjd->bhij", h(q), h(k)) * 32 ** -0.5
    o = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), h(v)).transpose(2, 3).reshape(B, 128, RT)
    (o * go.double()).sum().backward()
    return {"o": o.detach(), "lse": torch.logsumexp(sim.detach(), dim=-1).reshape(-1), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def _run(N, q, k, v, go):
    L = N.lib()
    B, _, RT = q.shape
    qd, kd, vd, god = (t.contiguous().cuda() for t in (q, k, v, go))
    od = torch.full_like(qd, float("nan"))
    lse, delta = torch.empty(B * 4 * RT, device="cuda"), torch.empty(B * 4 * RT, device="cuda")
    N.check(L.dq_attn_fwd(N.ptr(qd), N.ptr(kd), N.ptr(vd), N.ptr(od), N.ptr(lse), B, RT, N.stream_ptr()), "dq_attn_fwd")
    dq, dk, dv = (torch.full_like(qd, float("nan")) for _ in range(3))
    N.check(L.dq_attn_bwd(N.ptr(qd), N.ptr(kd), N.ptr(vd), N.ptr(od), N.ptr(god), N.ptr(lse), N.ptr(delta), N.ptr(dq), N.ptr(dk), N.ptr(dv),
                          B, RT, N.stream_ptr()), "dq_attn_bwd")
    torch.cuda.synchronize()
    return {"o": od.cpu(), "lse": lse.cpu(), "dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu()}


@pytest.mark.parametrize("RT", [31, 33, 400, 413, 2000])
@pytest.mark.parametrize("kind", ["default", "wide"])
def test_attention_kernels_vs_float64(N, kind, RT):
    B = 1 if RT > 1000 else 2
    q, k, v, go = _inputs(kind, B, RT)
    ref = _ref64(q, k, v, go)
    got = _run(N, q, k, v, go)
    err = {n: float((got[n].double() - ref[n]).abs().max() / ref[n].abs().max()) for n in OUTPUTS}
    print(f"ATTN_SPLIT_ERR ('{kind}', {RT}): (" + ", ".join(f"{err[n]:.3e}" for n in OUTPUTS) + "),")
    for n, bound in zip(OUTPUTS, PARENT_ERR[(kind, RT)]):
        assert err[n] <= 2.0 * bound, (n, err[n], bound)


@pytest.mark.parametrize("RT", [31, 33, 400, 413, 2000])
def test_window_does_not_depend_on_its_batch(N, RT):
    """every window of a batch-32 call equals the single-window call, bit for bit"""
    q, k, v, go = _inputs("default", 32, RT)
    full = _run(N, q, k, v, go)
    for b in range(32):
        one = _run(N, q[b:b + 1], k[b:b + 1], v[b:b + 1], go[b:b + 1])
        for n in ("o", "dq", "dk", "dv"):
            assert torch.equal(one[n][0], full[n][b]), (b, n)
        assert torch.equal(one["lse"], full["lse"][b * 4 * RT:(b + 1) * 4 * RT]), (b, "lse")
