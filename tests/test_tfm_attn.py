"""The fused inference attention of the CustomTransformer's sampling path (csrc/k_tfm_attn.hip) against float64, through dq_tfm_attn_fwd.

Per (sample, head) o = softmax(q k^T / sqrt(dh)) v.  The reference is float64 on the CPU over the same fp32 inputs, written here.  The yardstick
is the three-launch path (form 0: scores GEMM, softmax rows, PV GEMM -- what dq_tfm_fwd runs) on the same inputs: the fused kernel's max-abs
error must be at most TWICE the three-launch path's on the same case, plus one fp32 ulp of the largest reference magnitude.  The arithmetic is
the same (fp32 products and sums, expf, one reciprocal); only the order of the sums differs, which the factor 2 covers; the ulp covers a case
on which the three-launch path happens to be exact.

Inputs: seeded normals, q scaled so that the scores have a standard deviation of about 3.  Every shape runs twice more with a constant added to
ONE key's scores for every query (the last feature of every head carries it: q = 3 there, k = c sqrt(dh) / 3 on that key and 0 elsewhere).
c = 60: the probability mass sits on that key (scores up to about 72; fp32 expf overflows only above 88.7, so this one checks the one-hot limit,
not the subtraction).  c = 100: scores of 90 - 110 on that key -- a softmax without the max subtraction gets inf / inf there, the correct
answer is finite.

Shapes (B, S1, S2, H, heads), Sk = S1 + S2: from one query and two keys up to the reference's layer, then both sides of the form
predicate's one bound, 4 (Sk (2 dh + 4) + 4 dh + 4 up4(Sk)) <= 160 KiB, at dh = 128 (Sk = 153 | 154) and at dh = 4 (Sk = 2558 | 2559).  Every case with Sk <= 68 must
report the fused form, so the kernel cannot be skipped silently.  Also: form -1 is the chosen form bit for bit, a second run repeats bit for
bit, nothing is written outside o.  Measured pairs: DESIGN.md section 29."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -2.5e33
CASES = [
    (1, 1, 1, 8, 2),       # one query, two keys, dh = 4
    (2, 5, 3, 32, 2),      # Sk = 8
    (3, 7, 6, 32, 1),      # Sk = 13: the up4 pitch of the three-launch path, a ragged key tail of the fused form
    (2, 17, 16, 64, 4),    # Sk = 33: one past a 32-tile
    (1, 33, 32, 64, 2),    # Sk = 65: one past a wave
    (2, 34, 34, 256, 2),   # the reference's rows at dh = 128
    (1, 34, 34, 1024, 8),  # the reference's layer exactly, one sample
    (1, 77, 76, 128, 1),   # Sk = 153 at dh = 128: the largest the fused form takes
    (1, 77, 77, 128, 1),   # Sk = 154: one past it -> three launches
    (1, 3, 2555, 8, 2),    # Sk = 2558 at dh = 4: the largest the fused form takes
    (1, 3, 2556, 8, 2),    # Sk = 2559: one past it
]
FUSED = {153: 1, 154: 0, 2558: 1, 2559: 0}  # the predicate at its bound


def _up4(v):
    return (v + 3) & ~3


def _inputs(B, S1, S2, H, heads, spike):
    """spike: the constant added to one key's scores (0: none)"""
    Sk, dh = S1 + S2, H // heads
    g = torch.Generator().manual_seed(1000 * Sk + H + heads + (7 if spike else 0) + (1 if spike > 60 else 0))
    q = 3.0 * torch.randn(B, S1, H, generator=g)
    kv = torch.randn(B, Sk, 2 * H, generator=g)
    if spike:
        j = Sk // 2
        for h in range(heads):
            c = h * dh + dh - 1
            q[:, :, c] = 3.0
            kv[:, :, c] = 0.0
            kv[:, j, c] = float(spike) * math.sqrt(dh) / 3.0
    return q, kv


def _reference(q, kv, heads):
    B, S1, H = q.shape
    Sk, dh = kv.shape[1], H // heads
    qd = q.double().reshape(B, S1, heads, dh).transpose(1, 2)
    kd = kv[..., :H].double().reshape(B, Sk, heads, dh).transpose(1, 2)
    vd = kv[..., H:].double().reshape(B, Sk, heads, dh).transpose(1, 2)
    p = torch.softmax(qd @ kd.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    return (p @ vd).transpose(1, 2).reshape(B, S1, H)


def _run(q, kv, heads, form):
    from dquartic import _native as N

    B, S1, H = q.shape
    Sk = kv.shape[1]
    band = 64
    buf = torch.full((band + q.numel() + band,), SENT, dtype=torch.float32, device=DEV)
    o = buf[band:band + q.numel()]
    prob = torch.empty(B * heads * S1 * _up4(Sk), dtype=torch.float32, device=DEV)
    rc = N.lib().dq_tfm_attn_fwd(N.ptr(q), N.ptr(kv), N.ptr(o), N.ptr(prob), B, S1, Sk, H, heads, form, N.stream_ptr())
    if rc:
        return rc, N.last_error()
    torch.cuda.synchronize()
    assert bool((buf[:band] == SENT).all()) and bool((buf[band + q.numel():] == SENT).all()), "written outside o"
    return 0, o.clone().view(B, S1, H)


@pytest.mark.parametrize("spike", [0, 60, 100], ids=["plain", "plus60", "plus100"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_attention_vs_float64(case, spike):
    from dquartic import _native as N

    B, S1, S2, H, heads = case
    Sk, dh = S1 + S2, H // heads
    chosen = N.lib().dq_tfm_attn_form(S1, Sk, dh)
    if Sk <= 68:
        assert chosen == 1, "every shape with Sk <= 68 (dh <= 128) takes the fused form"
    if Sk in FUSED:
        assert chosen == FUSED[Sk]
    q, kv = _inputs(B, S1, S2, H, heads, spike)
    ref = _reference(q, kv, heads)
    assert torch.isfinite(ref).all()
    qd, kvd = q.to(DEV), kv.to(DEV)
    rc, gemm = _run(qd, kvd, heads, 0)
    assert rc == 0, gemm
    rc, auto = _run(qd, kvd, heads, -1)
    assert rc == 0, auto
    err_gemm = float((gemm.cpu().double() - ref).abs().max())
    ulp = float(np.spacing(np.float32(ref.abs().max())))
    if chosen == 0:
        rc, msg = _run(qd, kvd, heads, 1)
        assert rc != 0 and "fused form does not take this shape" in msg  # refused with a message, never a silent fallback
        assert torch.equal(auto.view(torch.int32), gemm.view(torch.int32))  # form -1 == the chosen form, bit for bit
        print(f"attn {case} spike={spike}: form 0 only, err_gemm={err_gemm:.3e}")
        return
    rc, fused = _run(qd, kvd, heads, 1)
    assert rc == 0, fused
    rc, again = _run(qd, kvd, heads, 1)
    assert rc == 0, again
    err_fused = float((fused.cpu().double() - ref).abs().max())
    print(f"attn {case} spike={spike}: err_fused={err_fused:.3e} err_gemm={err_gemm:.3e} ulp={ulp:.3e}")
    assert torch.isfinite(fused).all()
    assert torch.equal(fused.view(torch.int32), again.view(torch.int32)), "a second run differs"
    assert torch.equal(auto.view(torch.int32), fused.view(torch.int32)), "form -1 is not the chosen form's result"
    assert err_fused <= 2.0 * err_gemm + ulp, (err_fused, err_gemm, ulp)
