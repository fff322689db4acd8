"""The three streaming kernels of the transformer's held-out evaluation alone (csrc/k_stream.hip, csrc/k_tfm.hip; DESIGN.md sections 31 and 36), at their loop edges.

dq_q_sample_repeats and dq_mse_per_window_repeats work on R repeats of B windows stacked repeat-major.  What is asserted is bitwise, against
the kernels that exist without them: the head equals dq_q_sample on x0 replicated R times; the tail equals dq_mse_per_window applied per
repeat (per_window and loss); noise == NULL / target == NULL (drawn in the kernel at draw index first_draw + r) equals the same call on
dq_randn's tensors stacked.  For the x0 objective loss_out[r] is also recomputed in float64 from per_window and the weight table: per_window
carries one fp32 rounding of each window's MSE and loss_out one of the sum, the weights are positive, so |loss - ref| <= 2 * 2^-24 |ref| (+ 1e-9
for fp64 noise; the bound of tests/test_eval_step.py).

Sizes: per on both sides of a slice of 8192 elements (8188, 8192, 8196), one float4 (4), three slices (16388); (R, B) in (1,1), (1,3), (3,1),
(3,2); window ids that are not 0 .. B-1; t including 0 and T-1; both objectives; auto_normalize on and off; and one case of 3 * 3 * 262148
elements, more than the 2048 * 256 lanes * 4 of one sweep of the grid-stride loop.  dq_tfm_kv_broadcast: on a sentinel-filled buffer, S2 * 2H at the
smallest size the handle admits (H = 8, S2 = 1: four float4), R = 1 (nothing written), and one copy longer than one sweep of its grid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 1000
U = 2.0 ** -24
HEAD, TAIL, CANARY = 64, 1024, 7251.0
CANARY_BITS = int(np.float32(CANARY).view(np.int32))
FIRST_DRAW = 3


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


class Pad:
    """an output between two canary zones, itself NaN before the call"""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((HEAD + n + TAIL,), CANARY, device="cuda")
        self.n = n
        self.view = self.buf[HEAD:HEAD + n]
        self.view.fill_(float("nan"))
        self.shape = shape

    def get(self):
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        assert bool((bits[:HEAD] == CANARY_BITS).all()) and bool((bits[HEAD + self.n:] == CANARY_BITS).all()), "wrote outside its output"
        return self.view.reshape(self.shape).clone()


def bits(v):
    return v.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def tables():
    betas = torch.linspace(1e-4, 0.02, T, dtype=torch.float64)
    ab = torch.cumprod(1 - betas, 0).float()
    lw = (ab / (1 - ab)).float()
    return ab.cuda(), lw.cuda()


def make_case(R, B, per, norm):
    g = torch.Generator().manual_seed(1000 * R + 100 * B + per + norm)
    x0 = torch.rand(B, per, generator=g)
    out = torch.randn(R, B, per, generator=g)
    t = torch.randint(0, T, (R, B), generator=g)
    if R * B > 1:
        t.view(-1)[0], t.view(-1)[-1] = 0, T - 1
    else:
        t.view(-1)[0] = 0 if norm else T - 1
    ids = torch.tensor([41, 7, 1 << 33][:B], dtype=torch.int64)  # neither 0 .. B-1 nor ordered; one beyond 32 bits
    seed = torch.tensor([0x5DEECE66D + per], dtype=torch.int64)
    return x0.cuda(), out.cuda(), t.cuda(), ids.cuda(), seed.cuda()


def randn_stack(N, seed, ids, R, B, per):
    z = torch.empty(R, B, per, device="cuda")
    for r in range(R):
        N.check(N.lib().dq_randn(N.ptr(z[r]), N.ptr(ids), N.ptr(seed), FIRST_DRAW + r, B, per, N.stream_ptr()), "dq_randn")
    return z


def head(N, ab, x0, t, noise, seed, ids, R, B, per, norm):
    x_t = Pad(R, B, per)
    N.check(N.lib().dq_q_sample_repeats(N.ptr(ab), N.ptr(x0), N.ptr(t), N.ptr(noise), N.ptr(seed), N.ptr(ids), FIRST_DRAW, N.ptr(x_t.view), B, R, per,
                                        norm, N.stream_ptr()), "dq_q_sample_repeats")
    return x_t.get()


def tail(N, out, target, Bt, tm, ta, seed, ids, lw, t, R, B, per):
    nbytes = N.lib().dq_mse_per_window_scratch_bytes(R * B, per)
    pw, loss, scratch = Pad(R, B), Pad(R), Pad(nbytes // 4)
    N.check(N.lib().dq_mse_per_window_repeats(N.ptr(out), N.ptr(target), Bt, tm, ta, N.ptr(seed), N.ptr(ids), FIRST_DRAW, N.ptr(lw), N.ptr(t),
                                              N.ptr(pw.view), N.ptr(loss.view), N.ptr(scratch.view), B, R, per, N.stream_ptr()),
            "dq_mse_per_window_repeats")
    scratch.get()
    return pw.get(), loss.get()


def tail_per_repeat(N, out, target_of, tm, ta, lw, t, R, B, per):
    """dq_mse_per_window, the kernel that exists without this feature, once per repeat"""
    pw, loss = torch.empty(R, B, device="cuda"), torch.empty(R, device="cuda")
    scratch = torch.empty(N.lib().dq_mse_per_window_scratch_bytes(B, per), dtype=torch.uint8, device="cuda")
    for r in range(R):
        N.check(N.lib().dq_mse_per_window(N.ptr(out[r]), N.ptr(target_of(r)), tm, ta, N.ptr(lw), N.ptr(t[r]), N.ptr(pw[r]), N.ptr(loss[r:r + 1]),
                                          N.ptr(scratch), B, per, N.stream_ptr()), "dq_mse_per_window")
    torch.cuda.synchronize()
    return pw, loss


def check_head_and_tail(N, tables, R, B, per, norm):
    ab, lw = tables
    x0, out, t, ids, seed = make_case(R, B, per, norm)
    z = randn_stack(N, seed, ids, R, B, per)
    # ---- the head: dq_q_sample on the inputs replicated R times
    ref_xt = torch.empty(R * B, per, device="cuda")
    N.check(N.lib().dq_q_sample(N.ptr(ab), N.ptr(x0.repeat(R, 1).contiguous()), N.ptr(t.reshape(-1)), N.ptr(z.reshape(R * B, per)), N.ptr(ref_xt),
                                R * B, per, norm, N.stream_ptr()), "dq_q_sample")
    read = head(N, ab, x0, t, z, None, None, R, B, per, norm)
    drawn = head(N, ab, x0, t, None, seed, ids, R, B, per, norm)
    assert torch.isfinite(ref_xt).all()
    assert torch.equal(bits(read).reshape(-1), bits(ref_xt).reshape(-1))
    assert torch.equal(bits(drawn), bits(read))
    # ---- the tail, eps objective: the noise as target, read (R * B windows) or drawn
    ref_pw, ref_loss = tail_per_repeat(N, out, lambda r: z[r], 1.0, 0.0, None, t, R, B, per)
    for target, Bt in ((z, R * B), (None, 0)):
        pw, loss = tail(N, out, target, Bt, 1.0, 0.0, seed, ids, None, t, R, B, per)
        assert torch.equal(bits(pw), bits(ref_pw)) and torch.equal(bits(loss), bits(ref_loss)), (Bt, pw, ref_pw)
    # ---- x0 objective: the shared x0 (B windows) as target, weighted by lw[t]
    tm, ta = (2.0, -1.0) if norm else (1.0, 0.0)
    ref_pw, ref_loss = tail_per_repeat(N, out, lambda r: x0, tm, ta, lw, t, R, B, per)
    pw, loss = tail(N, out, x0, B, tm, ta, None, None, lw, t, R, B, per)
    assert torch.equal(bits(pw), bits(ref_pw)) and torch.equal(bits(loss), bits(ref_loss))
    ref64 = (lw.double()[t] * pw.double()).mean(dim=1).cpu().numpy()
    got = loss.double().cpu().numpy()
    print(f"R={R} B={B} per={per} norm={norm}: max |loss - ref| / bound = {(np.abs(got - ref64) / (2 * U * np.abs(ref64) + 1e-9)).max():.3f}")
    assert np.all(np.abs(got - ref64) <= 2 * U * np.abs(ref64) + 1e-9), (got, ref64)
    tp = x0 * tm + ta  # fp32: one multiply, one add
    mse64 = ((out.double() - tp.double()[None]) ** 2).mean(dim=2).cpu().numpy()
    assert np.all(np.abs(pw.double().cpu().numpy() - mse64) <= 2 * U * np.abs(mse64) + 1e-9)


@pytest.mark.parametrize("norm", [1, 0], ids=["norm", "raw"])
@pytest.mark.parametrize("R,B", [(1, 1), (1, 3), (3, 1), (3, 2)])
@pytest.mark.parametrize("per", [4, 8188, 8192, 8196, 16388])
def test_head_and_tail_bitwise(N, tables, per, R, B, norm):
    check_head_and_tail(N, tables, R, B, per, norm)


def test_head_and_tail_wrap_the_grid_stride_loop(N, tables):
    R, B, per = 3, 3, 262148
    assert R * B * per > 2048 * 256 * 4
    check_head_and_tail(N, tables, R, B, per, 1)


def test_draws_follow_the_window_id_and_the_repeat(N, tables):
    ab, _ = tables
    R, B, per = 3, 2, 8196
    x0, out, t, ids, seed = make_case(R, B, per, 1)
    a = head(N, ab, x0, t, None, seed, ids, R, B, per, 1)
    default_ids = head(N, ab, x0, t, None, seed, None, R, B, per, 1)
    explicit = head(N, ab, x0, t, None, seed, torch.arange(B, device="cuda"), R, B, per, 1)
    assert torch.equal(bits(default_ids), bits(explicit)) and not torch.equal(a, default_ids)
    t_same = t[:1].repeat(R, 1).contiguous()  # the same timestep in every repeat: only the draw index tells them apart
    b = head(N, ab, x0, t_same, None, seed, ids, R, B, per, 1)
    assert not torch.equal(b[0], b[1]) and not torch.equal(b[1], b[2])


BROADCAST = [(2, 3, 1, 1, 8), (3, 2, 5, 7, 8), (1, 4, 3, 2, 16), (2, 1, 3, 4, 8), (8, 5, 34, 2, 1024)]


@pytest.mark.parametrize("B,R,S2,S1,H", BROADCAST)
def test_kv_broadcast(N, B, R, S2, S1, H):
    Sk, n = S1 + S2, R * B
    if (B, R) == (8, 5):
        assert (R - 1) * B * S2 * 2 * H // 4 > 2048 * 256  # more float4 than one sweep of the grid
    pad = Pad(n, Sk, 2 * H)
    g = torch.Generator().manual_seed(B + 10 * R)
    before = torch.randn(n, Sk, 2 * H, generator=g).cuda()
    before[B:, :S2] = CANARY  # the sentinel where the copy must land
    pad.view.copy_(before.reshape(-1))
    N.check(N.lib().dq_tfm_kv_broadcast(N.ptr(pad.view), B, R, S2, Sk, H, N.stream_ptr()), "dq_tfm_kv_broadcast")
    after = pad.get()
    assert torch.equal(bits(after[:, S2:]), bits(before[:, S2:]))  # the forward's own rows of every sample
    assert torch.equal(bits(after[:B]), bits(before[:B]))  # the source samples
    for r in range(1, R):
        assert torch.equal(bits(after[r * B:(r + 1) * B, :S2]), bits(before[:B, :S2])), r
    if R == 1:
        assert torch.equal(bits(after), bits(before))
