"""dq_recon_metrics (csrc/k_metrics.hip) against a float64 numpy evaluation of the definitions in include/dq_hip.h on the same fp32 inputs.

Shapes: the smallest, odd ones, more than one block, and one at each edge of the kernels' own partition (constants below, named beside
the launch code they come from): a row segment of METRIC_ROW_SEG columns -1 / exact / +1, a scan chunk of METRIC_COL_ROWS rows, a column
tile of 64 lanes, a block of 4 waves of work items, and the finish kernel's 256-thread stride over scans and over columns.

Bound (derived, not measured): every sum is fp64 over fp32 inputs, so a result carries one fp32 rounding (2^-24 relative) plus fp64 noise
of at most n 2^-53 relative; |out - ref| <= 2 * 2^-24 * |ref| + 1e-9 for every metric, counts compared exactly.  Validity (a norm or a
variance being zero) is never a coin toss: the reference asserts that every norm / variance it meets is either that of an exactly
zero / exactly constant vector or far above fp64 noise (`positive`).  Outputs sit between canaries and start as NaN; the scratch has
exactly the documented size."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

METRIC_ROW_SEG = 4096   # dq_kernels.h: m/z columns of a scan one wave of k_metric_rows sums
METRIC_COL_ROWS = 64    # dq_kernels.h: scans of a column one lane of k_metric_cols sums
WAVE = 64               # k_metric_cols: lane = column, a tile is 64 columns
WAVES_PER_BLOCK = 4     # launch_recon_metrics: dim3(256), one work item per wave
FINISH_THREADS = 256    # k_metric_finish: a thread takes every 256th scan / column
ROW_MOMENTS, COL_MOMENTS, METRIC_COUNT = 10, 5, 9
U = 2.0 ** -24
HEAD, TAIL, CANARY = 64, 4096, 7251.0
CANARY_BITS = int(np.float32(CANARY).view(np.int32))

ISSUE_SHAPES = [(1, 1, 1), (3, 2, 5), (3, 17, 37), (2, 16, 64), (2, 65, 63), (1, 3, 4099)]
EDGE_SHAPES = (
    [(1, 2, METRIC_ROW_SEG + d) for d in (-1, 0, 1)]                 # one row segment -1 / exact / +1
    + [(1, METRIC_COL_ROWS + d, 3) for d in (-1, 0, 1)]              # one scan chunk
    + [(1, 3, WAVE + d) for d in (-1, 0, 1)]                         # one column tile
    + [(1, WAVES_PER_BLOCK + d, 5) for d in (-1, 0, 1)]              # one block of row work items
    + [(1, FINISH_THREADS + d, 2) for d in (-1, 0, 1)]               # the finish kernel's stride over scans
    + [(1, 2, FINISH_THREADS + d) for d in (-1, 0, 1)]               # ... and over columns
)
CONTENTS = ["random", "equal", "zero_scans", "const_cols", "zero_window", "mixed_sign"]
CONTENT_SHAPES = [(3, 17, 37), (2, 65, 63), (1, 3, 4099)]


def cdiv(a, b):
    return -(-a // b)


def documented_scratch_bytes(B, RT, MZ):
    """include/dq_hip.h: 8 * B * (10 * RT * ceil(MZ / 4096) + 5 * MZ * ceil(RT / 64))"""
    return 8 * B * (ROW_MOMENTS * RT * cdiv(MZ, METRIC_ROW_SEG) + COL_MOMENTS * MZ * cdiv(RT, METRIC_COL_ROWS))


def make_case(content, B, RT, MZ, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * B + 31 * RT + 101 * MZ + CONTENTS.index(content))
    P = rng.random((B, RT, MZ), dtype=np.float32)
    T = rng.random((B, RT, MZ), dtype=np.float32)
    if content == "equal":
        P = T.copy()
    elif content == "zero_scans":  # an all-zero target scan, an all-zero pred scan, and (window 0) a scan that is zero in both
        T[:, 0, :] = 0
        P[:, RT - 1, :] = 0
        P[0, RT // 2, :] = 0
        T[0, RT // 2, :] = 0
    elif content == "const_cols":  # a constant target column, a constant pred column, and (window 0) a column constant in both
        T[:, :, 0] = np.float32(0.3)
        P[:, :, MZ - 1] = np.float32(0.7)
        P[0, :, MZ // 2] = np.float32(0.1)
        T[0, :, MZ // 2] = np.float32(0.9)
    elif content == "zero_window":  # window 0 zero in both; the last window (B > 1) zero in the target only
        P[0] = 0
        T[0] = 0
        if B > 1:
            T[B - 1] = 0
    elif content == "mixed_sign":
        P, T = 2 * P - 1, 2 * T - 1
    return np.ascontiguousarray(P, np.float32), np.ascontiguousarray(T, np.float32)


def positive(x, centred):
    """Is the squared norm (centred: the variance) of the float64 vector x positive?  Exactly zero / constant: no.  Otherwise it must lie
    far above fp64 noise (asserted), so that no rounding of a sum decides validity."""
    x = x.reshape(-1)
    if np.all(x == (x[0] if centred else 0.0)):
        return False
    c = x - x.mean() if centred else x
    # (fp64 noise of a sum of x.size squares is at most x.size * 2^-53 of the sum of squares; the inputs stay a factor of 64 above that)
    assert (c * c).sum() > 64 * x.size * 2.0 ** -53 * max((x * x).sum(), 1e-30), "test input within fp64 noise of a validity threshold"
    return True


def cosine64(p, t):
    if not (positive(p, False) and positive(t, False)):
        return 0.0
    return float((p * t).sum() / math.sqrt((p * p).sum() * (t * t).sum()))


def sa64(c):
    return 1.0 - 2.0 * math.acos(min(1.0, max(-1.0, c))) / math.pi


def pearson64(p, t):
    if not (positive(p, True) and positive(t, True)):
        return 0.0
    pc, tc = p - p.mean(), t - t.mean()
    return float((pc * tc).sum() / math.sqrt((pc * pc).sum() * (tc * tc).sum()))


def reference(P, T):
    """(B, 9) float64 from the definitions, on the promoted fp32 inputs"""
    out = np.zeros((P.shape[0], METRIC_COUNT))
    for b in range(P.shape[0]):
        p, t = P[b].astype(np.float64), T[b].astype(np.float64)
        RT, MZ = p.shape
        d = p - t
        c = cosine64(p.reshape(-1), t.reshape(-1))
        scans = [sa64(cosine64(p[r], t[r])) for r in range(RT) if positive(t[r], False)]
        xics = [pearson64(p[:, k], t[:, k]) for k in range(MZ) if positive(t[:, k], True)]
        out[b] = [(d * d).sum() / d.size, np.abs(d).sum() / d.size, c, sa64(c), pearson64(p.reshape(-1), t.reshape(-1)),
                  np.mean(scans) if scans else 0.0, len(scans), np.mean(xics) if xics else 0.0, len(xics)]
    return out


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


class Pad:
    """n floats between canaries (compared bitwise through an int view), NaN to begin with"""

    def __init__(self, n):
        self.buf = torch.full((HEAD + n + TAIL,), CANARY, device="cuda")
        self.n = n
        self.view = self.buf[HEAD:HEAD + n]
        self.view.fill_(float("nan"))

    def intact(self):
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        return bool((bits[:HEAD] == CANARY_BITS).all()) and bool((bits[HEAD + self.n:] == CANARY_BITS).all())


def run(N, P, T):
    B, RT, MZ = P.shape
    nbytes = documented_scratch_bytes(B, RT, MZ)
    assert N.lib().dq_recon_metrics_scratch_bytes(B, RT, MZ) == nbytes
    p, t = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
    out, scratch = Pad(B * METRIC_COUNT), Pad(nbytes // 4)
    assert scratch.view.data_ptr() % 8 == 0
    N.check(N.lib().dq_recon_metrics(N.ptr(p), N.ptr(t), N.ptr(out.view), N.ptr(scratch.view), nbytes, B, RT, MZ, N.stream_ptr()),
            "dq_recon_metrics")
    assert out.intact() and scratch.intact()
    return out.view.cpu().numpy().reshape(B, METRIC_COUNT).copy()


def check(N, P, T):
    got, ref = run(N, P, T), reference(P, T)
    names = N.METRIC_NAMES
    assert len(names) == METRIC_COUNT
    for i, name in enumerate(names):
        g, r = got[:, i].astype(np.float64), ref[:, i]
        print(f"{name}: max |out - ref| = {np.abs(g - r).max():.3e} (ref max {np.abs(r).max():.6g})")
        if name.endswith("_count"):
            assert np.array_equal(g, r), (name, g, r)
        else:
            assert np.all(np.abs(g - r) <= 2 * U * np.abs(r) + 1e-9), (name, g, r)
    return got, ref


@pytest.mark.parametrize("B,RT,MZ", ISSUE_SHAPES + EDGE_SHAPES)
def test_shapes(N, B, RT, MZ):
    check(N, *make_case("random", B, RT, MZ))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("B,RT,MZ", CONTENT_SHAPES)
def test_contents(N, B, RT, MZ, content):
    P, T = make_case(content, B, RT, MZ)
    got, ref = check(N, P, T)
    col = {n: i for i, n in enumerate(N.METRIC_NAMES)}
    if content == "equal":  # cosine, sa and pearson are 1 within the bound; nothing differs
        for name in ("cosine", "sa", "pearson", "scan_sa", "xic_r"):
            assert np.all(np.abs(got[:, col[name]] - 1.0) <= 2 * U + 1e-9), name
        assert np.all(got[:, col["mse"]] == 0) and np.all(got[:, col["mae"]] == 0)
    if content == "zero_scans":  # the all-zero target scans are not counted (window 0 has two)
        assert got[0, col["scan_count"]] == RT - (2 if RT // 2 != 0 else 1) and np.all(got[1:, col["scan_count"]] == RT - 1)
    if content == "const_cols":
        assert got[0, col["xic_count"]] == MZ - (2 if MZ // 2 != 0 else 1) and np.all(got[1:, col["xic_count"]] == MZ - 1)
    if content == "zero_window":
        assert np.all(got[0] == 0)
        if B > 1:
            assert got[B - 1, col["scan_count"]] == 0 and got[B - 1, col["cosine"]] == 0 and got[B - 1, col["mse"]] > 0


def test_a_window_does_not_depend_on_its_batch(N):
    P, T = make_case("random", 5, 17, 37)
    P[3, 4, :] = 0
    T[2, :, 5] = np.float32(0.5)
    batched = run(N, P, T)
    for j in range(5):
        alone = run(N, P[j:j + 1].copy(), T[j:j + 1].copy())
        assert np.array_equal(alone[0].view(np.int32), batched[j].view(np.int32)), j


def test_rejections(N):
    p = torch.zeros(2, 3, 5, device="cuda")
    out = torch.full((2 * METRIC_COUNT,), float("nan"), device="cuda")
    scratch = torch.empty(documented_scratch_bytes(2, 3, 5) // 8, dtype=torch.float64, device="cuda")
    L = N.lib()
    assert L.dq_recon_metrics(N.ptr(p), N.ptr(p), N.ptr(out), N.ptr(scratch), scratch.numel() * 8 - 8, 2, 3, 5, N.stream_ptr()) != 0
    assert b"scratch too small" in L.dq_last_error()
    assert L.dq_recon_metrics(N.ptr(p), N.ptr(p), N.ptr(out), N.ptr(scratch), scratch.numel() * 8, 2, 0, 5, N.stream_ptr()) != 0
    assert L.dq_recon_metrics(N.ptr(p), None, N.ptr(out), N.ptr(scratch), scratch.numel() * 8, 2, 3, 5, N.stream_ptr()) != 0
    assert L.dq_recon_metrics_scratch_bytes(0, 3, 5) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
