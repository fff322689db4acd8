"""CPU: the GEMM launcher's plan and its refusals (csrc/k_gemm.hip: choose(), part_scratch(), launch_gemm), without a device.

dq_debug_gemm_plan evaluates the launcher's own planning function, so the invariants below hold for what launch_gemm launches: a product
runs as `full` (whole rounds of 256 tiles, unsplit) plus `rest` (the remaining tiles, possibly with the reduction split), the two cover
the (cdiv(M, bm) x cdiv(N, 128)) tile grid exactly once, and the splits cut the reduction into non-empty ranges of whole k-tiles.
The refusals of launch_gemm are reached through dq_gemm_ex with made-up, 16-byte aligned addresses: each returns before the first HIP call.
"""
import ctypes

import pytest


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


def cdiv(a, b):
    return -(-a // b)


# around the multiples of the three tile heights (32, 64, 128), of the tile width (128) and of 128 k; K around the multiples of the k-tile (32)
MS = (1, 31, 32, 33, 64, 65, 128, 129, 257, 1025, 2048, 2176)
NS = (1, 127, 128, 129, 257, 1030, 2048, 4100, 33000)
KS = (1, 31, 32, 33, 64, 97, 1000, 4000)
SPLITS = (0, 1, 3, 64)
MAX_SPLIT_TILES = 1024  # tiles x splits of a chosen split: the bound the transformer's fixed scratch (1024 x 128 x 128 floats) relies on


def check_plan(N, M, Nn, K, batch, kbatch, splits):
    p = N.gemm_plan(M, Nn, K, batch, kbatch, splits)
    what = (M, Nn, K, batch, kbatch, splits, p)
    bm, full, rest = p["bm"], p["full"], p["rest"]
    kv = kbatch * cdiv(K, 32) * 32 if kbatch > 1 else K
    assert p["kv"] == kv, what
    assert bm in (32, 64, 128), what
    assert bm == 32 if M <= 32 else bm <= 64 if M <= 64 else True, what  # never a taller tile than the rows need
    tiles = cdiv(M, bm) * cdiv(Nn, 128)
    assert full["ntiles"] % 256 == 0 and full["ntiles"] >= 0 and rest["ntiles"] >= 0, what
    assert full["ntiles"] + rest["ntiles"] == tiles, what
    assert full["tile_base"] == 0, what
    if rest["ntiles"]:
        assert rest["tile_base"] == full["ntiles"], what
    assert full["splits"] == 1, what
    need = 0
    for part in (full, rest):
        if not part["ntiles"]:
            continue
        s, kps = part["splits"], part["k_per_split"]
        assert s >= 1 and kps > 0 and kps % 32 == 0, what
        assert (s - 1) * kps < kv <= s * kps, what  # no empty split, nothing left over
        if s > 1:
            need = max(need, s * batch * part["ntiles"] * bm * 128)
    if splits == 0 and batch == 1:
        assert rest["ntiles"] < 256 and rest["ntiles"] * rest["splits"] <= MAX_SPLIT_TILES, what
    if splits == 0 and batch > 1:
        assert full["ntiles"] == 0 and rest["splits"] == 1, what  # batched products run as one unsplit launch
    if splits > 0:
        assert full["ntiles"] == 0 and rest["splits"] <= min(splits, cdiv(kv, 32)), what  # one launch; capped at the k-tiles
        if splits == 1:
            assert rest["splits"] == 1, what
    # scratch: what the split parts need, and never more than the query promises
    assert p["scratch"] == need, what
    if splits == 0 and batch == 1:
        assert p["scratch"] <= N.lib().dq_gemm_scratch_floats(M, Nn, kv), what
        assert p["scratch"] <= MAX_SPLIT_TILES * 128 * 128, what
    if splits == 0 and batch > 1:
        assert p["scratch"] == 0, what
    if splits > 0:
        assert p["scratch"] <= min(splits, cdiv(kv, 32)) * batch * tiles * bm * 128, what
    return p


def test_plan_invariants(N):
    seen, n = set(), 0
    for M in MS:
        for Nn in NS:
            for K in KS:
                for batch, kbatch in ((1, 1), (3, 1), (1, 3), (3, 3)):
                    for splits in SPLITS:
                        p = check_plan(N, M, Nn, K, batch, kbatch, splits)
                        n += 1
                        seen.add((p["bm"], p["full"]["ntiles"] > 0, p["rest"]["ntiles"] > 0, p["rest"]["splits"] > 1))
    assert n == len(MS) * len(NS) * len(KS) * 4 * len(SPLITS)
    # the sweep reaches every tile height, both one- and two-launch plans, split and unsplit remainders, and a full launch with nothing left
    assert {s[0] for s in seen} == {32, 64, 128}
    for bm in (32, 64, 128):
        assert (bm, True, True, False) in seen and (bm, False, True, True) in seen, (bm, seen)
    assert any(s[1] and s[2] and s[3] for s in seen) and any(s[1] and not s[2] for s in seen), seen


def test_plan_of_the_shapes_the_gpu_tests_name(N):
    """The plans tests/test_gemm_paths.py asserts on the device, checked here too so that a change of the cost model shows without one."""
    g = N.gemm_plan
    assert (g(190, 8100, 36)["bm"], g(190, 8100, 36)["rest"]["ntiles"]) == (64, 192)
    assert (g(1500, 2100, 36)["bm"], g(1500, 2100, 36)["rest"]["ntiles"]) == (128, 204)
    p = g(33, 32800, 256)
    assert (p["bm"], p["full"]["ntiles"], p["rest"]) == (64, 256, {"tile_base": 256, "ntiles": 1, "splits": 8, "k_per_split": 32})
    p = g(40, 120, 33, kbatch=3, splits=2)
    assert (p["kv"], p["rest"]["splits"], p["rest"]["k_per_split"]) == (192, 2, 96)  # the boundary falls inside the second sample's block
    assert g(40, 120, 413, kbatch=3)["rest"]["splits"] == 39


def test_plan_hook_refuses_bad_arguments(N):
    lib = N.lib()
    buf = (ctypes.c_int32 * 10)()
    assert lib.dq_debug_gemm_plan(8, 8, 8, 1, 1, 0, buf, 10, None) == 10  # the scratch output is optional
    assert lib.dq_debug_gemm_plan(8, 8, 8, 1, 1, 0, buf, 9, None) == -1
    assert lib.dq_debug_gemm_plan(8, 8, 8, 1, 1, 0, None, 10, None) == -1
    for bad in ((0, 8, 8, 1, 1, 0), (8, 0, 8, 1, 1, 0), (8, 8, 0, 1, 1, 0), (8, 8, 8, 0, 1, 0), (8, 8, 8, 1, 0, 0), (8, 8, 8, 1, 1, -1)):
        assert lib.dq_debug_gemm_plan(*bad, buf, 10, None) == -1, bad


# ------------------------------------------------------------------------------------------------ launcher contracts
A0, B0, C0, D0, S0 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # made-up addresses: nothing below dereferences them


def refused(nat, word, **fields):
    d = dict(A=A0, B=B0, C=C0, M=40, N=40, K=40, lda=40, ldb=40, ldc=40)
    d.update(fields)
    rc = nat.gemm_ex(nat.gemm_desc(**d))
    msg = nat.lib().dq_last_error().decode()
    assert rc == 2 and word in msg, (rc, msg)


def test_launcher_refusals(N):
    refused(N, "not built", a_kmajor=0, b_kmajor=1)
    refused(N, "`add`", add=D0, accumulate=1)
    refused(N, "`add`", add=D0, splits=2, K=64, lda=64, ldb=64, scratch=S0, scratch_floats=1 << 40)
    refused(N, "leading dimensions", lda=42)
    refused(N, "leading dimensions", ldb=42)
    refused(N, "16-byte aligned", A=A0 + 4)
    refused(N, "16-byte aligned", B=B0 + 8)
    for stride in ("sAo", "sAi", "sBo", "sBi"):
        strides = dict(sAo=1600, sAi=800, sBo=1600, sBi=800, sCo=1600, sCi=800)
        strides[stride] += 2
        refused(N, "batch strides", batch=4, inner=2, **strides)
    refused(N, "k-batch", kbatch=2, sAk=1602, sBk=1600)
    refused(N, "k-batch", kbatch=2, sAk=1600, sBk=1601)
    refused(N, "k-batch", kbatch=0)
    refused(N, "reduction length", K=0)
    refused(N, "batch split", inner=0)
    refused(N, "missing operand", A=None)
    refused(N, "missing operand", C=None)
    # a split plan (140 x 128 x 1000 is split by the launcher's own choice) without scratch, or with one float too few
    need = N.gemm_plan(140, 128, 1000)["scratch"]
    assert need > 0 and N.gemm_plan(140, 128, 1000)["rest"]["splits"] > 1
    refused(N, "scratch", M=140, N=128, K=1000, lda=1000, ldb=1000, ldc=128)
    refused(N, "scratch", M=140, N=128, K=1000, lda=1000, ldb=1000, ldc=128, scratch=S0, scratch_floats=need - 1)
    refused(N, "scratch", splits=2, K=64, lda=64, ldb=64, scratch=S0, scratch_floats=2 * 2 * 32 * 128 - 1)
    refused(N, "exceeds the grid", batch=2000, splits=64, K=2048, lda=2048, ldb=2048, scratch=S0, scratch_floats=1 << 50)
    refused(N, "precision", precision=2)
    assert N.lib().dq_gemm_ex(None, None) == 2 and b"null descriptor" in N.lib().dq_last_error()


def test_nothing_to_do_returns_zero(N):
    for empty in (dict(M=0), dict(N=0), dict(batch=0), dict(M=-3), dict(batch=-1)):
        d = dict(A=A0, B=B0, C=C0, M=40, N=40, K=40, lda=40, ldb=40, ldc=40)
        d.update(empty)
        assert N.gemm_ex(N.gemm_desc(**d)) == 0, empty
