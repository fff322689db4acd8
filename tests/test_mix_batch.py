"""``dq_mix_batch`` (k_mix.hip) on the GPU, bit for bit against ``dq_pair_batch`` where the two overlap and against
the numpy fp32 transcription of its rules (tests/test_mix_host.py) everywhere else.  The dataset is a slice of a larger allocation whose
neighbouring windows are NaN canaries, so a wrong index lands in allocated memory and shows as a NaN; every output sits between
sentinels, and ``run`` checks after every call that none of them moved."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from test_mix_host import mix_batch_ref
from test_stochastic_sampler import SEED, _dev_ids, _dev_seed

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, 12345.0  # floats around every output (a multiple of 4: the outputs stay 16-byte aligned)
OUTS = ("ms2_target", "ms1_target", "ms2_cond", "ms2_rest", "weights_out")
IDS = [7, 2 ** 33 + 1, 0, 2 ** 40, 3]


def same(got, want):
    """bit equality; a NaN equals a NaN (its sign and payload are the divider's business)"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def resident(a, canary=float("nan")):
    """a (n, ...) host array as a device tensor that is windows 1 .. n of an allocation of n + 2: the neighbours are `canary` (NaN shows
    in anything computed from it; the min / max reduction ignores a NaN, so the test of unused rows also runs with a large finite one)"""
    big = torch.full((a.shape[0] + 2,) + a.shape[1:], canary, device="cuda")
    big[1:-1] = torch.from_numpy(a).cuda()
    return big[1:-1]


def padded(*shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda")
    return buf, buf[PAD:PAD + n].view(*shape)


def untouched(buf):
    h = buf.cpu()
    return bool((h[:PAD] == SENTINEL).all() and (h[-PAD:] == SENTINEL).all())


def run(d2, d1, idx, count, K, weights=None, E=3, ids=None, draw=0, scale_target=1, with_rest=True, seed=SEED):
    """one call on the resident tensors d2 (n, RT, MZ) / d1 (n, ...); idx (K, B) and count (B) or None are host arrays -> dict of arrays"""
    from dquartic import _native as N

    n, RT, MZ = d2.shape
    B = idx.shape[1]
    bufs = {"ms2_target": padded(B, RT, MZ), "ms1_target": padded(B, *d1.shape[1:]), "ms2_cond": padded(B, RT, MZ),
            "ms2_rest": padded(B, RT, MZ), "weights_out": padded(B, K)}
    scratch = padded(N.lib().dq_mix_batch_scratch_bytes(B, K) // 4)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
    count_d = None if count is None else torch.tensor(list(count), dtype=torch.int32, device="cuda")
    ids_d, seed_d = None if ids is None else _dev_ids(list(ids)), _dev_seed(seed)
    fixed = None if weights is None else (ctypes.c_float * K)(*weights)
    p = {k: N.ptr(v[1]) for k, v in bufs.items()}
    N.check(N.lib().dq_mix_batch(N.ptr(d2), N.ptr(d1), n, N.ptr(idx_d), N.ptr(count_d), B, K, RT, MZ, d1[0].numel(), fixed, E, N.ptr(seed_d),
                                 N.ptr(ids_d), draw, scale_target, p["ms2_target"], p["ms1_target"], p["ms2_cond"],
                                 p["ms2_rest"] if with_rest else None, p["weights_out"], N.ptr(scratch[1]), scratch[1].numel() * 4,
                                 N.stream_ptr()), "dq_mix_batch")
    torch.cuda.synchronize()
    for k, (buf, _) in {**bufs, "scratch": scratch}.items():
        assert untouched(buf), k  # nothing outside an output is written
    if not with_rest:
        assert bool((bufs["ms2_rest"][0] == SENTINEL).all())  # a NULL ms2_rest: not written anywhere
    return {k: v[1].cpu().numpy() for k, v in bufs.items() if with_rest or k != "ms2_rest"}


def pool(n, RT, MZ, ms1_shape, seed=0):
    rng = np.random.default_rng(seed)
    ms2 = (rng.lognormal(0, 1, (n, RT, MZ)) * 50).astype(np.float32)
    ms1 = (rng.lognormal(0, 1, (n,) + ms1_shape) * 500).astype(np.float32)
    return ms2, ms1


# ---------------------------------------------------------------------------------------------------------------- (a)
# per/4 = 5 (empty chunks), 33 (one past a multiple of the chunks), 256 (exactly one block of k_mix per window), 6400 (25 blocks per
# window, the bench shape; MS1 of 400 spans two of them), 16896 (above 64 * 256: the capped grid walks a window in two strides)
@pytest.mark.parametrize("RT,MZ", [(5, 4), (3, 44), (16, 64), (400, 64), (264, 256)])
def test_two_fixed_components_are_the_pair_batch(RT, MZ):
    from dquartic import _native as N

    ms2, ms1 = pool(8, RT, MZ, (RT,))
    ms2[5], ms2[6] = 0.25, 0.25  # a constant pair: 0 / 0
    d2, d1 = resident(ms2), resident(ms1)
    i1, i2 = [0, 5, 2], [1, 6, 7]
    B = 3
    idx = torch.tensor(i1 + i2, dtype=torch.int64, device="cuda")
    new = lambda *s: torch.empty(s, device="cuda")
    a, b, c, m1, m2 = new(B, RT, MZ), new(B, RT, MZ), new(B, RT, MZ), new(B, RT), new(B, RT)
    sc = torch.empty(N.lib().dq_pair_batch_scratch_bytes(B) // 4, device="cuda")
    for w in ((0.5, 0.5), (0.7, 0.3)):
        N.check(N.lib().dq_pair_batch(N.ptr(d2), N.ptr(d1), 8, N.ptr(idx), B, RT, MZ, RT, w[0], w[1], N.ptr(a), N.ptr(m1), N.ptr(b), N.ptr(m2),
                                      N.ptr(c), N.ptr(sc), sc.numel() * 4, N.stream_ptr()), "dq_pair_batch")
        got = run(d2, d1, np.array([i1, i2]), None, 2, weights=w, scale_target=0)
        assert np.isnan(got["ms2_target"][1]).all() and np.isnan(got["ms2_cond"][1]).all() and not np.isnan(got["ms2_cond"][[0, 2]]).any()
        assert same(got["ms2_target"], a.cpu().numpy()) and same(got["ms1_target"], m1.cpu().numpy()) and same(got["ms2_cond"], c.cpu().numpy())
        assert same(got["ms2_rest"][[0, 2]], b.cpu().numpy()[[0, 2]] * np.float32(w[1]))  # the other window's product
        assert same(got["weights_out"], np.array([w] * B, dtype=np.float32))
        ref = mix_batch_ref(ms2, ms1, np.array([i1, i2]), None, 2, w, 0, None, None, 0, False)
        assert all(same(got[k], ref[k]) for k in OUTS)


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("ms1_shape", [(5,), (5, 3)], ids=["ms1_1d", "ms1_3ch"])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_drawn_weights_match_the_transcription(K, ms1_shape):
    RT, MZ, n, B = 5, 12, 10, 5  # per/4 = 15: chunks of one and two float4
    ms2, ms1 = pool(n, RT, MZ, ms1_shape, seed=K)
    d2, d1 = resident(ms2), resident(ms1)
    rng = np.random.default_rng(K)
    idx = np.stack([rng.permutation(n)[:K] for _ in range(B)], axis=1)
    count = [1, 2, K, max(1, K - 1), (K + 1) // 2]  # 1 .. K in one batch
    for E, ids, draw, scale, with_rest in itertools.product((0, 1, 4, 16), (IDS, None), (0, 5), (0, 1), (True, False)):
        got = run(d2, d1, idx, count, K, E=E, ids=ids, draw=draw, scale_target=scale, with_rest=with_rest)
        ref = mix_batch_ref(ms2, ms1, idx, count, K, None, E, SEED, ids, draw, scale)
        for k in got:
            assert same(got[k], ref[k]), (k, E, ids, draw, scale, with_rest)
        assert not np.isnan(got["ms2_cond"]).any()
    # NULL counts: K everywhere
    got, ref = run(d2, d1, idx, None, K, E=4, ids=IDS), mix_batch_ref(ms2, ms1, idx, None, K, None, 4, SEED, IDS, 0, True)
    assert all(same(got[k], ref[k]) for k in OUTS) and (got["weights_out"] > 0).all()
    # fixed weights under counts: w_j for the present components, 0 after, nothing renormalised
    fixed = [0.5 ** (j + 1) for j in range(K)]
    got, ref = run(d2, d1, idx, count, K, weights=fixed), mix_batch_ref(ms2, ms1, idx, count, K, fixed, 3, None, None, 0, True)
    assert all(same(got[k], ref[k]) for k in OUTS) and got["weights_out"][0].tolist() == [0.5] + [0.0] * (K - 1)


@pytest.mark.parametrize("RT,MZ,ms1_shape", [(400, 64, (400,)), (264, 256, (264, 3)), (65, 4, (65, 5))],
                         ids=["25_blocks", "two_strides_of_64_blocks", "ms1_longer_than_ms2"])
def test_more_than_one_block_per_window(RT, MZ, ms1_shape):
    """k_mix's grid is (min(ceil(max(RT MZ / 4, ms1_per) / 256), 64), B): blocks 1.. of a window, the stride between them, and -- above
    RT MZ = 65536 -- the second trip of a block through its window; the MS1 loop shares the grid (792 elements here span four blocks, and
    at (65, 4) the MS1 row of 325 is what sizes the grid: the second block has MS1 work only)"""
    K, B, n = 3, 3, 6
    ms2, ms1 = pool(n, RT, MZ, ms1_shape, seed=5)
    d2, d1 = resident(ms2), resident(ms1)
    idx = np.array([[0, 3, 5], [1, 4, 2], [2, 0, 4]])
    count = [3, 1, 2]
    for scale, with_rest in ((1, True), (0, False)):
        got = run(d2, d1, idx, count, K, E=4, ids=IDS[:B], draw=1, scale_target=scale, with_rest=with_rest)
        ref = mix_batch_ref(ms2, ms1, idx, count, K, None, 4, SEED, IDS[:B], 1, scale)
        for k in got:
            assert same(got[k], ref[k]), (k, scale)
        assert not np.isnan(got["ms2_cond"]).any() and not np.isnan(got["ms1_target"]).any()
    bad = idx.copy()
    bad[0, 1] = n  # the NaN fill of a refused window walks the same grid
    got = run(d2, d1, bad, count, K, E=4, ids=IDS[:B], draw=1)
    assert all(np.isnan(got[k][1]).all() and same(got[k][[0, 2]], ref_k[[0, 2]]) for k, ref_k in
               mix_batch_ref(ms2, ms1, idx, count, K, None, 4, SEED, IDS[:B], 1, 1).items())


# ---------------------------------------------------------------------------------------------------------------- (c)
def test_a_window_alone_is_the_window_in_its_batch():
    K, B = 3, 5
    ms2, ms1 = pool(9, 16, 64, (16,), seed=1)
    d2, d1 = resident(ms2), resident(ms1)
    rng = np.random.default_rng(1)
    idx = np.stack([rng.permutation(9)[:K] for _ in range(B)], axis=1)
    count = [3, 1, 2, 3, 2]
    batch = run(d2, d1, idx, count, K, E=4, ids=IDS, draw=2)
    ref = mix_batch_ref(ms2, ms1, idx, count, K, None, 4, SEED, IDS, 2, True)
    assert all(same(batch[k], ref[k]) for k in OUTS)  # (16, 64): one full block of the mix kernel per window, 32 float4 a chunk
    alone = run(d2, d1, idx[:, 3:4], count[3:4], K, E=4, ids=IDS[3:4], draw=2)
    assert all(same(alone[k][0], batch[k][3]) for k in OUTS)
    # under another id, or without ids (position 0), it draws other weights
    assert not np.array_equal(run(d2, d1, idx[:, 3:4], count[3:4], K, E=4, ids=[IDS[2]], draw=2)["weights_out"][0], batch["weights_out"][3])
    assert not np.array_equal(run(d2, d1, idx[:, 3:4], count[3:4], K, E=4, ids=None, draw=2)["weights_out"][0], batch["weights_out"][3])


# ---------------------------------------------------------------------------------------------------------------- (d)
def test_unused_rows_are_never_read_and_bad_indices_poison_their_window_only():
    K, B, n = 4, 5, 9
    ms2, ms1 = pool(n, 16, 64, (16, 3), seed=2)
    d2, d1 = resident(ms2), resident(ms1)
    rng = np.random.default_rng(2)
    idx = np.stack([rng.permutation(n)[:K] for _ in range(B)], axis=1)
    count = np.array([2, 1, 4, 3, 2])
    base = run(d2, d1, idx, count, K, E=4, ids=IDS)
    assert not any(np.isnan(v).any() for v in base.values())
    wild = idx.copy()
    for b in range(B):
        wild[count[b]:, b] = [n, -1, n, -1][:K - count[b]]  # n is the canary behind the dataset, -1 the one in front of it
    # NaN canaries show a read in the mix kernel; 1e30 ones also one in the min / max kernel, whose fminf / fmaxf drop a NaN
    for canary in (float("nan"), 1e30):
        got = run(resident(ms2, canary), resident(ms1, canary), wild, count, K, E=4, ids=IDS)
        assert all(np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)) for k in OUTS), canary
    # a USED index of n or -1 (the target's, or a later component's): that window is NaN in every output, the others keep their bits
    for b, j, bad in ((0, 0, n), (2, 3, -1), (3, 1, n), (4, 1, -(2 ** 40)), (1, 0, 2 ** 40)):
        poisoned = idx.copy()
        poisoned[j, b] = bad
        got = run(d2, d1, poisoned, count, K, E=4, ids=IDS)
        keep = [r for r in range(B) if r != b]
        for k in OUTS:
            assert np.isnan(got[k][b]).all(), (b, j, bad, k)
            assert np.array_equal(got[k][keep].view(np.uint32), base[k][keep].view(np.uint32)), (b, j, bad, k)
    # a count outside 1..K is refused the same way (nothing of the window is read)
    got = run(d2, d1, idx, [2, 0, 4, 5, 2], K, E=4, ids=IDS)
    for k in OUTS:
        assert np.isnan(got[k][[1, 3]]).all() and np.array_equal(got[k][[0, 2, 4]].view(np.uint32), base[k][[0, 2, 4]].view(np.uint32))
