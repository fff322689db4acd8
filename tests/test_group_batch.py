"""``dq_mix_group_batch`` (k_mix.hip) on the GPU: every output bit for bit against the numpy fp32 transcription of
its rules (tests/group_eval_ref.py), and the three exact anchors against ``dq_mix_batch`` run on the GPU.  As in tests/test_mix_batch.py
the dataset is a slice of a larger allocation whose neighbouring windows are NaN canaries, every output sits between sentinels, and
``run_group`` checks after every call that none of them moved.  Inputs are lognormal (hi > lo everywhere) except where NaN is the point."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from group_eval_ref import GROUP_OUTS, mix_group_batch_ref
from test_mix_batch import IDS, padded, pool, resident, run, same, untouched, SENTINEL
from test_stochastic_sampler import SEED, _dev_ids, _dev_seed

pytestmark = pytest.mark.gpu


def run_group(d2, d1, idx, count, K, P, weights=None, E=3, ids=None, draw=0, scale_target=1, with_rest=True, seed=SEED):
    """one call on the resident tensors d2 (n, RT, MZ) / d1 (n, ...); idx (K, G) and count (G) or None are host arrays -> dict of arrays"""
    from dquartic import _native as N

    n, RT, MZ = d2.shape
    G = idx.shape[1]
    bufs = {"ms2_target": padded(P * G, RT, MZ), "ms1_target": padded(P * G, *d1.shape[1:]), "ms2_cond": padded(P * G, RT, MZ),
            "ms2_rest": padded(G, RT, MZ), "weights_out": padded(G, K)}
    nbytes = N.lib().dq_mix_group_batch_scratch_bytes(G, K, P)
    assert nbytes == 8 * G * (8 + P)
    scratch = padded(nbytes // 4)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
    count_d = None if count is None else torch.tensor(list(count), dtype=torch.int32, device="cuda")
    ids_d, seed_d = None if ids is None else _dev_ids(list(ids)), _dev_seed(seed)
    fixed = None if weights is None else (ctypes.c_float * K)(*weights)
    p = {k: N.ptr(v[1]) for k, v in bufs.items()}
    N.check(N.lib().dq_mix_group_batch(N.ptr(d2), N.ptr(d1), n, N.ptr(idx_d), N.ptr(count_d), G, K, P, RT, MZ, d1[0].numel(), fixed, E,
                                       N.ptr(seed_d), N.ptr(ids_d), draw, scale_target, p["ms2_target"], p["ms1_target"], p["ms2_cond"],
                                       p["ms2_rest"] if with_rest else None, p["weights_out"], N.ptr(scratch[1]), nbytes, N.stream_ptr()),
            "dq_mix_group_batch")
    torch.cuda.synchronize()
    for k, (buf, _) in {**bufs, "scratch": scratch}.items():
        assert untouched(buf), k  # nothing outside an output is written
    if not with_rest:
        assert bool((bufs["ms2_rest"][0] == SENTINEL).all())  # a NULL ms2_rest: not written anywhere
    return {k: v[1].cpu().numpy() for k, v in bufs.items() if with_rest or k != "ms2_rest"}


def groups(n, K, P, G, seed):
    """indices (K, G) of distinct windows and counts mixed over [P, K] (K first, then P, then what lies between)"""
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(n)[:K] for _ in range(G)], axis=1)
    count = [(K, P, (P + K) // 2)[g % 3] for g in range(G)]
    return idx, count


# per = 4: one float4, seven of the eight chunks empty; per = 36: nine float4 over eight chunks (uneven); per = 4 * (64 * 256 + 3): above
# the 64 blocks x 256 lanes of the mix kernel's capped grid, three float4 into the second trip of the strided walk.
# ms1_per 1, 5, 300: a single value (lo == hi would be 0 / 0: the one case is covered where NaN is the point), a few, and -- against per / 4 = 1
# or 9 -- an MS1 row longer than the window's float4 count, which then sizes the grid (two blocks at 300).
SHAPES = [(1, 4, (5,)), (1, 4, (300,)), (3, 12, (5,)), (3, 12, (100, 3)), (64 * 256 + 3, 4, (5,))]


@pytest.mark.parametrize("RT,MZ,ms1_shape", SHAPES, ids=["per4", "per4_ms1_300", "per36", "per36_ms1_300", "strided_walk"])
def test_every_output_matches_the_transcription_at_the_window_sizes(RT, MZ, ms1_shape):
    K, P, G, n = 4, 2, 3, 6
    ms2, ms1 = pool(n, RT, MZ, ms1_shape, seed=RT)
    d2, d1 = resident(ms2), resident(ms1)
    idx, count = groups(n, K, P, G, RT)
    for scale, with_rest, ids in ((1, True, IDS[:G]), (0, False, None)):
        got = run_group(d2, d1, idx, count, K, P, E=4, ids=ids, draw=1, scale_target=scale, with_rest=with_rest)
        ref = mix_group_batch_ref(ms2, ms1, idx, count, K, P, None, 4, SEED, ids, 1, scale)
        for k in got:
            assert same(got[k], ref[k]), (k, scale)
        assert not any(np.isnan(v).any() for v in got.values())


def test_a_single_value_ms1_row():
    """ms1_per = 1: lo == hi, so the member's MS1 is 0 / 0 -- NaN in the transcription and in the kernel, and nowhere else"""
    K, P, G, n = 2, 2, 1, 4
    ms2, ms1 = pool(n, 3, 12, (1,), seed=3)
    got = run_group(resident(ms2), resident(ms1), np.array([[0], [2]]), None, K, P, E=2)
    ref = mix_group_batch_ref(ms2, ms1, np.array([[0], [2]]), None, K, P, None, 2, SEED, None, 0, 1)
    assert all(same(got[k], ref[k]) for k in GROUP_OUTS) and np.isnan(got["ms1_target"]).all() and not np.isnan(got["ms2_cond"]).any()


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("P,K", [(P, K) for P in (1, 2, 3, 8) for K in (2, 4, 8) if P <= K])
def test_members_and_components(P, K, G):
    """P in {1, 2, 3, 8} x K in {2, 4, 8} (P <= K is the call's rule; its refusal: tests/test_group_eval_host.py) x G, with the counts mixed
    over [P, K]; drawn and fixed weights, both scale_target values, ms2_rest null and given, ids null and given.  Per member: the anchors
    against dq_mix_batch on the GPU."""
    RT, MZ, n = 5, 12, 10  # per / 4 = 15: chunks of one and two float4
    ms2, ms1 = pool(n, RT, MZ, (7,), seed=10 * K + P)
    d2, d1 = resident(ms2), resident(ms1)
    idx, count = groups(n, K, P, G, 10 * K + P)
    fixed = [0.5 ** (j + 1) for j in range(K)]
    for weights, ids, scale, with_rest in itertools.product((None, fixed), (IDS[:G], None), (0, 1), (True, False)):
        got = run_group(d2, d1, idx, count, K, P, weights=weights, E=4, ids=ids, draw=2, scale_target=scale, with_rest=with_rest)
        ref = mix_group_batch_ref(ms2, ms1, idx, count, K, P, weights, 4, SEED, ids, 2, scale)
        for k in got:
            assert same(got[k], ref[k]), (k, weights is None, ids is None, scale, with_rest)
        assert not any(np.isnan(v).any() for v in got.values())
        # anchor 1: the mixture in every slice, the weights, member 0's target and MS1 are dq_mix_batch's on the same arguments
        one = run(d2, d1, idx, count, K, weights=weights, E=4, ids=ids, draw=2, scale_target=scale)
        assert same(got["weights_out"], one["weights_out"]) and same(got["ms2_target"][:G], one["ms2_target"])
        assert same(got["ms1_target"][:G], one["ms1_target"])
        for p in range(P):
            assert same(got["ms2_cond"][p * G:(p + 1) * G], one["ms2_cond"]), p
        # anchor 2, fixed weights: member p is dq_mix_batch's target with rows 0 and p of idx and weights 0 and p swapped
        if weights is not None:
            for p in range(1, P):
                sw_idx, sw_w = idx.copy(), list(weights)
                sw_idx[[0, p]] = sw_idx[[p, 0]]
                sw_w[0], sw_w[p] = sw_w[p], sw_w[0]
                other = run(d2, d1, sw_idx, count, K, weights=sw_w, E=4, ids=ids, draw=2, scale_target=scale)
                assert same(got["ms2_target"][p * G:(p + 1) * G], other["ms2_target"]), p
                assert same(got["ms1_target"][p * G:(p + 1) * G], other["ms1_target"]), p
        # anchor 3, scale_target and count == P: the members' targets added in order are the mixture
        if scale:
            for g in range(G):
                if count[g] == P:
                    total = got["ms2_target"][g].copy()
                    for p in range(1, P):
                        total = total + got["ms2_target"][p * G + g]
                    assert same(total, got["ms2_cond"][g]), g
                    if with_rest:
                        assert (got["ms2_rest"][g] == 0).all()


def test_refused_groups_are_nan_between_untouched_neighbours():
    K, P, G, n = 4, 2, 5, 9
    ms2, ms1 = pool(n, 16, 64, (16, 3), seed=2)
    d2, d1 = resident(ms2), resident(ms1)
    rng = np.random.default_rng(2)
    idx = np.stack([rng.permutation(n)[:K] for _ in range(G)], axis=1)
    count = np.array([2, 3, 4, 3, 2])
    base = run_group(d2, d1, idx, count, K, P, E=4, ids=IDS)
    assert not any(np.isnan(v).any() for v in base.values())
    assert all(same(base[k], v) for k, v in mix_group_batch_ref(ms2, ms1, idx, count, K, P, None, 4, SEED, IDS, 0, 1).items())

    def rows(k, g):  # the rows of group g in output k
        return [g] if k in ("ms2_rest", "weights_out") else [p * G + g for p in range(P)]

    def check(got, bad_groups):
        for k in GROUP_OUTS:
            hit = sorted(r for g in bad_groups for r in rows(k, g))
            keep = [r for r in range(len(base[k])) if r not in hit]
            assert np.isnan(got[k][hit]).all(), k
            assert np.array_equal(got[k][keep].view(np.uint32), base[k][keep].view(np.uint32)), k

    # rows j >= count are never read: wild indices there change nothing (NaN canaries show a read in the mix pass, 1e30 ones in the min / max)
    wild = idx.copy()
    for g in range(G):
        wild[count[g]:, g] = [n, -1][:K - count[g]]
    for canary in (float("nan"), 1e30):
        got = run_group(resident(ms2, canary), resident(ms1, canary), wild, count, K, P, E=4, ids=IDS)
        assert all(np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)) for k in GROUP_OUTS), canary
    # a count below P (a valid count for dq_mix_batch), above K, or 0
    for g, c in ((1, 1), (3, 5), (2, 0)):
        bad = count.copy()
        bad[g] = c
        check(run_group(d2, d1, idx, bad, K, P, E=4, ids=IDS), [g])
    # a used index out of range: a member's, or a later component's
    for g, j, v in ((0, 0, n), (0, 1, -1), (2, 3, n), (3, 2, 2 ** 40), (4, 1, -(2 ** 40))):
        poisoned = idx.copy()
        poisoned[j, g] = v
        check(run_group(d2, d1, poisoned, count, K, P, E=4, ids=IDS), [g])
    # two at once, first and last group
    bad = count.copy()
    bad[0], bad[4] = 1, 9
    check(run_group(d2, d1, idx, bad, K, P, E=4, ids=IDS), [0, 4])


def test_a_group_alone_is_the_group_in_its_batch():
    K, P, G, n = 3, 2, 4, 9
    ms2, ms1 = pool(n, 16, 64, (16,), seed=1)
    d2, d1 = resident(ms2), resident(ms1)
    rng = np.random.default_rng(1)
    idx = np.stack([rng.permutation(n)[:K] for _ in range(G)], axis=1)
    count = [3, 2, 3, 2]
    batch = run_group(d2, d1, idx, count, K, P, E=4, ids=IDS[:G], draw=2)
    for g in (0, 3):
        alone = run_group(d2, d1, idx[:, g:g + 1], count[g:g + 1], K, P, E=4, ids=IDS[g:g + 1], draw=2)
        for k in GROUP_OUTS:
            want = batch[k][g:g + 1] if k in ("ms2_rest", "weights_out") else batch[k][g::G]
            assert same(alone[k], want), (g, k)
    # under another id it draws other weights
    assert not np.array_equal(run_group(d2, d1, idx[:, 3:4], count[3:4], K, P, E=4, ids=[IDS[2]], draw=2)["weights_out"][0], batch["weights_out"][3])
