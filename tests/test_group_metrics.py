"""``dq_group_metrics`` (k_group_metrics.hip) on the GPU against the float64 statement of tests/group_eval_ref.py.

The bound, per output: one fp32 rounding of the reference, 2^-24 |ref|, plus n 2^-52 times the same ratio formed over absolute values
(``group_metrics_ref`` returns both terms added up): an fp64 sum of n terms carries at most n roundings of 2^-53 relative to the sum of
the terms' magnitudes, in the numerator and in the denominator.  The worst observed share of the bound is printed per case.

The partition's boundaries (csrc/k_group_metrics.hip): a block takes a chunk of 4096 elements of a window in passes of 256 lanes x 4
elements, so a window of 1024 elements is exactly one pass of one block and 1025 the first lane's second pass; 4096 is exactly one chunk
and 4097 the second block's first element.  Lanes read 16 bytes where RT * MZ % 4 == 0 and the three tensors are 16-byte aligned, four
bytes otherwise: every shape runs at both alignments where it can, and the two forms must give the same bits."""
import numpy as np
import pytest
import torch

from group_eval_ref import group_metrics_ref

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, 12345.0
SHAPES = [(1, 1), (3, 5), (7, 4), (16, 64), (5, 205), (64, 64), (17, 241)]  # n = 1, 15, 28, 1024 | 1025, 4096 | 4097


def on_device(a, off):
    """a host array as a contiguous device tensor whose base pointer is `off` floats past a 16-byte boundary"""
    buf = torch.empty(a.size + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * off
    return v


def run(pred, target, mix, P, off=0):
    """(cross (G, P, P), group (G, 3)) as host arrays; outputs and scratch sit between sentinels"""
    from dquartic import _native as N

    G, RT, MZ = mix.shape
    d = [on_device(np.ascontiguousarray(a, dtype=np.float32), off) for a in (pred, target, mix)]
    nbytes = N.lib().dq_group_metrics_scratch_bytes(G, P, RT, MZ)
    assert nbytes == 8 * G * (P + 1) * (P + 2) * ((RT * MZ + 4095) // 4096)
    bufs = [torch.full((k + 2 * PAD,), SENTINEL, device="cuda") for k in (G * P * P, G * 3)]
    scratch = torch.full((nbytes // 8 + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    N.check(N.lib().dq_group_metrics(N.ptr(d[0]), N.ptr(d[1]), N.ptr(d[2]), N.ptr(bufs[0][PAD:]), N.ptr(bufs[1][PAD:]), N.ptr(scratch[PAD:]),
                                     nbytes, G, P, RT, MZ, N.stream_ptr()), "dq_group_metrics")
    torch.cuda.synchronize()
    for b in bufs + [scratch]:
        h = b.cpu()
        assert bool((h[:PAD] == SENTINEL).all() and (h[-PAD:] == SENTINEL).all())  # nothing outside an output is written
    return bufs[0][PAD:-PAD].cpu().numpy().reshape(G, P, P), bufs[1][PAD:-PAD].cpu().numpy().reshape(G, 3)


def data(P, G, RT, MZ, seed):
    """predictions with negative parts around targets that overlap (the members share peaks), and a mixture near their sum"""
    rng = np.random.default_rng(seed)
    shared = rng.random((1, G, RT, MZ))
    target = (0.6 * rng.random((P, G, RT, MZ)) + 0.4 * shared).astype(np.float32)
    pred = (target + 0.3 * rng.standard_normal((P, G, RT, MZ))).astype(np.float32)
    mix = (target.sum(0) * rng.uniform(0.7, 1.3, (G, RT, MZ)) - 0.1).astype(np.float32)  # some elements negative: m+ = 0 there
    return pred.reshape(P * G, RT, MZ), target.reshape(P * G, RT, MZ), mix


def within(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("RT,MZ", SHAPES)
def test_against_float64(RT, MZ, P, G):
    from dquartic.model import evaluation as E

    pred, target, mix = data(P, G, RT, MZ, seed=RT * MZ + P)
    cross_ref, group_ref, b_cross, b_group = group_metrics_ref(pred, target, mix, P)
    results = []
    for off in (0, 1):  # 16-byte aligned; 4 bytes off (the one-element form, also what per % 4 != 0 takes at any alignment)
        cross, group = run(pred, target, mix, P, off)
        share = max(within(cross, cross_ref, b_cross), within(group, group_ref, b_group))
        print(f"group_metrics ({RT}, {MZ}) P={P} G={G} off={off}: worst share of the bound {share:.3f}")
        results.append((cross, group))
    assert np.array_equal(results[0][0].view(np.uint32), results[1][0].view(np.uint32))  # the two access forms: the same bits
    assert np.array_equal(results[0][1].view(np.uint32), results[1][1].view(np.uint32))
    cross, group = results[0]
    # the diagonal is dq_recon_metrics' cosine of window p G + g, within 1 fp32 ulp
    cos = E.recon_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()).cpu().numpy()[:, 2].reshape(P, G)
    for g in range(G):
        for p in range(P):
            assert abs(float(cross[g, p, p]) - float(cos[p, g])) <= float(np.spacing(np.abs(cos[p, g]))), (g, p)
    # a repeat equals itself, and a group alone equals the group in its batch, bit for bit
    again = run(pred, target, mix, P)
    assert np.array_equal(again[0].view(np.uint32), cross.view(np.uint32)) and np.array_equal(again[1].view(np.uint32), group.view(np.uint32))
    if G > 1:
        g = G - 1
        alone = run(pred[g::G], target[g::G], mix[g:g + 1], P)
        assert np.array_equal(alone[0][0].view(np.uint32), cross[g].view(np.uint32)), g
        assert np.array_equal(alone[1][0].view(np.uint32), group[g].view(np.uint32)), g


def test_the_stated_zeros():
    P, G, RT, MZ = 3, 3, 7, 4
    pred, target, mix = data(P, G, RT, MZ, seed=5)
    pred, target, mix = pred.copy(), target.copy(), mix.copy()
    pred[0 * G + 0] = 0.0      # group 0: member 0 predicts nothing
    target[1 * G + 0] = 0.0    # group 0: member 1 has no target
    mix[1] = -np.abs(mix[1])   # group 1: nothing positive in the mixture
    pred[2::G] = -np.abs(pred[2::G])  # group 2: every member all negative
    cross, group = run(pred, target, mix, P)
    cross_ref, group_ref, b_cross, b_group = group_metrics_ref(pred, target, mix, P)
    within(cross, cross_ref, b_cross)
    within(group, group_ref, b_group)
    assert (cross[0, 0, :] == 0).all() and (cross[0, :, 1] == 0).all() and cross[0, 1, 0] != 0 and cross[0, 2, 2] > 0
    assert group[1].tolist() == [0.0, 0.0, 0.0]  # a zero mixture: both ratios are 0, not 0 / 0
    assert group[2, 0] == 0.0 and group[2, 1] == 1.0 and group[2, 2] > 0  # S = 0: nothing in excess, everything unexplained
    assert (cross[2] <= 0).all() and (cross[2] < 0).any()  # (all-negative predictions against positive targets)
    # an exact case: two members that split the mixture exactly, each on its own target
    t = np.zeros((2, 1, 2, 4), dtype=np.float32)
    t[0, 0, 0], t[1, 0, 1] = [1, 2, 3, 4], [4, 3, 2, 1]
    cross, group = run(t.reshape(2, 2, 4), t.reshape(2, 2, 4), t.sum(0), 2)
    assert cross[0].tolist() == [[1.0, 0.0], [0.0, 1.0]] and group[0].tolist() == [0.0, 0.0, 20.0]
    cross, group = run(2 * t.reshape(2, 2, 4), t.reshape(2, 2, 4), t.sum(0), 2)
    assert cross[0].tolist() == [[1.0, 0.0], [0.0, 1.0]] and group[0].tolist() == [1.0, 0.0, 20.0]
