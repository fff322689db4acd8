"""``dq_group_project`` (csrc/k_group.hip) on the GPU against tests/joint_ref.py: the numpy fp32 transcription BIT FOR
BIT, and the float64 rule within the running bound derived there (u = 2^-24 per fp32 operation on the path, operands' errors carried to
first order; elements whose float64 sum lies within four bounds of 0 are left to the bit-for-bit check).

Every combination of P in {1, 2, 3, 8}, the three objectives, both modes, auto_normalize on / off and strength in {1, 0.5} runs over the
shapes at which the kernel can go wrong:
  per = 4, G = 3     one lane-step per window of the 16-byte form
  per = 6, G = 3     no multiple of 4: the one-element form
  per = 8, G = 2     x0_out 4 bytes off 16-byte alignment: the one-element form by alignment, between canaries
  per = 12, G = 1    a single group
  in place           x0_out == net
  a later row        coef_dev pointing at row 2 of a table (the device-side step counter, which the stand-alone entry does not take, is
                     covered by captured == eager in tests/test_joint_sample.py: replays 1 and 2 read rows 1 and 2)
and once each form walks more than a full sweep of the grid (2048 blocks of 256 lanes): 524296 lane-steps, 8 of them in the second sweep.
A group's result does not depend on G: alone equals inside a batch."""
import ctypes

import numpy as np
import pytest
import torch

import joint_ref as R
from joint_ref import F

pytestmark = pytest.mark.gpu

ROWS = np.array([[0.31, 0.95, 0.0, 0.0], [0.9, 0.44, 0.0, 0.0], [0.8, 0.6, 0.0, 0.0]], dtype=F)  # [sa, sb, -, -]
CANARY = 12345.0


def project(pred, x, net, mix, row, mode, strength, normalize, in_place=False, offset=0, table_row=0):
    """one dq_group_project call on device copies -> x0' (P, G, per) as numpy.  offset: x0_out sits that many floats behind a 16-byte
    aligned address, between canaries; table_row: coef_dev points at that row of a table whose other rows would give something else"""
    from dquartic import _native as N

    P, G, per = net.shape
    xd, nd, md = torch.from_numpy(x).cuda(), torch.from_numpy(net).cuda(), torch.from_numpy(mix).cuda()
    table = np.full((table_row + 1, 4), 7.0, dtype=F)
    table[table_row] = row
    cd = torch.from_numpy(table).cuda()
    n = net.size
    buf = torch.full((n + 8,), CANARY, device="cuda")
    assert all(t.data_ptr() % 16 == 0 for t in (xd, nd, md, cd, buf))
    out_ptr = N.ptr(nd) if in_place else ctypes.c_void_p(buf.data_ptr() + 4 * offset)
    N.check(N.lib().dq_group_project(N.ptr(xd), N.ptr(nd), out_ptr, N.ptr(md), ctypes.c_void_p(cd.data_ptr() + 16 * table_row), R.PREDS[pred],
                                     1 if normalize else 0, G, P, per, R.MODES[mode], ctypes.c_float(strength), N.stream_ptr()),
            "dq_group_project")
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(md.cpu().numpy(), mix)
    if in_place:
        assert (buf == CANARY).all()
        return nd.cpu().numpy()
    assert np.array_equal(nd.cpu().numpy(), net)
    b = buf.cpu().numpy()
    assert (b[:offset] == CANARY).all() and (b[offset + n:] == CANARY).all()
    return b[offset:offset + n].reshape(P, G, per)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


SHAPES = (dict(G=3, per=4), dict(G=3, per=6), dict(G=2, per=8, offset=1), dict(G=1, per=12), dict(G=2, per=8, in_place=True),
          dict(G=2, per=8, table_row=2), dict(G=3, per=6, in_place=True))


@pytest.mark.parametrize("pred", list(R.PREDS))
@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_bits_of_the_transcription_and_the_float64_bound(P, pred):
    rng = np.random.default_rng(1000 * P + R.PREDS[pred])
    moved = 0
    for si, shape in enumerate(SHAPES):
        shape = dict(shape)
        G, per = shape.pop("G"), shape.pop("per")
        x, net, mix = R.inputs(rng, P, G, per)
        row = ROWS[si % len(ROWS)]
        x0 = R.x0_f32(pred, row[0], row[1], x, net)
        for mode in R.MODES:
            for normalize in (True, False):
                for strength in (1.0, 0.5):
                    got = project(pred, x, net, mix, row, mode, strength, normalize, **shape)
                    want, _ = R.project_f32(x0, mix, mode, strength, normalize)
                    assert same_bits(got, want), (shape, G, per, mode, normalize, strength, np.abs(got - want).max())
                    ref, bound = R.project_f64(pred, row[0], row[1], x, net, mix, mode, strength, normalize)
                    ok = np.isfinite(bound)
                    assert (np.abs(got - ref)[ok] <= bound[ok]).all(), (shape, mode, normalize, strength)
                    moved += int((got != x0).sum())
    assert moved > 0  # (the pass did something: the cases are not all under their mixtures)


@pytest.mark.parametrize("form", ["vector", "one_element"])
def test_longer_than_a_full_sweep_of_the_grid(form):
    """2048 blocks x 256 lanes = 524288 lane-steps per sweep; 524296 are asked for, so the last 8 belong to the first lanes' second turn"""
    G, per, P = (4, 524296, 1) if form == "vector" else (4, 131074, 2)  # (per % 4 == 0: 16-byte form, G per / 4 lane-steps; per % 4 == 2: G per)
    assert (G * per // 4 if form == "vector" else G * per) == 524296
    rng = np.random.default_rng(3)
    x, net, mix = R.inputs(rng, P, G, per)
    row = ROWS[1]
    got = project("v_prediction", x, net, mix, row, "bound", 1.0, True)
    want, q = R.project_f32(R.x0_f32("v_prediction", row[0], row[1], x, net), mix, "bound", 1.0, True)
    assert same_bits(got, want)
    tail = (got != R.x0_f32("v_prediction", row[0], row[1], x, net))[:, -1, -32:]
    assert tail.any()  # the second sweep's elements were projected, not just copied


def test_a_group_alone_is_the_group_in_a_batch():
    rng = np.random.default_rng(11)
    for P, per in ((3, 8), (2, 6), (8, 4)):
        G = 5
        x, net, mix = R.inputs(rng, P, G, per)
        for pred in R.PREDS:
            for mode in R.MODES:
                whole = project(pred, x, net, mix, ROWS[2], mode, 0.5, True)
                for g in (0, 3, 4):
                    alone = project(pred, np.ascontiguousarray(x[:, g:g + 1]), np.ascontiguousarray(net[:, g:g + 1]),
                                    np.ascontiguousarray(mix[g:g + 1]), ROWS[2], mode, 0.5, True)
                    assert same_bits(alone, np.ascontiguousarray(whole[:, g:g + 1])), (P, per, pred, mode, g)


def test_nothing_to_do():
    from dquartic import _native as N

    d = torch.zeros(16, device="cuda")
    for G, per in ((0, 8), (2, 0)):
        assert N.lib().dq_group_project(N.ptr(d), N.ptr(d), N.ptr(d), N.ptr(d), N.ptr(d), 0, 1, G, 2, per, 1, ctypes.c_float(1.0), N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (d == 0).all()
