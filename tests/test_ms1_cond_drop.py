"""``dq_ms1_cond_drop`` (k_cond_drop.hip) against the numpy transcription of its drop rule
(tests/test_guidance_host.py): dropped windows equal the null exactly, kept windows are bit copies -- shapes (5, 4) and (5, 3, 3)
(M1 = 3: 45 floats, the 16-byte loop straddles windows and leaves a tail), a pointer 4 bytes off 16 (the one-element loop), p = 0,
``out`` aliased to ``in``, a window alone under its id, NULL ids and another draw.  Exact comparisons throughout: the kernel copies or
stores a constant."""
import ctypes

import numpy as np
import pytest
import torch

from test_guidance_host import DROP_P, cond_drop_ref, drop_mask
from test_stochastic_sampler import SEED, _dev_ids, _dev_seed

pytestmark = pytest.mark.gpu

NULL = -0.75
IDS = [0, 1, 2, 3, 4]  # what NULL ids mean; the seed of this file drops some and keeps some of them (test_guidance_host.py asserts it)


def run(ms1, ids, draw, p, offset=0, alias=False, null=NULL, null_ids=False):
    """the kernel on a device copy of ms1 (B, ...), input and output `offset` floats behind 16-byte aligned addresses, between canaries"""
    from dquartic import _native as N

    B, n = ms1.shape[0], ms1.numel()
    src = torch.full((n + 8,), 777.0, device="cuda")
    src[offset:offset + n] = ms1.reshape(-1).cuda()
    dst = src if alias else torch.full((n + 8,), 12345.0, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ids_d, seed_d = _dev_ids(list(ids)), _dev_seed(SEED)
    N.check(N.lib().dq_ms1_cond_drop(ctypes.c_void_p(src.data_ptr() + 4 * offset), ctypes.c_void_p(dst.data_ptr() + 4 * offset),
                                     None if null_ids else N.ptr(ids_d), N.ptr(seed_d), draw, ctypes.c_double(p), ctypes.c_float(null), B, n // B,
                                     N.stream_ptr()), "dq_ms1_cond_drop")
    out = dst.cpu()
    canary = 777.0 if alias else 12345.0
    assert (out[:offset] == canary).all() and (out[offset + n:] == canary).all()
    if not alias:
        assert torch.equal(src.cpu()[offset:offset + n].view(torch.int32), ms1.reshape(-1).view(torch.int32))  # the input is read only (bits: a NaN too)
    return out[offset:offset + n].reshape(ms1.shape).numpy()


@pytest.mark.parametrize("shape", [(5, 4), (5, 3, 3)])
def test_cond_drop_matches_the_transcription(shape):
    g = torch.Generator().manual_seed(3)
    ms1 = torch.rand(*shape, generator=g)
    m0 = drop_mask(SEED, IDS, 0, DROP_P)
    assert 1 <= int(m0.sum()) <= 4  # asserted on the transcription first: some windows dropped, some kept
    ref = cond_drop_ref(ms1.numpy(), SEED, IDS, 0, DROP_P, NULL)
    assert (ref[m0] == np.float32(NULL)).all() and np.array_equal(ref[~m0], ms1.numpy()[~m0])
    for kw in (dict(), dict(offset=1), dict(alias=True), dict(offset=1, alias=True), dict(null_ids=True)):
        out = run(ms1, IDS, 0, DROP_P, **kw)
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), kw  # dropped: the null exactly; kept: bit copies
    # p = 0: a bit copy of everything, whatever the draw
    for d in (0, 5):
        assert np.array_equal(run(ms1, IDS, d, 0.0), ms1.numpy())
    # other ids (64-bit), other draws, other probabilities
    ids = [7, 2 ** 33 + 1, 0, 2 ** 40, 3]
    for d, p in ((0, DROP_P), (1, DROP_P), (2, 0.25), (3, 0.9)):
        assert np.array_equal(run(ms1, ids, d, p), cond_drop_ref(ms1.numpy(), SEED, ids, d, p, NULL)), (d, p)
    # another draw changes the pattern: on the transcription first, then on the kernel
    d1 = next(d for d in range(1, 16) if not np.array_equal(drop_mask(SEED, IDS, d, DROP_P), m0))
    out0, out1 = run(ms1, IDS, 0, DROP_P), run(ms1, IDS, d1, DROP_P)
    assert not np.array_equal(out0, out1) and np.array_equal(out1, cond_drop_ref(ms1.numpy(), SEED, IDS, d1, DROP_P, NULL))
    # a window alone decides as it does in the batch, under its id (both loops)
    for b, w in enumerate(IDS):
        for off in (0, 1):
            assert np.array_equal(run(ms1[b:b + 1].contiguous(), [w], 0, DROP_P, offset=off), ref[b:b + 1]), (b, off)
    # a NaN in a kept window is copied, a NaN null is stored (bit patterns, no arithmetic)
    nan = ms1.clone()
    nan[~torch.from_numpy(m0)] = float("nan")
    out = run(nan, IDS, 0, DROP_P)
    assert np.isnan(out[~m0]).all() and (out[m0] == np.float32(NULL)).all()


def test_cond_drop_more_than_one_block():
    """(300, 7): 2100 floats -- three blocks of the 16-byte loop with windows straddling every lane, and a tail"""
    g = torch.Generator().manual_seed(4)
    ms1 = torch.rand(300, 7, generator=g)
    ids = list(range(100, 400))
    ref = cond_drop_ref(ms1.numpy(), SEED, ids, 2, 0.3, NULL)
    frac = float((ref == np.float32(NULL)).all(axis=1).mean())
    assert 0.2 < frac < 0.4, frac
    for off in (0, 1):
        assert np.array_equal(run(ms1, ids, 2, 0.3, offset=off), ref), off
