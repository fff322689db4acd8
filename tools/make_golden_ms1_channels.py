#!/usr/bin/env python3
"""Generate tests/golden/ms1_channels.npz by running the REFERENCE's UNet1d with a multi-channel MS1 on the CPU.

Runs where the reference checkout is at hand only (``DQ_REFERENCE``, as oracle/make_golden.py); nothing of the reference is copied:

    python tools/make_golden_ms1_channels.py            # writes tests/golden/ms1_channels.npz
    python tools/make_golden_ms1_channels.py --verify   # writes nothing: regenerates and compares every array bit for bit

Configuration: ``UNet1d(dim=4, dim_mults=(1, 2, 2, 3), channels=1, init_cond_channels=1, attn_cond_channels=10, downsample_dim=64,
simple=True)`` at RT = 16, B = 1, RoPE disabled (the identity stand-in of oracle/make_golden.py: RoPE stays "parity unpinned").  The
reference folds a 3-D ``attn_cond (B, RT, M1)`` to ``(B, M1, RT)`` in front of ``attn_cond_proj`` (unet1d.py:1122-1130).

Contents (data only, packed so that the file stays below 1 MiB -- the bottleneck of this configuration has 96 channels, 200k weights):
  * the weights: the reference's default initialisation plus a seeded perturbation, ROUNDED TO MULTIPLES OF 2**-8 BEFORE the reference runs,
    so that ``w_q`` (int16, value * 256, all tensors of ``w_names`` / ``w_shapes`` back to back in state_dict order) holds them exactly;
    ``freqs`` is the one non-trainable state_dict entry (``mid_attn.fn.fn.rotary_emb.freqs``);
  * seeded ``x``, ``init_cond``, ``attn_cond (1, 16, 10)``, ``t``, ``gout``; the reference's ``y``, ``dx``, ``dinit_cond``, ``dattn_cond`` for
    ``(y * gout).sum()``, exact;
  * ``g_flat``: every parameter gradient (``g_names``, shapes as in ``w_shapes``) back to back, float32 ROUNDED TO 16 MANTISSA BITS (relative
    error <= 2**-17 = 7.6e-6 per element, a thirteenth of the tightest tolerance the fixture is compared at; 200k incompressible floats
    would not fit otherwise);
  * ``init_sum`` (float64) / ``init_head`` (first <= 4 values, zero-padded): per-tensor checksums of the default initialisation under
    ``torch.manual_seed(123)``, in ``w_names`` order with ``freqs`` last.

``unpack(npz)`` returns ``(state_dict, grads, init_sum, init_head)`` as dictionaries of arrays.
"""
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
NAME = "ms1_channels.npz"
CFG = dict(dim=4, dim_mults=(1, 2, 2, 3), channels=1, conditional=True, init_cond_channels=1, attn_cond_channels=10, tfer_dim_mult=620,
           downsample_dim=64, simple=True)
B, RT, MZ, M1 = 1, 16, 64, 10
FREQS = "mid_attn.fn.fn.rotary_emb.freqs"


def unpack(g):
    """(state_dict, grads, init_sum, init_head) from the loaded file: dictionaries of numpy arrays keyed by state_dict name."""
    names = [str(k) for k in g["w_names"]]
    shapes = {k: tuple(int(v) for v in row if v) for k, row in zip(names, g["w_shapes"])}
    wq, sd, off = g["w_q"].astype(np.float32) / np.float32(256.0), {}, 0
    for k in names:
        n = int(np.prod(shapes[k]))
        sd[k] = wq[off:off + n].reshape(shapes[k])
        off += n
    assert off == wq.size
    out_sd = {}
    for k in names:  # the reference registers rotary_emb ahead of to_qv
        if k == "mid_attn.fn.fn.to_qv.weight":
            out_sd[FREQS] = g["freqs"]
        out_sd[k] = sd[k]
    grads, off = {}, 0
    for k in (str(k) for k in g["g_names"]):
        n = int(np.prod(shapes[k]))
        grads[k] = g["g_flat"][off:off + n].reshape(shapes[k])
        off += n
    assert off == g["g_flat"].size
    order = names + [FREQS]
    return out_sd, grads, dict(zip(order, g["init_sum"])), dict(zip(order, g["init_head"]))


def generate(path):
    from oracle.make_golden import _import_reference, npd, randomize_

    _, U, rope = _import_reference()
    rope.RotaryEmbedding.IDENTITY = True
    try:
        torch.manual_seed(29)
        g = torch.Generator().manual_seed(2910)
        net = U.UNet1d(**CFG)
        randomize_(net, g)
        with torch.no_grad():
            for n_, p_ in net.named_parameters():
                if n_ != FREQS:
                    p_.copy_(torch.round(p_ * 256.0) / 256.0)
        x = torch.randn(B, RT, MZ, generator=g).requires_grad_(True)
        c2 = torch.randn(B, RT, MZ, generator=g).requires_grad_(True)
        c1 = torch.randn(B, RT, M1, generator=g).requires_grad_(True)
        t = torch.tensor([417])
        gout = torch.randn(B, RT, MZ, generator=g)
        y = net(x, t, c2, c1)
        (y * gout).sum().backward()
        out = {"x": x, "init_cond": c2, "attn_cond": c1, "t": t, "gout": gout, "y": y, "dx": x.grad, "dinit_cond": c2.grad,
               "dattn_cond": c1.grad}
        sd = net.state_dict()
        names = [k for k in sd if k != FREQS]
        out["w_names"] = np.array(names)
        out["w_shapes"] = np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in names], np.int32)
        wq = torch.cat([sd[k].reshape(-1) for k in names]) * 256.0
        assert torch.equal(wq, wq.round()) and float(wq.abs().max()) < 32768
        out["w_q"] = wq.to(torch.int16)
        out["freqs"] = sd[FREQS]
        grads = {n_: p_.grad for n_, p_ in net.named_parameters() if p_.grad is not None}
        out["g_names"] = np.array(list(grads))
        gf = torch.cat([v.reshape(-1) for v in grads.values()]).numpy().view(np.uint32).astype(np.uint64)
        out["g_flat"] = (((gf + 0x40 + ((gf >> 7) & 1) - 1) >> 7) << 7).astype(np.uint32).view(np.float32)  # round to nearest even at bit 7
        torch.manual_seed(123)
        isd = U.UNet1d(**CFG).state_dict()
        order = names + [FREQS]
        out["init_sum"] = np.array([isd[k].double().sum().item() for k in order], np.float64)
        out["init_head"] = np.stack([np.pad(isd[k].reshape(-1)[:4].numpy(), (0, max(0, 4 - isd[k].numel()))) for k in order])
    finally:
        rope.RotaryEmbedding.IDENTITY = False
    np.savez_compressed(path, **npd(out))
    return path


def main(argv):
    out = os.path.join(REPO, "tests", "golden", NAME)
    if "--verify" in argv:
        new = np.load(generate(os.path.join(tempfile.mkdtemp(prefix="dq_ms1_golden_"), NAME)))
        old = np.load(out)
        keys = sorted(set(new.files) | set(old.files))
        diff = [k for k in keys if k not in new.files or k not in old.files or new[k].shape != old[k].shape or new[k].dtype != old[k].dtype
                or new[k].tobytes() != old[k].tobytes()]
        print(f"[verify] regenerate {NAME}: {len(keys) - len(diff)} / {len(keys)} arrays bit-identical" + (f"; DIFFERENT: {diff[:8]}" if diff else ""))
        return 1 if diff else 0
    generate(out)
    print(NAME, os.path.getsize(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
