"""The product library's two schedules of the backward pass: weight gradients, slot reduces and the pieces nothing on the data-gradient chain waits
for on the side queue (``dq_plan_set_side_stream(plan, 1)``, the default) against everything on the caller's stream (``0``).  The queue decides
WHERE a launch runs, never what it computes: loss and flat gradients are bit-identical.  (tests/test_tiny_levels.py compares the same two
schedules on the development build, through its environment switches.)

B = 2, RT = 16 are the smallest shapes that still take every branch of the queue:
  * the default multipliers at m/z 64: the tiny levels, the hand-over of the collected slot reduces at level 2 (short rows), and the 16-channel
    bottleneck with its attention's front and back inside the ResnetBlock launches;
  * the same at m/z 128: long rows, no hand-over;
  * multipliers (1, 2, 2, 3) with 10 MS1 channels (tests/test_ms1_channels.py): the wide bottleneck, the multi-channel MS1 weight gradient.
Whoever asks for d loss / d x keeps the tail of the pass on the main stream: dq_unet_fwd + dq_unet_bwd with and without grad_x give the same
flat gradients."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, RT = 2, 16
CONFIGS = {
    "default_mz64": dict(dim_mults=(1, 2, 2, 3, 3, 4, 4), downsample_dim=64, attn_cond_channels=1),
    "default_mz128": dict(dim_mults=(1, 2, 2, 3, 3, 4, 4), downsample_dim=128, attn_cond_channels=1),
    "wide_mid": dict(dim_mults=(1, 2, 2, 3), downsample_dim=64, attn_cond_channels=10),
}


def _net(kw):
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(3)
    net = UNet1d(dim=4, channels=1, conditional=True, init_cond_channels=1, simple=True, **kw).cuda()
    with torch.no_grad():
        for _, p in net.trainable_named():
            p.add_(torch.randn_like(p) * 0.05)  # biases / gains off their initial 0 / 1
    return net


def _inputs(kw):
    g = torch.Generator().manual_seed(11)
    MZ, M1 = kw["downsample_dim"], kw["attn_cond_channels"]
    c1 = torch.rand(B, RT, M1, generator=g) if M1 > 1 else torch.rand(B, RT, generator=g)
    return (torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, MZ, generator=g).cuda(), c1.cuda(),
            torch.tensor([999, 3]).cuda(), torch.randn(B, RT, MZ, generator=g).cuda())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_train_step_is_bitwise_equal_with_and_without_the_side_stream(name):
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel

    kw = CONFIGS[name]
    net = _net(kw)
    dm = DDIMDiffusionModel(model_class=net, device="cuda")
    x0, c2, c1, t, noise = _inputs(kw)
    runs = {}
    try:
        for side in (1, 0, 1):
            N.check(N.lib().dq_plan_set_side_stream(net._plan, side), "dq_plan_set_side_stream")
            loss = dm.train_step_fused(x0, c2, c1, t=t, noise=noise, zero_grads=True)
            torch.cuda.synchronize()
            got = (loss.clone(), net.flat_grads().clone())
            assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[1]).all()) and float(got[1].abs().max()) > 0
            ref = runs.setdefault(side, got)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])  # (the forked step repeats itself)
    finally:
        N.lib().dq_plan_set_side_stream(net._plan, 1)
    assert torch.equal(runs[1][0], runs[0][0]), (float(runs[1][0]), float(runs[0][0]))
    assert torch.equal(runs[1][1], runs[0][1]), float((runs[1][1] - runs[0][1]).abs().max())


def test_backward_gradients_do_not_depend_on_grad_x():
    from dquartic import _native as N

    kw = CONFIGS["default_mz64"]
    net = _net(kw)
    x, c2, c1, t, gout = _inputs(kw)
    xs, ts, ic, ac, _, _, _ = net._prep(x, t, c2, c1)
    net._ensure_flat()
    ws = net.workspace(B, RT, True)

    def pair(want_gx):
        net._run_fwd(xs, ts, ic, ac, training=True, ws=ws)
        grads = torch.zeros_like(net.flat_params)
        gx = torch.full_like(xs, float("nan")) if want_gx else None
        N.check(N.lib().dq_unet_bwd(net._plan, N.ptr(net.flat_params), N.ptr(net.rope_freqs()), N.ptr(ic), 1.0, 0.0, N.ptr(gout), N.ptr(grads),
                                    N.ptr(gx), N.ptr(ws), ws.numel(), B, RT, N.stream_ptr()), "dq_unet_bwd")
        torch.cuda.synchronize()
        return grads, gx

    with_gx, gx = pair(True)
    without, _ = pair(False)
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    assert float(without.abs().max()) > 0
    assert torch.equal(with_gx, without), float((with_gx - without).abs().max())
