"""GPU parity AT THE SIZES THE BENCH IS QUOTED ON (BASELINE.json configs[1], [3], [4]), all through the C ABI, against the oracle:

  * configs[1]: ``_train_one_batch`` semantics at (32, 400, 64) -- loss and all 395 parameter gradients vs the per-sample oracle
    loop (batched semantics = the B = 1 reference applied to every sample, loss = mean over samples);
  * configs[3]: ``sample`` at B = 512, 50 steps, hipGraph replay -- windows 0 and 511 vs the oracle (per-step eps <= 1e-4 relative,
    the tolerance north_star states), batch independence bit for bit at windows {0, 1, 255, 510, 511} (B = 2 / B = 1 re-runs), x_T
    untouched, second output == mixture - denoised;
  * configs[4]: one (2000, 256) window -- forward eps, loss and all gradients vs the oracle;
  * determinism: two ``dq_train_step`` calls on the same inputs give bit-identical flat gradients and loss.

Tolerances (fp32): loss 2e-5 relative; per-step eps 1e-4 of the step's eps scale; parameter gradients 2e-5 of
max(|ref|, 1e-4 * largest gradient) per tensor -- ten times what the kernels show (a gradient that is analytically zero is round-off in the oracle too).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-5   # observed on MI355X: 1.1e-6 (batch 32), 1.8e-6 (2000 x 256)
EPS_TOL = 1e-4    # the tolerance north_star states; observed 3.5e-6 (50 steps), 7.8e-6 (2000 x 256)


def _net(mz, seed, perturb=0.05):
    from dquartic.model.unet1d import UNet1d

    torch.manual_seed(seed)
    net = UNet1d(dim=4, channels=1, dim_mults=(1, 2, 2, 3, 3, 4, 4), conditional=True, init_cond_channels=1,
                 attn_cond_channels=1, downsample_dim=mz, simple=True)
    with torch.no_grad():  # no fixture may hide a transposed or ignored weight: move every tensor off its init (gains off 1)
        for p in net.parameters():
            if p.requires_grad:
                p.add_(perturb * torch.randn_like(p))
    params = {k: v.detach().clone().cpu() for k, v in net.state_dict().items()}
    return net, params


def _oracle_grads(params, mz, x0, c2, c1, t, nz):
    """per-sample loop of the B = 1 oracle: loss = mean_b loss_b, gradients accumulated"""
    from oracle import dq_oracle as O

    po = {k: v.clone().requires_grad_(not k.endswith("freqs")) for k, v in params.items()}
    od = O.Diffusion(po, O.UNetConfig(downsample_dim=mz))
    B = x0.shape[0]
    losses, eps = [], []
    for b in range(B):
        lb, eb = od.train_loss(x0[b:b + 1], c2[b:b + 1], c1[b:b + 1], t[b:b + 1], nz[b:b + 1])
        (lb / B).backward()
        losses.append(float(lb))
        eps.append(eb.detach())
    return sum(losses) / B, torch.cat(eps), po


def _check_grads(net, po, tol=GRAD_TOL):
    from oracle import dq_oracle as O

    keys = O.trainable_keys(po)
    gmax = max(float(po[k].grad.abs().max()) for k in keys)
    named = dict(net.named_parameters())
    worst = ("", 0.0)
    for k in keys:
        ref = po[k].grad
        e = float((named[k].grad.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-4 * gmax)
        if e > worst[1]:
            worst = (k, e)
    assert len(keys) == 395
    assert worst[1] <= tol, worst
    return worst


_ORACLE_CACHE = {}


def _cached(key, fn):
    """the oracle side of a test that runs once per LinearAttention dispatch (la_form): computed once per session"""
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = fn()
    return _ORACLE_CACHE[key]


def test_train_one_batch_at_bench_size_vs_oracle(la_form):
    """configs[1]: batch 32 of (400, 64) windows -- the exact workload ``bench.py``'s ``value`` is quoted on, under every LinearAttention
    dispatch: ``default`` is the kernel set of the bench line (the library's own rule at 12,800 rows), ``rows`` / ``register`` force either
    form at every level it exists for."""
    from dquartic.model.model import DDIMDiffusionModel

    net, params = _net(64, 11)
    dm = DDIMDiffusionModel(model_class=net.cuda(), device="cuda")
    B, RT, MZ = 32, 400, 64
    g = torch.Generator().manual_seed(5)
    x0, c2, c1 = torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[0], t[1] = 0, 999  # both ends of the schedule are in the batch
    nz = torch.randn(B, RT, MZ, generator=g)
    lo, _, po = _cached("train32", lambda: _oracle_grads(params, MZ, x0, c2, c1, t, nz))
    net.train()
    loss = dm.train_step_fused(x0.cuda(), c2.cuda(), c1.cuda(), t=t.cuda(), noise=nz.cuda())
    assert abs(float(loss) - lo) < 2e-5 * abs(lo), (float(loss), lo)
    worst = _check_grads(net, po)
    print("batch-32 train step [%s]: loss" % la_form, float(loss), "oracle", lo, "worst grad", worst)
    # the optimiser half of _train_one_batch on the same gradients: pre-clip norm vs the oracle's
    gn_ref = float(torch.sqrt(sum((po[k].grad.double() ** 2).sum() for k in po if po[k].grad is not None)))
    dm._set_optimizer(1e-5)
    dm.optimizer.grad_scale = 1.0
    dm.optimizer.step()
    assert abs(float(dm.optimizer.last_grad_norm) - gn_ref) < 1e-4 * gn_ref


def test_train_step_at_reference_window_vs_oracle():
    """The reference's own window length, RT = 34 (MZ 64), at batch 128: 4,352 rows per level, so the deep levels' ResnetBlock backward
    takes the row form under the library's own rule (k_res_rows.hip), with a 2-row last tile in every sample of every such block.  Loss and
    all 395 gradients vs the per-sample oracle."""
    from dquartic import _native as N
    from dquartic.model.model import DDIMDiffusionModel

    B, RT, MZ = 128, 34, 64
    assert N.get_option("res_rows_bwd_min_rows") < 0 and B * RT >= N.get_option_effective("res_rows_bwd_min_rows")
    for cinA, cinB, C, n in ((12, 0, 12, 4), (12, 0, 12, 2), (16, 12, 16, 2), (12, 12, 12, 4), (12, 8, 12, 8)):  # the row-form blocks at MZ 64
        assert N.resblock_forms(cinA, cinB, C, B * RT, n, RT)[1] == "rows", (cinA, cinB, C, n)
    net, params = _net(MZ, 15)
    dm = DDIMDiffusionModel(model_class=net.cuda(), device="cuda")
    g = torch.Generator().manual_seed(9)
    x0, c2, c1 = torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    nz = torch.randn(B, RT, MZ, generator=g)
    lo, _, po = _oracle_grads(params, MZ, x0, c2, c1, t, nz)
    net.train()
    loss = dm.train_step_fused(x0.cuda(), c2.cuda(), c1.cuda(), t=t.cuda(), noise=nz.cuda())
    assert abs(float(loss) - lo) < 2e-5 * abs(lo), (float(loss), lo)
    worst = _check_grads(net, po)
    print("batch-128 RT-34 train step: loss", float(loss), "oracle", lo, "worst grad", worst)


def test_train_step_is_bitwise_repeatable():
    """two dq_train_step calls on the same inputs: identical loss and flat gradient, bit for bit (no order-dependent float
    atomics anywhere on the path; SURVEY section 5 'race detection')"""
    from dquartic.model.model import DDIMDiffusionModel

    net, _ = _net(64, 12)
    dm = DDIMDiffusionModel(model_class=net.cuda(), device="cuda")
    B, RT, MZ = 32, 400, 64
    g = torch.Generator().manual_seed(6)
    x0, c2, c1 = (torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, MZ, generator=g).cuda(), torch.rand(B, RT, generator=g).cuda())
    t, nz = torch.randint(0, 1000, (B,), generator=g).cuda(), torch.randn(B, RT, MZ, generator=g).cuda()
    runs = []
    for _ in range(3):
        loss = dm.train_step_fused(x0, c2, c1, t=t, noise=nz)
        torch.cuda.synchronize()
        runs.append((loss.clone(), net.flat_grads().clone()))
    for l, gr in runs[1:]:
        assert torch.equal(l, runs[0][0])
        assert torch.equal(gr, runs[0][1]), int((gr != runs[0][1]).sum())


def test_train_step_schedule_stress():
    """The same fused step queued back to back WITHOUT a synchronisation in between, many times: loss and gradients stay bit-identical.  The step runs
    on two queues that share scratch buffers; a missing ordering between them shows up as a run-to-run difference
    (tools/race_stress.py is the long form: 4 shapes x 300 steps, profiles/r04_race_stress.log)."""
    from dquartic.model.model import DDIMDiffusionModel

    net, _ = _net(64, 14)
    dm = DDIMDiffusionModel(model_class=net.cuda(), device="cuda")
    for B, RT, reps in ((3, 70, 100), (8, 400, 50)):
        g = torch.Generator().manual_seed(B)
        x0, c2, c1 = (torch.rand(B, RT, 64, generator=g).cuda(), torch.rand(B, RT, 64, generator=g).cuda(), torch.rand(B, RT, generator=g).cuda())
        t, nz = torch.randint(0, 1000, (B,), generator=g).cuda(), torch.randn(B, RT, 64, generator=g).cuda()
        ref = None
        bad = 0
        for _ in range(reps):
            loss = dm.train_step_fused(x0, c2, c1, t=t, noise=nz, zero_grads=True)
            cur = (loss.clone(), net.flat_grads().clone())
            if ref is None:
                ref = cur
            elif not (torch.equal(cur[0], ref[0]) and torch.equal(cur[1], ref[1])):
                bad += 1
        torch.cuda.synchronize()
        assert bad == 0, (B, RT, bad)


def test_sample_batch512_graph_vs_oracle_and_batch_independence(la_form):
    """configs[3]: 50-step DDIM sampling of 512 windows through the hipGraph-captured step, under every LinearAttention dispatch
    (``default`` at 204,800 rows = the per-row forward at the deep levels, as bench.py's sampling leg runs it).

    Every big kernel of the step is ONE resident round of workgroups that loops over tiles, so a dropped tail tile would be finite garbage
    in a HIGH window: batch independence is checked bit for bit at windows {0, 1, 255, 510, 511} (B = 2 / B = 1 re-runs of exactly those
    windows), and the oracle faces window 0 AND window 511."""
    from dquartic.model.model import DDIMDiffusionModel
    from oracle import dq_oracle as O

    net, params = _net(64, 13)
    dm = DDIMDiffusionModel(model_class=net.cuda(), device="cuda")
    assert dm.use_graph
    B, RT, MZ, NS = 512, 400, 64, 50
    g = torch.Generator().manual_seed(7)
    xT, c2, c1 = torch.randn(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    xd, c2d, c1d = xT.cuda(), c2.cuda(), c1.cuda()
    net.eval()
    with torch.no_grad():
        s, pn = dm.sample(xd, c2d, c1d, num_steps=NS)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), xT)                                         # x_T untouched
    assert float((pn - (c2d - s)).abs().max()) < 1e-6                        # model.py:321-322: mixture - denoised
    assert bool(torch.isfinite(s).all())
    # batch independence, bit for bit: each group of windows re-run alone (graph on), the first group also without the graph.  The product
    # picks the LinearAttention form by row count, so under the default rule a batch of 2 would take the OTHER forward form than the batch
    # of 512 (204,800 rows: the per-row form): the re-runs pin the form the big batch ran, and the small batch under its own rule is held
    # to the fp32 tolerance instead.
    from dquartic import _native as N
    if la_form == "default":
        assert B * RT >= N.get_option_effective("la_small_min_rows") and N.get_option("la_small_min_rows") < 0  # (the rule, not a forced value)
        with torch.no_grad():
            s_rule, _ = dm.sample(xd[:2].contiguous(), c2d[:2].contiguous(), c1d[:2].contiguous(), num_steps=NS)
        assert float((s_rule - s[:2]).abs().max() / s[:2].abs().max()) < 5e-4
        N.set_option("la_small_min_rows", 0)
    traj = {}
    for idx in ([0, 1], [255], [510, 511]):
        sel = torch.tensor(idx)
        with torch.no_grad():
            s2, pn2 = dm.sample(xd[sel].contiguous(), c2d[sel].contiguous(), c1d[sel].contiguous(), num_steps=NS)
            dm.use_graph = False
            s2e, _, tx, te = dm.sample(xd[sel].contiguous(), c2d[sel].contiguous(), c1d[sel].contiguous(), num_steps=NS, return_trajectory=True)
            dm.use_graph = True
        assert torch.equal(s2, s2e), idx
        assert torch.equal(s[sel.cuda()], s2) and torch.equal(pn[sel.cuda()], pn2), idx
        for j, w in enumerate(idx):
            traj[w] = [e[j:j + 1].cpu() for e in te]
    # windows 0 and 511 against the oracle (50 CPU steps per window): per-step eps (<= 1e-4 of the step's eps scale) and the denoised window;
    # the windows in between are tied to their own small-batch runs above, and those to the same kernels
    def oracle_window(w):
        tr = []
        with torch.no_grad():
            so, _ = O.Diffusion(params, O.UNetConfig(downsample_dim=64)).sample(xT[w:w + 1], c2[w:w + 1], c1[w:w + 1], NS, trace=tr)
        return so, [e for _, _, e in tr]
    for w in (0, 511):
        so, eps_o = _cached(("sample512", w), lambda: oracle_window(w))
        worst = 0.0
        for i, e in enumerate(eps_o):
            worst = max(worst, float((traj[w][i] - e).abs().max() / e.abs().max()))
        print("50-step sampling [%s], window %d: worst per-step eps rel err" % (la_form, w), worst, "final MSE", float(((s[w:w + 1].cpu() - so) ** 2).mean()))
        assert worst < EPS_TOL, (w, worst)
        assert float(((s[w:w + 1].cpu() - so) ** 2).mean()) < 1e-8           # denoised-MS2 MSE
        assert float((s[w:w + 1].cpu() - so).abs().max() / so.abs().max()) < 5e-4


def test_large_window_2000x256_vs_oracle():
    """configs[4]: one (2000, 256) window: 63 key blocks in the bottleneck attention, LinearAttention rows of 256 / 128 positions,
    bottleneck width 64.  Forward eps, loss and all gradients vs the oracle."""
    from dquartic.model.model import DDIMDiffusionModel
    from oracle import dq_oracle as O

    net, params = _net(256, 14)
    dm = DDIMDiffusionModel(model_class=net.cuda(), device="cuda")
    B, RT, MZ = 1, 2000, 256
    g = torch.Generator().manual_seed(8)
    x0, c2, c1 = torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, MZ, generator=g), torch.rand(B, RT, generator=g)
    t, nz = torch.tensor([412]), torch.randn(B, RT, MZ, generator=g)
    lo, eps_o, po = _oracle_grads(params, MZ, x0, c2, c1, t, nz)
    net.train()
    loss = dm.train_step_fused(x0.cuda(), c2.cuda(), c1.cuda(), t=t.cuda(), noise=nz.cuda())
    assert abs(float(loss) - lo) < 2e-5 * abs(lo), (float(loss), lo)
    worst = _check_grads(net, po)
    net.eval()
    with torch.no_grad():
        xt = O.q_sample(O.make_schedule()["alpha_bars"], O.normalize(x0), t, nz)
        y = net(xt.cuda(), t.cuda(), O.normalize(c2).cuda(), O.normalize(c1).cuda())
    e = float((y.cpu() - eps_o).abs().max() / eps_o.abs().max())
    print("2000x256 window: loss", float(loss), "oracle", lo, "eps rel err", e, "worst grad", worst)
    assert e < EPS_TOL, e
    # batch independence at this shape too: window 0 of a batch of two is the batch-1 result, bit for bit
    with torch.no_grad():
        x2 = torch.cat([xt, torch.rand(1, RT, MZ, generator=g) * 2 - 1]).cuda()
        t2 = torch.cat([t, torch.tensor([77])]).cuda()
        c22 = torch.cat([O.normalize(c2), torch.rand(1, RT, MZ, generator=g) * 2 - 1]).cuda()
        c12 = torch.cat([O.normalize(c1), torch.rand(1, RT, generator=g) * 2 - 1]).cuda()
        y2 = net(x2, t2, c22, c12)
    assert torch.equal(y2[:1], y)
