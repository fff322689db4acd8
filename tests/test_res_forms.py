"""The ResnetBlock row-form backward (k_res_rows.hip, k_res_rows_bwd<C, N, WR>) against a float64 oracle, instantiation by instantiation.

In the product the row form takes a block from res_rows_bwd_min_rows rows on (the device rule: 16 x compute units, 4,096 rows on
MI355X).  The option of that name forces it at a few rows, so each of the 12 instantiations (C in {12, 16} x N in {2, 4, 8} x with /
without res_conv) runs here at the channel splits the network uses and at the row counts where a tiled kernel goes wrong: a tile short of
/ one over 16 rows, the reference's RT = 34 (a 2-row last tile and a fourth wave without rows), one workgroup and one row more, and 7
workgroups per sample.  Every case first asserts the form the library reports (dq_resblock_forms), so a moved threshold or predicate
fails here instead of silently testing another kernel.

Reference: oracle.dq_oracle's block / _scale_shift in float64, with d(scale, shift) taken per sample (the scale / shift vector is a leaf).
Tolerances are those of tests/test_blocks_gpu.py::test_resnet_block_backward_vs_oracle_autograd, as max-abs error over max |ref|.
The gradient buffers sit inside larger ones with canaries on both sides; every launch must leave them untouched."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

OUT_TOL, DX_TOL, W_TOL, DSS_TOL = 1e-5, 2e-5, 5e-5, 5e-5
RES_KEYS = ("mlp.1.weight", "mlp.1.bias", "block1.proj.weight", "block1.proj.bias", "block1.norm.g", "block2.proj.weight",
            "block2.proj.bias", "block2.norm.g", "res_conv.weight", "res_conv.bias")
HEAD, TAIL, CANARY = 64, 4096, 7251.0  # floats before / after each gradient view (the tail holds more than a tile's 15 dead rows)


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


@pytest.fixture
def forced(N):
    """the row form at every row count; the default rule again afterwards"""
    N.set_option("res_rows_bwd_min_rows", 0)
    yield
    N.set_option("res_rows_bwd_min_rows", -1)


def err(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double().reshape(a.shape)
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def make_case(C, cinA, cinB, n, B, rps, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    cin = cinA + cinB
    wd = {"mlp.1.weight": r(2 * C, 16) * 0.3, "mlp.1.bias": r(2 * C) * 0.1, "block1.proj.weight": r(C, cin, 3) * 0.3,
          "block1.proj.bias": r(C) * 0.1, "block1.norm.g": torch.rand(1, C, 1, generator=gen) + 0.5,
          "block2.proj.weight": r(C, C, 3) * 0.3, "block2.proj.bias": r(C) * 0.1, "block2.norm.g": torch.rand(1, C, 1, generator=gen) + 0.5}
    if cin != C:
        wd["res_conv.weight"], wd["res_conv.bias"] = r(C, cin, 1) * 0.3, r(C) * 0.1
    rows = B * rps
    return wd, r(rows, cin, n), r(B, 16), r(rows, C, n)


def reference(wd, x, temb, gy, rps):
    """float64: out, dx, the weight gradients and d(scale, shift) per sample (B, 2C)"""
    from oracle import dq_oracle as O

    p = {"b." + k: v.double().requires_grad_() for k, v in wd.items()}
    xo, td = x.double().requires_grad_(), temb.double()
    ssv = torch.cat(O._scale_shift(p, "b", td, 1), dim=1)[:, :, 0].detach().requires_grad_()  # sample b's [scale | shift]: a leaf
    scale, shift = ssv.repeat_interleave(rps, dim=0)[:, :, None].chunk(2, dim=1)
    h = O.block(p, "b.block2", O.block(p, "b.block1", xo, (scale, shift)))
    y = h + (F.conv1d(xo, p["b.res_conv.weight"], p["b.res_conv.bias"]) if "b.res_conv.weight" in p else xo)
    with torch.no_grad():  # the leaf path is the oracle's block
        assert float((y - O.resnet_block(p, "b", xo, td, rps)).abs().max()) < 1e-12
    (y * gy.double()).sum().backward()
    return y.detach(), xo.grad, {k: p["b." + k].grad for k in wd if not k.startswith("mlp.")}, ssv.grad


class Block:
    """one ResnetBlock through dq_resblock_fwd / dq_resblock_bwd; the input gradients are views into canary-padded buffers"""

    def __init__(self, N, wd, x, temb, cinA, rps):
        self.N, self.L = N, N.lib()
        self.rows, cin, self.n = x.shape
        self.C, self.cinA, self.cinB, self.rps = wd["block1.proj.weight"].shape[0], cinA, cin - cinA, rps
        self.keys = [k for k in RES_KEYS if k in wd]
        self.sizes = [wd[k].numel() for k in self.keys]
        self.flat = torch.cat([wd[k].reshape(-1) for k in self.keys]).cuda()
        self.xA = x[:, :cinA].contiguous().cuda()
        self.xB = x[:, cinA:].contiguous().cuda() if self.cinB else None
        self.temb = temb.cuda()
        self.nws = self.L.dq_resblock_workspace_floats(cin, self.C, self.rows, self.n, rps)
        assert self.nws > 0
        self.ws = torch.empty(self.nws, device="cuda")
        self.bufs = []
        self.dA = self._padded(self.rows * cinA * self.n)
        self.dB = self._padded(self.rows * self.cinB * self.n) if self.cinB else None

    def _padded(self, m):
        buf = torch.full((HEAD + m + TAIL,), CANARY, device="cuda")
        view = buf[HEAD:HEAD + m]
        assert view.data_ptr() % 16 == 0
        self.bufs.append(buf)
        return view

    def canaries_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:HEAD] == CANARY).all()) and bool((b[-TAIL:] == CANARY).all()) for b in self.bufs)

    def forms(self):
        return self.N.resblock_forms(self.cinA, self.cinB, self.C, self.rows, self.n, self.rps)

    def forward(self):
        out = torch.empty(self.rows, self.C, self.n, device="cuda")
        self.N.check(self.L.dq_resblock_fwd(self.N.ptr(self.flat), self.N.ptr(self.xA), self.cinA, self.N.ptr(self.xB), self.cinB,
                                            self.N.ptr(self.temb), self.N.ptr(out), self.C, self.rows, self.n, self.rps, 1,
                                            self.N.ptr(self.ws), self.nws, self.N.stream_ptr()), "dq_resblock_fwd")
        return out

    def fill(self, how):
        """the interiors of dA / dB: 'zero', 'nan' or a random prefill (returned)"""
        pre = []
        for d in (self.dA, self.dB):
            if d is None:
                pre.append(None)
            elif how == "zero":
                d.zero_()
            elif how == "nan":
                d.fill_(float("nan"))
            else:
                d.copy_(torch.randn(d.numel(), generator=how) * 0.5)
            pre.append(None if d is None else d.clone())
        return pre

    def backward(self, gy):
        """gy given: dA / dB accumulate, dss copied out.  gy None: the gradient of the output was placed at dq_resblock_dout_offset and
        dA / dB are stored (first writer); dss is not copied out."""
        grads = torch.zeros_like(self.flat)
        dss = torch.full((self.rows // self.rps, 2 * self.C), float("nan"), device="cuda")
        gyd = gy.contiguous().cuda() if gy is not None else None
        self.N.check(self.L.dq_resblock_bwd(self.N.ptr(self.flat), self.N.ptr(self.xA), self.cinA, self.N.ptr(self.xB), self.cinB,
                                            self.N.ptr(gyd), self.N.ptr(self.dA), self.N.ptr(self.dB), self.N.ptr(grads), self.N.ptr(dss),
                                            self.C, self.rows, self.n, self.rps, self.N.ptr(self.ws), self.nws, self.N.stream_ptr()),
                     "dq_resblock_bwd")
        torch.cuda.synchronize()
        gd, o = {}, 0
        for k, m in zip(self.keys, self.sizes):
            gd[k] = grads[o:o + m]
            o += m
        return gd, dss

    def place_dout(self, gy):
        off = self.L.dq_resblock_dout_offset(self.cinA + self.cinB, self.C, self.rows, self.n, self.rps)
        assert off >= 0 and off + gy.numel() <= self.nws
        self.ws[off:off + gy.numel()].copy_(gy.reshape(-1))

    def dx(self, pre=(None, None)):
        parts = []
        for d, p, c in ((self.dA, pre[0], self.cinA), (self.dB, pre[1], self.cinB)):
            if d is not None:
                parts.append((d.double() - p.double() if p is not None else d.double()).reshape(self.rows, c, self.n))
        return torch.cat(parts, dim=1)


def check_grads(gd, ref_g, what):
    worst = max((err(gd[k], ref_g[k]), k) for k in ref_g)
    assert worst[0] < W_TOL, (what, worst)
    return worst[0]


# (C, cinA, cinB, n, rows per sample).  Downs: identity residual (WR = false).  Ups: cat(x, skip) with res_conv at the splits of
# dim_mults (1, 2, 2, 3, 3, 4, 4) at MZ 64 / 256, plus a narrow skip and one off-network block (cinA != C, no skip).  Each instantiation
# runs at RT = 34 and at two other row counts; every row count of {2, 15, 16, 17, 34, 64, 65, 400} appears.
MATRIX = [
    (12, 12, 0, 2, 34), (12, 12, 0, 2, 16), (12, 12, 0, 2, 2),                       # <12, 2, false>
    (12, 12, 0, 4, 34), (12, 12, 0, 4, 64), (12, 12, 0, 4, 15),                      # <12, 4, false>
    (12, 12, 0, 8, 34), (12, 12, 0, 8, 16), (12, 12, 0, 8, 400),                     # <12, 8, false>
    (16, 16, 0, 2, 34), (16, 16, 0, 2, 64), (16, 16, 0, 2, 17),                      # <16, 2, false>
    (16, 16, 0, 4, 34), (16, 16, 0, 4, 16), (16, 16, 0, 4, 65),                      # <16, 4, false>
    (16, 16, 0, 8, 34), (16, 16, 0, 8, 64), (16, 16, 0, 8, 2),                       # <16, 8, false>
    (12, 12, 12, 2, 34), (12, 12, 12, 2, 16), (12, 12, 12, 2, 65),                   # <12, 2, true>
    (12, 12, 12, 4, 34), (12, 12, 12, 4, 64), (12, 12, 12, 4, 400),                  # <12, 4, true>
    (12, 12, 8, 8, 34), (12, 12, 8, 8, 16), (12, 12, 8, 8, 17),                      # <12, 8, true>
    (16, 16, 12, 2, 34), (16, 16, 12, 2, 64), (16, 16, 12, 2, 15),                   # <16, 2, true>
    (16, 16, 16, 4, 34), (16, 16, 16, 4, 64), (16, 16, 16, 4, 2),                    # <16, 4, true>
    (16, 16, 12, 8, 34), (16, 16, 12, 8, 16), (16, 16, 12, 8, 400),                  # <16, 8, true>
    (16, 16, 4, 4, 34), (16, 16, 4, 4, 17),                                          # narrow skip
    (12, 8, 0, 4, 34), (12, 8, 0, 4, 65),                                            # res_conv without a skip
]
# one case per instantiation at the reference's RT = 34, for the edge checks
EDGES = [m for m in MATRIX if m[4] == 34 and m[:3] not in ((16, 16, 4), (12, 8, 0))]


def _case(N, C, cinA, cinB, n, rps, B=None):
    B = B or (2 if rps >= 400 else 3)
    wd, x, temb, gy = make_case(C, cinA, cinB, n, B, rps, seed=1000 * C + 100 * cinB + 10 * n + rps)
    blk = Block(N, wd, x, temb, cinA, rps)
    return blk, wd, x, temb, gy


def test_matrix_covers_every_instantiation():
    inst = {(C, n, cinA + cinB != C) for C, cinA, cinB, n, _ in MATRIX}
    assert inst == {(C, n, wr) for C in (12, 16) for n in (2, 4, 8) for wr in (False, True)}
    assert {m[4] for m in MATRIX} == {2, 15, 16, 17, 34, 64, 65, 400}
    assert len(EDGES) == 12 and {(C, n, cinA + cinB != C) for C, cinA, cinB, n, _ in EDGES} == inst


@pytest.mark.parametrize("C,cinA,cinB,n,rps", MATRIX)
def test_rows_backward_vs_float64_oracle(N, forced, C, cinA, cinB, n, rps):
    """forward, d input, every weight gradient and each sample's d(scale, shift) of the forced row form"""
    blk, wd, x, temb, gy = _case(N, C, cinA, cinB, n, rps)
    assert blk.forms()[1] == "rows"
    y, dx_ref, g_ref, dss_ref = reference(wd, x, temb, gy, rps)
    out = blk.forward()
    blk.fill("zero")
    gd, dss = blk.backward(gy)
    e = {"out": err(out, y), "dx": err(blk.dx(), dx_ref), "w": check_grads(gd, g_ref, "grads"), "dss": err(dss, dss_ref)}
    print(f"rows<{C},{n},{cinA + cinB != C}> cin {cinA}+{cinB} rps {rps}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["out"] < OUT_TOL, e
    assert e["dx"] < DX_TOL, e
    assert e["dss"] < DSS_TOL, e
    assert blk.canaries_intact()


@pytest.mark.parametrize("C,cinA,cinB,n,rps", EDGES)
def test_rows_backward_accumulates(N, forced, C, cinA, cinB, n, rps):
    """dA / dB hold earlier gradient: the kernel adds to it (a store would pass on zeroed buffers)"""
    blk, wd, x, temb, gy = _case(N, C, cinA, cinB, n, rps)
    assert blk.forms()[1] == "rows"
    _, dx_ref, g_ref, dss_ref = reference(wd, x, temb, gy, rps)
    blk.forward()
    pre = blk.fill(torch.Generator().manual_seed(rps + n))
    gd, dss = blk.backward(gy)
    e = err(blk.dx(pre), dx_ref)
    print(f"accumulate rows<{C},{n},{cinA + cinB != C}>: dx {e:.2e}")
    assert e < DX_TOL, e
    check_grads(gd, g_ref, "grads")
    assert err(dss, dss_ref) < DSS_TOL


@pytest.mark.parametrize("C,cinA,cinB,n,rps", EDGES)
def test_rows_backward_store_mode_writes_every_element(N, forced, C, cinA, cinB, n, rps):
    """dout == NULL: d out already in the workspace, dA / dB plain stores over NaN -- every element written, and right"""
    blk, wd, x, temb, gy = _case(N, C, cinA, cinB, n, rps)
    assert blk.forms()[1] == "rows"
    _, dx_ref, g_ref, _ = reference(wd, x, temb, gy, rps)
    blk.forward()
    blk.place_dout(gy.cuda())
    blk.fill("nan")
    gd, _ = blk.backward(None)
    dx = blk.dx()
    assert bool(torch.isfinite(dx).all()), int((~torch.isfinite(dx)).sum())
    e = err(dx, dx_ref)
    print(f"store rows<{C},{n},{cinA + cinB != C}>: dx {e:.2e}")
    assert e < DX_TOL, e
    check_grads(gd, g_ref, "grads")


@pytest.mark.parametrize("C,cinA,cinB,n,rps", EDGES)
def test_rows_backward_writes_nothing_past_the_gradient(N, forced, C, cinA, cinB, n, rps):
    """the last sample's ragged tile (2 live rows of 16) and its empty fourth wave: the canaries around dA / dB stay, in both modes"""
    blk, wd, x, temb, gy = _case(N, C, cinA, cinB, n, rps)
    assert blk.forms()[1] == "rows"
    blk.forward()
    blk.fill("zero")
    blk.backward(gy)
    assert blk.canaries_intact()
    blk.place_dout(gy.cuda())
    blk.backward(None)
    assert blk.canaries_intact()


@pytest.mark.parametrize("C,cinA,cinB,n,rps", EDGES)
def test_rows_backward_is_bitwise_repeatable(N, forced, C, cinA, cinB, n, rps):
    """ordered partial sums, no float atomics: two identical calls agree to the bit"""
    blk, wd, x, temb, gy = _case(N, C, cinA, cinB, n, rps)
    assert blk.forms()[1] == "rows"
    blk.forward()
    runs = []
    for _ in range(2):
        blk.fill("zero")
        gd, dss = blk.backward(gy)
        runs.append((blk.dx(), torch.cat([g.reshape(-1) for g in gd.values()]), dss))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_default_rule_edges(N):
    """option at -1: the row form from the device rule's row count on (rounded up to whole RT = 34 samples), the channel-parallel one
    just below; the first against the oracle"""
    assert N.get_option("res_rows_bwd_min_rows") < 0
    thr = N.get_option_effective("res_rows_bwd_min_rows")
    assert thr > 0
    C, cinA, cinB, n, rps = 12, 12, 8, 8, 34
    B_at, B_below = -(-thr // rps), (thr - 1) // rps
    assert N.resblock_forms(cinA, cinB, C, B_below * rps, n, rps)[1] == "cp"
    blk, wd, x, temb, gy = _case(N, C, cinA, cinB, n, rps, B=B_at)
    assert blk.forms()[1] == "rows"
    y, dx_ref, g_ref, dss_ref = reference(wd, x, temb, gy, rps)
    out = blk.forward()
    blk.fill("zero")
    gd, dss = blk.backward(gy)
    e = {"out": err(out, y), "dx": err(blk.dx(), dx_ref), "w": check_grads(gd, g_ref, "grads"), "dss": err(dss, dss_ref)}
    print(f"default rule: {B_at * rps} rows (threshold {thr}): " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["out"] < OUT_TOL and e["dx"] < DX_TOL and e["dss"] < DSS_TOL, e
    assert blk.canaries_intact()


# ---- the one-launch form (k_res_bwd_wg, k_res_wg.hip) at the loop edges of its slot reduce -------------------------------------------------
# k_res_wg_reduce is the ordered slot sum of csrc/dq_slots.h with G = 16 groups, eight loads in flight: the edge counts are 1, G, G + 1,
# 2 G + 1, 7 G, 7 G + 1, 8 G + 1, 9 G + 1, 15 G + 1.  A sample of rows_per_sample = 2 rows of 8 positions is one workgroup (res_wg_grid:
# one 256-position tile per sample), so the weight gradients add up B slots and a sample's d(scale, shift) one; (4, 4, 0, 8, 544, 2) has 17
# workgroups per sample (17 tiles of 256 positions), its d(scale, shift) sums then run over 17 slots and the weights' over 34.
WG_SLOT_EDGES = [(4, 4, 0, 8, 2, B) for B in (1, 16, 17, 33, 112, 113, 129, 145, 241)] + [(4, 4, 0, 8, 544, 2), (8, 8, 4, 8, 2, 113)]


def wg_slots(n, rps, B):
    """(workgroups per sample, slots of a weight gradient): res_wg_grid of k_res_wg.hip"""
    tiles_ps = -(-rps * n // 256)
    tpb = max(1, (tiles_ps * B + 1023) // 1024)
    gx = -(-tiles_ps // tpb)
    return gx, gx * B


@pytest.mark.parametrize("C,cinA,cinB,n,rps,B", WG_SLOT_EDGES)
def test_wg_backward_slot_count_edges(N, C, cinA, cinB, n, rps, B):
    """forward, d input, every weight gradient and each sample's d(scale, shift) of the one-launch form, under the bounds of the row form"""
    assert wg_slots(n, rps, B) == ((17, 34) if rps == 544 else (1, B))
    blk, wd, x, temb, gy = _case(N, C, cinA, cinB, n, rps, B=B)
    assert blk.forms()[1] == "wg"
    y, dx_ref, g_ref, dss_ref = reference(wd, x, temb, gy, rps)
    out = blk.forward()
    blk.fill("zero")
    gd, dss = blk.backward(gy)
    e = {"out": err(out, y), "dx": err(blk.dx(), dx_ref), "w": check_grads(gd, g_ref, "grads"), "dss": err(dss, dss_ref)}
    print(f"wg<{C},{cinA + cinB != C}> cin {cinA}+{cinB} rps {rps} B {B}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["out"] < OUT_TOL, e
    assert e["dx"] < DX_TOL, e
    assert e["dss"] < DSS_TOL, e
    assert blk.canaries_intact()


# (C, cinA, cinB, n, rows per sample) outside res_rows_bwd_usable, and the form each takes instead
FALL_THROUGH = [((16, 20, 0, 4, 34), "plain"),    # cinA over 16
                ((16, 16, 6, 4, 34), "cp"),       # cinB not a multiple of 4
                ((8, 8, 0, 4, 34), "plain"),      # C = 8
                ((12, 12, 0, 16, 34), "plain"),   # rows of 16 positions
                ((12, 12, 0, 4, 1), "plain")]     # one row per sample


@pytest.mark.parametrize("shape,form", FALL_THROUGH)
def test_predicate_fall_through(N, forced, shape, form):
    C, cinA, cinB, n, rps = shape
    assert N.resblock_forms(cinA, cinB, C, 3 * rps, n, rps)[1] == form


def test_fall_through_runs_correctly_with_the_option_forced(N, forced):
    """a shape the row form rejects still computes the block when the option asks for the row form everywhere"""
    C, cinA, cinB, n, rps = 16, 16, 6, 4, 34
    blk, wd, x, temb, gy = _case(N, C, cinA, cinB, n, rps)
    assert blk.forms()[1] == "cp"
    y, dx_ref, g_ref, dss_ref = reference(wd, x, temb, gy, rps)
    out = blk.forward()
    blk.fill("zero")
    gd, dss = blk.backward(gy)
    assert err(out, y) < OUT_TOL and err(blk.dx(), dx_ref) < DX_TOL and err(dss, dss_ref) < DSS_TOL
    check_grads(gd, g_ref, "grads")
    assert blk.canaries_intact()
