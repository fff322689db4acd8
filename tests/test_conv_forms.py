"""The convolution backward (dq_conv_bwd: k_conv_bwd_wg<C, PRE, CP>, k_conv_bwd_data<4, K, MODE>, k_conv_wgrad<4, 4, K, MODE>,
k_conv_wgrad_v4<4, 4, K> + k_wgrad_reduce, and the batched-GEMM data route) against float64 autograd, form by form.

dq_conv_bwd dispatches through the network's own rule, so every case first asserts the kernels dq_conv_bwd_forms reports: a moved
threshold or predicate fails here instead of silently testing another kernel.  The gradient views (dxA, dxB, [dW | dbias]) sit in
canary-padded buffers.  [dW | dbias] is always accumulated onto a prefill; dx is stored or accumulated (the case says which).

Reference: float64 autograd of F.conv1d (stride 1 'same'), F.conv1d(stride 2, pad 1) (down) and F.interpolate(x2, nearest) + F.conv1d(pad 1)
(up), checked once against the oracle's own resample convs and against dq_conv_fwd.  Each case runs with two kinds of input:

 (a) exact: every tensor, prefills included, from {-1, 0, 1}; sum |terms| of every output element is asserted below 2^24 on the float64
     reference, so every fp32 partial sum in any order is an integer below 2^24, hence exact, and the kernel must EQUAL the reference.
     This is the check that sees a dropped, doubled or misplaced item.
 (b) standard normal (weights x 0.3): |got - ref| <= D * 2^-24 * sum |terms| per element, sum |terms| from the float64 reference run on
     the absolute values, D = the longest chain of dependent fp32 additions an element passes through in its kernel, counted from the
     source (an fma counts as one addition; the products of an fma / MFMA are not rounded):

     data gradient
       plain (k_conv_bwd_data)  cout * NT fmas into acc (NT = K taps at stride 1, 2 down, 6 up) + the add onto the old value
                                                                                                   D = cout * NT + 1
       gemm  (k_gemm, unsplit because batch = rows > 1)  cout MFMA steps into the accumulator + the add onto C
                                                                                                   D = cout + 1
       wg    (k_conv_bwd_wg)    C MFMAs (one product each) into every accumulator; down: (e0 + e1) and the old value; stride 1: the three
                                tap accumulators (2 adds) and the old value; up: one more for the lane pair
                                                                                                   D = C + 2 | C + 3 | C + 4
     weight / bias gradient: the slots of gx (wg: gx * B) blocks go through the ordered reduce (k_wgrad_reduce, k_res_wg_reduce): thread
     (element, g) adds slots g, g + 16, ... alternately into two sums (ceil(ceil(slots / 16) / 2) adds), s0 + s1, 16 adds over g, the +=
                                                                                                   R(slots) = ceil(ceil(slots / 16) / 2) + 18
       scalar (k_conv_wgrad)    one fma per item of the grid-stride loop, wave_sum (4 DPP steps + 2), the four waves (2)
                                                                                                   D = items + 8 + R(gx)
       v4     (k_conv_wgrad_v4) four fmas per item (bias: 2 adds inside the item + 1)                D = 4 * items4 + 8 + R(gx)
       wg     (k_conv_bwd_wg)   16 MFMA steps per tile, tpb tiles per workgroup, blocks_sum (4)      D = 16 * tpb + 4 + R(gx * B)

     Observed worst error / bound per form (MI355X, the normal-input runs of every case below): RATIOS_OBSERVED.  The data gradient's
     largest ratios come from short chains (4 output channels, D = 5 .. 6, over 2 to 8 million elements: one rounding is a large share of the bound); the long
     chains stay far below, rounding errors adding like a random walk.  A margin above 1.0 is not allowed -- the bound is a derivation.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

S1, DOWN, UP = 0, 1, 2
HEAD, TAIL, CANARY = 64, 4096, 7251.0  # floats before / after each gradient view
U = 2.0 ** -24
# worst observed error / bound, by (data form | weight-gradient form), over the normal-input runs of every matrix case (a record, not a bound)
RATIOS_OBSERVED = {"data wg": 0.51, "data gemm": 0.26, "data plain": 0.64, "wgrad wg": 0.022, "wgrad v4": 0.064, "wgrad scalar": 0.071}


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


def cdiv(a, b):
    return -(-a // b)


class Case:
    """(cout, cinA, cinB, K, mode, B, rps, n_in) + has_bias, accumulate, which dx is left out, whether w is 16-byte aligned"""

    def __init__(self, cout, cinA, cinB, K, mode, B, rps, n_in, bias=True, acc=False, null=None, w_aligned=True):
        self.cout, self.cinA, self.cinB, self.K, self.mode, self.B, self.rps, self.n_in = cout, cinA, cinB, K, mode, B, rps, n_in
        self.bias, self.acc, self.null, self.w_aligned = bias, acc, null, w_aligned
        self.cin, self.rows = cinA + cinB, B * rps
        self.n_out = n_in // 2 if mode == DOWN else (2 * n_in if mode == UP else n_in)

    def __repr__(self):
        return (f"{('s1', 'down', 'up')[self.mode]}k{self.K} {self.cinA}+{self.cinB}->{self.cout} B{self.B} rps{self.rps} n{self.n_in}->{self.n_out}"
                f"{'' if self.bias else ' nobias'}{' acc' if self.acc else ''}{' no-dx' + self.null if self.null else ''}{'' if self.w_aligned else ' w+1'}")

    def args(self):
        return (self.cout, self.cinA, self.cinB, self.K, self.mode, self.rows, self.n_in, self.n_out, self.rps)

    def with_(self, **kw):
        c = Case(self.cout, self.cinA, self.cinB, self.K, self.mode, self.B, self.rps, self.n_in, self.bias, self.acc, self.null, self.w_aligned)
        for k, v in kw.items():
            setattr(c, k, v)
        c.rows = c.B * c.rps
        return c

    # ---- the chain lengths D of the module docstring, with the launchers' grid arithmetic (k_conv.hip, k_conv_wg.hip)
    def depth(self, data_form, wgrad_form):
        R = lambda slots: cdiv(cdiv(slots, 16), 2) + 18
        total = self.rows * self.n_out
        if data_form == "wg":
            tiles_ps = cdiv(self.rps * self.n_out, 256)
            tpb = max(1, (tiles_ps * self.B + 511) // 512)
            gx = cdiv(tiles_ps, tpb)
            return self.cout + {DOWN: 2, S1: 3, UP: 4}[self.mode], 16 * tpb + 4 + R(gx * self.B)
        d_data = self.cout + 1 if data_form == "gemm" else self.cout * {S1: self.K, DOWN: 2, UP: 6}[self.mode] + 1
        tiles = cdiv(self.cout, 4) * cdiv(self.cin, 4)
        v4 = wgrad_form == "v4"
        gx = max(1, min(cdiv(total, 256 * (8 if v4 else 4)), 512, max(1, 2048 // tiles)))
        items = cdiv(total // 4 if v4 else total, gx * 256)
        return d_data, (4 if v4 else 1) * items + 8 + R(gx)


def ref_forward(x, w, b, mode):
    if mode == S1:
        return F.conv1d(x, w, b, padding=(w.shape[2] - 1) // 2)
    if mode == DOWN:
        return F.conv1d(x, w, b, stride=2, padding=1)
    return F.conv1d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)


def ref_backward(x, w, gy, mode):
    """float64 autograd: (dx, [dW | dbias] flat)"""
    x, w = x.double().requires_grad_(), w.double().requires_grad_()
    b = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    (ref_forward(x, w, b, mode) * gy.double()).sum().backward()
    return x.grad, torch.cat([w.grad.reshape(-1), b.grad])


def draw(c, kind, seed):
    """x, w, gy and the prefills of dx and [dW | dbias]: 'exact' from {-1, 0, 1}, 'normal' standard normal with the weights x 0.3"""
    gen = torch.Generator().manual_seed(seed)
    if kind == "exact":
        r = lambda *s: torch.randint(-1, 2, s, generator=gen).float()
        ws = 1.0
    else:
        r = lambda *s: torch.randn(*s, generator=gen)
        ws = 0.3
    return (r(c.rows, c.cin, c.n_in), r(c.cout, c.cin, c.K) * ws, r(c.rows, c.cout, c.n_out), r(c.rows, c.cin, c.n_in),
            r(c.cout * c.cin * c.K + c.cout))


_REF = {}


def reference(c, kind, seed):
    """the float64 gradients and sum |terms| of every element (without the prefills), computed once per (case shape, kind, seed)"""
    key = (c.args(), kind, seed)
    if key not in _REF:
        if len(_REF) > 8:
            _REF.clear()
        x, w, gy, pre_x, pre_p = draw(c, kind, seed)
        dx, dp = ref_backward(x, w, gy, c.mode)
        ax, ap = ref_backward(x.abs(), w.abs(), gy.abs(), c.mode)
        _REF[key] = (x, w, gy, pre_x, pre_p, dx, dp, ax, ap)
    return _REF[key]


class Conv:
    """one conv backward through dq_conv_bwd; the gradients are views into canary-padded buffers"""

    def __init__(self, N, c, x, w, gy):
        self.N, self.L, self.c = N, N.lib(), c
        self.xA = x[:, :c.cinA].contiguous().cuda()
        self.xB = x[:, c.cinA:].contiguous().cuda() if c.cinB else None
        wbuf = torch.zeros(w.numel() + 8, device="cuda")
        off = 4 if c.w_aligned else 5  # (torch allocations are 16-byte aligned and more)
        self.w = wbuf[off:off + w.numel()]
        self.w.copy_(w.reshape(-1))
        assert (self.w.data_ptr() % 16 == 0) == c.w_aligned
        self.gy = gy.contiguous().cuda()
        self.np = c.cout * c.cin * c.K + (c.cout if c.bias else 0)
        self.bufs = []
        self.dA = None if c.null == "A" else self._padded(c.rows * c.cinA * c.n_in)
        self.dB = None if c.null == "B" or not c.cinB else self._padded(c.rows * c.cinB * c.n_in)
        self.dp = self._padded(self.np)
        self.nws = self.L.dq_conv_bwd_workspace_floats(*c.args())
        assert self.nws > 0
        self.ws = torch.full((self.nws + TAIL,), CANARY, device="cuda")
        self.bufs.append(self.ws)

    def _padded(self, m):
        buf = torch.full((HEAD + m + TAIL,), CANARY, device="cuda")
        view = buf[HEAD:HEAD + m]
        assert view.data_ptr() % 16 == 0
        self.bufs.append(buf)
        return view

    def canaries_intact(self):
        torch.cuda.synchronize()
        ok = all(bool((b[-TAIL:] == CANARY).all()) for b in self.bufs)
        return ok and all(bool((b[:HEAD] == CANARY).all()) for b in self.bufs[:-1])

    def forms(self):
        c = self.c
        return self.N.conv_bwd_forms(*c.args(), has_bias=c.bias, w_aligned=c.w_aligned)

    def fill(self, pre_x, pre_p):
        """prefill of the gradient views from the (rows, cin, n_in) / flat tensors (a float: that value everywhere)"""
        c = self.c
        for d, lo, hi in ((self.dA, 0, c.cinA), (self.dB, c.cinA, c.cin)):
            if d is not None:
                d.copy_(pre_x[:, lo:hi].reshape(-1)) if torch.is_tensor(pre_x) else d.fill_(pre_x)
        self.dp.copy_(self.flat_params(pre_p)) if torch.is_tensor(pre_p) else self.dp.fill_(pre_p)

    def flat_params(self, p):
        """[dW | dbias] of the reference layout cut to this case (no bias: the weight part)"""
        return p[:self.np]

    def run(self, accumulate=None):
        c, P = self.c, self.N.ptr
        acc = c.acc if accumulate is None else accumulate
        self.N.check(self.L.dq_conv_bwd(P(self.xA), c.cinA, P(self.xB), c.cinB, P(self.w), P(self.gy), P(self.dA), P(self.dB), P(self.dp),
                                        int(c.bias), c.cout, c.K, c.mode, c.rows, c.n_in, c.n_out, c.rps, int(acc), P(self.ws), self.nws,
                                        self.N.stream_ptr()), "dq_conv_bwd")
        torch.cuda.synchronize()

    def dx(self):
        """the written parts of d cat(xA, xB) as (rows, channels, n_in) on the host, and their channel index in the concat input"""
        c, parts, idx = self.c, [], []
        for d, lo, hi in ((self.dA, 0, c.cinA), (self.dB, c.cinA, c.cin)):
            if d is not None:
                parts.append(d.cpu().reshape(c.rows, hi - lo, c.n_in))
                idx += list(range(lo, hi))
        return (torch.cat(parts, dim=1) if parts else torch.zeros(c.rows, 0, c.n_in)), idx


def run_and_compare(N, c, kind, expect, seed=0):
    """one launch; exact: equality with the float64 reference, normal: the derived bound.  Returns the worst error / bound (data, weights)."""
    x, w, gy, pre_x, pre_p, dx_ref, dp_ref, ax, ap = reference(c, kind, seed)
    cv = Conv(N, c, x, w, gy)
    forms = cv.forms()
    assert forms == expect, (c, forms)
    cv.fill(pre_x if c.acc else float("nan"), pre_p)
    cv.run()
    assert cv.canaries_intact(), c
    dx, idx = cv.dx()
    dp = cv.dp.cpu()
    want_x = dx_ref[:, idx] + (pre_x[:, idx].double() if c.acc else 0.0)
    sum_x = ax[:, idx] + (pre_x[:, idx].abs().double() if c.acc else 0.0)
    want_p = cv.flat_params(dp_ref + pre_p.double())
    sum_p = cv.flat_params(ap + pre_p.abs().double())
    if kind == "exact":
        assert float(sum_x.max() if sum_x.numel() else 0) < 2 ** 24 and float(sum_p.max()) < 2 ** 24, (c, float(sum_p.max()))
        bad_x, bad_p = int((dx.double() != want_x).sum()), int((dp.double() != want_p).sum())
        print(f"{c}: {forms} exact, sum |terms| <= {float(sum_p.max()):.0f}; wrong elements dx {bad_x} dparams {bad_p}")
        assert torch.equal(dx.double(), want_x), (c, "dx", bad_x)
        assert torch.equal(dp.double(), want_p), (c, "dparams", bad_p, (dp.double() - want_p).abs().max())
        return 0.0, 0.0
    d_data, d_w = c.depth(*forms)
    rx = float(((dx.double() - want_x).abs() / (d_data * U * sum_x).clamp_min(1e-300)).max()) if dx.numel() else 0.0
    rp = float(((dp.double() - want_p).abs() / (d_w * U * sum_p).clamp_min(1e-300)).max())
    print(f"{c}: {forms} D {d_data} / {d_w}; worst error / bound: RATIO data_{forms[0]} {rx:.4f} wgrad_{forms[1]} {rp:.4f}")
    assert rx <= 1.0, (c, "dx", rx)
    assert rp <= 1.0, (c, "dparams", rp)
    return rx, rp


# ---------------------------------------------------------------------------------------------------------------------------------
# A. k_conv_bwd_wg<C, PRE, CP>: all 21 instantiations, two cases each.  n (the conv's OUTPUT row length) cycles through 1 .. 64 (up: 2 .. 64)
# and rows_per_sample * n through: below a tile, exactly one 256-position tile, a tile + one row, RT = 34, RT = 400.
# ---------------------------------------------------------------------------------------------------------------------------------
WG_INST = {DOWN: [(4, 4), (8, 4), (8, 8), (12, 8), (12, 12), (16, 12), (16, 16)],
           UP: [(4, 4), (4, 8), (8, 8), (8, 12), (12, 12), (12, 16), (16, 16)],
           S1: [(4, 4), (4, 8), (8, 8), (8, 12), (12, 12), (12, 16), (16, 16)]}
WG_KINDS = ("below", "tile", "tile+row", "rt34", "rt400")


def _wg_rps(kind, n):
    return {"below": max(2, 255 // n - (1 if n > 1 else 0)), "tile": 256 // n, "tile+row": 256 // n + 1, "rt34": 34, "rt400": 400}[kind]


def _wg_case(mode, C, cp, n, kind, B=3, acc=False):
    n_in = 2 * n if mode == DOWN else (n // 2 if mode == UP else n)
    return Case(C, cp, 0, 4 if mode == DOWN else 3, mode, B, _wg_rps(kind, n), n_in, acc=acc)


def _wg_matrix():
    out = []
    for mode in (DOWN, UP, S1):
        ns = [2, 4, 8, 16, 32, 64, 2] if mode == UP else [1, 2, 4, 8, 16, 32, 64]
        for i, (C, cp) in enumerate(WG_INST[mode]):
            out.append(_wg_case(mode, C, cp, ns[i], WG_KINDS[i % 5], acc=bool(i & 1)))
            out.append(_wg_case(mode, C, cp, ns[(i + 3) % 7], WG_KINDS[(i + 2) % 5], acc=not (i & 1)))
    # several tiles per workgroup: tpb = 2 with gx = 50, and 101 tiles (the last workgroup holds one)
    for rps in (400, 404):
        out.append(Case(4, 4, 0, 4, DOWN, 6, rps, 128, acc=rps == 404))
        out.append(Case(4, 8, 0, 3, UP, 6, rps, 32, acc=rps == 400))
    return out


WG_MATRIX = _wg_matrix()

# ---------------------------------------------------------------------------------------------------------------------------------
# B. k_conv_bwd_data<4, K, MODE> (and whichever weight-gradient kernel the shape takes): rows * n_in around a 256-thread block, every
# channel-chunk count, concat splits with one gradient left out, odd row lengths, and the global-weights branch (cout * 4 * K > 4096).
# ---------------------------------------------------------------------------------------------------------------------------------
PLAIN_MATRIX = [
    (Case(3, 1, 0, 1, S1, 3, 85, 1), "scalar"),                             # 255 items
    (Case(5, 2, 0, 1, S1, 1, 128, 2, bias=False, acc=True), "scalar"),      # 256
    (Case(4, 4, 2, 1, S1, 1, 257, 1, null="A"), "scalar"),                  # 257; cin 6 = 4 + 2, dxA left out
    (Case(1028, 6, 0, 1, S1, 3, 2, 5, bias=False, acc=True), "scalar"),     # global weights: 1028 * 4 * 1 = 4112 > 4096
    (Case(2, 16, 0, 3, S1, 1, 85, 3, acc=True), "scalar"),                  # 255; four channel chunks
    (Case(6, 1, 0, 3, S1, 1, 4, 64), "v4"),                                 # 256
    (Case(8, 2, 4, 3, S1, 1, 103, 5, acc=True, null="B"), "scalar"),        # 515; dxB left out
    (Case(344, 4, 0, 3, S1, 3, 2, 5), "scalar"),                            # global weights: 344 * 4 * 3 = 4128 > 4096
    (Case(4, 2, 0, 7, S1, 3, 17, 5, acc=True), "scalar"),                   # 255
    (Case(3, 6, 0, 7, S1, 1, 4, 64, bias=False), "v4"),                     # 256
    (Case(8, 1, 0, 7, S1, 1, 257, 1, acc=True), "scalar"),                  # 257
    (Case(2, 10, 6, 7, S1, 3, 3, 64, null="A"), "v4"),                      # 576; cin 16 = 10 + 6
    (Case(4, 1, 0, 4, DOWN, 1, 128, 2, acc=True), "scalar"),                # 256; 2 -> 1 positions
    (Case(5, 2, 0, 4, DOWN, 1, 4, 64), "scalar"),                           # 256
    (Case(6, 4, 2, 4, DOWN, 1, 43, 6, bias=False, acc=True, null="B"), "scalar"),  # 258
    (Case(4, 16, 0, 4, DOWN, 3, 3, 64, bias=False), "scalar"),              # 576
    (Case(3, 1, 0, 3, UP, 3, 85, 1, acc=True), "scalar"),                   # 255; 1 -> 2 positions
    (Case(4, 2, 0, 3, UP, 1, 256, 1, bias=False), "scalar"),                # 256
    (Case(2, 6, 0, 3, UP, 1, 257, 1, acc=True), "scalar"),                  # 257
    (Case(5, 12, 4, 3, UP, 3, 3, 64, null="A"), "scalar"),                  # 576; 64 -> 128 positions
    (Case(7, 3, 3, 3, UP, 1, 52, 5, acc=True, null="B"), "scalar"),         # 260
]

# ---------------------------------------------------------------------------------------------------------------------------------
# C. the weight gradient: k_conv_wgrad<4, 4, K, MODE> (SCALAR) and k_conv_wgrad_v4<4, 4, K> (V4) + k_wgrad_reduce.  513 rows = three samples
# of 171: more than one block of the grid-stride loop at every n.  The V4 item counts sit at the grid's edges: gx = ceil(positions / 2048)
# blocks of 256 threads x 4 positions, so gx * 2048 positions are exactly two sweeps; the capped grid (gx = 512) takes four sweeps and 2052
# positions more.  (B = 1 where the position count has no factor 3; none of these shapes is a k_conv_bwd_wg one.)
# ---------------------------------------------------------------------------------------------------------------------------------
WGRAD_MATRIX = [
    (Case(1, 1, 0, 1, S1, 3, 171, 1), "scalar"),
    (Case(4, 2, 0, 1, S1, 3, 171, 2, bias=False), "scalar"),
    (Case(6, 4, 2, 1, S1, 3, 171, 5), "scalar"),
    (Case(16, 32, 0, 3, S1, 3, 171, 1, bias=False), "scalar"),
    (Case(4, 1, 1, 3, S1, 3, 171, 2), "scalar"),
    (Case(1, 6, 0, 3, S1, 3, 171, 5), "scalar"),
    (Case(6, 2, 0, 7, S1, 3, 171, 1), "scalar"),
    (Case(16, 1, 0, 7, S1, 3, 171, 2, bias=False), "scalar"),
    (Case(4, 4, 2, 7, S1, 3, 171, 5), "scalar"),
    (Case(6, 20, 12, 4, DOWN, 3, 171, 8), "scalar"),
    (Case(16, 6, 0, 4, DOWN, 3, 171, 2, bias=False), "scalar"),
    (Case(4, 1, 0, 3, UP, 3, 171, 4), "scalar"),
    (Case(1, 16, 16, 3, UP, 3, 171, 1, bias=False), "scalar"),
    (Case(1, 2, 0, 1, S1, 3, 171, 4), "v4"),
    (Case(6, 32, 0, 1, S1, 3, 171, 8, bias=False), "v4"),
    (Case(16, 4, 2, 1, S1, 3, 43, 64), "v4"),
    (Case(4, 6, 0, 3, S1, 3, 171, 4), "v4"),
    (Case(16, 1, 0, 3, S1, 3, 171, 8), "v4"),
    (Case(6, 1, 1, 3, S1, 3, 43, 64, bias=False), "v4"),
    (Case(4, 32, 0, 7, S1, 3, 171, 4, bias=False), "v4"),
    (Case(1, 4, 2, 7, S1, 3, 171, 8), "v4"),
    (Case(6, 2, 0, 7, S1, 3, 43, 64), "v4"),
    (Case(4, 4, 0, 1, S1, 1, 1535, 4), "v4"),       # 3 * 2048 - 4 positions
    (Case(4, 4, 0, 1, S1, 3, 512, 4), "v4"),        # 3 * 2048
    (Case(4, 4, 0, 1, S1, 1, 1537, 4), "v4"),       # 3 * 2048 + 4: a fourth block
    (Case(4, 4, 0, 3, S1, 3, 512, 4, bias=False), "v4"),
    (Case(16, 16, 16, 3, S1, 3, 684, 64), "v4"),    # 32 channel tiles: gx capped at 2048 / 32 = 64 (131,328 positions ask for 65)
]
CAPPED = Case(4, 4, 0, 1, S1, 1, 524801, 4)         # 2 * 512 * 2048 + 2052 positions: gx capped at 512 (WGRAD_MAX_PARTS)

# ---------------------------------------------------------------------------------------------------------------------------------
# C2. the slot count of the weight-gradient reduce at every loop edge of the ordered slot sum (csrc/dq_slots.h; G = 16 groups, two slots
# at a time: 1, G, G + 1, 2 G + 1, and the cap of 512).  K = 1, cout = cin = 4 is one channel tile, so the scalar form at n = 1 leaves
# gx = ceil(rows / 1024) slots: rows = 1024 (slots - 1) + 1.  One v4 case (n = 4: gx = ceil(4 rows / 2048)) at 17 slots.
# ---------------------------------------------------------------------------------------------------------------------------------
SLOT_EDGES = [(Case(4, 4, 0, 1, S1, 1, 1024 * (k - 1) + 1, 1), "scalar", k) for k in (1, 16, 17, 33, 512)] + \
             [(Case(4, 4, 0, 1, S1, 1, 8193, 4), "v4", 17)]


def wgrad_slots(c, wform):
    """gx of launch_conv_wgrad (k_conv.hip: wgrad_parts)"""
    tiles = cdiv(c.cout, 4) * cdiv(c.cin, 4)
    return max(1, min(cdiv(c.rows * c.n_out, 256 * (8 if wform == "v4" else 4)), 512, max(1, 2048 // tiles)))


# ---------------------------------------------------------------------------------------------------------------------------------
# D. the batched-GEMM data route of the bottleneck attention's projections (q | v, k, to_out -- whose bias does not enter the data gradient)
# ---------------------------------------------------------------------------------------------------------------------------------
GEMM_MATRIX = [Case(cout, cin, 0, 1, S1, 3, 1, n, bias=bias, acc=acc)
               for (cout, cin, bias) in ((256, 16, False), (128, 16, False), (16, 128, True)) for n in (12, 400) for acc in (False, True)]

# one case per form for the edge checks: (case, forms)
EDGES = [(_wg_case(DOWN, 8, 4, 16, "rt34"), ("wg", "wg")), (_wg_case(UP, 8, 12, 8, "rt34"), ("wg", "wg")), (_wg_case(S1, 12, 16, 4, "rt34"), ("wg", "wg")),
         (Case(5, 2, 1, 1, S1, 3, 29, 3), ("plain", "scalar")), (Case(3, 4, 2, 3, S1, 3, 11, 8), ("plain", "v4")),
         (Case(2, 1, 0, 7, S1, 3, 7, 64, bias=False), ("plain", "v4")), (Case(6, 5, 0, 4, DOWN, 3, 23, 6), ("plain", "scalar")),
         (Case(4, 3, 3, 3, UP, 3, 19, 5), ("plain", "scalar")), (Case(128, 16, 0, 1, S1, 3, 1, 36, bias=False), ("gemm", "v4"))]


def test_matrix_covers_every_instantiation():
    inst = {(c.cout, c.mode, c.cinA) for c in WG_MATRIX}
    assert inst == {(C, mode, cp) for mode, lst in WG_INST.items() for C, cp in lst} and len(inst) == 21
    for mode in (DOWN, UP, S1):
        assert {c.n_out for c in WG_MATRIX if c.mode == mode} == ({2, 4, 8, 16, 32, 64} if mode == UP else {1, 2, 4, 8, 16, 32, 64})
    per = [(c.rps * c.n_out, c.n_out, c.rps) for c in WG_MATRIX]
    assert any(p < 256 for p, _, _ in per) and any(p == 256 for p, _, _ in per) and any(p == 256 + n for p, n, _ in per)
    assert {34, 400, 404} <= {r for _, _, r in per}
    assert {(c.K, c.mode) for c, _ in PLAIN_MATRIX} == {(1, S1), (3, S1), (7, S1), (4, DOWN), (3, UP)}
    assert {255, 256, 257} <= {c.rows * c.n_in for c, _ in PLAIN_MATRIX} and {1, 2, 6, 16} <= {c.cin for c, _ in PLAIN_MATRIX}
    assert {1, 2, 3, 5, 64} <= {c.n_in for c, _ in PLAIN_MATRIX} and {"A", "B"} <= {c.null for c, _ in PLAIN_MATRIX}
    assert any(c.cout * 4 * c.K > 4096 for c, _ in PLAIN_MATRIX if c.K == 1) and any(c.cout * 4 * c.K > 4096 for c, _ in PLAIN_MATRIX if c.K == 3)
    sc = {(c.K, c.mode, c.n_out) for c, f in WGRAD_MATRIX if f == "scalar"}
    assert {(K, S1, n) for K in (1, 3, 7) for n in (1, 2, 5)} <= sc and {m for _, m, _ in sc} == {S1, DOWN, UP}
    assert {(c.K, c.n_out) for c, f in WGRAD_MATRIX if f == "v4"} >= {(K, n) for K in (1, 3, 7) for n in (4, 8, 64)}
    assert {1, 4, 6, 16} <= {c.cout for c, _ in WGRAD_MATRIX} and {1, 2, 6, 32} <= {c.cin for c, _ in WGRAD_MATRIX}
    assert {True, False} == {c.bias for c, _ in WGRAD_MATRIX} and any(c.cinB for c, _ in WGRAD_MATRIX)
    assert {c.rows * c.n_out for c, _ in WGRAD_MATRIX} >= {6140, 6144, 6148} and CAPPED.rows * CAPPED.n_out == 2 * 512 * 2048 + 2052
    assert {(c.cout, c.cin, c.n_in, c.acc) for c in GEMM_MATRIX} == {(co, ci, n, a) for co, ci in ((256, 16), (128, 16), (16, 128))
                                                                      for n in (12, 400) for a in (False, True)}
    assert {f for _, f in EDGES} == {("wg", "wg"), ("plain", "scalar"), ("plain", "v4"), ("gemm", "v4")}
    assert {(c.K, c.mode) for c, f in EDGES if f[0] == "plain"} == {(1, S1), (3, S1), (7, S1), (4, DOWN), (3, UP)}


def test_reference_forward_is_the_oracles_and_dq_conv_fwd(N, golden):
    """the float64 reference conv of this file against the oracle's own Downsample / k3 / Upsample convs (their inputs and outputs tapped
    from a whole forward pass), and dq_conv_fwd against it"""
    import numpy as np
    from conftest import sub
    from oracle import dq_oracle as O

    g = golden("unet_default_rt16.npz")
    T = lambda a: torch.as_tensor(np.asarray(a))
    p = {k: v.double() for k, v in sub(g, "w/").items()}
    taps = {}
    O.unet_forward(p, O.UNetConfig(downsample_dim=64), T(g["x"]).double(), T(g["t"]), T(g["init_cond"]).double(), T(g["attn_cond"]).double(), taps=taps)
    L = len([k for k in taps if k.startswith("down") and k.endswith(".in")])
    for name, wk, mode in ((("down0", "downs.0.3", DOWN), (f"down{L - 1}", f"downs.{L - 1}.3", S1), ("up0", "ups.0.3.1", UP), (f"up{L - 1}", f"ups.{L - 1}.3", S1))):
        x, w, b = taps[name + ".in"], p[wk + ".weight"], p[wk + ".bias"]
        y = ref_forward(x, w, b, mode)
        assert torch.equal(y, taps[name]), name
        out = torch.empty(y.shape, device="cuda")
        xf, wf, bf = x.float().contiguous(), w.float().contiguous(), b.float()
        xd, wd, bd = xf.cuda(), wf.cuda(), bf.cuda()
        N.check(N.lib().dq_conv_fwd(N.ptr(xd), N.ptr(wd), N.ptr(bd), None, 0, N.ptr(out), w.shape[0], w.shape[1], w.shape[2], mode,
                                    x.shape[0], x.shape[2], y.shape[2], N.stream_ptr()), "dq_conv_fwd")
        # the bias and cin * K fmas in a chain: (cin * K + 1) roundings at the most over sum |terms|
        y32, a32 = ref_forward(xf.double(), wf.double(), bf.double(), mode), ref_forward(xf.double().abs(), wf.double().abs(), bf.double().abs(), mode)
        ratio = float(((out.cpu().double() - y32).abs() / ((w.shape[1] * w.shape[2] + 1) * U * a32)).max())
        assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("c", WG_MATRIX, ids=repr)
def test_conv_bwd_wg(N, c, kind):
    run_and_compare(N, c, kind, ("wg", "wg"))


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("c,wform", PLAIN_MATRIX, ids=lambda v: repr(v) if isinstance(v, Case) else v)
def test_conv_bwd_data_plain(N, c, wform, kind):
    run_and_compare(N, c, kind, ("plain", wform))


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("c,wform", WGRAD_MATRIX, ids=lambda v: repr(v) if isinstance(v, Case) else v)
def test_conv_wgrad(N, c, wform, kind):
    run_and_compare(N, c, kind, ("plain", wform))


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("c,wform,slots", SLOT_EDGES, ids=lambda v: repr(v) if isinstance(v, Case) else str(v))
def test_conv_wgrad_slot_count_edges(N, c, wform, slots, kind):
    """the ordered reduce with 1, 16, 17, 33 and 512 slots (v4: 17): no slot dropped, doubled or read past the last"""
    assert wgrad_slots(c, wform) == slots
    run_and_compare(N, c, kind, ("plain", wform))


@pytest.mark.parametrize("kind", ["exact", "normal"])
def test_conv_wgrad_capped_grid(N, kind):
    """gx = WGRAD_MAX_PARTS: four sweeps of the 512-block grid and 2052 positions; 34 MB per tensor, sum |terms| <= 2.1 M < 2^24"""
    run_and_compare(N, CAPPED, kind, ("plain", "v4"))


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("c", GEMM_MATRIX, ids=repr)
def test_conv_bwd_data_gemm(N, c, kind):
    run_and_compare(N, c, kind, ("gemm", "v4"))


# ---- edge checks, one case per form ------------------------------------------------------------------------------------------------
def _edge(N, c, forms, kind="exact"):
    x, w, gy, pre_x, pre_p = reference(c, kind, 1)[:5]
    cv = Conv(N, c, x, w, gy)
    assert cv.forms() == forms, (c, cv.forms())
    return cv, pre_x, pre_p


@pytest.mark.parametrize("c,forms", EDGES, ids=lambda v: repr(v) if isinstance(v, Case) else None)
def test_accumulate_equals_store_plus_prefill(N, c, forms):
    """exact inputs: every sum is exact, so the accumulating launch must equal the storing one + the prefill, bit for bit"""
    cv, pre_x, pre_p = _edge(N, c, forms)
    cv.fill(float("nan"), 0.0)
    cv.run(accumulate=False)
    stored, idx = cv.dx()
    cv.fill(pre_x, 0.0)
    cv.run(accumulate=True)
    assert torch.equal(cv.dx()[0], stored + pre_x[:, idx])
    assert cv.canaries_intact()


@pytest.mark.parametrize("c,forms", EDGES, ids=lambda v: repr(v) if isinstance(v, Case) else None)
def test_store_overwrites_nan_everywhere(N, c, forms):
    cv, pre_x, pre_p = _edge(N, c, forms, "normal")
    cv.fill(float("nan"), 0.0)
    cv.run(accumulate=False)
    dx, _ = cv.dx()
    assert bool(torch.isfinite(dx).all()), (c, int((~torch.isfinite(dx)).sum()))
    assert bool(torch.isfinite(cv.dp).all())
    assert cv.canaries_intact()


@pytest.mark.parametrize("c,forms", EDGES, ids=lambda v: repr(v) if isinstance(v, Case) else None)
def test_bitwise_repeatable(N, c, forms):
    """ordered partial sums, no float atomics"""
    cv, pre_x, pre_p = _edge(N, c, forms, "normal")
    runs = []
    for _ in range(2):
        cv.fill(pre_x, pre_p)
        cv.run(accumulate=True)
        runs.append((cv.dx()[0], cv.dp.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert cv.canaries_intact()


@pytest.mark.parametrize("c,forms", EDGES, ids=lambda v: repr(v) if isinstance(v, Case) else None)
def test_each_sample_equals_the_sample_alone(N, c, forms):
    """the data gradient of sample b in the batch and of sample b run alone (B = 1) agree bit for bit: no item crosses a sample boundary"""
    cv, pre_x, pre_p = _edge(N, c, forms, "normal")
    x, w, gy = reference(c, "normal", 1)[:3]
    cv.fill(float("nan"), 0.0)
    cv.run(accumulate=False)
    whole, idx = cv.dx()
    one = c.with_(B=1)
    for b in range(c.B):
        sl = slice(b * c.rps, (b + 1) * c.rps)
        cb = Conv(N, one, x[sl], w, gy[sl])
        assert cb.forms()[0] == forms[0], (one, cb.forms())
        cb.fill(float("nan"), 0.0)
        cb.run(accumulate=False)
        assert torch.equal(cb.dx()[0], whole[sl]), (c, b)
        assert cb.canaries_intact()


# ---- shapes k_conv_bwd_wg or the GEMM route reject: the form they take instead, asserted, then run against the reference -------------------
FALL_THROUGH = [
    (Case(8, 8, 0, 3, S1, 6, 1, 8), ("plain", "v4")),                           # one row per sample
    (Case(8, 8, 0, 3, S1, 3, 5, 128), ("plain", "v4")),                         # rows of 128 positions
    (Case(8, 8, 0, 3, UP, 3, 34, 1), ("wg", "wg")),                             # (up to n = 2 is still the one-launch form ...)
    (Case(4, 4, 0, 4, DOWN, 3, 34, 2), ("wg", "wg")),                           # (... and so is down to n = 1)
    (Case(8, 16, 0, 3, S1, 3, 34, 8), ("plain", "v4")),                         # cp outside the built pairs
    (Case(16, 8, 0, 4, DOWN, 3, 34, 16), ("plain", "scalar")),                  # cp outside the built pairs
    (Case(8, 8, 0, 3, S1, 3, 34, 8, bias=False), ("plain", "v4")),              # no bias gradient adjacent to the weight's
    (Case(8, 4, 4, 3, S1, 3, 34, 8), ("plain", "v4")),                          # a concat input
    (Case(128, 16, 0, 1, S1, 3, 1, 12, bias=False, w_aligned=False), ("plain", "v4")),  # a weight one float off 16 bytes: no GEMM
    (Case(128, 16, 0, 1, S1, 3, 1, 10, bias=False), ("plain", "scalar")),       # n not a multiple of 4: no GEMM
]


def test_up_at_one_position_is_rejected(N):
    """an Upsample conv writes n_out = 2 n_in positions, so "up at n = 1" is not a shape: both calls refuse it (k_conv_bwd_wg's own n >= 2
    guard is then never the deciding one; the smallest real shape, 1 -> 2 positions, is in FALL_THROUGH and takes the one-launch form)"""
    assert N.lib().dq_conv_bwd_workspace_floats(8, 8, 0, 3, UP, 102, 1, 1, 34) == -1
    with pytest.raises(RuntimeError, match="n_out = 2 n_in"):
        N.conv_bwd_forms(8, 8, 0, 3, UP, 102, 1, 1, 34)


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("c,forms", FALL_THROUGH, ids=lambda v: repr(v) if isinstance(v, Case) else None)
def test_fall_through(N, c, forms, kind):
    run_and_compare(N, c, kind, forms)
    run_and_compare(N, c.with_(acc=True), kind, forms)
