"""Residual(PreNorm(LinearAttention)) in every kernel form against a float64 oracle, instantiation by instantiation.

One stand-alone call goes through one of seven kernel families, chosen by row length, row count, two options and pointer alignment
(la_fwd_form in k_linattn.hip, la_bwd_form in k_la_bwd.hip; dq_linattn_forms answers from the same predicates without launching):

  forward   small     k_la_small<C, N>            (12|16, 2|4), (12, 8)       forced by la_small_min_rows = 0
            rows      k_la_rows_fwd<C, N>         (8|12|16, 2|4)              la_small_min_rows = 2^40, la_rows_bwd_min_rows = 0
            register  k_linattn_fwd<C, N, CAN_BF> C in {4..16} x N in {1..64}  both options 2^40
            long      k_linattn_fwd_long<C, N>    fixed (C, 128 | 256), N = 0 (run-time length) x 4 C: rows of 128+ / not 2^k positions
  backward  rows      k_la_rows_bwd<C, N>         (8|12|16, 2|4)
            register  k_linattn_bwd<C, N>, k_linattn_bwd1<C>
            long      k_linattn_bwd_long<C, N>    between two norm-backward launches

Every case first asserts the form the library reports, so a moved threshold or predicate fails here instead of silently testing another
kernel.  Each instantiation runs at row counts at the edges of its own tiling: the 16-row tiles of the rows kernels (1, 15, 16, 17, the
reference's RT = 34, more tiles than one resident round with a ragged tail), the 32-row tiles of k_la_small (4 per workgroup), the units of
32 / N rows of the register kernels (one unit short / over, four units + 1, more units than the backward's resident blocks so that a wave
walks several with a ragged last one) and the 2,048-wave round of the long-row backward.

The forward is checked in y and y_pre (the pre-norm output it saves for the backward).  The backward runs twice per case: accumulating
into a random prefill of dx and of the five parameter gradients (dq_linattn_bwd), then storing dx over NaN (dq_linattn_bwd_store, the mode
the network uses).  Every output is a view inside a larger buffer with canaries on both sides.

Reference: oracle.dq_oracle.linear_attention in float64 with its autograd; errors are max-abs over max |ref|, per tensor, with the
tolerances of tests/test_hip_backward.py::_la_bwd_case."""
import ctypes

import pytest
import torch

Y_TOL = 1e-5
HEAD, TAIL, CANARY = 64, 4096, 7251.0  # floats before / after each output view
BIG = 1 << 40
FORCE = {"small": (0, BIG), "rows": (BIG, 0), "register": (BIG, BIG), "long": (BIG, BIG)}  # (la_small_min_rows, la_rows_bwd_min_rows)
KEYS = ("w_qkv", "w_out", "b_out", "g_pre", "g_out")  # dq_linattn_bwd's parameter order
ORACLE_POSITIONS = 1 << 16  # positions per float64 oracle chunk (memory; parameter gradients add up over the chunks)
LONG_FIXED = ((4, 128), (4, 256), (8, 128), (8, 256), (12, 128), (16, 128))


def grad_tol(rows, wscale):
    return 2e-5 if (rows < 1000 and wscale < 1.0) else 1e-4  # long fp32 sums (fixed order) and sharp softmaxes lose a little


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


@pytest.fixture
def force(N):
    """sets the two options for a form; the default rule again afterwards"""
    def set_form(form):
        small, rows = FORCE[form]
        N.set_option("la_small_min_rows", small)
        N.set_option("la_rows_bwd_min_rows", rows)

    yield set_form
    N.set_option("la_small_min_rows", -1)
    N.set_option("la_rows_bwd_min_rows", -1)


def err(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double().reshape(a.shape)
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def make_case(C, n, rows, wscale):
    gen = torch.Generator().manual_seed(100003 * C + 1009 * n + rows + int(10 * wscale))
    w = {"w_qkv": torch.randn(384, C, generator=gen) * wscale, "w_out": torch.randn(C, 128, generator=gen) * 0.2,
         "b_out": torch.randn(C, generator=gen) * 0.1, "g_pre": torch.rand(C, generator=gen) + 0.5, "g_out": torch.rand(C, generator=gen) + 0.5}
    return torch.randn(rows, C, n, generator=gen), w, torch.randn(rows, C, n, generator=gen)


_ORACLE = {}


def reference(C, n, rows, wscale, grad=True):
    """the case's inputs and the float64 oracle: y, y_pre and (grad) dx and the five parameter gradients (flat, KEYS order).  The last
    result is kept: the forms of one shape follow each other in the matrix."""
    key = (C, n, rows, wscale)
    hit = _ORACLE.get(key)
    if hit is not None and (hit[3]["dx"] is not None or not grad):
        return hit
    from oracle import dq_oracle as O

    x, w, gy = make_case(C, n, rows, wscale)
    shape = {"w_qkv": (384, C, 1), "w_out": (C, 128, 1), "b_out": (C,), "g_pre": (1, C, 1), "g_out": (1, C, 1)}
    name = {"w_qkv": "la.fn.fn.to_qkv.weight", "w_out": "la.fn.fn.to_out.0.weight", "b_out": "la.fn.fn.to_out.0.bias",
            "g_pre": "la.fn.norm.g", "g_out": "la.fn.fn.to_out.1.g"}
    p = {name[k]: w[k].double().reshape(shape[k]).requires_grad_(grad) for k in KEYS}
    ys, pres, dxs = [], [], []
    step = max(1, ORACLE_POSITIONS // n)
    for r0 in range(0, rows, step):
        xc = x[r0:r0 + step].double().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            y, pre = O.linear_attention(p, "la", xc, return_pre=True)
            if grad:
                (y * gy[r0:r0 + step].double()).sum().backward()
                dxs.append(xc.grad)
        ys.append(y.detach())
        pres.append(pre.detach())
    ref = {"y": torch.cat(ys), "y_pre": torch.cat(pres), "dx": torch.cat(dxs) if grad else None}
    for k in KEYS:
        ref[k] = p[name[k]].grad.reshape(-1) if grad else None
    _ORACLE.clear()
    _ORACLE[key] = (x, w, gy, ref)
    return _ORACLE[key]


class LA:
    """one LinearAttention block through the stand-alone calls; every output is a view inside a canary-padded buffer"""

    def __init__(self, N, x, w, gy, x_offset=0, dx_offset=0):
        self.N, self.L = N, N.lib()
        self.rows, self.C, self.n = x.shape
        self.bufs = []
        xb = torch.empty(x.numel() + 4, device="cuda")  # x_offset = 1: not 16-byte aligned
        self.x = xb[x_offset:x_offset + x.numel()].view(x.shape)
        self.x.copy_(x)
        self.gy = gy.cuda()
        self.w = {k: v.cuda() for k, v in w.items()}
        self.y, self.ypre = self._padded(x.numel()).view(x.shape), self._padded(x.numel()).view(x.shape)
        self.dx = self._padded(x.numel(), dx_offset).view(x.shape)
        self.g = {k: self._padded(v.numel()) for k, v in w.items()}
        self.scratch = torch.empty(2 * x.numel() + 2048 * 512 * self.C, device="cuda")
        self.prep = torch.zeros(self.L.dq_linattn_prep_floats(), device="cuda")

    def _padded(self, m, offset=0):
        buf = torch.full((HEAD + m + TAIL,), CANARY, device="cuda")
        view = buf[HEAD + offset:HEAD + offset + m]
        assert (view.data_ptr() % 16 == 0) == (offset % 4 == 0)
        self.bufs.append((buf, offset))
        return view.zero_()

    def canaries_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:HEAD + o] == CANARY).all()) and bool((b[HEAD + o + m:] == CANARY).all())
                   for (b, o), m in zip(self.bufs, [self.x.numel()] * 3 + [t.numel() for t in self.g.values()]))

    def forms(self, prepared=True):
        return self.N.linattn_forms(self.C, self.rows, self.n, prepared)

    def wp(self):
        return [self.N.ptr(self.w[k]) for k in KEYS]

    def forward(self):
        """dq_linattn_fwd_prepared for rows of <= 64 positions (the network's path), dq_linattn_fwd otherwise"""
        N, L, s = self.N, self.L, self.N.stream_ptr()
        wq, wo, bo, gp, go = self.wp()
        if self.n <= 64 and self.n & (self.n - 1) == 0:
            N.check(L.dq_linattn_prepare(wq, wo, gp, self.C, N.ptr(self.prep), s), "dq_linattn_prepare")
            N.check(L.dq_linattn_fwd_prepared(N.ptr(self.x), N.ptr(self.y), N.ptr(self.ypre), wq, wo, bo, gp, go, N.ptr(self.prep),
                                              self.C, self.rows, self.n, s), "dq_linattn_fwd_prepared")
        else:
            N.check(L.dq_linattn_fwd(N.ptr(self.x), N.ptr(self.y), N.ptr(self.ypre), wq, wo, bo, gp, go, self.C, self.rows, self.n, s),
                    "dq_linattn_fwd")
        torch.cuda.synchronize()
        return self.y.clone(), self.ypre.clone()

    def backward(self, store, ypre=None):
        """dq_linattn_bwd (dx +=) or dq_linattn_bwd_store (dx =); the parameter gradients accumulate either way"""
        N = self.N
        fn = self.L.dq_linattn_bwd_store if store else self.L.dq_linattn_bwd
        ypre = self.ypre if ypre is None else ypre
        N.check(fn(N.ptr(self.x), N.ptr(ypre), N.ptr(self.gy), N.ptr(self.dx), *self.wp(), *[N.ptr(self.g[k]) for k in KEYS],
                   N.ptr(self.scratch), self.C, self.rows, self.n, N.stream_ptr()), "dq_linattn_bwd_store" if store else "dq_linattn_bwd")
        torch.cuda.synchronize()
        return self.dx.clone(), {k: v.clone() for k, v in self.g.items()}


def instantiations(form, C, n):
    """the kernels a (form, C, n) case runs: ('fwd' | 'bwd', family, C, N)"""
    if form == "long":
        N_ = n if (C, n) in LONG_FIXED else 0
        return {("fwd", "long", C, N_), ("bwd", "long", C, N_)}
    if form == "small":
        return {("fwd", "small", C, n)}
    if form == "rows":
        return {("fwd", "rows", C, n), ("bwd", "rows", C, n)}
    return {("fwd", "register", C, n), ("bwd", "register1" if n == 1 else "register", C, n)}


CENSUS = ({("fwd", "small", C, n) for C, n in ((12, 2), (16, 2), (12, 4), (16, 4), (12, 8))}
          | {(d, "rows", C, n) for d in ("fwd", "bwd") for C in (8, 12, 16) for n in (2, 4)}
          | {("fwd", "register", C, n) for C in (4, 8, 12, 16) for n in (1, 2, 4, 8, 16, 32, 64)}
          | {("bwd", "register", C, n) for C in (4, 8, 12, 16) for n in (2, 4, 8, 16, 32, 64)}
          | {("bwd", "register1", C, 1) for C in (4, 8, 12, 16)}
          | {(d, "long", C, n) for d in ("fwd", "bwd") for C, n in LONG_FIXED + tuple((C, 0) for C in (4, 8, 12, 16))})


def _register_rows(C, n):
    """one unit (32 / n rows, four per workgroup) short / over, four units + 1, and more units than the backward's resident blocks (at most
    ~2,000 slots), a wave then walking several units with a ragged last one"""
    unit = 32 // n if n < 32 else 1
    big = {1: 40007, 2: 40007, 4: 40007 if C == 8 else 20007, 8: 8011, 16: 4005, 32: 2003, 64: 2003}[n]
    return [unit - 1 if unit > 1 else 1, unit + 1, 4 * unit + 1, big]


def _matrix():
    m = []
    for C in (4, 8, 12, 16):
        for n in (1, 2, 4, 8, 16, 32, 64):
            rows = _register_rows(C, n)
            if (C, n) in {(8, 2), (12, 2), (16, 2), (8, 4), (12, 4), (16, 4)}:
                rows = sorted(set(rows) | {1, 15, 16, 17, 34})  # + the 16-row tiles of the rows kernels (the big count: > 2,048 / 1,024 tiles)
            for r in rows:
                if (C, n) in {(8, 2), (12, 2), (16, 2), (8, 4), (12, 4), (16, 4)} and r in (1, 15, 16, 17, 34, max(rows)):
                    m.append(("rows", C, n, r, 0.4))
                if r in _register_rows(C, n):
                    m.append(("register", C, n, r, 0.4))
    for C, n in ((12, 2), (16, 2), (12, 4), (16, 4), (12, 8)):  # 32-row tiles, 4 per workgroup: a tile +- 1, a workgroup + 1, 33 workgroups
        for r in (31, 33, 129, 4111):
            m.append(("small", C, n, r, 0.4))
    m.append(("small", 16, 2, 266257, 0.4))  # 8,321 tiles: more than 8 workgroups per CU of 256 hold, ragged last tile
    for C, n in LONG_FIXED:
        for r in (1, 5, 2049):  # 2,049 rows: two rows per wave in launch_linattn_bwd_long, the last wave with one
            m.append(("long", C, n, r, 0.4))
    for C, ns in ((4, (1000, 320)), (8, (625, 96)), (12, (320, 1000)), (16, (96, 625))):  # run-time lengths (N = 0)
        m += [("long", C, ns[0], 1, 0.4), ("long", C, ns[1], 5, 0.4), ("long", C, 96, 2049, 0.4)]
    # logits beyond the bounded-softmax criterion of k_linattn_prepare: the shifted-softmax variant of each kernel
    m += [("small", 12, 4, 129, 3.0), ("small", 16, 2, 33, 3.0), ("rows", 16, 2, 34, 3.0), ("rows", 8, 4, 17, 3.0),
          ("register", 12, 4, 33, 3.0), ("register", 8, 16, 9, 3.0), ("register", 4, 1, 33, 3.0), ("long", 8, 128, 5, 3.0),
          ("long", 12, 96, 5, 3.0)]
    return m


MATRIX = _matrix()


def test_matrix_covers_every_instantiation():
    seen = {}
    for form, C, n, rows, _ in MATRIX:
        for inst in instantiations(form, C, n):
            seen.setdefault(inst, set()).add(rows)
    assert set(seen) == CENSUS, set(seen) ^ CENSUS
    assert all(len(r) >= 3 for r in seen.values()), {k: v for k, v in seen.items() if len(v) < 3}
    assert {form for form, *_, ws in MATRIX if ws >= 3.0} == set(FORCE)
    assert {n for form, C, n, *_ in MATRIX if form == "long" and (C, n) not in LONG_FIXED} >= {96, 320, 625, 1000}
    assert len(MATRIX) == len(set(MATRIX))


def _check_forward(la, ref, e):
    y, ypre = la.forward()
    e["y"], e["y_pre"] = err(y, ref["y"]), err(ypre, ref["y_pre"])
    return y, ypre


def _check_backward(la, ref, e, gen):
    """accumulate over a random prefill (at the scale of each reference tensor), then store over NaN; returns the store-mode dx"""
    pre = {"dx": torch.randn(la.dx.shape, generator=gen) * 0.5 * float(ref["dx"].abs().max())}
    for k in KEYS:
        pre[k] = torch.randn(la.g[k].shape, generator=gen) * 0.5 * float(ref[k].abs().max())
    la.dx.copy_(pre["dx"])
    for k in KEYS:
        la.g[k].copy_(pre[k])
    dx, g = la.backward(store=False)
    e["acc dx"] = err(dx.cpu().double() - pre["dx"].double(), ref["dx"])
    e["acc dW"] = max(err(g[k].cpu().double() - pre[k].double(), ref[k]) for k in KEYS)
    la.dx.fill_(float("nan"))
    for k in KEYS:
        la.g[k].zero_()
    dx, g = la.backward(store=True)
    assert bool(torch.isfinite(dx).all()), int((~torch.isfinite(dx)).sum())
    e["store dx"] = err(dx, ref["dx"])
    e["store dW"] = max(err(g[k], ref[k]) for k in KEYS)
    return dx


# Slot counts at the loop edges of the ordered slot sum (csrc/dq_slots.h; for G groups: 1, G, G + 1, 2 G + 1, 7 G, 7 G + 1, 8 G + 1,
# 9 G + 1, 15 G + 1).
#   k_linattn_dw_reduce_multi (G = 8): the register form at n = 32 takes one unit per row and leaves one slot per unit while the units fit
#     one resident round (linattn_bwd_n in k_la_bwd.hip: at least 256 workgroups), so slots = rows.
#   k_linattn_dw_reduce (G = 16): the long-row form.  launch_linattn_bwd_long (k_la_long.hip) gives a wave ceil(rows / 2048) rows and leaves
#     a slot per wave: waves = ceil(rows / ceil(rows / 2048)) = rows up to 2,048 rows; the counts 1, 17, 113, 129 are the row counts.
SLOT_EDGES = ([("register", 4, 32, r, 0.4) for r in (1, 8, 9, 17, 56, 57, 65, 73, 121)] + [("register", 16, 32, r, 0.4) for r in (57, 121)]
              + [("long", 4, 128, r, 0.4) for r in (1, 17, 113, 129)])


@pytest.mark.gpu
@pytest.mark.parametrize("form,C,n,rows,wscale", MATRIX + [m for m in SLOT_EDGES if m not in MATRIX])
def test_form_vs_float64_oracle(N, force, form, C, n, rows, wscale):
    """MATRIX, and SLOT_EDGES: the slot count of the reduce behind the backward at each loop edge of the ordered slot sum.  The long-row
    form leaves one slot per wave, and launch_linattn_bwd_long's rule is waves = ceil(rows / ceil(rows / 2048)): up to 2,048 rows that is
    the row count, so rows 1, 17, 113, 129 are 1, G + 1, 7 G + 1, 8 G + 1 slots at G = 16."""
    force(form)
    prepared = form != "long"
    fwd_form, bwd_form = N.linattn_forms(C, rows, n, prepared)
    assert fwd_form == form, (fwd_form, bwd_form)
    if form != "small":
        assert bwd_form == form, (fwd_form, bwd_form)
    x, w, gy, ref = reference(C, n, rows, wscale, grad=form != "small")
    la = LA(N, x, w, gy)
    e = {}
    _check_forward(la, ref, e)
    if form != "small":
        _check_backward(la, ref, e, torch.Generator().manual_seed(rows))
    inst = ", ".join(f"{d} {fam}<{C},{N_}>" for d, fam, _, N_ in sorted(instantiations(form, C, n)))
    print(f"{form:8s} C {C:2d} n {n:4d} rows {rows:6d} wscale {wscale}: forms ({fwd_form}, {bwd_form}) [{inst}] "
          + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["y"] < Y_TOL and e["y_pre"] < Y_TOL, e
    tol = grad_tol(rows, wscale)
    assert all(v < tol for k, v in e.items() if k not in ("y", "y_pre")), (tol, e)
    assert la.canaries_intact()


# (form, C, n, rows): several resident rounds of the backward's workgroups / waves
ROUNDS = [("rows", 16, 4, 40007), ("rows", 8, 2, 40007), ("register", 12, 2, 40007), ("register", 4, 64, 4003), ("long", 8, 128, 6001)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,C,n,rows", ROUNDS)
def test_backward_is_bitwise_repeatable(N, force, form, C, n, rows):
    """ordered partial sums, no float atomics: two identical calls agree to the bit (the forward too)"""
    force(form)
    assert N.linattn_forms(C, rows, n, form != "long") == (form, form)
    x, w, gy = make_case(C, n, rows, 0.4)
    la = LA(N, x, w, gy)
    runs = []
    for _ in range(2):
        y, ypre = la.forward()
        la.dx.zero_()
        for t in la.g.values():
            t.zero_()
        dx, g = la.backward(store=False)
        runs.append([y, ypre, dx] + [g[k] for k in KEYS])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert la.canaries_intact()


# (form, C, n, rows of the large call): rows [a, b) of it against the same rows run alone, one slice in the middle, one holding the ragged tail
INDEPENDENT = [("small", 12, 4, 204817), ("rows", 16, 4, 20007), ("rows", 12, 2, 40007), ("register", 12, 2, 40007),
               ("register", 8, 8, 8011), ("long", 8, 128, 6001)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,C,n,rows", INDEPENDENT)
def test_rows_are_independent(N, force, form, C, n, rows):
    """a row's y, y_pre and dx do not depend on the rows around it, nor on the tile / unit / resident round it falls in.  The register-resident
    backward (k_linattn_bwd, rows of < 32 positions) forms a unit's products on the matrix pipe with the unit's rows side by side, so a row's
    dx can differ in the last bit when it sits at another place inside its unit; its slices start on a unit boundary."""
    force(form)
    prepared = form != "long"
    x, w, gy = make_case(C, n, rows, 0.4)
    big = LA(N, x, w, gy)
    assert big.forms(prepared)[0] == form
    y, ypre = big.forward()
    dx = None
    if form != "small":
        assert big.forms(prepared)[1] == form
        big.dx.zero_()
        dx, _ = big.backward(store=False)
    slices = ((rows // 2 + 5, rows // 2 + 42), (rows - 61, rows))
    if form == "register":  # (a row keeps its place inside its unit of 32 / n rows: see below)
        slices = tuple((a // 32 * 32, b) for a, b in slices)
    for a, b in slices:
        alone = LA(N, x[a:b], w, gy[a:b])
        assert alone.forms(prepared)[0] == form
        ya, ypa = alone.forward()
        assert torch.equal(ya, y[a:b]) and torch.equal(ypa, ypre[a:b]), (a, b)
        if dx is not None:
            alone.dx.zero_()
            dxa, _ = alone.backward(store=False, ypre=ypre[a:b])
            assert torch.equal(dxa, dx[a:b]), (a, b, float((dxa - dx[a:b]).abs().max()))
        assert alone.canaries_intact()
    assert big.canaries_intact()


@pytest.mark.gpu
def test_default_rule_edges(N):
    """options at -1: k_la_small from the device rule's row count T on, k_la_rows_fwd at T - 1; the case at T against the oracle"""
    assert N.get_option("la_small_min_rows") < 0 and N.get_option("la_rows_bwd_min_rows") < 0
    T = N.get_option_effective("la_small_min_rows")
    assert T > 1
    C, n = 12, 4
    assert N.linattn_forms(C, T - 1, n) == ("rows", "rows")
    assert N.linattn_forms(C, T, n) == ("small", "rows")
    x, w, gy, ref = reference(C, n, T, 0.4)
    la = LA(N, x, w, gy)
    e = {}
    _check_forward(la, ref, e)
    _check_backward(la, ref, e, torch.Generator().manual_seed(T))
    print(f"default rule: C {C} n {n} rows {T} (threshold): forms {la.forms()} " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["y"] < Y_TOL and e["y_pre"] < Y_TOL, e
    assert all(v < grad_tol(T, 0.4) for k, v in e.items() if k not in ("y", "y_pre")), e
    assert la.canaries_intact()


@pytest.mark.gpu
@pytest.mark.parametrize("form,C,n,rows", [("small", 12, 4, 129), ("small", 16, 2, 33), ("rows", 16, 4, 34), ("rows", 8, 2, 17)])
def test_alignment_fall_through(N, force, form, C, n, rows):
    """x (forward) or dx (backward) one float off 16-byte alignment with the small / rows form forced: the call takes the register form
    (bit for bit what the register form computes on aligned tensors) and matches the oracle"""
    x, w, gy, ref = reference(C, n, rows, 0.4)
    force("register")
    aligned = LA(N, x, w, gy)
    assert aligned.forms() == ("register", "register")
    y_reg, ypre_reg = aligned.forward()
    aligned.dx.zero_()
    dx_reg, g_reg = aligned.backward(store=False)
    force(form)
    assert N.linattn_forms(C, rows, n)[0] == form  # (what aligned tensors would take)
    la = LA(N, x, w, gy, x_offset=1)
    assert la.x.data_ptr() % 16 != 0
    y, ypre = la.forward()
    assert torch.equal(y, y_reg) and torch.equal(ypre, ypre_reg)
    e = {"y": err(y, ref["y"]), "y_pre": err(ypre, ref["y_pre"])}
    if form == "rows":
        assert N.linattn_forms(C, rows, n)[1] == "rows"
        lb = LA(N, x, w, gy, dx_offset=1)
        assert lb.dx.data_ptr() % 16 != 0
        lb.forward()
        lb.dx.zero_()
        dx, g = lb.backward(store=False, ypre=ypre_reg)
        assert torch.equal(dx, dx_reg) and all(torch.equal(g[k], g_reg[k]) for k in KEYS)
        e["dx"] = err(dx, ref["dx"])
        e["dW"] = max(err(g[k], ref[k]) for k in KEYS)
        assert lb.canaries_intact()
    print(f"unaligned, {form} forced: C {C} n {n} rows {rows}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["y"] < Y_TOL and e["y_pre"] < Y_TOL, e
    assert all(v < grad_tol(rows, 0.4) for k, v in e.items() if k not in ("y", "y_pre")), e
    assert la.canaries_intact()


# ---- the query alone (no GPU: explicit option values never ask the device) ----------------------------------------------------------

def test_forms_query(N, force):
    force("small")
    assert N.linattn_forms(16, 31, 2) == ("small", "register")
    assert N.linattn_forms(12, 1, 8) == ("small", "register")
    assert N.linattn_forms(16, 100, 4, prepared=False) == ("register", "register")  # dq_linattn_fwd: no prepared weights
    force("rows")
    assert N.linattn_forms(8, 1, 2) == ("rows", "rows")
    assert N.linattn_forms(12, 20001, 4) == ("rows", "rows")
    assert N.linattn_forms(12, 33, 8) == ("register", "register")
    assert N.linattn_forms(16, 0, 2) == ("rows", "rows")
    force("register")
    assert N.linattn_forms(16, 204817, 2) == ("register", "register")
    assert N.linattn_forms(4, 5, 64) == ("register", "register")
    for C, n in ((4, 128), (8, 256), (16, 96), (12, 3), (4, 1000)):
        assert N.linattn_forms(C, 7, n, prepared=False) == ("long", "long")
    N.set_option("la_small_min_rows", 1000)
    N.set_option("la_rows_bwd_min_rows", 100)
    assert N.linattn_forms(12, 1000, 4) == ("small", "rows")
    assert N.linattn_forms(12, 999, 4) == ("rows", "rows")
    assert N.linattn_forms(12, 99, 4) == ("register", "register")
    with pytest.raises(RuntimeError):
        N.linattn_forms(16, 5, 128)  # dq_linattn_fwd_prepared takes rows of <= 64 positions only
    with pytest.raises(RuntimeError):
        N.linattn_forms(6, 5, 2)


@pytest.mark.parametrize("C,n,form,fwd,bwd", [(4, 2, "rows", "register", "register"), (8, 8, "small", "register", "register"),
                                              (8, 8, "rows", "register", "register"), (4, 4, "small", "register", "register"),
                                              (8, 2, "small", "register", "register")])
def test_shape_fall_through(N, force, C, n, form, fwd, bwd):
    """shapes a form has no instantiation for take the register form even with that form forced"""
    force(form)
    assert N.linattn_forms(C, 34, n) == (fwd, bwd)


def test_backward_of_4_gb_takes_the_register_form(N, force):
    """k_la_rows_bwd addresses with 32-bit byte offsets: a tensor of 4 GB or more goes to the register-resident kernel"""
    force("rows")
    assert N.linattn_forms(16, (1 << 25) - 1, 2) == ("rows", "rows")
    assert N.linattn_forms(16, 1 << 25, 2) == ("rows", "register")


def test_unaligned_prepared_weights_fail_on_the_host(N):
    """dq_linattn_fwd_prepared rejects a prepared-weights pointer off 16-byte alignment before any launch (the stand-in pointers are never
    dereferenced)"""
    L = N.lib()
    base = 1 << 20
    p = [ctypes.c_void_p(base)] * 8
    rc = L.dq_linattn_fwd_prepared(*p, ctypes.c_void_p(base + 4), 12, 34, 4, None)
    assert rc != 0
    assert b"prepared weights" in L.dq_last_error()
