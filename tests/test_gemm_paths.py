"""The matrix-core GEMM (csrc/k_gemm.hip: k_gemm / k_gemm_s3 at 32, 64 and 128 rows per tile, k_gemm_split_reduce, launch_gemm) against a
float64 product, path by path: every tile form in every layout, the two-launch plans (whole rounds of 256 tiles + a remainder with a
non-zero tile base), the batched operand patterns of the attention and of the wide bottleneck, the reduction over samples of the wide
weight gradient (kbatch), bias_m / add / alpha.  Every case goes through dq_gemm_ex in both precisions.

Path: a case first asserts through dq_debug_gemm_plan (the launcher's own planning function) that it takes the path it is named after,
so a change of the cost model fails here instead of silently testing another kernel.

Reference: the float64 product of the same device tensors (torch), with bias / bias_m / alpha / the old C / `add` applied in float64.
Tolerances are the ones the project states for the two precisions (tests/test_tfm.py), nothing new:
    fp32     |C - ref| <  2e-6 * max|ref| * max(1, sqrt(Kr) / 8)          ref = alpha * A B + bias + bias_m, as the stored result
    bf16x3   |C - ref| <  2e-5 * sqrt(Kr) * max|A| * max|B| * |alpha|
with Kr the whole reduction length (kbatch * K).  A run with accumulate / add keeps the tolerance of its product.  The fp32 result must be
at least as close as the bf16x3 one (up to 1e-6 max|ref|).

Guards: the operands live in buffers filled with NaN wherever the product must not look (rows / columns beyond M, N, K, the pad columns
up to lda / ldb, the P pad of the wide layouts, the other half of a [K | V] tensor, before and behind every buffer, the split scratch and
what lies around it), so one element read past a mask turns a result into NaN.  C is pre-filled with a sentinel; everything outside the
(M x N) window of every batch element must be bit-identical afterwards (ldc pad columns, the gaps between batch elements, the guards).
Every case runs twice and must repeat bit for bit.

Observed worst error / tolerance per group (RATIOS_OBSERVED below): measured on MI355X, 2026-10-18; a record, not a bound.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 7251.0  # floats before / behind every buffer (a multiple of 4: the views stay 16-byte aligned)
PRECISIONS = ("fp32", "bf16x3")
# worst observed |err| / tolerance by case group and precision (MI355X, 2026-10-18), over every case of the group below
RATIOS_OBSERVED = {
    "tile forms": {"fp32": 0.163, "bf16x3": 0.126}, "two-launch plans": {"fp32": 0.196, "bf16x3": 0.202},
    "attention products": {"fp32": 0.131, "bf16x3": 0.093}, "wide_gemm pattern": {"fp32": 0.152, "bf16x3": 0.067},
    "wide_wgrad pattern (k-batched)": {"fp32": 0.068, "bf16x3": 0.090}, "alpha": {"fp32": 0.189, "bf16x3": 0.082},
}


@pytest.fixture(scope="module")
def N():
    from dquartic import _native

    _native.lib()
    return _native


def cdiv(a, b):
    return -(-a // b)


def up4(v):
    return (v + 3) // 4 * 4


class Product:
    """One launch_gemm product over flat, guarded buffers.  Operand z = (zo, zi), k-block b lives at off + zo s?o + zi s?i + b s?k floats."""

    def __init__(self, M, N, K, layout="kk", lda=None, ldb=None, ldc=None, batch=1, inner=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), kbatch=1, sAk=0,
                 sBk=0, offA=0, offB=0, offC=0, nA=None, nB=None, nC=None):
        self.M, self.N, self.K, self.a_k, self.b_k = M, N, K, layout[0] == "k", layout[1] == "k"
        self.lda = lda if lda is not None else up4(K if self.a_k else M) + 4  # at least four pad columns of NaN
        self.ldb = ldb if ldb is not None else up4(K if self.b_k else N) + 4
        self.ldc = ldc if ldc is not None else N + 3  # an odd pitch: C has no alignment contract
        self.batch, self.inner, self.sA, self.sB, self.sC, self.kbatch, self.sAk, self.sBk = batch, inner, sA, sB, sC, kbatch, sAk, sBk
        self.offA, self.offB, self.offC = offA, offB, offC
        zo = batch // inner
        assert zo * inner == batch
        self.zo = zo
        rows_a, rows_b = (M if self.a_k else K), (N if self.b_k else K)
        self.nA = nA if nA is not None else offA + (zo - 1) * sA[0] + (inner - 1) * sA[1] + (kbatch - 1) * sAk + rows_a * self.lda
        self.nB = nB if nB is not None else offB + (zo - 1) * sB[0] + (inner - 1) * sB[1] + (kbatch - 1) * sBk + rows_b * self.ldb
        self.nC = nC if nC is not None else offC + (zo - 1) * sC[0] + (inner - 1) * sC[1] + M * self.ldc
        self.Kr = kbatch * K

    def a_view(self, buf, fill=False):
        """(zo, zi, b, M, K) view of A in the flat buffer; fill: the dimensions of stride 0 (a shared operand) collapsed, for writing."""
        sm, sk = (self.lda, 1) if self.a_k else (1, self.lda)
        return self._view(buf, GUARD + self.offA, (self.zo, self.inner, self.kbatch, self.M, self.K), (self.sA[0], self.sA[1], self.sAk, sm, sk), fill)

    def b_view(self, buf, fill=False):
        """(zo, zi, b, K, N) view of B."""
        sk, sn = (1, self.ldb) if self.b_k else (self.ldb, 1)
        return self._view(buf, GUARD + self.offB, (self.zo, self.inner, self.kbatch, self.K, self.N), (self.sB[0], self.sB[1], self.sBk, sk, sn), fill)

    def c_view(self, buf):
        """(zo, zi, M, N) view of C (or of `add`, laid out like C)."""
        return self._view(buf, GUARD + self.offC, (self.zo, self.inner, self.M, self.N), (self.sC[0], self.sC[1], self.ldc, 1), False)

    @staticmethod
    def _view(buf, off, sizes, strides, fill):
        if fill:
            sizes = tuple(1 if st == 0 and sz > 1 else sz for sz, st in zip(sizes, strides))
        return torch.as_strided(buf, sizes, strides, off)


def nan_buffer(n):
    return torch.full((n + 2 * GUARD,), float("nan"), device="cuda")


def bits(t):
    return t.view(torch.int32)


class Data:
    """Operands of a Product, drawn once (standard normal) and shared by its variants; float64 product computed once."""

    def __init__(self, p, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.p = p
        self.A, self.B = nan_buffer(p.nA), nan_buffer(p.nB)
        for view in (p.a_view(self.A, fill=True), p.b_view(self.B, fill=True)):
            view.copy_(torch.randn(view.shape, device="cuda", generator=g))
        Ad, Bd = p.a_view(self.A).double(), p.b_view(self.B).double()
        assert not torch.isnan(Ad).any() and not torch.isnan(Bd).any()
        self.prod = torch.einsum("oibmk,oibkn->oimn", Ad, Bd)
        self.amax, self.bmax = float(Ad.abs().max()), float(Bd.abs().max())
        # bias (N), bias_m (M), the old C and `add` (like C), each inside NaN
        self.bias, self.bias_m = nan_buffer(p.N), nan_buffer(p.M)
        self.bias[GUARD:GUARD + p.N] = torch.randn(p.N, device="cuda", generator=g)
        self.bias_m[GUARD:GUARD + p.M] = torch.randn(p.M, device="cuda", generator=g)
        self.C0 = torch.full((p.nC + 2 * GUARD,), SENTINEL, device="cuda")
        self.add = nan_buffer(p.nC)
        for buf in (self.C0, self.add):
            v = p.c_view(buf)
            v.copy_(torch.randn(v.shape, device="cuda", generator=g))
        self.Csent = torch.full((p.nC + 2 * GUARD,), SENTINEL, device="cuda")
        self.window = torch.zeros(p.nC + 2 * GUARD, dtype=torch.bool, device="cuda")
        p.c_view(self.window).fill_(True)
        assert int(self.window.sum()) == p.batch * p.M * p.N  # the windows of the batch elements do not overlap


def run_variant(N, d, group, bias=False, bias_m=False, accumulate=False, add=False, alpha=1.0, splits=0, expect=None):
    """Runs the product in both precisions with the given epilogue; asserts the plan (`expect`: a dict of bm / full / ntiles / splits /
    k_per_split, compared with the hook's answer), the tolerances, the guards and the repeatability.  Returns {precision: err / tol}."""
    p = d.p
    plan = N.gemm_plan(p.M, p.N, p.K, p.batch, p.kbatch, splits)
    got_plan = {"bm": plan["bm"], "full": plan["full"]["ntiles"], "ntiles": plan["rest"]["ntiles"], "splits": plan["rest"]["splits"],
                "k_per_split": plan["rest"]["k_per_split"], "kv": plan["kv"]}
    for k, v in (expect or {}).items():
        assert got_plan[k] == v, f"{group}: the launcher no longer takes the path this case is named after: {k} = {got_plan[k]}, expected {v} ({plan})"
    if plan["full"]["ntiles"]:
        assert plan["rest"]["ntiles"] == 0 or plan["rest"]["tile_base"] == plan["full"]["ntiles"]
    ref0 = alpha * d.prod
    if bias:
        ref0 = ref0 + d.bias[GUARD:GUARD + p.N].double()
    if bias_m:
        ref0 = ref0 + d.bias_m[GUARD:GUARD + p.M].double()[:, None]
    ref = ref0
    if accumulate:
        ref = ref + p.c_view(d.C0).double()
    if add:
        ref = ref + p.c_view(d.add).double()
    tol = {"fp32": 2e-6 * float(ref0.abs().max()) * max(1.0, math.sqrt(p.Kr) / 8),
           "bf16x3": 2e-5 * math.sqrt(p.Kr) * d.amax * d.bmax * abs(alpha)}
    Cinit = d.C0 if accumulate else d.Csent
    need = plan["scratch"]
    errs = {}
    for prec in PRECISIONS:
        outs = []
        for _ in range(2):
            C = Cinit.clone()
            scratch = nan_buffer(need)
            desc = N.gemm_desc(
                A=d.A.data_ptr() + 4 * (GUARD + p.offA), B=d.B.data_ptr() + 4 * (GUARD + p.offB), C=C.data_ptr() + 4 * (GUARD + p.offC),
                bias=d.bias.data_ptr() + 4 * GUARD if bias else None, bias_m=d.bias_m.data_ptr() + 4 * GUARD if bias_m else None,
                add=d.add.data_ptr() + 4 * (GUARD + p.offC) if add else None,
                scratch=scratch.data_ptr() + 4 * GUARD if need else None, scratch_floats=need,
                M=p.M, N=p.N, K=p.K, lda=p.lda, ldb=p.ldb, ldc=p.ldc, a_kmajor=int(p.a_k), b_kmajor=int(p.b_k), batch=p.batch, inner=p.inner,
                sAo=p.sA[0], sAi=p.sA[1], sBo=p.sB[0], sBi=p.sB[1], sCo=p.sC[0], sCi=p.sC[1], kbatch=p.kbatch, sAk=p.sAk, sBk=p.sBk,
                accumulate=int(accumulate), splits=splits, alpha=alpha, precision=N.PRECISIONS[prec])
            N.check(N.gemm_ex(desc, N.stream_ptr()), f"dq_gemm_ex ({group}, {prec})")
            torch.cuda.synchronize()
            # nothing written around the scratch the plan asked for
            assert torch.isnan(scratch[:GUARD]).all() and torch.isnan(scratch[GUARD + need:]).all(), (group, prec)
            outs.append(C)
        C = outs[0]
        assert torch.equal(bits(outs[0]), bits(outs[1])), f"{group} {prec}: not bitwise repeatable"
        assert torch.equal(bits(C)[~d.window], bits(Cinit)[~d.window]), f"{group} {prec}: wrote outside the M x N windows of C"
        got = p.c_view(C).double()
        assert not torch.isnan(got).any(), f"{group} {prec}: a masked operand element reached the result"
        errs[prec] = float((got - ref).abs().max())
        print(f"[gemm_paths] {group} {prec} acc={int(accumulate)} add={int(add)} alpha={alpha} splits={splits} plan={got_plan} "
              f"err={errs[prec]:.3e} tol={tol[prec]:.3e} ratio={errs[prec] / tol[prec]:.3f}")
    for prec in PRECISIONS:
        assert errs[prec] < tol[prec], (group, prec, errs[prec], tol[prec])
    assert errs["fp32"] <= errs["bf16x3"] + 1e-6 * float(ref.abs().max()), (group, errs)  # the fp32 kernel is at least as close
    return {prec: errs[prec] / tol[prec] for prec in PRECISIONS}


# ------------------------------------------------------------------------------------------------ a. tile forms x layouts
# (name, M, N, K, forced splits of the case itself, plan of the case, plan of the same shape under a forced split of 3)
TILE_FORMS = [
    ("bm64 one round", 190, 8100, 36, 0, dict(bm=64, full=0, ntiles=192, splits=1), dict(splits=2, k_per_split=32)),
    ("bm64 153 tiles", 1030, 1030, 68, 0, dict(bm=64, full=0, ntiles=153, splits=1), dict(splits=3, k_per_split=32)),
    ("bm128 204 tiles", 1500, 2100, 36, 0, dict(bm=128, full=0, ntiles=204, splits=1), dict(bm=128, ntiles=204, splits=2, k_per_split=32)),
    ("bm128 81 tiles x 3", 1030, 1030, 68, 3, dict(bm=128, full=0, ntiles=81, splits=3, k_per_split=32), None),
]


@pytest.mark.parametrize("layout", ["kk", "kn", "mn"])
@pytest.mark.parametrize("case", TILE_FORMS, ids=[c[0].replace(" ", "-") for c in TILE_FORMS])
def test_tile_forms(N, case, layout):
    name, M, Nn, K, splits, expect, expect3 = case
    d = Data(Product(M, Nn, K, layout), seed=M * 7 + Nn)
    group = f"tile {name} {layout}"
    run_variant(N, d, group, bias=True, splits=splits, expect=expect)
    run_variant(N, d, group, accumulate=True, splits=splits, expect=expect)
    if expect3 is not None:
        run_variant(N, d, group + " split3", bias=True, splits=3, expect=expect3)


# ------------------------------------------------------------------------------------------------ b. two-launch plans
TWO_LAUNCH = [
    # K shorter than one k-tile; 2 tiles behind a round
    ("32: 256 + 2", 20, 33000, 8, ("kk", "kn"), dict(bm=32, full=256, ntiles=2, splits=1)),
    # 41 remaining tiles: not a multiple of 8, the XCD remap of the rest launch ends in an identity tail
    ("128: 256 + 41", 1027, 4100, 36, ("mn",), dict(bm=128, full=256, ntiles=41, splits=1)),
    ("64: 512 + 64", 515, 8100, 132, ("kn",), dict(bm=64, full=512, ntiles=64, splits=1)),
    # one split tile behind a round: the partial-tile index with tile_base != 0
    ("64: 256 + 1 x 8", 33, 32800, 256, ("kk", "kn", "mn"), dict(bm=64, full=256, ntiles=1, splits=8, k_per_split=32)),
]


@pytest.mark.parametrize("case", [(c, l) for c in TWO_LAUNCH for l in c[4]], ids=[f"{c[0].replace(' ', '')}-{l}" for c in TWO_LAUNCH for l in c[4]])
def test_two_launch_plans(N, case):
    (name, M, Nn, K, _, expect), layout = case
    d = Data(Product(M, Nn, K, layout), seed=M + Nn + K)
    group = f"two-launch {name} {layout}"
    run_variant(N, d, group, bias=True, expect=expect)
    run_variant(N, d, group, accumulate=True, expect=expect)


# ------------------------------------------------------------------------------------------------ c. batched
B_, HEADS, DH, S1, SK = 3, 3, 20, 34, 54
H_, LDP = HEADS * DH, up4(SK)
QS, KVS, PS = S1 * H_, SK * 2 * H_, S1 * LDP  # per-sample floats of q / o, of [K | V], of one head's probabilities


def attn_product(which):
    """The operand patterns of the transformer's six batched attention products (dq_tfm.hip: attn_gemm): q, dO, o as (B, S1, H) with a head's
    dh columns at zi * dh, [K | V] and its gradient as (B, Sk, 2 H), the probabilities as (B, heads, S1, ldp)."""
    kw = dict(batch=B_ * HEADS, inner=HEADS)
    if which in (0, 2):  # scores = Q K^T, dP = dO V^T
        return Product(S1, SK, DH, "kk", lda=H_, sA=(QS, DH), ldb=2 * H_, sB=(KVS, DH), offB=H_ if which == 2 else 0, nB=B_ * KVS,
                       ldc=LDP, sC=(PS * HEADS, PS), nA=B_ * QS, nC=B_ * HEADS * PS, **kw)
    if which in (1, 4):  # O = P V, dQ = dS K
        return Product(S1, DH, SK, "kn", lda=LDP, sA=(PS * HEADS, PS), nA=B_ * HEADS * PS, ldb=2 * H_, sB=(KVS, DH), offB=H_ if which == 1 else 0,
                       nB=B_ * KVS, ldc=H_, sC=(QS, DH), nC=B_ * QS, **kw)
    # dV = P^T dO, dK = dS^T Q, into the V / K half of d[K | V]
    return Product(SK, DH, S1, "mn", lda=LDP, sA=(PS * HEADS, PS), nA=B_ * HEADS * PS, ldb=H_, sB=(QS, DH), nB=B_ * QS,
                   ldc=2 * H_, sC=(KVS, DH), offC=H_ if which == 3 else 0, nC=B_ * KVS, **kw)


@pytest.mark.parametrize("which", range(6), ids=["scores", "PV", "dP", "dV", "dQ", "dK"])
def test_attention_products(N, which):
    d = Data(attn_product(which), seed=100 + which)
    expect = dict(bm=32, full=0, ntiles=2, splits=1)
    run_variant(N, d, f"attn {which}", splits=1, expect=expect)  # attn_gemm forces the unsplit plan
    run_variant(N, d, f"attn {which}", accumulate=True, splits=1, expect=expect)


@pytest.mark.parametrize("a_layout", ["k", "m"])
@pytest.mark.parametrize("Bsz", [1, 3])
@pytest.mark.parametrize("RT", [33, 413])
def test_wide_gemm_pattern(N, RT, Bsz, a_layout):
    """dq_ops.hip: wide_gemm -- a shared weight (sAo = 0) against (Bsz, rows, P) tensors, N = RT < P = RT rounded up to 4."""
    M, K, P = 40, 120, up4(RT)
    p = Product(M, RT, K, a_layout + "n", sA=(0, 0), ldb=P, sB=(K * P, 0), ldc=P, sC=(M * P, 0), batch=Bsz)
    d = Data(p, seed=RT + Bsz)
    expect = dict(bm=32, full=0, ntiles=2 * cdiv(RT, 128), splits=1)
    group = f"wide RT{RT} B{Bsz} {a_layout}"
    run_variant(N, d, group, bias_m=True, expect=expect)
    run_variant(N, d, group, accumulate=True, expect=expect)
    run_variant(N, d, group + " add", bias_m=True, add=True, splits=1, expect=expect)  # attn_out = x + W o + b in one epilogue


# ------------------------------------------------------------------------------------------------ d. k-batched
@pytest.mark.parametrize("MN", [(40, 120), (12, 36)])
@pytest.mark.parametrize("Bsz", [1, 3])
@pytest.mark.parametrize("RT", [31, 33, 413])
def test_wide_wgrad_pattern(N, RT, Bsz, MN):
    """dq_ops.hip: wide_wgrad -- dW (M, N) += sum over the samples of dY_b (M, RT) X_b^T, both k-major (Bsz, ., P) tensors, K = RT any length."""
    M, Nn = MN
    P = up4(RT)
    p = Product(M, Nn, RT, "kk", lda=P, ldb=P, ldc=Nn, kbatch=Bsz, sAk=M * P, sBk=Nn * P)
    d = Data(p, seed=RT * 3 + Bsz + M)
    expect = dict(bm=32, full=0, kv=Bsz * cdiv(RT, 32) * 32 if Bsz > 1 else RT)
    expect["splits"] = {31: 1, 33: 1, 413: 39 if Bsz > 1 else 13}[RT]
    run_variant(N, d, f"wgrad RT{RT} B{Bsz} {M}x{Nn}", accumulate=True, expect=expect)


def test_wide_wgrad_split_inside_a_sample(N):
    """kp = 64, k_per_split = 96: the second split starts in the middle of the second sample's block."""
    RT, Bsz, M, Nn = 33, 3, 40, 120
    P = up4(RT)
    d = Data(Product(M, Nn, RT, "kk", lda=P, ldb=P, ldc=Nn, kbatch=Bsz, sAk=M * P, sBk=Nn * P), seed=7)
    run_variant(N, d, "wgrad forced split", accumulate=True, splits=2, expect=dict(bm=32, kv=192, splits=2, k_per_split=96))
    run_variant(N, d, "wgrad forced split", bias=True, alpha=-0.37, splits=2, expect=dict(splits=2))


# ------------------------------------------------------------------------------------------------ e. alpha
def test_alpha(N):
    """alpha scales the product only: not the bias, not the old C; the split path applies it in the reduce kernel."""
    d = Data(Product(1030, 1030, 68, "kk"), seed=11)
    run_variant(N, d, "alpha unsplit", bias=True, alpha=-0.37, expect=dict(bm=64, splits=1))
    run_variant(N, d, "alpha split", bias=True, alpha=-0.37, splits=3, expect=dict(bm=128, splits=3))
    run_variant(N, d, "alpha unsplit acc", accumulate=True, alpha=-0.37, expect=dict(splits=1))
    run_variant(N, d, "alpha split acc", accumulate=True, bias=True, alpha=-0.37, splits=3, expect=dict(splits=3))
    d = Data(Product(40, 413, 120, "kn", ldb=416, sB=(120 * 416, 0), ldc=416, sC=(40 * 416, 0), batch=3), seed=12)
    run_variant(N, d, "alpha batched", bias_m=True, alpha=-0.37, expect=dict(bm=32, splits=1))
