"""az_gemm_f32's K-major fp32 family, dispatch class by dispatch class, against CPU references.

Every forward shape that launch_x3 does not take (M <= 64, K < 1024 or N < 256, gathered or
concatenated rows) falls to this family: the M <= 8 GEMVs (gemv_full<MR, S>, gemv_rows, the chunked
gemv_f32<MR>), gemm_tall, and the fp32 MFMA tiles -- the register-staged 64 x 64 tile (`reg64`),
the LDS-DMA 128 x 128 tile with its split-K model (glds_splits, up to 16 splits), the 128 x 64
tile and the 256 x 128 8-wave tile (splits_256x128) -- with the split-K reduce in its seven float4
instantiations and its scalar form.  Here:

  * TABLE names, per class, the shapes that reach it; the coverage test runs all of them once in a
    child process on the tuning library with AZ_GEMM_PRINT=1 and holds every row to the class (and
    split count) the dispatcher prints, so a dispatcher change that empties a class fails there;
  * integer operands (x in {-1, 0, 1}, w in {-2 .. 2}, bias, R, C in {-3 .. 3}, G in {-2 .. 2})
    make every product and partial sum an exact integer: the WHOLE output is torch.equal to the
    fp32 CPU product for act = NONE / RELU and for R + G * relu(..) with beta = 1 onto an integer
    C, in every split-K form;
  * real operands (uniform +-1 rows, +-1 / sqrt(K) weights) against float64 within the project's
    fp32 dot-product bound (gradcheck.check_dot_error, 1e-6 * (sum_k |a_k b_k| + |b|)), also
    through SIGMOID and TANH;
  * an epilogue / layout matrix on one small shape per family: no bias, a bias 4 B off 16-B
    alignment, N % 4 != 0, column-slice outputs, R / G with their own leading dimensions, c_rows
    scatter, beta = 1, C2, the [x, x2] concat at both ends of K, gathered rows;
  * two CPU-only tests: the exactness condition and the dropped-k-range control.

Classes that had no direct test before this file: 14 of the 19 gemv_full<MR, S> instantiations,
gemv_f32<2> / <4> and <8> at 1024 < K <= 2048, the 128 x 128 tile at any split count but 1 (so
also the scalar reduce above 8 splits and reduce4<2..4, 6, 7>), the 128 x 64 tile, the 256 x 128
tile in fp32, reg64 at split counts 2..7, and two of gemm_tall's five (N, K) instantiations.

Worst error / bound per class on MI355X (real operands, act = NONE; $AZ_REPORT_DIR/margins.jsonl
has every shape and activation): gemv_full 0.037 (S = 1) falling to 0.016 (S = 16), gemv_rows
0.017, gemv_f32 0.023; reg64 0.20 at one split, 0.04-0.07 at 3-8; the 128 x 128 tile 0.17 at
S = 1 falling to 0.03 at S = 16; 128 x 64 0.17; 256 x 128 0.20 at S = 2, 0.05 at S = 8; gemm_tall
0.28.  Through SIGMOID / TANH the same or lower, except SIGMOID at K = 4 (0.35 of the bound with
its output-rounding term, see ACT_ULPS).  Nothing came near the bound and every integer case was
exact: the file found no kernel fault.

How the table was derived (a comment, not an oracle -- the print is): M <= 8 -> GEMV, S the
smallest of {1, 2, 4, 8, 13, 16} with K <= 256 S and MR S <= 32 (MR = 1, 2, 4, 8 for M = 1, 2,
3-4, 5-8), gemv_rows for M >= 3 at 2048 < K <= 3328, else chunked; M > 64, K >= 1024, N >= 256 ->
launch_x3 (not this family); M > 256 and 218..256 blocks of 256 x 128 with K / S >= 256 -> the
256 x 128 tile; M > 128 -> 128 x 64 at >= 256 tiles of 128 x 128, else 128 x 128 with glds_splits'
cost model; everything else, and any gathered / concatenated A, -> reg64 with plan()'s split
(min(8, ceil(1024 / tiles), K / 128)).  These rules use the literal 256, not the device's CU count,
so the table holds on any gfx950 part and needs no CU assertion."""
import functools
import hashlib
import json
import os
import re
import subprocess
import sys
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import report
from gradcheck import check_dot_error
from test_gpu_gemm_widths import _drop_k_range

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3

# kind: "" = plain x, "x2" = the [x, x2] concat (K0 = K / 2 rounded to 4), "rows" = gathered rows
Case = namedtuple("Case", "M N K cls kind", defaults=("",))

# ---------------------------------------------------------------------------------------- GEMV
GEMV_KS = (252, 256, 260, 508, 512, 516, 1020, 1024, 1028, 2044, 2048, 2052, 3324, 3328, 3332,
           4092, 4096, 4100)          # 256 S - 4, 256 S, 256 S + 4 for S = 1, 2, 4, 8, 13, 16
# per M, the class at each K of GEMV_KS: a number = gemv_full's S, r = gemv_rows, c = chunked
GEMV_ROWS = {
    1: (1, "1 1 2 2 2 4 4 4 8 8 8 13 13 13 16 16 16 c"),
    2: (2, "1 1 2 2 2 4 4 4 8 8 8 13 13 13 16 16 16 c"),
    3: (4, "1 1 2 2 2 4 4 4 8 8 8 r r r c c c c"),
    4: (4, "1 1 2 2 2 4 4 4 8 8 8 r r r c c c c"),
    5: (8, "1 1 2 2 2 4 4 4 c c c r r r c c c c"),
    8: (8, "1 1 2 2 2 4 4 4 c c c r r r c c c c"),
}


def _gemv_cls(mr, tok):
    return ("gemv_rows" if tok == "r" else f"gemv_f32<{mr}>" if tok == "c"
            else f"gemv_full<{mr},{tok}>")


GEMV = [Case(M, N, K, _gemv_cls(mr, tok))
        for M, (mr, toks) in GEMV_ROWS.items() for K, tok in zip(GEMV_KS, toks.split())
        for N in (37, 1001)]
GEMV += [Case(2, 3136, 2052, "gemv_full<2,13>"), Case(4, 3136, 3332, "gemv_f32<4>"),
         Case(8, 3136, 1028, "gemv_f32<8>")]

# --------------------------------------------------------------------------------------- tiles
TILES = (
    # 128 x 128 + glds_splits: M = 129 (2 x 2 tiles at N = 200, the second column tile partial)
    [Case(129, 200, K, f"glds128x128/S{S}") for K, S in
     ((260, 2), (384, 3), (512, 4), (640, 5), (768, 6), (900, 8), (1152, 9), (1540, 13),
      (3136, 14), (1920, 15), (2048, 16))] +
    [Case(4100, 8, 996, "glds128x128/S7"), Case(4100, 72, 996, "glds128x128/S7"),
     Case(3150, 8, 1540, "glds128x128/S10"), Case(3150, 72, 1540, "glds128x128/S10"),
     Case(130, 70, 48, "glds128x128/S1"),
     Case(3150, 512, 512, "glds128x128/S2")] +          # TicTacToe fc2, the lock-step batch
    # 128 x 64: >= 256 tiles of 128 x 128
    [Case(4096, 1024, 256, "glds128x64/S2"), Case(7000, 520, 4, "glds128x64/S1"),
     Case(7000, 520, 384, "glds128x64/S3")] +
    # 256 x 128 in fp32 through splits_256x128
    [Case(2049, 3136, 4, "glds2_256x128/S1"), Case(1025, 3136, 512, "glds2_256x128/S2"),
     Case(513, 3136, 768, "glds2_256x128/S3"), Case(7000, 200, 1024, "glds2_256x128/S4"),
     Case(8200, 8, 2048, "glds2_256x128/S7"), Case(8200, 72, 2048, "glds2_256x128/S7"),
     Case(7000, 8, 2048, "glds2_256x128/S8"), Case(7000, 72, 2048, "glds2_256x128/S8"),
     Case(8192, 512, 512, "glds2_256x128/S2")] +        # TicTacToe fc2 at evaluate()'s chunk
    # reg64: small M (N = 70: N % 4 != 0, N = 72: float4 epilogue), gathered / concatenated rows
    [Case(9, N, K, f"reg64/S{S}") for N in (70, 72) for K, S in
     ((4, 1), (260, 2), (384, 3), (512, 4), (640, 5), (768, 6), (996, 7), (1024, 8))] +
    [Case(64, 3136, 3136, "reg64/S8"), Case(128, 300, 132, "reg64/S1"),
     Case(300, 72, 260, "reg64/S2", "x2"), Case(300, 72, 516, "reg64/S4", "rows")] +
    # gemm_tall: the two (N, K) instantiations test_linear_tall_skinny never runs
    [Case(16384, 128, 128, "tall"), Case(16385, 256, 64, "tall")]
)
CASES = GEMV + TILES
TABLE = {}                      # class -> [(M, N, K)]
for _c in CASES:
    TABLE.setdefault(_c.cls, []).append((_c.M, _c.N, _c.K))

# every class the table must reach (the coverage test's list)
REQUIRED = (
    [f"gemv_full<{mr},{S}>" for mr in (1, 2, 4, 8) for S in (1, 2, 4, 8, 13, 16) if mr * S <= 32] +
    ["gemv_rows"] + [f"gemv_f32<{mr}>" for mr in (1, 2, 4, 8)] +
    [f"reg64/S{S}" for S in range(1, 9)] +
    [f"glds128x128/S{S}" for S in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16)] +
    [f"glds128x64/S{S}" for S in (1, 2, 3)] +
    [f"glds2_256x128/S{S}" for S in (1, 2, 3, 4, 7, 8)] + ["tall"]
)
REQUIRED_REDUCES = [f"reduce4<{S}>" for S in range(2, 9)] + ["scalar"]

# shapes that satisfy full_waves_256x128 (N >= 1024, K >= 1024, >= 4 rounds of 256 blocks, the
# last >= 95 % full: >= 973 tiles) with the class and rule the product rules give them: launch_x3
# takes every M > 64; it declines M <= 64, so 973 column tiles under one row tile reach the branch
FULL_WAVES_SMALL_M = (9, 124420, 1024)
FULL_WAVES_PROBES = [((32768, 1024, 1024), "x3/S1", None),
                     (FULL_WAVES_SMALL_M, "glds2_256x128/S2", "full_waves")]

# The epilogue / layout matrix: one small shape per family (its class without gather / concat).
MATRIX_SHAPES = [
    Case(4, 72, 260, "gemv_full<4,2>"),
    Case(40, 72, 516, "reg64/S4"),
    Case(130, 72, 48, "glds128x128/S1"),
    Case(129, 72, 640, "glds128x128/S5"),        # reduce4<5>, scalar when vec_epi = 0
    Case(129, 72, 1152, "glds128x128/S9"),       # the scalar reduce above 8 splits
    Case(7000, 520, 384, "glds128x64/S3"),
    Case(513, 3136, 768, "glds2_256x128/S3"),
]
VARIANTS = ("plain", "no_bias", "bias_off4", "n_odd", "ldc_aligned", "ldc_off4", "ldc_odd",
            "gated_ld", "gated_off4", "c_rows", "beta1", "c2", "x2_k4", "x2_km4", "a_rows")
# variants whose operands break the float4 epilogue's alignment test (vec_epi = 0)
NOT_VEC = ("bias_off4", "n_odd", "ldc_off4", "ldc_odd", "gated_off4")
SENTINEL = -77.0


def _max_m(N, K):
    return max(c.M for c in CASES + MATRIX_SHAPES if (c.N, c.K) == (N, K))


def _id(c):
    return f"{c.cls}-M{c.M}_N{c.N}_K{c.K}" + (f"_{c.kind}" if c.kind else "")


def _rows(M):
    """Gathered row indices: descending, with every third one repeating its predecessor."""
    r = torch.arange(M - 1, -1, -1, dtype=torch.int32)
    r[2::3] = r[1::3][:len(r[2::3])]
    return r


# ------------------------------------------------------------------------------- operands (CPU)
@functools.lru_cache(maxsize=None)
def int_operands(N, K):
    """Integer-valued fp32 operands of one (N, K), generated once: x [max M][K] in {-1, 0, 1},
    w [N][K] in {-2 .. 2}, b [N] in {-3 .. 3}."""
    g = torch.Generator().manual_seed(7000 * N + K)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    return SimpleNamespace(x=ri(-1, 1, _max_m(N, K), K), w=ri(-2, 2, N, K), b=ri(-3, 3, N))


@functools.lru_cache(maxsize=None)
def int_reference(N, K):
    """The fp32 CPU product p = x w^T of int_operands(N, K) for all max-M rows (rows are
    independent: the first M serve every M)."""
    d = int_operands(N, K)
    return d.x @ d.w.T


@functools.lru_cache(maxsize=None)
def int_magnitude(N, K):
    """max_ij of (sum_k |a_ik b_jk| + |bias_j|) * max|G| + max|R| + max|C|: below 2^24 every
    partial sum of every summation order, and every epilogue this file runs, is an exactly
    representable integer on the CPU and on the GPU."""
    d = int_operands(N, K)
    return float((d.x.abs() @ d.w.abs().T + d.b.abs()).max()) * 2 + 3 + 3


@functools.lru_cache(maxsize=None)
def real_operands(N, K):
    """Real-valued operands of one (N, K): uniform +-1 rows, +-1 / sqrt(K) weights, bias in
    +-0.5."""
    g = torch.Generator().manual_seed(9000 * N + K)
    return SimpleNamespace(x=torch.rand((_max_m(N, K), K), generator=g) * 2 - 1,
                           w=(torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5,
                           b=torch.rand((N,), generator=g) - 0.5)


@functools.lru_cache(maxsize=None)
def real_reference(N, K):
    """float64 y = x w^T + b of real_operands(N, K) for all max-M rows and the magnitudes
    sum_k |x_k w_k| + |b| the bound is relative to."""
    d = real_operands(N, K)
    x, w, b = d.x.double(), d.w.double(), d.b.double()
    return SimpleNamespace(y=(x @ w.T + b).numpy(), mag=(x.abs() @ w.abs().T + b.abs()).numpy())


# The activated outputs: tanh / sigmoid are 1-Lipschitz, so the dot product's error passes through
# at most unchanged; on top the fp32 result of the activation itself carries the rounding of
# expf / tanhf (<= 2 ulp), of 1 + e and of the division (<= 0.5 ulp each) -- at most ACT_ULPS = 4
# ulp of the result.  Without this term the bound 1e-6 * (sum |x w| + |b|) falls below half an ulp
# of sigmoid's 0.5 wherever the magnitude is under 0.03 (K = 4 rows), which no fp32 result meets.
ACT_ULPS = 4
ACTS = ((ACT_NONE, "none", lambda t: t), (ACT_SIGMOID, "sigmoid", lambda t: 1 / (1 + np.exp(-t))),
        (ACT_TANH, "tanh", np.tanh))


def real_ratio(got, ref, mag, act):
    """max |got - act(ref)| / bound with bound = 1e-6 * mag (+ ACT_ULPS ulp of the activated
    value); asserts it through gradcheck.check_dot_error."""
    want = ACTS[[a[0] for a in ACTS].index(act)][2](ref)
    bound = mag if act == ACT_NONE else mag + ACT_ULPS * 2.0 ** -24 * np.abs(want) / 1e-6
    got = np.asarray(got, np.float64)
    ratio = float((np.abs(got - want) / (1e-6 * bound)).max())
    assert np.isfinite(got).all()
    check_dot_error(got, want, bound)
    return ratio


def literal_ratio(got, ref, mag, act):
    """The figure without the ACT_ULPS term, max |got - act(ref)| / (1e-6 * mag): reported, not
    asserted (above 1 for SIGMOID at K = 4, where it asks for less than the output's rounding)."""
    want = ACTS[[a[0] for a in ACTS].index(act)][2](ref)
    return float((np.abs(np.asarray(got, np.float64) - want) / (1e-6 * mag)).max())


def _select(c, t):
    """The rows of a max-M reference the case's A holds (gathered rows: x[rows])."""
    return t[_rows(c.M).long().to(t.device)] if c.kind == "rows" else t[:c.M]


# ------------------------------------------------------------------------------- CPU-only tests
def test_integer_operands_are_exact():
    """The condition that makes the integer cases exact, on this file's operands: for every
    (N, K) of the table and the matrix, (max_ij sum_k |a_ik b_jk| + |bias_j|) max|G| + max|R| +
    max|C| < 2^24; the products are integers, and at one shape the fp32 CPU product is the
    float64 one."""
    for N, K in sorted({(c.N, c.K) for c in CASES + MATRIX_SHAPES}):
        mag = int_magnitude(N, K)
        assert 0 < mag < 2 ** 24, (N, K, mag)
        assert mag <= (2 * K + 3) * 2 + 6
    d, p = int_operands(200, 3136), int_reference(200, 3136)
    assert (p == p.round()).all() and p.abs().max() > 100
    assert torch.equal(p.double(), d.x.double() @ d.w.double().T)


def test_integer_check_rejects_a_dropped_k_range():
    """The control, on the CPU at the largest K of a tile shape (64 x 3136 x 3136, reg64 with 8
    splits): the fp32 CPU product stands in for the GPU's result; with one 32-wide k range of one
    64 x 64 tile missing, torch.equal fails.  The same fault on the real operands: a float64
    product with the range missing is outside the 1e-6 bound at almost every element of the tile
    (32 products of ~1 / (3 sqrt K) against 1e-6 * sqrt(K) / 4: three orders of magnitude), so
    there the bound catches it too; what only the integer form catches is anything smaller --
    at K = 3136 one missing product stays inside the bound for the elements whose product is below
    1e-6 * mag, while on the integer operands any nonzero product breaks equality."""
    M, N, K = 64, 3136, 3136
    rows, cols, k0 = torch.arange(0, 64), torch.arange(3072, 3136), 2400   # the last column tile
    di, p = int_operands(N, K), int_reference(N, K)
    assert not torch.equal(_drop_k_range(p[:M], di.x[:M], di.w, rows, cols, k0), p[:M])
    d, r = real_operands(N, K), real_reference(N, K)
    good = torch.from_numpy(r.y[:M])
    assert real_ratio(good.numpy(), r.y[:M], r.mag[:M], ACT_NONE) == 0.0
    bad = _drop_k_range(good, d.x[:M], d.w, rows, cols, k0).numpy()
    with pytest.raises(AssertionError):
        real_ratio(bad, r.y[:M], r.mag[:M], ACT_NONE)
    e = np.abs(bad - r.y[:M])[:, 3072:] / (1e-6 * r.mag[:M][:, 3072:])
    print(f"dropped 32-k range, real operands: {float((e > 1).mean()):.4f} of the tile's "
          f"elements over the bound, median ratio {float(np.median(e)):.0f}")
    assert (e > 1).mean() > 0.99
    # one missing product: inside the bound where |x_k w_k| <= 1e-6 * mag
    # (P(|u v| < t) = t (1 - ln t) for uniform u, v; t = 1e-6 * mag * sqrt(K) ~ 8e-4: 0.6 %)
    one = np.abs((d.x[:M, None, k0:k0 + 32].double() *
                  d.w[None, 3072:, k0:k0 + 32].double()).numpy())
    hidden = float((one <= 1e-6 * r.mag[:M][:, 3072:, None]).mean())
    print(f"one dropped product, real operands: {hidden:.4f} of the products stay inside")
    assert 0 < hidden < 0.05


# ------------------------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def ops():
    from azhip import ops as _ops
    from azhip import _lib
    _lib.lib()
    return _ops


class _Device:
    """Per-(N, K) device copies, made on first use and kept for the module."""

    def __init__(self):
        self.cache = {}

    def ints(self, N, K):
        if ("i", N, K) not in self.cache:
            d = int_operands(N, K)
            assert int_magnitude(N, K) < 2 ** 24
            self.cache[("i", N, K)] = SimpleNamespace(
                x=d.x.cuda(), w=d.w.cuda(), b=d.b.cuda(), p=int_reference(N, K).cuda())
        return self.cache[("i", N, K)]

    def reals(self, N, K):
        if ("r", N, K) not in self.cache:
            d = real_operands(N, K)
            self.cache[("r", N, K)] = SimpleNamespace(x=d.x.cuda(), w=d.w.cuda(), b=d.b.cuda())
        return self.cache[("r", N, K)]


@pytest.fixture(scope="module")
def dev(ops):
    d = _Device()
    yield d
    torch.cuda.synchronize()
    d.cache.clear()


def _first_diff(got, ref):
    """(row, column, got, expected, count) of the first differing element, for the message."""
    bad = (got != ref).nonzero()
    if not len(bad):
        return None
    i, j = (int(v) for v in bad[0])
    return i, j, float(got[i, j]), float(ref[i, j]), int(len(bad))


def _a_args(c, x, k0=None):
    """ops.linear's A arguments of a case: (x, kwargs)."""
    if c.kind == "x2" or k0 is not None:
        k0 = k0 if k0 is not None else c.K // 2 // 4 * 4
        return x[:c.M, :k0], dict(x2=x[:c.M, k0:].contiguous())
    if c.kind == "rows":
        return x, dict(a_rows=_rows(c.M).to(x.device), M=c.M)
    return x[:c.M], {}


def _ints(lo, hi, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float().cuda()


@gpu
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_integer_exact(ops, dev, c):
    """ops.linear on integer operands: act = NONE and RELU with bias, then the gated residual
    R + G * relu(..) with beta = 1 onto an integer C -- the whole output equals the CPU product
    (carried through the exact integer epilogue)."""
    e = dev.ints(c.N, c.K)
    x, kw = _a_args(c, e.x)
    lin = _select(c, e.p) + e.b
    for act, ref in ((ACT_NONE, lin), (ACT_RELU, torch.relu(lin))):
        y = ops.linear(x, e.w, e.b, act=act, **kw)
        assert torch.equal(y, ref), (act, _first_diff(y, ref))
    R, G, C0 = (_ints(-h, h, (c.M, c.N), s) for h, s in ((3, 1), (2, 2), (3, 3)))
    out = C0.clone()
    ops.linear(x, e.w, e.b, act=ACT_RELU, R=R, G=G, beta=1.0, out=out, **kw)
    ref = C0 + (R + G * torch.relu(lin))
    assert torch.equal(out, ref), ("gated", _first_diff(out, ref))


@gpu
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_real_accuracy(ops, dev, c):
    """ops.linear on uniform operands against float64: every element within 1e-6 of
    sum_k |x_k w_k| + |b| (gradcheck.check_dot_error), also through SIGMOID and TANH."""
    e, r = dev.reals(c.N, c.K), real_reference(c.N, c.K)
    x, kw = _a_args(c, e.x)
    ref, mag = (_select(c, torch.from_numpy(t)).numpy() for t in (r.y, r.mag))
    ratios = {}
    for act, name, _ in ACTS:
        y = ops.linear(x, e.w, e.b, act=act, **kw).cpu().numpy()
        ratios[name] = real_ratio(y, ref, mag, act)
        if act != ACT_NONE:
            ratios[name + "_without_ulp_term"] = literal_ratio(y, ref, mag, act)
    report(f"gemm_dispatch/{c.cls}/M{c.M}_N{c.N}_K{c.K}" + (f"_{c.kind}" if c.kind else ""),
           ratio_to_bound=max(v for k, v in ratios.items() if "_" not in k), **ratios)
    print(f"gemm_dispatch/{_id(c)}: err / bound " +
          " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


# ------------------------------------------------------------------- epilogue / layout matrix
def run_variant(ops, dev, c, v):
    """One cell of the matrix on integer operands (act = RELU with bias unless the variant says
    otherwise).  Returns [(name, got, expected)]: every tensor the call may write, whole --
    the columns / rows around a slice or a scatter must keep SENTINEL."""
    M, N, K = c.M, c.N, c.K
    e = dev.ints(N, K)
    w, b, p = e.w, e.b, e.p[:M]
    if v == "n_odd":
        N -= 2                                           # 72 -> 70, 520 -> 518, 3136 -> 3134
        w, b, p = w[:N], b[:N], p[:, :N]
    if v == "no_bias":
        b = None
    if v == "bias_off4":
        store = torch.zeros(N + 1, device="cuda")
        store[1:] = b
        b = store[1:]
        assert b.data_ptr() % 16 == 4
    k0 = {"x2_k4": 4, "x2_km4": K - 4}.get(v)
    x, kw = _a_args(c, e.x, k0)
    if v == "a_rows":
        x, kw = e.x, dict(a_rows=_rows(M).cuda(), M=M)
        p = p[_rows(M).long().cuda()]
    val = torch.relu(p + b if b is not None else p)      # the pre-gate value (C2's)
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")  # noqa: E731
    if v in ("ldc_aligned", "ldc_off4", "ldc_odd"):
        off, wide = {"ldc_aligned": (4, N + 8), "ldc_off4": (1, N + 8), "ldc_odd": (0, N + 3)}[v]
        buf, want = full(M, wide), full(M, wide)
        out = buf[:, off:off + N]
        assert out.data_ptr() % 16 == 4 * (off % 4) and out.stride(0) == wide
        want[:, off:off + N] = val
        ops.linear(x, w, b, act=ACT_RELU, out=out, **kw)
        return [("out", buf, want)]
    if v in ("gated_ld", "gated_off4"):
        off = 4 if v == "gated_ld" else 1
        Rw, Gw = _ints(-3, 3, (M, N + 8), 11), _ints(-2, 2, (M, N + 12), 12)
        R, G = Rw[:, off:off + N], Gw[:, 4:4 + N]
        y = ops.linear(x, w, b, act=ACT_RELU, R=R, G=G, **kw)
        return [("out", y, R + G * val)]
    if v == "c_rows":
        V = M + 5
        cr = torch.randperm(V, generator=torch.Generator().manual_seed(V))[:M].int().cuda()
        R, G = _ints(-3, 3, (V, N), 13), _ints(-2, 2, (M, N), 14)     # R by c_rows, G by row
        buf, want = full(V, N), full(V, N)
        want[cr.long()] = R[cr.long()] + G * val
        ops.linear(x, w, b, act=ACT_RELU, R=R, G=G, c_rows=cr, out=buf, M=M, **kw)
        return [("out", buf, want)]
    if v == "beta1":
        C0 = _ints(-3, 3, (M, N), 15)
        out = C0.clone()
        ops.linear(x, w, b, act=ACT_RELU, beta=1.0, out=out, **kw)
        return [("out", out, C0 + val)]
    if v == "c2":
        R, G, C2 = _ints(-3, 3, (M, N), 16), _ints(-2, 2, (M, N), 17), full(M, N)
        y = ops.linear(x, w, b, act=ACT_RELU, R=R, G=G, C2=C2, **kw)
        return [("out", y, R + G * val), ("C2", C2, val)]
    y = ops.linear(x, w, b, act=ACT_RELU, **kw)
    return [("out", y, val)]


@gpu
@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("c", MATRIX_SHAPES, ids=_id)
def test_epilogue_matrix(ops, dev, c, v):
    """Every cell of the matrix is the exact integer result, in every tensor the call writes and
    nowhere else."""
    for name, got, want in run_variant(ops, dev, c, v):
        assert torch.equal(got, want), (name, _first_diff(got, want))


@gpu
@pytest.mark.parametrize("c", MATRIX_SHAPES, ids=_id)
def test_rejected_operands(ops, dev, c):
    """What az_gemm_f32 rejects is rejected (AZ_EINVAL), not computed: a concat split off a
    multiple of 4, an A row stride off a multiple of 4, a W 4 B off 16-B alignment; the output
    keeps its sentinel."""
    e = dev.ints(c.N, c.K)
    x = e.x[:c.M]
    out = torch.full((c.M, c.N), SENTINEL, device="cuda")
    xs = torch.zeros((c.M, c.K + 1), device="cuda")[:, :c.K]             # lda = K + 1
    ws = torch.zeros(c.N * c.K + 1, device="cuda")[1:].view(c.N, c.K)    # base 4 B off
    for what, call in (
            ("K0 % 4", lambda: ops.linear(x[:, :6], e.w, e.b, x2=x[:, 6:].contiguous(), out=out)),
            ("lda % 4", lambda: ops.linear(xs, e.w, e.b, out=out)),
            ("B alignment", lambda: ops.linear(x, ws, e.b, out=out))):
        with pytest.raises(RuntimeError, match="az_gemm_f32"):
            call()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@gpu
def test_full_waves_branch_small_m(ops):
    """The one product-reachable way into the full_waves_256x128 branch: M = 9 under 973 column
    tiles (N = 124,420, K = 1024; the 256 x 128 tile with plan()'s 2 splits).  The weight is a
    1001-row block repeated down N -- 1001 shares no factor with the 128-column tile, so every
    tile sees another phase of it -- and the reference is the CPU product of the block, repeated:
    integer operands equal it exactly, real ones stay within the fp32 dot-product bound."""
    M, N, K = FULL_WAVES_SMALL_M
    N0 = 1001
    reps = -(-N // N0)
    g = torch.Generator().manual_seed(N)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    x, w0, b0 = ri(-1, 1, M, K), ri(-2, 2, N0, K), ri(-3, 3, N0)
    tile = lambda t: t.cuda().repeat(reps, *([1] * (t.dim() - 1)))[:N]  # noqa: E731
    assert float((x.abs() @ w0.abs().T + b0.abs()).max()) < 2 ** 24
    ref = torch.relu(x @ w0.T + b0).repeat(1, reps)[:, :N]
    y = ops.linear(x.cuda(), tile(w0), tile(b0), act=ACT_RELU)
    assert torch.equal(y.cpu(), ref), _first_diff(y.cpu(), ref)
    x, w0, b0 = (torch.rand((M, K), generator=g) * 2 - 1,
                 (torch.rand((N0, K), generator=g) * 2 - 1) / K ** 0.5,
                 torch.rand((N0,), generator=g) - 0.5)
    y = ops.linear(x.cuda(), tile(w0), tile(b0)).cpu().numpy()
    ref = (x.double() @ w0.double().T + b0.double()).repeat(1, reps)[:, :N].numpy()
    mag = (x.double().abs() @ w0.double().abs().T + b0.double().abs()).repeat(1, reps)[:, :N]
    ratio = real_ratio(y, ref, mag.numpy(), ACT_NONE)
    report(f"gemm_dispatch/glds2_256x128_full_waves/M{M}_N{N}_K{K}", ratio_to_bound=ratio)
    print(f"gemm_dispatch/full_waves M{M}_N{N}_K{K}: err / bound {ratio:.3f}")


# ------------------------------------------------------------------------------ coverage (2e)
LINE = re.compile(r"gemm M=(\d+) N=(\d+) K=(\d+): (\w+) (.*)vec_epi=(\d)$")
REDUCE = re.compile(r"reduce M=(\d+) N=(\d+): (reduce4<\d>|scalar)")


def parse_launch(line):
    """A `gemm ...` line of AZ_GEMM_PRINT as (M, N, K, class, vec_epi, rule), class in the table's
    notation; None for any other line."""
    m = LINE.match(line)
    if not m:
        return None
    M, N, K, fam, rest, vec = m.groups()
    f = dict(t.split("=") for t in rest.split())
    if fam == "gemv_full":
        cls = f"gemv_full<{f['MR']},{f['S']}>"
    elif fam == "gemv_f32":
        cls = f"gemv_f32<{f['MR']}>"
    elif fam in ("gemv_rows", "tall"):
        cls = fam
    else:
        cls = f"{fam}/S{f['splits']}"
    return int(M), int(N), int(K), cls, int(vec), f.get("rule")


def _digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _real_call(ops, dev, c):
    e = dev.reals(c.N, c.K)
    x, kw = _a_args(c, e.x)
    return ops.linear(x, e.w, e.b, **kw)


def _child(path):
    """The coverage test's child (tuning library, AZ_GEMM_PRINT=1): a `case` line on stderr before
    each launch (the library's lines follow it) -- every table shape once on the real operands
    (their output digests into `path`), the full_waves probes on zeros, then the matrix, each
    cell checked here too."""
    from azhip import ops as _ops
    dev, out = _Device(), {}
    say = lambda s: (sys.stderr.write(s + "\n"), sys.stderr.flush())  # noqa: E731
    for c in CASES:
        say(f"case table {_id(c)}")
        out[_id(c)] = _digest(_real_call(_ops, dev, c))
    for (M, N, K), _, _ in FULL_WAVES_PROBES:
        say(f"case probe M{M}_N{N}_K{K}")
        z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
        _ops.linear(z(M, K), z(N, K), z(N))
        torch.cuda.synchronize()
    for c in MATRIX_SHAPES:
        for v in VARIANTS:
            say(f"case matrix {_id(c)} {v}")
            for name, got, want in run_variant(_ops, dev, c, v):
                assert torch.equal(got, want), (_id(c), v, name)
    with open(path, "w") as f:
        json.dump(out, f)
    print("ok")


@gpu
def test_table_covers_the_dispatch(ops, dev, tmp_path):
    """One child process on the tuning library prints every launch: each table shape takes the
    class (for tiles, the split count) the table names, every class of REQUIRED and every reduce
    kernel is reached, each tile family runs with vec_epi = 1 and = 0, no shape that satisfies
    full_waves_256x128 reaches the fp32 tile under the product rules, and the child's outputs are
    the product library's bits.  The family's rules use the literal 256, not the device's CU
    count, so there is no CU assertion.  A dispatcher change that empties a class fails here:
    give the table a new shape for it."""
    env = dict(os.environ)
    for k in [k for k in env if k.startswith(("AZ_GEMM_", "AZ_GEMV_", "AZ_CSK", "AZ_NO_",
                                              "AZ_SPLITK_", "AZ_HEADS_", "AZ_AB_LIB"))]:
        env.pop(k)
    env.update(AZ_TUNING_LIB="1", AZ_GEMM_PRINT="1")
    path = str(tmp_path / "digests.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    launches, reduces, case = {}, {}, None
    for line in r.stderr.splitlines():
        if line.startswith("case "):
            case = line[5:]
            continue
        q = parse_launch(line)
        if q:
            assert case is not None and case not in launches, f"two launches for {case}: {line}"
            launches[case] = q
        m = REDUCE.match(line)
        if m:
            reduces[case] = m.group(3)
    # each table shape took the class the table names
    reached = {}
    for c in CASES:
        q = launches.get(f"table {_id(c)}")
        assert q is not None, f"no launch printed for {_id(c)}"
        assert q[:3] == (c.M, c.N, c.K), (c, q)
        assert q[3] == c.cls, (f"{c.M} x {c.N} x {c.K} takes {q[3]}, the table says {c.cls}: "
                               "give the table a new shape for it")
        reached.setdefault(q[3], []).append((c.M, c.N, c.K))
    for cls in REQUIRED:
        assert cls in reached, f"no table shape reaches {cls}: give the table a new shape for it"
        print(f"gemm_dispatch/reached {cls}: {reached[cls][0]} (+{len(reached[cls]) - 1})")
        report(f"gemm_dispatch/reached/{cls}", shapes=reached[cls])
    assert set(reached) == set(REQUIRED), set(reached) - set(REQUIRED)
    got_reduces = set(reduces.values())
    for k in REQUIRED_REDUCES:
        assert k in got_reduces, f"no shape runs the split-K reduce as {k}"
    # a split launch is reduced, an unsplit one is not
    for case, q in launches.items():
        split = "/S" in q[3] and not q[3].endswith("/S1")
        assert (case in reduces) == split, (case, q, reduces.get(case))
    # full_waves_256x128: x3 takes the M > 64 shapes first; only M <= 64 under >= 973 column
    # tiles reaches the branch, and no table or matrix shape does
    for (M, N, K), cls, rule in FULL_WAVES_PROBES:
        q = launches[f"probe M{M}_N{N}_K{K}"]
        assert (q[3], q[5]) == (cls, rule), (M, N, K, q)
    assert all(q[5] != "full_waves" for case, q in launches.items() if not case.startswith("probe"))
    # the matrix: both epilogue forms per tile family, the variants' alignment as intended
    vec = {}
    for case, q in launches.items():
        if case.startswith("matrix "):
            vec.setdefault(q[3].split("/")[0].split("<")[0], set()).add(q[4])
            assert q[4] == (0 if case.split()[-1] in NOT_VEC else 1), (case, q)
    for fam in ("reg64", "glds128x128", "glds128x64", "glds2_256x128"):
        assert vec.get(fam) == {0, 1}, (fam, vec.get(fam))
    # the child's outputs are the product library's bits
    child = json.load(open(path))
    for c in CASES:
        assert child[_id(c)] == _digest(_real_call(ops, dev, c)), f"{_id(c)}: tuning vs product"


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "alphazero-gnn_amd"))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[1])
