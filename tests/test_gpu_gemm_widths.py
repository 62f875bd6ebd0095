"""output_transform's GEMMs and heads at every board width, against plain CPU references.

The fp16-split GEMM path (launch_x3: gemm_x3 / gemm_p3 split-K tiles, gemm_x3_csk stream-K with
csk_fixup4_kernel, the split-K reduce kernels) and the heads stages fused onto it run at
F = 64 n^2 = 1024 / 1600 / 2304 / 4096 for the 4x4 .. 8x8 Connect4 evaluators and at
K = 1152 -> N = 512 / 1152 for TicTacToe 5x5; the rest of the suite checks them against a
reference at N = K = 3136 only, where the stream-K planner has no choice but an in {1, 5} and
at in {1, 13} (25 tiles; 13 wide tiles, a prime) and the split counts are 8 and 5.  Here:

  * integer operands (x in {-1, 0, 1}, w in {-2 .. 2}, bias in {-3 .. 3}) make every kept product
    and partial sum an integer times a power of two, so the WHOLE output equals the CPU product
    (torch.equal) in every form -- a wrong tile index or a dropped k range cannot hide in a
    tolerance; the condition (sum_k |a_k b_k| + |bias| < 2^24) is asserted on the CPU;
  * real operands fill the low fp16 planes: every row of 256 random columns and the last (partial)
    256-column block within x3_bound(K) of float64;
  * one child process on the tuning library prints the stream-K plans, so the test fails when the
    table below stops covering the plan space (1 < an < N tiles, an = N tiles, 1 < at < wide
    tiles, tail / no tail, >= 4 pieces);
  * az_transform_heads_fwd / az_linear_heads_fwd at the widths: hidden and y per GEMM, the heads
    against a float64 restatement, y = NULL against the y path, registered against unregistered
    weights;
  * two CPU-only tests: the exactness condition, and that the checks reject a tile with one
    32-k range missing.

The (M, class) table was derived from launch_x3's conditions for 256 CUs and the default
workspace; classes and S values are comments, not assertions, except through the plan test."""
import functools
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import assert_close, report
from test_gpu_kernels import _registered, x3_bound, x3_ratio, x3_reference, x3_report

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

# (N, K) -> [(M, class)]: s128 = 128 x 128 split-K tiles (M <= 256), s256 = 256 x 128 split-K
# tiles, csk = stream-K.  Each M is the smallest of its class (derived, 256 CUs):
TABLE = {
    (1024, 1024): [(65, "s128"), (129, "s128"),        # S = 4, S = 4
                   (257, "s256"), (1793, "s256"),      # S = 4, S = 4
                   (2049, "csk"), (3000, "csk")],      # a tail of 1 row; no tail
    (1600, 1600): [(65, "s128"), (129, "s128"),        # S = 6, S = 6
                   (257, "s256"), (769, "s256"),       # S = 6, S = 4
                   (1025, "csk"), (2048, "csk")],      # tail; no tail, an = 13
    (2304, 2304): [(65, "s128"), (129, "s128"),        # S = 8, S = 7
                   (257, "s256"), (1576, "s256"),      # S = 7, S = 2
                   (769, "csk"), (2100, "csk")],       # tail; tail with at = 3
    (4096, 4096): [(65, "s128"), (129, "s128"),        # S = 8, S = 4
                   (257, "s256"), (769, "s256"),       # S = 4, S = 2
                   (513, "csk"), (700, "csk"), (1100, "csk")],   # tail, at = 2; no tail; tail
    (512, 1152): [(65, "s128"), (257, "s256"), (700, "s256")],   # TicTacToe 5x5 fc1 / fc2
    (1152, 1152): [(65, "s128"), (257, "s256"), (700, "s256")],  # and its output_transform
}
CASES = [(M, N, K) for (N, K), rows in TABLE.items() for M, _ in rows]
STREAMK = [(M, N, K) for (N, K), rows in TABLE.items() for M, c in rows if c == "csk"]


def _max_m(N, K):
    return max(M for M, _ in TABLE[(N, K)])


# ------------------------------------------------------------------------------- operands (CPU)
@functools.lru_cache(maxsize=None)
def int_operands(N, K):
    """Integer-valued fp32 operands of one width, generated once: x [max M][K] in {-1, 0, 1},
    w [N][K] in {-2 .. 2}, b [N] in {-3 .. 3}, and for square widths a second layer w2, b2."""
    g = torch.Generator().manual_seed(1000 * N + K)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    d = SimpleNamespace(x=ri(-1, 1, _max_m(N, K), K), w=ri(-2, 2, N, K), b=ri(-3, 3, N))
    if N == K:
        d.w2, d.b2 = ri(-2, 2, N, K), ri(-3, 3, N)
    return d


@functools.lru_cache(maxsize=None)
def int_reference(N, K):
    """fp32 CPU products of int_operands(N, K) for all max-M rows (rows are independent, so the
    first M serve every M): y = x w^T + b, h = relu(y), y2 = h w2^T + b2, with the largest
    sum_k |a_k b_k| + |bias| of each GEMM.  Below 2^24 every partial sum of every summation order
    is an exactly representable integer, on the CPU and in all of the GPU's forms."""
    d = int_operands(N, K)
    r = SimpleNamespace(y=d.x @ d.w.T + d.b, mag2=0.0)
    r.mag = float((d.x.abs() @ d.w.abs().T + d.b.abs()).max())
    r.h = torch.relu(r.y)
    if N == K:
        r.y2 = r.h @ d.w2.T + d.b2
        r.mag2 = float((r.h @ d.w2.abs().T + d.b2.abs()).max())
    return r


@functools.lru_cache(maxsize=None)
def real_operands(N, K):
    """Real-valued operands of one width, as output_transform's: uniform +-1 rows, +-1 / sqrt(K)
    weights; the columns the accuracy check reads (256 random ones and the last N % 256 or 256,
    the wide stream-K tile's partial block) and their float64 reference for all max-M rows."""
    g = torch.Generator().manual_seed(2000 * N + K)
    d = SimpleNamespace(x=torch.rand((_max_m(N, K), K), generator=g) * 2 - 1,
                        w=(torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5,
                        b=torch.rand((N,), generator=g) - 0.5)
    last = N % 256 or 256
    d.cols = torch.cat([torch.randperm(N - last, generator=g)[:256], torch.arange(N - last, N)])
    d.ref, d.mag = x3_reference(d.x, d.w[d.cols], d.b[d.cols])
    return d


def check_real(y_cols, d, M, K, what=None):
    """The real-valued check: y_cols (M rows of the sampled columns) within x3_bound(K) of the
    float64 reference, relative to sum_k |x_k w_k| + |b|; returns the largest ratio."""
    e = x3_ratio(y_cols, d.ref[:M], d.mag[:M])
    rep = {"M": M, "N": d.w.shape[0], "K": K, "x3_max": float(e.max()), "x3_mean": float(e.mean()),
           "bound": x3_bound(K), "ratio_to_bound": float(e.max()) / x3_bound(K)}
    if what:
        rep["operands"] = what
        x3_report(rep)
    assert np.isfinite(e).all() and e.max() <= x3_bound(K), rep
    return rep


def _drop_k_range(y, x, w, rows, cols, k0):
    """y with the k range [k0, k0 + 32) of the tile rows x cols removed from its sums: what a
    stream-K block that skips one k step, or a fix-up that misses a piece, would leave."""
    y = y.clone()
    xs = x[rows, k0:k0 + 32].to(y.dtype)
    y[rows[:, None], cols[None, :]] -= xs @ w[cols, k0:k0 + 32].to(y.dtype).T
    return y


# ------------------------------------------------------------------------------- CPU-only tests
@pytest.mark.parametrize("N,K", list(TABLE))
def test_integer_operands_are_exact(N, K):
    """The condition that makes the integer cases exact, on this file's operands:
    max_ij sum_k |a_ik| |b_jk| + |bias_j| < 2^24 for the first GEMM and for the second on the
    ReLU'd result; at the one width checked in float64 the fp32 CPU product is the float64 one."""
    r = int_reference(N, K)
    assert 0 < r.mag < 2 ** 24 and r.mag2 < 2 ** 24, (r.mag, r.mag2)
    assert (r.y == r.y.round()).all() and r.y.abs().max() <= r.mag
    if N == K:
        assert r.h.max() > 100          # rows in the hundreds through the second GEMM's scaling
    if (N, K) == (1600, 1600):
        d = int_operands(N, K)
        y64 = d.x.double() @ d.w.double().T + d.b.double()
        assert torch.equal(r.y.double(), y64)
        assert torch.equal(r.y2.double(), torch.relu(y64) @ d.w2.double().T + d.b2.double())


def test_checks_reject_a_dropped_k_range():
    """The checks can fail: at F = 1600, M = 1025, a float64 product stands in for the GPU's
    result and passes the real-valued check; with one 32-k range of one 256 x 128 tile missing
    it is rejected, and the same fault on the integer operands breaks equality."""
    N = K = 1600
    M = 1025
    d = real_operands(N, K)
    rows, tile = torch.arange(256, 512), torch.arange(640, 768)      # tile (mt, nt) = (1, 5)
    hit = torch.isin(d.cols, tile).nonzero()[:, 0]      # the sampled columns inside the tile
    assert len(hit) > 0, "the sampled columns must reach the faulted tile"
    good = d.ref[:M].clone()
    assert check_real(good, d, M, K)["x3_max"] == 0.0
    bad = _drop_k_range(good, d.x[:M], d.w[d.cols], rows, hit, 320)
    with pytest.raises(AssertionError):
        check_real(bad, d, M, K)
    e = x3_ratio(bad, d.ref[:M], d.mag[:M])
    assert e.max() > 100 * x3_bound(K)         # not a marginal miss: ~1e-3 against ~2e-6
    di, ri = int_operands(N, K), int_reference(N, K)
    assert not torch.equal(_drop_k_range(ri.y[:M], di.x[:M], di.w, rows, tile, 320), ri.y[:M])


# ------------------------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def ops():
    from azhip import ops as _ops
    from azhip import _lib
    _lib.lib()
    return _ops


class _Device:
    """Per-width device copies, made on first use and kept for the module: the operands, the
    weights once more in registered storage (az_weights_register: cached P2 planes) and the CPU
    references."""

    def __init__(self):
        self.cache, self.unreg = {}, []

    def reg(self, t):
        t = t.cuda()
        self.unreg.append(_registered(t))
        return t

    def ints(self, N, K):
        if ("i", N, K) not in self.cache:
            d, r = int_operands(N, K), int_reference(N, K)
            assert r.mag < 2 ** 24 and r.mag2 < 2 ** 24
            e = SimpleNamespace(x=d.x.cuda(), w=d.w.cuda(), b=d.b.cuda(), wr=self.reg(d.w),
                                y=r.y.cuda(), h=r.h.cuda())
            if N == K:
                e.w2, e.b2, e.w2r, e.y2 = d.w2.cuda(), d.b2.cuda(), self.reg(d.w2), r.y2.cuda()
            self.cache[("i", N, K)] = e
        return self.cache[("i", N, K)]

    def reals(self, N, K):
        if ("r", N, K) not in self.cache:
            d = real_operands(N, K)
            self.cache[("r", N, K)] = SimpleNamespace(
                x=d.x.cuda(), w=d.w.cuda(), b=d.b.cuda(), wr=self.reg(d.w), cols=d.cols.cuda())
        return self.cache[("r", N, K)]

    def close(self):
        for u in self.unreg:
            u()
        self.cache.clear()


@pytest.fixture(scope="module")
def dev(ops):
    d = _Device()
    yield d
    torch.cuda.synchronize()
    d.close()


def _first_diff(got, ref):
    """(row, column, got, expected) of the first differing element, for the failure message."""
    bad = (got != ref).nonzero()
    if not len(bad):
        return None
    i, j = (int(v) for v in bad[0])
    return i, j, float(got[i, j]), float(ref[i, j]), int(len(bad))


@gpu
@pytest.mark.parametrize("M,N,K", CASES)
def test_linear_integer_exact(ops, dev, M, N, K):
    """ops.linear on integer operands, act = 0 and RELU, registered (P2 planes) and unregistered
    (in-tile split) weights: the whole output equals the CPU product, and the two forms are the
    same bits; for square widths the second GEMM on the first's ReLU output too, as
    output_transform chains them."""
    e = dev.ints(N, K)
    x = e.x[:M]
    for act, ref in ((ops.ACT_NONE, e.y[:M]), (ops.ACT_RELU, e.h[:M])):
        yr = ops.linear(x, e.wr, e.b, act=act)
        yu = ops.linear(x, e.w, e.b, act=act)
        assert torch.equal(yr, ref), ("registered", act, _first_diff(yr, ref))
        assert torch.equal(yu, ref), ("unregistered", act, _first_diff(yu, ref))
        assert torch.equal(yr, yu)
    if N == K:
        y2r = ops.linear(yr, e.w2r, e.b2)
        y2u = ops.linear(yu, e.w2, e.b2)
        assert torch.equal(y2r, e.y2[:M]), ("registered, 2nd", _first_diff(y2r, e.y2[:M]))
        assert torch.equal(y2u, e.y2[:M]), ("unregistered, 2nd", _first_diff(y2u, e.y2[:M]))


@gpu
@pytest.mark.parametrize("M,N,K", CASES)
def test_linear_real_accuracy(ops, dev, M, N, K):
    """ops.linear on uniform operands (both fp16 planes in use): every row of 256 random columns
    and of the last N % 256 or 256 within x3_bound(K) of float64; registered and unregistered
    weights give the same bits."""
    e, d = dev.reals(N, K), real_operands(N, K)
    yr = ops.linear(e.x[:M], e.wr, e.b)
    yu = ops.linear(e.x[:M], e.w, e.b)
    assert torch.equal(yr, yu)
    rep = check_real(yr[:, e.cols].cpu(), d, M, K, what="uniform, widths table")
    print(f"gemm_widths/M{M}_N{N}_K{K}: max err / bound {rep['ratio_to_bound']:.3f}")


PLAN = re.compile(r"csk M=(\d+): am=(\d+) an=(\d+) cycles=(\d+) bf=(\d+) tail=(\d+) at=(\d+) "
                  r"ct=(\d+) bt=(\d+) B=(\d+) pieces=(\d+)")
PLAN_KEYS = ("M", "am", "an", "cycles", "bf", "tail", "at", "ct", "bt", "B", "pieces")


def _child(path):
    """The plan test's child (tuning library, AZ_CSK_PRINT=1): act = 0 GEMMs of the whole table on
    the integer operands, registered weights; a `shape` line on stderr before each launch (the
    library's plan lines follow it), the stream-K shapes' outputs into `path`."""
    from azhip import ops as _ops
    keep, out = [], {}
    for (N, K), rows in TABLE.items():
        d = int_operands(N, K)
        x, w, b = d.x.cuda(), d.w.cuda(), d.b.cuda()
        keep.append((w, _registered(w)))
        for M, cls in rows:
            sys.stderr.write(f"shape M={M} N={N} K={K}\n")
            sys.stderr.flush()
            y = _ops.linear(x[:M], w, b)
            torch.cuda.synchronize()
            if cls == "csk":
                out[f"y_{M}_{N}_{K}"] = y.cpu().numpy()
    np.savez(path, **out)
    print("ok")


@gpu
def test_streamk_plans_cover_the_plan_space(ops, dev, tmp_path):
    """One child process on the tuning library prints the stream-K plan of every launch: exactly
    the table's stream-K shapes take that form, their plans reach every class the block-to-tile
    arithmetic distinguishes, and the child's outputs are the product library's bits.  A planner
    change that empties a class fails here: give the table a new M for it."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == 256, f"the widths table was derived for 256 CUs, this device has {cus}"
    env = dict(os.environ)
    for k in [k for k in env if k.startswith(("AZ_GEMM_", "AZ_CSK", "AZ_NO_", "AZ_SPLITK_",
                                              "AZ_HEADS_", "AZ_AB_LIB"))]:
        env.pop(k)
    env.update(AZ_TUNING_LIB="1", AZ_CSK_PRINT="1")
    path = str(tmp_path / "streamk.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    plans, shape = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"shape M=(\d+) N=(\d+) K=(\d+)", line)
        if m:
            shape = tuple(int(v) for v in m.groups())
            continue
        m = PLAN.match(line)
        if m:
            q = dict(zip(PLAN_KEYS, (int(v) for v in m.groups())))
            assert shape is not None and q["M"] == shape[0], line
            assert shape not in plans, f"two plans for one launch: {shape}"
            plans[shape] = q
    for s in STREAMK:
        assert s in plans, f"{s} did not take the stream-K form"
    assert set(plans) == set(STREAMK), f"unexpected stream-K shapes: {set(plans) - set(STREAMK)}"
    for (M, N, K), q in sorted(plans.items(), key=lambda t: (t[0][1], t[0][0])):
        print(f"gemm_widths/plan N={N}: csk M={M}: " +
              " ".join(f"{k}={q[k]}" for k in PLAN_KEYS[1:]))
        report(f"gemm_widths/plan/M{M}_N{N}_K{K}", **q)
    nt = lambda s: (s[1] + 127) // 128      # noqa: E731
    ntw = lambda s: (s[1] + 255) // 256     # noqa: E731
    assert any(1 < q["an"] < nt(s) for s, q in plans.items()), "no plan with 1 < an < N tiles"
    assert any(q["an"] == nt(s) for s, q in plans.items()), "no plan with one cycle over all N tiles"
    assert any(q["tail"] and 1 < q["at"] < ntw(s) for s, q in plans.items()), \
        "no tail plan with 1 < at < wide tiles"
    assert any(q["tail"] for q in plans.values()) and any(not q["tail"] for q in plans.values())
    assert any(q["pieces"] >= 4 for q in plans.values()), "no tile cut into >= 4 pieces"
    got = np.load(path)
    for M, N, K in STREAMK:
        e = dev.ints(N, K)
        y = ops.linear(e.x[:M], e.wr, e.b)
        assert torch.equal(y, e.y[:M])
        assert np.array_equal(got[f"y_{M}_{N}_{K}"], y.cpu().numpy()), (M, N, K)


# ---------------------------------------------------------------------------------------- heads
# (F, A) of the evaluators (A = n + 1) and (4096, 8), the 16-chunk boundary of the composed /
# rowsw kernels (64 * 16 = 1,024 threads); per F: the first composed-heads size, a 256 x 128
# split-K size and a stream-K size of the table, and at 4096 also 769 (S = 2, the smallest split
# count: its own instantiations of the reduce + heads kernels)
HEADS_FA = [(1024, 5), (1600, 6), (2304, 7), (4096, 9), (4096, 8)]
HEADS_B = {1024: (65, 257, 2049), 1600: (65, 257, 1025), 2304: (65, 257, 769),
           4096: (65, 257, 513, 769)}
HEADS_CASES = [(F, A, B) for F, A in HEADS_FA for B in HEADS_B[F]]


@functools.lru_cache(maxsize=None)
def heads_operands(F):
    """output_transform of width F on uniform rows: +-1 / sqrt(F) weights, small biases; the
    float64 hidden = relu(x W0^T + b0) and y = hidden W2^T + b2 for all rows, the fp32 rows xl
    that az_linear_heads_fwd gets (the float64 hidden, rounded) with their float64 yl, and the
    sampled columns with the magnitudes x3_bound is relative to."""
    Bm = max(HEADS_B[F])
    g = torch.Generator().manual_seed(3000 + F)
    u = lambda *s: torch.rand(s, generator=g) * 2 - 1  # noqa: E731
    d = SimpleNamespace(x=u(Bm, F), w0=u(F, F) / F ** 0.5, w2=u(F, F) / F ** 0.5,
                        b0=u(F) * 0.05, b2=u(F) * 0.05)
    last = F % 256 or 256
    d.cols = torch.cat([torch.randperm(F - last, generator=g)[:256], torch.arange(F - last, F)])
    d.hid64 = torch.relu(d.x.double() @ d.w0.double().T + d.b0.double())
    d.y64 = d.hid64 @ d.w2.double().T + d.b2.double()
    d.hid_mag = d.x.double().abs() @ d.w0[d.cols].double().abs().T + d.b0[d.cols].double().abs()
    d.xl = d.hid64.float()
    d.yl64 = d.xl.double() @ d.w2.double().T + d.b2.double()
    d.yl_mag = d.xl.double().abs() @ d.w2[d.cols].double().abs().T + d.b2[d.cols].double().abs()
    return d


@functools.lru_cache(maxsize=None)
def head_weights(F, A):
    g = torch.Generator().manual_seed(10 * F + A)
    u = lambda *s: torch.rand(s, generator=g) * 2 - 1  # noqa: E731
    return SimpleNamespace(wp=u(A, F) / F ** 0.5, wv=u(1, F) / F ** 0.5, bp=u(A) * 0.5,
                           bv=u(1) * 0.5)


def _heads64(y64, h):
    """Connect4GNN.py:48-57 on float64 rows: (log_softmax, softmax, tanh)."""
    lg = y64 @ h.wp.double().T + h.bp.double()
    lp = lg - torch.logsumexp(lg, 1, keepdim=True)
    v = torch.tanh(y64 @ h.wv.double().T + h.bv.double())[:, 0]
    return lp.numpy(), lp.exp().numpy(), v.numpy()


def _heads_dev(dev, F, A):
    """Device copies for the heads tests: operands, registered W0 / W2, head weights."""
    key = ("h", F)
    if key not in dev.cache:
        d = heads_operands(F)
        dev.cache[key] = SimpleNamespace(
            x=d.x.cuda(), xl=d.xl.cuda(), b0=d.b0.cuda(), b2=d.b2.cuda(), w0=d.w0.cuda(),
            w2=d.w2.cuda(), w0r=dev.reg(d.w0), w2r=dev.reg(d.w2), cols=d.cols.cuda())
    if ("hw", F, A) not in dev.cache:
        h = head_weights(F, A)
        dev.cache[("hw", F, A)] = [t.cuda() for t in (h.wp, h.bp, h.wv, h.bv)]
    return dev.cache[key], dev.cache[("hw", F, A)]


def _nan_outputs(ops, B, F, A, want_y, hidden=True):
    """NaN-filled output tensors and a workspace whose every byte is 0xFF (NaN as fp32)."""
    L = ops._lib.lib()
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    ws = ops.workspace(torch.device("cuda", torch.cuda.current_device()),
                       max(int(L.az_transform_heads_ws_bytes(B, F, A)), 96 << 20))
    ws.fill_(255)
    kw = dict(logp=nan(B, A), pi=nan(B, A), v=nan(B))
    if hidden:
        kw["hidden"] = nan(B, F)
    if want_y:
        kw["y"] = nan(B, F)
    return kw


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts if t is not None)


@gpu
@pytest.mark.parametrize("F,A,B", HEADS_CASES)
def test_transform_heads_at_widths(ops, dev, F, A, B):
    """az_transform_heads_fwd with y formed and y = NULL, registered and unregistered weights,
    every output and the workspace NaN before each call: hidden within x3_bound(F) of float64
    and y of the float64 product of the GPU's own hidden (so the bound is per GEMM); logp, pi, v
    within 1e-5 of the float64 restatement; y = NULL within 2e-6 of the y path; registered and
    unregistered bit-identical; everything finite."""
    e, hw = _heads_dev(dev, F, A)
    d, h = heads_operands(F), head_weights(F, A)
    x = e.x[:B]
    res = {}
    for regd in (True, False):
        w0, w2 = (e.w0r, e.w2r) if regd else (e.w0, e.w2)
        for want_y in (True, False):
            lp, pi, v, y, hid = ops.transform_heads(x, w0, e.b0, w2, e.b2, *hw, want_y=want_y,
                                                    **_nan_outputs(ops, B, F, A, want_y))
            torch.cuda.synchronize()
            assert (y is not None) == want_y and _finite(lp, pi, v, y, hid), (regd, want_y)
            res[(regd, want_y)] = (lp, pi, v, hid, y)
    for want_y in (True, False):
        for a, b in zip(res[(True, want_y)], res[(False, want_y)]):
            assert a is None or torch.equal(a, b), ("registered vs unregistered", want_y)
    lp, pi, v, hid, y = res[(True, True)]
    tl, tp, tv, th, _ = res[(True, False)]
    assert torch.equal(th, hid)
    tag = f"heads_widths/F{F}_A{A}_B{B}"
    eh = x3_ratio(hid[:, e.cols].cpu(), d.hid64[:B][:, d.cols], d.hid_mag[:B])
    yref, ymag = x3_reference(hid.cpu(), d.w2[d.cols], d.b2[d.cols])
    ey = x3_ratio(y[:, e.cols].cpu(), yref, ymag)
    lim = x3_bound(F)
    for name, err in (("hidden", eh), ("y", ey)):
        x3_report({"check": f"{tag}/{name}", "M": B, "N": F, "K": F, "x3_max": float(err.max()),
                   "bound": lim, "ratio_to_bound": float(err.max()) / lim})
        assert err.max() <= lim, (name, float(err.max()), lim)
    olp, opi, ov = _heads64(d.y64[:B], h)
    for pre, (a, b, c) in (("", (lp, pi, v)), ("no_y/", (tl, tp, tv))):
        assert_close(f"{tag}/{pre}logp_vs_fp64", a.cpu().numpy(), olp, 1e-5)
        assert_close(f"{tag}/{pre}pi_vs_fp64", b.cpu().numpy(), opi, 1e-5)
        assert_close(f"{tag}/{pre}v_vs_fp64", c.cpu().numpy(), ov, 1e-5)
    assert_close(f"{tag}/logp_vs_y_path", tl.cpu().numpy(), lp.cpu().numpy(), 2e-6)
    assert_close(f"{tag}/v_vs_y_path", tv.cpu().numpy(), v.cpu().numpy(), 2e-6)


@gpu
@pytest.mark.parametrize("F,A,B", HEADS_CASES)
def test_linear_heads_at_widths(ops, dev, F, A, B):
    """az_linear_heads_fwd (output_transform.2 + heads) on ReLU'd rows, the same matrix of forms:
    y within x3_bound(F) of float64, the heads within 1e-5 of the float64 restatement, y = NULL
    within 2e-6 of the y path, registered and unregistered bit-identical, everything finite."""
    e, hw = _heads_dev(dev, F, A)
    d, h = heads_operands(F), head_weights(F, A)
    x = e.xl[:B]
    res = {}
    for regd in (True, False):
        w2 = e.w2r if regd else e.w2
        for want_y in (True, False):
            lp, pi, v, y = ops.linear_heads(x, w2, e.b2, *hw, want_y=want_y,
                                            **_nan_outputs(ops, B, F, A, want_y, hidden=False))
            torch.cuda.synchronize()
            assert (y is not None) == want_y and _finite(lp, pi, v, y), (regd, want_y)
            res[(regd, want_y)] = (lp, pi, v, y)
    for want_y in (True, False):
        for a, b in zip(res[(True, want_y)], res[(False, want_y)]):
            assert a is None or torch.equal(a, b), ("registered vs unregistered", want_y)
    lp, pi, v, y = res[(True, True)]
    tl, tp, tv, _ = res[(True, False)]
    tag = f"linear_heads_widths/F{F}_A{A}_B{B}"
    ey = x3_ratio(y[:, e.cols].cpu(), d.yl64[:B][:, d.cols], d.yl_mag[:B])
    lim = x3_bound(F)
    x3_report({"check": f"{tag}/y", "M": B, "N": F, "K": F, "x3_max": float(ey.max()),
               "bound": lim, "ratio_to_bound": float(ey.max()) / lim})
    assert ey.max() <= lim, (float(ey.max()), lim)
    olp, opi, ov = _heads64(d.yl64[:B], h)
    for pre, (a, b, c) in (("", (lp, pi, v)), ("no_y/", (tl, tp, tv))):
        assert_close(f"{tag}/{pre}logp_vs_fp64", a.cpu().numpy(), olp, 1e-5)
        assert_close(f"{tag}/{pre}pi_vs_fp64", b.cpu().numpy(), opi, 1e-5)
        assert_close(f"{tag}/{pre}v_vs_fp64", c.cpu().numpy(), ov, 1e-5)
    assert_close(f"{tag}/logp_vs_y_path", tl.cpu().numpy(), lp.cpu().numpy(), 2e-6)
    assert_close(f"{tag}/v_vs_y_path", tv.cpu().numpy(), v.cpu().numpy(), 2e-6)


@gpu
@pytest.mark.parametrize("F,A,B", HEADS_CASES)
def test_transform_heads_integer_exact(ops, dev, F, A, B):
    """az_transform_heads_fwd with y formed, on the integer operands: hidden and y equal the CPU
    products (torch.equal) -- the fused reduce + split of output_transform.0's slabs
    (splitk_reduce_split_kernel) and the P2 GEMM fed from its planes on registered weights, the
    plain reduce and the in-tile split on unregistered ones; the heads are finite."""
    e = dev.ints(F, F)
    _, hw = _heads_dev(dev, F, A)
    x = e.x[:B]
    for regd in (True, False):
        w0, w2 = (e.wr, e.w2r) if regd else (e.w, e.w2)
        lp, pi, v, y, hid = ops.transform_heads(x, w0, e.b, w2, e.b2, *hw,
                                                **_nan_outputs(ops, B, F, A, True))
        torch.cuda.synchronize()
        assert torch.equal(hid, e.h[:B]), (regd, "hidden", _first_diff(hid, e.h[:B]))
        assert torch.equal(y, e.y2[:B]), (regd, "y", _first_diff(y, e.y2[:B]))
        assert not any(bool(torch.isnan(t).any()) for t in (lp, pi, v))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "alphazero-gnn_amd"))
    _child(sys.argv[1])
