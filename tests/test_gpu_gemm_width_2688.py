"""output_transform's GEMMs at N = K = 2688, the width of the standard 7 x 6 Connect4 board
(F = 64 * 7 * 6), through ops.linear and az_transform_heads_fwd -- tests/test_gpu_gemm_widths.py's
checks at the one width its table lacks.  2688 = 21 column tiles of 128 = 10.5 wide tiles of 256
(the wide stream-K tile's last block is partial), 84 k-steps of 32.

The Ms are one per dispatch class of launch_x3, derived from its conditions for 256 CUs and the
default workspace (the derivation the header of tests/test_gpu_gemm_widths.py describes; `_class`
below restates it and a CPU test holds the table to it):
  * M <= 256, 128 x 128 tiles:  65 -> 21 tiles, S = 8 (kc = 352);  129 -> 42 tiles, S = 6;
  * M > 256, 256 x 128 tiles, split-K:  257 -> 42 tiles, S = 6;  769 -> 84 tiles, S = 3
    (252 blocks = 98 % of a round: not stream-K);
  * stream-K (>= 64 tiles, the split-K grid below 90 % of its last round):  1025 -> 105 tiles,
    S = 2 -> 210 blocks = 82 %, a tail row of 1 (rows_last <= 128 runs as wide tiles);  1200 -> the
    same 105 tiles, rows_last = 176 > 128: no tail row.

Integer operands (x in {-1, 0, 1}, w in {-2 .. 2}, bias in {-3 .. 3}) make every partial sum an
exactly representable integer, so the whole output equals the CPU product in every form; real
operands fill the low fp16 planes and are held to x3_bound(K) of float64 on 256 random columns plus
the last (partial) 256-column block."""
import functools
from types import SimpleNamespace

import pytest

from test_gpu_gemm_widths import _first_diff, _nan_outputs
from test_gpu_kernels import _registered, x3_bound, x3_ratio, x3_reference, x3_report

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

N = K = 2688
A = 8
TABLE = [(65, "s128"), (129, "s128"), (257, "s256"), (769, "s256"), (1025, "csk"), (1200, "csk")]
MAX_M = max(M for M, _ in TABLE)


def _class(M, N, K, cus=256):
    """launch_x3's choice: 128 x 128 split-K tiles, 256 x 128 split-K tiles or stream-K, with the
    split count (the default workspace never limits it at these sizes)."""
    bm = 256 if M > 256 else 128
    tiles = -(-M // bm) * -(-N // 128)
    S = min(256 // tiles, 8) if tiles < 256 else 1
    while S > 1 and K // S < 256:
        S -= 1
    kc = -(-(-(-K // S)) // 32) * 32 if S > 1 else K
    S = -(-K // kc) if S > 1 else 1
    if bm == 128:
        return "s128", S
    blocks = tiles * S
    rounds = -(-blocks // cus)
    iters = tiles * -(-K // 32)
    if tiles >= 64 and blocks / (rounds * cus) < 0.9 and iters // min(cus, iters) >= 8:
        return "csk", S
    return "s256", S


def test_table_holds_one_m_per_dispatch_class():
    """The table against the restated dispatch rule: the classes, two split counts among the
    256 x 128 split-K sizes, the smallest stream-K M, and a tail and a no-tail stream-K row."""
    got = {M: _class(M, N, K) for M, _ in TABLE}
    assert [got[M][0] for M, _ in TABLE] == [c for _, c in TABLE]
    assert got[65] == ("s128", 8) and got[129] == ("s128", 6)
    assert got[257] == ("s256", 6) and got[769] == ("s256", 3)
    assert min(M for M in range(65, 1300) if _class(M, N, K)[0] == "csk") == 1025
    tail = lambda M: -(-M // 256) > 1 and (M - 1) % 256 + 1 <= 128      # noqa: E731
    assert tail(1025) and not tail(1200)


@functools.lru_cache(maxsize=None)
def int_operands():
    g = torch.Generator().manual_seed(1000 * N + K)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    d = SimpleNamespace(x=ri(-1, 1, MAX_M, K), w=ri(-2, 2, N, K), b=ri(-3, 3, N),
                        w2=ri(-2, 2, N, K), b2=ri(-3, 3, N))
    d.y = d.x @ d.w.T + d.b
    d.mag = float((d.x.abs() @ d.w.abs().T + d.b.abs()).max())
    d.h = torch.relu(d.y)
    d.y2 = d.h @ d.w2.T + d.b2
    d.mag2 = float((d.h @ d.w2.abs().T + d.b2.abs()).max())
    return d


@functools.lru_cache(maxsize=None)
def real_operands():
    g = torch.Generator().manual_seed(2000 * N + K)
    d = SimpleNamespace(x=torch.rand((MAX_M, K), generator=g) * 2 - 1,
                        w=(torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5,
                        b=torch.rand((N,), generator=g) - 0.5)
    last = N % 256 or 256
    assert last == 128
    d.cols = torch.cat([torch.randperm(N - last, generator=g)[:256], torch.arange(N - last, N)])
    d.ref, d.mag = x3_reference(d.x, d.w[d.cols], d.b[d.cols])
    return d


def test_integer_operands_are_exact_at_2688():
    """sum_k |a_k b_k| + |bias| < 2^24 for both GEMMs, so every partial sum in every summation
    order is an exactly representable integer; the fp32 CPU product is the float64 one."""
    d = int_operands()
    assert 0 < d.mag < 2 ** 24 and 0 < d.mag2 < 2 ** 24, (d.mag, d.mag2)
    assert (d.y == d.y.round()).all() and d.h.max() > 100
    y64 = d.x[:70].double() @ d.w.double().T + d.b.double()
    assert torch.equal(d.y[:70].double(), y64)
    assert torch.equal(d.y2[:70].double(), torch.relu(y64) @ d.w2.double().T + d.b2.double())


@pytest.fixture(scope="module")
def ops():
    from azhip import ops as _ops
    from azhip import _lib
    _lib.lib()
    return _ops


@pytest.fixture(scope="module")
def dev(ops):
    """Device copies, the weights once more in registered storage (cached P2 planes)."""
    unreg = []

    def reg(t):
        t = t.cuda()
        unreg.append(_registered(t))
        return t

    d, r = int_operands(), real_operands()
    assert d.mag < 2 ** 24 and d.mag2 < 2 ** 24
    g = torch.Generator().manual_seed(10 * N + A)
    u = lambda *s: torch.rand(s, generator=g) * 2 - 1  # noqa: E731
    e = SimpleNamespace(
        x=d.x.cuda(), w=d.w.cuda(), b=d.b.cuda(), wr=reg(d.w), w2=d.w2.cuda(), b2=d.b2.cuda(),
        w2r=reg(d.w2), y=d.y.cuda(), h=d.h.cuda(), y2=d.y2.cuda(),
        rx=r.x.cuda(), rw=r.w.cuda(), rb=r.b.cuda(), rwr=reg(r.w), cols=r.cols.cuda(),
        hw=[t.cuda() for t in (u(A, N) / N ** 0.5, u(A) * 0.5, u(1, N) / N ** 0.5, u(1) * 0.5)])
    yield e
    torch.cuda.synchronize()
    for f in unreg:
        f()


@gpu
@pytest.mark.parametrize("M,cls", TABLE)
def test_linear_integer_exact_at_2688(ops, dev, M, cls):
    """ops.linear on integer operands, act = 0 and RELU, registered (P2 planes) and unregistered
    (in-tile split) weights: the whole output equals the CPU product; the second GEMM on the
    first's ReLU output too, as output_transform chains them."""
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    e = dev
    x = e.x[:M]
    for act, ref in ((ops.ACT_NONE, e.y[:M]), (ops.ACT_RELU, e.h[:M])):
        yr = ops.linear(x, e.wr, e.b, act=act)
        yu = ops.linear(x, e.w, e.b, act=act)
        assert torch.equal(yr, ref), (cls, "registered", act, _first_diff(yr, ref))
        assert torch.equal(yu, ref), (cls, "unregistered", act, _first_diff(yu, ref))
    y2r = ops.linear(yr, e.w2r, e.b2)
    y2u = ops.linear(yu, e.w2, e.b2)
    assert torch.equal(y2r, e.y2[:M]), (cls, "registered, 2nd", _first_diff(y2r, e.y2[:M]))
    assert torch.equal(y2u, e.y2[:M]), (cls, "unregistered, 2nd", _first_diff(y2u, e.y2[:M]))


@gpu
@pytest.mark.parametrize("M,cls", TABLE)
def test_transform_heads_integer_exact_at_2688(ops, dev, M, cls):
    """az_transform_heads_fwd with y formed, on the integer operands: hidden and y equal the CPU
    products on registered and unregistered weights; the heads are finite."""
    e = dev
    x = e.x[:M]
    for regd in (True, False):
        w0, w2 = (e.wr, e.w2r) if regd else (e.w, e.w2)
        lp, pi, v, y, hid = ops.transform_heads(x, w0, e.b, w2, e.b2, *e.hw,
                                                **_nan_outputs(ops, M, N, A, True))
        torch.cuda.synchronize()
        assert torch.equal(hid, e.h[:M]), (cls, regd, "hidden", _first_diff(hid, e.h[:M]))
        assert torch.equal(y, e.y2[:M]), (cls, regd, "y", _first_diff(y, e.y2[:M]))
        assert not any(bool(torch.isnan(t).any()) for t in (lp, pi, v))


@gpu
@pytest.mark.parametrize("M,cls", TABLE)
def test_linear_real_accuracy_at_2688(ops, dev, M, cls):
    """ops.linear on uniform operands (both fp16 planes in use): every row of 256 random columns
    and of the last 128 (the partial wide block) within x3_bound(K) of float64; registered and
    unregistered weights give the same bits."""
    import numpy as np
    e, d = dev, real_operands()
    yr = ops.linear(e.rx[:M], e.rwr, e.rb)
    yu = ops.linear(e.rx[:M], e.rw, e.rb)
    assert torch.equal(yr, yu)
    err = x3_ratio(yr[:, e.cols].cpu(), d.ref[:M], d.mag[:M])
    rep = {"M": M, "N": N, "K": K, "x3_max": float(err.max()), "x3_mean": float(err.mean()),
           "bound": x3_bound(K), "ratio_to_bound": float(err.max()) / x3_bound(K),
           "operands": "uniform, width 2688"}
    x3_report(rep)
    print(f"gemm_width_2688/M{M}_{cls}: max err / bound {rep['ratio_to_bound']:.3f}")
    assert np.isfinite(err).all() and err.max() <= x3_bound(K), rep
