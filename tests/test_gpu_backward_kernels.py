"""The backward helper kernels of include/az_hip.h one by one on the MI355X, at ragged shapes,
against the plain float64 references of tests/gradcheck.py (tests/test_backward_refs.py checks
those on the CPU).

Wherever a kernel moves data or sums products the inputs are integers in {-3..3}: every fp32
product and partial sum is then exact in any order (test_backward_refs.py asserts the largest
sum of |products| of each case is below 2^24), the comparison is equality, and one dropped,
doubled or misplaced element fails.  Outputs start as NaN, so an element that is never written
fails too; padding that a kernel must not read is NaN as well.  az_heads_loss_bwd (expf) is
compared against float64 with a bound derived per element.  The shape tables of
tests/gradcheck.py carry the Connect4 4x4 .. 8x8 boards' shapes (C = 64, HW = 16 / 25 / 36 / 64,
K = 1600 in az_heads_bwd), and the transposed GEMM forms run at their widths F = 64 n^2 too."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gradcheck as gc  # noqa: E402
from gradcheck import cu  # noqa: E402

pytestmark = pytest.mark.gpu

AZ_OK, AZ_EINVAL = 0, -1


@pytest.fixture(scope="module")
def L():
    from azhip import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def ops(L):
    from azhip import ops as _ops
    return _ops


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def nans(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def same(got, want):
    """Exact equality with a float64 reference (NaN anywhere fails)."""
    got = got.cpu().numpy().astype(np.float64)
    want = np.asarray(want, np.float64).reshape(got.shape)
    bad = np.flatnonzero(~(got == want).reshape(-1))
    assert bad.size == 0, (bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


# ------------------------------------------------------------------------------ im2col3x3
@pytest.mark.parametrize("kind,C", [("int8", 1), ("fp32", 3), ("fp32", 32)])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("H,W", gc.IM2COL_HW)
def test_im2col3x3(L, kind, C, pad, H, W):
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    for B in (1, 3):
        rng = np.random.default_rng(B * 1000 + C * 10 + H + W + pad)
        if kind == "int8":
            x0 = rng.integers(-1, 2, size=(B, H, W)).astype(np.int8)
        else:
            x0 = gc.ints(rng, (B, C, H, W))
        x = cu(x0)
        for ldc in (gc.up4(9 * C), gc.up4(9 * C + 7)):
            cols = nans(B * Ho * Wo, ldc)
            rc = L.az_im2col3x3(_p(x), int(kind == "int8"), B, C, H, W, pad, ldc, _p(cols), None)
            assert rc == AZ_OK
            same(cols, gc.im2col3x3_ref(x0, pad, ldc))       # the row tail included: exactly 0


# ------------------------------------------------------------------------------ col2im3x3_drelu
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("H,W", gc.COL2IM_HW)
@pytest.mark.parametrize("C", [32, 64])
def test_col2im3x3_drelu(L, pad, H, W, C):
    """dcols' padding columns and a guard of one image's rows after its end are NaN: a tap read
    from a wrong row or column poisons the sum."""
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    for B in (1, 3):
        for ldc in (9 * C, 9 * C + 4):
            d0, a0 = gc.col2im_inputs(B, C, H, W, pad, ldc)
            buf = nans((B + 1) * Ho * Wo, ldc)
            buf[:B * Ho * Wo] = cu(d0)
            a, dz = cu(a0), nans(B * H * W, C)
            rc = L.az_col2im3x3_drelu(_p(buf), ldc, _p(a), B, C, H, W, pad, _p(dz), None)
            assert rc == AZ_OK
            same(dz, gc.col2im3x3_drelu_ref(d0, a0, pad))


# ------------------------------------------------------------------------------ nchw_drelu_to_pm
@pytest.mark.parametrize("B,C,HW", gc.NCHW_PM_SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_nchw_drelu_to_pm(L, B, C, HW, masked):
    rng = np.random.default_rng(B * C + HW)
    dy, y = gc.ints(rng, (B, C * HW)), gc.ints(rng, (B, C * HW))
    assert (y == 0).any() and (y < 0).any()
    m = rng.integers(0, 2, size=(B, C * HW)).astype(np.uint8) if masked else None
    dyd, yd, md, dz = cu(dy), cu(y), cu(m) if masked else None, nans(B * HW, C)
    rc = L.az_nchw_drelu_to_pm(_p(dyd), _p(yd), _p(md), 2.0, B, C, HW, _p(dz), None)
    assert rc == AZ_OK
    same(dz, gc.nchw_drelu_to_pm_ref(dy, y, B, C, HW, m, 2.0))


# ------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("n", [1, 255, 257, 3 * 3136])
def test_mask_scale(L, n):
    rng = np.random.default_rng(n)
    x = gc.ints(rng, (n,))
    m = rng.integers(0, 2, size=n).astype(np.uint8)
    xd, md, y = cu(x), cu(m), nans(n)
    assert L.az_mask_scale(_p(xd), _p(md), 2.0, n, _p(y), None) == AZ_OK
    same(y, x.astype(np.float64) * m * 2.0)


def test_dropout_mask(ops):
    n = 1 << 20
    a = ops.dropout_mask(n, 0.3, 1234, "cuda")
    assert torch.equal(a, ops.dropout_mask(n, 0.3, 1234, "cuda"))          # reproducible
    assert not torch.equal(a, ops.dropout_mask(n, 0.3, 1235, "cuda"))      # seeded
    assert set(a.unique().tolist()) <= {0, 1}
    assert ops.dropout_mask(4099, 0.0, 7, "cuda").min().item() == 1         # p = 0 keeps all
    for p in (0.3, 0.5):
        keep = ops.dropout_mask(n, p, 99, "cuda").double().mean().item()
        six_sigma = 6 * np.sqrt(p * (1 - p) / n)          # 0.0027 and 0.0029
        assert abs(keep - (1 - p)) <= six_sigma, (p, keep)
    # element i depends on (seed, i) alone, not on the launch size
    assert torch.equal(a[:1000], ops.dropout_mask(1000, 0.3, 1234, "cuda"))


# ------------------------------------------------------------------------------ colsum
@pytest.mark.parametrize("R", gc.COLSUM_R)
@pytest.mark.parametrize("C", gc.COLSUM_C)
def test_colsum(ops, R, C):
    X0, out0 = gc.colsum_inputs(R, C)
    for pad in (0, 5):                       # ldx = C and C + 5 (a column slice, NaN beside it)
        wide = nans(R, C + pad)
        wide[:, :C] = cu(X0)
        X = wide[:, :C]
        assert X.stride(0) == C + pad
        for beta in gc.COLSUM_BETA:
            out = nans(C) if beta == 0 else cu(out0)
            ops.colsum(X, out, beta)
            same(out, gc.colsum_ref(X0, out0, beta))


@pytest.mark.parametrize("R", [1, 1025, 4099])
def test_colsum_workspace_size_is_what_the_call_accepts(L, R):
    C = 7
    X0, _ = gc.colsum_inputs(R, C)
    n = int(L.az_colsum_ws_bytes(R, C))
    assert n == ((R + 1023) // 1024) * C * 4
    ws = torch.empty((n,), dtype=torch.uint8, device="cuda")
    X, out = cu(X0), nans(C)
    assert L.az_colsum(_p(X), R, C, C, _p(out), 0.0, _p(ws), n, None) == AZ_OK
    same(out, gc.colsum_ref(X0))
    # az_last_error is per thread: the rejected call runs on a thread of its own, so the main
    # thread keeps the empty message tests/test_lib_abi.py expects whatever the test order
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(
        (L.az_colsum(_p(X), R, C, C, _p(out), 0.0, _p(ws), n - 1, None), L.az_last_error())))
    t.start()
    t.join()
    assert seen[0][0] == AZ_EINVAL and b"workspace" in seen[0][1]


# ------------------------------------------------------------------------------ heads_bwd
def _heads_bwd_case(ops, A, K, B, form, ldh=None):
    d0 = gc.heads_bwd_inputs(A, K, B)
    ref = gc.heads_bwd_ref(d0["dl"], d0["dv"], d0["hp"], d0["hp"] if form == "c4" else d0["hv"],
                           d0["wp"], d0["wv"])
    ldh = ldh or K

    def rows(a):                             # [B][K] in rows of ldh floats, NaN behind each row
        t = nans(B, ldh)
        t[:, :K] = cu(a)
        return t[:, :K]
    hp = rows(d0["hp"])
    hv = hp if form == "c4" else rows(d0["hv"])
    dl, dv, wp, wv = (cu(d0[k]) for k in ("dl", "dv", "wp", "wv"))
    grads = None
    if form != "dhonly":
        grads = {"wp": nans(A, K), "bp": nans(A), "wv": nans(1, K), "bv": nans(1)}
    dh_buf = dhv_buf = dh = dhv = None
    if form != "wonly":
        dh_buf = nans(B, ldh)
        dh = dh_buf[:, :K]
        if form != "c4":
            dhv_buf = nans(B, ldh)
            dhv = dhv_buf[:, :K]
    ops.heads_bwd(dl, dv, hp, wp, wv, hv=hv, grads=grads, dh=dh, dhv=dhv)
    if grads is not None:
        for k in ("wp", "bp", "wv", "bv"):
            same(grads[k], ref[k])
    if form == "c4":
        same(dh, ref["dhp"] + ref["dhv"])
    elif form != "wonly":
        same(dh, ref["dhp"])
        same(dhv, ref["dhv"])
    for buf in (dh_buf, dhv_buf):            # nothing written behind a row
        if buf is not None and ldh > K:
            assert torch.isnan(buf[:, K:]).all()


@pytest.mark.parametrize("A,K,B,form", gc.heads_bwd_cases())
def test_heads_bwd(ops, A, K, B, form):
    """c4: hv is hp and one fused dh; ttt: separate hp / hv, dh and dhv; wonly: weight grads
    only; dhonly: dh and dhv only.  A <= 8 / <= 16 / <= 32 are three kernel instances; K = 252,
    260 and 1600 (a 5x5 Connect4 board) end inside a 256-column block."""
    _heads_bwd_case(ops, A, K, B, form)


def test_heads_bwd_with_padded_rows(ops):
    """ldhp = ldhv = lddhp = K + 8: the floats behind every row are NaN on input and stay NaN on
    output."""
    _heads_bwd_case(ops, 26, 252, 3, "ttt", ldh=260)
    _heads_bwd_case(ops, 9, 260, 65, "c4", ldh=268)


# ------------------------------------------------------------------------------ heads_loss_bwd
@pytest.mark.parametrize("A", [1, 8, 10, 26])
@pytest.mark.parametrize("B", [1, 257])
def test_heads_loss_bwd(ops, A, B):
    """Per element against float64 of the same fp32 inputs:
        dlogits  8 u (exp(l) sum(pi) + |pi|) / Bn      dvpre  8 u |2 (z - v) / Bn|
        policy loss row  8 u sum|pi l| / Bn            value loss row  8 u (z - v)^2 / Bn
    u = 2^-24.  8 covers the at most five roundings of each formula plus expf's 1 ulp."""
    rng = np.random.default_rng(A * 1000 + B)
    logits = rng.uniform(-8, 8, (B, A))
    logp = (logits - np.log(np.exp(logits).sum(1, keepdims=True))).astype(np.float32)
    v = np.tanh(rng.uniform(-2, 2, B)).astype(np.float32)
    tpi = rng.dirichlet(np.ones(A), B).astype(np.float32)
    tpi[::5] = 0.0
    tv = rng.uniform(-1, 1, B).astype(np.float32)
    u8 = 8 * gc.U32
    l64, t64 = logp.astype(np.float64), tpi.astype(np.float64)
    d = tv.astype(np.float64) - v.astype(np.float64)
    for B_norm in (B, 3 * B):
        dlog, dv, rows = gc.heads_loss_bwd_ref(logp, v, tpi, tv, B_norm)
        bounds = {"dlogits": u8 * (np.exp(l64) * t64.sum(1, keepdims=True) + np.abs(t64)) / B_norm,
                  "dvpre": u8 * np.abs(2 * d / B_norm),
                  "loss_pi": u8 * np.abs(t64 * l64).sum(1) / B_norm,
                  "loss_v": u8 * d * d / B_norm}
        for with_rows in (True, False):
            lrows = nans(B, 2) if with_rows else None
            gl, gv = ops.heads_loss_bwd(cu(logp), cu(v), cu(tpi), cu(tv), B_norm=B_norm,
                                        loss_rows=lrows)
            got = {"dlogits": (gl, dlog), "dvpre": (gv, dv)}
            if with_rows:
                got["loss_pi"] = (lrows[:, 0], rows[:, 0])
                got["loss_v"] = (lrows[:, 1], rows[:, 1])
            for k, (g, r) in got.items():
                err = np.abs(g.cpu().numpy().astype(np.float64) - r)
                worst = float((err / np.maximum(bounds[k], 1e-300)).max()) if err.max() > 0 else 0.0
                print(f"heads_loss_bwd A={A} B={B} Bn={B_norm} {k}: {8 * worst:.2f} u of 8")
                assert (err <= bounds[k]).all(), (k, B_norm, 8 * worst)


# ------------------------------------------------------------------------------ transposed GEMMs
def _desc(ops, M, N, K, A, lda, akm, Bm, ldb, C, ldc, beta=0.0, b_rows=None, act=0, G=None):
    d = ops.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A, d.lda, d.a_kmajor = A.data_ptr(), lda, akm
    d.B, d.ldb, d.b_kmajor = Bm.data_ptr(), ldb, 0
    d.b_rows = b_rows.data_ptr() if b_rows is not None else None
    d.act = act
    if G is not None:
        d.G, d.ldg = G.data_ptr(), G.stride(0)
    d.beta = beta
    d.C, d.ldc = C.data_ptr(), ldc
    return d


def _run(ops, d, split):
    """split: a workspace that lets az_gemm_f32 split K; else ws = NULL, i.e. one split."""
    ops.gemm(d, torch.device("cuda", torch.cuda.current_device()) if split else None)
    assert bool(d.ws) == split


def _tn_operands(M, N, K):
    a0, b0, rows0, c0 = gc.tn_inputs(M, N, K)
    b0 = b0.copy()
    b0[:, N:] = np.nan                         # ldb > N: the floats behind a row are not B
    return a0, b0, rows0, c0


@pytest.mark.parametrize("M,N,K", gc.TN_SHAPES)
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("split", [True, False])
def test_gemm_tn_ragged(ops, M, N, K, beta, split):
    """C = a^T b (+ C): weight gradients with K = B H W -- 1, odd, a K tail in the last split."""
    a0, b0, _, c0 = _tn_operands(M, N, K)
    a, b = cu(a0), cu(b0)
    C = cu(c0) if beta else nans(M, N)
    _run(ops, _desc(ops, M, N, K, a, M, 0, b, b.stride(0), C, N, beta=beta), split)
    ref = a0.astype(np.float64).T @ b0[:K, :N].astype(np.float64) + beta * c0
    same(C, ref)


@pytest.mark.parametrize("M,N,K", gc.TN_SHAPES)
def test_gemm_tn_into_a_column_half(ops, M, N, K):
    """ldc = 2N with C offset by N columns (the halves of gate_w / upd_w1 in node_update_bwd):
    the other half keeps its sentinel."""
    a0, b0, _, _ = _tn_operands(M, N, K)
    a, b = cu(a0), cu(b0)
    full = torch.full((M, 2 * N), 7777.0, device="cuda")
    C = full[:, N:]
    _run(ops, _desc(ops, M, N, K, a, M, 0, b, b.stride(0), C, 2 * N), True)
    same(C, a0.astype(np.float64).T @ b0[:K, :N].astype(np.float64))
    assert (full[:, :N] == 7777.0).all()


@pytest.mark.parametrize("M,N,K", gc.TN_SHAPES)
def test_gemm_tn_gathered_b_rows(ops, M, N, K):
    """b_rows: K rows picked, unsorted, from a larger N-major B."""
    a0, b0, rows0, c0 = _tn_operands(M, N, K)
    a, b, rows = cu(a0), cu(b0), cu(rows0)
    for beta, split in ((0.0, True), (1.0, False)):
        C = cu(c0) if beta else nans(M, N)
        _run(ops, _desc(ops, M, N, K, a, M, 0, b, b.stride(0), C, N, beta=beta, b_rows=rows),
             split)
        same(C, a0.astype(np.float64).T @ b0[rows0][:, :N].astype(np.float64) + beta * c0)


@pytest.mark.parametrize("M,N,K", gc.NN_SHAPES)
@pytest.mark.parametrize("form", ["plain", "drelu", "beta1"])
def test_gemm_nn_ragged(ops, M, N, K, form):
    """C = a b with an N-major b (input gradients), the DRELU epilogue and accumulation."""
    a0, b0, g0, c0 = gc.nn_inputs(M, N, K)
    a, b = cu(a0), cu(b0)
    ref = a0.astype(np.float64) @ b0.astype(np.float64)
    if form == "drelu":
        ref = ref * (g0 > 0)
    elif form == "beta1":
        ref = ref + c0
    for split in (True, False):
        C = cu(c0) if form == "beta1" else nans(M, N)
        d = _desc(ops, M, N, K, a, K, 1, b, N, C, N, beta=1.0 if form == "beta1" else 0.0,
                  act=ops.ACT_DRELU if form == "drelu" else 0, G=cu(g0) if form == "drelu" else None)
        _run(ops, d, split)
        same(C, ref)


# ------------------------------------------------- the transposed forms at the board widths
EXACT = 2 ** 24
WS_BYTES = 256 << 20           # ops.workspace's default, what _run(split=True) hands the library


def tn_planned_splits(M, N, K, ws_bytes=WS_BYTES):
    """plan()'s rule (csrc/az_gemm.hip) for the 64 x 64 x 32 register tile every transposed form
    takes, restated: with fewer than 1024 tiles K is cut into min(ceil(1024 / tiles), 8,
    K // 128) parts (at least four 32-k steps each) whose M x N slabs fit the workspace; each
    part is a whole number of k steps, so the count is ceil(K / kc)."""
    tiles = -(-M // 64) * -(-N // 64)
    S = min(-(-1024 // tiles), 8, K // 128) if tiles < 1024 else 1
    while S > 1 and S * M * N * 4 > ws_bytes:
        S -= 1
    if S <= 1:
        return 1, K
    kc = -(-(-(-K // S)) // 32) * 32
    return -(-K // kc), kc


@functools.lru_cache(maxsize=None)
def _tn_board_case(M, N, K):
    """Operands of one board-width TN shape and the float64 products of the plain and the
    gathered form, computed once; the exactness condition is asserted on them."""
    a0, b0, rows0, c0 = _tn_operands(M, N, K)
    a64 = a0.astype(np.float64).T
    plain = a64 @ b0[:K, :N].astype(np.float64)
    gathered = a64 @ b0[rows0][:, :N].astype(np.float64)
    for bb in (b0[:K, :N], b0[rows0][:, :N]):
        assert (np.abs(a64) @ np.abs(bb).astype(np.float64) + np.abs(c0)).max() < EXACT
    return a0, b0, rows0, c0, plain, gathered


@pytest.mark.parametrize("M,N,K", gc.TN_BOARD_SHAPES)
@pytest.mark.parametrize("form", ["beta0", "beta1", "column_half", "b_rows"])
def test_gemm_tn_at_board_widths(ops, M, N, K, form):
    """C = a^T b, the F x F weight gradients of az_mlp2_bwd / node_update_bwd at F = 64 n^2 for
    the 4x4 .. 8x8 Connect4 boards, with a split workspace: plain with beta 0 and 1, into a column
    half (ldc = 2N, C offset by N columns, the other half keeps its sentinel), and with b_rows
    gathering K unsorted rows of a larger B.  Integer operands in {-3..3}: every sum is below 2^24
    (asserted on the CPU product), so the fp32 result equals the float64 product.

    The library does not report the split count of a launch, so the test restates plan()'s rule
    (tn_planned_splits) and asserts the class it gives: (1024, 1024, 257) and (1600, 1600, 300)
    are cut in two with a K tail in the second part, (2304, 2304, 33) and (4096, 4096, 1) are
    not cut; the count is printed."""
    S, kc = tn_planned_splits(M, N, K)
    print(f"gemm_tn_board/M{M}_N{N}_K{K}: planned splits {S}, {kc} k per split")
    assert (S, kc) == {257: (2, 160), 300: (2, 160), 33: (1, 33), 1: (1, 1)}[K]
    assert S == 1 or 0 < K - (S - 1) * kc < kc            # the last part is a partial one
    a0, b0, rows0, c0, plain, gathered = _tn_board_case(M, N, K)
    a, b = cu(a0), cu(b0)
    if form == "column_half":
        full = torch.full((M, 2 * N), 7777.0, device="cuda")
        C = full[:, N:]
        _run(ops, _desc(ops, M, N, K, a, M, 0, b, b.stride(0), C, 2 * N), True)
        same(C, plain)
        assert bool((full[:, :N] == 7777.0).all())
        return
    beta = 1.0 if form == "beta1" else 0.0
    C = cu(c0) if beta else nans(M, N)
    rows = cu(rows0) if form == "b_rows" else None
    _run(ops, _desc(ops, M, N, K, a, M, 0, b, b.stride(0), C, N, beta=beta, b_rows=rows), True)
    same(C, (gathered if form == "b_rows" else plain) + beta * c0)


@functools.lru_cache(maxsize=None)
def _nn_board_case(M, N, K):
    a0, b0, g0, c0 = gc.nn_inputs(M, N, K)
    assert (g0 == 0).any() and (g0 < 0).any()
    assert (np.abs(a0).astype(np.float64) @ np.abs(b0) + np.abs(c0)).max() < EXACT
    return a0, b0, g0, c0, a0.astype(np.float64) @ b0.astype(np.float64)


@pytest.mark.parametrize("M,N,K", gc.NN_BOARD_SHAPES)
@pytest.mark.parametrize("form", ["plain", "drelu", "beta1"])
def test_gemm_nn_at_board_widths(ops, M, N, K, form):
    """C = a b with an N-major b at N = 2F, K = F: node_update_bwd's dc = du1pre Wu1 + dgpre Wg
    on the four boards (M = 1 is the star's single destination), plain, through the DRELU gate
    (zeros and negatives in it) and accumulating, each with and without a split workspace.
    Integer operands, sums below 2^24 (asserted), equality with the float64 product."""
    a0, b0, g0, c0, ref = _nn_board_case(M, N, K)
    if form == "drelu":
        ref = ref * (g0 > 0)
    elif form == "beta1":
        ref = ref + c0
    a, b = cu(a0), cu(b0)
    G = cu(g0) if form == "drelu" else None
    for split in (True, False):
        C = cu(c0) if form == "beta1" else nans(M, N)
        d = _desc(ops, M, N, K, a, K, 1, b, N, C, N, beta=1.0 if form == "beta1" else 0.0,
                  act=ops.ACT_DRELU if form == "drelu" else 0, G=G)
        _run(ops, d, split)
        same(C, ref)


@pytest.mark.parametrize("form,M,N,K", [("tn", 64, 64, 4099), ("tn", 32, 9, 1617),
                                        ("nn", 297, 576, 128), ("tn", 1600, 1600, 300),
                                        ("nn", 9, 3200, 1600)])
def test_gemm_transposed_forms_real_valued(ops, form, M, N, K):
    """Uniform +-1 data against float64 at 1e-6 of sum |a b|: a reduced-precision path would pass
    the integer cases above and below.  The last two are a 5x5 Connect4 board's F x F weight
    gradient (two K splits) and its node_update_bwd input gradient."""
    rng = np.random.default_rng(M + N + K)
    b0 = rng.uniform(-1, 1, (K, gc.up4(N))).astype(np.float32)
    C = nans(M, N)
    if form == "tn":
        a0 = rng.uniform(-1, 1, (K, M)).astype(np.float32)
        _run(ops, _desc(ops, M, N, K, cu(a0), M, 0, cu(b0), b0.shape[1], C, N), True)
        a64 = a0.astype(np.float64).T
    else:
        a0 = rng.uniform(-1, 1, (M, K)).astype(np.float32)
        _run(ops, _desc(ops, M, N, K, cu(a0), K, 1, cu(b0), b0.shape[1], C, N), True)
        a64 = a0.astype(np.float64)
    b64 = b0[:, :N].astype(np.float64)
    gc.check_dot_error(C.cpu().numpy(), a64 @ b64, np.abs(a64) @ np.abs(b64))
