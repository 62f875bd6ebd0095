"""CPU checks of the float64 references in tests/gradcheck.py that the HIP backward kernels are
compared with (tests/test_gpu_backward_kernels.py), against torch's own unfold / autograd; and
of the input conditions those GPU tests rest on: integer data whose every sum of |products|
stays below 2^24 (so fp32 is exact in any order), and graphs with the stated degrees."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gradcheck as gc  # noqa: E402

EXACT = 2 ** 24


def _unfold_cols(x, pad):
    """torch's im2col in the kernels' layout: [(b, y, x)][c*9 + kh*3 + kw]."""
    u = torch.nn.functional.unfold(x, 3, padding=pad)           # [B, C*9, Ho*Wo]
    return u.transpose(1, 2).reshape(-1, u.shape[1])


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("H,W", [(3, 3), (4, 5), (5, 4), (7, 7), (5, 5), (6, 6), (8, 8)])
def test_im2col_ref_is_unfold(C, pad, H, W):
    rng = np.random.default_rng(C * 100 + pad * 10 + H + W)
    x = rng.standard_normal((3, C, H, W))
    want = _unfold_cols(torch.from_numpy(x), pad).numpy()
    np.testing.assert_array_equal(gc.im2col3x3_ref(x, pad), want)
    wide = gc.im2col3x3_ref(x, pad, ldc=gc.up4(9 * C + 7))
    np.testing.assert_array_equal(wide[:, :9 * C], want)
    assert not wide[:, 9 * C:].any()
    if C == 1:                                                  # the int8 board form [B,H,W]
        np.testing.assert_array_equal(gc.im2col3x3_ref(x[:, 0], pad), want)


@pytest.mark.parametrize("C", [2, 32])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("H,W", [(3, 3), (4, 4), (5, 4), (7, 7), (5, 5), (6, 6), (8, 8)])
def test_col2im_ref_is_autograd_of_unfold(C, pad, H, W):
    rng = np.random.default_rng(C * 100 + pad * 10 + H + W)
    B = 2
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    ldc = 9 * C + 4
    dcols = np.full((B * Ho * Wo, ldc), np.nan)
    dcols[:, :9 * C] = rng.standard_normal((B * Ho * Wo, 9 * C))
    a = rng.standard_normal((B, C, H, W))
    a[rng.random(a.shape) < 0.2] = 0.0
    x = torch.zeros((B, C, H, W), dtype=torch.float64, requires_grad=True)
    (_unfold_cols(x, pad) * torch.from_numpy(dcols[:, :9 * C])).sum().backward()
    want = (x.grad * torch.from_numpy(a > 0)).permute(0, 2, 3, 1).reshape(B * H * W, C).numpy()
    np.testing.assert_allclose(gc.col2im3x3_drelu_ref(dcols, a, pad), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("B,C,HW", gc.NCHW_PM_SHAPES)
def test_nchw_drelu_to_pm_ref_is_autograd(B, C, HW):
    """s = dropout(relu(pre)) in NCHW from a position-major pre [B*HW][C]: d loss / d pre for
    loss = sum(s * dy) is the kernel's dz."""
    rng = np.random.default_rng(B + C + HW)
    dy = rng.standard_normal((B, C * HW))
    pre0 = rng.standard_normal((B * HW, C))
    pre0[rng.random(pre0.shape) < 0.2] = 0.0
    mask = (rng.random((B, C * HW)) < 0.7).astype(np.uint8)
    for m, scale in ((mask, 2.0), (None, 1.0)):
        pre = torch.from_numpy(pre0).requires_grad_(True)
        y = torch.relu(pre).reshape(B, HW, C).permute(0, 2, 1).reshape(B, C * HW)     # NCHW
        s = y if m is None else y * torch.from_numpy(m.astype(np.float64)) * scale
        (s * torch.from_numpy(dy)).sum().backward()
        got = gc.nchw_drelu_to_pm_ref(dy, y.detach().numpy(), B, C, HW, m, scale)
        np.testing.assert_array_equal(got, pre.grad.numpy())


def test_colsum_ref():
    rng = np.random.default_rng(0)
    X, out = rng.standard_normal((37, 5)), rng.standard_normal(5)
    np.testing.assert_allclose(gc.colsum_ref(X), np.ones(37) @ X, atol=1e-13)
    np.testing.assert_allclose(gc.colsum_ref(X, out, -2.0), np.ones(37) @ X - 2 * out, atol=1e-13)
    assert not np.isnan(gc.colsum_ref(X, np.full(5, np.nan), 0.0)).any()


@pytest.mark.parametrize("A", [1, 8, 10, 26])
@pytest.mark.parametrize("B", [1, 7])
def test_heads_loss_bwd_ref_is_autograd_of_losses(A, B):
    from oracle import torch_ref as R
    rng = np.random.default_rng(A * 10 + B)
    logits = torch.from_numpy(rng.uniform(-8, 8, (B, A))).requires_grad_(True)
    pre = torch.from_numpy(rng.uniform(-2, 2, B)).requires_grad_(True)
    tpi = rng.dirichlet(np.ones(A), B)
    tpi[::3] = 0.0
    tv = rng.uniform(-1, 1, B)
    logp, v = torch.log_softmax(logits, 1), torch.tanh(pre)
    loss = R.losses(logp, v, tpi, tv)
    loss.backward()
    dlog, dv, rows = gc.heads_loss_bwd_ref(logp.detach().numpy(), v.detach().numpy(), tpi, tv)
    np.testing.assert_allclose(dlog, logits.grad.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(dv, pre.grad.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(rows.sum(), loss.item(), rtol=1e-13)
    # B_norm: the same rows as a shard of a 3B batch -- every output scales by B / B_norm
    dlog3, dv3, rows3 = gc.heads_loss_bwd_ref(logp.detach().numpy(), v.detach().numpy(), tpi, tv,
                                              B_norm=3 * B)
    for a3, a1 in ((dlog3, dlog), (dv3, dv), (rows3, rows)):
        np.testing.assert_allclose(a3 * 3, a1, rtol=1e-14, atol=0)


@pytest.mark.parametrize("A,K,B", [(1, 4, 1), (17, 12, 5), (26, 8, 3)])
def test_heads_bwd_ref_is_autograd_of_two_linear_heads(A, K, B):
    rng = np.random.default_rng(A + K + B)
    t = {k: torch.from_numpy(rng.standard_normal(s)).requires_grad_(True)
         for k, s in (("hp", (B, K)), ("hv", (B, K)), ("wp", (A, K)), ("bp", (A,)),
                      ("wv", (1, K)), ("bv", (1,)))}
    dl, dv = rng.standard_normal((B, A)), rng.standard_normal(B)
    F = torch.nn.functional
    out = (F.linear(t["hp"], t["wp"], t["bp"]) * torch.from_numpy(dl)).sum() + \
        (F.linear(t["hv"], t["wv"], t["bv"])[:, 0] * torch.from_numpy(dv)).sum()
    out.backward()
    r = gc.heads_bwd_ref(dl, dv, t["hp"].detach().numpy(), t["hv"].detach().numpy(),
                         t["wp"].detach().numpy(), t["wv"].detach().numpy())
    for k, g in (("wp", "wp"), ("bp", "bp"), ("wv", "wv"), ("bv", "bv"), ("dhp", "hp"),
                 ("dhv", "hv")):
        np.testing.assert_allclose(r[k], t[g].grad.numpy(), rtol=0, atol=1e-12, err_msg=k)


# ------------------------------------------------------------------ exactness of the integer data
def _is_small_int(*arrays):
    return all(np.array_equal(a, np.round(a)) and np.abs(a).max() <= 3 for a in arrays)


@pytest.mark.parametrize("M,N,K", gc.TN_SHAPES + gc.TN_BOARD_SHAPES)
def test_tn_integer_data_is_exact_in_fp32(M, N, K):
    a, b, rows, c0 = gc.tn_inputs(M, N, K)
    assert _is_small_int(a, b, c0) and len(set(rows.tolist())) == K
    a64 = np.abs(a).astype(np.float64)
    for bb in (b[:K, :N], b[rows][:, :N]):
        assert (a64.T @ np.abs(bb) + np.abs(c0)).max() < EXACT


@pytest.mark.parametrize("M,N,K", gc.NN_SHAPES + gc.NN_BOARD_SHAPES)
def test_nn_integer_data_is_exact_in_fp32(M, N, K):
    a, b, g, c0 = gc.nn_inputs(M, N, K)
    assert _is_small_int(a, b, g, c0) and (g == 0).any() and (g < 0).any()
    assert (np.abs(a).astype(np.float64) @ np.abs(b) + np.abs(c0)).max() < EXACT


def test_heads_bwd_cases_cover_every_size_and_form():
    cases = gc.heads_bwd_cases()
    for B in (3, 65):
        sub = [c for c in cases if c[2] == B]
        assert {c[0] for c in sub} == set(gc.HEADS_A)
        assert {c[1] for c in sub} == set(gc.HEADS_K)
        assert {c[3] for c in sub} == set(gc.HEADS_FORMS)
    assert any(c[2] == 1 for c in cases)


@pytest.mark.parametrize("A,K,B,form", gc.heads_bwd_cases())
def test_heads_bwd_integer_data_is_exact_in_fp32(A, K, B, form):
    d = {k: np.abs(v).astype(np.float64) for k, v in gc.heads_bwd_inputs(A, K, B).items()}
    assert _is_small_int(*gc.heads_bwd_inputs(A, K, B).values())
    r = gc.heads_bwd_ref(d["dl"], d["dv"], d["hp"], d["hv"], d["wp"], d["wv"])
    assert max(v.max() for v in r.values()) < EXACT
    assert (r["dhp"] + r["dhv"]).max() < EXACT


@pytest.mark.parametrize("R", gc.COLSUM_R)
@pytest.mark.parametrize("C", gc.COLSUM_C)
def test_colsum_integer_data_is_exact_in_fp32(R, C):
    X, out = gc.colsum_inputs(R, C)
    assert _is_small_int(X, out)
    for beta in gc.COLSUM_BETA:
        assert (np.abs(X).astype(np.float64).sum(0) + abs(beta) * np.abs(out)).max() < EXACT


def test_col2im_integer_data_is_exact_in_fp32():
    for H, W in gc.COL2IM_HW:
        for pad in (0, 1):
            dcols, a = gc.col2im_inputs(3, 64, H, W, pad, 9 * 64 + 4)
            assert _is_small_int(dcols[:, :9 * 64], a) and np.isnan(dcols[:, 9 * 64:]).all()
            assert (a == 0).any() and (a < 0).any()
            # nine taps of at most 3 each
            assert np.abs(gc.col2im3x3_drelu_ref(np.abs(np.nan_to_num(dcols)), np.ones_like(a),
                                                 pad)).max() <= 27 < EXACT


# ------------------------------------------------------------------ the graphs
def _degrees(rowptr):
    return np.diff(rowptr)


def test_mixed_degree_graph_has_the_stated_shape():
    for V in (320, 40):
        rowptr, col = gc.mixed_degree_graph(V)
        deg = _degrees(rowptr)
        assert len(deg) == V and not deg[:10].any() and (deg[10:] > 0).all()
        assert list(deg[10:14]) == [65, 130, 200, 256] and deg.max() == 256
        assert deg[14:].max() <= 6
        dst = np.repeat(np.arange(V), deg)
        assert ((col == dst) & (dst == 20)).any()                      # a self-loop
        assert list(col[rowptr[21]:rowptr[22]]) == [5, 5, 5]           # one source three times
        assert V - 1 not in col and col.min() >= 0                     # never a source
    rowptr, _ = gc.mixed_degree_graph(320)
    E, D = int(rowptr[-1]), int((_degrees(rowptr) > 0).sum())
    assert D == 310 and E < 16 * D                                     # the edges kernel runs


def test_few_destinations_graph_takes_the_dots_path():
    rowptr, col = gc.few_destinations_graph()
    deg = _degrees(rowptr)
    assert {int(v): int(deg[v]) for v in np.flatnonzero(deg)} == {0: 40, 17: 63, 63: 50}
    assert int(rowptr[-1]) >= 16 * 3 and col.max() < 64


def test_one_wide_destination_graph():
    rowptr, col = gc.one_wide_destination_graph()
    deg = _degrees(rowptr)
    assert deg[7] == 300 and np.delete(deg, 7).max() <= 4 and deg.min() >= 1
    assert int(rowptr[-1]) < 16 * 400 and col.max() < 400
