"""Shared helpers of the backward tests (not a test module).

* check_grad / abs_contributions: the gradient criterion of tests/test_gpu_train.py (its
  docstring derives it), used unchanged by tests/test_gpu_grads_ragged.py and
  tests/test_gpu_grads_boards.py, with the targets, boards and autograd references they share.
* Plain float64 references of the backward helper kernels, written from the formulas in
  include/az_hip.h alone (no azhip import): tests/test_backward_refs.py checks them on the CPU
  against torch (unfold / autograd), tests/test_gpu_backward_kernels.py compares the HIP kernels
  with them.
* Generators of the small-integer inputs of the exact-comparison tests.  With values in
  {-3..3} every fp32 product and every partial sum is an integer far below 2^24, so any
  summation order gives the exact result and the comparison needs no tolerance;
  test_backward_refs.py asserts that condition on the very inputs the GPU tests use.
* Builders of the irregular graphs of the GNN layer backward tests.
"""
import numpy as np

U32 = 2.0 ** -24
C_ROUND = 4
MARGINS = {}     # name -> the C_ROUND this tensor needed (reported by test_report_margins)


def check_grad(name, got, ref64, ref32, S=None):
    got = np.asarray(got, np.float64).reshape(-1)
    r = np.asarray(ref64, np.float64).reshape(-1)
    r32 = np.asarray(ref32, np.float64).reshape(-1)
    scale = max(np.abs(r).max(), 1e-30)
    err = np.abs(got - r)
    e_t32 = np.abs(r32 - r).max()
    if S is None:
        assert err.max() <= 10 * e_t32 + 1e-7 * scale, (name, err.max(), e_t32, scale)
        return
    S = np.asarray(S, np.float64).reshape(-1)
    over = err - 10 * e_t32
    need = float(np.max(np.where(over > 0, over / np.maximum(U32 * S, 1e-300), 0.0)))
    MARGINS[name] = need
    assert need <= C_ROUND, (name, err.max(), e_t32, need)


def abs_contributions(run, P):
    """S per parameter of the float64 restatement: |dy|^T |x| (weights) and sum |dy| (biases)
    over every F.linear / F.conv2d that uses it, dy = d loss / d (that call's output).  `run`
    builds the loss from P; the hooks fire during its backward."""
    import torch
    import torch.nn.functional as F
    S = {k: torch.zeros_like(v.detach()) for k, v in P.items()}
    name = {id(v): k for k, v in P.items()}
    lin, conv = F.linear, F.conv2d

    def track(y, x, w, b, kind, kw):
        kw_, kb_ = name.get(id(w)), (name.get(id(b)) if b is not None else None)
        if not y.requires_grad or (kw_ is None and kb_ is None):
            return
        xa = x.detach().abs()

        def hook(dy):
            d = dy.detach().abs()
            if kind == "linear":
                d2, x2 = d.reshape(-1, d.shape[-1]), xa.reshape(-1, xa.shape[-1])
                if kw_:
                    S[kw_] += d2.T @ x2
                if kb_:
                    S[kb_] += d2.sum(0)
            else:
                if kw_:
                    S[kw_] += torch.nn.grad.conv2d_weight(xa, w.shape, d, **kw)
                if kb_:
                    S[kb_] += d.sum((0, 2, 3))
        y.register_hook(hook)

    def lin_t(x, w, b=None):
        y = lin(x, w, b)
        track(y, x, w, b, "linear", {})
        return y

    def conv_t(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        y = conv(x, w, b, stride, padding, dilation, groups)
        track(y, x, w, b, "conv", dict(stride=stride, padding=padding, dilation=dilation,
                                       groups=groups))
        return y
    F.linear, F.conv2d = lin_t, conv_t
    try:
        run(P).backward()
    finally:
        F.linear, F.conv2d = lin, conv
    return {k: v.numpy() for k, v in S.items()}


def check_dot_error(got, ref, bound, tol=1e-6):
    """fp32 dot products vs an fp64 reference: |err| <= tol * sum_k |a_k b_k| per element
    (MI355X_MICROARCH.md: f32 MFMA error ~0.75-3.5e-7 of sum|a.b| up to K=4096)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    worst = (err / (np.asarray(bound, np.float64) + 1e-30)).max()
    assert worst < tol, worst


def cu(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def make_net(kind, W, G=None, dropout=0.0, n=None):
    """Connect4Net (n x n, A = n + 1, F = 64 n^2; default n = 7) or TicTacToeNet (n x n, default
    n = 3) on the weights W, with a two-layer PolicyValueGNN(F) on G.  Connect4 training is
    checked at n = 4..8 (tests/test_gpu_grads_boards.py and, at 7, test_gpu_train.py /
    test_gpu_grads_ragged.py), TicTacToe at 3..5."""
    from types import SimpleNamespace
    from azhip import nets
    if kind == "c4":
        n = 7 if n is None else n
        game = SimpleNamespace(getBoardSize=lambda: (n, n), getActionSize=lambda: n + 1)
        net = nets.Connect4Net(game, {"dropout": dropout}, init=W)
        F = 64 * n * n
    else:
        n = 3 if n is None else n
        game = SimpleNamespace(getBoardSize=lambda: (n, n), getActionSize=lambda: n * n + 1)
        net = nets.TicTacToeNet(game, {}, init=W)
        F = 128 * (n - 2) * (n - 2)
    gnn = nets.PolicyValueGNN(F, 2, init=G) if G is not None else None
    return net, gnn


# ------------------------------------------------------------------- whole-network gradients
def targets(B, A, seed):
    """Training targets: pi rows from Dirichlet(1), z uniform in (-1, 1), fp32."""
    rng = np.random.default_rng(seed)
    return (rng.dirichlet(np.ones(A), B).astype(np.float32),
            rng.uniform(-1, 1, B).astype(np.float32))


def random_boards(n, B, seed):
    return np.random.default_rng(seed).integers(-1, 2, size=(B, n, n)).astype(np.int8)


def ref_grads(fn, W, dtype):
    """Autograd gradients of the loss fn(P) of oracle.torch_ref on the weights W in `dtype`."""
    from oracle import torch_ref as R
    P = R.params(W, dtype)
    fn(P).backward()
    return {k: v.grad.numpy() for k, v in P.items() if v.grad is not None}


def check_cnn_grads(name, net, W, fn, guard=None):
    """net.params.grads against float64 / float32 autograd of fn with S from abs_contributions
    (check_grad's criterion), every tensor of W; `guard(name, g64, S)` sees the float64
    reference before anything is compared."""
    import torch
    from oracle import torch_ref as R
    got = {k: v.cpu().numpy() for k, v in net.params.grads.items()}
    g64, g32 = ref_grads(fn, W, torch.float64), ref_grads(fn, W, torch.float32)
    S = abs_contributions(fn, R.params(W, torch.float64))
    assert set(g64) == set(W)
    if guard is not None:
        guard(name, g64, S)
    for k in g64:
        check_grad(f"{name}/{k}", got[k], g64[k], g32[k], S[k])


MIN_LIVE = 1.0 / 8


def guard_reference(name, g64, S, all_zero=()):
    """A reference that is mostly zeros checks nothing, so before a comparison:

    * every float64 reference tensor has a non-zero maximum;
    * of a tensor other than a bias, counting the elements that any term reaches at all
      (S > 0: an element whose every term |dy| |x| is exactly zero -- a dead ReLU unit, a dropped
      or ReLU-zero feature -- is zero by the network's structure, in the reference and in any
      correct kernel), at most half are exact zeros, and at least MIN_LIVE of the tensor is
      reached.  MIN_LIVE = 1/8: the sparsest gradients here are outer products of ONE row pair
      (a batch of one, the star's single destination), a ReLU'd row (about half live) times a
      ReLU'd row kept with probability 0.7 (about 0.35 live), 0.175 of the tensor.

    `all_zero` names the tensors (by a part of the key) that the case makes identically zero -- the
    attention MLP on a one-edge star, whose single normalised weight is 1 whatever the logit:
    they must be exactly zero instead."""
    for k, g in g64.items():
        g, live = np.asarray(g), np.asarray(S[k]) > 0
        if any(s in k for s in all_zero):
            assert not g.any(), (name, k, "expected identically zero")
            continue
        assert np.abs(g).max() > 0, (name, k, "all-zero reference")
        if k.endswith("bias"):
            continue
        zeros_live = int(((g == 0) & live).sum())
        assert not (g[~live] != 0).any(), (name, k)
        assert 2 * zeros_live <= int(live.sum()), (name, k, zeros_live, int(live.sum()))
        assert live.mean() >= MIN_LIVE, (name, k, float(live.mean()))


# ------------------------------------------------------------------------------ references
def im2col3x3_ref(x, pad, ldc=None):
    """cols[(b,y,x)][c*9+kh*3+kw] = in[b][c][y+kh-pad][x+kw-pad] (0 outside), rows of ldc >= 9C
    floats with a zero tail.  x: [B,C,H,W] (or [B,H,W], C = 1).  float64."""
    x = np.asarray(x, np.float64)
    if x.ndim == 3:
        x = x[:, None]
    B, C, H, W = x.shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    ldc = 9 * C if ldc is None else ldc
    xp = np.zeros((B, C, H + 2 * pad, W + 2 * pad))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    cols = np.zeros((B, Ho, Wo, ldc))
    for c in range(C):
        for kh in range(3):
            for kw in range(3):
                cols[:, :, :, c * 9 + kh * 3 + kw] = xp[:, c, kh:kh + Ho, kw:kw + Wo]
    return cols.reshape(B * Ho * Wo, ldc)


def col2im3x3_drelu_ref(dcols, a, pad):
    """dz[(b,y,x)][c] = sum_{kh,kw} dcols[(b,y-kh+pad,x-kw+pad)][c*9+kh*3+kw] * (a[b][c][y][x] > 0)
    over the taps whose output pixel exists.  dcols: [B*Ho*Wo, ldc] (columns >= 9C are never
    read), a: [B,C,H,W].  float64, [B*H*W, C]."""
    a = np.asarray(a, np.float64)
    B, C, H, W = a.shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    d = np.asarray(dcols, np.float64)[:, :9 * C].reshape(B, Ho, Wo, C, 3, 3)
    dz = np.zeros((B, H, W, C))
    for kh in range(3):
        for kw in range(3):
            for yo in range(Ho):
                y = yo + kh - pad
                if y < 0 or y >= H:
                    continue
                for xo in range(Wo):
                    xx = xo + kw - pad
                    if xx < 0 or xx >= W:
                        continue
                    dz[:, y, xx, :] += d[:, yo, xo, :, kh, kw]
    dz *= (a > 0).transpose(0, 2, 3, 1)
    return dz.reshape(B * H * W, C)


def nchw_drelu_to_pm_ref(dy, y, B, C, HW, mask=None, scale=1.0):
    """dz[b*HW+p][c] = dy[b][c*HW+p] * (mask ? mask*scale : 1) * (y > 0).  float64."""
    g = np.asarray(dy, np.float64).reshape(B, C, HW)
    if mask is not None:
        g = g * (np.asarray(mask).reshape(B, C, HW) != 0) * float(scale)
    g = g * (np.asarray(y, np.float64).reshape(B, C, HW) > 0)
    return g.transpose(0, 2, 1).reshape(B * HW, C)


def colsum_ref(X, out=None, beta=0.0):
    """out[j] = beta*out[j] + sum_i X[i][j]; beta == 0 does not read out.  float64."""
    s = np.asarray(X, np.float64).sum(0)
    return s if beta == 0 else float(beta) * np.asarray(out, np.float64) + s


def heads_loss_bwd_ref(logp, v, tpi, tv, B_norm=None):
    """l = -sum(pi*logp)/Bn + sum((z-v)^2)/Bn:  dlogits = (exp(logp) sum_a pi_a - pi)/Bn,
    dvpre = -2 (z-v)/Bn (1-v^2), loss_rows = [-sum_a pi logp / Bn, (z-v)^2 / Bn].  float64."""
    l, v = np.asarray(logp, np.float64), np.asarray(v, np.float64)
    t, z = np.asarray(tpi, np.float64), np.asarray(tv, np.float64)
    bn = float(B_norm or l.shape[0])
    dlog = (np.exp(l) * t.sum(1, keepdims=True) - t) / bn
    dv = -2.0 * (z - v) / bn * (1.0 - v * v)
    rows = np.stack([-(t * l).sum(1) / bn, (z - v) ** 2 / bn], 1)
    return dlog, dv, rows


def heads_bwd_ref(dl, dv, hp, hv, wp, wv):
    """dwp = dl^T hp, dbp = colsum(dl), dwv = dv^T hv, dbv = sum(dv), dhp = dl wp,
    dhv = dv wv (their sum when the caller fuses both heads into one buffer).  float64."""
    dl, dv = np.asarray(dl, np.float64), np.asarray(dv, np.float64).reshape(-1, 1)
    hp, hv = np.asarray(hp, np.float64), np.asarray(hv, np.float64)
    wp, wv = np.asarray(wp, np.float64), np.asarray(wv, np.float64).reshape(1, -1)
    return {"wp": dl.T @ hp, "bp": dl.sum(0), "wv": dv.T @ hv, "bv": dv.sum(0),
            "dhp": dl @ wp, "dhv": dv @ wv}


# ------------------------------------------------------------------------------ integer data
def ints(rng, shape, lo=-3, hi=3):
    """fp32 integers in {lo..hi}."""
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def up4(n):
    return (n + 3) // 4 * 4


TN_SHAPES = [(32, 9, 1), (32, 9, 1617), (128, 576, 1), (128, 576, 33), (64, 288, 49),
             (256, 64, 1027), (64, 64, 4099)]
NN_SHAPES = [(1, 576, 128), (9, 288, 64), (33, 128, 64), (297, 576, 128)]
TN_EXTRA_ROWS = 37     # rows of the larger B that the b_rows case gathers K of
# The training path's GEMMs at the Connect4 board widths F = 64 n^2, n = 4, 5, 6, 8: F x F
# weight gradients over K rows (the first two split K, with a K tail in the last split), and
# node_update_bwd's B x 2F input gradient with K = F (M = 1: the star's single destination)
TN_BOARD_SHAPES = [(1024, 1024, 257), (1600, 1600, 300), (2304, 2304, 33), (4096, 4096, 1)]
NN_BOARD_SHAPES = [(33, 2048, 1024), (9, 3200, 1600), (1, 4608, 2304), (3, 8192, 4096)]


def tn_inputs(M, N, K):
    """C[M,N] (+)= a^T b: a [K][M], b [K + TN_EXTRA_ROWS][ldb = up4(N)] of which b_rows picks K
    (the plain cases use the first K), c0 [M][N] the accumulator start."""
    rng = np.random.default_rng(1000 * M + 10 * N + K)
    a = ints(rng, (K, M))
    b = ints(rng, (K + TN_EXTRA_ROWS, up4(N)))
    rows = rng.permutation(K + TN_EXTRA_ROWS)[:K].astype(np.int32)
    c0 = ints(rng, (M, N))
    return a, b, rows, c0


def nn_inputs(M, N, K):
    """C[M,N] (+)= a b: a [M][K], b [K][N], g [M][N] the DRELU gate (zeros and negatives),
    c0 the accumulator start."""
    rng = np.random.default_rng(2000 * M + 10 * N + K)
    return ints(rng, (M, K)), ints(rng, (K, N)), ints(rng, (M, N)), ints(rng, (M, N))


HEADS_A = (1, 8, 9, 16, 17, 26, 32)
HEADS_K = (4, 252, 260, 3136, 1600)     # 1600 = 64 * 5^2: six 256-column blocks and a quarter
HEADS_FORMS = ("c4", "ttt", "wonly", "dhonly")


def heads_bwd_cases():
    """(A, K, B, form): every A, every K and every call form with B = 3 and with B = 65, and
    two single-row cases.  The first four K cycle over the seven A; K = 1600 cycles once over
    the four forms with every other A (B = 3: A = 1, 9, 17, 32; B = 65: A = 8, 16, 26, 1), so
    each form and each of the three kernel instances meets the partial seventh block."""
    cases = []
    for bi, B in enumerate((3, 65)):
        for i, A in enumerate(HEADS_A):
            cases.append((A, HEADS_K[(i + bi) % 4], B, HEADS_FORMS[(i + 2 * bi) % 4]))
    for bi, B in enumerate((3, 65)):
        for j, form in enumerate(HEADS_FORMS):
            cases.append((HEADS_A[(2 * j + bi) % len(HEADS_A)], HEADS_K[4], B, form))
    return cases + [(17, 260, 1, "c4"), (1, 4, 1, "ttt")]


def heads_bwd_inputs(A, K, B):
    rng = np.random.default_rng(100000 * A + 100 * K + B)
    return {"dl": ints(rng, (B, A)), "dv": ints(rng, (B,)), "hp": ints(rng, (B, K)),
            "hv": ints(rng, (B, K)), "wp": ints(rng, (A, K)), "wv": ints(rng, (1, K))}


COLSUM_R = (1, 3, 1023, 1025, 4099)
COLSUM_C = (1, 7, 300)
COLSUM_BETA = (0.0, 1.0, -2.0)


def colsum_inputs(R, C):
    rng = np.random.default_rng(10 * R + C)
    return ints(rng, (R, C)), ints(rng, (C,))


COL2IM_HW = ((3, 3), (4, 4), (5, 4), (7, 7), (5, 5), (6, 6), (8, 8))
IM2COL_HW = ((3, 3), (4, 5), (7, 7), (5, 5), (6, 6), (8, 8))
# (B, C, HW) of az_nchw_drelu_to_pm: the TicTacToe heads and conv3, Connect4 7x7, and Connect4's
# conv2 output on 4x4 / 5x5 / 6x6 / 8x8 boards
NCHW_PM_SHAPES = ((1, 512, 1), (3, 128, 4), (5, 64, 49), (3, 64, 16), (2, 64, 25), (2, 64, 36),
                  (1, 64, 64))


def col2im_inputs(B, C, H, W, pad, ldc):
    """dcols [B*Ho*Wo][ldc] with the columns >= 9C set to NaN, a [B,C,H,W] with zeros and
    negatives."""
    rng = np.random.default_rng(((B * 100 + C) * 10 + H) * 100 + W * 10 + pad + ldc)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    dcols = np.full((B * Ho * Wo, ldc), np.nan, np.float32)
    dcols[:, :9 * C] = ints(rng, (B * Ho * Wo, 9 * C))
    return dcols, ints(rng, (B, C, H, W))


# ------------------------------------------------------------------------------ graphs
def csr_from_lists(src_lists):
    deg = np.array([len(s) for s in src_lists], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = np.array([s for l in src_lists for s in l], np.int64)
    return rowptr, col


def mixed_degree_graph(V=320, seed=320):
    """Destination-sorted CSR with: nodes 0..9 without in-edges (D < V); nodes 10..13 with
    in-degrees 65, 130, 200, 256 (the second, third and fourth register slot of
    gnn_agg_bwd_edges_kernel, and the last offset they hold); node 20 with a self-loop; node 21
    with three edges from the same source; every other node 1..6 random sources.  Node V-1 is
    never a source."""
    rng = np.random.default_rng(seed)
    big = {10: 65, 11: 130, 12: 200, 13: 256}
    src = []
    for v in range(V):
        if v < 10:
            src.append([])
        elif v in big:
            src.append(list(rng.integers(0, V - 1, big[v])))
        elif v == 21:
            src.append([5, 5, 5])
        else:
            s = list(rng.integers(0, V - 1, int(rng.integers(1, 7))))
            if v == 20:
                s[0] = 20
            src.append(s)
    return csr_from_lists(src)


def few_destinations_graph(V=64):
    """Three destinations (0, 17, 63) with in-degrees 40, 63, 50: E >= 16 D, the dots / finish
    pair with more than one destination and a compact dst_index."""
    rng = np.random.default_rng(64)
    deg = {0: 40, 17: 63, 63: 50}
    return csr_from_lists([list(rng.integers(0, V, deg[v])) if v in deg else []
                           for v in range(V)])


def one_wide_destination_graph(V=400, wide=7, deg=300):
    """One destination above the 256 register-held edges, the rest with 1..4 (E < 16 D)."""
    rng = np.random.default_rng(400)
    return csr_from_lists([list(rng.integers(0, V, deg if v == wide else int(rng.integers(1, 5))))
                           for v in range(V)])
