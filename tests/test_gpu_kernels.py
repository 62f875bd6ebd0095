"""Kernel-level parity on the MI355X: every C-ABI entry point against the oracle (numpy
float64 restatement of the reference) or, for plain GEMM shapes, a torch fp32 reference."""
import numpy as np
import pytest

from conftest import assert_close, golden, split_weights
from gradcheck import check_dot_error  # noqa: F401  (shared with the backward tests)

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    from azhip import ops as _ops
    from azhip import _lib
    _lib.lib()
    return _ops


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("M,N,K", [(1, 3136, 3136), (3, 37, 64), (8, 128, 6272), (64, 128, 3136),
                                   (512, 3136, 3136), (130, 70, 48), (4096, 256, 64),
                                   (1, 7, 4096), (2, 1001, 260), (5, 300, 1024), (1, 33, 4100),
                                   (32768, 1024, 1024), (3, 3136, 3136), (8, 3136, 3136),
                                   (6, 1000, 2500)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_vs_torch(ops, M, N, K, act):
    g = torch.Generator().manual_seed(M * 7 + N + K + act)
    x = torch.rand((M, K), generator=g) * 2 - 1
    w = (torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5
    b = torch.rand((N,), generator=g) - 0.5
    ref = x.double() @ w.double().T + b.double()
    ref = [lambda t: t, torch.relu, torch.sigmoid][act](ref)
    y = ops.linear(x.cuda(), w.cuda(), b.cuda(), act=act).cpu()
    bound = x.double().abs() @ w.double().abs().T + b.double().abs()
    check_dot_error(y.numpy(), ref.numpy(), bound.numpy())


U32 = 2.0 ** -24          # fp32 unit roundoff


def x3_bound(K, lam=8.0):
    """Per-element error bound of the large K-major GEMMs (az_gemm.hip gemm_x3 in either form),
    as a multiple of sum_k |a_k b_k| (+ |bias|), derived from the algorithm, not from observed
    errors:
    * bf16 form (x3, tuning build AZ_GEMM_PREC=x3): a = h + m + l (round-to-nearest-even bf16
      terms) leaves |a - (h+m+l)| <= 2^-24 |a|, and the three dropped cross terms m l', l m', l l'
      are <= 2^-23 (1 + 2^-8)^2 |a||b|: <= 2^-22 |a||b| per product, rigorously;
    * fp16 form (h3, the product): each row is scaled by a power of two s so its largest |a s|
      lies in [2^13, 2^14) (W's rows in [2^9, 2^10)), a s = h + l + r with |r| <= 2^-22 |a s|
      while l is a normal fp16 (|a s| >= 2^-2) and |r| <= 2^-25 otherwise (<= 2^-38 of the row's
      largest |a s|); with the dropped l l' <= 2^-22 |a s||b s'|, <= 3 * 2^-22 |a||b| per product
      plus that floor (az_x3.h split2s);
    * the kept bf16 x bf16 / fp16 x fp16 products are exact in fp32 (8 + 8 / 11 + 11 bits);
    * accumulation: one output element is a chain of (6 or 3) * ceil(K / 16) MFMA accumulations
      (one fp32 rounding each; S <= 8 chains for split-K, whose reduce adds <= 8 + 2 more; 16 more
      for a rounding inside each MFMA).  For n roundings the probabilistic bound of Higham and
      Mary (SIAM J. Sci. Comput. 41(5), 2019) is |err| <= lam sqrt(n) u sum|terms|, failing with
      probability <= 2 n exp(-lam^2 / 2) per element (lam = 8: < 1e-10 for n < 1e4).
    The chain is taken at its longest (x3, S = 1: the largest sqrt(n)) and the representation
    term at the larger (h3's 3 * 2^-22), so one bound covers both forms."""
    n = 6 * ((K + 15) // 16) + 16 + 8 + 2
    return 3 * 2.0 ** -22 + lam * np.sqrt(n) * U32


def x3_reference(x, w, b):
    """(float64 x w^T + b, sum_k |x_k w_k| + |b|): the reference and the magnitude x3_bound is a
    multiple of, as float64 torch tensors (CPU; shared by the width tests)."""
    xd, wd, bd = x.double(), w.double(), b.double()
    return xd @ wd.T + bd, xd.abs() @ wd.abs().T + bd.abs()


def x3_ratio(y, ref, mag):
    """|y - ref| / mag per element (numpy float64): what is held against x3_bound(K)."""
    return (y.double() - ref).abs().numpy() / (mag.numpy() + 1e-300)


def x3_report(rep):
    """Append `rep` to $AZ_REPORT_DIR/x3_accuracy.jsonl (no-op without the variable)."""
    d = os.environ.get("AZ_REPORT_DIR")
    if d:
        import json
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "x3_accuracy.jsonl"), "a") as f:
            f.write(json.dumps(rep) + "\n")


def _x3_check(ops, x, w, b, rows=None, report=None):
    """x3 GEMM (M x K) @ (N x K)^T + b against float64 on `rows` (all when None)."""
    y = ops.linear(x.cuda(), w.cuda(), b.cuda(), act=0).cpu().double()
    xs = x if rows is None else x[rows]
    ys = y if rows is None else y[rows]
    e = x3_ratio(ys, *x3_reference(xs, w, b))
    lim = x3_bound(x.shape[1])
    rep = {"M": x.shape[0], "N": w.shape[0], "K": x.shape[1], "x3_max": float(e.max()),
           "x3_mean": float(e.mean()), "bound": lim}
    if report:
        rep.update(report)
        x3_report(rep)
    assert e.max() <= lim, rep
    return rep


@pytest.mark.parametrize("M,N,K", [(512, 3136, 3136), (800, 3136, 3136), (1576, 3136, 3136), (700, 3136, 3136),
                                   (64, 3136, 3136), (37, 1001, 1028), (4096, 1024, 2048)])
def test_x3_gemm_has_fp32_accuracy(ops, M, N, K):
    """The K-major GEMMs with M > 64, K >= 1024, N >= 256 (output_transform; the self-play
    leg's ~1,576-row batches) run gemm_x3: fp32 operands split into three bf16 terms, six cross
    products on the bf16 matrix cores (M <= 64 takes the fp32 MFMA tile).  Error vs float64
    within x3_bound(K) (derived above) on uniform operands scaled like output_transform."""
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.rand((M, K), generator=g) * 2 - 1
    w = (torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5
    b = torch.rand((N,), generator=g) - 0.5
    rep = _x3_check(ops, x, w, b, report={"operands": "uniform"})
    cpu = (x @ w.T + b).double()
    ref = x.double() @ w.double().T + b.double()
    bound = (x.double().abs() @ w.double().abs().T + b.double().abs()).numpy()
    rep_cpu = float(((cpu - ref).abs().numpy() / bound).max())
    assert rep["x3_max"] <= x3_bound(K) and rep_cpu <= x3_bound(K)   # torch fp32 meets it too


@pytest.mark.parametrize("M", [700, 800, 1576, 2048, 2100, 3150, 4000])
def test_streamk_gemm_deterministic_and_accurate(ops, M):
    """Self-play batch sizes (M ~ 700 .. 4,000 at 3136 x 3136) run gemm_x3 in cycled stream-K
    form (az_gemm.hip gemm_x3_csk: macro-tile cycles cut into equal k ranges per block, split
    tiles summed by csk_fixup4_kernel in piece order; a last m-row with <= 128 real rows --
    M = 700, 800, 1576, 2100, 3150 -- as 128 x 256 tiles): every call returns the same bits, and
    every row (the tail rows included) of 256 random columns plus the last 64 (the partial wide
    tile) is within x3_bound of float64."""
    N = K = 3136
    g = torch.Generator().manual_seed(M)
    x = torch.rand((M, K), generator=g) * 2 - 1
    w = (torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5
    b = torch.rand((N,), generator=g) - 0.5
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y1 = ops.linear(xd, wd, bd, act=1)
    y2 = ops.linear(xd, wd, bd, act=1)
    assert torch.equal(y1, y2)
    cols = torch.cat([torch.randperm(N - 64, generator=g)[:256], torch.arange(N - 64, N)])
    ref = torch.relu(x.double() @ w[cols].double().T + b[cols].double())
    bound = (x.double().abs() @ w[cols].double().abs().T + b[cols].double().abs()).numpy()
    e = ((y1.cpu()[:, cols].double() - ref).abs().numpy() / bound).max()
    assert e <= x3_bound(K), e


def test_x3_gemm_accuracy_at_65536_rows(ops):
    """The large-batch leg's shape (M = 65,536: the 128x128 x3 tile, no split): 512 sampled
    rows against float64 (rows are independent)."""
    M, N, K = 65536, 3136, 3136
    g = torch.Generator().manual_seed(65536)
    x = torch.rand((M, K), generator=g) * 2 - 1
    w = (torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5
    b = torch.rand((N,), generator=g) - 0.5
    rows = torch.randperm(M, generator=g)[:512]
    _x3_check(ops, x, w, b, rows=rows, report={"operands": "uniform, 512 sampled rows"})


def test_x3_gemm_accuracy_on_real_path_operands(ops):
    """Operands of the real path: ReLU'd Connect4 trunk features of 1,576 boards (the self-play
    batch) times output_transform.0 / .2 weights after three train() calls (Adam moves them off
    the uniform init and widens their range), and the second GEMM on the first's ReLU output."""
    from types import SimpleNamespace
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Game import Connect4Game
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    W = synthetic_state_dict(connect4_net_spec(7), 1)
    G = synthetic_state_dict(gnn_spec(3136, 2), 2)
    args = SimpleNamespace(lr=0.01, dropout=0.3, epochs=4, batch_size=64, gnn_layers=2,
                           use_gnn=True)
    net = Connect4GNNWrapper(Connect4Game(7), args)
    net.nnet.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    net.gnn.load_state_dict({k: torch.from_numpy(v) for k, v in G.items()})
    rng = np.random.default_rng(3)
    boards = rng.integers(-1, 2, size=(256, 7, 7)).astype(np.int64)
    pis = rng.dirichlet(np.ones(8), 256)
    zs = rng.choice([-1, 1], 256)
    ex = [(boards[i], pis[i], int(zs[i])) for i in range(256)]
    gex = [(boards[i], 1, pis[i], np.float32(0.1), pis[i], np.float32(zs[i] * 0.5), int(zs[i]))
           for i in range(64)]
    np.random.seed(0)
    for _ in range(3):
        net.train(ex, gex)
    sd = {k: v.detach().cpu() for k, v in net.gnn.state_dict().items()}
    w0, b0 = sd["output_transform.0.weight"], sd["output_transform.0.bias"]
    w2, b2 = sd["output_transform.2.weight"], sd["output_transform.2.bias"]
    pos = rng.integers(-1, 2, size=(1576, 7, 7)).astype(np.int8)
    feat = net.extract_features(torch.from_numpy(pos).cuda()).detach().cpu().float()
    assert (feat >= 0).all() and feat.abs().max() > 0
    r0 = _x3_check(ops, feat, w0, b0, report={"operands": "trunk features x trained W0"})
    h = torch.relu(feat.double() @ w0.double().T + b0.double()).float()
    r2 = _x3_check(ops, h, w2, b2, report={"operands": "relu(h) x trained W2"})
    assert r0["x3_max"] < x3_bound(3136) and r2["x3_max"] < x3_bound(3136)


def test_x3_gemm_keeps_all_six_products(ops):
    """A discriminating case for the split itself: every operand is 1 + 2^-9 + d with
    d in [1.5, 2) * 2^-18 (exact in fp32), so its bf16 terms are h = 1, m = 2^-9, l = d > 0: the
    l cross terms are positive and add up over K instead of averaging out.  A scheme without
    them (four bf16 products) misses x3_bound(1024) on EVERY element (checked in float64 here);
    the GEMM (the fp16 form: 11 + 11 bits per operand) must stay inside it."""
    M, N, K = 256, 512, 1024
    g = torch.Generator().manual_seed(6)

    def operand(r, c):
        j = torch.randint(16, 32, (r, c), generator=g).double()
        return (1 + 2.0 ** -9 + 2.0 ** -18 * (1 + j / 32)).float()

    x = operand(M, K)
    w = operand(N, K) / K
    b = torch.zeros((N,))
    rep = _x3_check(ops, x, w, b, report={"operands": "1 + 2^-9 + d, positive l terms"})
    xh = x.to(torch.bfloat16).double()
    xm = (x.double() - xh).float().to(torch.bfloat16).double()
    wh = w.to(torch.bfloat16).double()
    wm = (w.double() - wh).float().to(torch.bfloat16).double()
    four = xh @ wh.T + xh @ wm.T + xm @ wh.T + xm @ wm.T
    ref = x.double() @ w.double().T
    e4 = ((four - ref).abs() / (x.double().abs() @ w.double().abs().T)).numpy()
    assert e4.min() > x3_bound(K) > rep["x3_max"], (float(e4.min()), rep)


def test_h3_gemm_keeps_the_cross_products(ops):
    """The fp16 form's split: every operand is (1 + 2^-12 (1 + j / 32)) * 2^e with j in [16, 32)
    (exact in fp32), so after the row scaling its fp16 terms are h = 2^e' and l = the 2^-12 part:
    the h*l cross products are positive and add up over K.  Without them (h*h only) every element
    misses x3_bound(1024) (checked in float64); the GEMM must stay inside it."""
    M, N, K = 256, 512, 1024
    g = torch.Generator().manual_seed(7)

    def operand(r, c):
        j = torch.randint(16, 32, (r, c), generator=g).double()
        return (1 + 2.0 ** -12 * (1 + j / 32)).float()

    x = operand(M, K)
    w = operand(N, K) / K
    b = torch.zeros((N,))
    rep = _x3_check(ops, x, w, b, report={"operands": "1 + 2^-12 d: positive fp16 l terms"})
    hh = x.half().double() @ (w * 1024).half().double().T / 1024    # h*h only (W row scale 2^10)
    ref = x.double() @ w.double().T
    e1 = ((hh - ref).abs() / (x.double().abs() @ w.double().abs().T)).numpy()
    assert e1.min() > x3_bound(K) > rep["x3_max"], (float(e1.min()), rep)


def test_h3_gemm_wide_dynamic_range(ops):
    """Rows whose values span 2^-30 .. 2^30 (and all-zero / single-value rows): the per-row
    power-of-two scaling keeps every row inside the bound; the fp16 range alone would overflow
    the large values and flush the small ones."""
    M, N, K = 300, 512, 1536
    g = torch.Generator().manual_seed(8)
    mag = 2.0 ** (torch.randint(-30, 31, (M, 1), generator=g).double()
                  + torch.randn((M, K), generator=g).double() * 3)
    x = (mag * torch.sign(torch.randn((M, K), generator=g).double())).float()
    x[0] = 0.0
    x[1] = 0.0
    x[1, 7] = 3.0e-30
    w = (torch.rand((N, K), generator=g) * 2 - 1) * 2.0 ** 20
    b = torch.zeros((N,))
    _x3_check(ops, x, w, b, report={"operands": "rows spanning 2^-30 .. 2^30, W ~ 2^20"})


def _registered(t):
    """Register a device tensor's storage like FlatParams does (az_weights_register), so its
    GEMMs take the cached fp16 planes; returns an unregister callable."""
    from azhip import _lib
    L = _lib.load()
    _lib.check(L.az_weights_register(t.data_ptr(), t.numel() * 4), "az_weights_register")
    return lambda: _lib.check(L.az_weights_unregister(t.data_ptr()), "az_weights_unregister")


def test_h3_weight_scales_follow_weight_updates(ops):
    """The fp16 form caches each REGISTERED weight matrix's row scales and fp16 planes between
    weight updates (az_weights_changed; az_adam_f32 and the parameter store call it).  Growing W
    4096x in place -- far past the scales' 64x headroom -- and announcing it gives the right
    result again; the same GEMM before the update is right too; unregistered storage is right
    without any announcement."""
    from azhip import params as P
    M, N, K = 512, 3136, 3136
    g = torch.Generator().manual_seed(9)
    x = torch.rand((M, K), generator=g) * 2 - 1
    w = ((torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5)
    b = torch.rand((N,), generator=g) - 0.5
    wd = w.cuda()
    unreg = _registered(wd)
    try:
        _x3_check_dev(ops, x, wd, w, b)
        wd.mul_(4096.0)
        P.weights_changed()
        _x3_check_dev(ops, x, wd, w * 4096.0, b)
    finally:
        unreg()
    wd.mul_(1.0 / 1024.0)                          # unregistered: per-call scales, no cache
    _x3_check_dev(ops, x, wd, w * 4.0, b)


def test_missed_weights_changed_serves_previous_weights(ops):
    """What INTEGRATION.md says a missed az_weights_changed() does on registered storage: above
    64 rows the GEMM multiplies by the cached planes, so it returns the PREVIOUS weights' result
    bit for bit (not a slightly less precise one); after the call it is the new weights'."""
    from azhip import params as P
    M, N, K = 300, 1024, 2048
    g = torch.Generator().manual_seed(10)
    x = (torch.rand((M, K), generator=g) * 2 - 1).cuda()
    w = ((torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5).cuda()
    b = torch.zeros((N,)).cuda()
    unreg = _registered(w)
    try:
        y0 = ops.linear(x, w, b)
        w.add_(0.01)
        y_stale = ops.linear(x, w, b)
        assert torch.equal(y_stale, y0)
        P.weights_changed()
        y1 = ops.linear(x, w, b)
        assert not torch.equal(y1, y0)
        _x3_check_dev(ops, x.cpu(), w, w.cpu(), b.cpu())
    finally:
        unreg()


def test_reference_side_adam_recipe_on_registered_weights(ops):
    """INTEGRATION.md §2's recipe for a reference-side integration that keeps torch.optim.Adam
    (Connect4GNN.py:132-135): register output_transform's weight storage, optimizer.step(),
    az_weights_changed(), predict -> the new weights' result (vs float64), at M = 512."""
    from azhip import _lib
    M, N, K = 512, 3136, 3136
    g = torch.Generator().manual_seed(11)
    x = (torch.rand((M, K), generator=g) * 2 - 1).cuda()
    lin = torch.nn.Linear(K, N).cuda()
    unreg = _registered(lin.weight.data)
    try:
        y0 = ops.linear(x, lin.weight.data, lin.bias.data)
        opt = torch.optim.Adam(lin.parameters(), lr=0.01)
        loss = (lin(x) ** 2).mean()
        loss.backward()
        opt.step()
        _lib.check(_lib.load().az_weights_changed(), "az_weights_changed")
        w1, b1 = lin.weight.data.cpu(), lin.bias.data.cpu()
        y1 = ops.linear(x, lin.weight.data, lin.bias.data)
        assert not torch.equal(y1, y0)
        _x3_check_dev(ops, x.cpu(), lin.weight.data, w1, b1)
    finally:
        unreg()


def test_flatparams_views_cannot_serve_stale_planes(ops):
    """FlatParams (the package's registered storage) finds torch-side writes itself: an
    in-place edit through a state_dict() view, a parameters() view or a torch optimizer-style
    update, with NO az_weights_changed call by the user, and the next c4_gnn_eval (B = 512: the
    cached-plane GEMMs) gives the new weights' result against float64; an az_adam_f32 step
    (the library's own write) likewise."""
    import oracle.nets as O
    from azhip.nets import Connect4Net, PolicyValueGNN
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    from types import SimpleNamespace
    W0 = synthetic_state_dict(connect4_net_spec(7), 5)
    game = SimpleNamespace(getBoardSize=lambda: (7, 7), getActionSize=lambda: 8)
    net = Connect4Net(game, {"dropout": 0.0}, init=W0).eval()
    G0 = {k: v for k, v in synthetic_state_dict(gnn_spec(3136, 2), 6).items()}
    gnn = PolicyValueGNN(3136, 2, init=G0).eval()
    boards = np.random.default_rng(12).integers(-1, 2, size=(512, 7, 7)).astype(np.int8)
    bd = cu(boards)

    def check(tag):
        lp, pi, v = ops.c4_gnn_eval(bd, net.params, gnn.params)
        W = {k: v.numpy() for k, v in net.params.cpu_state_dict().items()}
        G = {k: gnn.params[k].cpu().numpy() for k in (
            "output_transform.0.weight", "output_transform.0.bias",
            "output_transform.2.weight", "output_transform.2.bias")}
        lp64, v64 = O.c4_heads(O.output_transform(O.c4_features(boards, W), G), W)
        assert_close(f"stale_planes/{tag}/pi", pi.cpu().numpy(), np.exp(lp64), 1e-5)
        assert_close(f"stale_planes/{tag}/v", v.cpu().numpy(), v64, 1e-5)

    check("initial")
    gnn.state_dict()["output_transform.0.weight"].mul_(1.5)           # state_dict view
    check("state_dict_view")
    for p in gnn.parameters():                                         # parameters() views
        if p.shape == (3136, 3136):
            p.add_(torch.sign(p) * 1e-3)                               # an Adam-like step
    check("parameters_views")
    P = gnn.params
    P.zero_grad()
    P.grad_flat.normal_(generator=torch.Generator(device="cuda").manual_seed(3))
    P.reset_adam()
    P.step = 1
    ops.adam(P.flat, P.grad_flat, P.m, P.v, 0.01, P.step)              # az_adam_f32
    check("az_adam_f32")


def _x3_check_dev(ops, x, wd, w, b):
    y = ops.linear(x.cuda(), wd, b.cuda(), act=0).cpu().double()
    ref = x.double() @ w.double().T + b.double()
    bound = (x.double().abs() @ w.double().abs().T + b.double().abs()).numpy()
    e = (y - ref).abs().numpy() / bound
    assert np.isfinite(y.numpy()).all() and e.max() <= x3_bound(x.shape[1]), float(e.max())


@pytest.mark.parametrize("K", [3136, 2500, 100])
def test_small_m_rows_are_batch1_bits(ops, K):
    """M <= 8 rows (gemv_full / gemv_rows): every row of a batch is bit-identical to the same row
    computed alone, whatever M -- the premise of the arena's speculative leaf batches."""
    g = torch.Generator().manual_seed(K)
    N = 3136
    x = (torch.rand((8, K), generator=g) * 2 - 1).cuda()
    w = ((torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5).cuda()
    b = (torch.rand((N,), generator=g) - 0.5).cuda()
    one = [ops.linear(x[i:i + 1].contiguous(), w, b, act=1).cpu() for i in range(8)]
    for M in range(2, 9):
        y = ops.linear(x[:M].contiguous(), w, b, act=1).cpu()
        for i in range(M):
            assert torch.equal(y[i:i + 1], one[i]), (M, i)


def test_linear_split_gather_gated(ops):
    g = torch.Generator().manual_seed(3)
    V, F = 40, 64
    x = torch.rand((V, F), generator=g) - 0.5
    agg = torch.rand((V, F), generator=g) - 0.5
    w = torch.rand((F, 2 * F), generator=g) - 0.5
    b = torch.rand((F,), generator=g)
    rows = torch.tensor([0, 5, 7, 39], dtype=torch.int32)
    Gt = torch.rand((4, F), generator=g)
    R = torch.rand((V, F), generator=g)
    out = torch.zeros((V, F))
    c = torch.cat([x, agg], 1)[rows.long()].double()
    ref = R.double()[rows.long()] + Gt.double() * (c @ w.double().T + b.double())
    for M in (4,):
        o = out.cuda()
        ops.linear(x.cuda(), w.cuda(), b.cuda(), x2=agg.cuda(), a_rows=rows.cuda(), R=R.cuda(),
                   G=Gt.cuda(), c_rows=rows.cuda(), out=o, M=M)
        got = o.cpu()[rows.long()]
        assert rel_err(got.numpy(), ref.numpy()) < 2e-6
        untouched = np.setdiff1d(np.arange(V), rows.numpy())
        assert np.all(o.cpu().numpy()[untouched] == 0)


@pytest.mark.parametrize("M,N,K,split,act", [(20007, 256, 64, False, 0), (16384, 64, 64, False, 1),
                                             (33000, 64, 128, True, 2), (16385, 64, 64, False, 0)])
def test_linear_tall_skinny(ops, M, N, K, split, act):
    """gemm_f32_tall (M >= 16384, K <= 128: the grid GNN layers) incl. the [x; agg] concat,
    the gathered-row and gated-residual epilogue, and a ragged last 32-row tile."""
    g = torch.Generator().manual_seed(M + N + K)
    K1 = K // 2 if split else K
    x = torch.rand((M, K1), generator=g) * 2 - 1
    x2 = torch.rand((M, K - K1), generator=g) * 2 - 1 if split else None
    w = (torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5
    b = torch.rand((N,), generator=g) - 0.5
    a = torch.cat([x, x2], 1) if split else x
    ref = a.double() @ w.double().T + b.double()
    ref = [lambda t: t, torch.relu, torch.sigmoid][act](ref)
    bound = (a.double().abs() @ w.double().abs().T + b.double().abs()).numpy()
    y = ops.linear(x.cuda(), w.cuda(), b.cuda(), act=act,
                   x2=x2.cuda() if split else None).cpu()
    check_dot_error(y.numpy(), ref.numpy(), bound)
    if N == 64 and not split:
        # gated residual with the pre-gate copy (C2), as the GNN layer's last GEMM uses it
        R = torch.rand((M, N), generator=g)
        G = torch.rand((M, N), generator=g)
        pre = torch.empty((M, N)).cuda()
        o = ops.linear(x.cuda(), w.cuda(), b.cuda(), R=R.cuda(), G=G.cuda(), C2=pre)
        lin = x.double() @ w.double().T + b.double()
        check_dot_error(pre.cpu().numpy(), lin.numpy(), bound)
        np.testing.assert_allclose(o.cpu().numpy(), (R.double() + G.double() * lin).numpy(),
                                   atol=1e-5)


@pytest.mark.parametrize("M,N,K", [(64, 3136, 64), (128, 256, 4096), (36, 20, 64)])
def test_matmul_tn_nn(ops, M, N, K):
    g = torch.Generator().manual_seed(11)
    a = torch.rand((K, M), generator=g) - 0.5      # a^T is [M, K]
    b = torch.rand((K, N), generator=g) - 0.5
    out = torch.ones((M, N)).cuda()
    ops.matmul_tn(a.cuda(), b.cuda(), out, M, N, K, beta=1.0)
    ref = a.double().T @ b.double() + 1
    check_dot_error(out.cpu().numpy(), ref.numpy(), (a.double().abs().T @ b.double().abs() + 1).numpy())
    a2 = torch.rand((M, K), generator=g) - 0.5
    out2 = torch.empty((M, N)).cuda()
    ops.matmul_nn(a2.cuda(), b.cuda(), out2, M, N, K)
    check_dot_error(out2.cpu().numpy(), (a2.double() @ b.double()).numpy(),
                    (a2.double().abs() @ b.double().abs()).numpy())


def test_c4_trunk_and_heads_vs_oracle(ops):
    from oracle import nets as O
    z = golden("c4_net.npz")
    W = split_weights(z, "w/")
    Wd = {k: cu(v) for k, v in W.items()}
    for B in (1, 3, 256):
        boards = np.concatenate([z["boards"]] * 2)[:B]
        feat = ops.c4_trunk(cu(boards), Wd)
        ref = O.c4_features(boards, W)
        np.testing.assert_allclose(feat.cpu().numpy(), ref, atol=1e-5, rtol=1e-5)
        logp, pi, v = ops.heads(feat, Wd["fc_policy.weight"], Wd["fc_policy.bias"],
                                Wd["fc_value.weight"], Wd["fc_value.bias"])
        rlp, rv = O.c4_heads(ref, W)
        np.testing.assert_allclose(logp.cpu().numpy(), rlp, atol=1e-5)
        np.testing.assert_allclose(v.cpu().numpy(), rv, atol=1e-5)
        np.testing.assert_allclose(pi.cpu().numpy(), np.exp(rlp), atol=1e-5)
    # golden reference outputs directly (batch-1 predict of the reference)
    np.testing.assert_allclose(pi.cpu().numpy()[:256], z["pi_b1"], atol=1e-5)
    np.testing.assert_allclose(v.cpu().numpy()[:256], z["v_b1"], atol=1e-5)


@pytest.mark.parametrize("B", [1, 3, 8, 32, 33, 100, 320, 321])
def test_c4_trunk_heads_fused_bit_identical(ops, B):
    """az_c4_trunk_heads_fwd (one launch for B <= 320, the unfused pair above) ==
    az_c4_trunk_fwd + az_heads_fwd bit for bit, and the oracle within 1e-5
    (Connect4Net.py:42-60)."""
    from oracle import nets as O
    z = golden("c4_net.npz")
    W = split_weights(z, "w/")
    Wd = {k: cu(v) for k, v in W.items()}
    boards = np.concatenate([z["boards"]] * 2)[:B]
    f0 = ops.c4_trunk(cu(boards), Wd)
    ref = ops.heads(f0, Wd["fc_policy.weight"], Wd["fc_policy.bias"], Wd["fc_value.weight"],
                    Wd["fc_value.bias"])
    f1, lp, pi, v = ops.c4_trunk_heads(cu(boards), Wd)
    assert torch.equal(f0, f1)
    for a, r in zip((lp, pi, v), ref):
        assert torch.equal(a, r)
    rlp, rv = O.c4_heads(O.c4_features(boards, W), W)
    np.testing.assert_allclose(lp.cpu().numpy(), rlp, atol=1e-5)
    np.testing.assert_allclose(v.cpu().numpy(), np.asarray(rv).reshape(-1), atol=1e-5)


def test_c4_trunk_every_boards_per_block_variant_bit_identical(ops):
    """az_c4_trunk_fwd picks boards per block NB = 1..8 from a rounds model (az_trunk.hip); on
    256 CUs the batch sizes below select NB = 1, 2, 3, 4, 5, 6, 7, 8.  A board's arithmetic does
    not depend on NB, so every row of every batch equals (torch.equal) the same board's row in
    the B = 2,000 (NB = 8) batch, and the first rows match the oracle within 1e-5."""
    from oracle import nets as O
    z = golden("c4_net.npz")
    W = split_weights(z, "w/")
    Wd = {k: cu(v) for k, v in W.items()}
    boards = np.random.default_rng(11).integers(-1, 2, size=(2000, 7, 7)).astype(np.int8)
    full = ops.c4_trunk(cu(boards), Wd)
    for B in (200, 500, 600, 1000, 1200, 1500, 1700, 1999):
        f = ops.c4_trunk(cu(boards[:B]), Wd)
        assert torch.equal(f, full[:B]), B
    np.testing.assert_allclose(full[:16].cpu().numpy(), O.c4_features(boards[:16], W),
                               atol=1e-5, rtol=1e-5)


def test_c4_trunk_large_batches(ops):
    """NB = 2/4/8 boards-per-workgroup variants and ragged tails."""
    from oracle import nets as O
    z = golden("c4_net.npz")
    W = split_weights(z, "w/")
    Wd = {k: cu(v) for k, v in W.items()}
    rng = np.random.default_rng(5)
    for B in (2047, 4100):
        boards = rng.integers(-1, 2, size=(B, 7, 7)).astype(np.int8)
        feat = ops.c4_trunk(cu(boards), Wd).cpu().numpy()
        sel = np.r_[0:8, B - 9:B]
        np.testing.assert_allclose(feat[sel], O.c4_features(boards[sel], W), atol=1e-5, rtol=1e-5)


def test_ttt_trunk_heads_vs_golden(ops):
    from oracle import nets as O
    z = golden("ttt3.npz")
    W, G = split_weights(z, "w/"), split_weights(z, "g/")
    Wd = {k: cu(v) for k, v in W.items()}
    Gd = {k: cu(v) for k, v in G.items()}
    b = cu(z["boards"])
    s = ops.conv3x3_relu(b, Wd["conv1.weight"], Wd["conv1.bias"], 1)
    s = ops.conv3x3_relu(s, Wd["conv2.weight"], Wd["conv2.bias"], 1)
    s = ops.conv3x3_relu(s, Wd["conv3.weight"], Wd["conv3.bias"], 0)
    feat = s.reshape(s.shape[0], -1)
    np.testing.assert_allclose(feat.cpu().numpy(), O.ttt_features(z["boards"], W), atol=1e-5)

    def heads(f):
        h1 = ops.linear(f, Wd["fc1.weight"], Wd["fc1.bias"], act=ops.ACT_RELU)
        h2 = ops.linear(f, Wd["fc2.weight"], Wd["fc2.bias"], act=ops.ACT_RELU)
        return ops.heads(h1, Wd["fc_policy.weight"], Wd["fc_policy.bias"], Wd["fc_value.weight"],
                         Wd["fc_value.bias"], hv=h2)
    _, pi, v = heads(feat)
    np.testing.assert_allclose(pi.cpu().numpy(), z["pi"], atol=1e-5)
    np.testing.assert_allclose(v.cpu().numpy(), z["v"], atol=1e-5)
    enh, _ = ops.mlp2(feat, Gd["output_transform.0.weight"], Gd["output_transform.0.bias"],
                      Gd["output_transform.2.weight"], Gd["output_transform.2.bias"])
    _, pi, v = heads(enh)
    np.testing.assert_allclose(pi.cpu().numpy(), z["pi_gnn"], atol=1e-5)
    np.testing.assert_allclose(v.cpu().numpy(), z["v_gnn"], atol=1e-5)


def _synth():
    from azhip.weights import gnn_spec, synthetic_state_dict
    z = golden("synth_gnn.npz")
    G = synthetic_state_dict(gnn_spec(64, 2), int(z["seed_w"]))
    rng = np.random.Generator(np.random.PCG64(int(z["seed_x"])))
    x0 = rng.random((1024, 64), dtype=np.float32) * np.float32(2) - np.float32(1)
    return z, G, x0


def test_grid_attention_and_aggregate_vs_oracle(ops):
    from oracle import nets as O
    z, G, x0 = _synth()
    g = ops.DeviceGraph(z["rowptr"], z["col"])
    Gd = {k: cu(v) for k, v in G.items()}
    x = cu(x0)
    w1 = Gd["layers.0.attention.0.weight"]
    P = ops.linear(x, w1.view(256, 64))
    alpha = ops.attn_score(g, P, 128, Gd["layers.0.attention.0.bias"],
                           Gd["layers.0.attention.2.weight"], Gd["layers.0.attention.2.bias"])
    L = {k[len("layers.0."):]: v.astype(np.float64) for k, v in G.items() if k.startswith("layers.0.")}
    deg = np.diff(z["rowptr"])
    dst = np.repeat(np.arange(1024), deg)
    ref_a = O.attention_scores_pairs(x0[dst].astype(np.float64), x0[z["col"]].astype(np.float64), L)
    np.testing.assert_allclose(alpha.cpu().numpy(), ref_a, atol=2e-6)
    agg = ops.aggregate(g, x, alpha).cpu().numpy()
    s = np.zeros(1024)
    np.add.at(s, dst, ref_a)
    ref_agg = np.zeros((1024, 64))
    np.add.at(ref_agg, dst, x0[z["col"]] * (ref_a / s[dst])[:, None])
    np.testing.assert_allclose(agg, ref_agg, atol=2e-6)


def test_fused_grid_attention_aggregate_bit_identical(ops):
    """az_gnn_layer_fwd on a grid runs attention + aggregation as ONE kernel
    (attn_aggregate_small_kernel); the alpha and agg it leaves in the layer workspace equal the
    separate az_gnn_attn_score_fwd + az_gnn_aggregate_fwd bit for bit (8 grids, ragged CSR
    degrees 2..4)."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    z, G, _ = _synth()
    g = bench._grid_graph(ops, "cuda", 8)
    gen = torch.Generator().manual_seed(11)
    x = (torch.rand((g.V, 64), generator=gen) * 2 - 1).cuda()
    Gd = {k: cu(v) for k, v in G.items()}
    Wl = {k[len("layers.0."):]: v for k, v in Gd.items() if k.startswith("layers.0.")}
    out, ws = ops.gnn_layer(g, x, Wl)
    V, E, H = g.V, g.E, 128
    a256 = lambda b: (b + 255) // 256 * 256                                  # noqa: E731
    P = ws[:V * 2 * H * 4].view(torch.float32).view(V, 2 * H)
    o_alpha = a256(V * 2 * H * 4)
    alpha_f = ws[o_alpha:o_alpha + E * 4].view(torch.float32)
    o_agg = o_alpha + a256(E * 4)
    agg_f = ws[o_agg:o_agg + V * 64 * 4].view(torch.float32).view(V, 64)
    alpha = ops.attn_score(g, P, H, Wl["attention.0.bias"], Wl["attention.2.weight"],
                           Wl["attention.2.bias"])
    agg = ops.aggregate(g, x, alpha)
    torch.cuda.synchronize()
    assert torch.equal(alpha, alpha_f)
    assert torch.equal(agg, agg_f)


def test_grid_layers_vs_golden(ops):
    z, G, x0 = _synth()
    g = ops.DeviceGraph(z["rowptr"], z["col"])
    Gd = {k: cu(v) for k, v in G.items()}
    x = cu(x0)
    outs = []
    for i in range(2):
        Wl = {k[len(f"layers.{i}."):]: v for k, v in Gd.items() if k.startswith(f"layers.{i}.")}
        x, _ = ops.gnn_layer(g, x, Wl)
        outs.append(x.cpu().numpy())
    np.testing.assert_allclose(outs[0], z["grid_x1"], atol=1e-5)
    np.testing.assert_allclose(outs[1], z["grid_x2"], atol=1e-5)
    y, _ = ops.mlp2(x, Gd["output_transform.0.weight"], Gd["output_transform.0.bias"],
                    Gd["output_transform.2.weight"], Gd["output_transform.2.bias"])
    np.testing.assert_allclose(y.cpu().numpy(), z["grid_out"], atol=1e-5)


def test_grid_layers_infer_vs_golden(ops):
    """Eval-mode layers (az_gnn_layer_infer: the source-projection GEMM + ONE fused kernel per
    layer, nothing saved) on the reference's 32x32 grid (G3): within 1e-5 of the reference."""
    z, G, x0 = _synth()
    g = ops.DeviceGraph(z["rowptr"], z["col"])
    Gd = {k: cu(v) for k, v in G.items()}
    x = cu(x0)
    for i, key in enumerate(("grid_x1", "grid_x2")):
        Wl = {k[len(f"layers.{i}."):]: v for k, v in Gd.items() if k.startswith(f"layers.{i}.")}
        x, _ = ops.gnn_layer(g, x, Wl, save=False)
        np.testing.assert_allclose(x.cpu().numpy(), z[key], atol=1e-5)


def _random_graph(V, maxdeg, seed, p_empty=0.1, local=True):
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, maxdeg + 1, V)
    deg[rng.random(V) < p_empty] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    if local:       # mostly nearby sources (grid-like), some far ones
        col = (np.repeat(np.arange(V), deg) + rng.integers(-40, 41, rowptr[-1])) % V
        far = rng.random(rowptr[-1]) < 0.05
        col[far] = rng.integers(0, V, far.sum())
    else:
        col = rng.integers(0, V, rowptr[-1])
    for d in range(V):                   # sorted, distinct sources per destination (as a CSR)
        seg = col[rowptr[d]:rowptr[d + 1]]
        col[rowptr[d]:rowptr[d + 1]] = np.sort(seg)
    return rowptr, col


@pytest.mark.parametrize("V,maxdeg,local", [(1000, 4, True), (4099, 4, False), (70001, 4, True),
                                            (3000, 6, True)])
def test_fused_layer_equals_training_path(ops, V, maxdeg, local):
    """az_gnn_layer_infer == az_gnn_layer_fwd (the unfused kernels the backward relies on) on
    random CSR graphs: ragged in-degrees 0..maxdeg (destination subsets, D < V, so untouched rows
    are copies), partial last tiles, arbitrary gathers; maxdeg > 4 takes the unfused path
    (bit-identical).  Small graphs are also checked against the oracle (gnn_utils.py:34-74)."""
    from oracle import nets as O
    _, G, _ = _synth()
    rowptr, col = _random_graph(V, maxdeg, seed=V)
    g = ops.DeviceGraph(rowptr, col)
    assert g.D < V
    Gd = {k: cu(v) for k, v in G.items()}
    x0 = (np.random.default_rng(V + 1).random((V, 64), dtype=np.float32) * 2 - 1)
    x = cu(x0)
    Wl = {k[len("layers.1."):]: v for k, v in Gd.items() if k.startswith("layers.1.")}
    a, _ = ops.gnn_layer(g, x, Wl, save=True)
    b, _ = ops.gnn_layer(g, x, Wl, save=False)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    if maxdeg > 4:
        np.testing.assert_array_equal(a, b)
    else:
        np.testing.assert_allclose(b, a, atol=2e-6, rtol=1e-6)
    empty = np.diff(rowptr) == 0
    np.testing.assert_array_equal(b[empty], x0[empty])
    if V <= 4099:
        ref = O.gnn_layer_csr(x0.astype(np.float64), rowptr, col, G, 1)
        np.testing.assert_allclose(b, ref, atol=1e-5)


def _band_graph(V, maxdeg, R, seed, p_empty=0.1):
    """Random node-ordered graph with every source within R of its destination (|s - d| <= R),
    ragged in-degrees 0..maxdeg, sorted distinct sources per destination."""
    rng = np.random.default_rng(seed)
    rowptr, col = [0], []
    for d in range(V):
        k = 0 if rng.random() < p_empty else int(rng.integers(1, maxdeg + 1))
        lo, hi = max(0, d - R), min(V - 1, d + R)
        cand = np.arange(lo, hi + 1)
        src = np.sort(rng.choice(cand, size=min(k, len(cand)), replace=False))
        col += src.tolist()
        rowptr.append(len(col))
    return np.array(rowptr), np.array(col)


@pytest.mark.parametrize("V,maxdeg,R", [(1000, 4, 32), (4099, 6, 32), (130, 3, 5), (64, 4, 32),
                                        (20011, 4, 20)])
def test_band_layer_equals_training_path(ops, V, maxdeg, R):
    """The band kernel (az_gnn_layer_infer on graphs with 0 < band <= 32: one launch, x / Ps in a
    rolling LDS window, bf16x3 MFMAs) == az_gnn_layer_fwd within 2e-6 and the oracle within
    1e-5 (gnn_utils.py:34-74) on random banded graphs: ragged in-degrees incl. 0 and above 4,
    V not a multiple of the 64-node tile, many tiles per block (V = 20,011)."""
    from oracle import nets as O
    _, G, _ = _synth()
    rowptr, col = _band_graph(V, maxdeg, R, seed=V + R)
    g = ops.DeviceGraph(rowptr, col)
    assert 0 < g.band <= 32 and g.D < V
    Gd = {k: cu(v) for k, v in G.items()}
    x0 = (np.random.default_rng(V + 2).random((V, 64), dtype=np.float32) * 2 - 1)
    x = cu(x0)
    Wl = {k[len("layers.1."):]: v for k, v in Gd.items() if k.startswith("layers.1.")}
    a, _ = ops.gnn_layer(g, x, Wl, save=True)
    b, _ = ops.gnn_layer(g, x, Wl, save=False)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    np.testing.assert_allclose(b, a, atol=2e-6, rtol=1e-6)
    empty = np.diff(rowptr) == 0
    np.testing.assert_array_equal(b[empty], x0[empty])
    if V <= 4099:
        ref = O.gnn_layer_csr(x0.astype(np.float64), rowptr, col, G, 1)
        np.testing.assert_allclose(b, ref, atol=1e-5)


def _grid_shard(graphs, h=32, w=32):
    """`graphs` disjoint 4-neighbour h x w grids, node-ordered (bench.py's config-5 shard)."""
    z = golden("synth_gnn.npz")
    rp, cl = z["rowptr"].astype(np.int64), z["col"].astype(np.int64)
    V1, E1 = h * w, len(cl)
    gi = np.arange(graphs, dtype=np.int64)
    rowptr = np.concatenate([(rp[:-1][None, :] + (gi * E1)[:, None]).ravel(), [graphs * E1]])
    col = (cl[None, :] + (gi * V1)[:, None]).ravel()
    return rowptr, col, rp, cl


def test_band_layer_and_forward_at_shard_size(ops):
    """Config 5 at the per-GPU shard the bench times (VERDICT r04 'do this' #2): 512 grids,
    V = 524,288, E = 2,031,616 -- 32 64-row tiles per block of the band kernel, so its LDS ring
    runs its long steady state.  Every row of the band layer against the training path's
    unfused kernels (2e-6), the eval forward (band layer 0, then layer 1 + output_transform in
    one launch) against the training-path layers + az_mlp2_fwd (4e-6), and grids 0, 255 and
    511 of both against the float64 oracle (gnn_utils.py:30-117) at 1e-5."""
    from azhip.nets import PolicyValueGNN
    from oracle import nets as O
    _, G, _ = _synth()
    rowptr, col, rp1, cl1 = _grid_shard(512)
    g = ops.DeviceGraph(rowptr, col)
    assert g.V == 524288 and g.E == 2031616 and 0 < g.band <= 32
    x0 = (np.random.default_rng(512).random((g.V, 64), dtype=np.float32) * 2 - 1)
    Gd = {k: cu(v) for k, v in G.items()}
    x = cu(x0)
    Wl = [{k[len(f"layers.{i}."):]: v for k, v in Gd.items() if k.startswith(f"layers.{i}.")}
          for i in range(2)]
    a1, _ = ops.gnn_layer(g, x, Wl[0], save=True)
    b1, _ = ops.gnn_layer(g, x, Wl[0], save=False)
    assert_close("config5_shard/band_layer_vs_training_path", b1.cpu().numpy(), a1.cpu().numpy(),
                 2e-6)
    a2, _ = ops.gnn_layer(g, a1, Wl[1], save=True)
    ref_y, _ = ops.mlp2(a2, Gd["output_transform.0.weight"], Gd["output_transform.0.bias"],
                        Gd["output_transform.2.weight"], Gd["output_transform.2.bias"])
    net = PolicyValueGNN(64, 2, init=G).eval()
    y = net.forward_graph(x, g)
    torch.cuda.synchronize()
    y, ref_y, b1 = y.cpu().numpy(), ref_y.cpu().numpy(), b1.cpu().numpy()
    assert_close("config5_shard/forward_vs_training_path", y, ref_y, 4e-6)
    for gi in (0, 255, 511):
        rows = slice(gi * 1024, (gi + 1) * 1024)
        xg = x0[rows].astype(np.float64)
        l1 = O.gnn_layer_csr(xg, rp1, cl1, G, 0)
        assert_close(f"config5_shard/band_layer_vs_oracle_grid{gi}", b1[rows], l1, 1e-5)
        yo = O.policy_value_gnn_csr(xg, rp1, cl1, G)
        assert_close(f"config5_shard/forward_vs_oracle_grid{gi}", y[rows], yo, 1e-5)


@pytest.mark.parametrize("kind", ["grid", "band", "random"])
def test_layer_ot_equals_layer_then_mlp2(ops, kind):
    """az_gnn_layer_ot_infer (the last layer + output_transform; ONE launch on band graphs,
    the layer's output never reaching HBM) == az_gnn_layer_fwd followed by az_mlp2_fwd
    (gnn_utils.py:87-117), on the reference's grid, a random band graph and a non-band graph."""
    z, G, x0 = _synth()
    if kind == "grid":
        rowptr, col = z["rowptr"], z["col"]
    elif kind == "band":
        rowptr, col = _band_graph(3001, 5, 32, seed=5)
    else:
        rowptr, col = _random_graph(2500, 4, seed=6)
    g = ops.DeviceGraph(rowptr, col)
    V = g.V
    x0 = (np.random.default_rng(V).random((V, 64), dtype=np.float32) * 2 - 1)
    Gd = {k: cu(v) for k, v in G.items()}
    x = cu(x0)
    Wl = {k[len("layers.1."):]: v for k, v in Gd.items() if k.startswith("layers.1.")}
    ot = [Gd["output_transform.0.weight"], Gd["output_transform.0.bias"],
          Gd["output_transform.2.weight"], Gd["output_transform.2.bias"]]
    a, _ = ops.gnn_layer(g, x, Wl, save=True)
    ref, _ = ops.mlp2(a, *ot)
    y, _ = ops.gnn_layer_ot(g, x, Wl, *ot)
    np.testing.assert_allclose(y.cpu().numpy(), ref.cpu().numpy(), atol=4e-6, rtol=1e-6)


def test_grid_forward_eval_vs_golden(ops):
    """PolicyValueGNN.forward_graph in eval mode (layer 0, then layer 1 + output_transform as
    one call) on the reference's 32x32 grid (G3): within 1e-5 of the reference's output."""
    from azhip.nets import PolicyValueGNN
    z, G, x0 = _synth()
    g = ops.DeviceGraph(z["rowptr"], z["col"])
    net = PolicyValueGNN(64, 2, init=G).eval()
    y = net.forward_graph(cu(x0), g)
    np.testing.assert_allclose(y.cpu().numpy(), z["grid_out"], atol=1e-5)


def test_band_layer_wide_dynamic_range(ops):
    """The band kernel's fp16 form scales every x, agg, u1, x_out and h row by its own power of
    two: rows spanning 10^-15 .. 10^15, all-zero rows (scale 1) and destinations without in-edges
    (x bit for bit) agree with the fp32 training path row by row, to 1e-3 of the row's magnitude.
    (A scale shared by a 64-row tile failed this at O(1).  The bound is looser than the 2e-6 of
    O(1) data because a score's absolute error grows with the features' magnitude and sigmoid
    turns it into a relative error of alpha, which multiplies a source up to 10^30 larger than
    the destination: measured worst 1.7e-4.)  Scores near fp32's denormal range are normalised
    as the reference does (S > 0 however small, gnn_utils.py:58)."""
    _, G, _ = _synth()
    V = 3000
    rowptr, col = _band_graph(V, 4, 32, seed=77, p_empty=0.05)
    g = ops.DeviceGraph(rowptr, col)
    rng = np.random.default_rng(78)
    x0 = (rng.random((V, 64), dtype=np.float32) * 2 - 1)
    x0 *= (10.0 ** rng.uniform(-15, 15, (V, 1))).astype(np.float32)
    x0[rng.random(V) < 0.05] = 0.0
    Gd = {k: cu(v) for k, v in G.items()}
    x = cu(x0)
    Wl = {k[len("layers.1."):]: v for k, v in Gd.items() if k.startswith("layers.1.")}
    a, _ = ops.gnn_layer(g, x, Wl, save=True)
    b, _ = ops.gnn_layer(g, x, Wl, save=False)
    a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    assert np.isfinite(b).all()
    scale = np.maximum(np.abs(a).max(1, keepdims=True), np.abs(x0).max(1, keepdims=True))
    err = np.abs(b - a) / np.maximum(scale, 1e-30)
    assert err.max() <= 1e-3, f"worst row error {err.max():.3g} of its magnitude"
    empty = np.diff(rowptr) == 0
    np.testing.assert_array_equal(b[empty], x0[empty])


def test_band_layer_with_understated_band(ops):
    """A caller claiming band 32 for a graph whose sources reach 40 nodes away and 5 % anywhere:
    out-of-window sources take the band kernel's slow path -- same result as the training path."""
    _, G, _ = _synth()
    V = 3000
    rowptr, col = _random_graph(V, 4, seed=91)
    g = ops.DeviceGraph(rowptr, col)
    assert g.band > 32
    Gd = {k: cu(v) for k, v in G.items()}
    x0 = (np.random.default_rng(92).random((V, 64), dtype=np.float32) * 2 - 1)
    x = cu(x0)
    Wl = {k[len("layers.0."):]: v for k, v in Gd.items() if k.startswith("layers.0.")}
    a, _ = ops.gnn_layer(g, x, Wl, save=True)
    g.c.band = 32
    b, _ = ops.gnn_layer(g, x, Wl, save=False)
    np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), atol=2e-6, rtol=1e-6)


@pytest.mark.parametrize("claimed", [4, 0, 2])
def test_fused_layer_with_understated_max_deg(ops, claimed):
    """az_graph.max_deg is the caller's claim; the eval-mode layer must not trust it: a graph with
    in-degrees up to 7 whose max_deg says 4 or 2 takes the fused kernel (edges past 4 on its
    slow path, none dropped), one whose max_deg is 0 (an unset field) the unfused kernels --
    every result equals the training path and the oracle (gnn_utils.py:34-74)."""
    from oracle import nets as O
    _, G, _ = _synth()
    V = 2000
    rowptr, col = _random_graph(V, 7, seed=77)
    g = ops.DeviceGraph(rowptr, col)
    assert g.max_deg == 7
    Gd = {k: cu(v) for k, v in G.items()}
    x0 = (np.random.default_rng(78).random((V, 64), dtype=np.float32) * 2 - 1)
    x = cu(x0)
    Wl = {k[len("layers.0."):]: v for k, v in Gd.items() if k.startswith("layers.0.")}
    a, _ = ops.gnn_layer(g, x, Wl, save=True)
    g.c.max_deg = claimed
    g.c.band = 0                      # keep this test on the degree-dispatched kernels
    b, _ = ops.gnn_layer(g, x, Wl, save=False)
    c, _ = ops.gnn_layer(g, x, Wl, save=True)     # the training path under the same claim
    a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
    if claimed == 0:
        np.testing.assert_array_equal(a, b)
    else:
        np.testing.assert_allclose(b, a, atol=2e-6, rtol=1e-6)
    np.testing.assert_allclose(c, a, atol=2e-6, rtol=1e-6)
    ref = O.gnn_layer_csr(x0.astype(np.float64), rowptr, col, G, 0)
    np.testing.assert_allclose(b, ref, atol=1e-5)
    np.testing.assert_allclose(c, ref, atol=1e-5)


def test_star_literal_n4096(ops):
    z, G, _ = _synth()
    Gd = {k: cu(v) for k, v in G.items()}
    rng = np.random.Generator(np.random.PCG64(int(z["seed_star"])))
    sx = rng.random((4096, 64), dtype=np.float32) * np.float32(2) - np.float32(1)
    g = ops.DeviceGraph.star(4096)
    x = cu(sx)
    for i in range(2):
        Wl = {k[len(f"layers.{i}."):]: v for k, v in Gd.items() if k.startswith(f"layers.{i}.")}
        x, _ = ops.gnn_layer(g, x, Wl)
    y, _ = ops.mlp2(x, Gd["output_transform.0.weight"], Gd["output_transform.0.bias"],
                    Gd["output_transform.2.weight"], Gd["output_transform.2.bias"])
    y = y.cpu().numpy()
    np.testing.assert_allclose(y[:65], z["star_out_head"], atol=1e-5)
    np.testing.assert_allclose(y.sum(1), z["star_out_rowsum"], atol=1e-4)


def test_c4_star_forward_vs_golden(ops, c4_gnn_weights):
    z = golden("c4_gnn.npz")
    W = split_weights(golden("c4_net.npz"), "w/")
    Wd = {k: cu(v) for k, v in W.items()}
    Gd = {k: cu(v) for k, v in c4_gnn_weights.items()}
    feat = ops.c4_trunk(cu(z["boards"]), Wd)
    g = ops.DeviceGraph.star(64)
    x = feat
    for i in range(2):
        Wl = {k[len(f"layers.{i}."):]: v for k, v in Gd.items() if k.startswith(f"layers.{i}.")}
        x, _ = ops.gnn_layer(g, x, Wl)
        np.testing.assert_allclose(x[0].cpu().numpy(), z["star_row0"][i], atol=1e-5)
        np.testing.assert_array_equal(x[1:].cpu().numpy(), feat[1:].cpu().numpy())
    y, _ = ops.mlp2(x, Gd["output_transform.0.weight"], Gd["output_transform.0.bias"],
                    Gd["output_transform.2.weight"], Gd["output_transform.2.bias"])
    logp, pi, v = ops.heads(y, Wd["fc_policy.weight"], Wd["fc_policy.bias"],
                            Wd["fc_value.weight"], Wd["fc_value.bias"])
    np.testing.assert_allclose(logp.cpu().numpy(), z["star_logp"], atol=1e-5)
    np.testing.assert_allclose(v.cpu().numpy(), z["star_v"], atol=1e-5)
    # per-row semantics (predict_with_gnn): layers are the identity on a 1-row input
    y1, _ = ops.mlp2(feat, Gd["output_transform.0.weight"], Gd["output_transform.0.bias"],
                     Gd["output_transform.2.weight"], Gd["output_transform.2.bias"])
    _, pi, v = ops.heads(y1, Wd["fc_policy.weight"], Wd["fc_policy.bias"],
                         Wd["fc_value.weight"], Wd["fc_value.bias"])
    np.testing.assert_allclose(pi.cpu().numpy(), z["pi_gnn_b1"], atol=1e-5)
    np.testing.assert_allclose(v.cpu().numpy(), z["v_gnn_b1"], atol=1e-5)


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 10007, 262147])
def test_adam_vs_oracle(ops, n):
    """Every size class of the unrolled kernel: tail only (n < 4), one partial block, several
    blocks with a ragged last one."""
    from oracle.nets import Adam
    rng = np.random.default_rng(n)
    p = rng.standard_normal(n).astype(np.float32)
    P = {"p": p.astype(np.float64)}
    opt = Adam(P, lr=1e-3)
    pd, md, vd = cu(p), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    for step in range(1, 4):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n)).astype(np.float32)
        ops.adam(pd, cu(g), md, vd, 1e-3, step)
        P = opt.step(P, {"p": g.astype(np.float64)})
    np.testing.assert_allclose(pd.cpu().numpy(), P["p"], atol=1e-6)


@pytest.mark.parametrize("B", [1, 5, 64, 300, 512, 1024, 4096])
def test_transform_heads_fused_equals_unfused(ops, B):
    """az_transform_heads_fwd (second GEMM's split-K reduction fused into the heads) is bit-
    identical to az_gemm_f32 x2 + az_heads_fwd, and matches the oracle within 1e-5
    (gnn_utils.py:115 then Connect4GNN.py:48-57, per row)."""
    from oracle import nets as O
    F, A = 3136, 8
    g = torch.Generator().manual_seed(B)
    x = torch.rand((B, F), generator=g) * 2 - 1
    w0 = (torch.rand((F, F), generator=g) * 2 - 1) / F ** 0.5
    w2 = (torch.rand((F, F), generator=g) * 2 - 1) / F ** 0.5
    b0, b2 = (torch.rand((F,), generator=g) - 0.5) * 0.1, (torch.rand((F,), generator=g) - 0.5) * 0.1
    wp = (torch.rand((A, F), generator=g) * 2 - 1) / F ** 0.5
    wv = (torch.rand((1, F), generator=g) * 2 - 1) / F ** 0.5
    bp, bv = torch.rand((A,), generator=g) - 0.5, torch.rand((1,), generator=g) - 0.5
    c = [t.cuda() for t in (x, w0, b0, w2, b2, wp, bp, wv, bv)]
    logp, pi, v, y, hid = ops.transform_heads(*c)
    h_ref = ops.linear(c[0], c[1], c[2], act=ops.ACT_RELU)
    y_ref = ops.linear(h_ref, c[3], c[4])
    lp_ref, pi_ref, v_ref = ops.heads(y_ref, c[5], c[6], c[7], c[8])
    torch.cuda.synchronize()
    assert torch.equal(hid, h_ref) and torch.equal(y, y_ref)
    assert torch.equal(logp, lp_ref) and torch.equal(pi, pi_ref) and torch.equal(v, v_ref)
    G = {"output_transform.0.weight": w0.numpy(), "output_transform.0.bias": b0.numpy(),
         "output_transform.2.weight": w2.numpy(), "output_transform.2.bias": b2.numpy()}
    W = {"fc_policy.weight": wp.numpy(), "fc_policy.bias": bp.numpy(),
         "fc_value.weight": wv.numpy(), "fc_value.bias": bv.numpy()}
    olp, ov = O.c4_heads(O.policy_value_gnn_per_row(x.numpy(), G), W)
    assert np.abs(logp.cpu().numpy() - olp).max() < 1e-5
    assert np.abs(v.cpu().numpy() - ov).max() < 1e-5


@pytest.mark.parametrize("B", [1, 9, 65, 300, 512, 1024, 1576, 4096])
@pytest.mark.parametrize("registered", [True, False])
def test_transform_heads_without_y(ops, B, registered):
    """az_transform_heads_fwd with y = NULL (what every evaluator calls): y is never formed --
    on the fp16 split-K tiles each block folds its tile of y into the heads' dot products
    (az_x3.h HeadsEpi) and heads_tiles_finalize_kernel sums them in tile order; other shapes
    (B <= 64, stream-K batches) form y in scratch.  The heads are linear in y
    (Connect4GNN.py:48-57), so this is the same function: within 1e-5 of the oracle
    (gnn_utils.py:115, per row), within 2e-6 of the y path, hidden bit-identical to it, and the
    same bits on registered (cached W planes) and unregistered (in-tile split) weights."""
    from oracle import nets as O
    F, A = 3136, 8
    g = torch.Generator().manual_seed(B + 77)
    x = torch.rand((B, F), generator=g) * 2 - 1
    w0 = (torch.rand((F, F), generator=g) * 2 - 1) / F ** 0.5
    w2 = (torch.rand((F, F), generator=g) * 2 - 1) / F ** 0.5
    b0, b2 = (torch.rand((F,), generator=g) - 0.5) * 0.1, (torch.rand((F,), generator=g) - 0.5) * 0.1
    wp = (torch.rand((A, F), generator=g) * 2 - 1) / F ** 0.5
    wv = (torch.rand((1, F), generator=g) * 2 - 1) / F ** 0.5
    bp, bv = torch.rand((A,), generator=g) - 0.5, torch.rand((1,), generator=g) - 0.5
    c = [t.cuda() for t in (x, w0, b0, w2, b2, wp, bp, wv, bv)]
    unreg = []
    if registered:
        unreg = [_registered(c[1]), _registered(c[3])]
    try:
        logp, pi, v, y, hid = ops.transform_heads(*c)
        tl, tp, tv, ty, th = ops.transform_heads(*c, want_y=False)
        if registered:
            cu_ = [t.clone() for t in c]              # the same values, unregistered storage
            ul, up, uv, _, _ = ops.transform_heads(*cu_, want_y=False)
            torch.cuda.synchronize()
            assert torch.equal(ul, tl) and torch.equal(up, tp) and torch.equal(uv, tv)
    finally:
        for u in unreg:
            u()
    torch.cuda.synchronize()
    assert ty is None and torch.equal(th, hid)
    assert_close(f"heads_without_y/B{B}/logp_vs_y_path", tl.cpu().numpy(), logp.cpu().numpy(), 2e-6)
    assert_close(f"heads_without_y/B{B}/v_vs_y_path", tv.cpu().numpy(), v.cpu().numpy(), 2e-6)
    G = {"output_transform.0.weight": w0.numpy(), "output_transform.0.bias": b0.numpy(),
         "output_transform.2.weight": w2.numpy(), "output_transform.2.bias": b2.numpy()}
    W = {"fc_policy.weight": wp.numpy(), "fc_policy.bias": bp.numpy(),
         "fc_value.weight": wv.numpy(), "fc_value.bias": bv.numpy()}
    olp, ov = O.c4_heads(O.policy_value_gnn_per_row(x.numpy(), G), W)
    assert_close(f"heads_without_y/B{B}/logp_vs_oracle", tl.cpu().numpy(), olp, 1e-5)
    assert_close(f"heads_without_y/B{B}/pi_vs_oracle", tp.cpu().numpy(), np.exp(olp), 1e-5)
    assert_close(f"heads_without_y/B{B}/v_vs_oracle", tv.cpu().numpy(), ov, 1e-5)


@pytest.mark.parametrize("A,K", [(8, 3136), (9, 512), (7, 256), (20, 1000)])
def test_heads_small_batch_bit_identical(ops, A, K):
    """B <= 32 runs the one-launch heads_rows_kernel; every row equals the two-launch path's
    (the same rows inside a B = 64 batch) bit for bit, and the fp64 heads within 1e-5
    (Connect4GNN.py:48-57)."""
    g = torch.Generator().manual_seed(A * K)
    x, y = torch.rand((64, K), generator=g) - 0.5, torch.rand((64, K), generator=g) - 0.5
    wp, bp = (torch.rand((A, K), generator=g) - 0.5) / 8, torch.rand((A,), generator=g) - 0.5
    wv, bv = (torch.rand((1, K), generator=g) - 0.5) / 8, torch.rand((1,), generator=g) - 0.5
    args = [cu(t) for t in (wp, bp, wv, bv)]
    ref = ops.heads(cu(x), *args, hv=cu(y))
    lg = x.double() @ wp.double().T + bp.double()
    lp64 = torch.log_softmax(lg, 1)
    v64 = torch.tanh(y.double() @ wv.double().T + bv.double())[:, 0]
    for B in (1, 5, 32):
        got = ops.heads(cu(x[:B]), *args, hv=cu(y[:B]))
        for a, r in zip(got, ref):
            assert torch.equal(a, r[:B])
        np.testing.assert_allclose(got[0].cpu().numpy(), lp64[:B].numpy(), atol=1e-5)
        np.testing.assert_allclose(got[2].cpu().numpy(), v64[:B].numpy(), atol=1e-5)


@pytest.mark.parametrize("F", [288, 4160])
@pytest.mark.parametrize("registered", [False, True])
def test_linear_heads_without_y_any_width(ops, F, registered):
    """az_linear_heads_fwd with y = NULL at a stream-K batch size (B = 1,576) and widths the
    stream-K heads epilogue cannot take (its finalize gives each lane one whole 64-column block:
    F = 288 leaves a half block, F = 4,160 is 65 blocks): the call falls back to a path that forms
    y, so the heads equal the y path within 2e-6 and fp64 (Connect4GNN.py:48-57 on
    gnn_utils.py:115's last Linear) within 1e-5."""
    B, A = 1576, 8
    g = torch.Generator().manual_seed(F + registered)
    x = torch.rand((B, F), generator=g) * 2 - 1
    w = (torch.rand((F, F), generator=g) * 2 - 1) / F ** 0.5
    b = (torch.rand((F,), generator=g) - 0.5) * 0.1
    wp = (torch.rand((A, F), generator=g) * 2 - 1) / F ** 0.5
    wv = (torch.rand((1, F), generator=g) * 2 - 1) / F ** 0.5
    bp, bv = torch.rand((A,), generator=g) - 0.5, torch.rand((1,), generator=g) - 0.5
    c = [t.cuda() for t in (x, w, b, wp, bp, wv, bv)]
    unreg = [_registered(c[1])] if registered else []
    try:
        logp, pi, v, y = ops.linear_heads(*c)
        tl, tp, tv, ty = ops.linear_heads(*c, want_y=False)
        torch.cuda.synchronize()
    finally:
        for u in unreg:
            u()
    assert ty is None
    assert_close(f"heads_any_width/F{F}/r{int(registered)}/logp_vs_y_path", tl.cpu().numpy(),
                 logp.cpu().numpy(), 2e-6)
    assert_close(f"heads_any_width/F{F}/r{int(registered)}/v_vs_y_path", tv.cpu().numpy(),
                 v.cpu().numpy(), 2e-6)
    yd = x.double() @ w.double().T + b.double()
    lg = yd @ wp.double().T + bp.double()
    olp = (lg - torch.logsumexp(lg, 1, keepdim=True)).numpy()
    ov = torch.tanh(yd @ wv.double().T + bv.double()).flatten().numpy()
    assert_close(f"heads_any_width/F{F}/r{int(registered)}/logp_vs_fp64", tl.cpu().numpy(), olp, 1e-5)
    assert_close(f"heads_any_width/F{F}/r{int(registered)}/v_vs_fp64", tv.cpu().numpy(), ov, 1e-5)
