"""Training on child stars on the MI355X: az_gnn_star_batch_fwd_train / az_gnn_star_batch_bwd
against float64 autograd on the forest-of-stars graph, T.gnn_star_grads on real boards with real
children, NetWrapper.train under args.gnn_neighbors_train, and the rejected arguments.

The criterion is tests/gradcheck.py's, unchanged (tests/test_gpu_train.py derives it): per element
|ours - ref64| <= 10 max|torch32 - ref64| + C_ROUND u32 S with S from abs_contributions for the
gradients; for the forward rows and the scalar losses the form without S.  guard_reference sees
every float64 reference first (test_references_are_not_vacuous runs it on the CPU, on the very
inputs the GPU tests use).

Kernel level: F = 1024 (the 4x4 board's width), H = 128, x random normal, weights at init scale,
dx0 random normal, loss = sum(dx0 * x0).  Star sizes per case:
  gemv       [9]                       M <= 8: the GEMV dispatch
  mixed      [1, 2, 5]                 a one-row star and a one-edge star among others
  past8      2..9 cycled over nine, 1  B just past 8
  tile       [34, 35]                  33 and 34 neighbours: both sides of the 32-neighbour tile
  split      1..6 cycled over 70       M > 64: the fp16-split GEMM form at K = 2F
  ones       [1, 1, 1, 1]              every layer gradient exactly zero, x0 = row 0 bit for bit
  pairs      [2, 2, 2]                 attention.* exactly zero
  onelayer   [1, 2, 5], L = 1          Pt is never used
  deep3      [1, 2, 5, 9, 34], L = 3   a middle layer: neither first nor last, so the forward reads
                                       and writes the row-0 buffer and the backward adds into a dt
                                       that already carries the layer above's accumulations
  deep4      [3, 1, 2, 10], L = 4      the deepest stack the kernels accept
and with L = 0 the forward returns the row 0s and the backward has nothing to write."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gradcheck import abs_contributions, check_grad, cu, guard_reference, targets  # noqa: E402

gpu = pytest.mark.gpu
F, H = 1024, 128
P_DROP = 0.3

CASES = {
    "gemv": ([9], 2),
    "mixed": ([1, 2, 5], 2),
    "past8": ([2, 3, 4, 5, 6, 7, 8, 9, 2, 1], 2),
    "tile": ([34, 35], 2),
    "split": (list(itertools.islice(itertools.cycle(range(1, 7)), 70)), 2),
    "ones": ([1, 1, 1, 1], 2),
    "pairs": ([2, 2, 2], 2),
    "onelayer": ([1, 2, 5], 1),
    "deep3": ([1, 2, 5, 9, 34], 3),
    "deep4": ([3, 1, 2, 10], 4),
}
SEEDS = {name: 8100 + i for i, name in enumerate(CASES)}
SEEDS["deep3"], SEEDS["deep4"] = 8300, 8301
# float64 autograd cancels d(a / a) exactly only where the roundings of its two terms agree; they
# do for all six weights of this seed's stars (test_references_are_not_vacuous holds it to that)
SEEDS["pairs"] = 8202
ALL_ZERO = {"pairs": ("attention.",)}
_REF = {}


def forest(sizes):
    """offs, and the CSR of the forest of stars (row 0 of a star has its other rows as sources)."""
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rowptr = np.zeros(int(offs[-1]) + 1, np.int64)
    col, e = [], 0
    for s, n in zip(offs[:-1], sizes):
        rowptr[s] = e
        e += n - 1
        rowptr[s + 1:s + n + 1] = e
        col += list(range(s + 1, s + n))
    return offs, rowptr, np.asarray(col, np.int64)


def layer_stack(x, PG, L, rowptr, col):
    from oracle import torch_ref as R
    for i in range(L):
        x = R.gnn_layer_csr(x, rowptr, col, PG, i)
    return x


def kernel_case(name):
    """Inputs of a kernel-level case: x [V][F], the layer weights, dx0 [B][F], the graph."""
    from azhip.weights import gnn_spec, synthetic_state_dict
    sizes, L = CASES[name]
    rng = np.random.default_rng(SEEDS[name])
    offs, rowptr, col = forest(sizes)
    G = synthetic_state_dict(gnn_spec(F, L), SEEDS[name])
    x = rng.standard_normal((int(offs[-1]), F)).astype(np.float32)
    dx0 = rng.standard_normal((len(sizes), F)).astype(np.float32)
    return sizes, L, offs, rowptr, col, G, x, dx0


def kernel_reference(name):
    """(x0 in float64 and float32, gradients in float64 and float32, S) of the layer tensors."""
    if name not in _REF:
        from oracle import torch_ref as R
        sizes, L, offs, rowptr, col, G, x, dx0 = kernel_case(name)
        GL = {k: v for k, v in G.items() if k.startswith("layers.")}
        assert len(GL) == 10 * L
        starts = torch.as_tensor(offs[:-1].astype(np.int64))

        def rows0(PG):
            dt = next(iter(PG.values())).dtype
            return layer_stack(torch.as_tensor(x).to(dt), PG, L, rowptr, col)[starts]

        def run(PG):
            return (torch.as_tensor(dx0).to(next(iter(PG.values())).dtype) * rows0(PG)).sum()
        out = {}
        # one thread: the exact zeros of `pairs` hang on the last bit of float64 sums, which the
        # number of threads a matrix product is split over would change
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            for dt in (torch.float64, torch.float32):
                P = R.params(GL, dt)
                x0 = rows0(P)
                (torch.as_tensor(dx0).to(dt) * x0).sum().backward()
                out[dt] = (x0.detach().numpy(),
                           {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape))
                            for k, v in P.items()})
            S = abs_contributions(run, R.params(GL, torch.float64))
        finally:
            torch.set_num_threads(threads)
        _REF[name] = (out[torch.float64], out[torch.float32], S)
    return _REF[name]


@pytest.mark.parametrize("name", [n for n in CASES if n != "ones"])
def test_references_are_not_vacuous(name):
    """CPU: the float64 reference of every kernel-level case passes guard_reference."""
    (_, g64), _, S = kernel_reference(name)
    guard_reference(f"star_train/{name}", g64, S, all_zero=ALL_ZERO.get(name, ()))


def run_kernels(name, nan_fill=False):
    """x0 and the layer gradients of one case from the HIP path."""
    from azhip import nets, ops
    sizes, L, offs, rowptr, col, G, x, dx0 = kernel_case(name)
    gnn = nets.PolicyValueGNN(F, L, init=G)
    gnn.params.sync()
    gnn.params.grad_flat.fill_(float("nan") if nan_fill else 0.0)
    GG = gnn.params.grads
    layers = [l.weights() for l in gnn.layers]
    xd, od = cu(x), cu(offs)
    keep = xd.clone()
    x0, save = ops.gnn_star_batch_fwd_train(xd, od, layers)
    grads = [{k[len(l.prefix):]: g for k, g in GG.items() if k.startswith(l.prefix)}
             for l in gnn.layers]
    ops.gnn_star_batch_bwd(xd, od, layers, save, cu(dx0), grads)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep)
    return x0.cpu(), {k: v.cpu().clone() for k, v in GG.items() if k.startswith("layers.")}


@gpu
@pytest.mark.parametrize("name", ["gemv", "mixed", "past8", "tile", "split", "pairs", "onelayer",
                                  "deep3", "deep4"])
def test_star_train_kernels_match_float64(name):
    """x0 and all 10 L layer tensors.  `mixed` and `deep3` run twice, the second time into gradient
    buffers full of NaN: equal bits (no atomics, fixed orders) and every element written.  The
    one-row star of `deep3` passes through its middle layer untouched: x0[b] is row 0 bit for
    bit."""
    (x0_64, g64), (x0_32, g32), S = kernel_reference(name)
    guard_reference(f"star_train/{name}", g64, S, all_zero=ALL_ZERO.get(name, ()))
    x0, got = run_kernels(name)
    sizes = CASES[name][0]
    assert np.isfinite(x0.numpy()).all()
    check_grad(f"star_train/{name}/x0", x0.numpy(), x0_64, x0_32)
    _, _, offs, _, _, _, x, _ = kernel_case(name)
    for b in np.flatnonzero(np.asarray(sizes) == 1):
        assert np.array_equal(x0.numpy()[b], x[offs[b]])
    assert set(got) == set(g64) and len(got) == 10 * CASES[name][1]
    for k in g64:
        if any(s in k for s in ALL_ZERO.get(name, ())):
            assert not got[k].numpy().any(), (name, k)
            continue
        check_grad(f"star_train/{name}/{k}", got[k].numpy(), g64[k], g32[k], S[k])
    if name in ("mixed", "deep3"):
        x0b, gotb = run_kernels(name, nan_fill=True)
        assert torch.equal(x0, x0b)
        for k in got:
            assert torch.equal(got[k], gotb[k]), k


@gpu
def test_one_row_stars_write_zeros():
    """Four one-row stars: every layer gradient is exactly zero (written over NaN) and x0 is
    row 0 bit for bit."""
    x0, got = run_kernels("ones", nan_fill=True)
    x = kernel_case("ones")[6]
    assert np.array_equal(x0.numpy(), x)
    assert len(got) == 20
    for k, g in got.items():
        assert torch.equal(g, torch.zeros_like(g)), k


@gpu
def test_no_layers_returns_row_zero_and_writes_nothing():
    """L = 0: gnn_star_batch_fwd_train gives every star's row 0 bit for bit (x untouched), and
    gnn_star_batch_bwd returns success with nothing to write: x, dx0 and the save buffer keep
    their bits."""
    from azhip import _lib, ops
    sizes = [1, 2, 5, 9]
    offs, _, _ = forest(sizes)
    rng = np.random.default_rng(8400)
    x = rng.standard_normal((int(offs[-1]), F)).astype(np.float32)
    xd, od = cu(x), cu(offs)
    x0, save = ops.gnn_star_batch_fwd_train(xd, od, [])
    torch.cuda.synchronize()
    assert tuple(x0.shape) == (len(sizes), F)
    assert np.array_equal(x0.cpu().numpy(), x[offs[:-1]])
    assert np.array_equal(xd.cpu().numpy(), x)
    dx0 = cu(rng.standard_normal((len(sizes), F)).astype(np.float32))
    keep_dx0 = dx0.clone()
    save.fill_(171)
    keep_save = save.clone()
    assert ops.gnn_star_batch_bwd(xd, od, [], save, dx0, []) is None      # _lib.check passed: rc 0
    torch.cuda.synchronize()
    assert torch.equal(dx0, keep_dx0) and torch.equal(save, keep_save)
    assert np.array_equal(xd.cpu().numpy(), x)
    # the entry point itself, with null layers / save / workspace / gradients: 0, no launch
    import ctypes
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib().az_gnn_star_batch_bwd(P(xd), P(od), len(sizes), int(offs[-1]), F, H, 0, None,
                                          None, ctypes.c_size_t(0), P(dx0), None, None,
                                          ctypes.c_size_t(0), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(dx0, keep_dx0)


# ------------------------------------------------------------------------------ whole step
def _play(game, moves):
    b, p = game.getInitBoard(), 1
    for a in moves:
        b, p = game.getNextState(b, p, a)
    return game.getCanonicalForm(b, p)


def step_case(kind, L=2):
    """(game, boards, net weights W, GNN weights G of L layers, dropout)."""
    from azhip.weights import (connect4_net_spec, gnn_spec, synthetic_state_dict,
                               tictactoe_net_spec)
    if kind == "c4_4x4":
        from connect4.Connect4Game import Connect4Game
        game = Connect4Game(4)
        boards = [_play(game, (0, 1)), _play(game, (2, 2, 2, 2)),          # a full column
                  _play(game, (0, 1, 0, 1, 0, 1, 0)),                       # terminal: one row
                  _play(game, ()), _play(game, (3, 0, 3, 1, 2))]
        assert game.getValidMoves(boards[1], 1)[2] == 0
        assert game.getGameEnded(boards[2], 1) != 0
        W = synthetic_state_dict(connect4_net_spec(4, 5), 611)
        return game, boards, W, synthetic_state_dict(gnn_spec(1024, L), 612), P_DROP
    if kind == "c4_7x6":
        from connect4.Connect4Game import Connect4Game
        game = Connect4Game(7, rows=6)
        boards = [_play(game, (3, 3, 4)), _play(game, (2, 2, 2, 2, 2, 2, 0, 4, 4)),
                  _play(game, (0, 6, 0, 6, 0, 5))]
        W = synthetic_state_dict(connect4_net_spec((7, 6), 8), 621)
        return game, boards, W, synthetic_state_dict(gnn_spec(2688, L), 622), P_DROP
    from tictactoe.TicTacToeGame import TicTacToeGame
    game = TicTacToeGame(3)
    boards = [_play(game, ()), _play(game, (4,)), _play(game, (0, 4, 8, 2)),
              _play(game, (0, 1, 2, 4, 3, 5, 7, 6))]
    W = synthetic_state_dict(tictactoe_net_spec(3, 10), 631)
    return game, boards, W, synthetic_state_dict(gnn_spec(128, L), 632), 0.0


def step_nets(kind, game, W, G, dropout, L=2):
    from types import SimpleNamespace
    from azhip import nets
    g = SimpleNamespace(getBoardSize=lambda: tuple(game.getBoardSize()),
                        getActionSize=lambda: game.getActionSize())
    if kind.startswith("c4"):
        net = nets.Connect4Net(g, {"dropout": dropout}, init=W)
    else:
        net = nets.TicTacToeNet(g, {}, init=W)
    return net, nets.PolicyValueGNN(net.feature_dim, L, init=G)


def step_loss(kind, W, rows, offs, rowptr, col, tpi, tv, m, parts=False, L=2):
    """The GNN step's loss on child stars as a function of the GNN's parameters: the frozen CNN's
    (dropped) features of all V rows, the layers per star, output_transform and the CNN's heads
    on the row 0s, the reference's loss over the B stars."""
    from oracle import torch_ref as R
    from test_gpu_grads_rect import c4_features_rect
    Pn = R.params(W, torch.float64, requires_grad=False)
    starts = torch.as_tensor(offs[:-1].astype(np.int64))

    def run(PG):
        Wn = {k: v.to(next(iter(PG.values())).dtype) for k, v in Pn.items()}
        feats = (c4_features_rect(rows, Wn, m, P_DROP) if kind.startswith("c4")
                 else R.ttt_features(rows, Wn))
        y = R.policy_value_gnn(feats, PG, L, rowptr, col)[starts]
        logp, v = (R.c4_heads if kind.startswith("c4") else R.ttt_heads)(y, Wn)
        if parts:
            B = len(tpi)
            return (-(torch.as_tensor(tpi).to(logp.dtype) * logp).sum() / B,
                    ((torch.as_tensor(tv).to(v.dtype) - v) ** 2).sum() / B)
        return R.losses(logp, v, tpi, tv)
    return run


@gpu
@pytest.mark.parametrize("kind", ["c4_4x4", "c4_7x6", "ttt_3x3"])
def test_gnn_star_grads_on_real_boards(kind):
    """All 24 tensors of T.gnn_star_grads and both loss terms.  Connect4 4x4: five leaves, one
    with a full column and one terminal (a one-row star), dropout 0.3 under an explicit mask over
    the V * F feature elements, read back for the reference; Connect4 7x6: three leaves;
    TicTacToe 3x3: four leaves, the empty board's star has 10 rows."""
    _check_star_step(kind, 2)


@gpu
@pytest.mark.parametrize("L", [0, 3])
def test_gnn_star_grads_at_other_depths(L):
    """The Connect4 4x4 case with gnn_layers 0 (only the four output_transform tensors exist: the
    row 0s go straight into output_transform) and 3 (a middle layer inside the whole step): every
    tensor and both loss terms."""
    _check_star_step("c4_4x4", L)


def _check_star_step(kind, L):
    import stars
    from azhip import ops, train as T
    from gradcheck import ref_grads
    from oracle import torch_ref as R
    game, boards, W, G, dropout = step_case(kind, L)
    rows, offs = stars.board_stars(game, boards)
    sizes = np.diff(offs)
    if kind == "c4_4x4":
        assert sizes.tolist() == [5, 4, 1, 5, 5]
    if kind == "ttt_3x3":
        assert sizes.max() == 10
    B, V, A = len(boards), len(rows), game.getActionSize()
    net, gnn = step_nets(kind, game, W, G, dropout, L)
    Fd = net.feature_dim
    tpi, tv = targets(B, A, 900 + V)
    mask = ops.dropout_mask(V * Fd, dropout, 7000 + V, "cuda") if dropout > 0 else None
    gnn.params.grad_flat.fill_(float("nan"))
    loss = T.gnn_star_grads(net, gnn, cu(rows), cu(offs), cu(tpi), cu(tv), drop_mask=mask)
    got = {k: v.cpu().numpy() for k, v in gnn.params.grads.items()}
    m = mask.cpu().numpy().reshape(V, Fd) if mask is not None else None
    _, rowptr, col = forest(sizes.tolist())
    run = step_loss(kind, W, rows, offs, rowptr, col, tpi, tv, m, L=L)
    g64, g32 = ref_grads(run, G, torch.float64), ref_grads(run, G, torch.float32)
    S = abs_contributions(run, R.params(G, torch.float64))
    assert set(g64) == set(G) == set(got) and len(g64) == 10 * L + 4
    name = f"star_step/{kind}" + ("" if L == 2 else f"/L{L}")
    guard_reference(name, g64, S)
    for k in g64:
        check_grad(f"{name}/{k}", got[k], g64[k], g32[k], S[k])
    parts = step_loss(kind, W, rows, offs, rowptr, col, tpi, tv, m, parts=True, L=L)
    with torch.no_grad():
        l64 = [float(t) for t in parts(R.params(G, torch.float64, requires_grad=False))]
        l32 = [float(t) for t in parts(R.params(G, torch.float32, requires_grad=False))]
    lg = loss.cpu().numpy()
    print(f"{name}: loss {lg.tolist()} ref {l64}")
    check_grad(f"{name}/l_pi", lg[0], l64[0], l32[0])
    check_grad(f"{name}/l_v", lg[1], l64[1], l32[1])


# ------------------------------------------------------------------------------ wrapper
def _wrapper(gnn_layers=2, **kw):
    from types import SimpleNamespace
    from connect4.Connect4Game import Connect4Game
    from connect4.Connect4GNN import Connect4GNNWrapper
    game = Connect4Game(4)
    args = SimpleNamespace(dropout=0.3, gnn_layers=gnn_layers, lr=0.001, epochs=1, batch_size=4,
                           **kw)
    torch.manual_seed(77)
    return game, Connect4GNNWrapper(game, args)


def _gnn_examples(game):
    boards = [_play(game, m) for m in ((), (0, 1), (2, 2, 2, 2), (3, 0, 3, 1, 2), (1, 1, 0),
                                       (0, 1, 0, 1, 0, 1, 0))]
    tpi, tv = targets(len(boards), game.getActionSize(), 41)
    return [(b, 1, None, None, tpi[i], float(tv[i]), None) for i, b in enumerate(boards)]


@gpu
def test_wrapper_trains_on_child_stars():
    """train() with the key on equals a hand-run gnn_star_step on the same draw and seed, bit for
    bit, and leaves the board network untouched; the evaluator then sees the new weights."""
    import stars
    from azhip import train as T
    from test_gpu_star_eval import _float64_star_eval
    game, w = _wrapper(use_gnn=True, gnn_neighbors=True, gnn_neighbors_train=True)
    assert w.game is game
    ex = _gnn_examples(game)
    _, ref = _wrapper(use_gnn=True, gnn_neighbors=True)
    ref.nnet.params.copy_flat_(w.nnet.params.flat)
    ref.gnn.params.copy_flat_(w.gnn.params.flat)
    net_before = w.nnet.params.flat.clone()
    gnn_before = w.gnn.params.flat.clone()
    np.random.seed(5)
    w.train([], ex)
    assert torch.equal(w.nnet.params.flat, net_before)
    assert not torch.equal(w.gnn.params.flat, gnn_before)
    np.random.seed(5)
    idx = np.random.randint(0, len(ex), min(len(ex), 4))
    rows, offs = stars.board_stars(game, [ex[i][0] for i in idx])
    ref.nnet.train()
    ref.gnn.train()
    ref.gnn.params.reset_adam()
    T.gnn_star_step(ref.nnet, ref.gnn, cu(rows), cu(offs),
                    cu(np.stack([ex[i][4] for i in idx]).astype(np.float32)),
                    cu(np.array([ex[i][5] for i in idx], np.float32)), 0.001, seed=1)
    torch.cuda.synchronize()
    assert torch.equal(w.gnn.params.flat, ref.gnn.params.flat)
    board = ex[3][0]
    kids = stars.children(game, board)
    pi, v = w.predict_with_gnn(board, neighbor_states=kids)
    pi64, _, v64 = _float64_star_eval([[np.asarray(board)] + kids], w.nnet.params, w.gnn.params, 2)
    assert np.abs(np.asarray(pi, np.float64) - pi64[0]).max() <= 1e-5
    assert abs(float(v) - float(v64[0])) <= 1e-5


@gpu
def test_wrapper_without_the_key_never_builds_stars(monkeypatch):
    from azhip import train as T

    def boom(*a, **k):
        raise AssertionError("the star path ran without gnn_neighbors_train")
    game, w = _wrapper(use_gnn=True, gnn_neighbors=True)
    monkeypatch.setattr(T, "gnn_star_step", boom)
    monkeypatch.setattr(T, "gnn_star_grads", boom)
    monkeypatch.setattr(type(w), "_gnn_star_batch", boom)
    before = w.gnn.params.flat.clone()
    np.random.seed(5)
    w.train([], _gnn_examples(game))
    assert not torch.equal(w.gnn.params.flat, before)


@gpu
@pytest.mark.parametrize("key", ["gnn_neighbors_train", "gnn_neighbors_lockstep"])
def test_depth_above_the_star_limit_is_rejected_at_construction(key):
    """gnn_layers above ops.STAR_MAX_LAYERS with a key that has no route but the packed-star
    kernels: the wrapper, and a Coach handed a deeper wrapper, raise ValueError naming the limit
    before any game is played -- not AZ_EINVAL inside train() after a self-play iteration.
    Without the keys the same depth builds (predict_star_batch then composes)."""
    import Coach as C
    from azhip import ops
    assert ops.STAR_MAX_LAYERS == 4
    flags = dict(use_gnn=True, gnn_neighbors=True)
    with pytest.raises(ValueError, match=rf"gnn_layers=5 > {ops.STAR_MAX_LAYERS}.*{key}"):
        _wrapper(gnn_layers=5, **flags, **{key: True})
    _wrapper(gnn_layers=4, **flags, **{key: True})             # the limit itself is accepted
    game, deep = _wrapper(gnn_layers=5, **flags)
    assert deep.gnn.num_layers == 5
    args = dict(vars(deep.args), **{key: True})
    with pytest.raises(ValueError, match=rf"gnn_layers=5 > {ops.STAR_MAX_LAYERS}.*{key}"):
        C.Coach(game, deep, args)


# ------------------------------------------------------------------------------ arguments
@gpu
def test_star_train_rejected_arguments():
    """A short save, a misaligned x, a host offs that does not ascend and L = 5 return AZ_EINVAL
    with a message and launch nothing (x0 and the gradients keep their NaNs)."""
    import ctypes
    from azhip import _lib, nets, ops
    B, V = 4, 20
    gnn = nets.PolicyValueGNN(F, 2)
    gnn.params.sync()
    gnn.params.grad_flat.fill_(float("nan"))
    dev = gnn.params.device
    L = _lib.lib()
    x = torch.zeros((V + 1, F), device=dev)
    x0 = torch.full((B, F), float("nan"), device=dev)
    dx0 = torch.zeros((B, F), device=dev)
    nsave = int(L.az_gnn_star_batch_save_bytes(B, V, F, H, 2))
    nws = int(L.az_gnn_star_batch_train_ws_bytes(B, V, F, H, 2))
    save = torch.empty((nsave,), dtype=torch.uint8, device=dev)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    lw = (ops.LayerW * 4)(*[ops.layer_weights(l.weights()) for l in gnn.layers] * 2)
    GG = gnn.params.grads
    lg = (ops.LayerGrads * 4)(*[ops.layer_grads({k[len(l.prefix):]: g for k, g in GG.items()
                                                 if k.startswith(l.prefix)})
                                for l in gnn.layers] * 2)
    hb = ops.HostBuffer(4096)
    ho = hb.view(0, torch.int32, (B + 1,))
    good = [0, 5, 6, 15, 20]
    P = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)  # noqa: E731
    sz = ctypes.c_size_t

    def fwd(offs=good, xo=0, ns=nsave, Lc=2):
        ho.numpy()[:] = offs
        return L.az_gnn_star_batch_fwd_train(P(x, xo), P(ho), B, V, F, H, Lc, lw, P(x0), P(save),
                                             sz(ns), P(ws), sz(nws), None)

    def bwd(offs=good, xo=0, ns=nsave, Lc=2):
        ho.numpy()[:] = offs
        return L.az_gnn_star_batch_bwd(P(x, xo), P(ho), B, V, F, H, Lc, lw, P(save), sz(ns),
                                       P(dx0), lg, P(ws), sz(nws), None)
    failed = []

    def run():
        try:
            for fn in (fwd, bwd):
                for kw, msg in ((dict(ns=nsave - 1), b"save of"), (dict(xo=4), b"alignment"),
                                (dict(offs=[0, 5, 5, 15, 20]), b"not ascending"),
                                (dict(offs=[0, 5, 6, 15, 19]), b"offs[0]"),
                                (dict(Lc=5), b"bad shape")):
                    assert fn(**kw) == -1, (fn.__name__, kw)
                    assert msg in L.az_last_error(), (kw, L.az_last_error())
        except BaseException as ex:   # reported on the test's own thread
            failed.append(ex)

    # az_last_error is per thread: the rejected calls run on a thread of their own, so the main
    # thread keeps the empty message tests/test_lib_abi.py expects when the whole suite runs in
    # one process (as tests/test_gpu_star_batch.py does)
    import threading
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failed:
        raise failed[0]
    torch.cuda.synchronize()
    assert bool(torch.isnan(x0).all()) and bool(torch.isnan(gnn.params.grad_flat).all())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(x0).any())
    for k, g in GG.items():                     # (the flat buffer's alignment gaps keep their NaNs)
        assert bool(torch.isnan(g).any()) == (not k.startswith("layers.")), k
