"""Batch-invariant evaluation on the MI355X (config key batch_invariant).

1. az_gemm_exact_f32 against the CPU restatement of its contract (tests/exact_ref.py: one fmaf
   chain per segment of az_gemm_exact_plan in ascending k, segment sums added in order, bias,
   activation) -- np.array_equal, with NaN behind every operand.
2. Row invariance of the GEMM: a row's bits at M = 257 (and at the row count from which a block
   walks the segments itself), alone, at another position of another batch, and twice.
3. az_eval_exact_fwd on four boards: every row at B = 1 .. 321 equals that board's B = 1 call;
   float64 parity at the project's 1e-5; device buffers and mapped host memory give equal bits.
4. The wrappers under the key: predict_both rows at B = 1 .. 513 equal the one-board calls,
   predict / predict_with_gnn equal those rows, batches above the scratch capacity run in chunks.
5. Self-play: 20 episodes at G = 1, G = 12 (one lane) and G = 20 (two lanes) give identical
   examples, three of them equal to the sequential Coach.executeEpisode."""
from types import SimpleNamespace

import numpy as np
import pytest

import exact_ref
from conftest import assert_close

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
NAN = float("nan")


# ------------------------------------------------------------------ 1. GEMM == the CPU chain
GEMM_SHAPES = [(16, 4), (36, 36), (132, 260), (512, 1152)]
GEMM_ROWS = (1, 2, 31, 33, 65)
_OPS, _REF = {}, {}


def _operands(N, K, M):
    """(A [M][K], W [N][K], bias [N]) uniform in [-1, 1], one draw per shape."""
    if (N, K, M) not in _OPS:
        rng = np.random.default_rng(1000 * N + K)
        _OPS[(N, K, M)] = tuple(rng.uniform(-1, 1, s).astype(np.float32)
                                for s in ((M, K), (N, K), (N,)))
    return _OPS[(N, K, M)]


def _chain(N, K, M, biased):
    """The CPU chain of all M rows, computed once per case: the smaller calls are its prefixes."""
    if (N, K, M, biased) not in _REF:
        if exact_ref.lib() is None:
            pytest.skip("no C++ compiler")
        A, W, b = _operands(N, K, M)
        _REF[(N, K, M, biased)] = exact_ref.linear(A, W, b if biased else None, relu=biased)
    return _REF[(N, K, M, biased)]


def _padded(a, rows, dev):
    """`a` in the corner of a NaN-filled allocation: `rows` NaN rows behind it and 4 NaN columns
    beside it (k past K), returned as the strided view of the data."""
    buf = torch.full((a.shape[0] + rows, a.shape[1] + 4), NAN, device=dev)
    buf[:a.shape[0], :a.shape[1]] = torch.from_numpy(a).to(dev)
    return buf[:a.shape[0], :a.shape[1]]


def _gemm(A, W, b, biased, dev):
    from azhip import ops
    M, N = A.shape[0], W.shape[0]
    x, w = _padded(A, 130, dev), _padded(W, 70, dev)
    out = torch.full((M + 8, N), NAN, device=dev)
    ops.linear_exact(x, w, torch.from_numpy(b).to(dev) if biased else None,
                     ops.ACT_RELU if biased else ops.ACT_NONE, out=out, M=M)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[M:]).all()                       # nothing stored past row M
    return got[:M]


@pytest.mark.parametrize("biased", [True, False], ids=["bias_relu", "plain"])
@pytest.mark.parametrize("N,K", GEMM_SHAPES)
def test_gemm_equals_cpu_chain(N, K, biased):
    """M = 1, 2, 31, 33, 65 (inside one 32-row MFMA tile, across two, past the second wave) at
    N, K that are no multiple of the 64-column tile, the 32-k tile or the 128-k segment; the rows
    behind A's row M and W's row N, and the columns behind K, hold NaN.  Values are compared, not
    the sign of a zero (a padded fmaf(0, 0, -0) gives +0)."""
    dev = torch.device("cuda")
    A, W, b = _operands(N, K, max(GEMM_ROWS))
    ref = _chain(N, K, max(GEMM_ROWS), biased)
    for M in GEMM_ROWS:
        got = _gemm(A[:M], W, b, biased, dev)
        assert np.array_equal(got, ref[:M]), (N, K, M, float(np.abs(got - ref[:M]).max()))


def test_gemm_equals_cpu_chain_at_3136():
    """M = 3, N = K = 3136: 11 segments over 49 column tiles, the widest layer of the networks."""
    dev = torch.device("cuda")
    A, W, b = _operands(3136, 3136, 3)
    got = _gemm(A, W, b, True, dev)
    assert np.array_equal(got, _chain(3136, 3136, 3, True))


# ------------------------------------------------------------------ 2. GEMM row invariance
@pytest.mark.parametrize("N,big", [(1024, 900), (3136, 257)])
def test_gemm_rows_do_not_depend_on_the_batch(N, big):
    """Row r of an M = 257 call equals the same row alone (M = 1), at another position of an
    M = 40 call and in a repeated call, torch.equal.  `big` is a row count at which the tile grid
    alone fills the GPU and a block walks all the segments itself instead of leaving their sums
    in the workspace (M = 257 at N = 3136; M = 900 at N = 1024): the same bits again, and three
    of its rows equal the CPU chain."""
    from azhip import ops
    dev = torch.device("cuda")
    K, r = N, 200
    rng = np.random.default_rng(N)
    A = torch.from_numpy(rng.uniform(-1, 1, (max(big, 257), K)).astype(np.float32)).to(dev)
    W = torch.from_numpy(rng.uniform(-1, 1, (N, K)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rng.uniform(-1, 1, N).astype(np.float32)).to(dev)
    L = ops._lib.lib()
    assert L.az_gemm_exact_ws_bytes(big, N, K) == 0 and L.az_gemm_exact_ws_bytes(40, N, K) > 0
    run = lambda x: ops.linear_exact(x, W, b, ops.ACT_RELU)  # noqa: E731
    c257 = run(A[:257])
    assert torch.equal(run(A[:257]), c257)                                     # twice
    assert torch.equal(run(A[r:r + 1])[0], c257[r])                            # alone
    other = torch.from_numpy(rng.uniform(-1, 1, (40, K)).astype(np.float32)).to(dev)
    other[7] = A[r]
    assert torch.equal(run(other)[7], c257[r])                                 # elsewhere
    cbig = run(A[:big])
    assert torch.equal(cbig[:257], c257[:big][:257])
    assert torch.equal(run(A[big - 1:big])[0], cbig[big - 1])
    if exact_ref.lib() is not None:
        rows = [0, r, big - 1]
        ref = exact_ref.linear(A[rows].cpu().numpy(), W.cpu().numpy(), b.cpu().numpy(), relu=True)
        assert np.array_equal(cbig[rows].cpu().numpy(), ref)


# ------------------------------------------------------------------ 3. the evaluator
EVAL_BOARDS = [("c4", 7, 7), ("c4", 4, 4), ("c4", 7, 6), ("ttt", 4, 4)]
EVAL_B = (1, 2, 9, 33, 321)          # across 8 rows and the 7x7 trunk's one-launch limit of 320
MAX_B = 321
_NETS, _EVALS, _ONE = {}, {}, {}


def _nets(board):
    """(board network, PolicyValueGNN with no layers, A) in eval mode, torch default init under a
    fixed seed; one board's networks at a time."""
    if board not in _NETS:
        from azhip import nets
        _NETS.clear()
        _EVALS.clear()
        _ONE.clear()
        kind, nx, ny = board
        A = nx + 1 if kind == "c4" else nx * ny + 1
        torch.manual_seed(7000 + 10 * nx + ny)
        game = SimpleNamespace(getBoardSize=lambda: (nx, ny), getActionSize=lambda: A)
        cls = nets.Connect4Net if kind == "c4" else nets.TicTacToeNet
        nnet = cls(game, {"dropout": 0.0}).eval()
        gnn = nets.PolicyValueGNN(nnet.feature_dim, 0).eval()
        _NETS[board] = (nnet, gnn, A)
    return _NETS[board]


def _eval_boards(board, B=MAX_B):
    _, nx, ny = board
    b = np.random.default_rng(nx * 100 + ny).integers(-1, 2, size=(B, nx, ny)).astype(np.int8)
    b[0] = 0
    b[1] = 1
    return b


def _evaluator(board):
    if board not in _EVALS:
        from azhip import ops
        nnet, gnn, A = _nets(board)
        dev = nnet.params.device
        ev = ops.EvalExact(nnet.params, gnn.params, ops.exact_board(nnet), A, MAX_B, dev)
        outs = [torch.empty((MAX_B, A) if i % 2 == 0 else (MAX_B,), device=dev) for i in range(4)]
        _EVALS[board] = (ev, outs)
    return _EVALS[board]


def _run(board, boards_t, B, outs=None, keep_logp=False):
    """One az_eval_exact_fwd call with every scratch buffer and output NaN before it -> (pi, v,
    gpi, gv) as numpy; rows B.. must stay NaN."""
    from azhip import ops
    ev, dev_outs = _evaluator(board)
    outs = dev_outs if outs is None else outs
    for t in (ev.feat, ev.h1, ev.h2, ev.hidden, ev.y, ev.logp, ev.glogp, *outs):
        if t is not None:
            t.fill_(NAN)
    ev.ws.view(torch.float32).fill_(NAN)
    ops.eval_exact(ev, boards_t, B, *outs)
    torch.cuda.synchronize()
    got = [o.cpu().numpy() if o.is_cuda else o.numpy().copy() for o in outs]
    for a in got:
        assert np.isnan(a[B:]).all() and np.isfinite(a[:B]).all(), (board, B)
    got = [a[:B].copy() for a in got]
    if keep_logp:
        got += [ev.logp[:B].cpu().numpy(), ev.glogp[:B].cpu().numpy()]
    return got


def _one_by_one(board):
    """Every board of _eval_boards evaluated alone (B = 1): the rows everything else must equal."""
    if board not in _ONE:
        nnet = _nets(board)[0]
        bt = torch.from_numpy(_eval_boards(board)).to(nnet.params.device)
        rows = [_run(board, bt[i:i + 1].contiguous(), 1) for i in range(MAX_B)]
        _ONE[board] = [np.concatenate([r[k] for r in rows]) for k in range(4)]
    return _ONE[board]


@pytest.mark.parametrize("board", EVAL_BOARDS, ids=lambda b: f"{b[0]}_{b[1]}x{b[2]}")
def test_eval_rows_are_batch1_bits_at_every_batch(board):
    """B = 1, 2, 9, 33, 321: every row of pi, v, gpi, gv is bit-identical to that board's own
    B = 1 call, and to the same board at another position (the batch reversed)."""
    nnet = _nets(board)[0]
    dev = nnet.params.device
    boards = _eval_boards(board)
    one = _one_by_one(board)
    for B in EVAL_B:
        got = _run(board, torch.from_numpy(boards[:B].copy()).to(dev), B)
        for k in range(4):
            assert np.array_equal(got[k], one[k][:B]), (board, B, k)
    for B in (33, 321):
        got = _run(board, torch.from_numpy(boards[:B][::-1].copy()).to(dev), B)
        for k in range(4):
            assert np.array_equal(got[k], one[k][:B][::-1]), (board, B, k)


@pytest.mark.parametrize("board", EVAL_BOARDS, ids=lambda b: f"{b[0]}_{b[1]}x{b[2]}")
def test_eval_from_host_buffers_equals_device_buffers(board):
    """Boards read from and outputs written to mapped host memory (ops.HostBuffer views): the bits
    of the device-buffer call."""
    from azhip import ops
    nnet, _, A = _nets(board)
    _, nx, ny = board
    B = 33
    boards = _eval_boards(board)[:B]
    one = _one_by_one(board)
    off = [0, 4096]
    for k in (A, 1, A, 1):
        off.append(off[-1] + (4 * B * k + 255) // 256 * 256)
    hb = ops.HostBuffer(off[-1])
    hin = hb.view(0, torch.int8, (B, nx, ny))
    hin.numpy()[:] = boards
    outs = [hb.view(off[1 + j], torch.float32, (B, k) if k > 1 else (B,))
            for j, k in enumerate((A, 1, A, 1))]
    got = _run(board, hin, B, outs=outs)
    for k in range(4):
        assert np.array_equal(got[k], one[k][:B]), (board, k)
    hb.close()


def _float64_eval(board, boards, W, G):
    """The network in float64: the convolutions in torch double (the board [cols][rows] is the
    image [1][cols][rows]), output_transform and the heads from oracle.nets."""
    import torch.nn.functional as Fn
    from oracle import nets as O
    Wn = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in W.views.items()}
    G64 = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in G.views.items()}
    t = lambda k: torch.from_numpy(Wn[k])  # noqa: E731
    x = torch.from_numpy(boards).double()[:, None]
    x = Fn.relu(Fn.conv2d(x, t("conv1.weight"), t("conv1.bias"), padding=1))
    x = Fn.relu(Fn.conv2d(x, t("conv2.weight"), t("conv2.bias"), padding=1))
    if board[0] == "ttt":
        x = Fn.relu(Fn.conv2d(x, t("conv3.weight"), t("conv3.bias"), padding=0))
    f = x.flatten(1).numpy()
    heads = O.c4_heads if board[0] == "c4" else O.ttt_heads
    logp, v = heads(f, Wn)
    glogp, gv = heads(O.output_transform(f, G64), Wn)
    return logp, v, glogp, gv


@pytest.mark.parametrize("board", EVAL_BOARDS, ids=lambda b: f"{b[0]}_{b[1]}x{b[2]}")
def test_eval_matches_float64(board):
    """pi, log pi and v of both heads against the float64 path at 33 boards: the project's 1e-5."""
    nnet, gnn, _ = _nets(board)
    B = 33
    boards = _eval_boards(board)[:B]
    logp, v, glogp, gv = _float64_eval(board, boards, nnet.params, gnn.params)
    got = _run(board, torch.from_numpy(boards.copy()).to(nnet.params.device), B, keep_logp=True)
    tag = f"eval_exact/{board[0]}_{board[1]}x{board[2]}"
    for name, g, r in (("pi", got[0], np.exp(logp)), ("v", got[1], v), ("logp", got[4], logp),
                       ("gnn_pi", got[2], np.exp(glogp)), ("gnn_v", got[3], gv),
                       ("gnn_logp", got[5], glogp)):
        worst = assert_close(f"{tag}/{name}", g, r, TOL)
        print(f"{tag}/{name}: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")


# ------------------------------------------------------------------ 4. the wrappers
WRAP_B = (1, 8, 9, 64, 513)


def _wrapper(kind, nx, ny, seed, **extra):
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Game import Connect4Game
    from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    torch.manual_seed(seed)
    args = SimpleNamespace(dropout=0.3, gnn_layers=2, batch_invariant=True, **extra)
    if kind == "c4":
        return Connect4GNNWrapper(Connect4Game(nx, rows=ny), args)
    return TicTacToeGNNWrapper(TicTacToeGame(nx), args)


def _game_boards(nx, ny, B, seed):
    return np.random.default_rng(seed).integers(-1, 2, size=(B, nx, ny)).astype(np.int8)


@pytest.mark.parametrize("kind,nx,ny", [("c4", 4, 4), ("c4", 7, 6), ("ttt", 4, 4)])
def test_wrapper_rows_equal_one_board_calls(kind, nx, ny, monkeypatch):
    """predict_both(boards[:B]) for B = 1, 8, 9, 64, 513: every row equals predict_both of that
    board alone; predict and predict_with_gnn (and their batched forms) equal those rows; a
    second wrapper with the same weights whose scratch holds 256 rows runs B = 513 as three
    chunks with the same bits; batch_invariant_rows says so."""
    from azhip import wrappers
    w = _wrapper(kind, nx, ny, 50 + nx + ny)
    assert w.batch_invariant_rows >= 1 << 20
    boards = _game_boards(nx, ny, max(WRAP_B), 9 * nx + ny)
    one = [w.predict_both(boards[i:i + 1]) for i in range(max(WRAP_B))]
    one = [np.concatenate([o[k] for o in one]) for k in range(4)]
    for B in WRAP_B:
        got = w.predict_both(boards[:B])
        for k in range(4):
            assert np.array_equal(got[k], one[k][:B]), (kind, nx, ny, B, k)
    for i in (0, 5, 300):
        pi, v = w.predict(boards[i])
        gpi, gv = w.predict_with_gnn(boards[i])
        assert np.array_equal(pi, one[0][i]) and v == one[1][i]
        assert np.array_equal(gpi, one[2][i]) and gv == one[3][i]
    pi, v = w.predict_batch(boards[:70])
    gpi, gv = w.predict_batch_with_gnn(boards[:70])
    for k, a in enumerate((pi, v, gpi, gv)):
        assert np.array_equal(a, one[k][:70]), k
    got = w.predict_both_async(boards[:9]).result()
    assert all(np.array_equal(got[k], one[k][:9]) for k in range(4))
    g = w._graph1("both")
    assert all(np.array_equal(a, one[k][:3]) for k, a in enumerate(g.run_rows(boards[:3])))
    # chunks: the same weights in a wrapper whose device scratch holds 256 rows
    monkeypatch.setattr(wrappers._ExactBatch, "CAP", 256)
    w2 = _wrapper(kind, nx, ny, 50 + nx + ny)
    w2.nnet.load_state_dict(w.nnet.params.cpu_state_dict())
    w2.gnn.load_state_dict(w.gnn.params.cpu_state_dict())
    got = w2.predict_both(boards[:513])
    assert w2._exact_directs[None].cap == 256
    for k in range(4):
        assert np.array_equal(got[k], one[k][:513]), (kind, nx, ny, "chunks", k)


def test_wrapper_rejects_a_board_without_a_fused_trunk():
    """The key on a 9x9 Connect4 board or a 4x6 one: ValueError when the wrapper is built."""
    for nx, ny in ((9, 9), (4, 6)):
        with pytest.raises(ValueError, match="batch_invariant.*fused trunk"):
            _wrapper("c4", nx, ny, 1)


def test_cnn_wrapper_rows_equal_one_board_calls():
    """The CNN-only wrappers take the key too (no GNN tail in the descriptor)."""
    from connect4.Connect4Net import Connect4NNetWrapper
    from connect4.Connect4Game import Connect4Game
    torch.manual_seed(3)
    w = Connect4NNetWrapper(Connect4Game(5, rows=4),
                            SimpleNamespace(dropout=0.3, batch_invariant=True))
    boards = _game_boards(5, 4, 70, 4)
    pi, v = w.predict_batch(boards)
    for i in (0, 9, 69):
        p1, v1 = w.predict(boards[i])
        assert np.array_equal(p1, pi[i]) and v1 == v[i]
    got = w.predict_batch_async(boards[:9]).result()
    assert np.array_equal(got[0], pi[:9]) and np.array_equal(got[1], v[:9]) and got[2] is None


# ------------------------------------------------------------------ 5. self-play
def test_selfplay_examples_do_not_depend_on_parallel_games(monkeypatch):
    """Connect4 4x4, GNN wrapper under the key, 12 simulations, 20 episodes with seed = episode:
    play_episodes_engine at G = 1, at G = 12 with one lane and at G = 20 with two lanes gives
    identical examples per episode, and three of them are the sequential Coach.executeEpisode's
    (batch-1 predict / predict_with_gnn).  The launches' row counts are recorded: batches of more
    than 8 rows -- where the default routes leave the batch-1 arithmetic -- must have occurred."""
    import lockstep_parity as LP
    from selfplay import play_episodes_engine
    from test_mcts_golden import Args
    from azhip.build import build_host
    build_host(verbose=False)
    w = _wrapper("c4", 4, 4, 77)
    game = w.game
    args = Args(numMCTSSims=12, cpuct=1.0, tempThreshold=6, use_gnn=True, expand_by=3,
                batch_invariant=True)
    rows = []
    orig = w._exact
    monkeypatch.setattr(w, "_exact", lambda boards, kind, stream=None: (
        rows.append(len(boards)), orig(boards, kind, stream))[1])
    eps = list(range(20))
    seeds = {e: e for e in eps}
    runs = []
    for G, lanes in ((1, 1), (12, 1), (20, 2)):
        n0 = len(rows)
        runs.append(play_episodes_engine(game, w, args, eps, seeds, parallel_games=G, threads=2,
                                         lanes=lanes))
        assert max(rows[n0:]) == 1 if G == 1 else max(rows[n0:]) > 8, (G, max(rows[n0:]))

    def same(x, y):
        return len(x) == len(y) and all(
            len(a) == len(b) and all(np.array_equal(np.asarray(p), np.asarray(q))
                                     for p, q in zip(a, b)) for a, b in zip(x, y))

    for e in eps:
        for other in runs[1:]:
            assert same(runs[0][e][0], other[e][0]), ("std", e)
            assert same(runs[0][e][1], other[e][1]), ("gnn", e)
        assert len(runs[0][e][0]) > 0 and len(runs[0][e][1]) > 0
    for e in (0, 7, 19):
        seq = LP.sequential(game, w, args, e)
        assert same(seq["std"], runs[2][e][0]), ("sequential std", e)
        assert same(seq["gnn"], runs[2][e][1]), ("sequential gnn", e)
