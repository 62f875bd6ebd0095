"""Training on child stars, the host side: stars.board_stars (the helper MCTS.leaf_children and
NetWrapper._train share) against [board] + leaf_children(board) on both of its routes, the
gnn_neighbors_train key's way through Coach and main.py, and the host-side checks of the new entry
points (no GPU)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest


class Args(SimpleNamespace):
    def __getitem__(self, k):
        return getattr(self, k)

    def get(self, k, default=None):
        return getattr(self, k, default)


@pytest.fixture(scope="module", autouse=True)
def host_lib():
    from azhip.build import build_host
    build_host(verbose=False)
    import mcts_native
    return mcts_native.lib()


def _games():
    from connect4.Connect4Game import Connect4Game
    from tictactoe.TicTacToeGame import TicTacToeGame
    return [("c4_4x4", Connect4Game(4), 14), ("c4_7x6", Connect4Game(7, rows=6), 36),
            ("ttt_3", TicTacToeGame(3), 8)]


def _positions(game, rng, count, max_moves):
    """Reachable canonical positions; a game that ends on the way contributes its terminal board."""
    out = []
    while len(out) < count:
        b, p = game.getInitBoard(), 1
        for _ in range(rng.integers(0, max_moves)):
            a = rng.choice(np.flatnonzero(game.getValidMoves(b, p)))
            b, p = game.getNextState(b, p, a)
            if game.getGameEnded(b, p) != 0:
                break
        out.append(game.getCanonicalForm(b, p))
    return out


@pytest.mark.parametrize("gi", range(3))
def test_board_stars_equal_leaf_children_on_both_routes(gi):
    import stars
    from MCTS import MCTS
    name, game, max_moves = _games()[gi]
    boards = _positions(game, np.random.default_rng(700 + gi), 120, max_moves)
    ended = [game.getGameEnded(b, 1) != 0 for b in boards]
    assert any(ended) and not all(ended)
    kids = MCTS(game, None, Args()).leaf_children
    want = [[np.asarray(b)] + ([] if e else kids(b)) for b, e in zip(boards, ended)]
    # leaf_children is the helper's own step, unchanged: the reference expression
    for b in boards[:20]:
        v = game.getValidMoves(b, 1)
        ref = [game.getCanonicalForm(*game.getNextState(b, 1, a))
               for a in range(game.getActionSize()) if v[a]]
        got = kids(b)
        assert len(got) == len(ref) and all(np.array_equal(x, y) for x, y in zip(got, ref))
    offs_want = np.concatenate([[0], np.cumsum([len(s) for s in want])])
    rows_want = np.stack([r for s in want for r in s]).astype(np.int8)
    for native in (True, False, None):
        rows, offs = stars.board_stars(game, boards, native=native)
        assert rows.dtype == np.int8 and offs.dtype == np.int32, native
        assert np.array_equal(offs, offs_want), native
        assert np.array_equal(rows, rows_want), native
    # without terminal boards the star is exactly [board] + leaf_children(board)
    live = [b for b, e in zip(boards, ended) if not e]
    rows, offs = stars.board_stars(game, live)
    assert np.array_equal(rows, np.stack([r for b in live for r in [np.asarray(b)] + kids(b)]))
    if name == "ttt_3":
        assert max(np.diff(offs)) == 10


def test_terminal_and_full_column_boards():
    import stars
    from connect4.Connect4Game import Connect4Game
    game = Connect4Game(4)
    b, p = game.getInitBoard(), 1
    for a in (0, 1, 0, 1, 0, 1, 0):              # player 1 fills column 0: four in a row
        b, p = game.getNextState(b, p, a)
    won = game.getCanonicalForm(b, p)
    assert game.getGameEnded(won, 1) != 0
    b, p = game.getInitBoard(), 1
    for a in (2, 2, 2, 2):                       # column 2 full, nobody has won
        b, p = game.getNextState(b, p, a)
    full = game.getCanonicalForm(b, p)
    assert game.getGameEnded(full, 1) == 0 and game.getValidMoves(full, 1)[2] == 0
    for native in (True, False):
        rows, offs = stars.board_stars(game, [won, full, won], native=native)
        assert offs.tolist() == [0, 1, 5, 6]
        assert np.array_equal(rows[0], won) and np.array_equal(rows[5], won)
        assert np.array_equal(rows[1], full)
    rows, offs = stars.board_stars(game, [])
    assert rows.shape == (0, 4, 4) and offs.tolist() == [0]


def test_python_route_serves_a_game_the_engine_does_not_know():
    """A game class of another name takes the Python route by default; native=True raises."""
    import stars
    from tictactoe.TicTacToeGame import TicTacToeGame

    class Other(TicTacToeGame):
        pass
    game = Other(3)
    board = game.getCanonicalForm(game.getInitBoard(), 1)
    rows, offs = stars.board_stars(game, [board])
    assert offs.tolist() == [0, 10]
    with pytest.raises(ValueError):
        stars.board_stars(game, [board], native=True)


class StubNet:
    def __init__(self, game, args=None):
        self.A = game.getActionSize()

    def predict(self, board):
        return np.full(self.A, 1.0 / self.A, np.float32), np.float32(0.0)

    predict_with_gnn = predict


def test_coach_needs_use_gnn_and_gnn_neighbors():
    import Coach as C
    from connect4.Connect4Game import Connect4Game
    game = Connect4Game(4)
    base = dict(numEps=1, numMCTSSims=2, cpuct=1.0, tempThreshold=3, expand_by=1)
    for bad in (dict(gnn_neighbors_train=True),
                dict(gnn_neighbors_train=True, use_gnn=True),
                dict(gnn_neighbors_train=True, gnn_neighbors=True),
                dict(gnn_neighbors_train=True, use_gnn=False, gnn_neighbors=True),
                dict(gnn_neighbors_train=True, use_gnn=True, gnn_neighbors=False)):
        with pytest.raises(ValueError, match="gnn_neighbors_train.*use_gnn.*gnn_neighbors"):
            C.Coach(game, StubNet(game), Args(**base, **bad))
    assert C.Coach(game, StubNet(game), Args(use_gnn=True, gnn_neighbors=True,
                                             gnn_neighbors_train=True, **base))
    assert C.Coach(game, StubNet(game), Args(use_gnn=True, gnn_neighbors=True, **base))
    assert C.Coach(game, StubNet(game), Args(**base))


def test_coach_rejects_a_depth_beyond_the_star_kernels():
    """A network with more GNN layers than ops.STAR_MAX_LAYERS under gnn_neighbors_train or
    gnn_neighbors_lockstep: ValueError naming the limit when the Coach is built, not AZ_EINVAL
    inside train() after a self-play iteration.  The limit itself, and a deeper network without
    the keys, are accepted."""
    import Coach as C
    from azhip import ops
    from connect4.Connect4Game import Connect4Game
    game = Connect4Game(4)
    base = dict(numEps=1, numMCTSSims=2, cpuct=1.0, tempThreshold=3, expand_by=1, use_gnn=True,
                gnn_neighbors=True)

    def net(layers):
        class Deep(StubNet):
            gnn = SimpleNamespace(num_layers=layers)
        return Deep(game)
    assert ops.STAR_MAX_LAYERS == 4
    for key in ("gnn_neighbors_train", "gnn_neighbors_lockstep"):
        with pytest.raises(ValueError, match=rf"gnn_layers=5 > 4.*{key}"):
            C.Coach(game, net(5), Args(**base, **{key: True}))
        assert C.Coach(game, net(4), Args(**base, **{key: True}))
    assert C.Coach(game, net(5), Args(**base))


def test_frozenlake_rejects_the_key():
    """FrozenLake has no GNN version, so use_gnn is never set for it: the key raises."""
    import Coach as C
    import main
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    args = main.config_to_args(main.load_config(os.path.join(main.HERE, "frozenlake",
                                                             "config.yaml")))
    assert args.gnn_neighbors_train is False
    args.gnn_neighbors_train = True
    game = FrozenLakeGame(4)
    with pytest.raises(ValueError, match="gnn_neighbors_train"):
        C.Coach(game, StubNet(game), args)


def test_main_carries_the_key(tmp_path):
    import main
    import yaml
    cfg = tmp_path / "config.yaml"
    doc = {"game": {"board_size": 4}, "training": {"checkpoint_path": str(tmp_path / "ck")},
           "neural_network": {"use_gnn": True}}
    cfg.write_text(yaml.safe_dump(doc))
    base = ["--game", "connect4", "--use_gnn", "--config", str(cfg)]
    assert main.parse(base).gnn_neighbors_train is None
    assert not main.build_args(main.parse(base)).get("gnn_neighbors_train", False)
    a = main.build_args(main.parse(base + ["--gnn_neighbors", "--gnn_neighbors_train"]))
    assert a.gnn_neighbors is True and a.gnn_neighbors_train is True
    doc["selfplay"] = {"gnn_neighbors": True, "gnn_neighbors_train": True}
    cfg.write_text(yaml.safe_dump(doc))
    assert main.build_args(main.parse(base)).gnn_neighbors_train is True
    for name in ("connect4", "tictactoe", "frozenlake"):     # the shipped configs name it, off
        shipped = main.config_to_args(main.load_config(os.path.join(main.HERE, name,
                                                                    "config.yaml")))
        assert shipped.gnn_neighbors_train is False


def test_star_train_host_checks_without_gpu():
    """Shape, null-pointer, alignment, save and workspace checks run on the host before any HIP
    call."""
    import ctypes
    import threading
    from azhip import _lib
    from azhip.build import build
    build(verbose=False)
    L = _lib.load()
    save_b, ws_b = L.az_gnn_star_batch_save_bytes, L.az_gnn_star_batch_train_ws_bytes
    assert save_b(4, 20, 1024, 128, 2) == 2 * save_b(4, 20, 1024, 128, 1) > 0
    assert ws_b(4, 20, 1024, 128, 2) > 0
    # what the header says a layer keeps, at least
    assert save_b(4, 20, 1024, 128, 1) >= 4 * (20 * 256 + 4 * 256 + 4 * 2048 + 3 * 4 * 1024 + 20 + 4)
    for bad in ((0, 20, 1024, 128, 2), (4, 3, 1024, 128, 2), (4, 20, 1000, 128, 2),
                (4, 20, 1024, 126, 2), (4, 20, 1024, 128, 5), (4, 20, 1024, 2048, 2)):
        assert save_b(*bad) == 0 and ws_b(*bad) == 0, bad
    fwd, bwd = L.az_gnn_star_batch_fwd_train, L.az_gnn_star_batch_bwd
    lw, lg = (_lib.LayerW * 4)(), (_lib.LayerGrads * 4)()
    buf = (ctypes.c_char * 8192)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    big = 1 << 40
    assert fwd(None, None, 0, 0, 1024, 128, 2, lw, None, None, 0, None, 0, None) == 0   # B == 0
    assert bwd(None, None, 0, 0, 1024, 128, 2, lw, None, 0, None, lg, None, 0, None) == 0
    x, offs, x0, sv, ws = p, p + 1024, p + 2048, p + 3072, p + 4096
    fcases = [((x, offs, 4, 20, 1024, 128, 5, lw, x0, sv, big, ws, big), b"bad shape"),
              ((x, offs, 4, 20, 1000, 128, 2, lw, x0, sv, big, ws, big), b"bad shape"),
              ((None, offs, 4, 20, 1024, 128, 2, lw, x0, sv, big, ws, big), b"null"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, None, sv, big, ws, big), b"null"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, x0, None, big, ws, big), b"null"),
              ((x + 4, offs, 4, 20, 1024, 128, 2, lw, x0, sv, big, ws, big), b"alignment"),
              ((x, offs + 2, 4, 20, 1024, 128, 2, lw, x0, sv, big, ws, big), b"alignment"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, x, sv, big, ws, big), b"alias"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, x0, sv, 1024, ws, big), b"save of"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, x0, sv, big, ws, 1024), b"workspace of"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, x0, sv, big, ws, big), b"null weight")]
    bcases = [((x, offs, 4, 20, 1024, 128, 5, lw, sv, big, x0, lg, ws, big), b"bad shape"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, sv, big, None, lg, ws, big), b"null"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, sv, big, x0 + 4, lg, ws, big), b"aligned"),
              ((x + 4, offs, 4, 20, 1024, 128, 2, lw, sv, big, x0, lg, ws, big), b"alignment"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, sv, 1024, x0, lg, ws, big), b"save of"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, sv, big, x0, lg, ws, 1024), b"workspace of"),
              ((x, offs, 4, 20, 1024, 128, 2, lw, sv, big, x0, lg, ws, big), b"null weight")]
    failed = []

    def run():
        try:
            for fn, cases in ((fwd, fcases), (bwd, bcases)):
                for a, msg in cases:
                    assert fn(*a, None) == -1, msg
                    assert msg in L.az_last_error(), (msg, L.az_last_error())
        except BaseException as ex:   # reported on the test's own thread
            failed.append(ex)

    # az_last_error is per thread: the rejected calls run on a thread of their own
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failed:
        raise failed[0]
