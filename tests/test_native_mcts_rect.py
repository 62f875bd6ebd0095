"""The native MCTS engine (libaz_mcts.so) on rectangular Connect4 boards, on the host.

* the rectangular rule probes (az_game_ended_rect / az_game_valids_rect /
  az_game_next_canonical_rect) against Connect4Game(cols, rows=rows) on random reachable
  positions of 7x6, 5x4, 4x6 and 9x7 (63 cells, the largest board of that aspect);
* whole engine episodes on 7x6 against the Python MCTS, with and without the GNN path
  (tests/test_native_mcts.py::test_engine_episodes_match_python_fuzz's check);
* 10x7 (70 cells): Engine raises ValueError, Coach._native_ok is false and Coach.selfPlay goes
  through the Python lock-step search (selfplay.play_episodes).
"""
import ctypes

import numpy as np
import pytest

from test_mcts_golden import Args
from test_native_mcts import HashNet, _random_positions


@pytest.fixture(scope="module", autouse=True)
def host_lib():
    from azhip.build import build_host
    build_host(verbose=False)
    import mcts_native
    return mcts_native.lib()


@pytest.mark.parametrize("shape", [(7, 6), (5, 4), (4, 6), (9, 7)])
def test_rect_rule_probes_match_the_python_game(host_lib, shape):
    from connect4.Connect4Game import Connect4Game
    cols, rows = shape
    game = Connect4Game(cols, rows=rows)
    A = game.getActionSize()
    P = ctypes.c_void_p
    rng = np.random.default_rng(100 * cols + rows)
    ended = 0
    for b in _random_positions(game, rng, 300):
        assert b.shape == (cols, rows)
        b8 = np.ascontiguousarray(b, np.int8)
        tag, val = ctypes.c_int(), ctypes.c_double()
        assert host_lib.az_game_ended_rect(0, cols, rows, b8.ctypes.data_as(P), ctypes.byref(tag),
                                           ctypes.byref(val)) == 0
        ref = game.getGameEnded(b, 1)
        ended += ref != 0
        assert (val.value, tag.value) == (float(ref), 0 if isinstance(ref, int) else 1)
        vv = np.zeros(A, np.int8)
        assert host_lib.az_game_valids_rect(0, cols, rows, b8.ctypes.data_as(P),
                                            vv.ctypes.data_as(P)) == 0
        valids = game.getValidMoves(b, 1)
        assert vv.tolist() == valids.tolist()
        for a in np.flatnonzero(valids):
            nb, pl = game.getNextState(b, 1, a)
            want = game.getCanonicalForm(nb, pl)
            out = np.full((cols, rows), 9, np.int8)
            assert host_lib.az_game_next_canonical_rect(0, cols, rows, b8.ctypes.data_as(P),
                                                        int(a), out.ctypes.data_as(P)) == 0
            assert out.tolist() == want.tolist()
    assert ended > 10                              # finished games are among the positions


def test_rect_probes_reject_what_the_engine_cannot_hold(host_lib):
    """More than 64 cells, a side below 4 on a rectangle and a rectangular TicTacToe are refused;
    the square forms are the rectangular ones with ny = nx."""
    P = ctypes.c_void_p
    b = np.zeros(80, np.int8)
    tag, val = ctypes.c_int(), ctypes.c_double()
    for game, nx, ny in ((0, 10, 7), (0, 3, 6), (0, 6, 3), (1, 3, 4)):
        assert host_lib.az_game_ended_rect(game, nx, ny, b.ctypes.data_as(P), ctypes.byref(tag),
                                           ctypes.byref(val)) < 0
        assert not host_lib.az_mcts_create_rect(game, nx, ny, 1, 1.0, 0)
    h = host_lib.az_mcts_create_rect(0, 7, 6, 2, 1.0, 0)
    assert h
    assert host_lib.az_mcts_action_size(P(h)) == 8
    host_lib.az_mcts_destroy(P(h))
    v1, v2 = np.zeros(4, np.int8), np.ones(4, np.int8)
    assert host_lib.az_game_valids(0, 3, b.ctypes.data_as(P), v1.ctypes.data_as(P)) == 0
    assert host_lib.az_game_valids_rect(0, 3, 3, b.ctypes.data_as(P), v2.ctypes.data_as(P)) == 0
    assert v1.tolist() == v2.tolist() == [1, 1, 1, 0]


@pytest.mark.parametrize("use_gnn", [False, True])
def test_engine_episodes_match_python_on_7x6(use_gnn):
    """Engine episodes == Python MCTS episodes on the standard board (same seeds, pseudo-random
    network), including example value types and pi list element types."""
    from connect4.Connect4Game import Connect4Game
    from selfplay import play_episodes, play_episodes_engine
    game = Connect4Game(7, rows=6)
    args = Args(numMCTSSims=12, cpuct=1.5, tempThreshold=6, use_gnn=use_gnn, expand_by=3)
    net = HashNet(game.getActionSize(), 61)
    eps = list(range(6))
    seeds = {e: 4242 + e for e in eps}
    py = play_episodes(game, net, args, eps, seeds, parallel_games=3)
    nat = play_episodes_engine(game, net, args, eps, seeds, parallel_games=4, threads=2)

    def typed(ex):
        return [tuple((type(x).__name__, np.asarray(x).tolist()) for x in row) for row in ex]
    for e in eps:
        assert len(py[e][0]) > 0 and np.asarray(py[e][0][0][0]).shape == (7, 6)
        assert typed(nat[e][0]) == typed(py[e][0]), e
        assert typed(nat[e][1]) == typed(py[e][1]), e


def test_engine_shapes_follow_the_board():
    from connect4.Connect4Game import Connect4Game
    from mcts_native import ArenaPlayer, Engine, game_kind, game_shape
    game = Connect4Game(7, rows=6)
    assert game_shape(game) == (0, (7, 6)) and game_kind(game) == (0, 7)
    assert game_shape(Connect4Game(7)) == (0, (7, 7))
    eng = Engine(game, 3, 1.0, True)
    assert eng.shape == (7, 6) and eng.cells == 42 and eng.A == 8
    assert eng.leaf_boards.shape == (3, 7, 6) and eng._b.shape == (7, 6)
    assert eng._sboards.shape[1:] == (7, 6)

    class Net:
        batch_invariant_rows = 8
    p = ArenaPlayer(game, Net(), Args(cpuct=1.0, use_gnn=False, numMCTSSims=2))
    assert p._batch.shape == (8, 7, 6)


def test_more_than_64_cells_falls_back_to_the_python_search(monkeypatch):
    """10x7: Engine raises ValueError, _native_ok is false, Coach.selfPlay runs play_episodes."""
    import Coach as C
    import selfplay
    from connect4.Connect4Game import Connect4Game
    from mcts_native import Engine
    game = Connect4Game(10, rows=7)
    with pytest.raises(ValueError, match="10x7"):
        Engine(game, 1, 1.0, False)
    assert not C._native_ok(game)
    assert C._native_ok(Connect4Game(9, rows=7)) and C._native_ok(Connect4Game(7, rows=6))

    class Net(HashNet):
        def __init__(self, game, args):
            super().__init__(game.getActionSize(), 3)

    args = Args(numEps=2, numMCTSSims=3, cpuct=1.0, tempThreshold=4, use_gnn=False, expand_by=1,
                parallel_games=2)
    used = []
    orig = selfplay.play_episodes

    def spy(*a, **k):
        used.append("python")
        return orig(*a, **k)

    def never(*a, **k):
        raise AssertionError("the native engine cannot hold a 10x7 board")

    monkeypatch.setattr(selfplay, "play_episodes", spy)
    monkeypatch.setattr(selfplay, "play_episodes_engine", never)
    np.random.seed(5)
    out = C.Coach(game, Net(game, args), args).selfPlay()
    assert used == ["python"] and len(out) == 2
    for std, _ in out:
        assert len(std) > 0 and np.asarray(std[0][0]).shape == (10, 7)
