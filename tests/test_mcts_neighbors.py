"""args.gnn_neighbors on the CPU, with fake networks that record their calls: what
MCTS.evaluate_request hands to predict_with_gnn with the flag off and on, how a failing network
degrades, that Coach keeps such a run on the Python search, and the flag's way through main.py."""
from types import SimpleNamespace

import numpy as np
import pytest


class Args(SimpleNamespace):
    def __getitem__(self, k):
        return getattr(self, k)


class RecordingNet:
    """Uniform priors, value 0; keeps (args, kwargs) of every predict_with_gnn call."""

    def __init__(self, game, args=None):
        self.A = game.getActionSize()
        self.calls = []

    def _out(self):
        return np.full(self.A, 1.0 / self.A, np.float32), np.float32(0.0)

    def predict(self, board):
        return self._out()

    def predict_with_gnn(self, *a, **k):
        self.calls.append((a, k))
        return self._out()


def _children(game, board):
    valids = game.getValidMoves(board, 1)
    return [game.getCanonicalForm(*game.getNextState(board, 1, a))
            for a in range(game.getActionSize()) if valids[a]]


def _c4_full_column():
    """7x6 position with column 2 full (six alternating discs) and a few more moves."""
    from connect4.Connect4Game import Connect4Game
    game = Connect4Game(7, rows=6)
    b, p = game.getInitBoard(), 1
    for a in (2, 2, 2, 2, 2, 2, 0, 4, 4):
        b, p = game.getNextState(b, p, a)
    board = game.getCanonicalForm(b, p)
    assert game.getGameEnded(board, 1) == 0 and game.getValidMoves(board, 1)[2] == 0
    return game, board


def test_flag_off_calls_predict_with_gnn_with_one_positional_argument():
    from MCTS import MCTS
    game, board = _c4_full_column()
    for args in (Args(numMCTSSims=4, cpuct=1.0, use_gnn=True),
                 Args(numMCTSSims=4, cpuct=1.0, use_gnn=True, gnn_neighbors=False),
                 {"numMCTSSims": 4, "cpuct": 1.0, "use_gnn": True}):
        net = RecordingNet(game)
        std, gnn, err = MCTS(game, net, args).evaluate_request((board, True))
        assert err is None and std is not None and gnn is not None
        assert len(net.calls) == 1
        a, k = net.calls[0]
        assert len(a) == 1 and k == {} and np.array_equal(a[0], board)
    net = RecordingNet(game)
    MCTS(game, net, Args(numMCTSSims=4, cpuct=1.0, use_gnn=True, gnn_neighbors=True)) \
        .evaluate_request((board, False))
    assert net.calls == []                      # no GNN evaluation asked for: none made


def test_flag_on_hands_over_the_children_in_action_order():
    """Connect4 7x6 with a full column (6 children, the full column's action skipped) and the
    opening (7 children); TicTacToe 3x3 (one child per empty cell, row-major)."""
    from MCTS import MCTS
    from tictactoe.TicTacToeGame import TicTacToeGame
    game, board = _c4_full_column()
    cases = [(game, board, 6), (game, game.getCanonicalForm(game.getInitBoard(), 1), 7)]
    ttt = TicTacToeGame(3)
    tb = np.array([[1, -1, 0], [0, 1, -1], [0, -1, 0]])
    cases.append((ttt, tb, 4))
    for g, b, n in cases:
        for args in (Args(numMCTSSims=4, cpuct=1.0, use_gnn=True, gnn_neighbors=True),
                     {"numMCTSSims": 4, "cpuct": 1.0, "use_gnn": True, "gnn_neighbors": True}):
            net = RecordingNet(g)
            mcts = MCTS(g, net, args)
            _, gnn, err = mcts.evaluate_request((b, True))
            assert err is None and gnn is not None
            (a, k), = net.calls
            assert len(a) == 1 and np.array_equal(a[0], b) and list(k) == ["neighbor_states"]
            kids = k["neighbor_states"]
            want = _children(g, b)
            assert len(kids) == len(want) == n
            for x, y in zip(kids, want):
                assert np.array_equal(x, y)
            # action order: child i differs from the (negated) leaf in exactly one cell, and the
            # actions that put it there ascend
            valid = np.flatnonzero(g.getValidMoves(b, 1))
            for i, a_ in enumerate(valid):
                nxt, player = g.getNextState(b, 1, a_)
                assert np.array_equal(kids[i], g.getCanonicalForm(nxt, player))
                assert int(np.sum(kids[i] != -np.asarray(b))) == 1


def test_a_terminal_child_is_included():
    from MCTS import MCTS
    from connect4.Connect4Game import Connect4Game
    game = Connect4Game(7, rows=6)
    b, p = game.getInitBoard(), 1
    for a in (0, 6, 0, 6, 0, 5):                # player 1 to move with three discs in column 0
        b, p = game.getNextState(b, p, a)
    board = game.getCanonicalForm(b, p)
    net = RecordingNet(game)
    MCTS(game, net, Args(numMCTSSims=2, cpuct=1.0, use_gnn=True, gnn_neighbors=True)) \
        .evaluate_request((board, True))
    kids = net.calls[0][1]["neighbor_states"]
    assert len(kids) == 7
    ended = [game.getGameEnded(k, 1) for k in kids]
    assert ended[0] != 0 and not any(ended[1:])  # action 0 wins: its child is terminal, and there


def test_whole_search_passes_children_at_every_leaf():
    from MCTS import MCTS
    game, board = _c4_full_column()
    net = RecordingNet(game)
    mcts = MCTS(game, net, Args(numMCTSSims=12, cpuct=1.0, use_gnn=True, gnn_neighbors=True))
    mcts.getActionProb(board, temp=1)
    assert len(net.calls) >= 7
    for a, k in net.calls:
        want = _children(game, a[0])
        assert len(k["neighbor_states"]) == len(want)
        assert all(np.array_equal(x, y) for x, y in zip(k["neighbor_states"], want))


@pytest.mark.nn_failures_expected
def test_a_failing_star_evaluation_degrades_through_nn_fallback():
    import nn_fallback
    from MCTS import MCTS
    game, board = _c4_full_column()

    class Failing(RecordingNet):
        def predict_with_gnn(self, *a, **k):
            raise RuntimeError("device lost")

    mcts = MCTS(game, Failing(game), Args(numMCTSSims=3, cpuct=1.0, use_gnn=True,
                                          gnn_neighbors=True))
    std, gnn, err = mcts.evaluate_request((board, True))
    assert std is not None and gnn is None and isinstance(err, RuntimeError)
    nn_fallback.reset()
    v = mcts.search(board)
    s = game.stringRepresentation(board)
    valids = game.getValidMoves(board, 1)
    assert v == 0 and np.allclose(mcts.Ps[s], valids / valids.sum())
    assert nn_fallback.total() == 1


def test_coach_keeps_gnn_neighbors_on_the_python_search(monkeypatch):
    import Coach as C
    import selfplay
    from connect4.Connect4Game import Connect4Game
    game = Connect4Game(7, rows=6)
    assert C._native_ok(game)                   # unchanged: the engine covers the board
    base = dict(numEps=1, numMCTSSims=2, cpuct=1.0, tempThreshold=3, use_gnn=True, expand_by=1)
    on = C.Coach(game, RecordingNet(game), Args(gnn_neighbors=True, **base))
    off = C.Coach(game, RecordingNet(game), Args(**base))
    assert off.uses_native_engine() and not on.uses_native_engine()
    assert C.Coach(game, RecordingNet(game), Args(gnn_neighbors=True, parallel_games=1, **base))

    def never(*a, **k):
        raise AssertionError("gnn_neighbors runs on the Python search")

    monkeypatch.setattr(selfplay, "play_episodes_engine", never)
    monkeypatch.setattr(selfplay, "play_episodes", never)
    np.random.seed(3)
    (std, gnn), = on.selfPlay()
    assert len(std) > 0 and len(on.nnet.calls) > 0
    assert all(list(k) == ["neighbor_states"] for _, k in on.nnet.calls)
    for bad in (dict(parallel_games=4), dict(parallel_games=2)):
        with pytest.raises(ValueError, match="gnn_neighbors.*parallel_games"):
            C.Coach(game, RecordingNet(game), Args(gnn_neighbors=True, **bad, **base))
    monkeypatch.setattr(C.D, "world_rank", lambda: (2, 0))
    with pytest.raises(ValueError, match="gnn_neighbors.*2 > 1 ranks"):
        C.Coach(game, RecordingNet(game), Args(gnn_neighbors=True, **base))
    assert C.Coach(game, RecordingNet(game), Args(**base))      # without the flag: as before


def test_main_carries_the_flag(tmp_path):
    import main
    import yaml
    cfg = tmp_path / "config.yaml"
    doc = {"game": {"board_size": 7}, "training": {"checkpoint_path": str(tmp_path / "ck")},
           "neural_network": {"use_gnn": True}}
    cfg.write_text(yaml.safe_dump(doc))
    base = ["--game", "connect4", "--use_gnn", "--config", str(cfg)]
    assert main.parse(base).gnn_neighbors is None
    assert not main.build_args(main.parse(base)).get("gnn_neighbors", False)
    assert main.build_args(main.parse(base + ["--gnn_neighbors"])).gnn_neighbors is True
    doc["selfplay"] = {"gnn_neighbors": True}
    cfg.write_text(yaml.safe_dump(doc))
    assert main.build_args(main.parse(base)).gnn_neighbors is True
    for name in ("connect4", "tictactoe"):      # the shipped configs name the key, off
        shipped = main.config_to_args(main.load_config(
            __import__("os").path.join(main.HERE, name, "config.yaml")))
        assert shipped.gnn_neighbors is False
