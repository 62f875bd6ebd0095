"""Lock-step self-play with gnn_neighbors on the CPU: the native star builder against the Python
rules, the lock-step drivers under args.gnn_neighbors_lockstep against the sequential
Coach.executeEpisode (deterministic hash networks whose GNN output is a function of the leaf AND
its children), the key's way through Coach and main.py, and the new symbols in both bindings."""
import os
import re
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from test_selfplay import _norm_gnn, _norm_std


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


def _children(game, board):
    from MCTS import MCTS
    return MCTS(game, None, Args()).leaf_children(board)


def _random_positions(game, rng, count, max_moves):
    """Reachable NON-terminal canonical positions."""
    out = []
    while len(out) < count:
        b, p = game.getInitBoard(), 1
        for _ in range(rng.integers(0, max_moves)):
            a = rng.choice(np.flatnonzero(game.getValidMoves(b, p)))
            nb, np_ = game.getNextState(b, p, a)
            if game.getGameEnded(nb, np_) != 0:
                break
            b, p = nb, np_
        out.append(game.getCanonicalForm(b, p))
    return out


def _c4(moves, cols=7, rows=6):
    from connect4.Connect4Game import Connect4Game
    game = Connect4Game(cols, rows=rows)
    b, p = game.getInitBoard(), 1
    for a in moves:
        b, p = game.getNextState(b, p, a)
    board = game.getCanonicalForm(b, p)
    assert game.getGameEnded(board, 1) == 0
    return game, board


def _star_cases():
    from connect4.Connect4Game import Connect4Game
    from tictactoe.TicTacToeGame import TicTacToeGame
    return [("c4_7x7", Connect4Game(7), 40), ("c4_7x6", Connect4Game(7, rows=6), 36),
            ("c4_4x4", Connect4Game(4), 14), ("c4_8x8", Connect4Game(8), 50),
            ("ttt_3", TicTacToeGame(3), 8), ("ttt_5", TicTacToeGame(5), 22)]


# ------------------------------------------------------------------ 1. the star builder
@pytest.mark.parametrize("ci", range(6))
def test_star_builder_equals_python_leaf_children(ci):
    import mcts_native
    name, game, max_moves = _star_cases()[ci]
    kind, shape = mcts_native.game_shape(game)
    rng = np.random.default_rng(100 + ci)
    boards = _random_positions(game, rng, 300, max_moves)
    if name == "c4_7x6":
        # a full column, and a position where action 0 wins (its child is terminal)
        g, full = _c4((2, 2, 2, 2, 2, 2, 0, 4, 4))
        assert g.getValidMoves(full, 1)[2] == 0
        g, win = _c4((0, 6, 0, 6, 0, 5))
        assert g.getGameEnded(_children(g, win)[0], 1) != 0
        boards += [full, win]
    want = [[np.asarray(b)] + _children(game, b) for b in boards]
    if name == "c4_7x6":
        assert len(want[-2]) == 7 and len(want[-1]) == 8
        assert game.getGameEnded(want[-1][1], 1) != 0                       # kept, though terminal
    b8 = np.stack(boards).astype(np.int8)
    rows1, offs1 = mcts_native.game_stars(kind, shape, b8, threads=1)
    rows4, offs4 = mcts_native.game_stars(kind, shape, b8, threads=4)
    assert rows1.dtype == np.int8 and offs1.dtype == np.int32
    assert np.array_equal(rows1, rows4) and np.array_equal(offs1, offs4)
    assert np.array_equal(offs1, np.concatenate([[0], np.cumsum([len(s) for s in want])]))
    assert np.array_equal(rows1, np.stack([r for s in want for r in s]))
    if name == "ttt_3":
        assert max(np.diff(offs1)) == 10                                    # the empty board
    # a short cap fails and writes nothing
    V = int(offs1[-1])
    out = np.full((V,) + shape, 7, np.int8)
    offs = np.full(len(boards) + 1, -5, np.int32)
    P = lambda a: a.__array_interface__["data"][0]  # noqa: E731
    rc = mcts_native.lib().az_game_stars_rect(kind, shape[0], shape[1], P(b8), len(boards), 2,
                                              P(out), P(offs), V - 1)
    assert rc == -1 and b"cap_rows" in mcts_native.lib().az_mcts_last_error()
    assert np.all(out == 7) and np.all(offs == -5)
    with pytest.raises(RuntimeError, match="cap_rows"):
        mcts_native.game_stars(kind, shape, b8, cap_rows=V - 1)
    rc = mcts_native.lib().az_game_stars_rect(kind, shape[0], shape[1], P(b8), len(boards), 2,
                                              P(out), P(offs), V)
    assert rc == V and np.array_equal(out, rows1) and np.array_equal(offs, offs1)


def test_star_builder_empty_and_bad_cells():
    import mcts_native
    rows, offs = mcts_native.game_stars(0, (7, 6), np.zeros((0, 7, 6), np.int8))
    assert rows.shape == (0, 7, 6) and offs.tolist() == [0]
    bad = np.zeros((1, 7, 6), np.int8)
    bad[0, 0, 0] = 2
    with pytest.raises(RuntimeError, match="-1/0/1"):
        mcts_native.game_stars(0, (7, 6), bad)


# ------------------------------------------------------------------ 2. lock-step parity
class StarHashNet:
    """Deterministic network: the standard output is a pure function of the leaf, the GNN output
    a pure function of (leaf, children in order).  predict_with_gnn(board, neighbor_states) and
    predict_both_stars(rows, offs) compute the same float32 values; every star either entry point
    receives is kept in self.stars."""

    def __init__(self, game, args=None, salt=5):
        self.A, self.salt = game.getActionSize(), salt
        self.stars = []
        self.star_calls = self.single_calls = 0

    def _row(self, tag, data):
        h = np.random.default_rng([self.salt, tag, zlib.crc32(data), zlib.adler32(data)])
        p = h.random(self.A).astype(np.float32)
        if h.random() < 0.2:
            p[h.integers(0, self.A)] = 0.0
        p /= p.sum()
        return p.astype(np.float32), np.float32(h.uniform(-1, 1))

    @staticmethod
    def _cells(b):
        return np.asarray(b, np.int8).tobytes()

    def predict(self, board):
        return self._row(0, self._cells(board))

    def _gnn(self, board, kids):
        self.stars.append([np.asarray(board, np.int8)] + [np.asarray(k, np.int8) for k in kids])
        return self._row(1, b"|".join([self._cells(board)] + [self._cells(k) for k in kids]))

    def predict_with_gnn(self, board, neighbor_states=None):
        self.single_calls += 1
        return self._gnn(board, list(neighbor_states) if neighbor_states is not None else [])

    def predict_batch(self, boards):
        rows = [self.predict(b) for b in boards]
        return np.stack([p for p, _ in rows]), np.array([v for _, v in rows], np.float32)

    def predict_both_stars(self, rows, offs):
        self.star_calls += 1
        n = len(offs) - 1
        std = [self.predict(rows[offs[i]]) for i in range(n)]
        gnn = [self._gnn(rows[offs[i]], list(rows[offs[i] + 1:offs[i + 1]])) for i in range(n)]
        return (np.stack([p for p, _ in std]), np.array([v for _, v in std], np.float32),
                np.stack([p for p, _ in gnn]), np.array([v for _, v in gnn], np.float32))

    # a network of this mode never sees a star-less GNN request
    def predict_both(self, boards):
        raise AssertionError("gnn_neighbors_lockstep must not call predict_both")


class PerLeafHashNet(StarHashNet):
    """The same values without batch entry points for stars (the per-leaf fallback)."""
    def __getattribute__(self, name):
        if name == "predict_both_stars":
            raise AttributeError(name)
        return object.__getattribute__(self, name)


def _parity_games():
    from connect4.Connect4Game import Connect4Game
    from tictactoe.TicTacToeGame import TicTacToeGame
    return [Connect4Game(7, rows=6), TicTacToeGame(3)]


def _assert_stars(game, net):
    assert net.stars
    for star in net.stars:
        want = [star[0]] + _children(game, star[0])
        assert len(star) == len(want)
        assert all(np.array_equal(x, y) for x, y in zip(star, want))


@pytest.mark.parametrize("net_cls", [StarHashNet, PerLeafHashNet])
@pytest.mark.parametrize("gi", [0, 1])
def test_lockstep_drivers_equal_sequential_episodes(gi, net_cls):
    """Fails without the feature: Coach raises for gnn_neighbors with parallel games and no
    driver hands a leaf's children to the network."""
    import Coach as C
    from selfplay import play_episodes, play_episodes_engine, play_episodes_native
    game = _parity_games()[gi]
    args = Args(numEps=1, numMCTSSims=[9, 12][gi], cpuct=1.0, tempThreshold=4, use_gnn=True,
                expand_by=2, gnn_neighbors=True, gnn_neighbors_lockstep=True)
    eps = list(range(4 if gi == 0 else 8))
    seeds = {e: 700 + 31 * gi + e for e in eps}
    ref_net = net_cls(game)
    seq = {}
    for e in eps:
        coach = C.Coach(game, ref_net, Args(**{**vars(args), "parallel_games": 1}))
        np.random.seed(seeds[e])
        seq[e] = coach.executeEpisode()
    _assert_stars(game, ref_net)
    assert any(len(seq[e][1]) > 0 for e in eps)          # GNN examples exist
    runs = []
    for G in (1, 3, 8):
        runs.append(("python", G, None, lambda n, G=G: play_episodes(
            game, n, args, eps, seeds, parallel_games=G)))
        for lanes in (1, 2):
            runs.append(("engine", G, lanes, lambda n, G=G, lanes=lanes: play_episodes_engine(
                game, n, args, eps, seeds, parallel_games=G, threads=2, lanes=lanes)))
    runs.append(("native", 3, 2, lambda n: play_episodes_native(
        game, n, args, eps, seeds, parallel_games=3, threads=2, lanes=2)))
    for name, G, lanes, run in runs:
        net = net_cls(game)
        got = run(net)
        for e in eps:
            assert _norm_std(got[e][0]) == _norm_std(seq[e][0]), (name, G, lanes, e)
            assert _norm_gnn(got[e][1]) == _norm_gnn(seq[e][1]), (name, G, lanes, e)
        _assert_stars(game, net)
        if net_cls is StarHashNet:
            assert net.star_calls > 0 and net.single_calls == 0, (name, G, lanes)
        else:
            assert net.single_calls > 0


def test_without_the_key_the_drivers_pass_no_children():
    """gnn_neighbors alone leaves the lock-step drivers as they were (predict_both on boards)."""
    from selfplay import lockstep_stars, play_episodes
    from test_native_mcts import HashNet
    game = _parity_games()[1]
    args = Args(numMCTSSims=5, cpuct=1.0, tempThreshold=4, use_gnn=True, expand_by=1,
                gnn_neighbors=True)
    assert not lockstep_stars(args)
    assert not lockstep_stars(Args(gnn_neighbors_lockstep=True, use_gnn=True))
    assert lockstep_stars({"gnn_neighbors_lockstep": True, "use_gnn": True, "gnn_neighbors": True})
    out = play_episodes(game, HashNet(game.getActionSize(), 3), args, [0], {0: 1},
                        parallel_games=1)
    assert len(out[0][0]) > 0


@pytest.mark.nn_failures_expected
def test_a_failed_star_batch_degrades_every_leaf():
    import nn_fallback
    from selfplay import play_episodes_engine
    game = _parity_games()[1]
    args = Args(numMCTSSims=4, cpuct=1.0, tempThreshold=4, use_gnn=False, expand_by=1,
                gnn_neighbors=True, gnn_neighbors_lockstep=True)

    class Failing(StarHashNet):
        def predict_both_stars(self, rows, offs):
            raise RuntimeError("device lost")

    # use_gnn off: the key is inert (no star is built, predict_batch serves the leaves)
    out = play_episodes_engine(game, Failing(game), args, [0], {0: 2}, parallel_games=1,
                               threads=1, lanes=1)
    assert len(out[0][0]) > 0 and nn_fallback.total() == 0
    # use_gnn on: an expand_tree root predict rides in a failed batch -> the error propagates
    # (MCTS.py:108-113), after the batch's leaves were degraded and counted
    args.use_gnn = True
    with pytest.raises(RuntimeError, match="device lost"):
        play_episodes_engine(game, Failing(game), args, [0], {0: 2}, parallel_games=1,
                             threads=1, lanes=1)
    assert nn_fallback.total() > 0


# ------------------------------------------------------------------ 3. Coach / main
def test_coach_accepts_the_key_and_plays_lock_step(monkeypatch):
    import Coach as C
    import selfplay
    game = _parity_games()[0]
    base = dict(numEps=3, numMCTSSims=3, cpuct=1.0, tempThreshold=3, use_gnn=True, expand_by=1)
    for bad in (dict(gnn_neighbors_lockstep=True),
                dict(gnn_neighbors_lockstep=True, gnn_neighbors=True, use_gnn=False),
                dict(gnn_neighbors_lockstep=True, gnn_neighbors=False)):
        with pytest.raises(ValueError, match="use_gnn.*gnn_neighbors|gnn_neighbors.*use_gnn"):
            C.Coach(game, StarHashNet(game), Args(**{**base, **bad}))
    on = dict(gnn_neighbors=True, gnn_neighbors_lockstep=True, parallel_games=4)
    coach = C.Coach(game, StarHashNet(game), Args(**base, **on))
    assert coach.selfplay_uses_native_engine() and not coach.uses_native_engine()
    monkeypatch.setattr(C.D, "world_rank", lambda: (2, 0))
    assert C.Coach(game, StarHashNet(game), Args(**base, **on))        # several ranks too
    monkeypatch.undo()
    seen = []
    for name in ("play_episodes_engine", "play_episodes"):
        orig = getattr(selfplay, name)
        monkeypatch.setattr(selfplay, name,
                            lambda *a, _o=orig, _n=name, **k: (seen.append(_n), _o(*a, **k))[1])
    out = coach.selfPlay()
    assert seen == ["play_episodes_engine"] and len(out) == 3
    assert coach.nnet.star_calls > 0 and coach.nnet.single_calls == 0
    _assert_stars(game, coach.nnet)
    seen.clear()
    py = C.Coach(game, StarHashNet(game), Args(selfplay_engine="python", **base, **on))
    assert not py.selfplay_uses_native_engine()
    assert len(py.selfPlay()) == 3 and seen == ["play_episodes"] and py.nnet.star_calls > 0
    # without the key, selfplay's predicate is the old one
    assert C.Coach(game, StarHashNet(game), Args(**base)).selfplay_uses_native_engine()
    assert not C.Coach(game, StarHashNet(game),
                       Args(gnn_neighbors=True, **base)).selfplay_uses_native_engine()


def test_main_carries_the_key(tmp_path):
    import main
    import yaml
    cfg = tmp_path / "config.yaml"
    doc = {"game": {"board_size": 7}, "training": {"checkpoint_path": str(tmp_path / "ck")},
           "neural_network": {"use_gnn": True}}
    cfg.write_text(yaml.safe_dump(doc))
    base = ["--game", "connect4", "--use_gnn", "--config", str(cfg)]
    assert main.parse(base).gnn_neighbors_lockstep is None
    assert not main.build_args(main.parse(base)).get("gnn_neighbors_lockstep", False)
    a = main.build_args(main.parse(base + ["--gnn_neighbors", "--gnn_neighbors_lockstep"]))
    assert a.gnn_neighbors is True and a.gnn_neighbors_lockstep is True
    doc["selfplay"] = {"gnn_neighbors": True, "gnn_neighbors_lockstep": True}
    cfg.write_text(yaml.safe_dump(doc))
    assert main.build_args(main.parse(base)).gnn_neighbors_lockstep is True
    for name in ("connect4", "tictactoe"):      # the shipped configs name the key, off
        shipped = main.config_to_args(main.load_config(os.path.join(main.HERE, name,
                                                                    "config.yaml")))
        assert shipped.gnn_neighbors_lockstep is False


# ------------------------------------------------------------------ 4. ABI
def test_new_symbols_in_both_bindings():
    import mcts_native
    from azhip import _lib
    from azhip.build import build
    build(verbose=False)
    for name in ("az_gnn_star_batch_ws_bytes", "az_gnn_star_batch_infer"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert "az_game_stars_rect" in mcts_native._SIGS
    assert hasattr(mcts_native.lib(), "az_game_stars_rect")
    hdr = open(os.path.join(ROOT, "include", "az_mcts.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(az_[a-z0-9_]+)\s*\(", hdr))
    assert "az_game_stars_rect" in declared and declared == set(mcts_native._SIGS)


def test_star_batch_host_checks_without_gpu():
    """Shape, null-pointer, alignment and workspace checks run on the host before any HIP call."""
    import ctypes
    from azhip import _lib
    from azhip.build import build
    build(verbose=False)
    L = _lib.load()
    ws_bytes = L.az_gnn_star_batch_ws_bytes
    assert ws_bytes(4, 20, 1024, 128, 2) > 0
    for bad in ((0, 20, 1024, 128, 2), (4, 3, 1024, 128, 2), (4, 20, 1000, 128, 2),
                (4, 20, 1024, 126, 2), (4, 20, 1024, 128, 5), (4, 20, 1024, 128, -1)):
        assert ws_bytes(*bad) == 0, bad
    assert ws_bytes(8, 80, 3136, 128, 2) >= ws_bytes(4, 20, 3136, 128, 2)
    fn = L.az_gnn_star_batch_infer
    lw = (_lib.LayerW * 4)()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    assert fn(None, None, 0, 0, 1024, 128, 2, lw, None, None, 0, None) == 0       # B == 0
    cases = [((p, p + 1024, 4, 20, 1000, 128, 2, lw, p + 2048, p, 1 << 40), b"bad shape"),
             ((p, p + 1024, 4, 20, 1024, 128, 5, lw, p + 2048, p, 1 << 40), b"bad shape"),
             ((p, p + 1024, 4, 3, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"bad shape"),
             ((None, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"null"),
             ((p, None, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"null"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, None, p, 1 << 40), b"null"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, None, 1 << 40), b"null"),
             ((p + 4, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"alignment"),
             ((p, p + 1026, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"alignment"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2052, p, 1 << 40), b"alignment"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p, p + 2048, 1 << 40), b"alias"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1024), b"too small"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"null weight")]
    failed = []

    def run():
        try:
            for a, msg in cases:
                assert fn(*a, None) == -1, msg
                assert msg in L.az_last_error(), (msg, L.az_last_error())
        except BaseException as ex:   # reported on the test's own thread
            failed.append(ex)

    # az_last_error is per thread: the rejected calls run on a thread of their own, so the main
    # thread keeps the empty message tests/test_lib_abi.py expects whatever the test order
    import threading
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failed:
        raise failed[0]
