"""FrozenLake on the host (no GPU): the rules against every answer the reference gave
(tests/golden/make_frozenlake_goldens.py), the registry, and the Python MCTS / Coach episode
replaying the reference's single-player searches bit for bit over recorded predictions."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden

MAP5 = ["SHFFF", "FFFHF", "FFFFF", "HFFFH", "FFFFG"]


def _game(tag):
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    return {"m4": lambda: FrozenLakeGame(map_size=4), "m8": lambda: FrozenLakeGame(map_size=8),
            "c5": lambda: FrozenLakeGame(map_size=4, custom_map=MAP5)}[tag]()


def _states(n):
    out = []
    for cell in range(n * n):
        b = np.zeros((n, n))
        b[cell // n, cell % n] = 1
        out.append(b)
    return out + [np.zeros((n, n))]


@pytest.mark.parametrize("tag", ["m4", "m8", "c5"])
def test_rules_match_reference(tag):
    z = golden("fl_rules.npz")
    g = _game(tag)
    n = len(z[f"{tag}_map"])
    assert g.map_size == n and g.getBoardSize() == (n, n) and g.getActionSize() == 4
    assert ["".join(c.decode() for c in row) for row in g.desc] == list(z[f"{tag}_map"])
    assert tuple(g.goal_pos) == tuple(z[f"{tag}_goal"])
    init = g.getInitBoard()
    assert init.dtype == np.float64 and np.array_equal(init, z[f"{tag}_init"])
    for i, b in enumerate(_states(n)):
        valid = g.getValidMoves(b, 1)
        assert valid.dtype == np.int8 and np.array_equal(valid, z[f"{tag}_valid"][i]), (tag, i)
        assert float(g.getGameEnded(b, 1)) == z[f"{tag}_ended"][i], (tag, i)
        assert g.stringRepresentation(b) == str(z[f"{tag}_str"][i])
        for a in range(4):
            nxt, player = g.getNextState(b, 1, a)
            assert player == 1 and np.array_equal(nxt, z[f"{tag}_next"][i, a]), (tag, i, a)
        assert g.getCanonicalForm(b, 1) is b
        sym = g.getSymmetries(b, [0.25] * 4)
        assert len(sym) == 1 and sym[0][0] is b


def test_interface_details():
    g = _game("m4")
    assert g.is_two_player is False
    assert g.desc.shape == (4, 4) and g.desc[1][1] == b"H" and g.desc[3][3] == b"G"
    assert g.goal_pos == (3, 3)
    assert _game("m8").desc[7][7] == b"G" and _game("m8").map_size == 8
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    assert FrozenLakeGame(map_size=5).map_size == 4          # anything but 8: the 4x4 map
    assert FrozenLakeGame(map_size=8, custom_map=["SF", "FG"]).map_size == 2   # custom map wins
    assert FrozenLakeGame(render_mode="human", is_slippery=True).render_mode == "human"


@pytest.mark.parametrize("bad", [["SFF", "FFF"], ["S"], ["SFFFFFFFF"] * 9, ["SF", "FFG"]])
def test_map_size_rejected(bad):
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    with pytest.raises(ValueError, match="square with 2 to 8"):
        FrozenLakeGame(custom_map=bad)


def test_render_prints_the_map(capsys):
    g = _game("m4")
    g.getNextState(g.getInitBoard(), 1, 1)
    g.render()
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 4 and lines[0].startswith(" S [F]")


def test_no_gymnasium_needed():
    import register  # noqa: F401
    import frozenlake.FrozenLakeGame  # noqa: F401
    assert "gymnasium" not in sys.modules


def test_registry():
    import register
    assert set(register.list_games()) >= {"tictactoe", "connect4", "frozenlake"}
    assert register.has_gnn_version("frozenlake") is False
    game_cls, net_cls = register.get_game("frozenlake")
    assert game_cls.__name__ == "FrozenLakeGame" and net_cls.__name__ == "FrozenLakeNet"
    with pytest.raises(ValueError, match="GNN version of 'frozenlake' is not implemented"):
        register.get_game("frozenlake", True)


def test_main_builds_the_game_from_the_config(tmp_path):
    import main as M
    args = M.config_to_args(M.load_config(os.path.join(M.HERE, "frozenlake", "config.yaml")))
    args.game = "frozenlake"
    game_cls, _ = M.get_game("frozenlake")
    g = M.create_game_instance(game_cls, args)
    assert g.map_size == 4 and g.is_slippery is False and g.render_mode is None
    assert args.embedding_dim == 128 and args.gnn_layers == 3 and args.cpuct == 2.0
    args.board_size, args.custom_map = 8, ["SFH", "FFF", "HFG"]
    assert M.create_game_instance(game_cls, args).map_size == 3
    assert M.pit_gnn_vs_regular("frozenlake", args) is None        # "no GNN version"


def test_native_engine_not_used():
    import Coach
    assert Coach._native_ok(_game("m4")) is False


class RecordedNet:
    """The recorded (pi, v) of a state; v has shape (1,) as FrozenLakeNet.predict returns it."""

    def __init__(self, z, S):
        self.pi, self.v, self.S, self.calls = z["pi"], z["v"], S, 0

    def predict(self, board):
        self.calls += 1
        i = self.S if np.sum(board) == 0 else int(np.argmax(board))
        return self.pi[i].copy(), self.v[i:i + 1].copy()


class Args(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def test_mcts_replays_reference_searches():
    from MCTS import MCTS
    meta = json.load(open(os.path.join(GOLDEN, "fl_mcts.json")))
    g = _game("m4")
    net = RecordedNet(golden("fl_mcts.npz"), 16)
    args = Args(meta["args"])
    states = _states(4)
    for run in meta["runs"]:
        board = states[run["start"]]
        s = g.stringRepresentation(board)
        m = MCTS(g, net, args)
        probs = m.getActionProb(board, temp=1)
        assert [int(m.Nsa.get((s, a), 0)) for a in range(4)] == run["counts"]
        assert [float(x) for x in probs] == run["probs"]
        q = [float(np.asarray(m.Qsa[(s, a)]).reshape(-1)[0]) if (s, a) in m.Qsa else None
             for a in range(4)]
        assert q == run["q"]
        assert len(m.Ns) == run["n_nodes"] and int(sum(m.Nsa.values())) == run["nsa_total"]
        np.random.seed(run["seed0"])
        assert [int(x) for x in MCTS(g, net, args).getActionProb(board, temp=0)] == run["probs0"]


def test_search_stops_where_a_descent_returns_to_a_state():
    """Priors that send (0,0) right and (0,1) left: the reference recurses without end; here the
    descent stops at the repeated state with value 0 and every simulation returns."""
    from MCTS import MCTS
    g = _game("m4")
    pi = np.full((17, 4), 0.01, np.float32)
    pi[:, 3] = 0.97
    pi[0] = [0.01, 0.97, 0.01, 0.01]
    net = RecordedNet({"pi": pi, "v": np.zeros(17, np.float32)}, 16)
    m = MCTS(g, net, Args(numMCTSSims=30, cpuct=2.0))
    probs = m.getActionProb(g.getInitBoard(), temp=1)
    assert abs(sum(probs) - 1) < 1e-6 and sum(m.Nsa.values()) >= 29


def test_episode_replays_reference():
    import Coach as C
    from MCTS import MCTS
    meta = json.load(open(os.path.join(GOLDEN, "fl_episode.json")))
    g = _game("m4")
    net = RecordedNet(golden("fl_mcts.npz"), 16)
    args = Args(meta["args"])
    orig = np.random.choice
    kinds = []
    for ep in meta["episodes"]:
        moves, cap = [0], 4 * len(ep["boards"])

        def choice(*a, moves=moves, cap=cap, **k):
            moves[0] += 1
            assert moves[0] <= cap, "the episode outran 4x the reference's length"
            return orig(*a, **k)

        coach = C.Coach.__new__(C.Coach)
        coach.game, coach.args, coach.nnet = g, args, net
        coach.mcts = MCTS(g, net, args)
        np.random.seed(ep["seed"])
        np.random.choice = choice
        try:
            std, gnn = coach.executeEpisode()
        finally:
            np.random.choice = orig
        assert gnn == []
        assert [np.asarray(b).astype(int).tolist() for b, _, _ in std] == ep["boards"]
        assert [[float(x) for x in p] for _, p, _ in std] == ep["pis"]
        assert [float(r) for _, _, r in std] == ep["rewards"]
        kinds.append(ep["kind"])
    assert kinds == ["goal", "hole"]
