"""The single-player Arena against the reference's results for scripted players
(tests/golden/fl_arena.json): (result, steps) of one episode, playGame, and the
(player1 better, player2 better, equal) triples of playGamesForSinglePlayer."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


class ScriptPlayer:
    """Plays a fixed action sequence, cyclically; startGame rewinds it."""

    def __init__(self, actions):
        self.actions, self.i = actions, 0

    def startGame(self):
        self.i = 0

    def __call__(self, board):
        a = self.actions[self.i % len(self.actions)]
        self.i += 1
        return a


@pytest.fixture(scope="module")
def meta():
    return json.load(open(os.path.join(GOLDEN, "fl_arena.json")))


@pytest.mark.parametrize("size", [4, 8])
def test_single_episodes(meta, size):
    from Arena import Arena
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    game = FrozenLakeGame(map_size=size)
    m = meta[str(size)]
    assert set(m["scripts"]) == {"path", "hole", "bounce", "invalid"}
    for name, want in m["singles"].items():
        arena = Arena(ScriptPlayer(m["scripts"][name]), ScriptPlayer(m["scripts"][name]), game)
        assert arena.is_single_player
        np.random.seed(want["seed"])
        result, steps = arena.playGameForSinglePlayer(arena.player1)
        assert (float(result), int(steps)) == (want["result"], want["steps"]), name
        np.random.seed(want["seed"])
        assert float(arena.playGame()) == want["play_game"], name
    assert m["singles"]["bounce"]["steps"] == 5 * size * size       # the cap, a draw
    assert m["singles"]["bounce"]["result"] == 0.0


@pytest.mark.parametrize("size", [4, 8])
def test_play_games_triples(meta, size):
    from Arena import Arena
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    game = FrozenLakeGame(map_size=size)
    m = meta[str(size)]
    assert len(m["pairs"]) == 16
    for pair, want in m["pairs"].items():
        a, b = pair.split(":")
        arena = Arena(ScriptPlayer(m["scripts"][a]), ScriptPlayer(m["scripts"][b]), game)
        np.random.seed(want["seed"])
        assert list(arena.playGames(want["num"])) == want["triple"], pair


def test_episode_starts_from_a_given_board_and_survives_a_failing_player():
    from Arena import Arena
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    game = FrozenLakeGame(map_size=4)
    board = np.zeros((4, 4))
    board[3, 2] = 1
    arena = Arena(ScriptPlayer([1]), None, game)
    assert arena.playGameForSinglePlayer(arena.player1, board) == (1.0, 1)
    assert board[3, 2] == 1 and board.sum() == 1               # the caller's board is untouched

    def broken(_):
        raise RuntimeError("no move")

    assert Arena(broken, None, game).playGameForSinglePlayer(broken) == (0, 1)
