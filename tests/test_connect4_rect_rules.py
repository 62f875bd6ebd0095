"""Connect4Game(board_size, rows): the rectangular rules on the host.

* Connect4Game(n, rows=n) is Connect4Game(n) in every output (one rule set, not one per shape);
* (7,6), (5,4) and (4,6) against a slow loop restatement of the rules, at every ply of seeded
  random playouts that are checked to contain full-board draws;
* win detection against the golden-pinned square game (tests/test_rules_golden.py): the stones of
  a rectangular board embedded in a square one give the same +-1 / no-win answer;
* the shapes that are refused.
"""
import numpy as np
import pytest

from connect4.Connect4Game import Connect4Game

SHAPES = ((7, 6), (5, 4), (4, 6))


def _playout(game, rng, visit, fill=False):
    """One random game from the empty board; visit(board, player) at every ply, the terminal one
    included.  fill=True prefers moves that do not end the game while one exists, which is how a
    random playout reaches the full board.  Returns the final getGameEnded(board, player)."""
    b, p = game.getInitBoard(), 1
    for _ in range(200):
        visit(b, p)
        r = game.getGameEnded(b, p)
        if r != 0:
            return r
        moves = np.flatnonzero(game.getValidMoves(b, p))
        if fill:
            quiet = [a for a in moves
                     if game.getGameEnded(*game.getNextState(b, p, a)) in (0, 1e-4)]
            moves = quiet or moves
        b, p = game.getNextState(b, p, rng.choice(moves))
    raise AssertionError("playout did not end")


@pytest.mark.parametrize("n", [5, 7])
def test_rows_equal_to_columns_is_the_square_game(n):
    """100 seeded playouts: every method of Connect4Game(n, rows=n) against Connect4Game(n)."""
    sq, rc = Connect4Game(n), Connect4Game(n, rows=n)
    assert rc.rows == n and rc.board_size == n and sq.rows == n
    assert rc.getBoardSize() == sq.getBoardSize() and rc.getActionSize() == sq.getActionSize()
    assert np.array_equal(rc.getInitBoard(), sq.getInitBoard())
    rng = np.random.default_rng(100 + n)
    plies = [0]

    def visit(b, p):
        plies[0] += 1
        va, vb = sq.getValidMoves(b, p), rc.getValidMoves(b, p)
        assert va.dtype == vb.dtype and va.tolist() == vb.tolist()
        for q in (p, -p):
            ea, eb = sq.getGameEnded(b, q), rc.getGameEnded(b, q)
            assert ea == eb and type(ea) is type(eb)
        assert np.array_equal(sq.getCanonicalForm(b, p), rc.getCanonicalForm(b, p))
        assert sq.stringRepresentation(b) == rc.stringRepresentation(b)
        pi = list(rng.random(n + 1))
        for (ba, pa), (bb, pb) in zip(sq.getSymmetries(b, pi), rc.getSymmetries(b, pi)):
            assert np.array_equal(ba, bb) and np.array_equal(pa, pb)
        for a in np.flatnonzero(va):
            (na, pa), (nb, pb) = sq.getNextState(b, p, a), rc.getNextState(b, p, a)
            assert pa == pb and np.array_equal(na, nb) and na.dtype == nb.dtype

    for i in range(100):
        _playout(sq, rng, visit, fill=i % 4 == 0)
    assert plies[0] > 1000


# ------------------------------------------------------------------ the rules, restated slowly
def _slow_valids(b, cols, rows):
    v = [0] * (cols + 1)
    for x in range(cols):
        if b[x][rows - 1] == 0:
            v[x] = 1
    if sum(v) == 0:
        v[cols] = 1                               # the pass, only when no column is open
    return v


def _slow_next(b, cols, rows, player, a):
    if a == cols:
        return b, -player
    nb = b.copy()
    for y in range(rows):                         # the lowest empty row
        if nb[a][y] == 0:
            nb[a][y] = player
            return nb, -player
    raise AssertionError("full column")


def _slow_run(b, cols, rows, who, w):
    for x in range(cols):
        for y in range(rows):
            for dx, dy in ((0, 1), (1, 0), (1, 1), (1, -1)):
                cells = [(x + dx * k, y + dy * k) for k in range(w)]
                if all(0 <= cx < cols and 0 <= cy < rows and b[cx][cy] == who
                       for cx, cy in cells):
                    return True
    return False


def _slow_ended(b, cols, rows, player, w=4):
    if _slow_run(b, cols, rows, player, w):
        return 1
    if _slow_run(b, cols, rows, -player, w):
        return -1
    if any(b[x][rows - 1] == 0 for x in range(cols)):
        return 0
    return 1e-4


@pytest.mark.parametrize("shape", SHAPES)
def test_rectangular_rules_against_the_slow_restatement(shape):
    """200 seeded playouts per shape, every ply: shape and action size, valid moves, the next state
    of every valid move, getGameEnded for both players (value and Python type), the canonical form,
    both symmetries and the string; at least one playout ends on the full board (1e-4, only the
    pass valid)."""
    cols, rows = shape
    game = Connect4Game(cols, rows=rows)
    assert game.board_size == cols and game.rows == rows
    assert game.getBoardSize() == (cols, rows) and game.getActionSize() == cols + 1
    init = game.getInitBoard()
    assert init.shape == (cols, rows) and init.dtype == np.int64 and not init.any()
    rng = np.random.default_rng(1000 * cols + rows)
    draws = [0]

    def visit(b, p):
        assert b.shape == (cols, rows)
        want_v = _slow_valids(b, cols, rows)
        got_v = game.getValidMoves(b, p)
        assert got_v.tolist() == want_v and got_v.dtype == np.int64
        for q in (p, -p):
            want, got = _slow_ended(b, cols, rows, q), game.getGameEnded(b, q)
            assert got == want and type(got) is type(want), (shape, q, got, want)
        if game.getGameEnded(b, p) == 1e-4:
            draws[0] += 1
            assert want_v == [0] * cols + [1]
            nb, np_ = game.getNextState(b, p, cols)
            assert nb is b and np_ == -p          # the pass: same board object
        assert np.array_equal(game.getCanonicalForm(b, p), p * b)
        assert game.stringRepresentation(b) == b.tobytes()
        pi = list(rng.random(cols + 1))
        (b0, p0), (b1, p1) = game.getSymmetries(b, pi)
        assert b0 is b and p0 is pi
        assert np.array_equal(b1, b[:, ::-1])     # np.fliplr of [column][row]: the kept quirk
        assert list(p1) == pi[cols - 1::-1] + [pi[cols]]
        for a in range(cols):
            if want_v[a]:
                (nb, q), (wb, wq) = game.getNextState(b, p, a), _slow_next(b, cols, rows, p, a)
                assert q == wq and np.array_equal(nb, wb) and nb is not b

    for i in range(200):
        _playout(game, rng, visit, fill=i % 2 == 0)
    assert draws[0] >= 1, f"no full-board draw among the playouts of {shape}"


@pytest.mark.parametrize("shape", SHAPES + ((9, 7),))
def test_wins_agree_with_the_square_game_on_embedded_stones(shape):
    """The stones of every ply of 60 playouts, placed in the corner of a max(cols, rows) square
    board: Connect4Game(max) -- pinned to the reference by tests/test_rules_golden.py -- sees a
    run of four exactly where the rectangular game does (the empty cells around add none)."""
    cols, rows = shape
    n = max(cols, rows)
    game, square = Connect4Game(cols, rows=rows), Connect4Game(n)
    rng = np.random.default_rng(7 * cols + rows)
    seen = {1: 0, -1: 0, 0: 0}

    def visit(b, p):
        big = np.zeros((n, n), np.int64)
        big[:cols, :rows] = b
        got, ref = game.getGameEnded(b, p), square.getGameEnded(big, p)
        g = got if got in (1, -1) else 0
        r = ref if ref in (1, -1) else 0
        assert g == r, (shape, got, ref)
        seen[g] += 1

    for i in range(60):
        _playout(game, rng, visit, fill=i % 3 == 0)
    assert seen[-1] > 0 and seen[0] > 0           # a finished game is a loss for the side to move


def test_display_takes_both_extents_from_the_board(capsys):
    game = Connect4Game(7, rows=6)
    b, _ = game.getNextState(game.getInitBoard(), 1, 2)
    Connect4Game.display(b)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 6 + 4 and out[0].split() == [str(j) for j in range(7)]
    assert out[2].startswith("5|") and out[7].startswith("0|") and "X" in out[7]


@pytest.mark.parametrize("shape", [(3, 6), (6, 3), (32, 6)])
def test_unsupported_rectangles_raise_naming_the_shape(shape):
    with pytest.raises(ValueError) as e:
        Connect4Game(shape[0], rows=shape[1])
    assert str(shape[0]) in str(e.value) and str(shape[1]) in str(e.value)


def test_main_passes_board_rows_to_connect4_only():
    """--board_rows / the config key board_rows reach Connect4Game(rows=...); absent: square."""
    import main
    from tictactoe.TicTacToeGame import TicTacToeGame
    a = main.dotdict(game="connect4", board_size=7, board_rows=6)
    g = main.create_game_instance(Connect4Game, a)
    assert g.getBoardSize() == (7, 6)
    g = main.create_game_instance(Connect4Game, main.dotdict(game="connect4", board_size=7))
    assert g.getBoardSize() == (7, 7) and g.win_length == 4
    t = main.create_game_instance(TicTacToeGame, main.dotdict(game="tictactoe", board_size=3,
                                                              board_rows=6))
    assert t.getBoardSize() == (3, 3)
    assert main.parse(["--game", "connect4", "--board_rows", "6"]).board_rows == 6
    assert main.parse(["--game", "connect4"]).board_rows is None
