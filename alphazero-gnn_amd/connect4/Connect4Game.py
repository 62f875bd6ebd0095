"""Connect4 rules (host), behaviour-identical to the reference connect4/Connect4Game.py on the
square boards it can express, and the same rules on rectangular ones.

A board of `board_size` columns and `rows` rows (rows=None: square, the reference's n x n board)
plus a pass action (Connect4Game.py:135-141); board[x][y] with x the column and y the row counted
from the bottom; pieces fall to the lowest empty y.  Connect4Game(7, rows=6) is the standard game.
There is ONE rule set: every method below is written for (columns, rows) and a square board is the
case rows == columns, so Connect4Game(n, rows=n) equals Connect4Game(n) in every output.  Win
checks are bitboard tests instead of Python loops (same boolean result).  Kept quirks:
  * the pass action is only legal when every column is full, and a full board is a draw
    worth 1e-4 (Connect4Game.py:154-183);
  * getSymmetries mirrors the board with np.fliplr, which on a [column][row] array flips the
    ROW (gravity) axis while pi is mirrored across columns (Connect4Game.py:208-212).  The two
    expressions are the reference's on every board shape, on purpose.
"""
import numpy as np


def _has_run(mask, w):
    """True when `mask` (bool [cols, rows], [column x][row y]) has w consecutive Trues along a
    column, a row or either diagonal (the four scans of Connect4Game.py:75-97), as a bitboard
    test: cell (x, y) is bit x*(rows+1) + y, the extra bit per column is always 0 so no run wraps,
    and a run of w along direction step s exists iff bb & bb>>s & ... & bb>>(w-1)s != 0."""
    cols, rows = mask.shape
    if w > max(cols, rows):
        return False
    padded = np.zeros((cols, rows + 1), dtype=bool)
    padded[:, :rows] = mask
    bb = int.from_bytes(np.packbits(padded.ravel(), bitorder="little").tobytes(), "little")
    for s in (1, rows + 1, rows + 2, rows):   # along y, along x, (x+1, y+1), (x+1, y-1)
        m = bb
        for k in range(1, w):
            m &= bb >> (k * s)
            if not m:
                break
        if m:
            return True
    return False


class Connect4Game:
    is_two_player = True

    def __init__(self, board_size=7, rows=None):
        self.board_size = board_size                  # columns
        self.rows = board_size if rows is None else rows
        # in a row to win: min(4, n) on the reference's square board, 4 once rows are given
        self.win_length = min(4, board_size) if rows is None else 4
        if self.rows != board_size and (board_size < 4 or self.rows < 4 or board_size + 1 > 32):
            raise ValueError(f"Connect4Game: unsupported board of {board_size} columns x "
                             f"{self.rows} rows (a rectangular board needs columns >= 4, "
                             f"rows >= 4 and columns + 1 <= 32 actions)")

    def getInitBoard(self):
        return np.zeros((self.board_size, self.rows), dtype=np.int64)

    def getBoardSize(self):
        return (self.board_size, self.rows)

    def getActionSize(self):
        return self.board_size + 1

    def getNextState(self, board, player, action):
        n = self.board_size
        if action == n:                       # pass: same board object, other player
            return (board, -player)
        nb = np.copy(board)
        empty = np.flatnonzero(nb[action] == 0)
        assert empty.size > 0, "Column is full!"
        nb[action, empty[0]] = player
        return (nb, -player)

    def getValidMoves(self, board, player):
        n = self.board_size
        valids = np.zeros(n + 1, dtype=np.int64)
        open_cols = np.asarray(board)[:, self.rows - 1] == 0
        if not open_cols.any():
            valids[-1] = 1
        else:
            valids[:n] = open_cols
        return valids

    def getGameEnded(self, board, player):
        b = np.asarray(board)
        w = self.win_length
        if _has_run(b == player, w):
            return 1
        if _has_run(b == -player, w):
            return -1
        if (b[:, self.rows - 1] == 0).any():
            return 0
        return 1e-4

    def getCanonicalForm(self, board, player):
        return player * board

    def getSymmetries(self, board, pi):
        n = self.board_size
        assert len(pi) == n + 1
        mirror_pi = np.copy(pi)
        mirror_pi[:n] = np.asarray(pi)[n - 1::-1] if n > 0 else mirror_pi[:n]
        return [(board, pi), (np.fliplr(board), mirror_pi)]

    def stringRepresentation(self, board):
        return board.tobytes()

    @staticmethod
    def display(board):
        n, rows = board.shape
        cols = " ".join(str(j) for j in range(n))
        print("  " + cols + " ")
        print(" +" + "--" * n + "+")
        for i in range(rows - 1, -1, -1):
            row = "".join({-1: "O ", 1: "X "}.get(int(board[j][i]), ". ") for j in range(n))
            print(f"{i}|{row}|")
        print(" +" + "--" * n + "+")
        print("  " + cols + " ")
