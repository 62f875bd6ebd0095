"""FrozenLake for AlphaZero-style MCTS (reference frozenlake/FrozenLakeGame.py:4-228), without
gymnasium: the reference takes only the map from it (`env.unwrapped.desc`) and runs its own
deterministic transitions, so the two standard maps are written out here.

The board is an N x N float array with a single 1 at the agent's cell; the all-zero board is
the special "empty" state whose every move leads to the start.  Actions: 0 up, 1 right, 2 down,
3 left.  One player: the canonical form is the board, the only symmetry the identity."""
import numpy as np

MAPS = {
    4: ["SFFF", "FHFH", "FFFH", "HFFG"],
    8: ["SFFFFFFF", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF", "FFFHFFFF", "FHHFFFHF", "FHFFHFHF",
        "FFFHFFFG"],
}
DIRECTIONS = [(-1, 0), (0, 1), (1, 0), (0, -1)]
MIN_SIZE, MAX_SIZE = 2, 8      # the HIP evaluator holds a board of up to 64 cells


class FrozenLakeGame:
    def __init__(self, map_size=4, custom_map=None, is_slippery=False, render_mode=None):
        self.is_two_player = False            # tells MCTS not to negate values on the way up
        self.action_size = 4
        self.is_slippery = is_slippery        # kept; transitions are deterministic either way
        self.render_mode = render_mode
        if custom_map is not None:
            rows = [str(r) for r in custom_map]
        else:
            rows = MAPS[8] if map_size == 8 else MAPS[4]
        n = len(rows)
        if not MIN_SIZE <= n <= MAX_SIZE or any(len(r) != n for r in rows):
            raise ValueError(f"FrozenLakeGame: the map must be square with {MIN_SIZE} to "
                             f"{MAX_SIZE} cells a side, got {n} row(s) of length(s) "
                             f"{sorted({len(r) for r in rows})}")
        # single bytes, as gymnasium's desc: desc[r][c] == b'H'
        self.desc = np.asarray([list(r) for r in rows], dtype="c")
        self.map_size = n
        self.goal_pos = self.find_goal_position()
        self.board = None                     # the last board getNextState made (for render)

    def _find(self, letter):
        hits = np.argwhere(self.desc == letter)
        return (int(hits[0][0]), int(hits[0][1])) if len(hits) else None

    def find_goal_position(self):
        return self._find(b"G") or (self.map_size - 1, self.map_size - 1)

    def getInitBoard(self):
        board = np.zeros((self.map_size, self.map_size))
        board[self._find(b"S") or (0, 0)] = 1
        return board

    def getBoardSize(self):
        return (self.map_size, self.map_size)

    def getActionSize(self):
        return self.action_size

    @staticmethod
    def _pos(board):
        return np.unravel_index(np.argmax(board), board.shape)

    def getNextState(self, board, player, action):
        if np.sum(board) == 0:
            return self.getInitBoard(), player
        row, col = self._pos(board)
        dr, dc = DIRECTIONS[action]
        nr, nc = row + dr, col + dc
        if not (0 <= nr < self.map_size and 0 <= nc < self.map_size):
            nr, nc = row, col
        nxt = np.zeros_like(board)
        nxt[nr, nc] = 1
        self.board = nxt
        return nxt, player

    def getValidMoves(self, board, player):
        """Moves that stay on the grid; none on a terminal cell.  Holes stay valid: the agent
        learns to avoid them from the reward."""
        valid = np.ones(self.action_size, dtype=np.int8)
        if self.getGameEnded(board, player) != 0:
            return np.zeros(self.action_size, dtype=np.int8)
        if np.sum(board) == 0:
            return valid
        row, col = self._pos(board)
        if row == 0:
            valid[0] = 0
        if row == self.map_size - 1:
            valid[2] = 0
        if col == 0:
            valid[3] = 0
        if col == self.map_size - 1:
            valid[1] = 0
        return valid

    def getGameEnded(self, board, player):
        """1.0 on the goal, -1.0 in a hole, 0 otherwise (the empty board included)."""
        if np.sum(board) == 0:
            return 0
        row, col = self._pos(board)
        if self.desc[row][col] == b"G":
            return 1.0
        if self.desc[row][col] == b"H":
            return -1.0
        return 0

    def getCanonicalForm(self, board, player):
        return board

    def getSymmetries(self, board, pi):
        return [(board, pi)]

    def stringRepresentation(self, board):
        if np.sum(board) == 0:
            return "empty"
        row, col = self._pos(board)
        return f"{row},{col}"

    def render(self):
        """Print the map with the agent's cell in brackets (text only)."""
        pos = None if self.board is None else tuple(int(i) for i in self._pos(self.board))
        for r in range(self.map_size):
            print("".join(f"[{self.desc[r][c].decode()}]" if (r, c) == pos
                          else f" {self.desc[r][c].decode()} " for c in range(self.map_size)))
