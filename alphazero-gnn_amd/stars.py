"""The child star of a board: the board as row 0, then the canonical next state of every valid
action in action order.  It is what the GNN sees under args.gnn_neighbors -- MCTS.leaf_children
hands rows 1.. to predict_with_gnn, az_game_stars_rect builds the packed form for lock-step
self-play -- and what it is trained on under args.gnn_neighbors_train (NetWrapper._train)."""
import numpy as np


def children(game, board):
    """The canonical next state of every valid action in action order, stepped the way
    MCTS.search_g steps (terminal children included)."""
    valids = game.getValidMoves(board, 1)
    return [game.getCanonicalForm(*game.getNextState(board, 1, a))
            for a in range(game.getActionSize()) if valids[a]]


def _native(game):
    """(kind, shape) when the native engine knows the game and is built, else None."""
    try:
        import mcts_native
        kind, shape = mcts_native.game_shape(game)
        mcts_native.lib()
        return kind, shape
    except (ValueError, RuntimeError, OSError):
        return None


def board_stars(game, boards, native=None, threads=1):
    """boards (canonical) -> (rows int8 [V][cols][rows], offs int32 [B+1]): star b is rows
    offs[b] .. offs[b+1]-1, boards[b] then children(game, boards[b]) -- the layout of
    az_game_stars_rect.  A terminal board, or one with no valid move, gives a one-row star.
    native: True builds the stars with mcts_native.game_stars (an error when the engine does not
    know the game), False with game.getNextState / getCanonicalForm, None (default) natively where
    the engine knows the game.  Both routes give the same arrays."""
    boards = [np.asarray(b) for b in boards]
    live = [game.getGameEnded(b, 1) == 0 for b in boards]
    eng = _native(game) if native is None else None
    if native:
        import mcts_native
        eng = mcts_native.game_shape(game)
    if eng is None:
        stars = [[b] + (children(game, b) if ok else []) for b, ok in zip(boards, live)]
        offs = np.zeros(len(stars) + 1, np.int32)
        offs[1:] = np.cumsum([len(s) for s in stars])
        shape = tuple(game.getBoardSize())
        rows = (np.stack([np.asarray(r) for s in stars for r in s]).astype(np.int8) if stars
                else np.empty((0,) + shape, np.int8))
        return rows, offs
    import mcts_native
    kind, shape = eng
    b8 = (np.stack(boards).astype(np.int8) if boards else np.empty((0,) + tuple(shape), np.int8))
    if all(live):
        return mcts_native.game_stars(kind, shape, b8, threads)
    keep = np.flatnonzero(live)
    lrows, loffs = mcts_native.game_stars(kind, shape, b8[keep], threads)
    sizes = np.ones(len(boards), np.int64)
    sizes[keep] = np.diff(loffs)
    offs = np.zeros(len(boards) + 1, np.int32)
    offs[1:] = np.cumsum(sizes)
    rows = np.empty((int(offs[-1]),) + tuple(shape), np.int8)
    for i, b in enumerate(keep):
        rows[offs[b]:offs[b + 1]] = lrows[loffs[i]:loffs[i + 1]]
    for b in np.flatnonzero(~np.asarray(live)):
        rows[offs[b]] = b8[b]
    return rows, offs
