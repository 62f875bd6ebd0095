"""Capture c4_star_leaf.npz from the reference (andrpac/alphazero-gnn) on CPU: the reference's GNN
evaluation of a Connect4 leaf TOGETHER WITH ITS CHILDREN, the star GNNLayer.forward is written for
(gnn_utils.py:38-43: row 0 the target state, the other rows path states).

Run ONLY in the build container, where the read-only reference is mounted:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_star_goldens.py

The reference is imported from /root/reference the way make_goldens.py imports it (nothing is
written there) and exercised through its own entry points; only boards and outputs are stored.

Network: the reference's Connect4GNNWrapper (7x7, 2 GNN layers) with c4_net.npz's `w/` weights and
the synthetic PolicyValueGNN weights azhip.weights.synthetic_state_dict(gnn_spec(3136, 2), seed)
with c4_gnn.npz's seed.  Six positions from seeded random playouts; position p is the star
[leaf] + [canonical next state of every valid action, in action order] cut to n_p = 2, 3, 5, 8, 8, 8
nodes (position 2 has a full column: 6 valid actions, of which the first 4 are kept).  Stored per
position: the boards [n][7][7] (int8, padded to 8 nodes), n, and row 0 of
apply_policy_value_heads(gnn(extract_features(boards))) in eval mode: log pi [8], v.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)

from connect4.Connect4Game import Connect4Game  # noqa: E402
from connect4.Connect4GNN import Connect4GNNWrapper  # noqa: E402

_spec = importlib.util.spec_from_file_location(
    "az_weights", os.path.join(REPO, "alphazero-gnn_amd", "azhip", "weights.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)

NODES = (2, 3, 5, 8, 8, 8)
FULL_COLUMN_AT = 2          # this position must have a full column
SEED = 20


class dotdict(dict):
    def __getattr__(self, name):
        return self[name]


def playout(game, rng, moves, fill=None):
    """Canonical board after `moves` uniformly random legal moves (first filling column `fill`)."""
    b, p = game.getInitBoard(), 1
    if fill is not None:
        for _ in range(7):
            b, p = game.getNextState(b, p, fill)
    for _ in range(moves):
        if game.getGameEnded(b, p) != 0:
            break
        v = game.getValidMoves(game.getCanonicalForm(b, p), 1)
        b, p = game.getNextState(b, p, int(rng.choice(np.flatnonzero(v))))
    return game.getCanonicalForm(b, p)


def star(game, board, n):
    valids = game.getValidMoves(board, 1)
    kids = [game.getCanonicalForm(*game.getNextState(board, 1, a))
            for a in range(game.getActionSize()) if valids[a]]
    return np.stack([board] + kids[:n - 1]).astype(np.int8)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    game = Connect4Game(7)
    g = Connect4GNNWrapper(game, dotdict(lr=0.001, dropout=0.3, epochs=20, batch_size=64,
                                         use_gnn=True, gnn_layers=2))
    c4 = np.load(os.path.join(HERE, "c4_net.npz"))
    g.nnet.load_state_dict({k[2:]: torch.from_numpy(c4[k]) for k in c4.files
                            if k.startswith("w/")})
    seed = int(np.load(os.path.join(HERE, "c4_gnn.npz"))["seed"])
    gsd = W.synthetic_state_dict(W.gnn_spec(3136, 2), seed)
    g.gnn.load_state_dict({k: torch.from_numpy(v) for k, v in gsd.items()})
    del gsd
    g.nnet.eval()
    g.gnn.eval()
    rng = np.random.default_rng(SEED)
    boards = np.zeros((len(NODES), 8, 7, 7), np.int8)
    logp = np.zeros((len(NODES), 8), np.float32)
    v = np.zeros((len(NODES),), np.float32)
    for p, n in enumerate(NODES):
        while True:
            leaf = playout(game, rng, int(rng.integers(2, 16)),
                           fill=int(rng.integers(0, 7)) if p == FULL_COLUMN_AT else None)
            if game.getGameEnded(leaf, 1) != 0:
                continue
            nv = int(np.sum(game.getValidMoves(leaf, 1)[:7]))
            if nv + 1 >= n and (p != FULL_COLUMN_AT or nv == 6):
                break
        nodes = star(game, leaf, n)
        assert nodes.shape[0] == n, (p, nodes.shape)
        boards[p, :n] = nodes
        with torch.no_grad():
            feats = g.extract_features(torch.FloatTensor(nodes.astype(np.float64)))
            lp, val = g.apply_policy_value_heads(g.gnn(feats))
        logp[p], v[p] = lp[0].numpy(), float(val[0, 0])
        print(f"position {p}: n={n} valid={nv} v={v[p]:+.6f}")
    np.savez(os.path.join(HERE, "c4_star_leaf.npz"), boards=boards,
             counts=np.array(NODES, np.int32), logp=logp, v=v, seed=np.int64(SEED))


if __name__ == "__main__":
    main()
