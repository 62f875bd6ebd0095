"""Cost of one evaluate() pass: N random Connect4 examples through nnet.evaluate, timed once after
a small warm-up call (allocations, first-use builds); "seconds" is the whole call, the host's
list-to-array conversions included, which "host_arrays_seconds" times again alone.  Prints one
JSON line.

    python tools/evaluate_probe.py [--n 100000] [--board 7] [--gnn] [--chunk 4096]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-gnn_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--board", type=int, default=7)
    ap.add_argument("--gnn", action="store_true")
    ap.add_argument("--chunk", type=int, default=4096)
    a = ap.parse_args()
    import torch
    from connect4.Connect4Game import Connect4Game
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Net import Connect4NNetWrapper
    game = Connect4Game(a.board)
    args = SimpleNamespace(dropout=0.3, gnn_layers=2, lr=0.001, epochs=1, batch_size=64,
                           use_gnn=a.gnn)
    w = (Connect4GNNWrapper if a.gnn else Connect4NNetWrapper)(game, args)
    rng = np.random.default_rng(0)
    A = game.getActionSize()
    boards = rng.integers(-1, 2, size=(a.n,) + tuple(game.getBoardSize())).astype(np.int8)
    pis = rng.dirichlet(np.ones(A), a.n).astype(np.float32)
    zs = rng.choice([-1.0, 1.0], a.n)
    std = [(boards[i], pis[i], float(zs[i])) for i in range(a.n)]
    gnn = [(boards[i], 1, pis[i], 0.0, pis[i], float(zs[i]), float(zs[i])) for i in range(a.n)] \
        if a.gnn else None
    w.evaluate(std[:a.chunk + 1], None if gnn is None else gnn[:a.chunk + 1], chunk=a.chunk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = w.evaluate(std, gnn, chunk=a.chunk)
    dt = time.perf_counter() - t0
    # the host part alone: the list-to-array conversions evaluate() makes of the same examples
    t0 = time.perf_counter()
    for ex, (ip, iv) in ((std, (1, 2)),) + (((gnn, (4, 5)),) if a.gnn else ()):
        np.ascontiguousarray(np.array([e[0] for e in ex]), dtype=np.int8)
        np.array([e[ip] for e in ex], dtype=np.float32)
        np.array([e[iv] for e in ex]).astype(np.float64).astype(np.float32)
    host = time.perf_counter() - t0
    print(json.dumps({"probe": "evaluate", "n": a.n, "board": a.board, "gnn": a.gnn,
                      "chunk": a.chunk, "seconds": round(dt, 4),
                      "host_arrays_seconds": round(host, 4), "loss": out["loss"],
                      "top1": out["top1"]}))


if __name__ == "__main__":
    main()
