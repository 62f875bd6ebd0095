"""Times the FrozenLake evaluator routes on one GPU (JSON on stdout):

    python tools/fl_eval_probe.py [--size 4|8] [--reps 200]

  table_fill_us     one az_fl_eval_fwd call over all S+1 states, host round trip included
  per_call_us       predict of one board through the evaluator (AZ_FL_TABLE=0)
  lookup_us         predict of one board from the whole-board table
  kernel_B{n}_us    az_fl_eval_fwd alone (device tensors, events) at B = 1, S+1, 1024
  train_step_us     az_fl_grads + az_clip_grad_norm + az_adam_step on a batch of 32 leaves
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-gnn_amd")]


class Args(dict):
    __getattr__ = dict.__getitem__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import torch
    from azhip.frozenlake import fl_eval_fwd
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    from frozenlake.FrozenLakeNet import FrozenLakeNet
    torch.manual_seed(0)
    game = FrozenLakeGame(map_size=a.size)
    w = FrozenLakeNet(game, Args(lr=1e-3, epochs=1, batch_size=32, embedding_dim=128,
                                 gnn_layers=3))
    n, S = a.size, a.size ** 2
    states = []
    for cell in range(S):
        b = np.zeros((n, n))
        b[cell // n, cell % n] = 1
        states.append(b)
    states.append(np.zeros((n, n)))
    out = {"size": a.size, "E": 128, "L": 3, "reps": a.reps}

    def timed(fn, reps=a.reps):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts)) * 1e6, 2)

    def fill():
        w._table = None
        w._get_table()

    out["table_fill_us"] = timed(fill, 50)
    board = states[n + 1]
    os.environ["AZ_FL_TABLE"] = "0"
    out["per_call_us"] = timed(lambda: w.predict(board))
    os.environ["AZ_FL_TABLE"] = "1"
    out["lookup_us"] = timed(lambda: w.predict(board))
    lists = [w._node_list(b) for b in states]
    for B in (1, S + 1, 1024):
        nodes = np.zeros((B, 5, S), np.float32)
        counts = np.zeros(B, np.int32)
        for i in range(B):
            nl = lists[i % len(lists)]
            nodes[i, :len(nl)] = np.asarray(nl, np.float32).reshape(len(nl), S)
            counts[i] = len(nl)
        dn, dc = torch.from_numpy(nodes).cuda(), torch.from_numpy(counts).cuda()
        pi, v = torch.empty((B, 4), device="cuda"), torch.empty(B, device="cuda")
        for _ in range(10):
            fl_eval_fwd(w.nnet, dn, dc, pi, v, B)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fl_eval_fwd(w.nnet, dn, dc, pi, v, B)
        e1.record()
        torch.cuda.synchronize()
        out[f"kernel_B{B}_us"] = round(e0.elapsed_time(e1) * 1e3 / a.reps, 2)
    rng = np.random.RandomState(0)
    live = [b for b in states[:S] if game.getGameEnded(b, 1) == 0]
    boards = [live[i] for i in rng.randint(0, len(live), 32)]
    pis = rng.dirichlet(np.ones(4), 32)
    vs = rng.choice([-1.0, 1.0], 32)
    w.nnet.params.reset_adam()

    def step():
        w.train_step(boards, pis, vs)
        torch.cuda.synchronize()

    out["train_step_us"] = timed(step, 50)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
