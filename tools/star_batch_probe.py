"""Batched star evaluation, timed end to end (host call -> results in host memory), the routes
alternating in one process:

  batched      predict_both_stars (az_gnn_star_batch_infer; also returns the leaves' standard heads)
  composition  _star_compose on the same stars (the forest-of-stars DeviceGraph through
               az_gnn_layer_fwd: the only route for more than 8 stars before the batched one)
  onecall      ceil(B / 8) calls of the one-call evaluator (az_c4_star_eval_fwd)

    python tools/star_batch_probe.py [--blocks 10] [--out FILE.json]
    python tools/star_batch_probe.py --selfplay [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/star_batch_probe.py --trace 7x6:512

Evaluation: 7x7, 7x6 and 4x4 (F = 3136 / 2688 / 1024), two GNN layers, stars of 8 nodes, B = 16,
64, 512 and 2,048.  Every figure is the median over `blocks` blocks; the spread is the blocks'
(max - min) / median.  The batched route is the default for a (board, B) class only where it beats
BOTH others by more than the larger of their spreads.  --selfplay: 7x6, 64 episodes, 25
simulations, gnn_neighbors_lockstep at parallel_games = 64 against the sequential Python search
with gnn_neighbors, each once, episodes / s.  --trace SHAPE:STARS runs only 20 batched calls of
that case (for a kernel trace taken in a run of its own).  Prints one JSON document.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-gnn_amd"))

from connect4.Connect4GNN import Connect4GNNWrapper  # noqa: E402
from connect4.Connect4Game import Connect4Game  # noqa: E402

SHAPES = ((7, 7), (7, 6), (4, 4))
BATCHES = (16, 64, 512, 2048)
NODES = 8


def game_of(shape):
    return Connect4Game(shape[0], rows=None if shape[0] == shape[1] else shape[1])


def wrapper(shape, seed=0, **extra):
    torch.manual_seed(seed)
    return Connect4GNNWrapper(game_of(shape), SimpleNamespace(gnn_layers=2, dropout=0.3, **extra))


def stars_of(shape, B, rng):
    lists = [list(rng.integers(-1, 2, size=(NODES,) + shape).astype(np.int8)) for _ in range(B)]
    rows = np.concatenate([np.stack(s) for s in lists])
    offs = (np.arange(B + 1) * NODES).astype(np.int32)
    return lists, rows, offs


def routes(w, lists, rows, offs):
    def onecall():
        out = [w.predict_star_batch(lists[i:i + 8]) for i in range(0, len(lists), 8)]
        assert w.star_route == "onecall"
        return np.concatenate([p for p, _ in out]), np.concatenate([v for _, v in out])

    def batched():
        _, _, gpi, gv = w.predict_both_stars(rows, offs)
        return gpi, gv

    return {"batched": batched, "composition": lambda: w._star_compose(lists), "onecall": onecall}


def ab(fns, blocks, calls):
    per = {r: [] for r in fns}
    for f in fns.values():
        for _ in range(2):
            f()
    for _ in range(blocks):
        for r, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            per[r].append((time.perf_counter() - t0) / calls * 1e6)
    out = {}
    for r, xs in per.items():
        med = float(np.median(xs))
        out[r] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4),
                  "blocks": [round(x, 1) for x in xs]}
    b = out["batched"]
    others = {r: out[r] for r in out if r != "batched"}
    best = min(others, key=lambda r: others[r]["us"])
    bar = max(o["spread"] for o in others.values())
    wins = all(o["us"] > b["us"] * (1.0 + bar) for o in others.values())
    out["verdict"] = "batched" if wins else best if \
        others[best]["us"] * (1.0 + max(bar, b["spread"])) < b["us"] else "tie"
    out["batched_speedup_over_best_other"] = round(others[best]["us"] / b["us"], 3)
    return out


def selfplay(out_path):
    from Coach import Coach
    from selfplay import episode_seeds, play_episodes_engine
    shape, n = (7, 6), 64
    base = dict(numEps=n, numMCTSSims=25, cpuct=1.0, tempThreshold=15, use_gnn=True, expand_by=5,
                gnn_neighbors=True)
    game = game_of(shape)
    w = wrapper(shape, **base)
    res = {"device": torch.cuda.get_device_name(0), "board": "7x6", "episodes": n,
           "numMCTSSims": 25, "expand_by": 5}
    args = SimpleNamespace(gnn_neighbors_lockstep=True, parallel_games=64, gnn_layers=2,
                           dropout=0.3, **base)
    eps = list(range(n))
    seeds = episode_seeds(1, eps)
    play_episodes_engine(game, w, args, eps[:8], seeds, parallel_games=8)        # warm-up
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = play_episodes_engine(game, w, args, eps, seeds, parallel_games=64, stats=stats)
    dt = time.perf_counter() - t0
    res["lockstep_G64"] = {"seconds": round(dt, 3), "episodes_per_s": round(n / dt, 2),
                           "rounds": stats.get("rounds"), "rows": stats.get("rows"),
                           "examples": sum(len(out[e][0]) for e in eps)}
    seq_args = SimpleNamespace(parallel_games=1, gnn_layers=2, dropout=0.3, **base)
    coach = Coach(game, w, seq_args)
    np.random.seed(1)
    coach.executeEpisode()                                                       # warm-up
    t0 = time.perf_counter()
    got = coach.selfPlay()
    dt = time.perf_counter() - t0
    res["sequential_python"] = {"seconds": round(dt, 3), "episodes_per_s": round(n / dt, 3),
                                "examples": sum(len(s) for s, _ in got)}
    res["speedup"] = round(res["lockstep_G64"]["episodes_per_s"] /
                           res["sequential_python"]["episodes_per_s"], 1)
    emit(res, out_path)


def emit(res, out_path):
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="SHAPE:STARS, e.g. 7x6:512")
    ap.add_argument("--selfplay", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    if a.selfplay:
        return selfplay(a.out)
    if a.trace:
        shape, n = a.trace.split(":")
        shape = tuple(int(s) for s in shape.split("x"))
        w = wrapper(shape)
        _, rows, offs = stars_of(shape, int(n), rng)
        for _ in range(20):
            w.predict_both_stars(rows, offs)
        return
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "gnn_layers": 2,
           "nodes_per_star": NODES,
           "unit": "us per B stars, host call to results in host memory"}
    for shape in SHAPES:
        w = wrapper(shape)
        tag = f"{shape[0]}x{shape[1]}"
        for B in BATCHES:
            lists, rows, offs = stars_of(shape, B, rng)
            fns = routes(w, lists, rows, offs)
            r = ab(fns, a.blocks, max(2, 512 // B))
            # the routes computed the same thing (a timing of wrong results cannot pass)
            got = {k: f() for k, f in fns.items()}
            for k in ("composition", "onecall"):
                r[f"max_abs_diff_pi_vs_{k}"] = float(np.abs(got["batched"][0] - got[k][0]).max())
                r[f"max_abs_diff_v_vs_{k}"] = float(np.abs(got["batched"][1] - got[k][1]).max())
            r["us_per_star_batched"] = round(r["batched"]["us"] / B, 2)
            res[f"{tag}/B{B}"] = r
            print(tag, B, {k: r[k]["us"] for k in fns}, r["verdict"], file=sys.stderr, flush=True)
        del w
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
