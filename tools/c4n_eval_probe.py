"""Connect4 evaluation routes on boards other than 7x7, timed end to end (host call -> results in
host memory), A/B in one process: the hipGraph / pinned-ring routes (AZ_B1_MODE=graph) against
the one-call route (az_c4n_eval_fwd).

    python tools/c4n_eval_probe.py [--blocks 12] [--calls 200] [--sizes 5,8] [--out FILE.json]

For every board size: batch-1 predict, predict_with_gnn, predict_both and predict_both of 8 rows;
a lock-step round of 2,048 boards (predict_both_async(...).result()); the arena leg (5x5, 8 games
at 25 simulations) with the speculative hit rate; and device time (events around back-to-back
launches) of the fused trunk against the two az_conv3x3_relu_fwd launches at 1, 8, 256 and 2,048
boards.  Every end-to-end figure is the median over `blocks` blocks of `calls` calls, the routes
alternating block by block; the spread is the blocks' (max - min) / median.  Prints one JSON
document.
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

ROUTES = ("graph", "direct")


def wrapper(n, route, seed=0):
    """A Connect4GNNWrapper whose calls take `route` (the environment is read per call, so it is
    set again around every timed block).  One GNN layer: the per-row evaluation runs only
    output_transform, and the layers of an 8x8 net are 335 MB each."""
    os.environ["AZ_B1_MODE"] = route
    torch.manual_seed(seed)
    return Connect4GNNWrapper(Connect4Game(n), SimpleNamespace(gnn_layers=1, dropout=0.3))


def ab(fns, blocks, calls):
    """fns: {route: callable}.  Alternating blocks -> {route: {us, spread, blocks}}."""
    per = {r: [] for r in fns}
    for r, f in fns.items():                      # warm-up: graph capture, scratch, caches
        os.environ["AZ_B1_MODE"] = r
        for _ in range(max(20, calls // 4)):
            f()
    for _ in range(blocks):
        for r, f in fns.items():
            os.environ["AZ_B1_MODE"] = r
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            per[r].append((time.perf_counter() - t0) / calls * 1e6)
    out = {}
    for r, xs in per.items():
        med = float(np.median(xs))
        out[r] = {"us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 4),
                  "blocks": [round(x, 2) for x in xs]}
    g, d = out.get("graph"), out.get("direct")
    if g and d:
        out["direct_over_graph"] = round(d["us"] / g["us"], 4)
        # faster by more than the run-to-run spread of either route, else a tie
        gap = abs(d["us"] - g["us"]) / min(d["us"], g["us"])
        out["verdict"] = ("tie" if gap <= max(g["spread"], d["spread"])
                          else "direct" if d["us"] < g["us"] else "graph")
    return out


def device_us(f, reps, rounds=5):
    """Median device time of f() in us: events around `reps` back-to-back calls."""
    for _ in range(5):
        f()
    xs = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        xs.append(e0.elapsed_time(e1) / reps * 1e3)
    return round(float(np.median(xs)), 2)


def trunk_times(w, n, rng):
    """Fused trunk (and trunk + heads) against the two conv launches (+ az_heads_fwd), device
    time per call."""
    from azhip import ops
    out = {}
    for B in (1, 8, 256, 2048):
        b = torch.from_numpy(rng.integers(-1, 2, size=(B, n, n)).astype(np.int8)).to(w.device)
        feat = torch.empty((B, 64 * n * n), device=w.device)
        reps = 200 if B <= 256 else 50
        out[str(B)] = {
            "fused_trunk_us": device_us(lambda: ops.c4n_trunk(b, w.nnet.params, out=feat), reps),
            "two_conv_us": device_us(lambda: w.nnet.features_eager(b), reps),
            "fused_trunk_heads_us": device_us(
                lambda: ops.c4n_trunk_heads(b, w.nnet.params, feat=feat), reps),
            "two_conv_heads_us": device_us(
                lambda: w.nnet.heads(w.nnet.features_eager(b)), reps),
        }
    return out


def arena_leg(n, route, games, sims):
    from Arena import Arena
    from mcts_native import ArenaPlayer
    game = Connect4Game(n)
    args = SimpleNamespace(numMCTSSims=sims, cpuct=1.0, use_gnn=True, gnn_layers=1)
    a, b = wrapper(n, route, 1), wrapper(n, route, 2)
    np.random.seed(7)
    p1, p2 = ArenaPlayer(game, a, args), ArenaPlayer(game, b, args)
    Arena(p1, p2, game).playGames(2)              # warm-up (graphs / descriptors)
    c0, h0 = p1.calls + p2.calls, p1.hits + p2.hits
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wld = Arena(p1, p2, game).playGames(games)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    calls, hits = p1.calls + p2.calls - c0, p1.hits + p2.hits - h0
    return {"seconds": round(dt, 4), "games": games, "sims": sims, "wld": [int(x) for x in wld],
            "net_calls": calls, "spec_hits": hits,
            "spec_hit_rate": round(hits / max(1, calls + hits), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sizes", default="5,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls,
           "unit": "us per call, host call to results in host memory", "n": {}}
    rng = np.random.default_rng(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        ws = {r: wrapper(n, r) for r in ROUTES}
        ws["direct"].nnet.params.copy_flat_(ws["graph"].nnet.params.flat)
        ws["direct"].gnn.params.copy_flat_(ws["graph"].gnn.params.flat)
        one = rng.integers(-1, 2, size=(n, n)).astype(np.int64)
        eight = rng.integers(-1, 2, size=(8, n, n)).astype(np.int64)
        big = rng.integers(-1, 2, size=(2048, n, n)).astype(np.int8)
        r = {}
        r["predict_b1"] = ab({k: (lambda w=w: w.predict(one)) for k, w in ws.items()},
                             a.blocks, a.calls)
        r["predict_with_gnn_b1"] = ab({k: (lambda w=w: w.predict_with_gnn(one))
                                       for k, w in ws.items()}, a.blocks, a.calls)
        r["predict_both_b1"] = ab({k: (lambda w=w: w.predict_both(one[None]))
                                   for k, w in ws.items()}, a.blocks, a.calls)
        r["predict_both_b8"] = ab({k: (lambda w=w: w.predict_both(eight))
                                   for k, w in ws.items()}, a.blocks, a.calls)
        r["lockstep_round_2048"] = ab({k: (lambda w=w: w.predict_both_async(big).result())
                                       for k, w in ws.items()}, a.blocks, max(10, a.calls // 10))
        # the same bits on both routes (checked here so a timing of wrong results cannot pass)
        os.environ["AZ_B1_MODE"] = "graph"
        g = ws["graph"].predict_both(eight)
        os.environ["AZ_B1_MODE"] = "direct"
        d = ws["direct"].predict_both(eight)
        r["both8_bit_identical"] = all(np.array_equal(x, y) for x, y in zip(g, d))
        r["trunk_device_us"] = trunk_times(ws["direct"], n, rng)
        res["n"][str(n)] = r
        del ws
        torch.cuda.empty_cache()
    res["arena_c4_5x5"] = {k: arena_leg(5, k, 8, 25) for k in ROUTES}
    os.environ.pop("AZ_B1_MODE", None)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
