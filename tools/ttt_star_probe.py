"""GNN evaluation of a TicTacToe leaf with its children, timed end to end (host call -> results in
host memory), the two routes alternating in one process:

  onecall      predict_star_batch under args.gnn_neighbors on the one-call evaluator
               (az_ttt_star_eval_fwd)
  composition  predict_star_batch with AZ_B1_MODE=graph: the forest-of-stars composition on the
               generic graph calls, the code these stars ran before the evaluator existed

    python tools/ttt_star_probe.py [--blocks 10] [--calls 100] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/ttt_star_probe.py --trace 5:1

One star and eight stars of n^2 + 1 nodes (the opening) on 3x3, 4x4 and 5x5 (F = 128 / 512 /
1,152), two GNN layers; predict_both of one board beside them, the price of a leaf without
neighbours.  Every figure is the median over `blocks` blocks of `calls` calls; the spread is the
blocks' (max - min) / median.  The one-call route is the faster one where it wins by more than the
larger spread.  --trace N:STARS runs only 200 one-call evaluations of that case (for a kernel trace
taken in a run of its own).  Prints one JSON document.
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

from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper  # noqa: E402
from tictactoe.TicTacToeGame import TicTacToeGame  # noqa: E402

SIDES = (3, 4, 5)


def wrapper(n, seed=0):
    torch.manual_seed(seed)
    return TicTacToeGNNWrapper(TicTacToeGame(n), SimpleNamespace(gnn_layers=2, dropout=0.3,
                                                                  gnn_neighbors=True))


def full_stars(rng, n, count):
    """`count` stars of n^2 + 1 random boards each."""
    return [list(rng.integers(-1, 2, size=(n * n + 1, n, n))) for _ in range(count)]


def ab(fns, blocks, calls):
    """fns: {route: (AZ_B1_MODE or None, callable)}.  Alternating blocks -> {route: {us, spread}}."""
    def use(env):
        os.environ.pop("AZ_B1_MODE", None)
        if env:
            os.environ["AZ_B1_MODE"] = env
    per = {r: [] for r in fns}
    for r, (env, f) in fns.items():
        use(env)
        for _ in range(max(10, calls // 4)):
            f()
    for _ in range(blocks):
        for r, (env, f) in fns.items():
            use(env)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            per[r].append((time.perf_counter() - t0) / calls * 1e6)
    use(None)
    out = {}
    for r, xs in per.items():
        med = float(np.median(xs))
        out[r] = {"us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 4),
                  "blocks": [round(x, 2) for x in xs]}
    if "composition" in out:
        one, par = out["onecall"], out["composition"]
        gap = abs(one["us"] - par["us"]) / min(one["us"], par["us"])
        out["composition_over_onecall"] = round(par["us"] / one["us"], 3)
        out["verdict"] = ("tie" if gap <= max(one["spread"], par["spread"])
                          else "onecall" if one["us"] < par["us"] else "composition")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="N:STARS, e.g. 5:1")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    if a.trace:
        n, count = (int(s) for s in a.trace.split(":"))
        w = wrapper(n)
        stars = full_stars(rng, n, count)
        for _ in range(200):
            w.predict_star_batch(stars)
        assert w.star_route == "onecall"
        return
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls,
           "gnn_layers": 2, "nodes_per_star": "n^2 + 1",
           "unit": "us per call, host call to results in host memory"}
    for n in SIDES:
        w = wrapper(n)
        tag = f"{n}x{n}"
        one = rng.integers(-1, 2, size=(n, n)).astype(np.int64)
        res[f"{tag}/predict_both_b1"] = ab(
            {"onecall": (None, lambda: w.predict_both(one[None]))}, a.blocks, a.calls)["onecall"]
        for count in (1, 8):
            stars = full_stars(rng, n, count)
            calls = a.calls if count == 1 else max(10, a.calls // 2)

            def run(route):
                out = w.predict_star_batch(stars)
                assert w.star_route == route, (w.star_route, route)
                return out

            r = ab({"onecall": (None, lambda: run("onecall")),
                    "composition": ("graph", lambda: run("composition"))}, a.blocks, calls)
            # the routes computed the same thing (a timing of wrong results cannot pass)
            pi, v = run("onecall")
            os.environ["AZ_B1_MODE"] = "graph"
            cpi, cv = run("composition")
            os.environ.pop("AZ_B1_MODE")
            r["max_abs_diff_pi"] = float(np.abs(pi - cpi).max())
            r["max_abs_diff_v"] = float(np.abs(v - cv).max())
            res[f"{tag}/stars{count}"] = r
        del w
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
