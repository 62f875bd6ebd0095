"""GNN evaluation of a leaf with its children, timed end to end (host call -> results in host
memory), the routes alternating in one process:

  onecall      predict_star_batch on the one-call evaluator (az_c4_star_eval_fwd)
  parent       the composition as the commit before the evaluator runs it: C4Evaluator.star_forward's
               body (features -> PolicyValueGNN.__call__ on the generic graph calls -> heads of
               every row -> host) once per star, row 0 kept
  composition  predict_star_batch with AZ_B1_MODE=graph (the forest-of-stars composition; reported
               for orientation, it decides nothing)

    python tools/star_eval_probe.py [--blocks 10] [--calls 100] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/star_eval_probe.py --trace 7x7:1

One star of 8 nodes and eight stars of 8 nodes on 7x7 and 7x6 (F = 3136 / 2688) and on 4x4, two
GNN layers; predict_both of one board beside them, the price of a leaf without neighbours.  Every
figure is the median over `blocks` blocks of `calls` calls; the spread is the blocks'
(max - min) / median.  The one-call route is the faster one where it wins by more than the larger
spread.  --trace SHAPE:STARS runs only 200 one-call evaluations of that case (for a kernel trace
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

from azhip import nets  # noqa: E402
from connect4.Connect4GNN import Connect4GNNWrapper  # noqa: E402
from connect4.Connect4Game import Connect4Game  # noqa: E402

SHAPES = ((7, 7), (7, 6), (4, 4))
FLOOR_US = 478.5e6 / 8e12 * 1e6      # the 7x7, L = 2 leaf reads 478.5 MB once; 8 TB/s peak


def wrapper(shape, seed=0):
    torch.manual_seed(seed)
    rows = None if shape[0] == shape[1] else shape[1]
    return Connect4GNNWrapper(Connect4Game(shape[0], rows=rows),
                              SimpleNamespace(gnn_layers=2, dropout=0.3))


def parent_route(w, stars):
    """C4Evaluator.star_forward on each star, row 0 kept."""
    out = []
    for nodes in stars:
        b = nets.boards_to_device(np.asarray(nodes), w.device)
        logp, _, v = w.nnet.heads(w.gnn(w.nnet.features(b)), want_pi=False)
        out.append((logp.cpu().numpy()[0], v.cpu().numpy()[0]))
    return out


def ab(fns, blocks, calls):
    """fns: {route: (env or None, callable)}.  Alternating blocks -> {route: {us, spread}}."""
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
    one, par = out["onecall"], out["parent"]
    gap = abs(one["us"] - par["us"]) / min(one["us"], par["us"])
    out["parent_over_onecall"] = round(par["us"] / one["us"], 3)
    out["verdict"] = ("tie" if gap <= max(one["spread"], par["spread"])
                      else "onecall" if one["us"] < par["us"] else "parent")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="SHAPE:STARS, e.g. 7x7:1")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    if a.trace:
        shape, n = a.trace.split(":")
        shape = tuple(int(s) for s in shape.split("x"))
        w = wrapper(shape)
        stars = [list(rng.integers(-1, 2, size=(8,) + shape)) for _ in range(int(n))]
        for _ in range(200):
            w.predict_star_batch(stars)
        assert w.star_route == "onecall"
        return
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls,
           "gnn_layers": 2, "nodes_per_star": 8, "floor_us_7x7": round(FLOOR_US, 1),
           "unit": "us per call, host call to results in host memory"}
    for shape in SHAPES:
        w = wrapper(shape)
        tag = f"{shape[0]}x{shape[1]}"
        one = rng.integers(-1, 2, size=shape).astype(np.int64)
        res[f"{tag}/predict_both_b1"] = ab(
            {"onecall": (None, lambda: w.predict_both(one[None])),
             "parent": (None, lambda: w.predict_both(one[None]))}, a.blocks, a.calls)["onecall"]
        for n in (1, 8):
            stars = [list(rng.integers(-1, 2, size=(8,) + shape)) for _ in range(n)]
            calls = a.calls if n == 1 else max(10, a.calls // 4)
            r = ab({"onecall": (None, lambda: w.predict_star_batch(stars)),
                    "parent": (None, lambda: parent_route(w, stars)),
                    "composition": ("graph", lambda: w.predict_star_batch(stars))},
                   a.blocks, calls)
            # the routes computed the same thing (a timing of wrong results cannot pass)
            pi, v = w.predict_star_batch(stars)
            ref = parent_route(w, stars)
            r["max_abs_diff_pi"] = float(max(np.abs(pi[i] - np.exp(ref[i][0])).max()
                                             for i in range(n)))
            r["max_abs_diff_v"] = float(max(abs(v[i] - ref[i][1]) for i in range(n)))
            res[f"{tag}/stars{n}"] = r
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
