"""What batch-invariant star evaluation costs (config key batch_invariant with gnn_neighbors;
DESIGN §10), timed end to end (host call -> results in host memory), the two wrappers alternating
in one process:

  key_off   predict_both_stars on the default route (az_gnn_star_batch_infer: az_gemm_f32's
            dispatch picks the tiles by the row count)
  key_on    predict_both_stars under args.batch_invariant (az_star_eval_exact_fwd: every product
            an exact-fp32 GEMM, the same bits at any batch)

    python tools/star_exact_probe.py [--blocks 10] [--out FILE.json]

4x4 and 7x7 (F = 1024 / 3136), two GNN layers, stars of 8 nodes, B = 16, 256 and 2,048.  Every
figure is the median over `blocks` blocks; the spread is the blocks' (max - min) / median.  This
is a reproducibility mode: the ratio is the price that is reported, not a pass criterion.  Prints
one JSON document.
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

SHAPES = ((4, 4), (7, 7))
BATCHES = (16, 256, 2048)
NODES = 8


def wrapper(shape, key):
    torch.manual_seed(0)
    return Connect4GNNWrapper(Connect4Game(shape[0]),
                              SimpleNamespace(gnn_layers=2, dropout=0.3, batch_invariant=key))


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
    out["price"] = round(out["key_on"]["us"] / out["key_off"]["us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "nodes": NODES, "gnn_layers": 2, "cases": {}}
    rng = np.random.default_rng(3)
    for shape in SHAPES:
        off, on = wrapper(shape, False), wrapper(shape, True)
        for B in BATCHES:
            rows = rng.integers(-1, 2, size=(B * NODES,) + shape).astype(np.int8)
            offs = (np.arange(B + 1) * NODES).astype(np.int32)
            fns = {"key_off": lambda: off.predict_both_stars(rows, offs),
                   "key_on": lambda: on.predict_both_stars(rows, offs)}
            x, y = fns["key_off"](), fns["key_on"]()
            assert on.star_route == "exact"
            err = max(float(np.abs(p - q).max()) for p, q in zip(x, y))
            case = ab(fns, a.blocks, 20 if B <= 256 else 5)
            case["max_abs_diff_between_routes"] = err
            res["cases"][f"{shape[0]}x{shape[1]}/B{B}"] = case
        del off, on
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
