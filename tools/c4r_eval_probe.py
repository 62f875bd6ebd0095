"""Connect4 evaluation routes on the standard 7 x 6 board, timed end to end (host call -> results
in host memory), A/B in one process: the hipGraph / pinned-ring routes (AZ_B1_MODE=graph) against
the one-call route (az_c4r_eval_fwd).  tools/c4n_eval_probe.py's method on the rectangular board.

    python tools/c4r_eval_probe.py [--blocks 10] [--calls 100] [--out FILE.json]

predict, predict_with_gnn and predict_both at 1 and 8 boards; a lock-step round of 2,048 boards
(predict_both_async(...).result()); and device time (events around back-to-back launches) of the
fused trunk against the two az_conv3x3_relu_fwd launches at 1, 256 and 2,048 boards, with the 7x7
board's MFMA trunk (another network, 49 positions) beside them for orientation.  Every end-to-end
figure is the median over `blocks` blocks of `calls` calls, the routes alternating block by block;
the spread is the blocks' (max - min) / median.  Prints one JSON document.
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-gnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from c4n_eval_probe import ROUTES, ab, device_us  # noqa: E402
from connect4.Connect4GNN import Connect4GNNWrapper  # noqa: E402
from connect4.Connect4Game import Connect4Game  # noqa: E402

SHAPE = (7, 6)


def wrapper(route, seed=0, shape=SHAPE):
    """A Connect4GNNWrapper whose calls take `route` (read per call, so it is set again around
    every timed block).  One GNN layer: the per-row evaluation runs only output_transform."""
    os.environ["AZ_B1_MODE"] = route
    torch.manual_seed(seed)
    rows = None if shape[0] == shape[1] else shape[1]
    return Connect4GNNWrapper(Connect4Game(shape[0], rows=rows),
                              SimpleNamespace(gnn_layers=1, dropout=0.3))


def trunk_times(w, w77, rng):
    """Fused trunk (and trunk + heads) against the two conv launches (+ az_heads_fwd), device
    time per call; the 7x7 MFMA trunk at the same batch sizes."""
    from azhip import ops
    out = {}
    for B in (1, 256, 2048):
        b = torch.from_numpy(rng.integers(-1, 2, size=(B,) + SHAPE).astype(np.int8)).to(w.device)
        b77 = torch.from_numpy(rng.integers(-1, 2, size=(B, 7, 7)).astype(np.int8)).to(w.device)
        feat = torch.empty((B, 64 * SHAPE[0] * SHAPE[1]), device=w.device)
        feat77 = torch.empty((B, 3136), device=w.device)
        reps = 200 if B <= 256 else 50
        out[str(B)] = {
            "fused_trunk_us": device_us(lambda: ops.c4r_trunk(b, w.nnet.params, out=feat), reps),
            "two_conv_us": device_us(lambda: w.nnet.features_eager(b), reps),
            "fused_trunk_heads_us": device_us(
                lambda: ops.c4r_trunk_heads(b, w.nnet.params, feat=feat), reps),
            "two_conv_heads_us": device_us(
                lambda: w.nnet.heads(w.nnet.features_eager(b)), reps),
            "mfma_trunk_7x7_us": device_us(
                lambda: ops.c4_trunk(b77, w77.nnet.params, out=feat77), reps),
        }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls,
           "board": list(SHAPE),
           "unit": "us per call, host call to results in host memory"}
    rng = np.random.default_rng(0)
    ws = {r: wrapper(r) for r in ROUTES}
    ws["direct"].nnet.params.copy_flat_(ws["graph"].nnet.params.flat)
    ws["direct"].gnn.params.copy_flat_(ws["graph"].gnn.params.flat)
    one = rng.integers(-1, 2, size=SHAPE).astype(np.int64)
    eight = rng.integers(-1, 2, size=(8,) + SHAPE).astype(np.int64)
    big = rng.integers(-1, 2, size=(2048,) + SHAPE).astype(np.int8)
    calls = {
        "predict_b1": lambda w: w.predict(one),
        "predict_with_gnn_b1": lambda w: w.predict_with_gnn(one),
        "predict_both_b1": lambda w: w.predict_both(one[None]),
        "predict_b8": lambda w: w.predict_batch(eight),
        "predict_with_gnn_b8": lambda w: w.predict_batch_with_gnn(eight),
        "predict_both_b8": lambda w: w.predict_both(eight),
    }
    for name, f in calls.items():
        res[name] = ab({k: (lambda w=w, f=f: f(w)) for k, w in ws.items()}, a.blocks, a.calls)
    res["lockstep_round_2048"] = ab({k: (lambda w=w: w.predict_both_async(big).result())
                                     for k, w in ws.items()}, a.blocks, max(10, a.calls // 10))
    # the same bits on both routes (checked here so a timing of wrong results cannot pass)
    os.environ["AZ_B1_MODE"] = "graph"
    g = ws["graph"].predict_both(eight)
    os.environ["AZ_B1_MODE"] = "direct"
    d = ws["direct"].predict_both(eight)
    res["both8_bit_identical"] = all(np.array_equal(x, y) for x, y in zip(g, d))
    res["trunk_device_us"] = trunk_times(ws["direct"], wrapper("direct", 1, (7, 7)), rng)
    os.environ.pop("AZ_B1_MODE", None)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
