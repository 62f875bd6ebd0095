"""The GNN gradient on child stars, timed (features included, Adam excluded), the routes
alternating in one process:

  packed       train.gnn_star_grads (az_gnn_star_batch_fwd_train / az_gnn_star_batch_bwd)
  composition  the same stars through calls that predate the packed path: ops.gnn_layer(save=True)
               and ops.gnn_layer_bwd on the forest-of-stars DeviceGraph, then mlp2 / heads on the
               row 0s (a gather and a scatter of the row 0s by torch indexing)
  batch_star   train.gnn_grads on B = 64 boards (the reference's star over the batch), for scale

    python tools/star_train_probe.py [--blocks 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/star_train_probe.py --trace c4_7x7:64

Cases: 64 and 256 stars of 8 rows on Connect4 7x7, 64 stars of 5 rows on 4x4, 64 stars of 10 rows
on TicTacToe 3x3; two GNN layers; random boards (the time does not depend on the cells).  Every
figure is the median over `blocks` blocks of `calls` gradient computations, device synchronised
around a block; the spread is the blocks' (max - min) / median.  The two routes' gradients are
compared before anything is timed.  --trace CASE:STARS runs only 20 packed computations of that
case (for a kernel trace taken in a run of its own).  Prints one JSON document.
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

from azhip import ops, train as T  # noqa: E402

# case -> (game kind, board shape, rows per star)
CASES = {"c4_7x7": ("c4", (7, 7), 8), "c4_4x4": ("c4", (4, 4), 5), "ttt_3x3": ("ttt", (3, 3), 10)}
RUNS = (("c4_7x7", 64), ("c4_7x7", 256), ("c4_4x4", 64), ("ttt_3x3", 64))


def wrapper(case):
    kind, shape, _ = CASES[case]
    torch.manual_seed(0)
    if kind == "c4":
        from connect4.Connect4GNN import Connect4GNNWrapper
        from connect4.Connect4Game import Connect4Game
        return Connect4GNNWrapper(Connect4Game(shape[0]), SimpleNamespace(gnn_layers=2,
                                                                          dropout=0.3))
    from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    return TicTacToeGNNWrapper(TicTacToeGame(shape[0]), SimpleNamespace(gnn_layers=2))


def inputs(w, case, B, rng):
    _, shape, n = CASES[case]
    dev = w.device
    rows = torch.from_numpy(rng.integers(-1, 2, size=(B * n,) + shape).astype(np.int8)).to(dev)
    offs = (np.arange(B + 1) * n).astype(np.int32)
    rowptr = np.zeros(B * n + 1, np.int64)
    col = []
    for b in range(B):
        s = b * n
        rowptr[s] = b * (n - 1)
        rowptr[s + 1:s + n + 1] = (b + 1) * (n - 1)
        col += list(range(s + 1, s + n))
    graph = ops.DeviceGraph(rowptr, np.asarray(col, np.int64), dev)
    starts = torch.from_numpy(offs[:-1].astype(np.int64)).to(dev)
    tpi = torch.from_numpy(rng.dirichlet(np.ones(w.action_size), B).astype(np.float32)).to(dev)
    tv = torch.from_numpy(rng.uniform(-1, 1, B).astype(np.float32)).to(dev)
    return rows, torch.from_numpy(offs).to(dev), graph, starts, tpi, tv


def composition_grads(net, gnn, rows, graph, starts, tpi, tv, seed):
    """gnn_star_grads' result from the generic graph calls."""
    GG = T._grads(gnn)
    c4 = T._kind(net) == "c4"
    fw = T.C4Forward(net, rows, net.dropout, seed) if c4 else T.TTTForward(net, rows)
    x = fw.s.contiguous()
    xs, wss = [x], []
    for layer in gnn.layers:
        x, ws = ops.gnn_layer(graph, x, layer.weights())
        xs.append(x)
        wss.append(ws)
    r0 = xs[-1][starts].contiguous()
    Wg = gnn.params.views
    y, hidden = ops.mlp2(r0, Wg["output_transform.0.weight"], Wg["output_transform.0.bias"],
                         Wg["output_transform.2.weight"], Wg["output_transform.2.bias"])
    logp, v, saved = (T.c4_heads_fwd if c4 else T.ttt_heads_fwd)(net, y)
    lrows = torch.empty((starts.numel(), 2), device=rows.device)
    dl, dv = ops.heads_loss_bwd(logp, v, tpi, tv, loss_rows=lrows)
    dy = (T.c4_heads_bwd if c4 else T.ttt_heads_bwd)(net, y, dl, dv, saved, None)
    d0 = ops.mlp2_bwd(r0, Wg["output_transform.0.weight"], Wg["output_transform.2.weight"], hidden,
                      dy, {"w0": GG["output_transform.0.weight"],
                           "b0": GG["output_transform.0.bias"],
                           "w2": GG["output_transform.2.weight"],
                           "b2": GG["output_transform.2.bias"]})
    dx = torch.zeros_like(xs[-1])
    dx[starts] = d0
    for li in range(len(gnn.layers) - 1, -1, -1):
        layer = gnn.layers[li]
        grads = {k[len(layer.prefix):]: g for k, g in GG.items() if k.startswith(layer.prefix)}
        dx = ops.gnn_layer_bwd(graph, xs[li], layer.weights(), wss[li], dx, grads)
    return lrows.sum(0)


def ab(fns, blocks, calls):
    per = {r: [] for r in fns}
    for f in fns.values():
        for _ in range(3):
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
    return out


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
    ap.add_argument("--trace", default=None, help="CASE:STARS, e.g. c4_7x7:64")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    if a.trace:
        case, B = a.trace.split(":")
        w = wrapper(case)
        w.nnet.train()
        w.gnn.train()
        rows, offs, _, _, tpi, tv = inputs(w, case, int(B), rng)
        for _ in range(20):
            T.gnn_star_grads(w.nnet, w.gnn, rows, offs, tpi, tv, seed=1)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "gnn_layers": 2,
           "unit": "us per GNN gradient computation (features .. every gradient), device time "
                   "between two synchronisations / calls"}
    wrappers = {}
    for case, B in RUNS:
        w = wrappers.get(case) or wrappers.setdefault(case, wrapper(case))
        w.nnet.train()
        w.gnn.train()
        net, gnn = w.nnet, w.gnn
        rows, offs, graph, starts, tpi, tv = inputs(w, case, B, rng)
        fns = {"packed": lambda: T.gnn_star_grads(net, gnn, rows, offs, tpi, tv, seed=1),
               "composition": lambda: composition_grads(net, gnn, rows, graph, starts, tpi, tv, 1)}
        if B == 64:
            boards = rows[:64].contiguous()
            fns["batch_star"] = lambda: T.gnn_grads(net, gnn, boards, tpi, tv, seed=1)
        # the two routes computed the same thing (a timing of wrong results cannot pass)
        lp = fns["packed"]().cpu().numpy()
        gp = gnn.params.grad_flat.clone()
        lc = fns["composition"]().cpu().numpy()
        gc = gnn.params.grad_flat
        scale = float(gc.abs().max())
        diff = float((gp - gc).abs().max())
        r = ab(fns, a.blocks, 5)
        r["stars"], r["rows_per_star"] = B, CASES[case][2]
        r["max_abs_grad_diff"], r["max_abs_grad"] = diff, scale
        r["loss_packed"], r["loss_composition"] = lp.tolist(), lc.tolist()
        p, c = r["packed"], r["composition"]
        r["composition_over_packed"] = round(c["us"] / p["us"], 3)
        bar = max(p["spread"], c["spread"])
        r["verdict"] = ("packed faster" if c["us"] > p["us"] * (1 + bar) else
                        "packed slower" if p["us"] > c["us"] * (1 + bar) else "within the spread")
        res[f"{case}/B{B}"] = r
        print(case, B, {k: r[k]["us"] for k in fns}, r["verdict"], diff, scale, file=sys.stderr,
              flush=True)
    emit(res, a.out)


if __name__ == "__main__":
    main()
