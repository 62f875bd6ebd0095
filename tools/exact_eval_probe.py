"""What batch-invariant evaluation costs on the MI355X (config key batch_invariant).

    python tools/exact_eval_probe.py [--blocks 7] [--out FILE.json]

1. az_gemm_exact_f32 at M = 1, 8, 512, 2048, N = K = 3136 (output_transform's layers on the 7x7
   board): device time per call (events around back-to-back calls on uniform [-1, 1] operands),
   the rate 2 M N K / t as a fraction of the 157.3 TF f32 MFMA peak, and at M = 1 the HBM floor of
   the 39.3 MB of weights at 8 TB/s over the time.  az_gemm_f32 (the default dispatch) on the same
   operands beside it.
2. predict_both on the 7x7 board at B = 1, 8, 512, 2048, key on against key off: two wrappers
   with the same weights in one process, alternating blocks, host call to results in host memory;
   median over the blocks and their spread.
3. Self-play on the 7x7 board, 64 episodes at parallel_games 64 and 25 simulations, key on and
   key off, alternating, three runs each: episodes/s.
Prints one JSON document."""
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

PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12
F = 3136


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
    return float(np.median(xs)), (max(xs) - min(xs)) / float(np.median(xs))


def gemm_times():
    from azhip import ops
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    W = torch.from_numpy(rng.uniform(-1, 1, (F, F)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rng.uniform(-1, 1, F).astype(np.float32)).to(dev)
    out = {"plan_segments": ops.gemm_exact_plan(F, F)}
    for M in (1, 8, 512, 2048):
        A = torch.from_numpy(rng.uniform(-1, 1, (M, F)).astype(np.float32)).to(dev)
        C = torch.empty((M, F), device=dev)
        reps = 200 if M <= 8 else 30
        us, spread = device_us(lambda: ops.linear_exact(A, W, b, ops.ACT_RELU, out=C), reps)
        us0, spread0 = device_us(lambda: ops.linear(A, W, b, ops.ACT_RELU, out=C), reps)
        flops = 2.0 * M * F * F
        row = {"exact_us": round(us, 2), "exact_spread": round(spread, 4),
               "exact_tflops": round(flops / us * 1e-6, 2),
               "exact_fraction_of_f32_mfma_peak": round(flops / (us * 1e-6) / PEAK_F32_MFMA, 4),
               "default_dispatch_us": round(us0, 2), "default_spread": round(spread0, 4),
               "exact_over_default": round(us / us0, 2)}
        if M == 1:
            floor_us = 4.0 * F * F / PEAK_HBM * 1e6
            row["hbm_floor_us"] = round(floor_us, 2)
            row["exact_fraction_of_hbm_floor"] = round(floor_us / us, 4)
        out[str(M)] = row
    return out


def wrappers():
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Game import Connect4Game
    ws = {}
    for name, key in (("off", False), ("on", True)):
        torch.manual_seed(0)
        ws[name] = Connect4GNNWrapper(Connect4Game(7), SimpleNamespace(
            gnn_layers=2, dropout=0.3, batch_invariant=key))
    ws["on"].nnet.params.copy_flat_(ws["off"].nnet.params.flat)
    ws["on"].gnn.params.copy_flat_(ws["off"].gnn.params.flat)
    return ws


def ab(fns, blocks, calls):
    per = {r: [] for r in fns}
    for f in fns.values():
        for _ in range(max(5, calls // 4)):
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
        out[r] = {"us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 4)}
    out["on_over_off"] = round(out["on"]["us"] / out["off"]["us"], 2)
    return out


def predict_times(ws, blocks):
    rng = np.random.default_rng(1)
    out = {}
    worst = 0.0
    for B in (1, 8, 512, 2048):
        boards = rng.integers(-1, 2, size=(B, 7, 7)).astype(np.int8)
        a, b = ws["off"].predict_both(boards), ws["on"].predict_both(boards)
        worst = max(worst, max(float(np.abs(x - y).max()) for x, y in zip(a, b)))
        calls = 200 if B <= 8 else 20
        out[str(B)] = ab({k: (lambda w=w: w.predict_both(boards)) for k, w in ws.items()},
                         blocks, calls)
    out["max_abs_difference_on_vs_off"] = worst
    return out


def selfplay_times(ws):
    from selfplay import play_episodes_engine
    args = dict(numMCTSSims=25, cpuct=1.0, tempThreshold=15, use_gnn=True, expand_by=5)
    eps = list(range(64))
    per = {"off": [], "on": []}
    for rep in range(4):                       # the first pass warms both routes up
        for k, w in ws.items():
            a = dict(args, batch_invariant=(k == "on"))
            t0 = time.perf_counter()
            play_episodes_engine(w.game, w, a, eps, {e: e for e in eps}, parallel_games=64,
                                 lanes=2)
            if rep:
                per[k].append(64 / (time.perf_counter() - t0))
    out = {k: {"episodes_per_s": round(float(np.median(v)), 2),
               "runs": [round(x, 2) for x in v]} for k, v in per.items()}
    out["off_over_on"] = round(out["off"]["episodes_per_s"] / out["on"]["episodes_per_s"], 2)
    out["setting"] = "7x7, 64 episodes, parallel_games 64, 25 simulations, 2 lanes, seed = episode"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0),
           "peaks": {"f32_mfma_tflops": PEAK_F32_MFMA * 1e-12, "hbm_tb_s": PEAK_HBM * 1e-12}}
    res["gemm_3136"] = gemm_times()
    ws = wrappers()
    res["predict_both_7x7_us"] = predict_times(ws, a.blocks)
    res["selfplay_7x7"] = selfplay_times(ws)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
