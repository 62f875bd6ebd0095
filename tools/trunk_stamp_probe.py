"""Probe: where a Connect4 trunk block's time goes.  libaz_hip_stamps.so = az_trunk.hip built
with -DAZ_TUNING -DAZ_TRUNK_STAMPS (linked with the tuning objects): lane 0 of every wave stamps
s_memrealtime (100 MHz) at the body's start, when the prologue's loads have landed, after conv2's
in-kernel weight split (unregistered weights only), after conv1's arithmetic, when conv1's planes
are stored, after conv2, when the rows are staged and when the rows / A planes are written.
Runs ops.c4_gnn_eval at B (registered weights: c4_trunk_split_a_kernel) and prints per-phase
medians over blocks and waves, and the spread of block start and end times.
    AZ_AB_LIB=libaz_hip_stamps.so python tools/trunk_stamp_probe.py [B] > phases.json"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-gnn_amd"))

PHASES = ["loads_landed", "weight_split", "conv1_arith", "c1_planes_in_lds", "conv2", "rows_staged",
          "rows_planes_written"]


def main():
    from azhip import ops, _lib
    from azhip.nets import C4Evaluator
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    L = _lib.load()
    ev = C4Evaluator(synthetic_state_dict(connect4_net_spec(7), 1),
                     synthetic_state_dict(gnn_spec(3136, 2), 2), device=torch.device("cuda"))
    W, G = ev.nnet.params, ev.gnn.params
    boards = torch.from_numpy(
        np.random.default_rng(0).integers(-1, 2, (B, 7, 7)).astype(np.int8)).cuda()
    for _ in range(50):
        ops.c4_gnn_eval(boards, W, G)
    blocks, NW, SL = B, 8, 8
    buf = torch.zeros(blocks * NW * SL, dtype=torch.int64, device="cuda")
    L.az_debug_trunk_stamps.argtypes = [ctypes.c_void_p]
    reps = []
    for _ in range(5):
        buf.zero_()
        assert L.az_debug_trunk_stamps(ctypes.c_void_p(buf.data_ptr())) == 0
        ops.c4_gnn_eval(boards, W, G)
        torch.cuda.synchronize()
        assert L.az_debug_trunk_stamps(ctypes.c_void_p(0)) == 0
        for _ in range(5):
            ops.c4_gnn_eval(boards, W, G)
        torch.cuda.synchronize()
        reps.append(buf.cpu().numpy().reshape(blocks, NW, SL).copy())
    med = lambda v: round(float(np.median(v)), 1)   # noqa: E731
    out = []
    for a in reps:
        used = a[:, :, 0] > 0                        # (block, wave) pairs that ran
        s = a.astype(np.float64) * 10.0              # 100 MHz ticks -> ns
        t0 = s[:, :, 0][used].min()
        ph = {}
        prev = s[:, :, 0]
        for k, name in enumerate(PHASES, start=1):
            ok = used & (a[:, :, k] > 0)
            if not ok.any():
                ph[name + "_ns"] = None              # point not in this build's path
                continue
            ph[name + "_ns"] = med((s[:, :, k] - prev)[ok])
            prev = np.where(ok, s[:, :, k], prev)
        end = s[:, :, 7]
        out.append({"B": B, "blocks": int(used.any(1).sum()), "waves_per_block": int(used[0].sum()),
                    "phases": ph, "block_ns": med((end - s[:, :, 0])[used]),
                    "block_start_ns": {"min": med((s[:, :, 0] - t0)[used].min()),
                                       "median": med((s[:, :, 0] - t0)[used]),
                                       "max": med((s[:, :, 0] - t0)[used].max())},
                    "kernel_span_ns": med((end - t0)[used].max())})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
