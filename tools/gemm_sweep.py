"""GEMM tuning sweep on the GPU box: time az_gemm_f32 under the tuning build's overrides (each
variant in its own subprocess since the overrides are read once):
    tallk                    gemm_tall (default dispatch) vs the tile kernels on the GNN shapes
    x3 Ms tiles splits       gemm_x3 tile 1 (256x128) / 2 (128x128) and split-K vs the fp32 tiles"""
import json
import os
os.environ.setdefault("AZ_TUNING_LIB", "1")   # A/B switches live in the tuning build
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, json, torch
sys.path.insert(0, "%s/alphazero-gnn_amd")
from azhip import ops
M, N, K = %d, %d, %d
x = torch.rand((M, K), device="cuda") * 2 - 1
w = (torch.rand((N, K), device="cuda") * 2 - 1) / K ** 0.5
b = torch.rand((N,), device="cuda")
y = torch.empty((M, N), device="cuda")
for _ in range(5):
    ops.linear(x, w, b, act=1, out=y)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
reps = 50
e0.record()
for _ in range(reps):
    ops.linear(x, w, b, act=1, out=y)
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) / reps * 1e3
ref = torch.relu(x.double() @ w.double().T + b.double())
scale = x.double().abs() @ w.double().abs().T
err = float(((y.double() - ref).abs() / (scale + 1e-30)).max())
print(json.dumps({"us": us, "tflops": 2 * M * N * K / us / 1e6, "rel_err": err}))
'''


def run(env, M=512, N=3136, K=3136):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, M, N, K)], env=e,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return {"error": r.stderr[-300:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "tallk":        # gemm_tall (default dispatch) vs the tile kernels (AZ_GEMM_NOTALL)
        for (M, N, K) in [(524288, 256, 64), (524288, 64, 64), (524288, 64, 128),
                          (524288, 128, 64), (20007, 64, 64)]:
            for env in ({}, {"AZ_GEMM_NOTALL": "1"}, {"AZ_GEMM_ABLATE": "4"},
                        {"AZ_GEMM_ABLATE": "8"}):
                res = run(env, M, N, K)
                print(json.dumps({"M": M, "N": N, "K": K, "env": env, **res}), flush=True)
        sys.exit(0)
    if mode == "x3":           # fp32 on the bf16 matrix cores (gemm_x3) vs the fp32 MFMA tiles
        # argv: Ms  tiles  splits ("auto" = the dispatch's own choice)
        shapes = [tuple(int(v) for v in (x + ":3136:3136").split(":")[:3])
                  for x in sys.argv[2].split(",")]     # "M" or "M:N:K"
        tiles = sys.argv[3].split(",")
        splits = sys.argv[4].split(",")
        for (M, N, K) in shapes:
            print(json.dumps({"M": M, "N": N, "K": K, "x3": "off",
                              **run({"AZ_GEMM_X3": "0"}, M, N, K)}), flush=True)
            for t in tiles:
                for sp in splits:
                    env = {"AZ_GEMM_X3": t}
                    if sp != "auto":
                        env["AZ_GEMM_SPLITS"] = sp
                    print(json.dumps({"M": M, "N": N, "K": K, "x3": t, "splits": sp,
                                      **run(env, M, N, K)}), flush=True)
        sys.exit(0)
    sys.exit("usage: gemm_sweep.py tallk | x3 Ms tiles(1,2) splits")
