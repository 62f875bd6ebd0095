"""The fused split-K reduce + composed heads launch (csrc/az_trunk.hip splitk_act_heads_kernel):
az_transform_heads_fwd with y NULL, A <= 8 and B > 64 sums output_transform.0's split-K slabs,
adds the bias, applies the ReLU and runs the heads composed with output_transform.2 on the rows
while they are in registers (gnn_utils.py:115, Connect4GNN.py:48-57).  The kernel it replaced,
splitk_act_heads_rowsw_kernel, stays in the tuning library under AZ_SPLITK_HEADS_MODE=old and is
the bit reference here; each switch is read once per process, so each side runs in a child
process of its own (this file run as a script) on the same seeded problems.

Problems: test_gpu_composed_heads.py's distribution.  F = 3136 with B in {65, 257, 300, 512, 513,
768} and A in {8, 7, 1}; F = 288 (A = 7, B = 65), whose last 256-column chunk is partial (32
columns), and F = 544 (A = 7, B = 65), three chunks with a partial last one.  On a 256-CU device
they reach the kernel with 8, 5, 5, 5, 3, 3 slabs at F = 3136 (one row per block up to 256 rows,
two above), 2 at F = 288 and 4 at F = 544.  The product dispatch takes the stream-K form for
B = 513 and 768 (no slabs); the children run with AZ_CSK=off, which keeps the split-K tiles
there, so the 256 x 128 tile's second split count reaches the kernel too.  The split
count of every call is printed by the library (AZ_SPLITK_HEADS_PRINT) and shown by the test."""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = (65, 257, 300, 512, 513, 768)
CASES = [(3136, A, B) for A in (8, 7, 1) for B in BS] + [(288, 7, 65), (544, 7, 65)]
EV_BS = (65, 257, 300, 512, 513)   # evaluator batches (hidden rows not requested)


def _rand(g, shape, lo, hi):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


_CPU = {}


def _cpu(kind, *key):
    """Seeded CPU tensors, made once per process: ("w", F) -> (w0, b0, w2, b2), ("h", F, A) ->
    (wp, bp, wv, bv), ("x", F, B) -> x."""
    k = (kind,) + key
    if k not in _CPU:
        F = key[0]
        s = F ** -0.5
        if kind == "w":
            g = torch.Generator().manual_seed(7 * F)
            _CPU[k] = (_rand(g, (F, F), -s, s), _rand(g, (F,), -0.05, 0.05),
                       _rand(g, (F, F), -s, s), _rand(g, (F,), -0.05, 0.05))
        elif kind == "h":
            A = key[1]
            g = torch.Generator().manual_seed(11 * F + A)
            _CPU[k] = (_rand(g, (A, F), -s, s), _rand(g, (A,), -0.5, 0.5),
                       _rand(g, (1, F), -s, s), _rand(g, (1,), -0.5, 0.5))
        else:
            g = torch.Generator().manual_seed(13 * F + key[1])
            _CPU[k] = _rand(g, (key[1], F), -1.0, 1.0)
    return _CPU[k]


_DEV = {}


def _dev(kind, *key):
    k = (kind,) + key
    if k not in _DEV:
        t = _cpu(kind, *key)
        _DEV[k] = t.cuda() if kind == "x" else tuple(u.cuda() for u in t)
    return _DEV[k]


def _args(F, A, B):
    w0, b0, w2, b2 = _dev("w", F)
    wp, bp, wv, bv = _dev("h", F, A)
    return _dev("x", F, B), w0, b0, w2, b2, wp, bp, wv, bv


def _boards(B):
    rng = np.random.default_rng(B)
    return torch.from_numpy(rng.integers(-1, 2, size=(B, 7, 7)).astype(np.int8)).cuda()


def _evaluator():
    from azhip.nets import C4Evaluator
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    return C4Evaluator(synthetic_state_dict(connect4_net_spec(7), 1),
                       synthetic_state_dict(gnn_spec(3136, 2), 2), device=torch.device("cuda"))


def _child(out_path):
    """Every case through az_transform_heads_fwd (y NULL, hidden rows requested: the C entry
    always hands them back) with output_transform's weights registered, and the evaluator's
    batches (hidden rows not requested) through az_c4_eval_fwd."""
    sys.path.insert(0, os.path.join(ROOT, "alphazero-gnn_amd"))
    from azhip import _lib, ops
    out = {}
    for F in sorted({c[0] for c in CASES}):
        for t in (_dev("w", F)[0], _dev("w", F)[2]):
            _lib.check(_lib.load().az_weights_register(t.data_ptr(), t.numel() * 4), "register")
    for F, A, B in CASES:
        logp, pi, v, _, _ = ops.transform_heads(*_args(F, A, B), want_y=False)
        for k, t in (("logp", logp), ("pi", pi), ("v", v)):
            out[f"{k}_{F}_{A}_{B}"] = t.cpu().numpy()
    ev = _evaluator()
    for B in EV_BS:
        logp, pi, v = ops.c4_gnn_eval(_boards(B), ev.nnet.params, ev.gnn.params)
        for k, t in (("logp", logp), ("pi", pi), ("v", v)):
            out[f"ev_{k}_{B}"] = t.cpu().numpy()
    np.savez(out_path, **out)
    print("ok")


def _run(tmp, name, env_extra, tuning=True):
    env = dict(os.environ)
    for k in ("AZ_TUNING_LIB", "AZ_SPLITK_HEADS_MODE", "AZ_SPLITK_HEADS_R", "AZ_CSK",
              "AZ_SPLITK_HEADS_PRINT"):
        env.pop(k, None)
    if tuning:
        env["AZ_TUNING_LIB"] = "1"
    env.update(env_extra)
    path = str(tmp / f"{name}.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env,
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    splits = [tuple(int(x) for x in m) for m in
              re.findall(r"splitk_act_heads B=(\d+) F=(\d+) A=(\d+) S=(\d+) h=(\d)", r.stderr)]
    return dict(np.load(path)), splits


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    """(new, old, product, the new side's (B, F, A, S, h) lines): the three libraries' results on
    the same problems, computed once."""
    tmp = tmp_path_factory.mktemp("reduce_heads")
    keep = {"AZ_CSK": "off", "AZ_SPLITK_HEADS_PRINT": "1"}
    new, splits = _run(tmp, "new", keep)
    old, splits_old = _run(tmp, "old", dict(keep, AZ_SPLITK_HEADS_MODE="old"))
    assert splits == splits_old
    prod, _ = _run(tmp, "product", {}, tuning=False)
    return new, old, prod, splits


@pytest.mark.timeout(600)
def test_new_kernel_equals_the_old_one_bitwise(sides):
    """log pi, pi and v of every case, and of the evaluator's batches, are the same bits from
    splitk_act_heads_kernel (tuning library's default) and from splitk_act_heads_rowsw_kernel
    (AZ_SPLITK_HEADS_MODE=old); the cases reach the kernel with at least two different split
    counts, both with and without the hidden rows' store."""
    new, old, _, splits = sides
    for B, F, A, S, h in splits:
        print(f"reduce+heads call: B={B} F={F} A={A} S={S} hidden_rows={h}")
    assert len({s[3] for s in splits if s[3] > 1}) >= 2, splits
    assert {s[4] for s in splits} == {0, 1}, splits
    took = {(s[1], s[2], s[0]) for s in splits if s[4] == 1}
    assert took >= set(CASES), sorted(set(CASES) - took)
    assert sorted(new) == sorted(old)
    for k, a in new.items():
        assert np.array_equal(a, old[k]), f"{k} differs from the old kernel"


def test_product_library_equals_the_tuning_default(sides):
    """The product library (no switches; stream-K instead of split-K tiles at B = 513 and 768)
    gives the tuning library's bits wherever both take the same GEMM form."""
    new, _, prod, _ = sides
    for k, a in new.items():
        if k.endswith(("_513", "_768")):
            continue
        assert np.array_equal(a, prod[k]), f"product library: {k} differs"


@pytest.fixture(scope="module")
def ops():
    from azhip import ops as o
    return o


@contextlib.contextmanager
def registered(tensors):
    from azhip import _lib
    L = _lib.load()
    done = []
    try:
        for t in tensors:
            _lib.check(L.az_weights_register(t.data_ptr(), t.numel() * 4), "az_weights_register")
            done.append(t)
        yield
    finally:
        for t in done:
            _lib.check(L.az_weights_unregister(t.data_ptr()), "az_weights_unregister")


@pytest.mark.parametrize("F,A,B", CASES)
def test_requested_hidden_rows(ops, F, A, B):
    """The hidden rows az_transform_heads_fwd hands back equal ops.linear(..., act=ACT_RELU)
    bitwise (the reduce's arithmetic is splitk_reduce's)."""
    a = _args(F, A, B)
    _, _, _, _, hid = ops.transform_heads(*a, want_y=False)
    want = ops.linear(a[0], a[1], a[2], act=ops.ACT_RELU)
    torch.cuda.synchronize()
    assert torch.equal(hid, want)


@pytest.mark.parametrize("B", EV_BS)
def test_heads_do_not_depend_on_the_hidden_rows_store(ops, B):
    """The evaluator never asks for the hidden rows (its scratch stays NaN: the kernel's form
    without the store); az_transform_heads_fwd on the same feature rows and weights always does.
    The heads are the same bits."""
    ev = _evaluator()
    Wn, Gn = ev.nnet.params, ev.gnn.params
    boards = _boards(B)
    hidden = torch.full((B, 3136), float("nan"), device="cuda")
    logp, pi, v = ops.c4_gnn_eval(boards, Wn, Gn, hidden=hidden)
    tl, tp, tv, _, th = ops.transform_heads(
        ops.c4_trunk(boards, Wn), Gn["output_transform.0.weight"], Gn["output_transform.0.bias"],
        Gn["output_transform.2.weight"], Gn["output_transform.2.bias"], Wn["fc_policy.weight"],
        Wn["fc_policy.bias"], Wn["fc_value.weight"], Wn["fc_value.bias"], want_y=False)
    torch.cuda.synchronize()
    assert torch.equal(logp, tl) and torch.equal(pi, tp) and torch.equal(v, tv)
    if B <= 512:   # split-K slabs: the fused kernel, which leaves the evaluator's rows alone
        assert bool(torch.isnan(hidden).all())
    assert not bool(torch.isnan(th).any())


_Y64 = {}


def _y64(F, B):
    """float64 output_transform of the float64 hidden rows (shared by the A cases)."""
    if (F, B) not in _Y64:
        w0, b0, w2, b2 = (t.double() for t in _cpu("w", F))
        hid = torch.relu(_cpu("x", F, B).double() @ w0.T + b0)
        _Y64[(F, B)] = hid @ w2.T + b2
    return _Y64[(F, B)]


@pytest.mark.parametrize("F,A,B", CASES)
def test_float64_parity(ops, F, A, B):
    """log pi, pi and v within 1e-6 of the float64 heads of the float64 hidden rows
    (test_gpu_composed_heads.py's bar, which holds the fp16-form GEMM of output_transform.0 as
    well as the composed heads)."""
    from conftest import assert_close
    wp, bp, wv, bv = (t.double() for t in _cpu("h", F, A))
    y = _y64(F, B)
    lg = y @ wp.T + bp
    lp64 = (lg - torch.logsumexp(lg, 1, keepdim=True)).numpy()
    v64 = torch.tanh(y @ wv.T + bv).flatten().numpy()
    logp, pi, v, _, _ = ops.transform_heads(*_args(F, A, B), want_y=False)
    tag = f"reduce_heads/F{F}_A{A}_B{B}"
    for name, got, ref in (("logp", logp, lp64), ("pi", pi, np.exp(lp64)), ("v", v, v64)):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print(f"{tag}/{name}: max err {err:.3g}, margin {1e-6 / err if err else float('inf'):.2f}x")
    assert_close(f"{tag}/logp_vs_fp64", logp.cpu().numpy(), lp64, 1e-6)
    assert_close(f"{tag}/pi_vs_fp64", pi.cpu().numpy(), np.exp(lp64), 1e-6)
    assert_close(f"{tag}/v_vs_fp64", v.cpu().numpy(), v64, 1e-6)


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_one_workspace_reused(ops, fill):
    """B = 512, 65, 512, 300 back to back on one workspace and stream: each result equals the
    same call on a fresh workspace -- also when the workspace held NaN bit patterns (0xFF bytes)
    before the first call: no stale partial, no read of bytes nobody wrote."""
    from azhip import _lib
    F, A = 3136, 8
    nbytes = max(max(int(_lib.lib().az_transform_heads_ws_bytes(B, F, A)) for B in (512, 300, 65)),
                 96 << 20)
    dev = torch.device("cuda")
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    got = []
    with ops.pinned_workspace(dev, ws):
        for B in (512, 65, 512, 300):
            got.append([t.clone() for t in ops.transform_heads(*_args(F, A, B), want_y=False)[:3]])
    for B, g in zip((512, 65, 512, 300), got):
        fresh = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
        with ops.pinned_workspace(dev, fresh):
            want = ops.transform_heads(*_args(F, A, B), want_y=False)[:3]
            torch.cuda.synchronize()
        for a, b in zip(g, want):
            assert torch.equal(a, b), f"B={B}: differs from the fresh-workspace call"
        del fresh


def test_registered_weights_give_the_same_bits(ops):
    """Registered weights (cached planes and composed rows) and unregistered clones (split and
    composed per call): equal bits."""
    a = _args(3136, 7, 300)
    want = ops.transform_heads(*a, want_y=False)
    reg = [t.clone() for t in a[1:]]
    with registered(reg):
        got = ops.transform_heads(a[0], *reg, want_y=False)
        torch.cuda.synchronize()
    for x, y in zip((got[0], got[1], got[2], got[4]), (want[0], want[1], want[2], want[4])):
        assert torch.equal(x, y)


if __name__ == "__main__":
    _child(sys.argv[1])
