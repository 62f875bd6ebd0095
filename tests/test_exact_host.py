"""Batch-invariant evaluation on the CPU: the K cut az_gemm_exact_plan reports, the host-side
argument checks of az_gemm_exact_f32 / az_eval_exact_fwd, the key's way through main.py, Coach and
the wrappers, and the CPU restatement of the arithmetic contract (tests/exact_ref.py) against exact
rational arithmetic."""
import ctypes
import inspect
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import exact_ref

AZ_OK, AZ_EINVAL = 0, -1
PLAN_SHAPES = [(16, 4), (132, 260), (512, 1152), (1024, 1024), (3136, 3136)]


class Args(SimpleNamespace):
    def __getitem__(self, k):
        return getattr(self, k)

    def get(self, k, default=None):
        return getattr(self, k, default)


def _on_own_thread(fn):
    """az_last_error is per thread: calls that are rejected on purpose run on a thread of their
    own, so the main thread keeps the empty message tests/test_lib_abi.py expects whatever the
    test order."""
    import functools
    import threading

    @functools.wraps(fn)
    def wrapper(*a, **k):
        failure = []

        def run():
            try:
                fn(*a, **k)
            except BaseException as ex:   # reported on the test's own thread
                failure.append(ex)

        t = threading.Thread(target=run)
        t.start()
        t.join()
        if failure:
            raise failure[0]
    return wrapper


@pytest.fixture(scope="module")
def L():
    from azhip.build import build
    build(verbose=False)
    from azhip import _lib
    return _lib.load()


# ------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("N,K", PLAN_SHAPES)
def test_plan_segments_are_contiguous_and_cover_k(L, N, K):
    from azhip import _lib, ops
    seg = ops.gemm_exact_plan(N, K)
    assert 1 <= len(seg) <= _lib.EXACT_MAX_SEGMENTS
    assert all(s > 0 for s in seg) and sum(seg) == K       # ascending cut points that end at K
    assert all(s % 4 == 0 for s in seg)
    assert seg == ops.gemm_exact_plan(N, K)                 # a pure function


@_on_own_thread
def test_plan_takes_no_m(L):
    """The cut is a function of (N, K): the C entry point and its bindings have no M to read."""
    from azhip import _lib, ops
    assert list(inspect.signature(ops.gemm_exact_plan).parameters) == ["N", "K"]
    res, argtypes = _lib.SIGNATURES["az_gemm_exact_plan"]
    assert len(argtypes) == 4                               # N, K, int* segments, int* seg_len
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "az_hip.h")).read()
    assert "int az_gemm_exact_plan(int N, int K, int* segments, int* seg_len);" in hdr
    n, seg = ctypes.c_int(0), (ctypes.c_int * 16)()
    assert L.az_gemm_exact_plan(6, 8, ctypes.byref(n), seg) == AZ_EINVAL      # N % 4
    assert L.az_gemm_exact_plan(8, 8, None, seg) == AZ_EINVAL and b"null" in L.az_last_error()
    # one row must still spread over the machine: the big layers are cut into several segments
    assert len(ops.gemm_exact_plan(3136, 3136)) > 1 and len(ops.gemm_exact_plan(16, 4)) == 1


# ------------------------------------------------------------------ 2. host-side validation
@_on_own_thread
def test_gemm_host_side_validation_without_gpu(L):
    """Like test_lib_abi.py::test_host_side_validation_without_gpu: bad arguments return AZ_EINVAL
    with a message before any HIP call, M = 0 is a no-op."""
    P = ctypes.c_void_p
    x = P(0x1000)                                            # never dereferenced: rejected first

    def call(M, N, K, A=x, W=x, C=x, ws=None, ws_bytes=0):
        return L.az_gemm_exact_f32(A, K, W, K, None, 0, C, N, M, N, K, ws, ws_bytes, None)

    assert call(0, 16, 4, A=None, W=None, C=None) == AZ_OK
    assert call(3, 18, 4) == AZ_EINVAL and b"N % 4" in L.az_last_error()
    assert call(3, 16, 6) == AZ_EINVAL and b"K % 4" in L.az_last_error()
    assert call(3, 16, 4, W=None) == AZ_EINVAL and b"null" in L.az_last_error()
    assert L.az_gemm_exact_f32(x, 4, x, 4, None, 3, x, 16, 3, 16, 4, None, 0, None) == AZ_EINVAL
    assert b"act" in L.az_last_error()                       # AZ_ACT_TANH is not offered
    need = L.az_gemm_exact_ws_bytes(3, 3136, 3136)
    assert need == len(exact_ref.plan(3136, 3136)) * 3 * 3136 * 4
    assert call(3, 3136, 3136, ws=None) == AZ_EINVAL and b"workspace" in L.az_last_error()
    assert call(3, 3136, 3136, ws=x, ws_bytes=need - 1) == AZ_EINVAL
    assert b"workspace" in L.az_last_error()
    assert L.az_gemm_exact_ws_bytes(3, 18, 4) == 0           # a rejected shape


def _eval_desc(_lib, game, nx, ny, A, max_B, fake=0x1000):
    F = 128 * (nx - 2) * (ny - 2) if game == _lib.EXACT_TTT else 64 * nx * ny
    d = _lib.EvalExact()
    d.game, d.nx, d.ny, d.A, d.F, d.max_B = game, nx, ny, A, F, max_B
    for name, _ in _lib.EvalExact._fields_:
        if name.endswith(("_w", "_b")) or name in ("feat", "h1", "h2", "hidden", "y", "logp",
                                                   "glogp", "ws"):
            setattr(d, name, fake)
    d.ws_bytes = 1 << 40
    return d


@_on_own_thread
def test_eval_host_side_validation_without_gpu(L):
    from azhip import _lib
    x = ctypes.c_void_p(0x1000)
    d = _eval_desc(_lib, _lib.EXACT_C4, 7, 7, 7, 4)

    def call(d, B, boards=x, v=x, gv=x):
        return L.az_eval_exact_fwd(ctypes.byref(d), boards, B, x, v, x, gv, None)

    assert call(d, 0, boards=None) == AZ_OK
    assert call(d, 5) == AZ_EINVAL and b"max_B" in L.az_last_error()
    assert L.az_eval_exact_fwd(None, x, 1, x, x, x, x, None) == AZ_EINVAL
    assert call(d, 1, boards=None) == AZ_EINVAL and b"null" in L.az_last_error()
    assert call(d, 1, v=None, gv=None) == AZ_EINVAL and b"neither" in L.az_last_error()
    d.ot0_w = None
    assert call(d, 1) == AZ_EINVAL and b"null" in L.az_last_error()
    d = _eval_desc(_lib, _lib.EXACT_C4, 7, 7, 7, 4)
    d.ws_bytes = L.az_eval_exact_ws_bytes(4, _lib.EXACT_C4, 7, 7, 7) - 1
    assert call(d, 1) == AZ_EINVAL and b"workspace" in L.az_last_error()
    d = _eval_desc(_lib, _lib.EXACT_C4, 7, 7, 40, 4)                 # A > 32
    assert call(d, 1) == AZ_EINVAL and b"A=40" in L.az_last_error()
    d = _eval_desc(_lib, _lib.EXACT_C4, 9, 9, 9, 4)                  # no fused trunk
    assert call(d, 1) == AZ_EINVAL and b"fused trunk" in L.az_last_error()
    d = _eval_desc(_lib, _lib.EXACT_TTT, 4, 4, 17, 4)
    d.fc1_w = None
    assert call(d, 1) == AZ_EINVAL and b"null" in L.az_last_error()
    assert L.az_eval_exact_ws_bytes(4, _lib.EXACT_C4, 9, 9, 9) == 0
    assert L.az_eval_exact_ws_bytes(4, _lib.EXACT_TTT, 6, 6, 37) == 0
    for game, nx, ny in ((_lib.EXACT_C4, 7, 7), (_lib.EXACT_C4, 4, 4), (_lib.EXACT_C4, 8, 7),
                         (_lib.EXACT_TTT, 3, 3), (_lib.EXACT_TTT, 5, 5)):
        assert L.az_eval_exact_ws_bytes(4096, game, nx, ny, 8) > 0


def test_eval_struct_layout_matches_header(L, tmp_path):
    """The ctypes mirror of az_eval_exact against what a C compiler makes of include/az_hip.h
    (test_lib_abi.py::test_struct_layouts_match_header's probe)."""
    import shutil
    import subprocess
    from azhip import _lib
    from conftest import ROOT
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    hdr = os.path.join(ROOT, "include", "az_hip.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', "int main(){",
             'printf("size %zu\\n", sizeof(az_eval_exact));']
    for f, _ in _lib.EvalExact._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(az_eval_exact, {f}));')
    lines.append('printf("maxseg %d\\n", AZ_EXACT_MAX_SEGMENTS);')
    lines.append('printf("games %d\\n", AZ_EXACT_C4 * 10 + AZ_EXACT_TTT);')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run([cc, str(src), "-o", str(tmp_path / "probe")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "probe")], capture_output=True,
                                                 text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.EvalExact)
    for f, _ in _lib.EvalExact._fields_:
        assert int(got[f]) == getattr(_lib.EvalExact, f).offset, f
    assert int(got["maxseg"]) == _lib.EXACT_MAX_SEGMENTS
    assert int(got["games"]) == _lib.EXACT_C4 * 10 + _lib.EXACT_TTT


# ------------------------------------------------------------------ 3. the key
def test_main_carries_the_key(tmp_path):
    import main
    import yaml
    cfg = tmp_path / "config.yaml"
    doc = {"game": {"board_size": 7}, "training": {"checkpoint_path": str(tmp_path / "ck")},
           "neural_network": {"use_gnn": True}}
    cfg.write_text(yaml.safe_dump(doc))
    base = ["--game", "connect4", "--use_gnn", "--config", str(cfg)]
    assert main.parse(base).batch_invariant is None
    assert not main.build_args(main.parse(base)).get("batch_invariant", False)
    assert main.build_args(main.parse(base + ["--batch_invariant"])).batch_invariant is True
    doc["selfplay"] = {"batch_invariant": True}
    cfg.write_text(yaml.safe_dump(doc))
    assert main.build_args(main.parse(base)).batch_invariant is True
    for name in ("connect4", "tictactoe", "frozenlake"):     # the shipped configs name the key, off
        shipped = main.config_to_args(main.load_config(os.path.join(main.HERE, name,
                                                                    "config.yaml")))
        assert shipped.batch_invariant is False
    assert "--batch_invariant" in main.__doc__


def test_coach_rejects_the_key_with_gnn_neighbors():
    import Coach as C
    from connect4.Connect4Game import Connect4Game
    from test_star_lockstep import StarHashNet
    from azhip.build import build_host
    build_host(verbose=False)
    game = Connect4Game(4)
    base = dict(numEps=1, numMCTSSims=2, cpuct=1.0, tempThreshold=2, use_gnn=True, expand_by=1)
    for extra in (dict(gnn_neighbors=True),
                  dict(gnn_neighbors=True, gnn_neighbors_lockstep=True, parallel_games=4)):
        with pytest.raises(ValueError, match="batch_invariant.*gnn_neighbors"):
            C.Coach(game, StarHashNet(game), Args(batch_invariant=True, **base, **extra))
        assert C.Coach(game, StarHashNet(game), Args(**base, **extra))      # the key off: as before
    assert C.Coach(game, StarHashNet(game), Args(batch_invariant=True, **base))


def test_arena_player_keeps_its_speculative_batch_at_8():
    """batch_invariant_rows is 1 << 30 under the key; the arena's speculative buffer stays 8."""
    import mcts_native
    from connect4.Connect4Game import Connect4Game
    from azhip.build import build_host
    build_host(verbose=False)
    game = Connect4Game(4)
    for rows, want in ((1 << 30, 8), (8, 8), (5, 5), (0, 0)):
        net = SimpleNamespace(batch_invariant_rows=rows)
        p = mcts_native.ArenaPlayer(game, net, Args(numMCTSSims=2, cpuct=1.0, use_gnn=True))
        assert p.spec == want


# ------------------------------------------------------------------ 4. the CPU restatement
def _need_ref():
    if exact_ref.lib() is None:
        pytest.skip("no C++ compiler")


def test_fma32_is_correctly_rounded():
    """The helper's std::fmaf against exact rational arithmetic: random triples, and products that
    land exactly half way between two floats (where a second rounding would show)."""
    _need_ref()
    rng = np.random.default_rng(7)
    f32 = np.float32
    triples = [(f32(a), f32(b), f32(c)) for a, b, c in rng.uniform(-1, 1, (40, 3))]
    triples += [(f32(a), f32(b), f32(c) * f32(2.0) ** int(e)) for (a, b, c), e in
                zip(rng.uniform(-1, 1, (16, 3)), rng.integers(-30, 30, 16))]
    one = f32(1.0)
    for k in (12, 11, 7):                      # (1 + 2^-k)^2 = 1 + 2^(1-k) + 2^(-2k)
        a = one + f32(2.0) ** -k
        triples += [(a, a, f32(0.0)), (a, a, f32(2.0) ** -24), (a, -a, f32(2.0) ** -24),
                    (a, a, -(f32(2.0) ** -(2 * k)) / f32(2.0))]
    # ties: 1 + 2^-24 exactly (to even: 1), 1 + 3 * 2^-24 (to even: 1 + 2^-22)
    triples += [(f32(2.0) ** -12, f32(2.0) ** -12, one),
                (f32(3.0) * f32(2.0) ** -12, f32(2.0) ** -12, one),
                (f32(2.0) ** -12, -(f32(2.0) ** -13), one),
                (f32(2.0) ** -100, f32(2.0) ** -49, f32(0.0)),          # subnormal result
                (f32(2.0) ** -100, f32(2.0) ** -50, f32(0.0))]          # half the smallest: 0
    ties = 0
    for a, b, c in triples:
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        want, tie = exact_ref.round_f32(exact, with_tie=True)
        got = exact_ref.fma32(a, b, c)
        assert got == want, (a, b, c, got, want)
        ties += tie
    assert ties >= 3                                        # the constructed ties are ties


def test_reference_chain_small_cases():
    """exact_ref.linear on shapes small enough to restate with fma32 call by call."""
    _need_ref()
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (3, 12)).astype(np.float32)
    w = rng.uniform(-1, 1, (4, 12)).astype(np.float32)
    b = rng.uniform(-1, 1, 4).astype(np.float32)
    seg = [8, 4]
    got = exact_ref.linear(x, w, b, relu=True, segments=seg)
    for i in range(3):
        for j in range(4):
            sums, k = [], 0
            for n in seg:
                acc = np.float32(0.0)
                for kk in range(k, k + n):
                    acc = exact_ref.fma32(x[i, kk], w[j, kk], acc)
                sums.append(acc)
                k += n
            t = np.float32(np.float32(sums[0] + sums[1]) + b[j])
            assert got[i, j] == (t if t > 0 else np.float32(0.0))
    # one segment, no bias, no activation: the plain chain
    got = exact_ref.linear(x, w, segments=[12])
    acc = np.float32(0.0)
    for kk in range(12):
        acc = exact_ref.fma32(x[2, kk], w[3, kk], acc)
    assert got[2, 3] == acc


def test_wrappers_reject_a_board_without_a_fused_trunk(monkeypatch):
    """The key on a board az_eval_exact_fwd has no trunk for: ValueError when the wrapper is built
    (the check precedes any GPU work; the network constructor is stubbed out, no device here)."""
    from azhip import nets, ops, wrappers
    from connect4.Connect4Game import Connect4Game

    class Net(nets.Connect4Net):
        def __init__(self, game, args, device=None):
            self.board_x, self.board_y = game.getBoardSize()
            self.n = self.board_x

    class W(wrappers.NetWrapper):
        net_class = Net

    monkeypatch.setattr(nets, "default_device", lambda: "cpu")
    with pytest.raises(ValueError, match="batch_invariant.*fused trunk"):
        W(Connect4Game(9), {"batch_invariant": True})
    assert W(Connect4Game(9), {}).batch_invariant is False
    assert W(Connect4Game(7, rows=6), {"batch_invariant": True}).batch_invariant is True
    assert ops.exact_board(Net(Connect4Game(5, rows=4), {})) is not None
    assert ops.exact_board(Net(Connect4Game(4, rows=6), {})) is None
