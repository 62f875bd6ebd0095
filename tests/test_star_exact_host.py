"""Batch-invariant star evaluation on the CPU (config key batch_invariant with gnn_neighbors;
DESIGN §10): the new entry points are exported and bound, every host-side rejection of
az_gemm_exact_ex, az_gnn_star_batch_exact_infer and az_star_eval_exact_fwd returns AZ_EINVAL with a
message before any HIP call, and the keys travel together through main.py and Coach."""
import ctypes
import os
import threading

import pytest

from test_exact_host import Args, _eval_desc, _on_own_thread

AZ_OK, AZ_EINVAL = 0, -1
NEW_SYMBOLS = ("az_gemm_exact_ex", "az_gemm_exact_ex_ws_bytes", "az_gnn_star_batch_exact_infer",
               "az_gnn_star_batch_exact_ws_bytes", "az_star_eval_exact_fwd",
               "az_star_eval_exact_ws_bytes")


@pytest.fixture(scope="module")
def L():
    from azhip.build import build
    build(verbose=False)
    from azhip import _lib
    return _lib.load()


def _buf(n=8192):
    buf = (ctypes.c_char * n)()
    p = ctypes.addressof(buf)
    return buf, p + (-p) % 16


def test_new_symbols_are_exported_and_bound(L):
    from azhip import _lib, ops
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    for name in ("linear_exact_ex", "gnn_star_batch_exact_infer", "gnn_star_batch_exact_ws_bytes",
                 "StarEvalExact", "star_eval_exact"):
        assert hasattr(ops, name), name
    import inspect
    assert list(inspect.signature(ops.linear_exact).parameters) == ["x", "w", "b", "act", "out",
                                                                    "M", "ws"]


def test_struct_layouts_match_header(L, tmp_path):
    """The ctypes mirrors of az_gemm_exact_desc and az_star_eval_exact against what a C compiler
    makes of include/az_hip.h."""
    import shutil
    import subprocess
    from azhip import _lib
    from conftest import ROOT
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    hdr = os.path.join(ROOT, "include", "az_hip.h")
    structs = {"az_gemm_exact_desc": _lib.GemmExactDesc, "az_star_eval_exact": _lib.StarEvalExact}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', "int main(){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run([cc, str(src), "-o", str(tmp_path / "probe")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "probe")], capture_output=True,
                                                 text=True, check=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


# ------------------------------------------------------------------ 1. az_gemm_exact_ex
@_on_own_thread
def test_gemm_ex_host_side_validation_without_gpu(L):
    from azhip import _lib
    x = 0x1000                                               # never dereferenced: rejected first

    def desc(M=3, N=16, K=8, **kw):
        d = _lib.GemmExactDesc()
        d.M, d.N, d.K, d.A, d.lda, d.W, d.ldw, d.C, d.ldc = M, N, K, x, K, x, K, x + 0x1000, N
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d):
        return L.az_gemm_exact_ex(ctypes.byref(d), None)

    assert L.az_gemm_exact_ex(None, None) == AZ_EINVAL and b"null" in L.az_last_error()
    assert call(desc(M=0, A=None, W=None, C=None)) == AZ_OK
    assert call(desc(N=18)) == AZ_EINVAL and b"N % 4" in L.az_last_error()
    assert call(desc(K=6)) == AZ_EINVAL and b"K % 4" in L.az_last_error()
    assert call(desc(act=_lib.ACT_TANH)) == AZ_EINVAL and b"act" in L.az_last_error()
    assert call(desc(W2=x, C2=x + 0x2000, act2=_lib.ACT_DRELU)) == AZ_EINVAL
    assert b"act2" in L.az_last_error()
    assert call(desc(W=None)) == AZ_EINVAL and b"null" in L.az_last_error()
    assert call(desc(W2=x)) == AZ_EINVAL and b"null" in L.az_last_error()       # no C2
    assert call(desc(C2=x + 0x2000)) == AZ_EINVAL and b"W2" in L.az_last_error()
    assert call(desc(R=x)) == AZ_EINVAL and b"both R and G" in L.az_last_error()
    assert call(desc(G=x)) == AZ_EINVAL and b"both R and G" in L.az_last_error()
    gated = dict(R=x, ldr=32, G=x, ldg=16)
    assert call(desc(act=_lib.ACT_RELU, **gated)) == AZ_EINVAL
    assert b"no activation" in L.az_last_error()
    assert call(desc(W2=x, C2=x + 0x2000, **gated)) == AZ_EINVAL
    assert b"paired" in L.az_last_error()
    assert call(desc(**dict(gated, ldr=12))) == AZ_EINVAL and b"ldr" in L.az_last_error()
    assert call(desc(**dict(gated, ldg=18))) == AZ_EINVAL and b"ldg" in L.az_last_error()
    assert call(desc(lda=4)) == AZ_EINVAL and b"leading" in L.az_last_error()
    assert call(desc(**dict(gated, R=x + 4))) == AZ_EINVAL and b"alignment" in L.az_last_error()
    assert call(desc(W2=x + 8, C2=x + 0x2000)) == AZ_EINVAL and b"alignment" in L.az_last_error()
    assert call(desc(W2=x, C2=x + 0x1000)) == AZ_EINVAL and b"alias" in L.az_last_error()
    # the spread form's slabs: one product's, and twice that for the paired launch
    one = L.az_gemm_exact_ex_ws_bytes(3, 3136, 3136, 0)
    assert one == L.az_gemm_exact_ws_bytes(3, 3136, 3136) > 0
    assert L.az_gemm_exact_ex_ws_bytes(3, 3136, 3136, 1) == 2 * one
    assert L.az_gemm_exact_ex_ws_bytes(3, 18, 4, 0) == 0     # a rejected shape
    big = dict(N=3136, K=3136, lda=3136, ldw=3136, ldc=3136)
    assert call(desc(**big)) == AZ_EINVAL and b"workspace" in L.az_last_error()
    assert call(desc(ws=x, ws_bytes=one - 1, **big)) == AZ_EINVAL
    assert call(desc(W2=x, C2=x + 0x2000, ws=x, ws_bytes=2 * one - 1, **big)) == AZ_EINVAL
    assert b"workspace" in L.az_last_error()


# ------------------------------------------------------------------ 2. the layer stack
def test_star_batch_exact_host_checks_without_gpu(L):
    """test_star_lockstep.py::test_star_batch_host_checks_without_gpu for the exact entry."""
    from azhip import _lib
    ws_bytes = L.az_gnn_star_batch_exact_ws_bytes
    assert ws_bytes(4, 20, 1024, 128, 2) > 0
    for bad in ((0, 20, 1024, 128, 2), (4, 3, 1024, 128, 2), (4, 20, 1000, 128, 2),
                (4, 20, 1024, 126, 2), (4, 20, 1024, 128, 5), (4, 20, 1024, 128, -1)):
        assert ws_bytes(*bad) == 0, bad
    # monotonic in B and V: a workspace sized for a capacity serves every smaller call
    sizes = [ws_bytes(B, V, 3136, 128, 2) for B, V in ((1, 1), (4, 20), (8, 80), (256, 1024),
                                                       (900, 4000), (4096, 40000))]
    assert sizes == sorted(sizes)
    fn = L.az_gnn_star_batch_exact_infer
    lw = (_lib.LayerW * 4)()
    buf, p = _buf()
    assert fn(None, None, 0, 0, 1024, 128, 2, lw, None, None, 0, None) == 0       # B == 0
    cases = [((p, p + 1024, 4, 20, 1000, 128, 2, lw, p + 2048, p, 1 << 40), b"bad shape"),
             ((p, p + 1024, 4, 20, 1024, 128, 5, lw, p + 2048, p, 1 << 40), b"bad shape"),
             ((p, p + 1024, 4, 3, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"bad shape"),
             ((None, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"null"),
             ((p, None, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"null"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, None, p, 1 << 40), b"null"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, None, 1 << 40), b"null"),
             ((p + 4, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"alignment"),
             ((p, p + 1026, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"alignment"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2052, p, 1 << 40), b"alignment"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p, p + 2048, 1 << 40), b"alias"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1024), b"too small"),
             ((p, p + 1024, 4, 20, 1024, 128, 1, lw, p + 2048, p, 1 << 40), b"null weight")]
    failed = []

    def run():
        try:
            for a, msg in cases:
                assert fn(*a, None) == AZ_EINVAL, msg
                assert msg in L.az_last_error(), (msg, L.az_last_error())
                assert b"az_gnn_star_batch_exact_infer" in L.az_last_error()
        except BaseException as ex:   # reported on the test's own thread
            failed.append(ex)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failed:
        raise failed[0]


# ------------------------------------------------------------------ 3. the evaluator
def _star_desc(_lib, game, nx, ny, A, max_B, max_V, L=2, H=128, fake=0x1000):
    d = _lib.StarEvalExact()
    d.e = _eval_desc(_lib, game, nx, ny, A, max_B, fake)
    d.L, d.H, d.max_V, d.leaf, d.x0 = L, H, max_V, fake, fake + 0x1000
    for i in range(L if 0 <= L <= 4 else 0):
        d.layers[i] = _lib.LayerW(*[fake] * 10)
    return d


@_on_own_thread
def test_star_eval_host_side_validation_without_gpu(L):
    from azhip import _lib
    x = ctypes.c_void_p(0x1000)
    buf, p = _buf()
    offs = (ctypes.c_int * 4).from_address(p)
    offs[:] = [0, 2, 3, 6]
    po = ctypes.c_void_p(p)
    C4, TTT = _lib.EXACT_C4, _lib.EXACT_TTT

    def call(d, B=3, V=6, rows=x, o=po, pi=x, v=x, gpi=x, gv=x):
        return L.az_star_eval_exact_fwd(ctypes.byref(d), rows, o, B, V, pi, v, gpi, gv, None)

    d = _star_desc(_lib, C4, 7, 7, 7, 4, 16)
    assert L.az_star_eval_exact_fwd(None, x, po, 1, 1, x, x, x, x, None) == AZ_EINVAL
    assert call(d, B=0, V=0, rows=None, o=None) == AZ_OK
    assert call(d, B=5, V=6) == AZ_EINVAL and b"max_B" in L.az_last_error()
    assert call(d, B=3, V=17) == AZ_EINVAL and b"max_V" in L.az_last_error()
    assert call(d, B=3, V=2) == AZ_EINVAL and b"B <= V" in L.az_last_error()
    for kw in (dict(rows=None), dict(o=None), dict(v=None), dict(gv=None)):
        assert call(d, **kw) == AZ_EINVAL and b"null" in L.az_last_error(), kw
    for field in ("leaf", "x0"):
        d = _star_desc(_lib, C4, 7, 7, 7, 4, 16)
        setattr(d, field, None)
        assert call(d) == AZ_EINVAL and b"null" in L.az_last_error(), field
    d = _star_desc(_lib, C4, 7, 7, 7, 4, 16)
    d.e.ot0_w = None
    assert call(d) == AZ_EINVAL and b"null" in L.az_last_error()
    d = _star_desc(_lib, C4, 7, 7, 7, 4, 16)
    d.layers[1].gate_w = None
    assert call(d) == AZ_EINVAL and b"null weight pointer in layer 1" in L.az_last_error()
    d = _star_desc(_lib, C4, 7, 7, 7, 4, 16)
    d.e.ws_bytes = L.az_star_eval_exact_ws_bytes(4, 16, C4, 7, 7, 7, 2, 128) - 1
    assert call(d) == AZ_EINVAL and b"workspace" in L.az_last_error()
    d = _star_desc(_lib, C4, 7, 7, 7, 4, 16, L=5)
    assert call(d) == AZ_EINVAL and b"L=5" in L.az_last_error()
    d = _star_desc(_lib, C4, 7, 7, 7, 4, 16, H=126)
    assert call(d) == AZ_EINVAL and b"H=126" in L.az_last_error()
    d = _star_desc(_lib, C4, 7, 7, 40, 4, 16)                        # A > 32
    assert call(d) == AZ_EINVAL and b"A=40" in L.az_last_error()
    d = _star_desc(_lib, C4, 9, 9, 9, 4, 16)                         # no fused trunk
    assert call(d) == AZ_EINVAL and b"fused trunk" in L.az_last_error()
    d = _star_desc(_lib, TTT, 4, 4, 17, 4, 16)
    d.e.fc1_w = None
    assert call(d) == AZ_EINVAL and b"null" in L.az_last_error()
    d = _star_desc(_lib, C4, 7, 7, 7, 4, 16)
    d.x0 = 0x2004
    assert call(d) == AZ_EINVAL and b"alignment" in L.az_last_error()
    assert call(_star_desc(_lib, C4, 7, 7, 7, 4, 16), o=ctypes.c_void_p(p + 2)) == AZ_EINVAL
    assert b"alignment" in L.az_last_error()


def test_star_eval_ws_bytes(L):
    from azhip import _lib
    C4, TTT = _lib.EXACT_C4, _lib.EXACT_TTT
    ws = L.az_star_eval_exact_ws_bytes
    # 0 for a board without a fused trunk, and for every other rejected shape
    assert ws(4, 16, C4, 9, 9, 9, 2, 128) == 0
    assert ws(4, 16, C4, 4, 6, 4, 2, 128) == 0
    assert ws(4, 16, TTT, 6, 6, 37, 2, 128) == 0
    assert ws(0, 16, C4, 7, 7, 7, 2, 128) == 0
    assert ws(4, 3, C4, 7, 7, 7, 2, 128) == 0                # max_V < max_B
    assert ws(4, 16, C4, 7, 7, 40, 2, 128) == 0
    assert ws(4, 16, C4, 7, 7, 7, 5, 128) == 0
    assert ws(4, 16, C4, 7, 7, 7, 2, 126) == 0
    for game, nx, ny in ((C4, 7, 7), (C4, 4, 4), (C4, 5, 5), (C4, 6, 6), (C4, 8, 8), (C4, 7, 6),
                         (C4, 6, 5), (C4, 5, 4), (C4, 8, 7), (TTT, 3, 3), (TTT, 4, 4),
                         (TTT, 5, 5)):
        assert ws(4096, 36864, game, nx, ny, 8, 2, 128) >= ws(256, 1024, game, nx, ny, 8, 2, 128) \
            > 0, (game, nx, ny)


# ------------------------------------------------------------------ 4. the keys together
def _invariant_star_net():
    from test_star_lockstep import StarHashNet

    class InvariantStarNet(StarHashNet):
        batch_invariant_stars = True

    return StarHashNet, InvariantStarNet


def test_coach_accepts_the_key_with_gnn_neighbors_for_an_invariant_network():
    import Coach as C
    from connect4.Connect4Game import Connect4Game
    from azhip.build import build_host
    build_host(verbose=False)
    plain, invariant = _invariant_star_net()
    game = Connect4Game(4)
    base = dict(numEps=1, numMCTSSims=2, cpuct=1.0, tempThreshold=2, use_gnn=True, expand_by=1)
    for extra in (dict(gnn_neighbors=True),
                  dict(gnn_neighbors=True, gnn_neighbors_lockstep=True, parallel_games=4)):
        coach = C.Coach(game, invariant(game), Args(batch_invariant=True, **base, **extra))
        assert coach.args.batch_invariant and coach.args.gnn_neighbors
        # without the attribute (or with it false) the refusal stands, message unchanged
        with pytest.raises(ValueError, match="batch_invariant cannot be combined with "
                                             "gnn_neighbors"):
            C.Coach(game, plain(game), Args(batch_invariant=True, **base, **extra))
        no = invariant(game)
        no.batch_invariant_stars = False
        with pytest.raises(ValueError, match="batch_invariant.*gnn_neighbors"):
            C.Coach(game, no, Args(batch_invariant=True, **base, **extra))
    # lock-step with the key still runs in the engine lanes
    coach = C.Coach(game, invariant(game),
                    Args(batch_invariant=True, gnn_neighbors=True, gnn_neighbors_lockstep=True,
                         parallel_games=4, **base))
    assert coach.selfplay_uses_native_engine()


def test_wrapper_property_and_depth_limit(monkeypatch):
    """batch_invariant_stars: the key and at most STAR_MAX_LAYERS layers; with more layers under
    the key the star entry points raise, they never fall to another route (no device needed: the
    check precedes any GPU work)."""
    from types import SimpleNamespace
    from azhip import ops, wrappers

    class W(wrappers.GNNWrapperMixin):
        def __init__(self, key, layers):
            self.batch_invariant = key
            self.gnn = SimpleNamespace(num_layers=layers, eval=lambda: None)
            self.nnet = SimpleNamespace(eval=lambda: None)
            self.action_size, self.board_x, self.board_y = 4, 4, 4
            self._sync_params = lambda: None

    assert W(True, 2).batch_invariant_stars is True
    assert W(True, ops.STAR_MAX_LAYERS).batch_invariant_stars is True
    assert W(True, ops.STAR_MAX_LAYERS + 1).batch_invariant_stars is False
    assert W(False, 2).batch_invariant_stars is False
    import numpy as np
    deep = W(True, ops.STAR_MAX_LAYERS + 1)
    board = np.zeros((4, 4), np.int8)
    rows, offs = np.zeros((2, 4, 4), np.int8), np.array([0, 2], np.int32)
    with pytest.raises(ValueError, match="at most 4 GNN layers"):
        deep.predict_star_batch([[board, board]])
    with pytest.raises(ValueError, match="at most 4 GNN layers"):
        deep.predict_with_gnn(board, [board])
    with pytest.raises(ValueError, match="at most 4 GNN layers"):
        deep.predict_both_stars(rows, offs)
    with pytest.raises(ValueError, match="at most 4 GNN layers"):
        deep.predict_both_stars_async(rows, offs)


def test_main_carries_the_keys_together(tmp_path):
    import main
    import yaml
    cfg = tmp_path / "config.yaml"
    doc = {"game": {"board_size": 4}, "training": {"checkpoint_path": str(tmp_path / "ck")},
           "neural_network": {"use_gnn": True}}
    cfg.write_text(yaml.safe_dump(doc))
    base = ["--game", "connect4", "--use_gnn", "--config", str(cfg)]
    a = main.build_args(main.parse(base + ["--batch_invariant", "--gnn_neighbors",
                                           "--gnn_neighbors_lockstep"]))
    assert a.batch_invariant is True and a.gnn_neighbors is True
    assert a.gnn_neighbors_lockstep is True
    a = main.build_args(main.parse(base + ["--batch_invariant", "--gnn_neighbors"]))
    assert a.batch_invariant is True and a.gnn_neighbors is True
    doc["selfplay"] = {"batch_invariant": True, "gnn_neighbors": True}
    cfg.write_text(yaml.safe_dump(doc))
    a = main.build_args(main.parse(base))
    assert a.batch_invariant is True and a.gnn_neighbors is True
    # the help text and the shipped comments no longer exclude the combination
    assert "not with --gnn_neighbors" not in main.__doc__
    assert "az_star_eval_exact_fwd" in main.__doc__
    for name in ("connect4", "tictactoe"):
        text = open(os.path.join(main.HERE, name, "config.yaml")).read()
        assert "not with" not in text.split("batch_invariant:")[1].split("gnn_neighbors_train")[0]
