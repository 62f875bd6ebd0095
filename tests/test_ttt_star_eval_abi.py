"""CPU checks of the TicTacToe star-evaluation boundary (az_gnn_star_packed_infer,
az_ttt_star_eval_fwd): the header, the library's exports and the ctypes binding agree on the four
entry points, the ctypes mirror of az_ttt_star_eval has the layout a C compiler gives the header's
struct, AZ_TTT_STAR_MAX_NODES is 26 beside the unchanged older macros and ABI version, the
workspace sizes, the host-side argument checks, and that the wrappers raise without a device.

The offs checks (a non-ascending offs, a 27-row star, offs[B] != V) are NOT here: the library
tells a mapped-host offs from a device one by asking the runtime, which knows neither without a
device, so they are held on the GPU (tests/test_gpu_ttt_star_eval.py)."""
import ctypes
import re
import threading

import pytest

from test_c4n_eval_abi import HEADER, _header_signature

NAMES = ("az_gnn_star_packed_infer_ws_bytes", "az_gnn_star_packed_infer",
         "az_ttt_star_eval_ws_bytes", "az_ttt_star_eval_fwd")
AZ_EINVAL = -1


@pytest.fixture(scope="module")
def built():
    from azhip.build import build
    return build(verbose=False)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_exports_and_binding_agree(built):
    from azhip import _lib
    assert re.search(r"typedef\s+struct\s+az_ttt_star_eval\s*\{", _header())
    lib = ctypes.CDLL(built)
    names = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        hres, hargs = _header_signature(name)
        assert res is names[hres], name
        assert len(args) == len(hargs), name
        for i, (a, h) in enumerate(zip(args, hargs)):
            if h == "ptr":
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, i)
            else:
                assert a is names[h], (name, i)
    assert _lib.SIGNATURES["az_ttt_star_eval_fwd"][1][0] is ctypes.POINTER(_lib.TttStarEval)
    assert _lib.SIGNATURES["az_gnn_star_packed_infer"][1][7] is ctypes.POINTER(_lib.LayerW)


def test_macros_and_abi_version(built):
    """AZ_TTT_STAR_MAX_NODES is 26 (a 5x5 leaf and its 25 children); the 9 row slots, 8 stars and 4
    layers of the Connect4 star kernels and the ABI version are what they were."""
    from azhip import _lib, ops
    for macro, value, expect in (("AZ_TTT_STAR_MAX_NODES", _lib.TTT_STAR_MAX_NODES, 26),
                                 ("AZ_STAR_MAX_NODES", _lib.STAR_MAX_NODES, 9),
                                 ("AZ_STAR_MAX_STARS", _lib.STAR_MAX_STARS, 8),
                                 ("AZ_STAR_MAX_LAYERS", _lib.STAR_MAX_LAYERS, 4),
                                 ("AZ_ABI_VERSION", _lib.load().az_abi_version(), 2)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", _header()).group(1)) == expect
        assert value == expect, macro
    assert ops.TTT_STAR_MAX_NODES == 26
    assert [ops.ttt_star_shape_ok(n) for n in (2, 3, 4, 5, 6)] == [False, True, True, True, False]


def test_ttt_star_eval_layout_matches_header(built, tmp_path):
    """Field order, every field offset, the layer array and the size of _lib.TttStarEval equal what
    a C compiler makes of az_ttt_star_eval."""
    import shutil
    import subprocess
    from azhip import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    cls, cname = _lib.TttStarEval, "az_ttt_star_eval"
    fields = [f for f, _ in cls._fields_]
    body = re.search(r"typedef\s+struct\s+az_ttt_star_eval\s*\{(.*?)\}\s*az_ttt_star_eval\s*;",
                     _header(), flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*(?:\[\w+\])?\s*;", body) == fields     # the header's field order
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             f'printf("{cname} %zu\\n", sizeof({cname}));',
             'printf("layer %zu\\n", sizeof(az_gnn_layer_w));']
    for f in fields:
        lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    assert int(got["layer"]) == ctypes.sizeof(_lib.LayerW)
    assert cls.layers.size == _lib.STAR_MAX_LAYERS * ctypes.sizeof(_lib.LayerW)
    for f in fields:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f


def test_workspace_sizes(built):
    """Both _ws_bytes return 0 for n = 2, n = 6, max_B = 0 or 9, L = 5 and A = 33 (F and H where
    the layer stack has no n and A), and are positive and increasing in max_B for n = 3..5."""
    from azhip import _lib
    L = _lib.load()
    ev, st = L.az_ttt_star_eval_ws_bytes, L.az_gnn_star_packed_infer_ws_bytes
    for args in ((8, 2, 5, 2), (8, 6, 37, 2), (0, 3, 10, 2), (9, 3, 10, 2), (8, 3, 10, 5),
                 (8, 3, 33, 2), (8, 3, 0, 2), (8, 3, 10, -1)):
        assert ev(*args) == 0, args
    for args in ((0, 128, 128, 2), (9, 128, 128, 2), (8, 128, 128, 5), (8, 128, 128, -1),
                 (8, 126, 128, 2), (8, 0, 128, 2), (8, 128, 64, 2)):
        assert st(*args) == 0, args
    for n in (3, 4, 5):
        F, A = 128 * (n - 2) ** 2, n * n + 1
        for Ln in (0, 2, 4):
            sizes = [ev(B, n, A, Ln) for B in range(1, 9)]
            stars = [st(B, F, 128, Ln) for B in range(1, 9)]
            assert sizes[0] > 0 and stars[0] > 0, (n, Ln)
            assert all(a < b for a, b in zip(sizes, sizes[1:])), (n, Ln, sizes)
            assert all(a < b for a, b in zip(stars, stars[1:])), (n, Ln, stars)
            assert all(e >= s for e, s in zip(sizes, stars))


def test_host_side_validation_without_gpu(built):
    """Both entry points check their arguments on the host before any HIP call: B = 0 is a no-op;
    a null descriptor, B = 9, an F that is not 128 (n-2)^2, misaligned scratch, a too-small
    workspace and the other bad shapes return AZ_EINVAL with the offending value in
    az_last_error()."""
    from azhip import _lib
    L = _lib.load()
    failure = []

    def run():
        try:
            _validation_calls(L, _lib)
        except BaseException as ex:   # reported on the test's own thread
            failure.append(ex)

    # az_last_error is per thread: the rejected calls run on a thread of their own, so the main
    # thread keeps the empty message tests/test_lib_abi.py expects whatever the test order
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failure:
        raise failure[0]


def _validation_calls(L, _lib):
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p = ctypes.c_void_p(base)
    odd = ctypes.c_void_p(base + 4)

    def call(d, B, V=None, gv=None, rows=None, offs=None):
        return L.az_ttt_star_eval_fwd(ctypes.byref(d) if d is not None else None, rows, offs, B,
                                      B if V is None else V, None, gv, None)

    assert call(None, 1) == AZ_EINVAL
    assert b"null descriptor" in L.az_last_error()

    def desc(full=False, **kw):
        d = _lib.TttStarEval()
        d.max_B, d.n, d.A, d.F, d.L = 8, 4, 17, 512, 2
        if full:
            for name, _ in _lib.TttStarEval._fields_:
                if name.endswith(("_w", "_b")) or name in ("feat", "x0", "hidden", "y", "h1", "h2",
                                                           "glogp", "ws"):
                    setattr(d, name, p)
            for i in range(_lib.STAR_MAX_LAYERS):
                d.layers[i] = _lib.LayerW(*[p] * len(_lib.LAYER_FIELDS))
            d.ws_bytes = L.az_ttt_star_eval_ws_bytes(8, 4, 17, 2)
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    assert call(desc(), 0) == 0                                   # nothing to do
    for n in (3, 4, 5):
        assert call(desc(n=n, A=n * n + 1, F=128 * (n - 2) ** 2), 0) == 0
    assert call(desc(), 9) == AZ_EINVAL
    assert b"B=9" in L.az_last_error()
    assert call(desc(max_B=4), 5) == AZ_EINVAL
    assert b"B=5" in L.az_last_error() and b"max_B=4" in L.az_last_error()
    assert call(desc(), -1) == AZ_EINVAL
    for n in (2, 6):
        assert call(desc(n=n, F=128 * (n - 2) ** 2), 1) == AZ_EINVAL
        assert b"n=%d" % n in L.az_last_error()
    assert call(desc(F=512 + 128), 1) == AZ_EINVAL
    assert b"F=640" in L.az_last_error()
    assert call(desc(A=33), 1) == AZ_EINVAL
    assert b"A=33" in L.az_last_error()
    assert call(desc(L=5), 1) == AZ_EINVAL
    assert b"L=5" in L.az_last_error()
    assert call(desc(L=-1), 1) == AZ_EINVAL
    assert call(desc(), 2, V=1) == AZ_EINVAL
    assert b"V=1" in L.az_last_error()
    assert call(desc(), 2, V=53) == AZ_EINVAL                     # more than 26 boards per star
    assert b"V=53" in L.az_last_error()
    assert call(desc(), 1) == AZ_EINVAL
    assert b"null pointer (rows / offs / gv)" in L.az_last_error()
    assert call(desc(), 1, gv=p, rows=p, offs=p) == AZ_EINVAL
    assert b"null pointer (weights)" in L.az_last_error()
    assert call(desc(full=True, y=None), 1, gv=p, rows=p, offs=p) == AZ_EINVAL
    assert b"null pointer (scratch" in L.az_last_error()
    for field in ("feat", "x0", "hidden", "y", "h1", "h2", "ws"):
        assert call(desc(full=True, **{field: odd}), 1, gv=p, rows=p, offs=p) == AZ_EINVAL, field
        assert b"scratch needs 16B alignment" in L.az_last_error(), field
    need = L.az_ttt_star_eval_ws_bytes(8, 4, 17, 2)
    assert call(desc(full=True, ws_bytes=need - 1), 1, gv=p, rows=p, offs=p) == AZ_EINVAL
    assert b"too small" in L.az_last_error()
    d = desc(full=True)
    d.layers[1].gate_w = None
    assert call(d, 1, gv=p, rows=p, offs=p) == AZ_EINVAL
    assert b"null weight pointer in layer 1" in L.az_last_error()
    # az_gnn_star_packed_infer
    infer = lambda B, V, F, H, Ln, x=None, x0=None, ws=None, nb=0, offs=None: \
        L.az_gnn_star_packed_infer(x, offs, B, V, F, H, Ln, None, x0, ws, nb, None)  # noqa: E731
    assert infer(0, 0, 512, 128, 2) == 0
    for args, word in (((9, 9, 512, 128, 2), b"B=9"), ((1, 1, 510, 128, 2), b"F=510"),
                       ((1, 1, 512, 64, 2), b"H=64"), ((1, 1, 512, 128, 5), b"L=5"),
                       ((1, 1, 512, 128, -1), b"L=-1")):
        assert infer(*args) == AZ_EINVAL
        assert word in L.az_last_error(), word
    assert infer(2, 1, 512, 128, 2) == AZ_EINVAL
    assert b"V=1" in L.az_last_error()
    assert infer(1, 27, 512, 128, 2) == AZ_EINVAL
    assert b"V=27" in L.az_last_error()
    assert infer(1, 1, 512, 128, 2) == AZ_EINVAL
    assert b"null pointer" in L.az_last_error()
    q = ctypes.c_void_p(base + 2048)
    assert infer(1, 1, 512, 128, 0, x=odd, x0=q, offs=p) == AZ_EINVAL
    assert b"alignment" in L.az_last_error()
    assert infer(1, 1, 512, 128, 0, x=p, x0=p, offs=p) == AZ_EINVAL
    assert b"alias" in L.az_last_error()
    lw = (_lib.LayerW * 2)(*[_lib.LayerW(*[p] * len(_lib.LAYER_FIELDS))] * 2)
    need = L.az_gnn_star_packed_infer_ws_bytes(1, 512, 128, 2)
    assert L.az_gnn_star_packed_infer(p, p, 1, 1, 512, 128, 2, lw, q, p, need - 1,
                                      None) == AZ_EINVAL
    assert b"too small" in L.az_last_error()


def test_wrappers_raise_without_a_device(built):
    """No CPU fallback: without a HIP device ops.TttStarEval, ops.gnn_star_packed_infer and the
    TicTacToe GNN wrapper raise, as every other entry of the package does."""
    import torch
    if torch.cuda.is_available():
        return                                   # the GPU suite covers the working path
    from types import SimpleNamespace
    from azhip import ops
    from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    with pytest.raises(RuntimeError, match="no HIP device"):
        ops.TttStarEval({}, {}, 3, 10, 2, 8, "cpu")
    with pytest.raises((RuntimeError, ValueError)):
        ops.gnn_star_packed_infer(torch.zeros(3, 128), torch.tensor([0, 3], dtype=torch.int32), [])
    with pytest.raises(RuntimeError, match="no HIP device"):
        TicTacToeGNNWrapper(TicTacToeGame(3),
                            SimpleNamespace(gnn_layers=2, dropout=0.3, gnn_neighbors=True))
