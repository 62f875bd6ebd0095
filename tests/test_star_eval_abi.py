"""CPU checks of the star-evaluation boundary (az_gnn_star_infer, az_c4_star_eval_fwd): the header
and the ctypes binding declare the same entry points with the same signatures, the ctypes mirror of
az_c4_star_eval has the layout a C compiler gives the header's struct, the ABI version is still 2,
the host-side argument checks of the entry points, and that the wrappers raise without a device."""
import ctypes
import re
import threading

import pytest

from test_c4n_eval_abi import HEADER, _header_signature

NAMES = ("az_gnn_star_infer_ws_bytes", "az_gnn_star_infer", "az_c4_star_eval_ws_bytes",
         "az_c4_star_eval_fwd")
AZ_EINVAL = -1


@pytest.fixture(scope="module")
def built():
    from azhip.build import build
    return build(verbose=False)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_and_binding_declare_the_same_signatures():
    from azhip import _lib
    assert re.search(r"typedef\s+struct\s+az_c4_star_eval\s*\{", _header())
    names = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name in NAMES:
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
    assert _lib.SIGNATURES["az_c4_star_eval_fwd"][1][0] is ctypes.POINTER(_lib.C4StarEval)
    assert _lib.SIGNATURES["az_gnn_star_infer"][1][7] is ctypes.POINTER(_lib.LayerW)
    for macro, value in (("AZ_STAR_MAX_NODES", _lib.STAR_MAX_NODES),
                         ("AZ_STAR_MAX_STARS", _lib.STAR_MAX_STARS),
                         ("AZ_STAR_MAX_LAYERS", _lib.STAR_MAX_LAYERS),
                         ("AZ_STAR_HIDDEN", _lib.STAR_HIDDEN)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", _header()).group(1)) == value
    assert (_lib.STAR_MAX_NODES, _lib.STAR_MAX_STARS) == (9, 8)


def test_abi_version_is_still_2(built):
    from azhip import _lib
    assert int(re.search(r"#define\s+AZ_ABI_VERSION\s+(\d+)", _header()).group(1)) == 2
    assert _lib.load().az_abi_version() == 2


def test_c4_star_eval_layout_matches_header(built, tmp_path):
    """Field order, every field offset, the layer array and the size of _lib.C4StarEval equal what
    a C compiler makes of az_c4_star_eval."""
    import shutil
    import subprocess
    from azhip import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    cls, cname = _lib.C4StarEval, "az_c4_star_eval"
    fields = [f for f, _ in cls._fields_]
    body = re.search(r"typedef\s+struct\s+az_c4_star_eval\s*\{(.*?)\}\s*az_c4_star_eval\s*;",
                     _header(), flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*(?:\[\w+\])?\s*;", body) == fields     # the header's field order
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             f'printf("{cname} %zu\\n", sizeof({cname}));',
             f'printf("layer %zu\\n", sizeof(az_gnn_layer_w));']
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


def test_host_side_validation_without_gpu(built):
    """Both entry points check their arguments on the host before any HIP call: B = 0 is a no-op,
    B = 9, a board without a fused trunk, L = 5, an F off by 64 and null pointers return AZ_EINVAL
    with the offending value in az_last_error()."""
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
    call = lambda d, B, gv=None, boards=None, counts=None: L.az_c4_star_eval_fwd(  # noqa: E731
        ctypes.byref(d) if d is not None else None, boards, counts, B, None, gv, None)
    assert call(None, 1) == AZ_EINVAL
    assert b"null descriptor" in L.az_last_error()

    def desc(**kw):
        d = _lib.C4StarEval()
        d.max_B, d.nx, d.ny, d.A, d.F, d.L = 8, 7, 6, 8, 2688, 2
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    assert call(desc(), 0) == 0                                   # nothing to do
    for shape in ((7, 7), (4, 4), (8, 8), (5, 4), (8, 7)):
        assert call(desc(nx=shape[0], ny=shape[1], F=64 * shape[0] * shape[1]), 0) == 0
    assert call(desc(), 9) == AZ_EINVAL
    assert b"B=9" in L.az_last_error()
    assert call(desc(max_B=4), 5) == AZ_EINVAL
    assert b"B=5" in L.az_last_error() and b"max_B=4" in L.az_last_error()
    assert call(desc(), -1) == AZ_EINVAL
    assert call(desc(nx=6, ny=7), 1) == AZ_EINVAL
    assert b"nx=6 ny=7" in L.az_last_error()
    assert call(desc(nx=9, ny=9, F=64 * 81), 1) == AZ_EINVAL
    assert b"nx=9 ny=9" in L.az_last_error()
    assert call(desc(L=5), 1) == AZ_EINVAL
    assert b"L=5" in L.az_last_error()
    assert call(desc(L=-1), 1) == AZ_EINVAL
    assert call(desc(F=2688 + 64), 1) == AZ_EINVAL
    assert b"F=2752" in L.az_last_error()
    assert call(desc(A=33), 1) == AZ_EINVAL
    assert b"A=33" in L.az_last_error()
    assert call(desc(), 1) == AZ_EINVAL
    assert b"null pointer" in L.az_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert call(desc(), 1, gv=p, boards=p, counts=p) == AZ_EINVAL
    assert b"null pointer (weights)" in L.az_last_error()
    # workspace sizes
    assert L.az_c4_star_eval_ws_bytes(8, 6, 7, 8, 2) == 0
    assert L.az_c4_star_eval_ws_bytes(9, 7, 6, 8, 2) == 0
    assert L.az_c4_star_eval_ws_bytes(8, 7, 6, 8, 5) == 0
    assert L.az_c4_star_eval_ws_bytes(8, 7, 6, 33, 2) == 0
    for nx, ny in ((7, 7), (4, 4), (5, 5), (6, 6), (8, 8), (7, 6), (6, 5), (5, 4), (8, 7)):
        F = 64 * nx * ny
        star = L.az_gnn_star_infer_ws_bytes(8, F, 128, 2)
        assert star > 0
        assert L.az_c4_star_eval_ws_bytes(8, nx, ny, nx + 1, 2) == \
            (star + 255) // 256 * 256 + L.az_transform_heads_ws_bytes(8, F, nx + 1)
    # az_gnn_star_infer
    infer = lambda B, F, H, Ln, ld=None, x=None, ws=None, nb=0: L.az_gnn_star_infer(  # noqa: E731
        x, 9 * F if ld is None else ld, x, B, F, H, Ln, None, x, ws, nb, None)
    assert infer(0, 1024, 128, 2) == 0
    for args, word in (((9, 1024, 128, 2), b"B=9"), ((1, 1022, 128, 2), b"F=1022"),
                       ((1, 1024, 127, 2), b"H=127"), ((1, 1024, 128, 5), b"L=5"),
                       ((1, 1024, 128, -1), b"L=-1")):
        assert infer(*args) == AZ_EINVAL
        assert word in L.az_last_error(), word
        assert L.az_gnn_star_infer_ws_bytes(*args) == 0
    assert infer(1, 1024, 128, 2, ld=1000) == AZ_EINVAL
    assert b"ldstar=1000" in L.az_last_error()
    assert infer(1, 1024, 128, 2) == AZ_EINVAL
    assert b"null pointer" in L.az_last_error()
    assert infer(1, 1024, 128, 0, x=ctypes.c_void_p(ctypes.addressof(buf) + 4)) == AZ_EINVAL
    assert b"alignment" in L.az_last_error()


def test_wrappers_raise_without_a_device(built):
    """No CPU fallback: without a HIP device ops.C4StarEval, ops.gnn_star_infer and the GNN wrapper
    raise, as every other entry of the package does."""
    import torch
    if torch.cuda.is_available():
        return                                   # the GPU suite covers the working path
    from types import SimpleNamespace
    from azhip import ops
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Game import Connect4Game
    with pytest.raises(RuntimeError, match="no HIP device"):
        ops.C4StarEval({}, {}, (7, 6), 8, 2, 8, "cpu")
    with pytest.raises((RuntimeError, ValueError)):
        ops.gnn_star_infer(torch.zeros(1, 9, 1024), torch.ones(1, dtype=torch.int32), [])
    with pytest.raises(RuntimeError, match="no HIP device"):
        Connect4GNNWrapper(Connect4Game(7, rows=6), SimpleNamespace(gnn_layers=2, dropout=0.3))
