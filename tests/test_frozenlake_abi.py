"""CPU checks of the FrozenLake boundary: the ctypes mirrors of az_fl_eval / az_fl_params against
what a C compiler makes of include/az_hip.h, the host-side argument checks of az_fl_eval_fwd,
az_fl_grads and az_clip_grad_norm, and the wrapper's refusal to run without a HIP device."""
import ctypes
import os

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "az_hip.h")


@pytest.fixture(scope="module")
def built():
    from azhip.build import build
    return build(verbose=False)


def test_fl_layouts_match_header(built, tmp_path):
    import shutil
    import subprocess
    from azhip import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler (the build needs one anyway)"
    structs = {"az_fl_params": _lib.FlParams, "az_fl_eval": _lib.FlEval}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("layers %d\\n", AZ_FL_MAX_LAYERS);')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(got["layers"]) == _lib.FL_MAX_LAYERS
    assert len(_lib.FlParams._fields_) == 10 and len(_lib.FlEval._fields_) == 7
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_fl_host_side_validation_without_gpu(built):
    import threading
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


def _desc(_lib, **over):
    d = _lib.FlEval()
    d.S, d.E, d.L, d.A, d.H, d.max_B = 16, 64, 2, 4, 128, 4
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _validation_calls(L, _lib):
    AZ_EINVAL = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ref = lambda d: ctypes.byref(d) if d is not None else None  # noqa: E731
    fwd = lambda d, B, nodes=None, counts=None, pi=None, v=None: L.az_fl_eval_fwd(  # noqa: E731
        ref(d), nodes, counts, B, pi, v, None, None)
    grads = lambda d, B, nodes=None, counts=None, g=None, rest=None, ws=None, nb=0: \
        L.az_fl_grads(ref(d), nodes, counts, B, rest, rest, ref(g), rest, None, ws, nb, None)  # noqa: E731
    for name, call in (("az_fl_eval_fwd", fwd), ("az_fl_grads", grads)):
        tag = name.encode()
        assert call(None, 1) == AZ_EINVAL
        assert tag + b": null descriptor" in L.az_last_error()
        for B, word in ((0, b"B=0"), (5, b"B=5 max_B=4"), (-1, b"B=-1")):
            assert call(_desc(_lib), B) == AZ_EINVAL
            assert tag in L.az_last_error() and word in L.az_last_error()
        for field, val, word in (("S", 65, b"S=65"), ("S", 3, b"S=3"), ("E", 96, b"E=96"),
                                 ("L", 0, b"L=0"), ("L", 5, b"L=5"), ("A", 7, b"A=7"),
                                 ("H", 256, b"H=256")):
            assert call(_desc(_lib, **{field: val}), 1) == AZ_EINVAL
            assert b"bad shape" in L.az_last_error() and word in L.az_last_error()
        assert call(_desc(_lib), 1, nodes=p) == AZ_EINVAL
        assert b"null counts" in L.az_last_error()
        assert call(_desc(_lib), 1, counts=p) == AZ_EINVAL            # nodes null
        assert b"null nodes / weight" in L.az_last_error()
        assert call(_desc(_lib), 1, nodes=p, counts=p) == AZ_EINVAL   # weights null
        assert b"null nodes / weight" in L.az_last_error()
    # complete weights: the remaining checks of each entry point
    d = _desc(_lib)
    w = (ctypes.c_float * 64)()
    wp = ctypes.cast(w, ctypes.c_void_p).value
    d.w = _full_params(_lib, wp)
    assert fwd(d, 1, nodes=p, counts=p) == AZ_EINVAL
    assert b"null pi / v" in L.az_last_error()
    mis = _desc(_lib)
    mis.w = _full_params(_lib, wp)
    mis.w.fe2_w = wp + 4
    assert fwd(mis, 1, nodes=p, counts=p, pi=p, v=p) == AZ_EINVAL
    assert b"16B alignment" in L.az_last_error()
    assert grads(d, 1, nodes=p, counts=p) == AZ_EINVAL
    assert b"null targets / loss" in L.az_last_error()
    assert grads(d, 1, nodes=p, counts=p, rest=p) == AZ_EINVAL
    assert b"null gradient pointer" in L.az_last_error()
    g = _full_params(_lib, wp)
    g.gnn_b[1] = None
    assert grads(d, 1, nodes=p, counts=p, rest=p, g=g) == AZ_EINVAL
    assert b"null gradient pointer" in L.az_last_error()
    g = _full_params(_lib, wp)
    assert grads(d, 1, nodes=p, counts=p, rest=p, g=g) == AZ_EINVAL
    assert b"workspace null or too small" in L.az_last_error()
    assert grads(d, 1, nodes=p, counts=p, rest=p, g=g, ws=p, nb=16) == AZ_EINVAL
    assert b"workspace null or too small" in L.az_last_error()
    assert L.az_fl_eval_ws_bytes(0, 16, 64, 2) == 0 and L.az_fl_eval_ws_bytes(4, 65, 64, 2) == 0
    assert L.az_fl_eval_ws_bytes(4, 16, 96, 2) == 0 and L.az_fl_eval_ws_bytes(4, 16, 64, 5) == 0
    assert 0 < L.az_fl_eval_ws_bytes(4, 16, 64, 2) < L.az_fl_eval_ws_bytes(5, 16, 64, 2)
    # az_clip_grad_norm
    bufs = (ctypes.c_void_p * 2)(wp, wp)
    sizes = (ctypes.c_int64 * 2)(8, 8)
    clip = L.az_clip_grad_norm
    assert clip(bufs, sizes, 0, 1.0, p, None) == AZ_EINVAL
    assert b"n=0 buffers" in L.az_last_error()
    assert clip(bufs, sizes, 17, 1.0, p, None) == AZ_EINVAL
    assert b"n=17 buffers" in L.az_last_error()
    assert clip(None, sizes, 2, 1.0, p, None) == AZ_EINVAL
    assert b"null pointer" in L.az_last_error()
    assert clip(bufs, sizes, 2, 1.0, None, None) == AZ_EINVAL
    assert b"null pointer" in L.az_last_error()
    assert clip(bufs, sizes, 2, 0.0, p, None) == AZ_EINVAL
    assert b"max_norm=0" in L.az_last_error()
    assert clip((ctypes.c_void_p * 2)(wp, None), sizes, 2, 1.0, p, None) == AZ_EINVAL
    assert b"buffer 1 is null" in L.az_last_error()
    assert clip(bufs, (ctypes.c_int64 * 2)(8, -1), 2, 1.0, p, None) == AZ_EINVAL
    assert b"buffer 1 is null or has a negative size" in L.az_last_error()


def _full_params(_lib, ptr):
    g = _lib.FlParams()
    for f, _ in _lib.FlParams._fields_:
        if f in ("gnn_w", "gnn_b"):
            arr = getattr(g, f)
            for i in range(_lib.FL_MAX_LAYERS):
                arr[i] = ptr
        else:
            setattr(g, f, ptr)
    return g


def test_wrapper_raises_without_a_device(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    from frozenlake.FrozenLakeNet import FrozenLakeNet
    with pytest.raises(RuntimeError, match="no HIP device"):
        FrozenLakeNet(FrozenLakeGame(), {"lr": 0.001, "embedding_dim": 64, "gnn_layers": 2})
