"""CPU checks of the az_ttt_eval boundary: the ctypes mirror of the descriptor against what a C
compiler makes of include/az_hip.h, and the host-side argument checks of az_ttt_eval_fwd."""
import ctypes
import os

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "az_hip.h")


@pytest.fixture(scope="module")
def built():
    from azhip.build import build
    return build(verbose=False)


def test_ttt_eval_layout_matches_header(built, tmp_path):
    """Every field offset of _lib.TttEval and its size equal offsetof / sizeof of az_ttt_eval."""
    import shutil
    import subprocess
    from azhip import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    cls, cname = _lib.TttEval, "az_ttt_eval"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for f, _ in cls._fields_:
        lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    assert len(cls._fields_) == 31
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f


def test_ttt_eval_host_side_validation_without_gpu(built):
    """az_ttt_eval_fwd checks its arguments on the host before any HIP call: a null descriptor,
    B outside 1..max_B, a bad n / A / F and null pointers return AZ_EINVAL with a message."""
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


def _validation_calls(L, _lib):
    AZ_EINVAL = -1
    call = lambda d, B, v=None: L.az_ttt_eval_fwd(  # noqa: E731
        ctypes.byref(d) if d is not None else None, None, B, None, v, None, None, None)
    assert call(None, 1) == AZ_EINVAL
    assert b"null descriptor" in L.az_last_error()
    d = _lib.TttEval()
    d.max_B, d.n, d.A, d.F = 4, 3, 10, 128
    assert call(d, 0) == AZ_EINVAL
    assert b"B=0" in L.az_last_error()
    assert call(d, 5) == AZ_EINVAL
    assert b"max_B" in L.az_last_error()
    for field, val, word in (("n", 6, b"n=6"), ("n", 2, b"n=2"), ("A", 33, b"A=33"),
                             ("F", 512, b"F=512")):
        bad = _lib.TttEval()
        bad.max_B, bad.n, bad.A, bad.F = 4, 3, 10, 128
        setattr(bad, field, val)
        assert call(bad, 1) == AZ_EINVAL
        assert word in L.az_last_error()
    assert call(d, 1) == AZ_EINVAL
    assert b"neither v nor gv" in L.az_last_error()
    v = (ctypes.c_float * 4)()
    assert call(d, 1, ctypes.cast(v, ctypes.c_void_p)) == AZ_EINVAL
    assert b"null" in L.az_last_error()
    assert L.az_ttt_eval_ws_bytes(4, 6, 10) == 0 and L.az_ttt_eval_ws_bytes(4, 3, 33) == 0
    assert L.az_ttt_eval_ws_bytes(8, 3, 10) < L.az_ttt_eval_ws_bytes(9, 3, 10)
    assert L.az_ttt_trunk_fwd(None, 0, 3, *[None] * 8) == 0
    assert L.az_ttt_trunk_fwd(None, 1, 6, *[None] * 8) == AZ_EINVAL
    assert L.az_ttt_trunk_fwd(None, 1, 3, *[None] * 8) == AZ_EINVAL
