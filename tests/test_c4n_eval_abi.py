"""CPU checks of the az_c4n_* boundary (Connect4 on 4x4, 5x5, 6x6 and 8x8 boards): the header and
the ctypes binding declare the same entry points with the same signatures, the ctypes mirror of
az_c4n_eval has the layout a C compiler gives the header's struct, the host-side argument checks
of the entry points, and which boards the wrappers route to the evaluator."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "az_hip.h")
NAMES = ("az_c4n_trunk_fwd", "az_c4n_trunk_heads_fwd", "az_c4n_eval_ws_bytes", "az_c4n_eval_fwd")


@pytest.fixture(scope="module")
def built():
    from azhip.build import build
    return build(verbose=False)


def _header_signature(name):
    """(return type, [parameter types]) of `name` as include/az_hip.h declares it, each type as
    the ctypes type the binding must use for it."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in az_hip.h"

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return "ptr"
        return decl.rsplit(" ", 1)[0].replace("const ", "").strip()

    return m.group(1), [ctype(p) for p in m.group(2).split(",")]


def test_header_and_binding_declare_the_same_signatures():
    from azhip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+az_c4n_eval\s*\{", src)
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
    assert _lib.SIGNATURES["az_c4n_eval_fwd"][1][0] is ctypes.POINTER(_lib.C4nEval)


def test_c4n_eval_layout_matches_header(built, tmp_path):
    """Field order, every field offset and the size of _lib.C4nEval equal what a C compiler makes
    of az_c4n_eval: az_c4_eval's fields without sync / err, then n and F."""
    import shutil
    import subprocess
    from azhip import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    cls, cname = _lib.C4nEval, "az_c4n_eval"
    fields = [f for f, _ in cls._fields_]
    assert fields == [f for f, _ in _lib.C4Eval._fields_ if f not in ("sync", "err")] + ["n", "F"]
    body = re.search(r"typedef\s+struct\s+az_c4n_eval\s*\{(.*?)\}\s*az_c4n_eval\s*;",
                     re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S), flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == fields       # the header's own field order
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
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
    for f in fields:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f


def test_c4n_host_side_validation_without_gpu(built):
    """az_c4n_eval_fwd and the trunk entry points check their arguments on the host before any
    HIP call: a null descriptor, B outside 1..max_B, n = 7 (with a pointer to az_c4_eval_fwd),
    other bad n / A / F and null pointers return AZ_EINVAL with a message."""
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
    call = lambda d, B, v=None: L.az_c4n_eval_fwd(  # noqa: E731
        ctypes.byref(d) if d is not None else None, None, B, None, v, None, None, None)
    assert call(None, 1) == AZ_EINVAL
    assert b"null descriptor" in L.az_last_error()

    def desc(**kw):
        d = _lib.C4nEval()
        d.max_B, d.n, d.A, d.F = 4, 5, 6, 1600
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    assert call(desc(), 0) == AZ_EINVAL
    assert b"B=0" in L.az_last_error()
    assert call(desc(), 5) == AZ_EINVAL
    assert b"max_B" in L.az_last_error()
    assert call(desc(n=7, F=3136), 1) == AZ_EINVAL
    assert b"n=7" in L.az_last_error() and b"az_c4_eval_fwd" in L.az_last_error()
    for kw, word in ((dict(n=9, F=64 * 81), b"n=9"), (dict(n=3, F=576), b"n=3"),
                     (dict(A=33), b"A=33"), (dict(A=0), b"A=0"), (dict(F=1664), b"F=1664")):
        assert call(desc(**kw), 1) == AZ_EINVAL
        assert word in L.az_last_error(), word
    assert call(desc(), 1) == AZ_EINVAL
    assert b"neither v nor gv" in L.az_last_error()
    v = (ctypes.c_float * 4)()
    assert call(desc(), 1, ctypes.cast(v, ctypes.c_void_p)) == AZ_EINVAL
    assert b"null" in L.az_last_error()
    for n in (3, 7, 9):
        assert L.az_c4n_eval_ws_bytes(4, n, 6) == 0
    assert L.az_c4n_eval_ws_bytes(4, 5, 33) == 0 and L.az_c4n_eval_ws_bytes(0, 5, 6) == 0
    for n in (4, 5, 6, 8):
        assert L.az_c4n_eval_ws_bytes(8, n, n + 1) == \
            L.az_transform_heads_ws_bytes(8, 64 * n * n, n + 1) > 0
    assert L.az_c4n_trunk_fwd(None, 0, 5, *[None] * 6) == 0
    assert L.az_c4n_trunk_fwd(None, 1, 7, *[None] * 6) == AZ_EINVAL
    assert b"n=7" in L.az_last_error()
    assert L.az_c4n_trunk_fwd(None, 1, 5, *[None] * 6) == AZ_EINVAL
    assert b"null" in L.az_last_error()
    heads_args = [None] * 6 + [6] + [None] * 7
    assert L.az_c4n_trunk_heads_fwd(None, 0, 5, *heads_args) == 0
    assert L.az_c4n_trunk_heads_fwd(None, 1, 5, *heads_args) == AZ_EINVAL
    assert b"null" in L.az_last_error()
    heads_args[6] = 40
    assert L.az_c4n_trunk_heads_fwd(None, 1, 5, *heads_args) == AZ_EINVAL
    assert b"A=40" in L.az_last_error()


def test_is_c4n_is_true_exactly_for_the_covered_boards():
    """_is_c4n: Connect4Net on n in {4, 5, 6, 8}; 7 keeps az_c4_eval_fwd, other n the eager path,
    and a TicTacToeNet of a covered side is not a Connect4 board."""
    from azhip import nets, ops, wrappers
    assert tuple(ops.C4N_SIDES) == (4, 5, 6, 8)

    def fake(cls, n):
        net = cls.__new__(cls)
        net.n = n
        return SimpleNamespace(nnet=net)

    for n in range(1, 12):
        w = fake(nets.Connect4Net, n)
        assert wrappers._is_c4n(w) == (n in (4, 5, 6, 8)), n
        assert not (wrappers._is_c4n(w) and wrappers._is_c4(w))
        assert not wrappers._is_c4n(fake(nets.TicTacToeNet, n))
    assert wrappers._is_c4(fake(nets.Connect4Net, 7))
