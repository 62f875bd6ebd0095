"""CPU checks of the az_c4r_* boundary (Connect4 on the rectangular boards 7x6, 6x5, 5x4 and 8x7):
the header and the ctypes binding declare the same entry points with the same signatures, the
ctypes mirror of az_c4r_eval has the layout a C compiler gives the header's struct, the host-side
argument checks of the entry points, and which boards the wrappers route where -- in particular
that a 7-column board which is not 7 rows high never counts as the 7x7 board."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

from conftest import ROOT
from test_c4n_eval_abi import _header_signature

HEADER = os.path.join(ROOT, "include", "az_hip.h")
NAMES = ("az_c4r_trunk_fwd", "az_c4r_trunk_heads_fwd", "az_c4r_eval_ws_bytes", "az_c4r_eval_fwd")
SHAPES = ((7, 6), (6, 5), (5, 4), (8, 7))


@pytest.fixture(scope="module")
def built():
    from azhip.build import build
    return build(verbose=False)


def test_header_and_binding_declare_the_same_signatures():
    from azhip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+az_c4r_eval\s*\{", src)
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
    assert _lib.SIGNATURES["az_c4r_eval_fwd"][1][0] is ctypes.POINTER(_lib.C4rEval)
    assert re.search(r"#define\s+AZ_ABI_VERSION\s+2\b", src)   # additive: the version stays 2


def test_c4r_eval_layout_matches_header(built, tmp_path):
    """Field order, every field offset and the size of _lib.C4rEval equal what a C compiler makes
    of az_c4r_eval: az_c4n_eval's fields with nx, ny in place of n."""
    import shutil
    import subprocess
    from azhip import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    cls, cname = _lib.C4rEval, "az_c4r_eval"
    fields = [f for f, _ in cls._fields_]
    c4n = [f for f, _ in _lib.C4nEval._fields_]
    assert fields == c4n[:c4n.index("n")] + ["nx", "ny"] + c4n[c4n.index("n") + 1:]
    body = re.search(r"typedef\s+struct\s+az_c4r_eval\s*\{(.*?)\}\s*az_c4r_eval\s*;",
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


def test_c4r_host_side_validation_without_gpu(built):
    """az_c4r_eval_fwd and the trunk entry points check their arguments on the host before any
    HIP call: a null descriptor, B outside 1..max_B, a square (n, n) (with the name of the
    evaluator that owns it), a transposed or unknown shape, bad A / F and null pointers return
    AZ_EINVAL with a message."""
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
    call = lambda d, B, v=None: L.az_c4r_eval_fwd(  # noqa: E731
        ctypes.byref(d) if d is not None else None, None, B, None, v, None, None, None)
    assert call(None, 1) == AZ_EINVAL
    assert b"null descriptor" in L.az_last_error()

    def desc(**kw):
        d = _lib.C4rEval()
        d.max_B, d.nx, d.ny, d.A, d.F = 4, 7, 6, 8, 2688
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    assert call(desc(), 0) == AZ_EINVAL
    assert b"B=0" in L.az_last_error()
    assert call(desc(), 5) == AZ_EINVAL
    assert b"max_B" in L.az_last_error()
    assert call(desc(ny=7, F=3136), 1) == AZ_EINVAL
    assert b"nx=7 ny=7" in L.az_last_error() and b"az_c4_eval_fwd's" in L.az_last_error()
    for n in (4, 5, 6, 8):
        assert call(desc(nx=n, ny=n, A=n + 1, F=64 * n * n), 1) == AZ_EINVAL
        assert b"nx=%d ny=%d" % (n, n) in L.az_last_error()
        assert b"az_c4n_eval_fwd's" in L.az_last_error()
    for kw, word in ((dict(nx=6, ny=7, A=7), b"nx=6 ny=7"), (dict(nx=4, ny=6, F=1536), b"nx=4 ny=6"),
                     (dict(nx=9, ny=9, F=64 * 81), b"nx=9 ny=9"), (dict(nx=7, ny=5), b"ny=5"),
                     (dict(A=33), b"A=33"), (dict(A=0), b"A=0"), (dict(F=2752), b"F=2752")):
        assert call(desc(**kw), 1) == AZ_EINVAL
        assert word in L.az_last_error(), word
    assert call(desc(), 1) == AZ_EINVAL
    assert b"neither v nor gv" in L.az_last_error()
    v = (ctypes.c_float * 4)()
    assert call(desc(), 1, ctypes.cast(v, ctypes.c_void_p)) == AZ_EINVAL
    assert b"null" in L.az_last_error()
    for nx, ny in ((7, 7), (6, 7), (5, 5), (4, 6), (9, 7), (0, 0)):
        assert L.az_c4r_eval_ws_bytes(4, nx, ny, nx + 1) == 0
    assert L.az_c4r_eval_ws_bytes(4, 7, 6, 33) == 0 and L.az_c4r_eval_ws_bytes(0, 7, 6, 8) == 0
    for nx, ny in SHAPES:
        assert L.az_c4r_eval_ws_bytes(8, nx, ny, nx + 1) == \
            L.az_transform_heads_ws_bytes(8, 64 * nx * ny, nx + 1) > 0
    assert L.az_c4r_trunk_fwd(None, 0, 7, 6, *[None] * 6) == 0
    assert L.az_c4r_trunk_fwd(None, 1, 7, 7, *[None] * 6) == AZ_EINVAL
    assert b"nx=7 ny=7" in L.az_last_error()
    assert L.az_c4r_trunk_fwd(None, 1, 6, 7, *[None] * 6) == AZ_EINVAL
    assert b"nx=6 ny=7" in L.az_last_error()
    assert L.az_c4r_trunk_fwd(None, 1, 7, 6, *[None] * 6) == AZ_EINVAL
    assert b"null" in L.az_last_error()
    heads_args = [None] * 6 + [8] + [None] * 7
    assert L.az_c4r_trunk_heads_fwd(None, 0, 7, 6, *heads_args) == 0
    assert L.az_c4r_trunk_heads_fwd(None, 1, 7, 6, *heads_args) == AZ_EINVAL
    assert b"null" in L.az_last_error()
    heads_args[6] = 40
    assert L.az_c4r_trunk_heads_fwd(None, 1, 7, 6, *heads_args) == AZ_EINVAL
    assert b"A=40" in L.az_last_error()


def test_routing_predicates_go_by_both_extents():
    """_is_c4 / _is_c4n / _is_c4r are mutually exclusive; 7 columns x 6 rows is az_c4r's, never
    the 7x7 MFMA trunk's; transposed and other shapes take no fused route; Connect4Net.route says
    the same."""
    from azhip import nets, ops, wrappers
    assert tuple(ops.C4R_SHAPES) == SHAPES

    def fake(cls, x, y):
        net = cls.__new__(cls)
        net.n, net.board_x, net.board_y = x, x, y
        return SimpleNamespace(nnet=net)

    for x in range(1, 11):
        for y in range(1, 11):
            w = fake(nets.Connect4Net, x, y)
            flags = (wrappers._is_c4(w), wrappers._is_c4n(w), wrappers._is_c4r(w))
            assert sum(flags) <= 1, (x, y)
            assert flags[0] == ((x, y) == (7, 7)), (x, y)
            assert flags[1] == (x == y and x in (4, 5, 6, 8)), (x, y)
            assert flags[2] == ((x, y) in SHAPES), (x, y)
            want = "c4" if flags[0] else "c4n" if flags[1] else "c4r" if flags[2] else "eager"
            assert w.nnet.route == want, (x, y)
            assert not wrappers._is_c4r(fake(nets.TicTacToeNet, x, y))
    w76 = fake(nets.Connect4Net, 7, 6)
    assert not wrappers._is_c4(w76) and w76.nnet.route == "c4r"


def test_spec_takes_a_shape_and_keeps_the_square_forms():
    from azhip.weights import connect4_net_spec
    assert connect4_net_spec(7) == connect4_net_spec((7, 7)) == connect4_net_spec()
    assert connect4_net_spec(5, 6) == connect4_net_spec((5, 5), 6) == connect4_net_spec(n=5)
    spec = dict(connect4_net_spec((7, 6)))
    assert spec["fc_policy.weight"] == (8, 2688) and spec["fc_value.weight"] == (1, 2688)
    assert dict(connect4_net_spec((4, 6)))["fc_policy.weight"] == (5, 1536)
    assert dict(connect4_net_spec((6, 7)))["fc_policy.weight"] == (7, 2688)
