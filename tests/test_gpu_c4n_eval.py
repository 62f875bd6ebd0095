"""az_c4n_eval_fwd, the one-call Connect4 evaluator for 4x4, 5x5, 6x6 and 8x8 boards, on the
MI355X: the fused trunk against the two conv launches, the heads formed from its LDS tile, the
evaluator against the eager path (bit for bit), row invariance of batches of <= 8, float64
parity, the wrapper routes, the arena with and without speculative leaf batches, the lock-step
route and argument validation.

F = 64 n^2 is 1024 / 1600 / 2304 / 4096: n = 5 ends in a partial 256-column heads chunk, n = 8
(A = 9) takes the 16-wide heads, and the output_transform GEMVs of <= 8 rows take the whole-K
kernel, gemv_rows (n = 6, >= 3 rows) or the chunked kernel (n = 8 and n = 5 at >= 5 rows)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import assert_close, report

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIDES = (4, 5, 6, 8)
TOL = 1e-5
MAX_B = 70


def _boards(n, B, seed):
    b = np.random.default_rng(seed).integers(-1, 2, size=(B, n, n)).astype(np.int8)
    b[0] = 0                                   # empty board
    if B > 1:
        b[1] = 1                               # a full board
    return b


_NETS, _EAGER, _EVALS = {}, {}, {}


def _nets(n):
    """(Connect4Net, PolicyValueGNN) in eval mode, torch default init under a fixed seed, built
    once per n.  The GNN has no message-passing layers: a per-row evaluation only runs
    output_transform (gnn_utils.py:35-36)."""
    if n not in _NETS:
        from azhip import nets
        torch.manual_seed(4000 + n)
        game = SimpleNamespace(getBoardSize=lambda: (n, n), getActionSize=lambda: n + 1)
        nnet = nets.Connect4Net(game, {"dropout": 0.0}).eval()
        gnn = nets.PolicyValueGNN(nnet.feature_dim, 0).eval()
        _NETS[n] = (nnet, gnn)
    return _NETS[n]


def _eager(n, B):
    """Today's eager calls on _boards(n, B): az_conv3x3_relu_fwd x 2, az_heads_fwd and
    az_transform_heads_fwd(y = NULL); computed once and shared."""
    if (n, B) not in _EAGER:
        from azhip import nets
        nnet, gnn = _nets(n)
        b = torch.from_numpy(_boards(n, B, 100 * n + B)).to(nnet.params.device)
        f = nnet.features_eager(b)
        logp, pi, v = nnet.heads(f)
        _, gpi, gv = nets.gnn_per_row_heads(nnet, gnn, f)
        torch.cuda.synchronize()
        _EAGER[(n, B)] = SimpleNamespace(b=b, feat=f, logp=logp, pi=pi, v=v, gpi=gpi, gv=gv)
    return _EAGER[(n, B)]


def _evaluator(n, max_B=MAX_B):
    """(C4nEval for max_B boards, its four output tensors), one per (n, max_B)."""
    if (n, max_B) not in _EVALS:
        from azhip import ops
        nnet, gnn = _nets(n)
        dev = nnet.params.device
        ev = ops.C4nEval(nnet.params, gnn.params, n, n + 1, max_B, dev)
        outs = [torch.empty((max_B, n + 1) if i % 2 == 0 else (max_B,), device=dev)
                for i in range(4)]
        _EVALS[(n, max_B)] = (ev, outs)
    return _EVALS[(n, max_B)]


def _run(n, b, B, kind, max_B=MAX_B):
    """One az_c4n_eval_fwd call of `kind` with every scratch and output NaN before it -> the four
    outputs as numpy (None where the kind has none); rows B.. must stay NaN."""
    from azhip import ops
    ev, outs = _evaluator(n, max_B)
    use = [kind != "gnn", kind != "gnn", kind != "std", kind != "std"]
    for t in (ev.feat, ev.hidden, ev.logp, ev.glogp, *outs):
        t.fill_(float("nan"))
    ops.c4n_eval(ev, b, B, *[o if u else None for o, u in zip(outs, use)])
    torch.cuda.synchronize()
    got = []
    for o, u in zip(outs, use):
        a = o.cpu().numpy()
        assert np.isnan(a[B if u else 0:]).all(), (n, B, kind)
        got.append(a[:B].copy() if u else None)
    return got


@pytest.mark.parametrize("n", SIDES)
def test_fused_trunk_equals_two_conv_calls(n):
    """az_c4n_trunk_fwd against az_conv3x3_relu_fwd x 2, torch.equal, at 1 and 3 boards (the empty
    and a full board among them); Connect4Net.features takes the fused kernel."""
    from azhip import ops
    nnet, _ = _nets(n)
    for B in (1, 3):
        e = _eager(n, B)
        got = torch.full((B, 64 * n * n), float("nan"), device=e.b.device)
        ops.c4n_trunk(e.b, nnet.params, out=got)
        assert torch.equal(got, e.feat), (n, B)
        assert torch.equal(nnet.features(e.b), e.feat), (n, B)


@pytest.mark.parametrize("n", SIDES)
def test_heads_from_the_lds_tile_equal_az_heads_fwd(n):
    """az_c4n_trunk_heads_fwd at 3 boards: feat, logp, pi, v torch.equal to features_eager +
    ops.heads (n = 5: the partial last chunk; n = 8: A = 9, the 16-wide heads)."""
    from azhip import ops
    nnet, _ = _nets(n)
    e = _eager(n, 3)
    feat, logp, pi, v = ops.c4n_trunk_heads(e.b, nnet.params)
    for name, got, ref in (("feat", feat, e.feat), ("logp", logp, e.logp), ("pi", pi, e.pi),
                           ("v", v, e.v)):
        assert torch.equal(got, ref), (n, name)
    f2, l2, p2, v2 = nnet.features_heads(e.b)
    assert torch.equal(f2, e.feat) and torch.equal(l2, e.logp) and torch.equal(p2, e.pi) \
        and torch.equal(v2, e.v)


@pytest.mark.parametrize("kind", ["std", "gnn", "both"])
@pytest.mark.parametrize("n", SIDES)
def test_eval_equals_eager_bit_for_bit(n, kind):
    """az_c4n_eval_fwd against the eager calls at the same B: 1, 9 (MFMA tiles) and 70 (the
    M > 64 GEMM dispatch; A <= 8 also crosses into the composed heads, A = 9 keeps the y form)."""
    for B in (1, 9, 70):
        e = _eager(n, B)
        ref = [x.cpu().numpy() for x in (e.pi, e.v, e.gpi, e.gv)]
        got = _run(n, e.b, B, kind)
        for k, g in enumerate(got):
            if g is not None:
                assert np.array_equal(g, ref[k]), (n, B, kind, k)


@pytest.mark.parametrize("n", SIDES)
def test_rows_of_small_batches_are_batch1_bits(n):
    """Every row of a batch of 2, 3, 5 and 8 boards equals that board's B = 1 call, bit for bit,
    all four outputs."""
    e = _eager(n, 8)
    one = [_run(n, e.b[i:i + 1].contiguous(), 1, "both") for i in range(8)]
    for B in (2, 3, 5, 8):
        got = _run(n, e.b, B, "both")
        for i in range(B):
            for k in range(4):
                assert np.array_equal(got[k][i], one[i][k][0]), (n, B, i, k)


def _float64_reference(boards, W, G):
    """Connect4Net.forward and the per-row GNN tail restated on the CPU in float64."""
    import torch.nn.functional as Fn
    t = lambda d, k: d[k].detach().cpu().double()  # noqa: E731
    x = torch.from_numpy(boards).double()[:, None]
    x = Fn.relu(Fn.conv2d(x, t(W, "conv1.weight"), t(W, "conv1.bias"), padding=1))
    x = Fn.relu(Fn.conv2d(x, t(W, "conv2.weight"), t(W, "conv2.bias"), padding=1))
    f = x.flatten(1)

    def heads(f):
        pi = torch.softmax(Fn.linear(f, t(W, "fc_policy.weight"), t(W, "fc_policy.bias")), 1)
        v = torch.tanh(Fn.linear(f, t(W, "fc_value.weight"), t(W, "fc_value.bias")))[:, 0]
        return [pi.numpy(), v.numpy()]

    y = Fn.linear(Fn.relu(Fn.linear(f, t(G, "output_transform.0.weight"),
                                    t(G, "output_transform.0.bias"))),
                  t(G, "output_transform.2.weight"), t(G, "output_transform.2.bias"))
    return heads(f) + heads(y)


@pytest.mark.parametrize("n", SIDES)
def test_eval_matches_float64_restatement(n):
    """The evaluator at 8 and 70 boards against a float64 torch-CPU restatement of the network
    (conv2d x 2, the heads, output_transform): |d pi| and |d v| <= 1e-5, margins printed."""
    nnet, gnn = _nets(n)
    for B in (8, 70):
        e = _eager(n, B)
        ref = _float64_reference(e.b.cpu().numpy(), nnet.params, gnn.params)
        got = _run(n, e.b, B, "both")
        errs = [float(np.abs(g.astype(np.float64) - r).max()) for g, r in zip(got, ref)]
        print(f"c4n_eval/n{n}/B{B}: max err pi {errs[0]:.3g} v {errs[1]:.3g} "
              f"gnn pi {errs[2]:.3g} gnn v {errs[3]:.3g}  "
              f"margin {TOL / max(max(errs), 1e-300):.1f}x")
        for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
            assert_close(f"c4n_eval/n{n}/B{B}/{name}", got[k], ref[k], TOL)


# Lock-step self-play batch sizes per board side (derived from the GEMM dispatch for 256 CUs and
# the widths' table in tests/test_gpu_gemm_widths.py): a 256 x 128 split-K size and a stream-K
# size of F = 64 n^2; the second evaluator per n is sized for the larger one
LOCKSTEP_B = {4: (257, 2049), 5: (257, 1025), 6: (257, 769), 8: (257, 513)}


@pytest.mark.parametrize("n,B", [(n, B) for n in SIDES for B in LOCKSTEP_B[n]])
def test_eval_at_lockstep_batch_sizes(n, B):
    """The evaluator at hundreds to thousands of boards (its own C4nEval of max_B = the stream-K
    size, so the MAX_B = 70 evaluator's workspace and plans above stay as they are): pi, v, gpi
    and gv within 1e-5 of the float64 restatement and np.array_equal to the eager path; rows
    B..max_B stay NaN (_run); the empty and the full board are rows 0 and 1."""
    nnet, gnn = _nets(n)
    max_B = LOCKSTEP_B[n][1]
    e = _eager(n, B)
    ref = _float64_reference(e.b.cpu().numpy(), nnet.params, gnn.params)
    eager = [x.cpu().numpy() for x in (e.pi, e.v, e.gpi, e.gv)]
    got = _run(n, e.b, B, "both", max_B)
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"c4n_eval/n{n}/B{B}/{name}", got[k], ref[k], TOL)
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert np.array_equal(got[k], eager[k]), (n, B, name)


def _wrapper(n, gnn=True, seed=0):
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Game import Connect4Game
    from connect4.Connect4Net import Connect4NNetWrapper
    torch.manual_seed(5000 + 10 * n + seed)
    cls = Connect4GNNWrapper if gnn else Connect4NNetWrapper
    return cls(Connect4Game(n), SimpleNamespace(gnn_layers=1, dropout=0.3))


def test_wrappers_take_the_one_call_routes():
    """Connect4GNNWrapper on 5x5 and Connect4NNetWrapper on 6x6: predict / predict_with_gnn /
    predict_both run _C4nBatch1Direct and equal the eager path; batch_invariant_rows is 8; a 7x7
    wrapper built in the same process still gets _Batch1Direct."""
    from azhip import nets, wrappers
    w = _wrapper(5)
    assert wrappers._is_c4n(w) and w.batch_invariant_rows == 8
    boards = _boards(5, 8, 77).astype(np.int64)
    pi, v = w.predict(boards[3])
    gpi, gv = w.predict_with_gnn(boards[3])
    both = w.predict_both(boards)
    for kind in ("std", "gnn", "both"):
        assert type(w._g1[kind]) is wrappers._C4nBatch1Direct, kind
    assert w._g1["both"].cap == 8 and w._g1["std"].cap == 1
    b = nets.boards_to_device(boards, w.device)
    f = w.nnet.features_eager(b)
    _, rpi, rv = w.nnet.heads(f)
    _, rgpi, rgv = nets.gnn_per_row_heads(w.nnet, w.gnn, f)
    ref = [x.cpu().numpy() for x in (rpi, rv, rgpi, rgv)]
    for k, got in enumerate((pi, v, gpi, gv)):
        assert np.array_equal(np.asarray(got), ref[k][3]), k
    for k in range(4):
        assert np.array_equal(np.asarray(both[k]), ref[k]), k
    c = _wrapper(6, gnn=False)
    b6 = _boards(6, 4, 78).astype(np.int64)
    cpi, cv = c.predict(b6[2])
    assert type(c._g1["std"]) is wrappers._C4nBatch1Direct
    f6 = c.nnet.features_eager(nets.boards_to_device(b6, c.device))
    _, rpi6, rv6 = c.nnet.heads(f6)
    assert np.array_equal(cpi, rpi6.cpu().numpy()[2]) and cv == rv6.cpu().numpy()[2]
    w7 = _wrapper(7)
    w7.predict(_boards(7, 1, 79)[0].astype(np.int64))
    w7.predict_both(_boards(7, 2, 80).astype(np.int64))
    assert type(w7._g1["std"]) is wrappers._Batch1Direct
    assert type(w7._g1["both"]) is wrappers._Batch1Direct


@pytest.mark.parametrize("var,val", [("AZ_B1_MODE", "graph"), ("AZ_NO_ZEROCOPY", "1")])
def test_environment_keeps_the_graph_routes(monkeypatch, var, val):
    """AZ_B1_MODE=graph and AZ_NO_ZEROCOPY=1 select the hipGraph / pinned-ring routes as before:
    no row-invariance promise, the same bits as the one-call route."""
    from azhip import wrappers
    direct = _wrapper(5)
    boards = _boards(5, 12, 21).astype(np.int64)
    ref1 = direct.predict(boards[5]) + direct.predict_with_gnn(boards[5])
    ref = direct.predict_both_async(boards).result()
    monkeypatch.setenv(var, val)
    w = _wrapper(5)
    assert w.batch_invariant_rows == 0
    got1 = w.predict(boards[5]) + w.predict_with_gnn(boards[5])
    assert isinstance(w._g1["std"], wrappers._Batch1Graph)
    assert isinstance(w._g1["gnn"], wrappers._Batch1Graph)
    pend = w.predict_both_async(boards)
    assert isinstance(pend, wrappers.PendingPrediction)
    for a, b in zip(got1 + pend.result(), ref1 + ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_arena_speculative_batches_equal_batch1_c4n():
    """Connect4 5x5 arena, GNN wrappers, 4 games at 25 simulations: speculative leaf batches
    (<= 8 boards, A = 6) play exactly the games of batch-1 leaves and serve some leaves from
    their rows."""
    from Arena import Arena
    from connect4.Connect4Game import Connect4Game
    from mcts_native import ArenaPlayer
    game = Connect4Game(5)
    args = SimpleNamespace(numMCTSSims=25, cpuct=1.0, use_gnn=True, gnn_layers=1)
    w, other = _wrapper(5, seed=1), _wrapper(5, seed=2)
    res, calls = [], []
    for prefetch in (False, True):
        np.random.seed(7)
        p1 = ArenaPlayer(game, w, args, prefetch=prefetch)
        p2 = ArenaPlayer(game, other, args, prefetch=prefetch)
        assert p1.spec == (8 if prefetch else 0)
        moves = []

        def rec(p):
            def f(x):
                a = p(x)
                moves.append((np.asarray(x).tobytes(), a))
                return a
            return f
        wld = Arena(rec(p1), rec(p2), game).playGames(4)
        res.append((wld, moves))
        calls.append((p1.calls + p2.calls, p1.hits + p2.hits))
    report("c4n_eval/arena_speculative_calls", batch1=calls[0], speculative=calls[1],
           wld=list(res[0][0]))
    assert res[0] == res[1]
    assert calls[1][1] > 0 and calls[1][0] + calls[1][1] == calls[0][0]


def test_lockstep_route_two_streams():
    """6x6: predict_both_async on two streams, 5 and 300 boards in flight together, read in
    reverse order: each equals the synchronous eager path; the per-stream evaluators are
    _C4nDirectBatch."""
    from azhip import nets, wrappers
    w = _wrapper(6)
    dev = w.device
    pool = _boards(6, 305, 31)
    sets = [pool[:5], pool[5:]]
    refs = []
    for s in sets:
        f = w.nnet.features_eager(nets.boards_to_device(s, dev))
        _, pi, v = w.nnet.heads(f)
        _, gpi, gv = nets.gnn_per_row_heads(w.nnet, w.gnn, f)
        refs.append([x.cpu().numpy() for x in (pi, v, gpi, gv)])
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    pend = [w.predict_both_async(b, stream=s) for b, s in zip(sets, (s1, s2))]
    assert all(isinstance(p, wrappers._PendingDirect) for p in pend)
    assert len(w._directs) == 2
    assert all(type(d) is wrappers._C4nDirectBatch for d in w._directs.values())
    for p, ref in reversed(list(zip(pend, refs))):
        for a, b in zip(p.result(), ref):
            assert np.array_equal(a, b)
    for a, b in zip(w.predict_both(sets[0]), refs[0]):       # the synchronous route, 5 rows
        assert np.array_equal(np.asarray(a), b)
    # the CNN-only wrapper takes the same route for predict_batch_async (no GNN tail, no workspace)
    c = _wrapper(6, gnn=False)
    c.nnet.params.copy_flat_(w.nnet.params.flat)
    pi, v, gpi, gv = c.predict_batch_async(sets[1]).result()
    assert gpi is None and gv is None
    assert np.array_equal(pi, refs[1][0]) and np.array_equal(v, refs[1][1])
    assert type(next(iter(c._directs.values()))) is wrappers._C4nDirectBatch


def test_validation_returns_einval_before_any_launch():
    """B = 0, B > max_B, n = 7, n = 9, F off by 64, A = 33 and a null weight pointer: AZ_EINVAL
    with the naming word in az_last_error, and nothing is launched (the NaN-filled outputs and
    scratch stay NaN); a valid call afterwards succeeds."""
    from azhip import _lib, ops
    nnet, gnn = _nets(5)
    dev = nnet.params.device
    L = _lib.lib()
    ev = ops.C4nEval(nnet.params, gnn.params, 5, 6, 4, dev)
    b = torch.from_numpy(_boards(5, 8, 1)).to(dev)
    outs = [torch.empty((4, 6), device=dev), torch.empty((4,), device=dev),
            torch.empty((4, 6), device=dev), torch.empty((4,), device=dev)]
    watched = [ev.feat, ev.hidden, ev.logp, ev.glogp, *outs]
    for t in watched:
        t.fill_(float("nan"))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(desc, B):
        return L.az_c4n_eval_fwd(ctypes.byref(desc), P(b), B, *[P(o) for o in outs], None)

    def copy(**kw):
        d = _lib.C4nEval()
        ctypes.memmove(ctypes.byref(d), ctypes.byref(ev.desc), ctypes.sizeof(d))
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    cases = ((ev.desc, 0, b"B=0"), (ev.desc, 5, b"max_B"), (copy(n=7, F=3136), 1, b"n=7"),
             (copy(n=9, F=64 * 81), 1, b"n=9"), (copy(F=1664), 1, b"F=1664"),
             (copy(A=33), 1, b"A=33"), (copy(fc_value_w=None), 1, b"null"))
    got = []
    # az_last_error is per thread: the rejected calls run on a thread of their own, so this
    # process's main thread keeps the empty message tests/test_lib_abi.py expects
    import threading
    t = threading.Thread(target=lambda: got.extend(
        (call(desc, B), bytes(L.az_last_error())) for desc, B, _ in cases))
    t.start()
    t.join()
    assert len(got) == len(cases)
    for (rc, msg), (_, _, word) in zip(got, cases):
        assert rc == -1 and word in msg, (word, rc, msg)
    assert b"az_c4_eval_fwd" in got[2][1]
    torch.cuda.synchronize()
    for t in watched:
        assert torch.isnan(t).all()
    assert call(ev.desc, 4) == 0
    torch.cuda.synchronize()
    assert not any(torch.isnan(o).any() for o in outs)
