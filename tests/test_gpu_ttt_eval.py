"""az_ttt_eval_fwd, the one-call TicTacToe evaluator, on the MI355X: the fused trunk against the
three conv launches, the evaluator against the eager path (bit for bit), row invariance of
batches of <= 8, reference parity on the new route, the arena with and without speculative leaf
batches, the lock-step route and argument validation."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import assert_close, golden, report, split_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
BATCHES = (1, 2, 7, 8, 9, 33, 257)
MAX_B = 260


def _state_dicts(n):
    """(CNN, GNN) weights: the goldens' for n = 3 / 4, PCG64 streams for n = 5."""
    from azhip.weights import gnn_spec, synthetic_state_dict, tictactoe_net_spec
    if n == 3:
        z = golden("ttt3.npz")
        return split_weights(z, "w/"), split_weights(z, "g/")
    if n == 4:
        z = golden("ttt4.npz")
        return (synthetic_state_dict(tictactoe_net_spec(4), int(z["seed_cnn"])),
                synthetic_state_dict(gnn_spec(512, 2), int(z["seed_gnn"])))
    return (synthetic_state_dict(tictactoe_net_spec(5), 51),
            synthetic_state_dict(gnn_spec(1152, 2), 52))


def _boards(n, B, seed):
    b = np.random.default_rng(seed).integers(-1, 2, size=(B, n, n)).astype(np.int8)
    b[0] = 0                                   # empty board
    if B > 1:
        b[1] = 1                               # full boards
    if B > 2:
        b[2] = -1
    return b


_NETS = {}


def _nets(n):
    """(TicTacToeNet, PolicyValueGNN) in eval mode with _state_dicts(n), built once per n."""
    if n not in _NETS:
        from azhip import nets
        W, G = _state_dicts(n)
        game = SimpleNamespace(getBoardSize=lambda: (n, n), getActionSize=lambda: n * n + 1)
        nnet = nets.TicTacToeNet(game, {}, init=W).eval()
        gnn = nets.PolicyValueGNN(nnet.feature_dim, 2, init=G).eval()
        _NETS[n] = (nnet, gnn)
    return _NETS[n]


def _wrapper(n):
    """TicTacToeGNNWrapper on an n x n board with _state_dicts(n)."""
    from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    W, G = _state_dicts(n)
    w = TicTacToeGNNWrapper(TicTacToeGame(n), SimpleNamespace(gnn_layers=2))
    w.nnet.load_state_dict(W)
    w.gnn.load_state_dict(G)
    return w


@pytest.mark.parametrize("n", [3, 4, 5])
def test_fused_trunk_equals_three_conv_calls(n):
    """az_ttt_trunk_fwd against az_conv3x3_relu_fwd x 3, torch.equal, at every batch size of
    the set (one block per board: 1 .. 257 blocks), boards on the device and in mapped host
    memory."""
    from azhip import ops
    nnet, _ = _nets(n)
    dev = nnet.params.device
    for B in BATCHES:
        b = torch.from_numpy(_boards(n, B, 100 * n + B)).to(dev)
        ref = nnet.features_eager(b)
        got = nnet.features(b)
        assert got.shape == (B, 128 * (n - 2) ** 2)
        assert torch.equal(got, ref), (n, B)
    hb = ops.HostBuffer(1024)
    hv = hb.view(0, torch.int8, (9, n, n))
    hv.numpy()[...] = _boards(n, 9, 7)
    out = torch.full((9, 128 * (n - 2) ** 2), float("nan"), device=dev)
    ops.ttt_trunk(hv, nnet.params, out=out)
    assert torch.equal(out, nnet.features_eager(hv.to(dev)))


@pytest.mark.parametrize("n", [3, 4, 5])
def test_eval_equals_eager_bit_for_bit(n):
    """az_ttt_eval_fwd against features_eager -> heads and gnn_per_row_heads: pi, v, gpi, gv with
    np.array_equal for std / gnn / both, outputs in device tensors and in HostBuffer views, every
    scratch and output buffer NaN before the call, rows B..max_B untouched."""
    from azhip import nets, ops
    nnet, gnn = _nets(n)
    dev = nnet.params.device
    A = n * n + 1
    ev = ops.TttEval(nnet.params, gnn.params, n, A, MAX_B, dev)
    sizes = (MAX_B * A, MAX_B, MAX_B * A, MAX_B)
    off = np.concatenate([[0], np.cumsum([(4 * s + 255) // 256 * 256 for s in sizes])])
    hb = ops.HostBuffer(int(off[-1]))
    host = [hb.view(int(off[i]), torch.float32, (MAX_B, A) if i % 2 == 0 else (MAX_B,))
            for i in range(4)]
    devo = [torch.empty((MAX_B, A) if i % 2 == 0 else (MAX_B,), device=dev) for i in range(4)]
    nan = float("nan")
    for B in BATCHES:
        b = torch.from_numpy(_boards(n, B, 10 * n + B)).to(dev)
        f = nnet.features_eager(b)
        _, pi, v = nnet.heads(f)
        _, gpi, gv = nets.gnn_per_row_heads(nnet, gnn, f)
        ref = [x.cpu().numpy() for x in (pi, v, gpi, gv)]
        for kind in ("std", "gnn", "both"):
            use = [kind != "gnn", kind != "gnn", kind != "std", kind != "std"]
            for outs in (devo, host):
                for t in (ev.feat, ev.h1, ev.h2, ev.hidden, ev.y, ev.logp, ev.glogp, *outs):
                    t.fill_(nan)
                ops.ttt_eval(ev, b, B, *[o if u else None for o, u in zip(outs, use)])
                torch.cuda.synchronize()
                for k, (o, u) in enumerate(zip(outs, use)):
                    got = o.cpu().numpy()
                    if u:
                        assert np.array_equal(got[:B], ref[k]), (n, B, kind, k)
                    assert np.isnan(got[B if u else 0:]).all(), (n, B, kind, k)


@pytest.mark.parametrize("n", [3, 4])
def test_rows_of_small_batches_are_batch1_bits(n):
    """batch_invariant_rows == 8: every row of predict_both on 2, 3, 5, 8 boards equals
    predict_both of that board alone, bit for bit, all four outputs."""
    w = _wrapper(n)
    assert w.batch_invariant_rows == 8
    boards = _boards(n, 8, 3).astype(np.int64)
    one = [[np.asarray(x) for x in w.predict_both(boards[i:i + 1])] for i in range(8)]
    for B in (2, 3, 5, 8):
        out = w.predict_both(boards[:B])
        for i in range(B):
            for k in range(4):
                a = np.asarray(out[k][i]).reshape(-1)
                assert np.array_equal(a, one[i][k].reshape(-1)), (n, B, i, k)


@pytest.mark.parametrize("var,val", [("AZ_B1_MODE", "graph"), ("AZ_NO_ZEROCOPY", "1")])
def test_environment_keeps_the_graph_routes(monkeypatch, var, val):
    """AZ_B1_MODE=graph and AZ_NO_ZEROCOPY=1 select the hipGraph / pinned-ring routes as before:
    no row-invariance promise, the same bits as the one-call route."""
    from azhip import wrappers
    direct = _wrapper(3)
    boards = _boards(3, 12, 21).astype(np.int64)
    ref1 = direct.predict(boards[5]) + direct.predict_with_gnn(boards[5])
    ref = direct.predict_both_async(boards).result()
    monkeypatch.setenv(var, val)
    w = _wrapper(3)
    assert w.batch_invariant_rows == 0
    got1 = w.predict(boards[5]) + w.predict_with_gnn(boards[5])
    assert isinstance(w._g1["std"], wrappers._Batch1Graph)
    pend = w.predict_both_async(boards)
    assert isinstance(pend, wrappers.PendingPrediction)
    for a, b in zip(got1 + pend.result(), ref1 + ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_ttt3_new_route_matches_reference():
    """G4 on the one-call route: positions 0::37 through batch-1 predict / predict_with_gnn and
    one predict_both of 8."""
    from azhip import wrappers
    z = golden("ttt3.npz")
    w = _wrapper(3)
    idx = np.arange(0, len(z["boards"]), 37)
    out = [[], [], [], []]
    for i in idx:
        b = z["boards"][i].astype(np.int64)
        for k, x in enumerate(w.predict(b) + w.predict_with_gnn(b)):
            out[k].append(x)
    assert isinstance(w._g1["std"], wrappers._TttBatch1Direct)
    assert isinstance(w._g1["gnn"], wrappers._TttBatch1Direct)
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"ttt_eval/ttt3/b1/{name}", np.array(out[k]), z[name][idx], TOL)
    both = w.predict_both(z["boards"][idx[:8]].astype(np.int64))
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"ttt_eval/ttt3/both8/{name}", both[k], z[name][idx[:8]], TOL)


def test_ttt4_new_route_matches_reference():
    """G4b on the one-call route: 64 boards, batch-1 calls and predict_both of 8."""
    z = golden("ttt4.npz")
    w = _wrapper(4)
    idx = np.arange(0, 2000, 2000 // 64)[:64]
    out = [[], [], [], []]
    for i in idx:
        b = z["boards"][i].astype(np.int64)
        for k, x in enumerate(w.predict(b) + w.predict_with_gnn(b)):
            out[k].append(x)
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"ttt_eval/ttt4/b1/{name}", np.array(out[k]), z[name][idx], TOL)
    both = w.predict_both(z["boards"][idx[:8]].astype(np.int64))
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"ttt_eval/ttt4/both8/{name}", both[k], z[name][idx[:8]], TOL)


def _float64_reference(boards, W, G):
    """TicTacToeNet.forward and the per-row GNN tail restated on the CPU in float64."""
    import torch.nn.functional as Fn
    t = lambda d, k: torch.from_numpy(np.asarray(d[k])).double()  # noqa: E731
    x = torch.from_numpy(boards).double()[:, None]
    x = Fn.relu(Fn.conv2d(x, t(W, "conv1.weight"), t(W, "conv1.bias"), padding=1))
    x = Fn.relu(Fn.conv2d(x, t(W, "conv2.weight"), t(W, "conv2.bias"), padding=1))
    x = Fn.relu(Fn.conv2d(x, t(W, "conv3.weight"), t(W, "conv3.bias")))
    f = x.flatten(1)

    def heads(f):
        h1 = Fn.relu(Fn.linear(f, t(W, "fc1.weight"), t(W, "fc1.bias")))
        h2 = Fn.relu(Fn.linear(f, t(W, "fc2.weight"), t(W, "fc2.bias")))
        pi = torch.softmax(Fn.linear(h1, t(W, "fc_policy.weight"), t(W, "fc_policy.bias")), 1)
        v = torch.tanh(Fn.linear(h2, t(W, "fc_value.weight"), t(W, "fc_value.bias")))[:, 0]
        return pi.numpy(), v.numpy()

    y = Fn.linear(Fn.relu(Fn.linear(f, t(G, "output_transform.0.weight"),
                                    t(G, "output_transform.0.bias"))),
                  t(G, "output_transform.2.weight"), t(G, "output_transform.2.bias"))
    return heads(f) + heads(y)


def test_ttt5_new_route_matches_float64_restatement():
    """n = 5 has no golden: the one-call route (batch-1 calls, predict_both of 8) against a
    float64 torch-CPU restatement of the network, held at the suite's 1e-5."""
    W, G = _state_dicts(5)
    w = _wrapper(5)
    boards = _boards(5, 16, 9)
    ref = _float64_reference(boards, W, G)
    out = [[], [], [], []]
    for b in boards:
        for k, x in enumerate(w.predict(b.astype(np.int64)) +
                              w.predict_with_gnn(b.astype(np.int64))):
            out[k].append(x)
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"ttt_eval/ttt5/b1/{name}", np.array(out[k]), ref[k], TOL)
    both = w.predict_both(boards[:8].astype(np.int64))
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"ttt_eval/ttt5/both8/{name}", both[k], ref[k][:8], TOL)


@pytest.mark.parametrize("B", [257, 700])
def test_ttt5_lockstep_batches_match_float64_restatement(B):
    """n = 5 at lock-step batch sizes: one az_ttt_eval_fwd call on 257 and 700 boards (fc1 / fc2
    are 1152 -> 512 and output_transform 1152 -> 1152 GEMMs on the 256 x 128 split-K tiles)
    against the float64 restatement at 1e-5, all four outputs; every scratch and output buffer
    NaN before the call, rows B.. untouched."""
    from azhip import ops
    W, G = _state_dicts(5)
    nnet, gnn = _nets(5)
    dev = nnet.params.device
    boards = _boards(5, B, 500 + B)
    ref = _float64_reference(boards, W, G)
    ev = ops.TttEval(nnet.params, gnn.params, 5, 26, B + 3, dev)
    outs = [torch.empty((B + 3, 26) if i % 2 == 0 else (B + 3,), device=dev) for i in range(4)]
    for t in (ev.feat, ev.h1, ev.h2, ev.hidden, ev.y, ev.logp, ev.glogp, *outs):
        t.fill_(float("nan"))
    ops.ttt_eval(ev, torch.from_numpy(boards).to(dev), B, *outs)
    torch.cuda.synchronize()
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        got = outs[k].cpu().numpy()
        assert np.isnan(got[B:]).all(), (B, name)
        assert_close(f"ttt_eval/ttt5/B{B}/{name}", got[:B], ref[k], TOL)


def test_arena_speculative_batches_equal_batch1_ttt():
    """TicTacToe 3x3 arena, golden GNN weights, 6 games at 25 simulations: speculative leaf
    batches play exactly the games of batch-1 leaves and serve some leaves from their rows."""
    from Arena import Arena
    from mcts_native import ArenaPlayer
    from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    game = TicTacToeGame(3)
    args = SimpleNamespace(numMCTSSims=25, cpuct=1.0, use_gnn=True, gnn_layers=2)
    w = _wrapper(3)
    torch.manual_seed(11)
    other = TicTacToeGNNWrapper(game, args)
    res, calls = [], []
    for prefetch in (False, True):
        np.random.seed(7)
        p1 = ArenaPlayer(game, w, args, prefetch=prefetch)
        p2 = ArenaPlayer(game, other, args, prefetch=prefetch)
        assert bool(p1.spec) == prefetch
        moves = []

        def rec(p):
            def f(x):
                a = p(x)
                moves.append((np.asarray(x).tobytes(), a))
                return a
            return f
        wld = Arena(rec(p1), rec(p2), game).playGames(6)
        res.append((wld, moves))
        calls.append((p1.calls + p2.calls, p1.hits + p2.hits))
    report("ttt_eval/arena_speculative_calls", batch1=calls[0], speculative=calls[1],
           wld=list(res[0][0]))
    assert res[0] == res[1]
    assert calls[1][1] > 0 and calls[1][0] + calls[1][1] == calls[0][0]


def test_lockstep_route_two_streams():
    """predict_both_async on two streams, 5 / 700 / 2,048 boards in flight together, read in
    reverse order: each equals predict_both of the same boards; a stale prediction object cannot
    hand back a ring entry a later prediction holds."""
    from azhip import wrappers
    w = _wrapper(4)
    dev = w.device
    z = golden("ttt4.npz")
    pool = np.concatenate([z["boards"], -z["boards"]]).astype(np.int8)
    sets = [pool[:5], pool[100:800], pool[900:2948]]
    refs = [w.predict_both(b) for b in sets]
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    pend = [w.predict_both_async(b, stream=s) for b, s in zip(sets, (s1, s2, s1))]
    assert all(isinstance(p, wrappers._PendingDirect) for p in pend)
    assert all(isinstance(d, wrappers._TttDirectBatch) for d in w._directs.values())
    for p, ref in reversed(list(zip(pend, refs))):
        got = p.result()
        for a, b in zip(got, ref):
            assert np.array_equal(a, np.asarray(b))
    # ownership token: the last prediction of stream 1 was read (its entry is free); a new one
    # takes that entry, and re-reading / releasing the stale object must not hand it back
    stale = pend[2]
    entry = stale.entry
    fresh = w.predict_both_async(sets[0], stream=s1)
    assert fresh.entry is entry and entry["busy"] and entry["owner"] == fresh.token
    stale.result()
    stale._release()
    assert entry["busy"] and entry["owner"] == fresh.token
    for a, b in zip(fresh.result(), refs[0]):
        assert np.array_equal(a, np.asarray(b))
    assert not entry["busy"]
    # the CNN-only wrapper takes the same route for predict_batch_async
    from tictactoe.TicTacToeNet import TicTacToeNNetWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    c = TicTacToeNNetWrapper(TicTacToeGame(4), SimpleNamespace())
    c.nnet.load_state_dict(_state_dicts(4)[0])
    pi, v, gpi, gv = c.predict_batch_async(sets[1]).result()
    assert gpi is None and gv is None
    assert np.array_equal(pi, np.asarray(refs[1][0])) and np.array_equal(v, np.asarray(refs[1][1]))
    assert isinstance(next(iter(c._directs.values())), wrappers._TttDirectBatch)


def test_validation_returns_einval_before_any_launch():
    """B = 0, B > max_B, A = 33, n = 6 and a null weight pointer: AZ_EINVAL with a message, and
    nothing is launched (the NaN-filled outputs and scratch stay NaN)."""
    from azhip import _lib, ops
    nnet, gnn = _nets(3)
    dev = nnet.params.device
    L = _lib.lib()
    ev = ops.TttEval(nnet.params, gnn.params, 3, 10, 4, dev)
    b = torch.from_numpy(_boards(3, 8, 1)).to(dev)
    outs = [torch.empty((4, 10), device=dev), torch.empty((4,), device=dev),
            torch.empty((4, 10), device=dev), torch.empty((4,), device=dev)]
    watched = [ev.feat, ev.h1, ev.h2, ev.hidden, ev.y, ev.logp, ev.glogp, *outs]
    for t in watched:
        t.fill_(float("nan"))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(desc, B):
        return L.az_ttt_eval_fwd(ctypes.byref(desc), P(b), B, *[P(o) for o in outs], None)

    def copy(**kw):
        d = _lib.TttEval()
        ctypes.memmove(ctypes.byref(d), ctypes.byref(ev.desc), ctypes.sizeof(d))
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    cases = ((ev.desc, 0, b"B=0"), (ev.desc, 5, b"max_B"), (copy(A=33), 1, b"A=33"),
             (copy(n=6), 1, b"n=6"), (copy(fc2_w=None), 1, b"null"))
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
    torch.cuda.synchronize()
    for t in watched:
        assert torch.isnan(t).all()
    assert call(ev.desc, 4) == 0
    torch.cuda.synchronize()
    assert not any(torch.isnan(o).any() for o in outs)
