"""az_c4r_eval_fwd, the one-call Connect4 evaluator for the rectangular boards 7x6 (the standard
game), 6x5, 5x4 and 8x7, on the MI355X: the fused trunk against the two conv launches, the heads
formed from its LDS tile, the evaluator against the eager path (bit for bit), row invariance of
batches of <= 8, float64 parity (which is also the orientation check: the float64 network reads the
board as a [1][cols][rows] image and flattens NCHW, so a swapped H / W or feature order cannot pass
on random boards), the lock-step batch sizes of 7x6, the wrapper routes, the arena with and without
speculative leaf batches, the lock-step route on two streams and argument validation.

F = 64 cols rows is 2688 / 1920 / 1280 / 3584: 7x6 and 6x5 end in a partial 256-column heads chunk
(10.5 and 7.5 chunks), 8x7 (A = 9) takes the 16-wide heads."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import assert_close, report

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = ((7, 6), (6, 5), (5, 4), (8, 7))
TOL = 1e-5
MAX_B = 70


def _boards(shape, B, seed):
    b = np.random.default_rng(seed).integers(-1, 2, size=(B,) + tuple(shape)).astype(np.int8)
    b[0] = 0                                   # empty board
    if B > 1:
        b[1] = 1                               # a full board
    return b


_NETS, _EAGER, _EVALS = {}, {}, {}


def _game(shape):
    return SimpleNamespace(getBoardSize=lambda: tuple(shape), getActionSize=lambda: shape[0] + 1)


def _nets(shape):
    """(Connect4Net, PolicyValueGNN) in eval mode, torch default init under a fixed seed, built
    once per shape.  The GNN has no message-passing layers: a per-row evaluation only runs
    output_transform (gnn_utils.py:35-36)."""
    if shape not in _NETS:
        from azhip import nets
        torch.manual_seed(6000 + 10 * shape[0] + shape[1])
        nnet = nets.Connect4Net(_game(shape), {"dropout": 0.0}).eval()
        assert nnet.feature_dim == 64 * shape[0] * shape[1]
        gnn = nets.PolicyValueGNN(nnet.feature_dim, 0).eval()
        _NETS[shape] = (nnet, gnn)
    return _NETS[shape]


def _eager(shape, B):
    """The eager calls on _boards(shape, B): az_conv3x3_relu_fwd x 2 (H = cols, W = rows),
    az_heads_fwd and az_transform_heads_fwd(y = NULL); computed once and shared."""
    if (shape, B) not in _EAGER:
        from azhip import nets
        nnet, gnn = _nets(shape)
        b = torch.from_numpy(_boards(shape, B, 1000 * shape[0] + 100 * shape[1] + B))
        b = b.to(nnet.params.device)
        f = nnet.features_eager(b)
        logp, pi, v = nnet.heads(f)
        _, gpi, gv = nets.gnn_per_row_heads(nnet, gnn, f)
        torch.cuda.synchronize()
        _EAGER[(shape, B)] = SimpleNamespace(b=b, feat=f, logp=logp, pi=pi, v=v, gpi=gpi, gv=gv)
    return _EAGER[(shape, B)]


def _evaluator(shape, max_B=MAX_B):
    """(C4rEval for max_B boards, its four output tensors), one per (shape, max_B)."""
    if (shape, max_B) not in _EVALS:
        from azhip import ops
        nnet, gnn = _nets(shape)
        dev = nnet.params.device
        A = shape[0] + 1
        ev = ops.C4rEval(nnet.params, gnn.params, shape, A, max_B, dev)
        outs = [torch.empty((max_B, A) if i % 2 == 0 else (max_B,), device=dev)
                for i in range(4)]
        _EVALS[(shape, max_B)] = (ev, outs)
    return _EVALS[(shape, max_B)]


def _run(shape, b, B, kind, max_B=MAX_B):
    """One az_c4r_eval_fwd call of `kind` with every scratch and output NaN before it -> the four
    outputs as numpy (None where the kind has none); rows B.. must stay NaN."""
    from azhip import ops
    ev, outs = _evaluator(shape, max_B)
    use = [kind != "gnn", kind != "gnn", kind != "std", kind != "std"]
    for t in (ev.feat, ev.hidden, ev.logp, ev.glogp, *outs):
        t.fill_(float("nan"))
    ops.c4r_eval(ev, b, B, *[o if u else None for o, u in zip(outs, use)])
    torch.cuda.synchronize()
    got = []
    for o, u in zip(outs, use):
        a = o.cpu().numpy()
        assert np.isnan(a[B if u else 0:]).all(), (shape, B, kind)
        got.append(a[:B].copy() if u else None)
    return got


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_trunk_equals_two_conv_calls(shape):
    """az_c4r_trunk_fwd against az_conv3x3_relu_fwd x 2, torch.equal, at 1 and 3 boards (the empty
    and a full board among them); Connect4Net.features takes the fused kernel."""
    from azhip import ops
    nnet, _ = _nets(shape)
    assert nnet.route == "c4r"
    F = 64 * shape[0] * shape[1]
    for B in (1, 3):
        e = _eager(shape, B)
        got = torch.full((B, F), float("nan"), device=e.b.device)
        ops.c4r_trunk(e.b, nnet.params, out=got)
        assert torch.equal(got, e.feat), (shape, B)
        assert torch.equal(nnet.features(e.b), e.feat), (shape, B)


@pytest.mark.parametrize("shape", SHAPES)
def test_heads_from_the_lds_tile_equal_az_heads_fwd(shape):
    """az_c4r_trunk_heads_fwd at 3 boards: feat, logp, pi, v torch.equal to features_eager +
    ops.heads (7x6, 6x5: the partial last chunk; 8x7: A = 9, the 16-wide heads)."""
    from azhip import ops
    nnet, _ = _nets(shape)
    e = _eager(shape, 3)
    feat, logp, pi, v = ops.c4r_trunk_heads(e.b, nnet.params)
    for name, got, ref in (("feat", feat, e.feat), ("logp", logp, e.logp), ("pi", pi, e.pi),
                           ("v", v, e.v)):
        assert torch.equal(got, ref), (shape, name)
    f2, l2, p2, v2 = nnet.features_heads(e.b)
    assert torch.equal(f2, e.feat) and torch.equal(l2, e.logp) and torch.equal(p2, e.pi) \
        and torch.equal(v2, e.v)


@pytest.mark.parametrize("kind", ["std", "gnn", "both"])
@pytest.mark.parametrize("shape", SHAPES)
def test_eval_equals_eager_bit_for_bit(shape, kind):
    """az_c4r_eval_fwd against the eager calls at the same B: 1, 9 (MFMA tiles) and 70 (the
    M > 64 GEMM dispatch; A <= 8 also crosses into the composed heads, A = 9 keeps the y form)."""
    for B in (1, 9, 70):
        e = _eager(shape, B)
        ref = [x.cpu().numpy() for x in (e.pi, e.v, e.gpi, e.gv)]
        got = _run(shape, e.b, B, kind)
        for k, g in enumerate(got):
            if g is not None:
                assert np.array_equal(g, ref[k]), (shape, B, kind, k)


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_of_small_batches_are_batch1_bits(shape):
    """Every row of a batch of 2, 3, 5 and 8 boards equals that board's B = 1 call, bit for bit,
    all four outputs."""
    e = _eager(shape, 8)
    one = [_run(shape, e.b[i:i + 1].contiguous(), 1, "both") for i in range(8)]
    for B in (2, 3, 5, 8):
        got = _run(shape, e.b, B, "both")
        for i in range(B):
            for k in range(4):
                assert np.array_equal(got[k][i], one[i][k][0]), (shape, B, i, k)


def _float64_reference(boards, W, G):
    """Connect4Net.forward and the per-row GNN tail restated on the CPU in float64: the board
    [B][cols][rows] is the image [B][1][cols][rows] (H = cols, W = rows), flattened NCHW."""
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

    if G is None:
        return heads(f)
    y = Fn.linear(Fn.relu(Fn.linear(f, t(G, "output_transform.0.weight"),
                                    t(G, "output_transform.0.bias"))),
                  t(G, "output_transform.2.weight"), t(G, "output_transform.2.bias"))
    return heads(f) + heads(y)


@pytest.mark.parametrize("shape", SHAPES)
def test_eval_matches_float64_restatement(shape):
    """The evaluator at 8 and 70 boards against a float64 torch-CPU restatement of the network
    (conv2d x 2, the heads, output_transform): |d pi| and |d v| <= 1e-5, margins printed."""
    nnet, gnn = _nets(shape)
    tag = f"c4r_eval/{shape[0]}x{shape[1]}"
    for B in (8, 70):
        e = _eager(shape, B)
        ref = _float64_reference(e.b.cpu().numpy(), nnet.params, gnn.params)
        got = _run(shape, e.b, B, "both")
        errs = [float(np.abs(g.astype(np.float64) - r).max()) for g, r in zip(got, ref)]
        print(f"{tag}/B{B}: max err pi {errs[0]:.3g} v {errs[1]:.3g} "
              f"gnn pi {errs[2]:.3g} gnn v {errs[3]:.3g}  "
              f"margin {TOL / max(max(errs), 1e-300):.1f}x")
        for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
            assert_close(f"{tag}/B{B}/{name}", got[k], ref[k], TOL)


# Lock-step self-play batch sizes of the 7x6 board, N = K = 2688, from launch_x3's conditions for
# 256 CUs (the derivation tests/test_gpu_gemm_widths.py's header describes; _x3_class below restates
# it).  M > 256 takes the 256 x 128 tile: 21 column tiles, ceil(M / 256) row tiles.
#   M = 257:  2 x 21 = 42 tiles (< 64: no stream-K), split-K with S = min(256 / 42, 8) = 6.
#   M = 513 .. 768: 63 tiles, still < 64.
#   M = 769 .. 1024: 84 tiles, S = 3, 252 blocks = 98 % of one round of 256 CUs: split-K.
#   M = 1025: 105 tiles, S = 2, 210 blocks = 82 % < 90 % of a round, 105 * 84 k-iterations over
#             256 blocks = 34 >= 8 each: stream-K.  1025 is the smallest stream-K M.
LOCKSTEP_B = (257, 1025)


def _x3_class(M, N, K, cus=256):
    """launch_x3's tile choice restated: "s128" / "s256" split-K tiles or "csk" (stream-K)."""
    if M <= 256:
        return "s128"
    tiles = -(-M // 256) * -(-N // 128)
    S = min(256 // tiles, 8) if tiles < 256 else 1
    while S > 1 and K // S < 256:
        S -= 1
    kc = -(-(-(-K // S)) // 32) * 32 if S > 1 else K
    blocks = tiles * (-(-K // kc) if S > 1 else 1)
    rounds = -(-blocks // cus)
    iters = tiles * -(-K // 32)
    if tiles >= 64 and blocks / (rounds * cus) < 0.9 and iters // min(cus, iters) >= 8:
        return "csk"
    return "s256"


@pytest.mark.parametrize("B", LOCKSTEP_B)
def test_eval_at_lockstep_batch_sizes_7x6(B):
    """The 7x6 evaluator at 257 boards (256 x 128 split-K tiles) and 1025 (the smallest stream-K
    size), its own C4rEval of max_B = 1025: pi, v, gpi and gv within 1e-5 of the float64
    restatement and np.array_equal to the eager path; rows B..max_B stay NaN (_run).  Both sizes
    are the fp16-form GEMM (az_gemm_form 3, against 1 at <= 64 rows); az_gemm_form does not tell
    split-K from stream-K, so that the two sizes take different tile forms is asserted on the
    restated dispatch rule, and that 1025 is the smallest such M."""
    from azhip import _lib
    shape = (7, 6)
    F = 2688
    L = _lib.lib()
    ws = int(L.az_transform_heads_ws_bytes(LOCKSTEP_B[1], F, 8))
    assert L.az_gemm_form(64, F, F, ws) == 1 and L.az_gemm_form(8, F, F, ws) == 0
    assert L.az_gemm_form(257, F, F, ws) == 3 and L.az_gemm_form(1025, F, F, ws) == 3
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    assert _x3_class(257, F, F) == "s256" and _x3_class(1025, F, F) == "csk"
    assert all(_x3_class(M, F, F) != "csk" for M in range(65, 1025))
    nnet, gnn = _nets(shape)
    max_B = LOCKSTEP_B[1]
    e = _eager(shape, B)
    ref = _float64_reference(e.b.cpu().numpy(), nnet.params, gnn.params)
    eager = [x.cpu().numpy() for x in (e.pi, e.v, e.gpi, e.gv)]
    got = _run(shape, e.b, B, "both", max_B)
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"c4r_eval/7x6/B{B}/{name}", got[k], ref[k], TOL)
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert np.array_equal(got[k], eager[k]), (B, name)


def _wrapper(shape, gnn=True, seed=0):
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Game import Connect4Game
    from connect4.Connect4Net import Connect4NNetWrapper
    torch.manual_seed(7000 + 100 * shape[0] + 10 * shape[1] + seed)
    cls = Connect4GNNWrapper if gnn else Connect4NNetWrapper
    rows = None if shape[0] == shape[1] else shape[1]
    return cls(Connect4Game(shape[0], rows=rows), SimpleNamespace(gnn_layers=1, dropout=0.3))


def _eager_rows(w, boards):
    from azhip import nets
    f = w.nnet.features_eager(nets.boards_to_device(boards, w.device))
    _, pi, v = w.nnet.heads(f)
    out = [pi, v]
    if w.has_gnn:
        _, gpi, gv = nets.gnn_per_row_heads(w.nnet, w.gnn, f)
        out += [gpi, gv]
    return [x.cpu().numpy() for x in out]


def test_wrappers_take_the_one_call_routes():
    """Connect4GNNWrapper and Connect4NNetWrapper on 7x6: predict / predict_with_gnn / predict_both
    run _C4rBatch1Direct -- not the 7x7 board's _Batch1Direct -- and equal the eager path;
    batch_invariant_rows is 8; a 7x7 wrapper built afterwards in the same process still gets
    _Batch1Direct; a 4x6 wrapper (no fused kernel) takes the graph route and predicts within 1e-5
    of float64."""
    from azhip import wrappers
    shape = (7, 6)
    w = _wrapper(shape)
    assert (w.board_x, w.board_y) == shape and w.action_size == 8
    assert wrappers._is_c4r(w) and not wrappers._is_c4(w) and not wrappers._is_c4n(w)
    assert w.batch_invariant_rows == 8
    boards = _boards(shape, 8, 77).astype(np.int64)
    pi, v = w.predict(boards[3])
    gpi, gv = w.predict_with_gnn(boards[3])
    both = w.predict_both(boards)
    for kind in ("std", "gnn", "both"):
        assert type(w._g1[kind]) is wrappers._C4rBatch1Direct, kind
        assert type(w._g1[kind]) is not wrappers._Batch1Direct
    assert w._g1["both"].cap == 8 and w._g1["std"].cap == 1
    ref = _eager_rows(w, boards)
    for k, got in enumerate((pi, v, gpi, gv)):
        assert np.array_equal(np.asarray(got), ref[k][3]), k
    for k in range(4):
        assert np.array_equal(np.asarray(both[k]), ref[k]), k
    c = _wrapper(shape, gnn=False)
    b6 = _boards(shape, 4, 78).astype(np.int64)
    cpi, cv = c.predict(b6[2])
    assert type(c._g1["std"]) is wrappers._C4rBatch1Direct
    cref = _eager_rows(c, b6)
    assert np.array_equal(cpi, cref[0][2]) and cv == cref[1][2]
    w7 = _wrapper((7, 7))
    w7.predict(_boards((7, 7), 1, 79)[0].astype(np.int64))
    w7.predict_both(_boards((7, 7), 2, 80).astype(np.int64))
    assert type(w7._g1["std"]) is wrappers._Batch1Direct
    assert type(w7._g1["both"]) is wrappers._Batch1Direct
    # 4 columns x 6 rows: no fused kernel, the routes a 9x9 board takes
    w46 = _wrapper((4, 6))
    assert w46.nnet.route == "eager" and w46.batch_invariant_rows == 0
    assert not (wrappers._is_c4r(w46) or wrappers._is_c4(w46) or wrappers._is_c4n(w46))
    b46 = _boards((4, 6), 6, 81).astype(np.int64)
    ref46 = _float64_reference(b46.astype(np.int8), w46.nnet.params, w46.gnn.params)
    p1, v1 = w46.predict(b46[2])
    g1, gv1 = w46.predict_with_gnn(b46[2])
    assert isinstance(w46._g1["std"], wrappers._Batch1Graph)
    for name, got, r in (("pi", p1, ref46[0][2]), ("v", v1, ref46[1][2]), ("gpi", g1, ref46[2][2]),
                         ("gv", gv1, ref46[3][2])):
        assert_close(f"c4r_eval/4x6/predict/{name}", np.asarray(got), np.asarray(r), TOL)
    got46 = w46.predict_both(b46)
    for k, name in enumerate(("pi", "v", "pi_gnn", "v_gnn")):
        assert_close(f"c4r_eval/4x6/predict_both/{name}", np.asarray(got46[k]), ref46[k], TOL)


@pytest.mark.parametrize("var,val", [("AZ_B1_MODE", "graph"), ("AZ_NO_ZEROCOPY", "1")])
def test_environment_keeps_the_graph_routes(monkeypatch, var, val):
    """AZ_B1_MODE=graph and AZ_NO_ZEROCOPY=1 select the hipGraph / pinned-ring routes as before:
    no row-invariance promise, the same bits as the one-call route."""
    from azhip import wrappers
    shape = (7, 6)
    direct = _wrapper(shape)
    boards = _boards(shape, 12, 21).astype(np.int64)
    ref1 = direct.predict(boards[5]) + direct.predict_with_gnn(boards[5])
    pend0 = direct.predict_both_async(boards)
    assert isinstance(pend0, wrappers._PendingDirect)
    assert type(next(iter(direct._directs.values()))) is wrappers._C4rDirectBatch
    ref = pend0.result()
    monkeypatch.setenv(var, val)
    w = _wrapper(shape)
    assert w.batch_invariant_rows == 0
    got1 = w.predict(boards[5]) + w.predict_with_gnn(boards[5])
    assert isinstance(w._g1["std"], wrappers._Batch1Graph)
    assert isinstance(w._g1["gnn"], wrappers._Batch1Graph)
    pend = w.predict_both_async(boards)
    assert isinstance(pend, wrappers.PendingPrediction)
    for a, b in zip(got1 + pend.result(), ref1 + ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_arena_speculative_batches_equal_batch1_7x6():
    """Connect4 7x6 arena, GNN wrappers, 4 games at 25 simulations: speculative leaf batches
    (<= 8 boards, A = 8) play exactly the games of batch-1 leaves and serve some leaves from
    their rows."""
    from Arena import Arena
    from connect4.Connect4Game import Connect4Game
    from mcts_native import ArenaPlayer
    shape = (7, 6)
    game = Connect4Game(7, rows=6)
    args = SimpleNamespace(numMCTSSims=25, cpuct=1.0, use_gnn=True, gnn_layers=1)
    w, other = _wrapper(shape, seed=1), _wrapper(shape, seed=2)
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
    report("c4r_eval/arena_speculative_calls", batch1=calls[0], speculative=calls[1],
           wld=list(res[0][0]))
    assert res[0] == res[1]
    assert calls[1][1] > 0 and calls[1][0] + calls[1][1] == calls[0][0]


def test_lockstep_route_two_streams():
    """7x6: predict_both_async on two streams, 5 and 300 boards in flight together, read in
    reverse order: each equals the synchronous eager path; the per-stream evaluators are
    _C4rDirectBatch; the CNN-only wrapper takes the same route for predict_batch_async."""
    from azhip import wrappers
    shape = (7, 6)
    w = _wrapper(shape)
    dev = w.device
    pool = _boards(shape, 305, 31)
    sets = [pool[:5], pool[5:]]
    refs = [_eager_rows(w, s) for s in sets]
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    pend = [w.predict_both_async(b, stream=s) for b, s in zip(sets, (s1, s2))]
    assert all(isinstance(p, wrappers._PendingDirect) for p in pend)
    assert len(w._directs) == 2
    assert all(type(d) is wrappers._C4rDirectBatch for d in w._directs.values())
    for p, ref in reversed(list(zip(pend, refs))):
        for a, b in zip(p.result(), ref):
            assert np.array_equal(a, b)
    for a, b in zip(w.predict_both(sets[0]), refs[0]):       # the synchronous route, 5 rows
        assert np.array_equal(np.asarray(a), b)
    c = _wrapper(shape, gnn=False)
    c.nnet.params.copy_flat_(w.nnet.params.flat)
    pi, v, gpi, gv = c.predict_batch_async(sets[1]).result()
    assert gpi is None and gv is None
    assert np.array_equal(pi, refs[1][0]) and np.array_equal(v, refs[1][1])
    assert type(next(iter(c._directs.values()))) is wrappers._C4rDirectBatch


def test_validation_returns_einval_before_any_launch():
    """B = 0, B > max_B, (7, 7), (6, 7), F off by 64, A = 33 and a null weight pointer: AZ_EINVAL
    with the naming word in az_last_error, and nothing is launched (the NaN-filled outputs and
    scratch stay NaN); a valid call afterwards succeeds."""
    from azhip import _lib, ops
    shape = (7, 6)
    nnet, gnn = _nets(shape)
    dev = nnet.params.device
    L = _lib.lib()
    ev = ops.C4rEval(nnet.params, gnn.params, shape, 8, 4, dev)
    b = torch.from_numpy(_boards(shape, 8, 1)).to(dev)
    outs = [torch.empty((4, 8), device=dev), torch.empty((4,), device=dev),
            torch.empty((4, 8), device=dev), torch.empty((4,), device=dev)]
    watched = [ev.feat, ev.hidden, ev.logp, ev.glogp, *outs]
    for t in watched:
        t.fill_(float("nan"))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(desc, B):
        return L.az_c4r_eval_fwd(ctypes.byref(desc), P(b), B, *[P(o) for o in outs], None)

    def copy(**kw):
        d = _lib.C4rEval()
        ctypes.memmove(ctypes.byref(d), ctypes.byref(ev.desc), ctypes.sizeof(d))
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    cases = ((ev.desc, 0, b"B=0"), (ev.desc, 5, b"max_B"),
             (copy(ny=7, F=3136), 1, b"nx=7 ny=7"), (copy(nx=6, ny=7, A=7), 1, b"nx=6 ny=7"),
             (copy(F=2752), 1, b"F=2752"), (copy(A=33), 1, b"A=33"),
             (copy(fc_value_w=None), 1, b"null"))
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
