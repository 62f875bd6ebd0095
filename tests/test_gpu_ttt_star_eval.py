"""TicTacToe stars on the MI355X: az_gnn_star_packed_infer (the layer stack on B <= 8 packed stars
of <= 26 rows) against float64 at F = 128, 512 and 1,152, the reference's quirks, independence of
a star from its pack, az_ttt_star_eval_fwd (trunk -> layers -> output_transform -> fc1 / fc2 ->
heads of row 0) on 3x3, 4x4 and 5x5 from device buffers and from mapped host memory, the trunk
inside the call, the host checks of a mapped offs, the reference's own outputs on the twelve
recorded positions, the wrappers' routes and a 25-simulation search with args.gnn_neighbors on
both routes.

Bar: atol 1e-5 on pi, log pi and v (the project's), and on the feature rows the layer stack
returns (values of order 1: fp32 against float64 over dot products of 2F <= 2,304 terms).  The
float64 restatement is tests/test_gpu_star_eval.py's (_float64_star_eval, _oracle_rows)."""
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import assert_close, golden, report
from test_gpu_star_eval import _f64, _float64_star_eval, _oracle_rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
NODES = 26
NAN = float("nan")
# node counts per width: 1, 2, 3 and 10 everywhere, 17 from F = 512, 26 at F = 1,152; the first
# star is the largest, so the B = 1 call wraps the per-wave loops too
COUNTS = {128: (10, 1, 2, 3, 10, 1, 2, 3), 512: (17, 1, 2, 3, 10, 17, 1, 2),
          1152: (26, 1, 2, 3, 10, 17, 26, 1)}
# (stars, layers): every B with L = 1 and 2, L = 4 at one B per F
CALLS = ((1, 1), (3, 1), (8, 1), (1, 2), (3, 2), (8, 2), (3, 4))

_GNN, _ORACLE = {}, {}


def _gnn(F):
    """A four-layer PolicyValueGNN per width (the calls use its first L layers)."""
    if F not in _GNN:
        from azhip import nets
        _GNN.clear()
        _ORACLE.clear()
        torch.manual_seed(9100 + F)
        _GNN[F] = nets.PolicyValueGNN(F, 4).eval()
    return _GNN[F]


def _features(F, counts, seed=1):
    """[B][26][F] in [-1, 1]; every slot at or beyond counts[b] is NaN."""
    x = np.random.default_rng(seed * 10007 + F).uniform(-1, 1, (len(counts), NODES, F))
    x = x.astype(np.float32)
    for b, n in enumerate(counts):
        x[b, n:] = np.nan
    return x


def _oracle(F):
    if F not in _ORACLE:
        _ORACLE[F] = _oracle_rows(_f64(_gnn(F).params), _features(F, COUNTS[F]), COUNTS[F], 4)
    return _ORACLE[F]


def _pack(x, counts):
    """Slots -> packed rows [V + 3][F] (three NaN rows past V) and offs."""
    rows = np.concatenate([x[b, :n] for b, n in enumerate(counts)] +
                          [np.full((3, x.shape[2]), np.nan, np.float32)])
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rows, offs


def _infer(gnn, x, counts, L):
    """ops.gnn_star_packed_infer on the stars x[b, :counts[b]]; rows past V, the workspace and
    the output hold NaN before the call."""
    from azhip import ops
    dev = gnn.params.device
    rows, offs = _pack(x, counts)
    V = int(offs[-1])
    xt = torch.from_numpy(rows).to(dev)
    ot = torch.from_numpy(offs).to(dev)
    out = torch.full((len(counts), x.shape[2]), NAN, device=dev)
    nb = max(256, int(ops._lib.lib().az_gnn_star_packed_infer_ws_bytes(len(counts), x.shape[2],
                                                                        128, L)))
    ws = torch.full((nb // 4,), NAN, device=dev).view(torch.uint8)
    gnn.params.sync()
    ops.gnn_star_packed_infer(xt[:V], ot, [l.weights() for l in gnn.layers[:L]], out=out, ws=ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("F", [128, 512, 1152])
def test_packed_infer_matches_float64(F):
    """az_gnn_star_packed_infer at B = 1, 3 and 8 with L = 1 and 2 (L = 4 at B = 3) against
    oracle.nets.gnn_layer_star in float64: F = 128 is half an attention slice, F = 1,152 ends in a
    half slice, stars of 17 and 26 rows wrap the per-wave loops."""
    gnn, counts = _gnn(F), COUNTS[F]
    x, ref = _features(F, counts), _oracle(F)
    for B, L in CALLS:
        got = _infer(gnn, x[:B], counts[:B], L).cpu().numpy()
        assert np.isfinite(got).all(), (F, B, L)
        worst = assert_close(f"ttt_star_infer/F{F}/B{B}/L{L}", got, np.stack(ref[L][:B]), TOL)
        print(f"ttt_star_infer F={F} B={B} L={L}: max err {worst:.3g} "
              f"({TOL / max(worst, 1e-300):.1f}x)")


def test_packed_infer_quirks():
    """A one-row star returns its row (torch.equal) at L = 0 and L = 2, alone and between two
    large stars; L = 0 is the gather of the row 0s; attention.2.bias = -200 makes every weight 0
    in fp32 (exp(200) overflows, as in the reference's own fp32 sigmoid), so the sum is 0, nothing
    is divided (gnn_utils.py:58-59) and the aggregate is 0.  In float64 sigmoid(-200) is 1.4e-87,
    not 0, so the float64 value of that case is the no-division branch written out: the node
    update of (t, agg = 0) in float64; that the fp32 restatement takes that branch is asserted."""
    from oracle import nets as O
    F = 512
    gnn, counts = _gnn(F), (17, 1, 10)
    x = _features(F, counts, seed=3)
    dev = gnn.params.device
    row = torch.from_numpy(x[1, 0]).to(dev)
    for L in (0, 2):
        assert torch.equal(_infer(gnn, x[1:2], counts[1:2], L)[0], row), L
        assert torch.equal(_infer(gnn, x, counts, L)[1], row), L
    assert torch.equal(_infer(gnn, x, counts, 0), torch.from_numpy(x[:, 0]).to(dev))
    bias = gnn.params["layers.0.attention.2.bias"]
    keep = bias.clone()
    try:
        bias.fill_(-200.0)
        G64 = _f64(gnn.params)
        trace = {}
        with np.errstate(over="ignore"):
            O.gnn_layer_star(x[0, :17], G64, 0, dtype=np.float32, trace=trace)
        assert not trace["agg"][0].any() and not trace["alpha_raw"][0].any()
        refs = []
        for b, n in enumerate(counts):
            t = x[b, :1].astype(np.float64)
            refs.append(t[0] if n == 1 else
                        O.node_update(t, np.zeros_like(t), O._layer(G64, 0, np.float64))[0])
        got = _infer(gnn, x, counts, 1).cpu().numpy()
        assert np.isfinite(got).all()
        worst = assert_close("ttt_star_infer/zero_weights", got, np.stack(refs), TOL)
        print(f"ttt_star_infer zero weights: max err {worst:.3g}")
    finally:
        bias.copy_(keep)


PACK = (26, 1, 17, 2, 10, 26, 3, 5)
ORDER = (5, 2, 0, 7, 4)


def test_rows_do_not_depend_on_the_pack():
    """F = 1,152, stars of 26, 1, 17, 2, 10, 26, 3 and 5 rows: star b of the 8-star pack is
    torch.equal to the same star alone and to the same star at another position of a pack with
    other neighbours; two calls give equal bits."""
    F = 1152
    gnn = _gnn(F)
    x = _features(F, PACK, seed=5)
    full = _infer(gnn, x, PACK, 2)
    assert torch.equal(full, _infer(gnn, x, PACK, 2))
    for b in range(8):
        alone = _infer(gnn, x[b:b + 1], PACK[b:b + 1], 2)
        assert torch.equal(alone[0], full[b]), b
    moved = _infer(gnn, x[list(ORDER)], [PACK[b] for b in ORDER], 2)
    for i, b in enumerate(ORDER):
        assert torch.equal(moved[i], full[b]), (i, b)


# ------------------------------------------------------------------------------ the evaluator
_NETS = {}


def _game(n):
    return SimpleNamespace(getBoardSize=lambda: (n, n), getActionSize=lambda: n * n + 1)


def _nets(n, L=2):
    if (n, L) not in _NETS:
        from azhip import nets
        _NETS.clear()
        _GNN.clear()
        _ORACLE.clear()
        torch.manual_seed(8700 + 10 * n + L)
        nnet = nets.TicTacToeNet(_game(n), {}).eval()
        _NETS[(n, L)] = (nnet, nets.PolicyValueGNN(nnet.feature_dim, L).eval())
    return _NETS[(n, L)]


def _real_stars(n):
    """The opening, a two-node position and a mid-game one of the recorded fixture, as lists of
    boards [leaf] + children."""
    z = golden("ttt_star_leaf.npz")
    return [z[f"boards_n{n}"][p, :z[f"counts_n{n}"][p]] for p in (0, 1, 2)]


def _pack_boards(lists):
    rows = np.concatenate([np.asarray(s, np.int8) for s in lists])
    offs = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    return rows, offs


def _run(ev, rows, offs, gpi, gv):
    from azhip import ops
    for t in (ev.feat, ev.x0, ev.hidden, ev.y, ev.h1, ev.h2, ev.glogp):
        t.fill_(NAN)
    ev.ws.view(torch.float32).fill_(NAN)
    ops.ttt_star_eval(ev, rows, offs, offs.numel() - 1, int(rows.shape[0]), gpi=gpi, gv=gv)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,L", [(3, 2), (4, 2), (5, 2), (3, 0), (3, 1), (3, 4), (5, 0), (5, 1),
                                 (5, 4)])
def test_star_eval_matches_float64_from_device_and_host_buffers(n, L):
    """az_ttt_star_eval_fwd on three real stars (the opening of n^2 + 1 boards, a two-node
    position, a mid-game one) against the float64 path: gpi, log gpi and gv within 1e-5, from
    device buffers and from HostBuffer views with equal bits, every scratch buffer NaN before."""
    from azhip import ops
    nnet, gnn = _nets(n, L)
    assert len(gnn.layers) == L
    dev = nnet.params.device
    A = n * n + 1
    lists = _real_stars(n)
    B = len(lists)
    rpi, rlogp, rv = _float64_star_eval(lists, nnet.params, gnn.params, L, heads="ttt")
    nnet.params.sync()
    gnn.params.sync()
    ev = ops.TttStarEval(nnet.params, gnn.params, n, A, L, 8, dev)
    rows, offs = _pack_boards(lists)
    gpi = torch.full((8, A), NAN, device=dev)
    gv = torch.full((8,), NAN, device=dev)
    _run(ev, torch.from_numpy(rows).to(dev), torch.from_numpy(offs).to(dev), gpi, gv)
    pi, v = gpi.cpu().numpy(), gv.cpu().numpy()
    assert np.isnan(pi[B:]).all() and np.isnan(v[B:]).all()
    tag = f"ttt_star_eval/{n}x{n}/L{L}"
    for name, got, ref in (("pi", pi[:B], rpi), ("logp", ev.glogp[:B].cpu().numpy(), rlogp),
                           ("v", v[:B], rv)):
        worst = assert_close(f"{tag}/device/{name}", got, ref, TOL)
        print(f"{tag} device {name}: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")
    # mapped host memory
    off = (rows.nbytes + 255) // 256 * 256
    hb = ops.HostBuffer(off + 256 + 1024 + 256)
    h_rows = hb.view(0, torch.int8, rows.shape)
    h_offs = hb.view(off, torch.int32, (B + 1,))
    h_pi = hb.view(off + 256, torch.float32, (8, A))
    h_v = hb.view(off + 256 + 1024, torch.float32, (8,))
    h_rows.numpy()[...] = rows
    h_offs.numpy()[...] = offs
    _run(ev, h_rows, h_offs, h_pi, h_v)
    assert np.array_equal(h_pi.numpy()[:B], pi[:B]) and np.array_equal(h_v.numpy()[:B], v[:B])
    del hb


def test_mapped_offs_is_checked_before_any_launch():
    """offs in mapped host memory: a non-ascending offs, a 27-row star and offs[B] != V are
    rejected on the host with a message, and nothing is written."""
    from azhip import ops
    n, A = 5, 26
    nnet, gnn = _nets(n, 2)
    dev = nnet.params.device
    ev = ops.TttStarEval(nnet.params, gnn.params, n, A, 2, 8, dev)
    hb = ops.HostBuffer(64 * 25 + 256 + 1024 + 256)
    h_rows = hb.view(0, torch.int8, (64, n, n))
    h_offs = hb.view(1600, torch.int32, (4,))
    h_pi = hb.view(1600 + 256, torch.float32, (8, A))
    h_v = hb.view(1600 + 256 + 1024, torch.float32, (8,))
    h_rows.zero_()
    for offs, V, word in (((0, 5, 5, 9), 9, "not ascending"), ((0, 5, 3, 9), 9, "not ascending"),
                          ((0, 27, 28, 30), 30, "27 rows"), ((0, 2, 4, 6), 7, "offs[B]=6"),
                          ((1, 2, 4, 6), 6, "offs[0]=1")):
        h_offs.numpy()[...] = offs
        h_pi.fill_(NAN)
        h_v.fill_(NAN)
        ev.feat.fill_(NAN)
        with pytest.raises(RuntimeError, match=word.replace("[", r"\[").replace("]", r"\]")):
            ops.ttt_star_eval(ev, h_rows, h_offs, 3, V, gpi=h_pi, gv=h_v)
        torch.cuda.synchronize()
        assert torch.isnan(h_v).all() and torch.isnan(ev.feat).all(), offs
        x = torch.zeros((V, 1152), device=dev)
        with pytest.raises(RuntimeError, match="az_gnn_star_packed_infer"):
            ops.gnn_star_packed_infer(x, h_offs, [l.weights() for l in gnn.layers])
    del hb


@pytest.mark.parametrize("n", [3, 5])
def test_trunk_inside_the_call_and_pack_independence(n):
    """Eight stars of PACK's sizes cut to n^2 + 1 boards (at n = 5: 26, 1, 17, 2, 10, 26, 3, 5;
    V <= 208): the feature rows the call leaves are torch.equal to ops.ttt_trunk of the same
    boards, and every star's gpi / gv is np.array_equal to the same star evaluated alone and at
    another position of a pack with other neighbours."""
    from azhip import ops
    nnet, gnn = _nets(n, 2)
    dev = nnet.params.device
    A = n * n + 1
    sizes = [min(s, n * n + 1) for s in PACK]
    rng = np.random.default_rng(40 + n)
    lists = [rng.integers(-1, 2, size=(s, n, n)).astype(np.int8) for s in sizes]
    nnet.params.sync()
    gnn.params.sync()
    ev = ops.TttStarEval(nnet.params, gnn.params, n, A, 2, 8, dev)
    gpi = torch.full((8, A), NAN, device=dev)
    gv = torch.full((8,), NAN, device=dev)

    def run(ls):
        rows, offs = _pack_boards(ls)
        _run(ev, torch.from_numpy(rows).to(dev), torch.from_numpy(offs).to(dev), gpi, gv)
        return rows, gpi.cpu().numpy()[:len(ls)], gv.cpu().numpy()[:len(ls)]

    rows, pi, v = run(lists)
    V = rows.shape[0]
    assert V == sum(sizes) <= 208
    assert torch.equal(ev.feat[:V], ops.ttt_trunk(torch.from_numpy(rows).to(dev), nnet.params))
    assert np.isfinite(pi).all() and np.isfinite(v).all()
    for b in range(8):
        _, p1, v1 = run(lists[b:b + 1])
        assert np.array_equal(p1[0], pi[b]) and v1[0] == v[b], (n, b)
    _, pm, vm = run([lists[b] for b in ORDER])
    for i, b in enumerate(ORDER):
        assert np.array_equal(pm[i], pi[b]) and vm[i] == v[b], (n, i, b)


# ------------------------------------------------------------------------------ the wrappers
def _wrapper(n, layers=2, seed=0, **keys):
    from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    _NETS.clear()
    _GNN.clear()
    _ORACLE.clear()
    torch.manual_seed(7600 + 10 * n + seed)
    game = TicTacToeGame(n)
    return game, TicTacToeGNNWrapper(game, SimpleNamespace(gnn_layers=layers, dropout=0.3, **keys))


@pytest.mark.parametrize("n", [3, 4, 5])
def test_reference_star_positions(n):
    """The reference's own apply_policy_value_heads(gnn(extract_features(boards)))[0] on the four
    recorded positions per board side (tests/golden/ttt_star_leaf.npz: the opening, one empty
    cell, a mid-game position with a terminal child, the board after one move) through
    predict_with_gnn(board, neighbor_states=...) under gnn_neighbors: the one-call route, pi,
    log pi and v within 1e-5."""
    from azhip import wrappers
    from azhip.weights import gnn_spec, synthetic_state_dict, tictactoe_net_spec
    z = golden("ttt_star_leaf.npz")
    _, w = _wrapper(n, gnn_neighbors=True)
    F = 128 * (n - 2) ** 2
    W = synthetic_state_dict(tictactoe_net_spec(n), int(z["net_seed"]) + n)
    G = synthetic_state_dict(gnn_spec(F, 2), int(z["gnn_seed"]) + n)
    w.nnet.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    w.gnn.load_state_dict({k: torch.from_numpy(v) for k, v in G.items()})
    counts = z[f"counts_n{n}"]
    assert tuple(counts[[0, 1, 3]]) == (n * n + 1, 2, n * n)
    for p, c in enumerate(counts):
        nodes = z[f"boards_n{n}"][p, :c].astype(np.int64)
        logp = z[f"logp_n{n}"][p].astype(np.float64)
        pi, v = w.predict_with_gnn(nodes[0], neighbor_states=list(nodes[1:]))
        assert w.star_route == "onecall"
        assert isinstance(w._ttt_star_direct, wrappers._TttStarDirect)
        tag = f"ttt_star_eval/reference/{n}x{n}/{p}"
        worst = max(assert_close(f"{tag}/pi", pi, np.exp(logp), TOL),
                    assert_close(f"{tag}/logp", np.log(pi), logp, TOL),
                    assert_close(f"{tag}/v", v, z[f"v_n{n}"][p], TOL))
        print(f"{tag}: {c} nodes, max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")


def test_wrapper_routes(monkeypatch):
    """3x3 under args.gnn_neighbors: 1 and 8 stars take the one-call evaluator (a star's bits those
    of the star alone); 9 stars the composition, or the batched route under gnn_neighbors_lockstep;
    a star of n^2 + 2 = 11 boards, gnn_layers = 5, AZ_B1_MODE=graph and AZ_NO_ZEROCOPY=1 the
    composition; batch_invariant the exact route; the same wrapper without the key the composition.
    Every result within 1e-5 of float64."""
    n, shape = 3, (3, 3)
    rng = np.random.default_rng(6)
    stars = [[b for b in rng.integers(-1, 2, size=(c,) + shape)]
             for c in (10, 2, 9, 1, 5, 10, 3, 8, 6)]
    big = [b for b in rng.integers(-1, 2, size=(11,) + shape)]
    _, w = _wrapper(n, gnn_neighbors=True)
    assert not hasattr(w, "star_route")
    rpi, _, rv = _float64_star_eval(stars + [big], w.nnet.params, w.gnn.params, 2, heads="ttt")

    def check(tag, w, lists, idx, route, ref=None):
        epi, ev = ref if ref is not None else (rpi, rv)
        pi, v = w.predict_star_batch(lists)
        assert w.star_route == route, (tag, w.star_route)
        assert pi.shape == (len(lists), 10) and v.shape == (len(lists),)
        worst = max(assert_close(f"ttt_star_eval/wrapper/{tag}/pi", pi, epi[idx], TOL),
                    assert_close(f"ttt_star_eval/wrapper/{tag}/v", v, ev[idx], TOL))
        print(f"ttt_star_eval wrapper {tag} -> {route}: max err {worst:.3g}")
        return pi, v

    p1, v1 = check("1", w, stars[:1], [0], "onecall")
    p8, v8 = check("8", w, stars[:8], list(range(8)), "onecall")
    assert np.array_equal(p8[0], p1[0]) and v8[0] == v1[0]
    pi, v = w.predict_with_gnn(stars[4][0], neighbor_states=stars[4][1:])
    assert w.star_route == "onecall"
    assert np.array_equal(pi, p8[4]) and v == v8[4]
    check("9", w, stars, list(range(9)), "composition")
    check("11nodes", w, [big, stars[1]], [9, 1], "composition")
    for var, val in (("AZ_B1_MODE", "graph"), ("AZ_NO_ZEROCOPY", "1")):
        with monkeypatch.context() as m:
            m.setenv(var, val)
            check(var, w, stars[:2], [0, 1], "composition")
    w.args.gnn_neighbors_lockstep = True
    check("9/lockstep", w, stars, list(range(9)), "batched")
    check("11nodes/lockstep", w, [big, stars[1]], [9, 1], "batched")
    check("8/lockstep", w, stars[:8], list(range(8)), "onecall")
    w.args.gnn_neighbors_lockstep = False
    w.args.gnn_neighbors = False
    check("8/no_key", w, stars[:8], list(range(8)), "composition")
    del w.args.gnn_neighbors
    check("1/no_key", w, stars[:1], [0], "composition")
    # other wrappers: five layers, batch_invariant
    _, w5 = _wrapper(n, layers=5, gnn_neighbors=True)
    ref5 = _float64_star_eval(stars[:3], w5.nnet.params, w5.gnn.params, 5, heads="ttt")
    check("L5", w5, stars[:3], [0, 1, 2], "composition", ref=(ref5[0], ref5[2]))
    _, wx = _wrapper(n, gnn_neighbors=True, batch_invariant=True)
    refx = _float64_star_eval(stars[:3], wx.nnet.params, wx.gnn.params, 2, heads="ttt")
    check("exact", wx, stars[:3], [0, 1, 2], "exact", ref=(refx[0], refx[2]))


def test_search_with_gnn_neighbors_on_both_routes(monkeypatch):
    """25 simulations of getActionProb on the 3x3 opening with use_gnn and gnn_neighbors, once on
    the one-call route and once on the composition: every GNN evaluation carried the leaf's
    children, the root counts sum to 24, the route names are as expected.  The two routes' counts
    are reported, not compared (their outputs differ in the last bits)."""
    from MCTS import MCTS
    game, w = _wrapper(3, seed=3, gnn_neighbors=True)
    args = SimpleNamespace(numMCTSSims=25, cpuct=1.0, use_gnn=True, gnn_neighbors=True)
    board = game.getCanonicalForm(game.getInitBoard(), 1)
    seen = []
    orig = w.predict_with_gnn

    def spy(b, neighbor_states=None):
        seen.append(len(neighbor_states))
        return orig(b, neighbor_states=neighbor_states)

    w.predict_with_gnn = spy
    counts = {}
    for route, env in (("onecall", None), ("composition", ("AZ_B1_MODE", "graph"))):
        with monkeypatch.context() as m:
            if env:
                m.setenv(*env)
            w.__dict__.pop("_g1", None)
            mcts = MCTS(game, w, args)
            mcts.getActionProb(board, temp=1)
            assert w.star_route == route
            counts[route] = mcts._root_counts(game.stringRepresentation(board))
            assert sum(counts[route]) == 24, (route, counts[route])
    w.__dict__.pop("_g1", None)
    print("root counts", counts)
    report("ttt_star_eval/search_counts", **{k: [int(c) for c in v] for k, v in counts.items()})
    assert len(seen) > 0 and all(c >= 1 for c in seen)
