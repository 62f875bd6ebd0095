"""GNN leaf evaluation over the leaf's children on the MI355X: az_gnn_star_infer (the layer stack on
B <= 8 stars of <= 9 rows) against float64, the reference's quirks, independence of a star from its
batch, az_c4_star_eval_fwd (trunk -> layers -> output_transform -> heads of row 0) on five board
shapes from device buffers and from mapped host memory, the composition route on the generic
graph calls, the reference's own outputs on six recorded positions, the wrappers' routes and a
25-simulation search with args.gnn_neighbors on both routes.

Bar: atol 1e-5 on pi, log pi and v (the project's), and on the feature rows az_gnn_star_infer
returns (values of order 1: fp32 against float64 over dot products of 2F <= 6,272 terms)."""
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import assert_close, golden, report, split_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
NODES = 9
# eight stars whose slices are the B = 1, 2, 5 and 8 calls: counts 1, 2, 3, 8 and 9 among them
COUNTS = (9, 1, 8, 2, 3, 8, 9, 5)
CALLS = ((0, 1, 1), (1, 3, 2), (3, 8, 3), (0, 8, 1), (0, 8, 2), (0, 8, 3))   # (first, last, L)
WIDTHS = (1024, 1280, 2688, 3136)

_GNN, _ORACLE = {}, {}


def _gnn(F, L=3):
    if (F, L) not in _GNN:
        from azhip import nets
        _GNN.clear()                              # one width's 0.7 GB at a time
        _ORACLE.clear()
        torch.manual_seed(9000 + F + L)
        _GNN[(F, L)] = nets.PolicyValueGNN(F, L).eval()
    return _GNN[(F, L)]


def _features(F, seed=1):
    """[8][9][F] in [-1, 1]; every slot at or beyond COUNTS[b] is NaN."""
    x = np.random.default_rng(seed * 10007 + F).uniform(-1, 1, (8, NODES, F)).astype(np.float32)
    for b, n in enumerate(COUNTS):
        x[b, n:] = np.nan
    return x


def _f64(params):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in params.views.items()}


def _oracle_rows(G64, x, counts, L):
    """rows[l][b]: row 0 of star b after l layers, float64 (oracle.nets.gnn_layer_star)."""
    from oracle.nets import gnn_layer_star
    rows = [[x[b, 0].astype(np.float64) for b in range(len(counts))]]
    cur = [x[b, :n].astype(np.float64) for b, n in enumerate(counts)]
    for l in range(L):
        with np.errstate(over="ignore"):
            cur = [gnn_layer_star(c, G64, l) for c in cur]
        rows.append([c[0] for c in cur])
    return rows


def _oracle(F):
    if F not in _ORACLE:
        gnn = _gnn(F)
        _ORACLE[F] = _oracle_rows(_f64(gnn.params), _features(F), COUNTS, 3)
    return _ORACLE[F]


def _infer(gnn, x, counts, L):
    from azhip import ops
    dev = gnn.params.device
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ct = torch.tensor(list(counts), dtype=torch.int32, device=dev)
    out = torch.full((xt.shape[0], xt.shape[2]), float("nan"), device=dev)
    gnn.params.sync()
    ops.gnn_star_infer(xt, ct, [l.weights() for l in gnn.layers[:L]], out=out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("F", WIDTHS)
def test_star_infer_matches_float64(F):
    """az_gnn_star_infer at B = 1, 2, 5 and 8 with mixed counts (1, 2, 3, 8, 9) and L = 1, 2, 3
    against oracle.nets.gnn_layer_star in float64; F = 2688 and 3136 end in a partial 256-column
    slice.  The unused slots hold NaN throughout."""
    gnn, x, ref = _gnn(F), _features(F), _oracle(F)
    for lo, hi, L in CALLS:
        got = _infer(gnn, x[lo:hi], COUNTS[lo:hi], L).cpu().numpy()
        assert np.isfinite(got).all(), (F, lo, hi, L)
        worst = assert_close(f"star_infer/F{F}/B{hi - lo}/L{L}", got, np.stack(ref[L][lo:hi]), TOL)
        print(f"star_infer F={F} B={hi - lo} L={L}: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")


def test_star_infer_four_layers():
    """L = 4, the deepest stack az_gnn_star_infer accepts (AZ_STAR_MAX_LAYERS), at F = 1024 on a
    four-layer net of its own: all eight stars of COUNTS in one call."""
    F = 1024
    gnn, x = _gnn(F, 4), _features(F)
    assert len(gnn.layers) == 4
    ref = _oracle_rows(_f64(gnn.params), x, COUNTS, 4)[4]
    got = _infer(gnn, x, COUNTS, 4).cpu().numpy()
    assert np.isfinite(got).all()
    worst = assert_close(f"star_infer/F{F}/B8/L4", got, np.stack(ref), TOL)
    print(f"star_infer F={F} B=8 L=4: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")


def test_star_infer_quirks():
    """A one-row star returns its feature row (torch.equal, also with L = 0); attention.2.bias =
    -1e4 underflows every weight to 0, so the aggregate is 0 and not divided (gnn_utils.py:58-59);
    duplicate neighbour rows: all against the float64 oracle."""
    F = 1280
    gnn, x = _gnn(F), _features(F)
    dev = gnn.params.device
    got = _infer(gnn, x, COUNTS, 2)
    assert torch.equal(got[1], torch.from_numpy(x[1, 0]).to(dev))
    got0 = _infer(gnn, x, COUNTS, 0)
    assert torch.equal(got0, torch.from_numpy(x[:, 0]).to(dev))
    # duplicates
    xd = x.copy()
    xd[0, 2] = xd[0, 1]
    xd[0, 5] = xd[0, 1]
    xd[2, 3] = xd[2, 7]
    G64 = _f64(gnn.params)
    ref = _oracle_rows(G64, xd[:3], COUNTS[:3], 2)[2]
    assert_close("star_infer/duplicates", _infer(gnn, xd[:3], COUNTS[:3], 2).cpu().numpy(),
                 np.stack(ref), TOL)
    # every attention weight 0
    bias = gnn.params["layers.0.attention.2.bias"]
    keep = bias.clone()
    try:
        bias.fill_(-1e4)
        G64["layers.0.attention.2.bias"] = np.array([-1e4])
        trace = {}
        from oracle.nets import gnn_layer_star
        with np.errstate(over="ignore"):
            r = gnn_layer_star(x[0, :9].astype(np.float64), G64, 0, trace=trace)
        assert not trace["agg"][0].any() and not trace["alpha_raw"][0].any()
        got = _infer(gnn, x[:1], COUNTS[:1], 1).cpu().numpy()
        assert_close("star_infer/zero_weights", got[0], r[0], TOL)
    finally:
        bias.copy_(keep)


def test_star_infer_rows_do_not_depend_on_the_batch():
    """Star b of the B = 8 call is torch.equal to the same star alone and to the same star at
    another position of another batch; NaN against 0 in the unused slots changes no bit; two calls
    give equal bits."""
    F = 2688
    gnn, x = _gnn(F), _features(F)
    full = _infer(gnn, x, COUNTS, 2)
    assert torch.equal(full, _infer(gnn, x, COUNTS, 2))
    for b in range(8):
        alone = _infer(gnn, x[b:b + 1], COUNTS[b:b + 1], 2)
        assert torch.equal(alone[0], full[b]), b
    order = [5, 2, 0, 7]
    moved = _infer(gnn, x[order], [COUNTS[b] for b in order], 2)
    for i, b in enumerate(order):
        assert torch.equal(moved[i], full[b]), (i, b)
    assert torch.equal(full, _infer(gnn, np.nan_to_num(x, nan=0.0), COUNTS, 2))
    # PolicyValueGNN.star_rows0: the same call over all of the network's layers
    xt = torch.from_numpy(x).to(gnn.params.device)
    assert torch.equal(gnn.star_rows0(xt, COUNTS), _infer(gnn, x, COUNTS, 3))
    assert torch.equal(gnn.star_rows0(xt[2:3], [COUNTS[2]]), _infer(gnn, x[2:3], COUNTS[2:3], 3))


# ------------------------------------------------------------------------------ the evaluator
SHAPES = ((7, 7), (4, 4), (8, 8), (7, 6), (5, 4))
STAR_COUNTS = (8, 1, 5)
_NETS, _REF = {}, {}


def _game(shape):
    return SimpleNamespace(getBoardSize=lambda: tuple(shape), getActionSize=lambda: shape[0] + 1)


def _nets(shape):
    if shape not in _NETS:
        from azhip import nets
        _NETS.clear()
        _GNN.clear()
        _ORACLE.clear()
        torch.manual_seed(8000 + 10 * shape[0] + shape[1])
        nnet = nets.Connect4Net(_game(shape), {"dropout": 0.0}).eval()
        _NETS[shape] = (nnet, nets.PolicyValueGNN(nnet.feature_dim, 2).eval())
    return _NETS[shape]


def _star_boards(shape, counts, seed):
    """int8 [B][9][cols][rows] in {-1, 0, 1}; slots at or beyond counts[b] hold 2s."""
    b = np.random.default_rng(seed).integers(-1, 2, size=(len(counts), NODES) + tuple(shape))
    b = b.astype(np.int8)
    for i, n in enumerate(counts):
        b[i, n:] = 2
    return b


def _float64_star_eval(node_lists, W, G, L, heads="c4"):
    """c4 features -> star layers -> output_transform -> heads, row 0 of every star, float64
    (the convolutions in torch double: the board [cols][rows] is the image [1][cols][rows])."""
    import torch.nn.functional as Fn
    from oracle import nets as O
    Wn = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in W.views.items()}
    G64 = _f64(G)
    rows = []
    for nodes in node_lists:
        xb = torch.from_numpy(np.asarray(nodes)).double()[:, None]
        t = lambda k: torch.from_numpy(Wn[k])  # noqa: E731
        xb = Fn.relu(Fn.conv2d(xb, t("conv1.weight"), t("conv1.bias"), padding=1))
        xb = Fn.relu(Fn.conv2d(xb, t("conv2.weight"), t("conv2.bias"), padding=1))
        if heads == "ttt":
            xb = Fn.relu(Fn.conv2d(xb, t("conv3.weight"), t("conv3.bias"), padding=0))
        f = xb.flatten(1).numpy()
        if heads == "c4" and f.shape[0] and np.asarray(nodes).shape[1] == np.asarray(nodes).shape[2]:
            assert np.allclose(f, O.c4_features(np.asarray(nodes), Wn), rtol=0, atol=1e-12)
        for l in range(L):
            f = O.gnn_layer_star(f, G64, l)
        rows.append(f[0])
    y = O.output_transform(np.stack(rows), G64)
    logp, v = (O.c4_heads if heads == "c4" else O.ttt_heads)(y, Wn)
    return np.exp(logp), logp, v


def _reference(shape):
    if shape not in _REF:
        nnet, gnn = _nets(shape)
        boards = _star_boards(shape, STAR_COUNTS, 31 * shape[0] + shape[1])
        lists = [boards[b, :n] for b, n in enumerate(STAR_COUNTS)]
        _REF.clear()
        _REF[shape] = (boards, _float64_star_eval(lists, nnet.params, gnn.params, 2))
    return _REF[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_star_eval_matches_float64_from_device_and_host_buffers(shape):
    """az_c4_star_eval_fwd on three stars (8, 1 and 5 boards; unused slots hold 2s) against the
    float64 path, from device buffers and from HostBuffer views with equal bits; a star alone and
    2s replaced by 0s give the same bits; the composition on the generic graph calls meets the
    same float64 values, and the two routes agree within twice the bar."""
    from azhip import nets, ops
    nnet, gnn = _nets(shape)
    dev = nnet.params.device
    A, B = shape[0] + 1, len(STAR_COUNTS)
    boards, (rpi, rlogp, rv) = _reference(shape)
    ev = ops.C4StarEval(nnet.params, gnn.params, shape, A, 2, 8, dev)
    tag = f"star_eval/{shape[0]}x{shape[1]}"

    def run(bd, cnt, n, gpi, gv):
        for t in (ev.feat, ev.x0, ev.hidden, ev.glogp):
            t.fill_(float("nan"))
        ops.c4_star_eval(ev, bd, cnt, n, gpi=gpi, gv=gv)
        torch.cuda.synchronize()

    d_b = torch.from_numpy(boards).to(dev)
    d_c = torch.tensor(STAR_COUNTS, dtype=torch.int32, device=dev)
    gpi = torch.full((8, A), float("nan"), device=dev)
    gv = torch.full((8,), float("nan"), device=dev)
    run(d_b, d_c, B, gpi, gv)
    pi, v = gpi.cpu().numpy(), gv.cpu().numpy()
    assert np.isnan(pi[B:]).all() and np.isnan(v[B:]).all()
    for name, got, ref in (("pi", pi[:B], rpi), ("logp", ev.glogp[:B].cpu().numpy(), rlogp),
                           ("v", v[:B], rv)):
        worst = assert_close(f"{tag}/device/{name}", got, ref, TOL)
        print(f"{tag} device {name}: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")
    # mapped host memory
    hb = ops.HostBuffer(boards.nbytes + 4096)
    off = (boards.nbytes + 255) // 256 * 256
    h_b = hb.view(0, torch.int8, boards.shape)
    h_c = hb.view(off, torch.int32, (8,))
    h_pi = hb.view(off + 256, torch.float32, (8, A))
    h_v = hb.view(off + 256 + 1024, torch.float32, (8,))
    h_b.numpy()[...] = boards
    h_c.numpy()[:B] = STAR_COUNTS
    run(h_b, h_c, B, h_pi, h_v)
    assert np.array_equal(h_pi.numpy()[:B], pi[:B]) and np.array_equal(h_v.numpy()[:B], v[:B])
    # a star alone, and other values in the unused slots
    for b in range(B):
        run(d_b[b:b + 1].contiguous(), d_c[b:b + 1].contiguous(), 1, gpi, gv)
        assert np.array_equal(gpi[0].cpu().numpy(), pi[b]) and gv[0].item() == v[b], (shape, b)
    zeros = boards.copy()
    zeros[zeros == 2] = 0
    run(torch.from_numpy(zeros).to(dev), d_c, B, gpi, gv)
    assert np.array_equal(gpi.cpu().numpy()[:B], pi[:B]) and np.array_equal(gv.cpu().numpy()[:B], v[:B])
    del hb
    # the composition: features -> gnn_layer(save=False) per layer on a forest of stars ->
    # transform_heads on the row 0s
    lists = [boards[b, :n] for b, n in enumerate(STAR_COUNTS)]
    starts = np.concatenate([[0], np.cumsum(STAR_COUNTS)[:-1]])
    rowptr, col, e = np.zeros(sum(STAR_COUNTS) + 1, np.int64), [], 0
    for s, n in zip(starts, STAR_COUNTS):
        rowptr[s] = e
        e += n - 1
        rowptr[s + 1:s + n + 1] = e
        col += list(range(s + 1, s + n))
    g = ops.DeviceGraph(rowptr, np.asarray(col, np.int64), dev)
    x = nnet.features(torch.from_numpy(np.concatenate(lists)).to(dev))
    for layer in gnn.layers:
        x, _ = ops.gnn_layer(g, x, layer.weights(), save=False)
    clogp, cpi, cv = nets.gnn_per_row_heads(nnet, gnn, x[torch.as_tensor(starts, device=dev)].contiguous())
    for name, got, ref, one in (("pi", cpi, rpi, pi[:B]), ("logp", clogp, rlogp, None),
                                ("v", cv, rv, v[:B])):
        got = got.cpu().numpy()
        assert_close(f"{tag}/composition/{name}", got, ref, TOL)
        if one is not None:
            assert_close(f"{tag}/routes/{name}", got, one, 2 * TOL)


@pytest.mark.parametrize("shape", [(4, 4), (7, 6)])
@pytest.mark.parametrize("L", [0, 1, 3, 4])
def test_star_eval_at_other_depths(shape, L):
    """az_c4_star_eval_fwd with no layer (row 0 goes straight into output_transform), one, three
    and four (AZ_STAR_MAX_LAYERS) layers on the square and the rectangular trunk: stars of 8, 1
    and 5 boards, one evaluator per (shape, L), pi, log pi and v against float64."""
    from azhip import nets, ops
    torch.manual_seed(8600 + 100 * shape[0] + 10 * shape[1] + L)
    nnet = nets.Connect4Net(_game(shape), {"dropout": 0.0}).eval()
    gnn = nets.PolicyValueGNN(nnet.feature_dim, L).eval()
    assert len(gnn.layers) == L
    dev = nnet.params.device
    A, B = shape[0] + 1, len(STAR_COUNTS)
    boards = _star_boards(shape, STAR_COUNTS, 57 * shape[0] + shape[1] + L)
    lists = [boards[b, :n] for b, n in enumerate(STAR_COUNTS)]
    rpi, rlogp, rv = _float64_star_eval(lists, nnet.params, gnn.params, L)
    nnet.params.sync()
    gnn.params.sync()
    ev = ops.C4StarEval(nnet.params, gnn.params, shape, A, L, 8, dev)
    for t in (ev.feat, ev.x0, ev.hidden, ev.glogp):
        t.fill_(float("nan"))
    gpi = torch.full((8, A), float("nan"), device=dev)
    gv = torch.full((8,), float("nan"), device=dev)
    ops.c4_star_eval(ev, torch.from_numpy(boards).to(dev),
                     torch.tensor(STAR_COUNTS, dtype=torch.int32, device=dev), B, gpi=gpi, gv=gv)
    torch.cuda.synchronize()
    pi, v = gpi.cpu().numpy(), gv.cpu().numpy()
    assert np.isnan(pi[B:]).all() and np.isnan(v[B:]).all()
    tag = f"star_eval/{shape[0]}x{shape[1]}/L{L}"
    for name, got, ref in (("pi", pi[:B], rpi), ("logp", ev.glogp[:B].cpu().numpy(), rlogp),
                           ("v", v[:B], rv)):
        worst = assert_close(f"{tag}/{name}", got, ref, TOL)
        print(f"{tag} {name}: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")


# ------------------------------------------------------------------------------ the wrappers
def _wrapper(shape, layers=2, seed=0):
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Game import Connect4Game
    _NETS.clear()
    _GNN.clear()
    _REF.clear()
    _ORACLE.clear()
    torch.manual_seed(7500 + 100 * shape[0] + 10 * shape[1] + seed)
    rows = None if shape[0] == shape[1] else shape[1]
    return Connect4GNNWrapper(Connect4Game(shape[0], rows=rows),
                              SimpleNamespace(gnn_layers=layers, dropout=0.3))


def test_reference_star_positions(c4_gnn_weights):
    """The reference's own apply_policy_value_heads(gnn(extract_features(boards)))[0] on six
    recorded 7x7 positions of 2, 3, 5, 8, 8 and 8 nodes (tests/golden/c4_star_leaf.npz) through
    predict_with_gnn(board, neighbor_states=...): pi, log pi and v within 1e-5."""
    from azhip import wrappers
    z = golden("c4_star_leaf.npz")
    w = _wrapper((7, 7))
    w.nnet.load_state_dict({k: torch.from_numpy(v) for k, v in
                            split_weights(golden("c4_net.npz"), "w/").items()})
    w.gnn.load_state_dict({k: torch.from_numpy(v) for k, v in c4_gnn_weights.items()})
    for p, n in enumerate(z["counts"]):
        nodes = z["boards"][p, :n].astype(np.int64)
        pi, v = w.predict_with_gnn(nodes[0], neighbor_states=list(nodes[1:]))
        assert w.star_route == "onecall" and isinstance(w._star_direct, wrappers._StarDirect)
        assert_close(f"star_eval/reference/{p}/pi", pi, np.exp(z["logp"][p].astype(np.float64)), TOL)
        assert_close(f"star_eval/reference/{p}/logp", np.log(pi), z["logp"][p], TOL)
        assert_close(f"star_eval/reference/{p}/v", v, z["v"][p], TOL)


def test_wrapper_routes_and_star_batches(monkeypatch):
    """predict_with_gnn(board, neighbor_states=[]) is predict_with_gnn(board); predict_star_batch
    on 7x6 with 1 and 8 stars takes the one-call evaluator, with 9 stars or a 10-node star the
    composition, and under AZ_B1_MODE=graph / AZ_NO_ZEROCOPY=1 the composition; every result within
    1e-5 of float64, and a star of the 8-star call has the bits of the same star alone."""
    shape = (7, 6)
    w = _wrapper(shape)
    rng = np.random.default_rng(5)
    stars = [[b for b in rng.integers(-1, 2, size=(n,) + shape)]
             for n in (8, 2, 9, 1, 5, 8, 3, 8, 6)]
    big = [b for b in rng.integers(-1, 2, size=(10,) + shape)]
    a = w.predict_with_gnn(stars[0][0])
    for empty in ([], None):
        b = w.predict_with_gnn(stars[0][0], neighbor_states=empty)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert not hasattr(w, "star_route")
    rpi, _, rv = _float64_star_eval(stars + [big], w.nnet.params, w.gnn.params, 2)

    def check(tag, lists, idx, route):
        pi, v = w.predict_star_batch(lists)
        assert w.star_route == route, (tag, w.star_route)
        assert pi.shape == (len(lists), 8) and v.shape == (len(lists),)
        assert_close(f"star_eval/wrapper/{tag}/pi", pi, rpi[idx], TOL)
        assert_close(f"star_eval/wrapper/{tag}/v", v, rv[idx], TOL)
        return pi, v

    p1, v1 = check("1", stars[:1], [0], "onecall")
    p8, v8 = check("8", stars[:8], list(range(8)), "onecall")
    assert np.array_equal(p8[0], p1[0]) and v8[0] == v1[0]
    check("9", stars, list(range(9)), "composition")
    check("10nodes", [big, stars[1]], [9, 1], "composition")
    pi, v = w.predict_with_gnn(stars[4][0], neighbor_states=stars[4][1:])
    assert w.star_route == "onecall"
    assert np.array_equal(pi, p8[4]) and v == v8[4]
    for var, val in (("AZ_B1_MODE", "graph"), ("AZ_NO_ZEROCOPY", "1")):
        with monkeypatch.context() as m:
            m.setenv(var, val)
            check(f"{var}", stars[:2], [0, 1], "composition")


def test_five_layers_take_the_composition():
    """gnn_layers = 5 is beyond every star kernel (ops.STAR_MAX_LAYERS = 4): predict_star_batch on
    a 4x4 wrapper takes the composition on the generic graph calls, within 1e-5 of float64."""
    from azhip import ops
    shape = (4, 4)
    w = _wrapper(shape, layers=5)
    assert w.gnn.num_layers == 5 > ops.STAR_MAX_LAYERS
    rng = np.random.default_rng(11)
    stars = [[b for b in rng.integers(-1, 2, size=(n,) + shape)] for n in (5, 1, 3)]
    pi, v = w.predict_star_batch(stars)
    assert w.star_route == "composition"
    rpi, _, rv = _float64_star_eval(stars, w.nnet.params, w.gnn.params, 5)
    assert pi.shape == (3, 5) and v.shape == (3,)
    worst = assert_close("star_eval/wrapper/L5/pi", pi, rpi, TOL)
    worst_v = assert_close("star_eval/wrapper/L5/v", v, rv, TOL)
    print(f"star_eval wrapper L=5: pi max err {worst:.3g}, v max err {worst_v:.3g}")


def test_tictactoe_star_takes_the_composition():
    """A TicTacToe 3x3 star (the leaf and its 4 children) through TicTacToeGNNWrapper: the
    composition route, pi and v within 1e-5 of float64."""
    from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    torch.manual_seed(77)
    game = TicTacToeGame(3)
    w = TicTacToeGNNWrapper(game, SimpleNamespace(gnn_layers=2, dropout=0.3))
    board = np.array([[1, -1, 0], [0, 1, -1], [0, -1, 0]])
    valids = game.getValidMoves(board, 1)
    kids = [game.getCanonicalForm(*game.getNextState(board, 1, a))
            for a in range(game.getActionSize()) if valids[a]]
    assert len(kids) == 4
    pi, v = w.predict_with_gnn(board, neighbor_states=kids)
    assert w.star_route == "composition"
    rpi, _, rv = _float64_star_eval([[board] + kids], w.nnet.params, w.gnn.params, 2, heads="ttt")
    assert_close("star_eval/ttt3/pi", pi, rpi[0], TOL)
    assert_close("star_eval/ttt3/v", v, rv[0], TOL)


def test_search_with_gnn_neighbors_on_both_routes(monkeypatch):
    """25 simulations of getActionProb on the 7x6 opening with args.gnn_neighbors: the one-call
    route and the composition give the SAME root visit counts (their outputs differ by a few
    1e-7, which moved no UCB choice on these weights); every GNN evaluation carried the leaf's
    children."""
    from MCTS import MCTS
    w = _wrapper((7, 6), seed=3)
    args = SimpleNamespace(numMCTSSims=25, cpuct=1.0, use_gnn=True, gnn_neighbors=True)
    game = __import__("connect4.Connect4Game", fromlist=["Connect4Game"]).Connect4Game(7, rows=6)
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
    w.__dict__.pop("_g1", None)
    print("root counts", counts)
    report("star_eval/search_counts", **{k: [int(c) for c in v] for k, v in counts.items()})
    assert len(seen) > 0 and all(n >= 1 for n in seen)
    assert sum(counts["onecall"]) == 24
    assert counts["onecall"] == counts["composition"]
