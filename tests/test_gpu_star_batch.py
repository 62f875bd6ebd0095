"""Batched star evaluation on the MI355X: az_gnn_star_batch_infer (the layer stack on any number
of packed stars of any size) against float64 at every GEMM dispatch class the route reaches, the
reference's quirks and the rejected arguments, predict_both_stars on four boards (chunked and
unchunked), predict_star_batch's routes, and a short engine self-play run under
args.gnn_neighbors_lockstep.

Bar: atol 1e-5 on pi, log pi and v (the project's), and on the feature rows
az_gnn_star_batch_infer returns (values of order 1), as tests/test_gpu_star_eval.py holds
az_gnn_star_infer to."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import assert_close, report
from test_gpu_star_eval import _f64, _float64_star_eval

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
# (F, B): the GEMM dispatch class of the three B-row products (gate.0, update_net.0, update_net.2)
# and of the V-row attention projection
CASES = ((1024, 9), (1024, 70), (1024, 300), (1280, 70), (2688, 70), (3136, 70))

_GNN, _ORACLE = {}, {}


def _gnn(F, L=3):
    if (F, L) not in _GNN:
        from azhip import nets
        _GNN.clear()                              # one width's 0.7 GB at a time
        _ORACLE.clear()
        torch.manual_seed(9100 + F + L)
        _GNN[(F, L)] = nets.PolicyValueGNN(F, L).eval()
    return _GNN[(F, L)]


def _sizes(F, B):
    """Star sizes cycling through 1, 2, 3, 8, 9; at F = 1024 star 5 has 26 rows (TicTacToe 5x5's
    largest) and star 7 has 40 (more than the 32 weights a block keeps in LDS: the two-pass
    form)."""
    s = list(itertools.islice(itertools.cycle((1, 2, 3, 8, 9)), B))
    if F == 1024:
        s[5], s[7] = 26, 40
    return s


def _stars(F, B, seed=1):
    sizes = _sizes(F, B)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = np.random.default_rng(seed * 7919 + F).uniform(-1, 1, (int(offs[-1]), F))
    return x.astype(np.float32), offs


def _oracle(F, B):
    """rows[l][b]: row 0 of star b after l layers in float64 (oracle.nets.gnn_layer_star); the
    B = 9 and 70 cases at F = 1024 are the first stars of the 300-star set."""
    Bmax = 300 if F == 1024 else B
    if F not in _ORACLE:
        from oracle.nets import gnn_layer_star
        G64 = _f64(_gnn(F).params)
        x, offs = _stars(F, Bmax)
        cur = [x[offs[b]:offs[b + 1]].astype(np.float64) for b in range(Bmax)]
        rows = [np.stack([c[0] for c in cur])]
        for l in range(3):
            cur = [gnn_layer_star(c, G64, l) for c in cur]
            rows.append(np.stack([c[0] for c in cur]))
        _ORACLE[F] = rows
    return [r[:B] for r in _ORACLE[F]]


def _infer(gnn, x, offs, L, pad_rows=0, offs_tensor=None):
    """x0 of the call; pad_rows rows of NaN follow x in the same allocation."""
    from azhip import ops
    dev = gnn.params.device
    full = torch.full((x.shape[0] + pad_rows, x.shape[1]), float("nan"), device=dev)
    full[:x.shape[0]] = torch.from_numpy(x).to(dev)
    ot = torch.from_numpy(np.asarray(offs, np.int32)).to(dev) if offs_tensor is None \
        else offs_tensor
    out = torch.full((len(offs) - 1, x.shape[1]), float("nan"), device=dev)
    gnn.params.sync()
    keep = full.clone()
    ops.gnn_star_batch_infer(full[:x.shape[0]], ot, [l.weights() for l in gnn.layers[:L]],
                             out=out)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(full, nan=7.0), torch.nan_to_num(keep, nan=7.0))
    return out


@pytest.mark.parametrize("F,B", CASES)
def test_star_batch_infer_matches_float64(F, B):
    """L = 1, 2, 3 against oracle.nets.gnn_layer_star.  Dispatch classes (az_gemm.hip, M = rows):
      F 1024 B 9    B-row products on the fp32 MFMA tile (8 < M <= 64); projection M = V = 99 on
                    gemm_x3's 128x128 split-product tile
      F 1024 B 70   B-row products on gemm_x3's 128x128 tile (64 < M <= 256); projection M = 384
                    on its 256x128 tile
      F 1024 B 300  B-row products on gemm_x3's 256x128 tile (M > 256); projection M = 1,442
      F 1280 / 2688 / 3136 B 70   the 128x128 tile at K = 2F = 2,560 / 5,376 / 6,272, projection
                    (M = 322) on the 256x128 tile at K = F
    (B <= 8, the GEMV class, is test_star_batch_small_batches_and_gemv_rows.)
    Star sizes cycle through 1, 2, 3, 8, 9 (plus 26 and 40 rows at F = 1024); three rows of NaN
    follow x."""
    gnn = _gnn(F)
    x, offs = _stars(F, 300 if F == 1024 else B)
    offs = offs[:B + 1]
    x = x[:offs[-1]]
    ref = _oracle(F, B)
    for L in (1, 2, 3):
        got = _infer(gnn, x, offs, L, pad_rows=3).cpu().numpy()
        assert np.isfinite(got).all(), (F, B, L)
        worst = assert_close(f"star_batch/F{F}/B{B}/L{L}", got, ref[L], TOL)
        print(f"star_batch F={F} B={B} V={offs[-1]} L={L}: max err {worst:.3g} "
              f"({TOL / max(worst, 1e-300):.1f}x)")


def test_star_batch_small_batches_and_gemv_rows():
    """B = 1 .. 8 (the M <= 8 GEMV class) and a batch of one-row stars only."""
    F = 1024
    gnn = _gnn(F)
    x, offs = _stars(F, 300)
    ref = _oracle(F, 8)
    for B in (1, 5, 8):
        got = _infer(gnn, x[:offs[B]], offs[:B + 1], 2).cpu().numpy()
        assert_close(f"star_batch/F{F}/B{B}/L2", got, ref[2][:B], TOL)
    ones = np.arange(6, dtype=np.int32)
    got = _infer(gnn, x[:5], ones, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(x[:5]))


def test_star_batch_quirks():
    """One-row stars return their row (torch.equal) at L = 0 and L = 3 among large stars; with
    attention.2.bias = -200 every weight underflows to 0 in fp32, the aggregate is 0 and the row
    is the float64 node update with agg = 0; x is never modified (checked in _infer); two calls
    give equal bits; a call from mapped host offs equals the call from device offs."""
    from azhip import ops
    from oracle.nets import _layer, node_update
    F, B = 1024, 70
    gnn = _gnn(F)
    x, offs = _stars(F, 300)
    offs = offs[:B + 1]
    x = x[:offs[-1]]
    sizes = np.diff(offs)
    single = np.flatnonzero(sizes == 1)
    assert len(single) >= 10 and sizes.max() == 40
    rows0 = torch.from_numpy(x[offs[:-1]])
    got0 = _infer(gnn, x, offs, 0).cpu()
    assert torch.equal(got0, rows0)
    got3 = _infer(gnn, x, offs, 3)
    assert torch.equal(got3.cpu()[single], rows0[single])
    assert torch.equal(got3, _infer(gnn, x, offs, 3))
    hb = ops.HostBuffer(4096)
    ho = hb.view(0, torch.int32, (B + 1,))
    ho.numpy()[:] = offs
    assert torch.equal(got3, _infer(gnn, x, offs, 3, offs_tensor=ho))
    bias = gnn.params["layers.0.attention.2.bias"]
    keep = bias.clone()
    try:
        bias.fill_(-200.0)
        got = _infer(gnn, x, offs, 1).cpu().numpy()
    finally:
        bias.copy_(keep)
    L0 = _layer(_f64(gnn.params), 0, np.float64)
    t = x[offs[:-1]].astype(np.float64)
    want = node_update(t, np.zeros_like(t), L0)
    want[single] = t[single]
    worst = assert_close("star_batch/zero_weights", got, want, TOL)
    print(f"star_batch zero weights: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")
    assert np.array_equal(got[single], x[offs[:-1]][single])


def test_star_batch_rejected_arguments():
    """Every rejected argument returns AZ_EINVAL with a message and launches nothing (x0 keeps its
    NaNs).  offs is checked on the host when it is mapped host memory; only such host-checked
    rejections are exercised (no bad offs ever reaches the device)."""
    import ctypes
    from azhip import _lib, ops
    F, B = 1024, 4
    gnn = _gnn(F)
    dev = gnn.params.device
    L = _lib.lib()
    x = torch.zeros((20, F), device=dev)
    x0 = torch.full((B, F), float("nan"), device=dev)
    nb = int(L.az_gnn_star_batch_ws_bytes(B, 20, F, 128, 2))
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    lw = (ops.LayerW * 2)(*[ops.layer_weights(l.weights()) for l in gnn.layers[:2]])
    hb = ops.HostBuffer(4096)
    ho = hb.view(0, torch.int32, (B + 1,))
    good = [0, 5, 6, 15, 20]
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(offs=good, xp=None, x0p=None, wsp=None, nbytes=nb, Bc=B, V=20, Fc=F, H=128, Lc=2,
             layers=lw):
        ho.numpy()[:] = offs
        return L.az_gnn_star_batch_infer(
            P(x) if xp is None else xp, P(ho), Bc, V, Fc, H, Lc, layers,
            P(x0) if x0p is None else x0p, P(ws) if wsp is None else wsp,
            ctypes.c_size_t(nbytes), None)

    bad = [(dict(offs=[0, 5, 5, 15, 20]), b"not ascending"),
           (dict(offs=[0, 5, 4, 15, 20]), b"not ascending"),
           (dict(offs=[1, 5, 6, 15, 20]), b"offs[0]"),
           (dict(offs=[0, 5, 6, 15, 19]), b"offs[0]"),
           (dict(nbytes=nb - 1), b"too small"),
           (dict(xp=ctypes.c_void_p(x.data_ptr() + 4)), b"alignment"),
           (dict(x0p=ctypes.c_void_p(x0.data_ptr() + 8)), b"alignment"),
           (dict(wsp=ctypes.c_void_p(ws.data_ptr() + 4)), b"alignment"),
           (dict(xp=ctypes.c_void_p(0)), b"null"),
           (dict(x0p=P(x)), b"alias"),
           (dict(Fc=1000), b"bad shape"), (dict(H=126), b"bad shape"), (dict(Lc=5), b"bad shape"),
           (dict(V=3), b"bad shape"),
           (dict(layers=(ops.LayerW * 2)()), b"null weight")]
    failed = []

    def run():
        try:
            for kw, msg in bad:
                assert call(**kw) == -1, kw
                assert msg in L.az_last_error(), (kw, L.az_last_error())
        except BaseException as ex:   # reported on the test's own thread
            failed.append(ex)

    # az_last_error is per thread: the rejected calls run on a thread of their own, so the main
    # thread keeps the empty message tests/test_lib_abi.py expects whatever the test order
    import threading
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failed:
        raise failed[0]
    torch.cuda.synchronize()
    assert torch.isnan(x0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(x0).all()
    assert call(Bc=0) == 0


@pytest.mark.parametrize("B", [9, 70])
def test_star_batch_infer_four_layers(B):
    """L = 4, the deepest stack az_gnn_star_batch_infer accepts (AZ_STAR_MAX_LAYERS), at F = 1024
    on a four-layer net of its own: the fp32 MFMA tile (B = 9) and gemm_x3's 128x128 tile
    (B = 70), three rows of NaN after x."""
    from oracle.nets import gnn_layer_star
    F = 1024
    gnn = _gnn(F, 4)
    assert len(gnn.layers) == 4
    x, offs = _stars(F, 300)
    offs = offs[:B + 1]
    x = x[:offs[-1]]
    G64 = _f64(gnn.params)
    cur = [x[offs[b]:offs[b + 1]].astype(np.float64) for b in range(B)]
    for l in range(4):
        cur = [gnn_layer_star(c, G64, l) for c in cur]
    got = _infer(gnn, x, offs, 4, pad_rows=3).cpu().numpy()
    assert np.isfinite(got).all()
    worst = assert_close(f"star_batch/F{F}/B{B}/L4", got, np.stack([c[0] for c in cur]), TOL)
    print(f"star_batch F={F} B={B} V={offs[-1]} L=4: max err {worst:.3g} "
          f"({TOL / max(worst, 1e-300):.1f}x)")


# ------------------------------------------------------------------------------ the wrappers
def _wrapper(kind, shape, seed=0, **extra):
    _GNN.clear()
    _ORACLE.clear()
    torch.manual_seed(7700 + 100 * shape[0] + 10 * shape[1] + seed)
    args = SimpleNamespace(gnn_layers=2, dropout=0.3, **extra)
    if kind == "ttt":
        from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
        from tictactoe.TicTacToeGame import TicTacToeGame
        game = TicTacToeGame(shape[0])
        return game, TicTacToeGNNWrapper(game, args)
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Game import Connect4Game
    game = Connect4Game(shape[0], rows=None if shape[0] == shape[1] else shape[1])
    return game, Connect4GNNWrapper(game, args)


def _children(game, board):
    from MCTS import MCTS
    return MCTS(game, None, SimpleNamespace()).leaf_children(board)


def _positions(game, n, seed):
    """n reachable non-terminal canonical positions with mixed child counts: the opening first,
    then random play of growing length."""
    rng = np.random.default_rng(seed)
    cells = int(np.prod(game.getBoardSize()))
    A = game.getActionSize()
    by_count = {}
    for _ in range(300):
        b, p = game.getInitBoard(), 1
        # moves kept to a few actions where possible, so that columns fill up
        allowed = set(rng.choice(A - 1, size=rng.integers(2, A), replace=False).tolist())
        for _ in range(rng.integers(1, cells)):
            valid = np.flatnonzero(game.getValidMoves(b, p))
            pick = [a for a in valid if a in allowed] or list(valid)
            nb, q = game.getNextState(b, p, rng.choice(pick))
            if game.getGameEnded(nb, q) != 0:
                break
            b, p = nb, q
        c = game.getCanonicalForm(b, p)
        by_count.setdefault(int(np.sum(game.getValidMoves(c, 1))), []).append(c)
    out = [game.getCanonicalForm(game.getInitBoard(), 1)]
    while len(out) < n:                   # round-robin over the child counts
        for k in sorted(by_count):
            if by_count[k] and len(out) < n:
                out.append(by_count[k].pop())
    return out


def _float64_std(boards, W, heads):
    """Trunk and standard heads of the leaves in float64."""
    import torch.nn.functional as Fn
    from oracle import nets as O
    Wn = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in W.views.items()}
    t = lambda k: torch.from_numpy(Wn[k])  # noqa: E731
    xb = torch.from_numpy(np.asarray(boards)).double()[:, None]
    xb = Fn.relu(Fn.conv2d(xb, t("conv1.weight"), t("conv1.bias"), padding=1))
    xb = Fn.relu(Fn.conv2d(xb, t("conv2.weight"), t("conv2.bias"), padding=1))
    if heads == "ttt":
        xb = Fn.relu(Fn.conv2d(xb, t("conv3.weight"), t("conv3.bias"), padding=0))
    logp, v = (O.c4_heads if heads == "c4" else O.ttt_heads)(xb.flatten(1).numpy(), Wn)
    return np.exp(logp), logp, v


def _three_chunk_budget(wrappers, offs, F):
    cr, cs, fixed = wrappers._star_chunk_cost(F)
    lin = cr * np.asarray(offs, np.int64) + cs * np.arange(len(offs))
    for b in range(1, len(offs)):
        budget = fixed + int(lin[b])
        if len(wrappers.star_chunks(offs, F, budget)) == 3:
            return budget
    raise AssertionError("no budget splits these stars into 3 chunks")


@pytest.mark.parametrize("kind,shape", [("c4", (4, 4)), ("c4", (7, 6)), ("c4", (7, 7)),
                                        ("ttt", (3, 3))])
def test_predict_both_stars_matches_float64(kind, shape, monkeypatch):
    """12 real positions with mixed child counts (TicTacToe 3x3: the empty board's 10-node star)
    against float64 trunk -> layers on the star -> output_transform -> heads of row 0, and the
    standard heads of the leaf; then the same call with the chunk budget small enough to split the
    12 stars into 3 chunks: within the bar of float64 too (its bits may differ from the unchunked
    call, whose GEMMs see other row counts)."""
    import mcts_native
    from azhip import wrappers
    game, w = _wrapper(kind, shape)
    boards = _positions(game, 12, 40 + shape[0] + shape[1])
    stars = [[np.asarray(b)] + _children(game, b) for b in boards]
    sizes = [len(s) for s in stars]
    assert len(set(sizes)) >= 3, sizes
    if kind == "ttt":
        assert max(sizes) == 10
    rows, offs = mcts_native.game_stars(*mcts_native.game_shape(game),
                                        np.stack(boards).astype(np.int8))
    assert np.array_equal(rows, np.stack([r for s in stars for r in s]))
    gref = _float64_star_eval(stars, w.nnet.params, w.gnn.params, 2, heads=kind)
    sref = _float64_std(np.stack(boards), w.nnet.params, kind)
    tag = f"star_batch/{kind}{shape[0]}x{shape[1]}"

    def check(sub, out):
        pi, v, gpi, gv = out
        A = game.getActionSize()
        assert pi.shape == gpi.shape == (12, A) and v.shape == gv.shape == (12,)
        for name, got, ref in (("pi", pi, sref[0]), ("logp", np.log(pi), sref[1]),
                               ("v", v, sref[2]), ("gpi", gpi, gref[0]),
                               ("glogp", np.log(gpi), gref[1]), ("gv", gv, gref[2])):
            worst = assert_close(f"{tag}/{sub}/{name}", got, ref, TOL)
            print(f"{tag} {sub} {name}: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")

    one = w.predict_both_stars(rows, offs)
    check("whole", one)
    again = w.predict_both_stars_async(rows, offs).result()
    assert all(np.array_equal(a, b) for a, b in zip(one, again))
    budget = _three_chunk_budget(wrappers, offs, w.feature_dim)
    monkeypatch.setattr(wrappers, "STAR_CHUNK_BYTES", budget)
    assert len(wrappers.star_chunks(offs, w.feature_dim)) == 3
    check("chunked", w.predict_both_stars(rows, offs))


def test_predict_star_batch_routes():
    """7x6 under args.gnn_neighbors_lockstep: 8 stars of <= 9 nodes take the one-call evaluator (a
    star's bits those of the star alone), 9 stars and a 10-node star the batched route; all within
    1e-5 of float64.  Without the key the same wrapper routes 9 stars as it always did (the
    composition, tests/test_gpu_star_eval.py)."""
    game, w = _wrapper("c4", (7, 6), seed=2, use_gnn=True, gnn_neighbors=True,
                       gnn_neighbors_lockstep=True)
    rng = np.random.default_rng(5)
    shape = (7, 6)
    stars = [[b for b in rng.integers(-1, 2, size=(n,) + shape)]
             for n in (8, 2, 9, 1, 5, 8, 3, 8, 6)]
    big = [b for b in rng.integers(-1, 2, size=(10,) + shape)]
    rpi, _, rv = _float64_star_eval(stars + [big], w.nnet.params, w.gnn.params, 2)

    def check(tag, lists, idx, route):
        pi, v = w.predict_star_batch(lists)
        assert w.star_route == route, (tag, w.star_route)
        assert_close(f"star_batch/routes/{tag}/pi", pi, rpi[idx], TOL)
        assert_close(f"star_batch/routes/{tag}/v", v, rv[idx], TOL)
        return pi, v

    p1, v1 = check("1", stars[:1], [0], "onecall")
    p8, v8 = check("8", stars[:8], list(range(8)), "onecall")
    assert np.array_equal(p8[0], p1[0]) and v8[0] == v1[0]
    check("9", stars, list(range(9)), "batched")
    check("10nodes", [big, stars[1]], [9, 1], "batched")
    w.args.gnn_neighbors_lockstep = False
    check("9/no_key", stars, list(range(9)), "composition")
    check("8/no_key", stars[:8], list(range(8)), "onecall")


def test_engine_selfplay_with_stars():
    """Connect4 4x4, 8 episodes, 6 simulations, expand_by 1, G = 4 on two lanes under
    gnn_neighbors_lockstep: every episode finishes with GNN examples, every network call was a
    predict_both_stars whose stars are the Python leaf_children of its leaves, nn_fallback counted
    nothing.  The action agreement with the sequential Python search (batch-1 star calls, other
    bits) is reported, not asserted."""
    import nn_fallback
    from Coach import Coach
    from selfplay import episode_seeds, play_episodes_engine
    game, w = _wrapper("c4", (4, 4), seed=4)
    args = SimpleNamespace(numEps=8, numMCTSSims=6, cpuct=1.0, tempThreshold=4, use_gnn=True,
                           expand_by=1, gnn_neighbors=True, gnn_neighbors_lockstep=True,
                           gnn_layers=2, dropout=0.3, parallel_games=4)
    calls = []
    orig = w.predict_both_stars_async

    def spy(rows, offs, stream=None):
        calls.append((np.array(rows), np.array(offs)))
        return orig(rows, offs, stream=stream)

    def never(*a, **k):
        raise AssertionError("a star-less network call under gnn_neighbors_lockstep")

    w.predict_both_stars_async = spy
    w.predict_both_async = w.predict_both = w.predict_batch_async = never
    eps = list(range(8))
    seeds = episode_seeds(11, eps)
    nn_fallback.reset()
    out = play_episodes_engine(game, w, args, eps, seeds, parallel_games=4, threads=2, lanes=2)
    assert sorted(out) == eps and nn_fallback.total() == 0
    assert all(len(out[e][0]) > 0 and len(out[e][1]) > 0 for e in eps)
    assert len(calls) > 0
    for rows, offs in calls:
        assert offs[0] == 0 and offs[-1] == len(rows)
        for b in range(len(offs) - 1):
            want = [rows[offs[b]]] + _children(game, rows[offs[b]])
            got = rows[offs[b]:offs[b + 1]]
            assert len(got) == len(want) and all(np.array_equal(x, y) for x, y in zip(got, want))
    # the sequential run of the same seeds: leading example boards that agree
    del w.predict_both_stars_async, w.predict_both_async, w.predict_both, w.predict_batch_async
    agree = total = 0
    for e in eps[:3]:
        np.random.seed(seeds[e])
        std, _ = Coach(game, w, args).executeEpisode()
        a = [np.asarray(x[0]).tolist() for x in std]
        b = [np.asarray(x[0]).tolist() for x in out[e][0]]
        total += max(len(a), len(b))
        agree += next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    print(f"engine stars vs sequential: {agree}/{total} leading example boards agree; "
          f"{len(calls)} star calls, {sum(len(o) - 1 for _, o in calls)} stars")
    report("star_batch/engine_agreement", agree=agree, total=total, calls=len(calls))
    assert nn_fallback.total() == 0
