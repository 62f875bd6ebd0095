"""Batch-invariant star evaluation on the MI355X (config key batch_invariant with gnn_neighbors;
DESIGN §10): the exact GEMM's node-update epilogues against the CPU chain (tests/exact_ref.py), the
exact layer stack's invariance and accuracy, the one-call evaluator's three promises, the wrappers'
exact star route, and lock-step self-play with stars that equals the sequential search.

Invariance is asserted with torch.equal / np.array_equal; accuracy is held to the project's 1e-5
bar against the float64 oracle of tests/test_gpu_star_batch.py."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import exact_ref
from conftest import assert_close, report
from test_gpu_exact import _padded
from test_gpu_star_batch import (_children, _float64_std, _gnn, _oracle, _positions, _stars,
                                 _wrapper)
from test_gpu_star_eval import _float64_star_eval

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
NAN = float("nan")
EPI_SHAPES = [(36, 36), (132, 260)]
EPI_ROWS = (1, 33, 65)


# ------------------------------------------------------------------ 1. the epilogues
def _operands(N, K, M, seed=0):
    rng = np.random.default_rng(1000 * N + K + seed)
    f = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return dict(A=f(M, K), W=f(N, K), b=f(N), W2=f(N, K), b2=f(N), G=f(M, N), R=f(M, 2 * N))


def _fma_rows(G, v, R):
    out = np.empty_like(v)
    for i, j in itertools.product(range(v.shape[0]), range(v.shape[1])):
        out[i, j] = exact_ref.fma32(G[i, j], v[i, j], R[i, j])
    return out


def _dev_ops(o, M, dev):
    """The operands on the device, NaN behind every one of them (rows past M / N, k past K)."""
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d = dict(A=_padded(o["A"][:M], 130, dev), W=_padded(o["W"], 70, dev),
             W2=_padded(o["W2"], 70, dev), b=t(o["b"]), b2=t(o["b2"]),
             G=_padded(o["G"][:M], 3, dev))
    Rbuf = torch.full((M + 3, o["R"].shape[1]), NAN, device=dev)
    Rbuf[:M] = t(o["R"][:M])
    d["R"] = Rbuf[:M, :o["W"].shape[0]]                   # ldr = 2N
    return d


def _out(M, N, dev):
    return torch.full((M + 8, N), NAN, device=dev)


def _rows(out, M):
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[M:]).all()                       # nothing stored past row M
    return got[:M]


@pytest.mark.parametrize("N,K", EPI_SHAPES)
def test_epilogues_equal_cpu_chain(N, K):
    """Gated residual, the paired launch and sigmoid at M = 1, 33, 65 with NaN behind the operands
    (test_gpu_exact._padded), each against exact_ref's chain."""
    from azhip import ops
    if exact_ref.lib() is None:
        pytest.skip("no C++ compiler")
    dev = torch.device("cuda")
    Mmax = max(EPI_ROWS)
    o = _operands(N, K, Mmax)
    lin = exact_ref.linear(o["A"], o["W"], o["b"])
    want_gated = _fma_rows(o["G"], lin, o["R"][:, :N])
    want_relu = exact_ref.linear(o["A"], o["W"], o["b"], relu=True)
    want_plain = exact_ref.linear(o["A"], o["W2"], o["b2"])
    sig_rows = {}
    for M in EPI_ROWS:
        d = _dev_ops(o, M, dev)
        # gated residual, R at ldr = 2N
        out = _out(M, N, dev)
        ops.linear_exact_ex(d["A"], d["W"], d["b"], out=out, M=M, R=d["R"], G=d["G"])
        assert np.array_equal(_rows(out, M), want_gated[:M]), (N, K, M, "gated")
        # paired: one ReLU output, one plain
        o1, o2 = _out(M, N, dev), _out(M, N, dev)
        ops.linear_exact_ex(d["A"], d["W"], d["b"], act=ops.ACT_RELU, out=o1, M=M, w2=d["W2"],
                            b2=d["b2"], act2=ops.ACT_NONE, out2=o2)
        g1, g2 = _rows(o1, M), _rows(o2, M)
        assert np.array_equal(g1, want_relu[:M]), (N, K, M, "pair/relu")
        assert np.array_equal(g2, want_plain[:M]), (N, K, M, "pair/plain")
        s1 = ops.linear_exact(d["A"], d["W"], d["b"], ops.ACT_RELU, M=M)
        s2 = ops.linear_exact(d["A"], d["W2"], d["b2"], ops.ACT_NONE, M=M)
        assert torch.equal(o1[:M], s1) and torch.equal(o2[:M], s2), (N, K, M, "pair/separate")
        # sigmoid
        out = _out(M, N, dev)
        ops.linear_exact_ex(d["A"], d["W"], d["b"], act=ops.ACT_SIGMOID, out=out, M=M)
        got = _rows(out, M)
        sig_rows[M] = out[:M].clone()
        ref = 1.0 / (1.0 + np.exp(-lin[:M].astype(np.float64)))
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print(f"sigmoid N={N} K={K} M={M}: max err {err:.3g} vs float64 sigmoid of the chain")
        report(f"star_exact/sigmoid/N{N}/K{K}/M{M}", max_err=err, tol=1e-6)
        assert err <= 1e-6, (N, K, M, err)
        assert (got > 0).all() and (got <= 1).all()
    for M in EPI_ROWS[:-1]:
        assert torch.equal(sig_rows[M], sig_rows[Mmax][:M]), (N, K, M, "sigmoid rows")


def test_epilogues_spread_and_direct_agree():
    """N = 1024, K = 2048: M = 40 runs spread over the segments (slabs and the reduce kernel's
    epilogue), M = 900 direct (8 row tiles x 16 column tiles; the paired launch is direct from 4
    row tiles on).  The 40 rows of one call equal the other's, for all three epilogues."""
    from azhip import _lib, ops
    dev = torch.device("cuda")
    N, K, Ms, Md = 1024, 2048, 40, 900
    L = _lib.lib()
    need = L.az_gemm_exact_ex_ws_bytes
    assert need(Ms, N, K, 0) > 0 and need(Ms, N, K, 1) > 0
    assert need(Md, N, K, 0) == 0 and need(896, N, K, 0) > 0 and need(Md, N, K, 1) == 0
    o = _operands(N, K, Md)
    t = {k: torch.from_numpy(v).to(dev) for k, v in o.items()}
    R = t["R"][:, :N]
    res = {}
    for M in (Ms, Md):
        gated = ops.linear_exact_ex(t["A"][:M], t["W"], t["b"], R=R[:M], G=t["G"][:M])
        sig, relu = ops.linear_exact_ex(t["A"][:M], t["W"], t["b"], act=ops.ACT_SIGMOID,
                                        w2=t["W2"], b2=t["b2"], act2=ops.ACT_RELU)
        one = ops.linear_exact_ex(t["A"][:M], t["W"], t["b"], act=ops.ACT_SIGMOID)
        torch.cuda.synchronize()
        assert torch.equal(one, sig), M                   # paired == single, spread and direct
        res[M] = (gated, sig, relu)
    for a, b, name in zip(res[Ms], res[Md], ("gated", "sigmoid", "relu")):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b[:Ms]), name
    want = ops.linear_exact(t["A"][:Ms], t["W2"], t["b2"], ops.ACT_RELU)
    assert torch.equal(res[Ms][2], want)


# ------------------------------------------------------------------ 2. layer stack invariance
SIZES = (1, 2, 5, 9, 33, 34, 40)


def _exact_infer(gnn, x, offs, L, offs_tensor=None):
    """x0 of az_gnn_star_batch_exact_infer; x (a device tensor) is left unchanged."""
    from azhip import ops
    dev = gnn.params.device
    ot = torch.from_numpy(np.asarray(offs, np.int32)).to(dev) if offs_tensor is None \
        else offs_tensor
    out = torch.full((len(offs) - 1, x.shape[1]), NAN, device=dev)
    gnn.params.sync()
    ops.gnn_star_batch_exact_infer(x, ot, [l.weights() for l in gnn.layers[:L]], out=out)
    torch.cuda.synchronize()
    return out


def _pack(stars, order, dev):
    """The stars `order` names packed into one x, and their offs."""
    x = torch.cat([stars[i] for i in order])
    offs = np.concatenate([[0], np.cumsum([stars[i].shape[0] for i in order])]).astype(np.int32)
    return x.to(dev), offs


def _orders(P, B):
    """The packs of B stars that carry the P probes (stars 0 .. P-1) away from position 0 where
    there is room: pairs of probes in swapped order for B = 2, else one pack of fillers (stars P ..)
    with the probes spread through it."""
    if B <= P:
        return [[p + 1, p] for p in range(0, P - 1, 2)]
    order = list(range(P, B))
    step = max(1, (B - 1) // P)
    for k in range(P):
        order.insert(1 + k * step, k)
    return [order]


def _invariance(F, L, packs, probe_sizes, filler_count, seed):
    """Probe stars alone (B = 1), then inside every pack of `packs` (B stars each) at other
    positions, then inside two packs split at a probe star: torch.equal throughout."""
    gnn = _gnn(F, 3)
    dev = gnn.params.device
    gen = torch.Generator().manual_seed(seed)
    sizes = list(probe_sizes) + list(itertools.islice(itertools.cycle(SIZES), filler_count))
    stars = [torch.rand((n, F), generator=gen) * 2 - 1 for n in sizes]
    P = len(probe_sizes)
    alone = []
    for p in range(P):
        x, offs = _pack(stars, [p], dev)
        keep = x.clone()
        alone.append(_exact_infer(gnn, x, offs, L)[0])
        assert torch.equal(x, keep)                       # x is never written
        assert torch.isfinite(alone[p]).all()
        if sizes[p] == 1:
            assert torch.equal(alone[p], x[0])            # a one-row star: its row, bit for bit
        else:
            assert not torch.equal(alone[p], x[0])
    for B, order in ((B, o) for B in packs for o in _orders(P, B)):
        where = {i: pos for pos, i in enumerate(order) if i < P}
        x, offs = _pack(stars, order, dev)
        got = _exact_infer(gnn, x, offs, L)
        for p, pos in where.items():
            assert torch.equal(got[pos], alone[p]), (F, L, B, int(offs[-1]), p, pos)
        if B == 900:
            assert int(offs[-1]) >= 3969                  # the projection runs direct too
        if B == 65:
            # the same stars as two packs split at a probe star
            cut = int(where[min(3, P - 1)])
            lo = _exact_infer(gnn, x[:int(offs[cut])], offs[:cut + 1], L)
            hi = _exact_infer(gnn, x[int(offs[cut]):], offs[cut:] - offs[cut], L)
            assert torch.equal(torch.cat([lo, hi]), got), (F, L, "split")
        del x, got
    return alone


@pytest.mark.parametrize("L", [1, 3])
def test_layer_stack_is_invariant(L):
    """F = 1024, H = 128.  L = 1 writes x0 directly, L = 3 exercises Pt.  Six probe stars of 1, 2,
    9, 34 (the first size that tiles the weights twice), 40 and 5 rows among fillers of 1, 2, 5, 9,
    33, 34 and 40 rows: alone, then in packs of B = 2, 33, 65 and 900 (V >= 3,969: every product
    direct) and in two packs split at a probe."""
    _invariance(1024, L, (2, 33, 65, 900), (1, 2, 9, 34, 40, 5), 900, 17 + L)


def test_layer_stack_is_invariant_at_3136():
    """F = 3136 (7x7), L = 2, B = 1 against B = 40."""
    _invariance(3136, 2, (40,), (1, 2, 9, 34), 40, 23)


# ------------------------------------------------------------------ 3. layer stack accuracy
@pytest.mark.parametrize("F,B", [(1024, 70), (3136, 9)])
def test_layer_stack_matches_float64(F, B):
    """L = 3 against oracle.nets.gnn_layer_star on test_gpu_star_batch's stars, the 1e-5 bar."""
    gnn = _gnn(F)
    x, offs = _stars(F, 300 if F == 1024 else B)
    offs = offs[:B + 1]
    x = x[:offs[-1]]
    ref = _oracle(F, B)
    got = _exact_infer(gnn, torch.from_numpy(x).to(gnn.params.device), offs, 3).cpu().numpy()
    assert np.isfinite(got).all()
    worst = assert_close(f"star_exact/F{F}/B{B}/L3", got, ref[3], TOL)
    print(f"star_exact F={F} B={B} V={offs[-1]} L=3: max err {worst:.3g} "
          f"({TOL / max(worst, 1e-300):.1f}x)")
    report(f"star_exact/margin/F{F}/B{B}", max_err=worst, margin=TOL / max(worst, 1e-300))


# ------------------------------------------------------------------ 4. the evaluator
def _game_stars(kind, shape, game, n, seed):
    """n stars of real positions with their children; star 1 is a childless leaf (one row), and on
    4x4 star 2 is a synthetic star of 40 rows."""
    boards = _positions(game, n, seed)
    stars = [[np.asarray(b, np.int8)] + [np.asarray(c, np.int8) for c in _children(game, b)]
             for b in boards]
    stars[1] = stars[1][:1]
    if kind == "c4" and shape == (4, 4):
        rng = np.random.default_rng(seed)
        stars[2] = [b for b in rng.integers(-1, 2, size=(40,) + shape).astype(np.int8)]
    return stars


def _packed(stars):
    rows = np.stack([r for s in stars for r in s]).astype(np.int8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in stars])]).astype(np.int32)
    return rows, offs


def _star_eval(ev, stars, dev, host=None):
    """(pi, v, gpi, gv) numpy of az_star_eval_exact_fwd from device buffers (host None) or from
    one mapped host buffer."""
    from azhip import ops
    rows, offs = _packed(stars)
    B, V, A = len(stars), len(rows), ev.A
    if host is None:
        r, o = torch.from_numpy(rows).to(dev), torch.from_numpy(offs).to(dev)
        outs = [torch.full(s, NAN, device=dev) for s in ((B, A), (B,), (B, A), (B,))]
    else:
        cell = rows[0].size
        off = [0]
        for nb in (V * cell, 4 * (B + 1), 4 * B * A, 4 * B, 4 * B * A, 4 * B):
            off.append(off[-1] + (nb + 255) // 256 * 256)
        assert off[-1] <= host.nbytes
        r = host.view(off[0], torch.int8, rows.shape)
        o = host.view(off[1], torch.int32, (B + 1,))
        outs = [host.view(off[2 + j], torch.float32, s)
                for j, s in enumerate(((B, A), (B,), (B, A), (B,)))]
        r.numpy()[:] = rows
        o.numpy()[:] = offs
        for t in outs:
            t.fill_(NAN)
    ops.star_eval_exact(ev, r, o, B, V, *outs)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in outs)


@pytest.mark.parametrize("kind,shape", [("c4", (4, 4)), ("c4", (7, 6)), ("c4", (7, 7)),
                                        ("ttt", (4, 4))])
def test_star_evaluator_promises(kind, shape):
    """B = 1, 9 and 70 stars (70 stars are more than 320 rows on 7x7: the trunk's form switch).
    A star's four rows are the same bits alone, at another position of a larger pack, across calls
    and from mapped host memory; pi / v equal az_eval_exact_fwd's of the leaf board; a one-row
    star's gpi / gv equal az_eval_exact_fwd's of that board; all within 1e-5 of float64."""
    from azhip import ops
    game, w = _wrapper(kind, shape, seed=6)
    dev = w.device
    W, G = w.nnet.params, w.gnn.params
    W.sync()
    G.sync()
    A = game.getActionSize()
    stars = _game_stars(kind, shape, game, 70, 60 + shape[0] + shape[1])
    nine = stars[:9]
    assert len(nine[1]) == 1 and len({len(s) for s in nine}) >= 3
    ev = ops.StarEvalExact(W, G, ops.exact_board(w.nnet), A, 2, 128, 2048, dev)
    pack9 = _star_eval(ev, nine, dev)
    assert all(np.isfinite(a).all() for a in pack9)
    # alone, and across calls
    for b in range(9):
        one = _star_eval(ev, nine[b:b + 1], dev)
        for k in range(4):
            assert np.array_equal(one[k][0], pack9[k][b]), (kind, shape, "alone", b, k)
    again = _star_eval(ev, nine, dev)
    assert all(np.array_equal(a, b) for a, b in zip(pack9, again))
    # 70 stars, the nine at the end in reverse order
    big = stars[9:] + nine[::-1]
    assert sum(len(s) for s in big) > (320 if shape == (7, 7) else 70)
    pack70 = _star_eval(ev, big, dev)
    for b in range(9):
        for k in range(4):
            assert np.array_equal(pack70[k][69 - b], pack9[k][b]), (kind, shape, "pack70", b, k)
    # mapped host memory
    hb = ops.HostBuffer(1 << 20)
    from_host = _star_eval(ev, big, dev, host=hb)
    assert all(np.array_equal(a, b) for a, b in zip(pack70, from_host))
    # the leaf boards through az_eval_exact_fwd
    leaves = torch.from_numpy(np.stack([s[0] for s in big]).astype(np.int8)).to(dev)
    ee = ops.EvalExact(W, G, ops.exact_board(w.nnet), A, 128, dev)
    outs = [torch.full(s, NAN, device=dev) for s in ((70, A), (70,), (70, A), (70,))]
    ops.eval_exact(ee, leaves, 70, *outs)
    torch.cuda.synchronize()
    lpi, lv, lgpi, lgv = (t.cpu().numpy() for t in outs)
    assert np.array_equal(pack70[0], lpi) and np.array_equal(pack70[1], lv)
    single = [b for b, s in enumerate(big) if len(s) == 1]
    assert single
    for b in single:
        assert np.array_equal(pack70[2][b], lgpi[b]) and pack70[3][b] == lgv[b]
    many = [b for b, s in enumerate(big) if len(s) > 1]
    assert not np.array_equal(pack70[2][many], lgpi[many])   # the children do count
    # float64
    gref = _float64_star_eval(nine, W, G, 2, heads=kind)
    sref = _float64_std(np.stack([s[0] for s in nine]), W, kind)
    tag = f"star_exact/eval/{kind}{shape[0]}x{shape[1]}"
    pi, v, gpi, gv = pack9
    for name, got, ref in (("pi", pi, sref[0]), ("logp", np.log(pi), sref[1]), ("v", v, sref[2]),
                           ("gpi", gpi, gref[0]), ("glogp", np.log(gpi), gref[1]),
                           ("gv", gv, gref[2])):
        worst = assert_close(f"{tag}/{name}", got, ref, TOL)
        print(f"{tag} {name}: max err {worst:.3g} ({TOL / max(worst, 1e-300):.1f}x)")


# ------------------------------------------------------------------ 5. the wrappers
def _three_chunk_budget(wrappers, offs, F):
    """test_gpu_star_batch._three_chunk_budget for the exact route's cost."""
    cost = wrappers._star_exact_chunk_cost(F)
    cr, cs, fixed = cost
    lin = cr * np.asarray(offs, np.int64) + cs * np.arange(len(offs))
    for b in range(1, len(offs)):
        budget = fixed + int(lin[b])
        if len(wrappers.star_chunks(offs, F, budget, cost)) == 3:
            return budget
    raise AssertionError("no budget splits these stars into 3 chunks")


def test_wrappers_take_the_exact_star_route(monkeypatch):
    """Under the key predict_with_gnn(board, neighbor_states) equals row b of a 70-star
    predict_star_batch and of predict_both_stars, whose standard rows equal predict; three chunks
    give the same bits; AZ_B1_MODE / AZ_NO_ZEROCOPY select nothing.  With the key off 8 small
    stars still take the one-call evaluator."""
    from azhip import wrappers
    game, w = _wrapper("c4", (4, 4), seed=8, batch_invariant=True, use_gnn=True,
                       gnn_neighbors=True)
    assert w.batch_invariant_stars is True
    stars = _game_stars("c4", (4, 4), game, 70, 91)
    rows, offs = _packed(stars)
    pi, v, gpi, gv = w.predict_both_stars(rows, offs)
    assert w.star_route == "exact"
    bpi, bv = w.predict_star_batch(stars)
    assert w.star_route == "exact"
    assert np.array_equal(bpi, gpi) and np.array_equal(bv, gv)
    for b in (0, 1, 2, 33, 69):
        w.star_route = None
        p1, v1 = w.predict_with_gnn(stars[b][0], stars[b][1:])
        if len(stars[b]) > 1:
            assert w.star_route == "exact"
        assert np.array_equal(p1, gpi[b]) and v1 == gv[b], b
        p0, v0 = w.predict(stars[b][0])
        assert np.array_equal(p0, pi[b]) and v0 == v[b], b
    monkeypatch.setenv("AZ_B1_MODE", "graph")
    monkeypatch.setenv("AZ_NO_ZEROCOPY", "1")
    p8, v8 = w.predict_star_batch(stars[:8])
    assert w.star_route == "exact"
    assert np.array_equal(p8, gpi[:8]) and np.array_equal(v8, gv[:8])
    monkeypatch.delenv("AZ_B1_MODE")
    monkeypatch.delenv("AZ_NO_ZEROCOPY")
    budget = _three_chunk_budget(wrappers, offs, w.feature_dim)
    monkeypatch.setattr(wrappers, "STAR_EXACT_CHUNK_BYTES", budget)
    batch = w._star_exact_batches[None]
    n0 = len(batch.calls)
    chunked = w.predict_both_stars(rows, offs)
    assert len(batch.calls) - n0 == 3 and w.star_route == "exact"
    assert sum(c[0] for c in batch.calls[n0:]) == 70
    for a, b in zip(chunked, (pi, v, gpi, gv)):
        assert np.array_equal(a, b)
    # the key off: the routes of today
    game, w0 = _wrapper("c4", (4, 4), seed=8, use_gnn=True, gnn_neighbors=True)
    assert w0.batch_invariant_stars is False
    small = [s[:9] for s in stars[:8]]
    w0.predict_star_batch(small)
    assert w0.star_route == "onecall"


# ------------------------------------------------------------------ 6. self-play
def test_selfplay_with_stars_does_not_depend_on_parallel_games():
    """Connect4 4x4, GNN wrapper with the key, gnn_neighbors and gnn_neighbors_lockstep, two GNN
    layers, 12 simulations, expand_by 1, 20 episodes with seed = episode: play_episodes_engine at
    (G, lanes) = (1, 1), (20, 1) and (24, 2) gives identical standard and GNN examples per
    episode, and episodes 0, 7 and 19 are the sequential Coach.executeEpisode's (Python search,
    predict plus predict_with_gnn(board, children)).  B and V of every star call are recorded."""
    import nn_fallback
    from Coach import Coach
    from selfplay import play_episodes_engine
    from azhip.build import build_host
    build_host(verbose=False)
    game, w = _wrapper("c4", (4, 4), seed=12, batch_invariant=True, use_gnn=True,
                       gnn_neighbors=True, gnn_neighbors_lockstep=True)
    args = SimpleNamespace(numEps=20, numMCTSSims=12, cpuct=1.0, tempThreshold=6, use_gnn=True,
                           expand_by=1, gnn_neighbors=True, gnn_neighbors_lockstep=True,
                           gnn_layers=2, dropout=0.3, batch_invariant=True, parallel_games=20)
    calls = []
    orig = w._exact_stars

    def spy(rows, offs, stream=None):
        calls.append((len(offs) - 1, int(np.asarray(offs)[-1])))
        return orig(rows, offs, stream)

    w._exact_stars = spy
    eps = list(range(20))
    seeds = {e: e for e in eps}
    nn_fallback.reset()
    runs, shapes = [], []
    for G, lanes in ((1, 1), (20, 1), (24, 2)):
        n0 = len(calls)
        runs.append(play_episodes_engine(game, w, args, eps, seeds, parallel_games=G, threads=2,
                                         lanes=lanes))
        shapes.append(calls[n0:])
        assert shapes[-1] and sorted(runs[-1]) == eps
        print(f"G={G} lanes={lanes}: {len(shapes[-1])} star calls, max B "
              f"{max(b for b, _ in shapes[-1])}, max V {max(v for _, v in shapes[-1])}")
    assert max(b for b, _ in shapes[0]) == 1
    assert max(b for b, _ in shapes[1]) > 8 and max(v for _, v in shapes[1]) > 64
    assert max(b for b, _ in shapes[2]) > 8 and max(v for _, v in shapes[2]) > 32
    assert w.star_route == "exact" and nn_fallback.total() == 0

    def same(x, y):
        return len(x) == len(y) and all(
            len(a) == len(b) and all(np.array_equal(np.asarray(p), np.asarray(q))
                                     for p, q in zip(a, b)) for a, b in zip(x, y))

    for e in eps:
        for other in runs[1:]:
            assert same(runs[0][e][0], other[e][0]), ("std", e)
            assert same(runs[0][e][1], other[e][1]), ("gnn", e)
        assert len(runs[0][e][0]) > 0 and len(runs[0][e][1]) > 0
    for e in (0, 7, 19):
        np.random.seed(seeds[e])
        std, gnn = Coach(game, w, args).executeEpisode()
        assert same(std, runs[2][e][0]), ("sequential std", e)
        assert same(gnn, runs[2][e][1]), ("sequential gnn", e)
    assert nn_fallback.total() == 0
