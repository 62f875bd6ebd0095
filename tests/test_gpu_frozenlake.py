"""FrozenLakeNet on the GPU against the reference's recorded outputs
(tests/golden/make_frozenlake_goldens.py): the one-launch evaluator az_fl_eval_fwd, its row
independence, the whole-board table, az_fl_grads / az_clip_grad_norm, train(), and the search
and Coach loop on top.  Bars: 1e-5 on pi and v, 1e-5 relative to a tensor's largest gradient
(the per-tensor bar the fixture records where the reference's own fp32 error is larger), 2e-5
on weights after train()."""
import os

import numpy as np
import pytest

from conftest import assert_close, golden, report

pytestmark = pytest.mark.gpu

SHAPES = {"4": (4, 64, 2), "8": (8, 128, 3)}


class Args(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _wrapper(n, E, L, weights=None, **kw):
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    from frozenlake.FrozenLakeNet import FrozenLakeNet
    args = Args(lr=1e-3, dropout=0.3, epochs=2, batch_size=8, embedding_dim=E, gnn_layers=L)
    args.update(kw)
    import torch
    with torch.random.fork_rng(devices=[]):      # a fixed initialisation, the global RNG untouched
        torch.manual_seed(1234)
        w = FrozenLakeNet(FrozenLakeGame(map_size=n), args)
    if weights is not None:
        w.nnet.load_state_dict(weights)
    return w


def _weights(z, prefix):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


def _states(n):
    out = []
    for cell in range(n * n):
        b = np.zeros((n, n))
        b[cell // n, cell % n] = 1
        out.append(b)
    return out + [np.zeros((n, n))]


@pytest.fixture(scope="module")
def nets():
    """One wrapper per forward fixture, with the fixture's weights (never trained here)."""
    out = {}
    for tag, (n, E, L) in SHAPES.items():
        z = golden(f"fl_net_{tag}.npz")
        out[tag] = (_wrapper(n, E, L, _weights(z, "w.")), z)
    return out


def _pack(w, node_lists):
    import torch
    B, S = len(node_lists), w.S
    nodes = np.zeros((B, 5, S), np.float32)
    counts = np.zeros((B,), np.int32)
    for i, nl in enumerate(node_lists):
        nodes[i, :len(nl)] = np.asarray(nl, np.float32).reshape(len(nl), S)
        counts[i] = len(nl)
    return torch.from_numpy(nodes).to(w.device), torch.from_numpy(counts).to(w.device)


def _eval(w, nodes, counts):
    import torch
    from azhip.frozenlake import fl_eval_fwd
    B = counts.shape[0]
    pi = torch.empty((B, 4), device=w.device)
    v = torch.empty((B,), device=w.device)
    fl_eval_fwd(w.nnet, nodes, counts, pi, v, B)
    torch.cuda.synchronize()
    return pi, v


# ------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("tag", ["4", "8"])
def test_forward_all_states_in_one_call(nets, tag):
    w, z = nets[tag]
    n = SHAPES[tag][0]
    nodes, counts = _pack(w, [w._node_list(b) for b in _states(n)])
    assert set(counts.cpu().tolist()) == {1, 3, 4, 5}
    pi, v = _eval(w, nodes, counts)
    for ref in ("64", "32"):
        assert_close(f"fl_fwd_{tag}_pi_vs_{ref}", pi.cpu().numpy(), z[f"pi{ref}"], 1e-5)
        assert_close(f"fl_fwd_{tag}_v_vs_{ref}", v.cpu().numpy(), z[f"v{ref}"], 1e-5)


@pytest.mark.parametrize("tag", ["4", "8"])
def test_forward_free_form_boards_with_explicit_nodes(nets, tag):
    import torch
    w, z = nets[tag]
    n = SHAPES[tag][0]
    counts = z["free_counts"]
    assert sorted(set(counts.tolist())) == [1, 2, 3, 4, 5]
    pi, v = _eval(w, torch.from_numpy(z["free_nodes"]).to(w.device),
                  torch.from_numpy(counts).to(w.device))
    for ref in ("64", "32"):
        assert_close(f"fl_free_{tag}_pi_vs_{ref}", pi.cpu().numpy(), z[f"free_pi{ref}"], 1e-5)
        assert_close(f"fl_free_{tag}_v_vs_{ref}", v.cpu().numpy(), z[f"free_v{ref}"], 1e-5)
    # the same boards through predict(board, neighbor_states): the per-call route, same bits
    for i, k in enumerate(counts):
        nl = [z["free_nodes"][i, j].reshape(n, n) for j in range(k)]
        p1, v1 = w.predict(nl[0], neighbor_states=nl)
        assert p1.dtype == np.float32 and p1.shape == (4,) and v1.shape == (1,)
        assert np.array_equal(p1, pi[i].cpu().numpy()) and v1[0] == v[i].item()


# ------------------------------------------------------------------------------------ rows
def test_rows_do_not_depend_on_the_batch(nets):
    import torch
    w, _ = nets["8"]
    nodes, counts = _pack(w, [w._node_list(b) for b in _states(8)])
    alone = [_eval(w, nodes[i:i + 1], counts[i:i + 1]) for i in range(65)]
    for B in (1, 2, 5, 17, 65):
        pi, v = _eval(w, nodes[:B].contiguous(), counts[:B].contiguous())
        pi2, v2 = _eval(w, nodes[:B].contiguous(), counts[:B].contiguous())
        assert torch.equal(pi, pi2) and torch.equal(v, v2)
        for i in range(B):
            assert torch.equal(pi[i], alone[i][0][0]) and torch.equal(v[i], alone[i][1][0]), (B, i)
    # rows at and beyond counts[b] are never read
    pi, v = _eval(w, nodes, counts)
    poisoned = nodes.clone()
    for i in range(65):
        poisoned[i, int(counts[i]):] = float("nan")
    pi2, v2 = _eval(w, poisoned, counts)
    assert torch.equal(pi, pi2) and torch.equal(v, v2) and not torch.isnan(pi2).any()


# ------------------------------------------------------------------------------------ table
@pytest.mark.parametrize("tag", ["4", "8"])
def test_table_and_per_call_routes_agree(nets, tag, monkeypatch):
    w, z = nets[tag]
    states = _states(SHAPES[tag][0])
    monkeypatch.setenv("AZ_FL_TABLE", "1")
    w._table = None
    calls = w.eval_calls
    table = [w.predict(b) for b in states]
    assert w.eval_calls == calls + 1            # one evaluator call filled the table
    again = [w.predict(b) for b in states]
    assert w.eval_calls == calls + 1            # cached states cost no evaluator call
    monkeypatch.setenv("AZ_FL_TABLE", "0")
    direct = [w.predict(b) for b in states]
    assert w.eval_calls == calls + 1 + len(states)
    for (p0, v0), (p1, v1), (p2, v2) in zip(table, again, direct):
        assert p0.shape == (4,) and v0.shape == (1,) and p0.dtype == v0.dtype == np.float32
        assert np.array_equal(p0, p1) and np.array_equal(v0, v1)
        assert np.array_equal(p0, p2) and np.array_equal(v0, v2)
    assert_close(f"fl_table_{tag}_pi", np.array([p for p, _ in table]), z["pi64"], 1e-5)
    monkeypatch.setenv("AZ_FL_TABLE", "1")
    bp, bv = w.predict_batch(np.array(states))
    assert bp.shape == (len(states), 4) and bv.shape == (len(states),)
    assert np.array_equal(bp, np.array([p for p, _ in table]))
    assert np.array_equal(bv, np.array([v[0] for _, v in table]))
    mixed = np.array(states[:3]) * np.array([1.0, 0.5, 1.0])[:, None, None]   # row 1: not one-hot
    mp, mv, _, _ = w.predict_batch_async(mixed).result()
    assert np.array_equal(mp[0], table[0][0]) and np.array_equal(mp[2], table[2][0])
    p_half, v_half = w.predict(mixed[1])
    assert np.array_equal(mp[1], p_half) and mv[1] == v_half[0]


def _table_matches_fresh_evaluation(w, monkeypatch):
    states = _states(w.board_size[0])
    monkeypatch.setenv("AZ_FL_TABLE", "1")
    table = [w.predict(b) for b in states]
    monkeypatch.setenv("AZ_FL_TABLE", "0")
    direct = [w.predict(b) for b in states]
    for (p0, v0), (p1, v1) in zip(table, direct):
        assert np.array_equal(p0, p1) and np.array_equal(v0, v1)
    return np.array([p for p, _ in table])


def test_table_follows_weight_changes(monkeypatch, tmp_path):
    z = golden("fl_train_4.npz")
    w = _wrapper(4, 64, 2, _weights(z, "start."))
    before = _table_matches_fresh_evaluation(w, monkeypatch)
    w.save_checkpoint(str(tmp_path), "start.pth.tar")
    np.random.seed(int(z["np_seed"]))
    w.train([(b, p, v) for b, p, v in zip(z["boards"], z["pis"], z["vs"])])
    trained = _table_matches_fresh_evaluation(w, monkeypatch)
    assert not np.array_equal(before, trained)
    snap = w.snapshot()
    w.load_checkpoint(str(tmp_path), "start.pth.tar")
    assert np.array_equal(_table_matches_fresh_evaluation(w, monkeypatch), before)
    w.restore(snap)
    assert np.array_equal(_table_matches_fresh_evaluation(w, monkeypatch), trained)
    w.load_checkpoint(str(tmp_path), "missing.pth.tar")          # prints and returns
    import torch
    ck = torch.load(os.path.join(str(tmp_path), "start.pth.tar"), weights_only=True)
    assert list(ck) == ["state_dict"] and list(ck["state_dict"]) == [
        "feature_extractor.0.weight", "feature_extractor.0.bias", "feature_extractor.2.weight",
        "feature_extractor.2.bias", "gnn_layers.0.W.weight", "gnn_layers.0.W.bias",
        "gnn_layers.1.W.weight", "gnn_layers.1.W.bias", "policy_head.weight", "policy_head.bias",
        "value_head.weight", "value_head.bias"]


@pytest.mark.nn_failures_expected
def test_nan_and_exception_fallbacks_are_counted():
    """FrozenLakeNet.py:220-230: a NaN policy becomes uniform, an exception uniform and 0.0;
    both are counted by nn_fallback instead of passing unseen."""
    import nn_fallback
    import torch
    w = _wrapper(4, 64, 2)
    board = w.game.getInitBoard()
    with torch.no_grad():
        w.nnet.params["policy_head.bias"][1] = float("nan")
    pi, v = w.predict(board)
    assert np.array_equal(pi, np.full(4, 0.25, np.float32)) and not np.isnan(v).any()
    assert nn_fallback.counts() == {"FrozenLakeNet.predict": 1}
    pi, v = w.predict(board, neighbor_states=[board] * 6)        # six nodes: rejected
    assert np.array_equal(pi, np.ones(4) / 4) and v == 0.0
    assert nn_fallback.counts() == {"FrozenLakeNet.predict": 2}


def test_fresh_wrapper_has_xavier_weights_and_zero_biases():
    w = _wrapper(4, 64, 2)
    sd = w.nnet.params.cpu_state_dict()
    for k, t in sd.items():
        if k.endswith("bias"):
            assert float(t.abs().max()) == 0.0, k
        else:
            fan_out, fan_in = t.shape
            want = (2.0 / (fan_in + fan_out)) ** 0.5
            assert 0.7 * want < float(t.std()) < 1.3 * want, k


# ------------------------------------------------------------------------------------ gradients
def _grad_setup(tag):
    import torch
    n, E, L = SHAPES[tag]
    z, g = golden(f"fl_net_{tag}.npz"), golden(f"fl_grad_{tag}.npz")
    weights = _weights(z, "w.")
    weights["policy_head.bias"] = g["policy_bias"]
    w = _wrapper(n, E, L, weights)
    dev = w.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return w, g, t(g["nodes"]), t(g["counts"]), t(g["tpi"]), t(g["tv"])


@pytest.mark.parametrize("tag", ["4", "8"])
def test_gradients_clip_and_determinism(tag):
    import torch
    from azhip.frozenlake import clip_grad_norm, fl_grads
    w, g, nodes, counts, tpi, tv = _grad_setup(tag)
    clip = golden(f"fl_grad_{tag}_clip.npz")
    assert {1, 3, 4, 5} <= set(g["counts"].tolist())
    loss, dl = fl_grads(w.nnet, nodes, counts, tpi, tv, want_dlogits=True)
    torch.cuda.synchronize()
    grads = {k: v.clone() for k, v in w.nnet.params.grads.items()}
    assert_close(f"fl_grad_{tag}_loss", loss.cpu().numpy(), [float(g["loss64"])], 1e-5,
                 rel_floor=1.0)
    for k, got in grads.items():
        ref = g[f"pre64.{k}"].astype(np.float64)
        top = float(np.abs(ref).max())
        assert top > 0, k
        assert_close(f"fl_grad_{tag}_pre.{k}", got.cpu().numpy() / top, ref / top,
                     float(g[f"bar.{k}"]))
    # the clamp of the loss: where pi < 1e-8 the target's weight reaches the logit only through
    # the other actions' softmax terms (log-softmax would give (pi - 0.5) / B there)
    a = int(g["clamp_action"])
    B = len(g["counts"])
    for r in g["clamp_rows"]:
        assert g["tpi"][r, a] == 0.5
        assert abs(dl[int(r), a].item()) < 1e-8 < 0.4 / B
    # a second run gives the same bits
    loss2, dl2 = fl_grads(w.nnet, nodes, counts, tpi, tv, want_dlogits=True)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2)
    for k, got in grads.items():
        assert torch.equal(got, w.nnet.params.grads[k]), k
    # rows at and beyond counts[b] are never read
    poisoned = nodes.clone()
    for i in range(B):
        poisoned[i, int(counts[i]):] = float("nan")
    loss3, _ = fl_grads(w.nnet, poisoned, counts, tpi, tv)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss3)
    for k, got in grads.items():
        assert torch.equal(got, w.nnet.params.grads[k]), k
    # clip_grad_norm_(max_norm=1.0) over the per-tensor buffers
    views = list(w.nnet.params.grads.values())
    norm = clip_grad_norm(views, 1.0)
    torch.cuda.synchronize()
    assert float(g["norm64"]) > 1.0
    assert_close(f"fl_grad_{tag}_norm", norm.cpu().numpy() / float(g["norm64"]), [1.0], 1e-5)
    for k, got in w.nnet.params.grads.items():
        ref = clip[f"post64.{k}"].astype(np.float64)
        top = float(np.abs(ref).max())
        assert_close(f"fl_grad_{tag}_post.{k}", got.cpu().numpy() / top, ref / top,
                     float(g[f"bar.{k}"]))
    # ... and the flat buffer in one piece gives the same norm as the list of its tensors
    fl_grads(w.nnet, nodes, counts, tpi, tv)
    norm_flat = clip_grad_norm([w.nnet.params.grad_flat], 1.0)
    torch.cuda.synchronize()
    assert_close(f"fl_grad_{tag}_norm_flat", norm_flat.cpu().numpy() / float(g["norm64"]), [1.0],
                 1e-5)


def test_clip_grad_norm_below_and_above_the_bound():
    import torch
    from azhip.frozenlake import clip_grad_norm
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(3)
    small = [(torch.randn(n, generator=gen) * 1e-3).to(dev) for n in (1, 7, 1025, 4096)]
    kept = [t.clone() for t in small]
    want = float(torch.sqrt(sum((t.double() ** 2).sum() for t in kept)))
    norm = clip_grad_norm(small, 1.0)
    assert want < 1.0 and abs(norm.item() - want) <= 1e-6 * want
    for a, b in zip(small, kept):
        assert torch.equal(a, b)                         # nothing may change below the bound
    big = [(torch.randn(n, generator=gen) * 3).to(dev) for n in (5, 300, 2049)]
    kept = [t.clone() for t in big]
    want = float(torch.sqrt(sum((t.double() ** 2).sum() for t in kept)))
    norm = clip_grad_norm(big, 1.0)
    norm2 = float(torch.sqrt(sum((t.double() ** 2).sum() for t in big)))
    assert want > 1.0 and abs(norm.item() - want) <= 1e-6 * want
    assert abs(norm2 - 1.0) < 1e-5
    coef = np.float32(1.0) / (np.float32(norm.item()) + np.float32(1e-6))
    for a, b in zip(big, kept):
        assert torch.equal(a, b * float(coef))
    # the same buffers again: the same bits
    again = [t.clone() for t in kept]
    assert torch.equal(clip_grad_norm(again, 1.0), norm)
    for a, b in zip(again, big):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------ training
def _train_fixture(name):
    z = golden(name + ".npz")
    n, E, L = int(z["map_size"]), int(z["E"]), int(z["L"])
    kw = dict(lr=float(z["lr"]), epochs=int(z["epochs"]), batch_size=int(z["batch_size"]))
    examples = [(b, p, v) for b, p, v in zip(z["boards"], z["pis"], z["vs"])]
    return z, (n, E, L), kw, examples


@pytest.mark.parametrize("name", ["fl_train_4", "fl_train_8x8_e64"])
def test_train_matches_reference_weights(name):
    z, shape, kw, examples = _train_fixture(name)
    w = _wrapper(*shape, _weights(z, "start."), **kw)
    np.random.seed(int(z["np_seed"]))
    w.train(list(examples))
    first = w.nnet.params.cpu_state_dict()
    worst32 = 0.0
    for k, got in first.items():
        worst32 = max(worst32, float(np.abs(got.numpy() - z[f"after32.{k}"]).max()))
        assert float(np.abs(got.numpy() - z[f"start.{k}"]).max()) > 0, k     # it did move
    report(f"{name}_vs_fp32", max_err=worst32, tol=2e-5)
    for k, got in first.items():
        assert_close(f"{name}.{k}", got.numpy(), z[f"after64.{k}"], 2e-5)
    # a second train() from the same start and seed: Adam starts afresh, so the same weights
    w.nnet.load_state_dict(_weights(z, "start."))
    np.random.seed(int(z["np_seed"]))
    w.train(list(examples))
    for k, got in w.nnet.params.cpu_state_dict().items():
        assert np.array_equal(got.numpy(), first[k].numpy()), k


@pytest.mark.parametrize("name", ["fl_train_4", "fl_train_8x8_e64"])
def test_train_predict_train(name, monkeypatch):
    """train(), predict of a cached state (the table fill carries S+1 leaves, more than a
    batch of 8), then train() again: the gradient workspace follows the descriptor's capacity."""
    monkeypatch.setenv("AZ_FL_TABLE", "1")
    z, shape, kw, examples = _train_fixture(name)
    assert kw["batch_size"] < shape[0] ** 2 + 1
    w = _wrapper(*shape, _weights(z, "start."), **kw)
    np.random.seed(int(z["np_seed"]))
    w.train(list(examples))
    once = w.nnet.params.flat.clone()
    fills = w.table_builds
    pi, v = w.predict(w.game.getInitBoard())
    assert w.table_builds == fills + 1 and abs(float(pi.sum()) - 1) < 1e-5
    np.random.seed(int(z["np_seed"]))
    w.train(list(examples))
    assert not (w.nnet.params.flat == once).all()
    pi2, _ = w.predict(w.game.getInitBoard())
    assert w.table_builds == fills + 2 and not np.array_equal(pi, pi2)
    # the predict in between changes nothing about the second train()
    ref = _wrapper(*shape, _weights(z, "start."), **kw)
    for _ in range(2):
        np.random.seed(int(z["np_seed"]))
        ref.train(list(examples))
    assert (ref.nnet.params.flat == w.nnet.params.flat).all()


def test_train_small_and_nan_inputs_leave_the_weights_alone():
    z, shape, kw, examples = _train_fixture("fl_train_4")
    w = _wrapper(*shape, _weights(z, "start."), **kw)
    start = w.nnet.params.flat.clone()
    w.train(examples[:3])                                    # fewer than 4: untouched
    assert (w.nnet.params.flat == start).all()
    bad = [(b.copy(), p, v) for b, p, v in examples[:8]]
    bad[5][0][0, 0] = np.nan
    np.random.seed(9)
    w.train(bad)                                             # its only batch holds a NaN: skipped
    assert (w.nnet.params.flat == start).all()
    after = np.random.random()
    np.random.seed(9)
    for _ in range(kw["epochs"]):                            # the shuffles were still drawn
        np.random.shuffle(list(range(8)))
    assert after == np.random.random()
    w.train([(b, p, None) for b, p, _ in examples[:8]])      # no example with a value
    assert (w.nnet.params.flat == start).all()


# ------------------------------------------------------------------------------------ search
def test_search_counts_same_with_table_on_and_off(nets, monkeypatch):
    from MCTS import MCTS
    w, _ = nets["4"]
    args = Args(numMCTSSims=25, cpuct=2.0)
    board = w.game.getInitBoard()
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("AZ_FL_TABLE", flag)
        m = MCTS(w.game, w, args)
        probs = m.getActionProb(board, temp=1)
        out.append((probs, [m.Nsa.get(("0,0", a), 0) for a in range(4)]))
    assert out[0] == out[1] and sum(out[0][1]) >= 1


def test_lockstep_selfplay_batches_its_leaves():
    """selfplay.play_episodes (the Python lock-step driver) serves the live games' leaves with
    one predict_batch call per round and yields the examples of the one-game-at-a-time search."""
    import selfplay
    from Coach import episode_g
    from MCTS import MCTS
    w = _wrapper(4, 64, 2)
    args = Args(numMCTSSims=10, cpuct=2.0, tempThreshold=10 ** 6)
    seeds = selfplay.episode_seeds(77, range(4))

    class Guard(selfplay.BatchEvaluator):
        def __call__(self, requests):
            assert self.calls < 20000, "self-play did not end"     # fail, never hang
            return super().__call__(requests)

    stats = {}
    got = selfplay.play_episodes(w.game, w, args, range(4), seeds, parallel_games=4,
                                 evaluator=Guard(w), stats=stats)
    assert stats["rows"] > stats["calls"] >= 1
    for e in range(4):
        rng = np.random.RandomState(seeds[e])
        m = MCTS(w.game, w, args, rng=rng)
        std, gnn = m.drive(episode_g(w.game, args, m, rng))
        assert gnn == [] and got[e][1] == [] and len(std) == len(got[e][0]) >= 1
        for (b0, p0, r0), (b1, p1, r1) in zip(std, got[e][0]):
            assert np.array_equal(b0, b1) and list(p0) == list(p1) and r0 == r1


def test_one_coach_iteration(tmp_path):
    import Coach as C
    args = Args(numIters=1, numEps=2, tempThreshold=10 ** 6, updateThreshold=0.55,
                maxlenOfQueue=1000, numItersForTrainExamplesHistory=2, numMCTSSims=10,
                cpuct=2.0, arenaCompare=2, checkpoint=str(tmp_path), lr=1e-3, dropout=0.3,
                epochs=1, batch_size=8, embedding_dim=64, gnn_layers=2)
    w = _wrapper(4, 64, 2, **args)
    assert C._native_ok(w.game) is False                     # the Python MCTS plays this game
    orig = np.random.choice
    moves = [0]

    def choice(*a, **k):
        moves[0] += 1
        assert moves[0] <= 5000, "self-play did not end"     # fail, never hang
        return orig(*a, **k)

    start = w.nnet.params.flat.clone()
    np.random.seed(21)
    np.random.choice = choice
    try:
        coach = C.Coach(w.game, w, args)
        coach.learn()
    finally:
        np.random.choice = orig
    assert len(coach.trainExamplesHistory) == 1 and len(coach.trainExamplesHistory[0][0]) >= 4
    assert not (w.nnet.params.flat == start).all()            # it trained, and kept the result
    for f in ("temp.pth.tar", "best.pth.tar", "checkpoint_1.pth.tar"):
        assert os.path.exists(os.path.join(str(tmp_path), f)), f
