"""Connect4 training on rectangular boards on the MI355X: whole-network gradients of T.cnn_grads
and T.gnn_grads on 7x6 (the standard game, F = 2688, A = 8), 5x4 (F = 1280, A = 6) and 4x6 (F =
1536, A = 5: no fused trunk, the two conv launches), and the hand-over from a training step to the
one-call evaluator az_c4r_eval_fwd.

What runs here for the first time: az_nchw_drelu_to_pm / az_im2col3x3 / az_col2im3x3_drelu with
H != W (HW = 42 / 20 / 24), az_heads_bwd at K = 2688 (a partial last 256-column block), and the
F x F backward GEMMs at those widths.

The gradient criterion is gradcheck.check_grad's, unchanged (tests/test_gpu_train.py derives it),
against float64 / float32 autograd; gradcheck.guard_reference keeps the references from being
vacuous.  oracle/torch_ref.c4_features is written for square boards, so its six lines are restated
here for [B, 1, cols, rows]; the oracle's c4_heads, losses and policy_value_gnn are used as they
are.  The evaluator check is bitwise: a cached evaluator against an uncached one on the same
weights."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gradcheck import abs_contributions, check_cnn_grads, check_grad, cu  # noqa: E402
from gradcheck import guard_reference, ref_grads, targets  # noqa: E402

gpu = pytest.mark.gpu
P_DROP = 0.3


@pytest.fixture(scope="module")
def lib():
    from azhip import _lib
    return _lib.lib()


def _weights(shape, gnn=True):
    """Synthetic weights of a cols x rows Connect4Net and its two-layer GNN."""
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    cols, rows = shape
    W = synthetic_state_dict(connect4_net_spec(shape, cols + 1), 400 + 10 * cols + rows)
    G = synthetic_state_dict(gnn_spec(64 * cols * rows, 2), 500 + 10 * cols + rows) if gnn \
        else None
    return W, G


def _make_net(shape, W, G=None, dropout=0.0):
    from azhip import nets
    game = SimpleNamespace(getBoardSize=lambda: tuple(shape),
                           getActionSize=lambda: shape[0] + 1)
    net = nets.Connect4Net(game, {"dropout": dropout}, init=W)
    gnn = nets.PolicyValueGNN(64 * shape[0] * shape[1], 2, init=G) if G is not None else None
    return net, gnn


def _boards(shape, B, seed):
    return np.random.default_rng(seed).integers(-1, 2, size=(B,) + tuple(shape)).astype(np.int8)


def c4_features_rect(boards, W, drop_mask=None, p=0.0):
    """connect4/Connect4Net.py:42-52 for a [B, cols, rows] board: the image is [B, 1, cols, rows]
    (oracle/torch_ref.c4_features with the second extent its own)."""
    import torch.nn.functional as F
    B, cols, rows = boards.shape
    s = torch.as_tensor(boards).to(W["conv1.weight"].dtype).view(B, 1, cols, rows)
    s = F.relu(F.conv2d(s, W["conv1.weight"], W["conv1.bias"], padding=1))
    s = F.relu(F.conv2d(s, W["conv2.weight"], W["conv2.bias"], padding=1))
    s = s.reshape(B, -1)
    if drop_mask is not None:
        s = s * torch.as_tensor(drop_mask).to(s.dtype).view_as(s) / (1.0 - p)
    return s


# ------------------------------------------------------------------------------ CNN gradients
@gpu
@pytest.mark.parametrize("shape,B", [((7, 6), 33), ((5, 4), 1), ((4, 6), 9)])
def test_rect_cnn_grads(lib, shape, B):
    """All eight tensors of T.cnn_grads with dropout 0.3 under an explicit mask, read back for
    the reference: 7x6 at an odd batch (K = 33 * 42 in the conv weight gradients), 5x4 at one row
    and 4x6 (rows > columns, the eager trunk) at 9."""
    from azhip import train as T, ops
    from oracle import torch_ref as R
    cols, rows = shape
    F, A = 64 * cols * rows, cols + 1
    W, _ = _weights(shape, gnn=False)
    net, _ = _make_net(shape, W, dropout=P_DROP)
    assert net.route == ("eager" if shape == (4, 6) else "c4r")
    boards = _boards(shape, B, 1000 * cols + 100 * rows + B)
    tpi, tv = targets(B, A, 10 * cols + rows + B)
    mask = ops.dropout_mask(B * F, P_DROP, 4000 + 100 * cols + 10 * rows + B, "cuda")
    T.cnn_grads(net, cu(boards), cu(tpi), cu(tv), drop_mask=mask)
    m = mask.cpu().numpy().reshape(B, F)

    def fn(P):
        logp, v = R.c4_heads(c4_features_rect(boards, P, m, P_DROP), P)
        return R.losses(logp, v, tpi, tv)

    check_cnn_grads(f"c4r{cols}x{rows}_cnn/B{B}", net, W, fn, guard=guard_reference)


# ------------------------------------------------------------------------------ GNN gradients
@gpu
@pytest.mark.parametrize("shape,B", [((7, 6), 9), ((5, 4), 33)])
def test_rect_gnn_grads_on_the_star(lib, shape, B):
    """All 24 tensors of T.gnn_grads on the star over the batch."""
    from azhip import train as T, ops
    from oracle import torch_ref as R
    cols, rows = shape
    F, A = 64 * cols * rows, cols + 1
    W, G = _weights(shape)
    net, gnn = _make_net(shape, W, G, dropout=P_DROP)
    boards = _boards(shape, B, 2000 * cols + 100 * rows + B)
    tpi, tv = targets(B, A, 30 * cols + rows + B)
    mask = ops.dropout_mask(B * F, P_DROP, 5000 + 100 * cols + 10 * rows + B, "cuda")
    T.gnn_grads(net, gnn, cu(boards), cu(tpi), cu(tv), drop_mask=mask)
    got = {k: v.cpu().numpy() for k, v in gnn.params.grads.items()}
    m = mask.cpu().numpy().reshape(B, F)
    Pn = R.params(W, torch.float64, requires_grad=False)

    def run(PG):
        Wn = {k: v.to(next(iter(PG.values())).dtype) for k, v in Pn.items()}
        y = R.policy_value_gnn(c4_features_rect(boards, Wn, m, P_DROP), PG)
        return R.losses(*R.c4_heads(y, Wn), tpi, tv)

    g64, g32 = ref_grads(run, G, torch.float64), ref_grads(run, G, torch.float32)
    S = abs_contributions(run, R.params(G, torch.float64))
    assert set(g64) == set(G) and len(g64) == 24
    name = f"c4r{cols}x{rows}_gnn/B{B}"
    guard_reference(name, g64, S)
    for k in g64:
        check_grad(f"{name}/{k}", got[k], g64[k], g32[k], S[k])


# ------------------------------------------------------------ a training step, then the evaluator
def _evaluate(ops, ev, boards, B):
    """One az_c4r_eval_fwd call, kind "both", on the first B boards -> [pi, v, gpi, gv] rows."""
    dev = boards.device
    outs = [torch.full((ev.max_B, ev.A) if i % 2 == 0 else (ev.max_B,), float("nan"), device=dev)
            for i in range(4)]
    ops.c4r_eval(ev, boards, B, *outs)
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(o[:B]).any()) for o in outs)
    return [o[:B].clone() for o in outs]


@gpu
@pytest.mark.parametrize("shape", [(7, 6), (5, 4)])
def test_c4r_evaluator_follows_training_steps(lib, shape):
    """A C4rEval on the two networks' parameter buffers, warmed at 65 boards (the composed heads)
    and at 8 (the GEMV path), then T.cnn_step and T.gnn_step on a 33-board batch.  After each step
    the same evaluator equals, bit for bit, a fresh one on new networks built from the stepped
    values; a CNN step moves all four outputs, a GNN step moves the GNN heads and leaves the
    standard heads bitwise alone."""
    from azhip import train as T, ops
    cols, rows = shape
    A, MAX_B = cols + 1, 70
    W, G = _weights(shape)
    net, gnn = _make_net(shape, W, G, dropout=P_DROP)
    dev = net.params.device
    ev = ops.C4rEval(net.params, gnn.params, shape, A, MAX_B, dev)
    eb = cu(_boards(shape, 65, 77))
    net.params.reset_adam()
    gnn.params.reset_adam()
    tb = cu(_boards(shape, 33, 78))
    tpi, tv = (cu(t) for t in targets(33, A, 79))

    def both():
        return {B: _evaluate(ops, ev, eb, B) for B in (65, 8)}

    def fresh():
        net2, gnn2 = _make_net(shape, net.params.cpu_state_dict(), gnn.params.cpu_state_dict(),
                               dropout=P_DROP)
        ev2 = ops.C4rEval(net2.params, gnn2.params, shape, A, MAX_B, dev)
        return {B: _evaluate(ops, ev2, eb, B) for B in (65, 8)}

    before = both()
    steps = ((lambda: T.cnn_step(net, tb, tpi, tv, 1e-2, seed=80), (1, 0), (True, True)),
             (lambda: T.gnn_step(net, gnn, tb, tpi, tv, 1e-2, seed=81), (1, 1), (False, True)))
    for step, counts, (std_moves, gnn_moves) in steps:
        step()
        assert (net.params.step, gnn.params.step) == counts
        after, want = both(), fresh()
        for B in (65, 8):
            for k, name in enumerate(("pi", "v", "gpi", "gv")):
                assert torch.equal(after[B][k], want[B][k]), (counts, B, name, "stale cache")
                moved = not torch.equal(after[B][k], before[B][k])
                assert moved == (std_moves if k < 2 else gnn_moves), (counts, B, name, moved)
        before = after


def test_checkpoint_keys_are_the_same_and_shapes_differ():
    """No GPU: a 7x7 and a 7x6 checkpoint have the same keys in the same order and differ in the
    fc widths, which is what FlatParams.load_state_dict refuses by name and shape."""
    from azhip.weights import connect4_net_spec
    s76, s77, s67 = (dict(connect4_net_spec(s)) for s in ((7, 6), 7, (6, 7)))
    assert list(s76) == list(s77) == list(s67)
    assert s76["fc_policy.weight"] == (8, 2688) and s77["fc_policy.weight"] == (8, 3136)
    assert s67["fc_policy.weight"] == (7, 2688)       # the transposed board: another A


@gpu
def test_loading_a_checkpoint_of_another_shape_fails_with_the_shapes(lib, tmp_path):
    from connect4.Connect4Game import Connect4Game
    from connect4.Connect4Net import Connect4NNetWrapper
    args = SimpleNamespace(dropout=0.3)
    w77 = Connect4NNetWrapper(Connect4Game(7), args)
    w77.save_checkpoint(str(tmp_path), "sq.pth.tar")
    w76 = Connect4NNetWrapper(Connect4Game(7, rows=6), args)
    with pytest.raises(RuntimeError) as e:
        w76.load_checkpoint(str(tmp_path), "sq.pth.tar")
    assert "3136" in str(e.value) and "2688" in str(e.value)
    w76.save_checkpoint(str(tmp_path), "rect.pth.tar")
    w76b = Connect4NNetWrapper(Connect4Game(7, rows=6), args)
    w76b.load_checkpoint(str(tmp_path), "rect.pth.tar")
    assert torch.equal(w76b.nnet.params.flat, w76.nnet.params.flat)
