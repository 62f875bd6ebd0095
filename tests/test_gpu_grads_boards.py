"""Connect4 training on 4x4, 5x5, 6x6 and 8x8 boards on the MI355X: whole-network gradients of
T.cnn_grads and T.gnn_grads at F = 64 n^2 = 1024 / 1600 / 2304 / 4096 and A = n + 1 = 5 / 6 / 7 / 9
(every other Connect4 gradient test runs at 7x7), and the hand-over from a training step to the
one-call evaluator of those boards.

What runs here for the first time: az_heads_bwd at K = F (1600 ends in a partial 256-column
block, A = 9 takes heads_bwd_kernel<16> in the fused form), az_nchw_drelu_to_pm / az_im2col3x3 /
az_col2im3x3_drelu at HW = 16 / 25 / 36 / 64, az_gnn_layer_bwd / az_mlp2_bwd / node_update_bwd at
those F -- and with them F x F weight-gradient GEMMs that split K (F = 1024 and 1600 have fewer
than 1024 64 x 64 tiles; 7x7's 2401 tiles never split) and reduce their slabs into a column
half of gate.0.weight / update_net.0.weight.

The gradient criterion is tests/test_gpu_train.py's, unchanged (its docstring derives it): per
element |ours - ref64| <= 10 max|torch32 - ref64| + C_ROUND u32 S, C_ROUND = 4, float64 / float32
autograd of oracle/torch_ref.py, S from abs_contributions.  Every tensor's needed C_ROUND lands
in gradcheck.MARGINS and so in grad_round_margins.json (test_gpu_train.py::test_report_margins,
which runs after this file).  gradcheck.guard_reference keeps the references from being vacuous,
and one CPU-only test shows that the criterion rejects a weight gradient that lost one batch row.
The evaluator check is bitwise: a cached evaluator against an uncached one on the same weights."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gradcheck as gc  # noqa: E402
from gradcheck import abs_contributions, check_cnn_grads, check_grad, cu  # noqa: E402
from gradcheck import guard_reference, make_net, random_boards, ref_grads, targets  # noqa: E402

gpu = pytest.mark.gpu
P_DROP = 0.3


@pytest.fixture(scope="module")
def lib():
    from azhip import _lib
    return _lib.lib()


def _weights(n, gnn=True):
    """Synthetic weights of an n x n Connect4Net (seed 40 + n) and its two-layer GNN (50 + n)."""
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    W = synthetic_state_dict(connect4_net_spec(n, n + 1), 40 + n)
    return W, (synthetic_state_dict(gnn_spec(64 * n * n, 2), 50 + n) if gnn else None)


# ------------------------------------------------------------------------------ CNN gradients
def cnn_case(n, B):
    """Boards and targets of one cnn_grads case, and the seed of its dropout mask."""
    return random_boards(n, B, 100 * n + B), *targets(B, n + 1, n + B), 4000 + 100 * n + B


def cnn_loss(boards, tpi, tv, m, scale=1.0, rows=None):
    """The CNN step's loss (Connect4GNN.py:148-152) on oracle.torch_ref with the keep mask m;
    `rows`: only the first `rows` batch rows' terms, still normalised by the whole batch."""
    from oracle import torch_ref as R
    r = len(boards) if rows is None else rows

    def fn(P):
        logp, v = R.c4_heads(R.c4_features(boards, P, m, P_DROP), P)
        return R.losses(logp[:r], v[:r], tpi[:r], tv[:r]) * (scale * r / len(boards))
    return fn


@gpu
@pytest.mark.parametrize("n,B,B_norm", [(4, 1, None), (4, 33, None), (5, 33, None), (6, 9, None),
                                        (8, 3, None), (8, 33, None), (5, 21, 64)])
def test_c4n_cnn_grads(lib, n, B, B_norm):
    """All eight tensors of T.cnn_grads with dropout 0.3 under an explicit mask, read back for
    the reference: one row, odd batches (K = B n^2 in the conv weight gradients: 16 .. 2112),
    and (5, 21, 64), a rank's shard of a 64-row batch normalised by the global batch."""
    from azhip import train as T, ops
    F = 64 * n * n
    W, _ = _weights(n, gnn=False)
    net, _ = make_net("c4", W, dropout=P_DROP, n=n)
    boards, tpi, tv, seed = cnn_case(n, B)
    mask = ops.dropout_mask(B * F, P_DROP, seed, "cuda")
    T.cnn_grads(net, cu(boards), cu(tpi), cu(tv), drop_mask=mask, B_norm=B_norm)
    m = mask.cpu().numpy().reshape(B, F)
    fn = cnn_loss(boards, tpi, tv, m, B / float(B_norm or B))
    check_cnn_grads(f"c4n{n}_cnn/B{B}" + (f"of{B_norm}" if B_norm else ""), net, W, fn,
                    guard=guard_reference)


# ------------------------------------------------------------------------------ GNN gradients
def gnn_case(n, B):
    return random_boards(n, B, 200 * n + B), *targets(B, n + 1, 3 * n + B), 5000 + 100 * n + B


def gnn_loss(W, boards, tpi, tv, m):
    """The GNN step's loss (Connect4GNN.py:187-193) as a function of the GNN's parameters: the
    frozen CNN's dropped features, PolicyValueGNN on the star over the batch, the CNN's heads."""
    from oracle import torch_ref as R
    Pn = R.params(W, torch.float64, requires_grad=False)

    def run(PG):
        Wn = {k: v.to(next(iter(PG.values())).dtype) for k, v in Pn.items()}
        y = R.policy_value_gnn(R.c4_features(boards, Wn, m, P_DROP), PG)
        return R.losses(*R.c4_heads(y, Wn), tpi, tv)
    return run


@gpu
@pytest.mark.parametrize("n,B", [(4, 2), (4, 5), (4, 260), (5, 33), (6, 9), (8, 3)])
def test_c4n_gnn_grads_on_the_star(lib, n, B):
    """All 24 tensors of T.gnn_grads on the star over the batch.  (4, 2) is the one-edge star:
    the attention MLP's gradient is identically zero there (the single normalised weight is 1),
    which the guard asserts of the reference instead of a non-zero maximum.  (4, 260): the
    F x F weight gradients of az_mlp2_bwd have K = 260 rows, 256 tiles and two K splits with a
    tail in the second, and row 0 has 259 in-edges (beyond the 256 register-held ones)."""
    from azhip import train as T, ops
    from oracle import torch_ref as R
    F = 64 * n * n
    W, G = _weights(n)
    net, gnn = make_net("c4", W, G, dropout=P_DROP, n=n)
    boards, tpi, tv, seed = gnn_case(n, B)
    mask = ops.dropout_mask(B * F, P_DROP, seed, "cuda")
    T.gnn_grads(net, gnn, cu(boards), cu(tpi), cu(tv), drop_mask=mask)
    got = {k: v.cpu().numpy() for k, v in gnn.params.grads.items()}
    run = gnn_loss(W, boards, tpi, tv, mask.cpu().numpy().reshape(B, F))
    g64, g32 = ref_grads(run, G, torch.float64), ref_grads(run, G, torch.float32)
    S = abs_contributions(run, R.params(G, torch.float64))
    assert set(g64) == set(G) and len(g64) == 24
    name = f"c4n{n}_gnn/B{B}"
    guard_reference(name, g64, S, all_zero=("attention.",) if B == 2 else ())
    for k in g64:
        check_grad(f"{name}/{k}", got[k], g64[k], g32[k], S[k])


# ------------------------------------------------------------ a training step, then the evaluator
def _evaluate(ops, ev, boards, B):
    """One az_c4n_eval_fwd call, kind "both", on the first B boards -> [pi, v, gpi, gv] rows."""
    dev = boards.device
    outs = [torch.full((ev.max_B, ev.A) if i % 2 == 0 else (ev.max_B,), float("nan"), device=dev)
            for i in range(4)]
    ops.c4n_eval(ev, boards, B, *outs)
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(o[:B]).any()) for o in outs)
    return [o[:B].clone() for o in outs]


@gpu
def test_c4n_evaluator_follows_training_steps(lib):
    """5x5 (F = 1600, A = 6): a C4nEval on the two networks' parameter buffers, warmed at 65
    boards (the first row count on the composed heads Wc = [fc_policy; fc_value] W2) and at 8
    (the GEMV path), then T.cnn_step and T.gnn_step on a 33-board batch.  After each step the
    same evaluator equals, bit for bit, a fresh one on new networks built from the stepped
    values; a CNN step moves all four outputs (the GNN heads through Wc's dependence on
    fc_policy.weight / fc_value.weight and through the trunk), a GNN step moves the GNN heads and
    leaves the standard heads bitwise alone; params.step advances on the stepped network only."""
    from azhip import train as T, ops
    n, A, F, MAX_B = 5, 6, 1600, 70
    W, G = _weights(n)
    net, gnn = make_net("c4", W, G, dropout=P_DROP, n=n)
    dev = net.params.device
    ev = ops.C4nEval(net.params, gnn.params, n, A, MAX_B, dev)
    eb = cu(random_boards(n, 65, 77))
    net.params.reset_adam()
    gnn.params.reset_adam()
    tb = cu(random_boards(n, 33, 78))
    tpi, tv = (cu(t) for t in targets(33, A, 79))

    def both():
        return {B: _evaluate(ops, ev, eb, B) for B in (65, 8)}

    def fresh():
        net2, gnn2 = make_net("c4", net.params.cpu_state_dict(), gnn.params.cpu_state_dict(),
                              dropout=P_DROP, n=n)
        ev2 = ops.C4nEval(net2.params, gnn2.params, n, A, MAX_B, dev)
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


# ------------------------------------------------------------------ the criterion can fail (CPU)
def test_criterion_rejects_a_lost_batch_row():
    """No GPU: at (n = 5, B = 33) the float32 autograd gradient passes check_grad, and the same
    gradient with the last batch row's loss term removed -- what a weight-gradient GEMM that
    loses its K tail computes -- is rejected for conv2.weight and for fc_policy.weight.  The
    references pass the vacuity guard."""
    from oracle import torch_ref as R
    n, B = 5, 33
    W, _ = _weights(n, gnn=False)
    boards, tpi, tv, seed = cnn_case(n, B)
    m = (np.random.default_rng(seed).random((B, 64 * n * n)) >= P_DROP).astype(np.uint8)
    fn = cnn_loss(boards, tpi, tv, m)
    g64, g32 = ref_grads(fn, W, torch.float64), ref_grads(fn, W, torch.float32)
    S = abs_contributions(fn, R.params(W, torch.float64))
    guard_reference("criterion", g64, S)
    lost = ref_grads(cnn_loss(boards, tpi, tv, m, rows=B - 1), W, torch.float32)
    kept = dict(gc.MARGINS)
    try:
        for k in ("conv2.weight", "fc_policy.weight"):
            check_grad("criterion/" + k, g32[k], g64[k], g32[k], S[k])
            with pytest.raises(AssertionError):
                check_grad("criterion/" + k, lost[k], g64[k], g32[k], S[k])
            assert gc.MARGINS["criterion/" + k] > 100 * gc.C_ROUND      # not a marginal miss
    finally:                        # keep this test's figures out of grad_round_margins.json
        gc.MARGINS.clear()
        gc.MARGINS.update(kept)
