"""T.gnn_grads (the GNN step on the star over the batch) at the depths --gnn_layers accepts besides
2: TicTacToe 3x3 (F = 128), gnn_layers 0, 1 and 3 at B = 5, and gnn_layers 3 at B = 1, where
there is no graph and every layer gradient is written as exactly zero.

Reference: oracle.torch_ref.policy_value_gnn(..., num_layers) under float64 / float32 autograd.
The criterion is tests/gradcheck.py's, unchanged (tests/test_gpu_train.py derives it): per element
|ours - ref64| <= 10 max|torch32 - ref64| + C_ROUND u32 S.  guard_reference sees every float64
reference first, and test_references_are_not_vacuous runs it on the CPU on the very inputs the GPU
test uses.  Every tensor's needed C_ROUND lands in gradcheck.MARGINS."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gradcheck import abs_contributions, check_grad, cu, guard_reference  # noqa: E402
from gradcheck import random_boards, ref_grads, targets  # noqa: E402

gpu = pytest.mark.gpu
F, A = 128, 10
CASES = [(0, 5), (1, 5), (3, 5), (3, 1)]          # (gnn_layers, B)
_REF = {}


def case(L, B):
    from azhip.weights import gnn_spec, synthetic_state_dict, tictactoe_net_spec
    W = synthetic_state_dict(tictactoe_net_spec(3, A), 700)
    G = synthetic_state_dict(gnn_spec(F, L), 710 + L)
    return W, G, random_boards(3, B, 720 + 10 * L + B), *targets(B, A, 730 + L + B)


def gnn_loss(W, boards, tpi, tv, L):
    """The GNN step's loss as a function of the GNN's parameters: the frozen board network's
    features, PolicyValueGNN with L layers on the star over the batch, the board network's heads
    on every row."""
    from oracle import torch_ref as R
    Pn = R.params(W, torch.float64, requires_grad=False)

    def run(PG):
        Wn = {k: v.to(next(iter(PG.values())).dtype) for k, v in Pn.items()}
        y = R.policy_value_gnn(R.ttt_features(boards, Wn), PG, L)
        return R.losses(*R.ttt_heads(y, Wn), tpi, tv)
    return run


def reference(L, B):
    """(float64 gradients, float32 gradients, S) of the tensors the case can reach: all 10 L + 4
    with a graph, the four output_transform tensors at B = 1."""
    if (L, B) not in _REF:
        from oracle import torch_ref as R
        W, G, boards, tpi, tv = case(L, B)
        run = gnn_loss(W, boards, tpi, tv, L)
        g64, g32 = ref_grads(run, G, torch.float64), ref_grads(run, G, torch.float32)
        S = abs_contributions(run, R.params(G, torch.float64))
        if B == 1:
            g64, g32 = ({k: v for k, v in g.items() if k.startswith("output_transform.")}
                        for g in (g64, g32))
        assert len(g64) == (10 * L if B > 1 else 0) + 4 and set(g64) <= set(G)
        _REF[(L, B)] = (g64, g32, S)
    return _REF[(L, B)]


@pytest.mark.parametrize("L,B", CASES)
def test_references_are_not_vacuous(L, B):
    """CPU: the float64 reference of every case passes guard_reference."""
    g64, _, S = reference(L, B)
    guard_reference(f"ttt3_gnn/L{L}/B{B}", g64, S)


@gpu
@pytest.mark.parametrize("L,B", CASES)
def test_gnn_grads_at_other_depths(L, B):
    """Every tensor of T.gnn_grads, written into gradient buffers full of NaN, and the loss."""
    from types import SimpleNamespace
    from azhip import nets, train as T
    from oracle import torch_ref as R
    W, G, boards, tpi, tv = case(L, B)
    g64, g32, S = reference(L, B)
    name = f"ttt3_gnn/L{L}/B{B}"
    guard_reference(name, g64, S)
    game = SimpleNamespace(getBoardSize=lambda: (3, 3), getActionSize=lambda: A)
    net = nets.TicTacToeNet(game, {}, init=W)
    gnn = nets.PolicyValueGNN(F, L, init=G)
    assert net.feature_dim == F and len(gnn.layers) == L
    gnn.params.grad_flat.fill_(float("nan"))
    loss = T.gnn_grads(net, gnn, cu(boards), cu(tpi), cu(tv))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in gnn.params.grads.items()}
    assert set(got) == set(G) and len(got) == 10 * L + 4
    for k in got:
        if k in g64:
            check_grad(f"{name}/{k}", got[k], g64[k], g32[k], S[k])
        else:                                   # B = 1: the layers are the identity
            assert k.startswith("layers.") and B == 1
            assert np.array_equal(got[k], np.zeros_like(got[k])), k
    run = gnn_loss(W, boards, tpi, tv, L)
    with torch.no_grad():
        l64 = float(run(R.params(G, torch.float64, requires_grad=False)))
        l32 = float(run(R.params(G, torch.float32, requires_grad=False)))
    total = float(loss.sum().item())
    print(f"{name}: loss {total} ref {l64}")
    check_grad(f"{name}/loss", total, l64, l32)
