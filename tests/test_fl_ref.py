"""CPU: tests/fl_ref.py, the float64 restatement of FrozenLakeNet that tests/
test_gpu_frozenlake_shapes.py measures the kernels against, held to the reference's recorded
outputs first: the forward fixtures to 1e-12, the loss, the clip norm and every pre- and
post-clip gradient tensor to 2e-7 of the tensor's largest entry (those tensors are stored rounded
to float32, a 6e-8 relative change)."""
import numpy as np
import pytest

from conftest import golden, split_weights

torch = pytest.importorskip("torch")

import fl_ref  # noqa: E402

SHAPES = {"4": (4, 64, 2), "8": (8, 128, 3)}


def node_list(game, board):
    nodes = [board]
    valids = game.getValidMoves(board, 1)
    for a in range(game.getActionSize()):
        if valids[a]:
            nxt, _ = game.getNextState(board, 1, a)
            nodes.append(game.getCanonicalForm(nxt, 1))
    return nodes


def pack(node_lists, S):
    nodes = np.full((len(node_lists), 5, S), np.nan, np.float32)
    counts = np.zeros((len(node_lists),), np.int32)
    for i, nl in enumerate(node_lists):
        nodes[i, :len(nl)] = np.asarray(nl, np.float32).reshape(len(nl), S)
        counts[i] = len(nl)
    return nodes, counts


@pytest.mark.parametrize("tag", ["4", "8"])
def test_forward_matches_the_recorded_float64_outputs(tag):
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    n, E, L = SHAPES[tag]
    z = golden(f"fl_net_{tag}.npz")
    W = split_weights(z, "w.")
    assert fl_ref.num_layers(W) == L
    assert [(k, tuple(W[k].shape)) for k in W] == fl_ref.spec(n * n, E, L)
    P = fl_ref.params(W)
    with torch.no_grad():
        pi, v, _ = fl_ref.forward(P, z["free_nodes"], z["free_counts"])
    assert np.abs(pi.numpy() - z["free_pi64"]).max() <= 1e-12
    assert np.abs(v.numpy() - z["free_v64"]).max() <= 1e-12
    game = FrozenLakeGame(map_size=n)
    states = []
    for cell in range(n * n):
        b = np.zeros((n, n))
        b[cell // n, cell % n] = 1
        states.append(b)
    states.append(np.zeros((n, n)))
    nodes, counts = pack([node_list(game, b) for b in states], n * n)
    with torch.no_grad():
        pi, v, _ = fl_ref.forward(P, nodes, counts)      # rows beyond counts[b] are NaN
    assert np.abs(pi.numpy() - z["pi64"]).max() <= 1e-12
    assert np.abs(v.numpy() - z["v64"]).max() <= 1e-12
    # float32 runs too, and stays within float32's reach of float64
    with torch.no_grad():
        pi32, v32, _ = fl_ref.forward(fl_ref.params(W, torch.float32), nodes, counts)
    assert pi32.dtype == torch.float32 and v32.dtype == torch.float32
    assert np.abs(pi32.numpy() - z["pi64"]).max() <= 1e-5


@pytest.mark.parametrize("tag", ["4", "8"])
def test_loss_gradients_and_clip_match_the_recorded_float64_batch(tag):
    z, g = golden(f"fl_net_{tag}.npz"), golden(f"fl_grad_{tag}.npz")
    post = golden(f"fl_grad_{tag}_clip.npz")
    W = split_weights(z, "w.")
    W["policy_head.bias"] = g["policy_bias"]
    r = fl_ref.grads(W, g["nodes"], g["counts"], g["tpi"], g["tv"])
    assert abs(r["loss"] - float(g["loss64"])) <= 2e-7 * abs(float(g["loss64"]))
    assert set(r["grads"]) == set(W)
    for k, got in r["grads"].items():
        ref = g[f"pre64.{k}"].astype(np.float64)
        assert np.abs(got - ref).max() <= 2e-7 * np.abs(ref).max(), k
    norm, clipped = fl_ref.clip(r["grads"], 1.0)
    assert abs(norm - float(g["norm64"])) <= 2e-7 * float(g["norm64"])
    for k, got in clipped.items():
        ref = post[f"post64.{k}"].astype(np.float64)
        assert np.abs(got - ref).max() <= 2e-7 * np.abs(ref).max(), k
    # the clamp rows: dloss / dlogit of the clamped action, by autograd through the clamp
    a = int(g["clamp_action"])
    for row in g["clamp_rows"]:
        assert r["pi"][row, a] < 1e-8 and abs(r["dlogits"][row, a]) < 1e-8
    # the float32 restatement runs, and no bar made from it falls below the project's 1e-5
    r32 = fl_ref.grads(W, g["nodes"], g["counts"], g["tpi"], g["tv"], torch.float32)
    assert all(t.dtype == np.float32 for t in r32["grads"].values())
    bars, _ = fl_ref.bars(r["grads"], r32["grads"])
    for k, bar in bars.items():
        assert bar >= 1e-5, (k, bar)
