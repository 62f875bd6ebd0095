"""Whole-network and GNN-layer gradients on the MI355X at the shapes training never ran: odd
and single-row batches (K = B H W odd or 1 in every weight-gradient GEMM), TicTacToe 4x4 / 5x5
(heads_bwd_kernel<32>, conv3 with more than one output pixel), a sharded batch normalised by
the global B, and irregular graphs in az_gnn_layer_bwd (in-degrees up to and beyond the 256
register-held edges of gnn_agg_bwd_edges_kernel, D < V, several destinations on the dots /
finish pair, H < 64, no edges at all).

The criterion is tests/test_gpu_train.py's (its docstring derives it): per element
|ours - ref64| <= 10 max|torch32 - ref64| + C_ROUND u32 S with C_ROUND = 4, float64 / float32
autograd of oracle/torch_ref.py, S from abs_contributions.  Every tensor's needed C_ROUND lands
in gradcheck.MARGINS and so in grad_round_margins.json (test_gpu_train.py::test_report_margins)."""
import numpy as np
import pytest

from conftest import golden, split_weights

torch = pytest.importorskip("torch")

import gradcheck as gc  # noqa: E402
from gradcheck import abs_contributions, check_grad, cu, make_net  # noqa: E402
from gradcheck import check_cnn_grads as _check_cnn, ref_grads as _ref  # noqa: E402
from gradcheck import random_boards, targets  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from azhip import _lib
    return _lib.lib()


def _ttt_weights(n):
    from azhip.weights import gnn_spec, synthetic_state_dict, tictactoe_net_spec
    F = 128 * (n - 2) * (n - 2)
    if n == 3:
        z = golden("ttt3.npz")
        return split_weights(z, "w/"), split_weights(z, "g/")
    if n == 4:
        z = golden("ttt4.npz")
        return (synthetic_state_dict(tictactoe_net_spec(4), int(z["seed_cnn"])),
                synthetic_state_dict(gnn_spec(F, 2), int(z["seed_gnn"])))
    return (synthetic_state_dict(tictactoe_net_spec(5), 51),
            synthetic_state_dict(gnn_spec(F, 2), 52))


@pytest.mark.parametrize("n,B", [(5, 1), (5, 5), (5, 33), (4, 3), (4, 33)])
def test_ttt_cnn_grads_larger_boards(lib, n, B):
    """A = 26 / 17 (heads_bwd_kernel<32>), conv3's col2im with 3x3 / 2x2 output pixels, and
    K = 9 B / 4 B, 25 B / 16 B in the conv weight gradients."""
    from azhip import train as T
    from oracle import torch_ref as R
    W, _ = _ttt_weights(n)
    net, _ = make_net("ttt", W, n=n)
    boards = random_boards(n, B, 100 * n + B)
    tpi, tv = targets(B, n * n + 1, n + B)
    T.cnn_grads(net, cu(boards), cu(tpi), cu(tv))

    def fn(P):
        return R.losses(*R.ttt_heads(R.ttt_features(boards, P), P), tpi, tv)
    _check_cnn(f"ttt{n}_cnn/B{B}", net, W, fn)


@pytest.mark.parametrize("B,B_norm", [(1, None), (33, None), (21, 64)])
def test_c4_cnn_grads_odd_batches(lib, B, B_norm):
    """Dropout 0.3 with an explicit mask; (21, 64) is a rank's shard of a 64-row batch
    (dist.row_shard on 3 ranks), normalised by the global batch."""
    from azhip import train as T, ops
    from oracle import torch_ref as R
    z = golden("c4_net.npz")
    W = split_weights(z, "w/")
    net, _ = make_net("c4", W, dropout=0.3)
    boards = z["boards"][5:5 + B]
    tpi, tv = targets(B, 8, 10 + B)
    mask = ops.dropout_mask(B * 3136, 0.3, 4321 + B, "cuda")
    T.cnn_grads(net, cu(boards), cu(tpi), cu(tv), drop_mask=mask, B_norm=B_norm)
    m = mask.cpu().numpy().reshape(B, 3136)
    scale = B / float(B_norm or B)

    def fn(P):
        return R.losses(*R.c4_heads(R.c4_features(boards, P, m, 0.3), P), tpi, tv) * scale
    _check_cnn(f"c4_cnn/B{B}" + (f"of{B_norm}" if B_norm else ""), net, W, fn)


@pytest.mark.parametrize("n,B", [(3, 2), (3, 33), (5, 5)])
def test_ttt_gnn_grads_small_and_odd_stars(lib, n, B):
    """The star over the batch at B = 2 (one edge), an odd B, and F = 1152 (5x5)."""
    from azhip import train as T
    from oracle import torch_ref as R
    W, G = _ttt_weights(n)
    net, gnn = make_net("ttt", W, G, n=n)
    boards = random_boards(n, B, 200 * n + B)
    tpi, tv = targets(B, n * n + 1, 3 * n + B)
    T.gnn_grads(net, gnn, cu(boards), cu(tpi), cu(tv))
    got = {k: v.cpu().numpy() for k, v in gnn.params.grads.items()}
    Pn = R.params(W, torch.float64, requires_grad=False)

    def run(PG):
        Wn = {k: v.to(next(iter(PG.values())).dtype) for k, v in Pn.items()}
        y = R.policy_value_gnn(R.ttt_features(boards, Wn), PG)
        return R.losses(*R.ttt_heads(y, Wn), tpi, tv)
    g64, g32 = _ref(run, G, torch.float64), _ref(run, G, torch.float32)
    S = abs_contributions(run, R.params(G, torch.float64))
    assert set(g64) == set(G)
    for k in g64:
        check_grad(f"ttt{n}_gnn/B{B}/{k}", got[k], g64[k], g32[k], S[k])


# ------------------------------------------------------------------------------ GNN layer bwd
class LayerCase:
    """One GNNLayer (layers.0 of synthetic weights) on a CSR graph: inputs, float64 / float32
    autograd of oracle.torch_ref.gnn_layer_csr, and S -- computed once per case."""

    def __init__(self, rowptr, col, F, H, seed):
        from azhip.weights import gnn_spec, synthetic_state_dict
        from oracle import torch_ref as R
        self.rowptr, self.col, self.F, self.H = rowptr, col, F, H
        self.V = V = len(rowptr) - 1
        self.spec = gnn_spec(F, 2, H)
        self.G = synthetic_state_dict(self.spec, seed)
        rng = np.random.default_rng(seed + 1)
        self.x0 = rng.uniform(-1, 1, (V, F)).astype(np.float32)
        self.dout = rng.standard_normal((V, F)).astype(np.float32)

        def loss(P, xt, dtype):
            out = R.gnn_layer_csr(xt, rowptr, col, P, 0)
            return out, (out * torch.from_numpy(self.dout).to(dtype)).sum()

        def ref(dtype):
            P = R.params(self.G, dtype)
            xt = torch.from_numpy(self.x0).to(dtype).requires_grad_(True)
            out, l = loss(P, xt, dtype)
            l.backward()
            gr = {k[len("layers.0."):]: v.grad.numpy() for k, v in P.items()
                  if k.startswith("layers.0.")}
            return gr, xt.grad.numpy(), out.detach().numpy()
        self.r64, self.dx64, self.y64 = ref(torch.float64)
        self.r32, self.dx32, _ = ref(torch.float32)
        self.S = abs_contributions(
            lambda P: loss(P, torch.from_numpy(self.x0).double(), torch.float64)[1],
            R.params(self.G, torch.float64))

    def run(self, claimed_max_deg=None):
        """Forward (save) + backward on the GPU from NaN-filled gradient buffers.  Returns
        (y, dx, grads) as device tensors."""
        from azhip import ops
        from azhip.params import FlatParams
        g = ops.DeviceGraph(self.rowptr, self.col)
        if claimed_max_deg is not None:
            g.c.max_deg = claimed_max_deg
        prm = FlatParams(self.spec, "cuda", self.G)
        Wl = {k[len("layers.0."):]: v for k, v in prm.views.items() if k.startswith("layers.0.")}
        x = cu(self.x0)
        y, ws = ops.gnn_layer(g, x, Wl, H=self.H)
        prm.grad_flat.fill_(float("nan"))
        Gl = {k[len("layers.0."):]: v for k, v in prm.grads.items() if k.startswith("layers.0.")}
        dx = torch.full_like(x, float("nan"))
        ops.gnn_layer_bwd(g, x, Wl, ws, cu(self.dout), Gl, dx=dx, H=self.H)
        torch.cuda.synchronize()
        self._keep = (g, prm)
        return y, dx, {k: v.clone() for k, v in Gl.items()}

    def check(self, name, y, dx, grads):
        np.testing.assert_allclose(y.cpu().numpy(), self.y64, atol=1e-5)
        check_grad(name + "/dx", dx.cpu().numpy(), self.dx64, self.dx32)
        assert set(grads) == set(self.r64) and len(grads) == 10
        for k in self.r64:
            check_grad(f"{name}/{k}", grads[k].cpu().numpy(), self.r64[k], self.r32[k],
                       self.S["layers.0." + k])


def test_layer_bwd_mixed_degrees_edges_path(lib):
    """V = 320, F = 64: in-degrees 0 (ten nodes: D < V, rows != NULL, dst_index -1), 1..6, and
    65 / 130 / 200 / 256 -- every register slot of gnn_agg_bwd_edges_kernel and its last offset;
    a self-loop, a repeated source, a node that is never a source.  E < 16 D."""
    rowptr, col = gc.mixed_degree_graph(320)
    D = int((np.diff(rowptr) > 0).sum())
    assert D < 320 and int(rowptr[-1]) < 16 * D
    case = LayerCase(rowptr, col, 64, 128, 320)
    case.check("mixed320", *case.run())


def test_layer_bwd_several_destinations_dots_path(lib):
    """V = 64, F = 320 (a partial second pass of the f += 256 loops): destinations 0, 17, 63
    with in-degrees 40, 63, 50, so E >= 16 D: gnn_agg_bwd_dots_kernel with a non-null dst_index
    and gnn_agg_bwd_finish_kernel with three rows."""
    rowptr, col = gc.few_destinations_graph(64)
    assert int(rowptr[-1]) >= 16 * 3
    case = LayerCase(rowptr, col, 320, 128, 64)
    case.check("dots64", *case.run())


def test_layer_bwd_narrow_hidden(lib):
    """H = 32 < 64 lanes (gnn_attn_bwd_nodes_kernel's q loop leaves half the wave idle) on the
    mixed-degree graph cut to V = 40."""
    rowptr, col = gc.mixed_degree_graph(40)
    case = LayerCase(rowptr, col, 64, 32, 40)
    case.check("mixed40_h32", *case.run())


def test_layer_bwd_without_edges(lib):
    """E = 0: every row passes through, dx is dout bit for bit and every parameter gradient is
    written as exactly zero."""
    case = LayerCase(np.zeros(9, np.int64), np.zeros(0, np.int64), 64, 128, 8)
    y, dx, grads = case.run()
    assert torch.equal(y, cu(case.x0))
    assert torch.equal(dx, cu(case.dout))
    assert len(grads) == 10
    for k, g in grads.items():
        assert torch.equal(g, torch.zeros_like(g)), k


def test_layer_bwd_does_not_trust_max_deg(lib):
    """az_graph.max_deg only picks kernels (include/az_hip.h): one destination with 300 in-edges
    -- beyond the 256 that gnn_agg_bwd_edges_kernel holds in registers -- among in-degrees 1..4,
    with the honest max_deg, with 4 and with 0 (an unset field).  All three match float64, and the
    two understated runs equal the honest one bit for bit (forward output, dx, every gradient);
    so does the backward pass alone on the honest forward's saved activations."""
    from azhip import ops
    rowptr, col = gc.one_wide_destination_graph()
    assert int(np.diff(rowptr).max()) == 300 and int(rowptr[-1]) < 16 * 400
    case = LayerCase(rowptr, col, 64, 128, 400)
    honest = case.run()
    case.check("wide300/honest", *honest)
    for claimed in (4, 0):
        got = case.run(claimed)
        case.check(f"wide300/claimed{claimed}", *got)
        assert torch.equal(got[0], honest[0]) and torch.equal(got[1], honest[1])
        for k in honest[2]:
            assert torch.equal(got[2][k], honest[2][k]), (claimed, k)
    # the backward alone, from the honest forward's workspace, under each claim
    g = ops.DeviceGraph(rowptr, col)
    from azhip.params import FlatParams
    prm = FlatParams(case.spec, "cuda", case.G)
    Wl = {k[len("layers.0."):]: v for k, v in prm.views.items() if k.startswith("layers.0.")}
    x, dout = cu(case.x0), cu(case.dout)
    _, ws = ops.gnn_layer(g, x, Wl)
    outs = []
    for claimed in (300, 4, 0):
        g.c.max_deg = claimed
        prm.grad_flat.fill_(float("nan"))
        Gl = {k[len("layers.0."):]: v for k, v in prm.grads.items() if k.startswith("layers.0.")}
        dx = ops.gnn_layer_bwd(g, x, Wl, ws, dout, Gl, dx=torch.full_like(x, float("nan")))
        outs.append([dx.clone()] + [Gl[k].clone() for k in sorted(Gl)])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert torch.equal(outs[0][0], honest[1])
