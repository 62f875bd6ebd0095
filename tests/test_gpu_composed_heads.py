"""The heads composed with output_transform.2 (csrc/az_weights.hip composed_heads): for y == NULL,
A <= 8 and B > 64 the evaluators never run the second GEMM -- the heads are linear in
y = hidden W2^T + b2 (Connect4GNN.py:106-114 on gnn_utils.py:115's last Linear), so
logits = hidden Wc^T + bc with Wc = [fc_policy.weight; fc_value.weight] W2 and
bc = [fc_policy.weight; fc_value.weight] b2 + [fc_policy.bias; fc_value.bias], composed in fp64
and rounded once, cached per weight generation when every input is registered storage."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from azhip import ops as o
    return o


@contextlib.contextmanager
def registered(tensors):
    """The tensors' storage as registered parameter storage (az_weights_register), as FlatParams
    does for a network's flat buffer."""
    from azhip import _lib
    L = _lib.load()
    done = []
    try:
        for t in tensors:
            _lib.check(L.az_weights_register(t.data_ptr(), t.numel() * 4), "az_weights_register")
            done.append(t)
        yield
    finally:
        for t in done:
            _lib.check(L.az_weights_unregister(t.data_ptr()), "az_weights_unregister")


def _changed():
    from azhip import _lib
    _lib.check(_lib.load().az_weights_changed(), "az_weights_changed")


def _problem(F, A, B, seed):
    """x and (w, b, wp, bp, wv, bv) with test_transform_heads_without_y's distribution."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, F), generator=g) * 2 - 1
    w = (torch.rand((F, F), generator=g) * 2 - 1) / F ** 0.5
    b = (torch.rand((F,), generator=g) - 0.5) * 0.1
    wp = (torch.rand((A, F), generator=g) * 2 - 1) / F ** 0.5
    wv = (torch.rand((1, F), generator=g) * 2 - 1) / F ** 0.5
    bp, bv = torch.rand((A,), generator=g) - 0.5, torch.rand((1,), generator=g) - 0.5
    return x, (w, b, wp, bp, wv, bv)


def _fp64_heads(x, w, b, wp, bp, wv, bv):
    yd = x.double() @ w.double().T + b.double()
    lg = yd @ wp.double().T + bp.double()
    lp = (lg - torch.logsumexp(lg, 1, keepdim=True)).numpy()
    return lp, torch.tanh(yd @ wv.double().T + bv.double()).flatten().numpy()


@pytest.mark.parametrize("F,A,B", [(3136, 8, 65), (3136, 8, 129), (288, 7, 65)])
def test_composed_heads_match_fp64_at_the_paths_edges(ops, F, A, B):
    """linear_heads(want_y=False) on given x at the first row count of the composed path (65),
    at 129, and at a width with a partial 256-column chunk and A < 8, against fp64 heads of
    x W2^T + b2: 1e-6 on log pi and v (about 10x what fp64-composed rows and an fp32 dot give;
    a wrong row of Wc or a dropped Wh b2 term shows at 1e-3 and above).  Registered weights
    (cached Wc) and unregistered ones (composed per call) give the same bits, and B = 64 -- the
    last row count on the GEMM path -- stays within the 1e-5 contract of the same fp64.
    Measured on MI355X: log pi 3.9e-7 / 4.8e-7 / 4.0e-7 for the three cases (margins 2.6x, 2.1x,
    2.5x: under 3x, and the same 3.9-4.4e-7 as the B = 64 GEMM path, i.e. the fp32 log-softmax's
    own rounding at |log pi| of 2-4, not the composition), pi 5-7e-8, v 4-7e-8 (14-24x)."""
    x, wts = _problem(F, A, B, 1000 * F + B)
    lp64, v64 = _fp64_heads(x, *wts)
    xd = x.cuda()
    cu = [t.cuda() for t in wts]
    ul, up, uv, uy = ops.linear_heads(xd, *cu, want_y=False)
    reg = [t.clone() for t in cu]
    with registered(reg):
        rl, rp, rv, _ = ops.linear_heads(xd, *reg, want_y=False)
        torch.cuda.synchronize()
    assert uy is None
    assert torch.equal(ul, rl) and torch.equal(up, rp) and torch.equal(uv, rv)
    tag = f"composed_heads/F{F}_A{A}_B{B}"
    assert_close(f"{tag}/logp_vs_fp64", ul.cpu().numpy(), lp64, 1e-6)
    assert_close(f"{tag}/pi_vs_fp64", up.cpu().numpy(), np.exp(lp64), 1e-6)
    assert_close(f"{tag}/v_vs_fp64", uv.cpu().numpy(), v64, 1e-6)
    bl, _, bv_, _ = ops.linear_heads(xd[:64].contiguous(), *cu, want_y=False)
    assert_close(f"{tag}/B64_logp_vs_fp64", bl.cpu().numpy(), lp64[:64], 1e-5)
    assert_close(f"{tag}/B64_v_vs_fp64", bv_.cpu().numpy(), v64[:64], 1e-5)


def test_composed_cache_follows_the_weights(ops):
    """Registered W2 and heads: after an in-place change of W2 announced by az_weights_changed
    the result equals, bitwise, the same call on unregistered clones of the new values; the same
    after changing only fc_policy.weight (Wc depends on the heads' weights, which no cache
    depended on before)."""
    F, A, B = 3136, 8, 65
    x, wts = _problem(F, A, B, 5)
    xd = x.cuda()
    reg = [t.cuda() for t in wts]
    with registered(reg):
        first = ops.linear_heads(xd, *reg, want_y=False)
        for which, delta in ((0, 0.01), (2, 0.02)):
            g = torch.Generator().manual_seed(which)
            reg[which].add_((torch.rand(reg[which].shape, generator=g) * delta).cuda())
            _changed()
            got = ops.linear_heads(xd, *reg, want_y=False)
            want = ops.linear_heads(xd, *[t.clone() for t in reg], want_y=False)
            torch.cuda.synchronize()
            for a, b in zip(got[:3], want[:3]):
                assert torch.equal(a, b), f"stale composed heads after changing input {which}"
            assert not torch.equal(got[0], first[0])
            first = got


def test_composed_cache_follows_an_adam_step():
    """One az_adam_step on the GNN's flat parameter buffer (it announces itself): the evaluator
    then equals one built fresh from the stepped values."""
    from azhip import ops
    from azhip.nets import C4Evaluator
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    dev = torch.device("cuda")
    ev = C4Evaluator(synthetic_state_dict(connect4_net_spec(7), 1),
                     synthetic_state_dict(gnn_spec(3136, 2), 2), device=dev)
    rng = np.random.default_rng(3)
    boards = torch.from_numpy(rng.integers(-1, 2, size=(65, 7, 7)).astype(np.int8)).cuda()
    before = [t.clone() for t in ops.c4_gnn_eval(boards, ev.nnet.params, ev.gnn.params)]
    P = ev.gnn.params
    g = torch.Generator().manual_seed(4)
    grad = (torch.rand((P.numel,), generator=g) - 0.5).cuda()
    ops.adam(P.flat, grad, torch.zeros_like(P.flat), torch.zeros_like(P.flat), 1e-2, 1)
    after = ops.c4_gnn_eval(boards, ev.nnet.params, ev.gnn.params)
    fresh = C4Evaluator(ev.nnet.params.cpu_state_dict(), P.cpu_state_dict(), device=dev)
    want = ops.c4_gnn_eval(boards, fresh.nnet.params, fresh.gnn.params)
    torch.cuda.synchronize()
    for a, b in zip(after, want):
        assert torch.equal(a, b)
    assert not torch.equal(after[0], before[0])


@pytest.fixture(scope="module")
def ev():
    from azhip.nets import C4Evaluator
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    W = synthetic_state_dict(connect4_net_spec(7), 1)
    G = synthetic_state_dict(gnn_spec(3136, 2), 2)
    return C4Evaluator(W, G, device=torch.device("cuda"))


def _first_stream_k_rows(cus, N=3136):
    """The smallest M whose M x 3136 x 3136 GEMM takes the stream-K form: the planner's rule
    (az_gemm.hip launch_x3) -- the 256 x 128 tile (M > 256), at least 64 tiles, and a split-K
    grid (S = min(cus / tiles, 8) k splits when tiles < cus) below 90 % of its last round."""
    for M in range(257, 8192):
        tiles = -(-M // 256) * -(-N // 128)
        S = min(256 // tiles, 8) if tiles < 256 else 1
        kc = -(-(-(-N // S)) // 32) * 32 if S > 1 else N
        blocks = tiles * (-(-N // kc) if S > 1 else 1)
        rounds = -(-blocks // cus)
        if tiles >= 64 and blocks / (rounds * cus) < 0.9:
            return M
    raise AssertionError("no stream-K batch size")


@pytest.mark.parametrize("which", ["first", "first_256_tile", "stream_k"])
def test_c4_gnn_eval_fused_equals_unfused(ev, which):
    """ops.c4_gnn_eval equals the unfused calls bitwise on each output_transform.0 dispatch:
    B = 65 (the first row count on the composed path and the first whose GEMM leaves split-K
    slabs: 128 x 128 tiles, 8 k splits), 257 (the first on the 256 x 128 tile, 5 k splits) and
    the first stream-K batch.  The evaluator's hidden scratch rows tell the dispatch apart: the
    fused reduce + heads kernel never writes them (NaN stays), stream-K leaves no slabs and the
    GEMM writes them."""
    from azhip import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = {"first": 65, "first_256_tile": 257, "stream_k": _first_stream_k_rows(cus)}[which]
    Wn, Gn = ev.nnet.params, ev.gnn.params
    rng = np.random.default_rng(B)
    boards = torch.from_numpy(rng.integers(-1, 2, size=(B, 7, 7)).astype(np.int8)).cuda()
    feat = torch.full((B, 3136), float("nan"), device="cuda")
    hidden = torch.full((B, 3136), float("nan"), device="cuda")
    logp, pi, v = ops.c4_gnn_eval(boards, Wn, Gn, feat=feat, hidden=hidden)
    f_u = ops.c4_trunk(boards, Wn)
    h_u = ops.linear(f_u, Gn["output_transform.0.weight"], Gn["output_transform.0.bias"],
                     act=ops.ACT_RELU)
    logp_u, pi_u, v_u, _ = ops.linear_heads(
        h_u, Gn["output_transform.2.weight"], Gn["output_transform.2.bias"],
        Wn["fc_policy.weight"], Wn["fc_policy.bias"], Wn["fc_value.weight"], Wn["fc_value.bias"],
        want_y=False)
    torch.cuda.synchronize()
    assert torch.equal(logp, logp_u) and torch.equal(pi, pi_u) and torch.equal(v, v_u)
    if which == "stream_k":
        assert torch.equal(hidden, h_u)
    else:
        assert bool(torch.isnan(hidden).all())


def test_composed_cache_on_two_streams(ops):
    """The same call on two streams right after a weight change: the first recomputes Wc into the
    entry's other buffer and publishes it after synchronising its stream, the second finds it;
    both equal the single-stream result (the double buffer's contract, as for the W planes)."""
    F, A, B = 3136, 8, 65
    x, wts = _problem(F, A, B, 6)
    xd = x.cuda()
    reg = [t.cuda() for t in wts]
    with registered(reg):
        ops.linear_heads(xd, *reg, want_y=False)
        reg[0].mul_(1.25)
        _changed()
        want = ops.linear_heads(xd, *[t.clone() for t in reg], want_y=False)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        got = []
        for s in streams:
            with torch.cuda.stream(s):
                got.append(ops.linear_heads(xd, *reg, want_y=False))
        torch.cuda.synchronize()
    for r in got:
        for a, b in zip(r[:3], want[:3]):
            assert torch.equal(a, b)
