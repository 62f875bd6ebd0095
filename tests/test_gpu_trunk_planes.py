"""conv2's fp16 fragment planes cached per weight generation (az_weights.hip conv2_planes) against the
in-kernel split: the Connect4 trunk with its weights in registered storage loads the cached planes
(the REGW kernels; 4-wave blocks above B = 512), with the same values in plain unregistered tensors
it stages conv2 through LDS and splits it in every wave.  Both must give the same bits -- the
features, output_transform.0's pre-split A planes and row scales, and the heads taken from the
trunk's LDS rows -- at every kernel form, for channel scales at the edges of the split, and after
in-place weight updates (the cache follows the weight generation).

The A planes and scales have no C-ABI of their own: they are read from the evaluator's workspace,
at the place az_trunk.hip's pre_region puts them (restated in _pre_region below)."""
import ctypes

import numpy as np
import pytest
import torch

F = 3136
CONV = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")


@pytest.fixture(scope="module")
def ev():
    from azhip.nets import C4Evaluator
    from azhip.weights import connect4_net_spec, gnn_spec, synthetic_state_dict
    W = synthetic_state_dict(connect4_net_spec(7), 1)
    G = synthetic_state_dict(gnn_spec(3136, 2), 2)
    return C4Evaluator(W, G, device=torch.device("cuda"))


def _boards(B, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-1, 2, size=(B, 7, 7)).astype(np.int8)


def _unregistered_conv(Wn):
    """Wn's tensors with the four conv tensors cloned out of registered storage."""
    return {k: (Wn[k].clone() if k in CONV else Wn[k]) for k in Wn.keys()}


def _a256(n):
    return (n + 255) // 256 * 256


def _pre_region(ws_bytes, B):
    """(planes offset, planes bytes, scales offset, scales bytes) of az_trunk.hip pre_region."""
    need = _a256(4 * B * F) + _a256(8 * B) + 256
    base = (ws_bytes - need + 255) // 256 * 256
    return base, 4 * B * F, base + _a256(4 * B * F), 8 * B


def _eval(boards, W, G, both):
    """One az_c4_eval_fwd call on a workspace of its own.  Returns the outputs and the pre-split A
    region (planes, scales) as left in the workspace, None where the call did not write it (the
    region is filled with 0xFF bytes first)."""
    from azhip import _lib
    L = _lib.lib()
    B, A, dev = boards.shape[0], W["fc_policy.weight"].shape[0], boards.device
    ws = torch.empty((max(int(L.az_transform_heads_ws_bytes(B, F, A)), 96 << 20),),
                     dtype=torch.uint8, device=dev)
    po, pn, so, sn = _pre_region(ws.numel(), B)
    ws[po:po + pn].fill_(0xFF)
    ws[so:so + sn].fill_(0xFF)
    feat, hidden, y = (torch.empty((B, F), device=dev) for _ in range(3))
    logp, glogp, pi, gpi = (torch.zeros((B, A), device=dev) for _ in range(4))
    v, gv = (torch.zeros((B,), device=dev) for _ in range(2))
    P = lambda t: t.data_ptr()  # noqa: E731
    desc = _lib.C4Eval(
        P(W["conv1.weight"]), P(W["conv1.bias"]), P(W["conv2.weight"]), P(W["conv2.bias"]),
        P(W["fc_policy.weight"]), P(W["fc_policy.bias"]), P(W["fc_value.weight"]),
        P(W["fc_value.bias"]), A, P(G["output_transform.0.weight"]),
        P(G["output_transform.0.bias"]), P(G["output_transform.2.weight"]),
        P(G["output_transform.2.bias"]), B, P(feat), P(hidden), P(y), P(logp), P(glogp), P(ws),
        ws.numel())
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(L.az_c4_eval_fwd(ctypes.byref(desc), vp(boards), B, vp(pi) if both else None,
                                vp(v) if both else None, vp(gpi), vp(gv),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "az_c4_eval_fwd")
    torch.cuda.synchronize()
    sc = ws[so:so + sn].clone()
    wrote = not bool((sc == 0xFF).all())
    return {"pi": pi, "v": v, "logp": logp, "gpi": gpi, "gv": gv, "glogp": glogp,
            "planes": ws[po:po + pn].clone() if wrote else None, "scales": sc if wrote else None}


def _same_eval(a, b, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    assert (a["planes"] is None) == (b["planes"] is None)
    if a["planes"] is not None:
        assert torch.equal(a["scales"], b["scales"]), "A row scales"
        assert torch.equal(a["planes"], b["planes"]), "A planes"


# B = 9, 64: one 8-wave block per CU at most; 257: just over; 512: the benchmark's NB = 1 split-A
# form, two blocks per CU; 513: the first size in the 4-wave form (three 8-wave rounds);
# 1,100: past one round of 4-wave blocks (1,024), ragged last round.  The unregistered side picks
# its own NB (2, 3 staged forms here), so every pair also crosses two row-tile orders.
@pytest.mark.gpu
@pytest.mark.parametrize("B", [9, 64, 257, 512, 513, 1100])
def test_cached_planes_equal_in_kernel_split(ev, B):
    from azhip import ops
    Wn, Gn = ev.nnet.params, ev.gnn.params
    Wc = _unregistered_conv(Wn)
    boards = torch.from_numpy(_boards(B, B)).cuda()
    feat_r = ops.c4_trunk(boards, Wn)
    feat_u = ops.c4_trunk(boards, Wc)
    torch.cuda.synchronize()
    bad = torch.nonzero((feat_r != feat_u).any(1)).flatten().tolist()
    assert not bad, f"B={B}: {len(bad)} feature rows differ, first {bad[:8]}"
    r = _eval(boards, Wn, Gn, both=False)
    u = _eval(boards, Wc, Gn, both=False)
    if 64 < B <= 1024:
        assert r["planes"] is not None, "the registered trunk hands its rows over pre-split"
    _same_eval(r, u, ("gpi", "gv", "glogp"))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [400, 700])
def test_heads_from_trunk_rows_equal(ev, B):
    """predict_both above the one-launch trunk + heads size: the split-A trunk also runs the
    standard heads on its LDS rows (trunk_rows_heads), in 8-wave blocks at every size; B = 400
    and 700 take different boards per block."""
    Wn, Gn = ev.nnet.params, ev.gnn.params
    boards = torch.from_numpy(_boards(B, B)).cuda()
    r = _eval(boards, Wn, Gn, both=True)
    u = _eval(boards, _unregistered_conv(Wn), Gn, both=True)
    assert r["planes"] is not None
    _same_eval(r, u, ("pi", "v", "logp", "gpi", "gv", "glogp"))
    assert float(r["pi"].sum()) > 0 and bool(torch.isfinite(r["v"]).all())


def _edge_weights():
    """Synthetic Connect4Net weights with conv2 output channels at the split's scale edges:
    0 all zeros, 1 largest weight ~1e-30, 2 largest ~1e30 (h3_scale's exponents 113 and -86, inside
    its +-120 clamp: the scales stay exact powers of two and no scaled product overflows), 3 one
    non-zero (positive) tap.  Channels 1 to 3 get a zero bias, so their outputs keep the weights'
    magnitude and the single tap shows.  Channel 2's weights are all positive: with mixed signs
    some of its outputs cancel to 1e-4 of their 288 products' magnitudes, where no fp32
    accumulation holds rtol = 1e-5 (and atol = 1e-5 means nothing at 1e30); channel 1 keeps its
    mixed signs and is held to the format-derived bound instead."""
    from azhip.weights import connect4_net_spec, synthetic_state_dict
    sd = synthetic_state_dict(connect4_net_spec(7), 5)
    w, b = sd["conv2.weight"], sd["conv2.bias"]
    w[0] = 0.0
    w[1] *= np.float32(1e-30) / np.abs(w[1]).max()
    w[2] = np.abs(w[2]) * (np.float32(1e30) / np.abs(w[2]).max())
    keep = np.abs(w[3, 17, 1, 2])
    w[3] = 0.0
    w[3, 17, 1, 2] = keep
    b[1] = b[2] = b[3] = 0.0
    return sd


def _edge_reference(sd, bnp):
    """float64 features and, per output, S = sum |a| |w| over conv2's 288 products (conv1's
    outputs a are >= 0 after the ReLU, so S is conv2 of |w| with no bias)."""
    from oracle import nets as O
    W64 = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    ref = O.c4_features(bnp, W64)
    Wabs = dict(W64)
    Wabs["conv2.weight"] = np.abs(W64["conv2.weight"])
    Wabs["conv2.bias"] = np.zeros_like(W64["conv2.bias"])
    return ref, O.c4_features(bnp, Wabs)


# Error bound of one conv2 output from the number formats.  Each operand x of a scaled row keeps
# |x s - h - l| <= 2^-22 |x s|, or 2^-39 of the row's largest value where l is subnormal (az_x3.h),
# and the l * l product is dropped: <= 3 * 2^-22 |a| |w| per product plus the floors,
# <= 2 * 2^-39 a_max w_max each.  The fp32 accumulation of 288 products + bias + scaling adds
# <= 290 * 2^-24 S, conv1's own fp32 fma chain (10 roundings) <= 10 * 2^-24 of a.  With
# S = sum |a| |w| over the 288 products: |err| <= EDGE_REL S + EDGE_FLOOR a_max w_max.
EDGE_REL = 3 * 2.0 ** -22 + 300 * 2.0 ** -24
EDGE_FLOOR = 288 * 2.0 ** -38


def _edge_bound(sd, S):
    """[9][64][49] bound; a_max <= max_c (sum |w1_c| + |b1_c|) for boards in {-1, 0, 1}."""
    a_max = (np.abs(sd["conv1.weight"].astype(np.float64)).reshape(32, 9).sum(1) +
             np.abs(sd["conv1.bias"].astype(np.float64))).max()
    w_max = np.abs(sd["conv2.weight"].astype(np.float64)).reshape(64, -1).max(1)
    return EDGE_REL * S.reshape(9, 64, 49) + (EDGE_FLOOR * a_max * w_max)[None, :, None]


def test_scale_edge_reference_is_meaningful():
    """CPU part of the edge-case check (the GPU test below relies on it; no GPU needed): the
    float64 reference is finite and fits fp32; the 1e-30 channel's outputs sit 24 orders of
    magnitude under the 1e-5 absolute tolerance, which alone would pass anything there, so the
    scaled channels also get the format-derived bound (_edge_bound), which resolves them."""
    sd = _edge_weights()
    ref, S = _edge_reference(sd, _boards(9, 9))
    assert np.isfinite(ref).all() and np.abs(ref).max() < 3e38
    r = ref.reshape(9, 64, 49)
    assert (r[:, 0] == np.maximum(sd["conv2.bias"][0], 0)).all()      # zero channel: relu(bias)
    assert 0 < r[:, 1].max() < 1e-29 and r[:, 2].max() > 1e29
    assert (r[:, 3] > 0).any()
    assert np.allclose(r[:, 2], S.reshape(9, 64, 49)[:, 2], rtol=1e-12)   # no cancellation there:
    # rtol * |ref| = 1e-5 S is 14x the split's 3 * 2^-22 S, so the tolerance is reachable and tight
    bound = _edge_bound(sd, S)
    assert bound[:, 1].max() < 1e-32              # the derived bound resolves the tiny channel
    assert (bound[:, 1:3] < 1e-3 * r[:, 1:3].max(axis=(0, 2))[None, :, None]).all()


@pytest.mark.gpu
def test_scale_edge_cases(ev):
    from azhip import ops
    from azhip.params import FlatParams
    from azhip.weights import connect4_net_spec
    sd = _edge_weights()
    bnp = _boards(9, 9)
    boards = torch.from_numpy(bnp).cuda()
    Pn = FlatParams(connect4_net_spec(7), "cuda", init=sd)
    Wc = {k: Pn[k].clone() for k in Pn.keys()}
    feat_r = ops.c4_trunk(boards, Pn)
    feat_u = ops.c4_trunk(boards, Wc)
    r = _eval(boards, Pn, ev.gnn.params, both=False)
    u = _eval(boards, {k: (Wc[k] if k in CONV else Pn[k]) for k in Pn.keys()}, ev.gnn.params,
              both=False)
    torch.cuda.synchronize()
    assert torch.equal(feat_r, feat_u)
    _same_eval(r, u, ())
    got = feat_r.double().cpu().numpy()
    ref, S = _edge_reference(sd, bnp)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    e3, bound = err.reshape(9, 64, 49), _edge_bound(sd, S)
    print("edge cases: max err / (1e-5 + 1e-5 |ref|) =",
          float((err / (1e-5 + 1e-5 * np.abs(ref))).max()),
          " max err / bound on the scaled channels =", float((e3[:, 1:3] / bound[:, 1:3]).max()))
    np.testing.assert_allclose(got, ref, atol=1e-5, rtol=1e-5)
    assert (e3[:, 1:3] <= bound[:, 1:3]).all(), "scaled channels: format-derived bound"


@pytest.mark.gpu
def test_cache_follows_weight_updates(ev):
    """torch.optim on registered storage, then the announcement (FlatParams.sync: the version
    counter moved -> az_weights_changed): the next call splits the new weights.  Two updates in a
    row, so both buffers of the cache entry are recomputed and published."""
    from azhip import ops
    from azhip.params import FlatParams
    from azhip.weights import connect4_net_spec, synthetic_state_dict
    Pn = FlatParams(connect4_net_spec(7), "cuda", init=synthetic_state_dict(connect4_net_spec(7), 3))
    boards = torch.from_numpy(_boards(64, 64)).cuda()
    w = Pn["conv2.weight"]
    opt = torch.optim.SGD([w], lr=0.05)
    prev = ops.c4_trunk(boards, Pn).clone()
    for step in range(2):
        g = torch.Generator().manual_seed(step)
        w.grad = (torch.rand(w.shape, generator=g) - 0.5).cuda()
        opt.step()
        Pn.sync()
        got = ops.c4_trunk(boards, Pn)
        want = ops.c4_trunk(boards, {k: Pn[k].clone() for k in Pn.keys()})
        r = _eval(boards, Pn, ev.gnn.params, both=False)
        u = _eval(boards, _unregistered_conv(Pn), ev.gnn.params, both=False)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"stale conv2 planes after update {step}"
        _same_eval(r, u, ("gpi", "gv"))
        assert not torch.equal(got, prev)
        prev = got.clone()
