"""Loss metrics on the MI355X: az_policy_value_metrics against float64 numpy on the same fp32
inputs, evaluate() on every wrapper against float64 metrics of the wrapper's own predictions, and
the per-epoch training losses train() keeps under args.log_losses.

Tolerance of the kernel.  Its only inexact steps are logf / expf and the fp32 products and
half-wave sums of one row (at most 32 terms of one sign); the rows are added in fp64.  The largest
relative error of any sum over every shape of test_kernel_matches_float64, measured on MI355X, is
KERNEL_REL_ERR = 1.05e-7, under two fp32 roundings (each case prints its own); the tests hold
every kernel comparison to 4x that, 4.2e-7.  A difference above 1e-5 would be a bug in the kernel,
not a tolerance, and fails on its own line."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KERNEL_REL_ERR = 1.05e-7         # measured: 1.049e-7 (A = 8, probabilities)
REL_BOUND = 4 * KERNEL_REL_ERR
FLT_MIN = float(np.finfo(np.float32).tiny)
NAMES = ("ce", "se", "top1", "entropy", "target_entropy", "n")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref_sums(p, v, tpi, tv, is_log=False):
    """The six sums in float64 from the fp32 inputs, by include/az_hip.h's rules: a term with
    t == 0 (or p == 0 in the entropy) is 0, log p is never below log(FLT_MIN), ties to the lowest
    index."""
    p64, t64 = np.asarray(p, np.float64), np.asarray(tpi, np.float64)
    B, A = t64.shape
    if is_log:
        lp = np.maximum(p64, math.log(FLT_MIN))
        pr = np.exp(p64)
    else:
        with np.errstate(divide="ignore"):
            lp = np.log(np.maximum(p64, FLT_MIN))
        pr = p64
    ce = -np.where(t64 != 0, t64 * lp, 0.0).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(pr > 0, pr * lp, 0.0).sum()
        tent = -np.where(t64 > 0, t64 * np.log(np.where(t64 > 0, t64, 1.0)), 0.0).sum()
    d = np.asarray(tv, np.float64).reshape(-1) - np.asarray(v, np.float64).reshape(-1)
    top = float((np.argmax(p64, 1) == np.argmax(t64, 1)).sum()) if B else 0.0
    return np.array([ce, (d * d).sum(), top, ent, tent, float(B)])


def run_kernel(p, v, tpi, tv, is_log=False, ldp=None, acc=None, accumulate=False):
    """ops.policy_value_metrics on host arrays; p goes into a [B][ldp] buffer whose padding is
    NaN.  Returns the device accumulator."""
    from azhip import ops
    B, A = tpi.shape
    ldp = A if ldp is None else ldp
    buf = np.full((max(B, 1), ldp), np.nan, np.float32)
    buf[:B, :A] = p
    dp = cu(buf)[:B, :A]
    return ops.policy_value_metrics(dp, cu(np.asarray(v, np.float32)), cu(tpi),
                                    cu(np.asarray(tv, np.float32)), acc=acc, accumulate=accumulate,
                                    is_log=is_log)


def inputs(B, A, seed, is_log=False):
    rng = np.random.default_rng(seed)
    z = (3 * rng.standard_normal((B, A))).astype(np.float32)
    z -= z.max(1, keepdims=True) if B else 0
    lse = np.log(np.exp(z.astype(np.float64)).sum(1, keepdims=True))
    logp = (z - lse).astype(np.float32)
    p = np.exp(logp.astype(np.float64)).astype(np.float32)
    tpi = rng.dirichlet(np.ones(A), B).astype(np.float32).reshape(B, A)
    if B > 3:
        tpi[1] = 0
        tpi[1, A // 2] = 1                                  # a one-hot target row
        tpi[2, 0] = 0                                       # a zero among the targets
    v = np.tanh(rng.standard_normal(B)).astype(np.float32)
    tv = rng.choice([-1.0, 1.0, 0.0, 0.5], B).astype(np.float32)
    return (logp if is_log else p), v, tpi, tv


def rel_err(got, ref):
    """Largest relative error of the four inexact sums (a reference of exactly 0 must be met
    exactly); top1 and n are asserted equal."""
    assert got[2] == ref[2] and got[5] == ref[5], (got, ref)
    worst = 0.0
    for k in (0, 1, 3, 4):
        if ref[k] == 0:
            assert got[k] == 0, (NAMES[k], got[k])
        else:
            worst = max(worst, abs(got[k] - ref[k]) / abs(ref[k]))
    assert np.isfinite(got).all()
    return worst


# ------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("is_log", [False, True])
@pytest.mark.parametrize("A", [1, 8, 10, 26, 32])
def test_kernel_matches_float64(A, is_log):
    """Fails without the feature: the library has no az_policy_value_metrics."""
    worst = 0.0
    for B in (1, 2, 63, 64, 65, 257, 1025):
        p, v, tpi, tv = inputs(B, A, 1000 * A + B, is_log)
        got = run_kernel(p, v, tpi, tv, is_log, ldp=A + 3).cpu().numpy()
        e = rel_err(got, ref_sums(p, v, tpi, tv, is_log))
        print(f"metrics A={A} B={B} is_log={int(is_log)}: rel err {e:.3e}")
        worst = max(worst, e)
    print(f"metrics A={A} is_log={int(is_log)}: worst rel err {worst:.3e} (bound {REL_BOUND:.1e})")
    assert worst <= 1e-5, "above 1e-5 is a bug, not a tolerance"
    assert worst <= REL_BOUND


def test_kernel_is_exact_where_float64_is():
    """Data on which the float64 result is exactly representable in the kernel's arithmetic, so
    every sum must EQUAL it: one-hot targets, v / tv small integers, and
    (a) log-probabilities that are small negative integers (is_log): the cross-entropy is an
        integer sum;
    (b) probabilities that are powers of two with p = 1 at the target: log 1 = 0 and the target
        entropy 1 log 1 = 0, whatever powers of two the other entries hold.
    log(2^-k) itself is irrational: no fp32 evaluation equals its float64 value.  For powers of
    two under the target the cross-entropy is therefore held to one fp32 rounding of each row's
    term (2^-24 relative), and to exactly the fp64 sum of the per-row values the same kernel gives
    for each row alone -- the accumulation over rows adds no error of its own."""
    rng = np.random.default_rng(3)
    B, A = 1025, 10
    hot = rng.integers(0, A, B)
    tpi = np.zeros((B, A), np.float32)
    tpi[np.arange(B), hot] = 1
    v = rng.integers(-2, 3, B).astype(np.float32)
    tv = rng.integers(-1, 2, B).astype(np.float32)
    # (a)
    lp = -rng.integers(1, 9, (B, A)).astype(np.float32)
    got = run_kernel(lp, v, tpi, tv, True).cpu().numpy()
    ref = ref_sums(lp, v, tpi, tv, True)
    for k in (0, 1, 2, 4, 5):
        assert got[k] == ref[k], (NAMES[k], got[k], ref[k])
    assert got[0] == float(-lp[np.arange(B), hot].astype(np.float64).sum()) and got[4] == 0
    # (b)
    p = np.exp2(-rng.integers(1, 9, (B, A))).astype(np.float32)
    p[np.arange(B), hot] = 1
    got = run_kernel(p, v, tpi, tv, False).cpu().numpy()
    ref = ref_sums(p, v, tpi, tv, False)
    for k in (0, 1, 2, 4, 5):
        assert got[k] == ref[k], (NAMES[k], got[k], ref[k])
    assert got[0] == 0 and got[2] == B
    # powers of two under the target
    B = 130
    p = np.exp2(-rng.integers(0, 9, (B, A))).astype(np.float32)
    got = run_kernel(p, v[:B], tpi[:B], tv[:B], False).cpu().numpy()
    ref = ref_sums(p, v[:B], tpi[:B], tv[:B], False)
    assert got[1] == ref[1] and got[2] == ref[2] and got[4] == 0 and got[5] == B
    assert abs(got[0] - ref[0]) <= 2.0 ** -24 * ref[0]
    rows = np.zeros(6)
    for b in range(B):
        rows += run_kernel(p[b:b + 1], v[b:b + 1], tpi[b:b + 1], tv[b:b + 1]).cpu().numpy()
    assert (got == rows).all(), (got, rows)


def test_kernel_edge_rows():
    A = 8
    p = np.full((6, A), 1.0 / A, np.float32)
    tpi = np.zeros((6, A), np.float32)
    v = np.zeros(6, np.float32)
    tv = np.zeros(6, np.float32)
    # row 0: an all-zero target row (argmax of the tie is 0, so is the uniform p's)
    # row 1: p == 0 where t == 0 (and NaN / inf there must not matter)
    p[1] = [0.5, 0, 0.5, 0, 0, 0, 0, 0]
    tpi[1] = [0.5, 0, 0.5, 0, 0, 0, 0, 0]
    # row 2: p == 0 where t > 0
    p[2] = [0, 1, 0, 0, 0, 0, 0, 0]
    tpi[2] = [0.25, 0.75, 0, 0, 0, 0, 0, 0]
    # row 3: ties in both argmaxes, lowest index on both sides: p -> 2, t -> 2
    p[3] = [0.1, 0.1, 0.3, 0.3, 0.1, 0.1, 0, 0]
    tpi[3] = [0, 0, 0.4, 0.2, 0.4, 0, 0, 0]
    # row 4: a tie in p only: p -> 1, t -> 5
    p[4] = [0, 0.5, 0, 0, 0, 0.5, 0, 0]
    tpi[4] = [0, 0, 0, 0, 0, 1, 0, 0]
    # row 5: the same tie the other way round: p -> 5, t -> 1 (tie) -> no match
    p[5] = [0, 0.25, 0, 0, 0, 0.75, 0, 0]
    tpi[5] = [0, 0.5, 0, 0, 0, 0.5, 0, 0]
    per_row = []
    for b in range(6):
        got = run_kernel(p[b:b + 1], v[b:b + 1], tpi[b:b + 1], tv[b:b + 1]).cpu().numpy()
        assert np.isfinite(got).all(), (b, got)
        per_row.append(got)
    ln = math.log
    assert per_row[0][0] == 0 and per_row[0][4] == 0 and per_row[0][2] == 1
    assert per_row[0][3] == pytest.approx(ln(A), rel=REL_BOUND)
    assert per_row[1][0] == pytest.approx(ln(2), rel=REL_BOUND)
    assert per_row[1][3] == pytest.approx(ln(2), rel=REL_BOUND) and per_row[1][2] == 1
    assert per_row[2][0] == pytest.approx(-0.25 * ln(FLT_MIN), rel=REL_BOUND)
    assert per_row[2][3] == 0 and per_row[2][2] == 1
    assert [int(r[2]) for r in per_row] == [1, 1, 1, 1, 0, 0]
    whole = run_kernel(p, v, tpi, tv).cpu().numpy()
    assert rel_err(whole, ref_sums(p, v, tpi, tv)) <= REL_BOUND
    assert rel_err(whole, np.sum(per_row, 0)) <= REL_BOUND
    # the zero-target rule holds whatever p is there: NaN and inf included
    bad = p.copy()
    bad[1, 1], bad[1, 3], bad[0, :] = np.nan, np.inf, np.nan
    got = run_kernel(bad, v, tpi, tv).cpu().numpy()
    assert got[0] == whole[0] and np.isfinite(got[[0, 1, 2, 4, 5]]).all()
    # the same rows as log-probabilities: -inf where p == 0
    with np.errstate(divide="ignore"):
        lp = np.log(p.astype(np.float64)).astype(np.float32)
    got = run_kernel(lp, v, tpi, tv, True).cpu().numpy()
    assert np.isfinite(got).all()
    assert rel_err(got, ref_sums(lp, v, tpi, tv, True)) <= REL_BOUND
    assert rel_err(got, whole) <= 2 * REL_BOUND


def test_kernel_no_rows():
    from azhip import ops
    z = np.zeros((0, 8), np.float32)
    e = np.zeros((0,), np.float32)
    acc = torch.full((6,), 7.0, dtype=torch.float64, device="cuda")
    ops.policy_value_metrics(cu(z), cu(e), cu(z), cu(e), acc=acc, accumulate=True)
    assert acc.cpu().tolist() == [7.0] * 6
    ops.policy_value_metrics(cu(z), cu(e), cu(z), cu(e), acc=acc, accumulate=False)
    assert acc.cpu().tolist() == [0.0] * 6


def test_kernel_accumulates_chunks_and_repeats_bits():
    from azhip import ops
    B, A = 1025, 26
    p, v, tpi, tv = inputs(B, A, 77)
    ref = ref_sums(p, v, tpi, tv)
    once = run_kernel(p, v, tpi, tv).cpu().numpy()
    assert rel_err(once, ref) <= REL_BOUND
    dp, dv, dt, dtv = cu(p), cu(v), cu(tpi), cu(tv)

    def chunked():
        acc = torch.zeros((6,), dtype=torch.float64, device="cuda")
        for c0 in range(0, B, 64):
            ops.policy_value_metrics(dp[c0:c0 + 64], dv[c0:c0 + 64], dt[c0:c0 + 64],
                                     dtv[c0:c0 + 64], acc=acc, accumulate=True)
        return acc
    a, b = chunked(), chunked()
    assert torch.equal(a, b)
    assert rel_err(a.cpu().numpy(), ref) <= REL_BOUND
    again = run_kernel(p, v, tpi, tv)
    assert np.array_equal(again.cpu().numpy(), once)
    # without accumulate the call overwrites
    ops.policy_value_metrics(dp, dv, dt, dtv, acc=a)
    assert np.array_equal(a.cpu().numpy(), once)


def test_kernel_rejects_bad_arguments():
    from azhip import _lib
    L = _lib.lib()
    t = torch.zeros(64, device="cuda")
    acc = torch.zeros(6, dtype=torch.float64, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    good = [P(t), 8, 0, P(t), P(t), P(t), 4, 8, P(acc), 0, P(ws), None]
    assert L.az_policy_value_metrics(*good) == 0
    torch.cuda.synchronize()

    def bad(i, val, word):
        a = list(good)
        a[i] = val
        assert L.az_policy_value_metrics(*a) == -1, (i, val)
        assert word in L.az_last_error().decode(), L.az_last_error()
    bad(6, -1, "B=-1")
    bad(7, 0, "A=0")
    bad(7, 33, "A=33")
    bad(1, 7, "ldp")
    bad(2, 2, "is_log")
    bad(8, None, "acc")
    bad(8, ctypes.c_void_p(acc.data_ptr() + 4), "acc")
    bad(0, None, "null")
    bad(3, None, "null")
    bad(4, None, "null")
    bad(5, None, "null")
    bad(10, None, "ws")
    assert L.az_policy_value_metrics_ws_bytes(1025, 8) == 17 * 6 * 8
    assert L.az_policy_value_metrics_ws_bytes(0, 8) == 0
    assert L.az_policy_value_metrics_ws_bytes(4, 33) == 0
    assert acc.cpu().abs().sum().item() >= 0


# ------------------------------------------------------------------------------ evaluate()
class Args(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _play_random(game, rng, count):
    """`count` canonical non-terminal boards from random play."""
    out = []
    while len(out) < count:
        board, cur = game.getInitBoard(), 1
        for _ in range(int(rng.integers(0, 12))):
            valid = np.flatnonzero(game.getValidMoves(board, cur))
            board, cur = game.getNextState(board, cur, int(rng.choice(valid)))
            if game.getGameEnded(board, cur) != 0:
                break
        else:
            out.append(np.array(game.getCanonicalForm(board, cur)))
    return out


def _examples(game, n, seed):
    rng = np.random.default_rng(seed)
    A = game.getActionSize()
    boards = _play_random(game, rng, n)
    pis = rng.dirichlet(np.ones(A), (2, n)).astype(np.float32)
    pis[0, 3] = 0
    pis[0, 3, 1] = 1
    zs = rng.choice([-1.0, 1.0], (2, n))
    std = [(boards[i], pis[0, i], float(zs[0, i])) for i in range(n)]
    gnn = [(boards[i], 1, pis[0, i], 0.0, pis[1, i], float(0.5 * zs[1, i]), float(zs[0, i]))
           for i in range(n)]
    return std, gnn


def _make(kind, **kw):
    from connect4.Connect4Game import Connect4Game
    from connect4.Connect4GNN import Connect4GNNWrapper
    from connect4.Connect4Net import Connect4NNetWrapper
    from tictactoe.TicTacToeGNN import TicTacToeGNNWrapper
    from tictactoe.TicTacToeGame import TicTacToeGame
    from tictactoe.TicTacToeNet import TicTacToeNNetWrapper
    game = {"c4_4x4": lambda: Connect4Game(4), "c4_7x6": lambda: Connect4Game(7, rows=6),
            "ttt_3x3": lambda: TicTacToeGame(3)}[kind]()
    gnn = kw.pop("gnn", False)
    args = Args(dropout=0.3, gnn_layers=2, lr=0.001, epochs=1, batch_size=8, use_gnn=gnn)
    args.update(kw)
    cls = ((Connect4GNNWrapper if gnn else Connect4NNetWrapper) if kind.startswith("c4")
           else (TicTacToeGNNWrapper if gnn else TicTacToeNNetWrapper))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(31)
        return game, cls(game, args)


def _state(w):
    nets_ = [w.nnet] + ([w.gnn] if getattr(w, "has_gnn", False) else [])
    out = []
    for n in nets_:
        P = n.params
        out += [P.flat.clone(), None if P.m is None else P.m.clone(),
                None if P.v is None else P.v.clone(), getattr(P, "step", None), n.training]
    return out + [getattr(w, "train_seed", None)]


def _same_state(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y)
        else:
            assert x == y


def _check_block(got, prefix, ref):
    d = max(ref[5], 1)
    want = {"loss_pi": ref[0] / d, "loss_v": ref[1] / d, "loss": (ref[0] + ref[1]) / d,
            "entropy": ref[3] / d, "target_entropy": ref[4] / d}
    for k, x in want.items():
        assert got[prefix + k] == pytest.approx(x, rel=REL_BOUND), (prefix + k, got[prefix + k], x)
    assert got[prefix + "top1"] == ref[2] / d and got[prefix + "n"] == int(ref[5])


EVAL_CASES = [("c4_4x4", {}), ("c4_7x6", {}), ("ttt_3x3", {}),
              ("c4_4x4", dict(gnn=True)), ("c4_7x6", dict(gnn=True)), ("ttt_3x3", dict(gnn=True)),
              ("c4_4x4", dict(gnn=True, gnn_neighbors=True)),
              ("c4_7x6", dict(gnn=True, gnn_neighbors=True)),
              ("ttt_3x3", dict(gnn=True, gnn_neighbors=True)),
              ("c4_4x4", dict(gnn=True, batch_invariant=True)),
              ("c4_7x6", dict(gnn=True, gnn_neighbors=True, batch_invariant=True))]


@pytest.mark.parametrize("kind,kw", EVAL_CASES,
                         ids=[k + "".join("+" + x for x in kw) for k, kw in EVAL_CASES])
def test_evaluate_equals_float64_metrics_of_the_predictions(kind, kw):
    """70 examples in chunks of 32 (a ragged last chunk).  The reference outputs come from the
    same wrapper's public predictions on the same boards, asked for in the same chunks so that
    they take the launches evaluate() takes (the GEMM dispatch picks its tile by the row count):
    predict_batch (+ predict_batch_with_gnn, the per-board route of predict_both on a batch)
    without gnn_neighbors, predict_both_stars on the child stars with it, predict_both under
    batch_invariant, where one call over all 70 boards gives the same bits.  What is left between
    the two sides is the kernel's own error, so the bound is the kernel's."""
    import stars
    game, w = _make(kind, **dict(kw))
    n, chunk = 70, 32
    std, gnn = _examples(game, n, 5)
    boards = np.stack([e[0] for e in std]).astype(np.int8)
    w.nnet.train()                                   # evaluate must leave the flags as they are
    if w.has_gnn:
        w.gnn.eval()
    w.train_seed = 9
    for net in [w.nnet] + ([w.gnn] if w.has_gnn else []):   # Adam moments that evaluate() must
        net.params.reset_adam()                             # leave alone: real, non-zero tensors
        net.params.m.fill_(0.25)
        net.params.v.fill_(0.5)
        net.params.step = 3
    before = _state(w)
    assert all(x is not None for x in before)
    rs = (np.random.get_state()[1].copy(), torch.random.get_rng_state().clone())
    got = w.evaluate(std, gnn if w.has_gnn else None, chunk=chunk)
    _same_state(before, _state(w))
    assert np.array_equal(rs[0], np.random.get_state()[1])
    assert torch.equal(rs[1], torch.random.get_rng_state())
    outs = []
    for c0 in range(0, n, chunk):
        b = boards[c0:c0 + chunk]
        if kw.get("batch_invariant"):
            continue
        if kw.get("gnn_neighbors"):
            pi, v = w.predict_batch(b)
            rows, offs = stars.board_stars(game, list(b))
            spi, sv, gpi, gv = w.predict_both_stars(rows, offs)
            outs.append((pi, v, gpi, gv, spi, sv))
        elif w.has_gnn:
            pi, v = w.predict_batch(b)
            gpi, gv = w.predict_batch_with_gnn(b)
            outs.append((pi, v, gpi, gv, pi, v))
        else:
            outs.append(w.predict_batch(b))
    if kw.get("batch_invariant"):
        pi, v, gpi, gv = w.predict_both(boards)
        if kw.get("gnn_neighbors"):
            rows, offs = stars.board_stars(game, list(boards))
            spi, sv, gpi, gv = w.predict_both_stars(rows, offs)
            assert np.array_equal(spi, pi) and np.array_equal(sv, v)
        outs.append((pi, v, gpi, gv, pi, v))
    cat = [np.concatenate([o[i] for o in outs]) for i in range(len(outs[0]))]
    tpi = np.stack([e[1] for e in std]).astype(np.float32)
    tv = np.array([e[2] for e in std], np.float32)
    _check_block(got, "", ref_sums(cat[0], cat[1], tpi, tv))
    if w.has_gnn:
        epi = np.stack([e[4] for e in gnn]).astype(np.float32)
        ev = np.array([e[5] for e in gnn], np.float32)
        _check_block(got, "gnn_", ref_sums(cat[2], cat[3], epi, ev))
        _check_block(got, "std_on_gnn_", ref_sums(cat[4], cat[5], epi, ev))
        assert got["gnn_loss"] != got["std_on_gnn_loss"]
        assert len(got) == 21
    else:
        assert len(got) == 7
    # the result repeats bit for bit (the predictions above switched to eval mode: put the flags
    # back where evaluate() has to leave them)
    w.nnet.train()
    if w.has_gnn:
        w.gnn.eval()
    assert w.evaluate(std, gnn if w.has_gnn else None, chunk=chunk) == got
    whole = w.evaluate(std, gnn if w.has_gnn else None)
    assert whole["n"] == n and whole["top1"] == got["top1"]
    # no examples: zeros, no NaN
    empty = w.evaluate([], [] if w.has_gnn else None)
    assert set(empty) == set(got) and all(x == 0 for x in empty.values())
    only_std = w.evaluate(std, chunk=chunk)
    assert set(only_std) == set(NAMES_OUT) and only_std["loss"] == got["loss"]
    _same_state(before, _state(w))


NAMES_OUT = ("loss_pi", "loss_v", "loss", "top1", "entropy", "target_entropy", "n")


def test_evaluate_frozenlake():
    from test_gpu_frozenlake import _train_fixture, _weights, _wrapper
    z, shape, kw, examples = _train_fixture("fl_train_4")
    w = _wrapper(*shape, _weights(z, "start."), **kw)
    ex = (list(examples) * 70)[:70]
    w.nnet.train()
    P = w.nnet.params
    P.reset_adam()
    P.m.fill_(0.25)
    P.v.fill_(0.5)
    P.step = 3
    before = [P.flat.clone(), P.m.clone(), P.v.clone()]
    rs = np.random.get_state()[1].copy()
    got = w.evaluate(ex, chunk=32)
    assert torch.equal(before[0], P.flat) and w.nnet.training is True
    assert torch.equal(before[1], P.m) and torch.equal(before[2], P.v) and P.step == 3
    assert np.array_equal(rs, np.random.get_state()[1])
    pis, vs = [], []
    for c0 in range(0, 70, 32):
        pi, v = w._eval_nodes([w._nodes_of(np.asarray(e[0], np.float32)) for e in ex[c0:c0 + 32]])
        pis.append(pi)
        vs.append(v)
    tpi = np.stack([e[1] for e in ex]).astype(np.float32)
    tv = np.array([e[2] for e in ex], np.float64).astype(np.float32)
    _check_block(got, "", ref_sums(np.concatenate(pis), np.concatenate(vs), tpi, tv))
    pb, vb = w.predict_batch([e[0] for e in ex[:8]])
    assert np.array_equal(pb, pis[0][:8]) and np.array_equal(vb, vs[0][:8])
    empty = w.evaluate([])
    assert set(empty) == set(NAMES_OUT) and all(x == 0 for x in empty.values())


# ------------------------------------------------------------------------------ train()
def _loss_ref(kind, dtype, W, G, boards, tpi, tv, mask, p, star):
    """(l_pi, l_v) of train()'s loss in `dtype` from oracle.torch_ref."""
    from oracle import torch_ref as R
    Pn = R.params(W, dtype, requires_grad=False)
    with torch.no_grad():
        f = R.c4_features(boards, Pn, mask, p)
        if G is not None:
            f = R.policy_value_gnn(f, R.params(G, dtype, requires_grad=False)) if star is None \
                else star(f, R.params(G, dtype, requires_grad=False))
        logp, v = R.c4_heads(f, Pn)
        t = torch.as_tensor(tpi).to(dtype)
        z = torch.as_tensor(tv).to(dtype)
        B = t.shape[0]
        return float(-(t * logp).sum() / B), float(((z - v) ** 2).sum() / B)


@pytest.mark.parametrize("star_train", [False, True])
def test_train_keeps_its_epoch_losses(star_train):
    """One-epoch train() runs from a saved state on Connect4 4x4 with args.log_losses:
    last_train_losses[0] against the loss recomputed in float64 (oracle.torch_ref) from a forward
    at the weights that epoch started from -- the same draw, the same dropout mask -- to the
    criterion tests/gradcheck.py applies to losses (check_grad without S: 10x torch's own fp32
    error of the same restatement plus 1e-7 of the value); and the weights after train() are the
    same bits with the key on and off.  The GNN step is the star over the batch, or every example
    on its own child star (gnn_neighbors_train)."""
    import stars
    from azhip import ops
    from gradcheck import check_grad
    from test_gpu_star_train import forest
    from oracle import torch_ref as R
    kw = dict(gnn=True, gnn_neighbors=True, gnn_neighbors_train=True) if star_train \
        else dict(gnn=True)
    game, w = _make("c4_4x4", log_losses=True, **kw)
    _, off = _make("c4_4x4", **kw)
    std, gnn = _examples(game, 12, 8)
    W = {k: t.numpy() for k, t in w.nnet.params.cpu_state_dict().items()}
    G = {k: t.numpy() for k, t in w.gnn.params.cpu_state_dict().items()}
    off.nnet.params.copy_flat_(w.nnet.params.flat)
    off.gnn.params.copy_flat_(w.gnn.params.flat)
    assert not hasattr(off, "last_train_losses")
    np.random.seed(21)
    w.train(std, gnn)
    np.random.seed(21)
    off.train(std, gnn)
    assert torch.equal(w.nnet.params.flat, off.nnet.params.flat)
    assert torch.equal(w.gnn.params.flat, off.gnn.params.flat)
    assert not hasattr(off, "last_train_losses") and w.train_seed == off.train_seed == 2
    (rec,) = w.last_train_losses
    assert rec["epoch"] == 0 and set(rec) == {"epoch", "loss_pi", "loss_v", "loss", "gnn_loss_pi",
                                             "gnn_loss_v", "gnn_loss"}
    # the CNN step's draw and mask (train_seed 1), at the starting weights
    np.random.seed(21)
    idx = np.random.randint(0, len(std), min(len(std), 8))
    boards = np.stack([std[i][0] for i in idx]).astype(np.int8)
    tpi = np.stack([std[i][1] for i in idx]).astype(np.float32)
    tv = np.array([std[i][2] for i in idx], np.float32)
    Fd = w.nnet.feature_dim
    m = ops.dropout_mask(len(idx) * Fd, 0.3, 1, "cuda").cpu().numpy().reshape(len(idx), Fd)
    l64 = _loss_ref("c4", torch.float64, W, None, boards, tpi, tv, m, 0.3, None)
    l32 = _loss_ref("c4", torch.float32, W, None, boards, tpi, tv, m, 0.3, None)
    print(f"train loss cnn: got {rec['loss_pi']}, {rec['loss_v']} ref {l64}")
    check_grad("train_losses/l_pi", rec["loss_pi"], l64[0], l32[0])
    check_grad("train_losses/l_v", rec["loss_v"], l64[1], l32[1])
    assert rec["loss"] == pytest.approx(rec["loss_pi"] + rec["loss_v"], rel=1e-12)
    # the GNN step's draw and mask (train_seed 2), at the board network's weights after its step
    W1 = {k: t.numpy() for k, t in w.nnet.params.cpu_state_dict().items()}
    gidx = np.random.randint(0, len(gnn), min(len(gnn), 8))
    gb = [gnn[i][0] for i in gidx]
    epi = np.stack([gnn[i][4] for i in gidx]).astype(np.float32)
    ev = np.array([gnn[i][5] for i in gidx], np.float32)
    if star_train:
        rows, offs = stars.board_stars(game, gb)
        sizes = np.diff(offs)
        _, rowptr, col = forest(sizes.tolist())
        first = torch.as_tensor(offs[:-1].astype(np.int64))

        def star(f, PG):
            return R.policy_value_gnn(f, PG, 2, rowptr, col)[first]
        boards_g = rows.astype(np.int8)
    else:
        star, boards_g = None, np.stack(gb).astype(np.int8)
    V = len(boards_g)
    gm = ops.dropout_mask(V * Fd, 0.3, 2, "cuda").cpu().numpy().reshape(V, Fd)
    g64 = _loss_ref("c4", torch.float64, W1, G, boards_g, epi, ev, gm, 0.3, star)
    g32 = _loss_ref("c4", torch.float32, W1, G, boards_g, epi, ev, gm, 0.3, star)
    print(f"train loss gnn: got {rec['gnn_loss_pi']}, {rec['gnn_loss_v']} ref {g64}")
    check_grad("train_losses/gnn_l_pi", rec["gnn_loss_pi"], g64[0], g32[0])
    check_grad("train_losses/gnn_l_v", rec["gnn_loss_v"], g64[1], g32[1])


def test_train_keeps_the_cnn_loss_when_the_rows_are_split(monkeypatch):
    """train_parallel = "allreduce" splits the CNN step's rows over the ranks; each rank keeps its
    rows' part of the loss and the parts are summed once after the last epoch.  On one rank the
    split step holds every row, so its record and its weights are those of the plain step."""
    game, plain = _make("c4_4x4", log_losses=True, epochs=2)
    _, split = _make("c4_4x4", log_losses=True, epochs=2)
    split.nnet.params.copy_flat_(plain.nnet.params.flat)
    monkeypatch.setattr(type(split), "_dp_world", lambda self: 2 if self is split else 1)
    std, _ = _examples(game, 12, 8)
    np.random.seed(4)
    plain.train(std)
    np.random.seed(4)
    split.train(std)
    assert torch.equal(plain.nnet.params.flat, split.nnet.params.flat)
    assert len(plain.last_train_losses) == 2 and "loss_pi" in plain.last_train_losses[1]
    assert split.last_train_losses == plain.last_train_losses


def test_train_keeps_frozenlake_epoch_losses():
    """FrozenLake's slot per epoch.  (1) One epoch whose single batch holds every example, from the
    saved weights: last_train_losses[0]["loss"] against the loss of tests/fl_ref.py's float64
    restatement on the leaves train() builds, to the criterion tests/gradcheck.py applies to
    losses (check_grad without S: 10x the float32 restatement's own error plus 1e-7 of the
    value).  (2) Two epochs of three batches: every slot is the mean of its own epoch's batch
    losses, bit for bit those of the same steps replayed by hand, and the weights after train()
    are the same bits with the key on and off."""
    import fl_ref
    from gradcheck import check_grad
    from test_gpu_frozenlake import _train_fixture, _weights, _wrapper
    z, shape, kw, examples = _train_fixture("fl_train_4")
    examples = list(examples)
    W = _weights(z, "start.")
    # (1)
    one = dict(kw, epochs=1, batch_size=len(examples))
    w = _wrapper(*shape, W, log_losses=True, **one)
    np.random.seed(3)
    w.train(list(examples))
    (rec,) = w.last_train_losses
    assert set(rec) == {"epoch", "loss"} and rec["epoch"] == 0
    lists = [w._nodes_of(np.asarray(e[0], dtype=np.float32)) for e in examples]
    S = shape[0] * shape[0]
    nodes = np.zeros((len(lists), 5, S), np.float32)
    counts = np.array([len(nl) for nl in lists], np.int32)
    for i, nl in enumerate(lists):
        nodes[i, :len(nl)] = np.asarray(nl, np.float32).reshape(len(nl), S)
    assert counts.min() >= 1 and counts.max() > 1
    tpi = np.stack([e[1] for e in examples]).astype(np.float32)
    tv = np.array([e[2] for e in examples], np.float64).astype(np.float32)
    ref = {}
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            pi, v, _ = fl_ref.forward(fl_ref.params(W, dt), nodes, counts)
            ref[dt] = float(fl_ref.loss_of(pi, v, tpi, tv))
    print(f"frozenlake train loss: got {rec['loss']} ref {ref[torch.float64]} "
          f"(float32 restatement {ref[torch.float32]})")
    check_grad("train_losses/frozenlake", rec["loss"], ref[torch.float64], ref[torch.float32])
    # (2)
    assert len(examples) > 2 * kw["batch_size"] and kw["epochs"] >= 2
    on = _wrapper(*shape, W, log_losses=True, **kw)
    off = _wrapper(*shape, W, **kw)
    np.random.seed(int(z["np_seed"]))
    on.train(list(examples))
    np.random.seed(int(z["np_seed"]))
    off.train(list(examples))
    assert torch.equal(on.nnet.params.flat, off.nnet.params.flat)
    assert not hasattr(off, "last_train_losses")
    hand = _wrapper(*shape, W, **kw)
    hand.nnet.params.reset_adam()
    np.random.seed(int(z["np_seed"]))
    ex, want = list(examples), []
    for _ in range(kw["epochs"]):
        np.random.shuffle(ex)
        losses = []
        for i in range(0, len(ex), kw["batch_size"]):
            boards, pis, vs = list(zip(*ex[i:i + kw["batch_size"]]))
            losses.append(hand.train_step(boards, pis, vs))
        want.append(float(torch.cat(losses).mean().item()))
    assert torch.equal(hand.nnet.params.flat, on.nnet.params.flat)
    assert on.last_train_losses == [{"epoch": e, "loss": x} for e, x in enumerate(want)]
    assert want[0] != want[1]
    # too few examples: train() returns before any epoch, and no earlier run's losses remain
    on.train(list(examples)[:3])
    assert on.last_train_losses == []
