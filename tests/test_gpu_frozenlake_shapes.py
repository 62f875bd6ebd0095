"""FrozenLakeNet's kernels over the grid they accept (S in 4..64, embedding_dim 64 or 128,
gnn_layers 1..4), against tests/fl_ref.py in float64 -- the restatement tests/test_fl_ref.py holds
to the recorded goldens.  tests/test_gpu_frozenlake.py reaches (S 16, E 64, L 2), (S 64, E 128,
L 3) and (S 64, E 64, L 2) only.

Cases (S, E, L, B):
  all eight (E, L) at S = 16 (4x4) and S = 25 (5x5), B = 12
  (E 64, L 1) and (E 128, L 4) at S = 4 (2x2, the minimum), 15 (3x5: fe0 rows start at odd float
  offsets), 63 (7x9) and 64, B = 12
  B = 1 at (25, 64, 4) and (16, 128, 1);  B = 300 at (25, 64, 3) on a net that served B = 12
  first: fl_wgrad_kernel's serial leaf loops, and max_B raised mid-life through grad_ws
Leaves: counts cycle 1..5 (B = 12: every count at least twice), node rows at and beyond counts[b]
are NaN, rows are 0/1 boards and every fourth a real-valued one.  Weights are Xavier-normal under
a fixed seed, biases uniform in (-0.1, 0.1): zero biases hide a wrong bias path.

Bars: pi and v within 1e-5 (the project's).  Gradients, written into buffers full of NaN: relative
to the tensor's largest |float64 gradient| 1e-5, widened to 4 x the float32 restatement's own
deviation where that exceeds 2.5e-6 (tests/golden/make_frozenlake_goldens.py's bar, computed here
from the reference alone; every widened tensor goes through conftest.report).  Before anything is
compared every float64 reference tensor is non-zero and at least 1/8 of the hidden units are live
after the feature extractor and after every layer (gradcheck.MIN_LIVE's spirit);
test_references_are_not_vacuous holds the references to that on the CPU."""
import numpy as np
import pytest

from conftest import assert_close, golden, report

torch = pytest.importorskip("torch")

import fl_ref  # noqa: E402
from gradcheck import MIN_LIVE, targets  # noqa: E402

gpu = pytest.mark.gpu
TOL = 1e-5
BOARDS = {4: (2, 2), 15: (3, 5), 16: (4, 4), 25: (5, 5), 63: (7, 9), 64: (8, 8)}
EL = [(E, L) for E in (64, 128) for L in (1, 2, 3, 4)]
GRID = [(S, E, L, 12) for S in (16, 25) for E, L in EL]
EDGES = [(S, E, L, 12) for S in (4, 15, 63, 64) for E, L in ((64, 1), (128, 4))]
SINGLE = [(25, 64, 4, 1), (16, 128, 1, 1)]
MANY = (25, 64, 3, 300)
CASES = GRID + EDGES + SINGLE + [MANY]
_REF = {}


def seed_of(S, E, L, B):
    return 1000 * S + E + 10 * L + B


def weights(S, E, L, seed):
    """Xavier-normal weights (std = sqrt(2 / (fan_in + fan_out))), biases uniform in (-0.1, 0.1)."""
    gen = torch.Generator().manual_seed(seed)
    W = {}
    for name, shape in fl_ref.spec(S, E, L):
        if name.endswith("weight"):
            std = (2.0 / (shape[0] + shape[1])) ** 0.5
            W[name] = (torch.randn(shape, generator=gen) * std).numpy()
        else:
            W[name] = (torch.rand(shape, generator=gen) * 0.2 - 0.1).numpy()
    return W


def leaves(S, B, seed):
    """nodes [B][5][S] (NaN at and beyond counts[b]), counts cycling 1..5."""
    rng = np.random.default_rng(seed)
    shift = 0 if B > 1 else (S + 3) % 5                   # B = 1: 4 nodes at S = 25, 5 at S = 16
    counts = np.array([1 + (i + shift) % 5 for i in range(B)], np.int32)
    nodes = np.full((B, 5, S), np.nan, np.float32)
    for b in range(B):
        for j in range(counts[b]):
            if (b + j) % 4 == 3:
                nodes[b, j] = rng.uniform(-1, 1, S)
            else:
                nodes[b, j] = rng.random(S) < 0.3
    return nodes, counts


def reference(case, W=None, tpi=None):
    """The case's inputs and its float64 / float32 restatement, computed once and shared."""
    key = case if W is None else None
    if key is None or key not in _REF:
        S, E, L, B = case[:4]
        seed = seed_of(S, E, L, B)
        nodes, counts = leaves(S, B, seed)
        tp, tv = targets(B, 4, seed + 1)
        r = {"W": weights(S, E, L, seed) if W is None else W, "nodes": nodes, "counts": counts,
             "tpi": tp if tpi is None else tpi, "tv": tv}
        r["r64"] = fl_ref.grads(r["W"], nodes, counts, r["tpi"], tv, torch.float64)
        r["r32"] = fl_ref.grads(r["W"], nodes, counts, r["tpi"], tv, torch.float32)
        r["bars"], r["widened"] = fl_ref.bars(r["r64"]["grads"], r["r32"]["grads"])
        r["live"] = fl_ref.live_fractions(r["W"], nodes, counts)
        if key is None:
            return r
        _REF[key] = r
    return _REF[key]


def guard(name, r):
    for k, g in r["r64"]["grads"].items():
        assert np.abs(g).max() > 0, (name, k, "all-zero reference")
    assert len(r["live"]) == fl_ref.num_layers(r["W"]) + 1
    assert min(r["live"]) >= MIN_LIVE, (name, r["live"])


def name_of(case):
    return "fl_shapes/S{}_E{}_L{}_B{}".format(*case)


def id_of(case):
    return "S{}-E{}-L{}-B{}".format(*case)


@pytest.mark.parametrize("case", CASES, ids=id_of)
def test_references_are_not_vacuous(case):
    """CPU: every case's float64 reference has no all-zero tensor and enough live units."""
    r = reference(case)
    guard(name_of(case), r)
    if case[3] == 12:
        assert all((r["counts"] == n).sum() >= 2 for n in range(1, 6))
    assert set(r["counts"].tolist()) <= {1, 2, 3, 4, 5}


# ------------------------------------------------------------------------------------ GPU side
def make_net(S, E, L, W):
    from azhip.frozenlake import EnhancedNNet
    net = EnhancedNNet(BOARDS[S], 4, {"embedding_dim": E, "gnn_layers": L})
    assert (net.S, net.E, net.L) == (S, E, L)
    net.load_state_dict(W)
    return net


def dev(net, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(net.device)


def evaluate(net, nodes, counts):
    from azhip.frozenlake import fl_eval_fwd
    B = len(counts)
    pi = torch.full((B, 4), float("nan"), device=net.device)
    v = torch.full((B,), float("nan"), device=net.device)
    fl_eval_fwd(net, dev(net, nodes), dev(net, counts), pi, v, B)
    torch.cuda.synchronize()
    return pi.cpu(), v.cpu()


def gradients(net, r, want_dlogits=False):
    """az_fl_grads into gradient buffers full of NaN -> (loss, dlogits, {name: numpy})."""
    from azhip.frozenlake import fl_grads
    net.params.grad_flat.fill_(float("nan"))
    loss, dl = fl_grads(net, dev(net, r["nodes"]), dev(net, r["counts"]), dev(net, r["tpi"]),
                        dev(net, r["tv"]), want_dlogits=want_dlogits)
    torch.cuda.synchronize()
    return loss.cpu(), dl, {k: g.cpu().numpy().copy() for k, g in net.params.grads.items()}


def check_forward(name, net, r):
    pi, v = evaluate(net, r["nodes"], r["counts"])
    e_pi = assert_close(f"{name}/pi", pi.numpy(), r["r64"]["pi"], TOL)
    e_v = assert_close(f"{name}/v", v.numpy(), r["r64"]["v"], TOL)
    print(f"{name}: pi max err {e_pi:.3g} ({TOL / max(e_pi, 1e-300):.1f}x), "
          f"v max err {e_v:.3g} ({TOL / max(e_v, 1e-300):.1f}x)")


def check_tensors(name, got, ref, r):
    """Every tensor against `ref` at the case's bars, relative to the reference's largest entry."""
    assert set(got) == set(ref)
    worst = 0.0
    for k, g in got.items():
        top = float(np.abs(ref[k]).max())
        assert top > 0, (name, k)
        if k in r["widened"]:
            report(f"{name}/widened/{k}", float32_deviation=r["widened"][k], bar=r["bars"][k])
            print(f"{name}: widened {k}: float32 deviation {r['widened'][k]:.3g} "
                  f"bar {r['bars'][k]:.3g}")
        err = assert_close(f"{name}/{k}", g / top, ref[k] / top, r["bars"][k])
        worst = max(worst, err / r["bars"][k])
    print(f"{name}: worst gradient error / bar {worst:.3g}")


def check_gradients(name, net, r, want_dlogits=False):
    loss, dl, got = gradients(net, r, want_dlogits)
    e = assert_close(f"{name}/loss", loss.numpy(), [r["r64"]["loss"]], TOL, rel_floor=1.0)
    print(f"{name}: loss {float(loss):.7g} ref {r['r64']['loss']:.7g} rel err {e:.3g}")
    check_tensors(f"{name}/grad", got, r["r64"]["grads"], r)
    return loss, dl, got


@gpu
@pytest.mark.parametrize("case", GRID + EDGES + SINGLE, ids=id_of)
def test_forward_and_gradients_match_float64(case):
    r = reference(case)
    name = name_of(case)
    guard(name, r)
    net = make_net(*case[:3], r["W"])
    check_forward(name, net, r)
    check_gradients(name, net, r)


@gpu
def test_three_hundred_leaves_after_twelve():
    """B = 300 on a net whose descriptor and workspace were sized by a B = 12 call: grad_ws raises
    max_B and reallocates, and every weight gradient sums 300 leaves serially."""
    S, E, L, _ = MANY
    big = reference(MANY)
    guard(name_of(MANY), big)
    W = big["W"]
    small = reference((S, E, L, 12), W=W)               # the B = 12 leaves on the same weights
    net = make_net(S, E, L, W)
    check_gradients(name_of(MANY) + "/first12", net, small)
    assert net.desc.max_B == 12
    check_forward(name_of(MANY), net, big)
    check_gradients(name_of(MANY), net, big)
    assert net.desc.max_B == 300
    check_gradients(name_of(MANY) + "/again12", net, small)        # the larger workspace, B = 12


@gpu
@pytest.mark.parametrize("E,L", EL)
def test_saturated_value_and_clamped_policy(E, L):
    """S = 16.  value_head.weight is scaled until the float64 value pre-activation of one leaf has
    |u| > 8 (1 - tanh^2 u < 5e-7: 1 - v * v in fp32 would keep one or two digits); policy_head.bias
    of action 2 is set so low that its float64 pi is below 1e-8 on row 3, whose target puts 0.5
    there and nowhere else in the batch: the clamp passes nothing, so dloss / dlogit of that
    action is below 1e-8 in magnitude (log-softmax would give about -0.5 / B)."""
    S, B, a, row = 16, 12, 2, 3
    base = reference((S, E, L, B))
    W = {k: v.copy() for k, v in base["W"].items()}
    u = base["r64"]["u"]
    W["value_head.weight"] *= np.float32(9.0 / np.abs(u - W["value_head.bias"][0]).max())
    W["policy_head.bias"][a] = -40.0
    tpi = base["tpi"].copy()
    tpi[:, a] = 0.0
    tpi /= tpi.sum(1, keepdims=True)
    tpi[row] *= 0.5
    tpi[row, a] = 0.5
    r = reference((S, E, L, B), W=W, tpi=tpi.astype(np.float32))
    name = f"fl_shapes/S{S}_E{E}_L{L}_B{B}/edges"
    guard(name, r)
    assert np.abs(r["r64"]["u"]).max() > 8
    assert r["r64"]["pi"][row, a] < 1e-8 and r["tpi"][row, a] == 0.5
    assert abs(r["r64"]["dlogits"][row, a]) < 1e-8
    net = make_net(S, E, L, W)
    check_forward(name, net, r)
    _, dl, _ = check_gradients(name, net, r, want_dlogits=True)
    assert abs(dl[row, a].item()) < 1e-8 < 0.4 / B
    assert_close(f"{name}/dlogits", dl.cpu().numpy(), r["r64"]["dlogits"], TOL)


@gpu
def test_determinism_and_row_independence():
    """(S 25, E 64, L 4): a second az_fl_grads call gives equal bits, and every row of the B = 12
    evaluation equals that leaf's own B = 1 call bit for bit."""
    case = (25, 64, 4, 12)
    r = reference(case)
    net = make_net(*case[:3], r["W"])
    loss, dl, got = gradients(net, r, want_dlogits=True)
    loss2, dl2, got2 = gradients(net, r, want_dlogits=True)
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2)
    for k in got:
        assert not np.isnan(got[k]).any() and np.array_equal(got[k], got2[k]), k
    pi, v = evaluate(net, r["nodes"], r["counts"])
    for b in range(case[3]):
        p1, v1 = evaluate(net, r["nodes"][b:b + 1], r["counts"][b:b + 1])
        assert torch.equal(p1[0], pi[b]) and torch.equal(v1[0], v[b]), b


@gpu
@pytest.mark.parametrize("S,E", [(25, 64), (16, 128)])
def test_clip_over_sixteen_buffers(S, E):
    """L = 4: the per-tensor views are 16 buffers, exactly CLIP_MAX_BUFS.  The value targets are
    pushed to -3 sign(v) so that the float64 norm exceeds 1 and the clip scales; the norm within
    1e-5 relative, the post-clip tensors at the gradient bars, and the flat buffer in one piece
    gives the same norm."""
    from azhip.frozenlake import clip_grad_norm, fl_grads
    case = (S, E, 4, 12)
    base = reference(case)
    r = dict(base)
    r["tv"] = (-3.0 * np.sign(base["r64"]["v"])).astype(np.float32)
    r["r64"] = fl_ref.grads(r["W"], r["nodes"], r["counts"], r["tpi"], r["tv"], torch.float64)
    r["r32"] = fl_ref.grads(r["W"], r["nodes"], r["counts"], r["tpi"], r["tv"], torch.float32)
    r["bars"], r["widened"] = fl_ref.bars(r["r64"]["grads"], r["r32"]["grads"])
    name = name_of(case) + "/clip"
    guard(name, r)
    norm64, post64 = fl_ref.clip(r["r64"]["grads"], 1.0)
    assert norm64 > 1.0, norm64
    net = make_net(*case[:3], r["W"])
    args = [dev(net, r[k]) for k in ("nodes", "counts", "tpi", "tv")]
    net.params.grad_flat.zero_()                      # (the flat buffer's alignment gaps stay 0)
    fl_grads(net, *args)
    views = list(net.params.grads.values())
    assert len(views) == 16
    norm = clip_grad_norm(views, 1.0)
    torch.cuda.synchronize()
    e = assert_close(f"{name}/norm", norm.cpu().numpy() / norm64, [1.0], TOL)
    print(f"{name}: norm {norm.item():.7g} ref {norm64:.7g} rel err {e:.3g}")
    check_tensors(f"{name}/post", {k: g.cpu().numpy() for k, g in net.params.grads.items()},
                  post64, r)
    fl_grads(net, *args)
    flat = clip_grad_norm([net.params.grad_flat], 1.0)
    torch.cuda.synchronize()
    assert_close(f"{name}/norm_flat", flat.cpu().numpy() / norm64, [1.0], TOL)
    assert abs(flat.item() - norm.item()) <= 1e-6 * norm64


# ------------------------------------------------------------------------------------ wrapper
class Args(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def one_hot_states(n):
    out = []
    for cell in range(n * n):
        b = np.zeros((n, n))
        b[cell // n, cell % n] = 1
        out.append(b)
    return out + [np.zeros((n, n))]


@gpu
@pytest.mark.parametrize("tag,E,L", [("c5", 128, 4), ("m4", 128, 1)])
def test_table_and_train_on_other_shapes(tag, E, L, monkeypatch):
    """The 5x5 custom map of fl_rules.npz with (E 128, L 4) and the 4x4 map with (E 128, L 1)
    through the wrapper: the whole-board table and the per-call route agree bit for bit; train()
    for 2 epochs on 20 examples moves every tensor; a second run from the same start and seed
    gives equal bits; predict on every state afterwards is within 1e-5 of the float64 restatement
    on the trained weights."""
    from frozenlake.FrozenLakeGame import FrozenLakeGame
    from frozenlake.FrozenLakeNet import FrozenLakeNet
    rows = [str(s) for s in golden("fl_rules.npz")[f"{tag}_map"]]
    game = FrozenLakeGame(custom_map=rows)
    n = len(rows)
    S = n * n
    assert S == (25 if tag == "c5" else 16)
    W = weights(S, E, L, seed_of(S, E, L, 20))
    w = FrozenLakeNet(game, Args(lr=1e-3, dropout=0.3, epochs=2, batch_size=8, embedding_dim=E,
                                 gnn_layers=L))
    w.nnet.load_state_dict(W)
    w._weights_changed()
    states = one_hot_states(n)

    def routes():
        monkeypatch.setenv("AZ_FL_TABLE", "1")
        calls = w.eval_calls
        table = [w.predict(b) for b in states]
        assert w.eval_calls == calls + 1            # one evaluator call filled the table
        monkeypatch.setenv("AZ_FL_TABLE", "0")
        direct = [w.predict(b) for b in states]
        assert w.eval_calls == calls + 1 + len(states)
        for (p0, v0), (p1, v1) in zip(table, direct):
            assert p0.shape == (4,) and v0.shape == (1,) and p0.dtype == v0.dtype == np.float32
            assert np.array_equal(p0, p1) and np.array_equal(v0, v1)
        return np.array([p for p, _ in table]), np.array([v[0] for _, v in table])

    def float64_of(weights_now):
        lists = [w._node_list(b) for b in states]
        nodes = np.full((len(lists), 5, S), np.nan, np.float32)
        counts = np.array([len(nl) for nl in lists], np.int32)
        for i, nl in enumerate(lists):
            nodes[i, :len(nl)] = np.asarray(nl, np.float32).reshape(len(nl), S)
        with torch.no_grad():
            pi, v, _ = fl_ref.forward(fl_ref.params(weights_now), nodes, counts)
        return pi.numpy(), v.numpy()

    name = f"fl_shapes/{tag}_E{E}_L{L}"
    pi0, v0 = routes()
    rpi, rv = float64_of(W)
    assert_close(f"{name}/start/pi", pi0, rpi, TOL)
    assert_close(f"{name}/start/v", v0, rv, TOL)
    rng = np.random.default_rng(seed_of(S, E, L, 21))
    cells = rng.integers(0, S + 1, 20)
    tpi, tv = targets(20, 4, seed_of(S, E, L, 22))
    examples = [(states[c], tpi[i].astype(np.float64), float(tv[i])) for i, c in enumerate(cells)]
    np.random.seed(31)
    w.train(list(examples))
    first = {k: t.numpy() for k, t in w.nnet.params.cpu_state_dict().items()}
    for k, t in first.items():
        assert np.isfinite(t).all() and np.abs(t - W[k]).max() > 0, k        # it did move
    pi1, v1 = routes()
    assert not np.array_equal(pi0, pi1)
    rpi, rv = float64_of(first)
    e_pi = assert_close(f"{name}/trained/pi", pi1, rpi, TOL)
    e_v = assert_close(f"{name}/trained/v", v1, rv, TOL)
    print(f"{name}: after train() pi max err {e_pi:.3g}, v max err {e_v:.3g}")
    w.nnet.load_state_dict(W)
    w._weights_changed()
    np.random.seed(31)
    w.train(list(examples))
    for k, t in w.nnet.params.cpu_state_dict().items():
        assert np.array_equal(t.numpy(), first[k]), k
