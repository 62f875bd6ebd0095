"""Generates the FrozenLake fixtures from the reference implementation (run once, on a machine
that has the reference tree; the tests only read the files it writes).

    python tests/golden/make_frozenlake_goldens.py path/to/reference

The reference's game imports gymnasium only for the map, so a stand-in module with the two
standard maps is put into sys.modules['gymnasium'] before the import; its transitions, network,
MCTS, Arena and Coach run unchanged, with torch only.

Files (each under 1 MB):
  fl_rules.npz             every rule answer for the 4x4 map, the 8x8 map and a 5x5 custom map
  fl_net_{4,8}.npz         weights, predict of every state and of 8 free-form boards, from the
                           fp32 module and from the module cast to float64 with an exact 1/n
                           adjacency
  fl_grad_{4,8}.npz        one training batch: loss, pre-clip gradients, clip norm, per-tensor bars
  fl_grad_{4,8}_clip.npz   the post-clip gradients of that batch
                           (gradient tensors of the float64 module are stored rounded to float32,
                           a 6e-8 relative change against bars of 1e-5, to stay under the size limit)
  fl_train_4.npz, fl_train_8x8_e64.npz   weights after train(), fp32 and float64
  fl_mcts.json / .npz      reference MCTS searches over recorded predictions
  fl_arena.json            single-player Arena results of scripted players
  fl_episode.json          two Coach.executeEpisode runs over recorded predictions
"""
import copy
import json
import os
import sys
import types
from collections import deque

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]

MAP4 = ["SFFF", "FHFH", "FFFH", "HFFG"]
MAP8 = ["SFFFFFFF", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF", "FFFHFFFF", "FHHFFFHF", "FHFFHFHF",
        "FFFHFFFG"]
MAP5 = ["SHFFF", "FFFHF", "FFFFF", "HFFFH", "FFFFG"]      # custom: a hole next to S


def install_gymnasium_stand_in():
    gym = types.ModuleType("gymnasium")

    class _Env:
        def __init__(self, desc):
            self.unwrapped = types.SimpleNamespace(desc=np.asarray([list(r) for r in desc],
                                                                   dtype="c"), s=0)

        def reset(self):
            return 0, {}

        def render(self):
            return None

    def make(id, desc=None, is_slippery=False, render_mode=None):
        if desc is None:
            desc = MAP8 if "8x8" in id else MAP4
        return _Env(desc)

    gym.make = make
    sys.modules["gymnasium"] = gym


install_gymnasium_stand_in()
sys.path.insert(0, REF)
from Arena import Arena  # noqa: E402
from Coach import Coach  # noqa: E402
from MCTS import MCTS  # noqa: E402
from frozenlake.FrozenLakeGame import FrozenLakeGame  # noqa: E402
from frozenlake.FrozenLakeNet import FrozenLakeNet  # noqa: E402


class Args(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def all_states(game):
    n = game.map_size
    out = []
    for cell in range(n * n):
        b = np.zeros((n, n))
        b[cell // n, cell % n] = 1
        out.append(b)
    out.append(np.zeros((n, n)))
    return out


def node_list(game, board):
    nodes = [board]
    valids = game.getValidMoves(board, 1)
    for a in range(4):
        if valids[a]:
            nodes.append(game.getNextState(board, 1, a)[0])
    return nodes


# ------------------------------------------------------------------------------------ rules
def make_rules():
    out = {}
    for tag, kw in (("m4", dict(map_size=4)), ("m8", dict(map_size=8)),
                    ("c5", dict(map_size=4, custom_map=MAP5))):
        g = FrozenLakeGame(**kw)
        n = g.map_size
        states = all_states(g)
        out[f"{tag}_map"] = np.array(["".join(x.decode() for x in row) for row in g.desc])
        out[f"{tag}_goal"] = np.array(g.goal_pos)
        out[f"{tag}_init"] = g.getInitBoard()
        out[f"{tag}_valid"] = np.array([g.getValidMoves(b, 1) for b in states], np.int8)
        out[f"{tag}_next"] = np.array([[g.getNextState(b, 1, a)[0] for a in range(4)]
                                       for b in states])
        out[f"{tag}_ended"] = np.array([float(g.getGameEnded(b, 1)) for b in states])
        out[f"{tag}_str"] = np.array([g.stringRepresentation(b) for b in states])
        assert out[f"{tag}_next"].shape == (n * n + 1, 4, n, n)
    np.savez_compressed(os.path.join(HERE, "fl_rules.npz"), **out)


# ------------------------------------------------------------------------------------ network
def make_net(game, E, L, seed, scale=3.0, bias_std=0.1, lr=1e-3, epochs=2, batch_size=8):
    args = Args(lr=lr, dropout=0.3, epochs=epochs, batch_size=batch_size, embedding_dim=E,
                gnn_layers=L)
    torch.manual_seed(seed)
    net = FrozenLakeNet(game, args)
    net.nnet.cpu()
    net.device = torch.device("cpu")
    if scale != 1.0 or bias_std:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for k, p in net.nnet.state_dict().items():
                if k.endswith("weight"):
                    p.mul_(scale)
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * bias_std)
    return net


def forward(nnet, net, nodes, dtype):
    """The module's forward for one node list, fp32 (the reference's own adjacency) or float64
    (exact 1/n adjacency)."""
    x = torch.tensor(np.array(nodes), dtype=dtype)
    n = x.shape[0]
    if dtype == torch.float64:
        adj = torch.full((n, n), 1.0 / n, dtype=dtype)
    else:
        adj = net.create_adjacency(n)
    return nnet(x[:1], x, adj.unsqueeze(0))


def loss_of(nnet, net, node_lists, tpi, tv, dtype):
    outs = [forward(nnet, net, nl, dtype) for nl in node_lists]
    out_pi = torch.cat([o[0] for o in outs], dim=0)
    out_v = torch.cat([o[1] for o in outs], dim=0)
    tpi = torch.tensor(tpi, dtype=dtype)
    tv = torch.tensor(tv, dtype=dtype)
    pi_loss = -torch.mean(torch.sum(tpi * torch.log(out_pi.clamp(min=1e-8)), dim=1))
    return pi_loss + torch.nn.functional.mse_loss(out_v.view(-1), tv), out_pi


def weights_of(nnet):
    return {k: v.detach().cpu().numpy().copy() for k, v in nnet.state_dict().items()}


def make_net_fixture(tag, map_size, E, L, seed, nbatch):
    game = FrozenLakeGame(map_size=map_size)
    n, S = game.map_size, game.map_size ** 2
    net = make_net(game, E, L, seed)
    net64 = copy.deepcopy(net.nnet).double()
    net.nnet.eval()
    net64.eval()
    out = {f"w.{k}": v for k, v in weights_of(net.nnet).items()}
    states = all_states(game)
    p32, v32, p64, v64 = [], [], [], []
    for b in states:
        pi, v = net.predict(b)
        p32.append(pi), v32.append(v[0])
        with torch.no_grad():
            pi, v = forward(net64, net, node_list(game, b), torch.float64)
        p64.append(pi[0].numpy()), v64.append(v[0, 0].item())
    out.update(pi32=np.array(p32), v32=np.array(v32), pi64=np.array(p64), v64=np.array(v64))
    # free-form boards with explicit node lists of 1..5 rows
    rng = np.random.RandomState(seed + 2)
    counts = np.array([1, 2, 3, 4, 5, 5, 3, 2], np.int32)
    free = np.zeros((8, 5, S), np.float32)
    f32p, f32v, f64p, f64v = [], [], [], []
    for i, k in enumerate(counts):
        free[i, :k] = rng.uniform(-1.0, 1.5, (k, S)).astype(np.float32)
        nodes = [free[i, j].reshape(n, n) for j in range(k)]
        pi, v = net.predict(nodes[0], neighbor_states=nodes)
        f32p.append(pi), f32v.append(v[0])
        with torch.no_grad():
            pi, v = forward(net64, net, nodes, torch.float64)
        f64p.append(pi[0].numpy()), f64v.append(v[0, 0].item())
    out.update(free_nodes=free, free_counts=counts, free_pi32=np.array(f32p),
               free_v32=np.array(f32v), free_pi64=np.array(f64p), free_v64=np.array(f64v))
    np.savez_compressed(os.path.join(HERE, f"fl_net_{tag}.npz"), **out)

    # ---- the gradient batch: the same weights with one policy bias pushed down, so that action
    # 3 has pi < 1e-8 everywhere and the clamp of the loss is live
    with torch.no_grad():
        net.nnet.policy_head.bias[3] -= 30.0
    net64 = copy.deepcopy(net.nnet).double()
    net.nnet.train()
    net64.train()
    holes = [c for c in range(S) if game.desc[c // n][c % n] == b"H"]
    goal = game.goal_pos[0] * n + game.goal_pos[1]
    inside = [c for c in range(S) if 0 < c // n < n - 1 and 0 < c % n < n - 1
              and c not in holes]
    edge = [c for c in range(1, n - 1)]
    forced = [holes[0], goal, 0, edge[0], inside[0], S]          # 1, 1, 3, 4, 5, 5 (empty) nodes
    cells = forced + [int(c) for c in rng.randint(0, S, nbatch - len(forced))]
    boards = np.array([states[c] for c in cells], np.float32)
    node_lists = [node_list(game, b) for b in boards]
    gcounts = np.array([len(nl) for nl in node_lists], np.int32)
    assert {1, 3, 4, 5} <= set(gcounts.tolist()), gcounts
    tpi = rng.dirichlet(np.ones(4), nbatch).astype(np.float32)
    tv = rng.choice([-1.0, 1.0], nbatch).astype(np.float32)
    clamp_rows = [2, 4]
    for r in clamp_rows:
        rest = rng.dirichlet(np.ones(3)).astype(np.float32) * 0.5
        tpi[r] = [rest[0], rest[1], rest[2], 0.5]
    gnodes = np.zeros((nbatch, 5, S), np.float32)
    for i, nl in enumerate(node_lists):
        gnodes[i, :len(nl)] = np.array(nl, np.float32).reshape(len(nl), S)
    res = {}
    for name, mod, dt in (("32", net.nnet, torch.float32), ("64", net64, torch.float64)):
        mod.zero_grad()
        loss, out_pi = loss_of(mod, net, node_lists, tpi, tv, dt)
        for r in clamp_rows:
            assert out_pi[r, 3].item() < 1e-8, (name, r, out_pi[r])
        loss.backward()
        pre = {k: p.grad.detach().numpy().copy() for k, p in mod.named_parameters()}
        norm = torch.nn.utils.clip_grad_norm_(mod.parameters(), max_norm=1.0)
        post = {k: p.grad.detach().numpy().copy() for k, p in mod.named_parameters()}
        res[name] = (loss.item(), pre, float(norm), post)
    # the fp32 path above against the reference's own train(): one epoch, one batch, no shuffle
    check_against_train(game, net, boards, tpi, tv, res["32"][3], nbatch)
    grad = dict(boards=boards, nodes=gnodes, counts=gcounts, tpi=tpi, tv=tv,
                clamp_rows=np.array(clamp_rows), clamp_action=np.array(3),
                policy_bias=net.nnet.policy_head.bias.detach().numpy().copy(),
                loss32=np.float32(res["32"][0]), loss64=np.float64(res["64"][0]),
                norm32=np.float32(res["32"][2]), norm64=np.float64(res["64"][2]))
    clip = {}
    widened = []
    for k in res["64"][1]:
        g32, g64 = res["32"][1][k], res["64"][1][k]
        top = float(np.abs(g64).max())
        rel = float(np.abs(g32 - g64).max()) / top if top > 0 else 0.0
        bar = 1e-5
        if rel > 2.5e-6:
            bar = 4 * rel
            widened.append((k, rel))
        grad[f"bar.{k}"] = np.float64(bar)
        grad[f"pre32.{k}"] = g32
        grad[f"pre64.{k}"] = g64.astype(np.float32)
        clip[f"post32.{k}"] = res["32"][3][k]
        clip[f"post64.{k}"] = res["64"][3][k].astype(np.float32)
    print(f"fl_grad_{tag}: loss {res['32'][0]:.6f} / {res['64'][0]:.6f}, norm {res['32'][2]:.4f}"
          f", tensors with a widened bar: {widened}")
    np.savez_compressed(os.path.join(HERE, f"fl_grad_{tag}.npz"), **grad)
    np.savez_compressed(os.path.join(HERE, f"fl_grad_{tag}_clip.npz"), **clip)
    return net


def check_against_train(game, net, boards, tpi, tv, post32, nbatch):
    """The reference's train() on the same batch (hooked at optimizer.step) must hold the same
    post-clip gradients as loss_of + backward + clip_grad_norm_ above."""
    ref = copy.deepcopy(net)
    ref.nnet = copy.deepcopy(net.nnet)
    ref.args = Args(ref.args, epochs=1, batch_size=nbatch)
    seen = {}
    orig_step, orig_shuffle = torch.optim.Adam.step, np.random.shuffle

    def step(self, *a, **k):
        seen.update({n: p.grad.detach().numpy().copy() for n, p in ref.nnet.named_parameters()})

    torch.optim.Adam.step = step
    np.random.shuffle = lambda x: None
    try:
        ref.train([(b, p, v) for b, p, v in zip(boards, tpi, tv)])
    finally:
        torch.optim.Adam.step, np.random.shuffle = orig_step, orig_shuffle
    for k, g in post32.items():
        assert np.array_equal(seen[k], g), k


# ------------------------------------------------------------------------------------ training
def train64(game, net, nnet64, examples, args):
    """FrozenLakeNet.train with the module in float64 and the exact 1/n adjacency (the same RNG
    use: one np.random.shuffle per epoch)."""
    nnet64.train()
    opt = torch.optim.Adam(nnet64.parameters(), lr=args.lr)
    examples = [(x[0], x[1], x[2]) for x in examples if x[2] is not None]
    for _ in range(args.epochs):
        np.random.shuffle(examples)
        bs = min(len(examples), args.batch_size)
        for i in range(0, len(examples), bs):
            boards, pis, vs = list(zip(*examples[i:i + bs]))
            nls = [node_list(game, np.asarray(b, np.float32)) for b in boards]
            opt.zero_grad()
            loss, _ = loss_of(nnet64, net, nls, np.array(pis, np.float32),
                              np.array(vs, np.float64).astype(np.float32), torch.float64)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(nnet64.parameters(), max_norm=1.0)
            opt.step()


def make_train_fixture(name, map_size, E, L, seed, nex, np_seed):
    game = FrozenLakeGame(map_size=map_size)
    n, S = game.map_size, game.map_size ** 2
    net = make_net(game, E, L, seed, scale=1.0, bias_std=0.0, lr=1e-3, epochs=2, batch_size=8)
    args = net.args
    nnet64 = copy.deepcopy(net.nnet).double()
    start = weights_of(net.nnet)
    rng = np.random.RandomState(seed + 3)
    live = [c for c in range(S) if game.desc[c // n][c % n] in (b"S", b"F")]
    states = all_states(game)
    boards = [states[c] for c in rng.choice(live, nex)]
    pis = [list(map(float, p)) for p in rng.dirichlet(np.ones(4), nex)]
    vs = [float(v) for v in rng.choice([-1.0, 1.0], nex)]
    examples = [(b, p, v) for b, p, v in zip(boards, pis, vs)]
    np.random.seed(np_seed)
    net.train(list(examples))
    np.random.seed(np_seed)
    train64(game, net, nnet64, list(examples), args)
    after32, after64 = weights_of(net.nnet), weights_of(nnet64)
    spread = max(float(np.abs(after32[k] - after64[k]).max()) for k in start)
    travel = max(float(np.abs(after64[k] - start[k]).max()) for k in start)
    print(f"{name}: fp32-vs-float64 spread {spread:.3g}, weight travel {travel:.3g}")
    assert spread <= 5e-6, spread
    out = dict(boards=np.array(boards), pis=np.array(pis), vs=np.array(vs),
               np_seed=np.array(np_seed), lr=np.array(args.lr), epochs=np.array(args.epochs),
               batch_size=np.array(args.batch_size), E=np.array(E), L=np.array(L),
               map_size=np.array(map_size), spread=np.array(spread))
    for k in start:
        out[f"start.{k}"] = start[k]
        out[f"after32.{k}"] = after32[k]
        out[f"after64.{k}"] = after64[k]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


# ------------------------------------------------------------------------------------ search
class RecordedNet:
    """A table of predictions looked up by state (guided_table)."""

    def __init__(self, game, pi, v):
        self.game, self.pi, self.v = game, pi, v
        self.S = game.map_size ** 2

    def predict(self, board):
        i = self.S if np.sum(board) == 0 else int(np.argmax(board))
        return self.pi[i].copy(), self.v[i:i + 1].copy()


def guided_table(game, seed):
    """Recorded predictions for the search fixtures: priors that lean towards the shortest way
    to the goal, with seeded noise, and noisy values.  (The reference's search recurses without
    end when a descent returns to a state it already passed, which priors of an untrained net
    soon cause on this map; these make every recorded search finish.)"""
    n, S = game.map_size, game.map_size ** 2
    rng = np.random.RandomState(seed)
    dist = {game.goal_pos: 0}
    queue = deque([game.goal_pos])
    moves = [(-1, 0), (0, 1), (1, 0), (0, -1)]
    while queue:
        r, c = queue.popleft()
        for dr, dc in moves:
            q = (r - dr, c - dc)
            if 0 <= q[0] < n and 0 <= q[1] < n and q not in dist and game.desc[q[0]][q[1]] != b"H":
                dist[q] = dist[(r, c)] + 1
                queue.append(q)
    pi = np.zeros((S + 1, 4), np.float32)
    v = np.zeros((S + 1,), np.float32)
    for cell in range(S + 1):
        logits = rng.normal(0, 0.5, 4)
        if cell < S:
            r, c = cell // n, cell % n
            for a, (dr, dc) in enumerate(moves):
                q = (r + dr, c + dc)
                if q in dist and dist[q] < dist.get((r, c), 99):
                    logits[a] += 2.0
        e = np.exp(logits - logits.max())
        pi[cell] = (e / e.sum()).astype(np.float32)
        v[cell] = np.float32(np.tanh(rng.normal(0, 0.5)))
    return pi, v


def make_mcts():
    game = FrozenLakeGame(map_size=4)
    args = Args(numMCTSSims=25, cpuct=2.0)
    states = all_states(game)
    for seed in range(100):
        pi, v = guided_table(game, seed)
        rec = RecordedNet(game, pi, v)
        runs = []
        try:
            for start in (0, 16, 9):             # the start cell, the empty board, cell (2,1)
                board = states[start]
                s = game.stringRepresentation(board)
                m = MCTS(game, rec, args)
                probs = m.getActionProb(board, temp=1)
                np.random.seed(7)
                m0 = MCTS(game, rec, args)
                probs0 = m0.getActionProb(board, temp=0)
                runs.append(dict(
                    start=start, counts=[int(m.Nsa.get((s, a), 0)) for a in range(4)],
                    probs=[float(x) for x in probs],
                    q=[float(np.asarray(m.Qsa[(s, a)]).reshape(-1)[0]) if (s, a) in m.Qsa
                       else None for a in range(4)],
                    n_nodes=len(m.Ns), nsa_total=int(sum(m.Nsa.values())),
                    seed0=7, probs0=[int(x) for x in probs0]))
            make_episodes(rec)
        except (RecursionError, AssertionError) as e:
            print(f"fl_mcts: table seed {seed} rejected ({type(e).__name__})")
            continue
        break
    else:
        raise AssertionError("no prediction table lets the reference's searches finish")
    json.dump(dict(args=dict(args), table_seed=seed, runs=runs),
              open(os.path.join(HERE, "fl_mcts.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "fl_mcts.npz"), pi=pi, v=v)


class _TooLong(BaseException):
    pass


def make_episodes(rec):
    game = FrozenLakeGame(map_size=4)
    args = Args(numMCTSSims=10, cpuct=2.0, tempThreshold=15)
    found = {}
    orig = np.random.choice
    for seed in range(200):
        moves = [0]

        def choice(*a, **k):
            moves[0] += 1
            if moves[0] > 200:
                raise _TooLong()
            return orig(*a, **k)

        coach = Coach.__new__(Coach)
        coach.game, coach.args, coach.nnet = game, args, rec
        coach.mcts = MCTS(game, rec, args)
        np.random.seed(seed)
        np.random.choice = choice
        try:
            std, _ = coach.executeEpisode()
        except (_TooLong, RecursionError):
            continue
        finally:
            np.random.choice = orig
        if len(std) > 64:
            continue
        kind = "goal" if std[0][2] > 0 else "hole"
        if kind not in found:
            found[kind] = dict(seed=seed, kind=kind,
                               boards=[np.asarray(b).astype(int).tolist() for b, _, _ in std],
                               pis=[[float(x) for x in p] for _, p, _ in std],
                               rewards=[float(r) for _, _, r in std])
        if len(found) == 2:
            break
    assert len(found) == 2, found.keys()
    json.dump(dict(args=dict(args), episodes=[found["goal"], found["hole"]]),
              open(os.path.join(HERE, "fl_episode.json"), "w"), indent=1)


# ------------------------------------------------------------------------------------ arena
class ScriptPlayer:
    """Plays a fixed action sequence, cyclically; startGame rewinds it."""

    def __init__(self, actions):
        self.actions, self.i = actions, 0

    def startGame(self):
        self.i = 0

    def __call__(self, board):
        a = self.actions[self.i % len(self.actions)]
        self.i += 1
        return a


def bfs(game, want):
    """Shortest action sequence from the start to a cell where want(cell letter)."""
    n = game.map_size
    start = tuple(int(i) for i in np.argwhere(game.getInitBoard() == 1)[0])
    seen, queue = {start: []}, deque([start])
    while queue:
        r, c = queue.popleft()
        if want(game.desc[r][c]):
            return seen[(r, c)]
        if game.desc[r][c] in (b"H", b"G"):
            continue
        for a, (dr, dc) in enumerate([(-1, 0), (0, 1), (1, 0), (0, -1)]):
            nr, nc = r + dr, c + dc
            if 0 <= nr < n and 0 <= nc < n and (nr, nc) not in seen:
                seen[(nr, nc)] = seen[(r, c)] + [a]
                queue.append((nr, nc))
    raise AssertionError("unreachable")


def make_arena():
    out = {}
    for size in (4, 8):
        game = FrozenLakeGame(map_size=size)
        scripts = dict(path=bfs(game, lambda x: x == b"G"), hole=bfs(game, lambda x: x == b"H"),
                       bounce=[1, 3], invalid=[0])
        names = list(scripts)
        singles, pairs = {}, {}
        for k in names:
            np.random.seed(11)
            arena = Arena(ScriptPlayer(scripts[k]), ScriptPlayer(scripts[k]), game)
            r, steps = arena.playGameForSinglePlayer(arena.player1)
            np.random.seed(11)
            singles[k] = dict(result=float(r), steps=int(steps), seed=11,
                              play_game=float(arena.playGame()))
        for a in names:
            for b in names:
                np.random.seed(13)
                arena = Arena(ScriptPlayer(scripts[a]), ScriptPlayer(scripts[b]), game)
                pairs[f"{a}:{b}"] = dict(seed=13, num=6,
                                         triple=[int(x) for x in
                                                 arena.playGamesForSinglePlayer(6)])
        out[str(size)] = dict(scripts=scripts, singles=singles, pairs=pairs)
    json.dump(out, open(os.path.join(HERE, "fl_arena.json"), "w"), indent=1)


if __name__ == "__main__":
    import logging
    logging.disable(logging.CRITICAL)
    make_rules()
    make_net_fixture("4", 4, 64, 2, seed=100, nbatch=16)
    make_net_fixture("8", 8, 128, 3, seed=200, nbatch=24)
    make_train_fixture("fl_train_4", 4, 64, 2, seed=300, nex=20, np_seed=5)
    make_train_fixture("fl_train_8x8_e64", 8, 64, 2, seed=400, nex=24, np_seed=6)
    make_mcts()
    make_arena()
    for f in sorted(os.listdir(HERE)):
        if f.startswith("fl_"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < (1 << 20), (f, size)
            print(f"{f}: {size} bytes")
