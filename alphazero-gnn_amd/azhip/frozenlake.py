"""FrozenLakeNet on libaz_hip (reference frozenlake/FrozenLakeNet.py:36-335): same constructor
(game, args), predict / train / save_checkpoint / load_checkpoint and state_dict keys, plus
batched entry points for lock-step self-play.

A leaf is the board and the next state of every valid action (1 to 5 node boards); the whole
evaluation of a batch of leaves is ONE az_fl_eval_fwd launch whose rows do not depend on the
batch.  A game has at most 65 distinct states (S one-hot boards and the empty board), so after
any weight change all of them are evaluated in one call and `predict` of such a board is a host
lookup; the two routes return the same bits.  AZ_FL_TABLE=0 turns the table off."""
import ctypes
import os

import numpy as np
import torch

import nn_fallback

from . import _lib, nets, ops, train as T
from .params import FlatParams

MAX_NODES, HIDDEN, ACTIONS = 5, 128, 4


def frozenlake_net_spec(S, E=64, L=2, A=ACTIONS):
    """(name, shape) in the reference's state_dict order (FrozenLakeNet.py:266-284)."""
    spec = [("feature_extractor.0.weight", (HIDDEN, S)), ("feature_extractor.0.bias", (HIDDEN,)),
            ("feature_extractor.2.weight", (E, HIDDEN)), ("feature_extractor.2.bias", (E,))]
    for i in range(L):
        spec += [(f"gnn_layers.{i}.W.weight", (E, E)), (f"gnn_layers.{i}.W.bias", (E,))]
    return spec + [("policy_head.weight", (A, E)), ("policy_head.bias", (A,)),
                   ("value_head.weight", (1, E)), ("value_head.bias", (1,))]


def _fl_params(views, L):
    """_lib.FlParams over a dict of tensors keyed like the state_dict."""
    P = lambda k: views[k].data_ptr()  # noqa: E731
    p = _lib.FlParams()
    p.fe0_w, p.fe0_b = P("feature_extractor.0.weight"), P("feature_extractor.0.bias")
    p.fe2_w, p.fe2_b = P("feature_extractor.2.weight"), P("feature_extractor.2.bias")
    for i in range(L):
        p.gnn_w[i] = P(f"gnn_layers.{i}.W.weight")
        p.gnn_b[i] = P(f"gnn_layers.{i}.W.bias")
    p.policy_w, p.policy_b = P("policy_head.weight"), P("policy_head.bias")
    p.value_w, p.value_b = P("value_head.weight"), P("value_head.bias")
    return p


class EnhancedNNet(nets._Net):
    """FrozenLakeNet.py:253-295: parameters in one flat HBM buffer, Xavier-normal weights and
    zero biases; the forward and backward passes are az_fl_eval_fwd / az_fl_grads."""

    def __init__(self, board_size, action_size, args, device=None):
        self.board_x, self.board_y = board_size
        self.action_size = action_size
        self.S = self.board_x * self.board_y
        self.E = int(nets._args_get(args, "embedding_dim", 64))
        self.L = int(nets._args_get(args, "gnn_layers", 2))
        if not 4 <= self.S <= 64 or self.E not in (64, 128) or not 1 <= self.L <= 4 \
                or action_size != ACTIONS:
            raise ValueError(f"FrozenLakeNet: unsupported shape S={self.S} embedding_dim={self.E} "
                             f"gnn_layers={self.L} actions={action_size} (S in 4..64, "
                             "embedding_dim 64 or 128, gnn_layers 1..4, 4 actions)")
        self.device = device or nets.default_device()
        spec = frozenlake_net_spec(self.S, self.E, self.L)
        init = {}
        for name, shape in spec:
            t = torch.zeros(shape)
            if name.endswith("weight"):
                torch.nn.init.xavier_normal_(t)
            init[name] = t
        self.params = FlatParams(spec, self.device, init=init)
        self.training = False
        self.desc = _lib.FlEval(self.S, self.E, self.L, ACTIONS, HIDDEN, 1,
                                _fl_params(self.params.views, self.L))
        self._ws = None

    def grad_ws(self, B):
        """The workspace az_fl_grads needs for B leaves.  The library sizes its check by the
        descriptor's max_B, which evaluator calls raise too (a table fill carries S+1 leaves), so
        the buffer is measured against the capacity as it stands now, not the one it was made
        for."""
        self.desc.max_B = max(B, self.desc.max_B)
        need = int(_lib.lib().az_fl_eval_ws_bytes(self.desc.max_B, self.S, self.E, self.L))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return self._ws


def fl_eval_fwd(net, nodes, counts, pi, v, B, stream=None):
    """az_fl_eval_fwd on tensors (device, or HostBuffer views): nodes f32 [B][5][S], counts i32
    [B] -> pi [B][4], v [B]."""
    net.params.sync()
    net.desc.max_B = max(net.desc.max_B, B)
    s = stream if stream is not None else torch.cuda.current_stream(net.device)
    _lib.check(_lib.lib().az_fl_eval_fwd(ctypes.byref(net.desc), ops._p(nodes), ops._p(counts), B,
                                         ops._p(pi), ops._p(v), None,
                                         ctypes.c_void_p(s.cuda_stream)), "az_fl_eval_fwd")


def fl_grads(net, nodes, counts, target_pi, target_v, want_dlogits=False):
    """az_fl_grads: the gradients of train()'s loss into net.params.grads (overwritten)
    -> (loss tensor [1], dloss/dlogits [B][4] or None)."""
    B = counts.shape[0]
    net.params.sync()
    net.params.grad_flat  # allocate
    ws = net.grad_ws(B)
    loss = torch.empty(1, device=net.device)
    dl = torch.empty((B, ACTIONS), device=net.device) if want_dlogits else None
    g = _fl_params(net.params.grads, net.L)
    _lib.check(_lib.lib().az_fl_grads(ctypes.byref(net.desc), ops._p(nodes), ops._p(counts), B,
                                      ops._p(target_pi), ops._p(target_v), ctypes.byref(g),
                                      ops._p(loss), ops._p(dl), ops._p(ws), ws.numel(),
                                      ops._stream()), "az_fl_grads")
    return loss, dl


def clip_grad_norm(tensors, max_norm=1.0):
    """az_clip_grad_norm over device tensors, in place -> the total norm (device tensor [1])."""
    n = len(tensors)
    bufs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    sizes = (ctypes.c_int64 * n)(*[t.numel() for t in tensors])
    norm = torch.empty(1, device=tensors[0].device)
    _lib.check(_lib.lib().az_clip_grad_norm(bufs, sizes, n, max_norm, ops._p(norm), ops._stream()),
               "az_clip_grad_norm")
    return norm


class _Staging:
    """Mapped host memory for one batch in flight: the kernel reads nodes / counts and writes
    pi / v in place."""

    def __init__(self, cap, S):
        off = [0]
        for nbytes in (4 * cap * MAX_NODES * S, 4 * cap, 4 * cap * ACTIONS, 4 * cap):
            off.append(off[-1] + (nbytes + 255) // 256 * 256)
        self.cap = cap
        self.hb = ops.HostBuffer(off[-1])
        self.nodes = self.hb.view(off[0], torch.float32, (cap, MAX_NODES, S))
        self.counts = self.hb.view(off[1], torch.int32, (cap,))
        self.pi = self.hb.view(off[2], torch.float32, (cap, ACTIONS))
        self.v = self.hb.view(off[3], torch.float32, (cap,))
        self.nodes_np, self.counts_np = self.nodes.numpy(), self.counts.numpy()
        self.pi_np, self.v_np = self.pi.numpy(), self.v.numpy()


class _Pending:
    """A batch queued on the stream; result() waits for its event -> (pi, v, None, None)."""

    def __init__(self, owner, staging, event, n, merge=None):
        self.owner, self.staging, self.event, self.n, self.merge = owner, staging, event, n, merge
        self.out = None

    def result(self):
        if self.out is None:
            pi, v = self.owner._collect(self.staging, self.event, self.n)
            self.staging = None
            if self.merge is not None:
                pi, v = self.merge(pi, v)
            self.out = (pi, v, None, None)
        return self.out

    def __del__(self):
        if self.staging is not None:        # dropped unread: free the staging once the GPU is done
            try:
                self.owner._collect(self.staging, self.event, 0)
            except Exception:               # interpreter shutdown
                pass


class _Ready:
    def __init__(self, pi, v):
        self.out = (pi, v, None, None)

    def result(self):
        return self.out


class FrozenLakeNet:
    """The reference's wrapper class of the same name (FrozenLakeNet.py:36-250)."""

    def __init__(self, game, args):
        self.board_size = game.getBoardSize()
        self.action_size = game.getActionSize()
        self.args = args
        self.game = game
        self.device = nets.default_device()          # raises without a HIP device
        self.nnet = EnhancedNNet(self.board_size, self.action_size, args, device=self.device)
        self.S = self.nnet.S
        self._free = []                  # idle _Staging buffers
        self._state_nodes = {}           # state index -> its node boards [k][N][N] (_nodes_of)
        self._weights_version = 0        # bumped by train steps, load_checkpoint, restore
        self._table = None               # (key, pi [S+1][4], v [S+1])
        self.table_builds = 0            # evaluator calls made to fill the table
        self.eval_calls = 0              # every az_fl_eval_fwd call of this wrapper

    # -- node lists --------------------------------------------------------------------------
    def _node_list(self, board):
        """The board, then the canonical next state of every valid action, in action order
        (FrozenLakeNet.py:198-207)."""
        nodes = [board]
        valids = self.game.getValidMoves(board, 1)
        for a in range(self.action_size):
            if valids[a]:
                nxt, _ = self.game.getNextState(board, 1, a)
                nodes.append(self.game.getCanonicalForm(nxt, 1))
        return nodes

    def _nodes_of(self, board):
        """_node_list, remembered per state for one-hot and empty boards (the rules do not
        change, and a map has at most 65 of them)."""
        idx = self._state_index(board)
        if idx is None:
            return self._node_list(board)
        nodes = self._state_nodes.get(idx)
        if nodes is None:
            nodes = self._node_list(np.array(board, dtype=np.float32))
            self._state_nodes[idx] = nodes = np.asarray(nodes, dtype=np.float32)
        return nodes

    # -- evaluation --------------------------------------------------------------------------
    def _launch_nodes(self, node_lists, merge=None):
        """Queue one az_fl_eval_fwd call over a list of node lists."""
        n = len(node_lists)
        for nodes in node_lists:
            if not 1 <= len(nodes) <= MAX_NODES:
                raise ValueError(f"FrozenLakeNet: a leaf has 1 to {MAX_NODES} nodes, "
                                 f"got {len(nodes)}")
        st = next((s for s in self._free if s.cap >= n), None)
        if st is not None:
            self._free.remove(st)
        else:
            st = _Staging(max(8, 1 << (n - 1).bit_length()), self.S)
        for i, nodes in enumerate(node_lists):
            k = len(nodes)
            st.nodes_np[i, :k] = np.asarray(nodes, dtype=np.float32).reshape(k, self.S)
            st.counts_np[i] = k
        stream = torch.cuda.current_stream(self.device)
        self.eval_calls += 1
        fl_eval_fwd(self.nnet, st.nodes, st.counts, st.pi, st.v, n, stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        return _Pending(self, st, ev, n, merge)

    def _collect(self, staging, event, n):
        event.synchronize()
        out = staging.pi_np[:n].copy(), staging.v_np[:n].copy()
        self._free.append(staging)
        return out

    def _eval_nodes(self, node_lists):
        pi, v, _, _ = self._launch_nodes(node_lists).result()
        return pi, v

    # -- the whole-board table ---------------------------------------------------------------
    def _table_on(self):
        return os.environ.get("AZ_FL_TABLE", "1") not in ("0",)

    def _state_index(self, board):
        """Row of the table for a one-hot board (its cell) or the empty board (S); None for
        any other board."""
        flat = np.asarray(board).reshape(-1)
        if flat.size != self.S:
            return None
        nz = np.flatnonzero(flat)
        if nz.size == 0:
            return self.S
        if nz.size == 1 and flat[nz[0]] == 1:
            return int(nz[0])
        return None

    def _get_table(self):
        key = (self._weights_version, self.nnet.params.flat._version)
        if self._table is None or self._table[0] != key:
            n = self.board_size[0]
            boards = []
            for cell in range(self.S):
                b = np.zeros((n, n))
                b[cell // n, cell % n] = 1
                boards.append(b)
            boards.append(np.zeros((n, n)))
            pi, v = self._eval_nodes([self._nodes_of(b) for b in boards])
            self.table_builds += 1
            self._table = (key, pi, v)
        return self._table[1], self._table[2]

    def _weights_changed(self):
        self._weights_version += 1

    # -- the reference's surface ---------------------------------------------------------------
    def predict(self, board, neighbor_states=None):
        """(pi float32[4], v float32[1]) of one board (FrozenLakeNet.py:178-230).  A NaN output
        becomes the uniform policy / value 0, an exception uniform and 0.0, both counted."""
        self.nnet.eval()
        try:
            idx = self._state_index(board) if neighbor_states is None and self._table_on() \
                else None
            if idx is not None:
                tpi, tv = self._get_table()
                pi, v = tpi[idx].copy(), tv[idx:idx + 1].copy()
            else:
                nodes = neighbor_states if neighbor_states is not None \
                    else self._nodes_of(board)
                bpi, bv = self._eval_nodes([nodes])
                pi, v = bpi[0], bv[0:1]
            if np.isnan(pi).any() or np.isnan(v).any():
                nn_fallback.record("FrozenLakeNet.predict", FloatingPointError("NaN output"))
                if np.isnan(pi).any():
                    pi = np.ones_like(pi) / pi.size
                if np.isnan(v).any():
                    v = np.zeros_like(v)
            return pi, v
        except nn_fallback.NNFailure:
            raise
        except Exception as e:
            nn_fallback.record("FrozenLakeNet.predict", e)
            return np.ones(self.action_size) / self.action_size, 0.0

    def predict_batch_async(self, boards, stream=None):
        """Row-wise predict of [B,N,N] boards without waiting: .result() -> (pi float32[B,4],
        v float32[B], None, None).  Cached states are served from the table; the others go to
        the GPU as one call on the current stream."""
        if stream is not None:
            raise ValueError("FrozenLakeNet.predict_batch_async runs on the current stream")
        self.nnet.eval()
        B = len(boards)
        idx = [self._state_index(b) for b in boards] if self._table_on() else [None] * B
        rest = [i for i in range(B) if idx[i] is None]
        pi = np.empty((B, ACTIONS), np.float32)
        v = np.empty((B,), np.float32)
        if len(rest) < B:
            tpi, tv = self._get_table()
            hit = [i for i in range(B) if idx[i] is not None]
            rows = [idx[i] for i in hit]
            pi[hit], v[hit] = tpi[rows], tv[rows]
        if not rest:
            return _Ready(pi, v)

        def merge(rpi, rv):
            pi[rest], v[rest] = rpi, rv
            return pi, v

        return self._launch_nodes([self._nodes_of(np.asarray(boards[i])) for i in rest], merge)

    def predict_batch(self, boards):
        pi, v, _, _ = self.predict_batch_async(boards).result()
        return pi, v

    # -- training ----------------------------------------------------------------------------
    def train_step(self, boards, pis, vs):
        """One batch: gradients, clip_grad_norm_(max_norm=1.0), Adam (FrozenLakeNet.py:113-168)
        -> the loss (device tensor)."""
        node_lists = [self._nodes_of(np.asarray(b, dtype=np.float32)) for b in boards]
        B = len(node_lists)
        nodes = np.zeros((B, MAX_NODES, self.S), np.float32)
        counts = np.empty((B,), np.int32)
        for i, nl in enumerate(node_lists):
            nodes[i, :len(nl)] = np.asarray(nl, dtype=np.float32).reshape(len(nl), self.S)
            counts[i] = len(nl)
        dev = self.device
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        loss, _ = fl_grads(self.nnet, to(nodes), to(counts), to(np.asarray(pis, np.float32)),
                           to(np.asarray(vs, np.float64).astype(np.float32)))
        clip_grad_norm([self.nnet.params.grad_flat], 1.0)
        T.adam_step(self.nnet, self.args.lr)
        self._weights_changed()
        return loss

    def train(self, examples):
        """FrozenLakeNet.py:76-176: a fresh Adam per call; every epoch shuffles the examples with
        np.random.shuffle and walks them in consecutive batches; a batch with a NaN is skipped."""
        self.nnet.train()
        # args.log_losses: every epoch's mean batch loss goes into its slot of a device buffer,
        # read once after the last epoch into last_train_losses (empty when no epoch runs)
        keep = bool(nets._args_get(self.args, "log_losses", False))
        if keep:
            self.last_train_losses = []
        if not examples or len(examples) < 4:
            print("Not enough examples for training, need at least 4")
            return
        print(f"Training on {len(examples)} examples")
        examples = [(x[0], x[1], x[2]) for x in examples if x[2] is not None]
        if not examples:
            return
        self.nnet.params.reset_adam()
        if keep:
            lbuf = torch.zeros((self.args.epochs,), device=self.device)
            ran = [False] * self.args.epochs
        for epoch in range(self.args.epochs):
            np.random.shuffle(examples)
            bs = min(len(examples), self.args.batch_size)
            losses = []
            for i in range(0, len(examples), bs):
                boards, pis, vs = list(zip(*examples[i:i + bs]))
                if any(np.isnan(np.sum(x)) for x in boards) or \
                        any(np.isnan(np.sum(x)) for x in pis) or any(np.isnan(x) for x in vs):
                    print("NaN values detected in input data, skipping batch")
                    continue
                losses.append(self.train_step(boards, pis, vs))
            if losses:
                mean = torch.cat(losses).mean()
                if keep:
                    lbuf[epoch].copy_(mean)
                    ran[epoch] = True
                avg = float(mean.item())
                print(f"Epoch {epoch + 1}/{self.args.epochs} - Loss: {avg:.4f}")
        torch.cuda.current_stream(self.device).synchronize()
        if keep:
            host = lbuf.cpu().numpy()
            self.last_train_losses = [dict(epoch=e, **({"loss": float(host[e])} if ran[e] else {}))
                                      for e in range(self.args.epochs)]

    def evaluate(self, examples, chunk=4096):
        """The losses of the network on `examples` ((board, pi, v), as train() takes them; v None
        is dropped as there) without training on them -> {loss_pi, loss_v, loss, top1, entropy,
        target_entropy, n} (NetWrapper.evaluate's keys; loss_pi + loss_v is the loss train()
        minimises).  Every board is evaluated on the leaf train() builds for it (_nodes_of) by
        az_fl_eval_fwd, `chunk` leaves a call, and scored by az_policy_value_metrics straight from
        the mapped host memory the evaluator wrote; one device-to-host read at the end.  Draws no
        random number, writes no weight or optimiser state and leaves the training flag as it
        was."""
        from . import metrics
        chunk = max(1, int(chunk))
        examples = [(x[0], x[1], x[2]) for x in (examples or []) if x[2] is not None]
        mode = self.nnet.training
        sums = metrics.MetricSums(self.device, 1)
        try:
            if examples:
                tpi, tv = metrics._targets([e[1] for e in examples], [e[2] for e in examples],
                                           ACTIONS, self.device)
                for c0 in range(0, len(examples), chunk):
                    part = examples[c0:c0 + chunk]
                    pend = self._launch_nodes([self._nodes_of(np.asarray(e[0], dtype=np.float32))
                                               for e in part])
                    sums.hold.append(pend)
                    st = pend.staging
                    sums.add(0, st.pi[:len(part)], st.v[:len(part)], tpi[c0:c0 + chunk],
                             tv[c0:c0 + chunk])
            host = sums.read()
        finally:
            sums.hold.clear()
            self.nnet.train(mode)
        return ops.metrics_dict(host[0])

    # -- checkpoints -------------------------------------------------------------------------
    def save_checkpoint(self, folder, filename):
        if not os.path.exists(folder):
            os.makedirs(folder)
        torch.save({"state_dict": self.nnet.params.cpu_state_dict()},
                   os.path.join(folder, filename))

    def load_checkpoint(self, folder, filename):
        filepath = os.path.join(folder, filename)
        if not os.path.exists(filepath):
            print(f"No model found at {filepath}")
            return
        checkpoint = torch.load(filepath, map_location="cpu", weights_only=True)
        self.nnet.load_state_dict(checkpoint["state_dict"])
        self._weights_changed()

    def snapshot(self):
        return {"nnet": self.nnet.params.flat.clone()}

    def restore(self, snap):
        self.nnet.params.copy_flat_(snap["nnet"])
        self._weights_changed()
