"""The reference's NeuralNet wrappers (Net.py:1-61 duck type) on libaz_hip.

Same constructor signature (game, args), same methods and return types as
connect4/Connect4Net.py:62-147, connect4/Connect4GNN.py:14-220, tictactoe/TicTacToeNet.py:50-104
and tictactoe/TicTacToeGNN.py:9-181, plus batched entry points (predict_batch,
predict_batch_with_gnn, predict_both) for lock-step self-play.  Checkpoints are the same
torch.save dict ({'state_dict': ..., 'gnn': ...}) with the same keys, so files move freely
between the reference and this implementation.
"""
import ctypes
import logging
import os

import numpy as np
import torch

from . import _lib, nets, ops, train as T
from .nets import boards_to_device

log = logging.getLogger(__name__)
# one-launch leaf hand-over timeouts in this process (each switches one evaluator to the
# four-launch path for good); bench.py reports it, so a degraded arena cannot go unnoticed
_LEAF_TIMEOUTS = [0]


def leaf_timeouts():
    """How many one-launch leaf evaluations timed out in this process (_Batch1Direct._call)."""
    return _LEAF_TIMEOUTS[0]


def _dev_array(rows, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(np.array(rows), dtype=dtype)).to(device)


class PendingPrediction:
    """A batched prediction in flight on the device stream: boards went up from pinned host
    memory, the kernels are queued, the outputs come back into pinned host memory behind an
    event.  result() waits for that event only (the host keeps working meanwhile)."""

    def __init__(self, out_host, event, n, A, both):
        self.out_host, self.event, self.n, self.A, self.both = out_host, event, n, A, both

    def result(self):
        self.event.synchronize()
        out = self.out_host[:self.n].numpy().copy()
        A = self.A
        if self.both:
            return out[:, :A], out[:, A], out[:, A + 1:2 * A + 1], out[:, 2 * A + 1]
        return out[:, :A], out[:, A], None, None


class _PendingDirect:
    """A batched Connect4 prediction queued by _DirectBatch: the kernels write pi / v straight
    into mapped host memory; result() waits for the event and copies them out.

    The ring entry is owned through a token: only the prediction that took the entry may hand
    it back.  (A stale prediction object -- read long ago, dropped only when its variable is
    rebound -- must not free an entry a LATER prediction now holds: the next launch would then
    take the same host buffers and overwrite that prediction's outputs, which is what two
    self-play lanes did before the token.)  result() may be called more than once."""

    _tokens = iter(range(1, 1 << 62))

    def __init__(self, entry, views, event, n):
        # entry: the ring entry (its HostBuffer stays alive and reserved until result())
        self.entry, self.views, self.event, self.n = entry, views, event, n
        self.token = next(self._tokens)
        self.out = None
        entry["busy"] = True
        entry["owner"] = self.token

    def _release(self):
        if self.entry.get("owner") == self.token:
            self.entry["owner"] = None
            self.entry["busy"] = False

    def result(self):
        if self.out is None:
            self.event.synchronize()
            n = self.n
            self.out = tuple(None if a is None else a.numpy()[:n].copy() for a in self.views)
            self._release()
        return self.out

    def __del__(self):
        # dropped unread: the entry is free again once the device is done with it
        if self.entry.get("owner") == self.token:
            self.event.synchronize()
            self._release()


class _DirectBatch:
    """Batched predict_both / predict_batch for the 7x7 Connect4Net as ONE az_c4_eval_fwd call
    per batch (trunk + heads [+ output_transform + heads]): boards are read from and outputs
    written to mapped host memory (ops.HostBuffer, a ring of `depth` so that several batches can
    be in flight), device scratch is shared (the stream orders the batches).  Replaces ~10
    torch-level launches, a pinned H2D and a D2H copy per lock-step round."""

    def __init__(self, w, stream=None):
        self.w, self.cap, self.ring = w, 0, []
        self.stream = stream      # None: the current stream; else this stream (own scratch)
        self.fn = _lib.lib().az_c4_eval_fwd
        self.fn_name = "az_c4_eval_fwd"

    def _grow(self, n):
        w, dev, A, F = self.w, self.w.device, self.w.action_size, 3136
        cap = max(1024, 1 << (int(n) - 1).bit_length())
        torch.cuda.synchronize(dev)               # in-flight batches may use the old scratch
        self.feat = torch.empty((cap, F), device=dev)
        self.hidden = torch.empty((cap, F), device=dev)
        self.y = torch.empty((cap, F), device=dev)
        self.logp = torch.empty((cap, A), device=dev)
        self.glogp = torch.empty((cap, A), device=dev)
        L = _lib.lib()
        nb = max(int(L.az_transform_heads_ws_bytes(cap, F, A)), int(L.az_heads_ws_bytes(cap, F, A)))
        self.ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        W, G = w.nnet.params, w.gnn.params
        P = lambda t: t.data_ptr()  # noqa: E731
        self.desc = _lib.C4Eval(
            P(W["conv1.weight"]), P(W["conv1.bias"]), P(W["conv2.weight"]), P(W["conv2.bias"]),
            P(W["fc_policy.weight"]), P(W["fc_policy.bias"]), P(W["fc_value.weight"]),
            P(W["fc_value.bias"]), A, P(G["output_transform.0.weight"]),
            P(G["output_transform.0.bias"]), P(G["output_transform.2.weight"]),
            P(G["output_transform.2.bias"]), cap, P(self.feat), P(self.hidden), P(self.y),
            P(self.logp), P(self.glogp), P(self.ws), self.ws.numel())
        self.ring = []        # entries still held by unread predictions keep their buffers
        self.cap = cap

    def _entry(self):
        """A host staging set no unread prediction holds (a new one when all are held)."""
        for e in self.ring:
            if not e["busy"]:
                return e
        w, cap, A = self.w, self.cap, self.w.action_size
        off = [0, (cap * w.board_x * w.board_y + 255) // 256 * 256]
        for k in (A, 1, A, 1):
            off.append(off[-1] + (4 * cap * k + 255) // 256 * 256)
        hb = ops.HostBuffer(off[-1])
        e = {"busy": False, "hb": hb,
             "in": hb.view(0, torch.int8, (cap, w.board_x, w.board_y)),
             "out": [hb.view(off[1 + j], torch.float32, (cap, k) if k > 1 else (cap,))
                     for j, k in enumerate((A, 1, A, 1))]}
        self.ring.append(e)
        return e

    def launch(self, boards, both):
        boards = np.asarray(boards)
        n = boards.shape[0]
        if n > self.cap:
            self._grow(n)
        e = self._entry()
        hin, outs = e["in"], e["out"]
        hin.numpy()[:n] = boards
        pi, v, gpi, gv = outs if both else (outs[0], outs[1], None, None)
        s = self.stream if self.stream is not None else torch.cuda.current_stream(self.w.device)
        P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        rc = self.fn(ctypes.byref(self.desc), ctypes.c_void_p(hin.data_ptr()), n, P(pi), P(v),
                     P(gpi), P(gv), ctypes.c_void_p(s.cuda_stream))
        if rc:
            _lib.check(rc, self.fn_name)
        ev = torch.cuda.Event()
        ev.record(s)
        return _PendingDirect(e, (pi, v, gpi, gv), ev, n)


class _TttDirectBatch(_DirectBatch):
    """_DirectBatch for the TicTacToeNet (n = 3..5): ONE az_ttt_eval_fwd call per batch, same
    host ring, same ownership tokens.  Without a GNN (the CNN-only wrapper) only `both=False`
    batches exist and the descriptor carries no output_transform."""

    def __init__(self, w, stream=None):
        super().__init__(w, stream)
        self.fn = _lib.lib().az_ttt_eval_fwd
        self.fn_name = "az_ttt_eval_fwd"

    def _grow(self, n):
        w = self.w
        cap = max(1024, 1 << (int(n) - 1).bit_length())
        torch.cuda.synchronize(w.device)          # in-flight batches may use the old scratch
        self.ev = ops.TttEval(w.nnet.params, w.gnn.params if w.has_gnn else None, w.nnet.n,
                              w.action_size, cap, w.device)
        self.desc = self.ev.desc
        self.ring = []        # entries still held by unread predictions keep their buffers
        self.cap = cap


class _C4nDirectBatch(_DirectBatch):
    """_DirectBatch for the Connect4Net on 4x4, 5x5, 6x6 and 8x8 boards: ONE az_c4n_eval_fwd call
    per batch, same host ring, same ownership tokens.  Without a GNN (the CNN-only wrapper) only
    `both=False` batches exist and the descriptor carries no output_transform (and no
    workspace)."""

    def __init__(self, w, stream=None):
        super().__init__(w, stream)
        self.fn = _lib.lib().az_c4n_eval_fwd
        self.fn_name = "az_c4n_eval_fwd"

    def _grow(self, n):
        w = self.w
        cap = max(1024, 1 << (int(n) - 1).bit_length())
        torch.cuda.synchronize(w.device)          # in-flight batches may use the old scratch
        self.ev = ops.C4nEval(w.nnet.params, w.gnn.params if w.has_gnn else None, w.nnet.n,
                              w.action_size, cap, w.device)
        self.desc = self.ev.desc
        self.ring = []        # entries still held by unread predictions keep their buffers
        self.cap = cap


class _C4rDirectBatch(_DirectBatch):
    """_DirectBatch for the Connect4Net on the rectangular boards of ops.C4R_SHAPES (7x6, 6x5, 5x4,
    8x7): ONE az_c4r_eval_fwd call per batch, same host ring, same ownership tokens.  Without a
    GNN (the CNN-only wrapper) only `both=False` batches exist and the descriptor carries no
    output_transform (and no workspace)."""

    def __init__(self, w, stream=None):
        super().__init__(w, stream)
        self.fn = _lib.lib().az_c4r_eval_fwd
        self.fn_name = "az_c4r_eval_fwd"

    def _grow(self, n):
        w = self.w
        cap = max(1024, 1 << (int(n) - 1).bit_length())
        torch.cuda.synchronize(w.device)          # in-flight batches may use the old scratch
        self.ev = ops.C4rEval(w.nnet.params, w.gnn.params if w.has_gnn else None,
                              (w.board_x, w.board_y), w.action_size, cap, w.device)
        self.desc = self.ev.desc
        self.ring = []        # entries still held by unread predictions keep their buffers
        self.cap = cap


class _ExactBatch(_DirectBatch):
    """_DirectBatch under args.batch_invariant, for every board with a fused trunk (Connect4 and
    TicTacToe, with or without a GNN): ONE az_eval_exact_fwd call per max_B rows, the same launch
    sequence at 1 row and at 4,096, so a board's outputs do not depend on the batch it rides in.
    Same host ring and ownership tokens; a batch above CAP rows runs as consecutive chunks on the
    same scratch, which invariance makes the same result.  kind: "std" -> (pi, v, None, None),
    "gnn" -> (None, None, gpi, gv), "both" -> all four."""

    CAP = 4096

    def __init__(self, w, stream=None):
        super().__init__(w, stream)
        self.fn = _lib.lib().az_eval_exact_fwd
        self.fn_name = "az_eval_exact_fwd"

    def _grow(self, n):
        w = self.w
        cap = min(self.CAP, max(1024, 1 << (int(n) - 1).bit_length()))
        torch.cuda.synchronize(w.device)          # in-flight batches may use the old scratch
        self.ev = ops.EvalExact(w.nnet.params, w.gnn.params if w.has_gnn else None,
                                ops.exact_board(w.nnet), w.action_size, cap, w.device)
        self.desc = self.ev.desc
        self.cap = cap

    def _entry(self, n):
        """A host staging set of >= n rows no unread prediction holds (idle smaller ones go)."""
        for e in self.ring:
            if not e["busy"] and e["rows"] >= n:
                return e
        self.ring = [e for e in self.ring if e["busy"]]
        w, A = self.w, self.w.action_size
        rows = max(1024, 1 << (int(n) - 1).bit_length())
        off = [0, (rows * w.board_x * w.board_y + 255) // 256 * 256]
        for k in (A, 1, A, 1):
            off.append(off[-1] + (4 * rows * k + 255) // 256 * 256)
        hb = ops.HostBuffer(off[-1])
        e = {"busy": False, "hb": hb, "rows": rows,
             "in": hb.view(0, torch.int8, (rows, w.board_x, w.board_y)),
             "out": [hb.view(off[1 + j], torch.float32, (rows, k) if k > 1 else (rows,))
                     for j, k in enumerate((A, 1, A, 1))]}
        self.ring.append(e)
        return e

    def launch(self, boards, both, kind=None):
        kind = kind or ("both" if both else "std")
        boards = np.asarray(boards)
        n = boards.shape[0]
        if n > self.cap and self.cap < self.CAP:
            self._grow(n)
        e = self._entry(n)
        hin, outs = e["in"], e["out"]
        hin.numpy()[:n] = boards.reshape(n, hin.shape[1], hin.shape[2])
        pi, v = (outs[0], outs[1]) if kind != "gnn" else (None, None)
        gpi, gv = (outs[2], outs[3]) if kind != "std" else (None, None)
        s = self.stream if self.stream is not None else torch.cuda.current_stream(self.w.device)
        P = lambda t, c0: None if t is None else ctypes.c_void_p(t[c0:].data_ptr())  # noqa: E731
        for c0 in range(0, n, self.cap):
            rc = self.fn(ctypes.byref(self.desc), P(hin, c0), min(self.cap, n - c0), P(pi, c0),
                         P(v, c0), P(gpi, c0), P(gv, c0), ctypes.c_void_p(s.cuda_stream))
            if rc:
                _lib.check(rc, self.fn_name)
        ev = torch.cuda.Event()
        ev.record(s)
        return _PendingDirect(e, (pi, v, gpi, gv), ev, n)


class _ExactBatch1:
    """What _graph1 hands out under args.batch_invariant: run() / run_rows() of the batch-1
    evaluators on the exact route (a batch-1 call is then just a batch of one row)."""

    def __init__(self, w, kind):
        self.w, self.kind = w, kind

    def run_rows(self, boards):
        return self.w._exact(boards, self.kind).result()

    def run(self, board):
        """One board -> the packed row [pi, v(, gpi, gv)]."""
        pi, v, gpi, gv = self.run_rows(np.asarray(board)[None])
        parts = [a.reshape(-1) for a in (pi, v, gpi, gv) if a is not None]
        return np.concatenate(parts).astype(np.float32, copy=False)


class _PinnedRing:
    """Pinned host staging buffers reused round-robin (`depth` predictions in flight)."""

    def __init__(self, depth=4):
        self.depth, self.i, self.bufs = depth, 0, {}

    def get(self, key, shape, dtype):
        k = (key, self.i % self.depth)
        b = self.bufs.get(k)
        if b is None or b.shape[0] < shape[0] or tuple(b.shape[1:]) != tuple(shape[1:]):
            b = torch.empty((max(shape[0], 1024),) + tuple(shape[1:]), dtype=dtype,
                            pin_memory=True)
            self.bufs[k] = b
        return b

    def advance(self):
        self.i += 1


class _Batch1Graph:
    """The whole batch-1 evaluation captured as ONE hipGraph: pinned host board -> H2D ->
    trunk -> heads [-> GNN tail] -> packed outputs -> D2H into pinned host memory.  MCTS asks
    for one leaf at a time wherever simulations depend on each other (the reference's
    MCTS.search, the arena's per-iteration trees), so this path is launch- and copy-latency
    bound; one replay replaces ~8 launches and two synchronous copies.  The kernels are the
    eager path's, so the outputs are bit-identical.  Parameters are updated in place (train,
    load_state_dict, restore), so the captured pointers stay valid.

    kind: "std" -> [pi, v], "gnn" -> [gnn_pi, gnn_v], "both" -> [pi, v, gnn_pi, gnn_v]."""

    def __init__(self, w, kind):
        dev = w.device
        A = w.action_size
        width = {"std": A + 1, "gnn": A + 1, "both": 2 * A + 2}[kind]
        # zero-copy staging (ops.HostBuffer): the trunk reads the board and the heads write
        # their pi / v straight from / into mapped host memory, so the graph has no copy
        # nodes; AZ_NO_ZEROCOPY=1 keeps the pinned-buffer + H2D / D2H copies instead
        self.host = None
        if os.environ.get("AZ_NO_ZEROCOPY", "0") in ("", "0"):
            try:
                self.host = ops.HostBuffer(256 + 4 * width)
            except RuntimeError:
                self.host = None
        if self.host is not None:
            self.h_in = self.host.view(0, torch.int8, (1, w.board_x, w.board_y))
            self.h_out = self.host.view(256, torch.float32, (1, width))
        else:
            self.h_in = torch.zeros((1, w.board_x, w.board_y), dtype=torch.int8, pin_memory=True)
            self.d_in = torch.zeros((1, w.board_x, w.board_y), dtype=torch.int8, device=dev)
            self.h_out = torch.zeros((1, width), dtype=torch.float32, pin_memory=True)
            self.d_out = torch.zeros((1, width), dtype=torch.float32, device=dev)
        zc = self.host is not None

        def body():
            if zc:
                o = self.h_out
                if kind in ("std", "both") and hasattr(w.nnet, "features_heads"):
                    f, _, _, _ = w.nnet.features_heads(self.h_in, pi=o[:, :A], v=o[:, A])
                elif kind in ("std", "both"):
                    f = w.nnet.features(self.h_in)
                    w.nnet.heads(f, pi=o[:, :A], v=o[:, A])
                else:
                    f = w.nnet.features(self.h_in)
                if kind in ("gnn", "both"):
                    c = 0 if kind == "gnn" else A + 1
                    nets.gnn_per_row_heads(w.nnet, w.gnn, f, pi=o[:, c:c + A], v=o[:, c + A])
                return
            self.d_in.copy_(self.h_in, non_blocking=True)
            f = w.nnet.features(self.d_in)
            parts = []
            if kind in ("std", "both"):
                _, pi, v = w.nnet.heads(f)
                parts += [pi, v[:, None]]
            if kind in ("gnn", "both"):
                _, gpi, gv = nets.gnn_per_row_heads(w.nnet, w.gnn, f)
                parts += [gpi, gv[:, None]]
            torch.cat(parts, dim=1, out=self.d_out)
            self.h_out.copy_(self.d_out, non_blocking=True)

        # the graph owns its workspace: the shared one is re-allocated when a large batch needs
        # more, which would leave a captured kernel pointing at freed memory
        self.ws = torch.empty((16 << 20,), dtype=torch.uint8, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with ops.pinned_workspace(dev, self.ws):
            with torch.cuda.stream(side):
                body()                   # eager warm-up on the same buffers
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                body()
        self.dev = dev

    def run(self, board):
        self.h_in.numpy()[0] = board
        self.graph.replay()
        torch.cuda.current_stream(self.dev).synchronize()
        return self.h_out.numpy()[0].copy()


class _Batch1Direct:
    """Connect4 evaluation of up to `cap` boards as ONE C call (az_c4_eval_fwd: 1 + 3 direct
    launches) with zero-copy staging: the boards are read and pi / v written in place in mapped
    host memory.  Measured on MI355X, a hipGraph replay costs ~14 us of host time before its
    first kernel runs, more than these launches, which overlap the GPU work they queue.  Same
    kernels as the eager path (bit-identical outputs); parameters are read through the pointers
    fixed here, which stay valid because every update is in place.  kind as _Batch1Graph.

    Output layout in the host buffer: pi [cap][A], v [cap] (kind std/both), then gpi [cap][A],
    gv [cap] (kind gnn/both); with cap = 1 that is the packed [pi, v(, gpi, gv)] row run()
    returns.  cap = 8 serves the arena's speculative leaf batches (rows <= 8 take the same
    GEMV arithmetic as one row: mcts_native.ArenaPlayer, tests/test_gpu_selfplay.py)."""

    def __init__(self, w, kind, cap=1):
        dev = w.device
        A = w.action_size
        self.kind, self.A, self.cap = kind, A, cap
        std = kind in ("std", "both")
        gnn = kind in ("gnn", "both")
        width = (A + 1) * (int(std) + int(gnn))
        self.host = ops.HostBuffer(256 * cap + 4 * width * cap)
        self.h_in = self.host.view(0, torch.int8, (cap, w.board_x, w.board_y))
        self.h_out = self.host.view(256 * cap, torch.float32, (cap * width,))
        F = 3136
        self.feat = torch.empty((cap, F), device=dev)
        self.hidden = torch.empty((cap, F), device=dev) if gnn else None
        self.y = torch.empty((cap, F), device=dev) if gnn else None
        self.logp = torch.empty((cap, A), device=dev)
        self.glogp = torch.empty((cap, A), device=dev)
        self.ws = torch.empty((16 << 20,), dtype=torch.uint8, device=dev)
        W = w.nnet.params
        G = w.gnn.params if gnn else None
        P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.desc = _lib.C4Eval(
            P(W["conv1.weight"]), P(W["conv1.bias"]), P(W["conv2.weight"]), P(W["conv2.bias"]),
            P(W["fc_policy.weight"]), P(W["fc_policy.bias"]), P(W["fc_value.weight"]),
            P(W["fc_value.bias"]), A,
            P(G["output_transform.0.weight"]) if gnn else None,
            P(G["output_transform.0.bias"]) if gnn else None,
            P(G["output_transform.2.weight"]) if gnn else None,
            P(G["output_transform.2.bias"]) if gnn else None,
            cap, P(self.feat), P(self.hidden), P(self.y), P(self.logp), P(self.glogp),
            P(self.ws), self.ws.numel())
        if kind == "both":
            # the one-launch form for 1-2 rows (c4_leaf_kernel): hand-over counters on the
            # device, zero between launches, and a host-visible timeout flag
            self.sync = torch.zeros(4096, dtype=torch.int32, device=dev)
            self.errbuf = ops.HostBuffer(256)
            self.err = self.errbuf.view(0, torch.int32, (1,))
            self.err.zero_()
            self.desc.sync = ctypes.c_void_p(self.sync.data_ptr())
            self.desc.err = ctypes.c_void_p(self.err.data_ptr())
            self.err_np = self.err.numpy()
        else:
            self.err_np = None
        L = _lib.lib()
        assert max(int(L.az_transform_heads_ws_bytes(cap, F, A)),
                   int(L.az_heads_ws_bytes(cap, F, A))) <= self.ws.numel()
        o = self.h_out.numpy()
        # views: pi [cap][A], v [cap], gpi [cap][A], gv [cap] (None where the kind has none)
        off, views = 0, []
        for on in (std, gnn):
            if on:
                views += [o[off:off + cap * A].reshape(cap, A), o[off + cap * A:off + cap * (A + 1)]]
                off += cap * (A + 1)
            else:
                views += [None, None]
        self.views = views
        self.args = (ctypes.byref(self.desc), ctypes.c_void_p(self.h_in.data_ptr()))
        self.outs = tuple(None if v is None else ctypes.c_void_p(v.ctypes.data) for v in views)
        self.fn = L.az_c4_eval_fwd
        self.fn_name = "az_c4_eval_fwd"
        self.dev = dev
        # the stream current at construction (the default stream, where train() updates the
        # parameters) serves every call: torch.cuda.current_stream() costs ~2.7 us per call
        self.stream = torch.cuda.current_stream(dev)
        self.sptr = ctypes.c_void_p(self.stream.cuda_stream)
        self.h_in_np = self.h_in.numpy()
        self.h_out_np = self.h_out.numpy()
        # keep the parameter tensors alive with the pointers taken above
        self._keep = (W, G)

    def _call(self, n):
        s = self.stream
        rc = self.fn(*self.args, n, *self.outs, self.sptr)
        if rc:
            _lib.check(rc, self.fn_name)
        s.synchronize()
        if self.err_np is not None and self.err_np[0]:
            # the one-launch form's hand-over timed out (its blocks were not all resident, e.g.
            # another process held CUs): discard the outputs, zero the counters, and evaluate
            # again with the four-launch path from now on
            self.sync.zero_()
            s.synchronize()
            self.err_np[0] = 0
            self.desc.sync = None
            self.desc.err = None
            self.err_np = None
            self.leaf_timeouts = getattr(self, "leaf_timeouts", 0) + 1
            _LEAF_TIMEOUTS[0] += 1
            log.warning("az_c4_eval_fwd: the one-launch leaf kernel's hand-over timed out (not "
                        "all its blocks were resident); this evaluator uses the four-launch path "
                        "from now on (%d timeout(s) in this process)", _LEAF_TIMEOUTS[0])
            rc = self.fn(*self.args, n, *self.outs, self.sptr)
            if rc:
                _lib.check(rc, "az_c4_eval_fwd")
            s.synchronize()

    def run(self, board):
        """One board -> the packed row [pi, v(, gpi, gv)] (cap 1)."""
        self.h_in_np[0] = board
        self._call(1)
        return self.h_out_np.copy()

    def run_rows(self, boards):
        """n <= cap boards -> (pi [n][A], v [n], gpi, gv) copies (None where the kind has none)."""
        n = len(boards)
        self.h_in_np[:n] = boards
        self._call(n)
        return tuple(None if v is None else v[:n].copy() for v in self.views)


class _TttBatch1Direct(_Batch1Direct):
    """_Batch1Direct for the TicTacToeNet (n = 3..5): up to `cap` boards as ONE az_ttt_eval_fwd
    call (4 launches for std, 6 for gnn / both; no in-kernel hand-over, so no timeout path).
    Same host layout, run() and run_rows() as the Connect4 evaluator."""

    eval_class = ops.TttEval
    fn_name = "az_ttt_eval_fwd"

    @staticmethod
    def _board_arg(w):
        """What eval_class takes for the board: the side."""
        return w.nnet.n

    def __init__(self, w, kind, cap=1):
        dev = w.device
        A = w.action_size
        self.kind, self.A, self.cap = kind, A, cap
        std = kind in ("std", "both")
        gnn = kind in ("gnn", "both")
        width = (A + 1) * (int(std) + int(gnn))
        self.host = ops.HostBuffer(256 * cap + 4 * width * cap)
        self.h_in = self.host.view(0, torch.int8, (cap, w.board_x, w.board_y))
        self.h_out = self.host.view(256 * cap, torch.float32, (cap * width,))
        self.ev = self.eval_class(w.nnet.params, w.gnn.params if gnn else None,
                                  self._board_arg(w), A, cap, dev)
        self.desc = self.ev.desc
        self.err_np = None
        o = self.h_out.numpy()
        # views: pi [cap][A], v [cap], gpi [cap][A], gv [cap] (None where the kind has none)
        off, views = 0, []
        for on in (std, gnn):
            if on:
                views += [o[off:off + cap * A].reshape(cap, A), o[off + cap * A:off + cap * (A + 1)]]
                off += cap * (A + 1)
            else:
                views += [None, None]
        self.views = views
        self.args = (ctypes.byref(self.desc), ctypes.c_void_p(self.h_in.data_ptr()))
        self.outs = tuple(None if v is None else ctypes.c_void_p(v.ctypes.data) for v in views)
        self.fn = getattr(_lib.lib(), self.fn_name)
        self.dev = dev
        self.stream = torch.cuda.current_stream(dev)
        self.sptr = ctypes.c_void_p(self.stream.cuda_stream)
        self.h_in_np = self.h_in.numpy()
        self.h_out_np = self.h_out.numpy()


class _C4nBatch1Direct(_TttBatch1Direct):
    """_Batch1Direct for the Connect4Net on 4x4, 5x5, 6x6 and 8x8 boards: up to `cap` boards as
    ONE az_c4n_eval_fwd call (1 launch for std, 4 for gnn / both; no in-kernel hand-over, so no
    timeout path).  Same host layout, run() and run_rows() as the 7x7 evaluator."""

    eval_class = ops.C4nEval
    fn_name = "az_c4n_eval_fwd"


class _C4rBatch1Direct(_TttBatch1Direct):
    """_Batch1Direct for the Connect4Net on the rectangular boards of ops.C4R_SHAPES (7x6, 6x5,
    5x4, 8x7): up to `cap` boards as ONE az_c4r_eval_fwd call (1 launch for std, 4 for gnn / both;
    no in-kernel hand-over, so no timeout path).  Same host layout, run() and run_rows() as the
    7x7 evaluator."""

    eval_class = ops.C4rEval
    fn_name = "az_c4r_eval_fwd"

    @staticmethod
    def _board_arg(w):
        return (w.board_x, w.board_y)


class _StarDirect:
    """GNN evaluation of up to 8 leaves with their neighbourhoods (stars of <= 9 boards) as ONE C
    call (az_c4_star_eval_fwd: the fused trunk, four launches per GNN layer, output_transform and
    the heads) with zero-copy staging, like _C4rBatch1Direct: boards and counts are read and gpi /
    gv written in place in mapped host memory.  A star's outputs are bit-identical to the same
    star evaluated alone."""

    cap = ops.STAR_MAX_STARS

    def __init__(self, w):
        dev, A, cap, N = w.device, w.action_size, self.cap, ops.STAR_MAX_NODES
        hw = w.board_x * w.board_y
        off = [0]
        for nbytes in (cap * N * hw, 4 * cap, 4 * cap * A, 4 * cap):
            off.append(off[-1] + (nbytes + 255) // 256 * 256)
        self.host = ops.HostBuffer(off[-1])
        self.h_in = self.host.view(off[0], torch.int8, (cap, N, w.board_x, w.board_y))
        self.h_counts = self.host.view(off[1], torch.int32, (cap,))
        self.h_pi = self.host.view(off[2], torch.float32, (cap, A))
        self.h_v = self.host.view(off[3], torch.float32, (cap,))
        self.h_in.zero_()
        self.ev = ops.C4StarEval(w.nnet.params, w.gnn.params, (w.board_x, w.board_y), A,
                                 w.gnn.num_layers, cap, dev)
        self.in_np, self.counts_np = self.h_in.numpy(), self.h_counts.numpy()
        self.pi_np, self.v_np = self.h_pi.numpy(), self.h_v.numpy()
        self.fn = _lib.lib().az_c4_star_eval_fwd
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        self.args = (ctypes.byref(self.ev.desc), P(self.h_in), P(self.h_counts))
        self.outs = (P(self.h_pi), P(self.h_v))
        self.stream = torch.cuda.current_stream(dev)
        self.sptr = ctypes.c_void_p(self.stream.cuda_stream)

    def run(self, node_lists):
        """len(node_lists) <= 8 stars of <= 9 boards each -> (gpi [B][A], gv [B]) copies."""
        B = len(node_lists)
        for b, nodes in enumerate(node_lists):
            self.counts_np[b] = len(nodes)
            self.in_np[b, :len(nodes)] = nodes
        rc = self.fn(*self.args, B, *self.outs, self.sptr)
        if rc:
            _lib.check(rc, "az_c4_star_eval_fwd")
        self.stream.synchronize()
        return self.pi_np[:B].copy(), self.v_np[:B].copy()


class _TttStarDirect:
    """_StarDirect for TicTacToe: up to 8 leaves with their neighbourhoods (stars of <= n^2 + 1
    boards, packed) as ONE C call (az_ttt_star_eval_fwd: the fused trunk, four launches per GNN
    layer, output_transform, fc1 / fc2 and the heads) with zero-copy staging: packed rows and offs
    are read and gpi / gv written in place in one mapped host buffer.  A star's outputs are
    bit-identical to the same star evaluated alone."""

    cap = ops.STAR_MAX_STARS

    def __init__(self, w):
        dev, A, cap = w.device, w.action_size, self.cap
        n = w.nnet.n
        self.nodes = n * n + 1
        off = [0]
        for nbytes in (cap * self.nodes * n * n, 4 * (cap + 1), 4 * cap * A, 4 * cap):
            off.append(off[-1] + (nbytes + 255) // 256 * 256)
        self.host = ops.HostBuffer(off[-1])
        self.h_in = self.host.view(off[0], torch.int8, (cap * self.nodes, n, n))
        self.h_offs = self.host.view(off[1], torch.int32, (cap + 1,))
        self.h_pi = self.host.view(off[2], torch.float32, (cap, A))
        self.h_v = self.host.view(off[3], torch.float32, (cap,))
        self.h_in.zero_()
        self.h_offs.zero_()
        self.ev = ops.TttStarEval(w.nnet.params, w.gnn.params, n, A, w.gnn.num_layers, cap, dev)
        self.in_np, self.offs_np = self.h_in.numpy(), self.h_offs.numpy()
        self.pi_np, self.v_np = self.h_pi.numpy(), self.h_v.numpy()
        self.fn = _lib.lib().az_ttt_star_eval_fwd
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        self.args = (ctypes.byref(self.ev.desc), P(self.h_in), P(self.h_offs))
        self.outs = (P(self.h_pi), P(self.h_v))
        self.stream = torch.cuda.current_stream(dev)
        self.sptr = ctypes.c_void_p(self.stream.cuda_stream)

    def run(self, node_lists):
        """len(node_lists) <= 8 stars of <= n^2 + 1 boards each -> (gpi [B][A], gv [B]) copies."""
        B, V = len(node_lists), 0
        for b, nodes in enumerate(node_lists):
            self.in_np[V:V + len(nodes)] = nodes
            V += len(nodes)
            self.offs_np[b + 1] = V
        rc = self.fn(*self.args, B, V, *self.outs, self.sptr)
        if rc:
            _lib.check(rc, "az_ttt_star_eval_fwd")
        self.stream.synchronize()
        return self.pi_np[:B].copy(), self.v_np[:B].copy()


# Device bytes one chunk of predict_both_stars may hold in the buffers that grow with the batch.
# Per packed row: its features (4 F) and, in az_gnn_star_batch_infer's workspace, the fp16 planes
# of the projection GEMM's A operand (4 F) and its P row (2 H 4 = 1 KB); per star: TA (8 F), gate,
# u1, the next row 0, the leaf row and x0 (4 F each) and its Pt row; fixed: the 40 MB of split-K
# slabs plus ~2 MB of scales.  At F = 3136 that is 26 KB per row and 88 KB per star, so 1 GiB
# holds about 4,000 stars of 9 boards: a 2,048-game lock-step round is one chunk.
STAR_CHUNK_BYTES = 1 << 30


def _star_chunk_cost(F):
    """(bytes per packed row, bytes per star, fixed bytes) of STAR_CHUNK_BYTES' derivation."""
    return 8 * F + 1024 + 64, 28 * F + 1024 + 64, 42 << 20


def star_chunks(offs, F, budget=None, cost=None):
    """Split B stars (offs int [B+1]) into consecutive runs [b0, b1) whose buffers stay under the
    budget (STAR_CHUNK_BYTES); a run is at least one star.  cost: the route's (bytes per packed
    row, bytes per star, fixed bytes), _star_chunk_cost(F) when None."""
    budget = STAR_CHUNK_BYTES if budget is None else budget
    cr, cs, fixed = _star_chunk_cost(F) if cost is None else cost
    B = len(offs) - 1
    lin = cr * np.asarray(offs, np.int64) + cs * np.arange(B + 1, dtype=np.int64)
    out, b0 = [], 0
    while b0 < B:
        b1 = int(np.searchsorted(lin, lin[b0] + budget - fixed, side="right")) - 1
        b1 = min(B, max(b1, b0 + 1))
        out.append((b0, b1))
        b0 = b1
    return out


class _StarBatch:
    """predict_both_stars for one stream: packed stars in mapped host memory (ops.HostBuffer, a
    ring so that several batches can be in flight), the trunk on all V rows, the standard heads on
    the B leaf rows, az_gnn_star_batch_infer, output_transform + heads on the row 0s, outputs
    written in place in mapped host memory.  Feature rows, row 0s and the workspace are allocated
    once per capacity (small head temporaries come from torch's caching allocator); a batch whose
    buffers would exceed STAR_CHUNK_BYTES runs as consecutive chunks on the same scratch."""

    def __init__(self, w, stream=None):
        self.w, self.stream = w, stream
        self.capV = self.capB = 0
        self.ring = []
        if w.gnn.num_layers > ops.STAR_MAX_LAYERS:
            raise ValueError(f"predict_both_stars: {w.gnn.num_layers} GNN layers > "
                             f"{ops.STAR_MAX_LAYERS} (az_gnn_star_batch_infer)")

    def _grow(self, V, B):
        w, dev, F = self.w, self.w.device, self.w.feature_dim
        capV = max(self.capV, (V + 1023) // 1024 * 1024)
        capB = max(self.capB, (B + 255) // 256 * 256)
        torch.cuda.synchronize(dev)               # in-flight batches may use the old scratch
        self.feat = torch.empty((capV, F), device=dev)
        self.leaf = torch.empty((capB, F), device=dev)
        self.x0 = torch.empty((capB, F), device=dev)
        nl = w.gnn.num_layers
        nb = ops.gnn_star_batch_ws_bytes(capB, capV, F, nl)
        if nb == 0:
            raise ValueError(f"az_gnn_star_batch_infer: unsupported shape B={capB} V={capV} F={F}")
        self.ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        self.layers = (ops.LayerW * max(nl, 1))(*[ops.layer_weights(l.weights())
                                                  for l in w.gnn.layers])
        # the heads' GEMMs take this stream's own workspace (the shared one would be written by
        # two lanes' streams at once)
        L, A = _lib.lib(), w.action_size
        hb = max(int(L.az_transform_heads_ws_bytes(capB, F, A)),
                 int(L.az_heads_ws_bytes(capB, F, A)), 64 << 20)
        self.hws = torch.empty((hb,), dtype=torch.uint8, device=dev)
        self.capV, self.capB = capV, capB

    def _entry(self, V, B):
        """A host staging set no unread prediction holds, large enough for V rows / B stars."""
        for e in self.ring:
            if not e["busy"] and e["V"] >= V and e["B"] >= B:
                return e
        self.ring = [e for e in self.ring if e["busy"]]   # too small and idle: dropped
        w, A = self.w, self.w.action_size
        cV, cB = (V + 1023) // 1024 * 1024, (B + 255) // 256 * 256
        off = [0]
        for nbytes in (cV * w.board_x * w.board_y, 4 * (2 * cB + 2), 4 * cB * A, 4 * cB,
                       4 * cB * A, 4 * cB):
            off.append(off[-1] + (nbytes + 255) // 256 * 256)
        hb = ops.HostBuffer(off[-1])
        e = {"busy": False, "hb": hb, "V": cV, "B": cB,
             "in": hb.view(off[0], torch.int8, (cV, w.board_x, w.board_y)),
             "offs": hb.view(off[1], torch.int32, (2 * cB + 2,)),
             "out": [hb.view(off[2 + j], torch.float32, (cB, k) if k > 1 else (cB,))
                     for j, k in enumerate((A, 1, A, 1))]}
        self.ring.append(e)
        return e

    def _features(self, b, out):
        """The wrapper's batched feature path into `out`: a fused trunk where the board has one,
        the conv launches otherwise."""
        net = self.w.nnet
        W = net.params
        if isinstance(net, nets.Connect4Net):
            fn = {"c4": ops.c4_trunk, "c4n": ops.c4n_trunk, "c4r": ops.c4r_trunk}.get(net.route)
            if fn is not None:
                return fn(b, W, out=out)
        elif isinstance(net, nets.TicTacToeNet) and 3 <= net.n <= 5:
            return ops.ttt_trunk(b, W, out=out)
        out.copy_(net.features(b))
        return out

    def launch(self, rows, offs):
        w, F, A = self.w, self.w.feature_dim, self.w.action_size
        rows = np.asarray(rows)
        offs = np.asarray(offs, dtype=np.int64)
        B, V = len(offs) - 1, int(offs[-1])
        if B < 1 or offs[0] != 0 or V != rows.shape[0] or np.any(np.diff(offs) < 1):
            raise ValueError("predict_both_stars: offs must ascend from 0 to len(rows), one or "
                             "more rows per star")
        chunks = star_chunks(offs, F, STAR_CHUNK_BYTES)
        mV = max(int(offs[b1] - offs[b0]) for b0, b1 in chunks)
        mB = max(b1 - b0 for b0, b1 in chunks)
        if mV > self.capV or mB > self.capB:
            self._grow(mV, mB)
        e = self._entry(V, B)
        hin, hoffs, (pi, v, gpi, gv) = e["in"], e["offs"], e["out"]
        hin.numpy()[:V] = rows
        ho = hoffs.numpy()
        s = self.stream if self.stream is not None else torch.cuda.current_stream(w.device)
        nl = w.gnn.num_layers
        with torch.cuda.stream(s), ops.pinned_workspace(w.device, self.hws):
            for c, (b0, b1) in enumerate(chunks):
                v0, v1, n = int(offs[b0]), int(offs[b1]), b1 - b0
                o0 = b0 + c                       # this chunk's rebased offs in the host buffer
                ho[o0:o0 + n + 1] = offs[b0:b1 + 1] - v0
                co = hoffs[o0:o0 + n + 1]
                feat = self._features(hin[v0:v1], self.feat[:v1 - v0])
                # the leaf rows (the layer stack at L = 0 is the gather of every star's row 0)
                ops.gnn_star_batch_infer(feat, co, [], out=self.leaf[:n], ws=self.ws, stream=s)
                w.nnet.heads(self.leaf[:n], pi=pi[b0:b1], v=v[b0:b1])
                ops.gnn_star_batch_infer(feat, co, self.layers if nl else [], out=self.x0[:n],
                                         ws=self.ws, stream=s)
                nets.gnn_per_row_heads(w.nnet, w.gnn, self.x0[:n], pi=gpi[b0:b1], v=gv[b0:b1])
        ev = torch.cuda.Event()
        ev.record(s)
        return _PendingDirect(e, (pi, v, gpi, gv), ev, B)


# The exact route's own budget (args.batch_invariant).  Per packed row: its features (4 F) and its
# P row (2 H 4 = 1 KB); per star: TA (8 F), gate, u1, the next row 0, the leaf row, x0, hidden and
# y (4 F each), its Pt row and the TicTacToe head rows (2 x 2 KB); fixed: the exact GEMMs' slabs,
# which end at a row count (the projection's 3,968 rows x 14 segments x 1 KB = 57 MB at F = 3136,
# the tail's 256 rows x 11 segments x 12.5 KB = 35 MB) -- 128 MB covers every board.  At F = 3136
# that is 13.5 KB per row and 117 KB per star: 1 GiB holds about 3,800 stars of 9 boards.
STAR_EXACT_CHUNK_BYTES = 1 << 30


def _star_exact_chunk_cost(F):
    """(bytes per packed row, bytes per star, fixed bytes) of STAR_EXACT_CHUNK_BYTES' derivation."""
    return 4 * F + 1024 + 64, 36 * F + 1024 + 4096 + 256, 128 << 20


class _StarExactBatch:
    """predict_both_stars under args.batch_invariant, for one stream: ONE az_star_eval_exact_fwd
    call per chunk (trunk, row-0 gather, standard tail, the exact layer stack, output_transform,
    heads), packed stars read from and outputs written to mapped host memory (ops.HostBuffer, a
    ring so that several batches can be in flight, _PendingDirect's ownership tokens).  Device
    scratch is allocated once per capacity; a batch whose buffers would exceed
    STAR_EXACT_CHUNK_BYTES runs as consecutive chunks on the same scratch, which changes no bits:
    a star's rows are a function of the star alone."""

    def __init__(self, w, stream=None):
        self.w, self.stream = w, stream
        self.capV = self.capB = 0
        self.ring = []
        self.ev = None
        self.calls = []           # (B, V) of every chunk, newest last (tests read it)

    def _grow(self, V, B):
        w = self.w
        capV = max(self.capV, (V + 1023) // 1024 * 1024)
        capB = max(self.capB, (B + 255) // 256 * 256)
        torch.cuda.synchronize(w.device)          # in-flight batches may use the old scratch
        self.ev = ops.StarEvalExact(w.nnet.params, w.gnn.params, ops.exact_board(w.nnet),
                                    w.action_size, w.gnn.num_layers, capB, capV, w.device)
        self.capV, self.capB = capV, capB

    _entry = _StarBatch._entry

    def launch(self, rows, offs):
        w, F = self.w, self.w.feature_dim
        rows = np.asarray(rows)
        offs = np.asarray(offs, dtype=np.int64)
        B, V = len(offs) - 1, int(offs[-1])
        if B < 1 or offs[0] != 0 or V != rows.shape[0] or np.any(np.diff(offs) < 1):
            raise ValueError("predict_both_stars: offs must ascend from 0 to len(rows), one or "
                             "more rows per star")
        chunks = star_chunks(offs, F, STAR_EXACT_CHUNK_BYTES, _star_exact_chunk_cost(F))
        mV = max(int(offs[b1] - offs[b0]) for b0, b1 in chunks)
        mB = max(b1 - b0 for b0, b1 in chunks)
        if mV > self.capV or mB > self.capB:
            self._grow(mV, mB)
        e = self._entry(V, B)
        hin, hoffs, (pi, v, gpi, gv) = e["in"], e["offs"], e["out"]
        hin.numpy()[:V] = rows.reshape(V, hin.shape[1], hin.shape[2])
        ho = hoffs.numpy()
        s = self.stream if self.stream is not None else torch.cuda.current_stream(w.device)
        for c, (b0, b1) in enumerate(chunks):
            v0, v1, n = int(offs[b0]), int(offs[b1]), b1 - b0
            o0 = b0 + c                           # this chunk's rebased offs in the host buffer
            ho[o0:o0 + n + 1] = offs[b0:b1 + 1] - v0
            ops.star_eval_exact(self.ev, hin[v0:v1], hoffs[o0:o0 + n + 1], n, v1 - v0,
                                pi=pi[b0:b1], v=v[b0:b1], gpi=gpi[b0:b1], gv=gv[b0:b1], stream=s)
            self.calls.append((n, v1 - v0))
        del self.calls[:-4096]
        ev = torch.cuda.Event()
        ev.record(s)
        return _PendingDirect(e, (pi, v, gpi, gv), ev, B)


def _c4_shape(w):
    """(columns, rows) of a Connect4Net wrapper's board, None for another network.  Both extents
    count: a 7-column board that is not 7 rows high is NOT the 7x7 board of az_c4_*."""
    net = w.nnet
    if not isinstance(net, nets.Connect4Net):
        return None
    return (getattr(net, "board_x", net.n), getattr(net, "board_y", net.n))


def _is_c4(w):
    return _c4_shape(w) == (7, 7)


def _is_ttt(w):
    return isinstance(w.nnet, nets.TicTacToeNet) and 3 <= w.nnet.n <= 5


def _is_c4n(w):
    s = _c4_shape(w)
    return s is not None and s[0] == s[1] and s[0] in ops.C4N_SIDES


def _is_c4r(w):
    """The rectangular Connect4 boards with a fused trunk and az_c4r_eval_fwd."""
    return _c4_shape(w) in ops.C4R_SHAPES


def _direct_ok(w):
    """az_c4_eval_fwd covers the 7x7 Connect4Net (+ PolicyValueGNN output_transform),
    az_c4n_eval_fwd the Connect4Net on 4x4, 5x5, 6x6 and 8x8 boards, az_c4r_eval_fwd the one on
    7x6, 6x5, 5x4 and 8x7 boards, az_ttt_eval_fwd the TicTacToeNet on 3x3 .. 5x5 boards.  Every
    other shape (9x9, 4x6, ...) takes the hipGraph / pinned-ring routes."""
    return (os.environ.get("AZ_B1_MODE", "direct") == "direct"
            and (_is_c4(w) or _is_c4n(w) or _is_c4r(w) or _is_ttt(w))
            and os.environ.get("AZ_NO_ZEROCOPY", "0") in ("", "0"))


def _graphs_enabled():
    return os.environ.get("AZ_NO_GRAPH", "0") in ("", "0")


def check_star_depth(who, num_layers, args):
    """The packed-star kernels (az_gnn_star_batch_infer / _fwd_train / _bwd) take at most
    ops.STAR_MAX_LAYERS layers, and the two keys that route self-play or training through them
    have no other route: rejected up front, like the action size, instead of after a self-play
    iteration (train()) or inside the first lock-step round."""
    for key in ("gnn_neighbors_train", "gnn_neighbors_lockstep"):
        if int(num_layers) > ops.STAR_MAX_LAYERS and nets._args_get(args, key, False):
            raise ValueError(f"{who}: gnn_layers={int(num_layers)} > {ops.STAR_MAX_LAYERS}, the "
                             f"most the packed-star kernels take, cannot be combined with {key}")


class NetWrapper:
    """Common body; subclasses choose the board network class and whether a GNN exists."""

    net_class = None
    has_gnn = False
    makedirs_on_save = True

    MAX_ACTIONS = 32      # the heads kernels keep a wave's A+1 weight chunks in registers

    def __init__(self, game, args):
        A = game.getActionSize()
        if A > self.MAX_ACTIONS:
            # rejected up front: MCTS would otherwise swallow every predict's error and play
            # a whole iteration on uniform priors before train() fails (MCTS.py:195-200)
            raise ValueError(f"{type(self).__name__}: action size {A} > {self.MAX_ACTIONS} is "
                             f"not supported by the HIP heads kernels (board {game.getBoardSize()})")
        self.device = nets.default_device()
        self.game = game          # the training stars of gnn_neighbors_train are built from it
        self.nnet = self.net_class(game, args, device=self.device)
        self.board_x, self.board_y = game.getBoardSize()
        self.action_size = game.getActionSize()
        self.args = args
        if self.has_gnn:
            self.feature_dim = self.nnet.feature_dim
            num_layers = nets._args_get(args, "gnn_layers", 2)
            check_star_depth(type(self).__name__, num_layers, args)
            self.gnn = nets.PolicyValueGNN(self.feature_dim, num_layers, device=self.device)
        self.train_seed = 0
        self.batch_invariant = bool(nets._args_get(args, "batch_invariant", False))
        if self.batch_invariant and ops.exact_board(self.nnet) is None:
            # rejected up front, like the action size: MCTS swallows a predict's error
            raise ValueError(f"{type(self).__name__}: batch_invariant needs a board with a fused "
                             f"trunk (Connect4 7x7, 4x4, 5x5, 6x6, 8x8, 7x6, 6x5, 5x4, 8x7; "
                             f"TicTacToe 3x3 .. 5x5), not {game.getBoardSize()}")

    # -- evaluation ------------------------------------------------------------------------
    def _sync_params(self):
        """FlatParams.sync for both nets: the batch-1 and lock-step paths read the weights by
        pointer, so torch-side writes are announced here before they run."""
        self.nnet.params.sync()
        if self.has_gnn:
            self.gnn.params.sync()

    def _exact(self, boards, kind, stream=None):
        """args.batch_invariant: queue `boards` on the exact route (_ExactBatch, one per stream);
        .result() -> (pi, v, gpi, gv), None where `kind` ("std", "gnn", "both") has none."""
        self._sync_params()
        self.nnet.eval()
        if self.has_gnn:
            self.gnn.eval()
        directs = self.__dict__.setdefault("_exact_directs", {})
        key = None if stream is None else stream.cuda_stream
        d = directs.get(key)
        if d is None:
            d = directs[key] = _ExactBatch(self, stream)
        return d.launch(boards, kind == "both", kind)

    def _graph1(self, kind):
        """The batch-1 graph of `kind`, captured on first use (None when disabled)."""
        if self.batch_invariant:
            return _ExactBatch1(self, kind)
        self._sync_params()
        if not _graphs_enabled():
            return None
        g = getattr(self, "_g1", None)
        if g is None:
            g = self._g1 = {}
        if kind not in g:
            self.nnet.eval()
            if self.has_gnn:
                self.gnn.eval()
            if _direct_ok(self):
                cls = (_TttBatch1Direct if _is_ttt(self) else
                       _C4nBatch1Direct if _is_c4n(self) else
                       _C4rBatch1Direct if _is_c4r(self) else _Batch1Direct)
                g[kind] = cls(self, kind, cap=8 if kind == "both" else 1)
            else:
                g[kind] = _Batch1Graph(self, kind)
        return g[kind]

    def _eval(self, boards, gnn):
        b = boards_to_device(boards, self.device)
        if b.dim() == 2:
            b = b.view(1, self.board_x, self.board_y)
        f = self.nnet.features(b)
        if gnn:
            _, pi, v = nets.gnn_per_row_heads(self.nnet, self.gnn, f)
            return pi, v
        _, pi, v = self.nnet.heads(f)
        return pi, v

    def predict(self, board, neighbor_states=None):
        """Net.predict: (pi float32[A], v float32) for one canonical board
        (Connect4GNN.py:59-84; `neighbor_states` is accepted and unused as in
        Connect4Net.py:110)."""
        self.nnet.eval()
        if self.batch_invariant:
            pi, v, _, _ = self._exact(np.asarray(board)[None], "std").result()
            return pi[0], v[0]
        g = self._graph1("std")
        if g is not None:
            out = g.run(board)
            return out[:-1], out[-1]
        pi, v = self._eval(board, False)
        out = torch.cat([pi[0], v]).cpu().numpy()
        return out[:-1], out[-1]

    def predict_batch(self, boards):
        """Row-wise predict for [B,cols,rows] boards -> (pi float32[B,A], v float32[B])."""
        self.nnet.eval()
        if self.batch_invariant and len(boards) > 0:
            pi, v, _, _ = self._exact(boards, "std").result()
            return pi, v
        if len(boards) == 1 and (g := self._graph1("std")) is not None:
            out = g.run(boards[0])
            return out[None, :-1], out[-1:]
        pi, v = self._eval(boards, False)
        return pi.cpu().numpy(), v.cpu().numpy()

    def _launch(self, boards, both, stream=None):
        """Queue a batched prediction; returns a PendingPrediction (see predict_*_async).
        stream: run it on that HIP stream with its own device scratch (the lock-step lanes give
        each lane a stream, so one lane's batch can overlap the other's on the GPU); the caller
        orders the stream after any parameter update (play_episodes_engine does)."""
        if self.batch_invariant and len(boards) > 0:
            return self._exact(boards, "both" if both else "std", stream)
        self._sync_params()
        if (self.has_gnn or _is_ttt(self) or _is_c4n(self) or _is_c4r(self)) \
                and _direct_ok(self) \
                and len(boards) > 0:
            directs = self.__dict__.setdefault("_directs", {})
            key = None if stream is None else stream.cuda_stream
            d = directs.get(key)
            if d is None:
                cls = (_TttDirectBatch if _is_ttt(self) else
                       _C4nDirectBatch if _is_c4n(self) else
                       _C4rDirectBatch if _is_c4r(self) else _DirectBatch)
                d = directs[key] = cls(self, stream)
            self.nnet.eval()
            if self.has_gnn:
                self.gnn.eval()
            return d.launch(boards, both)
        if not hasattr(self, "_ring"):
            self._ring = _PinnedRing()
        boards = np.asarray(boards)
        n = boards.shape[0]
        A = self.action_size
        hb = self._ring.get("in", (n,) + boards.shape[1:], torch.int8)
        hb[:n].numpy()[...] = boards
        b = hb[:n].to(self.device, non_blocking=True)
        self.nnet.eval()
        f = self.nnet.features(b)
        _, pi, v = self.nnet.heads(f)
        if both:
            self.gnn.eval()
            _, gpi, gv = nets.gnn_per_row_heads(self.nnet, self.gnn, f)
            out = torch.cat([pi, v[:, None], gpi, gv[:, None]], dim=1)
        else:
            out = torch.cat([pi, v[:, None]], dim=1)
        ho = self._ring.get("out", tuple(out.shape), torch.float32)
        ho[:n].copy_(out, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring.advance()
        return PendingPrediction(ho, ev, n, A, both)

    def predict_batch_async(self, boards):
        """predict_batch without waiting: .result() -> (pi, v, None, None)."""
        return self._launch(boards, False)

    def save_checkpoint(self, folder, filename):
        if self.makedirs_on_save and not os.path.exists(folder):
            os.makedirs(folder)
        filepath = os.path.join(folder, filename) if self.has_gnn else folder + "/" + filename
        payload = {"state_dict": self.nnet.params.cpu_state_dict()}
        if self.has_gnn:
            payload["gnn"] = self.gnn.params.cpu_state_dict()
        torch.save(payload, filepath)

    def load_checkpoint(self, folder, filename):
        filepath = os.path.join(folder, filename) if self.has_gnn else folder + "/" + filename
        checkpoint = torch.load(filepath, map_location="cpu", weights_only=True)
        self.nnet.load_state_dict(checkpoint["state_dict"])
        if self.has_gnn:
            if "gnn" in checkpoint:
                self.gnn.load_state_dict(checkpoint["gnn"])
            else:
                print(f"GNN state not found in {filepath}, initializing new GNN")

    # -- training --------------------------------------------------------------------------
    def _cnn_batch(self, examples):
        batch_idx = np.random.randint(0, len(examples), min(len(examples), self.args.batch_size))
        boards, pis, vs = list(zip(*[examples[i] for i in batch_idx]))
        return (_dev_array(boards, np.int8, self.device),
                _dev_array(pis, np.float32, self.device),
                _dev_array(np.array(vs).astype(np.float64), np.float32, self.device))

    def _gnn_draw(self, gnn_examples):
        batch_idx = np.random.randint(0, len(gnn_examples),
                                      min(len(gnn_examples), self.args.batch_size))
        batch = [gnn_examples[i] for i in batch_idx]
        boards = [b for b, _, _, _, _, _, _ in batch]
        pis = [p for _, _, _, _, p, _, _ in batch]
        vs = [v for _, _, _, _, _, v, _ in batch]
        return (boards, _dev_array(pis, np.float32, self.device),
                _dev_array(np.array(vs).astype(np.float64), np.float32, self.device))

    def _gnn_batch(self, gnn_examples):
        boards, pis, vs = self._gnn_draw(gnn_examples)
        return _dev_array(boards, np.int8, self.device), pis, vs

    def _gnn_star_batch(self, gnn_examples):
        """_gnn_batch's draw (the same np.random call) with every sampled board expanded into its
        child star: (rows int8 [V,cols,rows], offs int32 [B+1], pis, vs) on the device."""
        import stars
        boards, pis, vs = self._gnn_draw(gnn_examples)
        rows, offs = stars.board_stars(self.game, boards)
        return (_dev_array(rows, np.int8, self.device),
                torch.from_numpy(np.ascontiguousarray(offs, np.int32)).to(self.device), pis, vs)

    def _train(self, examples, gnn_examples=None):
        """Connect4GNN.py:122-197: fresh Adam per call, `epochs` x (CNN step on a batch sampled
        with replacement by np.random.randint; GNN step on a second sample)."""
        lr = self.args.lr
        self._sync_params()
        # args.log_losses: the (l_pi, l_v) every step already forms on the device go into one slot
        # per epoch and are read once after the last epoch (no per-epoch host read); without the
        # key nothing is allocated and the launches are the ones of a run without it
        keep = bool(nets._args_get(self.args, "log_losses", False))
        if keep:
            lbuf = torch.zeros((self.args.epochs, 4), device=self.device)
            cnn_ran, gnn_ran = [False] * self.args.epochs, [False] * self.args.epochs
        cnn_split = False
        if (nets._args_get(self.args, "train_parallel", "replicas") == "auto"
                and getattr(self, "_tp_auto", None) is None):
            from . import dist as D
            if D.world_rank()[0] > 1:
                self._tp_auto, self.train_parallel_probe = self._probe_train_parallel(
                    examples, gnn_examples)
        self.nnet.params.reset_adam()
        if self.has_gnn:
            self.gnn.params.reset_adam()
        for epoch in range(self.args.epochs):
            self.nnet.train()
            if self.has_gnn:
                self.gnn.train()
            loss = gloss = None
            if examples:
                b, p, v = self._cnn_batch(examples)
                self.train_seed += 1
                if self._dp_world() > 1:
                    # the rows are split over the ranks: this is this rank's rows' part of the
                    # loss (normalised by the global batch); the parts are summed once, below
                    loss = self._cnn_step_allreduce(b, p, v, lr)
                    cnn_split = True
                    if keep:
                        cnn_ran[epoch] = True     # a rank without rows adds nothing to the sum
                else:
                    loss = T.cnn_step(self.nnet, b, p, v, lr, seed=self.train_seed)
            if (self.has_gnn and gnn_examples and len(gnn_examples) > 0
                    and nets._args_get(self.args, "gnn_neighbors_train", False)):
                # every example on its own child star; deterministic, so it runs whole on every
                # rank in every train_parallel mode and the replicas stay equal
                rows, offs, p, v = self._gnn_star_batch(gnn_examples)
                self.train_seed += 1
                gloss = T.gnn_star_step(self.nnet, self.gnn, rows, offs, p, v, lr,
                                        seed=self.train_seed)
            elif self.has_gnn and gnn_examples and len(gnn_examples) > 0:
                b, p, v = self._gnn_batch(gnn_examples)
                self.train_seed += 1
                if self._dp_world() > 1:
                    gloss = T.gnn_step_dp(self.nnet, self.gnn, b, p, v, lr, seed=self.train_seed,
                                          grad_sync=nets._args_get(self.args, "gnn_grad_sync",
                                                                   "row0"))
                else:
                    gloss = T.gnn_step(self.nnet, self.gnn, b, p, v, lr, seed=self.train_seed)
            if keep and loss is not None:
                lbuf[epoch, 0:2].copy_(loss)
                cnn_ran[epoch] = True
            if keep and gloss is not None:
                lbuf[epoch, 2:4].copy_(gloss)
                gnn_ran[epoch] = True
        if keep and cnn_split:
            # train_parallel = "allreduce": one all_reduce of every epoch's CNN loss parts, queued
            # behind the last step (only under the key; the steps' own collectives are untouched)
            from . import dist as D
            parts = lbuf[:, 0:2].contiguous()
            D.allreduce_sum_(parts)
            lbuf[:, 0:2].copy_(parts)
        torch.cuda.current_stream().synchronize()
        if keep:
            from . import metrics
            self.last_train_losses = metrics.train_losses(lbuf, cnn_ran, gnn_ran)

    def evaluate(self, examples, gnn_examples=None, chunk=4096):
        """The losses of the network on `examples` ((board, pi, v) tuples, as train() takes
        them) without training on them -> {loss_pi, loss_v, loss, top1, entropy, target_entropy,
        n}: loss_pi = mean -sum(pi log p), loss_v = mean (v - z)^2, loss their sum (the quantity
        train() minimises), top1 the share of rows whose argmax p is argmax pi, the two entropies
        in nats, n the row count; all zeros for no examples.  On a GNN wrapper `gnn_examples`
        (Coach's seven fields; board, expanded_pi and expanded_v are read) add gnn_* -- the GNN
        outputs against expanded_pi / expanded_v -- and std_on_gnn_* -- the standard heads on the
        same boards against the same targets, from the same forward -- so that their difference
        is what the GNN buys.  The outputs are the search's: eval mode, the per-board route of
        predict_both on a batch (the exact one under args.batch_invariant); under
        args.gnn_neighbors the gnn_examples' boards are scored with their child stars
        (stars.board_stars, predict_both_stars), the standard block's boards -- whose outputs
        no star changes -- stay on the per-board route.  `chunk` boards are evaluated at a time
        and scored by az_policy_value_metrics into accumulators on the device, read once at the
        end (azhip/metrics.py).  Draws no random number, writes no parameter, optimiser state or
        train_seed, leaves the training flags as they were; under a process group every rank
        computes the whole result."""
        from . import metrics
        return metrics.evaluate_wrapper(self, examples, gnn_examples, chunk)

    def _dp_world(self):
        """>1 when the train steps are data-parallel over ranks (args.train_parallel ==
        "allreduce" under torch.distributed: CNN rows split + gradient all_reduce, the GNN step
        as train.gnn_step_dp); "replicas" (default) runs them whole everywhere; "auto" is
        whichever _probe_train_parallel measured faster on this process group."""
        from . import dist as D
        mode = nets._args_get(self.args, "train_parallel", "replicas")
        if mode == "auto":
            mode = getattr(self, "_tp_auto", None) or "replicas"
        if mode != "allreduce":
            return 1
        return D.world_rank()[0]

    def _probe_train_parallel(self, examples, gnn_examples):
        """train_parallel="auto" ('choose by measurement'): before the first
        train() under a process group of P > 1 ranks, time one gradient computation each way on
        this node -- the whole batch on every rank (replicas) against the data-parallel form
        with its collectives (the CNN rows sharded + the 188 KB all_reduce; the GNN step's
        sharded trunk, gathered features and the 78.7 MB output_transform all_reduce, or the
        478.6 MB one for gnn_grad_sync="flat") -- and keep the faster.  The Adam step is the same
        in both modes, so it is not timed.  The probe uses the first batch_size examples (no
        np.random draw: the training batches stay the reference's) and only writes gradient
        buffers, which every step overwrites.  Times are max over ranks, so every rank makes the
        same choice.  Returns (choice, {timings in ms})."""
        import time
        import torch.distributed as dist
        from . import dist as D
        world, rank = D.world_rank()
        sync = nets._args_get(self.args, "gnn_grad_sync", "row0")
        n = self.args.batch_size
        # every rank must probe the same jobs (each runs barriers and an all_reduce sized by
        # the job list): keep the kinds of examples every rank holds
        have = torch.tensor([1.0 if examples else 0.0,
                             1.0 if (self.has_gnn and gnn_examples) else 0.0],
                            dtype=torch.float64, device=self.device)
        dist.all_reduce(have, op=dist.ReduceOp.MIN)
        if have[0].item() == 0.0:
            examples = []
        if have[1].item() == 0.0:
            gnn_examples = []
        jobs = {}
        if examples:
            sel = examples[:n]
            b = _dev_array([e[0] for e in sel], np.int8, self.device)
            p = _dev_array([e[1] for e in sel], np.float32, self.device)
            v = _dev_array(np.array([e[2] for e in sel]).astype(np.float64), np.float32,
                           self.device)
            Bg = b.shape[0]
            r0, r1 = D.row_shard(Bg, world, rank)

            def cnn_dp():
                T.cnn_grads(self.nnet, b[r0:r1], p[r0:r1], v[r0:r1], seed=1, B_norm=Bg)
                D.allreduce_sum_(self.nnet.params.grad_flat)

            jobs["cnn"] = (lambda: T.cnn_grads(self.nnet, b, p, v, seed=1), cnn_dp)
        if self.has_gnn and gnn_examples:
            sel = gnn_examples[:n]
            gb = _dev_array([e[0] for e in sel], np.int8, self.device)
            gp = _dev_array([e[4] for e in sel], np.float32, self.device)
            gv = _dev_array(np.array([e[5] for e in sel]).astype(np.float64), np.float32,
                            self.device)
            jobs["gnn"] = (lambda: T.gnn_grads(self.nnet, self.gnn, gb, gp, gv, seed=1),
                           lambda: T.gnn_grads_dp(self.nnet, self.gnn, gb, gp, gv, seed=1,
                                                  grad_sync=sync))

        def timed(fn, reps=3):
            fn()                                      # first call: allocations, workspaces
            ts = []
            for _ in range(reps):
                dist.barrier()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)) * 1e3

        names, vals = [], []
        for k, (rep, dp) in jobs.items():
            names += [f"{k}_replicas_ms", f"{k}_allreduce_ms"]
            vals += [timed(rep), timed(dp)]
        t = torch.tensor(vals, dtype=torch.float64, device=self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        res = dict(zip(names, [round(float(x), 4) for x in t.tolist()]))
        rep_ms = sum(res[k] for k in names if k.endswith("_replicas_ms"))
        dp_ms = sum(res[k] for k in names if k.endswith("_allreduce_ms"))
        res.update(world=world, gnn_grad_sync=sync)
        return ("allreduce" if dp_ms < rep_ms else "replicas"), res

    def _cnn_step_allreduce(self, b, p, v, lr):
        """CNN step with the sampled rows split over ranks: each rank's loss is normalised by
        the GLOBAL batch, the flat gradient is summed with one all_reduce (RCCL), then every
        rank applies the identical Adam step.  The dropout mask is the global batch's mask
        (same counter-based seed), sliced to this rank's rows."""
        from . import dist as D
        world, rank = D.world_rank()
        Bg = b.shape[0]
        r0, r1 = D.row_shard(Bg, world, rank)
        F = self.nnet.feature_dim
        drop = float(getattr(self.nnet, "dropout", 0.0)) \
            if isinstance(self.nnet, nets.Connect4Net) else 0.0
        mask = None
        if drop > 0.0:
            mask = ops.dropout_mask(Bg * F, drop, self.train_seed, self.device)[r0 * F:r1 * F]
        P = self.nnet.params
        if r1 > r0:
            loss = T.cnn_grads(self.nnet, b[r0:r1], p[r0:r1], v[r0:r1], seed=self.train_seed,
                               drop_mask=mask, B_norm=Bg)
        else:
            P.grad_flat.zero_()
            loss = None
        D.allreduce_sum_(P.grad_flat)
        T.adam_step(self.nnet, lr)
        return loss

    def snapshot(self):
        """Device copy of every parameter buffer (Coach's temp checkpoint, in memory)."""
        snap = {"nnet": self.nnet.params.flat.clone()}
        if self.has_gnn:
            snap["gnn"] = self.gnn.params.flat.clone()
        return snap

    def restore(self, snap):
        self.nnet.params.copy_flat_(snap["nnet"])
        if self.has_gnn:
            self.gnn.params.copy_flat_(snap["gnn"])


class GNNWrapperMixin:
    """predict / predict_with_gnn pair of the GNN wrappers (Connect4GNN.py:59-120)."""

    has_gnn = True

    @property
    def batch_invariant_rows(self):
        """Largest batch whose predict_both rows are bit-identical to batch-1 calls: the 7x7
        Connect4 evaluator (az_c4_eval_fwd), the one for 4x4, 5x5, 6x6 and 8x8 boards
        (az_c4n_eval_fwd), the one for 7x6, 6x5, 5x4 and 8x7 boards (az_c4r_eval_fwd) and the
        TicTacToe one (az_ttt_eval_fwd, n = 3..5) compute every row of a batch of <= 8 with the
        batch-1 arithmetic (tests/test_gpu_selfplay.py, tests/test_gpu_c4n_eval.py,
        tests/test_gpu_c4r_eval.py, tests/test_gpu_ttt_eval.py); 0 = no such guarantee.  Under
        args.batch_invariant every entry point is az_eval_exact_fwd, invariant at any batch size
        (tests/test_gpu_exact.py): 1 << 30."""
        if self.batch_invariant:
            return 1 << 30
        return 8 if _direct_ok(self) else 0

    @property
    def batch_invariant_stars(self):
        """True when the star entry points (predict_with_gnn with neighbours, predict_star_batch,
        predict_both_stars) are batch-invariant too: args.batch_invariant is set and the GNN has
        at most ops.STAR_MAX_LAYERS layers, the most az_star_eval_exact_fwd takes.  Coach accepts
        batch_invariant with gnn_neighbors only for a network that says so."""
        return bool(self.batch_invariant and self.gnn.num_layers <= ops.STAR_MAX_LAYERS)

    def _exact_stars(self, rows, offs, stream=None):
        """args.batch_invariant: queue packed stars on the exact route (_StarExactBatch, one per
        stream); .result() -> (pi, v, gpi, gv).  Never another route: more layers than the exact
        evaluator takes is an error."""
        if not self.batch_invariant_stars:
            raise ValueError(f"{type(self).__name__}: batch_invariant evaluates stars through "
                             f"az_star_eval_exact_fwd, which takes at most {ops.STAR_MAX_LAYERS} "
                             f"GNN layers, not {self.gnn.num_layers}")
        self.nnet.eval()
        self.gnn.eval()
        self._sync_params()
        batches = self.__dict__.setdefault("_star_exact_batches", {})
        key = None if stream is None else stream.cuda_stream
        d = batches.get(key)
        if d is None:
            d = batches[key] = _StarExactBatch(self, stream)
        self.star_route = "exact"
        return d.launch(rows, offs)

    def predict(self, board):
        return NetWrapper.predict(self, board)

    def _star_direct_ok(self):
        """The one-call star evaluator (az_c4_star_eval_fwd) serves Connect4 boards with a fused
        trunk; AZ_B1_MODE=graph or AZ_NO_ZEROCOPY=1 select the composition, as they select the
        older routes elsewhere."""
        s = _c4_shape(self)
        return (s is not None and ops.star_shape_ok(s)
                and self.gnn.num_layers <= ops.STAR_MAX_LAYERS
                and os.environ.get("AZ_B1_MODE", "direct") == "direct"
                and os.environ.get("AZ_NO_ZEROCOPY", "0") in ("", "0"))

    def _ttt_star_direct_ok(self):
        """The one-call TicTacToe star evaluator (az_ttt_star_eval_fwd) serves 3x3 .. 5x5 boards
        under args.gnn_neighbors, the key of the mode that evaluates stars at inference: without
        the key every route is what it was.  AZ_B1_MODE=graph or AZ_NO_ZEROCOPY=1 select the
        composition, as they do for Connect4."""
        return (_is_ttt(self) and ops.ttt_star_shape_ok(self.nnet.n)
                and bool(nets._args_get(self.args, "gnn_neighbors", False))
                and self.gnn.num_layers <= ops.STAR_MAX_LAYERS
                and os.environ.get("AZ_B1_MODE", "direct") == "direct"
                and os.environ.get("AZ_NO_ZEROCOPY", "0") in ("", "0"))

    def _star_compose(self, node_lists):
        """Any number of stars of any size on any wrapper: the trunk on every board, the layers on
        a forest-of-stars graph through the generic graph calls, output_transform and the heads on
        the row 0s.  No new kernel and no batch-invariance promise."""
        counts = tuple(len(nodes) for nodes in node_lists)
        boards = np.concatenate([np.asarray(nodes, dtype=np.int8).reshape(
            len(nodes), self.board_x, self.board_y) for nodes in node_lists])
        x = self.nnet.features(boards_to_device(boards, self.device))
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        if max(counts) > 1:
            cache = self.__dict__.setdefault("_star_graphs", {})
            g = cache.get(counts)
            if g is None:
                if len(cache) >= 64:
                    cache.clear()
                rowptr = np.full(sum(counts) + 1, 0, np.int64)
                col, e = [], 0
                for s, n in zip(starts, counts):
                    rowptr[s] = e
                    e += n - 1
                    rowptr[s + 1:s + n + 1] = e
                    col += list(range(s + 1, s + n))
                g = cache[counts] = ops.DeviceGraph(rowptr, np.asarray(col, np.int64),
                                                    self.device)
            self.gnn.params.sync()
            for layer in self.gnn.layers:
                x, self.gnn._ws = ops.gnn_layer(g, x, layer.weights(), ws=self.gnn._ws,
                                                save=False)
        rows0 = x[torch.as_tensor(starts, device=self.device)].contiguous()
        _, pi, v = nets.gnn_per_row_heads(self.nnet, self.gnn, rows0)
        out = torch.cat([pi, v[:, None]], dim=1).cpu().numpy()
        return out[:, :-1], out[:, -1]

    def predict_star_batch(self, node_lists):
        """GNN evaluation of B leaves with their neighbourhoods: node_lists[b] is the star
        [board] + neighbor_states of leaf b (canonical boards, row 0 the leaf).  Returns
        (gpi float32[B][A], gv float32[B]): the heads of row 0 after PolicyValueGNN.forward on
        each star (Connect4GNN.py:86-120 on a star instead of a 1-row input).  Connect4 boards
        with a fused trunk, <= 9 nodes and <= 8 stars take the one-call evaluator ("onecall",
        today's bits); under args.gnn_neighbors so do TicTacToe 3x3 .. 5x5 boards with <= n^2 + 1
        nodes and <= 8 stars (az_ttt_star_eval_fwd; without that key a TicTacToe star keeps the
        composition).  Under args.gnn_neighbors_lockstep -- the opt-in key of the batched mode;
        without it every route is what it was -- more than 8 stars, or a star of more than 9
        nodes, takes predict_both_stars on every wrapper ("batched").  What is left takes the
        composition (<= 8 small stars on another wrapper, or under AZ_B1_MODE=graph /
        AZ_NO_ZEROCOPY=1; without the key also every larger batch).  Under the key those two
        switches select nothing above 8 stars: measured end to end at 16 .. 2,048 stars of 8 nodes
        on 7x7, 7x6 and 4x4, the batched route beat the composition 1.17x - 3.4x, everywhere by
        more than the larger spread.  self.star_route names the route
        taken.  Under args.batch_invariant every call, of any number of stars of any size,
        with or without the lock-step key and whatever AZ_B1_MODE / AZ_NO_ZEROCOPY say, takes
        the exact star route ("exact"; ValueError when the GNN has more layers than it takes)."""
        self.nnet.eval()
        self.gnn.eval()
        self._sync_params()
        A = self.action_size
        if len(node_lists) == 0:
            return np.zeros((0, A), np.float32), np.zeros((0,), np.float32)
        if self.batch_invariant:
            rows = np.concatenate([np.asarray(nodes, dtype=np.int8).reshape(
                len(nodes), self.board_x, self.board_y) for nodes in node_lists])
            offs = np.concatenate([[0], np.cumsum([len(nodes) for nodes in node_lists])])
            _, _, gpi, gv = self._exact_stars(rows, offs).result()
            return gpi, gv
        small = (len(node_lists) <= ops.STAR_MAX_STARS
                 and max(len(nodes) for nodes in node_lists) <= ops.STAR_MAX_NODES)
        if self._star_direct_ok() and small:
            d = self.__dict__.get("_star_direct")
            if d is None:
                d = self._star_direct = _StarDirect(self)
            self.star_route = "onecall"
            return d.run(node_lists)
        if self._ttt_star_direct_ok() and len(node_lists) <= ops.STAR_MAX_STARS and \
                max(len(nodes) for nodes in node_lists) <= self.nnet.n ** 2 + 1:
            d = self.__dict__.get("_ttt_star_direct")
            if d is None:
                d = self._ttt_star_direct = _TttStarDirect(self)
            self.star_route = "onecall"
            return d.run(node_lists)
        if (not small and self.gnn.num_layers <= ops.STAR_MAX_LAYERS
                and nets._args_get(self.args, "gnn_neighbors_lockstep", False)):
            self.star_route = "batched"
            rows = np.concatenate([np.asarray(nodes, dtype=np.int8).reshape(
                len(nodes), self.board_x, self.board_y) for nodes in node_lists])
            offs = np.concatenate([[0], np.cumsum([len(nodes) for nodes in node_lists])])
            _, _, gpi, gv = self.predict_both_stars(rows, offs.astype(np.int32))
            return gpi, gv
        self.star_route = "composition"
        return self._star_compose(node_lists)

    def _star_batch(self, stream=None):
        batches = self.__dict__.setdefault("_star_batches", {})
        key = None if stream is None else stream.cuda_stream
        d = batches.get(key)
        if d is None:
            d = batches[key] = _StarBatch(self, stream)
        return d

    def predict_both_stars_async(self, rows, offs, stream=None):
        """predict_both_stars without waiting: .result() -> (pi, v, gnn_pi, gnn_v).  stream: run
        on that HIP stream with its own device scratch (the lock-step lanes give each lane one);
        the caller orders the stream after any parameter update."""
        if self.batch_invariant:
            return self._exact_stars(rows, offs, stream)
        self.nnet.eval()
        self.gnn.eval()
        self._sync_params()
        return self._star_batch(stream).launch(rows, offs)

    def predict_both_stars(self, rows, offs):
        """Standard and GNN predictions of B leaves with their neighbourhoods, the batched form of
        predict + predict_with_gnn(board, neighbor_states=...): rows int8 [V][cols][rows] packed
        stars, offs int32 [B+1] (star b = rows offs[b] .. offs[b+1]-1, row 0 the leaf; the layout
        of az_game_stars_rect).  One trunk pass over the V rows, the standard heads on the B leaf
        rows, az_gnn_star_batch_infer, output_transform and the heads on the row 0s; one host copy
        out -> (pi [B][A], v [B], gnn_pi [B][A], gnn_v [B]).  Rows are within 1e-5 of the
        batch-1 calls, not bit-identical to them, and a batch split by STAR_CHUNK_BYTES may differ
        in bits from the unsplit one (the GEMM dispatch chooses its tile by the row count).
        Under args.batch_invariant the call is az_star_eval_exact_fwd instead ("exact"): a star's
        four rows are the same bits alone, in any batch and however the batch is chunked, pi / v
        equal predict(leaf) and a one-row star's gnn_pi / gnn_v equal predict_with_gnn(leaf)."""
        return self.predict_both_stars_async(rows, offs).result()

    def predict_with_gnn(self, board, neighbor_states=None):
        """GNN-enhanced prediction.  Without neighbours: a 1-row input, so the message-passing
        layers are the identity (gnn_utils.py:35-36) and only output_transform runs before the
        heads.  With `neighbor_states` (a list of canonical boards, Connect4Net.py:110): the star
        [board] + neighbor_states goes through the layers and row 0 through the heads
        (predict_star_batch)."""
        if neighbor_states is not None and len(neighbor_states) > 0:
            pi, v = self.predict_star_batch([[board] + list(neighbor_states)])
            return pi[0], v[0]
        self.nnet.eval()
        self.gnn.eval()
        if self.batch_invariant:
            _, _, gpi, gv = self._exact(np.asarray(board)[None], "gnn").result()
            return gpi[0], gv[0]
        g = self._graph1("gnn")
        if g is not None:
            out = g.run(board)
            return out[:-1], out[-1]
        pi, v = self._eval(board, True)
        out = torch.cat([pi[0], v]).cpu().numpy()
        return out[:-1], out[-1]

    def predict_batch_with_gnn(self, boards):
        self.nnet.eval()
        self.gnn.eval()
        if self.batch_invariant and len(boards) > 0:
            _, _, gpi, gv = self._exact(boards, "gnn").result()
            return gpi, gv
        pi, v = self._eval(boards, True)
        return pi.cpu().numpy(), v.cpu().numpy()

    def predict_both(self, boards):
        """Standard and GNN predictions of a batch from ONE trunk pass (what MCTS.search asks
        for every new leaf, MCTS.py:169-174) -> (pi, v, gnn_pi, gnn_v), one host copy."""
        self.nnet.eval()
        self.gnn.eval()
        A = self.action_size
        if self.batch_invariant and len(boards) > 0:
            return self._exact(boards, "both").result()
        g = self._graph1("both") if len(boards) <= 8 else None
        if isinstance(g, _Batch1Direct) and len(boards) > 0:
            return g.run_rows(np.asarray(boards))
        if len(boards) == 1 and g is not None:
            out = g.run(boards[0])[None]
            return out[:, :A], out[:, A], out[:, A + 1:2 * A + 1], out[:, 2 * A + 1]
        b = boards_to_device(boards, self.device)
        f = self.nnet.features(b)
        _, pi, v = self.nnet.heads(f)
        _, gpi, gv = nets.gnn_per_row_heads(self.nnet, self.gnn, f)
        out = torch.cat([pi, v[:, None], gpi, gv[:, None]], dim=1).cpu().numpy()
        return out[:, :A], out[:, A], out[:, A + 1:2 * A + 1], out[:, 2 * A + 1]

    def predict_both_async(self, boards, stream=None):
        """predict_both without waiting: .result() -> (pi, v, gnn_pi, gnn_v)."""
        return self._launch(boards, True, stream)

    def train(self, examples, gnn_examples=None):
        self._train(examples, gnn_examples)

    def extract_features(self, board_tensor):
        """Connect4GNN.py:31-46 / TicTacToeGNN.py:25-34 on device boards.  As in the reference,
        the Connect4 features go through dropout while `nnet.training` is set (the mask comes
        from the counter-based device RNG, not torch's generator)."""
        b = boards_to_device(board_tensor, self.device)
        if b.dim() == 2:
            b = b.view(1, self.board_x, self.board_y)
        f = self.nnet.features(b)
        p = float(getattr(self.nnet, "dropout", 0.0)) if isinstance(self.nnet, nets.Connect4Net) \
            else 0.0
        if self.nnet.training and p > 0.0:
            self.train_seed += 1
            mask = ops.dropout_mask(f.numel(), p, self.train_seed, f.device)
            f = ops.mask_scale(f, mask, 1.0 / (1.0 - p))
        return f

    def apply_policy_value_heads(self, features):
        """Connect4GNN.py:48-57 / TicTacToeGNN.py:36-45: features [B,F] on HBM ->
        (log_pi [B,A], v [B,1])."""
        logp, _, v = self.nnet.heads(features.contiguous(), want_pi=False)
        return logp, v.view(-1, 1)


class CNNWrapperMixin:
    has_gnn = False

    def train(self, examples):
        self._train(examples, None)
