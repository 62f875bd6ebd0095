"""evaluate(): the losses of a network on a list of examples, without training on them.

The network outputs are the ones the search sees (eval mode, no dropout), scored chunk by chunk by
az_policy_value_metrics, which adds every chunk's sums to float64 accumulators on the device; the
accumulators are read once, after the last chunk.  Nothing in between waits for the device: the
targets go up in one copy before the first chunk, and a route that writes its outputs into mapped
host memory (the exact and the star evaluators) is scored from that memory by the kernel, its
staging held until the final read (so such a pass takes one ring entry of mapped host memory per
chunk -- a chunk's boards and outputs, about 0.5 MB at 4,096 7x7 boards, 25 entries for 100,000
examples -- which stay in the evaluator's ring as idle entries for later batches).  No random numbers are drawn and no parameter, optimiser state
or train_seed is written."""
import numpy as np
import torch

from . import nets, ops
from .nets import boards_to_device


class MetricSums:
    """`blocks` accumulators of ops.METRICS on the device: add() queues one
    az_policy_value_metrics call, read() is the pass's one device-to-host copy."""

    def __init__(self, device, blocks):
        self.acc = torch.zeros((blocks, len(ops.METRICS)), dtype=torch.float64, device=device)
        self.ws = torch.empty((1 << 16,), dtype=torch.uint8, device=device)
        self.hold = []            # predictions whose mapped host outputs a queued call reads

    def add(self, block, p, v, target_pi, target_v):
        ops.policy_value_metrics(p, v, target_pi, target_v, acc=self.acc[block], accumulate=True,
                                 ws=self.ws)

    def read(self):
        out = self.acc.cpu().numpy()
        self.hold.clear()         # the copy waited for every queued call
        return out


def _targets(pis, vs, A, device):
    """Example targets -> (pi fp32 [n][A], v fp32 [n]) on the device, one copy each, rounded as
    train() rounds them."""
    pi = np.ascontiguousarray(np.array(pis, dtype=np.float32).reshape(len(pis), A))
    v = np.ascontiguousarray(np.array(vs).astype(np.float64).astype(np.float32).reshape(-1))
    return torch.from_numpy(pi).to(device), torch.from_numpy(v).to(device)


def _outputs(w, boards, both, sums):
    """(pi, v, gpi, gv) of a chunk of boards on the per-board route predict_both takes on a batch
    (gpi / gv None unless `both`): device tensors, or views of mapped host memory under
    batch_invariant (az_eval_exact_fwd)."""
    n = len(boards)
    if w.batch_invariant:
        pend = w._exact(boards, "both" if both else "std")
        sums.hold.append(pend)
        return tuple(None if t is None else t[:n] for t in pend.views)
    w.nnet.eval()
    f = w.nnet.features(boards_to_device(boards, w.device))
    _, pi, v = w.nnet.heads(f)
    if not both:
        return pi, v, None, None
    w.gnn.eval()
    _, gpi, gv = nets.gnn_per_row_heads(w.nnet, w.gnn, f)
    return pi, v, gpi, gv


def _star_outputs(w, boards, sums):
    """(pi, v, gpi, gv) of a chunk of boards, each scored with its child star (stars.board_stars,
    predict_both_stars: the route gnn_neighbors_lockstep uses, az_star_eval_exact_fwd under
    batch_invariant); the call splits the chunk by its own star chunk limits.  Views of mapped
    host memory."""
    import stars
    rows, offs = stars.board_stars(w.game, list(boards))
    pend = w.predict_both_stars_async(rows, offs)
    sums.hold.append(pend)
    return tuple(t[:len(boards)] for t in pend.views)


def evaluate_wrapper(w, examples, gnn_examples=None, chunk=4096):
    """NetWrapper.evaluate (azhip/wrappers.py)."""
    chunk = max(1, int(chunk))
    examples = examples or []
    want_gnn = w.has_gnn and gnn_examples is not None
    gnn_examples = gnn_examples or []
    if gnn_examples and not w.has_gnn:
        raise ValueError(f"{type(w).__name__}.evaluate: gnn_examples need a GNN wrapper")
    A, shape = w.action_size, (w.board_x, w.board_y)
    modes = [w.nnet.training] + ([w.gnn.training] if w.has_gnn else [])
    use_stars = w.has_gnn and bool(nets._args_get(w.args, "gnn_neighbors", False))
    sums = MetricSums(w.device, 3)
    try:
        if examples:
            boards = np.ascontiguousarray(np.array([e[0] for e in examples]),
                                          dtype=np.int8).reshape((-1,) + shape)
            tpi, tv = _targets([e[1] for e in examples], [e[2] for e in examples], A, w.device)
            for c0 in range(0, len(boards), chunk):
                pi, v, _, _ = _outputs(w, boards[c0:c0 + chunk], False, sums)
                sums.add(0, pi, v, tpi[c0:c0 + chunk], tv[c0:c0 + chunk])
        if gnn_examples:
            boards = np.ascontiguousarray(np.array([e[0] for e in gnn_examples]),
                                          dtype=np.int8).reshape((-1,) + shape)
            tpi, tv = _targets([e[4] for e in gnn_examples], [e[5] for e in gnn_examples], A,
                               w.device)
            for c0 in range(0, len(boards), chunk):
                b = boards[c0:c0 + chunk]
                pi, v, gpi, gv = _star_outputs(w, b, sums) if use_stars \
                    else _outputs(w, b, True, sums)
                sums.add(1, gpi, gv, tpi[c0:c0 + chunk], tv[c0:c0 + chunk])
                sums.add(2, pi, v, tpi[c0:c0 + chunk], tv[c0:c0 + chunk])
        host = sums.read()
    finally:
        sums.hold.clear()
        w.nnet.train(modes[0])
        if w.has_gnn:
            w.gnn.train(modes[1])
    out = ops.metrics_dict(host[0])
    if want_gnn:
        out.update(ops.metrics_dict(host[1], "gnn_"))
        out.update(ops.metrics_dict(host[2], "std_on_gnn_"))
    return out


def train_losses(buf, cnn_ran, gnn_ran):
    """The [epochs][4] device buffer train() filled under log_losses (l_pi, l_v of the CNN step,
    then of the GNN step) -> one dict per epoch with the keys of the steps that stored their loss
    (cnn_ran[e] / gnn_ran[e]); the one host read of the buffer."""
    rows = buf.cpu().numpy().astype(np.float64)
    out = []
    for e, (lp, lv, gp, gv) in enumerate(rows):
        d = {"epoch": e}
        if cnn_ran[e]:
            d.update(loss_pi=float(lp), loss_v=float(lv), loss=float(lp + lv))
        if gnn_ran[e]:
            d.update(gnn_loss_pi=float(gp), gnn_loss_v=float(gv), gnn_loss=float(gp + gv))
        out.append(d)
    return out
