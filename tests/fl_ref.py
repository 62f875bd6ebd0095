"""A plain-torch restatement of FrozenLakeNet (not a test module), written from the formulas in
include/az_hip.h and the header of csrc/az_fl.hip: no azhip import, no collapsed form.  It runs
in float64 (the yardstick) and in float32 (whose deviation from float64 sets the widened bars).
tests/test_fl_ref.py holds it to the committed goldens on the CPU before any GPU test uses it.

Per leaf b with n = counts[b] node rows x_j:
  h_j = relu(fe2 relu(fe0 x_j));   L times  h <- relu(A_n (W_l h + b_l)),
  A_n = D^-1/2 1 1^T D^-1/2 (the n x n all-ones adjacency, D its row sums);
  pi = softmax(policy_head h[0]);  v = tanh(value_head h[0])
loss = -sum(tpi log(clamp(pi, min=1e-8))) / B + sum((v - tv)^2) / B
clip: clip_grad_norm_(max_norm) semantics, coef = min(max_norm / (norm + 1e-6), 1)."""
import numpy as np
import torch
import torch.nn.functional as Fn

PI_MIN = 1e-8


def spec(S, E, L, A=4, H=128):
    """(name, shape) in state_dict order."""
    out = [("feature_extractor.0.weight", (H, S)), ("feature_extractor.0.bias", (H,)),
           ("feature_extractor.2.weight", (E, H)), ("feature_extractor.2.bias", (E,))]
    for i in range(L):
        out += [(f"gnn_layers.{i}.W.weight", (E, E)), (f"gnn_layers.{i}.W.bias", (E,))]
    return out + [("policy_head.weight", (A, E)), ("policy_head.bias", (A,)),
                  ("value_head.weight", (1, E)), ("value_head.bias", (1,))]


def num_layers(W):
    return sum(1 for k in W if k.startswith("gnn_layers.") and k.endswith(".W.weight"))


def params(W, dtype=torch.float64, requires_grad=False):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(requires_grad)
            for k, v in W.items()}


def adjacency(n, dtype):
    A = torch.ones((n, n), dtype=dtype)
    d = A.sum(1).pow(-0.5)
    return d[:, None] * A * d[None, :]


def forward(P, nodes, counts, trace=None):
    """pi [B][4], v [B] and u [B] (the value pre-activation) of leaves nodes [B][5][S], of which
    the first counts[b] rows of leaf b are read.  `trace`, a list, receives per leaf the row-0
    activations after the feature extractor and after every layer."""
    dt = P["policy_head.weight"].dtype
    L = num_layers(P)
    nodes = np.asarray(nodes)
    pis, vs, us = [], [], []
    for b in range(len(counts)):
        n = int(counts[b])
        x = torch.as_tensor(nodes[b, :n]).to(dt)
        h = Fn.relu(Fn.linear(x, P["feature_extractor.0.weight"], P["feature_extractor.0.bias"]))
        h = Fn.relu(Fn.linear(h, P["feature_extractor.2.weight"], P["feature_extractor.2.bias"]))
        An = adjacency(n, dt)
        acts = [h[0].detach()]
        for l in range(L):
            h = Fn.relu(An @ Fn.linear(h, P[f"gnn_layers.{l}.W.weight"],
                                       P[f"gnn_layers.{l}.W.bias"]))
            acts.append(h[0].detach())
        if trace is not None:
            trace.append(acts)
        u = Fn.linear(h[0], P["value_head.weight"], P["value_head.bias"])[0]
        pis.append(torch.softmax(Fn.linear(h[0], P["policy_head.weight"], P["policy_head.bias"]),
                                 0))
        vs.append(torch.tanh(u))
        us.append(u)
    return torch.stack(pis), torch.stack(vs), torch.stack(us)


def loss_of(pi, v, tpi, tv):
    B = pi.shape[0]
    tpi = torch.as_tensor(np.asarray(tpi)).to(pi.dtype)
    tv = torch.as_tensor(np.asarray(tv)).to(pi.dtype)
    return -(tpi * torch.log(pi.clamp(min=PI_MIN))).sum() / B + ((v - tv) ** 2).sum() / B


def clip(grads, max_norm=1.0):
    """(total norm, clipped copies) of a dict of numpy gradients, in their dtype."""
    ts = [torch.as_tensor(g) for g in grads.values()]
    norm = torch.sqrt(sum((t ** 2).sum() for t in ts))
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return float(norm), {k: (torch.as_tensor(g) * coef).numpy() for k, g in grads.items()}


def grads(W, nodes, counts, tpi, tv, dtype=torch.float64):
    """One training batch by autograd -> dict(loss, grads, dlogits [B][4], pi, v, u)."""
    P = params(W, dtype, requires_grad=True)
    pi, v, u = forward(P, nodes, counts)
    pi.retain_grad()
    loss = loss_of(pi, v, tpi, tv)
    loss.backward()
    p, gp = pi.detach(), pi.grad
    dlogits = p * (gp - (gp * p).sum(1, keepdim=True))           # softmax backward
    return {"loss": float(loss.detach()), "grads": {k: t.grad.numpy() for k, t in P.items()},
            "dlogits": dlogits.numpy(), "pi": p.numpy(), "v": v.detach().numpy(),
            "u": u.detach().numpy()}


def live_fractions(W, nodes, counts):
    """Per stage (feature extractor, then every layer) the fraction of hidden units that are
    positive on row 0 of at least one leaf, in float64."""
    trace = []
    with torch.no_grad():
        forward(params(W), nodes, counts, trace)
    return [float((torch.stack([a[i] for a in trace]) > 0).any(0).double().mean())
            for i in range(len(trace[0]))]


def bars(g64, g32):
    """tests/golden/make_frozenlake_goldens.py's per-tensor bar, relative to the tensor's largest
    |float64 gradient|: 1e-5, or 4 x the float32 restatement's own deviation where that exceeds
    2.5e-6 -> ({name: bar}, {name: deviation} of the widened ones)."""
    out, widened = {}, {}
    for k, r in g64.items():
        top = float(np.abs(r).max())
        rel = float(np.abs(np.asarray(g32[k], np.float64) - r).max()) / top if top > 0 else 0.0
        out[k] = 1e-5
        if rel > 2.5e-6:
            out[k] = 4 * rel
            widened[k] = rel
    return out, widened
