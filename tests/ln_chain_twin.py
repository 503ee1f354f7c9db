"""Reference for hidden-layer chains of Dense, LayerNorm and BatchNorm layers: the semantics of DESIGN.md section 3.5 restated in torch on
the CPU, with autograd, around the registry's RbQ10 and Expo models.  Built on tests/bn_chain_twin.py (the mechanistic models, the leaf
order, the losses, the optimiser rules and BatchNorm itself are its own); what is new here is the LayerNorm layer and a forward that knows it.

LayerNorm: every sample over its own n features, y = act(scale (x - mean(x)) / sqrt(var(x) + eps) + bias) with the BIASED variance, the
gradient through both.  No state: training, evaluation and prediction are the same function.  Flat theta in the engine's leaf order
(model.leaves(): a LayerNorm's `bias`, then its `scale`).  `dtype` is a parameter: float64 = the reference the device is held to,
float32 = what fp32 arithmetic itself can reach.
"""
import numpy as np
import torch

from easyhybrid_jl_amd.models import _bn_kind, _ln_kind

from tests.bn_chain_twin import ACT, IN_EPS, MECH, adam, batch_norm, descent, initial_state, loss_of, unpack, update_state, weight_l2  # noqa: F401


def layer_norm(x, scale, bias, eps):
    """x (B, n) -> scale xh + bias, every row over its own n entries; mean first, the variance of the centred values"""
    d = x - x.mean(1, keepdim=True)
    xh = d / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    return xh if scale is None else scale * xh + bias


def forward(model, theta, X, forcings, rows, state=None, train=True, dtype=torch.float64, requires_grad=False):
    """rows: the minibatch (indices into the columns of X (P, N)) -> (yhat (n,), {parameter: (n,)}, theta tensor, {layer: (mean_B, var_B)})"""
    th = torch.tensor(np.asarray(theta), dtype=dtype, requires_grad=requires_grad)
    layers, glob = unpack(model, th)
    rows = np.asarray(rows, np.int64)
    state = state if state is not None else initial_state(model)
    h = torch.tensor(np.asarray(X), dtype=dtype)[:, rows].T
    stats = {}
    if model.config.get("input_batchnorm"):
        h, stats["in"] = batch_norm(h, None, None, IN_EPS, None if train else state["in"])
    acts = model.layer_activations or [model.config["activation"]] * (len(model.NN) - 1)
    for li, leaves in enumerate(layers):
        a = acts[li] if li < len(acts) else "identity"
        if _ln_kind(a):
            h = ACT[a.split(":", 1)[1]](layer_norm(h, leaves.get("scale"), leaves.get("bias"), model.layernorm[li]))
        elif _bn_kind(a):
            _, eps = model.batchnorm[li]
            h, stats[li] = batch_norm(h, leaves.get("scale"), leaves.get("bias"), eps, None if train else state[li])
            h = ACT[a.split(":", 1)[1]](h)
        else:
            h = ACT[a](h @ leaves["weight"].T + leaves["bias"])
    n = len(rows)
    names, fnames, fn = MECH[model.mechanistic_model.name]
    par = {}
    for nm in names:
        lo, hi = float(model.parameters.lower(nm)), float(model.parameters.upper(nm))
        if nm in model.neural_param_names:
            o_k = h[:, model.neural_param_names.index(nm)]
            par[nm] = lo + (hi - lo) * torch.sigmoid(o_k) if model.scale_nn_outputs else o_k
        elif nm in model.global_param_names:
            par[nm] = (lo + (hi - lo) * torch.sigmoid(glob[model.global_param_names.index(nm)])).expand(n)
        else:
            par[nm] = torch.full((n,), float(model.parameters.default(nm)), dtype=dtype)
    frc = {k: torch.tensor(np.asarray(forcings[k]), dtype=dtype)[rows] for k in fnames}
    return fn(par, frc), par, th, stats


def loss_and_grad(model, theta, X, forcings, y, rows, kind="mse", dtype=torch.float64, with_stats=False, l2=0.0):
    """train mode -> (loss, gradient (n_theta,), n_valid[, batch statistics]); l2: lambda of a WeightL2 term over the Dense weights, added to the loss"""
    yhat, _, th, stats = forward(model, theta, X, forcings, rows, None, True, dtype, requires_grad=True)
    yt = torch.tensor(np.asarray(y)[np.asarray(rows, np.int64)], dtype=dtype)
    nv = int((~torch.isnan(yt)).sum())
    loss = loss_of(yhat, yt, kind)
    if l2:
        layers, _ = unpack(model, th)
        loss = loss + l2 * sum((l["weight"] ** 2).sum() for l in layers if "weight" in l)
    loss.backward()
    out = (float(loss.detach()), th.grad.numpy().astype(np.float64), nv)
    return out + (stats,) if with_stats else out


def predict(model, theta, X, forcings, rows, state=None, dtype=torch.float64):
    """test mode (BatchNorm layers on the running statistics `state`; a LayerNorm layer as in training) -> (yhat, {parameter: values})"""
    with torch.no_grad():
        yhat, par, _, _ = forward(model, theta, X, forcings, rows, state, False, dtype)
    return yhat.numpy(), {k: v.numpy() for k, v in par.items()}


def train_steps(model, theta, X, forcings, y, batches, rule, kind="mse"):
    """one step per (first, count) of `batches` with the twin's fp64 gradient and the optimiser rule in NumPy fp32 (Optimisers.jl op for op)
    -> (theta, running statistics of the BatchNorm layers, if any)"""
    th, ost, state = np.asarray(theta, np.float32).copy(), {}, initial_state(model)
    for a, n in batches:
        rows = np.arange(a, a + n)
        _, g, _, stats = loss_and_grad(model, th, X, forcings, y, rows, kind, torch.float64, with_stats=True)
        state = update_state(model, state, stats, n)
        th = rule(th, g.astype(np.float32), ost)
    return th, state
