"""Reference for sequence models around any of the three recurrent cells: tests/seq_closure_twin.py's forward with the recurrent step
written out op by op for LSTMCell, GRUCell and RNNCell, torch on the CPU with autograd.

    Dense(P -> I, act) -> cell(I -> H) over the window -> Dense(H -> H, act) -> Dense(H -> K) at the last `ow` steps
    -> sigma-scaling -> mechanistic model `mech(**forcings, **parameters) -> dict`, output `out` -> masked loss

The Dense / head / mechanistic parts and the losses are tests/seq_twin.py's; only the cell's leaves and its step are new here.
"""
import numpy as np
import torch

import easyhybrid_jl_amd as eh
from tests import seq_closure_twin as ct
from tests import seq_twin as tw

GATES = {"lstm": 4, "gru": 3, "rnn": 1}


def make_cell(kind, I, H, act="tanh"):
    """-> the cell's description: kind "lstm" | "gru" | "rnn" (`act`: the RNNCell's activation)"""
    return {"lstm": lambda: eh.LSTMCell(I, H), "gru": lambda: eh.GRUCell(I, H), "rnn": lambda: eh.RNNCell(I, H, activation=act)}[kind]()


def chain(kind, I, H, act="tanh"):
    return eh.Chain(eh.Recurrence(make_cell(kind, I, H, act)))


def unpack(model, th):
    """flat theta (a tensor) -> the ten leaves and the raw globals, ComponentArray order; the cell's leaves have GATES[cell] blocks of H rows"""
    P, (I, H, _), K = len(model.predictors), model.hidden_layers, len(model.neural_param_names)
    G = GATES[model.cell]
    shapes = [("w_in", (I, P)), ("b_in", (I,)), ("w_ih", (G * H, I)), ("w_hh", (G * H, H)), ("b_ih", (G * H,)), ("b_hh", (G * H,)),
              ("w_hd", (H, H)), ("b_hd", (H,)), ("w_out", (K, H)), ("b_out", (K,))]
    out, off = {}, 0
    for name, shp in shapes:
        n = int(np.prod(shp))
        v = th[off:off + n]
        out[name] = v.reshape(shp[::-1]).T if len(shp) == 2 else v      # column-major matrices
        off += n
    out["glob"] = th[off:]
    assert off + len(model.global_param_names) == th.numel()
    return out


def cell_step(kind, p, x, h, c, act=torch.tanh, tanh=torch.tanh):
    """one step of the cell on (n, I) inputs and (n, H) state -> (h', c'); `p` holds w_ih, w_hh, b_ih, b_hh; c is the LSTM's alone"""
    H = h.shape[1]
    if kind == "lstm":
        z = x @ p["w_ih"].T + h @ p["w_hh"].T + p["b_ih"] + p["b_hh"]
        i, f, g, o = (z[:, k * H:(k + 1) * H] for k in range(4))
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * tanh(g)
        return torch.sigmoid(o) * tanh(c), c
    if kind == "gru":
        zi = x @ p["w_ih"].T + p["b_ih"]
        zh = h @ p["w_hh"].T + p["b_hh"]
        r = torch.sigmoid(zi[:, :H] + zh[:, :H])
        z = torch.sigmoid(zi[:, H:2 * H] + zh[:, H:2 * H])
        q = zh[:, 2 * H:]                                                # W_hn h + b_hn: the reset gate multiplies it
        n = tanh(zi[:, 2 * H:] + r * q)
        return (1.0 - z) * n + z * h, c
    if kind == "rnn":
        return act(x @ p["w_ih"].T + p["b_ih"] + h @ p["w_hh"].T + p["b_hh"]), c
    raise KeyError(kind)


def forward(model, mech, out, theta, X, forcings, starts, W, ow, dtype=torch.float64, requires_grad=False, tanh=torch.tanh):
    """-> (yhat (n, ow), {parameter: (n, ow)}, theta tensor).  `tanh`: the spelling of the LSTM's and the GRU's tanh (the fuzz runs the
    fp32 twin with a second one, tests/seq_fuzz_cases.py)"""
    th = torch.tensor(np.asarray(theta), dtype=dtype, requires_grad=requires_grad)
    p = unpack(model, th)
    act = tw.ACT[model.config["activation"]]
    cact = tw.ACT[model.cell_activation] if model.cell == "rnn" else None
    Xt = torch.tensor(np.asarray(X), dtype=dtype)
    starts = np.asarray(starts, np.int64)
    n, H = len(starts), p["w_hd"].shape[0]
    h = torch.zeros(n, H, dtype=dtype)
    c = torch.zeros(n, H, dtype=dtype)
    outs = []
    for t in range(W):
        x = act(Xt[:, starts + t].T @ p["w_in"].T + p["b_in"])
        h, c = cell_step(model.cell, p, x, h, c, cact, tanh)
        if t >= W - ow:
            outs.append(act(h @ p["w_hd"].T + p["b_hd"]) @ p["w_out"].T + p["b_out"])
    O = torch.stack(outs, 1)                                             # (n, ow, K)
    par = {}
    for nm in model.mechanistic_model.params:
        lo, hi = float(model.parameters.lower(nm)), float(model.parameters.upper(nm))
        if nm in model.neural_param_names:
            o_k = O[:, :, model.neural_param_names.index(nm)]
            par[nm] = lo + (hi - lo) * torch.sigmoid(o_k) if model.scale_nn_outputs else o_k
        elif nm in model.global_param_names:
            par[nm] = (lo + (hi - lo) * torch.sigmoid(p["glob"][model.global_param_names.index(nm)])).expand(n, ow)
        else:
            par[nm] = torch.full((n, ow), float(model.parameters.default(nm)), dtype=dtype)
    rows = starts[:, None] + (W - ow) + np.arange(ow)[None, :]
    frc = {k: torch.tensor(np.asarray(forcings[k]), dtype=dtype)[rows] for k in model.mechanistic_model.forcings}
    res = mech(**frc, **par)
    return list(res.values())[out], par, th


def loss_and_grad(model, mech, out, theta, X, forcings, y, starts, W, ow, lam, kind="mse", dtype=torch.float64, tanh=torch.tanh):
    """-> (loss, gradient (n_theta,), n_valid)"""
    yhat, _, th = forward(model, mech, out, theta, X, forcings, starts, W, ow, dtype, requires_grad=True, tanh=tanh)
    yt = torch.tensor(tw.targets_of(y, starts, W, ow, lam), dtype=dtype)
    nv = int((~torch.isnan(yt)).sum())
    if nv == 0:
        return float("nan"), np.zeros(th.numel()), 0
    loss = tw.loss_of(yhat, yt, kind)
    if not loss.requires_grad:                                           # (a target that no trained parameter reaches)
        return float(loss), np.zeros(th.numel()), nv
    loss.backward()
    return float(loss.detach()), th.grad.numpy().astype(np.float64), nv


def predict(model, mech, out, theta, X, forcings, starts, W, ow, dtype=torch.float64):
    with torch.no_grad():
        yhat, par, _ = forward(model, mech, out, theta, X, forcings, starts, W, ow, dtype)
    return yhat.numpy(), {k: v.numpy() for k, v in par.items()}


# ---- the models the CPU and the GPU tests share (tests/seq_closure_twin.py's tables, closures and series) ---------------------------------
def rbq10_model(kind, I, H, act="tanh", cell_act="tanh", scale=True, P=2):
    """RbQ10 from the registry: rb neural, Q10 global -> (model, torch spelling, output index)"""
    model = eh.constructHybridModel([f"x{i}" for i in range(P)], ["ta"], ["reco"], eh.RbQ10, dict(ct.RBQ10_TABLE), ["rb"], ["Q10"],
                                    hidden_layers=chain(kind, I, H, cell_act), activation=act, scale_nn_outputs=scale)
    return model, ct.rbq10_torch, 0


def fluxpart_model(kind, target, I, H, act="tanh", cell_act="tanh"):
    model = eh.constructHybridModel(["x0", "x1"], ["SW_IN", "TA"], [target], eh.FluxPartModelQ10, dict(ct.FLUXPART_TABLE), ["RUE", "Rb"], ["Q10"],
                                    hidden_layers=chain(kind, I, H, cell_act), activation=act, scale_nn_outputs=True)
    return model, ct.fluxpart_torch, ["NEE", "GPP", "RECO"].index(target)


def closure_model(kind, cid, I, H, act="tanh", cell_act="tanh", scale=True, predictors=("x0", "x1")):
    """tests/seq_closure_twin.py `closure_model` around the given cell"""
    fn, fn_t, table, forc, outs, target, neural, glob = ct.CLOSURES[cid]
    ms = eh.models.resolve_mech(fn, list(table), list(forc), list(outs))
    model = eh.constructHybridModel(list(predictors), list(forc), [target], ms, dict(table), neural, glob, hidden_layers=chain(kind, I, H, cell_act),
                                    activation=act, scale_nn_outputs=scale)
    return model, fn_t, list(ms.outputs).index(target)
