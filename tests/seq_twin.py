"""Reference for the sequence models: the semantics of DESIGN.md section 3.9 restated in torch on the CPU, with autograd.

    Dense(P -> I, act) -> LSTMCell(I -> H) over the window -> Dense(H -> H, act) -> Dense(H -> K) at the last `ow` steps
    -> sigma-scaling -> mechanistic model with the forcings of the same step -> masked loss over the valid (window, j) pairs

Flat theta in, loss / gradient / predictions out; `dtype` is a parameter (float64 = the reference the device is held to, float32 = what
fp32 arithmetic itself can reach).  Exact tanh / sigmoid (the device uses NNlib's fast forms, as Lux does).
"""
import numpy as np
import torch

MECH = {
    "RbQ10": (("rb", "Q10"), ("ta",), lambda p, f: p["rb"] * p["Q10"] ** (0.1 * (f["ta"] - 15.0))),
    "Expo_resp_model": (("Resp0", "k"), ("T",), lambda p, f: p["Resp0"] * torch.exp(p["k"] * f["T"])),
}
ACT = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu, "identity": lambda z: z, "swish": lambda z: z * torch.sigmoid(z)}


def unpack(model, th):
    """flat theta (a tensor) -> the ten leaves and the raw globals, ComponentArray order"""
    P, (I, H, _), K = len(model.predictors), model.hidden_layers, len(model.neural_param_names)
    shapes = [("w_in", (I, P)), ("b_in", (I,)), ("w_ih", (4 * H, I)), ("w_hh", (4 * H, H)), ("b_ih", (4 * H,)), ("b_hh", (4 * H,)),
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


def forward(model, theta, X, forcings, starts, W, ow, dtype=torch.float64, requires_grad=False):
    """-> (yhat (n, ow), {parameter: (n, ow)}, theta tensor)"""
    th = torch.tensor(np.asarray(theta), dtype=dtype, requires_grad=requires_grad)
    p = unpack(model, th)
    act = ACT[model.config["activation"]]
    Xt = torch.tensor(np.asarray(X), dtype=dtype)
    starts = np.asarray(starts, np.int64)
    n, H = len(starts), p["w_hd"].shape[0]
    h = torch.zeros(n, H, dtype=dtype)
    c = torch.zeros(n, H, dtype=dtype)
    outs = []
    for t in range(W):
        x = act(Xt[:, starts + t].T @ p["w_in"].T + p["b_in"])
        z = x @ p["w_ih"].T + h @ p["w_hh"].T + p["b_ih"] + p["b_hh"]
        i, f, g, o = (z[:, k * H:(k + 1) * H] for k in range(4))
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        if t >= W - ow:
            outs.append(act(h @ p["w_hd"].T + p["b_hd"]) @ p["w_out"].T + p["b_out"])
    O = torch.stack(outs, 1)                                             # (n, ow, K)
    names, fnames, fn = MECH[model.mechanistic_model.name]
    par = {}
    for nm in names:
        lo, hi = float(model.parameters.lower(nm)), float(model.parameters.upper(nm))
        if nm in model.neural_param_names:
            o_k = O[:, :, model.neural_param_names.index(nm)]
            par[nm] = lo + (hi - lo) * torch.sigmoid(o_k) if model.scale_nn_outputs else o_k
        elif nm in model.global_param_names:
            par[nm] = (lo + (hi - lo) * torch.sigmoid(p["glob"][model.global_param_names.index(nm)])).expand(n, ow)
        else:
            par[nm] = torch.full((n, ow), float(model.parameters.default(nm)), dtype=dtype)
    rows = starts[:, None] + (W - ow) + np.arange(ow)[None, :]
    frc = {k: torch.tensor(np.asarray(forcings[k]), dtype=dtype)[rows] for k in fnames}
    return fn(par, frc), par, th


def loss_of(yhat, yt, kind):
    m = ~torch.isnan(yt)
    r = yhat[m] - yt[m]
    if kind == "mse":
        return (r * r).mean()
    if kind == "rmse":
        return torch.sqrt((r * r).mean())
    if kind == "mae":
        return r.abs().mean()
    if kind == "nseLoss":
        return (r * r).sum() / ((yt[m] - yt[m].mean()) ** 2).sum()
    raise KeyError(kind)


def targets_of(y, starts, W, ow, lam):
    rows = np.asarray(starts, np.int64)[:, None] + (W - ow + lam) + np.arange(ow)[None, :]
    return np.asarray(y)[rows]


def loss_and_grad(model, theta, X, forcings, y, starts, W, ow, lam, kind="mse", dtype=torch.float64):
    """-> (loss, gradient (n_theta,), n_valid)"""
    yhat, _, th = forward(model, theta, X, forcings, starts, W, ow, dtype, requires_grad=True)
    yt = torch.tensor(targets_of(y, starts, W, ow, lam), dtype=dtype)
    nv = int((~torch.isnan(yt)).sum())
    if nv == 0:
        return float("nan"), np.zeros(th.numel()), 0
    loss = loss_of(yhat, yt, kind)
    loss.backward()
    return float(loss.detach()), th.grad.numpy().astype(np.float64), nv


def predict(model, theta, X, forcings, starts, W, ow, dtype=torch.float64):
    with torch.no_grad():
        yhat, par, _ = forward(model, theta, X, forcings, starts, W, ow, dtype)
    return yhat.numpy(), {k: v.numpy() for k, v in par.items()}
