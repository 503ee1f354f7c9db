"""Reference for sequence models around a recorded closure or a multi-output registry model: tests/seq_twin.py's forward restated in
torch with the mechanistic model passed in as a function and the index of the output the one target reads.

Every test closure is written twice: a NumPy spelling, which the recorder traces into the device program, and a torch spelling, which
autograd differentiates here.  (The literal constants of flux3 are exactly representable in fp32, so the recorded program -- constants in
fp32 -- and the fp64 twin agree to rounding; rbq10 keeps the reference's 0.1, as tests/closures.py does.)  The parity cases the CPU and the
GPU tests share live here too, with the one series they run on.
"""
import numpy as np
import torch

import easyhybrid_jl_amd as eh
from tests import seq_twin as tw


# ---- closure 1: RbQ10 written by hand (one neural, one global parameter) ---------------------------------------------------------
def rbq10_np(*, ta, rb, Q10):
    return dict(reco=rb * Q10 ** (0.1 * (ta - 15.0)))


def rbq10_torch(*, ta, rb, Q10):
    return dict(reco=rb * Q10 ** (0.1 * (ta - 15.0)))


RBQ10_TABLE = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}


# ---- closures 2 and 3: flux partitioning, three outputs ---------------------------------------------------------------------------
def flux3_np(*, sw, ta, vpd, rue, rb, q10, k):
    """light-saturating GPP with a VPD limitation; Q10 respiration damped in the cold plus a growth term; nee = reco - gpp"""
    lim = np.where(vpd > 10.0, np.exp(-k * (vpd - 10.0)), 1.0)
    light = sw / (1.0 + 0.001953125 * sw)
    gpp = rue * light * lim * 0.0625
    base = rb * np.exp(np.log(q10) * (0.125 * (ta - 16.0)))
    damp = 1.0 / (1.0 + np.exp(-0.5 * (ta + 5.0)))
    reco = base * damp + 0.25 * gpp
    return dict(nee=reco - gpp, gpp=gpp, reco=reco)


def flux3_torch(*, sw, ta, vpd, rue, rb, q10, k):
    lim = torch.where(vpd > 10.0, torch.exp(-k * (vpd - 10.0)), torch.ones_like(vpd))
    light = sw / (1.0 + 0.001953125 * sw)
    gpp = rue * light * lim * 0.0625
    base = rb * torch.exp(torch.log(q10) * (0.125 * (ta - 16.0)))
    damp = 1.0 / (1.0 + torch.exp(-0.5 * (ta + 5.0)))
    reco = base * damp + 0.25 * gpp
    return dict(nee=reco - gpp, gpp=gpp, reco=reco)


FLUX3_TABLE = {"rue": (0.3, 0.0, 1.0), "rb": (3.0, 0.0, 13.0), "q10": (2.0, 1.0, 4.0), "k": (0.0625, 0.0, 0.5)}
FLUX3_FORCINGS, FLUX3_OUTPUTS = ["sw", "ta", "vpd"], ["nee", "gpp", "reco"]


# ---- the registry's three-output model (src/models/FluxPartModel_Q10_Lux.jl:50-79), torch spelling only ----------------------------
def fluxpart_torch(*, SW_IN, TA, RUE, Rb, Q10):
    gpp = SW_IN * RUE / 12.011
    reco = Rb * Q10 ** (0.1 * (TA - 15.0))
    return dict(NEE=reco - gpp, GPP=gpp, RECO=reco)


FLUXPART_TABLE = {"RUE": (0.1, 0.0, 1.0), "Rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}

# closure id -> (NumPy spelling, torch spelling, parameter table, forcings, outputs, target, neural, global)
CLOSURES = {
    1: (rbq10_np, rbq10_torch, RBQ10_TABLE, ["ta"], ["reco"], "reco", ["rb"], ["Q10"]),
    2: (flux3_np, flux3_torch, FLUX3_TABLE, FLUX3_FORCINGS, FLUX3_OUTPUTS, "reco", ["rue", "rb"], ["q10"]),      # k is fixed
    3: (flux3_np, flux3_torch, FLUX3_TABLE, FLUX3_FORCINGS, FLUX3_OUTPUTS, "nee", ["rue", "rb"], ["q10"]),
}


def _chain(I, H):
    return eh.Chain(eh.Recurrence(eh.LSTMCell(I, H)))


def closure_model(cid, I, H, act="tanh", scale=True, predictors=("x0", "x1")):
    """-> (model, torch spelling, output index of the target).  The closure is recorded with ALL its outputs, as a user's closure returns
    more than the target (the reference's LSTM tutorial returns (; reco, Q10, rb)); the one target then names its output."""
    fn, fn_t, table, forc, outs, target, neural, glob = CLOSURES[cid]
    ms = eh.models.resolve_mech(fn, list(table), list(forc), list(outs))
    model = eh.constructHybridModel(list(predictors), list(forc), [target], ms, dict(table), neural, glob, hidden_layers=_chain(I, H),
                                    activation=act, scale_nn_outputs=scale)
    return model, fn_t, list(ms.outputs).index(target)


def fluxpart_model(target, I, H, act="tanh"):
    model = eh.constructHybridModel(["x0", "x1"], ["SW_IN", "TA"], [target], eh.FluxPartModelQ10, dict(FLUXPART_TABLE), ["RUE", "Rb"], ["Q10"],
                                    hidden_layers=_chain(I, H), activation=act, scale_nn_outputs=True)
    return model, fluxpart_torch, ["NEE", "GPP", "RECO"].index(target)


# ---- the twin ------------------------------------------------------------------------------------------------------------------------
def forward(model, mech, out, theta, X, forcings, starts, W, ow, dtype=torch.float64, requires_grad=False, tanh=torch.tanh):
    """tests/seq_twin.py `forward` with the mechanistic stage `mech(**forcings, **parameters) -> dict`, of which output `out` is the
    prediction -> (yhat (n, ow), {parameter: (n, ow)}, theta tensor).  `tanh`: the spelling of the cell's two tanh (tests/seq_fuzz_cases.py
    runs the fp32 twin with a second one)"""
    th = torch.tensor(np.asarray(theta), dtype=dtype, requires_grad=requires_grad)
    p = tw.unpack(model, th)
    act = tw.ACT[model.config["activation"]]
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
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * tanh(g)
        h = torch.sigmoid(o) * tanh(c)
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


# ---- the series: 400 rows, 10 % NaN targets (tests/test_gpu_seq.py's construction, with the forcings and targets of the flux closure) -----
LROWS = 400
_SERIES = {}


def series(rows=LROWS, nan_frac=0.1):
    """-> (X (2, rows), {forcing: (rows,)}, {target: (rows,)}): computed once and left unchanged.  `ta` / `reco` are the series of
    tests/test_gpu_seq.py; SW_IN / TA name sw / ta for the registry's flux-partitioning model."""
    key = (rows, nan_frac)
    if key not in _SERIES:
        rng = np.random.default_rng(1234 + 2)
        X = (0.6 * rng.standard_normal((2, rows))).astype(np.float32)
        X[0] = np.cumsum(X[0]) * 0.2                                     # something a memory can use
        ta = (10 + 8 * rng.standard_normal(rows)).astype(np.float32)
        reco = (3.0 + np.tanh(X[0])) * 2.0 ** (0.1 * (ta - 15.0)) + 0.1 * rng.standard_normal(rows)
        reco = reco.astype(np.float32)
        reco[rng.random(rows) < nan_frac] = np.nan
        sw = rng.uniform(0.0, 800.0, rows).astype(np.float32)
        vpd = rng.uniform(0.0, 30.0, rows).astype(np.float32)
        f64 = lambda a: a.astype(np.float64)
        truth = flux3_np(sw=f64(sw), ta=f64(ta), vpd=f64(vpd), rue=0.3 + 0.2 * np.tanh(f64(X[1])), rb=3.0 + np.tanh(f64(X[0])), q10=2.0, k=0.0625)
        frc = {"ta": ta, "sw": sw, "vpd": vpd, "SW_IN": sw, "TA": ta}
        tg = {"reco": reco}
        for name in ("nee", "gpp", "reco"):
            v = (truth[name] + 0.2 * rng.standard_normal(rows)).astype(np.float32)
            v[rng.random(rows) < nan_frac] = np.nan
            tg["flux_" + name] = v
        tg.update(NEE=tg["flux_nee"], GPP=tg["flux_gpp"], RECO=tg["flux_reco"])
        for a in [X, *frc.values(), *tg.values()]:
            a.setflags(write=False)
        _SERIES[key] = (X, frc, tg)
    return _SERIES[key]


def target_series(cid_or_name):
    """the target series a closure (1, 2, 3) or a FluxPartModelQ10 output name is compared with"""
    _, _, tg = series()
    return tg[{1: "reco", 2: "flux_reco", 3: "flux_nee"}.get(cid_or_name, cid_or_name)]


def all_starts(rows, W, lam, s=1):
    return np.arange(0, rows - W - lam + 1, s, dtype=np.int32)


# ---- the parity cases ---------------------------------------------------------------------------------------------------------------
SHAPES = [(6, 2, 5, 2, 1), (32, 32, 3, 3, 0), (20, 9, 7, 3, 0), (15, 15, 10, 1, 0), (9, 24, 6, 2, 1)]      # (I, H, W, ow, lam)
SHAPE_IDS = ["I6H2", "I32H32", "I20H9", "tutorial", "I9H24"]          # (appended to only: `variant` pairs by position)
COUNTS = [5, 17, 70, 300]


def variant(si, ci):
    """-> (closure, activation, sigma-scaling, loss, shuffled idx) of a case: every value of the issue's list occurs over the first 16 cases"""
    k = si * len(COUNTS) + ci
    cid = (1, 2, 3)[k % 3]
    scale = not (cid == 1 and (k // 3) % 2 == 0)          # raw NN outputs on closure 1 only (the flux closure divides and takes logs of its parameters)
    return cid, ("tanh", "sigmoid")[(k // 2) % 2], scale, ("mse", "nseLoss", "mae")[(k + k // 3) % 3], ci == 2 or k % 5 == 0


def case(si, ci):
    """-> everything a parity case is made of: (model, torch closure, output index, X, forcings, y, theta, selected starts, W, ow, lam,
    loss kind, engine keywords selecting the same windows, all starts)"""
    (I, H, W, ow, lam), count = SHAPES[si], COUNTS[ci]
    cid, act, scale, kind, shuffled = variant(si, ci)
    model, fn_t, out = closure_model(cid, I, H, act, scale)
    X, frc, _ = series()
    y = target_series(cid)
    starts = all_starts(LROWS, W, lam)
    theta = model.initialparameters(100 + 10 * si + ci)
    if shuffled:
        idx = np.random.default_rng(7 + si + ci).permutation(len(starts))[:count].astype(np.int32)
        sel, kw = starts[idx], dict(idx=idx)
    else:
        sel, kw = starts[:count], dict(first=0, count=count)
    return model, fn_t, out, X, frc, y, theta, sel, W, ow, lam, kind, kw, starts
