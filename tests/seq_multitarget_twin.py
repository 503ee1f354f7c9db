"""Reference for sequence models with several targets: the forward of tests/seq_closure_twin.py (with the recurrent step of
tests/seq_cells_twin.py for the other cells) returning EVERY output of the mechanistic model, and the reference's loss over them
(compute_loss.jl:92-145): target t reads its own output, its own column and so its own NaN mask, its own loss kind, and the per-target
losses are aggregated by `agg`,

    loss = a * sum_t w_t * sum_{(window, j) valid for t} term_t        term = r^2 (mse, nseLoss) | |r| (mae),
    w_t = 1 / n_t (mse, mae) | 1 / sum (y - mean y)^2 (nseLoss),       a = 1 (agg = sum) | 1 / T (mean)

over the materialised windows -- a row of the series that several windows read counts once per window.  A target without a valid
entry adds nothing.  fp64 torch on the CPU, the gradient from autograd.
"""
import numpy as np
import torch

import easyhybrid_jl_amd as eh
from tests import seq_cells_twin as cw
from tests import seq_closure_twin as ct
from tests import seq_twin as tw

KINDS = ("mse", "mae", "nseLoss")


def _all_outputs(mech):
    return lambda **kw: {"all": torch.stack(list(mech(**kw).values()), 0)}


def forward(model, mech, outs, theta, X, forcings, starts, W, ow, dtype=torch.float64, requires_grad=False):
    """-> (yhat (T, n, ow): output outs[t] of the model for target t, {parameter: (n, ow)}, theta tensor)"""
    yall, par, th = cw.forward(model, _all_outputs(mech), 0, theta, X, forcings, starts, W, ow, dtype, requires_grad)
    return yall[list(outs)], par, th


def targets_of(ys, starts, W, ow, lam):
    """the materialised targets (T, n, ow): row start + W - ow + j + lam of every target's series"""
    return np.stack([tw.targets_of(y, starts, W, ow, lam) for y in ys], 0)


def weights(ys, starts, W, ow, lam, kinds, agg="sum"):
    """-> (w (T,), n (T,)): the weight of every target's residual terms and its count of valid entries; 0 for a target without one"""
    yt = targets_of(ys, starts, W, ow, lam).astype(np.float64)
    a = 1.0 / len(ys) if agg == "mean" else 1.0
    w, n = np.zeros(len(ys)), np.zeros(len(ys), np.int64)
    for t, kind in enumerate(kinds):
        v = yt[t][~np.isnan(yt[t])]
        n[t] = v.size
        if v.size:
            w[t] = a / (((v - v.mean()) ** 2).sum() if kind == "nseLoss" else v.size)
    return w, n


def loss_of(yhat, yt, kinds, agg="sum"):
    """the aggregated loss of (T, n, ow) predictions against (T, n, ow) targets: tests/seq_twin.py `loss_of` per target with a valid entry"""
    terms = [tw.loss_of(yhat[t], yt[t], kind) for t, kind in enumerate(kinds) if bool((~torch.isnan(yt[t])).any())]
    loss = terms[0]
    for x in terms[1:]:
        loss = loss + x
    return loss / len(kinds) if agg == "mean" else loss


def loss_and_grad(model, mech, outs, theta, X, forcings, ys, starts, W, ow, lam, kinds, agg="sum", dtype=torch.float64):
    """-> (loss, gradient (n_theta,), valid entries per target (T,)); kinds: one loss kind per target"""
    assert len(kinds) == len(outs) == len(ys) and all(k in KINDS for k in kinds)
    yhat, _, th = forward(model, mech, outs, theta, X, forcings, starts, W, ow, dtype, requires_grad=True)
    yt = torch.tensor(targets_of(ys, starts, W, ow, lam), dtype=dtype)
    nv = (~torch.isnan(yt)).sum(dim=(1, 2)).numpy()
    if nv.sum() == 0:
        return float("nan"), np.zeros(th.numel()), nv
    loss = loss_of(yhat, yt, kinds, agg)
    if not loss.requires_grad:
        return float(loss), np.zeros(th.numel()), nv
    loss.backward()
    return float(loss.detach()), th.grad.numpy().astype(np.float64), nv


def predict(model, mech, outs, theta, X, forcings, starts, W, ow, dtype=torch.float64):
    with torch.no_grad():
        yhat, par, _ = forward(model, mech, outs, theta, X, forcings, starts, W, ow, dtype)
    return yhat.numpy(), {k: v.numpy() for k, v in par.items()}


# ---- models: several targets around the registry's three-output model and around the three-output closure ---------------------------
FLUXPART_OUTPUTS = ["NEE", "GPP", "RECO"]


def fluxpart_model(kind, targets, I, H, act="tanh", cell_act="tanh"):
    """FluxPartModelQ10 observed at `targets` (names of its outputs, any order) -> (model, torch spelling, output index per target)"""
    model = eh.constructHybridModel(["x0", "x1"], ["SW_IN", "TA"], list(targets), eh.FluxPartModelQ10, dict(ct.FLUXPART_TABLE), ["RUE", "Rb"], ["Q10"],
                                    hidden_layers=cw.chain(kind, I, H, cell_act), activation=act, scale_nn_outputs=True)
    return model, ct.fluxpart_torch, [FLUXPART_OUTPUTS.index(t) for t in targets]


def flux3_model(kind, targets, I, H, act="tanh", cell_act="tanh"):
    """the recorded closure flux3 (tests/seq_closure_twin.py) observed at `targets` of nee / gpp / reco"""
    ms = eh.models.resolve_mech(ct.flux3_np, list(ct.FLUX3_TABLE), list(ct.FLUX3_FORCINGS), list(ct.FLUX3_OUTPUTS))
    model = eh.constructHybridModel(["x0", "x1"], list(ct.FLUX3_FORCINGS), list(targets), ms, dict(ct.FLUX3_TABLE), ["rue", "rb"], ["q10"],
                                    hidden_layers=cw.chain(kind, I, H, cell_act), activation=act, scale_nn_outputs=True)
    return model, ct.flux3_torch, [list(ms.outputs).index(t) for t in targets]


def masked_targets(names, seed, frac=0.2, head="fluxpart"):
    """the series' targets `names` (NaN-free copies of the truth + noise) under NaN masks of their own: about `frac` of each, seeded"""
    _, _, tg = ct.series()
    rng = np.random.default_rng(seed)
    out = []
    for nm in names:
        key = nm if head == "fluxpart" else "flux_" + nm
        v = np.array(tg[key], np.float32)
        fill = np.nanmean(v)
        v = np.where(np.isnan(v), np.float32(fill) + 0.1 * rng.standard_normal(v.size).astype(np.float32), v).astype(np.float32)
        v[rng.random(v.size) < frac] = np.nan
        out.append(v)
    return out
