"""The inputs of the optimiser-chain tests, shared by tests/test_chain.py (CPU: are they well posed?) and tests/test_gpu_chain.py.

Four paths, the smallest shapes that select each step kernel family:

    perwave    RbQ10 [16, 16], 512 rows, batches of 128                     (util.rbq10_case(512, ...))
    rowsplit   one hidden layer of 96, the same rows
    lform      [512, 256] at batch 64: 133 122 parameters, so the norm spans many workgroups (the layer-wise form)
    seq        the tutorial sequence model I = H = 15, W = 10, 128 windows of the 400-row series of tests/seq_closure_twin.py

and five chains.  The thresholds come from the twin (tests/chain_twin.py), never from the device: delta is a quarter of the first
batch's largest gradient entry, and omega lies between two of the four norms of the twin's fp64 trajectory (tune_omega), a hundredth
away from each at least, so that some steps clip and some do not.  Everything is computed once, cached and left unchanged."""
import numpy as np

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho

from tests import util
from tests.chain_twin import ChainTwin

PATHS = ("perwave", "rowsplit", "lform", "seq")
CHAINS = ("clipnorm_adam", "clipnorm_inf_descent", "clipgrad_rmsprop", "adam_weightdecay", "full")
NSTEPS = 4
INF = float("inf")
_CASES, _TUNED, _TRAJ = {}, {}, {}
_HIDDEN = {"perwave": (16, 16), "rowsplit": (96,), "lform": (512, 256)}
# Learning rate of the Adam-like rules (Adam, AdamW, RMSProp) in the trajectories.  Their first steps are sign-like -- lr g / (|g| + eps)
# -- so a relative rounding error e of ONE gradient entry moves that parameter by about lr e, whoever computes the gradient.  Among 133 122
# entries summed over 64 samples some cancel to a thousandth of their terms (e ~ 1e-3 in fp32): at lr = 0.01 the twin's own fp32 and fp64
# runs then differ by up to 5.6e-4 on the layer-wise shape, which the 3e-5 bar cannot tell from a defect.  The layer-wise trajectories
# therefore run at Optimisers.jl's default 0.001, and tests/test_chain.py holds every trajectory's fp32 twin to a TENTH of the bar against
# its fp64 run, so that an ill-conditioned input fails there, as an input.
LR = {"perwave": 0.01, "rowsplit": 0.01, "lform": 0.001, "seq": 0.01}
RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}


def _f32(x):
    return float(np.float32(x))


def case(path):
    if path in _CASES:
        return _CASES[path]
    if path == "seq":
        from tests import seq_closure_twin as ct
        X, frc, tg = ct.series()
        model = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"],
                                        hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(15, 15))), activation="tanh", scale_nn_outputs=True)
        W, ow, lam = 10, 1, 1
        c = dict(kind="seq", model=model, X=X, ta=frc["ta"], y=tg["reco"], W=W, ow=ow, lam=lam, starts=ct.all_starts(ct.LROWS, W, lam),
                 theta=model.initialparameters(21), batches=[(0, 128), (128, 128), (256, 128), (60, 128), (200, 128)])
    else:
        spec, theta, X, f, y = util.rbq10_case(512, "tanh", True, 0.1, hidden=_HIDDEN[path])
        n = 64 if path == "lform" else 128
        c = dict(kind="mlp", spec=spec, theta=theta, X=X, f=f, y=y, batches=[(a * n, n) for a in range(4)] + [(n // 2, n)])
    c["path"] = path
    c["theta"] = np.asarray(c["theta"], np.float32)
    c["theta"].setflags(write=False)
    _CASES[path] = c
    return c


def make_engine(c):
    if c["kind"] == "seq":
        eng = c["model"].engine(0)
        eng.set_data(eh.EH_SPLIT_TRAIN, c["X"], [c["ta"]], [c["y"]])
        eng.set_sequences(eh.EH_SPLIT_TRAIN, c["W"], c["ow"], c["lam"], c["starts"])
        eng.set_params(c["theta"])
        return eng
    return util.load_engine(c["spec"], c["theta"], c["X"], c["f"], c["y"])


def grad(c, th, k, dtype):
    """(gradient of batch k at th as `dtype`, the batch has a valid sample): the fp32 / fp64 oracle; for the sequence path the torch twin
    in fp64, cast -- as tests/test_gpu_parity.py::test_other_optimiser_rules and tests/test_gpu_seq.py take theirs"""
    a, n = c["batches"][k]
    if c["kind"] == "seq":
        import torch
        from tests import seq_twin as tw
        _, g, nv = tw.loss_and_grad(c["model"], np.asarray(th), c["X"], {"ta": c["ta"]}, c["y"], c["starts"][a:a + n], c["W"], c["ow"], c["lam"], "mse", torch.float64)
        return np.asarray(g).astype(dtype), nv > 0
    sl = slice(a, a + n)
    _, g, nv = ho.loss_and_grad(c["spec"], np.asarray(th, dtype), c["X"][:, sl], {k_: v[sl] for k_, v in c["f"].items()},
                                {k_: v[sl] for k_, v in c["y"].items()}, dtype)
    return np.asarray(g).astype(dtype), sum(nv) > 0


def _chain(name, omega, delta, lr=0.01):
    """(stages, opt_init's keyword arguments of the rule); lr: the learning rate of the Adam-like rules (see LR)"""
    if name == "clipnorm_adam":
        return [("clipnorm", omega, 2.0, True), ("rule",)], dict(rule="Adam", lr=lr)
    if name == "clipnorm_inf_descent":
        # (the largest gradient entries of these cases are 20 to 30: a learning rate that keeps the unclipped step at a few hundredths)
        return [("clipnorm", omega, INF, True), ("rule",)], dict(rule="Descent", lr=0.002)
    if name == "clipgrad_rmsprop":
        return [("clipgrad", delta), ("rule",)], dict(rule="RMSProp", lr=lr, beta1=0.9)
    if name == "adam_weightdecay":
        return [("rule",), ("weightdecay", _f32(0.01))], dict(rule="Adam", lr=lr)
    if name == "full":      # WeightDecay + ClipNorm(p = 1) + ClipGrad + AdamW + ClipGrad (the last one at half the learning rate: Adam's first steps are about lr)
        return ([("weightdecay", _f32(1e-3)), ("clipnorm", omega, 1.0, True), ("clipgrad", delta), ("rule",), ("clipgrad", _f32(0.5 * lr))],
                dict(rule="AdamW", lr=lr, weight_decay=0.01))
    raise KeyError(name)


def run_twin(c, stages, rule, dtype, nsteps=NSTEPS, grads=None):
    tw = ChainTwin(c["theta"].size, stages, dtype=dtype, **rule)
    th = c["theta"].astype(dtype)
    for k in range(nsteps):
        g, valid = grads[k] if grads is not None else grad(c, th, k, dtype)
        th = tw.step(th, g, valid)
    return th, tw


def tune_omega(run, nsteps=NSTEPS):
    """omega for which `run(omega) -> ChainTwin` (an fp64 trajectory) clips some of its steps and not others, every norm farther than 1e-2
    relative from it.  Clipping changes the trajectory, so the candidates -- geometric means of neighbouring norms, the middle pair
    first -- are taken from the latest trajectory until one holds."""
    omega, tried = 1e30, []
    for _ in range(12):
        tw = run(omega)
        n = [x for x in tw.norms if x is not None]
        if 0 < tw.clipped < nsteps and min(abs(x - omega) / omega for x in n) > 1e-2:
            return omega
        s_ = sorted(n)
        cands = [_f32(np.sqrt(s_[i] * s_[i + 1])) for i in (1, 0, 2) if i + 1 < len(s_)]
        new = [w for w in cands if w not in tried]
        if not new:
            break
        omega = new[0]
        tried.append(omega)
    raise AssertionError(f"no threshold found: tried {tried}")


def chain(path, name):
    """the chain `name` on `path` with its thresholds picked from the twin -> (stages, rule)"""
    key = (path, name)
    if key not in _TUNED:
        c = case(path)
        g0, _ = grad(c, c["theta"].astype(np.float64), 0, np.float64)
        delta = _f32(0.25 * np.abs(g0).max())
        stages, rule = _chain(name, 1e30, delta, LR[path])
        if any(s[0] == "clipnorm" for s in stages):
            omega = tune_omega(lambda w: run_twin(c, *_chain(name, w, delta, LR[path]), np.float64)[1])
            stages, rule = _chain(name, omega, delta, LR[path])
        _TUNED[key] = (stages, rule)
    return _TUNED[key]


def trajectory(path, name, dtype):
    """NSTEPS steps of the twin in dtype on the oracle's gradient in dtype -> (theta, ChainTwin)"""
    key = (path, name, np.dtype(dtype).name)
    if key not in _TRAJ:
        stages, rule = chain(path, name)
        th, tw = run_twin(case(path), stages, rule, dtype)
        th.setflags(write=False)
        _TRAJ[key] = (th, tw)
    return _TRAJ[key]
