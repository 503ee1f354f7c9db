"""Shared by tests/test_activations.py and tests/test_gpu_activations.py: the activation closures with their derivatives written out by
hand, the model cases, and the two bridges the tests need -- the oracle's act_fwd / act_bwd serving these closures by name (the oracle
looks the two functions up as module globals at call time, so a pytest `monkeypatch` is enough), and the package model of a spec
whose activations are such names."""
import contextlib
import dataclasses
import functools

import numpy as np

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho

from tests import util


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def leakyrelu02(x):
    return np.where(x > 0.0, x, 0.2 * x)


_G = 0.7978845608028654      # sqrt(2 / pi)

# name -> (the closure in NumPy, its derivative by hand in NumPy, the kinks of the derivative).  At a kink the hand derivative takes the
# side the closure's own `where` / `clip` takes, which is what the reverse sweep over its tape gives.
ACT_CASES = {
    "square": (lambda x: x ** 2, lambda x: 2.0 * x, ()),
    "softplus": (eh.softplus, lambda x: _sig(x), ()),
    "elu": (eh.elu, lambda x: np.where(x > 0.0, 1.0, np.exp(np.minimum(x, 0.0))), (0.0,)),      # (the derivative is continuous there, the second is not)
    "leakyrelu": (eh.leakyrelu, lambda x: np.where(x > 0.0, 1.0, 0.01), (0.0,)),
    "gelu_tanh": (eh.gelu_tanh, lambda x: 0.5 * (1.0 + np.tanh(_G * (x + 0.044715 * x ** 3)))
                  + 0.5 * x * (1.0 - np.tanh(_G * (x + 0.044715 * x ** 3)) ** 2) * _G * (1.0 + 3 * 0.044715 * x ** 2), ()),
    "hard_sigmoid": (eh.hard_sigmoid_act, lambda x: np.where((0.2 * x + 0.5 >= 0.0) & (0.2 * x + 0.5 <= 1.0), 0.2, 0.0), (-2.5, 2.5)),
    "xsin": (lambda x: x * np.sin(x), lambda x: np.sin(x) + x * np.cos(x), ()),
    "tanh_twin": (lambda z: np.tanh(z), lambda x: 1.0 - np.tanh(x) ** 2, ()),
    "sigmoid_twin": (lambda z: 1 / (1 + np.exp(-z)), lambda x: _sig(x) * (1.0 - _sig(x)), ()),
    "leakyrelu02": (leakyrelu02, lambda x: np.where(x > 0.0, 1.0, 0.2), (0.0,)),
}
BUILTIN = ("tanh", "sigmoid", "relu", "swish", "identity")


def closure(name):
    """what the package takes for activation `name`: the closure of a case, the string of a built-in"""
    return ACT_CASES[name][0] if name in ACT_CASES else name


def _oracle_acts():
    fwd0, bwd0 = ho.act_fwd, ho.act_bwd

    def fwd(name, z):
        return np.asarray(ACT_CASES[name][0](z)).astype(z.dtype) if name in ACT_CASES else fwd0(name, z)

    def bwd(name, z, h):
        return np.asarray(ACT_CASES[name][1](z)).astype(z.dtype) if name in ACT_CASES else bwd0(name, z, h)
    return fwd, bwd


def patch_oracle(monkeypatch):
    """ho.act_fwd / ho.act_bwd answer the case names next to their own five, in the dtype they are called in"""
    fwd, bwd = _oracle_acts()
    monkeypatch.setattr(ho, "act_fwd", fwd)
    monkeypatch.setattr(ho, "act_bwd", bwd)


@contextlib.contextmanager
def oracle_acts():
    """the same outside a test function (the shared references below)"""
    saved = ho.act_fwd, ho.act_bwd
    ho.act_fwd, ho.act_bwd = _oracle_acts()
    try:
        yield
    finally:
        ho.act_fwd, ho.act_bwd = saved


# ---- model cases: RbQ10, scale_nn_outputs = True, 10 % NaN targets ------------------------------------------------------------------
# id -> dict(hidden, acts[, bn]) for one network (acts: one per hidden layer; "all": activation=f for every layer), dict(nets, acts) for MultiNN
MODEL_CASES = {
    "16x16_softplus_elu": dict(hidden=[16, 16], acts=["softplus", "elu"]),                                     # per-wave kernel, the headline shape
    "16x16_softplus_all": dict(hidden=[16, 16], acts=["softplus", "softplus"], all=True),                      # activation = f: nothing collapses
    "24_square": dict(hidden=[24], acts=["square"], all=True),                                                 # one hidden layer
    "16x32x8_leaky_tanh_square_bn": dict(hidden=[16, 32, 8], acts=["leakyrelu", "tanh", "square"], bn=True),   # three widths, recorded next to built-in
    "64x48_gelu_softplus": dict(hidden=[64, 48], acts=["gelu_tanh", "softplus"]),                              # the 64-wide kernel
    "96x120_elu_square": dict(hidden=[96, 120], acts=["elu", "square"]),                                       # row-split
    "nets_softplus_sigmoid": dict(nets=[([0], [24, 12]), ([1, 2, 3], [30, 20])], acts=["softplus", "sigmoid"]),   # a net boundary inside a 16-row block
    "nets_square_elu_depths": dict(nets=[([0, 1], [16, 8]), ([2], [8])], acts=["square", "elu"]),              # the shallower net on identity blocks
}


def make_spec(case):
    c = MODEL_CASES[case] if isinstance(case, str) else case
    if "nets" in c:
        return ho.HybridSpec(4, [1], "rbq10", dict(ho.RBQ10_PARAMS), ["rb", "Q10"], [], ["reco"], c["acts"][0], True, nets=c["nets"], net_activations=list(c["acts"]))
    spec = ho.HybridSpec(3, list(c["hidden"]), "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], c["acts"][0], True,
                         layer_activations=None if c.get("all") else list(c["acts"]))
    spec.input_batchnorm = bool(c.get("bn", False))
    return spec


def make_data(spec, B, seed=12):
    """inputs as test_single_network_with_an_activation_per_layer / test_multinn_per_network_activations make them"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((spec.n_pred, B)).astype(np.float32)
    f = {"ta": rng.uniform(0, 30, B).astype(np.float32)}
    yv = rng.uniform(1, 9, B).astype(np.float32)
    yv[rng.random(B) < 0.1] = np.nan
    return X, f, {"reco": yv}, ho.init_theta(spec, 8, np.float32)


NSTEPS = 7


def batches_of(B):
    n = min(160, B // NSTEPS) if B >= 10 * NSTEPS else B
    return [(i * n, n) for i in range(NSTEPS)] if n < B else [(0, B)] * NSTEPS


@functools.lru_cache(maxsize=None)
def reference(case, B, seed=12):
    """the oracle's answers for a model case, computed once per session and shared: inputs, fp64 loss / gradient / forward / mse, the fp32
    ones, and the Adam trajectory of batches_of(B) in fp32 (what the device is held against) and in fp64"""
    spec = make_spec(case)
    X, f, y, theta = make_data(spec, B, seed)
    with oracle_acts():
        th64 = theta.astype(np.float64)
        l64, g64, nv = ho.loss_and_grad(spec, th64, X, f, y)
        l32, g32, _ = ho.loss_and_grad(spec, theta, X, f, y, dtype=np.float32)
        # (input BatchNorm: a fresh engine's forward / eval run in test mode on the initial running statistics)
        fwd = ho.forward(spec, th64, X, f, bn_state=ho.bn_init(spec), train_mode=False) if spec.input_batchnorm else ho.forward(spec, th64, X, f)
        yy = y["reco"].astype(np.float64)
        mse = ho.loss_fn(fwd["reco"], yy, ~np.isnan(yy), "mse")
        bt = batches_of(B)
        t32, ls32 = ho.train_steps(spec, theta, X, f, y, bt, dtype=np.float32)
        t64, _ = ho.train_steps(spec, th64, X, f, y, bt, dtype=np.float64)
    return dict(spec=spec, X=X, f=f, y=y, theta=theta, l64=l64, g64=g64, nv=sum(nv), l32=l32, g32=g32, fwd=fwd, mse=mse, batches=bt,
                t32=np.asarray(t32), t64=np.asarray(t64), losses32=ls32)


MODEL_RUNS = [(c, 300) for c in MODEL_CASES] + [("16x16_softplus_elu", 65)]      # (B = 65: one sample past a 64-sample tile)


def model_from_spec(spec, **kw):
    """util.model_from_spec for a spec whose activations may be case names: those go to the package as closures"""
    if spec.nets is not None:
        preds = {n: [f"x{i}" for i in rows] for n, (rows, _) in zip(spec.neural, spec.nets)}
        hl = {n: list(h) for n, (_, h) in zip(spec.neural, spec.nets)}
        act = closure(spec.activation) if spec.net_activations is None else {n: closure(a) for n, a in zip(spec.neural, spec.net_activations)}
        return eh.constructHybridModel(preds, ["ta"], list(spec.targets), eh.RbQ10, dict(spec.parameters), list(spec.glob), hidden_layers=hl, activation=act,
                                       scale_nn_outputs=spec.scale_nn_outputs, input_batchnorm=spec.input_batchnorm, **kw)
    hidden, act = list(spec.hidden), closure(spec.activation)
    if spec.layer_activations is not None:
        la = spec.layer_activations
        act = closure(la[0])
        hidden = eh.Chain(*[eh.Dense(hidden[i], hidden[i + 1], closure(la[i + 1])) for i in range(len(hidden) - 1)]) if len(hidden) > 1 else hidden
    return eh.constructHybridModel([f"x{i}" for i in range(spec.n_pred)], ["ta"], list(spec.targets), eh.RbQ10, dict(spec.parameters), list(spec.neural),
                                   list(spec.glob), hidden_layers=hidden, activation=act, scale_nn_outputs=spec.scale_nn_outputs,
                                   input_batchnorm=spec.input_batchnorm, **kw)


def layout_spec(spec):
    """the same spec with built-in activation names: what util.check_gradient reads the leaf table from (the layout does not depend on them)"""
    return dataclasses.replace(spec, activation="tanh", layer_activations=None if spec.layer_activations is None else ["tanh"] * len(spec.layer_activations),
                               net_activations=None if spec.net_activations is None else ["tanh"] * len(spec.net_activations))


def load_engine(spec, theta, X, f, y, model=None):
    return util.load_engine(spec, theta, X, f, y, engine=(model or model_from_spec(spec)).engine())


def act_structs(names):
    """the eh_act_program array of the cases `names`, through the package's own recorder"""
    from easyhybrid_jl_amd import _lib as L
    from easyhybrid_jl_amd.program import trace_activation
    arr = (L.ActProgram * len(names))()
    for j, n in enumerate(names):
        pg = trace_activation(ACT_CASES[n][0])
        arr[j].n_instr, arr[j].n_const, arr[j].out_slot = len(pg.code), len(pg.consts), pg.out[0]
        for i, w in enumerate(pg.words()):
            arr[j].code[i] = w
        for i, c in enumerate(pg.consts):
            arr[j].consts[i] = c
    return arr
