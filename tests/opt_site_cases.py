"""The cases of tests/test_gpu_opt_sites.py as data, with what the oracle says about each: the CPU file (tests/test_opt_sites.py) checks
the conditions on the inputs for every one of them, the GPU file runs them.  All models are RbQ10 hybrids (tanh unless said, sigma-scaled
outputs, Q10 global); a case is (model, minibatch, steps): step k trains on samples [k B, (k + 1) B).  Nothing here touches the GPU
but the engine() of a case, which only the GPU file calls."""
import functools

import numpy as np

from oracle import hybrid_oracle as ho
from tests import opt_site_twin as tw

F = np.float32
MODELS = {
    "headline": dict(P=2, hidden=(16, 16)),                         # [2, 16, 16, 1] + Q10: 338 parameters, per-wave kernels
    "w64": dict(P=32, hidden=(64, 64, 64)),                         # per-wave, n_acc >= 8192
    "w128": dict(P=2, hidden=(128, 128)),                           # row-split, n_acc >= 8192
    "lf4": dict(P=2, hidden=(160, 80, 40, 20)),                     # layer-wise; n_theta = 17 442 = 2 mod 4
    "lf4odd": dict(P=2, hidden=(160, 80, 41, 20)),                  # layer-wise; n_theta = 17 543 = 3 mod 4
    "lfswish": dict(P=2, hidden=(96, 80, 64, 48), act="swish"),     # layer-wise; tile edges off 32
    "lf129": dict(P=2, hidden=(129,)),                              # layer-wise by width, one hidden layer; a width that is no multiple of four
    # a second layer of more than 256 inputs stays outside the one-launch tail chain: its delta product takes the chain's side job, which
    # the 32 x 32 epilogue (eh_dw_apply64_kernel) waits for (eh_lform_train)
    "lf288": dict(P=2, hidden=(288, 80, 40, 20)),                   # tile edges off 32: 80, 40, 20
    "lf264s": dict(P=2, hidden=(264, 80, 48), act="swish"),
    "lf272p12": dict(P=12, hidden=(272, 64)),                       # twelve inputs: the first layer's product is a tiled one
    "tutorial": dict(P=2, hidden=(1024, 512, 256, 128, 64)),        # 700 418 parameters
}
MULTI_NETS = [([0, 1], [160, 80, 40]), ([2, 3], [144, 24])]          # a MultiNN model on the layer-wise form (widths above 128)
RULE_NAMES = ("Adam", "AdamW", "RMSProp", "Descent", "grouped")
STATE_SEED, GROUP_SEED = 11, 5

# (model, minibatch, steps) of every GPU case
CASES = [
    ("headline", 1, 1), ("headline", 64, 1), ("headline", 257, 1), ("headline", 257, 2), ("headline", 64, 2), ("headline", 4349, 1), ("headline", 4349, 2),
    ("w64", 257, 1), ("w128", 257, 1),
    ("lf4", 300, 1), ("lf4odd", 300, 1), ("lf4", 37, 1), ("lf4", 65, 1), ("lf4", 130, 1), ("lf4", 256, 1), ("lf129", 64, 1), ("tutorial", 37, 1),
    ("lf288", 48, 1), ("lf288", 64, 1), ("lf264s", 48, 1), ("lf264s", 64, 1), ("lf272p12", 48, 1), ("lf272p12", 64, 1), ("tutorial", 64, 1),
    ("lf4", 64, 1), ("lf4", 80, 1), ("lf4", 128, 1), ("lfswish", 64, 1), ("lfswish", 80, 1), ("lfswish", 128, 1),
    ("multi", 64, 1), ("bnchain", 64, 1), ("lnchain", 64, 1), ("lstm", 33, 1),
]


@functools.lru_cache(maxsize=None)
def model_spec(model):
    if model == "multi":
        return ho.HybridSpec(4, [1], "rbq10", dict(ho.RBQ10_PARAMS), ["rb", "Q10"], [], ["reco"], "tanh", True, nets=MULTI_NETS)
    d = MODELS[model]
    return ho.HybridSpec(d["P"], list(d["hidden"]), "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], d.get("act", "tanh"), True)


@functools.lru_cache(maxsize=None)
def data(model, n):
    """(spec, theta0, X, forcings, targets) with n samples; a tenth of the targets missing, the first sample never (a minibatch of one)"""
    spec = model_spec(model)
    X2, f, y = ho.make_synth_rbq10(n, 42, 0.1)
    X2 = (X2 / F(50.0)).astype(F)                       # (activations out of saturation, as tests/util.py rbq10_case)
    rng = np.random.default_rng(9)
    X = np.concatenate([X2, (0.5 * rng.standard_normal((spec.n_pred - 2, n))).astype(F)], axis=0) if spec.n_pred > 2 else X2
    if np.isnan(y["reco"][0]):
        y["reco"][0] = F(3.0)
    theta = ho.init_theta(spec, 1, F)
    for a in (X, theta, f["ta"], y["reco"]):
        a.setflags(write=False)
    return spec, theta, X, f, y


class SpecCase:
    """an oracle HybridSpec model: the NumPy oracle's fp32 and fp64 gradients; step k trains on samples [k B, (k + 1) B)"""
    def __init__(self, model, B, steps):
        self.model, self.B, self.steps = model, B, steps
        self.spec, self.theta0, self.X, self.f, self.y = data(model, B * steps)

    def grads(self, k, theta):
        sl = slice(k * self.B, (k + 1) * self.B)
        X, f, y = self.X[:, sl], {n: v[sl] for n, v in self.f.items()}, {n: v[sl] for n, v in self.y.items()}
        g32 = ho.loss_and_grad(self.spec, np.asarray(theta, F), X, f, y, np.float32)[1]
        g64 = ho.loss_and_grad(self.spec, np.asarray(theta, np.float64), X, f, y, np.float64)[1]
        return np.asarray(g32).astype(F), np.asarray(g64).astype(F)

    def engine(self, nan=False):
        from tests import util
        y = {k: np.full_like(v, np.nan) for k, v in self.y.items()} if nan else self.y
        return util.load_engine(self.spec, self.theta0, self.X, self.f, y)


RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}


def _series(P, rows, seed):
    rng = np.random.default_rng(seed)
    X = (0.8 * rng.standard_normal((P, rows))).astype(F)
    ta = (10 + 8 * rng.standard_normal(rows)).astype(F)
    y = ((3.0 + np.tanh(X[0] - X[0].mean())) * 2.0 ** (0.1 * (ta - 15.0)) + 0.1 * rng.standard_normal(rows)).astype(F)
    y[rng.random(rows) < 0.1] = np.nan
    return X, ta, y


class NormChainCase:
    """BatchNorm / LayerNorm layers inside the hidden-layer chain (layer-wise form): the torch twins' fp32 and fp64 gradients.  Every leaf
    is moved off its initial value, so that scale and bias of the norm layers are not 1 and 0"""
    def __init__(self, model, B, steps):
        import easyhybrid_jl_amd as eh
        from tests import bn_chain_twin, ln_chain_twin
        self.model, self.B, self.steps = model, B, steps
        if model == "bnchain":
            hl, self.tw = eh.Chain(eh.Dense(16, 17, "tanh"), eh.BatchNorm(17), eh.Dense(17, 8, "relu"), eh.BatchNorm(8, "sigmoid")), bn_chain_twin
        else:
            hl, self.tw = eh.Chain(eh.Dense(16, 17, "tanh"), eh.LayerNorm(17), eh.Dense(17, 8, "relu"), eh.LayerNorm(8, "sigmoid")), ln_chain_twin
        self.m = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=hl, activation="tanh",
                                         scale_nn_outputs=True)
        self.X, self.ta, self.y = _series(2, B * steps, 77)
        th = self.m.initialparameters(21)
        self.theta0 = (th + 0.1 * np.random.default_rng(21).standard_normal(th.size)).astype(F)

    def grads(self, k, theta):
        import torch
        rows = np.arange(k * self.B, (k + 1) * self.B)
        g = [self.tw.loss_and_grad(self.m, np.asarray(theta, F), self.X, {"ta": self.ta}, self.y, rows, "mse", dt)[1] for dt in (torch.float32, torch.float64)]
        return np.asarray(g[0]).astype(F), np.asarray(g[1]).astype(F)

    def engine(self, nan=False):
        e = self.m.engine(0)
        e.set_option("aot_spec", 0)
        e.set_data(0, self.X, [self.ta], [np.full_like(self.y, np.nan) if nan else self.y])
        e.set_params(self.theta0)
        return e


class SeqCase:
    """LSTMCell(4, 4) behind a Dense(2, 4), windows of 5 records: the torch twin's gradients; a sample is a window"""
    W, OW, LAM = 5, 1, 0

    def __init__(self, model, B, steps):
        import easyhybrid_jl_amd as eh
        self.model, self.B, self.steps = model, B, steps
        self.m = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"],
                                         hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(4, 4))), activation="tanh", scale_nn_outputs=True)
        n = B * steps
        self.X, self.ta, self.y = _series(2, n + self.W + self.LAM, 1234)
        self.X = self.X.copy()
        self.X[0] = np.cumsum(self.X[0]) * 0.2
        self.starts = np.arange(n, dtype=np.int32)
        self.theta0 = np.asarray(self.m.initialparameters(10), F)

    def grads(self, k, theta):
        import torch
        from tests import seq_twin
        sel = self.starts[k * self.B:(k + 1) * self.B]
        g = [seq_twin.loss_and_grad(self.m, np.asarray(theta, F), self.X, {"ta": self.ta}, self.y, sel, self.W, self.OW, self.LAM, "mse", dt)[1]
             for dt in (torch.float32, torch.float64)]
        return np.asarray(g[0]).astype(F), np.asarray(g[1]).astype(F)

    def engine(self, nan=False):
        e = self.m.engine(0)
        e.set_data(0, self.X, [self.ta], [np.full_like(self.y, np.nan) if nan else self.y])
        e.set_sequences(0, self.W, self.OW, self.LAM, self.starts)
        e.set_params(self.theta0)
        return e


@functools.lru_cache(maxsize=None)
def case(model, B, steps):
    return {"bnchain": NormChainCase, "lnchain": NormChainCase, "lstm": SeqCase}.get(model, SpecCase)(model, B, steps)


def rules_of(name, n):
    """(rules, group) of a rule name: one rule (a dict, no groups) or the grouped handle (four rules, a group per element)"""
    if name == "grouped":
        return tw.GROUPED, tw.random_groups(n, len(tw.GROUPED), GROUP_SEED)
    return tw.RULES[name], None


@functools.lru_cache(maxsize=None)
def first_grads(model, B, steps):
    """the oracle's gradients of step 0 at theta0: the same for every rule, computed once"""
    c = case(model, B, steps)
    return c.grads(0, c.theta0)


@functools.lru_cache(maxsize=None)
def reference(model, B, steps, rule_name):
    """What the oracle alone says about a case: the warm state, and per step the two gradients (fp32, fp64 sums, both as float32), the bar's
    first term and the twin's state after the step (fed the fp32 gradient)"""
    c = case(model, B, steps)
    theta0 = c.theta0
    n = theta0.size
    rules, group = rules_of(rule_name, n)
    g32, g64 = first_grads(model, B, steps)
    s = float(np.max(np.abs(g32)))
    m0, v0 = tw.warm_state(n, s, STATE_SEED)
    bt0 = tw.warm_products(rules)
    st = (theta0.copy(), m0, v0, bt0)
    per_step = []
    for k in range(steps):
        if k > 0:
            g32, g64 = c.grads(k, st[0])
        err = tw.self_error(rules, group, g32, g64, *st)
        nxt = tw.step(rules, group, g32, *st)
        per_step.append(dict(g32=g32, g64=g64, err=err, before=st, after=nxt))
        st = nxt
    return dict(rules=rules, group=group, theta0=theta0, m0=m0, v0=v0, bt0=bt0, s=s, steps=per_step)


def check_case_inputs(model, B, steps, rule_name):
    ref = reference(model, B, steps, rule_name)
    out = []
    for k, s in enumerate(ref["steps"]):
        out.append(tw.check_inputs(f"{model} B={B} step {k} {rule_name}", ref["rules"], ref["group"], s["g32"], s["g64"], *s["before"]))
    return out
