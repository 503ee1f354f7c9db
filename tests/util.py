"""Shared helpers for the tests: oracle spec <-> package model, standard cases."""
import os

import numpy as np

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho

MECH_NAME = {"rbq10": "RbQ10", "expo": "Expo_resp_model", "linear": "LinearHM", "expo2pool": "Expo2Pool",
             "rs_components": "Rs_components", "rs_components3f": "Rs_components3F", "fluxpart": "FluxPartModelQ10"}


def register_closure(name, fn, params, forcings, targets):
    """A user closure as mechanistic model `name` on both sides: the package records it when the model is constructed
    (MECH_NAME[name] = the callable); the oracle gets the recorded program as plain data plus the closure itself."""
    from easyhybrid_jl_amd.program import trace
    prog = trace(fn, list(params), list(forcings), list(targets))
    MECH_NAME[name] = fn
    return ho.program_mech(name, prog.as_dict(), fn)


def register_loss(name, fn):
    """A custom training loss on both sides: returns what the package takes (the callable); the oracle gets the recorded
    per-sample program plus the function itself under training-loss kind `name`."""
    from easyhybrid_jl_amd.program import trace_loss
    wrapped = fn
    if name == "relative_sq":                        # (a function that returns per-sample terms: the oracle needs the scalar)
        wrapped = lambda yh, y: np.mean(fn(yh, y))
    ho.loss_program(name, trace_loss(fn).as_dict(), wrapped)
    return fn


def model_from_spec(spec: ho.HybridSpec):
    mm = ho.MECH[spec.mech][0]
    if spec.nets is not None:
        preds = {n: [f"x{i}" for i in rows] for n, (rows, _) in zip(spec.neural, spec.nets)}
        hl = {n: list(h) for n, (_, h) in zip(spec.neural, spec.nets)}
        return eh.constructHybridModel(preds, list(mm.forcings), list(spec.targets), MECH_NAME[spec.mech], dict(spec.parameters),
                                       list(spec.glob), hidden_layers=hl,
                                       activation=spec.activation if spec.net_activations is None else dict(zip(spec.neural, spec.net_activations)),
                                       scale_nn_outputs=spec.scale_nn_outputs, input_batchnorm=getattr(spec, "input_batchnorm", False),
                                       precision=getattr(spec, "precision", "f32"))
    hidden, act = list(spec.hidden), spec.activation
    if getattr(spec, "layer_activations", None) is not None:      # hidden_layers::Chain: the first hidden layer takes the model's activation, the others their own
        la = spec.layer_activations
        act = la[0]
        hidden = eh.Chain(*[eh.Dense(hidden[i], hidden[i + 1], la[i + 1]) for i in range(len(hidden) - 1)]) if len(hidden) > 1 else hidden
    return eh.constructHybridModel([f"x{i}" for i in range(spec.n_pred)], list(mm.forcings), list(spec.targets),
                                   MECH_NAME[spec.mech], dict(spec.parameters), list(spec.neural), list(spec.glob),
                                   hidden_layers=hidden, activation=act,
                                   scale_nn_outputs=spec.scale_nn_outputs, input_batchnorm=getattr(spec, "input_batchnorm", False),
                                   precision=getattr(spec, "precision", "f32"))


def load_engine(spec, theta, X, forcings, targets, split=0, engine=None):
    mm = ho.MECH[spec.mech][0]
    eng = engine or model_from_spec(spec).engine()
    # the parity tests are about the generic kernels and the ones compiled at run time; the kernels specialised AHEAD of time for the
    # canonical descriptors (csrc/eh_spec.hip) have their own tests (tests/test_gpu_headline.py, and every train() front-door test runs them)
    eng.set_option("aot_spec", 0)
    if spec.nets is not None:                         # the per-net predictor matrices stacked row-wise
        X = np.concatenate([X[rows] for rows, _ in spec.nets], axis=0)
    eng.set_data(split, X, [forcings[f] for f in mm.forcings], [targets[t] for t in spec.targets])
    eng.set_params(np.asarray(theta, np.float32))
    return eng


def relerr(a, b):
    """max |a - b| over max |b|: the error of the largest entries (what a norm-wise bound sees)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def elem_relerr(a, b, floor_frac=1e-3):
    """element-wise relative error max_i |a_i - b_i| / max(|b_i|, floor), floor = floor_frac * max |b|: every entry that is not
    tiny against the largest one has to be right to the stated number of digits on its own"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    floor = max(floor_frac * float(np.max(np.abs(b))), 1e-30)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


# ---- the gradient leaf by leaf: one weight matrix, one bias vector, one global parameter at a time ------------------------------------
def leaf_table(spec: ho.HybridSpec):
    """[(name, start, stop)] over flat theta: the leaves of model_from_spec(spec).leaves() -- the layout tests/test_plan.py holds against
    the device plan -- in order, then one row per global parameter; the last stop is spec.n_theta"""
    table, off = [], 0
    for k, li, name, shape in model_from_spec(spec).leaves():
        n = int(np.prod(shape))
        net = spec.neural[k] if spec.nets is not None else "nn"
        table.append((f"{net}.layer_{li + 1}.{name}", off, off + n))
        off += n
    for g in spec.glob:
        table.append((g, off, off + 1))
        off += 1
    assert off == spec.n_theta, (off, spec.n_theta)
    return table


def leaf_errors(g, g64, table, floor=1e-3):
    """per leaf: max |g - g64| over the leaf / max(max |g64| over the leaf, floor * max |g64| overall) -- relerr() of every leaf on its own
    size; the floor (elem_relerr's default) makes the check of a dead leaf absolute"""
    g = np.asarray(g, np.float64); g64 = np.asarray(g64, np.float64)
    gmax = float(np.max(np.abs(g64))) if g64.size else 0.0
    return [float(np.max(np.abs(g[a:b] - g64[a:b])) / max(float(np.max(np.abs(g64[a:b]))), floor * gmax, 1e-300)) for _, a, b in table]


def leaf_shares(g64, table):
    """per leaf: its largest entry over the largest entry of the whole gradient"""
    g64 = np.asarray(g64, np.float64)
    gmax = max(float(np.max(np.abs(g64))), 1e-300)
    return [float(np.max(np.abs(g64[a:b]))) / gmax for _, a, b in table]


REF32_ORDERS = 3          # seeded permutations of the samples besides the given order: four summation orders


def ref32_orders(spec, theta, X, f, y, n_perm=REF32_ORDERS, **kw):
    """the closure check_gradient() takes as `ref32`: the oracle's gradient in dtype=np.float32 on the batch in its given order and in
    n_perm seeded permutations of its samples; **kw is what the test passes to the oracle itself (kind, bn_state, l2, agg, extra)"""
    def run():
        B = X.shape[1]
        out = []
        for p in range(n_perm + 1):
            ix = np.arange(B) if p == 0 else np.random.default_rng(4242 + p).permutation(B)
            _, g32, _ = ho.loss_and_grad(spec, np.asarray(theta, np.float32), X[:, ix], {k: v[ix] for k, v in f.items()},
                                         {k: v[ix] for k, v in y.items()}, dtype=np.float32, **kw)
            out.append(np.asarray(g32, np.float64))
        return out
    return run


def ref32_leaf_errors(ref32, g64, table, floor=1e-3):
    """e32 per leaf: the largest of the leaf errors of the fp32 oracle's orders against the fp64 gradient"""
    return [max(es) for es in zip(*[leaf_errors(g, g64, table, floor) for g in ref32()])]


def _leaf_log(line):
    path = os.environ.get("EH_LEAF_LOG")          # a measuring run keeps every case's worst leaf; unset, nothing is written
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def check_gradient(grad, g64, spec, bar, ref32, floor=1e-3):
    """Every leaf of `grad` against the fp64 oracle's on the leaf's own size: a leaf passes at leaf_errors() <= bar; only for the leaves that
    miss, ref32() is evaluated (at most once) and the leaf passes at <= 4 e32, e32 what the oracle itself loses on that leaf in fp32 over its
    summation orders -- the factor tests/test_gpu_fuzz.py puts on the whole gradient.  Fails naming the leaf, its share of the global
    maximum, the device error and e32."""
    table = leaf_table(spec)
    assert np.asarray(grad).shape == np.asarray(g64).shape == (spec.n_theta,), (np.shape(grad), np.shape(g64), spec.n_theta)
    errs = leaf_errors(grad, g64, table, floor)
    share = leaf_shares(g64, table)
    miss = [i for i, e in enumerate(errs) if not e <= bar]
    e32, bad = None, []
    if miss:
        e32 = ref32_leaf_errors(ref32, g64, table, floor)
        bad = [i for i in miss if not errs[i] <= 4.0 * e32[i]]
    if os.environ.get("EH_LEAF_LOG"):
        e32 = e32 or ref32_leaf_errors(ref32, g64, table, floor)
        w = max(range(len(errs)), key=lambda i: errs[i] / max(bar, 4.0 * e32[i]))
        _leaf_log(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]} | worst leaf {table[w][0]} | device {errs[w]:.3e} | e32 {e32[w]:.3e} | "
                  f"share {share[w]:.3e} | bar {bar:g} | floor {floor:g} | leaves {len(errs)} | escaped {len(miss) - len(bad)} | failed {len(bad)}")
    assert not bad, "; ".join(f"leaf {table[i][0]} (share of the global maximum {share[i]:.2e}): device {errs[i]:.3e} > bar {bar:g} and > 4 x e32 = 4 x {e32[i]:.3e}"
                              for i in bad)


def rbq10_case(B, act="tanh", scale=False, nan_frac=0.0, seed=42, hidden=(16, 16), theta_seed=1):
    spec = ho.rbq10_spec(hidden, act, scale)
    X, f, y = ho.make_synth_rbq10(B, seed, nan_frac)
    X = (X / np.float32(50.0)).astype(np.float32)      # keep activations out of saturation for a sharp test
    theta = ho.init_theta(spec, theta_seed, np.float32)
    return spec, theta, X, f, y


# ---- eh_eval's metrics against a reference set (tests/test_gpu_eval.py, tests/test_oracle_selfcheck.py) --------------------------------
METRICS = ("mse", "rmse", "mae", "sse", "r2", "nse", "pearson", "kge", "pbkge", "alpha", "beta")
REL_METRICS = ("mse", "rmse", "mae", "sse", "alpha", "beta")          # relative bars
ABS_METRICS = ("r2", "nse", "pearson", "kge", "pbkge")                 # absolute bars (values near 0 or 1)


def metric_mismatches(got, ref, rel, abs_=None, keys=METRICS):
    """[(metric, got, ref)] of the metrics outside their bar, n exactly included.  abs_ = None: every metric relative to `rel` (floor
    1e-12), the ABS_METRICS absolute to `rel`; abs_ given: pytest.approx(ref, rel=rel, abs=abs_) on every metric.  A non-finite reference
    value must be matched exactly: NaN by NaN, an infinity by the same infinity."""
    bad = []
    if float(got["n"]) != float(ref["n"]):
        bad.append(("n", got["n"], ref["n"]))
    for k in keys:
        g, r = float(got[k]), float(ref[k])
        if not np.isfinite(r) or not np.isfinite(g):
            if not ((np.isnan(r) and np.isnan(g)) or g == r):
                bad.append((k, g, r))
            continue
        tol = max(rel * abs(r), abs_) if abs_ is not None else (rel if k in ABS_METRICS else max(rel * abs(r), 1e-12))
        if abs(g - r) > tol:
            bad.append((k, g, r))
    return bad
