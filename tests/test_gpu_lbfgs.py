"""L-BFGS on the device (csrc/eh_lbfgs.hpp) against its NumPy twin (tests/lbfgs_twin.py) on the oracle's fp64 loss and
gradient: the same line-search decisions, step lengths to 1e-5 relative, parameters within the project's trajectory bar
3e-5 * max(1, max |theta_ref|) (tests/test_gpu_parity.py) -- after the twin's own fp32 run has been held to a tenth of it, the pattern of
tests/test_gpu_seq.py.  Then the invariants of a longer solve, both launch forms, a sequence model, reproducibility, the edge cases and
the train() front door."""
import sys
import warnings

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
import easyhybrid_jl_amd.train  # noqa: F401
from oracle import hybrid_oracle as ho

from tests import lbfgs_twin as tw
from tests import seq_twin
from tests import util

pytestmark = pytest.mark.gpu

BAR, T_REL = 3e-5, 1e-5
RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}

_CASES, _TWIN = {}, {}


def case(k):
    """(spec, theta, X, forcings, targets), computed once and left unchanged"""
    if k not in _CASES:
        if k == 1:
            _CASES[k] = util.rbq10_case(512, act="tanh", scale=True, nan_frac=0.1)
        elif k == 2:
            _CASES[k] = util.rbq10_case(300, act="sigmoid", scale=True, nan_frac=0.1, hidden=(8,))
        else:          # a layer-wise net: 66 k parameters, 66 workgroups in the dots kernel
            _CASES[k] = util.rbq10_case(256, act="tanh", scale=True, nan_frac=0.1, hidden=(256, 256))
    return _CASES[k]


def oracle_fg(c):
    spec, _, X, f, y = c

    def fg(x):
        l, g, nv = ho.loss_and_grad(spec, np.asarray(x, np.float64), X, f, y)
        return l, g, float(sum(nv))
    return fg


def twin(k, iters, dtype=np.float64, **kw):
    key = (k, iters, np.dtype(dtype).name, tuple(sorted(kw.items())))
    if key not in _TWIN:
        c = case(k)
        _TWIN[key] = tw.lbfgs(oracle_fg(c), c[1], iters, dtype=dtype, **kw)
    return _TWIN[key]


def engine(k):
    spec, theta, X, f, y = case(k)
    return util.load_engine(spec, theta, X, f, y)


def solve(eng, iters, extra=0, **kw):
    eng.lbfgs_init(**kw)
    eng.lbfgs_set_batch()
    st = eng.lbfgs_solve(iters)
    if extra:
        eng.lbfgs_run(extra)
        st = eng.lbfgs_status()
    return st, eng.lbfgs_trace(), eng.get_params()


def against_twin(st, trace, theta, ref, ref32, what):
    """device against the fp64 twin `ref`, after the twin's fp32 run `ref32` has been held to a tenth of the bar"""
    scale = max(1.0, float(np.abs(ref.theta).max()))
    e32 = float(np.abs(ref32.theta.astype(np.float64) - ref.theta).max())
    assert [(t["decisions"], t["trials"]) for t in ref32.trace] == [(t["decisions"], t["trials"]) for t in ref.trace]
    assert e32 <= 0.1 * BAR * scale, e32
    err = float(np.abs(theta.astype(np.float64) - ref.theta).max())
    trel = max(abs(a["t"] - b["t"]) / b["t"] for a, b in zip(trace, ref.trace))
    print(f"{what}: iterations {st['iterations']} evaluations {st['evaluations']} ({ref.evaluations})  decisions {[t['decisions'] for t in trace]}  "
          f"t rel {trel:.2e}  theta err {err:.2e} (twin fp32 {e32:.2e}, bar {BAR * scale:.2e})  f {st['f0']:.6f} ({ref.f:.6f})")
    assert st["iterations"] == ref.iterations and st["evaluations"] == ref.evaluations and st["status"] == ref.status
    assert [(t["decisions"], t["trials"]) for t in trace] == [(t["decisions"], t["trials"]) for t in ref.trace]
    assert trel <= T_REL
    assert err <= BAR * scale
    assert abs(st["f0"] - ref.f) <= 1e-5 * abs(ref.f)


@pytest.mark.parametrize("k", [1, 2])
def test_trajectory_against_the_twin(k):
    eng = engine(k)
    st, trace, theta = solve(eng, 5)
    against_twin(st, trace, theta, twin(k, 5), twin(k, 5, np.float32), f"case {k}")
    if k == 1:
        assert "A" in trace[2]["decisions"]                       # the backtracking branch
    # the expansion branch: t doubles from 1e-4 until the curvature test passes
    eng.set_params(case(k)[1])
    st, trace, theta = solve(eng, 6, initial_step=1e-4)
    against_twin(st, trace, theta, twin(k, 6, initial_step=1e-4), twin(k, 6, np.float32, initial_step=1e-4), f"case {k}, initial_step 1e-4")
    assert trace[0]["decisions"].startswith("C")
    eng.close()


def test_invariants_over_30_iterations():
    eng = engine(1)
    st, trace, theta = solve(eng, 30)
    ref = twin(1, 30)
    fs = [t["f"] for t in trace]
    print(f"30 iterations: f {fs[0]:.4f} -> {st['f0']:.6f} (twin {ref.f:.6f}), {st['evaluations']} evaluations (twin {ref.evaluations}), status {st['status']}")
    assert st["iterations"] == len(trace) == 30 and st["status"] == "maxiters"
    assert all(b <= a for a, b in zip(fs, fs[1:]))
    assert all(t["sy"] > 0 for t in trace)
    assert st["evaluations"] <= st["iterations"] * 20 + 1 and trace[-1]["evaluations"] == st["evaluations"]
    assert st["f0"] <= 1.05 * ref.f
    assert 1 <= st["pairs"] <= 10
    eng.close()


def test_many_workgroups_and_both_launch_forms():
    k = 3
    ref, ref32 = twin(k, 3), twin(k, 3, np.float32)
    out = []
    for one_max in (-1, 0, 1 << 20):                  # the default, always three kernels, always one launch
        eng = engine(k)
        assert eng.n_theta > 60000
        eng.set_option("lbfgs_one_max", one_max)
        st, trace, theta = solve(eng, 3)
        eng.close()
        against_twin(st, trace, theta, ref, ref32, f"hidden (256, 256), lbfgs_one_max {one_max}")
        out.append((st, trace, theta))
    assert np.array_equal(out[1][2], out[2][2]) and out[1][0] == out[2][0] and out[1][1] == out[2][1]
    assert np.array_equal(out[0][2], out[1][2])


def test_sequence_model():
    I, H, W, ow, lam, count = 15, 15, 10, 1, 0, 128
    model = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"],
                                    hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(I, H))), activation="tanh", scale_nn_outputs=True)
    rng = np.random.default_rng(1236)
    rows = 160
    X = (0.6 * rng.standard_normal((2, rows))).astype(np.float32)
    X[0] = np.cumsum(X[0]) * 0.2
    ta = (10 + 8 * rng.standard_normal(rows)).astype(np.float32)
    y = ((3.0 + np.tanh(X[0])) * 2.0 ** (0.1 * (ta - 15.0)) + 0.1 * rng.standard_normal(rows)).astype(np.float32)
    y[rng.random(rows) < 0.1] = np.nan
    starts = np.arange(0, rows - W - lam + 1, dtype=np.int32)[:count]
    theta0 = model.initialparameters(10)
    assert theta0.size == 2222 and starts.size == count

    def fg_of(dtype):
        def fg(x):
            return seq_twin.loss_and_grad(model, np.asarray(x), X, {"ta": ta}, y, starts, W, ow, lam, "mse", dtype)
        return fg
    ref = tw.lbfgs(fg_of(torch.float64), theta0, 3)
    ref32 = tw.lbfgs(fg_of(torch.float32), theta0, 3, dtype=np.float32)
    eng = model.engine(0)
    eng.set_data(L.EH_SPLIT_TRAIN, X, [ta], [y])
    eng.set_sequences(L.EH_SPLIT_TRAIN, W, ow, lam, starts)
    eng.set_params(theta0)
    st, trace, theta = solve(eng, 3)
    eng.close()
    against_twin(st, trace, theta, ref, ref32, "sequence model")


def test_reproducible_and_surplus_evaluations_are_harmless():
    runs = []
    for extra in (0, 0, 7):
        eng = engine(1)
        st, trace, theta = solve(eng, 8, extra=extra)
        runs.append((st, trace, theta, eng.loss_and_grad()[:2]))
        eng.close()
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and np.array_equal(r[2], runs[0][2])
        assert r[3][0] == runs[0][3][0] and np.array_equal(r[3][1], runs[0][3][1])      # the kernels read the image: same image, same bits
    assert runs[0][0]["status"] == "maxiters" and runs[0][0]["iterations"] == 8


def test_edge_cases():
    spec, theta0, X, f, y = case(1)
    eng = engine(1)
    eng.lbfgs_init()
    eng.lbfgs_set_batch()
    st = eng.lbfgs_solve(0)                           # maxiters = 0: the starting point is evaluated, nothing moves
    assert st["status"] == "maxiters" and st["iterations"] == 0 and st["evaluations"] == 1
    assert np.array_equal(eng.get_params(), theta0)
    l0 = eng.loss_and_grad()[0]
    assert st["f0"] == pytest.approx(l0, rel=1e-6)
    eng.close()
    # no valid target in the batch: "empty batch", theta and the image untouched
    ynan = {t: np.full_like(v, np.nan) for t, v in y.items()}
    eng = util.load_engine(spec, theta0, X, f, ynan)
    eng.lbfgs_init()
    eng.lbfgs_set_batch()
    st = eng.lbfgs_solve(5)
    assert st["status"] == "empty batch" and st["iterations"] == 0
    assert np.array_equal(eng.get_params(), theta0)
    ref = util.load_engine(spec, theta0, X, f, y)
    eng.set_data(L.EH_SPLIT_TRAIN, X, [f["ta"]], [y["reco"]])
    a, b = eng.loss_and_grad(), ref.loss_and_grad()
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    # opt_init returns the handle to the Optimisers path: an Adam step equals the bits of a handle that never saw L-BFGS
    eng.lbfgs_init()
    with pytest.raises(NotImplementedError, match="L-BFGS"):
        eng.graph_begin()
    for e in (eng, ref):
        e.opt_init("Adam", 0.01)
    la, lb = eng.train_step(0, 512), ref.train_step(0, 512)
    assert la == lb and np.array_equal(eng.get_params(), ref.get_params())
    with pytest.raises(RuntimeError, match="eh_lbfgs_init"):
        eng.lbfgs_run(1)
    eng.close(); ref.close()


def test_train_front_door():
    data = eh.synthetic.make_synth_rbq10(2000, 11, 0.05)

    def model(**kw):
        return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"],
                                       hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True, **kw)
    res = eh.train(model(), data, opt=eh.LBFGS(), full_batch=True, maxiters=40, eval_every=10, random_seed=3)
    val = [h["mse"]["sum"] for h in res.val_history]
    print(f"full batch: validation mse {val}, status {res.lbfgs_status}")
    assert len(res.val_history) == 5 and len(res.train_history) == 5
    assert res.best_loss == min(val) and res.best_epoch == 10 * int(np.argmin(val))
    assert val[-1] < 0.5 * val[0]
    assert res.lbfgs_status["iterations"] == 40 == len(res.lbfgs_trace) and res.lbfgs_status["evaluations"] <= 40 * 20 + 1
    res.release()
    res = eh.train(model(), data, opt=eh.LBFGS(), full_batch=False, nepochs=2, batchsize=512, inner_maxiters=4, random_seed=3, maxiters=7)
    val = [h["mse"]["sum"] for h in res.val_history]
    print(f"minibatches: validation mse {val}, status {res.lbfgs_status}")
    assert len(res.val_history) == 3 and res.lbfgs_status["iterations"] <= 4 and val[-1] < val[0]
    res.release()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = eh.train(model(), data, opt=eh.LBFGS(m=4), full_batch=True, maxiters=3, promote_f64=True, random_seed=3)
    assert len([x for x in w if "promote_f64" in str(x.message)]) == 1 and res.lbfgs_status["pairs"] <= 3
    res.release()
    # refusals on a live handle
    eng = model().engine(0)
    eng.set_dropout([0.2, 0.0])
    with pytest.raises(NotImplementedError, match="dropout"):
        eng.lbfgs_init()
    eng.close()
    eng = model(input_batchnorm=True).engine(0)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        eng.lbfgs_init()
    eng.close()
    eng = model().engine(0)
    with pytest.raises(ValueError):
        eng.lbfgs_init(m=17)
    with pytest.raises(ValueError):
        eng.lbfgs_init(c1=0.9, c2=0.5)
    eng.close()
    with pytest.raises(NotImplementedError, match="distributed"):
        eh.train(model(), data, opt=eh.LBFGS(), distributed=True)
