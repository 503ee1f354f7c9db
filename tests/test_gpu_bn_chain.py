"""BatchNorm layers inside hidden-layer chains on the device (csrc/eh_bnl.hpp, on the layer-wise form) against the torch twin
(tests/bn_chain_twin.py, fp64): loss and gradient, optimiser steps, the running statistics, test-mode evaluation and predictions, the
layer state, reproducibility, the train() front door, refusals on a live handle.

Tolerances are the project's own (tests/test_gpu_lform.py, tests/test_gpu_seq.py): loss and gradient norm within 1e-5 relative of the
fp64 twin, the worst entry within 1e-5 of the largest, entry by entry within 5e-4 down to 1e-3 of the largest entry.  Every parity check
first holds the twin's own fp32 run to a tenth of each bar: an ill-conditioned input fails as an input."""
import ctypes as C

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L

from tests import bn_chain_twin as tw
from tests import util

pytestmark = pytest.mark.gpu

TOL, ETOL, PTOL = 1e-5, 5e-4, 1e-5
ROWS = 400
RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}
EXPO = {"k": (0.01, 0.0, 0.2), "Resp0": (2.0, 0.0, 8.0)}
WIDTHS, COUNTS = [5, 16, 17, 130], [1, 5, 17, 64, 300]
POSITIONS = ["first", "last", "two", "noaffine", "activation"]


def chain_of(position, n):
    """the layer positions of the issue around width n (the second width: another remainder modulo 4, another column block count)"""
    m = {5: 8, 16: 17, 17: 12, 130: 16}[n]
    return {"first": lambda: eh.Chain(eh.BatchNorm(n), eh.Dense(n, m, "tanh")),
            "last": lambda: eh.Chain(eh.Dense(n, n, "swish"), eh.BatchNorm(n, "sigmoid")),
            "two": lambda: eh.Chain(eh.BatchNorm(n), eh.Dense(n, m, "tanh"), eh.BatchNorm(m, "relu")),
            "noaffine": lambda: eh.Chain(eh.Dense(n, n, "tanh"), eh.BatchNorm(n, "swish", affine=False), eh.Dense(n, m, "sigmoid")),
            "activation": lambda: eh.Chain(eh.BatchNorm(n, "tanh"), eh.Dense(n, n, "sigmoid"))}[position]()


def make_model(hl, mech="rbq10", act="tanh", scale=True, P=2, input_batchnorm=False):
    preds = [f"x{i}" for i in range(P)]
    if mech == "rbq10":
        return eh.constructHybridModel(preds, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=hl, activation=act,
                                       scale_nn_outputs=scale, input_batchnorm=input_batchnorm)
    return eh.constructHybridModel(preds, ["T"], ["Resp_obs"], eh.Expo_resp_model, dict(EXPO), ["Resp0", "k"], [], hidden_layers=hl, activation=act,
                                   scale_nn_outputs=scale, input_batchnorm=input_batchnorm)


_DATA = {}


def data(P=2, offset=False, nan_frac=0.1):
    """(X (P, ROWS), forcing, target): computed once per shape and left unchanged.  offset: the predictors sit 50 sigma from zero"""
    key = (P, offset, nan_frac)
    if key not in _DATA:
        rng = np.random.default_rng(77 + P)
        X = (0.8 * rng.standard_normal((P, ROWS))).astype(np.float32)
        if offset:
            X = (5.0 + 0.1 * X / 0.8).astype(np.float32)
        ta = (10 + 8 * rng.standard_normal(ROWS)).astype(np.float32)
        y = ((3.0 + np.tanh(X[0] - X[0].mean())) * 2.0 ** (0.1 * (ta - 15.0)) + 0.1 * rng.standard_normal(ROWS)).astype(np.float32)
        y[rng.random(ROWS) < nan_frac] = np.nan
        for a in (X, ta, y):
            a.setflags(write=False)
        _DATA[key] = (X, ta, y)
    return _DATA[key]


def theta_of(model, seed):
    """initial parameters, every leaf moved a little: scale and bias of the BatchNorm layers away from 1 and 0"""
    th = model.initialparameters(seed)
    return (th + 0.1 * np.random.default_rng(seed).standard_normal(th.size)).astype(np.float32)


def twin_pair(model, theta, X, ta, y, rows, kind):
    """(loss, gradient, n_valid) of the fp64 twin, and how far the twin's own fp32 run is from it in units of a TENTH of each bar"""
    f = {model.forcing[0]: ta}
    l64, g64, nv64 = tw.loss_and_grad(model, theta, X, f, y, rows, kind, torch.float64)
    l32, g32, _ = tw.loss_and_grad(model, theta, X, f, y, rows, kind, torch.float32)
    n64 = float(np.linalg.norm(g64))
    own = max(abs(l32 - l64) / abs(l64) / (0.1 * TOL), abs(float(np.linalg.norm(g32)) - n64) / n64 / (0.1 * TOL),
              util.relerr(g32, g64) / (0.1 * TOL), util.elem_relerr(g32, g64, 1e-3) / (0.1 * ETOL))
    return (l64, g64, nv64), own


def conditioned_theta(model, X, ta, y, rows, kind, seed, shape=lambda th, j: th):
    """The parameters of a case: the first of seed, seed + 100, ... at which fp32 arithmetic itself -- the twin's fp32 run against its fp64
    run, nothing of the device -- stays within 0.7 of the tenth of every bar.  BatchNorm's backward is a difference of sums, and an entry of
    the gradient near 1e-3 of the largest may come out of terms a thousand times its size: such a draw is an ill-conditioned input (about
    one draw in five here), and the check below would fail it as one."""
    for j in range(12):
        theta = shape(theta_of(model, seed + 100 * j), j)
        if twin_pair(model, theta, X, ta, y, rows, kind)[1] <= 0.7:
            return theta
    pytest.fail("no well-conditioned parameters among twelve draws: the case itself is ill-conditioned")


def engine_of(model, X, ta, y, theta, split=L.EH_SPLIT_TRAIN):
    eng = model.engine(0)
    eng.set_data(split, X, [ta], [y])
    eng.set_params(theta)
    return eng


def variant(wi, ci):
    """position, loss, mechanistic model, shuffled idx of a case: every one of each over the twenty cases"""
    k = wi * len(COUNTS) + ci
    kind = "mse" if COUNTS[ci] == 1 else ("mse", "mae", "nseLoss")[k % 3]      # (one row: nseLoss has no variance to divide by)
    return POSITIONS[(wi + ci) % 5], kind, ("rbq10", "expo")[(k // 2) % 2], k % 2 == 1


def rows_of(y, count, shuffled, seed):
    """the minibatch: a window, or shuffled indices; a batch of one row takes a row with a target"""
    if count == 1:
        return np.array([int(np.flatnonzero(~np.isnan(y))[seed])], np.int32), True
    if shuffled:
        return np.random.default_rng(seed).permutation(ROWS)[:count].astype(np.int32), True
    return np.arange(13, 13 + count, dtype=np.int32), False


def check(model, eng, theta, X, ta, y, rows, as_idx, kind):
    (l64, g64, nv64), own = twin_pair(model, theta, X, ta, y, rows, kind)
    n64 = float(np.linalg.norm(g64))
    assert own <= 1.0, own                                            # the input itself: fp32 arithmetic reaches a tenth of every bar
    eng.set_training_loss(kind)
    loss, grad, nv = eng.loss_and_grad(idx=rows) if as_idx else eng.loss_and_grad(first=int(rows[0]), count=len(rows))
    gn = float(np.linalg.norm(grad.astype(np.float64)))
    print(f"bn chain parity: loss rel {abs(loss - l64) / abs(l64):.2e}  norm rel {abs(gn - n64) / n64:.2e}  max rel {util.relerr(grad, g64):.2e}  "
          f"entry rel {util.elem_relerr(grad, g64, 1e-3):.2e}  n_valid {nv}")
    assert nv == nv64
    assert abs(loss - l64) <= TOL * abs(l64), (loss, l64)
    assert abs(gn - n64) <= TOL * n64
    assert util.relerr(grad, g64) <= TOL, util.relerr(grad, g64)
    assert util.elem_relerr(grad, g64, 1e-3) <= ETOL, util.elem_relerr(grad, g64, 1e-3)


@pytest.mark.parametrize("ci", range(len(COUNTS)), ids=[f"B{c}" for c in COUNTS])
@pytest.mark.parametrize("wi", range(len(WIDTHS)), ids=[f"n{w}" for w in WIDTHS])
def test_loss_and_gradient_against_the_twin(wi, ci):
    n, count = WIDTHS[wi], COUNTS[ci]
    position, kind, mech, shuffled = variant(wi, ci)
    model = make_model(chain_of(position, n), mech)
    X, ta, y = data()
    rows, as_idx = rows_of(y, count, shuffled, 3 + ci)
    theta = conditioned_theta(model, X, ta, y, rows, kind, 10 + wi)
    eng = engine_of(model, X, ta, y, theta)
    bn0 = [eng.get_layer_state(l) for l in model.bn_layers]
    check(model, eng, theta, X, ta, y, rows, as_idx, kind)
    for l, (m0, v0) in zip(model.bn_layers, bn0):                     # eh_loss_and_grad: batch statistics, the running ones left alone
        m1, v1 = eng.get_layer_state(l)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and not m0.any() and np.array_equal(v0, np.ones_like(v0))
    eng.close()


def test_every_variant_is_covered():
    seen = {variant(wi, ci) for wi in range(len(WIDTHS)) for ci in range(len(COUNTS))}
    assert {v[0] for v in seen} == set(POSITIONS) and {v[1] for v in seen} == {"mse", "mae", "nseLoss"}
    assert {v[2] for v in seen} == {"rbq10", "expo"} and {v[3] for v in seen} == {True, False}
    for n in WIDTHS:                                                    # every position at every width somewhere in the file: here or below
        assert len({variant(WIDTHS.index(n), ci)[0] for ci in range(len(COUNTS))}) == 5


@pytest.mark.parametrize("position", POSITIONS)
def test_input_batchnorm_together_with_the_layers(position):
    model = make_model(chain_of(position, 17), "rbq10", "sigmoid", input_batchnorm=True, P=3)
    X, ta, y = data(3)
    rows, as_idx = rows_of(y, 300 if position == "two" else 64, position != "last", 9)
    theta = conditioned_theta(model, X, ta, y, rows, "mse", 5)
    eng = engine_of(model, X, ta, y, theta)
    check(model, eng, theta, X, ta, y, rows, as_idx, "mse")
    eng.close()


@pytest.mark.parametrize("count", [17, 300])
def test_columns_far_from_zero(count):
    """The BatchNorm layer's columns sit some fifty sigma from zero (a first layer with biases of +-100 and weights of order two, identity
    activation): the sums about the batch's first row keep the variance, and the mean kept as first row + mean about it keeps x - mean.
    Predictors on a 2^-10 grid and first-layer weights on a 2^-4 grid make that layer's output exact in fp32, so that the twin's fp32 run
    measures the arithmetic of the BatchNorm layer and not the rounding of its input."""
    model = make_model(eh.Chain(eh.BatchNorm(16), eh.Dense(16, 17, "tanh"), eh.BatchNorm(17)), "rbq10", "identity")
    X, ta, y = data(2)
    X = (np.round(X * 1024) / 1024).astype(np.float32)

    def shape(th, j):
        rng = np.random.default_rng(j)
        th[:32] = np.round(2.0 * rng.standard_normal(32) * 16) / 16
        th[32:48] = 100.0 * np.sign(rng.standard_normal(16))
        return th
    rows = np.arange(40, 40 + count, dtype=np.int32)
    theta = conditioned_theta(model, X, ta, y, rows, "mse", 6, shape)
    layers, _ = model.unpack(theta)
    h = X.T.astype(np.float64) @ layers[0][0].T.astype(np.float64) + layers[0][1]
    assert np.array_equal(h, h.astype(np.float32)) and np.median(np.abs(h.mean(0)) / h.std(0)) > 40      # the case is what it says
    eng = engine_of(model, X, ta, y, theta)
    check(model, eng, theta, X, ta, y, rows, False, "mse")
    eng.close()


BATCHES = [(0, 128), (128, 128), (50, 200)]


def steps_case():
    model = make_model(eh.Chain(eh.Dense(16, 17, "tanh"), eh.BatchNorm(17), eh.Dense(17, 8, "relu"), eh.BatchNorm(8, "sigmoid", momentum=0.3)), input_batchnorm=True)
    X, ta, y = data()
    return model, X, ta, y, theta_of(model, 21)


def check_state(model, eng, state):
    for l in model.bn_layers:
        m, v = eng.get_layer_state(l)
        scale = np.maximum(np.abs(state[l][0]), 1e-3 * np.max(np.abs(state[l][0])))
        assert np.max(np.abs(m - state[l][0]) / scale) <= 1e-5, (l, np.max(np.abs(m - state[l][0]) / scale))
        assert np.max(np.abs(v - state[l][1]) / np.abs(state[l][1])) <= 1e-5, (l, np.max(np.abs(v - state[l][1]) / np.abs(state[l][1])))
    m, v = eng.get_bn_state()
    assert np.allclose(m, state["in"][0], rtol=1e-5, atol=1e-7) and np.allclose(v, state["in"][1], rtol=1e-5)


@pytest.mark.parametrize("rule", ["Descent", "Adam"])
def test_three_steps_running_statistics_and_test_mode(rule):
    model, X, ta, y, theta = steps_case()
    eng = engine_of(model, X, ta, y, theta)
    eng.set_data(L.EH_SPLIT_VAL, X, [ta], [y])
    lr = 0.05 if rule == "Descent" else 1e-2
    eng.opt_init(rule, lr)
    for a, n in BATCHES:
        eng.train_step(a, n)
    ref, state = tw.train_steps(model, theta, X, {"ta": ta}, y, BATCHES, tw.descent(lr) if rule == "Descent" else tw.adam(lr))
    got = eng.get_params()
    d = float(np.max(np.abs(got - ref)))
    print(rule, "max|dtheta|", d)
    # (Adam's first steps are sign-like: tests/test_gpu_seq.py, tests/test_gpu_parity.py)
    assert d <= (1e-5 if rule == "Descent" else 2e-5) * max(1.0, float(np.max(np.abs(ref))))
    check_state(model, eng, state)
    # test mode on those statistics: predictions, parameters and the metrics of eh_eval
    first, count = 7, 301
    rows = np.arange(first, first + count)
    pred, par = tw.predict(model, got, X, {"ta": ta}, rows, {"in": eng.get_bn_state(), **{l: eng.get_layer_state(l) for l in model.bn_layers}})
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * np.max(np.abs(b)))))
    out = eng.forward(L.EH_SPLIT_VAL, first, count)
    assert rel(out["reco"], pred) <= PTOL, rel(out["reco"], pred)
    assert rel(out["parameters"]["rb"], par["rb"]) <= PTOL
    metrics, yh = eng.eval(L.EH_SPLIT_VAL, first, count, predictions=True)
    assert np.array_equal(yh["reco"], out["reco"])
    ok = ~np.isnan(y[rows])
    assert metrics[0]["n"] == ok.sum() and metrics[0]["mse"] == pytest.approx(float(np.mean((pred[ok] - y[rows][ok].astype(np.float64)) ** 2)), rel=2e-5)
    eng.close()


def test_layer_state_round_trip():
    model, X, ta, y, theta = steps_case()
    eng = engine_of(model, X, ta, y, theta)
    assert model.bn_layers == [2, 4]
    rng = np.random.default_rng(1)
    want = {l: (rng.standard_normal(w).astype(np.float32), (0.5 + rng.random(w)).astype(np.float32)) for l, w in ((2, 17), (4, 8))}
    for l, (m, v) in want.items():
        eng.set_layer_state(l, m, v)
    for l, (m, v) in want.items():
        gm, gv = eng.get_layer_state(l)
        assert np.array_equal(gm, m) and np.array_equal(gv, v)
    before = eng.forward(L.EH_SPLIT_TRAIN, 0, 50)["reco"]
    eng.set_layer_state(4, want[4][0] + 1.0, want[4][1])
    assert not np.array_equal(eng.forward(L.EH_SPLIT_TRAIN, 0, 50)["reco"], before)      # forward runs on them
    with pytest.raises(eh.EngineError, match="hidden layer 1 is no BatchNorm layer"):
        eng.get_layer_state(1)
    with pytest.raises(ValueError, match="the layer has 17 units"):
        eng.set_layer_state(2, np.zeros(8, np.float32), np.ones(8, np.float32))
    eng.close()


def cols_of(rows, seed):
    c = eh.synthetic.make_synth_rbq10(rows, seed, 0.05)
    c["sw_pot"] = (c["sw_pot"] / np.float32(50)).astype(np.float32)
    c["dsw_pot"] = (c["dsw_pot"] / np.float32(50)).astype(np.float32)
    return c


def tutorial_model():
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], activation="sigmoid", scale_nn_outputs=True,
                                   hidden_layers=eh.Chain(eh.Dense(16, 16, "sigmoid"), eh.BatchNorm(16), eh.Dense(16, 8, "sigmoid"), eh.BatchNorm(8)), input_batchnorm=True)


def same_state(a, b):
    return all(np.array_equal(a.st["st_layers"][l][k], b.st["st_layers"][l][k]) for l in a.st["st_layers"] for k in ("running_mean", "running_var"))


def test_two_seeded_runs_are_the_same_bits():
    cols = cols_of(600, 3)
    a, b = [eh.train(tutorial_model(), cols, nepochs=4, batchsize=128, opt=eh.Adam(0.01), random_seed=11, loss_types=["mse", "nse"]) for _ in range(2)]
    assert np.array_equal(a.ps, b.ps) and a.best_epoch == b.best_epoch and a.best_loss == b.best_loss
    assert sorted(a.st["st_layers"]) == [2, 4] and same_state(a, b)
    ha = [[h[lt]["reco"] for lt in ("mse", "nse")] for h in a.train_history + a.val_history]
    hb = [[h[lt]["reco"] for lt in ("mse", "nse")] for h in b.train_history + b.val_history]
    assert np.array_equal(np.asarray(ha), np.asarray(hb)) and len(a.train_history) == 5


def val_mse(out):
    vp = out.val_obs_pred
    ok = ~np.isnan(vp["reco"])
    return float(np.mean((vp["reco_pred"][ok].astype(np.float64) - vp["reco"][ok]) ** 2))


def test_train_end_to_end_returns_the_best_model_with_its_state():
    cols = cols_of(2000, 5)
    # a rate that overshoots: the validation loss turns, the patience runs out, and the model that comes back is an earlier epoch's
    out = eh.train(tutorial_model(), cols, nepochs=40, batchsize=128, opt=eh.Adam(0.05), patience=3, random_seed=1, loss_types=["mse", "nse"])
    print("best epoch", out.best_epoch, "of", len(out.val_history) - 1, "best", out.best_loss, "first", out.val_history[0]["mse"]["sum"])
    assert out.best_epoch > 0 and out.best_loss < out.val_history[0]["mse"]["sum"]
    assert np.isfinite(out.val_obs_pred["reco_pred"]).all()
    # the predictions of the returned model (its parameters AND its running statistics, input layer and chain) give the best loss again
    assert val_mse(out) == pytest.approx(out.best_loss, rel=1e-5)
    assert out.val_history[out.best_epoch]["mse"]["sum"] == out.best_loss
    # train_from continues with the state: the first evaluation of the continued run is the returned model's
    if out.best_epoch < len(out.val_history) - 1:
        final = eh.train(tutorial_model(), cols, nepochs=40, batchsize=128, opt=eh.Adam(0.05), patience=3, random_seed=1, loss_types=["mse", "nse"], return_model="final")
        assert not same_state(final, out) and val_mse(final) == pytest.approx(final.val_history[-1]["mse"]["sum"], rel=1e-5)


def test_train_from_carries_the_layer_state():
    cols = cols_of(800, 7)
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], activation="sigmoid", scale_nn_outputs=True,
                                    hidden_layers=eh.Chain(eh.Dense(16, 16, "sigmoid"), eh.BatchNorm(16)))
    a = eh.train(model, cols, nepochs=3, batchsize=128, opt=eh.Adam(0.01), random_seed=2, loss_types=["mse"], return_model="final")
    b = eh.train(model, cols, nepochs=0, batchsize=128, opt=eh.Adam(0.01), random_seed=2, loss_types=["mse"], train_from=a)
    assert same_state(a, b) and np.array_equal(a.ps, b.ps)
    assert b.val_history[0]["mse"]["sum"] == a.val_history[-1]["mse"]["sum"]          # the same model: parameters and running statistics
    c = eh.train(model, cols, nepochs=0, batchsize=128, opt=eh.Adam(0.01), random_seed=2, loss_types=["mse"], train_from=(a.ps, {}))
    assert c.val_history[0]["mse"]["sum"] != a.val_history[-1]["mse"]["sum"]          # without the state: the statistics of a fresh layer
    d = eh.train(model, cols, nepochs=2, batchsize=128, opt=eh.Adam(0.01), random_seed=3, loss_types=["mse"], train_from=a, return_model="final")
    assert not same_state(a, d)


def test_refusals_on_a_live_handle():
    model, X, ta, y, theta = steps_case()
    eng = engine_of(model, X, ta, y, theta)
    for what, call in (("fused_update", lambda: eng.set_option("fused_update", 1)), ("multi_step", lambda: eng.set_option("multi_step", 1)),
                       ("specialize", lambda: eng.set_option("specialize", 1)), ("precision", lambda: eng.set_option("precision", 1)),
                       ("eh_dp_grad", lambda: eng.dp_grad(0, 64)), ("eh_graph_begin", lambda: eng.graph_begin()),
                       ("eh_lbfgs_init", lambda: eng.lbfgs_init())):
        with pytest.raises(NotImplementedError, match=what + ".*BatchNorm layers in the chain"):
            call()
    lib = eng._lib
    assert lib.eh_set_option(eng._h, b"fused_update", 1) == L.EH_EUNSUPPORTED and lib.eh_dp_grad(eng._h, 0, 64) == L.EH_EUNSUPPORTED
    hs = (C.c_void_p * 1)(eng._h)
    assert lib.eh_comm_init_local(hs, 1) == L.EH_EUNSUPPORTED and b"BatchNorm layers in the chain are not built for data parallelism" in lib.eh_last_error(eng._h)
    eng.set_option("fused_update", 2)                            # "where it is reproducible": the pair is
    eng.set_option("multi_step", 0)
    eng.opt_init("Adam", 0.01)
    eng.train_step(0, 64)                                        # ... and the handle trains on
    assert np.isfinite(eng.get_params()).all() and eng.get_layer_state(2)[0].any()
    with pytest.raises(NotImplementedError, match="fused_update"):
        eh.train(tutorial_model(), cols_of(300, 1), nepochs=1, fused_update=True)
    eng.close()
