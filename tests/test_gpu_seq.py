"""Sequence models on the device (csrc/eh_seq.hpp) against the torch twin (tests/seq_twin.py, fp64): loss and gradient of the windowed
step with BPTT, optimiser steps, evaluation and predictions, reproducibility, the train() front door, refusals on a live handle.

Tolerances are the project's own (tests/test_gpu_lform.py): loss and gradient norm within 1e-5 relative of the fp64 twin, entry by
entry within 5e-4 down to 1e-3 of the largest entry.  Every parity check first holds the twin's own fp32 run to a tenth of the bar: an
ill-conditioned input fails as an input.  (fp32 against fp64 twin, W = 1 .. 32, I = H up to 32: loss 2.4e-7, norm 1.9e-7, entries 8.9e-7.)"""
import sys

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
import easyhybrid_jl_amd.train  # noqa: F401
from oracle import hybrid_oracle as ho

from tests import seq_twin as tw
from tests import util

T = sys.modules["easyhybrid_jl_amd.train"]      # (the package exports the function `train` under the module's name)
pytestmark = pytest.mark.gpu

TOL, ETOL = 1e-5, 5e-4
E2E_REL, E2E_ABS, PTOL = 2e-5, 2e-6, 1e-5          # tests/test_gpu_eval.py
LROWS = 400
RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}
EXPO = {"k": (0.01, 0.0, 0.2), "Resp0": (2.0, 0.0, 8.0)}


def _model(I, H, mech="rbq10", act="tanh", scale=True, P=2):
    hl = eh.Chain(eh.Recurrence(eh.LSTMCell(I, H)))
    preds = [f"x{i}" for i in range(P)]
    if mech == "rbq10":       # one neural + one global parameter
        return eh.constructHybridModel(preds, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=hl, activation=act, scale_nn_outputs=scale)
    return eh.constructHybridModel(preds, ["T"], ["Resp_obs"], eh.Expo_resp_model, dict(EXPO), ["Resp0", "k"], [], hidden_layers=hl, activation=act, scale_nn_outputs=scale)


_SERIES = {}


def _series(P=2, rows=LROWS, nan_frac=0.1):
    """(X (P, rows), forcing (rows,), target (rows,)): computed once per shape and left unchanged"""
    key = (P, rows, nan_frac)
    if key not in _SERIES:
        rng = np.random.default_rng(1234 + P)
        X = (0.6 * rng.standard_normal((P, rows))).astype(np.float32)
        X[0] = np.cumsum(X[0]) * 0.2                                     # something a memory can use
        ta = (10 + 8 * rng.standard_normal(rows)).astype(np.float32)
        y = (3.0 + np.tanh(X[0])) * 2.0 ** (0.1 * (ta - 15.0)) + 0.1 * rng.standard_normal(rows)
        y = y.astype(np.float32)
        y[rng.random(rows) < nan_frac] = np.nan
        for a in (X, ta, y):
            a.setflags(write=False)
        _SERIES[key] = (X, ta, y)
    return _SERIES[key]


def _engine(model, X, ta, y, W, ow, lam, starts, theta, split=L.EH_SPLIT_TRAIN):
    eng = model.engine(0)
    eng.set_data(split, X, [ta], [y])
    eng.set_sequences(split, W, ow, lam, starts)
    eng.set_params(theta)
    return eng


def _all_starts(rows, W, lam, s=1):
    return np.arange(0, rows - W - lam + 1, s, dtype=np.int32)


def _check(model, eng, theta, X, ta, y, sel, W, ow, lam, kind, **kw):
    fname = model.forcing[0]
    l64, g64, nv64 = tw.loss_and_grad(model, theta, X, {fname: ta}, y, sel, W, ow, lam, kind, torch.float64)
    l32, g32, _ = tw.loss_and_grad(model, theta, X, {fname: ta}, y, sel, W, ow, lam, kind, torch.float32)
    n64 = float(np.linalg.norm(g64))
    # the input itself: fp32 arithmetic reaches a tenth of the bar
    assert abs(l32 - l64) <= 0.1 * TOL * abs(l64) and abs(float(np.linalg.norm(g32)) - n64) <= 0.1 * TOL * n64, (l32, l64)
    assert util.elem_relerr(g32, g64, 1e-3) <= 0.1 * ETOL, util.elem_relerr(g32, g64, 1e-3)
    loss, grad, nv = eng.loss_and_grad(**kw)
    print(f"seq parity: loss rel {abs(loss - l64) / abs(l64):.2e}  norm rel {abs(float(np.linalg.norm(grad.astype(np.float64))) - n64) / n64:.2e}  "
          f"max rel {util.relerr(grad, g64):.2e}  entry rel {util.elem_relerr(grad, g64, 1e-3):.2e}  n_valid {nv}")
    assert nv == nv64
    assert abs(loss - l64) <= TOL * abs(l64), (loss, l64)
    assert abs(float(np.linalg.norm(grad.astype(np.float64))) - n64) <= TOL * n64
    assert util.relerr(grad, g64) <= TOL, util.relerr(grad, g64)
    assert util.elem_relerr(grad, g64, 1e-3) <= ETOL, util.elem_relerr(grad, g64, 1e-3)


SHAPES = [(15, 15, 10, 1, 0), (6, 2, 5, 2, 1), (16, 16, 1, 1, 0), (15, 15, 4, 4, 0), (32, 32, 32, 4, 1), (20, 9, 7, 3, 0), (5, 32, 12, 3, 1)]
COUNTS = [5, 17, 33, 300]


def _variant(si, ci):
    """activation, sigma-scaling, loss and mechanistic model of a case: every pairing of the issue's list occurs over the first 24 cases"""
    k = si * len(COUNTS) + ci
    mech = "expo" if k % 3 == 1 else "rbq10"
    scale = True if mech == "expo" else (k % 2 == 0)          # (Expo with raw NN outputs: exp(o T) overflows -- an input, not a kernel, question)
    return ("tanh", "sigmoid")[(k // 2) % 2], scale, ("mse", "nseLoss")[(k // 3) % 2], mech


@pytest.mark.parametrize("ci", range(len(COUNTS)), ids=[f"n{c}" for c in COUNTS])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=["tutorial", "I6H2", "W1", "ow4", "I32H32W32", "I20H9", "I5H32"])
def test_loss_and_gradient_against_the_twin(si, ci):
    (I, H, W, ow, lam), count = SHAPES[si], COUNTS[ci]
    act, scale, kind, mech = _variant(si, ci)
    model = _model(I, H, mech, act, scale)
    X, ta, y = _series()
    starts = _all_starts(LROWS, W, lam)
    theta = model.initialparameters(10 + si)
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    eng.set_training_loss(kind)
    _check(model, eng, theta, X, ta, y, starts[:count], W, ow, lam, kind, first=0, count=count)
    eng.close()


def test_every_pairing_is_covered():
    seen = {_variant(si, ci) for si in range(len(SHAPES)) for ci in range(len(COUNTS))}
    assert {v[0] for v in seen} == {"tanh", "sigmoid"} and {v[1] for v in seen} == {True, False}
    assert {v[2] for v in seen} == {"mse", "nseLoss"} and {v[3] for v in seen} == {"rbq10", "expo"}


def test_shuffled_idx_and_output_shift_3():
    model = _model(15, 15, "rbq10", "tanh", True)
    X, ta, y = _series()
    W, ow, lam = 10, 2, 1
    theta = model.initialparameters(4)
    starts = _all_starts(LROWS, W, lam)
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    idx = np.random.default_rng(5).permutation(len(starts))[:77].astype(np.int32)
    _check(model, eng, theta, X, ta, y, starts[idx], W, ow, lam, "mse", idx=idx)
    eng.close()
    s3 = eh.split_into_sequences(X, y[None], input_window=W, output_window=ow, output_shift=3, lead_time=lam).starts
    assert s3[:3].tolist() == [0, 3, 6]
    eng = _engine(model, X, ta, y, W, ow, lam, s3, theta)
    _check(model, eng, theta, X, ta, y, s3[20:90], W, ow, lam, "mse", first=20, count=70)
    eng.close()


def test_second_predictor_block():
    """P = 18: the Dense-in contraction takes a second block of 16 predictors"""
    model = _model(6, 5, "rbq10", "sigmoid", True, P=18)
    X, ta, y = _series(18)
    W, ow, lam = 3, 2, 0
    theta = model.initialparameters(8)
    starts = _all_starts(LROWS, W, lam)
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    _check(model, eng, theta, X, ta, y, starts[:50], W, ow, lam, "mse", first=0, count=50)
    eng.close()


def test_several_tiles_per_wave():
    """one workgroup for 300 windows: every wave walks four or five tiles with its accumulators (and its workspace slot) kept across them"""
    I, H, W, ow, lam = 20, 9, 7, 3, 0
    model = _model(I, H, "rbq10", "tanh", True)
    X, ta, y = _series()
    starts = _all_starts(LROWS, W, lam)
    theta = model.initialparameters(12)
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    wide = eng.forward(L.EH_SPLIT_TRAIN, 0, 300)
    m_wide, _ = eng.eval(L.EH_SPLIT_TRAIN, 0, 300)
    eng.set_option("max_blocks", 1)
    _check(model, eng, theta, X, ta, y, starts[:300], W, ow, lam, "mse", first=0, count=300)
    one = eng.forward(L.EH_SPLIT_TRAIN, 0, 300)
    assert np.array_equal(one["reco"], wide["reco"]) and np.array_equal(one["parameters"]["rb"], wide["parameters"]["rb"])      # a window's values do not depend on the grid
    m_one, _ = eng.eval(L.EH_SPLIT_TRAIN, 0, 300)
    assert m_one[0]["n"] == m_wide[0]["n"] and m_one[0]["mse"] == pytest.approx(m_wide[0]["mse"], rel=1e-6)
    eng.close()


def test_weight_l2_walks_the_dense_weights_only():
    model = _model(15, 15)
    X, ta, y = _series()
    W, ow, lam = 6, 1, 1
    theta = model.initialparameters(2)
    starts = _all_starts(LROWS, W, lam)
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    l0, g0, _ = eng.loss_and_grad(first=0, count=100)
    eng.set_weight_l2(0.01, False)
    l1, g1, _ = eng.loss_and_grad(first=0, count=100)
    m = model.l2_mask(None, "weight")
    w = theta[m].astype(np.float64)
    assert l1 - l0 == pytest.approx(0.01 * float(w @ w), rel=1e-4)
    assert np.allclose(g1[m] - g0[m], 0.02 * theta[m], rtol=1e-3, atol=1e-7) and np.array_equal(g1[~m], g0[~m])
    eng.close()


def test_a_minibatch_without_a_valid_target_changes_nothing():
    model = _model(15, 15)
    X, ta, y = _series()
    W, ow, lam = 5, 2, 1
    y = y.copy()
    y[:40] = np.nan                                             # every target of windows 0 .. 34 - W
    theta = model.initialparameters(3)
    eng = _engine(model, X, ta, y, W, ow, lam, _all_starts(LROWS, W, lam), theta)
    eng.opt_init("Adam", 0.01)
    eng.train_step(100, 64)
    th1 = eng.get_params()
    m1, v1, bt1 = eng.get_opt_state()
    assert not np.array_equal(th1, theta)
    loss = eng.train_step(0, 30)
    assert np.isnan(loss)
    m2, v2, bt2 = eng.get_opt_state()
    assert np.array_equal(eng.get_params(), th1) and np.array_equal(m1, m2) and np.array_equal(v1, v2) and np.array_equal(np.asarray(bt1), np.asarray(bt2))
    l, g, nv = eng.loss_and_grad(first=0, count=30)
    assert nv == 0 and np.isnan(l)
    eng.close()


BATCHES = [(0, 128), (128, 128), (50, 200)]


def _tutorial_case():
    model = _model(15, 15, "rbq10", "tanh", True)
    X, ta, y = _series()
    W, ow, lam = 10, 1, 1
    return model, X, ta, y, W, ow, lam, _all_starts(LROWS, W, lam), model.initialparameters(21)


def _twin_steps(model, theta, X, ta, y, starts, W, ow, lam, rule):
    """the three steps with the twin's fp64 gradient and the optimiser rule in NumPy fp32 (Optimisers.jl op for op)"""
    th = theta.copy()
    state = {}
    for a, n in BATCHES:
        _, g, _ = tw.loss_and_grad(model, th, X, {"ta": ta}, y, starts[a:a + n], W, ow, lam, "mse", torch.float64)
        th = rule(th, g.astype(np.float32), state)
    return th


def _descent(lr):
    return lambda th, g, st: th - np.float32(lr) * g


def _rmsprop(lr, rho=0.9, eps=1e-8):
    def rule(th, g, st):
        st["v"] = np.float32(rho) * st.get("v", np.zeros_like(th)) + np.float32(1 - rho) * g * g
        return th - g * (np.float32(lr) / (np.sqrt(st["v"]) + np.float32(eps)))
    return rule


def _adam(lr, b1=0.9, b2=0.999, eps=1e-8):
    def rule(th, g, st):
        b1f, b2f = np.float32(b1), np.float32(b2)
        st["m"] = b1f * st.get("m", np.zeros_like(th)) + (np.float32(1) - b1f) * g
        st["v"] = b2f * st.get("v", np.zeros_like(th)) + (np.float32(1) - b2f) * g * g
        st["p1"], st["p2"] = st.get("p1", np.float32(1)) * b1f, st.get("p2", np.float32(1)) * b2f
        return th - st["m"] / (np.float32(1) - st["p1"]) / (np.sqrt(st["v"] / (np.float32(1) - st["p2"])) + np.float32(eps)) * np.float32(lr)
    return rule


def test_three_descent_steps():
    model, X, ta, y, W, ow, lam, starts, theta = _tutorial_case()
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    eng.opt_init("Descent", 0.05)
    for a, n in BATCHES:
        eng.train_step(a, n)
    ref = _twin_steps(model, theta, X, ta, y, starts, W, ow, lam, _descent(0.05))
    d = float(np.max(np.abs(eng.get_params() - ref)))
    print("descent max|dtheta|", d)
    assert d <= 1e-5 * max(1.0, float(np.max(np.abs(ref))))
    eng.close()


def test_three_rmsprop_steps():
    model, X, ta, y, W, ow, lam, starts, theta = _tutorial_case()
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    eng.opt_init("RMSProp", 0.001)
    for a, n in BATCHES:
        eng.train_step(a, n)
    ref = _twin_steps(model, theta, X, ta, y, starts, W, ow, lam, _rmsprop(0.001))
    d = np.abs(eng.get_params() - ref)
    print("rmsprop", float(np.mean(d <= 2e-5)), float(d.max()))
    assert np.mean(d <= 2e-5) >= 0.999 and d.max() <= 2.5e-3, (np.mean(d <= 2e-5), d.max())      # tests/test_gpu_lform.py
    eng.close()


def test_three_steps_with_a_rule_per_branch():
    model, X, ta, y, W, ow, lam, starts, theta = _tutorial_case()
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    T._opt_setup(eng, {"ps": eh.Adam(1e-2), "Q10": eh.Descent(5e-2)}, model)
    for a, n in BATCHES:
        eng.train_step(a, n)
    br = model.opt_branches()
    adam, desc = _adam(1e-2), _descent(5e-2)

    def rule(th, g, st):
        out = adam(th, g, st)
        lo, hi = br["Q10"]
        out[lo:hi] = desc(th, g, st)[lo:hi]
        return out
    ref = _twin_steps(model, theta, X, ta, y, starts, W, ow, lam, rule)
    got = eng.get_params()
    lo, hi = br["ps"]
    scale = max(1.0, float(np.max(np.abs(ref))))
    print("branches", float(np.max(np.abs(got[lo:hi] - ref[lo:hi]))), float(np.max(np.abs(got[hi:] - ref[hi:]))))
    assert np.max(np.abs(got[lo:hi] - ref[lo:hi])) <= 2e-5 * scale           # Adam's first steps are sign-like: tests/test_gpu_parity.py
    assert np.max(np.abs(got[hi:] - ref[hi:])) <= 1e-5 * scale
    eng.close()


@pytest.mark.parametrize("I,H,W,ow,lam,mech", [(15, 15, 10, 1, 1, "rbq10"), (20, 9, 7, 3, 0, "expo")])
def test_evaluation_and_predictions(I, H, W, ow, lam, mech):
    model = _model(I, H, mech, "tanh", True)
    X, ta, y = _series()
    starts = _all_starts(LROWS, W, lam)
    theta = model.initialparameters(6)
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta, split=L.EH_SPLIT_VAL)
    first, count = 7, 301
    sel = starts[first:first + count]
    pred, par = tw.predict(model, theta, X, {model.forcing[0]: ta}, sel, W, ow)
    yt = tw.targets_of(y, sel, W, ow, lam)
    tname = model.targets[0]
    metrics, yh = eng.eval(L.EH_SPLIT_VAL, first, count, predictions=True)
    assert yh[tname].shape == (count, ow)
    ref = ho.metrics_ref(pred.ravel(), yt.ravel(), ~np.isnan(yt.ravel()))
    bad = util.metric_mismatches(metrics[0], ref, E2E_REL, E2E_ABS)
    assert not bad, bad
    out = eng.forward(L.EH_SPLIT_VAL, first, count)
    assert out[tname].shape == (count, ow) and np.array_equal(out[tname], yh[tname])
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * np.max(np.abs(b)))))
    assert rel(out[tname], pred) <= PTOL, rel(out[tname], pred)
    for name in model.mechanistic_model.params:
        assert out["parameters"][name].shape == (count, ow)
        assert rel(out["parameters"][name], par[name]) <= PTOL, (name, rel(out["parameters"][name], par[name]))
    eng.close()


def _cols(rows, seed):
    c = eh.synthetic.make_synth_rbq10(rows, seed, 0.05)
    c["sw_pot"] = (c["sw_pot"] / np.float32(50)).astype(np.float32)
    c["dsw_pot"] = (c["dsw_pot"] / np.float32(50)).astype(np.float32)
    return c


def _tutorial_model():
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"],
                                   hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(15, 15))), activation="tanh", scale_nn_outputs=True)


def test_two_seeded_runs_are_the_same_bits():
    cols = _cols(600, 3)
    runs = [eh.train(_tutorial_model(), cols, nepochs=5, batchsize=128, opt=eh.RMSProp(0.01), random_seed=11, loss_types=["mse", "nse"],
                     sequence_kwargs=dict(input_window=10, output_window=1, output_shift=1, lead_time=1)) for _ in range(2)]
    a, b = runs
    assert np.array_equal(a.ps, b.ps) and a.best_epoch == b.best_epoch
    ha = [[h[lt]["reco"] for lt in ("mse", "nse")] for h in a.train_history + a.val_history]
    hb = [[h[lt]["reco"] for lt in ("mse", "nse")] for h in b.train_history + b.val_history]
    assert np.array_equal(np.asarray(ha), np.asarray(hb)) and len(a.train_history) == 6


def test_tutorial_end_to_end():
    cols = _cols(2000, 5)
    kw = dict(input_window=10, output_window=1, output_shift=1, lead_time=1)
    out = eh.train(_tutorial_model(), cols, nepochs=20, batchsize=128, opt=eh.RMSProp(0.01), training_loss="nseLoss", loss_types=["mse", "nse"],
                   random_seed=1, sequence_kwargs=kw)
    assert out.best_loss < out.val_history[0]["mse"]["sum"] and out.best_epoch > 0
    (_, _, wtr), (_, _, wva) = eh.split_data(cols, _tutorial_model(), sequence_kwargs=kw)
    vp = out.val_obs_pred
    assert vp["reco_pred"].shape == (len(wva.starts) * 1,) and vp["reco"].shape == vp["reco_pred"].shape
    assert np.array_equal(vp["reco"], cols["reco"][wva.target_rows().ravel()], equal_nan=True)
    assert out.train_obs_pred["reco_pred"].shape == (len(wtr.starts),) and out.train_diffs["rb"].shape == (len(wtr.starts),)
    assert np.isfinite(vp["reco_pred"]).all()


def test_refusals_on_a_live_handle():
    model, X, ta, y, W, ow, lam, starts, theta = _tutorial_case()
    eng = _engine(model, X, ta, y, W, ow, lam, starts, theta)
    for what, call in (("fused_update", lambda: eng.set_option("fused_update", 1)), ("multi_step", lambda: eng.set_option("multi_step", 1)),
                       ("specialize", lambda: eng.set_option("specialize", 1)), ("precision", lambda: eng.set_option("precision", 1)),
                       ("eh_dp_grad", lambda: eng.dp_grad(0, 64)), ("training_loss", lambda: eng.set_training_loss("pearsonLoss")),
                       ("eh_graph_begin", lambda: eng.graph_begin())):
        with pytest.raises(NotImplementedError, match=what):
            call()
    assert eng._lib.eh_set_option(eng._h, b"fused_update", 1) == L.EH_EUNSUPPORTED
    assert eng._lib.eh_dp_grad(eng._h, 0, 64) == L.EH_EUNSUPPORTED
    eng.set_option("fused_update", 2)                            # "where it is reproducible": the pair is
    # a second target: refused by the constructor, with the reason
    d = model.to_desc()
    d.n_targets = 2
    d.target_output[1] = 0
    h = __import__("ctypes").c_void_p()
    assert eng._lib.eh_create(__import__("ctypes").byref(d), __import__("ctypes").byref(h)) == L.EH_EUNSUPPORTED
    assert b"2 targets" in eng._lib.eh_last_error(None)
    # windows are checked against the series; a feed-forward handle has no windows
    with pytest.raises(ValueError, match="starts"):
        eng.set_sequences(L.EH_SPLIT_TRAIN, W, ow, lam, np.array([0, LROWS - W], np.int32))
    with pytest.raises(ValueError, match="input_window"):
        eng.set_sequences(L.EH_SPLIT_TRAIN, L.EH_MAX_SEQ_WINDOW + 1, 1, 0, np.array([0], np.int32))
    eng.close()
    ff = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=[8]).engine(0)
    ff.set_data(L.EH_SPLIT_TRAIN, X, [ta], [y])
    with pytest.raises(NotImplementedError, match="no LSTM layer"):
        ff.set_sequences(L.EH_SPLIT_TRAIN, 5, 1, 1, np.array([0], np.int32))
    ff.close()
