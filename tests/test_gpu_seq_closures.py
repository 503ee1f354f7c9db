"""Sequence models around recorded closures and multi-output registry models on the device (csrc/eh_seq.hpp, EH_SEQ_HEAD_PROG /
EH_SEQ_HEAD_MULTI) against the torch twin (tests/seq_closure_twin.py, fp64): loss and gradient on the interpreter and on the kernels
compiled at run time, the registry model next to its hand-written closure, optimiser steps, evaluation and predictions, train().

Tolerances are those of tests/test_gpu_seq.py.  tests/test_seq_closures.py holds every parity case, as an input, to a tenth of the bar
in the twin's own fp32 run, and asserts that the cases cover every closure, loss, activation, scaling and index form."""
import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
from oracle import hybrid_oracle as ho

from tests import seq_closure_twin as ct
from tests import seq_twin as tw
from tests import util

pytestmark = pytest.mark.gpu

TOL, ETOL = 1e-5, 5e-4
E2E_REL, E2E_ABS, PTOL = 2e-5, 2e-6, 1e-5
LROWS = ct.LROWS


def _engine(model, X, frc, y, W, ow, lam, starts, theta, jit, split=L.EH_SPLIT_TRAIN):
    eng = model.engine(0)
    eng.set_option("jit", jit)
    eng.set_data(split, X, [frc[f] for f in model.forcing], [y])
    eng.set_sequences(split, W, ow, lam, starts)
    eng.set_params(theta)
    return eng


def _compiled_or_not(eng, jit):
    """after the first launch: jit = 1 ran the kernels compiled at run time (never the interpreter in their place), jit = 0 did not"""
    n, log = eng.jit_status()
    assert n == jit, f"jit = {jit}, eh_jit_status reports {n} compiled kernels: {log[:600]}"


def _check(model, fn_t, out, eng, theta, X, frc, y, sel, W, ow, lam, kind, jit=None, **kw):
    l64, g64, nv64 = ct.loss_and_grad(model, fn_t, out, theta, X, frc, y, sel, W, ow, lam, kind, torch.float64)
    n64 = float(np.linalg.norm(g64))
    loss, grad, nv = eng.loss_and_grad(**kw)
    if jit is not None:
        _compiled_or_not(eng, jit)
    print(f"seq closure parity: loss rel {abs(loss - l64) / abs(l64):.2e}  norm rel {abs(float(np.linalg.norm(grad.astype(np.float64))) - n64) / n64:.2e}  "
          f"max rel {util.relerr(grad, g64):.2e}  entry rel {util.elem_relerr(grad, g64, 1e-3):.2e}  n_valid {nv}")
    assert nv == nv64
    assert abs(loss - l64) <= TOL * abs(l64), (loss, l64)
    assert abs(float(np.linalg.norm(grad.astype(np.float64))) - n64) <= TOL * n64
    assert util.relerr(grad, g64) <= TOL, util.relerr(grad, g64)
    assert util.elem_relerr(grad, g64, 1e-3) <= ETOL, util.elem_relerr(grad, g64, 1e-3)
    return loss, grad


@pytest.mark.parametrize("jit", [0, 1], ids=["interpreted", "compiled"])
@pytest.mark.parametrize("ci", range(len(ct.COUNTS)), ids=[f"n{c}" for c in ct.COUNTS])
@pytest.mark.parametrize("si", range(len(ct.SHAPES)), ids=ct.SHAPE_IDS)
def test_loss_and_gradient_against_the_twin(si, ci, jit):
    model, fn_t, out, X, frc, y, theta, sel, W, ow, lam, kind, kw, starts = ct.case(si, ci)
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta, jit)
    eng.set_training_loss(kind)
    if ct.COUNTS[ci] == 300:
        eng.set_option("max_blocks", 1)          # one workgroup: every wave walks four or five tiles (test_several_tiles_per_wave)
    _check(model, fn_t, out, eng, theta, X, frc, y, sel, W, ow, lam, kind, jit=jit, **kw)
    eng.close()


@pytest.mark.parametrize("jit", [0, 1], ids=["interpreted", "compiled"])
def test_closure_1_against_the_registry_model(jit):
    """the tutorial case: RbQ10 written by hand and RbQ10 of the registry (not bitwise: the two may take different pow paths)"""
    I, H, W, ow, lam = 15, 15, 10, 1, 0
    mc, fn_t, out = ct.closure_model(1, I, H)
    mr = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], eh.RbQ10, dict(ct.RBQ10_TABLE), ["rb"], ["Q10"], hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(I, H))),
                                 activation="tanh", scale_nn_outputs=True)
    X, frc, _ = ct.series()
    y = ct.target_series(1)
    starts = ct.all_starts(LROWS, W, lam)
    theta = mc.initialparameters(21)
    assert mr.n_theta == mc.n_theta
    ec = _engine(mc, X, frc, y, W, ow, lam, starts, theta, jit)
    er = _engine(mr, X, frc, y, W, ow, lam, starts, theta, jit)
    lc, gc = _check(mc, fn_t, out, ec, theta, X, frc, y, starts[:128], W, ow, lam, "mse", jit=jit, first=0, count=128)
    lr, gr, _ = er.loss_and_grad(first=0, count=128)
    assert er.jit_status()[0] == 0
    assert abs(lc - lr) <= TOL * abs(lr) and util.relerr(gc, gr) <= TOL and util.elem_relerr(gc, gr, 1e-3) <= ETOL
    ec.close(); er.close()


@pytest.mark.parametrize("target", ["NEE", "GPP", "RECO"])
def test_fluxpart_from_the_registry(target):
    model, fn_t, out = ct.fluxpart_model(target, 6, 2)
    X, frc, tg = ct.series()
    W, ow, lam = 5, 2, 1
    starts = ct.all_starts(LROWS, W, lam)
    theta = model.initialparameters(31)
    eng = _engine(model, X, frc, tg[target], W, ow, lam, starts, theta, 1)
    _check(model, fn_t, out, eng, theta, X, frc, tg[target], starts[:17], W, ow, lam, "mse", jit=0, first=0, count=17)      # (a registry model: nothing to compile)
    pred, par = ct.predict(model, fn_t, out, theta, X, frc, starts[:17], W, ow)
    got = eng.forward(L.EH_SPLIT_TRAIN, 0, 17)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * np.max(np.abs(b)))))
    assert got[target].shape == (17, ow) and rel(got[target], pred) <= PTOL, rel(got[target], pred)
    eng.close()


@pytest.mark.parametrize("jit", [0, 1], ids=["interpreted", "compiled"])
def test_a_minibatch_without_a_valid_target_changes_nothing(jit):
    model, fn_t, out = ct.closure_model(2, 15, 15)
    X, frc, _ = ct.series()
    W, ow, lam = 5, 2, 1
    y = ct.target_series(2).copy()
    y[:40] = np.nan                                             # every target of windows 0 .. 34 - W
    theta = model.initialparameters(3)
    eng = _engine(model, X, frc, y, W, ow, lam, ct.all_starts(LROWS, W, lam), theta, jit)
    eng.opt_init("Adam", 0.01)
    eng.train_step(100, 64)
    _compiled_or_not(eng, jit)
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


@pytest.mark.parametrize("jit", [0, 1], ids=["interpreted", "compiled"])
def test_three_rmsprop_steps(jit):
    I, H, W, ow, lam = 15, 15, 10, 1, 1
    model, fn_t, out = ct.closure_model(2, I, H)
    X, frc, _ = ct.series()
    y = ct.target_series(2)
    starts = ct.all_starts(LROWS, W, lam)
    theta = model.initialparameters(21)
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta, jit)
    eng.opt_init("RMSProp", 0.001)
    for a, n in BATCHES:
        eng.train_step(a, n)
    _compiled_or_not(eng, jit)
    th, v = theta.copy(), np.zeros_like(theta)
    for a, n in BATCHES:          # the twin's fp64 gradient, the rule in NumPy fp32 (Optimisers.jl op for op)
        _, g, _ = ct.loss_and_grad(model, fn_t, out, th, X, frc, y, starts[a:a + n], W, ow, lam, "mse", torch.float64)
        g = g.astype(np.float32)
        v = np.float32(0.9) * v + np.float32(1 - 0.9) * g * g
        th = th - g * (np.float32(0.001) / (np.sqrt(v) + np.float32(1e-8)))
    d = np.abs(eng.get_params() - th)
    print("rmsprop", float(np.mean(d <= 2e-5)), float(d.max()))
    assert np.mean(d <= 2e-5) >= 0.999 and d.max() <= 2.5e-3, (np.mean(d <= 2e-5), d.max())      # tests/test_gpu_seq.py
    eng.close()


@pytest.mark.parametrize("jit", [0, 1], ids=["interpreted", "compiled"])
def test_evaluation_and_predictions(jit):
    I, H, W, ow, lam = 20, 9, 7, 3, 0
    model, fn_t, out = ct.closure_model(2, I, H)
    X, frc, _ = ct.series()
    y = ct.target_series(2)
    starts = ct.all_starts(LROWS, W, lam)
    theta = model.initialparameters(6)
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta, jit, split=L.EH_SPLIT_VAL)
    first, count = 7, 301
    sel = starts[first:first + count]
    pred, par = ct.predict(model, fn_t, out, theta, X, frc, sel, W, ow)
    yt = tw.targets_of(y, sel, W, ow, lam)
    tname = model.targets[0]
    metrics, yh = eng.eval(L.EH_SPLIT_VAL, first, count, predictions=True)
    _compiled_or_not(eng, jit)
    assert yh[tname].shape == (count, ow)
    ref = ho.metrics_ref(pred.ravel(), yt.ravel(), ~np.isnan(yt.ravel()))
    bad = util.metric_mismatches(metrics[0], ref, E2E_REL, E2E_ABS)
    assert not bad, bad
    res = eng.forward(L.EH_SPLIT_VAL, first, count)
    assert res[tname].shape == (count, ow) and np.array_equal(res[tname], yh[tname])
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * np.max(np.abs(b)))))
    assert rel(res[tname], pred) <= PTOL, rel(res[tname], pred)
    for name in model.mechanistic_model.params:
        assert res["parameters"][name].shape == (count, ow)
        assert rel(res["parameters"][name], par[name]) <= PTOL, (name, rel(res["parameters"][name], par[name]))
    eng.close()


def test_a_compiled_kernel_that_disagrees_with_the_interpreter_is_not_used(monkeypatch):
    """the first training pass runs both forms; a compiled kernel that computes something else (here: the check is told it did) leaves the
    handle on the interpreter, eh_jit_status says why, and the result is the interpreter's"""
    model, fn_t, out, X, frc, y, theta, sel, W, ow, lam, kind, kw, starts = ct.case(3, 1)
    monkeypatch.setenv("EH_DEBUG_JIT_SKEW", "1")
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta, 1)
    eng.set_training_loss(kind)
    _check(model, fn_t, out, eng, theta, X, frc, y, sel, W, ow, lam, kind, **kw)
    n, log = eng.jit_status()
    assert n == 0 and "disagrees with the interpreter" in log, (n, log[:300])
    eng.close()


def test_extra_loss_and_recorded_losses_stay_refused():
    model, _, _ = ct.closure_model(1, 15, 15)
    X, frc, _ = ct.series()
    eng = _engine(model, X, frc, ct.target_series(1), 10, 1, 1, ct.all_starts(LROWS, 10, 1), model.initialparameters(1), 0)
    with pytest.raises(NotImplementedError):
        eng.set_training_loss(lambda yhat, y: np.mean(np.abs(yhat - y) ** 3))
    eng.close()
    cols = eh.synthetic.make_synth_rbq10(300, 1, 0.05)
    with pytest.raises(NotImplementedError, match="extra_loss"):
        eh.train(_tutorial_closure_model(), cols, nepochs=1, batchsize=64, opt=eh.RMSProp(0.01), extra_loss=lambda yhat: np.mean(yhat["reco"]),
                 sequence_kwargs=dict(input_window=10, output_window=1, output_shift=1, lead_time=1))


def _cols(rows, seed):
    c = eh.synthetic.make_synth_rbq10(rows, seed, 0.05)
    c["sw_pot"] = (c["sw_pot"] / np.float32(50)).astype(np.float32)
    c["dsw_pot"] = (c["dsw_pot"] / np.float32(50)).astype(np.float32)
    return c


def _tutorial_closure_model():
    """the reference's LSTM tutorial with its mechanistic model as the user's own closure"""
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], ct.rbq10_np, dict(ct.RBQ10_TABLE), ["rb"], ["Q10"],
                                   hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(15, 15))), activation="tanh", scale_nn_outputs=True)


def test_train_end_to_end_and_two_seeded_runs_are_the_same_bits():
    cols = _cols(600, 3)
    kw = dict(input_window=10, output_window=1, output_shift=1, lead_time=1)
    runs = [eh.train(_tutorial_closure_model(), cols, nepochs=2, batchsize=128, opt=eh.RMSProp(0.01), training_loss="nseLoss", random_seed=11,
                     sequence_kwargs=kw) for _ in range(2)]
    a, b = runs
    (_, _, wtr), (_, _, wva) = eh.split_data(cols, _tutorial_closure_model(), sequence_kwargs=kw)
    assert a.train_obs_pred["reco_pred"].shape == (len(wtr.starts),) and a.val_obs_pred["reco_pred"].shape == (len(wva.starts),)
    assert np.isfinite(a.train_obs_pred["reco_pred"]).all() and np.isfinite(a.val_obs_pred["reco_pred"]).all()
    assert a.train_diffs["rb"].shape == (len(wtr.starts),) and np.isfinite(a.train_diffs["rb"]).all()
    assert np.array_equal(a.ps, b.ps) and np.array_equal(a.val_obs_pred["reco_pred"], b.val_obs_pred["reco_pred"])
    assert np.array_equal(a.train_obs_pred["reco_pred"], b.train_obs_pred["reco_pred"])
