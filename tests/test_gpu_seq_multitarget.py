"""Sequence models with several targets on the device (csrc/eh_seq.hpp, the MT kernels; eh_seq_count_kernel) against the fp64 torch twin
of tests/seq_multitarget_twin.py: loss, gradient, every metric per target and the predictions over the cases of
tests/seq_multitarget_cases.py (tests/test_seq_multitarget.py holds them, as inputs, to being well posed); an empty target; the
one-target kernel next to a two-target model whose second target is empty; reproducibility, an optimiser trajectory, train(), refusals.

The bars are those of tests/test_gpu_seq_closures.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
from oracle import hybrid_oracle as ho

from tests import seq_cells_twin as cw
from tests import seq_closure_twin as ct
from tests import seq_multitarget_cases as mc
from tests import seq_multitarget_twin as mt
from tests import util

pytestmark = pytest.mark.gpu

TOL, ETOL = 1e-5, 5e-4
E2E_REL, E2E_ABS, PTOL = 2e-5, 2e-6, 1e-5
LROWS = ct.LROWS


def _engine(model, X, frc, ys, W, ow, lam, starts, theta, jit=0, kinds=None, agg="sum", split=L.EH_SPLIT_TRAIN):
    eng = model.engine(0)
    eng.set_option("jit", jit)
    eng.set_data(split, X, [frc[f] for f in model.forcing], list(ys))
    eng.set_sequences(split, W, ow, lam, starts)
    eng.set_params(theta)
    if kinds is not None:
        eng.set_training_loss(eh.PerTarget(tuple(kinds)))
    eng.set_agg(agg)
    return eng


def _rel(a, b):
    """entry-wise relative error at the 1e-3 floor (tests/test_gpu_seq_closures.py)"""
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * np.max(np.abs(b)))))


def _check_grad(tag, loss, grad, nv, l64, g64, nv64):
    n64 = float(np.linalg.norm(g64))
    print(f"{tag}: loss rel {abs(loss - l64) / abs(l64):.2e}  norm rel {abs(float(np.linalg.norm(grad.astype(np.float64))) - n64) / n64:.2e}  "
          f"max rel {util.relerr(grad, g64):.2e}  entry rel {util.elem_relerr(grad, g64, 1e-3):.2e}  n_valid {nv}")
    assert nv == int(np.sum(nv64))
    assert abs(loss - l64) <= TOL * abs(l64), (loss, l64)
    assert abs(float(np.linalg.norm(grad.astype(np.float64))) - n64) <= TOL * n64
    assert util.relerr(grad, g64) <= TOL, util.relerr(grad, g64)
    assert util.elem_relerr(grad, g64, 1e-3) <= ETOL, util.elem_relerr(grad, g64, 1e-3)


@pytest.mark.parametrize("case", mc.CASES, ids=mc.IDS)
def test_loss_gradient_metrics_and_predictions_against_the_twin(case):
    model, fn_t, outs, X, frc, ys, theta, sel, kw, starts, jit = mc.build(case)
    W, ow, lam, kinds, agg, T = mc.W, case["ow"], case["lam"], case["kinds"], case["agg"], case["T"]
    eng = _engine(model, X, frc, ys, W, ow, lam, starts, theta, jit, kinds, agg)
    l64, g64, nv64 = mt.loss_and_grad(model, fn_t, outs, theta, X, frc, ys, sel, W, ow, lam, kinds, agg)
    loss, grad, nv = eng.loss_and_grad(**kw)
    if case["head"] != "fluxpart":
        n, log = eng.jit_status()
        assert n == jit, f"jit = {jit}, eh_jit_status reports {n} compiled kernels: {log[:600]}"      # compiled: the kernel built at run time took over
    _check_grad(case["id"], loss, grad, nv, l64, g64, nv64)
    # evaluation and predictions over a window of the split (they take first / count): the case's count from its first window on
    first, count = mc.EVAL_FIRST, case["count"]
    esel = starts[first:first + count]
    pred, par = mt.predict(model, fn_t, outs, theta, X, frc, esel, W, ow)
    yt = mt.targets_of(ys, esel, W, ow, lam)
    metrics, yh = eng.eval(L.EH_SPLIT_TRAIN, first, count, predictions=True)
    got = eng.forward(L.EH_SPLIT_TRAIN, first, count)
    assert len(metrics) == T
    for t, name in enumerate(model.targets):
        ref = ho.metrics_ref(pred[t].ravel(), yt[t].ravel(), ~np.isnan(yt[t].ravel()))
        bad = util.metric_mismatches(metrics[t], ref, E2E_REL, E2E_ABS)
        assert not bad, (name, bad)
        assert got[name].shape == (count, ow) and np.array_equal(got[name], yh[name])
        print(f"  {name}: prediction rel {_rel(got[name], pred[t]):.2e}")
        assert _rel(got[name], pred[t]) <= PTOL, (name, _rel(got[name], pred[t]))
    for name in model.mechanistic_model.params:
        assert got["parameters"][name].shape == (count, ow) and _rel(got["parameters"][name], par[name]) <= PTOL, name
    eng.close()


def _three_target_case(head="fluxpart", kind="lstm", I=7, H=20, jit=0):
    names = ["RECO", "NEE", "GPP"] if head == "fluxpart" else ["reco", "nee", "gpp"]
    model, fn_t, outs = (mt.fluxpart_model if head == "fluxpart" else mt.flux3_model)(kind, names, I, H)
    X, frc, _ = ct.series()
    ys = mt.masked_targets(names, 42, 0.2, head)
    W, ow, lam = 6, 3, 1
    return model, fn_t, outs, X, frc, ys, W, ow, lam, ct.all_starts(LROWS, W, lam), model.initialparameters(9)


@pytest.mark.parametrize("head,jit", [("fluxpart", 0), ("flux3", 0), ("flux3", 1)], ids=["fluxpart", "flux3-interpreted", "flux3-compiled"])
def test_an_empty_target_adds_nothing(head, jit):
    """one target all-NaN in the batch: its count is 0, its loss term 0, the gradient the twin's of the other two; every target empty: no update"""
    model, fn_t, outs, X, frc, ys, W, ow, lam, starts, theta = _three_target_case(head, jit=jit)
    ys = [y.copy() for y in ys]
    ys[1][:] = np.nan
    for y in ys:
        y[:40] = np.nan                                         # every target of windows 0 .. 30
    kinds = ("mse", "nseLoss", "mae")
    eng = _engine(model, X, frc, ys, W, ow, lam, starts, theta, jit, kinds)
    sel = starts[100:170]
    l64, g64, nv64 = mt.loss_and_grad(model, fn_t, outs, theta, X, frc, ys, sel, W, ow, lam, kinds)
    l2, g2, nv2 = mt.loss_and_grad(model, fn_t, [outs[0], outs[2]], theta, X, frc, [ys[0], ys[2]], sel, W, ow, lam, ("mse", "mae"))
    assert nv64[1] == 0 and l64 == l2 and np.array_equal(g64, g2)
    loss, grad, nv = eng.loss_and_grad(first=100, count=70)
    _check_grad("empty target", loss, grad, nv, l2, g2, nv2)
    metrics, _ = eng.eval(L.EH_SPLIT_TRAIN, 100, 70)
    assert metrics[1]["n"] == 0 and np.isnan(metrics[1]["mse"]) and metrics[0]["n"] == nv2[0] and metrics[2]["n"] == nv2[1]
    eng.opt_init("Adam", 0.01)
    eng.train_step(100, 70)
    th1 = eng.get_params()
    m1, v1, bt1 = eng.get_opt_state()
    assert not np.array_equal(th1, theta)
    assert np.isnan(eng.train_step(0, 30))                      # no target has a valid entry: skipped
    m2, v2, bt2 = eng.get_opt_state()
    assert np.array_equal(eng.get_params(), th1) and np.array_equal(m1, m2) and np.array_equal(v1, v2) and np.array_equal(np.asarray(bt1), np.asarray(bt2))
    l, g, n0 = eng.loss_and_grad(first=0, count=30)
    assert n0 == 0 and np.isnan(l)
    eng.close()


@pytest.mark.parametrize("kind", ["mse", "mae", "nseLoss"])
def test_two_targets_with_an_empty_second_are_the_one_target_step(kind):
    """the one-target step is normalised after the pass, the two-target step weighted before it: equal to TOL, not to the bit"""
    X, frc, tg = ct.series()
    W, ow, lam = 6, 3, 1
    starts = ct.all_starts(LROWS, W, lam)
    m2, _, _ = mt.fluxpart_model("lstm", ["RECO", "GPP"], 15, 15)
    m1, _, _ = ct.fluxpart_model("RECO", 15, 15)
    theta = m1.initialparameters(4)
    assert m1.n_theta == m2.n_theta
    e2 = _engine(m2, X, frc, [tg["RECO"], np.full(LROWS, np.nan, np.float32)], W, ow, lam, starts, theta, 0, (kind, "mse"))
    e1 = _engine(m1, X, frc, [tg["RECO"]], W, ow, lam, starts, theta)
    e1.set_training_loss(kind)
    l2, g2, n2 = e2.loss_and_grad(first=5, count=70)
    l1, g1, n1 = e1.loss_and_grad(first=5, count=70)
    print("one target vs two", abs(l2 - l1) / abs(l1), util.relerr(g2, g1), util.elem_relerr(g2, g1, 1e-3))
    assert n1 == n2 and abs(l2 - l1) <= TOL * abs(l1) and util.relerr(g2, g1) <= TOL and util.elem_relerr(g2, g1, 1e-3) <= ETOL
    e1.close(); e2.close()


BATCHES = [(0, 128), (128, 128), (50, 200), (200, 150), (10, 70)]


@pytest.mark.parametrize("head,jit", [("fluxpart", 0), ("flux3", 1)], ids=["fluxpart", "flux3-compiled"])
def test_five_rmsprop_steps(head, jit):
    """the twin's fp64 gradient, the rule in NumPy fp32 (Optimisers.jl op for op): the bars of the three-step test of tests/test_gpu_seq.py"""
    model, fn_t, outs, X, frc, ys, W, ow, lam, starts, theta = _three_target_case(head, I=15, H=15, jit=jit)
    kinds = ("nseLoss", "mse", "mae")
    eng = _engine(model, X, frc, ys, W, ow, lam, starts, theta, jit, kinds)
    eng.opt_init("RMSProp", 0.001)
    for a, n in BATCHES:
        eng.train_step(a, n)
    if head != "fluxpart":
        assert eng.jit_status()[0] == jit
    th, v = theta.copy(), np.zeros_like(theta)
    for a, n in BATCHES:
        _, g, _ = mt.loss_and_grad(model, fn_t, outs, th, X, frc, ys, starts[a:a + n], W, ow, lam, kinds)
        g = g.astype(np.float32)
        v = np.float32(0.9) * v + np.float32(1 - 0.9) * g * g
        th = th - g * (np.float32(0.001) / (np.sqrt(v) + np.float32(1e-8)))
    d = np.abs(eng.get_params() - th)
    print("rmsprop", float(np.mean(d <= 2e-5)), float(d.max()))
    assert np.mean(d <= 2e-5) >= 0.999 and d.max() <= 2.5e-3, (np.mean(d <= 2e-5), d.max())
    eng.close()


# ---- train() ------------------------------------------------------------------------------------------------------------------------
def _flux_columns(rows, seed):
    """a seeded synthetic series for FluxPartModelQ10: two predictors that drive RUE and Rb, its three fluxes with noise and gaps of their own"""
    rng = np.random.default_rng(seed)
    x0 = (np.cumsum(0.6 * rng.standard_normal(rows)) * 0.2).astype(np.float32)
    x1 = (0.6 * rng.standard_normal(rows)).astype(np.float32)
    sw = rng.uniform(0.0, 800.0, rows).astype(np.float32)
    ta = (10 + 8 * rng.standard_normal(rows)).astype(np.float32)
    tr = ct.fluxpart_torch(SW_IN=torch.tensor(sw, dtype=torch.float64), TA=torch.tensor(ta, dtype=torch.float64),
                           RUE=torch.tensor(0.3 + 0.2 * np.tanh(x1.astype(np.float64))), Rb=torch.tensor(3.0 + np.tanh(x0.astype(np.float64))), Q10=2.0)
    cols = {"x0": x0, "x1": x1, "SW_IN": sw, "TA": ta}
    for name in ("NEE", "GPP", "RECO"):
        v = (tr[name].numpy() + 0.2 * rng.standard_normal(rows)).astype(np.float32)
        v[rng.random(rows) < 0.1] = np.nan
        cols[name] = v
    return cols


def _flux_model(targets=("NEE", "RECO")):
    return eh.constructHybridModel(["x0", "x1"], ["SW_IN", "TA"], list(targets), eh.FluxPartModelQ10, dict(ct.FLUXPART_TABLE), ["RUE", "Rb"], ["Q10"],
                                   hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(15, 15))), scale_nn_outputs=True)


SEQ_KW = dict(input_window=10, output_window=3, output_shift=1, lead_time=1)


def test_train_end_to_end():
    cols = _flux_columns(400, 3)
    kw = dict(batchsize=128, opt=eh.RMSProp(0.01), training_loss=eh.PerTarget(("nseLoss", "mse")), loss_types=["mse", "nse"], random_seed=1, return_model="final",
              sequence_kwargs=SEQ_KW)
    out = eh.train(_flux_model(), cols, nepochs=12, **kw)
    for t in ("NEE", "RECO"):                                   # the loss of every target falls
        assert out.train_history[-1]["mse"][t] < out.train_history[0]["mse"][t], t
    (_, _, wtr), (_, _, wva) = eh.split_data(cols, _flux_model(), sequence_kwargs=SEQ_KW)
    nva, ow = len(wva.starts), 3
    vp = out.val_obs_pred
    for t in ("NEE", "RECO"):                                   # the tables stay as for one target: one row per (window, j), a column pair per target
        assert vp[t + "_pred"].shape == (nva * ow,) and vp[t].shape == (nva * ow,) and np.isfinite(vp[t + "_pred"]).all()
        assert np.array_equal(vp[t], cols[t][wva.target_rows()].reshape(-1), equal_nan=True)
    assert not np.array_equal(vp["NEE_pred"], vp["RECO_pred"])
    more = eh.train(_flux_model(), cols, nepochs=3, train_from=out, **kw)          # continues from the returned parameters
    for t in ("NEE", "RECO"):
        assert more.train_history[0]["mse"][t] == out.train_history[-1]["mse"][t]
    assert not np.array_equal(more.ps, out.ps) and np.isfinite(more.ps).all()


def test_two_seeded_runs_of_a_three_target_model_are_the_same_bits():
    cols = _flux_columns(400, 5)
    kw = dict(nepochs=3, batchsize=128, opt=eh.RMSProp(0.01), training_loss=eh.PerTarget(("nseLoss", "mse", "mae")), loss_types=["mse", "nse"], random_seed=11,
              sequence_kwargs=SEQ_KW)
    a, b = [eh.train(_flux_model(("RECO", "NEE", "GPP")), cols, **kw) for _ in range(2)]
    assert np.array_equal(a.ps, b.ps) and a.best_epoch == b.best_epoch
    hist = lambda r: np.asarray([[h[lt][t] for lt in ("mse", "nse") for t in ("RECO", "NEE", "GPP")] for h in r.train_history + r.val_history])
    assert np.array_equal(hist(a), hist(b)) and len(a.train_history) == 4


def test_lbfgs_on_the_full_batch_decreases_the_objective():
    cols = _flux_columns(300, 7)
    out = eh.train(_flux_model(), cols, opt=eh.LBFGS(), full_batch=True, maxiters=15, eval_every=5, training_loss=eh.PerTarget(("nseLoss", "mse")), loss_types=["mse", "nse"],
                   random_seed=2, sequence_kwargs=SEQ_KW)
    first, last = out.train_history[0], out.train_history[-1]
    assert last["mse"]["NEE"] + last["mse"]["RECO"] < first["mse"]["NEE"] + first["mse"]["RECO"] and np.isfinite(out.ps).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_with_their_reasons():
    model, fn_t, outs, X, frc, ys, W, ow, lam, starts, theta = _three_target_case()
    eng = _engine(model, X, frc, ys, W, ow, lam, starts, theta)
    err = lambda: eng._lib.eh_last_error(eng._h)
    for what, call in (("rmse", lambda: eng.set_training_loss("rmse")), ("rmse", lambda: eng.set_training_loss(eh.PerTarget(("mse", "rmse", "mae")))),
                       ("training_loss", lambda: eng.set_training_loss("pearsonLoss")), ("pearson", lambda: eng.set_training_loss(eh.PerTarget(("mse", "pearsonLoss", "mae")))),
                       ("eh_graph_begin", lambda: eng.graph_begin()), ("eh_dp_grad", lambda: eng.dp_grad(0, 64))):
        with pytest.raises(NotImplementedError, match=what):
            call()
    roles = (C.c_int32 * 3)(0, 0, 1)
    assert eng._lib.eh_set_target_roles(eng._h, roles, 3) == L.EH_EUNSUPPORTED and b"extra_loss of the predictions" in err() and b"recorded loss" in err()
    assert eng._lib.eh_set_target_roles(eng._h, (C.c_int32 * 3)(0, 0, 0), 3) == L.EH_OK
    with pytest.raises(NotImplementedError):
        eng.set_training_loss(lambda yhat, y: np.mean(np.abs(yhat - y) ** 3))
    eng.set_training_loss(eh.PerTarget(("mae", "nseLoss", "mse")))          # what is built
    eng.close()
    d = cw.rbq10_model("lstm", 15, 15)[0].to_desc()              # two targets around single-output RbQ10
    d.n_targets = 2; d.target_output[1] = 0
    h = C.c_void_p()
    lib = L.lib()
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"around a model with one output" in lib.eh_last_error(None) and not h.value
    assert lib.eh_create_seq_targets(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"around a model with one output" in lib.eh_last_error(None) and not h.value
    d = model.to_desc()                                          # eh_create itself keeps its answer; several targets are asked for by name
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"several: eh_create_seq_targets" in lib.eh_last_error(None) and not h.value
