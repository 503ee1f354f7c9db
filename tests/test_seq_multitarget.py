"""Sequence models with several targets, without a GPU: the twin of tests/seq_multitarget_twin.py against central differences, against a
plain count over materialised windows and against the one-target twin; the parity cases of tests/seq_multitarget_cases.py as inputs; the
descriptor, the per-target losses and the prediction tables on the host; and what eh_create says before a device is touched."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
import easyhybrid_jl_amd.train  # noqa: F401  (the module; the package's `train` is the function)

from tests import seq_cells_twin as cw
from tests import seq_closure_twin as ct
from tests import seq_multitarget_cases as mc
from tests import seq_multitarget_twin as mt
from tests import seq_twin as tw
from tests import util

T = sys.modules["easyhybrid_jl_amd.train"]
TOL, ETOL = 1e-5, 5e-4          # the device's bars (tests/test_gpu_seq_closures.py); the twin's self-checks hold a tenth of them


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cell_act,head", [("lstm", "tanh", "fluxpart"), ("gru", "tanh", "flux3"), ("rnn", "relu", "fluxpart")])
def test_twin_gradient_is_the_central_difference(kind, cell_act, head):
    """autograd through the twin against central differences of its fp64 loss, every entry of theta, three targets with three loss kinds and
    masks of their own, agg = mean: the bar of tests/test_seq_cells.py (a tenth of the device's bars; step 1e-5: truncation ~1e-10,
    rounding ~1e-11)"""
    make = mt.fluxpart_model if head == "fluxpart" else mt.flux3_model
    names = ["RECO", "NEE", "GPP"] if head == "fluxpart" else ["reco", "nee", "gpp"]
    model, fn_t, outs = make(kind, names, 5, 4, cell_act=cell_act)
    X, frc, _ = ct.series()
    ys = mt.masked_targets(names, 77, 0.2, head)
    W, ow, lam, kinds = 5, 2, 1, ("nseLoss", "mse", "mae")
    sel = ct.all_starts(ct.LROWS, W, lam)[3:40]
    theta = model.initialparameters(5).astype(np.float64)
    _, g, nv = mt.loss_and_grad(model, fn_t, outs, theta, X, frc, ys, sel, W, ow, lam, kinds, "mean")
    assert (nv > 30).all() and np.isfinite(g).all()
    yt = torch.tensor(mt.targets_of(ys, sel, W, ow, lam), dtype=torch.float64)
    loss = lambda th: float(mt.loss_of(mt.forward(model, fn_t, outs, th, X, frc, sel, W, ow)[0], yt, kinds, "mean"))
    eps, fd = 1e-5, np.zeros_like(g)
    for i in range(len(theta)):
        e = np.zeros_like(theta); e[i] = eps
        fd[i] = (loss(theta + e) - loss(theta - e)) / (2 * eps)
    n = float(np.linalg.norm(fd))
    print(kind, head, "norm rel", abs(float(np.linalg.norm(g)) - n) / n, "entry rel", util.elem_relerr(g, fd, 1e-3))
    assert abs(float(np.linalg.norm(g)) - n) <= 0.1 * TOL * n
    assert util.elem_relerr(g, fd, 1e-3) <= 0.1 * ETOL


def test_twin_weights_are_a_plain_count_over_materialised_windows():
    """w_t = a / n_t (mse, mae), a / sum (y - mean y)^2 (nseLoss) over the (window, j) entries -- overlapping windows read a row of the
    series once each -- and sum_t w_t sum term_t is the twin's loss"""
    names = ["NEE", "GPP", "RECO"]
    ys = mt.masked_targets(names, 5, 0.2)
    ys[1][:] = np.nan                                           # a target without a valid entry: weight 0
    W, ow, lam, kinds = 6, 3, 1, ("mae", "mse", "nseLoss")
    sel = ct.all_starts(ct.LROWS, W, lam)[10:47]
    for agg, a in (("sum", 1.0), ("mean", 1.0 / 3.0)):
        w, n = mt.weights(ys, sel, W, ow, lam, kinds, agg)
        for t in range(3):
            vals = [float(ys[t][s + W - ow + j + lam]) for s in sel for j in range(ow)]          # the windows, materialised one by one
            vals = np.array([v for v in vals if not np.isnan(v)], np.float64)
            assert n[t] == len(vals)
            if t == 1:
                assert n[t] == 0 and w[t] == 0.0
            elif kinds[t] == "nseLoss":
                assert np.isclose(w[t], a / ((vals - vals.mean()) ** 2).sum(), rtol=1e-13)
            else:
                assert w[t] == a / len(vals)
        assert n[0] > len(set(sel)) and n[0] != np.count_nonzero(~np.isnan(ys[0][sel.min():sel.max() + W + lam]))      # (rows counted once per window)
        model, fn_t, outs = mt.fluxpart_model("lstm", names, 5, 4)
        theta = model.initialparameters(2)
        X, frc, _ = ct.series()
        yhat, _ = mt.predict(model, fn_t, outs, theta, X, frc, sel, W, ow)
        yt = mt.targets_of(ys, sel, W, ow, lam)
        by_w = 0.0
        for t in range(3):
            m = ~np.isnan(yt[t])
            r = yhat[t][m] - yt[t][m]
            by_w += w[t] * (np.abs(r).sum() if kinds[t] == "mae" else (r * r).sum())
        loss, _, nv = mt.loss_and_grad(model, fn_t, outs, theta, X, frc, ys, sel, W, ow, lam, kinds, agg)
        assert list(nv) == list(n) and np.isclose(loss, by_w, rtol=1e-12)


@pytest.mark.parametrize("kind", ["mse", "mae", "nseLoss"])
@pytest.mark.parametrize("target", ["NEE", "GPP", "RECO"])
def test_one_target_is_the_closure_twin_exactly(target, kind):
    model, fn_t, outs = mt.fluxpart_model("lstm", [target], 6, 2)
    m1, _, out = ct.fluxpart_model(target, 6, 2)
    X, frc, tg = ct.series()
    W, ow, lam = 5, 2, 1
    sel = ct.all_starts(ct.LROWS, W, lam)[:17]
    theta = model.initialparameters(31)
    l, g, nv = mt.loss_and_grad(model, fn_t, outs, theta, X, frc, [tg[target]], sel, W, ow, lam, (kind,))
    l1, g1, nv1 = ct.loss_and_grad(m1, fn_t, out, theta, X, frc, tg[target], sel, W, ow, lam, kind)
    assert outs == [out] and l == l1 and np.array_equal(g, g1) and int(nv[0]) == nv1
    assert np.array_equal(mt.predict(model, fn_t, outs, theta, X, frc, sel, W, ow)[0][0], ct.predict(m1, fn_t, out, theta, X, frc, sel, W, ow)[0])


# ---- the parity cases as inputs -----------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_they_must():
    cs = mc.CASES
    triples = {(c["widths"], c["head"], c["cell"]) for c in cs if c["T"] == 3 and c["ow"] == 3}
    assert len(triples) == len(mc.WIDTHS) * len(mc.HEADS) * len(mc.CELLS) == 36
    assert {c["T"] for c in cs} == {2, 3} and {c["ow"] for c in cs} == {1, 3} and {c["lam"] for c in cs} == {0, 1} and {c["count"] for c in cs} == {13, 37, 70}
    assert {c["agg"] for c in cs} == {"sum", "mean"} and {c["shuffled"] for c in cs} == {True, False}
    kinds = {c["kinds"] for c in cs}
    assert {("mse",) * 3, ("mae",) * 3, ("nseLoss",) * 3, ("nseLoss", "mse", "mae")} <= kinds
    assert any(c["targets"][:2] == ["RECO", "NEE"] for c in cs) and any(c["targets"] == ["reco", "gpp", "nee"] for c in cs)
    assert len(set(mc.IDS)) == len(cs)


@pytest.mark.parametrize("case", mc.CASES, ids=mc.IDS)
def test_case_inputs_are_well_posed(case):
    """every target of every case keeps at least two distinct valid observations among its (window, j) entries -- nseLoss's weight is finite
    -- and a mask of its own"""
    model, fn_t, outs, X, frc, ys, theta, sel, kw, starts, jit = mc.build(case)
    assert len(model.targets) == case["T"] == len(outs) and list(model.to_desc().target_output[:case["T"]]) == outs
    yt = mt.targets_of(ys, sel, mc.W, case["ow"], case["lam"])
    for t in range(case["T"]):
        v = yt[t][~np.isnan(yt[t])]
        assert len(np.unique(v)) >= 2
    masks = [np.isnan(y) for y in ys]
    assert all(not np.array_equal(masks[0], m) for m in masks[1:])
    w, n = mt.weights(ys, sel, mc.W, case["ow"], case["lam"], case["kinds"], case["agg"])
    assert np.isfinite(w).all() and (w > 0).all() and (n >= 2).all()
    # the predictions that are compared: NEE = RECO - GPP does not cancel (tests/seq_multitarget_cases.py)
    esel = starts[mc.EVAL_FIRST:mc.EVAL_FIRST + case["count"]]
    full, _ = mt.predict(model, fn_t, [0, 1, 2], theta, X, frc, esel, mc.W, case["ow"])          # nee | gpp | reco
    nee = np.abs(full[0])
    factor = float(np.max((np.abs(full[1]) + np.abs(full[2])) / np.maximum(nee, 1e-3 * nee.max())))
    assert factor <= mc.CANCEL_MAX, factor


# ---- host logic ---------------------------------------------------------------------------------------------------------------------
def test_descriptor_of_two_and_three_targets():
    for targets, want in ((["RECO", "NEE"], [2, 0]), (["GPP", "RECO", "NEE"], [1, 2, 0])):
        d = mt.fluxpart_model("lstm", targets, 15, 15)[0].to_desc()
        assert d.n_targets == len(targets) and list(d.target_output[:len(targets)]) == want and d.mech != L.EH_MECH_PROGRAM
    d = mt.flux3_model("gru", ["reco", "gpp"], 7, 20)[0].to_desc()
    assert d.n_targets == 2 and list(d.target_output[:2]) == [2, 1] and d.mech == L.EH_MECH_PROGRAM and d.prog_n_out == 3


class _Lib:
    """stands in for the library under HybridEngine.set_training_loss: records what reaches eh_set_target_losses / eh_set_option"""
    def __init__(self):
        self.calls = []

    def eh_set_target_losses(self, h, kinds, n):
        self.calls.append(("target_losses", [int(kinds[i]) for i in range(n)]))
        return L.EH_OK

    def eh_set_option(self, h, name, value):
        self.calls.append((name.decode(), int(value)))
        return L.EH_OK


def _stub_engine(targets):
    eng = object.__new__(eh.HybridEngine)
    eng._lib, eng._h, eng.n_pseudo, eng.target_names, eng.extra_entries = _Lib(), C.c_void_p(), 0, list(targets), []
    eng.n_targets_total, eng.n_par, eng.param_names = len(targets), 3, ["RUE", "Rb", "Q10"]
    return eng


def test_per_target_losses_reach_the_library_as_one_kind_per_target():
    """what becomes loss_t: 4 bits per target, in the order of the targets"""
    eng = _stub_engine(["RECO", "NEE", "GPP"])
    eng.set_training_loss(eh.PerTarget(("nseLoss", "mse", "mae")))
    assert eng._lib.calls == [("target_losses", [L.TRAINING_LOSSES[k] for k in ("nseLoss", "mse", "mae")])] and eng._loss_kinds == ["nseLoss", "mse", "mae"]
    eng = _stub_engine(["RECO", "NEE"])
    eng.set_training_loss("mae")
    assert eng._lib.calls == [("training_loss", L.TRAINING_LOSSES["mae"])]
    with pytest.raises(AssertionError, match="must match"):
        eng.set_training_loss(eh.PerTarget(("mse",)))


def test_prediction_arrays_are_windows_by_ow_per_target():
    eng = _stub_engine(["RECO", "NEE"])
    ys, ps, yp, pp = eng._outs(11, True, True, 3)
    assert [a.shape for a in ys] == [(11, 3)] * 2 and [a.shape for a in ps] == [(11, 3)] * 3 and len(yp) == 2 and len(pp) == 3

    class Eng:                                                  # the engine as _prediction_tables reads it
        n_samples = {L.EH_SPLIT_TRAIN: 11, L.EH_SPLIT_VAL: 4}
        seq_ow = {L.EH_SPLIT_TRAIN: 3, L.EH_SPLIT_VAL: 3}

        def forward(self, split):
            n = self.n_samples[split]
            out = {t: np.full((n, 3), k, np.float32) for k, t in enumerate(["RECO", "NEE"])}
            out["parameters"] = {"Rb": np.zeros((n, 3), np.float32)}
            return out

    class Model:
        targets = ["RECO", "NEE"]

    obs = lambda n: {t: np.zeros((n, 3), np.float32) for t in Model.targets}
    tr, va, dtr, dva = T._prediction_tables(Eng(), Model, obs(11), obs(4))
    for tab, n in ((tr, 11), (va, 4)):                           # the tables stay what they are for one target: one row per (window, j), a column pair per target
        assert set(tab) == {"RECO", "NEE", "RECO_pred", "NEE_pred"}
        assert all(v.shape == (n * 3,) for v in tab.values()) and (tab["NEE_pred"] == 1).all() and (tab["RECO_pred"] == 0).all()
    assert dtr["Rb"].shape == (33,) and dva["Rb"].shape == (12,)


def test_losses_a_sequence_model_does_not_train_on_are_refused_with_the_reason():
    cols = {k: np.zeros(40, np.float32) for k in ("x0", "x1", "SW_IN", "TA", "NEE", "RECO")}
    model = mt.fluxpart_model("lstm", ["NEE", "RECO"], 15, 15)[0]
    kw = dict(nepochs=1, batchsize=16, sequence_kwargs=dict(input_window=10, output_window=3, output_shift=1, lead_time=1))
    with pytest.raises(NotImplementedError, match="'rmse' on 2 targets needs a pass ahead of the step"):
        eh.train(model, cols, training_loss=eh.PerTarget(("rmse", "mse")), **kw)
    with pytest.raises(NotImplementedError, match="'rmse' on 2 targets"):
        eh.train(model, cols, training_loss="rmse", **kw)
    with pytest.raises(NotImplementedError, match="'pearsonLoss' needs the batch moments"):
        eh.train(model, cols, training_loss=eh.PerTarget(("mse", "pearsonLoss")), **kw)
    with pytest.raises(NotImplementedError, match="recorded loss"):
        eh.train(model, cols, training_loss=eh.PerTarget(("mse", lambda yh, y: np.mean((yh - y) ** 4))), **kw)
    with pytest.raises(NotImplementedError, match="extra_loss"):
        eh.train(model, cols, extra_loss=lambda yhat: np.mean(yhat["NEE"]), **kw)
    T._sequence_loss_check("rmse", 1)                           # one target: as before
    T._sequence_loss_check(eh.PerTarget(("nseLoss", "mse", "mae")), 3)


# ---- eh_create, before a device is touched --------------------------------------------------------------------------------------------
def test_eh_create_accepts_several_targets_and_refuses_with_the_reason():
    lib = L.lib()
    h = C.c_void_p()
    err = lambda: lib.eh_last_error(None)
    for kind, cell_act in mc.CELLS:
        for model in (mt.fluxpart_model(kind, ["RECO", "NEE"], 15, 15, cell_act=cell_act)[0], mt.fluxpart_model(kind, ["GPP", "RECO", "NEE"], 32, 32, cell_act=cell_act)[0],
                      mt.flux3_model(kind, ["nee", "reco"], 7, 20, cell_act=cell_act)[0], mt.flux3_model(kind, ["reco", "gpp", "nee"], 20, 7, cell_act=cell_act)[0]):
            d = model.to_desc()                                  # the descriptor is taken: the constructor gets as far as the device, or makes the handle
            rc = lib.eh_create_seq_targets(C.byref(d), C.byref(h))
            assert (rc == L.EH_EHIP and b"no HIP device" in err() and not h.value) or (rc == L.EH_OK and lib.eh_destroy(h) == L.EH_OK), err()
    d = cw.rbq10_model("lstm", 15, 15)[0].to_desc()              # several targets around a model with one output
    d.n_targets = 2; d.target_output[1] = 0
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"2 targets around a model with one output" in err() and not h.value
    d = mt.fluxpart_model("lstm", ["RECO", "NEE"], 15, 15)[0].to_desc()
    d.target_output[1] = 3                                       # an output the model does not have
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EINVAL and b"names an output the model does not have (it has 3)" in err() and not h.value
    # eh_create itself answers a sequence descriptor with several targets as it always has; they are asked for by name
    d = mt.fluxpart_model("lstm", ["RECO", "NEE"], 15, 15)[0].to_desc()
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"several: eh_create_seq_targets" in err() and not h.value
    rc = lib.eh_create_seq_targets(C.byref(d), C.byref(h))
    assert (rc == L.EH_EHIP and b"no HIP device" in err() and not h.value) or (rc == L.EH_OK and lib.eh_destroy(h) == L.EH_OK)
    d.target_output[1] = 3
    assert lib.eh_create_seq_targets(C.byref(d), C.byref(h)) == L.EH_EINVAL and b"names an output the model does not have" in err()
    d = cw.rbq10_model("lstm", 15, 15)[0].to_desc()
    d.n_targets = 2; d.target_output[1] = 0
    assert lib.eh_create_seq_targets(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"around a model with one output" in err()
    d = mt.fluxpart_model("lstm", ["RECO", "NEE"], 15, 15)[0].to_desc()
    d.n_targets = L.EH_MAX_TARG + 1
    assert lib.eh_create(C.byref(d), C.byref(h)) != L.EH_OK and not h.value
