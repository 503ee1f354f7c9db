"""-m gpu: sequence models around GRUCell and RNNCell on the device (csrc/eh_seq.hpp, template parameter CELL) against the fp64 torch
twin (tests/seq_cells_twin.py): loss and gradient on every pairing of block class and window count, index forms, the GRU's two n-block
biases, optimiser steps, evaluation and predictions, the three head forms, reproducibility, train() with L-BFGS, and the seeded fuzz of
tests/seq_cells_fuzz_cases.py.

Structure and tolerances are those of tests/test_gpu_seq.py and tests/test_gpu_seq_fuzz.py, unchanged: loss and gradient norm within 1e-5
relative of the fp64 twin, entry by entry within 5e-4 down to 1e-3 of the largest entry; the cells add sigma, tanh and fp32 MFMA
contractions over at most 32 terms, nothing of a new kind.  Every parity check first holds the twin's own fp32 run to a tenth of the bar.
(On an MI355X, 162 passed in 13 s; fuzz, worst loss / gradient norm / entry-wise error over the 40 seeds of a cell: GRU 8.2e-7 / 6.3e-7 /
4.2e-5, RNN 2.1e-7 / 2.4e-7 / 7.4e-5; per (NBI, NBH) class in DESIGN.md section 3.9.)"""
import sys

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
import easyhybrid_jl_amd.train  # noqa: F401
from oracle import hybrid_oracle as ho

from tests import seq_cells_fuzz_cases as cfz
from tests import seq_cells_twin as cw
from tests import seq_closure_twin as ct
from tests import seq_twin as tw
from tests import util

T = sys.modules["easyhybrid_jl_amd.train"]
pytestmark = pytest.mark.gpu

TOL, ETOL = 1e-5, 5e-4
E2E_REL, E2E_ABS, PTOL = 2e-5, 2e-6, 1e-5          # tests/test_gpu_eval.py
LROWS = ct.LROWS
CELLS = [("gru", "tanh"), ("rnn", "tanh")]
CELL_IDS = ["gru", "rnn"]


def _engine(model, X, frc, y, W, ow, lam, starts, theta, split=L.EH_SPLIT_TRAIN, jit=None):
    eng = model.engine(0)
    if jit is not None:
        eng.set_option("jit", jit)
    eng.set_data(split, X, [frc[f] for f in model.forcing], [y])
    eng.set_sequences(split, W, ow, lam, starts)
    eng.set_params(theta)
    return eng


def _compiled_or_not(eng, jit):
    """tests/test_gpu_seq_closures.py: jit = 1 ran the kernels compiled at run time, verified against the interpreter; jit = 0 did not"""
    n, log = eng.jit_status()
    assert n == jit, f"jit = {jit}, eh_jit_status reports {n} compiled kernels: {log[:600]}"


def _parity(what, loss, grad, nv, l64, g64, nv64):
    n64 = float(np.linalg.norm(g64))
    norm = float(np.linalg.norm(grad.astype(np.float64)))
    print(f"seq cells parity: loss rel {abs(loss - l64) / abs(l64):.2e}  norm rel {abs(norm - n64) / n64:.2e}  max rel {util.relerr(grad, g64):.2e}  "
          f"entry rel {util.elem_relerr(grad, g64, 1e-3):.2e}  n_valid {nv}  | {what}")
    assert nv == nv64
    assert abs(loss - l64) <= TOL * abs(l64), (loss, l64)
    assert abs(norm - n64) <= TOL * n64
    assert util.relerr(grad, g64) <= TOL, util.relerr(grad, g64)
    assert util.elem_relerr(grad, g64, 1e-3) <= ETOL, util.elem_relerr(grad, g64, 1e-3)


def _check(what, model, fn_t, out, eng, theta, X, frc, y, sel, W, ow, lam, kind, **kw):
    l64, g64, nv64 = cw.loss_and_grad(model, fn_t, out, theta, X, frc, y, sel, W, ow, lam, kind, torch.float64)
    l32, g32, _ = cw.loss_and_grad(model, fn_t, out, theta, X, frc, y, sel, W, ow, lam, kind, torch.float32)
    n64 = float(np.linalg.norm(g64))
    # the input itself: fp32 arithmetic reaches a tenth of the bar
    assert abs(l32 - l64) <= 0.1 * TOL * abs(l64) and abs(float(np.linalg.norm(g32)) - n64) <= 0.1 * TOL * n64, (l32, l64)
    assert util.elem_relerr(g32, g64, 1e-3) <= 0.1 * ETOL, util.elem_relerr(g32, g64, 1e-3)
    loss, grad, nv = eng.loss_and_grad(**kw)
    _parity(what, loss, grad, nv, l64, g64, nv64)
    return loss, grad


# ---- loss and gradient: every pairing of a block class and a window count, for both cells ---------------------------------------------
BLOCKS = [(6, 2), (15, 15), (5, 32), (20, 9), (32, 32), (17, 17)]       # (I, H); (17, 17): padding rows in a second block of both
WINDOWS = [(1, 1, 0), (7, 3, 0), (10, 1, 1), (6, 6, 1)]                   # (W, ow, lead time)
COUNTS = [1, 16, 17, 100, 300]                                            # 300 on one workgroup: more tiles than waves
LOSSES = ["mse", "mae", "nseLoss"]


def _variant(bi, ci):
    """-> (window, loss, RNN activation) of a pairing: each window and each loss meets each block class and each count"""
    kind = LOSSES[(bi + 2 * ci) % 3] if COUNTS[ci] > 1 else ("mse", "mae")[bi % 2]      # (nseLoss of one window with ow = 1 divides by zero)
    return WINDOWS[(bi + ci) % 4], kind, ("tanh", "relu")[(bi + ci // 2) % 2]


def test_every_pairing_is_covered():
    seen = {(bi, ci): _variant(bi, ci) for bi in range(len(BLOCKS)) for ci in range(len(COUNTS))}
    for bi in range(len(BLOCKS)):
        assert {seen[bi, ci][1] for ci in range(len(COUNTS))} == set(LOSSES) and {seen[bi, ci][2] for ci in range(len(COUNTS))} == {"tanh", "relu"}
        assert len({seen[bi, ci][0] for ci in range(len(COUNTS))}) == 4
    for ci in range(len(COUNTS)):
        assert len({seen[bi, ci][0] for bi in range(len(BLOCKS))}) == 4


@pytest.mark.parametrize("ci", range(len(COUNTS)), ids=[f"n{c}" for c in COUNTS])
@pytest.mark.parametrize("bi", range(len(BLOCKS)), ids=[f"I{i}H{h}" for i, h in BLOCKS])
@pytest.mark.parametrize("cell", ["gru", "rnn"])
def test_loss_and_gradient_against_the_twin(cell, bi, ci):
    (I, H), count = BLOCKS[bi], COUNTS[ci]
    (W, ow, lam), kind, cell_act = _variant(bi, ci)
    model, fn_t, out = cw.rbq10_model(cell, I, H, act=("tanh", "sigmoid")[ci % 2], cell_act=cell_act)
    X, frc, _ = ct.series()                                         # 400 rows, 10 % NaN targets
    y = ct.target_series(1)
    starts = ct.all_starts(LROWS, W, lam)
    theta = model.initialparameters(10 + bi)
    first = 0
    if count == 1:                                                  # the one window: the first with a valid target
        first = int(np.argmax(~np.isnan(tw.targets_of(y, starts, W, ow, lam)).all(1)))
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta)
    eng.set_training_loss(kind)
    if count == 300:
        eng.set_option("max_blocks", 1)                             # tests/test_gpu_seq.py test_several_tiles_per_wave: four or five tiles a wave
    _check(f"{cell}:{cell_act} I{I} H{H} W{W} ow{ow} lam{lam} n{count} {kind}", model, fn_t, out, eng, theta, X, frc, y, starts[first:first + count], W, ow, lam, kind,
           first=first, count=count)
    eng.close()


@pytest.mark.parametrize("cell,cell_act", CELLS, ids=CELL_IDS)
def test_shuffled_idx_and_output_shift_3(cell, cell_act):
    model, fn_t, out = cw.rbq10_model(cell, 15, 15, cell_act=cell_act)
    X, frc, _ = ct.series()
    y = ct.target_series(1)
    W, ow, lam = 10, 2, 1
    theta = model.initialparameters(4)
    starts = ct.all_starts(LROWS, W, lam)
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta)
    idx = np.random.default_rng(5).permutation(len(starts))[:77].astype(np.int32)
    _check("shuffled idx", model, fn_t, out, eng, theta, X, frc, y, starts[idx], W, ow, lam, "mse", idx=idx)
    eng.close()
    s3 = eh.split_into_sequences(X, y[None], input_window=W, output_window=ow, output_shift=3, lead_time=lam).starts
    assert s3[:3].tolist() == [0, 3, 6]
    eng = _engine(model, X, frc, y, W, ow, lam, s3, theta)
    _check("output_shift 3", model, fn_t, out, eng, theta, X, frc, y, s3[20:90], W, ow, lam, "mse", first=20, count=70)
    eng.close()


@pytest.mark.parametrize("I,H", [(6, 5), (17, 17)])
def test_gru_bias_gradients_differ_in_the_n_block_only(I, H):
    """b_hn sits inside the reset gate's product, b_in outside: their gradients differ; those of the r and z halves are one sum written
    twice.  A kernel that folds b_hn into b_in as the LSTM's are folded gets the first wrong (and the loss with it)."""
    model, fn_t, out = cw.rbq10_model("gru", I, H)
    X, frc, _ = ct.series()
    y = ct.target_series(1)
    W, ow, lam = 6, 2, 0
    starts = ct.all_starts(LROWS, W, lam)
    theta = model.initialparameters(1)
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta)
    _, grad = _check("gru biases", model, fn_t, out, eng, theta, X, frc, y, starts[:50], W, ow, lam, "mse", first=0, count=50)
    eng.close()
    _, g64, _ = cw.loss_and_grad(model, fn_t, out, theta, X, frc, y, starts[:50], W, ow, lam, "mse")
    o = I * 2 + I + 3 * H * I + 3 * H * H
    bih, bhh, r_ih, r_hh = grad[o:o + 3 * H], grad[o + 3 * H:o + 6 * H], g64[o:o + 3 * H], g64[o + 3 * H:o + 6 * H]
    assert np.array_equal(bih[:2 * H], bhh[:2 * H])
    assert np.abs(r_ih[2 * H:] - r_hh[2 * H:]).max() > 1e-2 * np.abs(r_ih[2 * H:]).max()             # they do differ, in the reference
    assert util.elem_relerr(bih[2 * H:], r_ih[2 * H:], 1e-3) <= ETOL and util.elem_relerr(bhh[2 * H:], r_hh[2 * H:], 1e-3) <= ETOL


def test_rnn_with_tanh_and_with_relu():
    """the cell's activation rides in the layer code: the same theta gives two different models, each its twin's"""
    X, frc, _ = ct.series()
    y = ct.target_series(1)
    W, ow, lam = 7, 3, 0
    starts = ct.all_starts(LROWS, W, lam)
    got = {}
    for cell_act in ("tanh", "relu", "swish"):
        model, fn_t, out = cw.rbq10_model("rnn", 20, 9, cell_act=cell_act)
        theta = model.initialparameters(12)
        eng = _engine(model, X, frc, y, W, ow, lam, starts, theta)
        got[cell_act] = _check(f"rnn {cell_act}", model, fn_t, out, eng, theta, X, frc, y, starts[:64], W, ow, lam, "mse", first=0, count=64)
        eng.close()
    assert got["tanh"][0] != got["relu"][0] != got["swish"][0]


# ---- optimiser steps ------------------------------------------------------------------------------------------------------------------
BATCHES = [(0, 128), (128, 128), (50, 200)]


def _tutorial_case(cell, cell_act):
    model, fn_t, out = cw.rbq10_model(cell, 15, 15, cell_act=cell_act)
    X, frc, _ = ct.series()
    W, ow, lam = 10, 1, 1
    return model, fn_t, out, X, frc, ct.target_series(1), W, ow, lam, ct.all_starts(LROWS, W, lam), model.initialparameters(21)


def _twin_steps(model, fn_t, out, theta, X, frc, y, starts, W, ow, lam, rule):
    """the three steps with the twin's fp64 gradient and the optimiser rule in NumPy fp32 (Optimisers.jl op for op)"""
    th, state = theta.copy(), {}
    for a, n in BATCHES:
        _, g, _ = cw.loss_and_grad(model, fn_t, out, th, X, frc, y, starts[a:a + n], W, ow, lam, "mse", torch.float64)
        th = rule(th, g.astype(np.float32), state)
    return th


def _rmsprop(lr, rho=0.9, eps=1e-8):
    def rule(th, g, st):
        st["v"] = np.float32(rho) * st.get("v", np.zeros_like(th)) + np.float32(1 - rho) * g * g
        return th - g * (np.float32(lr) / (np.sqrt(st["v"]) + np.float32(eps)))
    return rule


@pytest.mark.parametrize("cell,cell_act", CELLS, ids=CELL_IDS)
def test_three_descent_and_three_rmsprop_steps(cell, cell_act):
    model, fn_t, out, X, frc, y, W, ow, lam, starts, theta = _tutorial_case(cell, cell_act)
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta)
    eng.opt_init("Descent", 0.05)
    for a, n in BATCHES:
        eng.train_step(a, n)
    ref = _twin_steps(model, fn_t, out, theta, X, frc, y, starts, W, ow, lam, lambda th, g, st: th - np.float32(0.05) * g)
    d = float(np.max(np.abs(eng.get_params() - ref)))
    print("descent max|dtheta|", d)
    assert d <= 1e-5 * max(1.0, float(np.max(np.abs(ref))))             # tests/test_gpu_seq.py test_three_descent_steps
    eng.close()
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta)
    eng.opt_init("RMSProp", 0.001)
    for a, n in BATCHES:
        eng.train_step(a, n)
    ref = _twin_steps(model, fn_t, out, theta, X, frc, y, starts, W, ow, lam, _rmsprop(0.001))
    d = np.abs(eng.get_params() - ref)
    print("rmsprop", float(np.mean(d <= 2e-5)), float(d.max()))
    assert np.mean(d <= 2e-5) >= 0.999 and d.max() <= 2.5e-3, (np.mean(d <= 2e-5), d.max())      # tests/test_gpu_seq.py test_three_rmsprop_steps
    eng.close()


@pytest.mark.parametrize("cell,cell_act", CELLS, ids=CELL_IDS)
def test_a_minibatch_without_a_valid_target_changes_nothing(cell, cell_act):
    model, fn_t, out, X, frc, y, W, ow, lam, starts, theta = _tutorial_case(cell, cell_act)
    y = y.copy()
    y[:40] = np.nan                                             # every target of windows 0 .. 29
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta)
    eng.opt_init("Adam", 0.01)
    eng.train_step(100, 64)
    th1 = eng.get_params()
    m1, v1, bt1 = eng.get_opt_state()
    assert not np.array_equal(th1, theta)
    loss = eng.train_step(0, 29)
    assert np.isnan(loss)
    m2, v2, bt2 = eng.get_opt_state()
    assert np.array_equal(eng.get_params(), th1) and np.array_equal(m1, m2) and np.array_equal(v1, v2) and np.array_equal(np.asarray(bt1), np.asarray(bt2))
    l, g, nv = eng.loss_and_grad(first=0, count=29)
    assert nv == 0 and np.isnan(l)
    eng.close()


# ---- evaluation, predictions, the other head forms ------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * np.max(np.abs(b)))))


@pytest.mark.parametrize("cell,cell_act", CELLS, ids=CELL_IDS)
def test_evaluation_and_predictions(cell, cell_act):
    I, H, W, ow, lam = 20, 9, 7, 3, 0
    model, fn_t, out = cw.rbq10_model(cell, I, H, cell_act=cell_act)
    X, frc, _ = ct.series()
    y = ct.target_series(1)
    starts = ct.all_starts(LROWS, W, lam)
    theta = model.initialparameters(6)
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta, split=L.EH_SPLIT_VAL)
    first, count = 7, 301
    sel = starts[first:first + count]
    pred, par = cw.predict(model, fn_t, out, theta, X, frc, sel, W, ow)
    yt = tw.targets_of(y, sel, W, ow, lam)
    metrics, yh = eng.eval(L.EH_SPLIT_VAL, first, count, predictions=True)
    assert yh["reco"].shape == (count, ow)
    bad = util.metric_mismatches(metrics[0], ho.metrics_ref(pred.ravel(), yt.ravel(), ~np.isnan(yt.ravel())), E2E_REL, E2E_ABS)
    assert not bad, bad
    res = eng.forward(L.EH_SPLIT_VAL, first, count)
    assert res["reco"].shape == (count, ow) and np.array_equal(res["reco"], yh["reco"])
    assert _rel(res["reco"], pred) <= PTOL, _rel(res["reco"], pred)
    for name in model.mechanistic_model.params:
        assert res["parameters"][name].shape == (count, ow)
        assert _rel(res["parameters"][name], par[name]) <= PTOL, (name, _rel(res["parameters"][name], par[name]))
    eng.close()


@pytest.mark.parametrize("cell,cell_act", CELLS, ids=CELL_IDS)
def test_fluxpart_with_the_target_on_output_1(cell, cell_act):
    model, fn_t, out = cw.fluxpart_model(cell, "GPP", 6, 2, cell_act=cell_act)
    assert out == 1
    X, frc, tg = ct.series()
    W, ow, lam = 5, 2, 1
    starts = ct.all_starts(LROWS, W, lam)
    theta = model.initialparameters(31)
    eng = _engine(model, X, frc, tg["GPP"], W, ow, lam, starts, theta)
    _check("fluxpart GPP", model, fn_t, out, eng, theta, X, frc, tg["GPP"], starts[:33], W, ow, lam, "mse", first=0, count=33)
    pred, _ = cw.predict(model, fn_t, out, theta, X, frc, starts[:33], W, ow)
    got = eng.forward(L.EH_SPLIT_TRAIN, 0, 33)
    assert got["GPP"].shape == (33, ow) and _rel(got["GPP"], pred) <= PTOL, _rel(got["GPP"], pred)
    eng.close()


@pytest.mark.parametrize("jit", [0, 1], ids=["interpreted", "compiled"])
@pytest.mark.parametrize("cell,cell_act", CELLS, ids=CELL_IDS)
def test_a_recorded_closure(cell, cell_act, jit):
    """closure 2 (three outputs, the target on `reco`): the interpreter, and the kernels compiled at run time around the program --
    which take over only once their training pass has agreed with the interpreter's (eh_jit_status counts them then)"""
    I, H, W, ow, lam = 20, 9, 7, 3, 0
    model, fn_t, out = cw.closure_model(cell, 2, I, H, cell_act=cell_act)
    X, frc, _ = ct.series()
    y = ct.target_series(2)
    starts = ct.all_starts(LROWS, W, lam)
    theta = model.initialparameters(41)
    eng = _engine(model, X, frc, y, W, ow, lam, starts, theta, jit=jit)
    eng.set_training_loss("nseLoss")
    _check(f"closure 2 jit={jit}", model, fn_t, out, eng, theta, X, frc, y, starts[:70], W, ow, lam, "nseLoss", first=0, count=70)
    _compiled_or_not(eng, jit)
    pred, _ = cw.predict(model, fn_t, out, theta, X, frc, starts[:70], W, ow)
    got = eng.forward(L.EH_SPLIT_TRAIN, 0, 70)
    assert _rel(got["reco"], pred) <= PTOL, _rel(got["reco"], pred)
    eng.close()


# ---- train() -----------------------------------------------------------------------------------------------------------------------------
def _cols(rows, seed):
    c = eh.synthetic.make_synth_rbq10(rows, seed, 0.05)
    c["sw_pot"] = (c["sw_pot"] / np.float32(50)).astype(np.float32)
    c["dsw_pot"] = (c["dsw_pot"] / np.float32(50)).astype(np.float32)
    return c


def _tutorial_model(cell, cell_act):
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ct.RBQ10_TABLE), ["rb"], ["Q10"],
                                   hidden_layers=cw.chain(cell, 15, 15, cell_act), activation="tanh", scale_nn_outputs=True)


SEQ_KW = dict(input_window=10, output_window=1, output_shift=1, lead_time=1)


@pytest.mark.parametrize("cell,cell_act", CELLS, ids=CELL_IDS)
def test_two_seeded_runs_are_the_same_bits(cell, cell_act):
    cols = _cols(600, 3)
    a, b = [eh.train(_tutorial_model(cell, cell_act), cols, nepochs=3, batchsize=128, opt=eh.RMSProp(0.01), random_seed=11, loss_types=["mse", "nse"],
                     sequence_kwargs=SEQ_KW) for _ in range(2)]
    assert a.ps.shape == ({"gru": 1742, "rnn": 782}[cell],)
    assert np.array_equal(a.ps, b.ps) and a.best_epoch == b.best_epoch
    ha = [[h[lt]["reco"] for lt in ("mse", "nse")] for h in a.train_history + a.val_history]
    hb = [[h[lt]["reco"] for lt in ("mse", "nse")] for h in b.train_history + b.val_history]
    assert np.array_equal(np.asarray(ha), np.asarray(hb)) and len(a.train_history) == 4
    assert np.isfinite(a.val_obs_pred["reco_pred"]).all() and a.train_history[-1]["mse"]["reco"] < a.train_history[0]["mse"]["reco"]


@pytest.mark.parametrize("cell,cell_act", CELLS, ids=CELL_IDS)
def test_lbfgs_lowers_the_loss(cell, cell_act):
    res = eh.train(_tutorial_model(cell, cell_act), _cols(600, 5), opt=eh.LBFGS(), full_batch=True, maxiters=5, random_seed=2, sequence_kwargs=SEQ_KW)
    st, trace = res.lbfgs_status, res.lbfgs_trace
    print("lbfgs", st, [r["f"] for r in trace])
    assert 1 <= st["iterations"] <= 5 and len(trace) == st["iterations"]
    assert trace[-1]["f"] < trace[0]["f"] and all(b["f"] <= a["f"] for a, b in zip(trace, trace[1:]))      # (the status's f0 is the last accepted value)
    assert st["f0"] == trace[-1]["f"]
    val = [h["mse"]["sum"] for h in res.val_history]
    assert np.isfinite(val).all()
    res.release()


# ---- the seeded fuzz -------------------------------------------------------------------------------------------------------------------
FUZZ = [(cell, seed) for cell in cfz.CELLS for seed in range(cfz.N_PER_CELL)]


@pytest.mark.parametrize("cell,seed", FUZZ, ids=[f"{c}-{s}" for c, s in FUZZ])
def test_random_sequence_model_matches_the_twin(cell, seed):
    """tests/test_gpu_seq_fuzz.py `_run`, loss and gradient: a case the generator accepted must pass -- there is no skip"""
    c = cfz.case(cell, seed)
    l64, g64, nv64 = c.ref
    eng = c.model.engine(0)
    if c.jit is not None:
        eng.set_option("jit", c.jit)
    eng.set_data(L.EH_SPLIT_TRAIN, c.X, [c.frc[f] for f in c.model.forcing], [c.y])
    eng.set_sequences(L.EH_SPLIT_TRAIN, c.W, c.ow, c.lam, c.starts)
    eng.set_params(c.theta)
    eng.set_training_loss(c.kind)
    if c.max_blocks is not None:
        eng.set_option("max_blocks", c.max_blocks)
    loss, grad, nv = eng.loss_and_grad(**c.kw)
    if c.jit is not None:
        _compiled_or_not(eng, c.jit)
    again = eng.loss_and_grad(**c.kw)
    eng.close()
    _parity(cfz.describe(c), loss, grad, nv, l64, g64, nv64)
    assert again[0] == loss and again[2] == nv and np.array_equal(again[1], grad)      # the same bits
