"""LayerNorm layers inside hidden-layer chains on the device (csrc/eh_lnl.hpp, on the layer-wise form) against the torch twin
(tests/ln_chain_twin.py, fp64): loss and gradient, optimiser steps, evaluation and predictions, reproducibility, the train() front door,
L-BFGS, graph capture, the data-parallel seam, a chain with both normalisers, refusals on a live handle.

Tolerances are the project's own (tests/test_gpu_bn_chain.py): loss and gradient norm within 1e-5 relative of the fp64 twin, the worst
entry within 1e-5 of the largest, entry by entry within 5e-4 down to 1e-3 of the largest entry.  Every parity check first holds the
twin's own fp32 run to a tenth of each bar: an ill-conditioned input fails as an input."""
import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L

from tests import lbfgs_twin
from tests import ln_chain_twin as tw
from tests import util
from tests.test_gpu_bn_chain import ETOL, PTOL, RBQ10, ROWS, TOL, cols_of, data, engine_of, make_model, rows_of, theta_of, val_mse

pytestmark = pytest.mark.gpu

WIDTHS, COUNTS = [1, 5, 16, 17, 64, 65, 130], [1, 5, 17, 64, 300]
POSITIONS = ["first", "last", "two", "noaffine", "activation"]
SECOND = {1: 4, 5: 8, 16: 17, 17: 12, 64: 65, 65: 64, 130: 16, 1024: 16}      # the second width of a chain: another segment / elements-per-lane geometry


def chain_of(position, n):
    """the layer positions of the issue around width n"""
    m = SECOND[n]
    return {"first": lambda: eh.Chain(eh.LayerNorm(n), eh.Dense(n, m, "tanh")),
            "last": lambda: eh.Chain(eh.Dense(n, n, "swish"), eh.LayerNorm(n, "sigmoid")),
            "two": lambda: eh.Chain(eh.LayerNorm(n), eh.Dense(n, m, "tanh"), eh.LayerNorm(m, "relu")),
            "noaffine": lambda: eh.Chain(eh.Dense(n, n, "tanh"), eh.LayerNorm(n, "swish", affine=False), eh.Dense(n, m, "sigmoid")),
            "activation": lambda: eh.Chain(eh.LayerNorm(n, "tanh"), eh.Dense(n, n, "sigmoid"))}[position]()


def twin_pair(model, theta, X, ta, y, rows, kind):
    """(loss, gradient, n_valid) of the fp64 twin, and how far the twin's own fp32 run is from it in units of a TENTH of each bar"""
    f = {model.forcing[0]: ta}
    l64, g64, nv64 = tw.loss_and_grad(model, theta, X, f, y, rows, kind, torch.float64)
    l32, g32, _ = tw.loss_and_grad(model, theta, X, f, y, rows, kind, torch.float32)
    n64 = float(np.linalg.norm(g64))
    own = max(abs(l32 - l64) / abs(l64) / (0.1 * TOL), abs(float(np.linalg.norm(g32)) - n64) / n64 / (0.1 * TOL),
              util.relerr(g32, g64) / (0.1 * TOL), util.elem_relerr(g32, g64, 1e-3) / (0.1 * ETOL))
    return (l64, g64, nv64), own


def conditioned_theta(model, X, ta, y, rows, kind, seed):
    """The parameters of a case: the first of seed, seed + 100, ... (twelve at most) at which fp32 arithmetic itself -- the twin's fp32 run
    against its fp64 run, nothing of the device -- stays within 0.7 of the tenth of every bar (tests/test_gpu_bn_chain.py's scheme)."""
    for j in range(12):
        theta = theta_of(model, seed + 100 * j)
        if twin_pair(model, theta, X, ta, y, rows, kind)[1] <= 0.7:
            return theta
    pytest.fail("no well-conditioned parameters among twelve draws: the case itself is ill-conditioned")


def variant(wi, ci):
    """position, loss, mechanistic model, shuffled idx of a case: every one of each over the thirty-five cases"""
    k = wi * len(COUNTS) + ci
    kind = "mse" if COUNTS[ci] == 1 else ("mse", "mae", "nseLoss")[k % 3]      # (one row: nseLoss has no variance to divide by)
    return POSITIONS[(wi + ci) % 5], kind, ("rbq10", "expo")[(k // 2) % 2], k % 2 == 1


def parity_case(wi, ci):
    """everything of a parity case that needs no device"""
    n, count = WIDTHS[wi], COUNTS[ci]
    position, kind, mech, shuffled = variant(wi, ci)
    model = make_model(chain_of(position, n), mech)
    X, ta, y = data()
    rows, as_idx = rows_of(y, count, shuffled, 3 + ci)
    return model, X, ta, y, rows, as_idx, kind, conditioned_theta(model, X, ta, y, rows, kind, 10 + wi)


def check(model, eng, theta, X, ta, y, rows, as_idx, kind):
    (l64, g64, nv64), own = twin_pair(model, theta, X, ta, y, rows, kind)
    n64 = float(np.linalg.norm(g64))
    assert own <= 1.0, own                                            # the input itself: fp32 arithmetic reaches a tenth of every bar
    eng.set_training_loss(kind)
    loss, grad, nv = eng.loss_and_grad(idx=rows) if as_idx else eng.loss_and_grad(first=int(rows[0]), count=len(rows))
    gn = float(np.linalg.norm(grad.astype(np.float64)))
    print(f"ln chain parity: loss rel {abs(loss - l64) / abs(l64):.2e}  norm rel {abs(gn - n64) / n64:.2e}  max rel {util.relerr(grad, g64):.2e}  "
          f"entry rel {util.elem_relerr(grad, g64, 1e-3):.2e}  n_valid {nv}")
    assert nv == nv64
    assert abs(loss - l64) <= TOL * abs(l64), (loss, l64)
    assert abs(gn - n64) <= TOL * n64
    assert util.relerr(grad, g64) <= TOL, util.relerr(grad, g64)
    assert util.elem_relerr(grad, g64, 1e-3) <= ETOL, util.elem_relerr(grad, g64, 1e-3)
    return grad


@pytest.mark.parametrize("ci", range(len(COUNTS)), ids=[f"B{c}" for c in COUNTS])
@pytest.mark.parametrize("wi", range(len(WIDTHS)), ids=[f"n{w}" for w in WIDTHS])
def test_loss_and_gradient_against_the_twin(wi, ci):
    model, X, ta, y, rows, as_idx, kind, theta = parity_case(wi, ci)
    eng = engine_of(model, X, ta, y, theta)
    grad = check(model, eng, theta, X, ta, y, rows, as_idx, kind)
    if WIDTHS[wi] == 1 and variant(wi, ci)[0] in ("first", "activation"):
        # one feature: zero variance, xh = 0, and nothing flows into the Dense layer in front of the LayerNorm -- its gradient is zero, exactly
        assert not grad[:model.NN[0][0] * model.NN[0][1] + model.NN[0][0]].any()
    eng.close()


def test_every_variant_is_covered():
    seen = {variant(wi, ci) for wi in range(len(WIDTHS)) for ci in range(len(COUNTS))}
    assert {v[0] for v in seen} == set(POSITIONS) and {v[1] for v in seen} == {"mse", "mae", "nseLoss"}
    assert {v[2] for v in seen} == {"rbq10", "expo"} and {v[3] for v in seen} == {True, False}
    for n in WIDTHS:                                                    # every position at every width
        assert len({variant(WIDTHS.index(n), ci)[0] for ci in range(len(COUNTS))}) == 5


@pytest.mark.parametrize("position", POSITIONS)
def test_behind_an_input_batchnorm(position):
    model = make_model(chain_of(position, 17), "rbq10", "sigmoid", input_batchnorm=True, P=3)
    X, ta, y = data(3)
    rows, as_idx = rows_of(y, 300 if position == "two" else 64, position != "last", 9)
    theta = conditioned_theta(model, X, ta, y, rows, "mse", 5)
    eng = engine_of(model, X, ta, y, theta)
    check(model, eng, theta, X, ta, y, rows, as_idx, "mse")
    eng.close()


def test_width_1024_sixteen_elements_per_lane():
    model = make_model(eh.Chain(eh.LayerNorm(1024, "tanh"), eh.Dense(1024, 16, "tanh")), "rbq10")
    X, ta, y = data()
    rows = np.arange(20, 84, dtype=np.int32)
    theta = conditioned_theta(model, X, ta, y, rows, "mse", 3)
    eng = engine_of(model, X, ta, y, theta)
    check(model, eng, theta, X, ta, y, rows, False, "mse")
    eng.close()


def test_predictors_far_from_zero():
    """predictors fifty sigma from zero (data(offset=True)): the rows of the first layer share a large common part, which the mean-first
    statistics of the LayerNorm behind it remove before anything is squared"""
    model = make_model(eh.Chain(eh.LayerNorm(16), eh.Dense(16, 17, "tanh"), eh.LayerNorm(17)), "rbq10", "identity")
    X, ta, y = data(2, offset=True)
    assert np.all(np.abs(X.mean(1)) / X.std(1) > 40)
    rows = np.arange(40, 104, dtype=np.int32)
    theta = conditioned_theta(model, X, ta, y, rows, "mse", 6)
    eng = engine_of(model, X, ta, y, theta)
    check(model, eng, theta, X, ta, y, rows, False, "mse")
    eng.close()


def test_a_chain_with_both_normalisers():
    model = make_model(eh.Chain(eh.BatchNorm(16), eh.Dense(16, 17, "tanh"), eh.LayerNorm(17, "relu"), eh.Dense(17, 8, "sigmoid"), eh.BatchNorm(8, affine=False)))
    X, ta, y = data()
    rows, as_idx = rows_of(y, 64, True, 4)
    theta = conditioned_theta(model, X, ta, y, rows, "mse", 8)
    eng = engine_of(model, X, ta, y, theta)
    check(model, eng, theta, X, ta, y, rows, as_idx, "mse")
    with pytest.raises(NotImplementedError, match="eh_graph_begin.*BatchNorm layers in the chain"):      # BatchNorm's refusals apply
        eng.graph_begin()
    with pytest.raises(eh.EngineError, match="hidden layer 3 is no BatchNorm layer"):                   # the LayerNorm layer has no state
        eng.get_layer_state(3)
    assert eng.get_layer_state(1)[1].shape == (16,)
    eng.close()


BATCHES = [(0, 128), (128, 128), (50, 200), (7, 64), (300, 100), (0, 400)]


def steps_case():
    model = make_model(eh.Chain(eh.Dense(16, 17, "tanh"), eh.LayerNorm(17), eh.Dense(17, 8, "relu"), eh.LayerNorm(8, "sigmoid", epsilon=1e-3)), input_batchnorm=True)
    X, ta, y = data()
    return model, X, ta, y, theta_of(model, 21)


def test_six_adam_steps_evaluation_and_predictions():
    """Six Adam steps against the twin's trajectory (its fp64 gradient, the rule in fp32).  The bar: Adam's first steps are sign-like, an
    entry moves by about lr a step whatever its size, and an entry of the gradient is right to ETOL relative (the parity bar above) -- so a
    step may differ by lr * ETOL, six of them by 6 * lr * ETOL = 3e-5."""
    model, X, ta, y, theta = steps_case()
    eng = engine_of(model, X, ta, y, theta)
    eng.set_data(L.EH_SPLIT_VAL, X, [ta], [y])
    lr = 1e-2
    eng.opt_init("Adam", lr)
    for a, n in BATCHES:
        eng.train_step(a, n)
    ref, state = tw.train_steps(model, theta, X, {"ta": ta}, y, BATCHES, tw.adam(lr))
    got = eng.get_params()
    d = float(np.max(np.abs(got - ref)))
    print("Adam, six steps: max|dtheta|", d)
    assert d <= 6 * lr * ETOL * max(1.0, float(np.max(np.abs(ref))))
    # evaluation and predictions: the train-mode pass (the input BatchNorm on its running statistics), nothing kept
    first, count = 7, 301
    rows = np.arange(first, first + count)
    pred, par = tw.predict(model, got, X, {"ta": ta}, rows, {"in": eng.get_bn_state()})
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * np.max(np.abs(b)))))
    out = eng.forward(L.EH_SPLIT_VAL, first, count)
    assert rel(out["reco"], pred) <= PTOL, rel(out["reco"], pred)
    assert rel(out["parameters"]["rb"], par["rb"]) <= PTOL
    metrics, yh = eng.eval(L.EH_SPLIT_VAL, first, count, predictions=True)
    assert np.array_equal(yh["reco"], out["reco"])
    ok = ~np.isnan(y[rows])
    assert metrics[0]["n"] == ok.sum() and metrics[0]["mse"] == pytest.approx(float(np.mean((pred[ok] - y[rows][ok].astype(np.float64)) ** 2)), rel=2e-5)
    eng.close()


def test_evaluation_is_the_training_forward():
    """no state and no mode: the loss eh_loss_and_grad reports (train mode) is the mse eh_eval reports of the same rows"""
    model = make_model(eh.Chain(eh.LayerNorm(17, "swish"), eh.Dense(17, 8, "tanh"), eh.LayerNorm(8)))
    X, ta, y = data()
    eng = engine_of(model, X, ta, y, theta_of(model, 2))
    loss, _, nv = eng.loss_and_grad(first=11, count=300)
    metrics = eng.eval(L.EH_SPLIT_TRAIN, 11, 300)
    metrics = metrics[0] if isinstance(metrics, tuple) else metrics
    assert metrics[0]["n"] == nv and metrics[0]["mse"] == pytest.approx(loss, rel=1e-5)      # (two fp32 sums of the same 300 terms, in two orders)
    eng.close()


def tutorial_model(input_batchnorm=True):
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], activation="sigmoid", scale_nn_outputs=True,
                                   hidden_layers=eh.Chain(eh.Dense(16, 16, "sigmoid"), eh.LayerNorm(16), eh.Dense(16, 8, "sigmoid"), eh.LayerNorm(8)), input_batchnorm=input_batchnorm)


def test_two_seeded_runs_are_the_same_bits():
    cols = cols_of(600, 3)
    a, b = [eh.train(tutorial_model(), cols, nepochs=4, batchsize=128, opt=eh.Adam(0.01), random_seed=11, loss_types=["mse", "nse"]) for _ in range(2)]
    assert np.array_equal(a.ps, b.ps) and a.best_epoch == b.best_epoch and a.best_loss == b.best_loss
    assert "st_layers" not in a.st                                      # no layer state to keep
    ha = [[h[lt]["reco"] for lt in ("mse", "nse")] for h in a.train_history + a.val_history]
    hb = [[h[lt]["reco"] for lt in ("mse", "nse")] for h in b.train_history + b.val_history]
    assert np.array_equal(np.asarray(ha), np.asarray(hb)) and len(a.train_history) == 5


def test_train_front_door_then_train_from():
    cols = cols_of(2000, 5)
    kw = dict(batchsize=128, opt=eh.Adam(0.01), random_seed=1, loss_types=["mse", "nse"])
    out = eh.train(tutorial_model(False), cols, nepochs=12, patience=5, return_model="final", **kw)
    print("validation mse", out.val_history[0]["mse"]["sum"], "->", out.val_history[-1]["mse"]["sum"])
    assert out.val_history[-1]["mse"]["sum"] < out.val_history[0]["mse"]["sum"]
    assert np.isfinite(out.val_obs_pred["reco_pred"]).all() and out.ps.size == tutorial_model(False).n_theta
    # the predictions of the returned model give the last validation loss again: evaluation needs the parameters alone
    assert val_mse(out) == pytest.approx(out.val_history[-1]["mse"]["sum"], rel=1e-5)
    b = eh.train(tutorial_model(False), cols, nepochs=0, train_from=out, **kw)
    assert np.array_equal(b.ps, out.ps) and b.val_history[0]["mse"]["sum"] == out.val_history[-1]["mse"]["sum"]
    c = eh.train(tutorial_model(False), cols, nepochs=2, train_from=out, return_model="final", **kw)
    assert not np.array_equal(c.ps, out.ps) and np.isfinite(c.ps).all()


def lbfgs_case():
    model = make_model(eh.Chain(eh.Dense(16, 16, "tanh"), eh.LayerNorm(16), eh.Dense(16, 8, "tanh"), eh.LayerNorm(8, "tanh")))
    X, ta, y = data()
    return model, X, ta, y, theta_of(model, 4)


LBFGS_ITERS = 4


def lbfgs_refs():
    """the twin's fp64 and fp32 solves around the chain twin's fp64 objective (no device)"""
    model, X, ta, y, theta = lbfgs_case()
    rows = np.arange(ROWS)

    def fg(x):
        l, g, nv = tw.loss_and_grad(model, np.asarray(x, np.float64), X, {"ta": ta}, y, rows)
        return l, g, float(nv)
    return lbfgs_twin.lbfgs(fg, theta, LBFGS_ITERS), lbfgs_twin.lbfgs(fg, theta, LBFGS_ITERS, dtype=np.float32)


def test_lbfgs_against_the_twin():
    """one L-BFGS solve (csrc/eh_lbfgs.hpp) against tests/lbfgs_twin.py around the chain twin's fp64 objective; bars and scheme of
    tests/test_gpu_lbfgs.py (the twin's own fp32 run is held to a tenth of the bar first)"""
    from tests.test_gpu_lbfgs import against_twin, solve
    model, X, ta, y, theta = lbfgs_case()
    ref, ref32 = lbfgs_refs()
    eng = engine_of(model, X, ta, y, theta)
    st, trace, got = solve(eng, LBFGS_ITERS)
    against_twin(st, trace, got, ref, ref32, "LayerNorm chain")
    eng.close()


def test_lbfgs_through_the_front_door():
    res = eh.train(tutorial_model(False), cols_of(1000, 9), opt=eh.LBFGS(), full_batch=True, maxiters=10, eval_every=5, random_seed=3)
    val = [h["mse"]["sum"] for h in res.val_history]
    print(f"LBFGS front door: validation mse {val}, status {res.lbfgs_status}")
    assert res.lbfgs_status["iterations"] >= 1 and np.isfinite(val).all() and val[-1] < val[0]
    res.release()


def test_weight_l2_rides_along():
    """loss + lambda * sum of the squared Dense weights (the LayerNorm leaves are not read): value and gradient against the twin"""
    model = make_model(eh.Chain(eh.Dense(16, 17, "tanh"), eh.LayerNorm(17), eh.Dense(17, 8, "relu"), eh.LayerNorm(8, "sigmoid")))
    X, ta, y = data()
    rows = np.arange(5, 305)
    theta = conditioned_theta(model, X, ta, y, rows, "mae", 31)
    eng = engine_of(model, X, ta, y, theta)
    eng.set_training_loss("mae")
    eng.set_weight_l2(0.01, False)
    loss, grad, _ = eng.loss_and_grad(first=5, count=300)
    l64, g64, _ = tw.loss_and_grad(model, theta, X, {"ta": ta}, y, rows, "mae", l2=0.01)
    assert abs(loss - l64) <= TOL * abs(l64) and util.relerr(grad, g64) <= TOL and util.elem_relerr(grad, g64, 1e-3) <= ETOL
    m = ~model.l2_mask(None, "weight")
    l0, g0, _ = tw.loss_and_grad(model, theta, X, {"ta": ta}, y, rows, "mae")
    assert np.array_equal(g64[m], g0[m]) and l64 > l0                    # the term touches the Dense weights alone
    eng.close()


def test_graph_capture_gives_the_same_bits():
    model, X, ta, y, theta = steps_case()
    eng = engine_of(model, X, ta, y, theta); eng.opt_init("Adam", 0.01)
    eng.train_step(0, 100, want_loss=False)                       # (eager: the layer-wise form sizes its buffers at the first step of a batch size)
    eng.set_params(theta); eng.opt_init("Adam", 0.01)
    ref = engine_of(model, X, ta, y, theta); ref.opt_init("Adam", 0.01)
    eng.graph_begin()
    for s_ in range(4):
        eng.train_step(s_ * 100, 100, want_loss=False)
    g = eng.graph_end()
    eng.graph_launch(g); eng.synchronize()
    for s_ in range(4):
        ref.train_step(s_ * 100, 100, want_loss=False)
    assert np.array_equal(eng.get_params(), ref.get_params()) and not np.array_equal(eng.get_params(), theta)
    eng.close(); ref.close()


def test_data_parallel_seam_two_shards_on_one_gpu():
    """eh_dp_grad of two shards, their raw partial vectors added (what the all-reduce does), eh_dp_apply: the step of the full batch.
    Nothing of a LayerNorm layer couples the samples, so the shards' sums add.  The gradient itself is checked against the fp64 twin."""
    model = make_model(eh.Chain(eh.Dense(16, 17, "tanh"), eh.LayerNorm(17), eh.Dense(17, 8, "relu"), eh.LayerNorm(8, "sigmoid")))
    X, ta, y = data()
    theta = conditioned_theta(model, X, ta, y, np.arange(400), "mse", 21)
    eng = engine_of(model, X, ta, y, theta); ref = engine_of(model, X, ta, y, theta)
    eng.opt_init("Descent", 0.05); ref.opt_init("Descent", 0.05)
    l_ref = ref.train_step(0, 400)
    ptr, n = eng.device_buffer(L.EH_BUF_GRAD)
    buf = torch.as_tensor(eh.dp._DevArray(ptr, n), device="cuda")
    acc = torch.zeros_like(buf)
    for k in range(2):
        eng.dp_grad(k * 200, 200); eng.synchronize(); acc += buf
    buf.copy_(acc); torch.cuda.synchronize()
    assert eng.dp_apply(want_loss=True) == pytest.approx(l_ref, rel=1e-5)
    # Descent: theta' = theta - lr g, so the two parameter vectors differ by lr times the difference of two fp32 gradients of the same sum
    # taken in another order: TOL of the largest entry each
    _, g64, _ = tw.loss_and_grad(model, theta, X, {"ta": ta}, y, np.arange(400))
    gmax = float(np.max(np.abs(g64)))
    assert np.max(np.abs(eng.get_params() - ref.get_params())) <= 0.05 * 2 * TOL * gmax + 2 * np.finfo(np.float32).eps * float(np.max(np.abs(theta)))
    assert util.relerr((theta - eng.get_params()) / np.float32(0.05), g64) <= 2 * TOL + 4 * np.finfo(np.float32).eps * float(np.max(np.abs(theta))) / (0.05 * gmax)
    eng.close(); ref.close()


def test_refusals_and_what_is_not_refused_on_a_live_handle():
    model, X, ta, y, theta = steps_case()
    eng = engine_of(model, X, ta, y, theta)
    for what, call in (("fused_update", lambda: eng.set_option("fused_update", 1)), ("multi_step", lambda: eng.set_option("multi_step", 1)),
                       ("specialize", lambda: eng.set_option("specialize", 1)), ("precision", lambda: eng.set_option("precision", 1))):
        with pytest.raises(NotImplementedError, match=what + ".*LayerNorm layers in the chain"):
            call()
    lib = eng._lib
    assert lib.eh_set_option(eng._h, b"fused_update", 1) == L.EH_EUNSUPPORTED and b"BatchNorm" not in lib.eh_last_error(eng._h)
    with pytest.raises(eh.EngineError, match="hidden layer 2 is no BatchNorm layer"):
        eng.get_layer_state(2)
    with pytest.raises(eh.EngineError, match="hidden layer 1 is no BatchNorm layer"):
        eng.set_layer_norm(1, epsilon=1e-4)
    with pytest.raises(ValueError, match="epsilon"):
        eng.set_layer_norm(2, epsilon=0.0)
    eng.set_option("fused_update", 2)                            # "where it is reproducible": the pair is
    eng.set_option("multi_step", 0)
    # epsilon is a kernel argument of the next launch
    before = eng.forward(L.EH_SPLIT_TRAIN, 0, 50)["reco"]
    eng.set_layer_norm(2, epsilon=0.5)
    assert not np.array_equal(eng.forward(L.EH_SPLIT_TRAIN, 0, 50)["reco"], before)
    eng.set_layer_norm(2, epsilon=1e-5)
    assert np.array_equal(eng.forward(L.EH_SPLIT_TRAIN, 0, 50)["reco"], before)
    eng.opt_init("Adam", 0.01)
    eng.train_step(0, 64)                                        # ... and the handle trains on
    assert np.isfinite(eng.get_params()).all()
    with pytest.raises(NotImplementedError, match="fused_update"):
        eh.train(tutorial_model(), cols_of(300, 1), nepochs=1, fused_update=True)
    eng.close()
