"""Recorded activations on the device: the generated functions element by element (eh_activation_apply), every model case against the
oracle, the recorded twins of two built-ins against the built-in per-layer kernel, the one-kernel steps and the epoch driver, the
disk cache, the all-reduce seam, and the refusals.  The oracle serves the case closures by name (tests/act_cases.py)."""
import functools
import os

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
from oracle import hybrid_oracle as ho

from tests import act_cases as ac
from tests import util

pytestmark = pytest.mark.gpu
TOL = 1e-5


# ---- 1. the generated device functions, element by element -------------------------------------------------------------------------------
def _grid():
    return np.concatenate([np.linspace(-8.0, 8.0, 4096), [0.0, 1e-30, -1e-30]]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _apply_all():
    """every case's (value, derivative) from the device on the grid, once per session; two handles (eight programs each); also the built-in
    tanh / sigmoid through the same kernel, and every case's error against its fp64 closure and hand derivative (norm-wise)"""
    z, out = _grid(), {}
    names = list(ac.ACT_CASES)
    for batch in (names[:8], names[8:]):
        # a model that names every program of the batch: one net per program (MultiNN, one hidden layer each)
        preds = {f"p{k}": ["a"] for k in range(len(batch))}
        fn = lambda **p: {"y": sum(p.values())}
        tab = {f"p{k}": (1.0, 0.0, 5.0) for k in range(len(batch))}
        m = eh.constructHybridModel(preds, [], ["y"], fn, tab, [], hidden_layers={k: [4] for k in preds},
                                    activation={f"p{k}": ac.ACT_CASES[n][0] for k, n in enumerate(batch)}, scale_nn_outputs=True)
        assert len(m.act_programs()) == len(batch)
        eng = m.engine()
        for j, n in enumerate(batch):
            out[n] = eng.activation_apply(j, z)
        out.setdefault("tanh", eng.activation_apply(-1 - L.ACTIVATIONS["tanh"], z))
        out.setdefault("sigmoid", eng.activation_apply(-1 - L.ACTIVATIONS["sigmoid"], z))
        eng.close()
    z64 = z.astype(np.float64)
    err = {n: (util.relerr(out[n][0], ac.ACT_CASES[n][0](z64)), util.relerr(out[n][1], ac.ACT_CASES[n][1](z64))) for n in ac.ACT_CASES}
    return out, err


def test_recorded_twins_equal_the_builtin_activations_bit_for_bit():
    out, _ = _apply_all()
    assert np.array_equal(out["tanh_twin"][0], out["tanh"][0]) and np.array_equal(out["tanh_twin"][1], out["tanh"][1])
    assert np.array_equal(out["sigmoid_twin"][0], out["sigmoid"][0]) and np.array_equal(out["sigmoid_twin"][1], out["sigmoid"][1])


@pytest.mark.parametrize("name", list(ac.ACT_CASES))
def test_generated_functions_element_by_element(name):
    """A case against its fp64 closure and hand derivative on 4 096 values in [-8, 8] plus 0 and +-1e-30.  The bar is what the device's own
    tanh / sigmoid achieve: four times the larger of the two recorded twins' errors against fp64 on the same values (norm-wise).

    Measured on an MI355X (value, derivative): square 3.0e-8, 0; softplus 3.6e-8, 8.6e-8; elu 7.7e-9, 4.3e-8; leakyrelu 6.7e-10, 2.2e-10;
    gelu_tanh 6.2e-8, 2.0e-7; hard_sigmoid 3.6e-8, 1.5e-8; xsin 6.9e-8, 7.9e-8; tanh_twin 2.24e-7, 4.48e-7; sigmoid_twin 1.02e-7, 3.86e-7;
    leakyrelu02 8.9e-9, 3.0e-9.  Bar: 4 x 4.48e-7 = 1.79e-6.  (gelu_tanh written with tanh itself, 0.5 x (1 + tanh u), gave 2.49e-6 for the
    derivative: the reverse sweep's 1 - t^2 cancels, and gelu's chain rule multiplies that term by up to 5; eh.gelu_tanh is NNlib's form
    x sigmoid(2 u) with the exponential written out, which has no such term.)"""
    _, err = _apply_all()
    bar = 4.0 * max(max(err["tanh_twin"]), max(err["sigmoid_twin"]))
    print(f"{name}: value {err[name][0]:.3e}, derivative {err[name][1]:.3e}; bar = 4 x max(twins) = {bar:.3e}")
    assert max(err[name]) <= bar, (name, err[name], bar)


# ---- 2. the model cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B", ac.MODEL_RUNS)
def test_model_case_against_the_oracle(case, B, monkeypatch):
    ac.patch_oracle(monkeypatch)
    r = ac.reference(case, B)
    spec, X, f, y, theta = r["spec"], r["X"], r["f"], r["y"], r["theta"]
    eng = ac.load_engine(spec, theta, X, f, y)
    loss, grad, nv = eng.loss_and_grad()
    njit, jlog = eng.jit_status()
    assert njit >= 1, jlog
    print(f"{case} B={B}: loss {abs(loss - r['l64']) / abs(r['l64']):.2e}, gradient {util.relerr(grad, r['g64']):.2e}")
    assert nv == r["nv"] and loss == pytest.approx(r["l64"], rel=TOL) and util.relerr(grad, r["g64"]) <= TOL
    util.check_gradient(grad, r["g64"], ac.layout_spec(spec), TOL, util.ref32_orders(spec, theta.astype(np.float64), X, f, y))
    out = eng.forward(0)
    assert util.relerr(out["reco"], r["fwd"]["reco"]) <= TOL and util.relerr(out["parameters"]["rb"], r["fwd"]["parameters"]["rb"]) <= TOL
    m, _ = eng.eval(0)
    assert m[0]["mse"] == pytest.approx(r["mse"], rel=3e-5)
    eng.opt_init("Adam", 0.01)
    losses = [eng.train_step(*b) for b in r["batches"]]
    dt = float(np.max(np.abs(eng.get_params() - r["t32"])))
    print(f"{case} B={B}: trajectory {dt / max(1.0, float(np.max(np.abs(r['t32'])))):.2e}")
    assert np.allclose(losses, r["losses32"], rtol=1e-4)
    assert dt <= 3e-5 * max(1.0, float(np.max(np.abs(r["t32"]))))
    eng.close()


# ---- 3. the recorded twins against the built-in per-layer kernel -------------------------------------------------------------------------------
def test_recorded_twins_against_the_builtin_per_layer_kernel():
    spec = ho.HybridSpec(3, [16, 16], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "tanh", True, layer_activations=["tanh", "sigmoid"])
    twin = ho.HybridSpec(3, [16, 16], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "tanh_twin", True, layer_activations=["tanh_twin", "sigmoid_twin"])
    X, f, y, theta = ac.make_data(spec, 1300)
    a, b = util.load_engine(spec, theta, X, f, y), ac.load_engine(twin, theta, X, f, y)
    assert len(ac.model_from_spec(twin).act_programs()) == 2
    la, ga, na = a.loss_and_grad()
    lb, gb, nb = b.loss_and_grad()
    print(f"twins against built-in: loss {abs(la - lb) / abs(la):.2e}, gradient {util.relerr(gb, ga):.2e}")
    assert na == nb and lb == pytest.approx(la, rel=2e-6) and util.relerr(gb, ga) <= 4e-6
    a.close(); b.close()


# ---- 4. the one-kernel steps, the epoch driver, the front door ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 2])
def test_fused_update_steps(fused, monkeypatch):
    ac.patch_oracle(monkeypatch)
    r = ac.reference("16x16_softplus_elu", 300)
    eng = ac.load_engine(r["spec"], r["theta"], r["X"], r["f"], r["y"])
    eng.opt_init("Adam", 0.01)
    eng.set_option("fused_update", fused)
    for b in r["batches"]:
        eng.train_step(*b, want_loss=False)
    eng.synchronize()
    assert eng.jit_status()[0] >= 1
    assert np.max(np.abs(eng.get_params() - r["t32"])) <= 3e-5 * max(1.0, float(np.max(np.abs(r["t32"]))))
    eng.close()


def test_epoch_driver_and_front_door(monkeypatch):
    ac.patch_oracle(monkeypatch)
    r = ac.reference("16x16_softplus_elu", 300)
    spec, X, f, y = r["spec"], r["X"], r["f"], r["y"]
    eng = ac.load_engine(spec, r["theta"], X, f, y)
    eng.opt_init("Adam", 0.01)
    la, na = eng.train_epoch(60, shuffle=False)
    th_ep, l_ep = ho.train_steps(spec, r["theta"], X, f, y, [(i * 60, 60) for i in range(5)], dtype=np.float32)
    assert na == 5 and la == pytest.approx(float(np.mean(l_ep)), rel=1e-4)
    assert np.max(np.abs(eng.get_params() - th_ep)) <= 3e-5 * max(1.0, float(np.max(np.abs(th_ep))))
    eng.close()
    Xb, fb, yb, _ = ac.make_data(spec, 2048)
    cols = {"x0": Xb[0], "x1": Xb[1], "x2": Xb[2], "ta": fb["ta"], "reco": yb["reco"]}
    model = eh.constructHybridModel(["x0", "x1", "x2"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], hidden_layers=[16, 16],
                                    activation=eh.softplus, scale_nn_outputs=True)
    o1 = eh.train(model, cols, nepochs=4, batchsize=256, random_seed=2)
    o2 = eh.train(model, cols, nepochs=4, batchsize=256, random_seed=2)
    assert np.array_equal(np.asarray(o1.ps), np.asarray(o2.ps))
    assert [h["mse"]["sum"] for h in o1.val_history] == [h["mse"]["sum"] for h in o2.val_history]
    assert len(o1.val_history) == 5 and o1.val_history[-1]["mse"]["sum"] < o1.val_history[0]["mse"]["sum"]
    assert isinstance(o1.model.activation if hasattr(o1, "model") else model.activation, eh.RecordedActivation)


# ---- 5. constants are part of the kernel, and of the cache key -----------------------------------------------------------------------------------
def test_two_slopes_and_the_disk_cache(monkeypatch, tmp_path):
    ac.patch_oracle(monkeypatch)
    monkeypatch.setenv("EH_JIT_CACHE", str(tmp_path))
    specs = {n: ho.HybridSpec(3, [16, 16], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], n, True) for n in ("leakyrelu", "leakyrelu02")}
    X, f, y, theta = ac.make_data(specs["leakyrelu"], 300)
    ref = {n: ho.loss_and_grad(s, theta.astype(np.float64), X, f, y) for n, s in specs.items()}
    assert util.relerr(ref["leakyrelu"][1], ref["leakyrelu02"][1]) > 1e-2
    grads = {}
    for order in (("leakyrelu", "leakyrelu02"), ("leakyrelu02", "leakyrelu")):      # (the second round finds both kernels in the cache)
        for n in order:
            eng = ac.load_engine(specs[n], theta, X, f, y)
            loss, grad, _ = eng.loss_and_grad()
            assert eng.jit_status()[0] >= 1
            eng.close()
            assert loss == pytest.approx(ref[n][0], rel=TOL) and util.relerr(grad, ref[n][1]) <= TOL, (order, n)
            assert n not in grads or np.array_equal(grads[n], grad)
            grads[n] = grad
    assert any(p.endswith(".eco") for p in os.listdir(tmp_path))
    assert util.relerr(grads["leakyrelu"], grads["leakyrelu02"]) > 1e-2


# ---- 6. the all-reduce seam -----------------------------------------------------------------------------------------------------------------------
def test_dp_seam_with_two_virtual_shards(monkeypatch):
    import torch
    ac.patch_oracle(monkeypatch)
    r = ac.reference("16x16_softplus_elu", 300)
    spec, X, f, y, theta = r["spec"], r["X"], r["f"], r["y"], r["theta"]
    ref = ac.load_engine(spec, theta, X, f, y); ref.opt_init("Adam", 0.01)
    l_ref = ref.train_step(0, 300)
    eng = ac.load_engine(spec, theta, X, f, y); eng.opt_init("Adam", 0.01)
    ptr, n = eng.device_buffer(L.EH_BUF_GRAD)
    buf = torch.as_tensor(eh.dp._DevArray(ptr, n), device="cuda")
    acc = torch.zeros_like(buf)
    for k in range(2):
        eng.dp_grad(k * 150, 150); eng.synchronize(); acc += buf
    buf.copy_(acc); torch.cuda.synchronize()
    assert eng.dp_apply(want_loss=True) == pytest.approx(l_ref, rel=1e-5)
    assert np.max(np.abs(eng.get_params() - ref.get_params())) <= 2e-6
    th_ref, _ = ho.train_steps(spec, theta, X, f, y, [(0, 300)], dtype=np.float32)
    assert np.max(np.abs(eng.get_params() - th_ref)) <= 2e-5
    ref.close(); eng.close()


# ---- 7. the refusals, on a live device ----------------------------------------------------------------------------------------------------------------
def _single(hidden, activation, **kw):
    return eh.constructHybridModel(["a", "b", "c"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], hidden_layers=hidden,
                                   activation=activation, scale_nn_outputs=True, **kw)


def test_refusals_on_a_live_device():
    sq = lambda x: x ** 2
    eng = _single([16, 16], sq).engine()           # (a live handle with recorded activations next to every refusal)
    with pytest.raises(NotImplementedError, match="layer-wise form"):
        _single([200, 64, 32], sq)
    with pytest.raises(NotImplementedError, match="layer-wise form"):
        _single([16, 16, 16, 16], sq)
    with pytest.raises(NotImplementedError, match="Recurrence"):
        _single(eh.Chain(eh.Recurrence(eh.LSTMCell(8, 8))), sq)
    with pytest.raises(NotImplementedError, match="precision = 'bf16_fwd'"):
        _single([96, 96], sq, precision="bf16_fwd")
    with pytest.raises(NotImplementedError, match="Dropout next to a recorded activation"):
        _single(eh.Chain(eh.Dense(16, 16, sq), eh.Dropout(0.5)), "tanh")
    X, f, y, _ = ac.make_data(ac.make_spec("24_square"), 256)
    cols = {"a": X[0], "b": X[1], "c": X[2], "ta": f["ta"], "reco": y["reco"]}
    with pytest.raises(NotImplementedError, match="kernels compiled at run time, which a group of models does not use"):
        eh.train_members(_single([16, 16], sq), cols, [{"random_seed": 1}, {"random_seed": 2}], nepochs=1, batchsize=64)
    # ... and the library's own answers on the handle
    with pytest.raises(Exception, match="recorded activations"):
        eng.set_dropout([0.5, 0.0])
    with pytest.raises(Exception, match="not per-net activations"):
        eng.set_option("precision", 1)
    eng.close()
    # the descriptors the Python surface refuses, handed to the library directly
    m = _single([16, 16], sq)
    d, progs = m.to_desc(), m.act_program_structs()
    d.n_hidden = 3; d.hidden[0], d.hidden[1], d.hidden[2] = 200, 64, 32; d.net_activation[2] = 0
    import ctypes as C
    h = C.c_void_p()
    assert L.lib().eh_create_activations(C.byref(d), progs, 1, C.byref(h)) == L.EH_EUNSUPPORTED and not h.value
    assert "not for the layer-wise form" in L.lib().eh_last_error(None).decode()
