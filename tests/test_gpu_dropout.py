"""Dropout on the device: the masks of eh_dropout_mask against the NumPy Philox, loss and gradient of the step kernels against the
fp64 twin under the same masks (every kernel path: P <= 4 / K == 1 fast paths, MFMA output layer, three layers, stored z, input
BatchNorm, several tiles, several workgroups), the step count's semantics, test mode, checkpoints, and train().

Bars: loss, gradient norm and largest-entry error 1e-5, element-wise 5e-4 (those of tests/test_gpu_seq.py and test_gpu_parity.py); the
twin's own fp32 run has to reach a tenth of each, so a miss is the kernel's."""
import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho
from tests import dropout_twin as dt
from tests import util

pytestmark = pytest.mark.gpu

TOL, ETOL = 1e-5, 5e-4
SEED = 161803
COUNTS = (5, 17, 33, 300)
BIG_STEP = (1 << 32) + 3


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _rb_data(n, n_pred=2, seed=11):
    rng = np.random.default_rng(seed)
    if n_pred == 2:
        X, f, y = ho.make_synth_rbq10(n, seed, 0.1)
        return (X / np.float32(50)).astype(np.float32), f, y
    X = (rng.standard_normal((n_pred, n)) * 0.5).astype(np.float32)
    ta = (10 + 10 * rng.standard_normal(n)).astype(np.float32)
    reco = (3.0 + np.tanh(X[0] + 0.5 * X[1])) * 2.0 ** (0.1 * (ta - 15.0)) + 0.1 * rng.standard_normal(n)
    reco[rng.random(n) < 0.1] = np.nan
    return X, {"ta": ta}, {"reco": reco.astype(np.float32)}


def _case(name, n=300):
    if name in ("A", "E"):
        spec = ho.rbq10_spec((16, 16), "sigmoid" if name == "E" else "tanh", True)
        spec.input_batchnorm = name == "E"
        rates = (0.5, 0.5)
        X, f, y = _rb_data(n)
    elif name == "B":          # two NN outputs: the MFMA output layer; 20 units: padding rows in the second block
        spec = ho.HybridSpec(3, [20], "expo", dict(ho.EXPO_PARAMS), ["k", "Resp0"], [], ["Resp_obs"], "sigmoid", True)
        rates = (0.2,)
        rng = np.random.default_rng(12)
        X = rng.random((3, n)).astype(np.float32)
        T = (rng.random(n) * 40 - 10).astype(np.float32)
        r = (1.0 + X[0]) * np.exp(0.05 * T) * (1 + 0.05 * rng.standard_normal(n))
        r[rng.random(n) < 0.1] = np.nan
        f, y = {"T": T}, {"Resp_obs": r.astype(np.float32)}
    elif name == "C":          # three layers of 3, 2 and 4 blocks, one without dropout between two with it
        spec = ho.HybridSpec(8, [40, 24, 64], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "relu", False)
        rates = (0.1, 0.0, 0.5)
        X, f, y = _rb_data(n, 8)
    elif name == "D":          # Chain(Dense(16, 32, swish), Dropout(0.5), Dense(32, 8, sigmoid)) under tanh: the images hold z
        spec = ho.HybridSpec(2, [16, 32, 8], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "tanh", True,
                             layer_activations=["tanh", "swish", "sigmoid"])
        rates = (0.0, 0.5, 0.0)
        X, f, y = _rb_data(n)
    else:
        raise KeyError(name)
    theta = ho.init_theta(spec, 3, np.float32)
    return spec, rates, theta, X, f, y


def _engine(spec, rates, theta, X, f, y, seed=SEED, step=0, **opts):
    eng = util.load_engine(spec, theta, X, f, y)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_dropout(rates, seed=seed, step=step)
    return eng


def _twin(spec, rates, theta, X, f, y, count, step, dtype, seed=SEED):
    masks = dt.masks_for(seed, step, count, spec.hidden, rates)
    sc = [dt.invp(p) for p in rates]
    mm = ho.MECH[spec.mech][0]
    return dt.loss_and_grad(spec, np.asarray(theta, np.float64), X[:, :count], {k: f[k][:count] for k in mm.forcings},
                            {t: y[t][:count] for t in spec.targets}, masks, sc, dtype)


def _check(eng, spec, rates, theta, X, f, y, count, step=0, tag=""):
    l64, g64, nv64 = _twin(spec, rates, theta, X, f, y, count, step, torch.float64)
    l32, g32, _ = _twin(spec, rates, theta, X, f, y, count, step, torch.float32)
    n64 = float(np.linalg.norm(g64))
    assert abs(l32 - l64) <= 0.1 * TOL * abs(l64) and abs(float(np.linalg.norm(g32)) - n64) <= 0.1 * TOL * n64, (l32, l64)
    assert util.elem_relerr(g32, g64, 1e-3) <= 0.1 * ETOL, util.elem_relerr(g32, g64, 1e-3)
    loss, grad, nv = eng.loss_and_grad(first=0, count=count)
    gn = float(np.linalg.norm(grad.astype(np.float64)))
    print(f"dropout parity {tag} n{count} step {step}: loss rel {abs(loss - l64) / abs(l64):.2e}  norm rel {abs(gn - n64) / n64:.2e}  "
          f"max rel {util.relerr(grad, g64):.2e}  entry rel {util.elem_relerr(grad, g64, 1e-3):.2e}  n_valid {nv}")
    assert nv == nv64
    assert abs(loss - l64) <= TOL * abs(l64), (loss, l64)
    assert abs(gn - n64) <= TOL * n64
    assert util.relerr(grad, g64) <= TOL, util.relerr(grad, g64)
    assert util.elem_relerr(grad, g64, 1e-3) <= ETOL, util.elem_relerr(grad, g64, 1e-3)


# ---- masks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_device_masks_are_the_numpy_masks(name):
    spec, rates, theta, X, f, y = _case(name, 64)
    eng = _engine(spec, rates, theta, X, f, y)
    for l, (w, p) in enumerate(zip(spec.hidden, rates)):
        for step in (0, 1, BIG_STEP):
            for count in COUNTS:
                got = eng.dropout_mask(l, step, count)
                assert got.shape == (count, w)
                assert np.array_equal(got, dt.keep_mask(SEED, step, count, l, w, p)), (name, l, step, count)
    eng.close()


def test_mask_statistics():
    spec = ho.HybridSpec(2, [64, 64], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "tanh", True)
    X, f, y = _rb_data(64)
    theta = ho.init_theta(spec, 3, np.float32)
    N = 4096 * 64
    for p in (0.5, 0.2):
        eng = _engine(spec, (p, p), theta, X, f, y)
        m = [[eng.dropout_mask(l, s, 4096) for s in range(4)] for l in range(2)]
        for l in range(2):
            for s in range(4):
                z = abs(m[l][s].mean() - (1 - p)) / np.sqrt(p * (1 - p) / N)
                print(f"keep fraction p {p} layer {l} step {s}: {m[l][s].mean():.5f} ({z:.2f} sigma)")
                assert z <= 4.0
        if p == 0.5:       # masks of two steps / of two layers agree on half of the draws
            for a, b, what in ((m[0][0], m[0][1], "step 0 / 1"), (m[0][0], m[1][0], "layer 0 / 1")):
                z = abs((a == b).mean() - 0.5) / np.sqrt(0.25 / N)
                print(f"agreement {what}: {(a == b).mean():.5f} ({z:.2f} sigma)")
                assert z <= 4.0
        eng.close()


# ---- loss and gradient against the fp64 twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_loss_and_gradient_match_the_twin(name):
    spec, rates, theta, X, f, y = _case(name)
    eng = _engine(spec, rates, theta, X, f, y)
    for count in COUNTS:
        _check(eng, spec, rates, theta, X, f, y, count, tag=name)
    eng.set_dropout(rates, seed=SEED, step=BIG_STEP)          # the step count's high word reaches the counter
    _check(eng, spec, rates, theta, X, f, y, 33, BIG_STEP, tag=name)
    njit, log = eng.jit_status()
    assert njit >= 1, log                                     # the kernels compiled at run time ran: there are no others
    eng.close()


@pytest.mark.parametrize("fast", [0, 1])
def test_case_a_without_the_fast_paths(fast):
    """fast_paths 3 (P <= 4 and K == 1 on the vector ALU) is the default the cases above take; 1 = K == 1 only, 0 = the MFMA forms"""
    spec, rates, theta, X, f, y = _case("A")
    eng = _engine(spec, rates, theta, X, f, y, fast_paths=fast)
    for count in (33, 300):
        _check(eng, spec, rates, theta, X, f, y, count, tag=f"A fast {fast}")
    eng.close()


def test_case_a_as_a_recorded_closure():
    """the mechanistic model written by hand: the kernels of recorded closures (FAST = 4, generic MFMA forms around the compiled program)"""
    from tests import closures as cl
    spec, rates, theta, X, f, y = _case("A")
    model = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], cl.rbq10_closure, dict(cl.RBQ10_TABLE), ["rb"], ["Q10"],
                                    hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    eng = model.engine(0)
    eng.set_data(0, X, [f["ta"]], [y["reco"]])
    eng.set_params(theta)
    eng.set_dropout(rates, seed=SEED)
    for count in (33, 300):
        _check(eng, spec, rates, theta, X, f, y, count, tag="A closure")
    eng.close()


@pytest.mark.parametrize("bn_in_kernel", [1, 0])
def test_case_e_input_batchnorm(bn_in_kernel):
    spec, rates, theta, X, f, y = _case("E")
    eng = _engine(spec, rates, theta, X, f, y, bn_in_kernel=bn_in_kernel)
    _check(eng, spec, rates, theta, X, f, y, 300, tag=f"E bn_in_kernel {bn_in_kernel}")
    eng.close()


def test_case_f_several_tiles_per_wave():
    spec, rates, theta, X, f, y = _case("A")
    eng = _engine(spec, rates, theta, X, f, y, max_blocks=1)
    _check(eng, spec, rates, theta, X, f, y, 300, tag="F")
    eng.close()


def test_case_g_several_workgroups():
    spec, rates, theta, X, f, y = _case("A", 5000)
    eng = _engine(spec, rates, theta, X, f, y)
    _check(eng, spec, rates, theta, X, f, y, 5000, tag="G")
    eng.close()


# ---- the step count ----------------------------------------------------------------------------------------------------------------
def test_loss_and_grad_returns_the_gradient_the_next_step_applies():
    spec, rates, theta, X, f, y = _case("A")
    eng = _engine(spec, rates, theta, X, f, y)
    eng.opt_init("Descent", 0.05)
    for k in range(2):
        th0 = eng.get_params()
        _, g, _ = eng.loss_and_grad(first=0, count=300)
        assert eng.get_dropout()[2] == k                      # not advanced
        eng.train_step(0, 300, want_loss=False)
        assert eng.get_dropout()[2] == k + 1
        # one fp32 multiply and subtract (fused or not) on the same gradient bits: an ulp of the largest parameter; another mask moves it by ~1e-2
        assert np.abs(eng.get_params() - (th0 - np.float32(0.05) * g)).max() <= 2.4e-7 * max(1.0, float(np.abs(th0).max()))
    eng.close()


@pytest.mark.parametrize("rule", ["Descent", "Adam"])
def test_three_steps_follow_the_twin_with_the_masks_of_steps_0_1_2(rule):
    spec, rates, theta, X, f, y = _case("A")
    eng = _engine(spec, rates, theta, X, f, y)
    lr = 0.05 if rule == "Descent" else 0.01
    eng.opt_init(rule, lr)
    th, st = theta.astype(np.float32).copy(), ho.adam_init(theta.size, np.float32)
    for step in range(3):
        eng.train_step(0, 300, want_loss=False)
        _, g, _ = _twin(spec, rates, th, X, f, y, 300, step, torch.float64)
        if rule == "Descent":
            th = (th - np.float32(lr) * g.astype(np.float32)).astype(np.float32)
        else:
            th = ho.adam_step(th, g.astype(np.float32), st, lr=lr)
    err = float(np.abs(eng.get_params() - th).max())
    print(f"three {rule} steps: max |theta - twin| {err:.2e}")
    assert err <= 1e-5 * max(1.0, float(np.abs(th).max()))
    assert eng.get_dropout()[2] == 3
    eng.close()


def test_an_all_nan_minibatch_changes_nothing_but_advances_the_count():
    spec, rates, theta, X, f, y = _case("A")
    y = {"reco": y["reco"].copy()}
    y["reco"][100:164] = np.nan
    for fused in (0, 1):
        eng = _engine(spec, rates, theta, X, f, y, fused_update=fused)
        eng.opt_init("Adam", 0.01)
        eng.train_step(0, 64, want_loss=False)
        eng.synchronize()
        th1, o1 = eng.get_params(), eng.get_opt_state()
        eng.train_step(100, 64, want_loss=False)
        th2, o2 = eng.get_params(), eng.get_opt_state()
        assert np.array_equal(th1.view(np.uint32), th2.view(np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(o1, o2))
        assert eng.get_dropout()[2] == 2
        eng.close()


def test_fused_update_follows_the_pair():
    spec, rates, theta, X, f, y = _case("A")
    a = _engine(spec, rates, theta, X, f, y); a.opt_init("Adam", 0.01)
    b = _engine(spec, rates, theta, X, f, y, fused_update=1); b.opt_init("Adam", 0.01)
    c = _engine(spec, rates, theta, X, f, y, fused_update=2); c.opt_init("Adam", 0.01)
    la, na = a.train_epoch(64, shuffle=False)
    lb, nb = b.train_epoch(64, shuffle=False)
    lc, nc = c.train_epoch(64, shuffle=False)
    assert na == nb == nc == 5 and lb == pytest.approx(la, rel=1e-5) and lc == pytest.approx(la, rel=1e-5)
    # (float atomics: the bar of tests/test_gpu_parity.py::test_fused_update_mode_matches_two_kernel_mode)
    assert np.max(np.abs(a.get_params() - b.get_params())) <= 2e-5
    assert np.max(np.abs(a.get_params() - c.get_params())) <= 2e-5
    assert a.get_dropout()[2] == b.get_dropout()[2] == c.get_dropout()[2] == 5
    for e in (a, b, c):
        e.close()


# ---- test mode, Dropout(0), checkpoints --------------------------------------------------------------------------------------------
def test_forward_and_eval_run_in_test_mode():
    spec, rates, theta, X, f, y = _case("A")
    eng = _engine(spec, rates, theta, X, f, y)
    out = eng.forward(0)
    ref = ho.forward(spec, theta.astype(np.float64), X, f, train_mode=False)
    assert util.relerr(out["reco"], ref["reco"]) <= 1e-5
    metrics, _ = eng.eval(0)
    m = ~np.isnan(y["reco"])
    mse = float(np.mean((ref["reco"][m] - y["reco"][m].astype(np.float64)) ** 2))
    assert metrics[0]["mse"] == pytest.approx(mse, rel=1e-5) and metrics[0]["n"] == int(m.sum())
    eng.close()


def _chain_model(*layers):
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                   hidden_layers=eh.Chain(*layers), activation="tanh", scale_nn_outputs=True)


def test_dropout_zero_is_the_chain_without_it():
    spec, rates, theta, X, f, y = _case("A")
    got = []
    for model in (_chain_model(eh.Dense(16, 16, "tanh"), eh.Dropout(0)), _chain_model(eh.Dense(16, 16, "tanh"))):
        eng = model.engine(0)
        eng.set_data(0, X, [f["ta"]], [y["reco"]])
        eng.set_params(theta)
        got.append(eng.loss_and_grad())
        eng.close()
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))


def test_a_model_with_dropout_layers_sets_the_engine_up():
    spec, rates, theta, X, f, y = _case("A")
    model = _chain_model(eh.Dropout(0.5), eh.Dense(16, 16, "tanh"), eh.Dropout(0.5))
    eng = model.engine(0)
    r, seed, step = eng.get_dropout()
    assert list(r) == [0.5, 0.5] and (seed, step) == (0, 0)
    eng.set_option("aot_spec", 0)
    eng.set_data(0, X, [f["ta"]], [y["reco"]])
    eng.set_params(theta)
    eng.set_dropout(r, seed=SEED, step=0)
    _check(eng, spec, rates, theta, X, f, y, 33, tag="front door engine")
    eng.close()


def test_a_checkpoint_resumes_the_mask_stream():
    spec, rates, theta, X, f, y = _case("A")
    def steps(eng, k0, k1):
        for k in range(k0, k1):
            eng.train_step(64 * k, 64, want_loss=False)
    full = _engine(spec, rates, theta, X, f, y); full.opt_init("Adam", 0.01)
    steps(full, 0, 4)
    first = _engine(spec, rates, theta, X, f, y); first.opt_init("Adam", 0.01)
    steps(first, 0, 2)
    r, seed, step = first.get_dropout()
    assert step == 2 and seed == SEED
    th, (m, v, bt) = first.get_params(), first.get_opt_state()
    out = []
    for _ in range(2):
        e = util.load_engine(spec, th, X, f, y); e.opt_init("Adam", 0.01)
        e.set_opt_state(m, v, bt)
        e.set_dropout(r, seed=seed, step=step)
        steps(e, 2, 4)
        out.append(e.get_params())
        e.close()
    ref = full.get_params()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)) and np.array_equal(out[0].view(np.uint32), ref.view(np.uint32))
    full.close(); first.close()


# ---- the front door ----------------------------------------------------------------------------------------------------------------
def test_train_is_reproducible_and_learns():
    from easyhybrid_jl_amd.synthetic import make_synth_rbq10
    data = make_synth_rbq10(2048, 7, 0.05)
    data["sw_pot"] = (data["sw_pot"] / np.float32(50)).astype(np.float32)
    data["dsw_pot"] = (data["dsw_pot"] / np.float32(50)).astype(np.float32)
    model = _chain_model(eh.Dense(16, 16, "tanh"), eh.Dropout(0.2))
    assert model.dropout == pytest.approx([0.0, 0.2])
    kw = dict(nepochs=4, batchsize=128, opt=eh.Adam(0.01), loss_types=["mse"], patience=100)
    a = eh.train(model, data, random_seed=5, **kw)
    b = eh.train(model, data, random_seed=5, **kw)
    c = eh.train(model, data, random_seed=6, **kw)
    assert np.array_equal(a.ps.view(np.uint32), b.ps.view(np.uint32))
    assert not np.array_equal(a.ps, c.ps)
    assert (a.dropout_seed, b.dropout_seed, c.dropout_seed) == (5, 5, 6) and a.dropout_step == b.dropout_step > 0
    val = [h["mse"]["reco"] for h in a.val_history]
    print("validation mse by epoch:", val)
    assert len(val) == 5 and np.all(np.isfinite(val)) and val[-1] < val[0]
    d = eh.train(model, data, random_seed=5, train_from=a, **kw)      # continues the step count: no mask of the first run comes back
    assert d.dropout_step == 2 * a.dropout_step
    e = eh.train(model, data, random_seed=6, train_from=a, **kw)      # another seed is another stream: from step 0
    assert (e.dropout_seed, e.dropout_step) == (6, a.dropout_step)
    for r in (a, b, c, d, e):
        r.release()
    with pytest.raises(NotImplementedError, match="Dropout layers are not built for data parallelism"):
        eh.train(model, data, random_seed=5, distributed=True, **kw)


def test_refusals_on_a_live_handle():
    spec, rates, theta, X, f, y = _case("A")
    eng = util.load_engine(spec, theta, X, f, y)
    for bad in ([0.5, 1.0], [-0.1, 0.5], [float("nan"), 0.0], [0.5]):
        with pytest.raises(ValueError, match="eh_set_dropout"):
            eng.set_dropout(bad)
    eng.set_dropout(rates, seed=SEED)
    eng.opt_init("Adam", 0.01)
    with pytest.raises(NotImplementedError, match="dropout"):
        eng._chk(eng._lib.eh_graph_begin(eng._h))
    for opt in ("precision", "row_split"):
        with pytest.raises(NotImplementedError, match="dropout"):
            eng.set_option(opt, 1)
    with pytest.raises(NotImplementedError, match="dropout"):
        eng._chk(eng._lib.eh_dp_grad(eng._h, 0, 64))
    with pytest.raises(NotImplementedError, match="dropout"):
        eng._chk(eng._lib.eh_dp_fused_step(eng._h, 0, 64, __import__("ctypes").byref(__import__("ctypes").c_int32())))
    eng.set_dropout([0.0, 0.0])                               # all zero removes it: the handle is an ordinary one again
    assert not eng.get_dropout()[0].any()
    l0, g0, _ = eng.loss_and_grad()
    plain = util.load_engine(spec, theta, X, f, y)
    l1, g1, _ = plain.loss_and_grad()
    assert l0 == l1 and np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    plain.close(); eng.close()
    # the kernel families without dropout
    wide = ho.HybridSpec(2, [128, 128], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "tanh", True)
    e = util.load_engine(wide, ho.init_theta(wide, 1, np.float32), X, f, y)
    with pytest.raises(NotImplementedError, match="row-split"):
        e.set_dropout([0.5, 0.5])
    e.close()
    deep = ho.HybridSpec(2, [16, 16, 16, 16], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "tanh", True)
    e = util.load_engine(deep, ho.init_theta(deep, 1, np.float32), X, f, y)
    with pytest.raises(NotImplementedError, match="layer-wise"):
        e.set_dropout([0.5, 0.5, 0.0, 0.0])
    e.close()
    # a bf16 handle (precision set before the rates): a row-split family too, the reason names the precision
    c5 = ho.c5_spec(precision="bf16")
    X5, f5, y5 = ho.make_synth_c5(64)
    e = util.load_engine(c5, ho.init_theta(c5, 1, np.float32), X5, f5, y5)
    with pytest.raises(NotImplementedError, match="bf16"):
        e.set_dropout([0.5, 0.5])
    e.close()
    # a sequence model
    seq = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                  hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(8, 8))), activation="tanh", scale_nn_outputs=True)
    e = seq.engine(0)
    with pytest.raises(NotImplementedError, match="sequence models"):
        e.set_dropout([0.5, 0.0, 0.5])
    e.close()
    # the peer-to-peer exchange, both ways round: not on a handle with dropout, no dropout on a handle set up for it
    e = _engine(spec, rates, theta, X, f, y, fused_update=1)
    with pytest.raises(NotImplementedError, match="eh_p2p_init: dropout"):
        e.p2p_init(1, 0)
    e.close()
    e = util.load_engine(spec, theta, X, f, y)
    e.opt_init("Adam", 0.01); e.set_option("fused_update", 1)
    e.p2p_init(1, 0)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        e.set_dropout(rates)
    e.close()
    multi = ho.HybridSpec(2, [1], "rbq10", dict(ho.RBQ10_PARAMS), ["rb", "Q10"], [], ["reco"], "tanh", True, nets=[([0], [8]), ([1], [8])])
    e = util.load_engine(multi, ho.init_theta(multi, 1, np.float32), X, f, y)
    with pytest.raises(NotImplementedError, match="MultiNN"):
        e.set_dropout([0.5])
    e.close()
