"""-m gpu: user closures as device programs (EH_MECH_PROGRAM) through the C ABI against the oracle, which runs the closure
itself on NumPy arrays and differentiates the recorded tape (oracle/hybrid_oracle.py `program_mech`).  Tolerance 1e-5."""
import os

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho
from tests import closures as cl
from tests import util

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _spec(name, fn, table, forc, targets, neural, glob, hidden, n_pred=3, act="tanh", scale=True):
    util.register_closure(name, fn, list(table), forc, targets)
    return ho.HybridSpec(n_pred, list(hidden), name, dict(table), list(neural), list(glob), list(targets), act, scale)


def _data(spec, forc_ranges, B, seed, nan_frac=0.1, noise=0.05):
    """Predictors U(-1,1); forcings in their ranges; targets = the model at a perturbed theta + noise, NaN-masked."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (spec.n_pred, B)).astype(np.float32)
    f = {k: rng.uniform(lo, hi, B).astype(np.float32) for k, (lo, hi) in forc_ranges.items()}
    theta = ho.init_theta(spec, seed + 1, np.float32)
    truth = ho.forward(spec, ho.init_theta(spec, seed + 2, np.float32).astype(np.float64), X, f)
    y = {}
    for t in spec.targets:
        v = truth[t] * (1.0 + noise * rng.normal(size=B))
        v[rng.uniform(size=B) < nan_frac] = np.nan
        y[t] = v.astype(np.float32)
    return theta, X, f, y


def _check(spec, theta, X, f, y, jit=1, **kw):
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_option("jit", jit)
    loss, grad, nv = eng.loss_and_grad(**kw)
    assert eng.jit_status()[0] == jit, eng.jit_status()[1]       # the run-time compiled kernels really ran (or really did not)
    if "first" in kw:
        sl = slice(kw["first"], kw["first"] + kw["count"])
        X, f, y = X[:, sl], {k: v[sl] for k, v in f.items()}, {k: v[sl] for k, v in y.items()}
    l0, g0, nv0 = ho.loss_and_grad(spec, np.asarray(theta, np.float64), X, f, y)
    assert nv == sum(nv0)
    assert abs(loss - l0) <= TOL * abs(l0)
    assert util.relerr(grad, g0) <= TOL
    util.check_gradient(grad, g0, spec, TOL, util.ref32_orders(spec, np.asarray(theta, np.float64), X, f, y))
    return eng


@pytest.mark.parametrize("jit", [1, 0])
@pytest.mark.parametrize("hidden", [(16, 16), (64, 64), (128, 128), (24,), (32, 16, 8)])
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_hand_written_rbq10_closure_equals_registry_model(hidden, act, jit):
    spec, theta, X, f, y = util.rbq10_case(700, act, True, 0.1, hidden=hidden)
    util.register_closure("rbq10_closure", cl.rbq10_closure, list(cl.RBQ10_TABLE), ["ta"], ["reco"])
    spec_c = ho.HybridSpec(spec.n_pred, list(spec.hidden), "rbq10_closure", dict(spec.parameters), list(spec.neural), list(spec.glob),
                           ["reco"], act, True)
    eng_c = util.load_engine(spec_c, theta, X, f, y)
    eng_c.set_option("jit", jit)
    eng_r = util.load_engine(spec, theta, X, f, y)
    lc, gc, nc = eng_c.loss_and_grad()
    assert eng_c.jit_status()[0] == jit and eng_r.jit_status()[0] == 0
    lr, gr, nr = eng_r.loss_and_grad()
    l0, g0, _ = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y)
    assert nc == nr and abs(lc - l0) <= TOL * abs(l0) and util.relerr(gc, g0) <= TOL
    util.check_gradient(gc, g0, spec, TOL, util.ref32_orders(spec, theta.astype(np.float64), X, f, y))
    assert abs(lc - lr) <= 2e-6 * abs(lr) and util.relerr(gc, gr) <= 4e-6        # the two device paths against each other
    eng_c.close(); eng_r.close()


@pytest.mark.parametrize("jit", [1, 0])
@pytest.mark.parametrize("targets", [["nee", "gpp", "reco"], ["nee"], ["gpp", "nee"]])
@pytest.mark.parametrize("hidden", [(32, 32), (128,)])
def test_three_output_flux_closure(targets, hidden, jit):
    spec = _spec("flux_closure", cl.flux_closure, cl.FLUX_TABLE, ["sw", "ta", "vpd"], targets, ["alpha", "rref", "gmax"], ["e0", "k"], hidden, n_pred=5)
    mm = ho.MECH["flux_closure"][0]
    theta, X, f, y = _data(spec, {k: r for k, r in dict(sw=(0, 800), ta=(-5, 30), vpd=(0, 30)).items() if k in mm.forcings}, 1300, 3)
    eng = _check(spec, theta, X, f, y, jit=jit)
    _check(spec, theta, X, f, y, jit=jit, first=130, count=1001).close()
    out = eng.forward(0)
    ref = ho.forward(spec, theta.astype(np.float64), X, f)
    for t in targets:
        assert util.relerr(out[t], ref[t]) <= TOL
    for p in ("alpha", "rref", "gmax", "e0", "k"):
        assert util.relerr(out["parameters"][p], np.broadcast_to(ref["parameters"][p], (1300,))) <= TOL
    eng.close()


@pytest.mark.parametrize("jit", [1, 0])
@pytest.mark.parametrize("neural,glob,scale", [(["a", "b", "c", "d"], [], True), (["a"], ["b", "c"], True), (["b", "d"], ["a"], False)])
def test_every_operation_closure(neural, glob, scale, jit):
    spec = _spec("allops_closure", cl.allops_closure, cl.ALLOPS_TABLE, ["u", "v"], ["y", "z"], neural, glob, (24, 24), n_pred=4, act="swish", scale=scale)
    theta, X, f, y = _data(spec, dict(u=(-1, 1), v=(-1, 1)), 900, 11)
    if not scale:                       # unscaled network outputs: keep c + 1.5 > 0 etc. by shrinking the last layer
        theta = theta.copy(); theta[:spec.n_nn] *= 0.3
    _check(spec, theta, X, f, y, jit=jit).close()


def test_closure_training_trajectory_eval_and_epoch_driver():
    for fused, targets, jit in ((0, ["nee", "reco"], 1), (1, ["nee"], 1), (1, ["nee"], 0)):            # (the one-kernel-per-step mode is single-target)
        spec = _spec("flux_closure", cl.flux_closure, cl.FLUX_TABLE, ["sw", "ta", "vpd"], targets, ["alpha", "rref"], ["gmax", "e0", "k"], (16, 16), n_pred=2)
        theta, X, f, y = _data(spec, dict(sw=(0, 800), ta=(-5, 30), vpd=(0, 30)), 2048, 21)
        eng = util.load_engine(spec, theta, X, f, y)
        eng.opt_init("Adam", 0.01)
        eng.set_option("fused_update", fused)
        eng.set_option("jit", jit)
        batches = [(i * 256, 256) for i in range(8)]
        losses = [eng.train_step(a, b) for a, b in batches]
        th_ref, l_ref = ho.train_steps(spec, theta, X, f, y, batches, dtype=np.float32)
        assert np.allclose(losses, l_ref, rtol=1e-4)
        assert np.max(np.abs(eng.get_params() - th_ref)) <= 3e-5 * max(1.0, float(np.max(np.abs(th_ref))))
        eng.close()
    spec = _spec("flux_closure", cl.flux_closure, cl.FLUX_TABLE, ["sw", "ta", "vpd"], ["nee", "reco"], ["alpha", "rref"], ["gmax", "e0", "k"], (16, 16), n_pred=2)
    theta, X, f, y = _data(spec, dict(sw=(0, 800), ta=(-5, 30), vpd=(0, 30)), 2048, 21)
    eng = util.load_engine(spec, theta, X, f, y, split=1)
    metrics, pred = eng.eval(1, predictions=True)
    ref = ho.forward(spec, theta.astype(np.float64), X, f)
    for t, name in enumerate(spec.targets):
        yy = y[name].astype(np.float64); mask = ~np.isnan(yy)
        assert metrics[t]["n"] == mask.sum()
        for k in ("mse", "r2", "pearson", "kge"):
            assert metrics[t][k] == pytest.approx(ho.loss_fn(ref[name], yy, mask, k), rel=2e-5, abs=2e-6), (name, k)
        assert util.relerr(pred[name], ref[name]) <= TOL
    eng.close()


@pytest.mark.parametrize("kind", ["mae", "nseLoss", "kgeLoss"])
def test_closure_with_other_training_losses(kind):
    spec = _spec("rbq10_closure", cl.rbq10_closure, cl.RBQ10_TABLE, ["ta"], ["reco"], ["rb"], ["Q10"], (16, 16), n_pred=2)
    _, theta, X, f, y = util.rbq10_case(1500, "tanh", True, 0.1)
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_training_loss(kind)
    loss, grad, nv = eng.loss_and_grad()
    l0, g0, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y, kind=kind)
    tol = 1e-4 if kind == "kgeLoss" else TOL
    assert nv == sum(nv0) and loss == pytest.approx(l0, rel=tol) and util.relerr(grad, g0) <= tol
    util.check_gradient(grad, g0, spec, tol, util.ref32_orders(spec, theta.astype(np.float64), X, f, y, kind=kind))
    eng.close()


def test_front_door_train_with_a_closure():
    cols = eh.synthetic.make_synth_rbq10(8192, 42)
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], cl.rbq10_closure, dict(cl.RBQ10_TABLE), ["rb"], ["Q10"],
                                    hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    out = eh.train(model, cols, nepochs=8, batchsize=512, opt=eh.Adam(0.01), random_seed=3)
    reg = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(cl.RBQ10_TABLE), ["rb"], ["Q10"],
                                  hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    ref = eh.train(reg, cols, nepochs=8, batchsize=512, opt=eh.Adam(0.01), random_seed=3)
    h, hr = out.train_history, ref.train_history
    assert h[-1]["mse"]["sum"] < 0.5 * h[0]["mse"]["sum"]
    assert h[-1]["mse"]["sum"] == pytest.approx(hr[-1]["mse"]["sum"], rel=2e-3)        # same model, two device paths, 128 Adam steps apart


# ----------------------------------------------------------------------------------------------
# seeded random closures: random expression DAGs over the whole operation set
# ----------------------------------------------------------------------------------------------
def _random_closure(rng, params, forcings, n_ops, n_out):
    """A NumPy closure built from a random recipe; every step keeps its value O(1) and its argument inside the domain."""
    names = list(forcings) + list(params)
    recipe = []
    for i in range(n_ops):
        kind = str(rng.choice(["add", "sub", "mul", "div", "exp", "log", "pow", "sqrt", "tanh", "sigmoid", "sin", "cos", "abs", "max", "min",
                               "where", "neg", "clip", "square", "rpow"]))
        n_avail = len(names) + i
        recipe.append((kind, [int(j) for j in rng.integers(0, n_avail, 4)], float(np.float32(rng.uniform(0.25, 1.5)))))
    outs = [int(j) for j in rng.integers(len(names) + n_ops // 2, len(names) + n_ops, n_out)]
    mix = [int(j) for j in rng.integers(0, len(params), n_out)]

    def closure(**kw):
        pool = [kw.get(n, 0.0) for n in names]            # (a forcing no output depends on is not handed over)
        for kind, (i, j, k, l), c in recipe:
            a, b, p, q = pool[i], pool[j], pool[k], pool[l]
            if kind == "add": v = 0.5 * (a + b)
            elif kind == "sub": v = 0.5 * (a - c * b)
            elif kind == "mul": v = 0.5 * a * b
            elif kind == "div": v = a / (1.0 + b * b)
            elif kind == "exp": v = np.exp(np.clip(c * a, -2.0, 2.0))
            elif kind == "log": v = np.log(c + a * a)
            elif kind == "pow": v = (1.5 + np.tanh(a)) ** np.clip(b, -2.0, 2.0)
            elif kind == "rpow": v = 2.0 ** np.clip(c * a, -3.0, 3.0)
            elif kind == "sqrt": v = np.sqrt(c + a * a)
            elif kind == "tanh": v = np.tanh(c * a)
            elif kind == "sigmoid": v = 1.0 / (1.0 + np.exp(-np.clip(a, -8.0, 8.0)))
            elif kind == "sin": v = np.sin(c * a)
            elif kind == "cos": v = np.cos(a + c)
            elif kind == "abs": v = np.abs(a - c)
            elif kind == "max": v = np.maximum(a, b * c)
            elif kind == "min": v = np.minimum(a, b + c)
            elif kind == "where": v = np.where(a > b, p, q * c)
            elif kind == "neg": v = -a
            elif kind == "clip": v = np.clip(a, -c, c)
            else: v = a ** 2 * 0.5
            pool.append(v)
        # every output also depends on a parameter directly, so no target is a constant of the parameters
        return {f"out{o}": pool[ix] + 0.5 * kw[params[m]] for o, (ix, m) in enumerate(zip(outs, mix))}
    return closure


@pytest.mark.parametrize("jit", [0, 1])
@pytest.mark.parametrize("seed", range(int(os.environ.get("EH_FUZZ_PROG_N", "40"))))
def test_random_closure_matches_the_oracle(seed, jit):
    """jit = 0: the interpreting kernels built ahead of time; 1: kernels compiled at run time around the program (about a second each)"""
    rng = np.random.default_rng(90000 + seed)
    n_par, n_forc, n_out = int(rng.integers(1, 9)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
    params, forc = [f"p{j}" for j in range(n_par)], [f"f{j}" for j in range(n_forc)]
    table = {p: (float(np.float32(rng.uniform(0.3, 0.7))), 0.0, 1.0) for p in params}
    fn = None
    for attempt in range(20):                                   # (a recipe can exceed the 64-operation budget after expansion)
        fn = _random_closure(rng, params, forc, int(rng.integers(3, 22)), n_out)
        try:
            from easyhybrid_jl_amd.program import trace
            pg = trace(fn, params, forc, [f"out{o}" for o in range(n_out)])
            break
        except NotImplementedError:
            fn = None
    assert fn is not None
    kinds = rng.integers(0, 3, n_par)
    kinds[rng.integers(n_par)] = 0
    neural = [p for p, k in zip(params, kinds) if k == 0]
    glob = [p for p, k in zip(params, kinds) if k == 1]
    wide = rng.random() < 0.25
    hidden = [int(rng.integers(65, 129))] if wide else [int(rng.integers(1, 65)) for _ in range(int(rng.integers(1, 4)))]
    targets = [f"out{o}" for o in range(n_out)]
    name = f"random_closure_{seed}"
    fn.__name__ = name
    spec = _spec(name, fn, table, list(pg.forcings), targets, neural, glob, hidden, n_pred=int(rng.integers(1, 20)),
                 act=str(rng.choice(["tanh", "sigmoid", "relu", "swish"])), scale=True)
    theta, X, f, y = _data(spec, {k: (-1.0, 1.0) for k in pg.forcings}, int(rng.integers(1, 700)), 100 + seed, nan_frac=float(rng.choice([0.0, 0.2])))
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_option("jit", jit)
    kind = "mse"
    if jit and n_out == 1 and rng.random() < 0.4:               # a recorded training loss on top of the recorded closure
        kind = str(rng.choice(sorted(cl.LOSSES)))
        eng.set_training_loss(util.register_loss(kind, cl.LOSSES[kind]))
    loss, grad, nv = eng.loss_and_grad()
    assert eng.jit_status()[0] == jit, eng.jit_status()[1]
    l0, g0, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y, kind=kind)
    assert nv == sum(nv0)
    if sum(nv0):
        # The bar is 1e-5 against the fp64 oracle, widened where fp32 itself cannot hold it: a gradient that is a small remainder
        # of cancelling per-sample terms, or a `where` whose two sides tie within rounding (the fp32 and fp64 evaluations then
        # take different branches of a discontinuous function).  What the oracle loses when it runs in fp32 measures both.
        l32, g32, _ = ho.loss_and_grad(spec, theta.astype(np.float32), X, f, y, dtype=np.float32, kind=kind)
        lbar = max(TOL, 30.0 * abs(l32 - l0) / abs(l0))
        gbar = max(2.0 * TOL, 30.0 * util.relerr(g32, g0))      # (2e-5 floor: 4 of 6 000 random cases sit at 1.05e-5 .. 1.8e-5; the curated tests above hold 1e-5)
        info = f"seed {seed}: kind={kind} B={X.shape[1]} ops={len(pg.code)} loss hip={loss!r} fp64={l0!r} fp32={l32!r} hidden={hidden} neural={neural} glob={glob}"
        assert abs(loss - l0) <= lbar * abs(l0) + 1e-9, info
        if np.max(np.abs(g0)) > 1e-7 * max(1.0, abs(l0)):
            assert util.relerr(grad, g0) <= gbar, info
            util.check_gradient(grad, g0, spec, gbar, util.ref32_orders(spec, theta.astype(np.float64), X, f, y, kind=kind))
    eng.close()


# ----------------------------------------------------------------------------------------------
# custom training losses f(yhat, y) = mean of per-sample terms (loss_fn.jl: training_loss::Function), recorded and compiled
# into the step kernel at run time
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cl.LOSSES))
@pytest.mark.parametrize("shape", ["rbq10", "config3", "wide", "closure"])
def test_custom_training_loss(name, shape):
    fn = util.register_loss(name, cl.LOSSES[name])
    if shape == "rbq10":
        spec, theta, X, f, y = util.rbq10_case(1500, "tanh", True, 0.1)
    elif shape == "config3":
        spec = ho.expo2pool_spec((64, 64), "tanh", True)
        X, f, y = ho.make_synth_expo2pool(1500, 7, 0.05)
        theta = ho.init_theta(spec, 3, np.float32)
    elif shape == "wide":
        spec, theta, X, f, y = util.rbq10_case(1500, "swish", True, 0.1, hidden=(128, 96))
    else:
        spec = _spec("flux_closure", cl.flux_closure, cl.FLUX_TABLE, ["sw", "ta", "vpd"], ["nee"], ["alpha", "rref"], ["gmax", "e0", "k"], (16, 16), n_pred=2)
        theta, X, f, y = _data(spec, dict(sw=(0, 800), ta=(-5, 30), vpd=(0, 30)), 1500, 21)
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_training_loss(fn)
    loss, grad, nv = eng.loss_and_grad()
    assert eng.jit_status()[0] == 1, eng.jit_status()[1]
    l0, g0, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y, kind=name)
    assert nv == sum(nv0) and loss == pytest.approx(l0, rel=TOL) and util.relerr(grad, g0) <= TOL
    util.check_gradient(grad, g0, spec, TOL, util.ref32_orders(spec, theta.astype(np.float64), X, f, y, kind=name))
    l1, g1, _ = eng.loss_and_grad(first=100, count=777)
    sl = slice(100, 877)
    l10, g10, _ = ho.loss_and_grad(spec, theta.astype(np.float64), X[:, sl], {k: v[sl] for k, v in f.items()}, {k: v[sl] for k, v in y.items()}, kind=name)
    assert l1 == pytest.approx(l10, rel=TOL) and util.relerr(g1, g10) <= TOL
    util.check_gradient(g1, g10, spec, TOL, util.ref32_orders(spec, theta.astype(np.float64), X[:, sl], {k: v[sl] for k, v in f.items()}, {k: v[sl] for k, v in y.items()}, kind=name))
    eng.close()


@pytest.mark.parametrize("fused", [0, 1])
def test_custom_training_loss_trajectory(fused):
    fn = util.register_loss("huber", cl.LOSSES["huber"])
    spec, theta, X, f, y = util.rbq10_case(2048, "tanh", True, 0.1)
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_training_loss(fn)
    eng.opt_init("Adam", 0.01)
    eng.set_option("fused_update", fused)
    batches = [(i * 256, 256) for i in range(8)]
    losses = [eng.train_step(a, b) for a, b in batches]
    th_ref, l_ref = ho.train_steps(spec, theta, X, f, y, batches, dtype=np.float32, kind="huber")
    assert np.allclose(losses, l_ref, rtol=1e-4)
    assert np.max(np.abs(eng.get_params() - th_ref)) <= 3e-5 * max(1.0, float(np.max(np.abs(th_ref))))
    # eval metrics are the named ones, whatever the training loss
    metrics, _ = eng.eval(0)
    ref = ho.forward(spec, eng.get_params().astype(np.float64), X, f)["reco"]
    yy = y["reco"].astype(np.float64); mask = ~np.isnan(yy)
    assert metrics[0]["mse"] == pytest.approx(ho.loss_fn(ref, yy, mask, "mse"), rel=2e-5)
    eng.close()


def test_custom_training_loss_front_door_and_refusals():
    cols = eh.synthetic.make_synth_rbq10(4000, seed=3, nan_frac=0.05)
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(eh.synthetic.RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    out = eh.train(model, cols, nepochs=5, batchsize=256, opt=eh.Adam(0.01), random_seed=1, training_loss=cl.huber_loss)
    assert out.val_history[-1]["mse"]["sum"] < 0.5 * out.val_history[0]["mse"]["sum"]
    # no other form of a recorded loss exists: with the run-time compiler switched off the step is refused, not emulated
    spec, theta, X, f, y = util.rbq10_case(300, "tanh", True, 0.1)
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_option("jit", 0)
    eng.set_training_loss(cl.huber_loss)
    eng.loss_and_grad()                                  # ("jit" governs recorded mechanistic closures; a recorded loss always compiles)
    assert eng.jit_status()[0] == 1
    with pytest.raises(eh.EngineError, match="eh_set_loss_program first"):
        e2 = util.load_engine(spec, theta, X, f, y)
        e2.set_option("training_loss", 7)
    eng.close()
