"""-m gpu: seeded random configurations of the whole descriptor space (shape, activation, mechanistic model, which
parameters are neural / global / fixed, scaling, BatchNorm, NaN pattern, batch size, window, training loss, kernel family
and variant) through the C ABI against the oracle.  One loss + gradient comparison per case."""
import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho
from tests import util

pytestmark = pytest.mark.gpu

TABLES = {
    "rbq10": dict(ho.RBQ10_PARAMS),
    "expo": dict(ho.EXPO_PARAMS),
    "linear": {"alpha": (1.0, -2.0, 3.0), "beta": (0.5, -1.0, 2.0)},
    "expo2pool": dict(ho.EXPO2POOL_PARAMS),
    "rs_components": {**{f"Rb_{c}": (1.0, 0.0, 5.0) for c in ("het", "root", "myc")},
                      **{f"Q10_{c}": (2.0 + 0.3 * i, 1.0, 4.0) for i, c in enumerate(("het", "root", "myc"))}},
    "fluxpart": {"RUE": (0.1, 0.0, 1.0), "Rb": (1.0, 0.0, 6.0), "Q10": (1.5, 1.0, 4.0)},
}
FORCING_RANGE = {"ta": (-5, 30), "T": (-0.5, 1.5), "x": (-1, 2), "SW_IN": (0, 800), "TA": (0, 30)}


def _case(seed, fastpath=False):
    """fastpath: only models the K == 1 / P <= 4 vector-ALU kernels serve (one neural parameter, few predictors, one target)"""
    rng = np.random.default_rng((500000 if fastpath else 1000) + seed)
    mech = rng.choice(list(TABLES))
    mm = ho.MECH[mech][0]
    names = list(mm.params)
    # every parameter neural / global / fixed at random, at least one neural
    kinds = rng.integers(0, 3, len(names))
    if fastpath:
        kinds = rng.integers(1, 3, len(names))
        kinds[rng.integers(len(names))] = 0
    if not (kinds == 0).any():
        kinds[rng.integers(len(names))] = 0
    neural = [n for n, k in zip(names, kinds) if k == 0]
    glob = [n for n, k in zip(names, kinds) if k == 1]
    rng.shuffle(neural); rng.shuffle(glob)
    wide = rng.random() < 0.3 and not fastpath
    nl = int(rng.integers(1, 3 if wide else 4))
    hidden = [int(rng.integers(65, 129)) if (wide and i == 0) else int(rng.integers(1, 129 if wide else 65)) for i in range(nl)]
    P = int(rng.integers(1, 7)) if fastpath else int(rng.integers(1, 33))
    act = str(rng.choice(["tanh", "sigmoid", "relu", "swish", "identity"]))
    scale = bool(rng.random() < 0.6) or mech in ("rbq10", "rs_components", "fluxpart")     # raw outputs could be negative bases of a power
    ntarg = 1 if fastpath else int(rng.integers(1, len(mm.outputs) + 1))
    targets = [str(t) for t in rng.permutation(list(mm.outputs))[:ntarg]]
    bn = bool(rng.random() < 0.25)
    nets = None
    if not fastpath and len(neural) >= 2 and rng.random() < 0.35:
        # MultiNNHybridModel: one single-output net per neural parameter on its own predictor rows, common depth,
        # widths that fit side by side (the engine runs them as one block-diagonal MLP)
        K = len(neural)
        P = max(P, K)
        cuts = np.sort(rng.choice(np.arange(1, P), K - 1, replace=False)) if K > 1 else np.array([], int)
        rows = np.split(rng.permutation(P), cuts)
        cap = (128 if wide else 64) // K
        nets = [([int(r) for r in rw], [int(rng.integers(1, cap + 1)) for _ in range(nl)]) for rw in rows]
        bn = False
    net_acts = None
    if nets is not None:
        # activation::NamedTuple: every second MultiNN model gives each net its own activation (a stream of its own, so the
        # configurations drawn before this existed stay what they were)
        rng_a = np.random.default_rng(900000 + seed)
        if rng_a.random() < 0.5:
            net_acts = [str(a) for a in rng_a.choice(["tanh", "sigmoid", "relu", "swish", "identity"], len(nets))]
        if nl > 1 and rng_a.random() < 0.4:          # hidden_layers::NamedTuple with vectors of different length: some nets shallower
            keep = int(rng_a.integers(len(nets)))    # (one keeps the full depth)
            nets = [(rw, hw if k == keep else hw[: int(rng_a.integers(1, nl + 1))]) for k, (rw, hw) in enumerate(nets)]
    spec = ho.HybridSpec(P, hidden, mech, TABLES[mech], neural, glob, targets, act, scale, input_batchnorm=bn, nets=nets,
                         net_activations=net_acts)
    B = int(rng.choice([1, 7, 31, 32, 33, 64, 257, 1000, 2049]))
    N = B + int(rng.integers(0, 200))
    X = (rng.standard_normal((P, N)) * rng.uniform(0.2, 1.5) + (rng.uniform(-3, 3) if bn else 0.0)).astype(np.float32)
    f = {k: rng.uniform(*FORCING_RANGE[k], N).astype(np.float32) for k in mm.forcings}
    y = {}
    for t in targets:
        v = rng.uniform(0.5, 6, N).astype(np.float32)
        v[rng.random(N) < rng.choice([0.0, 0.1, 0.6])] = np.nan
        y[t] = v
    kind = "mse" if ntarg > 1 else str(rng.choice(["mse", "mse", "rmse", "mae", "nseLoss", "kgeLoss", "pearsonLoss"]))
    first = int(rng.integers(0, N - B + 1))
    return spec, ho.init_theta(spec, seed, np.float32), X, f, y, kind, first, B, rng


@pytest.mark.parametrize("fastpath", [False, True])
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("EH_FUZZ_N", "60"))))
def test_random_configuration_matches_the_oracle(seed, fastpath):
    spec, theta, X, f, y, kind, first, B, rng = _case(seed, fastpath)
    sl = slice(first, first + B)
    yb = {k: v[sl] for k, v in y.items()}
    if kind in ("kgeLoss", "pearsonLoss", "nseLoss") and sum(int((~np.isnan(v)).sum()) for v in yb.values()) < 3:
        kind = "mse"                                              # variance / correlation of fewer than 3 points
    eng = util.load_engine(spec, theta, X, f, y)
    if kind != "mse":
        eng.set_training_loss(kind)
    for opt, val in (("variant", 0), ("row_split", 1), ("fast_paths", 0)):
        if rng.random() < 0.3:
            try:
                eng.set_option(opt, val)
            except (NotImplementedError, ValueError):
                pass
    try:
        loss, grad, nv = eng.loss_and_grad(first=first, count=B)
    except eh.EngineError as e:                                   # (a failed run-time build says why)
        raise AssertionError(f"{e}; jit: {eng.jit_status()}") from e
    l0, g0, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind=kind,
                                   bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
    # (correlation of nearly constant predictions -- a random sigmoid net squeezed through a one-unit layer -- is as
    # ill-conditioned as it sounds: 1e-3 here, the well-conditioned cases of test_gpu_parity.py hold 1e-4)
    tol = 1e-3 if kind in ("kgeLoss", "pearsonLoss") else 1e-5
    assert nv == sum(nv0)
    if sum(nv0) == 0:
        assert np.isnan(loss) and not grad.any()
    else:
        yscale = float(np.nanmax(np.abs(np.concatenate(list(yb.values())))))
        # (kgeLoss / pearsonLoss are differences from 1 of O(1) statistics: a value near zero carries their absolute rounding, ~1e-6 in fp32)
        atol = tol * yscale * (yscale if kind == "mse" else 1.0) if kind in ("mse", "mae", "rmse") else (1e-5 if kind in ("kgeLoss", "pearsonLoss") else None)
        assert loss == pytest.approx(l0, rel=tol, abs=atol), (kind, spec)
        if np.max(np.abs(g0)) > 1e-7 * max(1.0, abs(l0)):         # (a loss the parameters cannot move has a gradient of pure rounding noise)
            err = util.relerr(grad, g0)
            if err > tol:
                # the arithmetic or the kernels?  Where the oracle itself, run in fp32, cannot hold the bar, the bar is four times what it loses (as in the raw-scale test below)
                # (seed 2753 of 5 000: pearsonLoss of 31 samples behind a two-unit relu layer -- device 3.0e-3, fp32 oracle 6.9e-2)
                _, g32, _ = ho.loss_and_grad(spec, theta.astype(np.float32), X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind=kind, dtype=np.float32,
                                             bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
                assert err <= max(tol, 4.0 * util.relerr(g32, g0)), (kind, spec, err, util.relerr(g32, g0))
            # Seed 1 (not fastpath): rmse of fluxpart's RECO over B = 7, Q10 from the network.  The output bias is ONE sum of seven deltas that cancel to
            # 1 / 42 of their absolute sum; each delta goes through eh_pow (v_log_f32, v_exp_f32), two reciprocals and the sigmoid scaling (csrc/eh_device.hpp,
            # eh_mech_extra), about one ulp each -- 3e-7 per delta, 1.30e-5 on the leaf.  Arithmetic the kernel is entitled to, shown on the reference side:
            # the fp32 oracle loses 1.69e-6 on that leaf over its four orders and 4.35e-6 over seventeen (16 permutations), within the factor 4 of the device.
            n_perm = 16 if (seed, fastpath) == (1, False) else util.REF32_ORDERS
            util.check_gradient(grad, g0, spec, tol, util.ref32_orders(spec, theta, X[:, sl], {k: v[sl] for k, v in f.items()}, yb, n_perm=n_perm, kind=kind,
                                                                      bn_state=ho.bn_init(spec) if spec.input_batchnorm else None))
        else:
            assert np.max(np.abs(grad)) <= 1e-5 * max(1.0, abs(l0)), (kind, spec)
    eng.close()


def _one_block_seeds(n, fastpath):
    """the first n fuzz seeds whose model runs on a one-block shape of the per-wave family (every hidden width <= 16, side-by-side nets
    included): the shapes whose run-time compiled kernels get the SLP vectoriser (csrc/eh_jit.hip)"""
    out, seed = [], 0
    while len(out) < n and seed < 20000:
        spec = _case(seed, fastpath)[0]
        widths = [sum(h[l] if l < len(h) else h[-1] for _, h in spec.nets) for l in range(max(len(h) for _, h in spec.nets))] if spec.nets else list(spec.hidden)
        if max(widths) <= 16:
            out.append(seed)
        seed += 1
    return out


@pytest.mark.parametrize("fastpath,seed", [(fp, s) for fp in (False, True) for s in _one_block_seeds(30, fp)])
def test_one_block_shapes_on_run_time_specialised_kernels(seed, fastpath):
    """the run-time kernels of the one-block shapes (NBH = 1) are built with the SLP vectoriser ON -- the pass that
    miscompiled a sibling group of kernels in round 2 -- so a slice of the fuzz runs on them in every suite run: 60 configurations
    with "specialize" = 1, loss and gradient against the oracle, and the library's own cross-check against the kernel built ahead of
    time (jit_verify) must have passed (the kernel is in use, nothing in the log)."""
    spec, theta, X, f, y, kind, first, B, rng = _case(seed, fastpath)
    sl = slice(first, first + B)
    yb = {k: v[sl] for k, v in y.items()}
    if kind in ("kgeLoss", "pearsonLoss", "nseLoss"):
        kind = "mse"                                              # (tiny batches: their statistics are the first test's business)
    eng = util.load_engine(spec, theta, X, f, y)
    if kind != "mse":
        eng.set_training_loss(kind)
    eng.set_option("specialize", 1)
    loss, grad, nv = eng.loss_and_grad(first=first, count=B)
    njit, jlog = eng.jit_status()
    assert njit >= 1 and "disagrees" not in jlog, jlog[:400]
    l0, g0, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind=kind,
                                   bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
    assert nv == sum(nv0)
    if sum(nv0) == 0:
        assert np.isnan(loss) and not grad.any()
    else:
        yscale = float(np.nanmax(np.abs(np.concatenate(list(yb.values())))))
        assert loss == pytest.approx(l0, rel=1e-5, abs=1e-5 * yscale * (yscale if kind == "mse" else 1.0)), (kind, spec)
        if np.max(np.abs(g0)) > 1e-7 * max(1.0, abs(l0)):
            err = util.relerr(grad, g0)
            if err > 1e-5:
                _, g32, _ = ho.loss_and_grad(spec, theta.astype(np.float32), X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind=kind, dtype=np.float32,
                                             bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
                assert err <= max(1e-5, 4.0 * util.relerr(g32, g0)), (kind, spec, err, util.relerr(g32, g0))
            util.check_gradient(grad, g0, spec, 1e-5, util.ref32_orders(spec, theta, X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind=kind,
                                                                      bn_state=ho.bn_init(spec) if spec.input_batchnorm else None))
    eng.close()


@pytest.mark.parametrize("fastpath", [False, True])
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("EH_FUZZ_N", "60")) // 3))
def test_random_configuration_at_the_raw_input_scale(seed, fastpath):
    """the same walk with the predictors left at the scale the reference's synthetic columns have (sw_pot ~ |50 + 20 N(0,1)|,
    test/test_split_data_train.jl:15-31) instead of O(1): saturated tanh / sigmoid units, large relu / swish / identity ones.
    sigma-scaled outputs (an un-scaled linear output of magnitude 100 is no physical parameter for any of the models)."""
    spec, theta, X, f, y, kind, first, B, rng = _case(40000 + seed, fastpath)
    spec.scale_nn_outputs = True
    rng2 = np.random.default_rng(50000 + seed)
    X = np.abs(50.0 + 20.0 * rng2.standard_normal(X.shape)).astype(np.float32)
    if kind in ("kgeLoss", "pearsonLoss", "nseLoss"):
        kind = "mse"                                              # (saturated nets predict near-constants: their correlation is noise)
    sl = slice(first, first + B)
    yb = {k: v[sl] for k, v in y.items()}
    eng = util.load_engine(spec, theta, X, f, y)
    if kind != "mse":
        eng.set_training_loss(kind)
    loss, grad, nv = eng.loss_and_grad(first=first, count=B)
    l0, g0, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind=kind,
                                   bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
    assert nv == sum(nv0)
    if sum(nv0) == 0:
        assert np.isnan(loss) and not grad.any()
    else:
        # Saturated sigmoid / tanh units and unbounded relu / swish / identity ones of magnitude 1e2-1e3 make the gradient a small
        # remainder of large terms: where the fp32 oracle (the reference's own arithmetic) cannot hold 1e-5 against the fp64 one, the
        # bar is four times what it loses.
        l32, g32, _ = ho.loss_and_grad(spec, theta.astype(np.float32), X[:, sl], {k: v[sl] for k, v in f.items()}, yb, dtype=np.float32, kind=kind,
                                       bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
        gmax = float(np.max(np.abs(g0)))
        lost = util.relerr(g32, g0) if gmax > 0 else 0.0          # what the reference's own precision loses on this gradient
        tol_l = min(1e-3, max(1e-5, 4 * abs(float(l32) - l0) / abs(l0)))
        tol_g = max(1e-5, 4 * lost)
        assert np.isfinite(l0) and loss == pytest.approx(l0, rel=tol_l), (kind, spec)
        if lost > 0.02:
            pass                                                  # (fp32 itself does not hold this gradient: every unit saturated, the remainder is rounding)
        elif gmax > 1e-7 * max(1.0, abs(l0)):
            assert util.relerr(grad, g0) <= tol_g, (kind, spec, util.relerr(grad, g0), tol_g)
            util.check_gradient(grad, g0, spec, 1e-5, util.ref32_orders(spec, theta, X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind=kind,
                                                                      bn_state=ho.bn_init(spec) if spec.input_batchnorm else None))
        else:
            assert np.max(np.abs(grad)) <= 1e-5 * max(1.0, abs(l0)), (kind, spec)
        out = eng.forward(eh.EH_SPLIT_TRAIN, first, B, params=False)
        ref = ho.forward(spec, theta.astype(np.float64), X[:, sl], {k: v[sl] for k, v in f.items()},
                         bn_state=ho.bn_init(spec) if spec.input_batchnorm else None, train_mode=False)
        for t in spec.targets:
            assert util.relerr(out[t], ref[t]) <= 1e-5, (t, spec)
    eng.close()


@pytest.mark.parametrize("fastpath", [False, True])
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("EH_FUZZ_N", "60")) // 2))
def test_random_configuration_trains_and_predicts_like_the_oracle(seed, fastpath):
    """a few optimiser steps (random rule, fused-update mode where the model allows it) and the forward / eval outputs"""
    spec, theta, X, f, y, kind, first, B, rng = _case(7000 + seed, fastpath)
    if kind in ("kgeLoss", "pearsonLoss", "nseLoss"):
        kind = "mse"                                    # (statistics of tiny batches: covered by the one-shot test above)
    N = X.shape[1]
    eng = util.load_engine(spec, theta, X, f, y)
    if kind != "mse":
        eng.set_training_loss(kind)
    fused = False
    if len(spec.targets) == 1 and rng.random() < 0.5:
        try:
            eng.set_option("fused_update", 1); fused = True
        except NotImplementedError:
            pass
    # plain gradient descent: Adam's first steps are sign-like, so rounding noise in a near-zero gradient entry would be
    # blown up to a full step (the Adam trajectory has its own, conditioned tests)
    b = max(1, N // 3)
    if spec.input_batchnorm and b < 16:
        pytest.skip("BatchNorm statistics of a handful of samples are ill-conditioned")
    eng.opt_init("Descent", 0.01)
    batches = [(i * b, b) for i in range(3) if (i + 1) * b <= N]
    losses = [eng.train_step(*bt) for bt in batches]
    st = ho.bn_init(spec) if spec.input_batchnorm else None
    th_ref = theta.astype(np.float32).copy(); l_ref = []
    for a0, n0 in batches:
        sl = slice(a0, a0 + n0)
        yb = {k: v[sl] for k, v in y.items()}
        if not any((~np.isnan(v)).any() for v in yb.values()):
            l_ref.append(float("nan")); continue
        l, g, _ = ho.loss_and_grad(spec, th_ref.astype(np.float64), X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind=kind, bn_state=st)
        if st is not None:
            _, new = ho.batchnorm_input(np.asarray(X[:, sl], np.float64), st, True, np.dtype(np.float64)); st.update(new)
        th_ref = (th_ref - np.float32(0.01) * g.astype(np.float32)).astype(np.float32); l_ref.append(float(l))
    ok = ~np.isnan(np.asarray(l_ref))
    assert np.array_equal(np.isnan(losses), ~ok)
    yscale = float(np.nanmax(np.abs(np.concatenate(list(y.values())))))
    assert np.allclose(np.asarray(losses)[ok], np.asarray(l_ref)[ok], rtol=3e-4, atol=1e-5 * yscale * yscale), (kind, fused, spec)
    th = eng.get_params()
    if not np.all(np.isfinite(th_ref)):
        assert not np.all(np.isfinite(th))               # (un-scaled outputs into an exponential: the descent diverges, for the oracle and for the engine)
        eng.close()
        pytest.skip("the descent trajectory diverges")
    assert np.max(np.abs(th - th_ref)) <= 1e-4 * max(1.0, float(np.max(np.abs(th_ref)))), (kind, fused, spec)
    out = eng.forward(0)
    ref = ho.forward(spec, th.astype(np.float64), X, f, bn_state=st, train_mode=False)
    for t in spec.targets:
        assert util.relerr(out[t], ref[t]) <= 3e-5, (t, spec)
    eng.close()


def _lform_case(seed):
    """networks only the layer-wise form holds (a width above 128 or more than three hidden layers; MultiNN models whose networks do
    not fit side by side), batch sizes on both sides of every switch of its small- and mid-batch paths (16 / 32-row tiles at 512, the
    few-rows products up to 1 024, grouped weight gradients up to 4 096, one-workgroup mechanistic stage up to 256)"""
    rng = np.random.default_rng(700000 + seed)
    mech = rng.choice(list(TABLES))
    mm = ho.MECH[mech][0]
    names = list(mm.params)
    kinds = rng.integers(0, 3, len(names))
    if not (kinds == 0).any():
        kinds[rng.integers(len(names))] = 0
    neural = [n for n, k in zip(names, kinds) if k == 0]
    glob = [n for n, k in zip(names, kinds) if k == 1]
    rng.shuffle(neural); rng.shuffle(glob)
    menu = [16, 32, 48, 64, 80, 96, 128, 144, 160, 192, 256, 320, 30, 129, 10]      # mostly whole 16-deep k groups (the aligned kernels), some not
    def widths(force):
        while True:
            nl = int(rng.integers(1, 7))
            w = [int(rng.choice(menu)) for _ in range(nl)]
            if not force or nl > 3 or max(w) > 128:
                return w
    P = int(rng.integers(1, 13))
    act = str(rng.choice(["tanh", "sigmoid", "relu", "swish", "identity"]))
    ntarg = int(rng.integers(1, len(mm.outputs) + 1))
    targets = [str(t) for t in rng.permutation(list(mm.outputs))[:ntarg]]
    nets, net_acts, hidden = None, None, widths(True)
    bn = bool(rng.random() < 0.3)
    if len(neural) >= 2 and rng.random() < 0.4:
        K = len(neural)
        P = max(P, K)
        cuts = np.sort(rng.choice(np.arange(1, P), K - 1, replace=False))
        rows = np.split(rng.permutation(P), cuts)
        nets = [([int(r) for r in rw], widths(k == 0)) for k, rw in enumerate(rows)]
        if rng.random() < 0.5:
            net_acts = [str(a) for a in rng.choice(["tanh", "sigmoid", "relu", "swish", "identity"], K)]
        bn = False
    spec = ho.HybridSpec(P, hidden, mech, TABLES[mech], neural, glob, targets, act, True, input_batchnorm=bn, nets=nets, net_activations=net_acts)
    B = int(rng.choice([1, 15, 16, 17, 64, 255, 256, 257, 500, 511, 512, 513, 1000, 1024, 1025, 2047, 4096, 4097, 5000]))
    N = B + int(rng.integers(0, 300))
    X = (rng.standard_normal((P, N)) * rng.uniform(0.2, 1.5) + (rng.uniform(-3, 3) if bn else 0.0)).astype(np.float32)
    f = {k: rng.uniform(*FORCING_RANGE[k], N).astype(np.float32) for k in mm.forcings}
    y = {}
    for t in targets:
        v = rng.uniform(0.5, 6, N).astype(np.float32)
        v[rng.random(N) < rng.choice([0.0, 0.1, 0.6])] = np.nan
        y[t] = v
    kind = "mse" if ntarg > 1 else str(rng.choice(["mse", "mse", "mse", "rmse", "mae", "nseLoss"]))
    gather = bool(rng.random() < 0.3)
    rng_l = np.random.default_rng(710000 + seed)          # (a stream of its own: the configurations drawn before this existed stay what they were)
    if rng_l.random() < 0.25:
        kind = "fuzz_huber"                               # a recorded loss function (every target): interpreted in this form
    return spec, ho.init_theta(spec, seed, np.float32), X, f, y, kind, B, N, gather, rng


def _fuzz_huber(yh, y):
    r = np.abs(yh - y)
    return np.mean(np.where(r <= 0.8, 0.5 * r * r, 0.8 * (r - 0.4)))


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("EH_FUZZ_N", "60")) // 2))
def test_random_layerwise_configuration_matches_the_oracle(seed):
    spec, theta, X, f, y, kind, B, N, gather, rng = _lform_case(seed)
    if gather:
        idx = rng.permutation(N)[:B].astype(np.int32)
        kw = {"idx": idx}
    else:
        first = int(rng.integers(0, N - B + 1))
        idx = np.arange(first, first + B)
        kw = {"first": first, "count": B}
    yb = {k: v[idx] for k, v in y.items()}
    if kind == "nseLoss" and sum(int((~np.isnan(v)).sum()) for v in yb.values()) < 3:
        kind = "mse"
    eng = util.load_engine(spec, theta, X, f, y)
    if kind == "fuzz_huber":
        util.register_loss("fuzz_huber", _fuzz_huber)
        eng.set_training_loss(_fuzz_huber)
        kind = tuple("fuzz_huber" for _ in spec.targets) if len(spec.targets) > 1 else "fuzz_huber"
    elif kind != "mse":
        eng.set_training_loss(kind)
    loss, grad, nv = eng.loss_and_grad(**kw)
    Xo = X
    l0, g0, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), Xo[:, idx], {k: v[idx] for k, v in f.items()}, yb, kind=kind,
                                   bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
    assert nv == sum(nv0)
    if sum(nv0) == 0:
        assert np.isnan(loss) and not grad.any()
    else:
        yscale = float(np.nanmax(np.abs(np.concatenate(list(yb.values())))))
        assert loss == pytest.approx(l0, rel=1e-5, abs=1e-5 * yscale * (yscale if kind == "mse" else 1.0) if kind in ("mse", "mae", "rmse", "fuzz_huber") or isinstance(kind, tuple) else None), (kind, spec, B)
        if np.max(np.abs(g0)) > 1e-7 * max(1.0, abs(l0)):
            err = util.relerr(grad, g0)
            if err > 1e-5:
                # six sigmoid layers in front of an mae loss: is it the arithmetic or the kernels?  The bar where fp32 itself cannot hold
                # 1e-5 is four times what the oracle loses when IT runs in fp32 (seed 859: device 9.9e-5, fp32 oracle 1.3e-4; seed 1503, one sample: 6.8e-5 / 2.8e-5)
                _, g32, _ = ho.loss_and_grad(spec, theta.astype(np.float32), X[:, idx], {k: v[idx] for k, v in f.items()}, yb, kind=kind, dtype=np.float32,
                                             bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
                assert err <= max(1e-5, 4.0 * util.relerr(g32, g0)), (kind, spec, B, err, util.relerr(g32, g0))
            util.check_gradient(grad, g0, spec, 1e-5, util.ref32_orders(spec, theta, X[:, idx], {k: v[idx] for k, v in f.items()}, yb, kind=kind,
                                                                      bn_state=ho.bn_init(spec) if spec.input_batchnorm else None))
        else:
            assert np.max(np.abs(grad)) <= 1e-5 * max(1.0, abs(l0)), (kind, spec, B)
    eng.close()


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("EH_FUZZ_N", "60"))))
def test_random_small_minibatch_epochs_several_steps_per_launch(seed):
    """eh_train_epoch on minibatches one workgroup covers: several fused-update steps per launch with the state in LDS (EH_MODE_TRAIN_MULTI)
    against one launch per step -- same arithmetic, only the order in which a workgroup's float atomics meet differs -- over random
    per-wave configurations with one target: shape, activation, mechanistic model, parameter kinds, scaling, BatchNorm, missing targets,
    optimiser, minibatch size (incl. sizes that leave a partial last minibatch), shuffled or not"""
    for sub in range(40):                                  # the next configuration of this seed's stream that the mode serves
        spec, theta, X, f, y, kind, first, B, rng = _case(7000 + 40 * seed + sub, fastpath=bool(seed % 2))
        if len(spec.targets) == 1 and spec.nets is None and max(spec.hidden) <= 64 and kind in ("mse", "rmse", "mae", "nseLoss"):
            break
    else:
        pytest.skip("no eligible configuration in this seed's stream")
    N = X.shape[1]
    batch = int(rng.choice([1, 5, 16, 32, 33, 64, 100, 128]))
    opt = [("Adam", 0.01), ("RMSProp", 0.005), ("AdamW", 0.01), ("Descent", 0.01)][int(rng.integers(4))]
    shuffle = bool(rng.integers(2))
    out = []
    for multi in (1, 0):
        eng = util.load_engine(spec, theta, X, f, y)
        eng.set_training_loss(kind)
        eng.opt_init(*opt)
        try:
            eng.set_option("fused_update", 1)
        except Exception:
            eng.close(); pytest.skip("no fused-update mode for this configuration")
        eng.set_option("multi_step", multi)
        l0, n0 = eng.train_epoch(batch, seed=seed, shuffle=shuffle)
        eng.train_epoch(batch, seed=seed + 1, shuffle=shuffle, want_loss=False)
        out.append((l0, n0, eng.get_params(), eng.forward(0, params=False)[spec.targets[0]]))
        eng.close()
    (l1, n1, t1, p1), (l0, n0, t0, p0) = out
    assert n1 == n0 == -(-N // batch)
    if not (np.all(np.isfinite(t0)) and np.isfinite(l0)):
        pytest.skip("the descent diverges for this configuration (one launch per step as well)")
    scale = max(1.0, float(np.max(np.abs(t0))))
    assert l1 == pytest.approx(l0, rel=1e-4, abs=1e-6), (spec, kind, batch, opt)
    assert np.max(np.abs(t1 - t0)) <= 1e-4 * scale, (spec, kind, batch, opt, float(np.max(np.abs(t1 - t0))))
    assert util.relerr(p1, p0) <= 1e-3


@pytest.mark.parametrize("opt", [("Descent", 0.01), ("RMSProp", 0.005), ("Adam", 0.01), ("AdamW", 0.01)])
@pytest.mark.parametrize("batch", [1, 33])
def test_several_steps_per_launch_are_bit_for_bit_one_launch_per_step(opt, batch):
    """A minibatch one workgroup covers takes no float atomic that meets another: the multi-step launch and one launch per step run the
    same operations in the same order, so their trajectories are IDENTICAL -- for every optimiser rule.  Found by the extended fuzz
    (EH_FUZZ_N=300, seed 296: plain SGD on single-sample minibatches of un-normalised predictors, a chaotic descent): Descent's
    `theta - eta * g` had been contracted into one fma in the multi-step kernel and not in the single-step one, one ulp per step that
    the descent amplified to O(1) within a few hundred steps; the optimiser rules are compiled without contraction since
    (csrc/eh_device.hpp eh_opt_update: "op for op", as Optimisers.jl's broadcasts and the oracle's NumPy)."""
    spec, theta, X, f, y, kind, first, B, rng = _case(7000 + 40 * 296, fastpath=False)
    for sub in range(40):
        spec, theta, X, f, y, kind, first, B, rng = _case(7000 + 40 * 296 + sub, fastpath=False)
        if len(spec.targets) == 1 and spec.nets is None and max(spec.hidden) <= 64 and kind in ("mse", "rmse", "mae", "nseLoss"):
            break
    n = 400
    X, f, y = X[:, :n], {k: v[:n] for k, v in f.items()}, {k: v[:n] for k, v in y.items()}
    out = []
    for multi in (1, 0):
        eng = util.load_engine(spec, theta, X, f, y)
        eng.set_training_loss(kind); eng.opt_init(*opt); eng.set_option("fused_update", 1); eng.set_option("multi_step", multi)
        l0, _ = eng.train_epoch(batch, seed=3, shuffle=True)
        out.append((l0, eng.get_params()))
        eng.close()
    assert np.all(np.isfinite(out[1][1]))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])

