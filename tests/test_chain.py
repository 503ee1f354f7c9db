"""Optimiser chains without a GPU: flattening and validation (train._opt_groups, eh_opt_init_chain on a null handle), the NumPy twin
(tests/chain_twin.py) against closed forms, and the inputs of the GPU cases (tests/chain_cases.py): on every step of every trajectory
the twin's fp64 norm lies farther than 1e-3 relative from omega -- a norm on the threshold flips on rounding, which is a question to the
input and not to a kernel -- and some steps clip while others do not."""
import ctypes as C
import sys

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
import easyhybrid_jl_amd.train  # noqa: F401
from oracle import hybrid_oracle as ho

from tests import chain_cases as cc
from tests.chain_twin import ChainTwin, norm_p

T = sys.modules["easyhybrid_jl_amd.train"]
INF = float("inf")


def _model():
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, {"rb": (3, 0, 13), "Q10": (2, 1, 4)}, ["rb"], ["Q10"], hidden_layers=[16, 16])


# ---- flattening and validation -------------------------------------------------------------------------------------------------------
def test_exports_and_frozen_dataclasses():
    for cls in (eh.OptimiserChain, eh.ClipGrad, eh.ClipNorm, eh.WeightDecay):
        assert getattr(T, cls.__name__) is cls
    assert (eh.ClipGrad().delta, eh.ClipNorm().omega, eh.ClipNorm().p, eh.ClipNorm().throw, eh.WeightDecay().lambda_) == (10.0, 10.0, 2.0, True, 5e-4)
    with pytest.raises(Exception):
        eh.ClipNorm(1.0).omega = 2.0
    with pytest.raises(Exception):
        eh.OptimiserChain(eh.Adam()).opts = ()
    assert eh.OptimiserChain(eh.ClipNorm(1.0), eh.Adam(0.01)) == eh.OptimiserChain(eh.ClipNorm(1.0), eh.Adam(0.01))


def test_a_chain_becomes_stages_and_one_rule_and_nested_chains_flatten():
    group, rules = T._opt_groups(eh.OptimiserChain(eh.ClipNorm(1), eh.Adam(0.01)), _model())
    assert group is None and len(rules) == 1
    assert rules[0] == dict(rule="Adam", lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, stages=[("clipnorm", 1.0, 2.0, True), ("rule",)])
    nested = eh.OptimiserChain(eh.WeightDecay(1e-3), eh.OptimiserChain(eh.ClipNorm(2.0, INF, throw=False), eh.OptimiserChain(eh.ClipGrad(0.5))),
                               eh.OptimiserChain(eh.AdamW(0.01, (0.8, 0.99), 0.1), eh.ClipGrad(0.005)))
    _, (a,) = T._opt_groups(nested, _model())
    assert a["stages"] == [("weightdecay", 1e-3), ("clipnorm", 2.0, INF, False), ("clipgrad", 0.5), ("rule",), ("clipgrad", 0.005)]
    assert (a["rule"], a["lr"], a["beta1"], a["beta2"], a["weight_decay"]) == ("AdamW", 0.01, 0.8, 0.99, 0.1)
    # eight stages are kept, a ninth is not
    eight = eh.OptimiserChain(*([eh.ClipGrad(1.0)] * 7), eh.Descent(0.1))
    assert len(T._opt_groups(eight, _model())[1][0]["stages"]) == 8
    with pytest.raises(NotImplementedError, match="at most 8"):
        T._opt_groups(eh.OptimiserChain(eh.ClipGrad(1.0), eight), _model())


@pytest.mark.parametrize("opt,exc,why", [
    (lambda: eh.OptimiserChain(eh.ClipGrad(1.0)), NotImplementedError, "without a rule"),
    (lambda: eh.OptimiserChain(eh.Adam(), eh.Descent()), NotImplementedError, "second rule"),
    (lambda: eh.OptimiserChain(eh.Adam(), eh.ClipNorm(1.0)), NotImplementedError, "behind the rule"),
    (lambda: eh.OptimiserChain(eh.ClipNorm(1.0), eh.ClipNorm(2.0), eh.Adam()), NotImplementedError, "second ClipNorm"),
    (lambda: eh.OptimiserChain(eh.ClipNorm(1.0, 3), eh.Adam()), NotImplementedError, "1-, 2- and Inf-norm"),
    (lambda: eh.OptimiserChain("Lion", eh.Adam()), NotImplementedError, "stage 'Lion'"),
    (lambda: eh.OptimiserChain(eh.ClipGrad(-1.0), eh.Adam()), ValueError, "delta"),
    (lambda: eh.OptimiserChain(eh.ClipNorm(0.0), eh.Adam()), ValueError, "omega"),
    (lambda: eh.OptimiserChain(eh.ClipNorm(-2.0), eh.Adam()), ValueError, "omega"),
    (lambda: eh.OptimiserChain(eh.Adam(), eh.WeightDecay(-1e-3)), ValueError, "lambda"),
    (lambda: {"ps": eh.OptimiserChain(eh.ClipNorm(1.0), eh.Adam())}, NotImplementedError, "per branch is not built"),
])
def test_every_refusal_with_its_reason(opt, exc, why):
    with pytest.raises(exc, match=why):
        T._opt_groups(opt(), _model())


def test_fused_update_true_is_refused_for_a_chain_with_the_reason():
    class Eng:
        has_chain = True
        opts = []

        def set_option(self, k, v):
            self.opts.append((k, v))
    with pytest.raises(NotImplementedError, match="norm of the whole"):
        T._apply_step_mode(Eng(), T.TrainConfig(fused_update=True))
    e = Eng()
    T._apply_step_mode(e, T.TrainConfig(fused_update="auto", random_seed=1))
    assert ("fused_update", 0) in e.opts          # the step + reduce + chain form


def test_c_entry_points_on_a_null_handle():
    lib = L.lib()
    st = (L.OptStage * 2)(L.OptStage(L.EH_STAGE_CLIPNORM, 1.0, 2.0, 1), L.OptStage(L.EH_STAGE_RULE, 0.0, 0.0, 0))
    assert lib.eh_opt_init_chain(None, st, 2, 0, 0.01, 0.9, 0.999, 1e-8, 0.0) == L.EH_EINVAL
    n = C.c_int64()
    assert lib.eh_opt_chain_status(None, C.byref(n), C.byref(n), C.byref(n)) == L.EH_EINVAL
    assert C.sizeof(L.OptStage) == 16 and L.EH_MAX_OPT_STAGES == 8


# ---- the twin against closed forms ---------------------------------------------------------------------------------------------------
def _rand(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * scale, rng.standard_normal(n)


@pytest.mark.parametrize("p", [1.0, 2.0, INF])
def test_a_clipped_descent_step_has_the_norm_eta_omega(p):
    g, x = _rand(1000, 1)
    eta, omega = 0.05, 0.3
    tw = ChainTwin(1000, [("clipnorm", omega, p, True), ("rule",)], rule="Descent", lr=eta, dtype=np.float64)
    new = tw.step(x, g)
    assert norm_p(g, p, np.float64) > omega and tw.status == (1, 1, 0)
    assert norm_p(x - new, p, np.float64) == pytest.approx(eta * omega, rel=1e-12)
    # below the threshold nothing is scaled
    tw = ChainTwin(1000, [("clipnorm", 1e6, p, True), ("rule",)], rule="Descent", lr=eta, dtype=np.float64)
    assert np.array_equal(tw.step(x, g), x - eta * g) and tw.status == (1, 0, 0)


def test_clipgrad_bounds_the_step_by_eta_delta():
    g, x = _rand(1000, 2, 3.0)
    tw = ChainTwin(1000, [("clipgrad", 0.5), ("rule",)], rule="Descent", lr=0.1, dtype=np.float64)
    d = x - tw.step(x, g)
    assert np.abs(d).max() <= 0.1 * 0.5 * (1 + 1e-12) and np.any(np.abs(g) > 0.5)
    small = np.abs(g) <= 0.5
    assert np.allclose(d[small], 0.1 * g[small], rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_adam_then_weightdecay_against_the_oracles_adam_step(dtype):
    """OptimiserChain(Adam(eta, beta), WeightDecay(lam)): x - (adam_dx + lam x); adam_step(..., weight_decay = w) is x - (adam_dx + eta w x)
    (AdamW, couple = true).  The two coincide where lam = eta w -- up to the rounding of that product and to the running products of beta
    (a power in the oracle), a few ulp."""
    g, x = _rand(300, 3)
    eta, w = 0.01, 0.2
    T_ = np.dtype(dtype).type
    lam = float(T_(eta) * T_(w))
    tw = ChainTwin(300, [("rule",), ("weightdecay", lam)], rule="Adam", lr=eta, dtype=dtype)
    th, ref, st = x.astype(dtype), x.astype(dtype), ho.adam_init(300, dtype)
    for k in range(4):
        gk = (g * (1 + 0.3 * k)).astype(dtype)
        th = tw.step(th, gk)
        ref = ho.adam_step(ref, gk, st, lr=eta, weight_decay=w)
    assert np.max(np.abs(th - ref)) <= 64 * np.finfo(dtype).eps * np.max(np.abs(ref))
    # and the plain rule is the oracle's (which squares the gradient as ((1 - b2) g) g where Optimisers and the twin take (1 - b2) abs2(g): ulps)
    a = ChainTwin(300, [("rule",)], rule="Adam", lr=eta, dtype=dtype).step(x.astype(dtype), g.astype(dtype))
    assert np.max(np.abs(a - ho.adam_step(x.astype(dtype), g.astype(dtype), ho.adam_init(300, dtype), lr=eta))) <= 8 * np.finfo(dtype).eps * np.max(np.abs(a))


def test_nan_and_non_finite_norms():
    g, x = _rand(50, 4)
    g[7] = np.nan
    for p in (1.0, 2.0, INF):
        tw = ChainTwin(50, [("clipnorm", 1.0, p, True), ("rule",)], rule="Adam", dtype=np.float32)
        assert np.array_equal(tw.step(x.astype(np.float32), g.astype(np.float32)), x.astype(np.float32)) and tw.status == (0, 0, 1)
        assert tw.bt1 == np.float32(0.9) and not tw.m.any()
        tw = ChainTwin(50, [("clipnorm", 1.0, p, False), ("rule",)], rule="Descent", dtype=np.float32)
        assert np.isnan(tw.step(x.astype(np.float32), g.astype(np.float32))).all() and tw.status == (1, 0, 1)      # lambda is NaN: Julia's min hands it through
    tw = ChainTwin(50, [("clipgrad", 1.0), ("rule",)], rule="Descent", dtype=np.float32)
    assert np.isnan(tw.step(x.astype(np.float32), g.astype(np.float32))[7])                                          # ... and so does clamp
    tw = ChainTwin(50, [("clipnorm", 1.0, 2.0, True), ("rule",)], rule="Adam", dtype=np.float32)
    assert np.array_equal(tw.step(x.astype(np.float32), g.astype(np.float32), valid=False), x.astype(np.float32)) and tw.status == (0, 0, 0)


# ---- the inputs of the GPU cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CHAINS)
@pytest.mark.parametrize("path", cc.PATHS)
def test_gpu_inputs_are_well_posed(path, name):
    stages, rule = cc.chain(path, name)
    _, tw = cc.trajectory(path, name, np.float64)
    assert tw.applied == cc.NSTEPS and tw.nonfinite == 0
    # the input itself: the twin's fp32 run stays within a tenth of the GPU test's bar of its fp64 run, entry by entry (tests/test_gpu_seq.py
    # holds its inputs the same way) -- the sign-like first steps of Adam / RMSProp turn one cancelling gradient entry into lr of error
    t32, t64 = cc.trajectory(path, name, np.float32)[0], cc.trajectory(path, name, np.float64)[0]
    assert np.max(np.abs(t32.astype(np.float64) - t64)) <= 0.1 * 3e-5 * max(1.0, float(np.max(np.abs(t64))))
    cn = [s for s in stages if s[0] == "clipnorm"]
    if not cn:
        return
    omega = cn[0][1]
    rel = [abs(n - omega) / omega for n in tw.norms]
    print(path, name, "omega", omega, "norms", tw.norms, "clipped", tw.clipped)
    assert len(tw.norms) == cc.NSTEPS and min(rel) > 1e-3, (omega, tw.norms)
    assert 0 < tw.clipped < cc.NSTEPS, (omega, tw.norms)
    # the fp32 twin decides every step the same way
    _, tw32 = cc.trajectory(path, name, np.float32)
    assert tw32.status == tw.status
