"""Optimiser chains on the device (csrc/eh_chain.hpp) on the four step-kernel paths of tests/chain_cases.py: bitwise identities against
the unchained step, trajectories against the NumPy twin, the apply pass on the device's own gradient, reproducibility and the other
hosts of the step (epoch driver, graph capture, the local data-parallel group), steps that change nothing, and train()."""
import sys

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
from easyhybrid_jl_amd.engine import HybridEngine
import easyhybrid_jl_amd.train  # noqa: F401
from oracle import hybrid_oracle as ho

from tests import chain_cases as cc
from tests import util
from tests.chain_twin import ChainTwin

T = sys.modules["easyhybrid_jl_amd.train"]
pytestmark = pytest.mark.gpu
INF = float("inf")

_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _engine(path):
    """one engine per path for the whole module: every test sets parameters and optimiser anew"""
    if path not in _ENGINES:
        _ENGINES[path] = cc.make_engine(cc.case(path))
        _ENGINES[path].set_option("fused_update", 0)
    return _ENGINES[path]


def _state(eng):
    m, v, bt = eng.get_opt_state()
    return [eng.get_params(), m, v, np.asarray(bt)]


def _run(eng, c, nsteps, init):
    eng.set_params(c["theta"])
    init(eng)
    losses = [eng.train_step(*c["batches"][k]) for k in range(nsteps)]
    return _state(eng) + [np.asarray(losses, np.float32)]


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# ---- 1. bitwise identities ---------------------------------------------------------------------------------------------------------
IDENTITIES = {
    "rule_alone": [("rule",)],
    "clipnorm_1e30": [("clipnorm", 1e30, 2.0, True), ("rule",)],
    "clipgrad_1e30": [("clipgrad", 1e30), ("rule",)],
    "weightdecay_0": [("rule",), ("weightdecay", 0.0)],
}


LFORM_256 = [(0, 256), (256, 256), (128, 256), (0, 256), (256, 256)]


@pytest.mark.parametrize("path,rule", [(p, "Adam") for p in cc.PATHS] + [("seq", "RMSProp"), ("lform256", "Adam")])
def test_chains_that_do_nothing_leave_the_bits_of_the_plain_rule(path, rule):
    """five steps, fused_update = 0: theta, m, v, the running products and the losses are bit-equal to eh_opt_init's -- the chain form
    does not move existing arithmetic (the rule in the chain IS eh_opt_update_at; a factor of exactly 1, a clamp that never bites and
    + 0 * x change no bit).
    lform: at batch 64 (one slab row) the unchained step takes its weight-gradient products through the kernel that has the optimiser in
    its epilogue; the chained step takes the SAME products, its epilogue handed Descent(-1) on a zeroed gradbuf so
    that exactly the gradient is left there -- the slab path's products sum the 64 samples in another order (2.4e-6 in theta after five
    steps, measured).  lform256 (not one of the issue's cases): 256 samples per step, two slab rows, where both run the slab path."""
    c = dict(cc.case("lform"), batches=LFORM_256) if path == "lform256" else cc.case(path)
    eng = _engine("lform" if path == "lform256" else path)
    plain = _run(eng, c, 5, lambda e: e.opt_init(rule, 0.01))
    assert not eng.has_chain and np.isfinite(plain[0]).all() and not np.array_equal(plain[0], c["theta"])
    for name, stages in IDENTITIES.items():
        got = _run(eng, c, 5, lambda e: e.opt_init_chain(stages, rule, 0.01))
        print(path, rule, name, "max |difference| of theta, m, v, beta products, losses:", [float(np.max(np.abs(x.astype(np.float64) - y))) for x, y in zip(plain, got)])
        assert eng.has_chain and _same_bits(plain, got), (path, rule, name)
        assert eng.chain_status() == (5, 0, 0)
    eng.opt_init(rule, 0.01)                  # back to the unchained paths
    with pytest.raises(eh.EngineError):
        eng.chain_status()


# ---- 2. trajectories against the twin -----------------------------------------------------------------------------------------------
def _assert_close(path, got, ref):
    d = np.abs(got - ref)
    if path == "seq":            # the bar of tests/test_gpu_seq.py::test_three_rmsprop_steps
        print("  within 2e-5:", float(np.mean(d <= 2e-5)), "max", float(d.max()))
        assert np.mean(d <= 2e-5) >= 0.999 and d.max() <= 2.5e-3, (np.mean(d <= 2e-5), d.max())
    else:                        # the bar of tests/test_gpu_parity.py::test_other_optimiser_rules
        bar = 3e-5 * max(1.0, float(np.max(np.abs(ref))))
        print("  max |dtheta|", float(d.max()), "bar", bar, "entries over it", int((d > bar).sum()), "of", d.size)
        assert d.max() <= bar, (float(d.max()), bar, int((d > bar).sum()))


@pytest.mark.parametrize("name", cc.CHAINS)
@pytest.mark.parametrize("path", cc.PATHS)
def test_four_steps_against_the_twin(path, name):
    c, eng = cc.case(path), _engine(path)
    stages, rule = cc.chain(path, name)
    ref, tw = cc.trajectory(path, name, np.float32)
    eng.set_params(c["theta"])
    eng.opt_init_chain(stages, **rule)
    for k in range(cc.NSTEPS):
        eng.train_step(*c["batches"][k], want_loss=False)
    print(path, name, "status", eng.chain_status(), "twin", tw.status, "norms", tw.norms)
    assert eng.chain_status() == tw.status
    _assert_close(path, eng.get_params(), ref)


# ---- 3. the apply pass in isolation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2.0, 1.0, INF])
@pytest.mark.parametrize("path", cc.PATHS)
def test_one_clipped_descent_step_on_the_devices_own_gradient(path, p):
    """The device's gradient of the batch (loss_and_grad: the gradbuf the step reads), one chained Descent step, the step against the fp32
    twin fed that gradient.  The norm's rounding has no derivable bound: the fp32 twin is measured against its fp64 run on the same
    gradient, and the device gets ten times that deviation with a floor of 1e-6, relative to the largest entry of the step.
    Measured on an MI355X, max |d - d_ref| / max |d|: the device against the fp32 twin 0 for p = 2 and Inf on all four paths, 1.0e-7 to
    1.2e-7 for p = 1 on perwave, rowsplit and lform (the device sums in double), 0 on seq; the fp32 twin against its fp64 run 5.2e-8 to
    1.1e-7 (seq: 1.5e-7).  So the bound in force is the floor, 1e-6, except on seq (1.5e-6)."""
    c, eng = cc.case(path), _engine(path)
    a, n = c["batches"][0]
    eng.set_params(c["theta"])
    _, g, nv = eng.loss_and_grad(eh.EH_SPLIT_TRAIN, a, n)
    assert nv > 0
    eta = 0.05
    omega = float(np.float32(0.5 * _norm(g, p)))          # half the norm: the step clips
    stages = [("clipnorm", omega, p, True), ("rule",)]
    eng.opt_init_chain(stages, "Descent", eta)
    eng.train_step(a, n, want_loss=False)
    assert eng.chain_status() == (1, 1, 0)
    d_dev = c["theta"].astype(np.float64) - eng.get_params().astype(np.float64)
    d32 = c["theta"].astype(np.float64) - ChainTwin(g.size, stages, rule="Descent", lr=eta, dtype=np.float32).step(c["theta"], g).astype(np.float64)
    d64 = c["theta"].astype(np.float64) - ChainTwin(g.size, stages, rule="Descent", lr=eta, dtype=np.float64).step(c["theta"].astype(np.float64), g.astype(np.float64))
    scale = float(np.abs(d64).max())
    twin_dev = float(np.abs(d32 - d64).max()) / scale
    dev = float(np.abs(d_dev - d32).max()) / scale
    print(f"{path} p={p}: device against fp32 twin {dev:.2e}, fp32 twin against fp64 {twin_dev:.2e}")
    assert dev <= max(10.0 * twin_dev, 1e-6), (dev, twin_dev)


def _norm(g, p):
    a = np.abs(np.asarray(g, np.float64))
    return np.sqrt(np.sum(a * a)) if p == 2 else (np.sum(a) if p == 1 else a.max())


# ---- 4. reproducibility and the other hosts of the step -----------------------------------------------------------------------------
def _pw(name="clipnorm_adam"):
    c = cc.case("perwave")
    stages, rule = cc.chain("perwave", name)
    return c, stages, rule


def test_two_runs_give_equal_bits():
    c, stages, rule = _pw()
    eng = _engine("perwave")
    a = _run(eng, c, 4, lambda e: e.opt_init_chain(stages, **rule))
    b = _run(eng, c, 4, lambda e: e.opt_init_chain(stages, **rule))
    assert _same_bits(a, b)
    c2, eng2 = cc.case("lform"), _engine("lform")           # ... and so does the two-pass form (norm kernel + apply kernel)
    st2, r2 = cc.chain("lform", "clipnorm_adam")
    assert _same_bits(_run(eng2, c2, 3, lambda e: e.opt_init_chain(st2, **r2)), _run(eng2, c2, 3, lambda e: e.opt_init_chain(st2, **r2)))


def _mix32(x, k):
    M = 0xFFFFFFFF
    x ^= k; x = (x * 0x9E3779B1) & M; x ^= x >> 15; x = (x * 0x85EBCA77) & M; x ^= x >> 13; x = (x * 0xC2B2AE3D) & M; x ^= x >> 16
    return x


def _epoch_permutation(n, seed):
    """the keyed permutation eh_train_epoch draws on the device (csrc/eh_kernels.hpp eh_perm32), restated"""
    M = 0xFFFFFFFF
    bits = 1
    while (1 << bits) < n:
        bits += 1
    hb = max(1, (bits + 1) // 2)
    mask = (1 << hb) - 1
    out = np.empty(n, np.int32)
    for i in range(n):
        x = i
        while True:
            Lh, R = x >> hb, x & mask
            for r in range(4):
                k = (((seed >> (16 * (r & 1))) & M) + 0x632BE5AB * (r + 1) + ((seed >> 32) & M)) & M
                Lh, R = R, Lh ^ (_mix32(R, k) & mask)
            x = (Lh << hb) | R
            if x < n:
                break
        out[i] = x
    return out


def test_shuffled_epoch_equals_the_same_steps_one_by_one():
    c, stages, rule = _pw()
    eng = _engine("perwave")
    eng.set_params(c["theta"]); eng.opt_init_chain(stages, **rule)
    _, ns = eng.train_epoch(100, seed=11, shuffle=True)
    a = _state(eng) + [np.asarray(eng.chain_status())]
    perm = _epoch_permutation(512, 11)
    assert ns == 6 and sorted(perm) == list(range(512))
    eng.set_params(c["theta"]); eng.opt_init_chain(stages, **rule)
    for s in range(0, 512, 100):
        eng.train_step(s, min(100, 512 - s), want_loss=False, idx=perm)
    b = _state(eng) + [np.asarray(eng.chain_status())]
    assert _same_bits(a[:4], b[:4]) and np.array_equal(a[4], b[4]) and a[4][0] == 6


def test_a_captured_graph_of_two_chained_steps_replays_to_the_eager_bits():
    c, stages, rule = _pw()
    eng = _engine("perwave")
    eng.set_params(c["theta"]); eng.opt_init_chain(stages, **rule)
    for _ in range(2):
        for k in range(2):
            eng.train_step(*c["batches"][k], want_loss=False)
    eager = _state(eng) + [np.asarray(eng.chain_status())]
    eng.set_params(c["theta"]); eng.opt_init_chain(stages, **rule)
    eng.graph_begin()
    for k in range(2):
        eng.train_step(*c["batches"][k], want_loss=False)
    gid = eng.graph_end()
    eng.set_params(c["theta"]); eng.set_opt_state(np.zeros_like(c["theta"]), np.zeros_like(c["theta"]), np.asarray([0.9, 0.999], np.float32))
    eng.graph_launch(gid); eng.graph_launch(gid)
    eng.synchronize()
    assert _same_bits(eager[:4], _state(eng))
    eng.opt_init("Adam", 0.01)                # a graph recorded with a chain is not replayed without it
    with pytest.raises(eh.EngineError, match="optimiser chain"):
        eng.graph_launch(gid)


def test_two_handles_of_the_local_group_match_one_handle_on_the_whole_batch():
    """eh_comm_init_local / eh_dp_train_step_group on one GPU: eh_dp_apply takes the norm of the all-reduced, globally normalised
    gradient.  Tolerance: the unchained step's (tests/test_gpu_comm.py: 2e-6 absolute; replicas bit-identical)."""
    from easyhybrid_jl_amd import dp
    c, stages, rule = _pw()
    spec, theta, X, f, y = c["spec"], c["theta"], c["X"], c["f"], c["y"]
    engs = []
    for r in range(2):
        lo, hi = dp.shard_range(512, r, 2)
        e = util.load_engine(spec, theta, X[:, lo:hi], {k: v[lo:hi] for k, v in f.items()}, {k: v[lo:hi] for k, v in y.items()})
        e.opt_init_chain(stages, **rule)
        engs.append(e)
    HybridEngine.comm_init_local(engs)
    ref = util.load_engine(spec, theta, X, f, y)
    ref.opt_init_chain(stages, **rule)
    for s in range(4):
        a = s * 64
        loss = HybridEngine.dp_train_step_group(engs, [a, a], 64, want_loss=True)
        idx = np.concatenate([np.arange(r * 256 + a, r * 256 + a + 64) for r in range(2)]).astype(np.int32)
        assert loss == pytest.approx(ref.train_step(0, idx.size, idx=idx), rel=2e-6)
    th = [e.get_params() for e in engs]
    assert np.array_equal(th[0], th[1])
    assert np.max(np.abs(th[0] - ref.get_params())) <= 2e-6
    st = ref.chain_status()
    assert engs[0].chain_status() == st and engs[1].chain_status() == st and st[0] == 4 and 0 < st[1]
    for e in engs:
        e.set_option("fused_update", 2)
    with pytest.raises(NotImplementedError, match="optimiser chain"):
        engs[0].dp_fused_step(0, 64)
    engs[0].comm_destroy()
    for e in engs:
        e.close()
    ref.close()


def _twin_on_oracle(spec, theta, X, f, y, batches, stages, rule, l2=None):
    tw = ChainTwin(theta.size, stages, dtype=np.float32, **rule)
    th = theta.astype(np.float32)
    for a, n in batches:
        sl = slice(a, a + n)
        _, g, _ = ho.loss_and_grad(spec, th, X[:, sl], {k: v[sl] for k, v in f.items()}, {k: v[sl] for k, v in y.items()}, np.float32, l2=l2)
        th = tw.step(th, g.astype(np.float32))
    return th, tw


def _omega_between(spec, theta, X, f, y, batches, rule, l2=None):
    """as tests/chain_cases.py: from the twin's fp64 trajectory, so that some of the steps clip"""
    def run(omega):
        tw = ChainTwin(theta.size, [("clipnorm", omega, 2.0, True), ("rule",)], dtype=np.float64, **rule)
        th = theta.astype(np.float64)
        for a, n in batches:
            sl = slice(a, a + n)
            _, g, _ = ho.loss_and_grad(spec, th, X[:, sl], {k: v[sl] for k, v in f.items()}, {k: v[sl] for k, v in y.items()}, np.float64, l2=l2)
            th = tw.step(th, g)
        return tw
    return cc.tune_omega(run)


def test_two_targets_and_a_weight_l2_term_against_the_twin():
    rule = dict(rule="Adam", lr=0.01)
    # FluxPartModelQ10, two targets with their own masks: the per-target weights are in the gradient the chain reads
    rng = np.random.default_rng(0)
    B = 512
    X = rng.standard_normal((4, B)).astype(np.float32)
    f = {"SW_IN": rng.uniform(0, 800, B).astype(np.float32), "TA": rng.uniform(0, 30, B).astype(np.float32)}
    nee = rng.normal(-3, 4, B).astype(np.float32); gpp = rng.uniform(0, 12, B).astype(np.float32)
    nee[rng.random(B) < 0.2] = np.nan; gpp[rng.random(B) < 0.35] = np.nan
    y = {"NEE": nee, "GPP": gpp}
    spec = ho.HybridSpec(4, [16, 16], "fluxpart", {"RUE": (0.1, 0.0, 1.0), "Rb": (1.0, 0.0, 6.0), "Q10": (1.5, 1.0, 4.0)}, ["RUE", "Rb"], ["Q10"], ["NEE", "GPP"], "tanh", True)
    theta = ho.init_theta(spec, 2, np.float32)
    batches = [(a, 128) for a in range(0, 512, 128)]
    stages = [("clipnorm", _omega_between(spec, theta, X, f, y, batches, rule), 2.0, True), ("rule",)]
    eng = util.load_engine(spec, theta, X, f, y)
    eng.opt_init_chain(stages, **rule)
    for b in batches:
        eng.train_step(*b, want_loss=False)
    ref, tw = _twin_on_oracle(spec, theta, X, f, y, batches, stages, rule)
    print("two targets: status", eng.chain_status(), "twin", tw.status, tw.norms)
    assert eng.chain_status() == tw.status and 0 < tw.clipped < 4
    _assert_close("fluxpart", eng.get_params(), ref)
    eng.close()
    # weight_l2: the reduction has added 2 lambda w to the gradient before the norm is taken
    c = cc.case("perwave")
    l2 = (0.2, False)
    stages = [("clipnorm", _omega_between(c["spec"], c["theta"], c["X"], c["f"], c["y"], c["batches"][:4], rule, l2), 2.0, True), ("rule",)]
    eng = cc.make_engine(c)
    eng.set_weight_l2(*l2)
    eng.opt_init_chain(stages, **rule)
    for b in c["batches"][:4]:
        eng.train_step(*b, want_loss=False)
    ref, tw = _twin_on_oracle(c["spec"], c["theta"], c["X"], c["f"], c["y"], c["batches"][:4], stages, rule, l2)
    print("weight_l2: status", eng.chain_status(), "twin", tw.status, tw.norms)
    assert eng.chain_status() == tw.status and 0 < tw.clipped < 4
    _assert_close("perwave", eng.get_params(), ref)
    eng.close()


# ---- 5. steps that change nothing, and train() ---------------------------------------------------------------------------------------
def test_a_batch_without_a_valid_sample_changes_nothing():
    c, stages, rule = _pw()
    y = {k: v.copy() for k, v in c["y"].items()}
    y["reco"][128:256] = np.nan
    eng = util.load_engine(c["spec"], c["theta"], c["X"], c["f"], y)
    eng.opt_init_chain(stages, **rule)
    eng.train_step(0, 128)
    before = _state(eng) + [np.asarray(eng.chain_status())]
    assert np.isnan(eng.train_step(128, 128))
    after = _state(eng) + [np.asarray(eng.chain_status())]
    assert _same_bits(before[:4], after[:4]) and np.array_equal(before[4], after[4]) and after[4][0] == 1
    eng.train_step(256, 128)
    assert eng.chain_status()[0] == 2 and not np.array_equal(eng.get_params(), after[0])
    eng.close()


def _overflowing_case():
    """one forcing value of 1e30: Q10^(0.1 (ta - 15)) overflows -- an arithmetic overflow in a healthy kernel"""
    c = cc.case("perwave")
    f = {k: v.copy() for k, v in c["f"].items()}
    y = {k: v.copy() for k, v in c["y"].items()}
    f["ta"][130] = 1e30
    y["reco"][130] = 1.0
    return c, f, y


def test_a_non_finite_norm_is_counted_and_under_throw_not_applied():
    c, f, y = _overflowing_case()
    eng = util.load_engine(c["spec"], c["theta"], c["X"], f, y)
    for p in (2.0, 1.0, INF):
        eng.set_params(c["theta"])
        eng.opt_init_chain([("clipnorm", 1.0, p, True), ("rule",)], "Adam", 0.01)
        eng.train_step(0, 128)
        before = _state(eng)
        eng.train_step(128, 128)                     # its loss is whatever the overflow made of it: reported as computed
        st = eng.chain_status()
        assert _same_bits(before, _state(eng)) and (st[0], st[2]) == (1, 1), (p, st)
        eng.train_step(256, 128)
        st = eng.chain_status()
        assert (st[0], st[2]) == (2, 1) and np.isfinite(eng.get_params()).all()
    # throw = false: the arithmetic simply runs (a non-finite norm makes a factor of 0 or NaN; 0 * Inf is NaN)
    eng.set_params(c["theta"])
    eng.opt_init_chain([("clipnorm", 1.0, 2.0, False), ("rule",)], "Descent", 0.01)
    eng.train_step(128, 128)
    st = eng.chain_status()
    assert st[0] == 1 and st[2] == 1 and not np.isfinite(eng.get_params()).all()
    eng.close()


def _frame(c, f, y):
    cols = {"sw_pot": c["X"][0], "dsw_pot": c["X"][1], "ta": f["ta"], "reco": y["reco"]}
    return cols


def test_train_raises_on_a_non_finite_norm_under_throw():
    c, f, y = _overflowing_case()
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    kw = dict(nepochs=1, batchsize=128, random_seed=3, split_data_at=0.8, shuffleobs=False, loss_types=["mse"])
    with pytest.raises(FloatingPointError, match="gradient has 2-norm"):
        eh.train(model, _frame(c, f, y), opt=eh.OptimiserChain(eh.ClipNorm(1.0), eh.Adam(0.01)), **kw)
    res = eh.train(model, _frame(c, f, y), opt=eh.OptimiserChain(eh.ClipNorm(1.0, throw=False), eh.Adam(0.01)), **kw)
    assert res.chain_nonfinite == 1 and res.chain_applied >= 1
    with pytest.raises(NotImplementedError, match="norm of the whole"):
        eh.train(model, _frame(c, c["f"], c["y"]), opt=eh.OptimiserChain(eh.ClipNorm(1.0), eh.Adam(0.01)), fused_update=True, **kw)


def test_train_on_the_sequence_tutorial_with_clipnorm_and_rmsprop():
    c = cc.case("seq")
    data = {"x0": c["X"][0], "x1": c["X"][1], "ta": c["ta"], "reco": c["y"]}
    kw = dict(nepochs=2, batchsize=128, random_seed=5, loss_types=["mse"], opt=eh.OptimiserChain(eh.ClipNorm(1.0), eh.RMSProp(0.01)),
              sequence_kwargs=dict(input_window=10, output_window=1, output_shift=1, lead_time=1))
    a = eh.train(c["model"], data, **kw)
    b = eh.train(c["model"], data, **kw)
    assert np.array_equal(a.ps.view(np.uint32), b.ps.view(np.uint32))
    assert (a.chain_applied, a.chain_clipped, a.chain_nonfinite) == (b.chain_applied, b.chain_clipped, b.chain_nonfinite)
    assert a.chain_applied > 0 and 0 <= a.chain_clipped <= a.chain_applied and a.chain_nonfinite == 0
    assert a.train_history[-1]["mse"]["reco"] < a.train_history[0]["mse"]["reco"]
    plain = eh.train(c["model"], data, **dict(kw, opt=eh.RMSProp(0.01)))
    assert plain.chain_applied is None
