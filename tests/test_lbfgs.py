"""L-BFGS (the reference's Optimization.jl driver) without a GPU: the NumPy twin the device is held against
(tests/lbfgs_twin.py) minimises and is stable in fp32, the decision and recursion code the device runs agrees with it when it is run
on the host (eh_lbfgs_host_decide), and the host-side bookkeeping of train(opt = LBFGS())."""
import ctypes as C
import warnings

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
from oracle import hybrid_oracle as ho

from tests import lbfgs_twin as tw
from tests import util

PARAMS = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}
# the trajectory bar of tests/test_gpu_parity.py, relative to max(1, max |theta_ref|)
GPU_BAR = 3e-5


def case(k):
    """the two cases the device is run on (tests/test_gpu_lbfgs.py): (spec, theta, X, forcings, targets)"""
    if k == 1:
        return util.rbq10_case(512, act="tanh", scale=True, nan_frac=0.1)
    return util.rbq10_case(300, act="sigmoid", scale=True, nan_frac=0.1, hidden=(8,))


def oracle_fg(c):
    spec, _, X, f, y = c

    def fg(x):
        l, g, nv = ho.loss_and_grad(spec, np.asarray(x, np.float64), X, f, y)
        return l, g, float(sum(nv))
    return fg


@pytest.fixture(scope="module")
def runs():
    """twin runs shared by the tests: (case, iterations, dtype name) -> Result"""
    out = {}
    for k in (1, 2):
        c = case(k)
        fg = oracle_fg(c)
        for it in (5, 10, 30) if k == 1 else (5, 10):
            out[k, it, "f64"] = tw.lbfgs(fg, c[1], it)
            out[k, it, "f32"] = tw.lbfgs(fg, c[1], it, dtype=np.float32)
    return out


def test_twin_minimises(runs):
    r = runs[1, 30, "f64"]
    fs = [t["f"] for t in r.trace]
    f_start = oracle_fg(case(1))(case(1)[1])[0]
    print(f"twin: {f_start:.4f} -> {r.f:.5f} in {r.evaluations} evaluations, {r.iterations} iterations")
    assert r.iterations == 30 and r.status == "maxiters"
    assert fs[0] < f_start and all(b <= a for a, b in zip(fs, fs[1:]))
    assert all(t["sy"] > 0 for t in r.trace)
    assert r.evaluations <= 30 * 20 + 1
    so = pytest.importorskip("scipy.optimize")
    c = case(1)
    fg = oracle_fg(c)
    res = so.minimize(lambda x: fg(x)[:2], c[1].astype(np.float64), jac=True, method="L-BFGS-B", options=dict(maxiter=30, maxcor=10, gtol=1e-5, ftol=0.0))
    print(f"scipy L-BFGS-B: {res.fun:.5f} in {res.nfev} evaluations")
    assert r.f <= 1.05 * res.fun


def test_twin_fp32_takes_the_same_decisions(runs):
    for k in (1, 2):
        a, b = runs[k, 10, "f64"], runs[k, 10, "f32"]
        assert [(t["decisions"], t["trials"]) for t in a.trace] == [(t["decisions"], t["trials"]) for t in b.trace]
        for it in (5, 10):
            a, b = runs[k, it, "f64"], runs[k, it, "f32"]
            print(f"case {k}, {it} iterations: max |theta32 - theta64| / max |theta64| = {np.abs(b.theta - a.theta).max() / np.abs(a.theta).max():.2e}")
        a, b = runs[k, 5, "f64"], runs[k, 5, "f32"]
        assert np.abs(b.theta - a.theta).max() <= 0.1 * GPU_BAR * max(1.0, np.abs(a.theta).max())
    assert "A" in runs[1, 5, "f64"].trace[2]["decisions"]           # the backtracking branch is on the path the device is run on


class HostDecide:
    """eh_lbfgs_host_decide with the state and the Gram matrix it keeps"""

    def __init__(self, maxiters, m=10, c1=1e-4, c2=0.9, max_linesearch=20, g_tol=1e-5, f_reltol=0.0, initial_step=0.0):
        self.o = L.LbfgsOpts(m, max_linesearch, c1, c2, g_tol, f_reltol, initial_step)
        self.m, self.maxiters = m, maxiters
        self.state = np.zeros(L.EH_LBFGS_STATE_DOUBLES)
        self.gram = np.zeros(L.EH_LBFGS_GRAM_DIM ** 2)
        self.rows = []

    def __call__(self, sums, f, n_valid=1.0):
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        q = np.zeros(8 + 6 * self.m)
        q[:len(sums)] = sums
        rec, row, wrote = np.zeros(L.EH_LBFGS_RECORD_DOUBLES), np.zeros(8), C.c_int32()
        st = L.lib().eh_lbfgs_host_decide(C.byref(self.o), self.maxiters, dp(self.state), dp(self.gram), dp(q), float(f), float(n_valid), dp(rec), dp(row), C.byref(wrote))
        assert st == L.EH_OK
        if wrote.value:
            self.rows.append(row)
        return dict(action=int(rec[0]), t=rec[1], slot=int(rec[2]), npairs=int(rec[3]), coef=rec[4:4 + 2 * self.m + 1].copy())

    @property
    def done(self):
        return int(self.state[0])


MOVES = (tw.REJECT, tw.ACCEPT, tw.RESTART, tw.ACCEPT_PAUSE)      # the actions whose t is the next trial's step


def follow(k, iters, **kw):
    """the host-side run of the device's decision code, fed the twin's own numbers along case k"""
    hd = HostDecide(iters, **kw)
    seen = []

    def observe(ev):
        got = hd(ev["sums"], ev["f"], ev["n_valid"])
        seen.append(ev["action"])
        assert got["action"] == ev["action"]
        if ev["action"] in MOVES:
            assert got["t"] == pytest.approx(ev["t"], rel=1e-12)
        if ev["action"] in (tw.ACCEPT, tw.ACCEPT_PAUSE):
            assert got["slot"] == ev["slot"] and got["npairs"] == ev["npairs"]
            assert np.abs(got["coef"] - ev["coef"]).max() <= 1e-12 * np.abs(ev["coef"]).max()
    c = case(k)
    r = tw.lbfgs(oracle_fg(c), c[1], iters, observe=observe, **kw)
    return r, hd, seen


def test_host_decide_follows_the_twin():
    r, hd, seen = follow(1, 30)
    assert len(hd.rows) == 30 and hd.done == 3 and r.status == "maxiters"
    assert seen.count(tw.REJECT) == r.evaluations - 31
    for row, t in zip(hd.rows, r.trace):
        assert row[0] == pytest.approx(t["f"], rel=1e-12) and row[1] == pytest.approx(t["t"], rel=1e-12) and int(row[2]) == t["trials"]
        assert eh.engine.lbfgs_trace_row(row)["decisions"] == t["decisions"] and int(row[7]) == t["evaluations"]
    # the expansion branch: four curvature rejections double t from 1e-4 to 0.0016
    r, hd, _ = follow(1, 6, initial_step=1e-4)
    assert r.trace[0]["decisions"] == "CCCC" and r.trace[0]["t"] == pytest.approx(0.0016, rel=1e-12)
    assert eh.engine.lbfgs_trace_row(hd.rows[0])["decisions"] == "CCCC" and hd.rows[0][1] == pytest.approx(0.0016, rel=1e-12)
    # a shorter history than the run: the ring wraps
    follow(2, 10, m=3)


def start(hd, gg=4.0, f=10.0):
    """the evaluation at the starting point: d = -g, t = min(1, 1 / ||g||)"""
    got = hd([0, 0, 0, 1.0, gg, 0, 0, 0], f)
    assert got["action"] == tw.ACCEPT and got["t"] == pytest.approx(min(1.0, gg ** -0.5)) and got["coef"][2 * hd.m] == -1.0
    return got["t"]


def test_host_decide_by_hand():
    # a loss that is not finite is a failed sufficient-decrease test: the bracket closes from above
    hd = HostDecide(5)
    t = start(hd)
    for bad in (float("nan"), float("inf")):
        got = hd([-1.0, 0, 0, 1.0, 4.0, 0, 0, 0], bad)
        assert got["action"] == tw.REJECT and got["t"] == pytest.approx(t / 2)
        t = got["t"]
    # a pair without curvature (s.y <= 1e-10 y.y) is accepted as an iterate and not stored: the next direction is -g again
    hd = HostDecide(5)
    start(hd)
    got = hd([-0.1, 1e-11, 1.0, 1.0, 4.0, 1.0, 0, 0], 9.0)
    assert got["action"] == tw.ACCEPT and got["slot"] == -1 and got["npairs"] == 0 and got["t"] == 1.0
    assert got["coef"][2 * hd.m] == -1.0 and not got["coef"][:2 * hd.m].any()
    got = hd([-0.1, 0.5, 1.0, 1.0, 4.0, 1.0, -0.2, 0.3], 8.0)           # ... and one with curvature is
    assert got["action"] == tw.ACCEPT and got["slot"] == 0 and got["npairs"] == 1
    # H0 = s.y / y.y = 0.5 and one pair: d = -(0.5 (g - a y) + (a - b) s) with a = s.g / s.y, b = y.(0.5 (g - a y)) / s.y
    a = -0.2 / 0.5
    b = (0.5 * (0.3 - a * 1.0)) / 0.5
    assert got["coef"][2 * hd.m] == pytest.approx(-0.5) and got["coef"][hd.m] == pytest.approx(0.5 * a) and got["coef"][0] == pytest.approx(-(a - b))
    # twenty rejections: the history is dropped and the search starts once more from -g0; twenty more end the solve at x0
    hd = HostDecide(5)
    t0 = start(hd)
    for k in range(19):
        assert hd([-1.0, 0, 0, 1.0, 4.0, 0, 0, 0], 11.0)["action"] == tw.REJECT
    got = hd([-1.0, 0, 0, 1.0, 4.0, 0, 0, 0], 11.0)
    assert got["action"] == tw.RESTART and got["t"] == pytest.approx(t0) and got["coef"][2 * hd.m] == -1.0 and hd.done == 0
    for k in range(19):
        assert hd([-1.0, 0, 0, 1.0, 4.0, 0, 0, 0], 11.0)["action"] == tw.REJECT
    assert hd([-1.0, 0, 0, 1.0, 4.0, 0, 0, 0], 11.0)["action"] == tw.FAIL_DONE and hd.done == 4
    evals = hd.state[3]
    assert hd([-1.0, 0, 0, 1.0, 4.0, 0, 0, 0], 1.0)["action"] == tw.NOOP and hd.state[3] == evals      # done: nothing changes
    # a batch without a valid target: "empty batch", nothing moves
    hd = HostDecide(5)
    assert hd([0] * 8, float("nan"), 0.0)["action"] == tw.NOOP and hd.done == 5
    # a gradient below g_tol at the start: converged before the first iteration; maxiters = 0: stopped there
    hd = HostDecide(5)
    assert hd([0, 0, 0, 1e-6, 1e-12, 0, 0, 0], 1.0)["action"] == tw.ACCEPT_DONE and hd.done == 1
    hd = HostDecide(0)
    assert hd([0, 0, 0, 1.0, 4.0, 0, 0, 0], 1.0)["action"] == tw.ACCEPT_PAUSE and hd.done == 3


def model(**kw):
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, PARAMS, ["rb"], ["Q10"], **kw)


def test_train_config_and_refusals():
    tc = eh.TrainConfig()
    assert (tc.full_batch, tc.promote_f64, tc.eval_every, tc.inner_maxiters) == (False, False, 1, 4)
    o = eh.LBFGS()
    assert (o.m, o.c1, o.c2, o.max_linesearch, o.initial_step) == (10, 1e-4, 0.9, 20, 0.0)
    with pytest.raises(TypeError, match="tolerance"):                      # not a solve keyword of this driver
        eh.train(model(), {}, opt=eh.LBFGS(), tolerance=1.0)
    for k in ("maxiters", "epochs", "g_tol", "f_reltol"):                  # ... and none of them is a keyword with an Optimisers rule
        with pytest.raises(TypeError, match=k):
            eh.train(model(), {}, **{k: 1})
    with pytest.raises(NotImplementedError, match="chain"):
        eh.train(model(), {}, opt=eh.OptimiserChain(eh.ClipGrad(1.0), eh.LBFGS()))
    with pytest.raises(NotImplementedError, match="per-branch"):
        eh.train(model(), {}, opt={"ps": eh.LBFGS()})
    with pytest.raises(NotImplementedError, match="distributed"):
        eh.train(model(), {}, opt=eh.LBFGS(), distributed=True)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        eh.train(model(input_batchnorm=True), {}, opt=eh.LBFGS())
    drop = model(hidden_layers=eh.Chain(eh.Dense(2, 8, "tanh"), eh.Dropout(0.2), eh.Dense(8, 8, "tanh")))
    with pytest.raises(NotImplementedError, match="Dropout"):
        eh.train(drop, {}, opt=eh.LBFGS())
    for bad in (dict(m=0), dict(m=17), dict(c1=0.0), dict(c1=0.95), dict(c2=1.0), dict(max_linesearch=0), dict(max_linesearch=49), dict(initial_step=-1.0)):
        with pytest.raises(ValueError):
            eh.train(model(), {}, opt=eh.LBFGS(**bad))
    with pytest.raises(ValueError):
        eh.train(model(), {}, opt=eh.LBFGS(), eval_every=0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(Exception):                                      # (the empty table fails afterwards; the warning is what is checked)
            eh.train(model(), {}, opt=eh.LBFGS(), promote_f64=True)
    assert len([x for x in w if "promote_f64" in str(x.message)]) == 1


def test_abi_null_handle_and_option_ranges():
    lib = L.lib()
    o = L.LbfgsOpts(10, 20, 1e-4, 0.9, 1e-5, 0.0, 0.0)
    st, n = L.LbfgsStat(), C.c_int64()
    assert lib.eh_lbfgs_init(None, C.byref(o)) == L.EH_EINVAL
    assert lib.eh_lbfgs_set_batch(None, 0, None, 0, 0, 0) == L.EH_EINVAL
    assert lib.eh_lbfgs_set_maxiters(None, 1) == L.EH_EINVAL
    assert lib.eh_lbfgs_run(None, 1) == L.EH_EINVAL
    assert lib.eh_lbfgs_status(None, C.byref(st)) == L.EH_EINVAL
    assert lib.eh_lbfgs_trace(None, None, 0, C.byref(n)) == L.EH_EINVAL
    assert lib.eh_version() == 4
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    bufs = [np.zeros(k) for k in (L.EH_LBFGS_STATE_DOUBLES, L.EH_LBFGS_GRAM_DIM ** 2, 8 + 6 * 16, L.EH_LBFGS_RECORD_DOUBLES, 8)]
    args = lambda oo: (C.byref(oo), 5, dp(bufs[0]), dp(bufs[1]), dp(bufs[2]), 1.0, 1.0, dp(bufs[3]), dp(bufs[4]), None)
    assert lib.eh_lbfgs_host_decide(None, 5, dp(bufs[0]), dp(bufs[1]), dp(bufs[2]), 1.0, 1.0, dp(bufs[3]), dp(bufs[4]), None) == L.EH_EINVAL
    for m, ls in ((0, 20), (17, 20), (10, 0), (10, 49)):
        assert lib.eh_lbfgs_host_decide(*args(L.LbfgsOpts(m, ls, 1e-4, 0.9, 1e-5, 0.0, 0.0))) == L.EH_EINVAL
    assert not bufs[0].any()
    assert lib.eh_lbfgs_host_decide(*args(L.LbfgsOpts(16, 48, 1e-4, 0.9, 1e-5, 0.0, 0.0))) == L.EH_OK
