"""The lean form of the single-step train kernels (eh_lean_fold, csrc/eh_device.hpp): the step's run-time
switches decided at build time for handles inside its contract.  It is the same source with the branches decided, so every case here
asks for the SAME BITS -- parameters, both moments, the beta products, every step's loss -- from a handle that runs the lean kernel and
from the same configuration with `set_option("lean", 0)`: at the edges of the ordered form's group fold (two workgroups of which the
second holds one sample; 17 workgroups, so that group 0 has two rows and the others one, with a partial last tile; 32 workgroups, two
full rows per group), on a grid that changes every step and across a minibatch without a valid target; ordered step and step + reduce
pair, contiguous windows and a permutation, the kernels built ahead of time and one compiled at run time.  eh_jit_status says which
form ran.  Handles outside the contract keep the general kernel, whatever the option says.  (The eligibility test is a function of
the handle, which does not exist without a device: its cases are the second half of this file, each with the oracle's numbers.)"""
import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho
from tests import util

pytestmark = pytest.mark.gpu

TOL = 1e-5                    # the suite's bar against the fp32 oracle (tests/test_gpu_parity.py)
N = 3 * 4349                  # samples of the shared data set: every window below fits, three disjoint windows of 4 349
STEPS = 6
SHAPES = {
    "b257": [(0, 257)] * STEPS,
    "b4349": [(0, 4349), (4349, 4349), (8698, 4349)] * 2,
    "b8192": [(0, 8192), (4000, 8192)] * 3,
    "grid_changes": [(0, 257), (300, 4349), (5000, 257), (4349, 4349), (9000, 257), (8698, 4349)],
    "nan_middle": [(0, 4349), (4349, 4349), (8698, 4349), (4349, 4349), (100, 257), (8698, 4349)],      # the window at 4 349: no valid target
}
_CASE = {}


def _case(shape, perm):
    """(spec, theta, X, f, y, idx): the headline model on the shared data set; `nan_middle` blanks the targets its middle window reads"""
    key = (shape == "nan_middle", perm)
    if key not in _CASE:
        spec, theta, X, f, y = util.rbq10_case(N, "tanh", True, 0.05)
        idx = np.random.default_rng(7).permutation(N).astype(np.int32) if perm else None
        if key[0]:
            y = {k: v.copy() for k, v in y.items()}
            rows = idx[4349:8698] if perm else np.arange(4349, 8698)
            for v in y.values():
                v[rows] = np.nan
        _CASE[key] = (spec, theta, X, f, y, idx)
    return _CASE[key]


def _engine(case, fused, kernels, lean, prepare=None):
    spec, theta, X, f, y, _ = case
    e = util.load_engine(spec, theta, X, f, y, engine=util.model_from_spec(spec).engine())
    e.set_option("aot_spec", int(kernels == "aot"))
    e.set_option("specialize", int(kernels == "jit"))
    (prepare or (lambda eng: eng.opt_init("Adam", 0.01)))(e)
    e.set_option("fused_update", fused)
    e.set_option("lean", lean)
    return e


def _run(e, windows, idx):
    losses = [e.train_step(a, c, idx=idx) for a, c in windows]
    e.synchronize()
    m, v, bt = e.get_opt_state()
    out = [np.asarray(losses, np.float32), e.get_params().copy(), m.copy(), v.copy(), np.asarray(bt).copy()]
    n, log = e.jit_status()
    e.close()
    return out, n, log


def _same(a, b):
    for name, u, w in zip(("losses", "params", "adam_m", "adam_v", "beta products"), a, b):
        assert np.array_equal(u, w, equal_nan=True), name


@pytest.mark.parametrize("kernels", ["aot", "jit"])
@pytest.mark.parametrize("perm", [False, True], ids=["contiguous", "permuted"])
@pytest.mark.parametrize("fused", [2, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_lean_kernel_gives_the_general_kernels_bits(shape, fused, perm, kernels):
    case = _case(shape, perm)
    got, n1, log1 = _run(_engine(case, fused, kernels, 1), SHAPES[shape], case[5])
    ref, n0, log0 = _run(_engine(case, fused, kernels, 0), SHAPES[shape], case[5])
    assert "train step kernel: lean" in log1 and "train step kernel: general" in log0, (log1[-200:], log0[-200:])
    assert n1 >= 1 and n0 >= 1 and log1.startswith("ahead-of-time") == (kernels == "aot") and log0.startswith("ahead-of-time") == (kernels == "aot")
    assert np.all(np.isfinite(ref[1])) and np.isnan(ref[0]).sum() == (2 if shape == "nan_middle" else 0)
    _same(ref, got)


@pytest.mark.parametrize("shape", ["b257", "grid_changes", "nan_middle"])
def test_lean_steps_against_the_oracle(shape):
    """the lean ordered step on contiguous windows against the fp32 oracle's Adam, to the suite's bar"""
    case = _case(shape, False)
    spec, theta, X, f, y, _ = case
    got, _, log = _run(_engine(case, 2, "aot", 1), SHAPES[shape], None)
    assert "train step kernel: lean" in log
    th_ref, l_ref = ho.train_steps(spec, theta, X, f, y, SHAPES[shape], dtype=np.float32)
    assert util.relerr(got[1], th_ref) <= TOL
    l_ref = np.asarray(l_ref, np.float64)
    ok = np.isfinite(l_ref)
    assert np.array_equal(np.isnan(got[0]), ~ok) and np.all(np.abs(got[0][ok] - l_ref[ok]) <= TOL * np.abs(l_ref[ok]))


# ---- handles outside the contract: the general kernel, whatever "lean" says ---------------------------------------------------
# rules[k] = opt_init's keyword arguments; element i of theta follows rules[group[i]] (one rule: one group)
OUTSIDE = {
    "AdamW": [dict(rule="AdamW", lr=0.01, weight_decay=0.01)],
    "RMSProp": [dict(rule="RMSProp", lr=0.01)],
    "Descent": [dict(rule="Descent", lr=0.01)],
    "per_branch_opt": [dict(rule="Adam", lr=0.01), dict(rule="Adam", lr=0.005)],      # the last element of theta (Q10) on the second rule
}
WIN = [(0, 4349), (4349, 257), (8698, 4349), (300, 4349)]
_RULE_REF = {}


def _group_of(n, rules):
    group = np.zeros(n, np.int32)
    if len(rules) > 1:
        group[-1:] = 1
    return group


def _rule_reference(what):
    """theta after WIN from the oracle's fp32 gradient and Optimisers.jl's rules op for op (ho.adam_step covers Adam and AdamW; RMSProp
    and Descent as tests/test_gpu_opt_branches.py writes them), every group with its own state; computed once per rule"""
    if what not in _RULE_REF:
        spec, theta, X, f, y, _ = _case("b4349", False)
        rules = OUTSIDE[what]
        th = theta.astype(np.float32).copy()
        group = _group_of(th.size, rules)
        st = [ho.adam_init(int((group == k).sum())) for k in range(len(rules))]
        vq = [np.zeros(int((group == k).sum()), np.float32) for k in range(len(rules))]
        for a, n in WIN:
            sl = slice(a, a + n)
            _, g, _ = ho.loss_and_grad(spec, th, X[:, sl], {k: v[sl] for k, v in f.items()}, {k: v[sl] for k, v in y.items()}, np.float32)
            g = g.astype(np.float32)
            for k, r in enumerate(rules):
                m, lr = group == k, np.float32(r["lr"])
                if r["rule"] == "Descent":
                    th[m] = th[m] - lr * g[m]
                elif r["rule"] == "RMSProp":
                    vq[k] = np.float32(0.9) * vq[k] + (np.float32(1) - np.float32(0.9)) * g[m] * g[m]
                    th[m] = th[m] - g[m] * (lr / (np.sqrt(vq[k]) + np.float32(1e-8)))
                else:
                    th[m] = ho.adam_step(th[m], g[m], st[k], lr=r["lr"], weight_decay=r.get("weight_decay", 0.0))
        _RULE_REF[what] = th
    return _RULE_REF[what]


def _prepare(what):
    rules = OUTSIDE[what]
    if len(rules) == 1:
        r = dict(rules[0])
        return lambda e: e.opt_init(r.pop("rule"), **r)
    return lambda e: e.opt_init_groups(_group_of(e.n_theta, rules), rules)


@pytest.mark.parametrize("fused", [2, 0])
@pytest.mark.parametrize("what", list(OUTSIDE))
def test_handles_outside_the_contract_run_the_general_kernel(what, fused):
    """another rule than Adam, or a rule per branch: the general kernel with the option on (eh_jit_status), the oracle's parameters
    to the suite's bar, and the same bits with the option off"""
    case = _case("b4349", False)
    got, _, log1 = _run(_engine(case, fused, "aot", 1, _prepare(what)), WIN, None)
    assert "train step kernel: general" in log1 and "train step kernel: lean" not in log1, (what, log1[-200:])
    ref = _rule_reference(what)
    assert np.max(np.abs(got[1] - ref)) <= TOL * max(1.0, float(np.max(np.abs(ref)))), (what, np.max(np.abs(got[1] - ref)))
    off, _, log0 = _run(_engine(case, fused, "aot", 0, _prepare(what)), WIN, None)
    assert "train step kernel: lean" not in log0
    _same(off, got)


@pytest.mark.parametrize("fused", [2, 0])
def test_handle_with_dropout_runs_the_general_kernel(fused):
    """dropout exists in run-time compiled train + eval kernels only: no lean form is built for them, the option changes nothing
    (the masks against their twin: tests/test_gpu_dropout.py)"""
    case = _case("b4349", False)

    def prepare(e):
        e.opt_init("Adam", 0.01)
        e.set_dropout([0.25, 0.1], seed=5)
    got, _, log1 = _run(_engine(case, fused, "jit", 1, prepare), WIN, None)
    off, _, log0 = _run(_engine(case, fused, "jit", 0, prepare), WIN, None)
    assert "train step kernel: general" in log1 and "train step kernel: lean" not in log1 and "train step kernel: lean" not in log0
    assert np.all(np.isfinite(got[1])) and not np.array_equal(got[1], case[1])
    _same(off, got)


def _check_oracle(spec, theta, X, f, y, windows, prepare_spec_kw, fused):
    out = []
    for lean in (1, 0):
        e = util.load_engine(spec, theta, X, f, y, engine=util.model_from_spec(spec).engine())
        e.set_option("aot_spec", 1)
        e.opt_init("Adam", 0.01)
        e.set_option("fused_update", fused)
        e.set_option("lean", lean)
        res, _, log = _run(e, windows, None)
        assert "train step kernel: lean" not in log and "train step kernel: general" in log, log[-200:]
        out.append(res)
    _same(out[1], out[0])
    th_ref, l_ref = ho.train_steps(spec, theta, X, f, y, windows, dtype=np.float32, **prepare_spec_kw)
    assert util.relerr(out[0][1], th_ref) <= TOL
    assert np.all(np.abs(out[0][0] - np.asarray(l_ref)) <= TOL * np.abs(np.asarray(l_ref)))


@pytest.mark.parametrize("fused", [1, 0])
def test_input_batchnorm_in_train_mode_stays_on_the_general_kernel(fused):
    spec = ho.rbq10_spec((16, 16), "tanh", True)
    spec.input_batchnorm = True
    X, f, y = ho.make_synth_rbq10(4096, 11, 0.1)           # raw predictors: what the normalisation is for
    theta = ho.init_theta(spec, 3, np.float32)
    _check_oracle(spec, theta, X, f, y, [(i * 1024, 1024) for i in range(4)], dict(bn_state=ho.bn_init(spec)), fused)


@pytest.mark.parametrize("fused", [1, 0])
def test_two_target_model_stays_on_the_general_kernel(fused):
    rng = np.random.default_rng(12)
    B = 4096
    pars = {"RUE": (0.1, 0.0, 1.0), "Rb": (1.0, 0.0, 6.0), "Q10": (1.5, 1.0, 4.0)}
    spec = ho.HybridSpec(2, [16, 16], "fluxpart", pars, ["RUE"], ["Rb", "Q10"], ["NEE", "GPP"], "tanh", True)
    X = rng.standard_normal((2, B)).astype(np.float32)
    f = {"SW_IN": (rng.random(B) * 400).astype(np.float32), "TA": (rng.random(B) * 30).astype(np.float32)}
    y = {"NEE": rng.standard_normal(B).astype(np.float32), "GPP": (rng.random(B) * 30).astype(np.float32)}
    y["NEE"][rng.random(B) < 0.3] = np.nan; y["GPP"][rng.random(B) < 0.1] = np.nan
    theta = ho.init_theta(spec, 1, np.float32)
    _check_oracle(spec, theta, X, f, y, [(i * 1024, 1024) for i in range(4)], {}, fused)


def test_multi_step_launch_at_batch_64_is_not_a_lean_launch():
    """an epoch of minibatches of 64 runs several steps per launch on the multi-step kernel: no lean form of it exists, and the option
    changes nothing"""
    spec, theta, X, f, y = util.rbq10_case(1024, "tanh", True, 0.05)
    out = []
    for lean in (1, 0):
        e = util.load_engine(spec, theta, X, f, y, engine=util.model_from_spec(spec).engine())
        e.set_option("aot_spec", 1)
        e.opt_init("Adam", 0.01)
        e.set_option("fused_update", 2)
        e.set_option("lean", lean)
        loss, nsteps = e.train_epoch(64, seed=3, shuffle=True)
        assert nsteps == 16
        e.synchronize()
        m, v, bt = e.get_opt_state()
        _, log = e.jit_status()
        assert "train step kernel: lean" not in log, log[-200:]
        out.append([np.float32(loss), e.get_params().copy(), m.copy(), v.copy(), np.asarray(bt).copy()])
        e.close()
    assert np.all(np.isfinite(out[0][1])) and not np.array_equal(out[0][1], theta)
    _same(out[1], out[0])


def test_option_and_diagnostics_move_a_handle_in_and_out_of_the_contract():
    """eligibility follows the configuration: Adam -> lean; AdamW on the same handle -> general; Adam again -> lean; "lean" 0 -> general;
    "lean" 1 -> lean; the diagnostics buffer armed (eh_debug_stamps) -> general for good"""
    import ctypes as C
    case = _case("b257", False)
    e = _engine(case, 2, "aot", 1)
    seen = []
    buf = (C.c_uint64 * 32)()
    for step in (lambda: None, lambda: e.opt_init("AdamW", 0.01, weight_decay=0.01), lambda: e.opt_init("Adam", 0.01), lambda: e.set_option("lean", 0),
                 lambda: e.set_option("lean", 1), lambda: e._lib.eh_debug_stamps(e._h, buf, 32)):
        step()
        e.train_step(0, 4349)
        seen.append("lean" if "train step kernel: lean" in e.jit_status()[1] else "general")
    e.close()
    assert seen == ["lean", "general", "lean", "general", "lean", "general"]
