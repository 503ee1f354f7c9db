"""Per-branch optimiser rules on the device (eh_opt_init_groups; TrainConfig.opt as a dict / NamedTuple, the reference's
build_opt_state, src/training/train.jl:78-93): every kernel family and step mode against the fp32 oracle with each branch's slice
updated by its own rule, plus exact invariants (two groups of one rule == that rule; a Descent(0) branch never moves), state round
trips, a local data-parallel group and the train() front door."""
import sys

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
import easyhybrid_jl_amd.train  # noqa: F401
from easyhybrid_jl_amd.engine import HybridEngine
from oracle import hybrid_oracle as ho
from tests import util

T = sys.modules["easyhybrid_jl_amd.train"]
pytestmark = pytest.mark.gpu
TOL = 3e-5


def _rules(model, opt):
    group, rules = T._opt_groups(opt, model)
    assert group is not None
    return group, rules


def _reference(spec, theta, X, f, y, windows, group, rules):
    """the oracle's fp32 gradient; each group's slice through its own rule and its own step count"""
    th = theta.astype(np.float32).copy()
    st = [ho.adam_init(int((group == k).sum())) for k in range(len(rules))]
    vq = [np.zeros(int((group == k).sum()), np.float32) for k in range(len(rules))]
    for a, n in windows:
        sl = slice(a, a + n)
        _, g, nv = ho.loss_and_grad(spec, th, X[:, sl], {k: v[sl] for k, v in f.items()}, {k: v[sl] for k, v in y.items()}, np.float32)
        if sum(nv) == 0:
            continue
        g = g.astype(np.float32)
        for k, r in enumerate(rules):
            m = group == k
            lr = np.float32(r["lr"])
            if r["rule"] == "Descent":
                th[m] = th[m] - lr * g[m]
            elif r["rule"] == "RMSProp":
                rho = np.float32(r.get("beta1", 0.9))
                vq[k] = rho * vq[k] + (np.float32(1) - rho) * g[m] * g[m]
                th[m] = th[m] - g[m] * (lr / (np.sqrt(vq[k]) + np.float32(r.get("eps", 1e-8))))
            else:
                th[m] = ho.adam_step(th[m], g[m], st[k], lr=r["lr"], b1=r.get("beta1", 0.9), b2=r.get("beta2", 0.999),
                                     eps=r.get("eps", 1e-8), weight_decay=r.get("weight_decay", 0.0))
    return th


def _close(got, ref):
    assert np.max(np.abs(got - ref)) <= TOL * max(1.0, float(np.max(np.abs(ref)))), np.max(np.abs(got - ref))


HEADLINE_OPT = {"ps": T.Adam(1e-2), "Q10": T.Descent(5e-2)}


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("aot,specialize", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_headline_shape_every_step_mode(fused, aot, specialize):
    spec, theta, X, f, y = util.rbq10_case(2048, "tanh", True, 0.1)
    model = util.model_from_spec(spec)
    group, rules = _rules(model, HEADLINE_OPT)
    eng = util.load_engine(spec, theta, X, f, y, engine=model.engine())
    eng.set_option("aot_spec", aot)
    if specialize:
        eng.set_option("specialize", 1)
    eng.set_option("fused_update", fused)
    eng.opt_init_groups(group, rules)
    windows = [(a, 512) for a in (0, 512, 1024, 1536, 0, 1024)]
    for a, n in windows:
        eng.train_step(a, n)
    ref = _reference(spec, theta, X, f, y, windows, group, rules)
    _close(eng.get_params(), ref)
    _, _, bt = eng.get_opt_state()
    assert bt.shape == (2, 2)
    assert bt[0, 0] == pytest.approx(0.9 ** 7, rel=1e-5) and bt[1, 0] == pytest.approx(0.9 ** 7, rel=1e-5)
    eng.close()


def _epoch_case(hidden, B, batch, act="tanh"):
    spec, theta, X, f, y = util.rbq10_case(B, act, True, 0.1, hidden=hidden)
    model = util.model_from_spec(spec)
    group, rules = _rules(model, {"ps": T.Adam(3e-3), "Q10": T.RMSProp(2e-2)})
    return spec, theta, X, f, y, model, group, rules


@pytest.mark.parametrize("fused,multi", [(0, 0), (1, 1), (2, 1)])
def test_one_workgroup_multi_step_epoch(fused, multi):
    spec, theta, X, f, y, model, group, rules = _epoch_case((16, 16), 640, 64)
    eng = util.load_engine(spec, theta, X, f, y, engine=model.engine())
    eng.set_option("fused_update", fused)
    eng.set_option("multi_step", multi)
    eng.opt_init_groups(group, rules)
    eng.train_epoch(64, shuffle=False)
    eng.train_epoch(64, shuffle=False)
    ref = _reference(spec, theta, X, f, y, [(a, 64) for a in range(0, 640, 64)] * 2, group, rules)
    _close(eng.get_params(), ref)
    eng.close()


@pytest.mark.parametrize("hidden,B,batch", [((128, 128), 2048, 512),                 # wide (row-split) family
                                            ((160, 80, 40, 20), 1024, 64),           # layer-wise, few rows
                                            ((160, 80, 40, 20), 4096, 2048),         # layer-wise, large batch
                                            ((1024, 512, 256, 128, 64), 512, 256)])  # the tutorial net
def test_wide_and_layerwise_families(hidden, B, batch):
    spec, theta, X, f, y, model, group, rules = _epoch_case(hidden, B, batch)
    eng = util.load_engine(spec, theta, X, f, y, engine=model.engine())
    eng.opt_init_groups(group, rules)
    windows = [(a, batch) for a in range(0, B, batch)][:4]
    for a, n in windows:
        eng.train_step(a, n)
    got, ref = eng.get_params(), _reference(spec, theta, X, f, y, windows, group, rules)
    eng.close()
    if len(hidden) <= 3 and max(hidden) <= 128:
        _close(got, ref)
        return
    # the layer-wise form: Adam turns last-ulp gradient differences of near-zero entries into lr-sized steps -- the bar
    # tests/test_gpu_lform.py puts on its trajectories; the global parameter (its own rule, a sum over the batch) to the full bar
    d = np.abs(got - ref)
    assert np.mean(d <= 2e-5) >= 0.999 and d.max() <= len(windows) * 3e-3 * 1.01, (np.mean(d <= 2e-5), d.max())
    q = model.opt_branches()["Q10"][0]
    assert d[q] <= TOL * max(1.0, abs(float(ref[q]))), d[q]


def _multi_data(n=1024):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((4, n)).astype(np.float32)
    f = {"ta": rng.uniform(0, 30, n).astype(np.float32)}
    y = {"reco": rng.uniform(1, 9, n).astype(np.float32)}
    y["reco"][::7] = np.nan
    return X, f, y


def _multi_run(spec, opt, expect_branches):
    X, f, y = _multi_data()
    model = util.model_from_spec(spec)
    assert list(model.opt_branches()) == expect_branches
    group, rules = _rules(model, opt)
    theta = ho.init_theta(spec, 6, np.float32)
    eng = util.load_engine(spec, theta, X, f, y, engine=model.engine())
    eng.opt_init_groups(group, rules)
    windows = [(a, 256) for a in range(0, 1024, 256)] * 2
    for a, n in windows:
        eng.train_step(a, n)
    _close(eng.get_params(), _reference(spec, theta, X, f, y, windows, group, rules))
    eng.close()
    return group, rules


def test_multi_network_one_rule_per_network():
    spec = ho.HybridSpec(4, [1], "rbq10", dict(ho.RBQ10_PARAMS), ["rb", "Q10"], [], ["reco"], "tanh", True,
                         nets=[([0, 1], [8, 8]), ([2, 3], [16, 8])])
    with pytest.warns(UserWarning, match="ignored"):
        _multi_run(spec, {"rb": T.Adam(1e-2), "Q10": T.RMSProp(5e-3), "ps": T.Descent(1.0)}, ["rb", "Q10"])


def test_multi_network_global_on_adamw_and_a_branch_left_out():
    spec = ho.HybridSpec(4, [1], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "tanh", True, nets=[([0, 1, 2], [16, 8])])
    group, rules = _multi_run(spec, {"Q10": T.AdamW(2e-2, (0.9, 0.999), 0.1)}, ["rb", "Q10"])
    assert rules[int(group[0])] == T._opt_args(T.Adam(0.001))           # "rb" left out: Optimisers.Adam()


# ---- exact invariants, every family (bf16 forms included) -------------------------------------------------------------------------
def _family_cases():
    return {
        "per-wave": lambda: util.rbq10_case(2048, "tanh", True, 0.1),
        "wide": lambda: util.rbq10_case(2048, "tanh", True, 0.1, hidden=(128, 128)),
        "layer-wise": lambda: util.rbq10_case(2048, "tanh", True, 0.1, hidden=(160, 80, 40, 20)),
        "bf16_fwd": lambda: (lambda s: (s, ho.init_theta(s, 3, np.float32), *ho.make_synth_c5(2048, 11, 0.1)))(ho.c5_spec(precision="bf16_fwd")),
        "bf16": lambda: (lambda s: (s, ho.init_theta(s, 3, np.float32), *ho.make_synth_c5(2048, 11, 0.1)))(ho.c5_spec(precision="bf16")),
    }


def _run(case, setup, fused=0, steps=((0, 512), (512, 512), (1024, 512), (0, 1024))):
    spec, theta, X, f, y = case
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_option("fused_update", fused)
    setup(eng)
    losses = [eng.train_step(a, n) for a, n in steps]
    m, v, bt = eng.get_opt_state()
    out = (eng.get_params(), m, v, np.asarray(bt), losses)
    eng.close()
    return out


@pytest.mark.parametrize("family,fused", [(k, 0) for k in _family_cases()] + [("per-wave", 1), ("per-wave", 2)])   # (fused_update: per-wave only)
def test_two_groups_of_one_rule_are_the_single_rule_bits(family, fused):
    case = _family_cases()[family]()
    n = case[1].size
    group = (np.arange(n) >= n // 3).astype(np.uint8)          # (a boundary inside the first layer's weights)
    r = dict(rule="Adam", lr=0.01)
    th1, m1, v1, bt1, l1 = _run(case, lambda e: e.opt_init(**r), fused)
    th2, m2, v2, bt2, l2 = _run(case, lambda e: e.opt_init_groups(group, [r, r]), fused)
    assert np.array_equal(th1, th2) and np.array_equal(m1, m2) and np.array_equal(v1, v2)
    assert bt2.shape == (2, 2) and np.array_equal(bt2[0], bt1) and np.array_equal(bt2[1], bt1)
    assert np.array_equal(np.asarray(l1), np.asarray(l2))


@pytest.mark.parametrize("family", list(_family_cases()))
def test_descent_zero_branch_is_frozen(family):
    case = _family_cases()[family]()
    theta = case[1]
    n = theta.size
    group = np.zeros(n, np.uint8)
    group[n - 7:] = 1                                           # the last output biases / globals frozen
    group[: n // 4] = 1                                         # and the first quarter
    th, m, v, bt, _ = _run(case, lambda e: e.opt_init_groups(group, [dict(rule="Adam", lr=0.01), dict(rule="Descent", lr=0.0)]))
    frozen = group == 1
    assert np.array_equal(th[frozen], theta[frozen])
    assert not np.array_equal(th[~frozen], theta[~frozen])
    assert np.all(m[frozen] == 0) and np.all(v[frozen] == 0)


# ---- state round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
def test_state_round_trip_resumes_with_the_same_bits(fused):
    spec, theta, X, f, y = util.rbq10_case(1024, "tanh", True, 0.1)
    model = util.model_from_spec(spec)
    group, rules = _rules(model, {"ps": T.AdamW(1e-2, (0.8, 0.99), 0.05), "Q10": T.Adam(3e-2, (0.7, 0.95))})
    a = util.load_engine(spec, theta, X, f, y, engine=model.engine())
    a.set_option("fused_update", fused)
    a.opt_init_groups(group, rules)
    for i in range(3):
        a.train_step(i * 256, 256)
    m, v, bt = a.get_opt_state()
    assert bt.shape == (2, 2) and bt[0, 0] != bt[1, 0]
    b = util.load_engine(spec, a.get_params(), X, f, y, engine=model.engine())
    b.set_option("fused_update", fused)
    b.opt_init_groups(group, rules)
    b.set_opt_state(m, v, bt)
    got = np.empty(4, np.float32)
    assert b._lib.eh_get_opt_beta_t(b._h, got.ctypes.data_as(util_fp()), 2) == 0
    assert np.array_equal(got.reshape(2, 2), bt)
    for e in (a, b):
        e.train_step(768, 256)
        e.train_step(0, 256)
    assert np.array_equal(a.get_params(), b.get_params())
    ma, va, bta = a.get_opt_state(); mb, vb, btb = b.get_opt_state()
    assert np.array_equal(ma, mb) and np.array_equal(va, vb) and np.array_equal(bta, btb)
    assert b._lib.eh_get_opt_beta_t(b._h, got.ctypes.data_as(util_fp()), 1) != 0      # the group count is checked
    a.close(); b.close()


def util_fp():
    import ctypes
    return ctypes.POINTER(ctypes.c_float)


def test_more_than_sixteen_groups_is_unsupported():
    spec, theta, X, f, y = util.rbq10_case(256, "tanh", True)
    eng = util.load_engine(spec, theta, X, f, y)
    group = (np.arange(theta.size) % 17).astype(np.uint8)
    with pytest.raises(NotImplementedError, match="at most 16"):                # EH_EUNSUPPORTED
        eng.opt_init_groups(group, [dict(rule="Descent", lr=0.01 * (k + 1)) for k in range(17)])
    eng.opt_init_groups(group % 16, [dict(rule="Descent", lr=0.01 * (k + 1)) for k in range(16)])
    eng.train_step(0, 256)
    eng.close()


# ---- data parallel: a local group of two handles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
def test_local_group_trains_like_one_engine_on_the_union(fused):
    from easyhybrid_jl_amd import dp
    B, world = 4096, 2
    spec, theta, X, f, y = util.rbq10_case(B, "tanh", True, 0.0)
    y["reco"][: B // world][::2] = np.nan
    model = util.model_from_spec(spec)
    group, rules = _rules(model, HEADLINE_OPT)
    engs = []
    for r in range(world):
        lo, hi = dp.shard_range(B, r, world)
        e = util.load_engine(spec, theta, X[:, lo:hi], {k: v[lo:hi] for k, v in f.items()}, {k: v[lo:hi] for k, v in y.items()},
                             engine=model.engine())
        e.opt_init_groups(group, rules)
        engs.append(e)
    HybridEngine.comm_init_local(engs)
    for e in engs:
        e.set_option("fused_update", fused)
    ref = util.load_engine(spec, theta, X, f, y, engine=model.engine())
    ref.opt_init_groups(group, rules)
    per = B // world
    win = per // 4
    for s in range(6):
        a = (s % 4) * win
        HybridEngine.dp_train_step_group(engs, [a] * world, win)
        idx = np.concatenate([np.arange(r * per + a, r * per + a + win) for r in range(world)]).astype(np.int32)
        ref.train_step(0, idx.size, want_loss=False, idx=idx)
    th = [e.get_params() for e in engs]
    assert np.array_equal(th[0], th[1])
    assert np.max(np.abs(th[0] - ref.get_params())) <= 2e-6
    bts = [e.get_opt_state()[2] for e in engs]
    assert np.array_equal(bts[0], bts[1]) and np.array_equal(bts[0], ref.get_opt_state()[2])
    engs[0].comm_destroy()
    for e in engs:
        e.close()
    ref.close()


# ---- the front door ---------------------------------------------------------------------------------------------------------------
def _cols(n=3000, seed=3):
    X, f, y = ho.make_synth_rbq10(n, seed, 0.1)
    return {"sw_pot": X[0], "dsw_pot": X[1], "ta": f["ta"], "reco": y["reco"]}


def test_front_door_train_with_per_branch_rules():
    cols = _cols()
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    kw = dict(nepochs=3, batchsize=256, random_seed=7, loss_types=["mse"])
    a = eh.train(model, cols, opt={"ps": eh.Adam(0.01), "Q10": eh.Descent(0.0)}, **kw)
    b = eh.train(model, cols, opt={"ps": eh.Adam(0.01), "Q10": eh.Descent(0.0)}, **kw)
    pa, pb = np.asarray(a.ps, np.float32), np.asarray(b.ps, np.float32)
    assert np.array_equal(pa, pb)
    q = model.opt_branches()["Q10"][0]
    c = eh.train(model, cols, opt={"ps": eh.Adam(0.01), "Q10": eh.Descent(0.5)}, **kw)
    pc = np.asarray(c.ps, np.float32)
    assert pc[q] != pa[q]                                       # Q10 moves under its own rule ...
    assert not np.array_equal(pc[:q], pa[:q])
    d = eh.train(model, cols, opt={"ps": eh.Adam(0.01), "Q10": eh.Descent(0.0)}, **{**kw, "nepochs": 1})
    assert np.asarray(d.ps, np.float32)[q] == pa[q]            # ... and stays where it started on Descent(0)
