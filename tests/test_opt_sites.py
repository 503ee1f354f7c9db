"""The NumPy side of the update-site tests (tests/test_gpu_opt_sites.py): the rule twin against the oracle's own rule lines, the conditions
on the inputs of every GPU case from the reference alone, and the sharpness of the comparator -- every way an update site can be wrong
that the trajectory tests let through must be rejected."""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho
from tests import opt_site_cases as oc
from tests import opt_site_twin as tw

F = np.float32


def _random(n, seed, pow2=False):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(F)
    if pow2:                    # signed powers of two: g * g and c * g are exact, so every grouping of (1 - beta2) * g * g is one number
        g = (np.sign(g) * 2.0 ** rng.integers(-12, 4, n)).astype(F)
    th = rng.uniform(-1, 1, n).astype(F)
    m = (rng.standard_normal(n) * 0.1).astype(F)
    v = (rng.uniform(0, 1, n) ** 2).astype(F)
    return g, th, m, v


# ---- the twin against the oracle ---------------------------------------------------------------------------------------------------
# ho.adam_step writes `(1 - b2) * grad * grad`, which NumPy evaluates as ((1 - b2) g) g; eh_opt_update -- and Optimisers.jl's
# `(1 - b2) * abs2(dx)` -- square first.  The two round differently in the last bit of v.  So: bit for bit on gradients that are signed
# powers of two, where both groupings are the same number (everything else of the rule -- m, the order of the divisions, sqrt, eps, the
# coupled decay -- runs on random values); on general gradients m bit for bit, v within two ulp (the two terms are an ulp of the term apart,
# which is at most an ulp of v, and each sum rounds by half an ulp) and theta within what two ulp of v can do.
@pytest.mark.parametrize("t", [1, 2, 41])
@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_twin_is_the_oracles_adam_step(name, t):
    r = tw.RULES[name]
    lr, b1, b2, eps, wd = tw.hyper(r)
    for pow2 in (True, False):
        g, th, m, v = _random(4096, 3 + t, pow2)
        st = dict(m=m.copy(), v=v.copy(), t=t - 1)
        th_o = ho.adam_step(th.copy(), g, st, lr=r["lr"], weight_decay=r.get("weight_decay", 0.0))
        bt = np.array([b1 ** t, b2 ** t], F)           # (the oracle's own products: a power, not a running product)
        th_t, m_t, v_t, bt_t = tw.step(r, None, g, th, m, v, bt)
        assert th_o.dtype == F and np.array_equal(m_t, st["m"])
        assert np.array_equal(bt_t, bt * np.array([b1, b2], F))
        if pow2:
            assert np.array_equal(v_t, st["v"]) and np.array_equal(th_t, th_o)
        else:
            assert np.all(np.abs(v_t.astype(np.float64) - st["v"]) <= 2 * tw.ulp(st["v"]))
            # d upd / upd = d v / (2 v) <= 2^-23: at most two ulp of the update, and the roundings of the steps behind it, each at most
            # half an ulp of the update (division, sum, product) or of theta (the coupled term, the final difference)
            upd = np.abs(th_o.astype(np.float64) - th) + np.abs(lr * wd * th)
            assert np.all(np.abs(th_t.astype(np.float64) - th_o) <= 4 * tw.ulp(upd) + 2 * tw.ulp(th_o))


def test_twin_is_the_suites_rmsprop_and_descent_lines():
    """RMSProp as tests/test_gpu_opt_branches.py writes it (rho v + (1 - rho) g g, left to right) and Descent as tests/test_gpu_parity.py
    does.  (test_gpu_parity.py's own RMSProp line takes float32(0.1) for 1 - rho; 1 - float32(0.9) is three ulp above it -- the engine
    and Optimisers.jl compute the difference.)"""
    for pow2 in (True, False):
        g, th, m, v = _random(4096, 8, pow2)
        r = tw.RULES["RMSProp"]
        rho, lr = F(0.9), F(r["lr"])
        vq = rho * v + (F(1) - rho) * g * g
        th_o = th - g * (lr / (np.sqrt(vq) + F(1e-8)))
        th_t, m_t, v_t, _ = tw.step(r, None, g, th, m, v, tw.warm_products(r))
        assert np.array_equal(m_t, m)
        if pow2:
            assert np.array_equal(v_t, vq) and np.array_equal(th_t, th_o)
        else:
            assert np.all(np.abs(v_t.astype(np.float64) - vq) <= 2 * tw.ulp(vq))
            assert np.all(np.abs(th_t.astype(np.float64) - th_o) <= 4 * tw.ulp(th_o.astype(np.float64) - th) + 2 * tw.ulp(th_o))
        r = tw.RULES["Descent"]
        th_t, m_t, v_t, bt_t = tw.step(r, None, g, th, m, v, tw.warm_products(r))
        assert np.array_equal(th_t, th - F(r["lr"]) * g) and np.array_equal(m_t, m) and np.array_equal(v_t, v)


def test_grouped_twin_is_the_rules_slice_by_slice_and_an_empty_batch_moves_nothing():
    g, th, m, v = _random(1000, 5)
    group = tw.random_groups(1000, 4, 2)
    bt = tw.warm_products(tw.GROUPED)
    assert bt.shape == (4, 2) and len({float(x) for x in bt[:, 0]}) == 4            # no two groups share a pair
    got = tw.step(tw.GROUPED, group, g, th, m, v, bt)
    for k, r in enumerate(tw.GROUPED):
        s = group == k
        one = tw.step(r, None, g[s], th[s], m[s], v[s], bt[k])
        for a, b in zip(got[:3], one[:3]):
            assert np.array_equal(a[s], b)
        assert np.array_equal(got[3][k], one[3])
    same = tw.step(tw.GROUPED, group, g, th, m, v, bt, valid=False)
    for a, b in zip(same, (th, m, v, bt)):
        assert np.array_equal(a, b)


def test_warm_state_ranges():
    m0, v0 = tw.warm_state(10000, 0.37, 1)
    assert m0.dtype == F and v0.dtype == F
    assert np.all((np.abs(m0) >= 2 * 0.37 * (1 - 1e-6)) & (np.abs(m0) <= 4 * 0.37 * (1 + 1e-6))) and 0.4 < np.mean(m0 > 0) < 0.6
    assert np.all((v0 >= 2 * 0.37 ** 2 * (1 - 1e-6)) & (v0 <= 4 * 0.37 ** 2 * (1 + 1e-6)))
    bt = tw.warm_products(tw.RULES["Adam"])
    assert bt.dtype == F and bt[0] == pytest.approx(0.9 ** 40, rel=1e-5) and bt[1] == pytest.approx(0.999 ** 40, rel=1e-5)


# ---- the conditions on the inputs, every case of the GPU file -------------------------------------------------------------------------
@pytest.mark.parametrize("model,B,steps", oc.CASES)
def test_inputs_of_every_gpu_case_meet_the_conditions(model, B, steps):
    for rule in oc.RULE_NAMES:
        ratios = oc.check_case_inputs(model, B, steps, rule)
        assert ratios
    oc.reference.cache_clear()


# ---- sharpness of the comparator ----------------------------------------------------------------------------------------------------------
def _sharp_case(rule_name):
    ref = oc.reference("headline", 257, 1, rule_name)
    s = ref["steps"][0]
    th, m, v, bt = s["after"]
    good = dict(theta=th.copy(), m=m.copy(), v=v.copy(), bt=bt.copy())
    bars = tw.element_bars(s["err"], good)
    return ref, s, good, bars


def _rejects(ref, good, bars, got, what):
    with pytest.raises(AssertionError, match=what):
        tw.compare("corrupted", got, good, bars, set_state=dict(m=ref["m0"], v=ref["v0"]), rules=ref["rules"], group=ref["group"], quiet=True)


@pytest.mark.parametrize("rule_name", oc.RULE_NAMES)
def test_comparator_accepts_the_reference_and_the_other_summation_order(rule_name):
    ref, s, good, bars = _sharp_case(rule_name)
    kw = dict(set_state=dict(m=ref["m0"], v=ref["v0"]), rules=ref["rules"], group=ref["group"], quiet=True)
    assert max(tw.compare("itself", good, good, bars, **kw).values()) == 0.0
    th, m, v, bt = tw.step(ref["rules"], ref["group"], s["g64"], *s["before"])
    worst = tw.compare("fp64 sums", dict(theta=th, m=m, v=v, bt=bt), good, bars, **kw)
    assert max(worst.values()) <= 0.25 + 1e-12            # (the bar's first term is four times this deviation)


@pytest.mark.parametrize("rule_name", oc.RULE_NAMES)
def test_comparator_rejects_every_corruption(rule_name):
    ref, s, good, bars = _sharp_case(rule_name)
    rules, group = tw.as_groups(ref["rules"], ref["group"], good["theta"].size)
    th0, m0, v0, bt0 = s["before"]
    g = s["g32"]
    n = g.size
    moves = np.flatnonzero(np.abs(good["theta"].astype(np.float64) - th0) > 100 * bars["theta"])
    for k, r in enumerate(rules):
        kind = r["rule"]
        own = moves[group[moves] == k]
        # one element not updated
        i = int(own[0])
        got = {x: a.copy() for x, a in good.items()}
        got["theta"][i], got["m"][i], got["v"][i] = th0[i], m0[i], v0[i]
        _rejects(ref, good, bars, got, rf"theta\[{i}\]")
        # one element updated twice
        i = int(own[1])
        got = {x: a.copy() for x, a in good.items()}
        one = tw.rule_update(r, g[i:i + 1], good["theta"][i:i + 1], good["m"][i:i + 1], good["v"][i:i + 1], bt0.reshape(-1, 2)[k, 0], bt0.reshape(-1, 2)[k, 1])
        got["theta"][i], got["m"][i], got["v"][i] = one[0][0], one[1][0], one[2][0]
        _rejects(ref, good, bars, got, rf"theta\[{i}\]")
        # one element given its neighbour's gradient, where the two differ by more than 1e-3 s
        cand = [int(j) for j in own if j + 1 < n and abs(float(g[j]) - float(g[j + 1])) > 1e-3 * ref["s"]]
        i = cand[0]
        got = {x: a.copy() for x, a in good.items()}
        one = tw.rule_update(r, g[i + 1:i + 2], th0[i:i + 1], m0[i:i + 1], v0[i:i + 1], bt0.reshape(-1, 2)[k, 0], bt0.reshape(-1, 2)[k, 1])
        got["theta"][i], got["m"][i], got["v"][i] = one[0][0], one[1][0], one[2][0]
        _rejects(ref, good, bars, got, rf"(theta|m|v)\[{i}\]")
        # state the rule does not keep, touched
        km, kv = tw.keeps(r)
        if not km:
            i = int(own[2])
            got = {x: a.copy() for x, a in good.items()}
            got["m"][i] = np.nextafter(got["m"][i], F(np.inf))
            _rejects(ref, good, bars, got, rf"m\[{i}\] was written although {kind} keeps no m")
        if not kv:
            i = int(own[3])
            got = {x: a.copy() for x, a in good.items()}
            got["v"][i] = np.nextafter(got["v"][i], F(np.inf))
            _rejects(ref, good, bars, got, rf"v\[{i}\] was written although {kind} keeps no v")
        # one element under another group's rule (and that group's products)
        if len(rules) > 1:
            for k2, r2 in enumerate(rules):
                if k2 == k:
                    continue
                i = int(own[4])
                got = {x: a.copy() for x, a in good.items()}
                one = tw.rule_update(r2, g[i:i + 1], th0[i:i + 1], m0[i:i + 1], v0[i:i + 1], bt0[k2, 0], bt0[k2, 1])
                got["theta"][i], got["m"][i], got["v"][i] = one[0][0], one[1][0], one[2][0]
                _rejects(ref, good, bars, got, rf"\[{i}\]")
            # the right rule under another group's products: the Adam rules divide by them
            if kind in ("Adam", "AdamW"):
                k2 = (k + 1) % len(rules)
                i = int(own[5])
                got = {x: a.copy() for x, a in good.items()}
                one = tw.rule_update(r, g[i:i + 1], th0[i:i + 1], m0[i:i + 1], v0[i:i + 1], bt0[k2, 0], bt0[k2, 1])
                got["theta"][i] = one[0][0]
                _rejects(ref, good, bars, got, rf"theta\[{i}\]")
    # the products not advanced (every group's, and one group's alone)
    got = {x: a.copy() for x, a in good.items()}
    got["bt"] = np.array(bt0, F)
    _rejects(ref, good, bars, got, "running products")
    if len(rules) > 1:
        got["bt"] = good["bt"].copy()
        got["bt"][2] = bt0[2]
        _rejects(ref, good, bars, got, "running products")
    # an update applied although no target was valid
    was = dict(theta=th0, m=m0, v=v0, bt=bt0)
    tw.compare_unchanged("no valid target", was, was)
    with pytest.raises(AssertionError, match="changed on a minibatch without a valid target"):
        tw.compare_unchanged("no valid target", good, was)
    got = {x: np.array(a, F) for x, a in was.items()}
    got["bt"] = good["bt"]
    with pytest.raises(AssertionError, match="bt changed"):
        tw.compare_unchanged("no valid target", got, was)
