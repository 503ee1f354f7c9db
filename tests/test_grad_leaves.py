"""The leaf-by-leaf gradient check of tests/util.py (leaf_table, leaf_errors, check_gradient), without a device: the table against the
oracle's own pack / unpack, that a gradient wrong in one small leaf passes relerr() and fails check_gradient(), and that the inputs of
the device tests stand on the reference alone -- the oracle run in fp32, in four summation orders, holds every leaf of them well inside
the bar the device is held to."""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho
from tests import grad_leaf_cases as glc
from tests import test_gpu_fuzz as fuzz
from tests import test_gpu_lform as lform
from tests import test_gpu_parity as parity
from tests import util

BAR = 1e-5


# ---- the table -----------------------------------------------------------------------------------------------------------------------
LINEAR = {"alpha": (1.0, -2.0, 3.0), "beta": (0.5, -1.0, 2.0)}
TABLE_SPECS = {
    "one layer": lambda: ho.rbq10_spec((7,), "tanh", True),
    "two layers": lambda: ho.rbq10_spec((16, 5), "tanh", False),
    "three layers": lambda: ho.HybridSpec(5, [9, 4, 6], "expo2pool", dict(ho.EXPO2POOL_PARAMS), ["R0a", "R0b"], ["ka", "kb"], ["Resp_obs"], "relu", True),
    "MultiNN, different depths": lambda: ho.HybridSpec(4, [1], "rbq10", dict(ho.RBQ10_PARAMS), ["rb", "Q10"], [], ["reco"], "tanh", True,
                                                       nets=[([0, 1], [5, 3]), ([2, 3], [4])]),
    "MultiNN with a global": lambda: ho.HybridSpec(6, [1], "rs_components", dict(ho.RS6_PARAMS), ["Rb_het", "Rb_root", "Rb_myc"], ["Q10_root", "Q10_het"], ["R_soil"],
                                                   "tanh", True, nets=[([0, 1], [6, 3, 2]), ([2], [4]), ([3, 4, 5], [2, 5])]),
    "no globals": lambda: ho.HybridSpec(3, [8, 8], "linear", LINEAR, ["alpha", "beta"], [], [], "tanh", True),
    "no network": lambda: ho.HybridSpec(2, [8], "linear", LINEAR, [], ["beta", "alpha"], [], "tanh", True),
}


@pytest.mark.parametrize("name", list(TABLE_SPECS))
def test_the_table_is_the_oracles_layout(name):
    """a distinct constant written into each leaf through the table comes out of ho.unpack as that leaf, and ho.pack puts it back"""
    spec = TABLE_SPECS[name]()
    table = util.leaf_table(spec)
    assert table[-1][2] == spec.n_theta and table[0][1] == 0
    assert all(a < b for _, a, b in table) and all(table[i][2] == table[i + 1][1] for i in range(len(table) - 1))
    assert len({n for n, _, _ in table}) == len(table)
    theta = np.zeros(spec.n_theta)
    for i, (_, a, b) in enumerate(table):
        theta[a:b] = i + 1
    nets, raw = ho.unpack(spec, theta)
    want = 1
    for Ws, (_, dims) in zip(nets, spec.net_list):
        assert len(Ws) == len(dims)
        for (W, b), (o, i) in zip(Ws, dims):
            assert W.shape == (o, i) and np.all(W == want) and b.shape == (o,) and np.all(b == want + 1)
            want += 2
    assert list(raw) == list(range(want, want + len(spec.glob))) and want + len(spec.glob) - 1 == len(table)
    assert [n for n, _, _ in table[len(table) - len(spec.glob):]] == list(spec.glob)
    assert np.array_equal(ho.pack(spec, nets, raw), theta)


def test_leaf_errors_is_relerr_of_each_leaf():
    table = [("a", 0, 3), ("b", 3, 4), ("dead", 4, 6)]
    g64 = np.array([1.0, -2.0, 0.5, 1e-4, 0.0, 0.0])
    g = g64 + np.array([0.0, 2e-3, 0.0, 1e-6, 1e-9, 0.0])
    e = util.leaf_errors(g, g64, table, floor=1e-3)
    assert e == pytest.approx([1e-3, 1e-6 / 2e-3, 1e-9 / 2e-3])          # b and the dead leaf sit on the floor, 1e-3 x 2.0
    e0 = util.leaf_errors(g, g64, table, floor=0.0)
    assert e0[:2] == pytest.approx([1e-3, 1e-2]) and e0[2] > 1e100          # without a floor a dead leaf must be exactly zero
    assert util.leaf_errors(g64, g64, table, floor=0.0) == [0.0, 0.0, 0.0]
    assert util.leaf_shares(g64, table) == pytest.approx([1.0, 5e-5, 0.0])


def test_ref32_is_evaluated_lazily_and_once():
    spec, theta, X, f, y = util.rbq10_case(12, "tanh", False)
    _, g64, _ = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y)
    calls = []
    inner = util.ref32_orders(spec, theta, X, f, y)

    def ref32():
        calls.append(1)
        return inner()
    util.check_gradient(g64, g64, spec, BAR, ref32)
    assert not calls                                                        # a passing case costs nothing extra
    orders = inner()
    assert len(orders) == 4 and all(g.shape == g64.shape for g in orders)
    assert any(not np.array_equal(orders[0], g) for g in orders[1:])       # (the permutations are other summation orders)
    bad = g64.copy(); bad[:] *= 1 + 1e-3
    with pytest.raises(AssertionError):
        util.check_gradient(bad, g64, spec, BAR, ref32)
    assert len(calls) == 1                                                  # every leaf missed: still one evaluation
    # the escape: a leaf as far off as the fp32 reference itself (and no further than four times that) passes
    table = util.leaf_table(spec)
    e32 = util.ref32_leaf_errors(inner, g64, table)
    worst = max(range(len(table)), key=lambda i: e32[i])
    _, a, b = table[worst]
    off = g64.copy(); off[a:b] = orders[int(np.argmax([util.leaf_errors(g, g64, table)[worst] for g in orders]))][a:b]
    util.check_gradient(off, g64, spec, 0.0, ref32)                         # (bar 0: only the escape can pass it)


# ---- a wrong gradient is caught --------------------------------------------------------------------------------------------------------
def _two_net():
    return glc.two_net_case(glc.TWO_NET_NARROW, 257)


WRONG = {
    # case, the small leaf, a large leaf
    "rbq10 B = 12": (lambda: util.rbq10_case(12, "tanh", False), "Q10", "nn.layer_3.weight"),
    "two networks": (_two_net, "Q10.layer_2.bias", "rb.layer_3.weight"),
    "headline B = 1000": (lambda: glc.headline_case(1000), "nn.layer_1.bias", "nn.layer_3.bias"),
}


@pytest.mark.parametrize("name", list(WRONG))
def test_a_gradient_wrong_in_one_small_leaf_is_caught(name):
    make, small, large = WRONG[name]
    spec, theta, X, f, y = make()
    _, g64, _ = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y)
    table = {n: (a, b) for n, a, b in util.leaf_table(spec)}
    ref32 = util.ref32_orders(spec, theta, X, f, y)
    util.check_gradient(g64, g64, spec, BAR, ref32)
    share = dict(zip(table, util.leaf_shares(g64, util.leaf_table(spec))))
    assert share[small] <= 5e-3 and share[large] >= 0.1, (share[small], share[large])
    a, b = table[small]
    g = g64.copy(); g[a:b] *= 1 + 1e-3
    assert util.relerr(g, g64) <= BAR                                       # the norm-wise check does not see it
    with pytest.raises(AssertionError, match="leaf " + small.replace(".", r"\.") + " "):
        util.check_gradient(g, g64, spec, BAR, ref32)
    a, b = table[large]
    g = g64.copy(); g[a:b] *= 1 + 1e-3
    assert util.relerr(g, g64) > BAR                                        # a large leaf: both notice
    with pytest.raises(AssertionError, match="leaf " + large.replace(".", r"\.") + " "):
        util.check_gradient(g, g64, spec, BAR, ref32)


def test_a_leak_between_the_two_networks_is_caught():
    """the two-network case: 1e-5 of the rb network's first-layer weight gradient added into the Q10 network's (a tenth of that leaf's own
    size), and half a percent of the Q10 network's bias sums lost -- both pass relerr() at 1e-5"""
    spec, theta, X, f, y = _two_net()
    _, g64, _ = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y)
    table = {n: (a, b) for n, a, b in util.leaf_table(spec)}
    ref32 = util.ref32_orders(spec, theta, X, f, y)
    (a, b), (c, d) = table["Q10.layer_1.weight"], table["rb.layer_1.weight"]
    g = g64.copy(); g[a:b] += 1e-5 * g64[c:c + (b - a)]
    assert util.relerr(g, g64) <= BAR
    with pytest.raises(AssertionError, match=r"leaf Q10\.layer_1\.weight "):
        util.check_gradient(g, g64, spec, BAR, ref32)
    g = g64.copy()
    for n, (a, b) in table.items():
        if n.startswith("Q10.") and n.endswith(".bias"):
            g[a:b] *= 0.995
    assert util.relerr(g, g64) <= BAR
    with pytest.raises(AssertionError, match=r"leaf Q10\.layer_1\.bias "):
        util.check_gradient(g, g64, spec, BAR, ref32)


# ---- the inputs stand on the reference alone ---------------------------------------------------------------------------------------------
def _e32(spec, theta, X, f, y, floor, **kw):
    _, g64, _ = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y, **kw)
    table = util.leaf_table(spec)
    return table, util.ref32_leaf_errors(util.ref32_orders(spec, theta, X, f, y, **kw), g64, table, floor), util.leaf_shares(g64, table)


def _holds_a_quarter(case, bar, floor, **kw):
    table, e32, share = _e32(*case, floor, **kw)
    bad = [(n, f"{e:.2e}", f"{s:.1e}") for (n, _, _), e, s in zip(table, e32, share) if not e <= bar / 4]
    assert not bad, bad


CORE = ([(f"grid {act} scale={scale} B={B}", (lambda act=act, scale=scale, B=B, nan=nan: util.rbq10_case(B, act, scale, nan)))
         for act in parity.GRID_ACTS for scale in (False, True) for B, nan in parity.GRID_BATCHES]
        + [(f"mlp {h}", (lambda h=h: parity.mlp_shape_case(h))) for h in parity.MLP_SHAPES]
        + [("config 3", parity.config3_case)]
        + [(f"sources {m} {n} {g}", (lambda m=m, n=n, g=g: parity.parameter_source_case(m, n, g))) for m, n, g in parity.PARAMETER_SOURCES])


@pytest.mark.parametrize("name", [n for n, _ in CORE])
def test_the_fp32_reference_holds_a_quarter_of_the_bar_on_the_core_cases(name):
    """the named core cases of tests/test_gpu_parity.py, as check_gradient() sees them there (floor 1e-3): every leaf, all four orders"""
    _holds_a_quarter(dict(CORE)[name](), BAR, 1e-3)


NEW_F32 = ([(f"two networks narrow B={B}", (lambda B=B: glc.two_net_case(glc.TWO_NET_NARROW, B))) for B in glc.TWO_NET_BATCHES]
           + [(f"two networks wide B={B}", (lambda B=B: glc.two_net_case(glc.TWO_NET_WIDE, B, glc.TWO_NET_WIDE_DRAW))) for B in glc.TWO_NET_BATCHES]
           + [(f"fast path B={B}", (lambda B=B: util.rbq10_case(B, "tanh", False))) for B in glc.FAST_PATH_BATCHES]
           + [(f"headline B={B}", (lambda B=B: glc.headline_case(B))) for B in glc.HEADLINE_BATCHES])


@pytest.mark.parametrize("name", [n for n, _ in NEW_F32])
def test_the_fp32_reference_holds_a_quarter_of_the_bar_on_the_new_cases(name):
    """the cases of tests/test_gpu_grad_leaves.py, as they are checked there: no floor under any leaf"""
    _holds_a_quarter(dict(NEW_F32)[name](), BAR, 0.0)


@pytest.mark.parametrize("B", glc.TWO_NET_BATCHES)
def test_the_layer_wise_two_network_case_stands_on_the_reference(B):
    """the first of tests/test_gpu_lform.py's MULTI shapes (wider than any fused envelope) with the two-network forcing"""
    _holds_a_quarter(glc.two_net_case(lform.MULTI[0][0], B), BAR, 0.0)


BF16_BARS = {"bf16_fwd": 5e-5, "bf16": 2e-5}          # tests/test_gpu_bf16.py


@pytest.mark.parametrize("precision", list(BF16_BARS))
@pytest.mark.parametrize("B", glc.TWO_NET_BATCHES)
def test_the_bf16_two_network_cases_stand_on_the_reference(B, precision):
    """the row-split kernel's bf16 modes: the reference is the oracle in the same `precision`, fp32 against fp64 -- the rounding flips
    tests/test_gpu_bf16.py describes are in its number too"""
    spec, theta, X, f, y = glc.two_net_case(glc.TWO_NET_WIDE, B, glc.TWO_NET_WIDE_DRAW)
    _holds_a_quarter((glc.two_net_spec_in(spec, precision), theta, X, f, y), BF16_BARS[precision], 0.0)


def test_the_weak_leaves_are_weak():
    """what the new cases are for: the leaves relerr() does not see are there, at the sizes the issue names"""
    for B in glc.TWO_NET_BATCHES:
        for nets in (glc.TWO_NET_NARROW, glc.TWO_NET_WIDE):
            table, _, share = _e32(*glc.two_net_case(nets, B, glc.TWO_NET_WIDE_DRAW if nets is glc.TWO_NET_WIDE else 0), 0.0)
            q = [s for (n, _, _), s in zip(table, share) if n.startswith("Q10.")]
            assert len(q) == 6 and 1e-6 < max(q) <= 1e-2, (B, nets, q)
    for B in glc.FAST_PATH_BATCHES:
        table, _, share = _e32(*util.rbq10_case(B, "tanh", False), 0.0)
        assert table[-1][0] == "Q10" and share[-1] <= 2e-2, share[-1]
    for B in glc.HEADLINE_BATCHES:
        table, _, share = _e32(*glc.headline_case(B), 0.0)
        assert table[1][0] == "nn.layer_1.bias" and share[1] <= 1e-2, share[1]


def _fuzz_kind_tol(seed, fastpath):
    spec, theta, X, f, y, kind, first, B, rng = fuzz._case(seed, fastpath)
    sl = slice(first, first + B)
    yb = {k: v[sl] for k, v in y.items()}
    if kind in ("kgeLoss", "pearsonLoss", "nseLoss") and sum(int((~np.isnan(v)).sum()) for v in yb.values()) < 3:
        kind = "mse"
    return spec, theta, X[:, sl], {k: v[sl] for k, v in f.items()}, yb, kind, (1e-3 if kind in ("kgeLoss", "pearsonLoss") else 1e-5)


def test_the_fuzz_seldom_needs_the_escape_on_the_reference_side():
    """fuzz seeds 0 .. 59 in both modes, each at its own bar: the live leaves on which the fp32 reference itself would need the escape
    (4 e32 above the bar) are at most one in twenty -- the leaf check of the fuzz is the bar, not the escape"""
    live = need = 0
    for fastpath in (False, True):
        for seed in range(60):
            spec, theta, X, f, y, kind, tol = _fuzz_kind_tol(seed, fastpath)
            kw = dict(kind=kind, bn_state=ho.bn_init(spec) if spec.input_batchnorm else None)
            l0, g64, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y, **kw)
            if sum(nv0) == 0 or not np.max(np.abs(g64)) > 1e-7 * max(1.0, abs(l0)):
                continue                                                  # (the test's own whole-gradient rule: nothing to compare)
            table = util.leaf_table(spec)
            e32 = util.ref32_leaf_errors(util.ref32_orders(spec, theta, X, f, y, **kw), g64, table)
            for (_, a, b), e in zip(table, e32):
                if np.max(np.abs(g64[a:b])) > 0:
                    live += 1
                    need += 4.0 * e > tol
    assert live >= 800 and need <= 0.05 * live, (need, live)
