"""Per-branch optimiser rules (TrainConfig.opt as a dict / NamedTuple, the reference's build_opt_state, src/training/train.jl:78-93):
the host side -- branch names and ranges, the group map over flat theta, defaults, warnings, merging, refusals.  No GPU."""
import collections
import sys
import warnings

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
import easyhybrid_jl_amd.train  # noqa: F401  (the module; the package's `train` is the function)
from oracle import hybrid_oracle as ho

from tests import util

T = sys.modules["easyhybrid_jl_amd.train"]


def _single():
    return util.model_from_spec(ho.rbq10_spec((16, 16), "tanh", True))


def _multi():
    return eh.constructHybridModel({"rb": ["sw_pot", "dsw_pot"], "Q10": ["sw_pot"]}, ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS),
                                   [], hidden_layers={"rb": [8], "Q10": [4, 4]}, activation="tanh")


def _no_net():
    return eh.constructHybridModel([], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), [], ["rb", "Q10"])


def test_branch_names_single_network():
    m = _single()
    br = m.opt_branches()
    assert list(br) == ["ps", "Q10"]
    assert br["ps"] == (0, m.n_nn) and br["Q10"] == (m.n_nn, m.n_nn + 1) and m.n_theta == m.n_nn + 1


def test_branch_names_multi_network_and_ranges_match_unpack():
    m = _multi()
    br = m.opt_branches()
    assert list(br) == ["rb", "Q10"]
    theta = np.arange(m.n_theta, dtype=np.float32)
    nets, glob = m.unpack(theta)
    for name, layers in nets.items():
        flat = np.concatenate([np.concatenate([W.flatten(order="F"), b]) for W, b in layers])
        lo, hi = br[name]
        assert np.array_equal(theta[lo:hi], flat)
    assert not glob and br["Q10"][1] == m.n_theta


def test_branch_names_without_network():
    m = _no_net()
    br = m.opt_branches()
    assert list(br) == ["ps", "rb", "Q10"] and br["ps"] == (0, 0)
    assert br["rb"] == (0, 1) and br["Q10"] == (1, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # "ps" is a branch (the reference's Chain()): no warning
        group, rules = T._opt_groups({"ps": T.Adam(0.01), "Q10": T.Descent(0.5)}, m)
    assert list(group) == [0, 1] and [r["rule"] for r in rules] == ["Adam", "Descent"]
    assert rules[0]["lr"] == pytest.approx(0.001)       # rb: the default Adam()


def test_group_map_against_unpack():
    m = _single()
    group, rules = T._opt_groups({"ps": T.Adam(1e-2), "Q10": T.Descent(5e-2)}, m)
    assert group.dtype == np.uint8 and group.size == m.n_theta
    theta = np.arange(m.n_theta, dtype=np.float32)
    _, glob = m.unpack(theta)
    q = int(glob["Q10"][0])
    assert group[q] == 1 and np.all(np.delete(group, q) == 0)
    assert rules == [T._opt_args(T.Adam(1e-2)), T._opt_args(T.Descent(5e-2))]


def test_namedtuple_form_equals_dict_form():
    m = _multi()
    NT = collections.namedtuple("NT", ["Q10", "rb"])
    g1, r1 = T._opt_groups(NT(Q10=T.RMSProp(1e-3), rb=T.AdamW(1e-2, (0.9, 0.999), 0.1)), m)
    g2, r2 = T._opt_groups({"rb": T.AdamW(1e-2, (0.9, 0.999), 0.1), "Q10": T.RMSProp(1e-3)}, m)
    assert np.array_equal(g1, g2) and r1 == r2
    lo, hi = m.opt_branches()["Q10"]
    assert np.all(g1[lo:hi] == 1) and np.all(g1[:lo] == 0) and r1[1]["rule"] == "RMSProp"


def test_missing_branch_takes_default_adam():
    m = _multi()
    group, rules = T._opt_groups({"rb": T.Descent(0.1)}, m)
    lo, hi = m.opt_branches()["Q10"]
    d = rules[int(group[lo])]
    assert d == T._opt_args(T.Adam(0.001, (0.9, 0.999), 1e-8))
    assert d != T._opt_args(T.TrainConfig().opt)        # not TrainConfig's Adam(0.01)


def test_unknown_keys_warn_and_are_ignored():
    m = _single()
    with pytest.warns(UserWarning, match=r"Per-branch optimizer keys not found in parameter tree, ignored: \[:RUE, :foo\]"):
        group, rules = T._opt_groups({"ps": T.Adam(0.01), "RUE": T.Descent(0.1), "foo": T.Adam(1.0), "Q10": T.Descent(0.2)}, m)
    assert len(rules) == 2 and rules[1] == T._opt_args(T.Descent(0.2))


def test_equal_rules_merge_to_the_single_rule_path():
    m = _multi()
    group, rules = T._opt_groups({"rb": T.Adam(0.01), "Q10": T.Adam(0.01)}, m)
    assert group is None and rules == [T._opt_args(T.Adam(0.01))]
    # every branch left out: all take the default, one rule
    group, rules = T._opt_groups({}, m)
    assert group is None and rules == [T._opt_args(T.Adam(0.001))]
    # equal after the float32 rounding eh_opt_init applies
    group, rules = T._opt_groups({"rb": T.Adam(0.1), "Q10": T.Adam(float(np.float32(0.1)))}, m)
    assert group is None


def test_single_rule_is_unchanged():
    group, rules = T._opt_groups(T.RMSProp(0.01), _single())
    assert group is None and rules == [T._opt_args(T.RMSProp(0.01))]


def test_state_tree_values_are_refused_naming_the_key():
    with pytest.raises(NotImplementedError, match="'Q10'"):
        T._opt_groups({"ps": T.Adam(0.01), "Q10": {"state": np.zeros(1)}}, _single())


def test_sixteen_group_limit():
    names = [f"g{k}" for k in range(17)]

    class Stub:                          # (17 global parameters: the resolution on a stand-in tree)
        n_theta = 17

        def opt_branches(self):
            return {n: (k, k + 1) for k, n in enumerate(names)}
    with pytest.raises(NotImplementedError, match="at most 16"):
        T._opt_groups({n: T.Descent(0.01 * (k + 1)) for k, n in enumerate(names)}, Stub())
    group, rules = T._opt_groups({n: T.Descent(0.01 * (min(k, 15) + 1)) for k, n in enumerate(names)}, Stub())
    assert len(rules) == 16 and group[15] == 15 and group[16] == 15
