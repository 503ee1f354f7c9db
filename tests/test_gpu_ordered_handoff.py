"""The ordered one-kernel step's hand-off (EhOrd, csrc/eh_device.hpp): rows marked "not written" by a signalling NaN instead of drained
before the ticket, and the rows' scalars folded on the DPP network.  Checked against the deterministic step + reduce pair
("fused_update" 0) with exact equality, where the marker's invariant is easiest to break: grids that change from step to step (rows that
one step writes and the next does not), switches between the step forms, recorded graphs replayed with steps of different grids, grouped
optimiser rules and a minibatch without a valid target."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

WG = 256                      # samples per workgroup of the headline kernels (16 x NT 2 x NW 8)


def _engine(mode, case, aot=1, groups=False):
    spec, theta, X, f, y = case
    model = util.model_from_spec(spec)
    e = util.load_engine(spec, theta, X, f, y, engine=model.engine())
    e.set_option("aot_spec", aot)
    if groups:                # two rules: the network's weights (Adam) and the global parameters (AdamW)
        group = np.zeros(e.n_theta, np.int32)
        group[-1:] = 1
        e.opt_init_groups(group, [dict(rule="Adam", lr=0.01), dict(rule="AdamW", lr=0.005, weight_decay=0.01)])
    else:
        e.opt_init("Adam", 0.01)
    e.set_option("fused_update", mode)
    return e


def _state(e):
    th = e.get_params().copy()
    m, v, bt = e.get_opt_state()
    return [th, m.copy(), v.copy(), np.asarray(bt).copy()]


def _same(a, b):
    assert len(a) == len(b)
    for u, w in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(w), equal_nan=True)


def _compare(case, script, ref_script=None, **kw):
    """script(engine) on the ordered step against (ref_script or script)(engine) on the pair: losses and state, bit for bit"""
    e = _engine(2, case, **kw)
    l2 = script(e); e.synchronize(); s2 = _state(e); e.close()
    e = _engine(0, case, **kw)
    l0 = (ref_script or script)(e); e.synchronize(); s0 = _state(e); e.close()
    assert np.all(np.isfinite(s0[0]))
    _same(l0, l2)
    _same(s0, s2)


# grids 1 ... 256 in an order that shrinks and grows them: 16-multiples and not, one workgroup (the float one-kernel step, one
# fixed order there), the full 256
GRIDS = [2, 256, 3, 17, 255, 1, 16, 33, 129, 31, 200, 2, 64, 256, 7, 1, 100, 18]


def _windows(n, grids, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for g in grids:
        c = int(g * WG - rng.integers(0, WG - 1)) if g > 1 else int(rng.integers(1, WG))
        out.append((int(rng.integers(0, n - c + 1)), c))
    return out


def _steps(windows):
    def script(e):
        return [e.train_step(a, c) for a, c in windows]
    return script


@pytest.mark.parametrize("aot", [1, 0])
def test_grids_that_change_every_step(aot):
    n = 70000
    case = util.rbq10_case(n, "tanh", True, 0.05)
    _compare(case, _steps(_windows(n, GRIDS)), aot=aot)


def test_grids_that_change_every_step_grouped_rules():
    n = 70000
    case = util.rbq10_case(n, "tanh", True, 0.05)
    _compare(case, _steps(_windows(n, GRIDS, seed=5)), groups=True)


def test_switch_ordered_float_pair_ordered():
    """2 -> 1 -> 0 -> 2 with training after each switch and an update pending at each.  The float-atomic steps get minibatches of one
    workgroup, where their sums meet in one order too, so the reference (0 -> 1 -> 0 -> 0) gives the same bits"""
    n = 40000
    case = util.rbq10_case(n, "tanh", True, 0.05)
    big = _windows(n, [40, 9, 130, 2, 77], seed=11)
    small = _windows(n, [1, 1, 1], seed=12)

    def run(modes):
        def script(e):
            out = []
            for mode, w in zip(modes, (big, small, big, big)):
                e.set_option("fused_update", mode)
                out += [e.train_step(a, c) for a, c in w]
            return out
        return script
    _compare(case, run((2, 1, 0, 2)), run((0, 1, 0, 0)))


def test_graph_with_changing_grids_replayed():
    n = 30000
    case = util.rbq10_case(n, "tanh", True, 0.05)
    first = (0, 8 * WG)
    # six steps (the fused modes' rotation comes back after six), the last of the same grid as the step in front of the recording
    w = [(100, 300), (2000, 9000), (500, 4500), (7000, 16 * WG + 1), (1234, 700), (4000, 8 * WG)]

    def script(e):
        e.train_step(*first, want_loss=False)
        e.graph_begin()
        for a, c in w:
            e.train_step(a, c, want_loss=False)
        g = e.graph_end()
        for _ in range(4):
            e.graph_launch(g)
        e.synchronize()
        return [e.train_step(0, 5000)]

    def plain(e):
        e.train_step(*first, want_loss=False)
        for _ in range(4):
            for a, c in w:
                e.train_step(a, c, want_loss=False)
        return [e.train_step(0, 5000)]
    _compare(case, script, plain)


def test_all_masked_minibatch_between_changing_grids():
    n = 30000
    spec, theta, X, f, y = util.rbq10_case(n, "tanh", True, 0.1)
    y = {k: v.copy() for k, v in y.items()}
    for v in y.values():
        v[10000:14000] = np.nan                          # a window without a valid target
    case = (spec, theta, X, f, y)
    w = [(0, 9000), (10000, 4000), (200, 3000), (10500, 3000), (15000, 12000), (10000, 4000), (3, 700)]
    _compare(case, _steps(w))
