"""The ordered one-kernel step's early election (EhOrd, csrc/eh_device.hpp: eh_ord_ticket, eh_ord_publish): the group's ticket is taken
behind the first barrier of the workgroup reduction, long before the rows are staged, so the folder regularly meets a row that is still
on its way and folds again in wait rounds.  Every comparison is against the deterministic step + reduce pair ("fused_update" 0) with
exact equality on the losses, theta, m, v and the beta powers.

The wait rounds are made certain with a test-only define of the run-time compiled kernels, EH_TEST_ORD_LATE_ROW=k: member k of every
group waits some 20 us between its ticket and its row stores -- five orders of magnitude under the hand-off's deadline, which no test
here lets expire.  The kernels built ahead of time never contain the define."""
import time

import numpy as np
import pytest

from tests import util
from tests.test_gpu_ordered_handoff import GRIDS, _same, _state, _windows

pytestmark = pytest.mark.gpu

WG = 256                      # samples per workgroup of the RbQ10 kernels (16 x NT 2 x NW 8)
N = 256 * WG + 4096


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one compilation per (descriptor, defines) for the whole module: the cache key covers the defines"""
    return str(tmp_path_factory.mktemp("eh_jit_cache"))


@pytest.fixture(scope="module")
def cases():
    # n_theta 338: the last wave of the folder folds the scalars; 642: wave 0 does, and a thread of the prologue owns more than one vector
    out = {338: util.rbq10_case(N, "tanh", True, 0.05), 642: util.rbq10_case(N, "tanh", True, 0.05, hidden=(32, 16)),
           "small": util.rbq10_case(70000, "tanh", True, 0.05)}
    assert out[338][1].size == 338 and out[642][1].size == 642
    return out


_REF = {}                     # (case key, script key) -> the pair's losses and state: computed once, shared, left unchanged


def _engine(mode, case, jit=None, env=None):
    """jit = None: the kernels built ahead of time; else the defines of kernels compiled at run time (env = (monkeypatch, cache dir))"""
    spec, theta, X, f, y = case
    if jit is not None:
        mp, cache = env
        mp.setenv("EH_JIT_CACHE", cache)
        if jit:
            mp.setenv("EH_JIT_DEFINES", jit)
        else:
            mp.delenv("EH_JIT_DEFINES", raising=False)
    e = util.load_engine(spec, theta, X, f, y, engine=util.model_from_spec(spec).engine())
    e.opt_init("Adam", 0.01)
    if jit is not None:
        e.set_option("aot_spec", 0)
        e.set_option("specialize", 1)
    e.set_option("fused_update", mode)
    return e


def _reference(key, case, script, jit, env):
    """the pair on the kernels of the same build as the ordered step's: built ahead of time, or compiled at run time (no defines: none
    of them touches the pair's kernels) -- the two binaries differ in the last bit of some gradient sums"""
    key = key + (jit is not None,)
    if key not in _REF:
        e = _engine(0, case, None if jit is None else "", env)
        l0 = script(e); e.synchronize(); s0 = _state(e); e.close()
        _REF[key] = (l0, s0)
    return _REF[key]


def _compare(key, case, script, ref_script=None, jit=None, env=None, finite=True):
    """script(engine) on the ordered step against (ref_script or script)(engine) on the pair: losses and state, bit for bit.
    synchronize raises when a hand-off ran into its deadline (the error word)"""
    e = _engine(2, case, jit, env)
    l2 = script(e); e.synchronize(); s2 = _state(e)
    if jit is not None:
        njit, jlog = e.jit_status()
        assert njit >= 1 and not jlog.startswith("ahead-of-time"), "the run-time compiled kernel did not run: " + jlog[:300]
    e.close()
    l0, s0 = _reference(key, case, ref_script or script, jit, env)
    assert not finite or np.all(np.isfinite(s0[0]))
    _same(l0, l2)
    _same(s0, s2)
    return l2, s2


def _win(grid, at):
    """a window of `grid` workgroups, the last of them ragged"""
    c = grid * WG - 37
    return (at % (N - c + 1), c)


def _grid_steps(grids):
    """every grid once with its update left to the next step's prologue, then once more with its loss asked for (the flush kernel)"""
    def script(e):
        for k, g in enumerate(grids):
            e.train_step(*_win(g, 911 * k + 5), want_loss=False)
        return [e.train_step(*_win(g, 613 * k + 1)) for k, g in enumerate(grids)]
    return script


# groups of one member (the folder alone: nothing to wait for), two, three, and the full sixteen
LATE_GRIDS = [2, 17, 33, 255, 256]


@pytest.mark.parametrize("n_theta", [338, 642])
@pytest.mark.parametrize("k", [0, 1, 15])
def test_late_row_goes_through_the_wait_rounds(cases, k, n_theta, monkeypatch, jit_cache):
    """member k of every group that has one stores its row 20 us late: its folder meets the marker in the gradient vectors and in the
    scalar vector.  (k = 15 exists at grid 256 only; the steps of the other grids run the plain path of the same binary.)"""
    _compare((n_theta, "late"), cases[n_theta], _grid_steps(LATE_GRIDS), jit=f"EH_TEST_ORD_LATE_ROW={k}", env=(monkeypatch, jit_cache))


@pytest.mark.parametrize("k", [0, 1])
def test_delayed_member_is_the_last_ticket(cases, k, monkeypatch, jit_cache):
    """groups of one member (k = 0: the delayed workgroup is its group's folder and takes its own row from LDS) and of two (k = 1: the
    second member, dispatched last, is delayed and as a rule takes the last ticket as well)"""
    _compare((338, "small groups"), cases[338], _grid_steps([2, 3, 16, 17, 18, 31, 32, 2]), jit=f"EH_TEST_ORD_LATE_ROW={k}", env=(monkeypatch, jit_cache))


def _handoff_steps(windows):
    def script(e):
        return [e.train_step(a, c) for a, c in windows]
    return script


@pytest.mark.parametrize("defines", ["", "EH_AB_ORD_TICKET_LATE", "EH_AB_ORD_TICKET_AT=8", "EH_AB_ORD_TICKET_AT=13", "EH_AB_ORD_TICKET_AT=14", None],
                         ids=["default", "late", "at8", "at13", "at14", "aot"])
def test_election_equivalence(cases, defines, monkeypatch, jit_cache):
    """grids that shrink and grow, one workgroup in between: wherever the ticket is taken, the pair's bits"""
    _compare(("small", "grids"), cases["small"], _handoff_steps(_windows(70000, GRIDS)), jit=defines, env=(monkeypatch, jit_cache))


def test_rows_and_a_minibatch_without_a_valid_target_with_a_late_row(cases, monkeypatch, jit_cache):
    spec, theta, X, f, y = cases[338]
    y = {k: v.copy() for k, v in y.items()}
    for v in y.values():
        v[3 * WG:6 * WG] = np.nan                        # workgroups 3, 4, 5 of a window at 0: their rows carry n = 0
        v[19 * WG:20 * WG] = np.nan                      # workgroup 19: member 1 of group 3, the delayed one
        v[20000:26000] = np.nan                          # a window without a valid target: no update
    case = (spec, theta, X, f, y)
    w = [(0, 40 * WG - 5), (20000, 6000), (0, 33 * WG), (20100, 5000), (20200, 600), (WG, 30 * WG - 1)]

    def script(e):
        for a, c in w:
            e.train_step(a, c, want_loss=False)
        return [e.train_step(a, c) for a, c in w]
    _compare((338, "masked"), case, script, jit="EH_TEST_ORD_LATE_ROW=1", env=(monkeypatch, jit_cache))


def test_genuine_nan_passes_after_one_look_with_a_late_row(cases, monkeypatch, jit_cache):
    """a NaN air temperature in one sample of workgroup 5 of a window at 0 (40 workgroups: group 5 has rows 5, 21, 37, and 21 is late)
    goes through the mechanistic model into the loss and every gradient element; from the second step on every sum is a NaN.  A NaN
    taken for a row that has not arrived would wait for the 2 s deadline, per step, and set the error word"""
    spec, theta, X, f, y = cases[338]
    f = {k: v.copy() for k, v in f.items()}
    f["ta"][5 * WG + 17] = np.nan
    case = (spec, theta, X, f, y)
    took = []

    def script(e):
        e.train_step(10000, 9000, want_loss=False)       # (a finite step first: the kernels are loaded)
        e.synchronize()
        t0 = time.perf_counter()
        out = [e.train_step(0, 40 * WG - 37)]            # loss and gradient NaN; flushed
        e.train_step(0, 40 * WG - 37, want_loss=False)   # every sum NaN from here on; consumed by the next prologue
        out.append(e.train_step(10000, 9000))
        e.synchronize()
        took.append(time.perf_counter() - t0)
        return out
    losses, state = _compare((338, "nan"), case, script, jit="EH_TEST_ORD_LATE_ROW=1", env=(monkeypatch, jit_cache), finite=False)
    assert np.isnan(losses[0]) and np.isnan(state[0]).any()
    assert max(took) < 1.0, took


def test_500_steps_back_to_back_at_grid_256(cases):
    def script(e):
        for k in range(500):
            e.train_step((k % 16) * WG, 256 * WG, want_loss=False)
        return []
    _compare((338, "500"), cases[338], script)


def test_graph_of_mixed_grids_replayed_with_flush_between(cases):
    w = [_win(g, 3000 * k + 9) for k, g in enumerate((256, 17, 2, 129, 40, 256))]

    def between(e):
        # two flushes between the replays, and a step of the recorded grid in front of the next replay, its update left pending (no
        # loss asked for): the slots' rotation comes back to the recorded state
        for at in (5, 900):
            e.synchronize()
            e.train_step(*_win(256, at), want_loss=False)

    def script(e):
        e.train_step(*_win(256, 5), want_loss=False)
        e.graph_begin()
        for a, c in w:
            e.train_step(a, c, want_loss=False)
        g = e.graph_end()
        for _ in range(2):
            e.graph_launch(g)
            between(e)
        return [e.train_step(*_win(256, 77))]

    def plain(e):
        e.train_step(*_win(256, 5), want_loss=False)
        for _ in range(2):
            for a, c in w:
                e.train_step(a, c, want_loss=False)
            between(e)
        return [e.train_step(*_win(256, 77))]
    _compare((338, "graph"), cases[338], script, plain)
