"""The ordered one-kernel step's plain group rows and early row stores (EhOrd, csrc/eh_device.hpp: eh_ord_publish, eh_ord_row_early).

Plain group rows (the default; EH_AB_ORD_GROW_WT restores the write-through stores): the folder's group row and block partials are plain
stores, which the end of the kernel publishes to the next kernel on the stream, their only reader.
Early row stores (EH_AB_ORD_ROWS_EARLY on run-time compiled kernels; measured and left off by default): every workgroup stores its row
out of the registers of the gather that has just summed it -- the gradient vectors packed inside the quads, the scalar vector taken out
of the wave that holds it -- in front of the staged barrier, the later folder included.

Both move data only: every comparison is against the deterministic step + reduce pair ("fused_update" 0) with exact equality on the
losses, theta, m, v and the beta powers, and every engine is synchronised (a hand-off that ran into its deadline raises there).

Shapes (n_theta = (h1 + 2)(h2 + 3) - 4 for hidden (h1, h2); the gather's thread e sums element e, 512 threads):
  338  the last gradient vector is half full; the scalar vector sits in lanes 18-21 of wave 5, not a quad
  320  a multiple of four: the scalar vector is a quad of its own
  642  a thread gathers two elements (two rounds of stores), and wave 0 folds the scalars
  126  hidden (8, 10): the scalar vector begins in lane 62 of wave 1 and ends in lane 1 of wave 2 -- the one vector that thread 0 still
       stores from the staging behind the barrier on the early path (eh_ord_scalars_split)
The test-only EH_TEST_ORD_LATE_ROW=k delays, on the early path, every wave of member k in front of its early stores: the folder meets the
marker and goes through the wait rounds.  No test here lets the hand-off's deadline expire."""
import ctypes as C
import re
import time

import numpy as np
import pytest

from tests import util
from tests.test_gpu_ordered_handoff import _same, _state
from tests.test_gpu_ordered_ticket import N, WG, _engine, _grid_steps, _reference, _win

pytestmark = pytest.mark.gpu

HIDDEN = {338: (16, 16), 320: (16, 15), 642: (32, 16), 126: (8, 10)}
# 2; 17: groups of two members and of one; 33; 256 (every window is ragged: the last workgroup is 37 samples short);
# 256 -> 17 -> 256 leaves the rows and partials of the larger grid stale under the smaller one
GRIDS = [2, 17, 33, 256, 17, 256]
EARLY = "EH_AB_ORD_ROWS_EARLY"
N_GRID_STEPS = 2 * len(GRIDS)     # _grid_steps: every grid twice, none of them one workgroup


def _compare(key, case, script, ref_script=None, jit=None, env=None, finite=True, n_ord=None):
    """script(engine) on the ordered step against (ref_script or script)(engine) on the pair: losses and state, bit for bit.
    synchronize raises when a hand-off ran into its deadline (the error word).  The engine must say that its steps ran as the ordered
    one-kernel step -- n_ord of them where the script's count is known -- and not as the pair it is compared with: a shape that
    quietly fell back would pass every comparison"""
    e = _engine(2, case, jit, env)
    l2 = script(e); e.synchronize(); s2 = _state(e)
    njit, jlog = e.jit_status()
    if jit is not None:
        assert njit >= 1 and not jlog.startswith("ahead-of-time"), "the run-time compiled kernel did not run: " + jlog[:300]
    m = re.search(r"ordered steps: (\d+)", jlog)
    assert m is not None, "no step ran as the ordered one-kernel step: " + jlog[-300:]
    # (a run-time compiled kernel takes the ordered step only once the pair's first step has checked it, step_launch in csrc/eh_api.hip:
    #  the first step of such an engine is the pair by design, every later one the ordered kernel)
    assert n_ord is None or int(m.group(1)) == n_ord - (jit is not None), (m.group(0), n_ord)
    e.close()
    l0, s0 = _reference(key, case, ref_script or script, jit, env)
    assert not finite or np.all(np.isfinite(s0[0]))
    _same(l0, l2)
    _same(s0, s2)
    return l2, s2


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one compilation per (descriptor, defines) for the whole module"""
    return str(tmp_path_factory.mktemp("eh_jit_cache"))


@pytest.fixture(scope="module")
def cases():
    out = {n: util.rbq10_case(N, "tanh", True, 0.05, hidden=h) for n, h in HIDDEN.items()}
    for n, c in out.items():
        assert c[1].size == n
    return out


@pytest.mark.parametrize("n_theta", sorted(HIDDEN))
def test_kernels_built_ahead_of_time(cases, n_theta):
    _compare((n_theta, "early grids"), cases[n_theta], _grid_steps(GRIDS), n_ord=N_GRID_STEPS)


@pytest.mark.parametrize("defines", ["", EARLY, "EH_AB_ORD_GROW_WT", EARLY + " EH_AB_ORD_GROW_WT", EARLY + " EH_AB_ORD_FOLDER_SLEEP=5"],
                         ids=["default", "rows_early", "grow_wt", "both", "rows_early_pause"])
def test_run_time_compiled_switches(cases, defines, monkeypatch, jit_cache):
    _compare((338, "early grids"), cases[338], _grid_steps(GRIDS), jit=defines, env=(monkeypatch, jit_cache), n_ord=N_GRID_STEPS)


@pytest.mark.parametrize("defines", ["", EARLY], ids=["default", "rows_early"])
@pytest.mark.parametrize("n_theta", [126, 320, 642])
def test_run_time_compiled_shapes(cases, n_theta, defines, monkeypatch, jit_cache):
    _compare((n_theta, "early grids"), cases[n_theta], _grid_steps(GRIDS), jit=defines, env=(monkeypatch, jit_cache), n_ord=N_GRID_STEPS)


@pytest.mark.parametrize("defines,early", [("", False), (EARLY, True), (EARLY + " EH_AB_ORD_ROW_SCALARS", False)],
                         ids=["default", "rows_early", "rows_early_row_scalars"])
def test_the_define_selects_the_early_path(cases, defines, early, monkeypatch, jit_cache):
    """a mistyped or ignored define would leave every comparison above on the staged path: the diagnostic stamps say which path ran.
    Slot [6] of a folder's tail (EH_ORD_ST_TAIL + 32 g + 2 * 6, csrc/eh_device.hpp) is the clock in front of the gather, written by the
    early path only; slot [0] is written by every ordered step.  (An armed stamp buffer runs the general form of the kernel.)"""
    ST_TAIL, TAILW = 256, 32                             # EH_ORD_ST_TAIL, EH_ORD_ST_TAILW
    words = ST_TAIL + TAILW * 16
    e = _engine(2, cases[338], "EH_STAMPS " + defines, (monkeypatch, jit_cache))
    buf = (C.c_uint64 * words)()
    assert e._lib.eh_debug_stamps(e._h, buf, words) == 0  # arms the buffer
    for k in range(3):
        e.train_step(*_win(256, 700 * k + 3), want_loss=False)
    assert e._lib.eh_debug_stamps(e._h, buf, words) == 0  # (synchronises)
    njit, jlog = e.jit_status()
    e.close()
    assert njit >= 1 and "ordered steps: 2" in jlog, jlog[-300:]      # (the first step of a run-time compiled engine is the pair)
    tail = np.array(list(buf), dtype=np.uint64)[ST_TAIL:].reshape(16, TAILW)
    assert np.all(tail[:, 0] > 0), "no folder stamped its tail: the ordered kernel's stamps did not run"
    assert np.all((tail[:, 12] > 0) == early), tail[:, 12]


@pytest.mark.parametrize("n_theta,k", [(338, 0), (338, 7), (338, 15), (642, 1), (126, 1)])
def test_late_member_on_the_early_path(cases, n_theta, k, monkeypatch, jit_cache):
    """member k of every group that has one stores its row 20 us late (the first, a middle and the last member; members 7 and 15 exist
    at grid 256 only): its folder, which does not pause on this path, meets the marker in the gradient vectors and in the scalar vector
    and folds again"""
    _compare((n_theta, "early grids"), cases[n_theta], _grid_steps(GRIDS), jit=f"{EARLY} EH_TEST_ORD_LATE_ROW={k}", env=(monkeypatch, jit_cache),
             n_ord=N_GRID_STEPS)


@pytest.mark.parametrize("k", [0, 7, 15])
def test_late_member_with_plain_group_rows(cases, k, monkeypatch, jit_cache):
    """the same on the default path (staged rows, plain group rows)"""
    _compare((338, "early grids"), cases[338], _grid_steps(GRIDS), jit=f"EH_TEST_ORD_LATE_ROW={k}", env=(monkeypatch, jit_cache), n_ord=N_GRID_STEPS)


def test_genuine_nan_passes_after_one_look(cases, monkeypatch, jit_cache):
    """a NaN air temperature in one sample of workgroup 5 of a window at 0 (40 workgroups) goes through the mechanistic model into the
    loss and every gradient element of that row, which on the run-time compiled kernels is also the late one; from the second step on
    every sum is a NaN.  A NaN taken for a row that has not arrived would wait for the 2 s deadline, per step, and set the error word"""
    spec, theta, X, f, y = cases[338]
    f = {k: v.copy() for k, v in f.items()}
    f["ta"][5 * WG + 17] = np.nan
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
    for jit in (None, "EH_TEST_ORD_LATE_ROW=0", EARLY + " EH_TEST_ORD_LATE_ROW=0"):
        losses, state = _compare((338, "early nan"), (spec, theta, X, f, y), script, jit=jit, env=(monkeypatch, jit_cache), finite=False,
                                 n_ord=4)
        assert np.isnan(losses[0]) and np.isnan(state[0]).any()
    assert max(took) < 1.0, took


def test_graph_replayed_with_flush_between(cases):
    w = [_win(g, 3000 * k + 9) for k, g in enumerate((256, 17, 2, 256, 33, 256))]

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
        for _ in range(3):
            e.graph_launch(g)
            between(e)
        return [e.train_step(*_win(256, 77))]

    def plain(e):
        e.train_step(*_win(256, 5), want_loss=False)
        for _ in range(3):
            for a, c in w:
                e.train_step(a, c, want_loss=False)
            between(e)
        return [e.train_step(*_win(256, 77))]
    _compare((338, "early graph"), cases[338], script, plain)
