"""The ordered one-kernel step's scalars [S | n | Sy | Syy] (EhOrd, csrc/eh_device.hpp): the last arriver of every row group folds its
group's rows into the four block partials of eh_reduce_kernel<true, 16>'s butterfly (its levels xor 32 and xor 16, which never leave a
group), the next prologue -- or eh_ord_flush_kernel -- reads one 16-byte vector per lane and finishes the butterfly.  The rows' scalar
vector is under the "not written" marker like a gradient vector.

The first test is the index map's specification: a float32 emulation of the butterfly as the reduce kernel runs it against the regrouped
form, for every grid.  The others run the ordered step ("fused_update" 2) against the deterministic step + reduce pair ("fused_update" 0)
with exact equality, at the edges of blocks and groups, over stale partials of absent groups, over rows without a valid target, with a
genuine NaN (which must pass the marker's check, not wait in it), through the flush kernel, back to back and in a recorded graph."""
import time

import numpy as np
import pytest

from tests import util

gpu = pytest.mark.gpu

WG = 256                      # samples per workgroup of the RbQ10 kernels (16 x NT 2 x NW 8)
ROWS, GROUPS = 256, 16        # EH_ORD_ROWS, EH_ORD_GROUPS


# ---- the specification: float32, no GPU -----------------------------------------------------------------------------------------------
def _butterfly_as_written(rows, grid):
    """eh_reduce_kernel<true, 16>: thread r holds 0 + row r (0 past the grid), an xor butterfly 32 ... 1 per 64 rows, (w0 + w1) + (w2 + w3)"""
    c = np.zeros((ROWS, 4), np.float32)
    c[:grid] = np.float32(0.0) + rows[:grid]
    lanes = np.arange(64)
    w = []
    for b in range(4):
        s = c[64 * b:64 * b + 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[lanes ^ off]
        assert all(np.array_equal(s[0].view(np.uint32), s[l].view(np.uint32)) for l in range(64))
        w.append(s[0])
    return (w[0] + w[1]) + (w[2] + w[3])


def _tail_partials(rows, grid, part, quads):
    """eh_ord_publish: the last arriver of group i writes part[q][i] = (c[4q] + c[4q+2]) + (c[4q+1] + c[4q+3]), c[k] = 0 + row i + 16 k of
    the group (0 past its end); absent groups keep what they held.  quads: as the kernel forms it, lane k holding c[k] -- two adds within
    the quad (partner k ^ 2, then k ^ 1), the quad's first lane stores"""
    zero = np.zeros(4, np.float32)
    lanes = np.arange(ROWS // GROUPS)
    for i in range(min(grid, GROUPS)):
        gsz = (grid - i + GROUPS - 1) // GROUPS
        c = np.stack([zero + rows[i + GROUPS * k] if k < gsz else zero + zero for k in lanes])
        if not quads:
            for q in range(4):
                part[q, i] = (c[4 * q] + c[4 * q + 2]) + (c[4 * q + 1] + c[4 * q + 3])
        else:
            s = c + c[lanes ^ 2]
            s = s + s[lanes ^ 1]
            for q in range(4):
                assert all(np.array_equal(s[4 * q].view(np.uint32), s[4 * q + j].view(np.uint32)) for j in range(4))
                part[q, i] = s[4 * q]


def _prologue_fold(part, prev_grid):
    """eh_ord_scalar_loads / eh_ord_scalar_fold: lane 16 q + i takes part[q][i] (0 where the pending step had no group i), xor 8 ... 1
    within its row of 16, the four rows' sums as (w0 + w1) + (w2 + w3)"""
    s = part.reshape(64, 4).copy()                      # [q][i][4] is lane 16 q + i's vector
    lanes = np.arange(64)
    s[(lanes & 15) >= prev_grid] = 0.0
    for off in (8, 4, 2, 1):
        s = s + s[lanes ^ off]
    return (s[0] + s[16]) + (s[32] + s[48])


def test_regrouped_butterfly_is_the_reduce_kernels_for_every_grid():
    rng = np.random.default_rng(20)
    bad = []
    part = (rng.standard_normal((4, GROUPS, 4)) * 1e6).astype(np.float32)       # stale from the start: never reset between the grids
    part[0, 3] = np.nan
    order = list(range(2, ROWS + 1))
    rng.shuffle(order)                                   # grids shrink and grow: absent groups keep stale partials
    for n, grid in enumerate(order):
        mag = 10.0 ** rng.integers(-3, 4, size=(ROWS, 4))                       # six decades
        rows = (rng.standard_normal((ROWS, 4)) * mag).astype(np.float32)
        rows[rng.random((ROWS, 4)) < 0.05] = -0.0
        if n % 7 == 0:
            rows[:, 1] = -0.0                            # a whole column of - 0: the sum is + 0 in both forms
        rows[grid:] = rng.standard_normal((ROWS - grid, 4)).astype(np.float32) * np.float32(1e9)       # rows past the grid: garbage
        want = _butterfly_as_written(rows, grid)
        for quads in (False, True):
            _tail_partials(rows, grid, part, quads)
            got = _prologue_fold(part, grid)
            if not np.array_equal(want.view(np.uint32), got.view(np.uint32)):
                bad.append((grid, quads, want, got))
    assert not bad, bad[:3]


# ---- on the GPU: ordered step against the pair ----------------------------------------------------------------------------------------
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


def _compare(case, script, ref_script=None, finite=True, **kw):
    """script(engine) on the ordered step against (ref_script or script)(engine) on the pair: losses and state, bit for bit.
    synchronize raises when a hand-off ran into its deadline"""
    e = _engine(2, case, **kw)
    l2 = script(e); e.synchronize(); s2 = _state(e); e.close()
    e = _engine(0, case, **kw)
    l0 = (ref_script or script)(e); e.synchronize(); s0 = _state(e); e.close()
    assert not finite or np.all(np.isfinite(s0[0]))
    _same(l0, l2)
    _same(s0, s2)
    return l2, s2


def _win(n, grid, at):
    """a window of `grid` workgroups, the last of them ragged"""
    c = grid * WG - 37
    return (at % (n - c + 1), c)


def _steps(n, grids):
    """every grid once with its update left to the next step's prologue, then once more with its loss asked for (the flush kernel)"""
    def script(e):
        for k, g in enumerate(grids):
            e.train_step(*_win(n, g, 911 * k + 5), want_loss=False)
        return [e.train_step(*_win(n, g, 613 * k + 1)) for k, g in enumerate(grids)]
    return script


N = 256 * WG + 4096
EDGES = [2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 191, 192, 193, 255, 256]


@pytest.fixture(scope="module")
def case338():
    return util.rbq10_case(N, "tanh", True, 0.05)


@gpu
@pytest.mark.parametrize("aot", [1, 0], ids=["aot", "jit"])
def test_block_and_group_edges(case338, aot):
    _compare(case338, _steps(N, EDGES), aot=aot)


@gpu
def test_block_and_group_edges_grouped_rules(case338):
    _compare(case338, _steps(N, EDGES), groups=True)


@gpu
def test_stale_partials_of_absent_groups(case338):
    _compare(case338, _steps(N, [256, 5, 256, 16, 3, 200, 2]))


@gpu
def test_rows_without_a_valid_target():
    spec, theta, X, f, y = util.rbq10_case(40000, "tanh", True, 0.05)
    y = {k: v.copy() for k, v in y.items()}
    for v in y.values():
        v[3 * WG:6 * WG] = np.nan                        # workgroups 3, 4, 5 of a window at 0: their rows carry n = 0
        v[19 * WG:20 * WG] = np.nan                      # workgroup 19: the second row of group 3
        v[20000:26000] = np.nan                          # a window without a valid target: no update
    case = (spec, theta, X, f, y)
    w = [(0, 40 * WG - 5), (20000, 6000), (0, 33 * WG), (20100, 5000), (20200, 600), (WG, 30 * WG - 1)]

    def script(e):
        for a, c in w:
            e.train_step(a, c, want_loss=False)
        return [e.train_step(a, c) for a, c in w]
    _compare(case, script)


@gpu
@pytest.mark.parametrize("where", ["predictor", "forcing"])
def test_genuine_nan_passes_the_marker(where):
    """One NaN input in one sample of workgroup 5 of a window at 0 (40 workgroups: group 5 has rows 5, 21, 37).  A NaN predictor does
    not survive the first tanh layer (eh_tanh saturates whatever fails x^2 < 66 to +-1), so that step stays finite on both sides;
    a NaN air temperature goes through the mechanistic model into the loss and every gradient element"""
    spec, theta, X, f, y = util.rbq10_case(20000, "tanh", True, 0.05)
    if where == "predictor":
        X = X.copy()
        X[0, 5 * WG + 17] = np.nan
    else:
        f = {k: v.copy() for k, v in f.items()}
        f["ta"][5 * WG + 17] = np.nan
    case = (spec, theta, X, f, y)
    took = []

    def script(e):
        e.train_step(10000, 9000, want_loss=False)       # (a finite step first: the kernels are loaded)
        e.synchronize()
        t0 = time.perf_counter()
        out = [e.train_step(0, 40 * WG - 37)]            # (forcing: loss and gradient NaN); flushed
        e.train_step(0, 40 * WG - 37, want_loss=False)   # (forcing: every sum NaN from here on); consumed by the next prologue
        out.append(e.train_step(10000, 9000))
        e.synchronize()
        took.append(time.perf_counter() - t0)
        return out
    losses, state = _compare(case, script, finite=False)
    if where == "forcing":
        assert np.isnan(losses[0]) and np.isnan(state[0]).any()
    # a NaN mistaken for a row that has not arrived would wait for the 2 s deadline (and set the error word, which synchronize raises)
    assert max(took) < 1.0, took


@gpu
def test_flush_path_then_further_steps(case338):
    def script(e):
        out = []
        for k, g in enumerate((17, 256, 17, 256)):
            e.train_step(*_win(N, g, 777 * k + 3), want_loss=False)
            e.synchronize()                              # eh_ord_flush_kernel takes the pending step
            out.append(e.get_params().copy())
            e.train_step(*_win(N, 256 if k & 1 else 40, 55 * k), want_loss=False)
            out.append(e.train_step(*_win(N, g, 31 * k + 9)))
        return out
    _compare(case338, script)


@gpu
def test_back_to_back_without_synchronisation(case338):
    def script(e):
        for k in range(500):
            e.train_step((k % 16) * WG, 256 * WG, want_loss=False)
        return []
    _compare(case338, script)


@gpu
@pytest.mark.parametrize("hidden, n_theta", [((16, 16), 338), ((32, 16), 642), ((11, 17), 256), ((25, 16), 509)], ids=["n338", "n642", "n256", "n509"])
def test_other_row_lengths(hidden, n_theta):
    """n_theta 256 and 509: ceil(n_theta / 4) is 64 and 128, so the scalar vector's thread in the tail is the first of a wave that has
    no gradient vector"""
    case = util.rbq10_case(N, "tanh", True, 0.05, hidden=hidden)
    assert case[1].size == n_theta
    _compare(case, _steps(N, [256, 17, 64, 3, 129, 256]))


@gpu
def test_one_graph_of_mixed_grids_replayed_with_flush_between(case338):
    w = [_win(N, g, 3000 * k + 9) for k, g in enumerate((256, 17, 2, 129, 40, 256))]

    def between(e):
        # two flushes between the replays, and a step of the recorded grid in front of the next replay, its update left pending (no
        # loss asked for): the slots' rotation comes back to the recorded state
        for at in (5, 900):
            e.synchronize()
            e.train_step(*_win(N, 256, at), want_loss=False)

    def script(e):
        e.train_step(*_win(N, 256, 5), want_loss=False)
        e.graph_begin()
        for a, c in w:
            e.train_step(a, c, want_loss=False)
        g = e.graph_end()
        for _ in range(2):
            e.graph_launch(g)
            between(e)
        return [e.train_step(*_win(N, 256, 77))]

    def plain(e):
        e.train_step(*_win(N, 256, 5), want_loss=False)
        for _ in range(2):
            for a, c in w:
                e.train_step(a, c, want_loss=False)
            between(e)
        return [e.train_step(*_win(N, 256, 77))]
    _compare(case338, script, plain)
