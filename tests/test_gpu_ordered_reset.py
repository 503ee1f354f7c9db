"""Who writes the "not written" marker back into the ordered step's rows (EhOrd, csrc/eh_device.hpp): the consumer of a pending ordered
step -- the next ordered step's prologue, or eh_ord_flush_kernel -- resets the rows of that step, workgroup b the rows b, b + grid, ...
A row left un-reset would be read as fresh by the step two launches on and change the bits; a row store that never lands would run into
the deadline, which eh_synchronize reports as EH_EHIP.  Every case is checked against the deterministic step + reduce pair
("fused_update" 0) with exact equality, and every engine is synchronised (the error word is read there)."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

WG = 256                      # samples per workgroup of the RbQ10 kernels (16 x NT 2 x NW 8)


def _engine(mode, case):
    spec, theta, X, f, y = case
    e = util.load_engine(spec, theta, X, f, y, engine=util.model_from_spec(spec).engine())
    e.opt_init("Adam", 0.01)
    e.set_option("fused_update", mode)
    return e


def _state(e):
    th = e.get_params().copy()
    m, v, bt = e.get_opt_state()
    return [th, m.copy(), v.copy(), np.asarray(bt).copy()]


def _compare(case, script):
    out = []
    for mode in (2, 0):
        e = _engine(mode, case)
        losses = script(e)
        e.synchronize()                     # (raises on EH_EHIP: a group's rows did not arrive)
        out.append((losses, _state(e)))
        e.close()
    (l2, s2), (l0, s0) = out
    assert np.all(np.isfinite(s0[0]))
    assert len(l0) == len(l2) and len(s0) == len(s2)
    for a, b in zip(l0 + s0, l2 + s2):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _win(n, grid, at):
    c = grid * WG - 37 if grid > 1 else 200
    return (at % (n - c), c)


def _flush_then_steps(n):
    def script(e):
        out = [e.train_step(*_win(n, 256, 11))]
        e.synchronize()                     # the flush kernel takes the pending 256-workgroup step
        for k, g in enumerate((2, 256, 2, 256)):
            out.append(e.train_step(*_win(n, g, 5000 * k + 3)))
        e.synchronize()
        out.append(e.train_step(*_win(n, 256, 7)))
        return out
    return script


def _shrink_grow(n):
    def script(e):
        # the 17-workgroup step resets the 256 rows of the step in front of it: each of its workgroups takes 15 or 16 of them
        return [e.train_step(*_win(n, g, 4000 * k + 1)) for k, g in enumerate((256, 17, 256, 17, 256, 256, 3, 256))]
    return script


N = 256 * WG + 4096


@pytest.mark.parametrize("hidden", [(16, 16), (16, 15), (32, 16)], ids=["n338", "n320", "n642"])
def test_flush_after_full_grid(hidden):
    """n_theta 338 (not a multiple of 4), 320 (a multiple of 4), 642 (more than two elements per thread)"""
    case = util.rbq10_case(N, "tanh", True, 0.05, hidden=hidden)
    _compare(case, _flush_then_steps(N))


@pytest.mark.parametrize("hidden", [(16, 16), (16, 15), (32, 16)], ids=["n338", "n320", "n642"])
def test_grid_shrinks_and_grows(hidden):
    case = util.rbq10_case(N, "tanh", True, 0.05, hidden=hidden)
    _compare(case, _shrink_grow(N))


def test_graph_replayed_with_flush_between():
    case = util.rbq10_case(N, "tanh", True, 0.05)
    w = [_win(N, g, 3000 * k + 9) for k, g in enumerate((256, 17, 2, 256, 40, 256))]

    def script(e):
        e.train_step(*_win(N, 256, 5), want_loss=False)
        e.graph_begin()
        for a, c in w:
            e.train_step(a, c, want_loss=False)
        g = e.graph_end()
        for _ in range(3):
            e.graph_launch(g)
            between(e)
        return [e.train_step(*_win(N, 256, 77))]

    def between(e):
        # two flushes between the replays (each resets the rows of a pending step), and a step of the recorded grid in front of the
        # next replay, its update left pending (no loss asked for): the rotation comes back to the recorded state
        for at in (5, 900):
            e.synchronize()
            e.train_step(*_win(N, 256, at), want_loss=False)

    def plain(e):
        e.train_step(*_win(N, 256, 5), want_loss=False)
        for _ in range(3):
            for a, c in w:
                e.train_step(a, c, want_loss=False)
            between(e)
        return [e.train_step(*_win(N, 256, 77))]

    out = []
    for mode, sc in ((2, script), (0, plain)):
        e = _engine(mode, case)
        losses = sc(e)
        e.synchronize()
        out.append((losses, _state(e)))
        e.close()
    (l2, s2), (l0, s0) = out
    assert np.all(np.isfinite(s0[0]))
    for a, b in zip(l0 + s0, l2 + s2):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
