"""The ordered one-kernel training step ("fused_update" 2 on minibatches of several workgroups; EH_MODE_TRAIN_ORD, csrc/eh_device.hpp
EhOrd) against the deterministic step + reduce pair it replaces ("fused_update" 0, same library): the same bits in parameters, Adam
moments, beta products and losses -- not merely close."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu


def _engine(mode, case, aot=0, specialize=0, rule="Adam", wd=0.0):
    spec, theta, X, f, y = case
    e = util.load_engine(spec, theta, X, f, y)
    e.set_option("aot_spec", aot)
    if specialize:
        e.set_option("specialize", 1)
    e.opt_init(rule, 0.01, weight_decay=wd)
    e.set_option("fused_update", mode)
    return e


def _state(e):
    th = e.get_params().copy()
    m, v, bt = e.get_opt_state()
    return [th, m.copy(), v.copy(), bt.copy()]


def _same(a, b):
    assert len(a) == len(b)
    for u, w in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(w), equal_nan=True)


def _run_both(case, script, **kw):
    """script(engine) -> list of losses; run under the pair and under the ordered step, compare everything"""
    out = []
    for mode in (0, 2):
        e = _engine(mode, case, **kw)
        losses = script(e)
        out.append((losses, _state(e)))
        e.close()
    (l0, s0), (l2, s2) = out
    assert np.all(np.isfinite(s0[0]))
    _same(l0, l2)
    _same(s0, s2)


def _steps(windows, last_loss=True):
    def script(e):
        for first, count in windows:
            e.train_step(first, count, want_loss=False)
        return [e.train_step(*windows[0])] if last_loss else []
    return script


def test_headline_batch_on_the_kernel_built_ahead_of_time():
    case = util.rbq10_case(4 * 65536, "tanh", True, 0.05)
    _run_both(case, _steps([((i % 4) * 65536, 65536) for i in range(7)]), aot=1)


@pytest.mark.parametrize("counts", [(512, 4300, 25000), (25000, 300, 4300, 600), (65536, 2000, 65536)])
def test_grids_that_are_not_multiples_of_16_and_change_between_steps(counts):
    case = util.rbq10_case(70000, "tanh", True, 0.1)
    windows = [((i * 977) % (70000 - c), c) for i, c in enumerate(counts * 3)]
    _run_both(case, _steps(windows))


@pytest.mark.parametrize("rule,wd", [("Adam", 0.0), ("AdamW", 0.01), ("RMSProp", 0.0), ("Descent", 0.0)])
def test_every_optimiser_rule(rule, wd):
    case = util.rbq10_case(20000, "sigmoid", False, 0.1)
    _run_both(case, _steps([(i * 3000, 5000) for i in range(5)]), rule=rule, wd=wd)


def test_all_masked_minibatch_is_skipped_as_by_the_pair():
    spec, theta, X, f, y = util.rbq10_case(4 * 4096, "tanh", True, 0.1)
    y = {k: v.copy() for k, v in y.items()}
    for v in y.values():
        v[4096:8192] = np.nan                                   # the second minibatch: no valid target at all
    case = (spec, theta, X, f, y)

    def script(e):
        l, n = e.train_epoch(4096, shuffle=False)
        return [l, n]
    _run_both(case, script)


@pytest.mark.parametrize("aot,specialize", [(0, 0), (0, 1)])
def test_generic_and_run_time_compiled_kernels(aot, specialize):
    case = util.rbq10_case(30000, "tanh", True, 0.05, hidden=(32, 16))
    _run_both(case, _steps([(i * 2000, 9000) for i in range(8)]), aot=aot, specialize=specialize)


@pytest.mark.parametrize("n,batch", [(9000, 2048), (8192 + 100, 2048)])
def test_epochs_with_shuffle_and_a_partial_last_minibatch(n, batch):
    """the last minibatch is smaller (808 samples: fewer workgroups; 100: one workgroup, the float-atomic one-kernel step, whose
    sums meet in one fixed order there) -- the pending ordered update is applied by whatever comes next"""
    case = util.rbq10_case(n, "tanh", True, 0.05)

    def script(e):
        out = []
        for ep in range(3):
            out += list(e.train_epoch(batch, seed=7 + ep, shuffle=True))
        return out
    _run_both(case, script)


def test_graph_replay():
    case = util.rbq10_case(16384, "tanh", True, 0.05)
    w = [((i % 8) * 2048, 2048) for i in range(6)]

    def script(e):
        e.train_step(0, 2048, want_loss=False)                  # (the fused modes record with an update pending)
        e.graph_begin()
        for first, count in w:
            e.train_step(first, count, want_loss=False)
        g = e.graph_end()
        for _ in range(3):
            e.graph_launch(g)
        e.synchronize()
        return [e.train_step(0, 2048)]

    def plain(e):                                               # (a capture records its steps without running them)
        e.train_step(0, 2048, want_loss=False)
        for _ in range(3):
            for first, count in w:
                e.train_step(first, count, want_loss=False)
        return [e.train_step(0, 2048)]
    e = _engine(2, case)
    l2 = script(e); s2 = _state(e); e.close()
    e = _engine(0, case)
    l0 = plain(e); s0 = _state(e); e.close()
    _same(l0, l2)
    _same(s0, s2)


def test_switching_modes_mid_run():
    """2 -> 0 -> 2 with an ordered update pending at each switch: the switch applies it (flush), the pair takes over, and back"""
    case = util.rbq10_case(20000, "tanh", True, 0.05)
    w = [(i * 1500, 6000) for i in range(4)]

    def script(e, switch):
        losses = []
        for mode in (2, 0, 2):
            if switch:
                e.set_option("fused_update", mode)
            for first, count in w:
                e.train_step(first, count, want_loss=False)
            losses.append(e.train_step(500, 3000))
            e.train_step(3000, 5000, want_loss=False)          # (pending across the switch)
        return losses
    e = _engine(2, case)
    l2 = script(e, True); s2 = _state(e); e.close()
    e = _engine(0, case)
    l0 = script(e, False); s0 = _state(e); e.close()
    _same(l0, l2)
    _same(s0, s2)
