"""-m gpu: the per-wave step kernel's workgroup reduction (csrc/eh_device.hpp, "7. workgroup reduction", the v2 branch) against the
form it replaced.  The reduction sums the 16 sample columns of every per-sample partial inside the wave before parking it (one word
per row) and gathers one word per live wave for every element; the parent parked the columns and summed them in the gather.  Same
additions in the same association, so the same bits: two engines run the SAME kernel source compiled at run time, one of them with
EH_AB_REDUCE_PARENT (the parent's parking and gather, kept verbatim for this), take the same four Adam steps, and everything the
steps leave behind -- losses, parameters, both moments, the beta powers -- has to be equal bit for bit.

Shapes: the per-wave shapes whose raw accumulators fit one wave workspace (AL.rw <= WAVE_WS) are the one- and two-block ones at their
default tiles; [*,16,16,*] is the headline's, [2,32,32,1] the wider one (NBH = 2: the K1 | PS vectors of two row blocks).  The
four-block shapes (hidden 64) park the v3 way and are not this code."""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho
from tests import util

pytestmark = pytest.mark.gpu
WG = 256                       # samples per workgroup of the narrow per-wave shapes (4 x 64 or 8 x 32)
NSTEPS = 4


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one compilation per (descriptor, defines) for the whole module: the cache key covers the defines"""
    return str(tmp_path_factory.mktemp("eh_jit_cache"))


@pytest.fixture(scope="module")
def cases():
    n = NSTEPS * 17 * WG
    return {
        "rbq10": util.rbq10_case(n, "tanh", True, 0.0),
        "rbq10_nan": util.rbq10_case(n, "tanh", True, 0.3),
        "rbq10_32": util.rbq10_case(n, "tanh", True, 0.0, hidden=(32, 32)),
        "expo2pool": _expo2pool(n),
    }


def _expo2pool(n):
    spec = ho.expo2pool_spec((16, 16), "tanh", True)
    X, f, y = ho.make_synth_expo2pool(n, 5, 0.1)
    return spec, ho.init_theta(spec, 3, np.float32), X, f, y


def _engine(case, fused, parent, monkeypatch, jit_cache):
    monkeypatch.setenv("EH_NO_AOT_SPEC", "1")
    monkeypatch.setenv("EH_JIT_CACHE", jit_cache)
    if parent:
        monkeypatch.setenv("EH_JIT_DEFINES", "EH_AB_REDUCE_PARENT")
    else:
        monkeypatch.delenv("EH_JIT_DEFINES", raising=False)
    eng = util.load_engine(*case)
    eng.opt_init("Adam", 0.01)
    eng.set_option("specialize", 1)
    eng.set_option("fused_update", fused)
    return eng


def _state(eng, losses):
    njit, jlog = eng.jit_status()
    assert njit >= 1 and not jlog.startswith("ahead-of-time"), "the run-time compiled kernel did not run: " + jlog[:300]
    m, v, bt = eng.get_opt_state()
    out = dict(losses=np.asarray(losses, np.float32), params=eng.get_params().copy(), m=m, v=v, bt=bt)
    eng.close()
    return out


def _steps(case, fused, window, parent, monkeypatch, jit_cache):
    eng = _engine(case, fused, parent, monkeypatch, jit_cache)
    losses = [eng.train_step(i * window, window) for i in range(NSTEPS)]
    return _state(eng, losses)


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (k, a[k].ravel()[:4], b[k].ravel()[:4])
    assert np.all(np.isfinite(a["params"])) and np.any(a["m"] != 0)


# 1 sample: one lane of one wave; 64: two of eight waves live; 200; three workgroups, the last with a partly filled tile and dead
# waves; 17 workgroups: the ordered step folds groups of two rows.  Float atomics (fused_update 1) are reproducible on one workgroup only.
WINDOWS = [1, 64, 200, 3 * WG - 37, 17 * WG]


@pytest.mark.parametrize("fused,window", [(f, w) for f in (0, 2) for w in WINDOWS] + [(1, w) for w in WINDOWS if w <= WG])
def test_headline_shape_steps_are_the_parents_bits(cases, fused, window, monkeypatch, jit_cache):
    a = _steps(cases["rbq10"], fused, window, False, monkeypatch, jit_cache)
    b = _steps(cases["rbq10"], fused, window, True, monkeypatch, jit_cache)
    _same(a, b)


@pytest.mark.parametrize("fused", [0, 2])
def test_masked_lanes_are_the_parents_bits(cases, fused, monkeypatch, jit_cache):
    a = _steps(cases["rbq10_nan"], fused, 3 * WG - 37, False, monkeypatch, jit_cache)
    b = _steps(cases["rbq10_nan"], fused, 3 * WG - 37, True, monkeypatch, jit_cache)
    _same(a, b)


@pytest.mark.parametrize("window", [64, 2 * WG - 5])
def test_shape_with_neither_fast_path_is_the_parents_bits(cases, window, monkeypatch, jit_cache):
    """Expo2Pool [8,16,16,4]: eight predictors, four network outputs -- the layer-0 and output accumulators are MFMA-contracted (parked
    raw), the output bias is a row-summed accumulator of its own (kbo)"""
    a = _steps(cases["expo2pool"], 0, window, False, monkeypatch, jit_cache)
    b = _steps(cases["expo2pool"], 0, window, True, monkeypatch, jit_cache)
    _same(a, b)


@pytest.mark.parametrize("fused,window", [(0, 2 * WG - 5), (2, 17 * WG)])
def test_two_block_shape_is_the_parents_bits(cases, fused, window, monkeypatch, jit_cache):
    """RbQ10 [2,32,32,1]: the widest per-wave shape that still parks the v2 way (K1 | PS layout: 18 accumulators, 4 624 floats per wave, in a
    wave workspace of 6 528 at the default 64-sample tiles)"""
    a = _steps(cases["rbq10_32"], fused, window, False, monkeypatch, jit_cache)
    b = _steps(cases["rbq10_32"], fused, window, True, monkeypatch, jit_cache)
    _same(a, b)


def test_multi_step_launch_is_the_parents_bits(cases, monkeypatch, jit_cache):
    """batch 64, two epochs in multi-step launches: the gather writes the sums straight into the launch's LDS state (ms_direct)"""
    spec, theta, X, f, y = cases["rbq10"]
    n = 40 * 64
    case = (spec, theta, X[:, :n], {k: v[:n] for k, v in f.items()}, {k: v[:n] for k, v in y.items()})
    out = []
    for parent in (False, True):
        eng = _engine(case, 1, parent, monkeypatch, jit_cache)
        eng.set_option("multi_step", 1)
        # the multi-step launch takes a run-time compiled kernel only once a single step has checked it against the generic one (multi_ok,
        # csrc/eh_api.hip): take that step first, so that every step of the epochs below runs in multi-step launches on both engines
        losses = [eng.train_step(0, 64)]
        assert eng.jit_status()[0] >= 1, eng.jit_status()[1][:300]
        losses += [eng.train_epoch(64, seed=k, shuffle=True)[0] for k in range(2)]
        out.append(_state(eng, losses))
    _same(*out)
