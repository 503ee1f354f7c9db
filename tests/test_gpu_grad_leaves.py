"""-m gpu: the smallest inputs on which a leaf of the gradient -- one weight matrix, one bias vector, one global parameter -- is orders of
magnitude below the largest entry, on the kernels bench.py and a default train() run: loss and gradient against the fp64 oracle, every
leaf on its own size with no floor under it (util.check_gradient, floor = 0).  tests/test_grad_leaves.py shows on the CPU that the
oracle run in fp32 holds a quarter of each bar on every leaf of these inputs, and that relerr() would not see the weak leaves at all."""
import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho
from tests import grad_leaf_cases as glc
from tests import test_gpu_lform as lform
from tests import util

pytestmark = pytest.mark.gpu
TOL = 1e-5
PRECISION = {0: ("f32", 1e-5, 1e-5), 1: ("bf16_fwd", 2e-5, 5e-5), 2: ("bf16", 2e-5, 2e-5)}      # oracle precision, loss bar, gradient bar (tests/test_gpu_bf16.py)


def _check(eng, spec, theta, X, f, y, ltol=TOL, gtol=TOL):
    loss, grad, nv = eng.loss_and_grad()
    l0, g0, nv0 = ho.loss_and_grad(spec, theta.astype(np.float64), X, f, y)
    assert nv == sum(nv0)
    assert abs(loss - l0) <= ltol * abs(l0), (loss, l0)
    assert util.relerr(grad, g0) <= gtol, util.relerr(grad, g0)
    util.check_gradient(grad, g0, spec, gtol, util.ref32_orders(spec, theta, X, f, y), floor=0.0)


def _generic(eng):
    n, log = eng.jit_status()
    assert n == 0, log[:300]


def _jit_used(eng):
    n, log = eng.jit_status()
    assert n >= 1 and not log.startswith("ahead-of-time") and "disagrees" not in log, log[:300]


# ---- two-network RbQ10: the Q10 network's leaves are 1e-4 .. 1e-3 of the largest entry ----------------------------------------------------
@pytest.mark.parametrize("specialize", [0, 1])
@pytest.mark.parametrize("B", glc.TWO_NET_BATCHES)
def test_two_networks_on_the_per_wave_kernels(B, specialize):
    spec, theta, X, f, y = glc.two_net_case(glc.TWO_NET_NARROW, B)
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_option("row_split", 0)                            # (24 wide side by side: the per-wave family)
    eng.set_option("specialize", specialize)
    _check(eng, spec, theta, X, f, y)
    (_jit_used if specialize else _generic)(eng)
    eng.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("B", glc.TWO_NET_BATCHES)
def test_two_networks_on_the_row_split_kernel(B, precision):
    spec, theta, X, f, y = glc.two_net_case(glc.TWO_NET_WIDE, B, glc.TWO_NET_WIDE_DRAW)
    prec, ltol, gtol = PRECISION[precision]
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_option("row_split", 1)
    eng.set_option("precision", precision)                    # (refused outside the row-split family)
    _check(eng, glc.two_net_spec_in(spec, prec), theta, X, f, y, ltol, gtol)
    _generic(eng)
    eng.close()


@pytest.mark.parametrize("B", glc.TWO_NET_BATCHES)
def test_two_networks_on_the_layer_wise_form(B):
    """the first of tests/test_gpu_lform.py's MULTI shapes (160 and 96 wide: no fused kernel holds them) with the same forcing"""
    spec, theta, X, f, y = glc.two_net_case(lform.MULTI[0][0], B)
    eng = util.load_engine(spec, theta, X, f, y)
    with pytest.raises(NotImplementedError, match="layer-wise form"):
        eng.set_option("precision", 1)
    _check(eng, spec, theta, X, f, y)
    _generic(eng)
    eng.close()


# ---- the K = 1 fast path: the weak leaf is the global Q10 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_paths", [3, 0])
@pytest.mark.parametrize("B", glc.FAST_PATH_BATCHES)
def test_the_global_parameter_behind_the_fast_path(B, fast_paths):
    """fast_paths 3 (the default: K == 1 and P <= 4 on the vector ALU) and 0 (the MFMA forms)"""
    spec, theta, X, f, y = util.rbq10_case(B, "tanh", False)
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_option("fast_paths", fast_paths)
    _check(eng, spec, theta, X, f, y)
    _generic(eng)
    eng.close()


# ---- the headline descriptor on raw inputs: the weak leaf is the first-layer bias behind a saturated tanh ------------------------------------
@pytest.mark.parametrize("kernel", ["aot", "generic", "specialize"])
@pytest.mark.parametrize("B", glc.HEADLINE_BATCHES)
def test_the_headline_descriptor_on_raw_inputs(B, kernel):
    spec, theta, X, f, y = glc.headline_case(B)
    assert float(np.median(X[0])) > 30                         # raw sw_pot: nothing was divided
    eng = glc.headline_model().engine(0)
    eng.set_data(eh.EH_SPLIT_TRAIN, X, [f["ta"]], [y["reco"]])
    eng.set_params(theta)
    eng.set_option("aot_spec", int(kernel == "aot"))
    eng.set_option("specialize", int(kernel == "specialize"))
    _check(eng, spec, theta, X, f, y)
    n, log = eng.jit_status()
    if kernel == "aot":
        assert n >= 1 and log.startswith("ahead-of-time: descriptor 0 "), log[:300]
    else:
        (_jit_used if kernel == "specialize" else _generic)(eng)
    eng.close()
