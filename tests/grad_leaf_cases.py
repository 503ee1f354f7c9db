"""The inputs of the leaf-by-leaf gradient tests (tests/test_grad_leaves.py on the CPU, tests/test_gpu_grad_leaves.py on the device): the
smallest cases in which a leaf of the gradient is orders of magnitude below the largest entry -- where relerr(), the largest error over
the largest entry, says nothing about it."""
import numpy as np

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10
from oracle import hybrid_oracle as ho

TWO_NET_NARROW = [([0, 1], [16, 16]), ([2], [8, 8])]             # per-wave kernels (generic, run-time compiled)
TWO_NET_WIDE = [([0, 1, 2], [64, 64]), ([3, 4], [64, 64])]       # 128 wide side by side: the row-split kernel
# the draw of the wide case: in the "bf16" modes a delta that rounds to the other bfloat16 neighbour in fp32 than in fp64 moves its leaf by
# far more than the bar (draw 0 at B = 257: rb.layer_1.weight of the fp32 oracle 17 bars off the fp64 one in "bf16", draws 2 and 6 likewise;
# one draw in three at B = 257, one in eight at 33).  Draw 5 has no such sample in any of the three precisions at either batch size, so the
# reference holds a quarter of every bar on it (tests/test_grad_leaves.py) -- the input was chosen for that, the bars were not.
TWO_NET_WIDE_DRAW = 5
TWO_NET_BATCHES = (33, 257)          # one sample into a second 32-sample tile; one sample past a 256-sample workgroup


def two_net_case(nets, B, seed=0):
    """RbQ10 with rb and Q10 each from a network of its own, run as one block-diagonal MLP.  ta within 15 +- 0.5: reco = rb Q10^((ta - 15) / 10)
    hardly moves with Q10, so every leaf of the Q10 network is 1e-4 .. 1e-3 of the largest entry.  Targets uniform(1, 6), 10 % missing."""
    P = max(max(r) for r, _ in nets) + 1
    spec = ho.HybridSpec(P, [1], "rbq10", dict(ho.RBQ10_PARAMS), ["rb", "Q10"], [], ["reco"], "tanh", True, nets=[(list(r), list(h)) for r, h in nets])
    rng = np.random.default_rng(31000 + 7 * B + seed)
    X = rng.standard_normal((P, B)).astype(np.float32)
    f = {"ta": rng.uniform(14.5, 15.5, B).astype(np.float32)}
    yv = rng.uniform(1, 6, B).astype(np.float32)
    yv[rng.random(B) < 0.1] = np.nan
    yv[0] = np.float32(3.0)          # (never all missing)
    return spec, ho.init_theta(spec, 6, np.float32), X, f, {"reco": yv}


def two_net_spec_in(spec, precision):
    """the same model in another `precision` of the oracle"""
    return ho.HybridSpec(spec.n_pred, list(spec.hidden), spec.mech, dict(spec.parameters), list(spec.neural), list(spec.glob), list(spec.targets),
                         spec.activation, spec.scale_nn_outputs, nets=spec.nets, precision=precision)


HEADLINE_BATCHES = (257, 1000)


def headline_model():
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                   hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)


def headline_case(B):
    """the headline descriptor on the benchmark's raw inputs (sw_pot ~ |50 + 20 N(0,1)|: the first layer's tanh saturated) from
    initialparameters(161803): the first-layer bias is 3e-3 of the largest entry"""
    cols = make_synth_rbq10(B, seed=42)
    X = np.stack([cols["sw_pot"], cols["dsw_pot"]]).astype(np.float32)
    theta = np.asarray(headline_model().initialparameters(161803), np.float32)
    return ho.rbq10_spec((16, 16), "tanh", True), theta, X, {"ta": cols["ta"]}, {"reco": cols["reco"]}


FAST_PATH_BATCHES = (12, 65)
