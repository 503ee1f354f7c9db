"""Step time of recorded activations next to the built-in per-layer kernel: RbQ10 [2,16,16,1], step + reduce pair.
  python tools/bench_activations.py [--batch 65536] [--steps 300] [--runs 5]
The recorded twins of tanh and sigmoid compute the arithmetic of the built-in ["tanh", "sigmoid"] per-layer kernel, so that kernel is the
yardstick: the two are run alternately, `runs` times each; softplus / elu / gelu_tanh next to them, and everything again at batch 64."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--nbatches", type=int, default=8)
a = ap.parse_args()

CONFIGS = {
    "builtin tanh,sigmoid": ("tanh", "sigmoid"),
    "recorded twins": (lambda z: np.tanh(z), lambda z: 1 / (1 + np.exp(-z))),
    "softplus,softplus": (eh.softplus, eh.softplus),
    "elu,elu": (eh.elu, eh.elu),
    "gelu_tanh,gelu_tanh": (eh.gelu_tanh, eh.gelu_tanh),
}


def engine(acts, B, cols):
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=eh.Chain(eh.Dense(16, 16, acts[1])), activation=acts[0], scale_nn_outputs=True)
    eng = model.engine(0)
    eng.set_data(0, np.stack([cols["sw_pot"], cols["dsw_pot"]]) / np.float32(50), [cols["ta"]], [cols["reco"]])
    eng.set_params(model.initialparameters(1)); eng.opt_init("Adam", 0.01)
    eng.set_option("fused_update", 0)                 # the step + reduce pair
    return eng


def timed(eng, B, steps, nb):
    def run(n, base=0):
        for s in range(n):
            eng.train_step(((base + s) % nb) * B, B, want_loss=False)
    run(20); eng.synchronize()
    t0 = time.perf_counter(); run(steps, 20); eng.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


for B in (a.batch, 64):
    cols = make_synth_rbq10(a.nbatches * B, 1)
    engs = {k: engine(v, B, cols) for k, v in CONFIGS.items()}
    res = {k: [] for k in CONFIGS}
    for r in range(a.runs):                           # alternating: one run of every configuration per round
        for k, e in engs.items():
            res[k].append(timed(e, B, a.steps, a.nbatches))
    for k, e in engs.items():
        njit, _ = e.jit_status()
        print(json.dumps({"batch": B, "config": k, "us_per_step": [round(x, 3) for x in res[k]], "median_us": round(float(np.median(res[k])), 3),
                          "spread_us": round(max(res[k]) - min(res[k]), 3), "jit_kernels": njit}))
        e.close()
    pair = res["builtin tanh,sigmoid"], res["recorded twins"]
    spread = max(max(p) - min(p) for p in pair)
    print(json.dumps({"batch": B, "twins_minus_builtin_median_us": round(float(np.median(pair[1]) - np.median(pair[0])), 3), "pair_spread_us": round(spread, 3),
                      "within_3x_spread": bool(abs(np.median(pair[1]) - np.median(pair[0])) <= 3 * spread)}))
