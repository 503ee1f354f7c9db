"""What dropout costs per step: the same handle with and without Dropout behind its hidden layers, alternated on one device, median
of the rounds.  Both forms run kernels compiled at run time around the model ("specialize" 1 without dropout), the step + reduce pair
(fused_update = 0), one launch per step.

  python tools/bench_dropout.py [--rounds 5] [--out FILE]

Shapes: case A (RbQ10 [2,16,16,1] tanh, rates 0.5 / 0.5) and case C ([8,40,24,64,1] relu, rates 0.1 / 0 / 0.5) of tests/test_gpu_dropout.py,
each at batch 512 and 65 536.  Times are host clocks around a burst of steps that ends in a device synchronisation."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
import numpy as np
import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS


def make(n_pred, hidden, act, scale, B, nb):
    rng = np.random.default_rng(1)
    names = [f"x{i}" for i in range(n_pred)]
    model = eh.constructHybridModel(names, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=hidden, activation=act, scale_nn_outputs=scale)
    n = nb * B
    X = (0.5 * rng.standard_normal((n_pred, n))).astype(np.float32)
    ta = (10 + 10 * rng.standard_normal(n)).astype(np.float32)
    y = ((3.0 + np.tanh(X[0])) * 2.0 ** (0.1 * (ta - 15.0))).astype(np.float32)
    eng = model.engine(0)
    eng.set_data(0, X, [ta], [y])
    eng.set_params(model.initialparameters(1))
    eng.set_option("fused_update", 0)
    eng.set_option("specialize", 1)
    return eng, [(k * B, B) for k in range(nb)]


SHAPES = [
    ("A RbQ10 [2,16,16,1] tanh p=(.5,.5) B=512", lambda: make(2, [16, 16], "tanh", True, 512, 8), (0.5, 0.5), 5000),
    ("A RbQ10 [2,16,16,1] tanh p=(.5,.5) B=65536", lambda: make(2, [16, 16], "tanh", True, 65536, 4), (0.5, 0.5), 3000),
    ("C RbQ10 [8,40,24,64,1] relu p=(.1,0,.5) B=512", lambda: make(8, [40, 24, 64], "relu", False, 512, 8), (0.1, 0.0, 0.5), 5000),
    ("C RbQ10 [8,40,24,64,1] relu p=(.1,0,.5) B=65536", lambda: make(8, [40, 24, 64], "relu", False, 65536, 4), (0.1, 0.0, 0.5), 1000),
]


def burst(eng, batches, n):
    for s in range(n):
        eng.train_step(*batches[s % len(batches)], want_loss=False)
    eng.synchronize()


lines = [f"dropout against the same model without it, us per step (step + reduce pair, kernels compiled at run time), median of {a.rounds} alternating rounds",
         f"{'shape':50s} {'plain':>9s} {'dropout':>9s} {'difference':>10s}   rounds (plain | dropout)"]
for name, mk, rates, steps in SHAPES:
    eng, batches = mk()
    eng.opt_init("Adam", 0.01)
    t = {"plain": [], "drop": []}
    zero = [0.0] * len(rates)
    for form in ("plain", "drop"):        # warm-up of both forms (the run-time compiler, code objects)
        eng.set_dropout(zero if form == "plain" else rates, seed=1)
        burst(eng, batches, 200)
    for r in range(a.rounds):
        for form in ("plain", "drop"):
            eng.set_dropout(zero if form == "plain" else rates, seed=1)
            burst(eng, batches, 50)
            t0 = time.perf_counter()
            burst(eng, batches, steps)
            t[form].append((time.perf_counter() - t0) / steps * 1e6)
    p, d = statistics.median(t["plain"]), statistics.median(t["drop"])
    lines.append(f"{name:50s} {p:9.2f} {d:9.2f} {d - p:10.2f}   " + " ".join(f"{x:.2f}" for x in t["plain"]) + " | " + " ".join(f"{x:.2f}" for x in t["drop"]))
    print(lines[-1], flush=True)
    eng.close()
text = "\n".join(lines) + "\n"
print(text)
if a.out:
    with open(a.out, "a") as f:
        f.write(text)
