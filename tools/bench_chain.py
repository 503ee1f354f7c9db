"""What an optimiser chain costs per step: OptimiserChain(ClipNorm(1), Adam(0.01)) against the same handle's unchained step + reduce
pair (fused_update = 0), alternated on one device, median of the rounds.

  python tools/bench_chain.py [--rounds 5] [--out FILE] [--one-max N]

Shapes: the headline (RbQ10 [2,16,16,1], batch 65 536), the same model at the tutorial's batch of 64, the layer-wise tutorial net
[1024,512,256,128,64] at batch 64, the sequence tutorial (I = H = 15, W = 10) at 128 windows.  --one-max sets EH_CHAIN_ONE (the largest
n_theta one workgroup takes norm and update of in one launch; 0: always the norm kernel + the apply kernel) before the library loads.
Times are host clocks around a burst of steps that ends in a device synchronisation."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--one-max", type=int, default=-1)
a = ap.parse_args()
if a.one_max >= 0:
    os.environ["EH_CHAIN_ONE"] = str(a.one_max)
import numpy as np
import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10

CHAIN = [("clipnorm", 1.0, 2.0, True), ("rule",)]


def mlp(hidden, act, B, nb, specialize):
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=hidden, activation=act, scale_nn_outputs=True)
    cols = make_synth_rbq10(nb * B, 1)
    eng = model.engine(0)
    eng.set_data(0, np.stack([cols["sw_pot"], cols["dsw_pot"]]), [cols["ta"]], [cols["reco"]])
    eng.set_params(model.initialparameters(1))
    eng.set_option("fused_update", 0)
    eng.set_option("specialize", specialize)
    return eng, [(k * B, B) for k in range(nb)]


def seq():
    rng = np.random.default_rng(3)
    rows = 1200
    X = (0.6 * rng.standard_normal((2, rows))).astype(np.float32)
    ta = (10 + 8 * rng.standard_normal(rows)).astype(np.float32)
    y = ((3.0 + np.tanh(X[0])) * 2.0 ** (0.1 * (ta - 15.0))).astype(np.float32)
    model = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(15, 15))), activation="tanh", scale_nn_outputs=True)
    eng = model.engine(0)
    eng.set_data(0, X, [ta], [y])
    eng.set_sequences(0, 10, 1, 1, np.arange(0, rows - 11, dtype=np.int32))
    eng.set_params(model.initialparameters(1))
    return eng, [(k * 128, 128) for k in range(8)]


SHAPES = [
    ("headline RbQ10 [2,16,16,1] B=65536", lambda: mlp([16, 16], "tanh", 65536, 8, 1), 10000),
    ("the same model B=64", lambda: mlp([16, 16], "tanh", 64, 8, 1), 10000),
    ("layer-wise [1024,512,256,128,64] B=64", lambda: mlp([1024, 512, 256, 128, 64], "sigmoid", 64, 8, 0), 2000),
    ("sequence tutorial I=H=15 W=10, 128 windows", seq, 2000),
]


def burst(eng, batches, n):
    for s in range(n):
        eng.train_step(*batches[s % len(batches)], want_loss=False)
    eng.synchronize()


lines = [f"optimiser chain ClipNorm(1) + Adam(0.01) against the unchained step + reduce pair, us per step, median of {a.rounds} alternating rounds"
         + (f" (EH_CHAIN_ONE={a.one_max})" if a.one_max >= 0 else ""),
         f"{'shape':48s} {'n_theta':>8s} {'unchained':>10s} {'chained':>10s} {'difference':>10s}   rounds (unchained | chained)"]
for name, make, steps in SHAPES:
    eng, batches = make()
    t = {"plain": [], "chain": []}
    for form in ("plain", "chain"):       # warm-up of both forms (code objects, the run-time compiler)
        eng.opt_init("Adam", 0.01) if form == "plain" else eng.opt_init_chain(CHAIN, "Adam", 0.01)
        burst(eng, batches, 200)
    for r in range(a.rounds):
        for form in ("plain", "chain"):
            eng.opt_init("Adam", 0.01) if form == "plain" else eng.opt_init_chain(CHAIN, "Adam", 0.01)
            burst(eng, batches, 50)
            t0 = time.perf_counter()
            burst(eng, batches, steps)
            t[form].append((time.perf_counter() - t0) / steps * 1e6)
    p, c = statistics.median(t["plain"]), statistics.median(t["chain"])
    lines.append(f"{name:48s} {eng.n_theta:8d} {p:10.2f} {c:10.2f} {c - p:10.2f}   " + " ".join(f"{x:.2f}" for x in t["plain"]) + " | " + " ".join(f"{x:.2f}" for x in t["chain"]))
    print(lines[-1], flush=True)
    eng.close()
text = "\n".join(lines) + "\n"
print(text)
if a.out:
    with open(a.out, "a") as f:
        f.write(text)
