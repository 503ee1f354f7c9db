"""Time of the training step with a BatchNorm layer behind every hidden Dense layer (csrc/eh_bnl.hpp) against the same net without them,
both on the plain layer-wise path: hidden_layers [64, 64] and the GPU tutorial's [1024, 512, 256, 128, 64] (BatchNorm behind its first
three layers: a BatchNorm layer counts towards the descriptor's eight hidden layers), sigmoid, RbQ10, Adam, at B = 64 and 65 536.
  python tools/bench_bn_chain.py [--steps 200] [--warmup 20] [--rounds 5] [--nets 64x64,1024x512x256x128x64] [--batches 64,65536]
The two engines of a (net, B) are ALTERNATED in one process, `rounds` times, `steps` timed steps each between two synchronisations
(a quarter of them at B >= 16 384).  The baseline is forced onto the path the BatchNorm handle runs: EH_FORCE_LFORM (the layer-wise form
whatever the widths) and the few-rows fusions off (EH_LFORM_NOFUSE, EH_LFORM_NOFIRST, EH_LFORM_NOTAIL, EH_LFORM_GROUP_MAX = 0), set
here before the library is loaded -- so this script measures nothing else.
One JSON line per (net, B): per variant the median us / step of the rounds with their minimum and maximum, the cost per BatchNorm layer
and the bytes its passes move -- forward: the column sums read X, the normalisation reads X and writes xh and Y (4 passes over [B][n]);
backward: the sums read dY, xh, Y, the delta pass reads dY, xh, Y and the layer below and writes dX (8 passes) -- as GB / s."""
import argparse, json, os, sys, time
for k, v in (("EH_FORCE_LFORM", "1"), ("EH_LFORM_NOFUSE", "1"), ("EH_LFORM_NOFIRST", "1"), ("EH_LFORM_NOTAIL", "1"), ("EH_LFORM_GROUP_MAX", "0")):
    os.environ[k] = v
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--nets", default="64x64,1024x512x256x128x64")
ap.add_argument("--batches", default="64,65536")
a = ap.parse_args()
PASSES = 12


def bn_count(widths):
    """BatchNorm layers behind the leading hidden Dense layers, as many as the descriptor's eight hidden layers leave room for"""
    return min(len(widths), eh._lib.EH_MAX_HIDDEN - len(widths))


def model_of(widths, bn):
    layers = []
    for i, w in enumerate(widths):
        if i:
            layers.append(eh.Dense(widths[i - 1], w, "sigmoid"))
        if i < bn_count(widths):
            layers.append(eh.BatchNorm(w))
    hl = eh.Chain(*layers) if bn else list(widths)
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"], hidden_layers=hl,
                                   activation="sigmoid", scale_nn_outputs=True)


nb = 2                                            # minibatches the steps rotate through
batches = [int(b) for b in a.batches.split(",")]
cols = make_synth_rbq10(nb * max(batches), 1, 0.05)
X = np.stack([cols["sw_pot"], cols["dsw_pot"]]) / np.float32(50)
for net in a.nets.split(","):
    widths = [int(w) for w in net.split("x")]
    for B in batches:
        steps = max(10, a.steps // 4) if B >= 16384 else a.steps
        engs = {}
        for name, bn in (("batchnorm", True), ("plain", False)):
            model = model_of(widths, bn)
            eng = model.engine(0)
            eng.set_data(0, X, [cols["ta"]], [cols["reco"]])
            eng.set_params(model.initialparameters(1))
            eng.opt_init("Adam", 0.001)
            for s in range(a.warmup):
                eng.train_step((s % nb) * B, B, want_loss=False)
            eng.synchronize()
            engs[name] = eng
        times = {name: [] for name in engs}
        for r in range(a.rounds):
            for name, eng in engs.items():
                t0 = time.perf_counter()
                for s in range(steps):
                    eng.train_step(((r * steps + s) % nb) * B, B, want_loss=False)
                eng.synchronize()
                times[name].append(1e6 * (time.perf_counter() - t0) / steps)
        out = {"hidden_layers": widths, "B": B, "rounds": a.rounds, "steps": steps}
        for name in engs:
            t = sorted(times[name])
            out[name] = {"us_per_step_median": t[len(t) // 2], "min": t[0], "max": t[-1]}
        extra = out["batchnorm"]["us_per_step_median"] - out["plain"]["us_per_step_median"]
        nbytes = PASSES * 4 * B * sum(widths[:bn_count(widths)])
        out["batchnorm_layers"] = bn_count(widths)
        out["per_batchnorm_layer_us"] = extra / bn_count(widths)
        out["batchnorm_bytes"] = nbytes
        out["batchnorm_GB_per_s"] = nbytes / (extra * 1e-6) / 1e9 if extra > 0 else None
        out["final_loss"] = {name: eng.train_step(0, B) for name, eng in engs.items()}
        print(json.dumps(out), flush=True)
        for eng in engs.values():
            eng.close()
