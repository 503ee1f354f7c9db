"""Throughput of the layer-wise form on the reference's GPU tutorial network (docs/literate/tutorials/synthetic_respiration_gpu.jl:79-92:
RbQ10, hidden_layers = [1024, 512, 256, 128, 64], sigmoid, scale_nn_outputs, input_batchnorm, RMSProp):  python tools/bench_lform.py [batch ...]
  python tools/bench_lform.py --norm [rounds]: the cost of one LayerNorm layer next to one BatchNorm layer (measure_norm below)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HIDDEN = [1024, 512, 256, 128, 64]
DIMS = [2] + HIDDEN + [1]
FLOP = 6 * sum(a * b for a, b in zip(DIMS[:-1], DIMS[1:]))      # per sample: forward, delta and weight-gradient products


def measure(B, device=0):
    """-> dict (one JSON line of this tool): steady-state time of eh_train_step at minibatch B.  Needs a GPU."""
    import easyhybrid_jl_amd as eh
    from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=HIDDEN, activation="sigmoid", scale_nn_outputs=True, input_batchnorm=True)
    nb = max(2, min(8, (1 << 19) // B))
    cols = make_synth_rbq10(nb * B, seed=1)
    X = np.stack([cols["sw_pot"], cols["dsw_pot"]]).astype(np.float32)
    eng = model.engine(device)
    try:
        eng.set_data(0, X, [cols["ta"]], [cols["reco"]])
        eng.set_params(model.initialparameters(1)); eng.opt_init("RMSProp", 0.001)
        steps = max(10, min(300, (1 << 22) // B))
        for s in range(5): eng.train_step((s % nb) * B, B, want_loss=False)
        eng.synchronize()
        t0 = time.perf_counter()
        for s in range(steps): eng.train_step((s % nb) * B, B, want_loss=False)
        eng.synchronize()
        us = 1e6 * (time.perf_counter() - t0) / steps
        return {"net": DIMS, "batch": B, "us_per_step": round(us, 1), "samples_per_s": round(B / us * 1e6), "algorithmic_TFLOPs": round(FLOP * B / us / 1e6, 2),
                "frac_f32_peak": round(FLOP * B / us / 1e6 / 157.3, 3), "steps": steps, "final_loss": eng.train_step(0, B)}
    finally:
        eng.close()


def measure_norm(width, B, rounds=5, steps=200, warmup=20, device=0):
    """-> dict: cost per step of ONE normalisation layer of `width` units -- LayerNorm (csrc/eh_lnl.hpp) next to BatchNorm (csrc/eh_bnl.hpp) at
    the same place, the middle of Dense(2 -> w) -> Dense(w -> w) -> norm -> Dense(w -> w) -> Dense(w -> 1), sigmoid, RbQ10, Adam -- against
    the same chain without it.  The three engines ALTERNATE in one process, `rounds` times, `steps` timed steps each between two
    synchronisations (a quarter of them at B >= 16 384); median of the rounds, minimum and maximum.  Needs the environment of
    `--norm` (below): every engine on the plain layer-wise path, the one a normalisation layer runs on."""
    import easyhybrid_jl_amd as eh
    from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10
    nb = 2
    cols = make_synth_rbq10(nb * B, seed=1, nan_frac=0.05)
    X = (np.stack([cols["sw_pot"], cols["dsw_pot"]]) / np.float32(50)).astype(np.float32)
    steps = max(10, steps // 4) if B >= 16384 else steps
    norms = {"layernorm": lambda: [eh.LayerNorm(width)], "batchnorm": lambda: [eh.BatchNorm(width)], "plain": lambda: []}
    engs = {}
    try:
        for name, norm in norms.items():
            hl = eh.Chain(eh.Dense(width, width, "sigmoid"), *norm(), eh.Dense(width, width, "sigmoid"))
            model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"], hidden_layers=hl,
                                            activation="sigmoid", scale_nn_outputs=True)
            eng = engs[name] = model.engine(device)
            eng.set_data(0, X, [cols["ta"]], [cols["reco"]])
            eng.set_params(model.initialparameters(1)); eng.opt_init("Adam", 0.001)
            for s in range(warmup): eng.train_step((s % nb) * B, B, want_loss=False)
            eng.synchronize()
        times = {name: [] for name in engs}
        for r in range(rounds):
            for name, eng in engs.items():
                t0 = time.perf_counter()
                for s in range(steps): eng.train_step(((r * steps + s) % nb) * B, B, want_loss=False)
                eng.synchronize()
                times[name].append(1e6 * (time.perf_counter() - t0) / steps)
        out = {"norm_layer_width": width, "batch": B, "rounds": rounds, "steps": steps}
        for name, t in times.items():
            t = sorted(t)
            out[name] = {"us_per_step_median": round(t[len(t) // 2], 2), "min": round(t[0], 2), "max": round(t[-1], 2)}
        for name in ("layernorm", "batchnorm"):
            out[f"per_{name}_layer_us"] = round(out[name]["us_per_step_median"] - out["plain"]["us_per_step_median"], 2)
        # the spread of the pair: the wider of the two variants' (max - min) over the rounds
        out["pair_spread_us"] = round(max(out[n]["max"] - out[n]["min"] for n in ("layernorm", "batchnorm")), 2)
        out["final_loss"] = {name: eng.train_step(0, B) for name, eng in engs.items()}
        return out
    finally:
        for eng in engs.values():
            eng.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--norm"]:      # python tools/bench_lform.py --norm [rounds]: one LayerNorm / BatchNorm layer, widths 16 and 1 024, B = 64 and 65 536
        # (before the library is loaded: the baseline on the path the normalised chains run -- the layer-wise form whatever the widths, its few-rows fusions off)
        for k, v in (("EH_FORCE_LFORM", "1"), ("EH_LFORM_NOFUSE", "1"), ("EH_LFORM_NOFIRST", "1"), ("EH_LFORM_NOTAIL", "1"), ("EH_LFORM_GROUP_MAX", "0")):
            os.environ[k] = v
        for width in (16, 1024):
            for B in (64, 65536):
                print(json.dumps(measure_norm(width, B, rounds=int(sys.argv[2]) if len(sys.argv) > 2 else 5)), flush=True)
        sys.exit(0)
    for B in [int(v) for v in sys.argv[1:]] or [64, 256, 1024, 4096, 16384, 65536]:
        print(json.dumps(measure(B)), flush=True)
