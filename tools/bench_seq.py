"""Time of the sequence-model training step (csrc/eh_seq.hpp): the LSTM tutorial's shape -- P = 2, I = H = 15, input_window 10,
output_window 1, RbQ10, RMSProp -- at 128 windows per step (the tutorial's batch), 1 024 and 16 384.
  python tools/bench_seq.py [--steps 300] [--warmup 20] [--windows 128,1024,16384] [--cpu-twin]
--steps / --warmup as in tools/bench_config.py: `warmup` untimed steps, then `steps` timed ones between two synchronisations.
The kernels' own time comes from the engine's events (eh_profile_enable) here and, for the record, from ONE run of this script under
`rocprofv3 --kernel-trace --stats -- python tools/bench_seq.py --windows 128 --steps 200` (profiles/r10/seq_step.txt).
--cpu-twin: the fp32 step of the torch restatement (tests/seq_twin.py, loss + autograd gradient) on 16 CPU threads, as context.
One JSON line per window count.
  python tools/bench_seq.py --closure [--steps 300] [--warmup 20] [--rounds 5] [--windows 128,16384] [--output-windows 1,10]
--closure: the mechanistic model three ways -- RbQ10 of the registry, the same formula as a recorded closure on the interpreter
("jit" = 0) and on the kernels compiled at run time ("jit" = 1) -- ALTERNATED in one process: `rounds` times round the three engines,
`steps` timed steps each.  One JSON line per (windows, output_window): per variant the median us / step of the rounds and their
minimum and maximum (the spread the comparison has to be read against).  profiles/r11/seq_closure_step.txt.
--cell lstm|gru|rnn: the recurrent cell of every mode above (RNNCell with tanh); default lstm.
  python tools/bench_seq.py --cells lstm,gru,rnn [--steps 300] [--warmup 20] [--rounds 5] [--windows 128,16384] [--output-windows 1,10]
--cells: the listed cells around the registry's RbQ10, ALTERNATED in one process as --closure alternates its three; same output.
  python tools/bench_seq.py --targets 3 [--steps 300] [--warmup 20] [--rounds 5] [--windows 128,16384] [--output-windows 1,10]
--targets N: 1 .. N targets (mse each) around the registry's FluxPartModelQ10 -- "fluxpart_T1" is the one-target kernel, the others the
kernels of several targets behind their count pre-pass -- and N targets around the three-output closure of the tests (flux3) compiled at
run time, ALTERNATED in one process as above; per line also the cost of a further target per launch and per head step, against the same
build's fluxpart_T1.  profiles/r22/seq_multitarget_step.txt."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--windows", default="128,1024,16384")
ap.add_argument("--input-window", type=int, default=10)
ap.add_argument("--output-window", type=int, default=1)
ap.add_argument("--width", type=int, default=15, help="I = H")
ap.add_argument("--cpu-twin", action="store_true")
ap.add_argument("--closure", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--output-windows", default="1,10")
ap.add_argument("--cell", default="lstm", choices=["lstm", "gru", "rnn"])
ap.add_argument("--cells", default=None, help="comma-separated cells to alternate")
ap.add_argument("--targets", type=int, default=0, help="1 .. N targets around FluxPartModelQ10, N around the compiled closure flux3")
a = ap.parse_args()


def rbq10_closure(*, ta, rb, Q10):
    """RbQ10 as a user writes it (the reference's LSTM tutorial returns the parameters next to the prediction)"""
    return dict(reco=rb * Q10 ** (0.1 * (ta - 15.0)), Q10=Q10, rb=rb)


CELL = {"lstm": lambda: eh.LSTMCell(a.width, a.width), "gru": lambda: eh.GRUCell(a.width, a.width), "rnn": lambda: eh.RNNCell(a.width, a.width, "tanh")}


def closure_bench():
    W, lam = a.input_window, 1
    counts = [int(c) for c in (a.windows if a.windows != "128,1024,16384" else "128,16384").split(",")]
    nb = 4
    rows = nb * max(counts) + W + lam
    cols = make_synth_rbq10(rows, 1, 0.05)
    X = np.stack([cols["sw_pot"], cols["dsw_pot"]]) / np.float32(50)
    starts = np.arange(rows - W - lam + 1, dtype=np.int32)
    mk = lambda mech, cell: eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], mech, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                                    hidden_layers=eh.Chain(eh.Recurrence(CELL[cell]())), activation="tanh", scale_nn_outputs=True)
    if a.cells:
        variants = [(c, eh.RbQ10, None, c) for c in a.cells.split(",")]
    else:
        variants = [("registry", eh.RbQ10, None, a.cell), ("closure_interpreted", rbq10_closure, 0, a.cell), ("closure_compiled", rbq10_closure, 1, a.cell)]
    for B in counts:
        for ow in [int(o) for o in a.output_windows.split(",")]:
            engs = []
            for name, mech, jit, cell in variants:
                model = mk(mech, cell)
                eng = model.engine(0)
                if jit is not None:
                    eng.set_option("jit", jit)
                eng.set_data(0, X, [cols["ta"]], [cols["reco"]])
                eng.set_sequences(0, W, ow, lam, starts)
                eng.set_params(model.initialparameters(1))
                eng.opt_init("RMSProp", 0.01)
                for s in range(a.warmup):
                    eng.train_step((s % nb) * B, B, want_loss=False)
                eng.synchronize()
                if eng.jit_status()[0] != (jit or 0):
                    raise SystemExit(f"{name}: eh_jit_status reports {eng.jit_status()[0]} compiled kernels: {eng.jit_status()[1][:400]}")
                engs.append(eng)
            times = {v[0]: [] for v in variants}
            for r in range(a.rounds):
                for (name, *_), eng in zip(variants, engs):
                    t0 = time.perf_counter()
                    for s in range(a.steps):
                        eng.train_step(((r * a.steps + s) % nb) * B, B, want_loss=False)
                    eng.synchronize()
                    times[name].append(1e6 * (time.perf_counter() - t0) / a.steps)
            out = {"windows": B, "input_window": W, "output_window": ow, "I": a.width, "H": a.width, "rounds": a.rounds, "steps": a.steps}
            for name, *_ in variants:
                t = sorted(times[name])
                out[name] = {"us_per_step_median": t[len(t) // 2], "min": t[0], "max": t[-1]}
            out["final_loss"] = {name: eng.train_step(0, B) for (name, *_), eng in zip(variants, engs)}
            print(json.dumps(out), flush=True)
            for eng in engs:
                eng.close()


def targets_bench():
    from tests import seq_closure_twin as ct
    W, lam, N = a.input_window, 1, a.targets
    if not 1 <= N <= 3:
        raise SystemExit("--targets: 1..3 (FluxPartModelQ10 and flux3 have three outputs)")
    counts = [int(c) for c in (a.windows if a.windows != "128,1024,16384" else "128,16384").split(",")]
    nb = 4
    rows = nb * max(counts) + W + lam
    rng = np.random.default_rng(1)
    X = (0.6 * rng.standard_normal((2, rows))).astype(np.float32)
    frc = {"SW_IN": rng.uniform(0.0, 800.0, rows).astype(np.float32), "TA": (10 + 8 * rng.standard_normal(rows)).astype(np.float32), "vpd": rng.uniform(0.0, 30.0, rows).astype(np.float32)}
    frc.update(sw=frc["SW_IN"], ta=frc["TA"])
    ys = []
    for _ in range(3):                                # noise with 5 % gaps of its own per target: the step's time does not depend on the values
        v = (3.0 + rng.standard_normal(rows)).astype(np.float32)
        v[rng.random(rows) < 0.05] = np.nan
        ys.append(v)
    starts = np.arange(rows - W - lam + 1, dtype=np.int32)
    chain = lambda: eh.Chain(eh.Recurrence(CELL[a.cell]()))
    flux3 = eh.models.resolve_mech(ct.flux3_np, list(ct.FLUX3_TABLE), list(ct.FLUX3_FORCINGS), list(ct.FLUX3_OUTPUTS))
    variants = [(f"fluxpart_T{T}", eh.constructHybridModel(["x0", "x1"], ["SW_IN", "TA"], ["NEE", "GPP", "RECO"][:T], eh.FluxPartModelQ10, dict(ct.FLUXPART_TABLE), ["RUE", "Rb"],
                                                           ["Q10"], hidden_layers=chain(), activation="tanh", scale_nn_outputs=True), None, T) for T in range(1, N + 1)]
    variants.append((f"flux3_compiled_T{N}", eh.constructHybridModel(["x0", "x1"], list(ct.FLUX3_FORCINGS), list(ct.FLUX3_OUTPUTS)[:N], flux3, dict(ct.FLUX3_TABLE), ["rue", "rb"],
                                                                     ["q10"], hidden_layers=chain(), activation="tanh", scale_nn_outputs=True), 1, N))
    for B in counts:
        for ow in [int(o) for o in a.output_windows.split(",")]:
            engs = []
            for name, model, jit, T in variants:
                eng = model.engine(0)
                if jit is not None:
                    eng.set_option("jit", jit)
                eng.set_data(0, X, [frc[f] for f in model.forcing], ys[:T])
                eng.set_sequences(0, W, ow, lam, starts)
                eng.set_params(model.initialparameters(1))
                eng.opt_init("RMSProp", 0.01)
                for s in range(a.warmup):
                    eng.train_step((s % nb) * B, B, want_loss=False)
                eng.synchronize()
                if eng.jit_status()[0] != (jit or 0):
                    raise SystemExit(f"{name}: eh_jit_status reports {eng.jit_status()[0]} compiled kernels: {eng.jit_status()[1][:400]}")
                engs.append(eng)
            times = {v[0]: [] for v in variants}
            for r in range(a.rounds):
                for (name, *_), eng in zip(variants, engs):
                    t0 = time.perf_counter()
                    for s in range(a.steps):
                        eng.train_step(((r * a.steps + s) % nb) * B, B, want_loss=False)
                    eng.synchronize()
                    times[name].append(1e6 * (time.perf_counter() - t0) / a.steps)
            out = {"windows": B, "input_window": W, "output_window": ow, "I": a.width, "H": a.width, "cell": a.cell, "rounds": a.rounds, "steps": a.steps}
            med = {}
            for name, *_ in variants:
                t = sorted(times[name])
                med[name] = t[len(t) // 2]
                out[name] = {"us_per_step_median": med[name], "min": t[0], "max": t[-1]}
            for T in range(2, N + 1):                 # against the same build's one-target step: per launch, and per head step and further target
                d = med[f"fluxpart_T{T}"] - med["fluxpart_T1"]
                out[f"further_targets_T{T}"] = {"us_per_launch": d, "us_per_head_step_and_target": d / (ow * (T - 1))}
            out["final_loss"] = {name: eng.train_step(0, B) for (name, *_), eng in zip(variants, engs)}
            print(json.dumps(out), flush=True)
            for eng in engs:
                eng.close()


if a.targets:
    targets_bench()
    sys.exit(0)
if a.closure or a.cells:
    closure_bench()
    sys.exit(0)
W, ow, lam = a.input_window, a.output_window, 1
model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                hidden_layers=eh.Chain(eh.Recurrence(CELL[a.cell]())), activation="tanh", scale_nn_outputs=True)
counts = [int(c) for c in a.windows.split(",")]
nb = 4                                            # minibatches the steps rotate through
rows = nb * max(counts) + W + lam
cols = make_synth_rbq10(rows, 1, 0.05)
X = np.stack([cols["sw_pot"], cols["dsw_pot"]]) / np.float32(50)
starts = np.arange(rows - W - lam + 1, dtype=np.int32)
theta = model.initialparameters(1)
nbh = (a.width + 15) // 16
for B in counts:
    eng = model.engine(0)
    eng.set_data(0, X, [cols["ta"]], [cols["reco"]])
    eng.set_sequences(0, W, ow, lam, starts)
    eng.set_params(theta)
    eng.opt_init("RMSProp", 0.01)

    def run(n, base=0):
        for s in range(n):
            eng.train_step(((base + s) % nb) * B, B, want_loss=False)
    run(a.warmup); eng.synchronize()
    t0 = time.perf_counter(); run(a.steps, a.warmup); eng.synchronize(); dt = time.perf_counter() - t0
    eng.profile_enable(True)
    run(min(a.steps, 200)); eng.synchronize()
    _, k_step, k_reduce = eng.profile_read()
    eng.profile_enable(False)
    tiles = (B + 15) // 16
    grid = max(1, min((tiles + 3) // 4, 256))
    out = {"windows": B, "input_window": W, "output_window": ow, "I": a.width, "H": a.width, "cell": a.cell, "n_theta": model.n_theta, "us_per_step": 1e6 * dt / a.steps,
           "windows_per_s": B * a.steps / dt, "step_kernel_us": 1e3 * k_step, "reduce_kernel_us": 1e3 * k_reduce, "workgroups": grid,
           "tiles_per_wave": -(-tiles // (4 * grid)), "workspace_bytes": grid * 4 * (W * {"lstm": 6, "gru": 5, "rnn": 2}[a.cell] * nbh + ow * (nbh + 1)) * 1024, "final_loss": eng.train_step(0, B)}
    if a.cpu_twin:
        import torch
        from tests import seq_twin as tw
        torch.set_num_threads(16)
        f = {"ta": cols["ta"]}
        for _ in range(2):
            tw.loss_and_grad(model, theta, X, f, cols["reco"], starts[:B], W, ow, lam, "mse", torch.float32)
        n = 5
        t0 = time.perf_counter()
        for _ in range(n):
            tw.loss_and_grad(model, theta, X, f, cols["reco"], starts[:B], W, ow, lam, "mse", torch.float32)
        out["cpu_twin_fp32_16_threads_us"] = 1e6 * (time.perf_counter() - t0) / n
    print(json.dumps(out))
    eng.close()
