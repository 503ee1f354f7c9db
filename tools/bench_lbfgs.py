"""What an objective evaluation of the device-resident L-BFGS solve costs, against what a user had before it: the same
algorithm on the host (tests/lbfgs_twin.py, fp32 vectors) around eh_set_params + eh_loss_and_grad, one synchronisation and one copy of
the gradient per evaluation.  Alternated on one device, median of the rounds.

  python tools/bench_lbfgs.py [--rounds 5] [--out FILE] [--threshold] [--profile headline|case1]

Default: the headline model (RbQ10 [2,16,16,1], batch 65 536) and the test case (the same model, 512 samples).  "host floor" is the host
path without any optimiser arithmetic: set_params + loss_and_grad alone.
--threshold: the one-launch form (dots + decision + update in one workgroup) against the three-kernel form over n_theta, batch 512
(engine option lbfgs_one_max 2^30 / 0): the table EH_LB_ONE_MAX comes from.
--profile: only device solves of that shape (three bursts), for a kernel trace.
A burst is WARM evaluations that fill the history, then N timed ones ending in eh_lbfgs_status (one synchronisation); a burst in which
the solve ended is not counted."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--threshold", action="store_true")
ap.add_argument("--profile", default="", choices=["", "headline", "case1"])
a = ap.parse_args()
import numpy as np
import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10
from tests import lbfgs_twin as tw

WARM, N = 14, 60


def mlp(hidden, B, specialize=1):
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=hidden, activation="tanh", scale_nn_outputs=True)
    cols = make_synth_rbq10(B, 1, 0.1)
    eng = model.engine(0)
    eng.set_data(0, np.stack([cols["sw_pot"], cols["dsw_pot"]]) / np.float32(50), [cols["ta"]], [cols["reco"]])
    eng.set_option("fused_update", 0)
    if list(hidden) == [16, 16]:                  # (the shape bench.py measures: on its kernel compiled at run time, as there)
        eng.set_option("specialize", specialize)
    return eng, model.initialparameters(1)


def seq(B=128):
    rng = np.random.default_rng(3)
    rows = B + 11
    X = (0.6 * rng.standard_normal((2, rows))).astype(np.float32)
    ta = (10 + 8 * rng.standard_normal(rows)).astype(np.float32)
    y = ((3.0 + np.tanh(X[0])) * 2.0 ** (0.1 * (ta - 15.0))).astype(np.float32)
    model = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                    hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(15, 15))), activation="tanh", scale_nn_outputs=True)
    eng = model.engine(0)
    eng.set_data(0, X, [ta], [y])
    eng.set_sequences(0, 10, 1, 1, np.arange(0, rows - 11, dtype=np.int32))
    return eng, model.initialparameters(1)


def device_burst(eng, theta0):
    """us per evaluation of the device-resident solve, or None if the solve ended inside the burst"""
    eng.set_params(theta0)
    eng.lbfgs_init(g_tol=0.0)
    eng.lbfgs_set_batch(maxiters=1 << 20)
    eng.lbfgs_run(WARM)
    eng.lbfgs_status()
    t0 = time.perf_counter()
    eng.lbfgs_run(N)
    st = eng.lbfgs_status()
    dt = time.perf_counter() - t0
    return dt / N * 1e6 if (st["code"] == 0 and st["evaluations"] == WARM + N) else None


def host_burst(eng, theta0):
    """us per evaluation of the twin on the host around set_params + loss_and_grad"""
    n = [0]

    def fg(x):
        n[0] += 1
        eng.set_params(x)
        l, g, nv = eng.loss_and_grad()
        return l, g, nv
    t0 = time.perf_counter()
    r = tw.lbfgs(fg, theta0, N - 4, g_tol=0.0, dtype=np.float32)
    return (time.perf_counter() - t0) / r.evaluations * 1e6


def floor_burst(eng, theta0):
    t0 = time.perf_counter()
    for _ in range(N):
        eng.set_params(theta0)
        eng.loss_and_grad()
    return (time.perf_counter() - t0) / N * 1e6


def med(xs):
    xs = [x for x in xs if x is not None]
    return statistics.median(xs) if xs else float("nan")


def fmt(xs):
    return " ".join("ended" if x is None else f"{x:.2f}" for x in xs)


lines = []
if a.profile:
    eng, th = mlp([16, 16], 65536 if a.profile == "headline" else 512)
    for _ in range(3):
        device_burst(eng, th)
    eng.close()
    sys.exit(0)
if not a.threshold:
    lines += [f"L-BFGS, us per objective evaluation, median of {a.rounds} alternating rounds ({WARM} evaluations to fill the history, then {N} timed)",
              f"{'shape':40s} {'n_theta':>8s} {'device':>8s} {'host twin':>10s} {'host floor':>10s}   rounds (device | host twin | host floor)"]
    for name, make in (("headline RbQ10 [2,16,16,1] B=65536", lambda: mlp([16, 16], 65536)), ("the same model, 512 samples (test case 1)", lambda: mlp([16, 16], 512))):
        eng, th = make()
        t = {"dev": [], "host": [], "floor": []}
        device_burst(eng, th); host_burst(eng, th); floor_burst(eng, th)         # warm-up: code objects, the run-time compiler
        for r in range(a.rounds):
            t["dev"].append(device_burst(eng, th))
            eng.opt_init("Adam", 0.01)                                            # (leaves L-BFGS mode: the handle a user of the parent commit has)
            t["host"].append(host_burst(eng, th))
            t["floor"].append(floor_burst(eng, th))
        lines.append(f"{name:40s} {eng.n_theta:8d} {med(t['dev']):8.2f} {med(t['host']):10.2f} {med(t['floor']):10.2f}   {fmt(t['dev'])} | {fmt(t['host'])} | {fmt(t['floor'])}")
        print(lines[-1], flush=True)
        eng.close()
else:
    lines += [f"L-BFGS, us per objective evaluation at 512 samples (sequence model: 128 windows): one launch for dots + decision + update against three, median of {a.rounds} alternating rounds",
              f"{'shape':32s} {'n_theta':>8s} {'one launch':>10s} {'three':>10s} {'one - three':>11s}   rounds (one | three)"]
    shapes = [("[2,16,16,1]", lambda: mlp([16, 16], 512)), ("[2,32,32,1]", lambda: mlp([32, 32], 512)), ("sequence I=H=15 W=10", seq),
              ("[2,64,64,1]", lambda: mlp([64, 64], 512)), ("[2,96,96,1]", lambda: mlp([96, 96], 512)), ("[2,128,128,1]", lambda: mlp([128, 128], 512)),
              ("[2,256,256,1] layer-wise", lambda: mlp([256, 256], 512))]
    for name, make in shapes:
        eng, th = make()
        t = {1: [], 3: []}
        for form in (1, 3):
            eng.set_option("lbfgs_one_max", (1 << 30) if form == 1 else 0)
            device_burst(eng, th)
        for r in range(a.rounds):
            for form in (1, 3):
                eng.set_option("lbfgs_one_max", (1 << 30) if form == 1 else 0)
                t[form].append(device_burst(eng, th))
        lines.append(f"{name:32s} {eng.n_theta:8d} {med(t[1]):10.2f} {med(t[3]):10.2f} {med(t[1]) - med(t[3]):11.2f}   {fmt(t[1])} | {fmt(t[3])}")
        print(lines[-1], flush=True)
        eng.close()
text = "\n".join(lines) + "\n"
if a.out:
    with open(a.out, "a") as f:
        f.write(text)
