"""What per-branch optimiser rules cost: one rule (eh_opt_init) against two groups of rules (eh_opt_init_groups, TrainConfig.opt =
{"ps": Adam(0.01), "Q10": Descent(0.05)}) on ONE lease, alternating, three rounds:
  - the headline step, RbQ10 [2,16,16,1] at batch 65 536: the seeded default ("fused_update" 2) and fused_update = True (float atomics)
  - the batch-64 epoch of one-workgroup multi-step launches (65 536 samples, 1 024 steps)
  - the layer-wise tutorial net [2,1024,512,256,128,64,1] at batch 64 and 1 024
python tools/bench_opt_groups.py [steps]   -> one JSON line, us per step"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
B, NB = 65536, 16
cols = make_synth_rbq10(NB * B, seed=42)
X = np.stack([cols["sw_pot"], cols["dsw_pot"]]).astype(np.float32)


def model_of(hidden, act):
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"],
                                   hidden_layers=list(hidden), activation=act, scale_nn_outputs=True)


def engine(model, n, grouped, fused):
    eng = model.engine(0)
    eng.set_data(eh.EH_SPLIT_TRAIN, X[:, :n], [cols["ta"][:n]], [cols["reco"][:n]])
    eng.set_params(model.initialparameters(161803))
    if grouped:
        group = np.zeros(model.n_theta, np.uint8)
        group[model.opt_branches()["Q10"][0]] = 1
        eng.opt_init_groups(group, [dict(rule="Adam", lr=0.01), dict(rule="Descent", lr=0.05)])
    else:
        eng.opt_init("Adam", 0.01)
    eng.set_option("fused_update", fused)
    return eng


def time_steps(eng, batch, n, k):
    nb = n // batch
    for s in range(min(200, k)):
        eng.train_step((s % nb) * batch, batch, want_loss=False)
    eng.synchronize()
    t0 = time.perf_counter()
    for s in range(k):
        eng.train_step((s % nb) * batch, batch, want_loss=False)
    eng.synchronize()
    eng.close()
    return 1e6 * (time.perf_counter() - t0) / k


def time_epoch(eng, batch, reps):
    eng.train_epoch(batch, shuffle=False, want_loss=False)
    eng.synchronize()
    t0 = time.perf_counter()
    ns = 0
    for _ in range(reps):
        _, n = eng.train_epoch(batch, shuffle=False, want_loss=False)
        ns += n
    eng.synchronize()
    eng.close()
    return 1e6 * (time.perf_counter() - t0) / ns


head, tut = model_of((16, 16), "tanh"), model_of((1024, 512, 256, 128, 64), "sigmoid")
cases = {
    "headline_seeded": lambda g: time_steps(engine(head, NB * B, g, 2), B, NB * B, steps),
    "headline_fused": lambda g: time_steps(engine(head, NB * B, g, 1), B, NB * B, steps),
    "epoch_b64": lambda g: time_epoch(engine(head, B, g, 1), 64, 3),
    "tutorial_b64": lambda g: time_steps(engine(tut, 8192, g, 0), 64, 8192, max(100, steps // 10)),
    "tutorial_b1024": lambda g: time_steps(engine(tut, 8192, g, 0), 1024, 8192, max(100, steps // 10)),
}
out = {}
for rep in range(3):
    for name, run in cases.items():
        for label, g in (("one_rule", False), ("two_groups", True)):
            out.setdefault(name, {}).setdefault(label, []).append(round(run(g), 3))
print(json.dumps({"what": "us per step, one rule vs two groups of rules, three alternating rounds on one lease", **out}))
