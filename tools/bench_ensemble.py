#!/usr/bin/env python3
"""Ensemble epochs and evaluations against the same work on an ordinary engine, one member after another.

    python tools/bench_ensemble.py [--members 1,8,64,256,512,1024] [--rows 4096] [--batch 64] [--reps 7] [--out profiles/ensemble_epoch.json]

Headline model RbQ10 [2, 16, 16, 1] tanh on the kernels specialised ahead of time (--aot 0: on the generic table), 4096 rows per member (every member its own random 4096 of a
16384-row table), minibatches of 64, shuffled epochs.  For every M: the time of one ensemble epoch (all M members, eh_ens_train_epoch) and
of one eh_ens_eval over the members' rows; next to them, measured in the same process on an ordinary engine of the same library that holds
4096 rows, one member's multi-step epoch (eh_train_epoch) and one eh_eval -- what training the members one after another costs M times.
Every figure is a host clock around calls that end in a device synchronisation; the two sides alternate, `reps` repetitions each after a
warm-up, and the table gives the median and the spread (max - min) of each.  The acceptance line compares the M = 64 epoch with 64 single
epochs: faster by more than three times the larger spread, or the launch is broken.  No GPU, no numbers: the tool fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import easyhybrid_jl_amd as eh                                            # noqa: E402
from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS, make_synth_rbq10     # noqa: E402


def timed(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e6


def stats(x):
    x = np.asarray(x)
    return {"median_us": float(np.median(x)), "spread_us": float(x.max() - x.min()), "min_us": float(x.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="1,8,64,256,512,1024")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--aot", type=int, default=1, help="1: the kernels specialised ahead of time for the headline descriptor; 0: the generic table")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Ms = [int(m) for m in a.members.split(",")]
    model = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"], hidden_layers=[16, 16],
                                    activation="tanh", scale_nn_outputs=True)
    N = 4 * a.rows
    cols = make_synth_rbq10(N, seed=1)
    X = np.stack([cols["sw_pot"] / np.float32(50), cols["dsw_pot"] / np.float32(50)]).astype(np.float32)
    rng = np.random.default_rng(0)
    theta = model.initialparameters(rng)

    def engine(rows=None):
        e = model.engine()
        sl = slice(None) if rows is None else rows
        e.set_data(0, X[:, sl], [cols["ta"][sl]], [cols["reco"][sl]])
        e.set_params(theta); e.opt_init("Adam", lr=0.01); e.set_option("fused_update", 1); e.set_option("aot_spec", a.aot)
        return e
    single = engine(np.sort(rng.permutation(N)[:a.rows]))
    table = []
    for M in Ms:
        eng = engine()
        ens = eng.ensemble(M, a.batch)
        for j in range(M):
            ens.set_params(j, theta); ens.set_opt(j, "Adam", lr=0.01 * (1 + j / (4 * M))); r = np.random.default_rng(j).permutation(N)[:a.rows]
            ens.set_rows(j, 0, r); ens.set_rows(j, 1, r)
        seeds = list(range(M))
        runs = {"ens_epoch": [], "ens_eval": [], "one_epoch": [], "one_eval": []}
        for rep in range(a.warmup + a.reps):
            t = {"ens_epoch": timed(lambda: ens.train_epoch(seeds, shuffle=True, want_loss=False), eng.synchronize),
                 "one_epoch": timed(lambda: single.train_epoch(a.batch, seed=rep, shuffle=True, want_loss=False), single.synchronize),
                 "ens_eval": timed(lambda: ens.eval(1), lambda: None),
                 "one_eval": timed(lambda: single.eval(0), lambda: None)}
            if rep >= a.warmup:
                for k, v in t.items():
                    runs[k].append(v)
        row = {"members": M, "rows_per_member": a.rows, "batch": a.batch, "steps_per_member": -(-a.rows // a.batch)}
        row.update({k: stats(v) for k, v in runs.items()})
        row["sequential_epochs_us"] = M * row["one_epoch"]["median_us"]
        row["epoch_ratio"] = row["sequential_epochs_us"] / row["ens_epoch"]["median_us"]
        row["eval_ratio"] = M * row["one_eval"]["median_us"] / row["ens_eval"]["median_us"]
        row["kernels"] = eng.jit_status()[1].split("\n")[0][:80] if a.aot else "generic table (aot_spec 0)"
        table.append(row)
        print(json.dumps(row), flush=True)
        ens.close(); eng.close()
    single.close()
    print(f"{'M':>5} {'ens epoch us':>14} {'spread':>8} {'1 epoch us':>11} {'spread':>8} {'M x 1 / ens':>12} {'ens eval us':>12} {'1 eval us':>10} {'M x 1 / ens':>12}")
    for r in table:
        print(f"{r['members']:>5} {r['ens_epoch']['median_us']:>14.1f} {r['ens_epoch']['spread_us']:>8.1f} {r['one_epoch']['median_us']:>11.1f} {r['one_epoch']['spread_us']:>8.1f} "
              f"{r['epoch_ratio']:>12.1f} {r['ens_eval']['median_us']:>12.1f} {r['one_eval']['median_us']:>10.1f} {r['eval_ratio']:>12.1f}")
    ok = None
    for r in table:
        if r["members"] == 64:
            margin = r["sequential_epochs_us"] - r["ens_epoch"]["median_us"]
            bar = 3 * max(r["ens_epoch"]["spread_us"], 64 * r["one_epoch"]["spread_us"])
            ok = margin > bar
            print(f"acceptance at M = 64: 64 single epochs {r['sequential_epochs_us']:.1f} us - ensemble epoch {r['ens_epoch']['median_us']:.1f} us = {margin:.1f} us, "
                  f"three times the larger spread {bar:.1f} us: {'PASS' if ok else 'FAIL'}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"table": table, "acceptance_m64": ok}, fh, indent=1)
    return 0 if ok in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
