"""Diagnostic: the account of the per-wave step kernel's workgroup reduction (csrc/eh_device.hpp, "7. workgroup reduction") on the
headline step (RbQ10 [2,16,16,1], B = 65 536) -- from the end of the tile to the end of the kernel, workgroup 0, in shader-clock cycles.
The kernel is compiled at run time with the stamps in:
    EH_NO_AOT_SPEC=1 EH_JIT_CACHE=0 EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_FINE" python tools/stamps_reduce.py
    EH_NO_AOT_SPEC=1 EH_JIT_CACHE=0 EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_FINE EH_AB_REDUCE_PARENT" python tools/stamps_reduce.py   (the
        parking and the gather of rounds 5-11 put back)
Both one-kernel forms are stamped, `fused_update` 1 (float atomics) and 2 (the ordered step).  Thread 0 (wave 0) stamps the phases;
thread 64 stamps the start and the end of wave 1's gather, so a gather that loads the waves unevenly shows.  Every number is the
median over the last `--reps` steps, each read back on its own (a synchronize per step: the steps run apart)."""
import argparse
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import util

WORDS, RED = 256, 200           # EH_STAMP_WORDS, EH_RED_ST
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
B = args.batch
defs = os.environ.get("EH_JIT_DEFINES", "")
if "EH_STAMPS_FINE" not in defs:
    sys.exit("set EH_JIT_DEFINES (see the docstring): a normal build records no stamps")
spec, theta, X, f, y = util.rbq10_case(8 * B, "tanh", True, 0.0)
print(f"EH_JIT_DEFINES='{defs}'  B = {B}  (median of {args.reps} steps, cycles of workgroup 0)")
for fused in (1, 2):
    eng = util.load_engine(spec, theta, X, f, y)
    eng.opt_init("Adam", 0.01)
    eng.set_option("specialize", 1)
    eng.set_option("fused_update", fused)
    buf = (C.c_uint64 * WORDS)()
    eng._lib.eh_debug_stamps(eng._h, buf, WORDS)          # arms the buffer
    rows = []
    for i in range(args.warmup + args.reps):
        eng.train_step((i % 8) * B, B, want_loss=False)
        eng._lib.eh_debug_stamps(eng._h, buf, WORDS)       # (synchronises)
        if i < args.warmup:
            continue
        st = np.array(list(buf), dtype=np.int64)
        cyc = lambda k: st[2 * k]
        g0, w1a, w1b = st[RED], st[RED + 2], st[RED + 4]
        rows.append([cyc(8) - cyc(0), cyc(13) - cyc(8), cyc(14) - cyc(13), cyc(12) - cyc(14), cyc(9) - cyc(12), g0 - cyc(9), cyc(15) - g0,
                     cyc(10) - cyc(15), cyc(10) - cyc(8), cyc(10) - cyc(0), w1b - w1a, g0 - w1b, (st[2 * 10 + 1] - st[1]) * 10])
    njit = eng.jit_status()[0]
    eng.close()
    med = np.median(np.array(rows), axis=0)
    lab = ["start -> end of the tile (0->8)", "wave sums (8->13)", "barrier 1 (13->14)", "parking (14->12)", "barrier 2 (12->9)",
           "gather, wave 0 (9->loop end)", "publish / p2p (loop end->15)", "end (15->10)", "reduction in all (8->10)", "kernel, workgroup 0 (0->10)",
           "gather, wave 1 (its start->its end)", "wave 1's gather end -> wave 0's", "kernel, workgroup 0, wall clock ns"]
    print(f"  fused_update = {fused}   (kernels compiled at run time: {njit})")
    for nm, v in zip(lab, med):
        print(f"    {nm:38s} {v:8.0f}")
