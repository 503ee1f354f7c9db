"""Diagnostic: what the step's run-time switches cost the headline step (RbQ10 [2,16,16,1], B = 65 536) -- the prologue taken apart, the
tile, the rest, in shader-clock cycles of workgroup 0, for the general and the lean form of the single-step train kernels
(eh_lean_fold, csrc/eh_device.hpp) out of ONE source in one session.  The kernels are compiled at run time with the stamps in:
    EH_NO_AOT_SPEC=1 EH_JIT_CACHE=0 EH_LEAN_DIAG=1 EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE" python tools/stamps_lean.py
        (EH_LEAN_DIAG=1: the lean form keeps the diagnostics pointer; the script switches the forms with the "lean" option)
tools/stamps_reduce.py and tools/stamps_ord.py take the reduction and the hand-off apart the same way: run them with EH_LEAN_DIAG=1 for
the lean form and with EH_NO_LEAN=1 for the general one.  Both one-kernel forms are stamped, `fused_update` 1 (float atomics) and 2 (the
ordered step).  Every number is the median over the last `--reps` steps, each read back on its own (a synchronize per step)."""
import argparse
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import util

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
B = args.batch
defs = os.environ.get("EH_JIT_DEFINES", "")
if "EH_STAMPS_PROLOGUE" not in defs or not os.environ.get("EH_LEAN_DIAG"):
    sys.exit("set EH_JIT_DEFINES and EH_LEAN_DIAG (see the docstring): a normal build records no stamps")
spec, theta, X, f, y = util.rbq10_case(8 * B, "tanh", True, 0.0)
LAB = ["kernel start -> state loads asked for (0->2)", "-> image asked for (2->3)", "-> image staged, sums folded (3->4)", "-> (4->5)",
       "-> X cleared, barrier (5->6)", "-> update applied (6->7)", "-> end of the prologue (7->1)", "prologue in all (0->1)",
       "tile (1->8)", "reduction + hand-off (8->10)", "kernel, workgroup 0 (0->10)", "kernel, workgroup 0, wall clock ns"]
print(f"EH_JIT_DEFINES='{defs}'  B = {B}  (median of {args.reps} steps, cycles of workgroup 0)")
table = {}
for fused in (1, 2):
    for lean in (0, 1):
        eng = util.load_engine(spec, theta, X, f, y)
        eng.opt_init("Adam", 0.01)
        eng.set_option("specialize", 1)
        eng.set_option("fused_update", fused)
        eng.set_option("lean", lean)
        buf = (C.c_uint64 * 32)()
        eng._lib.eh_debug_stamps(eng._h, buf, 32)          # arms the buffer
        rows = []
        for i in range(args.warmup + args.reps):
            eng.train_step((i % 8) * B, B, want_loss=False)
            eng._lib.eh_debug_stamps(eng._h, buf, 32)       # (synchronises)
            if i < args.warmup:
                continue
            st = np.array(list(buf), dtype=np.int64)
            c = lambda k: st[2 * k]
            rows.append([c(2) - c(0), c(3) - c(2), c(4) - c(3), c(5) - c(4), c(6) - c(5), c(7) - c(6), c(1) - c(7), c(1) - c(0),
                         c(8) - c(1), c(10) - c(8), c(10) - c(0), (st[2 * 10 + 1] - st[1]) * 10])
        form = eng.jit_status()[1]
        eng.close()
        want = "train step kernel: lean" if lean else "train step kernel: general"
        if want not in form:
            sys.exit(f"fused_update = {fused}, lean = {lean}: the other form ran ({form[-120:]})")
        table[(fused, lean)] = np.median(np.array(rows), axis=0)
for fused in (1, 2):
    print(f"  fused_update = {fused}{'':34s} {'general':>9s} {'lean':>9s} {'saved':>9s}")
    for k, nm in enumerate(LAB):
        g, l = table[(fused, 0)][k], table[(fused, 1)][k]
        print(f"    {nm:46s} {g:9.0f} {l:9.0f} {g - l:9.0f}")
