"""Diagnostic: where the ordered one-kernel step (fused_update = 2, EH_MODE_TRAIN_ORD) spends its hand-off -- the tail of every group's last
arriver (the stamps of workgroup 0 do not see it) and the ordered part of the prologue -- on the headline step (RbQ10 [2,16,16,1], B = 65 536).
The kernel is compiled at run time with the stamps in:
    EH_NO_AOT_SPEC=1 EH_JIT_CACHE=0 EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE" python tools/stamps_ord.py
    EH_NO_AOT_SPEC=1 EH_JIT_CACHE=0 EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_PARENT" python tools/stamps_ord.py   (the drain and
        the shuffle butterfly put back; implies EH_AB_ORD_ROW_SCALARS)
    EH_NO_AOT_SPEC=1 EH_JIT_CACHE=0 EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_ROW_SCALARS" python tools/stamps_ord.py   (the
        prologue reads the 256 rows' scalar vectors and folds all six butterfly levels, as before the tail formed the block partials)
    EH_NO_AOT_SPEC=1 EH_JIT_CACHE=0 EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_FOLD_WAVE0" python tools/stamps_ord.py   (wave 0
        folds the block partials, not the last wave)
The scalar fold's slot is stamped by the wave that folds (its image staged -> its fold done).
Every number is the median over the last `--reps` steps, each read back on its own (a synchronize per step: the steps run apart)."""
import argparse
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import util

ST_TAIL, ST_PRO, WORDS, GROUPS = 32, 32 + 10 * 16, 256, 16
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
B = args.batch
defs = os.environ.get("EH_JIT_DEFINES", "")
if "EH_STAMPS" not in defs:
    sys.exit("set EH_JIT_DEFINES (see the docstring): a normal build records no stamps")
spec, theta, X, f, y = util.rbq10_case(8 * B, "tanh", True, 0.0)
eng = util.load_engine(spec, theta, X, f, y)
eng.opt_init("Adam", 0.01)
eng.set_option("specialize", 1)
eng.set_option("fused_update", 2)
buf = (C.c_uint64 * WORDS)()
eng._lib.eh_debug_stamps(eng._h, buf, WORDS)          # arms the buffer
rows = []
for i in range(args.warmup + args.reps):
    eng.train_step((i % 8) * B, B, want_loss=False)
    eng._lib.eh_debug_stamps(eng._h, buf, WORDS)       # (synchronises)
    if i < args.warmup:
        continue
    st = np.array(list(buf), dtype=np.int64)
    tail = st[ST_TAIL:ST_TAIL + 10 * GROUPS].reshape(GROUPS, 5, 2)
    ngrp = int((tail[:, 0, 1] > 0).sum())
    wall = tail[:, :, 1]
    last = int(np.argmax(wall[:, 4]))                   # the group whose row is stored last: the end of the step
    t0 = st[0 * 2 + 1]                                  # workgroup 0's start (wall clock)
    pro = st[ST_PRO:ST_PRO + 4].reshape(2, 2)
    rows.append(dict(
        ngrp=ngrp,
        # the last-finishing group's tail, in its shader-clock cycles: row staged -> barrier passed and the row's stores issued (wave 0) ->
        # ticket known -> rows folded -> group row stored
        tail_cyc=np.diff(tail[last, :, 0]),
        tail_ns=np.diff(wall[last]) * 10,
        tail_ns_mean=(np.diff(wall[:ngrp], axis=1) * 10).mean(axis=0),
        end_ns=(wall[last, 4] - t0) * 10,               # workgroup 0's start to the last group row stored
        wg0_ns=(st[10 * 2 + 1] - t0) * 10,              # workgroup 0's own start to end
        fold_cyc=pro[1, 0] - pro[0, 0], fold_ns=(pro[1, 1] - pro[0, 1]) * 10,
        pro_cyc=np.array([st[2 * k] for k in (0, 2, 3, 4, 5, 6, 7, 1)], dtype=np.int64),
    ))
eng.close()
med = lambda k: np.median(np.array([r[k] for r in rows]), axis=0)
print(f"EH_JIT_DEFINES='{defs}'  B = {B}  groups stamped: {int(med('ngrp'))}  (median of {len(rows)} steps)")
lab = ["barrier, row stores issued", "ticket", "rows loaded + folded", "group row stored"]
tc, tn, tm = med("tail_cyc"), med("tail_ns"), med("tail_ns_mean")
print("  tail of the group that finishes last (cycles / ns; ns mean over the groups):")
for k, nm in enumerate(lab):
    print(f"    {nm:26s} {tc[k]:8.0f} cycles {tn[k]:8.0f} ns   {tm[k]:8.0f} ns")
print(f"    {'sum':26s} {tc.sum():8.0f} cycles {tn.sum():8.0f} ns")
print(f"  workgroup 0 start -> last group row stored  {med('end_ns'):8.0f} ns   (workgroup 0 start -> its end {med('wg0_ns'):.0f} ns)")
print(f"  prologue, ordered scalar fold (its wave)    {med('fold_cyc'):8.0f} cycles {med('fold_ns'):8.0f} ns")
pc = np.diff(np.array([r["pro_cyc"] for r in rows]), axis=1)
plab = ["state loads issued", "exchange words requested", "image staged + ordered fold", "(p2p wait)", "statistics + X images cleared",
        "update applied", "scalars, barrier"]
print("  prologue of workgroup 0 (EH_STAMPS_PROLOGUE slots, cycles):")
for k, nm in enumerate(plab):
    print(f"    {nm:32s} {np.median(pc[:, k]):8.0f}")
