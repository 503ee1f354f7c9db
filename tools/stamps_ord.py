"""Diagnostic: where the ordered one-kernel step (fused_update = 2, EH_MODE_TRAIN_ORD) spends its hand-off -- the tail of every group's
folder (the stamps of workgroup 0 do not see it) and the ordered part of the prologue -- on the headline step (RbQ10 [2,16,16,1], B = 65 536).
The kernel is compiled at run time with the stamps in:
    EH_NO_AOT_SPEC=1 EH_JIT_CACHE=0 EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE" python tools/stamps_ord.py
    ... EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_TICKET_LATE" ...   (the election behind the row stores, with its own barrier)
    ... EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_TICKET_AT=8" ...   (the early ticket at the end of the tile; 13: behind
        the wave sums; 14, the default: behind the first barrier of the workgroup reduction)
    ... EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_PARENT" ...   (the drain and the shuffle butterfly put back; implies
        EH_AB_ORD_ROW_SCALARS)
    ... EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_ROW_SCALARS" ...   (the prologue reads the 256 rows' scalar vectors and
        folds all six butterfly levels, as before the tail formed the block partials)
    ... EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_FOLD_WAVE0" ...   (wave 0 folds the block partials, not the last wave)
    ... EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_ROWS_EARLY" ...   (the gather stores the row in front of the staged barrier,
        not wave 0 behind it; the folder's pause is then 0 unless EH_AB_ORD_FOLDER_SLEEP says otherwise)
    ... EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_GROW_WT" ...   (group rows and block partials stored write-through)
    ... EH_JIT_DEFINES="EH_STAMPS EH_STAMPS_PROLOGUE EH_AB_ORD_FOLDER_SLEEP=n" ...   (the folder's pause, n x 64 cycles)
The scalar fold's slot is stamped by the wave that folds (its image staged -> its fold done).
The tail's slots are the median over the last `--reps` steps, each read back on its own (a synchronize per step: the steps run apart);
the wait rounds are counted over the same steps: a folder "waited" when any of its lanes met a row under the marker and loaded it again."""
import argparse
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import util

# EH_ORD_ST_PRO, EH_ORD_ST_TAIL, EH_ORD_ST_TAILW, EH_STAMP_WORDS (csrc/eh_device.hpp)
ST_PRO, ST_TAIL, TAILW, GROUPS = 32 + 10 * 16, 256, 32, 16
WORDS = ST_TAIL + TAILW * GROUPS
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
B = args.batch
defs = os.environ.get("EH_JIT_DEFINES", "")
if "EH_STAMPS" not in defs:
    sys.exit("set EH_JIT_DEFINES (see the docstring): a normal build records no stamps")
late = "EH_AB_ORD_TICKET_LATE" in defs
spec, theta, X, f, y = util.rbq10_case(8 * B, "tanh", True, 0.0)
eng = util.load_engine(spec, theta, X, f, y)
eng.opt_init("Adam", 0.01)
eng.set_option("specialize", 1)
eng.set_option("fused_update", 2)
buf = (C.c_uint64 * WORDS)()
eng._lib.eh_debug_stamps(eng._h, buf, WORDS)          # arms the buffer
# the folder's path: [0] row staged, ([6] LATE: row stores issued,) [1] election known, [2] loads issued, [3] first pass folded,
# [4] wait rounds over, [5] group row stored
# the early row stores: [6] the gather begins -- its rounds issue the row's stores -- then [0] as above
early = "EH_AB_ORD_ROWS_EARLY" in defs and not late and not any(d in defs for d in ("EH_AB_ORD_ROW_SCALARS", "EH_AB_ORD_PARENT"))
path = [0, 6, 1, 2, 3, 4, 5] if late else [6, 0, 1, 2, 3, 4, 5] if early else [0, 1, 2, 3, 4, 5]
lab = (["barrier, row stores issued", "ticket"] if late else
       ["gather, row stores issued", "staged barrier, election read"] if early else ["staged barrier, election read"]) + \
      ["loads issued", "first pass folded", "wait rounds", "group row stored"]
rows = []
for i in range(args.warmup + args.reps):
    eng.train_step((i % 8) * B, B, want_loss=False)
    eng._lib.eh_debug_stamps(eng._h, buf, WORDS)       # (synchronises)
    if i < args.warmup:
        continue
    st = np.array(list(buf), dtype=np.int64)
    grp = st[ST_TAIL:ST_TAIL + TAILW * GROUPS].reshape(GROUPS, TAILW)
    tail = grp[:, :16].reshape(GROUPS, 8, 2)[:, path, :]
    ngrp = int((tail[:, 0, 1] > 0).sum())
    wall = tail[:, :, 1]
    last = int(np.argmax(wall[:, -1]))                  # the group whose row is stored last: the end of the step
    t0 = st[0 * 2 + 1]                                  # workgroup 0's start (wall clock)
    pro = st[ST_PRO:ST_PRO + 4].reshape(2, 2)
    ww = grp[:ngrp, 16:25]                              # per wave of the folder: rounds | late rows << 16 (word 24: the scalar vector's wave)
    rounds, mask = ww & 0xFFFF, (ww >> 16) & 0xFFFF
    rows.append(dict(
        ngrp=ngrp,
        tail_cyc=np.diff(tail[last, :, 0]),
        tail_ns=np.diff(wall[last]) * 10,
        tail_ns_mean=(np.diff(wall[:ngrp], axis=1) * 10).mean(axis=0),
        end_ns=(wall[last, -1] - t0) * 10,              # workgroup 0's start to the last group row stored
        wg0_ns=(st[10 * 2 + 1] - t0) * 10,              # workgroup 0's own start to end
        fold_cyc=pro[1, 0] - pro[0, 0], fold_ns=(pro[1, 1] - pro[0, 1]) * 10,
        pro_cyc=np.array([st[2 * k] for k in (0, 2, 3, 4, 5, 6, 7, 1)], dtype=np.int64),
        waited=(rounds.max(axis=1) > 0),                # per folder
        waited_last=bool(rounds[last].max() > 0),
        max_rounds=int(rounds.max()),
        wait_cyc=np.diff(tail[:ngrp, :, 0], axis=1)[:, -2],      # thread 0 of every folder: cycles between "first pass folded" and "wait rounds over"
        late_rows=np.bitwise_or.reduce(mask, axis=1),   # per folder: bit k = row k of the group met under the marker
    ))
eng.close()
med = lambda k: np.median(np.array([r[k] for r in rows]), axis=0)
print(f"EH_JIT_DEFINES='{defs}'  B = {B}  groups stamped: {int(med('ngrp'))}  (median of {len(rows)} steps)")
tc, tn, tm = med("tail_cyc"), med("tail_ns"), med("tail_ns_mean")
print("  tail of the folder that finishes last (cycles / ns; ns mean over the groups):")
for k, nm in enumerate(lab):
    print(f"    {nm:30s} {tc[k]:8.0f} cycles {tn[k]:8.0f} ns   {tm[k]:8.0f} ns")
print(f"    {'sum':30s} {tc.sum():8.0f} cycles {tn.sum():8.0f} ns")
print(f"  workgroup 0 start -> last group row stored  {med('end_ns'):8.0f} ns   (workgroup 0 start -> its end {med('wg0_ns'):.0f} ns)")
waited = np.array([r["waited"] for r in rows])          # [steps][folders]
wc = np.array([r["wait_cyc"] for r in rows])
print("  wait rounds (a folder met a row of its group under the marker and loaded it again):")
print(f"    steps with a folder that waited        {100.0 * waited.any(axis=1).mean():6.1f} %")
print(f"    steps whose last folder waited         {100.0 * np.mean([r['waited_last'] for r in rows]):6.1f} %")
print(f"    folders that waited, per step          {waited.sum(axis=1).mean():6.2f} of {waited.shape[1]}   ({100.0 * waited.mean():.1f} % of all folders)")
print(f"    most rounds of one lane                {max(r['max_rounds'] for r in rows):6d}")
print(f"    cycles in the rounds, thread 0 of a folder that waited: median {np.median(wc[waited]) if waited.any() else 0:.0f}, mean over all folders {wc.mean():.0f}")
hist = np.zeros(16, dtype=np.int64)
for r in rows:
    for m in r["late_rows"]:
        hist += (int(m) >> np.arange(16)) & 1
print("    which row of the group was late (count over folders and steps, rows 0..15): " + " ".join(str(int(h)) for h in hist))
print(f"  prologue, ordered scalar fold (its wave)    {med('fold_cyc'):8.0f} cycles {med('fold_ns'):8.0f} ns")
pc = np.diff(np.array([r["pro_cyc"] for r in rows]), axis=1)
plab = ["state loads issued", "exchange words requested", "image staged + ordered fold", "(p2p wait)", "statistics + X images cleared",
        "update applied", "scalars, barrier"]
print("  prologue of workgroup 0 (EH_STAMPS_PROLOGUE slots, cycles):")
for k, nm in enumerate(plab):
    print(f"    {nm:32s} {np.median(pc[:, k]):8.0f}")
