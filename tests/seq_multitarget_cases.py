"""The parity cases of sequence models with several targets, shared by tests/test_seq_multitarget.py (which checks on the CPU that every
case is well posed) and tests/test_gpu_seq_multitarget.py (which runs them on the device against tests/seq_multitarget_twin.py).

The smallest shapes at which the kernel can still go wrong: one width pair per (NBI, NBH) block class; 13 windows are one partial tile,
37 three tiles (the last partial) in one workgroup, 70 two workgroups whose slab rows are folded; W = 6 with ow 1 or 3, lead time 0 or 1.
Every (class, head form, cell) triple occurs with three targets and ow = 3; the other values ride along by position.

The forcings are the shared series' in dim light and mild weather (`forcings`): NEE = RECO - GPP is a difference, and where the two cancel
an fp32 kernel cannot hold NEE to 1e-5 of its own magnitude whatever it does -- each operand carries a few ulps, ~3e-7 of itself.  With
RECO several times GPP nothing cancels; tests/test_seq_multitarget.py holds every case to (|RECO| + |GPP|) <= CANCEL_MAX * max(|NEE|, floor)
over the windows whose predictions are compared."""
import itertools

import numpy as np

from tests import seq_closure_twin as ct
from tests import seq_multitarget_twin as mt

WIDTHS = [(5, 7), (7, 20), (20, 7), (32, 32)]                 # (I, H): block classes (1, 1), (1, 2), (2, 1), (2, 2)
HEADS = ["fluxpart", "flux3-interpreted", "flux3-compiled"]
CELLS = [("lstm", "tanh"), ("gru", "tanh"), ("rnn", "relu")]
COUNTS = [13, 37, 70]
W = 6
EVAL_FIRST = 3                                               # evaluation and predictions: the case's count of windows from this one on
CANCEL_MAX = 16.0                                            # 1e-5 / (2 * 3e-7): the operands' error, with a factor two to spare
KINDS3 = [("mse", "mse", "mse"), ("mae", "mae", "mae"), ("nseLoss", "nseLoss", "nseLoss"), ("nseLoss", "mse", "mae")]
ORDERS3 = list(itertools.permutations(range(3)))


def _case(k, wi, head, ci, T, ow, order=None):
    names = mt.FLUXPART_OUTPUTS if head == "fluxpart" else list(ct.FLUX3_OUTPUTS)
    order = ORDERS3[k % 6][:T] if order is None else order
    kinds = KINDS3[k % 4][:T]
    return dict(id=f"{k:02d}-I{WIDTHS[wi][0]}H{WIDTHS[wi][1]}-{head}-{CELLS[ci][0]}-T{T}-ow{ow}", widths=WIDTHS[wi], head=head, cell=CELLS[ci], T=T, ow=ow,
                lam=k % 2, count=COUNTS[k % 3], targets=[names[o] for o in order], kinds=kinds, agg="mean" if k % 5 == 0 else "sum",
                shuffled=k % 4 == 1, seed=1000 + k)


def _cases():
    out, k = [], 0
    for wi, head, ci in itertools.product(range(4), HEADS, range(3)):          # every triple: three targets, ow = 3
        out.append(_case(k, wi, head, ci, 3, 3))
        k += 1
    # two targets, ow = 1, and the targets in an order other than the outputs' (RECO before NEE)
    for wi, head, ci, T, ow, order in [(0, "fluxpart", 0, 2, 1, (2, 0)), (1, "flux3-interpreted", 1, 2, 3, (2, 0)), (2, "flux3-compiled", 2, 2, 1, (1, 2)),
                                       (3, "fluxpart", 1, 2, 3, (0, 2)), (3, "flux3-compiled", 0, 2, 3, (2, 1)), (0, "flux3-interpreted", 2, 3, 1, (2, 1, 0)),
                                       (1, "fluxpart", 2, 2, 1, (1, 0)), (2, "flux3-compiled", 1, 3, 1, (1, 2, 0))]:
        out.append(_case(k, wi, head, ci, T, ow, order))
        k += 1
    return out


CASES = _cases()
IDS = [c["id"] for c in CASES]


_FORCINGS = {}


def forcings():
    """the series' forcings with the light scaled to 0 .. 40 and the temperature to 22 +- a few degrees: computed once, left unchanged"""
    if not _FORCINGS:
        _, frc, _ = ct.series()
        sw = (frc["sw"] * np.float32(0.05)).astype(np.float32)
        ta = (np.float32(22.0) + np.float32(0.3) * (frc["ta"] - np.float32(10.0))).astype(np.float32)
        _FORCINGS.update(sw=sw, SW_IN=sw, ta=ta, TA=ta, vpd=frc["vpd"])
        for a in _FORCINGS.values():
            a.setflags(write=False)
    return _FORCINGS


def build(case):
    """-> (model, torch spelling, output index per target, X, forcings, target series (T of them), theta, selected starts, engine
    keywords selecting the same windows, all starts, jit)"""
    I, H = case["widths"]
    kind, cell_act = case["cell"]
    head = case["head"]
    if head == "fluxpart":
        model, fn_t, outs = mt.fluxpart_model(kind, case["targets"], I, H, cell_act=cell_act)
    else:
        model, fn_t, outs = mt.flux3_model(kind, case["targets"], I, H, cell_act=cell_act)
    X = ct.series()[0]
    frc = forcings()
    ys = mt.masked_targets(case["targets"], case["seed"], 0.2, "fluxpart" if head == "fluxpart" else "flux3")
    starts = ct.all_starts(ct.LROWS, W, case["lam"])
    theta = model.initialparameters(case["seed"])
    if case["shuffled"]:
        idx = np.random.default_rng(case["seed"]).permutation(len(starts))[:case["count"]].astype(np.int32)
        sel, kw = starts[idx], dict(idx=idx)
    else:
        sel, kw = starts[:case["count"]], dict(first=0, count=case["count"])
    return model, fn_t, outs, X, frc, ys, theta, sel, kw, starts, (1 if head == "flux3-compiled" else 0)
