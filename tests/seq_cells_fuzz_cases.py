"""Seeded random sequence-model cases around GRUCell and RNNCell for tests/test_seq_cells.py (CPU) and tests/test_gpu_seq_cells.py (GPU):
tests/seq_fuzz_cases.py's generator -- its parameter ranges, head forms, selections and input condition -- with the cell as one more
parameter and the fp64 twin of tests/seq_cells_twin.py as the reference.

`case(cell, seed)`, seed in range(N_PER_CELL), is deterministic: stream `np.random.default_rng((BASE, CELLS.index(cell), seed, sub))`.  Tied to
the seed, not drawn:

  * the (NBI, NBH) class is `seed % 4`: ten seeds per class and cell;
  * `seed // 4` picks the head form: 0 / 1 are closures 2 / 3 of tests/seq_closure_twin.py (EH_SEQ_HEAD_PROG) interpreted / compiled at run
    time, 2 is FluxPartModelQ10 (EH_SEQ_HEAD_MULTI), the other seven draw a single-output registry model (EH_SEQ_HEAD_MECH) -- so every
    class of every cell has each of the four;
  * an RNNCell's activation is `ACTS[(seed // 4) % 5]`: each of the five twice per class.

As there, an ill-conditioned draw is an input question: `case` walks sub-seeds until the case has three valid targets, a non-zero fp64
gradient, and the twin's own fp32 runs within a tenth of the project's bars of its fp64 run.  No case is dropped: every (cell, seed) gives
one.  tests/test_seq_cells.py caps how many may need a redraw.
"""
import types

import numpy as np
import torch

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho

from tests import seq_cells_twin as cw
from tests import seq_fuzz_cases as fz
from tests import util
from tests.test_gpu_fuzz import FORCING_RANGE, TABLES

TOL, ETOL = fz.TOL, fz.ETOL
BASE = 1_400_000
CELLS = ("gru", "rnn")
N_PER_CELL = 40
MAX_SUB = 20


def block_class(seed):
    """-> (NBI, NBH) of a seed"""
    return 1 + (seed % 4) // 2, 1 + seed % 2


def head_of(seed):
    """-> ("prog", jit) | ("multi", None) | ("mech", None)"""
    r = seed // 4
    return ("prog", r) if r < 2 else (("multi" if r == 2 else "mech"), None)


def _draw(cell, seed, sub):
    rng = np.random.default_rng((BASE, CELLS.index(cell), seed, sub))
    nbi, nbh = block_class(seed)
    head, jit = head_of(seed)
    I = int(rng.choice(fz.I_SMALL if nbi == 1 else fz.I_LARGE))
    H = int(rng.choice(fz.H_SMALL if nbh == 1 else fz.H_LARGE))
    P = int(rng.choice(fz.PS))
    W = int(rng.choice(fz.WS))
    ow = int(np.clip(rng.choice([1, 2, W // 2, W]), 1, W))
    lam = int(rng.choice(fz.LAMS))
    shift = int(rng.choice(fz.SHIFTS))
    count = int(rng.choice(fz.COUNTS))
    nan_frac = float(rng.choice(fz.NAN_FRACS))
    if count == 1:                                       # one window has its `ow` targets and no more: all of at least three steps, none missing
        W = W if W >= 3 else int(rng.choice([w for w in fz.WS if w >= 3]))
        ow, nan_frac = W, 0.0
    act = str(rng.choice(fz.ACTS))
    cell_act = fz.ACTS[(seed // 4) % 5] if cell == "rnn" else None
    kind = str(rng.choice(fz.LOSSES))
    selection = str(rng.choice(fz.SELECTIONS))
    max_blocks = [None, 1, 3][int(rng.integers(3))]
    preds = [f"x{i}" for i in range(P)]
    if head == "prog":
        cid = int(rng.choice([2, 3]))
        mech, scale = f"closure{cid}", True
        model, fn_t, out = cw.closure_model(cell, cid, I, H, act, cell_act or "tanh", True, preds)
        franges = fz.CLOSURE_FORCING_RANGE
    else:
        mech = "fluxpart" if head == "multi" else str(rng.choice(fz.SINGLE))
        mm = ho.MECH[mech][0]
        names = list(mm.params)
        target = str(rng.choice(list(mm.outputs)))
        kinds = rng.integers(0, 3, len(names))          # every parameter neural / global / fixed at random, at least one neural
        if not (kinds == 0).any():
            kinds[rng.integers(len(names))] = 0
        feeds = [j for j, n in enumerate(names) if n in fz.FEEDS.get(target, names)]
        if all(kinds[j] == 2 for j in feeds):            # (a target none of whose parameters is trained has no gradient at all)
            kinds[feeds[int(rng.integers(len(feeds)))]] = 0
        neural = [n for n, k in zip(names, kinds) if k == 0]
        glob = [n for n, k in zip(names, kinds) if k == 1]
        rng.shuffle(neural); rng.shuffle(glob)
        scale = bool(rng.random() < 0.6) or mech in fz.SCALED
        model = eh.constructHybridModel(preds, list(mm.forcings), [target], util.MECH_NAME[mech], dict(TABLES[mech]), neural, glob,
                                        hidden_layers=cw.chain(cell, I, H, cell_act or "tanh"), activation=act, scale_nn_outputs=scale)
        fn_t, out = fz.registry_mech(mech), list(mm.outputs).index(target)
        franges = FORCING_RANGE
    X = (0.6 * rng.standard_normal((P, fz.LROWS))).astype(np.float32)
    X[0] = np.cumsum(X[0]) * 0.2
    frc = {f: rng.uniform(*franges[f], fz.LROWS).astype(np.float32) for f in model.forcing}
    y = rng.uniform(0.5, 6, fz.LROWS).astype(np.float32)
    y[rng.random(fz.LROWS) < nan_frac] = np.nan
    starts = eh.split_into_sequences(X, y[None], input_window=W, output_window=ow, output_shift=shift, lead_time=lam).starts
    nwin = len(starts)
    if selection == "contiguous":                        # first > 0
        count = max(1, min(count, nwin - 1))
        first = int(rng.integers(1, nwin - count + 1))
        idx, kw = np.arange(first, first + count, dtype=np.int32), dict(first=first, count=count)
    else:
        count = min(count, nwin)
        if selection == "shuffled":
            idx = rng.permutation(nwin)[:count].astype(np.int32)
        else:
            idx = rng.integers(0, nwin, count).astype(np.int32)
            idx[-1] = idx[0]                             # (at least one window twice, where there are two)
        kw = dict(idx=idx)
    theta = model.initialparameters(int(rng.integers(1 << 30)))
    for a in (X, y, starts, idx, theta, *frc.values()):
        a.setflags(write=False)
    return types.SimpleNamespace(
        cell=cell, cell_act=cell_act, seed=seed, sub=sub, nbi=nbi, nbh=nbh, head=head, jit=jit, mech=mech, I=I, H=H, P=P, K=len(model.neural_param_names),
        W=W, ow=ow, lam=lam, shift=shift, count=count, nan_frac=nan_frac, act=act, scale=scale, kind=kind, selection=selection, max_blocks=max_blocks,
        model=model, fn_t=fn_t, out=out, X=X, frc=frc, y=y, theta=theta, starts=starts, idx=idx, sel=starts[idx], kw=kw)


def describe(c):
    return (f"{c.cell}{'' if c.cell_act is None else ':' + c.cell_act} seed {c.seed}.{c.sub} NBI{c.nbi} NBH{c.nbh} {c.head}{'' if c.jit is None else ' jit=%d' % c.jit} "
            f"{c.mech} I{c.I} H{c.H} P{c.P} K{c.K} W{c.W} ow{c.ow} lam{c.lam} shift{c.shift} n{c.count} {c.selection} nan{c.nan_frac} {c.act} "
            f"{'scaled' if c.scale else 'raw'} {c.kind} max_blocks {c.max_blocks}")


def _twin(c, dtype, tanh=torch.tanh):
    return cw.loss_and_grad(c.model, c.fn_t, c.out, c.theta, c.X, c.frc, c.y, c.sel, c.W, c.ow, c.lam, c.kind, dtype, tanh=tanh)


def input_errors(c):
    """tests/seq_fuzz_cases.py `input_errors`: the twin's fp32 runs (both spellings of tanh, the worse counts) against its fp64 run
    -> (n_valid, fp64 gradient norm, loss rel, norm rel, entry rel); fills c.ref"""
    l64, g64, nv = _twin(c, torch.float64)
    c.ref = (l64, g64, nv)
    n64 = float(np.linalg.norm(g64))
    if nv < 3 or not n64 > 0 or not np.isfinite(l64) or l64 == 0 or not np.isfinite(g64).all():
        return nv, n64, np.inf, np.inf, np.inf
    runs = [_twin(c, torch.float32, tanh) for tanh in (torch.tanh, fz.tanh_by_sigmoid)]
    return (nv, n64, max(abs(l32 - l64) / abs(l64) for l32, _, _ in runs), max(abs(float(np.linalg.norm(g32)) - n64) / n64 for _, g32, _ in runs),
            max(util.elem_relerr(g32, g64, 1e-3) for _, g32, _ in runs))


def acceptable(c):
    nv, n64, el, en, ee = input_errors(c)
    c.input_errors = (el, en, ee)
    return nv >= 3 and n64 > 0 and el <= 0.1 * TOL and en <= 0.1 * TOL and ee <= 0.1 * ETOL


_CASES = {}


def case(cell, seed):
    """-> the accepted case of (cell, seed): model, twin closure, data, selection, engine keywords, fp64 reference `ref`"""
    if (cell, seed) not in _CASES:
        for sub in range(MAX_SUB):
            c = _draw(cell, seed, sub)
            if acceptable(c):
                break
        else:
            raise AssertionError(f"{cell} seed {seed}: no well-conditioned case in {MAX_SUB} sub-seeds")
        _CASES[(cell, seed)] = c
    return _CASES[(cell, seed)]
