"""The cases of tests/test_gpu_seq_fuzz.py without a GPU: every case as an input (the twin's own fp32 run reaches a tenth of the bar),
how often the generator had to redraw, what the cases cover, and what eh_create says to their descriptors before a device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

from easyhybrid_jl_amd import _lib as L

from tests import seq_fuzz_cases as fz
from tests import util

N = int(os.environ.get("EH_SEQ_FUZZ_N", "48"))
CLASSES = [(1, 1), (1, 2), (2, 1), (2, 2)]


@pytest.mark.parametrize("seed", range(N))
def test_case_inputs(seed):
    """tests/test_seq_closures.py `_input_reaches_a_tenth_of_the_bar`, on the case the generator accepted"""
    c = fz.case(seed)
    l64, g64, nv = c.ref
    el, en, ee = c.input_errors
    print(fz.describe(c), f"| fp32 twin against fp64: loss {el:.1e} norm {en:.1e} entries {ee:.1e}")
    assert nv >= 3 and float(np.linalg.norm(g64)) > 0
    assert el <= 0.1 * fz.TOL and en <= 0.1 * fz.TOL
    assert ee <= 0.1 * fz.ETOL
    assert ((c.I - 1) // 16 + 1, (c.H - 1) // 16 + 1) == (c.nbi, c.nbh) == fz.block_class(seed)
    assert c.count == len(c.sel) and (c.sel == c.starts[c.idx]).all() and c.idx.max() < len(c.starts)
    assert int(c.sel.max()) + c.W + c.lam <= fz.LROWS
    if fz.has_eval(seed):          # the evaluation sub-test's own input condition held too (it is part of what `case` accepts)
        e = fz.eval_reference(c)
        assert e is not None and e.first + e.count <= len(c.starts) and e.pred.shape == (e.count, c.ow)


def test_saturated_gates_are_an_input_question():
    """Seed 27's first draw, found by the extended run (EH_SEQ_FUZZ_N=400): W = 64 behind an identity Dense-in drives cell states past
    19, where 1 - tanh^2 is the last ulp of tanh.  The fp32 twin with torch's tanh holds a tenth of the entry-wise bar (4.0e-5 of 5e-5
    allowed), the same twin with tanh spelled 2 sigma(2z) - 1 loses 8.6e-4, the device (NNlib's fast forms) 1.5e-3: the input condition
    runs both spellings since, and this draw is redrawn."""
    import torch
    c = fz._draw(27, 0)
    assert (c.W, c.act, c.mech, c.I, c.H) == (64, "identity", "rs_components", 17, 2)
    assert not fz.acceptable(c)
    l64, g64, _ = c.ref
    one = util.elem_relerr(fz._twin(c, c.theta, c.sel, c.kind, torch.float32)[1], g64, 1e-3)
    assert one <= 0.1 * fz.ETOL < c.input_errors[2], (one, c.input_errors)
    assert fz.case(27).sub > 0


def test_workspace_cap_case_input():
    c = fz.ws_cap_case(own_fp32=True)
    (l64, g64, nv), (l32, g32, _) = c.ref, c.ref32
    n64 = float(np.linalg.norm(g64))
    assert nv > 0 and n64 > 0
    assert abs(l32 - l64) <= 0.1 * fz.TOL * abs(l64) and abs(float(np.linalg.norm(g32)) - n64) <= 0.1 * fz.TOL * n64, (l32, l64)
    assert util.elem_relerr(g32, g64, 1e-3) <= 0.1 * fz.ETOL, util.elem_relerr(g32, g64, 1e-3)


def test_at_most_a_tenth_of_the_seeds_needed_a_redraw():
    """the generator may not quietly narrow itself to easy inputs: a seed whose first draw was refused, or whose optimiser-step
    sub-test is dropped (the twin's own fp32 trajectory misses a tenth of that test's bar), counts"""
    redrawn = [s for s in range(N) if fz.case(s).sub > 0]
    dropped = [s for s in range(N) if fz.has_steps(s) and fz.steps_reference(fz.case(s)) is None]
    print("redrawn", redrawn, "optimiser steps dropped", dropped)
    assert len(set(redrawn) | set(dropped)) <= 0.1 * N, (redrawn, dropped)


def test_coverage():
    cs = [fz.case(s) for s in range(N)]
    of = lambda nb: [c for c in cs if (c.nbi, c.nbh) == nb]
    for nb in CLASSES:
        assert len(of(nb)) >= N // 4, nb
        assert {(c.head, c.jit) for c in of(nb)} >= {("mech", None), ("multi", None), ("prog", 0), ("prog", 1)}, nb
    assert {c.act for c in cs} == set(fz.ACTS) and {c.kind for c in cs} == set(fz.LOSSES)
    assert any(c.K >= 5 for c in cs)                                     # NN output rows of the second lane group
    assert any(c.P > 16 and c.I > 16 for c in cs)                        # the second predictor block with NBI = 2
    assert any(c.W == 64 for c in cs) and any(c.W == 1 for c in cs) and any(c.ow == c.W for c in cs)
    assert any(c.count % 64 == 0 for c in cs) and any(c.count == 1 for c in cs)
    assert any(c.n_fixed >= 1 and c.head != "prog" for c in cs) and any(c.n_global >= 2 for c in cs)
    assert any(not c.scale for c in cs)                                  # raw NN outputs
    assert {c.selection for c in cs} == set(fz.SELECTIONS)
    assert {c.max_blocks for c in cs} == {None, 1, 3}
    assert any(fz.has_steps(c.seed) and fz.steps_reference(c) is not None for c in cs)


@pytest.mark.parametrize("seed", range(N))
def test_eh_create_accepts_the_descriptor(seed):
    """tests/test_seq_closures.py: the case's descriptor gets as far as the device"""
    lib = L.lib()
    d = fz.case(seed).model.to_desc()
    h = C.c_void_p()
    rc = lib.eh_create(C.byref(d), C.byref(h))
    assert rc != L.EH_EUNSUPPORTED, lib.eh_last_error(None)
    if rc == L.EH_OK:
        assert h.value
        assert lib.eh_destroy(h) == L.EH_OK
    else:
        assert rc == L.EH_EHIP and b"no HIP device" in lib.eh_last_error(None) and not h.value
