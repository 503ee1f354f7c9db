"""Sequence models around recorded closures and multi-output registry models, without a GPU: the two spellings of every test closure
against each other, the parity cases of tests/test_gpu_seq_closures.py as inputs (the twin's own fp32 run reaches a tenth of the bar), and
what eh_create says to their descriptors before a device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

from easyhybrid_jl_amd import _lib as L
from easyhybrid_jl_amd import program

from tests import seq_closure_twin as ct
from tests import util

TOL, ETOL = 1e-5, 5e-4          # tests/test_gpu_seq.py


@pytest.mark.parametrize("cid", [1, 2])
def test_the_two_spellings_of_a_closure_agree(cid):
    fn, fn_t, table, forc, outs = ct.CLOSURES[cid][:5]
    rng = np.random.default_rng(cid)
    n = 1000
    rng_of = dict(ta=(-15.0, 35.0), sw=(0.0, 800.0), vpd=(0.0, 30.0))
    args = {f: rng.uniform(*rng_of[f], n) for f in forc}
    args.update({p: rng.uniform(lo + 1e-3, hi, n) for p, (_, lo, hi) in table.items()})
    a = fn(**args)
    b = fn_t(**{k: torch.tensor(v, dtype=torch.float64) for k, v in args.items()})
    assert list(a) == list(b) == list(outs)
    for name in outs:
        assert np.allclose(a[name], b[name].numpy(), rtol=1e-12, atol=1e-12), name
    if cid == 2:
        assert (args["vpd"] > 10.0).any() and (args["vpd"] <= 10.0).any()          # both branches of the where


def test_the_flux_closure_as_recorded():
    pg = program.trace(ct.flux3_np, list(ct.FLUX3_TABLE), ct.FLUX3_FORCINGS, ct.FLUX3_OUTPUTS)
    ops = {program.OP_NAMES[c[0]] for c in pg.code}
    assert len(pg.code) >= 20 and {"exp", "select", "log", "gt"} <= ops
    assert pg.outputs == ("nee", "gpp", "reco") and set(pg.forcings) == {"sw", "ta", "vpd"} and len(pg.out) == 3
    m2, _, o2 = ct.closure_model(2, 15, 15)
    m3, _, o3 = ct.closure_model(3, 15, 15)
    assert (o2, o3) == (2, 0) and m2.to_desc().target_output[0] == 2 and m3.to_desc().target_output[0] == 0
    d = m2.to_desc()
    assert d.mech == L.EH_MECH_PROGRAM and d.prog_n_out == 3 and d.prog_n_forc == 3 and d.n_params == 4
    assert [d.param_kind[j] for j in range(4)] == [L.PAR_NEURAL, L.PAR_NEURAL, L.PAR_GLOBAL, L.PAR_FIXED]


def test_every_pairing_is_covered():
    seen = {ct.variant(si, ci) for si in range(len(ct.SHAPES)) for ci in range(len(ct.COUNTS))}
    assert {v[0] for v in seen} == {1, 2, 3} and {v[1] for v in seen} == {"tanh", "sigmoid"}
    assert {v[2] for v in seen} == {True, False} and {v[0] for v in seen if not v[2]} == {1}
    assert {v[3] for v in seen} == {"mse", "nseLoss", "mae"} and {v[4] for v in seen} == {True, False}
    assert {(v[0], v[3]) for v in seen} == {(c, l) for c in (1, 2, 3) for l in ("mse", "nseLoss", "mae")}


def _input_reaches_a_tenth_of_the_bar(model, fn_t, out, theta, X, frc, y, sel, W, ow, lam, kind):
    l64, g64, nv = ct.loss_and_grad(model, fn_t, out, theta, X, frc, y, sel, W, ow, lam, kind, torch.float64)
    l32, g32, _ = ct.loss_and_grad(model, fn_t, out, theta, X, frc, y, sel, W, ow, lam, kind, torch.float32)
    n64 = float(np.linalg.norm(g64))
    assert nv > 0 and n64 > 0
    assert abs(l32 - l64) <= 0.1 * TOL * abs(l64) and abs(float(np.linalg.norm(g32)) - n64) <= 0.1 * TOL * n64, (l32, l64)
    assert util.elem_relerr(g32, g64, 1e-3) <= 0.1 * ETOL, util.elem_relerr(g32, g64, 1e-3)


@pytest.mark.parametrize("ci", range(len(ct.COUNTS)), ids=[f"n{c}" for c in ct.COUNTS])
@pytest.mark.parametrize("si", range(len(ct.SHAPES)), ids=ct.SHAPE_IDS)
def test_parity_case_inputs(si, ci):
    model, fn_t, out, X, frc, y, theta, sel, W, ow, lam, kind, _, _ = ct.case(si, ci)
    _input_reaches_a_tenth_of_the_bar(model, fn_t, out, theta, X, frc, y, sel, W, ow, lam, kind)


@pytest.mark.parametrize("target", ["NEE", "GPP", "RECO"])
def test_fluxpart_case_inputs(target):
    model, fn_t, out = ct.fluxpart_model(target, 6, 2)
    X, frc, tg = ct.series()
    W, ow, lam = 5, 2, 1
    _input_reaches_a_tenth_of_the_bar(model, fn_t, out, model.initialparameters(31), X, frc, tg[target], ct.all_starts(ct.LROWS, W, lam)[:17], W, ow, lam, "mse")


def _descriptors():
    return {"closure 1": ct.closure_model(1, 15, 15)[0].to_desc(), "closure 2": ct.closure_model(2, 15, 15)[0].to_desc(),
            "FluxPartModelQ10": ct.fluxpart_model("RECO", 15, 15)[0].to_desc()}


@pytest.mark.parametrize("which", ["closure 1", "closure 2", "FluxPartModelQ10"])
def test_eh_create_accepts_the_descriptor(which):
    """a sequence model around a recorded closure / a registry model with three outputs gets as far as the device"""
    lib = L.lib()
    d = _descriptors()[which]
    h = C.c_void_p()
    rc = lib.eh_create(C.byref(d), C.byref(h))
    assert rc != L.EH_EUNSUPPORTED, lib.eh_last_error(None)
    if rc == L.EH_OK:
        assert h.value
        assert lib.eh_destroy(h) == L.EH_OK
    else:
        assert rc == L.EH_EHIP and b"no HIP device" in lib.eh_last_error(None) and not h.value


@pytest.mark.parametrize("which", ["closure 1", "closure 2", "FluxPartModelQ10"])
def test_a_second_target_is_still_refused(which):
    lib = L.lib()
    d = _descriptors()[which]
    d.n_targets = 2
    d.target_output[1] = 0
    h = C.c_void_p()
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED
    assert b"no kernel for a sequence model with 2 targets" in lib.eh_last_error(None) and not h.value
