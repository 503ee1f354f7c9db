"""Recorded activations without a device: the recorder, the model surface, the planner's answers through ctypes, the generated device source
compiled for the host and for gfx950, and the inputs of tests/test_gpu_activations.py."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
from easyhybrid_jl_amd.program import ACT_MAX_CONST, ACT_MAX_PROG, eval_activation, trace_activation
from oracle import hybrid_oracle as ho

from tests import act_cases as ac
from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- 1. the recorder -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ac.ACT_CASES))
def test_case_records_and_its_tape_is_the_closure(name):
    """The host evaluation of the recorded program -- forward tape, reverse sweep seeded with 1, fp64, the constants as the closure spells
    them (the program's own are their fp32 values: 0.01 is 0.00999999978, which alone is 2e-10 of the result) -- equals the closure and
    the derivative written out by hand to 1e-12; the hand derivative equals central differences to 1e-6 away from its kinks."""
    fn, dfn, kinks = ac.ACT_CASES[name]
    prog = trace_activation(fn)
    assert 1 <= len(prog.code) <= ACT_MAX_PROG and len(prog.consts) <= ACT_MAX_CONST and prog.out[0] >= 28
    z = np.linspace(-6.0, 6.0, 4801)
    z = z[np.all([np.abs(z - k) >= 1e-3 for k in kinks], axis=0)] if kinks else z
    a, da = eval_activation(prog, z)
    assert np.max(np.abs(a - fn(z))) <= 1e-12 and np.max(np.abs(da - dfn(z))) <= 1e-12
    h = 1e-5
    assert np.max(np.abs((fn(z + h) - fn(z - h)) / (2 * h) - dfn(z))) <= 1e-6
    if name == "tanh_twin":
        assert [c[0] for c in prog.code] == [9]              # the one `tanh` operation ...
    if name == "sigmoid_twin":
        assert [c[0] for c in prog.code] == [10]             # ... and 1 / (1 + exp(-z)) the one `sigmoid` operation: the device's own functions


def test_models_hard_sigmoid_records_as_it_stands():
    a = trace_activation(eh.hard_sigmoid)
    b = trace_activation(eh.hard_sigmoid_act)
    assert a.words() == b.words() and a.consts == b.consts


# ---- 2. what the recorder refuses --------------------------------------------------------------------------------------------------------
def test_trace_activation_refusals():
    with pytest.raises(TypeError, match="not a traced per-sample value"):
        trace_activation(lambda x: 1.0)
    with pytest.raises(NotImplementedError, match="reduction"):
        trace_activation(lambda x: np.mean(x * x))
    with pytest.raises(NotImplementedError, match="reduction"):
        trace_activation(lambda x: np.sum(abs(x)))
    with pytest.raises(NotImplementedError, match="only elementwise operations"):
        trace_activation(lambda x: np.cumsum(x))

    def branchy(x):
        return x if x > 0 else 0.0 * x
    with pytest.raises(NotImplementedError, match="Python control flow"):
        trace_activation(branchy)
    with pytest.raises(NotImplementedError, match="takes 2 arguments"):
        trace_activation(lambda x, alpha: alpha * x)

    def long_one(x):
        for k in range(ACT_MAX_PROG + 1):
            x = np.sin(x)
        return x
    with pytest.raises(NotImplementedError, match=f"{ACT_MAX_PROG + 1} operations"):
        trace_activation(long_one)

    def many_constants(x):
        return sum(np.sin(x * (1.5 + k)) for k in range(ACT_MAX_CONST + 1))
    with pytest.raises(NotImplementedError, match="constants"):
        trace_activation(many_constants)
    assert len(trace_activation(lambda x: x * 1.0 + 0.0 * 3.0).code) >= 1      # (folding is the loss recorder's)


# ---- 3. the model surface ----------------------------------------------------------------------------------------------------------------
def _single(hidden, activation, **kw):
    return eh.constructHybridModel(["a", "b", "c"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], hidden_layers=hidden,
                                   activation=activation, scale_nn_outputs=True, **kw)


def test_model_surface():
    # a callable in all three places
    m = _single([16, 16], eh.softplus)
    d = m.to_desc()
    assert isinstance(m.activation, eh.RecordedActivation) and isinstance(m.activation, str) and m.layer_activations is None
    assert (d.activation, d.n_nets, list(d.net_activation[:3])) == (L.EH_ACT_PER_NET, 0, [8, 8, 0])          # one for all: nothing collapses
    assert len(m.act_programs()) == 1 and m.act_program_structs()[0].n_instr == len(m.activation.program.code)
    m = _single(eh.Chain(eh.Dense(16, 32, "tanh"), eh.Dense(32, 8, lambda x: x ** 2)), eh.leakyrelu)
    d = m.to_desc()
    assert m.layer_activations[1] == "tanh" and [type(a) for a in m.layer_activations] == [eh.RecordedActivation, str, eh.RecordedActivation]
    assert (d.activation, list(d.net_activation[:4])) == (L.EH_ACT_PER_NET, [8, L.ACTIVATIONS["tanh"], 9, 0])
    mm = eh.constructHybridModel({"rb": ["a"], "Q10": ["b", "c"]}, ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), [],
                                 hidden_layers={"rb": [24, 12], "Q10": [30, 20]}, activation={"rb": eh.softplus, "Q10": "tanh"}, scale_nn_outputs=True)
    d = mm.to_desc()
    assert mm.net_activations[1] == "tanh" and isinstance(mm.activation["rb"], eh.RecordedActivation)
    assert (d.activation, d.n_nets, list(d.net_activation[:3])) == (L.EH_ACT_PER_NET, 2, [8, 0, 0])
    # identical programs are stored once, whatever the closures are called; a constant makes another program
    same = _single(eh.Chain(eh.Dense(16, 16, lambda v: np.where(v > 0.0, v, 0.01 * v)), eh.Dense(16, 16, ac.leakyrelu02)), eh.leakyrelu)
    assert list(same.to_desc().net_activation[:3]) == [8, 8, 9] and len(same.act_programs()) == 2
    # np.tanh stays the built-in one, strings keep their meaning, what is refused stays refused
    plain = _single([16, 16], np.tanh)
    assert plain.activation == "tanh" and type(plain.activation) is str and plain.to_desc().activation == L.ACTIVATIONS["tanh"] and not plain.act_programs()
    assert _single(eh.Chain(eh.Dense(16, 16, np.tanh)), "tanh").layer_activations is None
    for name in ("gelu", "softplus", "elu", "leakyrelu"):
        with pytest.raises(NotImplementedError, match="has no device implementation"):
            _single([16, 16], name)
    # gain 1.0, size of theta
    m = _single([16, 16], eh.softplus)
    th, th_sig = m.initialparameters(3), _single([16, 16], "sigmoid").initialparameters(3)
    assert th.size == m.n_theta == 3 * 16 + 16 + 16 * 16 + 16 + 16 + 1 + 1 and np.array_equal(th, th_sig)      # (sigmoid's gain is 1.0 as well)
    # the entries survive copies
    m2 = copy.deepcopy(m)
    assert m2.activation == m.activation and m2.activation.program == m.activation.program and m2.to_desc().net_activation[0] == 8
    # a ninth distinct program
    nine = [(lambda c: (lambda x: np.where(x > 0.0, x, (0.1 + 0.05 * c) * x)))(k) for k in range(9)]
    with pytest.raises(NotImplementedError, match="9 distinct recorded activations"):
        _single(eh.Chain(*[eh.Dense(4, 4, f) for f in nine[1:]]), nine[0])


def test_python_refusals_ahead_of_any_upload():
    sq = lambda x: x ** 2
    with pytest.raises(NotImplementedError, match="layer-wise form"):
        _single([200, 64, 32], sq)
    with pytest.raises(NotImplementedError, match="layer-wise form"):
        _single([16, 16, 16, 16], sq)
    with pytest.raises(NotImplementedError, match="Recurrence"):
        eh.constructHybridModel(["a", "b", "c"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(8, 8))), activation=sq, scale_nn_outputs=True)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        _single(eh.Chain(eh.Dense(16, 16, sq), eh.BatchNorm(16)), "tanh")
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        _single(eh.Chain(eh.LayerNorm(16), eh.Dense(16, 16, "tanh")), sq)
    with pytest.raises(NotImplementedError, match="precision = 'bf16_fwd'"):
        _single([96, 96], sq, precision="bf16_fwd")
    with pytest.raises(NotImplementedError, match="Dropout next to a recorded activation"):
        _single(eh.Chain(eh.Dense(16, 16, sq), eh.Dropout(0.5)), "tanh")
    from easyhybrid_jl_amd.train import _members_refusals, DataConfig, TrainConfig
    with pytest.raises(NotImplementedError, match="kernels compiled at run time, which a group of models does not use"):
        _members_refusals(_single([16, 16], sq), TrainConfig(), DataConfig(), [])


# ---- 4. the library's answers, no device ---------------------------------------------------------------------------------------------------
def _create_acts(d, progs, n=None):
    h = C.c_void_p()
    st = L.lib().eh_create_activations(C.byref(d), progs, len(progs) if n is None else n, C.byref(h))
    assert not h.value or L.lib().eh_destroy(h) == 0
    return st, L.lib().eh_last_error(None).decode()


def _good():
    m = ac.model_from_spec(ac.make_spec("16x16_softplus_elu"))
    return m.to_desc(), m.act_program_structs()


def test_eh_create_keeps_its_answer_to_the_recorded_ids():
    for j in range(8):
        d, _ = _good()
        d.net_activation[0] = L.EH_ACT_RECORDED + j
        h = C.c_void_p()
        assert L.lib().eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and not h.value
        assert L.lib().eh_last_error(None).decode() == f"eh_create: unknown activation id {8 + j} for hidden layer 0"
    d, progs = _good()
    st, msg = _create_acts(d, progs)
    import torch
    if not torch.cuda.is_available():        # accepted by the planner: the next thing it needs is a device
        assert st == L.EH_EHIP and "no HIP device" in msg


def _mutated(fn):
    d, progs = _good()
    fn(d, progs)
    return _create_acts(d, progs)


def test_eh_create_activations_refuses_malformed_programs():
    W = lambda op, a=0, b=0, c=0: op | a << 8 | b << 16 | c << 24
    cases = [
        (lambda d, p: setattr(p[0], "n_instr", 0), L.EH_EUNSUPPORTED, "activation program 0 has 0 instructions (1..32)"),
        (lambda d, p: setattr(p[1], "n_instr", 33), L.EH_EUNSUPPORTED, "activation program 1 has 33 instructions (1..32)"),
        (lambda d, p: setattr(p[0], "n_const", 9), L.EH_EUNSUPPORTED, "activation program 0 has 9 constants (0..8)"),
        (lambda d, p: p[0].code.__setitem__(0, W(18, 0)), L.EH_EUNSUPPORTED, "activation program 0, instruction 0 has unknown opcode 18"),
        (lambda d, p: p[0].code.__setitem__(0, W(13, 28)), L.EH_EINVAL, "activation program 0, instruction 0, operand 0 names slot 28 (undefined at that point"),
        (lambda d, p: p[0].code.__setitem__(0, W(13, 1)), L.EH_EINVAL, "operand 0 names slot 1 (undefined"),                     # slot 1 holds nothing
        (lambda d, p: p[0].code.__setitem__(0, W(13, 12 + p[0].n_const)), L.EH_EINVAL, "operand 0 names slot 14 (undefined"),    # a constant it does not have
        (lambda d, p: p[0].code.__setitem__(0, W(13, 0, 5)), L.EH_EINVAL, "operand 1 names slot 5 (undefined at that point, or a non-zero unused operand)"),
        (lambda d, p: setattr(p[1], "out_slot", 28 + p[1].n_instr), L.EH_EINVAL, "activation program 1: output slot 33"),
        (lambda d, p: setattr(p[1], "out_slot", 0), L.EH_EINVAL, "activation program 1: output slot 0"),
        (lambda d, p: d.net_activation.__setitem__(1, 10), L.EH_EINVAL, "hidden layer 1 names recorded activation 2, 2 programs were given"),
        (lambda d, p: d.net_activation.__setitem__(1, 8), L.EH_EINVAL, "activation program 1 is named by no hidden layer"),
        (lambda d, p: d.net_activation.__setitem__(1, 16), L.EH_EUNSUPPORTED, "eh_create: no kernel for an LSTM layer"),          # (the descriptor's own refusals come first)
        (lambda d, p: setattr(d, "activation", 0), L.EH_EINVAL, "2 activation programs, but activation = 0"),
    ]
    for fn, status, text in cases:
        st, msg = _mutated(fn)
        assert st == status and text in msg, (st, msg, text)
    d, progs = _good()
    assert _create_acts(d, progs, n=9)[0] == L.EH_EINVAL and "9 activation programs (0..8)" in L.lib().eh_last_error(None).decode()
    st, msg = _create_acts(d, progs, n=0)          # no programs: eh_create's own answer
    assert st == L.EH_EUNSUPPORTED and msg == "eh_create: unknown activation id 8 for hidden layer 0"


def test_eh_create_activations_refuses_what_is_out_of_scope():
    def wide(d, p):
        d.n_hidden = 3; d.hidden[0], d.hidden[1], d.hidden[2] = 200, 64, 32; d.net_activation[2] = 0

    def deep(d, p):
        d.n_hidden = 4; d.hidden[2] = d.hidden[3] = 16; d.net_activation[2] = d.net_activation[3] = 0

    def wide3(d, p):
        d.n_hidden = 3; d.hidden[0], d.hidden[1], d.hidden[2] = 96, 64, 32; d.net_activation[2] = 0

    def seq(d, p):
        d.n_hidden = 3; d.hidden[0] = d.hidden[1] = d.hidden[2] = 15; d.net_activation[0], d.net_activation[1], d.net_activation[2] = 8, L.EH_LAYER_LSTM, 9

    def bn(d, p):
        d.n_hidden = 3; d.hidden[2] = 16; d.net_activation[2] = L.EH_LAYER_BATCHNORM

    def ln(d, p):
        d.n_hidden = 3; d.hidden[2] = 16; d.net_activation[2] = L.EH_LAYER_LAYERNORM + 1
    for fn, text in [(wide, "not for the layer-wise form this network would run on (P = 3, K = 1, widest layer 200, 3 hidden layers)"),
                     (deep, "not for the layer-wise form this network would run on (P = 3, K = 1, widest layer 16, 4 hidden layers)"),
                     (wide3, "widest layer 96, 3 hidden layers"),
                     (seq, "recorded activations are not built for sequence models"),
                     (bn, "recorded activations are not built for chains with BatchNorm / LayerNorm layers"),
                     (ln, "recorded activations are not built for chains with BatchNorm / LayerNorm layers")]:
        st, msg = _mutated(fn)
        assert st == L.EH_EUNSUPPORTED and text in msg, (st, msg)


# ---- 5. the generated source ---------------------------------------------------------------------------------------------------------------
def _source(names):
    arr = ac.act_structs(names)
    n = L.lib().eh_activation_source(arr, len(names), None, 0)
    assert n > 1
    buf = C.create_string_buffer(n)
    assert L.lib().eh_activation_source(arr, len(names), buf, n - 1) == n and L.lib().eh_activation_source(arr, len(names), buf, n) == 0
    return buf.value.decode()


BATCHES = [list(ac.ACT_CASES)[:8], list(ac.ACT_CASES)[8:]]          # (a handle, and a generated header, holds up to eight programs)


def test_activation_source_refuses_malformed_programs():
    arr = ac.act_structs(["square"])
    arr[0].code[0] = 200
    assert L.lib().eh_activation_source(arr, 1, None, 0) == L.EH_EUNSUPPORTED and "unknown opcode 200" in L.lib().eh_last_error(None).decode()
    assert L.lib().eh_activation_source(arr, 0, None, 0) == L.EH_EINVAL


@pytest.mark.parametrize("batch", [0, 1])
def test_generated_source_on_the_host_matches_the_closures(batch, tmp_path):
    """eh_jit_act.inc behind tests/act_host_shim.h as one stand-alone program (the C library's tanh / exp stand in for the device's):
    values and derivatives against the fp64 closures and hand derivatives, norm-wise to 1e-5."""
    names = BATCHES[batch]
    (tmp_path / "eh_jit_act.inc").write_text(_source(names))
    (tmp_path / "main.cpp").write_text(
        '#include "act_host_shim.h"\n#include "eh_jit_act.inc"\n'
        "int main() {\n"
        f"    for (int j = 0; j < {len(names)}; ++j)\n"
        "        for (int i = 0; i <= 480; ++i) {\n"
        "            const float z = -6.0f + 0.025f * (float)i + 0.0078125f;\n"          # (clear of the kinks at 0 and +-2.5)
        '            std::printf("%d %.9g %.9g %.9g\\n", j, (double)z, (double)eh_jit_act(j, z), (double)eh_jit_dact(j, z));\n'
        "        }\n    return 0;\n}\n")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.check_call([cxx, "-O1", "-std=c++17", f"-I{HERE}", f"-I{tmp_path}", str(tmp_path / "main.cpp"), "-o", str(tmp_path / "act_host")])
    rows = np.array([[float(v) for v in line.split()] for line in subprocess.check_output([str(tmp_path / "act_host")]).decode().splitlines()])
    assert rows.shape == (len(names) * 481, 4)
    for j, name in enumerate(names):
        fn, dfn, _ = ac.ACT_CASES[name]
        r = rows[rows[:, 0] == j]
        ea, ed = util.relerr(r[:, 2], fn(r[:, 1])), util.relerr(r[:, 3], dfn(r[:, 1]))
        print(f"{name}: host value relerr {ea:.2e}, derivative relerr {ed:.2e}")
        assert ea <= 1e-5 and ed <= 1e-5, (name, ea, ed)


@pytest.mark.parametrize("batch", [0, 1])
def test_generated_source_compiles_for_gfx950(batch, tmp_path):
    """the same text where the step kernels include it -- csrc/eh_device.hpp under EH_JIT_ACTPROG -- with a wrapper kernel, device only"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    names = BATCHES[batch]
    (tmp_path / "eh_jit_act.inc").write_text(_source(names))
    (tmp_path / "wrap.hip").write_text(
        '#define EH_JIT_ACTPROG 1\n#include "eh_device.hpp"\n'
        'extern "C" __global__ void act_wrap(int id, const float* z, long long n, float* a, float* da) {\n'
        "    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;\n"
        "    if (i < n) { a[i] = eh_act_id(id, z[i]); da[i] = eh_dact_z_id(id, z[i]); }\n}\n")
    out = tmp_path / "wrap.co"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{tmp_path}",
                           f"-I{ROOT}/easyhybrid.jl_amd/csrc", f"-I{ROOT}/include", "-c", str(tmp_path / "wrap.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    assert out.stat().st_size > 0


# ---- 6. the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------
TOL = 1e-5


@pytest.mark.parametrize("case,B", ac.MODEL_RUNS)
def test_gpu_inputs_are_well_posed(case, B):
    """The oracle's own fp32 loss and gradient within half of the parity bar of its fp64 ones, its fp32 Adam trajectory within a tenth of
    the trajectory bar of its fp64 one (the rule of tests/test_chain.py): what the device is held to is then the device's to miss."""
    r = ac.reference(case, B)
    el, eg = abs(r["l32"] - r["l64"]) / abs(r["l64"]), util.relerr(r["g32"], r["g64"])
    et = float(np.max(np.abs(r["t32"].astype(np.float64) - r["t64"]))) / max(1.0, float(np.max(np.abs(r["t64"]))))
    print(f"{case} B={B}: fp32 oracle against fp64: loss {el:.2e}, gradient {eg:.2e}, trajectory {et:.2e}")
    assert np.isfinite(r["l64"]) and r["nv"] > 0.8 * B and np.max(np.abs(r["g64"])) > 0
    assert el <= 0.5 * TOL and eg <= 0.5 * TOL
    assert et <= 0.1 * 3e-5
