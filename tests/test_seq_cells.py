"""GRUCell and RNNCell in sequence models, without a GPU: parameter tree and descriptor, what eh_create says before a device is touched,
the twin of tests/seq_cells_twin.py against torch's own cells and against central differences, and the fuzz cases of
tests/seq_cells_fuzz_cases.py as inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L

from tests import seq_cells_fuzz_cases as cfz
from tests import seq_cells_twin as cw
from tests import seq_closure_twin as ct
from tests import util

RBQ10 = dict(ct.RBQ10_TABLE)
CELLS = [("gru", "tanh"), ("rnn", "tanh"), ("rnn", "relu")]
CELL_IDS = ["gru", "rnn-tanh", "rnn-relu"]


def _tutorial(kind, I=15, H=15, cell_act="tanh", **kw):
    """the reference's LSTM tutorial with the cell's name edited: hidden_layers = Chain(Recurrence(GRUCell(15 => 15)))"""
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"],
                                   hidden_layers=cw.chain(kind, I, H, cell_act), activation="tanh", scale_nn_outputs=True, **kw)


# ---- parameter tree and descriptor -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,G,n_theta", [("gru", 3, 1742), ("rnn", 1, 782), ("lstm", 4, 2222)])
def test_parameter_tree(kind, G, n_theta):
    m = _tutorial(kind)
    assert m.n_theta == 45 + (2 * G * 15 * 15 + 2 * G * 15) + 240 + 16 + 1 == n_theta
    assert m.hidden_layers == [15, 15, 15] and m.lstm_layer == 1 and m.cell == kind
    assert m.layer_activations == ["tanh", {"gru": "gru", "rnn": "rnn:tanh", "lstm": "lstm"}[kind], "tanh"]
    assert [(n, s) for _, _, n, s in m.leaves()] == [("weight", (15, 2)), ("bias", (15,)), ("weight_ih", (G * 15, 15)), ("weight_hh", (G * 15, 15)),
                                                    ("bias_ih", (G * 15,)), ("bias_hh", (G * 15,)), ("weight", (15, 15)), ("bias", (15,)), ("weight", (1, 15)), ("bias", (1,))]
    assert int(m.l2_mask(None, "weight").sum()) == 270 and int(m.l2_mask(None, "bias").sum()) == 31      # (cell leaves are not named weight / bias)
    assert m.opt_branches() == {"ps": (0, n_theta - 1), "Q10": (n_theta - 1, n_theta)}
    theta = m.initialparameters(3)
    assert theta.shape == (n_theta,) and theta.dtype == np.float32
    n_cell = 2 * G * 15 * 15 + 2 * G * 15
    off = 45
    for _, li, name, shape in m.leaves():                           # U(+-1/sqrt(H)) on every cell leaf
        if li == 1:
            leaf = theta[off:off + int(np.prod(shape))]
            assert np.abs(leaf).max() <= 1 / np.sqrt(15) and np.abs(leaf).max() > 0.8 / np.sqrt(15), name
            off += int(np.prod(shape))
    assert off == 45 + n_cell
    layers, glob = m.unpack(theta)
    (w0, b0), cell, (w2, b2), (w3, b3) = layers
    assert cell["weight_ih"].shape == (G * 15, 15) and cell["weight_hh"].shape == (G * 15, 15) and cell["bias_ih"].shape == cell["bias_hh"].shape == (G * 15,)
    flat = np.concatenate([w0.flatten(order="F"), b0, cell["weight_ih"].flatten(order="F"), cell["weight_hh"].flatten(order="F"), cell["bias_ih"],
                           cell["bias_hh"], w2.flatten(order="F"), b2, w3.flatten(order="F"), b3, glob["Q10"]])
    assert np.array_equal(flat, theta)                              # unpack round-trips
    p = cw.unpack(m, torch.tensor(theta))                           # the twin reads the same leaves
    assert np.array_equal(p["w_ih"].numpy(), cell["weight_ih"]) and np.array_equal(p["b_hh"].numpy(), cell["bias_hh"]) and np.array_equal(p["w_out"].numpy(), w3)


def test_descriptors():
    assert (L.EH_LAYER_LSTM, L.EH_LAYER_GRU, L.EH_LAYER_RNN) == (16, 24, 32)
    for kind, cell_act, code in (("gru", "tanh", L.EH_LAYER_GRU), ("rnn", "tanh", L.EH_LAYER_RNN), ("rnn", "relu", L.EH_LAYER_RNN + L.ACTIVATIONS["relu"]),
                                 ("rnn", "identity", L.EH_LAYER_RNN + 4)):
        d = _tutorial(kind, 6, 2, cell_act).to_desc()
        assert (d.activation, d.n_nets, d.n_hidden, list(d.hidden[:3]), list(d.net_activation[:3])) == (L.EH_ACT_PER_NET, 0, 3, [6, 2, 2], [0, code, 0])
    assert C.sizeof(L.ModelDesc) == _tutorial("lstm").to_desc().struct_size       # eh_model_desc keeps its size
    assert repr(eh.GRUCell(3, 4)) == "GRUCell(3 => 4)" and repr(eh.RNNCell(3, 4, "relu")) == "RNNCell(3 => 4, relu)" and eh.RNNCell(3, 4).activation == "tanh"
    with pytest.raises(NotImplementedError, match="no device implementation"):
        eh.RNNCell(3, 4, "gelu")


# ---- eh_create, before a device is touched -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cell_act", CELLS, ids=CELL_IDS)
def test_eh_create_reaches_the_device(kind, cell_act):
    """around RbQ10, FluxPartModelQ10 and a recorded closure; both block counts"""
    models = [_tutorial(kind, 15, 15, cell_act), _tutorial(kind, 32, 32, cell_act), _tutorial(kind, 17, 17, cell_act),
              cw.fluxpart_model(kind, "GPP", 15, 15, cell_act=cell_act)[0], cw.closure_model(kind, 2, 20, 9, cell_act=cell_act)[0]]
    for m in models:
        with pytest.raises(eh.EngineError, match="no HIP device"):
            m.engine(0)


@pytest.mark.parametrize("kind,cell_act", CELLS, ids=CELL_IDS)
def test_the_lstm_refusals_hold_for_the_cell(kind, cell_act):
    lib = L.lib()
    h = C.c_void_p()
    err = lambda: lib.eh_last_error(None)
    desc = lambda **kw: _tutorial(kind, cell_act=cell_act, **kw).to_desc()
    code = desc().net_activation[1]
    for I, H in ((33, 15), (15, 33)):
        d = desc(I=I, H=H)
        assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for LSTM widths" in err()
    d = desc()
    d.n_targets = 2; d.target_output[1] = 0
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for a sequence model with 2 targets" in err()
    d = desc(input_batchnorm=True)
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for input BatchNorm" in err()
    d = desc()
    d.n_nets = 1; d.net_n_predictors[0] = 2; d.net_activation[0] = code
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for a MultiNN sequence model" in err()
    for other in (code, L.EH_LAYER_LSTM, L.EH_LAYER_GRU, L.EH_LAYER_RNN + 1):             # two recurrent layers of any kinds
        d = desc()
        d.net_activation[2] = other
        assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EINVAL and b"2 EH_LAYER_LSTM layers" in err()
    d = desc()
    d.net_activation[0] = code; d.net_activation[1] = 0
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EINVAL and b"hidden layer 0" in err()
    d = desc()
    d.hidden[2] = 14
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for an LSTM layer" in err()
    d = desc()
    d.net_activation[1] = L.EH_LAYER_RNN + 5                                               # no such activation: not a layer code at all
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"unknown activation id 37" in err()
    assert not h.value
    # the Python front door
    mk = lambda hl, **kw: eh.constructHybridModel(["a"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=hl, **kw)
    cell = lambda: cw.make_cell(kind, 8, 8, cell_act)
    with pytest.raises(NotImplementedError, match="stacked or non-final"):
        mk(eh.Chain(eh.Recurrence(cell()), eh.Recurrence(eh.LSTMCell(8, 8))))
    with pytest.raises(NotImplementedError, match="return_sequence"):
        mk(eh.Chain(eh.Recurrence(cell(), return_sequence=False)))
    with pytest.raises(NotImplementedError, match="MultiNN"):
        eh.constructHybridModel({"rb": ["a"]}, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["Q10"], hidden_layers=eh.Chain(eh.Recurrence(cell())))
    with pytest.raises(NotImplementedError, match="Dropout|stacked or non-final"):
        mk(eh.Chain(eh.Dropout(0.5), eh.Recurrence(cell())))


# ---- the twin against torch's cells and against central differences -----------------------------------------------------------------
@pytest.mark.parametrize("kind,cell_act", CELLS, ids=CELL_IDS)
def test_twin_cell_step_is_torchs(kind, cell_act):
    """weights copied in, five steps from a zero state, fp64: the op-by-op step and torch.nn.GRUCell / RNNCell agree to 1e-12"""
    I, H, n = 5, 7, 6
    torch.manual_seed(3)
    ref = (torch.nn.GRUCell(I, H) if kind == "gru" else torch.nn.RNNCell(I, H, nonlinearity=cell_act)).double()
    p = dict(w_ih=ref.weight_ih.detach(), w_hh=ref.weight_hh.detach(), b_ih=ref.bias_ih.detach(), b_hh=ref.bias_hh.detach())
    assert p["w_ih"].shape == (cw.GATES[kind] * H, I)
    xs = torch.randn(5, n, I, dtype=torch.float64)
    h = h_ref = torch.zeros(n, H, dtype=torch.float64)
    for t in range(5):
        h, _ = cw.cell_step(kind, p, xs[t], h, None, cw.tw.ACT[cell_act])
        with torch.no_grad():
            h_ref = ref(xs[t], h_ref)
        assert float((h - h_ref).abs().max()) <= 1e-12, t
    assert float(h.abs().max()) > 0.05


@pytest.mark.parametrize("kind,cell_act", CELLS + [("rnn", "swish")], ids=CELL_IDS + ["rnn-swish"])
def test_twin_gradient_is_the_central_difference(kind, cell_act):
    """Autograd through the whole twin against central differences of its fp64 loss, every entry of theta.  The bar is the one
    tests/test_seq_fuzz.py holds a reference to -- a tenth of the device's bars: 1e-6 on the gradient's norm, 5e-5 entry-wise down to 1e-3 of
    the largest entry.  With step 1e-5 on O(1) parameters the difference quotient's truncation error is ~1e-10 f''' and its rounding error
    ~1e-16 |loss| / 1e-5 = 1e-11, both several orders below that.  (relu: no pre-activation of this case lies within the step of its kink.)"""
    model, fn_t, out = cw.rbq10_model(kind, 5, 4, cell_act=cell_act)
    X, frc, _ = ct.series()
    y = ct.target_series(1)
    W, ow, lam = 5, 2, 1
    sel = ct.all_starts(ct.LROWS, W, lam)[3:40]
    theta = model.initialparameters(5).astype(np.float64)
    _, g, nv = cw.loss_and_grad(model, fn_t, out, theta, X, frc, y, sel, W, ow, lam, "mse")
    assert nv > 30 and np.isfinite(g).all()
    yt = torch.tensor(cw.tw.targets_of(y, sel, W, ow, lam), dtype=torch.float64)
    loss = lambda th: float(cw.tw.loss_of(cw.forward(model, fn_t, out, th, X, frc, sel, W, ow)[0], yt, "mse"))
    eps, fd = 1e-5, np.zeros_like(g)
    for i in range(len(theta)):
        e = np.zeros_like(theta); e[i] = eps
        fd[i] = (loss(theta + e) - loss(theta - e)) / (2 * eps)
    n = float(np.linalg.norm(fd))
    print(kind, cell_act, "norm rel", abs(float(np.linalg.norm(g)) - n) / n, "entry rel", util.elem_relerr(g, fd, 1e-3))
    assert abs(float(np.linalg.norm(g)) - n) <= 0.1 * cfz.TOL * n
    assert util.elem_relerr(g, fd, 1e-3) <= 0.1 * cfz.ETOL


def test_gru_bias_gradients_differ_in_the_n_block_only():
    """what the device test of the same name checks, on the twin: b_hn sits inside the reset gate's product, b_in outside"""
    model, fn_t, out = cw.rbq10_model("gru", 6, 5)
    X, frc, _ = ct.series()
    _, g, _ = cw.loss_and_grad(model, fn_t, out, model.initialparameters(1), X, frc, ct.target_series(1), ct.all_starts(ct.LROWS, 6, 0)[:50], 6, 2, 0)
    H, o = 5, 6 * 2 + 6 + 15 * 6 + 15 * 5
    bih, bhh = g[o:o + 3 * H], g[o + 3 * H:o + 6 * H]
    assert np.array_equal(bih[:2 * H], bhh[:2 * H]) and np.abs(bih[2 * H:] - bhh[2 * H:]).max() > 1e-3 * np.abs(bih[2 * H:]).max()


# ---- the fuzz cases as inputs -------------------------------------------------------------------------------------------------------
FUZZ = [(cell, seed) for cell in cfz.CELLS for seed in range(cfz.N_PER_CELL)]


@pytest.mark.parametrize("cell,seed", FUZZ, ids=[f"{c}-{s}" for c, s in FUZZ])
def test_fuzz_case_inputs(cell, seed):
    c = cfz.case(cell, seed)
    l64, g64, nv = c.ref
    el, en, ee = c.input_errors
    print(cfz.describe(c), f"| fp32 twin against fp64: loss {el:.1e} norm {en:.1e} entries {ee:.1e}")
    assert np.isfinite(l64) and np.isfinite(g64).all() and nv >= 1          # the twin is finite and a target is valid
    assert nv >= 3 and float(np.linalg.norm(g64)) > 0 and el <= 0.1 * cfz.TOL and en <= 0.1 * cfz.TOL and ee <= 0.1 * cfz.ETOL
    assert ((c.I - 1) // 16 + 1, (c.H - 1) // 16 + 1) == (c.nbi, c.nbh) == cfz.block_class(seed)
    assert c.count == len(c.sel) and int(c.sel.max()) + c.W + c.lam <= cfz.fz.LROWS
    assert c.model.cell == cell and c.model.cell_activation == c.cell_act


def test_fuzz_coverage_and_redraws():
    for cell in cfz.CELLS:
        cs = [cfz.case(cell, s) for s in range(cfz.N_PER_CELL)]
        for nb in [(1, 1), (1, 2), (2, 1), (2, 2)]:
            of = [c for c in cs if (c.nbi, c.nbh) == nb]
            assert len(of) == 10, (cell, nb)
            assert {(c.head, c.jit) for c in of} == {("mech", None), ("multi", None), ("prog", 0), ("prog", 1)}, (cell, nb)
            if cell == "rnn":
                assert {c.cell_act for c in of} == set(cfz.fz.ACTS), nb
        assert {c.kind for c in cs} == set(cfz.fz.LOSSES) and {c.act for c in cs} == set(cfz.fz.ACTS)
        assert any(c.W >= 63 for c in cs) and any(c.W <= 2 for c in cs) and any(c.P > 16 for c in cs) and any(c.count > 64 for c in cs)
        redrawn = [c.seed for c in cs if c.sub > 0]
        print(cell, "redrawn", redrawn)
        assert len(redrawn) <= 0.1 * cfz.N_PER_CELL, (cell, redrawn)      # (the generator may not narrow itself to easy inputs: tests/test_seq_fuzz.py)


@pytest.mark.parametrize("cell,seed", FUZZ, ids=[f"{c}-{s}" for c, s in FUZZ])
def test_eh_create_accepts_the_fuzz_descriptor(cell, seed):
    lib = L.lib()
    d = cfz.case(cell, seed).model.to_desc()
    h = C.c_void_p()
    rc = lib.eh_create(C.byref(d), C.byref(h))
    assert rc != L.EH_EUNSUPPORTED, lib.eh_last_error(None)
    if rc == L.EH_OK:
        assert h.value and lib.eh_destroy(h) == L.EH_OK
    else:
        assert rc == L.EH_EHIP and b"no HIP device" in lib.eh_last_error(None) and not h.value
