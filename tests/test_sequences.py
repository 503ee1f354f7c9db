"""Sequence models without a GPU: the windows against hand-written index lists, the tutorial model's parameter tree and descriptor, and
the refusals eh_create / eh_set_sequences give before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L

RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}


def _tutorial(I=15, H=15, **kw):
    """docs/literate/tutorials/example_synthetic_lstm.jl: hidden_layers = Chain(Recurrence(LSTMCell(15 => 15)))"""
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"],
                                   hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(I, H))), activation="tanh", scale_nn_outputs=True, **kw)


# ---- windows ---------------------------------------------------------------------------------------------------------------------
def test_windows_against_hand_written_indices():
    L_ = 12
    x = np.stack([np.arange(L_, dtype=np.float32), 100 + np.arange(L_, dtype=np.float32)])
    y = (1000 + np.arange(L_, dtype=np.float32))[None]
    s = eh.split_into_sequences(x, y, input_window=5, output_window=2, output_shift=3, lead_time=1)
    assert s.starts.tolist() == [0, 3, 6] and s.starts.dtype == np.int32
    assert s.target_rows(0).tolist() == [4, 5]
    assert s.target_rows().tolist() == [[4, 5], [7, 8], [10, 11]]
    assert s.x.shape == (2, 5, 3) and s.y.shape == (1, 2, 3)
    assert s.x[0, :, 1].tolist() == [3, 4, 5, 6, 7] and s.x[1, :, 2].tolist() == [106, 107, 108, 109, 110]
    assert s.y[0, :, 0].tolist() == [1004, 1005] and s.y[0, :, 2].tolist() == [1010, 1011]


def test_windows_lead_zero_and_full_output_window():
    x = np.arange(7, dtype=np.float32)[None]
    s = eh.split_into_sequences(x, 10 * x, input_window=3, output_window=3, output_shift=1, lead_time=0)
    assert s.starts.tolist() == [0, 1, 2, 3, 4]
    assert s.target_rows(4).tolist() == [4, 5, 6]                  # prediction j against the target of its own input step
    assert np.array_equal(s.y[0], 10 * s.x[0])
    one = eh.split_into_sequences(x, x, input_window=7, output_window=1, lead_time=0)
    assert one.starts.tolist() == [0] and one.target_rows(0).tolist() == [6]


def test_window_argument_errors():
    x = np.zeros((1, 6), np.float32)
    with pytest.raises(ValueError, match="windows too long"):
        eh.split_into_sequences(x, x, input_window=5, lead_time=2)               # W + lam > L
    with pytest.raises(ValueError, match="lead_time"):
        eh.split_into_sequences(x, x, input_window=2, lead_time=-1)
    with pytest.raises(ValueError, match="same time length"):
        eh.split_into_sequences(x, np.zeros((1, 5), np.float32))
    with pytest.raises(ValueError, match="output_window"):
        eh.split_into_sequences(x, x, input_window=2, output_window=3)
    with pytest.raises(ValueError, match="feature, time"):
        eh.split_into_sequences(np.zeros(6, np.float32), x)


def test_filter_sequences_drops_exactly_the_bad_windows():
    L_ = 14
    x = np.stack([np.arange(L_, dtype=np.float32), np.ones(L_, np.float32)])
    y = np.arange(L_, dtype=np.float32)[None].copy()
    x[1, 5] = np.nan                       # inside windows starting at 3, 4, 5 (W = 3)
    y[0, [9, 10]] = np.nan                 # every target of the window starting at 6 (rows 9, 10) -- one of two for 5 and 7
    s = eh.split_into_sequences(x, y, input_window=3, output_window=2, output_shift=1, lead_time=2)
    assert s.starts.tolist() == list(range(0, 10))
    f = eh.filter_sequences(s)
    assert f.starts.tolist() == [0, 1, 2, 7, 8, 9]
    assert f.x.shape == (2, 3, 6) and f.y.shape == (1, 2, 6) and not np.isnan(f.x).any()
    assert np.isnan(f.y[0, :, 3]).tolist() == [True, False]        # window 7: targets at rows 10, 11


# ---- the tutorial model -----------------------------------------------------------------------------------------------------------
def test_tutorial_model_parameter_tree():
    m = _tutorial()
    assert m.n_theta == 45 + 1920 + 240 + 16 + 1 == 2222
    assert m.hidden_layers == [15, 15, 15] and m.layer_activations == ["tanh", "lstm", "tanh"] and m.lstm_layer == 1
    assert [(n, s) for _, _, n, s in m.leaves()] == [("weight", (15, 2)), ("bias", (15,)), ("weight_ih", (60, 15)), ("weight_hh", (60, 15)),
                                                    ("bias_ih", (60,)), ("bias_hh", (60,)), ("weight", (15, 15)), ("bias", (15,)), ("weight", (1, 15)), ("bias", (1,))]
    assert int(m.l2_mask(None, "weight").sum()) == 30 + 225 + 15 == 270 and int(m.weight_mask().sum()) == 270
    assert int(m.l2_mask(None, "bias").sum()) == 15 + 15 + 1       # (bias_ih / bias_hh are not leaves named "bias")
    assert m.opt_branches() == {"ps": (0, 2221), "Q10": (2221, 2222)}
    theta = m.initialparameters(3)
    assert theta.shape == (2222,) and theta.dtype == np.float32
    lstm = theta[45:45 + 1920]
    assert np.abs(lstm).max() <= 1 / np.sqrt(15) and np.abs(lstm).max() > 0.9 / np.sqrt(15)      # U(+-1/sqrt(H)), every leaf
    layers, glob = m.unpack(theta)
    (w0, b0), cell, (w2, b2), (w3, b3) = layers
    assert w0.shape == (15, 2) and cell["weight_ih"].shape == (60, 15) and cell["weight_hh"].shape == (60, 15) and w3.shape == (1, 15)
    flat = np.concatenate([w0.flatten(order="F"), b0, cell["weight_ih"].flatten(order="F"), cell["weight_hh"].flatten(order="F"), cell["bias_ih"],
                           cell["bias_hh"], w2.flatten(order="F"), b2, w3.flatten(order="F"), b3, glob["Q10"]])
    assert np.array_equal(flat, theta)                             # unpack round-trips


def test_tutorial_model_descriptor():
    d = _tutorial().to_desc()
    assert (d.activation, d.n_nets, d.n_hidden, list(d.hidden[:3]), list(d.net_activation[:3])) == (
        L.EH_ACT_PER_NET, 0, 3, [15, 15, 15], [L.ACTIVATIONS["tanh"], L.EH_LAYER_LSTM, L.ACTIVATIONS["tanh"]])
    assert L.EH_LAYER_LSTM == 16 and L.EH_MAX_SEQ_WINDOW == 64
    d = _tutorial(6, 2).to_desc()
    assert list(d.hidden[:3]) == [6, 2, 2]


def test_other_recurrent_chains_are_refused_with_the_reason():
    mk = lambda hl, **kw: eh.constructHybridModel(["a"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=hl, **kw)
    with pytest.raises(NotImplementedError, match="stacked or non-final"):
        mk(eh.Chain(eh.Recurrence(eh.LSTMCell(8, 8)), eh.Recurrence(eh.LSTMCell(8, 8))))
    with pytest.raises(NotImplementedError, match="stacked or non-final"):
        mk(eh.Chain(eh.Dense(4, 8, "tanh"), eh.Recurrence(eh.LSTMCell(8, 8))))
    with pytest.raises(NotImplementedError, match="return_sequence"):
        mk(eh.Chain(eh.Recurrence(eh.LSTMCell(8, 8), return_sequence=False)))
    with pytest.raises(NotImplementedError, match="only LSTMCell"):
        mk(eh.Chain(eh.Recurrence(eh.Dense(8, 8))))
    with pytest.raises(NotImplementedError, match="MultiNN"):
        eh.constructHybridModel({"rb": ["a"]}, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["Q10"], hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(8, 8))))


# ---- refusals of the C ABI, before a device is touched ----------------------------------------------------------------------------
def test_eh_create_refuses_malformed_lstm_descriptors():
    lib = L.lib()
    h = C.c_void_p()
    err = lambda: lib.eh_last_error(None)

    def desc(**kw):
        d = _tutorial(**kw).to_desc()
        return d
    d = desc()
    d.net_activation[0] = L.EH_LAYER_LSTM; d.net_activation[1] = 0                     # LSTM at layer 0
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EINVAL and b"hidden layer 0" in err()
    d = desc()
    d.net_activation[2] = L.EH_LAYER_LSTM                                               # two LSTM layers
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EINVAL and b"2 EH_LAYER_LSTM layers" in err()
    d = desc()
    d.hidden[2] = 14                                                                    # head Dense not H x H
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for an LSTM layer" in err()
    d = desc()
    d.n_hidden = 2
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for an LSTM layer" in err()
    for I, H in ((33, 15), (15, 33)):
        d = desc(I=I, H=H)
        assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for LSTM widths" in err()
    d = desc()
    d.n_nets = 1; d.net_n_predictors[0] = 2; d.net_activation[0] = L.EH_LAYER_LSTM      # MultiNN: net_activation[k] is network k's
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for a MultiNN sequence model" in err()
    d = desc(input_batchnorm=True)
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for input BatchNorm" in err()
    d = desc()
    d.n_targets = 2; d.target_output[1] = 0                                             # more than one target
    assert lib.eh_create(C.byref(d), C.byref(h)) == L.EH_EUNSUPPORTED and b"no kernel for a sequence model with 2 targets" in err()
    assert not h.value
    # a well-formed one gets as far as the device
    with pytest.raises(eh.EngineError, match="no HIP device"):
        _tutorial().engine(0)
    with pytest.raises(eh.EngineError, match="no HIP device"):
        _tutorial(32, 32).engine(0)


def test_eh_set_sequences_null_handle():
    lib = L.lib()
    st = (C.c_int32 * 2)(0, 1)
    assert lib.eh_set_sequences(None, 0, 5, 1, 1, st, 2) == L.EH_EINVAL


def test_train_refuses_sequence_kwargs_on_a_feed_forward_model():
    m = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=[8])
    cols = eh.synthetic.make_synth_rbq10(64, 1)
    with pytest.raises(ValueError, match="no Recurrence layer"):
        eh.train(m, cols, nepochs=1, sequence_kwargs=dict(input_window=4))


def test_split_data_windows():
    m = _tutorial()
    cols = eh.synthetic.make_synth_rbq10(60, 1, 0.2)
    cols["sw_pot"][7] = np.nan
    (Xf, y, wtr), (_, _, wva) = eh.split_data(cols, m, sequence_kwargs=dict(input_window=4, output_window=2, lead_time=1))
    X, forc = Xf
    assert X.shape == (2, 60) and forc["ta"].shape == (60,) and y["reco"].shape == (60,)       # no row dropped: both splits index the series
    allw = np.concatenate([wtr.starts, wva.starts])
    keep = [a for a in range(0, 60 - 4 - 1 + 1) if not a <= 7 <= a + 3 and not np.isnan(cols["reco"][[a + 3, a + 4]]).all()]
    assert allw.tolist() == keep
    assert len(wtr.starts) == round(0.8 * len(keep))
    assert wtr.input_window == 4 and wtr.output_window == 2 and wtr.lead_time == 1
