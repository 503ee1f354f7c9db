"""Dropout in hidden-layer chains, the parts that need no GPU: the generator's known answers, the twin against the oracle's own
torch twin, how a Chain with Dropout layers is read (and refused), and the three new symbols of the library."""
import ctypes

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
from oracle import hybrid_oracle as ho
from oracle import torch_twin as tt
from tests import dropout_twin as dt
from tests import util


def _hex(words):
    return " ".join(f"{int(np.asarray(w).reshape(-1)[0]):08x}" for w in words)


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    assert _hex(dt.philox4x32_10(*ctr, *key)) == want


def test_mask_rule():
    assert dt.threshold(0.5) == 1 << 31 and dt.threshold(0.0) == 0
    assert dt.threshold(0.2) == int(np.floor(float(np.float32(0.2)) * 2.0 ** 32))          # the float32 rate of the C ABI
    assert dt.threshold(np.nextafter(np.float32(1), np.float32(0))) <= 0xFFFFFFFF
    assert dt.invp(0.5) == np.float32(2) and dt.invp(0.2).dtype == np.float32
    m = dt.keep_mask(161803, 3, 50, 1, 18, 0.5)
    assert m.shape == (50, 18) and m.dtype == bool
    # word u & 3 of call (k, 32 l + (u >> 2)): unit 6 of sample 7 is word 2 of the call with counter (7, 33, 3, 0)
    w = dt.philox4x32_10(7, 33, 3, 0, 161803, 0)
    assert m[7, 6] == (int(w[2]) >= 1 << 31)
    # the step's high word and the seed's high word are part of counter and key
    assert not np.array_equal(dt.keep_mask(161803, 3, 50, 1, 18, 0.5), dt.keep_mask(161803, 3 + (1 << 32), 50, 1, 18, 0.5))
    assert not np.array_equal(dt.keep_mask(161803, 3, 50, 1, 18, 0.5), dt.keep_mask(161803 + (1 << 32), 3, 50, 1, 18, 0.5))


@pytest.mark.parametrize("case", ["rbq10", "chain", "bn"])
def test_twin_with_all_keep_masks_is_the_oracles_twin(case):
    if case == "chain":
        spec = ho.HybridSpec(2, [16, 32, 8], "rbq10", dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"], ["reco"], "tanh", True,
                             layer_activations=["tanh", "swish", "sigmoid"])
    else:
        spec = ho.rbq10_spec((16, 16), "sigmoid" if case == "bn" else "tanh", True)
        spec.input_batchnorm = case == "bn"
    X, f, y = ho.make_synth_rbq10(77, 5, 0.1)
    X = (X / np.float32(50)).astype(np.float32)
    theta = ho.init_theta(spec, 2, np.float32).astype(np.float64)
    l0, g0 = tt.loss_and_grad(spec, theta, X, f, y)
    masks = [np.ones((77, w), bool) for w in spec.hidden]
    l1, g1, nv = dt.loss_and_grad(spec, theta, X, f, y, masks, [1.0] * len(masks))
    l2, g2, _ = dt.loss_and_grad(spec, theta, X, f, y)
    assert nv == int(np.sum(~np.isnan(y["reco"])))
    assert abs(l1 - l0) <= 1e-12 * abs(l0) and util.relerr(g1, g0) <= 1e-12
    assert abs(l2 - l0) <= 1e-12 * abs(l0) and util.relerr(g2, g0) <= 1e-12
    # and a mask does something: the gradient of a dropped unit's incoming weights is zero
    masks[0][:, 3] = False
    _, g3, _ = dt.loss_and_grad(spec, theta, X, f, y, masks, [1.0] * len(masks))
    W0 = g3[:spec.hidden[0] * 2].reshape(2, spec.hidden[0]).T
    assert np.all(W0[3] == 0) and np.any(W0[2] != 0)


def _model(hidden_layers, **kw):
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                   hidden_layers=hidden_layers, activation="tanh", scale_nn_outputs=True, **kw)


def test_chain_parsing_positions():
    D, Dr, Ch = eh.Dense, eh.Dropout, eh.Chain
    m = _model(Ch(D(16, 16, "tanh"), Dr(0.2), D(16, 16, "tanh")))
    assert m.hidden_layers == [16, 16, 16] and m.dropout == pytest.approx([0.0, 0.2, 0.0]) and m.layer_activations is None
    # as the first element: the layer the reference prepends (Dense(in_dim, first_h, activation))
    m = _model(Ch(Dr(0.5), D(16, 24, "tanh"), Dr(0.25)))
    assert m.hidden_layers == [16, 24] and m.dropout == [0.5, 0.25]
    # per-layer activations keep their layers
    m = _model(Ch(D(16, 32, "swish"), Dr(0.5), D(32, 8, "sigmoid")))
    assert m.hidden_layers == [16, 32, 8] and m.dropout == [0.0, 0.5, 0.0] and m.layer_activations == ["tanh", "swish", "sigmoid"]
    # Dropout(0) is Lux's NoOpLayer: the same model as the chain without it
    a, b = _model(Ch(D(16, 16, "tanh"), Dr(0), D(16, 16, "tanh"))), _model(Ch(D(16, 16, "tanh"), D(16, 16, "tanh")))
    assert a.dropout is None and a.NN == b.NN and a.n_theta == b.n_theta
    assert _model([16, 16]).dropout is None
    assert repr(Dr(0.5)) == "Dropout(0.5)"


def test_chain_parsing_refusals():
    D, Dr, Ch = eh.Dense, eh.Dropout, eh.Chain
    with pytest.raises(NotImplementedError, match="two Dropout layers in a row"):
        _model(Ch(D(16, 16, "tanh"), Dr(0.2), Dr(0.3)))
    with pytest.raises(NotImplementedError, match="two Dropout layers in a row"):
        _model(Ch(D(16, 16, "tanh"), Dr(0.2), Dr(0)))
    for p in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="0 <= p < 1"):
            Dr(p)
    with pytest.raises(NotImplementedError, match="dims"):
        Dr(0.5, dims=1)
    with pytest.raises(NotImplementedError, match="MultiNN"):
        eh.constructHybridModel({"rb": ["sw_pot"], "Q10": ["dsw_pot"]}, ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), [],
                                hidden_layers=Ch(D(8, 8, "tanh"), Dr(0.5)), activation="tanh")
    with pytest.raises(NotImplementedError, match="per-wave fused family"):
        _model(Ch(D(16, 128, "tanh"), Dr(0.5)))
    with pytest.raises(NotImplementedError, match="per-wave fused family"):
        _model(Ch(D(16, 16, "tanh"), Dr(0.5), D(16, 16, "tanh"), D(16, 16, "tanh")))
    # the refusals that were there keep firing for what triggered them
    class Other:
        pass
    with pytest.raises(NotImplementedError, match="only Dense layers have a device kernel"):
        _model(Ch(D(16, 16, "tanh"), Other()))
    with pytest.raises(NotImplementedError, match="only Dense layers have a device kernel"):
        _model(Ch(D(16, 16, "tanh"), Dr(0.5), Other()))
    with pytest.raises(NotImplementedError, match="stacked or non-final"):
        _model(Ch(eh.Recurrence(eh.LSTMCell(8, 8)), D(8, 8, "tanh")))
    with pytest.raises(NotImplementedError, match="stacked or non-final"):
        _model(Ch(Dr(0.5), eh.Recurrence(eh.LSTMCell(8, 8))))
    with pytest.raises(ValueError, match="empty Chain"):
        _model(Ch(Dr(0.5)))


def test_the_library_exports_the_dropout_entry_points():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("eh_set_dropout", "eh_get_dropout", "eh_dropout_mask"):
        assert getattr(lib, name) is not None and name in L.SIGNATURES
    assert L.lib().eh_version() == 4
