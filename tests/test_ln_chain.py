"""LayerNorm layers inside hidden-layer chains, without a GPU: chain parsing, parameter tree, masks and descriptor, what the constructor and
eh_create refuse before a device is touched, and the twin of tests/ln_chain_twin.py against torch's own layer_norm."""
import ctypes as C

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L

from tests import ln_chain_twin as tw

RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}


def _model(hl, P=3, act="tanh", **kw):
    return eh.constructHybridModel([f"x{i}" for i in range(P)], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=hl, activation=act, **kw)


def _issue_chain():
    return eh.Chain(eh.Dense(16, 16, "tanh"), eh.LayerNorm(16), eh.Dense(16, 8, "relu"), eh.LayerNorm(8, "sigmoid"))


def test_chain_parsing_and_widths_from_layernorm_dims():
    m = _model(_issue_chain())
    # Dense(P, 16, tanh) in front (first_h from the chain), then the four layers, then Dense(8, 1)
    assert m.hidden_layers == [16, 16, 16, 8, 8]
    assert m.layer_activations == ["tanh", "tanh", "ln:identity", "relu", "ln:sigmoid"]
    assert m.NN == [(16, 3), (16, 16), (16, 16), (8, 16), (8, 8), (1, 8)] and m.ln_layers == [2, 4] and m.bn_layers == [] and m.norm_layers == [2, 4]
    assert m.layernorm == {2: 1e-5, 4: 1e-5} and m.batchnorm is None
    # a chain may begin or end with one: first_h / last_h come from its dims; a leading one sits behind the Dense(P -> n) put in front
    m = _model(eh.Chain(eh.LayerNorm(16), eh.Dense(16, 12, "tanh")))
    assert m.hidden_layers == [16, 16, 12] and m.ln_layers == [1] and m.NN[0] == (16, 3) and m.NN[-1] == (1, 12)
    m = _model(eh.Chain(eh.Dense(5, 7, "relu"), eh.LayerNorm((7,), "swish", affine=False, epsilon=1e-3)))
    assert m.hidden_layers == [5, 7, 7] and m.layer_activations[-1] == "ln0:swish" and m.NN[-1] == (1, 7) and m.layernorm == {2: 1e-3}
    assert repr(eh.LayerNorm(16)) == "LayerNorm(16, identity)" and repr(eh.LayerNorm(8, "sigmoid")) == "LayerNorm(8, sigmoid)"
    # both normalisers in one chain
    m = _model(eh.Chain(eh.BatchNorm(8), eh.Dense(8, 8, "tanh"), eh.LayerNorm(8)))
    assert m.bn_layers == [1] and m.ln_layers == [3] and m.norm_layers == [1, 3] and m.layer_activations == ["tanh", "bn:identity", "tanh", "ln:identity"]
    with pytest.raises(ValueError, match=r"LayerNorm\(9\), the layer in front of it gives 16"):
        _model(eh.Chain(eh.Dense(16, 16), eh.LayerNorm(9)))
    with pytest.raises(ValueError, match="takes 4 inputs"):
        _model(eh.Chain(eh.LayerNorm(16), eh.Dense(4, 4)))


def test_theta_layout_initial_values_and_unpack_round_trip():
    m = _model(_issue_chain())
    names = [(li, name, shape) for _, li, name, shape in m.leaves()]
    # a LayerNorm's leaves: bias first, then scale (the reverse of BatchNorm's)
    assert names == [(0, "weight", (16, 3)), (0, "bias", (16,)), (1, "weight", (16, 16)), (1, "bias", (16,)), (2, "bias", (16,)), (2, "scale", (16,)),
                     (3, "weight", (8, 16)), (3, "bias", (8,)), (4, "bias", (8,)), (4, "scale", (8,)), (5, "weight", (1, 8)), (5, "bias", (1,))]
    assert m.n_nn == 64 + 272 + 32 + 136 + 16 + 9 and m.n_theta == m.n_nn + 1
    th = m.initialparameters(0)
    assert th.shape == (m.n_theta,) and th.dtype == np.float32
    assert np.array_equal(th[64 + 272:64 + 272 + 32], np.r_[np.zeros(16), np.ones(16)])      # bias = zeros, then scale = ones
    layers, glob = m.unpack(th)
    assert len(layers) == 6 and isinstance(layers[2], dict) and isinstance(layers[0], tuple) and list(layers[2]) == ["bias", "scale"]
    assert np.array_equal(layers[2]["scale"], np.ones(16)) and np.array_equal(layers[2]["bias"], np.zeros(16))
    assert np.array_equal(layers[4]["scale"], np.ones(8)) and np.array_equal(layers[4]["bias"], np.zeros(8))
    assert layers[3][0].shape == (8, 16) and layers[3][1].shape == (8,) and list(glob) == ["Q10"]
    # round trip on distinct values: the leaves in order, matrices column-major, are theta again
    th = np.arange(m.n_theta, dtype=np.float32)
    layers, glob = m.unpack(th)
    flat = []
    for l in layers:
        flat += [l["bias"], l["scale"]] if isinstance(l, dict) and l else ([] if isinstance(l, dict) else [l[0].flatten(order="F"), l[1]])
    assert np.array_equal(np.concatenate(flat + [glob["Q10"]]), th)
    # the twin reads the same layout
    tl, tg = tw.unpack(m, torch.tensor(th))
    assert np.array_equal(tl[3]["weight"].numpy(), layers[3][0]) and np.array_equal(tl[4]["scale"].numpy(), layers[4]["scale"]) and tg.numel() == 1
    assert np.array_equal(tl[4]["bias"].numpy(), layers[4]["bias"])
    assert m.opt_branches() == {"ps": (0, m.n_nn), "Q10": (m.n_nn, m.n_nn + 1)}
    # affine = false adds no leaf
    m0 = _model(eh.Chain(eh.Dense(16, 16), eh.LayerNorm(16, affine=False)))
    assert [n for _, _, n, _ in m0.leaves()] == ["weight", "bias"] * 3 and m0.unpack(m0.initialparameters(1))[0][2] == {}
    # a chain with both: each kind in its own order
    mb = _model(eh.Chain(eh.BatchNorm(8), eh.LayerNorm(8)))
    assert [(li, n) for _, li, n, _ in mb.leaves()][2:6] == [(1, "scale"), (1, "bias"), (2, "bias"), (2, "scale")]


def test_weight_l2_leaves_layernorm_out():
    m = _model(_issue_chain())
    th = np.random.default_rng(3).standard_normal(m.n_theta).astype(np.float32)
    layers, _ = m.unpack(th)
    manual = sum(float((l[0].astype(np.float64) ** 2).sum()) for l in layers if isinstance(l, tuple))
    mw, mb = m.l2_mask(None, "weight"), m.l2_mask(None, "bias")
    assert mw.sum() == 48 + 256 + 128 + 8 and mb.sum() == 16 + 16 + 8 + 1
    assert float((th[mw].astype(np.float64) ** 2).sum()) == pytest.approx(manual, rel=1e-12)
    assert tw.weight_l2(m, th) == pytest.approx(manual, rel=1e-12)
    o = 0
    for _, li, n, shape in m.leaves():
        k = int(np.prod(shape))
        if li in m.ln_layers:
            assert not mw[o:o + k].any() and not mb[o:o + k].any() and not m.weight_mask()[o:o + k].any()
        o += k


def test_descriptor_codes_and_size():
    m = _model(eh.Chain(eh.Dense(16, 16, "tanh"), eh.LayerNorm(16), eh.Dense(16, 8, "relu"), eh.LayerNorm(8, "sigmoid", affine=False)), input_batchnorm=True)
    d = m.to_desc()
    plain = _model([16, 16]).to_desc()
    assert d.struct_size == plain.struct_size == C.sizeof(L.ModelDesc)
    assert d.n_hidden == 5 and list(d.hidden)[:5] == [16, 16, 16, 8, 8] and d.n_nets == 0 and d.activation == L.EH_ACT_PER_NET and d.input_batchnorm == 1
    assert list(d.net_activation)[:5] == [0, 0, L.EH_LAYER_LAYERNORM + 4, 2, L.EH_LAYER_LAYERNORM + L.EH_LAYER_LN_NOAFFINE + 1]
    assert L.EH_LAYER_LAYERNORM == 56 and L.EH_LAYER_LAYERNORM + L.EH_LAYER_LN_NOAFFINE + 4 == 68
    # a LayerNorm layer counts towards the eight hidden layers
    with pytest.raises(NotImplementedError, match="hidden layers"):
        _model(eh.Chain(*([eh.Dense(8, 8), eh.LayerNorm(8)] * 4))).to_desc()
    assert _model(eh.Chain(*([eh.Dense(8, 8), eh.LayerNorm(8)] * 3 + [eh.Dense(8, 8)]))).to_desc().n_hidden == 8


def test_refusals_of_the_constructor():
    with pytest.raises(NotImplementedError, match="LayerNorm layers in a MultiNN model"):
        eh.constructHybridModel({"rb": ["a"], "Q10": ["b"]}, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), [], hidden_layers=eh.Chain(eh.Dense(8, 8), eh.LayerNorm(8)))
    with pytest.raises(NotImplementedError, match="LayerNorm layer next to a Dropout"):
        _model(eh.Chain(eh.Dense(8, 8), eh.Dropout(0.1), eh.LayerNorm(8)))
    with pytest.raises(NotImplementedError, match="LayerNorm layer next to a Recurrence"):
        _model(eh.Chain(eh.LayerNorm(8), eh.Recurrence(eh.LSTMCell(8, 8))))
    with pytest.raises(NotImplementedError, match=r"LayerNorm\(\(4, 8\)\): only a 1-D shape"):
        eh.LayerNorm((4, 8))
    with pytest.raises(NotImplementedError, match=r"LayerNorm\(dims = 1\)"):
        eh.LayerNorm(8, dims=1)
    with pytest.raises(NotImplementedError, match="precision = 'bf16' with LayerNorm layers"):
        _model(eh.Chain(eh.Dense(8, 8), eh.LayerNorm(8)), precision="bf16")
    with pytest.raises(NotImplementedError, match="no device implementation"):
        eh.LayerNorm(8, "gelu")
    with pytest.raises(NotImplementedError, match="rows of up to 1024 features"):
        eh.LayerNorm(1025)
    for eps in (0.0, -1e-5):
        with pytest.raises(ValueError, match="epsilon"):
            eh.LayerNorm(8, epsilon=eps)
    with pytest.raises(ValueError, match="at least one unit"):
        eh.LayerNorm(0)


def _create(d):
    lib, h = L.lib(), C.c_void_p()
    rc = lib.eh_create(C.byref(d), C.byref(h))
    msg = lib.eh_last_error(None)
    if rc == L.EH_OK:
        assert h.value and lib.eh_destroy(h) == L.EH_OK
    return rc, msg, h


def test_eh_create_before_a_device_is_touched():
    chains = [_issue_chain(), eh.Chain(eh.LayerNorm(16), eh.Dense(16, 16, "tanh")), eh.Chain(eh.Dense(5, 130), eh.LayerNorm(130, "swish", affine=False)),
              eh.Chain(eh.LayerNorm(1024)), eh.Chain(eh.LayerNorm(1)), eh.Chain(eh.BatchNorm(8), eh.Dense(8, 8, "tanh"), eh.LayerNorm(8))]
    for hl in chains:
        for bn in (False, True):
            rc, msg, h = _create(_model(hl, input_batchnorm=bn).to_desc())      # well formed: the constructor gets as far as the device
            assert rc == L.EH_OK or (rc == L.EH_EHIP and b"no HIP device" in msg and not h.value), msg
            assert b"BatchNorm" not in msg or any(isinstance(l, eh.BatchNorm) for l in hl.layers)
    d = _model(_issue_chain()).to_desc()
    d.hidden[2] = 12                                                   # a LayerNorm of another width than the layer in front of it
    rc, msg, h = _create(d)
    assert rc == L.EH_EINVAL and b"LayerNorm layer 2 has width 12, the layer in front of it 16" in msg and not h.value
    d = _model(_issue_chain()).to_desc()
    d.net_activation[0] = L.EH_LAYER_LAYERNORM
    rc, msg, _ = _create(d)
    assert rc == L.EH_EINVAL and b"EH_LAYER_LAYERNORM at hidden layer 0" in msg
    d = _model(_issue_chain()).to_desc()
    d.n_nets = 1; d.net_n_predictors[0] = 3; d.net_activation[0] = L.EH_LAYER_LAYERNORM + 4
    rc, msg, _ = _create(d)
    assert rc == L.EH_EUNSUPPORTED and b"no kernel for LayerNorm layers in a MultiNN model" in msg and b"BatchNorm" not in msg
    d = _model(_issue_chain()).to_desc()
    d.net_activation[1] = L.EH_LAYER_LSTM
    rc, msg, _ = _create(d)
    assert rc == L.EH_EUNSUPPORTED and b"both a LayerNorm layer and a recurrent layer" in msg and b"BatchNorm" not in msg
    d = _model(eh.Chain(eh.Dense(16, 1024), eh.LayerNorm(1024))).to_desc()
    d.hidden[1] = d.hidden[2] = 1025                                   # wider than a wave's registers hold
    rc, msg, _ = _create(d)
    assert rc == L.EH_EUNSUPPORTED and b"no kernel for a LayerNorm layer of width 1025" in msg
    for code in (17, 37, 45, 47, 53, 54, 55, 61, 63, 69):               # between and behind the layer codes: no activation, no layer
        d = _model(_issue_chain()).to_desc()
        d.net_activation[1] = code
        rc, msg, _ = _create(d)
        assert rc == L.EH_EUNSUPPORTED and f"unknown activation id {code}".encode() in msg, (code, msg)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("B,n", [(1, 1), (1, 5), (7, 16), (64, 17)])
def test_the_twin_is_torchs_layer_norm(B, n, affine):
    g = torch.Generator().manual_seed(B * 100 + n)
    x = (3.0 + 2.0 * torch.randn(B, n, generator=g, dtype=torch.float64)).requires_grad_(True)
    w = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True) if affine else None
    b = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True) if affine else None
    eps = 1e-5
    y = tw.layer_norm(x, w, b, eps)
    ref = torch.nn.functional.layer_norm(x, (n,), w, b, eps)
    assert torch.allclose(y, ref, rtol=1e-12, atol=1e-12)
    c = torch.randn(B, n, generator=g, dtype=torch.float64)
    leaves = [x] + ([w, b] if affine else [])
    for a, r in zip(torch.autograd.grad((y * c).sum(), leaves), torch.autograd.grad((ref * c).sum(), leaves)):
        assert torch.allclose(a, r, rtol=1e-9, atol=1e-12)
    if n == 1:                                                          # zero variance: xh = 0, y = bias, nothing flows into x
        assert torch.equal(y, b.expand(B, 1) if affine else torch.zeros(B, 1, dtype=torch.float64))
        assert torch.equal(torch.autograd.grad((tw.layer_norm(x, w, b, eps) * c).sum(), [x])[0], torch.zeros(B, 1, dtype=torch.float64))


def test_twin_gradient_against_central_differences():
    m = _model(eh.Chain(eh.LayerNorm(5, "tanh"), eh.Dense(5, 4, "sigmoid"), eh.LayerNorm(4, affine=False)), P=2, input_batchnorm=True, scale_nn_outputs=True)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((2, 20)); ta = 10 + 5 * rng.standard_normal(20); y = 3 + rng.standard_normal(20)
    y[3] = np.nan
    th = m.initialparameters(2).astype(np.float64) + 0.1 * rng.standard_normal(m.n_theta)
    rows = np.arange(20)
    _, g, nv = tw.loss_and_grad(m, th, X, {"ta": ta}, y, rows)
    assert nv == 19
    for i in rng.choice(m.n_theta, 12, replace=False):
        e = np.zeros(m.n_theta); e[i] = 1e-6
        fd = (tw.loss_and_grad(m, th + e, X, {"ta": ta}, y, rows)[0] - tw.loss_and_grad(m, th - e, X, {"ta": ta}, y, rows)[0]) / 2e-6
        assert fd == pytest.approx(g[i], rel=1e-5, abs=1e-8)
    # no state: the test-mode forward is the train-mode one
    m1 = _model(eh.Chain(eh.LayerNorm(5, "swish"), eh.Dense(5, 5, "tanh")), P=2)
    th1 = m1.initialparameters(1)
    yt = tw.forward(m1, th1, X, {"ta": ta}, rows, train=True)[0]
    ye = tw.forward(m1, th1, X, {"ta": ta}, rows, train=False)[0]
    assert torch.equal(yt, ye) and np.array_equal(tw.predict(m1, th1, X, {"ta": ta}, rows)[0], yt.detach().numpy())
