"""BatchNorm layers inside hidden-layer chains, without a GPU: chain parsing, parameter tree, masks and descriptor, what the constructor,
train() and eh_create refuse before a device is touched, and the twin of tests/bn_chain_twin.py against torch's own batch_norm."""
import ctypes as C

import numpy as np
import pytest
import torch

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L

from tests import bn_chain_twin as tw

RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}


def _model(hl, P=3, act="tanh", **kw):
    return eh.constructHybridModel([f"x{i}" for i in range(P)], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=hl, activation=act, **kw)


def _issue_chain():
    return eh.Chain(eh.Dense(16, 16, "tanh"), eh.BatchNorm(16), eh.Dense(16, 8, "relu"), eh.BatchNorm(8, "sigmoid"))


def test_chain_parsing_and_widths_from_batchnorm_dims():
    m = _model(_issue_chain())
    # Dense(P, 16, tanh) in front (first_h from the chain), then the four layers, then Dense(8, 1)
    assert m.hidden_layers == [16, 16, 16, 8, 8]
    assert m.layer_activations == ["tanh", "tanh", "bn:identity", "relu", "bn:sigmoid"]
    assert m.NN == [(16, 3), (16, 16), (16, 16), (8, 16), (8, 8), (1, 8)] and m.bn_layers == [2, 4]
    assert m.batchnorm == {2: (0.1, 1e-5), 4: (0.1, 1e-5)}
    # a chain may begin or end with one: first_h / last_h come from its dims (NNModels.jl:156-169)
    m = _model(eh.Chain(eh.BatchNorm(16), eh.Dense(16, 12, "tanh")))
    assert m.hidden_layers == [16, 16, 12] and m.bn_layers == [1] and m.NN[0] == (16, 3) and m.NN[-1] == (1, 12)
    m = _model(eh.Chain(eh.Dense(5, 7, "relu"), eh.BatchNorm(7, "swish", affine=False, momentum=0.3, epsilon=1e-3)))
    assert m.hidden_layers == [5, 7, 7] and m.layer_activations[-1] == "bn0:swish" and m.NN[-1] == (1, 7) and m.batchnorm == {2: (0.3, 1e-3)}
    assert repr(eh.BatchNorm(16)) == "BatchNorm(16)" and repr(eh.BatchNorm(8, "sigmoid")) == "BatchNorm(8, sigmoid)"
    assert repr(eh.BatchNorm(8, affine=False)) == "BatchNorm(8, affine=false)"
    with pytest.raises(ValueError, match=r"BatchNorm\(9\), the layer in front of it gives 16"):
        _model(eh.Chain(eh.Dense(16, 16), eh.BatchNorm(9)))
    with pytest.raises(ValueError, match="takes 4 inputs"):
        _model(eh.Chain(eh.BatchNorm(16), eh.Dense(4, 4)))


def test_theta_layout_initial_values_and_unpack_round_trip():
    m = _model(_issue_chain())
    names = [(li, name, shape) for _, li, name, shape in m.leaves()]
    assert names == [(0, "weight", (16, 3)), (0, "bias", (16,)), (1, "weight", (16, 16)), (1, "bias", (16,)), (2, "scale", (16,)), (2, "bias", (16,)),
                     (3, "weight", (8, 16)), (3, "bias", (8,)), (4, "scale", (8,)), (4, "bias", (8,)), (5, "weight", (1, 8)), (5, "bias", (1,))]
    assert m.n_nn == 64 + 272 + 32 + 136 + 16 + 9 and m.n_theta == m.n_nn + 1
    th = m.initialparameters(0)
    assert th.shape == (m.n_theta,) and th.dtype == np.float32
    layers, glob = m.unpack(th)
    assert len(layers) == 6 and isinstance(layers[2], dict) and isinstance(layers[0], tuple)
    assert np.array_equal(layers[2]["scale"], np.ones(16)) and np.array_equal(layers[2]["bias"], np.zeros(16))
    assert np.array_equal(layers[4]["scale"], np.ones(8)) and np.array_equal(layers[4]["bias"], np.zeros(8))
    assert layers[3][0].shape == (8, 16) and layers[3][1].shape == (8,) and list(glob) == ["Q10"]
    # round trip: the leaves in order, matrices column-major, are theta again
    flat = []
    for l in layers:
        flat += [l["scale"], l["bias"]] if isinstance(l, dict) and l else ([] if isinstance(l, dict) else [l[0].flatten(order="F"), l[1]])
    assert np.array_equal(np.concatenate(flat + [glob["Q10"]]), th)
    # the twin reads the same layout
    tl, tg = tw.unpack(m, torch.tensor(th))
    assert np.array_equal(tl[3]["weight"].numpy(), layers[3][0]) and np.array_equal(tl[4]["scale"].numpy(), layers[4]["scale"]) and tg.numel() == 1
    assert m.opt_branches() == {"ps": (0, m.n_nn), "Q10": (m.n_nn, m.n_nn + 1)}
    # affine = false adds no leaf
    m0 = _model(eh.Chain(eh.Dense(16, 16), eh.BatchNorm(16, affine=False)))
    assert [n for _, _, n, _ in m0.leaves()] == ["weight", "bias"] * 3 and m0.unpack(m0.initialparameters(1))[0][2] == {}


def test_weight_l2_leaves_batchnorm_out():
    """the reference's own test (test/test_extract_weights.jl:10-14): weight_l2 over a chain with BatchNorm = the manual sum over the Dense matrices"""
    m = _model(_issue_chain())
    th = np.random.default_rng(3).standard_normal(m.n_theta).astype(np.float32)
    layers, _ = m.unpack(th)
    manual = sum(float((l[0].astype(np.float64) ** 2).sum()) for l in layers if isinstance(l, tuple))
    mw, mb = m.l2_mask(None, "weight"), m.l2_mask(None, "bias")
    assert mw.sum() == 48 + 256 + 128 + 8 and mb.sum() == 16 + 16 + 8 + 1
    assert float((th[mw].astype(np.float64) ** 2).sum()) == pytest.approx(manual, rel=1e-12)
    assert tw.weight_l2(m, th) == pytest.approx(manual, rel=1e-12)
    off = {(li, n): None for _, li, n, _ in m.leaves()}
    o = 0
    for _, li, n, shape in m.leaves():
        off[(li, n)] = (o, o + int(np.prod(shape)))
        o += int(np.prod(shape))
    for li in m.bn_layers:
        for leaf in ("scale", "bias"):
            lo, hi = off[(li, leaf)]
            assert not mw[lo:hi].any() and not mb[lo:hi].any() and not m.weight_mask()[lo:hi].any()
    c = m.l2_coefficients([eh.WeightL2(0.5, normalize=True)])
    assert np.count_nonzero(c) == mw.sum() and c[mw][0] == pytest.approx(0.5 / mw.sum())


def test_descriptor_codes_and_size():
    m = _model(eh.Chain(eh.Dense(16, 16, "tanh"), eh.BatchNorm(16), eh.Dense(16, 8, "relu"), eh.BatchNorm(8, "sigmoid", affine=False)), input_batchnorm=True)
    d = m.to_desc()
    plain = _model([16, 16]).to_desc()
    assert d.struct_size == plain.struct_size == C.sizeof(L.ModelDesc)
    assert d.n_hidden == 5 and list(d.hidden)[:5] == [16, 16, 16, 8, 8] and d.n_nets == 0 and d.activation == L.EH_ACT_PER_NET and d.input_batchnorm == 1
    assert list(d.net_activation)[:5] == [0, 0, L.EH_LAYER_BATCHNORM + 4, 2, L.EH_LAYER_BATCHNORM + L.EH_LAYER_BN_NOAFFINE + 1]
    assert L.EH_LAYER_BATCHNORM == 40 and L.EH_LAYER_BATCHNORM + L.EH_LAYER_BN_NOAFFINE + 4 == 52
    # a BatchNorm layer counts towards the eight hidden layers
    with pytest.raises(NotImplementedError, match="hidden layers"):
        _model(eh.Chain(*([eh.Dense(8, 8), eh.BatchNorm(8)] * 4))).to_desc()
    assert _model(eh.Chain(*([eh.Dense(8, 8), eh.BatchNorm(8)] * 3 + [eh.Dense(8, 8)]))).to_desc().n_hidden == 8


def test_refusals_of_the_constructor_and_of_train():
    with pytest.raises(NotImplementedError, match="BatchNorm layers in a MultiNN model"):
        eh.constructHybridModel({"rb": ["a"], "Q10": ["b"]}, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), [], hidden_layers=eh.Chain(eh.Dense(8, 8), eh.BatchNorm(8)))
    with pytest.raises(NotImplementedError, match="BatchNorm layer next to a Dropout"):
        _model(eh.Chain(eh.Dense(8, 8), eh.Dropout(0.1), eh.BatchNorm(8)))
    with pytest.raises(NotImplementedError, match="BatchNorm layer next to a Recurrence"):
        _model(eh.Chain(eh.BatchNorm(8), eh.Recurrence(eh.LSTMCell(8, 8))))
    with pytest.raises(NotImplementedError, match="track_stats = false"):
        eh.BatchNorm(8, track_stats=False)
    with pytest.raises(NotImplementedError, match="precision = 'bf16' with BatchNorm layers"):
        _model(eh.Chain(eh.Dense(8, 8), eh.BatchNorm(8)), precision="bf16")
    with pytest.raises(NotImplementedError, match="no device implementation"):
        eh.BatchNorm(8, "gelu")
    with pytest.raises(ValueError, match="momentum"):
        eh.BatchNorm(8, momentum=1.5)
    m = _model(eh.Chain(eh.Dense(8, 8), eh.BatchNorm(8)), P=2)
    cols = eh.synthetic.make_synth_rbq10(64, 1, 0.0)
    cols = {"x0": cols["sw_pot"], "x1": cols["dsw_pot"], "ta": cols["ta"], "reco": cols["reco"]}
    with pytest.raises(NotImplementedError, match=r"LBFGS\(\)\): BatchNorm layers in hidden_layers"):
        eh.train(m, cols, opt=eh.LBFGS(), nepochs=1)
    with pytest.raises(NotImplementedError, match=r"distributed=True\): BatchNorm layers in hidden_layers"):
        eh.train(m, cols, distributed=True, nepochs=1)


def _create(d):
    lib, h = L.lib(), C.c_void_p()
    rc = lib.eh_create(C.byref(d), C.byref(h))
    msg = lib.eh_last_error(None)
    if rc == L.EH_OK:
        assert h.value and lib.eh_destroy(h) == L.EH_OK
    return rc, msg, h


def test_eh_create_before_a_device_is_touched():
    chains = [_issue_chain(), eh.Chain(eh.BatchNorm(16), eh.Dense(16, 16, "tanh")), eh.Chain(eh.Dense(5, 130), eh.BatchNorm(130, "swish", affine=False))]
    for hl in chains:
        for bn in (False, True):
            rc, msg, h = _create(_model(hl, input_batchnorm=bn).to_desc())      # well formed: the constructor gets as far as the device
            assert rc == L.EH_OK or (rc == L.EH_EHIP and b"no HIP device" in msg and not h.value), msg
    d = _model(_issue_chain()).to_desc()
    d.hidden[2] = 12                                                   # a BatchNorm of another width than the layer in front of it
    rc, msg, h = _create(d)
    assert rc == L.EH_EINVAL and b"BatchNorm layer 2 has width 12, the layer in front of it 16" in msg and not h.value
    d = _model(_issue_chain()).to_desc()
    d.net_activation[0] = L.EH_LAYER_BATCHNORM
    rc, msg, _ = _create(d)
    assert rc == L.EH_EINVAL and b"EH_LAYER_BATCHNORM at hidden layer 0" in msg
    d = _model(_issue_chain()).to_desc()
    d.n_nets = 1; d.net_n_predictors[0] = 3; d.net_activation[0] = L.EH_LAYER_BATCHNORM + 4
    rc, msg, _ = _create(d)
    assert rc == L.EH_EUNSUPPORTED and b"no kernel for BatchNorm layers in a MultiNN model" in msg
    d = _model(_issue_chain()).to_desc()
    d.net_activation[1] = L.EH_LAYER_LSTM
    rc, msg, _ = _create(d)
    assert rc == L.EH_EUNSUPPORTED and b"both a BatchNorm layer and a recurrent layer" in msg
    for code in (37, 45, 47, 53):                                       # between and behind the layer codes: no activation, no layer
        d = _model(_issue_chain()).to_desc()
        d.net_activation[1] = code
        rc, msg, _ = _create(d)
        assert rc == L.EH_EUNSUPPORTED and f"unknown activation id {code}".encode() in msg


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("B,n", [(1, 5), (7, 16), (64, 17)])
def test_the_twin_is_torchs_batch_norm(B, n, affine):
    g = torch.Generator().manual_seed(B * 100 + n)
    x = (3.0 + 2.0 * torch.randn(B, n, generator=g, dtype=torch.float64)).requires_grad_(True)
    w = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True) if affine else None
    b = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True) if affine else None
    eps, mom = 1e-5, 0.1
    y, (mu, var) = tw.batch_norm(x, w, b, eps)
    rm, rv = torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
    if B > 1:                                                           # (torch refuses one value per channel in training; Lux does not)
        ref = torch.nn.functional.batch_norm(x, rm, rv, w, b, training=True, momentum=mom, eps=eps)
        assert torch.allclose(y, ref, rtol=1e-12, atol=1e-12)
        c = torch.randn(B, n, generator=g, dtype=torch.float64)
        leaves = [x] + ([w, b] if affine else [])
        for a, r in zip(torch.autograd.grad((y * c).sum(), leaves), torch.autograd.grad((ref * c).sum(), leaves)):
            assert torch.allclose(a, r, rtol=1e-9, atol=1e-12)
    else:
        assert torch.equal(var, torch.zeros(n, dtype=torch.float64)) and torch.allclose(y, b if affine else torch.zeros(n, dtype=torch.float64))

    class M:      # what update_state reads of a model
        batchnorm = {1: (mom, eps)}
    new = tw.update_state(M, {"in": None, 1: (np.zeros(n), np.ones(n))}, {1: (mu, var)}, B)
    if B > 1:
        assert np.allclose(new[1][0], rm.numpy(), rtol=1e-12) and np.allclose(new[1][1], rv.numpy(), rtol=1e-12)      # torch moved its buffers in place
    else:
        assert np.allclose(new[1][1], 0.9)
    # test mode
    yt, _ = tw.batch_norm(x.detach(), w, b, eps, running=new[1])
    ref = torch.nn.functional.batch_norm(x.detach(), torch.tensor(new[1][0]), torch.tensor(new[1][1]), w, b, training=False, eps=eps)
    assert torch.allclose(yt, ref, rtol=1e-12, atol=1e-12)


def test_twin_gradient_against_central_differences():
    m = _model(eh.Chain(eh.BatchNorm(5, "tanh"), eh.Dense(5, 4, "sigmoid"), eh.BatchNorm(4, affine=False)), P=2, input_batchnorm=True, scale_nn_outputs=True)
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
