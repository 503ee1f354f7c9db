"""Ensembles, the part that needs no GPU: the C entry points as the header declares them, the front door's fold -> row-list logic
against train()'s own split, the validation of member dicts, and every refusal train_members gives before it touches a device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from easyhybrid_jl_amd import _lib as L
from tests import closures as cl

T = importlib.import_module("easyhybrid_jl_amd.train")          # (the package's attribute `train` is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}
CTYPE = {"eh_handle*": C.c_void_p, "eh_ensemble*": C.c_void_p, "eh_ensemble**": C.POINTER(C.c_void_p), "int32_t": C.c_int32, "int64_t": C.c_int64,
         "float": C.c_float, "float*": C.POINTER(C.c_float), "const float*": C.POINTER(C.c_float), "const int32_t*": C.POINTER(C.c_int32),
         "const uint64_t*": C.POINTER(C.c_uint64), "const uint8_t*": C.POINTER(C.c_uint8), "int64_t*": C.POINTER(C.c_int64),
         "eh_target_metrics*": C.POINTER(L.TargetMetrics)}
ENTRIES = ["eh_ens_create", "eh_ens_destroy", "eh_ens_set_params", "eh_ens_get_params", "eh_ens_set_opt", "eh_ens_get_opt_state", "eh_ens_set_opt_state",
           "eh_ens_get_bn_state", "eh_ens_set_bn_state", "eh_ens_set_rows", "eh_ens_train_epoch", "eh_ens_eval", "eh_ens_load", "eh_ens_store"]


def _model(**kw):
    args = dict(hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    args.update(kw)
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, PARAMS, ["rb"], ["Q10"], **args)


def _table(n=50, seed=0):
    rng = np.random.default_rng(seed)
    return {"sw_pot": rng.random(n, np.float32), "dsw_pot": rng.random(n, np.float32), "ta": (10 + 10 * rng.random(n)).astype(np.float32),
            "reco": (1 + rng.random(n)).astype(np.float32)}


def test_entry_points_exist_with_the_headers_signatures():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "easyhybrid_hip.h")).read(), flags=re.S)
    lib = L.lib()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"int32_t\s+(eh_ens_[a-z_]+)\s*\(([^)]*)\)\s*;", txt)}
    assert sorted(decl) == sorted(ENTRIES)
    for name, params in decl.items():
        want = []
        for p in params.split(","):
            typ = re.sub(r"\s*\b[a-z_0-9]+\s*$", "", p.strip())           # drop the parameter's name
            want.append(CTYPE[re.sub(r"\s*\*", "*", typ)])
        fn = getattr(lib, name)                                          # (AttributeError: declared, not exported)
        res, args = L.SIGNATURES[name]
        assert res is C.c_int32 and fn.restype is C.c_int32
        assert len(args) == len(want), name
        for i, (a, w) in enumerate(zip(args, want)):
            assert a is w or (a is C.c_void_p and w is C.c_void_p), (name, i, a, w)
    assert re.search(r"#define\s+EH_ENS_MAX_MEMBERS\s+4096\b", txt) and L.EH_ENS_MAX_MEMBERS == 4096
    assert lib.eh_version() == 4                                         # added without a new ABI version
    assert lib.eh_ens_destroy(None) == L.EH_OK
    out = C.c_void_p()
    assert lib.eh_ens_create(None, 2, 64, C.byref(out)) == L.EH_EINVAL and lib.eh_ens_eval(None, 0, None) == L.EH_EINVAL


def test_fold_row_lists_are_train_s_own_split():
    """k = 3 on 50 rows, one fold without a single valid target: a member's two row lists pick, from the one screened table, exactly the
    rows split_data gathers for train(..., folds =, val_fold = v) -- the same rows in the same order."""
    model = _model()
    cols = _table(50)
    folds = np.arange(50) % 3
    y = cols["reco"].copy()
    y[folds == 2] = np.nan
    y[[0, 7]] = np.nan
    X = np.stack([cols["sw_pot"], cols["dsw_pot"]])
    data = ((X, {"ta": cols["ta"]}), {"reco": y})                      # a prepared table: no row is screened out, the empty fold stays
    for v in range(3):
        dc = T.DataConfig(folds=folds, val_fold=v)
        tr, va = T._member_rows(model, data, dc, np.random.default_rng(0))
        assert tr.dtype == np.int32 and va.dtype == np.int32
        ((xtr, ftr), ytr), ((xva, fva), yva) = T.split_data(data, model, dc, np.random.default_rng(0))
        assert np.array_equal(X[:, tr], xtr) and np.array_equal(X[:, va], xva)
        assert np.array_equal(cols["ta"][tr], ftr["ta"]) and np.array_equal(cols["ta"][va], fva["ta"])
        assert np.array_equal(y[tr], ytr["reco"], equal_nan=True) and np.array_equal(y[va], yva["reco"], equal_nan=True)
        assert len(tr) + len(va) == 50 and np.array_equal(np.sort(va), np.flatnonzero(folds == v))
    assert np.all(np.isnan(y[T._member_rows(model, data, T.DataConfig(folds=folds, val_fold=2), None)[1]]))
    # a table of columns: rows without a target are screened out first (prepare_data), folds has one entry per row that is kept
    cols2 = dict(cols, reco=np.where(np.arange(50) % 10 == 0, np.nan, cols["reco"]).astype(np.float32))
    kept = np.flatnonzero(~np.isnan(cols2["reco"]))
    f2 = np.arange(len(kept)) % 3
    dc = T.DataConfig(folds=f2, val_fold=1)
    tr, va = T._member_rows(model, cols2, dc, None)
    ((xtr, _), _), ((xva, _), yva) = T.split_data(cols2, model, dc)
    (Xs, _), ys = T.prepare_data(model, cols2)
    assert np.array_equal(Xs[:, tr], xtr) and np.array_equal(Xs[:, va], xva) and np.array_equal(ys["reco"][va], yva["reco"])
    # no folds: the common contiguous split, shuffled or not, as train() draws it
    for sh in (False, True):
        dc = T.DataConfig(shuffleobs=sh, split_data_at=0.7)
        tr, va = T._member_rows(model, cols, dc, np.random.default_rng(3))
        ((xtr, _), _), ((xva, _), _) = T.split_data(cols, model, dc, np.random.default_rng(3))
        assert np.array_equal(X[:, tr], xtr) and np.array_equal(X[:, va], xva) and len(tr) == 35


def test_member_dicts_are_validated():
    model, cols = _model(), _table()
    with pytest.raises(ValueError, match="unknown key"):
        eh.train_members(model, cols, [{"val_fold": 0, "batchsize": 32}], folds=np.arange(50) % 2)
    with pytest.raises(ValueError, match="mix optimiser rules"):
        eh.train_members(model, cols, [{"opt": eh.Adam(0.01)}, {"opt": eh.RMSProp(0.01)}])
    with pytest.raises(ValueError, match="mix optimiser rules"):
        eh.train_members(model, cols, [{}, {"opt": eh.Descent(0.1)}])                      # (the common opt is Adam)
    with pytest.raises(ValueError, match="non-empty list"):
        eh.train_members(model, cols, [])
    with pytest.raises(ValueError, match="not a dict"):
        eh.train_members(model, cols, [3])
    with pytest.raises(TypeError, match="unknown keyword"):
        eh.train_members(model, cols, [{}], nepoch=3)
    cfgs = T._member_configs(T.TrainConfig(opt=eh.Adam(0.01), random_seed=7), T.DataConfig(folds=np.arange(50) % 2),
                             [{"val_fold": 1}, {"random_seed": 9, "opt": eh.Adam(0.002)}])
    assert (cfgs[0][1].val_fold, cfgs[0][0].random_seed, cfgs[0][0].opt.eta) == (1, 7, 0.01)
    assert (cfgs[1][1].val_fold, cfgs[1][0].random_seed, cfgs[1][0].opt.eta) == (None, 9, 0.002)


def _refusals():
    folds = np.arange(50) % 2
    m = [{"val_fold": 0}, {"val_fold": 1}]
    seq = _model(hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(2, 8))))
    closure = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], cl.rbq10_closure, dict(cl.RBQ10_TABLE), ["rb"], ["Q10"], hidden_layers=[16, 16])
    drop = _model(hidden_layers=eh.Chain(eh.Dense(16, 16, "tanh"), eh.Dropout(0.2)))
    bnl = _model(hidden_layers=eh.Chain(eh.Dense(16, 16, "tanh"), eh.BatchNorm(16)))
    return [
        ("distributed", _model(), m, dict(folds=folds, distributed=True), "distributed training"),
        ("LBFGS", _model(), m, dict(folds=folds, opt=eh.LBFGS()), "LBFGS"),
        ("LBFGS of one member", _model(), [{"opt": eh.LBFGS()}], {}, "LBFGS"),
        ("OptimiserChain", _model(), m, dict(folds=folds, opt=eh.OptimiserChain(eh.ClipNorm(1.0), eh.Adam(0.01))), "OptimiserChain"),
        ("per-branch opt", _model(), m, dict(folds=folds, opt={"rb": eh.Adam(0.01)}), "per-branch opt"),
        ("sequence model", seq, m, dict(folds=folds), "sequence models"),
        ("sequence_kwargs", _model(), m, dict(folds=folds, sequence_kwargs=dict(input_window=4)), "sequence models"),
        ("extra_loss", _model(), m, dict(folds=folds, extra_loss=eh.WeightL2(1e-3)), "extra_loss"),
        ("recorded loss", _model(), m, dict(folds=folds, training_loss=lambda yh, y: np.mean((yh - y) ** 2)), "recorded losses"),
        ("per-target losses", _model(), m, dict(folds=folds, training_loss=eh.PerTarget(("mse",))), "recorded losses"),
        ("closure", closure, m, dict(folds=folds), "recorded mechanistic closure"),
        ("dropout", drop, m, dict(folds=folds), "Dropout layers"),
        ("BatchNorm layer", bnl, m, dict(folds=folds), "layer-wise form"),
        ("pearsonLoss", _model(), m, dict(folds=folds, training_loss="pearsonLoss"), "two-pass losses"),
        ("kgeLoss", _model(), m, dict(folds=folds, training_loss="kgeLoss"), "two-pass losses"),
        ("pbkgeLoss", _model(), m, dict(folds=folds, training_loss="pbkgeLoss"), "two-pass losses"),
        ("precision bf16", _model(precision="bf16"), m, dict(folds=folds), "row-split bf16 kernels"),
        ("precision bf16_fwd", _model(precision="bf16_fwd"), m, dict(folds=folds), "row-split bf16 kernels"),
        ("per-layer activations", _model(hidden_layers=eh.Chain(eh.Dense(16, 32, "relu"), eh.Dense(32, 8, "sigmoid"))), m, dict(folds=folds), "per-net or per-layer activations"),
        ("per-net activations", eh.constructHybridModel({"rb": ["sw_pot"], "Q10": ["dsw_pot"]}, ["ta"], ["reco"], eh.RbQ10, PARAMS, [], hidden_layers={"rb": [16], "Q10": [8]},
                                                          activation={"rb": "tanh", "Q10": "sigmoid"}), m, dict(folds=folds), "per-net or per-layer activations"),
        ("specialize", _model(), m, dict(folds=folds, specialize=True), "compiled at run time"),
        ("fused_update off", _model(), m, dict(folds=folds, fused_update=False), "step \\+ reduce pair"),
        ("train_from", _model(), m, dict(folds=folds, train_from=(np.zeros(338, np.float32),)), "train_from"),
    ]


@pytest.mark.parametrize("case", range(23))
def test_up_front_refusals_name_their_cause(case):
    name, model, members, kw, why = _refusals()[case]
    with pytest.raises(NotImplementedError, match=why):
        eh.train_members(model, _table(), members, nepochs=1, **kw)


def test_several_targets_are_refused_up_front():
    flux = eh.constructHybridModel([f"x{i}" for i in range(6)], ["SW_IN", "TA"], ["NEE", "GPP"], eh.FluxPartModelQ10,
                                   {"RUE": (0.1, 0.0, 1.0), "Rb": (1.0, 0.0, 6.0), "Q10": (1.5, 1.0, 4.0)}, ["RUE", "Rb"], ["Q10"],
                                   hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    with pytest.raises(NotImplementedError, match="several targets"):
        eh.train_members(flux, {}, [{}])


def test_train_folds_is_the_tutorial_s_loop():
    seen = {}
    orig = T.train_members
    try:
        T.train_members = lambda model, data, members, **kw: seen.update(members=members, kw=kw) or "results"
        folds = np.array([2, 0, 1, 2, 0, 1, 1])
        assert T.train_folds("model", "data", folds, nepochs=3) == "results"
        assert seen["members"] == [{"val_fold": 0}, {"val_fold": 1}, {"val_fold": 2}] and seen["kw"]["nepochs"] == 3 and seen["kw"]["folds"] is folds
        T.train_folds("model", {"fold": np.array([1, 1, 5])}, "fold")
        assert seen["members"] == [{"val_fold": 1}, {"val_fold": 5}] and seen["kw"]["folds"] == "fold"
    finally:
        T.train_members = orig
