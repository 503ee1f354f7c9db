"""Ensembles on the device (eh_ens_*, HybridEngine.ensemble, train_members / train_folds): every member of an ensemble launch is held
BIT FOR BIT to what an ordinary engine of the same library computes for it.

The reference of member j is an ordinary engine whose training split holds the member's rows, uploaded in the member's row order, with the
same theta_0, rule and numbers, `fused_update` 1, `multi_step` 1 and `aot_spec` as the ensemble's engine, driven by
train_epoch(B, seed_j, shuffle).  Equality means np.array_equal on the uint32 views of theta, m, v and the beta products.  Neither entry
point hands out the per-step losses, only their mean over the epoch (the float32 values summed in the same order in double, rounded to
float32), which is compared on its bits: a WEAKER check than step-by-step equality -- one ulp in one of several steps can vanish in the
rounding of the mean.  It is exact where an epoch is ONE step: the 64-row member of test_three_members_ragged_and_unequal (three epochs)
and all 300 members of test_more_members_than_compute_units.  The evaluation metrics are held to the end-to-end bars of
tests/test_gpu_eval.py (E2E_REL / E2E_ABS): the two sides reduce the same predictions about different metric shifts."""
import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from oracle import hybrid_oracle as ho
from tests import util

pytestmark = pytest.mark.gpu
E2E_REL, E2E_ABS = 2e-5, 2e-6          # tests/test_gpu_eval.py: metrics end to end
AOT = [pytest.param(0, id="generic"), pytest.param(1, id="specialised ahead of time")]


def _take(X, f, y, rows):
    return X[:, rows], {k: v[rows] for k, v in f.items()}, {k: v[rows] for k, v in y.items()}


def _engine(spec, theta, X, f, y, aot=0, rows=None):
    if rows is not None:
        X, f, y = _take(X, f, y, rows)
    eng = util.load_engine(spec, theta, X, f, y)
    eng.set_option("aot_spec", aot); eng.set_option("fused_update", 1); eng.set_option("multi_step", 1)
    return eng


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _state(obj, j=None):
    """theta, m, v, beta products (and the running statistics of an input BatchNorm) of an engine, or of member j of an ensemble"""
    eng = obj if j is None else obj.engine
    args = () if j is None else (j,)
    out = [obj.get_params(*args), *obj.get_opt_state(*args)]
    if eng.desc.input_batchnorm:
        out += list(obj.get_bn_state(*args))
    return [_bits(a) for a in out]


def _assert_same(ens, j, ref, what=""):
    for name, a, b in zip(("theta", "m", "v", "beta products", "running mean", "running var"), _state(ens, j), _state(ref)):
        assert np.array_equal(a, b), (what, "member", j, name, int(np.count_nonzero(a != b)), "words differ")


def _same_loss(a, b):
    return (np.isnan(a) and np.isnan(b)) or _bits([a])[0] == _bits([b])[0]


OPTS = [("Adam", dict(lr=0.01)), ("Adam", dict(lr=0.003)), ("RMSProp", dict(lr=0.002, beta1=0.9))]


def _ensemble_and_refs(spec, X, f, y, rows, B, aot, opts=None, theta_seed=10):
    """an engine over the whole table with an ensemble of len(rows) members on it, and the members' reference engines (None: no rows)"""
    opts = opts or [OPTS[j % 3] for j in range(len(rows))]
    thetas = [ho.init_theta(spec, theta_seed + j, np.float32) for j in range(len(rows))]
    eng = _engine(spec, thetas[0], X, f, y, aot)
    ens = eng.ensemble(len(rows), B)
    refs = []
    for j, r in enumerate(rows):
        ens.set_params(j, thetas[j]); ens.set_opt(j, opts[j][0], **opts[j][1]); ens.set_rows(j, 0, r); ens.set_rows(j, 1, r)
        ref = None
        if len(r):
            ref = _engine(spec, thetas[j], X, f, y, aot, r)
            ref.opt_init(opts[j][0], **opts[j][1])
        refs.append(ref)
    return eng, ens, refs


def _epoch(ens, refs, B, seeds, shuffle, what, active=None):
    loss, steps = ens.train_epoch(seeds, shuffle=shuffle, active=active)
    for j, ref in enumerate(refs):
        if ref is None or (active is not None and not active[j]):
            continue
        l_ref, n_ref = ref.train_epoch(B, seed=seeds[j], shuffle=shuffle)
        assert steps[j] == n_ref and _same_loss(loss[j], l_ref), (what, j, steps[j], n_ref, loss[j], l_ref)
        _assert_same(ens, j, ref, what)
    return loss, steps


@pytest.mark.parametrize("aot", AOT)
def test_three_members_ragged_and_unequal(aot):
    spec, _, X, f, y = util.rbq10_case(200, "tanh", True, 0.1, seed=5)
    rng = np.random.default_rng(0)
    rows = [np.arange(200), rng.permutation(200)[:136], np.arange(64) + 70]      # 3 x 64 + 8 | 2 x 64 + 8, scrambled | exactly one minibatch
    eng, ens, refs = _ensemble_and_refs(spec, X, f, y, rows, 64, aot)
    loss, steps = _epoch(ens, refs, 64, [11, 12, 13], True, "shuffled epoch 1")
    assert list(steps) == [4, 3, 1] and np.all(np.isfinite(loss))
    _epoch(ens, refs, 64, [21, 22, 23], True, "shuffled epoch 2")
    _epoch(ens, refs, 64, [0, 0, 0], False, "unshuffled epoch")
    th = [ens.get_params(j) for j in range(3)]
    assert not np.array_equal(th[0], th[1]) and not np.array_equal(th[1], th[2])
    nj, log = eng.jit_status()
    assert log.startswith("ahead-of-time") == bool(aot), log[:200]
    ens.close(); eng.close()


def test_chunking_and_idle_members():
    """B = 1: 300 steps are two launches for member 0; member 1 (10 steps) idles through the second, member 2 (no rows) through both.  An
    idle launch must not flip a member's parameter set: the second epoch catches that."""
    spec, _, X, f, y = util.rbq10_case(200, "tanh", True, 0.1, seed=5)
    rng = np.random.default_rng(1)
    rows = [rng.integers(0, 200, 300), rng.permutation(200)[:10], np.empty(0, np.int64)]
    eng, ens, refs = _ensemble_and_refs(spec, X, f, y, rows, 1, 0)
    before = _state(ens, 2)
    for ep in range(2):
        loss, steps = _epoch(ens, refs, 1, [5 + ep, 6 + ep, 7 + ep], True, f"epoch {ep + 1}")
        assert list(steps) == [300, 10, 0] and np.isnan(loss[2])
    assert all(np.array_equal(a, b) for a, b in zip(before, _state(ens, 2)))
    ens.close(); eng.close()


def test_all_nan_minibatch_inside_one_member_is_skipped():
    spec, _, X, f, y = util.rbq10_case(256, "tanh", True, 0.0, seed=6)
    y = {"reco": y["reco"].copy()}
    y["reco"][64:128] = np.nan
    rows = [np.arange(192), np.arange(128, 256), np.r_[np.arange(64), np.arange(128, 192)]]      # member 2: member 0 without the empty minibatch
    opts = [OPTS[0], OPTS[2], OPTS[0]]
    eng, ens, refs = _ensemble_and_refs(spec, X, f, y, rows, 64, 0, opts)
    ens.set_params(2, ens.get_params(0))
    refs[2].set_params(ens.get_params(0))
    loss, steps = _epoch(ens, refs, 64, [0, 0, 0], False, "unshuffled")
    assert list(steps) == [3, 2, 2]
    # the skipped step left nothing behind: theta, moments and the beta products are those of the two steps that had data
    assert all(np.array_equal(a, b) for a, b in zip(_state(ens, 0), _state(ens, 2)))
    assert _same_loss(loss[0], loss[2])
    ens.close(); eng.close()


def test_inactive_member_keeps_its_bits():
    spec, _, X, f, y = util.rbq10_case(200, "tanh", True, 0.1, seed=5)
    rows = [np.arange(200), np.arange(150), np.arange(50, 200)]
    eng, ens, refs = _ensemble_and_refs(spec, X, f, y, rows, 64, 0)
    before = _state(ens, 1)
    loss, steps = _epoch(ens, refs, 64, [1, 2, 3], True, "member 1 inactive", active=[1, 0, 1])
    assert list(steps) == [4, 0, 3] and np.isnan(loss[1])
    assert all(np.array_equal(a, b) for a, b in zip(before, _state(ens, 1)))
    _epoch(ens, refs, 64, [4, 5, 6], True, "all active")          # member 1's first epoch, the others' second
    ens.close(); eng.close()


def test_more_members_than_compute_units():
    spec, _, X, f, y = util.rbq10_case(128, "tanh", True, 0.1, seed=8)
    M = 300
    rows = [np.random.default_rng(100 + j).permutation(128)[:64] for j in range(M)]
    thetas = [ho.init_theta(spec, 200 + j, np.float32) for j in range(M)]
    eng = _engine(spec, thetas[0], X, f, y)
    ens = eng.ensemble(M, 64)
    for j in range(M):
        ens.set_params(j, thetas[j]); ens.set_opt(j, "Adam", lr=0.01 + 1e-5 * j); ens.set_rows(j, 0, rows[j])
    loss, steps = ens.train_epoch(list(range(M)), shuffle=True)
    assert np.all(steps == 1) and np.all(np.isfinite(loss))
    for j in (0, 255, 256, 299):
        ref = _engine(spec, thetas[j], X, f, y, 0, rows[j])
        ref.opt_init("Adam", lr=0.01 + 1e-5 * j)
        l_ref, _ = ref.train_epoch(64, seed=j, shuffle=True)
        assert _same_loss(loss[j], l_ref)
        _assert_same(ens, j, ref, "M = 300")
        ref.close()
    ens.close(); eng.close()


@pytest.mark.parametrize("aot", AOT)
def test_input_batchnorm(aot):
    spec = ho.rbq10_spec((16, 16), "tanh", True)                   # the rbq10_bn case of tests/test_gpu_parity.py: raw predictors
    spec.input_batchnorm = True
    X, f, y = ho.make_synth_rbq10(300, 5, 0.1)
    rows = [np.arange(300), np.arange(100, 300), np.random.default_rng(2).permutation(300)[:170]]
    eng, ens, refs = _ensemble_and_refs(spec, X, f, y, rows, 64, aot, theta_seed=3)
    _epoch(ens, refs, 64, [1, 2, 3], True, "epoch 1")
    _epoch(ens, refs, 64, [0, 0, 0], False, "epoch 2")
    rm = [ens.get_bn_state(j)[0] for j in range(3)]
    assert not np.array_equal(rm[0], rm[1]) and np.all(np.abs(rm[0]) > 0)
    ens.close(); eng.close()


def test_evaluation_and_predictions_of_a_loaded_member():
    spec, _, X, f, y = util.rbq10_case(500, "tanh", True, 0.1, seed=9)
    rng = np.random.default_rng(3)
    rows = [np.arange(500), rng.permutation(500)[:333], np.arange(64)]
    ev_rows = [np.arange(100, 500), np.arange(0, 500, 3), np.arange(17)]
    eng, ens, refs = _ensemble_and_refs(spec, X, f, y, rows, 64, 0)
    for j in range(3):
        ens.set_rows(j, 1, ev_rows[j])
    _epoch(ens, refs, 64, [1, 2, 3], True, "epoch")
    for which, rr in ((1, ev_rows), (0, rows)):
        got = ens.eval(which)
        for j in range(3):
            holder = _engine(spec, ens.get_params(j), X, f, y, 0, rr[j])
            want, pred = holder.eval(0, predictions=True)
            bad = util.metric_mismatches(got[j][0], want[0], E2E_REL, E2E_ABS)
            assert not bad, (which, j, bad)
            if which == 1:
                ens.load(j)
                mine = eng.forward(0)
                assert np.array_equal(_bits(mine["reco"][rr[j]]), _bits(pred["reco"]))
                assert np.array_equal(_bits(mine["parameters"]["rb"][rr[j]]), _bits(holder.forward(0)["parameters"]["rb"]))
            holder.close()
    ens.close(); eng.close()


def test_load_store_round_trip_and_continued_training():
    spec, _, X, f, y = util.rbq10_case(200, "tanh", True, 0.1, seed=5)
    rows = [np.arange(200), np.random.default_rng(4).permutation(200)[:128]]
    eng, ens, refs = _ensemble_and_refs(spec, X, f, y, rows, 64, 0)
    _epoch(ens, refs, 64, [1, 2], True, "epoch")
    for j in range(2):
        before = _state(ens, j)
        ens.load(j)
        assert all(np.array_equal(a, b) for a, b in zip(before, _state(eng)))      # the engine IS the member
        ens.store(j)
        assert all(np.array_equal(a, b) for a, b in zip(before, _state(ens, j)))
    ens.load(1)                                                   # ordinary steps on the engine continue member 1 as its reference continues
    for k in range(2):
        l_a = eng.train_step(64 * k, 64, idx=rows[1].astype(np.int32))
        l_b = refs[1].train_step(64 * k, 64)
        assert _same_loss(l_a, l_b)
    assert all(np.array_equal(a, b) for a, b in zip(_state(eng), _state(refs[1])))
    ens.store(1)
    _assert_same(ens, 1, refs[1], "stored back")
    _epoch(ens, refs, 64, [7, 8], True, "epoch after the steps")
    ens.close(); eng.close()


def test_live_handle_refusals():
    def handle(hidden=(16, 16), n=200, fused=True, model=None):
        spec, theta, X, f, y = util.rbq10_case(n, "tanh", True, 0.1, seed=5, hidden=hidden)
        if model is None:
            eng = util.load_engine(spec, theta, X, f, y)
        else:
            eng = model.engine()
            eng.set_data(0, X, [f["ta"]], [y["reco"]])
        if fused:
            eng.set_option("fused_update", 1)
        return eng
    for eng, batch, why in ((handle((128, 128), fused=False), 64, "row-split kernels"),
                            (handle((16, 16, 16, 16), fused=False), 64, "layer-wise form"),
                            (handle(n=5000), 4096, "4096 samples is more than one workgroup covers"),
                            (handle(fused=False), 64, "not in fused-update mode")):
        with pytest.raises(NotImplementedError, match=why):
            eng.ensemble(2, batch)
        eng.close()
    drop = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                   hidden_layers=eh.Chain(eh.Dense(16, 16, "tanh"), eh.Dropout(0.2)), activation="tanh", scale_nn_outputs=True)
    eng = handle(model=drop, fused=False)
    with pytest.raises(NotImplementedError, match="Dropout needs a step kernel compiled at run time"):
        eng.ensemble(2, 64)
    eng.close()
    eng = handle()
    with pytest.raises(ValueError, match="members"):
        eng.ensemble(0, 64)
    ens = eng.ensemble(2, 64)
    spec, theta, X, f, y = util.rbq10_case(200, "tanh", True, 0.1, seed=5)
    for call in (lambda: eng.set_data(0, X, [f["ta"]], [y["reco"]]), lambda: eng.set_option("multi_step", 0), lambda: eng.opt_init("Adam", 0.01)):
        with pytest.raises(eh.EngineError, match="carries an ensemble"):
            call()
    with pytest.raises(ValueError, match="outside"):
        ens.set_rows(0, 0, [0, 200])
    with pytest.raises(eh.EngineError, match="no optimiser"):
        ens.train_epoch()
    ens.close()
    eng.set_option("multi_step", 0)                               # free again
    eng.close()


def test_every_other_refusal_sentence_of_a_live_handle():
    """one case per sentence of eh_ens_create's refusal that test_live_handle_refusals does not reach, each matched on its own text; then the
    entry points that stay open on a handle with an ensemble and can move it out of what eh_ens_create checked"""
    from tests import closures as cl

    def handle(hidden=(16, 16), fused=True, bn=False, **spec_kw):
        spec, theta, X, f, y = util.rbq10_case(700, "tanh", True, 0.1, seed=5, hidden=hidden)
        for k, v in spec_kw.items():
            setattr(spec, k, v)
        spec.input_batchnorm = bn
        eng = util.load_engine(spec, theta, X, f, y)
        if fused:
            eng.set_option("fused_update", 1)
        return eng

    def refused(eng, why, batch=64):
        with pytest.raises(NotImplementedError, match=why):
            eng.ensemble(2, batch)

    eng = handle((128, 128), fused=False, precision="bf16_fwd"); refused(eng, "row-split bf16 kernels"); eng.close()
    eng = handle(fused=False); eng.set_training_loss("pearsonLoss"); refused(eng, "two-pass losses"); eng.close()
    eng = handle(fused=False); eng.set_training_loss(lambda yh, y: np.mean((yh - y) ** 2)); refused(eng, "A recorded loss runs on kernels compiled at run time"); eng.close()
    eng = handle(); eng.set_option("multi_step", 0); refused(eng, "multi_step option is off"); eng.close()
    eng = handle(); eng.profile_enable(1); refused(eng, "Profiling is enabled"); eng.close()
    eng = handle(); eng.set_option("specialize", 1); refused(eng, "kernels compiled at run time \\(option specialize\\)"); eng.close()
    eng = handle((32, 32)); refused(eng, "do not fit the LDS")          # (1186 parameters: 147 KB of state behind the work space); eng.close()
    eng = handle(bn=True); refused(eng, "Input BatchNorm takes its statistics inside the step kernel only", batch=600); eng.close()
    eng = handle(bn=True); eng.set_option("bn_in_kernel", 0); refused(eng, "Input BatchNorm takes its statistics inside the step kernel only"); eng.close()
    eng = handle(fused=False); eng.opt_init_chain([("clipgrad", 1.0), ("rule",)], rule="Adam", lr=0.01); refused(eng, "An OptimiserChain is installed"); eng.close()
    eng = handle(); eh.HybridEngine.comm_init_local([eng]); refused(eng, "Data parallelism is set up"); eng.comm_destroy(); eng.close()
    per_layer = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                        hidden_layers=eh.Chain(eh.Dense(16, 32, "relu"), eh.Dense(32, 8, "sigmoid")), activation="tanh", scale_nn_outputs=True)
    closure = eh.constructHybridModel(["x0", "x1"], ["ta"], ["reco"], cl.rbq10_closure, dict(cl.RBQ10_TABLE), ["rb"], ["Q10"], hidden_layers=[16, 16],
                                      activation="tanh", scale_nn_outputs=True)
    flux = eh.constructHybridModel([f"x{i}" for i in range(6)], ["SW_IN", "TA"], ["NEE", "GPP"], eh.FluxPartModelQ10,
                                   {"RUE": (0.1, 0.0, 1.0), "Rb": (1.0, 0.0, 6.0), "Q10": (1.5, 1.0, 4.0)}, ["RUE", "Rb"], ["Q10"],
                                   hidden_layers=[16, 16], activation="tanh", scale_nn_outputs=True)
    seq = eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(ho.RBQ10_PARAMS), ["rb"], ["Q10"],
                                  hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(2, 8))), activation="tanh", scale_nn_outputs=True)
    for model, why in ((per_layer, "Per-net or per-layer activations"), (closure, "A recorded mechanistic closure"), (flux, "Several targets"),
                       (seq, "Sequence models train on windows")):
        eng = model.engine()
        refused(eng, why)
        eng.close()
    # a capture in progress: the recorded sequence is six steps, one full rotation of the engine's state
    eng = handle(); eng.opt_init("Adam", 0.01)
    eng.train_step(0, 64, want_loss=False)
    eng.graph_begin()
    refused(eng, "A graph is being captured")
    for i in range(6):
        eng.train_step(64 * i, 64, want_loss=False)
    eng.graph_end()
    eng.synchronize()
    # ... and with an ensemble on the handle
    ens = eng.ensemble(2, 64)
    with pytest.raises(eh.EngineError, match="eh_graph_begin: the handle carries an ensemble"):
        eng.graph_begin()
    theta = ens.get_params(0)
    with pytest.raises(eh.EngineError, match="carries an ensemble"):
        eng.set_training_loss("pearsonLoss")                  # (an option: closed while an ensemble exists)
    eng.profile_enable(1)                                     # (not closed: every launch asks again)
    for call in (lambda: ens.train_epoch([1, 2]), lambda: ens.eval(0)):
        with pytest.raises(eh.EngineError, match="has left the configuration its ensemble was created in.*Profiling is enabled"):
            call()
    assert np.array_equal(_bits(theta), _bits(ens.get_params(0)))
    eng.profile_enable(0)
    loss, steps = ens.train_epoch([1, 2])
    assert list(steps) == [11, 11] and np.all(np.isfinite(loss))
    eng.close()                                               # closes its ensemble first
    assert not ens._e.value


# ---- the front door --------------------------------------------------------------------------------------------------------------
def _front_model():
    from easyhybrid_jl_amd.synthetic import RBQ10_PARAMS
    return eh.constructHybridModel(["sw_pot", "dsw_pot"], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10_PARAMS), ["rb"], ["Q10"], hidden_layers=[16, 16],
                                   activation="tanh", scale_nn_outputs=True)


def test_train_folds_front_door():
    from easyhybrid_jl_amd.synthetic import make_synth_rbq10
    from easyhybrid_jl_amd.train import prepare_data
    cols = make_synth_rbq10(600, seed=3)
    cols = dict(cols, sw_pot=cols["sw_pot"] / np.float32(50), dsw_pot=cols["dsw_pot"] / np.float32(50))
    model = _front_model()
    folds = np.arange(600) % 3
    kw = dict(nepochs=3, batchsize=64, random_seed=5, return_model="final", loss_types=["mse", "r2", "pearson"], distributed=False)
    res = eh.train_folds(model, cols, folds, **kw)
    again = eh.train_folds(model, cols, folds, **kw)
    assert len(res) == 3
    (X, forc), targ = prepare_data(model, cols)
    for v in range(3):
        assert np.array_equal(_bits(res[v].ps), _bits(again[v].ps)) and res[v].val_history == again[v].val_history
        tr = np.flatnonzero(folds != v)
        # by hand at the engine: the fold's training rows in table order, theta_0 and the epoch seeds as train() draws them from the seed
        eng = model.engine()
        eng.set_data(0, X[:, tr], [forc["ta"][tr]], [targ["reco"][tr]])
        eng.set_params(model.initialparameters(np.random.default_rng(5)))
        eng.opt_init("Adam", lr=0.01)
        eng.set_option("fused_update", 2)
        for epoch in (1, 2, 3):
            eng.train_epoch(64, seed=5 + epoch, shuffle=True, want_loss=False)
        assert np.array_equal(_bits(res[v].ps), _bits(eng.get_params())), v
        eng.close()
        one = eh.train(model, cols, folds=folds, val_fold=v, specialize=False, **kw)
        assert np.array_equal(_bits(res[v].ps), _bits(one.ps))
        assert len(res[v].val_history) == len(one.val_history) == 4
        for a, b in zip(res[v].val_history + res[v].train_history, one.val_history + one.train_history):
            for lt in kw["loss_types"]:
                assert a[lt]["reco"] == pytest.approx(b[lt]["reco"], rel=E2E_REL, abs=E2E_ABS), (v, lt, a[lt], b[lt])
        assert np.array_equal(_bits(res[v].val_obs_pred["reco_pred"]), _bits(one.val_obs_pred["reco_pred"]))
        assert np.array_equal(res[v].val_obs_pred["reco"], cols["reco"][folds == v])


def test_train_members_sweep_over_learning_rates_and_seeds():
    from easyhybrid_jl_amd.synthetic import make_synth_rbq10
    cols = make_synth_rbq10(400, seed=4)
    cols = dict(cols, sw_pot=cols["sw_pot"] / np.float32(50), dsw_pot=cols["dsw_pot"] / np.float32(50))
    members = [{"opt": eh.Adam(lr), "random_seed": s} for lr in (0.01, 0.002) for s in (1, 2)]
    res = eh.train_members(_front_model(), cols, members, nepochs=2, batchsize=64, patience=1, distributed=False)
    assert len(res) == 4 and all(r.ps.size == 338 for r in res)
    assert len({r.ps.tobytes() for r in res}) == 4
    one = eh.train(_front_model(), cols, nepochs=2, batchsize=64, patience=1, specialize=False, opt=eh.Adam(0.002), random_seed=2, distributed=False)
    assert np.array_equal(_bits(res[3].ps), _bits(one.ps)) and res[3].best_epoch == one.best_epoch
