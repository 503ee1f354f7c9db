"""Every place the optimiser rule (eh_opt_update, csrc/eh_device.hpp) is called from, element by element: ONE step (two where the update
is applied by the next step's prologue) from a warm state, against the rule's float32 twin (tests/opt_site_twin.py) fed the device's own
gradient.  The trajectory tests start from a young Adam state, where rounding noise of near-zero gradient entries becomes lr-sized moves,
and so have to let a share of the elements go; here theta, m and v of every element are held to the bar
    4 max_j |rule(g32)_j - rule(g64)_j| + 2 ulp(|x_ref,i|)        (g32, g64: the oracle's two summation orders; nothing from the device)
while each of them moves by thousands of bars (tests/test_opt_sites.py checks that on the reference alone).  An element a site never
updates, updates twice, updates with its neighbour's gradient or under another group's rule or products sticks out by orders of magnitude.

Per case: (1) the gradient from a reference handle R (the kernels built ahead of time off, as tests/util.py load_engine leaves them);
(2) the handle under test: set_params, opt_init*, set_opt_state(warm), the step(s); (3) theta, m, v and the products against the twin;
(4) the parameter image: loss_and_grad on the stepped handle == loss_and_grad of a fresh handle given get_params(), bit for bit; (5) the
same site on targets that are all NaN: nothing moves, bit for bit.  eh_jit_status' "update sites:" counts prove which site applied the
update.  Rules: Adam, AdamW (wd 0.05), RMSProp (lr 0.01 each), Descent (lr 0.05) and a grouped handle with one group per rule and a group
id drawn per element."""
import numpy as np
import pytest

import easyhybrid_jl_amd as eh
from tests import opt_site_cases as oc
from tests import opt_site_twin as tw

pytestmark = pytest.mark.gpu
TRAIN = eh.EH_SPLIT_TRAIN
RULES = list(oc.RULE_NAMES)


def status(e):
    """(log, {site: count}) of eh_jit_status"""
    _, log = e.jit_status()
    sites = {}
    if "update sites:" in log:
        w = log.split("update sites:")[1].split(";")[0].split()
        sites = dict(zip(w[::2], (int(x) for x in w[1::2])))
    return log, sites


def plain_init(e, rules, group):
    if group is None:
        r = dict(rules)
        e.opt_init(r.pop("rule"), **r)
    else:
        e.opt_init_groups(group, rules)


def make_engine(case, ref, configure, init=plain_init, nan=False, warm=True):
    e = case.engine(nan)
    if configure:
        configure(e)
    init(e, ref["rules"], ref["group"])
    if warm:
        e.set_opt_state(ref["m0"], ref["v0"], ref["bt0"])
    return e


def run_steps(e, B, steps):
    for k in range(steps):
        e.train_step(k * B, B, want_loss=False)


def state_of(e):
    e.synchronize()
    m, v, bt = e.get_opt_state()
    return dict(theta=e.get_params(), m=m, v=v, bt=np.asarray(bt, np.float32))


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_site(site, model, B, rule, configure=None, steps=1, run=run_steps, init=plain_init, expect=None):
    """the five checks of a case (module docstring).  expect(log, sites): proof that the named site applied the update."""
    ref = oc.reference(model, B, steps, rule)
    rules, group = ref["rules"], ref["group"]
    case = oc.case(model, B, steps)
    R = make_engine(case, ref, None, warm=False)
    E = make_engine(case, ref, configure, init)
    st = (ref["theta0"], ref["m0"], ref["v0"], ref["bt0"])
    for k in range(steps):                      # the twin fed the reference handle's gradient at the twin's own parameters
        R.set_params(st[0])
        _, g, nv = R.loss_and_grad(TRAIN, k * B, B)
        assert nv > 0
        st = tw.step(rules, group, g, *st)
    R.close()
    run(E, B, steps)
    got = state_of(E)
    want = dict(theta=st[0], m=st[1], v=st[2], bt=st[3])
    bars = tw.element_bars(tw.add_errors(*[s["err"] for s in ref["steps"]]), want, steps)
    log, sites = status(E)
    print(f"opt-site {site} [{model} B={B} x{steps} {rule}]: {sites} {log[-120:] if 'train step kernel' in log else ''}")
    tw.compare(f"{site} [{model} B={B} x{steps} {rule}]", got, want, bars, set_state=dict(m=ref["m0"], v=ref["v0"]), rules=rules, group=group)
    if expect:
        expect(log, sites)
    # the parameter image behind the update: what the stepped handle computes from it == a fresh handle given the parameters
    l1, g1, n1 = E.loss_and_grad(TRAIN, 0, B)
    E.close()
    Fh = make_engine(case, ref, configure, init, warm=False)
    Fh.set_params(got["theta"])
    l2, g2, n2 = Fh.loss_and_grad(TRAIN, 0, B)
    Fh.close()
    assert n1 == n2 and same_bits(np.float32(l1), np.float32(l2)) and same_bits(g1, g2), \
        f"{site}: the stepped handle's parameter image is not its parameters ({int(np.sum(g1.view(np.uint32) != g2.view(np.uint32)))} gradient entries differ)"
    # no valid target: nothing moves
    N = make_engine(case, ref, configure, init, nan=True)
    run(N, B, steps)
    after = state_of(N)
    N.close()
    tw.compare_unchanged(f"{site} [{model} B={B} x{steps} {rule}]", after, dict(theta=ref["theta0"], m=ref["m0"], v=ref["v0"], bt=ref["bt0"]))
    if ref["theta0"].size > 1 << 16:             # (the tutorial net's reference is 40 MB per rule: not kept for the session)
        oc.reference.cache_clear()


def only(**want):
    """the update sites that applied something are exactly these, that often"""
    def expect(log, sites):
        assert sites == want, (sites, want, log[-300:])
    return expect


def option(**kw):
    def configure(e):
        for k, v in kw.items():
            e.set_option(k, v)
    return configure


# ---- eh_reduce_kernel<true, ...> behind the step ("fused_update" 0) ---------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("B", [1, 64, 257])
def test_reduce16(B, rule):
    """n_acc = 342 < 8192, not layer-wise: 16 columns per workgroup (eh_do_step); one slab row (B <= 256) and two"""
    check_site("reduce<16>", "headline", B, rule, option(fused_update=0), expect=only(reduce16=1))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("model", ["w64", "w128"])
def test_reduce64(model, rule):
    """n_acc >= 8192: 64 columns per workgroup, behind the per-wave kernels (P = 32, three layers of 64) and the row-split ones (128, 128)"""
    check_site("reduce<64>", model, 257, rule, option(fused_update=0), expect=only(reduce64=1))


def test_row_split_and_layerwise_handles_have_no_one_kernel_sites():
    """the one-kernel steps ("fused_update" 1 and its flush / prologue apply) exist for the per-wave kernels only: the row-split family
    refuses the option, so eh_reduce_kernel is its one update site (csrc/eh_wide.hpp calls the rule nowhere)"""
    ref = oc.reference("w128", 257, 1, "Adam")
    e = make_engine(oc.case("w128", 257, 1), ref, None)
    with pytest.raises(NotImplementedError, match="fused_update is not built for hidden widths above 64"):
        e.set_option("fused_update", 1)
    e.train_step(0, 257, want_loss=False)
    e.synchronize()
    assert status(e)[1] == dict(reduce64=1)
    e.close()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("model", ["lf4", "lf4odd"])
def test_reduce256_four_columns_per_thread(model, rule):
    """layer-wise, more than one slab row (B = 300 > 256), n_acc >= 16384: four columns per thread on 16-byte accesses; n_theta = 2 and
    3 mod 4, so the thread across the end of theta takes the scalar path"""
    assert oc.case(model, 300, 1).theta0.size % 4 == (2 if model == "lf4" else 3)
    check_site("reduce<256,4,VEC>", model, 300, rule, expect=only(reduce256v4=1))


# ---- "fused_update" 1: the float-atomic one-kernel step; its update is applied by eh_fused_flush_kernel or by the next step's prologue ----
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("B,steps", [(257, 1), (257, 2), (64, 1), (64, 2)])
def test_fused_flush_and_prologue_apply(B, steps, rule):
    """the general step kernel ("lean" 0).  One step: the flush applies it.  Two steps: the second step's prologue applies the first (the
    eight-shard fold; every workgroup rebuilds its image, the stores spread by (idx & gmask) == blockIdx.x), the flush the second."""
    def expect(log, sites):
        assert "train step kernel: general" in log and "train step kernel: lean" not in log, log[-200:]
        assert sites == (dict(fused_flush=1) if steps == 1 else dict(prologue=1, fused_flush=1)), sites
    check_site("flush / prologue", "headline", B, rule, option(fused_update=1, lean=0), steps=steps, expect=expect)


# ---- "fused_update" 2: the ordered step; eh_ord_flush_kernel or the next ordered step's prologue (the ordered group fold) -------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("B,steps", [(257, 1), (257, 2), (4349, 1), (4349, 2)])
@pytest.mark.parametrize("kernels", ["aot-lean", "aot-general", "generic"])
def test_ordered_step(kernels, B, steps, rule):
    """2 and 17 workgroups; the kernels built ahead of time (what a default handle runs) in their lean form -- Adam alone has one -- and with
    "lean" 0, and the generic kernels"""
    cfg = dict(aot_spec=0 if kernels == "generic" else 1, fused_update=2, lean=0 if kernels == "aot-general" else 1)

    def expect(log, sites):
        assert f"ordered steps: {steps}" in log, log[-200:]
        assert sites == (dict(ord_flush=1) if steps == 1 else dict(ord_prologue=1, ord_flush=1)), sites
        if kernels != "generic":
            assert log.startswith("ahead-of-time"), log[:200]
        lean = kernels == "aot-lean" and rule == "Adam"
        assert ("train step kernel: lean" in log) == lean and ("train step kernel: general" in log) == (not lean), log[-200:]
    check_site("ordered step", "headline", B, rule, option(**cfg), steps=steps, expect=expect)


# ---- the multi-step launch: eh_ms_apply ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_multi_step_launch(rule):
    """train_epoch(64) over 128 samples with "multi_step" 1: both steps in one launch, each applying its own update from LDS"""
    def run(e, B, steps):
        _, n = e.train_epoch(B, shuffle=False, want_loss=False)
        assert n == steps
    check_site("eh_ms_apply", "headline", 64, rule, option(fused_update=1, multi_step=1), steps=2, run=run, expect=only(multi_step=2))


# ---- the data-parallel seam: eh_apply_kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_dp_apply(rule):
    def run(e, B, steps):
        e.dp_grad(0, B)
        e.dp_apply()
    check_site("eh_apply_kernel", "headline", 257, rule, run=run, expect=only(dp_apply=1))


# ---- the layer-wise epilogues ----------------------------------------------------------------------------------------------------------------
# eh_lform_train (csrc/eh_lform.hip): the optimiser runs in the epilogue of the grouped weight-gradient launch when the minibatch is ONE slab
# row (B <= 128) and every weight-gradient product sits in the grouped launch -- the tiled ones take 16-byte pieces, so B is a multiple of 16
# and every width a multiple of four.  eh_dw_apply64_kernel (32 x 32 tiles, the samples split over the waves) where also B <= 64 and a delta
# product outside the tail chain has summed the chain's partial rows on the side (a layer of more than 256 inputs above the first);
# eh_dw_apply_kernel (64 x 64 tiles) otherwise.  Every other minibatch goes through the reduction.
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("model,B", [(m, b) for m in ("lf288", "lf264s", "lf272p12") for b in (48, 64)] + [("tutorial", 64)])
def test_dw_apply64(model, B, rule):
    """tile edges off 32 (80, 40, 20; 264, 48; 272, 12 inputs), thin products (the first layer's two inputs, the output layer), tiled ones, the
    bias column sums and the global parameter; the tutorial net"""
    check_site("eh_dw_apply64_kernel", model, B, rule, expect=only(dw_apply64=1))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("model,B", [(m, b) for m in ("lf4", "lfswish") for b in (64, 80, 128)] + [("lf129", 64)])
def test_dw_apply(model, B, rule):
    """one slab row, 64 x 64 tiles: the whole net inside the tail chain (B = 64 too), or 64 < B <= 128; one hidden layer of 129 units: thin
    products only (two inputs, one output), so the width need not be a multiple of four"""
    check_site("eh_dw_apply_kernel", model, B, rule, expect=only(dw_apply=1))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("model,B,site", [("lf4", 37, "reduce256v4"), ("lf4", 65, "reduce256v4"), ("lf4", 130, "reduce256v4"), ("lf4", 256, "reduce256v4"),
                                          ("tutorial", 37, "reduce256v4")])
def test_layerwise_minibatches_the_epilogues_do_not_take(model, B, site, rule):
    """no multiple of 16 (37, 65), two slab rows (130, 256): the step + reduce pair, four columns per thread"""
    check_site("layer-wise, reduce", model, B, rule, expect=only(**{site: 1}))


@pytest.mark.parametrize("rule", RULES)
def test_multi_network_layerwise(rule):
    """a MultiNN model on the layer-wise form at B = 64: the tail chain whose partial rows the epilogues pick up is built for one network
    (eh_lform_train), so the step goes through the reduction -- n_acc >= 16384 and one slab row: four columns per thread"""
    check_site("MultiNN layer-wise", "multi", 64, rule, expect=only(reduce256v4=1))


# ---- norm layers inside the chain, the sequence step, the optimiser chain ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("model", ["bnchain", "lnchain"])
def test_norm_chain_leaves(model, rule):
    """Dense, norm, Dense, norm at B = 64: scale and bias of the norm layers are leaves of theta like any other, compared element by element.
    Norm layers keep the step off the grouped weight gradients (eh_lform_train), so it goes through the reduction; n_acc < 8192"""
    check_site("norm-layer chain", model, 64, rule, expect=only(reduce16=1))


@pytest.mark.parametrize("rule", RULES)
def test_sequence_reduce(rule):
    """LSTMCell(4, 4), windows of 5 records, 33 windows: the step + reduce pair, n_acc < 8192"""
    check_site("sequence reduce", "lstm", 33, rule, expect=only(reduce16=1))


@pytest.mark.parametrize("rule", [r for r in RULES if r != "grouped"])
def test_chain_apply_of_the_do_nothing_chain(rule):
    """OptimiserChain(rule): the reduction leaves the gradient, eh_chain_apply_kernel applies it.  (A chain takes one rule: eh_opt_init_chain
    has no groups, so no grouped handle here.  The chain's other stages: tests/test_gpu_chain.py.)"""
    def init(e, rules, group):
        r = dict(rules)
        e.opt_init_chain([("rule",)], **r)
    check_site("eh_chain_apply_kernel", "headline", 257, rule, option(fused_update=0), init=init, expect=only(chain=1))
