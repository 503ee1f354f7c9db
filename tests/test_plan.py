"""The plan eh_create builds its handle from (csrc/eh_plan.hpp), checked without a device through the stand-alone csrc/eh_plan_dump:
its refusals against what the parent's eh_create answered to the same corpus (tests/golden/create_answers.json, recorded by
tools/record_create_answers.py), its layout of flat theta against models.py -- the independent second implementation --, and the EhNet
of the canonical descriptors against the strings their ahead-of-time kernels were built with (csrc/Makefile, SPECDEF_*)."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easyhybrid.jl_amd", "csrc")
DUMP = os.path.join(ROOT, "easyhybrid.jl_amd", "eh_plan_dump")
_spec = importlib.util.spec_from_file_location("record_create_answers", os.path.join(ROOT, "tools", "record_create_answers.py"))
rca = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rca)

P_REFUSAL = "eh_create: no kernel for P="      # the one refusal ahead of the device check that needs the kernel tables: eh_create's own, behind the plan


def dump(cases, tmp_path):
    path = os.path.join(str(tmp_path), "descs.bin")
    rca.write_records(cases, path)
    out = subprocess.run([DUMP, path], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    return [json.loads(line) for line in out]


@pytest.fixture(scope="module")
def corpus():
    return rca.corpus()


@pytest.fixture(scope="module")
def golden():
    with open(rca.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plans(corpus, tmp_path_factory):
    return dump(corpus, tmp_path_factory.mktemp("plan"))


def test_the_corpus_is_the_recorded_one(corpus, golden):
    assert len(corpus) == len(golden["cases"]) and rca.digest(corpus) == golden["corpus_sha256"]


def test_the_planner_answers_what_the_parent_answered(corpus, golden, plans):
    bad = []
    for (label, _, b), (rc, mi), got in zip(corpus, golden["cases"], plans):
        if rc == 0:
            ok = got["rc"] == 0 and "leaves" in got
        elif golden["messages"][mi].startswith(P_REFUSAL):      # the planner passes it on; eh_create refuses when no fused kernel holds it
            d = rca.L.ModelDesc.from_buffer_copy(b)
            ok = got["rc"] == 0 and got["family"] in ("fused", "norm") and d.input_batchnorm != 0 and d.n_predictors > 32
        else:
            ok = got["rc"] == rc and got["msg"] == golden["messages"][mi]
        if not ok:
            bad.append((label, rc, golden["messages"][mi] if mi >= 0 else None, {k: got[k] for k in ("rc", "msg") if k in got}))
    assert not bad, (len(bad), bad[:5])


def test_the_corpus_reaches_the_refusals(golden):
    """at least a third of the cases are refusals, and they reach at least 50 of the refusal sites ahead of the device check"""
    n_ref = sum(1 for rc, _ in golden["cases"] if rc != 0)
    assert 3 * n_ref >= len(golden["cases"]), (n_ref, len(golden["cases"]))
    with open(os.path.join(CSRC, "eh_plan.hpp")) as f:
        sites = rca.fail_sites(f.read())
    with open(os.path.join(CSRC, "eh_api.hip")) as f:
        sites += [s for s in rca.fail_sites(f.read(), r"fail\(nullptr") if s[0].startswith(P_REFUSAL)]
    assert 50 <= len(sites) <= 64, len(sites)
    reached = rca.sites_reached(sites, golden["messages"])
    assert len(reached) >= 50, (len(reached), sorted(set(s[0] for s in sites) - set(reached)))


MODELS = []
for _name, _m, _several, _bn_ok in rca.base_models():
    MODELS.append((_name, _m, _several))
    if _bn_ok:
        MODELS.append((_name + "+input_bn", rca.input_bn(_m), _several))


@pytest.fixture(scope="module")
def model_plans(tmp_path_factory):
    return dump([(name, several, bytes(m.to_desc())) for name, m, several in MODELS], tmp_path_factory.mktemp("models"))


@pytest.mark.parametrize("i", range(len(MODELS)), ids=[m[0] for m in MODELS])
def test_the_layout_is_pythons(i, model_plans):
    _, m, _ = MODELS[i]
    p = model_plans[i]
    assert p["rc"] == 0, p
    want, off = [], 0
    for k, li, name, shape in m.leaves():
        want.append([k, li, name, off, shape[0], shape[1] if len(shape) == 2 else 0])
        off += int(np.prod(shape))
    assert [l[:6] for l in p["leaves"]] == want
    assert p["n_theta"] == m.n_theta and p["g_off"] == off and p["g_off"] + len(m.global_param_names) == p["n_theta"]
    mask = np.zeros(m.n_theta, bool)
    for _, _, _, o, rows, cols, w in p["leaves"]:
        mask[o:o + rows * max(cols, 1)] = w
    assert np.array_equal(mask, m.weight_mask()) and p["n_weights"] == int(mask.sum())
    assert p["n_acc"] == m.n_theta + 1 + len(m.targets) + 2
    # a BatchNorm layer's running statistics: [mean | var] of its width, one behind the other in chain order
    bn = [l for l in m.bn_layers]
    widths = [m.NN[l][0] for l in bn]
    assert p["norm"]["layers"] == [[l, 2 * sum(widths[:j]), w] for j, (l, w) in enumerate(zip(bn, widths))] and p["norm"]["total"] == 2 * sum(widths)
    assert p["norm"]["widest"] == max([m.NN[l][0] for l in m.norm_layers], default=0)
    family = "none" if not m.nets else "seq" if m.lstm_layer is not None else "norm" if m.norm_layers else "fused"
    assert p["family"] == family


def test_the_canonical_descriptors_still_hit_their_kernels(model_plans):
    """SPECDEF_0 .. SPECDEF_6: the EhNet of the plan is the -DEH_SPEC_NET= string the ahead-of-time kernel was compiled around (every
    field the constructor sets; the loss fields keep their default 0), and the block counts are the kernel's shape"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        specs = dict(re.findall(r"^SPECDEF_(\d) := (.*)$", f.read(), re.M))
    assert sorted(specs) == list("0123456")
    by_name = {MODELS[i][0]: p for i, p in enumerate(model_plans)}
    for k, name in (("0", "rbq10_scaled"), ("1", "rbq10_raw"), ("5", "rbq10_sigmoid"), ("2", "expo2pool"), ("3", "rs3f"), ("4", "rs3f"), ("6", "rs3f")):
        p = by_name[name]
        assert p["net"].replace(" ", "") == re.search(r"-DEH_SPEC_NET=(\S+)", specs[k]).group(1), (k, p["net"])
        nbi, nbh, nl = re.search(r"-DEH_SPEC_SHAPE=(\d+),(\d+),(\d+),", specs[k]).groups()
        assert (p["nbi"], p["nbh"], p["family"]) == (int(nbi), int(nbh), "fused") and len({l[1] for l in p["leaves"]}) == int(nl) + 1
        assert p["act"] == int(re.search(r"-DEH_SPEC_ACT=(\d)", specs[k]).group(1))
