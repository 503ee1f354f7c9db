"""The corpus of descriptors behind tests/test_plan.py, and the recorder of what eh_create answers to them.

    python tools/record_create_answers.py            # record tests/golden/create_answers.json with the library in the tree
    EASYHYBRID_HIP_LIB=/path/to/libeasyhybrid_hip.so python tools/record_create_answers.py      # ... with another build (the parent commit's)

The corpus is deterministic (no random generator): a base descriptor per model family (base_models), then single-field mutations of every
integer field and every array element in use, to the values of MUTATIONS, deduplicated.  One float mutation rides along (a parameter's
upper bound set to its lower bound: no integer reaches that check).  The recorder must run on a machine WITHOUT a HIP device: there
eh_create answers every descriptor it would build with "no HIP device", which is recorded as "accepted" (status 0, no message); with
a device it would build thousands of handles, and refuses to start.  The file holds the distinct messages once and (status, message
index) per case, plus the digest of the corpus it was recorded for."""
import ctypes as C
import hashlib
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import easyhybrid_jl_amd as eh                      # noqa: E402
from easyhybrid_jl_amd import _lib as L              # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "create_answers.json")
RBQ10 = {"rb": (3.0, 0.0, 13.0), "Q10": (2.0, 1.0, 4.0)}
EXPO2 = {"R0a": (1.0, 0.0, 5.0), "ka": (0.05, 0.0, 0.2), "R0b": (1.0, 0.0, 5.0), "kb": (0.02, 0.0, 0.2)}
RS3F = {n: (1.0, 0.0, 5.0) for n in ("Rb_het", "Rb_root", "Rb_myc")}
RS3F.update({n: (2.0, 1.0, 4.0) for n in ("Q10_het", "Q10_root", "Q10_myc")})
FLUXPART = {"RUE": (0.1, 0.0, 1.0), "Rb": (1.0, 0.0, 6.0), "Q10": (1.5, 1.0, 4.0)}


def two_output_closure(*, ta, sw, a, b, c):
    """a recorded closure with two outputs (EH_MECH_PROGRAM)"""
    r = a * b ** (0.125 * (ta - 15.0))
    return dict(r=r, g=r - c * sw)


TWO_OUT = {"a": (3.0, 0.0, 13.0), "b": (2.0, 1.0, 4.0), "c": (0.5, 0.0, 2.0)}


def _rbq10(hl, P=2, act="tanh", **kw):
    return eh.constructHybridModel([f"x{i}" for i in range(P)], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), ["rb"], ["Q10"], hidden_layers=hl, activation=act, **kw)


def _seq(cell, n, **kw):
    return _rbq10(eh.Chain(eh.Recurrence(cell(n, n) if cell is not eh.RNNCell else cell(n, n, "relu"))), **kw)


def base_models():
    """[(name, model, several_targets entry point, input BatchNorm allowed)]: one model of every family eh_create knows"""
    D, BN, LN = eh.Dense, eh.BatchNorm, eh.LayerNorm
    rs_pred = [f"p{i}" for i in range(32)]
    out = [
        ("rbq10_scaled", _rbq10([16, 16], scale_nn_outputs=True), False, True),
        ("rbq10_raw", _rbq10([16, 16]), False, True),
        ("rbq10_sigmoid", _rbq10([16, 16], act="sigmoid", scale_nn_outputs=True), False, True),
        ("expo2pool", eh.constructHybridModel([f"p{i}" for i in range(8)], ["T"], ["Resp_obs"], eh.Expo2Pool, dict(EXPO2), list(EXPO2), [],
                                              hidden_layers=[64, 64], scale_nn_outputs=True), False, True),
        ("rs3f", eh.constructHybridModel(rs_pred, ["ta", "sw_in", "vpd"], ["R_soil"], eh.Rs_components3F, dict(RS3F), list(RS3F), [],
                                         hidden_layers=[128, 128], scale_nn_outputs=True), False, True),
        ("lform_160", _rbq10([160, 64, 32, 16], act="sigmoid", scale_nn_outputs=True), False, True),
        ("multinn_acts", eh.constructHybridModel({"rb": ["a", "b"], "Q10": ["b"]}, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), [],
                                                 hidden_layers={"rb": [16, 16], "Q10": [8, 4]}, activation={"rb": "tanh", "Q10": "sigmoid"}), False, True),
        ("multinn_depths", eh.constructHybridModel({"rb": ["a"], "Q10": ["b"]}, ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), [],
                                                   hidden_layers={"rb": [16], "Q10": [8, 4]}), False, True),
        ("chain_acts", _rbq10(eh.Chain(D(16, 16, "tanh"), D(16, 8, "relu"))), False, True),
        ("chain_bn", _rbq10(eh.Chain(D(16, 16, "tanh"), BN(16), D(16, 8, "relu"), BN(8, "sigmoid"))), False, True),
        ("chain_bn_plain", _rbq10(eh.Chain(D(5, 7, "relu"), BN(7, "swish", affine=False))), False, True),
        ("chain_ln", _rbq10(eh.Chain(D(16, 16, "tanh"), LN(16), D(16, 8, "relu"), LN(8, "sigmoid"))), False, True),
        ("chain_ln_plain", _rbq10(eh.Chain(D(5, 7, "relu"), LN(7, "swish", affine=False))), False, True),
        ("chain_bn_ln", _rbq10(eh.Chain(BN(8), D(8, 8, "tanh"), LN(8))), False, True),
    ]
    for cell, nm in ((eh.LSTMCell, "lstm"), (eh.GRUCell, "gru"), (eh.RNNCell, "rnn")):
        out += [(f"{nm}_{n}", _seq(cell, n), False, False) for n in (15, 17)]
    flux = eh.constructHybridModel(["x0", "x1"], ["SW_IN", "TA"], ["RECO", "NEE"], eh.FluxPartModelQ10, dict(FLUXPART), ["RUE", "Rb"], ["Q10"],
                                   hidden_layers=eh.Chain(eh.Recurrence(eh.LSTMCell(15, 15))), scale_nn_outputs=True)
    out.append(("fluxpart_seq_two_targets", flux, True, False))
    out.append(("no_nn", eh.constructHybridModel([], ["ta"], ["reco"], eh.RbQ10, dict(RBQ10), [], ["rb", "Q10"]), False, False))
    ms = eh.models.resolve_mech(two_output_closure, list(TWO_OUT), ["ta", "sw"], ["r", "g"])
    out.append(("closure_two_outputs", eh.constructHybridModel(["x0", "x1"], ["ta", "sw"], ["g", "r"], ms, dict(TWO_OUT), ["a", "b"], ["c"],
                                                               hidden_layers=[16], scale_nn_outputs=True), False, True))
    return out


def input_bn(model):
    """the same model with the constructor's input_batchnorm"""
    import copy
    m = copy.copy(model)
    m.config = dict(model.config, input_batchnorm=True)
    return m


# (129 and 1025 thinned out: with them the golden file passes 100 KB, and they reach no refusal the others do not)
MUTATIONS = lambda v: (-1, 0, 1, v - 1, v + 1, 17, 33, 1 << 30)      # noqa: E731


def _in_use(d):
    """(field, index tuple) of every integer field and array element the descriptor uses"""
    per = d.n_nets if d.n_nets > 0 else d.n_hidden
    counts = {"hidden": d.n_hidden, "param_kind": d.n_params, "param_index": d.n_params, "forcing_index": d.n_forcings, "target_output": d.n_targets,
              "net_n_predictors": d.n_nets, "net_depth": d.n_nets, "net_activation": per if d.activation == L.EH_ACT_PER_NET else 0,
              "prog_out": d.prog_n_out if d.mech == L.EH_MECH_PROGRAM else 0, "prog_code": d.prog_len if d.mech == L.EH_MECH_PROGRAM else 0}
    for name, ctype in L.ModelDesc._fields_:
        if ctype in (C.c_int32, C.c_uint32):
            yield name, ()
        elif name == "net_hidden":
            for k in range(max(0, min(d.n_nets, L.EH_MAX_NETS))):
                for l in range(max(0, min(d.n_hidden, L.EH_MAX_HIDDEN))):
                    yield name, (k, l)
        elif name in counts:
            for i in range(max(0, min(counts[name], ctype._length_))):
                yield name, (i,)


def _get(d, name, ix):
    v = getattr(d, name)
    for i in ix:
        v = v[i]
    return v


def _set(d, name, ix, val):
    if not ix:
        setattr(d, name, val)
        return
    a = getattr(d, name)
    for i in ix[:-1]:
        a = a[i]
    a[ix[-1]] = val


def _wrap(name, v):
    return v & 0xFFFFFFFF if name == "prog_code" else v


def corpus():
    """[(label, several_targets, descriptor bytes)], deduplicated on (entry point, bytes), in a fixed order"""
    bases = []
    for name, m, several, bn_ok in base_models():
        bases.append((name, m.to_desc(), several))
        if several:
            bases.append((name + "@eh_create", m.to_desc(), False))
        if bn_ok:
            bases.append((name + "+input_bn", input_bn(m).to_desc(), several))
    out, seen = [], set()

    def add(label, several, d):
        b = bytes(d)
        if (several, b) not in seen:
            seen.add((several, b))
            out.append((label, several, b))
    for name, d0, several in bases:
        add(name, several, d0)
        for field, ix in _in_use(d0):
            v = int(_get(d0, field, ix))
            for m in MUTATIONS(v):
                d = L.ModelDesc.from_buffer_copy(bytes(d0))
                _set(d, field, ix, _wrap(field, m))
                add(f"{name}:{field}{list(ix)}={m}", several, d)
        for j in range(d0.n_params):
            d = L.ModelDesc.from_buffer_copy(bytes(d0))
            d.param_upper[j] = d.param_lower[j]
            add(f"{name}:param_upper[{j}]=lower", several, d)
    return out


def digest(cases):
    h = hashlib.sha256()
    for _, several, b in cases:
        h.update(struct.pack("<i", int(several)) + b)
    return h.hexdigest()


def write_records(cases, path):
    """the input of csrc/eh_plan_dump: [int32 several | descriptor] per case"""
    with open(path, "wb") as f:
        for _, several, b in cases:
            f.write(struct.pack("<i", int(several)) + b)


def record(cases):
    lib = L.lib()
    msgs, rows = [], []
    for label, several, b in cases:
        d = L.ModelDesc.from_buffer_copy(b)
        h = C.c_void_p()
        rc = (lib.eh_create_seq_targets if several else lib.eh_create)(C.byref(d), C.byref(h))
        if rc == L.EH_OK:
            raise SystemExit(f"{label}: eh_create built a handle -- this recorder is for a machine without a HIP device")
        msg = lib.eh_last_error(None).decode()
        if rc == L.EH_EHIP and msg.startswith("eh_create: no HIP device"):
            rows.append([0, -1])
            continue
        if msg not in msgs:
            msgs.append(msg)
        rows.append([rc, msgs.index(msg)])
    return msgs, rows


def fail_sites(text, call=r"eh_plan_fail\(msg"):
    """the message formats of the refusal sites in a source text, each as a regular expression a message of that site matches in full"""
    import re
    out = []
    for m in re.finditer(call + r',\s*EH_\w+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text):
        fmt = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1)))
        rx = re.escape(fmt)
        for spec, pat in ((r"%zu", r"\d+"), (r"%d", r"-?\d+"), (r"%u", r"\d+"), (r"%s", r".*")):
            rx = rx.replace(re.escape(spec), pat)
        out.append((fmt, re.compile(rx + r"\Z", re.S)))
    return out


def sites_reached(sites, messages):
    return [fmt for fmt, rx in sites if any(rx.match(m) for m in messages)]


def main():
    cases = corpus()
    msgs, rows = record(cases)
    doc = {"library": "the parent commit of the change that introduced csrc/eh_plan.hpp, on a machine without a HIP device",
           "corpus_sha256": digest(cases), "messages": msgs, "cases": rows}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    nref = sum(1 for r in rows if r[0] != 0)
    print(f"{len(cases)} cases, {nref} refusals, {len(msgs)} distinct messages, {os.path.getsize(GOLDEN)} bytes -> {GOLDEN}")


if __name__ == "__main__":
    main()
