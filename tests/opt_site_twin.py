"""The optimiser rule of csrc/eh_device.hpp (eh_opt_update) in NumPy, float32 op for op, with what a test of ONE update site needs
around it: a warm state, the bar of an element, the conditions the inputs have to meet, and the element-by-element comparator.

Why a warm state: the first Adam / RMSProp steps are sign-like (m / sqrt(v) ~ g / |g|), so two summation orders of one gradient end
lr apart on the entries near zero.  From moments 40 steps old, |m0| in [2, 4] s and v0 in [2, 4] s^2 (s = max |g|), one step is a smooth
function of g: two summation orders end a few 1e-9 apart in theta, while every element still moves by thousands of bars.

The running products: the engine keeps, per group, the pair (beta1^t, beta2^t) the NEXT update divides by; an update uses the pair as it
stands and leaves pair * (beta1, beta2) behind (eh_reduce_kernel's tail, eh_opt_advance_groups).  No GPU in here."""
import numpy as np

F = np.float32
AGE = 40                      # the warm state's products are AGE steps old (group k of a grouped handle: AGE + 4 k, so that no two groups share a pair)

RULES = {
    "Adam": dict(rule="Adam", lr=0.01),
    "AdamW": dict(rule="AdamW", lr=0.01, weight_decay=0.05),
    "RMSProp": dict(rule="RMSProp", lr=0.01),
    "Descent": dict(rule="Descent", lr=0.05),
}
GROUPED = [RULES["Adam"], RULES["AdamW"], RULES["RMSProp"], RULES["Descent"]]       # the grouped handle: one group per rule


def hyper(r):
    return (F(r.get("lr", 0.01)), F(r.get("beta1", 0.9)), F(r.get("beta2", 0.999)), F(r.get("eps", 1e-8)), F(r.get("weight_decay", 0.0)))


def keeps(r):
    """(keeps m, keeps v) of a rule: state a rule does not keep is never written"""
    return {"Adam": (True, True), "AdamW": (True, True), "RMSProp": (False, True), "Descent": (False, False)}[r.get("rule", "Adam")]


def rule_update(r, g, th, m, v, bt1, bt2):
    """eh_opt_update on arrays: every operation rounds to float32, in the order the device code writes them"""
    lr, b1, b2, eps, wd = hyper(r)
    g, th, m, v = (np.asarray(a, F) for a in (g, th, m, v))
    bt1, bt2 = F(bt1), F(bt2)
    one = F(1)
    kind = r.get("rule", "Adam")
    if kind in ("Adam", "AdamW"):
        m = b1 * m + (one - b1) * g
        v = b2 * v + (one - b2) * (g * g)
        upd = m / (one - bt1) / (np.sqrt(v / (one - bt2)) + eps) * lr
        if kind == "AdamW":
            upd = upd + lr * wd * th                   # AdamW(couple = true): (lr * wd) * theta
        th = th - upd
    elif kind == "RMSProp":                            # RMSProp(eta, rho = beta1, eps)
        v = b1 * v + (one - b1) * (g * g)
        th = th - g * (lr / (np.sqrt(v) + eps))
    elif kind == "Descent":
        th = th - lr * g
    else:
        raise ValueError(kind)
    return th.astype(F), m.astype(F), v.astype(F)


def as_groups(rules, group, n):
    """(list of rules, group id per element) of a single rule (a dict, group None) or a grouped handle"""
    if isinstance(rules, dict):
        return [rules], np.zeros(n, np.uint8)
    return list(rules), np.asarray(group, np.uint8)


def step(rules, group, g, th, m, v, bt, valid=True):
    """One update of every element under its group's rule and that group's own products.  bt: (2,) for one rule, (n_groups, 2) for groups.
    Returns (theta, m, v, bt advanced); valid = False (no sample of the minibatch had a target): everything as it came."""
    th, m, v = (np.array(a, F) for a in (th, m, v))
    bt = np.array(bt, F)
    if not valid:
        return th, m, v, bt
    rl, gid = as_groups(rules, group, th.size)
    b = bt.reshape(len(rl), 2)
    out = b.copy()
    g = np.asarray(g, F)
    for k, r in enumerate(rl):
        sel = gid == k
        th[sel], m[sel], v[sel] = rule_update(r, g[sel], th[sel], m[sel], v[sel], b[k, 0], b[k, 1])
        _, b1, b2, _, _ = hyper(r)
        out[k, 0] = b[k, 0] * b1
        out[k, 1] = b[k, 1] * b2
    return th, m, v, out.reshape(bt.shape)


def warm_products(rules):
    """float32(beta)^age per group: (2,) for one rule, (n_groups, 2) for a list"""
    rl = [rules] if isinstance(rules, dict) else list(rules)
    bt = np.empty((len(rl), 2), F)
    for k, r in enumerate(rl):
        _, b1, b2, _, _ = hyper(r)
        bt[k] = (b1 ** F(AGE + 4 * k), b2 ** F(AGE + 4 * k))
    return bt[0] if isinstance(rules, dict) else bt


def warm_state(n, s, seed):
    """moments as old steps with gradients of size s left them: |m0| in [2, 4] s with random signs, v0 in [2, 4] s^2"""
    rng = np.random.default_rng(seed)
    s = np.float64(s)
    m0 = (rng.uniform(2.0, 4.0, n) * s * rng.choice([-1.0, 1.0], n)).astype(F)
    v0 = (rng.uniform(2.0, 4.0, n) * s * s).astype(F)
    return m0, v0


def random_groups(n, n_groups, seed):
    """a group per ELEMENT from a seeded generator: borders inside every vector, tile and lane segment"""
    return np.random.default_rng(seed).integers(0, n_groups, n).astype(np.uint8)


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, F)).astype(F)).astype(np.float64)


def self_error(rules, group, g32, g64, th0, m0, v0, bt0):
    """the reference against itself, per element: 4 max_j |rule_x(g32)_j - rule_x(g64)_j| for x in theta, m, v -- the oracle's fp32 and fp64
    gradients of one case (two summation orders of the same sum), both cast to float32 before the rule; the margin of four is
    tests/test_gpu_fuzz.py's"""
    a = step(rules, group, np.asarray(g32).astype(F), th0, m0, v0, bt0)
    b = step(rules, group, np.asarray(g64).astype(F), th0, m0, v0, bt0)
    rl, gid = as_groups(rules, group, np.asarray(th0).size)
    out = {}
    for i, x in enumerate(("theta", "m", "v")):
        d = np.abs(a[i].astype(np.float64) - b[i].astype(np.float64))
        e = np.zeros(d.size)
        for k in range(len(rl)):            # (a grouped handle: the maximum over the elements of the element's own group -- never above the one over all)
            sel = gid == k
            if sel.any():
                e[sel] = 4.0 * float(d[sel].max())
        out[x] = e
    return out


def add_errors(*es):
    """the bar's first term over several steps: m and v carry a step's deviation on with factors beta < 1, theta with factor 1 plus the
    deviation of the update, itself a contraction of those of m and v under a warm state -- so the deviations of the steps at most add"""
    return {k: sum(e[k] for e in es) for k in ("theta", "m", "v")}


def element_bars(err, ref, steps=1):
    """bar of element i of x: err[x] + 2 ulp(|x_ref,i|) per step"""
    return {k: err[k] + 2.0 * steps * ulp(ref[k]) for k in ("theta", "m", "v")}


def check_inputs(name, rules, group, g32, g64, th0, m0, v0, bt0):
    """The conditions a case's inputs must meet, from the reference alone: under Adam / AdamW every element of theta, m and v moves by at
    least 1000 bars, under RMSProp every element of v does, under Descent at least 85 % of the elements of theta move by more than 100
    bars.  Returns the smallest ratios (for the record)."""
    rl, gid = as_groups(rules, group, np.asarray(th0).size)
    err = self_error(rules, group, g32, g64, th0, m0, v0, bt0)
    th, m, v, _ = step(rules, group, np.asarray(g32).astype(F), th0, m0, v0, bt0)
    ref = {"theta": th, "m": m, "v": v}
    bars = element_bars(err, ref)
    x0 = {"theta": np.asarray(th0, F), "m": np.asarray(m0, F), "v": np.asarray(v0, F)}
    move = {k: np.abs(ref[k].astype(np.float64) - x0[k].astype(np.float64)) / bars[k] for k in ref}
    out = {}
    for k, r in enumerate(rl):
        sel = gid == k
        if not sel.any():
            continue
        kind = r.get("rule", "Adam")
        if kind in ("Adam", "AdamW"):
            for x in ("theta", "m", "v"):
                lo = float(move[x][sel].min())
                out[f"{kind}.{x}"] = lo
                assert lo >= 1000.0, f"{name}: {kind} element of {x} moves by only {lo:.1f} bars"
        elif kind == "RMSProp":
            lo = float(move["v"][sel].min())
            out["RMSProp.v"] = lo
            assert lo >= 1000.0, f"{name}: RMSProp element of v moves by only {lo:.1f} bars"
        else:
            share = float(np.mean(move["theta"][sel] > 100.0))
            out["Descent.share"] = share
            assert share >= 0.85, f"{name}: only {100 * share:.1f} % of the Descent elements of theta move by more than 100 bars"
    return out


def compare(site, got, ref, bars, set_state=None, rules=None, group=None, quiet=False):
    """Element by element: got / ref = dicts theta, m, v, bt; bars = element_bars(...).  State a rule does not keep (m under RMSProp, m and
    v under Descent; those elements of a grouped handle) must be the bits that were set (set_state = dict m, v), and the products must be
    the float32 products exactly.  Prints the largest deviation in units of the bar; raises AssertionError naming the worst element.
    Returns {x: largest deviation / bar}."""
    worst = {}
    bad = []
    n = np.asarray(ref["theta"]).size
    for x in ("theta", "m", "v"):
        g_, r_ = np.asarray(got[x], F), np.asarray(ref[x], F)
        assert g_.shape == r_.shape, f"{site}: {x} has shape {g_.shape}, expected {r_.shape}"
        d = np.abs(g_.astype(np.float64) - r_.astype(np.float64))
        d[~np.isfinite(d)] = np.inf
        ratio = d / bars[x]
        i = int(np.argmax(ratio))
        worst[x] = float(ratio[i])
        if not ratio[i] <= 1.0:
            bad.append(f"{x}[{i}] = {g_[i]!r}, reference {r_[i]!r}: {ratio[i]:.3g} bars ({int(np.sum(~(ratio <= 1.0)))} of {n} elements over the bar)")
    if rules is not None and set_state is not None:
        rl, gid = as_groups(rules, group, n)
        for k, r in enumerate(rl):
            km, kv = keeps(r)
            sel = gid == k
            for x, kept in (("m", km), ("v", kv)):
                if kept or not sel.any():
                    continue
                a, b = np.asarray(got[x], F)[sel], np.asarray(set_state[x], F)[sel]
                if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
                    j = int(np.flatnonzero(sel)[np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))[0]])
                    bad.append(f"{x}[{j}] was written although {r['rule']} keeps no {x}")
    gb, rb = np.asarray(got["bt"], F), np.asarray(ref["bt"], F)
    if gb.shape != rb.shape or not np.array_equal(gb.view(np.uint32), rb.view(np.uint32)):
        bad.append(f"running products {gb.tolist()}, expected exactly {rb.tolist()}")
    if not quiet:
        print(f"opt-site {site}: largest deviation / bar  theta {worst['theta']:.3g}  m {worst['m']:.3g}  v {worst['v']:.3g}"
              f"  (bars: theta {float(np.median(bars['theta'])):.3g}  m {float(np.median(bars['m'])):.3g}  v {float(np.median(bars['v'])):.3g}, median)")
    assert not bad, f"{site}: " + "; ".join(bad)
    return worst


def compare_unchanged(site, got, was):
    """a minibatch without a valid target moves nothing: theta, m, v and the products are the bits that were set"""
    for x in ("theta", "m", "v", "bt"):
        a, b = np.asarray(got[x], F), np.asarray(was[x], F)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            f"{site}: {x} changed on a minibatch without a valid target ({int(np.sum(a.view(np.uint32) != b.view(np.uint32)))} elements)"
