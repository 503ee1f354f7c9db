"""NumPy twin of the device's L-BFGS (csrc/eh_lbfgs.hpp): history m, the weak-Wolfe bisection line search of Lewis and
Overton, the two-loop recursion on coefficient vectors over the basis {S_0.., Y_0.., g} with the basis' Gram matrix.  Every scalar in
float64; theta, the gradients and the history in `dtype`.  Written from the algorithm's description, not from the device code: the
tests hold the one against the other.

    lbfgs(fg, x, maxiters, ...) -> Result(theta, f, evaluations, trace, status, iterations)

fg(x) -> (loss, gradient) or (loss, gradient, n_valid); trace: one dict per accepted iteration with f, t, trials, g_inf, sy, decisions
("A" per trial that failed the sufficient-decrease test, "C" per trial that failed the curvature test), evaluations.
`observe`, if given, is called once per evaluation with what the decision saw and what it decided (the seam of the host-logic test).
"""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "theta f evaluations trace status iterations")
NOOP, REJECT, ACCEPT, ACCEPT_DONE, RESTART, FAIL_DONE, ACCEPT_PAUSE = range(7)


def _dot(a, b):
    return float(np.dot(np.asarray(a, np.float64), np.asarray(b, np.float64)))


def _row_dot(m, npairs, c, G, row):
    a = 0.0
    for j in range(npairs):
        a += c[j] * G[row, j]
    for j in range(npairs):
        a += c[m + j] * G[row, m + j]
    return a + c[2 * m] * G[row, 2 * m]


def direction(m, npairs, head, G):
    """coefficients of d = -H g over [S_0 .. S_{m-1}, Y_0 .. Y_{m-1}, g] and g.d"""
    ig = 2 * m
    c = np.zeros(2 * m + 1)
    c[ig] = 1.0
    order = [(head - 1 - k) % m for k in range(npairs)]          # newest first
    alpha = {}
    for i in order:
        alpha[i] = _row_dot(m, npairs, c, G, i) / G[i, m + i]
        c[m + i] -= alpha[i]
    if npairs:
        i = order[0]
        c *= G[i, m + i] / G[m + i, m + i]
    for i in reversed(order):
        beta = _row_dot(m, npairs, c, G, m + i) / G[i, m + i]
        c[i] += alpha[i] - beta
    c = -c
    return c, _row_dot(m, npairs, c, G, ig)


def lbfgs(fg, x, maxiters, m=10, c1=1e-4, c2=0.9, max_linesearch=20, g_tol=1e-5, f_reltol=0.0, initial_step=0.0, dtype=np.float64, observe=None):
    def call(th):
        r = fg(th)
        return float(r[0]), np.asarray(r[1], dtype), (float(r[2]) if len(r) > 2 else 1.0)

    def first_t(gg):
        return initial_step if initial_step > 0 else min(1.0, 1.0 / np.sqrt(gg)) if gg > 0 else 1.0

    def combine(c, npairs, g):
        acc = np.zeros(n)
        for j in range(npairs):
            acc += c[j] * S[j].astype(np.float64)
        for j in range(npairs):
            acc += c[m + j] * Y[j].astype(np.float64)
        return (acc + c[ig] * g.astype(np.float64)).astype(dtype)

    def move(x0, t, d):
        return (x0.astype(np.float64) + t * d.astype(np.float64)).astype(dtype)

    n, ig = int(np.size(x)), 2 * m
    theta = np.array(x, dtype)
    S, Y = np.zeros((m, n), dtype), np.zeros((m, n), dtype)
    G = np.zeros((2 * m + 1, 2 * m + 1))
    x0, g0, d = np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    npairs = head = fails = iters = evals = 0
    trace = []

    def sums(g):
        s, y = theta - x0, g - g0
        q = np.zeros(8 + 6 * m)
        q[:8] = [_dot(g, d), _dot(s, y), _dot(y, y), float(np.max(np.abs(g))) if n else 0.0, _dot(g, g), _dot(s, s), _dot(s, g), _dot(y, g)]
        for j in range(npairs):
            for w, H in ((0, S), (1, Y)):
                b = w * m + j
                q[8 + 3 * b: 8 + 3 * b + 3] = [_dot(g, H[j]), _dot(s, H[j]), _dot(y, H[j])]
        return s, y, q

    def seen(q, f, nv, action, t, slot, c):
        if observe is not None:
            observe(dict(sums=q.copy(), f=f, n_valid=nv, action=action, t=t, slot=slot, npairs=npairs, coef=np.array(c, np.float64)))

    # the evaluation at the starting point
    f, g, nv = call(theta)
    evals += 1
    s, y, q = sums(g)
    if not nv > 0:
        seen(q, f, nv, NOOP, 0.0, -1, np.zeros(2 * m + 1))
        return Result(theta, f, evals, trace, "empty batch", 0)
    f0, gg0, ginf = f, q[4], q[3]
    x0, g0 = theta.copy(), g.copy()
    G[ig, ig] = gg0
    status = None
    if not (np.isfinite(f) and np.isfinite(gg0)):
        status = "line search failed"
    elif ginf <= g_tol:
        status = "converged on g"
    if status:
        seen(q, f, nv, ACCEPT_DONE, 0.0, -1, np.zeros(2 * m + 1))
        return Result(theta, f0, evals, trace, status, 0)
    c = np.zeros(2 * m + 1)
    c[ig] = -1.0
    d, dg0, t = combine(c, 0, g0), -gg0, first_t(gg0)
    lo, hi, trials, dec = 0.0, np.inf, 0, ""
    if maxiters <= 0:
        seen(q, f, nv, ACCEPT_PAUSE, t, -1, c)
        return Result(theta, f0, evals, trace, "maxiters", 0)
    seen(q, f, nv, ACCEPT, t, -1, c)
    theta = move(x0, t, d)
    while True:
        f, g, nv = call(theta)
        evals += 1
        s, y, q = sums(g)
        trials += 1
        accept = False
        if not np.isfinite(f) or f > f0 + c1 * t * dg0:
            hi, dec = t, dec + "A"
        elif q[0] < c2 * dg0:
            lo, dec = t, dec + "C"
        else:
            accept = True
        if not accept:
            if trials >= max_linesearch:
                if fails >= 1:
                    seen(q, f, nv, FAIL_DONE, t, -1, np.zeros(2 * m + 1))
                    return Result(x0.copy(), f0, evals, trace, "line search failed", iters)
                fails, npairs, head = 1, 0, 0
                c = np.zeros(2 * m + 1)
                c[ig] = -1.0
                d, dg0, t = combine(c, 0, g0), -gg0, first_t(gg0)
                lo, hi, trials, dec = 0.0, np.inf, 0, ""
                seen(q, f, nv, RESTART, t, -1, c)
            else:
                t = 0.5 * (lo + hi) if np.isfinite(hi) else 2.0 * lo
                seen(q, f, nv, REJECT, t, -1, np.zeros(2 * m + 1))
            theta = move(x0, t, d)
            continue
        iters += 1
        fails = 0
        sy, yy, gg, ginf = q[1], q[2], q[4], q[3]
        trace.append(dict(f=f, t=t, trials=trials, g_inf=ginf, sy=sy, decisions=dec, evaluations=evals))
        status = None
        if ginf <= g_tol:
            status = "converged on g"
        elif f_reltol > 0 and (f0 - f) / max(abs(f0), abs(f), 1.0) <= f_reltol:
            status = "converged on f"
        elif iters >= maxiters:
            status = "maxiters"
        slot, old = -1, npairs
        if sy > 1e-10 * yy:
            slot = head
            for j in range(old):
                if j == slot:
                    continue
                for b in (j, m + j):
                    G[slot, b] = G[b, slot] = q[8 + 3 * b + 1]
                    G[m + slot, b] = G[b, m + slot] = q[8 + 3 * b + 2]
            G[slot, slot], G[m + slot, m + slot] = q[5], yy
            G[slot, m + slot] = G[m + slot, slot] = sy
            S[slot], Y[slot] = s, y
            head, npairs = (head + 1) % m, min(npairs + 1, m)
        for j in range(old):
            if j == slot:
                continue
            for b in (j, m + j):
                G[ig, b] = G[b, ig] = q[8 + 3 * b]
        if slot >= 0:
            G[ig, slot] = G[slot, ig] = q[6]
            G[ig, m + slot] = G[m + slot, ig] = q[7]
        G[ig, ig] = gg
        f0, gg0 = f, gg
        x0, g0 = theta.copy(), g.copy()
        if status and status != "maxiters":
            seen(q, f, nv, ACCEPT_DONE, 1.0, slot, np.zeros(2 * m + 1))
            return Result(theta, f0, evals, trace, status, iters)
        c, dg0 = direction(m, npairs, head, G)
        if not dg0 < 0:
            npairs = head = 0
            slot = -1
            c = np.zeros(2 * m + 1)
            c[ig] = -1.0
            dg0 = -gg
        d = combine(c, npairs, g0)
        t, lo, hi, trials, dec = 1.0, 0.0, np.inf, 0, ""
        if status:
            seen(q, f, nv, ACCEPT_PAUSE, t, slot, c)
            return Result(theta, f0, evals, trace, status, iters)
        seen(q, f, nv, ACCEPT, t, slot, c)
        theta = move(x0, t, d)
