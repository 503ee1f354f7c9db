"""NumPy twin of the optimiser chain (Optimisers.OptimiserChain around one rule), op for op in `dtype`.

    OptimiserChain(o1, ..., on):  dx passes through the stages in order, each seeing the current parameter x; then x <- x - dx
    ClipGrad(delta)               dx <- clamp(dx, -delta, delta)
    ClipNorm(omega, p; throw)     nrm = ||dx||_p over ALL of flat theta; lam = min(omega / nrm, 1), a NaN going through; dx <- dx lam.
                                  throw and a non-finite nrm: Optimisers raises -- the step is not applied (and is counted)
    WeightDecay(lam)              dx <- dx + lam x
    rule                          dx <- the rule's update: oracle/hybrid_oracle.adam_step's arithmetic (Adam, AdamW with couple = true)
                                  and the restatements of RMSProp / Descent in tests/test_gpu_parity.py::test_other_optimiser_rules

Stages are tuples: ("rule",), ("clipgrad", delta), ("clipnorm", omega, p, throw), ("weightdecay", lam) -- what
HybridEngine.opt_init_chain takes.  The rule is opt_init's keyword arguments."""
import numpy as np


def norm_p(t, p, dtype):
    """||t||_p as the chain takes it: the sum in `dtype` (NumPy's pairwise sum), NaN kept by the Inf-norm"""
    a = np.abs(t.astype(dtype))
    if p == 2:
        return dtype(np.sqrt(np.sum(a * a, dtype=dtype)))
    if p == 1:
        return dtype(np.sum(a, dtype=dtype))
    return dtype(np.nan) if np.isnan(a).any() else dtype(a.max() if a.size else 0)


class ChainTwin:
    def __init__(self, n, stages, rule="Adam", lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, dtype=np.float32):
        T = self.T = np.dtype(dtype).type
        self.stages, self.rule = [tuple(s) for s in stages], rule
        self.lr, self.b1, self.b2, self.eps, self.wd = T(lr), T(beta1), T(beta2), T(eps), T(weight_decay)
        self.m, self.v = np.zeros(n, T), np.zeros(n, T)
        self.bt1, self.bt2 = self.b1, self.b2            # running products, started at beta (t = 1)
        self.applied = self.clipped = self.nonfinite = 0
        self.norms = []                                  # the norm of every step that had one (None for a step without valid sample)

    def _rule_dx(self, g):
        T = self.T
        if self.rule in ("Adam", "AdamW"):
            m = self.b1 * self.m + (T(1) - self.b1) * g
            v = self.b2 * self.v + (T(1) - self.b2) * (g * g)
            dx = m / (T(1) - self.bt1) / (np.sqrt(v / (T(1) - self.bt2)) + self.eps) * self.lr
            return dx, m, v
        if self.rule == "RMSProp":                       # RMSProp(eta, rho = beta1, eps)
            v = self.b1 * self.v + (T(1) - self.b1) * (g * g)
            return g * (self.lr / (np.sqrt(v) + self.eps)), self.m, v
        return self.lr * g, self.m, self.v               # Descent(eta)

    def step(self, theta, grad, valid=True):
        """one step on theta (array of dtype) with gradient grad; returns the new theta.  valid = False: a batch without a valid sample"""
        T = self.T
        x = np.asarray(theta, T)
        if not valid:
            self.norms.append(None)
            return x.copy()
        with np.errstate(all="ignore"):
            dx = np.asarray(grad, T).copy()
            m, v = self.m, self.v
            clipped = False
            for st in self.stages:
                if st[0] == "clipgrad":
                    d = T(st[1])
                    dx = np.where(dx < -d, -d, np.where(dx > d, d, dx)).astype(T)      # (a NaN goes through, as Julia's clamp)
                elif st[0] == "weightdecay":
                    dx = dx + T(st[1]) * x
                elif st[0] == "clipnorm":
                    omega, p, thr = T(st[1]), float(st[2]) if len(st) > 2 else 2.0, (st[3] if len(st) > 3 else True)
                    nrm = norm_p(dx, p, T)
                    self.norms.append(float(nrm))
                    if not np.isfinite(nrm):
                        self.nonfinite += 1
                        if thr:
                            return x.copy()
                    r = omega / nrm
                    lam = r if np.isnan(r) else (r if r < T(1) else T(1))
                    clipped = bool(lam < T(1))
                    dx = dx * lam
                elif st[0] == "rule":
                    dx, m, v = self._rule_dx(dx)
                    if self.rule == "AdamW":
                        dx = dx + self.lr * self.wd * x
                else:
                    raise ValueError(st)
            self.m, self.v = m.astype(T), v.astype(T)
            self.bt1, self.bt2 = self.bt1 * self.b1, self.bt2 * self.b2
            self.applied += 1
            self.clipped += int(clipped)
            return (x - dx).astype(T)

    @property
    def status(self):
        return self.applied, self.clipped, self.nonfinite
