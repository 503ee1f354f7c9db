"""Host-side mirror of the reference's training front door.

  train(model, data; nepochs, batchsize, opt, training_loss, loss_types, agg, random_seed, ...)
                                             -- src/training/train.jl:95-136,211-219
  TrainConfig (the fields the step consumes) -- src/config/TrainingConfig.jl:9-160, validate_config :162-185
  DataConfig  (split fields)                 -- src/config/DataConfig.jl:7-59
  prepare_data / split_data                  -- src/data/prepare_data.jl:31-63, src/data/split_data.jl:8-79
  EarlyStopping / best_or_final / TrainResults -- src/training/early_stopping.jl, src/config/TrainingConfig.jl:190-223

The per-minibatch work (`run_epoch!`, src/training/epoch.jl:13-33) and the per-epoch evaluation
(`evaluate_epoch`, :53-66) are calls into the HIP engine; this file is bookkeeping only.
"""
from __future__ import annotations

import copy
import os
import time
import warnings
from dataclasses import dataclass, field, replace
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _lib as L
from .models import SingleNNHybridModel

# ---------------------------------------------------------------------------------------------
# optimiser rule specs (Optimisers.jl constructors; reference re-exports them, EasyHybrid.jl:59)
# ---------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class Adam:
    eta: float = 0.001
    beta: tuple = (0.9, 0.999)
    epsilon: float = 1e-8


@dataclass(frozen=True)
class AdamW:
    eta: float = 0.001
    beta: tuple = (0.9, 0.999)
    lambda_: float = 0.0
    epsilon: float = 1e-8


@dataclass(frozen=True)
class RMSProp:
    eta: float = 0.001
    rho: float = 0.9
    epsilon: float = 1e-8


@dataclass(frozen=True)
class Descent:
    eta: float = 0.1


@dataclass(frozen=True)
class ClipGrad:                       # dx <- clamp(dx, -delta, delta)
    delta: float = 10.0


@dataclass(frozen=True)
class ClipNorm:                       # dx <- dx * min(omega / norm(dx, p), 1), the norm over all of flat theta; throw: a non-finite norm is an error
    omega: float = 10.0
    p: float = 2.0
    throw: bool = True


@dataclass(frozen=True)
class WeightDecay:                    # dx <- dx + lambda * x (no learning rate in it)
    lambda_: float = 5e-4


@dataclass(frozen=True)
class LBFGS:
    """L-BFGS through the reference's Optimization.jl driver (src/training/train_optimization.jl): history m, weak-Wolfe bisection line
    search (sufficient decrease c1, curvature c2, at most max_linesearch trials per iteration); initial_step 0 = min(1, 1 / ||g||) on
    the first iteration.  Runs on the device; see TrainConfig.full_batch / eval_every / inner_maxiters."""
    m: int = 10
    c1: float = 1e-4
    c2: float = 0.9
    max_linesearch: int = 20
    initial_step: float = 0.0


@dataclass(frozen=True, init=False)
class OptimiserChain:
    """OptimiserChain(o1, ..., on): the gradient passes through the stages in order, each seeing the current parameter, then
    x <- x - dx.  On the device: exactly one rule, ClipGrad / WeightDecay stages on either side of it, at most one ClipNorm
    (p = 1, 2 or Inf) in front of it, at most 8 stages; nested chains flatten."""
    opts: tuple = ()

    def __init__(self, *opts):
        object.__setattr__(self, "opts", tuple(opts))


def _chain_args(chain):
    """OptimiserChain -> opt_init_chain's keyword arguments (stages + the rule's), or the reason why the device does not run it"""
    flat = []

    def walk(c):
        for o in c.opts:
            if isinstance(o, OptimiserChain):
                walk(o)
            else:
                flat.append(o)
    walk(chain)
    stages, rule, have_norm = [], None, False
    for o in flat:
        if isinstance(o, _RULES):
            if rule is not None:
                raise NotImplementedError(f"OptimiserChain: a second rule {o!r} -- a chain on the device holds exactly one of Adam/AdamW/RMSProp/Descent")
            rule = _opt_args(o)
            stages.append(("rule",))
        elif isinstance(o, ClipGrad):
            if not o.delta >= 0:
                raise ValueError(f"{o!r}: delta must not be negative")
            stages.append(("clipgrad", float(o.delta)))
        elif isinstance(o, WeightDecay):
            if not o.lambda_ >= 0:
                raise ValueError(f"{o!r}: lambda must not be negative")
            stages.append(("weightdecay", float(o.lambda_)))
        elif isinstance(o, ClipNorm):
            if not o.omega > 0:
                raise ValueError(f"{o!r}: omega must be positive")
            if float(o.p) not in (1.0, 2.0, float("inf")):
                raise NotImplementedError(f"{o!r}: the device computes the 1-, 2- and Inf-norm")
            if have_norm:
                raise NotImplementedError("OptimiserChain: a second ClipNorm -- one norm pass per step is built")
            if rule is not None:
                raise NotImplementedError("OptimiserChain: ClipNorm behind the rule needs the norm of the update, a second pass over it: not built "
                                          "(put it in front of the rule)")
            have_norm = True
            stages.append(("clipnorm", float(o.omega), float(o.p), bool(o.throw)))
        elif isinstance(o, LBFGS):
            raise NotImplementedError("OptimiserChain: LBFGS is not an Optimisers.jl rule -- it takes the Optimization.jl driver and its own line search, "
                                      "and cannot be a stage of a chain (pass opt = LBFGS() on its own)")
        else:
            raise NotImplementedError(f"OptimiserChain stage {o!r}: ClipGrad, ClipNorm, WeightDecay and one Adam/AdamW/RMSProp/Descent rule run on the device")
    if rule is None:
        raise NotImplementedError("OptimiserChain without a rule: a chain on the device holds exactly one of Adam/AdamW/RMSProp/Descent")
    if len(stages) > L.EH_MAX_OPT_STAGES:
        raise NotImplementedError(f"OptimiserChain: {len(stages)} stages, the device keeps at most {L.EH_MAX_OPT_STAGES}")
    return dict(rule, stages=stages)


def _opt_args(opt):
    if isinstance(opt, OptimiserChain):
        return _chain_args(opt)
    if isinstance(opt, Adam):
        return dict(rule="Adam", lr=opt.eta, beta1=opt.beta[0], beta2=opt.beta[1], eps=opt.epsilon)
    if isinstance(opt, AdamW):
        return dict(rule="AdamW", lr=opt.eta, beta1=opt.beta[0], beta2=opt.beta[1], eps=opt.epsilon, weight_decay=opt.lambda_)
    if isinstance(opt, RMSProp):
        return dict(rule="RMSProp", lr=opt.eta, beta1=opt.rho, eps=opt.epsilon)
    if isinstance(opt, Descent):
        return dict(rule="Descent", lr=opt.eta)
    if isinstance(opt, LBFGS):
        raise NotImplementedError("LBFGS is not an Optimisers.jl rule: train(opt = LBFGS()) takes the Optimization.jl driver on the device; "
                                  "it cannot be handed to opt_init")
    raise NotImplementedError(f"optimiser {opt!r}: Optimisers.jl-style Adam/AdamW/RMSProp/Descent and, of the Optimization.jl path "
                              "(src/training/train_optimization.jl), LBFGS run on the device")


_RULES = (Adam, AdamW, RMSProp, Descent)
_DEFAULT_BRANCH_RULE = Adam(0.001, (0.9, 0.999), 1e-8)          # build_opt_state's default_rule = Optimisers.Adam() (train.jl:78)


def _rule_key(a):
    """the rule as eh_opt_init receives it (float32 hyper-parameters, the engine's defaults filled in): equal keys, equal bits"""
    f = lambda x: float(np.float32(x))
    return (a["rule"], f(a["lr"]), f(a.get("beta1", 0.9)), f(a.get("beta2", 0.999)), f(a.get("eps", 1e-8)), f(a.get("weight_decay", 0.0)))


def _opt_groups(opt, model):
    """TrainConfig.opt -> (group, rules): one rule (group None, rules [its eh_opt_init arguments]) or a rule per top-level branch of
    the parameter tree (build_opt_state, src/training/train.jl:78-93): group[i] = the rule of flat-theta element i, branches with the
    same rule merged.  `opt` is a rule, or a dict / NamedTuple of branch name -> rule; branches it leaves out take Adam()."""
    if isinstance(opt, _RULES):
        return None, [_opt_args(opt)]
    if isinstance(opt, tuple) and hasattr(opt, "_asdict"):
        opt = opt._asdict()
    if not isinstance(opt, dict):
        return None, [_opt_args(opt)]                                 # (raises NotImplementedError)
    for k, r in opt.items():
        if isinstance(r, OptimiserChain):
            raise NotImplementedError(f"per-branch optimiser {k!r}: an OptimiserChain per branch is not built (Optimisers applies it per leaf array "
                                      "there, so ClipNorm's norm would be per layer matrix); one chain for the whole model is")
        if isinstance(r, LBFGS):
            raise NotImplementedError(f"per-branch optimiser {k!r}: LBFGS works on the whole parameter vector (one line search, one history): "
                                      "not built as a per-branch rule")
        if not isinstance(r, _RULES):
            raise NotImplementedError(f"per-branch optimiser {k!r}: {r!r} -- only Adam/AdamW/RMSProp/Descent rules run on the device "
                                      "(pre-built Optimisers.setup state trees are not supported)")
    branches = model.opt_branches()
    extra = [k for k in opt if k not in branches]
    if extra:
        warnings.warn("Per-branch optimizer keys not found in parameter tree, ignored: [" + ", ".join(":" + str(k) for k in extra) + "]")
    keys, rules = [], []
    group = np.zeros(model.n_theta, np.uint8)
    for name, (lo, hi) in branches.items():
        if hi == lo:
            continue                                                  # (an empty branch: no element follows its rule)
        a = _opt_args(opt.get(name, _DEFAULT_BRANCH_RULE))
        k = _rule_key(a)
        if k not in keys:
            keys.append(k); rules.append(a)
        group[lo:hi] = keys.index(k)
    if len(rules) > L.EH_MAX_OPT_GROUPS:
        raise NotImplementedError(f"per-branch optimiser: {len(rules)} distinct rules, the device keeps at most {L.EH_MAX_OPT_GROUPS}")
    if len(rules) <= 1:
        return None, rules or [_opt_args(_DEFAULT_BRANCH_RULE)]
    return group, rules


def _opt_setup(eng, opt, model):
    group, rules = _opt_groups(opt, model)
    if group is None and "stages" in rules[0]:
        eng.opt_init_chain(**rules[0])
    elif group is None:
        eng.opt_init(**rules[0])
    else:
        eng.opt_init_groups(group, rules)


# ---------------------------------------------------------------------------------------------
# configs
# ---------------------------------------------------------------------------------------------

_MAXIMIZE = {"pearson", "r2", "nse", "kge"}                      # loss_fn.jl:181-187
_DEVICE_METRICS = {"mse", "rmse", "mae", "r2", "nse", "pearson", "kge", "pbkge"}


def isbetter(new, best, loss_type) -> bool:                      # loss_fn.jl:189-194
    return new > best if loss_type in _MAXIMIZE else new < best


def check_training_loss(loss_type):                              # loss_fn.jl:196-205
    if loss_type in _MAXIMIZE:
        raise ValueError(f"Got a metric that is defined as `to be maximized` as a training loss: {loss_type}. "
                         "For training you must use a true loss (to be minimized), e.g. :mse.")


@dataclass
class WeightL2:
    """One term of extra_loss = (yhat, ps) -> (; name = lam * weight_l2(ps; key, normalize), ...) (src/utils/extract_weights.jl:
    64-91) -- the extra losses the device knows: functions of the parameters that are sums of squares of Dense leaves.
    net: the network of a MultiNNHybridModel the walk starts at (`weight_l2(ps.Rb; ...)`, the reference's own example), None =
    the whole tree; key: "weight" (default) or "bias".  TrainConfig.extra_loss takes one term, a list of terms or a dict
    name -> term (the NamedTuple the closure returns).  Closures of yhat cannot run inside the kernel."""
    lam: float
    normalize: bool = False
    net: Optional[str] = None
    key: str = "weight"
    name: Optional[str] = None

    def label(self) -> str:
        return self.name or ("weight_l2" if self.net is None and self.key == "weight" else f"l2_{self.net or self.key}")


def _extra_fn(extra_loss):
    """TrainConfig.extra_loss -> the function of the predictions in it (`extra_loss(yhat[, ps])`, compute_loss.jl:31-34), or None.
    It may stand alone or in a list next to WeightL2 terms; it is recorded (program.trace_extra_loss) when the engine is created."""
    if callable(extra_loss) and not isinstance(extra_loss, WeightL2):
        return extra_loss
    if isinstance(extra_loss, (list, tuple)):
        fns = [v for v in extra_loss if callable(v) and not isinstance(v, WeightL2)]
        if len(fns) > 1:
            raise ValueError("extra_loss: one function of the predictions (it may return several entries)")
        return fns[0] if fns else None
    return None


def _extra_terms(extra_loss) -> List[WeightL2]:
    """TrainConfig.extra_loss -> its WeightL2 terms ([] for None; a function of the predictions is _extra_fn's); anything else is refused"""
    if extra_loss is None:
        return []
    if callable(extra_loss) and not isinstance(extra_loss, WeightL2):
        return []
    if isinstance(extra_loss, (list, tuple)) and any(callable(v) and not isinstance(v, WeightL2) for v in extra_loss):
        extra_loss = [v for v in extra_loss if isinstance(v, WeightL2)]
        if not extra_loss:
            return []
    if isinstance(extra_loss, WeightL2):
        return [extra_loss]
    if isinstance(extra_loss, dict) and extra_loss and all(isinstance(v, WeightL2) for v in extra_loss.values()):
        return [WeightL2(v.lam, v.normalize, v.net, v.key, str(k)) for k, v in extra_loss.items()]
    if isinstance(extra_loss, (list, tuple)) and extra_loss and all(isinstance(v, WeightL2) for v in extra_loss):
        terms = list(extra_loss)
        if len({t.label() for t in terms}) != len(terms):
            raise ValueError("extra_loss: two terms with the same name (a NamedTuple has distinct fields): give them `name`s")
        return terms
    raise NotImplementedError("extra_loss: WeightL2 terms (one, a list or a dict of them) and / or ONE function of the predictions "
                              "`f(yhat[, ps])` returning np.sum(...) / np.mean(...) entries are built")


def _apply_extra_loss(eng, model, terms: List[WeightL2], agg: str = "sum", n_fn_entries: int = 0):
    """the extra loss terms and `agg` (TrainingConfig.jl:76-77): the training loss is agg([agg(per-target losses), extra entries...])
    (compute_loss.jl:31-34,50-53) -- the engine needs the number of extra entries for agg = mean"""
    if len(terms) == 1 and terms[0].net is None and terms[0].key == "weight":
        eng.set_weight_l2(terms[0].lam, terms[0].normalize)
    elif terms:
        eng.set_weight_l2_coef(model.l2_coefficients(terms))
    eng.set_agg(agg, len(terms) + n_fn_entries)          # (entries of a function of the predictions ride on targets of their own: engine(extra_fn=...))


def _agg_name(agg) -> str:
    """TrainConfig.agg -> "sum" / "mean" (the two the device implements); the functions themselves are accepted like the reference's
    `agg::Function` (sum, np.sum, np.mean, statistics.mean)"""
    name = agg if isinstance(agg, str) else getattr(agg, "__name__", None)
    if name in ("sum", "nansum", "fsum"):
        return "sum"
    if name in ("mean", "nanmean", "fmean", "average"):
        return "mean"
    raise NotImplementedError(f"agg {agg!r}: the device implements sum and mean (TrainingConfig.jl:76-77)")


def _extra_loss_values(model, theta, terms: List[WeightL2], agg: str = "sum", fn=None, preds=None) -> Dict[str, float]:
    """the extra losses of flat parameters `theta` -- and, fn / preds, of the predictions of one split -- (host side, for the history;
    compute_loss.jl:39-44: each entry and their agg)"""
    th = np.asarray(theta, np.float64)
    out = {}
    if fn is not None and preds is not None:
        import inspect
        try:
            two = len([p for p in inspect.signature(fn).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) and p.default is p.empty]) >= 2
        except (TypeError, ValueError):
            two = False
        class _Ps:                                    # `ps` as the function sees it in the reference: the global parameters' raw one-element vectors
            def __init__(self, glob): self._g = glob
            def __getattr__(self, k):
                if k.startswith("_") or k not in self._g:
                    raise AttributeError(k)
                return np.asarray(self._g[k], np.float64)
            def __getitem__(self, k): return np.asarray(self._g[k], np.float64)
        res = fn(preds, _Ps(model.unpack(np.asarray(theta, np.float32))[1])) if two else fn(preds)
        if hasattr(res, "_asdict"):
            res = res._asdict()
        items = res.items() if isinstance(res, dict) else [(f"extra_{i + 1}", v) for i, v in enumerate(res if isinstance(res, (list, tuple)) else [res])]
        for k, v in items:
            out[str(k)] = float(v)
    for t in terms:
        m = model.l2_mask(t.net, t.key)
        sq = float(np.sum(th[m] * th[m]))
        out[t.label()] = float(t.lam) * (sq / max(1, int(m.sum())) if t.normalize else sq)
    vals = list(out.values())
    out[agg] = float(sum(vals) / len(vals)) if (agg == "mean" and vals) else float(sum(vals))      # (; extra_loss_values..., Symbol(agg) => agg(...)), compute_loss.jl:42-44
    return out


@dataclass
class TrainConfig:
    nepochs: int = 200
    batchsize: int = 64
    opt: Any = field(default_factory=lambda: Adam(0.01))
    patience: int = 2**62
    training_loss: Any = "mse"           # a name, or a function f(yhat, y) -> np.mean(per-sample terms) (loss_fn.jl: training_loss::Function)
    loss_types: List[str] = field(default_factory=lambda: ["mse", "r2"])
    agg: Any = "sum"                     # TrainingConfig.jl:76-77 `agg::Function`: "sum" / "mean" (or the functions themselves)
    extra_loss: Any = None               # TrainingConfig.jl:74; None, a WeightL2 term, or a list / dict (name -> term) of them
    train_from: Any = None
    random_seed: Optional[int] = 161803
    return_model: str = "best"
    keep_history: bool = True
    show_progress: bool = False
    device: int = 0
    # not in the reference (it has no multi-GPU path): None = data parallel iff torch.distributed is initialised with
    # more than one rank; True / False force it.  `batchsize` stays the GLOBAL minibatch, split evenly over the ranks.
    distributed: Optional[bool] = None
    # not in the reference -- how the device runs the step (DESIGN.md sections 3.8 and 6):
    #   specialize   "auto" (default): step kernels compiled at run time (hiprtc) with this model's descriptor as a compile-time
    #                constant -- before the first step when `random_seed` is set (a reproducible run: about a second the first time, instant
    #                from the disk cache), in a background thread otherwise (training starts on the kernels built ahead of time and
    #                switches when the compiled one is ready; the two binaries agree to ~1e-6, not bit for bit).  True: compile before the
    #                first step.  False: only the kernels built ahead of time.  Every compiled kernel is checked against the one built
    #                ahead of time on the first batch before it takes over (eh_jit_status says when it was refused).
    #   fused_update "auto" (default): one kernel per step where the model allows it (single target, per-wave kernel family, no
    #                weight_l2 / moment-based loss) -- the optimiser update of a step runs in the prologue of the next one and the
    #                partial sums meet through float atomics, reproducible to ~1e-7, not bitwise.  A run with `random_seed` set -- the
    #                default, as in the reference (TrainingConfig.jl:85-86), where a seeded CPU run IS reproducible -- takes that form
    #                only where it is bitwise reproducible: minibatches one workgroup covers (up to 256 samples: several steps per
    #                launch, sums in one fixed order); larger minibatches run the deterministic step + reduce/optimiser pair (14.6
    #                against 10.2 us per step at batch 65 536 on the headline model, tools/bench_step_modes.py: `random_seed=None` or
    #                `fused_update=True` buys the difference back).  False: always the deterministic pair.  True: insist on one kernel
    #                per step (raises where it is not built).  (An ORDERED one-kernel form -- fixed-point sums, integer atomics -- was
    #                built and measured in round 6: 13.9 us, and 0.6 us on the float form it shared the kernel with; removed.)
    # bench.py measures specialize on and the reproducible form (fused_update = 2, what "auto" takes when seeded) at the engine;
    # with --full also fused_update = True.
    specialize: Any = "auto"
    fused_update: Any = "auto"
    # not in the reference: "lazy" (default) = the observed-vs-predicted tables and the physical parameters of the returned model
    # (TrainResults.train_obs_pred / val_obs_pred / train_diffs / val_diffs, train.jl:130-136) are computed when they are first read --
    # the engine stays resident until then (or until the results are dropped / TrainResults.release()); "eager" = before train() returns,
    # as the reference does.  Same values either way.  (An engine the caller passed in is never kept: eager.)
    predictions: str = "lazy"
    # not in the reference: True = TrainResults.timing splits the wall-clock of the epoch loop into training steps / evaluation passes /
    # host bookkeeping (one extra device synchronisation per epoch, after the steps, so that the split is clean: bench.py `train_e2e`)
    timing: bool = False
    # the Optimization.jl driver only (opt = LBFGS(); TrainingConfig.jl:127-159):
    #   full_batch      True: one solve over the whole training split (solve keywords maxiters, g_tol, f_reltol), a train / validation
    #                   snapshot every `eval_every` accepted iterations; False: `nepochs` passes over the shuffled minibatches, a fresh solve
    #                   of `inner_maxiters` iterations on each, warm-started from the current parameters, one snapshot per pass
    #   promote_f64     accepted with a warning: the parameters stay fp32 on the device, the recurrences are in double already
    full_batch: bool = False
    promote_f64: bool = False
    eval_every: int = 1
    inner_maxiters: int = 4


_SOLVE_KEYWORDS = ("maxiters", "epochs", "g_tol", "f_reltol")          # what train() hands on to the solve (the reference: solve(...; kwargs...))


@dataclass
class DataConfig:
    shuffleobs: bool = False
    split_by_id: Any = None
    split_data_at: float = 0.8
    folds: Any = None
    val_fold: Optional[int] = None
    # sequence models (split_data.jl:28): dict(input_window = 10, output_window = 1, output_shift = 1, lead_time = 1) or a part of it; the
    # series is cut into windows, the windows are filtered (filter_sequences) and THEY are split into training and validation
    sequence_kwargs: Optional[dict] = None


def _apply_step_mode(eng, tc: "TrainConfig", seq: bool = False):
    """TrainConfig.specialize / fused_update -> engine options (single-GPU training)"""
    if tc.fused_update not in (True, False, "auto") or tc.specialize not in (True, False, "auto"):
        raise ValueError("specialize / fused_update must be True, False or 'auto'")
    if getattr(eng, "has_chain", False):      # an optimiser chain: step kernel + reduction + chain kernels (the norm needs the whole gradient first)
        if tc.fused_update is True:
            raise NotImplementedError("fused_update=True: the one-kernel step is not built for an OptimiserChain (ClipNorm needs the norm of the whole "
                                      "gradient before any element moves); 'auto' and False run the step + reduce + chain kernels")
        if not seq:
            eng.set_option("fused_update", 0)
            eng.set_option("specialize", (1 if tc.random_seed is not None else 2) if tc.specialize == "auto" else int(bool(tc.specialize)))
        elif tc.specialize is True:
            eng.set_option("specialize", 1)
        return
    if seq:      # sequence models always run the reproducible step + reduce pair on the one kernel family: "auto" is that; True is refused by the engine
        if tc.fused_update is True:
            eng.set_option("fused_update", 1)
        if tc.specialize is True:
            eng.set_option("specialize", 1)
        return
    if tc.fused_update is not False:
        try:
            # "auto" in a seeded run: one kernel per step only where that is bitwise reproducible (engine option value 2: minibatches one
            # workgroup covers), the deterministic pair elsewhere -- two default train(random_seed = s) calls are the same bits
            # "auto" in a seeded run: one kernel per step only where that is bitwise reproducible (engine option value 2: minibatches one
            # workgroup covers), the deterministic pair elsewhere -- two default train(random_seed = s) calls are the same bits
            eng.set_option("fused_update", 2 if (tc.fused_update == "auto" and tc.random_seed is not None) else 1)
        except (NotImplementedError, RuntimeError):
            if tc.fused_update is True:
                raise
    # "auto": a run that asked for reproducibility (random_seed set -- the default, TrainingConfig.jl:86) compiles BEFORE the first step
    # (about a second the first time, instant from the disk cache): the background build would switch binaries at a timing-dependent step,
    # and the two agree to ~1e-6, not bit for bit (advisor, round 3).  Without a seed the build runs in the background.
    eng.set_option("specialize", (1 if tc.random_seed is not None else 2) if tc.specialize == "auto" else int(bool(tc.specialize)))


def validate_config(cfg: TrainConfig):                           # TrainingConfig.jl:162-185
    if cfg.nepochs < 0:
        raise ValueError("nepochs must be >= 0")
    if cfg.batchsize < 1:
        raise ValueError("batchsize must be >= 1")
    if cfg.return_model not in ("best", "final"):
        raise ValueError("return_model must be :best or :final")
    if not cfg.loss_types:
        raise ValueError("loss_types must not be empty")
    from .engine import PerTarget
    tl = cfg.training_loss
    per_target = tl.losses if isinstance(tl, PerTarget) else (tl if isinstance(tl, (list, tuple)) and tl and not callable(tl[0]) else None)
    if per_target is not None:                                   # PerTarget((l_1, ..., l_T)), compute_loss.jl:128-145
        for lt in per_target:
            if callable(lt) or (isinstance(lt, (list, tuple)) and lt and callable(lt[0])):      # a function, or (f, args) / (f, kwargs): recorded and compiled into the step kernel
                continue
            check_training_loss(lt)
            if lt not in L.TRAINING_LOSSES:
                raise NotImplementedError(f"training_loss {lt!r}: the device implements {sorted(L.TRAINING_LOSSES)}")
    elif not callable(tl) and not (isinstance(tl, (list, tuple)) and tl and callable(tl[0])):      # a function (or (f, args), (f, kwargs): loss_fn.jl:92-107) is recorded and compiled into the step kernel
        check_training_loss(cfg.training_loss)
        if cfg.training_loss not in L.TRAINING_LOSSES:
            raise NotImplementedError(f"training_loss {cfg.training_loss!r}: the fused kernel implements {sorted(L.TRAINING_LOSSES)} "
                                      "or a function f(yhat, y) = mean of per-sample terms")
    _agg_name(cfg.agg)                    # sum or mean
    _extra_terms(cfg.extra_loss)          # (refuses what the device cannot run)
    for lt in cfg.loss_types:
        if lt not in _DEVICE_METRICS:
            raise NotImplementedError(f"loss type {lt!r} is not computed by the eval kernel (have {sorted(_DEVICE_METRICS)})")


# ---------------------------------------------------------------------------------------------
# data preparation (host; runs once)
# ---------------------------------------------------------------------------------------------


def _columns(data) -> Dict[str, np.ndarray]:
    if hasattr(data, "columns") and hasattr(data, "__getitem__") and not isinstance(data, dict):   # pandas DataFrame
        return {str(c): np.asarray(data[c]) for c in data.columns}
    if isinstance(data, dict):
        return {k: np.asarray(v) for k, v in data.items()}
    raise TypeError("data must be a dict of columns, a pandas DataFrame or a prepared ((X, forcings), targets) tuple")


def prepare_data(model: SingleNNHybridModel, data, drop_missing_rows: bool = True):
    """-> ((X (P,N) float32, {forcing: (N,)}), {target: (N,)}); prepare_data.jl:31-63."""
    if isinstance(data, tuple):
        return data
    cols = _columns(data)
    need = list(dict.fromkeys(list(model.predictors) + list(model.forcing) + list(model.targets)))
    for c in need:
        if c not in cols:
            raise KeyError(f"column {c!r} missing from data")
    # (float32 / float64 columns stay what they are -- the device data are Float32 like the reference's, prepare_data.jl:58-60 -- anything
    #  else goes through float64; no copy is made where none is needed: at 4 M rows the copies ARE the cost of this function)
    arr = {c: (a if (a := np.asarray(cols[c])).dtype in (np.float32, np.float64) else a.astype(np.float64)) for c in need}
    n = len(next(iter(arr.values())))
    if drop_missing_rows:
        predforce = [c for c in need if c not in model.targets]
        miss = np.zeros(n, bool)
        for c in predforce:
            miss |= np.isnan(arr[c])
        some_target = np.zeros(n, bool)
        for c in model.targets:
            some_target |= ~np.isnan(arr[c])
        keep = ~miss & some_target
        if not keep.all():
            arr = {c: v[keep] for c, v in arr.items()}
    nkept = len(next(iter(arr.values())))
    if model.predictors:
        X = np.empty((len(model.predictors), nkept), np.float32)
        for i, p_ in enumerate(model.predictors):
            X[i] = arr[p_]                                        # (one pass per column, cast on the way)
    else:
        X = np.zeros((0, nkept), np.float32)                      # (no predictors: a model without a network)
    return (X, {f: arr[f].astype(np.float32, copy=False) for f in model.forcing}), {t: arr[t].astype(np.float32, copy=False) for t in model.targets}


def _no_nan(a) -> bool:
    """no NaN in `a`, found by ONE reduction pass without a temporary: a NaN anywhere makes the sum NaN (so does inf - inf: then the exact
    test decides).  np.isnan(a) | ... over 4 M rows allocates and walks a boolean array per column -- a third of a short train() call."""
    return not bool(np.isnan(np.add.reduce(a))) or not bool(np.isnan(a).any())


def _column_views(model, data, cfg: DataConfig):
    """the caller's table as float32 column views, if the common case applies (see _split_columns) -> (columns, names, rows) or None"""
    if isinstance(data, tuple) or cfg.shuffleobs or cfg.split_by_id is not None or cfg.folds is not None or cfg.val_fold is not None:
        return None
    cols = _columns(data)
    need = list(dict.fromkeys(list(model.predictors) + list(model.forcing) + list(model.targets)))
    arr = {}
    for c in need:
        if c not in cols:
            raise KeyError(f"column {c!r} missing from data")
        a = np.asarray(cols[c])
        if a.dtype != np.float32 or a.ndim != 1 or not a.flags.c_contiguous:
            return None
        arr[c] = a
    if not model.predictors:
        return None
    n = len(next(iter(arr.values())))
    if any(len(a) != n for a in arr.values()) or n == 0:
        return None
    return arr, need, n


def _no_row_to_drop(model, arr, need, n) -> bool:
    """prepare_data.jl:31-63 keeps a row whose predictors and forcings are all there and that has some target: true if that is every row"""
    if n >= (1 << 20) and len(need) > 1:                              # (the reductions release the interpreter lock: one thread per column)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(4, len(need))) as ex:
            clean = dict(zip(need, ex.map(_no_nan, [arr[c] for c in need])))
    else:
        clean = {c: _no_nan(arr[c]) for c in need}
    if not all(clean[c] for c in need if c not in model.targets):
        return False                                                  # rows to drop: the general path
    if len(model.targets) == 1:
        if not clean[model.targets[0]]:
            return False                                              # (a row without its only target is dropped)
    elif not any(clean[t] for t in model.targets):
        some = np.zeros(n, bool)
        for t in model.targets:
            some |= ~np.isnan(arr[t])
        if not some.all():
            return False
    return True


def _take_views(model, arr, cfg: DataConfig, n):
    k = int(np.clip(round(cfg.split_data_at * n), 0, n))             # MLUtils.splitobs(at = ...)

    def take(sl):
        return ([arr[p][sl] for p in model.predictors], {f: arr[f][sl] for f in model.forcing}), {t: arr[t][sl] for t in model.targets}
    return take(slice(0, k)), take(slice(k, n))


def _split_columns(model, data, cfg: DataConfig):
    """The common case of train(model, table; ...) without copying the table: float columns, the contiguous split of MLUtils.splitobs
    (no shuffleobs / split_by_id / folds), no row to drop (prepare_data.jl:31-63 keeps a row whose predictors and forcings are all there and
    that has some target) -> (train, val), each ((predictor rows: list of (N,) views), {forcing: view}), {target: view}); None = take the
    general path (prepare_data + split_data: same result, through copies)."""
    cv = _column_views(model, data, cfg)
    if cv is None or not _no_row_to_drop(model, *cv):
        return None
    return _take_views(model, cv[0], cfg, cv[2])


class _EarlyUpload:
    """train() on a large table: the engine is created and both splits are uploaded by a worker thread WHILE the columns are screened for
    rows to drop (1.6 ms of a 16 ms call on the 4 M-row headline data set -- the screen only decides whether the views may be used as they
    are; the upload's staged copies release the interpreter lock).  If the screen says no, the engine is closed and the general path runs."""
    def __init__(self, model, device, xfn, views):
        import threading
        self.engine, self.error, self.engine_s, self.upload_s = None, None, 0.0, 0.0
        (xtr, ftr, ytr), (xva, fva, yva) = [(a[0][0], a[0][1], a[1]) for a in views]

        def work():
            try:
                t0 = time.perf_counter()
                eng = model.engine(device, extra_fn=xfn)
                self.engine = eng
                t1 = time.perf_counter()
                eng.set_data(L.EH_SPLIT_TRAIN, xtr, [ftr[f] for f in model.forcing], [ytr[t] for t in model.targets])
                eng.set_data(L.EH_SPLIT_VAL, xva, [fva[f] for f in model.forcing], [yva[t] for t in model.targets])
                self.engine_s, self.upload_s = t1 - t0, time.perf_counter() - t1
            except BaseException as e:                  # (re-raised by the caller's thread)
                self.error = e
        self._t = threading.Thread(target=work, name="eh-early-upload")
        self._t.start()

    def join(self, keep: bool):
        self._t.join()
        if self.error is not None or not keep:
            if self.engine is not None:
                self.engine.close()
            if self.error is not None:
                raise self.error
            return None
        return self.engine


SEQUENCE_DEFAULTS = dict(input_window=10, output_window=1, output_shift=1, lead_time=1)      # split_data.jl:28


SEQUENCE_LOSSES = ("mse", "mae", "nseLoss")      # what a sequence model trains on, per target (one target: rmse as well)


def _sequence_loss_check(tl, n_targets: int):
    """training_loss of a sequence model -- one kind, or PerTarget((l_1, ..., l_T)) -- against the losses its step kernel has: the others
    are refused here, with the reason, before an engine is made"""
    from .engine import PerTarget
    kinds = list(tl.losses) if isinstance(tl, PerTarget) else (list(tl) if isinstance(tl, (list, tuple)) and tl and not callable(tl[0]) else [tl])
    for k in kinds:
        if callable(k) or (isinstance(k, (list, tuple)) and k and callable(k[0])):
            raise NotImplementedError(f"sequence models: a function as training loss is a recorded loss, which is not built for them (have {list(SEQUENCE_LOSSES)})")
        if k == "rmse" and n_targets == 1 and len(kinds) == 1:
            continue
        if k == "rmse":
            raise NotImplementedError(f"sequence models: training loss 'rmse' on {n_targets} targets needs a pass ahead of the step (its scale cannot be applied "
                                      f"after it), which is not built for them (have {list(SEQUENCE_LOSSES)})")
        if k not in SEQUENCE_LOSSES:
            raise NotImplementedError(f"sequence models: training loss {k!r} needs the batch moments of the predictions (two passes), which is not built for them "
                                      f"(have {list(SEQUENCE_LOSSES)})")


def _sequence_splits(model, data, cfg: DataConfig, rng: Optional[np.random.Generator] = None):
    """sequence models (split_data.jl:26-78): the whole series (no row is dropped), its windows filtered, and the surviving WINDOWS split
    by split_data_at / shuffleobs -> ((X, forcings), targets), train windows, validation windows.  Both splits index the same series."""
    from .sequences import Sequences, filter_sequences, split_into_sequences
    kw = dict(SEQUENCE_DEFAULTS)
    unknown = set(cfg.sequence_kwargs or {}) - set(kw)
    if unknown:
        raise TypeError(f"sequence_kwargs: unknown keys {sorted(unknown)} (have {sorted(kw)})")
    kw.update(cfg.sequence_kwargs or {})
    if cfg.split_by_id is not None or cfg.folds is not None or cfg.val_fold is not None:
        raise NotImplementedError("sequence models: split_by_id / folds are not built (windows are split by split_data_at / shuffleobs)")
    (X, forc), targ = prepare_data(model, data, drop_missing_rows=False)
    seq = filter_sequences(split_into_sequences(X, np.stack([targ[t] for t in model.targets]), **kw))
    n = len(seq.starts)
    k = int(np.clip(round(cfg.split_data_at * n), 0, n))               # MLUtils.splitobs(at = ...)
    idx = (rng or np.random.default_rng()).permutation(n) if cfg.shuffleobs else np.arange(n)

    def pick(ix):
        return Sequences(seq.starts[ix], seq.x[:, :, ix], seq.y[:, :, ix], seq.input_window, seq.output_window, seq.lead_time)
    return ((X, forc), targ), pick(idx[:k]), pick(idx[k:])


def _split_rows(cfg: DataConfig, n: int, raw_cols, rng: Optional[np.random.Generator] = None):
    """which of the n screened rows (prepare_data) train and which validate, each an index array or a slice: split_data.jl:8-79.  One
    copy of the rules for split_data and for train_members, which hands the rows to the device as lists instead of gathering them."""
    if cfg.split_by_id is not None and cfg.folds is not None:
        raise ValueError("split_by_id and folds are not supported together; do the split when constructing folds")
    if cfg.split_by_id is not None:
        ids = np.asarray(raw_cols[cfg.split_by_id] if isinstance(cfg.split_by_id, str) else cfg.split_by_id)
        if len(ids) != n:
            raise ValueError("split_by_id needs one id per retained sample (drop NaN rows first)")
        uniq = np.array(list(dict.fromkeys(ids.tolist())))
        if cfg.shuffleobs:
            uniq = (rng or np.random.default_rng()).permutation(uniq)
        k = int(np.clip(round(cfg.split_data_at * len(uniq)), 0, len(uniq)))
        tr = np.flatnonzero(np.isin(ids, uniq[:k])); va = np.flatnonzero(np.isin(ids, uniq[k:]))
    elif cfg.folds is not None or cfg.val_fold is not None:
        if cfg.folds is None or cfg.val_fold is None:
            raise AssertionError("Provide folds together with val_fold.")
        f = np.asarray(raw_cols[cfg.folds] if isinstance(cfg.folds, str) else cfg.folds)
        if len(f) != n:
            raise AssertionError(f"length(folds) ({len(f)}) must equal number of samples ({n}).")
        va = np.flatnonzero(f == cfg.val_fold)
        if va.size == 0:
            raise AssertionError(f"No samples assigned to validation fold {cfg.val_fold}.")
        tr = np.setdiff1d(np.arange(n), va)
    else:
        k = int(np.clip(round(cfg.split_data_at * n), 0, n))           # MLUtils.splitobs(at = ...)
        if cfg.shuffleobs:
            idx = (rng or np.random.default_rng()).permutation(n)
            tr, va = idx[:k], idx[k:]
        else:
            tr, va = slice(0, k), slice(k, n)                           # contiguous halves: views, no gather
    return tr, va


def split_data(data, model, cfg: DataConfig = DataConfig(), rng: Optional[np.random.Generator] = None, sequence_kwargs: Optional[dict] = None):
    """split_data.jl:8-79 -> (train, val) each ((X, forcings), targets).  With sequence_kwargs (or a model with an LSTM layer): each
    ((X, forcings), targets, windows) -- the whole series and the split's windows (sequences.Sequences)."""
    if sequence_kwargs is not None or cfg.sequence_kwargs is not None or getattr(model, "lstm_layer", None) is not None:
        if sequence_kwargs is not None:
            cfg = copy.copy(cfg); cfg.sequence_kwargs = sequence_kwargs
        series, wtr, wva = _sequence_splits(model, data, cfg, rng)
        return (series[0], series[1], wtr), (series[0], series[1], wva)
    raw_cols = _columns(data) if not isinstance(data, tuple) else None
    (X, forc), targ = prepare_data(model, data)
    tr, va = _split_rows(cfg, X.shape[1], raw_cols, rng)

    def take(ix):
        return (np.ascontiguousarray(X[:, ix]), {k: v[ix] for k, v in forc.items()}), {k: v[ix] for k, v in targ.items()}
    return take(tr), take(va)


# ---------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------


@dataclass
class EpochSnapshot:                                               # initialization.jl:53-58
    l_train: dict
    l_val: dict
    y_train: Optional[dict] = None
    y_val: Optional[dict] = None


def _prediction_tables(eng, model, ytr, yva):
    """(train_obs_pred, val_obs_pred, train_diffs, val_diffs) of the model the engine holds: one forward pass per split (train.jl:130-136)"""
    def obs_pred(split, y):
        if eng.n_samples[split] == 0:
            return {}, None
        o = eng.forward(split)
        if eng.seq_ow[split]:                    # sequence models: one row per (window, j)
            d = {t: np.asarray(y[t]).reshape(-1) for t in model.targets}
            d.update({t + "_pred": o[t].reshape(-1) for t in model.targets})
            return d, {k: v.reshape(-1) for k, v in o["parameters"].items()}
        d = {t: y[t] for t in model.targets}
        d.update({t + "_pred": o[t] for t in model.targets})
        return d, o["parameters"]
    tr_op, tr_diff = obs_pred(L.EH_SPLIT_TRAIN, ytr)
    va_op, va_diff = obs_pred(L.EH_SPLIT_VAL, yva)
    return tr_op, va_op, tr_diff, va_diff


class _PendingPredictions:
    """The observed-vs-predicted tables and physical parameters of a finished train() call that nobody has looked at yet: the engine --
    parameters and BatchNorm state of the returned model set, both splits resident -- stays open until the first of the four fields is
    read (one forward pass per split + the copies to the host, then the engine is closed) or the results are dropped.  On the
    headline data set the eager copies are 50 MB into freshly mapped host memory: 1-22 ms of a 24-45 ms call, most of its
    run-to-run spread (tools/e2e_breakdown.py)."""

    def __init__(self, eng, model, ytr, yva):
        self.eng, self.model, self.ytr, self.yva, self.out = eng, model, ytr, yva, None

    def resolve(self):
        if self.out is None:
            try:
                self.out = _prediction_tables(self.eng, self.model, self.ytr, self.yva)
            finally:
                self.release()
        return self.out

    def release(self):
        eng, self.eng = self.eng, None
        if eng is not None:
            eng.close()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class TrainResults:                                                # TrainingConfig.jl:190-223
    """train_history, val_history, epoch_history, train_obs_pred, val_obs_pred, train_diffs, val_diffs, ps, st, best_epoch, best_loss
    (+ timing).  The four prediction fields may be pending (TrainConfig.predictions = "lazy", the default for an engine train() made
    itself): they are computed, exactly as the eager form would have, when first read; `release()` drops them and the device memory."""

    def __init__(self, train_history, val_history, epoch_history, train_obs_pred, val_obs_pred, train_diffs, val_diffs, ps, st, best_epoch, best_loss,
                 timing=None, pending: Optional[_PendingPredictions] = None, chain_status=None, dropout_state=None, lbfgs=None):
        self.train_history, self.val_history, self.epoch_history = train_history, val_history, epoch_history
        self._pred = (train_obs_pred, val_obs_pred, train_diffs, val_diffs)
        self._pending = pending
        self.ps, self.st, self.best_epoch, self.best_loss = ps, st, best_epoch, best_loss
        self.timing = timing           # TrainConfig.timing: seconds of the call by part
        # opt = OptimiserChain(...): steps applied, of them with ClipNorm's factor below 1 (their fraction is how one tunes omega), steps with a non-finite norm
        self.chain_applied, self.chain_clipped, self.chain_nonfinite = chain_status if chain_status is not None else (None, None, None)
        # a model with Dropout layers: the seed of the run's masks and the count of training steps behind it (train_from continues there)
        self.dropout_seed, self.dropout_step = dropout_state if dropout_state is not None else (None, None)
        # opt = LBFGS(): the status of the (last) solve -- iterations, evaluations, f0, g_inf, last_t, pairs, status -- and its trace, one
        # dict per accepted iteration (f, t, trials, g_inf, sy, decisions, evaluations)
        self.lbfgs_status, self.lbfgs_trace = lbfgs if lbfgs is not None else (None, None)

    def _get(self, i):
        if self._pending is not None:
            self._pred = self._pending.resolve()
            self._pending = None
        return self._pred[i]

    train_obs_pred = property(lambda self: self._get(0))
    val_obs_pred = property(lambda self: self._get(1))
    train_diffs = property(lambda self: self._get(2))
    val_diffs = property(lambda self: self._get(3))

    @property
    def predictions_pending(self) -> bool:
        return self._pending is not None

    def release(self):
        """drop pending predictions (and the engine that would have made them) without computing them"""
        if self._pending is not None:
            self._pending.release()
            self._pending = None
            self._pred = ({}, {}, None, None)


def _losses(engine, split, targets, loss_types, agg="sum"):
    """(mse = (reco = .., sum = ..), r2 = (...)) as nested dicts, the aggregate under the name of `agg`; compute_loss.jl:55-66."""
    if engine.n_samples[split] == 0:
        return _losses_of(None, targets, loss_types, agg)
    return _losses_of(engine.eval(split)[0], targets, loss_types, agg)


def _losses_of(metrics, targets, loss_types, agg="sum"):
    """the same from one model's evaluated metrics (a list of dicts, one per target); None: nothing was evaluated (an empty split)"""
    if metrics is None:
        return {lt: {**{t: float("nan") for t in targets}, agg: float("nan")} for lt in loss_types}
    out = {}
    for lt in loss_types:
        per = {t: metrics[i][lt] for i, t in enumerate(targets)}
        tot = float(sum(per[t] for t in targets))
        per[agg] = tot / len(targets) if agg == "mean" else tot
        out[lt] = per
    return out


def _chain_check(eng, epoch):
    """opt = OptimiserChain(...): the engine's counters (applied, clipped, non-finite) where the epoch loop has synchronised anyway;
    ClipNorm(throw = true) and a step whose norm was not finite: Optimisers.jl's error (that step was not applied).  None without a chain."""
    if not getattr(eng, "has_chain", False):
        return None
    stat = eng.chain_status()
    cn = [st for st in eng._chain if st[0] == "clipnorm"]
    if cn and cn[0][3] and stat[2]:
        raise FloatingPointError(f"gradient has {cn[0][2]:g}-norm that is not finite in {stat[2]} step(s) up to epoch {epoch} "
                                 "(ClipNorm(throw = true)): those steps were not applied")
    return stat


def _lbfgs_misplaced(opt):
    """LBFGS anywhere but as `opt` itself: the reason, before anything is uploaded"""
    if isinstance(opt, OptimiserChain):
        _chain_has_lbfgs = lambda c: any(isinstance(o, LBFGS) or (isinstance(o, OptimiserChain) and _chain_has_lbfgs(o)) for o in c.opts)
        if _chain_has_lbfgs(opt):
            _chain_args(OptimiserChain(LBFGS()))
    if isinstance(opt, tuple) and hasattr(opt, "_asdict"):
        opt = opt._asdict()
    if isinstance(opt, dict):
        for k, r in opt.items():
            if isinstance(r, LBFGS):
                raise NotImplementedError(f"per-branch optimiser {k!r}: LBFGS works on the whole parameter vector (one line search, one history): "
                                          "not built as a per-branch rule")


def _lbfgs_check(model, tc: TrainConfig, solve_kw):
    """opt = LBFGS(): what the Optimization.jl driver on the device does not run, with the reason; the solve keywords it drops"""
    o = tc.opt
    if not (1 <= int(o.m) <= L.EH_LBFGS_MAX_M):
        raise ValueError(f"LBFGS(m = {o.m}): the history holds 1..{L.EH_LBFGS_MAX_M} pairs")
    if not (0 < o.c1 < o.c2 < 1):
        raise ValueError(f"LBFGS(c1 = {o.c1}, c2 = {o.c2}): need 0 < c1 < c2 < 1")
    if not (1 <= int(o.max_linesearch) <= 48):
        raise ValueError(f"LBFGS(max_linesearch = {o.max_linesearch}): 1..48")
    if not o.initial_step >= 0:
        raise ValueError(f"LBFGS(initial_step = {o.initial_step}): must not be negative")
    if tc.eval_every < 1 or tc.inner_maxiters < 1:
        raise ValueError("eval_every and inner_maxiters must be >= 1")
    if getattr(model, "dropout", None) is not None:
        raise NotImplementedError("train(opt = LBFGS()): Dropout layers -- the line search needs the same objective at every trial point, the masks "
                                  "change with every pass: not built")
    if getattr(model, "bn_layers", None):
        raise NotImplementedError("train(opt = LBFGS()): BatchNorm layers in hidden_layers -- the Optimization.jl driver carries no layer state "
                                  "(their running statistics would stay at their start): not built")
    if bool(model.config.get("input_batchnorm")):
        raise NotImplementedError("train(opt = LBFGS()): input BatchNorm -- the reference's Optimization.jl driver never carries the layer state: not built")
    if tc.distributed is True:
        raise NotImplementedError("train(opt = LBFGS(), distributed=True): data parallelism is not built for the Optimization.jl driver")
    if tc.promote_f64:
        warnings.warn("promote_f64: the parameters stay float32 on the device; every scalar of the L-BFGS recurrences (dot products, step lengths, "
                      "the two-loop coefficients) is kept in double already, and the field works around a Lux issue this path does not have")
    if not tc.full_batch:                 # train_optimization.jl drops them for the minibatch solves: inner_maxiters and nepochs rule there
        solve_kw.pop("maxiters", None)
        solve_kw.pop("epochs", None)


def _want_distributed(tc: TrainConfig) -> bool:
    if tc.distributed is not None:
        return bool(tc.distributed)
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    except Exception:
        return False


def _train_distributed(model, tc: TrainConfig, rng, train_split, val_split) -> TrainResults:
    """The epoch loop of `train` with the steps sharded over the ranks of the default process group (one process per
    GPU).  Every rank holds a contiguous shard of the training split as its train data and takes batchsize / world
    samples of it per step (per-shard shuffling: the sample ORDER differs from a global shuffle, the distribution does
    not); gradients meet through DataParallel (peer-to-peer stores or one RCCL all-reduce per step).  Evaluation is
    replicated: a second engine per rank holds the full train / validation splits, so history, early stopping and the
    returned TrainResults are identical on every rank without further communication."""
    import torch
    import torch.distributed as dist
    from .dp import DataParallel, shard_range
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("train(distributed=True) needs an initialised torch.distributed process group (one rank per GPU)")
    (xtr, ftr, ytr), (xva, fva, yva) = train_split, val_split
    world, rank = dist.get_world_size(), dist.get_rank()
    device = torch.cuda.current_device()
    N = xtr.shape[1]
    lo, hi = shard_range(N, rank, world)
    xfn = _extra_fn(tc.extra_loss)                    # extra_loss as a function of the predictions: its entries are targets of the TRAINING engine
    ev = model.engine(device)                         # evaluation replica: full splits
    eng = model.engine(device, extra_fn=xfn)          # training replica: this rank's shard
    try:
        ev.set_data(L.EH_SPLIT_TRAIN, xtr, [ftr[f] for f in model.forcing], [ytr[t] for t in model.targets])
        ev.set_data(L.EH_SPLIT_VAL, xva, [fva[f] for f in model.forcing], [yva[t] for t in model.targets])
        eng.set_data(L.EH_SPLIT_TRAIN, xtr[:, lo:hi], [ftr[f][lo:hi] for f in model.forcing], [ytr[t][lo:hi] for t in model.targets])
        if tc.train_from is None:
            theta = model.initialparameters(rng)      # same seed -> same start on every rank
        else:
            theta = np.asarray(tc.train_from.ps if isinstance(tc.train_from, TrainResults) else tc.train_from[0], np.float32)
        eng.set_params(theta); ev.set_params(theta)
        _opt_setup(eng, tc.opt, model)
        eng.set_training_loss(tc.training_loss)
        xterms = _extra_terms(tc.extra_loss)          # functions of the replicated parameters: every rank adds the same terms in eh_dp_apply
        aggn = _agg_name(tc.agg)
        _apply_extra_loss(eng, model, xterms, aggn, eng.n_pseudo)
        drv = DataParallel(eng, fused=tc.fused_update is not False, specialize=bool(tc.specialize))      # ("auto" compiles before the first step here: every rank has to be ready together)
        has_bn = bool(model.config.get("input_batchnorm"))
        first_lt = tc.loss_types[0]

        def snapshot():
            eng.synchronize()
            ev.set_params(eng.get_params())
            if has_bn:
                ev.set_bn_state(*eng.get_bn_state())
            snap = EpochSnapshot(_losses(ev, L.EH_SPLIT_TRAIN, model.targets, tc.loss_types, aggn),
                                 _losses(ev, L.EH_SPLIT_VAL, model.targets, tc.loss_types, aggn))
            if xterms or xfn is not None:
                for d, split in ((snap.l_train, L.EH_SPLIT_TRAIN), (snap.l_val, L.EH_SPLIT_VAL)):
                    preds = ev.forward(split, params=False) if (xfn is not None and ev.n_samples[split]) else None
                    d["extra_loss"] = _extra_loss_values(model, eng.get_params(), xterms, aggn, xfn, preds)
            return snap
        init = snapshot()
        history = [init]
        best_loss, best_ps, best_epoch, counter = init.l_val[first_lt][aggn], theta.copy(), 0, 0
        best_bn = eng.get_bn_state() if has_bn else None            # early_stopping.jl update!: best_ps AND best_st
        seed0 = tc.random_seed if tc.random_seed is not None else 0
        b = -(-tc.batchsize // world)                 # samples per rank per step
        steps = -(-(-(-N // world)) // b)             # ceil(largest shard / b): the same number of steps on every rank
        n_loc = hi - lo
        for epoch in range(1, tc.nepochs + 1):
            eng.dp_shuffle(seed0 + epoch + 7919 * rank)
            for s_ in range(steps):
                first = min(s_ * b, n_loc)
                drv.step(first, min(b, n_loc - first))
            snap = snapshot()
            _chain_check(eng, epoch)
            if tc.keep_history:
                history.append(snap)
            cur = snap.l_val[first_lt][aggn]
            if isbetter(cur, best_loss, first_lt):
                best_loss, best_ps, best_epoch, counter = cur, eng.get_params(), epoch, 0
                if has_bn:
                    best_bn = eng.get_bn_state()
                if not tc.keep_history:
                    history[0] = snap
            else:
                counter += 1
            if counter >= tc.patience:
                break
        eng.synchronize()
        ps = best_ps if tc.return_model == "best" else eng.get_params()
        bn_out = (best_bn if tc.return_model == "best" else eng.get_bn_state()) if has_bn else None      # best_or_final
        ev.set_params(ps)
        if has_bn:
            ev.set_bn_state(*bn_out)

        def obs_pred(split, y):
            if ev.n_samples[split] == 0:
                return {}, None
            out = ev.forward(split)
            d = {t: y[t] for t in model.targets}
            d.update({t + "_pred": out[t] for t in model.targets})
            return d, out["parameters"]
        tr_op, tr_diff = obs_pred(L.EH_SPLIT_TRAIN, ytr)
        va_op, va_diff = obs_pred(L.EH_SPLIT_VAL, yva)
        st = {"fixed": {f: np.float32(model.parameters.default(f)) for f in model.fixed_param_names}}
        if has_bn:
            st["st_nn"] = {"running_mean": bn_out[0], "running_var": bn_out[1]}
        return TrainResults([s.l_train for s in history], [s.l_val for s in history], history, tr_op, va_op, tr_diff, va_diff,
                            ps, st, best_epoch, best_loss, chain_status=_chain_check(eng, best_epoch))
    finally:
        eng.close(); ev.close()


_GC_FROZEN = 0


def _freeze_gc_once(at_end=False):
    """The first train() call of a process runs ONE full garbage collection and freezes what survives it (gc.freeze: the interpreter's,
    NumPy's and -- if it is loaded -- torch's module-level objects, about a million of them).  Without this the cyclic collector's first
    full pass lands in the middle of the second to fourth call and walks all of them: 40-100 ms of a 17 ms call (tools/e2e_breakdown2.py:
    the spike sat wherever the allocation count happened to cross the threshold -- engine creation, upload, the first evaluation -- and
    was the 2 x run-to-run spread of a short train() call that rounds 4 and 5 could not explain).  EH_NO_GC_FREEZE=1 leaves the
    collector alone."""
    global _GC_FROZEN
    import sys
    # (torch imported since the last freeze: its objects are new to the collector -- once more; and once more when the first call of the
    #  process ENDS -- what it imported and built on the way, the engine library's bindings and the run-time compiler among it, was a 45 ms
    #  full pass at the end of the second call, tools/e2e_spikes.py)
    state = (4 if "torch" in sys.modules else 2) + (1 if at_end else 0)
    if _GC_FROZEN >= state or os.environ.get("EH_NO_GC_FREEZE"):
        return
    _GC_FROZEN = state
    import gc
    if gc.isenabled():
        gc.collect()
        gc.freeze()


def train(model: SingleNNHybridModel, data, save_ps=(), *, train_cfg: Optional[TrainConfig] = None,
          data_cfg: Optional[DataConfig] = None, engine=None, **kwargs) -> Optional[TrainResults]:
    """train(model, data; kwargs...) -> TrainResults (train.jl:211-219 -> _train :95-136).
    Flat kwargs override config fields exactly like override_configs (train.jl:300-314)."""
    tc = copy.copy(train_cfg) if train_cfg else TrainConfig()
    dc = copy.copy(data_cfg) if data_cfg else DataConfig()
    solve_kw = {}
    for k, v in kwargs.items():
        if hasattr(tc, k):
            setattr(tc, k, v)
        elif hasattr(dc, k):
            setattr(dc, k, v)
        elif k in _SOLVE_KEYWORDS and isinstance(kwargs.get("opt", tc.opt), LBFGS):
            solve_kw[k] = v
        else:
            raise TypeError(f"train: unknown keyword {k!r}")
    validate_config(tc)
    lbfgs = tc.opt if isinstance(tc.opt, LBFGS) else None
    if lbfgs is not None:
        _lbfgs_check(model, tc, solve_kw)
    else:
        _lbfgs_misplaced(tc.opt)
    _freeze_gc_once()
    t_call = time.perf_counter()
    rng = np.random.default_rng(tc.random_seed)
    dist_run = _want_distributed(tc)
    own = engine is None
    has_drop = getattr(model, "dropout", None) is not None
    if lbfgs is not None and dist_run:
        raise NotImplementedError("train(opt = LBFGS(), distributed=True): data parallelism is not built for the Optimization.jl driver")
    if has_drop and dist_run:
        raise NotImplementedError("train(distributed=True): Dropout layers are not built for data parallelism (the masks are drawn per handle)")
    bn_layers = list(getattr(model, "bn_layers", None) or [])
    if bn_layers and dist_run:
        raise NotImplementedError("train(distributed=True): BatchNorm layers in hidden_layers are not built for data parallelism (their statistics would "
                                  "have to be those of the global batch)")
    xfn = _extra_fn(tc.extra_loss)                    # extra_loss as a function of the predictions (compute_loss.jl:31-34): recorded, its entries ride on targets of their own
    if xfn is not None and engine is not None and not engine.n_pseudo:
        raise ValueError("train(engine = ...): an extra_loss of the predictions needs an engine created with it (model.engine(device, extra_fn = f))")
    # the caller's float32 columns as they are: views, no stacked copy (4 M rows: 7 -> 1 ms); on a large table the upload starts before the
    # screen for rows to drop has finished (_EarlyUpload)
    fast, early = None, None
    is_seq = model.lstm_layer is not None
    if dc.sequence_kwargs is not None and not is_seq:
        raise ValueError("sequence_kwargs: the model has no Recurrence layer (hidden_layers = Chain(Recurrence(LSTMCell(I, H))))")
    if is_seq and (dist_run or xfn is not None):
        raise NotImplementedError("sequence models: data parallelism and an extra_loss of the predictions are not built")
    if is_seq:
        _sequence_loss_check(tc.training_loss, len(model.targets))
    wtr = wva = None
    if is_seq:
        ((xs, fs), ys), wtr, wva = _sequence_splits(model, data, dc, rng)
        if len(wtr.starts) == 0:
            return None
    cv = None if (dist_run or is_seq) else _column_views(model, data, dc)
    if cv is not None:
        views = _take_views(model, cv[0], dc, cv[2])
        if own and cv[2] >= (1 << 20) and len(views[0][0][0][0]) > 0 and not os.environ.get("EH_NO_EARLY_UPLOAD"):      # (a large table, a training split that is not empty)
            early = _EarlyUpload(model, tc.device, xfn, views)
        ok = False
        try:
            ok = _no_row_to_drop(model, *cv)
        finally:
            if early is not None:
                engine_early = early.join(keep=ok)
        fast = views if ok else None
        if not ok:
            early = None
    if is_seq:       # the series goes to both splits; what the result tables call "observed" is the target of every (window, j)
        (xtr, ftr, ytr), (xva, fva, yva) = (xs, fs, ys), (xs, fs, ys)
    else:
        (xtr, ftr, ytr), (xva, fva, yva) = [(a[0][0], a[0][1], a[1]) for a in (fast if fast is not None else split_data(data, model, dc, rng))]
    if (len(xtr[0]) if isinstance(xtr, list) else xtr.shape[1]) == 0:
        if early is not None:
            engine_early.close()
        return None                                                # train.jl:186 ("returns nothing on empty splits")
    if dist_run:
        return _train_distributed(model, tc, rng, (xtr, ftr, ytr), (xva, fva, yva))
    t_prep = time.perf_counter()
    if early is not None:
        eng = engine_early
        # (prepare_s: what the call waited for beyond the worker's engine + upload -- the part of the screen that did not hide behind them)
        t_prep = t_call + max(0.0, (t_prep - t_call) - early.engine_s - early.upload_s)
        t_eng = t_prep + early.engine_s
    else:
        eng = engine if engine is not None else model.engine(tc.device, extra_fn=xfn)
        t_eng = time.perf_counter()
    keep_engine = False
    try:
        if early is None:
            eng.set_data(L.EH_SPLIT_TRAIN, xtr, [ftr[f] for f in model.forcing], [ytr[t] for t in model.targets])
            eng.set_data(L.EH_SPLIT_VAL, xva, [fva[f] for f in model.forcing], [yva[t] for t in model.targets])
        if is_seq:
            for split, w in ((L.EH_SPLIT_TRAIN, wtr), (L.EH_SPLIT_VAL, wva)):
                eng.set_sequences(split, w.input_window, w.output_window, w.lead_time, w.starts)
            ytr = {t: ys[t][wtr.target_rows()] for t in model.targets}
            yva = {t: ys[t][wva.target_rows()] for t in model.targets}
        if tc.timing:
            eng.synchronize()
        t_up = time.perf_counter()
        if tc.train_from is None:
            theta = model.initialparameters(rng)
        else:
            theta = np.asarray(tc.train_from.ps if isinstance(tc.train_from, TrainResults) else tc.train_from[0], np.float32)
        eng.set_params(theta)
        if bn_layers and tc.train_from is not None:      # the layer state of the model the run continues from (its st.st_layers)
            st_from = tc.train_from.st if isinstance(tc.train_from, TrainResults) else (tc.train_from[1] if len(tc.train_from) > 1 else None)
            for l, s_l in ((st_from or {}).get("st_layers") or {}).items():
                eng.set_layer_state(int(l), s_l["running_mean"], s_l["running_var"])
        if lbfgs is None:
            _opt_setup(eng, tc.opt, model)
        eng.set_training_loss(tc.training_loss)
        xterms = _extra_terms(tc.extra_loss)
        aggn = _agg_name(tc.agg)
        _apply_extra_loss(eng, model, xterms, aggn, eng.n_pseudo)
        _apply_step_mode(eng, replace(tc, fused_update=False) if lbfgs is not None else tc, is_seq or bool(bn_layers) or bool(getattr(model, "ln_layers", None)))      # (BatchNorm / LayerNorm layers: the engine runs the pair, as for sequence models)
        if lbfgs is not None:      # (after the losses and options: the mode refuses what changes the objective between trial points)
            eng.lbfgs_init(m=lbfgs.m, c1=lbfgs.c1, c2=lbfgs.c2, max_linesearch=lbfgs.max_linesearch, initial_step=lbfgs.initial_step,
                           g_tol=float(solve_kw.get("g_tol", 1e-5)), f_reltol=float(solve_kw.get("f_reltol", 0.0)))
        drop_seed = None
        if has_drop:
            # masks keyed by the run's seed; without one the run continues the seed of the TrainResults it starts from, or draws one (reported
            # as dropout_seed either way).  A run continued under the SAME seed continues the step count, so no mask of the first run comes
            # back; under another seed the stream is a new one and starts at step 0.  (The engine runs a dropout handle one launch per step.)
            prev = tc.train_from if isinstance(tc.train_from, TrainResults) and tc.train_from.dropout_seed is not None else None
            if tc.random_seed is not None:
                drop_seed = int(tc.random_seed)
            elif prev is not None:
                drop_seed = int(prev.dropout_seed)
            else:
                drop_seed = int(np.random.SeedSequence().generate_state(2, np.uint32).view(np.uint64)[0])
            eng.set_dropout(model.dropout, seed=drop_seed, step=int(prev.dropout_step) if (prev is not None and int(prev.dropout_seed) == drop_seed) else 0)
        first_lt = tc.loss_types[0]

        def snapshot():
            snap = EpochSnapshot(_losses(eng, L.EH_SPLIT_TRAIN, model.targets, tc.loss_types, aggn),
                                 _losses(eng, L.EH_SPLIT_VAL, model.targets, tc.loss_types, aggn))
            if xterms or xfn is not None:                # compute_loss.jl:39-44: eval mode reports the extra losses next to the metrics
                for d, split in ((snap.l_train, L.EH_SPLIT_TRAIN), (snap.l_val, L.EH_SPLIT_VAL)):
                    preds = eng.forward(split, params=False) if (xfn is not None and eng.n_samples[split]) else None
                    d["extra_loss"] = _extra_loss_values(model, eng.get_params(), xterms, aggn, xfn, preds)
            return snap
        t_setup = time.perf_counter()
        init = snapshot()
        history = [init]
        best_loss, best_ps, best_epoch, counter = init.l_val[first_lt][aggn], theta.copy(), 0, 0
        has_bn = bool(model.config.get("input_batchnorm"))
        best_bn = eng.get_bn_state() if has_bn else None            # early_stopping.jl update!: best_ps AND best_st
        best_ls = {l: eng.get_layer_state(l) for l in bn_layers}      # ... the BatchNorm layers of the chain belong to best_st too
        seed0 = tc.random_seed if tc.random_seed is not None else int(rng.integers(2**31))
        tm = {"steps_s": 0.0, "eval_s": 0.0, "host_s": 0.0, "epochs": 0} if tc.timing else None
        if tm is not None:
            # outside the epoch loop, part by part: split + cast of the caller's columns | engine creation | interleave +
            # upload of both splits | parameters, optimiser, options (incl. a run-time compilation that is not in the disk cache) | the
            # evaluation of epoch 0
            tm.update(prepare_s=t_prep - t_call, engine_s=t_eng - t_prep, upload_s=t_up - t_eng, setup_s=t_setup - t_up, initial_eval_s=time.perf_counter() - t_setup)
        chain_stat = _chain_check(eng, 0)
        t_loop = time.perf_counter()
        lb_out = [None, None]

        def lbfgs_snapshot(index):
            """a snapshot at history index `index` (iteration or pass); True when the patience has run out"""
            nonlocal best_loss, best_ps, best_epoch, counter
            snap = snapshot()
            if tc.keep_history:
                history.append(snap)
            cur = snap.l_val[first_lt][aggn]
            if isbetter(cur, best_loss, first_lt):
                best_loss, best_ps, best_epoch, counter = cur, eng.get_params(), index, 0
                if not tc.keep_history:
                    history[0] = snap
            else:
                counter += 1
            return counter >= tc.patience
        if lbfgs is not None and tc.full_batch:                  # one solve over the training split, paused every eval_every iterations (_optim_callback)
            maxiters = int(solve_kw.get("maxiters", 1000))
            eng.lbfgs_set_batch(L.EH_SPLIT_TRAIN)
            at, st = 0, eng.lbfgs_status()
            while at < maxiters and st["code"] in (0, 3):
                st = eng.lbfgs_solve(min(maxiters, at + tc.eval_every))
                if st["iterations"] == at:                       # (converged, failed or empty at the iterate the last snapshot saw)
                    break
                at = st["iterations"]
                if lbfgs_snapshot(at):
                    break
            lb_out = [st, eng.lbfgs_trace()]
        elif lbfgs is not None:                                  # _run_minibatch!: a fresh solve on every minibatch, warm-started
            ntr = eng.n_samples[L.EH_SPLIT_TRAIN]
            for epoch in range(1, tc.nepochs + 1):
                perm = rng.permutation(ntr).astype(np.int32)
                for lo in range(0, ntr, tc.batchsize):
                    eng.lbfgs_set_batch(L.EH_SPLIT_TRAIN, idx=perm[lo:lo + tc.batchsize])
                    st = eng.lbfgs_solve(tc.inner_maxiters)      # (an empty minibatch: "empty batch" after its first evaluation, theta untouched)
                    lb_out = [st, None]
                if lbfgs_snapshot(epoch):
                    break
            if lb_out[0] is not None:
                lb_out[1] = eng.lbfgs_trace()
        for epoch in range(1, (tc.nepochs if lbfgs is None else 0) + 1):
            t0 = time.perf_counter()
            eng.train_epoch(tc.batchsize, seed=seed0 + epoch, shuffle=True, want_loss=False)      # run_epoch!
            if tm is not None:
                eng.synchronize()
                t1 = time.perf_counter()
            snap = snapshot()                                                                  # evaluate_epoch
            chain_stat = _chain_check(eng, epoch)                                              # (the evaluation has synchronised)
            if tm is not None:
                t2 = time.perf_counter()
                tm["steps_s"] += t1 - t0; tm["eval_s"] += t2 - t1; tm["epochs"] += 1
            if tc.keep_history:
                history.append(snap)
            cur = snap.l_val[first_lt][aggn]
            if isbetter(cur, best_loss, first_lt):                                             # early_stopping.jl:16-42
                best_loss, best_ps, best_epoch, counter = cur, eng.get_params(), epoch, 0
                if has_bn:
                    best_bn = eng.get_bn_state()
                best_ls = {l: eng.get_layer_state(l) for l in bn_layers}
                if not tc.keep_history:
                    history[0] = snap
            else:
                counter += 1
            if counter >= tc.patience:
                break
        if tm is not None:
            eng.synchronize()
            tm["loop_s"] = time.perf_counter() - t_loop
            tm["host_s"] = tm["loop_s"] - tm["steps_s"] - tm["eval_s"]
        t_final = time.perf_counter()
        drop_step = eng.get_dropout()[2] if has_drop else None
        ps = best_ps if tc.return_model == "best" else eng.get_params()                        # best_or_final
        bn_out = (best_bn if tc.return_model == "best" else eng.get_bn_state()) if has_bn else None
        eng.set_params(ps)
        if has_bn:
            eng.set_bn_state(*bn_out)                                # the predictions below use the state that belongs to `ps`
        ls_out = best_ls if tc.return_model == "best" else {l: eng.get_layer_state(l) for l in bn_layers}
        for l, (m_l, v_l) in ls_out.items():
            eng.set_layer_state(l, m_l, v_l)

        fixed = {f: np.float32(model.parameters.default(f)) for f in model.fixed_param_names}
        st = {"fixed": fixed}
        if has_bn:
            st["st_nn"] = {"running_mean": bn_out[0], "running_var": bn_out[1]}      # Lux BatchNorm state of the returned model (best_or_final)
        if bn_layers:      # ... and of the chain's BatchNorm layers, by hidden layer
            st["st_layers"] = {l: {"running_mean": m_l, "running_var": v_l} for l, (m_l, v_l) in ls_out.items()}
        if tc.predictions not in ("lazy", "eager"):
            raise ValueError("predictions must be 'lazy' or 'eager'")
        if own and tc.predictions == "lazy":
            pending = _PendingPredictions(eng, model, ytr, yva)
            keep_engine = True           # (the results own it from here: closed when the predictions are read, released or dropped)
            preds = (None, None, None, None)
        else:
            pending, preds = None, _prediction_tables(eng, model, ytr, yva)
        if tm is not None:
            tm["final_predictions_s"] = time.perf_counter() - t_final       # (eager: forward over both splits with the returned parameters + the copies to the host)
            tm["call_s_before_close"] = time.perf_counter() - t_call
        return TrainResults([s.l_train for s in history], [s.l_val for s in history], history, *preds,
                            ps, st, best_epoch, best_loss, tm, pending, chain_stat, (drop_seed, drop_step) if has_drop else None,
                            lbfgs=lb_out if lbfgs is not None else None)
    finally:
        if own and not keep_engine:
            eng.close()
        _freeze_gc_once(at_end=True)


# ---------------------------------------------------------------------------------------------
# groups of models trained side by side: cross-validation folds, sweeps over optimiser numbers, repeated seeds
# ---------------------------------------------------------------------------------------------

_MEMBER_KEYS = ("val_fold", "random_seed", "opt")


def _member_configs(tc: TrainConfig, dc: DataConfig, members):
    """the member dicts -> [(TrainConfig, DataConfig)], one pair per member: the common configuration with the member's overrides"""
    if not isinstance(members, (list, tuple)) or not members:
        raise ValueError("train_members: members must be a non-empty list of dicts")
    out = []
    for j, m in enumerate(members):
        if not isinstance(m, dict):
            raise ValueError(f"train_members: member {j} is {type(m).__name__}, not a dict")
        extra = [k for k in m if k not in _MEMBER_KEYS]
        if extra:
            raise ValueError(f"train_members: member {j} has unknown key(s) {extra}; a member may override {list(_MEMBER_KEYS)}, everything else is common")
        tcj, dcj = copy.copy(tc), copy.copy(dc)
        if "random_seed" in m:
            tcj.random_seed = m["random_seed"]
        if "opt" in m:
            tcj.opt = m["opt"]
        if "val_fold" in m:
            dcj.val_fold = m["val_fold"]
        out.append((tcj, dcj))
    kinds = {type(c.opt).__name__ for c, _ in out if isinstance(c.opt, _RULES)}
    if len(kinds) > 1:
        raise ValueError(f"train_members: the members mix optimiser rules {sorted(kinds)}: one rule type for all, its numbers are free per member")
    return out


def _per_net(model) -> bool:
    """the descriptor asks for an activation per network / per layer (EH_ACT_PER_NET)"""
    try:
        return int(model.to_desc().activation) == L.EH_ACT_PER_NET
    except Exception:
        return False


def _members_refusals(model, tc: TrainConfig, dc: DataConfig, cfgs):
    """what train_members does not run, each with its reason, before anything is uploaded or trained"""
    who = "train_members"
    if tc.distributed is True or _want_distributed(tc):
        raise NotImplementedError(f"{who}: distributed training (data parallelism) is not built for groups of models: the members already fill the device, a workgroup each")
    for c, _ in cfgs:
        if isinstance(c.opt, LBFGS):
            raise NotImplementedError(f"{who}: LBFGS (the Optimization.jl driver, a line search per model) is not built for groups of models")
        if isinstance(c.opt, OptimiserChain):
            raise NotImplementedError(f"{who}: an OptimiserChain (ClipNorm needs the norm of the whole gradient ahead of the update) is not built for groups of models")
        if isinstance(c.opt, dict) or (isinstance(c.opt, tuple) and hasattr(c.opt, "_asdict")):
            raise NotImplementedError(f"{who}: a per-branch opt (a rule per branch of the parameter tree) is not built for groups of models: one rule per member")
        if not isinstance(c.opt, _RULES):
            _opt_args(c.opt)                         # (raises with the reason)
    if getattr(model, "lstm_layer", None) is not None or dc.sequence_kwargs is not None:
        raise NotImplementedError(f"{who}: sequence models (Recurrence layers, windows) are not built for groups of models")
    if tc.extra_loss is not None:
        raise NotImplementedError(f"{who}: an extra_loss runs on the step + reduce pair, not in the one-workgroup step a member trains with")
    from .engine import PerTarget
    tl = tc.training_loss
    if callable(tl) or isinstance(tl, PerTarget) or isinstance(tl, (list, tuple)):
        raise NotImplementedError(f"{who}: recorded losses (a function as training_loss), per-target losses and closures run on kernels compiled at run time, "
                                  "which a group of models does not use")
    if getattr(getattr(model, "mechanistic_model", None), "fn", None) is not None:
        raise NotImplementedError(f"{who}: a recorded mechanistic closure runs on kernels compiled at run time, which a group of models does not use")
    if isinstance(tl, str) and tl in ("pearsonLoss", "kgeLoss", "pbkgeLoss"):
        raise NotImplementedError(f"{who}: the two-pass losses (pearsonLoss, kgeLoss, pbkgeLoss) take two forward passes for the batch moments ahead of every "
                                  "step, which the one-workgroup step a member trains with does not run")
    if model.config.get("precision", "f32") != "f32":
        raise NotImplementedError(f"{who}: precision={model.config.get('precision')!r} runs on the row-split bf16 kernels, whose step needs several workgroups")
    if len(model.targets) != 1:
        raise NotImplementedError(f"{who}: several targets need a counting pass ahead of every step: not built for groups of models")
    if getattr(model, "dropout", None) is not None:
        raise NotImplementedError(f"{who}: Dropout layers run on a step kernel compiled at run time, which a group of models does not use")
    if getattr(model, "bn_layers", None) or getattr(model, "ln_layers", None):
        raise NotImplementedError(f"{who}: BatchNorm / LayerNorm layers inside hidden_layers run in the layer-wise form, not in the one-workgroup step")
    if _per_net(model):
        raise NotImplementedError(f"{who}: per-net or per-layer activations run on kernels compiled at run time, which a group of models does not use")
    if tc.specialize is True:
        raise NotImplementedError(f"{who}: specialize=True asks for kernels compiled at run time; a group of models runs the kernels built ahead of time "
                                  "('auto' and False)")
    if tc.fused_update is False:
        raise NotImplementedError(f"{who}: fused_update=False asks for the step + reduce pair; a member trains with the one-workgroup multi-step launch")
    if tc.train_from is not None:
        raise NotImplementedError(f"{who}: train_from is not built for groups of models (every member starts from the parameters its seed draws)")


def _member_rows(model, data, dc: DataConfig, rng, n: Optional[int] = None, raw_cols=None):
    """one member's share of the screened table: (training rows, validation rows) as int32 index arrays, in the order split_data takes them.
    n, raw_cols: the screened table's rows and the caller's columns where the caller has them already (train_members screens once)"""
    if n is None:
        raw_cols = _columns(data) if not isinstance(data, tuple) else None
        n = prepare_data(model, data)[0][0].shape[1]
    tr, va = _split_rows(dc, n, raw_cols, rng)
    ix = np.arange(n, dtype=np.int32)
    return ix[tr], ix[va]


def train_members(model: SingleNNHybridModel, data, members, *, train_cfg: Optional[TrainConfig] = None, data_cfg: Optional[DataConfig] = None,
                  **kwargs) -> List[Optional[TrainResults]]:
    """Several train(model, data; ...) runs that share the model and the table, side by side on one engine: members = [{...}, ...], each
    dict overriding `val_fold`, `random_seed` and / or `opt` (one rule type for all, numbers free) of the common configuration.  Member j's
    data split and initial parameters are those of train(model, data, **common, **members[j]); the table is uploaded once and a fold
    becomes two row lists; every epoch of all members is one launch (a workgroup per member), every evaluation one synchronisation.
    Early stopping, the best-model snapshot and the histories follow train() per member; a stopped member sits out the later launches.
    Returns one TrainResults per member (None where train() would return None: an empty training split), predictions computed eagerly.
    Runs where one workgroup covers a minibatch of a one-target model on the kernels built ahead of time; everything else is refused
    with its reason before any training."""
    tc = copy.copy(train_cfg) if train_cfg else TrainConfig()
    dc = copy.copy(data_cfg) if data_cfg else DataConfig()
    for k, v in kwargs.items():
        if hasattr(tc, k):
            setattr(tc, k, v)
        elif hasattr(dc, k):
            setattr(dc, k, v)
        else:
            raise TypeError(f"train_members: unknown keyword {k!r}")
    cfgs = _member_configs(tc, dc, members)
    for c, _ in cfgs:
        validate_config(c)
    _members_refusals(model, tc, dc, cfgs)
    if tc.predictions not in ("lazy", "eager"):
        raise ValueError("predictions must be 'lazy' or 'eager'")
    M = len(cfgs)
    (X, forc), targ = prepare_data(model, data)
    raw_cols = _columns(data) if not isinstance(data, tuple) else None
    if X.shape[1] == 0:
        return [None] * M
    # per member, train()'s own order of draws: the split (shuffleobs), then theta_0, then the epoch seeds
    rows, theta0, seed0 = [], [], []
    for tcj, dcj in cfgs:
        rng = np.random.default_rng(tcj.random_seed)
        rows.append(_member_rows(model, data, dcj, rng, X.shape[1], raw_cols))
        theta0.append(model.initialparameters(rng))
        seed0.append(tcj.random_seed if tcj.random_seed is not None else int(rng.integers(2**31)))
    live = [len(r[0]) > 0 for r in rows]
    aggn = _agg_name(tc.agg)
    first_lt = tc.loss_types[0]
    has_bn = bool(model.config.get("input_batchnorm"))
    eng = model.engine(tc.device)
    ens = None
    try:
        eng.set_data(L.EH_SPLIT_TRAIN, X, [forc[f] for f in model.forcing], [targ[t] for t in model.targets])
        eng.set_params(theta0[0])
        eng.set_training_loss(tc.training_loss)
        _apply_step_mode(eng, replace(tc, specialize=False))
        ens = eng.ensemble(M, tc.batchsize)
        for j, (tcj, _) in enumerate(cfgs):
            ens.set_params(j, theta0[j])
            ens.set_opt(j, **_opt_args(tcj.opt))
            ens.set_rows(j, 0, rows[j][0])
            ens.set_rows(j, 1, rows[j][1])

        def snapshots():
            mtr, mva = ens.eval(0), ens.eval(1)
            return [EpochSnapshot(_losses_of(mtr[j] if len(rows[j][0]) else None, model.targets, tc.loss_types, aggn),
                                  _losses_of(mva[j] if len(rows[j][1]) else None, model.targets, tc.loss_types, aggn)) for j in range(M)]
        init = snapshots()
        history = [[s] for s in init]
        best_loss = [s.l_val[first_lt][aggn] for s in init]
        best_ps = [t.copy() for t in theta0]
        best_bn = [ens.get_bn_state(j) if has_bn else None for j in range(M)]
        best_epoch, counter = [0] * M, [0] * M
        active = list(live)
        for epoch in range(1, tc.nepochs + 1):
            if not any(active):
                break
            ens.train_epoch([s + epoch for s in seed0], shuffle=True, active=active, want_loss=False)      # run_epoch! of every member still training
            snaps = snapshots()                                                                              # evaluate_epoch
            for j in range(M):
                if not active[j]:
                    continue
                snap = snaps[j]
                if tc.keep_history:
                    history[j].append(snap)
                cur = snap.l_val[first_lt][aggn]
                if isbetter(cur, best_loss[j], first_lt):                                                    # early_stopping.jl:16-42
                    best_loss[j], best_ps[j], best_epoch[j], counter[j] = cur, ens.get_params(j), epoch, 0
                    if has_bn:
                        best_bn[j] = ens.get_bn_state(j)
                    if not tc.keep_history:
                        history[j][0] = snap
                else:
                    counter[j] += 1
                if counter[j] >= tc.patience:
                    active[j] = False
        fixed = {f: np.float32(model.parameters.default(f)) for f in model.fixed_param_names}
        results = []
        for j in range(M):
            if not live[j]:
                results.append(None)                                                                          # train.jl:186
                continue
            ps = best_ps[j] if tc.return_model == "best" else ens.get_params(j)                               # best_or_final
            bn_out = (best_bn[j] if tc.return_model == "best" else ens.get_bn_state(j)) if has_bn else None
            ens.set_params(j, ps)
            if has_bn:
                ens.set_bn_state(j, *bn_out)
            ens.load(j)                                   # the engine is member j: one forward pass over the table, the member's rows picked from it
            o = eng.forward(L.EH_SPLIT_TRAIN)

            def obs_pred(ix):
                if len(ix) == 0:
                    return {}, None
                d = {t: targ[t][ix] for t in model.targets}
                d.update({t + "_pred": o[t][ix] for t in model.targets})
                return d, {k: v[ix] for k, v in o["parameters"].items()}
            tr_op, tr_diff = obs_pred(rows[j][0])
            va_op, va_diff = obs_pred(rows[j][1])
            st = {"fixed": fixed}
            if has_bn:
                st["st_nn"] = {"running_mean": bn_out[0], "running_var": bn_out[1]}
            h = history[j]
            results.append(TrainResults([s.l_train for s in h], [s.l_val for s in h], h, tr_op, va_op, tr_diff, va_diff, ps, st, best_epoch[j], best_loss[j]))
        return results
    finally:
        if ens is not None:
            ens.close()
        eng.close()


def train_folds(model: SingleNNHybridModel, data, folds, **train_kwargs) -> List[Optional[TrainResults]]:
    """k-fold cross-validation, the loop of docs/literate/tutorials/folds.jl in one call: one model per fold value v of `folds` (an array
    with one entry per retained row, or a column name), validated on the rows with folds == v and trained on the rest, all side by side
    (train_members).  Returns the results in the order of sorted(set(folds))."""
    f = np.asarray(_columns(data)[folds] if isinstance(folds, str) else folds)
    return train_members(model, data, [{"val_fold": v} for v in sorted(set(f.tolist()))], folds=folds, **train_kwargs)
