"""Host-side mirror of the reference's model constructor API.

  constructHybridModel(predictors, forcing, targets, mechanistic_model, parameters,
                       neural_param_names, global_param_names; hidden_layers=[32, 32], activation=tanh,
                       scale_nn_outputs=false, input_batchnorm=false, start_from_default=true)
                                                   -- src/models/GenericHybridModel.jl:89-140
  SingleNNHybridModel (alias HybridModel)          -- src/models/GenericHybridModel.jl:44-63
  build_parameters / ParameterContainer            -- src/models/helpers_for_HybridModel.jl:39-52,95-102
  scale_single_param, inv_sigmoid, ...             -- src/models/GenericHybridModel.jl:348-365

The reference accepts any Julia closure as `mechanistic_model`.  The engine has hand-derived device code
for the models of its registry (the reference's own RbQ10, Expo, Linear, Rs_components, FluxPart formulas
plus the build-defined two-pool Expo of BASELINE config 3), selected by name or by the tagged Python
callables below; any other callable `f(**forcings, **params) -> dict` of elementwise arithmetic is called
once with tracer values and handed to the device as a straight-line program (program.py, EH_MECH_PROGRAM),
which the step kernel evaluates and differentiates per sample.  What cannot be recorded raises
NotImplementedError -- never a silent CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L

# ---------------------------------------------------------------------------------------------
# mechanistic model registry (names = kwargs of the reference's Julia functions)
# ---------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class MechSpec:
    id: int
    name: str
    params: Tuple[str, ...]
    forcings: Tuple[str, ...]
    outputs: Tuple[str, ...]
    program: Optional[object] = None     # program.Program for a traced closure (id 6)
    fn: Optional[object] = None          # ... and the closure itself (an extra loss over several of its outputs traces it again, program.trace_extra_loss_mixed)


MECH_REGISTRY: Dict[str, MechSpec] = {
    "RbQ10": MechSpec(0, "RbQ10", ("rb", "Q10"), ("ta",), ("reco",)),
    "Expo_resp_model": MechSpec(1, "Expo_resp_model", ("Resp0", "k"), ("T",), ("Resp_obs",)),
    "LinearHM": MechSpec(2, "LinearHM", ("alpha", "beta"), ("x",), ("obs",)),
    "Expo2Pool": MechSpec(3, "Expo2Pool", ("R0a", "ka", "R0b", "kb"), ("T",), ("Resp_obs",)),
    "Rs_components": MechSpec(4, "Rs_components", ("Rb_het", "Rb_root", "Rb_myc", "Q10_het", "Q10_root", "Q10_myc"),
                              ("ta",), ("R_soil",)),
    "Rs_components3F": MechSpec(7, "Rs_components3F", ("Rb_het", "Rb_root", "Rb_myc", "Q10_het", "Q10_root", "Q10_myc"),
                                ("ta", "sw_in", "vpd"), ("R_soil",)),
    "FluxPartModelQ10": MechSpec(5, "FluxPartModelQ10", ("RUE", "Rb", "Q10"), ("SW_IN", "TA"), ("NEE", "GPP", "RECO")),
}


def _tag(name):
    def deco(fn):
        fn.eh_mech = MECH_REGISTRY[name]
        return fn
    return deco


@_tag("RbQ10")
def RbQ10(*, ta, Q10, rb, tref=15.0):
    """test/test_split_data_train.jl:36-39 (documentation of the formula; the device evaluates it)."""
    raise NotImplementedError("mechanistic models are evaluated on the device; this callable is a registry tag")


@_tag("Expo_resp_model")
def Expo_resp_model(*, T, Resp0, k):
    """projects/ExpoHybrid/ExpoHybridEstim.jl:69-85"""
    raise NotImplementedError("registry tag")


@_tag("LinearHM")
def LinearHM(*, x, alpha, beta):
    """src/models/LinearHM.jl:61-68"""
    raise NotImplementedError("registry tag")


@_tag("Expo2Pool")
def Expo2Pool(*, T, R0a, ka, R0b, kb):
    """build-defined: R0a*exp(ka*T) + R0b*exp(kb*T) (BASELINE.json config 3)"""
    raise NotImplementedError("registry tag")


@_tag("Rs_components")
def Rs_components(*, ta, Rb_het, Rb_root, Rb_myc, Q10_het, Q10_root, Q10_myc):
    """src/models/Rs_components.jl:40-57"""
    raise NotImplementedError("registry tag")


@_tag("Rs_components3F")
def Rs_components3F(*, ta, sw_in, vpd, Rb_het, Rb_root, Rb_myc, Q10_het, Q10_root, Q10_myc):
    """build-defined (BASELINE.json config 5, "3 forcings ... RbQ10-family M"): R_het + sw_in*R_root + vpd*R_myc with the pools of
    src/models/Rs_components.jl:45-55, R_c = Rb_c*Q10_c^(0.1(ta-15))"""
    raise NotImplementedError("registry tag")


@_tag("FluxPartModelQ10")
def FluxPartModelQ10(*, SW_IN, TA, RUE, Rb, Q10):
    """src/models/FluxPartModel_Q10_Lux.jl:50-79: GPP = SW_IN*RUE/12.011, RECO = Rb*Q10^(0.1(TA-15)), NEE = RECO - GPP"""
    raise NotImplementedError("registry tag")


def resolve_mech(m, params=None, forcing=None, targets=None) -> MechSpec:
    if isinstance(m, MechSpec):
        return m
    if isinstance(m, str):
        if m in MECH_REGISTRY:
            return MECH_REGISTRY[m]
        raise NotImplementedError(f"mechanistic model {m!r} is not in the device registry {sorted(MECH_REGISTRY)}")
    spec = getattr(m, "eh_mech", None)
    if spec is None:
        if not callable(m) or params is None:
            raise NotImplementedError(f"mechanistic model {m!r}: pass a registry name {sorted(MECH_REGISTRY)} or a callable")
        from .program import trace
        prog = trace(m, params, forcing, targets)      # GenericHybridModel.jl:420-425: f(; forcing..., params...)
        spec = MechSpec(L.EH_MECH_PROGRAM, getattr(m, "__name__", "closure"), prog.params, prog.forcings, prog.outputs, prog, m)
    return spec


# ---------------------------------------------------------------------------------------------
# parameter table + scaling helpers
# ---------------------------------------------------------------------------------------------


class ParameterContainer:
    """(default, lower, upper) table; helpers_for_HybridModel.jl:95-102, GenericHybridModel.jl:22-30."""

    def __init__(self, values: Dict[str, Tuple[float, float, float]]):
        for k, v in values.items():
            if len(v) != 3:
                raise ValueError(f"parameter {k} must be (default, lower, upper)")
        self.values = {k: tuple(np.float32(x) for x in v) for k, v in values.items()}

    def names(self):
        return list(self.values)

    def default(self, n): return self.values[n][0]
    def lower(self, n): return self.values[n][1]
    def upper(self, n): return self.values[n][2]


def build_parameters(parameters, f=None) -> ParameterContainer:
    return parameters if isinstance(parameters, ParameterContainer) else ParameterContainer(dict(parameters))


def sigmoid(x):
    x = np.asarray(x, np.float32)
    return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)


def inv_sigmoid(y):
    y = np.asarray(y, np.float32)
    return np.log(y / (1 - y))                                   # GenericHybridModel.jl:354


def scale_single_param(name, raw_val, hm: ParameterContainer):
    lo, hi = hm.lower(name), hm.upper(name)
    return lo + (hi - lo) * sigmoid(raw_val)                       # GenericHybridModel.jl:348-352


def scale_single_param_minmax(name, hm: ParameterContainer):
    lo, hi = hm.lower(name), hm.upper(name)
    return inv_sigmoid((hm.default(name) - lo) / (hi - lo))       # GenericHybridModel.jl:361-365


def hard_sigmoid(x):
    return np.clip(0.2 * np.asarray(x) + 0.5, 0.0, 1.0)           # GenericHybridModel.jl:9-11


def inv_hard_sigmoid(y):
    return (np.asarray(y) - 0.5) / 0.2                            # GenericHybridModel.jl:16-18


# ---------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------

_ACT_ALIASES = {"tanh": "tanh", "sigmoid": "sigmoid", "relu": "relu", "swish": "swish", "identity": "identity",
                "σ": "sigmoid", "sigmoid_fast": "sigmoid", "tanh_fast": "tanh"}
_ACT_GAIN = {"tanh": 5.0 / 3.0, "relu": math.sqrt(2.0), "sigmoid": 1.0, "swish": 1.0, "identity": 1.0}


def _act_name(a) -> str:
    name = a if isinstance(a, str) else getattr(a, "__name__", str(a))
    if name not in _ACT_ALIASES:
        raise NotImplementedError(f"activation {name!r} has no device implementation (have {sorted(set(_ACT_ALIASES.values()))})")
    return _ACT_ALIASES[name]


class RecordedActivation(str):
    """An activation given as a closure, recorded as a device program (program.trace_activation).  It stands where the name of a built-in
    activation stands -- model.activation, layer_activations, net_activations, config -- and is a string itself, "recorded:<name>:<digest
    of the program's words and constants>", so that everything that carries, compares, copies or prints those entries keeps working; the
    program rides along as `.program`.  Two closures that record to the same words and constants carry the same digest."""

    def __new__(cls, value, program=None):
        s = super().__new__(cls, value)
        s.program = program
        return s

    def __getnewargs__(self):                  # (copy / deepcopy / pickle)
        return (str(self), self.program)

    @classmethod
    def record(cls, fn):
        import hashlib
        from .program import trace_activation
        prog = trace_activation(fn)
        key = hashlib.sha1(repr((prog.words(), [np.float32(c).tobytes().hex() for c in prog.consts], prog.out)).encode()).hexdigest()[:12]
        name = getattr(fn, "__name__", type(fn).__name__).strip("<>")
        return cls(f"recorded:{name}:{key}", prog)

    def same_program(self, other) -> bool:
        p, q = self.program, other.program
        return p.words() == q.words() and [np.float32(c).tobytes() for c in p.consts] == [np.float32(c).tobytes() for c in q.consts] and p.out == q.out


def _is_recorded(a) -> bool:
    return isinstance(a, RecordedActivation)


def _act_of(a):
    """an `activation` argument -> the name of a built-in activation (strings and callables named like one, `np.tanh`: exactly as
    _act_name answers them), or the RecordedActivation of any other callable"""
    if isinstance(a, RecordedActivation):
        return a
    if isinstance(a, str) or not callable(a) or getattr(a, "__name__", None) in _ACT_ALIASES:
        return _act_name(a)
    return RecordedActivation.record(a)


def _act_gain(a) -> float:
    return 1.0 if _is_recorded(a) else _ACT_GAIN[a]       # (Lux: kaiming_uniform's default gain for a function it does not know)


# the common Lux / NNlib activations beyond the five built-in ones, as plain closures: they record like a user's own
def softplus(x):
    # NNlib: log1p(exp(-abs(x))) + relu(x), with relu written as (x + |x|) / 2: the reverse sweep takes |x|' = 0 at x = 0, which gives
    # softplus'(0) = 1/2 exactly (max(x, 0) would hand the whole derivative to one side there)
    return 0.5 * (x + abs(x)) + np.log(1.0 + np.exp(-abs(x)))


def elu(x):
    return np.where(x > 0.0, x, np.exp(np.minimum(x, 0.0)) - 1.0)         # alpha = 1; (the minimum keeps the branch not taken finite)


def leakyrelu(x):
    return np.where(x > 0.0, x, 0.01 * x)


def gelu_tanh(x):
    # 0.5 x (1 + tanh u), u = sqrt(2/pi) (x + 0.044715 x^3), in NNlib's form x sigmoid(2 u), the logistic written with its exponential:
    # the reverse sweep then never forms 1 - tanh(u)^2, whose cancellation gelu's chain rule would multiply by up to 5 (x near 4).
    # (the minimum keeps exp finite for x below -9, where the value is -0 and the derivative 0)
    v = 1.5957691216057308 * x * (1.0 + 0.044715 * x * x)
    return x / (1.0 + np.exp(np.minimum(-v, 80.0)))


def hard_sigmoid_act(x):
    return np.clip(0.2 * x + 0.5, 0.0, 1.0)                               # (hard_sigmoid above, without its np.asarray: that one is for parameter values)


class Dense:
    """Lux `Dense(in => out, activation)` as a DESCRIPTION of a layer (no weights): what `hidden_layers = Chain(...)` is made of."""

    def __init__(self, in_dims: int, out_dims: int, activation="identity"):
        self.in_dims, self.out_dims, self.activation = int(in_dims), int(out_dims), activation

    def __repr__(self):
        return f"Dense({self.in_dims} => {self.out_dims}, {self.activation if isinstance(self.activation, str) else getattr(self.activation, '__name__', self.activation)})"


class LSTMCell:
    """Lux `LSTMCell(in => out)` as a DESCRIPTION (defaults only: use_bias = true, train_state = false, zero initial h and c)."""

    def __init__(self, in_dims: int, out_dims: int):
        self.in_dims, self.out_dims = int(in_dims), int(out_dims)

    def __repr__(self):
        return f"LSTMCell({self.in_dims} => {self.out_dims})"


class GRUCell:
    """Lux `GRUCell(in => out)` as a DESCRIPTION (defaults only: use_bias = true, train_state = false, zero initial h).  Gate blocks
    [r | z | n]: h' = (1 - z) n + z h, n = tanh(W_in x + b_in + r (W_hn h + b_hn)) -- torch.nn.GRUCell's algebra and order."""

    def __init__(self, in_dims: int, out_dims: int):
        self.in_dims, self.out_dims = int(in_dims), int(out_dims)

    def __repr__(self):
        return f"GRUCell({self.in_dims} => {self.out_dims})"


class RNNCell:
    """Lux `RNNCell(in => out, activation)` as a DESCRIPTION (defaults only: use_bias = true, train_state = false, zero initial h):
    h' = activation(W_ih x + b_ih + W_hh h + b_hh), the activation one of the Dense layers' five (default tanh)."""

    def __init__(self, in_dims: int, out_dims: int, activation="tanh"):
        self.in_dims, self.out_dims, self.activation = int(in_dims), int(out_dims), _act_name(activation)

    def __repr__(self):
        return f"RNNCell({self.in_dims} => {self.out_dims}, {self.activation})"


class Recurrence:
    """Lux `Recurrence(cell; return_sequence)`.  The reference always runs it with return_sequence = true (NNModels.jl:172-176)."""

    def __init__(self, cell, return_sequence: bool = True):
        self.cell, self.return_sequence = cell, bool(return_sequence)

    def __repr__(self):
        return f"Recurrence({self.cell!r})"


class Dropout:
    """Lux `Dropout(p)` with `dims = :` as a DESCRIPTION: in training every unit of the hidden layer in front of it is zeroed with
    probability p and the others are multiplied by 1 / (1 - p); identity in evaluation.  The masks come from the engine's own
    counter-based generator (Philox4x32-10, keyed by the training seed), not from Julia's RNG stream."""

    def __init__(self, p, dims=None, **kwargs):
        if dims is not None or kwargs:
            raise NotImplementedError(f"Dropout(dims = {dims!r}{', ...' if kwargs else ''}): only the default dims = : (one draw per unit and sample) has a device kernel")
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"Dropout(p = {p!r}): the device kernels take 0 <= p < 1")
        self.p = p

    def __repr__(self):
        return f"Dropout({self.p})"


class BatchNorm:
    """Lux `BatchNorm(n, activation; affine, track_stats, momentum, epsilon)` as a DESCRIPTION of a layer inside `hidden_layers = Chain(...)`:
    in training y = activation(scale (x - mean_B) / sqrt(var_B + epsilon) + bias) over all rows of the minibatch, the gradient through both
    statistics; evaluation and predictions use the running statistics (start 0 / 1, moved by `momentum`, the variance by the unbiased
    estimate).  affine = True adds the leaves `scale` (ones) and `bias` (zeros); no weight_l2 term reads them."""

    def __init__(self, dims: int, activation="identity", affine: bool = True, track_stats: bool = True, momentum: float = 0.1, epsilon: float = 1e-5):
        if not track_stats:
            raise NotImplementedError("BatchNorm(track_stats = false): evaluation on the statistics of its own batch has no device kernel (the layer keeps running statistics)")
        self.dims, self.activation, self.affine, self.track_stats = int(dims), _act_name(activation), bool(affine), True
        self.momentum, self.epsilon = float(momentum), float(epsilon)
        if self.dims < 1:
            raise ValueError(f"BatchNorm({dims!r}): the layer needs at least one unit")
        if not 0.0 <= self.momentum <= 1.0 or not self.epsilon > 0.0:
            raise ValueError(f"BatchNorm(momentum = {momentum!r}, epsilon = {epsilon!r}): 0 <= momentum <= 1, epsilon > 0")

    def __repr__(self):
        return f"BatchNorm({self.dims}{'' if self.activation == 'identity' else ', ' + self.activation}{'' if self.affine else ', affine=false'})"


BN_LAYER = "bn:"          # the "activation" of a hidden layer that is BatchNorm(n, act): "bn:<act>", EH_LAYER_BATCHNORM + the activation's id
BN_LAYER_NOAFFINE = "bn0:"    # ... with affine = false: EH_LAYER_BATCHNORM + EH_LAYER_BN_NOAFFINE + the activation's id


def _bn_kind(a) -> int:
    """a hidden layer's "activation" -> 1 when the layer is a BatchNorm with scale / bias, 2 without, 0 otherwise"""
    if not isinstance(a, str):
        return 0
    return 1 if a.startswith(BN_LAYER) else (2 if a.startswith(BN_LAYER_NOAFFINE) else 0)


LAYERNORM_MAX_WIDTH = 1024      # a row of the layer lives in one wave's registers (csrc/eh_lnl.hpp, EH_MAX_LAYERNORM_WIDTH)


class LayerNorm:
    """Lux `LayerNorm(shape, activation; epsilon, dims, affine)` for a 1-D shape `(n,)` as a DESCRIPTION of a layer inside
    `hidden_layers = Chain(...)`: every sample over its own n features, y = activation(scale (x - mean(x)) / sqrt(var(x) + epsilon) + bias)
    with the biased variance, the gradient through both.  No state: training, evaluation and predictions run the same pass.  affine = True
    adds the leaves `bias` (zeros) and `scale` (ones), in that order; no weight_l2 term reads them."""

    def __init__(self, shape, activation="identity", affine: bool = True, epsilon: float = 1e-5, dims=None):
        if isinstance(shape, (tuple, list)):
            if len(shape) != 1:
                raise NotImplementedError(f"LayerNorm({tuple(shape)!r}): only a 1-D shape (n,) behind a layer of width n has a device kernel")
            shape = shape[0]
        if dims is not None:
            raise NotImplementedError(f"LayerNorm(dims = {dims!r}): only the default dims = : (all features of a sample) has a device kernel")
        self.dims, self.activation, self.affine, self.epsilon = int(shape), _act_name(activation), bool(affine), float(epsilon)
        if self.dims < 1:
            raise ValueError(f"LayerNorm({shape!r}): the layer needs at least one unit")
        if not self.epsilon > 0.0:
            raise ValueError(f"LayerNorm(epsilon = {epsilon!r}): epsilon > 0")
        if self.dims > LAYERNORM_MAX_WIDTH:
            raise NotImplementedError(f"LayerNorm({self.dims}): the device kernels take rows of up to {LAYERNORM_MAX_WIDTH} features")

    def __repr__(self):
        return f"LayerNorm({self.dims}, {self.activation})"


LN_LAYER = "ln:"          # the "activation" of a hidden layer that is LayerNorm(n, act): "ln:<act>", EH_LAYER_LAYERNORM + the activation's id
LN_LAYER_NOAFFINE = "ln0:"    # ... with affine = false: EH_LAYER_LAYERNORM + EH_LAYER_LN_NOAFFINE + the activation's id


def _ln_kind(a) -> int:
    """a hidden layer's "activation" -> 1 when the layer is a LayerNorm with bias / scale, 2 without, 0 otherwise"""
    if not isinstance(a, str):
        return 0
    return 1 if a.startswith(LN_LAYER) else (2 if a.startswith(LN_LAYER_NOAFFINE) else 0)


def _norm_leaves(a):
    """a hidden layer's "activation" -> None for a Dense or recurrent layer, otherwise the names of the normalisation layer's leaves in theta
    order: BatchNorm (scale, bias), LayerNorm (bias, scale), () with affine = false"""
    if _bn_kind(a):
        return ("scale", "bias") if _bn_kind(a) == 1 else ()
    if _ln_kind(a):
        return ("bias", "scale") if _ln_kind(a) == 1 else ()
    return None


def _split_dropout(hidden_layers):
    """Chain with Dropout layers -> (the Chain without them, [p_0 .. p_{L-1}] per hidden layer or None).  A Dropout belongs to the hidden
    layer in front of it; as the first element that is the layer the reference prepends (Dense(in_dim, first_h, activation)).
    Dropout(0) is Lux's NoOpLayer and disappears.  Chains around a Recurrence are left to _hidden_widths (and its refusals)."""
    if not isinstance(hidden_layers, Chain) or not any(isinstance(l, Dropout) for l in hidden_layers.layers):
        return hidden_layers, None
    if any(isinstance(l, (Recurrence, BatchNorm, LayerNorm)) for l in hidden_layers.layers):
        return hidden_layers, None
    rest, rates, prev = [], {}, False
    for i, l in enumerate(hidden_layers.layers):
        if isinstance(l, Dropout):
            if prev:
                raise NotImplementedError(f"hidden_layers Chain: layers {i} and {i + 1} are both Dropout; two Dropout layers in a row have no device kernel (write one with the combined rate)")
            prev = True
            if l.p > 0.0:
                rates[len(rest)] = l.p
        else:
            prev = False
            rest.append(l)
    n = len(rest) + 1
    return Chain(*rest), ([rates.get(l, 0.0) for l in range(n)] if rates else None)


DROPOUT_MAX_WIDTH, DROPOUT_MAX_LAYERS = 64, 3      # the per-wave fused kernel family (csrc/eh_device.hpp)


LSTM_LAYER = "lstm"      # the "activation" of a hidden layer that is Recurrence(LSTMCell): EH_LAYER_LSTM in the descriptor
GRU_LAYER = "gru"        # ... Recurrence(GRUCell): EH_LAYER_GRU
RNN_LAYER = "rnn:"       # ... Recurrence(RNNCell(.., act)): "rnn:<act>", EH_LAYER_RNN + the activation's id
CELL_GATES = {"lstm": 4, "gru": 3, "rnn": 1}      # gate blocks of H rows in weight_ih / weight_hh / bias_ih / bias_hh


def _cell_kind(a) -> Optional[str]:
    """a hidden layer's "activation" -> "lstm" | "gru" | "rnn" when the layer is a Recurrence, None when it is a Dense layer"""
    if a == LSTM_LAYER or a == GRU_LAYER:
        return a
    return "rnn" if isinstance(a, str) and a.startswith(RNN_LAYER) else None


def _layer_code(a: str) -> int:
    """net_activation[l] of the descriptor"""
    kind = _cell_kind(a)
    if _bn_kind(a) == 1:
        return L.EH_LAYER_BATCHNORM + L.ACTIVATIONS[a[len(BN_LAYER):]]
    if _bn_kind(a) == 2:
        return L.EH_LAYER_BATCHNORM + L.EH_LAYER_BN_NOAFFINE + L.ACTIVATIONS[a[len(BN_LAYER_NOAFFINE):]]
    if _ln_kind(a) == 1:
        return L.EH_LAYER_LAYERNORM + L.ACTIVATIONS[a[len(LN_LAYER):]]
    if _ln_kind(a) == 2:
        return L.EH_LAYER_LAYERNORM + L.EH_LAYER_LN_NOAFFINE + L.ACTIVATIONS[a[len(LN_LAYER_NOAFFINE):]]
    if kind == "rnn":
        return L.EH_LAYER_RNN + L.ACTIVATIONS[a[len(RNN_LAYER):]]
    return {"lstm": L.EH_LAYER_LSTM, "gru": L.EH_LAYER_GRU}[kind] if kind else L.ACTIVATIONS[a]


class Chain:
    """`hidden_layers::Chain` (NNModels.jl:145-219): the user gives the HIDDEN layers only; the reference wraps them as
    Dense(in_dim, first_h, activation) -> layers... -> Dense(last_h, out_dim), first_h / last_h read off the chain's own dimensions."""

    def __init__(self, *layers):
        self.layers = list(layers)


def _hidden_widths(hidden_layers, act: str, per_layer: bool = False):
    """hidden_layers as the vector of widths the device kernels are built around.  A Chain of Dense layers IS such a vector --
    [first_h, out_1, ..., out_n], the first hidden layer (the one the reference puts in front, Dense(in_dim, first_h, activation)) using
    the model's `activation` and layer i the one it was written with (NNModels.jl:205-211).  Other layer types have no kernel and are
    refused with the reason.  per_layer: also return the hidden layers' activations when they are not all the model's (None otherwise);
    without it such a chain is refused (the MultiNN form: its networks differ by network, not by layer)."""
    if isinstance(hidden_layers, Chain):
        ls = hidden_layers.layers
        if not ls:
            raise ValueError("hidden_layers: an empty Chain has no dimensions (NNModels.jl: 'Could not determine input dimension of hidden_layers Chain.')")
        if any(isinstance(l, (BatchNorm, LayerNorm)) for l in ls):
            return _bn_chain_widths(ls, act, per_layer)
        if any(isinstance(l, Recurrence) for l in ls):
            # a chain that ends in Recurrence(LSTMCell) gets its sequence head (NNModels.jl:171-211):
            # Dense(in_dim, I, act) -> Recurrence(LSTMCell(I => H)) -> RecurrenceOutputDense(H => H, act) -> Dense(H, out_dim), per time step
            if not per_layer:
                raise NotImplementedError("hidden_layers Chain: Recurrence layers in a MultiNN model have no device kernel (sequence models are single-network)")
            if _is_recorded(act):
                raise NotImplementedError("a recorded activation (a closure) around a Recurrence: the sequence kernels are built ahead of time around the five built-in activations")
            if len(ls) != 1:
                raise NotImplementedError(f"hidden_layers Chain: {len(ls)} layers around a Recurrence; the device kernel holds Chain(Recurrence(LSTMCell(I => H))) "
                                          "alone (stacked or non-final Recurrence layers are not built)")
            r = ls[0]
            if not isinstance(r.cell, (LSTMCell, GRUCell, RNNCell)):
                raise NotImplementedError(f"hidden_layers Chain: Recurrence({type(r.cell).__name__}); only LSTMCell, GRUCell and RNNCell have a device kernel")
            if not r.return_sequence:
                raise NotImplementedError("hidden_layers Chain: Recurrence(return_sequence = false) is not built (the reference always sets it true)")
            cell = LSTM_LAYER if isinstance(r.cell, LSTMCell) else (GRU_LAYER if isinstance(r.cell, GRUCell) else RNN_LAYER + r.cell.activation)
            return [r.cell.in_dims, r.cell.out_dims, r.cell.out_dims], [act, cell, act]
        acts = [act]
        for i, l in enumerate(ls):
            if not isinstance(l, Dense):
                raise NotImplementedError(f"hidden_layers Chain: layer {i + 1} is {type(l).__name__}; only Dense layers have a device kernel")
            acts.append(_act_of(l.activation))
            if acts[-1] != act and not per_layer:
                raise NotImplementedError(f"hidden_layers Chain: layer {i + 1} uses {acts[-1]!r}, the model {act!r}: the networks of a MultiNN model "
                                          "apply ONE activation to all their hidden layers (per NETWORK activations exist: activation = {...}; "
                                          "a single network takes an activation per layer)")
            if i and l.in_dims != ls[i - 1].out_dims:
                raise ValueError(f"hidden_layers Chain: layer {i + 1} takes {l.in_dims} inputs, layer {i} gives {ls[i - 1].out_dims}")
        widths = [ls[0].in_dims] + [l.out_dims for l in ls]
        return (widths, acts if any(a != act for a in acts) else None) if per_layer else widths
    if not isinstance(hidden_layers, (list, tuple)):
        raise NotImplementedError(f"hidden_layers of type {type(hidden_layers).__name__}: pass the widths or a Chain of Dense layers")
    widths = [int(h) for h in hidden_layers]
    return (widths, None) if per_layer else widths


def _bn_chain_widths(ls, act: str, per_layer: bool):
    """a Chain that holds BatchNorm / LayerNorm layers next to Dense layers -> (widths, activations) with one entry per hidden layer of the
    descriptor: the Dense layer the reference puts in front (first_h read off the chain's first layer -- a normalisation layer's dims,
    NNModels.jl:156-169), then every layer of the chain, a BatchNorm / LayerNorm as an entry as wide as the layer in front of it"""
    what = "BatchNorm" if any(isinstance(l, BatchNorm) for l in ls) else "LayerNorm"      # (the messages name the kind the chain holds; both: BatchNorm's)
    if not per_layer:
        raise NotImplementedError(f"hidden_layers Chain: {what} layers in a MultiNN model have no device kernel (they are built for single-network models)")
    if any(isinstance(l, Recurrence) for l in ls):
        raise NotImplementedError(f"hidden_layers Chain: a {what} layer next to a Recurrence has no device kernel (sequence models take no {what})")
    if any(isinstance(l, Dropout) for l in ls):
        raise NotImplementedError(f"hidden_layers Chain: a {what} layer next to a Dropout has no device kernel (dropout runs on the fused per-wave kernels, {what} layer by layer)")
    if _is_recorded(act) or any(isinstance(l, Dense) and _is_recorded(_act_of(l.activation)) for l in ls):
        raise NotImplementedError(f"hidden_layers Chain: a recorded activation (a closure) next to a {what} layer has no device kernel ({what} chains run layer by layer, "
                                  "on kernels built ahead of time around the five built-in activations)")
    first = ls[0].dims if isinstance(ls[0], (BatchNorm, LayerNorm)) else getattr(ls[0], "in_dims", None)
    widths, acts, w = [first], [act], first
    for i, l in enumerate(ls):
        if isinstance(l, BatchNorm):
            if l.dims != w:
                raise ValueError(f"hidden_layers Chain: layer {i + 1} is BatchNorm({l.dims}), the layer in front of it gives {w}")
            acts.append((BN_LAYER if l.affine else BN_LAYER_NOAFFINE) + l.activation)
        elif isinstance(l, LayerNorm):
            if l.dims != w:
                raise ValueError(f"hidden_layers Chain: layer {i + 1} is LayerNorm({l.dims}), the layer in front of it gives {w}")
            acts.append((LN_LAYER if l.affine else LN_LAYER_NOAFFINE) + l.activation)
        elif isinstance(l, Dense):
            if l.in_dims != w:
                raise ValueError(f"hidden_layers Chain: layer {i + 1} takes {l.in_dims} inputs, the layer in front of it gives {w}")
            w = l.out_dims
            acts.append(_act_name(l.activation))
        else:
            raise NotImplementedError(f"hidden_layers Chain: layer {i + 1} is {type(l).__name__}; only Dense, BatchNorm and LayerNorm layers have a device kernel here")
        widths.append(w)
    return widths, acts


def _distinct_recorded(acts):
    seen: List[RecordedActivation] = []
    for a in acts:
        if _is_recorded(a) and not any(r.same_program(a) for r in seen):
            seen.append(a)
            yield a


def _recorded_refusals(acts, widths, n_pred: int, n_out: int, kwargs: dict, dropout):
    """where a recorded activation does not run, each with its reason, ahead of any upload (the library's planner answers the same
    descriptors the same way: csrc/eh_plan.hpp)"""
    n_rec = sum(1 for _ in _distinct_recorded(acts))
    if n_rec > L.EH_MAX_ACT_PROGS:
        raise NotImplementedError(f"{n_rec} distinct recorded activations in one model (device limit {L.EH_MAX_ACT_PROGS}; identical programs count once)")
    if kwargs.get("precision", "f32") != "f32":
        raise NotImplementedError(f"precision = {kwargs['precision']!r} with a recorded activation: the bf16 kernels keep only the rounded activation, "
                                  "a recorded activation takes value and derivative from the pre-activation (fp32 only)")
    if dropout is not None:
        raise NotImplementedError("hidden_layers Chain: Dropout next to a recorded activation has no device kernel (the dropout kernels are built around the five built-in activations)")
    w, nl = max(widths), len(widths)
    if w > 128 or nl > 3 or (w > 64 and nl > 2) or n_pred > 32 or n_out > 16:
        raise NotImplementedError(f"a recorded activation on hidden layers {list(widths)} ({n_pred} predictors, {n_out} outputs): recorded activations are built for the fused "
                                  "kernels (up to 32 predictors and 16 outputs; widths up to 64 with at most 3 hidden layers, or up to 128 with at most 2), this network would run "
                                  "in the layer-wise form, whose activations live in kernels built ahead of time")


@dataclass
class SingleNNHybridModel:
    """Field-for-field mirror of the reference struct (GenericHybridModel.jl:44-63); `NN` is the
    list of Dense (out, in) shapes that prepare_hidden_chain (NNModels.jl:220-231) would build."""
    NN: List[Tuple[int, int]]
    predictors: List[str]
    forcing: List[str]
    targets: List[str]
    mechanistic_model: MechSpec
    parameters: ParameterContainer
    neural_param_names: List[str]
    global_param_names: List[str]
    fixed_param_names: List[str]
    scale_nn_outputs: bool
    start_from_default: bool
    config: dict = field(default_factory=dict)
    # MultiNNHybridModel: NNs[name] = Dense shapes of the single-output net predicting `name`, predictor_sets[name] = its columns
    NNs: Optional[Dict[str, List[Tuple[int, int]]]] = None
    predictor_sets: Optional[Dict[str, List[str]]] = None
    net_activations: Optional[List[str]] = None      # MultiNN with activation::NamedTuple: the activation of net k (None = one for all)
    layer_activations: Optional[List[str]] = None    # single network from `hidden_layers::Chain` whose layers differ: the activation of hidden layer l (None = one for all)
    dropout: Optional[List[float]] = None            # `hidden_layers::Chain` with Dropout layers: the rate behind hidden layer l (None = none anywhere)
    batchnorm: Optional[Dict[int, Tuple[float, float]]] = None      # `hidden_layers::Chain` with BatchNorm layers: hidden layer l -> (momentum, epsilon) (None = none anywhere)
    layernorm: Optional[Dict[int, float]] = None     # ... with LayerNorm layers: hidden layer l -> epsilon (None = none anywhere)

    # -- sizes ---------------------------------------------------------------------------------
    @property
    def hidden_layers(self) -> List[int]:
        return [o for o, _ in self.NN[:-1]]

    @property
    def nets(self) -> List[List[Tuple[int, int]]]:
        if not self.NN and self.NNs is None:
            return []                  # no neural parameter: `NN = Chain()` (GenericHybridModel.jl:112-125), theta holds the raw globals only
        return [self.NN] if self.NNs is None else [self.NNs[k] for k in self.neural_param_names]

    @property
    def lstm_layer(self) -> Optional[int]:
        """index into NN of the layer that is a Recurrence (sequence models; the name is from when LSTMCell was the one cell), or None"""
        for l, a in enumerate(self.layer_activations or ()):
            if _cell_kind(a) is not None:
                return l
        return None

    @property
    def cell(self) -> Optional[str]:
        """"lstm" | "gru" | "rnn" of a sequence model, None otherwise"""
        ll = self.lstm_layer
        return None if ll is None else _cell_kind(self.layer_activations[ll])

    @property
    def cell_activation(self) -> Optional[str]:
        """the activation of a sequence model's RNNCell, None otherwise"""
        return self.layer_activations[self.lstm_layer][len(RNN_LAYER):] if self.cell == "rnn" else None

    @property
    def bn_layers(self) -> List[int]:
        """the hidden layers (indices into NN, = the descriptor's) that are BatchNorm layers, in chain order"""
        return [l for l, a in enumerate(self.layer_activations or ()) if _bn_kind(a)]

    @property
    def ln_layers(self) -> List[int]:
        """the hidden layers that are LayerNorm layers, in chain order"""
        return [l for l, a in enumerate(self.layer_activations or ()) if _ln_kind(a)]

    @property
    def norm_layers(self) -> List[int]:
        """bn_layers and ln_layers together: the hidden layers that are no Dense layers but normalise the one in front of them"""
        return [l for l, a in enumerate(self.layer_activations or ()) if _norm_leaves(a) is not None]

    def leaves(self):
        """[(network index, layer index, leaf name, shape)] of the networks in ComponentArray order: Dense layers have `weight` (out, in) and
        `bias`; the recurrent layer `weight_ih` (nH, I), `weight_hh` (nH, H), `bias_ih`, `bias_hh` (nH): n = 4 gate blocks [i | f | g | o] of
        an LSTMCell, 3 [r | z | n] of a GRUCell, 1 of an RNNCell"""
        out, ll = [], self.lstm_layer
        ng = CELL_GATES.get(self.cell, 0)
        for k, net in enumerate(self.nets):
            for li, (o, i) in enumerate(net):
                norm = _norm_leaves(self.layer_activations[li]) if (self.layer_activations is not None and li < len(self.layer_activations)) else None
                if norm is not None:       # BatchNorm: `scale` and `bias`; LayerNorm: `bias` and `scale` (affine), or nothing
                    out += [(k, li, name, (o,)) for name in norm]
                elif ll is not None and li == ll:
                    out += [(k, li, "weight_ih", (ng * o, i)), (k, li, "weight_hh", (ng * o, o)), (k, li, "bias_ih", (ng * o,)), (k, li, "bias_hh", (ng * o,))]
                else:
                    out += [(k, li, "weight", (o, i)), (k, li, "bias", (o,))]
        return out

    @property
    def n_nn(self) -> int:
        return sum(int(np.prod(shape)) for _, _, _, shape in self.leaves())

    @property
    def n_theta(self) -> int:
        return self.n_nn + len(self.global_param_names)

    @property
    def activation(self):
        """the name, or {network: name} when the networks differ (the reference keeps the NamedTuple in `config`)"""
        return self.config["activation"]

    def activation_of(self, k: int, layer: Optional[int] = None) -> str:
        if self.layer_activations is not None and layer is not None:
            return self.layer_activations[layer]
        return self.config["activation"] if self.net_activations is None else self.net_activations[k]

    # -- LuxCore.initialparameters analogue (GenericHybridModel.jl:236-256) ----------------------
    def initialparameters(self, rng: Union[int, np.random.Generator] = 0) -> np.ndarray:
        """Flat theta in the reference's ComponentArray order.  Lux >= 1.0 Dense defaults (third
        party, from its docs): weight kaiming_uniform with the activation's gain, bias
        U(+-1/sqrt(fan_in)).  NumPy's stream, not Julia's Xoshiro -- parity tests inject theta."""
        rng = np.random.default_rng(rng) if not isinstance(rng, np.random.Generator) else rng
        parts = []
        for k, net in enumerate(self.nets):
            for li, (o, i) in enumerate(net):
                if li in self.norm_layers:     # BatchNorm, LayerNorm: scale = ones, bias = zeros (affine), or no leaf at all
                    parts += [np.ones(o, np.float32) if name == "scale" else np.zeros(o, np.float32) for name in _norm_leaves(self.layer_activations[li])]
                    continue
                if li == self.lstm_layer:      # LSTMCell, GRUCell, RNNCell: every leaf U(+-1/sqrt(H))
                    bh = 1 / math.sqrt(o)
                    parts += [rng.uniform(-bh, bh, shape).astype(np.float32).flatten(order="F") for _, l2, _, shape in self.leaves() if l2 == li]
                    continue
                gain = _act_gain(self.activation_of(k, li)) if li < len(net) - 1 else 1.0      # (a Dense layer in front of a BatchNorm keeps the gain of its own activation)
                bw = gain * math.sqrt(3.0 / i)
                parts.append(rng.uniform(-bw, bw, (o, i)).astype(np.float32).flatten(order="F"))
                parts.append(rng.uniform(-1 / math.sqrt(i), 1 / math.sqrt(i), o).astype(np.float32))
        for g in self.global_param_names:
            if self.start_from_default:
                parts.append(np.asarray([scale_single_param_minmax(g, self.parameters)], np.float32))
            else:
                parts.append(rng.random(1).astype(np.float32))
        return np.concatenate(parts).astype(np.float32)

    def weight_mask(self) -> np.ndarray:
        """True at the flat-theta positions of the Dense weight matrices (the leaves weight_l2 sums, src/utils/extract_weights.jl:69-91)"""
        m = np.zeros(self.n_theta, bool)
        off = 0
        for _, _, name, shape in self.leaves():      # (a cell's leaves are weight_ih / weight_hh: not matched)
            n = int(np.prod(shape))
            m[off:off + n] = name == "weight"
            off += n
        return m

    def l2_mask(self, net=None, key: str = "weight") -> np.ndarray:
        """the flat-theta positions weight_l2(ps or ps.<net>; key) walks (extract_weights.jl:69-91): the leaves named `key`
        (:weight or :bias) of every network, or of the network predicting `net` (a MultiNNHybridModel's `ps.<net>`)"""
        if key not in ("weight", "bias"):
            raise ValueError(f"weight_l2: key = {key!r} (Dense layers have :weight and :bias leaves)")
        names = [None] if self.NNs is None else list(self.neural_param_names)
        if net is not None and net not in names:
            raise KeyError(f"weight_l2: no network named {net!r} (networks: {[n for n in names if n is not None]})")
        m = np.zeros(self.n_theta, bool)
        off, bn = 0, set(self.norm_layers)
        for k, li, leaf, shape in self.leaves():
            n = int(np.prod(shape))
            if (net is None or net == names[k]) and leaf == key and li not in bn:      # (extract_weights.jl:24: a BatchNorm's / LayerNorm's scale / bias are skipped)
                m[off:off + n] = True
            off += n
        return m

    def l2_coefficients(self, terms) -> np.ndarray:
        """terms [WeightL2...] -> one coefficient per flat-theta entry: sum of the terms == sum_i coef[i] * theta_i^2 (eh_set_weight_l2_coef)"""
        c = np.zeros(self.n_theta, np.float64)
        for t in terms:
            m = self.l2_mask(t.net, t.key)
            n = int(m.sum())
            c[m] += float(t.lam) / (n if t.normalize and n > 0 else 1)
        return c.astype(np.float32)

    def unpack(self, theta: np.ndarray):
        """flat theta -> (ps = [(weight (out,in), bias)...], {global: raw})"""
        off, nets = 0, []
        if self.norm_layers:                 # a BatchNorm / LayerNorm layer unpacks to a dict of its leaves ({} with affine = false)
            layers = [{} if li in self.norm_layers else [None, None] for li in range(len(self.NN))]
            for _, li, name, shape in self.leaves():
                n = int(np.prod(shape))
                v = theta[off:off + n].reshape(shape, order="F") if len(shape) == 2 else theta[off:off + n]
                off += n
                if li in self.norm_layers:
                    layers[li][name] = v
                else:
                    layers[li][0 if name == "weight" else 1] = v
            return [l if isinstance(l, dict) else tuple(l) for l in layers], {g: theta[off + j:off + j + 1] for j, g in enumerate(self.global_param_names)}
        if self.lstm_layer is not None:      # sequence model: the recurrent layer unpacks to a dict of its four leaves
            layers, cur = [], {}
            for _, li, name, shape in self.leaves():
                n = int(np.prod(shape))
                cur[name] = theta[off:off + n].reshape(shape, order="F") if len(shape) == 2 else theta[off:off + n]
                off += n
                if name in ("bias", "bias_hh"):
                    layers.append(cur if li == self.lstm_layer else (cur["weight"], cur["bias"]))
                    cur = {}
            return layers, {g: theta[off + j:off + j + 1] for j, g in enumerate(self.global_param_names)}
        for net in self.nets:
            layers = []
            for o, i in net:
                W = theta[off:off + o * i].reshape((o, i), order="F"); off += o * i
                b = theta[off:off + o]; off += o
                layers.append((W, b))
            nets.append(layers)
        glob = {g: theta[off + j:off + j + 1] for j, g in enumerate(self.global_param_names)}
        return ((nets[0] if nets else []) if self.NNs is None else dict(zip(self.neural_param_names, nets))), glob

    def opt_branches(self) -> Dict[str, Tuple[int, int]]:
        """top-level branches of the parameter tree -> their [lo, hi) in flat theta, in ComponentArray order (what a per-branch
        TrainConfig.opt names, src/training/train.jl:78-93): the network `ps` of one network (empty without one: the reference's
        `Chain()`), one branch per network of a MultiNN model, named by its neural parameter, then each global parameter"""
        out, off = {}, 0
        names = ["ps"] if self.NNs is None else list(self.neural_param_names)
        nets = self.nets if self.nets else [[]]
        for name, net in zip(names, nets):
            n = self.n_nn if (self.lstm_layer is not None or self.norm_layers) else sum(o * i + o for o, i in net)
            out[name] = (off, off + n)
            off += n
        for g in self.global_param_names:
            out[g] = (off, off + 1)
            off += 1
        return out

    def act_programs(self) -> List["RecordedActivation"]:
        """the model's distinct recorded activations in order of first appearance; identical programs (same words and constants) count once"""
        cands = list(self.net_activations or self.layer_activations or [])
        if not cands and _is_recorded(self.config.get("activation")):
            cands = [self.config["activation"]]
        out: List[RecordedActivation] = []
        for a in cands:
            if _is_recorded(a) and not any(r.same_program(a) for r in out):
                out.append(a)
        return out

    def act_program_structs(self):
        """the eh_act_program array eh_create_activations takes, or None"""
        progs = self.act_programs()
        if not progs:
            return None
        arr = (L.ActProgram * len(progs))()
        for j, r in enumerate(progs):
            pg = r.program
            arr[j].n_instr, arr[j].n_const, arr[j].out_slot = len(pg.code), len(pg.consts), pg.out[0]
            for i, w in enumerate(pg.words()):
                arr[j].code[i] = w
            for i, c in enumerate(pg.consts):
                arr[j].consts[i] = c
        return arr

    # -- C descriptor ----------------------------------------------------------------------------
    def to_desc(self, device: int = 0, extra_outputs=(), mech: Optional[MechSpec] = None) -> L.ModelDesc:
        ms = mech if mech is not None else self.mechanistic_model      # (mech: the model's closure with the extra loss's entries as outputs of their own)
        d = L.ModelDesc()
        d.struct_size = __import__("ctypes").sizeof(L.ModelDesc)
        d.device = device
        d.n_predictors = len(self.predictors)
        hl = self.hidden_layers
        if not (1 if self.NN else 0) <= len(hl) <= L.EH_MAX_HIDDEN:
            raise NotImplementedError(f"{len(hl)} hidden layers (device kernels: 1..{L.EH_MAX_HIDDEN})")
        d.n_hidden = len(hl)
        for k, w in enumerate(hl):
            d.hidden[k] = w
        if self.NNs is not None:
            if len(self.NNs) > L.EH_MAX_NETS:
                raise NotImplementedError(f"{len(self.NNs)} neural networks (device limit {L.EH_MAX_NETS})")
            d.n_nets = len(self.NNs)
            for k, name in enumerate(self.neural_param_names):
                net = self.NNs[name]
                d.net_n_predictors[k] = net[0][1]
                d.net_depth[k] = len(net) - 1
                for l, (o, _) in enumerate(net[:-1]):
                    d.net_hidden[k][l] = o
        progs = self.act_programs()                # recorded activations: program j is what the id EH_ACT_RECORDED + j names

        def code(a):
            return L.EH_ACT_RECORDED + next(j for j, r in enumerate(progs) if r.same_program(a)) if _is_recorded(a) else _layer_code(a)
        if self.net_activations is not None:       # per-net activations: kernels compiled at run time around the descriptor
            d.activation = L.EH_ACT_PER_NET
            for k, a in enumerate(self.net_activations):
                d.net_activation[k] = code(a)
        elif self.layer_activations is not None:   # an activation per hidden layer (n_nets = 0): net_activation[l] is layer l's
            d.activation = L.EH_ACT_PER_NET
            for l, a in enumerate(self.layer_activations):
                d.net_activation[l] = code(a)
        elif _is_recorded(self.activation):        # one recorded activation for all: still the per-net / per-layer form, every entry naming it
            d.activation = L.EH_ACT_PER_NET
            for k in range(len(self.NNs) if self.NNs is not None else len(hl)):
                d.net_activation[k] = code(self.activation)
        else:
            d.activation = L.ACTIVATIONS[self.activation]
        d.scale_nn_outputs = int(self.scale_nn_outputs)
        d.input_batchnorm = int(bool(self.config.get("input_batchnorm", False)))
        d.mech = ms.id
        d.n_params = len(ms.params)
        for j, p in enumerate(ms.params):
            if p in self.neural_param_names:
                d.param_kind[j], d.param_index[j] = L.PAR_NEURAL, self.neural_param_names.index(p)
            elif p in self.global_param_names:
                d.param_kind[j], d.param_index[j] = L.PAR_GLOBAL, self.global_param_names.index(p)
            else:
                d.param_kind[j], d.param_index[j] = L.PAR_FIXED, 0
            d.param_default[j] = self.parameters.default(p)
            d.param_lower[j] = self.parameters.lower(p)
            d.param_upper[j] = self.parameters.upper(p)
        d.n_forcings = len(self.forcing)
        for f, name in enumerate(ms.forcings):
            d.forcing_index[f] = self.forcing.index(name)
        # (extra_outputs: entries of an extra loss that is a function of the predictions ride on targets of their own, behind the data
        #  targets -- include/easyhybrid_hip.h: eh_set_target_roles; each observes the output its entry reads)
        all_t = list(self.targets) + list(extra_outputs)
        if len(all_t) > L.EH_MAX_TARG:
            raise NotImplementedError(f"{len(self.targets)} targets + {len(extra_outputs)} extra-loss entries of the predictions: the device holds {L.EH_MAX_TARG} in all")
        d.n_targets = len(all_t)
        for t, name in enumerate(all_t):
            d.target_output[t] = ms.outputs.index(name)
        if ms.program is not None:
            pg = ms.program
            d.prog_len, d.prog_n_const, d.prog_n_forc, d.prog_n_out = len(pg.code), len(pg.consts), len(pg.forcings), len(pg.out)
            for i, w in enumerate(pg.words()):
                d.prog_code[i] = w
            for i, c in enumerate(pg.consts):
                d.prog_const[i] = c
            for i, o in enumerate(pg.out):
                d.prog_out[i] = o
        return d

    def engine(self, device: int = 0, extra_fn=None):
        """precision (a build extension, BASELINE.json config 5; the reference is Float32 end to end; csrc/eh_wide_bf16.hpp):
        "bf16_fwd" = Dense products of the forward pass on bf16 operands with fp32 accumulation, fp32-exact backward;
        "bf16" = bf16 operands in both passes (every backward delta rounded to bf16 once), fp32 accumulation."""
        from .engine import HybridEngine
        entries, mech = [], None
        if extra_fn is not None:                      # extra_loss(yhat[, ps]) of the predictions: recorded, one more target per entry
            from .program import trace_extra_loss, trace_extra_loss_mixed
            ms = self.mechanistic_model
            try:
                entries = trace_extra_loss(extra_fn, list(self.targets))
            except (NotImplementedError, KeyError, TypeError) as e:
                # an entry over several predictions, over outputs that are no targets, or over predictions and global parameters
                # (compute_loss.jl:31-34): possible where the mechanistic model is a recorded closure -- its per-sample expression
                # becomes one more output of the model's program
                if ms.fn is None:
                    raise NotImplementedError(f"extra_loss: {e} -- entries that mix predictions (or read global parameters) need the mechanistic model "
                                              f"as a Python closure (the recorder adds them to its program); {ms.name!r} is a built-in of the device registry") from e
                bounds = {p: (float(self.parameters.lower(p)), float(self.parameters.upper(p))) for p in self.global_param_names}
                prog, entries = trace_extra_loss_mixed(ms.fn, extra_fn, list(ms.params), list(self.forcing), list(self.targets), list(self.global_param_names), bounds)
                mech = MechSpec(ms.id, ms.name, prog.params, prog.forcings, prog.outputs, prog, ms.fn)
        eng = HybridEngine(self.to_desc(device, [e[1] for e in entries], mech), len(self.mechanistic_model.params), self.targets,
                           list(self.mechanistic_model.params), n_pseudo=len(entries), act_programs=self.act_program_structs())
        if entries:
            eng.set_extra_entries(entries)
        prec = self.config.get("precision", "f32")
        if prec not in ("f32", "bf16_fwd", "bf16"):
            raise ValueError(f"precision {prec!r}: 'f32', 'bf16_fwd' or 'bf16'")
        try:
            if prec != "f32":
                eng.set_option("precision", 1 if prec == "bf16_fwd" else 2)
            if self.dropout is not None:                  # (train() sets the seed of its run and the step it continues from)
                eng.set_dropout(self.dropout, seed=0, step=0)
            for l, (mom, eps) in (self.batchnorm or {}).items():
                if (mom, eps) != (0.1, 1e-5):
                    eng.set_layer_norm(l, mom, eps)
            for l, eps in (self.layernorm or {}).items():
                if eps != 1e-5:
                    eng.set_layer_norm(l, epsilon=eps)
        except Exception:
            eng.close()
            raise
        return eng


HybridModel = SingleNNHybridModel     # spelling used by BASELINE.json's north_star


def _construct_multi(predictors: Dict[str, Sequence[str]], forcing, targets, mechanistic_model, parameters, global_param_names, *,
                     hidden_layers, activation, scale_nn_outputs, input_batchnorm, start_from_default, **kwargs):
    """MultiNNHybridModel: one single-output MLP per key of `predictors` (= neural parameter) on its own predictor set."""
    parameters = build_parameters(parameters, mechanistic_model)
    ms = resolve_mech(mechanistic_model, parameters.names(), list(forcing), list(targets))
    all_names = parameters.names()
    neural = list(predictors)
    glob = list(global_param_names or [])
    if not all(n in all_names for n in neural):
        raise AssertionError("neural_param_names ⊆ param_names")
    net_acts = None
    if isinstance(activation, dict):               # activation::NamedTuple (GenericHybridModel.jl:168-176)
        if not isinstance(hidden_layers, dict):    # the reference reads activation[nn_name] only next to hidden_layers[nn_name]
            raise TypeError("activation given per network needs hidden_layers given per network as well")
        net_acts = [_act_of(activation[k]) for k in neural]
        act = net_acts[0]
        if len(set(net_acts)) == 1:
            net_acts = None
    else:
        act = _act_of(activation)
    acts_k = dict(zip(neural, net_acts)) if net_acts is not None else {k: act for k in neural}
    for hl_k in (hidden_layers.values() if isinstance(hidden_layers, dict) else [hidden_layers]):
        if isinstance(hl_k, Chain) and any(isinstance(l, Dropout) for l in hl_k.layers) and not any(isinstance(l, Recurrence) for l in hl_k.layers):
            raise NotImplementedError("hidden_layers Chain: Dropout layers in a MultiNN model have no device kernel (dropout is built for single-network models)")
    hl = ({k: _hidden_widths(hidden_layers[k], acts_k[k]) for k in neural} if isinstance(hidden_layers, dict)
          else {k: _hidden_widths(hidden_layers, acts_k[k]) for k in neural})
    hidden_layers = hl if isinstance(hidden_layers, dict) else next(iter(hl.values()), [])
    if any(_is_recorded(a) for a in acts_k.values()):
        nl_ = max((len(v) for v in hl.values()), default=0)
        _recorded_refusals(list(acts_k.values()), [sum(hl[k][min(l, len(hl[k]) - 1)] for k in neural) for l in range(nl_)], sum(len(predictors[k]) for k in neural), len(neural), kwargs, None)
    if any(len(v) < 1 for v in hl.values()):
        raise NotImplementedError("a network without a hidden layer")
    for p in ms.params:
        if p not in all_names:
            raise ValueError(f"mechanistic model {ms.name} needs parameter {p!r}; the table has {all_names}")
    forcing, targets = list(forcing), list(targets)
    for f in ms.forcings:
        if f not in forcing:
            raise ValueError(f"mechanistic model {ms.name} needs forcing {f!r}; got {forcing}")
    for t in targets:
        if t not in ms.outputs:
            raise ValueError(f"target {t!r} is not an output of {ms.name} {ms.outputs}")
    NNs, flat_pred = {}, []
    for k in neural:
        preds = list(predictors[k])
        if not preds:
            raise NotImplementedError("a network without predictors")
        dims = [len(preds)] + [int(w) for w in hl[k]] + [1]
        NNs[k] = [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)]
        flat_pred += preds                                   # the per-net predictor matrices stacked row-wise
    # hidden_layers::NamedTuple may give the nets different depths (test/test_generic_hybrid_model.jl:346): in the block-diagonal
    # envelope a shallower net is carried to the output layer by identity blocks as wide as its last hidden layer
    nl = max(len(v) for v in hl.values())
    tot = [sum(hl[k][min(l, len(hl[k]) - 1)] for k in neural) for l in range(nl)]
    NN = [(a, b) for a, b in zip(tot + [len(neural)], [len(flat_pred)] + tot)]     # the block-diagonal envelope
    fixed = [n for n in all_names if n not in neural and n not in glob]
    config = dict(hidden_layers=hidden_layers, activation=act if net_acts is None else dict(zip(neural, net_acts)),
                  scale_nn_outputs=scale_nn_outputs, input_batchnorm=input_batchnorm, start_from_default=start_from_default, **kwargs)
    return SingleNNHybridModel(NN, flat_pred, forcing, targets, ms, parameters, neural, glob, fixed, bool(scale_nn_outputs),
                               bool(start_from_default), config, NNs=NNs, predictor_sets={k: list(v) for k, v in predictors.items()},
                               net_activations=net_acts)


MultiNNHybridModel = SingleNNHybridModel      # one class serves both; `.NNs is not None` marks the multi-network form


def constructHybridModel(predictors, forcing: Sequence[str], targets: Sequence[str], mechanistic_model,
                         parameters, neural_param_names: Sequence[str] = None, global_param_names: Sequence[str] = None, *,
                         hidden_layers: Sequence[int] = (32, 32), activation="tanh", scale_nn_outputs: bool = False,
                         input_batchnorm: bool = False, start_from_default: bool = True, **kwargs) -> SingleNNHybridModel:
    """GenericHybridModel.jl:89-140 (Vector{Symbol} predictors form)."""
    if isinstance(predictors, dict):
        # NamedTuple-predictors form (GenericHybridModel.jl:142-206): here `neural_param_names` is the reference's
        # `global_param_names` argument position; accept both call shapes
        return _construct_multi(predictors, forcing, targets, mechanistic_model, parameters,
                                global_param_names if global_param_names is not None else neural_param_names,
                                hidden_layers=hidden_layers, activation=activation, scale_nn_outputs=scale_nn_outputs,
                                input_batchnorm=input_batchnorm, start_from_default=start_from_default, **kwargs)
    parameters = build_parameters(parameters, mechanistic_model)
    ms = resolve_mech(mechanistic_model, parameters.names(), list(forcing), list(targets))
    all_names = parameters.names()
    if not all(n in all_names for n in neural_param_names):
        raise AssertionError("neural_param_names ⊆ param_names")                      # GenericHybridModel.jl:110
    predictors, forcing, targets = list(predictors), list(forcing), list(targets)
    neural_param_names, global_param_names = list(neural_param_names), list(global_param_names)
    no_nn = len(predictors) == 0 or len(neural_param_names) == 0          # "if empty predictors do not construct NN" (GenericHybridModel.jl:112-125)
    if no_nn and neural_param_names:
        # the reference builds `NN = Chain()` here and its forward then fails on the missing NN outputs; said up front instead
        raise ValueError("neural_param_names given but no predictors: a neural parameter needs a network input")
    if no_nn and not global_param_names:
        raise ValueError("a model with neither neural nor global parameters has nothing to train")
    for p in ms.params:
        if p not in all_names:
            raise ValueError(f"mechanistic model {ms.name} needs parameter {p!r}; the table has {all_names}")
    extra = [n for n in all_names if n not in ms.params]
    if extra:
        raise ValueError(f"parameters {extra} are not arguments of {ms.name}{ms.params}")
    for f in ms.forcings:
        if f not in forcing:
            raise ValueError(f"mechanistic model {ms.name} needs forcing {f!r}; got {forcing}")
    for t in targets:
        if t not in ms.outputs:
            raise ValueError(f"target {t!r} is not an output of {ms.name} {ms.outputs}")
    act = _act_of(activation)
    chain = hidden_layers
    hidden_layers, dropout = _split_dropout(hidden_layers)
    hidden_layers, layer_acts = _hidden_widths(hidden_layers, act, per_layer=True)
    batchnorm = None
    if any(_bn_kind(a) for a in (layer_acts or ())):
        if kwargs.get("precision", "f32") != "f32":
            raise NotImplementedError(f"precision = {kwargs['precision']!r} with BatchNorm layers in hidden_layers: they run on the fp32 layer-wise kernels only")
        bns = [l for l in chain.layers if isinstance(l, BatchNorm)]
        batchnorm = {i: (b.momentum, b.epsilon) for i, b in zip([i for i, a in enumerate(layer_acts) if _bn_kind(a)], bns)}
    layernorm = None
    if any(_ln_kind(a) for a in (layer_acts or ())):
        if kwargs.get("precision", "f32") != "f32":
            raise NotImplementedError(f"precision = {kwargs['precision']!r} with LayerNorm layers in hidden_layers: they run on the fp32 layer-wise kernels only")
        lns = [l for l in chain.layers if isinstance(l, LayerNorm)]
        layernorm = {i: b.epsilon for i, b in zip([i for i, a in enumerate(layer_acts) if _ln_kind(a)], lns)}
    if dropout is not None and (len(hidden_layers) > DROPOUT_MAX_LAYERS or max(hidden_layers) > DROPOUT_MAX_WIDTH):
        raise NotImplementedError(f"hidden_layers Chain: Dropout on hidden layers {hidden_layers}: the dropout kernels are the per-wave fused family, "
                                  f"1..{DROPOUT_MAX_LAYERS} hidden layers of at most {DROPOUT_MAX_WIDTH} units")
    if not no_nn and (_is_recorded(act) or any(_is_recorded(a) for a in (layer_acts or ()))):
        _recorded_refusals([act] if layer_acts is None else layer_acts, hidden_layers, len(predictors), len(neural_param_names), kwargs, dropout)
    dims = [len(predictors)] + hidden_layers + [len(neural_param_names)]
    NN = [] if no_nn else [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)]
    if no_nn:
        input_batchnorm = False                                  # (nothing to normalise: the predictors feed no network)
    fixed = [n for n in all_names if n not in neural_param_names and n not in global_param_names]    # :127
    config = dict(hidden_layers=list(hidden_layers), activation=act, scale_nn_outputs=scale_nn_outputs,
                  input_batchnorm=input_batchnorm, start_from_default=start_from_default, **kwargs)
    if layer_acts is not None and not no_nn:
        config["layer_activations"] = list(layer_acts)
    return SingleNNHybridModel(NN, predictors, forcing, targets, ms, parameters, neural_param_names, global_param_names,
                               fixed, bool(scale_nn_outputs), bool(start_from_default), config,
                               layer_activations=None if no_nn else layer_acts, dropout=None if no_nn else dropout,
                               batchnorm=None if no_nn else batchnorm, layernorm=None if no_nn else layernorm)
