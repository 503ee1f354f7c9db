"""easyhybrid.jl_amd -- MI355X-native engine for the EasyHybrid.jl training-step hot path.

Host-side mirror of the reference interface (constructHybridModel / SingleNNHybridModel / train)
over the C ABI of libeasyhybrid_hip.so.  The directory name contains a dot, so it is loaded through
the root-level shim module `easyhybrid_jl_amd` (import easyhybrid_jl_amd as eh).
"""
from . import _lib
from .engine import EngineError, Ensemble, HybridEngine, PerTarget
from .models import (BatchNorm, LayerNorm, Chain, Dense, Dropout, LSTMCell, GRUCell, RNNCell, Recurrence, Expo2Pool, Expo_resp_model, FluxPartModelQ10, HybridModel, LinearHM, MECH_REGISTRY, MultiNNHybridModel, ParameterContainer, RbQ10,
                     Rs_components, Rs_components3F, SingleNNHybridModel, build_parameters, constructHybridModel, hard_sigmoid,
                     RecordedActivation, softplus, elu, leakyrelu, gelu_tanh, hard_sigmoid_act,
                     inv_hard_sigmoid, inv_sigmoid, scale_single_param, scale_single_param_minmax, sigmoid)
from .train import (Adam, AdamW, ClipGrad, ClipNorm, DataConfig, Descent, EpochSnapshot, LBFGS, OptimiserChain, RMSProp, TrainConfig, TrainResults, WeightDecay, WeightL2,
                    check_training_loss, isbetter, prepare_data, split_data, train, train_folds, train_members, validate_config)
from .sequences import Sequences, filter_sequences, split_into_sequences
from . import dp, sequences, synthetic

EH_SPLIT_TRAIN, EH_SPLIT_VAL = _lib.EH_SPLIT_TRAIN, _lib.EH_SPLIT_VAL
