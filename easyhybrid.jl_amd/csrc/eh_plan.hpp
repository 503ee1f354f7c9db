// The plan of a model: everything eh_create decides about a descriptor before it touches a device.  eh_plan_model checks the
// descriptor, places the networks as blocks of the padded MLP, lays flat theta out as ONE table of parameter leaves, names the kernel
// family the descriptor asks for and fills the EhNet -- a pure function: no HIP runtime call, no handle, no global.  eh_api.hip
// builds the handle from its result and keeps it (eh_handle_s::plan); eh_plan_dump.hip prints it, so that tests/test_plan.py can hold
// the layout against models.py, and the refusals against the recorded ones, on a machine without a device.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "eh_device.hpp"
#include "eh_seq.hpp"

// what the descriptor asks for: no network (mechanistic stage + reduce), the sequence kernels, normalisation layers (always layer by
// layer), or a fused kernel where a shape for (nbi, nbh, n_hidden) is built and the layer-wise form otherwise (eh_create looks)
enum { EH_FAMILY_NONE = 0, EH_FAMILY_SEQ, EH_FAMILY_NORM, EH_FAMILY_FUSED };
// an entry of a network's chain: a Dense layer, or Lux's BatchNorm / LayerNorm behind the layer in front of it (in = out = its width)
enum { EH_LK_DENSE = 0, EH_LK_BN_AFFINE, EH_LK_BN, EH_LK_LN_AFFINE, EH_LK_LN };
inline bool eh_is_norm(int kind) { return kind != EH_LK_DENSE; }
inline bool eh_is_layernorm(int kind) { return kind == EH_LK_LN_AFFINE || kind == EH_LK_LN; }
inline bool eh_affine(int kind) { return kind == EH_LK_BN_AFFINE || kind == EH_LK_LN_AFFINE; }
// a parameter leaf, named as the reference's ComponentArray names it
enum { EH_LEAF_WEIGHT = 0, EH_LEAF_BIAS, EH_LEAF_SCALE, EH_LEAF_WEIGHT_IH, EH_LEAF_WEIGHT_HH, EH_LEAF_BIAS_IH, EH_LEAF_BIAS_HH };
inline const char* eh_leaf_name(int kind) {
    static const char* const n[] = {"weight", "bias", "scale", "weight_ih", "weight_hh", "bias_ih", "bias_hh"};
    return n[kind];
}
// one row per leaf, in canonical (flat theta) order; layer: its place in its own network's chain; a matrix is column-major (rows, cols),
// a vector has cols == 0; is_weight: a Dense weight matrix, what weight_l2 sums (extract_weights.jl:69-91: not a cell's weight_ih /
// weight_hh, not a BatchNorm's scale)
struct EhLeaf {
    int net, layer, kind, off, rows, cols;
    bool is_weight;
    int size() const { return rows * std::max(cols, 1); }
};
// one network as a chain of layers (SingleNN: one; MultiNN: one single-output network per neural parameter, each on its own predictor
// rows and at its own depth): what the layer-wise form runs.  woff / boff of a normalisation layer: its scale / bias
struct EhLNet {
    int nl = 0, c0 = 0, orow = 0, act = 0;
    int lact[EH_MAX_HIDDEN + 1] = {0}, kind[EH_MAX_HIDDEN + 1] = {0};
    int in[EH_MAX_HIDDEN + 1] = {0}, out[EH_MAX_HIDDEN + 1] = {0}, woff[EH_MAX_HIDDEN + 1] = {0}, boff[EH_MAX_HIDDEN + 1] = {0};
};

struct EhPlan {
    eh_model_desc desc{};                               // the descriptor, a MultiNN's net_depth / net_hidden / net_activation spelled out (what the run-time compiler reads)
    int act = 0;                                        // the effective activation (EH_ACT_PER_NET only where the rows really differ)
    int family = EH_FAMILY_NONE;
    int K = 0, G = 0, maxw = 0, nbi = 0, nbh = 0;       // nbh: 16-row blocks of the widest layer rounded up to 1 2 4 8 (0: wider than any fused kernel)
    // block placement of every net inside the padded (block-diagonal) MLP
    int n_nets = 1;                                     // 1 for SingleNN
    int net_P[EH_MAX_NETS] = {0}, net_K[EH_MAX_NETS] = {0};
    int net_w[EH_MAX_NETS][EH_MAX_HIDDEN] = {{0}};      // hidden widths of net k
    int net_d[EH_MAX_NETS] = {0};                       // hidden layers of net k (layers past them: identity blocks, not in theta)
    int net_c0[EH_MAX_NETS] = {0};                      // first predictor row of net k
    int net_r0[EH_MAX_NETS][EH_MAX_HIDDEN + 1] = {{0}}; // first row of net k in layer l (l == n_hidden: output row)
    int tot_w[EH_MAX_HIDDEN] = {0};                     // total (summed) hidden widths
    EhNet net{};                                        // (the loss fields stay 0: eh_set_option sets them on the handle's copy)
    int C = 0, n_acc = 0, n_par = 0;                    // columns of a record; [grad | S | n_valid per target | Sy | Syy]; mechanistic parameters
    std::vector<EhLeaf> leaves;
    int n_weights = 0;                                  // entries of the is_weight leaves
    int l_nnets = 0;                                    // 0: no chain of layers (no neural parameter, or a sequence model)
    EhLNet l_net[EH_MAX_NETS];
    // normalisation layers of l_net[0]: a BatchNorm layer l keeps [running mean | running var] at bnl_off[l] of bnl_tot floats
    bool bnl = false, lnl = false;
    int bnl_off[EH_MAX_HIDDEN + 1] = {0}, bnl_tot = 0, norm_maxn = 0;      // norm_maxn: the widest layer of either kind
    // sequence models: Dense(P -> I) -> cell(I -> H) -> Dense(H -> H) -> Dense(H -> K); seq_off: the ten leaves' offsets (EH_SEQ_WIN .. EH_SEQ_BOUT)
    int seq_cell = 0, seq_act_cell = 0, seq_I = 0, seq_H = 0, seq_nbi = 0, seq_nbh = 0, seq_act_in = 0, seq_act_hd = 0;
    int seq_off[EH_SEQ_NOFF] = {0};
    std::vector<eh_act_program> acts;                   // recorded activations (eh_create_activations): program j is what net_activation = EH_ACT_RECORDED + j names
};

inline int eh_plan_fail(std::string* msg, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *msg = buf;
    return code;
}

#include "eh_plan_act.hpp"      // what eh_create_activations adds to the checks below (eh_plan_fail is its way out too)

struct EhMechInfo { int n_par, n_forc, n_out; };
inline bool eh_mech_info(int mech, EhMechInfo* mi, const eh_model_desc* d = nullptr) {
    switch (mech) {
        case EH_MECH_PROGRAM: if (!d) return false; *mi = {d->n_params, d->prog_n_forc, d->prog_n_out}; return true;
        case EH_MECH_RBQ10: *mi = {2, 1, 1}; return true;
        case EH_MECH_EXPO: *mi = {2, 1, 1}; return true;
        case EH_MECH_LINEAR: *mi = {2, 1, 1}; return true;
        case EH_MECH_EXPO2POOL: *mi = {4, 1, 1}; return true;
        case EH_MECH_RS_COMPONENTS: *mi = {6, 1, 1}; return true;
        case EH_MECH_RS_COMPONENTS3F: *mi = {6, 3, 1}; return true;
        case EH_MECH_FLUXPART: *mi = {3, 2, 3}; return true;
        default: return false;
    }
}

// Sequence models (EH_LAYER_LSTM, EH_LAYER_GRU or EH_LAYER_RNN + activation in the per-layer activation slots; the messages say "LSTM"
// for every cell): 0 = the descriptor has no recurrent layer, 1 = the one shape that is built -- Dense(P -> I) -> cell(I -> H) ->
// Dense(H -> H) -> Dense(H -> K), eh_seq.hpp --, otherwise the status of the refusal.
inline bool eh_seq_layer_code(int a) { return a == EH_LAYER_LSTM || a == EH_LAYER_GRU || (a >= EH_LAYER_RNN && a <= EH_LAYER_RNN + EH_ACT_IDENTITY); }
inline int eh_seq_desc_check(const eh_model_desc* d, int n_out, bool several_targets, std::string* msg) {
    if (d->activation != EH_ACT_PER_NET) return 0;
    const int na = std::min(d->n_nets > 0 ? d->n_nets : d->n_hidden, (int)EH_MAX_NETS);
    int n_lstm = 0, at = -1;
    for (int l = 0; l < na; ++l)
        if (eh_seq_layer_code(d->net_activation[l])) { if (at < 0) at = l; ++n_lstm; }
    if (!n_lstm) return 0;
    if (d->n_nets > 0) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for a MultiNN sequence model (EH_LAYER_LSTM with n_nets = %d)", d->n_nets);
    if (at == 0) return eh_plan_fail(msg, EH_EINVAL, "eh_create: EH_LAYER_LSTM at hidden layer 0: the LSTM layer takes the Dense layer in front of it");
    if (n_lstm > 1) return eh_plan_fail(msg, EH_EINVAL, "eh_create: %d EH_LAYER_LSTM layers (one, at hidden layer 1: stacked Recurrence layers are not built)", n_lstm);
    if (d->n_hidden != 3 || at != 1 || d->hidden[2] != d->hidden[1])
        return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for an LSTM layer at hidden layer %d of %d (built: n_hidden = 3, hidden = [I, H, H], the LSTM at layer 1)", at, d->n_hidden);
    if (d->hidden[0] < 1 || d->hidden[1] < 1) return eh_plan_fail(msg, EH_EINVAL, "eh_create: hidden = [%d, %d, ..]", d->hidden[0], d->hidden[1]);
    if (d->hidden[0] > 32 || d->hidden[1] > 32) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for LSTM widths I = %d, H = %d (built: up to 32 each)", d->hidden[0], d->hidden[1]);
    if (d->n_predictors > 32) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for a sequence model with P = %d predictors (built: up to 32)", d->n_predictors);
    if (d->input_batchnorm) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for input BatchNorm on a sequence model (3-D input)");
    if (d->n_targets < 1 || d->n_targets > EH_MAX_TARG) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for a sequence model with %d targets (built: 1..%d)", d->n_targets, (int)EH_MAX_TARG);
    for (int t = 0; t < d->n_targets; ++t)
        if (d->target_output[t] < 0 || d->target_output[t] >= n_out)
            return eh_plan_fail(msg, EH_EINVAL, "eh_create: sequence model: target_output[%d] = %d names an output the model does not have (it has %d)", t, d->target_output[t], n_out);
    if (d->n_targets > 1 && n_out < 2)
        return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for a sequence model with %d targets around a model with one output (every target would observe the same value)", d->n_targets);
    // eh_create keeps what it has always answered to such a descriptor, for the one reason that the tests of the one-target kernels pin that
    // answer (include/easyhybrid_hip.h, eh_create_seq_targets): several targets are asked for by name
    if (d->n_targets > 1 && !several_targets)
        return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for a sequence model with %d targets behind this entry point (one target per sequence handle; several: eh_create_seq_targets)", d->n_targets);
    // (around every mechanistic model: registry, several outputs, recorded closure; every target names its output, in any order -- two
    //  targets on one output are taken as the feed-forward families take them)
    return 1;
}

// The two kinds of normalisation layer inside the chain: net_activation[l] = base [+ noaffine] + the layer's eh_activation; `first` /
// `second`: the order of the affine leaves in theta (Lux: BatchNorm scale, bias; LayerNorm bias, scale); max_width: 0 = any
struct EhNormKind { int base, noaffine, affine_kind; const char* name; const char* code; int first, second, max_width; };
inline const EhNormKind* eh_norm_kind(int a) {
    static const EhNormKind kinds[2] = {
        {EH_LAYER_BATCHNORM, EH_LAYER_BN_NOAFFINE, EH_LK_BN_AFFINE, "BatchNorm", "EH_LAYER_BATCHNORM", EH_LEAF_SCALE, EH_LEAF_BIAS, 0},
        {EH_LAYER_LAYERNORM, EH_LAYER_LN_NOAFFINE, EH_LK_LN_AFFINE, "LayerNorm", "EH_LAYER_LAYERNORM", EH_LEAF_BIAS, EH_LEAF_SCALE, EH_MAX_LAYERNORM_WIDTH}};
    for (const EhNormKind& k : kinds) {
        const int b = a - k.base;
        if ((b >= 0 && b <= EH_ACT_IDENTITY) || (b >= k.noaffine && b <= k.noaffine + EH_ACT_IDENTITY)) return &k;
    }
    return nullptr;
}
// layers of kind `nk` (eh_norm_kind of its base code) in the descriptor: 0 = none, 1 = well formed (one network, every such layer as wide
// as the layer in front of it), otherwise the status of the refusal
inline int eh_norm_desc_check(const eh_model_desc* d, const EhNormKind* nk, std::string* msg) {
    if (d->activation != EH_ACT_PER_NET) return 0;
    const int na = std::min(d->n_nets > 0 ? d->n_nets : d->n_hidden, (int)EH_MAX_NETS);
    int n_norm = 0;
    bool cell = false;
    for (int l = 0; l < na; ++l) { n_norm += eh_norm_kind(d->net_activation[l]) == nk ? 1 : 0; cell = cell || eh_seq_layer_code(d->net_activation[l]); }
    if (!n_norm) return 0;
    if (d->n_nets > 0) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for %s layers in a MultiNN model (%s with n_nets = %d)", nk->name, nk->code, d->n_nets);
    if (cell) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for a chain that holds both a %s layer and a recurrent layer", nk->name);
    for (int l = 0; l < na; ++l) {
        if (eh_norm_kind(d->net_activation[l]) != nk) continue;
        if (l == 0) return eh_plan_fail(msg, EH_EINVAL, "eh_create: %s at hidden layer 0: a %s layer normalises the layer in front of it (hidden layer 0 is a Dense layer)", nk->code, nk->name);
        if (d->hidden[l] != d->hidden[l - 1]) return eh_plan_fail(msg, EH_EINVAL, "eh_create: %s layer %d has width %d, the layer in front of it %d", nk->name, l, d->hidden[l], d->hidden[l - 1]);
        if (nk->max_width && d->hidden[l] > nk->max_width)
            return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: no kernel for a %s layer of width %d (built: up to %d, a row in one wave's registers)", nk->name, d->hidden[l], nk->max_width);
    }
    return 1;
}

// acts / n_acts: the programs of recorded activations (eh_create_activations); eh_create passes none, and then answers the ids that name
// them as it always has
inline int eh_plan_model(const eh_model_desc* d, bool seq_several_targets, EhPlan* out, std::string* msg, const eh_act_program* acts = nullptr, int n_acts = 0) {
    *out = EhPlan();
    EhPlan& p = *out;
    if (d->struct_size != (int32_t)sizeof(eh_model_desc)) return eh_plan_fail(msg, EH_EINVAL, "eh_create: struct_size %d != %zu", d->struct_size, sizeof(eh_model_desc));
    if (const int rc = eh_act_programs_check(acts, n_acts, "eh_create_activations", msg)) return rc;
    EhMechInfo mi;
    if (!eh_mech_info(d->mech, &mi, d)) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: unknown mechanistic model id %d (no silent fallback)", d->mech);
    const bool desc_layers = d->activation == EH_ACT_PER_NET && d->n_hidden >= 0 && d->n_hidden <= EH_MAX_HIDDEN && d->n_nets >= 0 && d->n_nets <= EH_MAX_NETS;
    const int bnk = desc_layers ? eh_norm_desc_check(d, eh_norm_kind(EH_LAYER_BATCHNORM), msg) : 0;
    if (bnk < 0) return bnk;
    const int lnk = desc_layers ? eh_norm_desc_check(d, eh_norm_kind(EH_LAYER_LAYERNORM), msg) : 0;
    if (lnk < 0) return lnk;
    const bool norm = bnk == 1 || lnk == 1;      // (a normalisation layer of either kind: an entry of the chain that is no Dense layer)
    const int seqk = (desc_layers && !norm) ? eh_seq_desc_check(d, mi.n_out, seq_several_targets, msg) : 0;
    if (seqk < 0) return seqk;
    const bool seq = seqk == 1;
    if (const int rc = eh_act_family_check(d, n_acts, seq, norm, msg)) return rc;
    if (d->mech == EH_MECH_PROGRAM) {
        // every operand must name a slot that holds a value when the instruction runs: the kernel indexes a per-lane array with them
        if (d->n_params < 1 || d->n_params > EH_MAX_PARAMS) return eh_plan_fail(msg, EH_EINVAL, "eh_create: a program takes 1..%d parameters, descriptor has %d", EH_MAX_PARAMS, d->n_params);
        if (d->prog_len < 1 || d->prog_len > EH_MAX_PROG) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: program of %d instructions (1..%d)", d->prog_len, EH_MAX_PROG);
        if (d->prog_n_const < 0 || d->prog_n_const > EH_MAX_PROG_CONST) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: program with %d constants (0..%d)", d->prog_n_const, EH_MAX_PROG_CONST);
        if (d->prog_n_forc < 0 || d->prog_n_forc > EH_MAX_FORC) return eh_plan_fail(msg, EH_EINVAL, "eh_create: program with %d forcings (0..%d)", d->prog_n_forc, EH_MAX_FORC);
        if (d->prog_n_out < 1 || d->prog_n_out > EH_MAX_PROG_OUT) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: program with %d outputs (1..%d)", d->prog_n_out, EH_MAX_PROG_OUT);
        auto slot_ok = [&](unsigned sl, int upto) {
            if (sl < EH_PROG_SLOT_FORC) return (int)sl < d->n_params;
            if (sl < EH_PROG_SLOT_CONST) return (int)sl - EH_PROG_SLOT_FORC < d->prog_n_forc;
            if (sl < EH_PROG_SLOT_INSTR) return (int)sl - EH_PROG_SLOT_CONST < d->prog_n_const;
            return (int)sl - EH_PROG_SLOT_INSTR < upto;
        };
        for (int i = 0; i < d->prog_len; ++i) {
            const unsigned w = d->prog_code[i], op = w & 255u;
            if (op >= EH_OP_COUNT) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: program instruction %d has unknown opcode %u", i, op);
            const int nop = (op == EH_OP_SELECT) ? 3 : (op == EH_OP_NEG || op == EH_OP_EXP || op == EH_OP_LOG || op == EH_OP_SQRT || op == EH_OP_TANH ||
                                                        op == EH_OP_SIGMOID || op == EH_OP_ABS || op == EH_OP_SIN || op == EH_OP_COS) ? 1 : 2;
            const unsigned sl[3] = {(w >> 8) & 255u, (w >> 16) & 255u, w >> 24};
            for (int k = 0; k < 3; ++k) {
                if (k < nop ? !slot_ok(sl[k], i) : sl[k] != 0u)
                    return eh_plan_fail(msg, EH_EINVAL, "eh_create: program instruction %d, operand %d names slot %u (undefined at that point, or a non-zero unused operand)", i, k, sl[k]);
            }
        }
        for (int o = 0; o < d->prog_n_out; ++o)
            if (d->prog_out[o] < 0 || !slot_ok((unsigned)d->prog_out[o], d->prog_len)) return eh_plan_fail(msg, EH_EINVAL, "eh_create: program output %d names slot %d", o, d->prog_out[o]);
    }
    if (d->activation < 0 || d->activation > EH_ACT_PER_NET) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: unknown activation id %d", d->activation);
    int act = d->activation;
    if (act == EH_ACT_PER_NET) {
        // n_nets >= 1: activation::NamedTuple of the MultiNN constructor (GenericHybridModel.jl:168-176), one activation per network;
        // n_nets == 0: `hidden_layers::Chain` of the single-network constructor (NNModels.jl:145-219: Dense layers that carry activations of
        // their own), one activation per hidden LAYER.  Both run on kernels compiled at run time around eh_row_act(layer, row).
        if (d->n_nets < 0 || d->n_nets > EH_MAX_NETS) return eh_plan_fail(msg, EH_EINVAL, "eh_create: n_nets = %d (0..%d)", d->n_nets, EH_MAX_NETS);
        const int na = d->n_nets > 0 ? d->n_nets : d->n_hidden;
        if (na < 1 || na > EH_MAX_HIDDEN) return eh_plan_fail(msg, EH_EINVAL, "eh_create: per-layer activations need 1..%d hidden layers (n_hidden = %d)", EH_MAX_HIDDEN, d->n_hidden);
        bool same = true, used[EH_MAX_ACT_PROGS] = {};
        for (int k = 0; k < na; ++k) {
            if (seq && eh_seq_layer_code(d->net_activation[k])) { same = false; continue; }
            if (norm && eh_norm_kind(d->net_activation[k])) { same = false; continue; }
            if (const int ra = eh_act_entry_check(d, k, n_acts, used, msg)) {      // names a recorded activation
                if (ra < 0) return ra;
                same = false;          // (never one of the kernels built ahead of time, even where every layer names the same program)
                continue;
            }
            if (d->net_activation[k] < 0 || d->net_activation[k] > EH_ACT_IDENTITY)
                return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create: unknown activation id %d for %s %d", d->net_activation[k], d->n_nets > 0 ? "net" : "hidden layer", k);
            same = same && d->net_activation[k] == d->net_activation[0];
        }
        if (same) act = d->net_activation[0];          // one activation after all: the kernels built ahead of time
        if (const int rc = eh_act_used_check(d, n_acts, used, msg)) return rc;
    }
    if (d->n_params != mi.n_par) return eh_plan_fail(msg, EH_EINVAL, "eh_create: model %d takes %d parameters, descriptor has %d", d->mech, mi.n_par, d->n_params);
    if (d->n_predictors < 0 || d->n_hidden < 0 || d->n_hidden > EH_MAX_HIDDEN) return eh_plan_fail(msg, EH_EINVAL, "eh_create: n_predictors %d, n_hidden %d (0..%d)", d->n_predictors, d->n_hidden, EH_MAX_HIDDEN);
    if (d->n_forcings < mi.n_forc || d->n_forcings > EH_MAX_FORC) return eh_plan_fail(msg, EH_EINVAL, "eh_create: n_forcings %d (model needs %d, max %d)", d->n_forcings, mi.n_forc, EH_MAX_FORC);
    if (d->n_targets < 1 || d->n_targets > EH_MAX_TARG) return eh_plan_fail(msg, EH_EINVAL, "eh_create: n_targets must be 1..%d", EH_MAX_TARG);
    int K = 0, G = 0;
    bool seenK[EH_MAX_PARAMS] = {}, seenG[EH_MAX_PARAMS] = {};
    for (int j = 0; j < d->n_params; ++j) {
        const int k = d->param_kind[j], ix = d->param_index[j];
        if (k == EH_PAR_NEURAL || k == EH_PAR_GLOBAL) {
            if (ix < 0 || ix >= EH_MAX_PARAMS) return eh_plan_fail(msg, EH_EINVAL, "eh_create: param_index[%d] = %d out of range", j, ix);
            bool* seen = k == EH_PAR_NEURAL ? seenK : seenG;
            if (seen[ix]) return eh_plan_fail(msg, EH_EINVAL, "eh_create: duplicate param_index %d", ix);
            seen[ix] = true;
            (k == EH_PAR_NEURAL ? K : G)++;
            if (!(d->param_upper[j] > d->param_lower[j]) && (k == EH_PAR_GLOBAL || d->scale_nn_outputs))
                return eh_plan_fail(msg, EH_EINVAL, "eh_create: parameter %d needs upper > lower for sigmoid scaling", j);
        } else if (k != EH_PAR_FIXED) {
            return eh_plan_fail(msg, EH_EINVAL, "eh_create: param_kind[%d] = %d", j, k);
        }
    }
    for (int i = 0; i < K; ++i) if (!seenK[i]) return eh_plan_fail(msg, EH_EINVAL, "eh_create: neural param_index values must be 0..K-1");
    for (int i = 0; i < G; ++i) if (!seenG[i]) return eh_plan_fail(msg, EH_EINVAL, "eh_create: global param_index values must be 0..G-1");
    // No neural parameter: the reference builds no network at all (`NN = Chain()`, GenericHybridModel.jl:112-125) and its forward
    // is global / fixed parameters -> M (:376-406).  Here: the layer-wise form with zero Dense layers (mechanistic stage + reduce).
    const bool no_nn = K == 0;
    if (no_nn) {
        if (G < 1) return eh_plan_fail(msg, EH_EINVAL, "eh_create: a model with neither neural nor global parameters has nothing to train");
        if (d->n_hidden != 0 || d->n_nets != 0 || d->input_batchnorm) return eh_plan_fail(msg, EH_EINVAL, "eh_create: no neural parameter: n_hidden, n_nets and input_batchnorm must be 0");
    } else {
        if (d->n_predictors < 1) return eh_plan_fail(msg, EH_EINVAL, "eh_create: n_predictors must be >= 1");
        if (d->n_hidden < 1) return eh_plan_fail(msg, EH_EINVAL, "eh_create: n_hidden must be 1..%d", EH_MAX_HIDDEN);
    }
    // nets and their block placement (SingleNN = one net with K outputs); layers past a net's own depth are identity blocks as wide as its last one
    const int nl = d->n_hidden;
    for (int k = 0; k < EH_MAX_NETS; ++k) p.net_d[k] = nl;
    bool mixed_depth = false;
    // (not a copy of the check above: that one runs for EH_ACT_PER_NET alone, this one answers every other activation)
    if (d->n_nets < 0 || d->n_nets > EH_MAX_NETS) return eh_plan_fail(msg, EH_EINVAL, "eh_create: n_nets = %d (0..%d)", d->n_nets, EH_MAX_NETS);
    if (d->n_nets > 0) {
        if (d->n_nets != K) return eh_plan_fail(msg, EH_EINVAL, "eh_create: MultiNN needs one net per neural parameter (%d nets, %d neural parameters)", d->n_nets, K);
        p.n_nets = d->n_nets;
        int ptot = 0;
        for (int k = 0; k < p.n_nets; ++k) {
            if (d->net_n_predictors[k] < 1) return eh_plan_fail(msg, EH_EINVAL, "eh_create: net %d has no predictors", k);
            p.net_P[k] = d->net_n_predictors[k]; p.net_K[k] = 1; ptot += p.net_P[k];
            if (d->net_depth[k] < 0 || d->net_depth[k] > nl) return eh_plan_fail(msg, EH_EINVAL, "eh_create: net_depth[%d] = %d (n_hidden = %d)", k, d->net_depth[k], nl);
            if (d->net_depth[k] > 0) p.net_d[k] = d->net_depth[k];
            mixed_depth = mixed_depth || p.net_d[k] != nl;
            for (int l = 0; l < nl; ++l) {
                if (l < p.net_d[k] && d->net_hidden[k][l] < 1) return eh_plan_fail(msg, EH_EINVAL, "eh_create: net_hidden[%d][%d] = %d", k, l, d->net_hidden[k][l]);
                p.net_w[k][l] = d->net_hidden[k][l < p.net_d[k] ? l : p.net_d[k] - 1]; p.tot_w[l] += p.net_w[k][l];
            }
        }
        if (mixed_depth) {
            bool full = false;
            for (int k = 0; k < p.n_nets; ++k) full = full || p.net_d[k] == nl;
            if (!full) return eh_plan_fail(msg, EH_EINVAL, "eh_create: n_hidden = %d but no net is that deep", nl);
            act = EH_ACT_PER_NET;            // the identity blocks need the row-dependent activation (kernels compiled at run time)
        }
        if (ptot != d->n_predictors) return eh_plan_fail(msg, EH_EINVAL, "eh_create: net_n_predictors sum to %d, n_predictors = %d", ptot, d->n_predictors);
    } else {
        p.net_P[0] = d->n_predictors; p.net_K[0] = K;
        for (int l = 0; l < nl; ++l) {
            if (d->hidden[l] < 1) return eh_plan_fail(msg, EH_EINVAL, "eh_create: hidden[%d] = %d", l, d->hidden[l]);
            p.net_w[0][l] = d->hidden[l]; p.tot_w[l] = d->hidden[l];
        }
    }
    for (int l = 0; l < nl; ++l) p.maxw = std::max(p.maxw, p.tot_w[l]);
    for (int f = 0; f < mi.n_forc; ++f)
        if (d->forcing_index[f] < 0 || d->forcing_index[f] >= d->n_forcings) return eh_plan_fail(msg, EH_EINVAL, "eh_create: forcing_index[%d] out of range", f);
    for (int t = 0; t < d->n_targets; ++t)
        if (d->target_output[t] < 0 || d->target_output[t] >= mi.n_out) return eh_plan_fail(msg, EH_EINVAL, "eh_create: target_output[%d] = %d (model has %d outputs)", t, d->target_output[t], mi.n_out);

    // recorded activations live in the fused kernels compiled at run time; the layer-wise form applies its activations in kernels built ahead of time
    if (const int rc = eh_act_shape_check(d, n_acts, p.maxw, K, msg)) return rc;

    // ---- accepted: from here on nothing is refused -------------------------------------------------------------------------------
    p.act = act; p.K = K; p.G = G;
    p.family = no_nn ? EH_FAMILY_NONE : seq ? EH_FAMILY_SEQ : norm ? EH_FAMILY_NORM : EH_FAMILY_FUSED;
    const int nbh_raw = (p.maxw + 15) / 16;
    p.nbi = (d->n_predictors + 15) / 16;
    p.nbh = nbh_raw <= 1 ? 1 : nbh_raw <= 2 ? 2 : nbh_raw <= 4 ? 4 : nbh_raw <= 8 ? 8 : 0;
    p.desc = *d;
    p.acts.assign(acts, acts + n_acts);
    if (d->n_nets > 0) {
        for (int k = 0; k < p.n_nets; ++k) {
            p.desc.net_depth[k] = p.net_d[k];
            for (int l = 0; l < nl; ++l) p.desc.net_hidden[k][l] = p.net_w[k][l];
            if (act == EH_ACT_PER_NET) p.desc.net_activation[k] = d->activation == EH_ACT_PER_NET ? d->net_activation[k] : d->activation;
        }
        if (act == EH_ACT_PER_NET) p.desc.activation = EH_ACT_PER_NET;
    }
    {
        int c0 = 0, r0[EH_MAX_HIDDEN] = {0};
        for (int k = 0; k < p.n_nets; ++k) {
            p.net_c0[k] = c0; c0 += p.net_P[k];
            for (int l = 0; l < nl; ++l) { p.net_r0[k][l] = r0[l]; r0[l] += p.net_w[k][l]; }
            p.net_r0[k][nl] = d->n_nets > 0 ? k : 0;            // output row
        }
    }
    // the layout of flat theta: the one walk over the leaves, in the reference's ComponentArray order
    int off = 0;
    auto leaf = [&](int net, int layer, int kind, int rows, int cols) {
        p.leaves.push_back({net, layer, kind, off, rows, cols, kind == EH_LEAF_WEIGHT});
        if (kind == EH_LEAF_WEIGHT) p.n_weights += rows * cols;
        off += p.leaves.back().size();
        return p.leaves.back().off;
    };
    if (seq) {      // Dense-in | weight_ih, weight_hh, bias_ih, bias_hh (NG gate blocks of H rows each) | head Dense | output Dense
        const int P = d->n_predictors, I = d->hidden[0], H = d->hidden[1], code = d->net_activation[1];
        p.seq_cell = code == EH_LAYER_LSTM ? EH_SEQ_CELL_LSTM : (code == EH_LAYER_GRU ? EH_SEQ_CELL_GRU : EH_SEQ_CELL_RNN);
        p.seq_act_cell = p.seq_cell == EH_SEQ_CELL_RNN ? code - EH_LAYER_RNN : 0;
        const int NG = eh_seq_gates(p.seq_cell);
        leaf(0, 0, EH_LEAF_WEIGHT, I, P); leaf(0, 0, EH_LEAF_BIAS, I, 0);
        leaf(0, 1, EH_LEAF_WEIGHT_IH, NG * H, I); leaf(0, 1, EH_LEAF_WEIGHT_HH, NG * H, H); leaf(0, 1, EH_LEAF_BIAS_IH, NG * H, 0); leaf(0, 1, EH_LEAF_BIAS_HH, NG * H, 0);
        leaf(0, 2, EH_LEAF_WEIGHT, H, H); leaf(0, 2, EH_LEAF_BIAS, H, 0);
        leaf(0, 3, EH_LEAF_WEIGHT, K, H); leaf(0, 3, EH_LEAF_BIAS, K, 0);
        for (int i = 0; i < EH_SEQ_NOFF; ++i) p.seq_off[i] = p.leaves[(size_t)i].off;      // (EH_SEQ_WIN .. EH_SEQ_BOUT is the leaves' order)
        p.seq_I = I; p.seq_H = H; p.seq_nbi = (I + 15) / 16; p.seq_nbh = (H + 15) / 16;
        p.seq_act_in = d->net_activation[0]; p.seq_act_hd = d->net_activation[2];
    } else if (!no_nn) {
        p.l_nnets = p.n_nets;
        for (int k = 0; k < p.n_nets; ++k) {
            EhLNet& L = p.l_net[k];
            L.nl = p.net_d[k] + 1; L.c0 = p.net_c0[k]; L.orow = d->n_nets > 0 ? k : 0;
            L.act = (d->n_nets > 0 && d->activation == EH_ACT_PER_NET) ? d->net_activation[k] : (act == EH_ACT_PER_NET ? d->activation : act);
            for (int l = 0; l <= EH_MAX_HIDDEN; ++l)      // (an activation per hidden layer: the single network of a `hidden_layers::Chain`)
                L.lact[l] = (d->n_nets == 0 && act == EH_ACT_PER_NET && l < nl) ? d->net_activation[l] : L.act;
            int in = p.net_P[k];
            for (int l = 0; l < L.nl; ++l) {
                const int o = l + 1 < L.nl ? p.net_w[k][l] : p.net_K[k];
                const EhNormKind* nk = (norm && l + 1 < L.nl) ? eh_norm_kind(d->net_activation[l]) : nullptr;
                L.in[l] = in; L.out[l] = nk ? in : o;
                if (nk) {      // scale and bias in the kind's order, or nothing (affine = false)
                    const int b = d->net_activation[l] - nk->base;
                    const bool affine = b < nk->noaffine;
                    L.kind[l] = nk->affine_kind + (affine ? 0 : 1); L.lact[l] = affine ? b : b - nk->noaffine;
                    L.woff[l] = L.boff[l] = off;
                    if (affine) for (const int lk : {nk->first, nk->second}) (lk == EH_LEAF_SCALE ? L.woff : L.boff)[l] = leaf(k, l, lk, in, 0);
                    if (eh_is_layernorm(L.kind[l])) p.lnl = true;
                    else { p.bnl = true; p.bnl_off[l] = p.bnl_tot; p.bnl_tot += 2 * in; }      // (a LayerNorm layer has no state)
                    p.norm_maxn = std::max(p.norm_maxn, in);
                    continue;
                }
                L.woff[l] = leaf(k, l, EH_LEAF_WEIGHT, o, in); L.boff[l] = leaf(k, l, EH_LEAF_BIAS, o, 0);
                in = o;
            }
        }
    }
    EhNet& n = p.net;
    memset(&n, 0, sizeof n);
    n.P = d->n_predictors; n.K = K; n.G = G; n.T = d->n_targets; n.F = d->n_forcings;
    n.g_off = off;
    n.n_theta = off + G;
    n.scale_nn = d->scale_nn_outputs ? 1 : 0;
    n.mech = d->mech; n.n_par = d->n_params;
    for (int j = 0; j < d->n_params; ++j) {
        n.par_kind |= (unsigned)d->param_kind[j] << (2 * j);
        n.par_idx |= (unsigned)(d->param_kind[j] == EH_PAR_FIXED ? 0 : d->param_index[j]) << (4 * j);
    }
    for (int j = d->n_params; j < EH_MAX_PARAMS; ++j) n.par_kind |= (unsigned)EH_PAR_FIXED << (2 * j);
    n.forc_col = 0xFFFFFFFFu;
    for (int f = 0; f < mi.n_forc; ++f) n.forc_col = (n.forc_col & ~(0xFFu << (8 * f))) | ((unsigned)d->forcing_index[f] << (8 * f));
    n.n_out = mi.n_out;
    for (int t = 0; t < d->n_targets; ++t) n.targ_out |= (unsigned)d->target_output[t] << (2 * t);
    p.C = n.P + n.F + n.T;
    p.n_par = d->n_params;
    p.n_acc = n.n_theta + 1 + n.T + 2;
    return EH_OK;
}
