// The planner's checks for recorded activations (eh_create_activations; include/easyhybrid_hip.h): the programs themselves, and what a
// descriptor that names them may ask for.  Included by eh_plan.hpp, whose eh_plan_model calls them at the matching places of its own walk
// over the descriptor; with no programs (eh_create) every one of them answers "nothing to say".  Pure functions, no HIP runtime call.
#pragma once

// operands of an instruction word (eh_prog_op): 1, 2 or 3
inline int eh_op_arity(unsigned op) {
    return (op == EH_OP_SELECT) ? 3 : (op == EH_OP_NEG || op == EH_OP_EXP || op == EH_OP_LOG || op == EH_OP_SQRT || op == EH_OP_TANH || op == EH_OP_SIGMOID ||
                                       op == EH_OP_ABS || op == EH_OP_SIN || op == EH_OP_COS) ? 1 : 2;
}
// the programs of recorded activations (eh_act_program): counts within the limits, opcodes known, every operand a slot that holds a value
// when its instruction runs -- the generated device functions index per-lane arrays with them
inline int eh_act_programs_check(const eh_act_program* acts, int n_acts, const char* who, std::string* msg) {
    if (n_acts < 0 || n_acts > EH_MAX_ACT_PROGS || (n_acts > 0 && !acts)) return eh_plan_fail(msg, EH_EINVAL, "%s: %d activation programs (0..%d)", who, n_acts, EH_MAX_ACT_PROGS);
    for (int j = 0; j < n_acts; ++j) {
        const eh_act_program& a = acts[j];
        if (a.n_instr < 1 || a.n_instr > EH_MAX_ACT_PROG) return eh_plan_fail(msg, EH_EUNSUPPORTED, "%s: activation program %d has %d instructions (1..%d)", who, j, a.n_instr, EH_MAX_ACT_PROG);
        if (a.n_const < 0 || a.n_const > EH_MAX_ACT_CONST) return eh_plan_fail(msg, EH_EUNSUPPORTED, "%s: activation program %d has %d constants (0..%d)", who, j, a.n_const, EH_MAX_ACT_CONST);
        auto slot_ok = [&](unsigned sl, int upto) {
            if (sl < EH_PROG_SLOT_CONST) return sl == 0u;                                   // z
            if (sl < EH_PROG_SLOT_INSTR) return (int)sl - EH_PROG_SLOT_CONST < a.n_const;
            return (int)sl - EH_PROG_SLOT_INSTR < upto;
        };
        for (int i = 0; i < a.n_instr; ++i) {
            const unsigned w = a.code[i], op = w & 255u;
            if (op >= EH_OP_COUNT) return eh_plan_fail(msg, EH_EUNSUPPORTED, "%s: activation program %d, instruction %d has unknown opcode %u", who, j, i, op);
            const int nop = eh_op_arity(op);
            const unsigned sl[3] = {(w >> 8) & 255u, (w >> 16) & 255u, w >> 24};
            for (int k = 0; k < 3; ++k)
                if (k < nop ? !slot_ok(sl[k], i) : sl[k] != 0u)
                    return eh_plan_fail(msg, EH_EINVAL, "%s: activation program %d, instruction %d, operand %d names slot %u (undefined at that point, or a non-zero unused operand)", who, j, i, k, sl[k]);
        }
        if (a.out_slot < EH_PROG_SLOT_INSTR || !slot_ok((unsigned)a.out_slot, a.n_instr)) return eh_plan_fail(msg, EH_EINVAL, "%s: activation program %d: output slot %d (the result of one of its instructions)", who, j, a.out_slot);
    }
    return EH_OK;
}

// programs are named through EH_ACT_PER_NET only
// sequence models and chains with normalisation layers run on kernels built ahead of time around the five built-in activations
inline int eh_act_family_check(const eh_model_desc* d, int n_acts, bool seq, bool norm, std::string* msg) {
    if (n_acts <= 0) return EH_OK;
    if (d->activation != EH_ACT_PER_NET)
        return eh_plan_fail(msg, EH_EINVAL, "eh_create_activations: %d activation programs, but activation = %d (EH_ACT_PER_NET with net_activation = EH_ACT_RECORDED + j names them)", n_acts, d->activation);
    if (seq) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create_activations: recorded activations are not built for sequence models (their kernels are built ahead of time around the five built-in activations)");
    if (norm) return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create_activations: recorded activations are not built for chains with BatchNorm / LayerNorm layers (they run layer by layer, on kernels built ahead of time)");
    return EH_OK;
}
// net_activation[k]: 0 = not the id of a recorded activation (the caller goes on as ever), 1 = names program j (marked in used), < 0 = refused
inline int eh_act_entry_check(const eh_model_desc* d, int k, int n_acts, bool* used, std::string* msg) {
    const int a = d->net_activation[k];
    if (n_acts <= 0 || a < EH_ACT_RECORDED || a >= EH_ACT_RECORDED + EH_MAX_ACT_PROGS) return 0;
    const int j = a - EH_ACT_RECORDED;
    if (j >= n_acts) return eh_plan_fail(msg, EH_EINVAL, "eh_create_activations: %s %d names recorded activation %d, %d programs were given", d->n_nets > 0 ? "net" : "hidden layer", k, j, n_acts);
    used[j] = true;
    return 1;
}
inline int eh_act_used_check(const eh_model_desc* d, int n_acts, const bool* used, std::string* msg) {
    for (int j = 0; j < n_acts; ++j)
        if (!used[j]) return eh_plan_fail(msg, EH_EINVAL, "eh_create_activations: activation program %d is named by no %s", j, d->n_nets > 0 ? "net" : "hidden layer");
    return EH_OK;
}
// recorded activations live in the fused kernels compiled at run time; the layer-wise form applies its activations in kernels built ahead of time
inline int eh_act_shape_check(const eh_model_desc* d, int n_acts, int maxw, int K, std::string* msg) {
    const int nl = d->n_hidden;
    if (n_acts > 0 && (maxw > 128 || nl > 3 || (maxw > 64 && nl > 2) || d->n_predictors > 32 || K > 16))
        return eh_plan_fail(msg, EH_EUNSUPPORTED, "eh_create_activations: recorded activations are built for the fused kernels (P <= 32, K <= 16, widths up to 64 with at most 3 hidden layers or "
                            "up to 128 with at most 2), not for the layer-wise form this network would run on (P = %d, K = %d, widest layer %d%s, %d hidden layers)",
                            d->n_predictors, K, maxw, d->n_nets > 0 ? " with the nets side by side" : "", nl);
    return EH_OK;
}
