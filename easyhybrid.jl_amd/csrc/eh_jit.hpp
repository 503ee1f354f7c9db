// Run-time compilation of the step kernels for a recorded closure (EH_MECH_PROGRAM).  The kernels built ahead of time
// interpret the program (per-lane value array in scratch memory, eh_device.hpp `eh_prog_forward`); here the same program is
// written out as straight-line C++ and the kernel template is instantiated around it with hiprtc, so the tape lives in
// registers and the mechanistic stage costs what a hand-derived registry model costs.  Falls back to the interpreter when
// hiprtc is unavailable or refuses (reported by eh_jit_status).
#pragma once
#include <string>
#include <vector>

#include "eh_arch.hpp"
#include "eh_seq.hpp"

struct EhJitKernel {
    hipModule_t mod = nullptr;
    hipFunction_t fn[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // EH_MODE_TRAIN, EH_MODE_EVAL, EH_MODE_TRAIN_P2P (when asked for), EH_MODE_TRAIN_MULTI and
                                                                           // EH_MODE_TRAIN_ORD (per-wave registry models with one target)
    hipFunction_t fn_lean[2] = {nullptr, nullptr};   // the lean form of EH_MODE_TRAIN [0] and EH_MODE_TRAIN_ORD [1] (eh_lean_fold, eh_device.hpp), where those two are built
    int nw = 0;
    size_t lds_bytes = 0;
    size_t lds_eval_bytes = 0;      // forward / evaluation kernel (0: lds_bytes)
};

// a recorded custom training loss (eh_set_loss_program): value slot 0 = yhat, 1 = y
struct EhLossProg1 {
    std::vector<unsigned> code;
    std::vector<float> consts;
    int out = 0;
};
struct EhLossProg : EhLossProg1 {          // the program every target without one of its own uses (eh_set_loss_program) ...
    EhLossProg1 per[4];                    // ... and the targets' own (eh_set_target_loss_program; PerTarget((f, g)), compute_loss.jl:128-145)
    int gen = 0;          // bumped by every eh_set_*loss_program: part of the cache key of the compiled kernels
    const EhLossProg1& of(int t) const { return per[t].code.empty() ? static_cast<const EhLossProg1&>(*this) : per[t]; }
    bool has(int t) const { return !of(t).code.empty(); }
};
// the generated eh_jit_loss.inc: float eh_jit_loss(int target, float yhat, float yobs, float& dl)
std::string eh_jit_loss_source(const EhLossProg& lp);
// the generated eh_jit_mech.inc (EhJitTape, eh_jit_fwd, eh_jit_rev) for a validated descriptor
std::string eh_jit_mech_source(const eh_model_desc& d);
// Compiles the train + eval (+ cross-GPU train) kernels of (arch, variant, activation, fast-path flags); false + log on failure.
// `spec` (optional) bakes the model descriptor into the kernels as a compile-time constant.
// allow_slp = false: never the SLP vectoriser (the flags of the kernels built ahead of time: a kernel that REPLACES one of those in the
// middle of a run -- "specialize" = 2 -- must give the same bits)
bool eh_jit_build(const eh_model_desc& d, const EhArchInfo* A, int variant, int act, int fast, const EhNet* spec, bool with_p2p,
                  const EhLossProg* loss, EhJitKernel* out, std::string* log, bool allow_slp = true, const float* drop = nullptr,
                  const std::vector<eh_act_program>* acts = nullptr);
// (acts: the programs of recorded activations, validated (eh_plan.hpp) -- compiled in under EH_JIT_ACTPROG with the generated eh_jit_act.inc,
//  next to EH_JIT_ROWACT whose eh_row_act hands out the ids EH_ACT_RECORDED + j that name them)
// the generated eh_jit_act.inc: eh_jit_act_<j>(z), eh_jit_dact_<j>(z) per program and the dispatchers eh_jit_act(j, z), eh_jit_dact(j, z)
std::string eh_jit_act_source(const eh_act_program* acts, int n_acts);
// eh_activation_apply's kernel (fn[0]): value and derivative of activation id -- built-in or EH_ACT_RECORDED + j -- through eh_act_id / eh_dact_z_id
bool eh_jit_build_act_apply(const std::vector<eh_act_program>& acts, EhJitKernel* out, std::string* log);
// (drop: dropout rates per hidden layer, d.n_hidden of them, or nullptr -- compiled in under EH_JIT_DROPOUT with the generated
//  eh_jit_dropout.inc; such kernels are single-step only)
// threshold of the keep test (a word below it drops the unit) and the factor on a kept unit for rate p in [0, 1): one definition for the
// generated header, eh_dropout_mask and the tests' twin
inline unsigned eh_drop_threshold(float p) { const double t = (double)p * 4294967296.0; return t >= 4294967295.0 ? 4294967295u : (unsigned)t; }
inline float eh_drop_scale(float p) { return 1.0f / (1.0f - p); }
hipError_t eh_jit_launch(const EhJitKernel* k, int mode, int grid, hipStream_t stream, const EhNet* net, const EhStepArgs* args, bool lean = false);
void eh_jit_release(EhJitKernel* k);
// Sequence models around a recorded closure (eh_seq.hpp, EH_SEQ_HEAD_PROG): the (NBI, NBH) instantiation of the three modes compiled
// around the generated eh_jit_fwd / eh_jit_rev; fn[EH_SEQ_TRAIN], fn[EH_SEQ_EVAL], fn[EH_SEQ_FORWARD].  Same disk cache as above.
// cell: EH_SEQ_CELL_*; mt: the kernels of several targets (the launch is the same: EhSeqArgs carries what they read)
bool eh_jit_build_seq(const eh_model_desc& d, int nbi, int nbh, int cell, bool mt, EhJitKernel* out, std::string* log);
hipError_t eh_jit_launch_seq(const EhJitKernel* k, int mode, int grid, hipStream_t stream, const EhNet* net, const EhSeqArgs* args);
