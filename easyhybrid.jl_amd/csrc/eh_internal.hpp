// Shared by the translation units of libeasyhybrid_hip.so: the handle behind the opaque eh_handle pointer, the error convention and the
// functions that cross units.  The units, each the only instantiation of its kernels:
//   eh_plan.hpp   (a header, no unit) the plan of a model: descriptor checks, block placement, the leaf table of flat theta, family, EhNet --
//                 pure host code that eh_api.hip builds the handle from; eh_plan_dump.hip is a stand-alone program that prints it
//   eh_api.hip    handle lifecycle, options, the training step and epoch, evaluation, the optimiser, graphs, the eh_dp_* seam
//                 (kernels: eh_kernels.hpp, eh_chain.hpp)
//   eh_data.hip   eh_set_data / eh_set_sequences, the pinned staging pair, the staged copies (eh_pack_kernel)
//   eh_lform.hip  the layer-wise execution form (eh_lform.hpp)
//   eh_lbfgs.hip  L-BFGS (eh_lbfgs.hpp)
//   eh_mech.hip   the stand-alone mechanistic stage, eh_mech_loss_vjp
//   eh_seq.hip    the sequence-model kernels (eh_seq.hpp)
//   eh_ens.hip    ensembles: M models of one handle's architecture trained by one launch, a workgroup each (eh_ens.hpp)
//   eh_comm.hip   the library's own collectives -- RCCL binding, local groups, the peer-to-peer exchange
// Not installed; the public ABI is include/easyhybrid_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types only: the library is bound at run time, by the first eh_comm_* call (see EhRccl in eh_comm.hip)

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "eh_arch.hpp"
#include "eh_jit.hpp"
#include "eh_plan.hpp"

// Where the optimiser mirrors theta into the padded parameter image the step kernel stages.
struct EhImg {
    float* image;
    const int* imap;     // canonical index -> image offset (-1 for the raw globals)
    int g_off, phi_off;
    int glob_par[EH_MAX_PARAMS];   // global g -> canonical mech parameter j
    float glo[EH_MAX_PARAMS], ghi[EH_MAX_PARAMS];
    // extra loss lambda * weight_l2(ps; normalize) (src/utils/extract_weights.jl:69-91): l2c = lambda or lambda / #weights;
    // the Dense weight matrices are the canonical entries whose image offset lies below the bias block
    float l2c;
    int b_off;
    const unsigned char* wflag;   // layer-wise form (no image, imap == nullptr): 1 at the canonical positions of Dense weights
    // several weight_l2 terms (one per network of a MultiNNHybridModel, each with its own lambda / normalisation, or the biases:
    // extract_weights.jl:64 `l2_Rb = lambda * weight_l2(ps.Rb; normalize = true)`): one coefficient per canonical entry,
    // extra loss = sum_i l2w[i] theta_i^2 (eh_set_weight_l2_coef); nullptr: the one-lambda form above
    const float* l2w;
    int n_theta;
    // agg = mean (src/config/TrainingConfig.jl:76-77; compute_loss.jl:31-34,50-53): the training loss is
    // mean([mean_t(L_t), extra terms...]) = agg_a * sum_t L_t + l2s * sum of the extra terms, agg_a = 1 / (T (1 + E)), l2s = 1 / (1 + E);
    // agg = sum: both 1
    float agg_a, l2s;
};
__device__ __forceinline__ bool eh_is_weight(const EhImg& im, int idx) { return idx < im.g_off && (im.imap ? im.imap[idx] < im.b_off : im.wflag[idx] != 0); }
// d(extra loss) / d theta_idx = 2 * this * theta_idx
__device__ __forceinline__ float eh_l2_coef(const EhImg& im, int idx) { return im.l2s * (im.l2w ? im.l2w[idx] : (eh_is_weight(im, idx) ? im.l2c : 0.0f)); }
__device__ __forceinline__ void eh_image_store(const EhImg& im, int idx, float th) {
    if (idx < im.g_off) {
        if (im.imap) im.image[im.imap[idx]] = th;      // (layer-wise form: the kernels read the canonical theta itself)
    } else {   // raw global -> physical value and sigmoid slope (GenericHybridModel.jl:348-352)
        const int g = idx - im.g_off, j = im.glob_par[g];
        const float s = 1.0f / (1.0f + expf(-th));
        im.image[im.phi_off + EH_IMG_PHI + j] = im.glo[g] + (im.ghi[g] - im.glo[g]) * s;
        im.image[im.phi_off + EH_IMG_DPHI + j] = (im.ghi[g] - im.glo[g]) * s * (1.0f - s);
    }
}
// the same store with the map entry fetched ahead, next to the element's state (a site that waits for ONE memory round trip):
// eh_image_map with the loads, eh_image_refresh behind the update.  -1: nothing to store for a network parameter (no map, or no place)
__device__ __forceinline__ int eh_image_map(const EhImg& im, int idx) { return (idx < im.g_off && im.imap) ? im.imap[idx] : -1; }
__device__ __forceinline__ void eh_image_refresh(const EhImg& im, int idx, int mp, float th) {
    if (idx < im.g_off) { if (mp >= 0) im.image[mp] = th; }
    else eh_image_store(im, idx, th);
}

// an optimiser chain (eh_opt_init_chain; the kernels are in eh_chain.hpp): handed to them by value
struct EhChain {
    int n;                             // stages, the rule among them (0: no chain installed)
    int kind[EH_MAX_OPT_STAGES];       // EH_STAGE_*
    float a[EH_MAX_OPT_STAGES];        // CLIPGRAD delta | CLIPNORM omega | WEIGHTDECAY lambda
    int i_norm, i_rule;                // position of ClipNorm (-1: none; else < i_rule) and of the rule
    int p;                             // ClipNorm: 1, 2, or 0 = Inf
    float omega;                       // ... its threshold (= a[i_norm])
    int thr;                           // ClipNorm(throw = true): a step with a non-finite norm is not applied
};

// The optimiser in the epilogue of the weight-gradient products (few rows, ONE slab row: the product IS the gradient, un-normalised):
// the element that would have gone to the slab goes through the update rule into theta / m / v instead -- no slab row written and read
// back, no reduce + optimiser launch behind the products (8.6 us of the tutorial net's 59 us step at batch 64).  EhLApply: what the
// host hands over (eh_do_step fills it, eh_lform_train decides; the kernels are in eh_lform.hpp).
struct EhLApply {
    float* slab; float* theta; float* m; float* v;
    const float* sc_in; float* sc_out;
    EhOpt o; float* loss_slot; float* gradbuf; EhImg im;
    int loss_kind, n_theta, g_off;
    const float* part; int nblk;         // the mechanistic stage's rows of partial sums ...
    const float* tot;                    // ... or, non-null, their sums [16] (a side job of an earlier launch of the step, EhGemmArgs::job_out)
    unsigned long long* stamps; int stamp_wg;      // diagnostic builds (-DEH_STAMPS): workgroup stamp_wg stamps its phases
};

// --------------------------------------------------------------------------------------------
// handle
// --------------------------------------------------------------------------------------------
constexpr int EH_MULTI_MAX = 256;         // steps per launch of the multi-step kernel (EH_MODE_TRAIN_MULTI): bounds a launch to a millisecond or two
constexpr int EH_EVAL_BLOCKS = 1024;      // evaluation passes of the per-wave kernels: up to four workgroups per CU (eval_grid_for, eh_api.hip)
constexpr int EH_EVAL_TILES = 64;        // most tiles one wave of an evaluation pass sums into its lanes' fp32 statistics (eval_grid_for: a floor on the grid)
// the metric shift c_t of a split (eh_set_data): the mean of its first EH_SHIFT_VALID valid values of target t, so that the centred sums of
// the metrics (sum (y - c)^2 - (sum (y - c))^2 / n) do not cancel in fp32; a target whose record starts with a gap is scanned further
constexpr long long EH_SHIFT_VALID = 4096;
enum { EH_MECH_MAXROWS = 65536 };            // eh_mech_loss_vjp: rows of partials (workgroups of the streaming kernel) at most: 4 MiB
enum { EH_LFORM_ROWS = 64 };                 // layer-wise form: partial slabs of the weight gradients (split over the samples of a minibatch)
enum { EH_BNL_CHUNKS = 256, EH_BNL_CHUNK_ROWS = 128 };      // BatchNorm layers (eh_bnl.hpp): partial rows of the column sums at most; rows a chunk holds at least
// the places an optimiser update is applied from (eh_handle_s::upd_site; eh_jit_status)
enum {
    EH_UPD_REDUCE16, EH_UPD_REDUCE64, EH_UPD_REDUCE256, EH_UPD_REDUCE256V4,      // eh_reduce_kernel<true, ...> behind a step or a sequence step
    EH_UPD_DW_APPLY, EH_UPD_DW_APPLY64,                                           // the layer-wise epilogues eh_dw_apply_kernel / eh_dw_apply64_kernel
    EH_UPD_FUSED_FLUSH, EH_UPD_ORD_FLUSH,                                         // eh_fused_flush_kernel / eh_ord_flush_kernel
    EH_UPD_PROLOGUE, EH_UPD_ORD_PROLOGUE,                                         // a one-kernel step whose prologue applied the pending update (float-atomic / ordered)
    EH_UPD_MULTI,                                                                 // steps of multi-step launches (eh_ms_apply)
    EH_UPD_DP_APPLY, EH_UPD_CHAIN,                                                // eh_apply_kernel / the chain kernels
    EH_UPD_SITES
};
static inline const char* eh_upd_site_name(int s) {
    static const char* const n[EH_UPD_SITES] = {"reduce16", "reduce64", "reduce256", "reduce256v4", "dw_apply", "dw_apply64", "fused_flush", "ord_flush",
                                                "prologue", "ord_prologue", "multi_step", "dp_apply", "chain"};
    return n[s];
}

struct EhShift4 { float c[EH_MAX_TARG]; };   // the shifts as a kernel argument (eh_count_kernel, eh_moment_*_kernel)
struct EhSplit {
    float* recs = nullptr;
    long long n = 0;
    float shift[EH_MAX_TARG] = {0, 0, 0, 0};
    EhShift4 shift4() const { EhShift4 s; for (int t = 0; t < EH_MAX_TARG; ++t) s.c[t] = shift[t]; return s; }
    // sequence models (eh_set_sequences): sample i of the split is the window of W records from starts[i]
    int* starts = nullptr;
    long long nwin = 0;
    int W = 0, ow = 0, lam = 0;
    long long samples() const { return starts ? nwin : n; }      // what first / count / idx of the entry points count
};

// kernel selector handed to EhVariant::launch: the fast-path bits, or 4 = the EH_MECH_PROGRAM kernels
#define KFAST(h) ((h)->net.mech == EH_MECH_PROGRAM ? 4 : (h)->fast)
#define TH(h) ((h)->thb[(h)->cur])
#define MM(h) ((h)->mb[(h)->cur])
#define VV(h) ((h)->vb[(h)->cur])

struct eh_handle_s {
    eh_model_desc desc;
    EhNet net;
    const EhArchInfo* arch = nullptr;
    const EhArchInfo* arch_alt = nullptr;   // the other kernel family built for this shape ("row_split" option), if any
    int variant = 0, act = 0, fast = 0;
    float* image = nullptr;
    int* imap = nullptr;
    int* rmap = nullptr;            // reduction map for the current kernel family / variant / fast-path flags (v3: the inverse map)
    size_t rmap_cap = 0;
    EhPlan plan;                    // what eh_plan_model made of the descriptor (eh_plan.hpp): block placement, the leaf table of flat theta, the layer tables; never changes
    char* mech_ws = nullptr;                            // eh_mech_loss_vjp: [counts | out | partial rows]
    size_t mech_ws_bytes = 0;
    EhImg img{};
    int device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;
    int n_acc = 0;
    float *thb[2] = {nullptr, nullptr}, *mb[2] = {nullptr, nullptr}, *vb[2] = {nullptr, nullptr};   // parameter sets (fused mode ping-pongs them)
    float* pset = nullptr;          // backing allocation of thb/mb/vb/sc
    float* sc = nullptr;            // [EH_MAX_OPT_GROUPS][2][2] running beta products per optimiser group, ping-pong (group 0 = the one rule)
    EhOptTab* opt_tab = nullptr;    // per-branch optimiser rules (eh_opt_init_groups): allocated once, so a recorded graph's pointer stays valid
    int opt_groups = 1;             // groups of the current rule table; h->opt.tab != nullptr when it came from eh_opt_init_groups
    struct EhLbfgs* lb = nullptr;   // eh_lbfgs_init: the L-BFGS state (eh_lbfgs.hpp; lb->active: the handle is in L-BFGS mode)
    int lb_one_max = -1;            // "lbfgs_one_max" option: n_theta up to which one launch takes dots + decision + update (-1: EH_LB_ONE_MAX)
    EhChain chain{};                // eh_opt_init_chain: chain.n != 0 -> every step is step kernel + eh_reduce_kernel<false> + the chain kernels
    int chain_gen = 0;              // 0: no chain; else the number of the eh_opt_init_chain call that installed it (what a recorded graph carries by value)
    double* chain_part = nullptr;   // [EH_CHAIN_PARTS] partial sums of the norm pass, then the three counters of eh_opt_chain_status (allocated by eh_opt_init_chain)
    int cur = 0, sc_sel = 0;
    // fused-update mode
    bool fused = false, pending = false, fused_det = false;   // fused_det ("fused_update" 2): one kernel per step only where one workgroup covers the minibatch
    float* gacc = nullptr;          // [3][EH_GSHARDS][n_acc] rotating gradient accumulators
    // ordered fused-update step (EH_MODE_TRAIN_ORD: "fused_update" 2 on minibatches of several workgroups; EhOrd, eh_device.hpp)
    unsigned* ord = nullptr;        // one allocation: the 16 group counters (2 KB), then rows [2][256][ord_rs], then group rows [2][16][ord_rs],
                                    // then the scalars' block partials [2 slots][4 blocks][16 groups][4 floats] (2 KB), addressed from the group rows
    unsigned* ord_err = nullptr;    // host memory: set by a group's last arriver whose rows did not arrive in time (EhOrd::err)
    int ord_rs = 0, ord_soff = 0;
    bool pend_ord = false;          // the pending update is an ordered step's (its sums in the row slots, not in gacc)
    int ord_grid = 0;               // workgroups of that step
    // cross-GPU exchange (EhP2P): an uncached, IPC-exported receive buffer of {value, sequence} words next to gacc
    bool p2p_on = false, p2p_alloc = false;
    unsigned long long* p2p_recv = nullptr;
    int p2p_world = 0, p2p_rank = 0;
    unsigned p2p_seq = 0;
    float* p2p_stage = nullptr;
    unsigned* p2p_ctr = nullptr;    // [0] top-level ticket, [1] error flag, [2] self-test mismatches, [32 (1 + g)] group tickets (eh_p2p_publish)
    EhP2P* p2p_dev = nullptr;
    EhP2P p2p_host{};               // the same descriptor, handed to the step kernels by value
    void* p2p_peer[EH_GSHARDS] = {nullptr};
    eh_handle_s* p2p_group[EH_GSHARDS] = {nullptr};   // eh_p2p_init_local: the members, by rank
    bool p2p_local = false;         // the peers are handles of this process (eh_p2p_init_local): plain pointers, nothing to unmap
    long long gstep = 0;
    float* pending_loss = nullptr;
    // input BatchNorm
    bool bn_on = false;
    float* bn_part = nullptr;       // [32][64] partials + c[32]
    float* bn_run = nullptr;        // [2][32] running mean / var
    float* bn_shift = nullptr;      // [32] common shift of the cross-GPU statistics (eh_set_bn_shift)
    float* bn_stat = nullptr;       // [65] sum d | sum d^2 | n of the current step, all-reduced by the host (EH_BUF_BNSTAT)
    float* tcount = nullptr;        // [EH_MAX_TARG][3] n_t | sum (y - c) | sum (y - c)^2 of the current step's shard, all-reduced by the caller (EH_BUF_TCOUNT)
    float* mombuf = nullptr;        // [EH_MAX_TARG][EH_EVAL_STATS] this shard's moments of (yhat, y) of the current step (eh_dp_moments), all-reduced by the caller (EH_BUF_MOMENT)
    int mom_stage = 0;              // eh_dp_moments: 0 = none, 1 = the sums about the shift are out, 2 = the sums about the global centre are out
    bool dp_moments = false;        // the step being launched takes its two-pass coefficients from the all-reduced moments (no local statistics passes)
    bool dp_weights = false;        // the step being launched takes its per-target weights from the all-reduced sums (no local counting pass)
    bool tcount_ready = false;      // eh_dp_counts ran for the step eh_dp_grad is about to take
    bool bn_ext = false;            // bn_stat holds the statistics of the step about to run
    bool bn_dp_update = false;
    bool opt_ready = false;
    int ens_live = 0;               // ensembles hanging off the handle (eh_ens.hip): while there is one, its data, options and optimiser stay as they are
    // sequence models (eh_seq.hpp): Dense-in -> LSTM -> head Dense -> output Dense over windows (EH_LAYER_LSTM); always the step + reduce pair
    bool seq = false;
    float* seq_ws = nullptr;         // what the backward needs of every step, per wave of the grid (allocated outside graph capture)
    long long seq_ws_floats = 0;
    // layer-wise execution form (eh_lform.hpp): networks no fused kernel holds
    bool lform = false;
    float* l_split = nullptr; size_t l_split_cap = 0;    // split-K partial products of the small-batch GEMMs
    unsigned* l_lprog = nullptr; int l_lprog_gen = -1;  // the recorded loss programs as the layer-wise form interprets them (device copy, generation it was made from)
    float* l_dk = nullptr; size_t l_dk_cap = 0;          // every layer's delta of a small-batch step (the weight gradients then run as one grouped launch)
    bool l_job_done = false;                              // lform_gemm -> eh_lform_train (eh_lform.hip): a few-rows product took the side job of summing the chain's partial rows
    EhLApply* l_apply = nullptr; bool l_applied = false;   // eh_do_step -> eh_lform_train: the optimiser may run in the epilogue of the grouped weight gradients / it did
    bool l_tail_fn[12] = {false};
    // BatchNorm layers inside the chain (eh_bnl.hpp; one network, always this form, its few-rows fusions off): per BatchNorm layer l of
    // plan.l_net[0], at plan.bnl_off[l] floats into bnl_run: [running mean | running var]; at twice that into bnl_stat: [first row | mean
    // about it | rstd] of the step, n each
    // LayerNorm layers (eh_lnl.hpp) set `lnl` instead: the same form with the same fusions off, no state; they share bnl_eps and -- for the
    // column sums of their leaves' gradients -- bnl_part, as wide as plan.norm_maxn, nothing else of this block
    bool bnl = false, lnl = false;
    float bnl_mom[EH_MAX_HIDDEN + 1] = {0}, bnl_eps[EH_MAX_HIDDEN + 1] = {0};      // eh_set_layer_norm (defaults: EH_BN_MOMENTUM, EH_BN_EPS)
    float *bnl_run = nullptr, *bnl_stat = nullptr;
    float* bnl_part = nullptr;                           // [EH_BNL_CHUNKS][2][widest] partial column sums, then [2][widest] their totals of the backward
    float* l_ws = nullptr;                               // [Xb | H_0 .. H_{NL-1} | D0 | D1 | O | mech partial rows]
    long long l_cap = 0;                                 // samples the workspace holds
    unsigned char* wflag = nullptr;
    int slab_rows = 256;
    ncclComm_t comm = nullptr;      // eh_comm_init: the library's own RCCL communicator (data parallelism without a host-side collective library)
    int comm_world = 0, comm_rank = 0;
    struct EhLocalGroup* lgroup = nullptr;   // eh_comm_init_local: handles of ONE process exchange through peer-mapped device memory, no RCCL
    unsigned roles = 0;             // eh_set_target_roles: 2 bits per target -- 0 a data target, 1 / 2 an entry of the extra loss (mean / sum over all samples of a recorded function of the prediction)
    int agg = 0, n_extra = 0;       // eh_set_option "agg" (0 = sum, 1 = mean) / "extra_terms" (entries the extra loss returns); img.agg_a / img.l2s follow
    EhOpt opt{};
    EhSplit split[2];
    float *slab = nullptr, *gradbuf = nullptr, *inv_n = nullptr, *loss_hist = nullptr;
    long long loss_cap = 0;
    int* perm = nullptr;
    long long perm_cap = 0;
    bool perm_valid = false;
    int fast_user = 3;              // what the fast_paths option allows (default: all)
    unsigned* prog = nullptr;       // EH_MECH_PROGRAM: device copy of the program (EhStepArgs::prog layout)
    // EH_MECH_PROGRAM: kernels compiled at run time around the program (eh_jit.hpp), one entry per (kernel family, variant) used
    // state: 0 = being compiled by `worker` ("specialize" = 2: the steps run the kernels built ahead of time meanwhile), 1 = ready, -1 = failed
    // verified: the kernel has been run next to the one built ahead of time on one window of the user's data and agreed (jit_verify, eh_api.hip)
    struct JitEntry { const EhArchInfo* arch; int variant, fast; bool spec, p2p; EhNet net; int loss_gen; float drop[EH_MAX_HIDDEN] = {0}; std::atomic<int> state{0}; EhJitKernel k; std::thread worker; std::string log; bool verified = false; };
    std::vector<std::unique_ptr<JitEntry>> jit;
    bool check_idx = false;         // "check_idx" option: range-check device-side minibatch indices before the step (debug)
    bool empty_nan = false;         // "empty_target_nan" option: eh_loss_and_grad reports NaN when a target of a non-empty batch has no valid sample (the reference's value; gradient unchanged)
    bool aot_spec = true;           // "aot_spec" option / EH_NO_AOT_SPEC: run the kernel specialised ahead of time when the descriptor is a canonical one (eh_spec.hip)
    bool lean = true;               // "lean" option / EH_NO_LEAN: the lean form of the single-step train kernels where the handle's configuration allows it (eh_lean_fold, eh_device.hpp)
    bool lean_cfg = false;          // ... and whether it does (lean_refresh, eh_api.hip: decided where the configuration changes, not per step)
    int lean_last = -1;             // the last single-step train launch ran the lean (1) / the general (0) kernel; -1: none yet (eh_jit_status)
    const struct EhSpecKernel* spec_used = nullptr;      // ... the one the last launch ran (eh_jit_status reports it)
    long long ord_steps = 0;        // training steps that ran as the ordered one-kernel step (EH_MODE_TRAIN_ORD; eh_jit_status reports the count)
    // optimiser updates launched per update site since the handle was created (host-side counts; eh_jit_status reports the non-zero ones as
    // "update sites: <name> <count> ...", names in eh_upd_site_name): which kernel applied a step is decided in several places on the host
    long long upd_site[EH_UPD_SITES] = {0};
    bool specialize_async = false;  // "specialize" = 2
    bool jit_on = true;             // "jit" option / EH_JIT=0: 0 = the interpreting kernels built ahead of time
    bool jit_failed = false;
    bool specialize = false;        // "specialize" option: every model gets kernels compiled around its descriptor
    EhLossProg loss_prog;           // eh_set_loss_program (EH_LOSS_PROGRAM)
    EhJitKernel act_apply;          // eh_activation_apply's kernel, built on first use (the programs: plan.acts -- fixed for the handle's life, so no part of a JitEntry's key)
    std::string jit_log;
    // eh_set_dropout: Lux Dropout(drop[l]) behind hidden layer l in the training passes (per-wave kernels compiled at run time with the
    // rates in them; eh_device.hpp EH_JIT_DROPOUT).  drop_step counts the training steps launched since, applied or not
    bool drop_on = false;
    float drop[EH_MAX_HIDDEN] = {0};
    unsigned long long drop_seed = 0, drop_step = 0;
    float* l2val = nullptr;         // lambda * weight_l2 of the current parameters (device scalar)
    float* l2w = nullptr;           // eh_set_weight_l2_coef: one coefficient per canonical entry (device)
    struct GraphRec { hipGraphExec_t exec; bool fused; int gslot, cur, sc_sel; bool pend_ord; int ord_grid; bool grouped; int chain_gen; };
    std::vector<GraphRec> graphs;         // eh_graph_*: captured step sequences + the rotation state they start (and must end) in
    bool capturing = false;
    GraphRec cap{};
    int max_blocks = 256;
    bool multi_step = true;         // "multi_step" option (eh_train_epoch: several one-workgroup steps per launch)
    bool bn_no_self = false;        // "bn_in_kernel" 0
    int eval_blocks = 0;            // "eval_blocks" option: workgroups of eh_eval / eh_forward (0 = per kernel family, eval_grid_for)
    int mech_blocks = 0;            // "mech_blocks" option: cap on the streaming kernel's workgroups (0: none -- one workgroup per `mech_tiles` tiles)
    int mech_tiles = 0;             // "mech_tiles" option: consecutive 256 V-sample tiles per workgroup (0: by model -- 2, multi-output models 8)
    // scratch for forward / eval outputs
    float* out_buf = nullptr;
    float* eval_host = nullptr;          // pinned, device-visible: the evaluation kernels store their per-workgroup sums straight into it
    float* eval_host_dev = nullptr;
    size_t eval_host_cap = 0;            // floats
    long long out_cap = 0;
    int* idx_buf = nullptr;
    long long idx_cap = 0;
    // profiling
    bool prof = false;
    int prof_stride = 1;            // events bracket bursts of this many steps (1 = every kernel of every step)
    long long prof_k = 0;
    std::vector<hipEvent_t> ev;   // 3 per step: before step kernel, between, after reduce
    size_t ev_used = 0;
    unsigned long long* stamps = nullptr;   // diagnostic builds only
    std::string err;
};


// error convention: the message goes to the handle (or, without one, to the slot eh_last_error(NULL) reads); the code comes back
int fail(eh_handle* h, int code, const char* fmt, ...);
extern std::string g_create_err;
#define HIPCHK(h, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail(h, e_ == hipErrorOutOfMemory ? EH_ENOMEM : EH_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// fused-update mode: apply the pending gradient so theta / m / v / image are current (eh_api.hip)
int flush_pending(eh_handle* h);
#define FLUSH(h)                          \
    do {                                  \
        int rc_ = flush_pending(h);       \
        if (rc_) return rc_;              \
    } while (0)

// a device buffer the stream may still be reading grows: drain, free, allocate (cap and need in elements)
template <class T, class N>
int eh_grow(eh_handle* h, T** buf, N* cap, N need) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    (void)hipFree(*buf);
    *buf = nullptr; *cap = 0;
    HIPCHK(h, hipMalloc(buf, (size_t)need * sizeof(T)));
    *cap = need;
    return EH_OK;
}

// bit t set: target t's training loss needs batch moments of the predictions ahead of the pass (two forward-only passes; eh_api.hip)
unsigned eh_two_pass_mask(const eh_handle* h);

// what every pass over a window of a split hands its kernels: the fields all of them set alike, the rest zero
inline EhStepArgs eh_step_args(const eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count) {
    EhStepArgs a{};
    a.prog = h->prog; a.recs = sp.recs; a.C = h->plan.C; a.idx = idx; a.first = first; a.count = count;
    for (int t = 0; t < EH_MAX_TARG; ++t) a.shift[t] = sp.shift[t];
    return a;
}

// eh_api.hip, for the units that run steps of their own (eh_lbfgs.hip) or sit inside one (eh_lform.hip).  The three launchers are the only
// callers of their kernels (eh_kernels.hpp): a unit that needs one of them calls these
int eh_do_step(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, bool apply, bool raw, float* loss_slot);
int eh_check_window(eh_handle* h, const EhSplit& sp, long long first, long long count, const char* who);
int eh_bn_prepare(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, bool update, EhStepArgs* a, bool consume = true);
int eh_launch_count(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, float* tcount = nullptr);      // per-target weights -> inv_n (tcount: the raw sums too)
int eh_launch_moment_centre(eh_handle* h, const EhSplit& sp, const float* rows, int nrows);      // rows of moment sums -> the centre of yhat in inv_n
int eh_launch_moment_coef(eh_handle* h, const EhSplit& sp, const float* rows, int nrows);        // ... about it -> k0 k1 k2 and the loss value in inv_n

// eh_lform.hip: one training step's gradient sums into *rows partial slab rows | forward + metric sums of a window, *rows rows of them in the slab
int eh_lform_train(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, int* rows, bool bn_update);
int eh_lform_eval(eh_handle* h, const EhSplit& sp, long long first, long long count, float* yhat, float* pout, int* rows);

// eh_api.hip, for eh_ens.hip: the reasons a handle cannot carry an ensemble at a batch size (empty: it can), the ensemble launch, an
// evaluation pass on arguments of the caller's making, theta -> a parameter image elsewhere, the epoch orders, sums -> metrics
std::string eh_ens_refusal(eh_handle* h, long long batch);
int eh_ens_launch_train(eh_handle* h, int members, const EhStepArgs* a, const EhEnsMember* mem);
int eh_ens_launch_eval(eh_handle* h, const EhStepArgs* a, int grid);
int eh_ens_eval_grid(const eh_handle* h, long long count);
int eh_ens_launch_image(eh_handle* h, const float* theta, float* image);
int eh_ens_launch_order(eh_handle* h, const EhEnsOrder* ord, int members, long long max_n);
void eh_opt_changed(eh_handle* h);
void eh_metrics_from_sums(const double* st, const float* shift, int T, eh_target_metrics* out);

// eh_lbfgs.hip: eh_destroy's share
void eh_lbfgs_release(eh_handle* h);

// eh_data.hip: large arrays between the caller's pageable memory and the device, through the pinned staging pair of eh_set_data
int eh_copy_out(eh_handle* h, float* dst, const float* src_dev, size_t n);
int eh_copy_in(eh_handle* h, float* dst_dev, const float* src, size_t n);

// eh_destroy's share of eh_comm.hip: leave the communicator / local group, unmap the peers, free the exchange buffers
void eh_comm_release(eh_handle* h);
