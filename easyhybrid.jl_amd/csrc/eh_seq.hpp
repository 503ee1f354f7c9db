// Sequence models: Dense(P -> I, act) -> Recurrence(cell(I -> H)) -> Dense(H -> H, act) -> Dense(H -> K) over windows of W consecutive
// records, with back-propagation through time; the cell is an LSTMCell, a GRUCell or an RNNCell (template
// parameter CELL; what follows is told for the LSTM).  eh_step_body's idiom stretched over time:
//
//   * one wave owns a tile of 16 windows for the whole forward and backward chain; the window sits on the MFMA N dimension and every
//     product runs on v_mfma_f32_16x16x4_f32.  A C/D block (lane (n = lane & 15, g = lane >> 4), register r <-> row 4g + r, window n)
//     is the B operand of the next product when MFMA r of a 16-deep contraction takes k = 4g + r and the weight fragment is read from
//     LDS in that order (one ds_read_b128 per lane): x_t, h_t and c_t never leave registers in the forward.
//   * what the backward needs of step t -- the post-activation gates, c_{t-1}, tanh(c_t), and at the head steps the head's
//     pre-activation and d loss / d o -- is parked in a workspace in global memory, in C/D register layout: every lane reads back only
//     the 16-byte words it stored itself, so no cache-scope question arises and no fence is needed.  x_t is recomputed from the
//     predictors (a Dense of P <= 32 inputs) instead of stored; h_{t-1} is o_{t-1} tanh(c_{t-1}) of the record before.
//   * weight gradients contract over the 16 windows: both operands transposed through a wave-private LDS tile (window on K), the
//     accumulators stay in registers across all steps and tiles of the wave (128 VGPRs for W_ih and W_hh at I = H = 32).
//   * the head (head Dense, output Dense, sigma-scaling, mechanistic model, residual) runs only at the `ow` steps the loss reads.
//     Its mechanistic stage comes in three forms (template parameter HEAD): a single-output registry model (eh_mech_eval), a registry
//     model with several outputs (eh_mech_extra gives the target's output and its Jacobian row), and a recorded closure
//     (EH_MECH_PROGRAM).  The closure's tape is per lane and lives only within the head step: the reverse sweep runs right there, seeded
//     with d loss / d yhat at the target's output, and leaves the per-parameter adjoint where d * dydp[j] stands for the registry models
//     -- nothing of the tape is parked in the workspace.  Built ahead of time the program is interpreted (the tape in scratch memory);
//     compiled at run time around the generated eh_jit_fwd / eh_jit_rev (eh_jit.hip, EH_JIT_MECH) the tape is registers.
//   * epilogue: the workgroup's waves are gathered in wave order into one slab row [n_theta gradient | S | n | Sy | Syy]
//     (eh_reduce_kernel's contract), so the step is bit-reproducible.
//   * several targets (template parameter MT, kernels of their own): the head evaluates every output once and loops over the targets
//     (eh_seq_head_targets).  Their normalisers differ, so the weights come from a count pre-pass over the minibatch's windows
//     (eh_seq_count_kernel) and the row is the one of the multi-target feed-forward steps, [n_theta gradient | loss | n_1 .. n_T].
//   * the other cells change the recurrent step alone -- geometry, head, Dense-in and epilogue are shared.  GRUCell, gate blocks
//     [r | z | n]: h' = (1 - z) n + z h with n = tanh(W_in x + b_in + r (W_hn h + b_hn)); the reset gate multiplies the hidden product, so
//     that product is a fourth accumulator chain q of its own and b_hn a bias row of its own (r and z fold b_ih + b_hh as the LSTM does).
//     Parked per step: r, z, n, q, h_t.  RNNCell: h' = act(W_ih x + W_hh h + b_ih + b_hh), act one of the Dense activations
//     (EhSeqArgs::act_cell); parked: the pre-activation and h_t.  h_{t-1} is the h_t of the record before for both.
#pragma once
#include "eh_device.hpp"

enum { EH_SEQ_TRAIN = 0, EH_SEQ_EVAL = 1, EH_SEQ_FORWARD = 2 };
enum { EH_SEQ_HEAD_MECH = 0, EH_SEQ_HEAD_MULTI = 1, EH_SEQ_HEAD_PROG = 2 };      // the mechanistic stage of the head: see above
constexpr int EH_SEQ_NW = 4;                 // waves per workgroup: one per SIMD (the accumulators take most of a wave's 512 registers)
enum { EH_SEQ_CELL_LSTM = 0, EH_SEQ_CELL_GRU = 1, EH_SEQ_CELL_RNN = 2 };         // the recurrent cell
constexpr int eh_seq_gates(int cell) { return cell == EH_SEQ_CELL_LSTM ? 4 : (cell == EH_SEQ_CELL_GRU ? 3 : 1); }        // gate blocks of weight_ih / weight_hh
constexpr int eh_seq_bias_rows(int cell) { return cell == EH_SEQ_CELL_RNN ? 1 : 4; }                                      // bias blocks in LDS (GRU: r | z | n_ih | n_hh)
constexpr int eh_seq_parked(int cell) { return cell == EH_SEQ_CELL_LSTM ? 6 : (cell == EH_SEQ_CELL_GRU ? 5 : 2); }       // C/D blocks parked per step and hidden block
constexpr int EH_SEQ_MTW = 16 * (1 + EH_MAX_TARG) + EH_MAX_TARG;      // several targets, TRAIN: floats of a wave's row of per-target scalars (eh_seq_head_targets)
constexpr int EH_SEQ_MTE = 16 * EH_EVAL_STATS * EH_MAX_TARG;          // ... EVAL: of its row of shifted sums, a column per window for each
constexpr int EH_SEQ_TS = 20;                // row stride of the transposition tile (16 windows + 4: 16-byte rows, no two rows in one bank group)

// canonical offsets into flat theta (ComponentArray order) and the LDS layout of the zero-padded parameters
enum { EH_SEQ_WIN = 0, EH_SEQ_BIN, EH_SEQ_WIH, EH_SEQ_WHH, EH_SEQ_BIH, EH_SEQ_BHH, EH_SEQ_WHD, EH_SEQ_BHD, EH_SEQ_WOUT, EH_SEQ_BOUT, EH_SEQ_NOFF };

struct EhSeqArgs {
    const float* recs;       // [n][C] records of the split: predictors | forcings | targets
    int C;
    const int* starts;       // window w starts at record starts[w]
    const int* idx;          // minibatch: window idx[first + k], or first + k when null
    long long first, count;  // in windows
    int W, ow, lam;
    const float* theta;      // canonical parameters
    const float* meta;       // PHI block of the parameter image (globals, bounds)
    float* slab;             // TRAIN: one row of n_acc floats per workgroup; EVAL: EH_EVAL_STATS floats per workgroup
    int n_acc;
    float* ws;               // TRAIN: ws_wave floats per wave of the grid
    long long ws_wave;
    float* yhat;             // FORWARD: [count][ow] predictions per target, `yld` apart ...
    float* pout;             // ... and [n_par][count * ow] parameters
    long long yld;
    float shift;             // metric shift (one target)
    int I, H, act_in, act_hd;
    int off[EH_SEQ_NOFF];
    const unsigned* prog;    // EH_SEQ_HEAD_PROG: the recorded closure (EhStepArgs::prog layout)
    int act_cell;            // EH_SEQ_CELL_RNN: the cell's activation
    // several targets (behind what the kernels of one target read, so that those stay what they are):
    const float* inv_n;      // TRAIN: the per-target table of the window count pre-pass (EH_TT floats per target, [0] the weight)
    float shift_t[EH_MAX_TARG];      // metric shift per target
};

template <int NBI, int NBH, int CELL = EH_SEQ_CELL_LSTM>
struct EhSeqGeom {
    static constexpr int NG = eh_seq_gates(CELL), NB = eh_seq_bias_rows(CELL);
    static constexpr int RI = 16 * NBI, RH = 16 * NBH, SP = 36, SI = RI + 4, SH = RH + 4;
    static constexpr int L_WIN = 0, L_WIH = L_WIN + RI * SP, L_WHH = L_WIH + NG * RH * SI, L_WHD = L_WHH + NG * RH * SH, L_WOUT = L_WHD + RH * SH,
                         L_BIN = L_WOUT + 16 * SH, L_BG = L_BIN + RI, L_BHD = L_BG + NB * RH, L_BOUT = L_BHD + RH, L_TILE = L_BOUT + 16,
                         L_GB = L_TILE + EH_SEQ_NW * 16 * EH_SEQ_TS, L_END = L_GB + EH_SEQ_NW * NB * RH;
};

#ifndef __HIPCC_RTC__      // (host side; this header is also compiled at run time, by hiprtc, around a recorded closure: eh_jit.hip)
// floats of workspace one wave needs: eh_seq_parked(cell) NBH blocks per step, NBH + 1 per head step, 256 floats a block
inline long long eh_seq_ws_floats(int nbh, int W, int ow, int cell = EH_SEQ_CELL_LSTM) { return ((long long)W * eh_seq_parked(cell) * nbh + (long long)ow * (nbh + 1)) * 256; }
int eh_seq_row_cap(int nbi, int nbh, int cell = EH_SEQ_CELL_LSTM);        // accumulators a slab row may hold (the row is staged in LDS over the parameters)
// head: EH_SEQ_HEAD_* of the model, cell: EH_SEQ_CELL_*, mt: the kernels of several targets (a missing instantiation is an error, never another path)
hipError_t eh_seq_launch(int nbi, int nbh, int mode, int head, int grid, hipStream_t stream, const EhNet& net, const EhSeqArgs& a, int cell = EH_SEQ_CELL_LSTM, bool mt = false);
#endif

#ifdef EH_SEQ_KERNELS
// four MFMAs of one 16-deep contraction: MFMA r takes k = 4g + r of both operands
__device__ __forceinline__ f32x4 eh_seq_mfma4(const f32x4 a, const f32x4 b, f32x4 c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[r], c, 0, 0, 0);
    return c;
}
__device__ __forceinline__ f32x4 eh_seq_act4(int id, const f32x4 z) { return f32x4{eh_act_id(id, z[0]), eh_act_id(id, z[1]), eh_act_id(id, z[2]), eh_act_id(id, z[3])}; }
__device__ __forceinline__ f32x4 eh_seq_dact4(int id, const f32x4 z) { return f32x4{eh_dact_z_id(id, z[0]), eh_dact_z_id(id, z[1]), eh_dact_z_id(id, z[2]), eh_dact_z_id(id, z[3])}; }
__device__ __forceinline__ f32x4 eh_seq_sig4(const f32x4 z) { return f32x4{eh_sigmoid(z[0]), eh_sigmoid(z[1]), eh_sigmoid(z[2]), eh_sigmoid(z[3])}; }
__device__ __forceinline__ f32x4 eh_seq_tanh4(const f32x4 z) { return f32x4{eh_tanh(z[0]), eh_tanh(z[1]), eh_tanh(z[2]), eh_tanh(z[3])}; }

// The head's mechanistic stage and loss of a model with several targets, one window per lane (eh_step_body's loop over the targets):
// every output of the model is evaluated once; target t takes its own output (net.targ_out), its own column of the record `yrow` and
// so its own mask, its own loss kind (net.loss_t) and its weight wt[t] from the count pre-pass, and seeds the adjoint of its output.
// One reverse pass takes all seeds: the Jacobian rows of the registry model, one sweep over the closure's tape.
//   TRAIN: the per-target scalars live in a wave-private LDS row (EH_SEQ_MTW floats; at I = H = 32 the accumulators leave no registers for
//          them): acc = the lane's column of [1 + EH_MAX_TARG][16] sums over the head steps -- [0] the weighted loss terms, [1 + t] the valid
//          entries of target t, touched by the lanes with `sums` --, wts = the targets' weights behind them; dp[j] = d loss / d parameter j
//   EVAL: acc = the lane's column of the wave's [EH_MAX_TARG][EH_EVAL_STATS][16] shifted sums, in LDS as well (in registers the 32 sums
//         took the kernels to 256 VGPRs and one wave per SIMD);  yt[t]: the prediction for target t (every mode)
template <int MODE, int HEAD>
__device__ __forceinline__ void eh_seq_head_targets(const EhNet& net, const EhSeqArgs& a, const float (&par)[EH_MAX_PARAMS], const float (&frc)[EH_MAX_FORC],
                                                    const float* yrow, bool live, bool sums, const float* wts, float* acc,
                                                    float (&yt)[EH_MAX_TARG], float (&dp)[EH_MAX_PARAMS]) {
    constexpr bool TRAIN = MODE == EH_SEQ_TRAIN, PROG = HEAD == EH_SEQ_HEAD_PROG;
    static_assert(HEAD != EH_SEQ_HEAD_MECH, "several targets need a model with several outputs");
    float yo[3] = {0.0f, 0.0f, 0.0f}, dydp[EH_MAX_PARAMS], Jx[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
#ifdef EH_JIT_MECH
    EhJitTape jtape;
    if constexpr (PROG) eh_jit_fwd(par, frc, jtape, yo[0], yo[1], yo[2]);
    else {
#else
    float pval[PROG ? EH_PROG_SLOTS : 1];
    if constexpr (PROG) {
        eh_prog_forward(a.prog, par, frc, pval);
        yo[0] = pval[a.prog[2]];
        if (net.n_out > 1) yo[1] = pval[a.prog[3]];
        if (net.n_out > 2) yo[2] = pval[a.prog[4]];
    } else {
#endif
#pragma unroll
        for (int j = 0; j < EH_MAX_PARAMS; ++j) dydp[j] = 0.0f;
        yo[0] = eh_mech_eval(net.mech, par, frc, dydp);
        eh_mech_extra(net.mech, par, frc, yo + 1, Jx);
    }
    float dyo[3] = {0.0f, 0.0f, 0.0f};                        // d loss / d output
    bool any = false;
#pragma unroll
    for (int t = 0; t < EH_MAX_TARG; ++t) {
        yt[t] = 0.0f;
        if (t < net.T) {
            const int to = (int)((net.targ_out >> (2 * t)) & 3u);
            const float y = to == 0 ? yo[0] : (to == 1 ? yo[1] : yo[2]), yobs = yrow[t];
            const bool valid = live && !__builtin_isnan(yobs);
            const float r = valid ? y - yobs : 0.0f;
            yt[t] = y;
            if constexpr (TRAIN) {
                const float w = wts[t];
                float d, lt;
                if (eh_target_mae(net.loss_t, t)) { lt = w * fabsf(r); d = r > 0.0f ? w : (r < 0.0f ? -w : 0.0f); }
                else { lt = w * r * r; d = 2.0f * w * r; }
                if (sums) { acc[0] += lt; acc[16 * (1 + t)] += valid ? 1.0f : 0.0f; }
                dyo[0] += to == 0 ? d : 0.0f; dyo[1] += to == 1 ? d : 0.0f; dyo[2] += to == 2 ? d : 0.0f;
                any = any || valid;
            } else if constexpr (MODE == EH_SEQ_EVAL) {
                if (valid && sums) {
                    const float cy = yobs - a.shift_t[t], ch = y - a.shift_t[t];
                    float* const e = acc + 16 * EH_EVAL_STATS * t;
                    e[0] = fmaf(r, r, e[0]); e[16] += cy; e[32] = fmaf(cy, cy, e[32]); e[48] += 1.0f;
                    e[64] += ch; e[80] = fmaf(ch, ch, e[80]); e[96] = fmaf(ch, cy, e[96]); e[112] += fabsf(r);
                }
            }
        }
    }
    if constexpr (TRAIN) {
#ifdef EH_JIT_MECH
        float padj[EH_MAX_PARAMS];
        if constexpr (PROG) eh_jit_rev(par, frc, jtape, dyo[0], dyo[1], dyo[2], padj);
#else
        float padj[PROG ? EH_PROG_SLOTS : 1];
        if constexpr (PROG) {
            const int nslot = EH_PROG_SLOT_INSTR + (int)a.prog[0];
            for (int i = 0; i < nslot; ++i) padj[i] = 0.0f;
            padj[a.prog[2]] += dyo[0];
            if (net.n_out > 1) padj[a.prog[3]] += dyo[1];
            if (net.n_out > 2) padj[a.prog[4]] += dyo[2];
            eh_prog_reverse(a.prog, pval, padj);
        }
#endif
#pragma unroll
        for (int j = 0; j < EH_MAX_PARAMS; ++j) {
            float v;
            if constexpr (PROG) v = padj[j];
            else v = dyo[0] * dydp[j] + (j < 3 ? dyo[1] * Jx[0][j] + dyo[2] * Jx[1][j] : 0.0f);
            dp[j] = any ? v : 0.0f;                           // (a window without a valid target adds nothing, whatever the model made of its record)
        }
    }
}

// MT: the head of a model with several targets (eh_seq_head_targets; the kernels of one target are the default and stay what they are)
template <int NBI, int NBH, int MODE, int HEAD = EH_SEQ_HEAD_MECH, int CELL = EH_SEQ_CELL_LSTM, bool MT = false>
__global__ __launch_bounds__(64 * EH_SEQ_NW) void eh_seq_kernel(const EhNet net, const EhSeqArgs a) {
    using G = EhSeqGeom<NBI, NBH, CELL>;
    constexpr bool TRAIN = MODE == EH_SEQ_TRAIN, PROG = HEAD == EH_SEQ_HEAD_PROG, LSTM = CELL == EH_SEQ_CELL_LSTM, GRU = CELL == EH_SEQ_CELL_GRU;
    constexpr int NG = G::NG, NB = G::NB, PER = eh_seq_parked(CELL);
    constexpr int RH = G::RH, SP = G::SP, SI = G::SI, SH = G::SH;
    // (a closure's tape takes registers at the head step that the registry models leave free: with PROG the gradient of the two head biases
    //  is summed over the windows at every head step and kept in a wave-private LDS row behind the layout, as the gate biases' is)
    __shared__ __attribute__((aligned(16))) float lds[G::L_END + (PROG ? EH_SEQ_NW * (RH + 16) : 0) + (MT && TRAIN ? EH_SEQ_NW * EH_SEQ_MTW : 0) + (MT && MODE == EH_SEQ_EVAL ? EH_SEQ_NW * EH_SEQ_MTE : 0)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
    const int P = net.P, I = a.I, H = a.H, K = net.K, C = a.C;

    // ---- parameters -> LDS, row-major, zero-padded to whole blocks (padding rows and columns are structural zeros) -------------
    for (int e = tid; e < G::L_TILE; e += 64 * EH_SEQ_NW) lds[e] = 0.0f;
    __syncthreads();
    {
        const float* th = a.theta;
        for (int e = tid; e < I * P; e += 64 * EH_SEQ_NW) lds[G::L_WIN + (e % I) * SP + e / I] = th[a.off[EH_SEQ_WIN] + e];
        for (int e = tid; e < NG * H * I; e += 64 * EH_SEQ_NW) { const int rf = e % (NG * H); lds[G::L_WIH + ((rf / H) * RH + rf % H) * SI + e / (NG * H)] = th[a.off[EH_SEQ_WIH] + e]; }
        for (int e = tid; e < NG * H * H; e += 64 * EH_SEQ_NW) { const int rf = e % (NG * H); lds[G::L_WHH + ((rf / H) * RH + rf % H) * SH + e / (NG * H)] = th[a.off[EH_SEQ_WHH] + e]; }
        for (int e = tid; e < H * H; e += 64 * EH_SEQ_NW) lds[G::L_WHD + (e % H) * SH + e / H] = th[a.off[EH_SEQ_WHD] + e];
        for (int e = tid; e < K * H; e += 64 * EH_SEQ_NW) lds[G::L_WOUT + (e % K) * SH + e / K] = th[a.off[EH_SEQ_WOUT] + e];
        for (int e = tid; e < I; e += 64 * EH_SEQ_NW) lds[G::L_BIN + e] = th[a.off[EH_SEQ_BIN] + e];
        if constexpr (GRU) {      // r and z fold their two biases; b_in and b_hn stay apart (rows 2 and 3)
            for (int e = tid; e < 3 * H; e += 64 * EH_SEQ_NW) {
                const float bi = th[a.off[EH_SEQ_BIH] + e], bh = th[a.off[EH_SEQ_BHH] + e];
                if (e < 2 * H) lds[G::L_BG + (e / H) * RH + e % H] = bi + bh;
                else { lds[G::L_BG + 2 * RH + e - 2 * H] = bi; lds[G::L_BG + 3 * RH + e - 2 * H] = bh; }
            }
        } else
        for (int e = tid; e < NG * H; e += 64 * EH_SEQ_NW) lds[G::L_BG + (e / H) * RH + e % H] = th[a.off[EH_SEQ_BIH] + e] + th[a.off[EH_SEQ_BHH] + e];
        for (int e = tid; e < H; e += 64 * EH_SEQ_NW) lds[G::L_BHD + e] = th[a.off[EH_SEQ_BHD] + e];
        for (int e = tid; e < K; e += 64 * EH_SEQ_NW) lds[G::L_BOUT + e] = th[a.off[EH_SEQ_BOUT] + e];
    }
    __syncthreads();

    float* const TT = lds + G::L_TILE + wave * 16 * EH_SEQ_TS;
    // the gate biases' gradient: summed over the 16 windows every step and kept in a wave-private LDS row (as per-lane registers they
    // are 32 more at H = 32, which the W_ih / W_hh accumulators leave no room for)
    float* const GB = lds + G::L_GB + wave * NB * RH;
    for (int e = lane; e < NB * RH; e += 64) GB[e] = 0.0f;
    float* const HB = lds + G::L_END + (PROG ? wave * (RH + 16) : 0);      // PROG: [RH] head Dense bias | [16] output Dense bias
    if constexpr (PROG) { for (int e = lane; e < RH + 16; e += 64) HB[e] = 0.0f; }
    // MT, TRAIN: the sums over the head steps per target, zeroed, and the targets' weights -- read here, once for all tiles and head steps
    float* const MTA = lds + G::L_END + (PROG ? EH_SEQ_NW * (RH + 16) : 0) + (MT && TRAIN ? wave * EH_SEQ_MTW : 0) + (MT && MODE == EH_SEQ_EVAL ? wave * EH_SEQ_MTE : 0);
    if constexpr (MT && TRAIN) {
        for (int e = lane; e < EH_SEQ_MTW; e += 64) { const int t = e - 16 * (1 + EH_MAX_TARG); MTA[e] = (t >= 0 && t < net.T) ? a.inv_n[EH_TT * t] : 0.0f; }
        EH_WAVE_SYNC();
    }
    if constexpr (MT && MODE == EH_SEQ_EVAL) {                 // MT, EVAL: the shifted sums per target
        for (int e = lane; e < EH_SEQ_MTE; e += 64) MTA[e] = 0.0f;
        EH_WAVE_SYNC();
    }
    // C/D block -> its transpose as an MFMA operand with the window on K: element r of the result = M[row n][window 4g + r]
    auto tr = [&](const f32x4 v) -> f32x4 {
#pragma unroll
        for (int r = 0; r < 4; ++r) TT[(4 * g + r) * EH_SEQ_TS + n] = v[r];
        EH_WAVE_SYNC();
        const f32x4 o = *reinterpret_cast<const f32x4*>(TT + n * EH_SEQ_TS + 4 * g);
        EH_WAVE_SYNC();
        return o;
    };
    // A fragment of W[row0 + n][k0 + 4g + r] (forward products) and of the transpose, W[row0 + 4g + r][col0 + n] (delta products)
    auto ldA = [&](int base, int stride, int row0, int k0) -> f32x4 { return *reinterpret_cast<const f32x4*>(lds + base + (row0 + n) * stride + k0 + 4 * g); };
    auto ldAT = [&](int base, int stride, int row0, int col0) -> f32x4 {
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = lds[base + (row0 + 4 * g + r) * stride + col0 + n];
        return o;
    };
    auto ldB = [&](int base, int row0) -> f32x4 { return *reinterpret_cast<const f32x4*>(lds + base + row0 + 4 * g); };      // a bias in C/D layout

    // h_t of a step, block hb, from the step's parked record (w4: this lane's word of the record's first block)
    auto h_of = [&](const f32x4* w4, int hb) -> f32x4 {
        if constexpr (LSTM) return w4[(hb * 6 + 3) * 64] * w4[(hb * 6 + 5) * 64];      // o tanh(c)
        else return w4[(hb * PER + PER - 1) * 64];
    };
    // Dense-in of one record per window: pre-activation blocks zx
    auto dense_in = [&](const float* rec, f32x4 (&zx)[NBI]) {
        f32x4 p[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int col = pb * 16 + 4 * g + r; p[pb][r] = col < P ? rec[col] : 0.0f; }
#pragma unroll
        for (int ib = 0; ib < NBI; ++ib) {
            zx[ib] = ldB(G::L_BIN, ib * 16);
            zx[ib] = eh_seq_mfma4(ldA(G::L_WIN, SP, ib * 16, 0), p[0], zx[ib]);
            if (P > 16) zx[ib] = eh_seq_mfma4(ldA(G::L_WIN, SP, ib * 16, 16), p[1], zx[ib]);
        }
    };

    // ---- accumulators (TRAIN): they live across all steps and tiles of the wave ------------------------------------------------
    const f32x4 Z4 = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 gWih[NG][NBH][NBI], gWhh[NG][NBH][NBH], gWin[NBI][2], gBin[NBI], gWhd[NBH][NBH], gBhd[NBH], gWout[NBH], gBout = Z4;
    float gp[EH_MAX_PARAMS], est[EH_EVAL_STATS];
#pragma unroll
    for (int q = 0; q < NG; ++q)
#pragma unroll
        for (int hb = 0; hb < NBH; ++hb) {
#pragma unroll
            for (int ib = 0; ib < NBI; ++ib) gWih[q][hb][ib] = Z4;
#pragma unroll
            for (int kb = 0; kb < NBH; ++kb) gWhh[q][hb][kb] = Z4;
        }
#pragma unroll
    for (int ib = 0; ib < NBI; ++ib) { gWin[ib][0] = Z4; gWin[ib][1] = Z4; gBin[ib] = Z4; }
#pragma unroll
    for (int hb = 0; hb < NBH; ++hb) {
        gBhd[hb] = Z4; gWout[hb] = Z4;
#pragma unroll
        for (int kb = 0; kb < NBH; ++kb) gWhd[hb][kb] = Z4;
    }
#pragma unroll
    for (int j = 0; j < EH_MAX_PARAMS; ++j) gp[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < EH_EVAL_STATS; ++k) est[k] = 0.0f;      // TRAIN: [0] S, [1] Sy, [2] Syy, [3] n

    const bool mae = net.loss == EH_LOSS_MAE;
    const int W = a.W, t_head = a.W - a.ow;
    const long long ntiles = (a.count + 15) / 16;
    float* const ws = TRAIN ? a.ws + (long long)(blockIdx.x * EH_SEQ_NW + wave) * a.ws_wave : nullptr;
    float* const wsh = TRAIN ? ws + (long long)W * PER * NBH * 256 : nullptr;

    for (long long tile = (long long)blockIdx.x * EH_SEQ_NW + wave; tile < ntiles; tile += (long long)gridDim.x * EH_SEQ_NW) {
        const long long kwin = tile * 16 + n;
        const bool live = kwin < a.count;
        const long long kc = live ? kwin : a.count - 1;       // (a lane past the end repeats the last window; it adds nothing)
        const int st = a.starts[a.idx ? a.idx[a.first + kc] : (int)(a.first + kc)];
        int stT[4];                                           // the starts of windows 4g + r (operands with the window on K)
#pragma unroll
        for (int r = 0; r < 4; ++r) stT[r] = __shfl(st, 4 * g + r, 64);

        // ================= forward ==================================================================================
        f32x4 h[NBH], c[NBH];
#pragma unroll
        for (int hb = 0; hb < NBH; ++hb) { h[hb] = Z4; c[hb] = Z4; }
        for (int t = 0; t < W; ++t) {
            const float* const rec = a.recs + (long long)(st + t) * C;
            f32x4 x[NBI];
            dense_in(rec, x);
#pragma unroll
            for (int ib = 0; ib < NBI; ++ib) x[ib] = eh_seq_act4(a.act_in, x[ib]);
            f32x4 hn[NBH];
#pragma unroll
            for (int hb = 0; hb < NBH; ++hb) {
                if constexpr (LSTM) {
                    // the four gate blocks of these 16 rows are independent chains: issued interleaved, each one's dependent MFMA latency
                    // hides behind the issue of the other three
                    f32x4 z[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) z[q] = ldB(G::L_BG, q * RH + hb * 16);
#pragma unroll
                    for (int ib = 0; ib < NBI; ++ib) {
                        f32x4 A[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) A[q] = ldA(G::L_WIH, SI, q * RH + hb * 16, ib * 16);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int q = 0; q < 4; ++q) z[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[q][r], x[ib][r], z[q], 0, 0, 0);
                    }
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb) {
                        f32x4 A[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) A[q] = ldA(G::L_WHH, SH, q * RH + hb * 16, kb * 16);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int q = 0; q < 4; ++q) z[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[q][r], h[kb][r], z[q], 0, 0, 0);
                    }
                    const f32x4 gi = eh_seq_sig4(z[0]), gf = eh_seq_sig4(z[1]), gg = eh_seq_tanh4(z[2]), go = eh_seq_sig4(z[3]);
                    const f32x4 cp = c[hb];
                    c[hb] = gf * cp + gi * gg;
                    const f32x4 tc = eh_seq_tanh4(c[hb]);
                    hn[hb] = go * tc;
                    if constexpr (TRAIN) {
                        f32x4* const w4 = reinterpret_cast<f32x4*>(ws) + ((long long)(t * NBH + hb) * 6) * 64 + lane;
                        w4[0] = gi; w4[64] = gf; w4[128] = gg; w4[192] = go; w4[256] = cp; w4[320] = tc;
                    }
                } else if constexpr (GRU) {
                    // four chains again: r, z, the input half of n, and q = W_hn h + b_hn (the reset gate multiplies q: it is not summed into n's chain)
                    f32x4 z[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) z[q] = ldB(G::L_BG, q * RH + hb * 16);
#pragma unroll
                    for (int ib = 0; ib < NBI; ++ib) {
                        f32x4 A[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) A[q] = ldA(G::L_WIH, SI, q * RH + hb * 16, ib * 16);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int q = 0; q < 3; ++q) z[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[q][r], x[ib][r], z[q], 0, 0, 0);
                    }
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb) {
                        f32x4 A[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) A[q] = ldA(G::L_WHH, SH, q * RH + hb * 16, kb * 16);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int q = 0; q < 3; ++q) z[q == 2 ? 3 : q] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[q][r], h[kb][r], z[q == 2 ? 3 : q], 0, 0, 0);
                    }
                    const f32x4 gr = eh_seq_sig4(z[0]), gz = eh_seq_sig4(z[1]), gq = z[3];
                    const f32x4 gn = eh_seq_tanh4(z[2] + gr * gq);
                    hn[hb] = (1.0f - gz) * gn + gz * h[hb];
                    if constexpr (TRAIN) {
                        f32x4* const w4 = reinterpret_cast<f32x4*>(ws) + ((long long)(t * NBH + hb) * PER) * 64 + lane;
                        w4[0] = gr; w4[64] = gz; w4[128] = gn; w4[192] = gq; w4[256] = hn[hb];
                    }
                } else {
                    f32x4 z = ldB(G::L_BG, hb * 16);
#pragma unroll
                    for (int ib = 0; ib < NBI; ++ib) z = eh_seq_mfma4(ldA(G::L_WIH, SI, hb * 16, ib * 16), x[ib], z);
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb) z = eh_seq_mfma4(ldA(G::L_WHH, SH, hb * 16, kb * 16), h[kb], z);
                    hn[hb] = eh_seq_act4(a.act_cell, z);
                    if constexpr (TRAIN) {
                        f32x4* const w4 = reinterpret_cast<f32x4*>(ws) + ((long long)(t * NBH + hb) * PER) * 64 + lane;
                        w4[0] = z; w4[64] = hn[hb];
                    }
                }
            }
#pragma unroll
            for (int hb = 0; hb < NBH; ++hb) h[hb] = hn[hb];
            if (t < t_head) continue;

            // ---- head: Dense(H -> H, act), Dense(H -> K), sigma-scaling, mechanistic model, residual ----
            const int j_out = t - t_head;
            f32x4 z1[NBH], a1[NBH];
#pragma unroll
            for (int hb = 0; hb < NBH; ++hb) {
                z1[hb] = ldB(G::L_BHD, hb * 16);
#pragma unroll
                for (int kb = 0; kb < NBH; ++kb) z1[hb] = eh_seq_mfma4(ldA(G::L_WHD, SH, hb * 16, kb * 16), h[kb], z1[hb]);
                a1[hb] = eh_seq_act4(a.act_hd, z1[hb]);
            }
            if constexpr (TRAIN && PROG) {                    // (parked before the program runs: the tape then has their registers)
                f32x4* const w4 = reinterpret_cast<f32x4*>(wsh) + (long long)j_out * (NBH + 1) * 64 + lane;
#pragma unroll
                for (int hb = 0; hb < NBH; ++hb) w4[hb * 64] = z1[hb];
            }
            f32x4 ob = ldB(G::L_BOUT, 0);
#pragma unroll
            for (int kb = 0; kb < NBH; ++kb) ob = eh_seq_mfma4(ldA(G::L_WOUT, SH, 0, kb * 16), a1[kb], ob);
            // one window per lane (the four lane groups repeat it; group 0 does the sums)
            float par[EH_MAX_PARAMS], sg[EH_MAX_PARAMS], dydp[EH_MAX_PARAMS], frc[EH_MAX_FORC], ovk[EH_MAX_PARAMS];
#pragma unroll
            for (int k = 0; k < EH_MAX_PARAMS; ++k) ovk[k] = __shfl(ob[k & 3], (k >> 2) * 16 + n, 64);      // NN output row k of this lane's window
#pragma unroll
            for (int j = 0; j < EH_MAX_PARAMS; ++j) {
                par[j] = a.meta[EH_IMG_PHI + j]; sg[j] = 0.0f; dydp[j] = 0.0f;
                const int row = (int)((net.par_idx >> (4 * j)) & 15u);
                float ov = 0.0f;
#pragma unroll
                for (int k = 0; k < EH_MAX_PARAMS; ++k) ov = row == k ? ovk[k] : ov;
                if (j < net.n_par && ((net.par_kind >> (2 * j)) & 3u) == EH_PAR_NEURAL) {
                    if (net.scale_nn) { const float s = eh_sigmoid(ov), sc = a.meta[EH_IMG_SC + j]; par[j] = fmaf(sc, s, a.meta[EH_IMG_LO + j]); sg[j] = sc * s * (1.0f - s); }
                    else { par[j] = ov; sg[j] = 1.0f; }
                }
            }
#pragma unroll
            for (int f = 0; f < EH_MAX_FORC; ++f) {
                const unsigned col = (net.forc_col >> (8 * f)) & 255u;
                frc[f] = col != 255u ? rec[P + col] : 0.0f;
            }
            if constexpr (MT) {                               // several targets: all of the mechanistic stage and the loss (eh_seq_head_targets)
                float yt[EH_MAX_TARG], dp[EH_MAX_PARAMS];
                eh_seq_head_targets<MODE, HEAD>(net, a, par, frc, a.recs + (long long)(st + t + a.lam) * C + P + net.F, live, g == 0, MTA + 16 * (1 + EH_MAX_TARG), MTA + n, yt, dp);
                if constexpr (TRAIN) {                        // (from here on as for one target, below)
                    float dps[EH_MAX_PARAMS];
#pragma unroll
                    for (int j = 0; j < EH_MAX_PARAMS; ++j) {
                        dps[j] = dp[j] * sg[j];
                        if (g == 0 && j < net.n_par && ((net.par_kind >> (2 * j)) & 3u) == EH_PAR_GLOBAL) gp[j] += dp[j];
                    }
                    f32x4 dob = Z4;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                        for (int j = 0; j < EH_MAX_PARAMS; ++j)
                            if (j < net.n_par && ((net.par_kind >> (2 * j)) & 3u) == EH_PAR_NEURAL && (int)((net.par_idx >> (4 * j)) & 15u) == 4 * g + rr) dob[rr] = dps[j];
                    f32x4* const w4 = reinterpret_cast<f32x4*>(wsh) + (long long)j_out * (NBH + 1) * 64 + lane;
                    if constexpr (!PROG) {
#pragma unroll
                        for (int hb = 0; hb < NBH; ++hb) w4[hb * 64] = z1[hb];
                    }
                    w4[NBH * 64] = dob;
                } else if (live && g == 0) {
                    const long long o = kwin * a.ow + j_out;
                    if (a.yhat) {
#pragma unroll
                        for (int tt = 0; tt < EH_MAX_TARG; ++tt)
                            if (tt < net.T) a.yhat[(long long)tt * a.yld + o] = yt[tt];
                    }
                    if (a.pout)
                        for (int j = 0; j < net.n_par; ++j) a.pout[(long long)j * a.yld + o] = par[j];
                }
                continue;
            }
            float y;
#ifdef EH_JIT_MECH
            EhJitTape jtape;                                  // (the generated straight-line program: every slot a named value)
            if constexpr (PROG) {
                const int to = (int)(net.targ_out & 3u);
                float yo[3];
                eh_jit_fwd(par, frc, jtape, yo[0], yo[1], yo[2]);
                y = to == 0 ? yo[0] : (to == 1 ? yo[1] : yo[2]);
            } else {
#else
            float pval[PROG ? EH_PROG_SLOTS : 1];             // the interpreter's tape: a per-lane array (scratch memory)
            if constexpr (PROG) {
                eh_prog_forward(a.prog, par, frc, pval);
                y = pval[a.prog[2 + (net.targ_out & 3u)]];
            } else {
#endif
                y = eh_mech_eval(net.mech, par, frc, dydp);
                if constexpr (HEAD == EH_SEQ_HEAD_MULTI) {    // the target is on output `to`: its value and its Jacobian row
                    const int to = (int)(net.targ_out & 3u);
                    float yx[2] = {0.0f, 0.0f}, Jx[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
                    eh_mech_extra(net.mech, par, frc, yx, Jx);
                    if (to > 0) {
                        y = to == 1 ? yx[0] : yx[1];
#pragma unroll
                        for (int j = 0; j < EH_MAX_PARAMS; ++j) dydp[j] = j < 3 ? (to == 1 ? Jx[0][j] : Jx[1][j]) : 0.0f;
                    }
                }
            }
            const float yobs = a.recs[(long long)(st + t + a.lam) * C + P + net.F];
            const bool valid = live && !__builtin_isnan(yobs);
            const float r = valid ? y - yobs : 0.0f, cy = valid ? yobs - a.shift : 0.0f;
            if constexpr (TRAIN) {
                float d;
                if (mae) { if (g == 0) est[0] += fabsf(r); d = r > 0.0f ? 1.0f : (r < 0.0f ? -1.0f : 0.0f); }
                else { if (g == 0) est[0] = fmaf(r, r, est[0]); d = 2.0f * r; }
                if (g == 0) { est[1] += cy; est[2] = fmaf(cy, cy, est[2]); est[3] += valid ? 1.0f : 0.0f; }
                // the per-parameter adjoint of a closure: the reverse sweep over the tape of this head step, seeded at the target's output
#ifdef EH_JIT_MECH
                float padj[EH_MAX_PARAMS];
                if constexpr (PROG) {
                    const int to = (int)(net.targ_out & 3u);
                    eh_jit_rev(par, frc, jtape, to == 0 ? d : 0.0f, to == 1 ? d : 0.0f, to == 2 ? d : 0.0f, padj);
                }
#else
                float padj[PROG ? EH_PROG_SLOTS : 1];
                if constexpr (PROG) {
                    const int nslot = EH_PROG_SLOT_INSTR + (int)a.prog[0];
                    for (int i = 0; i < nslot; ++i) padj[i] = 0.0f;
                    padj[a.prog[2 + (net.targ_out & 3u)]] += d;
                    eh_prog_reverse(a.prog, pval, padj);
                }
#endif
                float dps[EH_MAX_PARAMS];
#pragma unroll
                for (int j = 0; j < EH_MAX_PARAMS; ++j) {
                    float dp;
                    if constexpr (PROG) dp = valid ? padj[j] : 0.0f;
                    else dp = valid ? d * dydp[j] : 0.0f;
                    dps[j] = dp * sg[j];
                    if (g == 0 && j < net.n_par && ((net.par_kind >> (2 * j)) & 3u) == EH_PAR_GLOBAL) gp[j] += dp;
                }
                f32x4 dob = Z4;                               // d loss / d o in C/D layout: row 4g + r = NN output row
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                    for (int j = 0; j < EH_MAX_PARAMS; ++j)
                        if (j < net.n_par && ((net.par_kind >> (2 * j)) & 3u) == EH_PAR_NEURAL && (int)((net.par_idx >> (4 * j)) & 15u) == 4 * g + rr) dob[rr] = dps[j];
                f32x4* const w4 = reinterpret_cast<f32x4*>(wsh) + (long long)j_out * (NBH + 1) * 64 + lane;
                if constexpr (!PROG) {
#pragma unroll
                    for (int hb = 0; hb < NBH; ++hb) w4[hb * 64] = z1[hb];
                }
                w4[NBH * 64] = dob;
            } else if constexpr (MODE == EH_SEQ_EVAL) {
                if (valid && g == 0) {
                    const float ch = y - a.shift;
                    est[0] = fmaf(r, r, est[0]); est[1] += cy; est[2] = fmaf(cy, cy, est[2]); est[3] += 1.0f;
                    est[4] += ch; est[5] = fmaf(ch, ch, est[5]); est[6] = fmaf(ch, cy, est[6]); est[7] += fabsf(r);
                }
            }
            if constexpr (!TRAIN) {
                if (live && g == 0) {
                    const long long o = kwin * a.ow + j_out;
                    if (a.yhat) a.yhat[o] = y;
                    if (a.pout)
                        for (int j = 0; j < net.n_par; ++j) a.pout[(long long)j * a.yld + o] = par[j];
                }
            }
        }
        if constexpr (!TRAIN) continue;

        // ================= backward through time ====================================================================
        f32x4 dh[NBH], dc[NBH];
#pragma unroll
        for (int hb = 0; hb < NBH; ++hb) { dh[hb] = Z4; dc[hb] = Z4; }
        for (int t = W - 1; t >= 0; --t) {
            const float* const rec = a.recs + (long long)(st + t) * C;
            const f32x4* const w4 = reinterpret_cast<const f32x4*>(ws) + (long long)t * NBH * PER * 64 + lane;
            if (t >= t_head) {
                // ---- head backward: its delta joins dh of this step ----
                const f32x4* const wh = reinterpret_cast<const f32x4*>(wsh) + (long long)(t - t_head) * (NBH + 1) * 64 + lane;
                const f32x4 dob = wh[NBH * 64];
                f32x4 z1[NBH], hT[NBH];
#pragma unroll
                for (int hb = 0; hb < NBH; ++hb) { z1[hb] = wh[hb * 64]; hT[hb] = tr(h_of(w4, hb)); }
                const f32x4 dobT = tr(dob);
                if constexpr (PROG) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float v = eh_row16_sum(dob[r]); if (n == 0) HB[RH + 4 * g + r] += v; }
                } else gBout += dob;
#pragma unroll
                for (int hb = 0; hb < NBH; ++hb) {
                    gWout[hb] = eh_seq_mfma4(dobT, tr(eh_seq_act4(a.act_hd, z1[hb])), gWout[hb]);
                    const f32x4 dz1 = eh_seq_mfma4(ldAT(G::L_WOUT, SH, 0, hb * 16), dob, Z4) * eh_seq_dact4(a.act_hd, z1[hb]);
                    if constexpr (PROG) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) { const float v = eh_row16_sum(dz1[r]); if (n == 0) HB[hb * 16 + 4 * g + r] += v; }
                    } else gBhd[hb] += dz1;
                    const f32x4 dz1T = tr(dz1);
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb) {
                        gWhd[hb][kb] = eh_seq_mfma4(dz1T, hT[kb], gWhd[hb][kb]);
                        dh[kb] = eh_seq_mfma4(ldAT(G::L_WHD, SH, hb * 16, kb * 16), dz1, dh[kb]);
                    }
                }
            }
            // ---- the operands of this step's weight gradients, window on K ----
            f32x4 zx[NBI], xT[NBI], hpT[NBH], hpv[NBH], dhn[NBH], dx[NBI];
            dense_in(rec, zx);
#pragma unroll
            for (int ib = 0; ib < NBI; ++ib) { xT[ib] = tr(eh_seq_act4(a.act_in, zx[ib])); dx[ib] = Z4; }
#pragma unroll
            for (int kb = 0; kb < NBH; ++kb) {
                f32x4 hp = Z4;
                if (t > 0) hp = h_of(w4 - NBH * PER * 64, kb);      // h_{t-1}: the record before (LSTM: o_{t-1} tanh(c_{t-1}))
                hpT[kb] = tr(hp);
                hpv[kb] = hp;                                       // (the GRU's own update reads it untransposed)
                dhn[kb] = Z4;
            }
#pragma unroll
            for (int hb = 0; hb < NBH; ++hb) {
                if constexpr (LSTM) {
                    const f32x4 gi = w4[(hb * 6 + 0) * 64], gf = w4[(hb * 6 + 1) * 64], gg = w4[(hb * 6 + 2) * 64], go = w4[(hb * 6 + 3) * 64],
                                cp = w4[(hb * 6 + 4) * 64], tc = w4[(hb * 6 + 5) * 64];
                    const f32x4 dcn = dc[hb] + dh[hb] * go * (1.0f - tc * tc);
                    f32x4 dz[4];
                    dz[0] = dcn * gg * gi * (1.0f - gi);
                    dz[1] = dcn * cp * gf * (1.0f - gf);
                    dz[2] = dcn * gi * (1.0f - gg * gg);
                    dz[3] = dh[hb] * tc * go * (1.0f - go);
                    dc[hb] = dcn * gf;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) { const float v = eh_row16_sum(dz[q][r]); if (n == 0) GB[q * RH + hb * 16 + 4 * g + r] += v; }
                        const f32x4 dzT = tr(dz[q]);
#pragma unroll
                        for (int ib = 0; ib < NBI; ++ib) gWih[q][hb][ib] = eh_seq_mfma4(dzT, xT[ib], gWih[q][hb][ib]);
#pragma unroll
                        for (int kb = 0; kb < NBH; ++kb) gWhh[q][hb][kb] = eh_seq_mfma4(dzT, hpT[kb], gWhh[q][hb][kb]);
                    }
                    // dh_{t-1} += W_hh^T dz, dx_t += W_ih^T dz: the four gates as interleaved chains again
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb)
#pragma unroll
                        for (int q = 0; q < 4; ++q) dhn[kb] = eh_seq_mfma4(ldAT(G::L_WHH, SH, q * RH + hb * 16, kb * 16), dz[q], dhn[kb]);
#pragma unroll
                    for (int ib = 0; ib < NBI; ++ib)
#pragma unroll
                        for (int q = 0; q < 4; ++q) dx[ib] = eh_seq_mfma4(ldAT(G::L_WIH, SI, q * RH + hb * 16, ib * 16), dz[q], dx[ib]);
                } else if constexpr (GRU) {
                    const f32x4 gr = w4[(hb * 5 + 0) * 64], gz = w4[(hb * 5 + 1) * 64], gn = w4[(hb * 5 + 2) * 64], gq = w4[(hb * 5 + 3) * 64];
                    f32x4 dz[4];                                    // [r | z | n_ih | n_hh]: the GB row's order
                    dz[2] = dh[hb] * (1.0f - gz) * (1.0f - gn * gn);
                    dz[1] = dh[hb] * (hpv[hb] - gn) * gz * (1.0f - gz);
                    dz[0] = dz[2] * gq * gr * (1.0f - gr);
                    dz[3] = dz[2] * gr;
                    dhn[hb] += dh[hb] * gz;
                    f32x4 dzT[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) { const float v = eh_row16_sum(dz[q][r]); if (n == 0) GB[q * RH + hb * 16 + 4 * g + r] += v; }
                        dzT[q] = tr(dz[q]);
                    }
                    // W_ih sees [r | z | n_ih], W_hh [r | z | n_hh]
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
#pragma unroll
                        for (int ib = 0; ib < NBI; ++ib) gWih[q][hb][ib] = eh_seq_mfma4(dzT[q], xT[ib], gWih[q][hb][ib]);
#pragma unroll
                        for (int kb = 0; kb < NBH; ++kb) gWhh[q][hb][kb] = eh_seq_mfma4(dzT[q == 2 ? 3 : q], hpT[kb], gWhh[q][hb][kb]);
                    }
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb)
#pragma unroll
                        for (int q = 0; q < 3; ++q) dhn[kb] = eh_seq_mfma4(ldAT(G::L_WHH, SH, q * RH + hb * 16, kb * 16), dz[q == 2 ? 3 : q], dhn[kb]);
#pragma unroll
                    for (int ib = 0; ib < NBI; ++ib)
#pragma unroll
                        for (int q = 0; q < 3; ++q) dx[ib] = eh_seq_mfma4(ldAT(G::L_WIH, SI, q * RH + hb * 16, ib * 16), dz[q], dx[ib]);
                } else {
                    const f32x4 dz = dh[hb] * eh_seq_dact4(a.act_cell, w4[(hb * 2) * 64]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float v = eh_row16_sum(dz[r]); if (n == 0) GB[hb * 16 + 4 * g + r] += v; }
                    const f32x4 dzT = tr(dz);
#pragma unroll
                    for (int ib = 0; ib < NBI; ++ib) gWih[0][hb][ib] = eh_seq_mfma4(dzT, xT[ib], gWih[0][hb][ib]);
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb) gWhh[0][hb][kb] = eh_seq_mfma4(dzT, hpT[kb], gWhh[0][hb][kb]);
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb) dhn[kb] = eh_seq_mfma4(ldAT(G::L_WHH, SH, hb * 16, kb * 16), dz, dhn[kb]);
#pragma unroll
                    for (int ib = 0; ib < NBI; ++ib) dx[ib] = eh_seq_mfma4(ldAT(G::L_WIH, SI, hb * 16, ib * 16), dz, dx[ib]);
                }
            }
#pragma unroll
            for (int kb = 0; kb < NBH; ++kb) dh[kb] = dhn[kb];
            // ---- Dense-in ----
#pragma unroll
            for (int ib = 0; ib < NBI; ++ib) {
                const f32x4 dzx = dx[ib] * eh_seq_dact4(a.act_in, zx[ib]);
                gBin[ib] += dzx;
                const f32x4 dzxT = tr(dzx);
#pragma unroll
                for (int pb = 0; pb < 2; ++pb)
                    if (pb * 16 < P) {
                        f32x4 pT;                              // predictor pb * 16 + n of windows 4g + r
#pragma unroll
                        for (int r = 0; r < 4; ++r) pT[r] = pb * 16 + n < P ? a.recs[(long long)(stT[r] + t) * C + pb * 16 + n] : 0.0f;
                        gWin[ib][pb] = eh_seq_mfma4(dzxT, pT, gWin[ib][pb]);
                    }
            }
        }
    }

    // ================= epilogue ===========================================================================================
    __syncthreads();                                           // every wave is through with the parameters: the row takes their place
    if constexpr (MODE == EH_SEQ_EVAL && MT) {                 // EH_EVAL_STATS sums per target, the targets one after the other (a.n_acc = EH_EVAL_STATS * T)
        constexpr int NS = EH_EVAL_STATS * EH_MAX_TARG;
#pragma unroll
        for (int t = 0; t < EH_MAX_TARG; ++t)
#pragma unroll
            for (int k = 0; k < EH_EVAL_STATS; ++k) { const float v = eh_wave_sum(g == 0 ? MTA[16 * (t * EH_EVAL_STATS + k) + n] : 0.0f); if (lane == 0) lds[wave * NS + t * EH_EVAL_STATS + k] = v; }
        __syncthreads();
        if (tid < EH_EVAL_STATS * net.T) {
            float s = 0.0f;
            for (int w = 0; w < EH_SEQ_NW; ++w) s += lds[w * NS + tid];
            a.slab[(long long)blockIdx.x * a.n_acc + tid] = s;
        }
    } else if constexpr (MODE == EH_SEQ_EVAL) {
#pragma unroll
        for (int k = 0; k < EH_EVAL_STATS; ++k) { const float v = eh_wave_sum(est[k]); if (lane == 0) lds[wave * EH_EVAL_STATS + k] = v; }
        __syncthreads();
        if (tid < EH_EVAL_STATS) {
            float s = 0.0f;
            for (int w = 0; w < EH_SEQ_NW; ++w) s += lds[w * EH_EVAL_STATS + tid];
            a.slab[(long long)blockIdx.x * a.n_acc + tid] = s;
        }
    }
    if constexpr (TRAIN) {
        float* const row = lds;
        for (int e = tid; e < a.n_acc; e += 64 * EH_SEQ_NW) row[e] = 0.0f;
        __syncthreads();
        constexpr int NSUM = MT ? 1 + EH_MAX_TARG : 4;
        float sums[NSUM], gps[EH_MAX_PARAMS];
#pragma unroll
        for (int k = 0; k < NSUM; ++k) sums[k] = eh_wave_sum(MT ? (g == 0 ? MTA[16 * k + n] : 0.0f) : est[k]);
#pragma unroll
        for (int j = 0; j < EH_MAX_PARAMS; ++j) gps[j] = eh_wave_sum(gp[j]) * a.meta[EH_IMG_DPHI + j];
        // a weight block: register r of lane (n, g) is row r0 + 4g + r (below `lim`), column c0 + n (below `ncol`) of a column-major matrix of `ld` rows
        auto putW = [&](const f32x4& acc, int off, int ld, int rbase, int lim, int r0, int c0, int ncol) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = r0 + 4 * g + r, col = c0 + n;
                if (rl < lim && col < ncol) row[off + col * ld + rbase + rl] += acc[r];
            }
        };
        // a bias block: the 16 windows of a row summed over its lanes
        auto putB = [&](const f32x4& acc, int off, int lim, int r0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = eh_row16_sum(acc[r]);
                const int rl = r0 + 4 * g + r;
                if (n == 0 && rl < lim) row[off + rl] += v;
            }
        };
        for (int w = 0; w < EH_SEQ_NW; ++w) {                  // wave order: the sums meet in one fixed order
            if (wave == w) {
#pragma unroll
                for (int q = 0; q < NG; ++q)
#pragma unroll
                    for (int hb = 0; hb < NBH; ++hb) {
#pragma unroll
                        for (int ib = 0; ib < NBI; ++ib) putW(gWih[q][hb][ib], a.off[EH_SEQ_WIH], NG * H, q * H, H, hb * 16, ib * 16, I);
#pragma unroll
                        for (int kb = 0; kb < NBH; ++kb) putW(gWhh[q][hb][kb], a.off[EH_SEQ_WHH], NG * H, q * H, H, hb * 16, kb * 16, H);
                    }
#pragma unroll
                for (int ib = 0; ib < NBI; ++ib) {
                    putW(gWin[ib][0], a.off[EH_SEQ_WIN], I, 0, I, ib * 16, 0, P);
                    putW(gWin[ib][1], a.off[EH_SEQ_WIN], I, 0, I, ib * 16, 16, P);
                    putB(gBin[ib], a.off[EH_SEQ_BIN], I, ib * 16);
                }
#pragma unroll
                for (int hb = 0; hb < NBH; ++hb) {
#pragma unroll
                    for (int kb = 0; kb < NBH; ++kb) putW(gWhd[hb][kb], a.off[EH_SEQ_WHD], H, 0, H, hb * 16, kb * 16, H);
                    if constexpr (!PROG) putB(gBhd[hb], a.off[EH_SEQ_BHD], H, hb * 16);
                    putW(gWout[hb], a.off[EH_SEQ_WOUT], K, 0, K, 0, hb * 16, H);
                }
                if constexpr (PROG) {
                    for (int e = lane; e < RH + 16; e += 64) {
                        if (e < H) row[a.off[EH_SEQ_BHD] + e] += HB[e];
                        else if (e >= RH && e - RH < K) row[a.off[EH_SEQ_BOUT] + e - RH] += HB[e];
                    }
                } else putB(gBout, a.off[EH_SEQ_BOUT], K, 0);
                if constexpr (GRU) {                           // r and z as below; the n block of b_ih is row 2, that of b_hh row 3
                    for (int e = lane; e < 4 * RH; e += 64)
                        if (e % RH < H) {
                            const int blk = e / RH, o = (blk < 2 ? blk : 2) * H + e % RH;
                            if (blk != 3) row[a.off[EH_SEQ_BIH] + o] += GB[e];
                            if (blk != 2) row[a.off[EH_SEQ_BHH] + o] += GB[e];
                        }
                } else
                for (int e = lane; e < NG * RH; e += 64)       // b_ih and b_hh: the same gradient, written to both
                    if (e % RH < H) { const int o = (e / RH) * H + e % RH; row[a.off[EH_SEQ_BIH] + o] += GB[e]; row[a.off[EH_SEQ_BHH] + o] += GB[e]; }
                if (lane == 0) {
                    if constexpr (MT) {                        // [loss | n_1 .. n_T]: the weights were exact, the sums are final (Sy, Syy behind them stay 0, nobody reads them)
                        row[net.n_theta] += sums[0];
#pragma unroll
                        for (int t = 0; t < EH_MAX_TARG; ++t)
                            if (t < net.T) row[net.n_theta + 1 + t] += sums[1 + t];
                    } else { row[net.n_theta] += sums[0]; row[net.n_theta + 1] += sums[3]; row[net.n_theta + 2] += sums[1]; row[net.n_theta + 3] += sums[2]; }
#pragma unroll
                    for (int j = 0; j < EH_MAX_PARAMS; ++j)
                        if (j < net.n_par && ((net.par_kind >> (2 * j)) & 3u) == EH_PAR_GLOBAL) row[net.g_off + (int)((net.par_idx >> (4 * j)) & 15u)] += gps[j];
                }
            }
            __syncthreads();
        }
        for (int e = tid; e < a.n_acc; e += 64 * EH_SEQ_NW) a.slab[(long long)blockIdx.x * a.n_acc + e] = row[e];
    }
}
#endif
