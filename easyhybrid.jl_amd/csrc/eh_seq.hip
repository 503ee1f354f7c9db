// The sequence-model kernels (eh_seq.hpp): one instantiation per padded block count of the cell's input and hidden widths, per mode and
// per form of the head's mechanistic stage (EH_SEQ_HEAD_*).  Compiled once per recurrent cell (-DEH_SEQ_UNIT_CELL=<EH_SEQ_CELL_*>, the
// Makefile's eh_seq.o / eh_seq_gru.o / eh_seq_rnn.o) so that the cells build side by side; the LSTM's unit also holds the dispatch.
// The kernels of models with several targets are units of their own again (-DEH_SEQ_UNIT_MT=1: eh_seq_mt.o / eh_seq_gru_mt.o /
// eh_seq_rnn_mt.o), around the two head forms that have several outputs.
#define EH_SEQ_KERNELS
#include "eh_seq.hpp"

#ifndef EH_SEQ_UNIT_CELL
#define EH_SEQ_UNIT_CELL EH_SEQ_CELL_LSTM
#endif
#ifndef EH_SEQ_UNIT_MT
#define EH_SEQ_UNIT_MT 0
#endif
#if EH_SEQ_UNIT_CELL == 0
#define EH_SEQ_UNIT_LAUNCH_1 eh_seq_launch_lstm
#elif EH_SEQ_UNIT_CELL == 1
#define EH_SEQ_UNIT_LAUNCH_1 eh_seq_launch_gru
#else
#define EH_SEQ_UNIT_LAUNCH_1 eh_seq_launch_rnn
#endif
#define EH_SEQ_CAT_(a, b) a##b
#define EH_SEQ_CAT(a, b) EH_SEQ_CAT_(a, b)
#if EH_SEQ_UNIT_MT
#define EH_SEQ_UNIT_LAUNCH EH_SEQ_CAT(EH_SEQ_UNIT_LAUNCH_1, _mt)
#else
#define EH_SEQ_UNIT_LAUNCH EH_SEQ_UNIT_LAUNCH_1
#endif
constexpr int CELL = EH_SEQ_UNIT_CELL;
constexpr bool MT = EH_SEQ_UNIT_MT != 0;

template <int NBI, int NBH, int HEAD>
static hipError_t seq_go_head(int mode, int grid, hipStream_t s, const EhNet& net, const EhSeqArgs& a) {
    const dim3 g((unsigned)grid), b(64 * EH_SEQ_NW);
    switch (mode) {
        case EH_SEQ_TRAIN: hipLaunchKernelGGL((eh_seq_kernel<NBI, NBH, EH_SEQ_TRAIN, HEAD, CELL, MT>), g, b, 0, s, net, a); break;
        case EH_SEQ_EVAL: hipLaunchKernelGGL((eh_seq_kernel<NBI, NBH, EH_SEQ_EVAL, HEAD, CELL, MT>), g, b, 0, s, net, a); break;
        case EH_SEQ_FORWARD: hipLaunchKernelGGL((eh_seq_kernel<NBI, NBH, EH_SEQ_FORWARD, HEAD, CELL, MT>), g, b, 0, s, net, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template <int NBI, int NBH>
static hipError_t seq_go(int mode, int head, int grid, hipStream_t s, const EhNet& net, const EhSeqArgs& a) {
    switch (head) {
#if !EH_SEQ_UNIT_MT
        case EH_SEQ_HEAD_MECH: return seq_go_head<NBI, NBH, EH_SEQ_HEAD_MECH>(mode, grid, s, net, a);
#endif
        case EH_SEQ_HEAD_MULTI: return seq_go_head<NBI, NBH, EH_SEQ_HEAD_MULTI>(mode, grid, s, net, a);
        case EH_SEQ_HEAD_PROG: return a.prog ? seq_go_head<NBI, NBH, EH_SEQ_HEAD_PROG>(mode, grid, s, net, a) : hipErrorInvalidValue;
        default: return hipErrorInvalidValue;                   // (several targets around a model with one output: no such kernel)
    }
}

hipError_t EH_SEQ_UNIT_LAUNCH(int nbi, int nbh, int mode, int head, int grid, hipStream_t stream, const EhNet& net, const EhSeqArgs& a) {
    if (MT && mode == EH_SEQ_TRAIN && !a.inv_n) return hipErrorInvalidValue;      // (the weights of the count pre-pass)
    if (nbi == 1 && nbh == 1) return seq_go<1, 1>(mode, head, grid, stream, net, a);
    if (nbi == 1 && nbh == 2) return seq_go<1, 2>(mode, head, grid, stream, net, a);
    if (nbi == 2 && nbh == 1) return seq_go<2, 1>(mode, head, grid, stream, net, a);
    if (nbi == 2 && nbh == 2) return seq_go<2, 2>(mode, head, grid, stream, net, a);
    return hipErrorInvalidValue;                                // (no kernel: an error, never another path)
}

#if EH_SEQ_UNIT_CELL == 0 && !EH_SEQ_UNIT_MT
#define EH_SEQ_UNIT_DECL(name) hipError_t name(int nbi, int nbh, int mode, int head, int grid, hipStream_t stream, const EhNet& net, const EhSeqArgs& a)
EH_SEQ_UNIT_DECL(eh_seq_launch_gru);
EH_SEQ_UNIT_DECL(eh_seq_launch_rnn);
EH_SEQ_UNIT_DECL(eh_seq_launch_lstm_mt);
EH_SEQ_UNIT_DECL(eh_seq_launch_gru_mt);
EH_SEQ_UNIT_DECL(eh_seq_launch_rnn_mt);

template <int C>
static int seq_row_cap(int nbi, int nbh) {
    return nbi == 1 ? (nbh == 1 ? EhSeqGeom<1, 1, C>::L_TILE : EhSeqGeom<1, 2, C>::L_TILE) : (nbh == 1 ? EhSeqGeom<2, 1, C>::L_TILE : EhSeqGeom<2, 2, C>::L_TILE);
}
int eh_seq_row_cap(int nbi, int nbh, int cell) {
    return cell == EH_SEQ_CELL_GRU ? seq_row_cap<EH_SEQ_CELL_GRU>(nbi, nbh) : (cell == EH_SEQ_CELL_RNN ? seq_row_cap<EH_SEQ_CELL_RNN>(nbi, nbh) : seq_row_cap<EH_SEQ_CELL_LSTM>(nbi, nbh));
}

hipError_t eh_seq_launch(int nbi, int nbh, int mode, int head, int grid, hipStream_t stream, const EhNet& net, const EhSeqArgs& a, int cell, bool mt) {
    switch (cell) {
        case EH_SEQ_CELL_LSTM: return mt ? eh_seq_launch_lstm_mt(nbi, nbh, mode, head, grid, stream, net, a) : eh_seq_launch_lstm(nbi, nbh, mode, head, grid, stream, net, a);
        case EH_SEQ_CELL_GRU: return mt ? eh_seq_launch_gru_mt(nbi, nbh, mode, head, grid, stream, net, a) : eh_seq_launch_gru(nbi, nbh, mode, head, grid, stream, net, a);
        case EH_SEQ_CELL_RNN: return mt ? eh_seq_launch_rnn_mt(nbi, nbh, mode, head, grid, stream, net, a) : eh_seq_launch_rnn(nbi, nbh, mode, head, grid, stream, net, a);
        default: return hipErrorInvalidValue;
    }
}
#endif
