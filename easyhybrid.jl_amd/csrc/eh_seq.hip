// The sequence-model kernels (eh_seq.hpp) as a translation unit of their own: one instantiation per padded block count of the
// LSTM's input and hidden widths, per mode and per form of the head's mechanistic stage (EH_SEQ_HEAD_*).
#define EH_SEQ_KERNELS
#include "eh_seq.hpp"

int eh_seq_row_cap(int nbi, int nbh) {
    return nbi == 1 ? (nbh == 1 ? EhSeqGeom<1, 1>::L_TILE : EhSeqGeom<1, 2>::L_TILE) : (nbh == 1 ? EhSeqGeom<2, 1>::L_TILE : EhSeqGeom<2, 2>::L_TILE);
}

template <int NBI, int NBH, int HEAD>
static hipError_t seq_go_head(int mode, int grid, hipStream_t s, const EhNet& net, const EhSeqArgs& a) {
    const dim3 g((unsigned)grid), b(64 * EH_SEQ_NW);
    switch (mode) {
        case EH_SEQ_TRAIN: hipLaunchKernelGGL((eh_seq_kernel<NBI, NBH, EH_SEQ_TRAIN, HEAD>), g, b, 0, s, net, a); break;
        case EH_SEQ_EVAL: hipLaunchKernelGGL((eh_seq_kernel<NBI, NBH, EH_SEQ_EVAL, HEAD>), g, b, 0, s, net, a); break;
        case EH_SEQ_FORWARD: hipLaunchKernelGGL((eh_seq_kernel<NBI, NBH, EH_SEQ_FORWARD, HEAD>), g, b, 0, s, net, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template <int NBI, int NBH>
static hipError_t seq_go(int mode, int head, int grid, hipStream_t s, const EhNet& net, const EhSeqArgs& a) {
    switch (head) {
        case EH_SEQ_HEAD_MECH: return seq_go_head<NBI, NBH, EH_SEQ_HEAD_MECH>(mode, grid, s, net, a);
        case EH_SEQ_HEAD_MULTI: return seq_go_head<NBI, NBH, EH_SEQ_HEAD_MULTI>(mode, grid, s, net, a);
        case EH_SEQ_HEAD_PROG: return a.prog ? seq_go_head<NBI, NBH, EH_SEQ_HEAD_PROG>(mode, grid, s, net, a) : hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
}

hipError_t eh_seq_launch(int nbi, int nbh, int mode, int head, int grid, hipStream_t stream, const EhNet& net, const EhSeqArgs& a) {
    if (nbi == 1 && nbh == 1) return seq_go<1, 1>(mode, head, grid, stream, net, a);
    if (nbi == 1 && nbh == 2) return seq_go<1, 2>(mode, head, grid, stream, net, a);
    if (nbi == 2 && nbh == 1) return seq_go<2, 1>(mode, head, grid, stream, net, a);
    if (nbi == 2 && nbh == 2) return seq_go<2, 2>(mode, head, grid, stream, net, a);
    return hipErrorInvalidValue;                                // (no kernel: an error, never another path)
}
