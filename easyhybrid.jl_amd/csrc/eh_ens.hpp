// Ensembles (eh_ens.hip): M models of ONE handle's architecture -- the folds of a cross-validation, the points of a
// hyper-parameter sweep, repeated seeds -- each trained by a workgroup of its own in one launch.  The launch is the multi-step launch
// (EH_MODE_TRAIN_MULTI, eh_device.hpp) with a member axis: grid (1, M), blockIdx.y the member.  The step body counts tiles, slab rows and shards
// with blockIdx.x / gridDim.x only, so with grid.x == 1 a member's workgroup sees exactly what the one workgroup of a multi-step launch
// sees, and computes the same bits.
#pragma once
#include "eh_device.hpp"

// What differs between the members, one record per member in device memory; everything else (the data table, the maps, the geometry,
// the batch size) is the shared kernel argument.  The workgroup reads its record once -- the address depends on blockIdx.y alone, so
// these are scalar loads -- and patches a private copy of the arguments.
struct EhEnsMember {
    float* pset;             // [2][3][n_theta] + the beta products, as EhFused::pset
    float* gacc;             // [3][EH_GSHARDS][n_acc] + 4
    float* image;            // the member's parameter image: staged by its first step, written back when the launch ends
    float* bn_run;           // [2][32] running statistics of the input BatchNorm
    const int* idx;          // the member's row order of this epoch: rows_j o perm(n_j, seed_j)
    float* ms_loss;          // the loss of the launch's step k goes to ms_loss[k]
    long long first, ms_end; // this launch starts at idx[first]; the member has ms_end rows
    int nsteps;              // steps of this launch; 0: the workgroup returns at once (a finished, empty or inactive member)
    int gslot, cur, sc_sel, pending;      // the member's own rotation state (an idle launch must not flip it: the host advances it per member)
    int rule;                // EhOpt of the member (eh_opt_update looks at the rule at run time)
    float lr, b1, b2, eps, wd;
    int pad;
};
static_assert(sizeof(EhEnsMember) % 8 == 0, "records are read as an array");
// one member's share of eh_ens_order_kernel (eh_kernels.hpp): out[i] = rows[perm(n, seed)(i)], i < n; rows == nullptr: the identity
struct EhEnsOrder {
    const int* rows;
    int* out;
    unsigned long long seed;
    unsigned n;
    int hb;                  // half the bits of n, as eh_perm_kernel takes them
};

#ifdef EH_SPEC_NS
namespace EH_SPEC_NS {
#endif
// The loop is the one of eh_step_kernel's EH_MODE_TRAIN_MULTI branch (eh_device.hpp), step for step -- the same LDS layout behind the
// work space, the same arguments into the same eh_step_body instantiation, the same write-back -- with the member's fields read from
// its record where that branch reads the kernel arguments.  It is a copy, not a shared function: moving the branch's body into one
// changed the code of all 319 multi-step instantiations that exist (tools/kernel_code_hashes.py), and those stay as they are.
// No workgroup of this launch reads or writes a word another one touches -- no flags, no tickets, no atomics on shared words: a member
// never waits, so it cannot hang.
template <int NBI, int NBH, int NL, int NT, int NW, int ACT, int FAST>
__global__ __launch_bounds__(64 * NW, (NW + 3) / 4) void eh_ens_kernel(const EhNet net, const EhStepArgs a, const EhEnsMember* __restrict__ mem) {
    eh_kernarg_warm<(int)(sizeof(EhNet) + sizeof(EhStepArgs))>();
    const EhEnsMember r = mem[blockIdx.y];
    if (r.nsteps <= 0) return;      // (uniform over the workgroup, ahead of every barrier and of the set flip)
    extern __shared__ __attribute__((aligned(16))) float eh_ms_smem[];
    using G = EhGeom<NBI, NBH, NL, NT, NW>;
    constexpr int NTHR = 64 * NW;
#ifdef EH_SPEC_NET
    constexpr EhNet cnet = {EH_SPEC_NET};
    const int nth = cnet.n_theta, g_off = cnet.g_off;
#else
    const int nth = net.n_theta, g_off = net.g_off;
#endif
    const int np = 6 * nth + 4, ng = 3 * EH_GSHARDS * a.n_acc + 4;      // (one rule per member: four running products)
    float* const l_pset = eh_ms_smem + G::TOTAL_FLOATS;
    float* const l_gacc = l_pset + ((np + 3) & ~3);
    int* const l_imap = reinterpret_cast<int*>(l_gacc + ((ng + 3) & ~3));
    for (int i = threadIdx.x; i < np; i += NTHR) l_pset[i] = r.pset[i];
    for (int i = threadIdx.x; i < ng; i += NTHR) l_gacc[i] = r.gacc[i];
    for (int i = threadIdx.x; i < g_off; i += NTHR) l_imap[i] = a.fz.imap[i];
    __syncthreads();
    EhCarry<(G::IP + 3) / 4> carry;
    carry.valid = false; carry.live = false;
    for (int k = 0; k < r.nsteps; ++k) {
        EhStepArgs b = a;
        b.idx = r.idx; b.image = r.image; b.image_out = r.image; b.bn_run = r.bn_run;
        b.first = r.first + (long long)k * a.ms_batch;
        const long long left = r.ms_end - b.first;
        b.count = left < (long long)a.ms_batch ? left : (long long)a.ms_batch;
        b.pf_first = b.first + a.ms_batch;
        b.pf_count = k + 1 < r.nsteps ? (left - a.ms_batch < (long long)a.ms_batch ? left - a.ms_batch : (long long)a.ms_batch) : 0;
        if (b.pf_count < 0) b.pf_count = 0;
        b.fz.pset = l_pset; b.fz.gacc = l_gacc; b.fz.imap = l_imap;
        b.fz.gslot = r.gslot;
        b.fz.cur = r.cur;
        b.fz.sc_sel = r.sc_sel;
        b.fz.pending = k ? 0 : r.pending;
        b.fz.loss_slot = nullptr;
        b.fz.opt.rule = r.rule; b.fz.opt.lr = r.lr; b.fz.opt.b1 = r.b1; b.fz.opt.b2 = r.b2; b.fz.opt.eps = r.eps; b.fz.opt.wd = r.wd; b.fz.opt.tab = nullptr;
        b.ms_nsteps = r.nsteps; b.ms_end = r.ms_end;
        b.ms_loss = r.ms_loss ? r.ms_loss + k : nullptr;
        b.ms_keep = k > 0;
        b.ms_direct = 1;
        eh_step_body<NBI, NBH, NL, NT, NW, ACT, EH_MODE_TRAIN, FAST>(net, b, &carry);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < a.n_acc; i += NTHR) l_gacc[(r.gslot * EH_GSHARDS) * a.n_acc + i] = 0.0f;      // (the steps used shard 0 of this slot as a plain array)
    __syncthreads();
    for (int i = threadIdx.x; i < np; i += NTHR) r.pset[i] = l_pset[i];
    for (int i = threadIdx.x; i < ng; i += NTHR) r.gacc[i] = l_gacc[i];
    // the member's parameter image goes back as it stands in LDS, except its normalisation block (the running statistics: written by the steps)
    for (int i = threadIdx.x; i < G::IMG_FLOATS; i += NTHR) {
        const int q = i - (G::PHI_OFF + EH_IMG_BNM);
        if (q < 0 || q >= 64) r.image[i] = eh_ms_smem[i];
    }
}
#ifdef EH_SPEC_NS
}   // namespace EH_SPEC_NS
using namespace EH_SPEC_NS;
#endif
