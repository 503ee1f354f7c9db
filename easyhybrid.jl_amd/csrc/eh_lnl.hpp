// LayerNorm layers inside a hidden-layer chain (EH_LAYER_LAYERNORM), on the layer-wise form (eh_lform.hpp): every sample is normalised over
// its own n features, so nothing couples the rows of a minibatch and the layer has no state.  With X [B][n] the row-major activations in
// front of it:
//
//   forward          mu = mean(x), var = mean((x - mu)^2), xh = (x - mu) rstd, Y = act(scale xh + bias)        eh_lnl_fwd_kernel
//                    (training keeps xh [B][n] and rstd [B]; evaluation and prediction run the same pass and keep nothing)
//   backward         dyh = dY .* act',  g = dyh .* scale,  a = mean(g),  b = mean(g .* xh)
//                    dX = rstd (g - a - xh b) .* act'_below                                                    eh_lnl_bwd_kernel
//                    d bias = colsum dyh, d scale = colsum dyh .* xh: the sums of a BatchNorm layer's backward, by its kernels
//                    (eh_bnl_colsum_kernel<true> + eh_bnl_fold_bwd_kernel: fixed chunk order, no atomics, slab row 0)
//
// A row lives in registers: a segment of `seg` lanes (a power of two, 1..64) holds it, PER elements per lane, element k of lane j being
// column j + k seg (so a wave's loads are contiguous).  Rows narrower than a wave share it -- 64 / seg rows per wave, four waves per
// workgroup --, rows wider than 64 take the whole wave with PER = 2, 4, 8 or 16 (n <= EH_MAX_LAYERNORM_WIDTH = 1024).  The mean is taken
// first and the variance from the centred values, both passes over registers; the sums cross lanes as xor butterflies within the segment
// (every lane ends with the same bits), no LDS.
#pragma once
#include "eh_lform.hpp"

struct EhLnlFwdArgs {
    const float* X;          // [B][n] the layer's input
    const float* scale;      // [n] or nullptr (affine = false: 1)
    const float* bias;       // [n] or nullptr (0)
    float* Y;                // [B][n]
    float* Xh;               // [B][n], nullable (evaluation: nothing kept)
    float* rstd;             // [B], nullable
    int B, n, seg, act; float eps;
};
struct EhLnlBwdArgs {
    const float* dY; const float* Xh; const float* Y;      // [B][n]
    const float* scale; const float* bias;                 // [n], nullable
    const float* rstd;                                     // [B]
    const float* Hb; int act_below;                        // what act' of the layer below is taken from (its output; swish: its pre-activation), [B][n]
    float* dX;
    int B, n, seg, act;
};

// the sum over the `seg` lanes of a segment, in every lane of it (a + b and b + a are the same bits: so are the lanes' results)
__device__ __forceinline__ float eh_lnl_seg_sum(float v, int seg) {
    for (int m = seg >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Loads are taken in loops of their own, without a branch between them -- a lane past the row's end or past the batch reads a clamped
// address and drops the value --, so that a lane's PER loads of an operand are in flight together: with a branch around each, every one
// of them waited for the one before (30.8 us per layer and step at n = 1 024, B = 64 against BatchNorm's 22.8).
template <int PER>
__global__ __launch_bounds__(256) void eh_lnl_fwd_kernel(const EhLnlFwdArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & (a.seg - 1);
    const long long r = ((long long)blockIdx.x * 4 + w) * (64 / a.seg) + (lane - j) / a.seg;
    const bool rok = r < a.B;      // (lanes of a row past the batch read row 0 and store nothing, but take part in the butterflies)
    const long long i0 = (rok ? r : 0) * a.n;
    const float nf = (float)a.n;
    float v[PER], sc[PER], bi[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) v[k] = a.X[i0 + min(j + k * a.seg, a.n - 1)];
    if (a.scale) {
#pragma unroll
        for (int k = 0; k < PER; ++k) { const int cc = min(j + k * a.seg, a.n - 1); sc[k] = a.scale[cc]; bi[k] = a.bias[cc]; }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) { sc[k] = 1.0f; bi[k] = 0.0f; }
    }
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        v[k] = j + k * a.seg < a.n ? v[k] : 0.0f;
        s += v[k];
    }
    const float mu = eh_lnl_seg_sum(s, a.seg) / nf;
    float q = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        v[k] = j + k * a.seg < a.n ? v[k] - mu : 0.0f;
        q = fmaf(v[k], v[k], q);
    }
    const float rstd = 1.0f / sqrtf(eh_lnl_seg_sum(q, a.seg) / nf + a.eps);
    if (!rok) return;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = j + k * a.seg;
        const float xh = v[k] * rstd;
        const float y = eh_act_rt(a.act, fmaf(sc[k], xh, bi[k]));
        if (c < a.n) {
            a.Y[i0 + c] = y;
            if (a.Xh) a.Xh[i0 + c] = xh;
        }
    }
    if (a.rstd && j == 0) a.rstd[r] = rstd;
}

template <int PER>
__global__ __launch_bounds__(256) void eh_lnl_bwd_kernel(const EhLnlBwdArgs a) {
#pragma clang fp contract(off)      // (g must be the rounded product its own mean was taken of: fused into g - a it leaves a residue that rstd multiplies -- n = 1 would not give dX = 0)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & (a.seg - 1);
    const long long r = ((long long)blockIdx.x * 4 + w) * (64 / a.seg) + (lane - j) / a.seg;
    const bool rok = r < a.B;
    const long long i0 = (rok ? r : 0) * a.n;
    const float nf = (float)a.n;
    float g[PER], xh[PER], y[PER], hb[PER], sc[PER], bi[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const long long i = i0 + min(j + k * a.seg, a.n - 1);
        g[k] = a.dY[i]; xh[k] = a.Xh[i]; y[k] = a.Y[i]; hb[k] = a.Hb[i];
    }
    if (a.scale) {
#pragma unroll
        for (int k = 0; k < PER; ++k) { const int cc = min(j + k * a.seg, a.n - 1); sc[k] = a.scale[cc]; bi[k] = a.bias[cc]; }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) { sc[k] = 1.0f; bi[k] = 0.0f; }
    }
    const float rs = a.rstd[rok ? r : 0];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const bool ok = rok && j + k * a.seg < a.n;
        const float d = g[k] * eh_dact_rt(a.act, a.act == EH_ACT_SWISH ? fmaf(sc[k], xh[k], bi[k]) : y[k]);      // dyh: the product eh_bnl_colsum_kernel<true> sums for d bias / d scale
        g[k] = ok ? d * sc[k] : 0.0f;
        xh[k] = ok ? xh[k] : 0.0f;
        s1 += g[k]; s2 = fmaf(g[k], xh[k], s2);
    }
    const float ma = eh_lnl_seg_sum(s1, a.seg) / nf, mb = eh_lnl_seg_sum(s2, a.seg) / nf;
    if (!rok) return;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = j + k * a.seg;
        const float dx = rs * ((g[k] - ma) - xh[k] * mb) * eh_dact_rt(a.act_below, hb[k]);
        if (c < a.n) a.dX[i0 + c] = dx;
    }
}
