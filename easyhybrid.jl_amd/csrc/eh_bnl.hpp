// BatchNorm layers inside a hidden-layer chain (EH_LAYER_BATCHNORM), on the layer-wise form (eh_lform.hpp): the layer couples the samples
// of a minibatch, so it runs as passes of its own between the Dense products.  With X [B][n] the row-major activations in front of it:
//
//   train forward    mu, var = column mean / biased variance of X (all B rows)      eh_bnl_colsum_kernel<false> + eh_bnl_fold_fwd_kernel
//                    xh = (X - mu) rstd,  Y = act(gamma xh + beta)                   eh_bnl_norm_kernel (keeps xh for the backward)
//                    (mu is kept as c + d, c the batch's first row and d the mean about it, and xh taken as ((X - c) - d) rstd: a column
//                     that sits far from zero loses no digits to the rounding of its mean)
//   test forward     the same pass on the running statistics, nothing kept
//   backward         dyh = dY .* act',  s1 = colsum dyh (= d beta),  s2 = colsum dyh .* xh (= d gamma)
//                                                                                    eh_bnl_colsum_kernel<true> + eh_bnl_fold_bwd_kernel
//                    dX = gamma rstd (dyh - s1 / B - xh s2 / B) .* act'_below        eh_bnl_dx_kernel
//
// Column sums: a workgroup of 4 waves takes 64 columns x one chunk of rows (wave w the rows w, w + 4, ...; a wave reads 256 contiguous
// bytes per row), adds its four waves in wave order and leaves one partial row; the fold kernel adds the chunks in chunk order.  No
// atomics: the same bits on every run.  The forward sums are taken about the batch's first row (as eh_bn_stats_kernel does), so
// sum d^2 - (sum d)^2 / B does not cancel for columns far from zero.  The backward is linear in dY: the leaves' sums go to the slab under
// the deferred-normalisation contract of the Dense gradients (row 0; zeros in the other rows).
#pragma once
#include "eh_lform.hpp"

struct EhBnlArgs {
    const float* X;          // [B][n] the layer's input (forward) | dY (backward)
    const float* Xh;         // backward: the kept xh
    const float* Y;          // backward: the layer's output (act' of tanh / sigmoid / relu)
    const float* gamma;      // [n] or nullptr (affine = false: 1)
    const float* beta;       // [n] or nullptr (0)
    float* part;             // [nchunk][2][n]
    int B, n, chunk, act;
};

// BWD = false: sums of d = X - X[0][c] and d^2;  BWD = true: sums of dyh = dY act' and dyh xh
template <bool BWD>
__global__ __launch_bounds__(256) void eh_bnl_colsum_kernel(const EhBnlArgs a) {
#pragma clang fp contract(off)      // (the sums add the ROUNDED dyh, the value eh_bnl_dx_kernel subtracts them from; the fused steps are written out)
    __shared__ float red[2][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * a.chunk, r1 = min(a.B, r0 + a.chunk);
    float s1 = 0.0f, s2 = 0.0f;
    if (c < a.n) {
        const float g = a.gamma ? a.gamma[c] : 1.0f, b = a.beta ? a.beta[c] : 0.0f;
        const float sh = BWD ? 0.0f : a.X[c];
#pragma unroll 4
        for (int r = r0 + w; r < r1; r += 4) {
            const long long i = (long long)r * a.n + c;
            if constexpr (BWD) {
                const float xh = a.Xh[i];
                const float d = a.X[i] * eh_dact_rt(a.act, a.act == EH_ACT_SWISH ? fmaf(g, xh, b) : a.Y[i]);
                s1 += d; s2 = fmaf(d, xh, s2);
            } else {
                const float d = a.X[i] - sh;
                s1 += d; s2 = fmaf(d, d, s2);
            }
        }
    }
    red[0][w][lane] = s1; red[1][w][lane] = s2;
    __syncthreads();
    if (w == 0 && c < a.n) {
        float* p = a.part + (size_t)blockIdx.y * 2 * a.n;
        p[c] = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
        p[a.n + c] = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
    }
}

// the chunks in chunk order -> stat = [c | d | rstd] of the step (mu = c + d); update: run = [mean | var] moves on (Lux: the unbiased variance, m / (m - 1))
__global__ __launch_bounds__(256) void eh_bnl_fold_fwd_kernel(const float* part, int nchunk, const float* X, int B, int n, float eps, float mom, float* stat, float* run, int update) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    float s1 = 0.0f, s2 = 0.0f;
    for (int k = 0; k < nchunk; ++k) { s1 += part[(size_t)k * 2 * n + c]; s2 += part[(size_t)k * 2 * n + n + c]; }
    const float m = (float)B, d = s1 / m;
    const float var = fmaxf(s2 / m - d * d, 0.0f), mu = X[c] + d;
    stat[c] = X[c]; stat[n + c] = d; stat[2 * n + c] = 1.0f / sqrtf(var + eps);
    if (update) {
        run[c] = (1.0f - mom) * run[c] + mom * mu;
        run[n + c] = (1.0f - mom) * run[n + c] + mom * (m > 1.0f ? m / (m - 1.0f) : 1.0f) * var;
    }
}

struct EhBnlNormArgs {
    const float* X; float* Y; float* Xh;      // Xh nullable (test mode: nothing kept)
    const float* mean; const float* second;   // [n] each; second = rstd, or -- from_var -- the running variance
    const float* d;                           // nullable, [n]: train mode, mean = the batch's first row and d the mean about it
    const float* gamma; const float* beta;
    long long tot; int n, act, from_var, vec; float eps;
};
__device__ __forceinline__ float eh_bnl_norm_one(const EhBnlNormArgs& a, float x, int c, float* xh_out) {
    const float r = a.from_var ? 1.0f / sqrtf(a.second[c] + a.eps) : a.second[c];
    const float xh = (a.d ? (x - a.mean[c]) - a.d[c] : x - a.mean[c]) * r;
    *xh_out = xh;
    return eh_act_rt(a.act, fmaf(a.gamma ? a.gamma[c] : 1.0f, xh, a.beta ? a.beta[c] : 0.0f));
}
// elementwise; vec (n % 4 == 0, every block 16-byte aligned): a thread takes four consecutive columns of one row as one 16-byte access
__global__ __launch_bounds__(256) void eh_bnl_norm_kernel(const EhBnlNormArgs a) {
    const long long stride = (long long)gridDim.x * 256;
    if (a.vec) {
        const long long n4 = a.tot >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            const float4 x = reinterpret_cast<const float4*>(a.X)[i];
            const int c = (int)((i << 2) % a.n);
            float4 y, xh;
            y.x = eh_bnl_norm_one(a, x.x, c, &xh.x); y.y = eh_bnl_norm_one(a, x.y, c + 1, &xh.y);
            y.z = eh_bnl_norm_one(a, x.z, c + 2, &xh.z); y.w = eh_bnl_norm_one(a, x.w, c + 3, &xh.w);
            reinterpret_cast<float4*>(a.Y)[i] = y;
            if (a.Xh) reinterpret_cast<float4*>(a.Xh)[i] = xh;
        }
        return;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.tot; i += stride) {
        float xh;
        a.Y[i] = eh_bnl_norm_one(a, a.X[i], (int)(i % a.n), &xh);
        if (a.Xh) a.Xh[i] = xh;
    }
}

// the chunks in chunk order -> sums = [s1 | s2] for eh_bnl_dx_kernel; affine: d gamma = s2, d beta = s1 into slab row 0, zeros into the other rows
__global__ __launch_bounds__(256) void eh_bnl_fold_bwd_kernel(const float* part, int nchunk, int n, float* sums, float* dgamma, float* dbeta, int nrows, long long n_acc) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    float s1 = 0.0f, s2 = 0.0f;
    for (int k = 0; k < nchunk; ++k) { s1 += part[(size_t)k * 2 * n + c]; s2 += part[(size_t)k * 2 * n + n + c]; }
    sums[c] = s1; sums[n + c] = s2;
    if (dgamma) {
        dgamma[c] = s2; dbeta[c] = s1;
        for (int r = 1; r < nrows; ++r) { dgamma[(size_t)r * n_acc + c] = 0.0f; dbeta[(size_t)r * n_acc + c] = 0.0f; }
    }
}

struct EhBnlDxArgs {
    const float* dY; const float* Xh; const float* Y;      // [B][n]
    const float* gamma; const float* beta; const float* rstd; const float* sums;      // [n] (gamma, beta nullable), [n], [2][n]
    const float* Hb; int act_below;                        // what act' of the layer below is taken from (its output; swish: its pre-activation), [B][n]
    float* dX;
    long long tot; int n, act, vec; float inv_b;
};
__device__ __forceinline__ float eh_bnl_dx_one(const EhBnlDxArgs& a, float dy, float xh, float y, float hb, int c) {
#pragma clang fp contract(off)      // (dyh must be the rounded product the column sums added up: fused into dyh - s1 it leaves a residue that rstd multiplies -- B = 1 would not give dX = 0)
    const float g = a.gamma ? a.gamma[c] : 1.0f, b = a.beta ? a.beta[c] : 0.0f;
    const float d = dy * eh_dact_rt(a.act, a.act == EH_ACT_SWISH ? fmaf(g, xh, b) : y);
    const float s1 = a.sums[c] * a.inv_b, s2 = a.sums[a.n + c] * a.inv_b;
    const float dx = g * a.rstd[c] * ((d - s1) - xh * s2);
    return dx * eh_dact_rt(a.act_below, hb);
}
__global__ __launch_bounds__(256) void eh_bnl_dx_kernel(const EhBnlDxArgs a) {
    const long long stride = (long long)gridDim.x * 256;
    if (a.vec) {
        const long long n4 = a.tot >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            const float4 dy = reinterpret_cast<const float4*>(a.dY)[i], xh = reinterpret_cast<const float4*>(a.Xh)[i];
            const float4 y = reinterpret_cast<const float4*>(a.Y)[i], hb = reinterpret_cast<const float4*>(a.Hb)[i];
            const int c = (int)((i << 2) % a.n);
            float4 o;
            o.x = eh_bnl_dx_one(a, dy.x, xh.x, y.x, hb.x, c); o.y = eh_bnl_dx_one(a, dy.y, xh.y, y.y, hb.y, c + 1);
            o.z = eh_bnl_dx_one(a, dy.z, xh.z, y.z, hb.z, c + 2); o.w = eh_bnl_dx_one(a, dy.w, xh.w, y.w, hb.w, c + 3);
            reinterpret_cast<float4*>(a.dX)[i] = o;
        }
        return;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.tot; i += stride)
        a.dX[i] = eh_bnl_dx_one(a, a.dY[i], a.Xh[i], a.Y[i], a.Hb[i], (int)(i % a.n));
}
