// OptimiserChain on the device (Optimisers.jl: ClipGrad, ClipNorm, WeightDecay around one rule).  Included by eh_api.hip only, behind
// eh_kernels.hpp.
//
// A handle with a chain runs the step kernel it runs anyway, then eh_reduce_kernel<false, ...> -- which leaves the finished gradient
// in gradbuf[0 .. n_theta) with the loss and the valid counts behind it -- and then the kernels below, which read gradbuf:
//
//   eh_chain_norm_kernel           sum |t|^p (or max |t|) of t = the stages in front of ClipNorm applied to g: one partial per workgroup
//   eh_chain_apply_kernel<false>   every workgroup folds the partials (same order everywhere: same lambda), then per element the
//                                  stages in order, the rule through eh_opt_update_at, the stages behind it; theta, m, v, the image
//   eh_chain_apply_kernel<true>    both in ONE workgroup, where n_theta is small enough for that to be faster (EH_CHAIN_ONE_MAX)
//
// Every sum runs in a fixed order (a thread's elements in ascending order, xor butterfly over the wave, the four waves as (0+1)+(2+3),
// the partials the same way): no atomics, the same bits run to run.  The sums are kept in double: 4 n_theta flops that nobody sees,
// and sum g^2 then neither overflows nor carries a rounding error worth speaking of into lambda.
// The data-parallel seam (eh_dp_apply) hands over the all-reduced RAW sums: EhChainSrc::raw makes the gradient from them exactly as
// eh_apply_kernel does (scale, weight_l2 term), so the norm there is the norm of the globally normalised gradient.
#pragma once
#include "eh_internal.hpp"

// n_theta up to which one workgroup takes norm and update in one launch (4 elements per thread).  Measured (tools/bench_chain.py,
// profiles/r13/chain_step.txt): at 338 parameters one launch adds 4.5 us to the step where norm kernel + apply kernel add 7.8; at 2 222
// (9 dependent elements per thread) it adds 10.0 against 6.3 -- about 3 us + 0.8 us per element of a thread, so the two meet near 1 100.
enum { EH_CHAIN_ONE_MAX = 1024 };
enum { EH_CHAIN_PARTS = 256 };         // workgroups of the norm pass at most = partials the apply pass folds, one per thread

struct EhChainSrc {
    int raw;                           // gradbuf = [raw sums | S | n_t .. | Sy | Syy] (data-parallel seam) instead of [gradient | loss | n_t ..]
    int loss_kind, T;
    unsigned tp_mask;
    const float* mom;
    const float* l2val;
};
struct EhChainHead { float cnt, scale, loss; };

// valid samples of the step; raw: also the scale of the sums and the loss value, as eh_apply_kernel makes them
__device__ __forceinline__ EhChainHead eh_chain_head(const float* gradbuf, int n_theta, const EhChainSrc& s, const EhImg& im) {
    EhChainHead hd{gradbuf[n_theta + 1], 1.0f, 0.0f};
    if (!s.raw) {
        for (int t = 1; t < s.T; ++t) hd.cnt += gradbuf[n_theta + 1 + t];
        return hd;
    }
    if (s.T == 1 && !s.tp_mask) eh_loss_finish(s.loss_kind, gradbuf[n_theta], hd.cnt, gradbuf[n_theta + 2], gradbuf[n_theta + 3], hd.scale, hd.loss, im.agg_a);
    else {
        for (int t = 1; t < s.T; ++t) hd.cnt += gradbuf[n_theta + 1 + t];
        hd.scale = hd.cnt > 0.0f ? 1.0f : 0.0f;
        hd.loss = hd.cnt > 0.0f ? gradbuf[n_theta] : __builtin_nanf("");
        if (s.mom && hd.cnt > 0.0f)
            for (int t = 0; t < s.T; ++t) hd.loss += ((s.tp_mask >> t) & 1u) ? s.mom[EH_TT * t + 7] : 0.0f;
    }
    if (s.l2val && hd.cnt > 0.0f) hd.loss += *s.l2val;
    return hd;
}
__device__ __forceinline__ float eh_chain_grad(const float* gradbuf, int idx, float th, const EhChainSrc& s, const EhChainHead& hd, const EhImg& im) {
    float g = gradbuf[idx];
    if (s.raw) {
        g *= hd.scale;
        if (s.l2val) { const float c2 = eh_l2_coef(im, idx); if (c2 != 0.0f) g = fmaf(2.0f * c2, th, g); }
    }
    return g;
}

// stages [lo, hi) of the chain on dx (none of them the rule); x = the parameter, lam = ClipNorm's factor.  Comparisons instead of
// fminf / fmaxf: Julia's clamp hands a NaN through, C's functions drop it.
__device__ __forceinline__ float eh_chain_stages(const EhChain& c, int lo, int hi, float dx, float x, float lam) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < EH_MAX_OPT_STAGES; ++k) {
        if (k < lo || k >= hi) continue;
        const float a = c.a[k];
        if (c.kind[k] == EH_STAGE_CLIPGRAD) dx = dx < -a ? -a : (dx > a ? a : dx);
        else if (c.kind[k] == EH_STAGE_WEIGHTDECAY) dx = dx + a * x;
        else if (c.kind[k] == EH_STAGE_CLIPNORM) dx = dx * lam;
    }
    return dx;
}

__device__ __forceinline__ double eh_chain_term(int p, float t) {
    const double a = fabs((double)t);
    return p == 2 ? a * a : a;
}
// (NaN stays: the comparison form of max keeps a NaN on either side)
__device__ __forceinline__ double eh_chain_comb(int p, double a, double b) { return p == 0 ? ((a > b || a != a) ? a : b) : a + b; }
// one value per thread of a 256-thread workgroup -> the same total in every thread
__device__ __forceinline__ double eh_chain_fold(int p, double a, double (&red)[4]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = eh_chain_comb(p, a, __shfl_xor(a, off, 64));
    __syncthreads();                                   // (red may still be read from a fold before this one)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    return eh_chain_comb(p, eh_chain_comb(p, red[0], red[1]), eh_chain_comb(p, red[2], red[3]));
}

__global__ __launch_bounds__(256) void eh_chain_norm_kernel(const float* __restrict__ gradbuf, int n_theta, const float* __restrict__ theta, EhChain c, EhChainSrc s,
                                                            EhImg im, double* __restrict__ part) {
    __shared__ double red[4];
    const EhChainHead hd = eh_chain_head(gradbuf, n_theta, s, im);
    double acc = 0.0;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n_theta; idx += gridDim.x * 256) {
        const float x = theta[idx];
        const float t = eh_chain_stages(c, 0, c.i_norm, eh_chain_grad(gradbuf, idx, x, s, hd, im), x, 1.0f);
        acc = eh_chain_comb(c.p, acc, eh_chain_term(c.p, t));
    }
    const double tot = eh_chain_fold(c.p, acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// ctr: [0] steps applied  [1] of them with lambda < 1  [2] steps with a non-finite norm (under `throw` they were not applied)
template <bool ONE>
__global__ __launch_bounds__(256) void eh_chain_apply_kernel(const float* __restrict__ gradbuf, int n_theta, float* theta, float* m, float* v, const float* sc_in,
                                                             float* sc_out, EhOpt o, EhChain c, EhChainSrc s, EhImg im, const double* __restrict__ part, int n_part,
                                                             float* loss_slot, unsigned long long* ctr) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const EhChainHead hd = eh_chain_head(gradbuf, n_theta, s, im);
    bool use_m, use_v;
    eh_opt_keeps(o, use_m, use_v);
    const float bt1 = sc_in[0], bt2 = sc_in[1];
    const int stride = ONE ? 256 : gridDim.x * 256;
    float lam = 1.0f, nrm = 0.0f;
    if (c.i_norm >= 0) {
        double acc = 0.0;
        if (ONE) {
            for (int idx = tid; idx < n_theta; idx += 256) {
                const float x = theta[idx];
                const float t = eh_chain_stages(c, 0, c.i_norm, eh_chain_grad(gradbuf, idx, x, s, hd, im), x, 1.0f);
                acc = eh_chain_comb(c.p, acc, eh_chain_term(c.p, t));
            }
        } else if (tid < n_part) acc = part[tid];
        const double tot = eh_chain_fold(c.p, acc, red);
        nrm = (float)(c.p == 2 ? sqrt(tot) : tot);
        const float r = c.omega / nrm;
        lam = r != r ? r : (r < 1.0f ? r : 1.0f);       // min(omega / nrm, 1) as Julia's min: a NaN goes through
    }
    const bool finite = __builtin_isfinite(nrm);
    const bool upd = hd.cnt > 0.0f && !(c.thr && !finite);
    if (upd) {
        for (int idx = blockIdx.x * 256 + tid; idx < n_theta; idx += stride) {
            float th, mm, vv;
            eh_opt_load_one(theta, m, v, idx, use_m, use_v, th, mm, vv);
            const float x = th;
            float dx = eh_chain_stages(c, 0, c.i_rule, eh_chain_grad(gradbuf, idx, x, s, hd, im), x, lam);
            if (c.i_rule + 1 == c.n) eh_opt_update_at(o, sc_in, idx, dx, bt1, bt2, th, mm, vv);      // the rule last: today's call, today's bits
            else {
                // the rule's dx for the stages behind it: the same call on a parameter of 0 leaves exactly -dx (every rule ends in
                // `th -= upd`); AdamW's decay term reads the parameter, so it is added here, in the order eh_opt_update adds it
#pragma clang fp contract(off)
                EhOpt o0 = o;
                if (o.rule == EH_OPT_ADAMW) o0.rule = EH_OPT_ADAM;
                float z = 0.0f;
                eh_opt_update_at(o0, sc_in, idx, dx, bt1, bt2, z, mm, vv);
                dx = -z;
                if (o.rule == EH_OPT_ADAMW) dx = dx + o.lr * o.wd * x;
                dx = eh_chain_stages(c, c.i_rule + 1, c.n, dx, x, lam);
                th = x - dx;
            }
            eh_opt_store_one(theta, m, v, idx, use_m, use_v, th, mm, vv);
            eh_image_store(im, idx, th);
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        eh_opt_advance_one(o, sc_out, upd, bt1, bt2);      // (a chain has one rule: no groups)
        if (s.raw && loss_slot) *loss_slot = hd.loss;      // (not raw: eh_reduce_kernel has written it)
        if (hd.cnt > 0.0f) {
            if (upd) { ctr[0] = ctr[0] + 1ull; if (lam < 1.0f) ctr[1] = ctr[1] + 1ull; }
            if (!finite) ctr[2] = ctr[2] + 1ull;
        }
    }
}
