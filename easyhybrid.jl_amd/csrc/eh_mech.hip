// The stand-alone mechanistic stage as a translation unit of its own: eh_mech_loss_vjp and its four kernels (launched nowhere else).
#include "eh_internal.hpp"

// ---------------------------------------------------------------------------------------------------------------------
// Mechanistic stage on its own (eh_mech_loss_vjp): o = NN outputs of an MLP that lives OUTSIDE this library -> physical
// parameters (sigma-scaling) -> M(par, forcings) -> masked MSE summed over the targets -> d loss / d o and the gradient of
// the raw global parameters.  Pure streaming: 4 (K + F + T) bytes read and 4 K written per sample, ~20-60 flop -- the one
// stage of the path that the HBM roof bounds.  Every lane owns V consecutive samples (V = 4: 16-byte
// loads and stores, a wave covers 1 KiB runs of every array); sums leave a workgroup once, as one row of partials.
// ---------------------------------------------------------------------------------------------------------------------
struct EhMechArgs {
    const float* o;                          // [K][ld] NN outputs (raw)
    const float* frc[EH_MAX_FORC];           // the F forcing arrays in eh_set_data order
    const float* y[EH_MAX_TARG];             // the T target arrays (NaN = missing)
    float* d_o;                              // [K][ld] d loss / d o
    float* yhat;                             // [T][ld] or nullptr
    long long n, ld;
    const float* meta;                       // parameter image, PHI block (values / d value d raw of the global and fixed parameters, lo, hi - lo)
    const unsigned long long* counts;        // valid samples per target (whole call), counted on the device ...
    unsigned long long counts_v[EH_MAX_TARG];   // ... or handed in by the caller (use_v)
    int use_v;
    float* part;                             // [gridDim.x][EH_MECH_PART] partial sums
    const unsigned* prog;                    // EH_MECH_PROGRAM: the recorded closure (EhStepArgs::prog layout)
    float agg_a;                             // factor of `agg` on the data loss (EhImg::agg_a)
    int tiles;                               // > 0: workgroup b owns the `tiles` consecutive 256 V-sample tiles from b * tiles (a front that moves through memory
                                             // with the dispatch order); 0: grid-stride trips (a capped grid)
};
enum { EH_MECH_PART = 16 };                  // [dL/dpar_j (8) | S_t (4) | pad]

template <int V>
__global__ __launch_bounds__(256) void eh_count_valid_kernel(EhMechArgs a, int T, unsigned long long* counts) {
    unsigned c[EH_MAX_TARG] = {0, 0, 0, 0};
    const long long stride = (long long)gridDim.x * 256 * V;
    for (long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V; i0 < a.n; i0 += 4 * stride)
#pragma unroll
        for (int t = 0; t < EH_MAX_TARG; ++t)
            if (t < T) {
                if constexpr (V == 4) {
                    f32x4 v[4];                                  // four trips requested before the first is examined
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = i0 + u * stride < a.n ? *(const f32x4*)(a.y[t] + i0 + u * stride) : f32x4{0, 0, 0, 0};
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (i0 + u * stride < a.n) c[t] += !__builtin_isnan(v[u][0]) + !__builtin_isnan(v[u][1]) + !__builtin_isnan(v[u][2]) + !__builtin_isnan(v[u][3]);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (i0 + u * stride < a.n) c[t] += !__builtin_isnan(a.y[t][i0 + u * stride]);
                }
            }
    __shared__ unsigned sh[4][EH_MAX_TARG];
#pragma unroll
    for (int t = 0; t < EH_MAX_TARG; ++t) {
        unsigned v = c[t];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < T) atomicAdd(&counts[threadIdx.x], (unsigned long long)(sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x]));
}

// (parameters, forcings, outputs) of a registry model: compile-time array sizes, so that a two-parameter model keeps a dozen
// values per sample in registers, not the 8 + 4 + 4 of the largest one (occupancy is what a streaming kernel lives on)
// (EH_MECH_PROGRAM, a recorded closure run by the interpreter of eh_device.hpp: the limits of the program format)
constexpr int eh_mech_np(int m) { return m == EH_MECH_PROGRAM ? EH_MAX_PARAMS : m == EH_MECH_EXPO2POOL ? 4 : (m == EH_MECH_RS_COMPONENTS || m == EH_MECH_RS_COMPONENTS3F) ? 6 : m == EH_MECH_FLUXPART ? 3 : 2; }
constexpr int eh_mech_nf(int m) { return m == EH_MECH_PROGRAM ? EH_MAX_FORC : m == EH_MECH_FLUXPART ? 2 : m == EH_MECH_RS_COMPONENTS3F ? 3 : 1; }
constexpr int eh_mech_no(int m) { return (m == EH_MECH_PROGRAM || m == EH_MECH_FLUXPART) ? 3 : 1; }

// (RbQ10: 68 VGPRs, seven waves per SIMD.  Forcing eight -- amdgpu_waves_per_eu(8): 64 VGPRs -- spills two registers, and a kernel
// with ANY scratch pays for the allocation at every wave launch, which a launch of tens of thousands of short workgroups cannot afford.)
template <int V, int MECH>
__global__ __launch_bounds__(256) void eh_mech_vjp_kernel(const EhNet net, EhMechArgs a) {
    constexpr int NP = eh_mech_np(MECH), NF = eh_mech_nf(MECH), NO = eh_mech_no(MECH), NTG = NO > 1 ? EH_MAX_TARG : 1;
    float cpar[NP], lo[NP], sc[NP], w[NTG];
    int row[NP];                                                 // NN output row of a neural parameter, -1 otherwise
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        cpar[j] = a.meta[EH_IMG_PHI + j]; lo[j] = a.meta[EH_IMG_LO + j]; sc[j] = a.meta[EH_IMG_SC + j];
        row[j] = (((net.par_kind >> (2 * j)) & 3u) == EH_PAR_NEURAL) ? (int)((net.par_idx >> (4 * j)) & 15u) : -1;
    }
#pragma unroll
    for (int t = 0; t < NTG; ++t) {
        const unsigned long long c = a.use_v ? a.counts_v[t] : a.counts[t];
        w[t] = (t < net.T && c > 0) ? a.agg_a / (float)c : 0.0f;
    }
    float gp[NP], S[NTG];
    const bool mae = net.loss == EH_LOSS_MAE;
#pragma unroll
    for (int j = 0; j < NP; ++j) gp[j] = 0.0f;
#pragma unroll
    for (int t = 0; t < NTG; ++t) S[t] = 0.0f;
    const long long i_first = a.tiles > 0 ? ((long long)blockIdx.x * a.tiles * 256 + threadIdx.x) * V : ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    const long long i_step = a.tiles > 0 ? 256ll * V : (long long)gridDim.x * 256 * V;
    // (no std::min here: it takes references, and a reference to a member of the by-value kernarg struct makes the compiler copy the
    // whole struct to scratch -- 200 bytes per lane and 24 VGPRs more, measured)
    const long long n_all = a.n, tile_end = (long long)(blockIdx.x + 1) * a.tiles * 256 * V;
    const long long i_end = (a.tiles > 0 && tile_end < n_all) ? tile_end : n_all;
    for (long long i = i_first; i < i_end; i += i_step) {
        float ov[NP][V], fv[NF][V], yv[NTG][V], dov[NP][V], yh[NTG][V];
        auto ld = [&](const float* p, float (&dst)[V]) {
            if constexpr (V == 4) { const f32x4 v = *(const f32x4*)(p + i); dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3]; }
            else dst[0] = p[i];
        };
        auto st = [&](float* p, const float (&src)[V]) {
            if constexpr (V == 4) *(f32x4*)(p + i) = f32x4{src[0], src[1], src[2], src[3]};
            else p[i] = src[0];
        };
        // every load of the tile is requested before the first use
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (row[j] >= 0) ld(a.o + (long long)row[j] * a.ld, ov[j]);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const unsigned col = (net.forc_col >> (8 * f)) & 255u;
            if (col != 255u) ld(a.frc[col], fv[f]);
            else
#pragma unroll
                for (int e = 0; e < V; ++e) fv[f][e] = 0.0f;
        }
#pragma unroll
        for (int t = 0; t < NTG; ++t)
            if (t < net.T) ld(a.y[t], yv[t]);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float par[EH_MAX_PARAMS], sg[NP], frc[EH_MAX_FORC];
#pragma unroll
            for (int j = NP; j < EH_MAX_PARAMS; ++j) par[j] = 0.0f;
#pragma unroll
            for (int f = NF; f < EH_MAX_FORC; ++f) frc[f] = 0.0f;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                par[j] = cpar[j]; sg[j] = 0.0f;
                if (row[j] >= 0) {
                    if (net.scale_nn) { const float s = eh_sigmoid(ov[j][e]); par[j] = fmaf(sc[j], s, lo[j]); sg[j] = sc[j] * s * (1.0f - s); }
                    else { par[j] = ov[j][e]; sg[j] = 1.0f; }
                }
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) frc[f] = fv[f][e];
            constexpr bool PROG = MECH == EH_MECH_PROGRAM;
            EhMechTape<PROG> tape;
            float y0, yx[2];
            eh_mech_fwd<PROG>(MECH, net.n_out, NO > 1, a.prog, par, frc, tape, y0, yx);
            float dy = 0.0f, dyx[2] = {0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < NTG; ++t)
                if (t < net.T) {
                    const int oi = NO > 1 ? (int)((net.targ_out >> (2 * t)) & 3u) : 0;
                    const float y = oi == 0 ? y0 : (oi == 1 ? yx[0] : yx[1]);
                    yh[t][e] = y;
                    const float r = __builtin_isnan(yv[t][e]) ? 0.0f : y - yv[t][e];
                    float d;
                    if (mae) { S[t] += fabsf(r); d = r > 0.0f ? w[t] : (r < 0.0f ? -w[t] : 0.0f); }      // mean |r| (loss_fn.jl:64-66)
                    else { S[t] = fmaf(r, r, S[t]); d = 2.0f * w[t] * r; }                              // mean r^2 (loss_fn.jl:61-63)
                    dy += oi == 0 ? d : 0.0f; dyx[0] += oi == 1 ? d : 0.0f; dyx[1] += oi == 2 ? d : 0.0f;
                }
            float dp[EH_MAX_PARAMS];                             // (a closure: the reverse sweep over the tape, what Zygote derives from it)
            eh_mech_rev<PROG>(net.n_out, NO > 1, a.prog, par, frc, tape, dy, dyx, dp);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                gp[j] += row[j] >= 0 ? 0.0f : dp[j];
                dov[j][e] = dp[j] * sg[j];
            }
        }
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (row[j] >= 0) st(a.d_o + (long long)row[j] * a.ld, dov[j]);
        if (a.yhat)
#pragma unroll
            for (int t = 0; t < NTG; ++t)
                if (t < net.T) st(a.yhat + (long long)t * a.ld, yh[t]);
    }
    __shared__ float sh[4][EH_MECH_PART];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float v = eh_wave_sum(k < 8 ? (k < NP ? gp[k < NP ? k : 0] : 0.0f) : (k - 8 < NTG ? S[k - 8 < NTG ? k - 8 : 0] : 0.0f));
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12) a.part[(long long)blockIdx.x * EH_MECH_PART + threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// rows of partials -> out[0] = loss, out[1 + j] = d loss / d raw global parameter j (canonical parameter order), fixed order:
// deterministic.  Up to 2 048 rows: eh_mech_finish_kernel alone (one workgroup, 64 row groups x 16 columns, all of a thread's loads
// -- rows written on other XCDs, each a trip to memory -- requested before the first add).  More rows: eh_mech_fold_kernel first,
// whose workgroup g folds rows [g rows_per, (g + 1) rows_per) into row g of a second, <= 64-row table for the finish kernel.  (One
// launch with a ticket for the last workgroup was measured and lost: 13.6 us at 4 096 rows, 37 us at 65 536 -- the release in front
// of the ticket writes back an L2 -- against 5.1-5.7 us for the plain one-workgroup kernel; profiles/r03/mech_stage_ab.txt.)
__device__ __forceinline__ float eh_mech_fold_rows(const float* part, int r0, int r1, float (*red)[EH_MECH_PART]) {
    const int k = threadIdx.x & 15, grp = threadIdx.x >> 4;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (int rb = r0 + grp; rb < r1; rb += 64 * 32) {
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = rb + 64 * u < r1 ? part[(long long)(rb + 64 * u) * EH_MECH_PART + k] : 0.0f;
#pragma unroll
        for (int u = 0; u < 32; u += 4) { s0 += v[u]; s1 += v[u + 1]; s2 += v[u + 2]; s3 += v[u + 3]; }
    }
    red[grp][k] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    float s = 0.0f;
    if (grp == 0)
        for (int g2 = 0; g2 < 64; ++g2) s += red[g2][k];
    return s;                                                    // (threads 0..15 hold column k's sum)
}
__global__ __launch_bounds__(1024) void eh_mech_fold_kernel(const float* part, int nblk, int rows_per, float* part2) {
    __shared__ float red[64][EH_MECH_PART];
    const int r0 = blockIdx.x * rows_per;
    const float s = eh_mech_fold_rows(part, r0, min(nblk, r0 + rows_per), red);
    if (threadIdx.x < EH_MECH_PART) part2[blockIdx.x * EH_MECH_PART + threadIdx.x] = s;
}
__global__ __launch_bounds__(1024) void eh_mech_finish_kernel(const float* part, int nblk, const EhNet net, const float* meta, const EhMechArgs a, float* out) {
    __shared__ float red[64][EH_MECH_PART];
    const int k = threadIdx.x & 15;
    const float s = eh_mech_fold_rows(part, 0, nblk, red);
    if (threadIdx.x >= EH_MECH_PART) return;
    __shared__ float St[EH_MAX_TARG];
    if (k >= 8 && k < 12) {
        const unsigned long long c = a.use_v ? a.counts_v[k - 8] : a.counts[k - 8];
        St[k - 8] = (k - 8 < net.T && c > 0) ? a.agg_a * s / (float)c : 0.0f;
    }
    else if (k < 8) out[1 + k] = (k < net.n_par && ((net.par_kind >> (2 * k)) & 3u) == EH_PAR_GLOBAL) ? s * meta[EH_IMG_DPHI + k] : 0.0f;
    EH_WAVE_SYNC();                                              // (the 16 threads left are lanes of one wave)
    if (k == 0) out[0] = (St[0] + St[1]) + (St[2] + St[3]);
}

extern "C" int32_t eh_mech_loss_vjp(eh_handle* h, int64_t count, int64_t ld, const float* o_dev, const float* const* forcings_dev, const float* const* targets_dev,
                         const int64_t* n_valid_in, float* d_o_dev, float* yhat_dev, float* loss, float* grad_global, int64_t* n_valid) {
    if (!h || !o_dev || !forcings_dev || !targets_dev || !d_o_dev) return EH_EINVAL;
    if (h->seq) return fail(h, EH_EUNSUPPORTED, "eh_mech_loss_vjp: not built for sequence models");
    const EhNet& net = h->net;
    if (net.K == 0) return fail(h, EH_EUNSUPPORTED, "eh_mech_loss_vjp: the model has no neural parameter (no NN outputs to differentiate by): eh_loss_and_grad / eh_train_step run it whole");
    if (net.loss != EH_LOSS_MSE && net.loss != EH_LOSS_MAE) return fail(h, EH_EUNSUPPORTED, "eh_mech_loss_vjp: training loss %d (built: mse, mae)", net.loss);
    if (count < 1 || ld < count) return fail(h, EH_EINVAL, "eh_mech_loss_vjp: count %lld, ld %lld", (long long)count, (long long)ld);
    for (int f = 0; f < net.F; ++f) if (!forcings_dev[f]) return fail(h, EH_EINVAL, "eh_mech_loss_vjp: forcing %d is null", f);
    for (int t = 0; t < net.T; ++t) if (!targets_dev[t]) return fail(h, EH_EINVAL, "eh_mech_loss_vjp: target %d is null", t);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    EhMechArgs a{};
    a.o = o_dev; a.d_o = d_o_dev; a.yhat = yhat_dev; a.n = count; a.ld = ld; a.meta = h->image + h->arch->phi_off;
    bool vec = count % 4 == 0 && ld % 4 == 0 && ((uintptr_t)o_dev | (uintptr_t)d_o_dev | (uintptr_t)yhat_dev) % 16 == 0;
    for (int f = 0; f < net.F; ++f) { a.frc[f] = forcings_dev[f]; vec = vec && (uintptr_t)forcings_dev[f] % 16 == 0; }
    for (int t = 0; t < net.T; ++t) { a.y[t] = targets_dev[t]; vec = vec && (uintptr_t)targets_dev[t] % 16 == 0; }
    if (net.mech == EH_MECH_PROGRAM) { vec = false; a.prog = h->prog; }        // the interpreter keeps its tape in scratch: one sample per lane
    const int per = vec ? 1024 : 256;                                      // samples per workgroup and tile
    if (net.n_out == 1 && net.T > 1) return fail(h, EH_EUNSUPPORTED, "eh_mech_loss_vjp: %d targets on a single-output model", net.T);
    // Many short workgroups, each on its own consecutive tiles: the accesses then move through the arrays as one front, in dispatch
    // order, which is what the memory system serves best (tools/ubench/stream31.hip: 5.8 TB/s for this 3 : 1 mix, against 4.8-5.3 for
    // a persistent grid of 1-4 k workgroups striding through it).  Rows of partials: one per workgroup, <= EH_MECH_MAXROWS.
    const long long ntile = (count + per - 1) / per;
    // (default: two tiles per workgroup; models with several outputs -- twice the streams, more registers per lane, fewer resident waves --
    //  eight: FluxPart 0.59 -> 0.63 of the roof per call, RbQ10 best at two, Expo2Pool indifferent; tools/bench_mech.py --tiles)
    int tiles = h->mech_tiles > 0 ? h->mech_tiles : (net.n_out > 1 ? 8 : 2);
    while ((ntile + tiles - 1) / tiles > EH_MECH_MAXROWS) tiles *= 2;
    int nblk = (int)((ntile + tiles - 1) / tiles);
    if (h->mech_blocks > 0 && nblk > h->mech_blocks) { nblk = h->mech_blocks; tiles = 0; }      // "mech_blocks" option: a capped, grid-striding launch
    a.tiles = tiles;
    a.agg_a = h->img.agg_a;
    const int nfold = nblk <= 2048 ? 0 : std::min(64, (nblk + 511) / 512);      // workgroups of the fold kernel (512 rows and more each)
    const int rows_per = nfold ? (nblk + nfold - 1) / nfold : 0;
    const size_t ws_bytes = EH_MAX_TARG * sizeof(unsigned long long) + 64 + 64 + (size_t)(64 + EH_MECH_MAXROWS) * EH_MECH_PART * sizeof(float);
    if (ws_bytes > h->mech_ws_bytes) { if (int rc = eh_grow(h, &h->mech_ws, &h->mech_ws_bytes, ws_bytes)) return rc; }
    // [counts (4 x u64) | out: loss + 8 gradients, padded to 32 floats | part2 [64][16] | part [rows][16]]
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(h->mech_ws);
    float* out = reinterpret_cast<float*>(h->mech_ws + EH_MAX_TARG * sizeof(unsigned long long));
    float* part2 = out + 32;
    a.part = part2 + 64 * EH_MECH_PART;
    a.counts = counts;
    unsigned long long hc[EH_MAX_TARG] = {0, 0, 0, 0};
    if (n_valid_in) {                        // masks are a property of the data set (src/training/train.jl:221-232): the caller may know the counts
        for (int t = 0; t < net.T; ++t) { if (n_valid_in[t] < 0 || n_valid_in[t] > count) return fail(h, EH_EINVAL, "eh_mech_loss_vjp: n_valid_in[%d] = %lld", t, (long long)n_valid_in[t]); hc[t] = (unsigned long long)n_valid_in[t]; }
        for (int t = 0; t < EH_MAX_TARG; ++t) a.counts_v[t] = hc[t];
        a.use_v = 1;                                             // travels in the kernarg segment: no copy, no counting pass
    } else {
        HIPCHK(h, hipMemsetAsync(counts, 0, sizeof hc, h->stream));
        const unsigned ncb = (unsigned)std::min(nblk, 512);      // (one atomic per workgroup and target on ONE address: they serialise, ~13 ns each)
        if (vec) hipLaunchKernelGGL(eh_count_valid_kernel<4>, dim3(ncb), dim3(256), 0, h->stream, a, net.T, counts);
        else hipLaunchKernelGGL(eh_count_valid_kernel<1>, dim3(ncb), dim3(256), 0, h->stream, a, net.T, counts);
        HIPCHK(h, hipGetLastError());
    }
#define EH_MECH_GO(M)                                                                                                              \
    case M:                                                                                                                      \
        if (vec) hipLaunchKernelGGL((eh_mech_vjp_kernel<4, M>), dim3((unsigned)nblk), dim3(256), 0, h->stream, net, a);           \
        else hipLaunchKernelGGL((eh_mech_vjp_kernel<1, M>), dim3((unsigned)nblk), dim3(256), 0, h->stream, net, a);               \
        break;
    switch (net.mech) {
        EH_MECH_GO(EH_MECH_RBQ10) EH_MECH_GO(EH_MECH_EXPO) EH_MECH_GO(EH_MECH_LINEAR) EH_MECH_GO(EH_MECH_EXPO2POOL)
        EH_MECH_GO(EH_MECH_RS_COMPONENTS) EH_MECH_GO(EH_MECH_RS_COMPONENTS3F) EH_MECH_GO(EH_MECH_FLUXPART)
        case EH_MECH_PROGRAM: hipLaunchKernelGGL((eh_mech_vjp_kernel<1, EH_MECH_PROGRAM>), dim3((unsigned)nblk), dim3(256), 0, h->stream, net, a); break;
        default: return fail(h, EH_EUNSUPPORTED, "eh_mech_loss_vjp: mechanistic model %d", net.mech);
    }
#undef EH_MECH_GO
    HIPCHK(h, hipGetLastError());
    if (nfold) {
        hipLaunchKernelGGL(eh_mech_fold_kernel, dim3((unsigned)nfold), dim3(1024), 0, h->stream, a.part, nblk, rows_per, part2);
        HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(eh_mech_finish_kernel, dim3(1), dim3(1024), 0, h->stream, nfold ? part2 : a.part, nfold ? nfold : nblk, net, a.meta, a, out);
    HIPCHK(h, hipGetLastError());
    if (!loss && !grad_global && !n_valid) return EH_OK;         // asynchronous use: results stay on the device, ordered on the handle's stream
    float ho[9];
    HIPCHK(h, hipMemcpyAsync(ho, out, sizeof ho, hipMemcpyDeviceToHost, h->stream));
    if (!a.use_v) HIPCHK(h, hipMemcpyAsync(hc, counts, sizeof hc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    long long nv = 0;
    for (int t = 0; t < net.T; ++t) nv += (long long)hc[t];
    if (n_valid) *n_valid = nv;
    if (loss) *loss = nv > 0 ? ho[0] : __builtin_nanf("");      // all-masked batch: skipped (epoch.jl:17-19)
    if (grad_global)
        for (int j = 0; j < h->desc.n_params; ++j)
            if (h->desc.param_kind[j] == EH_PAR_GLOBAL) grad_global[h->desc.param_index[j]] = ho[1 + j];
    return EH_OK;
}
