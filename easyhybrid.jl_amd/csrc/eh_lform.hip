// The layer-wise execution form (eh_lform.hpp) as a translation unit of its own: workspace, the product dispatcher, forward, the training
// step and the evaluation pass, and the only instantiation of the form's kernels.  eh_api.hip enters through eh_lform_train and
// eh_lform_eval; the per-target weights, the moment coefficients and input BatchNorm come from its launchers (eh_internal.hpp).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#define EH_LFORM_KERNELS
#include "eh_lform.hpp"
#include "eh_bnl.hpp"
#include "eh_lnl.hpp"

struct EhLWs { float *Xb, *H[EH_MAX_NETS][EH_MAX_HIDDEN], *Z[EH_MAX_NETS][EH_MAX_HIDDEN], *R[EH_MAX_HIDDEN], *D[2], *O, *part; long long ldo; };      // (R[l]: a LayerNorm layer's rstd, one per sample)
static long long lform_floats_per_sample(const eh_handle* h) {
    long long w = h->net.P + 16, maxw = 0;
    for (int k = 0; k < h->plan.l_nnets; ++k)
        for (int l = 0; l + 1 < h->plan.l_net[k].nl; ++l) {
            w += h->plan.l_net[k].out[l] * ((h->plan.l_net[k].lact[l] == EH_ACT_SWISH || eh_is_norm(h->plan.l_net[k].kind[l])) ? 2 : 1);      // swish keeps the pre-activation too, a BatchNorm / LayerNorm layer its normalised input
            w += eh_is_layernorm(h->plan.l_net[k].kind[l]) ? 1 : 0;      // ... a LayerNorm layer its rows' rstd
            maxw = std::max<long long>(maxw, h->plan.l_net[k].out[l]);
        }
    return w + 2 * maxw;
}
// an allocation would be needed while a graph is being recorded: drop the recording (the engine stays usable) and say what to do
static int lform_alloc_in_capture(eh_handle* h, const char* what) {
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(h->stream, &g);
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    h->capturing = false;
    return fail(h, EH_ESTATE, "%s: the layer-wise form sizes this buffer at the first step that needs it -- run one step of this batch size (and training loss) "
                              "before eh_graph_begin, then record; the recording was dropped", what);
}
static int lform_workspace(eh_handle* h, long long count, EhLWs* W) {
    const long long cap_need = (count + 127) / 128 * 128;
    if (cap_need > h->l_cap) {
        if (h->capturing) return lform_alloc_in_capture(h, "workspace");
        HIPCHK(h, hipStreamSynchronize(h->stream));
        (void)hipFree(h->l_ws);
        h->l_ws = nullptr; h->l_cap = 0;
        HIPCHK(h, hipMalloc(&h->l_ws, ((size_t)cap_need * lform_floats_per_sample(h) + (size_t)4096 * EH_EVAL_STATS * EH_MAX_TARG) * sizeof(float)));
        h->l_cap = cap_need;
    }
    const long long cap = h->l_cap;
    float* p = h->l_ws;
    long long maxw = 0;
    W->Xb = p; p += cap * h->net.P;
    for (int k = 0; k < h->plan.l_nnets; ++k)
        for (int l = 0; l + 1 < h->plan.l_net[k].nl; ++l) {
            const long long o = h->plan.l_net[k].out[l];
            maxw = std::max(maxw, o);
            W->H[k][l] = p; p += cap * o;
            W->Z[k][l] = nullptr;
            if (h->plan.l_net[k].lact[l] == EH_ACT_SWISH || eh_is_norm(h->plan.l_net[k].kind[l])) { W->Z[k][l] = p; p += cap * o; }
            if (k == 0) { W->R[l] = nullptr; if (eh_is_layernorm(h->plan.l_net[k].kind[l])) { W->R[l] = p; p += cap; } }      // (cap is a multiple of 128: what follows stays 16-byte aligned)
        }
    W->D[0] = p; p += cap * maxw;
    W->D[1] = p; p += cap * maxw;
    W->O = p; p += cap * 16; W->ldo = cap;
    W->part = p;
    return EH_OK;
}
static const bool g_gemm_novec = getenv("EH_GEMM_NOVEC") != nullptr;      // (A/B switch of the measurement tools)
// a weight gradient (A transposed, plain store) with a thin side runs as a streaming kernel (eh_thin_gemm_kernel): its arguments
static bool lform_thin_args(const EhGemmArgs& g, bool btr, EhThinArgs* out) {
    if (g_gemm_novec || !(g.M <= 8 || g.N <= 8) || (g.M <= 8 ? btr : !btr)) return false;
    EhThinArgs t{};
    t.K = g.K; t.kchunk = g.kchunk; t.C = g.C; t.c_z = g.c_zstride; t.cs_z = g.c_zstride;
    if (g.M <= 8) {          // few inputs: wide = B (dZ [B x out]), thin = A (the layer's input [B x in])
        t.wide = g.B; t.ldw = g.ldb; t.ncols = g.N; t.thin = g.A; t.tsb = g.lda; t.tsj = 1; t.J = g.M; t.c_col = 1; t.c_j = g.ldc; t.cs_wide = g.colsum;
    } else {                 // few outputs, dO stored [K][ldo]: wide = A (the layer's input [B x in]), thin = B
        t.wide = g.A; t.ldw = g.lda; t.ncols = g.M; t.thin = g.B; t.tsb = 1; t.tsj = g.ldb; t.J = g.N; t.c_col = g.ldc; t.c_j = 1; t.cs_thin = g.colsum;
    }
    *out = t;
    return true;
}
template <bool ATR, bool BTR, int EPI>
static void lform_gemm(eh_handle* h, const EhGemmArgs& g, int nz) {
    const bool novec = g_gemm_novec;
    if constexpr (EPI == EH_GEPI_STORE && ATR) {
        EhThinArgs t;
        if (lform_thin_args(g, BTR, &t)) {
            hipLaunchKernelGGL(eh_thin_gemm_kernel, dim3((unsigned)((t.ncols + 63) / 64), (unsigned)nz), dim3(256), 0, h->stream, t);
            return;
        }
    }
    if (!novec && nz == 1 && g.kchunk >= g.K) {          // products with a degenerate dimension: streaming kernels (eh_lform.hpp)
        const long long tot = (long long)g.M * g.N;
        const unsigned sg = (unsigned)std::max<long long>(1, std::min<long long>(2048, (tot + 255) / 256));
        if (EPI == EH_GEPI_BIAS_ACT && !ATR && !BTR && g.K <= 8) { hipLaunchKernelGGL(eh_thin_fwd_k_kernel, dim3(sg), dim3(256), 0, h->stream, g); return; }
        if (EPI == EH_GEPI_BIAS_T && !ATR && !BTR && g.N <= 16 && g.M <= 16384) {
            hipLaunchKernelGGL(eh_thin_fwd_n_kernel, dim3((unsigned)std::max(1, std::min(1024, (g.M + 3) / 4))), dim3(256), 0, h->stream, g);
            return;
        }
        if (EPI == EH_GEPI_DACT && ATR && BTR && g.K <= 16) { hipLaunchKernelGGL(eh_thin_dact_kernel, dim3(sg), dim3(256), 0, h->stream, g); return; }
    }
    if constexpr (EPI == EH_GEPI_BIAS_ACT || EPI == EH_GEPI_DACT) {
        // few rows, deep k: split-K into partial products + a combine pass (eh_splitk_combine_kernel)
        static const bool nosplit = getenv("EH_GEMM_NOSPLIT") != nullptr;
        static const bool nofew = getenv("EH_GEMM_NOFEWROWS") != nullptr;
        static const int fewmax = getenv("EH_GEMM_FEWROWS_MAX") ? atoi(getenv("EH_GEMM_FEWROWS_MAX")) : 1024;
        if constexpr (!ATR) {
            // ... or, without the combine pass, one 16 x 16 tile per workgroup with the k range split over its waves (eh_fewrows_gemm_kernel)
            if (!novec && !nofew && nz == 1 && g.M <= fewmax && g.K >= 64 && g.kchunk >= g.K && eh_gemm_vec_ok(g, ATR, BTR)) {
                EhGemmArgs p = g;
                p.kchunk = std::max(16, ((g.K + 15) / 16 + 15) / 16 * 16);         // <= 16 slices of whole 16-deep groups
                const int nw = (g.K + p.kchunk - 1) / p.kchunk;
                static const int few32 = getenv("EH_GEMM_FEW32_MIN") ? atoi(getenv("EH_GEMM_FEW32_MIN")) : 512;       // rows from which the 32 x 32 tile runs
                if (g.M >= few32) hipLaunchKernelGGL((eh_fewrows32_gemm_kernel<BTR, EPI>), dim3((unsigned)((g.N + 31) / 32), (unsigned)((g.M + 31) / 32)), dim3(64u * (unsigned)nw), 0, h->stream, p);
                else {
                    hipLaunchKernelGGL((eh_fewrows_gemm_kernel<BTR, EPI>), dim3((unsigned)((g.N + 15) / 16), (unsigned)((g.M + 15) / 16)), dim3(64u * (unsigned)nw), 0, h->stream, p);
                    if (p.job_part) h->l_job_done = true;      // (the one product kernel that takes the side job, EhGemmArgs::job_part)
                }
                return;
            }
        }
        if (!novec && !nosplit && nz == 1 && g.M <= 256 && g.K >= 128 && g.kchunk >= g.K && eh_gemm_vec_ok(g, ATR, BTR)) {
            int kc = std::max(32, ((g.K + 15) / 16 + 15) / 16 * 16);          // ~16 parts, whole 16-deep steps
            const int ns = (g.K + kc - 1) / kc;
            const size_t need = (size_t)ns * g.M * g.N;
            if (ns > 1) {
                if (need > h->l_split_cap && !h->capturing) {      // (while a graph is being recorded: no allocation -- the tiled kernel below runs instead)
                    if (hipStreamSynchronize(h->stream) == hipSuccess) { (void)hipFree(h->l_split); h->l_split = nullptr; h->l_split_cap = 0; }
                    if (hipMalloc(&h->l_split, need * sizeof(float)) == hipSuccess) h->l_split_cap = need; else (void)hipGetLastError();
                }
                if (need <= h->l_split_cap) {
                    EhGemmArgs p = g;
                    p.C = h->l_split; p.ldc = g.N; p.c_zstride = (long long)g.M * g.N; p.kchunk = kc; p.colsum = nullptr; p.bias = nullptr; p.H = nullptr; p.Z = nullptr;
                    const dim3 g64((unsigned)((g.N + 63) / 64), (unsigned)((g.M + 63) / 64), (unsigned)ns);
                    hipLaunchKernelGGL((eh_gemm_kernel<ATR, BTR, EH_GEPI_STORE, true, 64>), g64, dim3(256), 0, h->stream, p);
                    const long long tot = (long long)g.M * g.N;
                    hipLaunchKernelGGL(eh_splitk_combine_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>(1024, (tot + 255) / 256))), dim3(256), 0, h->stream,
                                       h->l_split, ns, (int)EPI, g);
                    return;
                }
            }
        }
    }
    const dim3 grid((unsigned)((g.N + 127) / 128), (unsigned)((g.M + 127) / 128), (unsigned)nz);
    const bool vec = !novec && eh_gemm_vec_ok(g, ATR, BTR);
    static const long long t128_min = getenv("EH_GEMM_T128_MIN") ? atoll(getenv("EH_GEMM_T128_MIN")) : 2048;
    if (vec && (long long)grid.x * grid.y * grid.z < t128_min) {      // fewer 128 x 128 tiles than CUs: 64 x 64 ones (four times the workgroups, a quarter of the work each)
        const dim3 grid64((unsigned)((g.N + 63) / 64), (unsigned)((g.M + 63) / 64), (unsigned)nz);
        hipLaunchKernelGGL((eh_gemm_kernel<ATR, BTR, EPI, true, 64>), grid64, dim3(256), 0, h->stream, g);
        return;
    }
    if (vec) hipLaunchKernelGGL((eh_gemm_kernel<ATR, BTR, EPI, true>), grid, dim3(256), 0, h->stream, g);
    else hipLaunchKernelGGL((eh_gemm_kernel<ATR, BTR, EPI, false>), grid, dim3(256), 0, h->stream, g);
}
// BatchNorm layer l of the one network (eh_bnl.hpp): H_l = act(scale xh + bias), xh from the statistics of this minibatch (train mode; kept in
// Z_l for the backward; `update`: the running statistics move on) or from the running ones (test mode, nothing kept)
static bool bnl_vec_ok(int n, std::initializer_list<const void*> ps) {
    if (n % 4) return false;
    for (const void* p : ps) if (reinterpret_cast<unsigned long long>(p) & 15ull) return false;
    return true;
}
static int bnl_chunks(int B, int* chunk) {
    const int nchunk = std::max(1, std::min<int>(EH_BNL_CHUNKS, (B + EH_BNL_CHUNK_ROWS - 1) / EH_BNL_CHUNK_ROWS));
    *chunk = (B + nchunk - 1) / nchunk;
    return (B + *chunk - 1) / *chunk;
}
static unsigned bnl_ew_grid(long long tot, bool vec) { return (unsigned)std::max<long long>(1, std::min<long long>(4096, ((vec ? tot / 4 : tot) + 255) / 256)); }
static int bnl_forward_layer(eh_handle* h, int l, int B, bool train_mode, bool update, const EhLWs& W) {
    const EhLNet& L = h->plan.l_net[0];
    const int n = L.out[l];
    const float* theta = TH(h);
    const float* gamma = eh_affine(L.kind[l]) ? theta + L.woff[l] : nullptr;
    const float* beta = eh_affine(L.kind[l]) ? theta + L.boff[l] : nullptr;
    const float* X = W.H[0][l - 1];
    float* stat = h->bnl_stat + 2 * h->plan.bnl_off[l];      // [c | d | rstd]
    float* run = h->bnl_run + h->plan.bnl_off[l];
    if (train_mode) {
        EhBnlArgs a{};
        a.X = X; a.part = h->bnl_part; a.B = B; a.n = n; a.act = L.lact[l];
        const int nchunk = bnl_chunks(B, &a.chunk);
        hipLaunchKernelGGL((eh_bnl_colsum_kernel<false>), dim3((unsigned)((n + 63) / 64), (unsigned)nchunk), dim3(256), 0, h->stream, a);
        hipLaunchKernelGGL(eh_bnl_fold_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float*)h->bnl_part, nchunk, X, B, n, h->bnl_eps[l], h->bnl_mom[l], stat, run, update ? 1 : 0);
    }
    EhBnlNormArgs na{};
    na.X = X; na.Y = W.H[0][l]; na.Xh = train_mode ? W.Z[0][l] : nullptr;
    na.mean = train_mode ? stat : run; na.d = train_mode ? stat + n : nullptr; na.second = train_mode ? stat + 2 * n : run + n; na.from_var = train_mode ? 0 : 1;
    na.gamma = gamma; na.beta = beta; na.tot = (long long)B * n; na.n = n; na.act = L.lact[l]; na.eps = h->bnl_eps[l];
    na.vec = bnl_vec_ok(n, {na.X, na.Y, na.Xh}) ? 1 : 0;
    hipLaunchKernelGGL(eh_bnl_norm_kernel, dim3(bnl_ew_grid(na.tot, na.vec != 0)), dim3(256), 0, h->stream, na);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}
// ... its backward: dY [B x n] -> d scale / d bias into the slab (row 0; zeros in the other rows), dZ of the layer below into dX
static int bnl_backward_layer(eh_handle* h, int l, int B, const float* dY, float* dX, int rows, const EhLWs& W) {
    const EhLNet& L = h->plan.l_net[0];
    const int n = L.out[l];
    const float* theta = TH(h);
    const bool affine = eh_affine(L.kind[l]);
    EhBnlArgs a{};
    a.X = dY; a.Xh = W.Z[0][l]; a.Y = W.H[0][l]; a.gamma = affine ? theta + L.woff[l] : nullptr; a.beta = affine ? theta + L.boff[l] : nullptr;
    a.part = h->bnl_part; a.B = B; a.n = n; a.act = L.lact[l];
    const int nchunk = bnl_chunks(B, &a.chunk);
    float* sums = h->bnl_part + (size_t)EH_BNL_CHUNKS * 2 * h->plan.norm_maxn;
    hipLaunchKernelGGL((eh_bnl_colsum_kernel<true>), dim3((unsigned)((n + 63) / 64), (unsigned)nchunk), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(eh_bnl_fold_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float*)h->bnl_part, nchunk, n, sums,
                       affine ? h->slab + L.woff[l] : nullptr, affine ? h->slab + L.boff[l] : nullptr, rows, (long long)h->n_acc);
    EhBnlDxArgs d{};
    d.dY = dY; d.Xh = a.Xh; d.Y = a.Y; d.gamma = a.gamma; d.beta = a.beta; d.rstd = h->bnl_stat + 2 * h->plan.bnl_off[l] + 2 * n; d.sums = sums;
    // (the layer below: a Dense layer's act' from its output -- swish: its pre-activation --; a BatchNorm layer takes its own in its own backward)
    d.act_below = eh_is_norm(L.kind[l - 1]) ? (int)EH_ACT_IDENTITY : L.lact[l - 1];
    d.Hb = (d.act_below == EH_ACT_SWISH) ? W.Z[0][l - 1] : W.H[0][l - 1];
    d.dX = dX; d.tot = (long long)B * n; d.n = n; d.act = L.lact[l]; d.inv_b = 1.0f / (float)B;
    d.vec = bnl_vec_ok(n, {d.dY, d.Xh, d.Y, d.Hb, d.dX}) ? 1 : 0;
    hipLaunchKernelGGL(eh_bnl_dx_kernel, dim3(bnl_ew_grid(d.tot, d.vec != 0)), dim3(256), 0, h->stream, d);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}
// LayerNorm layer l of the one network (eh_lnl.hpp): H_l = act(scale xh + bias), every row normalised over its own features; `keep`: xh into Z_l
// and rstd into R_l for the backward (training), otherwise the same pass with nothing kept
static void lnl_geometry(int n, int B, int* seg, int* per, unsigned* grid) {
    int s = 1;
    while (s < n && s < 64) s *= 2;
    int p = 1;
    while ((long long)s * p < n) p *= 2;      // (n <= EH_MAX_LAYERNORM_WIDTH, eh_create: p <= 16)
    *seg = s; *per = p;
    const long long rows_wg = 4ll * (64 / s);
    *grid = (unsigned)((B + rows_wg - 1) / rows_wg);
}
static int lnl_forward_layer(eh_handle* h, int l, int B, bool keep, const EhLWs& W) {
    const EhLNet& L = h->plan.l_net[0];
    const float* theta = TH(h);
    EhLnlFwdArgs a{};
    a.X = W.H[0][l - 1]; a.Y = W.H[0][l]; a.Xh = keep ? W.Z[0][l] : nullptr; a.rstd = keep ? W.R[l] : nullptr;
    a.scale = eh_affine(L.kind[l]) ? theta + L.woff[l] : nullptr; a.bias = eh_affine(L.kind[l]) ? theta + L.boff[l] : nullptr;
    a.B = B; a.n = L.out[l]; a.act = L.lact[l]; a.eps = h->bnl_eps[l];
    int per; unsigned grid;
    lnl_geometry(a.n, B, &a.seg, &per, &grid);
    switch (per) {
        case 1: hipLaunchKernelGGL((eh_lnl_fwd_kernel<1>), dim3(grid), dim3(256), 0, h->stream, a); break;
        case 2: hipLaunchKernelGGL((eh_lnl_fwd_kernel<2>), dim3(grid), dim3(256), 0, h->stream, a); break;
        case 4: hipLaunchKernelGGL((eh_lnl_fwd_kernel<4>), dim3(grid), dim3(256), 0, h->stream, a); break;
        case 8: hipLaunchKernelGGL((eh_lnl_fwd_kernel<8>), dim3(grid), dim3(256), 0, h->stream, a); break;
        case 16: hipLaunchKernelGGL((eh_lnl_fwd_kernel<16>), dim3(grid), dim3(256), 0, h->stream, a); break;
        default: return fail(h, EH_EUNSUPPORTED, "layer-wise form: no kernel for a LayerNorm layer of width %d", a.n);
    }
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}
// ... its backward: dY [B x n] -> dZ of the layer below into dX (one launch); affine: d scale / d bias as column sums over the rows, by the
// BatchNorm layers' two kernels, into the slab (row 0; zeros in the other rows)
static int lnl_backward_layer(eh_handle* h, int l, int B, const float* dY, float* dX, int rows, const EhLWs& W) {
    const EhLNet& L = h->plan.l_net[0];
    const int n = L.out[l];
    const float* theta = TH(h);
    const bool affine = eh_affine(L.kind[l]);
    EhLnlBwdArgs d{};
    d.dY = dY; d.Xh = W.Z[0][l]; d.Y = W.H[0][l]; d.rstd = W.R[l];
    d.scale = affine ? theta + L.woff[l] : nullptr; d.bias = affine ? theta + L.boff[l] : nullptr;
    d.act_below = eh_is_norm(L.kind[l - 1]) ? (int)EH_ACT_IDENTITY : L.lact[l - 1];
    d.Hb = (d.act_below == EH_ACT_SWISH) ? W.Z[0][l - 1] : W.H[0][l - 1];
    d.dX = dX; d.B = B; d.n = n; d.act = L.lact[l];
    int per; unsigned grid;
    lnl_geometry(n, B, &d.seg, &per, &grid);
    switch (per) {
        case 1: hipLaunchKernelGGL((eh_lnl_bwd_kernel<1>), dim3(grid), dim3(256), 0, h->stream, d); break;
        case 2: hipLaunchKernelGGL((eh_lnl_bwd_kernel<2>), dim3(grid), dim3(256), 0, h->stream, d); break;
        case 4: hipLaunchKernelGGL((eh_lnl_bwd_kernel<4>), dim3(grid), dim3(256), 0, h->stream, d); break;
        case 8: hipLaunchKernelGGL((eh_lnl_bwd_kernel<8>), dim3(grid), dim3(256), 0, h->stream, d); break;
        case 16: hipLaunchKernelGGL((eh_lnl_bwd_kernel<16>), dim3(grid), dim3(256), 0, h->stream, d); break;
        default: return fail(h, EH_EUNSUPPORTED, "layer-wise form: no kernel for a LayerNorm layer of width %d", n);
    }
    if (affine) {
        EhBnlArgs a{};
        a.X = dY; a.Xh = d.Xh; a.Y = d.Y; a.gamma = d.scale; a.beta = d.bias; a.part = h->bnl_part; a.B = B; a.n = n; a.act = L.lact[l];
        const int nchunk = bnl_chunks(B, &a.chunk);
        float* sums = h->bnl_part + (size_t)EH_BNL_CHUNKS * 2 * h->plan.norm_maxn;      // (the totals: nothing reads them here, the leaves' gradients are all of them)
        hipLaunchKernelGGL((eh_bnl_colsum_kernel<true>), dim3((unsigned)((n + 63) / 64), (unsigned)nchunk), dim3(256), 0, h->stream, a);
        hipLaunchKernelGGL(eh_bnl_fold_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float*)h->bnl_part, nchunk, n, sums,
                           h->slab + L.woff[l], h->slab + L.boff[l], rows, (long long)h->n_acc);
    }
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}
// minibatch -> Xb (input BatchNorm applied), forward through every Dense layer; O^T [K][ldo] = the raw NN outputs
// (lstop >= 0: a one-network model, only its layers below `lstop` run here -- the rest belongs to eh_lform_tailchain_kernel)
static int lform_forward(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, bool train_mode, bool bn_update, const EhLWs& W, int lstop = -1) {
    const EhNet& net = h->net;
    const int B = (int)count;
    if (h->plan.l_nnets == 0) return EH_OK;        // no network (no neural parameter): the mechanistic stage reads the records itself
    EhStepArgs bn{};
    // (small minibatches: the prep kernel takes the batch statistics itself -- one dependent launch fewer)
    static const bool nofuse_env = getenv("EH_LFORM_NOFUSE") != nullptr;
    const bool nofuse = nofuse_env || h->bnl || h->lnl;      // (BatchNorm / LayerNorm layers in the chain: the plain loop below, one launch per layer and pass)
    const bool bn_self = train_mode && h->bn_on && !h->bn_ext && count > 0 && count <= 256 && !nofuse;
    if (train_mode && !bn_self) { if (int rc = eh_bn_prepare(h, sp, idx, first, count, bn_update, &bn)) return rc; }
    EhLPrepArgs pa{};
    pa.recs = sp.recs; pa.C = h->plan.C; pa.P = net.P; pa.idx = idx; pa.first = first; pa.count = B; pa.Xb = W.Xb; pa.meta = h->image;
    pa.bn_part = bn.bn_part; pa.bn_nblk = bn.bn_nblk; pa.bn_c = bn.bn_c; pa.bn_n = bn.bn_n; pa.bn_update = bn.bn_update; pa.bn_run = h->bn_run;
    if (bn_self) { pa.bn_self = 1; pa.bn_update = bn_update ? 1 : 0; }
    static const bool stamp_first = getenv("EH_STAMP_FIRST") != nullptr;      // (diagnostic builds: the stamps of the first launch instead of the chain kernel's)
    pa.stamps = stamp_first ? h->stamps : nullptr;
    const long long tot = (long long)B * net.P;
    const float* theta = TH(h);
    // Few rows: minibatch matrix + BatchNorm + first layer + the SECOND layer's few-rows product as one launch (eh_fewrows_first_kernel) where
    // the second layer is a hidden layer that would run eh_fewrows_gemm_kernel anyway
    bool fused01 = false;
    {
        static const bool nofirst = getenv("EH_LFORM_NOFIRST") != nullptr;
        static const bool nofew = getenv("EH_GEMM_NOFEWROWS") != nullptr;
        static const int first_maxb = getenv("EH_LFORM_FIRST_MAXB") ? atoi(getenv("EH_LFORM_FIRST_MAXB")) : 64;   // every workgroup takes the statistics itself: a loss from ~128 rows up
        const EhLNet& L0 = h->plan.l_net[0];
        const int stop = lstop >= 0 ? lstop : L0.nl;
        auto al16 = [](const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; };
        if (!nofirst && !nofuse && !nofew && !g_gemm_novec && L0.nl >= 3 && stop >= 2 && L0.in[0] <= 4 && B >= 1 && B <= first_maxb &&
            L0.out[0] >= 64 && (L0.out[0] % 16) == 0 && (L0.out[1] % 4) == 0 &&
            al16(theta + L0.woff[0]) && al16(theta + L0.boff[0]) && al16(theta + L0.woff[1])) {
            EhGemmArgs f{};
            f.lda = net.P; f.B = theta + L0.woff[0]; f.ldb = L0.out[0]; f.M = B; f.N = L0.out[0]; f.K = L0.in[0]; f.kchunk = f.K;
            f.bias = theta + L0.boff[0]; f.act = L0.lact[0]; f.C = W.H[0][0]; f.ldc = L0.out[0]; f.Z = W.Z[0][0];
            EhGemmArgs g{};
            g.A = nullptr; g.lda = L0.in[1]; g.B = theta + L0.woff[1]; g.ldb = L0.out[1];
            g.M = B; g.N = L0.out[1]; g.K = L0.in[1]; g.c_zstride = 0;
            g.bias = theta + L0.boff[1]; g.act = L0.lact[1]; g.C = W.H[0][1]; g.ldc = L0.out[1]; g.Z = W.Z[0][1];
            g.kchunk = std::max(16, ((g.K + 15) / 16 + 15) / 16 * 16);         // <= 16 slices of whole 16-deep groups (lform_gemm's few-rows rule)
            const int nwv = (g.K + g.kchunk - 1) / g.kchunk;
            if (f.K <= 2) hipLaunchKernelGGL((eh_fewrows_first_kernel<EH_GEPI_BIAS_ACT, 2>), dim3((unsigned)((g.N + 15) / 16), (unsigned)((g.M + 15) / 16)), dim3(64u * (unsigned)nwv), 0, h->stream, pa, f, g, L0.c0);
            else hipLaunchKernelGGL((eh_fewrows_first_kernel<EH_GEPI_BIAS_ACT, 4>), dim3((unsigned)((g.N + 15) / 16), (unsigned)((g.M + 15) / 16)), dim3(64u * (unsigned)nwv), 0, h->stream, pa, f, g, L0.c0);
            HIPCHK(h, hipGetLastError());
            fused01 = true;
        }
    }
    // the first network's first layer rides along when it is one of the few-predictor products (K <= 8, hidden layer behind it)
    bool fused0 = false;
    if (!fused01) {
        const EhLNet& L0 = h->plan.l_net[0];
        if (!nofuse && !g_gemm_novec && L0.nl >= 2 && L0.in[0] <= 8 && lstop != 0) {
            EhGemmArgs g{};
            g.A = nullptr; g.lda = net.P; g.B = theta + L0.woff[0]; g.ldb = L0.out[0];
            g.M = B; g.N = L0.out[0]; g.K = L0.in[0]; g.kchunk = g.K; g.bias = theta + L0.boff[0]; g.act = L0.lact[0];
            g.C = W.H[0][0]; g.ldc = L0.out[0]; g.Z = W.Z[0][0];
            const long long totc = (long long)g.M * g.N;
            hipLaunchKernelGGL((eh_lform_prep_kernel<true>), dim3((unsigned)std::max<long long>(1, std::min<long long>(2048, (std::max(tot, totc) + 255) / 256))), dim3(256), 0, h->stream, pa, g, L0.c0);
            fused0 = true;
        }
    }
    if (!fused0 && !fused01) hipLaunchKernelGGL((eh_lform_prep_kernel<false>), dim3((unsigned)std::max<long long>(1, std::min<long long>(1024, (tot + 255) / 256))), dim3(256), 0, h->stream, pa, EhGemmArgs{}, 0);
    HIPCHK(h, hipGetLastError());
    for (int k = 0; k < h->plan.l_nnets; ++k) {
        const EhLNet& L = h->plan.l_net[k];
        for (int l = 0; l < (lstop >= 0 ? lstop : L.nl); ++l) {
            if ((fused0 || fused01) && k == 0 && l == 0) continue;
            if (fused01 && k == 0 && l == 1) continue;
            if (eh_is_layernorm(L.kind[l])) { if (int rc = lnl_forward_layer(h, l, B, train_mode, W)) return rc; continue; }
            if (eh_is_norm(L.kind[l])) { if (int rc = bnl_forward_layer(h, l, B, train_mode, bn_update, W)) return rc; continue; }
            EhGemmArgs g{};
            g.A = l == 0 ? W.Xb + L.c0 : W.H[k][l - 1]; g.lda = l == 0 ? net.P : L.in[l];      // (a network's predictors: its columns of the minibatch matrix)
            g.B = theta + L.woff[l]; g.ldb = L.out[l];                   // canonical (out, in) column-major == [in][out] row-major
            g.M = B; g.N = L.out[l]; g.K = L.in[l]; g.kchunk = g.K; g.c_zstride = 0;
            g.bias = theta + L.boff[l]; g.act = L.lact[l];
            if (l + 1 < L.nl) { g.C = W.H[k][l]; g.ldc = L.out[l]; g.Z = W.Z[k][l]; lform_gemm<false, false, EH_GEPI_BIAS_ACT>(h, g, 1); }
            else { g.C = W.O + (long long)L.orow * W.ldo; g.ldc = W.ldo; lform_gemm<false, false, EH_GEPI_BIAS_T>(h, g, 1); }
            HIPCHK(h, hipGetLastError());
        }
    }
    return EH_OK;
}
// one training step's gradient sums into `rows` partial slab rows (the contract of the fused step kernels: eh_reduce_kernel follows)
int eh_lform_train(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, int* rows_out, bool bn_update) {
    const EhNet& net = h->net;
    EhLWs W;
    if (int rc = lform_workspace(h, std::max<long long>(count, 1), &W)) return rc;
    const int B = (int)count;
    // slab rows = sample chunks the weight-gradient products are split over (their only source of parallelism beyond the tiles of the
    // weight matrix itself): >= EH_LFORM_CHUNK samples each, at most EH_LFORM_ROWS of them
    static const long long lchunk = getenv("EH_LFORM_CHUNK") ? std::max(64, atoi(getenv("EH_LFORM_CHUNK"))) : 128;
    const int rows = (int)std::max<long long>(1, std::min<long long>(EH_LFORM_ROWS, (count + lchunk - 1) / lchunk));
    const int chunk = std::max(16, (int)(((count + rows - 1) / rows + 15) / 16 * 16));
    *rows_out = rows;
    if (net.T > 1 && !h->dp_weights) {        // (data-parallel step: eh_dp_grad has just filled inv_n with the weights of the GLOBAL batch)
        if (int rc = eh_launch_count(h, sp, idx, first, count)) return rc;
    }
    if (count <= 0) {                          // nothing to do: an all-zero partial (the reduce kernel then skips the update)
        HIPCHK(h, hipMemsetAsync(h->slab, 0, (size_t)h->n_acc * sizeof(float), h->stream));
        return EH_OK;
    }
    const unsigned tpm = eh_two_pass_mask(h);
    // Small minibatches: every layer's delta is kept (l_dk), the chain of delta products runs first and the weight gradients -- a
    // handful of tiles each, 4-6 us per dependent launch -- follow as ONE grouped launch of the tiled ones and one of the thin ones.
    static const long long lgroup_max = getenv("EH_LFORM_GROUP_MAX") ? atoll(getenv("EH_LFORM_GROUP_MAX")) : 4096;
    bool grouped = count <= lgroup_max && h->plan.l_nnets > 0 && !h->bnl && !h->lnl;      // (the kept-deltas groups and the tail chain behind them hold Dense layers only)
    long long dk_floats = 0;
    // (sized by THIS minibatch, rounded up to a power of two -- not by the largest one the path serves: a B = 64 step of a deep, wide
    //  MultiNN model used to ask for up to the 1 GiB cap; advisor, round 3.  A larger batch later re-grows it, outside a capture.)
    long long dk_rows = 64;
    while (dk_rows < count) dk_rows *= 2;
    if (grouped) {
        for (int k = 0; k < h->plan.l_nnets; ++k)
            for (int l = 0; l + 1 < h->plan.l_net[k].nl; ++l) dk_floats += dk_rows * h->plan.l_net[k].out[l];
        if (dk_floats > (1ll << 28)) { grouped = false; h->jit_log = "layer-wise form: kept deltas of this minibatch exceed 1 GiB -- weight gradients run layer by layer (slower small-batch steps)"; }
        else if ((size_t)dk_floats > h->l_dk_cap) {
            if (h->capturing) return lform_alloc_in_capture(h, "kept deltas");
            HIPCHK(h, hipStreamSynchronize(h->stream));
            (void)hipFree(h->l_dk); h->l_dk = nullptr; h->l_dk_cap = 0;
            if (hipMalloc(&h->l_dk, (size_t)dk_floats * sizeof(float)) == hipSuccess) h->l_dk_cap = (size_t)dk_floats;
            else { (void)hipGetLastError(); grouped = false; h->jit_log = "layer-wise form: no memory for the kept deltas of the grouped small-batch path -- weight gradients run layer by layer (slower small-batch steps)"; }
        }
    }
    // Few rows, one network: the narrow end of the network -- every layer from `tail_s` on, the mechanistic stage and the deltas back
    // down to layer tail_s - 1 -- is ONE launch with a workgroup per row (eh_lform_tailchain_kernel, eh_lform.hpp)
    static const bool notail = getenv("EH_LFORM_NOTAIL") != nullptr;
    int tail_s = -1;
    // (a workgroup per ROW up to 256 rows: every CU streams the suffix's weights once whatever the number of rows -- 57.5 / 61.3 / 70.1 / 77.5 us
    //  per step at 96 / 128 / 192 / 256 rows against 70.9 / 74.2 / 80.1 / 86.6 with the products launched one by one.  With FOUR rows per
    //  workgroup, the form of the round's first half for more than 64 rows, it was slower than either: 75.5 / 78.6 / 90.2 / 96.7; those
    //  instantiations are gone.)
    if (!notail && grouped && h->plan.l_nnets == 1 && count <= 256 && !tpm && !g_gemm_novec) {
        const EhLNet& L = h->plan.l_net[0];
        long long wsum = 0;
        for (int l = L.nl - 1; l >= 0; --l) {
            if (L.in[l] > (int)EH_LTAIL_MAXW || L.out[l] > (int)EH_LTAIL_MAXW || wsum + (long long)L.in[l] * L.out[l] > (96ll << 10)) break;
            wsum += (long long)L.in[l] * L.out[l];
            tail_s = l;
        }
    }
    if (int rc = lform_forward(h, sp, idx, first, count, true, bn_update, W, tail_s)) return rc;
    // (diagnostic builds: EH_STAMP_DW / EH_STAMP_FIRST hand the stamps to the weight-gradient launch / the first launch instead of the chain kernel)
    static const bool stamp_dw = getenv("EH_STAMP_DW") != nullptr, stamp_first = getenv("EH_STAMP_FIRST") != nullptr;
    EhStepArgs a = eh_step_args(h, sp, idx, first, count);
    a.stamps = (stamp_dw || stamp_first) ? nullptr : h->stamps;
    if (tpm) {
        // losses that need batch statistics of yhat (see launch_train_kernel): the NN outputs O stay where the forward left them, so
        // the two statistics passes are two runs of the mechanistic stage alone (eval form), not two forwards
        EhStepArgs e = a;
        e.inv_n = nullptr; e.yld = count;
        const int egrid = (int)std::min<long long>(256, (count + 255) / 256);
        EhLMechArgs me{W.O, W.ldo, h->slab};                   // [egrid][EH_EVAL_STATS * T] (the slab is rewritten by the training pass afterwards)
        for (int pass = 0; pass < 2; ++pass) {
            if (net.mech == EH_MECH_PROGRAM) hipLaunchKernelGGL((eh_lform_mech_kernel<false, true>), dim3(egrid), dim3(256), 0, h->stream, net, e, me, h->image);
            else hipLaunchKernelGGL((eh_lform_mech_kernel<false, false>), dim3(egrid), dim3(256), 0, h->stream, net, e, me, h->image);
            HIPCHK(h, hipGetLastError());
            if (int rc = pass == 0 ? eh_launch_moment_centre(h, sp, h->slab, egrid) : eh_launch_moment_coef(h, sp, h->slab, egrid)) return rc;
            e.inv_n = h->inv_n;
        }
    }
    a.inv_n = (net.T > 1 || tpm) ? h->inv_n : nullptr;
    // recorded loss functions: no kernel is compiled at run time in this form -- the mechanistic kernel interprets their tapes
    bool lprog = false;
    for (int t = 0; t < net.T; ++t) lprog = lprog || ((net.loss_t >> (4 * t)) & 15u) == (unsigned)EH_LOSS_PROGRAM;
    if (lprog) {
        if (h->l_lprog_gen != h->loss_prog.gen) {
            if (h->capturing) return lform_alloc_in_capture(h, "recorded loss programs");
            std::vector<unsigned> img((size_t)EH_MAX_TARG * EH_LPROG_WORDS, 0u);
            for (int t = 0; t < net.T; ++t) {
                if (!h->loss_prog.has(t)) continue;
                const EhLossProg1& lp = h->loss_prog.of(t);
                unsigned* q = img.data() + (size_t)t * EH_LPROG_WORDS;
                q[0] = (unsigned)lp.code.size(); q[1] = 1u; q[2] = (unsigned)lp.out;
                for (size_t k = 0; k < lp.consts.size() && k < (size_t)EH_MAX_PROG_CONST; ++k) memcpy(&q[8 + k], &lp.consts[k], sizeof(float));
                for (size_t i = 0; i < lp.code.size() && i < (size_t)EH_MAX_PROG; ++i) q[24 + i] = lp.code[i];
            }
            if (!h->l_lprog) HIPCHK(h, hipMalloc(&h->l_lprog, img.size() * sizeof(unsigned)));
            HIPCHK(h, hipStreamSynchronize(h->stream));          // (steps in flight read the old programs)
            HIPCHK(h, hipMemcpy(h->l_lprog, img.data(), img.size() * sizeof(unsigned), hipMemcpyHostToDevice));
            h->l_lprog_gen = h->loss_prog.gen;
        }
        a.lprog = h->l_lprog;
    }
    EhLMechArgs m{W.O, W.ldo, W.part, nullptr, 0, 0};
    const int mgrid = (int)std::min<long long>(2048, (count + 255) / 256);
    static const bool nofuse = getenv("EH_LFORM_NOFUSE") != nullptr;
    if (mgrid == 1 && !nofuse) { m.slab = h->slab; m.nrows = rows; m.n_acc = (long long)h->n_acc; }      // one workgroup: it writes the slab's tail columns itself
    EhLTailJob tjob{nullptr, 0, nullptr, 0, 0};
    if (tail_s >= 0) {
        const EhLNet& L = h->plan.l_net[0];
        const float* theta = TH(h);
        EhLTailArgs t{};
        t.nl = L.nl - tail_s;
        // dZ_l of the hidden layers where the grouped weight gradients will look for them (the order of the backward loop below: from the top)
        float* dptr[EH_MAX_HIDDEN + 1] = {nullptr};
        { float* q = h->l_dk; for (int l = L.nl - 1; l >= 1; --l) { dptr[l - 1] = q; q += dk_rows * L.in[l]; } }
        int wmax = 4;
        for (int j = 0; j < t.nl; ++j) {
            const int l = tail_s + j;
            EhLTailLayer& T = t.L[j];
            T.W = theta + L.woff[l]; T.b = theta + L.boff[l]; T.in = L.in[l]; T.out = L.out[l]; T.act = L.lact[l];
            T.vec = ((reinterpret_cast<unsigned long long>(T.W) & 15ull) == 0 && (T.out & 3) == 0) ? 1 : 0;
            const bool hidden = l + 1 < L.nl;
            T.H = hidden ? W.H[0][l] : nullptr; T.Z = hidden ? W.Z[0][l] : nullptr; T.D = hidden ? dptr[l] : nullptr;
            eh_ltail_geometry(T);
            if (hidden && T.act == EH_ACT_SWISH) t.any_swish = 1;
            wmax = std::max(wmax, std::max(T.in, T.out));
        }
        (void)wmax;
        t.wmax = (int)EH_LTAIL_MAXW;        // (rows of EH_LTAIL_MAXW + EH_LTAIL_PAD floats whatever the widths: a product reads on past a row's width into zeros, up to the next power of two)
        t.Hin = tail_s == 0 ? W.Xb + L.c0 : W.H[0][tail_s - 1]; t.ldin = tail_s == 0 ? net.P : L.in[tail_s];
        t.act_below = tail_s > 0 ? L.lact[tail_s - 1] : EH_ACT_IDENTITY;
        t.Zin = (tail_s > 0 && t.act_below == EH_ACT_SWISH) ? W.Z[0][tail_s - 1] : nullptr;
        if (t.Zin) t.any_swish = 1;
        t.Dbelow = tail_s > 0 ? dptr[tail_s - 1] : nullptr;
        t.O = W.O + (long long)L.orow * W.ldo; t.ldo = W.ldo; t.part = W.part;
        const int R = 1;
        const int tgrid = (int)((count + R - 1) / R);
        const size_t lds0 = eh_ltail_lds_bytes(R, t.nl, t.wmax, t.any_swish != 0);
        const bool mp = net.mech == EH_MECH_PROGRAM;
        const void* fn = lprog ? (mp ? (const void*)&eh_lform_tailchain_kernel<1, true, true> : (const void*)&eh_lform_tailchain_kernel<1, false, true>)
                               : (mp ? (const void*)&eh_lform_tailchain_kernel<1, true, false> : (const void*)&eh_lform_tailchain_kernel<1, false, false>);
        // one or two hidden layers + the output layer whose weights fit the threads' registers: they stay there for the delta products (eh_lform_tailkeep_kernel)
        static const bool nokeep = getenv("EH_LFORM_NOKEEP") != nullptr;
        int trf = 0;
        const bool keep = !nokeep && R == 1 && eh_ltail_keep_ok(t, (int)count, &trf);
        size_t lds = lds0;
        if (keep) {
            lds = lds0 + ((size_t)trf + 8) * sizeof(float);
            fn = lprog ? (mp ? (const void*)&eh_lform_tailkeep_kernel<true, true> : (const void*)&eh_lform_tailkeep_kernel<false, true>)
                       : (mp ? (const void*)&eh_lform_tailkeep_kernel<true, false> : (const void*)&eh_lform_tailkeep_kernel<false, false>);
        }
        if (lds > EH_LDS_LIMIT) return fail(h, EH_EUNSUPPORTED, "layer-wise form: %zu bytes of LDS for the tail chain", lds);
        bool& prepared = h->l_tail_fn[(keep ? 8 : 0) + (lprog ? 2 : 0) + (mp ? 1 : 0)];      // (per handle = per device)
        if (!prepared) { HIPCHK(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)EH_LDS_LIMIT)); prepared = true; }
        void* kargs[] = {(void*)&net, (void*)&a, (void*)&t, (void*)&h->image};
        HIPCHK(h, hipLaunchKernel(fn, dim3((unsigned)tgrid), dim3(EH_LTAIL_THREADS), kargs, lds, h->stream));
        tjob = EhLTailJob{W.part, tgrid, h->slab, rows, (long long)h->n_acc};
    } else
    if (lprog) {
        if (net.mech == EH_MECH_PROGRAM) hipLaunchKernelGGL((eh_lform_mech_kernel<true, true, true>), dim3(mgrid), dim3(256), 0, h->stream, net, a, m, h->image);
        else hipLaunchKernelGGL((eh_lform_mech_kernel<true, false, true>), dim3(mgrid), dim3(256), 0, h->stream, net, a, m, h->image);
    }
    else if (net.mech == EH_MECH_PROGRAM) hipLaunchKernelGGL((eh_lform_mech_kernel<true, true>), dim3(mgrid), dim3(256), 0, h->stream, net, a, m, h->image);
    else hipLaunchKernelGGL((eh_lform_mech_kernel<true, false>), dim3(mgrid), dim3(256), 0, h->stream, net, a, m, h->image);
    HIPCHK(h, hipGetLastError());
    if (!m.slab && tail_s < 0) {
        hipLaunchKernelGGL(eh_lform_tail_kernel, dim3(1), dim3(256), 0, h->stream, W.part, mgrid, net, h->slab, rows, (long long)h->n_acc);
        HIPCHK(h, hipGetLastError());
    }
    // backward, every network from its output layer down; dZ of the output layer = its rows of d loss / d O^T, still [K][ldo]
    const float* theta = TH(h);
    EhGemmGroup GG{}; EhThinGroup TG{};
    float* tot_job = nullptr;              // where a delta product's side job leaves the sums of the chain's partial rows (only the few-rows product kernel takes the job: l_job_done)
    h->l_job_done = false;
    bool all_grouped = true;               // every weight-gradient product of the step sits in GG / TG (none launched on its own, no group flushed early)
    auto flush_tiled = [&]() {
        if (GG.n > 0) hipLaunchKernelGGL((eh_gemm_group_kernel<true, false, EH_GEPI_STORE, true, 64>), dim3((unsigned)GG.t0[GG.n]), dim3(256), 0, h->stream, GG);
        GG.n = 0;
    };
    auto flush_thin = [&]() {
        if (TG.n > 0) hipLaunchKernelGGL(eh_thin_gemm_group_kernel, dim3((unsigned)TG.t0[TG.n]), dim3(256), 0, h->stream, TG);
        TG.n = 0;
    };
    float* dkp = h->l_dk;
    for (int k = 0; k < h->plan.l_nnets; ++k) {
        const EhLNet& L = h->plan.l_net[k];
        const float* dZ = W.O + (long long)L.orow * W.ldo;
        bool dz_t = true;                      // dZ stored transposed ([out][B])
        int which = 0;
        for (int l = L.nl - 1; l >= 0; --l) {
            const int in = L.in[l], out = L.out[l];
            if (eh_is_norm(L.kind[l])) {                    // a BatchNorm / LayerNorm layer: dZ is d loss / d its output; its leaves' sums to the slab, the delta of the layer below to the other buffer
                float* const dnext = W.D[which];
                if (int rc = eh_is_layernorm(L.kind[l]) ? lnl_backward_layer(h, l, B, dZ, dnext, rows, W) : bnl_backward_layer(h, l, B, dZ, dnext, rows, W)) return rc;
                dZ = dnext; dz_t = false; which ^= 1;
                continue;
            }
            const float* Hprev = l == 0 ? W.Xb + L.c0 : W.H[k][l - 1];
            const long long ldp = l == 0 ? net.P : in;
            EhGemmArgs g{};                    // dW_l^T [in x out] = Hprev^T [in x B] * dZ_l [B x out], split over the samples
            g.A = Hprev; g.lda = ldp; g.B = dZ; g.ldb = dz_t ? W.ldo : out;
            g.C = h->slab + L.woff[l]; g.ldc = out; g.M = in; g.N = out; g.K = B; g.kchunk = chunk; g.c_zstride = h->n_acc;
            g.colsum = h->slab + L.boff[l];      // db_l = column sums of dZ_l, from the same tiles
            EhThinArgs ta;
            if (grouped && lform_thin_args(g, dz_t, &ta)) {
                if (TG.n == EH_GEMM_GROUP) { flush_thin(); all_grouped = false; HIPCHK(h, hipGetLastError()); }
                const int gx = (ta.ncols + 63) / 64;
                TG.a[TG.n] = ta; TG.gx[TG.n] = gx; TG.t0[TG.n + 1] = TG.t0[TG.n] + gx * rows; ++TG.n;
            } else if (grouped && !dz_t && eh_gemm_vec_ok(g, true, false)) {
                if (GG.n == EH_GEMM_GROUP) { flush_tiled(); all_grouped = false; HIPCHK(h, hipGetLastError()); }
                const int gx = (g.N + 63) / 64, gy = (g.M + 63) / 64;
                GG.g[GG.n] = g; GG.gx[GG.n] = gx; GG.gy[GG.n] = gy; GG.t0[GG.n + 1] = GG.t0[GG.n] + gx * gy * rows; ++GG.n;
            } else {
                // (in grouped mode too: dZ_l stays where it is until the step ends)
                all_grouped = false;
                if (dz_t) lform_gemm<true, true, EH_GEPI_STORE>(h, g, rows); else lform_gemm<true, false, EH_GEPI_STORE>(h, g, rows);
                HIPCHK(h, hipGetLastError());
            }
            if (l > 0) {                       // dZ_{l-1} [B x in] = (dZ_l [B x out] * W_l [out x in]) .* act'(H_{l-1})  (swish: act' from the stored Z_{l-1})
                EhGemmArgs b{};
                b.A = dZ; b.lda = dz_t ? W.ldo : out; b.B = theta + L.woff[l]; b.ldb = out;        // W_l element (k = out, n = in) at n * out + k
                float* const dnext = grouped ? dkp : W.D[which];
                if (grouped) dkp += dk_rows * in;
                if (!(tail_s >= 0 && l >= tail_s)) {      // (the tail chain has left this delta where the weight gradients look for it)
                    if (tjob.part && !h->l_job_done && h->l_apply && rows == 1) {      // (its first workgroup also adds up the chain's rows of partial sums: eh_dw_apply_kernel finds them ready)
                        b.job_part = tjob.part; b.job_nblk = tjob.nblk; b.job_out = W.part + (size_t)2048 * EH_LMECH_PART;
                        tot_job = b.job_out;
                    }
                    b.C = dnext; b.ldc = in; b.M = B; b.N = in; b.K = out; b.kchunk = out; b.c_zstride = 0;
                    b.H = L.lact[l - 1] == EH_ACT_SWISH ? W.Z[k][l - 1] : W.H[k][l - 1]; b.ldh = in; b.act = L.lact[l - 1];
                    if (eh_is_norm(L.kind[l - 1])) { b.H = W.H[k][l - 1]; b.act = EH_ACT_IDENTITY; }      // (the layer below is a BatchNorm layer: its backward applies its own act')
                    if (dz_t) lform_gemm<true, true, EH_GEPI_DACT>(h, b, 1); else lform_gemm<false, true, EH_GEPI_DACT>(h, b, 1);
                    HIPCHK(h, hipGetLastError());
                }
                dZ = dnext; dz_t = false; which ^= 1;
            }
        }
    }
    static const bool nodwmerge = getenv("EH_LFORM_NODWMERGE") != nullptr;
    static const bool noapply = getenv("EH_LFORM_NOAPPLY") != nullptr;
    if (h->l_apply && !noapply && tjob.part && all_grouped && rows == 1) {
        // one slab row: the products ARE the gradient -- the optimiser runs in their epilogues (eh_dw_apply_kernel), no reduce launch behind them
        EhLApply ap = *h->l_apply;
        ap.slab = h->slab; ap.part = tjob.part; ap.nblk = tjob.nblk; ap.tot = h->l_job_done ? tot_job : nullptr;
        ap.stamps = stamp_dw ? h->stamps : nullptr;      // (diagnostic builds: the stamps of this launch instead of the chain kernel's)
        ap.stamp_wg = stamp_dw ? atoi(getenv("EH_STAMP_DW")) : 0;
        if (ap.stamp_wg < 0) ap.stamp_wg += TG.t0[TG.n] + GG.t0[GG.n] + 1;
        static const bool noapply64 = getenv("EH_LFORM_NOAPPLY64") != nullptr;
        if (B <= 64 && ap.tot && !noapply64) {       // everything requested at once, 32 x 32 tiles with the samples split over the waves (eh_dw_apply64_kernel)
            for (int i = 0; i < GG.n; ++i) {
                GG.gx[i] = (GG.g[i].N + 31) / 32; GG.gy[i] = (GG.g[i].M + 31) / 32;
                GG.t0[i + 1] = GG.t0[i] + GG.gx[i] * GG.gy[i];
            }
            if (ap.stamp_wg < 0) ap.stamp_wg = TG.t0[TG.n] + GG.t0[GG.n];
#ifdef EH_STAMPS
            if (ap.stamps) { hipMemsetAsync(ap.stamps + 28, 0xff, 8, h->stream); hipMemsetAsync(ap.stamps + 30, 0, 8, h->stream); }
#endif
            hipLaunchKernelGGL(eh_dw_apply64_kernel, dim3((unsigned)(TG.t0[TG.n] + 8 * ((GG.t0[GG.n] + 7) / 8) + 1)), dim3(256), 0, h->stream, GG, TG, net, ap);
            if (!h->chain.n) ++h->upd_site[EH_UPD_DW_APPLY64];      // (under a chain the epilogue only leaves the gradient, eh_do_step)
        } else {
        hipLaunchKernelGGL(eh_dw_apply_kernel, dim3((unsigned)(TG.t0[TG.n] + GG.t0[GG.n] + 1)), dim3(256), 0, h->stream, GG, TG, net, ap);
        if (!h->chain.n) ++h->upd_site[EH_UPD_DW_APPLY];
        }
        HIPCHK(h, hipGetLastError());
        h->l_applied = true;
        return EH_OK;
    }
    if (tjob.part || (TG.n > 0 && GG.n > 0 && !nodwmerge)) {       // what is left of both groups: one launch (+ the workgroup that sums the tail chain's partial rows)
        hipLaunchKernelGGL(eh_dw_group_kernel, dim3((unsigned)(TG.t0[TG.n] + GG.t0[GG.n] + (tjob.part ? 1 : 0))), dim3(256), 0, h->stream, GG, TG, tjob, net);
        TG.n = 0; GG.n = 0;
        HIPCHK(h, hipGetLastError());
    }
    flush_thin(); HIPCHK(h, hipGetLastError());
    flush_tiled(); HIPCHK(h, hipGetLastError());
    return EH_OK;
}
// forward + metric sums of samples [first, first+count) in chunks; per-workgroup rows of EH_EVAL_STATS * T sums land in the slab
int eh_lform_eval(eh_handle* h, const EhSplit& sp, long long first, long long count, float* yhat, float* pout, int* rows_out) {
    const EhNet& net = h->net;
    const long long CH = 65536;
    int rows = 0;
    const int ncol = EH_EVAL_STATS * net.T;
    for (long long c0 = 0; c0 < count; c0 += CH) {
        const long long n = std::min(CH, count - c0);
        EhLWs W;
        if (int rc = lform_workspace(h, n, &W)) return rc;
        if (int rc = lform_forward(h, sp, nullptr, first + c0, n, false, false, W)) return rc;
        EhStepArgs a = eh_step_args(h, sp, nullptr, first + c0, n);
        a.yhat = yhat ? yhat + c0 : nullptr; a.pout = pout ? pout + c0 : nullptr; a.yld = count;
        const int mgrid = (int)std::min<long long>(256, (n + 255) / 256);
        if ((size_t)(rows + mgrid) * ncol > std::max((size_t)h->slab_rows * std::max(h->n_acc, ncol), (size_t)1 << 20)) return fail(h, EH_ENOMEM, "eh_eval: window too large for the metric rows");
        EhLMechArgs m{W.O, W.ldo, h->slab + (size_t)rows * ncol};
        if (net.mech == EH_MECH_PROGRAM) hipLaunchKernelGGL((eh_lform_mech_kernel<false, true>), dim3(mgrid), dim3(256), 0, h->stream, net, a, m, h->image);
        else hipLaunchKernelGGL((eh_lform_mech_kernel<false, false>), dim3(mgrid), dim3(256), 0, h->stream, net, a, m, h->image);
        HIPCHK(h, hipGetLastError());
        rows += mgrid;
    }
    *rows_out = std::max(rows, 0);
    return EH_OK;
}
