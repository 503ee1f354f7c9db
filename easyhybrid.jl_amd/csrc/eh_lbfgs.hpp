// L-BFGS on the device (the reference's Optimization.jl driver, src/training/train_optimization.jl).  eh_lbfgs.hip is its unit: it defines
// EH_LBFGS_KERNELS and holds the only instantiation of the decision code and the kernels; everybody else sees the constants and EhLbfgs.
//
// One objective evaluation is always the same launches, enqueued without a synchronisation:
//
//   eh_do_step(apply = false)    the step kernel and eh_reduce_kernel<false, ...> the handle runs anyway: gradient, loss and valid counts
//                              in gradbuf, at the trial point theta
//   eh_lbfgs_dots_kernel       every dot product the decision may need, one row of partial sums per workgroup (at most EH_LB_PARTS)
//   eh_lbfgs_decide_kernel     ONE workgroup: folds the rows in row order, then one thread runs eh_lb_decide -- the weak-Wolfe bisection
//                              of Lewis and Overton and, on accept, the two-loop recursion in COEFFICIENT space: the direction is a
//                              combination of the basis {S_0.., Y_0.., g}, and the recursion only needs the basis' Gram matrix, which is
//                              kept in device memory and gets the new rows of this evaluation.  Nothing is summed between dependent steps
//   eh_lbfgs_apply_kernel      element-wise: the pair into its ring slot, x0 <- theta, g0 <- g, d <- sum coef_j basis_j,
//                              theta <- x0 + t d, the parameter image through eh_image_store
//   eh_lbfgs_one_kernel        all three in ONE workgroup where n_theta is small (EH_LB_ONE_MAX).  It walks the same virtual
//                              workgroups in the same order as the three-kernel form, so the two give the same bits
//
// No workgroup waits for another, nothing spins, no atomics: the launches' stream order is the only ordering.  Once the solve is done
// (state[EH_LS_DONE] != 0) the kernels write nothing, so evaluations enqueued behind the end of a solve are harmless.
// Sums in a fixed order as in eh_chain_norm_kernel (a thread's elements ascending, xor butterfly over the wave, the waves as
// (0+1)+(2+3), the rows ascending) and in double; theta, the gradients and the history stay fp32.
// eh_lb_decide and eh_lb_direction are __host__ __device__: eh_lbfgs_host_decide runs the very same code on the CPU.
#pragma once
#include "eh_internal.hpp"

enum { EH_LB_MAX_M = EH_LBFGS_MAX_M, EH_LB_NB = 2 * EH_LBFGS_MAX_M + 1, EH_LB_PARTS = 256, EH_LB_TRACE_ROWS = 4096 };
// the sums of one evaluation: q[0 .. 8) and, for basis vector j (S_j: j < m, Y_{j-m}: m <= j < 2m), q[8 + 3 j ..] = g.H_j, s.H_j, y.H_j
enum { EH_LQ_GD = 0, EH_LQ_SY, EH_LQ_YY, EH_LQ_GINF, EH_LQ_GG, EH_LQ_SS, EH_LQ_SG, EH_LQ_YG, EH_LQ_HIST = 8 };
enum { EH_LB_NQ_MAX = EH_LQ_HIST + 6 * EH_LBFGS_MAX_M };
// the solve's scalars, all kept as doubles (counts too: exact)
enum { EH_LS_DONE = 0, EH_LS_PHASE, EH_LS_ITERS, EH_LS_EVALS, EH_LS_F0, EH_LS_GINF0, EH_LS_GG0, EH_LS_DG0, EH_LS_T, EH_LS_LO, EH_LS_HI, EH_LS_TRIALS,
       EH_LS_AMASK_LO, EH_LS_AMASK_HI, EH_LS_NPAIRS, EH_LS_HEAD, EH_LS_FAILS, EH_LS_LAST_T, EH_LS_ROWS };
// decision record: [action, t, ring slot of the new pair or -1, pairs held, coefficients of d over the 2m + 1 basis vectors]
enum { EH_LR_ACTION = 0, EH_LR_T, EH_LR_SLOT, EH_LR_NPAIRS, EH_LR_COEF = 4 };
enum { EH_LA_NOOP = 0, EH_LA_REJECT = 1, EH_LA_ACCEPT = 2, EH_LA_ACCEPT_DONE = 3, EH_LA_RESTART = 4, EH_LA_FAIL_DONE = 5,
       EH_LA_ACCEPT_PAUSE = 6 /* maxiters reached: everything of ACCEPT but the move to the next trial point (eh_lbfgs_resume_kernel makes it) */ };

static_assert(EH_LS_ROWS < EH_LBFGS_STATE_DOUBLES, "state");
static_assert(EH_LR_COEF + EH_LB_NB <= EH_LBFGS_RECORD_DOUBLES, "record");
static_assert(EH_LB_NQ_MAX <= EH_LBFGS_SUMS_DOUBLES, "sums");

// the handle's side (eh_lbfgs_init)
enum { EH_LB_DBL_HEAD = EH_LBFGS_STATE_DOUBLES + EH_LBFGS_RECORD_DOUBLES + EH_LB_NB * EH_LB_NB };      // state | record | Gram matrix, then the partial rows
// n_theta up to which one workgroup takes dots, decision and update in one launch.  Measured (tools/bench_lbfgs.py --threshold,
// profiles/r15/lbfgs.txt): at 338 parameters one launch is 2.2 us per evaluation cheaper than three (55.8 against 58.0), at 1 186 it is
// 15.9 us dearer (86.8 against 70.9) -- 0.037 us per parameter against 0.015, so the two meet near 440.
enum { EH_LB_ONE_MAX = 384 };
struct EhLbfgs {
    bool active = false, batch_set = false, empty = false;
    eh_lbfgs_opts o{};
    int maxiters = 100, nq = 0, m_cap = 0;
    float* vec = nullptr;          // x0 | g0 | d | S[m] | Y[m]
    double* dbl = nullptr;         // EH_LB_DBL_HEAD doubles, then [EH_LB_PARTS][nq]
    float* trace = nullptr;
    int* idx = nullptr;            // the batch's indices where the caller's were on the host
    long long idx_cap = 0;
    int split = 0;
    const int* didx = nullptr;
    long long first = 0, count = 0;
};

#ifdef EH_LBFGS_KERNELS
#ifndef EH_HD
#define EH_HD __host__ __device__ inline
#endif

EH_HD bool eh_lb_finite(double x) { return x - x == 0.0; }

// first step of a steepest-descent restart: min(1, 1 / ||g||_2) unless the caller fixed it
EH_HD double eh_lb_first_t(const eh_lbfgs_opts& o, double gg) {
    if (o.initial_step > 0.0) return o.initial_step;
    const double r = 1.0 / sqrt(gg);
    return r < 1.0 ? r : 1.0;
}

// sum_j c_j G[row][j] over the valid basis vectors: S_0 .. S_{np-1}, Y_0 .. Y_{np-1}, g -- in that order.  Fixed trip counts with the
// slots that hold nothing contributing +0: on the device one lane runs this on operands in LDS, and a loop of np dependent
// load-then-add steps cost 35 us of a 48 us evaluation (profiles/r15/lbfgs.txt); unrolled, the loads are issued together.
EH_HD double eh_lb_row_dot(int m, int np, const double* c, const double* G, int row) {
    const double* g = G + row * EH_LB_NB;
    double ps[EH_LB_MAX_M], py[EH_LB_MAX_M];
#pragma unroll
    for (int j = 0; j < EH_LB_MAX_M; ++j) {            // (m + j <= 31: inside both arrays whatever m is)
        const double vs = c[j] * g[j], vy = c[m + j] * g[m + j];
        ps[j] = j < np ? vs : 0.0;
        py[j] = j < np ? vy : 0.0;
    }
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < EH_LB_MAX_M; ++j) a += ps[j];
#pragma unroll
    for (int j = 0; j < EH_LB_MAX_M; ++j) a += py[j];
    return a + c[2 * m] * g[2 * m];
}

// two-loop recursion on coefficient vectors, H0 = (s.y / y.y) I of the newest pair: coef <- the coefficients of d = -H g; returns g.d
EH_HD double eh_lb_direction(int m, int np, int head, const double* G, double* coef) {
    const int ig = 2 * m;
    double alpha[EH_LB_MAX_M];
    for (int j = 0; j <= ig; ++j) coef[j] = 0.0;
    coef[ig] = 1.0;
    for (int k = 0; k < np; ++k) {                       // newest -> oldest
        const int i = (head - 1 - k + 2 * m) % m;
        const double a = eh_lb_row_dot(m, np, coef, G, i) / G[i * EH_LB_NB + m + i];
        alpha[k] = a;
        coef[m + i] -= a;
    }
    if (np > 0) {
        const int i = (head - 1 + m) % m;
        const double gamma = G[i * EH_LB_NB + m + i] / G[(m + i) * EH_LB_NB + m + i];
        for (int j = 0; j <= ig; ++j) coef[j] *= gamma;
    }
    for (int k = np - 1; k >= 0; --k) {                  // oldest -> newest
        const int i = (head - 1 - k + 2 * m) % m;
        const double b = eh_lb_row_dot(m, np, coef, G, m + i) / G[i * EH_LB_NB + m + i];
        coef[i] += alpha[k] - b;
    }
    for (int j = 0; j <= ig; ++j) coef[j] = -coef[j];
    return eh_lb_row_dot(m, np, coef, G, ig);
}

EH_HD void eh_lb_new_search(double* st, double dg0, double t) {
    st[EH_LS_DG0] = dg0; st[EH_LS_T] = t; st[EH_LS_LO] = 0.0; st[EH_LS_HI] = INFINITY;
    st[EH_LS_TRIALS] = 0.0; st[EH_LS_AMASK_LO] = 0.0; st[EH_LS_AMASK_HI] = 0.0;
}

// One evaluation's decision.  st: EH_LS_*; G: Gram matrix [EH_LB_NB][EH_LB_NB] of the basis; q: this evaluation's sums (EH_LQ_*); f, nv:
// loss and valid samples; rec: the decision record; row: [f, t, trials, ||g||inf, s.y, Armijo mask bits 0-23, bits 24-47, evaluations]
// of an accepted iteration.  Returns 1 when it wrote a trace row.
EH_HD int eh_lb_decide(const eh_lbfgs_opts& o, int maxiters, double* st, double* G, const double* q, double f, double nv, double* rec, double* row) {
    const int m = o.m, ig = 2 * m;
    rec[EH_LR_ACTION] = EH_LA_NOOP; rec[EH_LR_T] = st[EH_LS_T]; rec[EH_LR_SLOT] = -1.0; rec[EH_LR_NPAIRS] = st[EH_LS_NPAIRS];
    for (int j = 0; j <= ig; ++j) rec[EH_LR_COEF + j] = 0.0;
    if (st[EH_LS_DONE] != 0.0) return 0;
    st[EH_LS_EVALS] += 1.0;
    const double gg = q[EH_LQ_GG], ginf = q[EH_LQ_GINF];
    if (st[EH_LS_PHASE] == 0.0) {                        // the evaluation at the starting point
        if (!(nv > 0.0)) { st[EH_LS_DONE] = EH_LBFGS_EMPTY_BATCH; return 0; }
        st[EH_LS_F0] = f; st[EH_LS_GINF0] = ginf; st[EH_LS_GG0] = gg; st[EH_LS_PHASE] = 1.0;
        G[ig * EH_LB_NB + ig] = gg;
        rec[EH_LR_ACTION] = EH_LA_ACCEPT_DONE;
        if (!eh_lb_finite(f) || !eh_lb_finite(gg)) { st[EH_LS_DONE] = EH_LBFGS_LINESEARCH_FAILED; return 0; }
        if (ginf <= o.g_tol) { st[EH_LS_DONE] = EH_LBFGS_CONVERGED_G; return 0; }
        const double t = eh_lb_first_t(o, gg);
        eh_lb_new_search(st, -gg, t);
        rec[EH_LR_ACTION] = EH_LA_ACCEPT; rec[EH_LR_T] = t; rec[EH_LR_NPAIRS] = 0.0; rec[EH_LR_COEF + ig] = -1.0;
        if (maxiters <= 0) { st[EH_LS_DONE] = EH_LBFGS_MAXITERS; rec[EH_LR_ACTION] = EH_LA_ACCEPT_PAUSE; }
        return 0;
    }
    const double t = st[EH_LS_T], f0 = st[EH_LS_F0], dg0 = st[EH_LS_DG0];
    const int trials = (int)st[EH_LS_TRIALS] + 1;
    st[EH_LS_TRIALS] = trials;
    bool accept = false;
    if (!eh_lb_finite(f) || f > f0 + o.c1 * t * dg0) {   // Armijo
        st[EH_LS_HI] = t;
        const int b = trials - 1;
        if (b < 24) st[EH_LS_AMASK_LO] += (double)(1 << b); else if (b < 48) st[EH_LS_AMASK_HI] += (double)(1 << (b - 24));
    } else if (q[EH_LQ_GD] < o.c2 * dg0) st[EH_LS_LO] = t;      // curvature
    else accept = true;
    if (!accept) {
        if (trials >= o.max_linesearch) {
            if (st[EH_LS_FAILS] >= 1.0) {                // the second failure in a row: the solve ends at x0
                st[EH_LS_DONE] = EH_LBFGS_LINESEARCH_FAILED;
                rec[EH_LR_ACTION] = EH_LA_FAIL_DONE;
                return 0;
            }
            st[EH_LS_FAILS] = 1.0; st[EH_LS_NPAIRS] = 0.0; st[EH_LS_HEAD] = 0.0;      // drop the history, once more from -g0
            const double t1 = eh_lb_first_t(o, st[EH_LS_GG0]);
            eh_lb_new_search(st, -st[EH_LS_GG0], t1);
            rec[EH_LR_ACTION] = EH_LA_RESTART; rec[EH_LR_T] = t1; rec[EH_LR_NPAIRS] = 0.0; rec[EH_LR_COEF + ig] = -1.0;
            return 0;
        }
        const double lo = st[EH_LS_LO], hi = st[EH_LS_HI];
        const double tn = eh_lb_finite(hi) ? 0.5 * (lo + hi) : 2.0 * lo;
        st[EH_LS_T] = tn;
        rec[EH_LR_ACTION] = EH_LA_REJECT; rec[EH_LR_T] = tn;
        return 0;
    }
    // accepted
    const double sy = q[EH_LQ_SY], yy = q[EH_LQ_YY];
    const int iters = (int)st[EH_LS_ITERS] + 1;
    st[EH_LS_ITERS] = iters; st[EH_LS_FAILS] = 0.0; st[EH_LS_LAST_T] = t;
    row[0] = f; row[1] = t; row[2] = trials; row[3] = ginf; row[4] = sy; row[5] = st[EH_LS_AMASK_LO]; row[6] = st[EH_LS_AMASK_HI]; row[7] = st[EH_LS_EVALS];
    int done = 0;
    if (ginf <= o.g_tol) done = EH_LBFGS_CONVERGED_G;
    else {
        const double a0 = fabs(f0), a1 = fabs(f);
        const double den = a0 > a1 ? (a0 > 1.0 ? a0 : 1.0) : (a1 > 1.0 ? a1 : 1.0);
        if (o.f_reltol > 0.0 && (f0 - f) / den <= o.f_reltol) done = EH_LBFGS_CONVERGED_F;
        else if (iters >= maxiters) done = EH_LBFGS_MAXITERS;
    }
    int np = (int)st[EH_LS_NPAIRS], head = (int)st[EH_LS_HEAD], p = -1;
    const int np_old = np;
    if (sy > 1e-10 * yy) {                               // the pair enters the ring
        p = head;
        for (int j = 0; j < np_old; ++j) {
            if (j == p) continue;
            for (int w = 0; w < 2; ++w) {                // against S_j (w = 0) and Y_j (w = 1)
                const int b = w * m + j;
                const double sh = q[EH_LQ_HIST + 3 * b + 1], yh = q[EH_LQ_HIST + 3 * b + 2];
                G[p * EH_LB_NB + b] = sh; G[b * EH_LB_NB + p] = sh;
                G[(m + p) * EH_LB_NB + b] = yh; G[b * EH_LB_NB + m + p] = yh;
            }
        }
        G[p * EH_LB_NB + p] = q[EH_LQ_SS];
        G[p * EH_LB_NB + m + p] = sy; G[(m + p) * EH_LB_NB + p] = sy;
        G[(m + p) * EH_LB_NB + m + p] = yy;
        head = (head + 1) % m;
        if (np < m) ++np;
    }
    for (int j = 0; j < np_old; ++j) {                   // the new gradient against the pairs that stay
        if (j == p) continue;
        for (int w = 0; w < 2; ++w) {
            const int b = w * m + j;
            const double gh = q[EH_LQ_HIST + 3 * b];
            G[ig * EH_LB_NB + b] = gh; G[b * EH_LB_NB + ig] = gh;
        }
    }
    if (p >= 0) {
        G[ig * EH_LB_NB + p] = q[EH_LQ_SG]; G[p * EH_LB_NB + ig] = q[EH_LQ_SG];
        G[ig * EH_LB_NB + m + p] = q[EH_LQ_YG]; G[(m + p) * EH_LB_NB + ig] = q[EH_LQ_YG];
    }
    G[ig * EH_LB_NB + ig] = gg;
    st[EH_LS_NPAIRS] = np; st[EH_LS_HEAD] = head;
    st[EH_LS_F0] = f; st[EH_LS_GINF0] = ginf; st[EH_LS_GG0] = gg;
    rec[EH_LR_SLOT] = p; rec[EH_LR_NPAIRS] = np;
    if (done && done != EH_LBFGS_MAXITERS) {
        st[EH_LS_DONE] = done;
        rec[EH_LR_ACTION] = EH_LA_ACCEPT_DONE;
        return 1;
    }
    double ndg = eh_lb_direction(m, np, head, G, rec + EH_LR_COEF);
    if (!(ndg < 0.0)) {                                  // not a descent direction (rounding in a nearly singular history): steepest descent
        st[EH_LS_NPAIRS] = 0.0; st[EH_LS_HEAD] = 0.0;
        rec[EH_LR_SLOT] = -1.0; rec[EH_LR_NPAIRS] = 0.0;
        for (int j = 0; j < ig; ++j) rec[EH_LR_COEF + j] = 0.0;
        rec[EH_LR_COEF + ig] = -1.0;
        ndg = -gg;
    }
    eh_lb_new_search(st, ndg, 1.0);
    rec[EH_LR_ACTION] = EH_LA_ACCEPT; rec[EH_LR_T] = 1.0;
    if (done) { st[EH_LS_DONE] = done; rec[EH_LR_ACTION] = EH_LA_ACCEPT_PAUSE; }      // maxiters: the next search is set up, theta stays at the accepted point
    return 1;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------------------------
struct EhLbfgsArgs {
    const float* gradbuf;          // [gradient | loss | n_t ..] of this evaluation
    float* theta;                  // the trial point
    float *x0, *g0, *d, *S, *Y;    // [n] each; S, Y: [m][n] ring slots
    double* st;                    // EH_LS_*
    double* rec;                   // EH_LR_*
    double* gram;                  // [EH_LB_NB][EH_LB_NB]
    double* part;                  // [EH_LB_PARTS][nq] partial rows
    float* trace;                  // [EH_LB_TRACE_ROWS][8]
    int n, T, nq, nparts, maxiters;
    eh_lbfgs_opts o;
};

__device__ __forceinline__ double eh_lb_wave_sum(double a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
    return a;
}
__device__ __forceinline__ double eh_lb_max(double a, double b) { return (a > b || a != a) ? a : b; }      // (a NaN stays)

// the partial row of (virtual) workgroup vb of nb: elements vb * 256 + tid, then every nb * 256 further.  red: [EH_LB_NQ_MAX][4]
__device__ __forceinline__ void eh_lb_dots_phase(const EhLbfgsArgs& a, int vb, int nb, int np, double (*red)[4]) {
    const int tid = threadIdx.x, w = tid >> 6, m = a.o.m, n = a.n;
    const bool lead = (tid & 63) == 0;
    __syncthreads();                                     // (red may still be read from the row before this one)
    for (int k = tid; k < a.nq * 4; k += 256) red[k >> 2][k & 3] = 0.0;
    __syncthreads();
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int idx = vb * 256 + tid; idx < n; idx += nb * 256) {
        const float gf = a.gradbuf[idx], sf = a.theta[idx] - a.x0[idx], yf = gf - a.g0[idx];
        const double g = gf, s = sf, y = yf;
        acc[EH_LQ_GD] += g * (double)a.d[idx];
        acc[EH_LQ_SY] += s * y; acc[EH_LQ_YY] += y * y;
        acc[EH_LQ_GINF] = eh_lb_max(acc[EH_LQ_GINF], fabs(g));
        acc[EH_LQ_GG] += g * g; acc[EH_LQ_SS] += s * s; acc[EH_LQ_SG] += s * g; acc[EH_LQ_YG] += y * g;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double v = acc[k];
        if (k == EH_LQ_GINF) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v = eh_lb_max(v, __shfl_xor(v, off, 64));
        } else v = eh_lb_wave_sum(v);
        if (lead) red[k][w] = v;
    }
    // the held pairs, S_0 .. S_{np-1} then Y_0 .. Y_{np-1}, four vectors per pass: their loads are in flight together and the twelve
    // butterflies interleave (one vector per pass waited for memory and for the shuffles twenty times per evaluation)
    for (int j0 = 0; j0 < 2 * np; j0 += 4) {
        const float* H[4];
        int b[4];
        double hg[4] = {0, 0, 0, 0}, hs[4] = {0, 0, 0, 0}, hy[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int jj = j0 + k < 2 * np ? j0 + k : j0;      // (past the end: the pass's first vector again, result dropped)
            b[k] = jj < np ? jj : m + (jj - np);
            H[k] = (jj < np ? a.S : a.Y) + (size_t)(jj < np ? jj : jj - np) * n;
        }
        for (int idx = vb * 256 + tid; idx < n; idx += nb * 256) {
            const float gf = a.gradbuf[idx], sf = a.theta[idx] - a.x0[idx], yf = gf - a.g0[idx];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double hv = H[k][idx];
                hg[k] += (double)gf * hv; hs[k] += (double)sf * hv; hy[k] += (double)yf * hv;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double vg = eh_lb_wave_sum(hg[k]), vs = eh_lb_wave_sum(hs[k]), vy = eh_lb_wave_sum(hy[k]);
            if (lead && j0 + k < 2 * np) { red[EH_LQ_HIST + 3 * b[k]][w] = vg; red[EH_LQ_HIST + 3 * b[k] + 1][w] = vs; red[EH_LQ_HIST + 3 * b[k] + 2][w] = vy; }
        }
    }
    __syncthreads();
    if (tid < a.nq) {
        const double* r = red[tid];
        a.part[(size_t)vb * a.nq + tid] = tid == EH_LQ_GINF ? eh_lb_max(eh_lb_max(r[0], r[1]), eh_lb_max(r[2], r[3])) : (r[0] + r[1]) + (r[2] + r[3]);
    }
}

// folds the nb rows in row order and decides; leaves the record in rec_s (LDS) and in global memory.  sh: scratch of EH_LB_NQ_MAX +
// EH_LBFGS_STATE_DOUBLES + EH_LB_NB * EH_LB_NB doubles
__device__ __forceinline__ void eh_lb_decide_phase(const EhLbfgsArgs& a, int nb, double* sh, double* rec_s) {
    const int tid = threadIdx.x;
    double* q = sh;
    double* st = sh + EH_LB_NQ_MAX;
    double* G = st + EH_LBFGS_STATE_DOUBLES;
    __syncthreads();                                     // (one-launch form: the rows were stored by this workgroup)
    if (tid < a.nq) {
        double v = 0.0;
        for (int r = 0; r < nb; ++r) {
            const double x = a.part[(size_t)r * a.nq + tid];
            v = tid == EH_LQ_GINF ? eh_lb_max(v, x) : v + x;
        }
        q[tid] = v;
    }
    for (int k = tid; k < EH_LBFGS_STATE_DOUBLES; k += 256) st[k] = a.st[k];
    for (int k = tid; k < EH_LB_NB * EH_LB_NB; k += 256) G[k] = a.gram[k];
    __syncthreads();
    if (tid == 0) {
        double nv = 0.0;
        for (int t = 0; t < a.T; ++t) nv += (double)a.gradbuf[a.n + 1 + t];
        double row[8];
        const int rows = (int)st[EH_LS_ROWS];
        if (eh_lb_decide(a.o, a.maxiters, st, G, q, (double)a.gradbuf[a.n], nv, rec_s, row)) {
            if (rows < (int)EH_LB_TRACE_ROWS)
                for (int k = 0; k < 8; ++k) a.trace[(size_t)rows * 8 + k] = (float)row[k];
            st[EH_LS_ROWS] = rows + 1;
        }
    }
    __syncthreads();
    const int action = (int)rec_s[EH_LR_ACTION];
    for (int k = tid; k < EH_LBFGS_STATE_DOUBLES; k += 256) a.st[k] = st[k];
    if (action == EH_LA_ACCEPT || action == EH_LA_ACCEPT_DONE || action == EH_LA_ACCEPT_PAUSE)
        for (int k = tid; k < EH_LB_NB * EH_LB_NB; k += 256) a.gram[k] = G[k];
    for (int k = tid; k < EH_LBFGS_RECORD_DOUBLES; k += 256) a.rec[k] = rec_s[k];
}

// elements first + tid, then every `stride` further, as the record says
__device__ __forceinline__ void eh_lb_apply_phase(const EhLbfgsArgs& a, const EhImg& im, const double* rec, int first, int stride) {
    const int action = (int)rec[EH_LR_ACTION];
    if (action == EH_LA_NOOP) return;
    const double t = rec[EH_LR_T];
    const int slot = (int)rec[EH_LR_SLOT], np = (int)rec[EH_LR_NPAIRS], m = a.o.m, n = a.n;
    const double* coef = rec + EH_LR_COEF;
    for (int idx = first + (int)threadIdx.x; idx < n; idx += stride) {
        float th;
        if (action == EH_LA_REJECT) th = (float)((double)a.x0[idx] + t * (double)a.d[idx]);
        else if (action == EH_LA_FAIL_DONE) th = a.x0[idx];
        else if (action == EH_LA_RESTART) {
            const float dd = -a.g0[idx];
            a.d[idx] = dd;
            th = (float)((double)a.x0[idx] + t * (double)dd);
        } else {
            const float x = a.theta[idx], g = a.gradbuf[idx];
            const float s = x - a.x0[idx], y = g - a.g0[idx];
            if (slot >= 0) { a.S[(size_t)slot * n + idx] = s; a.Y[(size_t)slot * n + idx] = y; }
            a.x0[idx] = x; a.g0[idx] = g;
            if (action == EH_LA_ACCEPT_DONE) continue;   // theta is the accepted point already
            double acc = 0.0;
            for (int j = 0; j < np; ++j) acc += coef[j] * (double)(j == slot ? s : a.S[(size_t)j * n + idx]);
            for (int j = 0; j < np; ++j) acc += coef[m + j] * (double)(j == slot ? y : a.Y[(size_t)j * n + idx]);
            acc += coef[2 * m] * (double)g;
            const float dd = (float)acc;
            a.d[idx] = dd;
            if (action == EH_LA_ACCEPT_PAUSE) continue;
            th = (float)((double)x + t * (double)dd);
        }
        a.theta[idx] = th;
        eh_image_store(im, idx, th);
    }
}

__global__ __launch_bounds__(256) void eh_lbfgs_dots_kernel(EhLbfgsArgs a) {
    __shared__ double red[EH_LB_NQ_MAX][4];
    if (a.st[EH_LS_DONE] != 0.0) return;                 // (the same word for every workgroup: the decide kernel of the evaluation before wrote it)
    eh_lb_dots_phase(a, blockIdx.x, gridDim.x, (int)a.st[EH_LS_NPAIRS], red);
}

__global__ __launch_bounds__(256) void eh_lbfgs_decide_kernel(EhLbfgsArgs a) {
    __shared__ double sh[EH_LB_NQ_MAX + EH_LBFGS_STATE_DOUBLES + EH_LB_NB * EH_LB_NB];
    __shared__ double rec_s[EH_LBFGS_RECORD_DOUBLES];
    if (a.st[EH_LS_DONE] != 0.0) {                       // surplus evaluation: the record says "nothing"
        if (threadIdx.x == 0) a.rec[EH_LR_ACTION] = EH_LA_NOOP;
        return;
    }
    eh_lb_decide_phase(a, a.nparts, sh, rec_s);
}

__global__ __launch_bounds__(256) void eh_lbfgs_apply_kernel(EhLbfgsArgs a, EhImg im) {
    __shared__ double rec_s[EH_LBFGS_RECORD_DOUBLES];
    for (int k = threadIdx.x; k < EH_LBFGS_RECORD_DOUBLES; k += 256) rec_s[k] = a.rec[k];
    __syncthreads();
    eh_lb_apply_phase(a, im, rec_s, blockIdx.x * 256, gridDim.x * 256);
}

__global__ __launch_bounds__(256) void eh_lbfgs_one_kernel(EhLbfgsArgs a, EhImg im) {
    __shared__ double red[EH_LB_NQ_MAX][4];
    __shared__ double sh[EH_LB_NQ_MAX + EH_LBFGS_STATE_DOUBLES + EH_LB_NB * EH_LB_NB];
    __shared__ double rec_s[EH_LBFGS_RECORD_DOUBLES];
    if (a.st[EH_LS_DONE] != 0.0) return;
    const int np = (int)a.st[EH_LS_NPAIRS];
    for (int vb = 0; vb < a.nparts; ++vb) eh_lb_dots_phase(a, vb, a.nparts, np, red);
    eh_lb_decide_phase(a, a.nparts, sh, rec_s);
    __syncthreads();
    eh_lb_apply_phase(a, im, rec_s, 0, 256);
}

// eh_lbfgs_set_maxiters on a solve that ended on its iteration limit: with a higher limit it goes on where it stopped -- theta to the
// first trial point of the search that is set up already.  One workgroup: every thread has read the state before thread 0 clears it.
__global__ __launch_bounds__(256) void eh_lbfgs_resume_kernel(EhLbfgsArgs a, EhImg im) {
    const bool go = a.st[EH_LS_DONE] == (double)EH_LBFGS_MAXITERS && a.st[EH_LS_ITERS] < (double)a.maxiters;
    const double t = a.st[EH_LS_T];
    __syncthreads();
    if (!go) return;
    for (int idx = threadIdx.x; idx < a.n; idx += 256) {
        const float th = (float)((double)a.x0[idx] + t * (double)a.d[idx]);
        a.theta[idx] = th;
        eh_image_store(im, idx, th);
    }
    if (threadIdx.x == 0) a.st[EH_LS_DONE] = 0.0;
}
#endif      // EH_LBFGS_KERNELS
