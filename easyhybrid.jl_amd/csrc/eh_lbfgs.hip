// L-BFGS on the device (eh_lbfgs.hpp) as a translation unit of its own: the eh_lbfgs_* entry points and the only instantiation of the
// five kernels.  An objective evaluation is a step of the handle (eh_do_step, eh_api.hip) and the kernels here behind it.
#include <cmath>

#define EH_LBFGS_KERNELS
#include "eh_lbfgs.hpp"

void eh_lbfgs_release(eh_handle* h) {
    if (!h->lb) return;
    (void)hipFree(h->lb->vec); (void)hipFree(h->lb->dbl); (void)hipFree(h->lb->trace); (void)hipFree(h->lb->idx);
    delete h->lb;
    h->lb = nullptr;
}

static EhLbfgsArgs lbfgs_args(const eh_handle* h) {
    const EhLbfgs* lb = h->lb;
    const int n = h->net.n_theta;
    EhLbfgsArgs a{};
    a.gradbuf = h->gradbuf; a.theta = TH(h);
    a.x0 = lb->vec; a.g0 = lb->vec + (size_t)n; a.d = lb->vec + 2 * (size_t)n; a.S = lb->vec + 3 * (size_t)n; a.Y = a.S + (size_t)lb->o.m * n;
    a.st = lb->dbl; a.rec = lb->dbl + EH_LBFGS_STATE_DOUBLES; a.gram = a.rec + EH_LBFGS_RECORD_DOUBLES; a.part = lb->dbl + EH_LB_DBL_HEAD;
    a.trace = lb->trace;
    a.n = n; a.T = h->net.T; a.nq = lb->nq; a.nparts = std::min<int>(EH_LB_PARTS, (n + 1023) / 1024); a.maxiters = lb->maxiters;
    a.o = lb->o;
    return a;
}

static int lbfgs_ready(eh_handle* h, const char* who) {
    if (!h->lb || !h->lb->active) return fail(h, EH_ESTATE, "%s: call eh_lbfgs_init first (eh_opt_init* leaves L-BFGS mode)", who);
    if (h->capturing) return fail(h, EH_EUNSUPPORTED, "%s: graph capture is not built for L-BFGS", who);
    return EH_OK;
}

extern "C" {

int32_t eh_lbfgs_init(eh_handle* h, const eh_lbfgs_opts* o) {
    if (!h || !o) return EH_EINVAL;
    if (o->m < 1 || o->m > EH_LBFGS_MAX_M) return fail(h, EH_EINVAL, "eh_lbfgs_init: m = %d (1..%d)", o->m, (int)EH_LBFGS_MAX_M);
    if (!(o->c1 > 0.0 && o->c1 < o->c2 && o->c2 < 1.0)) return fail(h, EH_EINVAL, "eh_lbfgs_init: need 0 < c1 < c2 < 1 (c1 = %g, c2 = %g)", o->c1, o->c2);
    if (o->max_linesearch < 1 || o->max_linesearch > 48) return fail(h, EH_EINVAL, "eh_lbfgs_init: max_linesearch = %d (1..48)", o->max_linesearch);
    if (!(o->g_tol >= 0.0) || !(o->f_reltol >= 0.0)) return fail(h, EH_EINVAL, "eh_lbfgs_init: g_tol = %g, f_reltol = %g (both >= 0)", o->g_tol, o->f_reltol);
    if (!(o->initial_step >= 0.0) || !std::isfinite(o->initial_step)) return fail(h, EH_EINVAL, "eh_lbfgs_init: initial_step = %g (>= 0; 0 = min(1, 1 / ||g||))", o->initial_step);
    if (h->capturing) return fail(h, EH_EUNSUPPORTED, "eh_lbfgs_init: graph capture is not built for L-BFGS");
    if (h->bnl) return fail(h, EH_EUNSUPPORTED, "eh_lbfgs_init: BatchNorm layers in the chain: the L-BFGS driver carries no layer state (the running statistics would stay at their start)");
    if (h->drop_on) return fail(h, EH_EUNSUPPORTED, "eh_lbfgs_init: dropout: the line search needs the same objective at every trial point, the masks change with every pass (eh_set_dropout with all rates zero removes it)");
    if (h->bn_on) return fail(h, EH_EUNSUPPORTED, "eh_lbfgs_init: input BatchNorm: the reference's Optimization.jl driver never carries the layer state, and that path is not built");
    if (h->comm || h->lgroup || h->p2p_on || h->p2p_alloc) return fail(h, EH_EUNSUPPORTED, "eh_lbfgs_init: data parallelism (a communicator or a peer-to-peer group on this handle) is not built for L-BFGS");
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->net.n_theta;
    if (!h->lb) h->lb = new EhLbfgs();
    EhLbfgs* lb = h->lb;
    lb->active = false;
    if (lb->m_cap < o->m) {
        (void)hipFree(lb->vec); lb->vec = nullptr; lb->m_cap = 0;
        HIPCHK(h, hipMalloc(&lb->vec, (3 + 2 * (size_t)o->m) * n * sizeof(float)));
        lb->m_cap = o->m;
    }
    if (!lb->dbl) HIPCHK(h, hipMalloc(&lb->dbl, (size_t)(EH_LB_DBL_HEAD + EH_LB_PARTS * EH_LB_NQ_MAX) * sizeof(double)));
    if (!lb->trace) HIPCHK(h, hipMalloc(&lb->trace, (size_t)EH_LB_TRACE_ROWS * 8 * sizeof(float)));
    HIPCHK(h, hipMemset(lb->vec, 0, (3 + 2 * (size_t)o->m) * n * sizeof(float)));
    HIPCHK(h, hipMemset(lb->dbl, 0, (size_t)EH_LB_DBL_HEAD * sizeof(double)));
    lb->o = *o; lb->nq = EH_LQ_HIST + 6 * o->m; lb->maxiters = 100;
    lb->batch_set = false; lb->empty = false;
    lb->active = true;
    return EH_OK;
}

int32_t eh_lbfgs_set_maxiters(eh_handle* h, int64_t n) {
    if (!h) return EH_EINVAL;
    if (int rc = lbfgs_ready(h, "eh_lbfgs_set_maxiters")) return rc;
    if (n < 0 || n > INT32_MAX) return fail(h, EH_EINVAL, "eh_lbfgs_set_maxiters: %lld", (long long)n);
    h->lb->maxiters = (int)n;
    if (h->lb->batch_set && !h->lb->empty) {      // a solve that stopped at a lower limit goes on (decided on the device: nothing is read back here)
        HIPCHK(h, hipSetDevice(h->device));
        FLUSH(h);
        hipLaunchKernelGGL(eh_lbfgs_resume_kernel, dim3(1), dim3(256), 0, h->stream, lbfgs_args(h), h->img);
        HIPCHK(h, hipGetLastError());
    }
    return EH_OK;
}

int32_t eh_lbfgs_set_batch(eh_handle* h, int32_t split, const int32_t* idx, int32_t idx_on_device, int64_t first, int64_t count) {
    if (!h) return EH_EINVAL;
    if (int rc = lbfgs_ready(h, "eh_lbfgs_set_batch")) return rc;
    if (split != EH_SPLIT_TRAIN && split != EH_SPLIT_VAL) return fail(h, EH_EINVAL, "eh_lbfgs_set_batch: split %d", split);
    EhLbfgs* lb = h->lb;
    EhSplit& sp = h->split[split];
    if (!sp.recs || sp.n == 0) return fail(h, EH_ESTATE, "eh_lbfgs_set_batch: no data set for this split (call eh_set_data)");
    if (first < 0 || count < 0) return fail(h, EH_EINVAL, "eh_lbfgs_set_batch: first %lld, count %lld", (long long)first, (long long)count);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    lb->batch_set = false;
    if (idx && !idx_on_device) {
        for (int64_t i = 0; i < count; ++i)
            if (idx[first + i] < 0 || idx[first + i] >= sp.samples()) return fail(h, EH_EINVAL, "eh_lbfgs_set_batch: idx[%lld] = %d outside 0..%lld", (long long)(first + i), idx[first + i], sp.samples());
        if (count > lb->idx_cap) {
            (void)hipFree(lb->idx); lb->idx = nullptr; lb->idx_cap = 0;
            HIPCHK(h, hipMalloc(&lb->idx, (size_t)count * sizeof(int)));
            lb->idx_cap = count;
        }
        if (count > 0) HIPCHK(h, hipMemcpy(lb->idx, idx + first, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
        lb->didx = lb->idx; first = 0;
    } else if (idx) lb->didx = idx;
    else {
        if (int rc = eh_check_window(h, sp, first, count, "eh_lbfgs_set_batch")) return rc;
        lb->didx = nullptr;
    }
    lb->split = split; lb->first = first; lb->count = count;
    HIPCHK(h, hipMemset(lb->dbl, 0, (size_t)EH_LB_DBL_HEAD * sizeof(double)));      // a fresh solve: no history, phase 0
    lb->empty = count == 0;
    lb->batch_set = true;
    return EH_OK;
}

int32_t eh_lbfgs_run(eh_handle* h, int64_t n_evals) {
    if (!h) return EH_EINVAL;
    if (int rc = lbfgs_ready(h, "eh_lbfgs_run")) return rc;
    EhLbfgs* lb = h->lb;
    if (!lb->batch_set) return fail(h, EH_ESTATE, "eh_lbfgs_run: call eh_lbfgs_set_batch first");
    if (n_evals < 0) return fail(h, EH_EINVAL, "eh_lbfgs_run: %lld evaluations", (long long)n_evals);
    if (h->drop_on || h->bn_on) return fail(h, EH_EUNSUPPORTED, "eh_lbfgs_run: dropout / input BatchNorm were switched on after eh_lbfgs_init: not built for L-BFGS");
    if (lb->empty) return EH_OK;
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    const int n = h->net.n_theta;
    const EhLbfgsArgs a = lbfgs_args(h);
    const bool one = n <= (h->lb_one_max >= 0 ? h->lb_one_max : (int)EH_LB_ONE_MAX);
    const EhSplit& sp = h->split[lb->split];
    for (int64_t e = 0; e < n_evals; ++e) {
        if (int rc = eh_do_step(h, sp, lb->didx, lb->first, lb->count, false, false, nullptr)) return rc;
        if (one) hipLaunchKernelGGL(eh_lbfgs_one_kernel, dim3(1), dim3(256), 0, h->stream, a, h->img);
        else {
            hipLaunchKernelGGL(eh_lbfgs_dots_kernel, dim3(a.nparts), dim3(256), 0, h->stream, a);
            hipLaunchKernelGGL(eh_lbfgs_decide_kernel, dim3(1), dim3(256), 0, h->stream, a);
            hipLaunchKernelGGL(eh_lbfgs_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, a, h->img);
        }
        HIPCHK(h, hipGetLastError());
    }
    return EH_OK;
}

int32_t eh_lbfgs_status(eh_handle* h, eh_lbfgs_stat* out) {
    if (!h || !out) return EH_EINVAL;
    if (int rc = lbfgs_ready(h, "eh_lbfgs_status")) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double st[EH_LBFGS_STATE_DOUBLES];
    HIPCHK(h, hipMemcpy(st, h->lb->dbl, sizeof st, hipMemcpyDeviceToHost));
    out->iterations = (int64_t)st[EH_LS_ITERS]; out->evaluations = (int64_t)st[EH_LS_EVALS];
    out->f0 = st[EH_LS_F0]; out->g_inf = st[EH_LS_GINF0]; out->last_t = st[EH_LS_LAST_T];
    out->pairs = (int32_t)st[EH_LS_NPAIRS];
    out->code = h->lb->empty ? (int32_t)EH_LBFGS_EMPTY_BATCH : (int32_t)st[EH_LS_DONE];
    return EH_OK;
}

int32_t eh_lbfgs_trace(eh_handle* h, float* out, int64_t max_rows, int64_t* n_rows) {
    if (!h || !n_rows || (max_rows > 0 && !out)) return EH_EINVAL;
    if (int rc = lbfgs_ready(h, "eh_lbfgs_trace")) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double rows = 0.0;
    HIPCHK(h, hipMemcpy(&rows, h->lb->dbl + EH_LS_ROWS, sizeof rows, hipMemcpyDeviceToHost));
    *n_rows = (int64_t)rows;
    const int64_t k = std::min<int64_t>(std::min<int64_t>((int64_t)rows, max_rows), (int64_t)EH_LB_TRACE_ROWS);
    if (k > 0) HIPCHK(h, hipMemcpy(out, h->lb->trace, (size_t)k * 8 * sizeof(float), hipMemcpyDeviceToHost));
    return EH_OK;
}

int32_t eh_lbfgs_host_decide(const eh_lbfgs_opts* o, int32_t maxiters, double* state, double* gram, const double* sums, double f, double n_valid,
                             double* record, double* trace_row, int32_t* wrote_row) {
    if (!o || !state || !gram || !sums || !record || !trace_row) return EH_EINVAL;
    if (o->m < 1 || o->m > EH_LBFGS_MAX_M || o->max_linesearch < 1 || o->max_linesearch > 48) return EH_EINVAL;
    const int w = eh_lb_decide(*o, maxiters, state, gram, sums, f, n_valid, record, trace_row);
    if (wrote_row) *wrote_row = w;
    return EH_OK;
}

}   // extern "C"
