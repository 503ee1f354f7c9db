// Ensembles: M models of one handle's architecture -- cross-validation folds, a sweep over optimiser settings, repeated seeds -- trained
// by ONE launch per chunk of an epoch, a workgroup per member (eh_ens.hpp).  This unit is host code: the members'
// state, their row lists, the records a launch reads, evaluation and the hand-over to and from the handle.  The kernels it launches
// live where their like live (the step kernels' units, eh_kernels.hpp) and are reached through the seam in eh_internal.hpp.
#include "eh_internal.hpp"

#include <algorithm>
#include <cmath>

struct eh_ensemble_s {
    eh_handle* h = nullptr;
    int M = 0;
    long long batch = 0;
    // per member, `*_f` floats apart: parameter sets + beta products | gradient accumulators | parameter image | BatchNorm running statistics
    size_t pset_f = 0, gacc_f = 0, img_f = 0;
    float *pset = nullptr, *gacc = nullptr, *image = nullptr, *bn_run = nullptr;
    struct Member {
        int cur = 0, sc_sel = 0;
        long long gstep = 0;            // launches that trained the member: its accumulator slot is gstep % 3, as the handle's
        EhOpt opt{};
        bool opt_set = false;
        int* rows[2] = {nullptr, nullptr};      // device row lists (train | evaluation); nullptr with all[k]: every row of the table
        long long n[2] = {0, 0};
        bool all[2] = {true, true};
    };
    std::vector<Member> mem;
    int* order = nullptr; long long order_cap = 0;        // the epoch orders of all members, one behind the other
    float* loss = nullptr; long long loss_cap = 0;        // the per-step losses of all members, one behind the other
    // what a launch reads: [chunks][M] member records, then M order records -- staged in pinned memory, copied on the stream
    char *rec_host = nullptr, *rec_dev = nullptr; size_t rec_cap = 0;
    hipEvent_t rec_ev = nullptr; bool rec_busy = false;
    bool failed = false;            // a chunk of an epoch could not be launched behind others that were: the members' state is unknown
    float *eval_host = nullptr, *eval_dev = nullptr; size_t eval_cap = 0;      // pinned, device-visible: every member's per-workgroup metric sums
    float* member_pset(int j) const { return pset + (size_t)j * pset_f; }
    float* th(int j) const { return member_pset(j) + (size_t)mem[j].cur * 3 * h->net.n_theta; }
    float* sc(int j) const { return member_pset(j) + (size_t)6 * h->net.n_theta; }
    long long rows_of(int j, int which) const { return mem[j].all[which] ? h->split[EH_SPLIT_TRAIN].n : mem[j].n[which]; }
};

namespace {
int member_check(eh_ensemble* e, int32_t j, const char* who) {
    if (j < 0 || j >= e->M) return fail(e->h, EH_EINVAL, "%s: member %d of %d", who, j, e->M);
    HIPCHK(e->h, hipSetDevice(e->h->device));
    return EH_OK;
}
// a device buffer the stream may still be reading grows (capacities in elements)
template <class T>
int grow(eh_handle* h, T** buf, long long* cap, long long need) {
    if (need <= *cap) return EH_OK;
    return eh_grow(h, buf, cap, need);
}
// eh_set_data, eh_set_option and eh_opt_init* are closed while an ensemble exists; the other entry points that can move the handle out of
// what eh_ens_create checked (a two-pass or recorded loss, dropout, a communicator, a capture ...) are not, so every launch asks again
int still_eligible(eh_ensemble* e, const char* who) {
    if (e->failed) return fail(e->h, EH_ESTATE, "%s: a launch of an earlier epoch failed half way, the members' state is unknown (set it again through eh_ens_destroy / eh_ens_create)", who);
    const std::string why = eh_ens_refusal(e->h, e->batch);
    if (why.empty()) return EH_OK;
    return fail(e->h, EH_ESTATE, "%s: the handle has left the configuration its ensemble was created in.  %s", who, why.c_str());
}
}   // namespace

extern "C" {

int32_t eh_ens_create(eh_handle* h, int32_t members, int64_t batchsize, eh_ensemble** out) {
    if (!h || !out) return EH_EINVAL;
    *out = nullptr;
    if (members < 1 || members > EH_ENS_MAX_MEMBERS) return fail(h, EH_EINVAL, "eh_ens_create: %d members (1 .. %d)", members, EH_ENS_MAX_MEMBERS);
    if (batchsize < 1) return fail(h, EH_EINVAL, "eh_ens_create: batchsize %lld", (long long)batchsize);
    HIPCHK(h, hipSetDevice(h->device));
    const std::string why = eh_ens_refusal(h, batchsize);
    if (!why.empty()) return fail(h, EH_EUNSUPPORTED, "eh_ens_create: an ensemble trains every member as the multi-step launch of one workgroup, which this handle does not run.  %s", why.c_str());
    const EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    if (!sp.recs || sp.n == 0) return fail(h, EH_ESTATE, "eh_ens_create: no training data (the members' row lists index the TRAIN table: call eh_set_data first)");
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::unique_ptr<eh_ensemble_s> e(new eh_ensemble_s());
    e->h = h; e->M = members; e->batch = batchsize;
    const size_t nt = (size_t)h->net.n_theta;
    e->pset_f = (6 * nt + 4 + 3) & ~(size_t)3;
    e->gacc_f = ((size_t)3 * EH_GSHARDS * h->n_acc + 4 + 3) & ~(size_t)3;
    e->img_f = ((size_t)h->arch->img_floats + 3) & ~(size_t)3;
    e->mem.resize((size_t)members);
    auto release = [&]() { (void)hipFree(e->pset); (void)hipFree(e->gacc); (void)hipFree(e->image); (void)hipFree(e->bn_run); if (e->rec_ev) (void)hipEventDestroy(e->rec_ev); };
#define HIPCHK_E(expr)                                                                                                           \
    do {                                                                                                                         \
        hipError_t e_ = (expr);                                                                                                  \
        if (e_ != hipSuccess) { release(); return fail(h, e_ == hipErrorOutOfMemory ? EH_ENOMEM : EH_EHIP, "eh_ens_create: %s: %s", #expr, hipGetErrorString(e_)); } \
    } while (0)
    HIPCHK_E(hipMalloc(&e->pset, (size_t)members * e->pset_f * sizeof(float)));
    HIPCHK_E(hipMalloc(&e->gacc, (size_t)members * e->gacc_f * sizeof(float)));
    HIPCHK_E(hipMalloc(&e->image, (size_t)members * e->img_f * sizeof(float)));
    HIPCHK_E(hipMalloc(&e->bn_run, (size_t)members * 64 * sizeof(float)));
    HIPCHK_E(hipEventCreateWithFlags(&e->rec_ev, hipEventDisableTiming));
    // every member starts as the handle stands: its parameters, its optimiser state and rule, its image (the constant parts among them)
    HIPCHK_E(hipMemset(e->bn_run, 0, (size_t)members * 64 * sizeof(float)));
    for (int j = 0; j < members; ++j) {
        HIPCHK_E(hipMemcpy(e->member_pset(j), h->pset, (6 * nt + 4) * sizeof(float), hipMemcpyDeviceToDevice));
        HIPCHK_E(hipMemcpy(e->gacc + (size_t)j * e->gacc_f, h->gacc, ((size_t)3 * EH_GSHARDS * h->n_acc + 4) * sizeof(float), hipMemcpyDeviceToDevice));
        HIPCHK_E(hipMemcpy(e->image + (size_t)j * e->img_f, h->image, (size_t)h->arch->img_floats * sizeof(float), hipMemcpyDeviceToDevice));
        if (h->bn_on) HIPCHK_E(hipMemcpy(e->bn_run + (size_t)j * 64, h->bn_run, 64 * sizeof(float), hipMemcpyDeviceToDevice));
        eh_ensemble_s::Member& m = e->mem[(size_t)j];
        m.cur = h->cur; m.sc_sel = h->sc_sel; m.gstep = h->gstep;
        m.opt = h->opt; m.opt.tab = nullptr;
        m.opt_set = h->opt_ready && h->opt.tab == nullptr;
    }
#undef HIPCHK_E
    ++h->ens_live;
    *out = e.release();
    return EH_OK;
}

int32_t eh_ens_destroy(eh_ensemble* e) {
    if (!e) return EH_OK;
    eh_handle* h = e->h;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (auto& m : e->mem) { (void)hipFree(m.rows[0]); (void)hipFree(m.rows[1]); }
    (void)hipFree(e->pset); (void)hipFree(e->gacc); (void)hipFree(e->image); (void)hipFree(e->bn_run);
    (void)hipFree(e->order); (void)hipFree(e->loss); (void)hipFree(e->rec_dev);
    if (e->rec_host) (void)hipHostFree(e->rec_host);
    if (e->eval_host) (void)hipHostFree(e->eval_host);
    if (e->rec_ev) (void)hipEventDestroy(e->rec_ev);
    --h->ens_live;
    delete e;
    return EH_OK;
}

int32_t eh_ens_set_params(eh_ensemble* e, int32_t j, const float* theta, int64_t n) {
    if (!e || !theta) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_set_params")) return rc;
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_ens_set_params: n = %lld, model has %d", (long long)n, h->net.n_theta);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(e->th(j), theta, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = eh_ens_launch_image(h, e->th(j), e->image + (size_t)j * e->img_f)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EH_OK;
}

int32_t eh_ens_get_params(eh_ensemble* e, int32_t j, float* theta, int64_t n) {
    if (!e || !theta) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_get_params")) return rc;
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_ens_get_params: n = %lld, model has %d", (long long)n, h->net.n_theta);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(theta, e->th(j), (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return EH_OK;
}

int32_t eh_ens_set_opt(eh_ensemble* e, int32_t j, int32_t rule, float lr, float beta1, float beta2, float eps, float weight_decay) {
    if (!e) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_set_opt")) return rc;
    if (rule < EH_OPT_ADAM || rule > EH_OPT_DESCENT) return fail(h, EH_EUNSUPPORTED, "eh_ens_set_opt: unknown rule %d (one of the four rules per member; per-branch tables and chains are not built for ensembles)", rule);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t nt = (size_t)h->net.n_theta;
    eh_ensemble_s::Member& m = e->mem[(size_t)j];
    HIPCHK(h, hipMemset(e->th(j) + nt, 0, 2 * nt * sizeof(float)));      // a new rule: zero moments, the running beta products at their start (as eh_opt_init)
    const float sc[4] = {beta1, beta2, beta1, beta2};
    HIPCHK(h, hipMemcpy(e->sc(j), sc, sizeof sc, hipMemcpyHostToDevice));
    m.sc_sel = 0;
    m.opt = EhOpt{rule, lr, beta1, beta2, eps, weight_decay, nullptr};
    m.opt_set = true;
    return EH_OK;
}

int32_t eh_ens_get_opt_state(eh_ensemble* e, int32_t j, float* mo, float* v, int64_t n, float* beta_t) {
    if (!e) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_get_opt_state")) return rc;
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_ens_get_opt_state: n");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (mo) HIPCHK(h, hipMemcpy(mo, e->th(j) + n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (v) HIPCHK(h, hipMemcpy(v, e->th(j) + 2 * n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (beta_t) HIPCHK(h, hipMemcpy(beta_t, e->sc(j) + 2 * e->mem[(size_t)j].sc_sel, 2 * sizeof(float), hipMemcpyDeviceToHost));
    return EH_OK;
}

int32_t eh_ens_set_opt_state(eh_ensemble* e, int32_t j, const float* mo, const float* v, int64_t n, const float* beta_t) {
    if (!e) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_set_opt_state")) return rc;
    if (!e->mem[(size_t)j].opt_set) return fail(h, EH_ESTATE, "eh_ens_set_opt_state: call eh_ens_set_opt for member %d first", j);
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_ens_set_opt_state: n");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (mo) HIPCHK(h, hipMemcpy(e->th(j) + n, mo, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (v) HIPCHK(h, hipMemcpy(e->th(j) + 2 * n, v, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (beta_t) HIPCHK(h, hipMemcpy(e->sc(j) + 2 * e->mem[(size_t)j].sc_sel, beta_t, 2 * sizeof(float), hipMemcpyHostToDevice));
    return EH_OK;
}

int32_t eh_ens_get_bn_state(eh_ensemble* e, int32_t j, float* running_mean, float* running_var, int64_t n) {
    if (!e || !running_mean || !running_var) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_get_bn_state")) return rc;
    if (!h->bn_on) return fail(h, EH_ESTATE, "eh_ens_get_bn_state: the model has no input BatchNorm");
    if (n != h->net.P) return fail(h, EH_EINVAL, "eh_ens_get_bn_state: n = %lld, model has %d predictors", (long long)n, h->net.P);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(running_mean, e->bn_run + (size_t)j * 64, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(running_var, e->bn_run + (size_t)j * 64 + 32, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return EH_OK;
}

int32_t eh_ens_set_bn_state(eh_ensemble* e, int32_t j, const float* running_mean, const float* running_var, int64_t n) {
    if (!e || !running_mean || !running_var) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_set_bn_state")) return rc;
    if (!h->bn_on) return fail(h, EH_ESTATE, "eh_ens_set_bn_state: the model has no input BatchNorm");
    if (n != h->net.P) return fail(h, EH_EINVAL, "eh_ens_set_bn_state: n = %lld, model has %d predictors", (long long)n, h->net.P);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<float> rstd((size_t)n);
    for (int64_t p = 0; p < n; ++p) rstd[(size_t)p] = 1.0f / std::sqrt(running_var[p] + EH_BN_EPS);
    float* const run = e->bn_run + (size_t)j * 64;
    float* const img = e->image + (size_t)j * e->img_f + h->arch->phi_off;
    HIPCHK(h, hipMemcpy(run, running_mean, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(run + 32, running_var, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(img + EH_IMG_BNM, running_mean, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(img + EH_IMG_BNR, rstd.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return EH_OK;
}

int32_t eh_ens_set_rows(eh_ensemble* e, int32_t j, int32_t which, const int32_t* rows, int64_t n) {
    if (!e) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_set_rows")) return rc;
    if (which != 0 && which != 1) return fail(h, EH_EINVAL, "eh_ens_set_rows: which = %d (0: training rows, 1: evaluation rows)", which);
    const long long N = h->split[EH_SPLIT_TRAIN].n;
    if (rows && (n < 0 || n > 0x7fffffffLL)) return fail(h, EH_EINVAL, "eh_ens_set_rows: n = %lld", (long long)n);
    if (rows)
        for (int64_t i = 0; i < n; ++i)
            if (rows[i] < 0 || rows[i] >= N) return fail(h, EH_EINVAL, "eh_ens_set_rows: rows[%lld] = %d outside 0..%lld", (long long)i, rows[i], N - 1);
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (a launch in flight may be reading the list it replaces)
    eh_ensemble_s::Member& m = e->mem[(size_t)j];
    (void)hipFree(m.rows[which]);
    m.rows[which] = nullptr; m.n[which] = 0; m.all[which] = rows == nullptr;
    if (rows && n > 0) {
        HIPCHK(h, hipMalloc(&m.rows[which], (size_t)n * sizeof(int)));
        HIPCHK(h, hipMemcpy(m.rows[which], rows, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        m.n[which] = n;
    }
    return EH_OK;
}

int32_t eh_ens_train_epoch(eh_ensemble* e, const uint64_t* seed, int32_t shuffle, const uint8_t* active, float* mean_loss, int64_t* n_steps) {
    if (!e) return EH_EINVAL;
    eh_handle* h = e->h;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = still_eligible(e, "eh_ens_train_epoch")) return rc;
    const int M = e->M;
    const long long B = e->batch;
    const EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    // rows, steps and where each member's share of the order and loss buffers starts
    std::vector<long long> nrow((size_t)M), steps((size_t)M), ooff((size_t)M), loff((size_t)M);
    long long osum = 0, lsum = 0, smax = 0, nmax = 0;
    for (int j = 0; j < M; ++j) {
        const bool on = !active || active[j];
        if (on && !e->mem[(size_t)j].opt_set) return fail(h, EH_ESTATE, "eh_ens_train_epoch: member %d has no optimiser (eh_ens_set_opt, or eh_opt_init on the handle before eh_ens_create)", j);
        nrow[(size_t)j] = on ? e->rows_of(j, 0) : 0;
        steps[(size_t)j] = (nrow[(size_t)j] + B - 1) / B;
        ooff[(size_t)j] = osum; loff[(size_t)j] = lsum;
        if (shuffle) osum += nrow[(size_t)j];
        lsum += steps[(size_t)j];
        smax = std::max(smax, steps[(size_t)j]); nmax = std::max(nmax, nrow[(size_t)j]);
    }
    if (n_steps) for (int j = 0; j < M; ++j) n_steps[j] = steps[(size_t)j];
    const double nan = std::nan("");
    if (smax == 0) { if (mean_loss) for (int j = 0; j < M; ++j) mean_loss[j] = (float)nan; return EH_OK; }
    if (int rc = grow(h, &e->order, &e->order_cap, osum)) return rc;
    if (int rc = grow(h, &e->loss, &e->loss_cap, lsum)) return rc;
    const int chunks = (int)((smax + EH_MULTI_MAX - 1) / EH_MULTI_MAX);
    const size_t rec_bytes = (size_t)chunks * M * sizeof(EhEnsMember), ord_bytes = (size_t)M * sizeof(EhEnsOrder);
    if (rec_bytes + ord_bytes > e->rec_cap) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (e->rec_host) (void)hipHostFree(e->rec_host);
        (void)hipFree(e->rec_dev);
        e->rec_host = nullptr; e->rec_dev = nullptr; e->rec_cap = 0; e->rec_busy = false;
        HIPCHK(h, hipHostMalloc((void**)&e->rec_host, rec_bytes + ord_bytes, hipHostMallocDefault));
        HIPCHK(h, hipMalloc(&e->rec_dev, rec_bytes + ord_bytes));
        e->rec_cap = rec_bytes + ord_bytes;
    }
    // (the staging copy of the epoch before has long been read: this wait returns at once, and is no wait for the kernels behind that copy)
    if (e->rec_busy) { HIPCHK(h, hipEventSynchronize(e->rec_ev)); e->rec_busy = false; }
    EhEnsMember* const rec = reinterpret_cast<EhEnsMember*>(e->rec_host);
    EhEnsOrder* const ord = reinterpret_cast<EhEnsOrder*>(e->rec_host + rec_bytes);
    int n_ord = 0;
    struct Rot { int cur, sc_sel; long long gstep; };
    std::vector<Rot> rot((size_t)M);          // the members' rotation state as the launches leave it: taken over once all of them are queued
    for (int j = 0; j < M; ++j) {
        const eh_ensemble_s::Member& m = e->mem[(size_t)j];
        Rot& q = rot[(size_t)j];
        q = Rot{m.cur, m.sc_sel, m.gstep};
        const long long n = nrow[(size_t)j];
        const int* idx = m.rows[0];                  // unshuffled: the list as given (nullptr: the table's own order)
        if (shuffle && n > 0) {
            int bits = 1;
            while ((1LL << bits) < n) ++bits;
            ord[n_ord++] = EhEnsOrder{m.rows[0], e->order + ooff[(size_t)j], seed ? (unsigned long long)seed[j] : 0ull, (unsigned)n, std::max(1, (bits + 1) / 2)};
            idx = e->order + ooff[(size_t)j];
        }
        for (int c = 0; c < chunks; ++c) {
            const long long done = (long long)c * EH_MULTI_MAX;
            const int nst = (int)std::max<long long>(0, std::min<long long>(EH_MULTI_MAX, steps[(size_t)j] - done));
            EhEnsMember& r = rec[(size_t)c * M + j];
            r = EhEnsMember{};
            r.pset = e->member_pset(j); r.gacc = e->gacc + (size_t)j * e->gacc_f; r.image = e->image + (size_t)j * e->img_f; r.bn_run = e->bn_run + (size_t)j * 64;
            r.idx = idx; r.ms_loss = e->loss + loff[(size_t)j] + done;
            r.first = done * B; r.ms_end = n; r.nsteps = nst;
            r.gslot = (int)(q.gstep % 3); r.cur = q.cur; r.sc_sel = q.sc_sel; r.pending = 0;
            r.rule = m.opt.rule; r.lr = m.opt.lr; r.b1 = m.opt.b1; r.b2 = m.opt.b2; r.eps = m.opt.eps; r.wd = m.opt.wd;
            // what the launch leaves behind, per member: its first step's prologue flipped the parameter set and rotated the accumulator slots
            // once -- a member without steps in the launch stays as it is
            if (nst > 0) { q.cur ^= 1; q.sc_sel ^= 1; q.gstep += 1; }
        }
    }
    HIPCHK(h, hipMemcpyAsync(e->rec_dev, e->rec_host, rec_bytes + ord_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(e->rec_ev, h->stream));
    e->rec_busy = true;
    if (n_ord) { if (int rc = eh_ens_launch_order(h, reinterpret_cast<const EhEnsOrder*>(e->rec_dev + rec_bytes), n_ord, nmax)) return rc; }
    // the arguments every member shares: do_fused_multi's, with the member's own fields left to its record
    EhStepArgs a = eh_step_args(h, sp, nullptr, 0, B);
    a.image = nullptr; a.slab = h->slab; a.n_acc = h->n_acc; a.inv_n = nullptr; a.rmap = h->rmap; a.stamps = nullptr;
    a.fz.imap = h->imap; a.fz.agg_a = h->img.agg_a;
    if (int rc = eh_bn_prepare(h, sp, nullptr, 0, B, true, &a)) return rc;
    a.bn_run = nullptr; a.image_out = nullptr;
    a.ms_batch = (int)B;
    for (int c = 0; c < chunks; ++c)
        if (int rc = eh_ens_launch_train(h, M, &a, reinterpret_cast<const EhEnsMember*>(e->rec_dev) + (size_t)c * M)) {
            // chunks 0 .. c-1 are queued and will run, this one and the later ones will not: the host's picture of the members' state would be
            // wrong either way, so the ensemble takes no further launches
            e->failed = true;
            return rc;
        }
    for (int j = 0; j < M; ++j) { eh_ensemble_s::Member& m = e->mem[(size_t)j]; m.cur = rot[(size_t)j].cur; m.sc_sel = rot[(size_t)j].sc_sel; m.gstep = rot[(size_t)j].gstep; }
    if (mean_loss) {
        std::vector<float> l((size_t)lsum);
        HIPCHK(h, hipMemcpyAsync(l.data(), e->loss, l.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int j = 0; j < M; ++j) {
            double sum = 0; long long cnt = 0;
            for (long long s = 0; s < steps[(size_t)j]; ++s) { const float x = l[(size_t)(loff[(size_t)j] + s)]; if (!std::isnan(x)) { sum += x; ++cnt; } }
            mean_loss[j] = cnt ? (float)(sum / cnt) : (float)nan;
        }
    }
    return EH_OK;
}

int32_t eh_ens_eval(eh_ensemble* e, int32_t which, eh_target_metrics* out) {
    if (!e || !out) return EH_EINVAL;
    eh_handle* h = e->h;
    if (which != 0 && which != 1) return fail(h, EH_EINVAL, "eh_ens_eval: which = %d (0: training rows, 1: evaluation rows)", which);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = still_eligible(e, "eh_ens_eval")) return rc;
    const int M = e->M, T = h->net.T, nst = EH_EVAL_STATS * T;
    const EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    // the existing evaluation kernels, one queued launch per member on its image and row list; every workgroup stores its sums straight into
    // one pinned buffer, read behind ONE synchronisation
    std::vector<int> grid((size_t)M);
    std::vector<size_t> off((size_t)M);
    size_t rows = 0;
    for (int j = 0; j < M; ++j) { grid[(size_t)j] = e->rows_of(j, which) > 0 ? eh_ens_eval_grid(h, e->rows_of(j, which)) : 0; off[(size_t)j] = rows; rows += (size_t)grid[(size_t)j]; }
    if (rows * nst > e->eval_cap) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (e->eval_host) (void)hipHostFree(e->eval_host);
        e->eval_host = nullptr; e->eval_dev = nullptr; e->eval_cap = 0;
        HIPCHK(h, hipHostMalloc((void**)&e->eval_host, rows * nst * sizeof(float), hipHostMallocMapped));
        HIPCHK(h, hipHostGetDevicePointer((void**)&e->eval_dev, e->eval_host, 0));
        e->eval_cap = rows * nst;
    }
    for (int j = 0; j < M; ++j) {
        if (!grid[(size_t)j]) continue;
        const long long n = e->rows_of(j, which);
        EhStepArgs a = eh_step_args(h, sp, e->mem[(size_t)j].rows[which], 0, n);
        a.image = e->image + (size_t)j * e->img_f; a.slab = e->eval_dev + off[(size_t)j] * nst; a.n_acc = nst; a.yld = n;
        if (int rc = eh_ens_launch_eval(h, &a, grid[(size_t)j])) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int j = 0; j < M; ++j) {
        double st[EH_MAX_TARG * EH_EVAL_STATS] = {0};
        for (int k = 0; k < nst; ++k) {
            double s = 0;
            for (int b = 0; b < grid[(size_t)j]; ++b) s += e->eval_host[(off[(size_t)j] + (size_t)b) * nst + k];
            st[k] = s;
        }
        eh_metrics_from_sums(st, sp.shift, T, out + (size_t)j * T);
    }
    return EH_OK;
}

int32_t eh_ens_load(eh_ensemble* e, int32_t j) {
    if (!e) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_load")) return rc;
    FLUSH(h);
    const eh_ensemble_s::Member& m = e->mem[(size_t)j];
    const size_t nt = (size_t)h->net.n_theta;
    HIPCHK(h, hipMemcpyAsync(h->pset, e->member_pset(j), (6 * nt + 4) * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->gacc, e->gacc + (size_t)j * e->gacc_f, ((size_t)3 * EH_GSHARDS * h->n_acc + 4) * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->image, e->image + (size_t)j * e->img_f, (size_t)h->arch->img_floats * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (h->bn_on) HIPCHK(h, hipMemcpyAsync(h->bn_run, e->bn_run + (size_t)j * 64, 64 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    h->cur = m.cur; h->sc_sel = m.sc_sel; h->gstep = m.gstep;
    h->pending = false; h->pend_ord = false; h->pending_loss = nullptr;
    if (m.opt_set) { h->opt = m.opt; h->opt_groups = 1; h->opt_ready = true; }
    eh_opt_changed(h);
    return EH_OK;
}

int32_t eh_ens_store(eh_ensemble* e, int32_t j) {
    if (!e) return EH_EINVAL;
    eh_handle* h = e->h;
    if (int rc = member_check(e, j, "eh_ens_store")) return rc;
    if (h->opt.tab) return fail(h, EH_ESTATE, "eh_ens_store: the handle holds per-branch optimiser rules, a member one rule");
    FLUSH(h);
    eh_ensemble_s::Member& m = e->mem[(size_t)j];
    const size_t nt = (size_t)h->net.n_theta;
    HIPCHK(h, hipMemcpyAsync(e->member_pset(j), h->pset, (6 * nt + 4) * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(e->gacc + (size_t)j * e->gacc_f, h->gacc, ((size_t)3 * EH_GSHARDS * h->n_acc + 4) * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(e->image + (size_t)j * e->img_f, h->image, (size_t)h->arch->img_floats * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (h->bn_on) HIPCHK(h, hipMemcpyAsync(e->bn_run + (size_t)j * 64, h->bn_run, 64 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    m.cur = h->cur; m.sc_sel = h->sc_sel; m.gstep = h->gstep;
    if (h->opt_ready) { m.opt = h->opt; m.opt_set = true; }
    return EH_OK;
}

}   // extern "C"
