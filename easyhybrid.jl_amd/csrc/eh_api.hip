// C ABI of libeasyhybrid_hip.so (declared in include/easyhybrid_hip.h): model, parameters, forward / eval, the training step and
// epoch, the optimiser, graphs, the data-parallel seam eh_dp_*.  The small kernels live in eh_kernels.hpp, the handle and the map of
// the other units (data upload, layer-wise form, L-BFGS, mechanistic stage, sequence kernels, collectives) in eh_internal.hpp.
// Everything here runs on one HIP stream per handle; there is no CPU compute path.
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <cfloat>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "eh_internal.hpp"
#include "eh_kernels.hpp"
#include "eh_chain.hpp"
#include "eh_lbfgs.hpp"
#include "eh_wide.hpp"
#include "eh_seq.hpp"

std::string g_create_err;

int fail(eh_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_err = buf;
    return code;
}

static unsigned two_pass_mask(const EhNet& net);

// ---- fused-update mode: apply the pending gradient so theta / m / v / image are current -----------
static int flush_one(eh_handle* h);
int flush_pending(eh_handle* h) {
    if (!h->pending) return EH_OK;
    // Publishing mode 1: a step's sums reach the peers from the NEXT kernel on each rank's stream -- the next step or this flush -- so a
    // drain is collective: the flush kernel waits for words that only the peers' own next kernels store.  Members of a one-process
    // local group are drained together here, all launches before anybody synchronises (advisor r05: eh_get_params / eh_eval / a loss
    // read / eh_set_option on ONE member used to run into the 2 s deadline and apply the step with the peers' sums read as 0).  Rank
    // processes cannot be reached from here: there every draining call has to be made on all ranks (dp.py).
    if (h->p2p_on && h->p2p_local && h->p2p_host.mode == 1) {
        for (int r = 0; r < h->p2p_world; ++r) {
            eh_handle* g = h->p2p_group[r];
            if (!g || g == h || !g->pending) continue;
            HIPCHK(g, hipSetDevice(g->device));
            if (int rc = flush_one(g)) return rc;
        }
        HIPCHK(h, hipSetDevice(h->device));
    }
    return flush_one(h);
}
static EhOrd ord_args(const eh_handle* h, int slot, int prev_grid) {
    EhOrd o{};
    o.cnt = h->ord;
    o.rows = reinterpret_cast<float*>(h->ord + 32 * EH_ORD_GROUPS);
    o.grows = o.rows + (size_t)2 * EH_ORD_ROWS * h->ord_rs;
    o.err = h->ord_err;
    o.rs = h->ord_rs; o.soff = h->ord_soff; o.slot = slot; o.prev_grid = prev_grid;
    return o;
}
static int flush_done(eh_handle* h) {      // the update is applied: the beta products advance, nothing is pending
    h->sc_sel ^= 1;
    h->pending = false;
    h->pend_ord = false;
    h->pending_loss = nullptr;
    return EH_OK;
}
static int flush_one(eh_handle* h) {
    const int nt = h->net.n_theta;
    if (h->pend_ord) {        // an ordered step's sums: its rows and group rows (the step wrote slot h->cur ^ 1, which is what slot h->cur reads)
        // (a workgroup per row of the step at least: each resets the rows it takes, the first ceil(nt / 256) also apply the update)
        hipLaunchKernelGGL(eh_ord_flush_kernel, dim3(std::max((nt + 255) / 256, h->ord_grid)), dim3(256), 0, h->stream, ord_args(h, h->cur, h->ord_grid), nt, TH(h), MM(h), VV(h),
                           h->sc + 2 * h->sc_sel, h->sc + 2 * (h->sc_sel ^ 1), h->opt, h->pending_loss, h->img, h->net.loss);
        HIPCHK(h, hipGetLastError());
        ++h->upd_site[EH_UPD_ORD_FLUSH];
        return flush_done(h);
    }
    const float* g_prev = h->gacc + (size_t)((h->gstep + 2) % 3) * EH_GSHARDS * h->n_acc;
    float* sc_in = h->sc + 2 * h->sc_sel;
    float* sc_out = h->sc + 2 * (h->sc_sel ^ 1);
    hipLaunchKernelGGL(eh_fused_flush_kernel, dim3((nt + 255) / 256), dim3(256), 0, h->stream, g_prev, h->n_acc, nt, TH(h), MM(h), VV(h), sc_in, sc_out,
                       h->opt, h->pending_loss, h->img, h->net.loss, h->p2p_on ? h->p2p_dev : nullptr, (int)((h->gstep + 2) % 3), h->p2p_seq, h->net.T);
    HIPCHK(h, hipGetLastError());
    ++h->upd_site[EH_UPD_FUSED_FLUSH];
    // Single GPU: nothing to clear -- the rotation keeps itself clean (the step that accumulates into slot g clears slot g + 1 in
    // its prologue and nobody reads a slot before the step after its clearing has filled it).  Under EhP2P the workgroups add
    // into a staging copy that the publishing workgroup reads whole: cleared here.
    if (h->p2p_on) HIPCHK(h, hipMemsetAsync(h->p2p_stage, 0, (size_t)3 * EH_GSHARDS * h->n_acc * sizeof(float), h->stream));
    return flush_done(h);
}
// Every trainable scalar of the model as (canonical flat index, layer, row, col) in the padded
// block-diagonal MLP.  col < 0 marks a bias.  SingleNN = one net covering everything.
struct EhEntry { int canon, l, row, col; };
static std::vector<EhEntry> enumerate_entries(const EhPlan& p) {      // (fused families: every leaf is a Dense weight or bias)
    std::vector<EhEntry> v;
    const int nl = p.desc.n_hidden;
    for (const EhLeaf& f : p.leaves) {
        const int k = f.net, l = f.layer < p.net_d[k] ? f.layer : nl;      // (the output layer of a shallower net sits behind its identity blocks)
        const int r0 = p.net_r0[k][l], c0 = l == 0 ? p.net_c0[k] : p.net_r0[k][l - 1];
        for (int col = 0; col < std::max(f.cols, 1); ++col)
            for (int row = 0; row < f.rows; ++row) v.push_back({f.off + row + f.rows * col, l, r0 + row, f.kind == EH_LEAF_WEIGHT ? c0 + col : -1});
    }
    return v;
}

// canonical index -> parameter-image offset; canonical index <-> accumulator element of the step
// kernel (rmap: where the element sits among the parked accumulators; see eh_acc_layout)
static int build_maps(eh_handle* h, bool with_imap) {
    const eh_model_desc& d = h->desc;
    const EhNet& n = h->net;
    const EhArchInfo* A = h->arch;
    const int nbi = A->nbi, nbh = A->nbh, nl = A->nl, fast = h->fast;
    const EhAccLayout L = eh_acc_layout(nbi, nbh, nl, fast);
    const std::vector<EhEntry> ent = enumerate_entries(h->plan);
    const int nwv = A->wide ? A->var[h->variant].nw : 4;
    const EhWideLayout WL = eh_wide_layout(nbi, nbh, nl, nwv);
    std::vector<int> imap((size_t)n.n_theta, -1), rmap((size_t)h->n_acc, 0);
    // v2 region[k][g][r][c] where one wave workspace holds a wave's raw accumulators, else v3 region[k][c][g][r] (eh_step_body, workgroup reduction)
    const bool v2 = A->wide || L.rw <= A->var[h->variant].red_floats / A->var[h->variant].nw;
    // (v2, an element that is a sum over the 16 samples of a row -- nlan == 16 below: its entry is the position of the row's FIRST column,
    //  lane & 15 == 0, i.e. k * 256 + row * 16 with row = 4 g + r.  The kernel parks such a row as ONE word at k * 256 + row and derives
    //  that word from the entry, (pos & ~255) | ((pos & 255) >> 4) -- eh_step_body, put_rows and the gather; EH_AB_REDUCE_PARENT reads
    //  the 16 columns at the entry itself.  nlan is 1 or 16, nothing else; the check below holds both to that.)
    auto at = [v2](int k, int lane, int r) { return v2 ? k * 256 + (lane >> 4) * 64 + r * 16 + (lane & 15) : k * 256 + (lane & 15) * 16 + (lane >> 4) * 4 + r; };
    for (const EhEntry& e : ent) {
        const int m = e.row / 16, g = (e.row % 16) / 4, r = e.row % 4;
        int img, k, lane, rr, nlan;
        if (e.col < 0) {                                   // bias of layer l
            img = A->b_off + e.l * A->hp + e.row;
            if (e.l < nl) { k = L.kb + e.l * nbh + m; lane = 16 * g; rr = r; nlan = 16; }
            else if (fast & 1) { k = -1; lane = 0; rr = 0; nlan = 1; }          // K1: scalar in the tail
            else { k = L.kbo; lane = 16 * (e.row / 4); rr = e.row % 4; nlan = 16; }
        } else if (e.l == 0) {
            img = A->w0_off + e.row * A->s0 + e.col;
            if (fast & 2) { k = L.kw0 + m * 4 + e.col; lane = 16 * g; rr = r; nlan = 16; }
            else { k = L.kw0 + m * nbi + e.col / 16; lane = 16 * g + e.col % 16; rr = r; nlan = 1; }
        } else if (e.l < nl) {
            img = A->wh_off + (e.l - 1) * A->hp * A->sh + e.row * A->sh + e.col;
            k = L.kwh + ((e.l - 1) * nbh + m) * nbh + e.col / 16; lane = 16 * g + e.col % 16; rr = r; nlan = 1;
        } else {
            img = A->wo_off + e.row * A->sh + e.col;
            if (fast & 1) { k = L.kwo + e.col / 16; lane = 16 * ((e.col % 16) / 4); rr = e.col % 4; nlan = 16; }
            else { k = L.kwo + e.col / 16; lane = 16 * (e.row / 4) + e.col % 16; rr = e.row % 4; nlan = 1; }
        }
        imap[e.canon] = img;
        if (A->wide) {
            // row-split kernel: wave w owns feature blocks [w*mb, (w+1)*mb) of every layer
            int w = 0, kk;
            const int mb = WL.mb;
            if (e.l < nl) {
                w = m / mb;
                const int mm = m % mb;
                if (e.col < 0) { kk = WL.kb + e.l * mb + mm; lane = 16 * g; rr = r; }
                else if (e.l == 0) { kk = WL.kw0 + mm * nbi + e.col / 16; lane = 16 * g + e.col % 16; rr = r; }
                else { kk = WL.kwh + ((e.l - 1) * mb + mm) * nbh + e.col / 16; lane = 16 * g + e.col % 16; rr = r; }
            } else if (e.col < 0) {
                kk = WL.kbo; lane = 16 * (e.row / 4); rr = e.row % 4;
            } else {
                const int q = e.col / 16;
                w = q / mb;
                kk = WL.kwo + q % mb; lane = 16 * (e.row / 4) + e.col % 16; rr = e.row % 4;
            }
            rmap[e.canon] = (w * WL.na + kk) * 256 + lane * 4 + rr;      // position in the kernel's LDS staging
            continue;
        }
        if (k < 0) { rmap[e.canon] = (L.na * 256 + 13) | (1 << 24); }
        else {
            if ((nlan != 1 && nlan != 16) || (nlan == 16 && (lane & 15) != 0)) return fail(h, EH_EINVAL, "build_maps: a row-summed accumulator element must start at its row's first column");
            rmap[e.canon] = at(k, lane, rr) | (nlan << 24);
        }
    }
    for (int j = 0; j < d.n_params; ++j)
        if (d.param_kind[j] == EH_PAR_GLOBAL) rmap[n.g_off + d.param_index[j]] = (L.na * 256 + j) | (1 << 24);
    rmap[n.n_theta] = (L.na * 256 + 8) | (1 << 24);
    for (int t = 0; t < n.T; ++t) rmap[n.n_theta + 1 + t] = (L.na * 256 + 9 + t) | (1 << 24);
    rmap[n.n_theta + 1 + n.T] = (L.na * 256 + 14) | (1 << 24);
    rmap[n.n_theta + 2 + n.T] = (L.na * 256 + 15) | (1 << 24);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (with_imap) {
        if (!h->imap) HIPCHK(h, hipMalloc(&h->imap, imap.size() * sizeof(int)));
        HIPCHK(h, hipMemcpy(h->imap, imap.data(), imap.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    // the per-wave kernel's v3 reduction gathers in accumulator order: it wants the INVERSE map, word of a parked accumulator -> canonical
    // index (-1: padding, structural zeros, the columns of a row sum but the first), then the 16 tail words
    const size_t emap_n = (size_t)L.na * 256 + 16;
    if (!A->wide && !v2) {
        std::vector<int> emap(emap_n, -1);
        for (int e = 0; e < h->n_acc; ++e) {
            const int pos = rmap[(size_t)e] & 0xFFFFFF;
            if (pos >= 0 && (size_t)pos < emap_n) emap[(size_t)pos] = e;
        }
        rmap.swap(emap);
    }
    if (rmap.size() > h->rmap_cap) {           // (the kernel family / variant / fast-path options change the layout, and with it the size)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        (void)hipFree(h->rmap); h->rmap = nullptr; h->rmap_cap = 0;
        const size_t want = std::max(rmap.size(), std::max((size_t)h->n_acc, emap_n));
        HIPCHK(h, hipMalloc(&h->rmap, want * sizeof(int)));
        h->rmap_cap = want;
    }
    HIPCHK(h, hipMemcpy(h->rmap, rmap.data(), rmap.size() * sizeof(int), hipMemcpyHostToDevice));
    return EH_OK;
}

// Which vector-ALU fast paths a model may use: bit 0 = single NN output (K == 1), bit 1 = P <= 4 predictors.  Single-target
// models only (the K == 1 kernels keep one residual per sample).  (Round 1 confined the P <= 4 path to the one-block shapes
// because the wider ReLU kernels lost the loss sum; that was the SLP vectoriser -- see the Makefile -- and is gone with it.)
static int fast_wanted(const EhArchInfo* A, int K, int P, int T, int mech) {
    if (!A->has_fast || T != 1 || K != 1 || mech == EH_MECH_PROGRAM) return 0;
    return 1 | (P <= 4 ? 2 : 0);
}

static const EhArchInfo* find_arch(int nbi, int nbh, int nl) {
#define EH_ARCH_TRY(a, b, c) if (nbi == a && nbh == b && nl == c) return eh_arch_##a##_##b##_##c();
    EH_ARCH_LIST(EH_ARCH_TRY)
#undef EH_ARCH_TRY
    return nullptr;
}
static const EhArchInfo* find_wide(int nbi, int nbh, int nl) {
#define EH_ARCH_TRY(a, b, c) if (nbi == a && nbh == b && nl == c) return eh_wide_##a##_##b##_##c();
    EH_WIDE_LIST(EH_ARCH_TRY)
#undef EH_ARCH_TRY
    return nullptr;
}
// The "shape" of a model that runs layer by layer (eh_lform.hpp): no fused kernel, no parameter image beyond the EH_IMG_* block
static hipError_t lform_prepare(void) { return hipSuccess; }
static hipError_t lform_launch(int, int, int, int, hipStream_t, const EhNet*, const EhStepArgs*) { return hipErrorNotSupported; }
static const EhArchInfo g_lform_arch = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, /*phi_off*/ 0, /*img_floats*/ EH_IMG_META, /*has_fast*/ 0, /*nvar*/ 1,
                                        {{4, 4, 0, 1 << 30, &lform_prepare, &lform_launch, 1, 0}, {}, {}, {}}, /*wide*/ 1};

static bool arch_fits(const EhArchInfo* A, int need) {
    for (int vi = 0; vi < A->nvar; ++vi)
        if ((long long)(A->var[vi].nw / 2) * need > A->var[vi].red_floats) return false;      // (family choice, not a hard limit: a gradient this large relative to the workspaces is summed across the waves in several rounds, the row-split kernel needs no such sum)
    return true;
}

namespace {
struct EvalHostBuf { float* host; float* dev; size_t cap; int device; };
std::mutex g_eval_pool_mu;
std::vector<EvalHostBuf> g_eval_pool;
}
// (see eval_host_acquire)
static void eval_host_release(eh_handle* h) {
    if (!h->eval_host) return;
    {
        std::lock_guard<std::mutex> lk(g_eval_pool_mu);
        if (g_eval_pool.size() < 8) { g_eval_pool.push_back({h->eval_host, h->eval_host_dev, h->eval_host_cap, h->device}); h->eval_host = nullptr; }
    }
    if (h->eval_host) (void)hipHostFree(h->eval_host);
    h->eval_host = nullptr; h->eval_host_dev = nullptr; h->eval_host_cap = 0;
}
// Launches the step kernel of the handle's (family, variant).  A recorded closure, or any model with the "specialize" option,
// runs a kernel compiled at run time (eh_jit.hpp; built on first use, one per descriptor state; a failed build or launch
// switches the handle to the kernels built ahead of time for good); everything else runs the table entry.
static bool jit_wanted(const eh_handle* h, int mode) {
    const bool prog = h->net.mech == EH_MECH_PROGRAM, closs = h->net.loss == EH_LOSS_PROGRAM;
    if (mode == EH_MODE_TRAIN_P2P && h->act == EH_ACT_PER_NET) return false;
    if (mode == EH_MODE_TRAIN_P2P) return h->jit_on && !h->jit_failed && h->specialize && !prog && !closs && !h->arch->wide;
    if (closs || h->act == EH_ACT_PER_NET || h->drop_on) return mode != EH_MODE_TRAIN_P2P;          // a recorded loss / per-net activations / dropout exist in run-time compiled kernels only
    return h->jit_on && !h->jit_failed && (h->specialize || prog);
}
// the compiled kernels for the handle's current (family, variant, descriptor); builds them on first use; nullptr = not available
static eh_handle_s::JitEntry* jit_entry(eh_handle* h) {
    const int kf = KFAST(h);
    const bool closs = h->net.loss == EH_LOSS_PROGRAM, prog = h->net.mech == EH_MECH_PROGRAM;
    const bool spec = h->specialize || prog || closs || h->act == EH_ACT_PER_NET || h->drop_on;        // a model that is compiled anyway gets its descriptor baked in as well
    float drop[EH_MAX_HIDDEN] = {0};
    if (h->drop_on) memcpy(drop, h->drop, sizeof drop);
    const bool want_p2p = h->specialize && h->p2p_on && !closs && !prog;
    const int lgen = closs ? h->loss_prog.gen : 0;
    for (auto& up : h->jit) {
        eh_handle_s::JitEntry& e = *up;
        if (e.arch == h->arch && e.variant == h->variant && e.fast == kf && e.spec == spec && (e.p2p || !want_p2p) && e.loss_gen == lgen && !memcmp(e.drop, drop, sizeof drop) &&
            (!e.spec || !memcmp(&e.net, &h->net, sizeof(EhNet)))) {
            const int st = e.state.load(std::memory_order_acquire);
            if (st < 0 && !h->jit_failed) { h->jit_log = e.log; h->jit_failed = true; }       // (a background build that failed: reported like a synchronous one)
            return st > 0 ? &e : nullptr;
        }
    }
    h->jit.emplace_back(new eh_handle_s::JitEntry());
    eh_handle_s::JitEntry* je = h->jit.back().get();
    je->arch = h->arch; je->variant = h->variant; je->fast = kf; je->spec = spec; je->p2p = want_p2p; je->net = h->net; je->loss_gen = lgen;
    memcpy(je->drop, drop, sizeof drop);
    // Only a kernel that merely REPLACES one built ahead of time may arrive later; a recorded closure / loss / per-net activation has no other form
    const bool async = h->specialize_async && !prog && !closs && h->act != EH_ACT_PER_NET && !h->drop_on && !want_p2p && !h->capturing;
    if (async) {
        const eh_model_desc desc = h->desc;
        const int act = h->act, device = h->device;
        je->worker = std::thread([je, desc, act, device]() {
            (void)hipSetDevice(device);
            const bool ok = eh_jit_build(desc, je->arch, je->variant, act, je->fast, &je->net, false, nullptr, &je->k, &je->log, /*allow_slp*/ false);
            je->state.store(ok ? 1 : -1, std::memory_order_release);
        });
        return nullptr;
    }
    const bool ok = eh_jit_build(h->desc, h->arch, h->variant, h->act, kf, spec ? &h->net : nullptr, want_p2p, closs ? &h->loss_prog : nullptr, &je->k, &je->log,
                                 /*allow_slp*/ true, h->drop_on ? je->drop : nullptr, h->plan.acts.empty() ? nullptr : &h->plan.acts);
    je->state.store(ok ? 1 : -1, std::memory_order_release);
    if (!ok) { h->jit_log = je->log; h->jit_failed = true; return nullptr; }
    return je;
}
// A kernel compiled at run time that merely REPLACES one built ahead of time (the "specialize" option on a registry model) is checked
// against it before it takes over: both run the training pass on one window of the step's own data (no update, no state touched),
// their partial sums are reduced, and loss sum, counts and un-normalised gradient must agree to 1e-5 of the gradient's largest
// entry.  The two are the same source -- constants folded, dead branches gone -- but different binaries (hiprtc; the SLP vectoriser
// on for the one-block shapes, which miscompiled a sibling group of kernels in round 2: a loss sum lost in a packed accumulator),
// and the retry ladder of the build only catches compiler refusals, not silent miscompiles.  On disagreement the handle keeps the
// kernels built ahead of time and says so in eh_jit_status.  ~100 us, once per compiled kernel.
static int grid_for(const eh_handle* h, long long count);
static bool jit_verify(eh_handle* h, eh_handle_s::JitEntry* je, const EhStepArgs* a) {
    const EhNet& net = h->net;
    EhStepArgs v = *a;
    v.fz.gacc = nullptr;                         // the two-kernel form of the pass: one slab row per workgroup, nothing else written
    v.count = std::min<long long>(a->count, 8192);
    v.bn_update = 0; v.stamps = nullptr; v.slab = h->slab; v.n_acc = h->n_acc;
    v.yhat = nullptr; v.pout = nullptr;
    if (v.count <= 0) return true;
    const int grid = grid_for(h, v.count);
    const size_t nb = (size_t)h->n_acc * sizeof(float);
    float* dev = nullptr;
    if (hipMalloc(&dev, 2 * nb) != hipSuccess) { (void)hipGetLastError(); return true; }      // (cannot check: not a reason to refuse the kernel)
    std::vector<float> host(2 * (size_t)h->n_acc);
    float* sc = h->sc;                           // (read by nothing: APPLY = false)
    bool launched = true;
    for (int k = 0; k < 2 && launched; ++k) {
        hipError_t e = k == 0 ? h->arch->var[h->variant].launch(EH_MODE_TRAIN, h->act, KFAST(h), grid, h->stream, &net, &v)
                              : eh_jit_launch(&je->k, EH_MODE_TRAIN, grid, h->stream, &net, &v);
        if (e != hipSuccess) { (void)hipGetLastError(); launched = false; break; }
        hipLaunchKernelGGL((eh_reduce_kernel<false, 16>), dim3((h->n_acc + 15) / 16), dim3(256), 0, h->stream, h->slab, grid, h->n_acc, net.n_theta, net.T, 0,
                           dev + (size_t)k * h->n_acc, TH(h), MM(h), VV(h), sc, sc, h->opt, (float*)nullptr, h->img, net.loss, (const float*)nullptr, (const float*)nullptr, 0u);
        if (hipGetLastError() != hipSuccess) { launched = false; break; }
    }
    bool ok = true;
    std::string why;
    if (launched && hipMemcpyAsync(host.data(), dev, 2 * nb, hipMemcpyDeviceToHost, h->stream) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess) {
        const float* A = host.data(); const float* B = A + h->n_acc;
        if (getenv("EH_DEBUG_JIT_SKEW")) host[(size_t)h->n_acc + net.n_theta] *= 1.01f;        // tests: the fall-back path without a second compiler run
        double gmax = 0.0, dmax = 0.0;
        for (int i = 0; i < net.n_theta; ++i) { gmax = std::max(gmax, (double)fabsf(A[i])); dmax = std::max(dmax, (double)fabsf(A[i] - B[i])); }
        const double sa = A[net.n_theta], sb = B[net.n_theta];
        bool counts = true;
        for (int t = 0; t < net.T; ++t) counts = counts && A[net.n_theta + 1 + t] == B[net.n_theta + 1 + t];
        const bool loss_ok = (std::isnan(sa) && std::isnan(sb)) || fabs(sa - sb) <= 1e-5 * fabs(sa) + 1e-30;      // (a window without a valid target: NaN on both sides)
        if (!(dmax <= 1e-5 * gmax + 1e-30) || !loss_ok || !counts || !std::isfinite(gmax)) {
            ok = false;
            char b[320];
            snprintf(b, sizeof b, "the kernel compiled at run time disagrees with the one built ahead of time on %lld samples of this model's data "
                     "(gradient: max |difference| %.3g against a largest entry of %.3g; loss sum %.9g vs %.9g; valid counts %s): the handle keeps the kernels built ahead of time",
                     v.count, dmax, gmax, sb, sa, counts ? "equal" : "DIFFERENT");
            why = b;
        }
    } else (void)hipGetLastError();
    (void)hipFree(dev);
    if (!ok) { je->state.store(-1); h->jit_failed = true; h->jit_log = why; }
    return ok;
}

// agg = mean: the data loss enters with 1 / (T_data (1 + E)), every entry of the extra loss with 1 / (1 + E) (EhImg); targets that stand
// for entries of the extra loss (eh_set_target_roles) are not data targets
static void eh_agg_factors(eh_handle* h) {
    int tdata = 0;
    for (int t = 0; t < h->net.T; ++t) tdata += ((h->roles >> (2 * t)) & 3u) == 0u ? 1 : 0;
    h->img.agg_a = h->agg ? 1.0f / ((float)std::max(1, tdata) * (float)(1 + h->n_extra)) : 1.0f;
    h->img.l2s = h->agg ? 1.0f / (float)(1 + h->n_extra) : 1.0f;
}

// the kernel specialised AHEAD OF TIME for this handle's descriptor, if it is one of the canonical ones (eh_spec.hip); nullptr otherwise
static const EhSpecKernel* spec_lookup(const eh_handle* h) {
    static const EhSpecKernel* const list[] = {
#define EH_SPEC_ITEM(k) eh_spec_##k(),
        EH_SPEC_LIST(EH_SPEC_ITEM)
#undef EH_SPEC_ITEM
    };
    // hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies per DEVICE: several handles of one process on different devices
    // (eh_p2p_init_local, eh_comm_init_local) each need the raised LDS limit (advisor, round 4: a per-process flag left every device but
    // the first with a kernel that failed to launch on every step and fell back silently)
    static std::mutex mu;
    static uint64_t prepared[sizeof list / sizeof list[0]] = {};          // bit d: prepared on device d
    if (!h->aot_spec || h->lform || h->act == EH_ACT_PER_NET || h->drop_on) return nullptr;
    const EhArchInfo* A = h->arch;
    const EhVariant& V = A->var[h->variant];
    const int kf = KFAST(h);
    for (size_t i = 0; i < sizeof list / sizeof list[0]; ++i) {
        const EhSpecKernel* k = list[i];
        if (k->wide != (A->wide != 0) || k->bf16 != V.bf16 || k->nbi != A->nbi || k->nbh != A->nbh || k->nl != A->nl || k->nt != V.nt || k->nw != V.nw ||
            k->act != h->act || k->fast != kf || (k->so != 0) != (V.so != 0) || memcmp(&k->net, &h->net, sizeof(EhNet)) != 0) continue;
        {
            std::lock_guard<std::mutex> lk(mu);
            const uint64_t bit = 1ull << (h->device & 63);
            if (!(prepared[i] & bit)) {
                if (hipSetDevice(h->device) != hipSuccess || k->prepare() != hipSuccess) { (void)hipGetLastError(); return nullptr; }
                prepared[i] |= bit;
            }
        }
        return k;
    }
    return nullptr;
}

// May the handle's single-step train launches (EH_MODE_TRAIN, EH_MODE_TRAIN_ORD) run the lean form of their kernel?  Decided here, from
// the handle's configuration, wherever that changes (creation, optimiser set-up, options, dropout, recorded losses, diagnostics) --
// not per step: one target trained on a one-pass loss, no input BatchNorm, no dropout, no recorded program or loss, one activation,
// ONE optimiser rule and that rule Adam, no diagnostics buffer.  "lean" = 0 / EH_NO_LEAN=1: never (the A/B).
// (EH_LEAN_DIAG=1, the measurement tools: a RUN-TIME COMPILED kernel built with EH_STAMPS through EH_JIT_DEFINES keeps the diagnostics
//  pointer in its lean form too -- tools/stamps_*.py then stamp both forms with one library.  The kernels built ahead of time never
//  take an armed diagnostics buffer in their lean form: lean_wanted is strict for them.)
static bool lean_diag_env() { static const bool on = getenv("EH_LEAN_DIAG") != nullptr; return on; }
static void lean_refresh(eh_handle* h) {
    static const bool env_off = getenv("EH_NO_LEAN") != nullptr;
#ifdef EH_STAMPS
    const bool diag = false;                     // (diagnostic builds: the lean kernel keeps the stamps, tools/stamps_*.py measure both forms)
#else
    const bool diag = h->stamps != nullptr && !lean_diag_env();
#endif
    h->lean_cfg = h->lean && !env_off && h->arch && !h->arch->wide && !h->lform && !h->seq && h->net.T == 1 && !h->bn_on && !h->drop_on &&
                  h->net.mech != EH_MECH_PROGRAM && h->net.loss != EH_LOSS_PROGRAM && h->act != EH_ACT_PER_NET && eh_two_pass_mask(h) == 0u &&
                  h->opt.tab == nullptr && h->opt.rule == EH_OPT_ADAM && !diag;
}
// ... and do this launch's arguments keep the contract (a cheap cross-check of what lean_refresh concluded: anything else runs the general kernel)
// (jit: the launch goes to a run-time compiled kernel -- the only place EH_LEAN_DIAG lets an armed diagnostics buffer through)
static bool lean_wanted(const eh_handle* h, const EhStepArgs* a, bool jit = false) {
    if (!h->lean_cfg) return false;
    if (eh_lean_args_ok(*a)) return true;
    if (!jit || !lean_diag_env() || !a->stamps) return false;
    EhStepArgs b = *a;
    b.stamps = nullptr;
    return eh_lean_args_ok(b);
}
// which form the single-step train launch ran (eh_jit_status reports the last one; EH_JIT_TRACE=1 prints every change)
static void lean_note(eh_handle* h, bool lean) {
    const int v = lean ? 1 : 0;
    if (h->lean_last != v && getenv("EH_JIT_TRACE")) fprintf(stderr, "eh_jit: train step kernel: %s\n", lean ? "lean" : "general");
    h->lean_last = v;
}

// One attempt on the kernel built ahead of time for the handle's descriptor (eh_spec.hip).  The single-step train modes take its lean form
// (eh_lean_fold, eh_device.hpp) where the unit holds one, the handle's configuration is inside the contract (lean_refresh) and the
// arguments say the same; a lean entry that refuses them has launched nothing, and the general kernel takes the step.
static hipError_t spec_launch(eh_handle* h, const EhSpecKernel* sk, int mode, int grid, const EhStepArgs* a) {
    const bool single = mode == EH_MODE_TRAIN || mode == EH_MODE_TRAIN_ORD;
    bool ln = single && sk->has_lean && lean_wanted(h, a);
    hipError_t e = sk->launch(mode, grid, h->stream, &h->net, a, ln);
    if (ln && e != hipSuccess) {
        (void)hipGetLastError();
        ln = false;
        e = sk->launch(mode, grid, h->stream, &h->net, a, false);
    }
    if (e == hipSuccess) { h->spec_used = sk; if (single) lean_note(h, ln); } else (void)hipGetLastError();
    return e;
}
// The step kernel of `mode` for the handle: ahead-of-time specialised (spec_lookup), compiled at run time (jit_entry), or the table
// entry of the handle's (family, variant) -- in that order, with fall-through rules that differ by mode and are the contract of the
// ordered step (its bits are those of the step + reduce pair only on the kernel the pair's step runs):
//   EH_MODE_TRAIN_ORD    when an ahead-of-time kernel matched, its result is final.  A run-time compiled kernel is used only once the
//                        pair's first step has checked it (`verified`, jit_verify) and only if it has the mode; otherwise
//                        hipErrorNotSupported, nothing launched: the caller runs the pair.
//   EH_MODE_TRAIN_MULTI  (the caller checked multi_ok) a failed ahead-of-time launch goes straight to the table, not to the run-time
//                        compiled kernel; that one is used only if `verified` (the single-step path does the check).
//   every other mode     a failed ahead-of-time launch (a mode the unit does not hold) falls through to the run-time compiled kernel and
//                        then the table.  Here jit_verify runs; a failed launch of the compiled kernel retires it; a recorded loss,
//                        dropout and per-net activations have no other form: hipErrorNotSupported instead of the table.
static hipError_t step_launch(eh_handle* h, int mode, int grid, const EhStepArgs* a) {
    const bool train = mode == EH_MODE_TRAIN, ord = mode == EH_MODE_TRAIN_ORD, multi = mode == EH_MODE_TRAIN_MULTI;
    const EhSpecKernel* sk = spec_lookup(h);
    if (sk) {
        const hipError_t e = spec_launch(h, sk, mode, grid, a);
        if (e == hipSuccess || ord) return e;
    }
    if (ord || multi) {      // the run-time compiled kernel of the single-step path, once that path has checked it against the generic one
        eh_handle_s::JitEntry* je = ((multi && sk) || !jit_wanted(h, EH_MODE_TRAIN)) ? nullptr : jit_entry(h);
        if (je && ord) {
            if (!je->verified || !je->k.fn[EH_MODE_TRAIN_ORD]) return hipErrorNotSupported;
            const bool ln = je->k.fn_lean[1] && lean_wanted(h, a, true);
            const hipError_t e = eh_jit_launch(&je->k, mode, grid, h->stream, &h->net, a, ln);
            if (e == hipSuccess) lean_note(h, ln);
            return e;
        }
        if (je && je->verified && je->k.fn[EH_MODE_TRAIN_MULTI]) {
            if (eh_jit_launch(&je->k, mode, grid, h->stream, &h->net, a) == hipSuccess) return hipSuccess;
            (void)hipGetLastError();
        }
        if (ord) lean_note(h, false);
        return h->arch->var[h->variant].launch(mode, h->act, KFAST(h), grid, h->stream, &h->net, a);
    }
    if (jit_wanted(h, mode)) {
        eh_handle_s::JitEntry* je = jit_entry(h);
        if (je && !je->verified && mode != EH_MODE_EVAL && !h->capturing && je->spec && h->net.mech != EH_MECH_PROGRAM && h->net.loss != EH_LOSS_PROGRAM &&
            h->act != EH_ACT_PER_NET && !h->drop_on && !getenv("EH_JIT_NO_VERIFY")) {      // (dropout: nothing built ahead of time computes the same)
            bool has_lprog = false;
            for (int t = 0; t < h->net.T; ++t) has_lprog = has_lprog || ((h->net.loss_t >> (4 * t)) & 15u) == (unsigned)EH_LOSS_PROGRAM;
            if (has_lprog || jit_verify(h, je, a)) je->verified = true; else je = nullptr;
        }
        if (je) {
            // (the lean entry of a module whose GENERAL train kernel jit_verify has checked against the one built ahead of time: the lean
            //  entry itself is not run through that check -- it is the same source in the same module, and tests/test_gpu_lean_step.py
            //  compares the two bit for bit)
            const bool ln = train && je->verified && je->k.fn_lean[0] && lean_wanted(h, a, true);
            const hipError_t e = eh_jit_launch(&je->k, mode, grid, h->stream, &h->net, a, ln);
            if (e == hipSuccess) { if (train) lean_note(h, ln); return e; }
            (void)hipGetLastError();
            je->state.store(-1); h->jit_failed = true;
            h->jit_log = std::string("launch of the run-time compiled kernel failed: ") + hipGetErrorString(e);
        }
        if ((h->net.loss == EH_LOSS_PROGRAM || h->drop_on) && mode != EH_MODE_EVAL) return hipErrorNotSupported;     // no other form of a recorded loss / of dropout exists
    }
    if (h->act == EH_ACT_PER_NET) return hipErrorNotSupported;       // (the table below has no such kernel; eh_create made sure the compiled one exists)
    if (train) lean_note(h, false);
    return h->arch->var[h->variant].launch(mode, h->act, KFAST(h), grid, h->stream, &h->net, a);
}

extern "C" {

int32_t eh_version(void) { return EH_ABI_VERSION; }

const char* eh_last_error(const eh_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

// Streams of destroyed handles are kept for the next handle on the same device: creating one takes 1.4-1.9 ms and destroying it as long
// again -- a fifth of a whole train() call on the reference's tutorial data set, which creates and destroys one engine per call.  At most
// eight per device are kept (more are destroyed); the kept ones live until the process ends.
static std::mutex g_stream_pool_mu;
static std::vector<std::pair<int, hipStream_t>> g_stream_pool;
static hipStream_t stream_pool_take(int device) {
    std::lock_guard<std::mutex> lk(g_stream_pool_mu);
    for (size_t i = 0; i < g_stream_pool.size(); ++i)
        if (g_stream_pool[i].first == device) { hipStream_t s = g_stream_pool[i].second; g_stream_pool.erase(g_stream_pool.begin() + (long)i); return s; }
    return nullptr;
}
static void stream_pool_give(int device, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(g_stream_pool_mu);
        int kept = 0;
        for (auto& e : g_stream_pool) kept += e.first == device;
        if (kept < 8 && !getenv("EH_NO_STREAM_POOL")) { g_stream_pool.emplace_back(device, s); return; }
    }
    (void)hipStreamDestroy(s);
}

static int32_t create_handle(const eh_model_desc* d, eh_handle** out, bool seq_several_targets, const eh_act_program* acts = nullptr, int n_acts = 0);
int32_t eh_create(const eh_model_desc* d, eh_handle** out) { return create_handle(d, out, false); }
int32_t eh_create_seq_targets(const eh_model_desc* d, eh_handle** out) { return create_handle(d, out, true); }
int32_t eh_create_activations(const eh_model_desc* d, const eh_act_program* progs, int32_t n_progs, eh_handle** out) {
    if (n_progs != 0 && !progs) return fail(nullptr, EH_EINVAL, "eh_create_activations: null argument");
    if (n_progs < 0) return fail(nullptr, EH_EINVAL, "eh_create_activations: %d activation programs (0..%d)", (int)n_progs, (int)EH_MAX_ACT_PROGS);
    return create_handle(d, out, false, progs, n_progs);
}
static int32_t create_handle(const eh_model_desc* d, eh_handle** out, bool seq_several_targets, const eh_act_program* acts, int n_acts) {
    if (!d || !out) return fail(nullptr, EH_EINVAL, "eh_create: null argument");
    *out = nullptr;
    // everything that needs no device: checks, block placement, the layout of flat theta, the family asked for, the EhNet (eh_plan.hpp)
    EhPlan plan;
    std::string why;
    if (const int rc = eh_plan_model(d, seq_several_targets, &plan, &why, acts, n_acts)) return fail(nullptr, rc, "%s", why.c_str());
    const bool no_nn = plan.family == EH_FAMILY_NONE, seq = plan.family == EH_FAMILY_SEQ;
    const EhNet n = plan.net;
    // (EH_FORCE_LFORM: A/B switch of the measurement tools -- every feed-forward model layer by layer, the baseline tools/bench_bn_chain.py compares with)
    static const bool force_lform = getenv("EH_FORCE_LFORM") != nullptr;
    // (normalisation layers never look for a fused kernel: a BatchNorm layer couples the samples of a minibatch, eh_bnl.hpp; a LayerNorm layer runs as a pass of its own too, eh_lnl.hpp)
    const bool try_fused = plan.family == EH_FAMILY_FUSED && !force_lform && plan.nbh && n.K <= 16;
    const EhArchInfo* const wide_arch = try_fused ? find_wide(plan.nbi, plan.nbh, d->n_hidden) : nullptr;
    const EhArchInfo* arch = try_fused ? find_arch(plan.nbi, plan.nbh, d->n_hidden) : nullptr;
    if (!arch) arch = wide_arch;
    bool lform = no_nn;
    if (no_nn || seq) arch = &g_lform_arch;      // (seq: its own kernel family, eh_seq.hpp; of the "architecture" only the PHI block of the image is used)
    else if (!arch) {
        // no fused kernel holds this network: run it layer by layer (eh_lform.hpp) where that form is built
        // (every activation, SingleNN and MultiNN alike: the layer-wise form runs each network as its own chain of products)
        if (n.K > 16 || (d->input_batchnorm && d->n_predictors > 32))
            return fail(nullptr, EH_EUNSUPPORTED, "eh_create: no kernel for P=%d, hidden max width %d%s, %d hidden layers, K=%d, activation %d (fused kernels: P<=32, K<=16, "
                        "width<=64 with <=3 layers or width<=128 with <=2; layer-wise form: K<=16, input BatchNorm with P<=32)",
                        d->n_predictors, plan.maxw, d->n_nets > 0 ? " (nets side by side)" : "", d->n_hidden, n.K, plan.act);
        arch = &g_lform_arch;
        lform = true;
    }
    // (the planner has refused the shapes no fused kernel holds; this answers what is left: EH_FORCE_LFORM, a shape the library was built without)
    if (n_acts > 0 && (lform || seq))
        return fail(nullptr, EH_EUNSUPPORTED, "eh_create_activations: recorded activations are built for the fused kernels, not for the layer-wise form this network runs on");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, EH_EHIP, "eh_create: no HIP device (this library has no CPU path)");
    if (d->device < 0 || d->device >= ndev) return fail(nullptr, EH_EINVAL, "eh_create: device %d of %d", d->device, ndev);

    eh_handle* h = new eh_handle_s();
    h->plan = std::move(plan);
    const EhPlan& p = h->plan;
    h->desc = p.desc; h->net = p.net; h->act = p.act; h->n_acc = p.n_acc;
    h->seq = seq; h->bnl = p.bnl; h->lnl = p.lnl;
    for (int l = 0; l < p.l_net[0].nl; ++l) {      // eh_set_layer_norm's defaults
        if (eh_is_norm(p.l_net[0].kind[l])) h->bnl_eps[l] = EH_BN_EPS;
        if (eh_is_norm(p.l_net[0].kind[l]) && !eh_is_layernorm(p.l_net[0].kind[l])) h->bnl_mom[l] = EH_BN_MOMENTUM;
    }
    h->device = d->device;
    h->arch = arch;
    h->lform = lform;
    h->variant = (arch->nvar > 1 && !arch->wide) ? 1 : 0;   // narrow nets: two waves per SIMD hide the latency of the short tile
    h->fast = fast_wanted(arch, n.K, n.P, n.T, d->mech);
    if (seq && h->n_acc > eh_seq_row_cap(p.seq_nbi, p.seq_nbh, p.seq_cell)) {
        delete h;
        return fail(nullptr, EH_EUNSUPPORTED, "eh_create: no kernel for a sequence model of %d parameters (the slab row is staged in LDS)", n.n_theta);
    }
    if (!lform && !seq && !arch_fits(arch, std::max(h->n_acc, EH_EVAL_STATS * n.T))) {
        // the per-wave kernel parks every wave's accumulators in LDS to sum them; the row-split kernel needs no such sum
        if (!wide_arch) {
            delete h;
            return fail(nullptr, EH_EUNSUPPORTED, "eh_create: %d accumulators exceed the kernel's reduction space", n.n_theta + 1 + n.T);
        }
        h->arch = arch = wide_arch;
        h->variant = 0;
        h->fast = 0;
    }
    h->arch_alt =(arch == wide_arch || seq || lform) ? nullptr : wide_arch;
#define HIPCHK_C(expr)                                                            \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fail(nullptr, e_ == hipErrorOutOfMemory ? EH_ENOMEM : EH_EHIP, "eh_create: %s: %s", #expr, hipGetErrorString(e_)); \
            eh_destroy(h);                                                        \
            return e_ == hipErrorOutOfMemory ? EH_ENOMEM : EH_EHIP;               \
        }                                                                         \
    } while (0)
    const bool ctrace = getenv("EH_CREATE_TRACE") != nullptr;          // diagnostics: where eh_create's milliseconds go
    auto ct0 = std::chrono::steady_clock::now();
    auto tick = [&](const char* what) {
        if (!ctrace) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[eh_create] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(t - ct0).count());
        ct0 = t;
    };
    HIPCHK_C(hipSetDevice(h->device));
    tick("hipSetDevice");
    if (!(h->own_stream = stream_pool_take(h->device))) HIPCHK_C(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    tick("stream");
    h->stream = h->own_stream;
    for (int vi = 0; vi < arch->nvar; ++vi) HIPCHK_C(arch->var[vi].prepare());
    tick("kernel attributes");
    if (const char* ej = getenv("EH_JIT")) h->jit_on = atoi(ej) != 0;
    if (const char* es = getenv("EH_SPECIALIZE")) h->specialize = atoi(es) != 0;      // (test runs: the whole suite on specialised kernels)
    if (getenv("EH_NO_AOT_SPEC")) h->aot_spec = false;                                // (A/B: the generic / run-time compiled kernels for a canonical descriptor)
    if (d->mech == EH_MECH_PROGRAM) {
        std::vector<unsigned> pb(EH_PROG_HDR + EH_MAX_PROG, 0u);
        pb[0] = (unsigned)d->prog_len; pb[1] = (unsigned)d->prog_n_out;
        for (int o = 0; o < EH_MAX_PROG_OUT; ++o) pb[2 + o] = (unsigned)(o < d->prog_n_out ? d->prog_out[o] : d->prog_out[0]);
        for (int k = 0; k < d->prog_n_const; ++k) memcpy(&pb[8 + k], &d->prog_const[k], sizeof(float));
        for (int i = 0; i < d->prog_len; ++i) pb[EH_PROG_HDR + i] = d->prog_code[i];
        HIPCHK_C(hipMalloc(&h->prog, pb.size() * sizeof(unsigned)));
        HIPCHK_C(hipMemcpy(h->prog, pb.data(), pb.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    }
    const size_t nt = (size_t)n.n_theta;
    // one allocation: [2][3][n_theta] parameter sets {theta, m, v}, then the [EH_MAX_OPT_GROUPS][2][2] running beta products (EhOptTab)
    HIPCHK_C(hipMalloc(&h->pset, (6 * nt + 4 * EH_MAX_OPT_GROUPS) * sizeof(float)));
    HIPCHK_C(hipMemset(h->pset, 0, (6 * nt + 4 * EH_MAX_OPT_GROUPS) * sizeof(float)));
    for (int k = 0; k < 2; ++k) { h->thb[k] = h->pset + (size_t)k * 3 * nt; h->mb[k] = h->thb[k] + nt; h->vb[k] = h->thb[k] + 2 * nt; }
    h->sc = h->pset + 6 * nt;
    h->bn_on = d->input_batchnorm != 0;
    if (h->bn_on) {
        HIPCHK_C(hipMalloc(&h->bn_part, (32 * 64 + 32) * sizeof(float)));
        HIPCHK_C(hipMalloc(&h->bn_run, 64 * sizeof(float)));
        HIPCHK_C(hipMalloc(&h->bn_shift, 32 * sizeof(float)));
        HIPCHK_C(hipMemset(h->bn_shift, 0, 32 * sizeof(float)));
        HIPCHK_C(hipMalloc(&h->bn_stat, 68 * sizeof(float)));
        HIPCHK_C(hipMemset(h->bn_stat, 0, 68 * sizeof(float)));
        float run0[64];
        for (int p = 0; p < 32; ++p) { run0[p] = 0.0f; run0[32 + p] = 1.0f; }     // LuxCore.initialstates(BatchNorm)
        HIPCHK_C(hipMemcpy(h->bn_run, run0, sizeof run0, hipMemcpyHostToDevice));
    }
    if (h->bnl || h->lnl) {   // BatchNorm layers: running statistics (LuxCore.initialstates: mean 0, var 1), the step's own; both kinds: the partial column sums
        const int tot = p.bnl_tot;          // (of the BatchNorm layers alone: a LayerNorm layer has no state)
        const EhLNet& L = p.l_net[0];
        if (h->bnl) {
            std::vector<float> run0((size_t)tot, 0.0f);
            for (int l = 0; l < L.nl; ++l)
                if (eh_is_norm(L.kind[l]) && !eh_is_layernorm(L.kind[l])) std::fill(run0.begin() + p.bnl_off[l] + L.out[l], run0.begin() + p.bnl_off[l] + 2 * L.out[l], 1.0f);
            HIPCHK_C(hipMalloc(&h->bnl_run, (size_t)tot * sizeof(float)));
            HIPCHK_C(hipMemcpy(h->bnl_run, run0.data(), (size_t)tot * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK_C(hipMalloc(&h->bnl_stat, (size_t)2 * tot * sizeof(float)));
            HIPCHK_C(hipMemset(h->bnl_stat, 0, (size_t)2 * tot * sizeof(float)));
        }
        HIPCHK_C(hipMalloc(&h->bnl_part, (size_t)(EH_BNL_CHUNKS + 1) * 2 * p.norm_maxn * sizeof(float)));
    }
    if (!lform && !seq) {     // (the fused-update accumulators: that mode exists for the per-wave kernels only)
        HIPCHK_C(hipMalloc(&h->gacc, ((size_t)3 * EH_GSHARDS * h->n_acc + 4) * sizeof(float)));      // (+4: the fused prologue reads five tail floats of every shard whatever T is)
        HIPCHK_C(hipMemset(h->gacc, 0, ((size_t)3 * EH_GSHARDS * h->n_acc + 4) * sizeof(float)));
        h->ord_soff = (n.n_theta + 3) & ~3;
        h->ord_rs = h->ord_soff + ((h->n_acc - n.n_theta + 3) & ~3);
        // (counters | rows | group rows | the scalars' block partials [2][4][16][4], addressed from the group rows: no pointer of their own)
        const size_t ob = sizeof(unsigned) * 32 * EH_ORD_GROUPS + sizeof(float) * ((size_t)2 * (EH_ORD_ROWS + EH_ORD_GROUPS) * h->ord_rs + 2 * EH_ORD_PART);
        HIPCHK_C(hipMalloc(&h->ord, ob));
        HIPCHK_C(hipMemset(h->ord, 0, ob));      // (the counters start at 0; every launch leaves them there)
        HIPCHK_C(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(h->ord + 32 * EH_ORD_GROUPS), (int)EH_ORD_EMPTY, (size_t)2 * EH_ORD_ROWS * h->ord_rs));      // (the rows: "not written")
        HIPCHK_C(hipHostMalloc((void**)&h->ord_err, sizeof(unsigned), hipHostMallocMapped));      // (host memory: eh_synchronize reads it without a copy)
        *h->ord_err = 0u;
    }
    tick("pset / bn / gacc");
    h->slab_rows = lform ? (int)EH_LFORM_ROWS : h->max_blocks;
    HIPCHK_C(hipMalloc(&h->slab, (std::max((size_t)h->slab_rows * std::max(h->n_acc, EH_EVAL_STATS * n.T), (size_t)1 << 20) + 16) * sizeof(float)));      // (>= 4 MB: the evaluation passes park their per-workgroup metric sums here)
    HIPCHK_C(hipMalloc(&h->gradbuf, (size_t)h->n_acc * sizeof(float)));
    HIPCHK_C(hipMalloc(&h->mombuf, EH_MAX_TARG * EH_EVAL_STATS * sizeof(float)));
    HIPCHK_C(hipMemset(h->mombuf, 0, EH_MAX_TARG * EH_EVAL_STATS * sizeof(float)));
    HIPCHK_C(hipMalloc(&h->tcount, 3 * EH_MAX_TARG * sizeof(float)));
    HIPCHK_C(hipMemset(h->tcount, 0, 3 * EH_MAX_TARG * sizeof(float)));
    HIPCHK_C(hipMalloc(&h->inv_n, EH_TT * EH_MAX_TARG * sizeof(float)));      // the per-target table (EhStepArgs::inv_n): weight, centre of yhat, k0 k1 k2, loss of every target
    HIPCHK_C(hipMemset(h->inv_n, 0, EH_TT * EH_MAX_TARG * sizeof(float)));
    HIPCHK_C(hipMemset(h->gradbuf, 0, (size_t)h->n_acc * sizeof(float)));
    tick("slab + small buffers");
    if (!lform && !seq) { if (int rc = build_maps(h, true)) { g_create_err = h->err; eh_destroy(h); return rc; } }
    else {                    // (no parameter image to tell a weight by: the leaves weight_l2 sums, flagged)
        std::vector<unsigned char> wf((size_t)n.n_theta, 0);
        for (const EhLeaf& f : p.leaves)
            if (f.is_weight) std::fill(wf.begin() + f.off, wf.begin() + f.off + f.size(), (unsigned char)1);
        HIPCHK_C(hipMalloc(&h->wflag, wf.size()));
        HIPCHK_C(hipMemcpy(h->wflag, wf.data(), wf.size(), hipMemcpyHostToDevice));
    }
    tick("maps");
    {   // parameter image (constant parts; theta is mirrored into it by eh_image_kernel / the optimiser)
        std::vector<float> img0((size_t)arch->img_floats, 0.0f);
        for (int j = 0; j < d->n_params; ++j) {
            if (d->param_kind[j] == EH_PAR_FIXED) img0[arch->phi_off + EH_IMG_PHI + j] = d->param_default[j];   // st.fixed, GenericHybridModel.jl:289-303
            img0[arch->phi_off + EH_IMG_LO + j] = d->param_lower[j];
            img0[arch->phi_off + EH_IMG_SC + j] = d->param_upper[j] - d->param_lower[j];
        }
        for (int q = 0; q < 32; ++q) { img0[arch->phi_off + EH_IMG_BNM + q] = 0.0f; img0[arch->phi_off + EH_IMG_BNR + q] = d->input_batchnorm ? 1.0f / std::sqrt(1.0f + EH_BN_EPS) : 1.0f; }
        const int nl = d->n_hidden;
        for (int k = 0; k < (lform ? 0 : p.n_nets); ++k)      // identity blocks that carry a shallower net to the output layer (fused envelope only: the layer-wise form runs every net at its own depth)
            for (int l = p.net_d[k]; l < nl; ++l)
                for (int i = 0; i < p.net_w[k][l]; ++i)
                    img0[arch->wh_off + (size_t)(l - 1) * arch->hp * arch->sh + (size_t)(p.net_r0[k][l] + i) * arch->sh + p.net_r0[k][l - 1] + i] = 1.0f;
        auto put_int = [&](int slot, int v) { memcpy(&img0[arch->phi_off + slot], &v, sizeof(int)); };
        if (!lform && !seq) { // (read by the fused kernels' end-of-kernel reduction only; sized for their four layers)
            // canonical offsets of net 0 (all there is for SingleNN); an identity block of it: where its output layer starts, nothing of the block in theta
            const EhLNet& L = p.l_net[0];
            for (int l = 0; l <= nl; ++l) {
                const int c = std::min(l, L.nl - 1);
                put_int(EH_IMG_WOFF + l, L.woff[c]); put_int(EH_IMG_BOFF + l, (l < nl && l >= L.nl - 1) ? L.woff[c] : L.boff[c]);
            }
            for (int l = 0; l < nl; ++l) put_int(EH_IMG_WIDTH + l, p.tot_w[l]);
        }
        for (int j = 0; j < d->n_params; ++j)
            if (d->param_kind[j] == EH_PAR_GLOBAL) put_int(EH_IMG_GPAR + d->param_index[j], j);
        HIPCHK_C(hipMalloc(&h->image, img0.size() * sizeof(float)));
        HIPCHK_C(hipMemcpy(h->image, img0.data(), img0.size() * sizeof(float), hipMemcpyHostToDevice));
        EhImg& im = h->img;
        im.image = h->image; im.imap = h->imap; im.g_off = n.g_off; im.phi_off = arch->phi_off;
        im.l2c = 0.0f; im.l2w = nullptr; im.n_theta = n.n_theta; im.b_off = arch->b_off; im.wflag = h->wflag;
        im.agg_a = 1.0f; im.l2s = 1.0f;          // agg = sum
        HIPCHK_C(hipMalloc(&h->l2val, sizeof(float)));
        HIPCHK_C(hipMemset(h->l2val, 0, sizeof(float)));
        for (int j = 0; j < d->n_params; ++j)
            if (d->param_kind[j] == EH_PAR_GLOBAL) {
                const int g = d->param_index[j];
                im.glob_par[g] = j; im.glo[g] = d->param_lower[j]; im.ghi[g] = d->param_upper[j];
            }
        tick("image");
        hipLaunchKernelGGL(eh_image_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, h->stream, TH(h), (int)nt, h->img);
        HIPCHK_C(hipGetLastError());
        tick("image kernel launch");
        HIPCHK_C(hipStreamSynchronize(h->stream));
        tick("synchronize");
    }
#undef HIPCHK_C
    if (h->act == EH_ACT_PER_NET && !h->lform && !h->seq && !jit_entry(h)) {         // built now, so that a missing run-time compiler is an error of the constructor
        const std::string log = h->jit_log;
        eh_destroy(h);
        return fail(nullptr, EH_EUNSUPPORTED, "eh_create: per-net activations need the run-time compiled kernel, which failed to build: %.600s", log.c_str());
    }
    lean_refresh(h);
    *out = h;
    return EH_OK;
}

int32_t eh_destroy(eh_handle* h) {
    if (!h) return EH_OK;
    if (h->ens_live) return fail(h, EH_ESTATE, "eh_destroy: the handle carries an ensemble (eh_ens_destroy it first)");
    (void)hipSetDevice(h->device);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    for (auto e : h->ev) (void)hipEventDestroy(e);
    for (auto& g : h->graphs) (void)hipGraphExecDestroy(g.exec);
    for (auto& e : h->jit) { if (e->worker.joinable()) e->worker.join(); eh_jit_release(&e->k); }
    eh_jit_release(&h->act_apply);
    eh_comm_release(h);             // communicator / local group / peer-to-peer mappings and buffers (eh_comm.hip)
    (void)hipSetDevice(h->device);
    (void)hipFree(h->pset); (void)hipFree(h->opt_tab);
    (void)hipFree(h->gacc); (void)hipFree(h->ord); if (h->ord_err) (void)hipHostFree(h->ord_err); (void)hipFree(h->bn_part); (void)hipFree(h->bn_run); (void)hipFree(h->bn_shift); (void)hipFree(h->bn_stat); (void)hipFree(h->tcount); (void)hipFree(h->mombuf); (void)hipFree(h->slab); (void)hipFree(h->gradbuf); (void)hipFree(h->inv_n);
    (void)hipFree(h->prog); (void)hipFree(h->l2val); (void)hipFree(h->l2w); (void)hipFree(h->loss_hist); (void)hipFree(h->perm); (void)hipFree(h->out_buf); (void)hipFree(h->idx_buf);
    eval_host_release(h);
    eh_lbfgs_release(h);
    (void)hipFree(h->mech_ws); (void)hipFree(h->l_ws); (void)hipFree(h->l_split); (void)hipFree(h->l_dk); (void)hipFree(h->l_lprog); (void)hipFree(h->wflag);
    (void)hipFree(h->bnl_run); (void)hipFree(h->bnl_stat); (void)hipFree(h->bnl_part);
    (void)hipFree(h->stamps); (void)hipFree(h->image); (void)hipFree(h->imap); (void)hipFree(h->rmap);
    (void)hipFree(h->split[0].recs); (void)hipFree(h->split[1].recs); (void)hipFree(h->split[0].starts); (void)hipFree(h->split[1].starts); (void)hipFree(h->seq_ws); (void)hipFree(h->chain_part);
    if (h->own_stream) stream_pool_give(h->device, h->own_stream);      // (drained above; the next handle on this device takes it over)
    delete h;
    return EH_OK;
}

int32_t eh_n_theta(const eh_handle* h, int64_t* n) {
    if (!h || !n) return EH_EINVAL;
    *n = h->net.n_theta;
    return EH_OK;
}

int32_t eh_set_stream(eh_handle* h, void* s) {
    if (!h) return EH_EINVAL;
    h->stream = s ? (hipStream_t)s : h->own_stream;
    return EH_OK;
}

int32_t eh_synchronize(eh_handle* h) {
    if (!h) return EH_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (polling hipStreamQuery instead was measured and is slower: 12.1-13.4 against 11.4-11.6 us per step in the 20-step run)
    if (h->p2p_on) {
        unsigned c[3] = {0, 0, 0};
        HIPCHK(h, hipMemcpy(c, h->p2p_ctr, sizeof c, hipMemcpyDeviceToHost));
        if (c[1]) return fail(h, EH_EHIP, "eh_synchronize: a cross-GPU exchange ran into its 2 s deadline (a rank is missing or out of step); results are invalid");
    }
    if (h->ord_err && *(volatile unsigned*)h->ord_err)
        return fail(h, EH_EHIP, "eh_synchronize: an ordered step's row of sums did not arrive within its 2 s deadline; results are invalid");
    return EH_OK;
}

// target < 0: the program of every target that has none of its own; 0 <= target < T: that target's own
static int set_loss_program(eh_handle* h, int target, const uint32_t* code, int32_t n_instr, const float* consts, int32_t n_const, int32_t out_slot, const char* who) {
    if (!h || !code || (n_const > 0 && !consts)) return EH_EINVAL;
    if (h->seq) return fail(h, EH_EUNSUPPORTED, "%s: recorded losses are not built for sequence models", who);
    if (n_instr < 1 || n_instr > EH_MAX_PROG) return fail(h, EH_EUNSUPPORTED, "%s: %d instructions (1..%d)", who, n_instr, EH_MAX_PROG);
    if (n_const < 0 || n_const > EH_MAX_PROG_CONST) return fail(h, EH_EUNSUPPORTED, "%s: %d constants (0..%d)", who, n_const, EH_MAX_PROG_CONST);
    auto slot_ok = [&](unsigned sl, int upto) {
        if (sl < EH_PROG_SLOT_CONST) return sl < 2u;                                   // yhat, y
        if (sl < EH_PROG_SLOT_INSTR) return (int)sl - EH_PROG_SLOT_CONST < n_const;
        return (int)sl - EH_PROG_SLOT_INSTR < upto;
    };
    for (int i = 0; i < n_instr; ++i) {
        const unsigned w = code[i], op = w & 255u;
        if (op >= EH_OP_COUNT) return fail(h, EH_EUNSUPPORTED, "%s: instruction %d has unknown opcode %u", who, i, op);
        const int nop = (op == EH_OP_SELECT) ? 3 : (op == EH_OP_NEG || op == EH_OP_EXP || op == EH_OP_LOG || op == EH_OP_SQRT || op == EH_OP_TANH ||
                                                    op == EH_OP_SIGMOID || op == EH_OP_ABS || op == EH_OP_SIN || op == EH_OP_COS) ? 1 : 2;
        const unsigned sl[3] = {(w >> 8) & 255u, (w >> 16) & 255u, w >> 24};
        for (int k = 0; k < 3; ++k)
            if (k < nop ? !slot_ok(sl[k], i) : sl[k] != 0u) return fail(h, EH_EINVAL, "%s: instruction %d, operand %d names slot %u (undefined at that point, or a non-zero unused operand)", who, i, k, sl[k]);
    }
    if (out_slot < 0 || !slot_ok((unsigned)out_slot, n_instr)) return fail(h, EH_EINVAL, "%s: output slot %d", who, out_slot);
    if (h->net.loss == EH_LOSS_PROGRAM) { HIPCHK(h, hipSetDevice(h->device)); FLUSH(h); }
    EhLossProg1& lp = target < 0 ? static_cast<EhLossProg1&>(h->loss_prog) : h->loss_prog.per[target];
    lp.code.assign(code, code + n_instr);
    lp.consts.assign(consts, consts + n_const);
    lp.out = out_slot;
    h->loss_prog.gen++;
    lean_refresh(h);
    return EH_OK;
}
int32_t eh_set_loss_program(eh_handle* h, const uint32_t* code, int32_t n_instr, const float* consts, int32_t n_const, int32_t out_slot) {
    if (h) for (int t = 0; t < EH_MAX_TARG; ++t) h->loss_prog.per[t] = EhLossProg1();        // one function for all targets again
    return set_loss_program(h, -1, code, n_instr, consts, n_const, out_slot, "eh_set_loss_program");
}
int32_t eh_set_target_loss_program(eh_handle* h, int32_t target, const uint32_t* code, int32_t n_instr, const float* consts, int32_t n_const, int32_t out_slot) {
    if (!h) return EH_EINVAL;
    if (target < 0 || target >= h->net.T) return fail(h, EH_EINVAL, "eh_set_target_loss_program: target %d of %d", target, h->net.T);
    return set_loss_program(h, target, code, n_instr, consts, n_const, out_slot, "eh_set_target_loss_program");
}

int32_t eh_set_target_losses(eh_handle* h, const int32_t* kinds, int32_t n) {
    if (!h || !kinds) return EH_EINVAL;
    if (n != h->net.T) return fail(h, EH_EINVAL, "eh_set_target_losses: %d losses for %d targets", n, h->net.T);
    unsigned lt = 0;
    bool same = true;
    bool any_prog = false, any_two = false;
    for (int t = 0; t < n; ++t) {
        if (kinds[t] < EH_LOSS_MSE || kinds[t] > EH_LOSS_PROGRAM) return fail(h, EH_EUNSUPPORTED, "eh_set_target_losses: loss %d for target %d is not implemented on the device", kinds[t], t);
        lt |= (unsigned)kinds[t] << (4 * t);
        same = same && kinds[t] == kinds[0];
        any_prog = any_prog || kinds[t] == EH_LOSS_PROGRAM;
        if (kinds[t] == EH_LOSS_PROGRAM && !h->loss_prog.has(t)) return fail(h, EH_ESTATE, "eh_set_target_losses: target %d: EH_LOSS_PROGRAM without a program (eh_set_loss_program / eh_set_target_loss_program first)", t);
        any_two = any_two || (kinds[t] >= EH_LOSS_PEARSONLOSS && kinds[t] <= EH_LOSS_PBKGELOSS) || (kinds[t] == EH_LOSS_RMSE && n > 1);
    }
    if (same) return eh_set_option(h, "training_loss", kinds[0]);
    if (h->seq) {                            // sequence models: mse, mae and nseLoss per target -- one pass, no recorded losses
        if (any_prog) return fail(h, EH_EUNSUPPORTED, "eh_set_target_losses: recorded losses (EH_LOSS_PROGRAM) are not built for sequence models");
        if (any_two) return fail(h, EH_EUNSUPPORTED, "eh_set_target_losses: rmse on several targets / pearson / kge losses need passes ahead of the step, which are not built for sequence models (per target: mse, mae, nseLoss)");
        HIPCHK(h, hipSetDevice(h->device));
        FLUSH(h);
        h->net.loss = EH_LOSS_MSE;
        h->net.loss_t = lt;
        return EH_OK;
    }
    if (any_two && h->fused) return fail(h, EH_EUNSUPPORTED, "rmse (on a multi-target model) / pearson / kge training losses take forward passes ahead of the step: switch fused_update off first");
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    // (what the single-kind code paths read -- the run-time compiler's "is there a recorded loss", the deferred normalisation of
    //  single-target steps; the kernels take every target's kind from loss_t)
    h->net.loss = any_prog ? EH_LOSS_PROGRAM : EH_LOSS_MSE;
    h->net.loss_t = lt;
    {   // two-pass losses exist in the generic kernels only (the K == 1 / P <= 4 fast paths stay untouched by them)
        const int want = h->lform ? 0 : fast_wanted(h->arch, h->net.K, h->net.P, h->net.T, h->net.mech);
        const int fast = any_two ? 0 : (want & h->fast_user);
        if (!h->lform && fast != h->fast) { h->fast = fast; return build_maps(h, false); }
    }
    return EH_OK;
}

// extra_loss as a function of the predictions (src/losses/compute_loss.jl:31-34; the reference's own test:
// `extra_loss = (yhat, ps) -> [sum(abs, yhat.var1), sum(abs, yhat.var2)]`, test/test_compute_loss.jl:257-285).  An entry that is the sum
// or the mean over ALL samples of the batch of a per-sample function f(yhat_o) of one model output is carried as one more TARGET: it
// observes output o (eh_model_desc::target_output), its data column holds no NaN (the host binding passes zeros), its per-sample loss is the
// recorded f (eh_set_target_loss_program, kind EH_LOSS_PROGRAM in eh_set_target_losses) -- and this call says so:
// roles[t] = 0 a data target | 1 an extra-loss entry, mean over all samples | 2 an extra-loss entry, sum over all samples.
// Such a target takes the extra loss's factor under agg = mean, no 1 / n when it is a sum, and does not count as a data target.
int32_t eh_set_target_roles(eh_handle* h, const int32_t* roles, int32_t n) {
    if (!h || !roles) return EH_EINVAL;
    if (n != h->net.T) return fail(h, EH_EINVAL, "eh_set_target_roles: %d roles for %d targets", n, h->net.T);
    if (h->seq)
        for (int t = 0; t < n; ++t)
            if (roles[t] != 0) return fail(h, EH_EUNSUPPORTED, "eh_set_target_roles: an extra_loss of the predictions (target %d as an entry of it) needs a recorded loss, which sequence models do not have", t);
    unsigned r = 0;
    int ndata = 0;
    for (int t = 0; t < n; ++t) {
        if (roles[t] < 0 || roles[t] > 2) return fail(h, EH_EINVAL, "eh_set_target_roles: role %d of target %d (0 data, 1 extra-loss mean, 2 extra-loss sum)", roles[t], t);
        r |= (unsigned)roles[t] << (2 * t);
        ndata += roles[t] == 0;
    }
    if (ndata == 0) return fail(h, EH_EINVAL, "eh_set_target_roles: at least one data target");
    if (r != 0 && h->net.T < 2) return fail(h, EH_EINVAL, "eh_set_target_roles: an extra-loss entry is a target of its own");
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    h->roles = r;
    eh_agg_factors(h);
    return EH_OK;
}

int32_t eh_jit_status(eh_handle* h, int32_t* n_compiled, char* log, int64_t log_bytes) {
    if (!h || !n_compiled) return EH_EINVAL;
    int n = 0;
    for (auto& e : h->jit) n += e->state.load(std::memory_order_acquire) > 0 ? 1 : 0;
    // a canonical descriptor runs the kernel specialised AHEAD of time (eh_spec.hip): counted like a compiled pair, the log says which it is
    std::string msg = h->jit_log;
    if (h->spec_used && h->aot_spec) { n += 1; msg = std::string("ahead-of-time: ") + h->spec_used->what + (msg.empty() ? "" : "; ") + msg; }
    // which form of the single-step train kernel the last such launch ran (eh_lean_fold, eh_device.hpp)
    if (h->lean_last >= 0) msg += std::string(msg.empty() ? "" : "; ") + (h->lean_last ? "train step kernel: lean" : "train step kernel: general");
    // how many training steps ran as the ordered one-kernel step (a step that fell back to the step + reduce pair is not counted)
    if (h->ord_steps > 0) msg += std::string(msg.empty() ? "" : "; ") + "ordered steps: " + std::to_string(h->ord_steps);
    // which update sites applied how many optimiser updates (host-side counts of the launches; the non-zero ones)
    {
        std::string sites;
        for (int s = 0; s < EH_UPD_SITES; ++s)
            if (h->upd_site[s] > 0) sites += std::string(" ") + eh_upd_site_name(s) + " " + std::to_string(h->upd_site[s]);
        if (!sites.empty()) msg += std::string(msg.empty() ? "" : "; ") + "update sites:" + sites;
    }
    *n_compiled = n;
    if (log && log_bytes > 0) {
        const size_t m = std::min((size_t)log_bytes - 1, msg.size());
        memcpy(log, msg.data(), m);
        log[m] = 0;
    }
    return EH_OK;
}

// may this handle train on the sample-owned bf16 kernel (eh_bf16_sample.hpp)?  One network (its slab row is the plain canonical order); the
// A/B switches of the measurement tools are read once and mean the same to the "precision" and the "variant" option (advisor r05)
static bool so_allowed(const eh_handle* h) {
    static const bool no_so = getenv("EH_NO_DIRECT_STORE") != nullptr || getenv("EH_NO_SAMPLE_OWNED") != nullptr;
    return !no_so && h->plan.n_nets == 1 && h->desc.n_nets == 0;
}

static int32_t set_option(eh_handle* h, const char* name, int64_t value);
int32_t eh_set_option(eh_handle* h, const char* name, int64_t value) {
    if (h && h->ens_live) return fail(h, EH_ESTATE, "eh_set_option: the handle carries an ensemble (eh_ens_destroy it first)");
    if (!h || !name) return EH_EINVAL;
    const int32_t rc = set_option(h, name, value);
    lean_refresh(h);                         // (an option may move the handle into or out of the lean kernels' contract)
    return rc;
}
static int32_t set_option(eh_handle* h, const char* name, int64_t value) {
    if (h->seq) {                            // sequence models: always the reproducible step + reduce pair on the one fp32 kernel family
        if (!strcmp(name, "fused_update")) {
            if (value < 0 || value > 2) return fail(h, EH_EINVAL, "fused_update must be 0, 1 or 2");
            if (value == 1) return fail(h, EH_EUNSUPPORTED, "fused_update: the one-kernel step is not built for sequence models (they run the step + reduce pair)");
            return EH_OK;                    // (2 = "where it is reproducible": the pair is)
        }
        if (!strcmp(name, "multi_step") || !strcmp(name, "specialize") || !strcmp(name, "precision")) {
            if (value) return fail(h, EH_EUNSUPPORTED, "%s: not built for sequence models (one fp32 kernel family, one launch per step)", name);
            return EH_OK;
        }
        if (!strcmp(name, "fast_paths") || !strcmp(name, "row_split") || !strcmp(name, "variant") || !strcmp(name, "aot_spec") || !strcmp(name, "bn_in_kernel") || !strcmp(name, "lean")) return EH_OK;
        if (!strcmp(name, "jit")) { h->jit_on = value != 0; return EH_OK; }      // a recorded closure: 1 = the kernels compiled around the program once built (seq_jit_entry), 0 = the interpreter
        if (!strcmp(name, "training_loss")) {
            if (value < EH_LOSS_MSE || value > EH_LOSS_PROGRAM) return fail(h, EH_EUNSUPPORTED, "training_loss %lld is not implemented on the device", (long long)value);
            if (value > EH_LOSS_NSELOSS) return fail(h, EH_EUNSUPPORTED, "training_loss %lld: sequence models train on mse, rmse, mae and nseLoss (the two-pass losses and recorded losses are not built for them)", (long long)value);
            if (value == EH_LOSS_RMSE && h->net.T > 1) return fail(h, EH_EUNSUPPORTED, "training_loss rmse: on a sequence model with %d targets it needs a pass ahead of the step (its scale cannot be applied after it), which is not built for sequence models: mse, mae and nseLoss are", h->net.T);
            HIPCHK(h, hipSetDevice(h->device));
            FLUSH(h);
            h->net.loss = (int)value;
            h->net.loss_t = 0;
            for (int t = 0; t < h->net.T; ++t) h->net.loss_t |= (unsigned)value << (4 * t);
            return EH_OK;
        }
    }
    if (h->bnl) {                            // BatchNorm layers in the chain: always the layer-wise step + reduce pair, fp32
        if (!strcmp(name, "fused_update")) {
            if (value < 0 || value > 2) return fail(h, EH_EINVAL, "fused_update must be 0, 1 or 2");
            if (value == 1) return fail(h, EH_EUNSUPPORTED, "fused_update: the one-kernel step is not built for BatchNorm layers in the chain (they run the layer-wise step + reduce pair)");
            return EH_OK;                    // (2 = "where it is reproducible": the pair is)
        }
        if (!strcmp(name, "multi_step") || !strcmp(name, "specialize") || !strcmp(name, "precision")) {
            if (value) return fail(h, EH_EUNSUPPORTED, "%s: not built for BatchNorm layers in the chain (fp32 layer-wise form, one step per launch sequence)", name);
            return EH_OK;
        }
    } else if (h->lnl) {                     // LayerNorm layers (and no BatchNorm layer): the same pair, the same refusals
        if (!strcmp(name, "fused_update")) {
            if (value < 0 || value > 2) return fail(h, EH_EINVAL, "fused_update must be 0, 1 or 2");
            if (value == 1) return fail(h, EH_EUNSUPPORTED, "fused_update: the one-kernel step is not built for LayerNorm layers in the chain (they run the layer-wise step + reduce pair)");
            return EH_OK;
        }
        if (!strcmp(name, "multi_step") || !strcmp(name, "specialize") || !strcmp(name, "precision")) {
            if (value) return fail(h, EH_EUNSUPPORTED, "%s: not built for LayerNorm layers in the chain (fp32 layer-wise form, one step per launch sequence)", name);
            return EH_OK;
        }
    }
    if (h->lform && (!strcmp(name, "fast_paths") || !strcmp(name, "row_split") || !strcmp(name, "variant") || !strcmp(name, "precision"))) {
        if (!strcmp(name, "precision") && value) return fail(h, EH_EUNSUPPORTED, "precision: the layer-wise form computes in fp32");
        return EH_OK;                        // tile / kernel-family knobs of the fused kernels: nothing to choose in the layer-wise form
    }
    if (h->drop_on && value && (!strcmp(name, "precision") || !strcmp(name, "row_split")))
        return fail(h, EH_EUNSUPPORTED, "%s: dropout is built for the fp32 per-wave kernels only (eh_set_dropout with all rates zero removes it)", name);
    if (!strcmp(name, "lbfgs_one_max")) {    // n_theta up to which an L-BFGS evaluation's dots + decision + update run as one launch (-1: the measured default; A/B, tests)
        if (value < -1 || value > INT32_MAX) return fail(h, EH_EINVAL, "lbfgs_one_max must be -1 or a parameter count");
        h->lb_one_max = (int)value;
        return EH_OK;
    }
    if (!strcmp(name, "max_blocks")) {
        if (value < 1 || value > 256) return fail(h, EH_EINVAL, "max_blocks must be 1..256 (one workgroup per CU)");
        h->max_blocks = (int)value;
        return EH_OK;
    }
    if (!strcmp(name, "bn_in_kernel")) {     // 0: always launch eh_bn_stats_kernel in front of a step with input BatchNorm (A/B, tests); 1 (default): small minibatches take their statistics inside the step kernel
        h->bn_no_self = value == 0;
        return EH_OK;
    }
    if (!strcmp(name, "multi_step")) {       // 1 (default): eh_train_epoch runs the steps of small minibatches (one workgroup each) several per launch; 0: one launch per step
        h->multi_step = value != 0;
        return EH_OK;
    }
    if (!strcmp(name, "eval_blocks")) {      // workgroups of the evaluation passes (eh_eval / eh_forward); 0 = the default of the kernel family
        if (value < 0 || value > 4096) return fail(h, EH_EINVAL, "eval_blocks must be 0 (default) .. 4096");
        h->eval_blocks = (int)value;
        return EH_OK;
    }
    if (!strcmp(name, "mech_blocks")) {      // workgroups of the stand-alone mechanistic stage (eh_mech_loss_vjp): rows of partials the finish kernel folds
        if (value < 0 || value > EH_MECH_MAXROWS) return fail(h, EH_EINVAL, "mech_blocks must be 0 (no cap) .. %d", (int)EH_MECH_MAXROWS);
        h->mech_blocks = (int)value;
        return EH_OK;
    }
    if (!strcmp(name, "mech_tiles")) {       // consecutive tiles (1 024 samples each) per workgroup of the stand-alone mechanistic stage
        if (value < 1 || value > 1024) return fail(h, EH_EINVAL, "mech_tiles must be 1..1024");
        h->mech_tiles = (int)value;
        return EH_OK;
    }
    if (!strcmp(name, "fast_paths")) {       // 0 forces the generic MFMA kernels (A/B testing)
        const int want = fast_wanted(h->arch, h->net.K, h->net.P, h->net.T, h->net.mech);
        h->fast_user = value ? (int)value : 0;
        h->fast = (h->net.loss >= EH_LOSS_PEARSONLOSS) ? 0 : (want & h->fast_user);
        HIPCHK(h, hipSetDevice(h->device));
        FLUSH(h);
        return build_maps(h, false);
    }
    if (!strcmp(name, "fused_update")) {     // 1: one kernel per step (float-atomic accumulation, not bitwise reproducible)
        if (value && two_pass_mask(h->net)) return fail(h, EH_EUNSUPPORTED, "fused_update: rmse (on a multi-target model) / pearson / kge training losses take forward passes ahead of the step");
        if (value && (h->img.l2c != 0.0f || h->img.l2w)) return fail(h, EH_EUNSUPPORTED, "fused_update: the weight_l2 extra loss is not built for it");
        if (value && h->arch->wide) return fail(h, EH_EUNSUPPORTED, "fused_update is not built for hidden widths above 64");
        if (!value && h->p2p_alloc) return fail(h, EH_ESTATE, "fused_update: eh_p2p_disable first");
        if (value < 0 || value > 2) return fail(h, EH_EINVAL, "fused_update must be 0, 1 or 2");
        if (value == 1 && h->chain.n) return fail(h, EH_EUNSUPPORTED, "fused_update: the one-kernel step is not built for an optimiser chain (ClipNorm needs the norm of the whole gradient before any element moves): 0 or 2 run the step + reduce + chain kernels");
        HIPCHK(h, hipSetDevice(h->device));
        FLUSH(h);
        h->fused = value != 0;
        // 2 = "where it is reproducible": the float-atomic one-kernel step only for minibatches ONE workgroup covers -- its sums meet in one
        // fixed order (several steps per launch with the state in LDS, or one add per accumulator) -- and for every larger minibatch the
        // ordered one-kernel step (EH_MODE_TRAIN_ORD, ord_ok) or, where that is not built, the deterministic step + reduce pair: the same bits.  What train() asks for when random_seed is set
        // (the reference's default, src/config/TrainingConfig.jl:85-86: a seeded CPU run IS reproducible).
        h->fused_det = value == 2;
        return EH_OK;
    }
    if (!strcmp(name, "training_loss")) {
        if (value < EH_LOSS_MSE || value > EH_LOSS_PROGRAM) return fail(h, EH_EUNSUPPORTED, "training_loss %lld is not implemented on the device", (long long)value);
        if (value == EH_LOSS_PROGRAM)
            for (int t = 0; t < h->net.T; ++t)
                if (!h->loss_prog.has(t)) return fail(h, EH_ESTATE, "training_loss EH_LOSS_PROGRAM: call eh_set_loss_program first");
        const bool two = (value >= EH_LOSS_PEARSONLOSS && value <= EH_LOSS_PBKGELOSS) || (value == EH_LOSS_RMSE && h->net.T > 1);
        if (two && h->fused) return fail(h, EH_EUNSUPPORTED, "rmse (on a multi-target model) / pearson / kge training losses take forward passes ahead of the step: switch fused_update off first");
        HIPCHK(h, hipSetDevice(h->device));
        FLUSH(h);
        h->net.loss = (int)value;
        h->net.loss_t = 0;
        for (int t = 0; t < h->net.T; ++t) h->net.loss_t |= (unsigned)value << (4 * t);
        if (!h->lform) {   // the two-pass losses exist in the generic kernels only (the K == 1 / P <= 4 fast paths stay untouched by them)
            const int want = fast_wanted(h->arch, h->net.K, h->net.P, h->net.T, h->net.mech);
            const int fast = (two || value >= EH_LOSS_PEARSONLOSS) ? 0 : (want & h->fast_user);
            if (fast != h->fast) { h->fast = fast; return build_maps(h, false); }
        }
        return EH_OK;
    }
    if (!strcmp(name, "jit")) {              // recorded closures: 1 = kernels compiled at run time around the program (default), 0 = the interpreter
        h->jit_on = value != 0;
        return EH_OK;
    }
    if (!strcmp(name, "agg") || !strcmp(name, "extra_terms")) {
        // `agg::Function` of the training configuration (src/config/TrainingConfig.jl:76-77): the training loss is
        // agg([agg(per-target losses), extra loss entries...]) (src/losses/compute_loss.jl:31-34,50-53).  0 = sum (default), 1 = mean;
        // "extra_terms" = the number of entries the extra loss returns (what eh_set_weight_l2 / eh_set_weight_l2_coef stand for: one
        // entry, or as many weight_l2 terms as the host folded into the coefficients) -- only `mean` needs it.
        if (!strcmp(name, "agg")) { if (value != 0 && value != 1) return fail(h, EH_EINVAL, "agg must be 0 (sum) or 1 (mean)"); }
        else if (value < 0 || value > 64) return fail(h, EH_EINVAL, "extra_terms must be 0..64");
        HIPCHK(h, hipSetDevice(h->device));
        FLUSH(h);                                 // (a pending fused update was computed under the old setting)
        if (!strcmp(name, "agg")) h->agg = (int)value; else h->n_extra = (int)value;
        eh_agg_factors(h);
        return EH_OK;
    }
    if (!strcmp(name, "check_idx")) {        // debug: range-check minibatch indices that live on the DEVICE (eh_train_step, idx_on_device != 0) before every step --
        h->check_idx = value != 0;           // a small kernel + one synchronisation per step; host indices are always checked
        return EH_OK;
    }
    if (!strcmp(name, "p2p_mode")) {         // who publishes a step's sums to the peers (EhP2P::mode, eh_device.hpp): 0 = the step's last workgroup to finish, elected by a
                                             // two-level ticket; 1 = workgroup 0 of the next kernel on the stream, no election.  EVERY rank switches at the same step.
        if (value != 0 && value != 1) return fail(h, EH_EINVAL, "p2p_mode must be 0 (election in the step's epilogue) or 1 (publish from the next kernel's prologue)");
        if (!h->p2p_on) return fail(h, EH_ESTATE, "p2p_mode: no peer-to-peer exchange on this handle (eh_p2p_init / eh_p2p_init_local first)");
        HIPCHK(h, hipSetDevice(h->device));
        FLUSH(h);                                // (no step pending across the switch: whoever was to publish it has done so)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->p2p_host.mode = (int)value;
        HIPCHK(h, hipMemcpy(h->p2p_dev, &h->p2p_host, sizeof(EhP2P), hipMemcpyHostToDevice));
        return EH_OK;
    }
    if (!strcmp(name, "empty_target_nan")) { // a target with no valid sample inside a batch that has some: the gradient is the reference's either way (that target adds
        h->empty_nan = value != 0;           // nothing); the VALUE is the sum of the other targets (0, default) or the reference's NaN = mean over an empty selection
        return EH_OK;                        // (1; src/losses/loss_fn.jl:61-63), reported by eh_loss_and_grad -- the seam where the reference's objective is called directly
    }
    if (!strcmp(name, "lean")) {             // 0 = never the lean form of the single-step train kernels (eh_lean_fold, eh_device.hpp): the general kernel, A/B
        h->lean = value != 0;
        return EH_OK;
    }
    if (!strcmp(name, "aot_spec")) {         // 0 = never the kernels specialised ahead of time for the canonical descriptors (eh_spec.hip): tests of the other paths, A/B
        h->aot_spec = value != 0;
        return EH_OK;
    }
    if (!strcmp(name, "specialize")) {       // 1 = step kernels compiled at run time with the model descriptor as a compile-time constant;
        h->specialize = value != 0;          // 2 = the same in a background thread: steps run the kernels built ahead of time until the
        h->specialize_async = value == 2;    //     compiled one is ready (~1 s, or a disk-cache hit), then switch -- same arithmetic, same results
        return EH_OK;
    }
    if (!strcmp(name, "row_split")) {        // A/B: the row-split kernel family (eh_wide.hpp) where both are built
        const bool now = h->arch->wide != 0;
        if ((value != 0) == now) return EH_OK;
        if (!h->arch_alt) return fail(h, EH_EUNSUPPORTED, "row_split: this model has only the %s kernel", now ? "row-split" : "per-wave");
        if (value && h->fused) return fail(h, EH_EUNSUPPORTED, "row_split: switch fused_update off first");
        if (h->arch->var[h->variant].bf16) return fail(h, EH_ESTATE, "row_split: the bf16-forward kernels exist in the row-split family only (set precision 0 first)");
        HIPCHK(h, hipSetDevice(h->device));
        FLUSH(h);
        std::swap(h->arch, h->arch_alt);
        h->variant = (h->arch->nvar > 1 && !h->arch->wide) ? 1 : 0;
        h->fast = (h->net.loss >= EH_LOSS_PEARSONLOSS) ? 0 : (fast_wanted(h->arch, h->net.K, h->net.P, h->net.T, h->net.mech) & h->fast_user);
        for (int vi = 0; vi < h->arch->nvar; ++vi) HIPCHK(h, h->arch->var[vi].prepare());
        return build_maps(h, false);
    }
    if (!strcmp(name, "precision")) {        // 0 = fp32 end to end (the reference's arithmetic); eh_wide_bf16.hpp: 1 = bf16 forward products, fp32 accumulate, fp32-exact
                                             // backward; 2 = bf16 operands in both passes (every backward delta rounded once), fp32 accumulate
        if (value < 0 || value > 2) return fail(h, EH_EINVAL, "precision must be 0 (f32), 1 (bf16 forward / fp32-exact backward) or 2 (bf16 operands in both passes, fp32 accumulate)");
        const int now = h->arch->var[h->variant].bf16;
        if ((int)value == now) return EH_OK;
        if (value) {
            if (h->act == EH_ACT_SWISH || h->act == EH_ACT_PER_NET)
                return fail(h, EH_EUNSUPPORTED, "precision: the bf16 kernels keep only the rounded activation (tanh / sigmoid / relu / identity; not swish, not per-net activations)");
            if (h->fused) return fail(h, EH_EUNSUPPORTED, "precision: switch fused_update off first (the row-split kernels have no such mode)");
            const EhArchInfo* W = h->arch->wide ? h->arch : h->arch_alt;
            // one network (the slab row in plain canonical order): the sample-owned training kernel (eh_bf16_sample.hpp); else the row-split one
            const bool so_ok = so_allowed(h);
            int vb = -1;
            if (W && so_ok) for (int vi = 0; vi < W->nvar; ++vi) if (W->var[vi].bf16 == (int)value && W->var[vi].so) { vb = vi; break; }
            if (W && vb < 0) for (int vi = 0; vi < W->nvar; ++vi) if (W->var[vi].bf16 == (int)value && !W->var[vi].so) { vb = vi; break; }
            if (vb < 0) return fail(h, EH_EUNSUPPORTED, "precision: no bf16 kernel is built for this shape (row-split shapes only: hidden width 33..128)");
            HIPCHK(h, hipSetDevice(h->device));
            FLUSH(h);
            if (W != h->arch) { std::swap(h->arch, h->arch_alt); h->fast = 0; }
            h->variant = vb;
            for (int vi = 0; vi < h->arch->nvar; ++vi) HIPCHK(h, h->arch->var[vi].prepare());
        } else {
            HIPCHK(h, hipSetDevice(h->device));
            FLUSH(h);
            h->variant = 0;
        }
        return build_maps(h, false);
    }
    if (!strcmp(name, "variant")) {
        if (value < 0 || value >= h->arch->nvar) return fail(h, EH_EINVAL, "variant must be 0..%d for this shape", h->arch->nvar - 1);
        if (h->arch->var[value].bf16 != h->arch->var[h->variant].bf16) return fail(h, EH_EINVAL, "variant %lld belongs to the other precision (set the \"precision\" option)", (long long)value);
        if (h->arch->var[value].so && !so_allowed(h))
            return fail(h, EH_EUNSUPPORTED, "variant %lld is the sample-owned training kernel: one-network models only (and not with EH_NO_DIRECT_STORE / EH_NO_SAMPLE_OWNED set)", (long long)value);
        h->variant = (int)value;
        HIPCHK(h, hipSetDevice(h->device));      // the reduction map depends on the variant (waves of a row-split workgroup; layout of the parked accumulators)
        return build_maps(h, false);
    }
    return fail(h, EH_EINVAL, "unknown option %s", name);
}

int32_t eh_set_params(eh_handle* h, const float* theta, int64_t n) {
    if (!h || !theta) return EH_EINVAL;
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_set_params: n = %lld, model has %d", (long long)n, h->net.n_theta);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (int rc = eh_copy_in(h, TH(h), theta, (size_t)n)) return rc;
    hipLaunchKernelGGL(eh_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, TH(h), (int)n, h->img);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EH_OK;
}

int32_t eh_get_params(eh_handle* h, float* theta, int64_t n) {
    if (!h || !theta) return EH_EINVAL;
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_get_params: n = %lld, model has %d", (long long)n, h->net.n_theta);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return eh_copy_out(h, theta, TH(h), (size_t)n);
}

}   // extern "C"

// ---- internal launch helpers ---------------------------------------------------------------------
static int ensure_events(eh_handle* h, size_t need) {
    while (h->ev.size() < need) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->ev.push_back(e);
    }
    return EH_OK;
}
// eh_profile_enable: three events per bracket -- before the step kernel, between it and the reduction, after -- around every step, or
// (stride S > 1) around every burst of S consecutive steps, the middle one then at the burst's end.  prof_begin in front of a step's
// first launch, prof_end behind its last; mid_marked: the caller has recorded the middle event itself (eh_do_step, stride 1)
struct EhProf { bool on, burst, last; };
static int prof_begin(eh_handle* h, EhProf* p) {
    p->on = h->prof && h->ev_used + 3 <= 3 * 8192;
    p->burst = h->prof_stride > 1;
    p->last = h->prof_k % h->prof_stride == h->prof_stride - 1;
    if (!p->on) return EH_OK;
    if (int rc = ensure_events(h, h->ev_used + 3)) return rc;
    if (h->prof_k % h->prof_stride == 0) HIPCHK(h, hipEventRecord(h->ev[h->ev_used], h->stream));
    h->prof_k++;
    return EH_OK;
}
static int prof_end(eh_handle* h, const EhProf& p, bool mid_marked) {
    if (!p.on || !p.last) return EH_OK;
    if (!mid_marked) HIPCHK(h, hipEventRecord(h->ev[h->ev_used + 1], h->stream));
    HIPCHK(h, hipEventRecord(h->ev[h->ev_used + 2], h->stream));
    h->ev_used += 3;
    return EH_OK;
}
static int grid_for(const eh_handle* h, long long count) {
    const EhVariant& v = h->arch->var[h->variant];
    const long long mt = 16LL * v.nt;
    const long long ntiles = (count + mt - 1) / mt;
    return (int)std::max<long long>(1, std::min<long long>((ntiles + (v.tiles ? v.tiles : v.nw) - 1) / (v.tiles ? v.tiles : v.nw), h->max_blocks));
}

// The evaluation passes hold no gradient accumulators: the per-wave kernels need a quarter to a half of the registers of their training
// form (headline shape: 60 against 128 VGPRs), so several workgroups fit a CU, and a forward over a whole split is a long chain of
// dependent per-tile latencies that more resident waves hide.  The row-split kernels fill a CU's LDS with one workgroup: no gain, and every
// extra workgroup pays the image prologue again.  The metric rows (EH_EVAL_STATS * T floats per workgroup) fit the slab's 4 MB floor.
static int eval_grid_for(const eh_handle* h, long long count) {
    const EhVariant& v = h->arch->var[h->variant];
    const long long mt = 16LL * v.nt, per = v.tiles ? v.tiles : v.nw;
    const long long ntiles = (count + mt - 1) / mt;
    int cap = h->max_blocks;
    if (h->eval_blocks > 0) cap = h->eval_blocks;
    else if (!h->arch->wide && h->max_blocks == 256) cap = EH_EVAL_BLOCKS;
    // Every lane sums its samples' statistics sequentially in fp32, the valid count among them, and the workgroup's sum is fp32 too: a
    // floor on the grid keeps a wave at EH_EVAL_TILES tiles or fewer, whatever cap "eval_blocks" sets, so the count stays exact (a
    // workgroup's fp32 count is not above 2^24) and the rounding of the sums bounded.  The floor stays within the slab's 4 MB of metric
    // rows (EH_EVAL_COPY); the default grids of the splits the benchmarks use are above it.
    const long long floor = std::min<long long>((ntiles + per * EH_EVAL_TILES - 1) / (per * EH_EVAL_TILES), (1LL << 20) / (EH_EVAL_STATS * EH_MAX_TARG));
    return (int)std::max<long long>(std::max<long long>(1, floor), std::min<long long>((ntiles + per - 1) / per, cap));
}

// per-target weights of the minibatch (1 / n_t, 1 / sum (y - ybar)^2) -> inv_n; tcount (eh_dp_counts): the shard's raw sums as well
int eh_launch_count(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, float* tcount) {
    const EhNet& net = h->net;
    hipLaunchKernelGGL(eh_count_kernel, dim3(net.T), dim3(256), 0, h->stream, sp.recs, h->plan.C, net.P + net.F, net.T, idx, first, count, h->inv_n, net.loss_t, sp.shift4(), h->img.agg_a, h->roles, h->img.l2s, tcount);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}
// two-pass losses: `nrows` rows of moment sums about the shift (the slab of a forward-only pass, or the all-reduced EH_BUF_MOMENT) -> the
// centre of yhat; the rows of the pass about that centre -> k0 k1 k2 and the loss value of every two-pass target, all in inv_n
int eh_launch_moment_centre(eh_handle* h, const EhSplit& sp, const float* rows, int nrows) {
    hipLaunchKernelGGL(eh_moment_centre_kernel, dim3(h->net.T), dim3(64), 0, h->stream, rows, nrows, h->net.T, h->net.loss_t, sp.shift4(), h->inv_n);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}
int eh_launch_moment_coef(eh_handle* h, const EhSplit& sp, const float* rows, int nrows) {
    hipLaunchKernelGGL(eh_moment_coef_kernel, dim3(h->net.T), dim3(64), 0, h->stream, rows, nrows, h->net.T, h->net.loss_t, sp.shift4(), h->inv_n, h->img.agg_a);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}

// input BatchNorm: statistics of the minibatch [first, first+count) -> a.bn_* (train-mode kernels only)
// consume = false: a forward-only pass in front of the step's training pass (eh_dp_moments) -- the global statistics stay for the passes behind it
int eh_bn_prepare(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, bool update, EhStepArgs* a, bool consume) {
    a->bn_part = nullptr; a->bn_nblk = 0; a->bn_update = 0; a->bn_run = h->bn_run; a->image_out = h->image;
    a->bn_c = nullptr; a->bn_n = nullptr;
    if (!h->bn_on) return EH_OK;
    if (h->bn_ext) {          // statistics of the GLOBAL batch, summed over the GPUs by the host since eh_dp_bn_stats
        a->bn_part = h->bn_stat; a->bn_nblk = 1; a->bn_c = h->bn_shift; a->bn_n = h->bn_stat + 64;
        a->bn_update = (update || h->bn_dp_update) ? 1 : 0;
        if (consume) { h->bn_ext = false; h->bn_dp_update = false; }
        return EH_OK;
    }
    if (count <= 0) return EH_OK;
    if (!h->arch->wide && !h->lform && count <= EH_BN_SELF_MAX && !h->bn_no_self) {      // small minibatch, per-wave kernel: the step kernel takes the statistics itself
        a->bn_nblk = -1; a->bn_update = update ? 1 : 0;
        return EH_OK;
    }
    const int nblk = (int)std::max<long long>(1, std::min<long long>(32, (count + 1023) / 1024));
    hipLaunchKernelGGL(eh_bn_stats_kernel, dim3(nblk), dim3(1024), 0, h->stream, sp.recs, h->plan.C, h->net.P, idx, (int)first, (int)count, h->bn_part, nullptr);
    HIPCHK(h, hipGetLastError());
    a->bn_part = h->bn_part; a->bn_nblk = nblk; a->bn_c = h->bn_part + nblk * 64; a->bn_update = update ? 1 : 0;
    return EH_OK;
}

// targets whose training loss takes two forward passes ahead of the training pass (batch statistics of yhat): bit t
static unsigned two_pass_mask(const EhNet& net) {
    unsigned m = 0;
    for (int t = 0; t < net.T; ++t) {
        const unsigned k = (net.loss_t >> (4 * t)) & 15u;
        if ((k >= (unsigned)EH_LOSS_PEARSONLOSS && k <= (unsigned)EH_LOSS_PBKGELOSS) || (k == (unsigned)EH_LOSS_RMSE && net.T > 1)) m |= 1u << t;
    }
    return m;
}
unsigned eh_two_pass_mask(const eh_handle* h) { return two_pass_mask(h->net); }
// ---- sequence models (eh_seq.hpp) --------------------------------------------------------------------------------------------
constexpr long long EH_SEQ_WS_CAP = 256ll << 20;      // bytes of backward workspace at most: fewer workgroups are launched when it binds
static int seq_grid_for(const eh_handle* h, const EhSplit& sp, long long count, bool train) {
    const long long ntiles = (count + 15) / 16;
    long long grid = std::max<long long>(1, std::min<long long>((ntiles + EH_SEQ_NW - 1) / EH_SEQ_NW, std::min(h->max_blocks, h->slab_rows)));
    if (train) grid = std::max<long long>(1, std::min<long long>(grid, EH_SEQ_WS_CAP / (4 * EH_SEQ_NW * eh_seq_ws_floats(h->plan.seq_nbh, sp.W, sp.ow, h->plan.seq_cell))));
    return (int)grid;
}
static EhSeqArgs seq_args(const eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count) {
    EhSeqArgs a{};
    a.recs = sp.recs; a.C = h->plan.C; a.starts = sp.starts; a.idx = idx; a.first = first; a.count = count;
    a.W = sp.W; a.ow = sp.ow; a.lam = sp.lam;
    a.theta = TH(h); a.meta = h->image + h->arch->phi_off; a.slab = h->slab; a.n_acc = h->n_acc;
    a.shift = sp.shift[0];
    for (int t = 0; t < EH_MAX_TARG; ++t) a.shift_t[t] = sp.shift[t];
    a.inv_n = h->net.T > 1 ? h->inv_n : nullptr;
    a.I = h->plan.seq_I; a.H = h->plan.seq_H; a.act_in = h->plan.seq_act_in; a.act_hd = h->plan.seq_act_hd; a.act_cell = h->plan.seq_act_cell;
    for (int k = 0; k < EH_SEQ_NOFF; ++k) a.off[k] = h->plan.seq_off[k];
    a.prog = h->prog;
    return a;
}
// A sequence model around a recorded closure: its (NBI, NBH) kernels compiled at run time around the generated program (eh_jit.hpp), built
// on first use.  nullptr = not wanted ("jit" = 0) or not available: a build that fails is reported by eh_jit_status and the handle goes on
// with the interpreting kernels built ahead of time.
static eh_handle_s::JitEntry* seq_jit_entry(eh_handle* h) {
    if (h->net.mech != EH_MECH_PROGRAM || !h->jit_on || h->jit_failed) return nullptr;
    if (!h->jit.empty()) return h->jit[0]->state.load(std::memory_order_acquire) > 0 ? h->jit[0].get() : nullptr;
    h->jit.emplace_back(new eh_handle_s::JitEntry());
    eh_handle_s::JitEntry* je = h->jit.back().get();
    je->arch = h->arch; je->variant = 0; je->fast = 0; je->spec = false; je->p2p = false; je->net = h->net; je->loss_gen = 0;
    const bool ok = eh_jit_build_seq(h->desc, h->plan.seq_nbi, h->plan.seq_nbh, h->plan.seq_cell, h->net.T > 1, &je->k, &je->log);
    je->state.store(ok ? 1 : -1, std::memory_order_release);
    if (!ok) { h->jit_log = je->log; h->jit_failed = true; return nullptr; }
    return je;
}
// The compiled kernels take over from the interpreter once their training pass has agreed with it on a minibatch of the user's own data:
// both run the pass (nothing but slab and workspace is written), and loss sum, valid count and un-normalised gradient, summed over the
// slab rows, must agree to 1e-5 of the gradient's largest entry (jit_verify's bar).  The two are the same arithmetic, but the compiled one
// is another binary from another compiler run, at the register pressure of these kernels (the run-time compiler that ships with PyTorch
// spills in TRAIN at NBI = NBH = 2, where the one of the build does not); the build's own errors only catch refusals.  On disagreement the
// handle stays on the interpreter and says so in eh_jit_status.  A minibatch without a valid target decides nothing: the next one does.
// Several targets: the row is [gradient | loss | n_1 .. n_T] under the weights of the count pre-pass (which has run: both passes read the
// same table); the loss column and all T count columns are compared, and a minibatch in which no target has a valid entry is the one skipped.
static void seq_jit_verify(eh_handle* h, eh_handle_s::JitEntry* je, int grid, const EhSeqArgs& a) {
    const EhNet& net = h->net;
    const size_t n = (size_t)grid * a.n_acc;
    std::vector<float> part[2] = {std::vector<float>(n), std::vector<float>(n)};
    bool ran = true;
    for (int k = 0; k < 2 && ran; ++k) {
        ran = (k == 0 ? eh_seq_launch(h->plan.seq_nbi, h->plan.seq_nbh, EH_SEQ_TRAIN, EH_SEQ_HEAD_PROG, grid, h->stream, net, a, h->plan.seq_cell, net.T > 1)
                      : eh_jit_launch_seq(&je->k, EH_SEQ_TRAIN, grid, h->stream, &net, &a)) == hipSuccess &&
              hipMemcpyAsync(part[k].data(), a.slab, n * sizeof(float), hipMemcpyDeviceToHost, h->stream) == hipSuccess;
    }
    ran = ran && hipStreamSynchronize(h->stream) == hipSuccess;
    std::string why;
    if (!ran) { (void)hipGetLastError(); why = "the run-time compiled sequence kernel could not be run next to the interpreter: the handle keeps the interpreter"; }
    else {
        auto col = [&](int k, int i) { double s = 0; for (int b = 0; b < grid; ++b) s += part[k][(size_t)b * a.n_acc + i]; return s; };
        double gmax = 0.0, dmax = 0.0;
        for (int i = 0; i < net.n_theta; ++i) { const double x = col(0, i), y = col(1, i); gmax = std::max(gmax, fabs(x)); dmax = std::max(dmax, fabs(x - y)); }
        const double sa = col(0, net.n_theta), sb = col(1, net.n_theta) * (getenv("EH_DEBUG_JIT_SKEW") ? 1.01 : 1.0);      // (tests: the fall-back path)
        bool counts = true;
        double ntot = 0.0;
        for (int t = 0; t < net.T; ++t) { counts = counts && col(0, net.n_theta + 1 + t) == col(1, net.n_theta + 1 + t); ntot += col(0, net.n_theta + 1 + t); }
        if (counts && ntot == 0.0) return;
        if (dmax <= 1e-5 * gmax + 1e-30 && fabs(sa - sb) <= 1e-5 * fabs(sa) + 1e-30 && counts && std::isfinite(gmax)) { je->verified = true; return; }
        char b[320];
        snprintf(b, sizeof b, "the sequence kernel compiled at run time disagrees with the interpreter on %lld windows of this model's data (gradient: max |difference| %.3g "
                 "against a largest entry of %.3g; loss sum %.9g vs %.9g; valid counts %s): the handle keeps the interpreter", a.count, dmax, gmax, sb, sa, counts ? "equal" : "DIFFERENT");
        why = b;
    }
    je->state.store(-1); h->jit_failed = true; h->jit_log = why;
}
static hipError_t seq_launch(eh_handle* h, int mode, int grid, const EhSeqArgs& a) {
    if (eh_handle_s::JitEntry* je = seq_jit_entry(h)) {
        if (mode == EH_SEQ_TRAIN && !je->verified) seq_jit_verify(h, je, grid, a);
    }
    if (eh_handle_s::JitEntry* je = seq_jit_entry(h)) {
        const hipError_t e = eh_jit_launch_seq(&je->k, mode, grid, h->stream, &h->net, &a);
        if (e == hipSuccess) return e;
        (void)hipGetLastError();
        je->state.store(-1); h->jit_failed = true;
        h->jit_log = std::string("launch of the run-time compiled sequence kernel failed: ") + hipGetErrorString(e);
    }
    const int head = h->net.mech == EH_MECH_PROGRAM ? EH_SEQ_HEAD_PROG : (h->net.n_out > 1 ? EH_SEQ_HEAD_MULTI : EH_SEQ_HEAD_MECH);
    return eh_seq_launch(h->plan.seq_nbi, h->plan.seq_nbh, mode, head, grid, h->stream, h->net, a, h->plan.seq_cell, h->net.T > 1);
}
// several targets: the per-target weights of this minibatch of windows -> inv_n (eh_seq_count_kernel), ahead of the training pass
static int seq_launch_count(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count) {
    const EhNet& net = h->net;
    hipLaunchKernelGGL(eh_seq_count_kernel, dim3(net.T), dim3(EH_SEQ_COUNT_NT), 0, h->stream, sp.recs, h->plan.C, net.P + net.F, sp.starts, idx, first, count, sp.W, sp.ow, sp.lam,
                       h->inv_n, net.loss_t, sp.shift4(), h->img.agg_a);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}
static int seq_train(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, int* grid_out) {
    if (!sp.starts) return fail(h, EH_ESTATE, "sequence model: no windows for this split (call eh_set_sequences after eh_set_data)");
    const int grid = seq_grid_for(h, sp, count, true);
    EhSeqArgs a = seq_args(h, sp, idx, first, count);
    a.ws_wave = eh_seq_ws_floats(h->plan.seq_nbh, sp.W, sp.ow, h->plan.seq_cell);
    const long long need = (long long)grid * EH_SEQ_NW * a.ws_wave;      // sized by the grid actually launched
    if (need > h->seq_ws_floats) { if (int rc = eh_grow(h, &h->seq_ws, &h->seq_ws_floats, need)) return rc; }
    a.ws = h->seq_ws;
    *grid_out = grid;
    if (h->net.T > 1) { if (int rc = seq_launch_count(h, sp, idx, first, count)) return rc; }
    HIPCHK(h, seq_launch(h, EH_SEQ_TRAIN, grid, a));
    return EH_OK;
}

// what a training launch returned -> status.  A handle with dropout has no kernel but the one compiled at run time: where that one
// is missing (the build failed: step_launch answers hipErrorNotSupported) the step fails with the compiler's log; any other HIP error
// keeps its own code
static int train_launch_status(eh_handle* h, hipError_t e) {
    if (e == hipErrorNotSupported && h->drop_on) {
        (void)hipGetLastError();
        return fail(h, EH_EUNSUPPORTED, "dropout: the step kernel is compiled at run time and there is no other: %s", h->jit_log.empty() ? "no log" : h->jit_log.c_str());
    }
    HIPCHK(h, e);
    return EH_OK;
}
static int launch_train_kernel(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, int* grid_out, bool bn_update) {
    if (h->seq) return seq_train(h, sp, idx, first, count, grid_out);
    if (h->lform) return eh_lform_train(h, sp, idx, first, count, grid_out, bn_update);
    const EhNet& net = h->net;
    if (net.T > 1 && !h->dp_weights) {
        if (int rc = eh_launch_count(h, sp, idx, first, count)) return rc;
    }
    const bool moment_loss = two_pass_mask(net) != 0;
    if (moment_loss && !h->dp_moments) {      // (data-parallel step: eh_dp_grad has just made the coefficients from the moments of the GLOBAL batch)
        // forward-only passes (train-mode BatchNorm statistics included): the batch mean of yhat, then the moments of
        // (yhat, y) about the means -> the coefficients of the per-sample d loss / d yhat that the training pass multiplies
        // into the VJP
        EhStepArgs e = eh_step_args(h, sp, idx, first, count);
        e.image = h->image; e.slab = h->slab; e.n_acc = EH_EVAL_STATS * net.T; e.rmap = h->rmap; e.stamps = nullptr;
        e.yld = count;
        if (int rc = eh_bn_prepare(h, sp, idx, first, count, false, &e)) return rc;
        const int egrid = count > 0 ? grid_for(h, count) : 1;
        HIPCHK(h, step_launch(h, EH_MODE_EVAL, egrid, &e));       // -> mean of yhat
        if (int rc = eh_launch_moment_centre(h, sp, h->slab, egrid)) return rc;
        e.inv_n = h->inv_n;                                                                                               // -> moments about it
        HIPCHK(h, step_launch(h, EH_MODE_EVAL, egrid, &e));
        if (int rc = eh_launch_moment_coef(h, sp, h->slab, egrid)) return rc;
    }
    EhStepArgs a = eh_step_args(h, sp, idx, first, count);
    a.image = h->image; a.slab = h->slab; a.n_acc = h->n_acc;
    a.inv_n = (net.T > 1 || moment_loss) ? h->inv_n : nullptr;
    a.rmap = h->rmap;
    // one network on a row-split bf16 kernel: the accumulators go to the slab row straight from the registers (canonical order is plain
    // column-major per layer; eh_wide_bf16.hpp) -- signalled by a null map
    static const bool no_direct = getenv("EH_NO_DIRECT_STORE") != nullptr;      // (A/B switch of the measurement tools)
    if (!no_direct && h->arch->wide && h->arch->var[h->variant].bf16 && h->plan.n_nets == 1 && h->desc.n_nets == 0) a.rmap = nullptr;
    a.stamps = h->stamps;
    a.fz.gacc = nullptr;
    if (h->drop_on) {
        if (moment_loss) return fail(h, EH_EUNSUPPORTED, "dropout: the two-pass training losses (pearsonLoss / kgeLoss / pbkgeLoss, rmse on several targets) take their batch moments in passes without masks: not built");
        eh_drop_set(a, h->drop_seed, h->drop_step);
    }
    if (int rc = eh_bn_prepare(h, sp, idx, first, count, bn_update, &a)) return rc;
    const int grid = grid_for(h, count);
    *grid_out = grid;
    return train_launch_status(h, step_launch(h, EH_MODE_TRAIN, grid, &a));
}

// one fused kernel: prologue applies the previous step's update, epilogue accumulates this step's sums
static int do_fused_step(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, float* loss_slot_for_this_step,
                         bool ord = false, bool* launched = nullptr) {
    if (h->pending && h->pend_ord != ord) FLUSH(h);      // (a pending update is applied by a step of its own kind only)
    EhProf prof;
    if (int rc = prof_begin(h, &prof)) return rc;
    EhStepArgs a = eh_step_args(h, sp, idx, first, count);
    a.image = h->image; a.slab = h->slab; a.n_acc = h->n_acc; a.inv_n = nullptr; a.rmap = h->rmap; a.stamps = h->stamps;
    if (h->net.T > 1) {      // multi-target: the per-target weights (1 / n_t, 1 / sum (y - ybar)^2) have to be known inside the streaming pass
        if (int rc = eh_launch_count(h, sp, idx, first, count)) return rc;
        a.inv_n = h->inv_n;
    }
    EhFused& z = a.fz;
    z.gacc = h->gacc; z.pset = h->pset; z.imap = h->imap; z.loss_slot = h->pending_loss;
    z.gslot = (int)(h->gstep % 3); z.cur = h->cur; z.sc_sel = h->sc_sel; z.pending = h->pending ? 1 : 0; z.opt = h->opt; z.agg_a = h->img.agg_a;
    a.p2p = h->p2p_on ? h->p2p_dev : nullptr;
    if (h->p2p_on) a.p2pv = h->p2p_host;
    a.p2p_seq = h->p2p_on ? ++h->p2p_seq : 0u;
    if (h->drop_on) { eh_drop_set(a, h->drop_seed, h->drop_step); }
    if (int rc = eh_bn_prepare(h, sp, idx, first, count, true, &a)) return rc;
    const int grid = grid_for(h, count);
    const bool was_pending = h->pending;      // (this step's prologue applies that update)
    if (ord) {
        a.ord = ord_args(h, h->cur, h->pending ? h->ord_grid : 0);
        const hipError_t e = step_launch(h, EH_MODE_TRAIN_ORD, grid, &a);
        if (e == hipErrorNotSupported) {          // (no such kernel for this handle: the caller runs the pair)
            if (prof.on) h->prof_k--;
            *launched = false;
            return EH_OK;
        }
        HIPCHK(h, e);
        *launched = true;
        h->ord_grid = grid;
    } else {
        if (int rc = train_launch_status(h, step_launch(h, h->p2p_on ? EH_MODE_TRAIN_P2P : EH_MODE_TRAIN, grid, &a))) return rc;
    }
    if (h->drop_on) h->drop_step++;      // (a training step was launched: the next one draws new masks, applied or not)
    // (the ordered step leaves the accumulator rotation alone: gstep counts the steps that add into gacc)
    h->cur ^= 1; h->sc_sel ^= 1;
    if (!ord) h->gstep++;
    if (was_pending) ++h->upd_site[ord ? EH_UPD_ORD_PROLOGUE : EH_UPD_PROLOGUE];
    h->pending = true;
    h->pend_ord = ord;
    h->pending_loss = loss_slot_for_this_step;
    return prof_end(h, prof, false);
}

// Several fused-update steps in one launch (EH_MODE_TRAIN_MULTI, eh_device.hpp): minibatches one workgroup covers -- the reference's
// default batch of 64 among them -- with the step-to-step state in LDS.
static bool multi_ok(const eh_handle* h, long long batch) {
    if (!h->fused || !h->multi_step || h->lform || h->arch->wide || h->p2p_on || h->prof || h->capturing || h->chain.n || h->drop_on) return false;
    if (h->net.T != 1 || h->net.mech == EH_MECH_PROGRAM || h->net.loss == EH_LOSS_PROGRAM || h->act == EH_ACT_PER_NET) return false;
    if (h->bn_on && (h->bn_ext || h->bn_no_self || batch > EH_BN_SELF_MAX)) return false;
    if (h->arch->var[h->variant].lds_bytes + sizeof(float) * (size_t)eh_ms_extra_floats(h->net.n_theta, h->n_acc, h->opt.tab != nullptr) > EH_LDS_LIMIT) return false;
    if (grid_for(h, batch) != 1) return false;
    if (!spec_lookup(h) && jit_wanted(h, EH_MODE_TRAIN)) {      // a model on kernels compiled at run time: its multi-step kernel, or one launch per step
        eh_handle_s::JitEntry* je = jit_entry(const_cast<eh_handle*>(h));      // (a compiled single-step kernel beats the GENERIC multi-step one: 7.4 against 9.0 us)
        if (je && (!je->verified || !je->k.fn[EH_MODE_TRAIN_MULTI])) return false;
    }
    return true;
}
static int do_fused_multi(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long batch, long long end, int nsteps, float* loss_slots) {
    if (h->pending && h->pend_ord) FLUSH(h);
    EhStepArgs a = eh_step_args(h, sp, idx, first, std::min(batch, end - first));
    a.image = h->image; a.slab = h->slab; a.n_acc = h->n_acc; a.inv_n = nullptr; a.rmap = h->rmap; a.stamps = h->stamps;      // (diagnostic builds: the stamps of the launch's LAST step remain)
    EhFused& z = a.fz;
    z.gacc = h->gacc; z.pset = h->pset; z.imap = h->imap; z.loss_slot = h->pending_loss;
    z.gslot = (int)(h->gstep % 3); z.cur = h->cur; z.sc_sel = h->sc_sel; z.pending = h->pending ? 1 : 0; z.opt = h->opt; z.agg_a = h->img.agg_a;
    a.p2p = nullptr; a.p2p_seq = 0u;
    if (int rc = eh_bn_prepare(h, sp, idx, first, a.count, true, &a)) return rc;       // (input BatchNorm: statistics inside the kernel, multi_ok made sure)
    a.ms_nsteps = nsteps; a.ms_batch = (int)batch; a.ms_end = end; a.ms_loss = loss_slots;
    HIPCHK(h, step_launch(h, EH_MODE_TRAIN_MULTI, 1, &a));
    if (h->pending) ++h->upd_site[EH_UPD_PROLOGUE];      // (the first step's prologue applied it)
    h->upd_site[EH_UPD_MULTI] += nsteps;
    // every step of the launch has applied its own update and written its own loss (eh_ms_apply): nothing is pending behind it; the first
    // step's prologue flipped the parameter set and rotated the accumulator slots once
    h->cur ^= 1; h->sc_sel ^= 1;
    h->gstep += 1;
    h->pending = false;
    h->pending_loss = nullptr;
    return EH_OK;
}

// ---- the seam of eh_ens.hip: what an ensemble needs of this unit's launchers and kernels -------------------------------------------------
// Why the handle cannot carry an ensemble at this batch size, one sentence per cause (empty: it can).  The conditions are multi_ok's --
// an ensemble launch IS the multi-step launch, per member -- minus its one way out (a run-time compiled kernel), plus what the handle
// types that never reach multi_ok would fail on.
std::string eh_ens_refusal(eh_handle* h, long long batch) {
    std::string w;
    auto say = [&](const char* t) { if (!w.empty()) w += " "; w += t; };
    if (h->seq) say("Sequence models train on windows with a kernel family of their own.");
    if (h->lform) say("The model runs in the layer-wise form (no fused step kernel holds it: more than three hidden layers, normalisation layers, or widths above 128).");
    if (!h->seq && !h->lform && h->arch->wide) say(h->arch->var[h->variant].bf16 ? "The model runs on the row-split bf16 kernels, whose step needs several workgroups." : "The model runs on the row-split kernels (hidden widths above 64), whose step is not the one-workgroup step.");
    if (!h->fused) say("The handle is not in fused-update mode (option fused_update).");
    if (!h->multi_step) say("The multi_step option is off.");
    if (h->p2p_on || h->comm || h->lgroup) say("Data parallelism is set up on the handle.");
    if (h->prof) say("Profiling is enabled on the handle.");
    if (h->capturing) say("A graph is being captured.");
    if (h->chain.n) say("An OptimiserChain is installed.");
    if (h->drop_on) say("Dropout needs a step kernel compiled at run time.");
    if (h->net.T != 1) say("Several targets need a counting pass ahead of every step.");
    if (h->net.mech == EH_MECH_PROGRAM) say("A recorded mechanistic closure runs on kernels compiled at run time.");
    if (h->net.loss == EH_LOSS_PROGRAM) say("A recorded loss runs on kernels compiled at run time.");
    if (eh_two_pass_mask(h)) say("The two-pass losses (pearsonLoss, kgeLoss, pbkgeLoss) take two forward passes ahead of every step.");
    if (h->act == EH_ACT_PER_NET) say("Per-net or per-layer activations run on kernels compiled at run time.");
    if (h->bn_on && (h->bn_ext || h->bn_no_self || batch > EH_BN_SELF_MAX)) say("Input BatchNorm takes its statistics inside the step kernel only for minibatches up to 512 samples (and not with bn_in_kernel 0).");
    if (!w.empty()) return w;
    char b[256];
    if (h->arch->var[h->variant].lds_bytes + sizeof(float) * (size_t)eh_ms_extra_floats(h->net.n_theta, h->n_acc, false) > EH_LDS_LIMIT) {
        snprintf(b, sizeof b, "The %d parameters with their optimiser state do not fit the LDS behind the step's work space.", h->net.n_theta);
        say(b);
    }
    if (grid_for(h, batch) != 1) {
        const EhVariant& v = h->arch->var[h->variant];
        snprintf(b, sizeof b, "A minibatch of %lld samples is more than one workgroup covers (%d).", batch, 16 * v.nt * (v.tiles ? v.tiles : v.nw));
        say(b);
    }
    if (!spec_lookup(h) && jit_wanted(h, EH_MODE_TRAIN)) say("The handle runs kernels compiled at run time (option specialize).");
    return w;
}
// the handle's optimiser rule was replaced from outside (eh_ens_load): what follows from it
void eh_opt_changed(eh_handle* h) { if (h->lb) h->lb->active = false; h->chain = EhChain{}; h->chain_gen = 0; lean_refresh(h); }
// one launch: `members` workgroups, each the multi-step launch of its record (eh_ens.hpp); the ahead-of-time specialised kernel where the handle runs one
int eh_ens_launch_train(eh_handle* h, int members, const EhStepArgs* a, const EhEnsMember* mem) {
    // (no way out to the generic kernel where the ahead-of-time one fails to launch: which kernel ran is part of a member's parity with an
    //  ordinary handle, and a failure is the caller's to see)
    const EhSpecKernel* sk = spec_lookup(h);
    if (sk && sk->launch_ens) {
        HIPCHK(h, sk->launch_ens(members, h->stream, &h->net, a, mem));
        h->spec_used = sk;
        return EH_OK;
    }
    const EhVariant& v = h->arch->var[h->variant];
    if (!v.launch_ens) return fail(h, EH_EUNSUPPORTED, "eh_ens_train_epoch: no ensemble kernel for this kernel family");
    HIPCHK(h, v.launch_ens(h->act, KFAST(h), members, h->stream, &h->net, a, mem));
    return EH_OK;
}
// an evaluation pass of the handle's kernels on the arguments as given (a member's image and row list); *grid in: 0 = by count
int eh_ens_launch_eval(eh_handle* h, const EhStepArgs* a, int grid) {
    HIPCHK(h, step_launch(h, EH_MODE_EVAL, grid, a));
    return EH_OK;
}
int eh_ens_eval_grid(const eh_handle* h, long long count) { return count > 0 ? eval_grid_for(h, count) : 1; }
// theta -> a member's parameter image
int eh_ens_launch_image(eh_handle* h, const float* theta, float* image) {
    EhImg im = h->img;
    im.image = image;
    hipLaunchKernelGGL(eh_image_kernel, dim3((unsigned)((h->net.n_theta + 255) / 256)), dim3(256), 0, h->stream, theta, h->net.n_theta, im);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}
// the epoch orders of all members in one launch: order[off_j + i] = rows_j[perm(n_j, seed_j)(i)] (eh_ens_order_kernel)
int eh_ens_launch_order(eh_handle* h, const EhEnsOrder* ord, int members, long long max_n) {
    if (max_n <= 0) return EH_OK;
    hipLaunchKernelGGL(eh_ens_order_kernel, dim3((unsigned)((max_n + 255) / 256), (unsigned)members), dim3(256), 0, h->stream, ord);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}

// The chain kernels (eh_chain.hpp) on the gradient in h->gradbuf.  raw: the data-parallel seam's all-reduced sums (eh_dp_apply), whose
// loss the apply pass writes to loss_slot; otherwise eh_reduce_kernel<false, ...> has written gradient and loss.
static int launch_chain(eh_handle* h, bool raw, float* sc_in, float* sc_out, float* loss_slot) {
    ++h->upd_site[EH_UPD_CHAIN];
    static const int one_env = getenv("EH_CHAIN_ONE") ? atoi(getenv("EH_CHAIN_ONE")) : -1;      // (A/B switch of tools/bench_chain.py: the largest n_theta one workgroup takes)
    const int nt = h->net.n_theta;
    const bool l2 = raw && (h->img.l2c != 0.0f || h->img.l2w);
    const unsigned tp = raw ? two_pass_mask(h->net) : 0u;
    const EhChainSrc src{raw ? 1 : 0, h->net.loss, h->net.T, tp, tp ? h->inv_n : nullptr, l2 ? h->l2val : nullptr};
    unsigned long long* ctr = reinterpret_cast<unsigned long long*>(h->chain_part + EH_CHAIN_PARTS);
    if (h->chain.i_norm < 0) {          // no norm to wait for: one element per thread
        hipLaunchKernelGGL(eh_chain_apply_kernel<false>, dim3((nt + 255) / 256), dim3(256), 0, h->stream, h->gradbuf, nt, TH(h), MM(h), VV(h), sc_in, sc_out, h->opt,
                           h->chain, src, h->img, h->chain_part, 0, loss_slot, ctr);
    } else if (nt <= (one_env >= 0 ? one_env : (int)EH_CHAIN_ONE_MAX)) {
        hipLaunchKernelGGL(eh_chain_apply_kernel<true>, dim3(1), dim3(256), 0, h->stream, h->gradbuf, nt, TH(h), MM(h), VV(h), sc_in, sc_out, h->opt,
                           h->chain, src, h->img, h->chain_part, 0, loss_slot, ctr);
    } else {
        const int nb = std::min<int>(EH_CHAIN_PARTS, (nt + 1023) / 1024);
        hipLaunchKernelGGL(eh_chain_norm_kernel, dim3(nb), dim3(256), 0, h->stream, h->gradbuf, nt, TH(h), h->chain, src, h->img, h->chain_part);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(eh_chain_apply_kernel<false>, dim3((nt + 255) / 256), dim3(256), 0, h->stream, h->gradbuf, nt, TH(h), MM(h), VV(h), sc_in, sc_out, h->opt,
                           h->chain, src, h->img, h->chain_part, nb, loss_slot, ctr);
    }
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}

// "fused_update" 2 on a minibatch of several workgroups: the ordered one-kernel step (EH_MODE_TRAIN_ORD) wherever "fused_update" 1 would be
// allowed and the pair's reduce would run eh_reduce_kernel<true, 16> on slab rows the per-wave kernels wrote -- its bits are that pair's
static bool ord_ok(const eh_handle* h, int grid) {
    static const int cw_env = getenv("EH_REDUCE_CW") ? atoi(getenv("EH_REDUCE_CW")) : 0;      // (the A/B switch of eh_do_step)
    if (!h->fused || !h->fused_det || !h->ord || grid <= 1 || grid > (int)EH_ORD_ROWS || h->chain.n || h->drop_on) return false;
    if (h->lform || h->arch->wide || h->p2p_on || h->net.T != 1 || h->net.mech == EH_MECH_PROGRAM || h->net.loss == EH_LOSS_PROGRAM || h->act == EH_ACT_PER_NET) return false;
    if (h->img.l2c != 0.0f || h->img.l2w || two_pass_mask(h->net) || h->dp_weights || h->dp_moments) return false;
    // (one target: the row's scalars are ONE 16-byte vector, all four words written by the gather -- the marker regime of the hand-off counts on it)
    if (h->n_acc != h->net.n_theta + 4 || h->ord_rs != h->ord_soff + 4) return false;
    // (the step stages its row in LDS over the parameter image before it stores it)
    return h->n_acc < 8192 && h->ord_rs <= h->arch->img_floats && (cw_env == 0 || cw_env == 16);
}

// fused step on the train split.  apply = update theta; loss_slot = device float for the loss.
int eh_do_step(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, bool apply, bool raw, float* loss_slot) {
    const EhNet& net = h->net;
    EhProf prof;
    if (int rc = prof_begin(h, &prof)) return rc;
    int grid = 1;
    const int deferred = (net.T == 1 && !raw) ? 1 : 0;
    const unsigned tp_mask = two_pass_mask(net);
    const bool moment_loss = tp_mask != 0;
    const bool l2 = (h->img.l2c != 0.0f || h->img.l2w) && !raw;      // (data-parallel seam: raw sums only -- the extra loss is added once, in eh_dp_apply)
    float* sc_in = h->sc + 2 * h->sc_sel;
    float* sc_out = h->sc + 2 * (h->sc_sel ^ 1);
    // layer-wise form, few rows: the optimiser may run in the epilogue of the grouped weight-gradient launch (eh_lform_train decides, eh_lform.hip; EhLApply)
    EhLApply lap{};
    h->l_apply = nullptr; h->l_applied = false;
    const bool chained = apply && h->chain.n != 0;      // an optimiser chain: the reduction leaves the gradient, the chain kernels apply it
    if (h->lform && apply && deferred && !l2 && !moment_loss && net.loss != EH_LOSS_PROGRAM) {
        lap.theta = TH(h); lap.m = MM(h); lap.v = VV(h); lap.sc_in = sc_in; lap.sc_out = sc_out; lap.o = h->opt; lap.loss_slot = loss_slot; lap.gradbuf = h->gradbuf;
        lap.im = h->img; lap.loss_kind = h->net.loss; lap.n_theta = net.n_theta; lap.g_off = net.g_off;
        if (chained) {
            // A chain needs the finished gradient, from the SAME products the unchained few-rows step takes (other product kernels sum the
            // samples in another order: other bits).  The epilogue is handed Descent(-1) on a zeroed "parameter" vector that is gradbuf itself:
            // 0 - (-1 g) leaves exactly g = sum * scale there, the loss and the counts behind it as always; no moments, no image (g_off = n_theta
            // and no map: eh_image_store has nothing to store), and the products it advances are written again by the chain's apply pass.
            HIPCHK(h, hipMemsetAsync(h->gradbuf, 0, (size_t)net.n_theta * sizeof(float), h->stream));
            lap.theta = h->gradbuf;               // (m, v: Descent keeps none, nobody reads or writes them)
            lap.o = EhOpt{EH_OPT_DESCENT, -1.0f, 1.0f, 1.0f, 0.0f, 0.0f, nullptr};
            lap.im.g_off = net.n_theta; lap.im.imap = nullptr;
        }
        h->l_apply = &lap;
    }
    int rc = launch_train_kernel(h, sp, idx, first, count, &grid, apply);
    h->l_apply = nullptr;
    if (rc) return rc;
    if (h->drop_on && apply) h->drop_step++;      // (eh_loss_and_grad leaves the count: its gradient is the one the next training step applies)
    const bool mid = prof.on && !prof.burst;      // (every step bracketed on its own: the mark between the step kernel and the reduction)
    if (mid) HIPCHK(h, hipEventRecord(h->ev[h->ev_used + 1], h->stream));
    if (h->l_applied) {                  // theta, the moments, the loss and the beta products are done (a chain: the gradient is; its kernels follow)
        h->l_applied = false;
        if (chained) {
            if (int rcc = launch_chain(h, false, sc_in, sc_out, nullptr)) return rcc;
        }
        h->sc_sel ^= 1;
        return prof_end(h, prof, mid);
    }
    if (l2) {
        hipLaunchKernelGGL(eh_weight_l2_kernel, dim3(1), dim3(256), 0, h->stream, TH(h), h->img, h->l2val);
        HIPCHK(h, hipGetLastError());
    }
    static const int cw_env = getenv("EH_REDUCE_CW") ? atoi(getenv("EH_REDUCE_CW")) : 0;      // (A/B switch of the measurement tools)
    const bool big = cw_env ? cw_env == 64 : h->n_acc >= 8192;          // enough columns to fill the chip with 64-column blocks
    // layer-wise form: few slab rows (<= 32) under very many columns (the tutorial net: 700 k): one column per thread -- with 64-column
    // blocks 3 of 4 threads had no row to read and the per-block part (counts, barriers) ran 11 k times: 29.6 us of a 250 us step at
    // B = 64 (tools/lform_trace.sh)
    const bool tall = cw_env ? cw_env == 256 : (h->lform && grid <= (int)EH_LFORM_ROWS && h->n_acc >= 16384);
    static const bool nc1 = getenv("EH_REDUCE_NC1") != nullptr;
    const bool tall4 = tall && !nc1;                                   // four columns per thread
    const int rgrid = tall4 ? (h->n_acc + 1023) / 1024 : tall ? (h->n_acc + 255) / 256 : big ? (h->n_acc + 63) / 64 : (h->n_acc + 15) / 16;
#define EH_REDUCE_GO(AP, ...)                                                                                                                       \
    hipLaunchKernelGGL((eh_reduce_kernel<AP, __VA_ARGS__>), dim3(rgrid), dim3(256), 0, h->stream, h->slab, grid, h->n_acc, net.n_theta, net.T, deferred, h->gradbuf, \
                       TH(h), MM(h), VV(h), sc_in, sc_out, h->opt, loss_slot, h->img, h->net.loss, (moment_loss && !raw) ? h->inv_n : nullptr, l2 ? h->l2val : nullptr, tp_mask)
    if (apply && !chained) {
        if (tall4) EH_REDUCE_GO(true, 256, 4, true); else if (tall) EH_REDUCE_GO(true, 256); else if (big) EH_REDUCE_GO(true, 64); else EH_REDUCE_GO(true, 16);
        ++h->upd_site[tall4 ? EH_UPD_REDUCE256V4 : tall ? EH_UPD_REDUCE256 : big ? EH_UPD_REDUCE64 : EH_UPD_REDUCE16];
        h->sc_sel ^= 1;
    } else {
        if (tall4) EH_REDUCE_GO(false, 256, 4, true); else if (tall) EH_REDUCE_GO(false, 256); else if (big) EH_REDUCE_GO(false, 64); else EH_REDUCE_GO(false, 16);
    }
#undef EH_REDUCE_GO
    HIPCHK(h, hipGetLastError());
    if (chained) {
        if (int rcc = launch_chain(h, false, sc_in, sc_out, nullptr)) return rcc;
        h->sc_sel ^= 1;
    }
    return prof_end(h, prof, mid);
}

static int ensure_loss_hist(eh_handle* h, long long need) {
    if (h->loss_cap >= need) return EH_OK;
    FLUSH(h);
    return eh_grow(h, &h->loss_hist, &h->loss_cap, need);
}

int eh_check_window(eh_handle* h, const EhSplit& sp, long long first, long long count, const char* who) {
    if (!sp.recs || sp.n == 0) return fail(h, EH_ESTATE, "%s: no data set for this split (call eh_set_data)", who);
    if (first < 0 || count < 0 || first + count > sp.samples()) return fail(h, EH_EINVAL, "%s: window [%lld, %lld) outside 0..%lld", who, first, first + count, sp.samples());
    return EH_OK;
}

// host minibatch indices -> the handle's device scratch (range-checked); the step then gathers through it from offset 0
static int stage_host_idx(eh_handle* h, const EhSplit& sp, const int32_t* idx, int64_t first, int64_t count, const char* who) {
    if (!sp.recs) return fail(h, EH_ESTATE, "%s: no data set for this split", who);
    if (count < 0 || first < 0) return fail(h, EH_EINVAL, "%s: first %lld, count %lld", who, (long long)first, (long long)count);
    if (h->capturing) return fail(h, EH_ESTATE, "%s: host indices cannot be recorded into a graph (upload them and pass idx_on_device = 1)", who);
    for (int64_t i = 0; i < count; ++i)
        if (idx[first + i] < 0 || idx[first + i] >= sp.samples()) return fail(h, EH_EINVAL, "%s: idx[%lld] = %d outside 0..%lld", who, (long long)(first + i), idx[first + i], sp.samples());
    if (count > h->idx_cap) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        (void)hipFree(h->idx_buf);
        h->idx_buf = nullptr; h->idx_cap = 0;
        HIPCHK(h, hipMalloc(&h->idx_buf, (size_t)std::max<int64_t>(count, 1) * sizeof(int)));
        h->idx_cap = count;
    }
    // (the previous step that read idx_buf is ahead of this copy in stream order)
    HIPCHK(h, hipMemcpyAsync(h->idx_buf, idx + first, (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return EH_OK;
}

// forward / eval on a window; stats (host, double) per target may be null
// The pinned buffers the evaluation kernels store their sums into outlive their handles in a small pool: pinning host memory costs
// some hundred microseconds, and train() creates (and closes) an engine per call -- 10 ms in all for the tutorial's 20 epochs.
static int eval_host_acquire(eh_handle* h, size_t need) {
    {
        std::lock_guard<std::mutex> lk(g_eval_pool_mu);
        for (size_t i = 0; i < g_eval_pool.size(); ++i)
            if (g_eval_pool[i].device == h->device && g_eval_pool[i].cap >= need) {
                h->eval_host = g_eval_pool[i].host; h->eval_host_dev = g_eval_pool[i].dev; h->eval_host_cap = g_eval_pool[i].cap;
                g_eval_pool.erase(g_eval_pool.begin() + (long)i);
                return EH_OK;
            }
    }
    const size_t cap = std::max<size_t>(need, (size_t)4096 * EH_EVAL_STATS * EH_MAX_TARG);
    HIPCHK(h, hipHostMalloc((void**)&h->eval_host, cap * sizeof(float), hipHostMallocMapped));
    HIPCHK(h, hipHostGetDevicePointer((void**)&h->eval_host_dev, h->eval_host, 0));
    h->eval_host_cap = cap;
    return EH_OK;
}

// sequence models: `count` windows, count * ow predictions [window][j] per target; EVAL leaves one row of shifted sums per workgroup in the
// slab, EH_EVAL_STATS per target
static int seq_eval(eh_handle* h, EhSplit& sp, long long first, long long count, double* stats, float* const* yhat, float* const* params) {
    if (!sp.starts) return fail(h, EH_ESTATE, "eh_eval: sequence model: no windows for this split (call eh_set_sequences after eh_set_data)");
    const int T = h->net.T, nst = EH_EVAL_STATS * T;
    const long long nout = count * sp.ow, need = (long long)((yhat ? T : 0) + (params ? h->plan.n_par : 0)) * nout;
    if (need > h->out_cap) { if (int rc2 = eh_grow(h, &h->out_buf, &h->out_cap, need)) return rc2; }
    EhSeqArgs a = seq_args(h, sp, nullptr, first, count);
    a.n_acc = nst;
    a.yhat = yhat ? h->out_buf : nullptr;
    a.pout = params ? h->out_buf + (yhat ? T * nout : 0) : nullptr;
    a.yld = nout;
    const int grid = seq_grid_for(h, sp, count, false);
    HIPCHK(h, seq_launch(h, stats ? EH_SEQ_EVAL : EH_SEQ_FORWARD, grid, a));
    std::vector<float> part;
    if (stats) {
        part.resize((size_t)grid * nst);
        HIPCHK(h, hipMemcpyAsync(part.data(), h->slab, part.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (stats)
        for (int k = 0; k < nst; ++k) {
            double s = 0;
            for (int b = 0; b < grid; ++b) s += part[(size_t)b * nst + k];
            stats[k] = s;
        }
    if (yhat)
        for (int t = 0; t < T; ++t)
            if (yhat[t]) { if (int rc = eh_copy_out(h, yhat[t], a.yhat + (long long)t * nout, (size_t)nout)) return rc; }
    if (params)
        for (int j = 0; j < h->plan.n_par; ++j)
            if (params[j]) { if (int rc = eh_copy_out(h, params[j], a.pout + (long long)j * nout, (size_t)nout)) return rc; }
    return EH_OK;
}

static int do_eval(eh_handle* h, int split, long long first, long long count, double* stats, float* const* yhat, float* const* params) {
    const EhNet& net = h->net;
    EhSplit& sp = h->split[split];
    HIPCHK(h, hipSetDevice(h->device));
    int rc = eh_check_window(h, sp, first, count, "eh_eval");
    if (rc) return rc;
    FLUSH(h);
    if (h->seq) return seq_eval(h, sp, first, count, stats, yhat, params);
    const long long need = (long long)(yhat ? net.T : 0) * count + (long long)(params ? h->plan.n_par : 0) * count;
    if (need > h->out_cap) { if (int rc2 = eh_grow(h, &h->out_buf, &h->out_cap, need)) return rc2; }
    EhStepArgs a = eh_step_args(h, sp, nullptr, first, count);
    a.image = h->image; a.slab = h->slab; a.n_acc = EH_EVAL_STATS * net.T;
    a.yhat = yhat ? h->out_buf : nullptr;
    a.pout = params ? h->out_buf + (yhat ? (long long)net.T * count : 0) : nullptr;
    a.yld = count;
    int grid = count > 0 ? (h->lform ? grid_for(h, count) : eval_grid_for(h, count)) : 1;
    // The per-workgroup sums (grid x 8 T floats) go to the host for the final fold in double.  The step kernels store them straight into
    // pinned, device-visible host memory -- the call is the kernel and one synchronisation; as a copy out of the slab into pageable
    // memory behind the kernel it was a staged transfer of its own, 25-30 us of a 105 us call over the headline split.
    const float* part = nullptr;
    std::vector<float> part_copy;
    static const bool no_zero_copy = getenv("EH_EVAL_COPY") != nullptr;      // (A/B switch of the measurement tools)
    if (!h->lform && !no_zero_copy) {
        const size_t need_host = (size_t)grid * a.n_acc;
        if (need_host > h->eval_host_cap) {
            HIPCHK(h, hipStreamSynchronize(h->stream));
            eval_host_release(h);
            if (int rc2 = eval_host_acquire(h, need_host)) return rc2;
        }
        a.slab = h->eval_host_dev;
        part = h->eval_host;
    }
    // (eh_profile_enable: HIP events on the engine's stream around the evaluation kernel too -- the kernel's own time beside the call's,
    //  which also holds the launch, the synchronisation and the reading of the sums; bench.py eh_eval_roofline)
    const bool prof_ev = h->prof && h->ev_used + 3 <= 3 * 8192 && ensure_events(h, h->ev_used + 3) == EH_OK;
    if (prof_ev) HIPCHK(h, hipEventRecord(h->ev[h->ev_used], h->stream));
    if (h->lform) { if ((rc = eh_lform_eval(h, sp, first, count, a.yhat, a.pout, &grid))) return rc; }
    else HIPCHK(h, step_launch(h, EH_MODE_EVAL, grid, &a));
    if (prof_ev) {
        HIPCHK(h, hipEventRecord(h->ev[h->ev_used + 1], h->stream));
        HIPCHK(h, hipEventRecord(h->ev[h->ev_used + 2], h->stream));
        h->ev_used += 3;
    }
    if (!part) {
        part_copy.resize((size_t)grid * a.n_acc);
        HIPCHK(h, hipMemcpyAsync(part_copy.data(), h->slab, part_copy.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        part = part_copy.data();
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (stats) {
        for (int k = 0; k < a.n_acc; ++k) {
            double s = 0;
            for (int b = 0; b < grid; ++b) s += part[(size_t)b * a.n_acc + k];
            stats[k] = s;
        }
    }
    if (yhat)
        for (int t = 0; t < net.T; ++t)
            if (yhat[t]) { if (int rc2 = eh_copy_out(h, yhat[t], a.yhat + (long long)t * count, (size_t)count)) return rc2; }
    if (params)
        for (int j = 0; j < h->plan.n_par; ++j)
            if (params[j]) { if (int rc2 = eh_copy_out(h, params[j], a.pout + (long long)j * count, (size_t)count)) return rc2; }
    return EH_OK;
}

// the metrics of eh_target_metrics from the EH_EVAL_STATS sums per target of an evaluation pass, taken about the shifts c_t (eh_eval, eh_ens_eval)
void eh_metrics_from_sums(const double* st, const float* shift, int T, eh_target_metrics* out) {
    const double nan = std::nan("");
    for (int t = 0; t < T; ++t) {
        const double* s = st + t * EH_EVAL_STATS;
        const double c = shift[t];
        const double S = s[0], Sy = s[1], Syy = s[2], n = s[3], Sh = s[4], Shh = s[5], Shy = s[6], A = s[7];
        eh_target_metrics& o = out[t];
        o.n = n; o.sse = S;
        if (n <= 0) { o.mse = o.rmse = o.mae = o.r2 = o.nse = o.pearson = o.kge = o.pbkge = o.beta = o.alpha = nan; continue; }
        // centred sums.  The raw ones are fp32 sums: a centred one below 64 ulp of its raw sum of squares has no correct digit left and
        // is the zero of a constant selection (one sample, a constant target or prediction), which loss_fn sees exactly.
        double ssy = Syy - Sy * Sy / n, ssh = Shh - Sh * Sh / n, shy = Shy - Sh * Sy / n;
        const double tiny = 64.0 * FLT_EPSILON;
        if (ssy <= tiny * Syy) ssy = 0.0;
        if (ssh <= tiny * Shh) ssh = 0.0;
        o.mse = S / n; o.rmse = std::sqrt(o.mse); o.mae = A / n;
        o.r2 = 1.0 - S / ssy;           // loss_fn(Val(:r2)), src/losses/loss_fn.jl:71-73 (a constant target: -Inf, or NaN for S = 0)
        o.nse = o.r2;                   // :nse has the same closed form (:85-86)
        o.pearson = ssy > 0.0 && ssh > 0.0 ? shy / std::sqrt(ssh * ssy) : nan;      // cor() of a constant vector is NaN
        o.alpha = std::sqrt(ssh / ssy); // std ratio (the n-1 cancels)
        o.beta = (c + Sh / n) / (c + Sy / n);
        o.kge = 1.0 - std::sqrt((o.pearson - 1) * (o.pearson - 1) + (o.alpha - 1) * (o.alpha - 1) + (o.beta - 1) * (o.beta - 1));
        o.pbkge = 1.0 - std::sqrt((o.pearson - 1) * (o.pearson - 1) + (o.beta - 1) * (o.beta - 1));
    }
}

extern "C" {

int32_t eh_forward(eh_handle* h, int32_t split, int64_t first, int64_t count, float* const* yhat, float* const* params) {
    if (!h) return EH_EINVAL;
    if (split != EH_SPLIT_TRAIN && split != EH_SPLIT_VAL) return fail(h, EH_EINVAL, "eh_forward: split %d", split);
    return do_eval(h, split, first, count, nullptr, yhat, params);
}

int32_t eh_eval(eh_handle* h, int32_t split, int64_t first, int64_t count, eh_target_metrics* out, float* const* yhat, float* const* params) {
    if (!h || !out) return EH_EINVAL;
    if (split != EH_SPLIT_TRAIN && split != EH_SPLIT_VAL) return fail(h, EH_EINVAL, "eh_eval: split %d", split);
    double st[EH_MAX_TARG * EH_EVAL_STATS] = {0};
    int rc = do_eval(h, split, first, count, st, yhat, params);
    if (rc) return rc;
    eh_metrics_from_sums(st, h->split[split].shift, h->net.T, out);
    return EH_OK;
}

int32_t eh_loss_and_grad(eh_handle* h, int32_t split, const int32_t* idx, int64_t first, int64_t count, float* loss, float* grad, int64_t* n_valid) {
    if (!h) return EH_EINVAL;
    if (split != EH_SPLIT_TRAIN && split != EH_SPLIT_VAL) return fail(h, EH_EINVAL, "eh_loss_and_grad: split %d", split);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    EhSplit& sp = h->split[split];
    int rc;
    const int* didx = nullptr;
    if (idx) {
        if ((rc = stage_host_idx(h, sp, idx, 0, count, "eh_loss_and_grad"))) return rc;
        didx = h->idx_buf;
        first = 0;
    } else {
        rc = eh_check_window(h, sp, first, count, "eh_loss_and_grad");
        if (rc) return rc;
    }
    rc = eh_do_step(h, sp, didx, first, count, false, false, nullptr);
    if (rc) return rc;
    std::vector<float> host((size_t)h->n_acc);
    HIPCHK(h, hipMemcpyAsync(host.data(), h->gradbuf, host.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int nt = h->net.n_theta;
    if (grad) memcpy(grad, host.data(), (size_t)nt * sizeof(float));
    if (loss) {
        *loss = host[nt];
        if (h->empty_nan && h->net.T > 1) {
            bool some = false, empty = false;
            for (int t = 0; t < h->net.T; ++t) { some = some || host[nt + 1 + t] > 0.0f; empty = empty || !(host[nt + 1 + t] > 0.0f); }
            if (some && empty) *loss = std::nanf("");
        }
    }
    if (n_valid) {
        double c = 0;
        for (int t = 0; t < h->net.T; ++t) c += host[nt + 1 + t];
        *n_valid = (int64_t)std::llround(c);
    }
    return EH_OK;
}

int32_t eh_get_bn_state(eh_handle* h, float* running_mean, float* running_var, int64_t n) {
    if (!h || !running_mean || !running_var) return EH_EINVAL;
    if (!h->bn_on) return fail(h, EH_ESTATE, "eh_get_bn_state: the model has no input BatchNorm");
    if (n != h->net.P) return fail(h, EH_EINVAL, "eh_get_bn_state: n = %lld, model has %d predictors", (long long)n, h->net.P);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(running_mean, h->bn_run, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(running_var, h->bn_run + 32, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return EH_OK;
}

int32_t eh_set_bn_state(eh_handle* h, const float* running_mean, const float* running_var, int64_t n) {
    if (!h || !running_mean || !running_var) return EH_EINVAL;
    if (!h->bn_on) return fail(h, EH_ESTATE, "eh_set_bn_state: the model has no input BatchNorm");
    if (n != h->net.P) return fail(h, EH_EINVAL, "eh_set_bn_state: n = %lld, model has %d predictors", (long long)n, h->net.P);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<float> rstd((size_t)n);
    for (int64_t p = 0; p < n; ++p) rstd[p] = 1.0f / std::sqrt(running_var[p] + EH_BN_EPS);
    HIPCHK(h, hipMemcpy(h->bn_run, running_mean, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->bn_run + 32, running_var, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->image + h->arch->phi_off + EH_IMG_BNM, running_mean, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->image + h->arch->phi_off + EH_IMG_BNR, rstd.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return EH_OK;
}

// running statistics of a BatchNorm layer inside the chain (eh_bnl.hpp)
static int layer_state_check(eh_handle* h, const char* who, int32_t layer, int64_t n) {
    if (!h->bnl || layer < 0 || layer >= h->plan.l_net[0].nl || !eh_is_norm(h->plan.l_net[0].kind[layer]) || eh_is_layernorm(h->plan.l_net[0].kind[layer])) return fail(h, EH_ESTATE, "%s: hidden layer %d is no BatchNorm layer", who, layer);
    if (n != h->plan.l_net[0].out[layer]) return fail(h, EH_EINVAL, "%s: n = %lld, the layer has %d units", who, (long long)n, h->plan.l_net[0].out[layer]);
    return EH_OK;
}
int32_t eh_get_layer_state(eh_handle* h, int32_t layer, float* running_mean, float* running_var, int64_t n) {
    if (!h || !running_mean || !running_var) return EH_EINVAL;
    if (int rc = layer_state_check(h, "eh_get_layer_state", layer, n)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(running_mean, h->bnl_run + h->plan.bnl_off[layer], (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(running_var, h->bnl_run + h->plan.bnl_off[layer] + n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return EH_OK;
}
int32_t eh_set_layer_state(eh_handle* h, int32_t layer, const float* running_mean, const float* running_var, int64_t n) {
    if (!h || !running_mean || !running_var) return EH_EINVAL;
    if (int rc = layer_state_check(h, "eh_set_layer_state", layer, n)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(h->bnl_run + h->plan.bnl_off[layer], running_mean, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->bnl_run + h->plan.bnl_off[layer] + n, running_var, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return EH_OK;
}
int32_t eh_set_layer_norm(eh_handle* h, int32_t layer, float momentum, float epsilon) {
    if (!h) return EH_EINVAL;
    const bool ln = h->lnl && layer >= 0 && layer < h->plan.l_net[0].nl && eh_is_layernorm(h->plan.l_net[0].kind[layer]);      // (a LayerNorm layer: its epsilon; it has no momentum to set)
    if (!ln) { if (int rc = layer_state_check(h, "eh_set_layer_norm", layer, h->bnl && layer >= 0 && layer < h->plan.l_net[0].nl ? h->plan.l_net[0].out[layer] : 0)) return rc; }
    if (!(momentum >= 0.0f && momentum <= 1.0f) || !(epsilon > 0.0f)) return fail(h, EH_EINVAL, "eh_set_layer_norm: momentum %g (0..1), epsilon %g (> 0)", (double)momentum, (double)epsilon);
    h->bnl_mom[layer] = momentum; h->bnl_eps[layer] = epsilon;      // (kernel arguments of the steps launched from now on)
    return EH_OK;
}

// a new rule (eh_opt_init, eh_opt_init_groups): out of L-BFGS mode, no chain, zero moments, the running beta products at their start
static int opt_restart(eh_handle* h, const float* sc, size_t sc_bytes) {
    if (h->lb) h->lb->active = false;
    h->chain = EhChain{}; h->chain_gen = 0;
    HIPCHK(h, hipMemset(MM(h), 0, (size_t)h->net.n_theta * sizeof(float)));
    HIPCHK(h, hipMemset(VV(h), 0, (size_t)h->net.n_theta * sizeof(float)));
    HIPCHK(h, hipMemcpy(h->sc, sc, sc_bytes, hipMemcpyHostToDevice));
    h->sc_sel = 0;
    h->opt_ready = true;
    lean_refresh(h);
    return EH_OK;
}
int32_t eh_opt_init(eh_handle* h, int32_t rule, float lr, float beta1, float beta2, float eps, float weight_decay) {
    if (!h) return EH_EINVAL;
    if (h->ens_live) return fail(h, EH_ESTATE, "eh_opt_init: the handle carries an ensemble (eh_ens_destroy it first)");
    if (rule < EH_OPT_ADAM || rule > EH_OPT_DESCENT) return fail(h, EH_EUNSUPPORTED, "eh_opt_init: unknown rule %d", rule);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->opt = EhOpt{rule, lr, beta1, beta2, eps, weight_decay, nullptr};
    h->opt_groups = 1;
    const float sc[4] = {beta1, beta2, beta1, beta2};   // Optimisers.jl starts the running product at beta (t = 1)
    return opt_restart(h, sc, sizeof sc);
}

int32_t eh_opt_init_groups(eh_handle* h, const uint8_t* group, int64_t n_theta, int32_t n_groups, const int32_t* rule, const float* hyper) {
    if (!h) return EH_EINVAL;
    if (h->ens_live) return fail(h, EH_ESTATE, "eh_opt_init_groups: the handle carries an ensemble (eh_ens_destroy it first)");
    if (!group || !rule || !hyper) return fail(h, EH_EINVAL, "eh_opt_init_groups: null table");
    if (n_theta != h->net.n_theta) return fail(h, EH_EINVAL, "eh_opt_init_groups: n_theta %lld, the model has %d", (long long)n_theta, h->net.n_theta);
    if (n_groups > EH_MAX_OPT_GROUPS) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_groups: %d groups (at most %d)", n_groups, EH_MAX_OPT_GROUPS);
    if (n_groups < 1) return fail(h, EH_EINVAL, "eh_opt_init_groups: %d groups", n_groups);
    for (int k = 0; k < n_groups; ++k)
        if (rule[k] < EH_OPT_ADAM || rule[k] > EH_OPT_DESCENT) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_groups: group %d: unknown rule %d", k, rule[k]);
    const size_t nt = (size_t)n_theta;
    for (size_t i = 0; i < nt; ++i)
        if (group[i] >= n_groups) return fail(h, EH_EINVAL, "eh_opt_init_groups: element %zu in group %d of %d", i, (int)group[i], n_groups);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t tab_bytes = offsetof(EhOptTab, gid) + ((nt + 3) & ~(size_t)3);
    std::vector<unsigned char> host(tab_bytes, 0);
    EhOptTab* const t = reinterpret_cast<EhOptTab*>(host.data());
    for (int k = 0; k < n_groups; ++k) {
        const float* hp = hyper + 5 * k;
        t->r[k] = EhOpt{rule[k], hp[0], hp[1], hp[2], hp[3], hp[4], nullptr};
    }
    t->n = n_groups;
    memcpy(host.data() + offsetof(EhOptTab, gid), group, nt);
    if (!h->opt_tab) HIPCHK(h, hipMalloc(&h->opt_tab, tab_bytes));       // (n_theta is fixed for the handle's life)
    HIPCHK(h, hipMemcpy(h->opt_tab, host.data(), tab_bytes, hipMemcpyHostToDevice));
    // (the handle's own rule names Adam, so every site moves m and v; its hyper-parameters are group 0's -- the table is what is read)
    h->opt = EhOpt{EH_OPT_ADAM, t->r[0].lr, t->r[0].b1, t->r[0].b2, t->r[0].eps, t->r[0].wd, h->opt_tab};
    h->opt_groups = n_groups;
    float sc[4 * EH_MAX_OPT_GROUPS] = {};
    for (int k = 0; k < n_groups; ++k) {       // group k, set s at [4 k + 2 s]; Optimisers.jl starts each product at beta (t = 1)
        sc[4 * k] = sc[4 * k + 2] = hyper[5 * k + 1];
        sc[4 * k + 1] = sc[4 * k + 3] = hyper[5 * k + 2];
    }
    return opt_restart(h, sc, sizeof sc);
}

int32_t eh_opt_init_chain(eh_handle* h, const eh_opt_stage* stages, int32_t n_stages, int32_t rule, float lr, float beta1, float beta2, float eps, float weight_decay) {
    if (!h || !stages) return EH_EINVAL;
    if (h->ens_live) return fail(h, EH_ESTATE, "eh_opt_init_chain: the handle carries an ensemble (eh_ens_destroy it first)");
    if (n_stages < 1) return fail(h, EH_EINVAL, "eh_opt_init_chain: %d stages", n_stages);
    if (n_stages > EH_MAX_OPT_STAGES) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: %d stages (at most %d, nested chains flattened)", n_stages, EH_MAX_OPT_STAGES);
    if (rule < EH_OPT_ADAM || rule > EH_OPT_DESCENT) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: unknown rule %d", rule);
    EhChain c{};
    c.n = n_stages; c.i_norm = -1; c.i_rule = -1; c.p = 2;
    for (int k = 0; k < n_stages; ++k) {
        const eh_opt_stage& st = stages[k];
        c.kind[k] = st.kind; c.a[k] = st.a;
        if (st.kind == EH_STAGE_RULE) {
            if (c.i_rule >= 0) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: stage %d: a second rule (a chain holds exactly one of Adam / AdamW / RMSProp / Descent)", k);
            c.i_rule = k;
        } else if (st.kind == EH_STAGE_CLIPGRAD) {
            if (!(st.a >= 0.0f)) return fail(h, EH_EINVAL, "eh_opt_init_chain: stage %d: ClipGrad(delta = %g)", k, (double)st.a);
        } else if (st.kind == EH_STAGE_WEIGHTDECAY) {
            if (!(st.a >= 0.0f)) return fail(h, EH_EINVAL, "eh_opt_init_chain: stage %d: WeightDecay(lambda = %g)", k, (double)st.a);
        } else if (st.kind == EH_STAGE_CLIPNORM) {
            if (!(st.a > 0.0f)) return fail(h, EH_EINVAL, "eh_opt_init_chain: stage %d: ClipNorm(omega = %g)", k, (double)st.a);
            if (c.i_norm >= 0) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: stage %d: a second ClipNorm (one norm pass per step is built)", k);
            if (c.i_rule >= 0) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: stage %d: ClipNorm behind the rule needs the norm of the UPDATE, a second pass over it: not built", k);
            if (st.b == 1.0f) c.p = 1; else if (st.b == 2.0f) c.p = 2; else if (st.b == INFINITY) c.p = 0;
            else return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: stage %d: ClipNorm with p = %g (1, 2 and Inf are built)", k, (double)st.b);
            c.i_norm = k; c.omega = st.a; c.thr = st.flags & 1;
        } else return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: stage %d: unknown kind %d", k, st.kind);
    }
    if (c.i_rule < 0) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: no EH_STAGE_RULE among the stages (a chain holds exactly one rule)");
    if (h->fused && !h->fused_det) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: the one-kernel step (fused_update 1) is not built for an optimiser chain: switch it to 0 or 2 first");
    if (h->p2p_alloc) return fail(h, EH_EUNSUPPORTED, "eh_opt_init_chain: the peer-to-peer fused exchange is not built for an optimiser chain: eh_p2p_disable first");
    int rc = eh_opt_init(h, rule, lr, beta1, beta2, eps, weight_decay);       // (drains the stream; zero moments; the products at beta)
    if (rc) return rc;
    if (!h->chain_part) HIPCHK(h, hipMalloc(&h->chain_part, (EH_CHAIN_PARTS + 3) * sizeof(double)));      // here, never inside a capture
    HIPCHK(h, hipMemset(h->chain_part, 0, (EH_CHAIN_PARTS + 3) * sizeof(double)));
    static int gen = 0;
    h->chain = c; h->chain_gen = ++gen;
    return EH_OK;
}

int32_t eh_opt_chain_status(eh_handle* h, int64_t* n_applied, int64_t* n_clipped, int64_t* n_nonfinite) {
    if (!h) return EH_EINVAL;
    if (!h->chain.n) return fail(h, EH_ESTATE, "eh_opt_chain_status: no optimiser chain (call eh_opt_init_chain first)");
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unsigned long long ctr[3];
    HIPCHK(h, hipMemcpy(ctr, h->chain_part + EH_CHAIN_PARTS, sizeof ctr, hipMemcpyDeviceToHost));
    if (n_applied) *n_applied = (int64_t)ctr[0];
    if (n_clipped) *n_clipped = (int64_t)ctr[1];
    if (n_nonfinite) *n_nonfinite = (int64_t)ctr[2];
    return EH_OK;
}

int32_t eh_get_opt_beta_t(eh_handle* h, float* bt, int32_t n_groups) {
    if (!h || !bt) return EH_EINVAL;
    if (n_groups != h->opt_groups) return fail(h, EH_EINVAL, "eh_get_opt_beta_t: %d groups, the handle has %d", n_groups, h->opt_groups);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float sc[4 * EH_MAX_OPT_GROUPS];
    HIPCHK(h, hipMemcpy(sc, h->sc, sizeof sc, hipMemcpyDeviceToHost));
    for (int k = 0; k < n_groups; ++k) { bt[2 * k] = sc[4 * k + 2 * h->sc_sel]; bt[2 * k + 1] = sc[4 * k + 2 * h->sc_sel + 1]; }
    return EH_OK;
}

int32_t eh_set_opt_beta_t(eh_handle* h, const float* bt, int32_t n_groups) {
    if (!h || !bt) return EH_EINVAL;
    if (!h->opt_ready) return fail(h, EH_ESTATE, "eh_set_opt_beta_t: call eh_opt_init or eh_opt_init_groups first");
    if (n_groups != h->opt_groups) return fail(h, EH_EINVAL, "eh_set_opt_beta_t: %d groups, the handle has %d", n_groups, h->opt_groups);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < n_groups; ++k)
        HIPCHK(h, hipMemcpy(h->sc + 4 * k + 2 * h->sc_sel, bt + 2 * k, 2 * sizeof(float), hipMemcpyHostToDevice));
    return EH_OK;
}

int32_t eh_get_opt_state(eh_handle* h, float* m, float* v, int64_t n, float* beta_t) {
    if (!h) return EH_EINVAL;
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_get_opt_state: n");
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (m) { if (int rc = eh_copy_out(h, m, MM(h), (size_t)n)) return rc; }
    if (v) { if (int rc = eh_copy_out(h, v, VV(h), (size_t)n)) return rc; }
    if (beta_t) HIPCHK(h, hipMemcpy(beta_t, h->sc + 2 * h->sc_sel, 2 * sizeof(float), hipMemcpyDeviceToHost));
    return EH_OK;
}

int32_t eh_set_opt_state(eh_handle* h, const float* m, const float* v, int64_t n, const float* beta_t) {
    if (!h) return EH_EINVAL;
    if (!h->opt_ready) return fail(h, EH_ESTATE, "eh_set_opt_state: call eh_opt_init first");
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_set_opt_state: n");
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (m) { if (int rc = eh_copy_in(h, MM(h), m, (size_t)n)) return rc; }
    if (v) { if (int rc = eh_copy_in(h, VV(h), v, (size_t)n)) return rc; }
    if (beta_t) HIPCHK(h, hipMemcpy(h->sc + 2 * h->sc_sel, beta_t, 2 * sizeof(float), hipMemcpyHostToDevice));
    return EH_OK;
}

// ---- dropout (eh_device.hpp: EH_JIT_DROPOUT) -----------------------------------------------------------
int32_t eh_set_dropout(eh_handle* h, const float* rate, int32_t n_hidden, uint64_t seed, uint64_t step) {
    if (!h) return EH_EINVAL;
    if (!rate || n_hidden != h->desc.n_hidden) return fail(h, EH_EINVAL, "eh_set_dropout: %d rates for %d hidden layers", (int)n_hidden, (int)h->desc.n_hidden);
    bool any = false;
    for (int l = 0; l < n_hidden; ++l) {
        if (!(rate[l] >= 0.0f && rate[l] < 1.0f)) return fail(h, EH_EINVAL, "eh_set_dropout: rate[%d] = %g (0 <= p < 1)", l, (double)rate[l]);
        any = any || rate[l] > 0.0f;
    }
    if (any) {
        const char* why = nullptr;
        if (h->seq) why = "sequence models";
        else if (h->lform) why = "the layer-wise form (more than 3 hidden layers or widths above 128)";
        else if (h->desc.n_nets != 0) why = "MultiNN models";
        else if (h->arch->var[h->variant].bf16) why = "the bf16 kernels (precision option)";      // (a row-split family too: said first)
        else if (h->arch->wide) why = "the row-split kernels (hidden widths above 64, or the row_split option)";
        else if (h->p2p_on || h->p2p_alloc || h->comm || h->lgroup) why = "data parallelism (a communicator or a peer-to-peer exchange is set up on this handle)";
        else if (h->capturing) why = "a handle that is recording a graph";
        else if (!h->plan.acts.empty()) why = "recorded activations (eh_create_activations: the mask would have to go through the recorded derivative's kernels, not built)";
        if (why) return fail(h, EH_EUNSUPPORTED, "eh_set_dropout: dropout is built for the fp32 per-wave fused kernels of single-network models, not for %s", why);
        if (!h->jit_on) return fail(h, EH_EUNSUPPORTED, "eh_set_dropout: the dropout kernels are compiled at run time and the jit option is off (EH_JIT=0)");
    }
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    h->drop_on = any;
    for (int l = 0; l < EH_MAX_HIDDEN; ++l) h->drop[l] = (any && l < n_hidden) ? rate[l] : 0.0f;
    h->drop_seed = seed; h->drop_step = step;
    if (any) { h->jit_failed = false; h->jit_log.clear(); }      // (a build that failed for other rates says nothing about these)
    lean_refresh(h);
    return EH_OK;
}

int32_t eh_get_dropout(eh_handle* h, float* rate, int32_t cap, uint64_t* seed, uint64_t* step) {
    if (!h) return EH_EINVAL;
    if (rate) {
        if (cap < h->desc.n_hidden) return fail(h, EH_EINVAL, "eh_get_dropout: room for %d rates, the model has %d hidden layers", (int)cap, (int)h->desc.n_hidden);
        for (int l = 0; l < h->desc.n_hidden; ++l) rate[l] = h->drop[l];
    }
    if (seed) *seed = h->drop_seed;
    if (step) *step = h->drop_step;
    return EH_OK;
}

int32_t eh_dropout_mask(eh_handle* h, int32_t layer, uint64_t step, int64_t count, uint8_t* keep) {
    if (!h || !keep) return EH_EINVAL;
    if (layer < 0 || layer >= h->desc.n_hidden || count < 0 || count > (1LL << 24)) return fail(h, EH_EINVAL, "eh_dropout_mask: layer %d, count %lld", (int)layer, (long long)count);
    if (h->desc.n_nets != 0) return fail(h, EH_EUNSUPPORTED, "eh_dropout_mask: single-network models only");
    const int width = h->desc.hidden[layer];
    if (count == 0) return EH_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = (size_t)count * (size_t)width;
    uint8_t* dev = nullptr;
    HIPCHK(h, hipMalloc(&dev, n));
    const int nq = (width + 3) / 4;
    const long long work = (long long)count * nq;
    hipLaunchKernelGGL(eh_dropout_mask_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, h->stream, (unsigned long long)h->drop_seed, (unsigned long long)step, (int)layer, width,
                       (long long)count, eh_drop_threshold(h->drop[layer]), dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(keep, dev, n, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(dev);
    HIPCHK(h, e);
    return EH_OK;
}

// ---- recorded activations (eh_device.hpp: EH_JIT_ACTPROG) ------------------------------------------------
// j >= 0: recorded activation j; -1 - id (id = EH_ACT_TANH .. EH_ACT_IDENTITY): the built-in one, through the same two device functions
int32_t eh_activation_apply(eh_handle* h, int32_t j, const float* z, int64_t n, float* a, float* da) {
    if (!h || !z || (!a && !da)) return EH_EINVAL;
    const int nprog = (int)h->plan.acts.size();
    if (!nprog) return fail(h, EH_ESTATE, "eh_activation_apply: the handle has no recorded activations (eh_create_activations)");
    if (j >= nprog || j < -1 - (int)EH_ACT_IDENTITY) return fail(h, EH_EINVAL, "eh_activation_apply: activation %d (recorded: 0..%d; built-in id: -1 - id)", (int)j, nprog - 1);
    if (n < 0 || n > (1LL << 28)) return fail(h, EH_EINVAL, "eh_activation_apply: n = %lld", (long long)n);
    if (n == 0) return EH_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->act_apply.fn[0]) {
        std::string log;
        if (!eh_jit_build_act_apply(h->plan.acts, &h->act_apply, &log)) return fail(h, EH_EUNSUPPORTED, "eh_activation_apply: the kernel failed to build: %.600s", log.c_str());
    }
    float* dev = nullptr;
    HIPCHK(h, hipMalloc(&dev, (size_t)3 * (size_t)n * sizeof(float)));
    hipError_t e = hipMemcpyAsync(dev, z, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        int id = j >= 0 ? (int)EH_ACT_RECORDED + (int)j : -1 - (int)j;
        const float* zd = dev;
        long long cnt = n;
        float *ad = a ? dev + n : nullptr, *dd = da ? dev + 2 * n : nullptr;
        void* params[] = {&id, &zd, &cnt, &ad, &dd};
        e = hipModuleLaunchKernel(h->act_apply.fn[0], (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, h->stream, params, nullptr);
    }
    if (e == hipSuccess && a) e = hipMemcpyAsync(a, dev + n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && da) e = hipMemcpyAsync(da, dev + 2 * n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(dev);
    HIPCHK(h, e);
    return EH_OK;
}

int32_t eh_activation_source(const eh_act_program* progs, int32_t n_progs, char* buf, int64_t bytes) {
    std::string why;
    if (n_progs < 1) return fail(nullptr, EH_EINVAL, "eh_activation_source: %d activation programs (1..%d)", (int)n_progs, (int)EH_MAX_ACT_PROGS);
    if (const int rc = eh_act_programs_check(progs, n_progs, "eh_activation_source", &why)) return fail(nullptr, rc, "%s", why.c_str());
    const std::string s = eh_jit_act_source(progs, n_progs);
    if (!buf || bytes < (int64_t)s.size() + 1) return (int32_t)s.size() + 1;
    memcpy(buf, s.c_str(), s.size() + 1);
    return EH_OK;
}

// One training step on the path the handle's mode takes; *one_kernel: a fused-update step (its update is pending), else the step + reduce pair.
// "fused_update" 2: the float-atomic one-kernel step only where one workgroup covers the minibatch, the ordered one elsewhere (ord_ok), the
// pair where that is not built; an optimiser chain: always the step + reduce + chain kernels
static int train_one(eh_handle* h, const EhSplit& sp, const int* idx, long long first, long long count, float* loss_slot, bool* one_kernel) {
    const int grid = h->seq ? 0 : grid_for(h, count);
    *one_kernel = false;
    if (h->fused && !(h->fused_det && grid != 1) && !h->chain.n) {
        if (int rc = do_fused_step(h, sp, idx, first, count, loss_slot)) return rc;
        *one_kernel = true;
    } else if (ord_ok(h, grid)) {
        if (int rc = do_fused_step(h, sp, idx, first, count, loss_slot, true, one_kernel)) return rc;
        if (*one_kernel) ++h->ord_steps;
    }
    if (*one_kernel) return EH_OK;
    FLUSH(h);                                  // ("fused_update" 2: a one-workgroup step may be pending in front of this larger one)
    return eh_do_step(h, sp, idx, first, count, true, false, loss_slot);
}
int32_t eh_train_step(eh_handle* h, const int32_t* idx, int32_t idx_on_device, int64_t first, int64_t count, float* loss_out) {
    if (!h) return EH_EINVAL;
    if (!h->opt_ready) return fail(h, EH_ESTATE, "eh_train_step: call eh_opt_init first");
    HIPCHK(h, hipSetDevice(h->device));
    EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    int rc;
    const int* didx = nullptr;
    if (idx && !idx_on_device) {
        if ((rc = stage_host_idx(h, sp, idx, first, count, "eh_train_step"))) return rc;
        didx = h->idx_buf;
        first = 0;
    } else if (idx) {
        if (!sp.recs || sp.n == 0) return fail(h, EH_ESTATE, "eh_train_step: no data set for this split (call eh_set_data)");
        if (first < 0 || count < 0) return fail(h, EH_EINVAL, "eh_train_step: first %lld, count %lld", (long long)first, (long long)count);
        didx = idx;
        if (h->check_idx && count > 0) {        // "check_idx" (debug): the entries idx[first .. first + count) of the caller's DEVICE array against the split's size
            if (h->capturing) return fail(h, EH_ESTATE, "eh_train_step: the check_idx option synchronises: not while a graph is recorded");
            unsigned* bad = nullptr;
            HIPCHK(h, hipMalloc(&bad, 2 * sizeof(unsigned)));
            HIPCHK(h, hipMemsetAsync(bad, 0, sizeof(unsigned), h->stream));
            HIPCHK(h, hipMemsetAsync(bad + 1, 0xFF, sizeof(unsigned), h->stream));      // (position of the first offender: a minimum)
            hipLaunchKernelGGL(eh_idx_check_kernel, dim3((unsigned)std::min<long long>(1024, (count + 255) / 256)), dim3(256), 0, h->stream, idx, (long long)first, (long long)count, (long long)sp.samples(), bad);
            unsigned res[2] = {0, 0};
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(res, bad, sizeof res, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            (void)hipFree(bad);
            HIPCHK(h, e);
            if (res[0]) return fail(h, EH_EINVAL, "eh_train_step: %u of the %lld device-side indices are outside 0..%lld (first offender: idx[%lld])", res[0], (long long)count, (long long)sp.samples() - 1, (long long)first + (long long)res[1]);
        }
    } else if ((rc = eh_check_window(h, sp, first, count, "eh_train_step"))) return rc;
    rc = ensure_loss_hist(h, 1);
    if (rc) return rc;
    bool one_kernel = false;
    if ((rc = train_one(h, sp, didx, first, count, loss_out ? h->loss_hist : nullptr, &one_kernel))) return rc;
    if (one_kernel && loss_out) FLUSH(h);
    if (loss_out) {
        HIPCHK(h, hipMemcpyAsync(loss_out, h->loss_hist, sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return EH_OK;
}

// device-side keyed permutation of the train split's sample indices into h->perm
static int make_permutation(eh_handle* h, long long N, uint64_t seed) {
    if (h->perm_cap < N) { if (int rc = eh_grow(h, &h->perm, &h->perm_cap, N)) return rc; }
    int bits = 1;
    while ((1LL << bits) < N) ++bits;
    const int hb = std::max(1, (bits + 1) / 2);
    hipLaunchKernelGGL(eh_perm_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, h->perm, (uint32_t)N, hb, seed);
    HIPCHK(h, hipGetLastError());
    return EH_OK;
}

// ---- hipGraph capture of a sequence of training steps -------------------------------------------------
int32_t eh_graph_begin(eh_handle* h) {
    if (!h) return EH_EINVAL;
    if (h->seq) return fail(h, EH_EUNSUPPORTED, "eh_graph_begin: graph capture is not built for sequence models");
    if (h->bnl) return fail(h, EH_EUNSUPPORTED, "eh_graph_begin: graph capture is not built for BatchNorm layers in the chain");
    if (h->drop_on) return fail(h, EH_EUNSUPPORTED, "eh_graph_begin: dropout: every step carries its own step count in its arguments, a recorded graph would replay one mask: not built");
    if (h->lb && h->lb->active) return fail(h, EH_EUNSUPPORTED, "eh_graph_begin: the handle is in L-BFGS mode (capture is not built for it): eh_opt_init* leaves the mode");
    if (h->capturing) return fail(h, EH_ESTATE, "eh_graph_begin: already capturing");
    if (h->ens_live) return fail(h, EH_ESTATE, "eh_graph_begin: the handle carries an ensemble, whose launches read records that change with every epoch (eh_ens_destroy it first)");
    // a fused-mode step applies the update of the step before it: the recorded sequence has to start (and every replay
    // has to find the engine) with such an update pending, or its first kernel would skip / re-apply one
    if (h->fused && !h->pending) return fail(h, EH_ESTATE, "eh_graph_begin: fused_update mode: run one training step first (and do not synchronize before capturing)");
    h->cap = {nullptr, h->fused, (int)(h->gstep % 3), h->cur, h->sc_sel, h->pend_ord, h->pend_ord ? h->ord_grid : 0, h->opt.tab != nullptr, h->chain_gen};
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure_loss_hist(h, 1);
    if (rc) return rc;
    if (jit_wanted(h, EH_MODE_TRAIN)) {
        // compile and load NOW, synchronously: hiprtc / hipModuleLoadData must not run beside a relaxed capture, and the kernel must
        // not change in the middle of the recorded sequence ("specialize" = 2 would otherwise hand the build to a worker thread)
        h->capturing = true;                    // (jit_entry builds in the calling thread while this is set)
        (void)jit_entry(h);
        h->capturing = false;
        for (auto& e : h->jit) if (e->worker.joinable()) e->worker.join();      // a build already in flight: wait for it
    }
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
    h->capturing = true;
    return EH_OK;
}

int32_t eh_graph_end(eh_handle* h, int32_t* graph_id) {
    if (!h || !graph_id) return EH_EINVAL;
    if (!h->capturing) return fail(h, EH_ESTATE, "eh_graph_end: not capturing");
    h->capturing = false;
    hipGraph_t g = nullptr;
    HIPCHK(h, hipStreamEndCapture(h->stream, &g));
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return fail(h, EH_EHIP, "eh_graph_end: hipGraphInstantiate: %s", hipGetErrorString(e));
    if (h->fused != h->cap.fused || (int)(h->gstep % 3) != h->cap.gslot || h->cur != h->cap.cur || h->sc_sel != h->cap.sc_sel ||
        h->pend_ord != h->cap.pend_ord || (h->pend_ord ? h->ord_grid : 0) != h->cap.ord_grid || (h->opt.tab != nullptr) != h->cap.grouped) {
        (void)hipGraphExecDestroy(ex);
        return fail(h, EH_EINVAL, "eh_graph_end: the recorded sequence does not bring the engine's rotation state back (record a multiple of 6 steps in fused_update mode, of 2 otherwise)");
    }
    h->cap.exec = ex;
    h->graphs.push_back(h->cap);
    *graph_id = (int32_t)h->graphs.size() - 1;
    return EH_OK;
}

int32_t eh_graph_launch(eh_handle* h, int32_t graph_id) {
    if (!h) return EH_EINVAL;
    if (graph_id < 0 || graph_id >= (int32_t)h->graphs.size()) return fail(h, EH_EINVAL, "eh_graph_launch: graph %d", graph_id);
    const eh_handle::GraphRec& g = h->graphs[(size_t)graph_id];
    if (g.fused != h->fused || g.gslot != (int)(h->gstep % 3) || g.cur != h->cur || g.sc_sel != h->sc_sel || (g.fused && !h->pending) ||
        g.pend_ord != h->pend_ord || g.ord_grid != (h->pend_ord ? h->ord_grid : 0))
        return fail(h, EH_ESTATE, "eh_graph_launch: the engine is not in the state the graph was recorded in (steps / synchronize in between: run steps until it is, with an update pending in fused_update mode)");
    // (the recorded kernels carry the optimiser by value: one rule, or the per-branch table -- whose contents may change, its address does not)
    if (g.grouped != (h->opt.tab != nullptr))
        return fail(h, EH_ESTATE, "eh_graph_launch: the graph was recorded with %s, the engine now has %s (eh_opt_init / eh_opt_init_groups)",
                    g.grouped ? "per-branch optimiser rules" : "one optimiser rule", g.grouped ? "one rule" : "per-branch rules");
    if (g.chain_gen != h->chain_gen)
        return fail(h, EH_ESTATE, "eh_graph_launch: the graph was recorded %s, the engine now has %s (eh_opt_init / eh_opt_init_chain)",
                    g.chain_gen ? "with an optimiser chain" : "without an optimiser chain", h->chain_gen ? "another chain" : "none");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipGraphLaunch(g.exec, h->stream));
    return EH_OK;
}

int32_t eh_train_epoch(eh_handle* h, int64_t batchsize, uint64_t seed, int32_t shuffle, float* mean_loss, int64_t* n_steps) {
    if (!h) return EH_EINVAL;
    if (!h->opt_ready) return fail(h, EH_ESTATE, "eh_train_epoch: call eh_opt_init first");
    if (batchsize < 1) return fail(h, EH_EINVAL, "eh_train_epoch: batchsize %lld", (long long)batchsize);
    HIPCHK(h, hipSetDevice(h->device));
    EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    if (!sp.recs || sp.n == 0) return fail(h, EH_ESTATE, "eh_train_epoch: no training data");
    if (h->seq && !sp.starts) return fail(h, EH_ESTATE, "eh_train_epoch: sequence model: no windows (call eh_set_sequences after eh_set_data)");
    const long long N = sp.samples();      // (sequence models: the epoch shuffles and batches windows)
    if (shuffle) {
        if (int rc = make_permutation(h, N, seed)) return rc;
        h->perm_valid = false;          // (the data-parallel window order of eh_dp_shuffle is gone)
    }
    const long long steps = (N + batchsize - 1) / batchsize;
    int rc = ensure_loss_hist(h, steps);
    if (rc) return rc;
    if (multi_ok(h, batchsize)) {          // one workgroup per step: up to EH_MULTI_MAX steps per launch
        for (long long s = 0; s < steps; s += EH_MULTI_MAX) {
            const int n = (int)std::min<long long>(EH_MULTI_MAX, steps - s);
            if ((rc = do_fused_multi(h, sp, shuffle ? h->perm : nullptr, s * batchsize, batchsize, N, n, h->loss_hist + s))) return rc;
        }
    } else
    for (long long s = 0; s < steps; ++s) {
        const long long first = s * batchsize;
        bool one_kernel;
        if ((rc = train_one(h, sp, shuffle ? h->perm : nullptr, first, std::min<long long>(batchsize, N - first), h->loss_hist + s, &one_kernel))) return rc;
    }
    if (mean_loss) FLUSH(h);
    if (n_steps) *n_steps = steps;
    if (mean_loss) {
        std::vector<float> l((size_t)steps);
        HIPCHK(h, hipMemcpyAsync(l.data(), h->loss_hist, l.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        double sum = 0; long long c = 0;
        for (float x : l) if (!std::isnan(x)) { sum += x; ++c; }
        *mean_loss = c ? (float)(sum / c) : std::nanf("");
    }
    return EH_OK;
}

int32_t eh_set_weight_l2(eh_handle* h, float lambda, int32_t normalize) {
    if (!h) return EH_EINVAL;
    if (!(lambda >= 0.0f)) return fail(h, EH_EINVAL, "eh_set_weight_l2: lambda = %g", (double)lambda);
    if (lambda != 0.0f && h->fused) return fail(h, EH_EUNSUPPORTED, "eh_set_weight_l2: not built for the fused_update mode: switch it off first");
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    h->img.l2c = (normalize && h->plan.n_weights > 0) ? lambda / (float)h->plan.n_weights : lambda;
    h->img.l2w = nullptr;
    return EH_OK;
}

int32_t eh_set_weight_l2_coef(eh_handle* h, const float* coef, int64_t n) {
    if (!h) return EH_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    if (!coef || n == 0) { h->img.l2w = nullptr; h->img.l2c = 0.0f; return EH_OK; }
    if (n != h->net.n_theta) return fail(h, EH_EINVAL, "eh_set_weight_l2_coef: %lld coefficients for %d parameters", (long long)n, h->net.n_theta);
    bool any = false;
    for (int64_t i = 0; i < n; ++i) {
        if (!(coef[i] >= 0.0f) || std::isinf(coef[i])) return fail(h, EH_EINVAL, "eh_set_weight_l2_coef: coefficient %lld = %g", (long long)i, (double)coef[i]);
        any = any || coef[i] != 0.0f;
    }
    if (any && h->fused) return fail(h, EH_EUNSUPPORTED, "eh_set_weight_l2_coef: not built for the fused_update mode: switch it off first");
    if (!any) { h->img.l2w = nullptr; h->img.l2c = 0.0f; return EH_OK; }
    if (!h->l2w) HIPCHK(h, hipMalloc(&h->l2w, (size_t)n * sizeof(float)));
    HIPCHK(h, hipMemcpyAsync(h->l2w, coef, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // (the caller's array may go away)
    h->img.l2w = h->l2w; h->img.l2c = 0.0f; h->img.n_theta = h->net.n_theta;
    return EH_OK;
}

// what no entry point of the data-parallel seam is built for
static int dp_refused(eh_handle* h, const char* who) {
    if (h->seq) return fail(h, EH_EUNSUPPORTED, "%s: data parallelism is not built for sequence models", who);
    if (h->lb && h->lb->active) return fail(h, EH_EUNSUPPORTED, "%s: the handle is in L-BFGS mode, which is not built for data parallelism (eh_opt_init* leaves the mode)", who);
    if (h->drop_on) return fail(h, EH_EUNSUPPORTED, "%s: dropout is not built for data parallelism (the masks are drawn per handle, from its own step count)", who);
    if (h->bnl) return fail(h, EH_EUNSUPPORTED, "%s: BatchNorm layers in the chain are not built for data parallelism (their statistics would have to be those of the global batch)", who);
    return EH_OK;
}
int32_t eh_dp_shuffle(eh_handle* h, uint64_t seed, int32_t on) {
    if (!h) return EH_EINVAL;
    if (h->seq) return fail(h, EH_EUNSUPPORTED, "eh_dp_shuffle: data parallelism is not built for sequence models");
    if (h->bnl) return fail(h, EH_EUNSUPPORTED, "eh_dp_shuffle: BatchNorm layers in the chain are not built for data parallelism (their statistics would have to be those of the global batch)");
    if (h->drop_on) return fail(h, EH_EUNSUPPORTED, "eh_dp_shuffle: dropout is not built for data parallelism (the masks are drawn per handle, from its own step count)");
    HIPCHK(h, hipSetDevice(h->device));
    if (!on) { h->perm_valid = false; return EH_OK; }      // (stream order keeps earlier steps on the old permutation)
    EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    if (!sp.recs || sp.n == 0) return fail(h, EH_ESTATE, "eh_dp_shuffle: no training data");
    if (int rc = make_permutation(h, sp.n, seed)) return rc;
    h->perm_valid = true;
    return EH_OK;
}

int32_t eh_dp_grad(eh_handle* h, int64_t first, int64_t count) {
    if (!h) return EH_EINVAL;
    if (int rc = dp_refused(h, "eh_dp_grad")) return rc;
    if (h->net.T != 1 && !h->tcount_ready) return fail(h, EH_ESTATE, "eh_dp_grad: multi-target model: call eh_dp_counts for this window and all-reduce EH_BUF_TCOUNT first");
    const unsigned tpm_dp = two_pass_mask(h->net);
    if (tpm_dp && h->mom_stage != 2) return fail(h, EH_ESTATE, "eh_dp_grad: rmse (multi-target) / pearson / kge training losses need the moments of the GLOBAL batch's predictions first: eh_dp_moments stage 0, all-reduce EH_BUF_MOMENT, stage 1, all-reduce");
    if (h->bn_on && !h->bn_ext) return fail(h, EH_ESTATE, "eh_dp_grad: input BatchNorm needs the global batch statistics: call eh_dp_bn_stats and all-reduce EH_BUF_BNSTAT first");
    h->bn_dp_update = h->bn_on;
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    int rc = eh_check_window(h, sp, first, count, "eh_dp_grad");
    if (rc) return rc;
    if (h->net.T != 1) {      // the weights of the GLOBAL batch from the all-reduced sums; the step kernel then normalises exactly
        hipLaunchKernelGGL(eh_weights_from_counts_kernel, dim3(1), dim3(64), 0, h->stream, h->tcount, h->net.T, h->net.loss_t, h->inv_n, h->img.agg_a, h->roles, h->img.l2s);
        HIPCHK(h, hipGetLastError());
        h->dp_weights = true;
    }
    if (tpm_dp) {             // the all-reduced moments about the global centre -> k0 k1 k2 and the loss value of every two-pass target
        if ((rc = eh_launch_moment_coef(h, sp, h->mombuf, 1))) return rc;
        h->dp_moments = true;
    }
    rc = eh_do_step(h, sp, h->perm_valid ? h->perm : nullptr, first, count, false, true, nullptr);
    h->dp_weights = false; h->tcount_ready = false; h->dp_moments = false; h->mom_stage = 0;
    return rc;
}

// multi-target models under data parallelism: this shard's per-target sums of the window into EH_BUF_TCOUNT
// ([n_t | sum (y - c) | sum (y - c)^2] per target, c = the split's target shift: the ranks must share it, eh_set_target_shift).
// The caller all-reduces the 12 floats; eh_dp_grad turns them into the weights 1 / n_t (mse, mae) or 1 / sum (y - ybar)^2 (nseLoss).
int32_t eh_dp_counts(eh_handle* h, int64_t first, int64_t count) {
    if (!h) return EH_EINVAL;
    if (int rc = dp_refused(h, "eh_dp_counts")) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    int rc = eh_check_window(h, sp, first, count, "eh_dp_counts");
    if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(h->tcount, 0, 3 * EH_MAX_TARG * sizeof(float), h->stream));
    if ((rc = eh_launch_count(h, sp, h->perm_valid ? h->perm : nullptr, first, count, h->tcount))) return rc;
    h->tcount_ready = true;
    return EH_OK;
}

// Two-pass training losses (pearsonLoss / kgeLoss / pbkgeLoss, rmse on a multi-target model; src/losses/loss_fn.jl:58-60,105-174)
// under data parallelism: d loss / d yhat_i = k0 + k1 (yhat_i - centre) + k2 (y_i - c) with coefficients made of the moments of the
// GLOBAL batch, so the shards exchange their moment sums twice ahead of the pass --
//   stage 0: forward-only pass over the window, this shard's sums about the common shift c into EH_BUF_MOMENT
//            ([T][EH_EVAL_STATS] floats: S, sum (y-c), sum (y-c)^2, n, sum (yhat-c), ...)          (caller: all-reduce)
//   stage 1: centre of yhat = c + sum (yhat - c) / n of the global batch; forward-only pass about it, sums into EH_BUF_MOMENT (all-reduce)
// -- and eh_dp_grad turns the all-reduced moments into the coefficients (same kernel as the single-GPU step) and runs the training
// pass with them: the sums in EH_BUF_GRAD are final, as for multi-target models.  Fused kernel families only (the layer-wise form
// keeps its statistics passes inside its own forward).
int32_t eh_dp_moments(eh_handle* h, int64_t first, int64_t count, int32_t stage) {
    if (!h) return EH_EINVAL;
    if (int rc = dp_refused(h, "eh_dp_moments")) return rc;
    const EhNet& net = h->net;
    if (!two_pass_mask(net)) return fail(h, EH_ESTATE, "eh_dp_moments: the training loss needs no batch moments of the predictions");
    if (h->lform) return fail(h, EH_EUNSUPPORTED, "eh_dp_moments: the layer-wise form has no data-parallel seam for the two-pass training losses");
    if (stage != 0 && stage != 1) return fail(h, EH_EINVAL, "eh_dp_moments: stage %d (0 or 1)", stage);
    if (stage == 1 && h->mom_stage != 1) return fail(h, EH_ESTATE, "eh_dp_moments: stage 1 follows stage 0 (and the all-reduce of EH_BUF_MOMENT)");
    if (h->bn_on && !h->bn_ext) return fail(h, EH_ESTATE, "eh_dp_moments: input BatchNorm needs the global batch statistics: call eh_dp_bn_stats and all-reduce EH_BUF_BNSTAT first");
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    if (int rc = eh_check_window(h, sp, first, count, "eh_dp_moments")) return rc;
    const int* idx = h->perm_valid ? h->perm : nullptr;
    EhStepArgs e = eh_step_args(h, sp, idx, first, count);
    e.image = h->image; e.slab = h->slab; e.n_acc = EH_EVAL_STATS * net.T; e.rmap = h->rmap; e.stamps = nullptr;
    e.yld = count;
    // (the global BatchNorm statistics of eh_dp_bn_stats serve both moment passes AND the training pass behind them: eh_dp_grad /
    //  eh_dp_fused_step consume them; advisor, round 4: stage 0 used to clear them and every later pass of the step failed)
    if (int rc = eh_bn_prepare(h, sp, idx, first, count, false, &e, /*consume*/ false)) return rc;
    if (stage == 1) {        // the all-reduced sums about the shift -> the centre of yhat of the global batch
        if (int rc = eh_launch_moment_centre(h, sp, h->mombuf, 1)) return rc;
        e.inv_n = h->inv_n;
    }
    const int egrid = count > 0 ? grid_for(h, count) : 1;
    if (count > 0) HIPCHK(h, step_launch(h, EH_MODE_EVAL, egrid, &e));
    else HIPCHK(h, hipMemsetAsync(h->slab, 0, (size_t)EH_EVAL_STATS * net.T * sizeof(float), h->stream));      // an empty shard window adds nothing
    hipLaunchKernelGGL(eh_moment_fold_kernel, dim3(1), dim3(64), 0, h->stream, h->slab, egrid, net.T, h->mombuf);
    HIPCHK(h, hipGetLastError());
    h->mom_stage = stage + 1;
    return EH_OK;
}

// common shift of the shifted target sums (nseLoss, metrics) -- under data parallelism every rank passes the same vector, e.g. the
// mean of each target over the global training set; eh_set_data resets it to the shard's own means
int32_t eh_set_target_shift(eh_handle* h, int32_t split, const float* shift, int64_t n) {
    if (!h || !shift) return EH_EINVAL;
    if (split != EH_SPLIT_TRAIN && split != EH_SPLIT_VAL) return fail(h, EH_EINVAL, "eh_set_target_shift: split %d", split);
    if (n != h->net.T) return fail(h, EH_EINVAL, "eh_set_target_shift: %lld values for %d targets", (long long)n, h->net.T);
    HIPCHK(h, hipSetDevice(h->device));
    FLUSH(h);
    for (int t = 0; t < h->net.T; ++t) h->split[split].shift[t] = shift[t];
    return EH_OK;
}

int32_t eh_dp_fused_step(eh_handle* h, int64_t first, int64_t count, int32_t* buffer_index) {
    if (!h || !buffer_index) return EH_EINVAL;
    if (int rc = dp_refused(h, "eh_dp_fused_step")) return rc;
    if (!h->fused) return fail(h, EH_ESTATE, "eh_dp_fused_step: set the fused_update option first");
    if (h->net.T != 1) return fail(h, EH_EUNSUPPORTED, "eh_dp_fused_step: multi-target models need the global per-target counts before the pass: use eh_dp_counts + eh_dp_grad (fused_update off)");
    if (h->bn_on && !h->bn_ext) return fail(h, EH_ESTATE, "eh_dp_fused_step: input BatchNorm needs the global batch statistics: call eh_dp_bn_stats and all-reduce EH_BUF_BNSTAT first");
    if (!h->opt_ready) return fail(h, EH_ESTATE, "eh_dp_fused_step: call eh_opt_init first");
    if (h->chain.n) return fail(h, EH_EUNSUPPORTED, "eh_dp_fused_step: not built for an optimiser chain (the norm needs the all-reduced gradient before the update): use eh_dp_grad + eh_dp_apply");
    HIPCHK(h, hipSetDevice(h->device));
    EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    int rc = eh_check_window(h, sp, first, count, "eh_dp_fused_step");
    if (rc) return rc;
    *buffer_index = h->p2p_on ? -1 : (int32_t)(h->gstep % 3);        // -1: the kernels exchange the sums themselves (eh_p2p_attach)
    return do_fused_step(h, sp, h->perm_valid ? h->perm : nullptr, first, count, nullptr);
}

int32_t eh_set_bn_shift(eh_handle* h, const float* shift, int64_t n) {
    if (!h || !shift) return EH_EINVAL;
    if (!h->bn_on) return fail(h, EH_ESTATE, "eh_set_bn_shift: the model has no input BatchNorm");
    if (n != h->net.P) return fail(h, EH_EINVAL, "eh_set_bn_shift: n = %lld, model has %d predictors", (long long)n, h->net.P);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(h->bn_shift, shift, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return EH_OK;
}

int32_t eh_dp_bn_stats(eh_handle* h, int64_t first, int64_t count) {
    if (!h) return EH_EINVAL;
    if (int rc = dp_refused(h, "eh_dp_bn_stats")) return rc;
    if (!h->bn_on) return fail(h, EH_ESTATE, "eh_dp_bn_stats: the model has no input BatchNorm");
    HIPCHK(h, hipSetDevice(h->device));
    EhSplit& sp = h->split[EH_SPLIT_TRAIN];
    int rc = eh_check_window(h, sp, first, count, "eh_dp_bn_stats");
    if (rc) return rc;
    const int* idx = h->perm_valid ? h->perm : nullptr;      // the same samples eh_dp_grad / eh_dp_fused_step will read
    const int nblk = (int)std::max<long long>(1, std::min<long long>(32, (count + 1023) / 1024));
    hipLaunchKernelGGL(eh_bn_stats_kernel, dim3(nblk), dim3(1024), 0, h->stream, sp.recs, h->plan.C, h->net.P, idx, (int)first, (int)count, h->bn_part, h->bn_shift);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(eh_bn_fold_kernel, dim3(1), dim3(64), 0, h->stream, h->bn_part, nblk, (int)count, h->bn_stat);
    HIPCHK(h, hipGetLastError());
    h->bn_ext = true;
    return EH_OK;
}

int32_t eh_dp_apply(eh_handle* h, float* loss_out) {
    if (!h) return EH_EINVAL;
    if (int rc = dp_refused(h, "eh_dp_apply")) return rc;
    if (!h->opt_ready) return fail(h, EH_ESTATE, "eh_dp_apply: call eh_opt_init first");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure_loss_hist(h, 1);
    if (rc) return rc;
    float* sc_in = h->sc + 2 * h->sc_sel;
    float* sc_out = h->sc + 2 * (h->sc_sel ^ 1);
    const int nt = h->net.n_theta;
    const bool l2 = h->img.l2c != 0.0f || h->img.l2w;
    if (l2) {                                                  // the extra loss is a function of the replicated parameters: every rank adds the same term
        hipLaunchKernelGGL(eh_weight_l2_kernel, dim3(1), dim3(256), 0, h->stream, TH(h), h->img, h->l2val);
        HIPCHK(h, hipGetLastError());
    }
    if (h->chain.n) {                                          // norm of the all-reduced, globally normalised gradient
        if ((rc = launch_chain(h, true, sc_in, sc_out, h->loss_hist))) return rc;
    } else {
        hipLaunchKernelGGL(eh_apply_kernel, dim3((nt + 255) / 256), dim3(256), 0, h->stream, h->gradbuf, nt, TH(h), MM(h), VV(h), sc_in, sc_out, h->opt,
                           h->loss_hist, h->img, h->net.loss, h->net.T, l2 ? h->l2val : nullptr, two_pass_mask(h->net) ? h->inv_n : nullptr, two_pass_mask(h->net));
        HIPCHK(h, hipGetLastError());
        ++h->upd_site[EH_UPD_DP_APPLY];
    }
    h->sc_sel ^= 1;
    if (loss_out) {
        HIPCHK(h, hipMemcpyAsync(loss_out, h->loss_hist, sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return EH_OK;
}

int32_t eh_device_buffer(eh_handle* h, int32_t which, void** dev_ptr, int64_t* n_floats) {
    if (!h || !dev_ptr || !n_floats) return EH_EINVAL;
    if (h->fused && which != EH_BUF_GRAD && which != EH_BUF_GACC && which != EH_BUF_BNSTAT && which != EH_BUF_TCOUNT && which != EH_BUF_MOMENT) return fail(h, EH_ESTATE, "eh_device_buffer: parameter buffers ping-pong in fused_update mode; switch it off first");
    switch (which) {
        case EH_BUF_GRAD: *dev_ptr = h->gradbuf; *n_floats = h->n_acc; return EH_OK;
        case EH_BUF_THETA: *dev_ptr = TH(h); *n_floats = h->net.n_theta; return EH_OK;
        case EH_BUF_OPT_M: *dev_ptr = MM(h); *n_floats = h->net.n_theta; return EH_OK;
        case EH_BUF_OPT_V: *dev_ptr = VV(h); *n_floats = h->net.n_theta; return EH_OK;
        case EH_BUF_GACC: *dev_ptr = h->gacc; *n_floats = (int64_t)3 * EH_GSHARDS * h->n_acc; return EH_OK;
        case EH_BUF_BNSTAT:
            if (!h->bn_on) return fail(h, EH_ESTATE, "eh_device_buffer: the model has no input BatchNorm");
            *dev_ptr = h->bn_stat; *n_floats = 65; return EH_OK;
        case EH_BUF_TCOUNT: *dev_ptr = h->tcount; *n_floats = 3 * EH_MAX_TARG; return EH_OK;
        case EH_BUF_MOMENT: *dev_ptr = h->mombuf; *n_floats = EH_MAX_TARG * EH_EVAL_STATS; return EH_OK;
        default: return fail(h, EH_EINVAL, "eh_device_buffer: which = %d", which);
    }
}

int32_t eh_debug_stamps(eh_handle* h, uint64_t* out, int32_t n) {
    if (!h || !out || n < 0 || n > EH_STAMP_WORDS) return EH_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->stamps) {   // first call arms the buffer; later calls read it
        HIPCHK(h, hipMalloc(&h->stamps, EH_STAMP_WORDS * sizeof(unsigned long long)));      // (behind the step's own stamps: the ordered step's hand-off, EH_ORD_ST_PRO / EH_ORD_ST_TAIL)
        HIPCHK(h, hipMemset(h->stamps, 0, EH_STAMP_WORDS * sizeof(unsigned long long)));
        memset(out, 0, (size_t)n * sizeof(uint64_t));
        lean_refresh(h);                     // (diagnostics are outside the lean kernels' contract)
        return EH_OK;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->stamps, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return EH_OK;
}

int32_t eh_profile_enable(eh_handle* h, int32_t on) {
    if (!h) return EH_EINVAL;
    h->prof = on != 0;
    h->prof_stride = on > 1 ? on : 1;        // on = S > 1: one event pair around every burst of S consecutive steps
    h->prof_k = 0;
    h->ev_used = 0;
    return EH_OK;
}

int32_t eh_profile_samples(eh_handle* h, double* ms, int64_t cap, int64_t* n_out) {
    if (!h || !n_out || (cap > 0 && !ms)) return EH_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int64_t n = std::min<int64_t>((int64_t)(h->ev_used / 3), cap);
    for (int64_t i = 0; i < n; ++i) {
        float t = 0;
        HIPCHK(h, hipEventElapsedTime(&t, h->ev[3 * i], h->ev[3 * i + 2]));
        ms[i] = t;
    }
    *n_out = n;
    return EH_OK;
}

int32_t eh_profile_read(eh_handle* h, int64_t* n_launches, double* mean_ms_step_kernel, double* mean_ms_reduce_kernel) {
    if (!h) return EH_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double a = 0, b = 0;
    const size_t n = h->ev_used / 3;
    for (size_t i = 0; i < n; ++i) {
        float ms = 0;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[3 * i], h->ev[3 * i + 1]));
        a += ms;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[3 * i + 1], h->ev[3 * i + 2]));
        b += ms;
    }
    if (n_launches) *n_launches = (int64_t)n;
    if (mean_ms_step_kernel) *mean_ms_step_kernel = n ? a / n : 0.0;
    if (mean_ms_reduce_kernel) *mean_ms_reduce_kernel = n ? b / n : 0.0;
    h->ev_used = 0;
    return EH_OK;
}

}   // extern "C"

