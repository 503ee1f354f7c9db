// Data upload as a translation unit of its own: eh_set_data and eh_set_sequences, the pinned staging pair they keep for the process, and the
// staged copies of large arrays the other entry points use (eh_copy_out, eh_copy_in).
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <cmath>
#include <mutex>

#include "eh_internal.hpp"

// (P x N col-major predictors, F forcing arrays, T target arrays) -> N records of C floats
struct EhPackArgs {
    const float* x;
    const float* forc[EH_MAX_FORC];
    const float* targ[EH_MAX_TARG];
};
__global__ void eh_pack_kernel(EhPackArgs a, float* recs, long long n, int P, int F, int T, int planes) {
    const int C = P + F + T;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * C) return;
    const long long s = e / C;
    const int j = (int)(e % C);
    float v;
    if (j < P) v = planes ? a.x[(long long)j * n + s] : a.x[s * P + j];
    else if (j < P + F) v = a.forc[j - P][s];
    else v = a.targ[j - P - F][s];
    recs[e] = v;
}

static std::mutex g_stage_mu;                 // eh_set_data's pinned staging pair (host memory: any device)
static float* g_stage[2] = {nullptr, nullptr};
static size_t g_stage_bytes = 0;
// (g_stage_mu held) the pair at `bytes` each or more; false: no pinned memory to be had, and no pair kept
static bool stage_ensure(size_t bytes) {
    if (g_stage_bytes >= bytes) return true;
    for (int k = 0; k < 2; ++k) { if (g_stage[k]) (void)hipHostFree(g_stage[k]); g_stage[k] = nullptr; }
    g_stage_bytes = 0;
    if (hipHostMalloc((void**)&g_stage[0], bytes, hipHostMallocPortable) == hipSuccess &&          // (portable: the next handle may sit on another device)
        hipHostMalloc((void**)&g_stage[1], bytes, hipHostMallocPortable) == hipSuccess) g_stage_bytes = bytes;
    else { (void)hipGetLastError(); for (int k = 0; k < 2; ++k) { if (g_stage[k]) (void)hipHostFree(g_stage[k]); g_stage[k] = nullptr; } }
    return g_stage_bytes >= bytes;
}

extern "C" {

int32_t eh_set_data(eh_handle* h, int32_t split, int64_t n, const float* x, const float* const* forcings, const float* const* targets,
                    int32_t on_device) {
    if (!h) return EH_EINVAL;
    if (h->ens_live) return fail(h, EH_ESTATE, "eh_set_data: the handle carries an ensemble, whose row lists index this table (eh_ens_destroy it first)");
    if (split != EH_SPLIT_TRAIN && split != EH_SPLIT_VAL) return fail(h, EH_EINVAL, "eh_set_data: split %d", split);
    if (n < 0 || n > 0x7fffffffLL) return fail(h, EH_EINVAL, "eh_set_data: n = %lld", (long long)n);
    if (on_device & ~(EH_DATA_ON_DEVICE | EH_DATA_X_PLANES | EH_DATA_X_ROWS)) return fail(h, EH_EINVAL, "eh_set_data: flags %d", on_device);
    if ((on_device & EH_DATA_X_ROWS) && (on_device & (EH_DATA_ON_DEVICE | EH_DATA_X_PLANES))) return fail(h, EH_EINVAL, "eh_set_data: EH_DATA_X_ROWS goes with host arrays only, and not with EH_DATA_X_PLANES");
    if (n > 0 && ((!x && h->net.P > 0) || !forcings || !targets)) return fail(h, EH_EINVAL, "eh_set_data: null array");
    const EhNet& net = h->net;
    HIPCHK(h, hipSetDevice(h->device));
    EhSplit& sp = h->split[split];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    (void)hipFree(sp.recs); (void)hipFree(sp.starts);
    sp.recs = nullptr; sp.n = 0; sp.starts = nullptr; sp.nwin = 0;
    if (split == EH_SPLIT_TRAIN) h->perm_valid = false;
    if (n == 0) return EH_OK;
    const int C = h->plan.C;
    static const bool dbg_t = getenv("EH_DEBUG_SET_DATA") != nullptr;      // (diagnostic: where an upload's wall clock goes)
    const auto t_a = std::chrono::steady_clock::now();
    HIPCHK(h, hipMalloc(&sp.recs, (size_t)n * C * sizeof(float)));
    const auto t_b = std::chrono::steady_clock::now();
    const bool planes = (on_device & EH_DATA_X_PLANES) != 0;       // x as P arrays of N (row-major P x N: what a NumPy host holds) instead of N records of P
    const bool xrows = (on_device & EH_DATA_X_ROWS) != 0;          // x as P POINTERS to arrays of N: the caller's own columns, never stacked into a matrix
    const float* const* const xr = reinterpret_cast<const float* const*>(x);
    if (xrows) for (int j = 0; j < net.P; ++j) if (!xr[j]) return fail(h, EH_EINVAL, "eh_set_data: predictor row %d is null", j);
    on_device &= EH_DATA_ON_DEVICE;
    if (on_device) {
        EhPackArgs pa{};
        pa.x = x;
        for (int f = 0; f < net.F; ++f) pa.forc[f] = forcings[f];
        for (int t = 0; t < net.T; ++t) pa.targ[t] = targets[t];
        const long long tot = (long long)n * C;
        hipLaunchKernelGGL(eh_pack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, pa, sp.recs, (long long)n, net.P, net.F, net.T, planes ? 1 : 0);
        HIPCHK(h, hipGetLastError());
        // metric shift: mean of the first EH_SHIFT_VALID valid targets, from small host copies (a record that starts with a gap is read on
        // until that many are found)
        std::vector<float> tmp((size_t)std::min<int64_t>(n, 4096));
        for (int t = 0; t < net.T; ++t) {
            double s = 0; long long c = 0;
            for (int64_t off = 0; off < n && c < EH_SHIFT_VALID; off += (int64_t)tmp.size()) {
                const size_t m = (size_t)std::min<int64_t>((int64_t)tmp.size(), n - off);
                HIPCHK(h, hipMemcpy(tmp.data(), targets[t] + off, m * sizeof(float), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < m && c < EH_SHIFT_VALID; ++i) if (!std::isnan(tmp[i])) { s += tmp[i]; ++c; }
            }
            sp.shift[t] = c ? (float)(s / c) : 0.0f;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
    } else {
        // records interleaved on the host in chunks of <= 1 M samples, through two pinned staging buffers: chunk k is packed (two
        // to eight threads, each on its own run of samples) while chunk k - 1 is on its way over PCIe.  (Rounds 1-3: one pageable 67 MB vector, one thread, one
        // blocking copy: 56 ms for the headline data set; the one-time cost a user's train() call pays before its first step.)
        for (int t = 0; t < net.T; ++t) {
            double sum = 0; long long c = 0;
            for (int64_t s = 0; s < n && c < EH_SHIFT_VALID; ++s) if (!std::isnan(targets[t][s])) { sum += targets[t][s]; ++c; }
            sp.shift[t] = c ? (float)(sum / c) : 0.0f;
        }
        const int64_t CH = std::min<int64_t>(n, (int64_t)1 << 20);
        // (the two pinned buffers are kept for the next call of the process -- pinning 2 x 16 MB costs as much as the upload they stage;
        //  a second thread uploading at the same time gets buffers of its own)
        float* stage[2] = {nullptr, nullptr};
        hipEvent_t done[2] = {nullptr, nullptr};
        const size_t stage_bytes = (size_t)CH * C * sizeof(float);
        std::unique_lock<std::mutex> pool_lk(g_stage_mu, std::try_to_lock);
        const bool pooled = pool_lk.owns_lock();
        bool pinned;
        if (pooled) {
            pinned = stage_ensure(stage_bytes);
            if (pinned) { stage[0] = g_stage[0]; stage[1] = g_stage[1]; }
        } else {
            pinned = hipHostMalloc((void**)&stage[0], stage_bytes, hipHostMallocDefault) == hipSuccess &&
                     hipHostMalloc((void**)&stage[1], stage_bytes, hipHostMallocDefault) == hipSuccess;
        }
        std::vector<float> pageable;
        if (!pinned) {                                   // (no pinned memory to be had: the plain path)
            (void)hipGetLastError();
            if (!pooled) { if (stage[0]) (void)hipHostFree(stage[0]); if (stage[1]) (void)hipHostFree(stage[1]); }
            pageable.resize((size_t)CH * C);
            stage[0] = stage[1] = pageable.data();
        } else {
            // (an event that cannot be made: the first one is not leaked and a one-off staging pair not kept; advisor, round 4)
            hipError_t ee = hipEventCreateWithFlags(&done[0], hipEventDisableTiming);
            if (ee == hipSuccess) { ee = hipEventCreateWithFlags(&done[1], hipEventDisableTiming); if (ee != hipSuccess) (void)hipEventDestroy(done[0]); }
            if (ee != hipSuccess) { if (!pooled) { (void)hipHostFree(stage[0]); (void)hipHostFree(stage[1]); } HIPCHK(h, ee); }
        }
        const auto t_c = std::chrono::steady_clock::now();
        const int P = net.P, F = net.F, T = net.T;
        auto pack = [&](float* dst, int64_t s0, int64_t s1, int64_t base) {
            for (int64_t s = s0; s < s1; ++s) {
                float* r = dst + (size_t)(s - base) * C;
                if (xrows) for (int j = 0; j < P; ++j) r[j] = xr[j][s];
                else if (planes) for (int j = 0; j < P; ++j) r[j] = x[(size_t)j * (size_t)n + (size_t)s];
                else for (int j = 0; j < P; ++j) r[j] = x[(size_t)s * P + j];
                for (int f = 0; f < F; ++f) r[P + f] = forcings[f][s];
                for (int t = 0; t < T; ++t) r[P + F + t] = targets[t][s];
            }
        };
        hipError_t err = hipSuccess;
        int k = 0;
        for (int64_t s0 = 0; s0 < n && err == hipSuccess; s0 += CH, ++k) {
            const int64_t cnt = std::min(CH, n - s0);
            float* const buf = stage[k & 1];
            const auto tq0 = std::chrono::steady_clock::now();
            if (pinned && k >= 2) err = hipEventSynchronize(done[k & 1]);       // the copy that last read this buffer is through
            if (err != hipSuccess) break;
            const auto tq1 = std::chrono::steady_clock::now();
            if (cnt >= 65536) {          // a chunk is interleaved by up to eight threads, each on its own run of samples
                const unsigned hw = std::thread::hardware_concurrency();
                static const int pack_max = getenv("EH_PACK_THREADS") ? std::max(1, atoi(getenv("EH_PACK_THREADS"))) : 8;
                const int nthr = (int)std::max<int64_t>(2, std::min<int64_t>({(int64_t)pack_max, (int64_t)(hw ? hw / 2 : 2), cnt / 32768}));
                const int64_t per = (cnt + nthr - 1) / nthr;
                std::vector<std::thread> others;
                int64_t mine_end = std::min(s0 + cnt, s0 + per);
                try {                    // (no exception crosses the C ABI: a thread that cannot be started leaves its run of samples to this one)
                    for (int w = 1; w < nthr; ++w) {
                        const int64_t a0 = s0 + w * per, a1 = std::min(s0 + cnt, a0 + per);
                        if (a0 < a1) others.emplace_back([&, a0, a1] { pack(buf, a0, a1, s0); });
                    }
                } catch (...) {
                    for (auto& t : others) t.join();
                    others.clear();
                    mine_end = s0 + cnt;         // single-threaded: everything (the threads that did start packed the same values into the same places)
                }
                pack(buf, s0, mine_end, s0);
                for (auto& t : others) t.join();
            } else pack(buf, s0, s0 + cnt, s0);
            const auto tq2 = std::chrono::steady_clock::now();
            if (pinned) {
                err = hipMemcpyAsync(sp.recs + (size_t)s0 * C, buf, (size_t)cnt * C * sizeof(float), hipMemcpyHostToDevice, h->stream);
                if (err == hipSuccess) err = hipEventRecord(done[k & 1], h->stream);
                if (dbg_t) {
                    auto ms = [](std::chrono::steady_clock::time_point u, std::chrono::steady_clock::time_point v) { return std::chrono::duration<double, std::milli>(v - u).count(); };
                    fprintf(stderr, "   chunk %d: wait %.2f pack %.2f enqueue %.2f ms\n", k, ms(tq0, tq1), ms(tq1, tq2), ms(tq2, std::chrono::steady_clock::now()));
                }
            } else err = hipMemcpy(sp.recs + (size_t)s0 * C, buf, (size_t)cnt * C * sizeof(float), hipMemcpyHostToDevice);
        }
        // always drained before the staging pair is released or handed to the next caller -- also after an error: copies of earlier chunks
        // may still be reading it (advisor, round 4)
        const auto t_d = std::chrono::steady_clock::now();
        { const hipError_t es = hipStreamSynchronize(h->stream); if (err == hipSuccess) err = es; }
        if (dbg_t) {
            auto ms = [](std::chrono::steady_clock::time_point u, std::chrono::steady_clock::time_point v) { return std::chrono::duration<double, std::milli>(v - u).count(); };
            fprintf(stderr, "eh_set_data n=%lld: hipMalloc %.2f ms, staging (pooled %d pinned %d) %.2f ms, pack + enqueue %.2f ms, drain %.2f ms\n", (long long)n, ms(t_a, t_b), (int)pooled, (int)pinned,
                    ms(t_b, t_c), ms(t_c, t_d), ms(t_d, std::chrono::steady_clock::now()));
        }
        if (pinned) { (void)hipEventDestroy(done[0]); (void)hipEventDestroy(done[1]); if (!pooled) { (void)hipHostFree(stage[0]); (void)hipHostFree(stage[1]); } }
        HIPCHK(h, err);
    }
    sp.n = n;
    return EH_OK;
}

int32_t eh_set_sequences(eh_handle* h, int32_t split, int32_t input_window, int32_t output_window, int32_t lead_time, const int32_t* starts, int64_t n_windows) {
    if (!h) return EH_EINVAL;
    if (!h->seq) return fail(h, EH_EUNSUPPORTED, "eh_set_sequences: the model has no LSTM layer (EH_LAYER_LSTM): its samples are single records");
    if (split != EH_SPLIT_TRAIN && split != EH_SPLIT_VAL) return fail(h, EH_EINVAL, "eh_set_sequences: split %d", split);
    if (input_window < 1 || input_window > EH_MAX_SEQ_WINDOW) return fail(h, EH_EINVAL, "eh_set_sequences: input_window %d (1..%d)", input_window, EH_MAX_SEQ_WINDOW);
    if (output_window < 1 || output_window > input_window) return fail(h, EH_EINVAL, "eh_set_sequences: output_window %d (1..input_window = %d)", output_window, input_window);
    if (lead_time < 0) return fail(h, EH_EINVAL, "eh_set_sequences: lead_time %d", lead_time);
    if (n_windows < 0 || n_windows > 0x7fffffffLL || (n_windows > 0 && !starts)) return fail(h, EH_EINVAL, "eh_set_sequences: n_windows = %lld", (long long)n_windows);
    EhSplit& sp = h->split[split];
    if (!sp.recs || sp.n == 0) return fail(h, EH_ESTATE, "eh_set_sequences: no data set for this split (call eh_set_data first)");
    const long long last = sp.n - input_window - lead_time;      // (every row a window reads -- inputs, forcings, targets -- lies inside the series)
    for (int64_t i = 0; i < n_windows; ++i)
        if (starts[i] < 0 || starts[i] > last) return fail(h, EH_EINVAL, "eh_set_sequences: starts[%lld] = %d outside 0..%lld (series of %lld rows, input_window %d, lead_time %d)", (long long)i, starts[i], last, sp.n, input_window, lead_time);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    (void)hipFree(sp.starts);
    sp.starts = nullptr; sp.nwin = 0;
    if (split == EH_SPLIT_TRAIN) h->perm_valid = false;
    HIPCHK(h, hipMalloc(&sp.starts, (size_t)std::max<int64_t>(n_windows, 1) * sizeof(int)));
    if (n_windows > 0) HIPCHK(h, hipMemcpy(sp.starts, starts, (size_t)n_windows * sizeof(int), hipMemcpyHostToDevice));
    sp.nwin = n_windows; sp.W = input_window; sp.ow = output_window; sp.lam = lead_time;
    return EH_OK;
}

}   // extern "C"

// A large result array to the caller's (pageable) memory: through the pinned staging pair of eh_set_data, chunk k + 1 on its way over
// PCIe while chunk k is copied out by the CPU.  (hipMemcpy straight into pageable memory pins the destination pages behind the
// scenes; with 50 MB of predictions per train() call on the headline data set that cost 1-27 ms per call depending on where the
// allocator had put the arrays -- and whatever the runtime queued to undo it made the NEXT call's first upload chunk wait 15-28 ms
// (tools/e2e_breakdown2.py).)  Small arrays, or a staging pair that is busy or cannot be had: the plain copy.
int eh_copy_out(eh_handle* h, float* dst, const float* src_dev, size_t n) {
    const size_t bytes = n * sizeof(float);
    std::unique_lock<std::mutex> lk(g_stage_mu, std::try_to_lock);
    if (bytes < ((size_t)256 << 10) || !lk.owns_lock()) { HIPCHK(h, hipMemcpy(dst, src_dev, bytes, hipMemcpyDeviceToHost)); return EH_OK; }
    const size_t want = (size_t)8 << 20;                     // 8 MB chunks
    if (!stage_ensure(want)) { HIPCHK(h, hipMemcpy(dst, src_dev, bytes, hipMemcpyDeviceToHost)); return EH_OK; }
    const size_t CH = std::min(g_stage_bytes, want) / sizeof(float);
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIPCHK(h, hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
    { const hipError_t e = hipEventCreateWithFlags(&ev[1], hipEventDisableTiming); if (e != hipSuccess) { (void)hipEventDestroy(ev[0]); HIPCHK(h, e); } }
    hipError_t err = hipSuccess;
    const size_t nch = (n + CH - 1) / CH;
    for (size_t k = 0; k <= nch && err == hipSuccess; ++k) {
        if (k < nch) {                                       // chunk k: device -> stage[k & 1]
            const size_t off = k * CH, cnt = std::min(CH, n - off);
            err = hipMemcpyAsync(g_stage[k & 1], src_dev + off, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream);
            if (err == hipSuccess) err = hipEventRecord(ev[k & 1], h->stream);
        }
        if (k >= 1 && err == hipSuccess) {                   // chunk k - 1: stage -> caller
            const size_t off = (k - 1) * CH, cnt = std::min(CH, n - off);
            err = hipEventSynchronize(ev[(k - 1) & 1]);
            if (err == hipSuccess) memcpy(dst + off, g_stage[(k - 1) & 1], cnt * sizeof(float));
        }
    }
    { const hipError_t es = hipStreamSynchronize(h->stream); if (err == hipSuccess) err = es; }      // (the pair is not handed on with a copy in flight)
    (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
    HIPCHK(h, err);
    return EH_OK;
}
// ... and the other way (the parameter vector of a wide model, eh_set_params: 2.8 MB for the tutorial's large net -- a plain hipMemcpy from
// pageable memory was 3 ms of every train() call and 33 ms of one call in eight, tools/e2e_spikes.py)
int eh_copy_in(eh_handle* h, float* dst_dev, const float* src, size_t n) {
    const size_t bytes = n * sizeof(float);
    std::unique_lock<std::mutex> lk(g_stage_mu, std::try_to_lock);
    const size_t want = (size_t)8 << 20;
    if (bytes < ((size_t)256 << 10) || !lk.owns_lock()) { HIPCHK(h, hipMemcpy(dst_dev, src, bytes, hipMemcpyHostToDevice)); return EH_OK; }
    if (!stage_ensure(want)) { HIPCHK(h, hipMemcpy(dst_dev, src, bytes, hipMemcpyHostToDevice)); return EH_OK; }
    const size_t CH = want / sizeof(float);
    hipError_t err = hipSuccess;
    for (size_t off = 0, k = 0; off < n && err == hipSuccess; off += CH, ++k) {
        const size_t cnt = std::min(CH, n - off);
        if (k >= 2) err = hipStreamSynchronize(h->stream);          // (the buffer about to be refilled has been read)
        if (err != hipSuccess) break;
        memcpy(g_stage[k & 1], src + off, cnt * sizeof(float));
        err = hipMemcpyAsync(dst_dev + off, g_stage[k & 1], cnt * sizeof(float), hipMemcpyHostToDevice, h->stream);
    }
    { const hipError_t es = hipStreamSynchronize(h->stream); if (err == hipSuccess) err = es; }
    HIPCHK(h, err);
    return EH_OK;
}
