// ---- instrumentation (bench.py roofline): hipEvent pairs around sampled launches ----
#include "prof.h"

#include <vector>

namespace {

struct ProfState {
    bool on = false;
    bool paused = false;
    long max_samples = 0;
    long stride = 1, seen = 0;
    long n = 0;
    double flop = 0.0;
    std::vector<hipEvent_t>* ev = nullptr;  // 2 per sample
    std::vector<double>* work = nullptr;    // 2 per sample: algorithmic FLOP, algorithmic bytes (vsx_prof_collect_roofline)
};

ProfState g_prof;

}  // namespace

namespace vsxg {

long prof_begin(hipStream_t stream) {
    const bool sample = g_prof.on && !g_prof.paused && g_prof.n < g_prof.max_samples && (g_prof.seen++ % g_prof.stride) == 0;
    if (!sample) return PROF_NOT_SAMPLED;
    if ((long)g_prof.ev->size() < 2 * (g_prof.n + 1)) {       // events are created when the first launch needs them, and kept
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            (void)vsx_fail(VSX_E_LAUNCH, "prof: hipEventCreate failed");
            return PROF_FAILED;
        }
        g_prof.ev->push_back(a);
        g_prof.ev->push_back(b);
    }
    (void)hipEventRecord((*g_prof.ev)[2 * g_prof.n], stream);
    return g_prof.n;
}

void prof_end(long handle, hipStream_t stream, double flop, double bytes) {
    (void)hipEventRecord((*g_prof.ev)[2 * handle + 1], stream);
    g_prof.n += 1;
    g_prof.flop += flop;
    g_prof.work->push_back(flop);
    g_prof.work->push_back(bytes);
}

}  // namespace vsxg

extern "C" int vsx_prof_enable(int64_t on, int64_t max_samples) {
    if (!g_prof.ev) g_prof.ev = new std::vector<hipEvent_t>();
    if (!g_prof.work) g_prof.work = new std::vector<double>();
    g_prof.work->clear();
    g_prof.on = on != 0;
    g_prof.stride = on > 1 ? on : 1;        // on = k > 1: bracket every k-th launch only
    g_prof.seen = 0;
    g_prof.max_samples = max_samples;
    g_prof.n = 0;
    g_prof.flop = 0.0;
    return VSX_OK;
}

// suspend / resume sampling without touching what has been collected (HIP-graph capture and replayed calls)
extern "C" int vsx_prof_pause(int64_t paused) {
    g_prof.paused = paused != 0;
    return VSX_OK;
}

// Per sampled launch: duration t, algorithmic FLOP f and algorithmic bytes b (A once + weights once + C once + residual once; a
// convolution reads every input pixel once).  A launch cannot finish before max(f / peak_flops, b / peak_bytes_per_s): the sum of
// those floors over the samples is what the same launches would take on BOTH rooflines at once (`floor_ms`), and
// `byte_bound_ms` is the measured time of the launches whose byte floor is the larger one.
extern "C" int vsx_prof_collect_roofline(double peak_flops, double peak_bytes_per_s, int64_t* n_launches, double* total_ms,
                                         double* total_flop, double* total_bytes, double* floor_ms, double* byte_bound_ms) {
    double ms = 0.0, bytes = 0.0, floor = 0.0, bb = 0.0;
    if (g_prof.ev) {
        for (long i = 0; i < g_prof.n; ++i) {
            hipEvent_t a = (*g_prof.ev)[2 * i], b = (*g_prof.ev)[2 * i + 1];
            if (hipEventSynchronize(b) != hipSuccess) return vsx_fail(VSX_E_LAUNCH, "prof: event sync failed");
            float t = 0.f;
            if (hipEventElapsedTime(&t, a, b) != hipSuccess) return vsx_fail(VSX_E_LAUNCH, "prof: elapsed failed");
            ms += t;
            if (g_prof.work && (long)g_prof.work->size() >= 2 * (i + 1) && peak_flops > 0.0 && peak_bytes_per_s > 0.0) {
                const double f = (*g_prof.work)[2 * i], by = (*g_prof.work)[2 * i + 1];
                const double tf = f / peak_flops, tb = by / peak_bytes_per_s;
                bytes += by;
                floor += 1e3 * (tf > tb ? tf : tb);
                if (tb > tf) bb += t;
            }
        }
    }
    if (n_launches) *n_launches = g_prof.n;
    if (total_ms) *total_ms = ms;
    if (total_flop) *total_flop = g_prof.flop;
    if (total_bytes) *total_bytes = bytes;
    if (floor_ms) *floor_ms = floor;
    if (byte_bound_ms) *byte_bound_ms = bb;
    g_prof.n = 0;
    g_prof.flop = 0.0;
    if (g_prof.work) g_prof.work->clear();
    return VSX_OK;
}

extern "C" int vsx_prof_collect(int64_t* n_launches, double* total_ms, double* total_flop) {
    return vsx_prof_collect_roofline(0.0, 0.0, n_launches, total_ms, total_flop, nullptr, nullptr, nullptr);
}
