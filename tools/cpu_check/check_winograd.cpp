// Runs videoswap_amd/csrc/winograd.hip (Winograd F(2x2, 3x3): input transform, output transform + epilogue, and the entry
// point around its batched vsx_gemm_f16 launch) on the CPU from the real source, under AddressSanitizer and
// UBSan, and compares with double-precision loops.  Every buffer has exactly the size the entry point is told (the
// workspace exactly vsx_conv3x3_winograd_workspace bytes), so a read or write past a tensor is a sanitizer report.
//   make -C tools/cpu_check check_winograd && tools/cpu_check/check_winograd
#ifdef CHECK_WINOGRAD_REAL_GEMM
#define CPUHIP_DYNAMIC_LDS_ONLY
#include "hip/hip_runtime.h"
#include "hip_gemm.h"

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <utility>

// ---- pieces of the HIP runtime / gfx950 builtins only gemm.hip needs (as in check_gemm_api.cpp) ----
struct uint2 { unsigned x, y; };
static inline uint2 make_uint2(unsigned a, unsigned b) { return uint2{a, b}; }
typedef void* hipEvent_t;
static inline hipError_t hipEventCreate(hipEvent_t* e) { *e = nullptr; return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
static inline hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static inline long long clock64() { return 0; }
struct cpuhip_u2 { unsigned v[2]; unsigned operator[](int i) const { return v[i]; } };
static inline cpuhip_u2 cpuhip_permlane32_swap(unsigned vdst, unsigned src) {
    unsigned* s = static_cast<unsigned*>(cpuhip::ctx.wave_scratch);
    const int l = (int)(cpuhip::ctx.tid.x & 63);
    s[l] = vdst;
    s[64 + l] = src;
    cpuhip::ctx.wave_bar->arrive_and_wait();
    cpuhip_u2 r;
    r.v[0] = l >= 32 ? s[64 + l - 32] : vdst;
    r.v[1] = l < 32 ? s[l + 32] : src;
    cpuhip::ctx.wave_bar->arrive_and_wait();
    return r;
}
#define __builtin_amdgcn_permlane32_swap(a, b, fi, bc) cpuhip_permlane32_swap(a, b)

#include "common.h"

int vsx_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fprintf(stderr, "\n");
    return code;
}
int vsx_check_launch(const char*) { return 0; }

#include "gemm_common.h"
namespace vsxg {
namespace {
CPUHIP_DEFINE_LDS
}
}
#include "gemm_pp.hip"
namespace {
CPUHIP_DEFINE_LDS
}
#include "gemm.hip"
#include "options.cpp"
#include "prof.cpp"
#else
// Default build: the GEMM stage is a stand-in that executes the batched description the entry point hands to vsx_gemm_f16
// element by element (fp32 sums, one rounding), reading and writing exactly what the description names; the real
// vsx_gemm_f16 has its own check (check_gemm_api.cpp).  -DCHECK_WINOGRAD_REAL_GEMM compiles the real GEMM sources in
// instead (make check_winograd_gemm: a minute of compilation, a minute of run time).
#include "hip/hip_runtime.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>

#include "common.h"

static long cpuhip_oob_reads = 0;
int vsx_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fprintf(stderr, "\n");
    return code;
}
int vsx_check_launch(const char*) { return 0; }
#include "options.cpp"

static int n_gemm_bad = 0;
extern "C" int vsx_gemm_f16(const vsx_gemm_desc* d, vsx_stream_t) {
    // the GEMM stage of include/vsx.h: plain rows, a batch of 16, no epilogue
    if (d->a_mode != 0 || d->batch0 != 16 || d->batch1 != 1 || d->bias || d->rowvec || d->residual || d->geglu || d->c_mode ||
        d->rowscale || d->rowstats || d->alpha != 1.0 || d->workspace)
        return ++n_gemm_bad, VSX_E_UNSUPPORTED;
    const half_t* A = (const half_t*)d->A;
    const half_t* B = (const half_t*)d->B;
    half_t* C = (half_t*)d->C;
    for (int64_t z = 0; z < d->batch0; ++z)
        for (int64_t m = 0; m < d->M; ++m)
            for (int64_t n = 0; n < d->N; ++n) {
                float acc = 0.f;
                for (int64_t k = 0; k < d->K; ++k) acc += (float)A[z * d->a_bs0 + m * d->lda + k] * (float)B[z * d->b_bs0 + n * d->ldb + k];
                C[z * d->c_bs0 + m * d->ldc + n] = (half_t)acc;
            }
    return VSX_OK;
}
#endif
#include "winograd.hip"

static unsigned rng_state = 31337u;
static float frand() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((rng_state >> 8) & 0xFFFF) / 32768.0f - 1.0f;
}

// exactly `n` halves at a 16-byte boundary: the sanitizer's red zone starts right behind the last one
struct HBuf {
    half_t* p = nullptr;
    size_t n = 0;
    explicit HBuf(size_t n_, float scale = 0.f) : n(n_) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, (n ? n : 1) * sizeof(half_t))) abort();
        p = (half_t*)q;
        for (size_t i = 0; i < n; ++i) p[i] = (half_t)(scale != 0.f ? frand() * scale : 0.f);
    }
    HBuf(const HBuf&) = delete;
    ~HBuf() { free(p); }
    double operator[](size_t i) const { return (double)p[i]; }
};

static int n_bad = 0;
static void verdict(const char* name, int rc, double num, double den, double tol) {
    const double rel = sqrt(num / (den > 0 ? den : 1));
    const bool ok = rc == 0 && rel < tol && cpuhip_oob_reads == 0;
    printf("%-72s rc %d rel-L2 %.2e %s%s\n", name, rc, rel, cpuhip_oob_reads ? "reads past a tensor " : "", ok ? "ok" : "FAIL");
    if (!ok) ++n_bad;
    cpuhip_oob_reads = 0;
}

static const double BT[4][4] = {{1, 0, -1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}, {0, 1, 0, -1}};
static const double AT[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};
static const double G[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};

// rpv: rows_per_vec (0: two images); cpad, rpad: ldc = N + cpad, ldr = N + rpad
struct Geo { int nimg, H, W, C1, C2, N; bool bias, rowvec, res; long rpv = 0; int cpad = 0, rpad = 0; };

static double pixel(const HBuf& a, const HBuf& a2, const Geo& g, int img, int y, int x, int c) {
    if (y < 0 || y >= g.H || x < 0 || x >= g.W) return 0.0;
    const size_t pix = ((size_t)img * g.H + y) * g.W + x;
    return c < g.C1 ? a[pix * g.C1 + c] : a2[pix * g.C2 + (c - g.C1)];
}

// the input transform kernel alone against B^T d B in double: one fp16 rounding apart
static void run_input(const Geo& g) {
    const int C = g.C1 + g.C2, th = g.H / 2, tw = g.W / 2;
    const long tiles = (long)g.nimg * th * tw;
    HBuf a((size_t)g.nimg * g.H * g.W * g.C1, 1.f), a2((size_t)g.nimg * g.H * g.W * g.C2, 1.f), v((size_t)16 * tiles * C);
    WinoIn p;
    p.A = a.p; p.A2 = g.C2 ? a2.p : nullptr; p.V = v.p;
    p.H = g.H; p.W = g.W; p.C1 = g.C1; p.C2 = g.C2; p.th = th; p.tw = tw; p.tiles = tiles;
    const long n = tiles * (C / 8);
    hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)((n + WG_THREADS - 1) / WG_THREADS)), dim3(WG_THREADS), 0, nullptr, p);
    double num = 0, den = 0;
    for (long t = 0; t < tiles; ++t) {
        const int img = (int)(t / (th * tw)), ti = (int)(t % (th * tw)) / tw, tj = (int)(t % tw);
        for (int c = 0; c < C; ++c)
            for (int xa = 0; xa < 4; ++xa)
                for (int xb = 0; xb < 4; ++xb) {
                    double want = 0;
                    for (int r = 0; r < 4; ++r)
                        for (int s = 0; s < 4; ++s) want += BT[xa][r] * pixel(a, a2, g, img, 2 * ti - 1 + r, 2 * tj - 1 + s, c) * BT[xb][s];
                    const double d = v[((size_t)(4 * xa + xb) * tiles + t) * C + c] - want;
                    num += d * d;
                    den += want * want;
                }
    }
    char name[128];
    snprintf(name, sizeof(name), "input transform %dx%dx%d C=%d+%d", g.nimg, g.H, g.W, g.C1, g.C2);
    verdict(name, 0, num, den, 4e-4);                    // one rounding to fp16: 2^-11 / sqrt 3 = 2.8e-4 at the worst
}

// rows_per_vec: what the geometry names, else a vector spans two images
static long rpv(const Geo& g) { return g.rpv ? g.rpv : 2L * g.H * g.W; }

// C with ldc = N + cpad: exactly (M - 1) ldc + N halves (a store behind the last row's N columns is a sanitizer report), the pad
// columns of the other rows hold a sentinel that must survive the call
static const float PAD_SENTINEL = 777.f;
static size_t padded(long M, int N, int pad) { return (size_t)(M - 1) * (N + pad) + N; }
static void fill_pads(HBuf& y, long M, int N, int pad) {
    for (long r = 0; r + 1 < M; ++r)
        for (int c = N; c < N + pad; ++c) y.p[(size_t)r * (N + pad) + c] = (half_t)PAD_SENTINEL;
}
static bool pads_intact(const HBuf& y, long M, int N, int pad) {
    for (long r = 0; r + 1 < M; ++r)
        for (int c = N; c < N + pad; ++c)
            if (y[(size_t)r * (N + pad) + c] != (double)PAD_SENTINEL) return false;
    return true;
}
static void tag(char* name, size_t n, const Geo& g) {
    const size_t at = strlen(name);
    if (g.rpv || g.cpad || g.rpad) snprintf(name + at, n - at, " rpv %ld ldc N+%d ldr N+%d", rpv(g), g.cpad, g.rpad);
}

static double epilogue(const Geo& g, const HBuf& bias, const HBuf& rowvec, const HBuf& res, long row, int n) {
    double e = 0;
    if (g.bias) e += bias[n];
    if (g.rowvec) e += rowvec[(size_t)(row / rpv(g)) * g.N + n];
    if (g.res) e += res[(size_t)row * (g.N + g.rpad) + n];
    return e;
}

// the output transform kernel alone against A^T Mt A + epilogue in double
static void run_output(const Geo& g) {
    const int th = g.H / 2, tw = g.W / 2;
    const long tiles = (long)g.nimg * th * tw, M = 4 * tiles;
    HBuf mt((size_t)16 * tiles * g.N, 1.f), y(padded(M, g.N, g.cpad)), bias(g.N, 0.5f), rowvec((size_t)((M + rpv(g) - 1) / rpv(g)) * g.N, 0.5f);
    HBuf res(padded(M, g.N, g.rpad), 1.f);
    fill_pads(y, M, g.N, g.cpad);
    WinoOut p;
    p.Mt = mt.p; p.Y = y.p; p.bias = g.bias ? bias.p : nullptr; p.rowvec = g.rowvec ? rowvec.p : nullptr;
    p.residual = g.res ? res.p : nullptr;
    p.rows_per_vec = rpv(g); p.ldc = g.N + g.cpad; p.ldr = g.N + g.rpad;
    p.H = g.H; p.W = g.W; p.N = g.N; p.th = th; p.tw = tw; p.tiles = tiles;
    const long n = tiles * (g.N / 8);
    hipLaunchKernelGGL(wino_output_kernel, dim3((unsigned)((n + WG_THREADS - 1) / WG_THREADS)), dim3(WG_THREADS), 0, nullptr, p);
    double num = 0, den = 0;
    for (long t = 0; t < tiles; ++t) {
        const int img = (int)(t / (th * tw)), ti = (int)(t % (th * tw)) / tw, tj = (int)(t % tw);
        for (int c = 0; c < g.N; ++c)
            for (int pi = 0; pi < 2; ++pi)
                for (int pj = 0; pj < 2; ++pj) {
                    double want = 0;
                    for (int xa = 0; xa < 4; ++xa)
                        for (int xb = 0; xb < 4; ++xb) want += AT[pi][xa] * mt[((size_t)(4 * xa + xb) * tiles + t) * g.N + c] * AT[pj][xb];
                    const long row = ((long)img * g.H + 2 * ti + pi) * g.W + 2 * tj + pj;
                    want += epilogue(g, bias, rowvec, res, row, c);
                    const double d = y[(size_t)row * (g.N + g.cpad) + c] - want;
                    num += d * d;
                    den += want * want;
                }
    }
    char name[128];
    snprintf(name, sizeof(name), "output transform %dx%dx%d N=%d%s%s%s", g.nimg, g.H, g.W, g.N, g.bias ? " bias" : "", g.rowvec ? " rowvec" : "",
             g.res ? " residual" : "");
    tag(name, sizeof(name), g);
    verdict(name, pads_intact(y, M, g.N, g.cpad) ? 0 : -1, num, den, 4e-4);
}

static vsx_gemm_desc conv_desc(const Geo& g) {
    vsx_gemm_desc d = {};
    d.M = (int64_t)g.nimg * g.H * g.W; d.N = g.N; d.K = 9 * (g.C1 + g.C2);
    d.batch0 = d.batch1 = 1;
    d.a_mode = 1; d.H = g.H; d.W = g.W; d.C1 = g.C1; d.C2 = g.C2; d.ks = 3; d.stride = 1;
    d.ldb = d.K; d.ldc = g.N + g.cpad; d.ldr = g.N + g.rpad; d.alpha = 1.0;
    d.pad_lo = d.pad_hi = -1;
    return d;
}

// the entry point against the nine-tap convolution in double
static void run_entry(const Geo& g) {
    const int C = g.C1 + g.C2;
    const long M = (long)g.nimg * g.H * g.W, tiles = M / 4;
    const float wscale = 1.0f / sqrtf(9.0f * C);
    HBuf a((size_t)M * g.C1, 1.f), a2((size_t)M * g.C2, 1.f), w((size_t)g.N * 9 * C, wscale), u((size_t)16 * g.N * C), y(padded(M, g.N, g.cpad));
    HBuf bias(g.N, 0.5f), rowvec((size_t)((M + rpv(g) - 1) / rpv(g)) * g.N, 0.5f), res(padded(M, g.N, g.rpad), 1.f);
    fill_pads(y, M, g.N, g.cpad);
    for (int n = 0; n < g.N; ++n)                        // U = G g G^T, rounded once (videoswap_amd.ops.winograd_weights)
        for (int c = 0; c < C; ++c)
            for (int xa = 0; xa < 4; ++xa)
                for (int xb = 0; xb < 4; ++xb) {
                    double s = 0;
                    for (int r = 0; r < 3; ++r)
                        for (int q = 0; q < 3; ++q) s += G[xa][r] * w[((size_t)n * 9 + 3 * r + q) * C + c] * G[xb][q];
                    u.p[((size_t)(4 * xa + xb) * g.N + n) * C + c] = (half_t)(float)s;
                }
    vsx_gemm_desc d = conv_desc(g);
    d.A = a.p; d.A2 = g.C2 ? a2.p : nullptr; d.B = w.p; d.C = y.p;
    d.bias = g.bias ? bias.p : nullptr;
    d.rowvec = g.rowvec ? rowvec.p : nullptr; d.rows_per_vec = g.rowvec ? rpv(g) : 0;
    d.residual = g.res ? res.p : nullptr;
    const int64_t need = vsx_conv3x3_winograd_workspace(&d);
    bool ok = need == 16 * tiles * (C + g.N) * 2;
    HBuf ws((size_t)need / 2);
    int rc = ok ? vsx_conv3x3_winograd_f16(&d, u.p, ws.p, need, nullptr) : -100;
    if (rc == 0 && !pads_intact(y, M, g.N, g.cpad)) rc = -101;
    double num = 0, den = 0;
    for (int img = 0; img < g.nimg; ++img)
        for (int yy = 0; yy < g.H; ++yy)
            for (int xx = 0; xx < g.W; ++xx) {
                const long row = ((long)img * g.H + yy) * g.W + xx;
                for (int n = 0; n < g.N; ++n) {
                    double want = 0;
                    for (int r = 0; r < 3; ++r)
                        for (int q = 0; q < 3; ++q)
                            for (int c = 0; c < C; ++c) want += w[((size_t)n * 9 + 3 * r + q) * C + c] * pixel(a, a2, g, img, yy - 1 + r, xx - 1 + q, c);
                    want += epilogue(g, bias, rowvec, res, row, n);
                    const double dd = y[(size_t)row * (g.N + g.cpad) + n] - want;
                    num += dd * dd;
                    den += want * want;
                }
            }
    char name[128];
    snprintf(name, sizeof(name), "entry point %dx%dx%d C=%d+%d N=%d%s%s%s", g.nimg, g.H, g.W, g.C1, g.C2, g.N, g.bias ? " bias" : "",
             g.rowvec ? " rowvec" : "", g.res ? " residual" : "");
    tag(name, sizeof(name), g);
    verdict(name, rc, num, den, 2e-3);                   // the project's bound for a convolution (the form sits near 6e-4)
}

static void run_refusals() {
    HBuf t(64);
    auto rc_of = [&](vsx_gemm_desc d) {
        d.A = t.p; d.B = t.p; d.C = t.p;
        if (d.C2) d.A2 = t.p;
        const bool none = vsx_conv3x3_winograd_workspace(&d) == 0 && vsx_conv3x3_winograd_auto(&d) == 0;
        return none ? vsx_conv3x3_winograd_f16(&d, t.p, t.p, 1 << 30, nullptr) : 0;
    };
    const Geo base{1, 4, 6, 8, 0, 8, true, false, false};
    bool ok = true;
    { Geo g = base; g.H = 5; ok = ok && rc_of(conv_desc(g)) == VSX_E_UNSUPPORTED; }               // odd H
    { Geo g = base; g.W = 7; ok = ok && rc_of(conv_desc(g)) == VSX_E_UNSUPPORTED; }               // odd W
    { vsx_gemm_desc d = conv_desc(base); d.stride = 2; ok = ok && rc_of(d) == VSX_E_UNSUPPORTED; }
    { vsx_gemm_desc d = conv_desc(base); d.upsample = 1; ok = ok && rc_of(d) == VSX_E_UNSUPPORTED; }
    { vsx_gemm_desc d = conv_desc(base); d.ks = 1; d.K = 8; ok = ok && rc_of(d) == VSX_E_UNSUPPORTED; }
    { vsx_gemm_desc d = conv_desc(base); d.pad_lo = 0; d.pad_hi = 1; ok = ok && rc_of(d) == VSX_E_UNSUPPORTED; }
    { vsx_gemm_desc d = conv_desc(base); d.geglu = 1; ok = ok && rc_of(d) == VSX_E_UNSUPPORTED; }
    { vsx_gemm_desc d = conv_desc(base); d.a_mode = 0; ok = ok && rc_of(d) == VSX_E_UNSUPPORTED; }
    { Geo g = base; g.C2 = 8; ok = ok && rc_of(conv_desc(g)) == VSX_E_UNSUPPORTED; }              // two sources below 64 channels
    { Geo g = base; g.N = 12; ok = ok && rc_of(conv_desc(g)) == VSX_E_UNSUPPORTED; }
    {                                                                                            // a workspace one byte short
        vsx_gemm_desc d = conv_desc(base);
        d.A = t.p; d.B = t.p; d.C = t.p;
        ok = ok && vsx_conv3x3_winograd_f16(&d, t.p, t.p, vsx_conv3x3_winograd_workspace(&d) - 1, nullptr) == VSX_E_WORKSPACE;
    }
    verdict("refusals (nothing is read or written)", ok ? 0 : -1, 0.0, 1.0, 1.0);
}

int main() {
    const int spatial[3][2] = {{2, 2}, {4, 6}, {8, 8}};   // 2 x 2: every window touches the padding on all sides
    const int chans[3][2] = {{8, 0}, {72, 0}, {64, 64}};
    for (int nimg : {1, 3})
        for (auto& hw : spatial) {
            for (auto& c : chans) run_input(Geo{nimg, hw[0], hw[1], c[0], c[1], 8, false, false, false});
            for (int N : {8, 40})
                for (int e = 0; e < 8; ++e) run_output(Geo{nimg, hw[0], hw[1], 8, 0, N, (e & 1) != 0, (e & 2) != 0, (e & 4) != 0});
        }
    // the entry point: every geometry, the eight epilogue combinations taken in turn ...
    int e = 0;
    for (int nimg : {1, 3})
        for (auto& hw : spatial)
            for (auto& c : chans)
                for (int N : {8, 40}) {
                    run_entry(Geo{nimg, hw[0], hw[1], c[0], c[1], N, (e & 1) != 0, (e & 2) != 0, (e & 4) != 0});
                    e = (e + 3) % 8;
                }
    // ... and all eight on one geometry (two sources, non-square, a row vector shared by two of the three images)
    for (e = 0; e < 8; ++e) run_entry(Geo{3, 4, 6, 64, 64, 40, (e & 1) != 0, (e & 2) != 0, (e & 4) != 0});
    // the edges tests/winograd_case.py aims the GPU parity cases at, from this program's own double loops: rows_per_vec = W (the two
    // rows of a tile take different vectors) and 3 (the two columns do), ldc > N with ldr != ldc above and below it, one tile per
    // image under both, and two sources of different widths in both orders
    for (long r : {6L, 3L, 1L}) {
        run_output(Geo{3, 4, 6, 8, 0, 40, true, true, true, r});
        run_entry(Geo{3, 4, 6, 72, 0, 40, true, true, true, r});
    }
    for (auto& pads : {std::pair<int, int>{8, 16}, {16, 0}, {0, 8}}) {
        run_output(Geo{3, 4, 6, 8, 0, 40, true, true, true, 0, pads.first, pads.second});
        run_entry(Geo{3, 4, 6, 72, 0, 40, true, true, true, 6, pads.first, pads.second});
    }
    run_output(Geo{3, 2, 2, 8, 0, 8, true, true, true, 2, 8, 0});
    run_entry(Geo{3, 2, 2, 8, 0, 8, true, true, true, 3, 8, 16});
    for (auto& c : {std::pair<int, int>{64, 128}, {128, 64}}) {
        run_input(Geo{3, 4, 6, c.first, c.second, 8, false, false, false});
        run_entry(Geo{3, 4, 6, c.first, c.second, 40, true, true, true, 3, 8, 0});
    }
    run_refusals();
#ifndef CHECK_WINOGRAD_REAL_GEMM
    if (n_gemm_bad) printf("the GEMM stage was handed %d description(s) that are not a plain batch of 16 FAIL\n", n_gemm_bad), ++n_bad;
#endif
    if (n_bad) {
        printf("%d check(s) FAILED\n", n_bad);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
