// Runs vsx_gemm_f16 — the C-ABI entry point with its shape checks, dispatch, the workgroup-per-tile kernels (gemm.hip), the
// persistent kernel (gemm_pp.hip) and the split-K combine — on the CPU from the real sources, and compares every case with a
// double-precision GEMM / convolution.  What check_gemm_pp.cpp is for the persistent kernel alone, this is for the whole
// entry point: dispatch thresholds (case 26: the plan of every UNet shape, pinned), tile-kernel epilogues (row-per-lane layout, permlane32 exchange, prefetched residual and
// bias), GEGLU, the transposed V^T store, split-K + combine, the LayerNorm fold.  See hip_gemm.h for what the emulation
// covers and what it cannot (asynchronous ordering of the LDS-DMA, register pressure, speed).
#define CPUHIP_DYNAMIC_LDS_ONLY
#include "hip/hip_runtime.h"
#include "hip_gemm.h"

#include <stdarg.h>

// ---- pieces of the HIP runtime / gfx950 builtins only gemm.hip needs ----
struct uint2 { unsigned x, y; };
static inline uint2 make_uint2(unsigned a, unsigned b) { return uint2{a, b}; }
typedef void* hipEvent_t;
static inline hipError_t hipEventCreate(hipEvent_t* e) { *e = nullptr; return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
static inline hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static inline long long clock64() { return 0; }
// v_permlane32_swap: lanes 32-63 of `vdst` trade places with lanes 0-31 of `src`; returns (new vdst, new src)
struct cpuhip_u2 { unsigned v[2]; unsigned operator[](int i) const { return v[i]; } };
static inline cpuhip_u2 cpuhip_permlane32_swap(unsigned vdst, unsigned src) {
    unsigned* s = static_cast<unsigned*>(cpuhip::ctx.wave_scratch);          // [0..63] vdst, [64..127] src
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


static unsigned rng_state = 4242u;
static float frand() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((rng_state >> 8) & 0xFFFF) / 32768.0f - 1.0f;
}
static std::vector<half_t> randh(size_t n, float scale = 1.0f) {
    std::vector<half_t> v(n);
    for (auto& x : v) x = (half_t)(frand() * scale);
    return v;
}
static double gelu(double x) { return 0.5 * x * (1.0 + erf(x / sqrt(2.0))); }
static int n_bad = 0;

static void report(const char* name, int rc, const std::vector<double>& want, const std::vector<half_t>& got, double tol = 3e-3) {
    double num = 0, den = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        const double d = (double)got[i] - want[i];
        num += d * d;
        den += want[i] * want[i];
    }
    const double rel = sqrt(num / (den > 0 ? den : 1));
    const bool ok = rc == 0 && rel < tol && cpuhip_oob_reads == 0;
    printf("%-58s rc %d rel-L2 %.2e %s%s\n", name, rc, rel, cpuhip_oob_reads ? "reads past a tensor " : "", ok ? "ok" : "FAIL");
    if (!ok) ++n_bad;
    cpuhip_oob_reads = 0;
}

// vsx_gemm_f16 through its three pieces, for the checks that look at what the launch made of the plan: *xcd_gm receives the XCD block
// grid of the tile launch (-1: another kernel family ran)
static int gemm_by_pieces(const vsx_gemm_desc& d, int* xcd_gm) {
    GemmParams p;
    int rc = fill_params(&d, p);
    if (rc != VSX_OK) return rc;
    const GemmPlan plan = plan_gemm(d, p, false);
    if (plan.refused) return VSX_E_UNSUPPORTED;
    if (plan.forced || plan.splits > 1) p.ws = (float*)d.workspace;
    rc = run_plan(plan, p, nullptr);
    *xcd_gm = plan.family == GEMM_TILE ? p.xcd_gm : -1;
    return rc;
}

struct Plain {
    const char* name;
    long M, N, K;
    bool res, rowvec, geglu, ln, vt;
    long rows_per_vec, rows_per_img;
    long pp;                // option gemm_pp for this case (0: tile kernels, 2: persistent kernel where eligible)
    bool splitk;
};

// plain GEMM through the public entry point, every epilogue kind of the descriptor
static std::vector<half_t> run_plain(const Plain& c, bool check = true, int* xcd_gm = nullptr) {
    const long brows = c.geglu ? 2 * c.N : c.N;
    auto A = randh((size_t)c.M * c.K), B = randh((size_t)brows * c.K, 1.0f / sqrtf((float)c.K)), bias = randh(brows);
    auto R = randh((size_t)c.M * c.N);
    const long nvec = c.rowvec ? (c.M + c.rows_per_vec - 1) / c.rows_per_vec : 1;
    auto RV = randh((size_t)nvec * c.N);
    std::vector<float> rowscale(2 * c.M), colvec(brows);
    for (long m = 0; m < c.M; ++m) { rowscale[2 * m] = 0.5f + 0.01f * (float)(m % 37); rowscale[2 * m + 1] = -0.3f + 0.02f * (float)(m % 11); }
    for (long n = 0; n < brows; ++n) { double s = 0; for (long k = 0; k < c.K; ++k) s += (double)B[n * c.K + k]; colvec[n] = (float)s; }
    auto dot = [&](long m, long row) {
        double s = 0;
        for (long k = 0; k < c.K; ++k) s += (double)A[m * c.K + k] * (double)B[row * c.K + k];
        if (c.ln) s = (double)rowscale[2 * m] * s + (double)rowscale[2 * m + 1] * (double)colvec[row];
        return s + (double)bias[row];
    };
    const long nimg = c.vt ? c.M / c.rows_per_img : 1;
    std::vector<double> want((size_t)c.M * c.N);
    for (long m = 0; m < c.M; ++m)
        for (long n = 0; n < c.N; ++n) {
            double v = c.geglu ? dot(m, n) * gelu(dot(m, c.N + n)) : dot(m, n);
            if (c.rowvec) v += (double)RV[(m / c.rows_per_vec) * c.N + n];
            if (c.res) v += (double)R[m * c.N + n];
            const size_t at = c.vt ? ((size_t)(m / c.rows_per_img) * c.N + n) * c.rows_per_img + m % c.rows_per_img : (size_t)m * c.N + n;
            want[at] = v;
        }
    std::vector<half_t> C((size_t)c.M * c.N, (half_t)-7.f);
    vsx_gemm_desc d{};
    d.M = c.M; d.N = c.N; d.K = c.K; d.batch0 = d.batch1 = 1;
    d.A = A.data(); d.lda = c.K; d.B = B.data(); d.ldb = c.K; d.C = C.data();
    d.ldc = c.vt ? c.rows_per_img : c.N;
    d.c_mode = c.vt ? 1 : 0; d.c_rows_per_img = c.vt ? c.rows_per_img : 0; d.c_img_stride = c.vt ? c.N * c.rows_per_img : 0;
    d.bias = bias.data();
    if (c.rowvec) { d.rowvec = RV.data(); d.rows_per_vec = c.rows_per_vec; }
    if (c.res) { d.residual = R.data(); d.ldr = c.N; }
    d.geglu = c.geglu; d.alpha = 1.0; d.pad_lo = d.pad_hi = -1;
    if (c.ln) { d.rowscale = rowscale.data(); d.colvec = colvec.data(); }
    std::vector<float> ws;
    if (c.splitk) {
        const int64_t bytes = vsx_gemm_workspace(&d);
        if (bytes <= 0) { printf("%-58s no split-K plan FAIL\n", c.name); ++n_bad; }
        ws.resize((size_t)bytes / 4 + 4);
        d.workspace = ws.data(); d.workspace_bytes = bytes;
    }
    (void)nimg;
    vsx_set_option("gemm_pp", c.pp);
    const int rc = xcd_gm ? gemm_by_pieces(d, xcd_gm) : vsx_gemm_f16(&d, nullptr);
    if (check) report(c.name, rc, want, C);
    return C;
}

// batched GEMM (attention scores: A [b0, b1, M, K], B [b0, b1, N, K])
static void run_batched(const char* name, long b0, long b1, long M, long N, long K) {
    const long nb = b0 * b1;
    auto A = randh((size_t)nb * M * K), B = randh((size_t)nb * N * K, 1.0f / sqrtf((float)K));
    std::vector<double> want((size_t)nb * M * N);
    for (long z = 0; z < nb; ++z)
        for (long m = 0; m < M; ++m)
            for (long n = 0; n < N; ++n) {
                double s = 0;
                for (long k = 0; k < K; ++k) s += (double)A[(z * M + m) * K + k] * (double)B[(z * N + n) * K + k];
                want[(z * M + m) * N + n] = 0.125 * s;
            }
    std::vector<half_t> C((size_t)nb * M * N, (half_t)-7.f);
    vsx_gemm_desc d{};
    d.M = M; d.N = N; d.K = K; d.batch0 = b0; d.batch1 = b1;
    d.A = A.data(); d.lda = K; d.a_bs1 = M * K; d.a_bs0 = b1 * M * K;
    d.B = B.data(); d.ldb = K; d.b_bs1 = N * K; d.b_bs0 = b1 * N * K;
    d.C = C.data(); d.ldc = N; d.c_bs1 = M * N; d.c_bs0 = b1 * M * N;
    d.alpha = 0.125; d.pad_lo = d.pad_hi = -1;
    vsx_set_option("gemm_pp", 1);
    report(name, vsx_gemm_f16(&d, nullptr), want, C);
}

// conv3x3(nearest_2x(x)) in its sub-pixel form (vsx_gemm_desc.upsample = 2): the four class matrices are built here the way
// videoswap_amd.ops.subpixel_weights does, the expectation is the NINE-tap convolution of the upsampled image with the original
// filter in double precision — the algebra, the descriptor handling and the scatter of the classes in one check.
static void run_subpixel(const char* name, int nimg, int Hs, int Ws, int C, int Cout) {
    const int H = 2 * Hs, W = 2 * Ws;
    const long M = (long)nimg * H * W, K = 9L * C;
    auto X = randh((size_t)nimg * Hs * Ws * C);
    auto Wt = randh((size_t)Cout * K, 1.0f / sqrtf((float)K)), bias = randh(Cout);
    std::vector<double> want((size_t)M * Cout);
    for (int i = 0; i < nimg; ++i)
        for (int ho = 0; ho < H; ++ho)
            for (int wo = 0; wo < W; ++wo)
                for (int co = 0; co < Cout; ++co) {
                    double s = (double)bias[co];
                    for (int kh = 0; kh < 3; ++kh)
                        for (int kw = 0; kw < 3; ++kw) {
                            const int h = ho - 1 + kh, w = wo - 1 + kw;
                            if (h < 0 || h >= H || w < 0 || w >= W) continue;
                            const half_t* wrow = Wt.data() + (size_t)co * K + (size_t)(kh * 3 + kw) * C;
                            const size_t pix = ((size_t)i * Hs + h / 2) * Ws + w / 2;
                            for (int c = 0; c < C; ++c) s += (double)X[pix * C + c] * (double)wrow[c];
                        }
                    want[((size_t)(i * H + ho) * W + wo) * Cout + co] = s;
                }
    // class 2 ph + pw: window tap (th, tw) of a pad-1 3x3 window on the source <- the filter taps that land on that source pixel
    std::vector<half_t> W4((size_t)4 * Cout * K, (half_t)0.f);
    const int taps[2][2][3] = {{{0, -1, -1}, {1, 2, -1}}, {{0, 1, -1}, {2, -1, -1}}};      // [parity][which of the two window taps] -> filter taps
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw)
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int co = 0; co < Cout; ++co)
                        for (int c = 0; c < C; ++c) {
                            float s = 0.f;
                            for (int fa = 0; fa < 3 && taps[ph][a][fa] >= 0; ++fa)
                                for (int fb = 0; fb < 3 && taps[pw][b][fb] >= 0; ++fb)
                                    s += (float)Wt[(size_t)co * K + (size_t)(taps[ph][a][fa] * 3 + taps[pw][b][fb]) * C + c];
                            W4[((size_t)(2 * ph + pw) * Cout + co) * K + (size_t)((ph + a) * 3 + (pw + b)) * C + c] = (half_t)s;
                        }
    std::vector<half_t> Cm((size_t)M * Cout, (half_t)-7.f);
    vsx_gemm_desc d{};
    d.M = M; d.N = Cout; d.K = K; d.batch0 = d.batch1 = 1;
    d.A = X.data(); d.a_mode = 1; d.H = H; d.W = W; d.C1 = C; d.ks = 3; d.stride = 1; d.upsample = 2;
    d.B = W4.data(); d.ldb = K; d.C = Cm.data(); d.ldc = Cout; d.bias = bias.data();
    d.alpha = 1.0; d.pad_lo = d.pad_hi = -1;
    vsx_set_option("gemm_pp", 2);
    const int rc = vsx_gemm_f16(&d, nullptr);
    vsx_set_option("gemm_pp", 1);
    report(name, rc, want, Cm);
    d.upsample = 2;
    const int rc2 = vsx_gemm_f16(&d, nullptr);          // too few tiles for the automatic choice: refused, not silently something else
    printf("%-58s rc %d %s\n", "  ... refused where the persistent kernel would not run", rc2, rc2 == VSX_E_UNSUPPORTED ? "ok" : "FAIL");
    if (rc2 != VSX_E_UNSUPPORTED) ++n_bad;
}

// 3x3 / 1x1 convolution with bias + time-embedding row vector + residual (both addends: the tile kernels)
static std::vector<half_t> run_conv(const char* name, int nimg, int H, int W, int C1, int C2, int Cout, int ks, int stride, int ups, bool splitk,
                                    long pp = 1, bool both_addends = true, int* xcd_gm = nullptr) {
    const int pad = ks / 2;
    const int Hs = ups ? H / 2 : H, Ws = ups ? W / 2 : W;
    const int Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
    const long M = (long)nimg * Ho * Wo, K = (long)ks * ks * (C1 + C2);
    auto X1 = randh((size_t)nimg * Hs * Ws * C1), X2 = randh((size_t)nimg * Hs * Ws * (C2 ? C2 : 1));
    auto Wt = randh((size_t)Cout * K, 1.0f / sqrtf((float)K)), bias = randh(Cout), rowvec = randh((size_t)nimg * Cout);
    auto R = randh((size_t)M * Cout);
    std::vector<double> want((size_t)M * Cout);
    for (int i = 0; i < nimg; ++i)
        for (int ho = 0; ho < Ho; ++ho)
            for (int wo = 0; wo < Wo; ++wo)
                for (int co = 0; co < Cout; ++co) {
                    const size_t at = ((size_t)(i * Ho + ho) * Wo + wo) * Cout + co;
                    double s = (double)bias[co] + (double)rowvec[(size_t)i * Cout + co] + (both_addends ? (double)R[at] : 0.0);
                    for (int kh = 0; kh < ks; ++kh)
                        for (int kw = 0; kw < ks; ++kw) {
                            const int h = ho * stride - pad + kh, w = wo * stride - pad + kw;
                            if (h < 0 || h >= H || w < 0 || w >= W) continue;
                            const int hs = ups ? h / 2 : h, wsrc = ups ? w / 2 : w;
                            const half_t* wrow = Wt.data() + (size_t)co * K + (size_t)(kh * ks + kw) * (C1 + C2);
                            const size_t pix = ((size_t)i * Hs + hs) * Ws + wsrc;
                            for (int c = 0; c < C1; ++c) s += (double)X1[pix * C1 + c] * (double)wrow[c];
                            for (int c = 0; c < C2; ++c) s += (double)X2[pix * C2 + c] * (double)wrow[C1 + c];
                        }
                    want[at] = s;
                }
    std::vector<half_t> C((size_t)M * Cout, (half_t)-7.f);
    vsx_gemm_desc d{};
    d.M = M; d.N = Cout; d.K = K; d.batch0 = d.batch1 = 1;
    d.A = X1.data(); d.A2 = C2 ? X2.data() : nullptr; d.a_mode = 1; d.H = H; d.W = W; d.C1 = C1; d.C2 = C2; d.ks = ks; d.stride = stride;
    d.upsample = ups;
    d.B = Wt.data(); d.ldb = K; d.C = C.data(); d.ldc = Cout;
    d.bias = bias.data(); d.rowvec = rowvec.data(); d.rows_per_vec = (long)Ho * Wo;
    if (both_addends) { d.residual = R.data(); d.ldr = Cout; }
    d.alpha = 1.0; d.pad_lo = d.pad_hi = -1;
    std::vector<float> ws;
    if (splitk) {
        const int64_t bytes = vsx_gemm_workspace(&d);
        if (bytes <= 0) { printf("%-58s no split-K plan FAIL\n", name); ++n_bad; }
        ws.resize((size_t)bytes / 4 + 4);
        d.workspace = ws.data(); d.workspace_bytes = bytes;
    }
    vsx_set_option("gemm_pp", pp);
    report(name, xcd_gm ? gemm_by_pieces(d, xcd_gm) : vsx_gemm_f16(&d, nullptr), want, C);
    return C;
}

// ---- case 26: the plan table ----
enum { PR_RES = 1, PR_ROWVEC = 2, PR_GEGLU = 4, PR_LN = 8, PR_VT = 16, PR_STATS = 32, PR_STATS_BAD = 64, PR_BIAS_ODD = 128 };
struct PlanRow {
    const char* name;
    long M, N, K;                                   // plain GEMM (M < 0: -M batches of 40 rows); a convolution derives M and K
    long nimg, H, W, C1, C2, ks, stride, ups;       // convolution (ks > 0)
    long flags;                                     // PR_*
    long pp, ws, ws_waves, tune;                    // options gemm_pp, gemm_ws, ws_waves, tile_tune
    // expected plan
    int family, BM, BN, WAVES_M, WAVES_N, deep, splits, nk_per;
    long stat_parts;
    long long workspace_bytes;
    int refused;
};

// The descriptor of a row.  No operand is ever touched (the plan is made from shapes, strides and alignments), so the pointers
// are made-up addresses with the alignment the row asks for.
static vsx_gemm_desc plan_desc(const PlanRow& r) {
    char* const mem = reinterpret_cast<char*>(0x10000000);
    vsx_gemm_desc d{};
    d.batch0 = d.batch1 = 1;
    d.N = r.N;
    d.A = mem; d.B = mem + 0x1000; d.C = mem + 0x2000;
    d.bias = mem + 0x3000 + ((r.flags & PR_BIAS_ODD) ? 2 : 0);
    d.alpha = 1.0; d.pad_lo = d.pad_hi = -1;
    d.geglu = (r.flags & PR_GEGLU) ? 1 : 0;
    long rows_per_vec = 32;
    if (r.ks > 0) {
        const long pad = r.ks / 2;
        const long Ho = (r.H + 2 * pad - r.ks) / r.stride + 1, Wo = (r.W + 2 * pad - r.ks) / r.stride + 1;
        d.M = r.nimg * Ho * Wo;
        d.K = r.ks * r.ks * (r.C1 + r.C2);
        d.a_mode = 1; d.H = r.H; d.W = r.W; d.C1 = r.C1; d.C2 = r.C2; d.ks = r.ks; d.stride = r.stride; d.upsample = r.ups;
        if (r.C2) d.A2 = mem + 0x4000;
        rows_per_vec = Ho * Wo;
    } else if (r.M < 0) {
        d.M = 40; d.K = r.K; d.batch0 = 2; d.batch1 = -r.M / 2;
        d.lda = d.K; d.a_bs1 = d.M * d.K; d.a_bs0 = d.batch1 * d.a_bs1;
        d.b_bs1 = d.N * d.K; d.b_bs0 = d.batch1 * d.b_bs1;
        d.c_bs1 = d.M * d.N; d.c_bs0 = d.batch1 * d.c_bs1;
    } else {
        d.M = r.M; d.K = r.K; d.lda = r.K;
    }
    d.ldb = d.K;
    d.ldc = d.N;
    if (r.flags & PR_VT) {
        const long rpi = d.K == 768 ? 77 : d.N == 320 ? 4096 : d.N == 640 ? 1024 : 256;     // text tokens, or the pixels of the UNet level
        d.c_mode = 1; d.c_rows_per_img = rpi; d.ldc = rpi; d.c_img_stride = d.N * rpi;
    }
    if (r.flags & PR_RES) { d.residual = mem + 0x5000; d.ldr = d.N; }
    if (r.flags & PR_ROWVEC) { d.rowvec = mem + 0x6000; d.rows_per_vec = rows_per_vec; }
    if (r.flags & PR_LN) { d.rowscale = mem + 0x7000; d.colvec = mem + 0x8000; }
    return d;
}

static void plan_options(const PlanRow& r) {
    vsx_set_option("gemm_pp", r.pp);
    vsx_set_option("gemm_ws", r.ws);
    vsx_set_option("ws_waves", r.ws_waves);
    vsx_set_option("tile_tune", r.tune);
}

// The plan of every row of gemm_plan_rows.inc (made from the launches of the revision before plan_gemm: see that file), and the two
// query functions against it.  Nothing is launched: "the launch" below is plan_gemm(..., assume_workspace = false), which is all
// vsx_gemm_f16 consults.
static void check_plans() {
    static const PlanRow rows[] = {
#include "gemm_plan_rows.inc"
    };
    int bad = 0, nsplit = 0;
    for (const PlanRow& r : rows) {
        plan_options(r);
        vsx_gemm_desc d = plan_desc(r);
        const int64_t parts = vsx_gemm_rowstats_parts(&d), bytes = vsx_gemm_workspace(&d);
        if (r.flags & (PR_STATS | PR_STATS_BAD)) { d.rowstats = (char*)d.A + 0x9000; d.rowstats_parts = parts + ((r.flags & PR_STATS_BAD) ? 1 : 0); }
        d.workspace = (char*)d.A + 0xA000;
        d.workspace_bytes = bytes;
        GemmParams p;
        const int rc = fill_params(&d, p);
        const GemmPlan plan = plan_gemm(d, p, false), asked = plan_gemm(d, p, true);
        bool ok = rc == VSX_OK && (int)plan.refused == r.refused && plan.stat_parts == r.stat_parts && parts == r.stat_parts &&
                  plan.workspace_bytes == r.workspace_bytes && asked.workspace_bytes == r.workspace_bytes && bytes == r.workspace_bytes &&
                  vsx_gemm_rowstats_parts(&d) == r.stat_parts && plan.splits == r.splits && plan.nk_per == r.nk_per;
        // what the host asks before it chooses a form: the launch's own status, refused exactly where the plan is
        const int status = vsx_gemm_check(&d);
        ok = ok && status == (r.refused ? VSX_E_UNSUPPORTED : VSX_OK);
        // the read-only query (vsx_gemm_plan) answers the same plan and the same status
        int64_t q[8];
        const int qrc = vsx_gemm_plan(&d, q);
        ok = ok && qrc == status && q[0] == (int)plan.family && q[4] == plan.splits && q[5] == (plan.splits > 1 ? plan.nk_per : 0) &&
             q[6] == plan.stat_parts && q[7] == (int)plan.refused;
        if (plan.family == GEMM_TILE) ok = ok && q[1] == plan.BM && q[2] == plan.BN && q[3] == (plan.deep ? 1 : 0);
        else ok = ok && q[1] == (plan.family == GEMM_PP256 ? 256 : plan.family == GEMM_PP128 ? 128 : 32) && q[2] == 320 && q[3] == 0;
        if (!r.refused) {
            ok = ok && (int)plan.family == r.family;
            if (r.family == GEMM_TILE)
                ok = ok && plan.BM == r.BM && plan.BN == r.BN && plan.WAVES_M == r.WAVES_M && plan.WAVES_N == r.WAVES_N && (int)plan.deep == r.deep;
        }
        if (r.splits > 1) {          // exactly the bytes asked for: split (above); one byte fewer, or no workspace at all: not split
            ++nsplit;
            d.workspace_bytes = bytes - 1;
            const GemmPlan shortp = plan_gemm(d, p, false);
            d.workspace = nullptr; d.workspace_bytes = bytes;
            const GemmPlan none = plan_gemm(d, p, false);
            ok = ok && shortp.splits == 1 && none.splits == 1 && shortp.family == GEMM_TILE && shortp.workspace_bytes == bytes;
        }
        if (!ok) {
            ++bad;
            printf("  plan of '%s': rc %d family %d tile %dx%d (%d x %d waves) deep %d splits %d x %d slabs, %ld parts (asked: %ld), %lld bytes (asked: %lld), refused %d, vsx_gemm_check %d  FAIL\n",
                   r.name, rc, (int)plan.family, plan.BM, plan.BN, plan.WAVES_M, plan.WAVES_N, (int)plan.deep, plan.splits, plan.nk_per,
                   plan.stat_parts, (long)parts, (long long)plan.workspace_bytes, (long long)bytes, (int)plan.refused, status);
        }
    }
    plan_options(PlanRow{"defaults", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 10, 0});
    const int n = (int)(sizeof(rows) / sizeof(rows[0]));
    printf("%-58s %d rows, %d split-K %s\n", "pinned plans (gemm_plan_rows.inc)", n, nsplit, bad == 0 && nsplit > 0 ? "ok" : "FAIL");
    n_bad += bad + (nsplit > 0 ? 0 : 1);
}

int main(int argc, char** argv) {
    // usage: check_gemm_api [case | -1 = all]; VSX_TUNE_TILE=1|2|3 in the environment forces the 128x320 / 128x160 / 256x320
    // tile kernel for the 320-column cases (the only way to reach them with problems this small)
    cpuhip_num_cus = 8;
    const int only = argc > 1 ? atoi(argv[1]) : -1;
    const Plain plain[] = {
        //  name                                              M    N    K   res  rowvec geglu ln    vT   rpv rpi pp splitK
        {"plain 200x320x128 +res (tile)",                    200, 320, 128, true, false, false, false, false, 0, 0, 0, false},
        {"plain 200x320x128 +rowvec +res (tile)",            200, 320, 128, true, true, false, false, false, 48, 0, 0, false},
        {"narrow 100x96x72 (64x64 tile, K tail, ragged N)",  100, 96, 72, true, false, false, false, false, 0, 0, 0, false},
        {"narrow 70x44x64 (scalar column edge)",             70, 44, 64, false, false, false, false, false, 0, 0, 0, false},
        {"geglu 150x160x64 (tile)",                          150, 160, 64, false, false, true, false, false, 0, 0, 0, false},
        {"geglu 90x48x64 (64x128 tile)",                     90, 48, 64, false, false, true, false, false, 0, 0, 0, false},
        {"V^T store 256x80x64, 128 rows per image",          256, 80, 64, false, false, false, false, true, 0, 128, 0, false},
        {"LayerNorm fold 200x320x128 (tile)",                200, 320, 128, false, false, false, true, false, 0, 0, 0, false},
        {"LayerNorm fold geglu 150x160x64 (tile)",           150, 160, 64, false, false, true, true, false, 0, 0, 0, false},
        {"LayerNorm fold V^T 256x80x64",                     256, 80, 64, false, false, false, true, true, 0, 128, 0, false},
        {"LayerNorm fold + PE row vector 192x320x64",        192, 320, 64, false, true, false, true, false, 32, 0, 0, false},
        {"split-K 128x320x1536 +res",                        128, 320, 1536, true, false, false, false, false, 0, 0, 0, true},
        {"split-K LayerNorm fold 100x320x1536",              100, 320, 1536, false, false, false, true, false, 0, 0, 0, true},
    };
    const int nplain = (int)(sizeof(plain) / sizeof(plain[0]));
    for (int i = 0; i < nplain; ++i)
        if (only < 0 || only == i) run_plain(plain[i]);
    if (only < 0 || only == nplain) {      // the persistent kernel through the entry point: bit for bit like the tile kernels
        Plain c = {"persistent 4096x320x64 +res vs tile kernels", 4096, 320, 64, true, false, false, false, false, 0, 0, 0, false};
        rng_state = 99u;
        const auto a = run_plain(c, false);
        c.pp = 2;
        rng_state = 99u;
        const auto b = run_plain(c, true);
        const bool same = memcmp(a.data(), b.data(), a.size() * sizeof(half_t)) == 0;
        printf("%-58s %s\n", "  ... bit-identical to gemm_pp = 0", same ? "ok" : "FAIL");
        n_bad += same ? 0 : 1;
    }
    if (only < 0 || only == nplain + 1) run_batched("batched 2x3 x (40x56x40) scores", 2, 3, 40, 56, 40);
    if (only < 0 || only == nplain + 2) run_conv("conv3x3 2x8x8 64+64->320 +rowvec +res", 2, 8, 8, 64, 64, 320, 3, 1, 0, false);
    if (only < 0 || only == nplain + 3) run_conv("conv3x3 1x12x8 72->96 /s2 (narrow tiles)", 1, 12, 8, 72, 0, 96, 3, 2, 0, false);
    if (only < 0 || only == nplain + 4) run_conv("conv1x1 2x8x8 128->320 nearest-2x", 2, 8, 8, 128, 0, 320, 1, 1, 1, false);
    if (only < 0 || only == nplain + 5) run_conv("conv3x3 split-K 1x8x8 192->320", 1, 8, 8, 192, 0, 320, 3, 1, 0, true);
    if (only < 0 || only == nplain + 7) run_subpixel("sub-pixel nearest-2x conv 4x(16x16 -> 32x32) 64->320", 4, 16, 16, 64, 320);
    if (only < 0 || only == nplain + 6) {      // the persistent convolution through the entry point: bit for bit like the tile kernels
        rng_state = 7u;
        const auto a = run_conv("conv3x3 4x32x32 64->320 +rowvec, tile kernels", 4, 32, 32, 64, 0, 320, 3, 1, 0, false, 0, false);
        rng_state = 7u;
        const auto b = run_conv("conv3x3 4x32x32 64->320 +rowvec, persistent kernel", 4, 32, 32, 64, 0, 320, 3, 1, 0, false, 2, false);
        const bool same = memcmp(a.data(), b.data(), a.size() * sizeof(half_t)) == 0;
        printf("%-58s %s\n", "  ... bit-identical (default K order)", same ? "ok" : "FAIL");
        n_bad += same ? 0 : 1;
    }
    if (only < 0 || only == nplain + 8) {
        // XCD BLOCK GRID of the tile kernels (gemm.hip): forced tiles / K slices so that problems this small have enough work
        // items; every case under the linear walk (xcd_walk 0) and under the block grid must agree bit for bit (the walk only
        // decides WHICH workgroup computes a tile), the block grid must actually have been chosen, and both match the
        // double-precision result (run_plain / run_conv report that)
        struct G { const char* name; long M, N, K; long tune; bool splitk; int want_gm; };
        const G cases[] = {{"XCD grid 4x2: 128x160 tiles, 8 x 4 tiles (1024x640x128)", 1024, 640, 128, 2, false, 4},
                           {"XCD grid 2x4: 128x320 tiles x 2 K slices (512x640x256)", 512, 640, 256, (2 << 8), true, 2},
                           {"XCD grid 1x8: 128x320 tiles x 4 K slices (256x640x512)", 256, 640, 512, (4 << 8), true, 1},
                           {"XCD grid 1x8: 128x320 tile x 8 K slices (128x640x1024)", 128, 640, 1024, (8 << 8), true, 1}};
        const bool quick = getenv("CPUHIP_QUICK") != nullptr;       // the CPU test suite: the first two grids and the convolution
        int idx = 0;
        for (const G& g : cases) {
            if (quick && idx++ >= 2) break;
            Plain c = {g.name, g.M, g.N, g.K, true, false, false, false, false, 0, 0, 0, g.splitk};
            vsx_set_option("tile_tune", g.tune);
            vsx_set_option("xcd_walk", 0);
            rng_state = 1234u;
            int gm0 = -1, gm1 = -1;
            const auto a = run_plain(c, false, &gm0);
            vsx_set_option("xcd_walk", 1);
            rng_state = 1234u;
            const auto b = run_plain(c, true, &gm1);
            const bool same = memcmp(a.data(), b.data(), a.size() * sizeof(half_t)) == 0;
            printf("%-58s %s (gm %d -> %d)\n", "  ... bit-identical to the linear walk, grid chosen", same && gm0 == 0 && gm1 == g.want_gm ? "ok" : "FAIL", gm0, gm1);
            n_bad += same && gm0 == 0 && gm1 == g.want_gm ? 0 : 1;
        }
        if (!quick) {
        vsx_set_option("tile_tune", (2 << 8));
        vsx_set_option("xcd_walk", 0);
        rng_state = 77u;
        const auto a = run_conv("conv3x3 8x8x8 192->640, 128x320 tiles x 2 K slices, linear walk", 8, 8, 8, 192, 0, 640, 3, 1, 0, true, 0, true);
        vsx_set_option("xcd_walk", 1);
        rng_state = 77u;
        int gm = -1;
        const auto b = run_conv("conv3x3 8x8x8 192->640, 128x320 tiles x 2 K slices, XCD block grid", 8, 8, 8, 192, 0, 640, 3, 1, 0, true, 0, true, &gm);
        const bool same = memcmp(a.data(), b.data(), a.size() * sizeof(half_t)) == 0;
        printf("%-58s %s (gm %d)\n", "  ... bit-identical, grid chosen", same && gm > 0 ? "ok" : "FAIL", gm);
        n_bad += same && gm > 0 ? 0 : 1;
        }
        vsx_set_option("tile_tune", 0);
        vsx_set_option("xcd_walk", 1);
    }
    if (only < 0 || only == nplain + 14) {
        // forced split counts that would leave the last K slice without a slab (5 slabs in 4 slices of ceil = 2: 2 + 2 + 1 + 0; the
        // automatic planner never asks for one): plan_splitk takes slices away until every slice has one.  An empty slice's
        // workgroups multiplied whatever the LDS ring held.
        struct E { const char* name; long K, tune; int splits; };
        const E cases[] = {{"split-K 100x320x320, 4 slices forced over 5 slabs -> 3", 320, (4 << 8), 3},
                           {"split-K 100x320x256, 3 slices forced over 4 slabs -> 2", 256, (3 << 8), 2}};
        for (const E& e : cases) {
            Plain c = {e.name, 100, 320, e.K, true, false, false, false, false, 0, 0, 0, true};
            vsx_set_option("tile_tune", e.tune);
            rng_state = 31u;
            run_plain(c, true);
            vsx_gemm_desc d{};
            d.M = c.M; d.N = c.N; d.K = c.K; d.batch0 = d.batch1 = 1; d.lda = d.ldb = c.K; d.ldc = c.N; d.alpha = 1.0; d.pad_lo = d.pad_hi = -1;
            d.A = d.B = d.C = d.workspace = reinterpret_cast<void*>(0x10000000);
            d.workspace_bytes = vsx_gemm_workspace(&d);
            int64_t q[8];
            const bool ok = vsx_gemm_plan(&d, q) == VSX_OK && q[4] == e.splits && (q[4] - 1) * q[5] < (c.K + 63) / 64;
            printf("%-58s %s (%ld slices of %ld slabs)\n", "  ... no slice without a slab", ok ? "ok" : "FAIL", (long)q[4], (long)q[5]);
            n_bad += ok ? 0 : 1;
        }
        vsx_set_option("tile_tune", 0);
    }
    if (only < 0 || only == nplain + 9) {
        // residual prefetch of the tile kernels BEHIND the last slab (gemm.hip, RES_LATE): ten slabs, every forced tile / ring
        // depth; pp_sched bit 64 (issue in iteration 0, no exact count) must agree bit for bit.  Run it under CPUHIP_DMA=late as
        // well: the counted waits then decide what has landed when a slab is multiplied.
        struct T { const char* name; long tune; long M, N; };
        const T tiles[] = {{"128x160 ring 2", 2, 200, 320}, {"128x160 ring 4", 2 + 16, 200, 320}, {"128x320", 1, 200, 640},
                           {"128x128", 4, 200, 256}, {"64x128", 5, 100, 256}, {"64x64", 6, 100, 128}};
        const bool quick = getenv("CPUHIP_QUICK") != nullptr;       // the CPU test suite: both ring depths of the 128x160 tile and the 64x64 tile
        for (const T& t : tiles) {
            if (quick && t.tune != 2 && t.tune != 2 + 16 && t.tune != 6) continue;
            char name[128];
            snprintf(name, sizeof name, "late residual prefetch, %s tile: %ldx%ldx640 +res", t.name, t.M, t.N);
            Plain c = {name, t.M, t.N, 640, true, false, false, false, false, 0, 0, 0, false};
            vsx_set_option("tile_tune", t.tune);
            vsx_set_option("pp_sched", 0);
            rng_state = 4321u;
            const auto a = run_plain(c, true);
            vsx_set_option("pp_sched", 64);
            rng_state = 4321u;
            const auto b = run_plain(c, false);
            const bool same = memcmp(a.data(), b.data(), a.size() * sizeof(half_t)) == 0;
            printf("%-58s %s\n", "  ... bit-identical to the early placement", same ? "ok" : "FAIL");
            n_bad += same ? 0 : 1;
        }
        vsx_set_option("tile_tune", 0);
        vsx_set_option("pp_sched", 0);
    }
    if (only < 0 || only == nplain + 10) {
        // the persistent kernel's transposed store (gemm_pp.hip, epilogue_vt) through the entry point: bit for bit like the tile
        // kernels' V^T store, plain and with the LayerNorm identity (gemm_pp = 4: 256-row tiles however few)
        for (int ln = 0; ln < 2; ++ln) {
            Plain c = {ln ? "V^T store 512x320x128 + LayerNorm fold, persistent vs tile kernels" : "V^T store 512x320x128, persistent vs tile kernels",
                       512, 320, 128, false, false, false, ln != 0, true, 0, 256, 0, false};
            rng_state = 555u;
            const auto a = run_plain(c, false);
            c.pp = 4;
            rng_state = 555u;
            const auto b = run_plain(c, true);
            const bool same = memcmp(a.data(), b.data(), a.size() * sizeof(half_t)) == 0;
            printf("%-58s %s\n", "  ... bit-identical to gemm_pp = 0", same ? "ok" : "FAIL");
            n_bad += same ? 0 : 1;
        }
        vsx_set_option("gemm_pp", 1);
    }
    if (only < 0 || only == nplain + 11) {
        // the weight-stationary kernel for K = N = 320 (gemm_pp.hip, gemm_ws320_kernel; option gemm_ws = 2: every eligible problem): 21
        // blocks of 32 rows over 8 workgroups (3 / 2 blocks each, so the out-of-range tail pieces are issued), bit for bit like the tile
        // kernels, with and without residual; with row statistics: 5 parts per row that add up to the sums of the rounded outputs
        for (int res = 0; res < 2; ++res)
            for (int st = 0; st < 2; ++st) {
                if (getenv("CPUHIP_QUICK") && res != st) continue;      // the CPU suite: bias only, and residual + statistics
                char name[96];
                snprintf(name, sizeof name, "weight-stationary 672x320x320%s%s vs tile kernels", res ? " +res" : "", st ? " +stats" : "");
                const long M = 672, N = 320, K = 320;
                rng_state = 4242u + res;
                auto A = randh((size_t)M * K), B = randh((size_t)N * K, 1.0f / sqrtf((float)K)), bias = randh(N), R = randh((size_t)M * N);
                std::vector<half_t> C0((size_t)M * N, (half_t)-7.f), C1((size_t)M * N, (half_t)-7.f);
                const long NP = (getenv("VSX_WS_WAVES") && atoi(getenv("VSX_WS_WAVES")) == 5) ? 5 : 10;       // statistic parts per row = waves per workgroup
                std::vector<float> stats((size_t)M * NP * 2, -1.f);
                vsx_gemm_desc d{};
                d.M = M; d.N = N; d.K = K; d.batch0 = d.batch1 = 1;
                d.A = A.data(); d.lda = K; d.B = B.data(); d.ldb = K; d.ldc = N; d.bias = bias.data();
                if (res) { d.residual = R.data(); d.ldr = N; }
                d.alpha = 1.0; d.pad_lo = d.pad_hi = -1;
                d.C = C0.data();
                vsx_set_option("gemm_pp", 0);
                vsx_set_option("gemm_ws", 0);
                const int rc0 = vsx_gemm_f16(&d, nullptr);
                d.C = C1.data();
                vsx_set_option("gemm_pp", 1);
                vsx_set_option("gemm_ws", 2);
                if (st) {
                    const long parts = vsx_gemm_rowstats_parts(&d);
                    if (parts != NP) { printf("%-58s rowstats parts %ld (want %ld) FAIL\n", name, parts, NP); ++n_bad; }
                    d.rowstats = stats.data(); d.rowstats_parts = NP;
                }
                const int rc1 = vsx_gemm_f16(&d, nullptr);
                vsx_set_option("gemm_ws", 0);
                bool same = rc0 == 0 && rc1 == 0 && memcmp(C0.data(), C1.data(), C0.size() * sizeof(half_t)) == 0;
                double worst = 0;
                if (st)
                    for (long m = 0; m < M; ++m) {
                        double s1 = 0, s2 = 0, w1 = 0, w2 = 0;
                        for (int part = 0; part < NP; ++part) { s1 += stats[(m * NP + part) * 2]; s2 += stats[(m * NP + part) * 2 + 1]; }
                        for (long n = 0; n < N; ++n) { const double v = (double)C1[m * N + n]; w1 += v; w2 += v * v; }
                        worst = fmax(worst, fmax(fabs(s1 - w1) / (1.0 + fabs(w1)), fabs(s2 - w2) / (1.0 + fabs(w2))));
                    }
                if (!same && getenv("CPUHIP_VERBOSE")) {
                    long bad = 0, first = -1;
                    for (long i = 0; i < M * N; ++i) if (memcmp(&C0[i], &C1[i], 2)) { if (first < 0) first = i; ++bad; }
                    printf("    %ld of %ld elements differ, first at row %ld col %ld: %f vs %f\n", bad, M * N, first / N, first % N, (double)C0[first], (double)C1[first]);
                    long colbad[5] = {0, 0, 0, 0, 0};
                    for (long i = 0; i < M * N; ++i) if (memcmp(&C0[i], &C1[i], 2)) ++colbad[(i % N) / 64];
                    printf("    per 64-column block: %ld %ld %ld %ld %ld\n", colbad[0], colbad[1], colbad[2], colbad[3], colbad[4]);
                }
                if (worst > 1e-4) same = false;
                printf("%-58s rc %d %d  %s%s\n", name, rc0, rc1, same ? "bit-identical" : "FAIL", st ? (worst <= 1e-4 ? ", statistics ok" : ", statistics off") : "");
                n_bad += same ? 0 : 1;
            }
        vsx_set_option("gemm_pp", 1);
    }
    if (only < 0 || only == nplain + 12) {
        // the same kernel over column slices (N = 640 / 960, K = 320) with the folded LayerNorm, the positional row vector (48 rows per
        // vector: blocks that meet two vectors) and a residual: bit for bit like the tile kernels
        const Plain cases[] = {
            {"weight-stationary 672x960x320 LayerNorm fold + row vector", 672, 960, 320, false, true, false, true, false, 48, 0, 0, false},
            {"weight-stationary 672x640x320 LayerNorm fold",               672, 640, 320, false, false, false, true, false, 0, 0, 0, false},
            {"weight-stationary 672x640x320 +res",                         672, 640, 320, true, false, false, false, false, 0, 0, 0, false},
            {"weight-stationary 672x320x320 LayerNorm fold + row vector",  672, 320, 320, false, true, false, true, false, 32, 0, 0, false},
        };
        for (const Plain& c0 : cases) {
            if (getenv("CPUHIP_QUICK") && (&c0 - cases) >= 2) continue;
            Plain c = c0;
            rng_state = 777u;
            vsx_set_option("gemm_ws", 0);
            c.pp = 0;
            const auto a = run_plain(c, false);
            rng_state = 777u;
            vsx_set_option("gemm_ws", 2);
            c.pp = 1;
            const auto b = run_plain(c, true);
            vsx_set_option("gemm_ws", 0);
            const bool same = memcmp(a.data(), b.data(), a.size() * sizeof(half_t)) == 0;
            printf("%-58s %s\n", "  ... bit-identical to the tile kernels", same ? "ok" : "FAIL");
            n_bad += same ? 0 : 1;
        }
        vsx_set_option("gemm_pp", 1);
    }
    if (only < 0 || only == nplain + 13) check_plans();      // which kernel every UNet shape, threshold and option value gets
    printf(n_bad ? "%d check(s) FAILED\n" : "all checks passed\n", n_bad);
    return n_bad ? 1 : 0;
}
