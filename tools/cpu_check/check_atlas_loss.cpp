// Runs videoswap_amd/csrc/atlas_loss.hip (K18: the batch gather and the fused losses of an atlas training step) on the CPU
// from its real source, under AddressSanitizer and UBSan.  Every buffer has exactly the size the entry point is told, so a
// read or write past a data array, a row block or a gradient tensor is a sanitizer report.
//   K18a against integer / double loops: N = 0 / 1 / 63 / 64 / 65 / 255 / 256 / 257 / 513, with and without the blocks 5 and
//     6, the first rows at the four image corners on frame 0 and on frame T - 1 (offsets that leave the image), and an index
//     outside the video, which must read nothing.
//   K18b: the 14 losses against double-precision loops, and every entry of the four gradient tensors against central
//     differences of the double-precision total: the same N, with and without the blocks 5 and 6, with and without the alpha
//     loss, no / one / all rows relevant.
//   The refusals.
//   make -C tools/cpu_check check_atlas_loss && tools/cpu_check/check_atlas_loss
#include <stdio.h>
#include <stdlib.h>

#include <vector>

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

// what K18 uses beyond hip/hip_runtime.h: the clearing of the two counts and an integer atomic add
static inline hipError_t hipMemsetAsync(void* p, int value, size_t bytes, hipStream_t) {
    memset(p, value, bytes);
    return hipSuccess;
}
static inline unsigned atomicAdd(unsigned* address, unsigned value) {
    return std::atomic_ref<unsigned>(*address).fetch_add(value, std::memory_order_relaxed);
}

#include "atlas_loss.hip"

static unsigned rng_state = 4242u;
static float frand() {                      // uniform in [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((rng_state >> 8) & 0xFFFF) / 65536.0f;
}
static float srand1() { return frand() * 2.f - 1.f; }

// exactly `n` elements: the sanitizer's red zone starts right behind the last one
template <typename T>
struct Buf {
    T* p = nullptr;
    size_t n = 0;
    explicit Buf(size_t n_) : n(n_) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, (n ? n : 1) * sizeof(T))) abort();
        p = (T*)q;
        for (size_t i = 0; i < n; ++i) p[i] = T(0);
    }
    Buf(const Buf&) = delete;
    ~Buf() { free(p); }
    T& operator[](size_t i) { return p[i]; }
};

static int n_bad = 0;
static void verdict(const char* name, bool ok, double err) {
    printf("%-72s max err %.2e  %s\n", name, err, ok ? "ok" : "FAIL");
    if (!ok) ++n_bad;
}

// ---------------------------------------------------------------------------------------------------------------------
// K18a
// ---------------------------------------------------------------------------------------------------------------------
struct Video {
    long H, W, T;
    Buf<float> video, dx, dy, mask, flow, flow_rev, fmask, rmask;
    Video(long H_, long W_, long T_)
        : H(H_), W(W_), T(T_), video(H_ * W_ * 3 * T_), dx(H_ * W_ * 3 * T_), dy(H_ * W_ * 3 * T_), mask(H_ * W_ * T_), flow(H_ * W_ * 2 * T_),
          flow_rev(H_ * W_ * 2 * T_), fmask(H_ * W_ * T_), rmask(H_ * W_ * T_) {
        for (size_t i = 0; i < video.n; ++i) video[i] = frand(), dx[i] = srand1() * 0.1f, dy[i] = srand1() * 0.1f;
        for (size_t i = 0; i < mask.n; ++i) mask[i] = frand() < 0.5f ? 1.f : frand(), fmask[i] = frand() < 0.6f ? 1.f : 0.f, rmask[i] = frand() < 0.6f ? 1.f : 0.f;
        for (size_t i = 0; i < flow.n; ++i) flow[i] = srand1() * 2.5f, flow_rev[i] = srand1() * 2.5f;
    }
};

static void run_batch(Video& v, long N, int with_global, bool hostile) {
    const long d = 1, D = 100, B = with_global ? 9 : 7, total = v.T * v.H * v.W;
    Buf<int64_t> idx(N);
    Buf<float> rows(B * N * 3), rgb(3 * N), rgb_dx(3 * N), rgb_dy(3 * N), gt(N), mf(N), mb(N);
    Buf<int32_t> counts(2);
    counts[0] = counts[1] = 77;
    const long corner[8][3] = {{0, 0, 0}, {0, 0, v.W - 1}, {0, v.H - 1, 0}, {0, v.H - 1, v.W - 1},
                               {v.T - 1, 0, 0}, {v.T - 1, 0, v.W - 1}, {v.T - 1, v.H - 1, 0}, {v.T - 1, v.H - 1, v.W - 1}};
    for (long r = 0; r < N; ++r) {
        idx[r] = (int64_t)(frand() * (float)total) % total;
        if (r < 8) idx[r] = (corner[r][0] * v.H + corner[r][1]) * v.W + corner[r][2];
    }
    if (hostile && N > 9) idx[8] = total, idx[9] = -1;                // outside the video: nothing may be read for these rows
    const int rc = vsx_atlas_batch_f32(idx.p, N, v.H, v.W, v.T, 1, v.video.p, v.dx.p, v.dy.p, v.mask.p, v.flow.p, v.flow_rev.p, v.fmask.p,
                                       v.rmask.p, d, D, with_global, rows.p, rgb.p, rgb_dx.p, rgb_dy.p, gt.p, mf.p, mb.p, counts.p, nullptr);
    bool ok = rc == VSX_OK;
    double err = 0;
    long cf = 0, cb = 0;
    const double hd = (double)(float)((double)(v.H > v.W ? v.H : v.W) / 2.0), ht = (double)(float)((double)v.T / 2.0);
    for (long r = 0; r < N && ok; ++r) {
        const long k = idx[r];
        if (k < 0 || k >= total) {
            for (long b = 0; b < B; ++b)
                for (int c = 0; c < 3; ++c) ok = ok && rows[(b * N + r) * 3 + c] != rows[(b * N + r) * 3 + c];
            ok = ok && rgb[3 * r] != rgb[3 * r] && gt[r] != gt[r] && mf[r] == 0.f && mb[r] == 0.f;
            continue;
        }
        const long f = k / (v.H * v.W), i = k % (v.H * v.W) / v.W, j = k % v.W, pix = i * v.W + j;
        const double fx = v.flow[(pix * 2) * v.T + f], fy = v.flow[(pix * 2 + 1) * v.T + f];
        const double rx = v.flow_rev[(pix * 2) * v.T + f], ry = v.flow_rev[(pix * 2 + 1) * v.T + f];
        double want[9][3] = {{(double)j, (double)i, (double)f}, {(double)j + 1, (double)i, (double)f}, {(double)j, (double)i + 1, (double)f},
                             {(double)j, (double)(i - d), (double)f}, {(double)(j - d), (double)i, (double)f},
                             {(double)j, (double)(i - D), (double)f}, {(double)(j - D), (double)i, (double)f},
                             {(double)(float)((float)j + (float)fx), (double)(float)((float)i + (float)fy), (double)f + 1},
                             {(double)(float)((float)j + (float)rx), (double)(float)((float)i + (float)ry), (double)f - 1}};
        for (long b = 0; b < B; ++b) {
            const long src = (!with_global && b >= 5) ? b + 2 : b;
            for (int c = 0; c < 3; ++c) {
                const double w = want[src][c] / (c < 2 ? hd : ht) - 1.0;
                const double e = fabs((double)rows[(b * N + r) * 3 + c] - w);
                err = fmax(err, e);
                ok = ok && e <= 1.2e-7 * fmax(1.0, fabs(w) + 1.0);            // two roundings of values below 8
            }
        }
        for (int c = 0; c < 3; ++c)
            ok = ok && rgb[3 * r + c] == v.video[(pix * 3 + c) * v.T + f] && rgb_dx[3 * r + c] == v.dx[(pix * 3 + c) * v.T + f] &&
                 rgb_dy[3 * r + c] == v.dy[(pix * 3 + c) * v.T + f];
        ok = ok && gt[r] == v.mask[pix * v.T + f] && mf[r] == v.fmask[pix * v.T + f] && mb[r] == v.rmask[pix * v.T + f];
        cf += mf[r] != 0.f, cb += mb[r] != 0.f;
    }
    ok = ok && counts[0] == cf && counts[1] == cb;
    char name[160];
    snprintf(name, sizeof(name), "atlas_batch %ldx%ldx%ld N=%ld %s%s", v.W, v.H, v.T, N, with_global ? "9 blocks" : "7 blocks", hostile ? " hostile idx" : "");
    verdict(name, ok, err);
}

// ---------------------------------------------------------------------------------------------------------------------
// K18b
// ---------------------------------------------------------------------------------------------------------------------
struct Row {                                 // one row's network outputs and data, in double
    double uv[2][9][2], a[5], c[6][3], rgb[3], dx[3], dy[3], gt, mf, mb;
};
constexpr int ROW_INPUTS = 2 * 9 * 2 + 5 + 18;

static double rigidity(const double (*uv)[2], int ba, int bb, double larger, double scale, double d) {
    const double k = larger / 2.0 / scale / d;
    const double du_dx = (uv[0][0] - uv[bb][0]) * k, du_dy = (uv[0][0] - uv[ba][0]) * k;
    const double dv_dx = (uv[0][1] - uv[bb][1]) * k, dv_dy = (uv[0][1] - uv[ba][1]) * k;
    const double p = du_dx * du_dx + dv_dx * dv_dx, q = du_dx * du_dy + dv_dx * dv_dy, r = du_dy * du_dy + dv_dy * dv_dy;
    const double a = p + 0.001, e = r + 0.001, det = a * e - q * q;
    return sqrt(p * p + 2 * q * q + r * r) + sqrt(e * e + 2 * q * q + a * a) / det;
}

// the 18 per-row sums of the kernel (AL_TERMS), B = 9 layout (blocks 5 and 6 unused without the global rigidity)
static void row_terms(const Row& r, const vsx_atlas_loss_cfg& cfg, double* t) {
    for (int k = 0; k < AL_TERMS; ++k) t[k] = 0;
    double a[5], out[3][3];
    for (int k = 0; k < 5; ++k) a[k] = 0.5 * (r.a[k] + 1.0) * 0.99 + 0.001;
    double cf[3][3], cb[3][3];
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) {
            cf[k][c] = (r.c[k][c] + 1.0) * 0.5, cb[k][c] = (r.c[3 + k][c] + 1.0) * 0.5;
            out[k][c] = cf[k][c] * a[k] + cb[k][c] * (1.0 - a[k]);
        }
    for (int c = 0; c < 3; ++c) {
        const double ex = r.dx[c] - (out[1][c] - out[0][c]), ey = r.dy[c] - (out[2][c] - out[0][c]);
        t[0] += ex * ex + ey * ey;
        t[1] += (out[0][c] - r.rgb[c]) * (out[0][c] - r.rgb[c]);
        t[3] += cf[0][c] * (1.0 - a[0]) * cf[0][c] * (1.0 - a[0]);
    }
    if (cfg.with_alpha_loss) t[2] = -r.gt * log(a[0]) - (1.0 - r.gt) * log(1.0 - a[0]);
    const double larger = (double)cfg.larger_dim, scale = (double)(float)cfg.uv_mapping_scale;
    for (int l = 0; l < 2; ++l) {
        t[4 + l] = rigidity(r.uv[l], 3, 4, larger, scale, (double)cfg.derivative_amount);
        if (cfg.with_global_rigidity) t[6 + l] = rigidity(r.uv[l], 5, 6, larger, scale, (double)cfg.global_derivative_amount);
        const double w = l == 0 ? a[0] : 1.0 - a[0];
        for (int dir = 0; dir < 2; ++dir) {
            if ((dir == 0 ? r.mf : r.mb) == 0.0) continue;
            const double eu = r.uv[l][7 + dir][0] - r.uv[l][0][0], ev = r.uv[l][7 + dir][1] - r.uv[l][0][1];
            t[8 + 2 * l + dir] = sqrt(eu * eu + ev * ev) * larger / (2.0 * scale) * w;
        }
    }
    if (r.mf != 0.0) t[12] = fabs(a[0] - a[3]);
    if (r.mb != 0.0) t[13] = fabs(a[4] - a[0]);
    if (a[0] > 0.5) t[14] = a[0], t[15] = 1;
    if (a[0] < 0.5) t[16] = a[0], t[17] = 1;
}

static void losses_of(const double* s, const vsx_atlas_loss_cfg& c, double N, double nf, double nb, double* L) {
    for (int k = 0; k < 8; ++k) L[k] = s[k] / N;
    if (!c.with_alpha_loss) L[2] = 0;
    if (!c.with_global_rigidity) L[6] = L[7] = 0;
    auto mean = [](double x, double n) { return n > 0 ? x / n : 0.0; };
    L[8] = 0.5 * mean(s[9], nb) + 0.5 * mean(s[8], nf);
    L[9] = 0.5 * mean(s[11], nb) + 0.5 * mean(s[10], nf);
    L[10] = 0.5 * (mean(s[12], nf) + mean(s[13], nb));
    L[11] = c.gradient_loss_weight * L[0] + c.rgb_loss_weight * L[1] + c.alpha_loss_weight * L[2] + c.sparsity_loss_weight * L[3] +
            c.rigidity_loss_weight * (L[4] + L[5]) + c.global_rigidity_fg_loss_weight * L[6] + c.global_rigidity_bg_loss_weight * L[7] +
            c.flow_loss_weight * (L[8] + L[9]) + c.alpha_flow_loss_weight * L[10];
    L[12] = s[14] / s[15];
    L[13] = s[16] / s[17];
}

// a row's share of total_loss (the counts are fixed: they do not depend on the network outputs)
static double row_total(const Row& r, const vsx_atlas_loss_cfg& c, double N, double nf, double nb) {
    double t[AL_TERMS], L[14];
    row_terms(r, c, t);
    losses_of(t, c, N, nf, nb, L);
    return L[11];
}

static double* row_input(Row& r, int k) {     // the k-th network output of a row
    if (k < 36) return &r.uv[k / 18][k % 18 / 2][k % 2];
    if (k < 41) return &r.a[k - 36];
    return &r.c[(k - 41) / 3][(k - 41) % 3];
}

// masks: 0 random, 1 none relevant, 2 one row, 3 all
static void run_losses(long N, int with_global, int with_alpha, int masks) {
    const long B = with_global ? 9 : 7;
    vsx_atlas_loss_cfg cfg{1000.0, 5000.0, 2000.0, 1000.0, 1.0, 5.0, 50.0, 5.0, 49.0, 0.8, 48, 1, 3, with_alpha, with_global};
    const float pixel = 2.f * 0.8f / 48.f;
    Buf<float> uv[2] = {Buf<float>(B * N * 2), Buf<float>(B * N * 2)}, araw(5 * N), atlas(6 * N * 3);
    Buf<float> rgb(3 * N), dx(3 * N), dy(3 * N), gt(N), mf(N), mb(N), losses(14), scratch((size_t)vsx_atlas_losses_workspace(N));
    Buf<float> g_uv[2] = {Buf<float>(B * N * 2), Buf<float>(B * N * 2)}, g_a(5 * N), g_c(6 * N * 3);
    Buf<int32_t> counts(2);
    auto pos = [&](int b) { return (!with_global && b >= 7) ? b - 2 : b; };
    for (long i = 0; i < N; ++i) {
        for (int l = 0; l < 2; ++l) {
            const float u = srand1(), v = srand1();
            auto put = [&](int b, float x, float y) { uv[l][2 * (pos(b) * N + i)] = x, uv[l][2 * (pos(b) * N + i) + 1] = y; };
            put(0, u, v), put(1, u + pixel * srand1(), v + pixel * srand1()), put(2, u + pixel * srand1(), v + pixel * srand1());
            for (int g = 0; g < (with_global ? 2 : 1); ++g) {              // Jacobians identity + 0.2 uniform: a determinant of at least 0.6
                const float amount = g ? 3.f : 1.f;
                const float j00 = 1.f + 0.2f * srand1(), j01 = 0.2f * srand1(), j10 = 0.2f * srand1(), j11 = 1.f + 0.2f * srand1();
                put(3 + 2 * g, u - pixel * amount * j01, v - pixel * amount * j11);
                put(4 + 2 * g, u - pixel * amount * j00, v - pixel * amount * j10);
            }
            put(7, u + pixel * (0.3f + frand()), v + pixel * srand1()), put(8, u + pixel * srand1(), v - pixel * (0.3f + frand()));
        }
        for (int k = 0; k < 5; ++k) araw[k * N + i] = srand1() * 0.999f;
        for (int k = 0; k < 6; ++k)
            for (int c = 0; c < 3; ++c) atlas[(k * N + i) * 3 + c] = srand1();
        for (int c = 0; c < 3; ++c) rgb[3 * i + c] = frand(), dx[3 * i + c] = 0.1f * srand1(), dy[3 * i + c] = 0.1f * srand1();
        gt[i] = frand() < 0.5f ? 1.f : frand();
        mf[i] = masks == 3 || (masks == 0 && frand() < 0.6f) || (masks == 2 && i == N / 2) ? 1.f : 0.f;
        mb[i] = masks == 3 || (masks == 0 && frand() < 0.6f) || (masks == 2 && i == N / 2) ? 1.f : 0.f;
        counts[0] += mf[i] != 0.f, counts[1] += mb[i] != 0.f;
    }
    for (size_t k = 0; k < g_a.n; ++k) g_a[k] = 9e9f;                       // every entry must be written
    for (int l = 0; l < 2; ++l)
        for (size_t k = 0; k < g_uv[l].n; ++k) g_uv[l][k] = 9e9f;
    for (size_t k = 0; k < g_c.n; ++k) g_c[k] = 9e9f;
    const int rc = vsx_atlas_losses_f32(uv[0].p, uv[1].p, araw.p, atlas.p, N, rgb.p, dx.p, dy.p, gt.p, mf.p, mb.p, counts.p, &cfg, losses.p,
                                        g_uv[0].p, g_uv[1].p, g_a.p, g_c.p, scratch.p, (int64_t)scratch.n, nullptr);
    bool ok = rc == VSX_OK;
    // the reference: double loops over the rows
    std::vector<Row> rows(N);
    double sums[AL_TERMS] = {0}, t[AL_TERMS], L[14];
    for (long i = 0; i < N; ++i) {
        Row& r = rows[i];
        memset(&r, 0, sizeof(r));
        for (int l = 0; l < 2; ++l)
            for (int b = 0; b < 9; ++b) {
                if (!with_global && (b == 5 || b == 6)) continue;
                r.uv[l][b][0] = uv[l][2 * (pos(b) * N + i)], r.uv[l][b][1] = uv[l][2 * (pos(b) * N + i) + 1];
            }
        for (int k = 0; k < 5; ++k) r.a[k] = araw[k * N + i];
        for (int k = 0; k < 6; ++k)
            for (int c = 0; c < 3; ++c) r.c[k][c] = atlas[(k * N + i) * 3 + c];
        for (int c = 0; c < 3; ++c) r.rgb[c] = rgb[3 * i + c], r.dx[c] = dx[3 * i + c], r.dy[c] = dy[3 * i + c];
        r.gt = gt[i], r.mf = mf[i], r.mb = mb[i];
        row_terms(r, cfg, t);
        for (int k = 0; k < AL_TERMS; ++k) sums[k] += t[k];
    }
    const double nf = counts[0], nb = counts[1];
    losses_of(sums, cfg, (double)N, nf, nb, L);
    double err = 0;
    for (int k = 0; k < 14; ++k) {
        const double got = losses[k];
        if (L[k] != L[k]) {                                                  // a mean over an empty set: NaN on both sides
            ok = ok && got != got;
            continue;
        }
        const double e = fabs(got - L[k]) / fmax(fabs(L[k]), 1e-30);
        if (L[k] != 0) err = fmax(err, e);
        ok = ok && (L[k] == 0 ? got == 0 : e <= 2e-5);                       // fp32 sums of up to 513 non-negative terms against double
    }
    // the gradients: central differences of the double total, one row at a time (a row's outputs enter its own terms only)
    double gmax[4] = {0, 0, 0, 0}, emax[4] = {0, 0, 0, 0};
    for (long i = 0; i < N; ++i)
        for (int k = 0; k < ROW_INPUTS; ++k) {
            const int b = k % 18 / 2;
            if (k < 36 && !with_global && (b == 5 || b == 6)) continue;
            Row r = rows[i];
            double* x = row_input(r, k);
            const double x0 = *x, h = k < 36 ? 1e-7 : 1e-6;
            *x = x0 + h;
            const double up = row_total(r, cfg, (double)N, nf, nb);
            *x = x0 - h;
            const double dn = row_total(r, cfg, (double)N, nf, nb);
            const double want = (up - dn) / (2 * h);
            double got;
            int which;
            if (k < 36) which = k / 18, got = g_uv[which][2 * (pos(b) * N + i) + k % 2];
            else if (k < 41) which = 2, got = g_a[(k - 36) * N + i];
            else which = 3, got = g_c[((k - 41) / 3 * N + i) * 3 + (k - 41) % 3];
            gmax[which] = fmax(gmax[which], fabs(want));
            emax[which] = fmax(emax[which], fabs(got - want));
        }
    for (int w = 0; w < 4; ++w)
        if (N > 0) {
            err = fmax(err, emax[w] / fmax(gmax[w], 1e-30));
            ok = ok && gmax[w] > 0 && emax[w] <= 2e-4 * gmax[w];             // fp32 analytic against double differences
        }
    char name[160];
    snprintf(name, sizeof(name), "atlas_losses N=%ld %s %s relevant rows: %s", N, with_global ? "9 blocks" : "7 blocks",
             with_alpha ? "alpha loss" : "no alpha loss", masks == 0 ? "random" : (masks == 1 ? "none" : (masks == 2 ? "one" : "all")));
    verdict(name, ok, err);
}

static void run_refusals() {
    Video v(3, 4, 2);
    const long N = 4;
    Buf<int64_t> idx(N);
    Buf<float> rows(9 * N * 3), o3(3 * N), o1(N), uv(9 * N * 2), a(5 * N), c(18 * N), losses(14), scratch(AL_TERMS);
    Buf<int32_t> counts(2);
    for (size_t i = 0; i < rows.n; ++i) rows[i] = 5.f;
    auto batch = [&](int64_t levels, const float* video, float* out_rows, int64_t d, const int64_t* ix) {
        return vsx_atlas_batch_f32(ix, N, v.H, v.W, v.T, levels, video, v.dx.p, v.dy.p, v.mask.p, v.flow.p, v.flow_rev.p, v.fmask.p, v.rmask.p, d, 100,
                                   1, out_rows, o3.p, o3.p, o3.p, o1.p, o1.p, o1.p, counts.p, nullptr);
    };
    bool ok = batch(1, v.video.p, rows.p, 1, idx.p) == VSX_OK;
    for (size_t i = 0; i < rows.n; ++i) rows[i] = 5.f;
    ok = ok && batch(2, v.video.p, rows.p, 1, idx.p) == VSX_E_UNSUPPORTED && batch(1, nullptr, rows.p, 1, idx.p) == VSX_E_BADSHAPE;
    ok = ok && batch(1, v.video.p, nullptr, 1, idx.p) == VSX_E_BADSHAPE && batch(1, v.video.p, rows.p, 0, idx.p) == VSX_E_BADSHAPE;
    ok = ok && batch(1, (const float*)((const char*)v.video.p + 2), rows.p, 1, idx.p) == VSX_E_BADSHAPE;
    ok = ok && batch(1, v.video.p, rows.p, 1, nullptr) == VSX_E_BADSHAPE && batch(1, v.video.p, rows.p, 1, (const int64_t*)((const char*)idx.p + 4)) == VSX_E_BADSHAPE;
    for (size_t i = 0; i < rows.n; ++i) ok = ok && rows[i] == 5.f;          // nothing was written
    vsx_atlas_loss_cfg cfg{1000.0, 5000.0, 2000.0, 1000.0, 1.0, 5.0, 50.0, 5.0, 49.0, 0.8, 48, 1, 3, 1, 1};
    for (size_t i = 0; i < losses.n; ++i) losses[i] = 5.f;
    auto loss = [&](const vsx_atlas_loss_cfg* cf, const float* in, float* g, int64_t floats) {
        return vsx_atlas_losses_f32(in, uv.p, a.p, c.p, N, o3.p, o3.p, o3.p, o1.p, o1.p, o1.p, counts.p, cf, losses.p, g, uv.p, a.p, c.p, scratch.p, floats,
                                    nullptr);
    };
    vsx_atlas_loss_cfg bad = cfg;
    ok = ok && loss(nullptr, uv.p, uv.p, AL_TERMS) == VSX_E_BADSHAPE && loss(&cfg, nullptr, uv.p, AL_TERMS) == VSX_E_BADSHAPE;
    ok = ok && loss(&cfg, uv.p, nullptr, AL_TERMS) == VSX_E_BADSHAPE && loss(&cfg, uv.p, uv.p, AL_TERMS - 1) == VSX_E_WORKSPACE;
    ok = ok && loss(&cfg, (const float*)((const char*)uv.p + 1), uv.p, AL_TERMS) == VSX_E_BADSHAPE;
    bad.uv_mapping_scale = 0.0;
    ok = ok && loss(&bad, uv.p, uv.p, AL_TERMS) == VSX_E_BADSHAPE;
    bad = cfg, bad.derivative_amount = 0;
    ok = ok && loss(&bad, uv.p, uv.p, AL_TERMS) == VSX_E_BADSHAPE;
    bad = cfg, bad.larger_dim = 0;
    ok = ok && loss(&bad, uv.p, uv.p, AL_TERMS) == VSX_E_BADSHAPE;
    for (size_t i = 0; i < losses.n; ++i) ok = ok && losses[i] == 5.f;
    ok = ok && vsx_atlas_losses_workspace(0) == AL_TERMS && vsx_atlas_losses_workspace(256) == AL_TERMS && vsx_atlas_losses_workspace(257) == 2 * AL_TERMS;
    verdict("atlas_batch / atlas_losses refusals (nothing is written)", ok, 0.0);
}

int main() {
    const long NS[] = {0, 1, 63, 64, 65, 255, 256, 257, 513};
    Video small(5, 7, 3), wide(2, 768, 2);
    for (long N : NS)
        for (int g : {1, 0}) run_batch(small, N, g, false);
    run_batch(wide, 257, 1, false);
    run_batch(small, 65, 1, true);
    for (long N : NS)
        for (int g : {1, 0})
            for (int a : {1, 0}) run_losses(N, g, a, 0);
    for (long N : {1L, 65L, 257L})
        for (int m : {1, 2, 3}) run_losses(N, 1, 1, m);
    run_refusals();
    if (n_bad) {
        printf("%d check(s) FAILED\n", n_bad);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
