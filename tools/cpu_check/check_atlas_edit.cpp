// Runs videoswap_amd/csrc/atlas_edit.hip (K15: texture reads, composition and masks of a video edited through its atlas)
// on the CPU from its real source, under AddressSanitizer and UBSan (float-cast-overflow included), and compares with a
// double-precision loop.  Every buffer has exactly the size the entry point is told, so a read or write past a texture, a
// mask or a row is a sanitizer report.  The hostile rows (NaN, +-inf, +-1e30, -0.0, just outside each edge of a box,
// exactly R - 1) are checked HERE and not on the GPU.
//   make -C tools/cpu_check check_atlas_edit && tools/cpu_check/check_atlas_edit
#include <stdio.h>
#include <stdlib.h>

#include <limits>
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

#include "atlas_edit.hip"

static unsigned rng_state = 777u;
static float frand() {                      // uniform in [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((rng_state >> 8) & 0xFFFF) / 65536.0f;
}

// exactly `n` floats at a 16-byte boundary: the sanitizer's red zone starts right behind the last one
struct Buf {
    float* p = nullptr;
    size_t n = 0;
    explicit Buf(size_t n_) : n(n_) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, (n ? n : 1) * sizeof(float))) abort();
        p = (float*)q;
        for (size_t i = 0; i < n; ++i) p[i] = 0.f;
    }
    Buf(const Buf&) = delete;
    ~Buf() { free(p); }
    float& operator[](size_t i) { return p[i]; }
};

struct Box { float minx, miny, ps; };

static int n_bad = 0;
static void verdict(const char* name, bool ok, double err, long hostile) {
    printf("%-58s max err %.2e  hostile rows %ld  %s\n", name, err, hostile, ok ? "ok" : "FAIL");
    if (!ok) ++n_bad;
}

struct Ref {
    bool rel;
    double rgb[3];
    int cell[4];
};
// the semantics of include/vsx.h K15: the position, the cell and the relevance in fp32, the colour in double from there
static Ref ref_layer(const float* tex, int R, int C, Box b, float shift, float u, float v, const float* base) {
    Ref r{};
    const float qx = u * 0.5f + shift, qy = v * 0.5f + shift;
    const float dx = qx - b.minx, dy = qy - b.miny;
    const float px = dx * b.ps, py = dy * b.ps;
    const float fx = floorf(px), fy = floorf(py), cx = ceilf(px), cy = ceilf(py);
    r.rel = fx >= 0.f && fy >= 0.f && cx < (float)R && cy < (float)R;
    if (!r.rel) return r;
    auto clip = [&](long k) { return (int)(k < 0 ? 0 : (k > R - 1 ? R - 1 : k)); };
    const int x0 = clip((long)fx), x1 = clip((long)fx + 1), y0 = clip((long)fy), y1 = clip((long)fy + 1);
    const double wa = ((double)x1 - px) * ((double)y1 - py), wb = ((double)x1 - px) * ((double)py - y0);
    const double wc = ((double)px - x0) * ((double)y1 - py), wd = ((double)px - x0) * ((double)py - y0);
    double col[4] = {0, 0, 0, 0};
    for (int k = 0; k < C; ++k)
        col[k] = tex[((long)y0 * R + x0) * C + k] * wa + tex[((long)y1 * R + x0) * C + k] * wb + tex[((long)y0 * R + x1) * C + k] * wc +
                 tex[((long)y1 * R + x1) * C + k] * wd;
    for (int k = 0; k < 3; ++k) r.rgb[k] = C == 4 ? col[k] * col[3] + (double)base[k] * (1.0 - col[3]) : col[k];
    r.cell[0] = (int)cy * R + (int)cx;
    r.cell[1] = (int)fy * R + (int)fx;
    r.cell[2] = (int)fy * R + (int)cx;
    r.cell[3] = (int)cy * R + (int)fx;
    return r;
}

// mode 0: random rows inside and outside the boxes; 1: every row in one cell; 2: the hostile rows
static void run_case(long N, int R, int CF, int CB, int mode) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float at_top = R == 2 ? 0.f : 2.f * ((float)(R - 1) / (float)R - 0.5f);       // px == R - 1 exactly in both boxes below
    const float eps = 2.3841858e-7f;                                                       // 2^-22: survives the halving and the shift
    const float hostile[] = {nan, inf, -inf, 1e30f, -1e30f, -0.0f, -1.f - eps, at_top + eps, at_top, -1.f};
    const int n_hostile = (int)(sizeof(hostile) / sizeof(hostile[0]));
    if (mode == 2) N = 4 * n_hostile;                                                      // each value as fg x, fg y, bg x, bg y
    const Box bf{0.f, 0.f, (float)R}, bb{-1.f, -1.f, (float)R};                             // [0, 1]^2 and [-1, 0]^2 at R texels
    Buf uvf(2 * N), uvb(2 * N), alpha(N), texf((size_t)R * R * CF), texb((size_t)R * R * CB), basef(3 * N), baseb(3 * N);
    Buf maskf((size_t)R * R), maskb((size_t)R * R), edit(3 * N), fg(3 * N), bg(3 * N);
    std::vector<uint8_t> rel(N ? N : 1, 0xee);
    for (size_t i = 0; i < texf.n; ++i) texf[i] = frand();
    for (size_t i = 0; i < texb.n; ++i) texb[i] = frand();
    for (long i = 0; i < N; ++i) {
        alpha[i] = 0.001f + 0.99f * frand();
        for (int k = 0; k < 3; ++k) basef[3 * i + k] = frand(), baseb[3 * i + k] = frand();
        for (int k = 0; k < 2; ++k) {
            uvf[2 * i + k] = mode == 1 ? -0.4f : frand() * 2.6f - 1.3f;                     // about a quarter of the rows outside
            uvb[2 * i + k] = mode == 1 ? -0.4f : frand() * 2.6f - 1.3f;
        }
        if (mode == 2) {
            uvf[2 * i] = uvf[2 * i + 1] = uvb[2 * i] = uvb[2 * i + 1] = -0.4f;             // inside, away from a texel edge
            const float h = hostile[i / 4];
            (i % 4 < 2 ? uvf : uvb)[2 * i + (i % 2)] = h;
        }
    }
    for (size_t i = 0; i < maskf.n; ++i) maskf[i] = 0.0005f * (float)(i % 3), maskb[i] = (i % 5 == 0) ? 0.25f : 0.f;   // initialised by the caller
    std::vector<float> wmf(maskf.p, maskf.p + maskf.n), wmb(maskb.p, maskb.p + maskb.n);
    const int rc = vsx_atlas_edit_f32(uvf.p, uvb.p, alpha.p, N, texf.p, R, R, CF, bf.minx, bf.miny, bf.ps, CF == 4 ? basef.p : nullptr,
                                      maskf.p, R, R, texb.p, R, R, CB, bb.minx, bb.miny, bb.ps, CB == 4 ? baseb.p : nullptr, maskb.p,
                                      R, R, edit.p, fg.p, bg.p, rel.data(), nullptr);
    double err = 0;
    bool ok = rc == 0;
    long hostile_rows = 0, n_rf = 0, n_rb = 0;
    for (long i = 0; i < N; ++i) {
        const Ref a = ref_layer(texf.p, R, CF, bf, 0.5f, uvf[2 * i], uvf[2 * i + 1], basef.p + 3 * i);
        const Ref b = ref_layer(texb.p, R, CB, bb, -0.5f, uvb[2 * i], uvb[2 * i + 1], baseb.p + 3 * i);
        n_rf += a.rel, n_rb += b.rel;
        ok = ok && rel[i] == (uint8_t)((a.rel ? 1 : 0) | (b.rel ? 2 : 0));
        for (int k = 0; k < 3; ++k) {
            const double wf = a.rel ? a.rgb[k] * alpha[i] : 0.0, wb = b.rel ? b.rgb[k] : 0.0;
            const double we = wf + (b.rel ? b.rgb[k] * (1.0 - (double)alpha[i]) : 0.0);
            err = fmax(err, fmax(fabs(fg[3 * i + k] - wf), fmax(fabs(bg[3 * i + k] - wb), fabs(edit[3 * i + k] - we))));
            if (!a.rel) ok = ok && fg[3 * i + k] == 0.f;
            if (!b.rel) ok = ok && bg[3 * i + k] == 0.f;
            if (!a.rel && !b.rel) ok = ok && edit[3 * i + k] == 0.f;
        }
        for (int k = 0; k < 4; ++k) {
            if (a.rel) wmf[a.cell[k]] = fmaxf(wmf[a.cell[k]], alpha[i]);
            if (b.rel) wmb[b.cell[k]] = 1.f;
        }
        if (mode == 2) {
            const int which = (int)(i / 4);
            const bool on_fg = i % 4 < 2;
            if (which < 5 || which == 6 || which == 7) {                                   // NaN, +-inf, +-1e30, just outside either edge
                ++hostile_rows;
                ok = ok && !(on_fg ? a.rel : b.rel) && (on_fg ? b.rel : a.rel);             // the other layer of the row is untouched by it
            } else {                                                                       // -0.0, exactly R - 1, exactly 0: relevant
                ok = ok && a.rel && b.rel;
                if (which == 8 && (on_fg ? CF : CB) == 3)                                  // x0 == x1 (or y0 == y1): a zero colour on a relevant row
                    for (int k = 0; k < 3; ++k) ok = ok && (on_fg ? fg : bg)[3 * i + k] == 0.f;
            }
        }
    }
    for (size_t i = 0; i < maskf.n; ++i) ok = ok && maskf[i] == wmf[i] && maskb[i] == wmb[i];   // masks: exactly the scatter-max
    if (mode == 0 && N >= 255) ok = ok && n_rf > 0 && n_rf < N && n_rb > 0 && n_rb < N;          // both branches of both layers
    if (mode == 1) ok = ok && n_rf == N && n_rb == N;
    ok = ok && err <= 2e-6;       // four products and three sums in fp32 on values in [0, 1]: a few 2^-24, against ~1e-1 for a wrong texel
    char name[128];
    snprintf(name, sizeof(name), "atlas_edit %s N=%ld R=%d C=(%d,%d)", mode == 0 ? "random" : (mode == 1 ? "one cell" : "hostile"), N, R, CF, CB);
    verdict(name, ok, err, hostile_rows);
}

static void run_refusals() {
    Buf t(64), o(12), m(16);
    std::vector<uint8_t> rel(4);
    auto call = [&](int64_t h, int64_t w, int64_t c, const float* base, float* mask, int64_t mh, const float* tex) {
        return vsx_atlas_edit_f32(o.p, o.p, o.p, 0, tex, h, w, c, 0.f, 0.f, 1.f, base, mask, mh, mh, t.p, 2, 2, 3, 0.f, 0.f, 1.f, nullptr,
                                  nullptr, 0, 0, o.p, o.p, o.p, rel.data(), nullptr);
    };
    bool ok = call(2, 2, 3, nullptr, nullptr, 0, t.p) == VSX_OK && call(2, 2, 4, o.p, m.p, 2, t.p) == VSX_OK;   // N = 0 works
    ok = ok && call(2, 2, 5, nullptr, nullptr, 0, t.p) == VSX_E_UNSUPPORTED && call(2, 2, 2, nullptr, nullptr, 0, t.p) == VSX_E_UNSUPPORTED;
    ok = ok && call(2, 3, 3, nullptr, nullptr, 0, t.p) == VSX_E_BADSHAPE && call(1, 1, 3, nullptr, nullptr, 0, t.p) == VSX_E_BADSHAPE;
    ok = ok && call(2, 2, 4, nullptr, nullptr, 0, t.p) == VSX_E_BADSHAPE && call(2, 2, 3, nullptr, m.p, 4, t.p) == VSX_E_BADSHAPE;
    ok = ok && call(26755, 26755, 3, nullptr, nullptr, 0, t.p) == VSX_E_BADSHAPE && call(2, 2, 3, nullptr, nullptr, 0, t.p + 1) == VSX_E_BADSHAPE;
    verdict("atlas_edit refusals (nothing is read)", ok, 0.0, 0);
}

int main() {
    for (int R : {2, 16})
        for (int C : {3, 4}) {
            for (long N : {1L, 255L, 256L, 257L}) run_case(N, R, C, C, 0);
            run_case(257, R, C, C, 1);
            run_case(0, R, C, C, 2);
        }
    run_case(257, 16, 3, 4, 0);
    run_case(257, 16, 4, 3, 0);
    run_case(1000, 4, 3, 3, 1);
    run_refusals();
    if (n_bad) {
        printf("%d check(s) FAILED\n", n_bad);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
