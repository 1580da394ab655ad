// Runs K17 on the CPU from its real source under AddressSanitizer and UBSan: the hash instantiation of the training forward
// (csrc/atlas.hip), the dEnc step and the grid backward (csrc/atlas_bwd.hip), and compares with double-precision loops.
// Every buffer (x, table, packed, out, saved, scratch, grad, grad_table, grad_x, grad_out) has exactly the size the workspace
// query states, so a read or write of a row >= N, of a column >= E or past the table is a sanitizer report.
// Each stage is judged on its own input: the layer gradients and dEnc against double loops over the activations the forward
// STORED, the grid backward against double loops over the dEnc the kernel left in scratch.  The float atomicAdd of the table
// gradient is a compare-exchange here (hip/hip_runtime.h); the work-items of a workgroup are OS threads, so its order varies.
//   make -C tools/cpu_check check_hash_fit && tools/cpu_check/check_hash_fit
#define CPUHIP_DYNAMIC_LDS_ONLY
#include "hip/hip_runtime.h"
#include "hip_mfma_f32.h"

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

namespace {
CPUHIP_DEFINE_LDS
}
#include "atlas.hip"
#include "atlas_bwd.hip"

static unsigned rng_state = 777u;
static float frand() {                      // uniform in [-1, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((rng_state >> 8) & 0xFFFF) / 32768.0f - 1.0f;
}

// exactly `n` floats at a 16-byte boundary: the sanitizer's red zone starts right behind the last one
struct Buf {
    float* p = nullptr;
    size_t n = 0;
    explicit Buf(size_t n_, float fill = 0.f) : n(n_) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, (n ? n : 1) * sizeof(float))) abort();
        p = (float*)q;
        for (size_t i = 0; i < n; ++i) p[i] = fill;
    }
    Buf(const Buf&) = delete;
    ~Buf() { free(p); }
    float& operator[](size_t i) { return p[i]; }
    bool all(float v) const {
        for (size_t i = 0; i < n; ++i)
            if (!(p[i] == v)) return false;
        return true;
    }
};

static int n_bad = 0;
static void verdict(const char* name, bool ok, double a, double b, double c) {
    printf("%-72s fwd %.1e layers %.1e grid %.1e  %s\n", name, a, b, c, ok ? "ok" : "FAIL");
    if (!ok) ++n_bad;
}

struct Grid {
    int n_levels, log2, base;
    double pls;
    int E() const { return 2 * n_levels; }
};
struct Net {
    int out_dim, hidden, layers, skip_mask, use_tanh;
    bool has_enc(int l) const { return l == 0 || ((skip_mask >> l) & 1); }
    int F(int l) const { return l == layers - 1 ? out_dim : hidden; }
    int K(int l, int E) const { return (l > 0 ? hidden : 0) + (has_enc(l) ? E : 0); }
};
struct Levels {
    std::vector<float> scale;
    std::vector<uint32_t> res, entries, offset, hashed;
    int64_t floats;
    explicit Levels(const Grid& g) : scale(g.n_levels), res(g.n_levels), entries(g.n_levels), offset(g.n_levels), hashed(g.n_levels) {
        floats = vsx_hash_grid_geometry(g.n_levels, 2, g.log2, g.base, g.pls, scale.data(), res.data(), entries.data(), offset.data(),
                                        hashed.data());
    }
};

// nn.Linear weights [F][K] -> the packed buffer of vsx.h K13
static size_t pack(const Net& n, int E, const std::vector<std::vector<float>>& W, const std::vector<std::vector<float>>& B, float* dst) {
    const int encp = (E + 7) / 8 * 8;
    size_t off = 0;
    for (int l = 0; l < n.layers; ++l) {
        const int Fp = l == n.layers - 1 ? 32 : n.hidden, kh = l > 0 ? n.hidden : 0, Kp = kh + (n.has_enc(l) ? encp : 0);
        if (dst) {
            for (int i = 0; i < Fp * Kp + Fp; ++i) dst[off + i] = 0.f;
            for (int f = 0; f < n.F(l); ++f) {
                for (int k = 0; k < n.K(l, E); ++k)
                    dst[off + ((size_t)((f / 32) * (Kp / 8) + k / 8) * 2 + (k % 8) / 4) * 128 + (f % 32) * 4 + k % 4] = W[l][(size_t)f * n.K(l, E) + k];
                dst[off + (size_t)Fp * Kp + f] = B[l][f];
            }
        }
        off += (size_t)Fp * Kp + Fp;
    }
    return off;
}

// the cell of a row on a level as vsx.h K14 states it (the position in fp32, like the kernel), weights in double
struct Cell {
    double w0, w1;
    uint32_t idx[4];
};
static Cell cell_of(const Levels& lv, int l, float x0, float x1) {
    const float p0 = fmaf(lv.scale[l], x0, 0.5f), p1 = fmaf(lv.scale[l], x1, 0.5f);
    const float f0 = floorf(p0), f1 = floorf(p1);
    Cell c;
    c.w0 = (double)lv.scale[l] * x0 + 0.5 - f0, c.w1 = (double)lv.scale[l] * x1 + 0.5 - f1;
    const uint32_t g0 = (uint32_t)(int)f0, g1 = (uint32_t)(int)f1;
    for (int k = 0; k < 4; ++k) {
        const uint32_t c0 = g0 + (k & 1), c1 = g1 + (k >> 1);
        const uint32_t i = lv.hashed[l] ? (c0 ^ (c1 * 2654435761u)) : c0 + c1 * lv.res[l];
        c.idx[k] = lv.offset[l] + i % lv.entries[l];
    }
    return c;
}

// the grid backward in double -> (err of grad_table, err of grad_x), each max |got - want| / the largest magnitude a correct
// term sum can reach (the sum of the absolute values of the terms: cancellation cannot make the yardstick small)
static void grid_backward_check(const Grid& g, const Levels& lv, long N, const float* x, const float* genc, const float* table,
                                const float* got_table, const float* got_x, double& e_table, double& e_x, bool& exact_zero) {
    const int E = g.E();
    std::vector<double> want_t(lv.floats, 0.0), mag_t(lv.floats, 0.0), want_x(2 * N, 0.0), mag_x(2 * N, 0.0);
    std::vector<char> touched(lv.floats, 0);
    for (long r = 0; r < N; ++r)
        for (int l = 0; l < g.n_levels; ++l) {
            const Cell c = cell_of(lv, l, x[2 * r], x[2 * r + 1]);
            for (int k = 0; k < 4; ++k) {
                const double a0 = (k & 1) ? c.w0 : 1 - c.w0, a1 = (k >> 1) ? c.w1 : 1 - c.w1;
                for (int f = 0; f < 2; ++f) {
                    const double ge = genc[r * E + 2 * l + f], t = table[2 * (size_t)c.idx[k] + f];
                    want_t[2 * (size_t)c.idx[k] + f] += a0 * a1 * ge, mag_t[2 * (size_t)c.idx[k] + f] += fabs(a0 * a1 * ge);
                    touched[2 * (size_t)c.idx[k] + f] = 1;
                    const double d0 = ((k & 1) ? 1 : -1) * a1 * t * ge * lv.scale[l], d1 = ((k >> 1) ? 1 : -1) * a0 * t * ge * lv.scale[l];
                    want_x[2 * r] += d0, want_x[2 * r + 1] += d1, mag_x[2 * r] += fabs(d0), mag_x[2 * r + 1] += fabs(d1);
                }
            }
        }
    e_table = e_x = 0, exact_zero = true;
    if (got_table) {
        double mx = 0, diff = 0;
        for (int64_t i = 0; i < lv.floats; ++i) {
            mx = fmax(mx, mag_t[i]), diff = fmax(diff, fabs(want_t[i] - got_table[i]));
            if (!touched[i] && got_table[i] != 0.f) exact_zero = false;
        }
        e_table = mx > 0 ? diff / mx : diff;
    }
    if (got_x) {
        double mx = 0, diff = 0;
        for (long i = 0; i < 2 * N; ++i) mx = fmax(mx, mag_x[i]), diff = fmax(diff, fabs(want_x[i] - got_x[i]));
        e_x = mx > 0 ? diff / mx : diff;
    }
}

enum Rows { UNIFORM, ONE_CELL };

static void run_case(const char* tag, const Net& n, const Grid& g, long N, Rows rows) {
    const int L = n.layers, E = g.E();
    const Levels lv(g);
    bool ok = lv.floats > 0;
    std::vector<std::vector<float>> W(L), B(L);
    for (int l = 0; l < L; ++l) {
        const float s = 1.0f / sqrtf((float)n.K(l, E));
        W[l].resize((size_t)n.F(l) * n.K(l, E));
        B[l].resize(n.F(l));
        for (auto& v : W[l]) v = frand() * s * 1.7f;
        for (auto& v : B[l]) v = frand() * s;
    }
    Buf packed(pack(n, E, W, B, nullptr));
    pack(n, E, W, B, packed.p);
    Buf table((size_t)lv.floats);
    for (size_t i = 0; i < table.n; ++i) table[i] = 0.5f * frand();
    int64_t sf = -1, scf = -1, gf = -1;
    ok = ok && vsx_hash_mlp_train_workspace(N, 2, g.n_levels, 2, g.log2, g.base, g.pls, n.out_dim, n.hidden, L, n.skip_mask, &sf, &scf, &gf) == VSX_OK;
    long P = 0;
    for (int l = 0; l < L; ++l) P += (long)n.F(l) * n.K(l, E) + n.F(l);
    const long chunks = (N + CMB_ROWS - 1) / CMB_ROWS;
    ok = ok && gf == P && sf == N * ((long)(L - 1) * n.hidden + E + n.out_dim);
    ok = ok && scf == chunks * P + 2 * N * n.hidden + N * n.out_dim + N * E;
    Buf x((size_t)N * 2), out((size_t)N * n.out_dim), out_plain((size_t)N * n.out_dim), saved((size_t)sf, -7.f);
    Buf gout((size_t)N * n.out_dim), scratch((size_t)scf, -3.f), grad((size_t)gf, 99.f), grad2((size_t)gf, 98.f);
    Buf gt((size_t)lv.floats, 97.f), gt2((size_t)lv.floats, 96.f), gx((size_t)N * 2, 95.f), gx2((size_t)N * 2, 94.f);
    for (long r = 0; r < N; ++r) {
        // ONE_CELL: every row inside one cell of the finest level (the cells of the coarser levels contain it or split it in two)
        x[2 * r] = rows == ONE_CELL ? 0.3f + 1e-4f * (1.0f + frand()) : frand();
        x[2 * r + 1] = rows == ONE_CELL ? -0.6f + 1e-4f * (1.0f + frand()) : frand();
    }
    for (size_t i = 0; i < gout.n; ++i) gout[i] = frand();

    ok = ok && vsx_hash_mlp_f32(x.p, N, 2, table.p, lv.floats, g.n_levels, 2, g.log2, g.base, g.pls, n.out_dim, n.hidden, L, n.skip_mask,
                                n.use_tanh, packed.p, (int64_t)packed.n, out_plain.p, nullptr) == VSX_OK;
    ok = ok && vsx_hash_mlp_fwd_train_f32(x.p, N, 2, table.p, lv.floats, g.n_levels, 2, g.log2, g.base, g.pls, n.out_dim, n.hidden, L,
                                          n.skip_mask, n.use_tanh, packed.p, (int64_t)packed.n, out.p, saved.p, sf, nullptr) == VSX_OK;
    ok = ok && memcmp(out.p, out_plain.p, out.n * sizeof(float)) == 0;                       // the same bits as K14

    // the forward against a double-precision network
    const float* sh = saved.p;
    const float* senc = saved.p + (size_t)(L - 1) * N * n.hidden;
    const float* sout = senc + (size_t)N * E;
    double e_fwd = 0;
    for (long r = 0; r < N; ++r) {
        std::vector<double> enc(E, 0.0), h, z;
        for (int l = 0; l < g.n_levels; ++l) {
            const Cell c = cell_of(lv, l, x[2 * r], x[2 * r + 1]);
            for (int k = 0; k < 4; ++k)
                for (int f = 0; f < 2; ++f)
                    enc[2 * l + f] += ((k & 1) ? c.w0 : 1 - c.w0) * ((k >> 1) ? c.w1 : 1 - c.w1) * table[2 * (size_t)c.idx[k] + f];
        }
        for (int e = 0; e < E; ++e) e_fwd = fmax(e_fwd, fabs(enc[e] - senc[r * E + e]));
        for (int l = 0; l < L; ++l) {
            std::vector<double> in(h);
            if (n.has_enc(l)) in.insert(in.end(), enc.begin(), enc.end());
            z.assign(n.F(l), 0.0);
            for (int f = 0; f < n.F(l); ++f) {
                double s = B[l][f];
                for (int k = 0; k < n.K(l, E); ++k) s += (double)W[l][(size_t)f * n.K(l, E) + k] * in[k];
                z[f] = s;
            }
            if (l < L - 1) {
                h.assign(n.hidden, 0.0);
                for (int f = 0; f < n.hidden; ++f) {
                    h[f] = z[f] > 0 ? z[f] : 0.0;
                    e_fwd = fmax(e_fwd, fabs(h[f] - sh[((size_t)l * N + r) * n.hidden + f]));
                }
            }
        }
        for (int f = 0; f < n.out_dim; ++f) {
            e_fwd = fmax(e_fwd, fabs((n.use_tanh ? tanh(z[f]) : z[f]) - out[r * n.out_dim + f]));
            ok = ok && sout[r * n.out_dim + f] == out[r * n.out_dim + f];
        }
    }
    // features of at most 0.5 (the fp32 position at scale <= 140 moves a weight by 1e-5), activations of O(1) through at most
    // four layers of at most 104 fp32 products: a few 1e-6; a wrong index gives O(0.1)
    ok = ok && e_fwd <= 3e-5;

    auto bwd = [&](Buf& gr, float* t, float* xx) {
        return vsx_hash_mlp_bwd_f32(gout.p, x.p, N, 2, table.p, lv.floats, g.n_levels, 2, g.log2, g.base, g.pls, n.out_dim, n.hidden, L,
                                    n.skip_mask, n.use_tanh, packed.p, (int64_t)packed.n, saved.p, sf, scratch.p, scf, gr.p, gf, t, xx,
                                    nullptr);
    };
    ok = ok && bwd(grad, gt.p, gx.p) == VSX_OK && bwd(grad2, gt2.p, gx2.p) == VSX_OK;
    ok = ok && memcmp(grad.p, grad2.p, grad.n * sizeof(float)) == 0 && memcmp(gx.p, gx2.p, gx.n * sizeof(float)) == 0;   // deterministic
    if (N == 0) ok = ok && grad.all(0.f) && gt.all(0.f);

    // layer gradients and dEnc in double over the STORED activations
    std::vector<double> want(P, 0.0), want_denc((size_t)N * E, 0.0);
    std::vector<long> goff(L);
    for (long l = 0, o = 0; l < L; ++l) goff[l] = o, o += (long)n.F(l) * n.K(l, E) + n.F(l);
    for (long r = 0; r < N; ++r) {
        std::vector<double> dz(n.out_dim);
        for (int f = 0; f < n.out_dim; ++f) {
            const double o = sout[r * n.out_dim + f];
            dz[f] = gout[r * n.out_dim + f] * (n.use_tanh ? 1.0 - o * o : 1.0);
        }
        for (int l = L - 1; l >= 0; --l) {
            const int kh = l > 0 ? n.hidden : 0, K = n.K(l, E);
            const float* hp = l > 0 ? sh + ((size_t)(l - 1) * N + r) * n.hidden : nullptr;
            for (int f = 0; f < n.F(l); ++f) {
                for (int k = 0; k < K; ++k) want[goff[l] + (long)f * K + k] += dz[f] * (k < kh ? hp[k] : senc[r * E + k - kh]);
                want[goff[l] + (long)n.F(l) * K + f] += dz[f];
            }
            if (l == 0) {                              // only layer 0 passes a gradient to the encoding
                for (int e = 0; e < E; ++e)
                    for (int f = 0; f < n.F(0); ++f) want_denc[r * E + e] += dz[f] * (double)W[0][(size_t)f * K + e];
                break;
            }
            std::vector<double> dh(n.hidden, 0.0);
            for (int k = 0; k < n.hidden; ++k) {
                if (!(hp[k] > 0.f)) continue;
                for (int f = 0; f < n.F(l); ++f) dh[k] += dz[f] * (double)W[l][(size_t)f * K + k];
            }
            dz = dh;
        }
    }
    double e_bwd = 0;
    for (int l = 0; l < L && N > 0; ++l) {
        const long K = n.K(l, E), nw = (long)n.F(l) * K;
        for (int part = 0; part < 2; ++part) {
            const long o = goff[l] + (part ? nw : 0), cnt = part ? n.F(l) : nw;
            double mx = 0, diff = 0;
            for (long i = 0; i < cnt; ++i) mx = fmax(mx, fabs(want[o + i])), diff = fmax(diff, fabs(want[o + i] - grad[o + i]));
            if (mx > 0) e_bwd = fmax(e_bwd, diff / mx);
            ok = ok && (mx > 0 || diff == 0);
        }
    }
    const float* denc = scratch.p + (scf - N * E);
    {
        double mx = 0, diff = 0;
        for (size_t i = 0; i < want_denc.size(); ++i) mx = fmax(mx, fabs(want_denc[i])), diff = fmax(diff, fabs(want_denc[i] - denc[i]));
        if (mx > 0) e_bwd = fmax(e_bwd, diff / mx);
    }
    // as check_atlas_fit: sums of at most 513 fp32 products, relative to the tensor's largest element
    ok = ok && e_bwd <= 2e-5;

    // the grid backward over the dEnc the kernel used; both calls' tables (the order of the atomic adds differs)
    double et = 0, ex = 0, et2 = 0, ex2 = 0;
    bool z1 = true, z2 = true;
    grid_backward_check(g, lv, N, x.p, denc, table.p, gt.p, gx.p, et, ex, z1);
    grid_backward_check(g, lv, N, x.p, denc, table.p, gt2.p, gx2.p, et2, ex2, z2);
    // at most 513 * 4 fp32 adds of one sign pattern per entry, eight fmaf per level and 20 levels per row, against the sum of
    // the terms' magnitudes: 1e-6 at most; a wrong corner, sign or level gives 1e-2 and more
    double e_grid = fmax(fmax(et, et2), fmax(ex, ex2));
    ok = ok && e_grid <= 2e-5 && z1 && z2;

    // the grid backward alone, on a random grad_enc: both, the table only, x only; a null output is not touched
    if (N > 0) {
        Buf genc((size_t)N * E), t1((size_t)lv.floats, 93.f), x1((size_t)N * 2, 92.f), t2((size_t)lv.floats, 91.f), x2((size_t)N * 2, 90.f);
        for (size_t i = 0; i < genc.n; ++i) genc[i] = frand();
        auto alone = [&](float* t, float* xx) {
            return vsx_hash_grid_bwd_f32(x.p, N, 2, genc.p, table.p, lv.floats, g.n_levels, 2, g.log2, g.base, g.pls, t, xx, nullptr);
        };
        ok = ok && alone(t1.p, x1.p) == VSX_OK && alone(t2.p, nullptr) == VSX_OK && alone(nullptr, x2.p) == VSX_OK;
        ok = ok && memcmp(x1.p, x2.p, x1.n * sizeof(float)) == 0;
        grid_backward_check(g, lv, N, x.p, genc.p, table.p, t1.p, x1.p, et, ex, z1);
        grid_backward_check(g, lv, N, x.p, genc.p, table.p, t2.p, nullptr, et2, ex2, z2);
        e_grid = fmax(e_grid, fmax(fmax(et, et2), ex));
        ok = ok && e_grid <= 2e-5 && z1 && z2;
    }
    char name[200];
    snprintf(name, sizeof(name), "hash_fit %s levels %d hidden %d layers %d skip 0x%x out %d tanh %d N=%ld", tag, g.n_levels, n.hidden,
             n.layers, n.skip_mask, n.out_dim, n.use_tanh, N);
    verdict(name, ok, e_fwd, e_bwd, e_grid);
}

static void run_refusals() {
    const Net n{3, 32, 2, 0, 1};
    const Grid g{4, 8, 4, 2.0};
    const Levels lv(g);
    const long N = 5;
    const int E = g.E();
    int64_t sf = 0, scf = 0, gf = 0;
    bool ok = vsx_hash_mlp_train_workspace(N, 2, 4, 2, 8, 4, 2.0, 3, 32, 2, 0, &sf, &scf, &gf) == VSX_OK;
    std::vector<std::vector<float>> W(2), B(2);
    for (int l = 0; l < 2; ++l) W[l].assign((size_t)n.F(l) * n.K(l, E), 0.25f), B[l].assign(n.F(l), 0.1f);
    Buf packed(pack(n, E, W, B, nullptr));
    pack(n, E, W, B, packed.p);
    Buf x(N * 2, 0.5f), table((size_t)lv.floats, 0.1f), out(N * 3, 55.f), saved((size_t)sf, 55.f), gout(N * 3, 1.f);
    Buf scratch((size_t)scf, 55.f), grad((size_t)gf, 55.f), gt((size_t)lv.floats, 55.f), gx(N * 2, 55.f), genc(N * E, 1.f);
    struct Opt {
        int64_t in_dim = 2, levels = 4, feats = 2, log2 = 8, base = 4;
        double pls = 2.0;
        int64_t odim = 3, hidden = 32, layers = 2, skip = 0, table_floats = -1, s = -1, sc = -1, g = -1;
        float* table = nullptr;
        float* gt = nullptr;
    };
    auto fwd = [&](Opt o) {
        return vsx_hash_mlp_fwd_train_f32(x.p, N, o.in_dim, o.table ? o.table : table.p, o.table_floats < 0 ? lv.floats : o.table_floats,
                                          o.levels, o.feats, o.log2, o.base, o.pls, o.odim, o.hidden, o.layers, o.skip, 1, packed.p,
                                          (int64_t)packed.n, out.p, saved.p, o.s < 0 ? sf : o.s, nullptr);
    };
    auto bwd = [&](Opt o) {
        return vsx_hash_mlp_bwd_f32(gout.p, x.p, N, o.in_dim, o.table ? o.table : table.p, o.table_floats < 0 ? lv.floats : o.table_floats,
                                    o.levels, o.feats, o.log2, o.base, o.pls, o.odim, o.hidden, o.layers, o.skip, 1, packed.p,
                                    (int64_t)packed.n, saved.p, o.s < 0 ? sf : o.s, scratch.p, o.sc < 0 ? scf : o.sc, grad.p,
                                    o.g < 0 ? gf : o.g, o.gt ? o.gt : gt.p, gx.p, nullptr);
    };
    auto alone = [&](Opt o) {
        return vsx_hash_grid_bwd_f32(x.p, N, o.in_dim, genc.p, o.table ? o.table : table.p, o.table_floats < 0 ? lv.floats : o.table_floats,
                                     o.levels, o.feats, o.log2, o.base, o.pls, o.gt ? o.gt : gt.p, gx.p, nullptr);
    };
    auto all3 = [&](Opt o, int want) { return fwd(o) == want && bwd(o) == want && alone(o) == want; };
    Opt o;
    // a short buffer: VSX_E_WORKSPACE
    o = Opt{}, o.s = sf - 1;
    ok = ok && fwd(o) == VSX_E_WORKSPACE && bwd(o) == VSX_E_WORKSPACE;
    o = Opt{}, o.sc = scf - 1;
    ok = ok && bwd(o) == VSX_E_WORKSPACE;
    o = Opt{}, o.g = gf - 1;
    ok = ok && bwd(o) == VSX_E_WORKSPACE;
    // a table of another length, a misaligned table or grad_table: VSX_E_BADSHAPE
    o = Opt{}, o.table_floats = lv.floats - 2;
    ok = ok && all3(o, VSX_E_BADSHAPE);
    o = Opt{}, o.table = table.p + 1;
    ok = ok && all3(o, VSX_E_BADSHAPE);
    o = Opt{}, o.gt = gt.p + 1;
    ok = ok && bwd(o) == VSX_E_BADSHAPE && alone(o) == VSX_E_BADSHAPE;
    // the options K14 refuses
    o = Opt{}, o.in_dim = 3;
    ok = ok && all3(o, VSX_E_UNSUPPORTED);
    o = Opt{}, o.feats = 4;
    ok = ok && all3(o, VSX_E_UNSUPPORTED);
    o = Opt{}, o.levels = 33;
    ok = ok && all3(o, VSX_E_UNSUPPORTED);
    o = Opt{}, o.log2 = 25;
    ok = ok && all3(o, VSX_E_UNSUPPORTED);
    o = Opt{}, o.base = 0;
    ok = ok && all3(o, VSX_E_UNSUPPORTED);
    o = Opt{}, o.pls = 0.5;
    ok = ok && all3(o, VSX_E_UNSUPPORTED);
    // the options K13 refuses
    o = Opt{}, o.hidden = 48;
    ok = ok && fwd(o) == VSX_E_UNSUPPORTED && bwd(o) == VSX_E_UNSUPPORTED;
    o = Opt{}, o.layers = 9;
    ok = ok && fwd(o) == VSX_E_UNSUPPORTED && bwd(o) == VSX_E_UNSUPPORTED;
    o = Opt{}, o.odim = 4;
    ok = ok && fwd(o) == VSX_E_UNSUPPORTED && bwd(o) == VSX_E_UNSUPPORTED;
    o = Opt{}, o.skip = 1;
    ok = ok && fwd(o) == VSX_E_UNSUPPORTED && bwd(o) == VSX_E_UNSUPPORTED;
    ok = ok && vsx_hash_mlp_train_workspace(N, 3, 4, 2, 8, 4, 2.0, 3, 32, 2, 0, &sf, &scf, &gf) == VSX_E_UNSUPPORTED;
    ok = ok && vsx_hash_mlp_train_workspace(N, 2, 4, 2, 8, 4, 2.0, 3, 48, 2, 0, &sf, &scf, &gf) == VSX_E_UNSUPPORTED;
    // nothing was written
    ok = ok && out.all(55.f) && saved.all(55.f) && scratch.all(55.f) && grad.all(55.f) && gt.all(55.f) && gx.all(55.f);
    verdict("hash_fit refusals (nothing is written)", ok, 0.0, 0.0, 0.0);
}

int main() {
    const Net small{3, 32, 2, 0x0, 1};          // two layers
    const Net skip{3, 64, 4, 0x4, 1};           // skip layer 2: its encoded columns get weight gradients and pass nothing on
    const Net linear{2, 32, 3, 0x0, 0};         // linear output
    const Grid dense{2, 10, 4, 2.0};            // 16 and 64 entries: both levels dense
    const Grid hashed{4, 8, 4, 2.0};            // the last level (res 32) is hashed into 256 entries
    const Grid twenty{20, 8, 4, 1.2};           // a second pass of levels, E = 40: neither a multiple of 32 nor of 16
    for (long N : {0L, 1L, 63L, 64L, 65L, 513L}) {
        run_case("dense", small, dense, N, UNIFORM);
        run_case("hashed", skip, hashed, N, UNIFORM);
    }
    for (long N : {1L, 65L}) run_case("twenty", linear, twenty, N, UNIFORM);
    run_case("twenty", skip, twenty, 513, UNIFORM);
    run_case("one cell", small, hashed, 513, ONE_CELL);
    run_case("one cell", linear, twenty, 65, ONE_CELL);
    run_refusals();
    if (n_bad) {
        printf("%d check(s) FAILED\n", n_bad);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
