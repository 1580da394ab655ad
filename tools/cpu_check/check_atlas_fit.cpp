// Runs the training forward of csrc/atlas.hip (the Train instantiation of coord_mlp_kernel) and csrc/atlas_bwd.hip (K16:
// weight and bias gradients of the coordinate MLP) on the CPU from their real source, under AddressSanitizer and UBSan, and
// compares with double-precision loops.  Every buffer (x, packed, out, saved, scratch, grad, grad_out) has exactly the size the
// workspace query states, so a read or write of a row >= N, of a padded feature or past a chunk is a sanitizer report.
// The forward is compared with a double-precision network; the backward is compared with double-precision loops over the
// activations the forward STORED (that is its contract: the ReLU mask is the stored activation's), so each kernel is judged
// on its own and a pre-activation within rounding of zero cannot blur the verdict.
//   make -C tools/cpu_check check_atlas_fit && tools/cpu_check/check_atlas_fit
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

static unsigned rng_state = 2024u;
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
static void verdict(const char* name, bool ok, double e_fwd, double e_bwd) {
    printf("%-64s fwd err %.2e  grad err %.2e  %s\n", name, e_fwd, e_bwd, ok ? "ok" : "FAIL");
    if (!ok) ++n_bad;
}

struct Net {
    int in_dim, out_dim, hidden, layers, pe_dim, skip_mask, use_tanh;     // pe_dim 0: pe_type none
    int enc() const { return pe_dim ? 2 * in_dim * pe_dim : in_dim; }
    bool has_enc(int l) const { return l == 0 || ((skip_mask >> l) & 1); }
    int F(int l) const { return l == layers - 1 ? out_dim : hidden; }
    int K(int l) const { return (l > 0 ? hidden : 0) + (has_enc(l) ? enc() : 0); }
};

// nn.Linear weights [F][K] -> the packed buffer of vsx.h K13
static size_t pack(const Net& n, const std::vector<std::vector<float>>& W, const std::vector<std::vector<float>>& B, float* dst) {
    const int encp = (n.enc() + 7) / 8 * 8;
    size_t off = 0;
    for (int l = 0; l < n.layers; ++l) {
        const int Fp = l == n.layers - 1 ? 32 : n.hidden, kh = l > 0 ? n.hidden : 0, Kp = kh + (n.has_enc(l) ? encp : 0);
        if (dst) {
            for (int i = 0; i < Fp * Kp + Fp; ++i) dst[off + i] = 0.f;
            for (int f = 0; f < n.F(l); ++f) {
                for (int k = 0; k < n.K(l); ++k)
                    dst[off + ((size_t)((f / 32) * (Kp / 8) + k / 8) * 2 + (k % 8) / 4) * 128 + (f % 32) * 4 + k % 4] = W[l][(size_t)f * n.K(l) + k];
                dst[off + (size_t)Fp * Kp + f] = B[l][f];
            }
        }
        off += (size_t)Fp * Kp + Fp;
    }
    return off;
}

static void run_case(const Net& n, long N) {
    const int L = n.layers, E = n.enc(), pe_type = n.pe_dim ? 1 : 0;
    std::vector<std::vector<float>> W(L), B(L);
    for (int l = 0; l < L; ++l) {
        const float s = 1.0f / sqrtf((float)n.K(l));
        W[l].resize((size_t)n.F(l) * n.K(l));
        B[l].resize(n.F(l));
        for (auto& v : W[l]) v = frand() * s * 1.7f;
        for (auto& v : B[l]) v = frand() * s;
    }
    Buf packed(pack(n, W, B, nullptr));
    pack(n, W, B, packed.p);
    int64_t sf = -1, scf = -1, gf = -1;
    bool ok = vsx_coord_mlp_train_workspace(N, n.in_dim, n.out_dim, n.hidden, L, pe_type, n.pe_dim, 0, n.skip_mask, &sf, &scf, &gf) == VSX_OK;
    long P = 0;
    for (int l = 0; l < L; ++l) P += (long)n.F(l) * n.K(l) + n.F(l);
    ok = ok && gf == P && sf == N * ((long)(L - 1) * n.hidden + E + n.out_dim);
    Buf x((size_t)N * n.in_dim), out((size_t)N * n.out_dim), out_plain((size_t)N * n.out_dim), saved((size_t)sf, -7.f);
    Buf gout((size_t)N * n.out_dim), scratch((size_t)scf, -3.f), grad((size_t)gf, 99.f), grad2((size_t)gf, 98.f);
    for (size_t i = 0; i < x.n; ++i) x[i] = frand();
    for (size_t i = 0; i < gout.n; ++i) gout[i] = frand();

    ok = ok && vsx_coord_mlp_f32(x.p, N, n.in_dim, n.out_dim, n.hidden, L, pe_type, n.pe_dim, 0, n.skip_mask, n.use_tanh, packed.p,
                                 (int64_t)packed.n, out_plain.p, nullptr) == VSX_OK;
    ok = ok && vsx_coord_mlp_fwd_train_f32(x.p, N, n.in_dim, n.out_dim, n.hidden, L, pe_type, n.pe_dim, 0, n.skip_mask, n.use_tanh,
                                           packed.p, (int64_t)packed.n, out.p, saved.p, sf, nullptr) == VSX_OK;
    ok = ok && memcmp(out.p, out_plain.p, out.n * sizeof(float)) == 0;                       // the same bits as K13

    // the forward against a double-precision network; the stored copy of `out` against `out`
    const float* sh = saved.p;
    const float* senc = saved.p + (size_t)(L - 1) * N * n.hidden;
    const float* sout = senc + (size_t)N * E;
    double e_fwd = 0;
    for (long r = 0; r < N; ++r) {
        std::vector<double> enc(E), h, z;
        for (int e = 0; e < E; ++e) {
            if (!n.pe_dim) {
                enc[e] = x[r * n.in_dim + e];
            } else {
                const int j = e / (2 * n.in_dim), rem = e % (2 * n.in_dim);
                const double arg = (double)x[r * n.in_dim + rem % n.in_dim] * (double)ldexpf(3.14159274101257324f, j);
                enc[e] = rem >= n.in_dim ? cos(arg) : sin(arg);
            }
            e_fwd = fmax(e_fwd, fabs(enc[e] - senc[r * E + e]));
        }
        for (int l = 0; l < L; ++l) {
            std::vector<double> in(h);
            if (n.has_enc(l)) in.insert(in.end(), enc.begin(), enc.end());
            z.assign(n.F(l), 0.0);
            for (int f = 0; f < n.F(l); ++f) {
                double s = B[l][f];
                for (int k = 0; k < n.K(l); ++k) s += (double)W[l][(size_t)f * n.K(l) + k] * in[k];
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
    // activations of O(1) through at most five layers of at most 82 fp32 products: a few 1e-6; a wrong index gives O(0.1)
    ok = ok && e_fwd <= 2e-5;
    if (N == 0) ok = ok && saved.n == 0;

    auto bwd = [&](Buf& g) {
        return vsx_coord_mlp_bwd_f32(gout.p, N, n.in_dim, n.out_dim, n.hidden, L, pe_type, n.pe_dim, 0, n.skip_mask, n.use_tanh, packed.p,
                                     (int64_t)packed.n, saved.p, sf, scratch.p, scf, g.p, gf, nullptr);
    };
    ok = ok && bwd(grad) == VSX_OK && bwd(grad2) == VSX_OK;
    ok = ok && memcmp(grad.p, grad2.p, grad.n * sizeof(float)) == 0;                          // deterministic
    if (N == 0) ok = ok && grad.all(0.f);

    // the backward in double over the STORED activations
    std::vector<double> want(P, 0.0);
    std::vector<long> goff(L);
    for (long l = 0, o = 0; l < L; ++l) goff[l] = o, o += (long)n.F(l) * n.K(l) + n.F(l);
    for (long r = 0; r < N; ++r) {
        std::vector<double> dz(n.out_dim);
        for (int f = 0; f < n.out_dim; ++f) {
            const double o = sout[r * n.out_dim + f];
            dz[f] = gout[r * n.out_dim + f] * (n.use_tanh ? 1.0 - o * o : 1.0);
        }
        for (int l = L - 1; l >= 0; --l) {
            const int kh = l > 0 ? n.hidden : 0, K = n.K(l);
            const float* hp = l > 0 ? sh + ((size_t)(l - 1) * N + r) * n.hidden : nullptr;
            for (int f = 0; f < n.F(l); ++f) {
                for (int k = 0; k < K; ++k) want[goff[l] + (long)f * K + k] += dz[f] * (k < kh ? hp[k] : senc[r * E + k - kh]);
                want[goff[l] + (long)n.F(l) * K + f] += dz[f];
            }
            if (l == 0) break;
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
        const long K = n.K(l), nw = (long)n.F(l) * K;
        for (int part = 0; part < 2; ++part) {                                                // weight, then bias: one tensor each
            const long o = goff[l] + (part ? nw : 0), cnt = part ? n.F(l) : nw;
            double mx = 0, diff = 0;
            for (long i = 0; i < cnt; ++i) mx = fmax(mx, fabs(want[o + i])), diff = fmax(diff, fabs(want[o + i] - grad[o + i]));
            if (mx > 0) e_bwd = fmax(e_bwd, diff / mx);
            ok = ok && (mx > 0 || diff == 0);
        }
    }
    // sums of at most 513 fp32 products per element, dZ through at most four fp32 layers, relative to the tensor's largest
    // element: about 1e-6; a dropped row, a wrong mask or a wrong column gives O(1e-2) and more
    ok = ok && e_bwd <= 2e-5;
    char name[160];
    snprintf(name, sizeof(name), "atlas_fit in %d pe %d hidden %d layers %d skip 0x%x out %d tanh %d N=%ld", n.in_dim, n.pe_dim, n.hidden,
             n.layers, n.skip_mask, n.out_dim, n.use_tanh, N);
    verdict(name, ok, e_fwd, e_bwd);
}

static void run_refusals() {
    const Net n{3, 2, 32, 3, 0, 0, 1};
    const long N = 5;
    int64_t sf = 0, scf = 0, gf = 0;
    bool ok = vsx_coord_mlp_train_workspace(N, 3, 2, 32, 3, 0, 0, 0, 0, &sf, &scf, &gf) == VSX_OK;
    std::vector<std::vector<float>> W(3), B(3);
    for (int l = 0; l < 3; ++l) W[l].assign((size_t)n.F(l) * n.K(l), 0.25f), B[l].assign(n.F(l), 0.1f);
    Buf packed(pack(n, W, B, nullptr));
    pack(n, W, B, packed.p);
    Buf x(N * 3, 0.5f), out(N * 2, 55.f), saved((size_t)sf, 55.f), gout(N * 2, 1.f), scratch((size_t)scf, 55.f), grad((size_t)gf, 55.f);
    auto fwd = [&](int64_t hidden, int64_t layers, int64_t pe_type, int64_t mlp_type, int64_t odim, int64_t saved_floats) {
        return vsx_coord_mlp_fwd_train_f32(x.p, N, 3, odim, hidden, layers, pe_type, 0, mlp_type, 0, 1, packed.p, (int64_t)packed.n, out.p,
                                           saved.p, saved_floats, nullptr);
    };
    auto bwd = [&](int64_t hidden, int64_t layers, int64_t pe_type, int64_t mlp_type, int64_t odim, int64_t s, int64_t sc, int64_t g) {
        return vsx_coord_mlp_bwd_f32(gout.p, N, 3, odim, hidden, layers, pe_type, 0, mlp_type, 0, 1, packed.p, (int64_t)packed.n, saved.p, s,
                                     scratch.p, sc, grad.p, g, nullptr);
    };
    // a short buffer: refused, nothing written
    ok = ok && fwd(32, 3, 0, 0, 2, sf - 1) == VSX_E_WORKSPACE;
    ok = ok && bwd(32, 3, 0, 0, 2, sf - 1, scf, gf) == VSX_E_WORKSPACE && bwd(32, 3, 0, 0, 2, sf, scf - 1, gf) == VSX_E_WORKSPACE;
    ok = ok && bwd(32, 3, 0, 0, 2, sf, scf, gf - 1) == VSX_E_WORKSPACE;
    // the options K13 refuses
    ok = ok && fwd(32, 3, 0, 1, 2, sf) == VSX_E_UNSUPPORTED && bwd(32, 3, 0, 1, 2, sf, scf, gf) == VSX_E_UNSUPPORTED;     // tcnn
    ok = ok && fwd(32, 3, 2, 0, 2, sf) == VSX_E_UNSUPPORTED && bwd(32, 3, 2, 0, 2, sf, scf, gf) == VSX_E_UNSUPPORTED;     // hash_encoding
    ok = ok && fwd(48, 3, 0, 0, 2, sf) == VSX_E_UNSUPPORTED && bwd(288, 3, 0, 0, 2, sf, scf, gf) == VSX_E_UNSUPPORTED;
    ok = ok && fwd(32, 9, 0, 0, 2, sf) == VSX_E_UNSUPPORTED && bwd(32, 1, 0, 0, 2, sf, scf, gf) == VSX_E_UNSUPPORTED;
    ok = ok && fwd(32, 3, 0, 0, 4, sf) == VSX_E_UNSUPPORTED && bwd(32, 3, 0, 0, 0, sf, scf, gf) == VSX_E_UNSUPPORTED;
    ok = ok && vsx_coord_mlp_train_workspace(N, 4, 2, 32, 3, 0, 0, 0, 0, &sf, &scf, &gf) == VSX_E_UNSUPPORTED;
    ok = ok && out.all(55.f) && saved.all(55.f) && scratch.all(55.f) && grad.all(55.f);
    ok = ok && vsx_coord_mlp_wgrad_rows() == CMB_ROWS;
    verdict("atlas_fit refusals (nothing is written)", ok, 0.0, 0.0);
}

int main() {
    const long R = (long)vsx_coord_mlp_wgrad_rows();
    const Net nets[] = {
        {3, 1, 32, 2, 0, 0x00, 1},      // two layers, the coordinates themselves
        {2, 3, 64, 3, 2, 0x00, 0},      // 8 encoded columns, linear output
        {3, 3, 32, 5, 3, 0x14, 1},      // 18 encoded columns, skip layers 2 and 4 (the output layer)
        {2, 1, 64, 5, 0, 0x00, 0},
    };
    for (const Net& n : nets)
        for (long N : {0L, 1L, 63L, 64L, 65L, R + 1}) run_case(n, N);
    run_refusals();
    if (n_bad) {
        printf("%d check(s) FAILED\n", n_bad);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
