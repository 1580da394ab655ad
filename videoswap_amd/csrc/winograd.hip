// Winograd F(2x2, 3x3) form of the stride-1 3x3 convolution (Lavin & Gray, "Fast Algorithms for Convolutional Neural
// Networks", 2015) for gfx950: a 2 x 2 output tile from a 4 x 4 input window with 16 multiplications per (input channel,
// output channel) instead of 36.
//
//   V[xi][tile][c]  = (B^T d B)[xi]        input transform   (this file; byte-bound)
//   Mt[xi][tile][n] = sum_c V[xi][tile][c] U[xi][n][c]       16 independent GEMMs = ONE batched vsx_gemm_f16 launch
//   Y[2x2][n]       = A^T Mt A  (+ bias, + row vector, + residual)   output transform (this file; byte-bound)
//
// tile = (image, i / 2, j / 2); d is the 4 x 4 window at (2 ti - 1, 2 tj - 1) of the zero-padded image; xi = 4 a + b runs over
// the transformed window.  U = G g G^T is made once per weight by the caller (videoswap_amd.ops.winograd_weights).
// Every transform is fp32 arithmetic on fp16 data with ONE rounding to fp16 (V, U, Mt, Y).  Layout is channels-last; a
// thread owns one 16-byte channel octet of one tile, like the GroupNorm kernels, so consecutive lanes read and write
// consecutive 16-byte pieces.  No LDS, no MFMA, no atomics: tools/cpu_check/check_winograd.cpp runs this file unmodified.
//
//   B^T = | 1  0 -1  0 |     G = | 1    0    0  |     A^T = | 1  1  1  0 |
//         | 0  1  1  0 |         | 1/2  1/2  1/2|           | 0  1 -1 -1 |
//         | 0 -1  1  0 |         | 1/2 -1/2  1/2|
//         | 0  1  0 -1 |         | 0    0    1  |
#include "common.h"
#include "options.h"

namespace {

constexpr int WG_THREADS = 256;

struct WinoIn {
    const half_t* A;        // [nimg, H, W, C1]
    const half_t* A2;       // [nimg, H, W, C2] or null
    half_t* V;              // [16][tiles][C1 + C2]
    int H, W, C1, C2, th, tw;
    long tiles;             // nimg * th * tw
};

struct WinoOut {
    const half_t* Mt;       // [16][tiles][N]
    half_t* Y;              // [nimg * H * W] rows of ldc
    const half_t* bias;     // [N] or null
    const half_t* rowvec;   // [ceil(M / rows_per_vec), N] or null
    const half_t* residual; // rows of ldr, or null
    long rows_per_vec, ldc, ldr;
    int H, W, N, th, tw;
    long tiles;
};

__global__ __launch_bounds__(WG_THREADS) void wino_input_kernel(const WinoIn p) {
    const int C = p.C1 + p.C2, octs = C >> 3;
    const long gid = (long)blockIdx.x * WG_THREADS + threadIdx.x;
    const long tile = gid / octs;
    if (tile >= p.tiles) return;
    const int c = (int)(gid - tile * octs) << 3;
    const int per_img = p.th * p.tw;
    const long img = tile / per_img;
    const int r = (int)(tile - img * per_img);
    const int ti = r / p.tw, tj = r - ti * p.tw;
    // an octet never straddles the two sources: C1 is a multiple of 8
    const half_t* src = c < p.C1 ? p.A + c : p.A2 + (c - p.C1);
    const int cs = c < p.C1 ? p.C1 : p.C2;
    src += img * (long)p.H * p.W * cs;
    h8 d[16];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int y = 2 * ti - 1 + a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int x = 2 * tj - 1 + b;
            const bool in = y >= 0 && y < p.H && x >= 0 && x < p.W;
            d[4 * a + b] = in ? as_h8(ld16(src + ((long)y * p.W + x) * cs)) : h8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    h8 v[16];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float t[16];
#pragma unroll
        for (int b = 0; b < 4; ++b) {               // B^T d: down the columns
            const float d0 = (float)d[b][e], d1 = (float)d[4 + b][e], d2 = (float)d[8 + b][e], d3 = (float)d[12 + b][e];
            t[b] = d0 - d2;
            t[4 + b] = d1 + d2;
            t[8 + b] = d2 - d1;
            t[12 + b] = d1 - d3;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {               // (B^T d) B: along the rows
            const float t0 = t[4 * a], t1 = t[4 * a + 1], t2 = t[4 * a + 2], t3 = t[4 * a + 3];
            v[4 * a][e] = (half_t)(t0 - t2);
            v[4 * a + 1][e] = (half_t)(t1 + t2);
            v[4 * a + 2][e] = (half_t)(t2 - t1);
            v[4 * a + 3][e] = (half_t)(t1 - t3);
        }
    }
    const long xi_stride = p.tiles * C;
    half_t* out = p.V + tile * C + c;
#pragma unroll
    for (int k = 0; k < 16; ++k) st16(out + k * xi_stride, as_u4(v[k]));
}

__global__ __launch_bounds__(WG_THREADS) void wino_output_kernel(const WinoOut p) {
    const int octs = p.N >> 3;
    const long gid = (long)blockIdx.x * WG_THREADS + threadIdx.x;
    const long tile = gid / octs;
    if (tile >= p.tiles) return;
    const int n = (int)(gid - tile * octs) << 3;
    const int per_img = p.th * p.tw;
    const long img = tile / per_img;
    const int r = (int)(tile - img * per_img);
    const int ti = r / p.tw, tj = r - ti * p.tw;
    const long xi_stride = p.tiles * p.N;
    const half_t* in = p.Mt + tile * p.N + n;
    h8 m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = as_h8(ld16(in + k * xi_stride));
    float y[4][8];                                  // [2 pi + pj][channel]
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float s[8];                                 // A^T Mt: [2][4]
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float m0 = (float)m[b][e], m1 = (float)m[4 + b][e], m2 = (float)m[8 + b][e], m3 = (float)m[12 + b][e];
            s[b] = m0 + m1 + m2;
            s[4 + b] = m1 - m2 - m3;
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            y[2 * a][e] = s[4 * a] + s[4 * a + 1] + s[4 * a + 2];
            y[2 * a + 1][e] = s[4 * a + 1] - s[4 * a + 2] - s[4 * a + 3];
        }
    }
    h8 bias = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p.bias) bias = as_h8(ld16(p.bias + n));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long row = (img * p.H + (2 * ti + (q >> 1))) * p.W + 2 * tj + (q & 1);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = y[q][e];
        // the direct path's epilogue order: + bias, + row vector, + residual last, one rounding
        if (p.bias) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += (float)bias[e];
        }
        if (p.rowvec) {
            const h8 b = as_h8(ld16(p.rowvec + (row / p.rows_per_vec) * p.N + n));
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += (float)b[e];
        }
        if (p.residual) {
            const h8 b = as_h8(ld16(p.residual + row * p.ldr + n));
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += (float)b[e];
        }
        h8 pk;
#pragma unroll
        for (int e = 0; e < 8; ++e) pk[e] = (half_t)o[e];
        st16(p.Y + row * p.ldc + n, as_u4(pk));
    }
}

// The descriptions this form takes (include/vsx.h).  `why` names the first condition that fails.
bool wino_supported(const vsx_gemm_desc* d, const char** why) {
    auto no = [&](const char* w) { *why = w; return false; };
    if (!d) return no("null descriptor");
    if (d->a_mode != 1 || d->ks != 3 || d->stride != 1 || d->upsample != 0) return no("a stride-1 3x3 convolution without upsampling only");
    if (!((d->pad_lo < 0 && d->pad_hi < 0) || (d->pad_lo == 1 && d->pad_hi == 1))) return no("symmetric padding 1 only");
    if (d->batch0 != 1 || d->batch1 != 1) return no("no batch");
    if (d->H <= 0 || d->W <= 0 || d->H % 2 || d->W % 2) return no("H and W must be even");
    if (d->C1 <= 0 || d->C1 % 8 || d->C2 < 0 || d->C2 % 8) return no("channel counts must be multiples of 8");
    if ((d->C2 == 0) != (d->A2 == nullptr)) return no("A2 / C2 mismatch");
    if (d->C2 && (d->C1 % 64 || d->C2 % 64)) return no("two sources need channel counts that are multiples of 64");
    if (d->N <= 0 || d->N % 8 || d->K != 9 * (d->C1 + d->C2)) return no("N must be a multiple of 8 and K = 9 (C1 + C2)");
    if (d->M <= 0 || d->M % (d->H * d->W)) return no("M must be a positive multiple of H * W");
    if (d->geglu || d->c_mode != 0 || d->rowscale || d->colvec || d->rowstats) return no("epilogue = bias / rowvec / residual only");
    if (d->alpha != 1.0) return no("alpha must be 1");
    if (d->ldc % 8 || d->ldc < d->N || (d->residual && (d->ldr % 8 || d->ldr < d->N))) return no("ldc / ldr must be multiples of 8, at least N");
    if (d->rowvec && d->rows_per_vec <= 0) return no("rows_per_vec");
    if (d->M * d->ldc >= (1L << 31) || d->M * d->ldr >= (1L << 31) || d->M * (d->C1 + d->C2) >= (1L << 31))
        return no("M * ldc, M * ldr and M * (C1 + C2) must be below 2^31 elements");
    return true;
}

}  // namespace

// bytes of workspace vsx_conv3x3_winograd_f16(d) needs (V then Mt); 0: d is not supported
extern "C" int64_t vsx_conv3x3_winograd_workspace(const vsx_gemm_desc* d) {
    const char* why;
    if (!wino_supported(d, &why)) return 0;
    return 16 * (d->M / 4) * (d->C1 + d->C2 + d->N) * (int64_t)sizeof(half_t);
}

// The choice under option "conv_winograd" = 1 (auto): the shapes where the three launches measured faster than the direct
// kernels at one and at two clips per step by more than either's spread (profiles/winograd_ab.txt: the 16 x 16 and 8 x 8 levels
// from 640 input channels, the 32 x 32 level from 1280), and no forced back end.  The only statement of the rule: videoswap_amd.ops.conv2d asks here.
extern "C" int64_t vsx_conv3x3_winograd_auto(const vsx_gemm_desc* d) {
    const char* why;
    const long mode = vsxg::gemm_option("conv_winograd");
    if (mode == 0 || !wino_supported(d, &why)) return 0;
    if (mode >= 2) return 1;
    if (vsxg::gemm_option("gemm_pp") != 1 || vsxg::gemm_option("tile_tune") != 0) return 0;
    const long cin = d->C1 + d->C2, pix = d->H * d->W;
    return (cin >= 640 && pix <= 256) || (cin >= 1280 && pix <= 1024) ? 1 : 0;
}

extern "C" int vsx_conv3x3_winograd_f16(const vsx_gemm_desc* d, const void* U, void* workspace, int64_t workspace_bytes,
                                        vsx_stream_t stream) {
    const char* why = "";
    VSX_REQUIRE(wino_supported(d, &why), VSX_E_UNSUPPORTED, "conv3x3_winograd: %s", why);
    VSX_REQUIRE(d->A && d->C && U && workspace, VSX_E_BADSHAPE, "conv3x3_winograd: null argument");
    VSX_REQUIRE(vsx_aligned16(d->A) && vsx_aligned16(d->A2) && vsx_aligned16(d->C) && vsx_aligned16(U) && vsx_aligned16(workspace) &&
                    vsx_aligned16(d->bias) && vsx_aligned16(d->rowvec) && vsx_aligned16(d->residual),
                VSX_E_BADSHAPE, "conv3x3_winograd: every pointer must be 16-byte aligned");
    VSX_REQUIRE(workspace_bytes >= vsx_conv3x3_winograd_workspace(d), VSX_E_WORKSPACE,
                "conv3x3_winograd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)vsx_conv3x3_winograd_workspace(d));
    const long C = d->C1 + d->C2, tiles = d->M / 4;
    half_t* V = (half_t*)workspace;
    half_t* Mt = V + 16 * tiles * C;
    hipStream_t s = (hipStream_t)stream;

    WinoIn pi;
    pi.A = (const half_t*)d->A;
    pi.A2 = (const half_t*)d->A2;
    pi.V = V;
    pi.H = (int)d->H; pi.W = (int)d->W; pi.C1 = (int)d->C1; pi.C2 = (int)d->C2;
    pi.th = (int)(d->H / 2); pi.tw = (int)(d->W / 2);
    pi.tiles = tiles;
    const long nin = tiles * (C / 8);
    hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)((nin + WG_THREADS - 1) / WG_THREADS)), dim3(WG_THREADS), 0, s, pi);
    int rc = vsx_check_launch("vsx_conv3x3_winograd_f16 (input transform)");
    if (rc != VSX_OK) return rc;

    vsx_gemm_desc g = {};                                      // 16 plain GEMMs [tiles, C] x [N, C]^T, no epilogue
    g.M = tiles; g.N = d->N; g.K = C;
    g.batch0 = 16; g.batch1 = 1;
    g.A = V; g.lda = C; g.a_bs0 = tiles * C;
    g.B = U; g.ldb = C; g.b_bs0 = d->N * C;
    g.C = Mt; g.ldc = d->N; g.c_bs0 = tiles * d->N;
    g.alpha = 1.0;
    g.pad_lo = g.pad_hi = -1;
    rc = vsx_gemm_f16(&g, stream);
    if (rc != VSX_OK) return rc;

    WinoOut po;
    po.Mt = Mt;
    po.Y = (half_t*)d->C;
    po.bias = (const half_t*)d->bias;
    po.rowvec = (const half_t*)d->rowvec;
    po.residual = (const half_t*)d->residual;
    po.rows_per_vec = d->rowvec ? d->rows_per_vec : 1;
    po.ldc = d->ldc; po.ldr = d->ldr;
    po.H = (int)d->H; po.W = (int)d->W; po.N = (int)d->N;
    po.th = pi.th; po.tw = pi.tw;
    po.tiles = tiles;
    const long nout = tiles * (d->N / 8);
    hipLaunchKernelGGL(wino_output_kernel, dim3((unsigned)((nout + WG_THREADS - 1) / WG_THREADS)), dim3(WG_THREADS), 0, s, po);
    return vsx_check_launch("vsx_conv3x3_winograd_f16 (output transform)");
}
