// K12 — DIFT semantic-point embeddings (extract_semantic_point.py:125-205, dift_util.py:230-267) for gfx950.
//
// The reference upsamples the ensemble-mean feature map [1, 1280, h, w] to full image resolution (nn.Upsample, bilinear,
// align_corners=False) on every query — 1.76 GB of fp32 at 448x768 — and then reads ONE pixel of it per (frame, point),
// or, for the heat map, takes cosine similarities against the whole upsampled map.  Bilinear interpolation is linear, so
// neither needs the upsampled tensor:
//   * vsx_dift_sample_points reads the four low-resolution neighbours of each point straight from the UNet tap's
//     [N, E, h, w, C] fp16 output, averages the E ensemble members in fp32 and interpolates: one wave per (frame, point);
//   * vsx_dift_cosine_map computes, per low-resolution pixel p, the dot products D[p, q] = <F_p, Q_q> and five Gram
//     bands <F_p, F_p'> (p' = p, right, down, down-right, down-left).  A full-resolution pixel's vector is
//     v = sum_i w_i F_i over its 4 taps, so <v, Q_q> = sum_i w_i D[i, q] and |v|^2 = sum_ij w_i w_j <F_i, F_j>, and the
//     full-resolution pass is per-pixel arithmetic on those numbers plus the (optional) store of the map.
#include "common.h"

namespace {

constexpr int DIFT_THREADS = 256;            // 4 waves
constexpr int DIFT_WAVES = DIFT_THREADS / 64;
constexpr int DIFT_BANDS = 5;                // self, right, down, down-right, down-left

// PyTorch's upsample_bilinear2d source index for align_corners=False and no explicit scale:
// src = max((dst + 0.5) * in / out - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), weights (1 - l, l)
struct Tap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Tap src_tap(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    float s = ((float)dst + 0.5f) * scale - 0.5f;
    s = s < 0.f ? 0.f : s;
    int i0 = min((int)s, in - 1);
    const float l1 = s - (float)i0;
    Tap t;
    t.i0 = i0;
    t.i1 = min(i0 + 1, in - 1);
    t.l0 = 1.f - l1;
    t.l1 = l1;
    return t;
}

__device__ __forceinline__ void ld8f(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8f(float* p, const float (&v)[8]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// One wave per (frame n, point p); lanes own 8 consecutive channels per 512-channel stride (16-byte loads of the fp16
// map, 32-byte stores of the fp32 vector).  vec = bilinear(mean_e feat[n, e]) at (y, x); cos against the query.
__global__ __launch_bounds__(DIFT_THREADS) void dift_sample_kernel(
    const half_t* __restrict__ feat, int E, int h, int w, int C, int H, int W, const int* __restrict__ coords, int N,
    int P, const float* __restrict__ query, int q_per_frame, float* __restrict__ vec, float* __restrict__ cosv) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * DIFT_WAVES + (threadIdx.x >> 6);     // n * P + p
    if (item >= (long)N * P) return;
    const int n = (int)(item / P), p = (int)(item % P);
    const int x = coords[item * 2 + 0], y = coords[item * 2 + 1];
    float* out = vec + item * C;
    if (x < 0) {                                                            // skipped point: zeros, cos 0
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = lane * 8; c < C; c += 512) st8f(out + c, z);
        if (cosv && lane == 0) cosv[item] = 0.f;
        return;
    }
    // the host validates 0 <= x < W, 0 <= y < H; the clamp only keeps a bad coordinate inside the map
    const Tap ty = src_tap(max(min(y, H - 1), 0), h, H), tx = src_tap(min(x, W - 1), w, W);
    const float inv_e = 1.f / (float)E;
    const float w00 = ty.l0 * tx.l0 * inv_e, w01 = ty.l0 * tx.l1 * inv_e;
    const float w10 = ty.l1 * tx.l0 * inv_e, w11 = ty.l1 * tx.l1 * inv_e;
    const long img = (long)h * w * C;
    const long o00 = ((long)ty.i0 * w + tx.i0) * C, o01 = ((long)ty.i0 * w + tx.i1) * C;
    const long o10 = ((long)ty.i1 * w + tx.i0) * C, o11 = ((long)ty.i1 * w + tx.i1) * C;
    const half_t* base = feat + (long)n * E * img;
    const float* q = query ? query + (q_per_frame ? item : (long)p) * C : nullptr;
    float dot = 0.f, nv = 0.f, nq = 0.f;
    for (int c = lane * 8; c < C; c += 512) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int e = 0; e < E; ++e) {
            const half_t* im = base + e * img + c;
            const h8 a = as_h8(ld16(im + o00)), b = as_h8(ld16(im + o01));
            const h8 d = as_h8(ld16(im + o10)), f = as_h8(ld16(im + o11));
#pragma unroll
            for (int j = 0; j < 8; ++j)
                acc[j] += w00 * (float)a[j] + w01 * (float)b[j] + w10 * (float)d[j] + w11 * (float)f[j];
        }
        st8f(out + c, acc);
        if (q) {
            float qv[8];
            ld8f(q + c, qv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                dot += acc[j] * qv[j];
                nv += acc[j] * acc[j];
                nq += qv[j] * qv[j];
            }
        }
    }
    if (cosv) {
        dot = wave_sum(dot);
        nv = wave_sum(nv);
        nq = wave_sum(nq);
        if (lane == 0) cosv[item] = q ? dot / fmaxf(sqrtf(nv) * sqrtf(nq), 1e-8f) : 0.f;
    }
}

// [N, E, h, w, C] fp16 -> [N, h, w, C] fp32 ensemble mean; one thread per 8 channels of one pixel
__global__ __launch_bounds__(DIFT_THREADS) void dift_mean_kernel(const half_t* __restrict__ feat, int E, long pix,
                                                                 int C, float* __restrict__ mean, long n8) {
    const long i = (long)blockIdx.x * DIFT_THREADS + threadIdx.x;          // (n * pix + s) * C/8 + c8
    if (i >= n8) return;
    const int c8 = C / 8;
    const long ns = i / c8;
    const long n = ns / pix, s = ns % pix;
    const long c = (i % c8) * 8;
    const half_t* src = feat + (n * E * pix + s) * C + c;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < E; ++e) {
        const h8 v = as_h8(ld16(src + (long)e * pix * C));
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
    }
    const float inv_e = 1.f / (float)E;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= inv_e;
    st8f(mean + ns * C + c, acc);
}

// One wave per (frame n, low-res pixel (yy, xx)): bands[n, pix, 0..4] = <F_p, F_p'> for p' = p, right, down, down-right,
// down-left (0 where p' is outside the map; the full-resolution pass never reads those), bands[n, pix, 5 + q] = <F_p, Q_q>.
// ~(5 + Q) * C FMAs per pixel: 1344 pixels x 21 x 1280 = 36 MFLOP at 28x48, Q = 16 — VALU dot products against an
// L2-resident map, far below the cost of one launch of the UNet that produced it.
__global__ __launch_bounds__(DIFT_THREADS) void dift_bands_kernel(const float* __restrict__ mean, int N, int h, int w,
                                                                  int C, const float* __restrict__ query, int Q,
                                                                  int q_per_frame, float* __restrict__ bands) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * DIFT_WAVES + (threadIdx.x >> 6);     // n * h * w + pix
    const long pix = (long)h * w;
    if (item >= (long)N * pix) return;
    const int n = (int)(item / pix);
    const int s = (int)(item % pix);
    const int yy = s / w, xx = s % w;
    const float* f = mean + item * C;
    const bool r = xx + 1 < w, d = yy + 1 < h, l = xx > 0;
    const float* fr = f + C;
    const float* fd = f + (long)w * C;
    const float* fdr = fd + C;
    const float* fdl = fd - C;
    float g[DIFT_BANDS] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = lane * 8; c < C; c += 512) {
        float a[8], b[8];
        ld8f(f + c, a);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[0] += a[j] * a[j];
        if (r) {
            ld8f(fr + c, b);
#pragma unroll
            for (int j = 0; j < 8; ++j) g[1] += a[j] * b[j];
        }
        if (d) {
            ld8f(fd + c, b);
#pragma unroll
            for (int j = 0; j < 8; ++j) g[2] += a[j] * b[j];
            if (r) {
                ld8f(fdr + c, b);
#pragma unroll
                for (int j = 0; j < 8; ++j) g[3] += a[j] * b[j];
            }
            if (l) {
                ld8f(fdl + c, b);
#pragma unroll
                for (int j = 0; j < 8; ++j) g[4] += a[j] * b[j];
            }
        }
    }
    float* out = bands + item * (DIFT_BANDS + Q);
#pragma unroll
    for (int k = 0; k < DIFT_BANDS; ++k) {
        const float v = wave_sum(g[k]);
        if (lane == 0) out[k] = v;
    }
    const float* qb = query + (q_per_frame ? (long)n * Q * C : 0);
    for (int qi = 0; qi < Q; ++qi) {
        float dq = 0.f;
        for (int c = lane * 8; c < C; c += 512) {
            float a[8], b[8];
            ld8f(f + c, a);
            ld8f(qb + (long)qi * C + c, b);
#pragma unroll
            for (int j = 0; j < 8; ++j) dq += a[j] * b[j];
        }
        dq = wave_sum(dq);
        if (lane == 0) out[DIFT_BANDS + qi] = dq;
    }
}

// float -> uint32 whose unsigned order is the float order (no NaNs on this path)
__device__ __forceinline__ unsigned ordered_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// grid (ceil(H*W / 256), Q, N); one thread per full-resolution pixel.  The argmax key of a pixel is
// (ordered cos << 32) | (~index): the largest key is the largest value, the first in row-major order among equal values
// (np.unravel_index(argmax)); a block reduces its keys in registers / LDS and issues ONE 64-bit atomic max.
__global__ __launch_bounds__(DIFT_THREADS) void dift_cosmap_kernel(const float* __restrict__ bands, int h, int w, int H,
                                                                   int W, int C, const float* __restrict__ query, int Q,
                                                                   int q_per_frame, float* __restrict__ cos_map,
                                                                   unsigned long long* __restrict__ keys) {
    __shared__ float red[DIFT_WAVES];
    __shared__ unsigned long long kred[DIFT_WAVES];
    const int qi = blockIdx.y, n = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // |Q_q|^2, one block-wide reduction
    const float* qv = query + ((q_per_frame ? (long)n * Q : 0) + qi) * C;
    float nq = 0.f;
    for (int c = threadIdx.x; c < C; c += DIFT_THREADS) nq += qv[c] * qv[c];
    nq = wave_sum(nq);
    if (lane == 0) red[wave] = nq;
    __syncthreads();
    nq = 0.f;
#pragma unroll
    for (int k = 0; k < DIFT_WAVES; ++k) nq += red[k];
    const float qnorm = sqrtf(nq);

    const long idx = (long)blockIdx.x * DIFT_THREADS + threadIdx.x;
    unsigned long long key = 0ull;
    if (idx < (long)H * W) {
        const int y = (int)(idx / W), x = (int)(idx % W);
        const Tap ty = src_tap(y, h, H), tx = src_tap(x, w, W);
        const int st = DIFT_BANDS + Q;
        const float* b00 = bands + (((long)n * h + ty.i0) * w + tx.i0) * st;
        const float* b01 = bands + (((long)n * h + ty.i0) * w + tx.i1) * st;
        const float* b10 = bands + (((long)n * h + ty.i1) * w + tx.i0) * st;
        const float* b11 = bands + (((long)n * h + ty.i1) * w + tx.i1) * st;
        const bool dx = tx.i1 > tx.i0, dy = ty.i1 > ty.i0;
        const float w00 = ty.l0 * tx.l0, w01 = ty.l0 * tx.l1, w10 = ty.l1 * tx.l0, w11 = ty.l1 * tx.l1;
        const float dot = w00 * b00[DIFT_BANDS + qi] + w01 * b01[DIFT_BANDS + qi] + w10 * b10[DIFT_BANDS + qi] +
                          w11 * b11[DIFT_BANDS + qi];
        // Gram entries of the tap pairs; a clamped tap coincides with its neighbour (the pair is then the self band)
        const float s00 = b00[0], s01 = b01[0], s10 = b10[0], s11 = b11[0];
        const float g0001 = dx ? b00[1] : s00;                              // (y0,x0)-(y0,x1)
        const float g1011 = dx ? b10[1] : s10;                              // (y1,x0)-(y1,x1)
        const float g0010 = dy ? b00[2] : s00;                              // (y0,x0)-(y1,x0)
        const float g0111 = dy ? b01[2] : s01;                              // (y0,x1)-(y1,x1)
        const float g0011 = dx ? (dy ? b00[3] : b00[1]) : (dy ? b00[2] : s00);   // (y0,x0)-(y1,x1)
        const float g0110 = dx ? (dy ? b01[4] : b00[1]) : (dy ? b00[2] : s00);   // (y0,x1)-(y1,x0)
        float nv = w00 * w00 * s00 + w01 * w01 * s01 + w10 * w10 * s10 + w11 * w11 * s11 +
                   2.f * (w00 * w01 * g0001 + w10 * w11 * g1011 + w00 * w10 * g0010 + w01 * w11 * g0111 +
                          w00 * w11 * g0011 + w01 * w10 * g0110);
        nv = fmaxf(nv, 0.f);
        const float cv = dot / fmaxf(sqrtf(nv) * qnorm, 1e-8f);
        if (cos_map) cos_map[((long)n * Q + qi) * H * W + idx] = cv;
        key = ((unsigned long long)ordered_bits(cv) << 32) | (unsigned long long)(0xffffffffu - (unsigned)idx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if (lane == 0) kred[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long best = kred[0];
#pragma unroll
        for (int k = 1; k < DIFT_WAVES; ++k) best = kred[k] > best ? kred[k] : best;
        if (best) atomicMax(keys + (long)n * Q + qi, best);
    }
}

__global__ void dift_argmax_kernel(const unsigned long long* __restrict__ keys, long nq, int W, int* __restrict__ yx,
                                   float* __restrict__ val) {
    const long i = (long)blockIdx.x * DIFT_THREADS + threadIdx.x;
    if (i >= nq) return;
    const unsigned long long k = keys[i];
    const unsigned idx = 0xffffffffu - (unsigned)(k & 0xffffffffull);
    yx[i * 2 + 0] = (int)(idx / (unsigned)W);
    yx[i * 2 + 1] = (int)(idx % (unsigned)W);
    val[i] = from_ordered_bits((unsigned)(k >> 32));
}

inline unsigned blocks_of(long n, long per) { return (unsigned)((n + per - 1) / per); }

// workspace layout: keys [N*Q] u64 | mean [N*h*w*C] f32 | bands [N*h*w*(5+Q)] f32, each 256-byte aligned
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" int vsx_dift_sample_points(const void* feat, int64_t N, int64_t E, int64_t h, int64_t w, int64_t C, int64_t H,
                                      int64_t W, const int32_t* coords, int64_t P, const float* query,
                                      int64_t query_per_frame, float* vec, float* cos_out, vsx_stream_t stream) {
    VSX_REQUIRE(feat && coords && vec, VSX_E_BADSHAPE, "dift_sample_points: null argument");
    VSX_REQUIRE(N > 0 && E > 0 && h > 0 && w > 0 && H > 0 && W > 0 && P >= 0 && C > 0 && C % 8 == 0, VSX_E_BADSHAPE,
                "dift_sample_points: bad sizes (C must be a multiple of 8)");
    VSX_REQUIRE(H * W < (1ll << 31) && N * P < (1ll << 31), VSX_E_BADSHAPE, "dift_sample_points: too large");
    VSX_REQUIRE(vsx_aligned16(feat) && vsx_aligned16(vec) && (!query || vsx_aligned16(query)), VSX_E_BADSHAPE,
                "dift_sample_points: feat / vec / query must be 16-byte aligned");
    VSX_REQUIRE(!cos_out || query, VSX_E_BADSHAPE, "dift_sample_points: cos needs query vectors");
    if (N * P == 0) return VSX_OK;
    hipLaunchKernelGGL(dift_sample_kernel, dim3(blocks_of(N * P, DIFT_WAVES)), dim3(DIFT_THREADS), 0,
                       (hipStream_t)stream, (const half_t*)feat, (int)E, (int)h, (int)w, (int)C, (int)H, (int)W,
                       (const int*)coords, (int)N, (int)P, query, (int)(query_per_frame != 0), vec, cos_out);
    return vsx_check_launch("vsx_dift_sample_points");
}

extern "C" int64_t vsx_dift_cosine_map_workspace(int64_t N, int64_t h, int64_t w, int64_t C, int64_t Q) {
    if (N <= 0 || h <= 0 || w <= 0 || C <= 0 || Q <= 0) return 0;
    return align256(N * Q * 8) + align256(N * h * w * C * 4) + align256(N * h * w * (DIFT_BANDS + Q) * 4);
}

extern "C" int vsx_dift_cosine_map(const void* feat, int64_t N, int64_t E, int64_t h, int64_t w, int64_t C, int64_t H,
                                   int64_t W, const float* query, int64_t Q, int64_t query_per_frame, void* workspace,
                                   int64_t workspace_bytes, float* cos_map, int32_t* argmax_yx, float* argmax_val,
                                   vsx_stream_t stream) {
    VSX_REQUIRE(feat && query && workspace && argmax_yx && argmax_val, VSX_E_BADSHAPE, "dift_cosine_map: null argument");
    VSX_REQUIRE(N > 0 && E > 0 && h > 0 && w > 0 && H > 0 && W > 0 && Q > 0 && C > 0 && C % 8 == 0, VSX_E_BADSHAPE,
                "dift_cosine_map: bad sizes (C must be a multiple of 8)");
    VSX_REQUIRE(H * W < (1ll << 31) && Q <= 65535 && N <= 65535, VSX_E_BADSHAPE, "dift_cosine_map: too large");
    VSX_REQUIRE(vsx_aligned16(feat) && vsx_aligned16(query) && vsx_aligned16(workspace), VSX_E_BADSHAPE,
                "dift_cosine_map: feat / query / workspace must be 16-byte aligned");
    const int64_t need = vsx_dift_cosine_map_workspace(N, h, w, C, Q);
    VSX_REQUIRE(workspace_bytes >= need, VSX_E_WORKSPACE, "dift_cosine_map: workspace %lld bytes < %lld",
                (long long)workspace_bytes, (long long)need);
    char* ws = (char*)workspace;
    unsigned long long* keys = (unsigned long long*)ws;
    float* mean = (float*)(ws + align256(N * Q * 8));
    float* bands = (float*)(ws + align256(N * Q * 8) + align256(N * h * w * C * 4));
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(keys, 0, (size_t)(N * Q * 8), s) != hipSuccess)
        return vsx_fail(VSX_E_LAUNCH, "dift_cosine_map: hipMemsetAsync failed");
    const long pix = (long)h * w;
    const long n8 = N * pix * (C / 8);
    hipLaunchKernelGGL(dift_mean_kernel, dim3(blocks_of(n8, DIFT_THREADS)), dim3(DIFT_THREADS), 0, s,
                       (const half_t*)feat, (int)E, pix, (int)C, mean, n8);
    int rc = vsx_check_launch("vsx_dift_cosine_map (mean)");
    if (rc) return rc;
    hipLaunchKernelGGL(dift_bands_kernel, dim3(blocks_of(N * pix, DIFT_WAVES)), dim3(DIFT_THREADS), 0, s, mean, (int)N,
                       (int)h, (int)w, (int)C, query, (int)Q, (int)(query_per_frame != 0), bands);
    rc = vsx_check_launch("vsx_dift_cosine_map (bands)");
    if (rc) return rc;
    hipLaunchKernelGGL(dift_cosmap_kernel, dim3(blocks_of(H * W, DIFT_THREADS), (unsigned)Q, (unsigned)N),
                       dim3(DIFT_THREADS), 0, s, bands, (int)h, (int)w, (int)H, (int)W, (int)C, query, (int)Q,
                       (int)(query_per_frame != 0), cos_map, keys);
    rc = vsx_check_launch("vsx_dift_cosine_map (map)");
    if (rc) return rc;
    hipLaunchKernelGGL(dift_argmax_kernel, dim3(blocks_of(N * Q, DIFT_THREADS)), dim3(DIFT_THREADS), 0, s, keys,
                       (long)(N * Q), (int)W, (int*)argmax_yx, argmax_val);
    return vsx_check_launch("vsx_dift_cosine_map (argmax)");
}
