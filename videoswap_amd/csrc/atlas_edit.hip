// K15 — editing a video through its atlas (videoswap/atlas/evaluate.py: get_colors :64-85, bilinear_interpolate_numpy
// :24-45, the mask lines :373-397 and the composition :399-404) for gfx950.
//
// A row is one video pixel that has been through FG_UV_Mapping, BG_UV_Mapping and F_Alpha.  Per layer the kernel turns
// the network's (u, v) into a position on a discrete texture image, reads the four surrounding texels, and composes the
// edited foreground, the edited background and their blend; optionally it marks the texels a row touched in two mask
// images.  ONE launch, one thread per row: ~60 B of streaming traffic per row plus four gathers per layer from a texture
// that stays in L2 / MALL.  No float atomic: the masks take an unsigned integer max on the float's bits (alpha > 0), so
// every output is independent of the order in which rows arrive.
//
// The position arithmetic restates the reference's fp32 tensor operations one rounding at a time: a row is relevant or
// not by a comparison on that position, so the file is compiled without contraction of a product and a sum into an FMA.
// Plain scalar loads and stores only (no vector types, no MFMA): tools/cpu_check runs this file unmodified on the host.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AE_THREADS = 256;

struct AeLayer {
    const float* tex;       // [R, R, C]
    const float* base;      // [N, 3], read when C == 4
    unsigned* mask;         // [R, R] fp32 seen as bits, or null
    float minx, miny, pixel_size, shift;
    int R;
};

struct AeParams {
    const float* uv_fg;     // [N, 2]
    const float* uv_bg;     // [N, 2]
    const float* alpha;     // [N]
    long N;
    AeLayer fg, bg;
    float* edit;            // [N, 3]
    float* out_fg;          // [N, 3]
    float* out_bg;          // [N, 3]
    unsigned char* relevant;
};

__device__ __forceinline__ int ae_clamp(int v, int top) { return v < 0 ? 0 : (v > top ? top : v); }

// -> relevant; rgb = the layer's colour, cell = the four mask cells (floor / ceil of y, floor / ceil of x) as offsets.
// A row that is not relevant (outside the image, NaN, +-inf, +-1e30) returns before any conversion to an integer: a
// relevant row has 0 <= floor <= ceil <= R - 1 in both coordinates, and every index is clamped on top of that.
template <int C>
__device__ __forceinline__ bool ae_sample(const AeLayer& L, const float* __restrict__ uv, long row, float (&rgb)[3],
                                          int (&cell)[4]) {
    const float u = uv[2 * row], v = uv[2 * row + 1];
    const float qx = u * 0.5f + L.shift, qy = v * 0.5f + L.shift;
    const float px = (qx - L.minx) * L.pixel_size, py = (qy - L.miny) * L.pixel_size;   // pixel_size of the x extent for both
    const float fx = floorf(px), fy = floorf(py), cx = ceilf(px), cy = ceilf(py);
    const float edge = (float)L.R;
    if (!(fx >= 0.f && fy >= 0.f && cx < edge && cy < edge)) return false;             // false for NaN as well
    const int top = L.R - 1;
    const int x0 = ae_clamp((int)fx, top), x1 = ae_clamp((int)fx + 1, top);
    const int y0 = ae_clamp((int)fy, top), y1 = ae_clamp((int)fy + 1, top);
    // weights from the CLIPPED corners: px == R - 1 gives x0 == x1 and a zero colour (the reference's behaviour)
    const float wx1 = (float)x1 - px, wx0 = px - (float)x0, wy1 = (float)y1 - py, wy0 = py - (float)y0;
    const float wa = wx1 * wy1, wb = wx1 * wy0, wc = wx0 * wy1, wd = wx0 * wy0;
    const float* ta = L.tex + (y0 * L.R + x0) * C;
    const float* tb = L.tex + (y1 * L.R + x0) * C;
    const float* tc = L.tex + (y0 * L.R + x1) * C;
    const float* td = L.tex + (y1 * L.R + x1) * C;
    float col[C];
#pragma unroll
    for (int k = 0; k < C; ++k) col[k] = ta[k] * wa + tb[k] * wb + tc[k] * wc + td[k] * wd;
    if constexpr (C == 4) {                                                             // RGBA overlay over the neural colour
        const float a = col[3], na = 1.f - col[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = col[k] * a + L.base[3 * row + k] * na;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = col[k];
    }
    const int xf = ae_clamp((int)fx, top), xc = ae_clamp((int)cx, top), yf = ae_clamp((int)fy, top), yc = ae_clamp((int)cy, top);
    cell[0] = yc * L.R + xc;
    cell[1] = yf * L.R + xf;
    cell[2] = yf * L.R + xc;
    cell[3] = yc * L.R + xf;
    return true;
}

// A mask word only grows, so a row that finds it at or above its own value has nothing to do: whatever is there later
// is at least what was read.  The read is served by L2 (agent scope), where the atomics land; rows that map to texels
// other rows have marked already (most of them: a frame covers far fewer texels than it has pixels) skip the atomic.
__device__ __forceinline__ void ae_raise(unsigned* word, unsigned bits) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) atomicMax(word, bits);
}

template <int CF, int CB>
__global__ __launch_bounds__(AE_THREADS) void atlas_edit_kernel(const AeParams p) {
    const long row = (long)blockIdx.x * AE_THREADS + threadIdx.x;
    if (row >= p.N) return;                                    // rows past N are not stored
    const float alpha = p.alpha[row];
    float cf[3] = {0.f, 0.f, 0.f}, cb[3] = {0.f, 0.f, 0.f};
    int cellf[4], cellb[4];
    const bool rf = ae_sample<CF>(p.fg, p.uv_fg, row, cf, cellf);
    const bool rb = ae_sample<CB>(p.bg, p.uv_bg, row, cb, cellb);
    const float na = 1.0f - alpha;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = rf ? cf[k] * alpha : 0.f;
        const float b = rb ? cb[k] : 0.f;
        const float t = rb ? cb[k] * na : 0.f;
        p.out_fg[3 * row + k] = f;
        p.out_bg[3 * row + k] = b;
        p.edit[3 * row + k] = f + t;
    }
    p.relevant[row] = (unsigned char)((rf ? 1 : 0) | (rb ? 2 : 0));
    if (rf && p.fg.mask) {                                     // max(old, alpha): alpha > 0, so the order of the bits is the order of the floats
        const unsigned bits = __builtin_bit_cast(unsigned, alpha);
#pragma unroll
        for (int k = 0; k < 4; ++k) ae_raise(p.fg.mask + cellf[k], bits);
    }
    if (rb && p.bg.mask) {
        const unsigned one = __builtin_bit_cast(unsigned, 1.0f);
#pragma unroll
        for (int k = 0; k < 4; ++k) ae_raise(p.bg.mask + cellb[k], one);
    }
}

inline bool ae_aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

int ae_layer(const char* name, AeLayer& L, const float* tex, int64_t h, int64_t w, int64_t c, float minx, float miny,
             float pixel_size, float shift, const float* base, float* mask, int64_t mask_h, int64_t mask_w) {
    VSX_REQUIRE(c == 3 || c == 4, VSX_E_UNSUPPORTED, "atlas_edit: %s texture has %lld channels (3 = RGB, 4 = RGBA overlay)", name,
                (long long)c);
    VSX_REQUIRE(tex, VSX_E_BADSHAPE, "atlas_edit: null %s texture", name);
    VSX_REQUIRE(h == w, VSX_E_BADSHAPE, "atlas_edit: %s texture is %lld x %lld, not square", name, (long long)h, (long long)w);
    VSX_REQUIRE(h >= 2, VSX_E_BADSHAPE, "atlas_edit: %s texture resolution %lld (at least 2)", name, (long long)h);
    VSX_REQUIRE(h * h * c < (1ll << 31), VSX_E_BADSHAPE, "atlas_edit: %s texture %lld x %lld x %lld does not fit 32-bit indices",
                name, (long long)h, (long long)h, (long long)c);
    VSX_REQUIRE(vsx_aligned16(tex), VSX_E_BADSHAPE, "atlas_edit: %s texture must be 16-byte aligned", name);
    VSX_REQUIRE(c == 3 || base, VSX_E_BADSHAPE, "atlas_edit: an RGBA %s texture needs the base colours it is laid over", name);
    VSX_REQUIRE(!base || ae_aligned(base, 4), VSX_E_BADSHAPE, "atlas_edit: %s base colours must be 4-byte aligned", name);
    VSX_REQUIRE(!mask || (mask_h == h && mask_w == h), VSX_E_BADSHAPE, "atlas_edit: %s mask is %lld x %lld, the texture %lld x %lld",
                name, (long long)mask_h, (long long)mask_w, (long long)h, (long long)h);
    VSX_REQUIRE(!mask || ae_aligned(mask, 4), VSX_E_BADSHAPE, "atlas_edit: %s mask must be 4-byte aligned", name);
    L.tex = tex;
    L.base = c == 4 ? base : nullptr;
    L.mask = (unsigned*)mask;
    L.minx = minx;
    L.miny = miny;
    L.pixel_size = pixel_size;
    L.shift = shift;
    L.R = (int)h;
    return VSX_OK;
}

}  // namespace

extern "C" int vsx_atlas_edit_f32(const float* uv_fg, const float* uv_bg, const float* alpha, int64_t N,
                                  const float* tex_fg, int64_t fg_h, int64_t fg_w, int64_t fg_c, float fg_minx, float fg_miny,
                                  float fg_pixel_size, const float* base_fg, float* mask_fg, int64_t mask_fg_h, int64_t mask_fg_w,
                                  const float* tex_bg, int64_t bg_h, int64_t bg_w, int64_t bg_c, float bg_minx, float bg_miny,
                                  float bg_pixel_size, const float* base_bg, float* mask_bg, int64_t mask_bg_h, int64_t mask_bg_w,
                                  float* edit, float* fg, float* bg, uint8_t* relevant, vsx_stream_t stream) {
    AeParams p;
    int rc = ae_layer("foreground", p.fg, tex_fg, fg_h, fg_w, fg_c, fg_minx, fg_miny, fg_pixel_size, 0.5f, base_fg, mask_fg,
                      mask_fg_h, mask_fg_w);
    if (rc) return rc;
    rc = ae_layer("background", p.bg, tex_bg, bg_h, bg_w, bg_c, bg_minx, bg_miny, bg_pixel_size, -0.5f, base_bg, mask_bg,
                  mask_bg_h, mask_bg_w);
    if (rc) return rc;
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * AE_THREADS, VSX_E_BADSHAPE, "atlas_edit: N = %lld", (long long)N);
    if (N == 0) return VSX_OK;
    VSX_REQUIRE(uv_fg && uv_bg && alpha && edit && fg && bg && relevant, VSX_E_BADSHAPE, "atlas_edit: null argument");
    VSX_REQUIRE(ae_aligned(uv_fg, 8) && ae_aligned(uv_bg, 8), VSX_E_BADSHAPE, "atlas_edit: uv_fg / uv_bg must be 8-byte aligned");
    VSX_REQUIRE(ae_aligned(alpha, 4) && ae_aligned(edit, 4) && ae_aligned(fg, 4) && ae_aligned(bg, 4), VSX_E_BADSHAPE,
                "atlas_edit: alpha / edit / fg / bg must be 4-byte aligned");
    p.uv_fg = uv_fg;
    p.uv_bg = uv_bg;
    p.alpha = alpha;
    p.N = (long)N;
    p.edit = edit;
    p.out_fg = fg;
    p.out_bg = bg;
    p.relevant = relevant;
    const dim3 grid((unsigned)((N + AE_THREADS - 1) / AE_THREADS)), block(AE_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (fg_c == 3 && bg_c == 3)
        hipLaunchKernelGGL((atlas_edit_kernel<3, 3>), grid, block, 0, s, p);
    else if (fg_c == 4 && bg_c == 3)
        hipLaunchKernelGGL((atlas_edit_kernel<4, 3>), grid, block, 0, s, p);
    else if (fg_c == 3 && bg_c == 4)
        hipLaunchKernelGGL((atlas_edit_kernel<3, 4>), grid, block, 0, s, p);
    else
        hipLaunchKernelGGL((atlas_edit_kernel<4, 4>), grid, block, 0, s, p);
    return vsx_check_launch("vsx_atlas_edit_f32");
}
