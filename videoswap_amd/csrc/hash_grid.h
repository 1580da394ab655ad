// The multiresolution hash grid of vsx.h K14 as the forward (atlas.hip, K14) and the backward (atlas_bwd.hip, K17) share it:
// the level table, its host-side geometry and option checks, and THE device code that turns a coordinate into a cell's four
// table entries and its two interpolation weights (hg_cell, hg_weight).  The forward gathers through them, the backward
// scatters through them: there is no second statement of the index arithmetic.
#pragma once
#include <math.h>

#include "coord_mlp.h"

namespace {

constexpr int HG_MAX_LEVELS = 32;
constexpr int HG_PASS = 16;          // levels per pass of a workgroup: 4 waves x 4 levels per thread

struct HgLevel {
    float scale;                     // grid cells per unit, minus the half-cell shift's 1
    uint32_t res, entries, offset;   // offset: first entry of the level in the table
    uint32_t hashed;                 // 0: dense index g0 + g1 * res, 1: spatial hash
};

struct HashGrid {
    static constexpr bool kHash = true;
    const float2* table;             // [sum entries][2 features], level-major
    int n_levels;
    HgLevel lv[HG_MAX_LEVELS];       // unused levels: entries 1, never read from the table
};

struct NoGrid {
    static constexpr bool kHash = false;
};

// The cell of (x0, x1) on one level: the interpolation weights w0, w1 along the two axes and the table entries idx[c]
// (the level's offset included) of its corners c = 0 .. 3, corner c at (g0 + (c & 1), g1 + (c >> 1)).  All index
// arithmetic is uint32 with wrap-around; every index is reduced modulo the level's entry count, so no coordinate
// (negative, huge, NaN) can address outside the table.
__device__ __forceinline__ void hg_cell(const HgLevel& lv, float x0, float x1, float& w0, float& w1, uint32_t (&idx)[4]) {
    const float p0 = fmaf(lv.scale, x0, 0.5f), p1 = fmaf(lv.scale, x1, 0.5f);
    const float fl0 = floorf(p0), fl1 = floorf(p1);
    const uint32_t g0 = (uint32_t)(int)fl0, g1 = (uint32_t)(int)fl1;
    w0 = p0 - fl0, w1 = p1 - fl1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t c0 = g0 + (c & 1), c1 = g1 + (c >> 1);
        uint32_t i = lv.hashed ? (c0 ^ (c1 * 2654435761u)) : c0 + c1 * lv.res;
        i %= lv.entries;
        idx[c] = lv.offset + i;
    }
}

// the bilinear weight of corner c
__device__ __forceinline__ float hg_weight(int c, float w0, float w1) {
    return ((c & 1) ? w0 : 1.f - w0) * ((c >> 1) ? w1 : 1.f - w1);
}

// THE definition of the level geometry (tiny-cuda-nn's GridEncoding constructor, restated): per level l
//   scale = exp2f(l * log2f(per_level_scale)) * base_resolution - 1   (fp32),   res = (uint32)ceilf(scale) + 1,
//   entries = min(round_up(res^2, 8), 2^log2_hashmap_size),   offset = the running sum of entries,
// and the index of a corner (g0, g1), uint32 with wrap-around: stride = 1; idx = g0, stride *= res; then, while
// stride <= entries, idx += g1 * stride, stride *= res; the level is HASHED when entries < stride afterwards.
// Returns the table's float count, or a negative VSX_E_* (the message names the option).
inline int64_t hg_geometry(const char* what, int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size,
                           int64_t base_resolution, double per_level_scale, HgLevel* lv) {
    VSX_REQUIRE(n_features == 2, VSX_E_UNSUPPORTED, "%s: n_features_per_level %lld (only 2)", what, (long long)n_features);
    VSX_REQUIRE(n_levels >= 1 && n_levels <= HG_MAX_LEVELS && n_levels * n_features <= CM_MAX_ENC, VSX_E_UNSUPPORTED,
                "%s: n_levels %lld (1 to %d, at most %d encoded columns)", what, (long long)n_levels, HG_MAX_LEVELS, CM_MAX_ENC);
    VSX_REQUIRE(log2_hashmap_size >= 3 && log2_hashmap_size <= 24, VSX_E_UNSUPPORTED, "%s: log2_hashmap_size %lld (3 to 24)",
                what, (long long)log2_hashmap_size);
    VSX_REQUIRE(base_resolution >= 1 && base_resolution <= 65536, VSX_E_UNSUPPORTED, "%s: base_resolution %lld (1 to 65536)",
                what, (long long)base_resolution);
    VSX_REQUIRE(per_level_scale >= 1.0 && per_level_scale <= 16.0, VSX_E_UNSUPPORTED, "%s: per_level_scale %g (1 to 16)", what,
                per_level_scale);
    const uint32_t cap = 1u << log2_hashmap_size;
    uint64_t offset = 0;
    for (int l = 0; l < HG_MAX_LEVELS; ++l) {
        lv[l] = HgLevel{0.f, 1u, 1u, 0u, 0u};
        if (l >= n_levels) continue;
        const float scale = exp2f((float)l * log2f((float)per_level_scale)) * (float)base_resolution - 1.0f;
        // inputs lie within [-2, 2]: 2 * scale + 1.5 must stay far inside int32 for (uint32)(int)floorf(pos)
        VSX_REQUIRE(scale >= 0.f && scale <= 16777216.f, VSX_E_UNSUPPORTED,
                    "%s: per_level_scale %g / base_resolution %lld: level %d has %g cells (at most 2^24)", what, per_level_scale,
                    (long long)base_resolution, l, (double)scale);
        const uint32_t res = (uint32_t)ceilf(scale) + 1u;
        const uint64_t dense = ((uint64_t)res * res + 7) / 8 * 8;
        const uint32_t entries = dense < cap ? (uint32_t)dense : cap;
        uint32_t stride = res;                                   // after dimension 0 (stride 1 <= entries always)
        if (stride <= entries) stride *= res;                    // dimension 1, uint32 wrap-around
        lv[l] = HgLevel{scale, res, entries, (uint32_t)offset, entries < stride ? 1u : 0u};
        offset += entries;
    }
    return (int64_t)offset * n_features;
}

// the grid's options alone (no table): the level table -> lv, the table's float count -> *need
inline int hg_options(const char* what, HgLevel* lv, int64_t* need, int64_t input_dim, int64_t n_levels, int64_t n_features,
                      int64_t log2_hashmap_size, int64_t base_resolution, double per_level_scale) {
    VSX_REQUIRE(input_dim == 2, VSX_E_UNSUPPORTED, "%s: input_dim %lld (the hash grid is implemented for 2 only)", what,
                (long long)input_dim);
    *need = hg_geometry(what, n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale, lv);
    return *need < 0 ? (int)*need : VSX_OK;
}

inline int hg_fill(const char* what, HashGrid& g, int64_t input_dim, const float* table, int64_t table_floats, int64_t n_levels,
                   int64_t n_features, int64_t log2_hashmap_size, int64_t base_resolution, double per_level_scale) {
    int64_t need = 0;
    const int rc = hg_options(what, g.lv, &need, input_dim, n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale);
    if (rc != VSX_OK) return rc;
    VSX_REQUIRE(table_floats == need, VSX_E_BADSHAPE, "%s: the grid table holds %lld floats, this configuration needs %lld", what,
                (long long)table_floats, (long long)need);
    g.table = reinterpret_cast<const float2*>(table), g.n_levels = (int)n_levels;
    return VSX_OK;
}

}  // namespace
