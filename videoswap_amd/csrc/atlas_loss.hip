// K18 — the data gather and the losses of a layered-neural-atlas training step (train_atlas.py:127-253,
// videoswap/atlas/loss_utils.py) for gfx950.
//
// K18a, vsx_atlas_batch_f32: ONE launch, one thread per sampled pixel.  It reads the pixel's colour, its two discrete
// derivatives, its mask value, its two optical flows and their masks from the device-resident arrays of load_input_data (in
// the reference's own layouts) and writes the query rows of every network call of the step, stacked in blocks of N rows
// (include/vsx.h K18 lists the blocks).  The coordinates are computed the way torch computes them on the CPU in the
// reference: (float)x / (float)(larger_dim / 2) - 1 with an IEEE division, the flow match as (float)x + flow first.  The two
// counts of relevant flow rows are integer atomic adds (exact, order-independent) into two words cleared on the stream.
//
// K18b, vsx_atlas_losses_f32: TWO launches whatever N is.  Every loss of the step is a mean of per-row values whose
// denominator is known beforehand (N, or a count of K18a), so a row's contribution to the gradient of total_loss with respect
// to each of the four network outputs is computed analytically in the pass that computes its loss value: launch 1 takes one
// row per thread, writes that row's entries of the four gradient tensors (every entry has exactly one writer), reduces the
// row's loss terms over its wave (shuffles) and its workgroup (LDS) and writes one partial vector per workgroup; launch 2 adds
// the partial vectors in index order and forms losses[14].  No atomics: two calls give the same bits.
//
// Plain fp32 VALU code: no MFMA, no LDS beyond the reduction, scalar loads and stores only (tools/cpu_check runs this file
// unmodified on the host).  Compiled without contraction of a product and a sum into an FMA, so that K18a's coordinates are
// the reference's bits and the host run of K18b is the device's arithmetic.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_WAVES = AL_THREADS / 64;
// per-row sums of launch 1: 0 gradient, 1 rgb, 2 alpha, 3 sparsity, 4 / 5 rigidity fg / bg, 6 / 7 global rigidity fg / bg,
// 8 / 9 flow fg forward / backward, 10 / 11 flow bg forward / backward, 12 / 13 alpha flow forward / backward,
// 14 / 15 the sum and the count of alpha > 0.5, 16 / 17 of alpha < 0.5
constexpr int AL_TERMS = 18;

// ---------------------------------------------------------------------------------------------------------------------
// K18a
// ---------------------------------------------------------------------------------------------------------------------
struct AbParams {
    const long long* idx;      // [N] flat pixel indices in the (frame, row, column) order of get_tuples
    long N, H, W, T;
    const float* video;        // [H, W, 3, T]
    const float* video_dx;
    const float* video_dy;
    const float* mask;         // [H, W, T]
    const float* flow;         // [H, W, 2, T, 1]
    const float* flow_rev;
    const float* flow_mask;    // [H, W, T, 1]
    const float* flow_rev_mask;
    long d, D;
    float half_dim, half_T;    // (float)(larger_dim / 2.0), (float)(T / 2.0)
    int with_global;
    float* rows;               // [B][N][3]
    float* rgb;                // [N, 3]
    float* rgb_dx;
    float* rgb_dy;
    float* alpha_gt;           // [N]
    float* m_fwd;              // [N]
    float* m_bwd;
    unsigned* counts;          // [2], cleared by the caller
};

__device__ __forceinline__ void ab_row(float* rows, long N, int block, long row, float x, float y, float t) {
    float* o = rows + ((long)block * N + row) * 3;
    o[0] = x;
    o[1] = y;
    o[2] = t;
}

__global__ __launch_bounds__(AL_THREADS) void atlas_batch_kernel(const AbParams p) {
    const long row = (long)blockIdx.x * AL_THREADS + threadIdx.x;
    float mf = 0.f, mb = 0.f;
    if (row < p.N) {
        const long long k = p.idx[row];
        const long HW = p.H * p.W;
        const int B = p.with_global ? 9 : 7;
        if (k < 0 || k >= (long long)(HW * p.T)) {
            // not a pixel of the video (the binding refuses such a batch before it gets here): nothing is read, and the row
            // is marked so that it cannot pass for data
            const float nan = __builtin_nanf("");
            for (int b = 0; b < B; ++b) ab_row(p.rows, p.N, b, row, nan, nan, nan);
            for (int c = 0; c < 3; ++c) p.rgb[3 * row + c] = p.rgb_dx[3 * row + c] = p.rgb_dy[3 * row + c] = nan;
            p.alpha_gt[row] = nan;
        } else {
            const long f = (long)(k / HW), rem = (long)(k % HW);
            const long i = rem / p.W, j = rem % p.W;
            const long pix = i * p.W + j;
            const float hd = p.half_dim, ht = p.half_T;
            const float x = (float)j / hd - 1.0f, y = (float)i / hd - 1.0f, t = (float)f / ht - 1.0f;
            ab_row(p.rows, p.N, 0, row, x, y, t);
            ab_row(p.rows, p.N, 1, row, (float)(j + 1) / hd - 1.0f, y, t);
            ab_row(p.rows, p.N, 2, row, x, (float)(i + 1) / hd - 1.0f, t);
            ab_row(p.rows, p.N, 3, row, x, (float)(i - p.d) / hd - 1.0f, t);
            ab_row(p.rows, p.N, 4, row, (float)(j - p.d) / hd - 1.0f, y, t);
            if (p.with_global) {
                ab_row(p.rows, p.N, 5, row, x, (float)(i - p.D) / hd - 1.0f, t);
                ab_row(p.rows, p.N, 6, row, (float)(j - p.D) / hd - 1.0f, y, t);
            }
            const long fl = pix * 2 * p.T + f;              // [H, W, 2, T, 1]: the x component; the y component T further
            const float fx = p.flow[fl], fy = p.flow[fl + p.T];
            const float rx = p.flow_rev[fl], ry = p.flow_rev[fl + p.T];
            ab_row(p.rows, p.N, B - 2, row, ((float)j + fx) / hd - 1.0f, ((float)i + fy) / hd - 1.0f, (float)(f + 1) / ht - 1.0f);
            ab_row(p.rows, p.N, B - 1, row, ((float)j + rx) / hd - 1.0f, ((float)i + ry) / hd - 1.0f, (float)(f - 1) / ht - 1.0f);
            const long px3 = pix * 3 * p.T + f;             // [H, W, 3, T]
            for (int c = 0; c < 3; ++c) {
                p.rgb[3 * row + c] = p.video[px3 + c * p.T];
                p.rgb_dx[3 * row + c] = p.video_dx[px3 + c * p.T];
                p.rgb_dy[3 * row + c] = p.video_dy[px3 + c * p.T];
            }
            p.alpha_gt[row] = p.mask[pix * p.T + f];
            mf = p.flow_mask[pix * p.T + f] != 0.f ? 1.f : 0.f;          // torch.where(mask): relevant where non-zero
            mb = p.flow_rev_mask[pix * p.T + f] != 0.f ? 1.f : 0.f;
        }
        p.m_fwd[row] = mf;
        p.m_bwd[row] = mb;
    }
    // at most 64 ones per wave: the float sums are exact, and integer adds have no order
    const float cf = wave_sum(mf), cb = wave_sum(mb);
    if ((threadIdx.x & 63) == 0) {
        if (cf > 0.f) atomicAdd(p.counts, (unsigned)cf);
        if (cb > 0.f) atomicAdd(p.counts + 1, (unsigned)cb);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// K18b
// ---------------------------------------------------------------------------------------------------------------------
struct AlParams {
    const float* uv_fg;        // [B N, 2]
    const float* uv_bg;
    const float* alpha_raw;    // [5 N]: blocks 0, 1, 2, forward match, backward match
    const float* rgb_atlas;    // [6 N, 3]: foreground of blocks 0, 1, 2, then background
    const float* rgb;
    const float* rgb_dx;
    const float* rgb_dy;
    const float* alpha_gt;
    const float* m_fwd;
    const float* m_bwd;
    const unsigned* counts;
    float* g_uv_fg;
    float* g_uv_bg;
    float* g_alpha_raw;
    float* g_rgb_atlas;
    float* partial;            // [blocks][AL_TERMS]
    float* losses;             // [14]
    long N;
    int B, with_alpha, with_global;
    float w_gradient, w_rgb, w_alpha, w_sparsity, w_rigidity, w_global_fg, w_global_bg, w_flow, w_alpha_flow;
    float scale, larger, d, D;
};

// get_rigidity_loss (loss_utils.py:52-112) of one row: (u0, v0) = uv(x, y, t), (ua, va) = uv(x, y - d, t), (ub, vb) =
// uv(x - d, y, t) -> the row's value; the gradient of coef * value is added to (gu0, gv0) and stored in the other four
__device__ __forceinline__ float al_rigidity(float u0, float v0, float ua, float va, float ub, float vb, float larger, float scale,
                                             float d, float coef, float& gu0, float& gv0, float& gua, float& gva, float& gub,
                                             float& gvb) {
    // the Jacobian as the reference forms it: difference * larger_dim / 2, then / uv_mapping_scale, then / derivative_amount
    const float du_dx = (u0 - ub) * larger / 2.0f / scale / d, du_dy = (u0 - ua) * larger / 2.0f / scale / d;
    const float dv_dx = (v0 - vb) * larger / 2.0f / scale / d, dv_dy = (v0 - va) * larger / 2.0f / scale / d;
    const float kj = larger / 2.0f / scale / d;
    const float p = du_dx * du_dx + dv_dx * dv_dx, q = du_dx * du_dy + dv_dx * dv_dy, r = du_dy * du_dy + dv_dy * dv_dy;   // JtJ
    const float a = p + 0.001f, e = r + 0.001f;
    const float det = a * e - q * q;                      // >= 0.001^2 by Cauchy-Schwarz: never zero
    const float i00 = e / det, i01 = -q / det, i11 = a / det;
    const float l1 = sqrtf((p * p + q * q) + (q * q + r * r));
    const float l2 = sqrtf((i00 * i00 + i01 * i01) + (i01 * i01 + i11 * i11));
    // d l1: p / l1, 2 q / l1, r / l1 (0 at the zero matrix);  d l2 through the three entries of the inverse
    const float s1 = l1 > 0.f ? 1.0f / l1 : 0.f;
    const float gi00 = i00 / l2, gi01 = 2.0f * i01 / l2, gi11 = i11 / l2;
    const float gdet = -(gi00 * i00 + gi01 * i01 + gi11 * i11) / det;
    const float gp = p * s1 + (gi11 / det + gdet * e);
    const float gr = r * s1 + (gi00 / det + gdet * a);
    const float gq = 2.0f * q * s1 + (-gi01 / det - gdet * 2.0f * q);
    const float g_du_dx = 2.0f * gp * du_dx + gq * du_dy, g_dv_dx = 2.0f * gp * dv_dx + gq * dv_dy;
    const float g_du_dy = 2.0f * gr * du_dy + gq * du_dx, g_dv_dy = 2.0f * gr * dv_dy + gq * dv_dx;
    const float c = coef * kj;
    gub = -c * g_du_dx;
    gvb = -c * g_dv_dx;
    gua = -c * g_du_dy;
    gva = -c * g_dv_dy;
    gu0 += c * (g_du_dx + g_du_dy);
    gv0 += c * (g_dv_dx + g_dv_dy);
    return l1 + l2;
}

// One direction of get_optical_flow_loss (:132-153, use_alpha=True) of one row: (um, vm) = uv of the flow match, `aw` = the
// alpha weight (alpha for the foreground, 1 - alpha for the background), m = the row's 0/1 relevance, coef = weight * 0.5 /
// count -> the row's value (0 where not relevant); gradients: the match's are stored, (gu0, gv0) and gaw are added to
__device__ __forceinline__ float al_flow(float u0, float v0, float um, float vm, float aw, float m, float coef, float larger,
                                         float scale, float& gu0, float& gv0, float& gum, float& gvm, float& gaw) {
    gum = gvm = 0.f;
    if (!(m != 0.f)) return 0.f;                          // a masked row: nothing of it is used, whatever the network gave
    const float eu = um - u0, ev = vm - v0;
    const float n = sqrtf(eu * eu + ev * ev);
    const float lf = n * larger / (2.0f * scale);
    if (n > 0.f) {                                        // the gradient of a norm at the zero vector is 0
        const float c = coef * aw * (larger / (2.0f * scale)) / n;
        gum = c * eu;
        gvm = c * ev;
        gu0 -= gum;
        gv0 -= gvm;
    }
    gaw += coef * lf;
    return lf * aw;
}

struct AlLayerOut {
    float rig, grig, ffwd, fbwd;
};

// everything a mapping network's output enters directly: both rigidity losses and the flow loss.  ga0 += d / d alpha of block 0
// (sign = +1 for the foreground, whose weight is alpha, -1 for the background, whose weight is 1 - alpha)
__device__ __forceinline__ AlLayerOut al_layer(const AlParams& p, const float* __restrict__ uv, float* __restrict__ g, long i,
                                               float w_global, float aw, float sign, float mf, float mb, float cf, float cb,
                                               float& ga0) {
    const long N = p.N;
    const int B = p.B;
    const float nf = (float)N;
    AlLayerOut o{0.f, 0.f, 0.f, 0.f};
    const float u0 = uv[2 * i], v0 = uv[2 * i + 1];
    float gu0 = 0.f, gv0 = 0.f, ga = 0.f, gb = 0.f, gc = 0.f, gd = 0.f;
    o.rig = al_rigidity(u0, v0, uv[2 * (3 * N + i)], uv[2 * (3 * N + i) + 1], uv[2 * (4 * N + i)], uv[2 * (4 * N + i) + 1], p.larger,
                        p.scale, p.d, p.w_rigidity / nf, gu0, gv0, ga, gb, gc, gd);
    g[2 * (3 * N + i)] = ga, g[2 * (3 * N + i) + 1] = gb, g[2 * (4 * N + i)] = gc, g[2 * (4 * N + i) + 1] = gd;
    if (p.with_global) {
        o.grig = al_rigidity(u0, v0, uv[2 * (5 * N + i)], uv[2 * (5 * N + i) + 1], uv[2 * (6 * N + i)], uv[2 * (6 * N + i) + 1],
                             p.larger, p.scale, p.D, w_global / nf, gu0, gv0, ga, gb, gc, gd);
        g[2 * (5 * N + i)] = ga, g[2 * (5 * N + i) + 1] = gb, g[2 * (6 * N + i)] = gc, g[2 * (6 * N + i) + 1] = gd;
    }
    float gaw = 0.f;
    const long rf = (long)(B - 2) * N + i, rb = (long)(B - 1) * N + i;
    o.ffwd = al_flow(u0, v0, uv[2 * rf], uv[2 * rf + 1], aw, mf, cf, p.larger, p.scale, gu0, gv0, ga, gb, gaw);
    g[2 * rf] = ga, g[2 * rf + 1] = gb;
    o.fbwd = al_flow(u0, v0, uv[2 * rb], uv[2 * rb + 1], aw, mb, cb, p.larger, p.scale, gu0, gv0, ga, gb, gaw);
    g[2 * rb] = ga, g[2 * rb + 1] = gb;
    ga0 += sign * gaw;
    g[2 * i] = gu0, g[2 * i + 1] = gv0;
    // blocks 1 and 2 reach the losses through F_Atlas only
    g[2 * (N + i)] = 0.f, g[2 * (N + i) + 1] = 0.f, g[2 * (2 * N + i)] = 0.f, g[2 * (2 * N + i) + 1] = 0.f;
    return o;
}

__device__ __forceinline__ float al_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }   // d |x|: 0 at 0

__device__ __forceinline__ void al_row(const AlParams& p, long i, float (&t)[AL_TERMS]) {
    const long N = p.N;
    const float nf = (float)N;
    // alpha of the five blocks F_Alpha sees, mapped to 0.001 .. 0.991 in the reference's three steps
    float a[5], ga[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        a[k] = 0.5f * (p.alpha_raw[k * N + i] + 1.0f) * 0.99f + 0.001f;
        ga[k] = 0.f;
    }
    const float a0 = a[0], na0 = 1.0f - a[0];
    const float mf = p.m_fwd[i], mb = p.m_bwd[i];
    const float nfw = (float)p.counts[0], nbw = (float)p.counts[1];
    // a relevant row implies a count of at least one
    const float cf_flow = mf != 0.f ? p.w_flow * 0.5f / nfw : 0.f, cb_flow = mb != 0.f ? p.w_flow * 0.5f / nbw : 0.f;

    // the mapping networks: rigidity and flow
    const AlLayerOut fg = al_layer(p, p.uv_fg, p.g_uv_fg, i, p.w_global_fg, a0, 1.0f, mf, mb, cf_flow, cb_flow, ga[0]);
    const AlLayerOut bg = al_layer(p, p.uv_bg, p.g_uv_bg, i, p.w_global_bg, na0, -1.0f, mf, mb, cf_flow, cb_flow, ga[0]);
    t[4] = fg.rig, t[5] = bg.rig, t[6] = fg.grig, t[7] = bg.grig;
    t[8] = fg.ffwd, t[9] = fg.fbwd, t[10] = bg.ffwd, t[11] = bg.fbwd;

    // the alpha flow loss (:212-233): |alpha - alpha_match| forward, |alpha_match - alpha| backward
    if (mf != 0.f) {
        const float dl = a0 - a[3], c = p.w_alpha_flow * 0.5f / nfw * al_sign(dl);
        t[12] = fabsf(dl);
        ga[0] += c;
        ga[3] -= c;
    }
    if (mb != 0.f) {
        const float dl = a[4] - a0, c = p.w_alpha_flow * 0.5f / nbw * al_sign(dl);
        t[13] = fabsf(dl);
        ga[4] += c;
        ga[0] -= c;
    }
    if (a0 > 0.5f) t[14] = a0, t[15] = 1.f;
    if (a0 < 0.5f) t[16] = a0, t[17] = 1.f;

    // the colours: rgb_output of blocks 0, 1, 2 from the two layers
    float cf[3][3], cb[3][3], out[3][3], gout[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cf[k][c] = (p.rgb_atlas[(k * N + i) * 3 + c] + 1.0f) * 0.5f;
            cb[k][c] = (p.rgb_atlas[((3 + k) * N + i) * 3 + c] + 1.0f) * 0.5f;
            out[k][c] = cf[k][c] * a[k] + cb[k][c] * (1.0f - a[k]);
        }
    float s_grad = 0.f, s_rgb = 0.f, s_sp = 0.f;
    float gcf0[3];
    const float c_grad = p.w_gradient / nf, c_rgb = p.w_rgb / nf, c_sp = p.w_sparsity / nf;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // get_gradient_loss (:5-48): the reconstruction's own forward differences against the precomputed ones
        const float ex = p.rgb_dx[3 * i + c] - (out[1][c] - out[0][c]), ey = p.rgb_dy[3 * i + c] - (out[2][c] - out[0][c]);
        s_grad += ex * ex + ey * ey;
        const float r = out[0][c] - p.rgb[3 * i + c];
        s_rgb += r * r;
        gout[1][c] = -2.0f * c_grad * ex;
        gout[2][c] = -2.0f * c_grad * ey;
        gout[0][c] = 2.0f * c_grad * (ex + ey) + 2.0f * c_rgb * r;
        // sparsity: |rgb_output_fg (1 - alpha)|^2
        const float s = cf[0][c] * na0;
        s_sp += s * s;
        gcf0[c] = 2.0f * c_sp * s * na0;
        ga[0] -= 2.0f * c_sp * s * cf[0][c];
    }
    t[0] = s_grad, t[1] = s_rgb, t[3] = s_sp;
    if (p.with_alpha) {
        const float gt = p.alpha_gt[i];
        t[2] = -gt * logf(a0) - (1.0f - gt) * logf(na0);
        ga[0] += p.w_alpha / nf * (-gt / a0 + (1.0f - gt) / na0);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // (atlas + 1) * 0.5: a factor 0.5 on the way back
            p.g_rgb_atlas[(k * N + i) * 3 + c] = (gout[k][c] * a[k] + (k == 0 ? gcf0[c] : 0.f)) * 0.5f;
            p.g_rgb_atlas[((3 + k) * N + i) * 3 + c] = gout[k][c] * (1.0f - a[k]) * 0.5f;
            dot += gout[k][c] * (cf[k][c] - cb[k][c]);
        }
        ga[k] += dot;
    }
    // 0.5 (raw + 1) * 0.99 + 0.001: a factor 0.495 on the way back
#pragma unroll
    for (int k = 0; k < 5; ++k) p.g_alpha_raw[k * N + i] = ga[k] * 0.495f;
}

__global__ __launch_bounds__(AL_THREADS) void atlas_losses_rows_kernel(const AlParams p) {
    __shared__ float red[AL_WAVES][AL_TERMS];
    const long i = (long)blockIdx.x * AL_THREADS + threadIdx.x;
    float t[AL_TERMS];
#pragma unroll
    for (int k = 0; k < AL_TERMS; ++k) t[k] = 0.f;
    if (i < p.N) al_row(p, i, t);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < AL_TERMS; ++k) {
        const float s = wave_sum(t[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < AL_TERMS) {
        float s = red[0][threadIdx.x];
        for (int w = 1; w < AL_WAVES; ++w) s += red[w][threadIdx.x];
        p.partial[(long)blockIdx.x * AL_TERMS + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void atlas_losses_finish_kernel(const AlParams p, long blocks) {
    __shared__ float fin[AL_TERMS];
    if (threadIdx.x < AL_TERMS) {
        float s = 0.f;
        for (long b = 0; b < blocks; ++b) s += p.partial[b * AL_TERMS + threadIdx.x];     // index order
        fin[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float nf = (float)p.N, nfw = (float)p.counts[0], nbw = (float)p.counts[1];
    float L[14];
    L[0] = fin[0] / nf;
    L[1] = fin[1] / nf;
    L[2] = p.with_alpha ? fin[2] / nf : 0.f;
    L[3] = fin[3] / nf;
    L[4] = fin[4] / nf;
    L[5] = fin[5] / nf;
    L[6] = p.with_global ? fin[6] / nf : 0.f;
    L[7] = p.with_global ? fin[7] / nf : 0.f;
    // a mean over no relevant row is 0 here (NaN in the reference)
    const float ff = nfw > 0.f ? fin[8] / nfw : 0.f, fb = nbw > 0.f ? fin[9] / nbw : 0.f;
    const float bf = nfw > 0.f ? fin[10] / nfw : 0.f, bb = nbw > 0.f ? fin[11] / nbw : 0.f;
    const float af = nfw > 0.f ? fin[12] / nfw : 0.f, ab = nbw > 0.f ? fin[13] / nbw : 0.f;
    L[8] = fb * 0.5f + ff * 0.5f;
    L[9] = bb * 0.5f + bf * 0.5f;
    L[10] = (af + ab) * 0.5f;
    float total = p.w_gradient * L[0];
    total += p.w_rgb * L[1];
    if (p.with_alpha) total += p.w_alpha * L[2];
    total += p.w_sparsity * L[3];
    total += p.w_rigidity * L[4];
    total += p.w_rigidity * L[5];
    if (p.with_global) {
        total += p.w_global_fg * L[6];
        total += p.w_global_bg * L[7];
    }
    total += p.w_flow * L[8];
    total += p.w_flow * L[9];
    total += p.w_alpha_flow * L[10];
    L[11] = total;
    L[12] = fin[14] / fin[15];                            // NaN on an empty set, as in the reference
    L[13] = fin[16] / fin[17];
    for (int k = 0; k < 14; ++k) p.losses[k] = L[k];
}

inline bool al_aligned(const void* p, uintptr_t a) { return p && (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

extern "C" int vsx_atlas_batch_f32(const int64_t* idx, int64_t N, int64_t H, int64_t W, int64_t T, int64_t flow_levels,
                                   const float* video, const float* video_dx, const float* video_dy, const float* mask,
                                   const float* flow, const float* flow_rev, const float* flow_mask,
                                   const float* flow_rev_mask, int64_t d, int64_t D, int64_t with_global, float* rows, float* rgb,
                                   float* rgb_dx, float* rgb_dy, float* alpha_gt, float* m_fwd, float* m_bwd, int32_t* counts,
                                   vsx_stream_t stream) {
    VSX_REQUIRE(flow_levels == 1, VSX_E_UNSUPPORTED, "atlas_batch: %lld flow levels (load_input_data has one: the last axis of optical_flows is 1)",
                (long long)flow_levels);
    VSX_REQUIRE(H >= 1 && W >= 1 && T >= 1 && H * W <= (1ll << 40) / 6 / T, VSX_E_BADSHAPE, "atlas_batch: video of %lld x %lld x %lld frames",
                (long long)H, (long long)W, (long long)T);
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) / 27, VSX_E_BADSHAPE, "atlas_batch: N = %lld", (long long)N);
    VSX_REQUIRE(d >= 1 && D >= 1 && d < (1 << 24) && D < (1 << 24), VSX_E_BADSHAPE, "atlas_batch: derivative amounts %lld, %lld (at least 1)",
                (long long)d, (long long)D);
    VSX_REQUIRE(al_aligned(counts, 4), VSX_E_BADSHAPE, "atlas_batch: counts is null or not 4-byte aligned");
    VSX_REQUIRE(al_aligned(video, 4) && al_aligned(video_dx, 4) && al_aligned(video_dy, 4) && al_aligned(mask, 4) && al_aligned(flow, 4) &&
                    al_aligned(flow_rev, 4) && al_aligned(flow_mask, 4) && al_aligned(flow_rev_mask, 4),
                VSX_E_BADSHAPE, "atlas_batch: a data array is null or not 4-byte aligned");
    if (N > 0) {
        VSX_REQUIRE(al_aligned(idx, 8), VSX_E_BADSHAPE, "atlas_batch: idx is null or not 8-byte aligned");
        VSX_REQUIRE(al_aligned(rows, 4) && al_aligned(rgb, 4) && al_aligned(rgb_dx, 4) && al_aligned(rgb_dy, 4) && al_aligned(alpha_gt, 4) &&
                        al_aligned(m_fwd, 4) && al_aligned(m_bwd, 4),
                    VSX_E_BADSHAPE, "atlas_batch: an output is null or not 4-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return vsx_fail(VSX_E_LAUNCH, "atlas_batch: hipMemsetAsync: %s", hipGetErrorString(e));
    if (N == 0) return VSX_OK;
    AbParams p;
    p.idx = (const long long*)idx;
    p.N = (long)N, p.H = (long)H, p.W = (long)W, p.T = (long)T;
    p.video = video, p.video_dx = video_dx, p.video_dy = video_dy, p.mask = mask;
    p.flow = flow, p.flow_rev = flow_rev, p.flow_mask = flow_mask, p.flow_rev_mask = flow_rev_mask;
    p.d = (long)d, p.D = (long)D;
    p.half_dim = (float)((double)(H > W ? H : W) / 2.0);
    p.half_T = (float)((double)T / 2.0);
    p.with_global = with_global ? 1 : 0;
    p.rows = rows, p.rgb = rgb, p.rgb_dx = rgb_dx, p.rgb_dy = rgb_dy, p.alpha_gt = alpha_gt, p.m_fwd = m_fwd, p.m_bwd = m_bwd;
    p.counts = (unsigned*)counts;
    const dim3 grid((unsigned)((N + AL_THREADS - 1) / AL_THREADS)), block(AL_THREADS);
    hipLaunchKernelGGL(atlas_batch_kernel, grid, block, 0, s, p);
    return vsx_check_launch("vsx_atlas_batch_f32");
}

extern "C" int64_t vsx_atlas_losses_workspace(int64_t N) {
    const int64_t blocks = N > 0 ? (N + AL_THREADS - 1) / AL_THREADS : 0;
    return (blocks > 0 ? blocks : 1) * AL_TERMS;
}

extern "C" int vsx_atlas_losses_f32(const float* uv_fg, const float* uv_bg, const float* alpha_raw, const float* rgb_atlas, int64_t N,
                                    const float* rgb, const float* rgb_dx, const float* rgb_dy, const float* alpha_gt,
                                    const float* m_fwd, const float* m_bwd, const int32_t* counts, const vsx_atlas_loss_cfg* cfg,
                                    float* losses, float* g_uv_fg, float* g_uv_bg, float* g_alpha_raw, float* g_rgb_atlas,
                                    float* scratch, int64_t scratch_floats, vsx_stream_t stream) {
    VSX_REQUIRE(cfg, VSX_E_BADSHAPE, "atlas_losses: null configuration");
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) / 27, VSX_E_BADSHAPE, "atlas_losses: N = %lld", (long long)N);
    VSX_REQUIRE(cfg->larger_dim >= 1 && cfg->larger_dim < (1 << 24) && cfg->derivative_amount >= 1 && cfg->global_derivative_amount >= 1 &&
                    cfg->derivative_amount < (1 << 24) && cfg->global_derivative_amount < (1 << 24),
                VSX_E_BADSHAPE, "atlas_losses: larger_dim %lld, derivative amounts %lld, %lld (each at least 1)", (long long)cfg->larger_dim,
                (long long)cfg->derivative_amount, (long long)cfg->global_derivative_amount);
    VSX_REQUIRE(cfg->uv_mapping_scale > 0.0, VSX_E_BADSHAPE, "atlas_losses: uv_mapping_scale %g (positive)", cfg->uv_mapping_scale);
    VSX_REQUIRE(scratch_floats >= vsx_atlas_losses_workspace(N), VSX_E_WORKSPACE, "atlas_losses: scratch holds %lld floats, %lld needed",
                (long long)scratch_floats, (long long)vsx_atlas_losses_workspace(N));
    VSX_REQUIRE(al_aligned(losses, 4) && al_aligned(scratch, 4) && al_aligned(counts, 4), VSX_E_BADSHAPE,
                "atlas_losses: losses, scratch or counts is null or not 4-byte aligned");
    if (N > 0) {
        VSX_REQUIRE(al_aligned(uv_fg, 4) && al_aligned(uv_bg, 4) && al_aligned(alpha_raw, 4) && al_aligned(rgb_atlas, 4) && al_aligned(rgb, 4) &&
                        al_aligned(rgb_dx, 4) && al_aligned(rgb_dy, 4) && al_aligned(alpha_gt, 4) && al_aligned(m_fwd, 4) && al_aligned(m_bwd, 4),
                    VSX_E_BADSHAPE, "atlas_losses: an input is null or not 4-byte aligned");
        VSX_REQUIRE(al_aligned(g_uv_fg, 4) && al_aligned(g_uv_bg, 4) && al_aligned(g_alpha_raw, 4) && al_aligned(g_rgb_atlas, 4), VSX_E_BADSHAPE,
                    "atlas_losses: a gradient output is null or not 4-byte aligned");
    }
    AlParams p;
    p.uv_fg = uv_fg, p.uv_bg = uv_bg, p.alpha_raw = alpha_raw, p.rgb_atlas = rgb_atlas;
    p.rgb = rgb, p.rgb_dx = rgb_dx, p.rgb_dy = rgb_dy, p.alpha_gt = alpha_gt, p.m_fwd = m_fwd, p.m_bwd = m_bwd;
    p.counts = (const unsigned*)counts;
    p.g_uv_fg = g_uv_fg, p.g_uv_bg = g_uv_bg, p.g_alpha_raw = g_alpha_raw, p.g_rgb_atlas = g_rgb_atlas;
    p.partial = scratch, p.losses = losses;
    p.N = (long)N;
    p.with_alpha = cfg->with_alpha_loss ? 1 : 0;
    p.with_global = cfg->with_global_rigidity ? 1 : 0;
    p.B = p.with_global ? 9 : 7;
    p.w_gradient = (float)cfg->gradient_loss_weight, p.w_rgb = (float)cfg->rgb_loss_weight, p.w_alpha = (float)cfg->alpha_loss_weight;
    p.w_sparsity = (float)cfg->sparsity_loss_weight, p.w_rigidity = (float)cfg->rigidity_loss_weight;
    p.w_global_fg = (float)cfg->global_rigidity_fg_loss_weight, p.w_global_bg = (float)cfg->global_rigidity_bg_loss_weight;
    p.w_flow = (float)cfg->flow_loss_weight, p.w_alpha_flow = (float)cfg->alpha_flow_loss_weight;
    p.scale = (float)cfg->uv_mapping_scale, p.larger = (float)cfg->larger_dim;
    p.d = (float)cfg->derivative_amount, p.D = (float)cfg->global_derivative_amount;
    hipStream_t s = (hipStream_t)stream;
    const long blocks = (long)((N + AL_THREADS - 1) / AL_THREADS);
    if (blocks > 0) {
        hipLaunchKernelGGL(atlas_losses_rows_kernel, dim3((unsigned)blocks), dim3(AL_THREADS), 0, s, p);
        const int rc = vsx_check_launch("vsx_atlas_losses_f32 (rows)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(atlas_losses_finish_kernel, dim3(1), dim3(64), 0, s, p, blocks);
    return vsx_check_launch("vsx_atlas_losses_f32 (finish)");
}
