// K16: weight and bias gradients of the coordinate MLP (K13, atlas.hip), exact fp32 on v_mfma_f32_32x32x2_f32, unfused and
// deterministic.  The forward's training instantiation has stored, per row, the encoded input, every hidden
// layer's activation after its ReLU and the output (`saved`, vsx.h K16).  From the output layer down, per layer l:
//   wgrad   dW_l = dZ_l^T In_l,  db_l = the column sums of dZ_l,  In_l = cat(H_{l-1}, enc) as the layer saw it.  The N rows are
//           cut into chunks of CMB_ROWS; a wave owns one 32 x 32 tile of [features] x [input columns, then one bias column] of
//           one chunk and writes it to that chunk's slice of `partial`.  A row pair is one MFMA (the rows are its k); the four
//           MFMAs of eight rows go to four accumulators that are added pairwise at the end, so a chain is CMB_ROWS / 4 rows.
//   dgrad   dZ_{l-1} = (dZ_l W_l[:, :hidden]) masked by H_{l-1} > 0, H_{l-1} as STORED.  A wave owns 32 rows x 32 columns; the
//           features are its k, again in four accumulators.  The encoded columns of a skip layer get no data gradient (the
//           reference concatenates a detached copy), and layer 0 none at all: nothing here differentiates the input.
// One last launch adds the chunks' partials in index order.  No atomics; the launch count is 2 * layers + 1 whatever N is.
// Operands come straight from global memory, one float per lane and MFMA (lanes 0 .. 31 read 128 consecutive bytes): the
// buffers of a 10 000-row batch sit in the L2, and peak rate is not what this file is for.  A row >= N, a feature >= F and
// an input column >= K are never read: their operand is a literal zero.
#include "coord_mlp.h"
#include "hash_grid.h"

namespace {

constexpr int CMB_ROWS = 512;        // rows per wgrad chunk (vsx_coord_mlp_wgrad_rows)
constexpr int CMB_THREADS = 256;

__device__ __forceinline__ f16v cmb_zero() {
    f16v z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// dz[i] = grad_out[i] * (1 - out[i]^2) (tanh) or grad_out[i]
__global__ __launch_bounds__(CMB_THREADS) void cmb_dz_out_kernel(const float* __restrict__ grad_out, const float* __restrict__ out,
                                                                  float* __restrict__ dz, long n, int use_tanh) {
    const long i = (long)blockIdx.x * CMB_THREADS + threadIdx.x;
    if (i >= n) return;
    const float o = out[i];
    dz[i] = use_tanh ? grad_out[i] * (1.0f - o * o) : grad_out[i];
}

// partial[chunk blockIdx.x][f * K + k] (the weight, K = kh + ke) and [F * K + f] (the bias) of one layer; `partial` points at
// the layer's place in chunk 0, P floats separate two chunks.  h [N, kh] (kh 0: none), enc [N, ke] (ke 0: none).
__global__ __launch_bounds__(CMB_THREADS) void cmb_wgrad_kernel(const float* __restrict__ dz, int F, const float* __restrict__ h, int kh,
                                                                 const float* __restrict__ enc, int ke, long N,
                                                                 float* __restrict__ partial, long P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const int nkh = kh / 32, nke = (ke + 31) / 32, nkt = nkh + nke + 1, nft = (F + 31) / 32;
    const int t = blockIdx.y * (CMB_THREADS / 64) + wave;
    if (t >= nft * nkt) return;
    const int ft = t / nkt, kt = t - ft * nkt;
    const long r0 = (long)blockIdx.x * CMB_ROWS, r1 = r0 + CMB_ROWS < N ? r0 + CMB_ROWS : N;

    // the B operand's source: a column of h, of enc, or the ones of the bias
    const float* src = nullptr;
    int ld = 0, c = 0;
    bool colok = true;
    if (kt < nkh) {
        src = h, ld = kh, c = kt * 32 + col;
    } else if (kt < nkh + nke) {
        src = enc, ld = ke, c = (kt - nkh) * 32 + col, colok = c < ke;
    } else {
        colok = col == 0;
    }
    const int f = ft * 32 + col;
    const bool fok = f < F;

    f16v acc[4] = {cmb_zero(), cmb_zero(), cmb_zero(), cmb_zero()};
    for (long r = r0; r < r1; r += 8) {
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long row = r + 2 * j + hi;
            const bool rowok = row < r1;
            a[j] = rowok && fok ? dz[row * F + f] : 0.f;
            b[j] = rowok && colok ? (src ? src[row * ld + c] : 1.0f) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc[j], 0, 0, 0);
    }

    float* out = partial + (long)blockIdx.x * P;
    const int K = kh + ke;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float v = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
        const int fo = ft * 32 + 8 * (i >> 2) + 4 * hi + (i & 3);
        if (fo < F && colok) {
            if (src)
                out[(long)fo * K + (kt < nkh ? c : kh + c)] = v;
            else
                out[(long)F * K + fo] = v;
        }
    }
}

// dh[row][k] = h[row][k] > 0 ? sum over f of dz[row][f] * W[f][k] : 0  for k < hidden; wl: the layer's packed weight
// ([F / 32][KB][2][32][4], vsx.h K13: W[f][k] at ((f / 32 * KB + k / 8) * 2 + k % 8 / 4) * 128 + f % 32 * 4 + k % 4)
__global__ __launch_bounds__(CMB_THREADS) void cmb_dgrad_kernel(const float* __restrict__ dz, int F, const float* __restrict__ wl, int KB,
                                                                 const float* __restrict__ h, int hidden, long N, float* __restrict__ dh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const int kt = blockIdx.y * (CMB_THREADS / 64) + wave;
    if (kt * 32 >= hidden) return;
    const long row0 = (long)blockIdx.x * 32, row = row0 + col;
    const bool rowok = row < N;
    const int k = kt * 32 + col;
    const float* wk = wl + ((long)(k >> 3) * 2 + ((k & 7) >> 2)) * 128 + (k & 3);

    f16v acc[4] = {cmb_zero(), cmb_zero(), cmb_zero(), cmb_zero()};
    for (int f0 = 0; f0 < F; f0 += 8) {
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = f0 + 4 * hi + j;             // f < 32 * ceil(F / 32): inside the packed layer, whose padding is zero
            a[j] = rowok && f < F ? dz[row * F + f] : 0.f;
            b[j] = wk[(long)(f >> 5) * KB * 256 + (f & 31) * 4];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const long orow = row0 + 8 * (i >> 2) + 4 * hi + (i & 3);
        if (orow < N) {
            const float v = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
            dh[orow * hidden + k] = h[orow * hidden + k] > 0.f ? v : 0.f;
        }
    }
}

// grad[i] = partial[0][i] + partial[1][i] + ... in chunk order
__global__ __launch_bounds__(CMB_THREADS) void cmb_reduce_kernel(const float* __restrict__ partial, long P, long chunks,
                                                                  float* __restrict__ grad) {
    const long i = (long)blockIdx.x * CMB_THREADS + threadIdx.x;
    if (i >= P) return;
    float s = partial[i];
    for (long c = 1; c < chunks; ++c) s += partial[c * P + i];
    grad[i] = s;
}

struct CmbNet {
    int64_t enc;
    long P;                                        // floats of `grad`
    long g_off[CM_MAX_LAYERS], w_off[CM_MAX_LAYERS];
    int F[CM_MAX_LAYERS], kh[CM_MAX_LAYERS], ke[CM_MAX_LAYERS], KB[CM_MAX_LAYERS];
};

// the layer stack's checks (the words of K13) and, for n.enc encoded columns, the geometry of `grad` (nn.Linear layout,
// unpadded) and of the packed buffer
int cmb_layout(const char* what, CmbNet& n, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers, int64_t skip_mask) {
    const int rc = cm_check_stack(what, output_dim, hidden_dim, mlp_layers, skip_mask);
    if (rc != VSX_OK) return rc;
    const long encp = cm_round_up(n.enc, 8);
    long g = 0, w = 0;
    for (int l = 0; l < mlp_layers; ++l) {
        const bool last = l == mlp_layers - 1, has_enc = cm_has_enc(l, skip_mask);
        n.F[l] = (int)(last ? output_dim : hidden_dim);
        n.kh[l] = l > 0 ? (int)hidden_dim : 0;
        n.ke[l] = has_enc ? (int)n.enc : 0;
        const long fp = last ? 32 : hidden_dim, kp = n.kh[l] + (has_enc ? encp : 0);
        n.KB[l] = (int)(kp / 8);
        n.g_off[l] = g, n.w_off[l] = w;
        g += (long)n.F[l] * (n.kh[l] + n.ke[l]) + n.F[l];
        w += fp * kp + fp;
    }
    n.P = g;
    return VSX_OK;
}

// a coordinate network: the option checks of K13, then cmb_layout
int cmb_net(const char* what, CmbNet& n, int64_t input_dim, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers,
            int64_t pe_type, int64_t pe_dim, int64_t mlp_type, int64_t skip_mask) {
    const int rc = cm_check_options(what, mlp_type, pe_type, input_dim, pe_dim, &n.enc);
    return rc != VSX_OK ? rc : cmb_layout(what, n, output_dim, hidden_dim, mlp_layers, skip_mask);
}

inline long cmb_chunks(long N) { return (N + CMB_ROWS - 1) / CMB_ROWS; }

inline long cmb_scratch_floats(const CmbNet& n, long N, int64_t output_dim, int64_t hidden_dim) {
    return cmb_chunks(N) * n.P + 2 * N * hidden_dim + N * output_dim;
}

// The 2 L + 1 launches of K16 for N > 0 rows, every buffer validated by the caller -> dZ_0 [N, hidden_dim] (in `scratch`):
// the gradient at layer 0's pre-activation, which K17 carries on into the encoding.
const float* cmb_chain(const CmbNet& n, const float* grad_out, int64_t N, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers,
                       int64_t use_tanh, const float* packed, const float* saved, float* scratch, float* grad, hipStream_t s) {
    const int L = (int)mlp_layers, hidden = (int)hidden_dim;
    const long chunks = cmb_chunks(N);
    float* partial = scratch;
    float* dzbuf[2] = {scratch + chunks * n.P, scratch + chunks * n.P + N * hidden};
    float* dz_out = dzbuf[1] + N * hidden;
    const float* saved_enc = saved + (long)(L - 1) * N * hidden;
    const float* saved_out = saved_enc + N * n.enc;
    const int waves = CMB_THREADS / 64;

    const long n_out = N * output_dim;
    hipLaunchKernelGGL(cmb_dz_out_kernel, dim3((unsigned)((n_out + CMB_THREADS - 1) / CMB_THREADS)), dim3(CMB_THREADS), 0, s, grad_out,
                       saved_out, dz_out, n_out, (int)(use_tanh != 0));
    const float* dz = dz_out;
    for (int l = L - 1; l >= 0; --l) {
        const float* h = l > 0 ? saved + (long)(l - 1) * N * hidden : nullptr;
        const int tiles = ((n.F[l] + 31) / 32) * (n.kh[l] / 32 + (n.ke[l] + 31) / 32 + 1);
        hipLaunchKernelGGL(cmb_wgrad_kernel, dim3((unsigned)chunks, (unsigned)((tiles + waves - 1) / waves)), dim3(CMB_THREADS), 0, s, dz,
                           n.F[l], h, n.kh[l], n.ke[l] ? saved_enc : nullptr, n.ke[l], (long)N, partial + n.g_off[l], n.P);
        if (l == 0) break;
        float* dh = dzbuf[l & 1];
        hipLaunchKernelGGL(cmb_dgrad_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)((hidden / 32 + waves - 1) / waves)),
                           dim3(CMB_THREADS), 0, s, dz, n.F[l], packed + n.w_off[l], n.KB[l], h, hidden, (long)N, dh);
        dz = dh;
    }
    hipLaunchKernelGGL(cmb_reduce_kernel, dim3((unsigned)((n.P + CMB_THREADS - 1) / CMB_THREADS)), dim3(CMB_THREADS), 0, s, partial, n.P,
                       chunks, grad);
    return dz;
}

}  // namespace

extern "C" int64_t vsx_coord_mlp_wgrad_rows(void) { return CMB_ROWS; }

extern "C" int vsx_coord_mlp_train_workspace(int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim,
                                             int64_t mlp_layers, int64_t pe_type, int64_t pe_dim, int64_t mlp_type,
                                             int64_t skip_mask, int64_t* saved_floats, int64_t* scratch_floats,
                                             int64_t* grad_floats) {
    CmbNet n;
    const int rc = cmb_net("coord_mlp_train_workspace", n, input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, mlp_type,
                           skip_mask);
    if (rc != VSX_OK) return rc;
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * CM_BM, VSX_E_BADSHAPE, "coord_mlp_train_workspace: N = %lld", (long long)N);
    if (saved_floats) *saved_floats = cm_saved_floats(N, n.enc, output_dim, hidden_dim, mlp_layers);
    if (scratch_floats) *scratch_floats = cmb_scratch_floats(n, N, output_dim, hidden_dim);
    if (grad_floats) *grad_floats = n.P;
    return VSX_OK;
}

extern "C" int vsx_coord_mlp_bwd_f32(const float* grad_out, int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim,
                                     int64_t mlp_layers, int64_t pe_type, int64_t pe_dim, int64_t mlp_type, int64_t skip_mask,
                                     int64_t use_tanh, const float* packed, int64_t packed_floats, const float* saved,
                                     int64_t saved_floats, float* scratch, int64_t scratch_floats, float* grad,
                                     int64_t grad_floats, vsx_stream_t stream) {
    const char* what = "coord_mlp_bwd";
    CmbNet n;
    const int rc = cmb_net(what, n, input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, mlp_type, skip_mask);
    if (rc != VSX_OK) return rc;
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * CM_BM, VSX_E_BADSHAPE, "%s: N = %lld", what, (long long)N);
    VSX_REQUIRE(grad, VSX_E_BADSHAPE, "%s: null argument", what);
    VSX_REQUIRE(grad_floats >= n.P, VSX_E_WORKSPACE, "%s: grad holds %lld floats, this network needs %lld", what,
                (long long)grad_floats, (long long)n.P);
    if (N == 0) {                                                  // no row, no launch: every gradient is zero
        const hipError_t e = hipMemsetAsync(grad, 0, (size_t)n.P * sizeof(float), (hipStream_t)stream);
        if (e != hipSuccess) return vsx_fail(VSX_E_LAUNCH, "%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
        return VSX_OK;
    }
    VSX_REQUIRE(grad_out && packed && saved && scratch, VSX_E_BADSHAPE, "%s: null argument", what);
    const int64_t need_packed = cm_packed_floats(n.enc, hidden_dim, mlp_layers, skip_mask);
    VSX_REQUIRE(packed_floats == need_packed, VSX_E_BADSHAPE, "%s: packed weights hold %lld floats, this network needs %lld", what,
                (long long)packed_floats, (long long)need_packed);
    const int64_t need_saved = cm_saved_floats(N, n.enc, output_dim, hidden_dim, mlp_layers);
    VSX_REQUIRE(saved_floats >= need_saved, VSX_E_WORKSPACE, "%s: saved holds %lld floats, N = %lld needs %lld", what,
                (long long)saved_floats, (long long)N, (long long)need_saved);
    const int64_t need_scratch = cmb_scratch_floats(n, N, output_dim, hidden_dim);
    VSX_REQUIRE(scratch_floats >= need_scratch, VSX_E_WORKSPACE, "%s: scratch holds %lld floats, N = %lld needs %lld", what,
                (long long)scratch_floats, (long long)N, (long long)need_scratch);

    cmb_chain(n, grad_out, N, output_dim, hidden_dim, mlp_layers, use_tanh, packed, saved, scratch, grad, (hipStream_t)stream);
    return vsx_check_launch("vsx_coord_mlp_bwd_f32");
}

// ------------------------------------------------------------------------------------------------
// K17: the gradients of the hash-grid texture network (K14): layer weights and biases by the K16 chain above on the activations
// the training forward of atlas.hip stored, then dEnc = dZ_0 W_0 over the encoded columns, then the grid backward: the table
// gradient (a scatter-add with fp32 atomics: NOT bit-reproducible) and the gradient of the input (no atomics).
// ------------------------------------------------------------------------------------------------
namespace {

// denc[row][k] = sum over f of dz[row][f] * W[f][k]  for k < E: cmb_dgrad_kernel without a mask, on the packed layer 0 (KB =
// round_up(E, 8) / 8 k-blocks).  A column >= E is neither read nor written; E need not be a multiple of 32.
__global__ __launch_bounds__(CMB_THREADS) void cmb_denc_kernel(const float* __restrict__ dz, int F, const float* __restrict__ wl, int KB,
                                                                int E, long N, float* __restrict__ denc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const int kt = blockIdx.y * (CMB_THREADS / 64) + wave;
    if (kt * 32 >= E) return;
    const long row0 = (long)blockIdx.x * 32, row = row0 + col;
    const bool rowok = row < N;
    const int k = kt * 32 + col;
    const bool kok = k < E;
    const float* wk = wl + ((long)(k >> 3) * 2 + ((k & 7) >> 2)) * 128 + (k & 3);

    f16v acc[4] = {cmb_zero(), cmb_zero(), cmb_zero(), cmb_zero()};
    for (int f0 = 0; f0 < F; f0 += 8) {
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = f0 + 4 * hi + j;             // F = hidden_dim, a multiple of 32: inside the packed layer
            a[j] = rowok && f < F ? dz[row * F + f] : 0.f;
            b[j] = kok ? wk[(long)(f >> 5) * KB * 256 + (f & 31) * 4] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const long orow = row0 + 8 * (i >> 2) + 4 * hi + (i & 3);
        if (orow < N && kok) denc[orow * E + k] = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
    }
}

// The grid backward, the thread mapping of the forward's encoding stage: row = tid & 63, wave w takes the levels 4 w .. 4 w + 3
// of every pass of 16.  Per row and level the cell comes from hg_cell, as in the forward.
//   grad_table (nullable): entry idx_c, feature f += weight_c * grad_enc[row][2 l + f]   (atomicAdd; the caller has zeroed it)
//   grad_x (nullable): per level, for d = 0, 1:  t_d = sum over f = 0, 1 of grad_enc[row][2 l + f] * s_df,  s_df = the sum over
//     the corners c = 0 .. 3, in that order, of fmaf(sign_dc * other_dc, table[idx_c][f], sum), sign_dc = +1 where bit d of c is
//     set, else -1, other_dc = the weight of c along the OTHER axis (w or 1 - w); a thread adds its levels in increasing order,
//     part_d = fmaf(scale_l, t_d, part_d); the four waves' parts meet in LDS and are added as ((p_0 + p_1) + p_2) + p_3.
// Rows past N and levels past n_levels neither read nor add.  Dynamic LDS: 4 * 64 * 2 floats.
__global__ __launch_bounds__(CM_THREADS) void hash_grid_bwd_kernel(const float* __restrict__ x, long N, const HashGrid g,
                                                                    const float* __restrict__ grad_enc, float* __restrict__ grad_table,
                                                                    float* __restrict__ grad_x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* part = reinterpret_cast<float*>(smem);                  // [4 waves][CM_BM rows][2]
    const int tid = threadIdx.x, r = tid & (CM_BM - 1), wave = tid >> 6, wl = __builtin_amdgcn_readfirstlane(wave);
    const long row = (long)blockIdx.x * CM_BM + r;
    const bool ok = row < N;
    const float x0 = ok ? x[row * 2] : 0.f, x1 = ok ? x[row * 2 + 1] : 0.f;
    const int E = 2 * g.n_levels;
    float px0 = 0.f, px1 = 0.f;
    for (int l0 = 0; l0 < g.n_levels; l0 += HG_PASS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int l = l0 + 4 * wl + j;
            if (!(ok && l < g.n_levels)) continue;
            const HgLevel lv = g.lv[l & (HG_MAX_LEVELS - 1)];
            float w0, w1;
            uint32_t idx[4];
            hg_cell(lv, x0, x1, w0, w1, idx);
            const float ga = grad_enc[row * E + 2 * l], gb = grad_enc[row * E + 2 * l + 1];
            if (grad_x) {
                float2 v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = g.table[idx[c]];
                float s0a = 0.f, s0b = 0.f, s1a = 0.f, s1b = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float o0 = (c >> 1) ? w1 : 1.f - w1, o1 = (c & 1) ? w0 : 1.f - w0;
                    const float d0 = (c & 1) ? o0 : -o0, d1 = (c >> 1) ? o1 : -o1;
                    s0a = fmaf(d0, v[c].x, s0a), s0b = fmaf(d0, v[c].y, s0b);
                    s1a = fmaf(d1, v[c].x, s1a), s1b = fmaf(d1, v[c].y, s1b);
                }
                px0 = fmaf(lv.scale, fmaf(gb, s0b, ga * s0a), px0);
                px1 = fmaf(lv.scale, fmaf(gb, s1b, ga * s1a), px1);
            }
            if (grad_table) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float w = hg_weight(c, w0, w1);
                    float* t = grad_table + (size_t)idx[c] * 2;
                    atomicAdd(t, w * ga);
                    atomicAdd(t + 1, w * gb);
                }
            }
        }
    }
    if (!grad_x) return;                                           // uniform: every thread of the grid leaves here
    part[(wave * CM_BM + r) * 2] = px0, part[(wave * CM_BM + r) * 2 + 1] = px1;
    __syncthreads();
    if (tid < 2 * CM_BM) {
        const long orow = (long)blockIdx.x * CM_BM + (tid >> 1);
        if (orow < N) grad_x[orow * 2 + (tid & 1)] = ((part[tid] + part[2 * CM_BM + tid]) + part[4 * CM_BM + tid]) + part[6 * CM_BM + tid];
    }
}

constexpr size_t HGB_LDS = 4 * CM_BM * 2 * sizeof(float);

// zero grad_table (when given), then, for N > 0, the one launch; everything validated
int hgb_launch(const char* what, const float* x, int64_t N, const HashGrid& g, const float* grad_enc, float* grad_table,
               int64_t table_floats, float* grad_x, hipStream_t s) {
    if (grad_table) {
        const hipError_t e = hipMemsetAsync(grad_table, 0, (size_t)table_floats * sizeof(float), s);
        if (e != hipSuccess) return vsx_fail(VSX_E_LAUNCH, "%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
    }
    if (N > 0 && (grad_table || grad_x))
        hipLaunchKernelGGL(hash_grid_bwd_kernel, dim3((unsigned)((N + CM_BM - 1) / CM_BM)), dim3(CM_THREADS), HGB_LDS, s, x, (long)N, g,
                           grad_enc, grad_table, grad_x);
    return VSX_OK;
}

inline long hmb_scratch_floats(const CmbNet& n, long N, int64_t output_dim, int64_t hidden_dim) {
    return cmb_scratch_floats(n, N, output_dim, hidden_dim) + N * n.enc;
}

}  // namespace

extern "C" int vsx_hash_mlp_train_workspace(int64_t N, int64_t input_dim, int64_t n_levels, int64_t n_features,
                                            int64_t log2_hashmap_size, int64_t base_resolution, double per_level_scale,
                                            int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers, int64_t skip_mask,
                                            int64_t* saved_floats, int64_t* scratch_floats, int64_t* grad_floats) {
    const char* what = "hash_mlp_train_workspace";
    HgLevel lv[HG_MAX_LEVELS];
    int64_t table_need = 0;
    int rc = hg_options(what, lv, &table_need, input_dim, n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale);
    if (rc != VSX_OK) return rc;
    CmbNet n;
    n.enc = n_levels * n_features;
    rc = cmb_layout(what, n, output_dim, hidden_dim, mlp_layers, skip_mask);
    if (rc != VSX_OK) return rc;
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * CM_BM, VSX_E_BADSHAPE, "%s: N = %lld", what, (long long)N);
    if (saved_floats) *saved_floats = cm_saved_floats(N, n.enc, output_dim, hidden_dim, mlp_layers);
    if (scratch_floats) *scratch_floats = hmb_scratch_floats(n, N, output_dim, hidden_dim);
    if (grad_floats) *grad_floats = n.P;
    return VSX_OK;
}

extern "C" int vsx_hash_grid_bwd_f32(const float* x, int64_t N, int64_t input_dim, const float* grad_enc, const float* table,
                                     int64_t table_floats, int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size,
                                     int64_t base_resolution, double per_level_scale, float* grad_table, float* grad_x,
                                     vsx_stream_t stream) {
    const char* what = "hash_grid_bwd";
    HashGrid g;
    const int rc = hg_fill(what, g, input_dim, table, table_floats, n_levels, n_features, log2_hashmap_size, base_resolution,
                           per_level_scale);
    if (rc != VSX_OK) return rc;
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * CM_BM, VSX_E_BADSHAPE, "%s: N = %lld", what, (long long)N);
    VSX_REQUIRE(!grad_table || vsx_aligned16(grad_table), VSX_E_BADSHAPE, "%s: grad_table must be 16-byte aligned", what);
    if (N == 0) return hgb_launch(what, x, 0, g, grad_enc, grad_table, table_floats, nullptr, (hipStream_t)stream);
    VSX_REQUIRE(x && grad_enc && table, VSX_E_BADSHAPE, "%s: null argument", what);
    VSX_REQUIRE(vsx_aligned16(table), VSX_E_BADSHAPE, "%s: the grid table must be 16-byte aligned", what);
    const int lrc = hgb_launch(what, x, N, g, grad_enc, grad_table, table_floats, grad_x, (hipStream_t)stream);
    return lrc != VSX_OK ? lrc : vsx_check_launch("vsx_hash_grid_bwd_f32");
}

extern "C" int vsx_hash_mlp_bwd_f32(const float* grad_out, const float* x, int64_t N, int64_t input_dim, const float* table,
                                    int64_t table_floats, int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size,
                                    int64_t base_resolution, double per_level_scale, int64_t output_dim, int64_t hidden_dim,
                                    int64_t mlp_layers, int64_t skip_mask, int64_t use_tanh, const float* packed,
                                    int64_t packed_floats, const float* saved, int64_t saved_floats, float* scratch,
                                    int64_t scratch_floats, float* grad, int64_t grad_floats, float* grad_table, float* grad_x,
                                    vsx_stream_t stream) {
    const char* what = "hash_mlp_bwd";
    HashGrid g;
    int rc = hg_fill(what, g, input_dim, table, table_floats, n_levels, n_features, log2_hashmap_size, base_resolution,
                     per_level_scale);
    if (rc != VSX_OK) return rc;
    CmbNet n;
    n.enc = n_levels * n_features;
    rc = cmb_layout(what, n, output_dim, hidden_dim, mlp_layers, skip_mask);
    if (rc != VSX_OK) return rc;
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * CM_BM, VSX_E_BADSHAPE, "%s: N = %lld", what, (long long)N);
    VSX_REQUIRE(grad, VSX_E_BADSHAPE, "%s: null argument", what);
    VSX_REQUIRE(!grad_table || vsx_aligned16(grad_table), VSX_E_BADSHAPE, "%s: grad_table must be 16-byte aligned", what);
    VSX_REQUIRE(grad_floats >= n.P, VSX_E_WORKSPACE, "%s: grad holds %lld floats, this network needs %lld", what,
                (long long)grad_floats, (long long)n.P);
    const hipStream_t s = (hipStream_t)stream;
    if (N == 0) {                                                  // no row, no launch: every gradient is zero
        const hipError_t e = hipMemsetAsync(grad, 0, (size_t)n.P * sizeof(float), s);
        if (e != hipSuccess) return vsx_fail(VSX_E_LAUNCH, "%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
        return hgb_launch(what, x, 0, g, nullptr, grad_table, table_floats, nullptr, s);
    }
    VSX_REQUIRE(grad_out && x && table && packed && saved && scratch, VSX_E_BADSHAPE, "%s: null argument", what);
    VSX_REQUIRE(vsx_aligned16(table), VSX_E_BADSHAPE, "%s: the grid table must be 16-byte aligned", what);
    const int64_t need_packed = cm_packed_floats(n.enc, hidden_dim, mlp_layers, skip_mask);
    VSX_REQUIRE(packed_floats == need_packed, VSX_E_BADSHAPE, "%s: packed weights hold %lld floats, this network needs %lld", what,
                (long long)packed_floats, (long long)need_packed);
    const int64_t need_saved = cm_saved_floats(N, n.enc, output_dim, hidden_dim, mlp_layers);
    VSX_REQUIRE(saved_floats >= need_saved, VSX_E_WORKSPACE, "%s: saved holds %lld floats, N = %lld needs %lld", what,
                (long long)saved_floats, (long long)N, (long long)need_saved);
    const int64_t need_scratch = hmb_scratch_floats(n, N, output_dim, hidden_dim);
    VSX_REQUIRE(scratch_floats >= need_scratch, VSX_E_WORKSPACE, "%s: scratch holds %lld floats, N = %lld needs %lld", what,
                (long long)scratch_floats, (long long)N, (long long)need_scratch);

    const float* dz0 = cmb_chain(n, grad_out, N, output_dim, hidden_dim, mlp_layers, use_tanh, packed, saved, scratch, grad, s);
    if (grad_table || grad_x) {
        float* denc = scratch + cmb_scratch_floats(n, N, output_dim, hidden_dim);
        const int waves = CMB_THREADS / 64, E = (int)n.enc;
        hipLaunchKernelGGL(cmb_denc_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)(((E + 31) / 32 + waves - 1) / waves)),
                           dim3(CMB_THREADS), 0, s, dz0, (int)hidden_dim, packed + n.w_off[0], n.KB[0], E, (long)N, denc);
        rc = hgb_launch(what, x, N, g, denc, grad_table, table_floats, grad_x, s);
        if (rc != VSX_OK) return rc;
    }
    return vsx_check_launch("vsx_hash_mlp_bwd_f32");
}
