// K13: fused coordinate MLP of the layered neural atlas (IMLP_Hash.forward with mlp_type 'origin',
// videoswap/atlas/implicit_neural_networks.py:164-195): optional sin/cos encoding, up to 8 Linear layers with ReLU between
// them, skip concatenation of the encoded input, optional tanh — one launch for N rows, exact fp32.
//
// One workgroup (4 waves) owns 64 rows.  The activations of those rows never leave the CU: they live in LDS as
// act[k / 4][row][k % 4] (a float4 per row and group of four features), the encoded input next to them in the same layout
// for layer 0 and the skip layers.  A layer is the product  D^T[feature][row] = W[feature][k] * act^T[k][row]  on
// v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulate, one rounding per product): the A operand is the weight, one
// 16-byte global load per lane and block of 8 k (the host packs W for exactly that, see vsx.h), the B operand one 16-byte
// LDS read.  A lane's 16 results of a 32x32 tile are 4 x 4 CONSECUTIVE features of ONE row, so the epilogue (bias, ReLU)
// writes float4s straight back into the layout the next layer reads.  Weights are not staged in LDS: at 64 cycles per MFMA
// a wave needs 16 bytes per lane of weight every 256 ... 512 cycles, which the L2 (all layers of a network: <= 2 MB) delivers
// with one k-block of prefetch; every weight is read once per workgroup and layer.
//
// Work split of a layer with nft = out_features / 32 feature tiles and 2 row tiles: nft > 2: wave w owns feature tiles
// w and w + 4, both row tiles (64 accumulator registers); nft <= 2 (hidden 32 / 64 and the output layer, padded to 32
// features): wave w owns feature tile w / 2, row tile w % 2.
//
// K14: the same kernel behind a multiresolution hash grid (tiny-cuda-nn's HashGrid, Linear interpolation, 2-D input, 2
// features per level: the texture network F_Atlas), and the grid alone.  The kernel is a template on the encoding; the grid
// instantiation fills `enc` by gathering the four corners of every level straight from the table in global memory (21 MB
// for the reference's configuration: it is not staged in LDS) and runs the same layer loop.  The definition of the grid
// (level geometry: hg_geometry; lookup: hg_encode4) is RESTATED from the published algorithm and has not been compared
// with tinycudann.
#include <math.h>

#include "coord_mlp.h"
#include "hash_grid.h"

namespace {

struct CoordMlpParams {
    const float* x;
    const float* w;                  // packed weights and biases (vsx.h)
    float* out;
    float* saved;                    // the training instantiation's stores (vsx.h K16); unused otherwise
    long N;
    int in_dim, out_dim, hidden, layers;
    int pe_dim;                      // 0: pe_type none
    int enc, encp;                   // encoded columns, and padded to 8
    int skip_mask, use_tanh;
    int w_off[CM_MAX_LAYERS], b_off[CM_MAX_LAYERS];   // in floats, multiples of 4
};

// The two features of the levels l0 .. l0 + 3 at (x0, x1): f[j] = sum over the four corners of the cell, in corner order,
// of weight * table entry; the cell, its entries and its weights are hg_cell's (hash_grid.h).  `ok` false (row past N) or a
// level past n_levels: nothing is gathered, the features are zero.  The 16 eight-byte loads are issued before the first use.
__device__ __forceinline__ void hg_encode4(const HashGrid& g, int l0, bool ok, float x0, float x1, float2 (&f)[4]) {
    float2 v[4][4];
    float w0[4], w1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = l0 + j;
        const HgLevel lv = g.lv[l & (HG_MAX_LEVELS - 1)];
        const bool use = ok && l < g.n_levels;
        uint32_t idx[4];
        hg_cell(lv, x0, x1, w0[j], w1[j], idx);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[j][c] = use ? g.table[idx[c]] : float2{0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float w = hg_weight(c, w0[j], w1[j]);
            a = fmaf(w, v[j][c].x, a), b = fmaf(w, v[j][c].y, b);
        }
        f[j] = float2{a, b};
    }
}

// acc[f][r] += W[tile ft[f]][kb0 .. kb0 + nkb) * lds[.. nkb)  for the wave's NF feature tiles and NR row tiles.
// wl: the layer's packed weight, KB its k-blocks per feature tile; lds: the k-block 0 of this part, [q][CM_BM] float4.
// S = 4 (one feature tile, one row tile only: 16 of the 64 accumulator registers are in use): the four MFMAs of a k-block
// go to four partial sums that are added pairwise at the end, so a summation chain is K / 4 long instead of K and the
// rounding error of the sum is that of a blocked CPU GEMM; S = 1: one chain over k, in order.
template <int NF, int NR, int S>
__device__ __forceinline__ void cm_accumulate(f16v (&acc)[2][2], const float* __restrict__ wl, int KB, int kb0, int nkb,
                                              const f4v* lds, const int (&ft)[2], int rt0, int lane) {
    const f4v* wp[NF];
    f4v wn[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        wp[f] = reinterpret_cast<const f4v*>(wl) + ((long)ft[f] * KB + kb0) * 64 + lane;
        wn[f] = wp[f][0];
    }
    const f4v* ap = lds + (lane >> 5) * CM_BM + rt0 * 32 + (lane & 31);
    static_assert(S == 1 || (S == 4 && NF == 1 && NR == 1), "partial sums: one tile per wave only");
    f16v part[S > 1 ? S - 1 : 1];
    if constexpr (S > 1) {
#pragma unroll
        for (int q = 0; q < S - 1; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) part[q][i] = 0.f;
    }
    for (int kb = 0; kb < nkb; ++kb) {
        f4v wc[NF], a[NR];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            wc[f] = wn[f];
            if (kb + 1 < nkb) wn[f] = wp[f][(long)(kb + 1) * 64];
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) a[r] = ap[2 * kb * CM_BM + r * 32];
        if constexpr (S > 1) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[0][0], a[0][0], acc[0][0], 0, 0, 0);
#pragma unroll
            for (int s = 1; s < 4; ++s) part[s - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[0][s], a[0][s], part[s - 1], 0, 0, 0);
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int r = 0; r < NR; ++r)
                        acc[f][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[f][s], a[r][s], acc[f][r], 0, 0, 0);
        }
    }
    if constexpr (S > 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[0][0][i] = (acc[0][0][i] + part[0][i]) + (part[1][i] + part[2][i]);
    }
}

template <int NF, int NR, int S = 1>
__device__ __forceinline__ void cm_layer(f16v (&acc)[2][2], const CoordMlpParams& p, int l, const f4v* act, const f4v* enc,
                                         const int (&ft)[2], int rt0, int lane) {
    const int kbh = l > 0 ? p.hidden / 8 : 0;
    const int kbe = (l == 0 || ((p.skip_mask >> l) & 1)) ? p.encp / 8 : 0;
    const float* wl = p.w + p.w_off[l];
    // torch.cat((x, input), 1): the hidden columns first, then the encoded input
    if (kbh) cm_accumulate<NF, NR, S>(acc, wl, kbh + kbe, 0, kbh, act, ft, rt0, lane);
    if (kbe) cm_accumulate<NF, NR, S>(acc, wl, kbh + kbe, kbh, kbe, enc, ft, rt0, lane);
}

// Train: the same arithmetic, and every row < N also stores what the backward reads (vsx.h K16 / K17): the encoded input
// (behind the hash grid: the two features of every level), every hidden layer's activation after its ReLU, and the output.
template <class Grid, bool Train = false>
__global__ __launch_bounds__(CM_THREADS) void coord_mlp_kernel(const CoordMlpParams p, const Grid g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f4v* act = reinterpret_cast<f4v*>(smem);                       // [hidden / 4][CM_BM]
    f4v* enc = act + (p.hidden / 4) * CM_BM;                       // [encp / 4][CM_BM]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * CM_BM;

    if constexpr (Grid::kHash) {
        // hash grid: row = tid & 63, wave w takes the levels 4 w .. 4 w + 3 of every pass of 16; the two features of level
        // l are the columns 2 l, 2 l + 1; rows past N (no gather) and the levels up to encp / 2 are zero
        const int r = tid & (CM_BM - 1), wl = __builtin_amdgcn_readfirstlane(wave);
        const bool ok = row0 + r < p.N;
        const float x0 = ok ? p.x[(row0 + r) * 2] : 0.f, x1 = ok ? p.x[(row0 + r) * 2 + 1] : 0.f;
        for (int l0 = 0; 2 * l0 < p.encp; l0 += HG_PASS) {
            float2 f[4];
            hg_encode4(g, l0 + 4 * wl, ok, x0, x1, f);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 2 * (l0 + 4 * wl + j);
                if (e < p.encp) *reinterpret_cast<float2*>(reinterpret_cast<float*>(enc) + ((e >> 2) * CM_BM + r) * 4 + (e & 3)) = f[j];
                if constexpr (Train) {
                    if (ok && e < p.enc)
                        *reinterpret_cast<float2*>(p.saved + (long)(p.layers - 1) * p.N * p.hidden + (row0 + r) * p.enc + e) = f[j];
                }
            }
        }
    } else {
        // the encoded input (positionalEncoding_vec: for each frequency 2^j pi the sines of all inputs, then the cosines), or
        // the raw coordinates; rows past N and the padding columns are zero
        for (int idx = tid; idx < p.encp * CM_BM; idx += CM_THREADS) {
            const int r = idx & (CM_BM - 1), e = idx / CM_BM;
            float v = 0.f;
            if (e < p.enc && row0 + r < p.N) {
                const float* xr = p.x + (row0 + r) * p.in_dim;
                if (p.pe_dim == 0) {
                    v = xr[e];
                } else {
                    const int j = e / (2 * p.in_dim), rem = e - j * 2 * p.in_dim;
                    const bool is_cos = rem >= p.in_dim;
                    const float arg = xr[is_cos ? rem - p.in_dim : rem] * ldexpf(3.14159274101257324f, j);   // fp32 (2^j pi)
                    v = is_cos ? cosf(arg) : sinf(arg);
                }
            }
            reinterpret_cast<float*>(enc)[((e >> 2) * CM_BM + r) * 4 + (e & 3)] = v;
            if constexpr (Train) {
                if (e < p.enc && row0 + r < p.N) p.saved[(long)(p.layers - 1) * p.N * p.hidden + (row0 + r) * p.enc + e] = v;
            }
        }
    }
    __syncthreads();

    for (int l = 0; l < p.layers; ++l) {
        const bool last = l == p.layers - 1;
        const int nft = last ? 1 : p.hidden / 32;
        int ft[2], rt0, nf, nr;
        if (nft <= 2) {
            ft[0] = wave >> 1, ft[1] = 0, rt0 = wave & 1, nr = 1;
            nf = ft[0] < nft ? 1 : 0;
        } else {
            ft[0] = wave, ft[1] = wave + 4, rt0 = 0, nr = 2;
            nf = ft[1] < nft ? 2 : (ft[0] < nft ? 1 : 0);
        }
        f16v acc[2][2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[f][r][i] = 0.f;
        if (nf == 2)
            cm_layer<2, 2>(acc, p, l, act, enc, ft, rt0, lane);
        else if (nf == 1 && nr == 2)
            cm_layer<1, 2>(acc, p, l, act, enc, ft, rt0, lane);
        else if (nf == 1)
            cm_layer<1, 1, Grid::kHash ? 4 : 1>(acc, p, l, act, enc, ft, rt0, lane);   // the output layer, and hidden <= 64
        const float* bias = p.w + p.b_off[l];
        if (last) {
            // features 0 .. out_dim - 1 of row (lane & 31): registers 0 .. 2 of the lanes 0 .. 31
            const long row = row0 + rt0 * 32 + (lane & 31);
            if (nf == 1 && lane < 32 && row < p.N) {
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    if (s < p.out_dim) {
                        float v = acc[0][0][s] + bias[s];
                        if (p.use_tanh) v = tanhf(v);
                        p.out[row * p.out_dim + s] = v;
                        if constexpr (Train) p.saved[((long)(p.layers - 1) * p.hidden + p.enc) * p.N + row * p.out_dim + s] = v;
                    }
                }
            }
            break;
        }
        __syncthreads();                                           // every wave has read this layer's input
#pragma unroll
        for (int f = 0; f < 2; ++f) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (f < nf && r < nr) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int fb = ft[f] * 32 + 8 * g + 4 * (lane >> 5);
                        const f4v b = *reinterpret_cast<const f4v*>(bias + fb);
                        f4v v;
#pragma unroll
                        for (int s = 0; s < 4; ++s) v[s] = fmaxf(acc[f][r][4 * g + s] + b[s], 0.f);   // ReLU before the next layer
                        act[(fb >> 2) * CM_BM + (rt0 + r) * 32 + (lane & 31)] = v;
                        if constexpr (Train) {
                            const long row = row0 + (rt0 + r) * 32 + (lane & 31);
                            if (row < p.N) *reinterpret_cast<f4v*>(p.saved + ((long)l * p.N + row) * p.hidden + fb) = v;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// the grid alone: out[row][2 l + f], the thread mapping of the fused kernel's encoding stage; rows past N neither gather
// nor store
__global__ __launch_bounds__(CM_THREADS) void hash_grid_kernel(const float* __restrict__ x, long N, const HashGrid g,
                                                               float* __restrict__ out) {
    const int tid = threadIdx.x, r = tid & (CM_BM - 1), wl = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long row = (long)blockIdx.x * CM_BM + r;
    const bool ok = row < N;
    const float x0 = ok ? x[row * 2] : 0.f, x1 = ok ? x[row * 2 + 1] : 0.f;
    for (int l0 = 0; l0 < g.n_levels; l0 += HG_PASS) {
        float2 f[4];
        hg_encode4(g, l0 + 4 * wl, ok, x0, x1, f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int l = l0 + 4 * wl + j;
            if (ok && l < g.n_levels) *reinterpret_cast<float2*>(out + row * (2 * g.n_levels) + 2 * l) = f[j];
        }
    }
}

// The layer stack's half of an entry point: validates it (every message under `what`; the unsupported options before
// N == 0, which the CALLER answers with VSX_OK after this returns VSX_OK) and fills the kernel arguments for `enc` encoded
// columns; pe_dim 0: the columns are not the sin/cos encoding.
int cm_prepare(const char* what, CoordMlpParams& p, const float* x, int64_t N, int64_t input_dim, int64_t output_dim,
               int64_t hidden_dim, int64_t mlp_layers, int64_t pe_dim, int64_t enc, int64_t skip_mask, int64_t use_tanh,
               const float* packed, int64_t packed_floats, float* out) {
    const int src = cm_check_stack(what, output_dim, hidden_dim, mlp_layers, skip_mask);
    if (src != VSX_OK) return src;
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * CM_BM, VSX_E_BADSHAPE, "%s: N = %lld", what, (long long)N);
    if (N == 0) return VSX_OK;
    VSX_REQUIRE(x && packed && out, VSX_E_BADSHAPE, "%s: null argument", what);
    VSX_REQUIRE(vsx_aligned16(packed), VSX_E_BADSHAPE, "%s: packed weights must be 16-byte aligned", what);
    const int64_t need = cm_packed_floats(enc, hidden_dim, mlp_layers, skip_mask);
    VSX_REQUIRE(packed_floats == need, VSX_E_BADSHAPE, "%s: packed weights hold %lld floats, this network needs %lld", what,
                (long long)packed_floats, (long long)need);

    p.x = x, p.w = packed, p.out = out, p.saved = nullptr, p.N = N;
    p.in_dim = (int)input_dim, p.out_dim = (int)output_dim, p.hidden = (int)hidden_dim, p.layers = (int)mlp_layers;
    p.pe_dim = (int)pe_dim;
    p.enc = (int)enc, p.encp = (int)cm_round_up(enc, 8);
    p.skip_mask = (int)skip_mask, p.use_tanh = use_tanh != 0;
    long off = 0;
    for (int l = 0; l < CM_MAX_LAYERS; ++l) {
        p.w_off[l] = p.b_off[l] = 0;
        if (l >= mlp_layers) continue;
        const long fp = l == mlp_layers - 1 ? 32 : hidden_dim;
        const long kp = (l > 0 ? hidden_dim : 0) + (cm_has_enc(l, skip_mask) ? p.encp : 0);
        p.w_off[l] = (int)off, p.b_off[l] = (int)(off + fp * kp);
        off += fp * kp + fp;
    }
    return VSX_OK;
}

template <class Grid, bool Train = false>
int cm_launch(const char* what, const CoordMlpParams& p, const Grid& g, vsx_stream_t stream) {
    const size_t smem = (size_t)(p.hidden + p.encp) * CM_BM * sizeof(float);     // <= 80 KiB: two workgroups per CU
    static size_t smem_attr = 64 * 1024;
    if (smem > smem_attr) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&coord_mlp_kernel<Grid, Train>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return vsx_fail(VSX_E_LAUNCH, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
        smem_attr = 160 * 1024;
    }
    hipLaunchKernelGGL((coord_mlp_kernel<Grid, Train>), dim3((unsigned)((p.N + CM_BM - 1) / CM_BM)), dim3(CM_THREADS), smem,
                       (hipStream_t)stream, p, g);
    return vsx_check_launch(what);
}

}  // namespace

extern "C" int vsx_coord_mlp_f32(const float* x, int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim,
                                 int64_t mlp_layers, int64_t pe_type, int64_t pe_dim, int64_t mlp_type, int64_t skip_mask,
                                 int64_t use_tanh, const float* packed, int64_t packed_floats, float* out,
                                 vsx_stream_t stream) {
    int64_t enc = 0;
    const int orc = cm_check_options("coord_mlp", mlp_type, pe_type, input_dim, pe_dim, &enc);
    if (orc != VSX_OK) return orc;
    CoordMlpParams p;
    const int rc = cm_prepare("coord_mlp", p, x, N, input_dim, output_dim, hidden_dim, mlp_layers, pe_type == 1 ? pe_dim : 0, enc,
                              skip_mask, use_tanh, packed, packed_floats, out);
    if (rc != VSX_OK || N == 0) return rc;
    return cm_launch("vsx_coord_mlp_f32", p, NoGrid{}, stream);
}

// K16, the forward half: vsx_coord_mlp_f32 with the stores of the training instantiation
extern "C" int vsx_coord_mlp_fwd_train_f32(const float* x, int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim,
                                           int64_t mlp_layers, int64_t pe_type, int64_t pe_dim, int64_t mlp_type,
                                           int64_t skip_mask, int64_t use_tanh, const float* packed, int64_t packed_floats,
                                           float* out, float* saved, int64_t saved_floats, vsx_stream_t stream) {
    int64_t enc = 0;
    const int orc = cm_check_options("coord_mlp_fwd_train", mlp_type, pe_type, input_dim, pe_dim, &enc);
    if (orc != VSX_OK) return orc;
    CoordMlpParams p;
    const int rc = cm_prepare("coord_mlp_fwd_train", p, x, N, input_dim, output_dim, hidden_dim, mlp_layers,
                              pe_type == 1 ? pe_dim : 0, enc, skip_mask, use_tanh, packed, packed_floats, out);
    if (rc != VSX_OK || N == 0) return rc;
    VSX_REQUIRE(saved && vsx_aligned16(saved), VSX_E_BADSHAPE, "coord_mlp_fwd_train: saved must be a 16-byte aligned buffer");
    const int64_t need = cm_saved_floats(N, enc, output_dim, hidden_dim, mlp_layers);
    VSX_REQUIRE(saved_floats >= need, VSX_E_WORKSPACE, "coord_mlp_fwd_train: saved holds %lld floats, N = %lld needs %lld",
                (long long)saved_floats, (long long)N, (long long)need);
    p.saved = saved;
    return cm_launch<NoGrid, true>("vsx_coord_mlp_fwd_train_f32", p, NoGrid{}, stream);
}

extern "C" int64_t vsx_hash_grid_geometry(int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size,
                                          int64_t base_resolution, double per_level_scale, float* scale, uint32_t* res,
                                          uint32_t* entries, uint32_t* offset, uint32_t* hashed) {
    HgLevel lv[HG_MAX_LEVELS];
    const int64_t floats = hg_geometry("hash_grid", n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale, lv);
    for (int l = 0; floats >= 0 && l < n_levels; ++l) {
        if (scale) scale[l] = lv[l].scale;
        if (res) res[l] = lv[l].res;
        if (entries) entries[l] = lv[l].entries;
        if (offset) offset[l] = lv[l].offset;
        if (hashed) hashed[l] = lv[l].hashed;
    }
    return floats;
}

extern "C" int vsx_hash_grid_f32(const float* x, int64_t N, int64_t input_dim, const float* table, int64_t table_floats,
                                 int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size, int64_t base_resolution,
                                 double per_level_scale, float* out, vsx_stream_t stream) {
    HashGrid g;
    const int rc = hg_fill("hash_grid", g, input_dim, table, table_floats, n_levels, n_features, log2_hashmap_size,
                           base_resolution, per_level_scale);
    if (rc != VSX_OK) return rc;
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * CM_BM, VSX_E_BADSHAPE, "hash_grid: N = %lld", (long long)N);
    if (N == 0) return VSX_OK;
    VSX_REQUIRE(x && table && out, VSX_E_BADSHAPE, "hash_grid: null argument");
    VSX_REQUIRE(vsx_aligned16(table), VSX_E_BADSHAPE, "hash_grid: the grid table must be 16-byte aligned");
    VSX_REQUIRE((((uintptr_t)out) & 7) == 0, VSX_E_BADSHAPE, "hash_grid: out must be 8-byte aligned");
    hipLaunchKernelGGL(hash_grid_kernel, dim3((unsigned)((N + CM_BM - 1) / CM_BM)), dim3(CM_THREADS), 0, (hipStream_t)stream,
                       x, (long)N, g, out);
    return vsx_check_launch("vsx_hash_grid_f32");
}

extern "C" int vsx_hash_mlp_f32(const float* x, int64_t N, int64_t input_dim, const float* table, int64_t table_floats,
                                int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size, int64_t base_resolution,
                                double per_level_scale, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers,
                                int64_t skip_mask, int64_t use_tanh, const float* packed, int64_t packed_floats, float* out,
                                vsx_stream_t stream) {
    HashGrid g;
    const int rc = hg_fill("hash_mlp", g, input_dim, table, table_floats, n_levels, n_features, log2_hashmap_size,
                           base_resolution, per_level_scale);
    if (rc != VSX_OK) return rc;
    // the table's own checks, ahead of the packed buffer's as they always were; N <= 0 is cm_prepare's to answer
    VSX_REQUIRE(N <= 0 || table, VSX_E_BADSHAPE, "hash_mlp: null argument");
    VSX_REQUIRE(N <= 0 || vsx_aligned16(table), VSX_E_BADSHAPE, "hash_mlp: the grid table must be 16-byte aligned");
    CoordMlpParams p;
    const int prc = cm_prepare("hash_mlp", p, x, N, 2, output_dim, hidden_dim, mlp_layers, 0, n_levels * n_features, skip_mask,
                               use_tanh, packed, packed_floats, out);
    if (prc != VSX_OK || N == 0) return prc;
    return cm_launch("vsx_hash_mlp_f32", p, g, stream);
}

// K17, the forward half: vsx_hash_mlp_f32 with the stores of the training instantiation
extern "C" int vsx_hash_mlp_fwd_train_f32(const float* x, int64_t N, int64_t input_dim, const float* table, int64_t table_floats,
                                          int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size, int64_t base_resolution,
                                          double per_level_scale, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers,
                                          int64_t skip_mask, int64_t use_tanh, const float* packed, int64_t packed_floats, float* out,
                                          float* saved, int64_t saved_floats, vsx_stream_t stream) {
    HashGrid g;
    const int rc = hg_fill("hash_mlp_fwd_train", g, input_dim, table, table_floats, n_levels, n_features, log2_hashmap_size,
                           base_resolution, per_level_scale);
    if (rc != VSX_OK) return rc;
    VSX_REQUIRE(N <= 0 || table, VSX_E_BADSHAPE, "hash_mlp_fwd_train: null argument");
    VSX_REQUIRE(N <= 0 || vsx_aligned16(table), VSX_E_BADSHAPE, "hash_mlp_fwd_train: the grid table must be 16-byte aligned");
    CoordMlpParams p;
    const int prc = cm_prepare("hash_mlp_fwd_train", p, x, N, 2, output_dim, hidden_dim, mlp_layers, 0, n_levels * n_features,
                               skip_mask, use_tanh, packed, packed_floats, out);
    if (prc != VSX_OK || N == 0) return prc;
    VSX_REQUIRE(saved && vsx_aligned16(saved), VSX_E_BADSHAPE, "hash_mlp_fwd_train: saved must be a 16-byte aligned buffer");
    const int64_t need = cm_saved_floats(N, n_levels * n_features, output_dim, hidden_dim, mlp_layers);
    VSX_REQUIRE(saved_floats >= need, VSX_E_WORKSPACE, "hash_mlp_fwd_train: saved holds %lld floats, N = %lld needs %lld",
                (long long)saved_floats, (long long)N, (long long)need);
    p.saved = saved;
    return cm_launch<HashGrid, true>("vsx_hash_mlp_fwd_train_f32", p, g, stream);
}
