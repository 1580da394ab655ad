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
#include <math.h>

#include "common.h"

namespace {

constexpr int CM_BM = 64;            // rows per workgroup
constexpr int CM_THREADS = 256;
constexpr int CM_MAX_LAYERS = 8;
constexpr int CM_MAX_ENC = 64;       // encoded input columns (2 * input_dim * pe_dim), padded to a multiple of 8

struct CoordMlpParams {
    const float* x;
    const float* w;                  // packed weights and biases (vsx.h)
    float* out;
    long N;
    int in_dim, out_dim, hidden, layers;
    int pe_dim;                      // 0: pe_type none
    int enc, encp;                   // encoded columns, and padded to 8
    int skip_mask, use_tanh;
    int w_off[CM_MAX_LAYERS], b_off[CM_MAX_LAYERS];   // in floats, multiples of 4
};

// acc[f][r] += W[tile ft[f]][kb0 .. kb0 + nkb) * lds[.. nkb)  for the wave's NF feature tiles and NR row tiles.
// wl: the layer's packed weight, KB its k-blocks per feature tile; lds: the k-block 0 of this part, [q][CM_BM] float4.
template <int NF, int NR>
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
    for (int kb = 0; kb < nkb; ++kb) {
        f4v wc[NF], a[NR];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            wc[f] = wn[f];
            if (kb + 1 < nkb) wn[f] = wp[f][(long)(kb + 1) * 64];
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) a[r] = ap[2 * kb * CM_BM + r * 32];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    acc[f][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[f][s], a[r][s], acc[f][r], 0, 0, 0);
    }
}

template <int NF, int NR>
__device__ __forceinline__ void cm_layer(f16v (&acc)[2][2], const CoordMlpParams& p, int l, const f4v* act, const f4v* enc,
                                         const int (&ft)[2], int rt0, int lane) {
    const int kbh = l > 0 ? p.hidden / 8 : 0;
    const int kbe = (l == 0 || ((p.skip_mask >> l) & 1)) ? p.encp / 8 : 0;
    const float* wl = p.w + p.w_off[l];
    // torch.cat((x, input), 1): the hidden columns first, then the encoded input
    if (kbh) cm_accumulate<NF, NR>(acc, wl, kbh + kbe, 0, kbh, act, ft, rt0, lane);
    if (kbe) cm_accumulate<NF, NR>(acc, wl, kbh + kbe, kbh, kbe, enc, ft, rt0, lane);
}

__global__ __launch_bounds__(CM_THREADS) void coord_mlp_kernel(const CoordMlpParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f4v* act = reinterpret_cast<f4v*>(smem);                       // [hidden / 4][CM_BM]
    f4v* enc = act + (p.hidden / 4) * CM_BM;                       // [encp / 4][CM_BM]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * CM_BM;

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
            cm_layer<1, 1>(acc, p, l, act, enc, ft, rt0, lane);
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
                    }
                }
            }
        }
        __syncthreads();
    }
}

inline long cm_round_up(long x, long m) { return (x + m - 1) / m * m; }

// floats of the packed weight buffer (vsx.h), arguments already validated
long cm_packed_floats(int64_t input_dim, int64_t hidden_dim, int64_t mlp_layers, int64_t pe_type, int64_t pe_dim,
                      int64_t skip_mask) {
    const long encp = cm_round_up(pe_type == 1 ? 2 * input_dim * pe_dim : input_dim, 8);
    long total = 0;
    for (int l = 0; l < mlp_layers; ++l) {
        const long fp = l == mlp_layers - 1 ? 32 : hidden_dim;
        const long kp = (l > 0 ? hidden_dim : 0) + ((l == 0 || ((skip_mask >> l) & 1)) ? encp : 0);
        total += fp * kp + fp;
    }
    return total;
}

}  // namespace

extern "C" int vsx_coord_mlp_f32(const float* x, int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim,
                                 int64_t mlp_layers, int64_t pe_type, int64_t pe_dim, int64_t mlp_type, int64_t skip_mask,
                                 int64_t use_tanh, const float* packed, int64_t packed_floats, float* out,
                                 vsx_stream_t stream) {
    VSX_REQUIRE(mlp_type == 0, VSX_E_UNSUPPORTED, "coord_mlp: mlp_type 'tcnn' (%lld) is not implemented, only 'origin'",
                (long long)mlp_type);
    VSX_REQUIRE(pe_type == 0 || pe_type == 1, VSX_E_UNSUPPORTED,
                "coord_mlp: pe_type 'hash_encoding' (%lld) is not implemented, only 'none' and 'encoding'", (long long)pe_type);
    VSX_REQUIRE(input_dim == 2 || input_dim == 3, VSX_E_UNSUPPORTED, "coord_mlp: input_dim %lld (2 or 3)", (long long)input_dim);
    VSX_REQUIRE(output_dim >= 1 && output_dim <= 3, VSX_E_UNSUPPORTED, "coord_mlp: output_dim %lld (1 to 3)", (long long)output_dim);
    VSX_REQUIRE(hidden_dim >= 32 && hidden_dim <= 256 && hidden_dim % 32 == 0, VSX_E_UNSUPPORTED,
                "coord_mlp: hidden_dim %lld (a multiple of 32 up to 256)", (long long)hidden_dim);
    VSX_REQUIRE(mlp_layers >= 2 && mlp_layers <= CM_MAX_LAYERS, VSX_E_UNSUPPORTED, "coord_mlp: mlp_layers %lld (2 to 8)",
                (long long)mlp_layers);
    const long enc = pe_type == 1 ? 2 * input_dim * pe_dim : input_dim;
    VSX_REQUIRE(pe_type == 0 || (pe_dim >= 1 && enc <= CM_MAX_ENC), VSX_E_UNSUPPORTED,
                "coord_mlp: pe_dim %lld (2 * input_dim * pe_dim must be 1 to %d)", (long long)pe_dim, CM_MAX_ENC);
    VSX_REQUIRE(skip_mask >= 0 && (skip_mask & 1) == 0 && (skip_mask >> mlp_layers) == 0, VSX_E_UNSUPPORTED,
                "coord_mlp: skip_layers must lie in 1 .. mlp_layers - 1 (mask 0x%llx)", (long long)skip_mask);
    VSX_REQUIRE(N >= 0 && N < (1ll << 31) * CM_BM, VSX_E_BADSHAPE, "coord_mlp: N = %lld", (long long)N);
    if (N == 0) return VSX_OK;
    VSX_REQUIRE(x && packed && out, VSX_E_BADSHAPE, "coord_mlp: null argument");
    VSX_REQUIRE(vsx_aligned16(packed), VSX_E_BADSHAPE, "coord_mlp: packed weights must be 16-byte aligned");
    const int64_t need = cm_packed_floats(input_dim, hidden_dim, mlp_layers, pe_type, pe_dim, skip_mask);
    VSX_REQUIRE(packed_floats == need, VSX_E_BADSHAPE, "coord_mlp: packed weights hold %lld floats, this network needs %lld",
                (long long)packed_floats, (long long)need);

    CoordMlpParams p;
    p.x = x, p.w = packed, p.out = out, p.N = N;
    p.in_dim = (int)input_dim, p.out_dim = (int)output_dim, p.hidden = (int)hidden_dim, p.layers = (int)mlp_layers;
    p.pe_dim = pe_type == 1 ? (int)pe_dim : 0;
    p.enc = (int)enc, p.encp = (int)cm_round_up(enc, 8);
    p.skip_mask = (int)skip_mask, p.use_tanh = use_tanh != 0;
    long off = 0;
    for (int l = 0; l < CM_MAX_LAYERS; ++l) {
        p.w_off[l] = p.b_off[l] = 0;
        if (l >= mlp_layers) continue;
        const long fp = l == mlp_layers - 1 ? 32 : hidden_dim;
        const long kp = (l > 0 ? hidden_dim : 0) + ((l == 0 || ((skip_mask >> l) & 1)) ? p.encp : 0);
        p.w_off[l] = (int)off, p.b_off[l] = (int)(off + fp * kp);
        off += fp * kp + fp;
    }
    const size_t smem = (size_t)(p.hidden + p.encp) * CM_BM * sizeof(float);     // <= 80 KiB: two workgroups per CU
    static size_t smem_attr = 64 * 1024;
    if (smem > smem_attr) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&coord_mlp_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return vsx_fail(VSX_E_LAUNCH, "coord_mlp: hipFuncSetAttribute: %s", hipGetErrorString(e));
        smem_attr = 160 * 1024;
    }
    hipLaunchKernelGGL(coord_mlp_kernel, dim3((unsigned)((N + CM_BM - 1) / CM_BM)), dim3(CM_THREADS), smem,
                       (hipStream_t)stream, p);
    return vsx_check_launch("vsx_coord_mlp_f32");
}
