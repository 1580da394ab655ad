/*
 * vsx.h — C ABI of libvsx.so, the MI355X (gfx950) denoising-path kernels for VideoSwap.
 *
 * This is the drop-in boundary of the hot path: the Python host classes in
 * videoswap_amd/ (same names and call signatures as the reference's UNet / Attention / pipeline
 * classes) bind exactly these entry points through ctypes.  Nothing here takes a torch type:
 * plain device pointers, sizes, element strides and the hipStream_t to launch on.
 *
 * Contract (all entry points):
 *   - every tensor is fp16 (IEEE binary16) in device memory unless stated; accumulation is fp32;
 *   - the CALLER owns all memory (inputs, outputs, workspaces); the library never allocates or
 *     frees device memory and never synchronises; every call is asynchronous on `stream`;
 *   - return 0 (VSX_OK) on success, a negative VSX_E_* code otherwise; vsx_last_error() returns a
 *     thread-local description of the last failure; no exception crosses the ABI;
 *   - pointers must be 16-byte aligned and row strides multiples of 8 elements (16-byte vector
 *     access) unless a function says otherwise; violations return VSX_E_BADSHAPE;
 *   - activations are channels-last: a video tensor the reference holds as [B,C,F,H,W]
 *     (reference videoswap/models/animatediff_models/resnet.py:12-16) lives here as
 *     [B*F, H, W, C] == token matrix [B*F*H*W, C].
 *
 * Each entry point cites the reference call site it replaces (file:line into showlab/VideoSwap).
 */
#ifndef VSX_H_
#define VSX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_ABI_VERSION 17

#define VSX_OK 0
#define VSX_E_BADSHAPE (-1)
#define VSX_E_UNSUPPORTED (-2)
#define VSX_E_LAUNCH (-3)
#define VSX_E_WORKSPACE (-4)

typedef void* vsx_stream_t; /* hipStream_t */

int vsx_abi_version(void);
const char* vsx_last_error(void);
/* sha256 (hex) of the kernel sources + flags the library was built from; the Python loader compares it with the
 * sources it sits next to and refuses a stale binary. */
const char* vsx_source_digest(void);
/* Tuning / test switch (process-wide, not thread-safe against concurrent launches): "gemm_pp" = 0 never / 1 default /
 * 2 always-when-eligible use of the persistent ping-pong GEMM kernel; "pp_sched" = its option bits (8: linear tile walk; 4: convolutions sum K
 * tap-major like the tile kernels instead of taps-inner; 16: a private A slab per convolution tap; 32: common piece order in every CU).  Results
 * are identical for every setting except bit 4 (same arithmetic; bit 4 selects another fp32 summation order of the same products).
 * "tile_tune" (diagnostics, tools/small_m_sweep.py) forces a tile / ring depth / K-slice count of the workgroup-per-tile kernels.
 * "conv_winograd" = 0 never / 1 default / 2 always-when-supported: what vsx_conv3x3_winograd_auto answers (below). */
int vsx_set_option(const char* name, int64_t value);
/* ABI 15: the current value of an option (its environment variable's, or the default, until vsx_set_option); an unknown name fails
 * like vsx_set_option. */
int vsx_get_option(const char* name, int64_t* value);

/* ------------------------------------------------------------------------------------------
 * K1/K2: MFMA GEMM / implicit-GEMM convolution with fused epilogues.
 *   C[z][m, n] = epilogue( alpha * sum_k A[z][m, k] * B[z][n, k] )        (both operands K-major)
 * Replaces: nn.Linear / 1x1 nn.Conv2d (attention.py:65,93; motion_module.py:113,136; diffusers
 * Attention.to_q/k/v/out, FeedForward), InflatedConv3d 3x3 (resnet.py:9-18), Downsample3D
 * (resnet.py:83), Upsample3D nearest-2x + conv (resnet.py:54,66), the channel concat of the up
 * blocks (unet_blocks.py:618,720), torch.baddbmm/bmm of get_attention_scores / probs @ V
 * (attention_register.py:70-76,150-156).
 * All integer fields are 64-bit so the struct has no padding on any ABI.
 * ------------------------------------------------------------------------------------------ */
typedef struct vsx_gemm_desc {
    int64_t M, N, K;     /* N = output columns (for geglu: N = K_out = half of B's rows) */
    int64_t batch0, batch1; /* grid.z = batch0*batch1; z0 = z / batch1, z1 = z % batch1 */

    /* A operand */
    const void* A;       /* a_mode 0: [M,K] row-major, row stride lda; a_mode 1: NHWC image(s) */
    const void* A2;      /* a_mode 1 only: second source concatenated on C (may be NULL) */
    int64_t lda, a_bs0, a_bs1;
    int64_t a_mode;      /* 0 = plain rows, 1 = implicit im2col of a ks x ks conv, pad ks/2 */
    int64_t H, W;        /* a_mode 1: logical input height/width (after the optional 2x upsample) */
    int64_t C1, C2;      /* a_mode 1: channels of A and A2 (C2 = 0 without A2); K = ks*ks*(C1+C2).  Multiples of 8;
                            with A2 both must be multiples of 64 (one K slab never straddles the two sources) */
    int64_t ks, stride;  /* a_mode 1: kernel size 1 or 3, stride 1 or 2 */
    int64_t upsample;    /* a_mode 1: 1 = A/A2 are [.., H/2, W/2, C], read as nearest-2x upsampled.
                            ABI v9: 2 = the same convolution in its SUB-PIXEL form (Upsample3D, resnet.py:54,66): a 3x3 window on
                            the upsampled image meets 2 x 2 source pixels, so output pixel (2i+ph, 2j+pw) is a 2x2-tap window on
                            the source with the coinciding filter rows / columns added up.  B = FOUR [N, 9 C] matrices, class
                            2 ph + pw first to last, whose taps (ph.., pw..) of a pad-1 3x3 window on the source hold the sums
                            (videoswap_amd.ops.subpixel_weights); 4/9 of the multiplications.  ks 3, stride 1, one source with
                            C1 % 64 == 0, bias only, N % 320 == 0, M/4 a multiple of 256 and a launch large enough for the
                            persistent kernel — VSX_E_UNSUPPORTED otherwise (use upsample = 1). */

    /* B operand: [N (or 2N for geglu), K] row-major (PyTorch Linear weight / OHWI conv weight) */
    const void* B;
    int64_t ldb, b_bs0, b_bs1;

    /* C */
    void* C;
    int64_t ldc, c_bs0, c_bs1;
    int64_t c_mode;         /* 0: C[m*ldc+n]; 1: transposed per image: C[img*c_img_stride + n*ldc + m%rows] */
    int64_t c_rows_per_img; /* c_mode 1: rows (tokens) per image */
    int64_t c_img_stride;   /* c_mode 1: element stride between images */

    /* epilogue */
    const void* bias;     /* [N] (geglu: [2N]) or NULL */
    const void* rowvec;   /* [ceil(M/rows_per_vec), N] added to row m from row m/rows_per_vec, or NULL
                             (time-embedding broadcast, resnet.py:172-176) */
    int64_t rows_per_vec;
    const void* residual; /* [M,N] with row stride ldr added after everything else, or NULL */
    int64_t ldr, r_bs0, r_bs1;
    int64_t geglu;        /* 1: out[m,n] = (acc_h+b_h) * gelu_erf(acc_g+b_g), h=row n, g=row N+n of B
                             (diffusers GEGLU used at attention.py:204, motion_module.py:218) */
    double alpha;
    /* optional split-K workspace (fp32 partial sums), caller-allocated: vsx_gemm_workspace(d) bytes, or NULL.  Small-M
       / long-K problems (the 8x8 and 16x16 UNet levels) are then sliced along K so that every CU gets a tile. */
    void* workspace;
    int64_t workspace_bytes;
    /* ABI v4, a_mode 1: zero padding before (top / left) and after (bottom / right) the image, 0..ks-1 each; the
       pair (-1, -1) selects the symmetric ks/2 of nn.Conv2d(padding=ks//2).  diffusers' VAE encoder downsamples with
       F.pad(x, (0, 1, 0, 1)) + a stride-2 conv without padding = (pad_lo, pad_hi) = (0, 1). */
    int64_t pad_lo, pad_hi;
    /* ABI v7: LayerNorm folded into the Linear that consumes it (attention.py:182,199,205 norm1/2/3 -> to_q/k/v, GEGLU;
       motion_module.py:213,219).  With W' = W o gamma as the B operand and A = the RAW activation,
           LN(x) W^T + b  =  rstd_m * acc[m,n]  -  rstd_m * mean_m * c1[n]  +  (beta W^T + b)[n]
       rowscale = fp32 [M][2] = (rstd_m, -rstd_m * mean_m) (vsx_row_stats), colvec = fp32 [N] (geglu: [2N]) = c1[n] =
       sum_k W'[n,k]; the last term is passed as `bias`, the temporal positional encoding pe W^T as `rowvec`.  The
       normalised tensor is never written or re-read.  Plain (a_mode 0), unbatched GEMMs only; NULL / NULL = off. */
    const void* rowscale;
    const void* colvec;
    /* ABI v8: row statistics of the OUTPUT, for a LayerNorm that follows this Linear (the producer side of the fold above:
       every LayerNorm input of the UNet is the output of a GEMM — proj_in, attention to_out + residual; attention.py:182,
       199,205, motion_module.py:213,219).  rowstats = fp32 [M][rowstats_parts][2] = (sum, sum of squares) of the ROUNDED
       fp16 outputs of row m over column part p, written by the epilogue that stores them; vsx_row_stats_combine turns the
       parts into the [M][2] rowscale of the consumer (one pass over 48 bytes per row instead of vsx_row_stats' pass over
       the whole row).  Only the persistent kernel emits them (plain GEMM, N a multiple of 320, epilogue = bias and / or
       residual or row vector): ASK FIRST with vsx_gemm_rowstats_parts(d) — the number of parts this launch will write
       (6 per 320 columns on the persistent kernel, one per wave — 10, or 5 — on the weight-stationary K = 320 kernel), 0 = it will not (keep rowstats NULL and use vsx_row_stats).  NULL / 0 = off. */
    void* rowstats;
    int64_t rowstats_parts;
} vsx_gemm_desc;

int vsx_gemm_f16(const vsx_gemm_desc* d, vsx_stream_t stream);
/* ABI 15: the status vsx_gemm_f16(d, stream) would return under the current options (the same checks and the same plan: one piece of
   code), without launching anything and without touching the memory d points at.  A caller that can describe a launch in two forms asks
   before it builds what only one of them needs (videoswap_amd.ops.conv2d: upsample = 2, else the nine-tap form). */
int vsx_gemm_check(const vsx_gemm_desc* d);
/* ABI 16: WHICH kernel vsx_gemm_f16(d, stream) would launch under the current options: the same checks and the same plan again
   (one piece of code), no HIP call, nothing d points at is read.  Returns the status of vsx_gemm_check(d) and writes
     out[0] family: 0 weight-stationary K = 320 kernel, 1 persistent 256-row tiles, 2 persistent 128-row tiles, 3 a workgroup-per-tile
            kernel; -1 where no plan was made (d fails the descriptor checks, or M == 0), the other seven are then 0
     out[1], out[2] BM, BN: the tile (32 x 320 row blocks for family 0, 256 / 128 x 320 for families 1 / 2)
     out[3] deep: the four-slot ring of the 128 x 160 tile
     out[4], out[5] splits, nk_per: K slices (1 = no split-K) and 64-wide K slabs per slice (0 without a split); d->workspace decides as
            in the launch (vsx_gemm_workspace says how much it takes)
     out[6] stat_parts: vsx_gemm_rowstats_parts(d)
     out[7] refused: 0, or why the launch is VSX_E_UNSUPPORTED although a kernel was chosen (1: the sub-pixel form off the persistent
            kernel, 2: rowstats_parts is not what the launch writes).
   For tests that aim a shape at one kernel's edge, and tools that report what ran. */
int vsx_gemm_plan(const vsx_gemm_desc* d, int64_t out[8]);
/* parts per row the launch described by d would write into d->rowstats (see above); the answer does not depend on
   d->rowstats / d->rowstats_parts themselves */
int64_t vsx_gemm_rowstats_parts(const vsx_gemm_desc* d);
/* bytes of `workspace` with which vsx_gemm_f16(d) takes the split-K path under the current options; 0: it would not split whatever it
   is given (another kernel takes the problem, or d does not pass the checks of vsx_gemm_f16) */
int64_t vsx_gemm_workspace(const vsx_gemm_desc* d);

/* Winograd F(2x2, 3x3) form of the stride-1 3x3 convolution (InflatedConv3d 3x3 of the resnets, resnet.py:9-18,170,181):
 * the SAME description as vsx_gemm_f16 would take, computed as an input transform V = B^T d B ([16][M/4][C1+C2]), sixteen
 * GEMMs [M/4, C1+C2] x [N, C1+C2]^T in one batched vsx_gemm_f16 launch, and an output transform A^T Mt A followed by the
 * direct path's epilogue in its order (+ bias, + rowvec row, + residual last): 16 multiplications per 2 x 2 output tile
 * and channel pair instead of 36 (csrc/winograd.hip).  fp32 transform arithmetic; V, U, Mt and the output are rounded to
 * fp16 once each, so the result differs from vsx_gemm_f16's by rounding (about twice its error against fp64).
 *   U: the transformed weights G g G^T, fp16 [16][N][C1+C2] (xi = 4 a + b outermost), made by the caller from B =
 *      [N, 3, 3, C1+C2] (videoswap_amd.ops.winograd_weights); d->B is not read.
 *   workspace: caller-allocated, 16-byte aligned, vsx_conv3x3_winograd_workspace(d) bytes (V, then Mt); that function
 *      returns 0 for a description this form does not take.  V is fp16 [16][M/4][C1+C2] at the start, Mt fp16 [16][M/4][N]
 *      right behind it (xi = 4 a + b outermost in both; tile = (image, row / 2, column / 2), row-major).  The call writes
 *      every element of both and clears nothing: both can be read back after it (tests/winograd_case.py does).
 *   Supported: a_mode 1, ks 3, stride 1, upsample 0, symmetric padding 1 (pad_lo = pad_hi = -1 or 1), H and W even, no
 *      batch, C1 / C2 / N multiples of 8 (two sources: C1, C2 multiples of 64), ldc / ldr multiples of 8, alpha 1,
 *      epilogue = bias / rowvec / residual.  Anything else: VSX_E_UNSUPPORTED; the library never falls back by itself.
 * vsx_conv3x3_winograd_auto(d): 1 where the caller should take this form under the current options ("conv_winograd":
 *   0 never, 1 = supported, (C1 + C2 >= 640 and H * W <= 256) or (C1 + C2 >= 1280 and H * W <= 1024), and no GEMM back end
 *   forced through "gemm_pp" / "tile_tune", 2 = whenever supported), else 0. */
int64_t vsx_conv3x3_winograd_workspace(const vsx_gemm_desc* d);
int64_t vsx_conv3x3_winograd_auto(const vsx_gemm_desc* d);
int vsx_conv3x3_winograd_f16(const vsx_gemm_desc* d, const void* U, void* workspace, int64_t workspace_bytes,
                             vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K3: GroupNorm over channels-last activations, two kernels.
 *   x = concat_C(x1[nimg, rows, C1], x2[nimg, rows, C2]); statistics per (img, group) over
 *   rows x (C/groups).  nimg = B and rows = F*H*W reproduces the reference's 5-D GroupNorm
 *   (resnet.py:166,177; unet.py:474: statistics pooled over frames); nimg = B*F, rows = H*W the
 *   per-frame one (attention.py:108; motion_module.py:146).
 * vsx_groupnorm_stats writes fp32 partial sums partial[img][chunk][group][2] (sum, sumsq) with
 * chunk count = vsx_groupnorm_chunks(rows, nimg); vsx_groupnorm_apply reduces them (deterministic
 * order) into stats[nimg][groups][2] = (mean, rstd) (fp32 workspace, caller-allocated) and writes
 * y = (x-mean)*rstd*gamma+beta (optionally SiLU) as one [nimg, rows, C1+C2].
 * In frame-sharded mode the caller all-reduces `partial` between the two calls and passes the
 * GLOBAL element count in `count_rows`.
 * ------------------------------------------------------------------------------------------ */
int64_t vsx_groupnorm_chunks(int64_t rows, int64_t nimg);
int vsx_groupnorm_stats(const void* x1, const void* x2, int64_t nimg, int64_t rows, int64_t C1,
                        int64_t C2, int64_t groups, float* partial, vsx_stream_t stream);
int vsx_groupnorm_apply(const void* x1, const void* x2, int64_t nimg, int64_t rows, int64_t C1,
                        int64_t C2, int64_t groups, const float* partial, int64_t nchunks,
                        int64_t count_rows, const void* gamma, const void* beta, float eps,
                        int64_t silu, float* stats, void* y, vsx_stream_t stream);

/* Row statistics of x[M, C] for a LayerNorm folded into its consumer GEMM (vsx_gemm_desc.rowscale):
 * stats[m] = (rstd_m, -rstd_m * mean_m), rstd = 1/sqrt(var + eps), fp32 statistics as in vsx_layernorm. */
int vsx_row_stats(const void* x, int64_t M, int64_t C, float eps, float* stats, vsx_stream_t stream);
/* the same stats[m] from the partial sums a producing GEMM wrote (vsx_gemm_desc.rowstats): parts [M][nparts][2] fp32 =
 * (sum, sum of squares) over disjoint column parts that cover the C columns; variance = E[x^2] - mean^2 in fp32. */
int vsx_row_stats_combine(const float* parts, int64_t M, int64_t nparts, int64_t C, float eps, float* stats,
                          vsx_stream_t stream);

/* K4: LayerNorm over the last dim of x[M, C] (attention.py:182,199,205; motion_module.py:213,219).
 * If pe != NULL, adds pe[((m / rows_per_frame) % frames) + frame_offset][c] (fp16 [max_len, C]) to
 * the normalised row: the AnimateDiff temporal positional encoding (motion_module.py:253-255,
 * 291-292) fused so that no '(b f) d c -> (b d) f c' copy is needed. */
int vsx_layernorm(const void* x, int64_t M, int64_t C, const void* gamma, const void* beta,
                  float eps, const void* pe, int64_t rows_per_frame, int64_t frames,
                  int64_t frame_offset, void* y, vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K5/K6: fused attention O = softmax(Q K^T * scale) V, online softmax, MFMA, never
 * materialising the scores.  Replaces F.scaled_dot_product_attention (diffusers AttnProcessor2_0,
 * the default processor of attention.py:174-194) and xformers.memory_efficient_attention
 * (edlora_util.py:61; attention_register.py:67,147).
 *   Q  [nb, nq, heads*d]  row stride ldq     K [nkvb, nk, heads*d] row stride ldk
 *   VT [nkvb, heads*d, ldvt] = V transposed per image (written by vsx_gemm_f16 c_mode 1);
 *       ldvt >= round_up(nk, 8)
 *   O  [nb, nq, heads*d]  row stride ldo
 * image b uses K/V image b / kv_div (kv_div = frames for cross-attention where the text
 * embedding is shared by all frames: the reference repeats it, attention.py:100-103).
 * d in {8,16,32,40,64,80,128,160}.  scale > 0 and finite (the kernel takes the row max before scaling);
 * anything else is VSX_E_BADSHAPE and nothing is launched.
 * ------------------------------------------------------------------------------------------ */
int vsx_attention_f16(const void* Q, const void* K, const void* VT, void* O, int64_t nb,
                      int64_t heads, int64_t nq, int64_t nk, int64_t d, int64_t ldq, int64_t ldk,
                      int64_t ldvt, int64_t ldo, int64_t q_bs, int64_t k_bs, int64_t vt_bs,
                      int64_t o_bs, int64_t kv_div, float scale, vsx_stream_t stream);

/* Training form of K5/K6 (ABI 8; the adapter training step differentiates through every attention of the frozen UNet,
 * trainer_videoswap.py:33-97):
 *   vsx_attention_lse_f16: the same forward, additionally writing lse[b][h][q] (fp32, row length lse_ld >= nq) = log2 of
 *       the softmax denominator in the scaled-score domain: P[q][k] = exp2(scale * log2(e) * q.k - lse[q]).
 *   vsx_attention_bwd_f16: dQ (and, when dK / dV are given, dK and dV) from dO WITHOUT materialising the [heads, nq, nk]
 *       probabilities: P is recomputed tile by tile from lse, dS = scale * P o (dO V^T - delta), delta[q] = dO[q].O[q]
 *       (computed here into the caller's `delta` buffer), dQ = dS K, dK = dS^T Q, dV = P^T dO; two MFMA kernels, no atomics.
 *       Q, O, dO, dQ [nb, nq, heads*d]; K, V, dK, dV [nb / kv_div, nk, heads*d]: all contiguous rows.
 *       QT, dOT [nb, heads*d, ldtq], KT [nb / kv_div, heads*d, ldtk]: per-image transposes, rows zero-padded to a multiple
 *       of 8 (QT / dOT only for dK / dV); lse, delta [nb, heads, lds], lds a multiple of 64, zero beyond nq.
 *       kv_div > 1 (text K / V shared by the frames of a clip): dQ only.  d in {40, 64, 80}
 *       (vsx_attention_bwd_supported); other head dims keep the materialised path of videoswap_amd/autograd.py.
 *   Both require scale > 0 and finite, as vsx_attention_f16 (VSX_E_BADSHAPE otherwise, nothing launched). */
int vsx_attention_lse_f16(const void* Q, const void* K, const void* VT, void* O, float* lse, int64_t lse_ld, int64_t nb,
                          int64_t heads, int64_t nq, int64_t nk, int64_t d, int64_t ldq, int64_t ldk, int64_t ldvt,
                          int64_t ldo, int64_t q_bs, int64_t k_bs, int64_t vt_bs, int64_t o_bs, int64_t kv_div,
                          float scale, vsx_stream_t stream);
int64_t vsx_attention_bwd_supported(int64_t d);
int vsx_attention_bwd_f16(const void* Q, const void* K, const void* V, const void* O, const void* dO, const void* QT,
                          const void* KT, const void* dOT, const float* lse, float* delta, void* dQ, void* dK, void* dV,
                          int64_t nb, int64_t heads, int64_t nq, int64_t nk, int64_t d, int64_t ldtq, int64_t ldtk,
                          int64_t lds, int64_t kv_div, float scale, vsx_stream_t stream);

/* K7 helper: in-place row softmax of fp16 scores S[nrows, ld] over the first ncols columns
 * (diffusers Attention.get_attention_scores softmax; probs are then handed to the
 * Prompt-to-Prompt controller, attention_register.py:70-76). */
int vsx_softmax_rows(void* S, int64_t nrows, int64_t ncols, int64_t ld, vsx_stream_t stream);
/* causal variant for the CLIP text encoder (transformers CLIPAttention with causal_attention_mask): row r is query
 * r % rows_per_seq and attends to columns <= that index; the other columns get probability 0. */
int vsx_softmax_rows_causal(void* S, int64_t nrows, int64_t ncols, int64_t ld, int64_t rows_per_seq,
                            vsx_stream_t stream);

/* K8: temporal self-attention across frames at every spatial site (motion_module.py:287-338),
 * computed directly on the [B, F, HW, heads*d] layout (no transposes).  q/k/v/o share row
 * stride ld.  In frame-sharded mode q holds the local fq frames and k/v the gathered fk frames.
 * Any finite scale: all three kernels scale the scores before they take the row max. */
int vsx_temporal_attention_f16(const void* Q, const void* K, const void* V, void* O, int64_t B,
                               int64_t fq, int64_t fk, int64_t hw, int64_t heads, int64_t d,
                               int64_t ldq, int64_t ldkv, int64_t ldo, float scale,
                               vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K11: element-wise glue.
 * ------------------------------------------------------------------------------------------ */
/* y = silu(x) (resnet.py:172: nonlinearity(temb)) ; n elements */
int vsx_silu(const void* x, void* y, int64_t n, vsx_stream_t stream);
/* y = x * sigmoid(1.702 x): CLIP's quick_gelu (text encoder MLP; edlora_util.py:144 runs it 16 x per prompt) */
int vsx_quick_gelu(const void* x, void* y, int64_t n, vsx_stream_t stream);
/* y = a + s*b (adapter residual add, unet_blocks.py:399-402; unet.py:434-438) */
int vsx_axpy(const void* a, const void* b, float s, void* y, int64_t n, vsx_stream_t stream);
/* Latent layout conversion at the UNet boundary.
 * pack:   x[B,Cin,F,H,W] -> y[B*F,H,W,Cpad] (channels >= Cin zero-filled), unet.py:411
 * unpack: x[B*F,H,W,Cs] (first Cout channels) -> y[B,Cout,F,H,W], unet.py:476 */
int vsx_pack_latents(const void* x, void* y, int64_t B, int64_t Cin, int64_t F, int64_t HW,
                     int64_t Cpad, vsx_stream_t stream);
int vsx_unpack_latents(const void* x, void* y, int64_t B, int64_t Cout, int64_t F, int64_t HW,
                       int64_t Cs, vsx_stream_t stream);
/* Classifier-free guidance + DDIM update in one pass (pipeline_videoswap.py:578-580,587 and the
 * diffusers DDIMScheduler.step / DDIMInverseScheduler.step arithmetic, eta = 0):
 *   eps = eps_u + g*(eps_c - eps_u)   (eps_c == NULL: eps = eps_u)
 *   x0  = (x - sqrt(1-a_t) eps)/sqrt(a_t);  out = sqrt(a_n) x0 + sqrt(1-a_n) eps
 * with fp32 arithmetic, fp16 storage. */
int vsx_cfg_ddim_step(const void* x, const void* eps_u, const void* eps_c, float guidance,
                      float alpha_t, float alpha_next, void* out, int64_t n, vsx_stream_t stream);
/* Latent blend of the Prompt-to-Prompt SpatialBlender (spatial_blend.py:142):
 * out = src + mask*(x - src); mask fp16 broadcast over channels: x,src [C, n_sp], mask [n_sp].
 * A mask of exactly 0 returns src and a mask of exactly 1 returns x, bit for bit. */
int vsx_masked_blend(const void* x, const void* src, const void* mask, void* out, int64_t C,
                     int64_t n_sp, vsx_stream_t stream);

/* K10: SparsePointAdapter scatter (adapter_model.py:25-47,112-131): for every visible point p in
 * frame f splat feat[p,:]*w onto the 4 bilinear corners (clamped to the edge, accumulating) of
 * out[f, y, x, :] (channels-last, fp16, must be zero-filled by the caller).
 * tracks [F,P,2] fp32 pixel coords (x,y); negative = invisible; selected[P] int32 0/1. */
int vsx_adapter_scatter(const float* tracks, const int32_t* selected, const void* feat, void* out,
                        int64_t F, int64_t P, int64_t C, int64_t h, int64_t w, float rate,
                        float out_scale, vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Launch-time instrumentation used by bench.py: when enabled, vsx_gemm_f16 brackets each of its
 * launches with hipEvents on the launch stream (at most `max_samples` launches are sampled;
 * on = k > 1 brackets every k-th launch only: the two event packets cost a few microseconds per
 * launch, 5 % of the whole loop when every launch is bracketed).
 * vsx_prof_collect synchronises those events and returns the number of sampled launches, their
 * summed duration (ms) and summed algorithmic FLOP (2*M*N*K*batch; geglu counts B's 2N rows).
 * ------------------------------------------------------------------------------------------ */
int vsx_prof_enable(int64_t on, int64_t max_samples);
/* suspend (1) / resume (0) the sampling: events cannot be recorded while a stream is being captured into a HIP graph */
int vsx_prof_pause(int64_t paused);
int vsx_prof_collect(int64_t* n_launches, double* total_ms, double* total_flop);
/* ABI 10: the same collection priced against BOTH rooflines.  Per sampled launch the algorithmic bytes are A once + weights
 * once + C once + residual once (a convolution reads every input pixel once); a launch cannot finish before
 * max(FLOP / peak_flops, bytes / peak_bytes_per_s).  floor_ms = the sum of those floors over the sampled launches (so
 * floor_ms / total_ms is the fraction of the ATTAINABLE rate the launch mix reached), byte_bound_ms = the measured time of the
 * launches whose byte floor is the larger of the two.  Like vsx_prof_collect it consumes the samples. */
int vsx_prof_collect_roofline(double peak_flops, double peak_bytes_per_s, int64_t* n_launches, double* total_ms,
                              double* total_flop, double* total_bytes, double* floor_ms, double* byte_bound_ms);

/* ------------------------------------------------------------------------------------------
 * RCCL collectives of the frame-sharded long-clip mode (the reference has no
 * counterpart: it cannot run clips longer than 24 frames, motion_module.py:237-255).  One
 * communicator per process (= per GPU).  Rank 0 calls vsx_comm_unique_id and distributes the 128
 * bytes out of band (torch.distributed store, MPI, a file); every rank then calls vsx_comm_init.
 * librccl is opened with dlopen at the first call: libvsx.so has no link-time dependency on it.
 * Collectives are asynchronous on `stream`; the caller orders them against compute with events.
 *   vsx_allgather_kv:  kv_local [batch][elems_per_batch] fp16 (the K|V rows of this rank's frames,
 *       elems_per_batch = f_local*hw*2C) -> kv_all [batch][nranks][elems_per_batch]: per batch item
 *       the ranks' frame slabs in rank order = the [B, F_total, hw, 2C] tensor
 *       vsx_temporal_attention_f16 reads with fk = F_total (K = columns [0,C), V = [C,2C), ldkv = 2C);
 *   vsx_allgather_f32: fp32 GroupNorm partial sums (vsx_groupnorm_stats) of every rank, rank order;
 *       vsx_groupnorm_apply then reduces them in a fixed order: identical statistics on every rank;
 *   vsx_allreduce_gnstats: in-place fp32 sum over the ranks;
 *   vsx_alltoall_f16: the frames <-> sites re-shard of FrameShard(exchange='sites') (everything between a motion
 *       module's proj_in and proj_out is local to a SITE, motion_module.py:138-162,222-234) as ONE group of
 *       ncclSend / ncclRecv straight from / into the strided activation layouts (no pack / unpack passes): for every
 *       peer p and block (o, i), o < nouter, i < ninner, `block_elems` contiguous fp16 elements travel from
 *           send + p*send_strides[0] + o*send_strides[1] + i*send_strides[2]   on this rank   to
 *           recv + r*recv_strides[0] + o*recv_strides[1] + i*recv_strides[2]   on rank p   (r = this rank; strides in
 *       elements).  frames -> sites ([B, f, P, hw/P, C] -> [B, P, f, hw/P, C]): nouter = B, ninner = f,
 *       block = hw/P*C, send strides (block, f*P*block, P*block), recv strides (f*block, P*f*block, block);
 *       sites -> frames is the same call with the two stride triples exchanged.
 *
 * Recording communicator (ABI 8): vsx_comm_init_recording(rank, nranks) makes this process rank `rank` of `nranks`
 * WITHOUT librccl: the collectives above run their argument checks, stride arithmetic, group structure and peer loop
 * unchanged, but every ncclSend / ncclRecv / ncclAllGather / ncclAllReduce / local copy is appended to a log instead
 * of being executed (no device work, the buffers are never dereferenced).  vsx_comm_recorded(out, capacity) drains the
 * log (out == NULL: number of pending records): 6 int64 per record = op (VSX_COMM_OP_*), peer (-1: none), source
 * offset, destination offset (ELEMENTS from the entry point's first / second buffer argument; -1: n/a), element count,
 * element size.  Replaying the logs of all ranks against each other (NCCL matching: the k-th send of rank a to rank b
 * meets the k-th receive of b from a) reproduces what a P-GPU node would do: tests/test_distributed.py checks the
 * result against FrameShard's layouts for P = 2, 4, 8 — the multi-rank marshalling of this ABI on a box with one GPU
 * or none.  vsx_comm_destroy ends the recording.
 * ------------------------------------------------------------------------------------------ */
#define VSX_COMM_OP_SEND 1
#define VSX_COMM_OP_RECV 2
#define VSX_COMM_OP_ALLGATHER 3   /* destination block of rank q at dst offset + q * count */
#define VSX_COMM_OP_ALLREDUCE 4
#define VSX_COMM_OP_LOCAL_COPY 5
#define VSX_COMM_OP_GROUP_START 6
#define VSX_COMM_OP_GROUP_END 7
int vsx_comm_unique_id(void* id128);
int vsx_comm_init(int64_t rank, int64_t nranks, const void* id128);
int vsx_comm_init_recording(int64_t rank, int64_t nranks);
int64_t vsx_comm_recorded(int64_t* out, int64_t capacity);
int64_t vsx_comm_size(void);
int64_t vsx_comm_rank(void);
int vsx_comm_destroy(void);
int vsx_allgather_kv(const void* kv_local, void* kv_all, int64_t batch, int64_t elems_per_batch,
                     vsx_stream_t stream);
int vsx_allgather_f32(const float* local, float* all, int64_t count, vsx_stream_t stream);
int vsx_allreduce_gnstats(float* partial, int64_t count, vsx_stream_t stream);
int vsx_alltoall_f16(const void* send, void* recv, int64_t nouter, int64_t ninner, int64_t block_elems,
                     const int64_t* send_strides, const int64_t* recv_strides, vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gradient path of the adapter training step (trainer_videoswap.py:33-97 —
 * `accelerator.backward(loss)` through the frozen UNet into the SparsePointAdapter, adapter_model.py:70-107).
 * Only DATA gradients are needed (the UNet's weights are frozen); the matrix work of the backward pass (linear /
 * conv dgrad, attention products, the adapter MLP's weight gradients) runs on vsx_gemm_f16 with transposed /
 * flipped operands (videoswap_amd/autograd.py).  These are the element-wise / reduction passes: fp16 tensors,
 * fp32 arithmetic, fixed-order reductions (no atomics: deterministic).
 *   vsx_geglu_fwd     y2 [M, 2N] (h | g pre-activations, kept for the backward) -> out [M, N] = h * gelu_erf(g)
 *                     (diffusers GEGLU as its own pass; inference fuses it into the GEMM epilogue and drops y2)
 *   vsx_geglu_bwd     dout [M, N], y2 [M, 2N] -> dy2 [M, 2N]
 *   vsx_silu_bwd      dx = dy * silu'(x)   (adapter MLP, adapter_model.py:12-22)
 *   vsx_groupnorm_bwd data gradient of vsx_groupnorm_apply (same arguments; statistics recomputed; dy [.., C1+C2]
 *                     -> dx1 [.., C1], dx2 [.., C2]); ws: vsx_groupnorm_bwd_workspace(nimg, rows, groups) FLOATS
 *                     (chunk partial sums of a two-level reduction, ABI 6)   (resnet.py:166-177)
 *   vsx_layernorm_bwd data gradient of vsx_layernorm (the positional encoding is added after the normalisation)
 *   vsx_softmax_bwd   dS = scale * P o (dP - rowsum(dP o P)) in place over dP, rows padded to ld
 *   vsx_sum_pool2x2   [n, 2h, 2w, c] -> [n, h, w, c]: gradient of the nearest-2x upsampling folded into a conv
 *   vsx_adapter_gather gradient of vsx_adapter_scatter with respect to feat [P, C] (adapter_model.py:25-47)
 * ------------------------------------------------------------------------------------------ */
int vsx_geglu_fwd(const void* y2, void* out, int64_t M, int64_t N, vsx_stream_t stream);
int vsx_geglu_bwd(const void* dout, const void* y2, void* dy2, int64_t M, int64_t N, vsx_stream_t stream);
int vsx_silu_bwd(const void* dy, const void* x, void* dx, int64_t n, vsx_stream_t stream);
int64_t vsx_groupnorm_bwd_workspace(int64_t nimg, int64_t rows, int64_t groups);
int vsx_groupnorm_bwd(const void* dy, const void* x1, const void* x2, int64_t nimg, int64_t rows, int64_t C1,
                      int64_t C2, int64_t groups, const void* gamma, const void* beta, float eps, int64_t silu,
                      void* ws, void* dx1, void* dx2, vsx_stream_t stream);
int vsx_layernorm_bwd(const void* dy, const void* x, const void* gamma, float eps, void* dx, int64_t M, int64_t C,
                      vsx_stream_t stream);
int vsx_softmax_bwd(const void* P, void* dP, int64_t nrows, int64_t ncols, int64_t ld, float scale,
                    vsx_stream_t stream);
int vsx_sum_pool2x2(const void* x, void* y, int64_t n, int64_t h, int64_t w, int64_t c, vsx_stream_t stream);
int vsx_adapter_gather(const float* tracks, const int32_t* selected, const void* dmap, void* dfeat, int64_t F,
                       int64_t P, int64_t C, int64_t h, int64_t w, float rate, float out_scale, vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K12 (ABI 11): DIFT semantic-point embeddings (extract_semantic_point.py:125-205, dift_util.py:230-267).
 * `feat` is the UNet feature tap of AnimateDiffUNet3DModel.forward_features: fp16 [N, E, h, w, C] channels-last
 * (N frames, E ensemble members), C a multiple of 8.  The reference averages the E maps, upsamples the mean to the
 * image size (H, W) with nn.Upsample(mode='bilinear', align_corners=False) and reads / compares pixels of that fp32
 * map; these entry points compute the same numbers without building it (csrc/dift.hip).
 *   vsx_dift_sample_points: coords int32 [N, P, 2] = (x, y) pixels of the output image, x < 0 = skip the point.
 *       vec fp32 [N, P, C] = the upsampled ensemble mean at (y, x) (zeros for a skipped point); optional
 *       cos fp32 [N, P] = <vec, q> / max(|vec| |q|, 1e-8) against query fp32 [P, C] (query_per_frame 0) or
 *       [N, P, C] (query_per_frame 1); 0 for a skipped point.  query may be NULL when cos is NULL.
 *   vsx_dift_cosine_map: Q query vectors fp32 [Q, C] (or [N, Q, C]); optional cos_map fp32 [N, Q, H, W] = the
 *       cosine of every pixel of the upsampled mean map with each query (NULL: not written); argmax_yx int32
 *       [N, Q, 2] = (y, x) of the largest cosine, the first in row-major order among equal values
 *       (np.unravel_index(argmax)); argmax_val fp32 [N, Q] its value.  workspace: caller-allocated,
 *       vsx_dift_cosine_map_workspace(N, h, w, C, Q) bytes.
 * ------------------------------------------------------------------------------------------ */
int vsx_dift_sample_points(const void* feat, int64_t N, int64_t E, int64_t h, int64_t w, int64_t C, int64_t H,
                           int64_t W, const int32_t* coords, int64_t P, const float* query, int64_t query_per_frame,
                           float* vec, float* cos_out, vsx_stream_t stream);
int64_t vsx_dift_cosine_map_workspace(int64_t N, int64_t h, int64_t w, int64_t C, int64_t Q);
int vsx_dift_cosine_map(const void* feat, int64_t N, int64_t E, int64_t h, int64_t w, int64_t C, int64_t H, int64_t W,
                        const float* query, int64_t Q, int64_t query_per_frame, void* workspace,
                        int64_t workspace_bytes, float* cos_map, int32_t* argmax_yx, float* argmax_val,
                        vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K13 (ABI 12): fused coordinate MLP of the layered neural atlas = IMLP_Hash.forward with mlp_type 'origin'
 * (videoswap/atlas/implicit_neural_networks.py:164-195; the three networks propagate_point_displacement.py evaluates).
 * ALL tensors are fp32 and the arithmetic is fp32 throughout (fp32-input MFMA: one rounding per product, fp32 sums).
 *   x [N, input_dim] (input_dim 2 or 3) -> out [N, output_dim] (output_dim 1 to 3), both dense row-major, any N >= 0.
 *   pe_type 0 = 'none' (the coordinates feed layer 0), 1 = 'encoding' (positionalEncoding_vec with pe_dim frequencies
 *   2^j pi: per frequency the sines of all inputs, then the cosines; 2 * input_dim * pe_dim <= 64 columns),
 *   2 = 'hash_encoding' -> VSX_E_UNSUPPORTED.  mlp_type 0 = 'origin', 1 = 'tcnn' -> VSX_E_UNSUPPORTED.
 *   mlp_layers 2 to 8 (the output layer included), hidden_dim a multiple of 32 up to 256, ReLU before every layer but
 *   the first, bias on every layer, tanh on the output when use_tanh != 0.  skip_mask: bit i set = layer i reads
 *   cat(hidden activations, encoded input) (skip_layers; i in 1 .. mlp_layers - 1).
 *   packed: every layer's weight and bias in the layout the kernel streams, 16-byte aligned, packed_floats in all.
 *   Layer l has K = (l > 0 ? hidden_dim : 0) + (l == 0 or skip ? E8 : 0) input columns, E8 = the encoded width rounded
 *   up to a multiple of 8, and F = hidden_dim output features (the last layer: 32); the nn.Linear weight [out, in] is
 *   zero-padded to [F, K] (the encoded columns sit after the hidden ones, as torch.cat((x, input), 1) puts them).
 *   Layers follow each other; a layer is F * K floats of weight, then F floats of bias.  The weight is stored as
 *   [F / 32][K / 8][2][32][4]: element [t][b][h][i][s] = W[32 t + i][8 b + 4 h + s] (the float4 that lane 32 h + i of
 *   a wave feeds to four consecutive v_mfma_f32_32x32x2_f32).
 * ------------------------------------------------------------------------------------------ */
int vsx_coord_mlp_f32(const float* x, int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim,
                      int64_t mlp_layers, int64_t pe_type, int64_t pe_dim, int64_t mlp_type, int64_t skip_mask,
                      int64_t use_tanh, const float* packed, int64_t packed_floats, float* out, vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K14 (ABI 13): multiresolution hash grid in front of the K13 layer stack = IMLP_Hash.forward with pe_type
 * 'hash_encoding', mlp_type 'origin' (the texture network F_Atlas; implicit_neural_networks.py:117-130, 166-195), and the
 * grid alone.  The grid is tiny-cuda-nn's HashGrid with Linear interpolation, RESTATED from the published algorithm:
 * it has not been compared with tinycudann, and this block is the one place that defines it.
 *   Configuration: n_levels (1 to 32, n_levels * n_features <= 64), n_features = n_features_per_level (2 only),
 *   log2_hashmap_size (<= 24), base_resolution, per_level_scale; input_dim 2 only; fp32 table.  Anything else:
 *   VSX_E_UNSUPPORTED, the message names the option.
 *   Level l:  scale = exp2f(l * log2f(per_level_scale)) * base_resolution - 1 (fp32);  res = (uint32)ceilf(scale) + 1;
 *   entries = min(round_up(res^2, 8), 2^log2_hashmap_size);  offset = sum of the entries of the levels before it.
 *   table: [sum of entries][n_features] fp32, level-major, 16-byte aligned, table_floats in all (checked).
 *   Lookup of x = (x_0, x_1), every x_d within [-2, 2], all integer arithmetic uint32 with wrap-around:
 *   pos_d = fmaf(scale, x_d, 0.5f);  g_d = (uint32)(int)floorf(pos_d);  w_d = pos_d - floorf(pos_d);  corner c = 0 .. 3 has
 *   the coordinates g_d + ((c >> d) & 1) and the weight prod_d (bit ? w_d : 1 - w_d); its entry is
 *   idx = g_0, stride = res;  if stride <= entries: idx += g_1 * stride, stride *= res;  if entries < stride:
 *   idx = g_0 ^ (g_1 * 2654435761);  idx %= entries.  A feature is the sum over the corners, in corner order, of
 *   fmaf(weight, table[offset + idx][f], sum); it is output column l * n_features + f.
 *   Inputs outside [-2, 2], infinities and NaN are not refused: the conversion of pos_d to an integer is then
 *   unspecified, and so are the values that come out.  Every idx is still reduced modulo entries, so no input reads
 *   outside the table.
 *   vsx_hash_mlp_f32 sums a layer that runs one 32 x 32 tile per wave (the output layer; every layer when hidden_dim
 *   <= 64) in four interleaved partial sums over k, added pairwise; K13 sums every layer in one chain.
 * vsx_hash_grid_geometry: the level table on the host (any of the five arrays may be NULL; n_levels elements each;
 *   hashed: 1 where the level takes the hash) -> the table's float count, or a negative VSX_E_*.
 * vsx_hash_grid_f32: x [N, 2] -> out [N, n_levels * n_features] (8-byte aligned).  Rows past N are not gathered.
 * vsx_hash_mlp_f32: x [N, 2] -> out [N, output_dim], one launch; output_dim, hidden_dim, mlp_layers, skip_mask, use_tanh,
 *   packed, packed_floats exactly as K13 with n_levels * n_features encoded columns.
 * ------------------------------------------------------------------------------------------ */
int64_t vsx_hash_grid_geometry(int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size, int64_t base_resolution,
                               double per_level_scale, float* scale, uint32_t* res, uint32_t* entries, uint32_t* offset,
                               uint32_t* hashed);
int vsx_hash_grid_f32(const float* x, int64_t N, int64_t input_dim, const float* table, int64_t table_floats,
                      int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size, int64_t base_resolution,
                      double per_level_scale, float* out, vsx_stream_t stream);
int vsx_hash_mlp_f32(const float* x, int64_t N, int64_t input_dim, const float* table, int64_t table_floats,
                     int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size, int64_t base_resolution,
                     double per_level_scale, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers, int64_t skip_mask,
                     int64_t use_tanh, const float* packed, int64_t packed_floats, float* out, vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K15 (ABI 14): a video edited through its atlas = the texture-reading half of evaluate_model (videoswap/atlas/evaluate.py:
 * get_colors :64-85 with bilinear_interpolate_numpy :24-45, the "was this texel ever used" masks :373-397 and the
 * composition :399-404), one launch for N rows (csrc/atlas_edit.hip).  A row is a video pixel that has been
 * through FG_UV_Mapping, BG_UV_Mapping and F_Alpha.  ALL tensors are fp32 and dense; every product and sum below is ONE fp32
 * operation (no FMA contraction), in the order written.
 *   uv_fg, uv_bg [N, 2] (8-byte aligned): the raw network outputs.  alpha [N]: already mapped to 0.001 .. 0.991; it must be
 *   positive.  Per layer a texture tex [R, R, C] (16-byte aligned; C = 3: the colour, C = 4: an RGBA overlay; R >= 2,
 *   R * R * C < 2^31; h != w is refused), its box (minx, miny, pixel_size = R / the box's x extent, formed by the caller
 *   in fp32), with C = 4 the colours base [N, 3] the overlay is laid over, and optionally a mask image [R, R] (h, w given
 *   and checked against R) that the caller has initialised.  The two layers may differ in R and C.
 *   Per layer, shift = +0.5 (foreground) / -0.5 (background):
 *     q = uv * 0.5 + shift;  px = (q.x - minx) * pixel_size;  py = (q.y - miny) * pixel_size   (the x extent's pixel_size for both)
 *     relevant = floor(px) >= 0 && floor(py) >= 0 && ceil(px) < R && ceil(py) < R   (false for NaN, +-inf and anything far outside)
 *     x0 = floor(px), x1 = x0 + 1, y0, y1 likewise, each CLIPPED to [0, R - 1];  weights from the clipped corners:
 *     wa = (x1 - px)(y1 - py), wb = (x1 - px)(py - y0), wc = (px - x0)(y1 - py), wd = (px - x0)(py - y0);
 *     colour = ((tex[y0, x0] wa + tex[y1, x0] wb) + tex[y0, x1] wc) + tex[y1, x1] wd   (px == R - 1 exactly: x0 == x1, a zero colour
 *     on a relevant row, as in the reference);  C = 4: colour.rgb = colour.rgb * colour.a + base * (1 - colour.a).
 *   Outputs, [N, 3] each (4-byte aligned):  fg = relevant_fg ? colour_fg * alpha : 0;  bg = relevant_bg ? colour_bg : 0;
 *   edit = fg + (relevant_bg ? colour_bg * (1 - alpha) : 0);  relevant [N] uint8: bit 0 foreground, bit 1 background.
 *   Rows past N are not stored.  A row that is not relevant to a layer reads nothing of that layer's texture or mask.
 *   Masks: a foreground-relevant row raises the cells (ceil py, ceil px), (floor py, floor px), (floor py, ceil px),
 *   (ceil py, floor px) of mask_fg to max(old, alpha); a background-relevant row sets those cells of mask_bg to 1.  Both are
 *   an unsigned integer atomic max on the float's bits: exact and independent of the order of the rows (no float atomic
 *   anywhere).  DEVIATION: the reference's fancy-indexed `masks1[idx] = np.maximum(masks1[idx], alpha)` keeps the LAST
 *   writer, not the maximum, when two rows of one 100k-pixel batch share a cell; this computes the true maximum.
 *   Every texture and mask index is formed from a clamped value; no input value can make the kernel read or write outside
 *   the buffers it was given.
 *   Refused (vsx_last_error names the layer): C not 3 or 4 (VSX_E_UNSUPPORTED); a non-square texture, R < 2, R * R * C >= 2^31,
 *   C = 4 without base, a mask of another size, a null or misaligned pointer (VSX_E_BADSHAPE).
 * ------------------------------------------------------------------------------------------ */
int vsx_atlas_edit_f32(const float* uv_fg, const float* uv_bg, const float* alpha, int64_t N,
                       const float* tex_fg, int64_t fg_h, int64_t fg_w, int64_t fg_c, float fg_minx, float fg_miny,
                       float fg_pixel_size, const float* base_fg, float* mask_fg, int64_t mask_fg_h, int64_t mask_fg_w,
                       const float* tex_bg, int64_t bg_h, int64_t bg_w, int64_t bg_c, float bg_minx, float bg_miny,
                       float bg_pixel_size, const float* base_bg, float* mask_bg, int64_t mask_bg_h, int64_t mask_bg_w,
                       float* edit, float* fg, float* bg, uint8_t* relevant, vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K16 (ABI 15, additive): weight and bias gradients of the K13 coordinate MLP, for fitting the mapping networks of an atlas
 * (pretrain_mapping, the inverse-mapping fit).  fp32 throughout on v_mfma_f32_32x32x2_f32; no gradient with respect to x;
 * no atomics: two calls on the same inputs give the same bits (csrc/atlas_bwd.hip).  The options, their
 * limits and the words of a refusal are K13's; E = the encoded width (input_dim, or 2 * input_dim * pe_dim), L = mlp_layers.
 * vsx_coord_mlp_train_workspace: the float counts of `saved`, of the backward's `scratch` and of `grad` for N rows (any of
 *   the three pointers may be NULL).  saved = N * ((L - 1) * hidden_dim + E + output_dim);
 *   scratch = ceil(N / R) * grad + 2 * N * hidden_dim + N * output_dim with R = vsx_coord_mlp_wgrad_rows() (512).
 * vsx_coord_mlp_fwd_train_f32: vsx_coord_mlp_f32 (the same kernel source, `out` bit-identical) that also fills `saved`
 *   (16-byte aligned), for the rows < N only:
 *     [L - 1][N][hidden_dim]  the activation of hidden layer l after its ReLU, l = 0 .. L - 2
 *     [N][E]                  the encoded input (the coordinates themselves with pe_type none), unpadded
 *     [N][output_dim]         out
 * vsx_coord_mlp_bwd_f32: grad_out [N, output_dim], `saved` as written above, `packed` as K13 -> grad, one flat buffer: per
 *   layer, in the order hidden.0 .. hidden.L-1, the weight gradient [out, in] row-major in the nn.Linear layout (UNPADDED;
 *   in = hidden columns, then the E encoded columns of layer 0 and of the skip layers), then the bias gradient [out].
 *     dZ_L = grad_out, times (1 - out^2) with use_tanh;  dW_l = dZ_l^T In_l,  db_l = the column sums of dZ_l, In_l =
 *     cat(H_{l-1}, enc);  dZ_{l-1} = (dZ_l W_l[:, :hidden_dim]) where the STORED H_{l-1} > 0, else 0.  The encoded columns of a
 *     skip layer receive weight gradients and pass none on (the reference concatenates a detached copy).
 *   Summation over rows: chunks of R rows; inside a chunk four interleaved partial sums of R / 4 rows each, added pairwise;
 *   the chunks' results are added in index order by a last launch.  2 L + 1 launches whatever N is.  Rows >= N are never read.
 *   N == 0: grad is set to zero, nothing is launched.  scratch is overwritten.
 *   Refused, nothing written: an unsupported option (VSX_E_UNSUPPORTED); saved, scratch or grad shorter than the workspace
 *   query says (VSX_E_WORKSPACE); a null pointer, a packed buffer of another size (VSX_E_BADSHAPE).
 * ------------------------------------------------------------------------------------------ */
int64_t vsx_coord_mlp_wgrad_rows(void);
int vsx_coord_mlp_train_workspace(int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers,
                                  int64_t pe_type, int64_t pe_dim, int64_t mlp_type, int64_t skip_mask, int64_t* saved_floats,
                                  int64_t* scratch_floats, int64_t* grad_floats);
int vsx_coord_mlp_fwd_train_f32(const float* x, int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim,
                                int64_t mlp_layers, int64_t pe_type, int64_t pe_dim, int64_t mlp_type, int64_t skip_mask,
                                int64_t use_tanh, const float* packed, int64_t packed_floats, float* out, float* saved,
                                int64_t saved_floats, vsx_stream_t stream);
int vsx_coord_mlp_bwd_f32(const float* grad_out, int64_t N, int64_t input_dim, int64_t output_dim, int64_t hidden_dim,
                          int64_t mlp_layers, int64_t pe_type, int64_t pe_dim, int64_t mlp_type, int64_t skip_mask,
                          int64_t use_tanh, const float* packed, int64_t packed_floats, const float* saved,
                          int64_t saved_floats, float* scratch, int64_t scratch_floats, float* grad, int64_t grad_floats,
                          vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K17 (ABI 15, additive): the gradients of the K14 hash-grid network (the texture network F_Atlas): grid table, layer weights
 * and biases, and the input x (csrc/atlas_bwd.hip, the training forward in csrc/atlas.hip).  fp32 throughout.
 * The grid's options, their limits and the words of a refusal are K14's, the layer stack's are K13's; E = n_levels *
 * n_features, L = mlp_layers.  The cell of a row on a level (pos_d, g_d, w_d, the four idx) is K14's, computed by the same
 * device code as the forward.
 * vsx_hash_mlp_train_workspace: the float counts of `saved`, `scratch` and `grad` for N rows (any pointer may be NULL).
 *   saved = N * ((L - 1) * hidden_dim + E + output_dim);  grad = K16's (the layers only, K16's layout and order);
 *   scratch = K16's (ceil(N / R) * grad + 2 * N * hidden_dim + N * output_dim) + N * E for dEnc.
 * vsx_hash_mlp_fwd_train_f32: vsx_hash_mlp_f32 (the same kernel source, `out` bit-identical) that also fills `saved` (16-byte
 *   aligned) in K16's layout, for the rows < N only: [L - 1][N][hidden_dim], [N][E] (the two features of every level, unpadded),
 *   [N][output_dim].
 * vsx_hash_mlp_bwd_f32: grad_out [N, output_dim], x [N, 2] and the table of the forward, `saved` as written above ->
 *   1. grad: the K16 chain unchanged (the same kernels, K16's summation orders) on the saved activations.  No atomics: two
 *      calls on the same inputs give the same bits.  The encoded columns of a skip layer receive weight gradients and pass
 *      nothing on to the grid (the reference concatenates a detached copy); only layer 0 does.
 *   2. dEnc [N, E] (in scratch) = dZ_0 W_0 over the E encoded columns of the packed layer 0, no mask: per element four
 *      interleaved partial sums over the features f (f mod 8 in {0,4}, {1,5}, {2,6}, {3,7}, each in increasing f), added
 *      pairwise (p_0 + p_1) + (p_2 + p_3).  A column >= E is neither read nor written.
 *   3. the grid backward from dEnc, as vsx_hash_grid_bwd_f32 below.
 *   grad_table [table_floats] (16-byte aligned) and grad_x [N, 2] may each be NULL: that gradient is not computed; with both
 *   NULL steps 2 and 3 are not launched.  scratch is overwritten.  2 L + 1 launches, + 2 with a grid gradient, + the
 *   clearing of grad_table, whatever N is.  N == 0: grad and grad_table are set to zero, nothing else is launched.
 * vsx_hash_grid_bwd_f32: the grid backward alone: x [N, 2], grad_enc [N, E] -> grad_table, grad_x (each nullable).  Per row
 *   and level l, with ga, gb = grad_enc[row][2 l], [2 l + 1]:
 *     grad_table[offset + idx_c][f] += weight_c * grad_enc[row][2 l + f]   for the corners c = 0 .. 3, weight_c as in K14.
 *       All table_floats of grad_table are first set to zero on the stream; the additions are fp32 atomic adds in global
 *       memory, in no defined order: grad_table is NOT bit-reproducible from run to run (tiny-cuda-nn's is not either).
 *       An entry that no corner of any row addresses stays exactly zero.
 *     grad_x[row][d], d = 0, 1:  s_df = the sum over the corners c = 0 .. 3, in that order, of fmaf(sign * other,
 *       table[offset + idx_c][f], sum), sign = +1 where bit d of c is set, else -1, other = the weight of c along the other
 *       axis (w or 1 - w);  t_d = fmaf(gb, s_d1, ga * s_d0);  a wave owns the levels 16 p + 4 w .. 16 p + 4 w + 3 (w = 0 .. 3,
 *       p = 0, 1) and adds them in increasing l: part_w = fmaf(scale_l, t_d, part_w);  the four parts cross the waves through
 *       LDS and grad_x[row][d] = ((part_0 + part_1) + part_2) + part_3.  No atomics: bit-reproducible.
 *   Rows past N neither read nor add.  Every idx is reduced modulo the level's entry count as in the forward: no input value
 *   can make the kernel read or write outside the table.  N == 0: grad_table is set to zero, nothing is launched.
 * Refused, nothing written: an unsupported option (VSX_E_UNSUPPORTED, K14's and K13's words); saved, scratch or grad shorter
 *   than the workspace query says (VSX_E_WORKSPACE); a null pointer, a table, grad_table or saved that is not 16-byte
 *   aligned, a table or a packed buffer of another length (VSX_E_BADSHAPE).
 * ------------------------------------------------------------------------------------------ */
int vsx_hash_mlp_train_workspace(int64_t N, int64_t input_dim, int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size,
                                 int64_t base_resolution, double per_level_scale, int64_t output_dim, int64_t hidden_dim,
                                 int64_t mlp_layers, int64_t skip_mask, int64_t* saved_floats, int64_t* scratch_floats,
                                 int64_t* grad_floats);
int vsx_hash_mlp_fwd_train_f32(const float* x, int64_t N, int64_t input_dim, const float* table, int64_t table_floats,
                               int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size, int64_t base_resolution,
                               double per_level_scale, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers,
                               int64_t skip_mask, int64_t use_tanh, const float* packed, int64_t packed_floats, float* out,
                               float* saved, int64_t saved_floats, vsx_stream_t stream);
int vsx_hash_mlp_bwd_f32(const float* grad_out, const float* x, int64_t N, int64_t input_dim, const float* table,
                         int64_t table_floats, int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size,
                         int64_t base_resolution, double per_level_scale, int64_t output_dim, int64_t hidden_dim,
                         int64_t mlp_layers, int64_t skip_mask, int64_t use_tanh, const float* packed, int64_t packed_floats,
                         const float* saved, int64_t saved_floats, float* scratch, int64_t scratch_floats, float* grad,
                         int64_t grad_floats, float* grad_table, float* grad_x, vsx_stream_t stream);
int vsx_hash_grid_bwd_f32(const float* x, int64_t N, int64_t input_dim, const float* grad_enc, const float* table,
                          int64_t table_floats, int64_t n_levels, int64_t n_features, int64_t log2_hashmap_size,
                          int64_t base_resolution, double per_level_scale, float* grad_table, float* grad_x,
                          vsx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K18 (ABI 17, additive): the data gather and the losses of a layered-neural-atlas training step (train_atlas.py:127-253,
 * videoswap/atlas/loss_utils.py; csrc/atlas_loss.hip).  fp32 throughout; every pointer 4-byte aligned (idx 8).
 *
 * vsx_atlas_batch_f32 (K18a, one launch and the clearing of `counts`): idx [N] int64, flat pixel indices in the (frame, row,
 *   column) order of get_tuples: f = idx / (H W), i = idx % (H W) / W, j = idx % W.  The arrays of load_input_data in the
 *   reference's layouts: video, video_dx, video_dy [H, W, 3, T]; mask [H, W, T]; flow, flow_rev [H, W, 2, T, 1]; flow_mask,
 *   flow_rev_mask [H, W, T, 1], relevant where non-zero.  d = derivative_amount, D = global_derivative_amount.
 *   rows [B][N][3], B = 9 with_global, else 7 (blocks 5 and 6 absent, the flow matches at 5 and 6):
 *     0 (x, y, t)   1 (x + 1, y, t)   2 (x, y + 1, t)   3 (x, y - d, t)   4 (x - d, y, t)   5 (x, y - D, t)   6 (x - D, y, t)
 *     7 (x + fx, y + fy, t + 1), the forward flow match      8 (x + rx, y + ry, t - 1), the backward flow match
 *   each coordinate as torch computes it on the CPU in the reference: (float)c / (float)(larger_dim / 2.0) - 1, larger_dim =
 *   max(H, W), the time (float)f / (float)(T / 2.0) - 1, the flow match ((float)j + fx) first; IEEE divisions, no reciprocal:
 *   every output is bit-equal to the torch statement.  Offsets may leave the image (x + 1 = W, x - D < 0, t + 1 = T): these
 *   are coordinates only, every table read uses the sampled pixel.  Blocks 7 and 8 hold all N rows, relevant or not.
 *   rgb, rgb_dx, rgb_dy [N, 3]; alpha_gt [N]; m_fwd, m_bwd [N] in {0, 1}; counts int32 [2] = the sums of m_fwd and of m_bwd
 *   (integer atomic adds: exact, order-independent).  N == 0: counts are cleared, nothing is launched.
 *   An idx outside 0 .. T H W - 1 reads nothing: its rows, colours and alpha_gt are NaN, its m_fwd and m_bwd 0 (the Python
 *   binding refuses such a batch on the host before it copies it).
 *   Refused, nothing written: flow_levels != 1 (VSX_E_UNSUPPORTED); a null or misaligned pointer, H, W, T, d or D < 1
 *   (VSX_E_BADSHAPE).
 *
 * vsx_atlas_losses_f32 (K18b, two launches whatever N is): uv_fg, uv_bg [B N, 2], the mapping networks' outputs on `rows`;
 *   alpha_raw [5 N], F_Alpha's tanh output on the blocks 0, 1, 2, 7, 8; rgb_atlas [6 N, 3], F_Atlas's tanh output on
 *   uv_fg * 0.5 + 0.5 of the blocks 0, 1, 2, then on uv_bg * 0.5 - 0.5 of the same; K18a's outputs; cfg below ->
 *   losses [14]: 0 gradient, 1 rgb, 2 alpha, 3 sparsity, 4 rigidity fg, 5 rigidity bg, 6 global rigidity fg, 7 global rigidity
 *     bg, 8 flow fg, 9 flow bg, 10 flow_alpha, 11 total, 12 alpha_mean_fg, 13 alpha_mean_bg.  The definitions are the
 *     reference's (train_atlas.py:152-162, 180-196; loss_utils.py:5-48, 52-112, 132-153 with use_alpha, 212-233); a term that
 *     is switched off (alpha without with_alpha_loss, global rigidity without with_global_rigidity) is 0 and not in the total.
 *   g_uv_fg, g_uv_bg, g_alpha_raw, g_rgb_atlas: the gradient of losses[11] with respect to the four inputs, in their shapes.
 *     alpha is NOT detached in the flow losses; rgb_output of block 0 enters the gradient loss; uv of block 0 enters both
 *     rigidity losses and both flow losses; uv of the blocks 1 and 2 reaches the losses through F_Atlas only (zero here).
 *   A flow mean is sum(m term) / sum(m) over all N rows with the 0/1 weights m; a row with m = 0 contributes nothing and gets
 *     a zero gradient whatever the networks gave for it (a select, not a product).  DEVIATION: with no relevant row the term
 *     is 0 with a zero gradient (NaN in the reference).  alpha_mean_fg / _bg are sum / count over alpha > 0.5 / < 0.5 (strict),
 *     NaN on an empty set as in the reference; log values, no gradient.  The gradient of a norm at the zero vector and of |x|
 *     at 0 is 0 (torch's conventions); so is the gradient of the sqrt of an all-zero JtJ (NaN in torch).
 *   Summation: launch 1 takes one row per thread and writes its entries of the four gradients (one writer per entry); the 18
 *     per-row sums (csrc/atlas_loss.hip AL_TERMS) are added over a wave by xor-shuffles (32, 16, .. 1), over the four waves of
 *     a 256-row workgroup in wave order, and stored per workgroup in scratch; launch 2 adds the workgroups in index order and
 *     divides.  No atomics: two calls give the same bits.  scratch: vsx_atlas_losses_workspace(N) floats, overwritten.
 *   N == 0: only launch 2 runs; the means over N are 0 / 0 = NaN as in torch, no gradient is written.
 *   The reference's `assert not isnan / isinf` on the Jacobians has no equivalent (it would need a host sync per step): a
 *   non-finite value shows in losses[11].
 *   Refused, nothing written: a null or misaligned pointer, larger_dim or a derivative amount < 1, uv_mapping_scale <= 0
 *   (VSX_E_BADSHAPE); a short scratch (VSX_E_WORKSPACE).
 * All fields are 8 bytes so the struct has no padding on any ABI.
 * ------------------------------------------------------------------------------------------ */
typedef struct vsx_atlas_loss_cfg {
    double gradient_loss_weight, rgb_loss_weight, alpha_loss_weight, sparsity_loss_weight, rigidity_loss_weight;
    double global_rigidity_fg_loss_weight, global_rigidity_bg_loss_weight, flow_loss_weight, alpha_flow_loss_weight;
    double uv_mapping_scale;
    int64_t larger_dim, derivative_amount, global_derivative_amount;
    int64_t with_alpha_loss, with_global_rigidity;
} vsx_atlas_loss_cfg;
int vsx_atlas_batch_f32(const int64_t* idx, int64_t N, int64_t H, int64_t W, int64_t T, int64_t flow_levels, const float* video,
                        const float* video_dx, const float* video_dy, const float* mask, const float* flow, const float* flow_rev,
                        const float* flow_mask, const float* flow_rev_mask, int64_t d, int64_t D, int64_t with_global,
                        float* rows, float* rgb, float* rgb_dx, float* rgb_dy, float* alpha_gt, float* m_fwd, float* m_bwd,
                        int32_t* counts, vsx_stream_t stream);
int64_t vsx_atlas_losses_workspace(int64_t N);
int vsx_atlas_losses_f32(const float* uv_fg, const float* uv_bg, const float* alpha_raw, const float* rgb_atlas, int64_t N,
                         const float* rgb, const float* rgb_dx, const float* rgb_dy, const float* alpha_gt, const float* m_fwd,
                         const float* m_bwd, const int32_t* counts, const vsx_atlas_loss_cfg* cfg, float* losses, float* g_uv_fg,
                         float* g_uv_bg, float* g_alpha_raw, float* g_rgb_atlas, float* scratch, int64_t scratch_floats,
                         vsx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSX_H_ */
