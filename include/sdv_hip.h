/*
 * sdv_hip.h - C ABI of libsdv_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * StableDiffusionWalkPipeline hot path.
 *
 * The reference (nateraw/stable-diffusion-videos) has no FFI layer: its hot path is five Python
 * calls into diffusers/ATen (SURVEY.md section 8b "inner boundary"):
 *     self.unet(x, t, encoder_hidden_states=ctx).sample      stable_diffusion_pipeline.py:418
 *     noise_pred_uncond + g * (text - uncond)                stable_diffusion_pipeline.py:422-423
 *     self.scheduler.step(eps, t, latents).prev_sample       stable_diffusion_pipeline.py:426
 *     self.vae.decode(latents).sample                        stable_diffusion_pipeline.py:433
 *     torch.lerp(...) / slerp(...)                           stable_diffusion_pipeline.py:467-468, utils.py:42-66
 * Each entry point below replaces the ATen/cuDNN/cuBLAS work one of those lines dispatches; the
 * line it replaces is cited on the declaration.  INTEGRATION.md shows the ctypes stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer (HBM) unless named host_*.
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it (no sync, no
 *     allocation) so the whole denoise step is hipGraph-capturable.
 *   - bf16 = raw uint16 storage; activations are NHWC ([N*H*W, C] row-major == token-major).
 *   - return value: 0 = ok, negative = argument error (message via sdv_last_error()).
 */
#ifndef SDV_HIP_H
#define SDV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t sdv_bf16;

#define SDV_OK 0
#define SDV_ERR_ARG (-1)
#define SDV_ERR_LAUNCH (-2)

const char* sdv_last_error(void);
int sdv_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM on the bf16 MFMA pipes (v_mfma_f32_32x32x16_bf16), fp32 accumulate.
 *     C[b][m][n] = epi( alpha * sum_k X[b][m][k] * W[b][n][k] )
 * `X` rows are activations (or any K-contiguous operand), `W` rows are weights.  K % 64 == 0.
 * Replaces: every nn.Linear / Conv2d(1x1) / Conv2d(3x3) / torch.matmul inside
 * UNet2DConditionModel.forward (stable_diffusion_pipeline.py:418) and AutoencoderKL.decode (:433).
 *
 * mode      0 dense rows; 1 conv3x3 stride 1 pad 1; 2 conv3x3 stride 2 pad 1;
 *           3 nearest-2x upsample followed by conv3x3 pad 1 (Upsample2D), gathered on the fly.
 *           4 the same op in phase form: output pixel (2y+py, 2x+px) only sees the 2 x 2 low-resolution pixels
 *             {y-1+py, y+py} x {x-1+px, x+px}, so the 3x3 filter collapses to four 2x2 filters (taps that hit the same
 *             source pixel are summed by the caller) - 4/9 of the multiplies.  W is [4 phases][N][2][2][Cin], ldw = 4*Cin,
 *             Hin = Hout = H, Win = Wout = W (LOW-resolution grid), M = nimg*H*W, C is the [nimg*2H*2W][ldc] output.
 *           For conv modes M = nimg*Hout*Wout, K = Cin and W is [N][3][3][Cin] (OHWI), ldw = 9*Cin.
 * X2/C1     optional second source: channels [0,C1) come from X, [C1,K) from X2 (skip-connection
 *           concat without materialising it).  C1 % 64 == 0.
 * epi       0: bf16 out = acc*alpha (+bias) (+R)      [ldc, residual R with ldr]
 *           1: GEGLU: W rows pre-interleaved per 32-row tile as [16 value | 16 gate]; out is [M][N/2]
 *           2: as 0, then SiLU
 *           3: as 0, then LeakyReLU(0.2)   (RRDBNet convs of the Real-ESRGAN upsampler, upsampling.py:25)
 *           4: as 0, then quick_gelu x*sigmoid(1.702x) (CLIP ViT-L/14 text MLP);  5: as 0, then exact-erf GELU (OpenCLIP-H)
 * bias      fp32; bias_mode 1 = per n, 2 = per m.  If step_ptr != NULL the bias row used is
 *           bias + (*step_ptr) * bias_step_stride (per-denoise-step time-embedding bias table).
 * zero_page unused since ABI v1 kernels zero-fill padding through the buffer-descriptor range check (may be NULL).
 * batch     blockIdx.z; element strides sX/sW/sC/sR (0 = shared).
 * C / R     alignment of the bf16 output and the residual.  The epilogue has three store paths and picks one per launch:
 *             staged       ldc % 8 == 0, N % 8 == 0 (GEGLU: N / 2), ldr % 8 == 0, sC % 8 == 0, sR % 8 == 0 and C, R and bias on
 *                          16-byte addresses: whole 16-byte row segments.  A launch that misses one of these is NOT an error, it
 *                          takes one of the two register-direct paths below;
 *             8-byte       ldc % 4 == 0 (and ldr % 4 == 0 when there is a residual), and every GEGLU launch: four columns of C
 *                          (and of R) move as ONE 8-byte access.  The kernel chooses this path from ldc / ldr alone, so this is a
 *                          REQUIREMENT: C and R must then lie on 8-byte addresses, and sC / sR of a batched launch must be
 *                          multiples of 4 elements.  sdv_gemm_bf16 refuses (SDV_ERR_ARG, nothing launched) a launch that breaks it;
 *             scalar       any other ldc / ldr: element by element, C and R need their natural 2-byte alignment only.
 *           The typed outputs (out_mode) need the natural alignment of their element; out_f32 moves as 16-byte pieces only where
 *           the kernel finds ldc % 4 == 0, sC % 4 == 0 and a 16-byte address, element by element otherwise.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdv_gemm_args {
    const sdv_bf16* X;
    const sdv_bf16* X2;
    const sdv_bf16* W;
    const float* bias;
    const sdv_bf16* R;
    sdv_bf16* C;
    const int32_t* step_ptr;
    const sdv_bf16* zero_page;
    int64_t sX, sW, sC, sR;
    int32_t M, N, K;
    int32_t ldx, ldx2, C1, ldw, ldc, ldr;
    int32_t mode, Hin, Win, Hout, Wout, circular;
    int32_t epi, bias_mode, bias_step_stride;
    int32_t batch;
    int32_t tile;    /* 0 auto (cost model); 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 256x128 (4 waves); 6 = 256x320, 7 = 256x256, 8 = 256x128,
                        9 = 128x320 (8 waves, persistent); 10 = 256x32, 11 = 256x64 (4 waves: the typed-output convolutions).  (12 - 14 of
                        ABI <= 9 - the LDS-ring tiles and the transposed 320x256 tile - were experiments; gone in ABI 10.) */
    float alpha;
    uint32_t div_hw_mul, div_hw_shr, div_w_mul, div_w_shr;   /* filled in by sdv_gemm_bf16 (mode 4 row mapping); callers leave 0 */
    int32_t alpha_cols;   /* > 0: alpha multiplies only output columns [0, alpha_cols) (the Q half of a fused [Q | K] projection:
                             q * softmax_scale * log2(e) is rounded to bf16 ONCE, here, not a second time inside the attention) */
    /* LayerNorm folded into the GEMMs around it (BasicTransformerBlock.norm1/2/3 -> to_q/k/v, ff.net.0): the PRODUCER of the
     * normalised tensor writes per-row partial (sum, sumsq) of its bf16 outputs to stats_out [batch][M][slots][2]
     * (slots = sdv_gemm_stats_slots(args)), sdv_rowstats_finalize turns them into (mean, rstd) per row, and the CONSUMER
     * runs on the UN-normalised tensor with gamma-scaled weights W' = gamma o W:
     *     LN(x) W^T + b = rstd * (x W'^T - mean * s) + (W beta + b),   s[n] = sum_k W'[n][k]   (pass W beta + b as `bias`)
     * ln_side 1: ln_stats [batch][M][2] belongs to the output rows, ln_s [N] to the columns.  (ABI <= 9 had a column-side form 2
     * for a transposed V^T projection; since ABI 10 V comes out of the fused QKV projection row-major - sdv_attention_bf16's
     * v_rowmajor - and that launch form, its tile and its epilogue are gone.) */
    const float* ln_stats;
    const float* ln_s;
    float* stats_out;
    int32_t ln_side;
    int32_t stats_p;      /* filled in by sdv_gemm_bf16 */
    /* fp8 != 0: X (X2) and W hold OCP e4m3 bytes instead of bf16 (ldx / ldw / C1 / K still count ELEMENTS; rows must be 16-byte
     * multiples).  v_mfma_f32_32x32x16_fp8_fp8, fp32 accumulate, bf16 output; pass the product of the two per-tensor
     * dequantisation scales as `alpha`.  BASELINE.json configs[4] ("SD-v1-4 fp8"): the reference has no fp8 line of its own
     * (its dtype is whatever torch_dtype says, stable_diffusion_pipeline.py:840-858); here the ResBlock convolutions take fp8
     * activations written by sdv_groupnorm_apply(Y8, q_scale) and fp8 weights.  Tiles 1 / 6 / 7 / 9.
     * fp8 == 2: the same operands on CDNA4's block-scaled form v_mfma_scale_f32_32x32x64_f8f6f4 with every block scale 1.0
     * (E8M0 127) - 64 K values per instruction at twice the bf16 / plain fp8 rate, two 64-wide K images per barrier interval;
     * tap-major K order only.  Same products as fp8 == 1: the results differ by the fp32 summation order at most. */
    int32_t fp8;
    /* out_mode != 0: the output leaves in another type than bf16 (C may then be NULL), 4-wave tiles only (auto: 256x32 for
     * N <= 32, 256x128 for wide outputs); the image forms 2 / 3 need N <= 32 and no batch:
     *   1  out_f32 [batch][M][ldc] fp32, batch stride sC (in floats), any N   (UNet conv_out 320 -> 4: the noise prediction stays
     *      fp32; the VAE mid-block attention's Q K^T: the scores reach sdv_softmax_rows_f32 unrounded - AttentionBlock of
     *      AutoencoderKL.decode, stable_diffusion_pipeline.py:433)
     *   2  image epilogue of the VAE's conv_out 128 -> 3 (stable_diffusion_pipeline.py:432-438 + numpy_to_pil :450):
     *      v = clamp(v / 2 + 0.5, 0, 1) -> out_f32 [M][ldc] (optional) and out_u8 [M][ldc] = round-half-even(255 v) (optional)
     *   3  as 2 with v = clamp(v, 0, 1)            (RRDBNet conv_last of the Real-ESRGAN upsampler, upsampling.py:25-28)
     * so that the Cout <= 4 convolutions run on the matrix cores (N padded to one 32-column MFMA tile). */
    int32_t out_mode;
    float* out_f32;
    uint8_t* out_u8;
    /* GroupNorm statistics out of the producing epilogue (ResnetBlock2D.norm1/2, Transformer2DModel.norm, conv_norm_out: the
     * reference's nn.GroupNorm reads the tensor once for the statistics and once to normalise it; here the first read is gone).
     * gn_out != NULL: fp32 [batch * M / 32][2][gn_ld] - for every block of 32 output rows and every output column the (sum, sumsq)
     * of the bf16 values the tile stores (one writer per entry: deterministic).  mode 4: block index = phase * (M / 32) + m / 32.
     * Needs epi 0, bf16 output, no fold / fp8 / out_mode, M % 32 == 0, 16-byte aligned operands (the row-major store sequence).
     * sdv_groupnorm_finalize turns the blocks of an image (and the channels of a group) into sdv_groupnorm_apply's partials. */
    float* gn_out;
    int32_t gn_ld;
    /* SPLIT-K for the small-batch regime (walk()'s default batch_size is 1, stable_diffusion_pipeline.py:571; its test uses 16): with
     * few samples the low-resolution convs / GEMMs have M = 128 ... 2048 rows against K up to 23 040 - a handful of tiles on 256 CUs.
     * split_k > 1 on entry (with out_mode 0 and out_f32 = a workspace of [split_k][M][N] floats): the launch MAY give every output tile
     * to up to split_k workgroups, each taking a contiguous range of K slabs and leaving its fp32 partial sums in the workspace; a
     * second pass adds them in split order (deterministic), applies alpha / bias / residual and rounds once.  Plain launches only
     * (epi 0, no alpha_cols / fold / statistics / fp8 / typed output / batch / phase form, C and R 8-byte aligned - anything else
     * runs unsplit), 4-wave tiles only (1 - 3), >= 1024 K values per split.
     * sdv_gemm_split_k(args) tells how many splits a launch would take (1 = none), so the caller can size the workspace. */
    int32_t split_k;
} sdv_gemm_args;

int sdv_gemm_bf16(const sdv_gemm_args* args, void* stream);
int sdv_gemm_stats_slots(const sdv_gemm_args* args);
int sdv_gemm_split_k(const sdv_gemm_args* args);

/* The 8-wave tiles (6-9) run as PERSISTENT workgroups - one per CU, each walking tiles b, b + grid, ... with the next tile's
 * first K slab prefetched behind the current tile's epilogue.  sdv_gemm_set_persistent(0) falls back to one workgroup per
 * tile (bit-identical results; for A/B timing in tools/).  Returns the previous setting. */
int sdv_gemm_set_persistent(int on);
/* > 0: at most n persistent workgroups per launch (default: one per CU).  It caps EVERY persistent kernel: the 8-wave tiles of
 * sdv_gemm_bf16 and the panel kernels of sdv_ffn_geglu_bf16 / sdv_linear320_bf16 / sdv_linear640_bf16 (one workgroup per 128-row
 * panel, at most one per CU).  Test / tools knob: with a small limit even a 32-tile problem - or a few hundred rows of a panel
 * kernel - WALKS tiles / panels, so the walk paths (next tile's first K slab behind the epilogue; the panel hand-over) can be put
 * under the oracle-based parity gates at sizes the CPU oracle finishes in seconds.  Results are bit-identical: the limit only
 * changes which workgroup computes a tile.  Returns the previous setting. */
int sdv_gemm_set_grid_limit(int n);
/* partial (sum, sumsq) [rows][slots][2] -> (mean, rstd) [rows][2] over C channels */
int sdv_rowstats_finalize(const float* partials, int64_t rows, int32_t slots, int32_t C, float eps, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused GEGLU feed-forward of a BasicTransformerBlock, ONE launch (csrc/sdv_ffn.hip):
 *     out[m][:] = X[m][:] + b2 + W2 . ( v * gelu(g) ),   [v | g] = LayerNorm(X[m]) W1^T + b1
 * Replaces norm3 -> ff.net.0 (GEGLU) -> ff.net.2 -> + residual of diffusers' BasicTransformerBlock inside unet(...)
 * (stable_diffusion_pipeline.py:418) - as two sdv_gemm_bf16 launches (epi 1 with ln_side 1, then a residual GEMM) the
 * [M][4C] GEGLU output went through HBM; here a workgroup keeps a 128-token panel on chip and streams the weights.
 *   X        [M][ldx] bf16, un-normalised (the residual stream);  ln_stats [M][2] fp32 (mean, rstd) of its rows
 *            (sdv_rowstats_finalize of the producer's stats_out)
 *   W1       [8C][C] bf16 = gamma o ff.net.0.proj.weight, rows GEGLU-interleaved in 32-row tiles [16 value | 16 gate]
 *            (the layout sdv_gemm_bf16's epi 1 takes)
 *   W1x      [8C][16] bf16, same row order: the LayerNorm fold's per-column terms as one more k-step of the matrix product.
 *            With s = row sums of W1 (fp32) and t = W beta + b (fp32), each split into three bf16 pieces (h + m + l):
 *            row = (s_h s_h s_m s_h s_l s_m t_h t_h | t_m t_h t_l t_m 0 0 0 0); the kernel multiplies it with the token's
 *            (m_h m_m m_h m_l m_h m_m r_h r_m | r_h r_l r_h r_m 0 0 0 0), m = -mean, r = 1 / rstd - the six leading cross terms
 *            of each product, 24 bits, accumulated in fp32:  LN(x) W^T + b = rstd (x W1^T - mean s + t / rstd)
 *   W2p      [C][4C] bf16 = ff.net.2.weight with its K axis permuted inside every block of 16: position 8 a + 4 b + e holds
 *            column 8 b + 4 a + e (a, b in {0, 1}, e in 0..3) - the order in which the MFMA accumulator layout hands the GEGLU
 *            outputs of a lane over as the next contraction's B operand;  bias2 [C]
 *   out      [M][ldo] bf16 (may alias nothing of the inputs)
 * C must be 320 (the 64 x 64 level of SD-1.x / the 96 x 96 level of SD-2.x at 768 x 768: wider levels keep the two-launch form -
 * their weights do not stay L2-resident per panel).  M is arbitrary (rows past M are not stored). */
int sdv_ffn_geglu_bf16(const sdv_bf16* X, const float* ln_stats, int64_t M, int32_t C, int32_t ldx, const sdv_bf16* W1, const sdv_bf16* W1x,
                       const sdv_bf16* W2p, const float* bias2, sdv_bf16* out, int32_t ldo, void* stream);

/* The (M, 320, 320) / (M, 960, 320) projections of the C = 320 transformer blocks on the same panel skeleton (csrc/sdv_ffn.hip):
 *     out[m][n] = bf16( alpha[n / 320] * rstd_m * ( X[m] . W[n] - mean_m * s_n + t_n / rstd_m ) )        R == NULL
 *     out[m][n] = bf16( X[m] . W[n] + t_n + R[m][n] )                                                    R != NULL (N = 320, no ln_stats / alpha)
 * Replaces proj_in, attn1.to_q/k/v (one fused N = 960 projection), attn1.to_out, attn2.to_q and attn2.to_out of Transformer2DModel /
 * BasicTransformerBlock inside unet(...) (stable_diffusion_pipeline.py:418) at the 64 x 64 level, which sdv_gemm_bf16's 256 x 320 tile
 * ran at 40 - 58 % of the achievable HBM rate.
 *   X        [M][ldx] bf16 (320 columns used);  W [N][320] bf16 (gamma-folded where a LayerNorm feeds the layer);  N = 320 or 960
 *   Wx       [N][16] bf16: the fold columns of (s, t) exactly as sdv_ffn_geglu_bf16's W1x - a plain bias is (s = 0, t = bias)
 *   ln_stats [M][2] fp32 (mean, rstd) of the rows of X, or NULL (mean 0, rstd 1: a plain biased projection)
 *   alpha    [N / 320] fp32 or NULL: one factor per block of 320 output columns (the Q third of the fused projection carries the
 *            softmax scale * log2 e: sdv_attention_bf16 q_prescaled)
 *   R        [M][ldr] bf16 residual or NULL;  out [M][ldo] bf16
 *   stats_out [M][2] fp32 or NULL (N = 320): (mean, rstd = rsqrt(var + eps)) of the STORED rows - what the next LayerNorm fold
 *            (ln_stats of a later call, sdv_gemm_args.ln_stats) consumes; no partial sums, no sdv_rowstats_finalize launch.
 *            One pass in fp32, var = max(E[y^2] - mean^2, 0): the variance carries an error of up to 1e-5 E[y^2], so for rows with
 *            a high |mean| / sigma the consumer's fold receives an rstd that is off by about half of 1e-5 E[y^2] / (var + eps)
 *            (measured, tests/test_panel_edges_gpu.py: below 1e-3 for |mean| > 10 sigma rows of the residual stream, 75 % for a
 *            constant row of 100s, whose true variance is 0)
 *   Vt       NULL, or (N = 960) [M / hw][320][ldvt] bf16: the LAST block of 320 columns - V of the fused Q K V projection - is stored
 *            TRANSPOSED per sample of hw tokens (hw % 128 == 0, M % hw == 0, ldvt >= hw), as sdv_attention_bf16 takes it with
 *            v_rowmajor = 0, and `out` ([M][ldo], ldo >= 640) receives only [Q | K] */
int sdv_linear320_bf16(const sdv_bf16* X, int64_t M, int32_t ldx, const sdv_bf16* W, const sdv_bf16* Wx, int32_t N, const float* ln_stats,
                       const float* alpha, const sdv_bf16* R, int32_t ldr, sdv_bf16* out, int32_t ldo, float* stats_out, float eps,
                       sdv_bf16* Vt, int32_t ldvt, int32_t hw, void* stream);

/* The same kernel for C = 640 rows (the 32 x 32 level): N = 640 (proj_in with stats_out, attn2.to_q) or 1920 (the fused Q K V projection,
 * row-major), formula and operands as sdv_linear320_bf16 with W [N][640] and alpha [N / 320].  No residual form and no transposed V: the
 * 40 input fragments of a wave's 32 rows already take 160 of its registers (attn.to_out / proj_out stay on sdv_gemm_bf16).
 * stats_out is available for N = 640. */
int sdv_linear640_bf16(const sdv_bf16* X, int64_t M, int32_t ldx, const sdv_bf16* W, const sdv_bf16* Wx, int32_t N, const float* ln_stats,
                       const float* alpha, sdv_bf16* out, int32_t ldo, float* stats_out, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Flash-style attention, softmax(Q K^T * scale) V, never materialising the score matrix.
 * Replaces CrossAttention.forward inside the UNet (self: Lk = Lq; cross: Lk = 77).
 *   Q  [B][Lq][ldq]   head h at columns [h*dh, (h+1)*dh)
 *   K  [B][Lk][ldk]   same head layout
 *   Vt v_rowmajor == 0: [B][H*dh][ldv] V TRANSPOSED (row = channel, column = key), ldv >= roundup(Lk,64), the columns >= Lk
 *                       must be finite (zero-filled) - the text context's V^T, projected once per walk;
 *      v_rowmajor != 0: [B][Lk][ldv] V as the projection wrote it (same head layout as K, ldv = its row stride: the V columns of
 *                       a fused [Q | K | V] projection - attn1.to_q / to_k / to_v of BasicTransformerBlock in ONE GEMM); the kernel
 *                       transposes in the LDS read (ds_read_b64_tr_b16), so the UNet's self-attention has no V^T launch
 *   O  [B][Lq][ldo]
 * dh in {40, 64, 80, 160}.  causal != 0 masks key > query (CLIPTextModel's causal mask, reached from
 * text_encoder(ids)[0], stable_diffusion_pipeline.py:819; needs Lq == Lk).
 * q_prescaled != 0: Q already holds q * scale * log2(e) (its projection GEMM applied it before its single bf16 rounding,
 * sdv_gemm_args.alpha / alpha_cols) and `scale` is ignored.  With q_prescaled == 0 the 40 / 80-wide-head kernels pre-multiply Q
 * themselves and round it to bf16 a second time: measured 4.6e-3 instead of 1.9e-3 rel-L2 once the logits are as peaked as a
 * trained model's (tests/test_kernels_gpu.py::test_attention_elementwise_bound).
 * ------------------------------------------------------------------------------------------ */
int sdv_attention_bf16(const sdv_bf16* Q, const sdv_bf16* K, const sdv_bf16* Vt, sdv_bf16* O,
                       int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh,
                       int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo, float scale, int32_t causal,
                       int32_t q_prescaled, int32_t v_rowmajor, void* stream);

/* row softmax in place over bf16 rows (1 head x 512 channels; kept for callers that hold bf16 scores) */
int sdv_softmax_rows_bf16(sdv_bf16* S, int64_t rows, int32_t cols, int32_t ld, void* stream);
/* row softmax of fp32 scores S [rows][lds] into bf16 probabilities P [rows][ldp] (P != S): torch.softmax(scores.float(), -1) of the
 * VAE mid-block attention (vae.decode, stable_diffusion_pipeline.py:433) - with sdv_gemm_args.out_mode 1 the scores are never
 * rounded to bf16, the probabilities are rounded once (as inside the flash kernel).  cols % 8 == 0, ldp % 8 == 0, lds % 4 == 0. */
int sdv_softmax_rows_f32(const float* S, sdv_bf16* P, int64_t rows, int32_t cols, int32_t lds, int32_t ldp, void* stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm (32 groups in SD) over NHWC activations, optionally over the channel-concat of two
 * tensors, fused with SiLU.  Replaces nn.GroupNorm + F.silu in ResnetBlock2D / Transformer2DModel.
 *   stats: partial (sum, sumsq) per (image, split, group) -> `partials` [nimg][splits][groups][2]
 *   apply: finalises mean/rstd from the partials and writes bf16 y = act((x-mean)*rstd*g + b)
 * ------------------------------------------------------------------------------------------ */
/* GroupNorm statistics from the producer's epilogue: P1 (and P2 for a channel concat [x, skip]) are sdv_gemm_args.gn_out arrays
 * [blocks][2][ld] of (sum, sumsq) per 32-row block and channel; image i owns blocks [i * bpi, (i + 1) * bpi) of each of `nrep`
 * repetitions `rep_stride` blocks apart (mode 4 producers: 4 phases).  Writes partials [nimg][splits][groups][2] (an image's
 * blocks cut into `splits` <= 64 ranges, one workgroup each) for sdv_groupnorm_apply with the same `splits` - the statistics
 * pass over the tensor (sdv_groupnorm_stats) is not needed then. */
int sdv_groupnorm_finalize(const float* P1, int32_t C1, int32_t ld1, int32_t bpi1, int32_t nrep1, int64_t rep_stride1,
                           const float* P2, int32_t C2, int32_t ld2, int32_t bpi2, int32_t nrep2, int64_t rep_stride2,
                           int32_t nimg, int32_t groups, int32_t splits, float* partials, void* stream);
int sdv_groupnorm_stats(const sdv_bf16* X, const sdv_bf16* X2, int32_t C1, int32_t C2, int32_t nimg,
                        int32_t HW, int32_t groups, int32_t splits, float* partials, void* stream);
/* Like sdv_groupnorm_stats, apply (bf16 and fp8) refuses splits <= 0, nimg <= 0 and HW <= 0 before any launch. */
int sdv_groupnorm_apply(const sdv_bf16* X, const sdv_bf16* X2, int32_t C1, int32_t C2, int32_t nimg,
                        int32_t HW, int32_t groups, int32_t splits, const float* partials,
                        const float* gamma, const float* beta, float eps, int32_t silu, sdv_bf16* Y,
                        void* stream);
/* as sdv_groupnorm_apply, writing OCP e4m3 bytes Y8 = sat(y * q_scale) (the fp8 conv's activation operand) */
int sdv_groupnorm_apply_fp8(const sdv_bf16* X, const sdv_bf16* X2, int32_t C1, int32_t C2, int32_t nimg,
                            int32_t HW, int32_t groups, int32_t splits, const float* partials,
                            const float* gamma, const float* beta, float eps, int32_t silu, uint8_t* Y8,
                            float q_scale, void* stream);
/* Debug aid for the fp8 path (BASELINE.json configs[4]): while `counter` (one device int32, or NULL = off, the default) is set,
 * every sdv_groupnorm_apply_fp8 launch adds the number of elements whose scaled value fell outside +-448 - i.e. that the e4m3
 * conversion clamped - to it.  A pilot calibration that is too tight for the prompts actually run then reads non-zero instead of
 * clipping silently.  Set it before a step is captured into a hipGraph (the pointer is a kernel argument). */
int sdv_groupnorm_fp8_set_saturation_counter(int32_t* counter);

/* LayerNorm over the last dim of [rows][C] bf16 (BasicTransformerBlock.norm1/2/3) */
int sdv_layernorm_bf16(const sdv_bf16* X, const float* gamma, const float* beta, float eps, int64_t rows,
                       int32_t C, sdv_bf16* Y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small-channel direct convolutions (no MFMA: K or N too small for a tile).
 *   conv3x3_cin_small : Cin <= 8  (UNet conv_in 4->320, VAE decoder.conv_in 4->512), bf16 NHWC out
 *   (the Cout <= 4 output convolutions - UNet conv_out 320->4, VAE conv_out 128->3, RRDBNet conv_last - run on the matrix cores:
 *    sdv_gemm_args.out_mode; the one-wave-per-pixel sdv_conv3x3_cout_small of ABI <= 9 is gone)
 * ------------------------------------------------------------------------------------------ */
int sdv_conv3x3_cin_small(const sdv_bf16* X, const sdv_bf16* W /*[Cout][3][3][Cin]*/, const float* bias,
                          sdv_bf16* Y, int32_t nimg, int32_t H, int32_t Wd, int32_t Cin, int32_t Cout,
                          int32_t circular, void* stream);
/* im2col of a 4-channel NHWC image for a 3x3 pad-1 conv: Y[pixel][64] = [9 taps x 4 channels | 28 zeros]; the conv is
 * then sdv_gemm_bf16 with K = 64 against weights zero-padded the same way (UNet conv_in, VAE decoder.conv_in). */
int sdv_im2col3x3_c4(const sdv_bf16* X, sdv_bf16* Y, int32_t nimg, int32_t H, int32_t Wd, int32_t circular, void* stream);

/* z = Wpq * (x * in_scale) + b per pixel, fp32 NHWC latents -> bf16 NHWC (1/0.18215 scaling of
 * stable_diffusion_pipeline.py:432 fused with AutoencoderKL.post_quant_conv) */
int sdv_latent_affine(const float* X, const float* Wpq /*[C][C]*/, const float* bias, float in_scale,
                      sdv_bf16* Y, int64_t npix, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Interpolation between walk endpoints (stable_diffusion_pipeline.py:466-468).
 *   slerp_stats: dot(v0,v1), |v0|^2, |v1|^2 over the WHOLE tensor (utils.py:51) -> stats[3] (fp64)
 *   slerp_batch: out[f] = slerp(T[f], v0, v1) for all frames f in one launch (utils.py:52-61);
 *                input is CHW fp32; output is written HWC (NHWC latents) when to_hwc != 0.
 *   lerp_batch : out[f] = torch.lerp(a, b, T[f]) (:467); fp32 in, bf16 and/or fp32 out.
 * T is a device array of fp32.
 * ------------------------------------------------------------------------------------------ */
int sdv_slerp_stats(const float* v0, const float* v1, int64_t n, double* stats, void* stream);
int sdv_slerp_batch(const float* v0, const float* v1, const double* stats, const float* T, int32_t nframes,
                    int32_t C, int32_t HW, int32_t to_hwc, float dot_threshold, float* out, void* stream);
int sdv_lerp_batch(const float* a, const float* b, const float* T, int32_t nframes, int64_t n,
                   float* out_f32, sdv_bf16* out_bf16, void* stream);

/* ------------------------------------------------------------------------------------------
 * One fused classifier-free-guidance + DDIM update (stable_diffusion_pipeline.py:414, 422-426):
 *     eps = eps_u + g (eps_c - eps_u);  x <- c_x * x + c_e * eps (+ sigma * noise)
 * coefs is a device table [nsteps][4] = {c_x, c_e, sigma, unused}; the row is *step_ptr.  For
 * v-prediction the host folds the conversion into a 2x2 per-step matrix (vpred != 0 -> coefs rows
 * are {c_xx, c_xv, sigma, 0}); same arithmetic.  Also writes the NEXT UNet input: bf16 copies of
 * the new latents for both CFG halves (x2[0:B] = x2[B:2B] = x) - the torch.cat([latents]*2) of :414.
 * eps layout [2B][HW][C] fp32 (uncond first) when cfg != 0, else [B][HW][C].
 * ------------------------------------------------------------------------------------------ */
int sdv_cfg_ddim_step(const float* eps, float* latents, sdv_bf16* x2, const float* coefs,
                      const int32_t* step_ptr, const float* noise, float guidance, int32_t cfg,
                      int64_t n_per_batch /* B*HW*C */, void* stream);
/* ------------------------------------------------------------------------------------------
 * The same for every OTHER scheduler the reference's constructor accepts (stable_diffusion_pipeline.py:71-78 - PNDM/PLMS
 * (the SD-v1 default), LMSDiscrete (examples/make_music_video.py:15), EulerDiscrete, EulerAncestral, DPM-Solver++ 2M):
 * `scheduler.scale_model_input` (:415), guidance (:422-423) and `scheduler.step(...).prev_sample` (:426) of ONE UNet
 * evaluation.  All of them are linear in (sample, model outputs), so the host precomputes one row per evaluation:
 *     table[step][16] = { a, c, w0, w1, w2, w3, u, v, s_in, s_noise, flags, head, 0, 0, 0, 0 }
 *     g = eps_u + guidance (eps_c - eps_u);   m = u x + v g;   comb = w0 m + w1 H[head-1] + w2 H[head-2] + w3 H[head-3]
 *     x' = a (flags & 4 ? xsave : x) + c comb (+ s_noise noise[step]);   flags & 2: xsave = x;   flags & 1: H[head] = m
 *     x2 = bf16(s_in x') for both CFG halves (the NEXT evaluation's scaled model input)
 * hist: fp32 [4][n] ring (indices mod 4), xsave: fp32 [n]; eps / latents / x2 / noise as for sdv_cfg_ddim_step.
 * ------------------------------------------------------------------------------------------ */
int sdv_cfg_multistep_step(const float* eps, float* latents, sdv_bf16* x2, float* hist, float* xsave, const float* table,
                           const int32_t* step_ptr, const float* noise, float guidance, int32_t cfg,
                           int64_t n_per_batch /* B*HW*C */, void* stream);
/* latents fp32 -> bf16 UNet input (both CFG halves); used once before step 0 */
int sdv_latents_to_unet_input(const float* latents, sdv_bf16* x2, int32_t cfg, int64_t n, void* stream);
int sdv_step_counter_add(int32_t* step_ptr, int32_t inc, void* stream);

/* sinusoidal timestep embedding (diffusers get_timestep_embedding, flip_sin_to_cos) -> fp32 [n][dim] */
int sdv_timestep_embedding(const float* timesteps, int32_t n, int32_t dim, int32_t flip_sin_to_cos,
                           float freq_shift, float* out, void* stream);
/* small fp32 linear: out[m][n] = sum_k act(x[m][k]) * w[n][k] + b[n] (+ add[n]); used once per
 * walk for the time-embedding MLP and the 22 time_emb_proj tables (M = num_inference_steps). */
int sdv_linear_small(const float* x, const sdv_bf16* w, const float* b, const float* add, float* out,
                     int32_t M, int32_t N, int32_t K, int32_t silu_in, void* stream);

/* layout helpers at the API boundary */
int sdv_nchw_to_nhwc_f32(const float* in, float* out, int32_t n, int32_t C, int32_t HW, void* stream);
int sdv_nhwc_to_nchw_f32(const float* in, float* out, int32_t n, int32_t C, int32_t HW, void* stream);
int sdv_f32_to_bf16(const float* in, sdv_bf16* out, int64_t n, void* stream);

/* CLIP text encoder input (text_encoder(ids)[0], stable_diffusion_pipeline.py:819): out[t] = tok[ids[t]] + pos[t % L],
 * fp32 tables -> bf16 rows; ids outside [0, vocab) are an error caught on the host side of the binding. */
int sdv_embed_tokens(const int64_t* ids, const float* tok /*[vocab][D]*/, const float* pos /*[L][D]*/, sdv_bf16* out,
                     int64_t n_tokens, int32_t L, int32_t D, int32_t vocab, void* stream);

/* Real-ESRGAN x4 upsampler (upsampling.py:25-28, :46: RRDBNet inside RealESRGANer.enhance) - the glue around
 * sdv_gemm_bf16 / sdv_im2col3x3_c4 / sdv_conv3x3_cout_small:
 *   rgb_u8_to_bf16_c4: uint8 RGB NHWC pixels -> 4-channel bf16 rows {r,g,b,0}*scale (pre_process: img/255)
 *   axpby_bf16:        out = alpha*a + beta*b over strided bf16 rows (RRDB: out*0.2 + x), cols/strides % 8 == 0 */
int sdv_rgb_u8_to_bf16_c4(const uint8_t* in, sdv_bf16* out, int64_t npix, float scale, void* stream);
int sdv_axpby_bf16(const sdv_bf16* a, int32_t lda, const sdv_bf16* b, int32_t ldb, sdv_bf16* out, int32_t ldo,
                   int64_t rows, int32_t cols, float alpha, float beta, void* stream);

/* ------------------------------------------------------------------------------------------
 * Safety checker (stable_diffusion_pipeline.py:440-447).  The CLIP vision tower between these two entry points runs on
 * sdv_gemm_bf16 / sdv_layernorm_bf16 / sdv_attention_bf16 (vision.py); csrc/sdv_vision.hip holds what is not a transformer.
 *
 * sdv_clip_preprocess_patches - replaces `self.feature_extractor(self.numpy_to_pil(image), return_tensors="pt")` (:441,
 * transformers.CLIPImageProcessor) AND the im2col of the stride-P patch convolution, in one launch:
 *   frames   uint8 RGB NHWC [n][H][W][3], contiguous (what the VAE image epilogue leaves in HBM)
 *   patches  bf16 [n * (S/P)^2][Kpad], 16-byte aligned: row = patch (image-major, then raster), column = (c, py, px), i.e. the
 *            flattened conv weight [hidden][3][P][P] is the GEMM's W; K = 3*P*P zero-padded to Kpad = roundup(K, 64) - the pad
 *            columns are written (as zeros) by the kernel
 *   x_* / y_* the two 1-D tap tables of PIL's bicubic resize (separable, a = -0.5, support 2*max(scale, 1), centre (i + 0.5)*scale,
 *            weights normalised to sum 1) restricted to the centre-crop window: for each of the S output samples of an axis the
 *            first source index (`off` int32 [S]), the tap count (`cnt` int32 [S], <= taps) and the weights (`w` fp32 [S][taps])
 *   host_mean / host_std   HOST pointers to 3 floats: value = (pixel / 255 - mean[c]) / std[c]
 * Both passes are fp32 with the horizontally filtered rows staged in LDS (no uint8 rounding between them, no resized image in
 * HBM); only the crop window is computed.  P * S * 12 + S * 12 bytes must fit in 64 KiB of LDS.
 *
 * sdv_safety_screen - replaces `self.safety_checker(images=image, clip_input=...)` behind the vision tower (:442-447, diffusers
 * StableDiffusionSafetyChecker.forward) and `images[idx] = np.zeros(...)`:
 *   cos = cosine similarity of image_embeds [n][D] with special_care_embeds [n_special][D] / concept_embeds [n_concept][D] (fp32);
 *   special = cos_s - special_thr (+ 0);  adj = 0.01 if any special > 0 else 0;  concept = cos_c - concept_thr + adj;
 *   flags[i] = any(concept > 0);  scores [n][n_special + n_concept] = [special | concept].
 *   frames (may be NULL; else 16-byte aligned, n frames of frame_bytes bytes each): flagged frames are overwritten with zeros.
 * Two launches on `stream` (head, black-out). */
int sdv_clip_preprocess_patches(const uint8_t* frames, sdv_bf16* patches, int32_t n, int32_t H, int32_t W, int32_t S, int32_t P,
                                int32_t Kpad, const int32_t* x_off, const int32_t* x_cnt, const float* x_w, int32_t x_taps,
                                const int32_t* y_off, const int32_t* y_cnt, const float* y_w, int32_t y_taps,
                                const float* host_mean, const float* host_std, void* stream);
int sdv_safety_screen(const float* image_embeds, const float* concept_embeds, const float* special_care_embeds,
                      const float* concept_thr, const float* special_thr, int32_t n, int32_t D, int32_t n_concept,
                      int32_t n_special, uint8_t* frames, int64_t frame_bytes, int32_t* flags, float* scores, void* stream);

/* ------------------------------------------------------------------------------------------
 * JPEG encoder (csrc/sdv_jpeg.hip).  Replaces the host-side JPEG compression of frames the GPU already holds: `image.save(frame_filepath)`
 * in make_clip_frames for a `.jpg` image_file_ext (stable_diffusion_pipeline.py:553) and the frame encode inside make_video_pyav
 * (utils.py:69-128) where the track is Motion-JPEG.  Only compressed bytes leave HBM.
 *
 * Stream: baseline sequential JFIF, 8 bit, 3 components, 4:2:0; MCU = 16 x 16 pixels = blocks Y00 Y01 Y10 Y11 Cb Cr; the frame is padded
 * to multiples of 16 by replicating its last row / column; the Annex K "typical" Huffman tables; restart interval = one MCU row
 * (ceil(W / 16) MCUs), RST0..RST7 cycling between the intervals, each interval padded to a byte with 1-bits, 0xFF stuffed with 0x00.
 *
 * sdv_jpeg_transform_u8   frames uint8 RGB NHWC [n][H][W][3] contiguous -> coef int16 [n][ceil(H/16)][ceil(W/16)][6][64] (16-byte
 *   aligned), each block in zigzag order: JFIF full-range YCbCr, chroma = mean of each 2 x 2, - 128, orthonormal 8 x 8 DCT-II, divided
 *   by the table entry, rounded to nearest with ties away from zero; fp32, nothing rounded in between.
 *   qtab_luma / qtab_chroma: HOST pointers to 64 entries in natural (row-major) order, each 1 .. 255.
 *
 * sdv_jpeg_entropy_pack   coef -> out: n complete files back to back, out[offsets[k] .. offsets[k + 1]) is file k; offsets int64 [n + 1]
 *   and needed int64 [1] (= offsets[n]) in GPU memory.  header: the header_len bytes SOI .. SOS that open every file (GPU memory,
 *   constant for one (H, W, quality)).  scratch: at least 12 bytes per restart interval (n * ceil(H/16)), 8-byte aligned.
 *   When *needed > out_cap NOTHING is written to out (offsets and needed still are): the caller retries with a buffer of *needed bytes.
 *   Three launches on `stream`: count (one wave per restart interval), scan, write (the same code, storing at the final positions).
 * 1 <= H, W <= 65535, 1 <= n <= 65535. */
int sdv_jpeg_transform_u8(const uint8_t* frames, int32_t n, int32_t H, int32_t W, const uint16_t* qtab_luma,
                          const uint16_t* qtab_chroma, int16_t* coef, void* stream);
int sdv_jpeg_entropy_pack(const int16_t* coef, int32_t n, int32_t H, int32_t W, const uint8_t* header, int32_t header_len,
                          void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* offsets, int64_t* needed,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * PNG encoder (csrc/sdv_png.hip).  Replaces the host-side PNG compression of frames the GPU already holds: `image.save(frame_filepath)`
 * in make_clip_frames for the default `.png` image_file_ext (stable_diffusion_pipeline.py:553).  Lossless; only compressed bytes
 * leave HBM.
 *
 * Stream: signature | IHDR (8 bit RGB, no interlace) | ONE IDAT | IEND.  Every row = filter-type byte + 3W bytes; the type is chosen
 * per row among all five by libpng's heuristic (minimum sum of v < 128 ? v : 256 - v over the filtered bytes, ties to the lowest
 * type; row 0 sees a row of zeros above).  zlib: `78 01`; the filtered rows are cut into stripes of stripe_rows rows, each stripe is
 * one dynamic-Huffman deflate block (BFINAL 0; literals and end-of-block only, no matches; HLIT 0, HDIST 0 with the one distance
 * length 0, HCLEN 15 with code-length code lengths 0 for 16 / 17 / 18 and 4 for 0 .. 15, so the 258 lengths follow as plain 4-bit
 * codes) and an empty stored block behind it, which pads to a byte: stripes are independent bit streams.  `03 00` (final fixed block,
 * end-of-block only) and the Adler-32 end the stream.  Literal code lengths per stripe: a Huffman code of the stripe's histogram
 * (end-of-block counts 1), limited to 15 bits where the tree is deeper, canonical codes (RFC 1951 3.2.2).
 * The 4 bytes of the IDAT chunk's CRC are written as zeros: the caller computes the CRC-32 over tag + data on the host, or calls
 * sdv_png_crc32.
 *
 * sdv_png_filter_u8      frames uint8 RGB NHWC [n][H][W][3] contiguous -> filtered uint8 [n][H][1 + 3W] and adler_rows uint32 [n][H][2]:
 *   per row (sum d_j, sum (R - j) d_j) mod 65521 over its R = 1 + 3W bytes, j = 0 .. R - 1.  One launch.
 *
 * sdv_png_deflate_pack   filtered (4-byte aligned) + adler_rows -> out: n complete files back to back, out[offsets[k] .. offsets[k + 1])
 *   is file k; offsets int64 [n + 1] and needed int64 [1] (= offsets[n]) in GPU memory.  header: the 33 bytes signature + IHDR chunk
 *   (GPU memory).  scratch: 8-byte aligned, at least 16 * S + 8 * ((n + 1) / 2) + 1040 * S bytes for S = n * ceil(H / stripe_rows)
 *   stripes.  lengths: NULL or uint8 [n][ceil(H / stripe_rows)][257], receives the literal / end-of-block code lengths used.
 *   When *needed > out_cap NOTHING is written to out (offsets, needed and lengths still are): the caller retries with *needed bytes.
 *   Three launches on `stream`: count (one wave per stripe: histogram, code lengths, codes, byte length), scan (positions, Adler-32),
 *   write (one wave per stripe, storing at the final positions).
 * 1 <= H, W <= 16384, 1 <= n <= 65535, 1 <= stripe_rows <= H.
 *
 * Matching mode (opt-in; additive, the version stays 12).  Container, filtering, Adler-32, `78 01`, the stripes, the empty stored
 * block behind each, `03 00` and one dynamic block per stripe are as above; only the inside of a stripe's block changes.  For one
 * stripe with bytes s[0 .. L), R = 1 + 3W:
 *   prices      l0[v]: the 257 code lengths of the Huffman-only code of this stripe (what sdv_png_deflate_pack would use).
 *   candidates  at position i with i + 3 <= L; every distance d has 1 <= d <= i and d <= 32768: the fixed distances 1, 2, 3, 4, 6,
 *               R - 3, R, R + 3, and one hash candidate d = i - j, j the LARGEST position with j < 64 * (i / 64), j + 3 <= L and
 *               h(j) == h(i), h(p) = ((s[p] | s[p+1] << 8 | s[p+2] << 16) * 0x9E3779B1 mod 2^32) >> 20 (12 bits): the hash sees only
 *               positions of earlier 64-position groups.
 *   length      the common prefix of s[i ..] and s[i - d ..] (overlap allowed), at most min(258, L - i); the best candidate is the
 *               longest, ties go to the smaller d.
 *   acceptance  a best match of length len >= 3 is taken iff  sum(l0[s[i + k]], k < len) > 12 + length extra bits + distance extra
 *               bits  (RFC 1951 3.2.5).
 *   parse       greedy from i = 0: an accepted match advances by len, else the literal by 1.  No match reaches outside its stripe.
 *   block       no accepted match in the stripe: the block of sdv_png_deflate_pack, byte for byte.  Else BFINAL 0, BTYPE 10,
 *               HLIT 29, HDIST 29, HCLEN 15, the same 19 code-length code lengths, 286 + 30 lengths as plain 4-bit codes, the
 *               tokens, end-of-block.  Literal / length code: Huffman of the token histogram over 286 symbols (end-of-block counts
 *               1); distance code: the same over 30 symbols, a single used symbol gets length 1; both limited to 15 bits.
 *
 * sdv_png_deflate_lz_pack  sdv_png_deflate_pack's arguments and contract (lengths: the PRICES l0), and: lz_scratch, 8-byte aligned, at
 *   least 4 * n H R + 8 * ((S + 1) / 2) + 1280 * S bytes: first the tokens, uint32 [n H R], a stripe's tokens from the index of its
 *   first filtered byte (len << 16 | dist for a match, the byte for a literal), then the token count of every stripe, uint32 [S],
 *   then code words.  ll_lengths / d_lengths: NULL or uint8 [n][stripes][286] / [n][stripes][30], the final code lengths of every
 *   stripe (a stripe without a match: l0 and zeros).  Six launches: count, match (one wave per stripe, 64 positions at a time),
 *   token count, scan, write (stripes without a match), token write.
 *
 * sdv_png_crc32            the CRC-32 (zlib's) of every file's IDAT tag + data, out[offsets[k] + 37 .. offsets[k + 1] - 16), stored
 *   big-endian into the 4-byte hole behind it.  offsets / needed: what a packer left in GPU memory; does nothing when
 *   *needed > out_cap.  acc: uint32 [n] workspace.  A memset and two launches: 256-byte chunks, each shifted to its place by
 *   x^(8 * bytes behind it) mod P and XOR-ed into its file's accumulator; then the preset and final-inversion terms and the store. */
int sdv_png_filter_u8(const uint8_t* frames, int32_t n, int32_t H, int32_t W, uint8_t* filtered, uint32_t* adler_rows, void* stream);
int sdv_png_deflate_pack(const uint8_t* filtered, const uint32_t* adler_rows, int32_t n, int32_t H, int32_t W, int32_t stripe_rows,
                         const uint8_t* header, int32_t header_len, void* scratch, int64_t scratch_bytes, uint8_t* out,
                         int64_t out_cap, int64_t* offsets, int64_t* needed, uint8_t* lengths, void* stream);
int sdv_png_deflate_lz_pack(const uint8_t* filtered, const uint32_t* adler_rows, int32_t n, int32_t H, int32_t W, int32_t stripe_rows,
                            const uint8_t* header, int32_t header_len, void* scratch, int64_t scratch_bytes, uint8_t* out,
                            int64_t out_cap, int64_t* offsets, int64_t* needed, uint8_t* lengths, void* lz_scratch,
                            int64_t lz_scratch_bytes, uint8_t* ll_lengths, uint8_t* d_lengths, void* stream);
int sdv_png_crc32(uint8_t* out, int64_t out_cap, const int64_t* offsets, const int64_t* needed, int32_t n, uint32_t* acc, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------------------
 * H.264 CAVLC intra encoder (utils.py:69-128: the reference's libx264 crf 10 yuv420p track).  Four additive entry points (50 with
 * them; the ABI version stays 12); opt-in (video.py: SDV_VIDEO_CODEC=h264-cavlc), the default track is untouched.
 *
 * Stream rule.  Parameter sets: those of the I_PCM track (profile 66 with constraint_set0/1, CAVLC, POC type 2, deblocking control
 * present, pic_init_qp 26).  Per picture one IDR slice NAL unit per macroblock row: first_mb_in_slice = row * mbw, slice_type 7,
 * frame_num 0, idr_pic_id = (first_index + frame) & 1 in every slice of the picture, slice_qp_delta = qp - 26,
 * disable_deblocking_filter_idc 1.  A slice boundary makes the row above unavailable: every row is an independent byte-aligned bit
 * stream, and one mp4 sample is the picture's mbh slices, each behind its 4-byte big-endian length.
 *   Macroblocks: Intra16x16, prediction mode 2 (DC: 128 for the first macroblock of a row, else (sum of the 16 reconstructed samples
 *   left of it + 8) >> 4), intra_chroma_pred_mode 0 (DC, 8.3.4 with the left neighbour only: per half column (sum of 4 + 2) >> 2),
 *   mb_qp_delta 0, mb_type = 1 + 2 + 4 cbp_chroma + 12 (cbp_luma == 15); cbp_luma = 15 when any luma AC level is nonzero, else 0;
 *   cbp_chroma = 2 when any chroma AC level is nonzero, else 1 when any chroma DC level is, else 0.
 *   Transform: W = Cf X Cf^T per 4x4 block of source - prediction; luma DCs Yd = (H Wd H + 1) >> 1, chroma DCs Yd = H2 Wd H2.
 *   Quantisation: |Z| = (|W| MF + f) >> qbits, sign kept, qbits = 15 + qp / 6, f = (1 << qbits) / 3, MF by qp % 6 and position class
 *   {13107 5243 8066, 11916 4660 7490, 10082 4194 6554, 9362 3647 5825, 8192 3355 5243, 7282 2893 4559}; DC blocks 2 f and
 *   qbits + 1.  Chroma uses QPc of Table 8-15 (chroma_qp_index_offset 0).
 *   CAVLC (9.2): Intra16x16DCLevel, the 16 AC blocks by luma4x4BlkIdx (15 levels each; only with cbp_luma 15), chroma DC Cb / Cr (with
 *   cbp_chroma > 0), chroma AC Cb 0..3, Cr 0..3 (with cbp_chroma 2).  nC from the AC TotalCoeff of the left / top blocks, the row above
 *   unavailable, an I_PCM neighbour counting 16.
 *   Reconstruction per 8.5 (dequantise, inverse transforms, clip) feeds the next macroblock's prediction.
 *   I_PCM (mb_type 25, alignment zeros, the 384 source samples) when macroblock_layer() would take more than 3200 bits (A.3.1) or a
 *   level needs level_prefix > 15; its reconstruction is the source, its blocks count TotalCoeff 16.
 *   Colour: Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16, Cb = ((S(-38 R - 74 G + 112 B) + 512) >> 10) + 128,
 *   Cr = ((S(112 R - 94 G - 18 B) + 512) >> 10) + 128, S the sum over the 2 x 2 box; planes edge-replicated to multiples of 16.
 *   NAL header 0x65 and emulation prevention as in h264.nal_unit.
 *
 * Capacity.  A macroblock takes at most 3200 bits = 400 bytes (I_PCM: 9 + 7 + 3072 bits), the slice header and the stop bit at most
 * 8 bytes, so a slice's RBSP at most 400 mbw + 8 bytes; emulation prevention adds at most one byte per two; with the NAL header and
 * the 4-byte length one slice takes at most
 *     slot = 5 + (400 mbw + 8) + (400 mbw + 8) / 2 = 600 mbw + 17 bytes,
 * a batch at most n mbh slot bytes - the out_cap that the packer demands (less is refused, nothing is launched).  The scratch buffer
 * holds one slot per slice at a stride of slot rounded up to 8, then an int64 start and an int32 length per slice:
 *     scratch_bytes >= n mbh (((slot + 7) & ~7) + 12).
 *
 * sdv_h264_planes_u8      frames uint8 [n][H][W][3] (H, W even, 2 .. 16384) -> y uint8 [n][16 mbh][16 mbw], cb / cr uint8
 *   [n][8 mbh][8 mbw].  One launch.
 * sdv_h264_encode_rows    planes (y 16-byte, cb / cr 8-byte aligned) -> every slice complete in its slot of scratch (8-byte aligned),
 *   and its length.  qp 0 .. 51.  One launch, one wave per slice.
 * sdv_h264_pack           slots -> out, the slices back to back in sample order; offsets int64 [n + 1]: sample k is
 *   out[offsets[k] .. offsets[k + 1]).  Two launches (scan, copy).
 * sdv_h264_vlc_tables     HOST pointers, no GPU work: the kernel's VLC tables as lengths uint8 [656] and codes uint16 [656] (length 0 =
 *   no such symbol).  coeff_token at [68 t + 4 TotalCoeff + TrailingOnes] for the tables t of nC 0-1, 2-3, 4-7, 8+, chroma DC at
 *   [272 + 4 TotalCoeff + TrailingOnes]; total_zeros at [292 + 16 (TotalCoeff - 1) + total_zeros], chroma DC at
 *   [532 + 4 (TotalCoeff - 1) + total_zeros]; run_before at [544 + 16 (min(zerosLeft, 7) - 1) + run_before]. */
int sdv_h264_planes_u8(const uint8_t* frames, int32_t n, int32_t H, int32_t W, uint8_t* y, uint8_t* cb, uint8_t* cr, void* stream);
int sdv_h264_encode_rows(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                         int32_t first_index, void* scratch, int64_t scratch_bytes, void* stream);
int sdv_h264_pack(void* scratch, int64_t scratch_bytes, int32_t n, int32_t mbh, int32_t mbw, uint8_t* out, int64_t out_cap,
                  int64_t* offsets, void* stream);
int sdv_h264_vlc_tables(uint8_t* host_lengths, uint16_t* host_codes, int32_t count);

/* ------------------------------------------------------------------------------------------------------------------------------------
 * H.264 P pictures (zero-motion inter prediction) for the CAVLC encoder above.  One additive entry point (51 with it; the ABI version
 * stays 12); opt-in (h264_cavlc.H264Encoder(gop=...), video.py: SDV_H264_GOP), gop 1 runs sdv_h264_encode_rows and writes its bytes.
 *
 * Stream rule.  Setting gop, an integer 1 .. 256.  Within one call picture k (position in the call) is an IDR picture iff k % gop == 0,
 * coded exactly as above (slice header, idr_pic_id = (first_index + k) & 1, frame_num 0); the others are P pictures.  Every call
 * starts a new GOP: no reference crosses a call.  Parameter sets unchanged (max_num_ref_frames 1, one active reference, POC type 2,
 * frame_num u(4)).
 *   P picture: one slice NAL unit per macroblock row, NAL header 0x41 (nal_ref_idc 2, type 1).  Slice header: first_mb_in_slice =
 *   row * mbw, slice_type 5, pic_parameter_set_id 0, frame_num = (k % gop) & 15, num_ref_idx_active_override_flag 0,
 *   ref_pic_list_modification_flag_l0 0, adaptive_ref_pic_marking_mode_flag 0, slice_qp_delta = qp - 26,
 *   disable_deblocking_filter_idc 1.  Slice data: mb_skip_run before every coded macroblock, and once more at the end of a slice that
 *   ends in skipped macroblocks.  Every vector is (0, 0): the row above is unavailable, so the predictor is (0, 0) and P_Skip infers it.
 *   Mode (luma only): sad_inter = sum |src - ref| over the co-located 16 x 16 of the previous picture's reconstruction, sad_intra =
 *   sum |src - DC| with the Intra16x16 DC predictor (128 at the start of a row); intra iff sad_intra < sad_inter, else inter.
 *   Inter: residual src - ref; every luma 4x4 block 16 coefficients (no DC transform); chroma as above (2x2 Hadamard of the DCs, 15
 *   AC).  Quantisation as above with f = (1 << qbits) / 6 (DC blocks 2 f, qbits + 1).  cbp luma bit b set iff any level of 8x8 block b
 *   is nonzero, chroma 0 / 1 / 2 as above.  cbp 0: P_Skip.  Else P_L0_16x16: mb_type ue(0), mvd_l0 se(0) se(0), coded_block_pattern
 *   me(v) by the inter column of Table 9-4 (codeNum -> cbp: 0 16 1 2 4 8 32 3 5 10 12 15 47 7 11 13 14 6 9 31 35 37 42 44 33 34 36 40
 *   39 43 45 46 17 18 20 24 19 21 26 28 23 27 29 30 22 25 38 41), mb_qp_delta se(0), residual: luma blocks by luma4x4BlkIdx in the 8x8s
 *   whose cbp bit is set (maxNumCoeff 16), chroma DC, chroma AC.
 *   nC as in 9.2.1: an uncoded or skipped block counts 0, an inter block its 16-coefficient TotalCoeff, an Intra16x16 block its AC
 *   TotalCoeff, I_PCM 16.
 *   Intra in a P slice: as in an IDR slice with mb_type ue(5 + intra mb_type); constrained_intra_pred_flag is 0, the left neighbour's
 *   reconstruction is used whatever its mode.  I_PCM: mb_type ue(30), by the same two triggers (macroblock_layer() above 3200 bits, or
 *   level_prefix > 15).
 *   Reconstruction per 8.5 of ALL samples of every macroblock (IDR pictures included; P_Skip copies the reference, I_PCM the source)
 *   into the planes ry / rcb / rcr: picture k's reference is picture k - 1 of them.  All integer: it is the decoder's picture.
 *
 * Capacity of the GOP path.  first_mb_in_slice < 2^20 takes at most 41 bits, so a P slice header takes at most 41 + 5 + 1 + 4 + 3 + 11 +
 * 3 = 68 bits (an IDR one 41 + 7 + 1 + 4 + 3 + 2 + 11 + 3 = 72); an mb_skip_run (< 1024) at most 21 bits; a coded macroblock at most
 * 3200 bits (I_PCM in a P slice 9 + 7 + 3072).  With one run per macroblock, the trailing run, the stop bit and 7 alignment zeros a
 * slice's RBSP takes at most (68 + 3221 mbw + 21 + 8 + 7) / 8 <= 403 mbw + 13 bytes, with emulation prevention, NAL header and length
 * at most 5 + 3 (403 mbw + 13) / 2 <= 604.5 mbw + 25 bytes.  That is above the intra slot, so the GOP path takes the slots of a
 * picture   mbw' = mbw + 1 + mbw / 64   macroblocks wide: 600 mbw' + 17 >= 600 mbw + 617 + 600 (mbw / 64 - 63 / 64) > 604.5 mbw + 25
 * for every mbw >= 1.  Scratch and output are those of the intra path at (n, mbh, mbw'), so sdv_h264_pack(scratch, n, mbh, mbw', ...)
 * packs them; mbw' <= 1024 limits the GOP path to mbw <= 1008.  The writer checks every store against its slot whatever the input.
 *
 * sdv_h264_encode_gops    planes as for sdv_h264_encode_rows; ry (16-byte aligned) / rcb / rcr (8-byte) uint8 in the planes' layout,
 *   written whole; scratch_bytes >= that of (n, mbh, mbw').  One launch, one wave per (GOP, macroblock row), the macroblock's 24 4x4
 *   blocks one lane each. */
int sdv_h264_encode_gops(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                         int32_t gop, int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDV_HIP_H */
