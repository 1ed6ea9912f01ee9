// Safety-checker glue around the CLIP vision tower (sdv_hip.h "Safety checker"): the two kernels that are not a transformer.
//
//   sdv_clip_preprocess_patches   uint8 RGB NHWC frames -> the patch-embedding GEMM operand (CLIPImageProcessor + the im2col of
//                                 the stride-P patch convolution), ONE launch, no intermediate image in HBM
//   sdv_safety_screen             cosine head of StableDiffusionSafetyChecker + black-out of the flagged frames
//
// Everything between them (patch GEMM, LayerNorms, attention, MLP) runs on sdv_gemm_bf16 / sdv_layernorm_bf16 /
// sdv_attention_bf16 (vision.py).
#include "sdv_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBudget = 64 * 1024;      // static + dynamic LDS a workgroup may take without opting in to more

// ---------------------------------------------------------------------------------------------------------------------------
// Preprocess.  PIL's Image.resize(BICUBIC) is separable: a horizontal pass over the rows the vertical pass needs, then the
// vertical pass; every output sample i has its own taps (first source index off[i], count cnt[i], weights w[i][0..cnt), already
// normalised to sum 1 - the host builds the tables, vision.py::resample_taps).  The tables here are those of the CROP window only
// (S entries per axis).  One workgroup = one band of P output rows of one frame = one row of patches:
//     for each chunk of source rows:  hbuf[r][ox][c] = sum_t wx[ox][t] * frame[r][xoff[ox] + t][c]        (pass 1, into LDS)
//                                     acc[py][ox][c] += wy[oy][r - yoff[oy]] * hbuf[r][ox][c]             (pass 2, LDS accumulators)
// both in fp32, no rounding in between; then (acc / 255 - mean[c]) / std[c] -> bf16 rows [(c, py, px) | zero pad] of the G patches.
// Every thread owns a fixed set of accumulators, so the only hazards are on hbuf (two barriers per chunk).
// Source indices are clamped into the frame: a corrupt table gives wrong pixels, never an access outside the buffer.
// ---------------------------------------------------------------------------------------------------------------------------
struct norm3_t { float mean[3], inv_std[3]; };

__global__ __launch_bounds__(kThreads) void clip_preprocess_kernel(
    const uint8_t* __restrict__ frames, uint16_t* __restrict__ out, const int* __restrict__ xoff, const int* __restrict__ xcnt,
    const float* __restrict__ xw, const int* __restrict__ yoff, const int* __restrict__ ycnt, const float* __restrict__ yw, int H, int W,
    int S, int P, int Kpad, int xtaps, int ytaps, int chunk_rows, norm3_t nrm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int G = S / P;
    const int gy = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int row3 = S * 3;
    const int nacc = P * row3;
    float* acc = lds;                   // [P][S][3]
    float* hbuf = lds + nacc;           // [chunk_rows][S][3]
    for (int a = tid; a < nacc; a += kThreads) acc[a] = 0.f;
    // source rows of the band: [lo, hi)
    int lo = H, hi = 0;
    for (int py = 0; py < P; ++py) {
        const int o = yoff[gy * P + py], c = min(max(ycnt[gy * P + py], 0), ytaps);
        lo = min(lo, o);
        hi = max(hi, o + c);
    }
    lo = max(lo, 0);
    hi = min(hi, H);
    const uint8_t* img = frames + (long long)b * H * W * 3;
    for (int r0 = lo; r0 < hi; r0 += chunk_rows) {
        const int nr = min(chunk_rows, hi - r0);
        __syncthreads();                // the previous chunk's pass 2 (and the zero fill) is done with hbuf / acc
        for (int i = tid; i < nr * row3; i += kThreads) {
            const int rr = i / row3, rem = i - rr * row3;
            const int ox = rem / 3, c = rem - ox * 3;
            const uint8_t* src = img + (long long)(r0 + rr) * W * 3 + c;
            const int x0 = xoff[ox], nt = min(max(xcnt[ox], 0), xtaps);
            const float* wt = xw + (long long)ox * xtaps;
            float s = 0.f;
            for (int t = 0; t < nt; ++t) s += wt[t] * (float)src[min(max(x0 + t, 0), W - 1) * 3];
            hbuf[i] = s;
        }
        __syncthreads();
        for (int a = tid; a < nacc; a += kThreads) {
            const int py = a / row3, rem = a - py * row3;
            const int oy = gy * P + py;
            const int y0 = yoff[oy], nt = min(max(ycnt[oy], 0), ytaps);
            const int t0 = max(r0 - y0, 0), t1 = min(r0 + nr - y0, nt);
            const float* wt = yw + (long long)oy * ytaps;
            float s = acc[a];
            for (int t = t0; t < t1; ++t) s += wt[t] * hbuf[(y0 + t - r0) * row3 + rem];
            acc[a] = s;
        }
    }
    __syncthreads();
    // patch rows of this band: G rows of Kpad columns, 8 columns (16 bytes) per thread and step
    const int K = 3 * P * P, PP = P * P;
    const int vec_per_row = Kpad / 8;
    uint16_t* orow = out + ((long long)b * G + gy) * G * Kpad;
    for (int v = tid; v < G * vec_per_row; v += kThreads) {
        const int gx = v / vec_per_row, col0 = (v - gx * vec_per_row) * 8;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            float val = 0.f;            // the pad columns K .. Kpad are written as zeros here, not by a memset
            if (col < K) {
                const int c = col / PP, r = col - c * PP;
                const int py = r / P, px = r - py * P;
                val = (acc[py * row3 + (gx * P + px) * 3 + c] * (1.0f / 255.0f) - nrm.mean[c]) * nrm.inv_std[c];
            }
            f[e] = val;
        }
        *(bf16x8_raw*)(orow + (long long)gx * Kpad + col0) = pack8(f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Screen.  One workgroup per image: cosine similarities of its embedding with the special-care and the concept embeddings (both
// sides L2-normalised, fp32), then the checker's threshold arithmetic; the black-out is a second grid over 16-byte pieces of the
// frame buffer that reads the flags of the first (same stream: ordered).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void safety_head_kernel(const float* __restrict__ emb, const float* __restrict__ concept_emb,
                                                               const float* __restrict__ special, const float* __restrict__ thr_c,
                                                               const float* __restrict__ thr_s, int D, int nc, int ns,
                                                               int* __restrict__ flags, float* __restrict__ scores) {
    __shared__ float cosv[64];
    __shared__ float red[kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* e = emb + (long long)b * D;
    float ss = 0.f;
    for (int d = tid; d < D; d += kThreads) ss += e[d] * e[d];
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float enorm = sqrtf(red[0] + red[1] + red[2] + red[3]);
    for (int j = wave; j < ns + nc; j += kThreads / 64) {          // row j: special-care embeddings first, then the concepts
        const float* v = j < ns ? special + (long long)j * D : concept_emb + (long long)(j - ns) * D;
        float dot = 0.f, vv = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float x = v[d];
            dot += x * e[d];
            vv += x * x;
        }
        dot = wave_sum(dot);
        vv = wave_sum(vv);
        if (lane == 0) cosv[j] = dot / (enorm * sqrtf(vv));
    }
    __syncthreads();
    if (tid == 0) {
        float adj = 0.f;
        for (int j = 0; j < ns; ++j) {
            const float s = cosv[j] - thr_s[j];                      // special = cos_s - thr_s + 0
            scores[(long long)b * (ns + nc) + j] = s;
            if (s > 0.f) adj = 0.01f;
        }
        int bad = 0;
        for (int j = 0; j < nc; ++j) {
            const float s = cosv[ns + j] - thr_c[j] + adj;           // concept = cos_c - thr_c + adj
            scores[(long long)b * (ns + nc) + ns + j] = s;
            bad |= s > 0.f;
        }
        flags[b] = bad;
    }
}

__global__ __launch_bounds__(kThreads) void safety_blackout_kernel(uint8_t* __restrict__ frames, const int* __restrict__ flags,
                                                                   long long frame_bytes, long long total_bytes) {
    const long long first = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (first >= total_bytes) return;
    const long long last = min(first + 15, total_bytes - 1);
    const long long f0 = first / frame_bytes, f1 = last / frame_bytes;
    if (f0 == f1 && last - first == 15) {
        if (flags[f0]) *(uint4*)(frames + first) = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    for (long long i = first; i <= last; ++i)                        // a piece that straddles two frames, or the tail
        if (flags[i / frame_bytes]) frames[i] = 0;
}

}  // namespace

extern "C" int sdv_clip_preprocess_patches(const uint8_t* frames, sdv_bf16* patches, int32_t n, int32_t H, int32_t W, int32_t S, int32_t P,
                                           int32_t Kpad, const int32_t* x_off, const int32_t* x_cnt, const float* x_w, int32_t x_taps,
                                           const int32_t* y_off, const int32_t* y_cnt, const float* y_w, int32_t y_taps,
                                           const float* host_mean, const float* host_std, void* stream) {
    SDV_REQUIRE(frames && patches && x_off && x_cnt && x_w && y_off && y_cnt && y_w && host_mean && host_std,
                "sdv_clip_preprocess_patches: null pointer");
    SDV_REQUIRE(n > 0 && H > 0 && W > 0 && S > 0 && P > 0 && S % P == 0, "sdv_clip_preprocess_patches: bad shape n=%d H=%d W=%d S=%d P=%d (S %% P == 0)",
                n, H, W, S, P);
    SDV_REQUIRE(n <= 65535 && S / P <= 65535, "sdv_clip_preprocess_patches: too many frames / patch rows for one grid");
    const long long K = 3LL * P * P;
    SDV_REQUIRE(Kpad == (K + 63) / 64 * 64, "sdv_clip_preprocess_patches: Kpad=%d must be 3*P*P = %lld rounded up to a multiple of 64", Kpad, K);
    SDV_REQUIRE((((uintptr_t)patches) & 15) == 0, "sdv_clip_preprocess_patches: patches must be 16-byte aligned (16-byte row stores)");
    SDV_REQUIRE(x_taps > 0 && y_taps > 0 && x_taps <= W && y_taps <= H, "sdv_clip_preprocess_patches: bad tap counts %d / %d", x_taps, y_taps);
    SDV_REQUIRE((long long)n * H * W * 3 < (1LL << 40) && (long long)n * (S / P) * (S / P) * Kpad < (1LL << 40), "sdv_clip_preprocess_patches: tensor too large");
    for (int c = 0; c < 3; ++c) SDV_REQUIRE(host_std[c] > 0.f, "sdv_clip_preprocess_patches: image_std must be positive");
    const long long acc_bytes = (long long)P * S * 3 * 4, row_bytes = (long long)S * 3 * 4;
    SDV_REQUIRE(acc_bytes + row_bytes <= kLdsBudget, "sdv_clip_preprocess_patches: a band of P=%d rows of S=%d pixels does not fit in LDS", P, S);
    int chunk = (int)((kLdsBudget - acc_bytes) / row_bytes);
    if (chunk > H) chunk = H;
    norm3_t nrm;
    for (int c = 0; c < 3; ++c) nrm.mean[c] = host_mean[c], nrm.inv_std[c] = 1.0f / host_std[c];
    const size_t lds = (size_t)(acc_bytes + (long long)chunk * row_bytes);
    hipLaunchKernelGGL(clip_preprocess_kernel, dim3((unsigned)(S / P), (unsigned)n), dim3(kThreads), lds, (hipStream_t)stream, frames, patches,
                       x_off, x_cnt, x_w, y_off, y_cnt, y_w, H, W, S, P, Kpad, x_taps, y_taps, chunk, nrm);
    SDV_CHECK_LAUNCH("sdv_clip_preprocess_patches");
    return SDV_OK;
}

extern "C" int sdv_safety_screen(const float* image_embeds, const float* concept_embeds, const float* special_care_embeds,
                                 const float* concept_thr, const float* special_thr, int32_t n, int32_t D, int32_t n_concept,
                                 int32_t n_special, uint8_t* frames, int64_t frame_bytes, int32_t* flags, float* scores, void* stream) {
    SDV_REQUIRE(image_embeds && concept_embeds && special_care_embeds && concept_thr && special_thr && flags && scores,
                "sdv_safety_screen: null pointer");
    SDV_REQUIRE(n > 0 && D > 0, "sdv_safety_screen: bad shape n=%d D=%d", n, D);
    SDV_REQUIRE(n_concept > 0 && n_special >= 0 && n_concept + n_special <= 64, "sdv_safety_screen: at most 64 concept + special-care rows, got %d + %d",
                n_concept, n_special);
    SDV_REQUIRE(frames == nullptr || frame_bytes > 0, "sdv_safety_screen: frames without a frame size");
    SDV_REQUIRE((((uintptr_t)frames) & 15) == 0, "sdv_safety_screen: frames must be 16-byte aligned (16-byte black-out stores)");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(safety_head_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, image_embeds, concept_embeds, special_care_embeds,
                       concept_thr, special_thr, D, n_concept, n_special, flags, scores);
    SDV_CHECK_LAUNCH("sdv_safety_screen (head)");
    if (frames) {
        const long long total = (long long)n * frame_bytes, pieces = (total + 15) / 16;
        SDV_REQUIRE((pieces + kThreads - 1) / kThreads < 0x7fffffffLL, "sdv_safety_screen: frame buffer too large");
        hipLaunchKernelGGL(safety_blackout_kernel, dim3((unsigned)((pieces + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, frames, flags,
                           (long long)frame_bytes, total);
        SDV_CHECK_LAUNCH("sdv_safety_screen (black-out)");
    }
    return SDV_OK;
}
