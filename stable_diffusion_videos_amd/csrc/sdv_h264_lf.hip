// In-loop deblocking filter of the H.264 track (sdv_hip_h264_lf.h "H.264 deblocking"): the filter kernel, and the kLf forms of the three
// per-position encode kernels of sdv_h264_step.h behind the _lf entry points.  A unit of its own so that sdv_h264.hip compiles what it
// compiled before (see sdv_h264_step.h).
#include "sdv_common.h"
#include "sdv_h264_core.h"
#include "sdv_hip_h264_lf.h"
#include "sdv_h264_step.h"

namespace {

// In-loop deblocking filter (sdv_hip_h264_lf.h "H.264 deblocking"): the reconstruction planes of the pictures at position k of their GOPs,
// in place.  ONE workgroup per picture.  The standard filters macroblocks in raster order; macroblock (x, y) needs the finished (x - 1, y),
// (x, y - 1) and (x + 1, y - 1) (whose left edge rewrites columns 13 .. 15 of (x, y - 1)), so the macroblocks of one d = x + 2 y are
// independent and every dependency has a smaller d: the workgroup's waves share out a diagonal, one macroblock a wave, and a workgroup
// fence and barrier (uniform control flow) separate two diagonals.  No wave waits on anything another workgroup writes.
//
// A wave stages its macroblock with the 4 columns to its left and the 4 rows above it (chroma: 2 and 2; never the corner, which no clause
// reads) in an LDS window of its own, runs the vertical edges (lanes 0 - 15 one luma row each, lanes 16 - 31 one chroma row of one
// plane each, the edges of a direction one after the other) and then the horizontal ones through h264_lf_luma_line /
// h264_lf_chroma_line, and stores only what the clauses may have changed: its macroblock, 3 columns (chroma 1) of the left neighbour and
// 3 rows (chroma 1) of the upper one - not the window it read, whose fourth column / row other waves of the diagonal may not own.
constexpr int kLfWaves = 16;
constexpr int kLfLumaStride = 32, kLfLumaAt = 4 * kLfLumaStride + 16;       // sample (0, 0) of the macroblock inside its 20-row window
constexpr int kLfChromaStride = 16, kLfChromaAt = 2 * kLfChromaStride + 8;  // the same in a 10-row chroma window
struct __attribute__((aligned(16))) h264_lf_window {
    uint8_t y[20 * kLfLumaStride];
    uint8_t c[2][10 * kLfChromaStride];
};

__global__ __launch_bounds__(kLfWaves * 64) void h264_deblock_kernel(uint8_t* ry, uint8_t* rcb, uint8_t* rcr, int n, int mbh, int mbw, int qp, int gop,
                                                                     int k, int subpel, const uint32_t* __restrict__ mbinfo,
                                                                     const int16_t* __restrict__ mv) {
    __shared__ h264_lf_window win[kLfWaves];
    const long long f = (long long)blockIdx.x * gop + k;
    if (f >= n || qp < 16) return;                      // indexA <= qp < 16: alpha' = 0, no sample can change
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    uint8_t* py = ry + f * mbh * 16 * lw;
    uint8_t* pc[2] = {rcb + f * mbh * 8 * cw, rcr + f * mbh * 8 * cw};
    const uint32_t* info = mbinfo + f * mbh * mbw;
    const int16_t* vec = mv + f * mbh * mbw * 2;
    h264_lf_window& wn = win[wave];
    uint8_t* wy = wn.y + kLfLumaAt;
    for (int d = 0; d <= mbw - 1 + 2 * (mbh - 1); ++d) {
        const int ylo = d > mbw - 1 ? (d - mbw + 2) >> 1 : 0, yhi = min(mbh - 1, d >> 1);
        for (int i0 = 0; i0 <= yhi - ylo; i0 += waves) {
            const bool active = i0 + wave <= yhi - ylo;
            const int my = ylo + i0 + wave, mx = d - 2 * my;
            uint8_t* gy = py;
            uint8_t* gc[2] = {pc[0], pc[1]};
            h264_lf_side q, left, up;
            q.info = 0, q.vx = q.vy = 0, left = up = q;
            if (active) {
                const int at = my * mbw + mx;
                q = h264_lf_side_of(info[at], vec + 2 * at, subpel);
                left = mx ? h264_lf_side_of(info[at - 1], vec + 2 * (at - 1), subpel) : q;
                up = my ? h264_lf_side_of(info[at - mbw], vec + 2 * (at - mbw), subpel) : q;
                gy += (long long)my * 16 * lw + mx * 16;
                gc[0] += (long long)my * 8 * cw + mx * 8, gc[1] += (long long)my * 8 * cw + mx * 8;
                if (lane < 16) {                        // the macroblock's luma rows
                    *(uint4*)(wy + lane * kLfLumaStride) = *(const uint4*)(gy + lane * lw);
                } else if (lane < 32) {                 // 4 columns of the left neighbour
                    const int l = lane - 16;
                    if (mx) *(uint32_t*)(wy + l * kLfLumaStride - 4) = *(const uint32_t*)(gy + l * lw - 4);
                } else if (lane < 36) {                 // 4 rows of the upper neighbour
                    const int l = lane - 36;            // -4 .. -1
                    if (my) *(uint4*)(wy + l * kLfLumaStride) = *(const uint4*)(gy + l * lw);
                } else if (lane < 52) {                 // the macroblock's chroma rows
                    const int c = (lane - 36) >> 3, l = (lane - 36) & 7;
                    *(uint2*)(wn.c[c] + kLfChromaAt + l * kLfChromaStride) = *(const uint2*)(gc[c] + l * cw);
                }
                if (lane < 16) {                        // 2 chroma columns of the left neighbour
                    const int c = lane >> 3, l = lane & 7;
                    if (mx) *(uint16_t*)(wn.c[c] + kLfChromaAt + l * kLfChromaStride - 2) = *(const uint16_t*)(gc[c] + l * cw - 2);
                } else if (lane < 20) {                 // 2 chroma rows of the upper neighbour
                    const int c = (lane - 16) >> 1, l = ((lane - 16) & 1) - 2;
                    if (my) *(uint2*)(wn.c[c] + kLfChromaAt + l * kLfChromaStride) = *(const uint2*)(gc[c] + l * cw);
                }
            }
            __syncthreads();
            for (int dir = 0; dir < 2; ++dir) {
                if (active) {
                    const bool edge0 = (dir ? my : mx) > 0;
                    const h264_lf_side& nb = dir ? up : left;
                    if (lane < 16) {
                        for (int e = edge0 ? 0 : 1; e < 4; ++e) h264_lf_luma_line(wy, kLfLumaStride, dir, e, lane, e ? q : nb, q, qp);
                    } else if (lane < 32) {
                        const int c = (lane - 16) >> 3, l = (lane - 16) & 7;
                        for (int e = edge0 ? 0 : 1; e < 2; ++e)
                            h264_lf_chroma_line(wn.c[c] + kLfChromaAt, kLfChromaStride, dir, e, l, e ? q : nb, q, qp);
                    }
                }
                __syncthreads();
            }
            if (active) {
                if (lane < 16) {
                    *(uint4*)(gy + lane * lw) = *(const uint4*)(wy + lane * kLfLumaStride);
                } else if (lane < 32) {
                    const int l = lane - 16;
                    if (mx)
                        for (int j = -3; j < 0; ++j) gy[l * lw + j] = wy[l * kLfLumaStride + j];
                } else if (lane < 35) {
                    const int l = lane - 35;            // -3 .. -1
                    if (my) *(uint4*)(gy + l * lw) = *(const uint4*)(wy + l * kLfLumaStride);
                } else if (lane < 51) {
                    const int c = (lane - 35) >> 3, l = (lane - 35) & 7;
                    *(uint2*)(gc[c] + l * cw) = *(const uint2*)(wn.c[c] + kLfChromaAt + l * kLfChromaStride);
                }
                if (lane < 16) {
                    const int c = lane >> 3, l = lane & 7;
                    if (mx) gc[c][l * cw - 1] = wn.c[c][kLfChromaAt + l * kLfChromaStride - 1];
                } else if (lane < 18) {
                    const int c = lane - 16;
                    if (my) *(uint2*)(gc[c] - cw) = *(const uint2*)(wn.c[c] + kLfChromaAt - kLfChromaStride);
                }
            }
        }
        __threadfence_block();                          // this diagonal's stores before the next diagonal's loads, inside the workgroup
        __syncthreads();
    }
}

}  // namespace

// ---- in-loop deblocking filter (include/sdv_hip_h264_lf.h): the three per-position entry points with the side information, and the filter ----
#define H264_MBINFO_ARGS(name)                                                                                                          \
    SDV_REQUIRE(mbinfo, name ": null pointer");                                                                                          \
    SDV_REQUIRE((((uintptr_t)mbinfo) & 3) == 0, name ": mbinfo must be 4-byte aligned");                                                \
    SDV_REQUIRE(n > 0 && mbh > 0 && mbw > 0 && mbinfo_count == (int64_t)n * mbh * mbw,                                                   \
                name ": mbinfo holds %lld words, %d pictures of %d x %d macroblocks have %lld", (long long)mbinfo_count, n, mbh, mbw,    \
                (long long)n * mbh * mbw)

extern "C" int sdv_h264_encode_gop_step_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                           int32_t gop, int32_t k, int32_t search, int32_t first_index, const int16_t* mv, uint8_t* ry, uint8_t* rcb,
                                           uint8_t* rcr, void* scratch, int64_t scratch_bytes, uint32_t* mbinfo, int64_t mbinfo_count, void* stream) {
    H264_MBINFO_ARGS("sdv_h264_encode_gop_step_lf");
    return h264_encode_gop_step_impl<true>(y, cb, cr, n, mbh, mbw, qp, gop, k, search, first_index, mv, ry, rcb, rcr, scratch, scratch_bytes, mbinfo, stream);
}

extern "C" int sdv_h264_encode_gop_step_sub_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                               int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                               uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, uint32_t* mbinfo,
                                               int64_t mbinfo_count, void* stream) {
    H264_MBINFO_ARGS("sdv_h264_encode_gop_step_sub_lf");
    return h264_encode_gop_step_sub_impl<true>(y, cb, cr, n, mbh, mbw, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, scratch_bytes,
                                         mbinfo, stream);
}

extern "C" int sdv_h264_encode_idr4_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                       int32_t gop, int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch,
                                       int64_t scratch_bytes, uint32_t* mbinfo, int64_t mbinfo_count, void* stream) {
    H264_MBINFO_ARGS("sdv_h264_encode_idr4_lf");
    return h264_encode_idr4_impl<true>(y, cb, cr, n, mbh, mbw, qp, gop, first_index, ry, rcb, rcr, scratch, scratch_bytes, mbinfo, stream);
}

extern "C" int sdv_h264_deblock(uint8_t* ry, uint8_t* rcb, uint8_t* rcr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t k,
                                int32_t subpel, const uint32_t* mbinfo, int64_t mbinfo_count, const int16_t* mv, int32_t waves, void* stream) {
    SDV_REQUIRE(ry && rcb && rcr && mv, "sdv_h264_deblock: null pointer");
    H264_MBINFO_ARGS("sdv_h264_deblock");
    H264_GRID_ARGS("sdv_h264_deblock");
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_deblock: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_deblock: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(k >= 0 && k < gop && k < n, "sdv_h264_deblock: position k=%d outside 0 .. min(gop, n) - 1 (gop=%d, n=%d)", k, gop, n);
    SDV_REQUIRE(subpel == 0 || h264_subpel_ok(subpel), "sdv_h264_deblock: subpel=%d must be 0, 1, 2 or 4", subpel);
    SDV_REQUIRE(waves >= 0 && waves <= kLfWaves, "sdv_h264_deblock: waves=%d outside 0 .. %d (0 = the default)", waves, (int)kLfWaves);
    SDV_REQUIRE((((uintptr_t)ry) & 15) == 0 && (((uintptr_t)rcb) & 7) == 0 && (((uintptr_t)rcr) & 7) == 0 && (((uintptr_t)mv) & 3) == 0,
                "sdv_h264_deblock: ry must be 16-byte, rcb / rcr 8-byte, mv 4-byte aligned");
    const int longest = min(mbh, (mbw + 1) / 2);        // macroblocks on the longest diagonal x + 2 y
    const int use = waves ? waves : min((int)kLfWaves, longest);
    const long long pictures = (n - k + gop - 1) / gop; // the GOPs that have a picture at position k
    hipLaunchKernelGGL(h264_deblock_kernel, dim3((unsigned)pictures), dim3(64 * use), 0, (hipStream_t)stream, ry, rcb, rcr, n, mbh, mbw, qp, gop, k,
                       subpel, mbinfo, mv);
    SDV_CHECK_LAUNCH("sdv_h264_deblock");
    return SDV_OK;
}
