/*
 * sdv_hip_h264_sub.h - sub-sample motion vectors for the H.264 GOP path: two more additive entry points of ABI 12 of libsdv_hip.so.
 * They are exported by the same library as those of sdv_hip.h and sdv_hip_ext.h, follow their conventions (device pointers, `stream` a
 * hipStream_t passed as void*, enqueue only, 0 = ok, negative = argument error with the message in sdv_last_error()) and leave every
 * entry point, struct and byte of those two headers as it is; sdv_abi_version() stays 12.  The Python binding keeps them in a table of
 * their own (hip.H264_SUB_SYMBOLS).
 */
#ifndef SDV_HIP_H264_SUB_H
#define SDV_HIP_H264_SUB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------------------------
 * H.264 sub-sample motion: odd whole-sample, half-sample and quarter-sample vectors for the motion-compensated P pictures of
 * sdv_hip_ext.h ("H.264 motion search").  Opt-in on top of gop > 1 and search > 0 (h264_cavlc.H264Encoder(subpel=...), video.py:
 * h264_subpel, SDV_H264_SUBPEL); subpel 0, the default, runs the launches of sdv_hip_ext.h and writes their bytes.  A setting, not a
 * measured optimum.  The stream has met no third-party decoder yet; tests/h264_sub_ref.py restates and decodes it.
 *
 * Stream rule (an addition to "H.264 motion search"; everything not named here is as there).  Setting subpel in {1, 2, 4}: the
 * denominator of the vector grid (1: every whole sample, 2: half samples, 4: quarter samples).
 *   Units.  Vectors are in QUARTER luma samples everywhere: mv, the chain to the right neighbour, mvd = v - mvp.
 *   Grid.  Every component is a multiple of 4 / subpel, |vx|, |vy| <= 4 search.
 *   Admission.  With ix0 = floor(vx / 4), ix1 = ceil(vx / 4) (likewise y) a vector is admitted for macroblock (mx, my) iff
 *   16 mx + ix0 >= 0 and 16 mx + ix1 + 16 <= 16 mbw, and the same for y: the whole samples around the displaced block lie inside the
 *   coded (padded) picture.  For whole-sample vectors that is the rule of "H.264 motion search"; a one-macroblock picture has only
 *   (0, 0).  The filter taps beyond those samples (2 before, 2 after) are read with the standard's coordinate clamp
 *   Clip3(0, w - 1, .), in the encoder and the decoder alike; chroma reads xIntC + 1 / yIntC + 1 with the same clamp.
 *   Luma prediction (8.4.2.2.1).  G the whole sample at the integer part, H right of it, M below G, N below H.
 *   b1 = E - 5F + 20G + 20H - 5I + J over the row, b = Clip1((b1 + 16) >> 5); h the same over the column;
 *   j = Clip1((j1 + 512) >> 10), j1 the 6-tap over the unclipped b1 intermediates; m the h-type sample one column to the right, s the
 *   b-type sample one row below.  By (xFrac, yFrac), x across:
 *     yFrac 0:  G                  a = (G + b + 1) >> 1   b                      c = (H + b + 1) >> 1
 *     yFrac 1:  d = (G + h + 1)>>1 e = (b + h + 1) >> 1   f = (b + j + 1) >> 1   g = (b + m + 1) >> 1
 *     yFrac 2:  h                  i = (h + j + 1) >> 1   j                      k = (j + m + 1) >> 1
 *     yFrac 3:  n = (M + h + 1)>>1 p = (h + s + 1) >> 1   q = (j + s + 1) >> 1   r = (m + s + 1) >> 1
 *   Chroma prediction (8.4.2.2.2).  The vector is in eighth chroma samples: xIntC = 8 mx + (vx >> 3), xFracC = vx & 7 (likewise y);
 *   pred = ((8 - xF)(8 - yF) A + xF (8 - yF) B + (8 - xF) yF C + xF yF D + 32) >> 6.
 *   Search.  On source luma, picture k against SOURCE picture k - 1; fractional candidates use the luma interpolation above on the
 *   source picture.  cost(v) = SAD(v) + lambda(qp) * (B(vx) + B(vy)), B(c) the length of se(c), c in quarter samples; the lambda table
 *   is unchanged.  Total order (cost, |vx| + |vy|, vy, vx) in quarter samples, the last two signed.  Stage 1: exhaustive over all
 *   admitted whole-sample vectors, odd ones included (at most 33 x 33) -> w1.  Stage 2 (subpel >= 2): the admitted ones of
 *   w1 + 2 (dx, dy), dx, dy in {-1, 0, 1} -> w2.  Stage 3 (subpel 4): the admitted ones of w2 + (dx, dy) -> w3.  A flat or repeated
 *   picture still yields (0, 0).
 *   Unchanged.  Mode decision, residual, cbp, nC, the I_PCM trigger (its counting pass includes the real mvd bits) and P_Skip (cbp 0
 *   AND v = (0, 0)); slice headers, frame_num, stss, parameter sets, slot capacity.
 *
 * sdv_h264_motion_search_sub    as sdv_h264_motion_search, plus subpel in {1, 2, 4}; search even, 2 .. 16.  mv: int16
 *   [n][mbh][mbw][2] (vx, vy) in QUARTER samples, zeros for the IDR pictures; sad (may be null): int32 [n][mbh][mbw], the winner's
 *   source SAD.  One launch, one wave per macroblock: a clamped window of the previous source picture in LDS; stage 1 with lanes owning
 *   candidates, stages 2 and 3 with lanes owning 4 of the 256 samples and one wave-wide sum per candidate.
 * sdv_h264_encode_gop_step_sub  as sdv_h264_encode_gop_step, plus subpel after search, mv in quarter samples.  One picture position per
 *   launch, one wave per (GOP, macroblock row); the caller enqueues the positions in order on one stream.  The kernel does not trust
 *   mv: a vector that is off the subpel grid, outside the range or not admitted is coded as (0, 0).  The prediction is interpolated
 *   from clamped 21 x 21 luma and 9 x 9 chroma windows of the reference reconstruction, so no read leaves a plane. */
int sdv_h264_motion_search_sub(const uint8_t* y, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t search, int32_t subpel,
                               int16_t* mv, int32_t* sad, void* stream);
int sdv_h264_encode_gop_step_sub(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                 int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv, uint8_t* ry,
                                 uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDV_HIP_H264_SUB_H */
