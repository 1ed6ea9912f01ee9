/*
 * sdv_hip_h264_part.h - macroblock partitions of the H.264 track: four more additive entry points of ABI 12 of libsdv_hip.so.  They are
 * exported by the same library as those of sdv_hip.h, sdv_hip_ext.h, sdv_hip_h264_sub.h, sdv_hip_h264_i4.h and sdv_hip_h264_lf.h, follow
 * their conventions (device pointers, `stream` a hipStream_t passed as void*, enqueue only, 0 = ok, negative = argument error with the
 * message in sdv_last_error()) and leave every entry point, struct and byte of those five headers as it is; sdv_abi_version() stays 12.
 * The Python binding keeps them in a table of its own (hip.H264_PART_SYMBOLS).
 */
#ifndef SDV_HIP_H264_PART_H
#define SDV_HIP_H264_PART_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------------------------
 * H.264 partitions: P_8x8 macroblocks with one vector per 8x8 luma quadrant, for P pictures whose macroblocks hold more than one motion.
 * Opt-in on top of gop > 1 and search > 0 (h264_cavlc.H264Encoder(part=1), video.py: h264_part, SDV_H264_PART); part 0, the default,
 * runs the launches of the other headers and writes their bytes, and so does part 1 with gop 1 or search 0.  Valid with every subpel (0,
 * 1, 2, 4), intra4 and deblock.  A setting, not a measured optimum.  The stream has met no third-party decoder yet;
 * tests/h264_part_ref.py restates and decodes it.  The gain on a real walk is unmeasured.
 *
 * Stream rule (everything not named here is as in the other five headers).
 *   Vectors.  Four per inter macroblock, one per 8x8 luma quadrant: mbPartIdx 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right.
 *   Always in QUARTER luma samples in the tensor mv, int16 [n][mbh][mbw][4][2] (vx, vy).  Grid by subpel: 0 - every component a multiple
 *   of 8 quarter units (the even whole-sample grid of sdv_hip_ext.h); 1, 2, 4 - a multiple of 4 / subpel as in sdv_hip_h264_sub.h.
 *   |vx|, |vy| <= 4 search.  Admission is the MACROBLOCK's own 16x16 rule of those headers, for all four vectors: with ix0 = floor(vx / 4),
 *   ix1 = ceil(vx / 4), 16 mx + ix0 >= 0 and 16 mx + ix1 + 16 <= 16 mbw, likewise y.  One candidate set serves every macroblock and every
 *   partition; no partition is admitted a vector the 16x16 block would be refused.
 *   Macroblock type.  Four equal vectors are coded exactly as before: P_Skip when cbp is 0 and v = (0, 0), else P_L0_16x16.  Otherwise
 *   P_8x8: mb_type ue(3); four sub_mb_type ue(0) (P_L0_8x8); no ref_idx (one active reference); mvd_l0 x then y for partitions 0, 1, 2,
 *   3; coded_block_pattern me(v) by the inter column; mb_qp_delta se(0) only with cbp != 0; the residual as before.  16x8, 8x16, sub-8x8
 *   partitions and P_8x8ref0 are never written.
 *   Vector prediction (8.4.1.3).  The row above is another slice - for all four partitions.  A partition that is not available, or is
 *   intra, has the vector (0, 0) and refIdx -1.  Where B and C are both unavailable and A is available, B and C take A's values.  The
 *   predictor is the one neighbour whose refIdx is 0 when exactly one is, else the componentwise median.  Per partition:
 *     0: A is the left macroblock's top-right 8x8 (its one vector when it is not P_8x8, (0, 0) when P_Skip); B, C, D are unavailable:
 *        mvp = mvA, (0, 0) when the left macroblock is absent or intra.
 *     1: A = partition 0; B is unavailable, C (above-right) and its replacement D too: mvp = v0.
 *     2: A is the left macroblock's bottom-right 8x8, B = partition 0, C = partition 1: median(A, v0, v1), A = (0, 0) when absent or intra
 *        (two neighbours then have refIdx 0, so the median it is).
 *     3: A = partition 2, B = partition 1; C lies in the macroblock to the right, not yet decoded, and is replaced by D = partition 0:
 *        median(v2, v1, v0).
 *   A P_L0_16x16 macroblock to the right of a P_8x8 one predicts from that macroblock's partition 1.  P_Skip still always infers (0, 0).
 *   Prediction.  Per partition: luma 8.4.2.2.1 on the 8x8 block, chroma 8.4.2.2.2 on the 4x4 block of each plane, with the partition's
 *   vector; filter taps and the chroma +1 sample read with the coordinate clamp Clip3(0, w - 1, .).  With whole even vectors it is the
 *   displaced copy.
 *   Mode, residual, capacity.  sad_inter is the sum over the four displaced partitions against the reconstruction; intra iff sad_intra <
 *   sad_inter.  Residual, quantisation, cbp, nC and the I_PCM triggers are unchanged; the counting pass includes the real bits of mb_type,
 *   the sub types and the four mvd pairs, so a coded macroblock still takes at most 3200 bits.  Capacity: a P slice of mbw macroblocks is
 *   at most 600 (mbw + 1 + mbw / 64) + 17 bytes as before - the header and trailing bits are unchanged, each coded macroblock is at most
 *   3200 bits = 400 bytes or I_PCM (384 bytes + at most 7 + 11 bits), each mb_skip_run at most 21 bits (mbw <= 1008), emulation
 *   prevention adds at most one byte in two; none of these figures depends on the macroblock type, so mbw' = mbw + 1 + mbw / 64 holds.
 *   Search.  On source pictures, one launch over all P pictures of a call.  Stage 1 is the exhaustive pass over the admitted whole-sample
 *   vectors (subpel 0: the even ones), keeping for every candidate the four quadrant SADs as well as their sum.  For quadrant q,
 *   cost8_q(v) = SAD_q(v) + lambda(qp) (B(vx) + B(vy)), B(c) the length of se(c) in quarter units, total order (cost, |vx| + |vy|, vy, vx).
 *   Stages 2 and 3 (subpel >= 2, subpel 4) refine each quadrant's winner by the rule of sdv_hip_h264_sub.h on its 64 samples.  The 16x16
 *   winner w16 is found exactly as before.  The four quadrant winners are taken iff sum_q cost8_q + 8 lambda(qp) < cost16(w16) (strict; 8
 *   = the extra syntax bits against P_L0_16x16: ue(3) for ue(0), and four ue(0)); otherwise w16 is written four times.  The mv tensor
 *   alone carries the decision.  A flat, repeated or uniformly moving picture yields four equal vectors everywhere.
 *   Loop filter.  With deblock 1, bS as in sdv_hip_h264_lf.h with the vectors compared per 4-sample segment between the 8x8 partitions that
 *   meet there.  Inner edges 4 and 12 lie inside a partition; inner edge 8, vertical and horizontal, separates two partitions and gets bS
 *   1 where their vectors differ by >= 4 in a component, unless coefficients make it 2.  A macroblock edge compares this macroblock's left
 *   or top partitions with the neighbour's right or bottom ones, half an edge at a time.
 *
 * Side information.  mbinfo as in sdv_hip_h264_lf.h; bit 18 keeps its meaning (all four coded vectors are (0, 0)); bits 19 .. 22: the
 * coded vector of partition 0 .. 3 is (0, 0) whatever `mv` holds (set in inter and P_Skip macroblocks; an intra macroblock's vectors are
 * never read).  Bits 23 .. 31 zero.
 *
 * Every entry point refuses, without a launch: null or misaligned pointers, counts that are not those of the grid (mv_count = 8 n mbh mbw
 * int16 elements, sad_count = 5 n mbh mbw, mbinfo_count = n mbh mbw), subpel outside {0, 1, 2, 4}, search odd or outside 2 .. 16.
 *
 * sdv_h264_motion_search_part  as sdv_h264_motion_search_sub with subpel 0 allowed; writes mv [n][mbh][mbw][4][2] (zeros for the IDR
 *   pictures) and, when sad is not null, sad int32 [n][mbh][mbw][5]: the source SADs of the four quadrant winners and of w16, whatever the
 *   decision.  One wave per macroblock, the LDS window of sdv_h264_motion_search_sub; lanes own candidates in stage 1 and samples in
 *   stages 2 / 3, where a quadrant is 16 lanes and the four refinements run side by side with 16-lane sums.
 * sdv_h264_encode_gop_step_part, sdv_h264_encode_gop_step_part_lf  as sdv_h264_encode_gop_step_sub and _sub_lf with subpel 0 .. 4 and four
 *   vectors per macroblock.  Each vector is validated for itself: one that is off the grid, out of range or not admitted is coded as
 *   (0, 0).  The prediction is interpolated from four clamped 13 x 13 luma and 5 x 5 chroma windows, so no read leaves a plane.  One wave
 *   per (GOP, macroblock row), the serial part on lane 0.  IDR pictures may go through the k = 0 step or through sdv_h264_encode_idr4(_lf).
 * sdv_h264_deblock_part  sdv_h264_deblock with the four-vector tensor (always quarter samples, so no subpel) and bits 19 .. 22. */
int sdv_h264_motion_search_part(const uint8_t* y, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t search, int32_t subpel,
                                int16_t* mv, int64_t mv_count, int32_t* sad, int64_t sad_count, void* stream);
int sdv_h264_encode_gop_step_part(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                  int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv, int64_t mv_count,
                                  uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, void* stream);
int sdv_h264_encode_gop_step_part_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                     int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                     int64_t mv_count, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                     uint32_t* mbinfo, int64_t mbinfo_count, void* stream);
int sdv_h264_deblock_part(uint8_t* ry, uint8_t* rcb, uint8_t* rcr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t k,
                          const uint32_t* mbinfo, int64_t mbinfo_count, const int16_t* mv, int64_t mv_count, int32_t waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDV_HIP_H264_PART_H */
