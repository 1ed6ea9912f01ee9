/*
 * sdv_hip_ext.h - additive codec extensions of ABI 12 of libsdv_hip.so.  The entry points below are exported by the same library as
 * those of sdv_hip.h, follow its conventions (device pointers, `stream` a hipStream_t passed as void*, enqueue only, 0 = ok, negative =
 * argument error with the message in sdv_last_error()) and leave every entry point, struct and byte of sdv_hip.h as it is;
 * sdv_abi_version() stays 12.  The Python binding keeps them in a table of their own (hip.EXTENSION_SYMBOLS).
 */
#ifndef SDV_HIP_EXT_H
#define SDV_HIP_EXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------------------------
 * H.264 motion search: motion-compensated P pictures for the GOP path of sdv_hip.h ("H.264 P pictures"), with vectors that are whole
 * samples in luma AND chroma.  Opt-in on top of gop > 1 (h264_cavlc.H264Encoder(search=...), video.py: h264_search, SDV_H264_SEARCH);
 * search 0, the default, runs sdv_h264_encode_gops and writes its bytes: no launch and no byte of any file changes.  Like qp 16 and
 * gop 1 the default and any other value are settings, not measured optima.
 *
 * Stream rule (an addition to "H.264 P pictures"; everything not named here is as there).  Setting search: an even integer 0 .. 16, the
 * largest |component| of a vector in luma samples.
 *   Vectors.  One vector v = (vx, vy) per macroblock of a P picture, every component a multiple of 2 luma samples (8 in quarter-sample
 *   units), |vx|, |vy| <= search.  The luma prediction is the copy of the reference displaced by (vx, vy), the chroma prediction the copy
 *   displaced by (vx / 2, vy / 2): no interpolation filter anywhere.  The displaced 16 x 16 block lies wholly inside the coded (padded)
 *   picture: candidates at the picture edge are clipped to that, a one-macroblock picture has only (0, 0).  (The bitstream would allow
 *   edge clamping; the encoder does not use it.)
 *   Search.  On SOURCE luma: picture k against source picture k - 1, not against the reconstruction - one launch over all P pictures of a
 *   call, independent of coding order; decoder-exactness is unaffected, because compensation and residual use the reconstruction.
 *   Exhaustive over the admitted candidates.  cost(v) = SAD(v) + lambda(qp) * (B(vx) + B(vy)), B(c) the length in bits of se(4 c) (the
 *   vector against a zero predictor, so the search does not depend on the left neighbour); lambda(qp) = max(1, round(2 ** ((qp - 12) /
 *   6))) as a 52-entry integer table (a setting).  The winner is the minimum under the total order (cost, |vx| + |vy|, vy, vx), the last
 *   two compared as signed integers - so a flat or repeated picture yields (0, 0) everywhere.
 *   Prediction of the vector.  The row above is another slice, so B, C and D are unavailable: mvp is the left neighbour's vector when
 *   the left neighbour is in the slice and inter (P_Skip counts, with (0, 0)), and (0, 0) when it is intra or I_PCM or when the macroblock
 *   is the first of its row.  mvd = 4 v - mvp in quarter samples, written se(mvd_x) se(mvd_y).  P_Skip always infers (0, 0).
 *   Mode.  Decided as in "H.264 P pictures" with the displaced reference: sad_inter = sum |src - rec[k - 1](x + vx, y + vy)|, intra iff
 *   sad_intra < sad_inter.  Inter residual, quantisation, cbp and nC exactly as there.  P_Skip requires cbp 0 AND v = (0, 0); cbp 0 with
 *   v != (0, 0) is P_L0_16x16 with coded_block_pattern codeNum 0 (and then no mb_qp_delta, 7.3.5).  The counting pass that triggers I_PCM
 *   above 3200 bits includes the mvd bits, so a coded macroblock still takes at most 3200 bits and the capacity derivation of sdv_hip.h
 *   (the slots of a picture mbw' = mbw + 1 + mbw / 64 macroblocks wide) holds unchanged.  Slice headers, frame_num, stss and parameter
 *   sets are unchanged; a vertical range of 16 is inside MaxVmvR of every level.
 *
 * sdv_h264_motion_search    y (16-byte aligned) as for sdv_h264_encode_gops; search even, 2 .. 16.  Writes mv: int16 [n][mbh][mbw][2]
 *   (vx, vy) in luma samples, zeros for the IDR pictures (k % gop == 0); sad (may be null): int32 [n][mbh][mbw], the winner's source
 *   SAD.  One launch, one wave per macroblock: the window of the previous source picture in LDS, lanes own candidates, one wave-wide
 *   minimum of the packed order.
 * sdv_h264_encode_gop_step  sdv_h264_encode_gops for ONE picture position k (0 .. min(gop, n) - 1) of every GOP of the call, with the
 *   vectors mv; the caller enqueues the positions in order on one stream, because row r of picture k reads rows r - 1 .. r + 1 of the
 *   reconstruction of picture k - 1 and the kernel boundary orders that.  The kernel does not trust mv: a vector that is odd, outside
 *   the range or leaves the picture is coded as (0, 0).  Planes, ry / rcb / rcr, scratch and its size as for sdv_h264_encode_gops; pack
 *   with sdv_h264_pack(scratch, n, mbh, mbw', ...).  One wave per (GOP, macroblock row). */
int sdv_h264_motion_search(const uint8_t* y, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t search, int16_t* mv,
                           int32_t* sad, void* stream);
int sdv_h264_encode_gop_step(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                             int32_t gop, int32_t k, int32_t search, int32_t first_index, const int16_t* mv, uint8_t* ry, uint8_t* rcb,
                             uint8_t* rcr, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDV_HIP_EXT_H */
