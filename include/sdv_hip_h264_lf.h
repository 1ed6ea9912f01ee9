/*
 * sdv_hip_h264_lf.h - the in-loop deblocking filter of the H.264 track: four more additive entry points of ABI 12 of libsdv_hip.so.  They
 * are exported by the same library as those of sdv_hip.h, sdv_hip_ext.h, sdv_hip_h264_sub.h and sdv_hip_h264_i4.h, follow their
 * conventions (device pointers, `stream` a hipStream_t passed as void*, enqueue only, 0 = ok, negative = argument error with the message
 * in sdv_last_error()) and leave every entry point, struct and byte of those four headers as it is; sdv_abi_version() stays 12.  The
 * Python binding keeps them in a table of its own (hip.H264_LF_SYMBOLS).
 */
#ifndef SDV_HIP_H264_LF_H
#define SDV_HIP_H264_LF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------------------------
 * H.264 deblocking: the normative loop filter (8.7) on the reconstruction planes, so that P pictures predict from filtered pictures and
 * a decoder shows filtered pictures.  Opt-in (h264_cavlc.H264Encoder(deblock=1), video.py: h264_deblock, SDV_H264_DEBLOCK); deblock 0,
 * the default, runs the launches of the other headers and writes their bytes.  Valid with every gop, search, subpel and intra4.  A
 * setting, not a measured optimum.  The stream and the three tables below have met no third-party decoder yet; tests/h264_lf_ref.py
 * restates, decodes and filters it.
 *
 * Stream rule (everything not named here is as in the other four headers).
 *   Slice headers.  disable_deblocking_filter_idc ue(0), slice_alpha_c0_offset_div2 se(0), slice_beta_offset_div2 se(0) in place of
 *   disable_deblocking_filter_idc ue(1): three bits either way, so every capacity bound holds unchanged.  Nothing else in the headers,
 *   the parameter sets (deblocking_filter_control_present_flag has been 1 from the start), stss or the macroblock layer changes.  Mode
 *   decisions, the motion search (it runs on source pictures) and the I_PCM triggers are untouched.  Intra prediction reads the
 *   UNFILTERED reconstruction (the chains in LDS), inter prediction the FILTERED reference picture, as 8.3 and 8.4 order.
 *   Filter.  8.7 for frame macroblocks, 4:2:0, transform_size_8x8_flag 0, filterOffsetA = filterOffsetB = 0, on the whole padded
 *   macroblock grid (the cropped-away border included, as in a decoder).  The left and the top picture edge are not filtered.  Slice
 *   boundaries ARE filtered (idc 0): the row above is another slice, and its samples, macroblock kinds and vectors take part in the top
 *   macroblock edge.
 *   Order.  Macroblocks in raster order.  Per macroblock: luma vertical edges (columns 0, 4, 8, 12) left to right, then luma horizontal
 *   edges (rows 0, 4, 8, 12) top to bottom, then the same for Cb and for Cr with the two chroma edges at 0 and 4.  Every edge sees what
 *   earlier edges and earlier macroblocks left.  Chroma edge c takes its bS from luma edge 2 c: chroma line l from luma lines 2 l, 2 l + 1.
 *   bS.  4 on a macroblock edge where either side is intra (I_NxN and I_PCM included); 3 on an inner edge of an intra macroblock; else 2
 *   where the 4x4 luma block on either side has a nonzero quantised coefficient; else 1 where the two sides' vectors differ by >= 4 in
 *   quarter-sample units in either component (there is one reference picture, so nothing else); else 0.  The vectors are even whole
 *   samples without subpel and quarter samples with it; both are brought to quarter units.  P_Skip here always has the vector (0, 0).
 *   Index.  qPp / qPq is 0 for an I_PCM macroblock and the slice qp otherwise (no nonzero mb_qp_delta is ever sent).  For chroma each
 *   side goes through the QPc table (chroma_qp_index_offset 0) first.  indexA = indexB = Clip3(0, 51, (qPp + qPq + 1) >> 1).
 *   Samples.  A line p3 p2 p1 p0 | q0 q1 q2 q3 is filtered when bS != 0 and |p0 - q0| < alpha and |p1 - p0| < beta and |q1 - q0| < beta.
 *     bS < 4: tc = tc0 + (ap < beta) + (aq < beta) in luma (ap = |p2 - p0|, aq = |q2 - q0|), tc0 + 1 in chroma; delta = Clip3(-tc, tc,
 *       (4 (q0 - p0) + (p1 - q1) + 4) >> 3); p0' = Clip1(p0 + delta), q0' = Clip1(q0 - delta); in luma also, where ap < beta,
 *       p1' = p1 + Clip3(-tc0, tc0, (p2 + ((p0 + q0 + 1) >> 1) - 2 p1) >> 1), and the same for q1 where aq < beta.
 *     bS 4, luma, where ap < beta and |p0 - q0| < (alpha >> 2) + 2: p0' = (p2 + 2 p1 + 2 p0 + 2 q0 + q1 + 4) >> 3, p1' = (p2 + p1 + p0 +
 *       q0 + 2) >> 2, p2' = (2 p3 + 3 p2 + p1 + p0 + q0 + 4) >> 3; otherwise, and always in chroma, p0' = (2 p1 + p0 + q1 + 2) >> 2.  The
 *       q side alike with aq.
 *   Tables, index 0 .. 51.
 *     alpha: sixteen 0, then 4 4 5 6 7 8 9 10 12 13 15 17 20 22 25 28 32 36 40 45 50 56 63 71 80 90 101 113 127 144 162 182 203 226 255 255.
 *     beta:  sixteen 0, then 2 2 2 3 3 3 3 4 4 4 6 6 7 7 8 8 9 9 10 10 11 11 12 12 13 13 14 14 15 15 16 16 17 17 18 18.
 *     tc0 (bS 1, 2, 3): 0 - 16 (0,0,0); 17 - 20 (0,0,1); 21 - 22 (0,1,1); 23 - 26 (1,1,1); 27 - 30 (1,1,2); 31 - 32 (1,2,3); 33 (2,2,3);
 *       34 (2,2,4); 35 - 36 (2,3,4); 37 (3,3,5); 38 - 39 (3,4,6); 40 (4,5,7); 41 (4,5,8); 42 (4,6,9); 43 (5,7,10); 44 (6,8,11); 45 (6,8,13);
 *       46 (7,10,14); 47 (8,11,16); 48 (9,12,18); 49 (10,13,20); 50 (11,15,23); 51 (13,17,25).
 *   Below index 16 alpha is 0 and no sample changes: at qp <= 15 the planes stay as they are (an I_PCM side only lowers the index).
 *
 * Side information.  mbinfo [n, mbh, mbw], one 32-bit word per macroblock, written by the _lf entry points and read by the filter:
 *   bits 0 .. 15  bit 4 by + bx is set when 4x4 luma block (bx, by) of an INTER macroblock kept a nonzero quantised coefficient (0 in
 *                 P_Skip and in every intra macroblock, where bS does not ask);
 *   bit 16        the macroblock is intra (Intra16x16, I_NxN or I_PCM);
 *   bit 17        the macroblock is I_PCM;
 *   bit 18        the coded vector is (0, 0) whatever `mv` holds (P_Skip, a zero vector, or a vector the stream rule did not admit);
 *   bits 19 .. 31 zero.
 *   The vector itself is read from the `mv` tensor of the motion search ([n, mbh, mbw, 2] int16).
 *
 * sdv_h264_encode_gop_step_lf, sdv_h264_encode_gop_step_sub_lf, sdv_h264_encode_idr4_lf
 *   sdv_h264_encode_gop_step, sdv_h264_encode_gop_step_sub and sdv_h264_encode_idr4 with two more arguments before `stream`: they write
 *   the slice headers above and the words of the macroblocks they code into mbinfo (mbinfo_count = n * mbh * mbw words, 4-byte aligned;
 *   lane 0 of the macroblock's wave, a plain vector store).  Everything else, bytes included, is the entry point without _lf.
 *
 * sdv_h264_deblock  filters ry / rcb / rcr of the pictures at position k of their GOPs (k = 0 .. min(gop, n) - 1) in place.  The caller
 *   enqueues it after the encode launch of position k and before that of k + 1, on the same stream, for every k: IDR pictures through
 *   sdv_h264_encode_idr4_lf or the k = 0 step of sdv_h264_encode_gop_step_lf.  `subpel` says what `mv` holds (0: even whole samples; 1,
 *   2, 4: quarter samples).  One workgroup per picture; its waves share out the macroblocks of one diagonal x + 2 y (they are
 *   independent, and every dependency of the standard's raster order lies on an earlier diagonal), one workgroup barrier between two
 *   diagonals; no wave waits on another workgroup.  `waves`: 0 = the default (as many as the longest diagonal has macroblocks, at most
 *   16), 1 .. 16 explicit; the result does not depend on it. */
int sdv_h264_encode_gop_step_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop,
                                int32_t k, int32_t search, int32_t first_index, const int16_t* mv, uint8_t* ry, uint8_t* rcb, uint8_t* rcr,
                                void* scratch, int64_t scratch_bytes, uint32_t* mbinfo, int64_t mbinfo_count, void* stream);
int sdv_h264_encode_gop_step_sub_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                    int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv, uint8_t* ry,
                                    uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, uint32_t* mbinfo, int64_t mbinfo_count,
                                    void* stream);
int sdv_h264_encode_idr4_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop,
                            int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, uint32_t* mbinfo,
                            int64_t mbinfo_count, void* stream);
int sdv_h264_deblock(uint8_t* ry, uint8_t* rcb, uint8_t* rcr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t k, int32_t subpel,
                     const uint32_t* mbinfo, int64_t mbinfo_count, const int16_t* mv, int32_t waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDV_HIP_H264_LF_H */
