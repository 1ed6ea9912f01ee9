/*
 * sdv_hip_h264_seg.h - several slices per macroblock row of the H.264 track: four more additive entry points of ABI 12 of libsdv_hip.so.
 * They are exported by the same library as those of sdv_hip.h, sdv_hip_ext.h, sdv_hip_h264_sub.h, sdv_hip_h264_i4.h, sdv_hip_h264_lf.h and
 * sdv_hip_h264_part.h, follow their conventions (device pointers, `stream` a hipStream_t passed as void*, enqueue only, 0 = ok, negative =
 * argument error with the message in sdv_last_error()) and leave every entry point, struct and byte of those six headers as it is;
 * sdv_abi_version() stays 12.  The Python binding keeps them in a table of its own (hip.H264_SEG_SYMBOLS).
 */
#ifndef SDV_HIP_H264_SEG_H
#define SDV_HIP_H264_SEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------------------------
 * H.264 row slices: every macroblock row of every picture is cut into up to S slices of nearly equal width, each an independent
 * byte-aligned bit stream with a wave of its own on the GPU.  The other headers code one slice per macroblock row, so their unit of
 * parallelism is the chain (GOP, row); here it is (GOP, row, slice).  Opt-in (h264_cavlc.H264Encoder(row_slices=S), video.py:
 * h264_row_slices, SDV_H264_ROW_SLICES); S is an integer 1 .. 16 and is valid with every gop (1 included), search, subpel, intra4,
 * deblock and part.  A setting, not a measured optimum.  The stream has met no third-party decoder yet; tests/h264_seg_ref.py restates and
 * decodes it.  The gain on a real walk is unmeasured.
 *
 * The number of slices actually written per row is   segs = max(1, min(S, mbw, 1024 / mbh))   (integer division).  It depends on the
 * frame size only, so the file does not depend on the upload batch.  The last term exists because sdv_h264_pack is reused as it is and
 * accepts at most 1024 slot rows a picture.  segs = 1 (S = 1, a picture one macroblock wide, a very tall one) is the route and the
 * bytes of the other headers.
 *
 * Stream rule (everything not named here is as in the other six headers).
 *   Geometry.  Slice s (0 .. segs - 1) of row r covers macroblocks m0 = s mbw / segs .. m1 = (s + 1) mbw / segs - 1 (integer division):
 *   the widths differ by at most one and none is empty.  first_mb_in_slice = r mbw + m0.  The slices of a picture stand in the sample in
 *   increasing first_mb_in_slice order (no arbitrary slice order), each behind its 4-byte length: one mp4 sample is mbh segs slices.
 *   frame_num, idr_pic_id, slice_qp_delta, the deblocking bits, the NAL header bytes, stss and the parameter sets are unchanged.
 *   A slice start is a row start.  The macroblock at m0 has no neighbour A (it lies in another slice) and no B, C, D as before; exactly
 *   the state of the first macroblock of a row applies.  Intra16x16 DC and chroma DC predict 128.  nC is 0.  mvp of partition 0, or of
 *   the one vector, is (0, 0); partition 2 takes the median with A = (0, 0) / refIdx -1.  P_Skip infers (0, 0).  mb_skip_run counts from
 *   zero, and a trailing run is written at the slice's end.  In I_NxN the four left blocks have no left samples and
 *   predIntra4x4PredMode is 2 for them; block 0 admits DC (128) only.  Intra inside a P slice does not read the left slice's
 *   reconstruction.
 *   What does not stop at a slice start.  Motion vectors: a prediction may read any part of the previous picture's reconstruction (the
 *   admission rule is the picture's, not the slice's).  The loop filter: with disable_deblocking_filter_idc 0 the left macroblock edge at
 *   m0 is filtered across the slice boundary with the usual bS, from both macroblocks' modes, coefficients and vectors, as the top edge
 *   of every row already is.  The search: it runs on source pictures and knows nothing of slices.
 *   Capacity.  A slice of w <= W = ceil(mbw / segs) macroblocks is bounded by the GOP path's derivation (sdv_hip.h "Capacity of the GOP
 *   path"): first_mb_in_slice = r mbw + m0 < 1024 * 1024 = 2^20 still takes at most 41 bits, so the header is at most 72 bits; an
 *   mb_skip_run is at most w <= 1008 and takes at most 21 bits; a coded macroblock at most 3200 bits or I_PCM.  So a slice takes at most
 *   604.5 w + 25 bytes, and its slot is 600 w' + 17 bytes with w' = W + 1 + W / 64 (h264_gop_slot_mbw(W)), which is above that for
 *   every W >= 1.  In numbers: mbw 128, segs 8: W 16, w' 17, slot 10217 bytes >= 604.5 * 16 + 25 = 9697; mbw 5, segs 2: W 3, w' 4, slot
 *   2417 >= 1838.5; mbw 3, segs 3: W 1, w' 2, slot 1217 >= 629.5; mbw 1008, segs 16: W 63, w' 64, slot 38417 >= 38108.5.  Scratch and
 *   output are those of the intra layout at (n, mbh segs, w'); the slot index of slice s of row r of picture f is (f mbh + r) segs + s;
 *   sdv_h264_pack(scratch, n, mbh segs, w', ...) packs them unchanged.  The writer checks every store against its slot whatever the
 *   input.
 *
 * One vector layout serves every route: mv int16 [n][mbh][mbw][4][2] in QUARTER samples as in sdv_hip_h264_part.h, validated per vector
 * (a vector off the subpel grid, out of range or not admitted is coded as (0, 0)).  A caller with one vector a macroblock writes it four
 * times, scaled to quarter samples; four equal vectors are coded as P_L0_16x16 / P_Skip by the partition rule.  mbinfo and the filter
 * between two positions are those of sdv_hip_h264_part.h (sdv_h264_deblock_part, unchanged: it never knew of slices).
 *
 * Every entry point refuses, without a launch: what its counterpart without `segs` refuses; segs outside 1 .. min(mbw, 16);
 * mbh segs > 1024; a scratch below the seg layout at (n, mbh, mbw, segs).
 *
 * sdv_h264_encode_gop_step_seg, sdv_h264_encode_gop_step_seg_lf  as sdv_h264_encode_gop_step_part and _part_lf with one wave per (GOP,
 *   macroblock row, slice): a grid of ngops mbh segs workgroups of 64 lanes, the macroblock loop m0 .. m1, the writer, the chain, the
 *   vector chain and the skip run initialised at m0 as at the start of a row.  k = 0 codes IDR pictures (Intra16x16 DC), so the same
 *   entry point serves gop 1.  Source, reconstruction, mv and mbinfo are addressed per picture.  With segs = 1 the bytes and planes are
 *   those of sdv_h264_encode_gop_step_part(_lf).
 * sdv_h264_encode_idr4_seg, sdv_h264_encode_idr4_seg_lf  as sdv_h264_encode_idr4 and _idr4_lf, cut the same way.  With segs = 1 the bytes
 *   and planes are those of sdv_h264_encode_idr4(_lf). */
int sdv_h264_encode_gop_step_seg(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                 int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv, int64_t mv_count,
                                 uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, int32_t segs, void* stream);
int sdv_h264_encode_gop_step_seg_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                    int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                    int64_t mv_count, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                    uint32_t* mbinfo, int64_t mbinfo_count, int32_t segs, void* stream);
int sdv_h264_encode_idr4_seg(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop,
                             int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, int32_t segs,
                             void* stream);
int sdv_h264_encode_idr4_seg_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                int32_t gop, int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                uint32_t* mbinfo, int64_t mbinfo_count, int32_t segs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDV_HIP_H264_SEG_H */
