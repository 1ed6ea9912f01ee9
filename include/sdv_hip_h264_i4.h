/*
 * sdv_hip_h264_i4.h - Intra4x4 prediction for the IDR pictures of the H.264 track: one more additive entry point of ABI 12 of
 * libsdv_hip.so.  It is exported by the same library as those of sdv_hip.h, sdv_hip_ext.h and sdv_hip_h264_sub.h, follows their
 * conventions (device pointers, `stream` a hipStream_t passed as void*, enqueue only, 0 = ok, negative = argument error with the message
 * in sdv_last_error()) and leaves every entry point, struct and byte of those three headers as it is; sdv_abi_version() stays 12.  The
 * Python binding keeps it in a table of its own (hip.H264_I4_SYMBOLS).
 */
#ifndef SDV_HIP_H264_I4_H
#define SDV_HIP_H264_I4_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------------------------
 * H.264 Intra4x4: every IDR picture of a call chooses per macroblock between I_NxN (Intra4x4, nine modes) and the Intra16x16 DC
 * macroblock of "H.264 CAVLC intra encoder", with I_PCM by that section's two triggers.  Opt-in (h264_cavlc.H264Encoder(intra4=1),
 * video.py: h264_intra4, SDV_H264_INTRA4); intra4 0, the default, runs the launches of the other headers and writes their bytes.  P
 * pictures are untouched: intra macroblocks inside P slices stay Intra16x16 DC, and no P-slice syntax depends on the IDR picture's
 * macroblock types.  A setting, not a measured optimum.  The stream has met no third-party decoder yet; tests/h264_i4_ref.py restates
 * and decodes it.
 *
 * Stream rule (everything not named here is as in "H.264 CAVLC intra encoder" and "H.264 P pictures").
 *   Slices, slice headers, parameter sets, idr_pic_id, stss and deblocking off are unchanged.  The row above is another slice, so "top"
 *   is never available for a macroblock's top edge.
 *   Availability for 4x4 block (bx, by) of macroblock m in its row:  top iff by >= 1;  left iff bx >= 1 or m > 0;  corner p[-1,-1] iff
 *   top and left;  top-right iff by >= 1 and bx <= 2 and (bx, by) not in {(1,1), (1,3)}, otherwise p[4..7,-1] = p[3,-1] (8.3.1.2).
 *   Modes.  V(0), DDL(3), VL(7) need top; H(1), HU(8) need left; DDR(4), VR(5), HD(6) need top, left and corner; DC(2) is always
 *   allowed.
 *   Predictors (8.3.1.2.1 - 8.3.1.2.9).  p[x,-1] the top row (x = 0 .. 7), p[-1,y] the left column, p[-1,-1] also p[-1,y] at y = -1
 *   and p[x,-1] at x = -1.
 *     V    p[x,-1].            H    p[-1,y].
 *     DC   (sum top + sum left + 4) >> 3 with both, (sum + 2) >> 2 with one, 128 with none.
 *     DDL  x = y = 3: (p[6,-1] + 3 p[7,-1] + 2) >> 2;  else (p[x+y,-1] + 2 p[x+y+1,-1] + p[x+y+2,-1] + 2) >> 2.
 *     DDR  x > y: (p[x-y-2,-1] + 2 p[x-y-1,-1] + p[x-y,-1] + 2) >> 2;  x < y: (p[-1,y-x-2] + 2 p[-1,y-x-1] + p[-1,y-x] + 2) >> 2;
 *          x = y: (p[0,-1] + 2 p[-1,-1] + p[-1,0] + 2) >> 2.
 *     VR   z = 2x - y, i = x - (y >> 1).  z even >= 0: (p[i-1,-1] + p[i,-1] + 1) >> 1;  z odd > 0: (p[i-2,-1] + 2 p[i-1,-1] + p[i,-1]
 *          + 2) >> 2;  z = -1: (p[-1,0] + 2 p[-1,-1] + p[0,-1] + 2) >> 2;  else (p[-1,y-1] + 2 p[-1,y-2] + p[-1,y-3] + 2) >> 2.
 *     HD   z = 2y - x, j = y - (x >> 1).  z even >= 0: (p[-1,j-1] + p[-1,j] + 1) >> 1;  z odd > 0: (p[-1,j-2] + 2 p[-1,j-1] + p[-1,j]
 *          + 2) >> 2;  z = -1: (p[-1,0] + 2 p[-1,-1] + p[0,-1] + 2) >> 2;  else (p[x-1,-1] + 2 p[x-2,-1] + p[x-3,-1] + 2) >> 2.
 *     VL   i = x + (y >> 1).  y even: (p[i,-1] + p[i+1,-1] + 1) >> 1;  y odd: (p[i,-1] + 2 p[i+1,-1] + p[i+2,-1] + 2) >> 2.
 *     HU   z = x + 2y, j = y + (x >> 1).  z in {0, 2, 4}: (p[-1,j] + p[-1,j+1] + 1) >> 1;  z in {1, 3}: (p[-1,j] + 2 p[-1,j+1] +
 *          p[-1,j+2] + 2) >> 2;  z = 5: (p[-1,2] + 3 p[-1,3] + 2) >> 2;  z > 5: p[-1,3].
 *   Syntax of I_NxN.  mb_type ue(0).  Per block in luma4x4BlkIdx order prev_intra4x4_pred_mode_flag u(1) and, if 0,
 *   rem_intra4x4_pred_mode u(3), rem = mode if mode < predicted else mode - 1; predicted = min(modeA, modeB), 2 when A or B is
 *   unavailable; a neighbour that is Intra16x16 or I_PCM counts as mode 2.  Then intra_chroma_pred_mode ue(0), then
 *   coded_block_pattern me(v) by the INTRA column of Table 9-4 (codeNum -> cbp: 47 31 15 0 23 27 29 30 7 11 13 14 39 43 45 46 16 3 5
 *   10 12 19 21 26 28 35 37 42 44 1 2 4 8 17 18 20 24 6 9 22 25 32 33 34 36 40 38 41), then mb_qp_delta se(0) only if cbp != 0, then the
 *   residual: for each 8x8 whose cbp bit is set its four blocks as 16-coefficient residual_blocks; chroma as today.  There is no luma DC
 *   transform.  Luma quantisation uses the intra dead zone f = (1 << qbits) / 3.  The cbp luma bit is set iff any level of the 8x8 is
 *   nonzero.  nC uses the 16-coefficient TotalCoeff, 0 in an uncoded 8x8; an Intra16x16 neighbour gives its AC TotalCoeff and I_PCM
 *   gives 16, as today.
 *   Decision.  Blocks are visited in blkIdx order, each predicted from the RECONSTRUCTION of its neighbours.  Block cost = SAD(src,
 *   pred) + lambda(qp) * (1 if mode == predicted else 4), with the motion search's lambda table; the winner is the minimum of (cost,
 *   mode).  The macroblock is I_NxN iff the sum of its block costs < sum |src - DC16| (strict), DC16 the macroblock's own DC: the
 *   rounded mean (sum + 128) >> 8 of its 256 source luma samples (what the left column mispredicts of it is one Intra16x16 DC level),
 *   so a flat macroblock stays Intra16x16, with or without a left neighbour.  Then the counting pass runs: the macroblock is I_PCM
 *   above 3200 bits or on level_prefix > 15; the reconstruction is then the source, and the modes handed to the right neighbour count
 *   as 2.  Chroma is unchanged.
 *   Capacity.  A coded macroblock is still <= 3200 bits.  The kernel always uses the GOP slot geometry (mbw' = mbw + 1 + mbw / 64,
 *   h264_gop_scratch_bytes / h264_gop_out_bytes; sdv_hip.h "Capacity of the GOP path"), also at gop 1, and the writer guards every
 *   store.
 *
 * sdv_h264_encode_idr4  planes as for sdv_h264_encode_gops.  Codes the pictures at positions k % gop == 0 of the call (all pictures at
 *   gop 1): their slices into the GOP slots of `scratch` (pack with sdv_h264_pack and mbw'), ALL their reconstructed samples into
 *   ry / rcb / rcr.  The other pictures' slots and planes are not touched: the caller then enqueues, for k = 1 .. min(gop, n) - 1 in
 *   order on the same stream, sdv_h264_encode_gop_step or sdv_h264_encode_gop_step_sub.  One wave per (IDR picture, macroblock row);
 *   inside a macroblock the sixteen blocks are a serial chain, each block's (mode, row) candidates spread over 36 lanes. */
int sdv_h264_encode_idr4(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop,
                         int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDV_HIP_H264_I4_H */
