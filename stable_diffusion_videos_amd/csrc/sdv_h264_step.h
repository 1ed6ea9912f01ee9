// The three per-position encode kernels of the H.264 track and their launch functions, shared by sdv_h264.hip (kLf false: the entry
// points of sdv_hip_ext.h, sdv_hip_h264_sub.h and sdv_hip_h264_i4.h) and sdv_h264_lf.hip (kLf true: their _lf forms of sdv_hip_h264_lf.h,
// "H.264 deblocking").  Each file instantiates ONE of the two forms, so each kernel is compiled in a unit where its pieces have the call
// sites they had before the second form existed: with both forms in one unit the inliner leaves the pieces of sdv_h264_core.h as calls
// (scratch 144 -> 304 bytes a lane in h264_idr4_kernel).  Include after sdv_common.h and sdv_h264_core.h.
#pragma once

namespace {

SDV_DEVICE int h264_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// h264_gops_kernel's body for ONE picture position k of every GOP, with the vectors of the search: one wave per (GOP, macroblock row).
// The host enqueues positions 0 .. min(gop, n) - 1 in order: with a vertical component row r of picture f reads rows r - 1 .. r + 1 of
// the reconstruction of picture f - 1, which other waves wrote, and the kernel boundary orders that.  The reference samples come from
// the displaced position (2-byte alignment in luma, 1-byte in chroma); a vector of ``mv`` that the stream rule does not admit is coded
// as (0, 0) (h264_mv_fetch).
//
// kLf ("H.264 deblocking", sdv_hip_h264_lf.h): the slice headers switch the loop filter on and lane 0 stores the macroblock's side
// information word (h264_lf_word) into mbinfo; kLf false is the kernel as it was and never reads the pointer.
template <bool kLf>
__global__ __launch_bounds__(64) void h264_gop_step_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr,
                                                           int n, int mbh, int mbw, int qp, int gop, int k, int search, int first_index,
                                                           const int16_t* __restrict__ mv, uint8_t* ry, uint8_t* rcb, uint8_t* rcr,
                                                           uint8_t* __restrict__ slots, long long stride, long long slot_bytes,
                                                           int32_t* __restrict__ lens, uint32_t* __restrict__ mbinfo) {
    __shared__ h264_gop_mb mb;
    const int lane = threadIdx.x;
    const int r = (int)(blockIdx.x % mbh);
    const long long f = (long long)(blockIdx.x / mbh) * gop + k;
    if (f >= n) return;
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    const bool p = k > 0;
    const long long row = f * mbh + r;
    uint8_t* slot = slots + row * stride;
    h264_writer w;
    h264_chain ch;
    h264_mv_chain mvc;
    int skip_run = 0;
    w.init(slot + 5, slot_bytes - 5);
    ch.have = 0;
    mvc.vx = mvc.vy = 0;
    if (lane == 0) {
        if (p) h264_p_slice_header(w, (unsigned)(r * mbw), (unsigned)k, qp, kLf ? 1 : 0);
        else h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp, kLf ? 1 : 0);
    }
    const long long yat = row * 16 * lw, cat = row * 8 * cw;                       // this row in picture f
    const long long ypic = (f - 1) * mbh * 16 * lw, cpic = (f - 1) * mbh * 8 * cw;  // picture f - 1 (read in P pictures only)
    for (int m = 0; m < mbw; ++m) {
        h264_mv_ref at;
        at.vx = at.vy = 0;
        if (p) {
            const int16_t* v = mv + (row * mbw + m) * 2;
            at = h264_mv_fetch(v[0], v[1], search, m, r, mbw, mbh);
            for (int i = lane; i < 128; i += 64) {      // luma: 16 rows of 8 sample pairs
                const int a = i >> 3, b = 2 * (i & 7);
                *(uint16_t*)(mb.fy + a * 16 + b) = *(const uint16_t*)(ry + ypic + at.yoff + a * lw + b);
            }
            for (int i = lane; i < 128; i += 64) {      // chroma: 2 x 8 rows of 8 samples
                const int c = i >> 6, a = (i >> 3) & 7, b = i & 7;
                mb.fc[c * 64 + a * 8 + b] = (c ? rcr : rcb)[cpic + at.coff + a * cw + b];
            }
        }
        if (lane < 16) {
            *(uint4*)(mb.sy + lane * 16) = *(const uint4*)(y + yat + lane * lw + m * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)(mb.sc + c * 64 + i * 8) = *(const uint2*)((c ? cr : cb) + cat + i * cw + m * 8);
        }
        if (lane == 0) h264_gop_pred(&mb, ch);
        __syncthreads();
        bool inter = false;
        if (p) {
            int si = 0, sp = 0;
            if (lane < 16) h264_gop_block_sad(&mb, lane, &si, &sp);
            si = h264_wave_sum(si), sp = h264_wave_sum(sp);
            inter = !(si < sp);
        }
        const bool mine = lane < 24 && h264_gop_block_forward(&mb, lane, inter, qp);
        const unsigned nz = (unsigned)__ballot(mine);
        __syncthreads();
        if (lane == 0) {
            const bool any_cdc = h264_gop_dc(&mb, inter, qp);
            h264_gop_serial_mv(&mb, nz, any_cdc, inter, p, ch, mvc, at.vx, at.vy, w, &skip_run);
            if constexpr (kLf) mbinfo[row * mbw + m] = h264_lf_word(mb.mode, nz, at.vx, at.vy);
        }
        __syncthreads();
        if (lane < 24) h264_gop_block_recon(&mb, lane, qp);
        __syncthreads();
        if (lane < 16) {
            *(uint4*)(ry + yat + lane * lw + m * 16) = *(const uint4*)(mb.ry + lane * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)((c ? rcr : rcb) + cat + i * cw + m * 8) = *(const uint2*)(mb.rc + c * 64 + i * 8);
        }
        if (lane == 0) h264_gop_chain(&mb, ch);
        __syncthreads();
    }
    if (lane == 0) {
        if (p && skip_run) h264_put_ue(w, (unsigned)skip_run);                     // the slice ends in skipped macroblocks
        w.put(1u, 1);                                   // rbsp_slice_trailing_bits
        while (w.n) w.put(0u, 1);
        const long long used = min(w.pos, slot_bytes - 5);      // (the capacity bound keeps pos below it; nothing was stored beyond)
        const unsigned len = (unsigned)(1 + used);
        slot[0] = (uint8_t)(len >> 24), slot[1] = (uint8_t)(len >> 16), slot[2] = (uint8_t)(len >> 8), slot[3] = (uint8_t)len;
        slot[4] = p ? 0x41 : 0x65;                      // nal_ref_idc 2, nal_unit_type 1 | nal_ref_idc 3, nal_unit_type 5
        lens[row] = (int32_t)(5 + used);
    }
}

// h264_gop_step_kernel with quarter-sample vectors: for a P macroblock the 21 x 21 luma window and the two 9 x 9 chroma windows of the
// reference RECONSTRUCTION are staged in LDS with clamped coordinates (no read leaves a plane, whatever the vector), then every lane
// interpolates 4 luma and 2 chroma samples of mb.fy / mb.fc.  Whole-sample vectors take the same path: fraction 0 is a copy.  A vector of
// ``mv`` that is off the subpel grid, out of range or not admitted is coded as (0, 0) (h264_sub_fetch).  Everything after the prediction
// is h264_gop_step_kernel's code with the vector and the chain in quarter samples.
// kLf: as in h264_gop_step_kernel.
template <bool kLf>
__global__ __launch_bounds__(64) void h264_gop_step_sub_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb,
                                                               const uint8_t* __restrict__ cr, int n, int mbh, int mbw, int qp, int gop, int k,
                                                               int search, int subpel, int first_index, const int16_t* __restrict__ mv, uint8_t* ry,
                                                               uint8_t* rcb, uint8_t* rcr, uint8_t* __restrict__ slots, long long stride,
                                                               long long slot_bytes, int32_t* __restrict__ lens, uint32_t* __restrict__ mbinfo) {
    constexpr int kLuma = kH264SubLumaWin * kH264SubLumaWin, kChroma = kH264SubChromaWin * kH264SubChromaWin;
    __shared__ h264_gop_mb mb;
    __shared__ uint8_t wy[kLuma];
    __shared__ uint8_t wc[2 * kChroma];
    const int lane = threadIdx.x;
    const int r = (int)(blockIdx.x % mbh);
    const long long f = (long long)(blockIdx.x / mbh) * gop + k;
    if (f >= n) return;
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    const bool p = k > 0;
    const long long row = f * mbh + r;
    uint8_t* slot = slots + row * stride;
    h264_writer w;
    h264_chain ch;
    h264_mv_chain mvc;
    int skip_run = 0;
    w.init(slot + 5, slot_bytes - 5);
    ch.have = 0;
    mvc.vx = mvc.vy = 0;
    if (lane == 0) {
        if (p) h264_p_slice_header(w, (unsigned)(r * mbw), (unsigned)k, qp, kLf ? 1 : 0);
        else h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp, kLf ? 1 : 0);
    }
    const long long yat = row * 16 * lw, cat = row * 8 * cw;                       // this row in picture f
    const long long ypic = (f - 1) * mbh * 16 * lw, cpic = (f - 1) * mbh * 8 * cw;  // picture f - 1 (read in P pictures only)
    for (int m = 0; m < mbw; ++m) {
        h264_sub_ref at = h264_sub_fetch(0, 0, search, subpel, m, r, mbw, mbh);
        if (p) {
            const int16_t* v = mv + (row * mbw + m) * 2;
            at = h264_sub_fetch(v[0], v[1], search, subpel, m, r, mbw, mbh);
            for (int i = lane; i < kLuma; i += 64) wy[i] = ry[ypic + h264_sub_luma_at(at, i, m, r, mbw, mbh)];
            for (int i = lane; i < 2 * kChroma; i += 64)
                wc[i] = (i < kChroma ? rcb : rcr)[cpic + h264_sub_chroma_at(at, i % kChroma, m, r, mbw, mbh)];
            __syncthreads();
            {
                const int a = lane >> 2, b = 4 * (lane & 3);                       // luma: 4 samples of row a
#pragma unroll
                for (int e = 0; e < 4; ++e) mb.fy[a * 16 + b + e] = (uint8_t)h264_sub_pred_luma(wy, at, b + e, a);
                const int c = lane >> 5, ca = (lane >> 2) & 7, cb2 = 2 * (lane & 3);   // chroma: 2 samples of row ca of component c
#pragma unroll
                for (int e = 0; e < 2; ++e) mb.fc[c * 64 + ca * 8 + cb2 + e] = (uint8_t)h264_sub_pred_chroma(wc + c * kChroma, at, cb2 + e, ca);
            }
        }
        if (lane < 16) {
            *(uint4*)(mb.sy + lane * 16) = *(const uint4*)(y + yat + lane * lw + m * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)(mb.sc + c * 64 + i * 8) = *(const uint2*)((c ? cr : cb) + cat + i * cw + m * 8);
        }
        if (lane == 0) h264_gop_pred(&mb, ch);
        __syncthreads();
        bool inter = false;
        if (p) {
            int si = 0, sp = 0;
            if (lane < 16) h264_gop_block_sad(&mb, lane, &si, &sp);
            si = h264_wave_sum(si), sp = h264_wave_sum(sp);
            inter = !(si < sp);
        }
        const bool mine = lane < 24 && h264_gop_block_forward(&mb, lane, inter, qp);
        const unsigned nz = (unsigned)__ballot(mine);
        __syncthreads();
        if (lane == 0) {
            const bool any_cdc = h264_gop_dc(&mb, inter, qp);
            h264_gop_serial_sub(&mb, nz, any_cdc, inter, p, ch, mvc, at.vx, at.vy, w, &skip_run);
            if constexpr (kLf) mbinfo[row * mbw + m] = h264_lf_word(mb.mode, nz, at.vx, at.vy);
        }
        __syncthreads();
        if (lane < 24) h264_gop_block_recon(&mb, lane, qp);
        __syncthreads();
        if (lane < 16) {
            *(uint4*)(ry + yat + lane * lw + m * 16) = *(const uint4*)(mb.ry + lane * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)((c ? rcr : rcb) + cat + i * cw + m * 8) = *(const uint2*)(mb.rc + c * 64 + i * 8);
        }
        if (lane == 0) h264_gop_chain(&mb, ch);
        __syncthreads();
    }
    if (lane == 0) {
        if (p && skip_run) h264_put_ue(w, (unsigned)skip_run);                     // the slice ends in skipped macroblocks
        w.put(1u, 1);                                   // rbsp_slice_trailing_bits
        while (w.n) w.put(0u, 1);
        const long long used = min(w.pos, slot_bytes - 5);      // (the capacity bound keeps pos below it; nothing was stored beyond)
        const unsigned len = (unsigned)(1 + used);
        slot[0] = (uint8_t)(len >> 24), slot[1] = (uint8_t)(len >> 16), slot[2] = (uint8_t)(len >> 8), slot[3] = (uint8_t)len;
        slot[4] = p ? 0x41 : 0x65;                      // nal_ref_idc 2, nal_unit_type 1 | nal_ref_idc 3, nal_unit_type 5
        lens[row] = (int32_t)(5 + used);
    }
}

// Intra4x4 IDR pictures (sdv_hip_h264_i4.h "H.264 Intra4x4"): one wave per (IDR picture, macroblock row) on h264_gop_step_kernel's
// skeleton - source staged in LDS, lane 0 keeps the serial coder, lanes 0 - 31 store the reconstruction.  The new part is the 16-step
// block loop: lane 0 has left the block's neighbour samples in LDS (from the LDS reconstruction and the chain's column); lane 4 m + r
// computes row r of mode m (36 lanes, 4 samples each, all through h264_i4_pred), a two-step shuffle sum gives every lane of a mode its
// SAD, one wave minimum of h264_i4_key picks the winner for all lanes alike; lane 0 transforms, quantises and reconstructs it into LDS
// and gathers the next block's neighbours; one barrier, in uniform control flow, ends the step.  Two waves per SIMD are asked for: left
// alone the compiler takes 256 VGPRs + 32 AGPRs (one wave per SIMD); held to 256 it needs 237 VGPRs and spills none.
// kLf: as in h264_gop_step_kernel (every macroblock of an IDR picture is intra: the word says so, and whether it is I_PCM).
template <bool kLf>
__global__ __launch_bounds__(64, 2) void h264_idr4_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr,
                                                       int n, int mbh, int mbw, int qp, int gop, int first_index, uint8_t* __restrict__ ry,
                                                       uint8_t* __restrict__ rcb, uint8_t* __restrict__ rcr, uint8_t* __restrict__ slots,
                                                       long long stride, long long slot_bytes, int32_t* __restrict__ lens,
                                                       uint32_t* __restrict__ mbinfo) {
    __shared__ h264_gop_mb mb;
    __shared__ h264_i4_mb i4;
    const int lane = threadIdx.x;
    const int r = (int)(blockIdx.x % mbh);
    const long long f = (long long)(blockIdx.x / mbh) * gop;
    if (f >= n) return;
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    const long long row = f * mbh + r;
    uint8_t* slot = slots + row * stride;
    h264_writer w;
    h264_i4_chain ch;
    w.init(slot + 5, slot_bytes - 5);
    ch.ch.have = 0;
    if (lane == 0) h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp, kLf ? 1 : 0);
    const long long yat = row * 16 * lw, cat = row * 8 * cw;
    const int lambda = h264_me_lambda(qp);
    const int cand_mode = lane >> 2, cand_row = lane & 3;
    for (int m = 0; m < mbw; ++m) {
        if (lane < 16) {
            *(uint4*)(mb.sy + lane * 16) = *(const uint4*)(y + yat + lane * lw + m * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)(mb.sc + c * 64 + i * 8) = *(const uint2*)((c ? cr : cb) + cat + i * cw + m * 8);
        }
        if (lane == 0) h264_i4_begin(&mb, &i4, ch);
        __syncthreads();
        const int dc16 = h264_i4_dc16(h264_wave_sum(lane < 16 ? h264_i4_block_sum(&mb, lane) : 0));
        const int sad16 = h264_wave_sum(lane < 16 ? h264_i4_block_sad16(&mb, lane, dc16) : 0);
        for (int b = 0; b < 16; ++b) {
            int bx, by;
            h264_gop_block_xy(b, &bx, &by);
            const int pm = h264_i4_pred_mode(&i4, bx >> 2, by >> 2);
            const bool ok = cand_mode < kH264I4Modes && h264_i4_mode_ok(cand_mode, i4.avail);
            int s = ok ? h264_i4_row_sad(&mb, &i4, b, cand_mode, cand_row) : 0;
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            unsigned key = ok ? h264_i4_key(s, lambda, cand_mode, pm) : 0xffffffffu;       // DC is always admitted, so there is a winner
#pragma unroll
            for (int o = 32; o; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o));
            if (lane == 0) h264_i4_block_code(&mb, &i4, b, key, qp);
            __syncthreads();
        }
        const bool use_i4 = i4.cost < sad16;
        const bool mine = lane < 24 && (lane >= 16 || !use_i4) && h264_gop_block_forward(&mb, lane, false, qp);
        const unsigned nz = (unsigned)__ballot(mine);
        __syncthreads();
        if (lane == 0) {
            const bool any_cdc = h264_gop_dc(&mb, false, qp);
            h264_i4_serial(&mb, &i4, use_i4, nz, any_cdc, ch, w);
            if constexpr (kLf) mbinfo[row * mbw + m] = h264_lf_word(mb.mode, 0u, 0, 0);
        }
        __syncthreads();
        if (lane < 24) h264_i4_block_recon(&mb, lane, qp);
        __syncthreads();
        if (lane < 16) {
            *(uint4*)(ry + yat + lane * lw + m * 16) = *(const uint4*)(mb.ry + lane * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)((c ? rcr : rcb) + cat + i * cw + m * 8) = *(const uint2*)(mb.rc + c * 64 + i * 8);
        }
        if (lane == 0) h264_gop_chain(&mb, ch.ch);
        __syncthreads();
    }
    if (lane == 0) {
        w.put(1u, 1);                                   // rbsp_slice_trailing_bits
        while (w.n) w.put(0u, 1);
        const long long used = min(w.pos, slot_bytes - 5);      // (the capacity bound keeps pos below it; nothing was stored beyond)
        const unsigned len = (unsigned)(1 + used);
        slot[0] = (uint8_t)(len >> 24), slot[1] = (uint8_t)(len >> 16), slot[2] = (uint8_t)(len >> 8), slot[3] = (uint8_t)len;
        slot[4] = 0x65;                                 // nal_ref_idc 3, nal_unit_type 5
        lens[row] = (int32_t)(5 + used);
    }
}

struct h264_layout {
    long long rows, slot, stride, starts_at, lens_at, bytes;
};
h264_layout h264_scratch_layout(int n, int mbh, int mbw) {
    h264_layout l;
    l.rows = (long long)n * mbh;
    l.slot = 600LL * mbw + 17;                          // the capacity formula of sdv_hip.h
    l.stride = (l.slot + 7) & ~7LL;
    l.starts_at = l.rows * l.stride;
    l.lens_at = l.starts_at + 8 * l.rows;
    l.bytes = l.lens_at + 4 * l.rows;
    return l;
}

// The GOP path's slots are those of a picture this many macroblocks wide (sdv_hip.h "Capacity of the GOP path"), so that sdv_h264_pack
// reads them with the same layout.
int h264_gop_slot_mbw(int mbw) { return mbw + 1 + mbw / 64; }

}  // namespace

#define H264_GRID_ARGS(name)                                                                                                       \
    SDV_REQUIRE(n > 0 && n <= 65535, name ": bad frame count n=%d (1 .. 65535)", n);                                                \
    SDV_REQUIRE(mbh >= 1 && mbh <= 1024 && mbw >= 1 && mbw <= 1024, name ": bad macroblock grid mbh=%d mbw=%d (1 .. 1024)", mbh, mbw); \
    SDV_REQUIRE((long long)n * mbh < 0x7fffffffLL, name ": too many macroblock rows for one grid")

// The launch functions behind the entry points and their _lf forms (which have checked mbinfo; it is null and unused with kLf false).
template <bool kLf>
static int h264_encode_gop_step_impl(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                     int32_t gop, int32_t k, int32_t search, int32_t first_index, const int16_t* mv, uint8_t* ry, uint8_t* rcb,
                                     uint8_t* rcr, void* scratch, int64_t scratch_bytes, uint32_t* mbinfo, void* stream) {
    SDV_REQUIRE(y && cb && cr && mv && ry && rcb && rcr && scratch, "sdv_h264_encode_gop_step: null pointer");
    H264_GRID_ARGS("sdv_h264_encode_gop_step");
    SDV_REQUIRE(mbw <= 1008, "sdv_h264_encode_gop_step: mbw=%d above 1008 (its slots are those of a wider picture, which must stay within 1024)", mbw);
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_encode_gop_step: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_encode_gop_step: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(k >= 0 && k < gop && k < n, "sdv_h264_encode_gop_step: position k=%d outside 0 .. min(gop, n) - 1 (gop=%d, n=%d)", k, gop, n);
    SDV_REQUIRE(search >= 2 && search <= kH264SearchMax && search % 2 == 0, "sdv_h264_encode_gop_step: search=%d must be even, 2 .. %d", search,
                (int)kH264SearchMax);
    SDV_REQUIRE(first_index >= 0, "sdv_h264_encode_gop_step: negative first_index");
    const h264_layout l = h264_scratch_layout(n, mbh, h264_gop_slot_mbw(mbw));
    SDV_REQUIRE(scratch_bytes >= l.bytes, "sdv_h264_encode_gop_step: scratch buffer too small: %lld bytes, %lld slices of %d macroblocks need %lld",
                (long long)scratch_bytes, l.rows, mbw, l.bytes);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)cb) & 7) == 0 && (((uintptr_t)cr) & 7) == 0 && (((uintptr_t)scratch) & 7) == 0,
                "sdv_h264_encode_gop_step: y must be 16-byte, cb / cr / scratch 8-byte aligned");
    SDV_REQUIRE((((uintptr_t)ry) & 15) == 0 && (((uintptr_t)rcb) & 7) == 0 && (((uintptr_t)rcr) & 7) == 0 && (((uintptr_t)mv) & 3) == 0,
                "sdv_h264_encode_gop_step: ry must be 16-byte, rcb / rcr 8-byte, mv 4-byte aligned");
    uint8_t* base = (uint8_t*)scratch;
    const long long chains = (long long)((n - k + gop - 1) / gop) * mbh;           // the GOPs that have a picture at position k
    hipLaunchKernelGGL(h264_gop_step_kernel<kLf>, dim3((unsigned)chains), dim3(64), 0, (hipStream_t)stream, y, cb,
                       cr, n, mbh, mbw, qp, gop, k, search, first_index, mv, ry, rcb, rcr, base, l.stride, l.slot, (int32_t*)(base + l.lens_at), mbinfo);
    SDV_CHECK_LAUNCH("sdv_h264_encode_gop_step");
    return SDV_OK;
}
template <bool kLf>
static int h264_encode_gop_step_sub_impl(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                         int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv, uint8_t* ry,
                                         uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, uint32_t* mbinfo, void* stream) {
    SDV_REQUIRE(y && cb && cr && mv && ry && rcb && rcr && scratch, "sdv_h264_encode_gop_step_sub: null pointer");
    H264_GRID_ARGS("sdv_h264_encode_gop_step_sub");
    SDV_REQUIRE(mbw <= 1008, "sdv_h264_encode_gop_step_sub: mbw=%d above 1008 (its slots are those of a wider picture, which must stay within 1024)",
                mbw);
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_encode_gop_step_sub: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_encode_gop_step_sub: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(k >= 0 && k < gop && k < n, "sdv_h264_encode_gop_step_sub: position k=%d outside 0 .. min(gop, n) - 1 (gop=%d, n=%d)", k, gop, n);
    SDV_REQUIRE(search >= 2 && search <= kH264SearchMax && search % 2 == 0, "sdv_h264_encode_gop_step_sub: search=%d must be even, 2 .. %d", search,
                (int)kH264SearchMax);
    SDV_REQUIRE(h264_subpel_ok(subpel), "sdv_h264_encode_gop_step_sub: subpel=%d must be 1, 2 or 4", subpel);
    SDV_REQUIRE(first_index >= 0, "sdv_h264_encode_gop_step_sub: negative first_index");
    const h264_layout l = h264_scratch_layout(n, mbh, h264_gop_slot_mbw(mbw));
    SDV_REQUIRE(scratch_bytes >= l.bytes, "sdv_h264_encode_gop_step_sub: scratch buffer too small: %lld bytes, %lld slices of %d macroblocks need %lld",
                (long long)scratch_bytes, l.rows, mbw, l.bytes);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)cb) & 7) == 0 && (((uintptr_t)cr) & 7) == 0 && (((uintptr_t)scratch) & 7) == 0,
                "sdv_h264_encode_gop_step_sub: y must be 16-byte, cb / cr / scratch 8-byte aligned");
    SDV_REQUIRE((((uintptr_t)ry) & 15) == 0 && (((uintptr_t)rcb) & 7) == 0 && (((uintptr_t)rcr) & 7) == 0 && (((uintptr_t)mv) & 3) == 0,
                "sdv_h264_encode_gop_step_sub: ry must be 16-byte, rcb / rcr 8-byte, mv 4-byte aligned");
    uint8_t* base = (uint8_t*)scratch;
    const long long chains = (long long)((n - k + gop - 1) / gop) * mbh;           // the GOPs that have a picture at position k
    hipLaunchKernelGGL(h264_gop_step_sub_kernel<kLf>, dim3((unsigned)chains), dim3(64), 0, (hipStream_t)stream,
                       y, cb, cr, n, mbh, mbw, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, base, l.stride, l.slot,
                       (int32_t*)(base + l.lens_at), mbinfo);
    SDV_CHECK_LAUNCH("sdv_h264_encode_gop_step_sub");
    return SDV_OK;
}
template <bool kLf>
static int h264_encode_idr4_impl(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop,
                                 int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, uint32_t* mbinfo,
                                 void* stream) {
    SDV_REQUIRE(y && cb && cr && ry && rcb && rcr && scratch, "sdv_h264_encode_idr4: null pointer");
    H264_GRID_ARGS("sdv_h264_encode_idr4");
    SDV_REQUIRE(mbw <= 1008, "sdv_h264_encode_idr4: mbw=%d above 1008 (its slots are those of a wider picture, which must stay within 1024)", mbw);
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_encode_idr4: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_encode_idr4: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(first_index >= 0, "sdv_h264_encode_idr4: negative first_index");
    const h264_layout l = h264_scratch_layout(n, mbh, h264_gop_slot_mbw(mbw));
    SDV_REQUIRE(scratch_bytes >= l.bytes, "sdv_h264_encode_idr4: scratch buffer too small: %lld bytes, %lld slices of %d macroblocks need %lld",
                (long long)scratch_bytes, l.rows, mbw, l.bytes);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)cb) & 7) == 0 && (((uintptr_t)cr) & 7) == 0 && (((uintptr_t)scratch) & 7) == 0,
                "sdv_h264_encode_idr4: y must be 16-byte, cb / cr / scratch 8-byte aligned");
    SDV_REQUIRE((((uintptr_t)ry) & 15) == 0 && (((uintptr_t)rcb) & 7) == 0 && (((uintptr_t)rcr) & 7) == 0,
                "sdv_h264_encode_idr4: ry must be 16-byte, rcb / rcr 8-byte aligned");
    uint8_t* base = (uint8_t*)scratch;
    const long long chains = (long long)((n + gop - 1) / gop) * mbh;               // the IDR pictures of the call
    hipLaunchKernelGGL(h264_idr4_kernel<kLf>, dim3((unsigned)chains), dim3(64), 0, (hipStream_t)stream, y, cb, cr, n, mbh,
                       mbw, qp, gop, first_index, ry, rcb, rcr, base, l.stride, l.slot, (int32_t*)(base + l.lens_at), mbinfo);
    SDV_CHECK_LAUNCH("sdv_h264_encode_idr4");
    return SDV_OK;
}
