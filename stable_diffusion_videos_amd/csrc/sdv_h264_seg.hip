// Row slices of the H.264 track (sdv_hip_h264_seg.h "H.264 row slices"): the four-vector per-position encode kernel of sdv_h264_part.hip and
// the Intra4x4 IDR kernel of sdv_h264_step.h, each with one wave per (GOP, macroblock row, slice) instead of one per (GOP, row).  Copies in a
// unit of their own: sdv_h264.hip, sdv_h264_lf.hip and sdv_h264_part.hip compile what they compiled before (the kernel templates of
// sdv_h264_step.h are not instantiated here; only its launch checks are used), and a row_slices 1 call runs their code.
#include "sdv_common.h"
#include "sdv_h264_core.h"
#include "sdv_hip_h264_seg.h"
#include "sdv_h264_step.h"

namespace {

// h264_gop_step_part_kernel (sdv_h264_part.hip) cut into slices: workgroup (g * mbh + r) * segs + s walks macroblocks m0 .. m1 of row r of
// picture g * gop + k.  The writer, the chain, the vector chain and the skip run start at m0 exactly as they start at m = 0 there, the
// header carries r * mbw + m0, and slot, length and ``lens`` use the slot index (f * mbh + r) * segs + s.  Source, reconstruction, ``mv``
// and ``mbinfo`` addressing stay per picture: a prediction may read any part of picture f - 1, which the previous launch finished.
// Slices of one row write disjoint macroblocks of picture f and read none of it but their own (the chain), so they are independent.
__global__ __launch_bounds__(64) void h264_gop_step_seg_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr,
                                                               int n, int mbh, int mbw, int qp, int gop, int k, int search, int subpel, int first_index,
                                                               const int16_t* __restrict__ mv, uint8_t* ry, uint8_t* rcb, uint8_t* rcr,
                                                               uint8_t* __restrict__ slots, long long stride, long long slot_bytes,
                                                               int32_t* __restrict__ lens, uint32_t* __restrict__ mbinfo, int segs) {
    constexpr int kLuma = kH264PartLumaWin * kH264PartLumaWin, kChroma = kH264PartChromaWin * kH264PartChromaWin;
    __shared__ h264_gop_mb mb;
    __shared__ uint8_t wy[4 * kLuma];
    __shared__ uint8_t wc[2 * 4 * kChroma];
    const int lane = threadIdx.x;
    const int s = (int)(blockIdx.x % segs);
    const int r = (int)(blockIdx.x / segs % mbh);
    const long long f = (long long)(blockIdx.x / segs / mbh) * gop + k;
    if (f >= n) return;
    const int m0 = h264_seg_first(s, mbw, segs), m1 = h264_seg_first(s + 1, mbw, segs);   // m0 .. m1 - 1
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    const bool p = k > 0;
    const int lf = mbinfo ? 1 : 0;
    const long long row = f * mbh + r;
    const long long at_slot = h264_seg_slot_index(f, r, s, mbh, segs);
    uint8_t* slot = slots + at_slot * stride;
    h264_writer w;
    h264_chain ch;
    h264_part_chain pc;
    int skip_run = 0;
    w.init(slot + 5, slot_bytes - 5);
    ch.have = 0;
    pc.v[0][0] = pc.v[0][1] = pc.v[1][0] = pc.v[1][1] = 0;
    if (lane == 0) {
        if (p) h264_p_slice_header(w, (unsigned)(r * mbw + m0), (unsigned)k, qp, lf);
        else h264_slice_header(w, (unsigned)(r * mbw + m0), (unsigned)((first_index + f) & 1), qp, lf);
    }
    const long long yat = row * 16 * lw, cat = row * 8 * cw;                       // this row in picture f
    const long long ypic = (f - 1) * mbh * 16 * lw, cpic = (f - 1) * mbh * 8 * cw;  // picture f - 1 (read in P pictures only)
    for (int m = m0; m < m1; ++m) {
        h264_sub_ref at[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) at[i] = h264_part_fetch(0, 0, search, subpel, m, r, mbw, mbh);
        if (p) {
            const int16_t* v = mv + (row * mbw + m) * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) at[i] = h264_part_fetch(v[2 * i], v[2 * i + 1], search, subpel, m, r, mbw, mbh);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                for (int j = lane; j < kLuma; j += 64) wy[i * kLuma + j] = ry[ypic + h264_part_luma_at(at[i], i, j, m, r, mbw, mbh)];
                if (lane < 2 * kChroma) {
                    const int c = lane >= kChroma ? 1 : 0, j = lane - c * kChroma;
                    wc[(c * 4 + i) * kChroma + j] = (c ? rcr : rcb)[cpic + h264_part_chroma_at(at[i], i, j, m, r, mbw, mbh)];
                }
            }
            __syncthreads();
            {
                const int a = lane >> 2, b = 4 * (lane & 3);                       // luma: 4 samples of row a, all in one partition
                const int part = 2 * (a >> 3) + (b >> 3);
                const h264_sub_ref la = part == 0 ? at[0] : part == 1 ? at[1] : part == 2 ? at[2] : at[3];
                const uint8_t* g = wy + part * kLuma + ((a & 7) + 2) * kH264PartLumaWin + (b & 7) + 2;
#pragma unroll
                for (int e = 0; e < 4; ++e) mb.fy[a * 16 + b + e] = (uint8_t)h264_sub_luma(g + e, kH264PartLumaWin, la.xf, la.yf);
                const int c = lane >> 5, ca = (lane >> 2) & 7, cb2 = 2 * (lane & 3);   // chroma: 2 samples of row ca of component c
                const int cpart = 2 * (ca >> 2) + (cb2 >> 2);
                const h264_sub_ref lc = cpart == 0 ? at[0] : cpart == 1 ? at[1] : cpart == 2 ? at[2] : at[3];
                const uint8_t* ga = wc + (c * 4 + cpart) * kChroma + (ca & 3) * kH264PartChromaWin + (cb2 & 3);
#pragma unroll
                for (int e = 0; e < 2; ++e) mb.fc[c * 64 + ca * 8 + cb2 + e] = (uint8_t)h264_sub_chroma(ga + e, kH264PartChromaWin, lc.cxf, lc.cyf);
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
            int v[4][2];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i][0] = at[i].vx, v[i][1] = at[i].vy;
            const bool any_cdc = h264_gop_dc(&mb, inter, qp);
            h264_gop_serial_part(&mb, nz, any_cdc, inter, p, ch, pc, v, w, &skip_run);
            if (mbinfo) mbinfo[row * mbw + m] = h264_part_lf_word(mb.mode, nz, v);
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
        lens[at_slot] = (int32_t)(5 + used);
    }
}

// h264_idr4_kernel (sdv_h264_step.h) cut the same way: workgroup (g * mbh + r) * segs + s, the Intra4x4 chain started at m0 (no left
// samples, no left modes, nC 0).  ``mbinfo`` null: the slice headers switch the loop filter off and nothing is stored; else they switch
// it on and lane 0 stores the macroblock's word.  Two waves per SIMD are asked for, as there.
__global__ __launch_bounds__(64, 2) void h264_idr4_seg_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr,
                                                              int n, int mbh, int mbw, int qp, int gop, int first_index, uint8_t* __restrict__ ry,
                                                              uint8_t* __restrict__ rcb, uint8_t* __restrict__ rcr, uint8_t* __restrict__ slots,
                                                              long long stride, long long slot_bytes, int32_t* __restrict__ lens,
                                                              uint32_t* __restrict__ mbinfo, int segs) {
    __shared__ h264_gop_mb mb;
    __shared__ h264_i4_mb i4;
    const int lane = threadIdx.x;
    const int s = (int)(blockIdx.x % segs);
    const int r = (int)(blockIdx.x / segs % mbh);
    const long long f = (long long)(blockIdx.x / segs / mbh) * gop;
    if (f >= n) return;
    const int m0 = h264_seg_first(s, mbw, segs), m1 = h264_seg_first(s + 1, mbw, segs);   // m0 .. m1 - 1
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    const long long row = f * mbh + r;
    const long long at_slot = h264_seg_slot_index(f, r, s, mbh, segs);
    uint8_t* slot = slots + at_slot * stride;
    h264_writer w;
    h264_i4_chain ch;
    w.init(slot + 5, slot_bytes - 5);
    ch.ch.have = 0;
    if (lane == 0) h264_slice_header(w, (unsigned)(r * mbw + m0), (unsigned)((first_index + f) & 1), qp, mbinfo ? 1 : 0);
    const long long yat = row * 16 * lw, cat = row * 8 * cw;
    const int lambda = h264_me_lambda(qp);
    const int cand_mode = lane >> 2, cand_row = lane & 3;
    for (int m = m0; m < m1; ++m) {
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
            int sd = ok ? h264_i4_row_sad(&mb, &i4, b, cand_mode, cand_row) : 0;
            sd += __shfl_xor(sd, 1);
            sd += __shfl_xor(sd, 2);
            unsigned key = ok ? h264_i4_key(sd, lambda, cand_mode, pm) : 0xffffffffu;      // DC is always admitted, so there is a winner
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
            if (mbinfo) mbinfo[row * mbw + m] = h264_lf_word(mb.mode, 0u, 0, 0);
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
        lens[at_slot] = (int32_t)(5 + used);
    }
}

}  // namespace

#define H264_SEG_MBINFO_ARGS(name)                                                                                                       \
    SDV_REQUIRE(mbinfo, name ": null pointer");                                                                                          \
    SDV_REQUIRE((((uintptr_t)mbinfo) & 3) == 0, name ": mbinfo must be 4-byte aligned");                                                \
    SDV_REQUIRE(n > 0 && mbh > 0 && mbw > 0 && mbinfo_count == (int64_t)n * mbh * mbw,                                                   \
                name ": mbinfo holds %lld words, %d pictures of %d x %d macroblocks have %lld", (long long)mbinfo_count, n, mbh, mbw,    \
                (long long)n * mbh * mbw)

// the checks the four entry points share; the grid (n mbh segs <= 65535 * 1024 workgroups) fits one launch
#define H264_SEG_COMMON_ARGS(name)                                                                                                       \
    SDV_REQUIRE(y && cb && cr && ry && rcb && rcr && scratch, "%s: null pointer", name);                                                 \
    SDV_REQUIRE(n > 0 && n <= 65535, "%s: bad frame count n=%d (1 .. 65535)", name, n);                                                   \
    SDV_REQUIRE(mbh >= 1 && mbh <= 1024 && mbw >= 1 && mbw <= 1024, "%s: bad macroblock grid mbh=%d mbw=%d (1 .. 1024)", name, mbh, mbw); \
    SDV_REQUIRE(mbw <= 1008, "%s: mbw=%d above 1008", name, mbw);                                                                         \
    SDV_REQUIRE(segs >= 1 && segs <= kH264SegMax && segs <= mbw, "%s: segs=%d outside 1 .. min(mbw, %d) = %d", name, segs,               \
                (int)kH264SegMax, mbw < (int)kH264SegMax ? mbw : (int)kH264SegMax);                                                       \
    SDV_REQUIRE((long long)mbh * segs <= kH264SegSlotRows, "%s: mbh * segs = %lld above %d slot rows a picture", name,                   \
                (long long)mbh * segs, (int)kH264SegSlotRows);                                                                            \
    SDV_REQUIRE((long long)n * mbh * segs < 0x7fffffffLL, "%s: too many slices for one grid", name);                                      \
    SDV_REQUIRE(qp >= 0 && qp <= 51, "%s: qp=%d outside 0 .. 51", name, qp);                                                              \
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "%s: gop=%d outside 1 .. %d", name, gop, (int)kH264GopMax);                              \
    SDV_REQUIRE(first_index >= 0, "%s: negative first_index", name);                                                                     \
    const h264_seg_layout l = h264_seg_scratch_layout(n, mbh, mbw, segs);                                                                \
    SDV_REQUIRE(scratch_bytes >= l.bytes, "%s: scratch buffer too small: %lld bytes, %lld slices of at most %d macroblocks need %lld",  \
                name, (long long)scratch_bytes, l.rows, h264_seg_width_max(mbw, segs), l.bytes);                                          \
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)cb) & 7) == 0 && (((uintptr_t)cr) & 7) == 0 && (((uintptr_t)scratch) & 7) == 0, \
                "%s: y must be 16-byte, cb / cr / scratch 8-byte aligned", name);                                                        \
    SDV_REQUIRE((((uintptr_t)ry) & 15) == 0 && (((uintptr_t)rcb) & 7) == 0 && (((uintptr_t)rcr) & 7) == 0,                               \
                "%s: ry must be 16-byte, rcb / rcr 8-byte aligned", name)

static int h264_encode_gop_step_seg_impl(const char* name, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw,
                                         int32_t qp, int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                         int64_t mv_count, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                         uint32_t* mbinfo, int32_t segs, void* stream) {
    H264_SEG_COMMON_ARGS(name);
    SDV_REQUIRE(mv, "%s: null pointer", name);
    SDV_REQUIRE((((uintptr_t)mv) & 3) == 0, "%s: mv must be 4-byte aligned", name);
    SDV_REQUIRE(mv_count == (int64_t)n * mbh * mbw * 8, "%s: mv holds %lld elements, %d pictures of %d x %d macroblocks with four vectors have %lld",
                name, (long long)mv_count, n, mbh, mbw, (long long)n * mbh * mbw * 8);
    SDV_REQUIRE(k >= 0 && k < gop && k < n, "%s: position k=%d outside 0 .. min(gop, n) - 1 (gop=%d, n=%d)", name, k, gop, n);
    SDV_REQUIRE(search >= 2 && search <= kH264SearchMax && search % 2 == 0, "%s: search=%d must be even, 2 .. %d", name, search, (int)kH264SearchMax);
    SDV_REQUIRE(h264_part_subpel_ok(subpel), "%s: subpel=%d must be 0, 1, 2 or 4", name, subpel);
    uint8_t* base = (uint8_t*)scratch;
    const long long chains = (long long)((n - k + gop - 1) / gop) * mbh * segs;    // the GOPs that have a picture at position k
    hipLaunchKernelGGL(h264_gop_step_seg_kernel, dim3((unsigned)chains), dim3(64), 0, (hipStream_t)stream, y, cb, cr, n, mbh, mbw, qp, gop, k, search,
                       subpel, first_index, mv, ry, rcb, rcr, base, l.stride, l.slot, (int32_t*)(base + l.lens_at), mbinfo, segs);
    SDV_CHECK_LAUNCH(name);
    return SDV_OK;
}

static int h264_encode_idr4_seg_impl(const char* name, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw,
                                     int32_t qp, int32_t gop, int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch,
                                     int64_t scratch_bytes, uint32_t* mbinfo, int32_t segs, void* stream) {
    H264_SEG_COMMON_ARGS(name);
    uint8_t* base = (uint8_t*)scratch;
    const long long chains = (long long)((n + gop - 1) / gop) * mbh * segs;        // the IDR pictures of the call
    hipLaunchKernelGGL(h264_idr4_seg_kernel, dim3((unsigned)chains), dim3(64), 0, (hipStream_t)stream, y, cb, cr, n, mbh, mbw, qp, gop, first_index, ry,
                       rcb, rcr, base, l.stride, l.slot, (int32_t*)(base + l.lens_at), mbinfo, segs);
    SDV_CHECK_LAUNCH(name);
    return SDV_OK;
}

extern "C" int sdv_h264_encode_gop_step_seg(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                            int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                            int64_t mv_count, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                            int32_t segs, void* stream) {
    return h264_encode_gop_step_seg_impl("sdv_h264_encode_gop_step_seg", y, cb, cr, n, mbh, mbw, qp, gop, k, search, subpel, first_index, mv, mv_count,
                                         ry, rcb, rcr, scratch, scratch_bytes, nullptr, segs, stream);
}

extern "C" int sdv_h264_encode_gop_step_seg_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                               int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                               int64_t mv_count, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                               uint32_t* mbinfo, int64_t mbinfo_count, int32_t segs, void* stream) {
    H264_SEG_MBINFO_ARGS("sdv_h264_encode_gop_step_seg_lf");
    return h264_encode_gop_step_seg_impl("sdv_h264_encode_gop_step_seg_lf", y, cb, cr, n, mbh, mbw, qp, gop, k, search, subpel, first_index, mv,
                                         mv_count, ry, rcb, rcr, scratch, scratch_bytes, mbinfo, segs, stream);
}

extern "C" int sdv_h264_encode_idr4_seg(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                        int32_t gop, int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch,
                                        int64_t scratch_bytes, int32_t segs, void* stream) {
    return h264_encode_idr4_seg_impl("sdv_h264_encode_idr4_seg", y, cb, cr, n, mbh, mbw, qp, gop, first_index, ry, rcb, rcr, scratch, scratch_bytes,
                                     nullptr, segs, stream);
}

extern "C" int sdv_h264_encode_idr4_seg_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                           int32_t gop, int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch,
                                           int64_t scratch_bytes, uint32_t* mbinfo, int64_t mbinfo_count, int32_t segs, void* stream) {
    H264_SEG_MBINFO_ARGS("sdv_h264_encode_idr4_seg_lf");
    return h264_encode_idr4_seg_impl("sdv_h264_encode_idr4_seg_lf", y, cb, cr, n, mbh, mbw, qp, gop, first_index, ry, rcb, rcr, scratch, scratch_bytes,
                                     mbinfo, segs, stream);
}
